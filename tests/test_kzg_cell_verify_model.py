"""The host model of the cell-proof verification (tests/kzg_cell_verify_model.py) against statements that do not share its route: the
interpolant by inverse transform equals the remainder of the blob's polynomial modulo X^64 - c_k, the shifts and constants are what the
kernels assume, and the pairing equation separates true claims from false ones and agrees with kzg_pairing_model.verify_kzg_proof on the
claim "(C - [I_k] G1) opens to 0 at c_k under [tau^64] G2". CPU only; a pairing of the model takes about 0.1 s."""
import random

import pytest

from tests import kzg_cell_verify_model as vm
from tests import kzg_cells_model as cm
from tests import kzg_model as km
from tests import kzg_pairing_model as pm

R = km.R
TAU = 0x1234567
KS = (0, 1, 64, 77, 127)


@pytest.fixture(scope="module")
def blob():
    """(coefficients, the 128 cells, C, [tau^64] G2) of a random blob on the setup of TAU"""
    rng = random.Random(7594_36)
    coeffs = [rng.randrange(R) for _ in range(cm.N)]
    return coeffs, cm.cells(coeffs), vm.g1_of(cm.evaluate(coeffs, TAU)), vm.tau64_g2(TAU)[0]


def proof_of(coeffs, k):
    return vm.g1_of(cm.evaluate(cm.quotient_by_cell(coeffs, k), TAU))


def test_constants():
    assert cm.cell_constant(0) == 1 and cm.cell_constant(1) == R - 1
    assert vm.W64 == pow(cm.OMEGA, 64, R) and pow(vm.W64, 64, R) == 1 and pow(vm.W64, 32, R) == R - 1
    for k in range(128):
        h = vm.cell_shift(k)
        assert pow(h, 64, R) == cm.cell_constant(k)
        assert cm.cell_points(k) == [h * pow(vm.W64, cm.brp(t, 6), R) % R for t in range(64)]
        # what k_kzg_cell_interpolate reads from the table of W^m, m < 4096: h_k^-i = W^(8192 - brp7(k) i), W^(4096 + m) = -W^m
        for i in (1, 63):
            down = cm.brp(k, 7) * i
            ex = 8192 - down if down else 0
            want = pow(h, -i, R)
            assert 0 <= ex < 8192 and (pow(cm.W, ex & 4095, R) * (-1 if ex >= 4096 else 1)) % R == want


@pytest.mark.parametrize("k", KS)
def test_the_two_interpolants_agree(blob, k):
    coeffs, cells, _, _ = blob
    got = vm.interpolant(k, cells[k])
    assert got == vm.interpolant_by_remainder(coeffs, k)
    for t, x in enumerate(cm.cell_points(k)[:4]):  # and it does interpolate
        assert cm.evaluate(got, x) == vm.cell_elements(cells[k])[t]
    # p = q_k (X^64 - c_k) + I_k at tau
    q = cm.evaluate(cm.quotient_by_cell(coeffs, k), TAU)
    assert (q * (pow(TAU, 64, R) - cm.cell_constant(k)) + cm.evaluate(got, TAU)) % R == cm.evaluate(coeffs, TAU)


def test_the_interpolant_commitment_over_points_is_the_one_by_tau(blob):
    from tests import kzg_open_model as om

    _, cells, _, _ = blob
    points = om.known_tau_setup(TAU, 64)
    assert vm.interpolant_commitment(77, cells[77], points=points) == vm.interpolant_commitment(77, cells[77], tau=TAU)


def test_true_false_and_swapped_claims_through_the_pairing(blob):
    coeffs, cells, c, t64 = blob
    p77, p5 = proof_of(coeffs, 77), proof_of(coeffs, 5)
    assert vm.verify_cell(c, 77, cells[77], p77, t64, tau=TAU)
    assert vm.verify_cell(c, 0, cells[0], proof_of(coeffs, 0), t64, tau=TAU)
    tampered = bytearray(cells[77])
    tampered[32 * 9 + 31] ^= 1
    assert not vm.verify_cell(c, 77, bytes(tampered), p77, t64, tau=TAU)
    assert not vm.verify_cell(c, 77, cells[77], p5, t64, tau=TAU)  # the proof of another cell
    assert not vm.verify_cell(c, 5, cells[77], p77, t64, tau=TAU)  # the right cell and proof under another index
    assert not vm.verify_cell(c, 77, cells[77], p77, pm.g2_mul(TAU, pm.G2_GEN), tau=TAU)  # [tau] G2 in place of [tau^64] G2


def test_the_claim_is_an_opening_of_c_minus_i_at_c_k(blob):
    coeffs, cells, c, t64 = blob
    for k, proof in ((77, proof_of(coeffs, 77)), (77, proof_of(coeffs, 5))):
        reduced = km.add(c, km.neg(vm.interpolant_commitment(k, cells[k], tau=TAU)))
        assert pm.verify_kzg_proof(reduced, cm.cell_constant(k), 0, proof, t64) == vm.verify_cell(c, k, cells[k], proof, t64, tau=TAU)
