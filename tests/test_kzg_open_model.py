"""The host model of the KZG proofs (tests/kzg_open_model.py) checked on its own, without a GPU, against statements that do not share its
route: the quotient multiplies back to the polynomial; on a setup whose tau is known the proof is [(p(tau) - y) / (tau - z)] G1 by one
double-and-add, for points off and ON the evaluation domain; evaluation-form elements equal direct evaluations; the challenge equals a
preimage put together by hand; and the model reproduces tests/golden/eip4844_proofs_kat.json."""
import hashlib
import json
import random

import pytest

from tests import kzg_model as km
from tests import kzg_open_model as om

TAU = 0x4844


def horner(coeffs, x):
    v = 0
    for a in reversed(coeffs):
        v = (v * x + a) % om.R
    return v


def test_omega_is_a_primitive_4096th_root_of_unity():
    assert om.OMEGA == pow(7, (om.R - 1) // 4096, om.R)
    assert pow(om.OMEGA, 4096, om.R) == 1 and pow(om.OMEGA, 2048, om.R) == om.R - 1
    assert [om.brp12(i) for i in (0, 1, 2, 3, 4095)] == [0, 2048, 1024, 3072, 4095]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 257])
def test_quotient_times_x_minus_z_plus_y_is_the_polynomial(n):
    rng = random.Random(n)
    p = [rng.randrange(om.R) for _ in range(n)]
    for z in (0, 1, om.R - 1, pow(om.OMEGA, 5, om.R), rng.randrange(1 << 128)):
        q, y = om.quotient(p, z)
        assert len(q) == max(n - 1, 0) and y == horner(p, z)
        back = [0] * max(n, 1)  # q(X) (X - z) + y
        for k, c in enumerate(q):
            back[k + 1] = (back[k + 1] + c) % om.R
            back[k] = (back[k] - c * z) % om.R
        back[0] = (back[0] + y) % om.R
        assert back[:n] == p and not any(back[n:])


@pytest.fixture(scope="module")
def tau_setup():
    return om.known_tau_setup(TAU, 4096)


@pytest.mark.parametrize("n", [3, 64, 4096])
def test_proof_on_a_known_tau_setup_is_one_scalar_multiplication(tau_setup, n):
    rng = random.Random(100 + n)
    p = [rng.randrange(om.R) for _ in range(n)]
    g = tau_setup[0]
    assert tau_setup[1] == km.mul_naive(TAU, g) and tau_setup[n - 1] == km.mul_naive(pow(TAU, n - 1, om.R), g)
    points = (rng.randrange(1 << 127, 1 << 128), 0, pow(om.OMEGA, 5, om.R))
    for z in points if n < 4096 else points[2:]:  # (a 4 095-term model commitment takes over a second)
        proof, y = om.open(p, z, tau_setup)
        k = (horner(p, TAU) - y) * pow((TAU - z) % om.R, om.R - 2, om.R) % om.R
        assert proof == km.compress(km.mul_naive(k, g)) == om.proof_by_tau(p, z, TAU)


def test_proofs_of_short_and_vanishing_polynomials(tau_setup):
    inf = km.compress(km.INF)
    assert om.open([], 5, tau_setup) == (inf, 0) and om.open([7], 5, tau_setup) == (inf, 7) and om.open([0] * 9, 5, tau_setup) == (inf, 0)
    s, z = [3, 1, 4, 1, 5], 92653
    p = [0] * 6  # (X - z) s(X)
    for k, c in enumerate(s):
        p[k + 1] = (p[k + 1] + c) % om.R
        p[k] = (p[k] - c * z) % om.R
    assert om.open(p, z, tau_setup) == (km.commit(s, tau_setup), 0)


def test_evaluation_form_is_the_direct_evaluation_at_the_bit_reversed_roots():
    blob = random.Random(7).randbytes(km.BLOB_BYTES)
    evals = om.blob_evaluations(blob)
    coeffs = om.blob_coefficients(blob)
    assert len(evals) == 131072 and coeffs[0] == km.blob_elements(blob)[4095]
    for i in (0, 1, 2, 5, 2047, 2048, 4095):
        assert int.from_bytes(evals[32 * i:32 * i + 32], "big") == horner(coeffs, pow(om.OMEGA, om.brp12(i), om.R)), i


def test_challenge_is_the_hash_of_the_preimage_put_together_by_hand():
    rng = random.Random(9)
    evals, commitment = rng.randbytes(131072), rng.randbytes(48)
    pre = bytearray(131152)
    pre[0:16] = b"FSBLOBVERIFY_V1_"
    pre[30], pre[31] = 0x10, 0x00  # 4096 in 16 big-endian bytes
    pre[32:32 + 131072] = evals
    pre[131104:] = commitment
    d = int.from_bytes(hashlib.sha256(bytes(pre)).digest(), "big")
    while d >= om.R:  # at most two subtractions
        d -= om.R
    assert om.blob_challenge(evals, commitment) == d
    assert (len(pre) + 9 + 63) // 64 == 2050  # SHA-256 compressions


@pytest.mark.parametrize("case", [0, 1])
def test_model_reproduces_the_golden_proofs(case):
    kat = json.load(open(om.KAT_FILE))["cases"][case]
    blob, record = om.kat_blobs()[case]
    got = om.kat_case(blob, record)
    for field, value in got.items():
        assert value == kat[field], field
    if case == 0:  # the zero polynomial: both proofs are the point at infinity, both values zero
        assert kat["opening_proof"] == kat["blob_proof"] == km.compress(km.INF).hex() and int(kat["blob_value"], 16) == 0
