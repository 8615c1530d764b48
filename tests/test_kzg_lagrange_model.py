"""The host model of the Lagrange-basis setup (tests/kzg_lagrange_model.py) against definitions that use none of its shortcuts, and the
committed fixture tests/golden/kzg_trusted_setup_g1_lagrange.bin (the ceremony's `lagrange_setup_brp`) against the ceremony's monomial
points by three sums that use nothing of a transform. No GPU."""
import hashlib
import os

import pytest

from tests import kzg_lagrange_model as lm
from tests import kzg_model as km
from tests import kzg_open_model as om

R = km.R
TAU = 0x4844
FIXTURE = os.path.join(km.GOLDEN, "kzg_trusted_setup_g1_lagrange.bin")
SHA256 = "000be46bb434946e041c7bc9757175591eb07bcdaff641ea6eca2552618dc39d"


@pytest.mark.parametrize("n", [8, 256, 4096])
def test_closed_form_is_the_inverse_transform_of_the_powers_and_sums_to_one(n):
    sc = lm.lagrange_scalars(TAU, n)
    powers = [pow(TAU, k, R) for k in range(n)]
    assert sc == lm.inverse_transform(powers)
    assert sum(sc) % R == 1
    assert lm.forward_transform(sc) == powers


def test_inverse_transform_is_the_definition():
    n, w = 8, lm.root(8)
    v = [(k * k * 0x1234567 + 5) % R for k in range(n)]
    n_inv, w_inv = pow(n, -1, R), pow(w, -1, R)
    assert lm.inverse_transform(v) == [n_inv * sum(pow(w_inv, j * k, R) * v[k] for k in range(n)) % R for j in range(n)]
    assert lm.forward_transform(v) == [sum(pow(w, j * k, R) * v[k] for k in range(n)) % R for j in range(n)]


@pytest.mark.parametrize("n", [8, 256])
def test_tau_on_the_domain(n):
    w = lm.root(n)
    sc = lm.lagrange_scalars(pow(w, 5, R), n)
    assert sc == [1 if j == 5 else 0 for j in range(n)]
    assert sc == lm.inverse_transform([pow(w, 5 * k, R) for k in range(n)])


def test_fixed_base_products_are_mul_naive():
    g = km.decompress(km.load_setup_bytes()[:48], check_subgroup=False)
    for k in (0, 1, 2, 255, 256, R - 1, R, 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF % R):
        assert km.to_affine(lm.generator_times(k)) == km.mul_naive(k % R, g), hex(k)


@pytest.mark.parametrize("n", [8, 16])
def test_lagrange_points_against_msm_naive(n):
    """L[u] = (1 / n) sum_k w^(-u k) S[k] by msm_naive over S[k] = [tau^k] G1, entry i of the handle = L[brp(i)]; and the identities
    sum_u L[u] = S[0], sum_u w^u L[u] = S[1]"""
    bits = n.bit_length() - 1
    setup = om.known_tau_setup(TAU, n)
    got = lm.lagrange_setup_brp(TAU, n)
    n_inv, w_inv = pow(n, -1, R), pow(lm.root(n), -1, R)
    for i in range(n):
        u = lm.brp(i, bits)
        want = km.msm_naive([n_inv * pow(w_inv, u * k, R) % R for k in range(n)], setup)
        assert got[48 * i:48 * i + 48] == km.compress(want), i
    lag = [km.decompress(got[48 * i:48 * i + 48], check_subgroup=False) for i in range(n)]
    assert km.msm_naive([1] * n, lag) == setup[0]
    assert km.msm_naive([pow(lm.root(n), lm.brp(i, bits), R) for i in range(n)], lag) == setup[1]


def test_fixture_digest():
    raw = open(FIXTURE, "rb").read()
    assert len(raw) == 4096 * 48
    assert hashlib.sha256(raw).hexdigest() == SHA256
    assert raw[:6].hex() == "a0413c0dcafe" and raw[44:48].hex() == "88c03654"
    assert raw[48:54].hex() == "837567ad073e" and raw[92:96].hex() == "d9cf79ee"
    assert raw[-48:-42].hex() == "825a6f586726" and raw[-4:].hex() == "81d7beb1"


def test_fixture_sums_give_back_monomial_points():
    """sum_u w^(k u) L[u] = S[k] for k = 0, 1 and 4095 (the forward transform's rows, one at a time by a bucket sum: no transform)"""
    raw = open(FIXTURE, "rb").read()
    setup = km.load_setup()
    w = lm.root(4096)
    lag = [km.decompress(raw[48 * i:48 * i + 48], check_subgroup=False) for i in range(4096)]  # entry i = L[brp12(i)]
    us = [lm.brp(i, 12) for i in range(4096)]
    for k in (0, 1, 4095):
        assert km.msm([pow(w, k * u, R) for u in us], lag) == setup[k], k
