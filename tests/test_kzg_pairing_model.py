"""The host model of the pairing and of KZG verification (tests/kzg_pairing_model.py) against statements that do not share its route:
the ceremony's [tau] G2 (tests/golden/kzg_trusted_setup_g2.bin, which no model of this tree produced) pairs with the ceremony's G1
points, the four golden proofs of eip4844_proofs_kat.json verify and their tampered twins do not, the pairing is bilinear and of order
r, the final exponentiation is the plain power by 3 (p^12 - 1) / r, and every tower operation agrees with its definition."""
import json
import os
import random

import pytest

from tests import kzg_model as km
from tests import kzg_open_model as om
from tests import kzg_pairing_model as pm

P, R = pm.P, pm.R


@pytest.fixture(scope="module")
def tau_g2():
    return pm.g2_decompress(pm.load_tau_g2_bytes())  # (with the subgroup check: [r] Q = O)


def rand_f2(rng):
    return (rng.randrange(P), rng.randrange(P))


def rand_f12(rng):
    return [rand_f2(rng) for _ in range(6)]


def test_tower_operations_agree_with_their_definitions():
    rng = random.Random(12)
    a, b, c = rand_f12(rng), rand_f12(rng), rand_f12(rng)
    assert pm.f12_mul(a, pm.F12_ONE) == a and pm.f12_mul(a, b) == pm.f12_mul(b, a)
    assert pm.f12_mul(pm.f12_mul(a, b), c) == pm.f12_mul(a, pm.f12_mul(b, c))
    w = [pm.F2_ZERO, pm.F2_ONE] + [pm.F2_ZERO] * 4
    assert pm.f12_pow(w, 6) == [pm.XI] + [pm.F2_ZERO] * 5  # w^6 = xi
    assert pm.f12_mul(a, pm.f12_inv(a)) == pm.F12_ONE
    assert pm.f12_inv([pm.F2_ZERO] * 6) == [pm.F2_ZERO] * 6
    assert pm.f12_frob(a, 1) == pm.f12_pow(a, P)  # the Frobenius maps are powers by p
    assert pm.f12_frob(a, 2) == pm.f12_frob(pm.f12_frob(a, 1), 1)
    assert pm.f12_frob(a, 3) == pm.f12_frob(pm.f12_frob(a, 2), 1)
    assert pm.f12_frob(a, 6) == pm.f12_frob(pm.f12_frob(a, 3), 3) == pm.f12_conj(a)
    l0, l2, l3 = rand_f2(rng), rand_f2(rng), rng.randrange(P)
    assert pm.f12_mul_line(a, l0, l2, l3) == pm.f12_mul(a, [l0, pm.F2_ZERO, l2, (l3, 0), pm.F2_ZERO, pm.F2_ZERO])
    x = rand_f2(rng)
    assert pm.f2_mul(x, pm.f2_inv(x)) == pm.F2_ONE and pm.f2_mul_xi(x) == pm.f2_mul(x, pm.XI)
    roots = 0
    for v in [rand_f2(rng) for _ in range(12)] + [pm.F2_ZERO, pm.F2_ONE, (P - 1, 0), (0, 1), (3, 0), (P - 3, 0)]:
        for sq in (v, pm.f2_sqr(v)):
            s = pm.f2_sqrt(sq)
            if s is not None:
                roots += 1
                assert pm.f2_sqr(s) == sq
            else:
                assert pm.f2_pow(sq, (P * P - 1) // 2) == (P - 1, 0)  # Euler: no root
    assert roots >= 18


def test_g2_fixture_generator_and_compression(tau_g2):
    assert pm.g2_on_twist(tau_g2) and pm.g2_mul(R, tau_g2) is pm.INF
    assert pm.g2_on_twist(pm.G2_GEN) and pm.g2_mul(R, pm.G2_GEN) is pm.INF
    raw = pm.load_tau_g2_bytes()
    assert pm.g2_compress(tau_g2) == raw
    for q in (pm.G2_GEN, pm.g2_neg(pm.G2_GEN), pm.g2_mul(5, pm.G2_GEN), pm.INF):
        assert pm.g2_decompress(pm.g2_compress(q)) == q
    # on the subgroup psi is multiplication by x = -X_ABS (the device's membership test); off it, it is not
    assert pm.g2_psi(tau_g2) == pm.g2_neg(pm.g2_mul(pm.X_ABS, tau_g2))
    outside = pm.outside_g2()
    assert pm.g2_on_twist(outside) and pm.g2_mul(R, outside) is not pm.INF
    assert pm.g2_psi(outside) != pm.g2_neg(pm.g2_mul(pm.X_ABS, outside))
    for bad, why in ((bytes([raw[0] & 0x7F]) + raw[1:], "bit 7"), (bytes([0xC0]) + bytes(94) + b"\x01", "infinity"),
                     (bytes([0x80 | (P >> 376)]) + (P & ((1 << 376) - 1)).to_bytes(47, "big") + bytes(48), ">= p"),
                     (bytes([0x80]) + bytes(47) + P.to_bytes(48, "big"), ">= p"), (pm.no_root_g2(), "no y"), (pm.g2_compress(outside), "subgroup")):
        with pytest.raises(km.BadPoint, match=why):
            pm.g2_decompress(bad)


def test_the_ceremony_points_pair(tau_g2):
    s = km.load_setup()
    assert pm.pairing_product_is_one([(s[1], pm.G2_GEN), (km.neg(s[0]), tau_g2)])  # e([tau] G1, G2) = e(G1, [tau] G2)
    assert not pm.pairing_product_is_one([(s[1], pm.G2_GEN), (km.neg(s[0]), pm.G2_GEN)])
    assert pm.pairing_product_is_one([(s[2], pm.G2_GEN), (km.neg(s[1]), tau_g2)])
    assert s[0] == pm.g1_gen()


def test_pairing_is_bilinear_of_order_r_and_the_final_exponentiation_is_the_plain_power():
    x = pm.X_ABS
    assert 3 * ((P ** 4 - P ** 2 + 1) // R) == (x + 1) ** 2 * (P - x) * (x * x + P * P - 1) + 3 and (P ** 4 - P ** 2 + 1) % R == 0
    assert (P ** 4 - P ** 2 + 1) % 3 == 1 and pm.FINAL_EXP_MULTIPLE == 3
    g1 = pm.g1_gen()
    f = pm.miller_loop([(g1, pm.G2_GEN)])
    e = pm.final_exp(f)
    assert e == pm.f12_pow(f, 3 * (P ** 12 - 1) // R)
    assert e != pm.F12_ONE and pm.f12_pow(e, R) == pm.F12_ONE
    assert pm.pairing(km.mul_naive(6, g1), pm.G2_GEN) == pm.f12_pow(e, 6) == pm.pairing(g1, pm.g2_mul(6, pm.G2_GEN))
    assert pm.pairing(km.mul_naive(2, g1), pm.g2_mul(3, pm.G2_GEN)) == pm.f12_pow(e, 6)
    assert pm.pairing(km.INF, pm.G2_GEN) == pm.F12_ONE == pm.pairing(g1, pm.INF)
    assert pm.pairing_product_is_one([(km.mul_naive(5, g1), pm.G2_GEN), (km.neg(g1), pm.g2_mul(5, pm.G2_GEN))])
    assert not pm.pairing_product_is_one([(km.mul_naive(5, g1), pm.G2_GEN), (km.neg(g1), pm.g2_mul(6, pm.G2_GEN))])


def golden_claims():
    """(name, commitment, z, y, proof) of the four golden proofs: both blobs, opening proof and blob proof"""
    wit = json.load(open(os.path.join(km.GOLDEN, "eip4844_kat.json")))["cases"]
    prf = json.load(open(om.KAT_FILE))["cases"]
    out = []
    for w, p in zip(wit, prf):
        c = km.decompress(bytes.fromhex(w["commitment"]))
        out.append((p["blob"] + "/opening", c, int(w["evaluation_point"], 16), int(w["opening_value"], 16), km.decompress(bytes.fromhex(p["opening_proof"]))))
        out.append((p["blob"] + "/blob", c, int(p["blob_challenge"], 16), int(p["blob_value"], 16), km.decompress(bytes.fromhex(p["blob_proof"]))))
    return out


def test_golden_proofs_verify_and_their_tampered_twins_do_not(tau_g2):
    claims = golden_claims()
    assert len(claims) == 4
    for i, (name, c, z, y, proof) in enumerate(claims):
        other = claims[(i + 2) % 4][1]
        assert other != c
        assert pm.verify_kzg_proof(c, z, y, proof, tau_g2), name
        assert not pm.verify_kzg_proof(c, z, (y + 1) % R, proof, tau_g2), name
        assert not pm.verify_kzg_proof(other, z, y, proof, tau_g2), name
        if name.startswith("zero"):
            # the zero blob is the zero polynomial: C = O, y = 0 and the proof is O, so p(z + 1) = 0 is as true as p(z) = 0, and -O = O
            assert c is km.INF and proof is km.INF and y == 0
            assert pm.verify_kzg_proof(c, (z + 1) % R, y, proof, tau_g2), name
        else:
            assert not pm.verify_kzg_proof(c, (z + 1) % R, y, proof, tau_g2), name
            assert not pm.verify_kzg_proof(c, z, y, km.neg(proof), tau_g2), name


def test_known_tau_setup_verifies_against_the_models_own_tau_g2():
    tau, n = 0x4844, 8
    pts = om.known_tau_setup(tau, n)
    t2 = pm.g2_mul(tau, pm.G2_GEN)
    rng = random.Random(4844)
    coeffs = [rng.randrange(R) for _ in range(n)]
    c = km.decompress(km.commit(coeffs, pts))
    for z in (0, 1, R - 1, rng.randrange(R)):
        y = sum(a * pow(z, k, R) for k, a in enumerate(coeffs)) % R
        proof = km.decompress(om.proof_by_tau(coeffs, z, tau))
        assert pm.verify_kzg_proof(c, z, y, proof, t2)
        assert not pm.verify_kzg_proof(c, z, (y + 1) % R, proof, t2)
        assert not pm.verify_kzg_proof(c, z, y, proof, pm.g2_mul(tau + 1, pm.G2_GEN))
