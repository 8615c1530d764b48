"""GPU: era_zkevm_test_harness_amd/csrc/bls12_381.cuh alone — the fields Fq and Fr (Montgomery products on v_mad_u64_u32, add, subtract,
inversion, Fq's square root) and the group G1 of BLS12-381 — against Python integers (tests/kzg_model.py for the group law).
tests/csrc_gpu/bls_field_test.hip is built with hipcc on the box, reads the cases this file writes and returns a result per case."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import kzg_model as km

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

(FQ_MUL, FQ_ADD, FQ_SUB, FQ_INV, FQ_SQRT, FQ_RAW_MUL, FQ_NEG) = range(7)
(FR_MUL, FR_ADD, FR_SUB, FR_INV) = range(10, 14)
FR_RAW_MUL = 15
(G1_DBL, G1_MADD, G1_ADD, G1_IN_SUBGROUP, G1_COMPRESS, G1_DECOMPRESS) = range(20, 26)
CASE = np.dtype([("op", "<u4"), ("in", "<u4", (72,))])
RESULT = np.dtype([("flag", "<u4"), ("out", "<u4", (24,))])
G = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
     0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)


def words(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def value(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def field_values(p, n_words, rng):
    """0, 1, 2, p - 1, p - 2, R mod p, values with all-ones words, and random ones"""
    top = (1 << (32 * n_words)) - 1
    ones = [top % p, (top >> 32) % p, ((1 << 64) - 1) << 32, (1 << (32 * (n_words - 1))) - 1, p - ((1 << 96) - 1), 0xFFFFFFFF]
    return [0, 1, 2, p - 1, p - 2, (1 << (32 * n_words)) % p] + ones + [rng.randrange(p) for _ in range(6)]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("bls")
    exe = str(d / "bls_field_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tests", "csrc_gpu", "bls_field_test.hip"), "-o", exe])

    def go(cases):
        arr = np.zeros(len(cases), CASE)
        for i, (op, ins) in enumerate(cases):
            arr[i]["op"] = op
            arr[i]["in"][:len(ins)] = ins
        arr.tofile(str(d / "cases.bin"))
        r = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith(f"ok {len(cases)}"), r.stdout[-2000:] + r.stderr[-2000:]
        return np.fromfile(str(d / "results.bin"), RESULT)

    return go


@pytest.mark.parametrize("name", ["fq", "fr"])
def test_field_operations_equal_python_integers(run, name):
    p, n, ops = (km.P, 12, (FQ_MUL, FQ_ADD, FQ_SUB, FQ_INV, FQ_RAW_MUL)) if name == "fq" else (km.R, 8, (FR_MUL, FR_ADD, FR_SUB, FR_INV, FR_RAW_MUL))
    mul, add, sub, inv, raw = ops
    rng = random.Random(381 + n)
    vals = field_values(p, n, rng)
    pairs = [(a, b) for a in vals for b in vals] + [(rng.randrange(p), rng.randrange(p)) for _ in range(256)]
    r_inv = pow(1 << (32 * n), -1, p)
    # the Montgomery product proper, a b R^-1: pairs whose last step subtracts p and pairs where it does not (both occur among these)
    below = sum(1 for a, b in pairs if ((a * b + ((-a * b * pow(p, -1, 1 << (32 * n))) % (1 << (32 * n))) * p) >> (32 * n)) < p)
    assert 0 < below < len(pairs)
    cases, want = [], []
    for a, b in pairs:
        for op, w in ((mul, a * b % p), (add, (a + b) % p), (sub, (a - b) % p), (raw, a * b * r_inv % p)):
            cases.append((op, words(a, 12) + words(b, 12)))
            want.append(w)
    for a in vals + [rng.randrange(p) for _ in range(32)]:
        cases.append((inv, words(a, 12)))
        want.append(pow(a, p - 2, p))
    res = run(cases)
    for (op, ins), w, r in zip(cases, want, res):
        assert value(r["out"][:n]) == w, (name, op, hex(value(ins[:12])), hex(value(ins[12:24])))


def test_fq_square_root_and_negation(run):
    rng = random.Random(4)
    vals = field_values(km.P, 12, rng) + [rng.randrange(km.P) for _ in range(64)]
    vals += [v * v % km.P for v in vals[:20]]
    res = run([(FQ_SQRT, words(a, 12)) for a in vals] + [(FQ_NEG, words(a, 12)) for a in vals])
    roots = 0
    for a, r in zip(vals, res[:len(vals)]):
        s = km.sqrt_fq(a)
        assert bool(r["flag"]) == (s is not None), hex(a)
        if s is not None:
            roots += 1
            assert value(r["out"][:12]) in (s, (km.P - s) % km.P)
    assert 20 <= roots < len(vals)
    for a, r in zip(vals, res[len(vals):]):
        assert value(r["out"][:12]) == (-a) % km.P


def _aff(pt):
    return [0] * 24 if pt is km.INF else words(pt[0], 12) + words(pt[1], 12)


def _point(r):
    x, y = value(r["out"][:12]), value(r["out"][12:])
    return km.INF if x == 0 and y == 0 else (x, y)


def test_group_law_is_complete(run):
    rng = random.Random(12)
    A, B = km.mul_naive(rng.randrange(1, km.R), G), km.mul_naive(rng.randrange(1, km.R), G)
    O = km.INF
    l1, l2 = rng.randrange(2, km.P), rng.randrange(2, km.P)

    def case(op, p, q=O, la=1, lb=1):
        return (op, _aff(p) + _aff(q) + words(la, 12) + words(lb, 12))

    cases, want = [], []
    for p, q in ((A, B), (B, A), (A, A), (A, km.neg(A)), (O, A), (A, O), (O, O), (G, G), (G, km.neg(G))):
        for la, lb in ((1, 1), (l1, l2)):  # Z = 1 and Z != 1 (equal points in different Jacobian coordinates still route to doubling)
            cases += [case(G1_MADD, p, q, la), case(G1_ADD, p, q, la, lb)]
            want += [km.add(p, q)] * 2
    for p in (A, B, G, O):
        for la in (1, l1):
            cases.append(case(G1_DBL, p, O, la))
            want.append(km.add(p, p))
    res = run(cases)
    for c, w, r in zip(cases, want, res):
        assert _point(r) == w, c[0]
    assert km.add(A, A) is not O and km.add(A, km.neg(A)) is O


def test_subgroup_check_compression_and_decompression(run):
    rng = random.Random(7)
    A = km.mul_naive(rng.randrange(1, km.R), G)
    # an on-curve point outside the order-r subgroup: the smallest x >= 1 with a root whose point r does not kill
    x = 1
    while True:
        y = km.sqrt_fq((x ** 3 + km.B) % km.P)
        if y is not None and km.mul_naive(km.R, (x, y)) is not km.INF:
            break
        x += 1
    outside = (x, y)
    pts = [G, A, km.neg(A), km.INF]
    enc = [km.compress(p) for p in pts]
    bad_bit7 = bytes([enc[0][0] & 0x7F]) + enc[0][1:]
    bad_inf = bytes([0xC0]) + bytes(46) + b"\x01"
    bad_x = bytes([0x80 | (km.P >> 376)]) + (km.P & ((1 << 376) - 1)).to_bytes(47, "big")
    xr = 1
    while km.sqrt_fq((xr ** 3 + km.B) % km.P) is not None:
        xr += 1
    no_root = bytes([0x80]) + xr.to_bytes(47, "big")
    dec_in = enc + [bad_bit7, bad_inf, bad_x, no_root, km.compress(outside)]
    dec_want = [0, 0, 0, 0, 1, 2, 3, 4, 0]  # (the subgroup check is a function of its own: in_subgroup)
    cases = [(G1_IN_SUBGROUP, _aff(p)) for p in (G, A, outside)] + [(G1_COMPRESS, _aff(p)) for p in pts + [outside]]
    cases += [(G1_DECOMPRESS, list(np.frombuffer(b, "<u4"))) for b in dec_in]
    res = run(cases)
    assert [int(r["flag"]) for r in res[:3]] == [1, 1, 0]  # the generator times r is O; so is any multiple's; not the outsider's
    for p, r in zip(pts + [outside], res[3:8]):
        assert r["out"][:12].tobytes() == km.compress(p)
    for b, w, r, p in zip(dec_in, dec_want, res[8:], pts + [None] * 4 + [outside]):
        assert int(r["flag"]) == w, b.hex()
        if w == 0:
            assert _point(r) == p
