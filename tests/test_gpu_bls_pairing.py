"""GPU: era_zkevm_test_harness_amd/csrc/bls12_381_pairing.cuh alone — the tower Fq2 / Fq12 over groups of 8 lanes, G2 decompression and
the prepared lines, the final exponentiation and the pairing — exactly equal to Python integers (tests/kzg_pairing_model.py).
tests/csrc_gpu/bls_pairing_test.hip is built with hipcc on the box, reads the cases this file writes and returns a result per case."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import kzg_model as km
from tests import kzg_pairing_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
P, R = pm.P, pm.R

(FQ2_MUL, FQ2_SQR, FQ2_INV, FQ2_SQRT) = range(4)
(G2_DECOMPRESS, G2_PREPARE) = (10, 11)
(F12_MUL, F12_SQR, F12_INV, F12_MUL_LINE, F12_CONJ, F12_FROB1, F12_FROB2, F12_FINAL_EXP, F12_PAIRING) = range(100, 109)
CASE = np.dtype([("op", "<u4"), ("in", "<u4", (288,))])
RESULT = np.dtype([("flag", "<u4"), ("out", "<u4", (144,))])
SPECIAL = [0, 1, P - 1, (1 << 384) % P, ((1 << 384) - 1) % P, ((1 << 352) - 1)]  # 0, 1, p - 1, R mod p, all-ones words


def words(v, n=12):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def value(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def w2(a):
    return words(a[0]) + words(a[1])


def w12(a):
    return [x for c in a for x in w2(c)]


def v2(w):
    return (value(w[:12]), value(w[12:24]))


def v12(w):
    return [v2(w[24 * k:24 * k + 24]) for k in range(6)]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("blsp")
    exe = str(d / "bls_pairing_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tests", "csrc_gpu", "bls_pairing_test.hip"), "-o", exe])

    def go(cases):
        cases = sorted(cases, key=lambda c: c[0])  # the program launches each run of equal operations on its own
        arr = np.zeros(len(cases), CASE)
        for i, (op, ins) in enumerate(cases):
            arr[i]["op"] = op
            arr[i]["in"][:len(ins)] = ins
        arr.tofile(str(d / "cases.bin"))
        r = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith(f"ok {len(cases)}"), r.stdout[-2000:] + r.stderr[-2000:]
        return cases, np.fromfile(str(d / "results.bin"), RESULT)

    return go


def test_fq2_operations_equal_python_integers(run):
    rng = random.Random(2)
    vals = [(a, b) for a in SPECIAL for b in SPECIAL] + [(rng.randrange(P), rng.randrange(P)) for _ in range(24)]
    cases, want = [], {}
    for a in vals:
        for b in rng.sample(vals, 6):
            cases.append((FQ2_MUL, w2(a) + w2(b)))
        cases += [(FQ2_SQR, w2(a)), (FQ2_INV, w2(a)), (FQ2_SQRT, w2(a)), (FQ2_SQRT, w2(pm.f2_sqr(a)))]
    cases, res = run(cases)
    roots = 0
    for (op, ins), r in zip(cases, res):
        a, b = v2(ins[:24]), v2(ins[24:48])
        got = v2(r["out"][:24])
        if op == FQ2_MUL:
            assert got == pm.f2_mul(a, b), (a, b)
        elif op == FQ2_SQR:
            assert got == pm.f2_sqr(a), a
        elif op == FQ2_INV:
            assert got == pm.f2_inv(a), a
        else:
            s = pm.f2_sqrt(a)
            assert bool(r["flag"]) == (s is not None), a
            if s is not None:
                roots += 1
                assert got == s, a  # the same root: the model walks the same algorithm
    assert roots >= len(vals)


def f12_operands(rng):
    """random elements, elements of special coefficients, and elements with a single nonzero coefficient at each k (a mis-routed xi wrap
    shows on those)"""
    out = [[(rng.randrange(P), rng.randrange(P)) for _ in range(6)] for _ in range(4)]
    out += [[(rng.choice(SPECIAL), rng.choice(SPECIAL)) for _ in range(6)] for _ in range(4)]
    for k in range(6):
        for c in ((1, 0), (0, 1), (rng.randrange(P), rng.randrange(P))):
            out.append([c if j == k else pm.F2_ZERO for j in range(6)])
    return out + [[pm.F2_ZERO] * 6, pm.F12_ONE]


def test_fq12_operations_equal_python_integers(run):
    rng = random.Random(12)
    ops = f12_operands(rng)
    cases = []
    for i, a in enumerate(ops):
        for b in [ops[(i + 1) % len(ops)]] + rng.sample(ops, 3) + [ops[8 + 3 * k] for k in range(6)]:
            cases.append((F12_MUL, w12(a) + w12(b)))
        l0, l2, l3 = rng.choice(ops)[0], rng.choice(ops)[1], rng.choice(SPECIAL + [rng.randrange(P)])
        cases.append((F12_MUL_LINE, w12(a) + w12([l0, pm.F2_ZERO, l2, (l3, 0), pm.F2_ZERO, pm.F2_ZERO])))
        cases += [(op, w12(a)) for op in (F12_SQR, F12_INV, F12_CONJ, F12_FROB1, F12_FROB2)]
    cases, res = run(cases)
    for (op, ins), r in zip(cases, res):
        a, b = v12(ins[:144]), v12(ins[144:])
        want = {F12_MUL: lambda: pm.f12_mul(a, b), F12_SQR: lambda: pm.f12_sqr(a), F12_INV: lambda: pm.f12_inv(a), F12_CONJ: lambda: pm.f12_frob(a, 6),
                F12_FROB1: lambda: pm.f12_frob(a, 1), F12_FROB2: lambda: pm.f12_frob(a, 2),
                F12_MUL_LINE: lambda: pm.f12_mul_line(a, b[0], b[2], b[3][0])}[op]()
        assert v12(r["out"]) == want, (op, a, b)
        assert bool(r["flag"]) == (want == pm.F12_ONE)


def test_g2_decompression_and_prepared_lines(run):
    tau_raw = pm.load_tau_g2_bytes()
    pts = [pm.g2_decompress(tau_raw)] + [pm.g2_mul(k, pm.G2_GEN) for k in (1, 2, 5, R - 1)]
    enc = [pm.g2_compress(q) for q in pts] + [pm.g2_compress(pm.INF)]
    assert enc[0] == tau_raw
    outside = pm.outside_g2()
    bad = [bytes([tau_raw[0] & 0x7F]) + tau_raw[1:], bytes([0xC0]) + bytes(94) + b"\x01",
           bytes([0x80 | (P >> 376)]) + (P & ((1 << 376) - 1)).to_bytes(47, "big") + bytes(48), bytes([0x80]) + bytes(47) + P.to_bytes(48, "big"), pm.no_root_g2()]
    dec = enc + bad + [pm.g2_compress(outside)]
    want_code = [0] * len(enc) + [1, 2, 3, 3, 4] + [0]  # (the subgroup check is g2_prepare's)
    cases = [(G2_DECOMPRESS, list(np.frombuffer(b, "<u4"))) for b in dec]
    cases += [(G2_PREPARE, w2(q[0]) + w2(q[1])) for q in pts + [outside]]
    cases, res = run(cases)
    for (op, ins), r, code, q in zip(cases[:len(dec)], res, want_code, pts + [pm.INF] + [None] * len(bad) + [outside]):
        assert int(r["flag"]) == code, bytes(np.array(ins[:24], "<u4").tobytes()).hex()
        if code == 0:
            got = (v2(r["out"][:24]), v2(r["out"][24:48]))
            assert got == (q if q is not pm.INF else (pm.F2_ZERO, pm.F2_ZERO))
    for (op, ins), r, q in zip(cases[len(dec):], res[len(dec):], pts + [outside]):
        assert bool(r["flag"]) == (q is not outside)
        lines, _ = pm.g2_lines(q)
        assert len(lines) == 68
        assert [v2(r["out"][24 * j:24 * j + 24]) for j in range(4)] == [lines[0][0], lines[0][1], lines[-1][0], lines[-1][1]]


def _aff(p):
    return [0] * 24 if p is km.INF else words(p[0]) + words(p[1])


def _pair_case(p0, q0, p1, q1):
    return (F12_PAIRING, _aff(p0) + _aff(p1) + w2(q0[0]) + w2(q0[1]) + w2(q1[0]) + w2(q1[1]))


def test_final_exponentiation_pairing_and_product_checks(run):
    rng = random.Random(381)
    g1, g2 = pm.g1_gen(), pm.G2_GEN
    O = km.INF
    fs = [pm.miller_loop([(g1, g2)]), [(rng.randrange(P), rng.randrange(P)) for _ in range(6)], pm.F12_ONE,
          [(rng.randrange(1, P), 0)] + [pm.F2_ZERO] * 5]
    cases = [(F12_FINAL_EXP, w12(f)) for f in fs]
    want = [pm.final_exp(f) for f in fs]
    assert want[2] == pm.F12_ONE == want[3]  # (an element of Fq goes to one)
    ab = [(1, 1), (2, 3), (rng.randrange(1, R), rng.randrange(1, R)), (R - 1, 7)]
    for a, b in ab:  # the full pairing: the second pair's P is infinity and contributes the factor 1
        p, q = km.mul_naive(a, g1), pm.g2_mul(b, g2)
        cases.append(_pair_case(p, q, O, g2))
        want.append(pm.pairing(p, q))
    a = rng.randrange(2, R)
    pt, q = km.mul_naive(rng.randrange(1, R), g1), pm.g2_mul(rng.randrange(1, R), g2)
    products = [((km.mul_naive(a, pt), q), (km.neg(pt), pm.g2_mul(a, q)), True),          # e(aP, Q) e(-P, aQ) = 1
                ((km.mul_naive(a, pt), q), (km.neg(pt), pm.g2_mul(a + 1, q)), False),
                ((O, q), (O, g2), True), ((O, q), (pt, g2), False)]
    for (p0, q0), (p1, q1), _ in products:
        cases.append(_pair_case(p0, q0, p1, q1))
        want.append(pm.final_exp(pm.miller_loop([(p0, q0), (p1, q1)])))
    assert [w == pm.F12_ONE for w in want[8:]] == [t for _, _, t in products]
    order = sorted(range(len(cases)), key=lambda i: cases[i][0])  # (run() sorts by operation; stable)
    _, res = run(cases)
    for i, r in zip(order, res):
        assert v12(r["out"]) == want[i], i
        assert bool(r["flag"]) == (want[i] == pm.F12_ONE), i
    e = want[4]
    assert want[5] == pm.f12_pow(e, 6)  # bilinear: e(2 G1, 3 G2) = e(G1, G2)^6
