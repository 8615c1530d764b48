"""The secp256k1 base-field arithmetic of the ECRecover accumulator chain (era_zkevm_test_harness_amd/csrc/ec_field.cuh), function by function:
the form with a value in one lane (ecf) and the form with a limb per lane, DPP row shifts and ballot carry-lookahead (ecl) — mul / add / sub of
both, ecl::pow_sqrt, Jacobian doubling and mixed addition of both — against plain Python integers. tests/csrc_gpu/ec_field_test.hip builds the
inputs (the 174 x 174 cross product of edge and seeded values, directed pairs for the branches no random pair takes, curve points with Z != 1
written here from secp256k1.py), classifies every input with a host word model of the device steps ("cover" lines: which branch, which carry)
and writes inputs and results to a file; the comparison with `% p`, with secp256k1.py's affine addition and the check that lanes 8..15 of every
ecl result hold zero are made here. The CPU test runs the program with --host-only (inputs, coverage, the model's results against Python
integers, no HIP call); the GPU test runs it whole: one launch of one wave, the device results equal to the model's and to Python's."""
import os
import subprocess

import numpy as np
import pytest

from era_zkevm_test_harness_amd import secp256k1 as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
P = ec.P
DIRECTED = 10  # pairs aimed at a branch each, beyond the cross product (ec_field_test.hip main)
U256 = (np.uint8, 32)
RECORD = np.dtype([("v", U256, 5), ("kind", "<u4"), ("pad0", "<u4", 7),
                   ("mul_l", U256), ("add_l", U256), ("sub_l", U256), ("mul_f", U256), ("add_f", U256), ("sub_f", U256),
                   ("jd_l", U256, 3), ("jd_f", U256, 3), ("ja_l", U256, 3), ("ja_f", U256, 3), ("sqrt_l", U256), ("high", "<u4"), ("pad1", "<u4", 7)])
# the conditions on the inputs: every outcome of every branch and carry seen (a bit per outcome; ec_field_test.hip model::init_cover)
COVER = {"ecl_mul": {"top": 3, "co": 3, "ripple": 3, "canon": 3, "canon_ripple": 3},
         "ecl_add": {"sum": 7, "ripple6": 3},
         "ecl_sub": {"borrow": 3, "through_equal": 3, "lane0_977": 3, "stage2_through": 3, "stage2_borrow_out": "unreachable"},
         "ecf_mul": {"R_hi": 3, "c2": 3, "cond_sub": 7},
         "ecf_add": {"cond_sub": 7},
         "ecf_sub": {"outcome": 7}}


def _int(a):
    return int.from_bytes(a.tobytes(), "little")


def _jac(p, l):
    """the Jacobian form (x l^2, y l^3, l) of an affine point"""
    return p[0] * l * l % P, p[1] * l * l * l % P, l


def _affine(x, y, z):
    zi = pow(z, -1, P)
    return x * zi * zi % P, y * zi * zi * zi % P


def _point_cases():
    """(X, Y, Z, x2, y2, the affine P, the affine Q): P = k G in Jacobian form with Z = l != 1, Q affine; the last two of every l are the degenerate
    inputs of the mixed addition: Q = P and Q = -P"""
    cases = []
    ls = [2, P - 1, 0xFFFFFFFF << 224, 0x1234567 + (0xFFFFFFFFFFFFFFFF << 96), pow(7, 1000, P)]
    for n, l in enumerate(ls):
        pt = ec.mul(0xC0FFEE + 977 * n, ec.G)
        for q in (ec.G, ec.mul(3 + n, pt), ec.neg(ec.mul(2, pt)), pt, ec.neg(pt)):
            cases.append(_jac(pt, l) + q + (pt, q))
    return cases


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ec_field") / "ec_field_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc_gpu", "ec_field_test.hip"), "-o", out])
    return out


def _run(exe, tmp_path, *flags):
    points = _point_cases()
    with open(tmp_path / "points.bin", "wb") as f:
        for c in points:
            f.write(b"".join(int(x).to_bytes(32, "little") for x in c[:5]))
    r = subprocess.run([exe, *flags, "--points", str(tmp_path / "points.bin"), "--out", str(tmp_path / "results.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout, np.fromfile(tmp_path / "results.bin", RECORD), points


def _assert_coverage(stdout, n):
    """one cover line per operation, every case counted, no outcome missing"""
    ops = {}
    for line in stdout.splitlines():
        w = line.split()
        if w and w[0] == "cover":
            assert "MISSING" not in w, line
            assert w[2] == "n" and int(w[3]) == n, line
            ops[w[1]] = {k: v if v == "unreachable" else int(v, 16) for k, v in zip(w[4::2], w[5::2])}
    assert ops == COVER


def _assert_equals_python_integers(rec, points):
    """every result of the file against Python integers; returns the number of cases"""
    n_pairs = rec.size - len(points)
    assert n_pairs >= 174 * 174 + DIRECTED
    assert not rec["high"].any(), np.flatnonzero(rec["high"])[:8]  # lanes 8..15 of every ecl result: zero
    n_sqrt = 0
    for i, q in enumerate(rec):
        a, b = _int(q["v"][0]), _int(q["v"][1])
        assert a < P and b < P
        got = [_int(q[k]) for k in ("mul_l", "mul_f", "add_l", "add_f", "sub_l", "sub_f")]
        assert got == [a * b % P] * 2 + [(a + b) % P] * 2 + [(a - b) % P] * 2, (i, hex(a), hex(b))
        assert int(q["kind"]) & 1 == (i >= n_pairs)
        if int(q["kind"]) & 2:
            n_sqrt += 1
            y = _int(q["sqrt_l"])
            assert y == pow(a, (P + 1) // 4, P), (i, hex(a))
            assert y * y % P == (a if pow(a, (P - 1) // 2, P) <= 1 else P - a)  # the root of a residue; of -a for a non-residue (p = 3 mod 4)
        for k in range(3):  # the two forms of the point formulas, on curve points and on arbitrary values alike
            assert q["jd_l"][k].tobytes() == q["jd_f"][k].tobytes() and q["ja_l"][k].tobytes() == q["ja_f"][k].tobytes(), i
    assert n_sqrt >= (174 * 174 + 36) // 37 + 5
    sqrt_of = {_int(q["v"][0]): _int(q["sqrt_l"]) for q in rec[:n_pairs] if int(q["kind"]) & 2}
    assert sqrt_of[0] == 0 and sqrt_of[1] in (1, P - 1) and sqrt_of[4] in (2, P - 2)
    assert pow(3, (P - 1) // 2, P) == P - 1 and sqrt_of[3] ** 2 % P == P - 3 and sqrt_of[P - 1] in (1, P - 1)  # the non-residues 3 and p - 1
    # the point formulas on curve points: secp256k1.py's affine addition, after (X / Z^2, Y / Z^3)
    n_degenerate = 0
    for q, (X, Y, Z, x2, y2, pt, other) in zip(rec[n_pairs:], points):
        assert [_int(q["v"][k]) for k in range(5)] == [X, Y, Z, x2, y2] and Z != 1 and _affine(X, Y, Z) == pt
        assert (pt[1] ** 2 - pt[0] ** 3 - 7) % P == 0 and (y2 * y2 - x2 ** 3 - 7) % P == 0
        jd = [_int(q["jd_l"][k]) for k in range(3)]
        assert _affine(*jd) == ec.add(pt, pt)
        ja = [_int(q["ja_l"][k]) for k in range(3)]
        if other[0] == pt[0]:  # the same point, or its negative: the formulas have no case distinction, the contract is Z == 0
            assert ja[2] == 0, (hex(X), hex(x2))
            n_degenerate += 1
        else:
            assert ja[2] != 0 and _affine(*ja) == ec.add(pt, other)
    assert n_degenerate == 2 * len(points) // 5 and len(points) >= 25
    return rec.size


def test_ec_field_inputs_cover_every_branch_and_the_model_equals_python_integers(exe, tmp_path):
    stdout, rec, points = _run(exe, tmp_path, "--host-only")
    n = _assert_equals_python_integers(rec, points)
    _assert_coverage(stdout, n)
    assert stdout.strip().splitlines()[-1] == f"ok {n} host-only"


@pytest.mark.gpu
def test_lane_form_and_register_form_equal_the_host_arithmetic(exe, tmp_path):
    stdout, rec, points = _run(exe, tmp_path)
    assert stdout.strip().splitlines()[-1].startswith("ok ") and not stdout.strip().endswith("host-only"), stdout[-2000:]
    assert int(stdout.strip().splitlines()[-1].split()[1]) >= 174 * 174
    n = _assert_equals_python_integers(rec, points)
    _assert_coverage(stdout, n)
    assert stdout.strip().splitlines()[-1] == f"ok {n}"
