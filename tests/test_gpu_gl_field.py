"""The Goldilocks field of csrc/gl64.cuh, function by function: tests/csrc_gpu/gl_field_test.hip compares every device form (add, sub, neg,
add_canon, reduce128, mul = mul_cyc, mul_sched, mul_lat, sqr, mul_add, pow7, pow7_lat, mul_small, mul_pow2, pow, inv, canon) and, on the
same inputs, every host form with `unsigned __int128 % p` written in the program. The inputs are the cross product of 18 edge words,
2^16 seeded tuples and sets built so that every carry of every form fires and does not fire; a host word model of the device steps counts
them, and the conditions asserted here are conditions on those inputs. The CPU test runs the program with --host-only (inputs, coverage
and host forms, no HIP call); the GPU test runs it whole."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EDGE_WORDS = 18
SEEDED = 1 << 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gl_field") / "gl_field_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc_gpu", "gl_field_test.hip"), "-o", out])
    return out


def _cover(stdout):
    """{operation: {key: int}} from the program's "cover <op> n <tuples> <key> <hex> ..." lines"""
    ops = {}
    for line in stdout.splitlines():
        w = line.split()
        if w and w[0] == "cover":
            assert "MISSING" not in w, line
            ops[w[1]] = {"n": int(w[3]), **{k: int(v, 16) for k, v in zip(w[4::2], w[5::2])}}
    return ops


def _assert_coverage(ops):
    two, one = EDGE_WORDS ** 2 + SEEDED, EDGE_WORDS + SEEDED
    for name in ("add", "sub", "add_canon", "reduce128", "mul", "mul_cyc", "mul_sched", "mul_lat"):
        assert ops[name]["n"] >= two, name
    for name in ("neg", "sqr", "pow7", "pow7_lat", "inv", "canon"):
        assert ops[name]["n"] >= one, name
    assert ops["mul_add"]["n"] >= EDGE_WORDS ** 3 + SEEDED
    assert ops["mul_small"]["n"] >= EDGE_WORDS + SEEDED
    assert ops["mul_pow2"]["n"] >= 32 * EDGE_WORDS + SEEDED
    assert ops["pow"]["n"] >= 6 * EDGE_WORDS
    # mul (= mul_cyc on the device): all eight combinations of (cm, c1, b1)
    assert ops["mul"]["flags"] == 0xFF and ops["mul_cyc"]["flags"] == 0xFF
    # mul_sched and the device mul_lat: (borrow of lo - hh, carry of + hl EPS) all four ways, cm both ways
    for name in ("mul_sched", "mul_lat"):
        assert ops[name]["bc"] == 0xF and ops[name]["cm"] == 0x3, name
    assert ops["reduce128"]["bc"] == 0xF
    assert ops["add"]["cc"] == 0b1011  # (c, c2) = (0,0), (1,0), (1,1)
    assert ops["sub"]["bb"] == 0b1011
    assert ops["add_canon"]["w"] == 0b11
    assert ops["mul_small"]["c"] == 0b11 and ops["mul_small"]["c3"] == 0b11
    assert ops["mul_pow2"]["s0"] == 0xFFFFFFFF and ops["mul_pow2"]["s1"] == 0xFFFFFFFE  # shift 0 has no high part to carry


def _total(stdout):
    last = stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok", stdout[-2000:]
    return int(last[1])


def test_gl_field_inputs_cover_every_carry(exe):
    r = subprocess.run([exe, "--host-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1].endswith("host-only")
    ops = _cover(r.stdout)
    _assert_coverage(ops)
    assert _total(r.stdout) == sum(o["n"] for o in ops.values())


@pytest.mark.gpu
def test_gl_field_device_forms_equal_int128(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ops = _cover(r.stdout)
    _assert_coverage(ops)
    assert len(ops) == 18 and _total(r.stdout) == sum(o["n"] for o in ops.values())
    assert not r.stdout.strip().endswith("host-only")
