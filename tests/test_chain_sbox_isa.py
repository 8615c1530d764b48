"""The S-box product of the chain forms (gl::mul_vcc, csrc/gl64.cuh) as gfx950 code. A lone chain wave's VALU count is its time
(DESIGN.md 5), and the product it replaces in the quad form (gl::mul_lat, ~25.7 instructions as the compiler emits it) was predicted to
shrink to ~17: at least half of that saving, 4 instructions for each of the 162 multiplications a lane runs in 16 permutations' worth of
wave-instructions — 40 per permutation — must show in the static count, or the asm statements have been wrapped in moves. hipcc
cross-compiles tests/csrc_gpu/p2_sbox_probe.hip as it stands and with -DGL_CHAIN_MUL_COMPILER_FORM (the parent's code); the
permutation's part is the difference between a kernel that runs one and the same kernel without it.

Measured: 258 VALU instructions per permutation against the parent's 319 (4 130 against 5 102 per wave-step of 16)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

MIN_SAVING = 40  # VALU instructions per permutation

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _kernel_lines(asm, name):
    body = asm[asm.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    return [ln.strip() for ln in body.splitlines() if ln.strip() and not ln.strip().startswith((";", "."))]


def _scratch(asm, name):
    return int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm[asm.index(".amdhsa_kernel " + name):]).group(1))


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("sbox")
    out = {}
    for form, flags in (("vcc", []), ("parent", ["-DGL_CHAIN_MUL_COMPILER_FORM"])):
        path = str(d / (form + ".s"))
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", *flags, "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "csrc_gpu", "p2_sbox_probe.hip"), "-o", path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(path).read()
        out[form] = (_kernel_lines(asm, "k_sbox_one"), _kernel_lines(asm, "k_sbox_none"), _scratch(asm, "k_sbox_one"))
    return out


def _valu(one, none):
    return sum(ln.startswith("v_") for ln in one) - sum(ln.startswith("v_") for ln in none)


def test_sbox_product_saves_at_least_40_valu_instructions_per_permutation(probes):
    new, old = _valu(*probes["vcc"][:2]), _valu(*probes["parent"][:2])
    print("VALU per wave-step of 16 permutations: mul_vcc %d, parent %d" % (new, old))
    assert 16 * 200 < new and old - new >= 16 * MIN_SAVING, (new, old)


def test_permutation_has_no_scratch_and_no_scalar_load(probes):
    one, none, scratch = probes["vcc"]
    assert scratch == 0
    assert not [ln for ln in one if ln.startswith(("scratch_", "buffer_"))]
    # (both kernels load the per-lane constants of Coop4::init the same way; the permutation adds no load and no GOT walk)
    smem = lambda lines: [ln for ln in lines if re.match(r"s_(buffer_)?load_|s_getpc", ln)]
    assert len(smem(one)) == len(smem(none)), smem(one)
