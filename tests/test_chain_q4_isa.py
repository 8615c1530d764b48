"""The quad-form Poseidon2 permutation (p2::Coop4, the permutation of the queue-chain kernels k_chain_full_q4 / q4x4) as gfx950 code: a
lone chain wave issues an instruction every ~4-8 cycles whatever it is, so its VALU count is its time. hipcc cross-compiles
tests/csrc_gpu/p2_quad_probe.hip; the permutation's part is the difference between a kernel that runs one and the same kernel without it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

VALU_BUDGET = 320  # wave-instructions per permutation; a wave runs 16 (one per quad)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _kernel_lines(asm, name):
    body = asm[asm.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    return [ln.strip() for ln in body.splitlines() if ln.strip() and not ln.strip().startswith((";", "."))]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("q4") / "probe.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "csrc_gpu", "p2_quad_probe.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    return _kernel_lines(asm, "k_q4_one"), _kernel_lines(asm, "k_q4_none")


def test_permutation_valu_count_within_budget(probe):
    one, none = probe
    valu = sum(ln.startswith("v_") for ln in one) - sum(ln.startswith("v_") for ln in none)
    assert 16 * 200 < valu <= 16 * VALU_BUDGET, valu


def test_permutation_has_no_scalar_memory_load(probe):
    one, none = probe
    # (both kernels load the per-lane constants of Coop4::init the same way; the permutation adds no load and no GOT walk)
    smem = lambda lines: [ln for ln in lines if re.match(r"s_(buffer_)?load_|s_getpc", ln)]
    assert len(smem(one)) == len(smem(none)), smem(one)


def test_permutation_is_straight_line(probe):
    one, _ = probe
    assert not [ln for ln in one if ln.startswith("s_cbranch")]


# VGPRs of the six queue-chain kernels before they became instantiations of one loop (ram_kernels.cuh, chain_body): the shared loop may
# not cost a form registers (docs/KERNELS.md 3.2, round 9)
CHAIN_VGPRS = {"k_chain_full": 93, "k_chain_full_x4": 93, "k_chain_full_q4": 162, "k_chain_full_q4x4": 162, "k_chain_full_p2": 242,
               "k_chain_full_lane": 140}


def test_quad_chain_kernels_use_no_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_api.hip"), "-o",
                        str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs)
    q4 = {n: s for n, s in zip(names, scratch) if "k_chain_full_q4" in n}
    assert len(q4) == 2, q4
    assert not any(q4.values()), q4
    # every form of the chain loop: no scratch, and no more VGPRs than its hand-written kernel had
    chain = {m.group(1): (s, v) for n, s, v in zip(names, scratch, vgprs) if (m := re.search(r"\d+(k_chain_full\w*?)EPKNS", n))}
    assert sorted(chain) == sorted(CHAIN_VGPRS), chain
    for k, (s, v) in chain.items():
        assert s == 0 and v <= CHAIN_VGPRS[k], (k, s, v)
