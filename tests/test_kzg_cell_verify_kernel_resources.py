"""The kernels of csrc/kzg_cell_verify_kernels.cuh under the rule of tests/test_kzg_kernel_resources.py: the unit compiles for gfx950 (ONCE
for this module: the `usage` fixture), every kernel exists in both launch forms (k_single, k_multi), uses no scratch (private-segment)
memory and has the static LDS it declares, and each keeps the vector registers measured when it was written. The kernels from before this
family are pinned by tests/test_kzg_kernel_resources.py, which passes unchanged: that is the proof that sharing k_kzg_cell_msm's body
moved none of them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


class Usage:
    """-Rpass-analysis=kernel-resource-usage of zkw_kzg.hip: one entry per kernel symbol, in the compiler's order."""

    def __init__(self, stderr):
        self.names = re.findall(r"Function Name: (\S+)", stderr)
        self.scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", stderr)]
        self.vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", stderr)]
        self.agprs = [int(x) for x in re.findall(r" AGPRs: (\d+)", stderr)]
        self.lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", stderr)]
        assert len(self.names) == len(self.scratch) == len(self.vgprs) == len(self.agprs) == len(self.lds)

    def forms(self, kernel, mangled):
        """{"k_single": index, "k_multi": index} of the symbols that hold `mangled` (the kernel's name as the test spells it in a
        mangled symbol); both launch forms must be there."""
        forms = {("k_single" if "k_single" in n else "k_multi"): k for k, n in enumerate(self.names) if mangled in n}
        assert sorted(forms) == ["k_multi", "k_single"], (kernel, forms)  # both launch forms
        return forms


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_kzg.hip"), "-o",
                        str(tmp_path_factory.mktemp("kzg") / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return Usage(r.stderr)


# static LDS bytes per workgroup: four cells of 64 elements of Fr; k_kzg_cell_msm's digits, 256 buckets and the fold's 128 points
CELL_MSM_LDS = 2048 + 256 * 144 + 128 * 144
LDS = {"k_kzg_cell_interpolate": 4 * 64 * 32, "k_kzg_cell_commit_msm": CELL_MSM_LDS, "k_kzg_verify_cell_points": 0}
# gfx950, -O3: (k_single, k_multi)
VGPRS = {"k_kzg_cell_interpolate": (68, 68), "k_kzg_cell_commit_msm": (248, 248), "k_kzg_verify_cell_points": (256, 256)}


def test_the_cell_verify_kernels_use_no_scratch_and_keep_their_registers_and_lds(usage):
    """k_kzg_cell_interpolate holds one product of Fr at a time (68 registers, like the blob transforms' 64 to 72). The 64-term sum is
    k_kzg_cell_msm's body with another addressing and has its figures: 57 344 bytes of static LDS, below the 64 KiB a workgroup may declare,
    and two waves a SIMD. k_kzg_verify_cell_points, like k_kzg_verify_points, holds the outlined product of Fq and a point addition around
    it and fills the 256 architectural registers, the rest of its values in accumulation registers, not in scratch."""
    u = usage
    assert CELL_MSM_LDS < 65536
    for kernel in LDS:
        for form, k in u.forms(kernel, f"L{len(kernel)}{kernel}E").items():
            assert u.scratch[k] == 0, (u.names[k], u.scratch[k])
            assert u.lds[k] == LDS[kernel], (u.names[k], u.lds[k])
            assert u.vgprs[k] <= 256, (u.names[k], u.vgprs[k])
            assert u.vgprs[k] == VGPRS[kernel][form == "k_multi"], (u.names[k], u.vgprs[k])
