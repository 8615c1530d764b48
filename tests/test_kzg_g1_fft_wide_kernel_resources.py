"""The kernels of csrc/kzg_g1_fft_wide_kernels.cuh under the rule of tests/test_kzg_cell_verify_kernel_resources.py: the unit compiles for
gfx950 (ONCE for this module: the `usage` fixture), every kernel exists in both launch forms (k_single, k_multi), uses no scratch
(private-segment) memory and has the static LDS it declares — none: the points of a wide transform live in HBM — and each keeps the vector
registers measured when it was written. The kernels from before this family are pinned by tests/test_kzg_kernel_resources.py and its
siblings, which pass unchanged: that is the proof that the wide transform moved none of them (k_kzg_g1_fft and k_kzg_g1_compress, which
it launches, included)."""
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


KERNELS = ("k_kzg_g1_fft_stage", "k_kzg_g1_fft_order", "k_kzg_g1_fft_load", "k_kzg_g1_affine")
# gfx950, -O3: (k_single, k_multi)
VGPRS = {"k_kzg_g1_fft_stage": (256, 256), "k_kzg_g1_fft_order": (256, 256), "k_kzg_g1_fft_load": (28, 28), "k_kzg_g1_affine": (108, 104)}


def test_the_wide_transform_kernels_use_no_scratch_no_lds_and_keep_their_registers(usage):
    """k_kzg_g1_fft_stage and k_kzg_g1_fft_order hold kzg_g1_mul_split (two doublings and a complete addition around a table read) and
    fill the 256 architectural registers like k_kzg_g1_fft, the rest of their values in accumulation registers, not in scratch: one
    wave a SIMD, which costs nothing where a whole setup is 32 waves. The two byte-form kernels hold a point, or one inversion."""
    u = usage
    for kernel in KERNELS:
        for form, k in u.forms(kernel, f"L{len(kernel)}{kernel}E").items():
            assert u.scratch[k] == 0, (u.names[k], u.scratch[k])
            assert u.lds[k] == 0, (u.names[k], u.lds[k])
            assert u.vgprs[k] <= 256, (u.names[k], u.vgprs[k])
            assert u.vgprs[k] == VGPRS[kernel][form == "k_multi"], (u.names[k], u.vgprs[k])
