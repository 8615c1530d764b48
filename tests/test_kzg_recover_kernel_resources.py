"""The kernels of EIP-7594 recovery (csrc/kzg_recover_kernels.cuh, driver csrc/zkw_kzg.hip) under the rule of
tests/test_kzg_cells_kernel_resources.py: the unit compiles for gfx950, every kernel exists in both launch forms (k_single, k_multi) and uses
no scratch (private-segment) memory — the 128-byte slot table is a kernel argument taken by reference, not a private copy — and the static
LDS is what the kernels declare: the 128 elements of k_kzg_recover_vanish's two transforms, and for k_kzg_recover_halves the word of the
range check (padded to 16 bytes ahead of the dynamic array); the two transform kernels take their 128 KiB at launch. No kernel uses more
than 256 vector registers: the eight waves of a 512-lane workgroup are two a SIMD, and two waves of 256 registers are what a SIMD holds."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# static LDS bytes per workgroup
LDS = {"k_kzg_recover_vanish": 128 * 32, "k_kzg_recover_halves": 16, "k_kzg_recover_quotient": 0, "k_kzg_recover_check": 0}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_recover_kernels_use_no_scratch_and_the_lds_they_declare(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_kzg.hip"), "-o",
                        str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds)
    for kernel, want in LDS.items():
        forms = {("k_single" if "k_single" in n else "k_multi"): k for k, n in enumerate(names) if f"L{len(kernel)}{kernel}E" in n}
        assert sorted(forms) == ["k_multi", "k_single"], (kernel, forms)  # both launch forms
        for k in forms.values():
            print(names[k][:60], "VGPRs", vgprs[k], "LDS", lds[k], "scratch", scratch[k])
            assert scratch[k] == 0, (names[k], scratch[k])
            assert lds[k] == want, (names[k], lds[k])
            assert vgprs[k] <= 256, (names[k], vgprs[k])
