"""The kernels of the EIP-7594 cells and cell proofs (csrc/kzg_cell_kernels.cuh, driver csrc/zkw_kzg.hip) under the rule of
tests/test_kzg_open_kernel_resources.py: the unit compiles for gfx950, every kernel exists in both launch forms (k_single, k_multi) and uses
no scratch (private-segment) memory — the window table of the G1 transform's products is in global memory on purpose, not a private array —
and the static LDS is what the kernels declare: the transform's 128 Jacobian points, the four 128-element vectors of k_kzg_cell_toeplitz,
and for k_kzg_cell_msm the digits, the 256 buckets and the fold's 128 points, which must stay below the 64 KiB a workgroup may declare
statically. The sum kernel keeps two waves on a SIMD (at most 256 vector registers)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# static LDS bytes per workgroup (k_kzg_cells declares its 128 KiB at launch)
LDS = {"k_kzg_g1_fft": 128 * 144, "k_kzg_g1_lift": 0, "k_kzg_g1_compress": 0, "k_kzg_cell_setup_x": 0, "k_kzg_cell_setup_affine": 0, "k_kzg_cell_wpow": 0,
       "k_kzg_cells": 0, "k_kzg_cell_toeplitz": 4 * 128 * 32, "k_kzg_cell_msm": 2048 + 256 * 144 + 128 * 144, "k_kzg_cell_horner": 0}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_cell_kernels_use_no_scratch_and_the_lds_they_declare(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_kzg.hip"), "-o",
                        str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds)
    assert LDS["k_kzg_cell_msm"] < 65536
    for kernel, want in LDS.items():
        forms = {("k_single" if "k_single" in n else "k_multi"): k for k, n in enumerate(names) if f"L{len(kernel)}{kernel}E" in n}
        assert sorted(forms) == ["k_multi", "k_single"], (kernel, forms)  # both launch forms
        for k in forms.values():
            assert scratch[k] == 0, (names[k], scratch[k])
            assert lds[k] == want, (names[k], lds[k])
            assert vgprs[k] <= 256, (names[k], vgprs[k])
