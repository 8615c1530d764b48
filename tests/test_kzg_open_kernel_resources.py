"""The kernels of the KZG proofs (csrc/kzg_open_kernels.cuh, driver csrc/zkw_kzg.hip) under the rule of tests/test_kzg_kernel_resources.py:
the unit compiles for gfx950, every kernel exists in both launch forms (k_single, k_multi) and uses no scratch (private-segment) memory,
and each keeps the vector registers measured when it was written. k_kzg_blob_ntt declares its 128 KiB of LDS at launch, so its static
figure is zero; the quotient's scan holds 256 elements of Fr (8 KiB) and the challenge's message schedules 64 blocks (16 KiB)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# gfx950, -O3: (k_single, k_multi)
VGPRS = {"k_kzg_quotient": (74, 74), "k_kzg_twiddles": (54, 54), "k_kzg_blob_ntt": (72, 72), "k_kzg_blob_challenge": (95, 95),
         "k_kzg_proofs_out": (6, 6)}
LDS = {"k_kzg_quotient": 8192, "k_kzg_twiddles": 0, "k_kzg_blob_ntt": 0, "k_kzg_blob_challenge": 16384, "k_kzg_proofs_out": 0}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kzg_open_kernels_use_no_scratch_and_keep_their_registers(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_kzg.hip"), "-o",
                        str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds)
    for kernel in VGPRS:
        forms = {("k_single" if "k_single" in n else "k_multi"): k for k, n in enumerate(names) if f"{len(kernel)}{kernel}" in n}
        assert sorted(forms) == ["k_multi", "k_single"], (kernel, forms)  # both launch forms
        for form, k in forms.items():
            assert scratch[k] == 0, (names[k], scratch[k])
            assert vgprs[k] == VGPRS[kernel][form == "k_multi"], (names[k], vgprs[k])
            assert lds[k] == LDS[kernel], (names[k], lds[k])
