"""The kernel of the producers from the evaluation form, k_kzg_blob_intt (csrc/kzg_open_kernels.cuh, driver csrc/zkw_kzg.hip), under the rule
of tests/test_kzg_open_kernel_resources.py: the unit compiles for gfx950, the kernel exists in both launch forms (k_single, k_multi), uses no
scratch (private-segment) memory and keeps the vector registers measured when it was written (64: it holds one product at a time like the
forward transform's 72, without that kernel's 31-byte loads). Its 128 KiB of LDS are declared at launch; the static figure is the word the
range check shares (a 16-byte slot)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# gfx950, -O3: (k_single, k_multi)
VGPRS = {"k_kzg_blob_intt": (64, 64)}
LDS = {"k_kzg_blob_intt": 16}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_inverse_transform_uses_no_scratch_and_keeps_its_registers(tmp_path):
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
