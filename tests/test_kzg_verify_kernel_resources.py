"""The kernels of the KZG verification (csrc/kzg_verify_kernels.cuh on csrc/bls12_381_pairing.cuh, driver csrc/zkw_kzg.hip) under the rule of
tests/test_kzg_kernel_resources.py: the unit compiles for gfx950, every kernel exists in both launch forms (k_single, k_multi) and uses no
scratch (private-segment) memory, and each keeps the vector registers measured when it was written. All three hold the outlined
product of Fq and the values around it and fill the 256 architectural registers (the rest of their values sit in accumulation
registers, not in scratch). k_kzg_verify_pairing declares the 27 648 bytes of its Fq12 slots at launch, so its static figure is zero."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# gfx950, -O3: (k_single, k_multi)
VGPRS = {"k_kzg_g2_prepare": (256, 256), "k_kzg_verify_points": (256, 256), "k_kzg_verify_pairing": (256, 256)}
LDS = {"k_kzg_g2_prepare": 0, "k_kzg_verify_points": 0, "k_kzg_verify_pairing": 0}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kzg_verify_kernels_use_no_scratch_and_keep_their_registers(tmp_path):
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
