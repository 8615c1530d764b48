"""The kernels that advance a witness tree (csrc/storage_witness_kernels.cuh, "advance") under the rule of tests/test_kernel_resources.py and
tests/test_storage_witness_kernel_resources.py: every one exists in both launch forms (k_single, k_multi) and uses no scratch
(private-segment) memory, and the fold and the paths kernel keep the vector registers measured when they were written — the fold is a
chain of 256 dependent Blake2s compressions per written key, k_sw_verify's class; a spill or a fold that outgrows it shows here, without a
GPU. k_swa_fold's LDS is the current height of 1 024 written keys (hashes, d, nxt, entries): 44 KB."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

KERNELS = ("k_swa_locate", "k_swa_compact", "k_swa_leaves", "k_swa_fold", "k_swa_level", "k_swa_paths")
# gfx950, -O3: (k_single, k_multi)
VGPRS = {"k_swa_fold": (60, 52), "k_swa_level": (38, 38), "k_swa_paths": (20, 29)}
FOLD_LDS = 1024 * (32 + 4 + 4 + 4)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_advance_kernels_use_no_scratch_and_keep_their_registers(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_storage_tree.hip"), "-o",
                        str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds)
    for kernel in KERNELS:
        forms = {("k_single" if "k_single" in n else "k_multi"): k for k, n in enumerate(names) if f"{len(kernel)}{kernel}E" in n}
        assert sorted(forms) == ["k_multi", "k_single"], (kernel, forms)  # both launch forms
        for form, k in forms.items():
            assert scratch[k] == 0, (names[k], scratch[k])
            assert lds[k] == (FOLD_LDS if kernel == "k_swa_fold" else 0), (names[k], lds[k])
            if kernel in VGPRS:
                assert vgprs[k] == VGPRS[kernel][form == "k_multi"], (names[k], vgprs[k])
