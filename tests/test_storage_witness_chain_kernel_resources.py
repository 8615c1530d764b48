"""The kernels of zkw_storage_tree_advance_witness_chain (csrc/storage_witness_kernels.cuh, "chain") under the rule of
tests/test_storage_witness_advance_kernel_resources.py: every one exists in both launch forms (k_single, k_multi), uses no scratch
(private-segment) memory and no LDS, and the walk and the wavefront step keep the vector registers measured when they were written — the
step runs 256 + K - 1 times per call with one Blake2s compression per fold thread, so a spill or a body that outgrows its occupancy shows
here, without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

KERNELS = ("k_swc_locate", "k_swc_compact", "k_swc_walk", "k_swc_step")
# gfx950, -O3: (k_single, k_multi)
VGPRS = {"k_swc_walk": (60, 61), "k_swc_step": (40, 40)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_chain_kernels_use_no_scratch_and_keep_their_registers(tmp_path):
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
            assert lds[k] == 0, (names[k], lds[k])
            if kernel in VGPRS:
                assert vgprs[k] == VGPRS[kernel][form == "k_multi"], (names[k], vgprs[k])
