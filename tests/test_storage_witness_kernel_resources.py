"""The witness trees' kernels (csrc/storage_witness_kernels.cuh) under the rule of tests/test_kernel_resources.py: no kernel of libzkw may use
scratch (private-segment) memory — k_sw_lookup runs on the blocks' storage contexts, whose queues would keep that scratch for good — and
the vector registers of the two kernels that matter, as measured when they were written: a later spill or a fold that no longer fits its
registers shows here, without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# gfx950, -O3, both launch forms (k_single, k_multi) alike
VGPRS = {"k_sw_lookup": 30, "k_sw_verify": 49}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_witness_kernels_use_no_scratch_and_keep_their_registers(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_storage_tree.hip"), "-o",
                        str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs)
    for kernel in ("k_sw_lookup", "k_sw_verify", "k_sw_gather", "k_sw_unique_keys", "k_sw_count"):
        forms = [k for k, n in enumerate(names) if f"{len(kernel)}{kernel}E" in n]
        assert len(forms) == 2, kernel  # both launch forms
        for k in forms:
            assert scratch[k] == 0, (names[k], scratch[k])
            if kernel in VGPRS:
                assert vgprs[k] == VGPRS[kernel], (names[k], vgprs[k])
