"""The storage tree's kernels under the rule of tests/test_kernel_resources.py: no kernel of libzkw may use scratch (private-segment)
memory — zkw_storage_tree_answer_queries runs on the blocks' storage contexts, whose queues would keep that scratch for good."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_tree_kernel_uses_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_storage_tree.hip"), "-o",
                        str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch)
    for kernel in ("k_st_query", "k_st_level", "k_st_levels", "k_st_leaves", "k_st_emit", "k_st_writes"):  # both launch forms of each
        assert sum(1 for n in names if f"{len(kernel)}{kernel}E" in n) == 2, kernel
    bad = {n: s for n, s in zip(names, scratch) if s}
    assert not bad, f"kernels with scratch memory: {bad}"
