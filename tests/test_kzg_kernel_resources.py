"""The kernels of the EIP-4844 blob witness (csrc/kzg_kernels.cuh, driver csrc/zkw_kzg.hip) under the rule of
tests/test_storage_witness_chain_kernel_resources.py: zkw_kzg.hip compiles for gfx950, every hot-path kernel exists in both launch forms
(k_single, k_multi) and uses no scratch (private-segment) memory, and each keeps the vector registers measured when it was written. A
Jacobian addition over 12-word field elements holds ~240 registers around an outlined multiplication whose operands must travel in
registers: a spill, or an operand that the calling convention moves to the stack (a kernel's figure includes its callees'), shows here,
without a GPU. The two kernels of
zkw_kzg_settings_create (k_kzg_decompress, k_kzg_table) run once per handle and are not pinned."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# commit: accumulate, reduce (finish + compress); opening and the short hashes (tail); linear hash; zkw_kzg_commit's range check
KERNELS = ("k_kzg_accumulate", "k_kzg_finish", "k_kzg_compress", "k_kzg_linear_hash", "k_kzg_tail", "k_kzg_check")
# gfx950, -O3: (k_single, k_multi)
VGPRS = {"k_kzg_accumulate": (229, 231), "k_kzg_finish": (243, 243), "k_kzg_compress": (244, 246),
         "k_kzg_linear_hash": (25, 26), "k_kzg_tail": (73, 77), "k_kzg_check": (26, 26)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kzg_kernels_use_no_scratch_and_keep_their_registers(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_kzg.hip"), "-o",
                        str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs)
    for kernel in KERNELS:
        forms = {("k_single" if "k_single" in n else "k_multi"): k for k, n in enumerate(names) if f"{len(kernel)}{kernel}E" in n}
        assert sorted(forms) == ["k_multi", "k_single"], (kernel, forms)  # both launch forms
        for form, k in forms.items():
            assert scratch[k] == 0, (names[k], scratch[k])
            assert vgprs[k] == VGPRS[kernel][form == "k_multi"], (names[k], vgprs[k])
