"""The kernels of csrc/zkw_kzg.hip, family by family, under the rule of tests/test_storage_witness_chain_kernel_resources.py: the unit
compiles for gfx950 (ONCE for this module: the `usage` fixture), every hot-path kernel exists in both launch forms (k_single, k_multi) and
uses no scratch (private-segment) memory, and each keeps the figures measured when it was written — vector registers, static LDS, or both;
every test says which and why. A spill, or an operand that the calling convention moves to the stack (a kernel's figure includes its
callees'), shows here, without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


class Usage:
    """-Rpass-analysis=kernel-resource-usage of zkw_kzg.hip: one entry per kernel symbol, in the compiler's order."""

    def __init__(self, stderr):
        self.names = re.findall(r"Function Name: (\S+)", stderr)
        self.scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", stderr)]
        self.vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", stderr)]
        self.agprs = [int(x) for x in re.findall(r" AGPRs: (\d+)", stderr)]
        self.lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", stderr)]
        assert len(self.names) == len(self.scratch) == len(self.vgprs) == len(self.agprs) == len(self.lds)

    def forms(self, kernel, mangled):
        """{"k_single": index, "k_multi": index} of the symbols that hold `mangled` (the kernel's name as the test spells it in a
        mangled symbol); both launch forms must be there."""
        forms = {("k_single" if "k_single" in n else "k_multi"): k for k, n in enumerate(self.names) if mangled in n}
        assert sorted(forms) == ["k_multi", "k_single"], (kernel, forms)  # both launch forms
        return forms


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "zkw_kzg.hip"), "-o",
                        str(tmp_path_factory.mktemp("kzg") / "x.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return Usage(r.stderr)


def test_kzg_kernels_use_no_scratch_and_keep_their_registers(usage):
    """The EIP-4844 blob witness (csrc/kzg_kernels.cuh). A Jacobian addition over 12-word field elements holds ~240 registers around an
    outlined multiplication whose operands must travel in registers. The two kernels of zkw_kzg_settings_create (k_kzg_decompress,
    k_kzg_table) run once per handle and are not pinned."""
    # commit: accumulate, reduce (finish + compress); opening and the short hashes (tail); linear hash; zkw_kzg_commit's range check
    # gfx950, -O3: (k_single, k_multi)
    VGPRS = {"k_kzg_accumulate": (229, 231), "k_kzg_finish": (243, 243), "k_kzg_compress": (244, 246),
             "k_kzg_linear_hash": (25, 26), "k_kzg_tail": (73, 77), "k_kzg_check": (26, 26)}
    u = usage
    for kernel in VGPRS:
        for form, k in u.forms(kernel, f"{len(kernel)}{kernel}E").items():
            assert u.scratch[k] == 0, (u.names[k], u.scratch[k])
            assert u.vgprs[k] == VGPRS[kernel][form == "k_multi"], (u.names[k], u.vgprs[k])


def _registers_and_lds(u, VGPRS, LDS):
    """(the check the open, verify and producer families share: no scratch, the registers and the static LDS as pinned)"""
    for kernel in VGPRS:
        for form, k in u.forms(kernel, f"{len(kernel)}{kernel}").items():
            assert u.scratch[k] == 0, (u.names[k], u.scratch[k])
            assert u.vgprs[k] == VGPRS[kernel][form == "k_multi"], (u.names[k], u.vgprs[k])
            assert u.lds[k] == LDS[kernel], (u.names[k], u.lds[k])


def test_kzg_open_kernels_use_no_scratch_and_keep_their_registers(usage):
    """The KZG proofs (csrc/kzg_open_kernels.cuh). k_kzg_blob_ntt declares its 128 KiB of LDS at launch, so its static figure is zero; the
    quotient's scan holds 256 elements of Fr (8 KiB) and the challenge's message schedules 64 blocks (16 KiB)."""
    # gfx950, -O3: (k_single, k_multi)
    VGPRS = {"k_kzg_quotient": (74, 74), "k_kzg_twiddles": (54, 54), "k_kzg_blob_ntt": (72, 72), "k_kzg_blob_challenge": (95, 95),
             "k_kzg_proofs_out": (6, 6)}
    LDS = {"k_kzg_quotient": 8192, "k_kzg_twiddles": 0, "k_kzg_blob_ntt": 0, "k_kzg_blob_challenge": 16384, "k_kzg_proofs_out": 0}
    _registers_and_lds(usage, VGPRS, LDS)


def test_kzg_verify_kernels_use_no_scratch_and_keep_their_registers(usage):
    """The KZG verification (csrc/kzg_verify_kernels.cuh on csrc/bls12_381_pairing.cuh). All three hold the outlined product of Fq and the
    values around it and fill the 256 architectural registers (the rest of their values sit in accumulation registers, not in scratch).
    k_kzg_verify_pairing declares the 27 648 bytes of its Fq12 slots at launch, so its static figure is zero."""
    # gfx950, -O3: (k_single, k_multi)
    VGPRS = {"k_kzg_g2_prepare": (256, 256), "k_kzg_verify_points": (256, 256), "k_kzg_verify_pairing": (256, 256)}
    LDS = {"k_kzg_g2_prepare": 0, "k_kzg_verify_points": 0, "k_kzg_verify_pairing": 0}
    _registers_and_lds(usage, VGPRS, LDS)


def test_kzg_blob_eval_uses_no_scratch_and_keeps_its_registers_and_lds(usage):
    """The blob evaluation (csrc/kzg_eval_kernels.cuh). The sixteen prefix products of Montgomery's trick (128 words) live in registers
    across the inversion, so the kernel fills the 256 architectural registers and keeps the rest in accumulation registers; its LDS is the
    add tree (256 x 32 bytes) and ten words of flags."""
    # gfx950, -O3: (k_single, k_multi)
    VGPRS = {"k_kzg_blob_eval": (256, 256)}
    AGPRS = {"k_kzg_blob_eval": (65, 65)}
    LDS = {"k_kzg_blob_eval": 8232}
    u = usage
    _registers_and_lds(u, VGPRS, LDS)
    for kernel in AGPRS:
        for form, k in u.forms(kernel, f"{len(kernel)}{kernel}").items():
            assert u.agprs[k] == AGPRS[kernel][form == "k_multi"], (u.names[k], u.agprs[k])


def test_the_inverse_transform_uses_no_scratch_and_keeps_its_registers(usage):
    """The kernel of the producers from the evaluation form, k_kzg_blob_intt (csrc/kzg_open_kernels.cuh). 64 vector registers: it holds one
    product at a time like the forward transform's 72, without that kernel's 31-byte loads. Its 128 KiB of LDS are declared at launch; the
    static figure is the word the range check shares (a 16-byte slot)."""
    # gfx950, -O3: (k_single, k_multi)
    VGPRS = {"k_kzg_blob_intt": (64, 64)}
    LDS = {"k_kzg_blob_intt": 16}
    _registers_and_lds(usage, VGPRS, LDS)


def _lds_and_two_waves(u, LDS, show=False):
    """(the check the cell and recovery families share: no scratch, the static LDS as declared, at most 256 vector registers)"""
    for kernel, want in LDS.items():
        for k in u.forms(kernel, f"L{len(kernel)}{kernel}E").values():
            if show:
                print(u.names[k][:60], "VGPRs", u.vgprs[k], "LDS", u.lds[k], "scratch", u.scratch[k])
            assert u.scratch[k] == 0, (u.names[k], u.scratch[k])
            assert u.lds[k] == want, (u.names[k], u.lds[k])
            assert u.vgprs[k] <= 256, (u.names[k], u.vgprs[k])


def test_the_cell_kernels_use_no_scratch_and_the_lds_they_declare(usage):
    """The EIP-7594 cells and cell proofs (csrc/kzg_cell_kernels.cuh). No scratch — the window table of the G1 transform's products is in
    global memory on purpose, not a private array — and the static LDS is what the kernels declare: the transform's 128 Jacobian points, the
    four 128-element vectors of k_kzg_cell_toeplitz, and for k_kzg_cell_msm the digits, the 256 buckets and the fold's 128 points, which must
    stay below the 64 KiB a workgroup may declare statically. The sum kernel keeps two waves on a SIMD (at most 256 vector registers)."""
    # static LDS bytes per workgroup (k_kzg_cells declares its 128 KiB at launch)
    LDS = {"k_kzg_g1_fft": 128 * 144, "k_kzg_g1_lift": 0, "k_kzg_g1_compress": 0, "k_kzg_cell_setup_x": 0, "k_kzg_cell_setup_affine": 0,
           "k_kzg_cell_wpow": 0, "k_kzg_cells": 0, "k_kzg_cell_toeplitz": 4 * 128 * 32, "k_kzg_cell_msm": 2048 + 256 * 144 + 128 * 144,
           "k_kzg_cell_horner": 0}
    assert LDS["k_kzg_cell_msm"] < 65536
    _lds_and_two_waves(usage, LDS)


def test_the_recover_kernels_use_no_scratch_and_the_lds_they_declare(usage):
    """EIP-7594 recovery (csrc/kzg_recover_kernels.cuh). No scratch — the 128-byte slot table is a kernel argument taken by reference, not a
    private copy — and the static LDS is what the kernels declare: the 128 elements of k_kzg_recover_vanish's two transforms, and for
    k_kzg_recover_halves the word of the range check (padded to 16 bytes ahead of the dynamic array); the two transform kernels take their
    128 KiB at launch. No kernel uses more than 256 vector registers: the eight waves of a 512-lane workgroup are two a SIMD, and two waves
    of 256 registers are what a SIMD holds."""
    # static LDS bytes per workgroup
    LDS = {"k_kzg_recover_vanish": 128 * 32, "k_kzg_recover_halves": 16, "k_kzg_recover_quotient": 0, "k_kzg_recover_check": 0}
    _lds_and_two_waves(usage, LDS, show=True)
