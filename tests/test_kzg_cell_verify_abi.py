"""CPU-side checks of the cell-proof verification boundary: include/zkw.h declares zkw_kzg_verify_cells and zkw_kzg_commit_cells with the
documented prototypes, the library exports them, and native.SYMBOLS, native.KzgVerifier and native.KzgSettings bind them; the verdict
codes keep their numbers and 5 is the new one."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkw_kzg_verify_cells", "zkw_kzg_commit_cells")


def test_prototypes(tmp_path):
    src = r"""
    #include <stddef.h>
    #include "zkw.h"
    /* assigning to pointers of the documented types fails to compile if a prototype differs */
    int (*p_verify)(const zkw_kzg_verifier *, const zkw_kzg_settings *, zkw_ctx *, const uint8_t *, const uint64_t *, const uint8_t *, const uint8_t *, size_t,
                    uint8_t *) = zkw_kzg_verify_cells;
    int (*p_commit)(const zkw_kzg_settings *, zkw_ctx *, const uint64_t *, const uint8_t *, size_t, uint8_t *) = zkw_kzg_commit_cells;
    int main(void){ return p_verify && p_commit ? 0 : 1; }
    """
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(tmp_path / "t.c")])
    from era_zkevm_test_harness_amd import build

    lib = build.build()
    subprocess.check_call(["gcc", "-o", str(tmp_path / "t"), str(tmp_path / "t.o"), lib, f"-Wl,-rpath,{os.path.dirname(lib)}", "-Wl,--allow-shlib-undefined"])
    subprocess.check_call([str(tmp_path / "t")])


def test_library_exports_the_symbols_and_python_binds_them():
    from era_zkevm_test_harness_amd import build, native

    lib = ctypes.CDLL(build.build())
    names = {n for n, _, _ in native.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in names, name
    assert callable(native.KzgVerifier.verify_cells) and callable(native.KzgSettings.commit_cells)
    assert (native.KZG_VERDICT_FAILS, native.KZG_VERDICT_HOLDS, native.KZG_VERDICT_BAD_COMMITMENT, native.KZG_VERDICT_BAD_PROOF,
            native.KZG_VERDICT_BAD_SCALAR, native.KZG_VERDICT_BAD_INDEX) == (0, 1, 2, 3, 4, 5)


def test_the_kernel_header_keeps_the_codes():
    text = open(os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc", "kzg_verify_kernels.cuh")).read()
    for name, code in (("KZG_VERDICT_FAILS", 0), ("KZG_VERDICT_HOLDS", 1), ("KZG_VERDICT_BAD_COMMITMENT", 2), ("KZG_VERDICT_BAD_PROOF", 3),
                       ("KZG_VERDICT_BAD_SCALAR", 4), ("KZG_VERDICT_BAD_INDEX", 5)):
        assert "%s = %d" % (name, code) in text, name
