"""CPU-side checks of the KZG verification boundary: include/zkw.h declares zkw_kzg_verifier_create / _free / _bytes, zkw_kzg_verify and
zkw_eip4844_verify with the documented prototypes, the library exports them, and native.SYMBOLS and native.KzgVerifier bind them."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkw_kzg_verifier_create", "zkw_kzg_verifier_free", "zkw_kzg_verifier_bytes", "zkw_kzg_verify", "zkw_eip4844_verify")


def test_prototypes(tmp_path):
    src = r"""
    #include <stddef.h>
    #include "zkw.h"
    /* assigning to pointers of the documented types fails to compile if a prototype differs */
    int (*p_create)(zkw_ctx *, const uint8_t *, zkw_kzg_verifier **) = zkw_kzg_verifier_create;
    void (*p_free)(zkw_kzg_verifier *) = zkw_kzg_verifier_free;
    size_t (*p_bytes)(const zkw_kzg_verifier *) = zkw_kzg_verifier_bytes;
    int (*p_verify)(const zkw_kzg_verifier *, zkw_ctx *, const uint8_t *, const uint8_t *, const uint8_t *, const uint8_t *, size_t, uint8_t *) = zkw_kzg_verify;
    int (*p_blob)(const zkw_kzg_verifier *, zkw_ctx *, const zkw_eip4844_record *, const zkw_eip4844_proof_record *, size_t, uint8_t *) = zkw_eip4844_verify;
    int main(void){ return p_create && p_free && p_bytes && p_verify && p_blob ? 0 : 1; }
    """
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(tmp_path / "t.c")])
    from era_zkevm_test_harness_amd import build

    lib = build.build()
    subprocess.check_call(["gcc", "-o", str(tmp_path / "t"), str(tmp_path / "t.o"), lib, f"-Wl,-rpath,{os.path.dirname(lib)}", "-Wl,--allow-shlib-undefined"])
    subprocess.check_call([str(tmp_path / "t")])


def test_library_exports_the_verification_symbols():
    from era_zkevm_test_harness_amd import build, native

    lib = ctypes.CDLL(build.build())
    names = {n for n, _, _ in native.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in names, name
    assert callable(native.KzgVerifier.verify) and callable(native.KzgVerifier.eip4844_verify)
    assert (native.KZG_VERDICT_FAILS, native.KZG_VERDICT_HOLDS, native.KZG_VERDICT_BAD_COMMITMENT, native.KZG_VERDICT_BAD_PROOF,
            native.KZG_VERDICT_BAD_SCALAR) == (0, 1, 2, 3, 4)
