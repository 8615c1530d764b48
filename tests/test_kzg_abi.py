"""CPU-side checks of the EIP-4844 boundary: include/zkw.h declares the KZG calls with the documented prototypes, zkw_eip4844_record is
192 bytes with the fields where numpy's EIP4844_RECORD has them, and the library exports every one of the symbols."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KZG_SYMBOLS = ("zkw_kzg_settings_create", "zkw_kzg_settings_free", "zkw_kzg_settings_num_points", "zkw_kzg_settings_bytes", "zkw_kzg_commit",
               "zkw_eip4844_witness")


def test_prototypes_and_record_layout(tmp_path):
    from era_zkevm_test_harness_amd import native

    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "zkw.h"
    /* assigning to pointers of the documented types fails to compile if a prototype differs */
    int (*p_create)(zkw_ctx *, const uint8_t *, size_t, zkw_kzg_settings **) = zkw_kzg_settings_create;
    void (*p_free)(zkw_kzg_settings *) = zkw_kzg_settings_free;
    size_t (*p_num)(const zkw_kzg_settings *) = zkw_kzg_settings_num_points;
    size_t (*p_bytes)(const zkw_kzg_settings *) = zkw_kzg_settings_bytes;
    int (*p_commit)(const zkw_kzg_settings *, zkw_ctx *, const uint8_t *, size_t, size_t, uint8_t *) = zkw_kzg_commit;
    int (*p_witness)(const zkw_kzg_settings *, zkw_ctx *, const uint8_t *, size_t, zkw_eip4844_record *) = zkw_eip4844_witness;
    int main(void){
      printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(zkw_eip4844_record), offsetof(zkw_eip4844_record, linear_hash),
             offsetof(zkw_eip4844_record, versioned_hash), offsetof(zkw_eip4844_record, output_hash),
             offsetof(zkw_eip4844_record, evaluation_point), offsetof(zkw_eip4844_record, opening_value), offsetof(zkw_eip4844_record, commitment));
      return 0; }
    """
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(tmp_path / "t.c")])
    from era_zkevm_test_harness_amd import build

    lib = build.build()
    subprocess.check_call(["gcc", "-o", str(tmp_path / "t"), str(tmp_path / "t.o"), lib, f"-Wl,-rpath,{os.path.dirname(lib)}", "-Wl,--allow-shlib-undefined"])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    rec = native.EIP4844_RECORD
    assert sizes[0] == 192 == rec.itemsize
    assert sizes[1:] == [rec.fields[f][1] for f in ("linear_hash", "versioned_hash", "output_hash", "evaluation_point", "opening_value", "commitment")]
    assert native.EIP4844_BLOB_BYTES == 126976


def test_library_exports_the_kzg_symbols():
    from era_zkevm_test_harness_amd import build, native

    lib = ctypes.CDLL(build.build())
    names = {n for n, _, _ in native.SYMBOLS}
    for name in KZG_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in names, name
    assert hasattr(native, "KzgSettings") and callable(native.KzgSettings.commit) and callable(native.KzgSettings.eip4844_witness)
