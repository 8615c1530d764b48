"""CPU-side checks of the witness trees' boundary (include/zkw.h): the three functions are declared with C-callable prototypes, the block
inputs did NOT grow for them (a witness tree travels in storage_tree_device), the Python binding types them as the header does, and
libzkw.so exports them."""
import ctypes
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WITNESS_FUNCTIONS = ["zkw_storage_tree_create_witness", "zkw_storage_tree_extract_witness", "zkw_storage_tree_is_witness"]
SIZEOF_BLOCK_INPUTS = 272  # as it was before witness trees: storage_tree_device is still the last member


def test_header_declares_the_witness_functions():
    from era_zkevm_test_harness_amd import native

    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "zkw.h"
    int (*p_create)(zkw_ctx *, const uint8_t *, const uint64_t *, const uint8_t *, const uint8_t *, size_t, const uint8_t *, uint64_t,
                    zkw_storage_tree **) = &zkw_storage_tree_create_witness;
    int (*p_extract)(const zkw_storage_tree *, zkw_ctx *, const uint8_t *, size_t, zkw_storage_tree **) = &zkw_storage_tree_extract_witness;
    int (*p_is)(const zkw_storage_tree *) = &zkw_storage_tree_is_witness;
    int main(void){ printf("%zu %zu\n", sizeof(zkw_block_inputs), offsetof(zkw_block_inputs, storage_tree_device)); return 0; }
    """
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # the addresses are only COMPILED (an assignment of the wrong type is an error); the sizes come from the same header without them
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", os.path.join(d, "t.o"),
                               os.path.join(d, "t.c")])
        open(os.path.join(d, "m.c"), "w").write("\n".join(line for line in src.splitlines() if "(*p_" not in line and "zkw_storage_tree **)" not in line))
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "m"), os.path.join(d, "m.c")])
        size, tree_off = (int(x) for x in subprocess.check_output([os.path.join(d, "m")]).decode().split())
    assert size == SIZEOF_BLOCK_INPUTS == ctypes.sizeof(native.BlockInputs)
    assert tree_off + ctypes.sizeof(ctypes.c_void_p) == size


def test_python_binding_types_the_witness_functions():
    from era_zkevm_test_harness_amd import native

    vp, sz, u64, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int
    want = {"zkw_storage_tree_create_witness": (i, [vp, vp, vp, vp, vp, sz, vp, u64, ctypes.POINTER(vp)]),
            "zkw_storage_tree_extract_witness": (i, [vp, vp, vp, sz, ctypes.POINTER(vp)]),
            "zkw_storage_tree_is_witness": (i, [vp])}
    typed = {name: (res, args) for name, res, args in native.SYMBOLS}
    for name in WITNESS_FUNCTIONS:
        assert name in typed, name
        assert typed[name][0] is want[name][0] and list(typed[name][1]) == want[name][1], name
    for attr in ("from_proofs", "extract_witness", "is_witness"):
        assert hasattr(native.StorageTreeDevice, attr), attr


def test_library_exports_the_witness_symbols():
    from era_zkevm_test_harness_amd import native

    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libzkw.so is not built (build() makes it): nothing to look up")
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in WITNESS_FUNCTIONS:
        assert hasattr(lib, name), f"{name} declared in include/zkw.h but not exported"
