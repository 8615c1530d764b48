"""CPU-side checks of the device-resident storage tree's boundary (include/zkw.h): every function of zkw_storage_tree and
zkw_block_apply_storage is declared with a C-callable prototype, zkw_block_inputs gained storage_tree_device AFTER
queues_on_device (every earlier offset stays), numpy / ctypes agree with the header, and libzkw.so exports the symbols."""
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TREE_FUNCTIONS = ["zkw_storage_tree_create", "zkw_storage_tree_free", "zkw_storage_tree_root", "zkw_storage_tree_next_enumeration_index",
                  "zkw_storage_tree_set_next_enumeration_index", "zkw_storage_tree_num_leaves", "zkw_storage_tree_insert",
                  "zkw_storage_tree_get_leaves", "zkw_storage_tree_answer_queries", "zkw_storage_tree_apply_queries",
                  "zkw_block_apply_storage"]


def _compile_and_run(src):
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        # the addresses are only COMPILED (-c: the typed pointers must accept them; there is no library to link against here) ...
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", os.path.join(d, "t.o"),
                               os.path.join(d, "t.c")])
        # ... and the offsets are printed by the same program without them
        open(os.path.join(d, "m.c"), "w").write(src.replace("TAKE_ADDRESSES 1", "TAKE_ADDRESSES 0"))
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "m"), os.path.join(d, "m.c")])
        return subprocess.check_output([os.path.join(d, "m")]).decode().split()


def test_header_declares_the_tree_and_the_block_field():
    from era_zkevm_test_harness_amd import native

    # the prototypes the issue's table fixes, as a C caller would write them down: an assignment of the wrong type is an error (-Werror)
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "zkw.h"
    #define TAKE_ADDRESSES 1
    #if TAKE_ADDRESSES
    int (*p_create)(zkw_ctx *, size_t, zkw_storage_tree **) = &zkw_storage_tree_create;
    void (*p_free)(zkw_storage_tree *) = &zkw_storage_tree_free;
    int (*p_root)(const zkw_storage_tree *, uint8_t *) = &zkw_storage_tree_root;
    uint64_t (*p_next)(const zkw_storage_tree *) = &zkw_storage_tree_next_enumeration_index;
    int (*p_set_next)(zkw_storage_tree *, uint64_t) = &zkw_storage_tree_set_next_enumeration_index;
    size_t (*p_num)(const zkw_storage_tree *) = &zkw_storage_tree_num_leaves;
    int (*p_insert)(zkw_storage_tree *, const uint8_t *, const uint8_t *, size_t) = &zkw_storage_tree_insert;
    int (*p_get)(const zkw_storage_tree *, const uint8_t *, size_t, uint64_t *, uint8_t *, uint8_t *) = &zkw_storage_tree_get_leaves;
    int (*p_answer)(const zkw_storage_tree *, zkw_ctx *, const zkw_log_query *, size_t, uint64_t *, uint8_t *) = &zkw_storage_tree_answer_queries;
    int (*p_apply)(zkw_storage_tree *, const zkw_log_query *, size_t) = &zkw_storage_tree_apply_queries;
    int (*p_block_apply)(const zkw_block *, zkw_storage_tree *) = &zkw_block_apply_storage;
    #endif
    int main(void){
      zkw_block_inputs in;
      const zkw_storage_tree *t = in.storage_tree_device = NULL;
      (void)t;
      printf("%zu %zu %zu %zu\n", offsetof(zkw_block_inputs, storage_tree_device), offsetof(zkw_block_inputs, queues_on_device),
             sizeof(zkw_block_inputs), offsetof(zkw_block_inputs, storage_tree));
      return 0; }
    """
    tree_off, queues_off, size, cb_off = (int(x) for x in _compile_and_run(src))
    assert tree_off > queues_off
    assert tree_off == native.BlockInputs.storage_tree_device.offset
    assert queues_off == native.BlockInputs.queues_on_device.offset
    assert cb_off == native.BlockInputs.storage_tree.offset
    assert size == ctypes.sizeof(native.BlockInputs)
    assert tree_off + ctypes.sizeof(ctypes.c_void_p) == size  # appended: the last field


def test_python_binding_types_every_tree_function():
    from era_zkevm_test_harness_amd import native

    typed = {name for name, _res, _args in native.SYMBOLS}
    for name in TREE_FUNCTIONS:
        assert name in typed, name
    for attr in ("insert", "get_leaves", "answer_queries", "apply_queries", "root", "next_enumeration_index", "num_leaves", "free"):
        assert hasattr(native.StorageTreeDevice, attr), attr
    assert hasattr(native.Block, "apply_storage")


def test_library_exports_the_tree_symbols():
    from era_zkevm_test_harness_amd import native

    if not os.path.exists(native.LIB_PATH):  # (the library is built by build(); without it there is nothing to look up)
        return
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in TREE_FUNCTIONS:
        assert hasattr(lib, name), f"{name} declared in include/zkw.h but not exported"
