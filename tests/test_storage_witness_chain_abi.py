"""zkw_storage_tree_advance_witness_chain is part of the public interface: the prototype is in include/zkw.h as the issue states it, the
binding declares it with a matching argument count and offers it on StorageTreeDevice, and the argument errors that need no device — they
are checked before the first HIP call — are return codes. No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "zkw_storage_tree_advance_witness_chain"
PROTOTYPE = ["const zkw_storage_tree *", "zkw_ctx *", "const zkw_log_query *", "const uint64_t *", "size_t", "zkw_storage_tree **", "zkw_storage_tree **"]


def test_prototype_is_in_the_header():
    with open(os.path.join(ROOT, "include", "zkw.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)  # without comments
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, NAME
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    types = [re.sub(r"\s*\b\w+$", "", p) if not p.endswith("*") else p for p in params]  # the parameter's name off
    assert types == PROTOTYPE, types
    # next to zkw_storage_tree_advance_witness_by_queries, ahead of the precompile builders
    assert text.index("zkw_storage_tree_advance_witness_by_queries") < text.index(NAME) < text.index("zkw_storage_tree_is_witness") < text.index("zkw_precompile_witness")


def test_binding_declares_it():
    with open(os.path.join(ROOT, "era_zkevm_test_harness_amd", "native.py")) as f:
        src = f.read()
    m = re.search(r'\("' + NAME + r'",\s*_int,\s*\[(.*)\]\)', src)
    assert m, NAME
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(PROTOTYPE)
    assert m.group(1).strip().endswith("C.POINTER(_vp), C.POINTER(_vp)")  # the K handles and the final table come back through the last two
    from era_zkevm_test_harness_amd import native

    assert callable(native.StorageTreeDevice.advance_chain)


def test_argument_errors_need_no_device():
    from era_zkevm_test_harness_amd import native

    lib = native.load()
    assert hasattr(lib, NAME)
    fn = getattr(lib, NAME)
    out = (C.c_void_p * 2)()
    fake = C.c_void_p(1 << 12)  # never dereferenced: every case below fails on an argument checked before the handles are looked at
    offs = lambda *v: (C.c_uint64 * len(v))(*v)  # noqa: E731
    cases = {
        "null witness": (None, fake, None, offs(0, 0), 1, out, None),
        "null context": (fake, None, None, offs(0, 0), 1, out, None),
        "null offsets": (fake, fake, None, None, 1, out, None),
        "null out": (fake, fake, None, offs(0, 0), 1, None, None),
        "no blocks": (fake, fake, None, offs(0), 0, out, None),
        "offsets do not start at 0": (fake, fake, None, offs(1, 2), 1, out, None),
        "decreasing offsets": (fake, fake, None, offs(0, 5, 3), 2, out, None),
        "queries announced, none given": (fake, fake, None, offs(0, 2, 3), 2, out, None),
    }
    for what, args in cases.items():
        assert fn(*args) == native.ERR_INVALID, what
        assert NAME in lib.zkw_last_error().decode(), what
        assert not out[0] and not out[1], what
