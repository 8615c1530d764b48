"""The host model of EIP-7594 recovery (tests/kzg_recover_model.py) against tests/kzg_cells_model.py (drop cells of a known blob, recover,
equal), the model against the host restatement of the device's route (the vanishing polynomial over a coset: its index arithmetic —
brp6(i' >> 6), the W table read backwards, the fold constants — is on record here before a kernel runs), the constants of
csrc/kzg_recover_kernels.cuh against their definitions, and the boundary: include/zkw.h declares zkw_kzg_recover_cells_blobs with the
documented prototype, the library exports it and the Python layer has it. No GPU."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from tests import kzg_cells_model as cm
from tests import kzg_model as km
from tests import kzg_open_model as om
from tests import kzg_recover_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = km.R


def index_sets():
    rng = random.Random(7594)
    return {"cells 0..63": list(range(64)), "cells 64..127": list(range(64, 128)), "the even cells": list(range(0, 128, 2)),
            "the odd cells": list(range(1, 128, 2)), "a random 64": sorted(rng.sample(range(128), 64)), "a random 65": sorted(rng.sample(range(128), 65)),
            "a random 100": sorted(rng.sample(range(128), 100)), "127 of 128": [k for k in range(128) if k != 77], "all 128": list(range(128))}


SETS = index_sets()


@pytest.fixture(scope="module")
def blob():
    """(coefficients lowest first, the model's cells) of a seeded random blob"""
    coeffs = om.blob_coefficients(random.Random(7595).randbytes(km.BLOB_BYTES))
    return coeffs, cm.cells(coeffs)


@pytest.mark.parametrize("name", list(SETS))
def test_both_routes_recover_a_known_blob(blob, name):
    coeffs, cells = blob
    idx = SETS[name]
    supplied = [cells[k] for k in idx]
    assert rm.recover(idx, supplied) == coeffs
    assert rm.vanishing_route(idx, supplied) == coeffs


def test_the_routes_agree_on_cells_from_no_blob():
    """64 cells of arbitrary elements below r: every such set is consistent, the polynomial has full degree"""
    rng = random.Random(7596)
    idx = SETS["a random 64"]
    supplied = [b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(64)) for _ in idx]
    full, coeffs = rm.recover_cells(idx, supplied)
    assert coeffs[4095] != 0 and [full[k] for k in idx] == supplied
    assert rm.vanishing_route(idx, supplied) == coeffs


def test_an_inconsistent_set_is_refused_and_has_no_wrong_cell(blob):
    coeffs, cells = blob
    idx = SETS["a random 65"]
    supplied = [bytearray(cells[k]) for k in idx]
    supplied[40][5 * 32 + 31] ^= 1  # one element of one cell changed by 1
    supplied = [bytes(c) for c in supplied]
    with pytest.raises(rm.Inconsistent):
        rm.recover(idx, supplied)
    # what the device compares: the cells of the polynomial the vanishing route gives. Every supplied cell differs from them
    again = cm.cells(rm.vanishing_route(idx, supplied))
    assert all(again[k] != c for k, c in zip(idx, supplied))
    # (the route itself interpolates E Z, of degree up to 8 191 here, and its quotient by Z has no remainder only on a consistent set)


def test_the_vanishing_values_and_the_index_arithmetic():
    for name in ("cells 0..63", "a random 64", "127 of 128", "all 128"):
        slot = rm.slot_table(SETS[name])
        zc, zinv = rm.vanishing_values(slot)
        missing = [k for k in range(128) if slot[k] == rm.ABSENT]
        assert [k for k in range(128) if zc[k] == 0] == missing

        def z_at(y):  # the product itself
            v = 1
            for k in missing:
                v = v * (y - cm.cell_constant(k)) % R
            return v

        assert all(zc[k] == z_at(cm.cell_constant(k)) for k in (0, 1, 64, 127))
        for e in (0, 1, 63, 64, 4095):  # Z at the coset point s w^e is inverse number e mod 64
            x = rm.SHIFT * pow(om.OMEGA, e, R) % R
            assert zinv[e % 64] * z_at(pow(x, 64, R)) % R == 1
    assert pow(rm.SHIFT, 8192, R) != 1
    for i in (0, 1, 63, 64, 4095):  # position i' of a forward transform holds the point w^brp12(i'), and brp12(i') mod 64 = brp6(i' >> 6)
        assert om.brp12(i) % 64 == cm.brp(i >> 6, 6)
    for i in (1, 2, 4095):  # W^-i = -W^(4096 - i)
        assert pow(cm.W, R - 1 - i, R) == R - pow(cm.W, 4096 - i, R)


def test_the_device_constants_are_their_definitions():
    text = open(os.path.join(ROOT, "era_zkevm_test_harness_amd", "csrc", "kzg_recover_kernels.cuh")).read()
    for name, value in rm.device_constants().items():
        m = re.search(r"bls::Fr %s\(\) \{\s*return bls::Fr\{\{([^}]*)\}\};" % name, text)
        assert m, name
        assert [int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")] == rm.montgomery_words(value), name
    a, b = rm.device_constants()["kzg_recover_fold_a"], rm.device_constants()["kzg_recover_fold_b"]
    assert (a + b) * 4096 * 4096 % R == 1 and (a - b) * 4096 * 4096 % R == pow(rm.SHIFT, 4096, R)
    assert rm.device_constants()["kzg_recover_s_inv"] * rm.SHIFT % R == 1


def test_prototype(tmp_path):
    src = r"""
    #include <stddef.h>
    #include "zkw.h"
    /* assigning to a pointer of the documented type fails to compile if the prototype differs */
    int (*p_recover)(const zkw_kzg_cell_settings *, zkw_ctx *, const uint8_t *, size_t, const uint8_t *, size_t, uint8_t *, uint8_t *) = zkw_kzg_recover_cells_blobs;
    int main(void){ return !p_recover; }
    """
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(tmp_path / "t.c")])
    from era_zkevm_test_harness_amd import build

    lib = build.build()
    subprocess.check_call(["gcc", "-o", str(tmp_path / "t"), str(tmp_path / "t.o"), lib, f"-Wl,-rpath,{os.path.dirname(lib)}", "-Wl,--allow-shlib-undefined"])
    subprocess.check_call([str(tmp_path / "t")])


def test_library_exports_the_symbol_and_python_has_the_entry_points():
    from era_zkevm_test_harness_amd import build, native

    lib = ctypes.CDLL(build.build())
    signatures = {n: (res, args) for n, res, args in native.SYMBOLS}
    assert hasattr(lib, "zkw_kzg_recover_cells_blobs")
    assert len(signatures["zkw_kzg_recover_cells_blobs"][1]) == 8
    assert callable(native.kzg_recover_cells) and callable(native.KzgCellSettings.recover_cells_and_proofs)


def test_the_docs_no_longer_say_recovery_is_not_offered():
    for path in ("include/zkw.h", "README.md", "docs/KERNELS.md", "era_zkevm_test_harness_amd/native.py"):
        text = open(os.path.join(ROOT, path)).read()
        assert "zkw_kzg_recover_cells_blobs" in text, path
        for line in text.splitlines():
            if "ot offered" in line:
                assert "recovery from half" not in line, (path, line)
