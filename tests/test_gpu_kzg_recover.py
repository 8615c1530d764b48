"""GPU: EIP-7594 recovery (csrc/kzg_recover_kernels.cuh, driver csrc/zkw_kzg.hip) — zkw_kzg_recover_cells_blobs. The expected values come from
three sides that share nothing with the device's route (the vanishing polynomial of the missing cells over a coset): the host model
tests/kzg_recover_model.py (per-cell inverse transforms and Lagrange interpolation), tests/kzg_cells_model.py on the original polynomial, and
the pinned calls zkw_kzg_cells_blobs and zkw_kzg_cell_proofs_blobs. A polynomial of degree below 4 096 through 4 096 points is unique, so
every comparison is byte-exact.

The geometry is fixed by the protocol, so the smallest shape is one blob; the cases are WHICH cells are present (z of degree 64 down to
z = 1, the blob itself present or wholly absent) and which blob. A call without proofs is a few launches; proofs carry FK20's floor, so
three cases ask for them. Every model answer is computed once per module."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import kzg_cells_model as cm
from tests import kzg_model as km
from tests import kzg_open_model as om
from tests import kzg_recover_model as rm

pytestmark = pytest.mark.gpu

R = km.R
N = 4096
EV = 32 * N
CELL = 2048


def index_sets():
    rng = random.Random(7594)
    return {"cells 0..63": list(range(64)), "cells 64..127": list(range(64, 128)), "the even cells": list(range(0, 128, 2)),
            "the odd cells": list(range(1, 128, 2)), "a random 64": sorted(rng.sample(range(128), 64)), "a random 65": sorted(rng.sample(range(128), 65)),
            "a random 100": sorted(rng.sample(range(128), 100)), "127 of 128": [k for k in range(128) if k != 77], "all 128": list(range(128))}


SETS = index_sets()
R64 = SETS["a random 64"]


def monomial(d, c=1):
    p = [0] * N
    p[d] = c
    return p


def blob_coefficients():
    rng = random.Random(7597)
    return {"random": [rng.randrange(R) for _ in range(N)], "pattern": om.blob_coefficients(km.pattern_blob()), "zero": [0] * N,
            "constant": monomial(0, rng.randrange(1, R)), "degree 63": [rng.randrange(R) for _ in range(64)] + [0] * (N - 64), "X^64": monomial(64),
            "X^4095": monomial(4095), "every element r - 1": monomial(0, R - 1), "every coefficient r - 1": [R - 1] * N}


BLOBS = tuple(blob_coefficients())
SPECIAL = BLOBS[2:]


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cell_settings(ctx):
    from era_zkevm_test_harness_amd import native

    s = native.KzgSettings(ctx, km.load_setup_bytes())
    cs = native.KzgCellSettings(s)
    s.free()
    yield cs
    cs.free()


def u8(raw):
    return np.frombuffer(raw, np.uint8)


def pick(cells, idx):
    """the supplied bytes: the cells of the list, in its order"""
    return b"".join(cells[k] for k in idx)


@pytest.fixture(scope="module")
def blobs(ctx):
    """name -> (coefficients, the model's 128 cells, zkw_kzg_cells_blobs of the blob's evaluation form)"""
    from era_zkevm_test_harness_amd import native

    out = {}
    for name, coeffs in blob_coefficients().items():
        cells = cm.cells(coeffs)
        device = native.kzg_cells_blobs(ctx, u8(b"".join(cells[:64])))
        assert device.shape == (1, 128, 2048)
        out[name] = (coeffs, cells, device.tobytes())
    assert b"".join(out["every element r - 1"][1][:64]) == (R - 1).to_bytes(32, "big") * N
    return out


@pytest.fixture(scope="module")
def no_blob():
    """64 cells of seeded random elements below r, and the model's recovery of them: (supplied bytes, the 128 cells, the coefficients)"""
    rng = random.Random(7598)
    supplied = [b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(64)) for _ in R64]
    full, coeffs = rm.recover_cells(R64, supplied)
    return b"".join(supplied), full, coeffs


# ---- which cells are present ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blob", ["random", "pattern"])
@pytest.mark.parametrize("which", list(SETS))
def test_every_set_of_cells_gives_the_blob_back(ctx, blobs, which, blob):
    from era_zkevm_test_harness_amd import native

    _, cells, device = blobs[blob]
    idx = SETS[which]
    got = native.kzg_recover_cells(ctx, idx, u8(pick(cells, idx)))
    assert got.shape == (1, 128, 2048)
    assert got.tobytes() == b"".join(cells)  # kzg_cells_model.cells of the original polynomial
    assert got.tobytes() == device  # zkw_kzg_cells_blobs of the original blob


def test_the_host_model_recovers_the_same(blobs):
    """the model on the sets the device is asked: recovery by the route that shares nothing with the kernels'"""
    coeffs, cells, _ = blobs["random"]
    for which in ("a random 64", "a random 65"):
        assert rm.recover(SETS[which], [cells[k] for k in SETS[which]]) == coeffs


# ---- which blobs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blob", SPECIAL)
def test_special_blobs_from_a_random_64(ctx, blobs, blob):
    from era_zkevm_test_harness_amd import native

    _, cells, device = blobs[blob]
    got = native.kzg_recover_cells(ctx, R64, u8(pick(cells, R64)))
    assert got.tobytes() == b"".join(cells) == device
    if blob == "zero":
        assert got.tobytes() == bytes(2 * EV)


# ---- cells from no blob --------------------------------------------------------------------------------------------------------------------
def test_cells_from_no_blob(ctx, no_blob):
    from era_zkevm_test_harness_amd import native

    supplied, full, coeffs = no_blob
    assert coeffs[N - 1] != 0  # no blob of pubdata: the polynomial has full degree all the same
    got = native.kzg_recover_cells(ctx, R64, u8(supplied))
    assert got.tobytes() == b"".join(full)
    for i, k in enumerate(R64):  # the supplied cells come back unchanged in their places
        assert got[0, k].tobytes() == supplied[CELL * i:CELL * i + CELL]


# ---- proofs --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a random 64", "127 of 128", "no blob"])
def test_proofs_are_those_of_the_recovered_blob(cell_settings, blobs, no_blob, case):
    if case == "no blob":
        supplied, full, coeffs = no_blob
        idx = R64
    else:
        coeffs, full, _ = blobs["random"]
        idx = SETS[case]
        supplied = pick(full, idx)
    assert rm.recover(idx, [supplied[CELL * i:CELL * i + CELL] for i in range(len(idx))]) == coeffs  # the model recovered it
    want_cells, want = cell_settings.cell_proofs_blobs(u8(rm.evaluation_form(coeffs)), cells=True)  # existing, pinned code
    cells, proofs = cell_settings.recover_cells_and_proofs(idx, u8(supplied))
    assert cells.shape == (1, 128, 2048) and proofs.shape == (1, 128, 48)
    assert proofs.tobytes() == want.tobytes() and len({p.tobytes() for p in proofs[0]}) == 128
    assert cells.tobytes() == want_cells.tobytes() == b"".join(full)


# ---- several blobs, no settings, pointer modes ---------------------------------------------------------------------------------------------
THREE = ("random", "X^4095", "every coefficient r - 1")


def test_three_blobs_in_one_call_equal_three_calls(ctx, blobs):
    from era_zkevm_test_harness_amd import native

    idx = SETS["a random 65"]
    supplied = b"".join(pick(blobs[b][1], idx) for b in THREE)
    got = native.kzg_recover_cells(ctx, idx, u8(supplied))  # proofs = NULL with cs = NULL
    assert got.shape == (3, 128, 2048)
    for j, b in enumerate(THREE):
        alone = native.kzg_recover_cells(ctx, idx, u8(pick(blobs[b][1], idx)))
        assert got[j].tobytes() == alone.tobytes() == b"".join(blobs[b][1])


def test_device_pointer_mode_at_odd_addresses(ctx, cell_settings, blobs):
    import torch

    from era_zkevm_test_harness_amd import native

    idx = SETS["a random 65"]
    supplied = b"".join(pick(blobs[b][1], idx) for b in THREE)
    want = b"".join(b"".join(blobs[b][1]) for b in THREE)
    want_proofs = cell_settings.cell_proofs_blobs(u8(b"".join(b"".join(blobs[b][1][:64]) for b in THREE))).tobytes()
    indices = np.array(idx, np.uint8)
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        buf = torch.zeros(len(supplied) + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.from_numpy(u8(supplied).copy()).cuda()
        out_c = torch.zeros(3 * 2 * EV + 1, dtype=torch.uint8, device="cuda")
        out_p = torch.zeros(3 * 128 * 48 + 1, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert (buf.data_ptr() + 1) % 2 == 1
        plain = native.kzg_recover_cells(ctx, idx, buf[1:])
        rc = native.load().zkw_kzg_recover_cells_blobs(cell_settings.handle, ctx.handle, native._np_ptr(indices), len(idx), C.c_void_p(buf.data_ptr() + 1), 3,
                                                       C.c_void_p(out_c.data_ptr() + 1), C.c_void_p(out_p.data_ptr() + 1))
        assert rc == 0, native.load().zkw_last_error().decode()
        ctx.synchronize()
        back = lambda t: t.cpu().numpy().tobytes()
        assert back(plain) == back(out_c[1:]) == want
        assert back(out_p[1:]) == want_proofs
        assert back(out_c[:1]) == b"\0" and back(out_p[:1]) == b"\0"
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_the_arguments_leave_the_outputs_untouched(ctx, cell_settings, blobs):
    from era_zkevm_test_harness_amd import native

    lib, p = native.load(), native._np_ptr
    cells = blobs["random"][1]
    data = u8(b"".join(cells) + cells[0])  # room for 129 cells
    out_c, out_p = np.full(2 * EV, 0xAA, np.uint8), np.full(128 * 48, 0xAA, np.uint8)
    h = cell_settings.handle

    def refused(idx, words, settings=h, proofs=True, n=1):
        indices = np.array(idx, np.uint8)
        rc = lib.zkw_kzg_recover_cells_blobs(settings, ctx.handle, p(indices), len(idx), p(data), n, p(out_c), p(out_p) if proofs else None)
        msg = lib.zkw_last_error().decode()
        assert rc == native.ERR_INVALID and "zkw_kzg_recover_cells_blobs" in msg and all(w in msg for w in words), msg
        assert (out_c == 0xAA).all() and (out_p == 0xAA).all(), idx

    refused(list(range(63)), ["63"])
    refused(list(range(128)) + [128], ["129"])
    refused(list(range(63)) + [128], ["cell_indices[63]", "128"])
    refused(list(range(10)) + [9] + list(range(11, 64)), ["cell_indices[10]", "ascend"])  # a duplicate
    refused(list(range(30)) + [31, 30] + list(range(32, 64)), ["cell_indices[31]", "ascend"])  # a descending pair
    refused(R64, ["settings"], settings=None)  # proofs without settings
    refused(R64, ["32767"], n=32768)
    with pytest.raises(native.ZkwError) as ei:  # the Python layer carries the message
        native.kzg_recover_cells(ctx, list(range(63)), data[:63 * CELL])
    assert ei.value.code == native.ERR_INVALID and "63" in str(ei.value)
    # no blobs: OK, and nothing is written
    indices = np.array(R64, np.uint8)
    assert lib.zkw_kzg_recover_cells_blobs(h, ctx.handle, p(indices), 64, p(data), 0, p(out_c), p(out_p)) == 0
    assert (out_c == 0xAA).all() and (out_p == 0xAA).all()
    assert native.kzg_recover_cells(ctx, R64, np.zeros(0, np.uint8)).shape == (0, 128, 2048)
    got = native.kzg_recover_cells(ctx, R64, u8(pick(cells, R64)))  # (the refusals leave the context usable)
    assert got.tobytes() == b"".join(cells)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("what", ["an element equal to r", "an inconsistent set"])
def test_refusals_by_the_data_leave_the_outputs_untouched_in_both_pointer_modes(ctx, cell_settings, blobs, what, device):
    import torch

    from era_zkevm_test_harness_amd import native

    lib = native.load()
    idx = SETS["a random 65"]
    three = [bytearray(pick(blobs[b][1], idx)) for b in THREE]
    if what == "an element equal to r":  # blob 1: element 5 of list position 40 (and, later in the blob, another one)
        three[1][CELL * 40 + 32 * 5:CELL * 40 + 32 * 6] = R.to_bytes(32, "big")
        three[1][CELL * 64 + 32 * 63:CELL * 64 + 32 * 64] = b"\xff" * 32
        words = ["element 5 of cell_indices[40]", "(cell %d)" % idx[40], "blob 1", "not below r"]
    else:  # blob 1: one element changed by 1
        three[1][CELL * 40 + 32 * 5 + 31] ^= 1
        words = ["blob 1", "do not lie on one polynomial"]
    bad = u8(b"".join(bytes(b) for b in three))
    indices = np.array(idx, np.uint8)
    if device:
        ctx.set_pointer_mode(native.PTR_DEVICE)
        d_bad = torch.from_numpy(bad.copy()).cuda()
        new = lambda n: torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
        ptr, back, src = (lambda t: C.c_void_p(t.data_ptr())), (lambda t: t.cpu().numpy()), d_bad
    else:
        new = lambda n: np.full(n, 0xAA, np.uint8)
        ptr, back, src = native._np_ptr, (lambda a: a), bad
    try:
        cells, proofs = new(3 * 2 * EV), new(3 * 128 * 48)
        if device:
            torch.cuda.synchronize()
        rc = lib.zkw_kzg_recover_cells_blobs(cell_settings.handle, ctx.handle, native._np_ptr(indices), len(idx), ptr(src), 3, ptr(cells), ptr(proofs))
        msg = lib.zkw_last_error().decode()
        ctx.synchronize()
        assert rc == native.ERR_INVALID and "zkw_kzg_recover_cells_blobs" in msg and all(w in msg for w in words), msg
        if what == "an inconsistent set":
            assert "cell_indices[" not in msg  # an inconsistent set has no wrong cell to name
        assert (back(cells) == 0xAA).all() and (back(proofs) == 0xAA).all()
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)
