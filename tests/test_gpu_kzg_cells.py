"""GPU: the EIP-7594 cells and cell proofs (csrc/kzg_cell_kernels.cuh, driver csrc/zkw_kzg.hip) — zkw_kzg_cell_settings,
zkw_kzg_cells_blobs, zkw_kzg_cell_proofs_blobs and zkw_eip4844_cell_proofs. Nothing public computes these on this tree's setup, so the
expected values come from algebra, by two routes that share nothing with FK20: on a setup whose tau is known, proof k is
[q_k(tau)] G1 with q_k by synthetic division and q_k(tau) by Horner in Fr (tests/kzg_cells_model.py); on the ceremony's setup the 128
proofs are zkw_kzg_commit of the model's 128 quotient polynomials, a call its own tests pin. A KZG proof is unique, so every comparison
is byte-exact.

The geometry is fixed at 4 096 coefficients, so the small cases are the blob contents: the polynomials whose quotients vanish, X^64 (every
quotient is 1), the monomials at the ends of the Toeplitz vectors of offsets 0 and 63, full-width scalars. Every model answer is computed
once per module."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import kzg_cells_model as cm
from tests import kzg_model as km
from tests import kzg_open_model as om

pytestmark = pytest.mark.gpu

TAU = 0x4844
R = km.R
N = 4096
EV = 32 * N
INF = km.compress(km.INF)


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def settings(ctx):
    from era_zkevm_test_harness_amd import native

    s = native.KzgSettings(ctx, km.load_setup_bytes())
    yield s
    s.free()


@pytest.fixture(scope="module")
def cell_settings(settings):
    from era_zkevm_test_harness_amd import native

    cs = native.KzgCellSettings(settings)
    assert cs.nbytes >= 8192 * 96  # at least the 8 192 points X_i[j]
    yield cs
    cs.free()


@pytest.fixture(scope="module")
def tau_cell_settings(ctx):
    from era_zkevm_test_harness_amd import native

    s = native.KzgSettings(ctx, b"".join(km.compress(p) for p in om.known_tau_setup(TAU, 4096)))
    cs = native.KzgCellSettings(s)
    s.free()  # the cell settings keep nothing of the handle they were made from
    yield cs
    cs.free()


def u8(raw):
    return np.frombuffer(raw, np.uint8)


def evaluation_form(coeffs):
    natural = om._ntt(list(coeffs), om.OMEGA)
    return b"".join(natural[om.brp12(i)].to_bytes(32, "big") for i in range(N))


def monomial(d, c=1):
    p = [0] * N
    p[d] = c
    return p


def case_coefficients():
    rng = random.Random(7594)
    cases = {"zero": [0] * N, "constant": monomial(0, rng.randrange(1, R)), "degree 63": [rng.randrange(R) for _ in range(64)] + [0] * (N - 64),
             "X^64": monomial(64)}
    for d in (4095, 4032, 127, 128, 191):
        cases["X^%d" % d] = monomial(d)
    cases["every element r - 1"] = monomial(0, R - 1)  # the evaluation form of the constant r - 1
    cases["every coefficient r - 1"] = [R - 1] * N
    cases["pattern"] = om.blob_coefficients(km.pattern_blob())
    cases["random"] = [rng.randrange(R) for _ in range(N)]
    return cases


NAMES = tuple(case_coefficients())
assert len(NAMES) == 13


@pytest.fixture(scope="module")
def cases():
    """name -> (coefficients lowest first, evaluation form)"""
    out = {name: (coeffs, evaluation_form(coeffs)) for name, coeffs in case_coefficients().items()}
    assert out["every element r - 1"][1] == (R - 1).to_bytes(32, "big") * N
    return out


@pytest.fixture(scope="module")
def tau_results(tau_cell_settings, cases):
    """name -> (cells, proofs) by zkw_kzg_cell_proofs_blobs on the known-tau setup, each blob in a call of its own"""
    out = {}
    for name, (_, ev) in cases.items():
        cells, proofs = tau_cell_settings.cell_proofs_blobs(u8(ev), cells=True)
        assert cells.shape == (1, 128, 2048) and proofs.shape == (1, 128, 48)
        out[name] = (cells[0].tobytes(), [p.tobytes() for p in proofs[0]])
    return out


# ---- (a) a setup whose tau is known: [q_k(tau)] G1 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_proofs_on_a_known_tau_setup(cases, tau_results, name):
    coeffs = cases[name][0]
    want = [cm.cell_proof_by_tau(coeffs, k, TAU) for k in range(128)]
    if name in ("zero", "constant", "degree 63", "every element r - 1"):
        assert want == [INF] * 128  # nothing to divide
    if name == "X^64":
        assert want == [km.load_setup_bytes()[:48]] * 128  # every quotient is 1: S[0], the generator
    assert tau_results[name][1] == want


# ---- (c) the cells ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cells_are_the_extended_evaluations(ctx, cases, tau_results, name):
    from era_zkevm_test_harness_amd import native

    coeffs, ev = cases[name]
    want = b"".join(cm.cells(coeffs))
    assert want[:EV] == ev  # cells 0..63 are the input, byte for byte
    assert tau_results[name][0] == want
    if name == "zero":
        assert want == bytes(2 * EV)
    if name in ("constant", "X^191", "random"):  # the call without settings
        got = native.kzg_cells_blobs(ctx, u8(ev))
        assert got.shape == (1, 128, 2048) and got.tobytes() == want


# ---- (b) the ceremony's setup: the commitments of the 128 quotient polynomials ------------------------------------------------------------
@pytest.mark.parametrize("name", ["pattern", "random"])
def test_proofs_on_the_ceremony_setup_are_the_commitments_of_the_quotients(settings, cell_settings, cases, name):
    coeffs, ev = cases[name]
    rows = b"".join(c.to_bytes(32, "little") for q in cm.quotients(coeffs) for c in q)
    want = settings.commit(u8(rows), 4032)
    assert want.shape == (128, 48) and len({w.tobytes() for w in want}) == 128
    got = cell_settings.cell_proofs_blobs(u8(ev))
    assert got.shape == (1, 128, 48) and got[0].tobytes() == want.tobytes()


# ---- (d) the pubdata form -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pubdata(settings, cell_settings):
    """(two pubdata blobs, their evaluation forms by zkw_eip4844_prove, (cells, proofs) of zkw_kzg_cell_proofs_blobs on those)"""
    blobs = u8(km.pattern_blob() + random.Random(7596).randbytes(km.BLOB_BYTES))
    rec = settings.eip4844_witness(blobs)
    _, ev = settings.eip4844_prove(blobs, rec, evaluations=True)
    return blobs, ev, cell_settings.cell_proofs_blobs(ev, cells=True)


def test_the_pubdata_call_equals_the_evaluation_form_call(cell_settings, cases, pubdata):
    blobs, ev, (want_cells, want_proofs) = pubdata
    assert ev[0].tobytes() == cases["pattern"][1]
    cells, proofs = cell_settings.eip4844_cell_proofs(blobs, cells=True)
    assert proofs.shape == (2, 128, 48) and proofs.tobytes() == want_proofs.tobytes()
    assert cells.shape == (2, 128, 2048) and cells.tobytes() == want_cells.tobytes()
    assert cells[:, :64].tobytes() == ev.tobytes()
    assert cell_settings.eip4844_cell_proofs(blobs).tobytes() == want_proofs.tobytes()  # cells == NULL


# ---- (e) (f) (g) batching, cells == NULL, pointer modes -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(cases, tau_results):
    names = ("random", "X^127", "every coefficient r - 1")
    return b"".join(cases[n][1] for n in names), b"".join(tau_results[n][0] for n in names), b"".join(b"".join(tau_results[n][1]) for n in names)


def test_three_blobs_in_one_call_equal_three_calls_and_cells_may_be_null(ctx, tau_cell_settings, three):
    from era_zkevm_test_harness_amd import native

    evs, want_cells, want_proofs = three
    cells, proofs = tau_cell_settings.cell_proofs_blobs(u8(evs), cells=True)
    assert proofs.tobytes() == want_proofs and cells.tobytes() == want_cells
    assert tau_cell_settings.cell_proofs_blobs(u8(evs)).tobytes() == want_proofs
    assert native.kzg_cells_blobs(ctx, u8(evs)).tobytes() == want_cells


def test_device_pointer_mode_at_an_odd_address(ctx, tau_cell_settings, cell_settings, three, pubdata):
    import torch

    from era_zkevm_test_harness_amd import native

    evs, want_cells, want_proofs = three
    blobs, _, (pub_cells, pub_proofs) = pubdata
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        buf = torch.zeros(3 * EV + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.from_numpy(u8(evs).copy()).cuda()
        d_blobs = torch.from_numpy(blobs.copy()).cuda()
        torch.cuda.synchronize()
        assert (buf.data_ptr() + 1) % 2 == 1
        cells, proofs = tau_cell_settings.cell_proofs_blobs(buf[1:], cells=True)
        only = tau_cell_settings.cell_proofs_blobs(buf[1:])
        alone = native.kzg_cells_blobs(ctx, buf[1:])
        c2, p2 = cell_settings.eip4844_cell_proofs(d_blobs, cells=True)
        # outputs at an odd address too
        out_c = torch.zeros(3 * 2 * EV + 1, dtype=torch.uint8, device="cuda")
        out_p = torch.zeros(3 * 128 * 48 + 1, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = native.load().zkw_kzg_cell_proofs_blobs(tau_cell_settings.handle, ctx.handle, C.c_void_p(buf.data_ptr() + 1), 3, C.c_void_p(out_c.data_ptr() + 1),
                                                     C.c_void_p(out_p.data_ptr() + 1))
        assert rc == 0, native.load().zkw_last_error().decode()
        ctx.synchronize()
        back = lambda t: t.cpu().numpy().tobytes()
        assert back(proofs) == back(only) == back(out_p[1:]) == want_proofs
        assert back(cells) == back(alone) == back(out_c[1:]) == want_cells
        assert back(c2) == pub_cells.tobytes() and back(p2) == pub_proofs.tobytes()
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


# ---- (h) refusals -------------------------------------------------------------------------------------------------------------------------
def with_elements(blob, changes):
    b = bytearray(blob)
    for i, v in changes.items():
        b[32 * i:32 * i + 32] = int(v).to_bytes(32, "big")
    return bytes(b)


@pytest.mark.parametrize("device", [False, True])
def test_an_element_equal_to_r_is_refused_by_name_and_the_outputs_stay_untouched(ctx, tau_cell_settings, cases, device):
    import torch

    from era_zkevm_test_harness_amd import native

    lib = native.load()
    good = cases["random"][1]
    bad = good + with_elements(good, {77: R, 4095: (1 << 256) - 1})
    if device:
        ctx.set_pointer_mode(native.PTR_DEVICE)
        d_bad = torch.from_numpy(u8(bad).copy()).cuda()
        new = lambda n: torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
        ptr, back, src = (lambda t: C.c_void_p(t.data_ptr())), (lambda t: t.cpu().numpy()), d_bad
        torch.cuda.synchronize()
    else:
        new = lambda n: np.full(n, 0xAA, np.uint8)
        ptr, back, src = native._np_ptr, (lambda a: a), u8(bad)
    try:
        cells, proofs = new(2 * 2 * EV), new(2 * 128 * 48)
        if device:
            torch.cuda.synchronize()
        for name, call in (("zkw_kzg_cell_proofs_blobs", lambda: lib.zkw_kzg_cell_proofs_blobs(tau_cell_settings.handle, ctx.handle, ptr(src), 2, ptr(cells), ptr(proofs))),
                           ("zkw_kzg_cells_blobs", lambda: lib.zkw_kzg_cells_blobs(ctx.handle, ptr(src), 2, ptr(cells)))):
            rc = call()
            msg = lib.zkw_last_error().decode()
            ctx.synchronize()
            assert rc == native.ERR_INVALID and name in msg and "element 77 of blob 1" in msg and "not below r" in msg, msg
            assert (back(cells) == 0xAA).all() and (back(proofs) == 0xAA).all(), name
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


def test_short_settings_too_many_blobs_and_no_blobs(ctx, settings, tau_cell_settings, cases, tau_results):
    from era_zkevm_test_harness_amd import native

    short = native.KzgSettings(ctx, km.load_setup_bytes()[:48 * 8])
    try:
        with pytest.raises(native.ZkwError) as ei:
            native.KzgCellSettings(short)
        assert ei.value.code == native.ERR_INVALID and "8 points" in str(ei.value)
    finally:
        short.free()
    lib, p = native.load(), native._np_ptr
    one = u8(cases["random"][1])
    cells, proofs = np.full(64, 0xAA, np.uint8), np.full(64, 0xAA, np.uint8)
    h = tau_cell_settings.handle
    for rc in (lib.zkw_kzg_cells_blobs(ctx.handle, p(one), 32768, p(cells)), lib.zkw_kzg_cell_proofs_blobs(h, ctx.handle, p(one), 32768, p(cells), p(proofs)),
               lib.zkw_eip4844_cell_proofs(h, ctx.handle, p(one), 32768, p(cells), p(proofs))):
        assert rc == native.ERR_INVALID and "32767" in lib.zkw_last_error().decode()
    # no blobs: OK, and nothing is written
    assert lib.zkw_kzg_cells_blobs(ctx.handle, p(one), 0, p(cells)) == 0
    assert lib.zkw_kzg_cell_proofs_blobs(h, ctx.handle, p(one), 0, p(cells), p(proofs)) == 0
    assert lib.zkw_eip4844_cell_proofs(h, ctx.handle, p(one), 0, p(cells), p(proofs)) == 0
    assert (cells == 0xAA).all() and (proofs == 0xAA).all()
    none = np.zeros(0, np.uint8)
    assert native.kzg_cells_blobs(ctx, none).shape == (0, 128, 2048) and tau_cell_settings.cell_proofs_blobs(none).shape == (0, 128, 48)
    got = tau_cell_settings.cell_proofs_blobs(one)  # (the refusals leave the context usable)
    assert [r.tobytes() for r in got[0]] == tau_results["random"][1]


# ---- (i) the handle -----------------------------------------------------------------------------------------------------------------------
def test_the_handle_keeps_its_context_and_a_freed_handle_leaves_it_usable(ctx, settings, cell_settings, cases):
    from era_zkevm_test_harness_amd import native

    assert cell_settings.nbytes > 0
    ev = u8(cases["pattern"][1])
    want = cell_settings.cell_proofs_blobs(ev).tobytes()
    other = native.Context(0)
    cs = native.KzgCellSettings(settings, ctx=other)
    assert cs.nbytes == cell_settings.nbytes
    other.close()  # the handle retains it
    assert cs.cell_proofs_blobs(ev, ctx=ctx).tobytes() == want  # from another context of the device
    cs.free()
    assert cs.nbytes == 0
    mine = native.KzgCellSettings(settings)
    mine.free()
    assert cell_settings.cell_proofs_blobs(ev).tobytes() == want  # the context outlives a handle made on it
