"""GPU: the verification of EIP-7594 cell proofs (csrc/kzg_cell_verify_kernels.cuh, driver csrc/zkw_kzg.hip) — zkw_kzg_verify_cells and
zkw_kzg_commit_cells. The claims live on a setup whose tau is known, so that [tau^64] G2 exists (tests/kzg_pairing_model.py: g2_mul): the
commitment is [p(tau)] G1 by the host, cells and proofs are the device's own zkw_kzg_cell_proofs_blobs (pinned by tests/test_gpu_kzg_cells.py),
and a claim is true or false by construction. Three sides that share nothing with the kernels' route say the same: the host model
tests/kzg_cell_verify_model.py (interpolation and a host pairing per claim), zkw_kzg_verify on the same verifier with the commitment of
C - [I_k] G1 made on the host, and for the interpolation commitment alone zkw_kzg_commit over the model's 64 coefficients on the ceremony's
setup.

The geometry is fixed by the protocol, so the small cases are contents and counts: 8 claims share a wave in k_kzg_verify_pairing, 64 a wave
in k_kzg_verify_cell_points and 4 a workgroup in k_kzg_cell_interpolate. A call is a few launches."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import kzg_cell_verify_model as vm
from tests import kzg_cells_model as cm
from tests import kzg_model as km
from tests import kzg_open_model as om
from tests import kzg_pairing_model as pm

pytestmark = pytest.mark.gpu

TAU = 0x4844
R, P = km.R, km.P
N = 4096
CELL = 2048
INF = km.compress(km.INF)
FAILS, HOLDS, BAD_COMMITMENT, BAD_PROOF, BAD_SCALAR, BAD_INDEX = range(6)


def u8(raw):
    return np.frombuffer(raw, np.uint8)


def monomial(d, c=1):
    p = [0] * N
    p[d] = c
    return p


def blob_coefficients():
    rng = random.Random(7594_36)
    return {"A": [rng.randrange(R) for _ in range(N)], "B": [rng.randrange(R) for _ in range(N)], "C": [rng.randrange(R) for _ in range(N)],
            "constant": monomial(0, rng.randrange(1, R)), "degree 63": [rng.randrange(R) for _ in range(64)] + [0] * (N - 64), "X^64": monomial(64),
            "zero": [0] * N, "every element r - 1": monomial(0, R - 1)}


SPECIAL = ("constant", "degree 63", "X^64", "zero", "every element r - 1")


def evaluation_form(coeffs):
    natural = om._ntt(list(coeffs), om.OMEGA)
    return b"".join(natural[om.brp12(i)].to_bytes(32, "big") for i in range(N))


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tau_points():
    return om.known_tau_setup(TAU, N)


@pytest.fixture(scope="module")
def tau_settings(ctx, tau_points):
    from era_zkevm_test_harness_amd import native

    s = native.KzgSettings(ctx, b"".join(km.compress(p) for p in tau_points))
    yield s
    s.free()


@pytest.fixture(scope="module")
def v64(ctx):
    from era_zkevm_test_harness_amd import native

    v = native.KzgVerifier(ctx, vm.tau64_g2(TAU)[1])
    yield v
    v.free()


@pytest.fixture(scope="module")
def blobs(tau_settings):
    """name -> (coefficients, commitment, the 128 cells, the 128 proofs): the commitment [p(tau)] G1 by the host, cells and proofs by
    zkw_kzg_cell_proofs_blobs on the known-tau setup"""
    from era_zkevm_test_harness_amd import native

    cs = native.KzgCellSettings(tau_settings)
    out = {}
    try:
        for name, coeffs in blob_coefficients().items():
            cells, proofs = cs.cell_proofs_blobs(u8(evaluation_form(coeffs)), cells=True)
            out[name] = (coeffs, km.compress(vm.g1_of(cm.evaluate(coeffs, TAU))), [c.tobytes() for c in cells[0]], [p.tobytes() for p in proofs[0]])
    finally:
        cs.free()
    return out


def claim(blobs, name, k, cell_of=None, proof_of=None, commitment_of=None):
    """(commitment, index, cell, proof): cell k of blob `name`, with parts of the claim taken from elsewhere"""
    _, c, cells, proofs = blobs[name]
    return (blobs[commitment_of][1] if commitment_of else c, k, cells[k if cell_of is None else cell_of], proofs[k if proof_of is None else proof_of])


def run(verifier, settings, claims, ctx=None):
    out = verifier.verify_cells(settings, u8(b"".join(c[0] for c in claims)), np.array([c[1] for c in claims], np.uint64), u8(b"".join(c[2] for c in claims)),
                                u8(b"".join(c[3] for c in claims)), ctx=ctx)
    assert out.shape == (len(claims),) and out.dtype == np.uint8
    return [int(x) for x in out]


def model(claim_, tau64=None):
    c, k, cell, proof = claim_
    tau64 = vm.tau64_g2(TAU)[0] if tau64 is None else tau64
    return vm.verify_cell(km.decompress(c, check_subgroup=False), k, cell, km.decompress(proof, check_subgroup=False), tau64, tau=TAU)


# ---- true claims ---------------------------------------------------------------------------------------------------------------------------
def test_all_128_cells_of_a_blob_in_one_call(v64, tau_settings, blobs):
    claims = [claim(blobs, "A", k) for k in range(128)]
    assert len({c[3] for c in claims}) == 128
    assert run(v64, tau_settings, claims) == [HOLDS] * 128
    assert model(claims[77])


@pytest.mark.parametrize("n", [1, 8, 9, 64, 65])
def test_lane_and_wave_edges(v64, tau_settings, blobs, n):
    """true claims with a false one (the proof of the next cell) at every seventh place: no period of 4, 8 or 64"""
    claims = [claim(blobs, "A", (3 * i) % 128, proof_of=(3 * i + 1) % 128 if i % 7 == 3 else None) for i in range(n)]
    assert run(v64, tau_settings, claims) == [FAILS if i % 7 == 3 else HOLDS for i in range(n)]


def test_three_blobs_by_four_columns_equal_twelve_calls(v64, tau_settings, blobs):
    claims = [claim(blobs, name, k) for name in ("A", "B", "C") for k in (0, 31, 64, 127)]
    together = run(v64, tau_settings, claims)
    assert together == [HOLDS] * 12
    assert [run(v64, tau_settings, [c])[0] for c in claims] == together


@pytest.mark.parametrize("name", SPECIAL)
def test_degenerate_polynomials(v64, tau_settings, blobs, name):
    coeffs, c, cells, proofs = blobs[name]
    ks = (0, 1, 77, 127)
    if name in ("constant", "degree 63", "zero", "every element r - 1"):
        assert all(proofs[k] == INF for k in ks)  # nothing to divide: pi = O
    if name == "X^64":
        assert all(proofs[k] == km.compress(pm.g1_gen()) for k in ks)  # q_k = 1
        assert vm.interpolant(77, cells[77]) == [cm.cell_constant(77)] + [0] * 63  # I_k = c_k
    if name == "degree 63":
        assert vm.interpolant(77, cells[77]) == coeffs[:64]  # I_k = p
    if name == "zero":
        assert c == INF and cells[77] == bytes(CELL)
    if name == "every element r - 1":
        assert cells[77] == (R - 1).to_bytes(32, "big") * 64
    assert run(v64, tau_settings, [claim(blobs, name, k) for k in ks]) == [HOLDS] * 4


# ---- false claims --------------------------------------------------------------------------------------------------------------------------
def test_false_claims(ctx, v64, tau_settings, blobs):
    from era_zkevm_test_harness_amd import native

    true = claim(blobs, "A", 77)
    tampered = bytearray(true[2])
    tampered[32 * 9 + 31] ^= 1
    false = [(true[0], 77, bytes(tampered), true[3]),        # one byte of one cell element changed
             claim(blobs, "A", 77, proof_of=5),                # cell k with the proof of cell k'
             claim(blobs, "A", 5, cell_of=77, proof_of=77),    # the right cell and proof under index k'
             claim(blobs, "A", 77, commitment_of="B")]         # the commitment of another blob
    assert run(v64, tau_settings, [true] + false + [true]) == [HOLDS] + [FAILS] * 4 + [HOLDS]
    assert model(true) and [model(f) for f in false] == [False] * 4  # the host model agrees on every one of them
    # a true claim against a verifier built from [tau] G2 instead of [tau^64] G2
    v1 = native.KzgVerifier(ctx, pm.g2_compress(pm.g2_mul(TAU, pm.G2_GEN)))
    try:
        assert run(v1, tau_settings, [true, claim(blobs, "B", 0)]) == [FAILS, FAILS]
        assert not model(true, tau64=pm.g2_mul(TAU, pm.G2_GEN))
    finally:
        v1.free()


# ---- codes ---------------------------------------------------------------------------------------------------------------------------------
def outside_g1():
    """an on-curve point outside the order-r subgroup"""
    x = 1
    while True:
        y = km.sqrt_fq((x ** 3 + km.B) % P)
        if y is not None and km.mul_naive(R, (x, y)) is not km.INF:
            return km.compress((x, y))
        x += 1


def not_on_curve():
    x = 1
    while km.sqrt_fq((x ** 3 + km.B) % P) is not None:
        x += 1
    return bytes([0x80]) + x.to_bytes(47, "big")


def with_element(cell, t, value):
    return cell[:32 * t] + value.to_bytes(32, "big") + cell[32 * t + 32:]


def test_codes(v64, tau_settings, blobs):
    c, k, cell, proof = claim(blobs, "A", 77)
    good = (c, k, cell, proof)
    r_at_63 = with_element(cell, 63, R)
    claims = [good,
              (not_on_curve(), k, cell, proof),                       # 2
              good,
              (c, k, cell, outside_g1()),                             # 3
              (c, k, with_element(cell, 0, R), proof),                # 4
              (c, k, r_at_63, proof),                                 # 4 (the last lane's element)
              (c, k, with_element(cell, 31, (1 << 256) - 1), proof),  # 4
              (c, 128, cell, proof),                                  # 5
              (c, 1 << 32, cell, proof),                              # 5: the upper word is read (the lower one is 0, a valid index)
              (c, (1 << 32) + 77, cell, proof),                       # 5
              (c, (1 << 64) - 1, cell, proof),                        # 5
              good,
              (not_on_curve(), 128, r_at_63, outside_g1()),           # every rule broken: the lowest code
              (c, 128, r_at_63, outside_g1()),                        # 3
              (c, 128, r_at_63, proof),                               # 4
              (bytes([c[0] & 0x7F]) + c[1:], k, cell, proof),         # 2: not a compressed point
              good]
    want = [HOLDS, BAD_COMMITMENT, HOLDS, BAD_PROOF, BAD_SCALAR, BAD_SCALAR, BAD_SCALAR, BAD_INDEX, BAD_INDEX, BAD_INDEX, BAD_INDEX, HOLDS, BAD_COMMITMENT,
            BAD_PROOF, BAD_SCALAR, BAD_COMMITMENT, HOLDS]
    assert run(v64, tau_settings, claims) == want  # (a bad claim between good ones leaves its neighbours' verdicts 1)
    assert claim(blobs, "A", 0)[1] == 0 and run(v64, tau_settings, [claim(blobs, "A", 0)]) == [HOLDS]  # index 0 itself is a good one


# ---- a second device route -------------------------------------------------------------------------------------------------------------------
def test_the_verdicts_equal_zkw_kzg_verify_on_the_reduced_claims(v64, tau_settings, blobs):
    """the claim is "C - [I_k] G1 opens to 0 at c_k" under [tau^64] G2: zkw_kzg_verify on the same verifier, the commitment made on the host"""
    tampered = bytearray(blobs["A"][2][9])
    tampered[31] ^= 1  # (the lowest bit of element 0)
    assert int.from_bytes(tampered[:32], "big") < R
    claims = [claim(blobs, "A", 0), claim(blobs, "A", 1), claim(blobs, "A", 64, proof_of=65), claim(blobs, "B", 127), claim(blobs, "A", 9, commitment_of="B"),
              claim(blobs, "X^64", 77), claim(blobs, "zero", 3), (blobs["A"][1], 9, bytes(tampered), blobs["A"][3][9]), claim(blobs, "C", 100),
              claim(blobs, "degree 63", 100, proof_of=None)]
    got = run(v64, tau_settings, claims)
    assert got == [HOLDS, HOLDS, FAILS, HOLDS, FAILS, HOLDS, HOLDS, FAILS, HOLDS, HOLDS]
    reduced = [km.compress(km.add(km.decompress(c, check_subgroup=False), km.neg(vm.interpolant_commitment(k, cell, tau=TAU)))) for c, k, cell, _ in claims]
    le = lambda vs: u8(b"".join(int(v).to_bytes(32, "little") for v in vs))
    other = v64.verify(u8(b"".join(reduced)), le([cm.cell_constant(k) for _, k, _, _ in claims]), le([0] * len(claims)), u8(b"".join(c[3] for c in claims)))
    assert [int(x) for x in other] == got


# ---- zkw_kzg_commit_cells --------------------------------------------------------------------------------------------------------------------
def random_cells(seed, n):
    """cells of no blob: any 64 elements below r have an interpolant"""
    rng = random.Random(seed)
    return [b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(64)) for _ in range(n)]


def test_commit_cells_on_the_known_tau_setup(tau_settings, blobs):
    ks = [0, 1, 64, 77, 127, 5, 77]
    cells = [blobs["A"][2][k] for k in ks[:5]] + [blobs["zero"][2][5], blobs["X^64"][2][77]]
    got = tau_settings.commit_cells(np.array(ks, np.uint64), u8(b"".join(cells)))
    assert got.shape == (7, 48)
    want = [km.compress(km.mul_naive(cm.evaluate(vm.interpolant(k, cell), TAU), pm.g1_gen())) for k, cell in zip(ks, cells)]
    assert [g.tobytes() for g in got] == want
    assert want[5] == INF and want[6] == km.compress(vm.g1_of(cm.cell_constant(77)))


def test_commit_cells_on_the_ceremony_setup_equals_commit_of_the_model_coefficients(ctx):
    from era_zkevm_test_harness_amd import native

    ks = [0, 1, 64, 77, 127, 100]
    cells = random_cells(64, 5) + [bytes(CELL)]
    rows = b"".join(b"".join(a.to_bytes(32, "little") for a in vm.interpolant(k, cell)) for k, cell in zip(ks, cells))
    full = native.KzgSettings(ctx, km.load_setup_bytes())
    short = native.KzgSettings(ctx, km.load_setup_bytes()[:64 * 48])
    try:
        assert short.num_points == 64 and short.nbytes < 200 * 1024
        want = full.commit(u8(rows), 64)
        got = full.commit_cells(np.array(ks, np.uint64), u8(b"".join(cells)))
        assert got.tobytes() == want.tobytes() and got[5].tobytes() == INF
        assert short.commit_cells(np.array(ks, np.uint64), u8(b"".join(cells))).tobytes() == want.tobytes()  # a handle of exactly 64 points
        first64 = [km.decompress(km.load_setup_bytes()[48 * i:48 * i + 48], check_subgroup=False) for i in range(64)]
        assert got[3].tobytes() == km.compress(vm.interpolant_commitment(77, cells[3], points=first64))  # and the model's sum over the same 64 points
    finally:
        full.free()
        short.free()


@pytest.mark.parametrize("device", [False, True])
def test_commit_cells_refuses_by_name_and_leaves_out_untouched(ctx, tau_settings, device):
    import torch

    from era_zkevm_test_harness_amd import native

    lib = native.load()
    cells = random_cells(65, 6)
    bad_element = list(cells)
    bad_element[4] = with_element(with_element(cells[4], 9, R), 40, (1 << 256) - 1)
    cases = [(bad_element, [0, 1, 2, 3, 4, 5], ["element 9 of cells[4]", "not below r"]), (cells, [0, 1, 128, 3, 4, 5], ["cell_indices[2]", "128"]),
             (cells, [0, 1, 2, 3, 4, 1 << 32], ["cell_indices[5]", "128"])]
    if device:
        ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        for data, idx, words in cases:
            raw, indices = u8(b"".join(data)), np.array(idx, np.uint64)
            if device:
                d_raw, d_idx = torch.from_numpy(raw.copy()).cuda(), torch.from_numpy(indices.view(np.int64).copy()).cuda()
                out = torch.full((6 * 48,), 0xAA, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                rc = lib.zkw_kzg_commit_cells(tau_settings.handle, ctx.handle, C.c_void_p(d_idx.data_ptr()), C.c_void_p(d_raw.data_ptr()), 6, C.c_void_p(out.data_ptr()))
            else:
                out = np.full(6 * 48, 0xAA, np.uint8)
                rc = lib.zkw_kzg_commit_cells(tau_settings.handle, ctx.handle, native._np_ptr(indices), native._np_ptr(raw), 6, native._np_ptr(out))
            msg = lib.zkw_last_error().decode()
            ctx.synchronize()
            assert rc == native.ERR_INVALID and "zkw_kzg_commit_cells" in msg and all(w in msg for w in words), msg
            assert ((out.cpu().numpy() if device else out) == 0xAA).all()
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)
    with pytest.raises(native.ZkwError) as ei:  # the Python layer carries the message
        tau_settings.commit_cells(np.array([128], np.uint64), u8(cells[0]))
    assert ei.value.code == native.ERR_INVALID and "cell_indices[0]" in str(ei.value)
    assert tau_settings.commit_cells(np.array([3], np.uint64), u8(cells[0])).shape == (1, 48)  # (the refusals leave the context usable)


# ---- pointer modes, limits, refusals by the arguments ----------------------------------------------------------------------------------------
def test_device_pointer_mode_at_odd_addresses(ctx, v64, tau_settings, blobs):
    import torch

    from era_zkevm_test_harness_amd import native

    claims = [claim(blobs, "A", (5 * i) % 128, proof_of=(5 * i + 1) % 128 if i in (2, 7) else None) for i in range(9)]
    claims[4] = (claims[4][0], 128, claims[4][2], claims[4][3])
    want = [HOLDS, HOLDS, FAILS, HOLDS, BAD_INDEX, HOLDS, HOLDS, FAILS, HOLDS]
    assert run(v64, tau_settings, claims) == want  # host pointer mode
    parts = [b"".join(c[0] for c in claims), np.array([c[1] for c in claims], np.uint64).tobytes(), b"".join(c[2] for c in claims), b"".join(c[3] for c in claims)]
    want_commitments = tau_settings.commit_cells(np.array([c[1] & 127 for c in claims], np.uint64), u8(parts[2])).tobytes()
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        bufs = []
        for raw in parts:
            b = torch.zeros(len(raw) + 1, dtype=torch.uint8, device="cuda")
            b[1:] = torch.from_numpy(u8(raw).copy()).cuda()
            bufs.append(b)
        verdicts = torch.full((9 + 2,), 0xAA, dtype=torch.uint8, device="cuda")
        out = torch.full((9 * 48 + 2,), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        at = lambda t: C.c_void_p(t.data_ptr() + 1)
        assert (bufs[2].data_ptr() + 1) % 2 == 1
        lib = native.load()
        rc = lib.zkw_kzg_verify_cells(v64.handle, tau_settings.handle, ctx.handle, at(bufs[0]), at(bufs[1]), at(bufs[2]), at(bufs[3]), 9, at(verdicts))
        assert rc == 0, lib.zkw_last_error().decode()
        good_idx = torch.zeros(9 * 8 + 1, dtype=torch.uint8, device="cuda")
        good_idx[1:] = torch.from_numpy(u8(np.array([c[1] & 127 for c in claims], np.uint64).tobytes()).copy()).cuda()
        torch.cuda.synchronize()
        rc = lib.zkw_kzg_commit_cells(tau_settings.handle, ctx.handle, at(good_idx), at(bufs[2]), 9, at(out))
        assert rc == 0, lib.zkw_last_error().decode()
        ctx.synchronize()
        assert verdicts.cpu().numpy().tolist() == [0xAA] + want + [0xAA]
        assert out.cpu().numpy().tobytes() == b"\xaa" + want_commitments + b"\xaa"
        # tensors through the Python layer
        t = lambda raw, dt=torch.uint8: torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda().view(dt)
        got = v64.verify_cells(tau_settings, t(parts[0]), t(parts[1], torch.int64), t(parts[2]), t(parts[3]))
        ctx.synchronize()
        assert got.is_cuda and got.cpu().numpy().tolist() == want
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


def test_refusals_by_the_arguments(ctx, v64, tau_settings, tau_points, blobs):
    from era_zkevm_test_harness_amd import native

    lib, p = native.load(), native._np_ptr
    c, k, cell, proof = claim(blobs, "A", 77)
    cm_, idx, cells, proofs = u8(c), np.array([k], np.uint64), u8(cell), u8(proof)
    verdicts, out = np.full(1, 0xAA, np.uint8), np.full(48, 0xAA, np.uint8)
    short = native.KzgSettings(ctx, b"".join(km.compress(q) for q in tau_points[:63]))
    try:
        rc = lib.zkw_kzg_verify_cells(v64.handle, short.handle, ctx.handle, p(cm_), p(idx), p(cells), p(proofs), 1, p(verdicts))
        msg = lib.zkw_last_error().decode()
        assert rc == native.ERR_INVALID and "zkw_kzg_verify_cells" in msg and "63 points" in msg, msg
        rc = lib.zkw_kzg_commit_cells(short.handle, ctx.handle, p(idx), p(cells), 1, p(out))
        msg = lib.zkw_last_error().decode()
        assert rc == native.ERR_INVALID and "zkw_kzg_commit_cells" in msg and "63 points" in msg, msg
    finally:
        short.free()
    rc = lib.zkw_kzg_verify_cells(v64.handle, tau_settings.handle, ctx.handle, p(cm_), p(idx), p(cells), p(proofs), (1 << 24) + 1, p(verdicts))
    assert rc == native.ERR_INVALID and "16777216" in lib.zkw_last_error().decode()
    rc = lib.zkw_kzg_verify_cells(v64.handle, tau_settings.handle, ctx.handle, p(cm_), None, p(cells), p(proofs), 1, p(verdicts))
    assert rc == native.ERR_INVALID and "null" in lib.zkw_last_error().decode()
    # no claims: OK, and nothing is written
    assert lib.zkw_kzg_verify_cells(v64.handle, tau_settings.handle, ctx.handle, None, None, None, None, 0, None) == 0
    assert lib.zkw_kzg_commit_cells(tau_settings.handle, ctx.handle, None, None, 0, None) == 0
    assert (verdicts == 0xAA).all() and (out == 0xAA).all()
    empty = np.zeros(0, np.uint8)
    assert v64.verify_cells(tau_settings, empty, np.zeros(0, np.uint64), empty, empty).shape == (0,)
    assert tau_settings.commit_cells(np.zeros(0, np.uint64), empty).shape == (0, 48)
    assert run(v64, tau_settings, [(c, k, cell, proof)]) == [HOLDS]  # (the refusals leave the context usable)
