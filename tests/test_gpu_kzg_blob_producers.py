"""GPU: the KZG producers from a blob in evaluation form (k_kzg_blob_intt in csrc/kzg_open_kernels.cuh, driver csrc/zkw_kzg.hip) —
zkw_kzg_blob_coefficients, zkw_kzg_commit_blobs, zkw_kzg_open_blobs and zkw_eip4844_prove_blobs. Expected values come from algebra and from
the committed known answers, never from the code under test: the inverse transform of a unit vector is a row of powers of w^-1; on a setup
whose tau is known the commitment of ANY evaluation-form blob is [p(tau)] G1 with p(tau) by the barycentric eval_poly of
tests/kzg_blob_verify_model.py (no transform on the expected side) and a proof is [(p(tau) - y) / (tau - z)] G1; on the ceremony's setup the
device's own verifier judges the reference's two tests (kzg/src/lib.rs:430-454), and the two golden blobs must give the records of
tests/golden/eip4844_proofs_kat.json. Commitments and proofs are unique, so every comparison is byte-exact.

A blob is always 4 096 elements (a workgroup of 512 lanes), so the small axis is the number of blobs. The unit vectors sit where a stage's
pairing changes hands: element 0 and 4 095, 1 (w = -1: every odd row negative), 2 047 | 2 048 (the two halves of the last stage undone).
Every model answer is computed once per module."""
import ctypes as C
import json
import random

import numpy as np
import pytest

from tests import kzg_blob_verify_model as bm
from tests import kzg_model as km
from tests import kzg_open_model as om
from tests import kzg_pairing_model as pm

pytestmark = pytest.mark.gpu

TAU = 0x4844
R = km.R
N = 4096
EV = 32 * N
INF = km.compress(km.INF)
N_INV = pow(N, -1, R)
ON_DOMAIN = (0, 1, 255, 256, 2047, 4095)


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
    assert s.nbytes == 32 * 4096 * 96  # the producers keep nothing in the handle: no second table
    s.free()


@pytest.fixture(scope="module")
def tau_settings(ctx):
    from era_zkevm_test_harness_amd import native

    s = native.KzgSettings(ctx, b"".join(km.compress(p) for p in om.known_tau_setup(TAU, 4096)))
    yield s
    s.free()


@pytest.fixture(scope="module")
def verifier(ctx):
    from era_zkevm_test_harness_amd import native

    v = native.KzgVerifier(ctx, pm.load_tau_g2_bytes())
    yield v
    v.free()


@pytest.fixture(scope="module")
def tau_verifier(ctx):
    from era_zkevm_test_harness_amd import native

    v = native.KzgVerifier(ctx, pm.g2_compress(pm.g2_mul(TAU, pm.G2_GEN)))
    yield v
    v.free()


def blob_of(elements):
    return b"".join(int(f).to_bytes(32, "big") for f in elements)


def random_blob(rng):
    return blob_of(rng.randrange(R) for _ in range(N))


def be32(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in values), np.uint8)


def u8(raw):
    return np.frombuffer(raw, np.uint8)


def ints(rows, order="big"):
    return [int.from_bytes(r.tobytes(), order) for r in rows]


def root(i):
    return pow(om.OMEGA, om.brp12(i), R)


def with_elements(blob, changes):
    b = bytearray(blob)
    for i, v in changes.items():
        b[32 * i:32 * i + 32] = int(v).to_bytes(32, "big")
    return bytes(b)


@pytest.fixture(scope="module")
def blob_a():
    blob = random_blob(random.Random(2901))
    assert max(bm.elements_of(blob)) >> 254  # full range: nobody's pubdata
    return blob


# ---- 1. the transform alone ------------------------------------------------------------------------------------------------------------
UNITS = (1, 0, 2047, 2048, 4095)
SOME_ROWS = (0, 1, 2, 2047, 2048, 4095)


@pytest.fixture(scope="module")
def golden_pattern(settings):
    """(pubdata blob, its evaluation form by zkw_eip4844_prove) of the golden pattern blob; the form is pinned by its SHA-256 in the KAT"""
    blob = km.pattern_blob()
    rec = settings.eip4844_witness(u8(blob))
    _, ev = settings.eip4844_prove(u8(blob), rec, evaluations=True)
    return blob, ev[0].tobytes()


@pytest.fixture(scope="module")
def transform_cases(golden_pattern):
    """[(evaluation form, {row k: expected coefficient})]: five unit vectors (every row of the first), a constant, X^4095, all r - 1, the
    golden pattern blob"""
    rng = random.Random(2902)
    out = []
    for i in UNITS:
        w_inv = pow(root(i), R - 2, R)
        rows = range(N) if i == 1 else SOME_ROWS
        out.append((blob_of(int(e == i) for e in range(N)), {k: N_INV * pow(w_inv, k, R) % R for k in rows}))
    c = rng.randrange(1, R)
    only = lambda k, v: {j: (v if j == k else 0) for j in range(N)}
    out.append((blob_of([c] * N), only(0, c)))
    out.append((blob_of(pow(root(i), R - 2, R) for i in range(N)), only(4095, 1)))  # w_i^4095 = 1 / w_i
    out.append((blob_of([R - 1] * N), only(0, R - 1)))
    blob, ev = golden_pattern
    out.append((ev, dict(enumerate(km.blob_elements(blob)[::-1]))))
    assert len(out) == 9 and len(out[0][1]) == N and out[0][1][1] == N_INV * (R - 1) % R  # 1 / w_1 = -1
    return out


@pytest.mark.parametrize("lo,hi", [(0, 0), (0, 1), (0, 3), (3, 6), (6, 9)])
def test_blob_coefficients_are_the_inverse_transform(ctx, transform_cases, lo, hi):
    from era_zkevm_test_harness_amd import native

    cases = transform_cases[lo:hi]
    got = native.kzg_blob_coefficients(ctx, u8(b"".join(c[0] for c in cases)))
    assert got.shape == (hi - lo, N, 32)
    for j, (_, want) in enumerate(cases):
        have = ints(got[j], "little")
        assert {k: have[k] for k in want} == want, lo + j


# ---- 2. a setup whose tau is known -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def by_tau(blob_a):
    """the true claim about blob_a by algebra: (p(tau), the challenge for [p(tau)] G1, the value there, the proof's scalar)"""
    c, q = bm.true_claim_by_tau(blob_a, TAU)
    z = om.blob_challenge(blob_a, bm.g1_of(c))
    return c, z, bm.eval_poly(bm.elements_of(blob_a), z), q


def test_commit_blobs_on_a_known_tau_setup(tau_settings, blob_a, by_tau):
    got = tau_settings.commit_blobs(u8(blob_a))
    assert got.shape == (1, 48) and got[0].tobytes() == bm.g1_of(by_tau[0])


def test_open_blobs_off_the_domain_and_on_it_in_one_call(tau_settings, blob_a, by_tau):
    elements = bm.elements_of(blob_a)
    points = [random.Random(2903).randrange(R)] + [root(i) for i in ON_DOMAIN]
    assert points[1] == 1 and points[2] == R - 1 and len(points) == 7
    proofs, values = tau_settings.open_blobs(u8(blob_a * 7), be32(points))
    assert proofs.shape == (7, 48) and values.shape == (7, 32)
    want = [bm.eval_poly(elements, z) for z in points]
    assert want[1:] == [elements[i] for i in ON_DOMAIN]  # on the domain the value is the element itself
    assert ints(values) == want
    for j, (z, y) in enumerate(zip(points, want)):
        assert proofs[j].tobytes() == bm.g1_of((by_tau[0] - y) * pow((TAU - z) % R, -1, R)), j


def test_prove_blobs_on_a_known_tau_setup(tau_settings, tau_verifier, blob_a, by_tau):
    c, z, y, q = by_tau
    commitment = u8(bm.g1_of(c))
    proofs, openings = tau_settings.eip4844_prove_blobs(u8(blob_a), commitment, openings=True)
    assert proofs.shape == (1, 48) and openings.shape == (1, 64)
    assert proofs[0].tobytes() == bm.g1_of(q)
    assert ints(openings[:, :32]) == [z] and ints(openings[:, 32:]) == [y]
    assert tau_settings.eip4844_prove_blobs(u8(blob_a), commitment)[0].tobytes() == bm.g1_of(q)  # openings == NULL
    assert tau_verifier.eip4844_verify_blobs(u8(blob_a), commitment, proofs).tolist() == [1]


# ---- 3. the reference's two tests on the ceremony's setup (lib.rs:430-454) -------------------------------------------------------------
def test_commit_open_verify(settings, verifier, blob_a):
    z = random.Random(2904).randrange(R)
    commitments = settings.commit_blobs(u8(blob_a))
    proofs, values = settings.open_blobs(u8(blob_a), be32([z]))
    assert ints(values) == [bm.eval_poly(bm.elements_of(blob_a), z)]
    little = lambda rows: np.ascontiguousarray(rows[:, ::-1])  # zkw_kzg_verify takes points and values little-endian
    assert verifier.verify(commitments, little(be32([z]).reshape(1, 32)), little(values), proofs).tolist() == [1]
    assert verifier.verify(commitments, little(be32([z ^ 1]).reshape(1, 32)), little(values), proofs).tolist() == [0]


def test_commit_prove_verify_random_challenge(settings, verifier, blob_a):
    commitments = settings.commit_blobs(u8(blob_a))
    proofs = settings.eip4844_prove_blobs(u8(blob_a), commitments)
    assert verifier.eip4844_verify_blobs(u8(blob_a), commitments, proofs).tolist() == [1]
    changed = bytearray(blob_a)
    changed[32 * 4095 + 31] ^= 1  # after proving
    assert verifier.eip4844_verify_blobs(u8(bytes(changed)), commitments, proofs).tolist() == [0]


# ---- 4. agreement with the pubdata path ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def proved(settings):
    """(records, proof records, evaluation forms) of the two golden blobs (zero, pattern) and a random one, by the pubdata path"""
    blobs = u8(bytes(km.BLOB_BYTES) + km.pattern_blob() + random.Random(2905).randbytes(km.BLOB_BYTES))
    rec = settings.eip4844_witness(blobs)
    prf, ev = settings.eip4844_prove(blobs, rec, evaluations=True)
    return rec, prf, ev


def padded_points(rec):
    return np.concatenate([np.zeros((len(rec), 16), np.uint8), rec["evaluation_point"]], axis=1)


def test_the_golden_blobs_give_the_records_of_the_pubdata_path(settings, proved):
    rec, prf, ev = proved
    kat = json.load(open(om.KAT_FILE))["cases"]
    golden = [r for _, r in om.kat_blobs()]
    commitments = settings.commit_blobs(ev)
    assert commitments.tobytes() == rec["commitment"].tobytes()
    proofs, values = settings.open_blobs(ev, padded_points(rec))
    assert proofs.tobytes() == prf["opening_proof"].tobytes() and values.tobytes() == rec["opening_value"].tobytes()
    blob_proofs, openings = settings.eip4844_prove_blobs(ev, rec["commitment"], openings=True)
    assert blob_proofs.tobytes() == prf["blob_proof"].tobytes()
    assert openings[:, :32].tobytes() == prf["blob_challenge"].tobytes() and openings[:, 32:].tobytes() == prf["blob_value"].tobytes()
    for j in (0, 1):  # the committed known answers
        assert commitments[j].tobytes() == golden[j]["commitment"] and values[j].tobytes() == golden[j]["opening_value"]
        assert proofs[j].tobytes().hex() == kat[j]["opening_proof"] and blob_proofs[j].tobytes().hex() == kat[j]["blob_proof"]
        assert openings[j, :32].tobytes().hex() == kat[j]["blob_challenge"] and openings[j, 32:].tobytes().hex() == kat[j]["blob_value"]


# ---- 5. degenerate blobs ---------------------------------------------------------------------------------------------------------------
def test_the_zero_blob_and_a_constant_blob(settings):
    rng = random.Random(2906)
    c, z = rng.randrange(1, R), rng.randrange(R)
    ev = u8(bytes(EV) + blob_of([c] * N))
    commitments = settings.commit_blobs(ev)
    assert commitments[0].tobytes() == INF and commitments[1].tobytes() == km.compress(km.mul_naive(c, km.load_setup()[0]))
    proofs, values = settings.open_blobs(ev, be32([z, z]))
    assert proofs[0].tobytes() == proofs[1].tobytes() == INF and ints(values) == [0, c]
    blob_proofs, openings = settings.eip4844_prove_blobs(ev, commitments, openings=True)
    assert blob_proofs[0].tobytes() == blob_proofs[1].tobytes() == INF and ints(openings[:, 32:]) == [0, c]
    assert ints(openings[:, :32]) == [om.blob_challenge(ev[j * EV:(j + 1) * EV].tobytes(), commitments[j].tobytes()) for j in (0, 1)]


# ---- 6. batching and pointer modes -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(settings, ctx, proved, blob_a):
    """three different blobs and what the four entry points return for each in a call of its own (host pointer mode)"""
    from era_zkevm_test_harness_amd import native

    rec, _, ev = proved
    blobs = [blob_a, ev[1].tobytes(), ev[2].tobytes()]
    rng = random.Random(2907)
    points = [rng.randrange(R), root(2048), rng.randrange(R)]
    commitments = [settings.commit_blobs(u8(b))[0].tobytes() for b in blobs]
    singles = {"coefficients": [native.kzg_blob_coefficients(ctx, u8(b))[0].tobytes() for b in blobs], "commit": commitments,
               "open": [tuple(x[0].tobytes() for x in settings.open_blobs(u8(b), be32([z]))) for b, z in zip(blobs, points)],
               "prove": [tuple(x[0].tobytes() for x in settings.eip4844_prove_blobs(u8(b), u8(c), openings=True)) for b, c in zip(blobs, commitments)]}
    assert commitments[1:] == [rec["commitment"][1].tobytes(), rec["commitment"][2].tobytes()]
    return blobs, points, singles


def all_four(settings, ctx, evals, points, commitments, to_bytes):
    from era_zkevm_test_harness_amd import native

    coeffs = native.kzg_blob_coefficients(ctx, evals)
    commits = settings.commit_blobs(evals)
    proofs, values = settings.open_blobs(evals, points)
    blob_proofs, openings = settings.eip4844_prove_blobs(evals, commitments, openings=True)
    return lambda: {"coefficients": [to_bytes(r) for r in coeffs], "commit": [to_bytes(r) for r in commits],
                    "open": [(to_bytes(p), to_bytes(v)) for p, v in zip(proofs, values)],
                    "prove": [(to_bytes(p), to_bytes(o)) for p, o in zip(blob_proofs, openings)]}


def test_three_blobs_in_one_call_equal_the_single_calls(settings, ctx, three):
    blobs, points, singles = three
    got = all_four(settings, ctx, u8(b"".join(blobs)), be32(points), u8(b"".join(singles["commit"])), lambda r: r.tobytes())()
    assert got == singles


def test_device_pointer_mode_at_an_odd_address_straight_after_the_prover(settings, ctx, three, proved):
    """the evaluation forms are written by zkw_eip4844_prove one byte into a buffer and read by the four calls with no host synchronisation
    in between; blobs 1 and 2 of `three` are the pubdata blobs 1 and 2 of `proved`"""
    import torch

    from era_zkevm_test_harness_amd import native

    blobs, points, singles = three
    rec = proved[0]
    pubdata = u8(km.pattern_blob() + random.Random(2905).randbytes(km.BLOB_BYTES))
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        d_blobs, d_rec = torch.from_numpy(pubdata.copy()).cuda(), torch.from_numpy(rec[1:].view(np.uint8).copy()).cuda()
        d_points, d_commitments = torch.from_numpy(be32(points[1:]).copy()).cuda(), torch.from_numpy(u8(b"".join(singles["commit"][1:])).copy()).cuda()
        d_out = torch.empty((2, native.EIP4844_PROOF_RECORD.itemsize), dtype=torch.uint8, device="cuda")
        buf = torch.zeros(2 * EV + 1, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        assert (buf.data_ptr() + 1) % 2 == 1
        rc = native.load().zkw_eip4844_prove(settings.handle, ctx.handle, ptr(d_blobs), 2, ptr(d_rec), ptr(d_out), C.c_void_p(buf.data_ptr() + 1))
        assert rc == 0, native.load().zkw_last_error().decode()
        result = all_four(settings, ctx, buf[1:], d_points, d_commitments, lambda r: r.cpu().numpy().tobytes())
        ctx.synchronize()
        got = result()
        assert buf[1:].cpu().numpy().tobytes() == b"".join(blobs[1:])
        assert got == {k: v[1:] for k, v in singles.items()}
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def raw_calls(settings, ctx, evals, points, commitments, n, device):
    """the four C calls with every output filled with 0xAA beforehand: [(name, return code, message, outputs as numpy)]"""
    import torch

    from era_zkevm_test_harness_amd import native

    lib = native.load()
    if device:
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
        new = lambda *shape: torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        back = lambda t: t.cpu().numpy()
    else:
        put, ptr, back = np.ascontiguousarray, native._np_ptr, lambda a: a
        new = lambda *shape: np.full(shape, 0xAA, np.uint8)
    ev, z, cm = put(evals), put(points), put(commitments)
    if device:
        torch.cuda.synchronize()
    outs = {"zkw_kzg_blob_coefficients": [new(n, N, 32)], "zkw_kzg_commit_blobs": [new(n, 48)], "zkw_kzg_open_blobs": [new(n, 48), new(n, 32)],
            "zkw_eip4844_prove_blobs": [new(n, 48), new(n, 64)]}
    if device:
        torch.cuda.synchronize()
    s, c = settings.handle, ctx.handle
    rcs = []
    for name, args in (("zkw_kzg_blob_coefficients", (c, ptr(ev), n)), ("zkw_kzg_commit_blobs", (s, c, ptr(ev), n)),
                       ("zkw_kzg_open_blobs", (s, c, ptr(ev), ptr(z), n)), ("zkw_eip4844_prove_blobs", (s, c, ptr(ev), ptr(cm), n))):
        rc = getattr(lib, name)(*args, *[ptr(o) for o in outs[name]])
        rcs.append((name, rc, lib.zkw_last_error().decode() if rc else ""))
    ctx.synchronize()
    return [(name, rc, msg, [back(o) for o in outs[name]]) for name, rc, msg in rcs]


@pytest.mark.parametrize("device", [False, True])
def test_an_element_equal_to_r_is_refused_by_name_and_the_outputs_stay_untouched(settings, ctx, three, device):
    from era_zkevm_test_harness_amd import native

    blobs, points, singles = three
    bad = blobs[0] + with_elements(blobs[1], {4095: R}) + blobs[2]
    commitments = u8(b"".join(singles["commit"]))
    if device:
        ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        for name, rc, msg, outs in raw_calls(settings, ctx, u8(bad), be32(points), commitments, 3, device):
            assert rc == native.ERR_INVALID and name in msg and "element 4095 of blob 1" in msg and "not below r" in msg, (name, msg)
            assert all((o == 0xAA).all() for o in outs), name
        # the lowest element of the lowest blob is the one named
        worse = with_elements(blobs[0], {4095: R, 17: (1 << 256) - 1}) + blobs[1] + with_elements(blobs[2], {0: R})
        for name, rc, msg, outs in raw_calls(settings, ctx, u8(worse), be32(points), commitments, 3, device):
            assert rc == native.ERR_INVALID and "element 17 of blob 0" in msg, (name, msg)
            assert all((o == 0xAA).all() for o in outs), name
        # the same calls without a fault
        for (name, rc, msg, outs), key in zip(raw_calls(settings, ctx, u8(b"".join(blobs)), be32(points), commitments, 3, device),
                                              ("coefficients", "commit", "open", "prove")):
            assert rc == 0, (name, msg)
            rows = [tuple(o[j].tobytes() for o in outs) for j in range(3)]
            assert [r[0] if len(r) == 1 else r for r in rows] == singles[key], name
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


def test_a_point_equal_to_r_is_refused(settings, ctx, three):
    from era_zkevm_test_harness_amd import native

    blobs, points, _ = three
    for where, point in ((1, R), (2, (1 << 256) - 1)):
        zs = list(points)
        zs[where] = point
        proofs, values = np.full((3, 48), 0xAA, np.uint8), np.full((3, 32), 0xAA, np.uint8)
        rc = native.load().zkw_kzg_open_blobs(settings.handle, ctx.handle, native._np_ptr(u8(b"".join(blobs))), native._np_ptr(be32(zs)), 3,
                                              native._np_ptr(proofs), native._np_ptr(values))
        msg = native.load().zkw_last_error().decode()
        assert rc == native.ERR_INVALID and f"point of blob {where}" in msg and "not below r" in msg, msg
        assert (proofs == 0xAA).all() and (values == 0xAA).all()
    with pytest.raises(native.ZkwError) as ei:
        settings.open_blobs(u8(blobs[0]), be32([R]))
    assert ei.value.code == native.ERR_INVALID and "point of blob 0" in str(ei.value)


def test_short_settings_too_many_blobs_and_no_blobs(settings, ctx, blob_a):
    from era_zkevm_test_harness_amd import native

    one, z, cm = u8(blob_a), be32([5]), u8(INF)
    s = native.KzgSettings(ctx, km.load_setup_bytes()[:48 * 8])
    try:
        for call in (lambda: s.commit_blobs(one), lambda: s.open_blobs(one, z), lambda: s.eip4844_prove_blobs(one, cm)):
            with pytest.raises(native.ZkwError) as ei:
                call()
            assert ei.value.code == native.ERR_INVALID and "8 points" in str(ei.value)
    finally:
        s.free()
    lib, out = native.load(), np.zeros(64, np.uint8)
    p = native._np_ptr
    for rc in (lib.zkw_kzg_blob_coefficients(ctx.handle, p(one), 32768, p(out)), lib.zkw_kzg_commit_blobs(settings.handle, ctx.handle, p(one), 32768, p(out)),
               lib.zkw_kzg_open_blobs(settings.handle, ctx.handle, p(one), p(z), 32768, p(out), p(out)),
               lib.zkw_eip4844_prove_blobs(settings.handle, ctx.handle, p(one), p(cm), 32768, p(out), None)):
        assert rc == native.ERR_INVALID and "32767" in lib.zkw_last_error().decode()
    none = np.zeros(0, np.uint8)
    assert native.kzg_blob_coefficients(ctx, none).shape == (0, N, 32)
    assert settings.commit_blobs(none).shape == (0, 48)
    proofs, values = settings.open_blobs(none, none)
    assert proofs.shape == (0, 48) and values.shape == (0, 32)
    proofs, openings = settings.eip4844_prove_blobs(none, none, openings=True)
    assert proofs.shape == (0, 48) and openings.shape == (0, 64)
    assert settings.commit_blobs(one)[0].tobytes() == settings.commit_blobs(one)[0].tobytes() != INF  # (the refusals leave the context usable)
