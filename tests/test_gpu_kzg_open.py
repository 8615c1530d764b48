"""GPU: the KZG proofs (csrc/kzg_open_kernels.cuh, csrc/zkw_kzg.hip) — zkw_kzg_open and zkw_eip4844_prove — against the host model in
plain Python integers (tests/kzg_open_model.py), the known answers of tests/golden/eip4844_proofs_kat.json and, on a setup whose tau is
known, against [(p(tau) - v) / (tau - x)] G1 computed in Fr on the host, which does not divide polynomials. A KZG proof is unique, so every
comparison is byte-exact. The settings are built once for the module; the model's answers are computed once and shared.

The sizes of zkw_kzg_open: k_kzg_quotient gives each of its 256 lanes a chunk of L = ceil(n / 256) coefficients, so n = 256 | 257 and
512 | 513 are where L changes (1 | 2 | 3), 255 and 513 leave lanes without work, 4095 leaves the last lane a short chunk, 4096 is the blob's size."""
import hashlib
import json
import random

import numpy as np
import pytest

from tests import kzg_model as km
from tests import kzg_open_model as om

pytestmark = pytest.mark.gpu

TAU = 0x4844
INF = km.compress(km.INF)
OMEGA5 = pow(om.OMEGA, 5, om.R)  # on the evaluation domain: where the reference branches


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
    assert s.nbytes == 32 * 4096 * 96  # the proofs keep nothing in the handle
    s.free()


@pytest.fixture(scope="module")
def tau_settings(ctx):
    from era_zkevm_test_harness_amd import native

    s = native.KzgSettings(ctx, b"".join(km.compress(p) for p in om.known_tau_setup(TAU, 4096)))
    yield s
    s.free()


def rows(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8)


def device_open(settings, polys, points):
    """[(proof bytes, value)] of polynomials of equal length, one call"""
    n = len(polys[0])
    proofs, values = settings.open(rows([c for p in polys for c in p]), n, rows(points))
    assert proofs.shape == (len(polys), 48) and values.shape == (len(polys), 32)
    return [(proofs[j].tobytes(), int.from_bytes(values[j].tobytes(), "little")) for j in range(len(polys))]


# ---- zkw_kzg_open -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_coeffs", [0, 1, 2, 3, 16, 17, 255, 256, 257, 512, 513, 4095, 4096])
def test_open_equals_the_model(settings, n_coeffs):
    rng = random.Random(n_coeffs)
    p = [rng.randrange(om.R) for _ in range(n_coeffs)]
    z = rng.randrange(1 << 253, om.R)
    want = om.open(p, z)
    assert device_open(settings, [p], [z]) == [want]
    if n_coeffs < 2:
        assert want[0] == INF


def test_open_at_special_points_in_one_call(settings):
    rng = random.Random(257)
    p = [rng.randrange(om.R) for _ in range(257)]
    points = [0, 1, om.R - 1, OMEGA5, rng.randrange(1 << 127, 1 << 128)]
    got = device_open(settings, [p] * len(points), points)
    for z, g in zip(points, got):
        assert g == om.open(p, z), z
    assert got[0][1] == p[0] and got[1][1] == sum(p) % om.R


def test_open_special_polynomials(settings):
    rng = random.Random(300)
    z = rng.randrange(om.R)
    assert device_open(settings, [[0] * 300], [z]) == [(INF, 0)]
    assert device_open(settings, [[om.R - 1]], [z]) == [(INF, om.R - 1)]  # a constant: the quotient is zero
    top = [om.R - 1] * 300
    assert device_open(settings, [top], [z]) == [om.open(top, z)]
    s = [rng.randrange(om.R) for _ in range(299)]
    p = [0] * 300  # (X - z) s(X): the value is 0 and the proof is the commitment of s
    for k, c in enumerate(s):
        p[k + 1] = (p[k + 1] + c) % om.R
        p[k] = (p[k] - c * z) % om.R
    assert device_open(settings, [p], [z]) == [(km.commit(s), 0)]


def test_three_polynomials_three_points_and_both_pointer_modes(ctx, settings):
    import torch

    from era_zkevm_test_harness_amd import native

    rng = random.Random(3)
    polys = [[rng.randrange(om.R) for _ in range(19)] for _ in range(3)]
    points = [rng.randrange(om.R) for _ in range(3)]
    singles = [device_open(settings, [p], [z])[0] for p, z in zip(polys, points)]
    assert singles[0] == om.open(polys[0], points[0])
    assert device_open(settings, polys, points) == singles
    flat = rows([c for p in polys for c in p])
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        for shift in (0, 1):  # the inputs at an odd byte address
            c = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), flat])).cuda()[shift:]
            z = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), rows(points)])).cuda()[shift:]
            assert c.data_ptr() % 2 == shift and z.data_ptr() % 2 == shift
            proofs, values = settings.open(c, 19, z)
            ctx.synchronize()
            assert proofs.is_cuda and values.is_cuda
            got = [(proofs[j].cpu().numpy().tobytes(), int.from_bytes(values[j].cpu().numpy().tobytes(), "little")) for j in range(3)]
            assert got == singles, shift
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


def raw_open(settings, ctx, coeffs, n_coeffs, n_polys, points):
    """the C call with outputs filled beforehand: (return code, message, proofs, values)"""
    from era_zkevm_test_harness_amd import native

    proofs, values = np.full((n_polys, 48), 0xAA, np.uint8), np.full((n_polys, 32), 0xAA, np.uint8)
    rc = native.load().zkw_kzg_open(settings.handle, ctx.handle, native._np_ptr(coeffs), n_coeffs, n_polys, native._np_ptr(points), native._np_ptr(proofs),
                                    native._np_ptr(values))
    return rc, native.load().zkw_last_error().decode(), proofs, values


def test_open_refusals_name_the_position_and_leave_the_outputs_untouched(ctx, settings):
    from era_zkevm_test_harness_amd import native

    good = [[1, 2, 3], [4, 5, 6]]
    cases = [(rows([1, 2, 3, 4, om.R, 6]), rows([7, 8]), "coefficient 1 of polynomial 1"),
             (rows(sum(good, [])), rows([7, om.R]), "point of polynomial 1"),
             (rows(sum(good, [])), rows([(1 << 256) - 1, 8]), "point of polynomial 0")]
    for coeffs, points, what in cases:
        rc, msg, proofs, values = raw_open(settings, ctx, coeffs, 3, 2, points)
        assert rc == native.ERR_INVALID and what in msg and "not below r" in msg, msg
        assert (proofs == 0xAA).all() and (values == 0xAA).all()
    rc, msg, proofs, values = raw_open(settings, ctx, rows([0] * 4097), 4097, 1, rows([1]))
    assert rc == native.ERR_INVALID and "4097" in msg and "4096" in msg, msg
    assert (proofs == 0xAA).all() and (values == 0xAA).all()
    rc, msg, proofs, values = raw_open(settings, ctx, rows(sum(good, [])), 3, 2, rows([7, 8]))  # the same call without a fault
    assert rc == 0 and [(proofs[j].tobytes(), int.from_bytes(values[j].tobytes(), "little")) for j in range(2)] == [om.open(p, z) for p, z in zip(good, (7, 8))]


# ---- zkw_eip4844_prove -------------------------------------------------------------------------------------------------------------------
def record_dict(rec):
    return {f: rec[f].tobytes() for f in rec.dtype.names}


def proof_fields(rec):
    return {f: rec[f].tobytes() for f in om.FIELDS}


def record_array(fields):
    from era_zkevm_test_harness_amd import native

    rec = np.zeros(1, native.EIP4844_RECORD)
    for f, v in fields.items():
        rec[f][0] = np.frombuffer(v, np.uint8)
    return rec


@pytest.mark.parametrize("name", ["random", "ones"])
def test_prove_on_a_known_tau_setup(tau_settings, name):
    blob = random.Random(4844).randbytes(km.BLOB_BYTES) if name == "random" else b"\xff" * km.BLOB_BYTES
    b = np.frombuffer(blob, np.uint8)
    rec = tau_settings.eip4844_witness(b)
    out, ev = tau_settings.eip4844_prove(b, rec, evaluations=True)
    assert out.shape == (1,) and ev.shape == (1, 131072)
    record, got = record_dict(rec[0]), proof_fields(out[0])
    coeffs = om.blob_coefficients(blob)
    tau_value = 0
    for a in reversed(coeffs):
        tau_value = (tau_value * TAU + a) % om.R
    assert record["commitment"] == km.compress(km.mul_naive(tau_value, km.load_setup()[0]))
    want = om.eip4844_prove(blob, record, proofs=False)
    assert ev[0].tobytes() == want["blob_evaluations"]
    assert got["blob_challenge"] == want["blob_challenge"] and got["blob_value"] == want["blob_value"]
    z, c = int.from_bytes(record["evaluation_point"], "big"), int.from_bytes(want["blob_challenge"], "big")
    assert got["opening_proof"] == om.proof_by_tau(coeffs, z, TAU)
    assert got["blob_proof"] == om.proof_by_tau(coeffs, c, TAU)


@pytest.fixture(scope="module")
def proved(settings):
    """name -> (blob, witness records, proof records of a call of its own without the evaluation form)"""
    rng = random.Random(16)
    out = {}
    for (blob, fields), name in zip(om.kat_blobs(), ("zero", "pattern")):
        out[name] = (blob, record_array(fields))
    for name, blob in (("random", rng.randbytes(km.BLOB_BYTES)), ("ones", b"\xff" * km.BLOB_BYTES)):
        out[name] = (blob, settings.eip4844_witness(np.frombuffer(blob, np.uint8)))
    return {name: (blob, rec, settings.eip4844_prove(np.frombuffer(blob, np.uint8), rec)) for name, (blob, rec) in out.items()}


@pytest.mark.parametrize("case", [0, 1])
def test_prove_the_golden_blobs(settings, proved, case):
    kat = json.load(open(om.KAT_FILE))["cases"][case]
    blob, rec, single = proved[("zero", "pattern")[case]]
    out, ev = settings.eip4844_prove(np.frombuffer(blob, np.uint8), rec, evaluations=True)
    for f in om.FIELDS:
        assert out[0][f].tobytes().hex() == kat[f], f
    assert hashlib.sha256(ev[0].tobytes()).hexdigest() == kat["blob_evaluations_sha256"]
    assert proof_fields(single[0]) == proof_fields(out[0])  # blob_evaluations == NULL gives the same record
    if case == 0:
        assert out[0]["opening_proof"].tobytes() == out[0]["blob_proof"].tobytes() == INF


def test_prove_a_random_blob_equals_the_model(settings, proved):
    blob, rec, single = proved["random"]
    want = om.eip4844_prove(blob, record_dict(rec[0]))
    assert proof_fields(single[0]) == {f: want[f] for f in om.FIELDS}
    _, ev = settings.eip4844_prove(np.frombuffer(blob, np.uint8), rec, evaluations=True)
    assert ev[0].tobytes() == want["blob_evaluations"]


def test_four_blobs_in_one_call_equal_the_single_calls(settings, proved):
    for order in (["pattern", "zero", "random", "ones"], ["ones", "random", "zero", "pattern"]):
        blobs = np.frombuffer(b"".join(proved[n][0] for n in order), np.uint8)
        recs = np.concatenate([proved[n][1] for n in order])
        out, ev = settings.eip4844_prove(blobs, recs, evaluations=True)
        assert out.shape == (4,) and ev.shape == (4, 131072)
        for j, n in enumerate(order):
            assert proof_fields(out[j]) == proof_fields(proved[n][2][0]), (order, n)
        assert [proof_fields(r) for r in settings.eip4844_prove(blobs, recs)] == [proof_fields(r) for r in out]
        assert ev[order.index("zero")].tobytes() == bytes(131072)


def test_prove_in_device_pointer_mode_straight_after_the_witness(ctx, settings, proved):
    """records taken from zkw_eip4844_witness on the same context with no host synchronisation in between; the blobs at an odd address"""
    import torch

    from era_zkevm_test_harness_amd import native

    names = ["random", "pattern"]
    raw = b"".join(proved[n][0] for n in names)
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        for shift in (0, 1):
            view = torch.from_numpy(np.frombuffer(bytes(shift) + raw, np.uint8).copy()).cuda()[shift:]
            rec = settings.eip4844_witness(view)
            out, ev = settings.eip4844_prove(view, rec, evaluations=True)
            bare = settings.eip4844_prove(view, rec)
            ctx.synchronize()
            got = out.cpu().numpy().view(native.EIP4844_PROOF_RECORD).reshape(-1)
            got_bare = bare.cpu().numpy().view(native.EIP4844_PROOF_RECORD).reshape(-1)
            for j, n in enumerate(names):
                assert proof_fields(got[j]) == proof_fields(got_bare[j]) == proof_fields(proved[n][2][0]), (shift, n)
            assert hashlib.sha256(ev[1].cpu().numpy().tobytes()).hexdigest() == json.load(open(om.KAT_FILE))["cases"][1]["blob_evaluations_sha256"]
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


def test_no_blobs_is_a_no_op_and_short_settings_are_refused(ctx, settings, proved):
    from era_zkevm_test_harness_amd import native

    assert settings.eip4844_prove(np.zeros(0, np.uint8), np.zeros(0, native.EIP4844_RECORD)).shape == (0,)
    proofs, values = settings.open(np.zeros(0, np.uint8), 5, np.zeros(0, np.uint8))
    assert proofs.shape == (0, 48) and values.shape == (0, 32)
    s = native.KzgSettings(ctx, km.load_setup_bytes()[:48 * 4095])
    try:
        with pytest.raises(native.ZkwError) as ei:
            s.eip4844_prove(np.frombuffer(proved["zero"][0], np.uint8), proved["zero"][1])
        assert ei.value.code == native.ERR_INVALID and "4095" in str(ei.value)
    finally:
        s.free()
