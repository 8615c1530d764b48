"""GPU: the EIP-4844 blob witness (csrc/kzg_kernels.cuh, csrc/zkw_kzg.hip) — zkw_kzg_settings_create, zkw_kzg_commit and
zkw_eip4844_witness — against the host model in plain Python integers (tests/kzg_model.py) and the known answers of
tests/golden/eip4844_kat.json. Every comparison is byte-exact. The settings of the public ceremony (tests/golden/kzg_trusted_setup_g1.bin)
are built once for the module; the model's witnesses are computed once and shared."""
import json
import os
import random
import threading

import numpy as np
import pytest

from tests import kzg_model as km

pytestmark = pytest.mark.gpu

FIELDS = ("linear_hash", "versioned_hash", "output_hash", "evaluation_point", "opening_value", "commitment")


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
    assert s.num_points == 4096 and s.nbytes == 32 * 4096 * 96
    yield s
    s.free()


def le32(v):
    return int(v).to_bytes(32, "little")


def coeff_rows(polys):
    return np.frombuffer(b"".join(le32(c) for p in polys for c in p), np.uint8)


def small_settings(ctx, points):
    from era_zkevm_test_harness_amd import native

    return native.KzgSettings(ctx, b"".join(km.compress(p) for p in points))


@pytest.fixture(scope="module")
def blobs():
    """name -> (blob, expected record fields): the two known answers from the golden file, the others from the model (once)"""
    kat = json.load(open(os.path.join(km.GOLDEN, "eip4844_kat.json")))["cases"]
    rng = random.Random(4844)
    first_only = bytes(rng.randrange(1, 256) for _ in range(31)) + bytes(km.BLOB_BYTES - 31)
    last_one = bytes(km.BLOB_BYTES - 31) + b"\x01" + bytes(30)
    out = {"zero": (bytes(km.BLOB_BYTES), {f: bytes.fromhex(kat[0][f]) for f in FIELDS}),
           "pattern": (km.pattern_blob(), {f: bytes.fromhex(kat[1][f]) for f in FIELDS})}
    for name, blob in (("ones", b"\xff" * km.BLOB_BYTES), ("first_only", first_only), ("last_one", last_one), ("random", rng.randbytes(km.BLOB_BYTES))):
        out[name] = (blob, km.eip4844_witness(blob))
    return out


def record_fields(rec):
    return {f: rec[f].tobytes() for f in FIELDS}


# ---- zkw_kzg_commit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_coeffs", [1, 2, 3, 255, 256, 257])
def test_commit_equals_the_model(ctx, settings, n_coeffs):
    rng = random.Random(n_coeffs)
    coeffs = [rng.randrange(1 << 254, km.R) for _ in range(n_coeffs)]
    got = settings.commit(coeff_rows([coeffs]), n_coeffs)
    assert got.shape == (1, 48) and got[0].tobytes() == km.commit(coeffs)


def test_commit_edge_polynomials(ctx, settings):
    raw = km.load_setup_bytes()
    assert settings.commit(coeff_rows([[0] * 7]), 7)[0].tobytes() == bytes([0xC0]) + bytes(47)
    for k in (0, 1, 4095):
        assert settings.commit(coeff_rows([[0] * k + [1]]), k + 1)[0].tobytes() == raw[48 * k:48 * k + 48], k
    g = km.load_setup()[0]
    assert settings.commit(coeff_rows([[km.R - 1]]), 1)[0].tobytes() == km.compress(km.neg(g))


@pytest.mark.parametrize("bad", [km.R, (1 << 256) - 1])
def test_commit_refuses_a_coefficient_that_is_not_below_r(ctx, settings, bad):
    from era_zkevm_test_harness_amd import native

    with pytest.raises(native.ZkwError) as ei:
        settings.commit(coeff_rows([[1, 2, 3], [4, bad, 6]]), 3)
    assert ei.value.code == native.ERR_INVALID and "coefficient 1 of polynomial 1" in str(ei.value)


def test_three_polynomials_in_one_call_and_both_pointer_modes(ctx, settings):
    import torch

    from era_zkevm_test_harness_amd import native

    rng = random.Random(3)
    polys = [[rng.randrange(km.R) for _ in range(19)] for _ in range(3)]
    singles = [settings.commit(coeff_rows([p]), 19)[0].tobytes() for p in polys]
    assert singles[0] == km.commit(polys[0])
    both = settings.commit(coeff_rows(polys), 19)
    assert [both[j].tobytes() for j in range(3)] == singles
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        dev = settings.commit(torch.from_numpy(coeff_rows(polys).copy()).cuda(), 19)
        ctx.synchronize()
        assert dev.is_cuda and [dev[j].cpu().numpy().tobytes() for j in range(3)] == singles
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


# ---- the group law in accumulation and reduction: settings that repeat and negate points ------------------------------------------------
def test_repeated_and_negated_setup_points(ctx):
    rng = random.Random(8)
    g = km.load_setup()[0]
    a, b = km.mul_naive(rng.randrange(1, km.R), g), km.mul_naive(rng.randrange(1, km.R), g)
    c = rng.randrange(1 << 254, km.R)
    s = small_settings(ctx, [a, a, km.neg(a), b])
    try:
        assert s.num_points == 4
        assert s.commit(coeff_rows([[c] * 4]), 4)[0].tobytes() == km.compress(km.mul_naive(c, km.add(a, b)))
    finally:
        s.free()
    s = small_settings(ctx, [a, km.neg(a)])
    try:
        assert s.commit(coeff_rows([[c, c]]), 2)[0].tobytes() == km.compress(km.INF)
    finally:
        s.free()
    s = small_settings(ctx, [a] * 300)
    try:
        assert s.commit(coeff_rows([[1] * 300]), 300)[0].tobytes() == km.compress(km.mul_naive(300, a))
    finally:
        s.free()
    s = small_settings(ctx, [a, km.INF, b])  # an infinity point inside the list is accepted and contributes nothing
    try:
        c2 = rng.randrange(km.R)
        want = km.add(km.mul_naive(c, a), km.mul_naive(c2, b))
        assert s.commit(coeff_rows([[c, 12345, c2]]), 3)[0].tobytes() == km.compress(want)
    finally:
        s.free()


# ---- zkw_eip4844_witness -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zero", "pattern", "ones", "first_only", "last_one", "random"])
def test_witness_field_by_field(ctx, settings, blobs, name):
    blob, want = blobs[name]
    rec = settings.eip4844_witness(np.frombuffer(blob, np.uint8))
    assert rec.shape == (1,)
    got = record_fields(rec[0])
    for f in FIELDS:
        assert got[f] == want[f], (name, f, got[f].hex(), want[f].hex())
    if name == "last_one":  # p(X) = 1: the commitment is the generator
        assert got["commitment"] == km.load_setup_bytes()[:48]


def test_four_blobs_in_one_call_equal_the_single_calls(ctx, settings, blobs):
    for order in (["pattern", "zero", "random", "ones"], ["ones", "random", "zero", "pattern"]):
        rec = settings.eip4844_witness(np.frombuffer(b"".join(blobs[n][0] for n in order), np.uint8))
        assert rec.shape == (4,)
        for j, n in enumerate(order):
            assert record_fields(rec[j]) == blobs[n][1], (order, n)


def test_witness_in_device_pointer_mode_from_an_odd_address(ctx, settings, blobs):
    """the sponge loads a blob by 8-byte words when it may and by bytes when the caller's pointer is not a multiple of 8"""
    import torch

    from era_zkevm_test_harness_amd import native

    names = ["random", "pattern"]
    raw = b"".join(blobs[n][0] for n in names)
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        for shift in (0, 1):
            buf = torch.from_numpy(np.frombuffer(bytes(shift) + raw, np.uint8).copy()).cuda()
            view = buf[shift:]
            assert view.data_ptr() % 8 == shift
            rec = settings.eip4844_witness(view)
            ctx.synchronize()
            got = rec.cpu().numpy().view(native.EIP4844_RECORD).reshape(-1)
            for j, n in enumerate(names):
                assert record_fields(got[j]) == blobs[n][1], (shift, n)
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)


def test_no_blobs_is_a_no_op_and_short_settings_are_refused(ctx, settings, blobs):
    from era_zkevm_test_harness_amd import native

    assert settings.eip4844_witness(np.zeros(0, np.uint8)).shape == (0,)
    s = native.KzgSettings(ctx, km.load_setup_bytes()[:48 * 4095])
    try:
        with pytest.raises(native.ZkwError) as ei:
            s.eip4844_witness(np.frombuffer(blobs["zero"][0], np.uint8))
        assert ei.value.code == native.ERR_INVALID and "4095" in str(ei.value)
    finally:
        s.free()


# ---- forgeries at creation ---------------------------------------------------------------------------------------------------------------
def _forgeries():
    raw = km.load_setup_bytes()
    x = 1  # an on-curve point outside the order-r subgroup: the smallest x >= 1 with a root that r does not kill
    while True:
        y = km.sqrt_fq((x ** 3 + km.B) % km.P)
        if y is not None and km.mul_naive(km.R, (x, y)) is not km.INF:
            break
        x += 1
    xr = 1
    while km.sqrt_fq((xr ** 3 + km.B) % km.P) is not None:
        xr += 1
    return {"bit 7 cleared": bytes([raw[0] & 0x7F]) + raw[1:48],
            "infinity flag with a nonzero x": bytes([0xC0]) + raw[1:48],
            "x = p": bytes([0x80 | (km.P >> 376)]) + (km.P & ((1 << 376) - 1)).to_bytes(47, "big"),
            "x without a root": bytes([0x80]) + xr.to_bytes(47, "big"),
            "outside the subgroup": km.compress((x, y))}


@pytest.mark.parametrize("what", ["bit 7 cleared", "infinity flag with a nonzero x", "x = p", "x without a root", "outside the subgroup"])
def test_creation_refuses_a_forged_point_and_names_its_position(ctx, what):
    from era_zkevm_test_harness_amd import native

    raw = km.load_setup_bytes()
    forged = _forgeries()[what]
    with pytest.raises(km.BadPoint):  # the model refuses it too (the last one by [r]P != O)
        km.decompress(forged)
    pos = 5
    points = raw[:48 * pos] + forged + raw[48 * (pos + 1):48 * 9]
    with pytest.raises(native.ZkwError) as ei:
        native.KzgSettings(ctx, points)
    assert ei.value.code == native.ERR_INVALID and f"point {pos} " in str(ei.value), str(ei.value)
    native.KzgSettings(ctx, raw[:48 * 9]).free()  # the same list without the forgery is accepted


# ---- two contexts on the same settings at once -------------------------------------------------------------------------------------------
def test_two_contexts_commit_on_the_same_settings_at_once(ctx, settings):
    from era_zkevm_test_harness_amd import native

    rng = random.Random(2)
    polys = [[rng.randrange(km.R) for _ in range(64)] for _ in range(2)]
    want = [settings.commit(coeff_rows([p]), 64)[0].tobytes() for p in polys]
    assert want[0] == km.commit(polys[0])
    got, errors = [None, None], []

    def work(i):
        try:
            c = native.Context(0)
            for _ in range(3):
                got[i] = settings.commit(coeff_rows([polys[i]]), 64, ctx=c)[0].tobytes()
            c.close()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got == want
