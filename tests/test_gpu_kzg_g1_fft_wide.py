"""GPU: the Fourier transform over G1 points beyond one wave (csrc/kzg_g1_fft_wide_kernels.cuh, zkw_kzg_g1_fft_wide in csrc/zkw_kzg.hip):
n = 256 (the smallest size that leaves the wave: one stage over HBM and two tail blocks), 512 (two stages: the twiddle stride between
stages and a two-bit block reversal) and 4 096 (the whole table, five stages). Inputs are [a_j] G for random full-range a_j, and the
expected outputs the generator times the transform of the scalars (tests/kzg_lagrange_model.py's fixed-base products, which share
nothing with the kernels), byte-exact: compressed points are unique."""
import random

import numpy as np
import pytest

from tests import kzg_lagrange_model as lm
from tests import kzg_model as km
from tests import kzg_open_model as om

pytestmark = pytest.mark.gpu

R = km.R
INF = km.compress(km.INF)


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


def g1(scalars):
    """[compress([s] G) for s]"""
    raw = lm.generator_points(scalars)
    return [raw[48 * k:48 * k + 48] for k in range(len(scalars))]


def u8(raw):
    return np.frombuffer(raw, np.uint8)


def fft(ctx, rows, n, inverse=False, entry="kzg_g1_fft_wide"):
    from era_zkevm_test_harness_amd import native

    out = getattr(native, entry)(ctx, u8(b"".join(rows)), n, inverse=inverse)
    assert out.shape == (len(rows) // n, n, 48)
    return [r.tobytes() for t in out for r in t]


def scalars_fft(a, inverse=False):
    n = len(a)
    w = lm.root(n)
    if not inverse:
        return om._ntt(list(a), w)
    return [v * pow(n, -1, R) % R for v in om._ntt(list(a), pow(w, -1, R))]


@pytest.fixture(scope="module")
def big():
    """4 096 full-range scalars and their points (computed once; the smaller cases take slices)"""
    rng = random.Random(4096)
    a = [rng.randrange(R) for _ in range(4096)]
    return a, g1(a)


@pytest.mark.parametrize("n", [256, 512])
def test_forward_inverse_and_round_trip(ctx, big, n):
    a, pts = big[0][:n], big[1][:n]
    got = fft(ctx, pts, n)
    assert got == g1(scalars_fft(a))
    assert fft(ctx, pts, n, inverse=True) == g1(scalars_fft(a, inverse=True))
    assert fft(ctx, got, n, inverse=True) == pts


def test_4096_points(ctx, big):
    a, pts = big
    got = fft(ctx, pts, 4096, inverse=True)
    assert got == g1(scalars_fft(a, inverse=True))
    assert fft(ctx, got, 4096) == pts


def test_1024_and_2048_points_round_trip_through_their_scale_rows(ctx, big):
    """(n = 4 096 above uses the last scale row only: 2^-10 and 2^-11 are reached here, against the forward transform the model pins)"""
    a, pts = big
    for n in (1024, 2048):
        got = fft(ctx, pts[:n], n)
        assert got[:3] + got[-3:] == g1([sum(pow(lm.root(n), u * j, R) * a[j] for j in range(n)) % R for u in (0, 1, 2, n - 3, n - 2, n - 1)])
        assert fft(ctx, got, n, inverse=True) == pts[:n]


def test_three_transforms_in_one_call_equal_three_calls(ctx, big):
    a, pts = big
    for inverse in (False, True):
        got = fft(ctx, pts[1024:1792], 256, inverse=inverse)
        assert got == [p for k in range(3) for p in fft(ctx, pts[1024 + 256 * k:1280 + 256 * k], 256, inverse=inverse)]
        assert got[256:512] == g1(scalars_fft(a[1280:1536], inverse=inverse))


def test_edge_inputs_at_256(ctx, big):
    a, pts = big
    n = 256
    assert fft(ctx, [INF] * n, n) == [INF] * n
    assert fft(ctx, [INF] * n, n, inverse=True) == [INF] * n
    assert fft(ctx, [pts[3]] + [INF] * (n - 1), n) == [pts[3]] * n  # one point: every output is that point
    # all inputs equal: the first stage subtracts a point from itself in every butterfly and multiplies the point at infinity
    assert fft(ctx, [pts[1]] * n, n) == g1([n * a[1]]) + [INF] * (n - 1)
    assert fft(ctx, [pts[1]] * n, n, inverse=True) == [pts[1]] + [INF] * (n - 1)
    minus = km.compress(km.neg(km.decompress(pts[2], check_subgroup=False)))
    alt = [a[2], R - a[2]] * (n // 2)  # P, -P alternating: u + v doubles in the stage whose halves meet a point with itself
    assert fft(ctx, [pts[2], minus] * (n // 2), n) == g1(scalars_fft(alt))
    assert scalars_fft(alt)[n // 2] == n * a[2] % R and sum(1 for s in scalars_fft(alt) if s) == 1


@pytest.mark.parametrize("n", [8, 128])
def test_up_to_128_points_the_bytes_are_the_wave_kernels(ctx, big, n):
    _, pts = big
    for inverse in (False, True):
        assert fft(ctx, pts[:2 * n], n, inverse=inverse) == fft(ctx, pts[:2 * n], n, inverse=inverse, entry="kzg_g1_fft")


def test_a_bad_point_is_refused_by_position_and_the_output_stays_untouched(ctx, big):
    from era_zkevm_test_harness_amd import native

    _, pts = big
    lib = native.load()
    x = next(x for x in range(1, 100) if km.sqrt_fq((x ** 3 + 4) % km.P) is None)
    off_curve = bytearray(x.to_bytes(48, "big"))
    off_curve[0] |= 0x80
    x = next(x for x in range(1, 100) if km.sqrt_fq((x ** 3 + 4) % km.P) is not None)
    on_curve_outside = bytearray(x.to_bytes(48, "big"))  # on the curve; the cofactor is huge, so not in the order-r subgroup
    on_curve_outside[0] |= 0x80
    for bad, why in ((bytes(off_curve), "no y"), (bytes(on_curve_outside), "subgroup"), (bytes(48), "not a compressed point")):
        rows = list(pts[:512])
        rows[256 + 5] = bad
        out = np.full((2, 256, 48), 0xAA, np.uint8)
        rc = lib.zkw_kzg_g1_fft_wide(ctx.handle, native._np_ptr(u8(b"".join(rows))), 256, 2, 0, native._np_ptr(out))
        msg = lib.zkw_last_error().decode()
        assert rc == native.ERR_INVALID and "point 5 of transform 1" in msg and why in msg, msg
        assert (out == 0xAA).all()


def test_bad_sizes_are_refused_and_the_context_stays_usable(ctx, big):
    from era_zkevm_test_harness_amd import native

    a, pts = big
    lib = native.load()
    src = u8(b"".join(pts))
    for n, n_ffts in ((0, 1), (3, 1), (8192, 1), (4096, 17)):
        out = np.full(48, 0xAA, np.uint8)  # (refused on its sizes, ahead of any read of the points)
        assert lib.zkw_kzg_g1_fft_wide(ctx.handle, native._np_ptr(src), n, n_ffts, 0, native._np_ptr(out)) == native.ERR_INVALID, (n, n_ffts)
        assert (out == 0xAA).all()
        assert "zkw_kzg_g1_fft_wide" in lib.zkw_last_error().decode()
    assert lib.zkw_kzg_g1_fft_wide(ctx.handle, None, 256, 0, 0, None) == 0  # no transforms: a no-op
    assert fft(ctx, pts[:256], 256) == g1(scalars_fft(a[:256]))


def test_device_pointer_mode_at_an_odd_address(ctx, big):
    import torch

    from era_zkevm_test_harness_amd import native

    _, pts = big
    want = fft(ctx, pts[:512], 256, inverse=True)
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        raw = u8(b"".join(pts[:512]))
        d_buf = torch.zeros(raw.size + 1, dtype=torch.uint8, device="cuda")
        d_buf[1:] = torch.from_numpy(raw.copy()).cuda()
        d_in = d_buf[1:]
        assert d_in.data_ptr() % 2 == 1
        torch.cuda.synchronize()
        out = native.kzg_g1_fft_wide(ctx, d_in, 256, inverse=True)
        ctx.synchronize()
        assert [r.tobytes() for t in out.cpu().numpy() for r in t] == want
        # a bad point in device pointer mode: the output tensor stays as it was
        d_buf[1 + 48 * 261:1 + 48 * 262] = 0
        d_out = torch.full((2 * 256 * 48 + 1,), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = native.load().zkw_kzg_g1_fft_wide(ctx.handle, d_in.data_ptr(), 256, 2, 1, d_out[1:].data_ptr())
        ctx.synchronize()
        assert rc == native.ERR_INVALID and "point 5 of transform 1" in native.load().zkw_last_error().decode()
        assert bool((d_out == 0xAA).all())
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)
