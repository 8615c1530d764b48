"""GPU: the Fourier transform over G1 points (k_kzg_g1_fft in csrc/kzg_cell_kernels.cuh, zkw_kzg_g1_fft in csrc/zkw_kzg.hip). Expected
values come from the definition, never from the code under test: out[u] = sum_j w_n^(u j) in[j] with w_n = 7^((r - 1) / n) — at n <= 8 by
n^2 double-and-add multiplications of the host model, at n = 128 on multiples of the generator, in[j] = [a_j] G, where the transform of the
points is the generator times the transform of the scalars. Compressed points are unique, so every comparison is byte-exact."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from tests import kzg_model as km
from tests import kzg_open_model as om

pytestmark = pytest.mark.gpu

R = km.R
INF = km.compress(km.INF)
G = km.decompress(km.load_setup_bytes()[:48], check_subgroup=False)


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def g1(s):
    """compress([s] G)"""
    return km.compress(km.mul_naive(s % R, G))


def root(n):
    return pow(7, (R - 1) // n, R)


def u8(raw):
    return np.frombuffer(raw, np.uint8)


def fft(ctx, rows, n, inverse=False):
    """rows: compressed points, a multiple of n of them -> the transformed rows"""
    from era_zkevm_test_harness_amd import native

    out = native.kzg_g1_fft(ctx, u8(b"".join(rows)), n, inverse=inverse)
    assert out.shape == (len(rows) // n, n, 48)
    return [r.tobytes() for t in out for r in t]


def scalars_fft(a, inverse=False):
    n = len(a)
    w = root(n)
    if not inverse:
        return om._ntt(list(a), w)
    return [v * pow(n, -1, R) % R for v in om._ntt(list(a), pow(w, -1, R))]


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_small_transforms_against_the_definition(ctx, n):
    rng = random.Random(7594 + n)
    a = [rng.randrange(1, R) for _ in range(n)]
    pts = [km.mul_naive(s, G) for s in a]
    w = root(n)
    assert pow(w, n, R) == 1 and (n == 1 or pow(w, n // 2, R) == R - 1)
    want = [km.compress(km.msm_naive([pow(w, u * j, R) for j in range(n)], pts)) for u in range(n)]
    assert fft(ctx, [km.compress(p) for p in pts], n) == want
    w_inv, n_inv = pow(w, -1, R), pow(n, -1, R)
    want = [km.compress(km.msm_naive([pow(w_inv, u * j, R) * n_inv % R for j in range(n)], pts)) for u in range(n)]
    assert fft(ctx, [km.compress(p) for p in pts], n, inverse=True) == want


@pytest.fixture(scope="module")
def big():
    """128 scalars and their points"""
    rng = random.Random(7595)
    a = [rng.randrange(R) for _ in range(128)]
    return a, [g1(s) for s in a]


def test_128_points_are_the_generator_times_the_transform_of_the_scalars(ctx, big):
    a, pts = big
    got = fft(ctx, pts, 128)
    assert got == [g1(s) for s in scalars_fft(a)]
    assert fft(ctx, got, 128, inverse=True) == pts  # inverse after forward is the identity
    assert fft(ctx, fft(ctx, pts[:8], 8, inverse=True), 8) == pts[:8]


def test_identity_inputs(ctx, big):
    a, pts = big
    assert fft(ctx, [INF] * 128, 128) == [INF] * 128
    assert fft(ctx, [INF] * 4, 4, inverse=True) == [INF] * 4
    # the upper half at infinity: the shape of every FK20 input
    half = a[:64] + [0] * 64
    assert fft(ctx, pts[:64] + [INF] * 64, 128) == [g1(s) for s in scalars_fft(half)]
    # a single point: every output is that point
    assert fft(ctx, [pts[0]] + [INF] * 15, 16) == [pts[0]] * 16


def test_equal_inputs_and_opposite_inputs(ctx, big):
    a, pts = big
    for n in (2, 8, 128):  # equal inputs: the first stage subtracts a point from itself in every butterfly
        assert fft(ctx, [pts[1]] * n, n) == [g1(n * a[1])] + [INF] * (n - 1), n
    minus = km.compress(km.neg(km.decompress(pts[2], check_subgroup=False)))
    assert fft(ctx, [pts[2], minus], 2) == [INF, g1(2 * a[2])]  # P + (-P), then P - (-P): the doubling inside an addition
    assert fft(ctx, [pts[2], minus] * 2, 4) == [g1(s) for s in scalars_fft([a[2], R - a[2]] * 2)]


def test_three_transforms_in_one_call(ctx, big):
    a, pts = big
    got = fft(ctx, pts[:24], 8)
    assert got == [g1(s) for k in range(3) for s in scalars_fft(a[8 * k:8 * k + 8])]
    assert got == [p for k in range(3) for p in fft(ctx, pts[8 * k:8 * k + 8], 8)]
    inv = fft(ctx, pts[:24], 8, inverse=True)
    assert inv == [g1(s) for k in range(3) for s in scalars_fft(a[8 * k:8 * k + 8], inverse=True)]


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
    assert km.mul_naive(R, km.decompress(bytes(on_curve_outside), check_subgroup=False)) is not km.INF
    for bad, why in ((bytes(off_curve), "no y"), (bytes(on_curve_outside), "subgroup"), (bytes(48), "not a compressed point")):
        rows = list(pts[:16])
        rows[8 + 5] = bad
        out = np.full((2, 8, 48), 0xAA, np.uint8)
        rc = lib.zkw_kzg_g1_fft(ctx.handle, native._np_ptr(u8(b"".join(rows))), 8, 2, 0, native._np_ptr(out))
        msg = lib.zkw_last_error().decode()
        assert rc == native.ERR_INVALID and "point 5 of transform 1" in msg and why in msg, msg
        assert (out == 0xAA).all()
    for n in (0, 3, 256):
        out = np.full(48, 0xAA, np.uint8)
        assert lib.zkw_kzg_g1_fft(ctx.handle, native._np_ptr(u8(pts[0])), n, 1, 0, native._np_ptr(out)) == native.ERR_INVALID
        assert (out == 0xAA).all()
    assert lib.zkw_kzg_g1_fft(ctx.handle, None, 8, 0, 0, None) == 0  # no transforms: a no-op
    assert fft(ctx, pts[:2], 2) == [g1(s) for s in scalars_fft(big[0][:2])]  # (the refusals leave the context usable)


def test_device_pointer_mode(ctx, big):
    import torch

    from era_zkevm_test_harness_amd import native

    _, pts = big
    want = fft(ctx, pts[:16], 8)
    ctx.set_pointer_mode(native.PTR_DEVICE)
    try:
        d_in = torch.from_numpy(u8(b"".join(pts[:16])).copy()).cuda()
        torch.cuda.synchronize()
        out = native.kzg_g1_fft(ctx, d_in, 8)
        ctx.synchronize()
        assert [r.tobytes() for t in out.cpu().numpy() for r in t] == want
    finally:
        ctx.set_pointer_mode(native.PTR_HOST)
