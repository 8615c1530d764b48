"""GPU: the setup in the Lagrange basis (zkw_kzg_settings_to_lagrange, _to_monomial, _points, _basis in csrc/zkw_kzg.hip over
csrc/kzg_g1_fft_wide_kernels.cuh). Expected values never come from the code under test: for a known tau the closed-form Lagrange scalars
and fixed-base products of tests/kzg_lagrange_model.py (no transform of points), for the ceremony's setup the committed fixture
tests/golden/kzg_trusted_setup_g1_lagrange.bin (a host transform, checked on the CPU by three sums) and the reference's own formula
compute_commitment = sum_i blob[i] lagrange_setup_brp[i] against the monomial route. Compressed points are unique: byte-exact throughout."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from tests import kzg_lagrange_model as lm
from tests import kzg_model as km
from tests import kzg_open_model as om

pytestmark = pytest.mark.gpu

R = km.R
TAU = 0x4844
N = 4096
INF = km.compress(km.INF)
FIXTURE = os.path.join(km.GOLDEN, "kzg_trusted_setup_g1_lagrange.bin")


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
def lagrange(ctx, settings):
    s = settings.to_lagrange()
    yield s
    s.free()


def setup_bytes(points):
    return b"".join(km.compress(p) for p in points)


def blob_of(elements):
    return b"".join(int(f).to_bytes(32, "big") for f in elements)


def little_endian(blob):
    """a blob's 4 096 elements of 32 big-endian bytes as zkw_kzg_commit's little-endian rows"""
    return np.frombuffer(blob, np.uint8).reshape(-1, 32)[:, ::-1].copy()


def make(ctx, raw):
    from era_zkevm_test_harness_amd import native

    return native.KzgSettings(ctx, raw)


@pytest.mark.parametrize("n", [256, 4096])
def test_known_tau(ctx, n):
    s = make(ctx, setup_bytes(om.known_tau_setup(TAU, n)))
    lag = s.to_lagrange()
    assert (s.basis, lag.basis, lag.num_points, lag.nbytes) == (0, 1, n, s.nbytes)
    assert lag.points().tobytes() == lm.lagrange_setup_brp(TAU, n)
    s.free()  # the source first: the new handle is independent of it
    back = lag.to_monomial()
    assert back.basis == 0 and back.points().tobytes() == lm.generator_points([pow(TAU, k, R) for k in range(n)])
    lag.free()
    back.free()


@pytest.mark.parametrize("n", [1, 2])
def test_sizes_one_and_two(ctx, n):
    setup = om.known_tau_setup(TAU, n)
    s = make(ctx, setup_bytes(setup))
    lag = s.to_lagrange()
    n_inv, w_inv = pow(n, -1, R), pow(lm.root(n), -1, R)
    want = [km.msm_naive([n_inv * pow(w_inv, u * k, R) % R for k in range(n)], setup) for u in range(n)]  # brp of one bit is itself
    assert lag.points().tobytes() == setup_bytes(want)
    assert s.points().tobytes() == setup_bytes(setup)
    back = lag.to_monomial()
    assert back.points().tobytes() == setup_bytes(setup)
    for h in (s, lag, back):
        h.free()


def test_tau_on_the_domain(ctx):
    """tau = w_256^5: l_u(tau) is 1 at u = 5 and 0 elsewhere, so the handle is the generator at brp8(5) and 255 points at infinity"""
    n, w = 256, lm.root(256)
    tau = pow(w, 5, R)
    mono = lm.generator_points([pow(tau, k, R) for k in range(n)])
    s = make(ctx, mono)
    lag = s.to_lagrange()
    want = [INF] * n
    want[lm.brp(5, 8)] = km.load_setup_bytes()[:48]
    assert lag.points().tobytes() == b"".join(want) == lm.lagrange_setup_brp(tau, n)
    fresh = make(ctx, b"".join(want))  # exactly those bytes, as a host with a Lagrange-only file holds them: basis 0
    back = fresh.to_monomial()
    assert fresh.basis == 0 and back.basis == 0 and back.points().tobytes() == mono
    for h in (s, lag, fresh, back):
        h.free()


def test_ceremony_setup_equals_the_fixture_and_comes_back(ctx, settings, lagrange):
    fixture = open(FIXTURE, "rb").read()
    assert lagrange.basis == 1 and lagrange.num_points == N and lagrange.nbytes == settings.nbytes
    assert lagrange.points().tobytes() == fixture
    back = lagrange.to_monomial()
    assert back.basis == 0 and back.points().tobytes() == km.load_setup_bytes()
    back.free()


def test_a_handle_from_the_fixtures_bytes_commits_and_opens_like_the_monomial_one(ctx, settings):
    from_file = make(ctx, open(FIXTURE, "rb").read())
    assert from_file.basis == 0  # (the library cannot know)
    mono = from_file.to_monomial()
    rng = random.Random(30)
    coeffs = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(N)), np.uint8)
    z = np.frombuffer(rng.randrange(R).to_bytes(32, "little"), np.uint8)
    assert mono.commit(coeffs, N).tobytes() == settings.commit(coeffs, N).tobytes()
    got, want = mono.open(coeffs, N, z), settings.open(coeffs, N, z)
    assert [np.asarray(a).tobytes() for a in got] == [np.asarray(a).tobytes() for a in want]
    from_file.free()
    mono.free()


def test_commit_on_the_lagrange_handle_is_the_references_compute_commitment(ctx, settings, lagrange):
    rng = random.Random(31)
    blobs = [blob_of(rng.randrange(R) for _ in range(N)), bytes(32 * N), blob_of([R - 1] * N)]
    for blob in blobs:
        want = settings.commit_blobs(np.frombuffer(blob, np.uint8)).tobytes()
        assert lagrange.commit(little_endian(blob), N).tobytes() == want
    assert lagrange.commit(little_endian(blobs[1]), N).tobytes() == INF


def test_the_evaluations_of_a_monomial_commit_to_its_setup_point(ctx, lagrange):
    """e[i] = X^k at w^brp12(i): sum_i e[i] S'[i] = [tau^k] G1 = S[k], with no host curve arithmetic"""
    w = lm.root(N)
    setup = km.load_setup_bytes()
    for k in (0, 1, 4095):
        evals = b"".join(pow(w, k * om.brp12(i), R).to_bytes(32, "little") for i in range(N))
        assert lagrange.commit(np.frombuffer(evals, np.uint8), N).tobytes() == setup[48 * k:48 * k + 48], k


def test_refusals_of_the_transform(ctx, settings, lagrange):
    from era_zkevm_test_harness_amd import native

    lib = native.load()
    raw = km.load_setup_bytes()
    for n in (3, 4095):
        s = make(ctx, raw[:48 * n])
        with pytest.raises(native.ZkwError) as e:
            s.to_lagrange()
        assert e.value.code == native.ERR_INVALID and "power of two" in str(e.value) and str(n) in str(e.value)
        with pytest.raises(native.ZkwError):
            s.to_monomial()
        s.free()
    with pytest.raises(native.ZkwError) as e:
        lagrange.to_lagrange()
    assert e.value.code == native.ERR_INVALID and "Lagrange basis already" in str(e.value)
    out = C.c_void_p(None)
    assert lib.zkw_kzg_settings_to_lagrange(None, ctx.handle, C.byref(out)) == native.ERR_INVALID and not out.value
    assert lib.zkw_kzg_settings_basis(None) == 0
    import torch

    if torch.cuda.device_count() > 1:  # a context on another device is refused as zkw_kzg_settings_create's callers are
        other = native.Context(1)
        with pytest.raises(native.ZkwError) as e:
            settings.to_lagrange(ctx=other)
        assert "device" in str(e.value)
        with pytest.raises(native.ZkwError):
            settings.points(ctx=other)
        other.close()
    assert settings.points().tobytes() == raw  # (the refusals leave handle and context usable)


def _aa(n):
    return np.full(n, 0xAA, np.uint8)


def _monomial_only_calls(native, lib, ctx, verifier, blob31, evals, record):
    """name -> (call on a settings handle -> return code, its output arrays): the nine calls that read S[k] as [tau^k] G1"""
    p = native._np_ptr
    z = np.frombuffer((5).to_bytes(32, "little"), np.uint8).copy()
    z_be = np.frombuffer((5).to_bytes(32, "big"), np.uint8).copy()
    coeffs = np.frombuffer(b"".join((7 * i + 1).to_bytes(32, "little") for i in range(8)), np.uint8).copy()
    idx = np.array([3], np.uint64)
    cell = np.frombuffer(evals.tobytes()[3 * 2048:4 * 2048], np.uint8).copy()
    commitment, proof = _aa(48), _aa(48)
    commitment[:] = np.frombuffer(km.load_setup_bytes()[:48], np.uint8)
    proof[:] = commitment
    outs = {k: [_aa(n) for n in sizes] for k, sizes in {
        "zkw_eip4844_witness": [192], "zkw_kzg_open": [48, 32], "zkw_eip4844_prove": [160], "zkw_kzg_commit_blobs": [48],
        "zkw_kzg_open_blobs": [48, 32], "zkw_eip4844_prove_blobs": [48, 64], "zkw_kzg_cell_settings_create": [],
        "zkw_kzg_commit_cells": [48], "zkw_kzg_verify_cells": [1]}.items()}
    o = {k: [p(a) for a in v] for k, v in outs.items()}

    def cell_settings(s):
        h = C.c_void_p(None)
        rc = lib.zkw_kzg_cell_settings_create(s, ctx.handle, C.byref(h))
        if h.value:
            lib.zkw_kzg_cell_settings_free(h)
        return rc

    calls = {
        "zkw_eip4844_witness": lambda s: lib.zkw_eip4844_witness(s, ctx.handle, p(blob31), 1, o["zkw_eip4844_witness"][0]),
        "zkw_kzg_open": lambda s: lib.zkw_kzg_open(s, ctx.handle, p(coeffs), 8, 1, p(z), *o["zkw_kzg_open"]),
        "zkw_eip4844_prove": lambda s: lib.zkw_eip4844_prove(s, ctx.handle, p(blob31), 1, p(record), o["zkw_eip4844_prove"][0], None),
        "zkw_kzg_commit_blobs": lambda s: lib.zkw_kzg_commit_blobs(s, ctx.handle, p(evals), 1, o["zkw_kzg_commit_blobs"][0]),
        "zkw_kzg_open_blobs": lambda s: lib.zkw_kzg_open_blobs(s, ctx.handle, p(evals), p(z_be), 1, *o["zkw_kzg_open_blobs"]),
        "zkw_eip4844_prove_blobs": lambda s: lib.zkw_eip4844_prove_blobs(s, ctx.handle, p(evals), p(commitment), 1, *o["zkw_eip4844_prove_blobs"]),
        "zkw_kzg_cell_settings_create": cell_settings,
        "zkw_kzg_commit_cells": lambda s: lib.zkw_kzg_commit_cells(s, ctx.handle, p(idx), p(cell), 1, o["zkw_kzg_commit_cells"][0]),
        "zkw_kzg_verify_cells": lambda s: lib.zkw_kzg_verify_cells(verifier.handle, s, ctx.handle, p(commitment), p(idx), p(cell), p(proof), 1,
                                                                   o["zkw_kzg_verify_cells"][0]),
    }
    return calls, outs, (z, z_be, coeffs, idx, cell, commitment, proof)


def test_the_nine_monomial_only_calls_refuse_a_lagrange_handle_and_serve_a_basis_0_one(ctx, settings, lagrange):
    from era_zkevm_test_harness_amd import native
    from tests import kzg_pairing_model as pm

    lib = native.load()
    verifier = native.KzgVerifier(ctx, pm.load_tau_g2_bytes())
    rng = random.Random(32)
    blob31 = np.frombuffer(bytes(rng.randrange(256) for _ in range(native.EIP4844_BLOB_BYTES)), np.uint8).copy()
    evals = np.frombuffer(blob_of(rng.randrange(R) for _ in range(N)), np.uint8).copy()
    record = settings.eip4844_witness(blob31)
    calls, outs, _keep = _monomial_only_calls(native, lib, ctx, verifier, blob31, evals, record)
    for name, call in calls.items():  # refused by name, ahead of any launch: the outputs keep their 0xAA
        rc = call(lagrange.handle)
        msg = lib.zkw_last_error().decode()
        assert rc == native.ERR_INVALID and name in msg and "Lagrange basis" in msg, (name, rc, msg)
        assert all((a == 0xAA).all() for a in outs[name]), name
    # a basis-0 handle with the same points (there and back) is served, and gives the bytes of the handle made from the file
    back = lagrange.to_monomial()
    want = {}
    for name, call in calls.items():
        assert call(settings.handle) == 0, (name, lib.zkw_last_error().decode())
        want[name] = [a.copy() for a in outs[name]]
        for a in outs[name]:
            a[:] = 0xAA
    for name, call in calls.items():
        assert call(back.handle) == 0, (name, lib.zkw_last_error().decode())
        assert all((a == b).all() for a, b in zip(outs[name], want[name])), name
        assert all(not (a == 0xAA).all() for a in outs[name]), name
    assert want["zkw_eip4844_witness"][0].tobytes() == record.tobytes()
    assert want["zkw_kzg_commit_blobs"][0].tobytes() == settings.commit_blobs(evals).tobytes()
    # zkw_kzg_commit knows no basis
    assert lagrange.commit(little_endian(evals.tobytes()), N).tobytes() == want["zkw_kzg_commit_blobs"][0].tobytes()
    back.free()
    verifier.free()
