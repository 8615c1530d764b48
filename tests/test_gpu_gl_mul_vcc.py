"""GPU: gl::mul_vcc, the S-box product of the chain forms (csrc/gl64.cuh). tests/csrc_gpu/gl_mul_vcc_test.hip checks it against the host
gl::mul_lat on the cross product of eleven edge words, on pairs that reach all eight combinations of its three flags and on 2^16 seeded
pairs; the chain API runs 64-item queues through the quad form at 16 chains (one wave) and 17 (a ragged second wave) and one 64-item
queue through the row form, each word for word against the oracle."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
P = 0xFFFFFFFF00000001
ITEMS = 64


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


def test_mul_vcc_equals_the_host_product(tmp_path):
    exe = str(tmp_path / "gl_mul_vcc_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc_gpu", "gl_mul_vcc_test.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert int(words[1]) >= 121 + (1 << 16) and words[3] == "ff"


def _queues(n_queues, seed):
    """n_queues queues of ITEMS items: canonical random words, every fourth queue of edge words only"""
    rng = np.random.default_rng(seed)
    offsets = (np.arange(n_queues + 1) * ITEMS).astype(np.uint64)
    enc = rng.integers(0, P, (n_queues * ITEMS, 8), dtype=np.uint64)
    tins = rng.integers(0, P, (n_queues, 12), dtype=np.uint64)
    edge = np.array([0, 1, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFE00000002], np.uint64)
    for k in range(0, n_queues, 4):
        enc[k * ITEMS:(k + 1) * ITEMS] = edge[rng.integers(0, len(edge), (ITEMS, 8))]
        tins[k] = edge[rng.integers(0, len(edge), 12)]
    return offsets, enc, tins


def _check(ctx, oracle, n_queues, form):
    offsets, enc, tins = _queues(n_queues, 100 + n_queues)
    ctx.set_chain_form(form)
    try:
        got = ctx.queue_push_chain_full_batch(enc, offsets, tins)
    finally:
        ctx.set_chain_form(0)
    for k in range(n_queues):
        assert np.array_equal(got[k * ITEMS:(k + 1) * ITEMS], oracle.queue_push_chain_full(enc[k * ITEMS:(k + 1) * ITEMS], tins[k])), k


@pytest.mark.parametrize("n_queues", [16, 17])
def test_quad_form_chains_of_64_items(ctx, oracle, n_queues):
    _check(ctx, oracle, n_queues, 4)


def test_row_form_chain_of_64_items(ctx, oracle):
    _check(ctx, oracle, 1, 0)  # below 4 096 chains dev_chains takes the row form by itself
