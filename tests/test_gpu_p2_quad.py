"""GPU: the quad form of the Poseidon2 permutation (p2::Coop4, the permutation of the queue-chain kernels k_chain_full_q4 / q4x4) with its
linear layers on 32-bit word planes. tests/csrc_gpu/p2_quad_test.hip checks it against the host p2::permute on 2^16 states, weak
non-canonical words among them; the chain API runs edge-valued queues (all p - 1, all zero, mixed) through the quad form at 16 chains
and, at >= 4 096 chains, through the 4-wave launch of the throughput path, against the oracle."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


def test_quad_form_permutation_equals_the_host_permutation(tmp_path):
    exe = str(tmp_path / "p2_quad_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc_gpu", "p2_quad_test.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) >= 1 << 16


def _edge_queues(n_queues, seed):
    """queues of all p - 1, all zero, and a mix of 0 / 1 / p - 1 / p - 2 / 2^32 - 1 / 2^32 words, with edge-valued incoming tails"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 5, n_queues)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(offsets[-1])
    words = np.array([0, 1, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFE00000002], np.uint64)
    enc = words[rng.integers(0, len(words), (n, 8))]
    tins = words[rng.integers(0, len(words), (n_queues, 12))]
    for k in range(n_queues):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        if k % 3 == 0:
            enc[lo:hi] = P - 1
            tins[k] = P - 1
        elif k % 3 == 1:
            enc[lo:hi] = 0
            tins[k] = 0
    return lens.tolist(), offsets, enc, tins


@pytest.mark.parametrize("n_queues", [16, 4100])
def test_quad_form_chains_on_edge_values(ctx, oracle, n_queues):
    lens, offsets, enc, tins = _edge_queues(n_queues, n_queues)
    if n_queues < 4096:  # dev_chains takes the quad form by itself from 4 096 chains on
        ctx.set_chain_form(4)
    try:
        got = ctx.queue_push_chain_full_batch(enc, offsets, tins)
    finally:
        ctx.set_chain_form(0)
    for k, ln in enumerate(lens):
        lo = int(offsets[k])
        assert np.array_equal(got[lo:lo + ln], oracle.queue_push_chain_full(enc[lo:lo + ln], tins[k])), k
