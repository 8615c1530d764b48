"""GPU: the segmented radix sort (csrc/radix_sort.cuh, radix_sort_pairs_segmented) and the RAM builder's sort on top of it, which sorts
every block of a batch inside its own segment and packs no block id into a key. tests/csrc_gpu/rs_seg_sort_test.hip compares the sort
with std::stable_sort of every segment (sizes, segment counts and checks: the program's header comment); the API test sends batches of
unequal blocks down each of the builder's three routes and compares the sorted queries with a stable numpy sort of every block."""
import os
import subprocess

import numpy as np
import pytest

from era_zkevm_test_harness_amd import synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "era_zkevm_test_harness_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_segmented_sort_equals_the_stable_host_sort_of_every_segment(tmp_path):
    if not os.path.exists(os.path.join(PKG, "libzkw.so")):
        from era_zkevm_test_harness_amd import build

        build.build()
    exe = str(tmp_path / "rs_seg_sort_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tests", "csrc_gpu", "rs_seg_sort_test.hip"), "-o", exe,
                           "-L" + PKG, "-lzkw", "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-2000:]
    # 17 segment shapes x 2 key families x (4 end_bits for u64 + 3 for u32)
    assert int(r.stdout.split()[1]) >= 17 * 2 * 7


@pytest.fixture(scope="module")
def ctx():
    from era_zkevm_test_harness_amd import native

    c = native.Context(0)
    yield c
    c.close()


LENS = [2049, 1, 1500, 4500]  # one pair more than a tile, one item, less than a tile, three tiles


@pytest.mark.parametrize("route,pages,indices,ts_start", [
    ("one", 64, 256, 1),                  # every field narrow: a single packed sort
    ("two", 2**32 - 9, 2**16, 2**31),     # 32 + 16 + 32 bits: timestamps first, then the packed cell word of 48 bits
    ("three", 2**32 - 9, 2**32, 2**31),   # 32 + 32 bits of cell alone: timestamps first, then the cell word as it is
])
def test_builder_sort_keeps_every_block_in_its_segment(ctx, route, pages, indices, ts_start):
    from era_zkevm_test_harness_amd import native

    offs = np.concatenate([[0], np.cumsum(LENS)]).astype(np.uint64)
    blocks = []
    for i, ln in enumerate(LENS):
        b = synthetic.ram_trace(ln, seed=1900 + i, pages=pages, indices=indices, ts_start=ts_start)
        if pages > 64:  # wide keys are sparse: fold most of them onto a few cells so that ties and runs exist
            fold = np.arange(ln) % 3 != 0
            b["page"][fold] = b["page"][0]
            b["index"][fold] = b["index"][fold] % 5
        b["timestamp"] = ts_start + (b["timestamp"] - ts_start) // 4  # (cell, timestamp) ties: the stable order shows
        blocks.append(b)
    q = np.concatenate(blocks)
    # what the route needs, asserted on the input: the widths of the three fields in this batch
    bits = [int(q[f].max()).bit_length() for f in ("page", "index", "timestamp")]
    assert {"one": sum(bits) <= 64, "two": sum(bits) > 64 and bits[0] + bits[1] < 64, "three": bits[0] + bits[1] == 64}[route], bits
    w = ctx.compute_ram_circuit_snapshots(q, 512, list(range(len(LENS))), block_offsets=offs)
    sq = w.get(native.RAM_SORTED_QUERIES)
    for b, ln in enumerate(LENS):
        lo = int(offs[b])
        blk = q[lo:lo + ln]
        exp = blk[np.lexsort((blk["timestamp"], blk["index"], blk["page"]))]  # stable
        assert np.array_equal(sq[lo:lo + ln], exp), (route, b, np.flatnonzero(sq[lo:lo + ln] != exp)[:8])
    w.free()
