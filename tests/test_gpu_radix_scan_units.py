"""GPU: the two primitives under every sorter and builder, on their own — the stable radix sort of csrc/radix_sort.cuh against std::stable_sort
and the tiled prefix counts / sums of csrc/scan_kernels.cuh against sequential loops, bit for bit. tests/csrc_gpu/rs_sort_test.hip and
scan_prefix_test.hip include the library's headers, call its drivers on a context of the built libzkw.so and launch the scan bodies whose
second loop round the drivers only reach at hundreds of millions of pairs on arrays made for the purpose (sizes, key families and checks: the
programs' header comments). Built with hipcc on the box, linked against the package's library."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "era_zkevm_test_harness_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _run(tmp_path, name, timeout):
    if not os.path.exists(os.path.join(PKG, "libzkw.so")):
        from era_zkevm_test_harness_amd import build

        build.build()
    exe = str(tmp_path / name)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tests", "csrc_gpu", name + ".hip"), "-o", exe,
                           "-L" + PKG, "-lzkw", "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-2000:]
    return int(r.stdout.split()[1])


def test_radix_sort_equals_the_stable_host_sort(tmp_path):
    # 96 (size, family, values) combinations x 6 end_bits for u32 and 9 for u64, 6 + 5 direct launches of the two scan bodies
    assert _run(tmp_path, "rs_sort_test", 120) >= 96 * 15 + 11


def test_prefix_scans_equal_the_sequential_sums(tmp_path):
    # 12 sizes x (5 flag inputs + 2 route inputs + 2 value inputs x 3 widths), 4 + 4 direct launches of the two offsets bodies
    assert _run(tmp_path, "scan_prefix_test", 120) >= 12 * 13 + 8
