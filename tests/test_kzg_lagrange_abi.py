"""CPU-side checks of the Lagrange-basis boundary, the way tests/test_kzg_cell_verify_abi.py checks its calls: include/zkw.h declares
zkw_kzg_g1_fft_wide, zkw_kzg_settings_to_lagrange, zkw_kzg_settings_to_monomial, zkw_kzg_settings_points and zkw_kzg_settings_basis with the
documented prototypes, the library exports them, and native.SYMBOLS, native.kzg_g1_fft_wide and native.KzgSettings bind them; the wide
transform's table is what tools/gen_kzg_cell_tables.py writes, next to the 136 rows of the wave kernel."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkw_kzg_g1_fft_wide", "zkw_kzg_settings_to_lagrange", "zkw_kzg_settings_to_monomial", "zkw_kzg_settings_points", "zkw_kzg_settings_basis")


def test_prototypes(tmp_path):
    src = r"""
    #include <stddef.h>
    #include "zkw.h"
    /* assigning to pointers of the documented types fails to compile if a prototype differs */
    int (*p_fft)(zkw_ctx *, const uint8_t *, size_t, size_t, int, uint8_t *) = zkw_kzg_g1_fft_wide;
    int (*p_lag)(const zkw_kzg_settings *, zkw_ctx *, zkw_kzg_settings **) = zkw_kzg_settings_to_lagrange;
    int (*p_mon)(const zkw_kzg_settings *, zkw_ctx *, zkw_kzg_settings **) = zkw_kzg_settings_to_monomial;
    int (*p_pts)(const zkw_kzg_settings *, zkw_ctx *, uint8_t *) = zkw_kzg_settings_points;
    int (*p_bas)(const zkw_kzg_settings *) = zkw_kzg_settings_basis;
    int main(void){ return p_fft && p_lag && p_mon && p_pts && p_bas && zkw_kzg_settings_basis(NULL) == 0 ? 0 : 1; }
    """
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(tmp_path / "t.c")])
    from era_zkevm_test_harness_amd import build

    lib = build.build()
    subprocess.check_call(["gcc", "-o", str(tmp_path / "t"), str(tmp_path / "t.o"), lib, f"-Wl,-rpath,{os.path.dirname(lib)}", "-Wl,--allow-shlib-undefined"])
    subprocess.check_call([str(tmp_path / "t")])


def test_library_exports_the_symbols_and_python_binds_them():
    from era_zkevm_test_harness_amd import build, native

    lib = ctypes.CDLL(build.build())
    names = {n for n, _, _ in native.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in names, name
    assert callable(native.kzg_g1_fft_wide)
    for method in ("to_lagrange", "to_monomial", "points", "_adopt"):
        assert callable(getattr(native.KzgSettings, method)), method
    assert isinstance(native.KzgSettings.basis, property)


def test_the_wide_table_is_the_generators_and_the_wave_rows_stay():
    from tools import gen_kzg_cell_tables as gen

    text = open(gen.OUT).read()
    assert text == gen.render()
    assert "c_kzg_g1_twiddle[136][8]" in text and "d_kzg_g1_twiddle_wide[2053][8]" in text
    rows = gen.wide_twiddle_rows()
    assert len(rows) == 2053
    w = pow(7, (gen.R - 1) // 4096, gen.R)
    for e in (0, 1, 31, 32, 1024, 2047):
        k1, k2 = rows[e]
        assert (k1 + k2 * gen.LAMBDA) % gen.R == pow(w, e, gen.R) and k1 < 1 << 128 and k2 < 1 << 128
        assert pow(w, 2048 + e, gen.R) == gen.R - pow(w, e, gen.R)  # the upper half is the negated point
    for e in range(64):  # row 32 e of the wide table is row e of the wave kernel's
        assert rows[32 * e] == gen.twiddle_rows()[e]
    for b in range(8, 13):
        k1, k2 = rows[2048 + b - 8]
        assert (k1 + k2 * gen.LAMBDA) * (1 << b) % gen.R == 1
