"""Writes era_zkevm_test_harness_amd/csrc/kzg_cell_tables.cuh: the constants of the EIP-7594 cell kernels (kzg_cell_kernels.cuh) that are
not worth computing on the device — the GLV split of the 128 twiddles of the G1 transform, the endomorphism's beta, the 8 192nd root of
unity W of the extended blob, and for the wide G1 transform (kzg_g1_fft_wide_kernels.cuh) the split of the lower half of the 4 096th roots. `python tools/gen_kzg_cell_tables.py` rewrites the file, `--check` compares it with what is committed
(tests/test_kzg_cells_model.py does the same and checks the statements the numbers rest on).

BLS12-381 has the endomorphism phi(x, y) = (beta x, y) on G1, beta a primitive cube root of unity of Fq, and phi(P) = [lambda] P with
lambda = z^2 - 1 for the curve's parameter z = -0xd201000000010000: lambda^2 + lambda + 1 = 0 mod r. lambda has 128 bits and r 255, so
a scalar k < r splits as k = k1 + k2 lambda with k1 = k mod lambda and k2 = k div lambda, both non-negative and below 2^128 — plain integer
division, no lattice and no signs. [k] P = [k1] P + [k2] phi(P) then takes 128 doublings instead of 255."""
import os
import sys

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
Z = 0xD201000000010000
LAMBDA = Z * Z - 1
BETA = 0x1A0111EA397FE699EC02408663D4DE85AA0D857D89759AD4897D29650FB85F9B409427EB4F49FFFD8BFD00000000AAAC
W128 = pow(7, (R - 1) // 128, R)
W8192 = pow(7, (R - 1) // 8192, R)
W4096 = W8192 * W8192 % R
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "era_zkevm_test_harness_amd", "csrc", "kzg_cell_tables.cuh")


def split(k):
    """(k1, k2): k = k1 + k2 LAMBDA, both below 2^128"""
    k2, k1 = divmod(k % R, LAMBDA)
    assert k1 < 1 << 128 and k2 < 1 << 128
    return k1, k2


def words(v, n):
    return ", ".join("0x%08xu" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(n))


def twiddle_rows():
    """row e: the split of W128^e (e < 128), then row 128 + b: the split of 2^-b mod r (b <= 7: the inverse transform's 1 / n)"""
    return [split(pow(W128, e, R)) for e in range(128)] + [split(pow(pow(2, b, R), -1, R)) for b in range(8)]


def wide_twiddle_rows():
    """row e: the split of W4096^e (e < 2048; the upper half is its negative), then row 2048 + b - 8: the split of 2^-b mod r (b = 8 .. 12)"""
    return [split(pow(W4096, e, R)) for e in range(2048)] + [split(pow(pow(2, b, R), -1, R)) for b in range(8, 13)]


def render():
    assert (LAMBDA * LAMBDA + LAMBDA + 1) % R == 0 and pow(BETA, 3, P) == 1 and BETA != 1
    assert pow(W128, 64, R) == R - 1 and pow(W8192, 4096, R) == R - 1 and W8192 * W8192 % R == pow(7, (R - 1) // 4096, R)
    lines = ["// kzg_cell_tables.cuh — written by tools/gen_kzg_cell_tables.py; do not edit. The constants of kzg_cell_kernels.cuh.",
             "#pragma once",
             "#include \"bls12_381.cuh\"",
             "",
             "namespace zkw {",
             "// rows 0..127: w128^e = k1 + k2 lambda for w128 = 7^((r - 1) / 128), words 0..3 = k1 and 4..7 = k2 (least significant first, plain",
             "// integers below 2^128); rows 128..135: the same split of 2^-b mod r",
             "static __constant__ bls::u32 c_kzg_g1_twiddle[136][8] = {"]
    for k1, k2 in twiddle_rows():
        lines.append("    {%s, %s}," % (words(k1, 4), words(k2, 4)))
    lines += ["};",
              "// beta (Montgomery form): (beta x, y) = [lambda] (x, y) on G1, lambda = 0x%x" % LAMBDA,
              "static __device__ __forceinline__ bls::Fq kzg_g1_beta() {",
              "    return bls::Fq{{%s}};" % words(BETA * (1 << 384) % P, 12),
              "}",
              "// W = 7^((r - 1) / 8192) (Montgomery form): W^2 is the blob's root of unity, kzg_omega()",
              "static __device__ __forceinline__ bls::Fr kzg_cell_w() {",
              "    return bls::Fr{{%s}};" % words(W8192 * (1 << 256) % R, 8),
              "}",
              "// rows 0..2047: w4096^e = k1 + k2 lambda for w4096 = 7^((r - 1) / 4096), the words as above (w4096^(2048 + e) = -w4096^e: the",
              "// kernel negates the point); rows 2048..2052: the split of 2^-b mod r, b = 8 .. 12. 64 KiB: in global memory, not in a constant bank",
              "static __device__ const bls::u32 d_kzg_g1_twiddle_wide[2053][8] = {"]
    assert pow(W4096, 2048, R) == R - 1 and pow(W4096, 32, R) == W128
    for k1, k2 in wide_twiddle_rows():
        lines.append("    {%s, %s}," % (words(k1, 4), words(k2, 4)))
    lines += ["};",
              "}  // namespace zkw",
              ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT).read() == text else "kzg_cell_tables.cuh is stale: run python tools/gen_kzg_cell_tables.py")
    with open(OUT, "w") as f:
        f.write(text)
    print(OUT)
