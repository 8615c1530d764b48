// gl_mul_flags.h — the host word model of the three flags of gl::mul_vcc and gl::mul_cyc (one algebra, csrc/gl64.cuh) and the pairs built
// for the two combinations that a seeded enumeration does not reach. Shared by gl_mul_vcc_test.hip and gl_field_test.hip.
#pragma once
#include <stdint.h>

// cm * 4 + c1 * 2 + b1 of the product a * b: cm — the cross terms a0 b1 + a1 b0 carry out of 64 bits; c1 — x = w2 * EPS + (w1:w0) wraps;
// b1 — the subtraction x - w3 borrows (w0..w3 the exact product's 32-bit words)
static inline int gl_mul_flags(uint64_t a, uint64_t b) {
    const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
    const unsigned __int128 q = (unsigned __int128)((uint64_t)a0 * b1) + (uint64_t)a1 * b0, pr = (unsigned __int128)a * b;
    const uint32_t w0 = (uint32_t)pr, w1 = (uint32_t)(pr >> 32), w2 = (uint32_t)(pr >> 64), w3 = (uint32_t)(pr >> 96);
    const unsigned __int128 x = (unsigned __int128)w2 * 0xFFFFFFFFu + (((uint64_t)w1 << 32) | w0);
    return (int)(q >> 64) * 4 + (int)(x >> 64) * 2 + ((uint64_t)x < w3 ? 1 : 0);
}

// cm with b1, with and without c1, needs a product whose words 1 and 2 cancel in x (about one pair in 2^32 and one in 2^64): pairs built
// for them (b = w0 / a mod 2^96 by lattice reduction, and a search)
static const uint64_t GL_MUL_BUILT_PAIRS[12][2] = {
    {0xe6eb8c9efd69fe29ull, 0xe7bd541e6870ff79ull}, {0xcd464138e6233255ull, 0xcbda28c7fd7a54caull}, {0xde527100f814e8a3ull, 0xe074284f872cabbdull},
    {0xe87c966cf77b9aa3ull, 0xd8a27c493fb105baull}, {0xe1da8978e06f5c67ull, 0xf426792c4ee52fccull}, {0xd8921396c0ddb74dull, 0xe1082b5b6fc7281eull},
    {0xc021c246e148b905ull, 0xc0ac1741fe4b8282ull}, {0xd65ca199c1c5f494ull, 0xed5dd83dd7ec64a2ull}, {0xe76c9686cff99085ull, 0xc5494e5ac62cdf56ull},
    {0xf1fefe17c04e698dull, 0xe3e33286e39402bbull}, {0xe0d3707dde9dbc8full, 0xdf6aec11ce98637full}, {0xfc0f574ccdb8abc9ull, 0xc41a5667f81c1196ull}};
