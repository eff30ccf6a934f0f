// polar_bits.h -- the word-level steps on bit-packed rows, the same text on the host and on the device.
//
// Packing.  A row of N bits is N / 32 words: bit j is bit j & 31 of word j >> 5.  A path's partial sums share one such row:
// level t (2^t elements), element e  <->  bit 2^t + e, so the levels below 5 are bits 1 .. 31 of word 0 and level t >= 5
// is the words 2^(t-5) .. 2^(t-4) - 1.  The saved left-child sums (bl) use this layout; the working sums (cur) of the level
// being formed start at bit 0 (word 0).  The kernel headers point here instead of restating it.
//
// x F^{(x)n} in natural order: x[j] ^= x[j + 2^s] for every j with bit s clear, s = 0 .. n - 1 (SCL_1024.c:242-250).  Inside
// a word the strides below 32 are shifts under a mask; the strides from 32 up are between words and belong to the caller.
#pragma once
#include <stdint.h>

namespace polar {

// x F^{(x)5} on the 32 elements of one word: stage s takes element j + 2^s into element j where bit s of j is clear
__host__ __device__ inline __attribute__((always_inline)) uint32_t polar_word_transform(uint32_t x)
{
    x ^= (x >> 1) & 0x55555555u;
    x ^= (x >> 2) & 0x33333333u;
    x ^= (x >> 4) & 0x0F0F0F0Fu;
    x ^= (x >> 8) & 0x00FF00FFu;
    x ^= (x >> 16) & 0x0000FFFFu;
    return x;
}

// the first n <= 5 stages: x F^{(x)n} on every aligned group of 2^n elements (N <= 32: the whole row is the low 2^n bits)
__host__ __device__ inline __attribute__((always_inline)) uint32_t polar_word_transform_n(uint32_t x, int n)
{
    for (int s = 0; s < n; ++s) {
        const uint32_t msk = (s == 0) ? 0x55555555u : (s == 1) ? 0x33333333u : (s == 2) ? 0x0F0F0F0Fu
                           : (s == 3) ? 0x00FF00FFu : 0x0000FFFFu;
        x ^= (x >> (1 << s)) & msk;
    }
    return x;
}

// updateBit below level 5 (SCL_1024.c:424-448), h = 2^t.  A right child of level t is done: its sums cur0 (bits 0 .. h - 1)
// and the saved left child's (level t of bl0: bits h .. 2h - 1) give level t + 1, (l ^ c, c), at bits 0 .. 2h - 1
__host__ __device__ inline __attribute__((always_inline)) uint32_t ps_fold0(uint32_t bl0, uint32_t cur0, int t)
{
    const int h = 1 << t;
    const uint32_t mask = (1u << h) - 1u;
    const uint32_t l = (bl0 >> h) & mask;
    const uint32_t c = cur0 & mask;
    return (l ^ c) | (c << h);
}

// A left child of level t is done: its sums cur0 (bits 0 .. h - 1) become level t of bl0, the other levels stay
__host__ __device__ inline __attribute__((always_inline)) uint32_t ps_save0(uint32_t bl0, uint32_t cur0, int t)
{
    const int h = 1 << t;
    const uint32_t mask = (1u << h) - 1u;
    return (bl0 & ~(mask << h)) | ((cur0 & mask) << h);
}

}  // namespace polar
