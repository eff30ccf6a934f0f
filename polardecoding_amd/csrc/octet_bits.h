// octet_bits.h -- the partial sums inside one octet of the pair kernel (scl_fast2.h), formed from the octet's raw bits.
//
// Bits 0..7 of a path's word bl0 hold the decided bits u_0 .. u_7 of the current octet as they are (0 where the leaf is
// frozen or not reached yet).  The sums the decoder needs are those of u F^{(x)3} over a prefix of the octet, and they are
// read three times per octet (the level-1 g before leaves 2 and 6, the level-2 g before leaf 4) plus once at leaf 7 (the
// octet's level-3 word), so they are formed where they are read: a stage of the transform is one shift and one
// xor-under-mask, and the mask selects the pairs the reader wants.  Plain constexpr functions: the kernel and the host
// see the same statement, and the static_asserts below hold it, for all 256 bytes, to the form that stored every
// intermediate sum after every leaf (restated here as stored_step / stored_c3) and to the sums spelled out bit by bit.
#pragma once
#include <cstdint>

namespace polar {
namespace octet_bits {

// stage S of the transform on the pairs `mask` selects: bit i (in mask) becomes x_i ^ x_{i + 2^S}
template <int S>
constexpr uint32_t stage(uint32_t x, uint32_t mask) { return x ^ ((x >> (1 << S)) & mask); }

// level 1 above leaves 0, 1: (u0 ^ u1, u1) at bits 0, 1 -- the g step before leaf 2 reads bit pos
constexpr uint32_t level1_lo(uint32_t b) { return stage<0>(b, 0x01u); }
// level 1 above leaves 4, 5: (u4 ^ u5, u5), shifted down to bits 0, 1 -- the g step before leaf 6 reads bit pos as well
// (read in place at bit 4 + pos, that shift amount is one more per-lane constant across the octet loop: ten more
// spilled VGPRs in the f64 kernels)
constexpr uint32_t level1_hi(uint32_t b) { return level1_lo(b >> 4); }
// level 2 above leaves 0..3: (u0^u1^u2^u3, u1^u3, u2^u3, u3) at bits 0..3 -- the g step before leaf 4 reads bit pos
constexpr uint32_t level2(uint32_t b) { return stage<1>(stage<0>(b, 0x05u), 0x03u); }
// level 3: the octet's eight sums at bits 0..7 (leaf 7; set_bit7 carries them on).  Only bits 0..7 of b are read and changed.
constexpr uint32_t level3(uint32_t b) { return stage<2>(stage<1>(stage<0>(b, 0x55u), 0x33u), 0x0Fu); }

// ---- the stored-sum form, as a reference for the asserts: after leaf K the word holds the last even leaf's bit at bit 1,
// the last finished pair's level-1 sums at bits 2, 3 and the first half's level-2 sums at bits 4..7; leaf 7 yields c3 ----
constexpr uint32_t stored_step(uint32_t w, int K, uint32_t bit)
{
    const uint32_t c1 = (((w >> 1) & 1u) ^ bit) | (bit << 1);
    const uint32_t c2 = (((w >> 2) & 3u) ^ c1) | (c1 << 2);
    if ((K & 1) == 0) return (w & ~2u) | (bit << 1);
    if ((K & 3) == 1) return (w & ~0xCu) | (c1 << 2);
    return (w & ~0xF0u) | (c2 << 4);   // K == 3
}
constexpr uint32_t stored_c3(uint32_t w, uint32_t bit)   // K == 7
{
    const uint32_t c1 = (((w >> 1) & 1u) ^ bit) | (bit << 1);
    const uint32_t c2 = (((w >> 2) & 3u) ^ c1) | (c1 << 2);
    return (((w >> 4) & 15u) ^ c2) | (c2 << 4);
}

constexpr uint32_t bit_of(uint32_t x, int k) { return (x >> k) & 1u; }

// every reader of the raw form sees what the stored form held at that point, for every byte u (a frozen leaf is a 0 bit)
constexpr bool equals_stored_form()
{
    for (uint32_t u = 0; u < 256; ++u) {
        uint32_t w = 0;
        for (int K = 0; K < 7; ++K) {
            const uint32_t raw = u & ((1u << K) - 1u);   // the raw bits in front of leaf K
            if (K == 2 && (level1_lo(raw) & 3u) != ((w >> 2) & 3u)) return false;
            if (K == 4 && (level2(raw) & 15u) != ((w >> 4) & 15u)) return false;
            if (K == 6 && (level1_hi(raw) & 3u) != ((w >> 2) & 3u)) return false;
            w = stored_step(w, K, bit_of(u, K));
            if ((K & 1) == 0 && bit_of(u & ((2u << K) - 1u), K) != bit_of(w, 1)) return false;   // the odd leaf's partner bit
        }
        if ((level3(u) & 0xFFu) != stored_c3(w, bit_of(u, 7))) return false;
        if (level3(u | 0xABCD00u) != ((level3(u) & 0xFFu) | 0xABCD00u)) return false;   // bits 8 and up pass through
    }
    return true;
}
// ... and the sums themselves, bit by bit
constexpr bool equals_spelled_out_sums()
{
    for (uint32_t u = 0; u < 256; ++u) {
        const uint32_t u0 = bit_of(u, 0), u1 = bit_of(u, 1), u2 = bit_of(u, 2), u3 = bit_of(u, 3);
        const uint32_t u4 = bit_of(u, 4), u5 = bit_of(u, 5), u6 = bit_of(u, 6), u7 = bit_of(u, 7);
        const uint32_t lo = level1_lo(u), hi = level1_hi(u), l2 = level2(u), l3 = level3(u);
        if (bit_of(lo, 0) != (u0 ^ u1) || bit_of(lo, 1) != u1) return false;
        if (bit_of(hi, 0) != (u4 ^ u5) || bit_of(hi, 1) != u5) return false;
        if (bit_of(l2, 0) != (u0 ^ u1 ^ u2 ^ u3) || bit_of(l2, 1) != (u1 ^ u3) || bit_of(l2, 2) != (u2 ^ u3) || bit_of(l2, 3) != u3)
            return false;
        const uint32_t want[8] = {u0 ^ u1 ^ u2 ^ u3 ^ u4 ^ u5 ^ u6 ^ u7, u1 ^ u3 ^ u5 ^ u7, u2 ^ u3 ^ u6 ^ u7, u3 ^ u7,
                                  u4 ^ u5 ^ u6 ^ u7, u5 ^ u7, u6 ^ u7, u7};
        for (int k = 0; k < 8; ++k)
            if (bit_of(l3, k) != want[k]) return false;
    }
    return true;
}
static_assert(equals_stored_form(), "the raw-bit readers differ from the stored partial sums");
static_assert(equals_spelled_out_sums(), "a mask of the octet transform is wrong");

}  // namespace octet_bits
}  // namespace polar
