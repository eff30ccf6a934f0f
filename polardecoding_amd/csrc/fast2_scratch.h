// fast2_scratch.h -- the order of the elements inside a level-7 / level-8 row of the pair kernel's scratch (scl_fast2.h).
//
// A lane of the pair kernel holds the elements e = pos + 4 rr of a row (pos = lane & 3, pass rr), so a path's four lanes
// read 32 contiguous bytes per f64 pass and the two elements a lane wants in consecutive passes, e0 and e0 + 4, lie 32 bytes
// apart: every scratch access was 8 bytes wide.  The scratch-level steps wait on memory requests, not on bytes (DESIGN.md
// 4.0), so the rows are stored in the order
//
//     sigma(e) = (e & ~7) | ((e & 3) << 1) | ((e >> 2) & 1)
//
// which swaps, inside every block of 8 elements, the bit that tells the passes 2m / 2m + 1 apart with the two bits of pos:
// sigma(pos + 8m) = 8m + 2 pos, sigma(pos + 8m + 4) = 8m + 2 pos + 1.  A lane's pair of passes is one aligned 16-byte (f32:
// 8-byte) access, a path's four lanes cover 64 contiguous bytes, and sigma(e + 8k) = sigma(e) + 8k: the + 64k, + 128 and
// + 32k strides of the readers pass through.  A row stays contiguous and private to its slot.
//
// The top-left level and the channel rows keep their order (a codeword's 32 lanes read 256 contiguous bytes of them).
// The f64 kernels use the order (Fast2Cfg::PAIRED); the f32 kernels keep element order and 4-byte accesses, where the
// permuted rows measured slower with 8-byte pairs and without.
//
// Plain constexpr functions: the kernel, the host and tests/test_fast2_scratch_order_host.py see the same statement, and
// the static_asserts below hold its properties over both row lengths, both element sizes and every pos.
#pragma once

namespace polar {
namespace fast2_scratch {

constexpr int ROW8 = 256, ROW7 = 128, SLOTS = 8;   // elements of a level-8 / level-7 row; rows per level and codeword
constexpr int ROW6 = 64, TL = 512;                 // the level-6 rows (not used) and the top-left level
// element offsets inside a codeword's scratch, and its size
constexpr int SC_L8 = 0;
constexpr int SC_L7 = SC_L8 + SLOTS * ROW8;
constexpr int SC_L6 = SC_L7 + SLOTS * ROW7;
constexpr int SC_TL = SC_L6 + SLOTS * ROW6;
constexpr int SCRATCH_CW = SC_TL + TL;

// storage index of element e of a level-7 / level-8 row
constexpr unsigned sigma(unsigned e) { return (e & ~7u) | ((e & 3u) << 1) | ((e >> 2) & 1u); }
// storage index of the pair (pos + 8m, pos + 8m + 4): the elements of lane pos in the passes 2m and 2m + 1
constexpr unsigned pair_at(unsigned pos, unsigned m) { return 8u * m + 2u * pos; }

constexpr bool bijection(int n)
{
    for (int s = 0; s < n; ++s) {
        int hits = 0;
        for (int e = 0; e < n; ++e) hits += sigma((unsigned)e) == (unsigned)s;
        if (hits != 1) return false;
    }
    return true;
}
// passes 2m, 2m + 1 of every lane: adjacent, the first at an index that is a multiple of two elements, and where pair_at says
constexpr bool pairs_adjacent_and_aligned(int n, int elem_bytes)
{
    for (unsigned pos = 0; pos < 4; ++pos)
        for (unsigned m = 0; 8 * m < (unsigned)n; ++m) {
            const unsigned a = sigma(pos + 8 * m), b = sigma(pos + 8 * m + 4);
            if (b != a + 1 || a % 2 || a != pair_at(pos, m)) return false;
            if ((a * (unsigned)elem_bytes) % (2u * (unsigned)elem_bytes)) return false;
        }
    return true;
}
// the four lanes of a path, two passes: 8 consecutive elements from a multiple of 8
constexpr bool path_covers_a_block(int n)
{
    for (unsigned m = 0; 8 * m < (unsigned)n; ++m) {
        unsigned seen = 0;
        for (unsigned pos = 0; pos < 4; ++pos)
            for (unsigned h = 0; h < 2; ++h) {
                const unsigned s = sigma(pos + 8 * m + 4 * h);
                if (s < 8 * m || s >= 8 * m + 8) return false;
                seen |= 1u << (s - 8 * m);
            }
        if (seen != 0xFFu) return false;
    }
    return true;
}
// the readers' strides pass through: sigma(e + 8k) = sigma(e) + 8k
constexpr bool strides_pass_through(int n)
{
    for (int e = 0; e < 8; ++e)
        for (int k = 0; 8 * k + e < n; ++k)
            if (sigma((unsigned)(e + 8 * k)) != sigma((unsigned)e) + 8u * (unsigned)k) return false;
    return true;
}
constexpr bool rows_pair_aligned()
{
    return SC_L8 % 2 == 0 && SC_L7 % 2 == 0 && SCRATCH_CW % 2 == 0 && ROW8 % 2 == 0 && ROW7 % 2 == 0;
}
static_assert(bijection(ROW7) && bijection(ROW8), "sigma is not a bijection on a row");
static_assert(pairs_adjacent_and_aligned(ROW7, 8) && pairs_adjacent_and_aligned(ROW8, 8) && pairs_adjacent_and_aligned(ROW7, 4) &&
                  pairs_adjacent_and_aligned(ROW8, 4),
              "a lane's two passes are not one aligned pair");
static_assert(path_covers_a_block(ROW7) && path_covers_a_block(ROW8), "a path's four lanes do not cover 8 consecutive elements");
static_assert(strides_pass_through(ROW7) && strides_pass_through(ROW8), "sigma(e + 8k) != sigma(e) + 8k");
static_assert(rows_pair_aligned(), "a row does not start at a multiple of two elements");

}  // namespace fast2_scratch
}  // namespace polar
