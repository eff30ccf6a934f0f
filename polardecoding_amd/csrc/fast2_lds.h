// fast2_lds.h -- where the pair kernel (scl_fast2.h) keeps its partial-sum rows in LDS.
//
// LDS serves a wave64 access in fixed lane groups, one cycle per group when no two lanes of the group want different
// addresses in one bank; every further address on a busy bank costs the group one more cycle.  The 4-byte accesses go in
// two groups of 32 lanes over 32 banks of a dword.  A lane of the pair kernel is (slot p = lane / 8, codeword c, pos): a
// 32-lane group holds four slots of both codewords.
//
// Rows.  The saved and the working partial sums are one row of NW = 32 words per (codeword, slot).  Rows that start at
// multiples of 32 words put word w of all eight rows of a group into ONE bank: every access by own row was 8-way.  Here a
// row starts at word row(slot) behind its codeword's base cw_base(c): 36 words per slot and 16 more for the second
// codeword, so the eight rows of a group start in the banks 0, 4, .. 28 -- word w of each in a bank of its own, and the
// four-word windows w0 + pos side by side over all 32 banks.  The rows a lane reaches through a pointer (pb(t)) can be any
// eight of the sixteen: two of those share a bank at most.
//
// The staircase table keeps its 48-byte cells (polar_lut.h).  Three arrays thr[c], T_lo[c], T_hi[c] halve its bank
// conflicts in tools/lds_bank_model.py and measured 1.6 % SLOWER (f32 1.9 %): a third LDS instruction per look-up costs more
// than the conflicts it saves.
//
// Plain constexpr functions: the kernel, the host and tools/lds_bank_model.py see the same statement, and the
// static_asserts below hold the bank properties over all slots, codewords and word windows.
#pragma once

namespace polar {
namespace fast2_lds {

// ---- partial-sum rows -------------------------------------------------------------------------------------------------
constexpr int NW = 32, SLOTS = 8, CWS = 2, BANKS32 = 32;
constexpr int ROW_STRIDE = 36;                               // words from one slot's row to the next
constexpr int CW_BASE = SLOTS * ROW_STRIDE + 16;             // words from codeword 0's rows to codeword 1's
constexpr int ROWS_WORDS = CW_BASE + SLOTS * ROW_STRIDE;     // one array of rows (both codewords)
constexpr int row(int slot) { return slot * ROW_STRIDE; }    // word offset of a slot's row behind cw_base(c)
constexpr int cw_base(int c) { return c * CW_BASE; }

constexpr bool rows_fit()
{
    if (ROW_STRIDE % 4 || CW_BASE % 4) return false;   // 16-byte aligned rows
    for (int s = 0; s + 1 < SLOTS; ++s)
        if (row(s) + NW > row(s + 1)) return false;
    return row(SLOTS - 1) + NW <= cw_base(1) && cw_base(1) + row(SLOTS - 1) + NW <= ROWS_WORDS;
}
// a 32-lane group g holds the slots 4g .. 4g+3 of both codewords.  Own rows: word w of the eight rows in eight banks, and
// the window w0 + pos (pos = 0..3; w0 any word: set_bit_lds reads at nw + w) of the eight rows in 32 banks
constexpr bool own_rows_conflict_free()
{
    for (int g = 0; g < 2; ++g)
        for (int w0 = 0; w0 + 4 <= NW; ++w0) {
            unsigned same = 0, window = 0;
            for (int c = 0; c < CWS; ++c)
                for (int s = 4 * g; s < 4 * g + 4; ++s) {
                    const unsigned b = 1u << ((cw_base(c) + row(s) + w0) % BANKS32);
                    if (same & b) return false;
                    same |= b;
                    for (int pos = 0; pos < 4; ++pos) {
                        const unsigned bw = 1u << ((cw_base(c) + row(s) + w0 + pos) % BANKS32);
                        if (window & bw) return false;
                        window |= bw;
                    }
                }
        }
    return true;
}
// rows by pointer: whichever rows the lanes of a group read (word w, or the window w0 + pos), the rows that meet in one
// bank; 2 = no worse than 2-way
constexpr int pointer_rows_worst()
{
    int worst = 0;
    for (int w0 = 0; w0 + 4 <= NW; ++w0)
        for (int bank = 0; bank < BANKS32; ++bank) {
            int same = 0, window = 0;
            for (int c = 0; c < CWS; ++c)
                for (int s = 0; s < SLOTS; ++s) {
                    const int a = cw_base(c) + row(s) + w0;
                    if (a % BANKS32 == bank) ++same;
                    for (int pos = 0; pos < 4; ++pos)
                        if ((a + pos) % BANKS32 == bank) ++window;
                }
            worst = same > worst ? same : worst;
            worst = window > worst ? window : worst;
        }
    return worst;
}
static_assert(rows_fit(), "partial-sum rows overlap or are not 16-byte aligned");
static_assert(own_rows_conflict_free(), "a group's own rows share a bank");
static_assert(pointer_rows_worst() <= 2, "pointer rows are worse than 2-way");

}  // namespace fast2_lds
}  // namespace polar
