// scl_wave_ops.h -- the steps of the one-wavefront-per-codeword list layout, written once.
//
// The layout: a workgroup is one 64-lane wavefront and decodes one codeword; lane = (slot p = lane / S, position pos =
// lane % S), S = 64 / L.  A slot's bit-packed rows are blw[p * NW + w] (saved left-child sums) and curw[p * NW + w] (working
// sums) in LDS, NW = N / 32, packed as polar_bits.h says; word 0 of both lives in registers (bl0, cur0).  State moves between
// slots with __shfl / __ballot.  scl_generic_body (scl_generic.h) and k_scl_q8 (scl_q8.h) take every step below;
// k_scl_big (scl_big.h) takes the pointer tables.
//
// Not here: the scan "least metric among the CRC-passing paths" behind the last leaf.  Generic, q8 and big each keep their
// copy: as a function the loop compiles differently from the in-place text, and that moved k_scl_big's whole instruction
// stream and took four k_scl_dyn instantiations (L = 2, f64) from 64 / 71 to 67 / 73 VGPRs, one wavefront per SIMD less
// (DESIGN.md 4.17).  The rule the copies share: strict <, so the first slot wins a tie; all live slots when none passes.
#pragma once
#include "polar_math.h"
#include "polar_bits.h"

namespace polar {

// per-level pointer table: LOGL bits per level, the slot whose buffer holds level t of this path
template <int LOGL>
__device__ __forceinline__ int ptr_get(uint64_t tbl, int t)
{
    if (LOGL == 0) return 0;
    return (int)((tbl >> (t * LOGL)) & ((1u << LOGL) - 1));
}
template <int LOGL>
__device__ __forceinline__ uint64_t ptr_set(uint64_t tbl, int t, int v)
{
    if (LOGL == 0) return 0;
    const uint64_t m = (uint64_t)((1u << LOGL) - 1) << (t * LOGL);
    return (tbl & ~m) | ((uint64_t)v << (t * LOGL));
}

// The m-th both-survivor (ascending slot) forks into the m-th dead slot (SCL_1024.c:636-661).  m_both / m_dead: ballots over
// the slots' leading lanes.  A dead slot with a both-survivor of its rank gets that slot in sg and true; every other slot
// keeps sg and gets false (a dead slot does when a median tie left fewer both-survivors than dead slots).
template <int S>
__device__ __forceinline__ bool fork_source(uint64_t m_both, uint64_t m_dead, int p, bool dead, int &sg)
{
    const int myrank = __popcll(m_dead & ((1ull << (p * S)) - 1ull));
    int src = sg;
    bool refilled = false;
    uint64_t bm = m_both;
    int cnt = 0;
    while (bm) {
        const int b = __builtin_ctzll(bm);
        if (dead && cnt == myrank) {
            src = b / S;
            refilled = true;
        }
        bm &= bm - 1;
        ++cnt;
    }
    sg = src;
    return refilled;
}

// updateBit at a level t >= 5 (SCL_1024.c:424-448; below 5: ps_fold0 / ps_save0).  A right child of level t is done:
// cur (words 0 .. nw - 1, nw = 2^(t-5)) and the saved left child (words nw .. 2 nw - 1 of blw) give level t + 1 in words
// 0 .. 2 nw - 1 of curw.  At t = 5 cur0 enters LDS first.  Barriers in uniform control flow; slot p holds a path iff p < act.
template <int S>
__device__ __forceinline__ void ps_update_rows(const uint32_t *blw, uint32_t *curw, int NW, int p, int pos, int act,
                                               uint32_t cur0, int t)
{
    const int nw = 1 << (t - 5);
    if (t == 5) {
        if (pos == 0 && p < act) curw[p * NW] = cur0;
        __syncthreads();
    }
    if (p < act) {
        for (int w = pos; w < nw; w += S) {
            const uint32_t c = curw[p * NW + w];
            const uint32_t l = blw[p * NW + nw + w];
            curw[p * NW + w] = l ^ c;
            curw[p * NW + w + nw] = c;
        }
    }
    __syncthreads();
}

// A left child of level t >= 5 is done: its sums (cur0 at t = 5, else words 0 .. nw - 1 of curw) become level t of blw
template <int S>
__device__ __forceinline__ void ps_save_rows(uint32_t *blw, const uint32_t *curw, int NW, int p, int pos, int act,
                                             uint32_t cur0, int t)
{
    const int nw = 1 << (t - 5);
    if (t == 5) {
        if (pos == 0 && p < act) blw[p * NW + 1] = cur0;
    } else if (p < act) {
        for (int w = pos; w < nw; w += S) blw[p * NW + nw + w] = curw[p * NW + w];
    }
    __syncthreads();
}

// u_hat = x_hat F^{(x)n} for N > 32, in place on the NW words of the chosen path's root partial sums, then stored to out
__device__ __forceinline__ void uhat_from_rows(uint32_t *xw, int NW, int n, int lane, uint32_t *out)
{
    for (int w = lane; w < NW; w += 64) xw[w] = polar_word_transform(xw[w]);
    __syncthreads();
    for (int s = 5; s < n; ++s) {
        const int hw = 1 << (s - 5);
        for (int w = lane; w < NW; w += 64)
            if (!(w & hw)) xw[w] ^= xw[w + hw];
        __syncthreads();
    }
    for (int w = lane; w < NW; w += 64) out[w] = xw[w];
}

}  // namespace polar
