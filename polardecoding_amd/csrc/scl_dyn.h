// scl_dyn.h -- SC / SCL / CA-SCL with dynamic frozen bits (include/polar_hip.h, "Dynamic frozen bits"): PAC codes, the
// parity-check bits of 5G PC-polar codes, any lower-triangular precoding.
//
// k_scl_dyn is scl_generic.h's scl_generic_body with DYN = true.  What DYN adds to k_scl_generic:
//
//     hist[L][N/32]            per path, bit j set once u_hat_j = 1 was decided.  Word 0 lives in a register (h0, shuffled
//                              with the path like bl0); words 1.. live in LDS behind cand and are copied with blw on every
//                              fork and refill.  For N = 32 the history is that one register.
//     P.row[N]                 row index of leaf j in the constraint matrix, -1 = not dynamic (wave-uniform)
//     P.mask[D][N/32]          dense rows: bit i of row d set <=> i is in S_{pos[d]}
//
// At a dynamic leaf the S lanes of a path AND / popcount their share of the words 0 .. j >> 5 of (hist, mask row), the
// parities are XOR-reduced over the S lanes, and the path continues with that bit: no fork, no ranking, no tie flag; in the
// list modes PM takes PHI(lambda, b) with the rounding of an information leaf's branch b.  The reduction sits in
// wave-uniform control flow (j and the row index are wave-uniform); lanes of dead paths compute and discard.  The output
// row is the chosen path's history, so the final u = x F^{(x)n} transform is not run.
#pragma once
#include "scl_generic.h"

namespace polar {

struct DynParams {
    SclParams s;
    const uint32_t *mask;   // [D][N/32]
    const int *row;         // [N]: row of leaf j, or -1
};

template <typename R, typename IN, int LOGL, bool GA>
__global__ __launch_bounds__(64) void k_scl_dyn(DynParams DP)
{
    scl_generic_body<R, IN, LOGL, GA, true>(DP.s, DP.mask, DP.row);
}

template <typename R, int LOGL>
constexpr size_t scl_dyn_lds_bytes(int N, bool ga)
{
    return scl_generic_lds_bytes<R, LOGL>(N, ga) + sizeof(uint32_t) * (size_t)(N / 32) * (1 << LOGL);
}

}  // namespace polar
