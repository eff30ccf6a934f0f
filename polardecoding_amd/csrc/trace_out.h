// trace_out.h -- what the TRACE hook and epilogue of scl_generic_body / k_scl_wide read and write (include/polar_hip.h,
// "Sent-path trace"): the sent word per frame, and five words per frame -- flags go to SclParams::flags as in every decode.
//
// TRACE keeps one flag per slot, `match`: the slot's decided bits 0 .. j equal the sent ones.  It moves with the path wherever
// crc / h0 move and is ANDed with (bit == sent_j) after every decision; sent_j is a bit of the frame's sent word j >> 5, loaded
// once per 32 leaves and uniform for the workgroup.  The leaf after whose decision no live slot carries the flag is the loss
// leaf; at a ranking leaf the count n0 / n1 of the sent candidate, the number the survivor test compares with L, is kept for it.
#pragma once
#include <stdint.h>

namespace polar {

struct TraceOut {
    const uint32_t *u;      // [B][N/32] the sent u, packed like the decisions
    int32_t *loss_leaf;     // [B] or null: the first leaf after which no live slot matches, N if there is none
    uint32_t *loss_rank;    // [B] or null: #{m < 2L : c_m <= c_sent} at a ranking loss leaf, else 0
    int32_t *rank;          // [B] or null: rank of the sent word in the final list (ascending (PM, slot)), -1 if it is not there
    int32_t *chosen;        // [B] or null: rank of the path the ordinary decode returns
};

// sent bit of leaf j from the word loaded at the last j with (j & 31) == 0
__device__ __forceinline__ int trace_sent_bit(uint32_t word, int j) { return (int)((word >> (j & 31)) & 1u); }

// one lane (thread) per frame writes the words that are asked for
__device__ __forceinline__ void trace_write(const TraceOut &T, int frame, int loss_leaf, uint32_t loss_rank, int rank, int chosen)
{
    if (T.loss_leaf) T.loss_leaf[frame] = loss_leaf;
    if (T.loss_rank) T.loss_rank[frame] = loss_rank;
    if (T.rank) T.rank[frame] = rank;
    if (T.chosen) T.chosen[frame] = chosen;
}

}  // namespace polar
