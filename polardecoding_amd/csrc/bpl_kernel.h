// bpl_kernel.h -- device glue of the BP list decoder over permuted factor graphs (POLAR_ALGO_BPL, include/polar_hip.h).
//
// An attempt is the BP kernel of the ctx (k_bp*.hip, stop rule G), unchanged, on a permuted row with a permuted frozen
// mask; what runs around it is here and in adaptive_kernel.h:
//   k_bpl_gather     dst[k][j] = src[idx ? idx[k] : base + k][sigma[j]]: the compaction gather of k_ad_gather and the
//                    permutation in one pass over the caller's input.  The writes are consecutive; the reads of one row
//                    (at most 32 KiB) are a permutation of index bits, a power-of-two stride that the L2 serves: a row is
//                    read exactly once, by one pass of consecutive threads, so no LDS staging.
//   k_bpl_scatter    un-permutes the packed decisions of an attempt (sigma mixes index bits below and above bit 5, so a
//                    word of the output collects bits of up to 32 words of the attempt) and writes bits, iters, flags and
//                    graph of the accepted frames to their original index (attempt 0: of every frame); adds the attempt's
//                    round trips to total_iters for every frame it ran.
//   k_ad_crc_check, k_ad_fail_count/scan/write (adaptive_kernel.h): the CRC of an attempt's decisions against the permuted
//                    table, and the stable compaction of the frames that are still open.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace polar {

constexpr int BPL_THREADS = 256;   // four wavefronts

// sigma: [N] uint16 (null: the identity); row = 1 << log_row elements of T; one element per thread
template <typename T>
__global__ __launch_bounds__(BPL_THREADS) void k_bpl_gather(const T *__restrict__ src, T *__restrict__ dst,
                                                           const uint32_t *__restrict__ idx, long long base,
                                                           const uint16_t *__restrict__ sigma, long long n, int log_row)
{
    const long long total = n << log_row;
    const long long row_mask = (1ll << log_row) - 1;
    for (long long t = (long long)blockIdx.x * BPL_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * BPL_THREADS) {
        const long long k = t >> log_row, j = t & row_mask;
        const long long f = idx ? (long long)idx[k] : base + k;
        dst[t] = src[(f << log_row) + (sigma ? (long long)sigma[j] : j)];
    }
}

// Entry k of an attempt's outputs (s_bits [n][NW] in the attempt's order, s_iters, s_flags) -> frame f = idx[k] (or base + k).
// The attempt accepts frame k iff (s_flags[k] & need) == need.  An accepted frame, and with `all` (attempt 0) every frame,
// gets u_hat[sigma(j)] = u'[j] -- sinv[j] = sigma^-1(j), null for the identity -- iters, flags and graph = p (Pn when it is
// written without being accepted: the fallback).  total[f] is set (all) or incremented by the round trips of the attempt.
// s_bits null: the attempt wrote bits, iters and flags in place (s_iters == iters, s_flags == flags); one thread per frame.
// One thread per output word otherwise; iters, flags, graph and total are nullable.
__global__ __launch_bounds__(BPL_THREADS) void k_bpl_scatter(const uint32_t *__restrict__ s_bits, const uint32_t *s_iters,
                                                            const uint32_t *s_flags, const uint32_t *__restrict__ idx,
                                                            long long base, long long n, int logNW,
                                                            const uint16_t *__restrict__ sinv, uint32_t need, uint32_t p,
                                                            uint32_t Pn, int all, uint32_t *__restrict__ bits,
                                                            uint32_t *iters, uint32_t *flags, uint32_t *__restrict__ graph,
                                                            uint32_t *__restrict__ total)
{
    const int lw = s_bits ? logNW : 0;
    const long long count = n << lw;
    const long long wmask = (1ll << lw) - 1;
    for (long long t = (long long)blockIdx.x * BPL_THREADS + threadIdx.x; t < count; t += (long long)gridDim.x * BPL_THREADS) {
        const long long k = t >> lw, w = t & wmask;
        const long long f = idx ? (long long)idx[k] : base + k;
        const uint32_t fl = s_flags[k];
        const bool acc = (fl & need) == need;
        const bool put = acc || all;
        if (s_bits && put) {
            const uint32_t *row = s_bits + (k << logNW);
            uint32_t v;
            if (sinv) {
                v = 0;
#pragma unroll 8
                for (int b = 0; b < 32; ++b) {
                    const uint32_t j = sinv[(w << 5) + b];
                    v |= ((row[j >> 5] >> (j & 31)) & 1u) << b;
                }
            } else {
                v = row[w];
            }
            bits[(f << logNW) + w] = v;
        }
        if (w == 0) {
            const uint32_t tp = s_iters[k];
            if (put) {
                if (iters) iters[f] = tp;
                if (flags) flags[f] = fl;
                if (graph) graph[f] = acc ? p : Pn;
            }
            if (total) total[f] = all ? tp : total[f] + tp;
        }
    }
}

}  // namespace polar
