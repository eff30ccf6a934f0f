// list_kernel.h -- what works on a list that polar_list_decode wrote (include/polar_hip.h, "List output"):
//
//     k_scl_list                     the LIST = true wrapper of scl_generic_body (L <= 32); for L = 64 .. 256 the LIST = true
//                                    instantiations of k_scl_wide (scl_wide.h, where ListParams lives)
//     k_list_select                  per (frame, mask): the first rank whose remainder equals the mask
//     k_list_gather                  per frame: the row of the list an index names
//     k_list_soft                    per frame: max-log LLRs over the list, in the u or in the x domain
//
// The list is sorted by rule 3 (ascending (PM, slot), padding behind count), so "first rank" is "least metric".
#pragma once
#include "scl_wide.h"

namespace polar {

template <typename R, typename IN, int LOGL, bool GA>
__global__ __launch_bounds__(64) void k_scl_list(ListParams LP)
{
    scl_generic_body<R, IN, LOGL, GA, true, true>(LP.d.s, LP.d.mask, LP.d.row, &LP.o);
}

// one thread per (frame, mask): idx[f][m] = the smallest k < min(count[f], L) with rem[f][k] == masks[m], else -1
__global__ __launch_bounds__(256) void k_list_select(const uint32_t *rem, const uint32_t *count, const uint32_t *masks, int L, int M,
                                                     size_t total, int32_t *idx)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t f = t / (size_t)M;
    const uint32_t want = masks[t - f * (size_t)M];
    const uint32_t cnt = count[f];
    const int c = cnt < (uint32_t)L ? (int)cnt : L;
    const uint32_t *r = rem + f * (size_t)L;
    int32_t k = -1;
    for (int q = c - 1; q >= 0; --q)
        if (r[q] == want) k = q;
    idx[t] = k;
}

// one thread per output word: out[f][w] = paths[f][k][w], k = idx[f * stride]; an index outside 0 .. L - 1 (-1: "none") is rank 0
__global__ __launch_bounds__(256) void k_list_gather(const uint32_t *paths, const int32_t *idx, int stride, int L, int NW, size_t total,
                                                     uint32_t *out)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t f = t / (size_t)NW;
    const int w = (int)(t - f * (size_t)NW);
    int32_t k = idx[f * (size_t)stride];
    if (k < 0 || k >= L) k = 0;
    out[t] = paths[(f * (size_t)L + (size_t)k) * NW + w];
}

struct ListSoftParams {
    const uint32_t *paths;   // [B][L][NW]
    const double *pm;        // [B][L]
    const uint32_t *count;   // [B]
    const uint32_t *rem;     // [B][L] or null
    uint32_t want_rem;
    int domain;              // 0: u, 1: x = u F^{(x)n}
    double clamp;
    int N, n, L, B;
    double *out;             // [B][N]
};

constexpr size_t list_soft_lds_bytes(int N, int L)
{
    return (size_t)L * (N / 32) * sizeof(uint32_t) + (size_t)L * (sizeof(double) + sizeof(int));
}

// One wavefront per frame.  The packed rows of the frame's candidates are read once, in consecutive words, into LDS
// (rows[c][NW], compacted: tgt[k] is the row of rank k, -1 for a rank that is no candidate), their metrics beside them;
// domain 1 turns every row into its codeword in place with the butterfly of the decode kernels' epilogue.  Then lane l takes
// the positions l, l + 64, ...: for each it walks the candidates (the 32 lanes of a half-wave read the same LDS word: a
// broadcast), keeps the least metric per bit value, and writes one double, so a wavefront's store covers 512 consecutive
// bytes of the row.
__global__ __launch_bounds__(64) void k_list_soft(ListSoftParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = P.N, NW = N >> 5, L = P.L;
    const int lane = threadIdx.x;
    double *cpm = reinterpret_cast<double *>(smem);
    int *tgt = reinterpret_cast<int *>(cpm + L);
    uint32_t *rows = reinterpret_cast<uint32_t *>(tgt + L);
    for (int f = blockIdx.x; f < P.B; f += (int)gridDim.x) {
        const uint32_t cnt_in = P.count[f];
        const int cnt = cnt_in < (uint32_t)L ? (int)cnt_in : L;
        const size_t fb = (size_t)f * L;
        // the candidate set: the ranks below count with the wanted remainder; all ranks below count if there is none (or no d_rem)
        bool any = false;
        if (P.rem) {
            bool mine = false;
            for (int k = lane; k < cnt; k += 64) mine |= P.rem[fb + k] == P.want_rem;
            any = __ballot(mine) != 0ull;
        }
        int nc = 0;   // candidates kept so far (wave-uniform)
        for (int k0 = 0; k0 < cnt; k0 += 64) {
            const int k = k0 + lane;
            const bool is = k < cnt && (!any || P.rem[fb + k] == P.want_rem);
            const uint64_t m = __ballot(is);
            const int c = nc + __popcll(m & ((1ull << lane) - 1ull));
            if (is) cpm[c] = P.pm[fb + k];
            if (k < cnt) tgt[k] = is ? c : -1;
            nc += __popcll(m);
        }
        __syncthreads();
        for (int i = lane; i < cnt * NW; i += 64) {
            const int k = i / NW, c = tgt[k];
            if (c >= 0) rows[c * NW + (i - k * NW)] = P.paths[fb * NW + i];
        }
        __syncthreads();
        if (P.domain == 1) {
            for (int i = lane; i < nc * NW; i += 64) rows[i] = polar_word_transform(rows[i]);
            __syncthreads();
            for (int s = 5; s < P.n; ++s) {
                const int hw = 1 << (s - 5);
                for (int i = lane; i < nc * NW; i += 64)
                    if (!((i % NW) & hw)) rows[i] ^= rows[i + hw];
                __syncthreads();
            }
        }
        for (int j = lane; j < N; j += 64) {
            double m0 = 0.0, m1 = 0.0;
            bool has0 = false, has1 = false;
            const int w = j >> 5, sh = j & 31;
            for (int c = 0; c < nc; ++c) {
                const bool b = (rows[c * NW + w] >> sh) & 1u;
                const double v = cpm[c];
                if (b) {
                    if (!has1 || v < m1) m1 = v;
                    has1 = true;
                } else {
                    if (!has0 || v < m0) m0 = v;
                    has0 = true;
                }
            }
            double o;
            if (!has1) o = P.clamp;          // also the empty list (count = 0)
            else if (!has0) o = -P.clamp;
            else {
                o = m1 - m0;
                if (o < -P.clamp) o = -P.clamp;
                if (o > P.clamp) o = P.clamp;
            }
            P.out[(size_t)f * N + j] = o;
        }
        __syncthreads();
    }
}

}  // namespace polar
