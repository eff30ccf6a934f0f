// adaptive_kernel.h -- device glue of the adaptive CA-SCL decoder (polar_cascl_set_stages, include/polar_hip.h).
//
// The stage decoders are the existing kernels, unchanged; what runs between two stages is here:
//   k_ad_crc_check   CRC syndrome of packed SC decisions (first stage L = 1): POLAR_FLAG_CRC_PASS into the flags word
//   k_ad_fail_count  \
//   k_ad_fail_scan    > stable compaction of the frames whose flags lack a bit of `need` (POLAR_FLAG_CRC_PASS here; BP list
//   k_ad_fail_write  /  decoding, bpl_kernel.h, asks for its own bits) into an index list + count
//                       (wave64 ballot + mbcnt inside a block, one-block scan of the block counts; no atomics)
//   k_ad_gather      rows idx[k] of the caller's input -> a contiguous stage buffer (16-byte loads when aligned)
//   k_ad_scatter     a stage's packed decisions, metric, flags and list size -> the original frame indices
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace polar {

constexpr uint32_t AD_CRC_PASS = 0x2u;   // POLAR_FLAG_CRC_PASS
constexpr int AD_THREADS = 256;          // four wavefronts
constexpr int AD_ROUNDS = 8;             // compaction: rounds of AD_THREADS frames per block
constexpr int AD_CHUNK = AD_THREADS * AD_ROUNDS;
constexpr int AD_SCAN_THREADS = 1024;

__device__ __forceinline__ uint32_t ad_mbcnt(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Frame f passes iff XOR over {j : u_hat_j = 1} of crc_tab[j] == 0 (the test the list kernels apply as they decide,
// scl_generic.h).  One lane per decision word, G = min(NW, 64) lanes per frame, 64 / G frames per wavefront (N <= 2048);
// at N = 4096 a lane takes words w and w + 64.  crc_tab sits in LDS transposed, tabT[b][w] = crc_tab[32 w + b], so the
// lanes of a frame read consecutive words (the other frames of the wavefront read the same ones: broadcast).
// flags[f] |= POLAR_FLAG_CRC_PASS on a pass; the SC kernels have written the rest of the word.
__global__ __launch_bounds__(AD_THREADS) void k_ad_crc_check(const uint32_t *__restrict__ bits,
                                                             const uint32_t *__restrict__ crc_tab, uint32_t *flags,
                                                             int NW, int B)
{
    extern __shared__ uint32_t tabT[];   // [32][NW]
    const int N = NW * 32;
    for (int j = threadIdx.x; j < N; j += AD_THREADS) tabT[(j & 31) * NW + (j >> 5)] = crc_tab[j];
    __syncthreads();
    const int G = NW < 64 ? NW : 64;
    const int lane = threadIdx.x & 63;
    const int sub = lane & (G - 1), grp = lane / G;
    const int fpw = 64 / G;
    const long long wave = (long long)blockIdx.x * (AD_THREADS / 64) + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * (AD_THREADS / 64);
    for (long long f0 = wave * fpw; f0 < B; f0 += nwaves * fpw) {   // uniform per wavefront
        const long long f = f0 + grp;
        uint32_t acc = 0;
        if (f < B) {
            for (int w = sub; w < NW; w += 64) {
                const uint32_t x = bits[(size_t)f * NW + w];
#pragma unroll
                for (int b = 0; b < 32; ++b) acc ^= tabT[b * NW + w] & (0u - ((x >> b) & 1u));
            }
        }
        for (int o = 1; o < G; o <<= 1) acc ^= __shfl_xor(acc, o);
        if (f < B && sub == 0 && acc == 0u) flags[f] |= AD_CRC_PASS;
    }
}

// number of failing frames ((flags & need) != need) among the AD_CHUNK frames of each block
__global__ __launch_bounds__(AD_THREADS) void k_ad_fail_count(const uint32_t *__restrict__ flags, int n, uint32_t need,
                                                              uint32_t *__restrict__ blk_cnt)
{
    __shared__ uint32_t wsum[AD_THREADS / 64];
    const long long base = (long long)blockIdx.x * AD_CHUNK;
    uint32_t cnt = 0;
#pragma unroll
    for (int r = 0; r < AD_ROUNDS; ++r) {
        const long long i = base + r * AD_THREADS + threadIdx.x;
        const bool fail = i < n && (flags[i] & need) != need;
        cnt += (uint32_t)__popcll(__ballot(fail));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int k = 0; k < AD_THREADS / 64; ++k) s += wsum[k];
        blk_cnt[blockIdx.x] = s;
    }
}

// exclusive scan of the block counts (one workgroup, AD_SCAN_THREADS block counts per round); *count = the total
__global__ __launch_bounds__(AD_SCAN_THREADS) void k_ad_fail_scan(const uint32_t *__restrict__ blk_cnt, int nblk,
                                                                  uint32_t *__restrict__ blk_off, uint32_t *count)
{
    __shared__ uint32_t wtot[AD_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += AD_SCAN_THREADS) {
        const int i = b0 + threadIdx.x;
        const uint32_t v = i < nblk ? blk_cnt[i] : 0u;
        uint32_t x = v;   // inclusive scan over the wavefront
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wtot[wave] = x;
        __syncthreads();
        uint32_t woff = 0, tot = 0;
        for (int k = 0; k < AD_SCAN_THREADS / 64; ++k) {
            if (k < wave) woff += wtot[k];
            tot += wtot[k];
        }
        if (i < nblk) blk_off[i] = carry + woff + x - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

// idx_out[blk_off[block] + rank] = idx_in[i] (or i when idx_in is null) for every failing i, in ascending order of i
__global__ __launch_bounds__(AD_THREADS) void k_ad_fail_write(const uint32_t *__restrict__ flags,
                                                              const uint32_t *__restrict__ idx_in, int n, uint32_t need,
                                                              const uint32_t *__restrict__ blk_off,
                                                              uint32_t *__restrict__ idx_out)
{
    __shared__ uint32_t wcnt[AD_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = blk_off[blockIdx.x];
    const long long base = (long long)blockIdx.x * AD_CHUNK;
    for (int r = 0; r < AD_ROUNDS; ++r) {
        const long long i = base + r * AD_THREADS + threadIdx.x;
        const bool fail = i < n && (flags[i] & need) != need;
        const unsigned long long m = __ballot(fail);
        if (lane == 0) wcnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t woff = 0, tot = 0;
        for (int k = 0; k < AD_THREADS / 64; ++k) {
            if (k < wave) woff += wcnt[k];
            tot += wcnt[k];
        }
        if (fail) idx_out[carry + woff + ad_mbcnt(m)] = idx_in ? idx_in[i] : (uint32_t)i;
        carry += tot;
        __syncthreads();   // wcnt is rewritten by the next round
    }
}

// dst[k][v] = src[idx[k]][v] for k < n, v < row (elements of T; row a power of two), one element per thread
template <typename T>
__global__ __launch_bounds__(AD_THREADS) void k_ad_gather(const T *__restrict__ src, T *__restrict__ dst,
                                                          const uint32_t *__restrict__ idx, long long n, int log_row)
{
    const long long total = n << log_row;
    const long long row_mask = (1ll << log_row) - 1;
    for (long long t = (long long)blockIdx.x * AD_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * AD_THREADS) {
        const long long k = t >> log_row;
        dst[t] = src[((long long)idx[k] << log_row) + (t & row_mask)];
    }
}

// frame idx[k] of the outputs <- entry k of a stage's outputs: decisions [n][NW], metric, flags; list[idx[k]] = L
__global__ __launch_bounds__(AD_THREADS) void k_ad_scatter(const uint32_t *__restrict__ s_bits,
                                                           const double *__restrict__ s_pm,
                                                           const uint32_t *__restrict__ s_flags,
                                                           const uint32_t *__restrict__ idx, long long n, int logNW,
                                                           uint32_t *__restrict__ bits, double *__restrict__ pm,
                                                           uint32_t *__restrict__ flags, uint32_t *__restrict__ list,
                                                           uint32_t L)
{
    const long long total = n << logNW;
    const long long wmask = (1ll << logNW) - 1;
    for (long long t = (long long)blockIdx.x * AD_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * AD_THREADS) {
        const long long k = t >> logNW, w = t & wmask;
        const long long f = idx[k];
        bits[(f << logNW) + w] = s_bits[t];
        if (w == 0) {
            if (pm) pm[f] = s_pm[k];
            if (flags) flags[f] = s_flags[k];
            if (list) list[f] = L;
        }
    }
}

}  // namespace polar
