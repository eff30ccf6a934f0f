// genie_lanes.h -- Monte-Carlo code construction (Arikan 2009, section IX; include/polar_hip.h "Monte-Carlo construction").
//
// k_genie_lanes: genie-aided SC for the all-zero codeword, ONE CODEWORD PER LANE, modelled on k_sc_lanes (sc_lanes.h) but a
// kernel of its own.  Every leaf is treated as frozen to 0, so every g step is cL + cU and every f step is the library's
// check node, in SC's operation order; no subtree is skipped.  What the kernel keeps is not a decision but two counters per
// leaf: how often the leaf LLR was negative (the genie-aided decision would have been wrong) and how often it was zero.
//
//   LLR levels 0..4: registers, the unrolled 32-leaf block; levels 5..n-1: the wavefront's slice of global scratch at
//     (2^t + e)*64 + lane; channel rows read in place -- all as in sc_lanes.h.
//   No partial sums at all (no LDS words, no select in g), no frozen-pattern tests: the block body is straight-line.
//   At a leaf: two wave ballots (lambda < 0, lambda == 0; lanes of the ragged last batch masked out), their popcounts are
//     uniform values; lane k of the wavefront keeps leaf k's pair, and lanes 0..31 add them to the workgroup's uint32
//     counters in LDS once per 32-leaf block.  LDS goes to the caller's uint64 counters once, at the end of the kernel.
//
// k_genie_rows: the design rows of rule 3 (all-zero codeword through BPSK + AWGN, as LLRs).
#pragma once
#include "polar_math.h"
#include "polar_lut.h"
#include "scl_generic.h"
#include "gen_common.h"

namespace polar {

struct GenieParams {
    const void *in;               // [B][N] double or float: LLRs, or y when sigma > 0
    double sigma;
    unsigned long long *counts;   // [2][N]: err row, tie row; the launch ADDS to them
    int N, n, B;
    void *scratch;                // per-wave slices, GenieCfg::scratch_bytes each
    unsigned *queue;              // job counter (polar_host.h work_queue()); null = jobs by a fixed stride
};

struct GenieRowsParams {
    void *out;                    // [B][N] double or float
    uint64_t seed, first_frame;
    double sigma;
    int N, B;
};

template <typename R>
struct GenieCfg {
    static constexpr int WAVES = 4;
    static constexpr int MIN_WAVES_PER_SIMD = 2;
    static constexpr size_t cnt_bytes(int N) { return sizeof(uint32_t) * 2 * (size_t)N; }   // err[N], tie[N]
    static constexpr size_t lds_bytes(int N) { return cnt_bytes(N) + Lut<R>::bytes; }
    static constexpr size_t scratch_bytes(int N) { return sizeof(R) * (size_t)N * 64; }   // levels 5 .. n-1: element indices < N
};

template <typename R>
struct GenieLanes {
    const Lut<R> &lut;
    bool have;       // this lane holds a frame (false only in the ragged last batch)
    int lane;
    uint32_t cnt;    // lane k: popcount of (lambda_k < 0) | popcount of (lambda_k == 0) << 16, k = leaf within the block

    // node of 2^T leaves starting at leaf K0 of the block, LLRs a[0..2^T)
    template <int T, int K0>
    __device__ __forceinline__ void rec(const R *a)
    {
        if constexpr (T == 0) {
            const uint32_t pe = (uint32_t)__popcll(__ballot(have && a[0] < R(0)));    // a NaN counts as neither
            const uint32_t pt = (uint32_t)__popcll(__ballot(have && a[0] == R(0)));   // -0.0 is a tie
            cnt = (lane == K0) ? (pe | (pt << 16)) : cnt;   // uniform value -> lane K0
        } else {
            constexpr int h = 1 << (T - 1);
            {
                R l[h];
#pragma unroll
                for (int e = 0; e < h; ++e) l[e] = chk_lut<R>(a[e], a[e + h], lut);
                rec<T - 1, K0>(l);
            }
            {
                R r[h];
#pragma unroll
                for (int e = 0; e < h; ++e) r[e] = a[e + h] + a[e];   // gfun with partner bit 0: cL + cU
                rec<T - 1, K0 + h>(r);
            }
        }
    }
};

template <typename R, typename IN>
__global__ __launch_bounds__(256, (GenieCfg<R>::MIN_WAVES_PER_SIMD)) void k_genie_lanes(GenieParams P)
{
    using Cfg = GenieCfg<R>;
    const int N = P.N, n = P.n, NW = N >> 5;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *cerr = reinterpret_cast<uint32_t *>(smem);   // [N] workgroup counters: lambda < 0
    uint32_t *ctie = cerr + N;                             // [N] lambda == 0
    unsigned char *lut_mem = smem + Cfg::cnt_bytes(N);
    for (int i = threadIdx.x; i < 2 * N; i += blockDim.x) cerr[i] = 0u;
    Lut<R>::build(lut_mem, threadIdx.x, blockDim.x);
    Lut<R> lut;
    lut.bind(lut_mem);
    __syncthreads();

    const int slot = blockIdx.x * Cfg::WAVES + wave, nslots = gridDim.x * Cfg::WAVES;
    R *lev = reinterpret_cast<R *>(reinterpret_cast<unsigned char *>(P.scratch) + (size_t)slot * Cfg::scratch_bytes(N)) + lane;
    // levb is lev, laundered once per 32-leaf block, so that the statically indexed row addresses are not hoisted out of the
    // batch loop and spilled (sc_lanes.h)
    R *levb = lev;
    auto at = [&](int idx) -> R * { return levb + (size_t)idx * 64; };
    auto sync = [] { __asm__ volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); };
    const int nbatch = (P.B + 63) >> 6;

    for (int batch = slot; batch < nbatch; batch = next_job_wave(P.queue, batch, nslots, nbatch)) {
        const int frame0 = batch << 6;
        const bool have = frame0 + lane < P.B;   // the ragged last batch: idle lanes compute on zeros and count nothing
        const IN *row = reinterpret_cast<const IN *>(P.in) + (size_t)(have ? frame0 + lane : 0) * N;
        const bool al16 = ((reinterpret_cast<uintptr_t>(P.in) | ((size_t)N * sizeof(IN))) & 15u) == 0;   // uniform
        auto chan16 = [&](int e0, R *dst) {   // elements e0 .. e0+15 of the lane's row (e0 a multiple of 16)
            IN raw[16];
            if (al16) {
                const IN *r = reinterpret_cast<const IN *>(__builtin_assume_aligned(row + e0, 16));
#pragma unroll
                for (int u = 0; u < 16; ++u) raw[u] = r[u];
            } else {
#pragma unroll
                for (int u = 0; u < 16; ++u) raw[u] = row[e0 + u];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                dst[u] = (R)channel_llr(have ? (double)raw[u] : 0.0, P.sigma);
            }
        };
        sync();
        for (int b = 0; b < NW; ++b) {
            levb = lev;
            __asm__ volatile("" : "+v"(levb));
            // ---- levels n-1 .. 5 above this block: g at the level where the path turns right, f below it ----
            // One pass computes level t (g or f of level t+1, or of the channel rows at t = n-1) and, when fuse, level
            // t-1 = f(level t) as well, so that level t is written once and not read back by the f step that follows.
            auto step = [&](int t, bool gstep, bool fuse) {
                const int h = 1 << t, hh = h >> 1;
                if (t == n - 1) {
                    for (int e0 = 0; e0 < (fuse ? hh : h); e0 += 16) {
                        R v[2][16];
#pragma unroll
                        for (int half = 0; half < 2; ++half) {
                            if (half == 1 && !fuse) break;
                            const int e = e0 + half * hh;
                            R a[16], c[16];
                            chan16(e, a);
                            chan16(e + h, c);
#pragma unroll
                            for (int u = 0; u < 16; ++u) {
                                v[half][u] = gstep ? c[u] + a[u] : chk_lut<R>(a[u], c[u], lut);
                                *at(h + e + u) = v[half][u];
                            }
                        }
                        if (fuse) {
#pragma unroll
                            for (int u = 0; u < 16; ++u) *at(hh + e0 + u) = chk_lut<R>(v[0][u], v[1][u], lut);
                        }
                    }
                } else {
                    for (int e0 = 0; e0 < (fuse ? hh : h); e0 += 8) {
                        R v[2][8];
#pragma unroll
                        for (int half = 0; half < 2; ++half) {
                            if (half == 1 && !fuse) break;
                            const int e = e0 + half * hh;
                            R a[8], c[8];
#pragma unroll
                            for (int u = 0; u < 8; ++u) {
                                a[u] = ld_bypass(at(2 * h + e + u));
                                c[u] = ld_bypass(at(2 * h + e + u + h));
                            }
#pragma unroll
                            for (int u = 0; u < 8; ++u) {
                                v[half][u] = gstep ? c[u] + a[u] : chk_lut<R>(a[u], c[u], lut);
                                *at(h + e + u) = v[half][u];
                            }
                        }
                        if (fuse) {
#pragma unroll
                            for (int u = 0; u < 8; ++u) *at(hh + e0 + u) = chk_lut<R>(v[0][u], v[1][u], lut);
                        }
                    }
                }
                sync();
            };
            int td = n - 1;
            bool gstep = false;
            if (b > 0) {
                td = __builtin_ctz((unsigned)b) + 5;
                gstep = true;
            }
            // Long codes (n > 7): the steps that produce level 5 run after this loop and leave it in registers
            while (td >= 5) {
                if (n > 7 && td <= 6) break;
                const bool fuse = td >= 6;
                step(td, gstep, fuse);
                td -= fuse ? 2 : 1;
                gstep = false;
            }
            R x5[32];   // level 5 of this block: read by the two halves of the block and by nobody else, so never stored
            if (n > 7 && td == 6) {   // level 6 from level 7 (stored: a later g step reads it), level 5 = f(level 6)
#pragma unroll
                for (int e0 = 0; e0 < 32; e0 += 8) {
                    R v[2][8];
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        const int e = e0 + half * 32;
                        R a[8], c[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            a[u] = ld_bypass(at(128 + e + u));
                            c[u] = ld_bypass(at(192 + e + u));
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            v[half][u] = gstep ? c[u] + a[u] : chk_lut<R>(a[u], c[u], lut);
                            *at(64 + e + u) = v[half][u];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) x5[e0 + u] = chk_lut<R>(v[0][u], v[1][u], lut);
                }
                sync();
            } else if (n > 7) {   // td == 5: level 5 from level 6
#pragma unroll
                for (int e0 = 0; e0 < 32; e0 += 8) {
                    R a[8], c[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        a[u] = ld_bypass(at(64 + e0 + u));
                        c[u] = ld_bypass(at(96 + e0 + u));
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) x5[e0 + u] = gstep ? c[u] + a[u] : chk_lut<R>(a[u], c[u], lut);
                }
            } else if (n == 5) {   // N = 32: level 5 IS the channel level, read in place
                chan16(0, x5);
                chan16(16, x5 + 16);
            } else {               // N = 64, 128: the generic steps above left level 5 in the scratch
#pragma unroll
                for (int u = 0; u < 32; ++u) x5[u] = ld_bypass(at(32 + u));
            }
            // ---- the 32-leaf block: level 5 in x5, levels 4..0 in registers, straight-line ----
            // the lane number is laundered like levb: the 32 (lane == k) masks are otherwise kept in SGPR pairs over the whole
            // batch loop and spilled
            int lb = lane;
            __asm__ volatile("" : "+v"(lb));
            GenieLanes<R> S{lut, have, lb, 0u};
            S.template rec<5, 0>(x5);
            if (lane < 32) {   // once per block and wave: 32 leaves' popcounts into the workgroup's counters
                const uint32_t pe = S.cnt & 0xFFFFu, pt = S.cnt >> 16;
                if (pe) atomicAdd(&cerr[b * 32 + lane], pe);
                if (pt) atomicAdd(&ctie[b * 32 + lane], pt);
            }
        }
    }
    // ---- workgroup counters -> the caller's uint64 counters, zeros skipped ----
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * N; i += blockDim.x) {
        const uint32_t v = cerr[i];
        if (v) atomicAdd(&P.counts[i], (unsigned long long)v);
    }
}

// Rule 3: element e of frame f is 2*y/sigma/sigma, y = 1 + sigma * z, z = normal (e & 1) of Philox(seed, first_frame + f,
// e >> 1, stream 2) by k_generate's Box-Muller.  One thread per pair of elements, one 8- or 16-byte store each.
template <typename OUT>
__global__ __launch_bounds__(256) void k_genie_rows(GenieRowsParams P)
{
    const int hN = P.N >> 1;
    const size_t total = (size_t)P.B * hN;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / hN;
        const uint32_t q = (uint32_t)(i - f * hN);
        const Philox g(P.seed, P.first_frame + (uint64_t)f, q, 2u);
        const double r = sqrt(-2.0 * log(g.u0()));
        double sn, cs;
        sincospi(2.0 * g.u1(), &sn, &cs);
        const double nz[2] = {r * cs, r * sn};
        OUT v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double y = 1.0 + P.sigma * nz[h];
            v[h] = (OUT)(2 * y / P.sigma / P.sigma);
        }
        OUT *dst = reinterpret_cast<OUT *>(P.out) + 2 * i;
        dst[0] = v[0];
        dst[1] = v[1];
    }
}

}  // namespace polar
