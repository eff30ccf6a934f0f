// scf_lanes.h -- CRC-aided SC-Flip (POLAR_ALGO_SCF, include/polar_hip.h; Afisiadis, Balatsoukas-Stimming and Burg, 2014).
//
// The decoder is k_sc_lanes (sc_lanes.h): one codeword per lane, the frozen schedule common to the wavefront, the same
// recursion, check node and input reads, so every decision and every leaf LLR is k_sc_lanes's, operation for operation.
// What differs is the leaf: k_scf_lanes<R, IN, MODE> takes a leaf policy.
//   SCF_CHECK   (pass A, every frame)  the SC decision, and the CRC syndrome accumulated as the bits are decided: the leaf
//               index j is wave-uniform, so crc_tab[j] is a scalar load and each lane adds it with one select.  Writes the
//               decisions, the flags word (POLAR_FLAG_CRC_PASS on a pass) and attempts = 0 / T.
//   SCF_RECORD  (the failing frames, one lane each) the same decisions again, keeping the lane's T smallest (|lambda_j|, j)
//               in a sorted list in LDS ([T][64] per wavefront, the current T-th key in a VGPR for early rejection).
//               Writes the T flip positions, ascending |lambda|, ties to the smaller j.
//   SCF_FLIP    (pass B, one lane per (failing frame, attempt t)) SC with the decision at leaf p_t inverted; the inverted bit
//               enters the partial sums of every later leaf.  Writes the decisions and the CRC pass bit of the pair.
// The dynamic rule (polar_scf_set_dynamic, include/polar_hip.h) adds three policies; a static context launches none of them:
//   SCF_RECORD_M  SCF_RECORD on the key M(0, j) = |lambda_j| + c * cnt_j, cnt_j the running count of information leaves with
//               |lambda| <= tau.  Writes the list itself (keys, leaves, length) for k_scf_merge.
//   SCF_FLIPSET (one lane per (failing frame, flip set E)) run(E): up to three ascending flip leaves per lane.  The next one
//               sits in a cursor that advances at each hit, so a leaf costs one compare.  Writes what SCF_FLIP writes.
//   SCF_FLIPREC run(E) as SCF_FLIPSET, and in the same run the lane's Tn smallest (M(E, j), j) over j > max(E): F_E
//               accumulates as the flipped leaves are reached, cnt counts from leaf 0.  Writes decisions, pass bit and list.
// Why the list is not kept in pass A: T = 32 at N = 2048 in f64 needs 24 KiB of LDS per wavefront on top of k_sc_lanes's
// 24 KiB, which halves the resident wavefronts of a pass that runs on every frame; re-decoding only the failing frames costs
// 1/T of pass B instead.
// No cross-lane operation runs under a divergent EXEC: the readlanes of the frozen schedule sit where k_sc_lanes has them,
// in wave-uniform control flow; the list insertion (divergent) touches only the lane's own LDS column.
#pragma once
#include "sc_lanes.h"
#include "scf_params.h"

namespace polar {

template <typename R>
struct ScfCfg {
    static constexpr int WAVES = 4;   // at most; fewer when the list of a recording policy does not fit 160 KiB (N = 2048, f64, T > 16)
    static constexpr bool keeps_list(int mode) { return mode == SCF_RECORD || mode == SCF_RECORD_M || mode == SCF_FLIPREC; }
    static constexpr size_t list_bytes(int T) { return (size_t)T * 64 * (sizeof(R) + sizeof(uint32_t)); }
    static constexpr size_t wave_bytes(int N, int T, int mode)
    {
        return ScLanesCfg<R>::wave_bytes(N) + (keeps_list(mode) ? list_bytes(T) : 0);
    }
    static constexpr size_t lds_bytes(int N, int T, int mode, int waves) { return wave_bytes(N, T, mode) * waves + Lut<R>::bytes; }
};

constexpr int SCF_NO_LEAF = 0x7fffffff;   // above every leaf index

template <typename R, int MODE>
struct ScfLanes {
    const Lut<R> &lut;
    uint32_t fz;              // frozen mask of the current 32-leaf block (uniform)
    uint32_t dec;             // decisions of the block, bit k = leaf k
    int j0;                   // first leaf of the block (uniform)
    const uint32_t *ctab;     // crc_tab + j0 (uniform)
    uint32_t crc;             // syndrome of the decisions so far
    int flip;                 // SCF_FLIP: the leaf whose decision is inverted (-1: none)
    R *key;                   // SCF_RECORD: key[i * 64] = i-th smallest |lambda| so far (this lane's column)
    uint32_t *pos;            // SCF_RECORD: its leaf
    int nT, cnt;              // SCF_RECORD: list length, entries filled
    R thr;                    // SCF_RECORD: key[(nT - 1) * 64] once the list is full
    int nf, f1, f2;           // SCF_FLIPSET, SCF_FLIPREC: the next leaf to invert and the two after it (SCF_NO_LEAF: none)
    int maxE;                 // SCF_RECORD_M, SCF_FLIPREC: leaves above it are recorded (-1: all; SCF_NO_LEAF: none)
    int tcnt;                 // SCF_RECORD_M, SCF_FLIPREC: information leaves so far with |lambda| <= tau
    R F, mc, tau;             // SCF_FLIPREC: sum of |lambda| over the flipped leaves so far; the rule's c and tau in R

    __device__ __forceinline__ void record(R v, int j)
    {
        if (cnt < nT || v < thr) {   // a later leaf with an equal key never goes before an earlier one
            int i = cnt < nT ? cnt : nT - 1;
            while (i > 0) {
                const R k = key[(i - 1) * 64];
                if (!(v < k)) break;
                key[i * 64] = k;
                pos[i * 64] = pos[(i - 1) * 64];
                --i;
            }
            key[i * 64] = v;
            pos[i * 64] = (uint32_t)j;
            if (cnt < nT) ++cnt;
            if (cnt == nT) thr = key[(nT - 1) * 64];
        }
    }

    // node of 2^T leaves starting at leaf K0 of the block, LLRs a[0..2^T); returns its partial sums (ScLanes::rec)
    template <int T, int K0>
    __device__ __forceinline__ uint32_t rec(const R *a)
    {
        constexpr uint32_t span = (T == 5) ? 0xFFFFFFFFu : ((1u << (1 << T)) - 1u);
        if (((fz >> K0) & span) == span) return 0u;
        if constexpr (T == 0) {
            uint32_t bit = (a[0] < R(0)) ? 1u : 0u;
            if constexpr (MODE == SCF_FLIP) bit ^= (j0 + K0 == flip) ? 1u : 0u;
            if constexpr (MODE >= SCF_RECORD_M) {
                const int j = j0 + K0;
                const R v = absr(a[0]);
                if constexpr (MODE != SCF_FLIPSET) tcnt += (v <= tau) ? 1 : 0;
                if constexpr (MODE != SCF_RECORD_M) {
                    if (j == nf) {
                        bit ^= 1u;
                        if constexpr (MODE == SCF_FLIPREC) F = F + v;
                        nf = f1;
                        f1 = f2;
                        f2 = SCF_NO_LEAF;
                    }
                }
                if constexpr (MODE != SCF_FLIPSET) {
                    if (j > maxE) record((F + v) + mc * (R)tcnt, j);   // rule 3: each operation rounded once (-ffp-contract=off)
                }
            }
            if constexpr (MODE == SCF_RECORD) {
                record(absr(a[0]), j0 + K0);
            } else if constexpr (MODE != SCF_RECORD_M) {
                const uint32_t t = ctab[K0];
                crc ^= bit ? t : 0u;
            }
            dec |= bit << K0;
            return bit;
        } else {
            constexpr int h = 1 << (T - 1);
            constexpr uint32_t half = (1u << h) - 1u;
            uint32_t bl = 0, br = 0;
            if (((fz >> K0) & half) != half) {
                R l[h];
#pragma unroll
                for (int e = 0; e < h; ++e) l[e] = chk_lut<R>(a[e], a[e + h], lut);
                bl = rec<T - 1, K0>(l);
            }
            if (((fz >> (K0 + h)) & half) != half) {
                R r[h];
#pragma unroll
                for (int e = 0; e < h; ++e) r[e] = gfun<R>(a[e], a[e + h], (bl >> e) & 1u);
                br = rec<T - 1, K0 + h>(r);
            }
            return (bl ^ br) | (br << h);
        }
    }
};

// k_sc_lanes with the leaf policy MODE (above).  The waves of a workgroup: blockDim.x / 64 (the host picks it).
template <typename R, typename IN, int MODE>
__global__ __launch_bounds__(256, (ScLanesCfg<R>::MIN_WAVES_PER_SIMD)) void k_scf_lanes(ScfParams P)
{
    using Cfg = ScfCfg<R>;
    const int N = P.N, n = P.n, NW = N >> 5;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = (int)(blockDim.x >> 6);
    const int nT = P.T;
    const int nL = (MODE >= SCF_RECORD_M) ? P.Tn : nT;   // length of the list in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *mine = smem + (size_t)wave * Cfg::wave_bytes(N, nL, MODE);
    uint32_t *blw = reinterpret_cast<uint32_t *>(mine);          // [NW][64]: saved left partial sums
    uint32_t *curw = blw + (size_t)NW * 64;                      // [NW/2][64] working partial sums
    R *lkey = reinterpret_cast<R *>(mine + ScLanesCfg<R>::wave_bytes(N)) + lane;    // SCF_RECORD: [T][64]
    uint32_t *lpos = reinterpret_cast<uint32_t *>(lkey - lane + (size_t)nL * 64) + lane;
    unsigned char *lut_mem = smem + (size_t)waves * Cfg::wave_bytes(N, nL, MODE);
    Lut<R>::build(lut_mem, threadIdx.x, blockDim.x);
    Lut<R> lut;
    lut.bind(lut_mem);
    __syncthreads();

    const int slot = blockIdx.x * waves + wave, nslots = gridDim.x * waves;
    R *lev = reinterpret_cast<R *>(reinterpret_cast<unsigned char *>(P.scratch) + (size_t)slot * ScLanesCfg<R>::scratch_bytes(N)) + lane;
    R *levb = lev;   // laundered once per 32-leaf block, as in k_sc_lanes
    auto at = [&](int idx) -> R * { return levb + (size_t)idx * 64; };
    auto sync = [] { __asm__ volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); };
    const int nbatch = (P.B + 63) >> 6;

    for (int batch = slot; batch < nbatch; batch = next_job_wave(P.queue, batch, nslots, nbatch)) {
        const int item = (batch << 6) + lane;
        const bool have = item < P.B;   // the ragged last batch: idle lanes compute on frame 0's row and store nothing
        size_t frame = 0;
        int flip = -1;
        if (have) {
            if constexpr (MODE == SCF_CHECK) frame = (size_t)item;
            else if constexpr (MODE == SCF_RECORD || MODE == SCF_RECORD_M) frame = P.idx[item];
            else {
                frame = P.idx[item / nT];
                if constexpr (MODE == SCF_FLIP) flip = (int)P.flips[item];
            }
        }
        int nf = SCF_NO_LEAF, f1 = SCF_NO_LEAF, f2 = SCF_NO_LEAF, maxE = SCF_NO_LEAF;
        if constexpr (MODE == SCF_RECORD_M) maxE = -1;
        if constexpr (MODE == SCF_FLIPSET || MODE == SCF_FLIPREC) {
            if (have) {   // an absent set (a level's list was shorter than its budget) inverts nothing and never passes
                const uint16_t *e = P.flips + (size_t)item * SCF_MAX_ORDER;
                if (e[0] != SCF_NO_POS) nf = maxE = (int)e[0];
                if (e[1] != SCF_NO_POS) f1 = maxE = (int)e[1];
                if (e[2] != SCF_NO_POS) f2 = maxE = (int)e[2];
            }
        }
        const bool valid = nf != SCF_NO_LEAF;
        int tcnt = 0;
        R F = R(0);
        const R mc = (R)P.mc, tau = (R)P.tau;
        const IN *row = reinterpret_cast<const IN *>(P.in) + frame * N;
        const bool al16 = ((reinterpret_cast<uintptr_t>(P.in) | ((size_t)N * sizeof(IN))) & 15u) == 0;   // uniform
        auto chan16 = [&](int e0, R *dst) {
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
        uint32_t crc = 0;
        int cnt = 0;
        R thr = R(0);
        uint32_t fwv = 0;
        for (int b = 0; b < NW; ++b) {
            levb = lev;
            __asm__ volatile("" : "+v"(levb));
            if ((b & 63) == 0) fwv = (b + lane < NW) ? P.frozen[b + lane] : 0xFFFFFFFFu;
            auto frozen_span = [&](int b0, int nwords) -> bool {
                uint32_t all = 0xFFFFFFFFu;
                for (int w = 0; w < nwords; ++w) all &= (uint32_t)__builtin_amdgcn_readlane((int)fwv, (b0 + w) & 63);
                return all == 0xFFFFFFFFu;
            };
            // ---- levels n-1 .. 5 above this block (k_sc_lanes) ----
            auto step = [&](int t, bool gstep, bool fuse) {
                const int h = 1 << t, hh = h >> 1;
                const uint32_t *bw = blw + (size_t)(h >> 5) * 64 + lane;
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
                            const uint32_t wv = gstep ? bw[(size_t)(e >> 5) * 64] : 0u;
#pragma unroll
                            for (int u = 0; u < 16; ++u) {
                                v[half][u] = gstep ? gfun<R>(a[u], c[u], (wv >> ((e + u) & 31)) & 1u) : chk_lut<R>(a[u], c[u], lut);
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
                            const uint32_t wv = gstep ? bw[(size_t)(e >> 5) * 64] : 0u;
#pragma unroll
                            for (int u = 0; u < 8; ++u) {
                                v[half][u] = gstep ? gfun<R>(a[u], c[u], (wv >> ((e + u) & 31)) & 1u) : chk_lut<R>(a[u], c[u], lut);
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
            bool live = true;
            int td = n - 1;
            bool gstep = false;
            if (b > 0) {
                td = __builtin_ctz((unsigned)b) + 5;
                gstep = true;
            }
            while (td >= 5) {
                live = !frozen_span(b, 1 << (td - 5));
                if (!live) break;
                if (n > 7 && td <= 6) break;
                const bool fuse = (td >= 6) && !frozen_span(b, 1 << (td - 6));
                step(td, gstep, fuse);
                td -= fuse ? 2 : 1;
                gstep = false;
            }
            R x5[32];
            if (live && n > 7 && td == 6) {
                const bool below = !frozen_span(b, 1);
                const uint32_t *bw = blw + (size_t)2 * 64 + lane;
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
                        const uint32_t wv = gstep ? bw[(size_t)half * 64] : 0u;
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            v[half][u] = gstep ? gfun<R>(a[u], c[u], (wv >> (e0 + u)) & 1u) : chk_lut<R>(a[u], c[u], lut);
                            *at(64 + e + u) = v[half][u];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) x5[e0 + u] = chk_lut<R>(v[0][u], v[1][u], lut);
                }
                sync();
                live = below;
            } else if (live && n > 7 && td == 5) {
                const uint32_t wv = gstep ? blw[(size_t)1 * 64 + lane] : 0u;
#pragma unroll
                for (int e0 = 0; e0 < 32; e0 += 8) {
                    R a[8], c[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        a[u] = ld_bypass(at(64 + e0 + u));
                        c[u] = ld_bypass(at(96 + e0 + u));
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        x5[e0 + u] = gstep ? gfun<R>(a[u], c[u], (wv >> (e0 + u)) & 1u) : chk_lut<R>(a[u], c[u], lut);
                }
            }
            // ---- the 32-leaf block: level 5 in x5, levels 4..0 in registers, the leaf policy at every information leaf ----
            uint32_t beta = 0, dec = 0;
            const uint32_t fz = (uint32_t)__builtin_amdgcn_readlane((int)fwv, b & 63);
            if (live && fz != 0xFFFFFFFFu) {
                ScfLanes<R, MODE> S{lut, fz, 0u, b << 5, P.crc_tab + (b << 5), crc, flip, lkey, lpos, nL, cnt, thr,
                                    nf, f1, f2, maxE, tcnt, F, mc, tau};
                uint32_t bl = 0, br = 0;
                if (n == 5) {
                    chan16(0, x5);
                    chan16(16, x5 + 16);
                } else if (n <= 7) {
#pragma unroll
                    for (int u = 0; u < 32; ++u) x5[u] = ld_bypass(at(32 + u));
                }
                if ((fz & 0xFFFFu) != 0xFFFFu) {
                    R l[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) l[e] = chk_lut<R>(x5[e], x5[16 + e], lut);
                    bl = S.template rec<4, 0>(l);
                }
                if ((fz >> 16) != 0xFFFFu) {
                    R r[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) r[e] = gfun<R>(x5[e], x5[16 + e], (bl >> e) & 1u);
                    br = S.template rec<4, 16>(r);
                }
                beta = (bl ^ br) | (br << 16);
                dec = S.dec;
                crc = S.crc;
                cnt = S.cnt;
                thr = S.thr;
                if constexpr (MODE >= SCF_RECORD_M) {
                    nf = S.nf;
                    f1 = S.f1;
                    f2 = S.f2;
                    tcnt = S.tcnt;
                    F = S.F;
                }
            }
            if constexpr (MODE != SCF_RECORD && MODE != SCF_RECORD_M) {
                if (have) P.out_bits[(size_t)item * NW + b] = dec;
            }
            // ---- partial sums upwards (k_sc_lanes) ----
            int t = 5;
            if constexpr (MODE >= SCF_RECORD_M) {
                if (n > 5) curw[lane] = beta;   // N = 32 has no curw ([NW/2][64]): the word after blw is the list's first key
            } else {
                curw[lane] = beta;
            }
            while (t < n - 1 && ((b >> (t - 5)) & 1)) {
                const int nw = 1 << (t - 5);
                for (int w = 0; w < nw; ++w) {
                    const uint32_t c = curw[w * 64 + lane];
                    const uint32_t l = blw[(nw + w) * 64 + lane];
                    curw[w * 64 + lane] = l ^ c;
                    curw[(w + nw) * 64 + lane] = c;
                }
                ++t;
            }
            if (t < n && !((b >> (t - 5)) & 1)) {
                const int nw = 1 << (t - 5);
                for (int w = 0; w < nw; ++w) blw[(nw + w) * 64 + lane] = curw[w * 64 + lane];
            }
        }
        if (have) {
            const bool pass = crc == 0u;
            if constexpr (MODE == SCF_CHECK) {
                if (P.pm) P.pm[item] = 0.0;
                if (P.flags) P.flags[item] = pass ? SCF_CRC_PASS : 0u;
                if (P.attempts) P.attempts[item] = pass ? 0u : (uint32_t)nT;
            } else if constexpr (MODE == SCF_FLIP) {
                P.flags[item] = pass ? 1u : 0u;
            } else if constexpr (MODE == SCF_RECORD) {
                for (int i = 0; i < nT; ++i) P.flips[(size_t)item * nT + i] = (uint16_t)lpos[i * 64];
            } else {
                if constexpr (MODE != SCF_RECORD_M) P.flags[item] = (pass && valid) ? 1u : 0u;
                if constexpr (MODE != SCF_FLIPSET) {
                    R *ok = reinterpret_cast<R *>(P.lkey) + (size_t)item * nL;
                    uint16_t *op = P.lpos + (size_t)item * nL;
                    for (int i = 0; i < cnt; ++i) {
                        ok[i] = lkey[i * 64];
                        op[i] = (uint16_t)lpos[i * 64];
                    }
                    P.lcnt[item] = (uint32_t)cnt;
                }
            }
        }
    }
}

// For each failing frame k of a chunk (frame idx[k]): the smallest t whose pair k * T + t - 1 passed.  Its decisions replace
// the frame's, POLAR_FLAG_CRC_PASS joins its flags and attempts = t.  Without a passing t nothing changes (pass A wrote
// the decisions of attempt 0, flags without the pass bit and attempts = T).  One thread per (frame, decision word).
__global__ __launch_bounds__(256) void k_scf_resolve(const uint32_t *__restrict__ pass, const uint32_t *__restrict__ pbits,
                                                     const uint32_t *__restrict__ idx, long long n, int T, int logNW,
                                                     uint32_t *__restrict__ bits, uint32_t *__restrict__ flags,
                                                     uint32_t *__restrict__ attempts)
{
    const long long total = n << logNW;
    const long long wmask = (1ll << logNW) - 1;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
        const long long k = q >> logNW, w = q & wmask;
        int t = 0;
        while (t < T && !pass[k * T + t]) ++t;
        if (t == T) continue;
        const long long f = idx[k];
        bits[(f << logNW) + w] = pbits[((k * T + t) << logNW) + w];
        if (w == 0) {
            if (flags) flags[f] |= SCF_CRC_PASS;
            if (attempts) attempts[f] = (uint32_t)(t + 1);
        }
    }
}

// k_scf_resolve for flip sets.  Pair k * T + t - 1 of failing frame k ran the set sets[(k * T + t - 1) * stride ..+ width)
// (a static context's flip list: stride = width = 1).  The smallest passing t is global attempt base + t; d_sets
// (nullable, [frames][3]) gets its set, -1 padded.  slot_pass (nullable, [n]) gets 1 where a pair of the frame passed and
// 0 elsewhere: the flags the next level's compaction reads.
__global__ __launch_bounds__(256) void k_scf_resolve_sets(const uint32_t *__restrict__ pass, const uint32_t *__restrict__ pbits,
                                                          const uint32_t *__restrict__ idx, long long n, int T, int logNW,
                                                          const uint16_t *__restrict__ sets, int stride, int width, int base,
                                                          uint32_t *__restrict__ bits, uint32_t *__restrict__ flags,
                                                          uint32_t *__restrict__ attempts, int32_t *__restrict__ d_sets,
                                                          uint32_t *__restrict__ slot_pass)
{
    const long long total = n << logNW;
    const long long wmask = (1ll << logNW) - 1;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
        const long long k = q >> logNW, w = q & wmask;
        int t = 0;
        while (t < T && !pass[k * T + t]) ++t;
        if (w == 0 && slot_pass) slot_pass[k] = t < T ? 1u : 0u;
        if (t == T) continue;
        const long long f = idx[k];
        bits[(f << logNW) + w] = pbits[((k * T + t) << logNW) + w];
        if (w == 0) {
            if (flags) flags[f] |= SCF_CRC_PASS;
            if (attempts) attempts[f] = (uint32_t)(base + t + 1);
            if (d_sets) {
                for (int e = 0; e < SCF_MAX_ORDER; ++e) {
                    const uint16_t p = e < width ? sets[(k * T + t) * stride + e] : SCF_NO_POS;
                    d_sets[f * SCF_MAX_ORDER + e] = p == SCF_NO_POS ? -1 : (int32_t)p;
                }
            }
        }
    }
}

// Rule 5 of the dynamic rule: the sets of the next level.  One thread per still-failing frame s, which sat in slot
// o = surv[s] of the level that just ran (surv null: o = s, nothing was compacted).  Its Tk pairs o * Tk + q kept sorted
// lists (lkey, lpos, lcnt: Tn entries at most, SCF_RECORD_M / SCF_FLIPREC); a Tk-way merge emits the Tn smallest
// (M, q, i): the heads are scanned in ascending q with a strict compare, so equal M goes to the smaller q, and a list is
// in (M, i) order already.  Comparisons only.  out_sets[(s * Tn + r) * 3 ..] = E_q with i appended (psets null: E_q is
// empty), absent sets where the candidates run out; idx_out[s] = idx_in[o] when the frames were compacted.
template <typename R>
__global__ __launch_bounds__(256) void k_scf_merge(const R *__restrict__ lkey, const uint16_t *__restrict__ lpos,
                                                   const uint32_t *__restrict__ lcnt, const uint16_t *__restrict__ psets,
                                                   const uint32_t *__restrict__ surv, const uint32_t *__restrict__ idx_in,
                                                   long long n, int Tk, int Tn, uint16_t *__restrict__ out_sets,
                                                   uint32_t *__restrict__ idx_out)
{
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < n; s += (long long)gridDim.x * 256) {
        const long long o = surv ? (long long)surv[s] : s;
        if (surv) idx_out[s] = idx_in[o];
        unsigned char head[SCF_MAX_T];
        for (int q = 0; q < Tk; ++q) head[q] = 0;
        for (int r = 0; r < Tn; ++r) {
            int best = -1;
            R bk = R(0);
            for (int q = 0; q < Tk; ++q) {
                const long long it = o * Tk + q;
                if (head[q] >= lcnt[it]) continue;
                const R k = lkey[it * Tn + head[q]];
                if (best < 0 || k < bk) {
                    best = q;
                    bk = k;
                }
            }
            uint16_t *e = out_sets + (s * Tn + r) * SCF_MAX_ORDER;
            if (best < 0) {
                e[0] = e[1] = e[2] = SCF_NO_POS;
                continue;
            }
            const long long it = o * Tk + best;
            int m = 0;
            if (psets)
                for (; m < SCF_MAX_ORDER - 1 && psets[it * SCF_MAX_ORDER + m] != SCF_NO_POS; ++m) e[m] = psets[it * SCF_MAX_ORDER + m];
            e[m++] = lpos[it * Tn + head[best]];
            for (; m < SCF_MAX_ORDER; ++m) e[m] = SCF_NO_POS;
            ++head[best];
        }
    }
}

}  // namespace polar
