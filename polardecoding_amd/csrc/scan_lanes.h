// scan_lanes.h -- soft-output SCAN decoder (POLAR_ALGO_SCAN, include/polar_hip.h), ONE CODEWORD PER LANE.
//
// SCAN is BP's message arithmetic on SC's schedule, so the kernel has k_sc_lanes' shape: a wavefront decodes 64 codewords
// in lock step, lane l working on frame 64*batch + l, and the schedule -- which subtrees are entered, and where a beta is
// +inf -- depends on the frozen mask only and is uniform.  No cross-lane instruction beyond one ballot at the top.
//
//   Levels 0..4 (a 32-leaf block): registers, template recursion (ScanBlock::rec), alphas down and betas up.
//   Levels 5..n: the wavefront's slice of a global scratch buffer, rows [element][lane] (every access one coalesced row):
//     A   alpha of the current path, level t at 2^t + e (the channel level n at N + e)               [0, 2N)
//     BL  beta of the node of the current path at level t, kept for its right sibling and its parent  [2N, 4N)
//     BR  the stored right-child betas, level t (1..n-1) at 4N + (t-1)*N/2 + (s - 2^t)/2 + e, s = the child's first leaf
//     Elements 0..31 of A (below level 5, never used as alphas) hold the block's lambdas on their way to llr_u.
//   The rows a lane reads are the rows the same lane wrote: plain loads and stores, program order.
//
// Skipping (consequences of rules 1-5, include/polar_hip.h): an all-frozen subtree is never entered and its beta is the
// constant +inf; an all-information subtree is entered in the last iteration only, downwards only, and its beta is the
// constant 0.  Neither constant is ever stored.  A parent with such a child uses the reduced forms
//   CHK(a, +inf) = a,  x + inf = inf,  CHK(a, b + 0) = chk(a, b),  b + CHK(a, 0) = b
// which have the values of the full rules; everything else goes through chk_inf, a select around chk_lut.
#pragma once
#include "polar_math.h"
#include "polar_lut.h"
#include "polar_params.h"
#include "scan_params.h"

namespace polar {

template <typename R>
struct ScanCfg {
    static constexpr int WAVES = 4;
    static constexpr size_t scratch_elems(int N, int n) { return 4 * (size_t)N + (size_t)(n - 1) * (size_t)(N / 2); }
    static constexpr size_t scratch_bytes(int N, int n) { return sizeof(R) * scratch_elems(N, n) * 64; }   // per wavefront
    static constexpr size_t lds_bytes() { return Lut<R>::bytes; }
};

// CHK-inf of the definition: b = +inf -> a; else a = +inf -> b; else chk.  chk_lut's value for an infinite operand is
// never used (its table index is clamped, so evaluating it is harmless).
template <typename R>
__device__ __forceinline__ R chk_inf(R a, R b, const Lut<R> &L)
{
    const R inf = R(__builtin_huge_val());
    R r = chk_lut<R>(a, b, L);
    r = (a == inf) ? b : r;
    r = (b == inf) ? a : r;
    return r;
}

template <typename R>
struct ScanBlock {
    const Lut<R> &lut;
    uint32_t fz;     // frozen mask of the 32-leaf block (uniform)
    uint32_t dec;    // decisions of the last iteration, bit k = leaf k
    bool first, last;
    R *br[4];        // stored right betas of the block's levels 1..4: element K0/2 + e of level t at br[t-1][(K0/2 + e)*64]
    R *lam;          // lambda of leaf k at lam[k*64]

    template <int T, int K0>
    static constexpr uint32_t span() { return (T == 5) ? 0xFFFFFFFFu : (((1u << ((1 << T) & 31)) - 1u) << K0); }

    // Node of 2^T leaves starting at leaf K0 of the block: alphas a[0..2^T) in, betas b[0..2^T) out.
    // Called only for a node that is entered: not all-frozen, and all-information only in the last iteration.
    template <int T, int K0>
    __device__ __forceinline__ void rec(const R *a, R *b)
    {
        const R inf = R(__builtin_huge_val());
        if constexpr (T == 0) {   // an information leaf in the last iteration
            lam[(size_t)K0 * 64] = a[0];
            dec |= ((a[0] < R(0)) ? 1u : 0u) << K0;
            b[0] = R(0);
        } else {
            constexpr int h = 1 << (T - 1);
            constexpr uint32_t sl = span<T - 1, K0>(), sr = span<T - 1, K0 + h>();
            const bool lF = (fz & sl) == sl, lI = (fz & sl) == 0u, rF = (fz & sr) == sr, rI = (fz & sr) == 0u;
            R *store = br[T >= 2 ? T - 2 : 0] + (size_t)(K0 / 2) * 64;   // the right child's level is T - 1 >= 1 when used: a leaf is never mixed
            R bl[h], brr[h];
            if (lF) {
#pragma unroll
                for (int e = 0; e < h; ++e) bl[e] = inf;
            } else if (lI && !last) {
#pragma unroll
                for (int e = 0; e < h; ++e) bl[e] = R(0);
            } else {
                R al[h];
                if (rF) {
#pragma unroll
                    for (int e = 0; e < h; ++e) al[e] = a[e];
                } else if (T < 2 || rI || first) {
#pragma unroll
                    for (int e = 0; e < h; ++e) al[e] = chk_lut<R>(a[e], a[e + h], lut);
                } else {
                    R p[h];
#pragma unroll
                    for (int e = 0; e < h; ++e) p[e] = store[(size_t)e * 64];
#pragma unroll
                    for (int e = 0; e < h; ++e) al[e] = chk_inf<R>(a[e], a[e + h] + p[e], lut);
                }
                rec<T - 1, K0>(al, bl);
            }
            if (rF) {
#pragma unroll
                for (int e = 0; e < h; ++e) brr[e] = inf;
            } else if (rI && !last) {
#pragma unroll
                for (int e = 0; e < h; ++e) brr[e] = R(0);
            } else {
                R ar[h];
                if (lF) {
#pragma unroll
                    for (int e = 0; e < h; ++e) ar[e] = a[e + h] + a[e];
                } else if (lI) {
#pragma unroll
                    for (int e = 0; e < h; ++e) ar[e] = a[e + h];
                } else {
#pragma unroll
                    for (int e = 0; e < h; ++e) ar[e] = a[e + h] + chk_inf<R>(a[e], bl[e], lut);
                }
                rec<T - 1, K0 + h>(ar, brr);
                if constexpr (T >= 2) {
                    if (!rI && !last) {
#pragma unroll
                        for (int e = 0; e < h; ++e) store[(size_t)e * 64] = brr[e];
                    }
                }
            }
            if (lI && rI) {   // an all-information node (last iteration): downwards only
#pragma unroll
                for (int e = 0; e < 2 * h; ++e) b[e] = R(0);
            } else if (lF) {
#pragma unroll
                for (int e = 0; e < h; ++e) {
                    b[e] = brr[e] + a[e + h];
                    b[e + h] = brr[e] + a[e];
                }
            } else if (rF) {
#pragma unroll
                for (int e = 0; e < h; ++e) {
                    b[e] = bl[e];
                    b[e + h] = inf;
                }
            } else {
#pragma unroll
                for (int e = 0; e < h; ++e) {
                    b[e] = chk_inf<R>(bl[e], brr[e] + a[e + h], lut);
                    b[e + h] = brr[e] + chk_inf<R>(bl[e], a[e], lut);
                }
            }
        }
    }
};

template <typename R, typename IN>
__global__ __launch_bounds__(256) void k_scan_lanes(ScanParams P)
{
    using Cfg = ScanCfg<R>;
    const int N = P.N, n = P.n, NW = N >> 5;   // 32 <= N <= 1024: the whole frozen mask is one word per lane
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Lut<R>::build(smem, threadIdx.x, blockDim.x);
    Lut<R> lut;
    lut.bind(smem);
    __syncthreads();   // the waves of a workgroup share the tables and nothing else

    const R inf = R(__builtin_huge_val());
    const int slot = blockIdx.x * Cfg::WAVES + wave, nslots = gridDim.x * Cfg::WAVES;
    R *base = reinterpret_cast<R *>(reinterpret_cast<unsigned char *>(P.scratch) + (size_t)slot * Cfg::scratch_bytes(N, n)) + lane;
    auto at = [&](size_t idx) -> R * { return base + idx * 64; };
    const size_t BL0 = 2 * (size_t)N, BR0 = 4 * (size_t)N, halfN = (size_t)(N / 2);
    const int nbatch = (P.B + 63) >> 6;

    const uint32_t fwv = (lane < NW) ? P.frozen[lane] : 0xFFFFFFFFu;   // lane l: frozen word of block l
    const uint64_t allF = __ballot(fwv == 0xFFFFFFFFu), allI = __ballot(fwv == 0u);
    // blocks b .. b + 2^(t-5) - 1: the leaves of the level-t node at block b
    auto blocks = [](int t, int b) -> uint64_t { return (((uint64_t)1 << (1 << (t - 5))) - 1u) << b; };   // t <= 10
    auto all_frozen = [&](int t, int b) -> bool { const uint64_t m = blocks(t, b); return (allF & m) == m; };
    auto all_info = [&](int t, int b) -> bool { const uint64_t m = blocks(t, b); return (allI & m) == m; };
    // where the node of level t at block b delivers its beta: root and left children to BL, right children to BR
    auto home = [&](int t, int b) -> R * {
        if (t == n || !((b >> (t - 5)) & 1)) return at(BL0 + ((size_t)1 << t));
        return at(BR0 + (size_t)(t - 1) * halfN + (((size_t)b << 5) - ((size_t)1 << t)) / 2);
    };

    for (int batch = slot; batch < nbatch; batch = next_job_wave(P.queue, batch, nslots, nbatch)) {
        const int frame0 = batch << 6;
        const bool have = frame0 + lane < P.B;   // the ragged last batch: idle lanes compute on zeros and store nothing
        const size_t frame = (size_t)(have ? frame0 + lane : 0);
        // ---- channel LLRs -> level n, sixteen consecutive elements of the lane's row per burst ----
        {
            const IN *row = reinterpret_cast<const IN *>(P.in) + frame * N;
            const bool al16 = ((reinterpret_cast<uintptr_t>(P.in) | ((size_t)N * sizeof(IN))) & 15u) == 0;   // uniform
            for (int e0 = 0; e0 < N; e0 += 16) {
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
                    *at((size_t)N + e0 + u) = (R)channel_llr(have ? (double)raw[u] : 0.0, P.sigma);
                }
            }
        }
        for (int it = 1; it <= P.iters; ++it) {
            const bool first = it == 1, last = it == P.iters;
            auto skipped = [&](int t, int b) -> bool { return all_frozen(t, b) || (!last && all_info(t, b)); };
            int t = n, b = 0;
            bool entering = true;
            for (;;) {
                if (entering) {
                    if (skipped(t, b)) {
                        entering = false;
                    } else if (t == 5) {
                        // ---- the 32-leaf block: level 5 from the scratch, levels 4..0 in registers ----
                        const uint32_t fz = (uint32_t)__builtin_amdgcn_readlane((int)fwv, b);
                        R x5[32], b5[32];
#pragma unroll
                        for (int u = 0; u < 32; ++u) x5[u] = *at(32 + u);
                        R *brb = at(BR0 + (size_t)b * 16);
                        ScanBlock<R> S{lut, fz, 0u, first, last, {brb, brb + halfN * 64, brb + 2 * halfN * 64, brb + 3 * halfN * 64}, at(0)};
                        S.template rec<5, 0>(x5, b5);
                        if (fz != 0u) {
                            R *H = home(5, b);
#pragma unroll
                            for (int u = 0; u < 32; ++u) H[(size_t)u * 64] = b5[u];
                        }
                        if (last) {
                            if (P.out_bits && have) P.out_bits[frame * NW + b] = S.dec;   // frozen leaves stay 0
                            if (P.llr_u && have) {
                                R *o = reinterpret_cast<R *>(P.llr_u) + frame * N + (size_t)b * 32;
#pragma unroll
                                for (int u = 0; u < 32; ++u) o[u] = ((fz >> u) & 1u) ? inf : *at(u);
                            }
                        }
                        entering = false;
                    } else {
                        // ---- left step: alpha of the left child (t-1, b) from this node's alpha and the stored right beta ----
                        const int h = 1 << (t - 1), nwc = 1 << (t - 6);
                        if (!skipped(t - 1, b)) {
                            const R *a = at((size_t)2 * h), *c = a + (size_t)h * 64;
                            R *o = at((size_t)h);
                            const bool rF = all_frozen(t - 1, b + nwc), plain = first || all_info(t - 1, b + nwc);
                            const R *pr = home(t - 1, b + nwc);
                            for (int e0 = 0; e0 < h; e0 += 8) {
                                R av[8], cv[8], pv[8];
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    av[u] = a[(size_t)(e0 + u) * 64];
                                    if (!rF) cv[u] = c[(size_t)(e0 + u) * 64];
                                    if (!rF && !plain) pv[u] = pr[(size_t)(e0 + u) * 64];
                                }
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    R v;
                                    if (rF) v = av[u];
                                    else if (plain) v = chk_lut<R>(av[u], cv[u], lut);
                                    else v = chk_inf<R>(av[u], cv[u] + pv[u], lut);
                                    o[(size_t)(e0 + u) * 64] = v;
                                }
                            }
                        }
                        --t;
                    }
                } else {
                    if (t == n) break;
                    const int nw = 1 << (t - 5), h = 1 << t;
                    const R *a = at((size_t)2 * h), *c = a + (size_t)h * 64;   // the parent's alpha, level t+1
                    if (!(b & nw)) {
                        // ---- right step: the left child (t, b) is done; alpha of its sibling (t, b + nw) ----
                        if (!skipped(t, b + nw)) {
                            const bool lF = all_frozen(t, b), lI = all_info(t, b);
                            const R *pl = at(BL0 + (size_t)h);
                            R *o = at((size_t)h);
                            for (int e0 = 0; e0 < h; e0 += 8) {
                                R av[8], cv[8], pv[8];
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    cv[u] = c[(size_t)(e0 + u) * 64];
                                    if (!lI) av[u] = a[(size_t)(e0 + u) * 64];
                                    if (!lI && !lF) pv[u] = pl[(size_t)(e0 + u) * 64];
                                }
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    R v;
                                    if (lF) v = cv[u] + av[u];
                                    else if (lI) v = cv[u];
                                    else v = cv[u] + chk_inf<R>(av[u], pv[u], lut);
                                    o[(size_t)(e0 + u) * 64] = v;
                                }
                            }
                        }
                        b += nw;
                        entering = true;
                    } else {
                        // ---- upwards: both children of (t+1, b - nw) are done; its beta goes to its home ----
                        const int pb = b - nw;
                        if (!all_info(t + 1, pb)) {
                            const bool lF = all_frozen(t, pb), lI = all_info(t, pb), rF = all_frozen(t, b), rI = all_info(t, b);
                            const R *pl = at(BL0 + (size_t)h), *pr = home(t, b);
                            R *H = home(t + 1, pb);
                            for (int e0 = 0; e0 < h; e0 += 8) {
                                R av[8], cv[8], lv[8], rv[8];
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    lv[u] = R(0);
                                    rv[u] = R(0);
                                    if (!rF) {
                                        av[u] = a[(size_t)(e0 + u) * 64];
                                        cv[u] = c[(size_t)(e0 + u) * 64];
                                    }
                                    if (!lF && !lI) lv[u] = pl[(size_t)(e0 + u) * 64];
                                    if (!rF && !rI) rv[u] = pr[(size_t)(e0 + u) * 64];
                                }
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    R lo, hi;
                                    if (lF) {
                                        lo = rv[u] + cv[u];
                                        hi = rv[u] + av[u];
                                    } else if (rF) {
                                        lo = lv[u];
                                        hi = inf;
                                    } else {
                                        lo = chk_inf<R>(lv[u], rv[u] + cv[u], lut);
                                        hi = rv[u] + chk_inf<R>(lv[u], av[u], lut);
                                    }
                                    H[(size_t)(e0 + u) * 64] = lo;
                                    H[(size_t)(e0 + u + h) * 64] = hi;
                                }
                            }
                        }
                        b = pb;
                        ++t;
                    }
                }
            }
        }
        // ---- what no block wrote: the all-frozen blocks' decisions and lambdas; then the root's beta ----
        if (have) {
            for (int b = 0; b < NW; ++b) {
                if (!all_frozen(5, b)) continue;
                if (P.out_bits) P.out_bits[frame * NW + b] = 0u;
                if (P.llr_u) {
                    R *o = reinterpret_cast<R *>(P.llr_u) + frame * N + (size_t)b * 32;
#pragma unroll
                    for (int u = 0; u < 32; ++u) o[u] = inf;
                }
            }
            if (P.ext_x) {
                R *o = reinterpret_cast<R *>(P.ext_x) + frame * N;
                const bool rootF = all_frozen(n, 0), rootI = all_info(n, 0);
                const R *H = at(BL0 + (size_t)N);
                for (int e0 = 0; e0 < N; e0 += 16) {
#pragma unroll
                    for (int u = 0; u < 16; ++u) o[e0 + u] = rootF ? inf : rootI ? R(0) : H[(size_t)(e0 + u) * 64];
                }
            }
        }
    }
}

}  // namespace polar
