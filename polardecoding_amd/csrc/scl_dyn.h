// scl_dyn.h -- SC / SCL / CA-SCL with dynamic frozen bits (include/polar_hip.h, "Dynamic frozen bits"): PAC codes, the
// parity-check bits of 5G PC-polar codes, any lower-triangular precoding.
//
// k_scl_dyn is k_scl_generic (scl_generic.h: one codeword per wavefront, lane = (path p, position pos), the same LDS layout,
// pointer table, schedule, survivor and tie rule, the same GA variant) plus what a dynamic frozen leaf needs:
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
// wave-uniform control flow (j and the row index are wave-uniform); lanes of dead paths compute and discard.
//
// k_generate_dyn is gen_kernel.h's transmit chain with the dynamic bits filled in ascending position before the encode.
#pragma once
#include "gen_common.h"
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
    const SclParams &P = DP.s;
    constexpr int L = 1 << LOGL;
    constexpr int S = 64 / L;
    const int N = P.N, n = P.n, NW = N >> 5;
    const int lane = threadIdx.x;
    const int p = lane / S, pos = lane % S;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    R *ch, *alpha;
    uint32_t *blw;
    if constexpr (GA) {
        ch = reinterpret_cast<R *>(P.scratch) + (size_t)blockIdx.x * (size_t)(L + 1) * N;
        alpha = ch + N;
        blw = reinterpret_cast<uint32_t *>(smem);
    } else {
        ch = reinterpret_cast<R *>(smem);
        alpha = ch + N;
        blw = reinterpret_cast<uint32_t *>(alpha + (size_t)L * N);
    }
    uint32_t *curw = blw + (size_t)L * NW;
    R *cand = reinterpret_cast<R *>(curw + (size_t)L * NW);
    uint32_t *hist = reinterpret_cast<uint32_t *>(cand + 2 * L);   // behind cand: L * NW may be odd, cand holds doubles
    unsigned char *lut_mem = reinterpret_cast<unsigned char *>(hist + (size_t)L * NW);
    lut_mem += (16 - (reinterpret_cast<uintptr_t>(lut_mem) & 15)) & 15;
    Lut<R>::build(lut_mem, lane, 64);
    Lut<R> lut;
    lut.bind(lut_mem);
    __syncthreads();
    auto ld = [](const R *q) -> R {
        if constexpr (GA) return ld_bypass(q);
        else return *q;
    };

    for (int frame = blockIdx.x; frame < P.B; frame = next_job_wave(P.queue, frame, (int)gridDim.x, P.B)) {
        {
            const IN *src = reinterpret_cast<const IN *>(P.in) + (size_t)frame * N;
            for (int i = lane; i < N; i += 64) {
                double v = (double)src[i];
                if (P.sigma > 0) v = llr_from_y(v, P.sigma);
                ch[i] = (R)v;
            }
        }
        for (int w = lane; w < L * NW; w += 64) hist[w] = 0u;
        __syncthreads();

        R PM = R(0);
        uint64_t ptrA = 0;
        uint32_t crc = 0, bl0 = 0, cur0 = 0, h0 = 0;
        uint32_t fl = 0;
        int act = 1;

        for (int j = 0; j < N; ++j) {
            // ================= LLR of leaf j for every active path (scl_generic.h) =================
            int tf;
            if (j > 0) {
                const int d = __builtin_ctz((unsigned)j);
                const int h = 1 << d;
                if (p < act) {
                    const R *src = (d + 1 == n) ? ch : alpha + (size_t)ptr_get<LOGL>(ptrA, d + 1) * N + (2 << d);
                    R *out = alpha + (size_t)p * N + h;
                    for (int e = pos; e < h; e += S) {
                        const int bi = h + e;
                        const uint32_t wv = (bi < 32) ? bl0 : blw[p * NW + (bi >> 5)];
                        out[e] = gfun<R>(ld(src + e), ld(src + e + h), (wv >> (bi & 31)) & 1);
                    }
                    ptrA = ptr_set<LOGL>(ptrA, d, p);
                }
                __syncthreads();
                tf = d - 1;
            } else {
                tf = n - 1;
            }
            for (int t = tf; t >= 0; --t) {
                const int h = 1 << t;
                if (p < act) {
                    const R *src = (t + 1 == n) ? ch : alpha + (size_t)ptr_get<LOGL>(ptrA, t + 1) * N + (2 << t);
                    R *out = alpha + (size_t)p * N + h;
                    for (int e = pos; e < h; e += S) out[e] = chk_lut<R>(ld(src + e), ld(src + e + h), lut);
                    ptrA = ptr_set<LOGL>(ptrA, t, p);
                }
                __syncthreads();
            }
            const R lam = (p < act) ? ld(alpha + (size_t)p * N + 1) : R(0);

            // ================= decision =================
            const bool frozen = (P.frozen[j >> 5] >> (j & 31)) & 1;
            const int row = DP.row[j];   // wave-uniform
            int bit = 0;
            if (row >= 0) {
                // dynamic frozen leaf: b = parity of (history AND mask row) over the words 0 .. j >> 5, every lane of the wave
                const uint32_t *mrow = DP.mask + (size_t)row * NW;
                uint32_t par = 0;
                for (int w = pos; w <= (j >> 5); w += S) {
                    const uint32_t hw = (w == 0) ? h0 : hist[p * NW + w];
                    par ^= (uint32_t)__popc(hw & mrow[w]);
                }
                for (int o = S >> 1; o > 0; o >>= 1) par ^= (uint32_t)__shfl_xor((int)par, o);
                bit = (int)(par & 1u);
                if (!P.sc_mode && p < act) PM = PM + (lut.tabv(lam) + (bit ? posmax(lam) : negmax(lam)));   // PHI(., b)
            } else if (P.sc_mode) {
                bit = (!frozen && lam < R(0)) ? 1 : 0;
            } else if (frozen) {
                if (p < act) PM += lut.tabv(lam) + negmax(lam);
            } else if (act < L) {
                // phase 1: every path forks, clone k -> k + act
                const bool is_new = (p >= act) && (p < 2 * act);
                const int sg = is_new ? p - act : p;
                const int sl = sg * S + pos;
                const R lam_s = __shfl(lam, sl);
                const R pm_s = __shfl(PM, sl);
                ptrA = __shfl(ptrA, sl);
                crc = __shfl(crc, sl);
                bl0 = __shfl(bl0, sl);
                h0 = __shfl(h0, sl);
                if (is_new) {
                    for (int w = 1 + pos; w < NW; w += S) {
                        blw[p * NW + w] = blw[sg * NW + w];
                        hist[p * NW + w] = hist[sg * NW + w];
                    }
                    bit = 1;
                    PM = pm_s + (lut.tabv(lam_s) + posmax(lam_s));
                } else if (p < act) {
                    PM = PM + (lut.tabv(lam) + negmax(lam));
                }
                act *= 2;
                __syncthreads();
            } else {
                // phase 2: keep the L best of 2L candidates; survivor and tie rule of scl_generic.h
                const R tt = lut.tabv(lam);
                const R c0 = PM + (tt + negmax(lam));
                const R c1 = PM + (tt + posmax(lam));
                if (pos == 0) {
                    cand[p] = c0;
                    cand[p + L] = c1;
                }
                __syncthreads();
                int n0 = 0, n1 = 0;
                for (int m = 0; m < 2 * L; ++m) {
                    const R v = cand[m];
                    n0 += (v <= c0);
                    n1 += (v <= c1);
                }
                const bool s0 = n0 <= L, s1 = n1 <= L;
                const bool lead = pos == 0;
                const uint64_t m_s0 = __ballot(lead && s0);
                const uint64_t m_s1 = __ballot(lead && s1);
                const uint64_t m_both = m_s0 & m_s1;
                const uint64_t m_dead = __ballot(lead) & ~(m_s0 | m_s1);
                if (__popcll(m_s0) + __popcll(m_s1) < L) fl |= 0x1u;  // median tie
                const bool dead = !s0 && !s1;
                const int myrank = __popcll(m_dead & ((1ull << (p * S)) - 1ull));
                int sg = p;
                bool refilled = false;
                {
                    uint64_t bm = m_both;
                    int cnt = 0;
                    while (bm) {
                        const int b = __builtin_ctzll(bm);
                        if (dead && cnt == myrank) {
                            sg = b / S;
                            refilled = true;
                        }
                        bm &= bm - 1;
                        ++cnt;
                    }
                }
                const int sl = sg * S + pos;
                const R c1_s = __shfl(c1, sl);
                ptrA = __shfl(ptrA, sl);
                crc = __shfl(crc, sl);
                bl0 = __shfl(bl0, sl);
                h0 = __shfl(h0, sl);
                if (refilled) {
                    for (int w = 1 + pos; w < NW; w += S) {
                        blw[p * NW + w] = blw[sg * NW + w];
                        hist[p * NW + w] = hist[sg * NW + w];
                    }
                    bit = 1;
                    PM = c1_s;
                } else if (s0) {
                    bit = 0;
                    PM = c0;
                } else if (s1) {
                    bit = 1;
                    PM = c1;
                } else {
                    bit = 0;  // an un-refilled dead slot continues as its 0-branch
                    PM = c0;
                }
                __syncthreads();
            }

            // ================= history: bit j of the path's decided bits =================
            if (j < 32) {
                h0 |= (uint32_t)bit << j;
            } else {
                if (pos == 0 && p < act && bit) hist[p * NW + (j >> 5)] |= 1u << (j & 31);
                __syncthreads();
            }

            // ================= partial sums (scl_generic.h) =================
            if (P.crc_tab && bit) crc ^= P.crc_tab[j];
            cur0 = (uint32_t)bit;
            int t = 0;
            while (t < n && ((j >> t) & 1)) {
                if (t < 5) {
                    const int h = 1 << t;
                    const uint32_t mask = (1u << h) - 1u;
                    const uint32_t l = (bl0 >> h) & mask;
                    const uint32_t c = cur0 & mask;
                    cur0 = (l ^ c) | (c << h);
                } else {
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
                ++t;
            }
            if (t < n) {
                if (t < 5) {
                    const int h = 1 << t;
                    const uint32_t mask = (1u << h) - 1u;
                    bl0 = (bl0 & ~(mask << h)) | ((cur0 & mask) << h);
                } else {
                    const int nw = 1 << (t - 5);
                    if (t == 5) {
                        if (pos == 0 && p < act) blw[p * NW + 1] = cur0;
                    } else if (p < act) {
                        for (int w = pos; w < nw; w += S) blw[p * NW + nw + w] = curw[p * NW + w];
                    }
                    __syncthreads();
                }
            }
        }

        // ================= choose the path (scl_generic.h) =================
        int best = 0;
        R best_pm = PM;
        if (!P.sc_mode) {
            const bool pass = (P.crc_tab != nullptr) && (crc == 0);
            const bool any = __ballot(pass && p < act) != 0ull;
            best = -1;
            best_pm = R(0);
            for (int q = 0; q < act; ++q) {
                const R pq = __shfl(PM, q * S);
                const int okq = __shfl((int)(any ? pass : true), q * S);
                if (okq && (best < 0 || pq < best_pm)) {
                    best = q;
                    best_pm = pq;
                }
            }
            if (any) fl |= 0x2u;
        }
        // u_hat of the chosen path is its history, dynamic bits included
        {
            const uint32_t w0 = __shfl(h0, best * S);
            for (int w = lane; w < NW; w += 64) P.out_bits[(size_t)frame * NW + w] = (w == 0) ? w0 : hist[best * NW + w];
        }
        if (lane == 0) {
            if (P.pm) P.pm[frame] = P.sc_mode ? 0.0 : (double)best_pm;
            if (P.flags) P.flags[frame] = P.sc_mode ? 0u : fl;
        }
        __syncthreads();
    }
}

template <typename R, int LOGL>
constexpr size_t scl_dyn_lds_bytes(int N, bool ga)
{
    return scl_generic_lds_bytes<R, LOGL>(N, ga) + sizeof(uint32_t) * (size_t)(N / 32) * (1 << LOGL);
}

struct GenDynParams {
    GenParams g;
    const uint32_t *mask;   // [D][N/32]
    const int *pos;         // [D] ascending
    int D;
};

// k_generate (gen_kernel.h) with the dynamic bits: payload, CRC and placement are the plain context's (same Philox stream 0),
// then u[pos[d]] = parity of (u AND mask row d) for d = 0 .. D-1 in ascending position, then encode and channel (stream 1).
__global__ __launch_bounds__(256) void k_generate_dyn(GenDynParams G)
{
    const GenParams &P = G.g;
    const int N = P.N, NW = N >> 5, KR = N >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    extern __shared__ unsigned char gsm[];
    unsigned char *ub = gsm + (size_t)wave * (N + 2 * 1024);
    uint32_t *vw = reinterpret_cast<uint32_t *>(ub + N);
    const int waves = blockDim.x >> 6;
    for (int f = blockIdx.x * waves + wave; f < P.B; f += gridDim.x * waves) {
        const uint64_t frame = P.first_frame + (uint64_t)f;
        const int kw = (P.K + 31) >> 5;
        for (int w = lane; w < kw + 2; w += 64) {
            uint32_t v = 0;
            if (w < kw) {
                v = Philox(P.seed, frame, (uint32_t)w, 0u).c[0];
                if (w == kw - 1 && (P.K & 31)) v &= (1u << (P.K & 31)) - 1u;
            }
            vw[w] = v;
        }
        for (int j = lane; j < N; j += 64) ub[j] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (P.gc_rows) {
            uint32_t par = 0;
            for (int k = lane; k < P.K; k += 64)
                if ((vw[k >> 5] >> (k & 31)) & 1u) par ^= P.gc_rows[k];
            for (int o = 32; o > 0; o >>= 1) par ^= __shfl_xor(par, o);
            for (int i = lane; i < P.A; i += 64) {
                const int q = i - P.crc_r;
                const uint32_t bit = (q < 0) ? ((par >> i) & 1u) : ((vw[q >> 5] >> (q & 31)) & 1u);
                ub[P.info_order[i]] = (unsigned char)bit;
            }
        } else {
            for (int i = lane; i < P.A; i += 64) {
                uint32_t bit = 0;
                for (int t = 0; t <= P.crc_r; ++t) {
                    const bool tap = (t < 32) ? ((P.crc_mask >> t) & 1u) : (P.crc_top != 0);
                    const int q = i - t;
                    if (tap && q >= 0 && q < P.K) bit ^= (vw[q >> 5] >> (q & 31)) & 1u;
                }
                ub[P.info_order[i]] = (unsigned char)bit;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // dynamic bits, ascending position: a row only refers to earlier positions
        for (int d = 0; d < G.D; ++d) {
            const int j = G.pos[d];
            const uint32_t *mrow = G.mask + (size_t)d * NW;
            uint32_t par = 0;
            for (int i = lane; i < j; i += 64) par ^= (uint32_t)ub[i] & (mrow[i >> 5] >> (i & 31));
            for (int o = 32; o > 0; o >>= 1) par ^= __shfl_xor(par, o);
            if (lane == 0) ub[j] = (unsigned char)(par & 1u);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        uint64_t u = 0;
        for (int k = 0; k < KR; ++k) u |= (uint64_t)(ub[lane + 64 * k] & 1) << k;
        if (P.u_bits) {
            for (int k = 0; k < KR; ++k) {
                const uint64_t m = __ballot((u >> k) & 1ull);
                if (lane == 0) {
                    P.u_bits[(size_t)f * NW + 2 * k] = (uint32_t)m;
                    P.u_bits[(size_t)f * NW + 2 * k + 1] = (uint32_t)(m >> 32);
                }
            }
        }
        uint64_t x = u;
        for (int s = 0; s < 6 && s < P.n; ++s) {
            const uint64_t o = __shfl_xor((unsigned long long)x, 1 << s);
            if (!(lane & (1 << s))) x ^= o;
        }
        for (int s = 6; s < P.n; ++s) {
            const int sh = 1 << (s - 6);
            uint64_t msk = 0;
            for (int k = 0; k < KR; ++k)
                if (!(k & sh)) msk |= 1ull << k;
            x ^= (x >> sh) & msk;
        }
        for (int k2 = 0; k2 < KR; k2 += 2) {
            const Philox g(P.seed, frame, (uint32_t)(lane + 64 * (k2 >> 1)), 1u);
            const double r = sqrt(-2.0 * log(g.u0()));
            double sn, cs;
            sincospi(2.0 * g.u1(), &sn, &cs);
            const double nz[2] = {r * cs, r * sn};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = k2 + h;
                if (k >= KR) break;
                const int j = lane + 64 * k;
                const double y = (((x >> k) & 1ull) ? -1.0 : 1.0) + P.sigma * nz[h];
                const double v = P.out_is_y ? y : 2 * y / P.sigma / P.sigma;
                if (P.out_is_f32) reinterpret_cast<float *>(P.out)[(size_t)f * N + j] = (float)v;
                else reinterpret_cast<double *>(P.out)[(size_t)f * N + j] = v;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace polar
