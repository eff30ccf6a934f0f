// scl_q8.h -- fixed-point min-sum SC / SCL / CA-SCL on int8 LLRs (POLAR_Q8; the definition is the "Fixed-point min-sum"
// section of include/polar_hip.h, rules 1-7).
//
// One codeword per wavefront (block = one 64-lane wave), persistent, jobs from the work queue.  Lane = (slot p, position pos):
// p = lane / S, pos = lane % S, S = 64 / L.  Everything a codeword needs is in LDS, one BYTE per LLR:
//
//     ch[N]                    quantised channel LLRs (level n), shared by all paths
//     alpha[L][N (+ pad)]      level t (2^t values) at byte offset 2^t of each slot's row
//     blw[L][N/32], curw[..]   saved left-child partial sums / working partial sums, bit-packed (polar_bits.h)
//     cand[2L]                 the 32-bit candidate keys of rule 5
//
// A level of 4 or more elements moves whole dwords: a lane loads the two source dwords (4 + 4 int8), unpacks them with
// sign-extending bit-field extracts, applies f or g to the four pairs and stores one dword.  A row's stride is N + 4 S bytes
// for L >= 4, so that the slots that share a group of 32 lanes (the unit LDS banks a ds_read_b32 / ds_write_b32 in) start
// S dwords apart and a wave-instruction of the wide levels touches every bank once.
//
// Slots and ranks.  Rule 5 orders the live paths; a path's position in that order is its rank.  Moving a path to the slot of
// its rank would copy its partial sums at every information leaf, so a path keeps its slot (forks copy the per-level pointer
// table ptrA and one row of packed partial sums, as scl_generic.h does: fork_source of scl_wave_ops.h, which also holds the
// partial-sum rows, the path choice and the epilogue) and carries its rank in a register.  The rank is only ever read as the
// low bits of a key.
//
// Ranking is by counting: every path counts the keys below its two candidate keys (all keys differ), which IS the position
// in the sorted order.  No floating point anywhere in this file's kernels except the quantiser, which is rule 1.
#pragma once
#include "polar_params.h"
#include "scl_wave_ops.h"

namespace polar {

struct Q8Params {
    const int8_t *in;          // [B][N] quantised channel LLRs, rows 4-byte aligned
    uint32_t *out_bits;        // [B][N/32]
    int32_t *pm;               // [B] or null
    uint32_t *flags;           // [B] or null
    const uint32_t *frozen;    // [N/32] bit j = leaf j frozen
    const uint32_t *crc_tab;   // [N] or null = no CRC
    int N, n, B;
    int sc_mode;               // 1: POLAR_ALGO_SC (L = 1, metric 0, flags 0)
    int Cc, Ci;                // clamp of the channel values / of the internal values
    unsigned *queue;           // job counter, null = fixed stride
};

// rule 1 from t = v * scale on: round to nearest even, clamp, NaN -> 0 (the same text on the host and on the device)
__host__ __device__ inline int8_t q8_round_clamp(double t, int Cc)
{
    if (t != t) return 0;
    const double r = __builtin_rint(t);
    return (int8_t)(r < (double)-Cc ? -Cc : r > (double)Cc ? Cc : (int)r);
}

// rule 2
__device__ __forceinline__ int q8_f(int a, int b)
{
    const int m = min(abs(a), abs(b));
    return ((a ^ b) < 0) ? -m : m;
}
__device__ __forceinline__ int q8_g(int a, int b, uint32_t u, int Ci) { return min(max(b + (u ? -a : a), -Ci), Ci); }
__device__ __forceinline__ int q8_byte(uint32_t w, int k) { return (int)(int8_t)(w >> (8 * k)); }
__device__ __forceinline__ uint32_t q8_pack(int a, int b, int c, int d)
{
    return ((uint32_t)a & 255u) | (((uint32_t)b & 255u) << 8) | (((uint32_t)c & 255u) << 16) | ((uint32_t)d << 24);
}

template <int LOGL>
constexpr int q8_row_bytes(int N)
{
    return N + (LOGL >= 2 ? 4 * (64 >> LOGL) : 0);
}
template <int LOGL>
constexpr size_t scl_q8_lds_bytes(int N)
{
    return (size_t)N + (size_t)(1 << LOGL) * q8_row_bytes<LOGL>(N) + 2 * sizeof(uint32_t) * (size_t)(N / 32) * (1 << LOGL) +
           sizeof(uint32_t) * 2 * (1 << LOGL);
}

template <int LOGL>
__global__ __launch_bounds__(64) void k_scl_q8(Q8Params P)
{
    constexpr int L = 1 << LOGL;
    constexpr int S = 64 / L;
    const int N = P.N, n = P.n, NW = N >> 5, ROW = q8_row_bytes<LOGL>(N);
    const int Ci = P.Ci;
    const int lane = threadIdx.x;
    const int p = lane / S, pos = lane % S;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int8_t *ch = reinterpret_cast<int8_t *>(smem);
    int8_t *alpha = ch + N;
    uint32_t *blw = reinterpret_cast<uint32_t *>(alpha + (size_t)L * ROW);
    uint32_t *curw = blw + (size_t)L * NW;
    uint32_t *cand = curw + (size_t)L * NW;

    for (int frame = blockIdx.x; frame < P.B; frame = next_job_wave(P.queue, frame, (int)gridDim.x, P.B)) {
        // ---- channel row, clamped to [-Cc, Cc] on load (rule 1) ----
        {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(P.in + (size_t)frame * N);
            const int Cc = P.Cc;
            for (int i = lane; i < (N >> 2); i += 64) {
                const uint32_t w = src[i];
                reinterpret_cast<uint32_t *>(ch)[i] =
                    q8_pack(min(max(q8_byte(w, 0), -Cc), Cc), min(max(q8_byte(w, 1), -Cc), Cc),
                            min(max(q8_byte(w, 2), -Cc), Cc), min(max(q8_byte(w, 3), -Cc), Cc));
            }
        }
        __syncthreads();

        int PM = 0, rk = 0;
        uint64_t ptrA = 0;
        uint32_t crc = 0, bl0 = 0, cur0 = 0;
        uint32_t fl = 0;
        int act = 1;

        for (int j = 0; j < N; ++j) {
            // ================= LLR of leaf j for every active path =================
            int tf;
            if (j > 0) {
                const int d = __builtin_ctz((unsigned)j);
                const int h = 1 << d;
                if (p < act) {
                    const int8_t *src = (d + 1 == n) ? ch : alpha + (size_t)ptr_get<LOGL>(ptrA, d + 1) * ROW + (2 << d);
                    int8_t *out = alpha + (size_t)p * ROW + h;
                    if (h >= 4) {
                        for (int e = 4 * pos; e < h; e += 4 * S) {
                            const int bi = h + e;
                            const uint32_t wv = (bi < 32) ? bl0 : blw[p * NW + (bi >> 5)];
                            const uint32_t u4 = wv >> (bi & 31);
                            const uint32_t a4 = *reinterpret_cast<const uint32_t *>(src + e);
                            const uint32_t b4 = *reinterpret_cast<const uint32_t *>(src + e + h);
                            *reinterpret_cast<uint32_t *>(out + e) =
                                q8_pack(q8_g(q8_byte(a4, 0), q8_byte(b4, 0), u4 & 1u, Ci), q8_g(q8_byte(a4, 1), q8_byte(b4, 1), u4 & 2u, Ci),
                                        q8_g(q8_byte(a4, 2), q8_byte(b4, 2), u4 & 4u, Ci), q8_g(q8_byte(a4, 3), q8_byte(b4, 3), u4 & 8u, Ci));
                        }
                    } else if (pos < h) {
                        out[pos] = (int8_t)q8_g(src[pos], src[pos + h], (bl0 >> (h + pos)) & 1u, Ci);
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
                    const int8_t *src = (t + 1 == n) ? ch : alpha + (size_t)ptr_get<LOGL>(ptrA, t + 1) * ROW + (2 << t);
                    int8_t *out = alpha + (size_t)p * ROW + h;
                    if (h >= 4) {
                        for (int e = 4 * pos; e < h; e += 4 * S) {
                            const uint32_t a4 = *reinterpret_cast<const uint32_t *>(src + e);
                            const uint32_t b4 = *reinterpret_cast<const uint32_t *>(src + e + h);
                            *reinterpret_cast<uint32_t *>(out + e) =
                                q8_pack(q8_f(q8_byte(a4, 0), q8_byte(b4, 0)), q8_f(q8_byte(a4, 1), q8_byte(b4, 1)),
                                        q8_f(q8_byte(a4, 2), q8_byte(b4, 2)), q8_f(q8_byte(a4, 3), q8_byte(b4, 3)));
                        }
                    } else if (pos < h) {
                        out[pos] = (int8_t)q8_f(src[pos], src[pos + h]);
                    }
                    ptrA = ptr_set<LOGL>(ptrA, t, p);
                }
                __syncthreads();
            }
            const int lam = (p < act) ? (int)alpha[(size_t)p * ROW + 1] : 0;
            const int al = abs(lam);
            const bool hard = lam < 0;

            // ================= decision =================
            const bool frozen = (P.frozen[j >> 5] >> (j & 31)) & 1;
            int bit = 0;
            if (P.sc_mode) {
                bit = (!frozen && hard) ? 1 : 0;   // rule 6, POLAR_ALGO_SC
            } else if (frozen) {
                if (p < act && hard) PM += al;     // rule 4
            } else {
                // rule 5: the two candidates of every live path and their keys; position in the sorted order = keys below
                const int c0 = PM + (hard ? al : 0);
                const int c1 = PM + (hard ? 0 : al);
                const uint32_t k0 = ((uint32_t)c0 << 6) | (uint32_t)rk;
                const uint32_t k1 = ((uint32_t)c1 << 6) | 32u | (uint32_t)rk;
                if (pos == 0 && p < act) {
                    cand[p] = k0;
                    cand[p + act] = k1;
                }
                __syncthreads();
                int n0 = 0, n1 = 0;
                for (int m = 0; m < 2 * act; ++m) {
                    const uint32_t v = cand[m];
                    n0 += (v < k0);
                    n1 += (v < k1);
                }
                if (act < L) {
                    // 2m <= L: every candidate is kept; the 1-branch of slot k goes to slot k + act
                    const bool is_new = (p >= act) && (p < 2 * act);
                    const int sg = is_new ? p - act : p;
                    const int sl = sg * S + pos;
                    const int c1_s = __shfl(c1, sl);
                    const int n1_s = __shfl(n1, sl);
                    ptrA = __shfl(ptrA, sl);
                    crc = __shfl(crc, sl);
                    bl0 = __shfl(bl0, sl);
                    if (is_new) {
                        for (int w = 1 + pos; w < NW; w += S) blw[p * NW + w] = blw[sg * NW + w];
                        bit = 1;
                        PM = c1_s;
                        rk = n1_s;
                    } else if (p < act) {
                        PM = c0;
                        rk = n0;
                    }
                    act *= 2;
                    __syncthreads();
                } else {
                    // 2L candidates, the L of least key survive
                    const bool s0 = n0 < L, s1 = n1 < L;
                    const bool lead = pos == 0;
                    // POLAR_FLAG_TIE: the candidates at sorted positions L - 1 and L have equal PM_c
                    const int vA = (n0 == L - 1) ? c0 : (n1 == L - 1) ? c1 : -1;
                    const int vB = (n0 == L) ? c0 : (n1 == L) ? c1 : -1;
                    const uint64_t mA = __ballot(lead && vA >= 0);
                    const uint64_t mB = __ballot(lead && vB >= 0);
                    if (__shfl(vA, __builtin_ctzll(mA)) == __shfl(vB, __builtin_ctzll(mB))) fl |= 0x1u;
                    const uint64_t m_s0 = __ballot(lead && s0);
                    const uint64_t m_s1 = __ballot(lead && s1);
                    const uint64_t m_both = m_s0 & m_s1;
                    const uint64_t m_dead = __ballot(lead) & ~(m_s0 | m_s1);
                    const bool dead = !s0 && !s1;
                    // exactly L keys are below the L-th, so there are as many dead slots as both-survivors: every dead
                    // slot is refilled, and `dead` stands for fork_source's result below
                    int sg = p;
                    fork_source<S>(m_both, m_dead, p, dead, sg);
                    const int sl = sg * S + pos;
                    const int c1_s = __shfl(c1, sl);
                    const int n1_s = __shfl(n1, sl);
                    ptrA = __shfl(ptrA, sl);
                    crc = __shfl(crc, sl);
                    bl0 = __shfl(bl0, sl);
                    if (dead) {
                        for (int w = 1 + pos; w < NW; w += S) blw[p * NW + w] = blw[sg * NW + w];
                        bit = 1;
                        PM = c1_s;
                        rk = n1_s;
                    } else if (s0) {
                        bit = 0;   // the 0-branch keeps the slot, alone or with its 1-branch forked away
                        PM = c0;
                        rk = n0;
                    } else {
                        bit = 1;
                        PM = c1;
                        rk = n1;
                    }
                    __syncthreads();
                }
            }

            // ================= partial sums (updateBit: polar_bits.h, scl_wave_ops.h) =================
            if (P.crc_tab && bit) crc ^= P.crc_tab[j];
            cur0 = (uint32_t)bit;
            int t = 0;
            while (t < n && ((j >> t) & 1)) {
                if (t < 5) cur0 = ps_fold0(bl0, cur0, t);
                else ps_update_rows<S>(blw, curw, NW, p, pos, act, cur0, t);
                ++t;
            }
            if (t < n) {
                if (t < 5) bl0 = ps_save0(bl0, cur0, t);
                else ps_save_rows<S>(blw, curw, NW, p, pos, act, cur0, t);
            }
        }

        // ================= choose the path (rule 6): least (PM, rank), among the CRC-passing paths if any =================
        int best = 0;
        uint32_t best_key = 0;
        if (!P.sc_mode) {
            const bool pass = (P.crc_tab != nullptr) && (crc == 0);
            const bool any = __ballot(pass && p < act) != 0ull;
            const uint32_t key = ((uint32_t)PM << 5) | (uint32_t)rk;
            best = -1;
            for (int q = 0; q < act; ++q) {
                const uint32_t kq = __shfl(key, q * S);
                const int okq = __shfl((int)(any ? pass : true), q * S);
                if (okq && (best < 0 || kq < best_key)) {
                    best = q;
                    best_key = kq;
                }
            }
            if (any) fl |= 0x2u;
        }
        // x_hat of the chosen path: root partial sums; u_hat = x_hat * F^{(x)n}
        if (n <= 5) {
            const uint32_t x = polar_word_transform_n(__shfl(cur0, best * S), n);
            if (lane == 0) P.out_bits[(size_t)frame * NW] = x;
        } else {
            uhat_from_rows(curw + (size_t)best * NW, NW, n, lane, P.out_bits + (size_t)frame * NW);
        }
        if (lane == 0) {
            if (P.pm) P.pm[frame] = P.sc_mode ? 0 : (int32_t)(best_key >> 5);
            if (P.flags) P.flags[frame] = P.sc_mode ? 0u : fl;
        }
        __syncthreads();
    }
}

// rule 1 on the device: one element per lane, coalesced
template <typename IN>
__global__ __launch_bounds__(256) void k_q8_quantize(const IN *in, int8_t *out, size_t count, double sigma, double scale, int Cc)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double v = (double)in[i];
    if (sigma > 0) v = llr_from_y(v, sigma);
    out[i] = q8_round_clamp(v * scale, Cc);
}

// the int32 metric as the double the float entry points report (exact: PM < 2^17)
__global__ __launch_bounds__(256) void k_q8_pm_f64(const int32_t *pm, double *out, size_t count)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = (double)pm[i];
}

}  // namespace polar
