// scl_generic.h -- generic (any N, any L = 2^LOGL <= 32) SC / SCL / CA-SCL decode kernel.
//
// One codeword per wavefront (block = one 64-lane wave).  Lane = (path p, position pos):
// p = lane / S, pos = lane % S, S = 64 / L.  All LLR levels live in LDS:
//
//     ch[N]                    channel LLRs (level n), shared by all paths
//     alpha[L][N]              level t (2^t values) at offset 2^t of each slot's row
//     blw[L][N/32], curw[..]   saved left-child partial sums / working partial sums, bit-packed (polar_bits.h)
//
// The reference clones whole factor graphs on every fork (copyPath / simpleCopy,
// SCL_1024.c:451-478: 81 % of its run time).  Here a fork copies a per-level pointer table
// (ptrA) instead: every slot owns one buffer per level, writes always go to the slot's own
// buffer, and in the lock-step schedule every live path rewrites level t before anybody reads
// it again.  The decided bits u_hat are never stored per path: the partial sums of the chosen
// path at the root are its codeword x_hat, and u_hat = x_hat * F^{(x)n} (F is an involution).
//
// Schedule = the reference's lazy recursion getLLR/updateBit (SCL_1024.c:404-448) in its
// natural-order form.  This kernel is the correctness baseline and
// the fallback for shapes without a tuned instantiation; scl_fast.h holds the tuned ones.
// The steps it shares with k_scl_q8 (fork pairing, partial sums at levels >= 5, path choice, epilogue) are scl_wave_ops.h's.
//
// The kernel text is scl_generic_body<..., DYN>; k_scl_generic is its DYN = false wrapper and k_scl_dyn (scl_dyn.h, which
// says what DYN adds: a per-path history of the decided bits and the dynamic frozen leaf) its DYN = true wrapper.
#pragma once
#include "polar_math.h"
#include "polar_lut.h"
#include "polar_params.h"
#include "list_out.h"
#include "trace_out.h"
#include "book_desc.h"
#include "scl_wave_ops.h"

namespace polar {

// GA = false: every LLR level of every path in LDS.  GA = true ("LLRs spill HBM", BASELINE config 5): the
// level arrays alpha[L][N] live in a per-workgroup slice of a global scratch buffer and the channel LLRs are
// read from the input; only the bit-packed partial sums stay in LDS.
// DYN = false: dyn_mask and dyn_row are never read.
// LIST = true (needs DYN, k_list.hip): the decode is the same; the epilogue writes every live slot to *LO in ascending
// (PM, slot) instead of the chosen path to P.out_bits / P.pm.  LIST = false: LO is never read.
// BOOK = true (needs DYN, k_book.hip): a code book.  P.N / P.n are the largest member's and fix the LDS layout, the scratch
// slice and the width of the output rows once per workgroup; every frame takes N, n, the frozen mask, the CRC table, the
// constraint tables and sc_mode from the descriptor BK->codes[BK->code[frame]] (book_desc.h), and its loops and row strides
// run on its own N.  Whatever a longer earlier frame left in LDS lies outside this frame's rows or is rewritten before it
// is read; hist, the one array read before it is written, is cleared over this frame's rows.  Output words from N / 32 up
// to P.N / 32 are written as 0, and every output is nullable.  BOOK = false: BK is never read.
// TRACE = true (needs DYN, not with LIST or BOOK; k_trace.hip): the decode is the same; every slot carries the match flag of
// trace_out.h, and the epilogue writes the frame's five trace words to *TO instead of the chosen path.  Every __ballot and
// __shfl it adds sits in wave-uniform control flow; the lanes choose what they contribute with ?:.  TRACE = false: TO is
// never read.
template <typename R, typename IN, int LOGL, bool GA, bool DYN, bool LIST = false, bool BOOK = false, bool TRACE = false>
__device__ __forceinline__ void scl_generic_body(const SclParams &P, const uint32_t *dyn_mask, const int *dyn_row,
                                                 const ListOut *LO = nullptr, const BookArgs *BK = nullptr,
                                                 const TraceOut *TO = nullptr)
{
    static_assert(DYN || !LIST, "the list epilogue reads the per-path history");
    static_assert(DYN || !BOOK, "a code book runs the dynamic leaf of every member");
    static_assert(!TRACE || (DYN && !LIST && !BOOK), "the trace runs the list decode of one code and has its own epilogue");
    constexpr int L = 1 << LOGL;
    constexpr int S = 64 / L;
    const int NL = P.N, NWL = NL >> 5;   // the layout's N: the frame's own N but in a code book
    const int lane = threadIdx.x;
    const int p = lane / S, pos = lane % S;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    R *ch, *alpha;
    uint32_t *blw;
    if constexpr (GA) {
        ch = reinterpret_cast<R *>(P.scratch) + (size_t)blockIdx.x * (size_t)(L + 1) * NL;
        alpha = ch + NL;
        blw = reinterpret_cast<uint32_t *>(smem);
    } else {
        ch = reinterpret_cast<R *>(smem);
        alpha = ch + NL;
        blw = reinterpret_cast<uint32_t *>(alpha + (size_t)L * NL);
    }
    uint32_t *curw = blw + (size_t)L * NWL;
    R *cand = reinterpret_cast<R *>(curw + (size_t)L * NWL);
    // table-driven staircase (polar_lut.h): same bits as polar_math.h's chk / phi, a third of the instructions
    unsigned char *lut_mem = reinterpret_cast<unsigned char *>(cand + 2 * L);
    // DYN: hist[L][NW] behind cand (L * NW may be odd, cand holds doubles) and the tables behind hist
    uint32_t *hist = reinterpret_cast<uint32_t *>(cand + 2 * L);
    if constexpr (DYN) lut_mem = reinterpret_cast<unsigned char *>(hist + (size_t)L * NWL);
    lut_mem += (16 - (reinterpret_cast<uintptr_t>(lut_mem) & 15)) & 15;
    Lut<R>::build(lut_mem, lane, 64);
    Lut<R> lut;
    lut.bind(lut_mem);
    __syncthreads();
    auto ld = [](const R *q) -> R {
        if constexpr (GA) return ld_bypass(q);
        else return *q;
    };

    for (int frame = blockIdx.x; frame < P.B; frame = next_job_wave(P.queue, frame, (int)gridDim.x, P.B)) {   // one wavefront per workgroup
        // ---- the frame's code: the launch's, or in a code book the member its index names ----
        int N = NL, n = P.n, NW = NWL, sc_mode = P.sc_mode;
        const uint32_t *fmask = P.frozen, *crc_tab = P.crc_tab;
        size_t ld_in = (size_t)NL;
        BookCode bc{};
        if constexpr (BOOK) {
            // the index comes from device memory: it is compared with C before any address is formed from it
            const uint32_t code = (uint32_t)__builtin_amdgcn_readfirstlane((int)BK->code[frame]);
            if (code >= BK->C) {
                if constexpr (LIST) {
                    if (LO->paths)
                        for (int w = lane; w < L * NWL; w += 64) LO->paths[(size_t)frame * L * NWL + w] = 0u;
                    if (lane < L) {
                        if (LO->pm) LO->pm[(size_t)frame * L + lane] = __builtin_huge_val();
                        if (LO->rem) LO->rem[(size_t)frame * L + lane] = 0u;
                    }
                    if (lane == 0 && LO->count) LO->count[frame] = 0u;
                } else {
                    if (P.out_bits)
                        for (int w = lane; w < NWL; w += 64) P.out_bits[(size_t)frame * NWL + w] = 0u;
                    if (lane == 0 && P.pm) P.pm[frame] = __builtin_huge_val();
                }
                if (lane == 0 && P.flags) P.flags[frame] = BOOK_FLAG_NO_CODE;
                continue;
            }
            bc = book_code(BK->codes, code);
            N = bc.N, n = bc.n, NW = N >> 5, sc_mode = bc.sc_mode;
            fmask = bc.frozen, crc_tab = bc.crc_tab;
            dyn_mask = bc.dyn_mask, dyn_row = bc.dyn_row;
            ld_in = BK->ld;
        }
        // ---- channel LLRs (SCL_1024.c:574-578) ----
        {
            const IN *src = reinterpret_cast<const IN *>(P.in) + (size_t)frame * ld_in;
            if (BOOK && bc.rm_mode != BOOK_RM_NONE) book_rm_load<R, IN>(ch, src, bc, P.sigma, lane);
            else
                for (int i = lane; i < N; i += 64) ch[i] = (R)channel_llr<IN>(src, i, P.sigma);
        }
        if constexpr (DYN)
            for (int w = lane; w < L * NW; w += 64) hist[w] = 0u;
        __syncthreads();

        R PM = R(0);
        uint64_t ptrA = 0;
        uint32_t crc = 0, bl0 = 0, cur0 = 0;
        uint32_t h0 = 0;   // DYN: word 0 of the path's history, shuffled with the path like bl0
        uint32_t fl = 0;
        int act = 1;
        // TRACE: slot 0 has decided nothing yet and matches; the sent word of the 32 leaves at hand; the loss leaf and its count
        bool match = TRACE && p == 0;
        uint32_t sent_w = 0, loss_rank = 0;
        int loss_leaf = N;

        for (int j = 0; j < N; ++j) {
            if constexpr (TRACE)
                if ((j & 31) == 0) sent_w = TO->u[(size_t)frame * NW + (j >> 5)];
            // ================= LLR of leaf j for every active path =================
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
            const bool frozen = (fmask[j >> 5] >> (j & 31)) & 1;
            int row = -1;   // DYN: row of leaf j in the constraint matrix, -1 = not dynamic (wave-uniform, like j)
            if constexpr (DYN) row = dyn_row[j];
            int bit = 0;
            uint32_t sent_n = 0;   // TRACE: at a ranking leaf the count of the sent candidate, taken before the pruning
            if (row >= 0) {
                // dynamic frozen leaf: b = parity of (history AND mask row) over the words 0 .. j >> 5, on every lane of the
                // wave (lanes of dead paths compute and discard); no fork, no ranking, no tie flag
                if constexpr (DYN) {
                    const uint32_t *mrow = dyn_mask + (size_t)row * NW;
                    uint32_t par = 0;
                    for (int w = pos; w <= (j >> 5); w += S) {
                        const uint32_t hw = (w == 0) ? h0 : hist[p * NW + w];
                        par ^= (uint32_t)__popc(hw & mrow[w]);
                    }
                    for (int o = S >> 1; o > 0; o >>= 1) par ^= (uint32_t)__shfl_xor((int)par, o);
                    bit = (int)(par & 1u);
                    // PHI(., b) with the rounding of an information leaf's branch b
                    if (!sc_mode && p < act) PM = PM + (lut.tabv(lam) + (bit ? posmax(lam) : negmax(lam)));
                }
            } else if (sc_mode) {
                bit = (!frozen && lam < R(0)) ? 1 : 0;  // SC_128.c:426-431
            } else if (frozen) {
                if (p < act) PM += lut.tabv(lam) + negmax(lam);  // PHI(.,0), SCL_1024.c:601-604, :662-665
            } else if (act < L) {
                // phase 1: every path forks, clone k -> k + act (SCL_1024.c:586-600)
                const bool is_new = (p >= act) && (p < 2 * act);
                const int sg = is_new ? p - act : p;
                const int sl = sg * S + pos;
                const R lam_s = __shfl(lam, sl);
                const R pm_s = __shfl(PM, sl);
                ptrA = __shfl(ptrA, sl);
                crc = __shfl(crc, sl);
                bl0 = __shfl(bl0, sl);
                if constexpr (DYN) h0 = __shfl(h0, sl);
                if constexpr (TRACE) match = __shfl((int)match, sl) != 0;
                if (is_new) {
                    for (int w = 1 + pos; w < NW; w += S) {
                        blw[p * NW + w] = blw[sg * NW + w];
                        if constexpr (DYN) hist[p * NW + w] = hist[sg * NW + w];
                    }
                    bit = 1;
                    PM = pm_s + (lut.tabv(lam_s) + posmax(lam_s));
                } else if (p < act) {
                    PM = PM + (lut.tabv(lam) + negmax(lam));
                }
                act *= 2;
                __syncthreads();
            } else {
                // phase 2: keep the L best of 2L candidates (SCL_1024.c:610-661)
                const R tt = lut.tabv(lam);
                const R c0 = PM + (tt + negmax(lam));
                const R c1 = PM + (tt + posmax(lam));
                if (pos == 0) {
                    cand[p] = c0;
                    cand[p + L] = c1;
                }
                __syncthreads();
                // strict "< med" with med = (L+1)-th smallest  <=>  #{m : c_m <= c} <= L
                int n0 = 0, n1 = 0;
                for (int m = 0; m < 2 * L; ++m) {
                    const R v = cand[m];
                    n0 += (v <= c0);
                    n1 += (v <= c1);
                }
                const bool s0 = n0 <= L, s1 = n1 <= L;
                if constexpr (TRACE) {
                    // the slot that matched after leaf j - 1 (at most one does): its count for the sent bit
                    const uint64_t m_match = __ballot(match);
                    const int n_sent = trace_sent_bit(sent_w, j) ? n1 : n0;
                    const int n_first = __shfl(n_sent, m_match ? __ffsll((unsigned long long)m_match) - 1 : 0);
                    sent_n = m_match ? (uint32_t)n_first : 0u;
                }
                const bool lead = pos == 0;
                const uint64_t m_s0 = __ballot(lead && s0);
                const uint64_t m_s1 = __ballot(lead && s1);
                const uint64_t m_both = m_s0 & m_s1;
                const uint64_t m_dead = __ballot(lead) & ~(m_s0 | m_s1);
                if (__popcll(m_s0) + __popcll(m_s1) < L) fl |= 0x1u;  // median tie ("Oops!", :621-622)
                const bool dead = !s0 && !s1;
                int sg = p;
                const bool refilled = fork_source<S>(m_both, m_dead, p, dead, sg);
                const int sl = sg * S + pos;
                const R c1_s = __shfl(c1, sl);
                ptrA = __shfl(ptrA, sl);
                crc = __shfl(crc, sl);
                bl0 = __shfl(bl0, sl);
                if constexpr (DYN) h0 = __shfl(h0, sl);
                if constexpr (TRACE) match = __shfl((int)match, sl) != 0;
                if (refilled) {
                    for (int w = 1 + pos; w < NW; w += S) {
                        blw[p * NW + w] = blw[sg * NW + w];
                        if constexpr (DYN) hist[p * NW + w] = hist[sg * NW + w];
                    }
                    bit = 1;
                    PM = c1_s;
                } else if (s0) {
                    bit = 0;  // class 0 or the staying half of class 2
                    PM = c0;
                } else if (s1) {
                    bit = 1;
                    PM = c1;
                } else {
                    bit = 0;  // tie rule: an un-refilled dead slot continues as its 0-branch
                    PM = c0;
                }
                __syncthreads();
            }

            // ================= TRACE: the match flag after the decision; the first leaf nobody matches after =================
            if constexpr (TRACE) {
                match = match && p < act && bit == trace_sent_bit(sent_w, j);
                const bool none = __ballot(match) == 0ull;
                if (none && loss_leaf == N) {
                    loss_leaf = j;
                    loss_rank = sent_n;
                }
            }

            // ================= DYN: bit j of the path's history =================
            if constexpr (DYN) {
                if (j < 32) {
                    h0 |= (uint32_t)bit << j;
                } else {
                    if (pos == 0 && p < act && bit) hist[p * NW + (j >> 5)] |= 1u << (j & 31);
                    __syncthreads();
                }
            }

            // ================= partial sums (updateBit, SCL_1024.c:424-448) =================
            if (crc_tab && bit) crc ^= crc_tab[j];
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

        // ================= choose the path (SCL_1024.c:667-674; CASCL_1024_L8.c:725-755) =================
        int best = 0;
        R best_pm = PM;
        if (!sc_mode) {
            const bool pass = (crc_tab != nullptr) && (crc == 0);
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
        // LIST: rank of this slot among the live ones in ascending (PM, slot), counted over the shuffled metrics; the S lanes
        // of a path write its history words to row `rank`, the lanes of a dead slot p the padding row p (>= act)
        if constexpr (LIST) {
            int rank = 0;
            for (int q = 0; q < act; ++q) {
                const R pq = __shfl(PM, q * S);
                rank += (pq < PM || (pq == PM && q < p)) ? 1 : 0;
            }
            const bool live = p < act;
            const size_t row = (size_t)frame * L + (size_t)(live ? rank : p);
            if constexpr (BOOK) {
                if (LO->paths)
                    for (int w = pos; w < NWL; w += S)
                        LO->paths[row * NWL + w] = (!live || w >= NW) ? 0u : (w == 0) ? h0 : hist[p * NW + w];
            } else if (LO->paths)
                for (int w = pos; w < NW; w += S) LO->paths[row * NW + w] = !live ? 0u : (w == 0) ? h0 : hist[p * NW + w];
            if (pos == 0) {
                if (LO->pm) LO->pm[row] = live ? (double)PM : __builtin_huge_val();
                if (LO->rem) LO->rem[row] = live ? crc : 0u;
            }
            if (lane == 0 && LO->count) LO->count[frame] = (uint32_t)act;
        }
        // TRACE: the rank of the LIST epilogue, read from the matching slot (at most one) and from the chosen one
        else if constexpr (TRACE) {
            int rank = 0;
            for (int q = 0; q < act; ++q) {
                const R pq = __shfl(PM, q * S);
                rank += (pq < PM || (pq == PM && q < p)) ? 1 : 0;
            }
            const uint64_t m_match = __ballot(match);
            const int r_first = __shfl(rank, m_match ? __ffsll((unsigned long long)m_match) - 1 : 0);
            const int r_best = __shfl(rank, best * S);
            if (lane == 0) trace_write(*TO, frame, loss_leaf, loss_rank, m_match ? r_first : -1, r_best);
        }
        // x_hat of the chosen path: root partial sums; u_hat = x_hat * F^{(x)n}.  DYN: u_hat is the chosen path's history
        else if constexpr (DYN) {
            const uint32_t w0 = __shfl(h0, best * S);
            if (!BOOK || P.out_bits)
                for (int w = lane; w < NWL; w += 64)
                    P.out_bits[(size_t)frame * NWL + w] = (BOOK && w >= NW) ? 0u : (w == 0) ? w0 : hist[best * NW + w];
        } else if (n <= 5) {
            const uint32_t x = polar_word_transform_n(__shfl(cur0, best * S), n);
            if (lane == 0) P.out_bits[(size_t)frame * NW] = x;
        } else {
            uhat_from_rows(curw + (size_t)best * NW, NW, n, lane, P.out_bits + (size_t)frame * NW);
        }
        if (lane == 0) {
            if (!LIST && P.pm) P.pm[frame] = sc_mode ? 0.0 : (double)best_pm;
            if (P.flags) P.flags[frame] = sc_mode ? 0u : fl;
        }
        __syncthreads();
    }
}

template <typename R, typename IN, int LOGL, bool GA>
__global__ __launch_bounds__(64) void k_scl_generic(SclParams P)
{
    scl_generic_body<R, IN, LOGL, GA, false>(P, nullptr, nullptr);
}

template <typename R, int LOGL>
constexpr size_t scl_generic_lds_bytes(int N, bool ga)
{
    return (ga ? 0 : sizeof(R) * (size_t)N * (1 + (1 << LOGL))) + 2 * sizeof(uint32_t) * (size_t)(N / 32) * (1 << LOGL) +
           sizeof(R) * 2 * (1 << LOGL) + 16 + Lut<R>::bytes;
}

}  // namespace polar
