// scl_wide.h -- SCL / CA-SCL with a wide list, L = 2^LOGL in {64, 128, 256}, plain or with dynamic frozen bits.
//
// The rule is scl_generic.h's (and scl_dyn.h's for DYN), word for word: phase 1 clones slot k into slot k + act, phase 2
// keeps the candidates c with #{m : c_m <= c} <= L, the m-th both-survivor (ascending slot) forks into the m-th dead slot,
// an un-refilled dead slot continues as its 0-branch, the tie flag is set iff fewer than L candidates survive at some leaf,
// a dynamic frozen leaf takes the parity of (history AND mask row) and adds PHI(lambda, b), and the output is the first slot
// of least metric among the live slots that pass the CRC (among all live slots if none passes or there is no CRC).  The
// arithmetic is chk_lut / lut.tabv / gfun in the same operation order, so the results equal scl_generic_body's bit for bit
// wherever both exist, and the CPU model's (tests/test_dyn_host.py dscl_model) everywhere.
// "Everywhere" includes the frames with a median tie: tests/test_gpu_wide.py holds that at L = 64 (one wavefront, N = 32 on
// a grid), tests/test_gpu_wide_families.py at L = 128 and 256 (2 and 4 wavefronts) on tied and degenerate rows, frozen sets
// outside the 5G order and dense constraint sets, where dead slots stay un-refilled, refills cross wavefronts and leaves
// have all 2L candidates equal (tests/test_wide_families_host.py asserts that the cases do).
//
// What differs is the mapping.  scl_generic_body gives a path S = 64 / L lanes of one wavefront and moves state between paths
// with __shfl / __ballot; that stops at 64 lanes.  Here one codeword has a workgroup of L threads (1, 2 or 4 wavefronts),
// one thread per path, and everything that crosses paths goes through LDS:
//
//     ch[N]                    channel LLRs (level n)
//     alpha[N][L]              level t of slot s: elements (2^t + e) * L + s -- scl_generic.h's alpha[L][N] transposed, so
//                              that the L threads writing element e of their own slots touch L consecutive words (no LDS
//                              bank conflicts; coalesced stores in the global-scratch variant)
//     blw / curw / hist [N/32][L]   bit-packed (polar_bits.h), transposed the same way; word 0 of blw and hist lives in
//                              registers (bl0, h0), cur0 is the working word below level 5
//     cand[2L]                 candidate metrics of a forking leaf: [p] = 0-branch, [L + p] = 1-branch of slot p
//     xptr / xcrc / xbl0 / xh0 [L]   the state that moves with a path, written by its owner before a fork, indexed by source slot
//     blist[L], wcnt[4][4]     per wavefront: the slots of its both-survivors in ascending order, and its counts
//
// SclParams::sc_mode is not read: SC has L = 1 and never comes here.
// GA = true: ch and alpha live in the workgroup's slice of the global scratch ((L + 1) * N values), read with ld_bypass.
//
// Each thread walks the whole level row of its path: at leaf j it reads level d + 1 (d = ctz j) through its pointer table and
// rewrites levels d .. 0 of its OWN slot, reading back only what it has just written.  Across threads the only reads are of
// level d + 1, which nobody writes at this leaf, so the level steps of one leaf need no barrier between them; one workgroup
// barrier after the LLR phase of every leaf keeps leaf j's reads ahead of leaf j + 1's writes (in the global variant every
// wavefront first waits for its own stores, wide_level_barrier()).  The partial-sum updates touch the thread's own words only.  A
// forking leaf adds three barriers: after the candidates and the exchange arrays are written, after the survivor classes
// are written, and after the refilled slots have copied their words.
//
// Every __syncthreads() and every __ballot sits in control flow that is uniform for the workgroup: the conditions around
// them are functions of j, the frozen mask, the constraint row and act only, never of the path.
//
// Against scl_wave_ops.h: the word-0 steps and the in-word transform are polar_bits.h's, as there.  The steps over rows stay
// here: a row is indexed [w * L + p], its one thread walks all of its words, and the partial-sum update has no barrier
// inside (scl_wave_ops.h's has S lanes per row and two), the fork pairing and the path choice go through LDS, not __shfl.
#pragma once
#include <type_traits>

#include "scl_dyn.h"

namespace polar {

// LDS carve-up, the same arithmetic on the host (launch) and in the kernel
template <typename R, int LOGL, bool DYN>
struct WideLds {
    static constexpr int L = 1 << LOGL;
    static constexpr int MISC_WORDS = 32;   // wcnt[4][4], the job slot, padding
    static constexpr size_t r_elems(int N, bool ga) { return (ga ? 0 : (size_t)N * (L + 1)) + 2 * L; }
    static constexpr size_t bit_words(int N) { return (size_t)(DYN ? 3 : 2) * (N / 32) * L; }
    static constexpr size_t bytes(int N, bool ga)
    {
        return sizeof(R) * r_elems(N, ga) + sizeof(uint64_t) * L + sizeof(uint32_t) * (bit_words(N) + 4 * L + MISC_WORDS) + 16 +
               Lut<R>::bytes;
    }
};

// The barrier behind a step that wrote ch / alpha.  GA: the rows pass from wavefront to wavefront through global memory and
// are read around the L1 (ld_bypass), so every wavefront first waits until its own stores have completed (vmcnt(0); the
// fence keeps the compiler from moving a store below the wait).
template <bool GA>
__device__ __forceinline__ void wide_level_barrier()
{
    if constexpr (GA) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0); expcnt and lgkmcnt left alone
    }
    __syncthreads();
}

// LIST = true (needs DYN; launched by k_list.hip): the kernel takes a ListParams, the decode is the same, and the epilogue
// writes every live slot to its ListOut in ascending (PM, slot) instead of the chosen path.
struct ListParams {
    DynParams d;
    ListOut o;
};

// TRACE = true (needs DYN, not with LIST; launched by k_trace.hip): the kernel takes a TraceParams, the decode is the same,
// every thread carries the match flag of trace_out.h for its slot, and the epilogue writes the frame's five trace words to its
// TraceOut instead of the chosen path.  At most one slot matches, so the flag crosses threads as a slot number: at an
// information leaf every wavefront ballots its flags and writes the matching slot (or -1) to its word wtr[wave] before the leaf's first barrier, every thread
// reads the words behind it, and the thread whose path comes from that slot with the sent bit matches afterwards.  The thread
// that matched knows from its own s0 / s1 / refill whether the sent candidate goes on, and keeps the loss leaf and the count;
// the epilogue collects them through four more words.  All eight words lie in MISC_WORDS.  The ballot sits in control flow
// that is uniform for the workgroup; the lanes choose what they contribute with ?:.
struct TraceParams {
    DynParams d;
    TraceOut t;
};
__device__ __forceinline__ const DynParams &wide_dyn(const DynParams &P) { return P; }
__device__ __forceinline__ const DynParams &wide_dyn(const ListParams &P) { return P.d; }
__device__ __forceinline__ const DynParams &wide_dyn(const TraceParams &P) { return P.d; }

template <typename R, typename IN, int LOGL, bool GA, bool DYN, bool LIST = false, bool TRACE = false>
__global__ __launch_bounds__(1 << LOGL) void k_scl_wide(
    typename std::conditional<TRACE, TraceParams, typename std::conditional<LIST, ListParams, DynParams>::type>::type KP)
{
    const DynParams &DP = wide_dyn(KP);
    static_assert(LOGL >= 6 && LOGL <= 8, "one thread per path: 1, 2 or 4 wavefronts");
    static_assert(DYN || !LIST, "the list epilogue reads the per-path history");
    static_assert(!TRACE || (DYN && !LIST), "the trace runs the list decode and has its own epilogue");
    constexpr int L = 1 << LOGL;
    constexpr int NWAVES = L / 64;
    using Lay = WideLds<R, LOGL, DYN>;
    const SclParams &P = DP.s;
    const int N = P.N, n = P.n, NW = N >> 5;
    const int p = threadIdx.x;
    const int wave = p >> 6, wlane = p & 63;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    R *ch, *alpha, *cand;
    if constexpr (GA) {
        ch = reinterpret_cast<R *>(P.scratch) + (size_t)blockIdx.x * (size_t)(L + 1) * N;
        alpha = ch + N;
        cand = reinterpret_cast<R *>(smem);
    } else {
        ch = reinterpret_cast<R *>(smem);
        alpha = ch + N;
        cand = alpha + (size_t)N * L;
    }
    uint64_t *xptr = reinterpret_cast<uint64_t *>(cand + 2 * L);
    uint32_t *blw = reinterpret_cast<uint32_t *>(xptr + L);
    uint32_t *curw = blw + (size_t)NW * L;
    uint32_t *hist = curw + (size_t)NW * L;   // DYN only
    uint32_t *xcrc = hist + (DYN ? (size_t)NW * L : 0);
    uint32_t *xbl0 = xcrc + L;
    uint32_t *xh0 = xbl0 + L;
    int *blist = reinterpret_cast<int *>(xh0 + L);
    int *wcnt = blist + L;               // [NWAVES][4]: both-survivors, dead slots, surviving candidates
    int *job_slot = wcnt + 16;
    int *wtr = wcnt + 20;                // TRACE: [NWAVES] the matching slot of each wavefront, -1 if it has none
    int *wout = wcnt + 24;               // TRACE: loss leaf, its count, rank of the sent word, rank of the chosen path
    unsigned char *lut_mem = reinterpret_cast<unsigned char *>(wcnt + Lay::MISC_WORDS);
    lut_mem += (16 - (reinterpret_cast<uintptr_t>(lut_mem) & 15)) & 15;
    Lut<R>::build(lut_mem, p, L);
    Lut<R> lut;
    lut.bind(lut_mem);
    __syncthreads();
    auto ld = [](const R *q) -> R {
        if constexpr (GA) return ld_bypass(q);
        else return *q;
    };

    for (int frame = blockIdx.x; frame < P.B; frame = next_job_block(P.queue, frame, (int)gridDim.x, P.B, job_slot)) {
        // ---- channel LLRs (SCL_1024.c:574-578) ----
        {
            const IN *src = reinterpret_cast<const IN *>(P.in) + (size_t)frame * N;
            for (int i = p; i < N; i += L) ch[i] = (R)channel_llr<IN>(src, i, P.sigma);
        }
        if constexpr (DYN)
            for (int w = 1; w < NW; ++w) hist[w * L + p] = 0u;
        wide_level_barrier<GA>();

        R PM = R(0);
        uint64_t ptrA = 0;
        uint32_t crc = 0, bl0 = 0, cur0 = 0;
        uint32_t h0 = 0;
        uint32_t fl = 0;
        int act = 1;
        // TRACE: slot 0 has decided nothing yet and matches; the sent word of the 32 leaves at hand; the loss leaf and its count
        bool match = TRACE && p == 0;
        uint32_t sent_w = 0, loss_rank = 0;
        int loss_leaf = N;

        for (int j = 0; j < N; ++j) {
            if constexpr (TRACE)
                if ((j & 31) == 0) sent_w = KP.t.u[(size_t)frame * NW + (j >> 5)];
            // ================= LLR of leaf j for every active path: the path's thread walks every level =================
            R lam = R(0);
            if (p < act) {
                int tf = n - 1;
                if (j > 0) {
                    const int d = __builtin_ctz((unsigned)j);
                    const int h = 1 << d;
                    const bool top = d + 1 == n;
                    const R *src = top ? ch : alpha + (size_t)(2 << d) * L + ptr_get<LOGL>(ptrA, top ? 0 : d + 1);
                    const int st = top ? 1 : L;
                    R *out = alpha + (size_t)h * L + p;
                    for (int e = 0; e < h; ++e) {
                        const int bi = h + e;
                        const uint32_t wv = (bi < 32) ? bl0 : blw[(bi >> 5) * L + p];
                        lam = gfun<R>(ld(src + (size_t)e * st), ld(src + (size_t)(e + h) * st), (wv >> (bi & 31)) & 1);
                        out[(size_t)e * L] = lam;
                    }
                    ptrA = ptr_set<LOGL>(ptrA, d, p);
                    tf = d - 1;
                }
                for (int t = tf; t >= 0; --t) {
                    const int h = 1 << t;
                    const bool top = t + 1 == n;
                    const R *src = top ? ch : alpha + (size_t)(2 << t) * L + ptr_get<LOGL>(ptrA, top ? 0 : t + 1);
                    const int st = top ? 1 : L;
                    R *out = alpha + (size_t)h * L + p;
                    for (int e = 0; e < h; ++e) {
                        lam = chk_lut<R>(ld(src + (size_t)e * st), ld(src + (size_t)(e + h) * st), lut);
                        out[(size_t)e * L] = lam;
                    }
                    ptrA = ptr_set<LOGL>(ptrA, t, p);
                }
            }
            wide_level_barrier<GA>();   // leaf j's reads of other slots' rows before leaf j + 1's writes

            // ================= decision =================
            const bool frozen = (P.frozen[j >> 5] >> (j & 31)) & 1;
            int row = -1;   // DYN: row of leaf j in the constraint matrix, -1 = not dynamic (uniform, like j)
            if constexpr (DYN) row = DP.row[j];
            int bit = 0;
            bool forked = false;     // TRACE: an information leaf, where paths move between slots
            bool sent_on = true;     // TRACE, on the thread that matches: the sent candidate goes on after this leaf's pruning
            uint32_t sent_n = 0;     // TRACE: at a ranking leaf the count of this thread's candidate with the sent bit
            bool from_match = match; // TRACE: the slot this thread's path comes from matched after leaf j - 1
            if (row >= 0) {
                // dynamic frozen leaf: b = parity of (history AND mask row) over the words 0 .. j >> 5; no fork, no ranking
                if constexpr (DYN) {
                    const uint32_t *mrow = DP.mask + (size_t)row * NW;
                    uint32_t par = 0;
                    for (int w = 0; w <= (j >> 5); ++w) {
                        const uint32_t hw = (w == 0) ? h0 : hist[w * L + p];
                        par ^= (uint32_t)__popc(hw & mrow[w]);
                    }
                    bit = (int)(par & 1u);
                    if (p < act) PM = PM + (lut.tabv(lam) + (bit ? posmax(lam) : negmax(lam)));
                }
            } else if (frozen) {
                if (p < act) PM += lut.tabv(lam) + negmax(lam);  // PHI(.,0), SCL_1024.c:601-604, :662-665
            } else {
                // an information leaf: every path offers its two branches
                const R tt = lut.tabv(lam);
                const R c0 = PM + (tt + negmax(lam));
                const R c1 = PM + (tt + posmax(lam));
                cand[p] = c0;
                cand[p + L] = c1;
                xptr[p] = ptrA;
                xcrc[p] = crc;
                xbl0[p] = bl0;
                if constexpr (DYN) xh0[p] = h0;
                if constexpr (TRACE) {
                    const uint64_t m_match = __ballot(match);
                    if (wlane == 0) wtr[wave] = m_match ? wave * 64 + __ffsll((unsigned long long)m_match) - 1 : -1;
                }
                __syncthreads();
                int m_slot = -1;      // TRACE: the slot that matched after leaf j - 1
                if constexpr (TRACE) {
                    forked = true;
                    for (int w = 0; w < NWAVES; ++w) m_slot = max(m_slot, wtr[w]);
                }
                int sg = p;           // the slot this thread's path comes from
                bool moved = false;   // it takes the 1-branch of slot sg
                if (act < L) {
                    // phase 1: every path forks, clone k -> k + act (SCL_1024.c:586-600)
                    moved = (p >= act) && (p < 2 * act);
                    if (moved) sg = p - act;
                    if (p < act) PM = c0;
                    act *= 2;
                } else {
                    // phase 2: keep the L best of 2L candidates (SCL_1024.c:610-661)
                    // strict "< med" with med = (L+1)-th smallest  <=>  #{m : c_m <= c} <= L
                    int n0 = 0, n1 = 0;
                    for (int m = 0; m < 2 * L; ++m) {
                        const R v = cand[m];
                        n0 += (v <= c0);
                        n1 += (v <= c1);
                    }
                    const bool s0 = n0 <= L, s1 = n1 <= L;
                    const bool both = s0 && s1, dead = !s0 && !s1;
                    const uint64_t m_s0 = __ballot(s0), m_s1 = __ballot(s1);
                    const uint64_t m_both = m_s0 & m_s1, m_dead = ~(m_s0 | m_s1);
                    const uint64_t below = (1ull << wlane) - 1ull;
                    if (both) blist[wave * 64 + __popcll(m_both & below)] = p;   // this wavefront's both-survivors, ascending
                    if (wlane == 0) {
                        wcnt[wave * 4 + 0] = __popcll(m_both);
                        wcnt[wave * 4 + 1] = __popcll(m_dead);
                        wcnt[wave * 4 + 2] = __popcll(m_s0) + __popcll(m_s1);
                    }
                    __syncthreads();
                    int n_both = 0, n_surv = 0, rank = __popcll(m_dead & below);   // rank: this slot among the dead ones
                    for (int w = 0; w < NWAVES; ++w) {
                        n_both += wcnt[w * 4 + 0];
                        n_surv += wcnt[w * 4 + 2];
                        if (w < wave) rank += wcnt[w * 4 + 1];
                    }
                    if (n_surv < L) fl |= 0x1u;  // median tie ("Oops!", :621-622)
                    // m-th both-survivor (ascending slot) forks into the m-th dead slot (:636-661)
                    if (dead && rank < n_both) {
                        int r = rank;
                        for (int w = 0; w < NWAVES; ++w) {
                            const int c = wcnt[w * 4 + 0];
                            if (r >= 0 && r < c) sg = blist[w * 64 + r];
                            r -= c;   // negative once found
                        }
                        moved = true;
                    } else if (s0) {
                        PM = c0;  // class 0 or the staying half of class 2
                    } else if (s1) {
                        bit = 1;
                        PM = c1;
                    } else {
                        PM = c0;  // tie rule: an un-refilled dead slot continues as its 0-branch
                    }
                    if constexpr (TRACE) {
                        // the 1-branch goes on iff it survives (in place, or as a both-survivor's fork: there are never more
                        // both-survivors than dead slots); the 0-branch iff it survives or the slot stays dead and un-refilled
                        const bool sent1 = trace_sent_bit(sent_w, j) != 0;
                        sent_on = sent1 ? s1 : (s0 || (dead && !moved));
                        sent_n = (uint32_t)(sent1 ? n1 : n0);
                    }
                }
                if constexpr (TRACE) from_match = sg == m_slot;
                if (moved) {
                    bit = 1;
                    PM = cand[sg + L];
                    ptrA = xptr[sg];
                    crc = xcrc[sg];
                    bl0 = xbl0[sg];
                    if constexpr (DYN) h0 = xh0[sg];
                    for (int w = 1; w < NW; ++w) {
                        blw[w * L + p] = blw[w * L + sg];
                        if constexpr (DYN) hist[w * L + p] = hist[w * L + sg];
                    }
                }
                __syncthreads();   // the copies read their sources before the owners go on
            }

            // ================= TRACE: the match flag after the decision; the leaf the sent path is lost at =================
            if constexpr (TRACE) {
                const int sent = trace_sent_bit(sent_w, j);
                if (match && (forked ? !sent_on : bit != sent)) {   // at most one thread, at most once per frame
                    loss_leaf = j;
                    loss_rank = sent_n;
                }
                match = from_match && p < act && bit == sent;
            }

            // ================= DYN: bit j of the path's history (the thread's own words) =================
            if constexpr (DYN) {
                if (j < 32) h0 |= (uint32_t)bit << j;
                else if (p < act && bit) hist[(j >> 5) * L + p] |= 1u << (j & 31);
            }

            // ================= partial sums (updateBit, SCL_1024.c:424-448), the thread's own words =================
            if (P.crc_tab && bit) crc ^= P.crc_tab[j];
            cur0 = (uint32_t)bit;
            int t = 0;
            while (t < n && ((j >> t) & 1)) {
                if (t < 5) {
                    cur0 = ps_fold0(bl0, cur0, t);
                } else if (p < act) {
                    const int nw = 1 << (t - 5);
                    if (t == 5) curw[p] = cur0;
                    for (int w = 0; w < nw; ++w) {
                        const uint32_t c = curw[w * L + p];
                        const uint32_t l = blw[(nw + w) * L + p];
                        curw[w * L + p] = l ^ c;
                        curw[(w + nw) * L + p] = c;
                    }
                }
                ++t;
            }
            if (t < n) {
                if (t < 5) {
                    bl0 = ps_save0(bl0, cur0, t);
                } else if (p < act) {
                    const int nw = 1 << (t - 5);
                    if (t == 5) blw[L + p] = cur0;
                    else
                        for (int w = 0; w < nw; ++w) blw[(nw + w) * L + p] = curw[w * L + p];
                }
            }
        }

        // ================= choose the path (SCL_1024.c:667-674; CASCL_1024_L8.c:725-755) =================
        // the first slot of least metric among the live slots that pass the CRC; among all live slots if none does
        cand[p] = PM;
        xcrc[p] = (P.crc_tab != nullptr && crc == 0) ? 1u : 0u;
        xbl0[p] = cur0;
        if constexpr (DYN) xh0[p] = h0;
        __syncthreads();
        int best = -1, best_ok = -1;
        R best_pm = R(0), best_ok_pm = R(0);
        for (int q = 0; q < act; ++q) {
            const R pq = cand[q];
            if (best < 0 || pq < best_pm) {
                best = q;
                best_pm = pq;
            }
            if (xcrc[q] && (best_ok < 0 || pq < best_ok_pm)) {
                best_ok = q;
                best_ok_pm = pq;
            }
        }
        if (best_ok >= 0) {
            best = best_ok;
            best_pm = best_ok_pm;
            fl |= 0x2u;
        }
        // LIST: rank of this slot among the live ones in ascending (PM, slot), counted over the metrics in cand[]; the path's
        // thread writes its history words to row `rank`, the thread of a dead slot p the padding row p (>= act)
        if constexpr (LIST) {
            const ListOut *LO = &KP.o;
            int rank = 0;
            for (int q = 0; q < act; ++q) {
                const R pq = cand[q];
                rank += (pq < PM || (pq == PM && q < p)) ? 1 : 0;
            }
            const bool live = p < act;
            const size_t row = (size_t)frame * L + (size_t)(live ? rank : p);
            if (LO->paths)
                for (int w = 0; w < NW; ++w) LO->paths[row * NW + w] = !live ? 0u : (w == 0) ? h0 : hist[w * L + p];
            if (LO->pm) LO->pm[row] = live ? (double)PM : __builtin_huge_val();
            if (LO->rem) LO->rem[row] = live ? crc : 0u;
            if (p == 0 && LO->count) LO->count[frame] = (uint32_t)act;
        }
        // TRACE: the rank of the LIST epilogue, taken from the matching thread (at most one) and from the chosen one; the
        // thread that saw the loss hands over its leaf and count
        else if constexpr (TRACE) {
            const TraceOut *TO = &KP.t;
            int rank = 0;
            for (int q = 0; q < act; ++q) {
                const R pq = cand[q];
                rank += (pq < PM || (pq == PM && q < p)) ? 1 : 0;
            }
            if (p == 0) {
                wout[0] = N;
                wout[1] = 0;
                wout[2] = -1;
            }
            __syncthreads();
            if (loss_leaf < N) {
                wout[0] = loss_leaf;
                wout[1] = (int)loss_rank;
            }
            if (match) wout[2] = rank;
            if (p == best) wout[3] = rank;
            __syncthreads();
            if (p == 0) trace_write(*TO, frame, wout[0], (uint32_t)wout[1], wout[2], wout[3]);
        }
        // x_hat of the chosen path: root partial sums; u_hat = x_hat * F^{(x)n}.  DYN: u_hat is the chosen path's history
        else if constexpr (DYN) {
            if (p < NW) P.out_bits[(size_t)frame * NW + p] = (p == 0) ? xh0[best] : hist[p * L + best];
        } else if (n <= 5) {
            if (p == 0) P.out_bits[(size_t)frame * NW] = polar_word_transform_n(xbl0[best], n);
        } else {
            uint32_t *xw = curw + best;   // word w at xw[w * L]
            if (p < NW) xw[p * L] = polar_word_transform(xw[p * L]);
            __syncthreads();
            for (int s = 5; s < n; ++s) {
                const int hw = 1 << (s - 5);
                if (p < NW && !(p & hw)) xw[p * L] ^= xw[(p + hw) * L];
                __syncthreads();
            }
            if (p < NW) P.out_bits[(size_t)frame * NW + p] = xw[p * L];
        }
        if (p == 0) {
            if (!LIST && P.pm) P.pm[frame] = (double)best_pm;
            if (P.flags) P.flags[frame] = fl;
        }
        __syncthreads();
    }
}

}  // namespace polar
