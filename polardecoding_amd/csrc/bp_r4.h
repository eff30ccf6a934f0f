// bp_r4.h -- flooding BP for N = 1024 (reference: BP, BP_1024.c:372-427), register-blocked.
//
// k_bp (bp_kernel.h) keeps every message row in LDS: 152 KB in f64, one codeword per CU, eight waves of dependent LDS
// round trips (VALU 47 % / LDS pipe 46 % busy).  Here the ten stages are taken two at a time ("radix 4"): a thread owns the
// four elements e + {0, s, 2s, 3s}, s = 4^g, that are closed under stages 2g and 2g+1, so the row between the two stages
// of a group -- R[2g+1] in the right-going sweep, L[2g+1] in the left-going one -- is produced and consumed by the same
// thread and lives in its registers for the whole decode.  Only the rows that cross a group boundary (R[2], R[4], R[6],
// R[8], L[2], L[4], L[6], L[8]) go through LDS: 64 KB per codeword in f64 instead of 152 KB -> two codewords per CU, each
// thread with two independent butterflies in flight per stage, 2.7 message accesses per butterfly instead of 6, and no
// per-stage index arithmetic (the element sets are compile-time functions of the group).  The four L rows are read from
// LDS once per iteration and kept in the reader's registers for the next right-going sweep, so they share ONE transfer
// row: 40 KB per codeword, three f64 codewords per CU (BpR4Cfg below).
//
// Threads: 256 per codeword, t = 64 w + x.  Group g < 4 removes element bits 2g, 2g+1, which are below bit 8: wave w works
// on elements [256 w, 256 w + 256) in all of them, so groups 0..3 hand rows over inside one wave (LDS executes a wave's
// operations in order; a wave-level fence is enough).  Group 4 (stages 8, 9) takes elements x' + 256 k: the only
// workgroup barriers are around it, two per iteration.
//
// Same operations on the same operands in the same order as the reference, stage by stage (operand order inside CHK and
// inside the sums kept); r[n] and, except in the last iteration, l[0] are not computed (nobody reads them).
#pragma once
#include "polar_lut.h"
#include "bp_kernel.h"

namespace polar {

// CHK form: chk_lut1 (one round trip, 56 bytes of LDS per CHK).  The forms measured against it: chk_idx (prefix popcount +
// one conflict-free threshold read per look-up, 24 bytes), chk_lut (50-cell table, 40 bytes per CHK from scattered cells),
// chk_cnt (staircase counted with 14 subtractions, 8 bytes) and chk_tab (the prefix count of chk_idx read from a 26-byte
// table: three VALU instructions less per look-up, one more LDS read in the dependent chain -- 0.92 M against 1.19 M: slower).
// With the messages out of LDS the table reads of chk_lut kept the LDS pipe 68 % busy at 42 % VALU (0.90 M frames/s f64);
// chk_cnt is VALU-bound by its f64 subtractions (0.85 M).  Measured (2^16 frames, 50 iterations): f64 chk_idx 1.04 M
// frames/s, chk_lut 0.89 M; f32 chk_idx 1.57 M, chk_lut 1.81 M (a float entry of the 50-cell table is half the bytes), so
// round 2 took chk_idx for double and chk_lut for float.  Round 3, after the L rows moved into registers (three codewords per
// CU, 39 % LDS busy): chk_lut1 is ahead in both types -- f64 1.206 -> 1.303 M frames/s, f32 1.81 -> 2.09 M (same box, 2^16
// frames, 50 iterations, decisions hashed equal; profiles/r03_ab_experiments.txt run 22): five VALU instructions less per
// CHK than chk_idx, and the LDS pipe now has the room for its 48 bytes per CHK.
// The kernel still builds the chk_cnt and chk_idx tables (off_dn, off_st), which nothing reads.

template <typename R>
struct BpR4Cfg {
    static constexpr int N = 1024, n = 10, NW = 32, THREADS = 256;
    // The rows L[2], L[4], L[6], L[8] are read from LDS once per iteration (by the left-going sweep), kept in the
    // reader's registers (Lb) for the right-going sweep of the next iteration, and so only need ONE transfer row in LDS:
    // 40 KB per codeword instead of 64 KB -> three f64 codewords per CU, no LDS initialisation per frame.
    static constexpr int MIN_BLOCKS = 3;
    static constexpr size_t rows_bytes = sizeof(R) * (size_t)N * 5;   // R2 R4 R6 R8, then the one L transfer row
    static constexpr size_t off_lut = rows_bytes;
    static constexpr size_t off_dn = off_lut + ((Lut<R>::bytes + 15) / 16) * 16;
    static constexpr size_t off_st = off_dn + sizeof(R) * 64;
    static constexpr size_t lds_bytes = off_st + Stair<R>::bytes;
    // stop rule G: the 32 words of u_hat and the 32 of x_hat behind the tables
    static constexpr size_t off_stop = ((lds_bytes + 15) / 16) * 16;
    static constexpr size_t lds_bytes_stop = off_stop + 2 * sizeof(uint32_t) * NW;
};
// the stop rule must not cost the f64 kernel its third codeword per CU (160 KB of LDS, 16 bytes of static LDS each)
static_assert(3 * (BpR4Cfg<double>::lds_bytes_stop + 16) <= 160 * 1024, "k_bp_r4<double, double, true>: LDS of three codewords per CU");

template <typename R, typename IN>
struct BpR4 {
    using C = BpR4Cfg<R>;
    static constexpr int N = C::N;
    R Ri[5][4], Li[5][4];   // interior rows R[2g+1], L[2g+1] at this thread's elements of group g
    R Lb[4][4];             // L[2g+2] at this thread's elements of group g, as read by the last left-going sweep
    R ch[4];                // channel LLRs at the group-4 elements
    R *rowR, *rowL;         // LDS: rowR + (g-1) N = R[2g], g = 1..4; rowL: the L transfer row
    Lut<R> lut;
    int t;                  // thread index 0..255
    uint32_t fz;            // frozen flags of elements 4t .. 4t+3 (group 0)

    __device__ __forceinline__ R chk2(R a, R b) const
    {
        return chk_lut1<R>(a, b, lut);
    }
    // first element of this thread in group G: t with two zero bits inserted at position 2G
    template <int G>
    __device__ __forceinline__ int e0() const
    {
        constexpr int sh = 2 * G;
        return ((t >> sh) << (sh + 2)) | (t & ((1 << sh) - 1));
    }
    __device__ __forceinline__ R prior(int k) const { return ((fz >> k) & 1u) ? R(999) : R(0); }   // BP_1024.c:386-391

    // One butterfly of the right-going sweep (BP_1024.c:395-404): inputs r[i] and l[i+1] at (upper, lower) -> r[i+1]
    __device__ __forceinline__ void bfR(R r0, R r1, R l0, R l1, R &o0, R &o1) const
    {
        o0 = chk2(r0, l1 + r1);
        o1 = r1 + chk2(r0, l0);
    }
    // One butterfly of the left-going sweep (BP_1024.c:406-415): inputs l[i+1] and r[i] -> l[i]
    __device__ __forceinline__ void bfL(R l0, R l1, R r0, R r1, R &o0, R &o1) const
    {
        o0 = chk2(l0, l1 + r1);
        o1 = l1 + chk2(r0, l0);
    }

    // ---- right-going sweep, group G: stages 2G (pairs k, k+1) and 2G+1 (pairs k, k+2) ----
    template <int G>
    __device__ __forceinline__ void sweepR()
    {
        constexpr int s = 1 << (2 * G);
        const int e = e0<G>();
        R rin[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) rin[k] = (G == 0) ? prior(k) : rowR[(G - 1) * N + e + k * s];
        // stage 2G: r[2G], l[2G+1] -> r[2G+1]
        bfR(rin[0], rin[1], Li[G][0], Li[G][1], Ri[G][0], Ri[G][1]);
        bfR(rin[2], rin[3], Li[G][2], Li[G][3], Ri[G][2], Ri[G][3]);
        if constexpr (G < 4) {
            // stage 2G+1: r[2G+1], l[2G+2] -> r[2G+2]
            R lin[4], o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) lin[k] = Lb[G][k];
            bfR(Ri[G][0], Ri[G][2], lin[0], lin[2], o[0], o[2]);
            bfR(Ri[G][1], Ri[G][3], lin[1], lin[3], o[1], o[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k) rowR[G * N + e + k * s] = o[k];
        }
        // G == 4: stage 9 would only produce r[10], which nobody reads
    }
    // stop rule: sweepR<4> and stage 9, whose r[10] is not stored, only its hard decisions x_hat = (l[10] + r[10] >= 0) ? 0 : 1
    // at the elements t + 256 k (bit k of the result)
    __device__ __forceinline__ uint32_t sweepR4_xhat()
    {
        sweepR<4>();
        R o[4];
        bfR(Ri[4][0], Ri[4][2], ch[0], ch[2], o[0], o[2]);
        bfR(Ri[4][1], Ri[4][3], ch[1], ch[3], o[1], o[3]);
        uint32_t x = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (!(ch[k] + o[k] >= R(0))) x |= 1u << k;
        return x;
    }

    // ---- left-going sweep, group G: stages 2G+1 then 2G ----
    template <int G, bool LAST>
    __device__ __forceinline__ void sweepL(uint32_t &bits)
    {
        constexpr int s = 1 << (2 * G);
        const int e = e0<G>();
        R lin[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) lin[k] = (G == 4) ? ch[k] : rowL[e + k * s];
        if constexpr (G < 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) Lb[G][k] = lin[k];
        }
        // stage 2G+1: l[2G+2], r[2G+1] -> l[2G+1]
        bfL(lin[0], lin[2], Ri[G][0], Ri[G][2], Li[G][0], Li[G][2]);
        bfL(lin[1], lin[3], Ri[G][1], Ri[G][3], Li[G][1], Li[G][3]);
        if constexpr (G > 0) {
            // stage 2G: l[2G+1], r[2G] -> l[2G]
            R rin[4], o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) rin[k] = rowR[(G - 1) * N + e + k * s];
            bfL(Li[G][0], Li[G][1], rin[0], rin[1], o[0], o[1]);
            bfL(Li[G][2], Li[G][3], rin[2], rin[3], o[2], o[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k) rowL[e + k * s] = o[k];
        } else if constexpr (LAST) {
            // stage 0, needed only for the decision (BP_1024.c:417-425): frozen -> 0, else (l[0] + r[0] >= 0) -> 0
            R o[4];
            bfL(Li[0][0], Li[0][1], prior(0), prior(1), o[0], o[1]);
            bfL(Li[0][2], Li[0][3], prior(2), prior(3), o[2], o[3]);
            bits = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!((fz >> k) & 1u) && !(o[k] + prior(k) >= R(0))) bits |= 1u << k;
        }
    }
};

__device__ __forceinline__ void bp_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// decisions of elements 4t .. 4t+3 of this thread (bits 0..3) -> word t >> 3 of u_hat, valid in lanes with t & 7 == 0
__device__ __forceinline__ uint32_t bp_r4_pack(uint32_t bits, int t)
{
    uint32_t w = bits << (4 * (t & 7));
    w |= (uint32_t)__shfl_xor((int)w, 1);
    w |= (uint32_t)__shfl_xor((int)w, 2);
    w |= (uint32_t)__shfl_xor((int)w, 4);
    return w;
}

// STOP (stop rule G): stage 9 forms x_hat (ballots into 32 LDS words), l[0] is computed in every round trip, and after the
// left-going sweep every wave encodes the 32 words of u_hat and compares: the same LDS words give every wave the same answer,
// so the break is workgroup-uniform with one barrier more per round trip.
template <typename R, typename IN, bool STOP = false>
__global__ __launch_bounds__(256, (BpR4Cfg<R>::MIN_BLOCKS)) void k_bp_r4(BpParams P)
{
    using C = BpR4Cfg<R>;
    constexpr int N = C::N, NW = C::NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    BpR4<R, IN> s;
    s.t = threadIdx.x;
    s.rowR = reinterpret_cast<R *>(smem);
    s.rowL = s.rowR + 4 * N;
    Lut<R>::build(smem + C::off_lut, threadIdx.x, blockDim.x);
    s.lut.bind(smem + C::off_lut);
    build_delta_by_count<R>(reinterpret_cast<R *>(smem + C::off_dn), threadIdx.x, blockDim.x);
    Stair<R>::build(smem + C::off_st, threadIdx.x, blockDim.x);
    uint32_t *uw = reinterpret_cast<uint32_t *>(smem + C::off_stop);   // STOP: [32] u_hat, [32] x_hat
    uint32_t *xw = uw + NW;
    {
        const int e = 4 * s.t;
        s.fz = (P.frozen[e >> 5] >> (e & 31)) & 0xFu;
    }
    __syncthreads();

    __shared__ int job_slot;
    for (int frame = blockIdx.x; frame < P.B; frame = next_job_block(P.queue, frame, (int)gridDim.x, P.B, &job_slot)) {
        const IN *src = reinterpret_cast<const IN *>(P.in) + (size_t)frame * N;
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // group-4 elements t + 256 k: coalesced
            s.ch[k] = (R)channel_llr<IN>(src, s.t + 256 * k, P.sigma);   // BP_1024.c:381-382
        }
#pragma unroll
        for (int g = 0; g < 5; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s.Ri[g][k] = R(0);   // BP_1024.c:384-386
                s.Li[g][k] = R(0);   // :378-380
                if (g < 4) s.Lb[g][k] = R(0);
            }

        uint32_t bits = 0;
        int done = P.iters;
        bool conv = false;
        for (int it = 0; it < P.iters; ++it) {
            s.template sweepR<0>(); bp_wave_fence();
            s.template sweepR<1>(); bp_wave_fence();
            s.template sweepR<2>(); bp_wave_fence();
            s.template sweepR<3>();
            __syncthreads();
            if constexpr (STOP) {
                // x_hat of elements 256 k + 64 w + lane: words 8 k + 2 w and 8 k + 2 w + 1
                const uint32_t xk = s.sweepR4_xhat();
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint64_t m = __ballot((xk >> k) & 1u);
                    if ((s.t & 63) == 0) {
                        xw[8 * k + 2 * (s.t >> 6)] = (uint32_t)m;
                        xw[8 * k + 2 * (s.t >> 6) + 1] = (uint32_t)(m >> 32);
                    }
                }
            } else {
                s.template sweepR<4>();
            }
            s.template sweepL<4, false>(bits);
            __syncthreads();
            s.template sweepL<3, false>(bits); bp_wave_fence();
            s.template sweepL<2, false>(bits); bp_wave_fence();
            s.template sweepL<1, false>(bits); bp_wave_fence();
            if constexpr (STOP) {
                s.template sweepL<0, true>(bits);
                const uint32_t w = bp_r4_pack(bits, s.t);
                if ((s.t & 7) == 0) uw[s.t >> 3] = w;
                __syncthreads();
                // u_hat / x_hat of round trip it + 1 are read before this wave reaches the next round trip's barrier, and
                // rewritten only after it
                if (bp_g_holds(uw, xw, NW)) {
                    done = it + 1;
                    conv = true;
                    break;
                }
            } else {
                if (it + 1 == P.iters) s.template sweepL<0, true>(bits);
                else s.template sweepL<0, false>(bits);
                bp_wave_fence();
            }
        }
        // decisions of elements 4t .. 4t+3: eight lanes make one output word
        const uint32_t w = bp_r4_pack(bits, s.t);
        if ((s.t & 7) == 0) P.out_bits[(size_t)frame * NW + (s.t >> 3)] = w;
        if (STOP && s.t == 0) bp_put_stats(P, frame, done, conv);
        __syncthreads();   // the LDS rows are cleared for the next frame
    }
}


}  // namespace polar
