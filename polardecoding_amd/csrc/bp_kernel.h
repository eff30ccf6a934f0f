// bp_kernel.h -- flooding belief-propagation decoder (reference: BP, BP_1024.c:372-427).
//
// One codeword per workgroup; one butterfly (two CHK) per thread and stage; all messages in LDS.
// The reference keeps l[0..n][N] and r[0..n][N].  Of those only l[1..n-1] and r[1..n-1] are ever
// re-read: l[n] is the channel LLR (constant), r[0] is the frozen prior 999/0 (BP_1024.c:386-391,
// taken from the mask), r[n] is written but never read, and l[0] is read only by the final hard
// decision (:417-425).  Dropping the dead rows leaves (2(n-1)+1) N reals = 152 KB for N = 1024 in
// f64, which is what lets a whole f64 codeword sit in one CU's 160 KB LDS.
// Stage order, operand order inside CHK and inside the sums are the reference's.
//
// Synchronisation: a wavefront's 64 butterflies of a stage touch 128 elements.  With butterfly b = 64w + x
// the stages 0..6 of wave w stay inside elements [128w, 128w + 128) ("map A"); for the stages 7..n-1 the wave
// takes instead the elements whose low 7 bits lie in a 2^(14-n)-wide window, all high bits ("map B"), which is
// closed under those stages.  Consecutive stages under the same map exchange data only inside one wave (LDS
// executes a wave's operations in order), so the workgroup barrier is needed only where the map changes:
// twice per iteration for N = 1024 instead of 18 times, and the waves of a codeword drift apart enough to
// overlap one wave's table reads with another's arithmetic.
#pragma once
#include "polar_bits.h"
#include "polar_math.h"
#include "polar_lut.h"
#include "polar_params.h"

namespace polar {


// first element of butterfly bb in stage i (the partner is 2^i further)
__device__ __forceinline__ int bp_elem(int bb, int i, int n)
{
    if (i < 7) return ((bb >> i) << (i + 1)) | (bb & ((1 << i) - 1));
    const int lo_bits = 14 - n, t = i - 7;
    const int x = bb & 63, c = bb >> 6;
    const int h = x >> lo_bits;
    const int hi = ((h >> t) << (t + 1)) | (h & ((1 << t) - 1));
    return (hi << 7) | (c << lo_bits) | (x & ((1 << lo_bits) - 1));
}

// barrier between two consecutive stages: workgroup-wide where the element map changes, else wave-local
__device__ __forceinline__ void bp_sync(int stage_a, int stage_b)
{
    if ((stage_a < 7) != (stage_b < 7)) __syncthreads();
    else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// ---- stop rule POLAR_BP_STOP_G (include/polar_hip.h): after a round trip, u_hat F^{(x)n} == x_hat? ----------------------
// x = u F^{(x)n} in natural order (gen_kernel.h): the strides below 32 are polar_word_transform (polar_bits.h).
// One wavefront: the N/32 <= 128 words of u_hat and x_hat (LDS) -> does u_hat F == x_hat hold?  Wave-uniform result.  Lane l
// holds words l and l + 64; strides of 32..1024 elements are lane exchanges, 2048 is the lane's own pair.
__device__ __forceinline__ bool bp_g_holds(const uint32_t *u, const uint32_t *x, int NW)
{
    const int lane = threadIdx.x & 63;
    uint32_t v0 = lane < NW ? polar_word_transform(u[lane]) : 0u;
    uint32_t v1 = lane + 64 < NW ? polar_word_transform(u[lane + 64]) : 0u;
    for (int sw = 1; sw < NW && sw < 64; sw <<= 1) {
        const uint32_t o0 = (uint32_t)__shfl_xor((int)v0, sw), o1 = (uint32_t)__shfl_xor((int)v1, sw);
        if (!(lane & sw)) {
            v0 ^= o0;
            v1 ^= o1;
        }
    }
    if (NW > 64) v0 ^= v1;
    const uint32_t x0 = lane < NW ? x[lane] : 0u, x1 = lane + 64 < NW ? x[lane + 64] : 0u;
    return __ballot(v0 != x0 || v1 != x1) == 0;
}
// round trips run and BP_FLAG_CONVERGED of one frame, where the caller asked for them
__device__ __forceinline__ void bp_put_stats(const BpParams &P, int frame, int iters, bool conv)
{
    if (P.iters_out) P.iters_out[frame] = (uint32_t)iters;
    if (P.flags_out) P.flags_out[frame] = conv ? BP_FLAG_CONVERGED : 0u;
}

// STOP (stop rule G): l[0] in every round trip, r[n] formed by the last R stage as the hard decisions x_hat (into LDS
// bits, the row itself is not stored), then one wave checks u_hat F == x_hat and publishes a workgroup-uniform flag.
template <typename R, typename IN, bool STOP = false>
__global__ __launch_bounds__(512) void k_bp(BpParams P)
{
    const int N = P.N, n = P.n, NW = N >> 5;
    const int tid = threadIdx.x, nt = blockDim.x;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    R *ch = reinterpret_cast<R *>(smem);
    R *lm = ch + N;                       // rows 1..n-1 of l
    R *rm = lm + (size_t)(n - 1) * N;     // rows 1..n-1 of r
    uint32_t *obits = reinterpret_cast<uint32_t *>(rm + (size_t)(n - 1) * N);  // [NW]
    uint32_t *xbits = obits + NW;         // STOP: [NW] x_hat, then the stop flag
    int *stopf = reinterpret_cast<int *>(xbits + NW);
    unsigned char *lut_mem = reinterpret_cast<unsigned char *>(STOP ? reinterpret_cast<uint32_t *>(stopf + 4) : obits + NW);
    lut_mem += (16 - (reinterpret_cast<uintptr_t>(lut_mem) & 15)) & 15;
    Lut<R>::build(lut_mem, tid, nt);
    Lut<R> lut;   // the stages are latency-bound chains (2 waves per SIMD in f64): chk_lut1 wins over the compact chk_lut
    lut.bind(lut_mem);
    __syncthreads();

    __shared__ int job_slot;
    for (int frame = blockIdx.x; frame < P.B; frame = next_job_block(P.queue, frame, (int)gridDim.x, P.B, &job_slot)) {
        const IN *src = reinterpret_cast<const IN *>(P.in) + (size_t)frame * N;
        for (int i = tid; i < N; i += nt) {
            ch[i] = (R)channel_llr<IN>(src, i, P.sigma);  // BP_1024.c:381-382
        }
        for (int i = tid; i < (n - 1) * N; i += nt) {
            lm[i] = R(0);  // BP_1024.c:378-380
            rm[i] = R(0);  // BP_1024.c:384-386
        }
        for (int i = tid; i < NW; i += nt) obits[i] = 0;
        if constexpr (STOP)
            for (int i = tid; i < NW; i += nt) xbits[i] = 0;
        __syncthreads();

        int done = P.iters;
        bool conv = false;
        for (int it = 0; it < P.iters; ++it) {
            const bool last = (it + 1 == P.iters);
            // R sweep (BP_1024.c:395-404); stage n-1 only produces r[n], which nobody reads (but the stop rule)
            for (int i = 0; i + (STOP ? 0 : 1) < n; ++i) {
                const int s = 1 << i;
                for (int b = tid; b < N / 2; b += nt) {
                    const int j = bp_elem(b, i, n);
                    R r0, r1;
                    if (i == 0) {
                        r0 = ((P.frozen[j >> 5] >> (j & 31)) & 1) ? R(999) : R(0);
                        r1 = ((P.frozen[(j + s) >> 5] >> ((j + s) & 31)) & 1) ? R(999) : R(0);
                    } else {
                        r0 = rm[(size_t)(i - 1) * N + j];
                        r1 = rm[(size_t)(i - 1) * N + j + s];
                    }
                    const R *lrow = (i + 1 == n) ? ch : lm + (size_t)i * N;
                    const R l0 = lrow[j], l1 = lrow[j + s];
                    const R a = chk_lut1<R>(r0, l1 + r1, lut);
                    const R c = r1 + chk_lut1<R>(r0, l0, lut);
                    if (STOP && i + 1 == n) {
                        // x_hat: (l[n] + r[n] >= 0) -> 0
                        if (!(l0 + a >= R(0))) atomicOr(&xbits[j >> 5], 1u << (j & 31));
                        if (!(l1 + c >= R(0))) atomicOr(&xbits[(j + s) >> 5], 1u << ((j + s) & 31));
                    } else {
                        rm[(size_t)i * N + j] = a;
                        rm[(size_t)i * N + j + s] = c;
                    }
                }
                bp_sync(i, i + 1);  // next: R stage i+1, or L stage n-1
            }
            // L sweep (BP_1024.c:406-415); l[0] is needed only for the decision
            for (int i = n - 1; i >= ((STOP || last) ? 0 : 1); --i) {
                const int s = 1 << i;
                for (int b = tid; b < N / 2; b += nt) {
                    const int j = bp_elem(b, i, n);
                    R r0, r1;
                    bool f0 = false, f1 = false;
                    if (i == 0) {
                        f0 = (P.frozen[j >> 5] >> (j & 31)) & 1;
                        f1 = (P.frozen[(j + s) >> 5] >> ((j + s) & 31)) & 1;
                        r0 = f0 ? R(999) : R(0);
                        r1 = f1 ? R(999) : R(0);
                    } else {
                        r0 = rm[(size_t)(i - 1) * N + j];
                        r1 = rm[(size_t)(i - 1) * N + j + s];
                    }
                    const R *lrow = (i + 1 == n) ? ch : lm + (size_t)i * N;
                    const R l0 = lrow[j], l1 = lrow[j + s];
                    const R a = chk_lut1<R>(l0, l1 + r1, lut);
                    const R c = l1 + chk_lut1<R>(r0, l0, lut);
                    if (i > 0) {
                        lm[(size_t)(i - 1) * N + j] = a;
                        lm[(size_t)(i - 1) * N + j + s] = c;
                    } else {
                        // BP_1024.c:417-425: frozen -> 0, else (l + r >= 0) -> 0
                        const uint32_t b0 = (!f0 && !(a + r0 >= R(0))) ? 1u : 0u;
                        const uint32_t b1 = (!f1 && !(c + r1 >= R(0))) ? 1u : 0u;
                        if (b0) atomicOr(&obits[j >> 5], 1u << (j & 31));
                        if (b1) atomicOr(&obits[(j + s) >> 5], 1u << ((j + s) & 31));
                    }
                }
                if (i > 0) bp_sync(i, i - 1);  // after L stage 1 comes R stage 0 of the next iteration
            }
            if constexpr (STOP) {
                __syncthreads();
                if (tid < 64) {
                    const bool hold = bp_g_holds(obits, xbits, NW);
                    if (!hold && !last)   // the next round trip ORs its decisions in afresh
                        for (int w = tid; w < NW; w += 64) obits[w] = xbits[w] = 0;
                    if (tid == 0) *stopf = hold;
                }
                __syncthreads();
                if (*stopf) {
                    done = it + 1;
                    conv = true;
                    break;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < NW; i += nt) P.out_bits[(size_t)frame * NW + i] = obits[i];
        if (STOP && tid == 0) bp_put_stats(P, frame, done, conv);
        __syncthreads();
    }
}


template <typename R>
constexpr size_t bp_lds_bytes(int N, int n, bool stop = false)
{
    return sizeof(R) * (size_t)N * (1 + 2 * (n - 1)) + sizeof(uint32_t) * (size_t)(N / 32) * (stop ? 2 : 1) + (stop ? 16 : 0) +
           16 + Lut<R>::bytes;
}

// ---- BP with per-stage read-outs (reference: BPr, BPr_128.c:373-575) -------------------------
// The same flooding schedule with every row kept (the read-out of stage i needs l[i] + r[i] for i = 0..n, so
// r[n] and l[0] are computed in every iteration as the reference does), one codeword per workgroup, N/2 threads.
// After the iterations listed in cp[] the hard decisions of every stage are carried back to the u side through
// the inverse butterflies (:417-438) and compared with the sent bits on the information set.

template <typename R, typename IN>
__global__ __launch_bounds__(256) void k_bp_readout(BpReadoutParams P)
{
    const int N = P.N, n = P.n, NW = N >> 5;
    const int tid = threadIdx.x, nt = blockDim.x;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    R *lm = reinterpret_cast<R *>(smem);                 // l[0..n][N]
    R *rm = lm + (size_t)(n + 1) * N;                     // r[0..n][N]
    unsigned char *bb = reinterpret_cast<unsigned char *>(rm + (size_t)(n + 1) * N);   // [N] read-out bits
    uint32_t *obits = reinterpret_cast<uint32_t *>(bb + N);                            // [NW]
    uint32_t *cnt = obits + NW;                                                        // [1]
    unsigned char *lut_mem = reinterpret_cast<unsigned char *>(cnt + 4);
    lut_mem += (16 - (reinterpret_cast<uintptr_t>(lut_mem) & 15)) & 15;
    Lut<R>::build(lut_mem, tid, nt);
    Lut<R> lut;
    lut.bind(lut_mem);
    __syncthreads();
#define LM(i, j) lm[(size_t)(i) * N + (j)]
#define RM(i, j) rm[(size_t)(i) * N + (j)]
    for (int frame = blockIdx.x; frame < P.B; frame += gridDim.x) {
        const IN *src = reinterpret_cast<const IN *>(P.in) + (size_t)frame * N;
        for (int i = tid; i < (n + 1) * N; i += nt) {
            lm[i] = R(0);   // BPr_128.c:379-381
            rm[i] = R(0);   // :385-387
        }
        __syncthreads();
        for (int j = tid; j < N; j += nt) {
            LM(n, j) = (R)channel_llr<IN>(src, j, P.sigma);                         // :382-383
            RM(0, j) = ((P.frozen[j >> 5] >> (j & 31)) & 1) ? R(999) : R(0);        // :388-393
        }
        for (int i = tid; i < NW; i += nt) obits[i] = 0;
        __syncthreads();
        int q = 0;
        for (int it = 0; it < P.iters; ++it) {
            for (int i = 0; i < n; ++i) {   // R sweep (:396-405)
                const int s = 1 << i;
                for (int b = tid; b < N / 2; b += nt) {
                    const int j = ((b >> i) << (i + 1)) | (b & (s - 1));
                    const R r0 = RM(i, j), r1 = RM(i, j + s), l0 = LM(i + 1, j), l1 = LM(i + 1, j + s);
                    RM(i + 1, j) = chk_lut<R>(r0, l1 + r1, lut);
                    RM(i + 1, j + s) = r1 + chk_lut<R>(r0, l0, lut);
                }
                __syncthreads();
            }
            for (int i = n - 1; i >= 0; --i) {   // L sweep (:406-415)
                const int s = 1 << i;
                for (int b = tid; b < N / 2; b += nt) {
                    const int j = ((b >> i) << (i + 1)) | (b & (s - 1));
                    const R r0 = RM(i, j), r1 = RM(i, j + s), l0 = LM(i + 1, j), l1 = LM(i + 1, j + s);
                    LM(i, j) = chk_lut<R>(l0, l1 + r1, lut);
                    LM(i, j + s) = l1 + chk_lut<R>(r0, l0, lut);
                }
                __syncthreads();
            }
            if (q < P.ncp && P.cp[q] == it + 1) {   // read-out (:417-438)
                for (int i = 0; i <= n; ++i) {
                    if (tid == 0) cnt[0] = 0;
                    for (int j = tid; j < N; j += nt) bb[j] = (LM(i, j) + RM(i, j) >= R(0)) ? 0 : 1;
                    __syncthreads();
                    for (int k = i; k > 0; --k) {
                        const int s = 1 << (k - 1);
                        for (int b = tid; b < N / 2; b += nt) {
                            const int j = ((b >> (k - 1)) << k) | (b & (s - 1));
                            bb[j] ^= bb[j + s];
                        }
                        __syncthreads();
                    }
                    uint32_t e = 0;
                    for (int j = tid; j < N; j += nt) {
                        const uint32_t sent = (P.u_bits[(size_t)frame * NW + (j >> 5)] >> (j & 31)) & 1u;
                        const uint32_t isinfo = (P.info[j >> 5] >> (j & 31)) & 1u;
                        e += isinfo & (sent ^ (uint32_t)bb[j]);
                    }
                    if (e) atomicAdd(&cnt[0], e);
                    __syncthreads();
                    if (tid == 0 && cnt[0]) atomicAdd(&P.E[(size_t)q * (n + 1) + i], (unsigned long long)cnt[0]);
                    __syncthreads();
                }
                ++q;
            }
        }
        for (int j = tid; j < N; j += nt) {   // :566-574
            const bool fr = (P.frozen[j >> 5] >> (j & 31)) & 1;
            if (!fr && !(LM(0, j) + RM(0, j) >= R(0))) atomicOr(&obits[j >> 5], 1u << (j & 31));
        }
        __syncthreads();
        if (P.out_bits)
            for (int i = tid; i < NW; i += nt) P.out_bits[(size_t)frame * NW + i] = obits[i];
        __syncthreads();
    }
#undef LM
#undef RM
}

template <typename R>
constexpr size_t bp_readout_lds_bytes(int N, int n)
{
    return sizeof(R) * 2 * (size_t)(n + 1) * N + (size_t)N + 4 * (size_t)(N / 32) + 16 + 16 + Lut<R>::bytes;
}

// ---- BP for block lengths whose messages do not fit one CU's LDS (N > 1024): same schedule, rows in a per-workgroup
// slice of a global scratch buffer (plain stores, sc1 loads, a workgroup barrier after every stage).  Correct and
// complete rather than fast: no reference program and no BASELINE config uses BP above N = 1024.
// Every row is kept here, so the stop rule (STOP) reads r[n] and l[0] as they are.
template <typename R, typename IN, bool STOP = false>
__global__ __launch_bounds__(512) void k_bp_global(BpParams P, R *scratch)
{
    const int N = P.N, n = P.n, NW = N >> 5;
    const int tid = threadIdx.x, nt = blockDim.x;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *obits = reinterpret_cast<uint32_t *>(smem);   // [NW]
    uint32_t *xbits = obits + NW;                            // STOP: [NW] x_hat, then the stop flag
    int *stopf = reinterpret_cast<int *>(xbits + NW);
    unsigned char *lut_mem = reinterpret_cast<unsigned char *>(STOP ? reinterpret_cast<uint32_t *>(stopf + 4) : obits + NW);
    lut_mem += (16 - (reinterpret_cast<uintptr_t>(lut_mem) & 15)) & 15;
    Lut<R>::build(lut_mem, tid, nt);
    Lut<R> lut;
    lut.bind(lut_mem);
    R *lm = scratch + (size_t)blockIdx.x * 2 * (size_t)(n + 1) * N;   // l[0..n][N]
    R *rm = lm + (size_t)(n + 1) * N;                                  // r[0..n][N]
    auto ld = [](const R *q) -> R { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    __syncthreads();
#define LM(i, j) lm[(size_t)(i) * N + (j)]
#define RM(i, j) rm[(size_t)(i) * N + (j)]
    for (int frame = blockIdx.x; frame < P.B; frame += gridDim.x) {
        const IN *src = reinterpret_cast<const IN *>(P.in) + (size_t)frame * N;
        for (int i = tid; i < (n + 1) * N; i += nt) {
            lm[i] = R(0);
            rm[i] = R(0);
        }
        __syncthreads();
        for (int j = tid; j < N; j += nt) {
            LM(n, j) = (R)channel_llr<IN>(src, j, P.sigma);
            RM(0, j) = ((P.frozen[j >> 5] >> (j & 31)) & 1) ? R(999) : R(0);
        }
        for (int i = tid; i < NW; i += nt) obits[i] = 0;
        if constexpr (STOP)
            for (int i = tid; i < NW; i += nt) xbits[i] = 0;
        __syncthreads();
        int done = P.iters;
        bool conv = false;
        for (int it = 0; it < P.iters; ++it) {
            for (int i = 0; i < n; ++i) {
                const int s = 1 << i;
                for (int b = tid; b < N / 2; b += nt) {
                    const int j = ((b >> i) << (i + 1)) | (b & (s - 1));
                    const R r0 = ld(&RM(i, j)), r1 = ld(&RM(i, j + s)), l0 = ld(&LM(i + 1, j)), l1 = ld(&LM(i + 1, j + s));
                    RM(i + 1, j) = chk_lut<R>(r0, l1 + r1, lut);
                    RM(i + 1, j + s) = r1 + chk_lut<R>(r0, l0, lut);
                }
                __syncthreads();
            }
            for (int i = n - 1; i >= 0; --i) {
                const int s = 1 << i;
                for (int b = tid; b < N / 2; b += nt) {
                    const int j = ((b >> i) << (i + 1)) | (b & (s - 1));
                    const R r0 = ld(&RM(i, j)), r1 = ld(&RM(i, j + s)), l0 = ld(&LM(i + 1, j)), l1 = ld(&LM(i + 1, j + s));
                    LM(i, j) = chk_lut<R>(l0, l1 + r1, lut);
                    LM(i, j + s) = l1 + chk_lut<R>(r0, l0, lut);
                }
                __syncthreads();
            }
            if constexpr (STOP) {
                for (int j = tid; j < N; j += nt) {
                    const bool fr = (P.frozen[j >> 5] >> (j & 31)) & 1;
                    if (!fr && !(ld(&LM(0, j)) + ld(&RM(0, j)) >= R(0))) atomicOr(&obits[j >> 5], 1u << (j & 31));
                    if (!(ld(&LM(n, j)) + ld(&RM(n, j)) >= R(0))) atomicOr(&xbits[j >> 5], 1u << (j & 31));
                }
                __syncthreads();
                if (tid < 64) {
                    const bool hold = bp_g_holds(obits, xbits, NW);
                    if (!hold)   // the decision below (or of the next round trip) ORs the bits in afresh
                        for (int w = tid; w < NW; w += 64) obits[w] = xbits[w] = 0;
                    if (tid == 0) *stopf = hold;
                }
                __syncthreads();
                if (*stopf) {
                    done = it + 1;
                    conv = true;
                    break;
                }
            }
        }
        for (int j = tid; j < N; j += nt) {
            const bool fr = (P.frozen[j >> 5] >> (j & 31)) & 1;
            if (!fr && !(ld(&LM(0, j)) + ld(&RM(0, j)) >= R(0))) atomicOr(&obits[j >> 5], 1u << (j & 31));
        }
        __syncthreads();
        for (int i = tid; i < NW; i += nt) P.out_bits[(size_t)frame * NW + i] = obits[i];
        if (STOP && tid == 0) bp_put_stats(P, frame, done, conv);
        __syncthreads();
    }
#undef LM
#undef RM
}

}  // namespace polar
