// rm_kernel.h -- 5G NR rate matching (TS 38.212 5.4.1, include/polar_hip.h rules 1-6) on the device.
//   k_rm_recover<IN>: the receiver's recovery, [B][E] received values -> [B][N] decoder rows (the hot path of every decode on
//                     a rate-matched context).  One workgroup per frame at a time: the row is loaded coalesced (16-byte
//                     loads, scalar head and tail when E breaks the alignment) into LDS, every output is gathered from LDS
//                     through J^-1 (from the 32-entry table in LDS) and, with ibil, the channel interleaver's table (also in
//                     LDS, loaded once per workgroup), and the N-wide row is stored coalesced.
//   k_generate_rm:    the transmit chain of k_generate (payload, CRC, placement, u F^{(x)n}) followed by rules 1-3 and
//                     BPSK + AWGN over the E sent values, one frame per wavefront.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gen_common.h"
#include "polar_math.h"

namespace polar {

constexpr int RM_THREADS = 256;
constexpr int RM_REPEAT = 1, RM_PUNCTURE = 2, RM_SHORTEN = 3;   // POLAR_RM_*
constexpr double RM_SHORT_LLR = 1048576.0;                       // POLAR_RM_SHORT_LLR

// the sub-block interleaver pattern P of 38.212 Table 5.4.1.1-1
__constant__ unsigned char kRmP[32] = {0, 1, 2, 4, 3, 5, 6, 7, 8, 16, 9, 17, 10, 18, 11, 19,
                                       12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31};

struct RmParams {
    const void *in;          // [B][E] double or float: LLRs, or y when sigma > 0
    void *out;               // [B][N] same type
    const uint16_t *ilv;     // [E] ibil: sent-row position of e_k; else null
    double sigma;
    int N, logS, E, B;       // S = N / 32 = 2^logS
    int mode;                // RM_REPEAT | RM_PUNCTURE | RM_SHORTEN
    int out_vec;             // out is 16-byte aligned: 16-byte stores
};

// LDS: [32] J^-1 table (int), [E] ilv table (uint16, ibil only, 16-byte padded), then the row with a head pad of up to
// 16 bytes so that it sits in LDS with the alignment it has in memory
__host__ __device__ inline size_t rm_recover_lds(int E, int ibil, size_t esz)
{
    return 128 + (ibil ? ((size_t)E * 2 + 15) / 16 * 16 : 0) + ((size_t)E * esz + 16 + 15) / 16 * 16;
}

template <typename IN>
__global__ __launch_bounds__(RM_THREADS) void k_rm_recover(RmParams P)
{
    constexpr int VEC = 16 / sizeof(IN);
    extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
    int *pinv = reinterpret_cast<int *>(rsm);
    uint16_t *ilv = reinterpret_cast<uint16_t *>(rsm + 128);
    IN *row = reinterpret_cast<IN *>(rsm + 128 + (P.ilv ? ((size_t)P.E * 2 + 15) / 16 * 16 : 0));
    const int tid = threadIdx.x, E = P.E, N = P.N, S1 = (1 << P.logS) - 1;
    if (tid < 32) pinv[kRmP[tid]] = tid;
    if (P.ilv)
        for (int k = tid; k < E; k += RM_THREADS) ilv[k] = P.ilv[k];
    const bool y = P.sigma > 0;
    for (int f = blockIdx.x; f < P.B; f += gridDim.x) {
        __syncthreads();   // the tables are in place; the previous frame's gathers are done with the row
        const IN *src = reinterpret_cast<const IN *>(P.in) + (size_t)f * E;
        const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 15);
        const int hs = mis / (int)sizeof(IN);                       // row[hs + k] = src[k]
        const int head = min(E, ((16 - mis) & 15) / (int)sizeof(IN));
        const int nv = (E - head) / VEC, tail0 = head + nv * VEC;
        if (tid < head) row[hs + tid] = src[tid];
        const uint4 *vs = reinterpret_cast<const uint4 *>(src + head);
        uint4 *vd = reinterpret_cast<uint4 *>(row + hs + head);
        for (int i = tid; i < nv; i += RM_THREADS) vd[i] = vs[i];
        if (tail0 + tid < E) row[hs + tail0 + tid] = src[tail0 + tid];
        __syncthreads();
        auto term = [&](int k) -> double {
            const double v = (double)row[hs + (P.ilv ? (int)ilv[k] : k)];
            return y ? llr_from_y(v, P.sigma) : v;
        };
        IN *dst = reinterpret_cast<IN *>(P.out) + (size_t)f * N;
        for (int p0 = tid * VEC; p0 < N; p0 += RM_THREADS * VEC) {
            IN o[VEC];
#pragma unroll
            for (int h = 0; h < VEC; ++h) {
                const int p = p0 + h;
                const int n = (pinv[p >> P.logS] << P.logS) | (p & S1);   // J(n) = p
                double v;
                if (P.mode == RM_REPEAT) {
                    v = term(n);
                    for (int k = n + N; k < E; k += N) v += term(k);
                } else if (P.mode == RM_PUNCTURE) {
                    v = (n < N - E) ? 0.0 : term(n - (N - E));
                } else {
                    v = (n < E) ? term(n) : RM_SHORT_LLR;
                }
                o[h] = (IN)v;
            }
            if (P.out_vec) {
                uint4 w;
                __builtin_memcpy(&w, o, sizeof w);
                *reinterpret_cast<uint4 *>(dst + p0) = w;
            } else {
#pragma unroll
                for (int h = 0; h < VEC; ++h) dst[p0 + h] = o[h];
            }
        }
    }
}

struct GenRmParams {
    GenParams g;             // out = [B][E]; everything else as for k_generate
    const uint16_t *ilv_inv; // [E] ibil: e index of sent position t; else null
    int E, logS, mode;
};

// k_generate's encoder (gen_common.h: payload, CRC multiply or systematic rows, placement, butterfly; same Philox stream 0
// payload), then per sent position t: e index k (channel interleaver), y index m (bit selection), codeword position J(m)
__global__ __launch_bounds__(256) void k_generate_rm(GenRmParams R)
{
    const GenParams &P = R.g;
    const int N = P.N, KR = N >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    extern __shared__ unsigned char gsm[];
    unsigned char *ub = gsm + (size_t)wave * (N + 2 * 1024);       // u bytes [N], then the codeword bytes
    uint32_t *vw = reinterpret_cast<uint32_t *>(ub + N);           // payload words [K/32 + 2]
    const int waves = blockDim.x >> 6;
    const int E = R.E, S1 = (1 << R.logS) - 1;
    for (int f = blockIdx.x * waves + wave; f < P.B; f += gridDim.x * waves) {
        const uint64_t frame = P.first_frame + (uint64_t)f;
        gen_place(P, frame, lane, ub, vw);
        const uint64_t u = gen_pack(ub, lane, KR);
        gen_emit_u(P, f, u, lane, KR);
        const uint64_t x = gen_encode(u, lane, P.n, KR);
        __builtin_amdgcn_wave_barrier();   // every lane has read its u bytes before they become codeword bytes
        for (int k = 0; k < KR; ++k) ub[lane + 64 * k] = (unsigned char)((x >> k) & 1ull);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // sent positions t = 2q, 2q + 1: one Philox block (stream 2) per pair, normal (t & 1) of it
        for (int q = lane; 2 * q < E; q += 64) {
            double nz[2];
            gen_normal_pair(P.seed, frame, (uint32_t)q, 2u, nz);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int t = 2 * q + h;
                if (t >= E) break;
                const int k = R.ilv_inv ? (int)R.ilv_inv[t] : t;
                const int m = (R.mode == RM_REPEAT) ? (k & (N - 1)) : (R.mode == RM_PUNCTURE) ? k + N - E : k;
                const int j = ((int)kRmP[m >> R.logS] << R.logS) | (m & S1);
                gen_put(P, (size_t)f * E + t, ub[j], nz[h]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace polar
