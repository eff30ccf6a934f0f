// enc_kernel.h -- the encoder side on packed rows (include/polar_hip.h "Encoder, payload extraction, systematic polar codes").
//   k_transform      out = (in [^ in2]) F^{(x)n} [& ~frozen] on rows [B][N/32]
//   k_place          payload [B][KW] -> CRC word w (A bits) -> z[I[i]] = w[i], an N-bit row
//   k_extract        N-bit row [-> its transform] -> w[i] = z[I[i]] -> payload [B][KW] and the CRC verdict
//   k_dyn_fill       the dynamic frozen bits of a placed row, ascending position (rule 9 of the dynamic-frozen section)
//   k_rm_select      codeword [B][N/32] -> sent row [B][ceil(E/32)] (rules 1-3 of the rate-matching section)
//   k_count_sys      polar_count_errors_device in systematic mode: popcount of ((u_hat ^ u) F^{(x)n}) & info
// Layout of every kernel: one packed word per lane.  A frame is held by a group of G = min(N/32, 64) consecutive lanes, lane g
// of the group has word g (N = 4096: words g and g + 64), so a wavefront loads and stores 64 consecutive words of the batch.
// The transform runs its stages below 32 inside the word (shift and mask), the stages 32 .. 1024 across the lanes of the
// group (__shfl_xor) and the stage 2048 between the lane's two registers: no LDS.  Place and extract move single bits between
// arbitrary words of a frame; they stage the frame's words in LDS (at most 4 x 128 words per wavefront), wave-synchronous.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_bits.h"

namespace polar {

constexpr int ENC_THREADS = 256;

// the sub-block interleaver pattern P of 38.212 Table 5.4.1.1-1 (rule 1 of the rate-matching section)
static __constant__ unsigned char kEncSubblock[32] = {0, 1, 2, 4, 3, 5, 6, 7, 8, 16, 9, 17, 10, 18, 11, 19,
                                                      12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31};

// group geometry of a block length: logG = log2 of the lanes per frame, WPL = words per lane
__host__ __device__ inline int enc_log_group(int NW)
{
    int l = 0;
    while ((1 << l) < NW && l < 6) ++l;
    return l;
}

// x F^{(x)n} on the words of one frame: x[k] is word g + 64 k of the frame, g the lane's index in its group of min(NW, 64)
template <int WPL>
__device__ __forceinline__ void enc_xform(uint32_t (&x)[WPL], int NW, int g)
{
#pragma unroll
    for (int k = 0; k < WPL; ++k) {
        x[k] = polar_word_transform(x[k]);   // the strides below 32
    }
    const int G = NW < 64 ? NW : 64;
    for (int o = 1; o < G; o <<= 1) {
#pragma unroll
        for (int k = 0; k < WPL; ++k) {
            const uint32_t t = (uint32_t)__shfl_xor((int)x[k], o);
            if (!(g & o)) x[k] ^= t;
        }
    }
    if (WPL == 2) x[0] ^= x[1];
}

struct XformParams {
    const uint32_t *in;       // [B][NW]
    const uint32_t *in2;      // [B][NW] XORed onto `in` first, or null
    const uint32_t *frozen;   // [NW] the frozen positions of the result are cleared, or null
    uint32_t *out;            // [B][NW]; may be `in`
    int NW, B;
};

template <int WPL>
__global__ __launch_bounds__(ENC_THREADS) void k_transform(XformParams P)
{
    const int logG = enc_log_group(P.NW);
    const size_t gid = (size_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    const size_t f = gid >> logG;
    const int g = (int)(gid & ((1u << logG) - 1u));
    const bool live = f < (size_t)P.B;   // whole groups are live or not: a live lane's shuffle partners are live
    uint32_t x[WPL];
#pragma unroll
    for (int k = 0; k < WPL; ++k) {
        const size_t at = f * (size_t)P.NW + g + 64 * k;
        x[k] = live ? P.in[at] : 0u;
        if (live && P.in2) x[k] ^= P.in2[at];
    }
    enc_xform<WPL>(x, P.NW, g);
    if (!live) return;
#pragma unroll
    for (int k = 0; k < WPL; ++k) {
        if (P.frozen) x[k] &= ~P.frozen[g + 64 * k];
        P.out[f * (size_t)P.NW + g + 64 * k] = x[k];
    }
}

struct CountSysParams {
    const uint32_t *uhat, *u;        // [B][NW]
    const uint32_t *info;            // [NW] the positions compared
    unsigned long long *counters;    // [2] block errors, bit errors
    uint32_t *frame_err;             // [B] or null
    int NW, B;
};

// x_hat ^ x = (u_hat ^ u) F^{(x)n}: one transform of the difference, counted on the information positions
template <int WPL>
__global__ __launch_bounds__(ENC_THREADS) void k_count_sys(CountSysParams P)
{
    const int logG = enc_log_group(P.NW);
    const size_t gid = (size_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    const size_t f = gid >> logG;
    const int g = (int)(gid & ((1u << logG) - 1u));
    const bool live = f < (size_t)P.B;
    uint32_t x[WPL];
#pragma unroll
    for (int k = 0; k < WPL; ++k) {
        const size_t at = f * (size_t)P.NW + g + 64 * k;
        x[k] = live ? (P.uhat[at] ^ P.u[at]) : 0u;
    }
    enc_xform<WPL>(x, P.NW, g);
    int e = 0;
#pragma unroll
    for (int k = 0; k < WPL; ++k)
        if (live) e += __popc(x[k] & P.info[g + 64 * k]);
    for (int o = 1; o < (1 << logG); o <<= 1) e += __shfl_xor(e, o);
    if (live && g == 0) {
        if (P.frame_err) P.frame_err[f] = (uint32_t)e;
        if (e) {
            atomicAdd(&P.counters[0], 1ull);
            atomicAdd(&P.counters[1], (unsigned long long)e);
        }
    }
}

struct PlaceParams {
    const uint32_t *payload;   // [B][KW]; bits at or above K in the last word are ignored
    uint32_t *z;               // [B][NW]
    const uint16_t *inv;       // [N] i with I[i] = j, 0xFFFF at a frozen j
    const uint32_t *rtab;      // [A] D^i mod g(D)
    uint32_t crc_mask;         // bit t set <=> D^t in g(D), t < 32; 1 when no CRC
    uint32_t crc_top;          // tap 32
    int crc_r, crc_sys;
    int N, K, A, B;
};

struct ExtractParams {
    const uint32_t *z;         // [B][NW] decisions (or, with xform, their transform is what is read)
    uint32_t *payload;         // [B][KW], bits at or above K zero
    uint32_t *ok;              // [B] or null
    const int *info_order;     // [A]
    const uint32_t *rtab;      // [A]
    uint32_t crc_mask, crc_top;
    int crc_r, crc_sys, xform;
    int N, K, A, B;
};

// word m of (p(D) D^sh) for a polynomial of nw words in LDS (words outside 0 .. nw-1 are zero)
__device__ __forceinline__ uint32_t enc_shl_word(const uint32_t *p, int nw, int m, int sh)
{
    const int q = m - (sh >> 5), s = sh & 31;
    uint32_t v = (q >= 0 && q < nw) ? p[q] << s : 0u;
    if (s && q >= 1 && q - 1 < nw) v |= p[q - 1] >> (32 - s);
    return v;
}

__device__ __forceinline__ void enc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// XOR over the lanes of a group of 2^logG lanes
__device__ __forceinline__ uint32_t enc_group_xor(uint32_t v, int logG)
{
    for (int o = 1; o < (1 << logG); o <<= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// per-wavefront LDS of k_place / k_extract: four buffers of (64 >> logG) frames x NW words = max(64, NW) words each
constexpr int ENC_LDS_WORDS = 4 * 128 * (ENC_THREADS / 64);

__global__ __launch_bounds__(ENC_THREADS) void k_place(PlaceParams P)
{
    __shared__ uint32_t lds[ENC_LDS_WORDS];
    const int NW = P.N >> 5, KW = (P.K + 31) >> 5, AW = (P.A + 31) >> 5;
    const int logG = enc_log_group(NW), G = 1 << logG;
    const size_t gid = (size_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    const size_t f = gid >> logG;
    const int g = (int)(gid & (size_t)(G - 1));
    const int slot = (threadIdx.x & 63) >> logG;                       // frame of this wavefront
    uint32_t *base = lds + (threadIdx.x >> 6) * (4 * 128) + slot * NW;
    const int stride = NW < 64 ? 64 : NW;                              // words per buffer
    uint32_t *vb = base, *wb = base + stride;
    const bool live = f < (size_t)P.B;
    // payload words, the last one cut at K
    for (int m = g; m < NW; m += G) {
        uint32_t v = (live && m < KW) ? P.payload[f * (size_t)KW + m] : 0u;
        if (m == KW - 1 && (P.K & 31)) v &= (1u << (P.K & 31)) - 1u;
        vb[m] = v;
    }
    enc_wave_sync();
    if (P.crc_sys) {
        // w[0..r) = D^r v mod g = XOR of D^(r+k) mod g over the set payload bits, w[r..A) = v
        uint32_t par = 0;
        for (int m = g; m < KW; m += G) {
            uint32_t v = vb[m];
            while (v) {
                const int b = __ffs((int)v) - 1;
                v &= v - 1;
                par ^= P.rtab[P.crc_r + 32 * m + b];
            }
        }
        par = enc_group_xor(par, logG);
        for (int m = g; m < NW; m += G) wb[m] = enc_shl_word(vb, KW, m, P.crc_r) | (m == 0 ? par : 0u);
    } else {
        // w(D) = v(D) g(D)
        for (int m = g; m < NW; m += G) {
            uint32_t w = 0;
            for (int t = 0; t <= P.crc_r; ++t) {
                const bool tap = (t < 32) ? ((P.crc_mask >> t) & 1u) : (P.crc_top != 0);
                if (tap) w ^= enc_shl_word(vb, KW, m, t);
            }
            wb[m] = m < AW ? w : 0u;
        }
    }
    enc_wave_sync();
    // z[j] = w[inv[j]]
    for (int m = g; m < NW; m += G) {
        uint32_t z = 0;
        for (int b = 0; b < 32; ++b) {
            const uint32_t i = P.inv[32 * m + b];
            if (i != 0xFFFFu) z |= ((wb[i >> 5] >> (i & 31)) & 1u) << b;
        }
        if (live) P.z[f * (size_t)NW + m] = z;
    }
}

__global__ __launch_bounds__(ENC_THREADS) void k_extract(ExtractParams P)
{
    __shared__ uint32_t lds[ENC_LDS_WORDS];
    const int NW = P.N >> 5, KW = (P.K + 31) >> 5, AW = (P.A + 31) >> 5;
    const int logG = enc_log_group(NW), G = 1 << logG;
    const size_t gid = (size_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    const size_t f = gid >> logG;
    const int g = (int)(gid & (size_t)(G - 1));
    const int slot = (threadIdx.x & 63) >> logG;
    uint32_t *base = lds + (threadIdx.x >> 6) * (4 * 128) + slot * NW;
    const int stride = NW < 64 ? 64 : NW;
    uint32_t *zb = base, *wb = base + stride, *pa = base + 2 * stride, *pb = base + 3 * stride;
    const bool live = f < (size_t)P.B;
    // the row, transformed first in systematic mode (x_hat = u_hat F^{(x)n})
    if (NW == 128) {
        uint32_t x[2];
        for (int k = 0; k < 2; ++k) x[k] = live ? P.z[f * (size_t)NW + g + 64 * k] : 0u;
        if (P.xform) enc_xform<2>(x, NW, g);
        zb[g] = x[0];
        zb[g + 64] = x[1];
    } else {
        uint32_t x[1] = {live ? P.z[f * (size_t)NW + g] : 0u};
        if (P.xform) enc_xform<1>(x, NW, g);
        zb[g] = x[0];
    }
    enc_wave_sync();
    // w[i] = z[I[i]], and its remainder modulo g(D)
    uint32_t rem = 0;
    for (int m = g; m < NW; m += G) {
        uint32_t w = 0;
        for (int b = 0; b < 32 && 32 * m + b < P.A; ++b) {
            const int j = P.info_order[32 * m + b];
            const uint32_t bit = (zb[j >> 5] >> (j & 31)) & 1u;
            w |= bit << b;
            if (bit) rem ^= P.rtab[32 * m + b];
        }
        wb[m] = w;
    }
    rem = enc_group_xor(rem, logG);
    enc_wave_sync();
    const uint32_t *q = pa;
    if (P.crc_sys) {
        for (int m = g; m < KW; m += G) {   // v = w[r..A)
            const int s = P.crc_r & 31, o = m + (P.crc_r >> 5);
            uint32_t v = (o < AW ? wb[o] : 0u) >> s;
            if (s && o + 1 < AW) v |= wb[o + 1] << (32 - s);
            pa[m] = v;
        }
    } else {
        // quotient of w by g: (w - rem) / g is exact, and 1 / g = g(D) g(D^2) g(D^4) ... g(D^(2^(m-1))) mod D^(2^m) over
        // GF(2) because g(D)^(2^m) = g(D^(2^m)) = 1 mod D^(2^m) (g_0 = 1).  The quotient has K bits: 2^m >= K is enough.
        for (int m = g; m < NW; m += G) pa[m] = (m < KW) ? (wb[m] ^ (m == 0 ? rem : 0u)) : 0u;
        uint32_t *src = pa, *dst = pb;
        for (int sh = 1; P.crc_r > 0 && sh < P.K; sh <<= 1) {
            enc_wave_sync();
            for (int m = g; m < KW; m += G) {
                uint32_t a = 0;
                for (int t = 0; t <= P.crc_r; ++t) {
                    const bool tap = (t < 32) ? ((P.crc_mask >> t) & 1u) : (P.crc_top != 0);
                    if (tap && (long long)t * sh < P.K) a ^= enc_shl_word(src, KW, m, t * sh);
                }
                dst[m] = a;
            }
            uint32_t *t = src; src = dst; dst = t;
        }
        q = src;
    }
    enc_wave_sync();
    for (int m = g; m < KW; m += G) {
        uint32_t v = q[m];
        if (m == KW - 1 && (P.K & 31)) v &= (1u << (P.K & 31)) - 1u;
        if (live) P.payload[f * (size_t)KW + m] = v;
    }
    if (live && g == 0 && P.ok) P.ok[f] = rem == 0u ? 1u : 0u;
}

struct DynFillParams {
    uint32_t *z;              // [B][NW] in place
    const uint32_t *mask;     // [D][NW]
    const int *pos;           // [D] ascending
    int D, NW, B;
};

// u[pos[d]] = parity of (u AND mask row d), d = 0 .. D-1: a row refers to earlier positions only.  N <= 1024: one word per lane.
__global__ __launch_bounds__(ENC_THREADS) void k_dyn_fill(DynFillParams P)
{
    const int logG = enc_log_group(P.NW);
    const size_t gid = (size_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    const size_t f = gid >> logG;
    const int g = (int)(gid & ((1u << logG) - 1u));
    const bool live = f < (size_t)P.B;
    uint32_t z = live ? P.z[f * (size_t)P.NW + g] : 0u;
    for (int d = 0; d < P.D; ++d) {
        const int j = P.pos[d];
        const uint32_t par = enc_group_xor(z & P.mask[(size_t)d * P.NW + g], logG);
        if (g == (j >> 5)) z = (z & ~(1u << (j & 31))) | ((uint32_t)(__popc(par) & 1) << (j & 31));
    }
    if (live) P.z[f * (size_t)P.NW + g] = z;
}

struct RmSelectParams {
    const uint32_t *x;         // [B][NW] codewords
    uint32_t *e;               // [B][EW] sent rows, bits at or above E zero
    const uint16_t *ilv_inv;   // [E] ibil: e index of sent position t; else null
    int N, logS, E, mode, B;   // mode: 1 repeat, 2 puncture, 3 shorten (POLAR_RM_*)
};

// one sent word per lane: sent position t -> e index k (channel interleaver) -> y index m (bit selection) -> J(m)
__global__ __launch_bounds__(ENC_THREADS) void k_rm_select(RmSelectParams P)
{
    const int NW = P.N >> 5, EW = (P.E + 31) >> 5, S1 = (1 << P.logS) - 1;
    const size_t gid = (size_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    const size_t f = gid / (size_t)EW;
    if (f >= (size_t)P.B) return;
    const int ew = (int)(gid - f * (size_t)EW);
    const uint32_t *row = P.x + f * (size_t)NW;
    uint32_t o = 0;
    for (int b = 0; b < 32; ++b) {
        const int t = 32 * ew + b;
        if (t >= P.E) break;
        const int k = P.ilv_inv ? (int)P.ilv_inv[t] : t;
        const int m = (P.mode == 1) ? (k & (P.N - 1)) : (P.mode == 2) ? k + P.N - P.E : k;
        const int j = ((int)kEncSubblock[m >> P.logS] << P.logS) | (m & S1);
        o |= ((row[j >> 5] >> (j & 31)) & 1u) << b;
    }
    P.e[f * (size_t)EW + ew] = o;
}

}  // namespace polar
