// gen_common.h -- what the device-side transmit chains share (gen_kernel.h k_generate, rm_kernel.h k_generate_rm, gen_dyn.h
// k_generate_dyn): their argument block, the counter-based generator (Philox4x32-10) and the steps of the chain, one frame
// per wavefront:  gen_place (payload, CRC, placement) -> gen_pack -> gen_emit_u -> gen_encode -> gen_normal_pair / gen_put.
// Layout: ub[N] holds one byte per u bit; lane l holds bits j = l + 64 k as bit k of a 64-bit word (KR = N / 64 bits used).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace polar {

struct GenParams {
    void *out;               // [B][N] double or float: LLR (2y/s/s) or y
    uint32_t *u_bits;        // [B][N/32] transmitted u, or null
    const int *info_order;   // [A]
    uint64_t seed, first_frame;
    double sigma;
    uint32_t crc_mask;       // bit t set <=> D^t in g(D), t < 32 (taps 0..r); 1 when no CRC
    uint32_t crc_top;        // tap r when r == 32 handled via crc_r
    int crc_r;
    const uint32_t *gc_rows; // systematic CRC (CASCL_1024_sys.c:48-561): row k = D^(r+k) mod g as an r-bit mask; else null
    int N, n, K, A, B;
    int out_is_f32, out_is_y;
    const uint32_t *sys_frozen;   // [N/32] frozen mask: systematic polar code (polar_set_systematic); null = off
};

struct Philox {
    uint32_t c[4];
    __device__ __forceinline__ static void round_(uint32_t *c, uint32_t k0, uint32_t k1)
    {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    }
    __device__ __forceinline__ Philox(uint64_t seed, uint64_t frame, uint32_t block, uint32_t stream)
    {
        c[0] = (uint32_t)frame; c[1] = (uint32_t)(frame >> 32); c[2] = block; c[3] = stream;
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            round_(c, k0, k1);
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
    }
    // two uniforms in (0,1] with 53 random bits each: k + 0.5 rounds to even for k >= 2^52, so 1.0 is reached (k = 2^53 - 1,
    // the normal is then 0) and 0 is not
    __device__ __forceinline__ double u0() const { return ((double)((((uint64_t)c[0] << 32) | c[1]) >> 11) + 0.5) * 0x1.0p-53; }
    __device__ __forceinline__ double u1() const { return ((double)((((uint64_t)c[2] << 32) | c[3]) >> 11) + 0.5) * 0x1.0p-53; }
};

// payload: K random bits (Philox stream 0) into vw[K/32 + 2]; CRC and placement u[I[i]] = w[i] into ub[N]; ends at the
// wavefront fence, after which every lane sees the whole of ub
__device__ __forceinline__ void gen_place(const GenParams &P, uint64_t frame, int lane, unsigned char *ub, uint32_t *vw)
{
    const int kw = (P.K + 31) >> 5;
    for (int w = lane; w < kw + 2; w += 64) {
        uint32_t v = 0;
        if (w < kw) {
            v = Philox(P.seed, frame, (uint32_t)w, 0u).c[0];
            if (w == kw - 1 && (P.K & 31)) v &= (1u << (P.K & 31)) - 1u;
        }
        vw[w] = v;
    }
    for (int j = lane; j < P.N; j += 64) ub[j] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (P.gc_rows) {
        // systematic CRC (CASCL_1024_sys.c:776-789): redundant part = sum of the generator rows of the set
        // payload bits, then the payload itself; placement u[I[i]] = w[i]
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
        // CRC multiply w(D) = v(D) g(D) (CASCL_1024_L8.c:251-266) and placement u[I[i]] = w[i] (:270-272)
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
}

// ub -> the lane word
__device__ __forceinline__ uint64_t gen_pack(const unsigned char *ub, int lane, int KR)
{
    uint64_t u = 0;
    for (int k = 0; k < KR; ++k) u |= (uint64_t)(ub[lane + 64 * k] & 1) << k;
    return u;
}

// the lane words -> row f of P.u_bits [B][N/32], when asked for
__device__ __forceinline__ void gen_emit_u(const GenParams &P, int f, uint64_t u, int lane, int KR)
{
    if (!P.u_bits) return;
    const int NW = P.N >> 5;
    for (int k = 0; k < KR; ++k) {
        const uint64_t m = __ballot((u >> k) & 1ull);  // bits j = 64k .. 64k+63
        if (lane == 0) {
            P.u_bits[(size_t)f * NW + 2 * k] = (uint32_t)m;
            P.u_bits[(size_t)f * NW + 2 * k + 1] = (uint32_t)(m >> 32);
        }
    }
}

// x = u F^{(x)n} (SCL_1024.c:242-250) on the lane words: strides < 64 across lanes, strides >= 64 inside the lane word
__device__ __forceinline__ uint64_t gen_encode(uint64_t x, int lane, int n, int KR)
{
    for (int s = 0; s < 6 && s < n; ++s) {
        const uint64_t o = __shfl_xor((unsigned long long)x, 1 << s);
        if (!(lane & (1 << s))) x ^= o;
    }
    for (int s = 6; s < n; ++s) {
        const int sh = 1 << (s - 6);
        uint64_t msk = 0;
        for (int k = 0; k < KR; ++k)
            if (!(k & sh)) msk |= 1ull << k;
        x ^= (x >> sh) & msk;
    }
    return x;
}

// two standard normals: Box-Muller on the two uniforms of Philox block `index` of `stream`
__device__ __forceinline__ void gen_normal_pair(uint64_t seed, uint64_t frame, uint32_t index, uint32_t stream, double nz[2])
{
    const Philox g(seed, frame, index, stream);
    const double r = sqrt(-2.0 * log(g.u0()));
    double sn, cs;
    sincospi(2.0 * g.u1(), &sn, &cs);
    nz[0] = r * cs;
    nz[1] = r * sn;
}

// one channel use: y = (1 - 2 bit) + sigma nz; element `idx` of P.out takes y, or the LLR 2 y / sigma / sigma
__device__ __forceinline__ void gen_put(const GenParams &P, size_t idx, bool bit, double nz)
{
    const double y = (bit ? -1.0 : 1.0) + P.sigma * nz;
    const double v = P.out_is_y ? y : 2 * y / P.sigma / P.sigma;
    if (P.out_is_f32) reinterpret_cast<float *>(P.out)[idx] = (float)v;
    else reinterpret_cast<double *>(P.out)[idx] = v;
}

// BPSK + AWGN over the N code bits of the lane words x (Philox stream 1: one block per pair of a lane's bits) into row f
__device__ __forceinline__ void gen_channel(const GenParams &P, uint64_t frame, int f, uint64_t x, int lane, int KR)
{
    for (int k2 = 0; k2 < KR; k2 += 2) {
        double nz[2];
        gen_normal_pair(P.seed, frame, (uint32_t)(lane + 64 * (k2 >> 1)), 1u, nz);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = k2 + h;
            if (k >= KR) break;   // N = 64: one element per lane, the second normal of the pair is not used
            gen_put(P, (size_t)f * P.N + (lane + 64 * k), (x >> k) & 1ull, nz[h]);
        }
    }
}

}  // namespace polar
