// gen_common.h -- what the device-side transmit chains share (gen_kernel.h k_generate, rm_kernel.h k_generate_rm): their
// argument block and the counter-based generator (Philox4x32-10).
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
    // two uniforms in (0,1) with 53 random bits each
    __device__ __forceinline__ double u0() const { return ((double)((((uint64_t)c[0] << 32) | c[1]) >> 11) + 0.5) * 0x1.0p-53; }
    __device__ __forceinline__ double u1() const { return ((double)((((uint64_t)c[2] << 32) | c[3]) >> 11) + 0.5) * 0x1.0p-53; }
};

}  // namespace polar
