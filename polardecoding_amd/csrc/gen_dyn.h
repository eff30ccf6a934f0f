// gen_dyn.h -- k_generate_dyn: the transmit chain of k_generate (gen_kernel.h; steps in gen_common.h) for a context with
// dynamic frozen bits (include/polar_hip.h, "Dynamic frozen bits"; the decoder is scl_dyn.h).
#pragma once
#include "gen_common.h"

namespace polar {

struct GenDynParams {
    GenParams g;
    const uint32_t *mask;   // [D][N/32]
    const int *pos;         // [D] ascending
    int D;
};

// payload, CRC and placement are the plain context's (same Philox stream 0), then u[pos[d]] = parity of (u AND mask row d)
// for d = 0 .. D-1 in ascending position, then encode and channel (stream 1)
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
        gen_place(P, frame, lane, ub, vw);
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
        const uint64_t u = gen_pack(ub, lane, KR);
        gen_emit_u(P, f, u, lane, KR);
        gen_channel(P, frame, f, gen_encode(u, lane, P.n, KR), lane, KR);
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace polar
