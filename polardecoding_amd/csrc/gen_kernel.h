// gen_kernel.h -- device-side transmit chain: payload -> CRC multiply by g(D) -> u[I[i]] = w[i]
// -> x = u F^{(x)n} -> BPSK + AWGN -> channel LLR, one frame per wavefront, for throughput-mode Monte-Carlo.
// Restates the SHAPE of main()'s frame loop (CASCL_1024_L8.c:245-292); it is NOT the reference's sequential
// generator: the payload and the noise come from a counter-based generator (Philox4x32-10, keyed by the seed,
// counter = global frame index + element), so that a frame depends only on (seed, frame index) and batches can
// be cut and sharded freely.  Bit-exact reproduction of the reference's Ranq1 / Marsaglia stream stays on the
// host (host/polar_sim.c), because that stream cannot be indexed per frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gen_common.h"

namespace polar {

// lane l holds codeword / u bits j = l + 64 k as bit k of a 16-bit (N = 1024) .. 64-bit (N = 4096) word
__global__ __launch_bounds__(256) void k_generate(GenParams P)
{
    const int N = P.N, KR = N >> 6;  // KR = bits per lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    extern __shared__ unsigned char gsm[];
    unsigned char *ub = gsm + (size_t)wave * (N + 2 * 1024);       // u bytes [N]
    uint32_t *vw = reinterpret_cast<uint32_t *>(ub + N);           // payload words [K/32 + 2]
    const int waves = blockDim.x >> 6;
    for (int f = blockIdx.x * waves + wave; f < P.B; f += gridDim.x * waves) {
        const uint64_t frame = P.first_frame + (uint64_t)f;
        gen_place(P, frame, lane, ub, vw);
        uint64_t u = gen_pack(ub, lane, KR);
        if (P.sys_frozen) {
            // systematic polar code: the placed row z becomes u = (z F) with the frozen positions cleared, so that x = u F
            // carries z on the information set (include/polar_hip.h)
            uint64_t fz = 0;
            for (int k = 0; k < KR; ++k) fz |= (uint64_t)((P.sys_frozen[2 * k + (lane >> 5)] >> (lane & 31)) & 1u) << k;
            u = gen_encode(u, lane, P.n, KR) & ~fz;
        }
        gen_emit_u(P, f, u, lane, KR);
        // channel: y = (1 - 2x) + sigma n, n from Box-Muller on Philox uniforms; LLR = 2 y / sigma / sigma
        gen_channel(P, frame, f, gen_encode(u, lane, P.n, KR), lane, KR);
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace polar
