// k_fast2.hip -- k_scl_fast2 (L = 8, N = 1024, two codewords per wavefront: the headline kernel) and its launch code
#include "polar_host.h"
#include "scl_fast2.h"

namespace {

// two codewords per wavefront (scl_fast2.h), N = 1024, L = 8
// FROM_Y: the rows are channel observations (P.sigma > 0): k_scl_fast2_y; else LLRs: k_scl_fast2.  Occupancy, grid, scratch
// and the work queue are planned for the instantiation that is launched.
template <typename R, typename IN, bool CRC_ON, bool FROM_Y>
int launch_fast2(polar_ctx *c, const polar::SclParams &P)
{
    using Cfg = polar::Fast2Cfg<R>;
    auto kern = FROM_Y ? polar::k_scl_fast2_y<R, IN, CRC_ON> : polar::k_scl_fast2<R, IN, CRC_ON>;
    constexpr int WAVES = Cfg::WAVES;
    const size_t lds = Cfg::total;
    const long long pairs = ((long long)P.B + 1) / 2;
    LaunchShape s{64 * WAVES, lds, pairs, WAVES};   // more pairs than resident wavefronts: the rest through the work queue
    s.scratch_per_block = Cfg::scratch_elems * sizeof(R) * WAVES;
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), s, &pl);
    if (rc) return rc;
    polar::SclParams Q = P;
    Q.scratch = pl.scratch;
    Q.queue = pl.queue;
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(64 * WAVES), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

template <bool FROM_Y>
int fast2_types(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32, bool crc)
{
    if (!r32) return crc ? launch_fast2<double, double, true, FROM_Y>(c, P) : launch_fast2<double, double, false, FROM_Y>(c, P);
    if (in32) return crc ? launch_fast2<float, float, true, FROM_Y>(c, P) : launch_fast2<float, float, false, FROM_Y>(c, P);
    return crc ? launch_fast2<float, double, true, FROM_Y>(c, P) : launch_fast2<float, double, false, FROM_Y>(c, P);
}

}  // namespace

int polar_tu::scl_fast2(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32, bool crc)
{
    if (P.N != 1024) return POLAR_ENOKERNEL;
    if (!r32 && in32) return POLAR_ENOKERNEL;
    if (P.sigma > 0) return fast2_types<true>(c, P, r32, in32, crc);
    return fast2_types<false>(c, P, r32, in32, crc);
}
