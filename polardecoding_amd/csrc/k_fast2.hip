// k_fast2.hip -- k_scl_fast2 (L = 8, N = 1024, two codewords per wavefront: the headline kernel) and its launch code
#include "polar_host.h"
#include "scl_fast2.h"

namespace {

// two codewords per wavefront (scl_fast2.h), N = 1024, L = 8
template <typename R, typename IN, bool CRC_ON>
int launch_fast2(polar_ctx *c, const polar::SclParams &P)
{
    using Cfg = polar::Fast2Cfg<R>;
    auto kern = polar::k_scl_fast2<R, IN, CRC_ON>;
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

}  // namespace

int polar_tu::scl_fast2(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32, bool crc)
{
    if (P.N != 1024) return POLAR_ENOKERNEL;
    if (!r32) {
        if (in32) return POLAR_ENOKERNEL;
        return crc ? launch_fast2<double, double, true>(c, P) : launch_fast2<double, double, false>(c, P);
    }
    if (in32) return crc ? launch_fast2<float, float, true>(c, P) : launch_fast2<float, float, false>(c, P);
    return crc ? launch_fast2<float, double, true>(c, P) : launch_fast2<float, double, false>(c, P);
}
