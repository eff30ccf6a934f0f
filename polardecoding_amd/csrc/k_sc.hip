// k_sc.hip -- k_sc_lanes (SC, one codeword per lane) and its launch code
#include "polar_host.h"
#include "sc_lanes.h"

namespace {

// SC, one codeword per lane (sc_lanes.h)
template <typename R, typename IN>
int launch_sc_lanes(polar_ctx *c, const polar::SclParams &P)
{
    using Cfg = polar::ScLanesCfg<R>;
    auto kern = polar::k_sc_lanes<R, IN>;
    const size_t lds = Cfg::lds_bytes(P.N);
    const int threads = 64 * Cfg::WAVES;
    const long long batches = ((long long)P.B + 63) / 64;
    LaunchShape s{threads, lds, batches, Cfg::WAVES};
    s.scratch_per_block = Cfg::scratch_bytes(P.N) * Cfg::WAVES;
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), s, &pl);
    if (rc) return rc;
    polar::SclParams Q = P;
    Q.scratch = pl.scratch;
    Q.queue = pl.queue;
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(threads), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

}  // namespace

int polar_tu::sc_lanes(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32)
{
    if (!r32) return in32 ? launch_sc_lanes<double, float>(c, P) : launch_sc_lanes<double, double>(c, P);
    return in32 ? launch_sc_lanes<float, float>(c, P) : launch_sc_lanes<float, double>(c, P);
}
