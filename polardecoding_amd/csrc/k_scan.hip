// k_scan.hip -- k_scan_lanes (SCAN, one codeword per lane, scan_lanes.h) and its launch code
#include "polar_host.h"
#include "scan_lanes.h"

namespace {

// The stored betas make a wavefront's slice large (N = 1024, f64: 4.25 MiB), so the resident wavefronts are limited by a
// byte budget for the ctx scratch as well as by the occupancy: at most 4 GiB.
constexpr size_t SCAN_SCRATCH_BUDGET = (size_t)4 << 30;

template <typename R, typename IN>
int launch_scan_lanes(polar_ctx *c, const polar::ScanParams &P)
{
    using Cfg = polar::ScanCfg<R>;
    auto kern = polar::k_scan_lanes<R, IN>;
    const size_t lds = Cfg::lds_bytes();
    const int threads = 64 * Cfg::WAVES;
    const size_t wg_bytes = Cfg::scratch_bytes(P.N, P.n) * Cfg::WAVES;
    const long long batches = ((long long)P.B + 63) / 64;
    LaunchShape s{threads, lds, batches, Cfg::WAVES};
    s.scratch_per_block = wg_bytes;
    s.grid_cap = std::max<long long>(1, (long long)(SCAN_SCRATCH_BUDGET / wg_bytes));
    s.set_lds_attr = false;   // the LDS holds the look-up table alone: far below the limit a kernel has anyway
    s.nomem_what = "SCAN scratch";   // a budget-sized request: out of memory leaves the ctx usable
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), s, &pl);
    if (rc) return rc;
    polar::ScanParams Q = P;
    Q.scratch = pl.scratch;
    Q.queue = pl.queue;
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.grid), dim3(threads), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

}  // namespace

int polar_tu::scan_lanes(polar_ctx *c, const polar::ScanParams &P, bool r32, bool in32)
{
    if (!r32) return in32 ? launch_scan_lanes<double, float>(c, P) : launch_scan_lanes<double, double>(c, P);
    return in32 ? launch_scan_lanes<float, float>(c, P) : launch_scan_lanes<float, double>(c, P);
}
