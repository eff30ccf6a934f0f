// k_genie.hip -- Monte-Carlo code construction kernels (genie_lanes.h) and their launch code
#include "polar_host.h"
#include "genie_lanes.h"

namespace {

template <typename R, typename IN>
int launch_genie_lanes(polar_ctx *c, const polar::GenieParams &P)
{
    using Cfg = polar::GenieCfg<R>;
    auto kern = polar::k_genie_lanes<R, IN>;
    const size_t lds = Cfg::lds_bytes(P.N);
    const int threads = 64 * Cfg::WAVES;
    const long long batches = ((long long)P.B + 63) / 64;
    LaunchShape s{threads, lds, batches, Cfg::WAVES};
    s.scratch_per_block = Cfg::scratch_bytes(P.N) * Cfg::WAVES;
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), s, &pl);
    if (rc) return rc;
    polar::GenieParams Q = P;
    Q.scratch = pl.scratch;
    Q.queue = pl.queue;
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(threads), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

}  // namespace

int polar_tu::genie_count(polar_ctx *c, const void *d_in, bool in32, double sigma, size_t B, unsigned long long *d_counts)
{
    if (B == 0) return POLAR_OK;
    // a workgroup's uint32 counters in LDS cannot wrap: it sees fewer than 2^32 frames in one launch
    if (B > 0x7fffffffull) return POLAR_EINVAL;
    polar::GenieParams P{};
    P.in = d_in; P.sigma = sigma; P.counts = d_counts;
    P.N = c->cfg.N; P.n = c->n; P.B = (int)B;
    const bool r32 = c->cfg.dtype == POLAR_F32;
    if (!r32) return in32 ? launch_genie_lanes<double, float>(c, P) : launch_genie_lanes<double, double>(c, P);
    return in32 ? launch_genie_lanes<float, float>(c, P) : launch_genie_lanes<float, double>(c, P);
}

int polar_tu::genie_rows(polar_ctx *c, unsigned long long seed, unsigned long long first_frame, double sigma, size_t B,
                         void *d_out, bool out32)
{
    if (B == 0) return POLAR_OK;
    polar::GenieRowsParams P{};
    P.out = d_out; P.seed = seed; P.first_frame = first_frame; P.sigma = sigma;
    P.N = c->cfg.N; P.B = (int)B;
    const size_t pairs = B * (size_t)(P.N / 2);
    const int grid = stride_grid(c, (long long)((pairs + 255) / 256), (long long)c->num_cu * 16);
    if (out32) hipLaunchKernelGGL(polar::k_genie_rows<float>, dim3(grid), dim3(256), 0, c->stream, P);
    else hipLaunchKernelGGL(polar::k_genie_rows<double>, dim3(grid), dim3(256), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
