// k_bp.hip -- flooding BP: k_bp_r4 (N = 1024), k_bp / k_bp_global (other N), k_bp_readout (BPr) and their launch code
#include "polar_host.h"
#include "bp_kernel.h"
#include "bp_r4.h"
#include "bp_w128.h"

namespace {

// N = 1024: the register-blocked kernel (bp_r4.h), three f64 codewords per CU; P.stop: its stop-rule instantiation
template <typename R, typename IN>
int launch_bp_r4(polar_ctx *c, const polar::BpParams &P)
{
    using Cfg = polar::BpR4Cfg<R>;
    auto kern = P.stop ? polar::k_bp_r4<R, IN, true> : polar::k_bp_r4<R, IN>;
    const size_t lds = P.stop ? Cfg::lds_bytes_stop : Cfg::lds_bytes;
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), LaunchShape{Cfg::THREADS, lds, P.B, 1}, &pl);
    if (rc) return rc;
    polar::BpParams Q = P;
    Q.queue = pl.queue;
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(Cfg::THREADS), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

// N = 128: one codeword per wavefront, every message in registers (bp_w128.h)
template <typename R, typename IN>
int launch_bp_w128(polar_ctx *c, const polar::BpParams &P)
{
    using Cfg = polar::BpW128Cfg<R>;
    auto kern = P.stop ? polar::k_bp_w128<R, IN, true> : polar::k_bp_w128<R, IN>;
    const size_t lds = Cfg::lds_bytes;
    LaunchShape s{64 * Cfg::WAVES, lds, P.B, Cfg::WAVES};
    s.set_lds_attr = false;   // the LDS holds the tables alone: far below the limit a kernel has anyway
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), s, &pl);
    if (rc) return rc;
    polar::BpParams Q = P;
    Q.queue = pl.queue;
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(64 * Cfg::WAVES), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

template <typename R, typename IN>
int launch_bp(polar_ctx *c, const polar::BpParams &P)
{
    const int variant = polar_tu::bp_variant(c);
    if (variant == polar_tu::BP_R4) return launch_bp_r4<R, IN>(c, P);
    if (variant == polar_tu::BP_W128) return launch_bp_w128<R, IN>(c, P);
    const bool stop = P.stop != 0;
    auto kern = stop ? polar::k_bp<R, IN, true> : polar::k_bp<R, IN>;
    const size_t lds = polar::bp_lds_bytes<R>(P.N, P.n, stop);
    if (lds > 160 * 1024) {   // messages do not fit a CU's LDS: rows in global scratch
        auto kg = stop ? polar::k_bp_global<R, IN, true> : polar::k_bp_global<R, IN>;
        const size_t lds_g = 4 * (size_t)(P.N / 32) * (stop ? 2 : 1) + (stop ? 16 : 0) + 16 + polar::Lut<R>::bytes;
        const int grid = stride_grid(c, P.B, (long long)2 * c->num_cu);
        record_plan(c, grid, P.B, 1, false);
        int rc = ensure(c, c->scratch, sizeof(R) * 2 * (size_t)(P.n + 1) * P.N * (size_t)grid);
        if (rc) return rc;
        hipLaunchKernelGGL(kg, dim3(grid), dim3(512), lds_g, c->stream, P, reinterpret_cast<R *>(c->scratch.p));
        HIP_TRY(c, hipGetLastError());
        return POLAR_OK;
    }
    const int threads = std::max(64, std::min(512, P.N / 2));
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), LaunchShape{threads, lds, P.B, 1}, &pl);
    if (rc) return rc;
    polar::BpParams Q = P;
    Q.queue = pl.queue;
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(threads), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

template <typename R, typename IN>
int launch_bp_readout(polar_ctx *c, const polar::BpReadoutParams &P)
{
    auto kern = polar::k_bp_readout<R, IN>;
    const size_t lds = polar::bp_readout_lds_bytes<R>(P.N, P.n);
    if (lds > 160 * 1024) return POLAR_ENOKERNEL;
    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    const int threads = std::max(64, std::min(256, P.N / 2));
    int occ = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, threads, lds));
    if (occ < 1) occ = 1;
    const int grid = stride_grid(c, P.B, (long long)occ * c->num_cu);
    record_plan(c, grid, P.B, 1, false);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

}  // namespace

int polar_tu::bp_variant(const polar_ctx *c)
{
    if (c->cfg.N == 1024 && !c->force_generic) return BP_R4;
    if (c->cfg.N == 128 && !c->force_generic) return BP_W128;
    return BP_PLAIN;
}

int polar_tu::bp(polar_ctx *c, const polar::BpParams &P, bool r32, bool in32)
{
    if (r32) return in32 ? launch_bp<float, float>(c, P) : launch_bp<float, double>(c, P);
    return in32 ? launch_bp<double, float>(c, P) : launch_bp<double, double>(c, P);
}

int polar_tu::bp_readout(polar_ctx *c, const polar::BpReadoutParams &P, bool r32, bool in32)
{
    if (r32) return in32 ? launch_bp_readout<float, float>(c, P) : launch_bp_readout<float, double>(c, P);
    return in32 ? launch_bp_readout<double, float>(c, P) : launch_bp_readout<double, double>(c, P);
}
