// k_big_launch.h -- launch code of k_scl_big shared by k_big_f32.hip and k_big_f64.hip (one translation unit per
// arithmetic type, compiled in parallel); each defines launch_big() with the splits that measured best for its type
#pragma once
#include "polar_host.h"
#include "scl_big.h"

namespace {

// big lists / long codes: low LLR levels in LDS, the rest in a per-wave scratch slice (scl_big.h)
template <typename R, typename IN, int LOGL, int TL, int TB, int RL = 0, int CH = 0>
int launch_big_v(polar_ctx *c, const polar::SclParams &P)
{
    using Cfg = polar::BigCfg<R, LOGL, TL, TB, RL>;
    auto kern = polar::k_scl_big<R, IN, LOGL, TL, TB, RL, CH>;
    const size_t lds = Cfg::lds_bytes;
    const int threads = 64 * Cfg::WAVES;
    LaunchShape s{threads, lds, P.B, Cfg::WAVES};
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

template <typename R, typename IN, int LOGL>
int launch_big(polar_ctx *c, const polar::SclParams &P);   // the including translation unit's choice of split

template <typename R, typename IN>
int launch_big_l(polar_ctx *c, const polar::SclParams &P)
{
    switch (c->logL) {
    case 1: return launch_big<R, IN, 1>(c, P);
    case 2: return launch_big<R, IN, 2>(c, P);
    case 3: return launch_big<R, IN, 3>(c, P);
    case 4: return launch_big<R, IN, 4>(c, P);
    case 5: return launch_big<R, IN, 5>(c, P);
    }
    return POLAR_ENOKERNEL;
}

}  // namespace
