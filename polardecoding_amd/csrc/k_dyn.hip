// k_dyn.hip -- dynamic frozen bits (scl_dyn.h): k_scl_dyn, k_generate_dyn and their launch code
#include "polar_host.h"
#include "scl_dyn.h"

namespace {

template <typename R, typename IN, int LOGL, bool GA>
int launch_dyn_v(polar_ctx *c, const polar::DynParams &P)
{
    auto kern = polar::k_scl_dyn<R, IN, LOGL, GA>;
    const size_t lds = polar::scl_dyn_lds_bytes<R, LOGL>(P.s.N, GA);
    if (lds > 160 * 1024) return POLAR_ENOKERNEL;
    LaunchShape s{64, lds, P.s.B, 1};
    if (GA) {   // the levels in global scratch: at most 8 blocks per CU
        s.scratch_per_block = sizeof(R) * (size_t)((1 << LOGL) + 1) * P.s.N;
        s.occ_cap = 8;
    }
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), s, &pl);
    if (rc) return rc;
    polar::DynParams Q = P;
    if (GA) Q.s.scratch = pl.scratch;
    Q.s.queue = pl.queue;   // the counter hangs off c->scratch with or without scratch bytes
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(64), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

template <typename R, typename IN, int LOGL>
int launch_dyn(polar_ctx *c, const polar::DynParams &P)
{
    if (polar::scl_dyn_lds_bytes<R, LOGL>(P.s.N, false) <= 160 * 1024 && !c->force_spill)
        return launch_dyn_v<R, IN, LOGL, false>(c, P);
    return launch_dyn_v<R, IN, LOGL, true>(c, P);
}

template <typename R, typename IN>
int launch_dyn_l(polar_ctx *c, const polar::DynParams &P)
{
    switch (c->logL) {
    case 0: return launch_dyn<R, IN, 0>(c, P);
    case 1: return launch_dyn<R, IN, 1>(c, P);
    case 2: return launch_dyn<R, IN, 2>(c, P);
    case 3: return launch_dyn<R, IN, 3>(c, P);
    case 4: return launch_dyn<R, IN, 4>(c, P);
    case 5: return launch_dyn<R, IN, 5>(c, P);
    }
    return POLAR_ENOKERNEL;
}

}  // namespace

int polar_tu::scl_dyn(polar_ctx *c, const polar::SclParams &S, bool r32, bool in32)
{
    polar::DynParams P{};
    P.s = S;
    P.mask = c->d_dyn_mask;
    P.row = c->d_dyn_row;
    if (r32) return in32 ? launch_dyn_l<float, float>(c, P) : launch_dyn_l<float, double>(c, P);
    return in32 ? launch_dyn_l<double, float>(c, P) : launch_dyn_l<double, double>(c, P);
}

int polar_tu::dyn_generate(polar_ctx *c, const polar::GenParams &G)
{
    polar::GenDynParams R{};
    R.g = G;
    R.mask = c->d_dyn_mask;
    R.pos = c->d_dyn_pos;
    R.D = (int)c->dyn_pos.size();
    const int waves = 4;
    const size_t lds = (size_t)waves * (G.N + 2 * 1024);
    const int grid = (int)std::min<size_t>(((size_t)G.B + waves - 1) / waves, (size_t)c->num_cu * 8);
    hipLaunchKernelGGL(polar::k_generate_dyn, dim3(grid), dim3(64 * waves), lds, c->stream, R);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
