// k_dyn.hip -- dynamic frozen bits: k_scl_dyn (scl_dyn.h), k_generate_dyn (gen_dyn.h) and their launch code
#include "gen_dyn.h"
#include "k_scl_launch.h"
#include "scl_dyn.h"

namespace {

struct DynKernel {
    using Params = polar::DynParams;
    template <typename R, typename IN, int LOGL, bool GA>
    static auto kernel() { return polar::k_scl_dyn<R, IN, LOGL, GA>; }
    template <typename R, int LOGL>
    static constexpr size_t lds_bytes(int N, bool ga) { return polar::scl_dyn_lds_bytes<R, LOGL>(N, ga); }
    static polar::SclParams &scl(Params &P) { return P.s; }
};

}  // namespace

int polar_tu::scl_dyn(polar_ctx *c, const polar::SclParams &S, bool r32, bool in32)
{
    polar::DynParams P{};
    P.s = S;
    P.mask = c->d_dyn_mask;
    P.row = c->d_dyn_row;
    return launch_scl_types<DynKernel>(c, P, r32, in32);
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
    const int grid = stride_grid(c, ((long long)G.B + waves - 1) / waves, (long long)c->num_cu * 8);
    hipLaunchKernelGGL(polar::k_generate_dyn, dim3(grid), dim3(64 * waves), lds, c->stream, R);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
