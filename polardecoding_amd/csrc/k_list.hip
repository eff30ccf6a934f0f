// k_list.hip -- list output (include/polar_hip.h, "List output"): the LIST instantiations of scl_generic_body (k_scl_list)
// and k_scl_wide, k_list_select, k_list_gather, k_list_soft (list_kernel.h) and their launch code
#include "k_scl_launch.h"
#include "list_kernel.h"

namespace {

struct ListKernel {
    using Params = polar::ListParams;
    template <typename R, typename IN, int LOGL, bool GA>
    static auto kernel() { return polar::k_scl_list<R, IN, LOGL, GA>; }
    template <typename R, int LOGL>
    static constexpr size_t lds_bytes(int N, bool ga) { return polar::scl_dyn_lds_bytes<R, LOGL>(N, ga); }
    static polar::SclParams &scl(Params &P) { return P.d.s; }
};

struct WideListKernel {
    using Params = polar::ListParams;
    template <typename R, typename IN, int LOGL, bool GA>
    static auto kernel() { return polar::k_scl_wide<R, IN, LOGL, GA, true, true>; }
    template <typename R, int LOGL>
    static constexpr size_t lds_bytes(int N, bool ga) { return polar::WideLds<R, LOGL, true>::bytes(N, ga); }
    static polar::SclParams &scl(Params &P) { return P.d.s; }
};

template <typename R, typename IN>
int launch_list_l(polar_ctx *c, const polar::ListParams &P)
{
    switch (c->logL) {
    case 6: return launch_scl<WideListKernel, R, IN, 6>(c, P);
    case 7: return launch_scl<WideListKernel, R, IN, 7>(c, P);
    case 8: return launch_scl<WideListKernel, R, IN, 8>(c, P);
    }
    return launch_scl_l<ListKernel, R, IN>(c, P);
}

int blocks_of(size_t total, int threads) { return (int)((total + threads - 1) / threads); }

}  // namespace

int polar_tu::list_decode(polar_ctx *c, const polar::SclParams &S, const uint32_t *d_mask, const int *d_row, bool r32, bool in32,
                          uint32_t *d_paths, double *d_pm, uint32_t *d_rem, uint32_t *d_count)
{
    if ((long long)c->logL * c->n > 64) return POLAR_ENOKERNEL;   // the 64-bit pointer table holds LOGL bits per level
    polar::ListParams P{};
    P.d.s = S;
    P.d.mask = d_mask;
    P.d.row = d_row;
    P.o = polar::ListOut{d_paths, d_pm, d_rem, d_count};
    if (r32) return in32 ? launch_list_l<float, float>(c, P) : launch_list_l<float, double>(c, P);
    return in32 ? launch_list_l<double, float>(c, P) : launch_list_l<double, double>(c, P);
}

int polar_tu::list_select(polar_ctx *c, const uint32_t *d_rem, const uint32_t *d_count, size_t B, const uint32_t *d_masks, int M,
                          int32_t *d_idx)
{
    const size_t total = B * (size_t)M;
    hipLaunchKernelGGL(polar::k_list_select, dim3(blocks_of(total, 256)), dim3(256), 0, c->stream, d_rem, d_count, d_masks, c->cfg.L,
                       M, total, d_idx);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::list_gather(polar_ctx *c, const uint32_t *d_paths, const int32_t *d_idx, int idx_stride, size_t B, uint32_t *d_out)
{
    const size_t total = B * (size_t)c->NW;
    hipLaunchKernelGGL(polar::k_list_gather, dim3(blocks_of(total, 256)), dim3(256), 0, c->stream, d_paths, d_idx, idx_stride,
                       c->cfg.L, c->NW, total, d_out);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::list_soft(polar_ctx *c, const uint32_t *d_paths, const double *d_pm, const uint32_t *d_count, const uint32_t *d_rem,
                        uint32_t want_rem, int domain, double clamp, size_t B, double *d_out)
{
    polar::ListSoftParams P{};
    P.paths = d_paths; P.pm = d_pm; P.count = d_count; P.rem = d_rem;
    P.want_rem = want_rem; P.domain = domain; P.clamp = clamp;
    P.N = c->cfg.N; P.n = c->n; P.L = c->cfg.L; P.B = (int)B;
    P.out = d_out;
    const size_t lds = polar::list_soft_lds_bytes(P.N, P.L);
    LaunchShape s{64, lds, P.B, 1};
    s.use_queue = false;   // frames by a fixed stride
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(polar::k_list_soft), s, &pl);
    if (rc) return rc;
    hipLaunchKernelGGL(polar::k_list_soft, dim3(pl.grid), dim3(64), lds, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
