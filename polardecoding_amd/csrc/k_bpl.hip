// k_bpl.hip -- launch code of the BP list decoder's glue kernels (bpl_kernel.h)
#include "bpl_kernel.h"
#include "polar_host.h"

namespace {

int grid_for(polar_ctx *c, long long items)
{
    const long long blocks = (items + polar::BPL_THREADS - 1) / polar::BPL_THREADS;
    return stride_grid(c, blocks, (long long)c->num_cu * 16);
}

}  // namespace

// rows idx[k] (idx null: base + k) of d_src, permuted by d_sigma ([N] uint16, null: identity) -> d_dst[0..n)
int polar_tu::bpl_gather(polar_ctx *c, const void *d_src, bool in32, void *d_dst, const uint32_t *d_idx, size_t base,
                         const uint16_t *d_sigma, size_t n)
{
    if (n == 0) return POLAR_OK;
    const int lr = c->n;
    const int grid = grid_for(c, (long long)n << lr);
    if (in32)
        hipLaunchKernelGGL(polar::k_bpl_gather<float>, dim3(grid), dim3(polar::BPL_THREADS), 0, c->stream, (const float *)d_src,
                           (float *)d_dst, d_idx, (long long)base, d_sigma, (long long)n, lr);
    else
        hipLaunchKernelGGL(polar::k_bpl_gather<double>, dim3(grid), dim3(polar::BPL_THREADS), 0, c->stream, (const double *)d_src,
                           (double *)d_dst, d_idx, (long long)base, d_sigma, (long long)n, lr);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::bpl_scatter(polar_ctx *c, const uint32_t *s_bits, const uint32_t *s_iters, const uint32_t *s_flags,
                          const uint32_t *d_idx, size_t base, size_t n, const uint16_t *d_sinv, uint32_t need, int p, int P,
                          bool all, uint32_t *d_bits, uint32_t *d_iters, uint32_t *d_flags, uint32_t *d_graph,
                          uint32_t *d_total)
{
    if (n == 0) return POLAR_OK;
    int lw = 0;
    while ((1 << lw) < c->NW) ++lw;
    const long long items = s_bits ? (long long)n << lw : (long long)n;
    hipLaunchKernelGGL(polar::k_bpl_scatter, dim3(grid_for(c, items)), dim3(polar::BPL_THREADS), 0, c->stream, s_bits, s_iters,
                       s_flags, d_idx, (long long)base, (long long)n, lw, d_sinv, need, (uint32_t)p, (uint32_t)P, all ? 1 : 0,
                       d_bits, d_iters, d_flags, d_graph, d_total);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
