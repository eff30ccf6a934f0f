// k_adaptive.hip -- launch code of the adaptive CA-SCL glue kernels (adaptive_kernel.h)
#include "adaptive_kernel.h"
#include "polar_host.h"

namespace {

int grid_for(polar_ctx *c, long long items)
{
    const long long blocks = (items + polar::AD_THREADS - 1) / polar::AD_THREADS;
    return stride_grid(c, blocks, (long long)c->num_cu * 16);
}

int log2i(long long v)
{
    int l = 0;
    while ((1ll << l) < v) ++l;
    return l;
}

}  // namespace

int polar_tu::ad_crc_check(polar_ctx *c, const uint32_t *d_bits, const uint32_t *d_crc_tab, uint32_t *d_flags, size_t B)
{
    const int NW = c->NW;
    const int G = NW < 64 ? NW : 64;
    const long long waves = ((long long)B * G + 63) / 64;
    const int grid = grid_for(c, waves * 64);
    const size_t lds = sizeof(uint32_t) * (size_t)NW * 32;
    hipLaunchKernelGGL(polar::k_ad_crc_check, dim3(grid), dim3(polar::AD_THREADS), lds, c->stream, d_bits, d_crc_tab,
                       d_flags, NW, (int)B);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

size_t polar_tu::ad_blocks(size_t n) { return (n + polar::AD_CHUNK - 1) / polar::AD_CHUNK; }

int polar_tu::ad_compact(polar_ctx *c, const uint32_t *d_flags, const uint32_t *d_idx_in, size_t n, uint32_t need,
                         uint32_t *d_blk, uint32_t *d_idx_out, uint32_t *d_count)
{
    const int nblk = (int)ad_blocks(n);
    uint32_t *blk_cnt = d_blk, *blk_off = d_blk + nblk;
    hipLaunchKernelGGL(polar::k_ad_fail_count, dim3(nblk), dim3(polar::AD_THREADS), 0, c->stream, d_flags, (int)n, need,
                       blk_cnt);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(polar::k_ad_fail_scan, dim3(1), dim3(polar::AD_SCAN_THREADS), 0, c->stream, blk_cnt, nblk, blk_off,
                       d_count);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(polar::k_ad_fail_write, dim3(nblk), dim3(polar::AD_THREADS), 0, c->stream, d_flags, d_idx_in, (int)n,
                       need, blk_off, d_idx_out);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::ad_gather(polar_ctx *c, const void *d_src, void *d_dst, const uint32_t *d_idx, size_t n, size_t row_bytes)
{
    if (n == 0) return POLAR_OK;
    // row_bytes = N * 4 or N * 8 with N a power of two >= 32: a multiple of 16
    const bool wide = ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 15) == 0;
    if (wide) {
        const int lr = log2i((long long)(row_bytes / 16));
        hipLaunchKernelGGL(polar::k_ad_gather<uint4>, dim3(grid_for(c, (long long)n << lr)), dim3(polar::AD_THREADS), 0,
                           c->stream, (const uint4 *)d_src, (uint4 *)d_dst, d_idx, (long long)n, lr);
    } else {
        const int lr = log2i((long long)(row_bytes / 4));
        hipLaunchKernelGGL(polar::k_ad_gather<uint32_t>, dim3(grid_for(c, (long long)n << lr)), dim3(polar::AD_THREADS), 0,
                           c->stream, (const uint32_t *)d_src, (uint32_t *)d_dst, d_idx, (long long)n, lr);
    }
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::ad_scatter(polar_ctx *c, const uint32_t *s_bits, const double *s_pm, const uint32_t *s_flags,
                         const uint32_t *d_idx, size_t n, uint32_t *d_bits, double *d_pm, uint32_t *d_flags, uint32_t *d_list,
                         int L)
{
    if (n == 0) return POLAR_OK;
    const int lw = log2i(c->NW);
    hipLaunchKernelGGL(polar::k_ad_scatter, dim3(grid_for(c, (long long)n << lw)), dim3(polar::AD_THREADS), 0, c->stream,
                       s_bits, s_pm, s_flags, d_idx, (long long)n, lw, d_bits, d_pm, d_flags, d_list, (uint32_t)L);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
