// k_scf.hip -- k_scf_lanes (CRC-aided SC-Flip, scf_lanes.h), k_scf_resolve(_sets), k_scf_merge and their launch code
#include "polar_host.h"
#include "scf_lanes.h"

namespace {

template <typename R, typename IN, int MODE>
int launch_scf_lanes(polar_ctx *c, const polar::ScfParams &P)
{
    using Cfg = polar::ScfCfg<R>;
    auto kern = polar::k_scf_lanes<R, IN, MODE>;
    int waves = Cfg::WAVES;
    const int lt = MODE >= polar::SCF_RECORD_M ? P.Tn : P.T;   // the list a recording policy keeps in LDS
    while (waves > 1 && Cfg::lds_bytes(P.N, lt, MODE, waves) > (size_t)160 * 1024) waves /= 2;
    const size_t lds = Cfg::lds_bytes(P.N, lt, MODE, waves);
    if (lds > (size_t)160 * 1024) return POLAR_ENOKERNEL;
    const int threads = 64 * waves;
    const long long batches = ((long long)P.B + 63) / 64;
    LaunchShape s{threads, lds, batches, waves};
    s.scratch_per_block = polar::ScLanesCfg<R>::scratch_bytes(P.N) * waves;
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), s, &pl);
    if (rc) return rc;
    polar::ScfParams Q = P;
    Q.scratch = pl.scratch;
    Q.queue = pl.queue;
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(threads), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

template <int MODE>
int launch_mode(polar_ctx *c, const polar::ScfParams &P, bool r32, bool in32)
{
    if (!r32) return in32 ? launch_scf_lanes<double, float, MODE>(c, P) : launch_scf_lanes<double, double, MODE>(c, P);
    return in32 ? launch_scf_lanes<float, float, MODE>(c, P) : launch_scf_lanes<float, double, MODE>(c, P);
}

}  // namespace

int polar_tu::scf_lanes(polar_ctx *c, const polar::ScfParams &P, int mode, bool r32, bool in32)
{
    if (P.B <= 0) return POLAR_OK;
    if (mode == polar::SCF_CHECK) return launch_mode<polar::SCF_CHECK>(c, P, r32, in32);
    if (mode == polar::SCF_RECORD) return launch_mode<polar::SCF_RECORD>(c, P, r32, in32);
    if (mode == polar::SCF_RECORD_M) return launch_mode<polar::SCF_RECORD_M>(c, P, r32, in32);
    if (mode == polar::SCF_FLIPSET) return launch_mode<polar::SCF_FLIPSET>(c, P, r32, in32);
    if (mode == polar::SCF_FLIPREC) return launch_mode<polar::SCF_FLIPREC>(c, P, r32, in32);
    return launch_mode<polar::SCF_FLIP>(c, P, r32, in32);
}

int polar_tu::scf_resolve(polar_ctx *c, const uint32_t *d_pass, const uint32_t *d_pbits, const uint32_t *d_idx, size_t n,
                          int T, uint32_t *d_bits, uint32_t *d_flags, uint32_t *d_attempts)
{
    if (n == 0) return POLAR_OK;
    int lw = 0;
    while ((1 << lw) < c->NW) ++lw;
    const long long items = (long long)n << lw;
    const int grid = stride_grid(c, (items + 255) / 256, (long long)c->num_cu * 16);
    hipLaunchKernelGGL(polar::k_scf_resolve, dim3(grid), dim3(256), 0, c->stream, d_pass, d_pbits, d_idx, (long long)n, T, lw,
                       d_bits, d_flags, d_attempts);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::scf_resolve_sets(polar_ctx *c, const uint32_t *d_pass, const uint32_t *d_pbits, const uint32_t *d_idx, size_t n,
                               int T, const uint16_t *d_sets_in, int stride, int width, int base, uint32_t *d_bits,
                               uint32_t *d_flags, uint32_t *d_attempts, int32_t *d_sets, uint32_t *d_slot_pass)
{
    if (n == 0) return POLAR_OK;
    int lw = 0;
    while ((1 << lw) < c->NW) ++lw;
    const long long items = (long long)n << lw;
    const int grid = stride_grid(c, (items + 255) / 256, (long long)c->num_cu * 16);
    hipLaunchKernelGGL(polar::k_scf_resolve_sets, dim3(grid), dim3(256), 0, c->stream, d_pass, d_pbits, d_idx, (long long)n, T,
                       lw, d_sets_in, stride, width, base, d_bits, d_flags, d_attempts, d_sets, d_slot_pass);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::scf_merge(polar_ctx *c, bool r32, const void *d_lkey, const uint16_t *d_lpos, const uint32_t *d_lcnt,
                        const uint16_t *d_psets, const uint32_t *d_surv, const uint32_t *d_idx_in, size_t n, int Tk, int Tn,
                        uint16_t *d_out_sets, uint32_t *d_idx_out)
{
    if (n == 0) return POLAR_OK;
    const int grid = stride_grid(c, ((long long)n + 255) / 256, (long long)c->num_cu * 16);
    if (r32)
        hipLaunchKernelGGL(polar::k_scf_merge<float>, dim3(grid), dim3(256), 0, c->stream, (const float *)d_lkey, d_lpos, d_lcnt,
                           d_psets, d_surv, d_idx_in, (long long)n, Tk, Tn, d_out_sets, d_idx_out);
    else
        hipLaunchKernelGGL(polar::k_scf_merge<double>, dim3(grid), dim3(256), 0, c->stream, (const double *)d_lkey, d_lpos,
                           d_lcnt, d_psets, d_surv, d_idx_in, (long long)n, Tk, Tn, d_out_sets, d_idx_out);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
