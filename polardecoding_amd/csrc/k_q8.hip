// k_q8.hip -- fixed-point min-sum decoding (POLAR_Q8): k_scl_q8, the quantiser and their launch code (scl_q8.h)
#include "polar_host.h"
#include "scl_q8.h"

namespace {

template <int LOGL>
int launch_q8(polar_ctx *c, polar::Q8Params P)
{
    auto kern = polar::k_scl_q8<LOGL>;
    LaunchShape s{64, polar::scl_q8_lds_bytes<LOGL>(P.N), P.B, 1};
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), s, &pl);
    if (rc) return rc;
    P.queue = pl.queue;
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(64), s.lds, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

}  // namespace

int polar_tu::q8_decode(polar_ctx *c, const int8_t *d_q, size_t B, uint32_t *d_bits, int32_t *d_pm, uint32_t *d_flags)
{
    polar::Q8Params P{};
    P.in = d_q; P.out_bits = d_bits; P.pm = d_pm; P.flags = d_flags;
    P.frozen = c->d_frozen;
    P.crc_tab = (c->cfg.algo == POLAR_ALGO_CASCL) ? c->d_crc_tab : nullptr;
    P.N = c->cfg.N; P.n = c->n; P.B = (int)B;
    P.sc_mode = (c->cfg.algo == POLAR_ALGO_SC) ? 1 : 0;
    P.Cc = (1 << (c->q8_qc - 1)) - 1;
    P.Ci = (1 << (c->q8_qi - 1)) - 1;
    switch (c->logL) {
    case 0: return launch_q8<0>(c, P);
    case 1: return launch_q8<1>(c, P);
    case 2: return launch_q8<2>(c, P);
    case 3: return launch_q8<3>(c, P);
    case 4: return launch_q8<4>(c, P);
    case 5: return launch_q8<5>(c, P);
    }
    return POLAR_ENOKERNEL;
}

int polar_tu::q8_quantize(polar_ctx *c, const void *d_in, bool in32, double sigma, size_t count, int8_t *d_out)
{
    if (count == 0) return POLAR_OK;
    const unsigned grid = (unsigned)((count + 255) / 256);
    const int Cc = (1 << (c->q8_qc - 1)) - 1;
    if (in32)
        hipLaunchKernelGGL(polar::k_q8_quantize<float>, dim3(grid), dim3(256), 0, c->stream, (const float *)d_in, d_out, count, sigma,
                           c->q8_scale, Cc);
    else
        hipLaunchKernelGGL(polar::k_q8_quantize<double>, dim3(grid), dim3(256), 0, c->stream, (const double *)d_in, d_out, count, sigma,
                           c->q8_scale, Cc);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::q8_pm_f64(polar_ctx *c, const int32_t *d_pm, size_t B, double *d_out)
{
    if (B == 0) return POLAR_OK;
    hipLaunchKernelGGL(polar::k_q8_pm_f64, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, d_pm, d_out, B);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

void polar_tu::q8_quantize_host(const double *in, size_t n, double sigma, double scale, int Cc, int8_t *out)
{
    for (size_t i = 0; i < n; ++i) {
        double v = in[i];
        if (sigma > 0) v = 2 * v / sigma / sigma;
        out[i] = polar::q8_round_clamp(v * scale, Cc);
    }
}
