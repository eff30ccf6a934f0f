// k_enc.hip -- the encoder-side kernels (enc_kernel.h) and their launch code
#include "polar_host.h"
#include "enc_kernel.h"

namespace {

// one lane per packed word (N = 4096: per two), ENC_THREADS lanes per workgroup
unsigned enc_grid(const polar_ctx *c, size_t B)
{
    const size_t lanes = B << polar::enc_log_group(c->NW);
    return (unsigned)((lanes + polar::ENC_THREADS - 1) / polar::ENC_THREADS);
}

void crc_taps_of(const polar_ctx *c, uint32_t *mask, uint32_t *top)
{
    *mask = c->cfg.crc_r == 0 ? 1u : 0u;
    *top = 0;
    for (int t : c->taps) {
        if (t < 32) *mask |= 1u << t;
        else *top = 1u;
    }
}

}  // namespace

int polar_tu::enc_transform(polar_ctx *c, const uint32_t *d_in, const uint32_t *d_in2, bool clear_frozen, size_t B,
                            uint32_t *d_out)
{
    if (B == 0) return POLAR_OK;
    polar::XformParams P{d_in, d_in2, clear_frozen ? c->d_frozen : nullptr, d_out, c->NW, (int)B};
    if (c->NW == 128) hipLaunchKernelGGL(polar::k_transform<2>, dim3(enc_grid(c, B)), dim3(polar::ENC_THREADS), 0, c->stream, P);
    else hipLaunchKernelGGL(polar::k_transform<1>, dim3(enc_grid(c, B)), dim3(polar::ENC_THREADS), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::enc_count_sys(polar_ctx *c, const uint32_t *d_uhat, const uint32_t *d_u, size_t B, unsigned long long *d_counters,
                            uint32_t *d_frame_err)
{
    if (B == 0) return POLAR_OK;
    polar::CountSysParams P{d_uhat, d_u, c->d_info, d_counters, d_frame_err, c->NW, (int)B};
    if (c->NW == 128) hipLaunchKernelGGL(polar::k_count_sys<2>, dim3(enc_grid(c, B)), dim3(polar::ENC_THREADS), 0, c->stream, P);
    else hipLaunchKernelGGL(polar::k_count_sys<1>, dim3(enc_grid(c, B)), dim3(polar::ENC_THREADS), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::enc_place(polar_ctx *c, const uint32_t *d_payload, size_t B, uint32_t *d_z)
{
    if (B == 0) return POLAR_OK;
    polar::PlaceParams P{};
    P.payload = d_payload; P.z = d_z; P.inv = c->d_enc_inv; P.rtab = c->d_enc_rtab;
    crc_taps_of(c, &P.crc_mask, &P.crc_top);
    P.crc_r = c->cfg.crc_r; P.crc_sys = c->cfg.crc_systematic;
    P.N = c->cfg.N; P.K = c->cfg.K; P.A = c->A; P.B = (int)B;
    hipLaunchKernelGGL(polar::k_place, dim3(enc_grid(c, B)), dim3(polar::ENC_THREADS), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::enc_extract(polar_ctx *c, const uint32_t *d_z, bool xform, size_t B, uint32_t *d_payload, uint32_t *d_ok)
{
    if (B == 0) return POLAR_OK;
    polar::ExtractParams P{};
    P.z = d_z; P.payload = d_payload; P.ok = d_ok; P.info_order = c->d_info_order; P.rtab = c->d_enc_rtab;
    crc_taps_of(c, &P.crc_mask, &P.crc_top);
    P.crc_r = c->cfg.crc_r; P.crc_sys = c->cfg.crc_systematic; P.xform = xform ? 1 : 0;
    P.N = c->cfg.N; P.K = c->cfg.K; P.A = c->A; P.B = (int)B;
    hipLaunchKernelGGL(polar::k_extract, dim3(enc_grid(c, B)), dim3(polar::ENC_THREADS), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::enc_dyn_fill(polar_ctx *c, uint32_t *d_z, size_t B)
{
    if (B == 0 || c->dyn_pos.empty()) return POLAR_OK;
    if (c->NW > 64) return POLAR_ENOKERNEL;   // dynamic contexts end at N = 1024: one word per lane
    polar::DynFillParams P{d_z, c->d_dyn_mask, c->d_dyn_pos, (int)c->dyn_pos.size(), c->NW, (int)B};
    hipLaunchKernelGGL(polar::k_dyn_fill, dim3(enc_grid(c, B)), dim3(polar::ENC_THREADS), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_tu::enc_rm_select(polar_ctx *c, const uint32_t *d_x, size_t B, uint32_t *d_e)
{
    if (B == 0) return POLAR_OK;
    polar::RmSelectParams P{};
    P.x = d_x; P.e = d_e; P.ilv_inv = c->rm_ibil ? c->d_rm_ilv_inv : nullptr;
    P.N = c->cfg.N; P.E = c->rm_E; P.mode = c->rm_mode; P.B = (int)B;
    P.logS = 0;
    while ((32 << P.logS) < P.N) ++P.logS;
    const size_t words = B * (size_t)((c->rm_E + 31) / 32);
    hipLaunchKernelGGL(polar::k_rm_select, dim3((unsigned)((words + polar::ENC_THREADS - 1) / polar::ENC_THREADS)),
                       dim3(polar::ENC_THREADS), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
