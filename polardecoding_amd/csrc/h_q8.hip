// h_q8.hip -- the entry points of fixed-point min-sum decoding (POLAR_Q8).
#include "polar_hostlib.h"

using namespace polar_host;

extern "C" {

// ---- fixed-point min-sum decoding (include/polar_hip.h, POLAR_Q8) ---------------------------------------------------------
static bool q8_quant_ok(double scale, int qc, int qi) { return scale > 0 && std::isfinite(scale) && qc >= 2 && qc <= qi && qi <= 8; }

int polar_q8_set_quant(polar_ctx *c, double scale, int qc, int qi)
{
    if (!c || c->cfg.dtype != POLAR_Q8 || !q8_quant_ok(scale, qc, qi)) return POLAR_EINVAL;
    c->q8_scale = scale;
    c->q8_qc = qc;
    c->q8_qi = qi;
    return POLAR_OK;
}

int polar_q8_get_quant(const polar_ctx *c, double *scale, int *qc, int *qi)
{
    if (!c || c->cfg.dtype != POLAR_Q8) return POLAR_EINVAL;
    if (scale) *scale = c->q8_scale;
    if (qc) *qc = c->q8_qc;
    if (qi) *qi = c->q8_qi;
    return POLAR_OK;
}

int polar_q8_quantize_host(const double *in, size_t n, double sigma, double scale, int qc, int8_t *out)
{
    if ((n && (!in || !out)) || !q8_quant_ok(scale, qc, 8) || sigma != sigma) return POLAR_EINVAL;
    polar_tu::q8_quantize_host(in, n, sigma, scale, (1 << (qc - 1)) - 1, out);
    return POLAR_OK;
}

int polar_q8_quantize_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, int8_t *d_out)
{
    if (!c || c->cfg.dtype != POLAR_Q8 || !d_in || !d_out || B > kMaxBatch) return POLAR_EINVAL;
    const size_t esz = in_is_f32 ? 4 : 8;
    if (reinterpret_cast<uintptr_t>(d_in) % esz) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    const size_t total = B * (size_t)c->cfg.N, CH = (size_t)1 << 30;   // elements per launch
    for (size_t off = 0; off < total; off += CH) {
        const int rc = polar_tu::q8_quantize(c, (const char *)d_in + off * esz, in_is_f32 != 0, sigma, std::min(CH, total - off), d_out + off);
        if (rc) return rc;
    }
    return POLAR_OK;
}

int polar_q8_decode_device(polar_ctx *c, const int8_t *d_q, size_t B, uint32_t *d_uhat_bits, int32_t *d_pm, uint32_t *d_flags)
{
    if (!c || c->cfg.dtype != POLAR_Q8 || !d_q || !d_uhat_bits || B > kMaxBatch) return POLAR_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_q) % 4) return POLAR_EINVAL;   // the kernel loads the rows as dwords
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    return polar_tu::q8_decode(c, d_q, B, d_uhat_bits, d_pm, d_flags);
}

int polar_q8_decode_batch(polar_ctx *c, const int8_t *q, size_t B, int *u_hat, int32_t *pm, unsigned *flags)
{
    if (!c || c->cfg.dtype != POLAR_Q8 || !q || !u_hat || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    const size_t N = (size_t)c->cfg.N, NW = (size_t)c->NW;
    int rc;
    if ((rc = ensure(c, c->q8_rows, B * N))) return rc;
    if ((rc = ensure(c, c->bits, B * NW * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->q8_pm, B * sizeof(int32_t)))) return rc;
    if ((rc = ensure(c, c->flags, B * sizeof(uint32_t)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->q8_rows.p, q, B * N, hipMemcpyHostToDevice, c->stream));
    if ((rc = polar_tu::q8_decode(c, (const int8_t *)c->q8_rows.p, B, (uint32_t *)c->bits.p, (int32_t *)c->q8_pm.p, (uint32_t *)c->flags.p)))
        return sync_fail(c, rc);
    std::vector<uint32_t> w(B * NW);
    HIP_TRY(c, hipMemcpyAsync(w.data(), c->bits.p, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (pm) HIP_TRY(c, hipMemcpyAsync(pm, c->q8_pm.p, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (flags) HIP_TRY(c, hipMemcpyAsync(flags, c->flags.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unpack_rows(w.data(), B, (int)N, u_hat);
    return POLAR_OK;
}

}  // extern "C"
