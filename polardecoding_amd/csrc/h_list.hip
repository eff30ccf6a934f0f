// h_list.hip -- list output: all L paths, masked-CRC selection, list soft output; the sent-path trace of the list decode.
#include "polar_hostlib.h"
#include "trace_out.h"

using namespace polar_host;

extern "C" {

// ---- list output (include/polar_hip.h, "List output") ------------------------------------------------------------------------
// rule 7: which contexts have a list.  POLAR_OK, or the refusal; the ctx is not touched.
static int list_ctx_check(const polar_ctx *c)
{
    if (!c) return POLAR_EINVAL;
    const polar_cfg &g = c->cfg;
    if ((g.algo != POLAR_ALGO_SCL && g.algo != POLAR_ALGO_CASCL) || g.dtype == POLAR_Q8) return POLAR_EINVAL;
    if (c->cascl_stages.size() > 1) return POLAR_EINVAL;
    if (g.N > 1024) return POLAR_ENOKERNEL;
    return POLAR_OK;
}

// the constraint tables the list kernel reads: the ctx's own on a dynamic ctx, else the D = 0 tables, built on first use
static int list_tables(polar_ctx *c, const uint32_t **mask, const int **row)
{
    if (c->is_dyn) {
        *mask = c->d_dyn_mask;
        *row = c->d_dyn_row;
        return POLAR_OK;
    }
    if (!c->d_list_row) {
        const std::vector<uint32_t> m((size_t)c->NW, 0u);
        const std::vector<int> r((size_t)c->cfg.N, -1);
        hipError_t e = hipSuccess;
        int rc;
        if ((rc = c->d_list_mask.upload(m.data(), m.size(), &e)) || (rc = c->d_list_row.upload(r.data(), r.size(), &e))) {
            c->d_list_mask.reset();
            c->d_list_row.reset();
            if (rc == POLAR_ENOMEM) (void)hipGetLastError();
            c->last_error = std::string("list tables: ") + hipGetErrorString(e);
            return rc;
        }
    }
    *mask = c->d_list_mask;
    *row = c->d_list_row;
    return POLAR_OK;
}

// the list decode of N-wide rows
static int list_decode_plain(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_paths, double *d_pm,
                             uint32_t *d_rem, uint32_t *d_count, uint32_t *d_flags)
{
    const polar_cfg &g = c->cfg;
    const bool crc = g.algo == POLAR_ALGO_CASCL;
    const uint32_t *mask = nullptr;
    const int *row = nullptr;
    int rc;
    if ((rc = list_tables(c, &mask, &row))) return rc;
    polar::SclParams P{};
    P.in = d_in; P.sigma = sigma; P.flags = d_flags;
    P.frozen = c->d_frozen;
    P.crc_tab = crc ? c->d_crc_tab.get() : nullptr;
    P.crc_r = crc ? g.crc_r : 0;
    P.N = g.N; P.n = c->n; P.B = (int)B;
    return polar_tu::list_decode(c, P, mask, row, g.dtype == POLAR_F32, in_is_f32 != 0, d_paths, d_pm, d_rem, d_count);
}

int polar_list_decode(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_paths, double *d_pm,
                      uint32_t *d_rem, uint32_t *d_count, uint32_t *d_flags)
{
    int rc = list_ctx_check(c);
    if (rc) return rc;
    const size_t esz = in_is_f32 ? 4 : 8;
    if (!d_in || (!d_paths && !d_pm && !d_rem && !d_count && !d_flags) || B > kMaxBatch ||
        (reinterpret_cast<uintptr_t>(d_in) % esz))
        return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    if (c->rm_mode == POLAR_RM_NONE) return list_decode_plain(c, d_in, in_is_f32, sigma, B, d_paths, d_pm, d_rem, d_count, d_flags);
    // a rate-matched ctx: the rows of E values are recovered first, in the chunks of decode_device_impl
    const size_t L = (size_t)c->cfg.L;
    return for_rm_chunks(c, d_in, in_is_f32, sigma, B, [&](const void *rows, size_t off, size_t nc) {
        return list_decode_plain(c, rows, in_is_f32, 0.0, nc, d_paths ? d_paths + off * L * (size_t)c->NW : nullptr,
                                 d_pm ? d_pm + off * L : nullptr, d_rem ? d_rem + off * L : nullptr,
                                 d_count ? d_count + off : nullptr, d_flags ? d_flags + off : nullptr);
    });
}

// host-buffer form: the batch goes through the device buffers in one piece
int polar_list_decode_host(polar_ctx *c, const double *llr_in, size_t B, int *paths, double *pm, unsigned *rem, unsigned *count,
                           unsigned *flags)
{
    int rc = list_ctx_check(c);
    if (rc) return rc;
    if (!llr_in || (!paths && !pm && !rem && !count && !flags) || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    const size_t N = (size_t)c->cfg.N, NW = (size_t)c->NW, L = (size_t)c->cfg.L;
    const size_t W = c->rm_mode != POLAR_RM_NONE ? (size_t)c->rm_E : N;
    static const char *what = "polar_list_decode_host";
    if ((rc = ensure_nomem(c, c->in, B * W * sizeof(double), what))) return rc;
    if (paths && (rc = ensure_nomem(c, c->list_paths, B * L * NW * sizeof(uint32_t), what))) return rc;
    if (pm && (rc = ensure_nomem(c, c->list_pm, B * L * sizeof(double), what))) return rc;
    if (rem && (rc = ensure_nomem(c, c->list_rem, B * L * sizeof(uint32_t), what))) return rc;
    if (count && (rc = ensure_nomem(c, c->list_cnt, B * sizeof(uint32_t), what))) return rc;
    if (flags && (rc = ensure_nomem(c, c->flags, B * sizeof(uint32_t), what))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->in.p, llr_in, B * W * sizeof(double), hipMemcpyHostToDevice, c->stream));
    rc = polar_list_decode(c, c->in.p, 0, 0.0, B, paths ? (uint32_t *)c->list_paths.p : nullptr,
                                  pm ? (double *)c->list_pm.p : nullptr, rem ? (uint32_t *)c->list_rem.p : nullptr,
                                  count ? (uint32_t *)c->list_cnt.p : nullptr, flags ? (uint32_t *)c->flags.p : nullptr);
    if (rc) return sync_fail(c, rc);
    std::vector<uint32_t> w(paths ? B * L * NW : 0);
    if (paths) HIP_TRY(c, hipMemcpyAsync(w.data(), c->list_paths.p, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (pm) HIP_TRY(c, hipMemcpyAsync(pm, c->list_pm.p, B * L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (rem) HIP_TRY(c, hipMemcpyAsync(rem, c->list_rem.p, B * L * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (count) HIP_TRY(c, hipMemcpyAsync(count, c->list_cnt.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (flags) HIP_TRY(c, hipMemcpyAsync(flags, c->flags.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (paths) unpack_rows(w.data(), B * L, (int)N, paths);
    return POLAR_OK;
}

int polar_list_select(polar_ctx *c, const uint32_t *d_rem, const uint32_t *d_count, size_t B, const uint32_t *d_masks, int M,
                      int32_t *d_idx)
{
    int rc = list_ctx_check(c);
    if (rc) return rc;
    if (!d_rem || !d_count || !d_masks || !d_idx || M < 1 || M > 64 || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    return polar_tu::list_select(c, d_rem, d_count, B, d_masks, M, d_idx);
}

int polar_list_gather(polar_ctx *c, const uint32_t *d_paths, const int32_t *d_idx, int idx_stride, size_t B,
                      uint32_t *d_uhat_bits)
{
    int rc = list_ctx_check(c);
    if (rc) return rc;
    if (!d_paths || !d_idx || !d_uhat_bits || idx_stride < 1 || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    return polar_tu::list_gather(c, d_paths, d_idx, idx_stride, B, d_uhat_bits);
}

int polar_list_soft(polar_ctx *c, const uint32_t *d_paths, const double *d_pm, const uint32_t *d_count, const uint32_t *d_rem,
                    uint32_t want_rem, int domain, double clamp, size_t B, double *d_out)
{
    int rc = list_ctx_check(c);
    if (rc) return rc;
    if (!d_paths || !d_pm || !d_count || !d_out || (domain != 0 && domain != 1) || !(clamp > 0) || !std::isfinite(clamp) ||
        B > kMaxBatch)
        return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    return polar_tu::list_soft(c, d_paths, d_pm, d_count, d_rem, want_rem, domain, clamp, B, d_out);
}

// ---- sent-path trace (include/polar_hip.h, "Sent-path trace") ---------------------------------------------------------------
// the trace of N-wide rows: list_decode_plain with the TRACE kernels
static int list_trace_plain(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, const polar::TraceOut &T,
                            uint32_t *d_flags)
{
    const polar_cfg &g = c->cfg;
    const bool crc = g.algo == POLAR_ALGO_CASCL;
    const uint32_t *mask = nullptr;
    const int *row = nullptr;
    int rc;
    if ((rc = list_tables(c, &mask, &row))) return rc;
    polar::SclParams P{};
    P.in = d_in; P.sigma = sigma; P.flags = d_flags;
    P.frozen = c->d_frozen;
    P.crc_tab = crc ? c->d_crc_tab.get() : nullptr;
    P.crc_r = crc ? g.crc_r : 0;
    P.N = g.N; P.n = c->n; P.B = (int)B;
    return polar_tu::list_trace(c, P, mask, row, g.dtype == POLAR_F32, in_is_f32 != 0, T);
}

int polar_list_trace(polar_ctx *c, const void *d_rows, int rows_are_f32, double sigma, const uint32_t *d_u_bits, size_t B,
                     int32_t *d_loss_leaf, uint32_t *d_loss_rank, int32_t *d_rank, int32_t *d_chosen, uint32_t *d_flags)
{
    int rc = list_ctx_check(c);
    if (rc) return rc;
    const size_t esz = rows_are_f32 ? 4 : 8;
    if (!d_rows || !d_u_bits || (!d_loss_leaf && !d_loss_rank && !d_rank && !d_chosen && !d_flags) || B > kMaxBatch ||
        (reinterpret_cast<uintptr_t>(d_rows) % esz))
        return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    const polar::TraceOut T{d_u_bits, d_loss_leaf, d_loss_rank, d_rank, d_chosen};
    if (c->rm_mode == POLAR_RM_NONE) return list_trace_plain(c, d_rows, rows_are_f32, sigma, B, T, d_flags);
    // a rate-matched ctx: the rows of E values are recovered first, in the chunks of decode_device_impl
    return for_rm_chunks(c, d_rows, rows_are_f32, sigma, B, [&](const void *rows, size_t off, size_t nc) {
        auto at = [off](auto *p) { return p ? p + off : nullptr; };
        const polar::TraceOut Tc{d_u_bits + off * (size_t)c->NW, at(d_loss_leaf), at(d_loss_rank), at(d_rank), at(d_chosen)};
        return list_trace_plain(c, rows, rows_are_f32, 0.0, nc, Tc, at(d_flags));
    });
}

int polar_list_trace_count(polar_ctx *c, const int32_t *d_loss_leaf, const int32_t *d_rank, const int32_t *d_chosen, size_t B,
                           uint64_t *d_hist)
{
    int rc = list_ctx_check(c);
    if (rc) return rc;
    if (!d_loss_leaf || !d_rank || !d_chosen || !d_hist || B > kMaxBatch || (reinterpret_cast<uintptr_t>(d_hist) % 8))
        return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    return polar_tu::trace_count(c, d_loss_leaf, d_rank, d_chosen, B, reinterpret_cast<unsigned long long *>(d_hist));
}

// host-buffer form: the batch goes through the device buffers in one piece
int polar_list_trace_host(polar_ctx *c, const double *llr_in, const int *u, size_t B, int *loss_leaf, unsigned *loss_rank,
                          int *rank, int *chosen, unsigned *flags)
{
    int rc = list_ctx_check(c);
    if (rc) return rc;
    if (!llr_in || !u || (!loss_leaf && !loss_rank && !rank && !chosen && !flags) || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    const size_t N = (size_t)c->cfg.N, NW = (size_t)c->NW;
    const size_t W = c->rm_mode != POLAR_RM_NONE ? (size_t)c->rm_E : N;
    static const char *what = "polar_list_trace_host";
    if ((rc = ensure_nomem(c, c->in, B * W * sizeof(double), what))) return rc;
    if ((rc = ensure_nomem(c, c->list_paths, B * NW * sizeof(uint32_t), what))) return rc;
    if (loss_leaf && (rc = ensure_nomem(c, c->list_cnt, B * sizeof(int32_t), what))) return rc;
    if (loss_rank && (rc = ensure_nomem(c, c->list_rem, B * sizeof(uint32_t), what))) return rc;
    if ((rank || chosen) && (rc = ensure_nomem(c, c->list_pm, 2 * B * sizeof(int32_t), what))) return rc;
    if (flags && (rc = ensure_nomem(c, c->flags, B * sizeof(uint32_t), what))) return rc;
    const std::vector<uint32_t> uw = pack_rows(u, B, (int)N);
    int32_t *d_rank = rank ? (int32_t *)c->list_pm.p : nullptr, *d_chosen = chosen ? (int32_t *)c->list_pm.p + B : nullptr;
    HIP_TRY(c, hipMemcpyAsync(c->in.p, llr_in, B * W * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->list_paths.p, uw.data(), uw.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    rc = polar_list_trace(c, c->in.p, 0, 0.0, (const uint32_t *)c->list_paths.p, B,
                          loss_leaf ? (int32_t *)c->list_cnt.p : nullptr, loss_rank ? (uint32_t *)c->list_rem.p : nullptr, d_rank,
                          d_chosen, flags ? (uint32_t *)c->flags.p : nullptr);
    if (rc) return sync_fail(c, rc);
    if (loss_leaf) HIP_TRY(c, hipMemcpyAsync(loss_leaf, c->list_cnt.p, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (loss_rank) HIP_TRY(c, hipMemcpyAsync(loss_rank, c->list_rem.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (rank) HIP_TRY(c, hipMemcpyAsync(rank, d_rank, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (chosen) HIP_TRY(c, hipMemcpyAsync(chosen, d_chosen, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (flags) HIP_TRY(c, hipMemcpyAsync(flags, c->flags.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // uw lives until here
    return POLAR_OK;
}

}  // extern "C"
