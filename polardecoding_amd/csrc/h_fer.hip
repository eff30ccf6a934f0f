// h_fer.hip -- error counting, the stop rule, Monte-Carlo construction, the device generator and the FER loop.  The one
// unit that holds the count and generator kernels (count_kernel.h, gen_kernel.h).
#include "polar_hostlib.h"

#include "count_kernel.h"
#include "gen_kernel.h"

using namespace polar_host;

namespace polar_host {

// generate -> decode -> count for B frames; the two counters stay in c->gen_cnt (device) and are copied to h[2] if h != null
int fer_batch_impl(polar_ctx *c, unsigned long long seed, unsigned long long first_frame, double snr_db, size_t B,
                   unsigned long long *h, uint32_t *d_frame_err)
{
    const int NW = c->NW;
    const int W = c->rm_mode != POLAR_RM_NONE ? c->rm_E : c->cfg.N;   // values per generated row
    const bool f32 = c->cfg.dtype != POLAR_F64;   // a Q8 ctx generates f32 rows and quantises them
    int rc;
    if ((rc = ensure(c, c->gen_llr, B * W * (f32 ? 4 : 8)))) return rc;
    if ((rc = ensure(c, c->gen_u, B * NW * 4))) return rc;
    if ((rc = ensure(c, c->bits, B * NW * 4))) return rc;
    if ((rc = ensure(c, c->gen_cnt, 16))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->gen_cnt.p, 0, 16, c->stream));
    // Two halves on two streams (own decode scratch each): the generator of one half and the partly filled last
    // pass of its decode overlap the other half's decode.  Frame i of the batch is the same frame either way
    // (the generator is counter-based), and the two counters are atomics.
    // (not with an adaptive CA-SCL rule: its stage buffers belong to one stream and it syncs between stages)
    // (nor for SC-Flip and BP list decoding, for the same reasons)
    const size_t half = (B >= 32768 && c->cascl_stages.empty() && c->cfg.algo != POLAR_ALGO_SCF && c->cfg.algo != POLAR_ALGO_BPL) ? (B / 2 + 63) / 64 * 64 : B;
    if (half < B && !c->lane_b.stream) {
        HIP_TRY(c, c->lane_b.stream.create(hipStreamNonBlocking));
        HIP_TRY(c, c->ev_b.create(hipEventDisableTiming));
    }
    const size_t esz = f32 ? 4 : 8;
    auto run_part = [&](size_t f0, size_t nf) -> int {
        int r;
        if ((r = polar_generate_device(c, seed, first_frame + f0, snr_db, nf, (char *)c->gen_llr.p + f0 * W * esz, f32 ? 1 : 0, 0,
                                       (uint32_t *)c->gen_u.p + f0 * NW))) return r;
        if ((r = decode_device_impl(c, (char *)c->gen_llr.p + f0 * W * esz, f32 ? 1 : 0, 0.0, nf, {.bits = (uint32_t *)c->bits.p + f0 * NW},
                                    c->d_frozen))) return r;
        return polar_count_errors_device(c, (uint32_t *)c->bits.p + f0 * NW, (uint32_t *)c->gen_u.p + f0 * NW, nf,
                                         (unsigned long long *)c->gen_cnt.p, d_frame_err ? d_frame_err + f0 : nullptr);
    };
    if (half < B) {
        // second half on lane_b's stream, after the counters were cleared on the main stream
        HIP_TRY(c, hipEventRecord(c->ev_b, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->lane_b.stream, c->ev_b, 0));
        hipError_t e;
        {
            OtherLane other(c);
            rc = run_part(half, B - half);
            e = hipEventRecord(c->ev_b, c->stream);   // behind the second half's work, before the first half is enqueued
        }
        if (rc) return rc;
        HIP_TRY(c, e);
    }
    if ((rc = run_part(0, half))) return rc;
    if (half < B) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_b, 0));
    if (h) {
        HIP_TRY(c, hipMemcpyAsync(h, c->gen_cnt.p, 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return POLAR_OK;
}

}  // namespace polar_host

extern "C" {

int polar_count_errors_device(polar_ctx *c, const uint32_t *d_uhat, const uint32_t *d_u, size_t B,
                              unsigned long long *d_counters, uint32_t *d_frame_err)
{
    if (!c || !d_uhat || !d_u || !d_counters) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    if (B == 0) return POLAR_OK;
    if (c->sys_polar) {   // systematic polar code: the comparison is on x_hat[I] against x[I]
        if (B > kMaxBatch) return POLAR_EINVAL;
        return polar_tu::enc_count_sys(c, d_uhat, d_u, B, d_counters, d_frame_err);
    }
    polar::CountParams P{d_uhat, d_u, c->d_info, d_counters, d_frame_err, c->NW, (int)B};
    const int waves_per_block = 4;
    const int grid = stride_grid(c, (long long)((B + waves_per_block - 1) / waves_per_block), (long long)c->num_cu * 8);
    hipLaunchKernelGGL(polar::k_count_errors, dim3(grid), dim3(64 * waves_per_block), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_stop_rule_cut_device(polar_ctx *c, const uint32_t *d_frame_err, size_t B, unsigned need, size_t min_frames,
                               unsigned long long *d_out)
{
    if (!c || !d_frame_err || !d_out || (need < 1 && min_frames < 1) || B > kMaxBatch) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    if (B == 0) {
        HIP_TRY(c, hipMemsetAsync(d_out, 0, 3 * sizeof(unsigned long long), c->stream));
        return POLAR_OK;
    }
    hipLaunchKernelGGL(polar::k_stop_cut, dim3(1), dim3(1024), 0, c->stream, d_frame_err, (int)B, need,
                       (int)std::min<size_t>(min_frames, B), d_out);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_stop_rule_batch_y(polar_ctx *c, const double *y, double sigma, const uint32_t *u_bits, size_t B, unsigned need,
                            size_t min_frames, size_t *consumed, unsigned long long *block_errors,
                            unsigned long long *bit_errors)
{
    if (!c || !y || !u_bits || !consumed || !block_errors || !bit_errors || (need < 1 && min_frames < 1) || !(sigma > 0))
        return POLAR_EINVAL;
    *consumed = 0; *block_errors = 0; *bit_errors = 0;
    if (B == 0) return POLAR_OK;
    if (B > kMaxBatch) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    const int NW = c->NW;
    const int W = c->rm_mode != POLAR_RM_NONE ? c->rm_E : c->cfg.N;   // values per row
    int rc;
    if ((rc = ensure(c, c->in, B * W * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->bits, B * NW * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->gen_u, B * NW * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->flags, B * sizeof(uint32_t)))) return rc;           // per-frame error counts
    if ((rc = ensure(c, c->gen_cnt, 5 * sizeof(unsigned long long)))) return rc;   // [0..2) totals, [2..5) the cut
    unsigned long long *cnt = (unsigned long long *)c->gen_cnt.p;
    HIP_TRY(c, hipMemcpyAsync(c->in.p, y, B * W * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->gen_u.p, u_bits, B * NW * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(cnt, 0, 5 * sizeof(unsigned long long), c->stream));
    if ((rc = decode_device_impl(c, c->in.p, 0, sigma, B, {.bits = (uint32_t *)c->bits.p}, c->d_frozen))) return sync_fail(c, rc);
    if ((rc = polar_count_errors_device(c, (uint32_t *)c->bits.p, (uint32_t *)c->gen_u.p, B, cnt, (uint32_t *)c->flags.p)))
        return sync_fail(c, rc);
    if ((rc = polar_stop_rule_cut_device(c, (uint32_t *)c->flags.p, B, need, min_frames, cnt + 2))) return sync_fail(c, rc);
    unsigned long long h[3];
    HIP_TRY(c, hipMemcpyAsync(h, cnt + 2, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *consumed = (size_t)h[0];
    *block_errors = h[1];
    *bit_errors = h[2];
    return POLAR_OK;
}

// ---- Monte-Carlo construction (include/polar_hip.h) ---------------------------------------------------------------------
int polar_genie_count_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint64_t *d_counts)
{
    if (!c || c->rm_mode != POLAR_RM_NONE || c->cfg.dtype == POLAR_Q8 || !d_in || !d_counts || B > kMaxBatch) return POLAR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_in) % (in_is_f32 ? 4 : 8)) || (reinterpret_cast<uintptr_t>(d_counts) % 8)) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return polar_tu::genie_count(c, d_in, in_is_f32 != 0, sigma, B, reinterpret_cast<unsigned long long *>(d_counts));
}

int polar_genie_rows_device(polar_ctx *c, unsigned long long seed, unsigned long long first_frame, double sigma, size_t B,
                            void *d_out, int out_is_f32)
{
    if (!c || c->rm_mode != POLAR_RM_NONE || c->cfg.dtype == POLAR_Q8 || !d_out || B > kMaxBatch || !(sigma > 0) || !std::isfinite(sigma)) return POLAR_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_out) % (out_is_f32 ? 4 : 8)) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return polar_tu::genie_rows(c, seed, first_frame, sigma, B, d_out, out_is_f32 != 0);
}

// design rows of the ctx dtype into ctx scratch, chunks of at most 256 MiB (the rule of the rate-matching path), counted chunk by chunk
int polar_construct_batch(polar_ctx *c, unsigned long long seed, unsigned long long first_frame, double sigma, size_t B,
                          uint64_t *d_counts)
{
    if (!c || c->rm_mode != POLAR_RM_NONE || c->cfg.dtype == POLAR_Q8 || !d_counts || B > kMaxBatch || !(sigma > 0) || !std::isfinite(sigma)) return POLAR_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_counts) % 8) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    const bool f32 = c->cfg.dtype == POLAR_F32;
    const size_t row = (size_t)c->cfg.N * (f32 ? 4 : 8);
    const size_t CH = chunk_rows(c, B, row);
    int rc;
    if ((rc = ensure(c, c->genie_rows, CH * row))) return rc;
    for (size_t off = 0; off < B; off += CH) {
        const size_t nc = std::min(CH, B - off);
        if ((rc = polar_tu::genie_rows(c, seed, first_frame + off, sigma, nc, c->genie_rows.p, f32))) return rc;
        if ((rc = polar_tu::genie_count(c, c->genie_rows.p, f32, 0.0, nc, reinterpret_cast<unsigned long long *>(d_counts)))) return rc;
    }
    return POLAR_OK;
}

int polar_construct_order(int N, const uint64_t *counts, const int *base_order, int *out)
{
    if (N < 32 || N > 4096 || (N & (N - 1)) || !counts || !out) return POLAR_EINVAL;
    std::vector<int> base = base_order ? std::vector<int>(base_order, base_order + N) : default_order(N);
    std::vector<unsigned char> seen((size_t)N, 0);
    for (int j : base) {
        if (j < 0 || j >= N || seen[(size_t)j]) return POLAR_EINVAL;
        seen[(size_t)j] = 1;
    }
    // score = 2 * err + tie, wider than the counters; descending score, equal scores in base order
    auto score = [&](int j) { return 2 * (unsigned __int128)counts[j] + counts[(size_t)N + j]; };
    std::stable_sort(base.begin(), base.end(), [&](int a, int b) { return score(a) > score(b); });
    std::copy(base.begin(), base.end(), out);
    return POLAR_OK;
}

int polar_generate_device(polar_ctx *c, unsigned long long seed, unsigned long long first_frame, double snr_db,
                          size_t B, void *d_out, int out_is_f32, int out_is_y, uint32_t *d_u_bits)
{
    if (!c || !d_out || B > kMaxBatch) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    if (B == 0) return POLAR_OK;
    const polar_cfg &g = c->cfg;
    if (g.N < 64) return POLAR_EINVAL;
    if (int rc = info_order_table(c)) return rc;
    polar::GenParams P{};
    P.out = d_out; P.u_bits = d_u_bits; P.info_order = c->d_info_order;
    P.seed = seed; P.first_frame = first_frame;
    P.sigma = std::pow(10.0, snr_db / -20.0);  // SCL_1024.c:226
    P.crc_r = g.crc_r; P.crc_mask = 0; P.crc_top = 0;
    P.gc_rows = c->d_gc_rows;
    if (g.crc_r == 0) P.crc_mask = 1u;
    for (int t : c->taps) {
        if (t < 32) P.crc_mask |= 1u << t;
        else P.crc_top = 1u;
    }
    P.N = g.N; P.n = c->n; P.K = g.K; P.A = c->A; P.B = (int)B;
    P.out_is_f32 = out_is_f32; P.out_is_y = out_is_y;
    P.sys_frozen = c->sys_polar ? c->d_frozen : nullptr;   // polar_set_systematic refuses rate-matched and dynamic contexts
    if (c->rm_mode != POLAR_RM_NONE) return polar_tu::rm_generate(c, P);   // [B][E] (include/polar_hip.h rules 1-3)
    if (c->is_dyn) return polar_tu::dyn_generate(c, P);                    // the dynamic bits filled in before the encode
    const int waves = 4;
    const size_t lds = (size_t)waves * (g.N + 2 * 1024);
    const int grid = stride_grid(c, (long long)((B + waves - 1) / waves), (long long)c->num_cu * 8);
    hipLaunchKernelGGL(polar::k_generate, dim3(grid), dim3(64 * waves), lds, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int polar_fer_batch(polar_ctx *c, unsigned long long seed, unsigned long long first_frame, double snr_db, size_t B,
                    unsigned long long *block_errors, unsigned long long *bit_errors)
{
    if (!c || !block_errors || !bit_errors) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    if (B == 0) return POLAR_OK;
    unsigned long long h[2] = {0, 0};
    const int rc = fer_batch_impl(c, seed, first_frame, snr_db, B, h);
    if (rc) return rc;
    *block_errors += h[0];
    *bit_errors += h[1];
    return POLAR_OK;
}

}  // extern "C"
