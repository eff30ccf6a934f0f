// polar_hostlib.h -- internal: what the host translation units share.  polar_hip.hip (construction, the kernel choice, the
// decode path, the host pipeline) and h_*.hip (one unit per concern, __graft_entry__.py HOST_TUS) include this header; the
// kernel units k_*.hip include polar_host.h only.  Every name here is in namespace polar_host: none is exported
// (polar_hip.map).  What one unit alone uses stays in that unit's anonymous namespace.
#pragma once
#include "polar_host.h"

#include <cmath>
#include <cstdio>
#include <thread>

#include "scf_params.h"
#include "scan_params.h"

namespace polar_host {

constexpr size_t kMaxBatch = 0x7fffffffull;   // frames per call: the kernels count them in an int

// The device-side outputs of one decode.
struct DecodeOut {            // every member nullable unless the decoder says otherwise
    uint32_t *bits;  double *pm;  uint32_t *flags;
    uint32_t *iters;          // BP round trips / CA-SCL deciding list size / SC-Flip attempt
    void *llr_u, *ext_x;      // SCAN
    uint32_t *graph, *total;  // BPL
    int32_t *sets;            // SC-Flip reported sets [B][SCF_MAX_ORDER]
};
// o from frame off of ctx c on: NW words of bits, N values of the ctx dtype of llr_u / ext_x and SCF_MAX_ORDER sets per
// frame, one element of every other member; null members stay null
inline DecodeOut advanced(const polar_ctx *c, const DecodeOut &o, size_t off)
{
    const size_t soft_row = (size_t)c->cfg.N * (c->cfg.dtype == POLAR_F32 ? 4 : 8);
    auto at = [off](auto *p, size_t stride) { return p ? p + off * stride : nullptr; };
    return {at(o.bits, (size_t)c->NW), at(o.pm, 1), at(o.flags, 1), at(o.iters, 1), at((char *)o.llr_u, soft_row),
            at((char *)o.ext_x, soft_row), at(o.graph, 1), at(o.total, 1), at(o.sets, polar::SCF_MAX_ORDER)};
}

// The caller's host outputs of host_batch(): u_hat [B][N] is required, the others are nullable.
struct HostOut {
    int *u_hat;  double *pm;  unsigned *flags;
    unsigned *iters, *graph, *total;
    int *sets;
};

// h_code.hip: code construction, no launch
std::vector<int> default_order(int N);
std::vector<uint32_t> make_crc_table(int N, int r, const std::vector<int> &taps, const std::vector<int> &I);
std::vector<uint32_t> make_crc_masks(int N, const std::vector<uint32_t> &tab);
int fill_phase_end(int N, const unsigned char *frozen);
int upload_crc_tables(polar_ctx *c, const std::vector<uint32_t> &t);
int info_order_table(polar_ctx *c);
bool has_crc(int algo);

// polar_hip.hip: the decode path
size_t chunk_rows(const polar_ctx *c, size_t B, size_t row_bytes, size_t floor = 64);
int decode_fixed(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits,
                 double *d_pm, uint32_t *d_flags, const uint32_t *d_frozen, uint32_t *d_iters = nullptr);
int decode_device_impl(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, const DecodeOut &o,
                       const uint32_t *d_frozen);
void refresh_kernel_name(polar_ctx *c);
void sync_stage_ctx(polar_ctx *c);
std::vector<uint32_t> pack_rows(const int *v, size_t rows, int width);
void unpack_rows(const uint32_t *w, size_t rows, int width, int *out);
int sync_fail(polar_ctx *c, int rc);
int host_batch(polar_ctx *c, const double *in, double sigma, const unsigned char *frozen_mask, size_t B, const HostOut &h);

// h_decoders.hip: the decoders around the fixed one (decode_device_plain, polar_hip.hip, chooses among them)
int cascl_adaptive(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits,
                   double *d_pm, uint32_t *d_flags, uint32_t *d_list);
int scf_decode(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits, double *d_pm,
               uint32_t *d_flags, uint32_t *d_attempts, int32_t *d_sets);
int bpl_decode(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits, double *d_pm,
               uint32_t *d_flags, uint32_t *d_iters, uint32_t *d_graph, uint32_t *d_total);
int scan_decode(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits, double *d_pm,
                uint32_t *d_flags, const uint32_t *d_frozen, void *d_llr_u, void *d_ext_x);

// h_fer.hip: generate -> decode -> count on one ctx (the groups of h_group.hip run it per GPU)
int fer_batch_impl(polar_ctx *c, unsigned long long seed, unsigned long long first_frame, double snr_db, size_t B,
                   unsigned long long *h, uint32_t *d_frame_err = nullptr);

// The rows of a rate-matched ctx (polar_create_rm) hold E values: k_rm_recover turns them into N-wide rows of the input type
// in ctx scratch, in chunks of at most 256 MiB, and body(rows, off, nc) decodes the nc frames from frame off on with
// sigma = 0 (include/polar_hip.h rule 7).  c->rm_rows belongs to c->stream (it is part of the lane, polar_host.h).
template <class Body> int for_rm_chunks(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, Body body)
{
    const size_t esz = in_is_f32 ? 4 : 8, row = (size_t)c->cfg.N * esz;
    const size_t CH = chunk_rows(c, B, row);
    int rc;
    if ((rc = ensure(c, c->rm_rows, CH * row))) return rc;
    for (size_t off = 0; off < B; off += CH) {
        const size_t nc = std::min(CH, B - off);
        if ((rc = polar_tu::rm_recover(c, (const char *)d_in + off * (size_t)c->rm_E * esz, in_is_f32 != 0, sigma, nc, c->rm_rows.p)))
            return rc;
        if ((rc = body(c->rm_rows.p, off, nc))) return rc;
    }
    return POLAR_OK;
}

}  // namespace polar_host
