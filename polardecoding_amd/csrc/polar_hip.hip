// polar_hip.hip -- C ABI (include/polar_hip.h) over the hand-written gfx950 kernels: construction, the kernel choice, the
// decode path and the chunked host pipeline.  The other concerns of the host side live in the h_*.hip units
// (polar_hostlib.h declares what crosses them), the kernels and their launch code in the k_*.hip units (polar_host.h).
// The only host unit that is compiled a second time with -DPOLAR_TESTING.
#include "polar_hostlib.h"
#ifdef POLAR_TESTING
#include "../../include/polar_hip_testing.h"
#endif

#include <mutex>

using namespace polar_host;

namespace {

static bool sc_lanes_ok(const polar_ctx *c, size_t B)
{
    return c->cfg.algo == POLAR_ALGO_SC && !c->force_generic && c->cfg.N <= 2048 && B >= 64;
}

bool fast_ok(const polar_ctx *c, int in_is_f32)
{
    const polar_cfg &g = c->cfg;
    if (c->force_generic || c->force_spill) return false;
    if (g.algo != POLAR_ALGO_SCL && g.algo != POLAR_ALGO_CASCL) return false;
    if (g.L != 8 || (g.N != 1024 && g.N != 128)) return false;
    if (g.dtype == POLAR_F64 && in_is_f32) return false;
    return true;
}

// The kernel family the fixed decoder of ctx c runs on a batch of B rows: decode_fixed() launches it, refresh_kernel_name()
// names it.  scl_big.h for SCL / CA-SCL with N >= 512, L >= 2 (shapes without a tuned kernel); else the generic kernel,
// LDS-resident when the levels fit (160 KB per CU), global-scratch variant otherwise.
enum class Family { BP, WIDE, DYN, SC_LANES, FAST, FAST2, FAST4, BIG, GENERIC };
Family kernel_family(const polar_ctx *c, int in_is_f32, size_t B)
{
    const polar_cfg &g = c->cfg;
    if (g.algo == POLAR_ALGO_BP || g.algo == POLAR_ALGO_BPL) return Family::BP;   // BPL: the kernel of every attempt
    if (c->logL > 5) return Family::WIDE;   // L = 64 / 128 / 256: one kernel, plain or with dynamic frozen bits
    if (c->is_dyn) return Family::DYN;   // dynamic frozen bits: one kernel for every shape
    if (sc_lanes_ok(c, B)) return Family::SC_LANES;
    if (fast_ok(c, in_is_f32)) {
#ifdef POLAR_TESTING
        if (g.N == 1024 && c->use_fast4) return Family::FAST4;
#endif
        if (g.N == 1024 && c->use_fast2) return Family::FAST2;
        return Family::FAST;
    }
    if (c->logL >= 1 && !c->force_generic && g.algo != POLAR_ALGO_SC && c->n >= 9) return Family::BIG;
    return Family::GENERIC;
}

// A Q8 ctx on float or double rows (include/polar_hip.h, fixed-point min-sum, rule 7): rule 1 into ctx scratch in chunks of
// at most 256 MiB of quantised rows, then k_scl_q8; the int32 metric reaches a double d_pm through q8_pm.  c->q8_rows belongs
// to c->stream (it is part of the lane, polar_host.h).
int q8_decode_rows(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits, double *d_pm,
                   uint32_t *d_flags)
{
    const size_t esz = in_is_f32 ? 4 : 8;
    if (reinterpret_cast<uintptr_t>(d_in) % esz) return POLAR_EINVAL;
    const size_t N = (size_t)c->cfg.N;
    const size_t CH = chunk_rows(c, B, N);
    int rc;
    if ((rc = ensure(c, c->q8_rows, CH * N))) return rc;
    if (d_pm && (rc = ensure(c, c->q8_pm, CH * sizeof(int32_t)))) return rc;
    for (size_t off = 0; off < B; off += CH) {
        const size_t nc = std::min(CH, B - off);
        int8_t *rows = (int8_t *)c->q8_rows.p;
        int32_t *pm = d_pm ? (int32_t *)c->q8_pm.p : nullptr;
        if ((rc = polar_tu::q8_quantize(c, (const char *)d_in + off * N * esz, in_is_f32 != 0, sigma, nc * N, rows))) return rc;
        if ((rc = polar_tu::q8_decode(c, rows, nc, d_bits + off * (size_t)c->NW, pm, d_flags ? d_flags + off : nullptr))) return rc;
        if (d_pm && (rc = polar_tu::q8_pm_f64(c, pm, nc, d_pm + off))) return rc;
    }
    return POLAR_OK;
}

// the decoder of ctx c on N-wide rows: the fixed decoder, or for a CA-SCL ctx with a stage rule the adaptive one, or SC-Flip.
// o.iters: BP round trips per frame; CA-SCL: the list size that decided each frame; SC-Flip: the attempt that decided it.
int decode_device_plain(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, const DecodeOut &o,
                        const uint32_t *d_frozen)
{
    uint32_t *d_iters = o.iters;
    if (c && c->cfg.algo == POLAR_ALGO_BPL) return bpl_decode(c, d_in, in_is_f32, sigma, B, o.bits, o.pm, o.flags, o.iters, o.graph, o.total);
    if (c && c->cfg.algo == POLAR_ALGO_SCAN) return scan_decode(c, d_in, in_is_f32, sigma, B, o.bits, o.pm, o.flags, d_frozen, o.llr_u, o.ext_x);
    if (c && c->cfg.algo == POLAR_ALGO_SCF) return scf_decode(c, d_in, in_is_f32, sigma, B, o.bits, o.pm, o.flags, o.iters, o.sets);
    if (c && c->cfg.algo == POLAR_ALGO_CASCL) {
        if (!d_in || !o.bits || B > kMaxBatch) return POLAR_EINVAL;
        if (B == 0) return POLAR_OK;
        if (!c->cascl_stages.empty()) return cascl_adaptive(c, d_in, in_is_f32, sigma, B, o.bits, o.pm, o.flags, o.iters);
        if (d_iters) HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_iters), c->cfg.L, B, c->stream));
        d_iters = nullptr;
    }
    return decode_fixed(c, d_in, in_is_f32, sigma, B, o.bits, o.pm, o.flags, d_frozen, d_iters);
}

// The rows of a rate-matched ctx (polar_create_rm) hold E values: k_rm_recover turns them into N-wide rows of the input type
// in ctx scratch, in chunks of at most 256 MiB, and body(rows, off, nc) decodes the nc frames from frame off on with
// sigma = 0 (include/polar_hip.h rule 7).  c->rm_rows belongs to c->stream (it is part of the lane, polar_host.h).

std::vector<uint32_t> pack_mask(const unsigned char *m, int N, bool invert)
{
    std::vector<uint32_t> w(N / 32, 0u);
    for (int j = 0; j < N; ++j)
        if ((m[j] != 0) != invert) w[j >> 5] |= 1u << (j & 31);
    return w;
}

// packed decisions -> the reference's int u_hat[N] (0/1), eight bits per table look-up
void unpack_words(const uint32_t *w, int NW, int *out)
{
    struct Row { int v[8]; };
    static const std::vector<Row> tab = [] {
        std::vector<Row> t(256);
        for (int b = 0; b < 256; ++b)
            for (int k = 0; k < 8; ++k) t[(size_t)b].v[k] = (b >> k) & 1;
        return t;
    }();
    for (int i = 0; i < NW; ++i) {
        const uint32_t x = w[i];
        std::memcpy(out + 32 * i, &tab[x & 255u], sizeof(Row));
        std::memcpy(out + 32 * i + 8, &tab[(x >> 8) & 255u], sizeof(Row));
        std::memcpy(out + 32 * i + 16, &tab[(x >> 16) & 255u], sizeof(Row));
        std::memcpy(out + 32 * i + 24, &tab[x >> 24], sizeof(Row));
    }
}

}  // namespace

namespace polar_host {

// Rows per pass where a batch goes through ctx scratch in chunks: at most c->chunk_bytes (256 MiB) of rows, at least `floor`
// of them, never more than the batch.
size_t chunk_rows(const polar_ctx *c, size_t B, size_t row_bytes, size_t floor)
{
    return std::min(B, std::max(floor, c->chunk_bytes / row_bytes));
}

// the fixed decoder of ctx c (its cfg.L / algo): the kernel selection every entry point uses
int decode_fixed(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits,
                 double *d_pm, uint32_t *d_flags, const uint32_t *d_frozen, uint32_t *d_iters)
{
    if (!c || !d_in || !d_bits) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    if (B > kMaxBatch) return POLAR_EINVAL;
    const polar_cfg &g = c->cfg;
    if (g.dtype == POLAR_Q8) return q8_decode_rows(c, d_in, in_is_f32, sigma, B, d_bits, d_pm, d_flags);
    const bool f32 = g.dtype == POLAR_F32;
    const Family fam = kernel_family(c, in_is_f32, B);
    if (fam == Family::BP) {
        polar::BpParams P{};
        P.in = d_in; P.sigma = sigma; P.out_bits = d_bits; P.frozen = d_frozen;
        P.N = g.N; P.n = c->n; P.B = (int)B; P.iters = g.bp_iters;
        if (d_pm) HIP_TRY(c, hipMemsetAsync(d_pm, 0, B * sizeof(double), c->stream));
        P.stop = c->bp_stop;
        if (P.stop != POLAR_BP_STOP_NONE) {   // the kernel writes both for every frame
            P.iters_out = d_iters;
            P.flags_out = d_flags;
        } else {
            if (d_flags) HIP_TRY(c, hipMemsetAsync(d_flags, 0, B * sizeof(uint32_t), c->stream));
            if (d_iters) HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_iters), g.bp_iters, B, c->stream));
        }
        return polar_tu::bp(c, P, f32, in_is_f32 != 0);
    }
    polar::SclParams P{};
    P.in = d_in; P.sigma = sigma; P.out_bits = d_bits; P.pm = d_pm; P.flags = d_flags;
    P.frozen = d_frozen;
    P.crc_tab = (g.algo == POLAR_ALGO_CASCL) ? c->d_crc_tab : nullptr;
    P.crc_mask = (g.algo == POLAR_ALGO_CASCL) ? c->d_crc_mask : nullptr;
    P.crc_r = (g.algo == POLAR_ALGO_CASCL) ? g.crc_r : 0;
    // the mask in use is the ctx's own or the per-call one of host_batch(): each has its phase end, any other mask has none
    P.fill_end = d_frozen == c->d_frozen ? c->fill_end : d_frozen == c->d_frozen_override ? c->fill_end_override : 0;
    P.N = g.N; P.n = c->n; P.B = (int)B;
    P.sc_mode = (g.algo == POLAR_ALGO_SC) ? 1 : 0;
    P.dbg = nullptr;
    P.scratch = nullptr;
    P.queue = nullptr;
    const bool in32 = in_is_f32 != 0;
    const bool crc = g.algo == POLAR_ALGO_CASCL;
    switch (fam) {
    case Family::WIDE: return polar_tu::scl_wide(c, P, f32, in32);
    case Family::DYN: return polar_tu::scl_dyn(c, P, f32, in32);
    case Family::SC_LANES: return polar_tu::sc_lanes(c, P, f32, in32);
#ifdef POLAR_TESTING
    case Family::FAST4: return polar_tu::scl_fast4(c, P, f32, in32, crc);
#endif
    case Family::FAST2: return polar_tu::scl_fast2(c, P, f32, in32, crc);
    case Family::FAST: return polar_tu::scl_fast(c, P, f32, in32, crc);
    case Family::BIG: return f32 ? polar_tu::scl_big_f32(c, P, in32) : polar_tu::scl_big_f64(c, P, in32);
    default: return polar_tu::scl_generic(c, P, f32, in32);
    }
}

// The stage contexts run on this ctx's stream with its test-only kernel choices (include/polar_hip_testing.h).
void sync_stage_ctx(polar_ctx *c)
{
    for (polar_ctx *s : c->stage_ctx) {
        if (!s) continue;
        s->stream.adopt(c->stream);
        s->force_generic = c->force_generic;
        s->force_spill = c->force_spill;
        s->use_fast2 = c->use_fast2;
        s->use_fast4 = c->use_fast4;
        s->big_split = c->big_split;
        s->chunk_bytes = c->chunk_bytes;
        s->resident_blocks = c->resident_blocks;
    }
}

// every decode of the C ABI: the ctx's decoder, behind the recovery on a rate-matched ctx
int decode_device_impl(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, const DecodeOut &o,
                       const uint32_t *d_frozen)
{
    if (!c || c->rm_mode == POLAR_RM_NONE) return decode_device_plain(c, d_in, in_is_f32, sigma, B, o, d_frozen);
    const size_t esz = in_is_f32 ? 4 : 8;
    const bool scan = c->cfg.algo == POLAR_ALGO_SCAN;   // its three outputs are nullable
    if (!d_in || (!o.bits && !scan) || B > kMaxBatch || (reinterpret_cast<uintptr_t>(d_in) % esz)) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    return for_rm_chunks(c, d_in, in_is_f32, sigma, B, [&](const void *rows, size_t off, size_t nc) {
        return decode_device_plain(c, rows, in_is_f32, 0.0, nc, advanced(c, o, off), d_frozen);
    });
}

// the kernel instantiation decode_device_impl will launch for this ctx: kernel_family() for input of the arithmetic type
// and a large batch, then the decoders around the fixed one
void refresh_kernel_name(polar_ctx *c)
{
    const polar_cfg &g = c->cfg;
    const char *ty = g.dtype == POLAR_F32 ? "float" : "double";
    char nm[128];
    const Family fam = kernel_family(c, g.dtype == POLAR_F32, 64);
    switch (fam) {
    case Family::BP: {
        const int v = polar_tu::bp_variant(c);
        snprintf(nm, sizeof nm, v == polar_tu::BP_R4 ? "k_bp_r4<%s>%s" : v == polar_tu::BP_W128 ? "k_bp_w128<%s>%s" : "k_bp<%s>%s", ty,
                 c->bp_stop == POLAR_BP_STOP_G ? " (stop rule G)" : "");
        break;
    }
    case Family::DYN:   // stands alone: replaces the wrappers below as well
        snprintf(nm, sizeof nm, "k_scl_dyn<%s,L=%d> (D=%d dynamic frozen bits)", ty, g.L, (int)c->dyn_pos.size());
        break;
    case Family::WIDE:
        if (c->is_dyn) snprintf(nm, sizeof nm, "k_scl_wide<%s,L=%d> (D=%d dynamic frozen bits)", ty, g.L, (int)c->dyn_pos.size());
        else snprintf(nm, sizeof nm, "k_scl_wide<%s,L=%d>", ty, g.L);
        break;
    case Family::SC_LANES: snprintf(nm, sizeof nm, "k_sc_lanes<%s> (batches of 64+; k_scl_generic below)", ty); break;
    case Family::FAST:
    case Family::FAST2:
    case Family::FAST4:
        snprintf(nm, sizeof nm, "k_scl_fast%s<%s,N=%d,L=8>", fam == Family::FAST4 ? "4" : fam == Family::FAST2 ? "2" : "", ty, g.N);
        break;
    case Family::BIG: snprintf(nm, sizeof nm, "k_scl_big<%s,L=%d>", ty, g.L); break;
    case Family::GENERIC: snprintf(nm, sizeof nm, "k_scl_generic<%s,L=%d>", ty, g.L); break;
    }
    if (g.algo == POLAR_ALGO_SCF)
        snprintf(nm, sizeof nm, "k_scf_lanes<%s> (SC-Flip, T=%d; pass A, k_ad_fail_count/scan/write, record, pass B, k_scf_resolve)",
                 ty, c->scf_T);
    if (g.algo == POLAR_ALGO_SCF && c->scf_omega > 0) {
        std::string b = std::to_string(c->scf_T);
        for (int k = 1; k < c->scf_omega; ++k) b += "," + std::to_string(c->scf_Tk[k]);
        snprintf(nm, sizeof nm, "k_scf_lanes<%s> (dynamic SC-Flip, omega=%d, T=%s, c=%g, tau=%g; k_scf_merge, k_scf_resolve_sets)", ty,
                 c->scf_omega, b.c_str(), c->scf_c, c->scf_tau);
    }
    if (g.algo == POLAR_ALGO_SCAN) snprintf(nm, sizeof nm, "k_scan_lanes<%s> (SCAN, I=%d)", ty, c->scan_I);
    if (g.algo == POLAR_ALGO_BPL) {
        const std::string bp = nm;
        snprintf(nm, sizeof nm, "%s x %d graphs%s; glue k_bpl_gather, k_bpl_scatter", bp.c_str(), (int)c->bpl_ident.size(),
                 g.crc_r > 0 ? " (CRC-aided)" : "");
    }
    if (g.dtype == POLAR_Q8) snprintf(nm, sizeof nm, "k_scl_q8<L=%d>", g.L);   // one kernel for SC / SCL / CA-SCL and every shape
    c->kernel_name = nm;
    if (!c->cascl_stages.empty()) {
        sync_stage_ctx(c);
        std::string a = "adaptive CA-SCL:";
        for (size_t i = 0; i < c->cascl_stages.size(); ++i) {
            polar_ctx *s = c->stage_ctx[i];
            if (s) refresh_kernel_name(s);
            a += (i ? " -> L=" : " L=") + std::to_string(c->cascl_stages[i]) + " " + (s ? s->kernel_name : std::string(nm));
        }
        a += "; glue k_ad_crc_check, k_ad_fail_count/scan/write, k_ad_gather, k_ad_scatter";
        c->kernel_name = a;
    }
    if (c->rm_mode != POLAR_RM_NONE) c->kernel_name = "k_rm_recover, then " + c->kernel_name;
    if (fam == Family::DYN || (fam == Family::WIDE && c->is_dyn)) c->kernel_name = nm;
}

// rows of `width` ints (non-zero = 1) -> rows of ceil(width / 32) words, value j of a row in bit j & 31 of its word j / 32
std::vector<uint32_t> pack_rows(const int *v, size_t rows, int width)
{
    const size_t W = (size_t)width, WW = (W + 31) / 32;
    std::vector<uint32_t> w(rows * WW, 0u);
    for (size_t r = 0; r < rows; ++r)
        for (size_t j = 0; j < W; ++j)
            if (v[r * W + j]) w[r * WW + (j >> 5)] |= 1u << (j & 31);
    return w;
}

// the reverse: the whole words of a row through unpack_words, the values of a last partial word one by one
void unpack_rows(const uint32_t *w, size_t rows, int width, int *out)
{
    const size_t W = (size_t)width, WW = (W + 31) / 32;
    for (size_t r = 0; r < rows; ++r) {
        unpack_words(w + r * WW, width / 32, out + r * W);
        for (size_t j = W / 32 * 32; j < W; ++j) out[r * W + j] = (int)((w[r * WW + (j >> 5)] >> (j & 31)) & 1u);
    }
}

// a one-piece host form whose launcher failed: nothing of the call is left in flight when it returns
int sync_fail(polar_ctx *c, int rc)
{
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

// helper threads per direction of the host pipeline (staging of the caller's rows / unpacking of the decisions)
constexpr unsigned HOST_THREADS = 6;   // 4 -> 6: end_to_end 4.4 -> 4.6-4.7 M frames/s; 8 and 12 no more (run 35)
int host_batch(polar_ctx *c, const double *in, double sigma, const unsigned char *frozen_mask, size_t B, const HostOut &h)
{
    int *const u_hat = h.u_hat;
    if (!c || !in || !u_hat) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    if (B == 0) return POLAR_OK;
    const int N = c->cfg.N, NW = c->NW;
    const int W = c->rm_mode != POLAR_RM_NONE ? c->rm_E : N;   // values per input row
    const uint32_t *d_frozen = c->d_frozen;
    if (frozen_mask) {
        if (has_crc(c->cfg.algo) || c->rm_mode != POLAR_RM_NONE || c->is_dyn || c->cfg.dtype == POLAR_Q8) return POLAR_EINVAL;
        std::vector<uint32_t> w = pack_mask(frozen_mask, N, false);
        if (!c->d_frozen_override) HIP_TRY(c, c->d_frozen_override.alloc((size_t)NW));
        HIP_TRY(c, hipMemcpyAsync(c->d_frozen_override, w.data(), NW * sizeof(uint32_t), hipMemcpyHostToDevice,
                                  c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // w goes out of scope
        d_frozen = c->d_frozen_override;
        c->fill_end_override = fill_phase_end(N, frozen_mask);
    }
    int rc;
    if ((rc = ensure(c, c->pm, B * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->flags, B * sizeof(uint32_t)))) return rc;
    // the optional outputs: the caller's array, its staging buffer, bytes per frame
    const struct { void *host; Buf *dev; size_t bytes; } opt[] = {{h.iters, &c->bp_iters, sizeof(uint32_t)},
                                                                   {h.graph, &c->bpl_graph, sizeof(uint32_t)},
                                                                   {h.total, &c->bpl_total, sizeof(uint32_t)},
                                                                   {h.sets, &c->scf_hsets, polar::SCF_MAX_ORDER * sizeof(int32_t)}};
    for (const auto &q : opt)
        if (q.host && (rc = ensure(c, *q.dev, B * q.bytes))) return rc;
    auto dev = [](const void *host, const Buf &b) { return host ? b.p : nullptr; };
    const DecodeOut staging{.pm = (double *)c->pm.p, .flags = (uint32_t *)c->flags.p, .iters = (uint32_t *)dev(h.iters, c->bp_iters),
                            .graph = (uint32_t *)dev(h.graph, c->bpl_graph), .total = (uint32_t *)dev(h.total, c->bpl_total),
                            .sets = (int32_t *)dev(h.sets, c->scf_hsets)};
    // Chunked pipeline: while chunk k is decoded, chunk k+1 crosses PCIe on a second stream and the decisions of
    // chunk k-1 are unpacked to the caller's int array by helper threads.  The input is pageable caller memory: a
    // hipMemcpyAsync from it is a single-threaded staging copy inside the runtime (about 18 GB/s) that blocks this thread.
    // Batches of several chunks are therefore staged HERE, by helper threads, into pinned buffers, and cross PCIe as true
    // asynchronous DMA.
    // chunk: 16384 frames, but at most 128 MiB of input (N = 1024: 16384 frames; N = 4096: 4096), so that the two pinned
    // staging buffers and the two device buffers stay at 256 MiB each whatever the block length
    const size_t CH = std::max<size_t>(256, std::min<size_t>(16384, ((size_t)128 << 20) / ((size_t)W * sizeof(double))));
    // Chunk boundaries.  Big batches ramp up and down (CH/8, CH/4, CH/2, CH ... CH, CH/2, CH/4, CH/8): nothing overlaps the
    // staging of the first chunk nor the copy-out and unpacking of the last one, so those two are small.
    std::vector<size_t> off{0};
    {
        std::vector<size_t> head, tail;
        size_t left = B;
        if (B >= 6 * CH && CH >= 2048) {
            for (size_t d = 8; d >= 2; d /= 2) {
                head.push_back(CH / d);
                tail.insert(tail.begin(), CH / d);
                left -= 2 * (CH / d);
            }
        }
        for (size_t h : head) off.push_back(off.back() + h);
        while (left > 0) {
            const size_t nfc = std::min(CH, left);
            off.push_back(off.back() + nfc);
            left -= nfc;
        }
        for (size_t t : tail) off.push_back(off.back() + t);
    }
    const size_t nch = off.size() - 1;
    const size_t chf = std::min(B, CH);
    for (int i = 0; i < 2; ++i) {
        if ((rc = ensure(c, c->in2[i], chf * W * sizeof(double)))) return rc;
        if ((rc = ensure(c, c->bits2[i], chf * NW * sizeof(uint32_t)))) return rc;
    }
    const bool staged = nch >= 3;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(c, c->h_bits[i].ensure(chf * NW * sizeof(uint32_t)));
        if (staged) HIP_TRY(c, c->h_in[i].ensure(chf * W * sizeof(double)));
    }
    if (!c->copy_stream) {
        HIP_TRY(c, c->copy_stream.create(hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(c, c->ev_in[i].create(hipEventDisableTiming));
            HIP_TRY(c, c->ev_free[i].create(hipEventDisableTiming));
            HIP_TRY(c, c->ev_out[i].create(hipEventDisableTiming));
        }
    }
    auto stage_chunk = [&](size_t k) {    // caller's rows of chunk k -> pinned h_in[k & 1], four threads
        const size_t f0 = off[k], nf = off[k + 1] - off[k];
        const double *src = in + f0 * (size_t)W;
        double *dst = c->h_in[k & 1];
        const unsigned nthr = HOST_THREADS;
        auto part = [=](unsigned t) {
            const size_t a = nf * t / nthr, b = nf * (t + 1) / nthr;
            std::memcpy(dst + a * (size_t)W, src + a * (size_t)W, (b - a) * (size_t)W * sizeof(double));
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nthr; ++t) pool.emplace_back(part, t);
        part(0);
        for (auto &th : pool) th.join();
    };
    std::thread worker;
    auto unpack_chunk = [&](size_t k) {   // decisions of chunk k: pinned words -> caller's int u_hat[][N]
        const size_t f0 = off[k], nf = off[k + 1] - off[k];
        const uint32_t *hb = c->h_bits[k & 1];
        const unsigned nthr = (unsigned)std::max<size_t>(1, std::min<size_t>(HOST_THREADS, nf / 1024));
        auto part = [=](unsigned t) {
            const size_t a = nf * t / nthr, b = nf * (t + 1) / nthr;
            for (size_t f = a; f < b; ++f) unpack_words(hb + f * NW, NW, u_hat + (f0 + f) * (size_t)N);
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nthr; ++t) pool.emplace_back(part, t);
        part(0);
        for (auto &th : pool) th.join();
    };
    auto fail_join = [&](int code) {
        if (worker.joinable()) worker.join();
        (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamSynchronize(c->stream);
        return code;
    };
    for (size_t k = 0; k < nch; ++k) {
        const int s = (int)(k & 1);
        const size_t f0 = off[k], nf = off[k + 1] - off[k];
        // the decode of chunk k-2 must be done with in2[s] before it is overwritten
        if (k >= 2 && hipStreamWaitEvent(c->copy_stream, c->ev_free[s], 0) != hipSuccess) return fail_join(POLAR_EDEVICE);
        const double *h_src = in + f0 * (size_t)W;
        if (staged) {
            // h_in[s] was the source of chunk k-2's DMA: that copy must have left it (ev_in[s] is recorded behind it)
            if (k >= 2 && hipEventSynchronize(c->ev_in[s]) != hipSuccess) return fail_join(POLAR_EDEVICE);
            stage_chunk(k);
            h_src = c->h_in[s];
        }
        if (hipMemcpyAsync(c->in2[s].p, h_src, nf * W * sizeof(double), hipMemcpyHostToDevice,
                           c->copy_stream) != hipSuccess) return fail_join(POLAR_EDEVICE);
        if (hipEventRecord(c->ev_in[s], c->copy_stream) != hipSuccess) return fail_join(POLAR_EDEVICE);
        if (hipStreamWaitEvent(c->stream, c->ev_in[s], 0) != hipSuccess) return fail_join(POLAR_EDEVICE);
        // h_bits[s] / bits2[s] were last used by chunk k-2, whose unpacking ran during the copy above
        if (worker.joinable()) worker.join();
        DecodeOut o = advanced(c, staging, f0);
        o.bits = (uint32_t *)c->bits2[s].p;
        if ((rc = decode_device_impl(c, c->in2[s].p, 0, sigma, nf, o, d_frozen))) return fail_join(rc);
        if (hipEventRecord(c->ev_free[s], c->stream) != hipSuccess) return fail_join(POLAR_EDEVICE);
        if (hipMemcpyAsync(c->h_bits[s], c->bits2[s].p, nf * NW * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) !=
            hipSuccess) return fail_join(POLAR_EDEVICE);
        if (hipEventRecord(c->ev_out[s], c->stream) != hipSuccess) return fail_join(POLAR_EDEVICE);
        // chunk k-1 was decoded while chunk k crossed PCIe: unpack it in the background during the next copy
        if (k >= 1) {
            if (hipEventSynchronize(c->ev_out[s ^ 1]) != hipSuccess) return fail_join(POLAR_EDEVICE);
            worker = std::thread(unpack_chunk, k - 1);
        }
    }
    if (worker.joinable()) worker.join();
    HIP_TRY(c, hipEventSynchronize(c->ev_out[(nch - 1) & 1]));
    unpack_chunk(nch - 1);
    if (h.pm) HIP_TRY(c, hipMemcpyAsync(h.pm, c->pm.p, B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h.flags) HIP_TRY(c, hipMemcpyAsync(h.flags, c->flags.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    for (const auto &q : opt)
        if (q.host) HIP_TRY(c, hipMemcpyAsync(q.host, q.dev->p, B * q.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return POLAR_OK;
}

}  // namespace polar_host

extern "C" {

static_assert(polar::BP_FLAG_CONVERGED == POLAR_FLAG_BP_CONVERGED, "kernel and C ABI flag bit");

const char *polar_version(void) { return "polar_hip 0.1 (gfx950)"; }

const char *polar_strerror(int code)
{
    switch (code) {
    case POLAR_OK: return "ok";
    case POLAR_EINVAL: return "invalid argument or unsupported configuration";
    case POLAR_ENOMEM: return "out of memory";
    case POLAR_EDEVICE: return "HIP runtime error";
    case POLAR_ENOKERNEL: return "no kernel instantiation for this shape";
    }
    return "unknown error";
}

const char *polar_last_error(const polar_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int polar_create(const polar_cfg *cfg, polar_ctx **out)
{
    if (!cfg || !out) return POLAR_EINVAL;
    *out = nullptr;
    const int N = cfg->N;
    if (N < 32 || N > 4096 || (N & (N - 1))) return POLAR_EINVAL;
    if (cfg->K < 1 || cfg->crc_r < 0 || cfg->crc_r > 32 || cfg->K + cfg->crc_r > N) return POLAR_EINVAL;
    if (cfg->algo < POLAR_ALGO_SC || cfg->algo > POLAR_ALGO_BPL) return POLAR_EINVAL;
    if (cfg->dtype != POLAR_F64 && cfg->dtype != POLAR_F32 && cfg->dtype != POLAR_Q8) return POLAR_EINVAL;
    int L = cfg->L;
    if (cfg->algo == POLAR_ALGO_SC || cfg->algo == POLAR_ALGO_BP || cfg->algo == POLAR_ALGO_SCF || cfg->algo == POLAR_ALGO_SCAN ||
        cfg->algo == POLAR_ALGO_BPL)
        L = 1;
    if (L < 1 || L > 256 || (L & (L - 1))) return POLAR_EINVAL;
    if (L > 32 && cfg->dtype == POLAR_Q8) return POLAR_EINVAL;   // wide lists (L = 64 / 128 / 256): float and double only
    const bool crc_optional = cfg->algo == POLAR_ALGO_BPL && cfg->crc_r == 0;   // BP list decoding: crc_r = 0 means none
    if (has_crc(cfg->algo) && !crc_optional && (cfg->crc_r < 1 || !cfg->crc_taps || cfg->n_taps < 2)) return POLAR_EINVAL;
    if ((cfg->algo == POLAR_ALGO_BP || cfg->algo == POLAR_ALGO_BPL) && cfg->bp_iters < 1) return POLAR_EINVAL;
    if (cfg->algo == POLAR_ALGO_SCF && N > 2048) return POLAR_ENOKERNEL;   // one codeword per lane: N <= 2048
    if (cfg->algo == POLAR_ALGO_SCAN && N > polar::SCAN_MAX_N) return POLAR_ENOKERNEL;
    // fixed-point min-sum: SC / SCL / CA-SCL up to N = 1024
    if (cfg->dtype == POLAR_Q8 && (N > 1024 || (cfg->algo != POLAR_ALGO_SC && cfg->algo != POLAR_ALGO_SCL && cfg->algo != POLAR_ALGO_CASCL)))
        return POLAR_ENOKERNEL;
    if (L > 32 && (long long)N * L > 65536) return POLAR_ENOKERNEL;   // k_scl_wide: its pointer table holds log2 L * log2 N <= 64 bits

    polar_ctx *c = new (std::nothrow) polar_ctx();
    if (!c) return POLAR_ENOMEM;
    c->cfg = *cfg;
    c->cfg.L = L;
    c->n = 0;
    while ((1 << c->n) < N) ++c->n;
    c->logL = 0;
    while ((1 << c->logL) < L) ++c->logL;
    c->NW = N / 32;
    const int r = has_crc(cfg->algo) ? cfg->crc_r : 0;
    c->cfg.crc_r = r;
    c->A = cfg->K + r;
    if (r > 0) {
        c->taps.assign(cfg->crc_taps, cfg->crc_taps + cfg->n_taps);
        bool has0 = false, hasr = false;
        for (int t : c->taps) {
            if (t < 0 || t > r) { delete c; return POLAR_EINVAL; }
            has0 |= (t == 0);
            hasr |= (t == r);
        }
        if (!has0 || !hasr) { delete c; return POLAR_EINVAL; }
    }
    c->cfg.crc_taps = c->taps.empty() ? nullptr : c->taps.data();
    if (cfg->info_order) {
        c->info_order.assign(cfg->info_order, cfg->info_order + c->A);
    } else {
        std::vector<int> q = default_order(N);
        c->info_order.assign(q.end() - c->A, q.end());  // I[i] = Q[N-(K+r)+i], CASCL_1024_L8.c:214-217
    }
    c->cfg.info_order = c->info_order.data();
    c->frozen.assign(N, 1);
    for (int i = 0; i < c->A; ++i) {
        const int j = c->info_order[i];
        if (j < 0 || j >= N || c->frozen[j] == 0) { delete c; return POLAR_EINVAL; }
        c->frozen[j] = 0;
    }
    c->h_crc_tab = make_crc_table(N, r, c->taps, c->info_order);
    c->scf_T = std::min(8, c->A);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        delete c;
        return POLAR_EDEVICE;
    }
    DeviceGuard guard(cfg->device);   // the calling thread's current device is restored on return
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, cfg->device);
    if (e != hipSuccess) {
        delete c;
        return POLAR_EDEVICE;
    }
    c->num_cu = prop.multiProcessorCount;
    auto cleanup = [&](int rc) {
        polar_destroy(c);
        return rc;
    };
    if (c->stream.create(hipStreamNonBlocking) != hipSuccess) return cleanup(POLAR_EDEVICE);
    if (c->ev0.create(hipEventDefault) != hipSuccess || c->ev1.create(hipEventDefault) != hipSuccess) return cleanup(POLAR_EDEVICE);
    std::vector<uint32_t> fw = pack_mask(c->frozen.data(), N, false);
    std::vector<uint32_t> iw = pack_mask(c->frozen.data(), N, true);
    c->cfg.crc_systematic = (cfg->crc_systematic && r > 0) ? 1 : 0;
    if (c->cfg.crc_systematic) {
        // error metric over the K payload positions I[r..K+r) only (CASCL_1024_sys.c:820-821)
        std::fill(iw.begin(), iw.end(), 0u);
        for (int i = r; i < c->A; ++i) iw[c->info_order[i] >> 5] |= 1u << (c->info_order[i] & 31);
        // generator rows D^(r+k) mod g (the literal Gc[K][r] of CASCL_1024_sys.c:48-561), bit j = coefficient of D^j
        std::vector<uint32_t> rows((size_t)cfg->K);
        uint64_t glow = 0;
        for (int t : c->taps)
            if (t < r) glow |= 1ull << t;
        const uint64_t top = 1ull << r;
        uint64_t rem = glow;   // D^r mod g
        for (int k = 0; k < cfg->K; ++k) {
            rows[(size_t)k] = (uint32_t)rem;
            rem <<= 1;
            if (rem & top) rem = (rem ^ top) ^ glow;
        }
        if (int rc = c->d_gc_rows.upload(rows.data(), rows.size())) return cleanup(rc);
    }
    // both allocations before either copy: out of memory is reported before a failed copy
    if (c->d_frozen.alloc((size_t)c->NW) != hipSuccess || c->d_info.alloc((size_t)c->NW) != hipSuccess) return cleanup(POLAR_ENOMEM);
    if (int rc = c->d_frozen.upload(fw.data(), (size_t)c->NW)) return cleanup(rc);
    c->fill_end = fill_phase_end(N, c->frozen.data());
    if (int rc = c->d_info.upload(iw.data(), (size_t)c->NW)) return cleanup(rc);
    if (r > 0)
        if (int rc = upload_crc_tables(c, c->h_crc_tab)) return cleanup(rc);
    if (cfg->algo == POLAR_ALGO_BPL) {   // every attempt stops by rule G; the default list: min(n, 8) cyclic shifts
        c->bp_stop = POLAR_BP_STOP_G;
        const int P = std::min(c->n, 8);
        std::vector<int> perms((size_t)P * c->n);
        polar_bpl_cyclic_graphs(c->n, P, perms.data());
        if (int rc = polar_bpl_set_graphs(c, perms.data(), P)) return cleanup(rc);
    }
    refresh_kernel_name(c);
    *out = c;
    return POLAR_OK;
}

void polar_destroy(polar_ctx *c)
{
    if (!c) return;
    DeviceGuard guard(c->cfg.device);
    for (hipStream_t st : {c->stream.get(), c->copy_stream.get(), c->lane_b.stream.get()})
        if (st) (void)hipStreamSynchronize(st);
    for (polar_ctx *s : c->stage_ctx) polar_destroy(s);   // they borrow c->stream (synchronized above)
    delete c;   // every member releases what it owns, on c's device
}

int polar_set_stream(polar_ctx *c, void *s)
{
    if (!c) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    if (c->stream.is_owned()) (void)hipStreamSynchronize(c->stream);
    c->stream.adopt((hipStream_t)s);   // destroys the stream polar_create made; the caller's is never destroyed here
    return POLAR_OK;
}

void *polar_get_stream(polar_ctx *c) { return c ? (void *)c->stream.get() : nullptr; }

int polar_synchronize(polar_ctx *c)
{
    if (!c) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return POLAR_OK;
}

int polar_ctx_info(const polar_ctx *c, int *N, int *K, int *A, int *L, int *algo, int *dtype)
{
    if (!c) return POLAR_EINVAL;
    if (N) *N = c->cfg.N;
    if (K) *K = c->cfg.K;
    if (A) *A = c->A;
    if (L) *L = c->cfg.L;
    if (algo) *algo = c->cfg.algo;
    if (dtype) *dtype = c->cfg.dtype;
    return POLAR_OK;
}

int polar_info_order(const polar_ctx *c, int *out, int n)
{
    if (!c || !out || n < c->A) return POLAR_EINVAL;
    for (int i = 0; i < c->A; ++i) out[i] = c->info_order[i];
    return POLAR_OK;
}

const char *polar_kernel_name(const polar_ctx *c) { return c ? c->kernel_name.c_str() : ""; }

int polar_rm_recover_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, void *d_out)
{
    if (!c || c->rm_mode == POLAR_RM_NONE || !d_in || !d_out || B > kMaxBatch) return POLAR_EINVAL;
    const size_t esz = in_is_f32 ? 4 : 8;
    if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) % esz) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return polar_tu::rm_recover(c, d_in, in_is_f32 != 0, sigma, B, d_out);
}

int polar_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits,
                        double *d_pm, uint32_t *d_flags)
{
    if (!c) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, {.bits = d_bits, .pm = d_pm, .flags = d_flags}, c->d_frozen);
}

int polar_decode_batch(polar_ctx *c, const double *llr_in, const unsigned char *frozen_mask, size_t B, int *u_hat,
                       double *pm_out, unsigned *flags)
{
    return host_batch(c, llr_in, 0.0, frozen_mask, B, {.u_hat = u_hat, .pm = pm_out, .flags = flags});
}

int polar_decode_batch_y(polar_ctx *c, const double *y, double sigma, size_t B, int *u_hat, double *pm_out,
                         unsigned *flags)
{
    if (!(sigma > 0)) return POLAR_EINVAL;
    return host_batch(c, y, sigma, nullptr, B, {.u_hat = u_hat, .pm = pm_out, .flags = flags});
}

int polar_decode(polar_ctx *c, const double *y, double sigma, int *u_hat)
{
    if (!(sigma > 0)) return POLAR_EINVAL;
    return host_batch(c, y, sigma, nullptr, 1, {.u_hat = u_hat});
}

int polar_decode_llr(const double *llr_in, const unsigned char *frozen_mask, int N, int L, int *u_hat)
{
    if (!llr_in || !frozen_mask || !u_hat) return POLAR_EINVAL;
    if (N < 32 || N > 4096 || (N & (N - 1)) || L < 1 || L > 32 || (L & (L - 1))) return POLAR_EINVAL;   // before frozen_mask[0..N) is read
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return POLAR_EDEVICE;
    static std::mutex mu;
    static std::vector<std::pair<std::vector<unsigned char>, polar_ctx *>> cache;
    std::lock_guard<std::mutex> lock(mu);
    std::vector<unsigned char> key(frozen_mask, frozen_mask + N);   // key = (mask, L, device): a ctx is bound to one GPU
    key.push_back((unsigned char)L);
    key.push_back((unsigned char)dev);
    polar_ctx *c = nullptr;
    for (auto &kv : cache)
        if (kv.first == key) c = kv.second;
    if (!c) {
        std::vector<int> info;
        for (int j = 0; j < N; ++j)
            if (!frozen_mask[j]) info.push_back(j);
        if (info.empty()) return POLAR_EINVAL;
        polar_cfg g{};
        g.N = N; g.K = (int)info.size(); g.L = L;
        g.algo = (L == 1) ? POLAR_ALGO_SC : POLAR_ALGO_SCL;
        g.info_order = info.data();
        g.dtype = POLAR_F64;
        g.device = dev;
        int rc = polar_create(&g, &c);
        if (rc) return rc;
        if (cache.size() >= 8) {
            polar_destroy(cache.front().second);
            cache.erase(cache.begin());
        }
        cache.emplace_back(key, c);
    }
    return host_batch(c, llr_in, 0.0, nullptr, 1, {.u_hat = u_hat});
}

#ifdef POLAR_TESTING
// ---- include/polar_hip_testing.h ----------------------------------------------------------------------------
int polar_testing_select_kernel(polar_ctx *c, int variant)
{
    if (!c || variant < POLAR_TEST_KERNEL_AUTO || variant > POLAR_TEST_KERNEL_FOUR_PER_WAVE) return POLAR_EINVAL;
    c->force_generic = (variant == POLAR_TEST_KERNEL_GENERIC || variant == POLAR_TEST_KERNEL_GENERIC_SPILL);
    c->force_spill = (variant == POLAR_TEST_KERNEL_GENERIC_SPILL || variant == POLAR_TEST_KERNEL_BIG);
    c->use_fast2 = (variant != POLAR_TEST_KERNEL_ONE_PER_WAVE);
    c->use_fast4 = (variant == POLAR_TEST_KERNEL_FOUR_PER_WAVE);
    refresh_kernel_name(c);
    return POLAR_OK;
}

int polar_testing_big_split(polar_ctx *c, int split)
{
    if (!c || (split != 0 && split != 35 && split != 46 && split != 57 && split != 351 && split != 371))
        return POLAR_EINVAL;
    c->big_split = split;
    return POLAR_OK;
}

int polar_testing_chunk_bytes(polar_ctx *c, size_t bytes)
{
    if (!c) return POLAR_EINVAL;
    c->chunk_bytes = bytes ? bytes : kChunkBytes;
    return POLAR_OK;
}

int polar_testing_resident_blocks(polar_ctx *c, int blocks)
{
    if (!c || blocks < 0) return POLAR_EINVAL;
    c->resident_blocks = blocks;
    sync_stage_ctx(c);
    return POLAR_OK;
}

int polar_testing_last_plan(const polar_ctx *c, int *grid, long long *jobs, int *jobs_per_block, int *queued)
{
    if (!c) return POLAR_EINVAL;
    if (grid) *grid = c->last_plan.grid;
    if (jobs) *jobs = c->last_plan.jobs;
    if (jobs_per_block) *jobs_per_block = c->last_plan.jobs_per_block;
    if (queued) *queued = c->last_plan.queued;
    return POLAR_OK;
}

int polar_testing_last_stride(const polar_ctx *c, int *grid, long long *need)
{
    if (!c) return POLAR_EINVAL;
    if (grid) *grid = c->last_stride.grid;
    if (need) *need = c->last_stride.need;
    return POLAR_OK;
}
#endif  // POLAR_TESTING

int polar_time_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B,
                             uint32_t *d_bits, int reps, float *ms)
{
    if (!c || !ms || reps < 1) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < reps; ++i) {
        int rc = decode_device_impl(c, d_in, in_is_f32, sigma, B, {.bits = d_bits}, c->d_frozen);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    float t = 0;
    HIP_TRY(c, hipEventElapsedTime(&t, c->ev0, c->ev1));
    *ms = t / (float)reps;
    return POLAR_OK;
}

}  // extern "C"
