// h_decoders.hip -- the decoders around the fixed one: adaptive CA-SCL, SC-Flip and its dynamic rule, BP list decoding,
// SCAN; the polar_bp_*, polar_cascl_*, polar_scf_*, polar_bpl_* and polar_scan_* entry points.
#include "polar_hostlib.h"

using namespace polar_host;

namespace {

// Entry points whose host reads a count back between launches refuse a stream that is being captured.
int refuse_capture(polar_ctx *c)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(c, hipStreamIsCapturing(c->stream, &cs));
    return cs != hipStreamCaptureStatusNone ? POLAR_EINVAL : POLAR_OK;
}

// The compaction buffers for lists of at most n frames: one list, its block counts and the device count; pingpong: the second
// list and the staged flags of the decoders whose later passes compact what the pass before left open.
int ensure_compaction(polar_ctx *c, size_t n, bool pingpong)
{
    int rc;
    if ((rc = ensure(c, c->ad_idx[0], n * sizeof(uint32_t)))) return rc;
    for (Buf *b : {&c->ad_idx[1], &c->ad_sflags})
        if (pingpong && (rc = ensure(c, *b, n * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->ad_blk, 2 * polar_tu::ad_blocks(n) * sizeof(uint32_t)))) return rc;
    return ensure(c, c->ad_cnt, sizeof(uint32_t));
}

// The frames of idx_in[0 .. n) (null: frames 0 .. n) whose flags lack a bit of `need`, in order, to idx_out; *count: how many,
// read back -- one 4-byte copy and a stream sync.
int compact_open(polar_ctx *c, const uint32_t *flags, const uint32_t *idx_in, size_t n, uint32_t need, uint32_t *idx_out, size_t *count)
{
    if (int rc = polar_tu::ad_compact(c, flags, idx_in, n, need, (uint32_t *)c->ad_blk.p, idx_out, (uint32_t *)c->ad_cnt.p)) return rc;
    uint32_t h = 0;
    HIP_TRY(c, hipMemcpyAsync(&h, c->ad_cnt.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *count = h;
    return POLAR_OK;
}

// sigma_pi(j) = sum over b of ((j >> b) & 1) << pi[b] (include/polar_hip.h, BP list decoding)
int bpl_sigma(const int *pi, int n, int j)
{
    int v = 0;
    for (int b = 0; b < n; ++b) v |= ((j >> b) & 1) << pi[b];
    return v;
}

}  // namespace

namespace polar_host {

// Adaptive CA-SCL (polar_cascl_set_stages): stage 0 decodes the whole batch into the caller's outputs; every later stage
// gathers the rows of the frames that failed the stage before (stable compaction of the flags words), decodes them with
// its list size and scatters the results back.  One 4-byte copy and a stream sync per later stage: the failing count.
int cascl_adaptive(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits,
                   double *d_pm, uint32_t *d_flags, uint32_t *d_list)
{
    int rc;
    if ((rc = refuse_capture(c))) return rc;   // the per-stage syncs cannot be captured
    sync_stage_ctx(c);
    const std::vector<int> &st = c->cascl_stages;
    const int m = (int)st.size(), N = c->cfg.N, NW = c->NW;
    const size_t row = (size_t)N * (in_is_f32 ? 4 : 8);
    // later stages run in chunks of at most 256 MiB of gathered input
    const size_t CH = chunk_rows(c, B, row);
    // every buffer of the call, before its first launch
    if (!d_flags) {
        if ((rc = ensure(c, c->ad_flags, B * sizeof(uint32_t)))) return rc;
        d_flags = (uint32_t *)c->ad_flags.p;
    }
    if ((rc = ensure_compaction(c, B, true))) return rc;
    if ((rc = ensure(c, c->ad_in, CH * row))) return rc;
    if ((rc = ensure(c, c->ad_bits, CH * NW * sizeof(uint32_t)))) return rc;
    if (d_pm && (rc = ensure(c, c->ad_pm, CH * sizeof(double)))) return rc;

    polar_ctx *s0 = c->stage_ctx[0] ? c->stage_ctx[0] : c;
    if ((rc = decode_fixed(s0, d_in, in_is_f32, sigma, B, d_bits, d_pm, d_flags, s0->d_frozen))) return rc;
    c->last_plan = s0->last_plan;   // a stage context's plan is read through its owner (polar_testing_last_plan)
    if (st[0] == 1 && (rc = polar_tu::ad_crc_check(c, d_bits, c->d_crc_tab, d_flags, B))) return rc;
    if (d_list) HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_list), st[0], B, c->stream));
    const uint32_t *cur_idx = nullptr, *cur_flags = d_flags;
    size_t n = B;
    for (int s = 1; s < m; ++s) {
        uint32_t *idx = (uint32_t *)c->ad_idx[(s - 1) & 1].p;
        if ((rc = compact_open(c, cur_flags, cur_idx, n, POLAR_FLAG_CRC_PASS, idx, &n))) return rc;
        if (n == 0) break;
        polar_ctx *sc = c->stage_ctx[(size_t)s] ? c->stage_ctx[(size_t)s] : c;
        uint32_t *sflags = (uint32_t *)c->ad_sflags.p;
        for (size_t off = 0; off < n; off += CH) {
            const size_t nc = std::min(CH, n - off);
            if ((rc = polar_tu::ad_gather(c, d_in, c->ad_in.p, idx + off, nc, row))) return rc;
            if ((rc = decode_fixed(sc, c->ad_in.p, in_is_f32, sigma, nc, (uint32_t *)c->ad_bits.p,
                                   d_pm ? (double *)c->ad_pm.p : nullptr, sflags + off, sc->d_frozen)))
                return rc;
            c->last_plan = sc->last_plan;
            if ((rc = polar_tu::ad_scatter(c, (uint32_t *)c->ad_bits.p, (double *)c->ad_pm.p, sflags + off, idx + off, nc,
                                           d_bits, d_pm, d_flags, d_list, st[(size_t)s])))
                return rc;
        }
        cur_idx = idx;
        cur_flags = sflags;
    }
    return POLAR_OK;
}

// CRC-aided SC-Flip (POLAR_ALGO_SCF, include/polar_hip.h).  Pass A decodes every frame with SC and checks its CRC; the
// frames that fail are compacted in a stable order (the adaptive rule's glue), decoded once more to find their T least
// reliable information decisions, and pass B runs all T single-flip attempts of every failing frame at once, one lane per
// (frame, attempt), in chunks of at most 256 MiB of decisions; k_scf_resolve keeps the first attempt that passes.  One
// 4-byte copy and a stream sync: the failing count.
//
// With the dynamic rule (polar_scf_set_dynamic) the steps are: check, compact, record (SCF_RECORD_M: each failing frame's
// T_1 best M(0, i), which k_scf_merge turns into the level-1 sets), then per level k: run the frame's T_k sets at once
// (SCF_FLIPREC below omega, keeping each pair's T_{k+1} best extensions; SCF_FLIPSET at omega) in chunks of at most 256 MiB
// of decisions, k_scf_resolve_sets, and below omega: compact the frames that still fail (4-byte copy and sync) and merge
// their pairs' lists into the sets of level k + 1.  d_sets (nullable) [B][3]: the reported set; a static ctx fills it too.
int scf_decode(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits, double *d_pm,
               uint32_t *d_flags, uint32_t *d_attempts, int32_t *d_sets)
{
    if (!d_in || !d_bits || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    int rc;
    if ((rc = refuse_capture(c))) return rc;   // the host reads the failing count
    const int T = c->scf_T, NW = c->NW;
    const int omega = T > 0 ? c->scf_omega : 0;
    int Tk[polar::SCF_MAX_ORDER + 1] = {T, 0, 0, 0}, Ttot = T;
    for (int k = 1; k < omega; ++k) Ttot += (Tk[k] = c->scf_Tk[k]);
    const bool r32 = c->cfg.dtype == POLAR_F32, in32 = in_is_f32 != 0;
    if (!d_flags) {
        if ((rc = ensure(c, c->ad_flags, B * sizeof(uint32_t)))) return rc;
        d_flags = (uint32_t *)c->ad_flags.p;
    }
    if (d_sets) HIP_TRY(c, hipMemsetAsync(d_sets, 0xFF, B * polar::SCF_MAX_ORDER * sizeof(int32_t), c->stream));   // -1
    polar::ScfParams P{};
    P.in = d_in; P.sigma = sigma; P.out_bits = d_bits; P.pm = d_pm; P.flags = d_flags; P.attempts = d_attempts;
    P.frozen = c->d_frozen; P.crc_tab = c->d_crc_tab;
    P.N = c->cfg.N; P.n = c->n; P.B = (int)B; P.T = Ttot;   // pass A writes attempts = 0 / P.T
    if ((rc = polar_tu::scf_lanes(c, P, polar::SCF_CHECK, r32, in32))) return rc;
    P.T = T;
    if (T == 0) return POLAR_OK;
    if ((rc = ensure_compaction(c, B, false))) return rc;
    uint32_t *idx = (uint32_t *)c->ad_idx[0].p;
    size_t n = 0, h = 0;
    if ((rc = compact_open(c, d_flags, nullptr, B, POLAR_FLAG_CRC_PASS, idx, &n))) return rc;
    if (n == 0) return POLAR_OK;
    if (omega > 0) {
        const size_t rsz = r32 ? 4 : 8, pair_bytes = (size_t)NW * sizeof(uint32_t);
        size_t pairs = 0, ents = 0, chmax = 0;   // per level: pairs n T_k, list entries n T_k T_{k+1}; pairs per chunk
        for (int k = 0; k < omega; ++k) {
            pairs = std::max(pairs, n * (size_t)Tk[k]);
            ents = std::max(ents, n * (size_t)(k ? Tk[k - 1] : 1) * (size_t)Tk[k]);
            chmax = std::max(chmax, chunk_rows(c, n, pair_bytes * (size_t)Tk[k], 1) * (size_t)Tk[k]);
        }
        // every buffer of the call, before the first launch of the rule
        for (Buf *b : {&c->scf_sets[0], &c->scf_sets[1]})
            if ((rc = ensure(c, *b, pairs * polar::SCF_MAX_ORDER * sizeof(uint16_t)))) return rc;
        if ((rc = ensure(c, c->scf_lkey, ents * rsz)) || (rc = ensure(c, c->scf_lpos, ents * sizeof(uint16_t))) ||
            (rc = ensure(c, c->scf_lcnt, pairs * sizeof(uint32_t))) || (rc = ensure(c, c->scf_spass, n * sizeof(uint32_t))) ||
            (rc = ensure(c, c->scf_surv, n * sizeof(uint32_t))) || (rc = ensure(c, c->ad_idx[1], n * sizeof(uint32_t))) ||
            (rc = ensure(c, c->scf_bits, chmax * pair_bytes)) || (rc = ensure(c, c->scf_pass, chmax * sizeof(uint32_t))))
            return rc;
        uint16_t *lpos = (uint16_t *)c->scf_lpos.p;
        uint32_t *lcnt = (uint32_t *)c->scf_lcnt.p, *spass = (uint32_t *)c->scf_spass.p, *surv = (uint32_t *)c->scf_surv.p;
        polar::ScfParams R = P;
        R.out_bits = nullptr; R.pm = nullptr; R.flags = nullptr; R.attempts = nullptr;
        R.mc = c->scf_c; R.tau = c->scf_tau; R.lkey = c->scf_lkey.p; R.lpos = lpos; R.lcnt = lcnt;
        // record: attempt 0 again, each failing frame's T_1 smallest (M(0, i), i); the level-1 sets are these positions
        R.idx = idx; R.B = (int)n; R.T = 1; R.Tn = Tk[0];
        if ((rc = polar_tu::scf_lanes(c, R, polar::SCF_RECORD_M, r32, in32))) return rc;
        int cur = 0, base = 0;
        if ((rc = polar_tu::scf_merge(c, r32, c->scf_lkey.p, lpos, lcnt, nullptr, nullptr, nullptr, n, 1, Tk[0],
                                      (uint16_t *)c->scf_sets[cur].p, nullptr)))
            return rc;
        for (int k = 0; k < omega; ++k) {   // level k + 1
            const bool last = k + 1 == omega;
            const size_t Tl = (size_t)Tk[k], Tnx = (size_t)Tk[k + 1];
            uint16_t *sets = (uint16_t *)c->scf_sets[cur].p;
            const size_t CH = chunk_rows(c, n, pair_bytes * Tl, 1);
            for (size_t off = 0; off < n; off += CH) {
                const size_t nc = std::min(CH, n - off);
                polar::ScfParams F = R;
                F.idx = idx + off; F.flips = sets + off * Tl * polar::SCF_MAX_ORDER; F.B = (int)(nc * Tl); F.T = (int)Tl;
                F.Tn = (int)Tnx;
                F.lkey = (char *)c->scf_lkey.p + off * Tl * Tnx * rsz; F.lpos = lpos + off * Tl * Tnx; F.lcnt = lcnt + off * Tl;
                F.out_bits = (uint32_t *)c->scf_bits.p; F.flags = (uint32_t *)c->scf_pass.p;
                if ((rc = polar_tu::scf_lanes(c, F, last ? polar::SCF_FLIPSET : polar::SCF_FLIPREC, r32, in32))) return rc;
                if ((rc = polar_tu::scf_resolve_sets(c, (uint32_t *)c->scf_pass.p, (uint32_t *)c->scf_bits.p, idx + off, nc,
                                                     (int)Tl, F.flips, polar::SCF_MAX_ORDER, k + 1, base, d_bits, d_flags,
                                                     d_attempts, d_sets, last ? nullptr : spass + off)))
                    return rc;
            }
            if (last) break;
            base += (int)Tl;
            if ((rc = compact_open(c, spass, nullptr, n, 1u, surv, &h))) return rc;
            if (h == 0) break;
            uint32_t *nidx = (uint32_t *)c->ad_idx[idx == (uint32_t *)c->ad_idx[0].p ? 1 : 0].p;
            if ((rc = polar_tu::scf_merge(c, r32, c->scf_lkey.p, lpos, lcnt, sets, surv, idx, h, (int)Tl, (int)Tnx,
                                          (uint16_t *)c->scf_sets[cur ^ 1].p, nidx)))
                return rc;
            idx = nidx;
            n = h;
            cur ^= 1;
        }
        return POLAR_OK;
    }
    // the flip list of every failing frame: attempt 0 again, its T smallest |lambda_j|
    if ((rc = ensure(c, c->scf_flips, n * (size_t)T * sizeof(uint16_t)))) return rc;
    uint16_t *flips = (uint16_t *)c->scf_flips.p;
    polar::ScfParams R = P;
    R.out_bits = nullptr; R.pm = nullptr; R.flags = nullptr; R.attempts = nullptr;
    R.idx = idx; R.flips = flips; R.B = (int)n;
    if ((rc = polar_tu::scf_lanes(c, R, polar::SCF_RECORD, r32, in32))) return rc;
    // pass B: frames [off, off + nc) of the list, T pairs each
    const size_t pair_bytes = (size_t)NW * sizeof(uint32_t);
    const size_t CH = chunk_rows(c, n, pair_bytes * (size_t)T, 1);
    if ((rc = ensure(c, c->scf_bits, CH * (size_t)T * pair_bytes))) return rc;
    if ((rc = ensure(c, c->scf_pass, CH * (size_t)T * sizeof(uint32_t)))) return rc;
    for (size_t off = 0; off < n; off += CH) {
        const size_t nc = std::min(CH, n - off);
        polar::ScfParams F = R;
        F.idx = idx + off; F.flips = flips + off * (size_t)T; F.B = (int)(nc * (size_t)T);
        F.out_bits = (uint32_t *)c->scf_bits.p; F.flags = (uint32_t *)c->scf_pass.p;
        if ((rc = polar_tu::scf_lanes(c, F, polar::SCF_FLIP, r32, in32))) return rc;
        if (d_sets)
            rc = polar_tu::scf_resolve_sets(c, (uint32_t *)c->scf_pass.p, (uint32_t *)c->scf_bits.p, idx + off, nc, T, F.flips,
                                            1, 1, 0, d_bits, d_flags, d_attempts, d_sets, nullptr);
        else
            rc = polar_tu::scf_resolve(c, (uint32_t *)c->scf_pass.p, (uint32_t *)c->scf_bits.p, idx + off, nc, T, d_bits,
                                       d_flags, d_attempts);
        if (rc) return rc;
    }
    return POLAR_OK;
}

// BP list decoding (POLAR_ALGO_BPL, include/polar_hip.h).  Attempt 0 runs on the whole batch: with pi_0 = identity straight
// into the caller's outputs (no permutation kernel), else through the staging buffers like every later attempt.  A later
// attempt compacts the frames that are still open (the adaptive rule's glue, asked for CONVERGED and, with a CRC, CRC_PASS),
// gathers their rows permuted, runs the ctx's BP kernel with the permuted frozen mask and scatters the accepted frames back
// un-permuted, in chunks of at most 256 MiB of gathered rows.  One 4-byte copy and a stream sync per later attempt.
int bpl_decode(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits, double *d_pm,
               uint32_t *d_flags, uint32_t *d_iters, uint32_t *d_graph, uint32_t *d_total)
{
    if (!d_in || !d_bits || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    int rc;
    if ((rc = refuse_capture(c))) return rc;   // the host reads the count of open frames
    const int P = (int)c->bpl_ident.size(), N = c->cfg.N, NW = c->NW;
    const bool crc = c->cfg.crc_r > 0, direct = c->bpl_ident[0] != 0;
    const uint32_t need = POLAR_FLAG_BP_CONVERGED | (crc ? POLAR_FLAG_CRC_PASS : 0u);
    const size_t row = (size_t)N * (in_is_f32 ? 4 : 8);
    const size_t CH = chunk_rows(c, B, row);
    // every buffer of the call, before its first launch
    if ((rc = ensure(c, c->bpl_siters, B * sizeof(uint32_t)))) return rc;
    if (!d_flags && (P > 1 || crc || d_graph || d_total)) {
        if ((rc = ensure(c, c->ad_flags, B * sizeof(uint32_t)))) return rc;
        d_flags = (uint32_t *)c->ad_flags.p;
    }
    if (P > 1 || !direct) {
        if ((rc = ensure_compaction(c, B, true))) return rc;
        if ((rc = ensure(c, c->ad_in, CH * row))) return rc;
        if ((rc = ensure(c, c->ad_bits, CH * NW * sizeof(uint32_t)))) return rc;
    }
    if (d_pm) HIP_TRY(c, hipMemsetAsync(d_pm, 0, B * sizeof(double), c->stream));
    uint32_t *siters = (uint32_t *)c->bpl_siters.p, *sflags = (uint32_t *)c->ad_sflags.p, *sbits = (uint32_t *)c->ad_bits.p;
    auto tables = [&](int p, const uint16_t **sig, const uint16_t **sinv, const uint32_t **fz, const uint32_t **tab) {
        const bool id = c->bpl_ident[(size_t)p] != 0;
        *sig = id ? nullptr : c->d_bpl_sigma + (size_t)p * N;
        *sinv = id ? nullptr : c->d_bpl_sinv + (size_t)p * N;
        *fz = c->d_bpl_frozen + (size_t)p * NW;
        *tab = crc ? c->d_bpl_crc + (size_t)p * N : nullptr;
    };
    // one chunk of attempt p through the staging buffers: frames idx[0..nc), or base .. base + nc when idx is null
    auto staged = [&](int p, const uint32_t *idx, size_t base, size_t nc, uint32_t *fl, uint32_t *it) -> int {
        const uint16_t *sig, *sinv;
        const uint32_t *fz, *tab;
        tables(p, &sig, &sinv, &fz, &tab);
        int r;
        if ((r = polar_tu::bpl_gather(c, d_in, in_is_f32 != 0, c->ad_in.p, idx, base, sig, nc))) return r;
        if ((r = decode_fixed(c, c->ad_in.p, in_is_f32, sigma, nc, sbits, nullptr, fl, fz, it))) return r;
        if (crc && (r = polar_tu::ad_crc_check(c, sbits, tab, fl, nc))) return r;
        return polar_tu::bpl_scatter(c, sbits, it, fl, idx, base, nc, sinv, need, p, P, p == 0, d_bits, d_iters, d_flags,
                                     d_graph, d_total);
    };
    const uint32_t *cur_flags;
    if (direct) {
        uint32_t *it0 = d_iters ? d_iters : siters;
        if ((rc = decode_fixed(c, d_in, in_is_f32, sigma, B, d_bits, nullptr, d_flags, c->d_bpl_frozen, it0))) return rc;
        if (crc && (rc = polar_tu::ad_crc_check(c, d_bits, c->d_bpl_crc, d_flags, B))) return rc;
        if ((d_graph || d_total) &&
            (rc = polar_tu::bpl_scatter(c, nullptr, it0, d_flags, nullptr, 0, B, nullptr, need, 0, P, true, d_bits, it0, d_flags,
                                        d_graph, d_total)))
            return rc;
        cur_flags = d_flags;
    } else {
        for (size_t off = 0; off < B; off += CH)
            if ((rc = staged(0, nullptr, off, std::min(CH, B - off), sflags + off, siters + off))) return rc;
        cur_flags = sflags;
    }
    const uint32_t *cur_idx = nullptr;
    size_t n = B;
    for (int p = 1; p < P; ++p) {
        uint32_t *idx = (uint32_t *)c->ad_idx[(p - 1) & 1].p;
        if ((rc = compact_open(c, cur_flags, cur_idx, n, need, idx, &n))) return rc;
        if (n == 0) break;
        for (size_t off = 0; off < n; off += CH)
            if ((rc = staged(p, idx + off, 0, std::min(CH, n - off), sflags + off, siters + off))) return rc;
        cur_idx = idx;
        cur_flags = sflags;
    }
    return POLAR_OK;
}

// SCAN (POLAR_ALGO_SCAN, include/polar_hip.h): one launch of k_scan_lanes, no host read-back.  Every output is nullable
// here: the soft-output entry point may ask for LLRs only.
int scan_decode(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits, double *d_pm,
                uint32_t *d_flags, const uint32_t *d_frozen, void *d_llr_u, void *d_ext_x)
{
    const size_t rsz = c->cfg.dtype == POLAR_F32 ? 4 : 8;
    if (!d_in || B > kMaxBatch || (reinterpret_cast<uintptr_t>(d_in) % (in_is_f32 ? 4 : 8))) return POLAR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_llr_u) | reinterpret_cast<uintptr_t>(d_ext_x)) % rsz) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    if (d_pm) HIP_TRY(c, hipMemsetAsync(d_pm, 0, B * sizeof(double), c->stream));
    if (d_flags) HIP_TRY(c, hipMemsetAsync(d_flags, 0, B * sizeof(uint32_t), c->stream));
    polar::ScanParams P{};
    P.in = d_in; P.sigma = sigma; P.out_bits = d_bits; P.llr_u = d_llr_u; P.ext_x = d_ext_x; P.frozen = d_frozen;
    P.N = c->cfg.N; P.n = c->n; P.B = (int)B; P.iters = c->scan_I;
    return polar_tu::scan_lanes(c, P, c->cfg.dtype == POLAR_F32, in_is_f32 != 0);
}

}  // namespace polar_host

extern "C" {

int polar_bp_set_stop(polar_ctx *c, int rule)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BP || (rule != POLAR_BP_STOP_NONE && rule != POLAR_BP_STOP_G)) return POLAR_EINVAL;
    c->bp_stop = rule;
    refresh_kernel_name(c);
    return POLAR_OK;
}

int polar_cascl_set_stages(polar_ctx *c, const int *stages, int n)
{
    if (!c || c->cfg.algo != POLAR_ALGO_CASCL || c->is_dyn || c->cfg.dtype == POLAR_Q8 || n < 0 || n > 6 || (n > 0 && !stages)) return POLAR_EINVAL;
    for (int i = 0; i < n; ++i) {
        const int L = stages[i];
        if (L < 1 || L > 32 || (L & (L - 1)) || (i && L <= stages[i - 1])) return POLAR_EINVAL;
    }
    if (n > 0 && stages[n - 1] != c->cfg.L) return POLAR_EINVAL;
    if (n > 1 && c->cfg.L < 2) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    std::vector<polar_ctx *> subs;
    if (n > 1) {
        subs.assign((size_t)n, nullptr);   // the last stage (L = cfg.L) is this ctx's own decoder
        for (int i = 0; i + 1 < n; ++i) {
            polar_cfg g = c->cfg;          // crc_taps / info_order point into c
            g.L = stages[i];
            if (stages[i] == 1) {          // SC over I[0..K+r): the CRC positions decoded as information bits
                g.algo = POLAR_ALGO_SC;
                g.K = c->A;
                g.crc_r = 0;
                g.crc_taps = nullptr;
                g.n_taps = 0;
                g.crc_systematic = 0;
            }
            int rc = polar_create(&g, &subs[(size_t)i]);
            if (!rc) rc = polar_set_stream(subs[(size_t)i], c->stream.get());
            if (!rc && c->sys_polar && subs[(size_t)i]->d_crc_tab)   // the stage reads the table of the mode that is on
                rc = upload_crc_tables(subs[(size_t)i], c->h_crc_tab_sys);
            if (rc) {
                for (polar_ctx *s : subs) polar_destroy(s);
                return rc;
            }
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // no queued work still uses the old stage contexts
    for (polar_ctx *s : c->stage_ctx) polar_destroy(s);
    c->stage_ctx = subs;
    c->cascl_stages = n > 1 ? std::vector<int>(stages, stages + n) : std::vector<int>();
    refresh_kernel_name(c);
    return POLAR_OK;
}

int polar_scf_set_flips(polar_ctx *c, int T)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF || T < 0 || T > polar::SCF_MAX_T || T > c->A) return POLAR_EINVAL;
    c->scf_T = T;
    refresh_kernel_name(c);
    return POLAR_OK;
}

int polar_scf_set_dynamic(polar_ctx *c, const int *budgets, int omega, double cc, double tau)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF || omega < 0 || omega > POLAR_SCF_MAX_ORDER) return POLAR_EINVAL;
    if (omega == 0) {   // back to the static rule; T stays
        c->scf_omega = 0;
        refresh_kernel_name(c);
        return POLAR_OK;
    }
    if (!budgets || !std::isfinite(cc) || !std::isfinite(tau) || cc < 0 || tau < 0) return POLAR_EINVAL;
    for (int k = 0; k < omega; ++k)
        if (budgets[k] < 1 || budgets[k] > polar::SCF_MAX_T || (k == 0 && budgets[k] > c->A)) return POLAR_EINVAL;
    c->scf_omega = omega;
    c->scf_T = budgets[0];
    for (int k = 0; k < POLAR_SCF_MAX_ORDER; ++k) c->scf_Tk[k] = k < omega ? budgets[k] : 0;
    c->scf_c = cc;
    c->scf_tau = tau;
    refresh_kernel_name(c);
    return POLAR_OK;
}

int polar_scf_get_dynamic(const polar_ctx *c, int *omega, int *budgets, double *cc, double *tau)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF) return POLAR_EINVAL;
    if (omega) *omega = c->scf_omega;
    if (budgets)
        for (int k = 0; k < POLAR_SCF_MAX_ORDER; ++k) budgets[k] = k == 0 ? c->scf_T : k < c->scf_omega ? c->scf_Tk[k] : 0;
    if (cc) *cc = c->scf_omega ? c->scf_c : 0.0;
    if (tau) *tau = c->scf_omega ? c->scf_tau : 0.0;
    return POLAR_OK;
}

int polar_scf_decode_sets_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_uhat_bits,
                                 uint32_t *d_flags, uint32_t *d_attempts, int32_t *d_sets)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, {.bits = d_uhat_bits, .flags = d_flags, .iters = d_attempts, .sets = d_sets},
                              c->d_frozen);
}

int polar_scf_decode_sets_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, unsigned *flags, unsigned *attempts,
                                int *sets)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, {.u_hat = u_hat, .flags = flags, .iters = attempts, .sets = sets});
}

int polar_scf_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_uhat_bits,
                            uint32_t *d_flags, uint32_t *d_attempts)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, {.bits = d_uhat_bits, .flags = d_flags, .iters = d_attempts}, c->d_frozen);
}

int polar_scf_decode_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, unsigned *flags, unsigned *attempts)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, {.u_hat = u_hat, .flags = flags, .iters = attempts});
}

int polar_bpl_cyclic_graphs(int n, int P, int *out)
{
    if (n < 5 || n > 12 || P < 1 || P > 32 || !out) return POLAR_EINVAL;
    for (int s = 0; s < P; ++s)
        for (int b = 0; b < n; ++b) out[s * n + b] = (b + s) % n;
    return POLAR_OK;
}

int polar_bpl_set_graphs(polar_ctx *c, const int *perms, int P)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BPL || !perms || P < 1 || P > 32) return POLAR_EINVAL;
    const int n = c->n, N = c->cfg.N, NW = c->NW;
    std::vector<unsigned char> ident((size_t)P, 1);
    for (int p = 0; p < P; ++p) {
        unsigned seen = 0;
        for (int b = 0; b < n; ++b) {
            const int v = perms[p * n + b];
            if (v < 0 || v >= n || ((seen >> v) & 1u)) return POLAR_EINVAL;
            seen |= 1u << v;
            if (v != b) ident[(size_t)p] = 0;
        }
    }
    const bool crc = c->cfg.crc_r > 0;
    std::vector<uint16_t> sig((size_t)P * N), sinv((size_t)P * N);
    std::vector<uint32_t> fz((size_t)P * NW, 0u), tab(crc ? (size_t)P * N : 0);
    for (int p = 0; p < P; ++p)
        for (int j = 0; j < N; ++j) {
            const int t = bpl_sigma(perms + p * n, n, j);
            sig[(size_t)p * N + j] = (uint16_t)t;
            sinv[(size_t)p * N + t] = (uint16_t)j;
            if (c->frozen[(size_t)t]) fz[(size_t)p * NW + (j >> 5)] |= 1u << (j & 31);
            if (crc) tab[(size_t)p * N + j] = c->h_crc_tab[(size_t)t];
        }
    DeviceGuard guard(c->cfg.device);
    DevMem<uint16_t> d_sig, d_sinv;
    DevMem<uint32_t> d_fz, d_tab;
    int rc;
    if ((rc = d_sig.upload(sig.data(), sig.size())) || (rc = d_sinv.upload(sinv.data(), sinv.size())) ||
        (rc = d_fz.upload(fz.data(), fz.size())) || (crc && (rc = d_tab.upload(tab.data(), tab.size()))))
        return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // no queued decode still reads the old tables
    c->d_bpl_sigma = std::move(d_sig);
    c->d_bpl_sinv = std::move(d_sinv);
    c->d_bpl_frozen = std::move(d_fz);
    c->d_bpl_crc = std::move(d_tab);
    c->bpl_perms.assign(perms, perms + (size_t)P * n);
    c->bpl_ident = ident;
    refresh_kernel_name(c);
    return POLAR_OK;
}

int polar_bpl_get_graphs(const polar_ctx *c, int *P, int *perms)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BPL) return POLAR_EINVAL;
    if (P) *P = (int)c->bpl_ident.size();
    if (perms) std::copy(c->bpl_perms.begin(), c->bpl_perms.end(), perms);
    return POLAR_OK;
}

int polar_bpl_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_uhat_bits,
                            uint32_t *d_iters, uint32_t *d_flags, uint32_t *d_graph, uint32_t *d_total_iters)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BPL) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return decode_device_impl(c, d_in, in_is_f32, sigma, B,
                              {.bits = d_uhat_bits, .flags = d_flags, .iters = d_iters, .graph = d_graph, .total = d_total_iters}, c->d_frozen);
}

int polar_bpl_decode_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, unsigned *iters, unsigned *flags,
                           unsigned *graph, unsigned *total_iters)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BPL) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, {.u_hat = u_hat, .flags = flags, .iters = iters, .graph = graph, .total = total_iters});
}

int polar_scan_set_iters(polar_ctx *c, int I)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCAN || I < 1 || I > polar::SCAN_MAX_ITERS) return POLAR_EINVAL;
    c->scan_I = I;
    refresh_kernel_name(c);
    return POLAR_OK;
}

int polar_scan_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_uhat_bits,
                             void *d_llr_u, void *d_ext_x)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCAN) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, {.bits = d_uhat_bits, .llr_u = d_llr_u, .ext_x = d_ext_x}, c->d_frozen);
}

// the soft outputs are [B][N] of the ctx dtype: the batch goes through the device buffers in one piece
int polar_scan_decode_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, void *llr_u, void *ext_x)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCAN || !llr_in) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    if (B > kMaxBatch) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    const int N = c->cfg.N, NW = c->NW;
    const size_t W = c->rm_mode != POLAR_RM_NONE ? (size_t)c->rm_E : (size_t)N;
    const size_t soft = B * (size_t)N * (c->cfg.dtype == POLAR_F32 ? 4 : 8);
    int rc;
    if ((rc = ensure(c, c->in, B * W * sizeof(double)))) return rc;
    if (u_hat && (rc = ensure(c, c->bits, B * NW * sizeof(uint32_t)))) return rc;
    if (llr_u && (rc = ensure(c, c->scan_llr, soft))) return rc;
    if (ext_x && (rc = ensure(c, c->scan_ext, soft))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->in.p, llr_in, B * W * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const DecodeOut o{.bits = u_hat ? (uint32_t *)c->bits.p : nullptr, .llr_u = llr_u ? c->scan_llr.p : nullptr,
                      .ext_x = ext_x ? c->scan_ext.p : nullptr};
    if ((rc = decode_device_impl(c, c->in.p, 0, 0.0, B, o, c->d_frozen))) return sync_fail(c, rc);
    std::vector<uint32_t> w;
    if (u_hat) {
        w.resize(B * (size_t)NW);
        HIP_TRY(c, hipMemcpyAsync(w.data(), c->bits.p, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (llr_u) HIP_TRY(c, hipMemcpyAsync(llr_u, c->scan_llr.p, soft, hipMemcpyDeviceToHost, c->stream));
    if (ext_x) HIP_TRY(c, hipMemcpyAsync(ext_x, c->scan_ext.p, soft, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (u_hat) unpack_rows(w.data(), B, N, u_hat);
    return POLAR_OK;
}

int polar_cascl_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_uhat_bits,
                              double *d_pm, uint32_t *d_flags, uint32_t *d_list)
{
    if (!c || c->cfg.algo != POLAR_ALGO_CASCL || c->is_dyn) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, {.bits = d_uhat_bits, .pm = d_pm, .flags = d_flags, .iters = d_list}, c->d_frozen);
}

int polar_cascl_decode_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, double *pm, unsigned *flags,
                             unsigned *list)
{
    if (!c || c->cfg.algo != POLAR_ALGO_CASCL || c->is_dyn) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, {.u_hat = u_hat, .pm = pm, .flags = flags, .iters = list});
}

int polar_bp_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_uhat_bits,
                           uint32_t *d_iters, uint32_t *d_flags)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BP) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, {.bits = d_uhat_bits, .flags = d_flags, .iters = d_iters}, c->d_frozen);
}

int polar_bp_decode_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, unsigned *iters, unsigned *flags)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BP) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, {.u_hat = u_hat, .flags = flags, .iters = iters});
}

int polar_bp_readout_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B,
                            const uint32_t *d_u_bits, const int *checkpoints, int ncp, unsigned long long *d_E,
                            uint32_t *d_uhat_bits)
{
    if (!c || !d_in || !d_u_bits || !checkpoints || !d_E) return POLAR_EINVAL;
    if (c->cfg.algo != POLAR_ALGO_BP || ncp < 1 || ncp > 8 || B > kMaxBatch) return POLAR_EINVAL;
    if (c->bp_stop != POLAR_BP_STOP_NONE) return POLAR_EINVAL;   // the checkpoints need every frame to run all round trips
    if (c->rm_mode != POLAR_RM_NONE) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    if (B == 0) return POLAR_OK;
    polar::BpReadoutParams P{};
    for (int i = 0; i < ncp; ++i) {
        if (checkpoints[i] < 1 || checkpoints[i] > c->cfg.bp_iters || (i && checkpoints[i] <= checkpoints[i - 1]))
            return POLAR_EINVAL;
        P.cp[i] = checkpoints[i];
    }
    P.ncp = ncp;
    P.in = d_in; P.sigma = sigma; P.out_bits = d_uhat_bits; P.frozen = c->d_frozen; P.info = c->d_info;
    P.u_bits = d_u_bits; P.E = d_E;
    P.N = c->cfg.N; P.n = c->n; P.B = (int)B; P.iters = c->cfg.bp_iters;
    return polar_tu::bp_readout(c, P, c->cfg.dtype == POLAR_F32, in_is_f32 != 0);
}

int polar_bp_readout_batch(polar_ctx *c, const double *in, double sigma, size_t B, const int *u, const int *checkpoints,
                           int ncp, unsigned long long *E, int *u_hat)
{
    if (!c || !in || !u || !checkpoints || !E) return POLAR_EINVAL;
    if (ncp < 1 || ncp > 8 || c->bp_stop != POLAR_BP_STOP_NONE || c->rm_mode != POLAR_RM_NONE) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    if (B == 0) return POLAR_OK;
    const int N = c->cfg.N, NW = c->NW, n = c->n;
    int rc;
    if ((rc = ensure(c, c->in, B * N * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->bits, B * NW * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->gen_u, B * NW * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->gen_cnt, sizeof(unsigned long long) * 8 * (size_t)(n + 1)))) return rc;
    const std::vector<uint32_t> uw = pack_rows(u, B, N);
    HIP_TRY(c, hipMemcpyAsync(c->in.p, in, B * N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->gen_u.p, uw.data(), uw.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->gen_cnt.p, 0, sizeof(unsigned long long) * 8 * (size_t)(n + 1), c->stream));
    rc = polar_bp_readout_device(c, c->in.p, 0, sigma, B, (const uint32_t *)c->gen_u.p, checkpoints, ncp,
                                 (unsigned long long *)c->gen_cnt.p, (uint32_t *)c->bits.p);
    if (rc) return sync_fail(c, rc);
    std::vector<unsigned long long> he((size_t)ncp * (n + 1));
    std::vector<uint32_t> hb(u_hat ? B * (size_t)NW : 0);
    HIP_TRY(c, hipMemcpyAsync(he.data(), c->gen_cnt.p, he.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (u_hat) HIP_TRY(c, hipMemcpyAsync(hb.data(), c->bits.p, hb.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < he.size(); ++i) E[i] += he[i];
    if (u_hat) unpack_rows(hb.data(), B, N, u_hat);
    return POLAR_OK;
}

}  // extern "C"
