// polar_hip.hip -- C ABI (include/polar_hip.h) over the hand-written gfx950 kernels.
// Host side: code construction (frozen set, CRC table), kernel dispatch, buffers, stream.  The kernels and their launch
// code live in the k_*.hip translation units (polar_host.h declares what they export).
#include "polar_host.h"
#ifdef POLAR_TESTING
#include "../../include/polar_hip_testing.h"
#endif

#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>

#include "count_kernel.h"
#include "gen_kernel.h"
#include "polar_bits.h"
#include "scf_params.h"
#include "scan_params.h"

namespace {

const int kQ5G[1024] = {
#include "q5g_table.inc"
};

// Reliability order when the caller gives none: the 5G sequence restricted to < N for N <= 1024
// (what every reference program hard-codes, SC_1024.c:42-91 / SC_128.c:41-51); for N > 1024 the
// reference has no table and this build uses the polarization-weight (beta-expansion)
// order, beta = 2^(1/4) -- "parity unpinned" for those sizes.
std::vector<int> default_order(int N)
{
    std::vector<int> q;
    if (N <= 1024) {
        for (int i = 0; i < 1024; ++i)
            if (kQ5G[i] < N) q.push_back(kQ5G[i]);
    } else {
        int n = 0;
        while ((1 << n) < N) ++n;
        std::vector<std::pair<double, int>> w(N);
        const double beta = std::pow(2.0, 0.25);
        for (int i = 0; i < N; ++i) {
            double s = 0;
            for (int b = 0; b < n; ++b)
                if ((i >> b) & 1) s += std::pow(beta, b);
            w[i] = {s, i};
        }
        std::stable_sort(w.begin(), w.end());
        for (auto &x : w) q.push_back(x.second);
    }
    return q;
}

// D^i mod g(D) for i = position of leaf j in the reliability-ordered CRC codeword
// (CRcheck, CASCL_1024_L8.c:569-598: C[i] = u_hat[I[i]], long division by g, pass iff remainder 0;
// the remainder is linear in the bits, so it can be accumulated as bits are decided).
std::vector<uint32_t> make_crc_table(int N, int r, const std::vector<int> &taps, const std::vector<int> &I)
{
    std::vector<uint32_t> tab(N, 0u);
    uint64_t glow = 0;
    for (int t : taps)
        if (t < r) glow |= 1ull << t;
    const uint64_t top = 1ull << r;
    uint64_t rem = 1;  // D^0
    if (r == 0) return tab;
    for (size_t i = 0; i < I.size(); ++i) {
        tab[I[i]] = (uint32_t)rem;
        rem <<= 1;
        if (rem & top) rem = (rem ^ top) ^ glow;
    }
    return tab;
}

// The same test read off the root partial sums x_hat = u_hat F^{(x)n} at the end of a frame (the pair kernel, scl_fast2.h):
// u_j = XOR over {k : j a subset of k} of x_hat_k, so XOR over {j : u_j = 1} of tab[j] = XOR over {k : x_hat_k = 1} of t[k]
// with t[k] = XOR over {j : j a subset of k} of tab[j] -- the table pushed through the transpose of the transform.  Bit i
// of that remainder is the parity of x_hat AND mask i, mask i = bit i of every t[k]: CRC_MASK_ROWS masks of N bits,
// m[i * N/32 + w] = positions 32w .. 32w+31 of mask i, all-zero masks from r up.
std::vector<uint32_t> make_crc_masks(int N, const std::vector<uint32_t> &tab)
{
    std::vector<uint32_t> t = tab;
    for (int s = 1; s < N; s <<= 1)
        for (int k = 0; k < N; ++k)
            if (k & s) t[(size_t)k] ^= t[(size_t)(k ^ s)];
    const int NW = N / 32;
    std::vector<uint32_t> m((size_t)polar::CRC_MASK_ROWS * NW, 0u);
    for (int k = 0; k < N; ++k)
        for (int i = 0; i < polar::CRC_MASK_ROWS; ++i)
            if ((t[(size_t)k] >> i) & 1u) m[(size_t)i * NW + (k >> 5)] |= 1u << (k & 31);
    return m;
}

// Where the list-filling phase of the pair kernel ends (scl_fast2.h fill_phase(); N = 1024): the leaves below E are decoded
// breadth-first on at most two paths per 64-leaf block.  E is the largest of 256, 192, 128 for which
//   (a) at most three information leaves lie below E,
//   (b) every one of them is one of the last two leaves of its 64-leaf block, and none lies below leaf 126 (the first 128
//       leaves are one butterfly: leaves 62 / 63 may not fork),
//   (c) for E > 128, exactly one of them lies below leaf 128 and no other one below E - 64: exactly two paths enter every
//       block behind leaf 128 (the phase decodes such a block for two paths),
// and 0 (the frozen run and the octets behind it, as without the phase) if there is none or E <= 8 * lead, lead = the
// leading all-frozen octets the kernel counts (at most 15).  frozen: [N] bytes, non-zero = frozen.
int fill_phase_end(int N, const unsigned char *frozen)
{
    if (N != 1024) return 0;
    int lead = 0;
    while (lead < 15) {
        bool all = true;
        for (int k = 0; k < 8; ++k) all = all && frozen[8 * lead + k] != 0;
        if (!all) break;
        ++lead;
    }
    for (int E = 256; E >= 128; E -= 64) {
        int count = 0, early = 0, first = 0;   // information leaves below E / in front of the last block / below leaf 128
        bool ok = true;
        for (int j = 0; j < E; ++j) {
            if (frozen[j]) continue;
            if ((j & 63) < 62 || j < 126) ok = false;   // (b)
            ++count;
            if (j < E - 64) ++early;
            if (j < 128) ++first;
        }
        if (E > 128 && !(first == 1 && early == 1)) ok = false;   // (c)
        if (ok && count <= 3 && E > 8 * lead) return E;
    }
    return 0;
}

// the CRC table t of a ctx and its masks to the device, synchronously (d_crc_tab and d_crc_mask always hold the same table)
int upload_crc_tables(polar_ctx *c, const std::vector<uint32_t> &t)
{
    const std::vector<uint32_t> m = make_crc_masks(c->cfg.N, t);
    if (int rc = c->d_crc_tab.upload(t.data(), t.size())) return rc;
    return c->d_crc_mask.upload(m.data(), m.size());
}

// Rows per pass where a batch goes through ctx scratch in chunks: at most c->chunk_bytes (256 MiB) of rows, at least `floor`
// of them, never more than the batch.
size_t chunk_rows(const polar_ctx *c, size_t B, size_t row_bytes, size_t floor = 64)
{
    return std::min(B, std::max(floor, c->chunk_bytes / row_bytes));
}

constexpr size_t kMaxBatch = 0x7fffffffull;   // frames per call: the kernels count them in an int

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

// contexts whose code carries a CRC: r, crc_tab, the generator's CRC multiply, the systematic K-bit error metric
// (BP list decoding: optional, crc_r = 0 is a code without one)
bool has_crc(int algo) { return algo == POLAR_ALGO_CASCL || algo == POLAR_ALGO_SCF || algo == POLAR_ALGO_BPL; }

// ---- 5G rate matching, host side (include/polar_hip.h rules 1-5) ----
const int kRmP[32] = {0, 1, 2, 4, 3, 5, 6, 7, 8, 16, 9, 17, 10, 18, 11, 19, 12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31};

int rm_J(int N, int n) { return kRmP[n / (N / 32)] * (N / 32) + n % (N / 32); }   // rule 1

bool rm_args_ok(int N, int A, int E)
{
    return N >= 32 && N <= 1024 && !(N & (N - 1)) && A >= 1 && E >= A && E <= 8192;
}

int rm_mode_of(int N, int A, int E)   // rule 2
{
    if (E >= N) return POLAR_RM_REPEAT;
    return (16 * A <= 7 * E) ? POLAR_RM_PUNCTURE : POLAR_RM_SHORTEN;
}

// rule 4: I[0..A) in ascending reliability; POLAR_EINVAL if fewer than A positions are left
int rm_order(int N, int A, int E, std::vector<int> &I)
{
    if (!rm_args_ok(N, A, E)) return POLAR_EINVAL;
    std::vector<unsigned char> pre((size_t)N, 0);   // Q_F,tmp
    const int mode = rm_mode_of(N, A, E);
    if (mode == POLAR_RM_PUNCTURE) {
        for (int n = 0; n < N - E; ++n) pre[(size_t)rm_J(N, n)] = 1;
        const int t = (4 * E >= 3 * N) ? (3 * N - 2 * E + 3) / 4 : (9 * N - 4 * E + 15) / 16;
        for (int i = 0; i < t; ++i) pre[(size_t)i] = 1;
    } else if (mode == POLAR_RM_SHORTEN) {
        for (int n = E; n < N; ++n) pre[(size_t)rm_J(N, n)] = 1;
    }
    const std::vector<int> q = default_order(N);
    I.clear();
    for (int i = N - 1; i >= 0 && (int)I.size() < A; --i)
        if (!pre[(size_t)q[(size_t)i]]) I.push_back(q[(size_t)i]);
    if ((int)I.size() < A) return POLAR_EINVAL;
    std::reverse(I.begin(), I.end());
    return POLAR_OK;
}

// rule 3: pos[k] = position of e_k in the sent row (triangle written by rows, read by columns, NULLs skipped)
std::vector<uint16_t> rm_channel_ilv(int E)
{
    int T = 0;
    while (T * (T + 1) / 2 < E) ++T;
    std::vector<int> kat((size_t)T * T, -1);   // e index at (i, j), -1 = NULL
    int k = 0;
    for (int i = 0; i < T; ++i)
        for (int j = 0; j < T - i; ++j, ++k) kat[(size_t)i * T + j] = k < E ? k : -1;
    std::vector<uint16_t> pos((size_t)E);
    int t = 0;
    for (int j = 0; j < T; ++j)
        for (int i = 0; i < T - j; ++i)
            if (kat[(size_t)i * T + j] >= 0) pos[(size_t)kat[(size_t)i * T + j]] = (uint16_t)t++;
    return pos;
}

// ---- dynamic frozen bits, host side (include/polar_hip.h "Dynamic frozen bits") ----
// coefficients of g(D) from its exponents: g_0 = 1 required, exponents distinct and below N
bool pac_poly(int N, const int *taps, int n_taps, std::vector<unsigned char> &g)
{
    if (N < 1 || !taps || n_taps < 1) return false;
    g.assign((size_t)N, 0);
    for (int i = 0; i < n_taps; ++i) {
        if (taps[i] < 0 || taps[i] >= N || g[(size_t)taps[i]]) return false;
        g[(size_t)taps[i]] = 1;
    }
    return g[0] == 1;
}

// h = 1 / g(D) mod D^N over GF(2): h_0 = 1, h_k = XOR over t >= 1 with g_t = 1 of h_{k-t}
std::vector<unsigned char> pac_inverse(const std::vector<unsigned char> &g)
{
    const int N = (int)g.size();
    std::vector<int> t1;
    for (int t = 1; t < N; ++t)
        if (g[(size_t)t]) t1.push_back(t);
    std::vector<unsigned char> h((size_t)N, 0);
    h[0] = 1;
    for (int k = 1; k < N; ++k) {
        unsigned char v = 0;
        for (int t : t1)
            if (t <= k) v ^= h[(size_t)(k - t)];
        h[(size_t)k] = v;
    }
    return h;
}

// rows -> caller's CSR arrays; idx may be null (sizes only)
int dyn_emit(const std::vector<int> &P, const std::vector<std::vector<int>> &rows, int *pos, int *ptr, int *idx, int idx_cap,
             int *nnz)
{
    int tot = 0;
    for (size_t d = 0; d < P.size(); ++d) {
        pos[d] = P[d];
        ptr[d] = tot;
        tot += (int)rows[d].size();
    }
    ptr[P.size()] = tot;
    if (nnz) *nnz = tot;
    if (!idx) return POLAR_OK;
    if (idx_cap < tot) return POLAR_EINVAL;
    int k = 0;
    for (const auto &r : rows)
        for (int i : r) idx[k++] = i;
    return POLAR_OK;
}

// I[0..A) on the device, built on first use: the generators and the encoder side read it
int info_order_table(polar_ctx *c)
{
    if (c->d_info_order) return POLAR_OK;
    hipError_t e = hipSuccess;
    if (c->d_info_order.upload(c->info_order.data(), (size_t)c->A, &e)) return fail(c, e, "info_order table");
    return POLAR_OK;
}

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

// the fixed decoder of ctx c (its cfg.L / algo): the kernel selection every entry point uses
int decode_fixed(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits,
                 double *d_pm, uint32_t *d_flags, const uint32_t *d_frozen, uint32_t *d_iters = nullptr)
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
void refresh_kernel_name(polar_ctx *c);
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
    }
}

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
               uint32_t *d_flags, uint32_t *d_attempts, int32_t *d_sets = nullptr)
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

// the decoder of ctx c on N-wide rows: the fixed decoder, or for a CA-SCL ctx with a stage rule the adaptive one, or SC-Flip.
// d_iters: BP round trips per frame; CA-SCL: the list size that decided each frame; SC-Flip: the attempt that decided it.
// d_graph, d_total: BP list decoding only.
int decode_device_plain(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits,
                        double *d_pm, uint32_t *d_flags, const uint32_t *d_frozen, uint32_t *d_iters, void *d_llr_u = nullptr,
                        void *d_ext_x = nullptr, uint32_t *d_graph = nullptr, uint32_t *d_total = nullptr,
                        int32_t *d_sets = nullptr)
{
    if (c && c->cfg.algo == POLAR_ALGO_BPL) return bpl_decode(c, d_in, in_is_f32, sigma, B, d_bits, d_pm, d_flags, d_iters, d_graph, d_total);
    if (c && c->cfg.algo == POLAR_ALGO_SCAN) return scan_decode(c, d_in, in_is_f32, sigma, B, d_bits, d_pm, d_flags, d_frozen, d_llr_u, d_ext_x);
    if (c && c->cfg.algo == POLAR_ALGO_SCF) return scf_decode(c, d_in, in_is_f32, sigma, B, d_bits, d_pm, d_flags, d_iters, d_sets);
    if (c && c->cfg.algo == POLAR_ALGO_CASCL) {
        if (!d_in || !d_bits || B > kMaxBatch) return POLAR_EINVAL;
        if (B == 0) return POLAR_OK;
        if (!c->cascl_stages.empty()) return cascl_adaptive(c, d_in, in_is_f32, sigma, B, d_bits, d_pm, d_flags, d_iters);
        if (d_iters) HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_iters), c->cfg.L, B, c->stream));
        d_iters = nullptr;
    }
    return decode_fixed(c, d_in, in_is_f32, sigma, B, d_bits, d_pm, d_flags, d_frozen, d_iters);
}

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

// every decode of the C ABI: the ctx's decoder, behind the recovery on a rate-matched ctx
int decode_device_impl(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_bits,
                       double *d_pm, uint32_t *d_flags, const uint32_t *d_frozen, uint32_t *d_iters = nullptr,
                       void *d_llr_u = nullptr, void *d_ext_x = nullptr, uint32_t *d_graph = nullptr, uint32_t *d_total = nullptr,
                       int32_t *d_sets = nullptr)
{
    if (!c || c->rm_mode == POLAR_RM_NONE)
        return decode_device_plain(c, d_in, in_is_f32, sigma, B, d_bits, d_pm, d_flags, d_frozen, d_iters, d_llr_u, d_ext_x,
                                   d_graph, d_total, d_sets);
    const size_t esz = in_is_f32 ? 4 : 8;
    const bool scan = c->cfg.algo == POLAR_ALGO_SCAN;   // its three outputs are nullable
    const size_t soft_row = (size_t)c->cfg.N * (c->cfg.dtype == POLAR_F32 ? 4 : 8);
    if (!d_in || (!d_bits && !scan) || B > kMaxBatch || (reinterpret_cast<uintptr_t>(d_in) % esz)) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    return for_rm_chunks(c, d_in, in_is_f32, sigma, B, [&](const void *rows, size_t off, size_t nc) {
        return decode_device_plain(c, rows, in_is_f32, 0.0, nc, d_bits ? d_bits + off * (size_t)c->NW : nullptr,
                                   d_pm ? d_pm + off : nullptr, d_flags ? d_flags + off : nullptr, d_frozen,
                                   d_iters ? d_iters + off : nullptr, d_llr_u ? (char *)d_llr_u + off * soft_row : nullptr,
                                   d_ext_x ? (char *)d_ext_x + off * soft_row : nullptr, d_graph ? d_graph + off : nullptr,
                                   d_total ? d_total + off : nullptr, d_sets ? d_sets + off * polar::SCF_MAX_ORDER : nullptr);
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
int host_batch(polar_ctx *c, const double *in, double sigma, const unsigned char *frozen_mask, size_t B,
               int *u_hat, double *pm_out, unsigned *flags, unsigned *iters = nullptr, unsigned *graph = nullptr,
               unsigned *total = nullptr, int *sets = nullptr)
{
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
    if (iters && (rc = ensure(c, c->bp_iters, B * sizeof(uint32_t)))) return rc;
    if (graph && (rc = ensure(c, c->bpl_graph, B * sizeof(uint32_t)))) return rc;
    if (total && (rc = ensure(c, c->bpl_total, B * sizeof(uint32_t)))) return rc;
    if (sets && (rc = ensure(c, c->scf_hsets, B * polar::SCF_MAX_ORDER * sizeof(int32_t)))) return rc;
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
        rc = decode_device_impl(c, c->in2[s].p, 0, sigma, nf, (uint32_t *)c->bits2[s].p, (double *)c->pm.p + f0,
                                (uint32_t *)c->flags.p + f0, d_frozen, iters ? (uint32_t *)c->bp_iters.p + f0 : nullptr, nullptr,
                                nullptr, graph ? (uint32_t *)c->bpl_graph.p + f0 : nullptr,
                                total ? (uint32_t *)c->bpl_total.p + f0 : nullptr,
                                sets ? (int32_t *)c->scf_hsets.p + f0 * polar::SCF_MAX_ORDER : nullptr);
        if (rc) return fail_join(rc);
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
    if (pm_out) HIP_TRY(c, hipMemcpyAsync(pm_out, c->pm.p, B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (flags) HIP_TRY(c, hipMemcpyAsync(flags, c->flags.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (iters) HIP_TRY(c, hipMemcpyAsync(iters, c->bp_iters.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (graph) HIP_TRY(c, hipMemcpyAsync(graph, c->bpl_graph.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (total) HIP_TRY(c, hipMemcpyAsync(total, c->bpl_total.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (sets)
        HIP_TRY(c, hipMemcpyAsync(sets, c->scf_hsets.p, B * polar::SCF_MAX_ORDER * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
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

// ---- 5G rate matching (include/polar_hip.h) ----------------------------------------------------------------------------
int polar_rm_select_n(int A, int E, int n_max)
{
    if (A < 1 || E < A || E > 8192 || (n_max != 9 && n_max != 10)) return POLAR_EINVAL;
    int cl = 0;   // ceil(log2 E)
    while ((1 << cl) < E) ++cl;
    const int n1 = (cl >= 1 && 8ll * E <= 9ll * (1ll << (cl - 1)) && 16ll * A < 9ll * E) ? cl - 1 : cl;
    int n2 = 0;   // ceil(log2 8A)
    while ((1ll << n2) < 8ll * A) ++n2;
    return 1 << std::max(std::min(std::min(n1, n2), n_max), 5);
}

int polar_rm_info_order(int N, int A, int E, int *out)
{
    if (!out) return POLAR_EINVAL;
    std::vector<int> I;
    const int rc = rm_order(N, A, E, I);
    if (rc) return rc;
    std::copy(I.begin(), I.end(), out);
    return POLAR_OK;
}

int polar_create_rm(const polar_cfg *cfg, int E, int ibil, polar_ctx **out)
{
    if (!cfg || !out) return POLAR_EINVAL;
    *out = nullptr;
    if (cfg->info_order || (ibil != 0 && ibil != 1)) return POLAR_EINVAL;
    if (cfg->dtype == POLAR_Q8) return POLAR_EINVAL;   // no rate-matched fixed-point contexts
    if (cfg->algo < POLAR_ALGO_SC || cfg->algo > POLAR_ALGO_BPL) return POLAR_EINVAL;
    const int r = has_crc(cfg->algo) ? cfg->crc_r : 0;
    if (cfg->K < 1 || r < 0 || r > 32) return POLAR_EINVAL;
    const int N = cfg->N, A = cfg->K + r;
    std::vector<int> I;
    if (rm_order(N, A, E, I)) return POLAR_EINVAL;   // N, E and A > N - |Q_F,tmp|
    polar_cfg g = *cfg;
    g.info_order = I.data();
    polar_ctx *c = nullptr;
    int rc = polar_create(&g, &c);
    if (rc) return rc;
    c->rm_E = E;
    c->rm_mode = rm_mode_of(N, A, E);
    c->rm_ibil = ibil;
    if (ibil) {
        const std::vector<uint16_t> pos = rm_channel_ilv(E);
        std::vector<uint16_t> inv((size_t)E);
        for (int k = 0; k < E; ++k) inv[pos[(size_t)k]] = (uint16_t)k;
        DeviceGuard guard(cfg->device);
        if ((rc = c->d_rm_ilv.upload(pos.data(), (size_t)E)) || (rc = c->d_rm_ilv_inv.upload(inv.data(), (size_t)E))) {
            polar_destroy(c);
            return rc;
        }
    }
    refresh_kernel_name(c);
    *out = c;
    return POLAR_OK;
}

int polar_rm_info(const polar_ctx *c, int *E, int *mode, int *ibil)
{
    if (!c) return POLAR_EINVAL;
    if (E) *E = c->rm_mode != POLAR_RM_NONE ? c->rm_E : c->cfg.N;
    if (mode) *mode = c->rm_mode;
    if (ibil) *ibil = c->rm_ibil;
    return POLAR_OK;
}

// ---- dynamic frozen bits (include/polar_hip.h) -------------------------------------------------------------------------
int polar_create_dyn(const polar_cfg *cfg, const polar_dyn *dyn, polar_ctx **out)
{
    if (!cfg || !out) return POLAR_EINVAL;
    *out = nullptr;
    const int N = cfg->N;
    if (N < 32 || N > 4096 || (N & (N - 1))) return POLAR_EINVAL;
    if (cfg->algo != POLAR_ALGO_SC && cfg->algo != POLAR_ALGO_SCL && cfg->algo != POLAR_ALGO_CASCL) return POLAR_EINVAL;
    if (cfg->dtype == POLAR_Q8) return POLAR_EINVAL;   // no dynamic fixed-point contexts
    const int r = has_crc(cfg->algo) ? cfg->crc_r : 0;
    if (cfg->K < 1 || r < 0 || r > 32 || cfg->K + r > N) return POLAR_EINVAL;
    if (N > 1024) return POLAR_ENOKERNEL;
    if (!dyn || dyn->D < 0 || dyn->D > N || !dyn->ptr || dyn->ptr[0] != 0 || (dyn->D > 0 && !dyn->pos)) return POLAR_EINVAL;
    // the frozen set of the cfg, as polar_create builds it
    const int A = cfg->K + r;
    std::vector<int> I;
    if (cfg->info_order) {
        I.assign(cfg->info_order, cfg->info_order + A);
    } else {
        const std::vector<int> q = default_order(N);
        I.assign(q.end() - A, q.end());
    }
    std::vector<unsigned char> frozen((size_t)N, 1);
    for (int j : I) {
        if (j < 0 || j >= N || !frozen[(size_t)j]) return POLAR_EINVAL;
        frozen[(size_t)j] = 0;
    }
    const int D = dyn->D, NW = N / 32;
    std::vector<uint32_t> mask((size_t)std::max(D, 1) * NW, 0u);
    std::vector<int> row((size_t)N, -1);
    for (int d = 0; d < D; ++d) {
        const int j = dyn->pos[d];
        if (j < 0 || j >= N || (d && j <= dyn->pos[d - 1]) || !frozen[(size_t)j]) return POLAR_EINVAL;
        const int a = dyn->ptr[d], b = dyn->ptr[d + 1];
        if (b < a || b - a > j || (b > a && !dyn->idx)) return POLAR_EINVAL;
        for (int k = a; k < b; ++k) {
            const int i = dyn->idx[k];
            if (i < 0 || i >= j || (k > a && i <= dyn->idx[k - 1])) return POLAR_EINVAL;
            mask[(size_t)d * NW + (i >> 5)] |= 1u << (i & 31);
        }
        row[(size_t)j] = d;
    }
    polar_ctx *c = nullptr;
    int rc = polar_create(cfg, &c);
    if (rc) return rc;
    c->is_dyn = true;
    c->dyn_pos.assign(dyn->pos, dyn->pos + D);
    DeviceGuard guard(cfg->device);
    if (c->d_dyn_pos.alloc((size_t)std::max(D, 1)) != hipSuccess) rc = POLAR_ENOMEM;   // never empty, D = 0 included
    if (rc || (rc = c->d_dyn_mask.upload(mask.data(), mask.size())) || (rc = c->d_dyn_row.upload(row.data(), (size_t)N)) ||
        (rc = c->d_dyn_pos.upload(dyn->pos, (size_t)D))) {
        polar_destroy(c);
        return rc;
    }
    refresh_kernel_name(c);
    *out = c;
    return POLAR_OK;
}

int polar_dyn_info(const polar_ctx *c, int *D, int *pos)
{
    if (!c) return POLAR_EINVAL;
    if (D) *D = c->is_dyn ? (int)c->dyn_pos.size() : -1;
    if (pos) std::copy(c->dyn_pos.begin(), c->dyn_pos.end(), pos);
    return POLAR_OK;
}

int polar_dyn_pac(int N, const int *info_order, int A, const int *g_taps, int n_taps, int *pos, int *ptr, int *idx,
                  int idx_cap, int *nnz)
{
    if (N < 32 || N > 4096 || (N & (N - 1)) || !info_order || A < 1 || A > N || !pos || !ptr) return POLAR_EINVAL;
    std::vector<unsigned char> g, info((size_t)N, 0);
    if (!pac_poly(N, g_taps, n_taps, g)) return POLAR_EINVAL;
    for (int i = 0; i < A; ++i) {
        const int j = info_order[i];
        if (j < 0 || j >= N || info[(size_t)j]) return POLAR_EINVAL;
        info[(size_t)j] = 1;
    }
    const std::vector<unsigned char> h = pac_inverse(g);
    std::vector<int> P;
    std::vector<std::vector<int>> rows;
    for (int j = 0; j < N; ++j) {
        if (info[(size_t)j]) continue;
        P.push_back(j);
        rows.emplace_back();
        for (int i = 0; i < j; ++i)
            if (h[(size_t)(j - i)]) rows.back().push_back(i);
    }
    return dyn_emit(P, rows, pos, ptr, idx, idx_cap, nnz);
}

int polar_pac_precode(int N, const int *g_taps, int n_taps, const int *v, size_t B, int *u)
{
    std::vector<unsigned char> g;
    if (!v || !u || !pac_poly(N, g_taps, n_taps, g)) return POLAR_EINVAL;
    std::vector<int> t;
    for (int k = 0; k < N; ++k)
        if (g[(size_t)k]) t.push_back(k);
    for (size_t b = 0; b < B; ++b)
        for (int j = 0; j < N; ++j) {   // u_j = XOR over taps t <= j of v_{j-t}
            int x = 0;
            for (int k : t)
                if (k <= j) x ^= v[b * (size_t)N + (size_t)(j - k)] & 1;
            u[b * (size_t)N + (size_t)j] = x;
        }
    return POLAR_OK;
}

int polar_pac_unprecode(int N, const int *g_taps, int n_taps, const int *u, size_t B, int *v)
{
    std::vector<unsigned char> g;
    if (!v || !u || u == v || !pac_poly(N, g_taps, n_taps, g)) return POLAR_EINVAL;
    std::vector<int> t;
    for (int k = 1; k < N; ++k)
        if (g[(size_t)k]) t.push_back(k);
    for (size_t b = 0; b < B; ++b)
        for (int j = 0; j < N; ++j) {   // v_j = u_j XOR the taps t >= 1 of the v already recovered
            int x = u[b * (size_t)N + (size_t)j] & 1;
            for (int k : t)
                if (k <= j) x ^= v[b * (size_t)N + (size_t)(j - k)];
            v[b * (size_t)N + (size_t)j] = x;
        }
    return POLAR_OK;
}

int polar_dyn_pc5g(int N, const int *q_i, int n_qi, int n_pc, int n_pc_wm, int *pos, int *ptr, int *idx, int idx_cap,
                   int *nnz, int *info_order)
{
    if (N < 32 || N > 4096 || (N & (N - 1)) || !q_i || !pos || !ptr || !info_order) return POLAR_EINVAL;
    if (n_pc < 0 || n_pc_wm < 0 || n_pc_wm > n_pc || n_qi <= n_pc || n_qi > N) return POLAR_EINVAL;
    std::vector<unsigned char> in_qi((size_t)N, 0), is_pc((size_t)N, 0);
    for (int i = 0; i < n_qi; ++i) {
        const int j = q_i[i];
        if (j < 0 || j >= N || in_qi[(size_t)j]) return POLAR_EINVAL;
        in_qi[(size_t)j] = 1;
    }
    for (int i = 0; i < n_pc - n_pc_wm; ++i) is_pc[(size_t)q_i[i]] = 1;   // the least reliable of Q_I
    // n_pc_wm more among the n_qi - n_pc most reliable: minimum row weight 2^popcount(j), equal weights to the more reliable
    for (int k = 0; k < n_pc_wm; ++k) {
        int best = -1;
        for (int i = n_pc; i < n_qi; ++i) {
            const int j = q_i[i];
            if (is_pc[(size_t)j]) continue;
            if (best < 0 || __builtin_popcount((unsigned)j) <= __builtin_popcount((unsigned)q_i[best])) best = i;
        }
        is_pc[(size_t)q_i[best]] = 1;
    }
    std::vector<int> P;
    std::vector<std::vector<int>> rows;
    for (int j = 0; j < N; ++j) {
        if (!is_pc[(size_t)j]) continue;
        P.push_back(j);
        rows.emplace_back();
        for (int i = j % 5; i < j; i += 5)
            if (in_qi[(size_t)i] && !is_pc[(size_t)i]) rows.back().push_back(i);
    }
    int k = 0;
    for (int i = 0; i < n_qi; ++i)
        if (!is_pc[(size_t)q_i[i]]) info_order[k++] = q_i[i];
    return dyn_emit(P, rows, pos, ptr, idx, idx_cap, nnz);
}

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
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, d_bits, d_pm, d_flags, c->d_frozen);
}

int polar_decode_batch(polar_ctx *c, const double *llr_in, const unsigned char *frozen_mask, size_t B, int *u_hat,
                       double *pm_out, unsigned *flags)
{
    return host_batch(c, llr_in, 0.0, frozen_mask, B, u_hat, pm_out, flags);
}

int polar_decode_batch_y(polar_ctx *c, const double *y, double sigma, size_t B, int *u_hat, double *pm_out,
                         unsigned *flags)
{
    if (!(sigma > 0)) return POLAR_EINVAL;
    return host_batch(c, y, sigma, nullptr, B, u_hat, pm_out, flags);
}

int polar_decode(polar_ctx *c, const double *y, double sigma, int *u_hat)
{
    if (!(sigma > 0)) return POLAR_EINVAL;
    return host_batch(c, y, sigma, nullptr, 1, u_hat, nullptr, nullptr);
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
    return host_batch(c, llr_in, 0.0, nullptr, 1, u_hat, nullptr, nullptr);
}

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
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, d_uhat_bits, nullptr, d_flags, c->d_frozen, d_attempts, nullptr,
                              nullptr, nullptr, nullptr, d_sets);
}

int polar_scf_decode_sets_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, unsigned *flags, unsigned *attempts,
                                int *sets)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, u_hat, nullptr, flags, attempts, nullptr, nullptr, sets);
}

int polar_scf_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_uhat_bits,
                            uint32_t *d_flags, uint32_t *d_attempts)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, d_uhat_bits, nullptr, d_flags, c->d_frozen, d_attempts);
}

int polar_scf_decode_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, unsigned *flags, unsigned *attempts)
{
    if (!c || c->cfg.algo != POLAR_ALGO_SCF) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, u_hat, nullptr, flags, attempts);
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
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, d_uhat_bits, nullptr, d_flags, c->d_frozen, d_iters, nullptr, nullptr,
                              d_graph, d_total_iters);
}

int polar_bpl_decode_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, unsigned *iters, unsigned *flags,
                           unsigned *graph, unsigned *total_iters)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BPL) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, u_hat, nullptr, flags, iters, graph, total_iters);
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
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, d_uhat_bits, nullptr, nullptr, c->d_frozen, nullptr, d_llr_u, d_ext_x);
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
    if ((rc = decode_device_impl(c, c->in.p, 0, 0.0, B, u_hat ? (uint32_t *)c->bits.p : nullptr, nullptr, nullptr, c->d_frozen,
                                 nullptr, llr_u ? c->scan_llr.p : nullptr, ext_x ? c->scan_ext.p : nullptr)))
        return sync_fail(c, rc);
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
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, d_uhat_bits, d_pm, d_flags, c->d_frozen, d_list);
}

int polar_cascl_decode_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, double *pm, unsigned *flags,
                             unsigned *list)
{
    if (!c || c->cfg.algo != POLAR_ALGO_CASCL || c->is_dyn) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, u_hat, pm, flags, list);
}

int polar_bp_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_uhat_bits,
                           uint32_t *d_iters, uint32_t *d_flags)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BP) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return decode_device_impl(c, d_in, in_is_f32, sigma, B, d_uhat_bits, nullptr, d_flags, c->d_frozen, d_iters);
}

int polar_bp_decode_batch(polar_ctx *c, const double *llr_in, size_t B, int *u_hat, unsigned *iters, unsigned *flags)
{
    if (!c || c->cfg.algo != POLAR_ALGO_BP) return POLAR_EINVAL;
    return host_batch(c, llr_in, 0.0, nullptr, B, u_hat, nullptr, flags, iters);
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
    int grid = (int)std::min<size_t>((B + waves_per_block - 1) / waves_per_block, (size_t)c->num_cu * 8);
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
    if ((rc = decode_device_impl(c, c->in.p, 0, sigma, B, (uint32_t *)c->bits.p, nullptr, nullptr, c->d_frozen))) return sync_fail(c, rc);
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
    int grid = (int)std::min<size_t>((B + waves - 1) / waves, (size_t)c->num_cu * 8);
    hipLaunchKernelGGL(polar::k_generate, dim3(grid), dim3(64 * waves), lds, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

// generate -> decode -> count for B frames; the two counters stay in c->gen_cnt (device) and are copied to h[2] if h != null
static int fer_batch_impl(polar_ctx *c, unsigned long long seed, unsigned long long first_frame, double snr_db, size_t B,
                          unsigned long long *h, uint32_t *d_frame_err = nullptr)
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
        if ((r = decode_device_impl(c, (char *)c->gen_llr.p + f0 * W * esz, f32 ? 1 : 0, 0.0, nf, (uint32_t *)c->bits.p + f0 * NW,
                                    nullptr, nullptr, c->d_frozen))) return r;
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

// ---- encoder, payload extraction, systematic polar codes (include/polar_hip.h) ------------------------------------------
namespace {

// x F^{(x)n} on one packed host row, the stages of enc_kernel.h
void host_transform(uint32_t *w, int NW)
{
    for (int i = 0; i < NW; ++i) w[i] = polar::polar_word_transform(w[i]);
    for (int o = 1; o < NW; o <<= 1)
        for (int i = 0; i < NW; ++i)
            if (!(i & o)) w[i] ^= w[i + o];
}

// the tables k_place / k_extract read, built on first use
int enc_tables(polar_ctx *c)
{
    const int N = c->cfg.N, A = c->A;
    if (int rc = info_order_table(c)) return rc;
    if (!c->d_enc_rtab) {
        std::vector<uint32_t> rtab((size_t)A);   // D^i mod g(D): make_crc_table keeps it at position I[i]
        for (int i = 0; i < A; ++i) rtab[(size_t)i] = c->h_crc_tab[(size_t)c->info_order[(size_t)i]];
        if (int rc = c->d_enc_rtab.upload(rtab.data(), rtab.size())) return rc;
    }
    if (!c->d_enc_inv) {
        std::vector<uint16_t> inv((size_t)N, (uint16_t)0xFFFFu);
        for (int i = 0; i < A; ++i) inv[(size_t)c->info_order[(size_t)i]] = (uint16_t)i;
        if (int rc = c->d_enc_inv.upload(inv.data(), inv.size())) return rc;
    }
    return POLAR_OK;
}

// scratch rows of the encoder grow with ensure_nomem: out of memory is POLAR_ENOMEM and leaves the ctx usable
const char *const kEncScratch = "encoder scratch";

// the CRC table of systematic mode: tab_sys[j] = XOR over {i : I[i] a subset of j} of crc_tab[I[i]] at unfrozen j, 0 at frozen j
// (x_c = XOR over {j : c subset of j} of u_j, so the syndrome of x[I] is a XOR over the set u bits as before)
void make_crc_table_sys(const polar_ctx *c, std::vector<uint32_t> &t)
{
    const int N = c->cfg.N;
    t = c->h_crc_tab;
    for (int s = 1; s < N; s <<= 1)
        for (int j = 0; j < N; ++j)
            if (j & s) t[(size_t)j] ^= t[(size_t)(j ^ s)];
    for (int j = 0; j < N; ++j)
        if (c->frozen[(size_t)j]) t[(size_t)j] = 0u;
}

}  // namespace

int polar_systematic_check(int N, const int *info_order, int A)
{
    if (N < 32 || N > 4096 || (N & (N - 1)) || !info_order || A < 1 || A > N) return POLAR_EINVAL;
    const int NW = N / 32;
    std::vector<uint32_t> keep((size_t)NW, 0u);
    for (int i = 0; i < A; ++i) {
        const int j = info_order[i];
        if (j < 0 || j >= N || ((keep[(size_t)(j >> 5)] >> (j & 31)) & 1u)) return POLAR_EINVAL;
        keep[(size_t)(j >> 5)] |= 1u << (j & 31);
    }
    // the two-pass encoder on every unit vector of I: x = ((e_j F) restricted to I) F must be e_j on I
    // (u = x F is then that restriction itself, zero on F)
    std::vector<uint32_t> w((size_t)NW);
    for (int i = 0; i < A; ++i) {
        const int j = info_order[i];
        std::fill(w.begin(), w.end(), 0u);
        w[(size_t)(j >> 5)] = 1u << (j & 31);
        host_transform(w.data(), NW);
        for (int k = 0; k < NW; ++k) w[(size_t)k] &= keep[(size_t)k];
        host_transform(w.data(), NW);
        for (int k = 0; k < NW; ++k)
            if ((w[(size_t)k] & keep[(size_t)k]) != (k == (j >> 5) ? 1u << (j & 31) : 0u)) return 0;
    }
    return 1;
}

int polar_crc_masks(int N, const int *info_order, int A, int crc_r, const int *crc_taps, int n_taps, int systematic,
                    uint32_t *crc_tab, uint32_t *masks)
{
    if (N < 32 || N > 4096 || (N & (N - 1)) || !info_order || A < 1 || A > N || crc_r < 1 || crc_r > 32 || !crc_taps ||
        n_taps < 2 || !masks)
        return POLAR_EINVAL;
    polar_ctx c;   // host members only: what make_crc_table_sys reads
    c.cfg.N = N;
    c.frozen.assign((size_t)N, 1);
    for (int i = 0; i < A; ++i) {
        if (info_order[i] < 0 || info_order[i] >= N) return POLAR_EINVAL;
        c.frozen[(size_t)info_order[i]] = 0;
    }
    c.h_crc_tab = make_crc_table(N, crc_r, std::vector<int>(crc_taps, crc_taps + n_taps), std::vector<int>(info_order, info_order + A));
    std::vector<uint32_t> t = c.h_crc_tab;
    if (systematic) make_crc_table_sys(&c, t);
    if (crc_tab) std::copy(t.begin(), t.end(), crc_tab);
    const std::vector<uint32_t> m = make_crc_masks(N, t);
    std::copy(m.begin(), m.end(), masks);
    return POLAR_OK;
}

int polar_fill_phase_end(int N, const int *info_order, int A)
{
    if (N < 32 || N > 4096 || (N & (N - 1)) || !info_order || A < 1 || A > N) return POLAR_EINVAL;
    std::vector<unsigned char> frozen((size_t)N, 1);
    for (int i = 0; i < A; ++i) {
        if (info_order[i] < 0 || info_order[i] >= N) return POLAR_EINVAL;
        frozen[(size_t)info_order[i]] = 0;
    }
    return fill_phase_end(N, frozen.data());
}

int polar_get_systematic(const polar_ctx *c) { return c && c->sys_polar ? 1 : 0; }

int polar_set_systematic(polar_ctx *c, int on)
{
    if (!c || (on != 0 && on != 1)) return POLAR_EINVAL;
    if ((on != 0) == c->sys_polar) return POLAR_OK;
    if (on) {
        if (c->is_dyn || c->rm_mode != POLAR_RM_NONE || c->cfg.dtype == POLAR_Q8 || c->cfg.algo == POLAR_ALGO_BPL) return POLAR_EINVAL;
        if (polar_systematic_check(c->cfg.N, c->info_order.data(), c->A) != 1) return POLAR_EINVAL;
    }
    DeviceGuard guard(c->cfg.device);
    if (c->d_crc_tab) {
        // CA-SCL, its adaptive stages and SC-Flip test the CRC through this table only: switch it with the mode
        if (c->h_crc_tab_sys.empty()) make_crc_table_sys(c, c->h_crc_tab_sys);
        const std::vector<uint32_t> &t = on ? c->h_crc_tab_sys : c->h_crc_tab;
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // no queued decode still reads the old table
        if (int rc = upload_crc_tables(c, t)) return rc;
        for (polar_ctx *s : c->stage_ctx)
            if (s && s->d_crc_tab)
                if (int rc = upload_crc_tables(s, t)) return rc;
    }
    c->sys_polar = on != 0;
    return POLAR_OK;
}

int polar_transform_device(polar_ctx *c, const uint32_t *d_in, size_t B, uint32_t *d_out)
{
    if (!c || !d_in || !d_out || B > kMaxBatch) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    return polar_tu::enc_transform(c, d_in, nullptr, false, B, d_out);
}

int polar_encode_device(polar_ctx *c, const uint32_t *d_payload, size_t B, uint32_t *d_u_bits, uint32_t *d_x_bits)
{
    if (!c || !d_payload || (!d_u_bits && !d_x_bits) || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    int rc;
    if ((rc = enc_tables(c))) return rc;
    const size_t row = (size_t)c->NW * sizeof(uint32_t);
    uint32_t *u = d_u_bits;
    if (!u) {
        if ((rc = ensure_nomem(c, c->enc_u, B * row, kEncScratch))) return rc;
        u = (uint32_t *)c->enc_u.p;
    }
    const bool rm = c->rm_mode != POLAR_RM_NONE;
    if (rm && d_x_bits && (rc = ensure_nomem(c, c->enc_x, B * row, kEncScratch))) return rc;
    if ((rc = polar_tu::enc_place(c, d_payload, B, u))) return rc;
    if (c->is_dyn && (rc = polar_tu::enc_dyn_fill(c, u, B))) return rc;
    // systematic: u = (z F) with the frozen positions cleared; x = u F then carries z on the information set
    if (c->sys_polar && (rc = polar_tu::enc_transform(c, u, nullptr, true, B, u))) return rc;
    if (!d_x_bits) return POLAR_OK;
    if (!rm) return polar_tu::enc_transform(c, u, nullptr, false, B, d_x_bits);
    if ((rc = polar_tu::enc_transform(c, u, nullptr, false, B, (uint32_t *)c->enc_x.p))) return rc;
    return polar_tu::enc_rm_select(c, (const uint32_t *)c->enc_x.p, B, d_x_bits);
}

int polar_payload_device(polar_ctx *c, const uint32_t *d_uhat_bits, size_t B, uint32_t *d_payload, uint32_t *d_crc_ok)
{
    if (!c || !d_uhat_bits || !d_payload || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    int rc;
    if ((rc = enc_tables(c))) return rc;
    // systematic: the kernel transforms u_hat to x_hat in registers as it loads the row, so no scratch row is needed
    return polar_tu::enc_extract(c, d_uhat_bits, c->sys_polar, B, d_payload, d_crc_ok);
}

int polar_encode_batch(polar_ctx *c, const int *payload, size_t B, int *u, int *x)
{
    if (!c || !payload || (!u && !x) || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    const int K = c->cfg.K, KW = (K + 31) / 32, N = c->cfg.N, NW = c->NW;
    const int W = c->rm_mode != POLAR_RM_NONE ? c->rm_E : N, XW = (W + 31) / 32;
    int rc;
    if ((rc = ensure_nomem(c, c->in, B * KW * 4, kEncScratch))) return rc;
    if ((rc = ensure_nomem(c, c->bits, B * NW * 4, kEncScratch))) return rc;
    if ((rc = ensure_nomem(c, c->enc_io, B * XW * 4, kEncScratch))) return rc;
    const std::vector<uint32_t> pw = pack_rows(payload, B, K);
    HIP_TRY(c, hipMemcpyAsync(c->in.p, pw.data(), pw.size() * 4, hipMemcpyHostToDevice, c->stream));
    rc = polar_encode_device(c, (const uint32_t *)c->in.p, B, (uint32_t *)c->bits.p, x ? (uint32_t *)c->enc_io.p : nullptr);
    if (rc) return sync_fail(c, rc);
    std::vector<uint32_t> hu(u ? B * (size_t)NW : 0), hx(x ? B * (size_t)XW : 0);
    if (u) HIP_TRY(c, hipMemcpyAsync(hu.data(), c->bits.p, hu.size() * 4, hipMemcpyDeviceToHost, c->stream));
    if (x) HIP_TRY(c, hipMemcpyAsync(hx.data(), c->enc_io.p, hx.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (u) unpack_rows(hu.data(), B, N, u);
    if (x) unpack_rows(hx.data(), B, W, x);
    return POLAR_OK;
}

int polar_payload_batch(polar_ctx *c, const int *u_hat, size_t B, int *payload, unsigned *crc_ok)
{
    if (!c || !u_hat || !payload || B > kMaxBatch) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(c->cfg.device);
    const int K = c->cfg.K, KW = (K + 31) / 32, N = c->cfg.N, NW = c->NW;
    int rc;
    if ((rc = ensure_nomem(c, c->in, B * KW * 4, kEncScratch))) return rc;
    if ((rc = ensure_nomem(c, c->bits, B * NW * 4, kEncScratch))) return rc;
    if ((rc = ensure_nomem(c, c->flags, B * 4, kEncScratch))) return rc;
    const std::vector<uint32_t> uw = pack_rows(u_hat, B, N);
    HIP_TRY(c, hipMemcpyAsync(c->bits.p, uw.data(), uw.size() * 4, hipMemcpyHostToDevice, c->stream));
    rc = polar_payload_device(c, (const uint32_t *)c->bits.p, B, (uint32_t *)c->in.p, (uint32_t *)c->flags.p);
    if (rc) return sync_fail(c, rc);
    std::vector<uint32_t> pw(B * (size_t)KW);
    HIP_TRY(c, hipMemcpyAsync(pw.data(), c->in.p, pw.size() * 4, hipMemcpyDeviceToHost, c->stream));
    if (crc_ok) HIP_TRY(c, hipMemcpyAsync(crc_ok, c->flags.p, B * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unpack_rows(pw.data(), B, K, payload);
    return POLAR_OK;
}

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

// ---- code books (include/polar_hip.h, "Code books") --------------------------------------------------------------------------
static_assert(polar::BOOK_RM_NONE == POLAR_RM_NONE && polar::BOOK_RM_REPEAT == POLAR_RM_REPEAT &&
                  polar::BOOK_RM_PUNCTURE == POLAR_RM_PUNCTURE && polar::BOOK_RM_SHORTEN == POLAR_RM_SHORTEN &&
                  polar::BOOK_RM_SHORT_LLR == POLAR_RM_SHORT_LLR && polar::BOOK_FLAG_NO_CODE == POLAR_FLAG_NO_CODE,
              "kernel and C ABI constants");

// A code book owns a snapshot of its members' tables (one device block, every table at a 64-byte boundary), the [C]
// descriptors that point into it, and an internal plain context of the largest member's N and the book's L and dtype: the
// book's stream, scratch, work queue and the staging of the host form are that context's.
struct polar_codebook {
    struct Member { int N, W, A; };
    polar_ctx *ictx = nullptr;
    std::vector<Member> members;
    int N_max = 0, W_max = 0, L = 0, dtype = POLAR_F64;
    bool sc = false;
    DevMem<unsigned char> d_tables;
    DevMem<polar::BookCode> d_codes;
    Buf code;   // polar_codebook_decode_host: the frames' code indices
    std::string kernel_name;
};

// rule 9 on the members alone: POLAR_OK, POLAR_EINVAL or POLAR_ENOKERNEL; nothing is touched
static int book_members_check(polar_ctx *const *members, int C)
{
    if (!members || C < 1 || C > polar::BOOK_MAX_C) return POLAR_EINVAL;
    for (int i = 0; i < C; ++i)
        if (!members[i]) return POLAR_EINVAL;
    const polar_cfg &g0 = members[0]->cfg;
    bool too_long = false;
    for (int i = 0; i < C; ++i) {
        const polar_ctx *m = members[i];
        const polar_cfg &g = m->cfg;
        const bool list = g.algo == POLAR_ALGO_SCL || g.algo == POLAR_ALGO_CASCL;
        if (!list && g.algo != POLAR_ALGO_SC) return POLAR_EINVAL;
        if ((g.algo == POLAR_ALGO_SC) != (g0.algo == POLAR_ALGO_SC)) return POLAR_EINVAL;
        if (g.dtype != POLAR_F64 && g.dtype != POLAR_F32) return POLAR_EINVAL;
        if (g.dtype != g0.dtype || g.L != g0.L || g.L > 32 || g.device != g0.device) return POLAR_EINVAL;
        if (m->sys_polar || m->cascl_stages.size() > 1) return POLAR_EINVAL;
        too_long |= g.N > polar::BOOK_MAX_N;
    }
    return too_long ? POLAR_ENOKERNEL : POLAR_OK;
}

int polar_codebook_create(polar_ctx *const *members, int C, polar_codebook **out)
{
    if (!out) return POLAR_EINVAL;
    *out = nullptr;
    int rc = book_members_check(members, C);
    if (rc) return rc;
    polar_codebook *cb = new (std::nothrow) polar_codebook();
    if (!cb) return POLAR_ENOMEM;
    auto cleanup = [&](int code) {
        polar_codebook_destroy(cb);
        return code;
    };
    const polar_cfg &g0 = members[0]->cfg;
    cb->L = g0.L;
    cb->dtype = g0.dtype;
    cb->sc = g0.algo == POLAR_ALGO_SC;
    for (int i = 0; i < C; ++i) {
        const polar_ctx *m = members[i];
        const int W = m->rm_mode != POLAR_RM_NONE ? m->rm_E : m->cfg.N;
        cb->members.push_back({m->cfg.N, W, m->A});
        cb->N_max = std::max(cb->N_max, m->cfg.N);
        cb->W_max = std::max(cb->W_max, W);
    }
    polar_cfg g{};
    g.N = cb->N_max; g.K = 1; g.L = cb->L; g.algo = cb->sc ? POLAR_ALGO_SC : POLAR_ALGO_SCL;
    g.dtype = cb->dtype; g.device = g0.device; g.bp_iters = 1;
    if ((rc = polar_create(&g, &cb->ictx))) return cleanup(rc);
    DeviceGuard guard(g0.device);

    // the snapshot: every table a member's decode reads, copied from the member's device tables into one host image
    struct Offsets { size_t frozen, crc, mask, row, ilv; bool has_crc, has_ilv; };
    std::vector<unsigned char> image;
    std::vector<Offsets> offs((size_t)C);
    auto room = [&](size_t bytes) {
        const size_t at = (image.size() + 63) & ~(size_t)63;
        image.resize(at + bytes, 0);
        return at;
    };
    hipError_t e = hipSuccess;
    auto fetch = [&](const void *dev, size_t bytes) {   // bytes of a member's device table -> their offset in the image
        const size_t at = room(bytes);
        if (e == hipSuccess) e = hipMemcpy(image.data() + at, dev, bytes, hipMemcpyDeviceToHost);
        return at;
    };
    for (int i = 0; i < C; ++i) {
        const polar_ctx *m = members[i];
        const size_t N = (size_t)m->cfg.N, NW = (size_t)m->NW, D = m->dyn_pos.size();
        Offsets &o = offs[(size_t)i];
        o.has_crc = m->cfg.algo == POLAR_ALGO_CASCL && m->d_crc_tab;
        o.has_ilv = m->rm_mode != POLAR_RM_NONE && m->rm_ibil && m->d_rm_ilv;
        o.frozen = fetch(m->d_frozen, NW * sizeof(uint32_t));
        o.crc = o.has_crc ? fetch(m->d_crc_tab, N * sizeof(uint32_t)) : 0;
        if (m->is_dyn && D > 0) {
            o.mask = fetch(m->d_dyn_mask, D * NW * sizeof(uint32_t));
            o.row = fetch(m->d_dyn_row, N * sizeof(int));
        } else {   // the D = 0 tables of list_tables(): one zero mask row, row -1 at every leaf
            o.mask = room(NW * sizeof(uint32_t));
            o.row = room(N * sizeof(int));
            std::memset(image.data() + o.row, 0xFF, N * sizeof(int));
        }
        o.ilv = o.has_ilv ? fetch(m->d_rm_ilv, (size_t)m->rm_E * sizeof(uint16_t)) : 0;
    }
    if (e != hipSuccess) return cleanup(fail(cb->ictx, e, "polar_codebook_create: reading a member's tables"));
    if ((rc = cb->d_tables.upload(image.data(), image.size()))) return cleanup(rc);
    std::vector<polar::BookCode> codes((size_t)C);
    const unsigned char *base = cb->d_tables.get();
    for (int i = 0; i < C; ++i) {
        const polar_ctx *m = members[i];
        const Offsets &o = offs[(size_t)i];
        polar::BookCode &d = codes[(size_t)i];
        d.frozen = reinterpret_cast<const uint32_t *>(base + o.frozen);
        d.crc_tab = o.has_crc ? reinterpret_cast<const uint32_t *>(base + o.crc) : nullptr;
        d.dyn_mask = reinterpret_cast<const uint32_t *>(base + o.mask);
        d.dyn_row = reinterpret_cast<const int *>(base + o.row);
        d.ilv = o.has_ilv ? reinterpret_cast<const uint16_t *>(base + o.ilv) : nullptr;
        d.N = m->cfg.N; d.n = m->n;
        d.E = m->rm_mode != POLAR_RM_NONE ? m->rm_E : m->cfg.N;
        d.logS = m->n - 5;
        d.rm_mode = m->rm_mode;
        d.sc_mode = m->cfg.algo == POLAR_ALGO_SC ? 1 : 0;
    }
    if ((rc = cb->d_codes.upload(codes.data(), codes.size()))) return cleanup(rc);
    char nm[128];
    snprintf(nm, sizeof nm, "k_scl_book<%s,L=%d> (C=%d codes, N_max=%d)", cb->dtype == POLAR_F32 ? "float" : "double", cb->L, C,
             cb->N_max);
    cb->kernel_name = nm;
    *out = cb;
    return POLAR_OK;
}

void polar_codebook_destroy(polar_codebook *cb)
{
    if (!cb) return;
    const int dev = cb->ictx ? cb->ictx->cfg.device : -1;
    polar_destroy(cb->ictx);   // synchronises the book's stream first
    if (dev < 0) {
        delete cb;
        return;
    }
    DeviceGuard guard(dev);
    delete cb;
}

int polar_codebook_info(const polar_codebook *cb, int *C, int *N_max, int *W_max, int *L, int *dtype)
{
    if (!cb) return POLAR_EINVAL;
    if (C) *C = (int)cb->members.size();
    if (N_max) *N_max = cb->N_max;
    if (W_max) *W_max = cb->W_max;
    if (L) *L = cb->L;
    if (dtype) *dtype = cb->dtype;
    return POLAR_OK;
}

int polar_codebook_member(const polar_codebook *cb, int c, int *N, int *W, int *A)
{
    if (!cb || c < 0 || c >= (int)cb->members.size()) return POLAR_EINVAL;
    if (N) *N = cb->members[(size_t)c].N;
    if (W) *W = cb->members[(size_t)c].W;
    if (A) *A = cb->members[(size_t)c].A;
    return POLAR_OK;
}

int polar_codebook_set_stream(polar_codebook *cb, void *s) { return cb ? polar_set_stream(cb->ictx, s) : POLAR_EINVAL; }
void *polar_codebook_get_stream(polar_codebook *cb) { return cb ? polar_get_stream(cb->ictx) : nullptr; }
int polar_codebook_synchronize(polar_codebook *cb) { return cb ? polar_synchronize(cb->ictx) : POLAR_EINVAL; }
const char *polar_codebook_kernel_name(const polar_codebook *cb) { return cb ? cb->kernel_name.c_str() : ""; }
const char *polar_codebook_last_error(const polar_codebook *cb) { return cb ? cb->ictx->last_error.c_str() : ""; }

// the arguments both device calls share (rule 9); any_out: at least one output is not NULL
static int book_call_check(const polar_codebook *cb, const void *d_in, int in_is_f32, size_t ld, const uint32_t *d_code, size_t B,
                           bool any_out)
{
    if (!cb || !d_in || !d_code || !any_out || B > kMaxBatch || ld < (size_t)cb->W_max) return POLAR_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_in) % (in_is_f32 ? 4 : 8)) return POLAR_EINVAL;
    return POLAR_OK;
}

static polar::SclParams book_params(const polar_codebook *cb, const void *d_in, double sigma, size_t B)
{
    polar::SclParams P{};
    P.in = d_in; P.sigma = sigma;
    P.N = cb->N_max; P.n = cb->ictx->n; P.B = (int)B;
    return P;
}

int polar_codebook_decode(polar_codebook *cb, const void *d_in, int in_is_f32, size_t ld, const uint32_t *d_code, double sigma,
                          size_t B, uint32_t *d_uhat_bits, double *d_pm, uint32_t *d_flags)
{
    int rc = book_call_check(cb, d_in, in_is_f32, ld, d_code, B, d_uhat_bits || d_pm || d_flags);
    if (rc) return rc;
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(cb->ictx->cfg.device);
    polar::SclParams P = book_params(cb, d_in, sigma, B);
    P.out_bits = d_uhat_bits; P.pm = d_pm; P.flags = d_flags;
    const polar::BookArgs K{cb->d_codes, d_code, (uint32_t)cb->members.size(), ld};
    return polar_tu::book_decode(cb->ictx, P, K, cb->dtype == POLAR_F32, in_is_f32 != 0);
}

int polar_codebook_list_decode(polar_codebook *cb, const void *d_in, int in_is_f32, size_t ld, const uint32_t *d_code, double sigma,
                               size_t B, uint32_t *d_paths, double *d_pm, uint32_t *d_rem, uint32_t *d_count, uint32_t *d_flags)
{
    int rc = book_call_check(cb, d_in, in_is_f32, ld, d_code, B, d_paths || d_pm || d_rem || d_count || d_flags);
    if (rc) return rc;
    if (cb->sc) return POLAR_EINVAL;   // an SC book has no list, as an SC context has none
    if (B == 0) return POLAR_OK;
    DeviceGuard guard(cb->ictx->cfg.device);
    polar::SclParams P = book_params(cb, d_in, sigma, B);
    P.flags = d_flags;
    const polar::BookArgs K{cb->d_codes, d_code, (uint32_t)cb->members.size(), ld};
    return polar_tu::book_list(cb->ictx, P, K, cb->dtype == POLAR_F32, in_is_f32 != 0, d_paths, d_pm, d_rem, d_count);
}

// host-buffer form: the batch goes through the device buffers in one piece
int polar_codebook_decode_host(polar_codebook *cb, const double *in, size_t ld, const uint32_t *code, double sigma, size_t B,
                               int *u_hat, double *pm, unsigned *flags)
{
    if (!cb || !in || !code || !u_hat || B > kMaxBatch || ld < (size_t)cb->W_max) return POLAR_EINVAL;
    if (B == 0) return POLAR_OK;
    polar_ctx *c = cb->ictx;
    DeviceGuard guard(c->cfg.device);
    const size_t NW = (size_t)cb->N_max / 32;
    static const char *what = "polar_codebook_decode_host";
    int rc;
    if ((rc = ensure_nomem(c, c->in, B * ld * sizeof(double), what))) return rc;
    if ((rc = ensure_nomem(c, cb->code, B * sizeof(uint32_t), what))) return rc;
    if ((rc = ensure_nomem(c, c->bits, B * NW * sizeof(uint32_t), what))) return rc;
    if (pm && (rc = ensure_nomem(c, c->pm, B * sizeof(double), what))) return rc;
    if (flags && (rc = ensure_nomem(c, c->flags, B * sizeof(uint32_t), what))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->in.p, in, B * ld * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(cb->code.p, code, B * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    rc = polar_codebook_decode(cb, c->in.p, 0, ld, (const uint32_t *)cb->code.p, sigma, B, (uint32_t *)c->bits.p,
                               pm ? (double *)c->pm.p : nullptr, flags ? (uint32_t *)c->flags.p : nullptr);
    if (rc) return sync_fail(c, rc);
    std::vector<uint32_t> w(B * NW);
    HIP_TRY(c, hipMemcpyAsync(w.data(), c->bits.p, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (pm) HIP_TRY(c, hipMemcpyAsync(pm, c->pm.p, B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (flags) HIP_TRY(c, hipMemcpyAsync(flags, c->flags.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unpack_rows(w.data(), B, cb->N_max, u_hat);
    return POLAR_OK;
}

// ---- frames sharded over the GPUs of one node, RCCL only for the final reduction -------------------------------
// RCCL is loaded on first use with dlopen (RTLD_LOCAL): the library has no link-time dependency on it, and a host process
// that carries its own copy (torch does) is not disturbed.
namespace {
struct RcclApi {
    void *handle = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
};
// ncclDataType_t / ncclRedOp_t as rccl.h numbers them (stable across NCCL 2.x: ncclUint32 = 3, ncclUint64 = 5,
// ncclSum = 0).  They are NOT trusted: polar_group_create runs known values through the loaded library with exactly
// these numbers (group_self_test) and refuses the group if the answer is not the 64-bit integer sum / the 32-bit
// gather in rank order -- a different enum layout or ABI gives POLAR_EDEVICE, never wrong counters.
constexpr int kNcclUint32 = 3, kNcclUint64 = 5, kNcclSum = 0;

RcclApi &rccl()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
        }
        if (!api.handle) return;
        api.CommInitAll = (int (*)(void **, int, const int *))dlsym(api.handle, "ncclCommInitAll");
        api.CommDestroy = (int (*)(void *))dlsym(api.handle, "ncclCommDestroy");
        api.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(api.handle, "ncclAllReduce");
        api.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(api.handle, "ncclAllGather");
        api.GroupStart = (int (*)())dlsym(api.handle, "ncclGroupStart");
        api.GroupEnd = (int (*)())dlsym(api.handle, "ncclGroupEnd");
        api.GetErrorString = (const char *(*)(int))dlsym(api.handle, "ncclGetErrorString");
        api.ok = api.CommInitAll && api.CommDestroy && api.AllReduce && api.AllGather && api.GroupStart && api.GroupEnd;
    });
    return api;
}
}  // namespace

struct polar_group {
    std::vector<polar_ctx *> ctx;
    std::vector<void *> comms;   // ncclComm_t per GPU
    std::vector<Buf> ferr;       // per GPU: its shard's per-frame error counts (exact stop rule)
    std::vector<Buf> recv;       // per GPU above 0: where the all-gather of the stop rule lands (GPU 0 receives into gathered)
    Buf gathered;                // GPU 0: the counts of all shards in frame order
    Buf cut_out;                 // GPU 0: k_stop_cut's three numbers
};

extern "C++" {
namespace {

// grouped collective over the ranks of the group, one call per rank between GroupStart / GroupEnd
template <typename F>
bool group_collective(polar_group *g, F &&per_rank)
{
    RcclApi &R = rccl();
    bool bad = R.GroupStart() != 0;
    for (int i = 0; i < (int)g->ctx.size() && !bad; ++i) {
        DeviceGuard guard(i);
        bad = per_rank(i) != 0;
    }
    return !((R.GroupEnd() != 0) || bad);
}

bool group_sync(polar_group *g)
{
    bool ok = true;
    for (int i = 0; i < (int)g->ctx.size(); ++i) {
        DeviceGuard guard(i);
        ok = (hipStreamSynchronize(g->ctx[(size_t)i]->stream) == hipSuccess) && ok;
    }
    return ok;
}

// Known answers through the loaded RCCL with the enum numbers this file uses: rank i contributes
// {2^40 + i + 1, 3} as uint64 -- the sum must be {n 2^40 + n(n+1)/2, 3n} (a 32-bit or floating type, or a different
// reduction, gives something else) -- and {0xC0DE0000 + i} as uint32, which must come back in rank order on every rank.
int group_self_test(polar_group *g)
{
    RcclApi &R = rccl();
    const int n = (int)g->ctx.size();
    for (int i = 0; i < n; ++i) {
        polar_ctx *c = g->ctx[(size_t)i];
        DeviceGuard guard(i);
        int rc = ensure(c, c->gen_cnt, 16);
        if (rc) return rc;
        if ((rc = ensure(c, g->ferr[(size_t)i], (size_t)(n + 1) * 4))) return rc;
        const unsigned long long v[2] = {(1ull << 40) + (unsigned long long)i + 1ull, 3ull};
        const uint32_t w = 0xC0DE0000u + (uint32_t)i;
        if (hipMemcpyAsync(c->gen_cnt.p, v, 16, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(g->ferr[(size_t)i].p, &w, 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return POLAR_EDEVICE;
    }
    if (!group_collective(g, [&](int i) {
            void *buf = g->ctx[(size_t)i]->gen_cnt.p;
            return R.AllReduce(buf, buf, 2, kNcclUint64, kNcclSum, g->comms[(size_t)i], g->ctx[(size_t)i]->stream);
        }))
        return POLAR_EDEVICE;
    if (!group_collective(g, [&](int i) {
            uint32_t *b = (uint32_t *)g->ferr[(size_t)i].p;
            return R.AllGather(b, b + 1, 1, kNcclUint32, g->comms[(size_t)i], g->ctx[(size_t)i]->stream);
        }))
        return POLAR_EDEVICE;
    const unsigned long long want0 = (unsigned long long)n * (1ull << 40) + (unsigned long long)n * (n + 1) / 2;
    for (int i = 0; i < n; ++i) {
        polar_ctx *c = g->ctx[(size_t)i];
        DeviceGuard guard(i);
        unsigned long long h[2] = {0, 0};
        std::vector<uint32_t> got((size_t)n);
        if (hipMemcpyAsync(h, c->gen_cnt.p, 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(got.data(), (uint32_t *)g->ferr[(size_t)i].p + 1, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return POLAR_EDEVICE;
        bool ok = h[0] == want0 && h[1] == 3ull * (unsigned long long)n;
        for (int q = 0; q < n; ++q) ok = ok && got[(size_t)q] == 0xC0DE0000u + (uint32_t)q;
        if (!ok) {
            c->last_error = "RCCL self-test: all-reduce(uint64, sum) / all-gather(uint32) did not return the known answer";
            return POLAR_EDEVICE;
        }
    }
    return POLAR_OK;
}

}  // namespace
}  // extern "C++"

void polar_group_destroy(polar_group *g)
{
    if (!g) return;
    RcclApi &R = rccl();
    for (void *cm : g->comms)
        if (cm && R.ok) (void)R.CommDestroy(cm);
    for (size_t i = 0; i < g->ferr.size(); ++i) {
        DeviceGuard guard((int)i);
        g->ferr[i].reset();
        g->recv[i].reset();
    }
    {
        DeviceGuard guard(0);
        g->gathered.reset();
        g->cut_out.reset();
    }
    for (polar_ctx *c : g->ctx) polar_destroy(c);
    delete g;
}

int polar_group_create(const polar_cfg *cfg, int ngpus, polar_group **out)
{
    if (!cfg || !out || ngpus < 1 || ngpus > 64) return POLAR_EINVAL;
    *out = nullptr;
    if (cfg->dtype == POLAR_Q8) return POLAR_EINVAL;   // the groups build float contexts only
    if ((cfg->algo == POLAR_ALGO_SCL || cfg->algo == POLAR_ALGO_CASCL) && cfg->L > 32) return POLAR_EINVAL;   // no wide lists in a group
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ngpus > ndev) return POLAR_EDEVICE;
    RcclApi &R = rccl();
    if (!R.ok) return POLAR_EDEVICE;   // no RCCL on this machine
    polar_group *g = new (std::nothrow) polar_group();
    if (!g) return POLAR_ENOMEM;
    g->ctx.assign((size_t)ngpus, nullptr);
    g->comms.assign((size_t)ngpus, nullptr);
    g->ferr.resize((size_t)ngpus);
    g->recv.resize((size_t)ngpus);
    std::vector<int> devs((size_t)ngpus);
    for (int i = 0; i < ngpus; ++i) {
        devs[(size_t)i] = i;
        polar_cfg one = *cfg;
        one.device = i;
        const int rc = polar_create(&one, &g->ctx[(size_t)i]);
        if (rc) {
            polar_group_destroy(g);
            return rc;
        }
    }
    if (R.CommInitAll(g->comms.data(), ngpus, devs.data()) != 0) {
        polar_group_destroy(g);
        return POLAR_EDEVICE;
    }
    const int st = group_self_test(g);   // wrong enum numbers / ABI: refuse the group instead of returning wrong counters
    if (st) {
        polar_group_destroy(g);
        return st;
    }
    *out = g;
    return POLAR_OK;
}

int polar_group_size(const polar_group *g) { return g ? (int)g->ctx.size() : 0; }

int polar_group_fer_batch(polar_group *g, unsigned long long seed, unsigned long long first_frame, double snr_db,
                          size_t frames_per_gpu, unsigned long long *block_errors, unsigned long long *bit_errors,
                          double *seconds)
{
    if (!g || !block_errors || !bit_errors) return POLAR_EINVAL;
    if (frames_per_gpu == 0) return POLAR_OK;
    RcclApi &R = rccl();
    const int ngpus = (int)g->ctx.size();
    std::vector<int> rcs((size_t)ngpus, POLAR_OK);
    std::vector<double> secs((size_t)ngpus, 0.0);
    // one host thread per GPU: its shard of the frame range, no data-path collective
    {
        std::vector<std::thread> th;
        for (int i = 0; i < ngpus; ++i)
            th.emplace_back([&, i] {
                polar_ctx *c = g->ctx[(size_t)i];
                DeviceGuard guard(i);
                const auto t0 = std::chrono::steady_clock::now();
                rcs[(size_t)i] = fer_batch_impl(c, seed, first_frame + (unsigned long long)i * frames_per_gpu, snr_db,
                                                frames_per_gpu, nullptr);
                if (rcs[(size_t)i] == POLAR_OK && hipStreamSynchronize(c->stream) != hipSuccess) rcs[(size_t)i] = POLAR_EDEVICE;
                secs[(size_t)i] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            });
        for (auto &t : th) t.join();
    }
    int rc = POLAR_OK;
    for (int i = 0; i < ngpus; ++i)
        if (rcs[(size_t)i]) rc = rcs[(size_t)i];
    // the only exchange: sum of the two counters over the GPUs (16 bytes per rank over xGMI)
    if (rc == POLAR_OK &&
        !group_collective(g, [&](int i) {
            void *buf = g->ctx[(size_t)i]->gen_cnt.p;
            return R.AllReduce(buf, buf, 2, kNcclUint64, kNcclSum, g->comms[(size_t)i], g->ctx[(size_t)i]->stream);
        }))
        rc = POLAR_EDEVICE;
    if (rc == POLAR_OK) {
        unsigned long long h[2] = {0, 0};
        {
            DeviceGuard guard(0);
            if (hipMemcpyAsync(h, g->ctx[0]->gen_cnt.p, 16, hipMemcpyDeviceToHost, g->ctx[0]->stream) != hipSuccess ||
                hipStreamSynchronize(g->ctx[0]->stream) != hipSuccess)
                rc = POLAR_EDEVICE;
        }
        for (int i = 1; i < ngpus; ++i) {   // every rank holds the sum: drain the other streams before the next call reuses the buffers
            DeviceGuard gg(i);
            if (hipStreamSynchronize(g->ctx[(size_t)i]->stream) != hipSuccess) rc = POLAR_EDEVICE;
        }
        if (rc == POLAR_OK) {
            *block_errors += h[0];
            *bit_errors += h[1];
        }
    }
    if (seconds) *seconds = *std::max_element(secs.begin(), secs.end());
    return rc;
}

// The reference's sequential stop rule (`for (run = 0; errBlock < BLE; run++)`, SCL_1024.c:228) over a batch that was
// decoded in shards: every GPU leaves the per-frame error counts of its shard on the device (k_count_errors), ONE
// ncclAllGather of frames_per_gpu x uint32 per rank puts them in frame order on every GPU, and k_stop_cut on GPU 0 finds the
// frame that brings the block errors to `need` exactly as polar_stop_rule_cut_device does for one GPU.  Frame f of the
// range is the same frame for every ngpus, so the three numbers do not depend on how many GPUs shared the batch.
int polar_group_stop_rule_batch(polar_group *g, unsigned long long seed, unsigned long long first_frame, double snr_db,
                                size_t frames_per_gpu, unsigned need, size_t min_frames, size_t *frames_used,
                                unsigned long long *block_errors, unsigned long long *bit_errors)
{
    if (!g || !frames_used || !block_errors || !bit_errors) return POLAR_EINVAL;
    const int ngpus = (int)g->ctx.size();
    const size_t total = frames_per_gpu * (size_t)ngpus;
    if (frames_per_gpu == 0 || total > kMaxBatch || min_frames > total) return POLAR_EINVAL;
    RcclApi &R = rccl();
    int rc = POLAR_OK;
    for (int i = 0; i < ngpus && !rc; ++i) {
        DeviceGuard guard(i);
        rc = ensure(g->ctx[(size_t)i], g->ferr[(size_t)i], std::max(frames_per_gpu, (size_t)ngpus + 1) * 4);
    }
    {
        DeviceGuard guard(0);
        if (!rc) rc = ensure(g->ctx[0], g->gathered, total * 4);
        if (!rc) rc = ensure(g->ctx[0], g->cut_out, 3 * sizeof(unsigned long long));
    }
    if (rc) return rc;
    std::vector<int> rcs((size_t)ngpus, POLAR_OK);
    {
        std::vector<std::thread> th;
        for (int i = 0; i < ngpus; ++i)
            th.emplace_back([&, i] {
                polar_ctx *c = g->ctx[(size_t)i];
                DeviceGuard guard(i);
                rcs[(size_t)i] = fer_batch_impl(c, seed, first_frame + (unsigned long long)i * frames_per_gpu, snr_db,
                                                frames_per_gpu, nullptr, (uint32_t *)g->ferr[(size_t)i].p);
                if (rcs[(size_t)i] == POLAR_OK && hipStreamSynchronize(c->stream) != hipSuccess) rcs[(size_t)i] = POLAR_EDEVICE;
            });
        for (auto &t : th) t.join();
    }
    for (int i = 0; i < ngpus; ++i)
        if (rcs[(size_t)i]) return rcs[(size_t)i];
    // rank i's counts land at [i * frames_per_gpu, (i + 1) * frames_per_gpu) of every rank's receive buffer; only
    // GPU 0's copy is used (ranks > 0 receive into a buffer of the same size, as the collective requires)
    // (the buffers belong to the group and only grow: nothing is allocated between GroupStart and GroupEnd)
    std::vector<void *> recv((size_t)ngpus);
    recv[0] = g->gathered.p;
    for (int i = 1; i < ngpus && !rc; ++i) {
        DeviceGuard guard(i);
        rc = ensure_nomem(g->ctx[(size_t)i], g->recv[(size_t)i], total * 4, "group receive buffer");
        recv[(size_t)i] = g->recv[(size_t)i].p;
    }
    if (!rc && !group_collective(g, [&](int i) {
            return R.AllGather(g->ferr[(size_t)i].p, recv[(size_t)i], frames_per_gpu, kNcclUint32, g->comms[(size_t)i],
                               g->ctx[(size_t)i]->stream);
        }))
        rc = POLAR_EDEVICE;
    if (!rc && !group_sync(g)) rc = POLAR_EDEVICE;
    if (rc) return rc;
    unsigned long long h[3] = {0, 0, 0};
    {
        DeviceGuard guard(0);
        polar_ctx *c0 = g->ctx[0];
        rc = polar_stop_rule_cut_device(c0, (const uint32_t *)g->gathered.p, total, need, min_frames,
                                        (unsigned long long *)g->cut_out.p);
        if (rc) return rc;
        if (hipMemcpyAsync(h, g->cut_out.p, sizeof h, hipMemcpyDeviceToHost, c0->stream) != hipSuccess ||
            hipStreamSynchronize(c0->stream) != hipSuccess)
            return POLAR_EDEVICE;
    }
    *frames_used = (size_t)h[0];
    *block_errors = h[1];
    *bit_errors = h[2];
    return POLAR_OK;
}

int polar_fer_multi_gpu(const polar_cfg *cfg, int ngpus, unsigned long long seed, unsigned long long first_frame, double snr_db,
                        size_t frames_per_gpu, unsigned long long *block_errors, unsigned long long *bit_errors,
                        double *seconds)
{
    if (!block_errors || !bit_errors) return POLAR_EINVAL;
    polar_group *g = nullptr;
    int rc = polar_group_create(cfg, ngpus, &g);
    if (rc) return rc;
    rc = polar_group_fer_batch(g, seed, first_frame, snr_db, frames_per_gpu, block_errors, bit_errors, seconds);
    polar_group_destroy(g);
    return rc;
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
#endif  // POLAR_TESTING

int polar_time_decode_device(polar_ctx *c, const void *d_in, int in_is_f32, double sigma, size_t B,
                             uint32_t *d_bits, int reps, float *ms)
{
    if (!c || !ms || reps < 1) return POLAR_EINVAL;
    DeviceGuard guard(c->cfg.device);
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < reps; ++i) {
        int rc = decode_device_impl(c, d_in, in_is_f32, sigma, B, d_bits, nullptr, nullptr, c->d_frozen);
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
