// h_enc.hip -- encoder, payload extraction, systematic polar codes.
#include "polar_hostlib.h"

#include "polar_bits.h"

using namespace polar_host;

extern "C" {

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

}  // extern "C"
