// h_book.hip -- code books: one launch decodes frames of different codes.
#include "polar_hostlib.h"

using namespace polar_host;

extern "C" {

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

}  // extern "C"
