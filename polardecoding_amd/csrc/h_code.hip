// h_code.hip -- code construction without a launch: reliability order, CRC tables, the phase end of the pair kernel; the
// host rules of 5G rate matching and dynamic frozen bits with their entry points.
#include "polar_hostlib.h"

using namespace polar_host;

namespace {

const int kQ5G[1024] = {
#include "q5g_table.inc"
};

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

}  // namespace

namespace polar_host {

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

// contexts whose code carries a CRC: r, crc_tab, the generator's CRC multiply, the systematic K-bit error metric
// (BP list decoding: optional, crc_r = 0 is a code without one)
bool has_crc(int algo) { return algo == POLAR_ALGO_CASCL || algo == POLAR_ALGO_SCF || algo == POLAR_ALGO_BPL; }

// I[0..A) on the device, built on first use: the generators and the encoder side read it
int info_order_table(polar_ctx *c)
{
    if (c->d_info_order) return POLAR_OK;
    hipError_t e = hipSuccess;
    if (c->d_info_order.upload(c->info_order.data(), (size_t)c->A, &e)) return fail(c, e, "info_order table");
    return POLAR_OK;
}

}  // namespace polar_host

extern "C" {

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

}  // extern "C"
