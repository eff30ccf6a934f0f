"""CPU: soft-output SCAN (POLAR_ALGO_SCAN, include/polar_hip.h).

scan_model() restates rules 1-8 of the header in numpy, vectorised over frames, on the oracle's CHK (CHK-inf is a np.where
around it).  With skip=True it applies the three consequences a kernel may use (all-frozen subtrees never entered,
all-information subtrees entered in the last iteration only and downwards only); the tests here hold the two forms equal.
tests/test_gpu_scan.py checks the library against it.  Also: the new C ABI is declared and exported."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def scan_model(frozen, llr, iters, dtype=np.float64, oracle=None, skip=False, stored=None):
    """Rules 1-8: (u_hat [B][N] int32, llr_u [B][N], ext_x [B][N]) of rows llr [B][N] after `iters` iterations in `dtype`.
    stored (a dict, optional) receives the stored right-child betas, key (level, first leaf)."""
    if oracle is None:
        from oracle import oracle_py as oracle
    fz = np.asarray(frozen) != 0
    N = fz.size
    n = N.bit_length() - 1
    assert 1 << n == N and iters >= 1
    llr = np.ascontiguousarray(llr, dtype=dtype).reshape(-1, N)
    B = llr.shape[0]
    inf = dtype(np.inf)
    zero = dtype(0)
    lam = np.full((B, N), inf, dtype=dtype)
    st = {} if stored is None else stored
    st.clear()

    def chk(a, b):
        return oracle.math(0, a.ravel(), b.ravel(), dtype=dtype).reshape(a.shape)

    def chk_inf(a, b):
        ai, bi = a == inf, b == inf
        r = chk(np.where(ai, zero, a), np.where(bi, zero, b))   # the value at an infinite operand is never used
        r = np.where(ai, b, r)
        return np.where(bi, a, r).astype(dtype)

    def down(t, s, alpha):   # an all-information subtree in the last iteration: alpha_l = chk(a, b), alpha_r = b
        if t == 0:
            lam[:, s] = alpha[:, 0]
            return
        h = 1 << (t - 1)
        down(t - 1, s, chk(alpha[:, :h], alpha[:, h:]))
        down(t - 1, s + h, alpha[:, h:])

    def visit(t, s, alpha, last):
        w = 1 << t
        f = fz[s:s + w]
        if skip and f.all():
            return np.full((B, w), inf, dtype=dtype)
        if skip and not f.any():
            if last:
                down(t, s, alpha)
            return np.zeros((B, w), dtype=dtype)
        if t == 0:                                                   # rule 1
            lam[:, s] = alpha[:, 0]
            return np.full((B, 1), inf if f[0] else zero, dtype=dtype)
        h = w // 2
        key = (t - 1, s + h)
        if key not in st:                                            # rule 2
            st[key] = np.full((B, h), inf if fz[s + h:s + w].all() else zero, dtype=dtype)
        a0, a1 = alpha[:, :h], alpha[:, h:]
        bl = visit(t - 1, s, chk_inf(a0, a1 + st[key]), last)        # rule 3
        br = visit(t - 1, s + h, a1 + chk_inf(a0, bl), last)         # rule 4
        st[key] = br
        return np.concatenate([chk_inf(bl, br + a1), br + chk_inf(bl, a0)], axis=1)   # rule 5

    ext = None
    with np.errstate(invalid="raise", over="raise"):                 # no inf - inf, no overflow: anywhere, ever
        for it in range(1, iters + 1):                               # rule 6
            ext = visit(n, 0, llr, it == iters)
    u = np.where(fz[None, :], 0, lam < 0).astype(np.int32)           # rule 7
    return u, np.where(fz[None, :], inf, lam).astype(dtype), ext.astype(dtype)


def oracle_frames(oracle, code, per, seed, dbs):
    llr, us = [], []
    for k, db in enumerate(dbs):
        sig = oracle.sigma_from_db(db)
        u, y = oracle.Sim(seed + k).frames(code, sig, per)
        us.append(u)
        llr += [oracle.llr_from_y(v, sig) for v in y]
    return np.stack(llr), np.concatenate(us)


def breaking_mask(N, seed):
    """A random mask that breaks the partial order, with all-frozen and all-information right children under mixed parents."""
    rng = np.random.default_rng(seed)
    fz = (rng.random(N) < 0.5).astype(np.uint8)
    fz[0], fz[1] = 0, 1                   # an information leaf before a frozen one
    fz[N - N // 4:] = 1                   # the right child of [N/2, N) all frozen, its left sibling mixed
    fz[N // 4 + N // 8:N // 2] = 0        # the right child of [N/4, N/2) all information
    fz[N // 4] = 1
    fz[24:32] = 1                         # inside one 32-leaf block too
    fz[16] = 0
    fz[40:48] = 0
    fz[32] = 1
    return fz


CASES = [(128, 64, 500, (1.0, 1.5, 2.0, 2.5)), (1024, 512, 40, (1.0, 2.0))]


@pytest.mark.parametrize("N,K,per,dbs", CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_model_values_are_sane(N, K, per, dbs, dtype, oracle):
    code = oracle.Code(N, K)
    llr, _ = oracle_frames(oracle, code, per, 900 + N, dbs)
    assert N != 128 or len(llr) >= 2000
    fz = np.asarray(code.frozen) != 0
    for iters in (1, 3):
        st = {}
        u, lu, ex = scan_model(code.frozen, llr, iters, dtype=dtype, oracle=oracle, stored=st)
        assert lu.dtype == dtype and ex.dtype == dtype
        for v in [lu, ex] + list(st.values()):
            assert not np.isnan(v).any() and not (v == -np.inf).any()
            assert (np.isinf(v) == np.isinf(v[0])[None, :]).all()    # +inf where the mask says, the same for all frames
        assert np.isfinite(lu[:, ~fz]).all() and np.isinf(lu[:, fz]).all()
        assert np.array_equal(u[:, ~fz], (lu[:, ~fz] < 0).astype(np.int32)) and not u[:, fz].any()


def test_all_information_code(oracle):
    N = 64
    rng = np.random.default_rng(5)
    llr = rng.normal(0.5, 2.0, size=(50, N))
    for iters in (1, 2):
        u, lu, ex = scan_model(np.zeros(N, dtype=np.uint8), llr, iters, oracle=oracle)
        assert (ex == 0).all()
        # SC's schedule with every partial sum soft and zero: f on the way left, the lower half on the way right
        want = np.empty_like(llr)
        for j in range(N):
            a = llr
            for t in range(N.bit_length() - 2, -1, -1):
                h = a.shape[1] // 2
                a = a[:, h:] if (j >> t) & 1 else oracle.math(0, a[:, :h].ravel(), a[:, h:].ravel()).reshape(-1, h)
            want[:, j] = a[:, 0]
        assert np.array_equal(lu, want)
        assert np.array_equal(u, (want < 0).astype(np.int32))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_information_leaf_by_hand(dtype, oracle):
    """N = 4, only leaf 3 unfrozen: a repetition code.  Every CHK-inf has an infinite operand, so the outputs are sums."""
    l = np.array([[0.7, -1.9, 0.3, 2.2], [-0.1, 0.4, -3.0, 0.2]], dtype=dtype)
    for iters in (1, 2, 5):
        u, lu, ex = scan_model([1, 1, 1, 0], l, iters, dtype=dtype, oracle=oracle)
        r0, r1 = l[:, 2] + l[:, 0], l[:, 3] + l[:, 1]
        assert np.array_equal(lu[:, 3], r1 + r0) and np.isinf(lu[:, :3]).all()
        assert np.array_equal(u[:, 3], (r1 + r0 < 0).astype(np.int32)) and not u[:, :3].any()
        want = np.stack([r1 + l[:, 2], r0 + l[:, 3], r1 + l[:, 0], r0 + l[:, 1]], axis=1)
        assert np.array_equal(ex, want)


@pytest.mark.parametrize("N,K,per,dbs", [(128, 64, 500, (1.0, 1.5, 2.0, 2.5)), (1024, 512, 100, (1.0, 1.5, 2.0))])
def test_block_errors_do_not_increase_with_iterations(N, K, per, dbs, oracle):
    code = oracle.Code(N, K)
    llr, us = oracle_frames(oracle, code, per, 1300 + N, dbs)
    io = code.info_order
    errs = {}
    for iters in (1, 4):
        u, _, _ = scan_model(code.frozen, llr, iters, oracle=oracle, skip=True)
        errs[iters] = int((u[:, io] != us[:, io]).any(axis=1).sum())
    print(f"N={N}: block errors I=1 {errs[1]}, I=4 {errs[4]} of {len(llr)}")
    assert 0 < errs[4] <= errs[1]


@pytest.mark.parametrize("which", ["5g_128", "5g_1024", "rate_0.9", "rate_0.1", "breaking_128", "breaking_256"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_skipping_rules_preserve_every_value(which, dtype, oracle):
    if which.startswith("5g"):
        N = int(which.split("_")[1])
        code = oracle.Code(N, N // 2)
        fz = np.asarray(code.frozen)
    elif which.startswith("rate"):
        N = 256
        code = oracle.Code(N, 230 if which == "rate_0.9" else 26)
        fz = np.asarray(code.frozen)
    else:
        N = int(which.split("_")[1])
        fz = breaking_mask(N, 77 + N)
    rng = np.random.default_rng(N)
    B = 24 if N == 1024 else 96
    sig = 0.8
    llr = 2 * (1 + sig * rng.normal(size=(B, N))) / sig / sig
    for iters in (1, 2, 4):
        sa, sb = {}, {}
        a = scan_model(fz, llr, iters, dtype=dtype, oracle=oracle, skip=False, stored=sa)
        b = scan_model(fz, llr, iters, dtype=dtype, oracle=oracle, skip=True, stored=sb)
        for x, y in zip(a, b):
            assert (x == y).all()
        assert sb and set(sb) <= set(sa)
        for k in sb:
            assert (sa[k] == sb[k]).all(), k


def test_scan_abi_is_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    assert re.search(r"#define\s+POLAR_ALGO_SCAN\s+5\b", hdr)
    names = ("polar_scan_set_iters", "polar_scan_decode_device", "polar_scan_decode_batch")
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    lib = os.path.join(REPO, "polardecoding_amd", "lib", "libpolar_hip.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in names:
        assert re.search(r"\b" + name + r"\b", out), name
    import polardecoding_amd as pa
    assert pa.ALGO_SCAN == 5 and callable(pa.SCAN)
    for m in ("set_scan_iters", "decode_scan_device", "decode_scan_batch"):
        assert callable(getattr(pa.Decoder, m)), m
