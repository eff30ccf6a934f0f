"""Monte-Carlo code construction (include/polar_hip.h, "Monte-Carlo code construction", rules 1-4), host side.

The model: genie-aided SC for the all-zero codeword is SC with EVERY leaf frozen, so `genie_model` is `sc_run` of
tests/test_scf_host.py (numpy on the oracle's check node; it returns every leaf's LLR) with an all-ones frozen set, then
rule 2's two comparisons.  Checked here for its properties and against the oracle's real SC; tests/test_gpu_construct.py
holds the kernels to it exactly.  polar_construct_order (rule 4) is host code of the library and is checked here through the
library, which loads without a GPU.  Also: the new C ABI is declared and exported, and the cases of the GPU exactness test
are shown not to be vacuous."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_scf_host import sc_run  # noqa: E402

# (N, sigma, B, seed) of the GPU exactness test (tests/test_gpu_construct.py), noise rows of design_rows().  The ragged
# sizes (B = 1, 63, 64k + 37) sit at the small N.  Every one of them must pass test_exactness_cases_are_not_vacuous below.
EXACT_CASES = [
    (32, 0.8, 4096, 11), (128, 0.8, 2048, 12), (512, 0.8, 1024, 13), (1024, 0.8, 512, 14), (2048, 0.8, 512, 15),
    (4096, 0.8, 256, 16),
    (32, 1.0, 1, 21), (32, 0.8, 63, 22), (32, 0.8, 64 * 5 + 37, 23), (64, 0.8, 64 * 9 + 37, 24),
    (128, 1.0, 1, 25), (128, 0.8, 63, 26), (128, 0.8, 64 * 3 + 37, 27),
]
EXACT_DTYPES = (np.float64, np.float32)


def design_rows(N, B, sigma, seed):
    """[B][N] float64 channel LLRs of the all-zero codeword over BPSK + AWGN: 2*y/sigma/sigma, y = 1 + sigma * z."""
    z = np.random.default_rng(seed).standard_normal((B, N))
    return 2 * (1 + sigma * z) / sigma / sigma


def genie_model(oracle, llr, dtype=np.float64):
    """Rules 1-2: (err [N], tie [N], lambda [B][N], u_hat [B][N]) of the rows llr [B][N] in `dtype`."""
    llr = np.ascontiguousarray(llr, dtype=dtype)
    N = llr.shape[1]
    u, lam = sc_run(oracle, np.ones(N, dtype=np.uint8), llr, dtype=dtype)
    assert lam.dtype == dtype
    err = (lam < 0).sum(axis=0).astype(np.uint64)
    tie = (lam == 0).sum(axis=0).astype(np.uint64)
    return err, tie, lam, u


def order_model(N, counts, base):
    """Rule 4 in numpy: descending 2*err + tie, equal scores in the order of `base`."""
    score = 2 * counts[0].astype(object) + counts[1].astype(object)
    return np.asarray(sorted(list(base), key=lambda j: -score[j]), dtype=np.int32)   # sorted() is stable


def _lib():
    import polardecoding_amd as pa
    if not os.path.exists(pa.lib_path()):
        import __graft_entry__ as g
        g.build()
    return pa.load_library()


# ---- the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", EXACT_DTYPES)
def test_model_properties(dtype, oracle):
    N, sigma, B = 128, 0.8, 2048
    err, tie, lam, u = genie_model(oracle, design_rows(N, B, sigma, 5), dtype)
    assert not u.any()                       # all decisions 0: every leaf is frozen
    assert ((err + tie) <= B).all()
    assert not np.isnan(lam).any() and tie.sum() == 0
    frac = err[0] / B
    print(f"N={N} B={B} leaf 0 errs on {frac:.4f}, arg-max leaf {int(err.argmax())}, err[N-1]={int(err[-1])}")
    assert abs(frac - 0.5) <= 0.06           # leaf 0 carries almost nothing (it need not be the arg-max)
    assert err[N - 1] == 0                   # the best channel never errs here


@pytest.mark.parametrize("dtype", EXACT_DTYPES)
def test_model_zero_rows_tie_everywhere_and_huge_rows_stay_finite(dtype, oracle):
    N, B = 64, 5
    err, tie, lam, u = genie_model(oracle, np.zeros((B, N)), dtype)
    assert (tie == B).all() and not err.any() and not u.any()
    err, tie, lam, _ = genie_model(oracle, -np.zeros((B, N)), dtype)   # -0.0 is a tie
    assert (tie == B).all() and not err.any()
    err, tie, lam, _ = genie_model(oracle, np.full((B, N), 1e30), np.float64)
    assert np.isfinite(lam).all() and not err.any() and not tie.any()
    print("largest lambda on rows of 1e30:", lam.max())


@pytest.mark.parametrize("N", [128, 512])
def test_model_agrees_with_the_oracles_sc_on_all_zero_decisions(N, oracle):
    """Where the oracle's real SC (K = N/2) decides the all-zero word, its partial sums are the genie's, so the model's
    lambda at the information leaves must decide 0 as well, on every such row."""
    sigma, B = 0.6, 256
    llr = design_rows(N, B, sigma, 40 + N)
    code = oracle.Code(N, N // 2)
    ref, _, _ = oracle.decode(code, llr, "SC")
    rows = ~ref.any(axis=1)
    assert rows.sum() >= B // 2, "low noise: most rows decode to the all-zero word"
    _, _, lam, _ = genie_model(oracle, llr[rows])
    info = np.flatnonzero(np.asarray(code.frozen) == 0)
    assert len(info) == N // 2
    assert (lam[:, info] >= 0).all()


@pytest.mark.parametrize("dtype", EXACT_DTYPES)
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "N%d-s%g-B%d" % c[:3])
def test_exactness_cases_are_not_vacuous(case, dtype, oracle):
    """Stated condition: each case of the GPU exactness test shows at least N/8 leaves with err > 0 and at least N/8 leaves
    with err = 0 in the model, so agreement is neither all-zero nor all-B counters."""
    N, sigma, B, seed = case
    err, tie, lam, _ = genie_model(oracle, design_rows(N, B, sigma, seed), dtype)
    print(f"N={N} sigma={sigma} B={B} {np.dtype(dtype).name}: leaves err=0 {(err == 0).sum()}, err>0 {(err > 0).sum()}, ties {tie.sum()}")
    assert (err > 0).sum() >= N // 8
    assert (err == 0).sum() >= N // 8
    assert not np.isnan(lam).any()


# ---- polar_construct_order ---------------------------------------------------------------------------------------------
def _order(lib, N, counts, base=None):
    cnt = np.ascontiguousarray(counts, dtype=np.uint64)
    out = np.full(N, -7, dtype=np.int32)
    b = None if base is None else np.ascontiguousarray(base, dtype=np.int32)
    rc = lib.polar_construct_order(N, cnt.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   None if b is None else b.ctypes.data_as(C.POINTER(C.c_int)),
                                   out.ctypes.data_as(C.POINTER(C.c_int)))
    return rc, out


@pytest.mark.parametrize("N", [32, 64, 128, 512, 1024, 2048, 4096])
def test_order_of_zero_counters_is_the_base_order(N, oracle):
    import polardecoding_amd as pa
    lib = _lib()
    rc, out = _order(lib, N, np.zeros((2, N)))
    assert rc == 0 and sorted(out.tolist()) == list(range(N))
    if N <= 1024:
        assert out.tolist() == oracle.q_for(N) == pa.q_sequence(N)
    else:   # polarization weight, beta = 2^(1/4), ascending, equal weights by index
        w = [sum(2 ** (b / 4) for b in range(N.bit_length() - 1) if (j >> b) & 1) for j in range(N)]
        assert sorted(w[j] for j in out) == [w[j] for j in out]
        assert out[0] == 0 and out[-1] == N - 1
    perm = np.random.default_rng(N).permutation(N).astype(np.int32)
    rc, out = _order(lib, N, np.zeros((2, N)), perm)
    assert rc == 0 and out.tolist() == perm.tolist()
    assert pa.construct_order(N, np.zeros((2, N), dtype=np.uint64)).tolist() == _order(lib, N, np.zeros((2, N)))[1].tolist()


def test_order_default_top_entries_are_what_polar_create_derives(oracle):
    """out + N - A of the default base order is the info_order polar_create derives for A unfrozen positions (N <= 1024:
    the 5G sequence restricted to < N, which is also what the oracle's Code uses)."""
    lib = _lib()
    for N, A in ((32, 16), (128, 64), (128, 70), (1024, 512), (1024, 536)):
        rc, out = _order(lib, N, np.zeros((2, N)))
        assert rc == 0
        assert out[N - A:].tolist() == oracle.q_for(N)[N - A:]
        frozen = np.ones(N, dtype=np.uint8)
        frozen[out[N - A:]] = 0
        assert frozen.tolist() == list(oracle.Code(N, A).frozen)


@pytest.mark.parametrize("N", [32, 256, 4096])
def test_order_random_counters(N):
    lib = _lib()
    rng = np.random.default_rng(7 * N)
    for hi in (3, 1000, 2 ** 40):
        counts = rng.integers(0, hi, size=(2, N)).astype(np.uint64)
        base = rng.permutation(N).astype(np.int32)
        rc, out = _order(lib, N, counts, base)
        assert rc == 0
        assert sorted(out.tolist()) == list(range(N))                     # a permutation
        score = 2 * counts[0].astype(object) + counts[1].astype(object)
        s = [score[j] for j in out]
        assert all(a >= b for a, b in zip(s, s[1:]))                      # descending score
        assert out.tolist() == order_model(N, counts, base).tolist()      # ties in base order
        rc, out = _order(lib, N, counts)
        assert rc == 0 and out.tolist() == order_model(N, counts, _order(lib, N, np.zeros((2, N)))[1]).tolist()


def test_order_weights_err_twice_tie():
    lib = _lib()
    N = 32
    base = np.arange(N, dtype=np.int32)
    c = np.zeros((2, N), dtype=np.uint64)
    c[0, 5] = 1          # one err
    c[1, 9] = 1          # one tie
    c[1, 20] = 2         # two ties = one err: equal scores, base order decides (5 before 20)
    rc, out = _order(lib, N, c, base)
    assert rc == 0 and out[:3].tolist() == [5, 20, 9]
    rc, out = _order(lib, N, c, base[::-1].copy())
    assert rc == 0 and out[:3].tolist() == [20, 5, 9]
    assert out[3:].tolist() == [j for j in base[::-1] if j not in (5, 9, 20)]
    c[:] = 0
    c[0, 3] = np.uint64(2 ** 63 + 5)   # 2 * err does not fit 64 bits: the score is wider than the counters
    c[0, 4] = np.uint64(7)
    c[1, 6] = np.uint64(2 ** 64 - 1)
    rc, out = _order(lib, N, c, base)
    assert rc == 0 and out[:3].tolist() == [3, 6, 4]


def test_order_refusals():
    lib = _lib()
    z = np.zeros((2, 8192), dtype=np.uint64)
    out = np.zeros(8192, dtype=np.int32)
    cp, op = z.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_int))
    for N in (0, 16, 48, 96, 8192, -32):
        assert lib.polar_construct_order(N, cp, None, op) == -1, N
    assert lib.polar_construct_order(64, None, None, op) == -1
    assert lib.polar_construct_order(64, cp, None, None) == -1
    for bad in (np.zeros(64), np.r_[np.arange(63), 64], np.r_[np.arange(63), -1], np.r_[0, np.arange(63)]):
        b = np.ascontiguousarray(bad, dtype=np.int32)
        assert lib.polar_construct_order(64, cp, b.ctypes.data_as(C.POINTER(C.c_int)), op) == -1
    assert lib.polar_construct_order(64, cp, None, op) == 0


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_construct_abi_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "polar_hip.h")).read(), flags=re.S)
    names = ("polar_genie_count_device", "polar_genie_rows_device", "polar_construct_batch", "polar_construct_order")
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    _lib()
    for lib in ("libpolar_hip.so", "libpolar_hip_testing.so"):
        path = os.path.join(REPO, "polardecoding_amd", "lib", lib)
        assert os.path.exists(path), "build the library first (__graft_entry__.build())"
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in names:
            assert re.search(r"\b" + name + r"\b", out), (lib, name)
    import polardecoding_amd as pa
    assert callable(pa.construct_order) and callable(pa.construct_mc)
    for m in ("genie_count_device", "genie_rows_device", "construct_batch"):
        assert callable(getattr(pa.Decoder, m)), m
