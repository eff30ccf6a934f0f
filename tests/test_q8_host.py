"""CPU: fixed-point min-sum decoding (include/polar_hip.h, dtype POLAR_Q8).  The host quantiser against the model's, the
model's list decoder against an exhaustive search over all words, and every refusal that is decided before a device is
touched.  polar_q8_set_quant needs a ctx, and a ctx needs a device: its range checks are in tests/test_gpu_q8.py."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import q8_model as M  # noqa: E402

CRC6 = (0, 5, 6)
EINVAL, EDEVICE, ENOKERNEL = -1, -3, -4
Q8 = 2


def _lib():
    import polardecoding_amd as pa
    lib = pa.load_library()
    lib.polar_q8_quantize_host.argtypes = [C.POINTER(C.c_double), C.c_size_t, C.c_double, C.c_double, C.c_int,
                                           C.POINTER(C.c_int8)]
    return pa, lib


def _quantize_host(lib, v, sigma, scale, qc):
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.full(v.size, 99, dtype=np.int8)
    rc = lib.polar_q8_quantize_host(v.ctypes.data_as(C.POINTER(C.c_double)), v.size, sigma, scale, qc,
                                    out.ctypes.data_as(C.POINTER(C.c_int8)))
    return rc, out


# ---- rule 1 -------------------------------------------------------------------------------------------------------------
def _quantiser_inputs():
    rng = np.random.default_rng(8)
    halves = np.arange(-260, 261) / 2.0                       # k + 0.5: ties to even; the integers in between
    big = np.array([1e3, -1e3, 1e30, -1e30, 1e308, -1e308, np.inf, -np.inf, np.nan, 0.0, -0.0, 127.49, 127.5, -127.5, 128.0])
    near = np.nextafter(halves, np.inf), np.nextafter(halves, -np.inf)
    return np.concatenate([halves, big, near[0], near[1], rng.normal(0, 40, 500), rng.normal(0, 3, 500)])


@pytest.mark.parametrize("qc", [2, 5, 8])
@pytest.mark.parametrize("scale", [1.0, 2.0, 0.3, 7.25])
def test_quantize_host_is_the_model(qc, scale):
    _, lib = _lib()
    v = _quantiser_inputs() / scale if scale in (1.0, 2.0) else _quantiser_inputs()
    v = np.concatenate([v, _quantiser_inputs()])
    rc, q = _quantize_host(lib, v, 0.0, scale, qc)
    assert rc == 0
    want = M.quantize(v, scale, qc)
    assert np.array_equal(q, want)
    Cc = M.clamp_of(qc)
    assert q.max() == Cc and q.min() == -Cc                   # the clamp is reached on both sides, -128 never appears
    # halves go to the even neighbour, NaN to 0, infinities to the clamp
    assert _quantize_host(lib, [0.5, 1.5, 2.5, -0.5, -1.5, -2.5], 0.0, 1.0, 8)[1].tolist() == [0, 2, 2, 0, -2, -2]
    assert _quantize_host(lib, [np.nan, np.inf, -np.inf], 0.0, scale, qc)[1].tolist() == [0, Cc, -Cc]


@pytest.mark.parametrize("sigma", [0.7079457843841379, 1.0, 0.31])
def test_quantize_host_with_sigma(sigma):
    _, lib = _lib()
    y = np.concatenate([np.random.default_rng(3).normal(0, 1.2, 2000), [np.nan, np.inf, -np.inf, 0.0]])
    for qc, scale in ((8, 2.0), (5, 1.0), (2, 4.0)):
        rc, q = _quantize_host(lib, y, sigma, scale, qc)
        assert rc == 0
        assert np.array_equal(q, M.quantize(y, scale, qc, sigma=sigma))
        # 2*y/sigma/sigma in that order, then one multiplication
        t = (2 * y / sigma / sigma) * scale
        assert np.array_equal(q[:2000], np.clip(np.rint(t[:2000]), -M.clamp_of(qc), M.clamp_of(qc)).astype(np.int8))


def test_quantize_host_refusals():
    _, lib = _lib()
    for scale, qc in ((0.0, 8), (-1.0, 8), (np.inf, 8), (np.nan, 8), (2.0, 1), (2.0, 9), (2.0, 0)):
        assert _quantize_host(lib, [1.0], 0.0, scale, qc)[0] == EINVAL
    assert _quantize_host(lib, [1.0], np.nan, 2.0, 8)[0] == EINVAL
    assert lib.polar_q8_quantize_host(None, 4, 0.0, 2.0, 8, None) == EINVAL
    assert lib.polar_q8_quantize_host(None, 0, 0.0, 2.0, 8, None) == 0


# ---- the model's list decoder against all 2^A words ----------------------------------------------------------------------
N_EX, A_EX = 32, 6


def _exhaustive(row, frozen, info):
    """(u_hat, PM) of rule 6 with nothing pruned, from forced-bit SC walks alone: the metric of every word, and the rank
    order of rule 5 rebuilt leaf by leaf from the words' metrics right after each information leaf"""
    words = list(itertools.product((0, 1), repeat=A_EX))
    pm, at = {}, {}
    for w in words:
        bits = np.zeros(N_EX, dtype=np.int64)
        bits[info] = w
        pm[w], at[w] = M.forced_metric(row, frozen, bits)
    rank = {(): 0}
    for k in range(A_EX):
        pre = sorted({w[:k + 1] for w in words}, key=lambda v: (at[v + (0,) * (A_EX - k - 1)][k], v[k], rank[v[:k]]))
        # the metric after information leaf k depends on the bits up to k only
        for v in pre:
            assert len({at[w][k] for w in words if w[:k + 1] == v}) == 1
        rank = {v: i for i, v in enumerate(pre)}
    best = min(words, key=lambda w: (pm[w], rank[w]))
    return best, pm


@pytest.mark.parametrize("lo,hi", [(-3, 3), (-127, 127)])
def test_model_scl_is_the_exhaustive_argmin(lo, hi):
    import polardecoding_amd as pa
    q = pa.q_sequence(N_EX)
    info = np.sort(np.asarray(q[N_EX - A_EX:]))
    frozen = np.ones(N_EX, dtype=np.uint8)
    frozen[info] = 0
    rng = np.random.default_rng([lo + 200, hi])
    ties = 0
    for row in rng.integers(lo, hi + 1, size=(200, N_EX)):
        u, pm, fl = M.decode(row, frozen, 1 << A_EX)          # 2^A <= L: nothing is ever pruned
        best, all_pm = _exhaustive(row, frozen, info)
        assert all_pm[best] == min(all_pm.values())
        assert tuple(u[info]) == best and pm == all_pm[best] and not u[frozen == 1].any()
        assert fl == 0                                         # no leaf has 2m > L
        ties += list(all_pm.values()).count(all_pm[best]) > 1
    if hi == 3:
        assert ties >= 10                                      # the small alphabet makes the tie rule decide some rows


def test_model_details():
    """-128 loads as -Cc; SC is L = 1 with metric and flags 0; the tie flag needs 2m > L and equal PM_c at L-1 | L"""
    frozen = np.ones(32, dtype=np.uint8)
    frozen[[15, 23, 27, 29, 30, 31]] = 0
    row = np.full(32, -128)
    a, b = M.decode(row, frozen, 4), M.decode(np.full(32, -127), frozen, 4)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    a, b = M.decode(np.full(32, -128), frozen, 4, qc=5), M.decode(np.full(32, -15), frozen, 4, qc=5)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    z = M.decode(np.zeros(32, dtype=np.int8), frozen, 2)
    assert not z[0].any() and z[1] == 0 and z[2] == M.FLAG_TIE    # every candidate has PM_c = 0
    u, pm, fl = M.decode(np.zeros(32, dtype=np.int8), frozen, 1, sc=True)
    assert not u.any() and pm == 0 and fl == 0
    rng = np.random.default_rng(1)
    for row in rng.integers(-40, 41, size=(20, 32)):
        u1 = M.decode(row, frozen, 1)[0]
        assert np.array_equal(u1, M.decode(row, frozen, 1, sc=True)[0])   # L = 1 makes SC's decisions
    assert M.f(np.array([-3, 3, 0, -5]), np.array([2, -7, -4, -5])).tolist() == [-2, -3, 0, 5]
    assert M.g(np.array([100, 100, -7]), np.array([100, 100, 3]), np.array([0, 1, 1]), 127).tolist() == [127, 0, 10]
    assert M.g(np.array([10]), np.array([10]), np.array([0]), 15).tolist() == [15]


# ---- polar_create and its refusals, decided before any device is touched ----------------------------------------------------
def _cfg(pa, N=64, K=32, algo=None, L=4, taps=None, dtype=Q8, bp_iters=10):
    cfg = pa.api._Cfg()
    t = np.asarray(taps if taps else [0], dtype=np.int32)
    cfg.N, cfg.K, cfg.L, cfg.algo = N, K, L, pa.ALGO_SCL if algo is None else algo
    cfg.crc_r, cfg.n_taps, cfg.crc_taps = (max(taps), len(taps), t.ctypes.data_as(C.POINTER(C.c_int))) if taps else (0, 0, None)
    cfg.bp_iters, cfg.dtype, cfg.device = bp_iters, dtype, 1 << 20   # no such device: a valid request ends in EDEVICE
    return cfg, t


def _create(pa, lib, fn="polar_create", extra=(), **kw):
    cfg, keep = _cfg(pa, **kw)
    h = C.c_void_p()
    rc = getattr(lib, fn)(C.byref(cfg), *extra, C.byref(h))
    assert not h.value or rc == 0
    if h.value:
        lib.polar_destroy(h)
    return rc


def test_create_q8_and_refusals():
    pa, lib = _lib()
    assert pa.Q8 == Q8
    for algo, taps, L in ((pa.ALGO_SC, None, 1), (pa.ALGO_SCL, None, 1), (pa.ALGO_SCL, None, 32), (pa.ALGO_CASCL, CRC6, 8)):
        for N in (32, 64, 1024):
            assert _create(pa, lib, N=N, K=N // 2, algo=algo, taps=taps, L=L) == EDEVICE   # valid: only the device is missing
    assert _create(pa, lib, N=2048, K=1024) == ENOKERNEL
    assert _create(pa, lib, N=4096, K=1024, algo=pa.ALGO_SC) == ENOKERNEL
    assert _create(pa, lib, algo=pa.ALGO_BP) == ENOKERNEL
    assert _create(pa, lib, algo=pa.ALGO_SCF, taps=CRC6) == ENOKERNEL
    assert _create(pa, lib, algo=pa.ALGO_SCAN) == ENOKERNEL
    assert _create(pa, lib, L=3) == EINVAL and _create(pa, lib, L=64) == EINVAL and _create(pa, lib, N=48) == EINVAL
    assert _create(pa, lib, dtype=3) == EINVAL                # no fourth dtype
    # the float dtypes keep their answers
    assert _create(pa, lib, N=2048, K=1024, dtype=pa.F32) == EDEVICE
    assert _create(pa, lib, algo=pa.ALGO_BP, dtype=pa.F64) == EDEVICE


def test_create_rm_dyn_group_refuse_q8():
    pa, lib = _lib()
    assert _create(pa, lib, fn="polar_create_rm", extra=(60, 0)) == EINVAL
    assert _create(pa, lib, fn="polar_create_rm", extra=(60, 0), dtype=pa.F32) == EDEVICE
    pos, ptr, idx = (np.asarray(a, dtype=np.int32) for a in ((0, 1), (0, 0, 1), (0,)))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    d = pa.api._Dyn(2, ip(pos), ip(ptr), ip(idx))
    assert _create(pa, lib, fn="polar_create_dyn", extra=(C.byref(d),)) == EINVAL
    assert _create(pa, lib, fn="polar_create_dyn", extra=(C.byref(d),), dtype=pa.F64) == EDEVICE
    cfg, keep = _cfg(pa)
    h = C.c_void_p()
    assert lib.polar_group_create(C.byref(cfg), 1, C.byref(h)) == EINVAL and not h.value
    blk, bits, sec = C.c_ulonglong(0), C.c_ulonglong(0), C.c_double(0)
    assert lib.polar_fer_multi_gpu(C.byref(cfg), 1, 1, 0, 2.0, 64, C.byref(blk), C.byref(bits), C.byref(sec)) == EINVAL


def test_q8_calls_refuse_a_null_ctx():
    _, lib = _lib()
    for name in ("polar_q8_set_quant", "polar_q8_get_quant", "polar_q8_quantize_device", "polar_q8_decode_device",
                 "polar_q8_decode_batch"):
        getattr(lib, name).restype = C.c_int
    assert lib.polar_q8_set_quant(None, C.c_double(2.0), 8, 8) == EINVAL
    assert lib.polar_q8_get_quant(None, None, None, None) == EINVAL
    assert lib.polar_q8_quantize_device(None, None, 0, C.c_double(0.0), C.c_size_t(0), None) == EINVAL
    assert lib.polar_q8_decode_device(None, None, C.c_size_t(0), None, None, None) == EINVAL
    assert lib.polar_q8_decode_batch(None, None, C.c_size_t(0), None, None, None) == EINVAL


def test_q8_abi_is_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    names = ("polar_q8_set_quant", "polar_q8_get_quant", "polar_q8_quantize_host", "polar_q8_quantize_device",
             "polar_q8_decode_device", "polar_q8_decode_batch")
    assert re.search(r"#define\s+POLAR_Q8\s+2\b", hdr)
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    for tag in ("libpolar_hip.so", "libpolar_hip_testing.so"):
        lib = os.path.join(REPO, "polardecoding_amd", "lib", tag)
        assert os.path.exists(lib), "build the library first (__graft_entry__.build())"
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in names:
            assert re.search(r"\b" + name + r"\b", out), (tag, name)
    import polardecoding_amd as pa
    for f in ("set_quant", "quantize", "quantize_device", "decode_q8_device", "decode_q8_batch"):
        assert callable(getattr(pa.Decoder, f)), f
    assert isinstance(pa.Decoder.quant, property)
