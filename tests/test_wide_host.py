"""CPU: wide lists (include/polar_hip.h, "Wide lists"): L = 64, 128, 256 for SCL / CA-SCL.

The rule of k_scl_wide is the one tests/test_dyn_host.py dscl_model states, for a larger L.  Here: that model at L = 64 against
the CPU oracle (which reaches L = 64) on decisions and metrics, and what polar_create / polar_create_dyn accept and refuse
for L > 32, with no device touched.  tests/test_gpu_wide.py holds the kernel to the model and to the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_dyn_host as M  # noqa: E402

OK, EINVAL, EDEVICE, ENOKERNEL = 0, -1, -3, -4


def awgn_llr(oracle, code, B, seed, db):
    sig = oracle.sigma_from_db(db)
    _, ys = oracle.Sim(seed).frames(code, sig, B)
    return np.stack([oracle.llr_from_y(y, sig) for y in ys])


@pytest.mark.parametrize("algo,N,K,taps", [("SCL", 128, 64, None), ("CASCL", 128, 64, M.CRC6), ("SCL", 64, 32, None)],
                         ids=["SCL128", "CASCL128", "SCL64"])
def test_model_at_L64_is_the_oracle(algo, N, K, taps, oracle):
    """48 AWGN frames at 1.5 dB; frames on which the oracle reports a median tie are left out (its tie rule is not the
    library's), at most a quarter of them"""
    B, L = 48, 64
    code = oracle.Code(N, K - (6 if taps else 0), taps)
    llr = awgn_llr(oracle, code, B, 700 + N, 1.5)
    ref, ref_pm, ties = oracle.decode(code, llr, algo, L=L)
    keep = ties == 0
    assert keep.sum() >= B * 3 // 4
    crc = (code.info_order, taps) if taps else None
    u, pm, fl = M.dscl_model(code.frozen, None, llr, L, crc=crc, oracle=oracle)
    assert np.array_equal(u[keep], ref[keep])
    assert np.array_equal(pm[keep], ref_pm[keep].astype(np.float64))
    assert not (fl[keep] & M.FLAG_TIE).any()
    assert ref[keep].any()


def _create(lib, pa, N, K, L, dtype=None, algo=None, taps=None):
    cfg = pa.api._Cfg()
    t = np.asarray(taps if taps else [0], dtype=np.int32)
    cfg.N, cfg.K, cfg.L, cfg.algo = N, K, L, pa.ALGO_SCL if algo is None else algo
    cfg.crc_r, cfg.n_taps, cfg.crc_taps = (max(taps), len(taps), t.ctypes.data_as(C.POINTER(C.c_int))) if taps else (0, 0, None)
    cfg.bp_iters, cfg.dtype, cfg.device = 10, pa.F64 if dtype is None else dtype, 1 << 20   # no such device
    h = C.c_void_p()
    rc = lib.polar_create(C.byref(cfg), C.byref(h))
    assert not h.value
    return rc


def test_create_accepts_and_refuses_without_a_device():
    import polardecoding_amd as pa
    lib = pa.load_library()
    # valid: only the device is missing
    assert _create(lib, pa, 64, 32, 64) == EDEVICE
    for N, L in ((1024, 64), (512, 128), (256, 256), (32, 256)):
        for dtype in (pa.F64, pa.F32):
            assert _create(lib, pa, N, N // 2, L, dtype=dtype) == EDEVICE, (N, L)
    assert _create(lib, pa, 128, 58, 64, algo=pa.ALGO_CASCL, taps=M.CRC6) == EDEVICE
    # no such list
    assert _create(lib, pa, 64, 32, 512) == EINVAL
    assert _create(lib, pa, 64, 32, 1024) == EINVAL
    for L in (48, 96, 100, 255):
        assert _create(lib, pa, 64, 32, L) == EINVAL, L
    # N * L > 65536: no kernel
    assert _create(lib, pa, 512, 256, 256) == ENOKERNEL
    assert _create(lib, pa, 1024, 512, 128) == ENOKERNEL
    assert _create(lib, pa, 2048, 1024, 64) == ENOKERNEL
    # fixed point stays at L <= 32
    assert _create(lib, pa, 64, 32, 64, dtype=pa.Q8) == EINVAL
    assert _create(lib, pa, 64, 32, 32, dtype=pa.Q8) == EDEVICE
    # what took L <= 32 still does
    assert _create(lib, pa, 4096, 2048, 32) == EDEVICE
    # algorithms without a list ignore L, as before
    assert _create(lib, pa, 64, 32, 512, algo=pa.ALGO_SC) == EDEVICE


def test_create_dyn_and_decode_llr():
    import polardecoding_amd as pa
    lib = pa.load_library()
    assert M._create_dyn(lib, pa, N=128, K=64, L=128) == EDEVICE
    assert M._create_dyn(lib, pa, N=256, K=128, L=256) == EDEVICE
    assert M._create_dyn(lib, pa, N=512, K=256, L=256) == ENOKERNEL
    assert M._create_dyn(lib, pa, N=128, K=64, L=512) == EINVAL
    # polar_decode_llr keeps its limit: refused before anything is read or a device is asked for
    llr = np.ones(64)
    fm = np.zeros(64, dtype=np.uint8)
    uh = np.zeros(64, dtype=np.int32)
    dp, bp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    for L in (64, 128, 256):
        assert lib.polar_decode_llr(dp(llr), bp(fm), 64, L, ip(uh)) == EINVAL


def test_header_documents_wide_lists():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "polar_hip.h")).read()
    assert "Wide lists" in hdr and "k_scl_wide" in hdr
