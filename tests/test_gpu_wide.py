"""GPU: wide lists, L = 64 / 128 / 256 (k_scl_wide, csrc/scl_wide.h), against the numpy model of tests/test_dyn_host.py and,
where it reaches (L = 64), against the CPU oracle.

Every comparison is by ==: u_hat bit for bit, the metric, the flags word.  The shapes are the smallest at which each
mechanism first exists: N = 32 (the whole history in registers, one wavefront), a list that never fills, L = 128 (the first
ranking, refill and exchange across wavefronts, history words in LDS), L = 256 in f32 (levels in LDS), in f64 and under the
test library's spill switch (levels in global scratch), the CRC mask on the final choice, the three shapes that fill the
64-bit pointer table (60, 63 and 64 bits), the work queue, the input forms, the FER gain over L = 32 and the refusal of
adaptive stages.  Model cost at N = 128 is 12 / 28 / 74 ms per frame for L = 64 / 128 / 256, hence the batch sizes.

The tied rows here are at N = 32, L = 64 (one wavefront); the rows at L = 128 and 256 are Gaussian and tie in no frame.  Ties,
un-refilled dead slots and refills across wavefronts at L = 128 and 256 are in tests/test_gpu_wide_families.py."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_dyn_host as M  # noqa: E402
import llr_families as F  # noqa: E402

F64, F32 = 0, 1
CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _frozen(N, info):
    f = np.ones(N, dtype=np.uint8)
    f[np.asarray(info)] = 0
    return f


def _info(N, A):
    import polardecoding_amd as pa
    return np.asarray(pa.q_sequence(N)[N - A:], dtype=np.int32)


def _run(dec, rows, dtype, N):
    """decode_device with metric and flags -> (u_hat, pm, flags)"""
    import torch
    B = len(rows)
    pm = torch.zeros(B, dtype=torch.float64, device="cuda")
    fl = torch.zeros(B, dtype=torch.int32, device="cuda")
    bits = dec.decode_device(_cuda(rows.astype(np.float32) if dtype == F32 else rows), pm=pm, flags=fl)
    dec.synchronize()
    return _unpack(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


def _same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def _np_dtype(dtype):
    return np.float32 if dtype == F32 else np.float64


def _rows_for(dtype, llr):
    return llr.astype(np.float32).astype(np.float64) if dtype == F32 else llr   # the f32 decoder reads exactly these values


# ---- 1, 2: N = 32, one wavefront, the whole history in registers ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _n32(K, dtype):
    io = _info(32, K)
    u, llr = M.make_frames(32, io, None, 64, 100 + K, dbs=(1.5,))
    rows = {"awgn": _rows_for(dtype, llr), "grid": F.grid(llr, *F.GRIDS[0])}   # the grid is exact in f32
    want = {k: M.dscl_model(_frozen(32, io), None, v, 64, dtype=_np_dtype(dtype)) for k, v in rows.items()}
    return io, u, rows, want


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_n32_l64_plain_scl_with_ties(dtype):
    import polardecoding_amd as pa
    io, u, rows, want = _n32(16, dtype)
    assert (want["grid"][2] & M.FLAG_TIE).any() and not (want["grid"][2] & M.FLAG_TIE).all()   # the tie rule and the flag run
    dec = pa.SCLdecode(32, 16, L=64, dtype=dtype)
    assert dec.kernel_name.startswith("k_scl_wide<") and dec.L == 64
    for k in rows:
        _same(_run(dec, rows[k], dtype, 32), want[k])
    dec.close()
    assert (want["awgn"][0] != u).any()


def test_n32_k5_the_list_never_fills():
    """five information leaves: 32 live slots of 64, the choice runs over the live ones only"""
    import polardecoding_amd as pa
    io, u, rows, want = _n32(5, F64)
    dec = pa.SCLdecode(32, 5, L=64)
    assert dec.kernel_name.startswith("k_scl_wide<")
    for k in rows:
        got = _run(dec, rows[k], F64, 32)
        _same(got, want[k])
        assert not got[2].any()                          # no ranking, no tie flag
    dec.close()


# ---- 3: two wavefronts, random dynamic constraints --------------------------------------------------------------------
def test_n64_l128_random_dynamic_constraints():
    import polardecoding_amd as pa
    N, K, L, B = 64, 32, 128, 48
    io = _info(N, K)
    dyn = M.random_dyn(N, _frozen(N, io), 3)
    u, llr = M.make_frames(N, io, dyn, B, 301, dbs=(0.0, 1.0, 1.5, 2.0))
    want = M.dscl_model(_frozen(N, io), dyn, llr, L)
    dec = pa.Decoder(N, K, pa.ALGO_SCL, L=L, info_order=io, dyn=dyn)
    assert dec.kernel_name.startswith("k_scl_wide<double,L=128>") and "dynamic" in dec.kernel_name
    got = _run(dec, llr, F64, N)
    dec.close()
    _same(got, want)
    assert got[0][:, dyn[0]].any() and (got[0] != u).any()


# ---- 4: four wavefronts, PAC(128, 64) ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pac128(dtype, L=256, B=24):
    import polardecoding_amd as pa
    io = pa.pac_info_order(128, 64, "rm")
    dyn = pa.dyn_pac(128, io, M.G133)
    u, llr = M.make_frames(128, io, dyn, B, 401, dbs=(0.0, 1.0, 1.5, 2.0))
    llr = _rows_for(dtype, llr)
    return u, llr, M.dscl_model(_frozen(128, io), dyn, llr, L, dtype=_np_dtype(dtype))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32-lds", "f64-global"])
def test_pac128_l256(dtype):
    import polardecoding_amd as pa
    u, llr, want = _pac128(dtype)
    dec = pa.PAC(128, 64, L=256, dtype=dtype)
    assert dec.kernel_name.startswith("k_scl_wide<") and dec.L == 256
    got = _run(dec, llr, dtype, 128)
    pos = dec.dyn_positions
    dec.close()
    _same(got, want)
    assert got[0][:, pos].any()


def test_pac128_l256_f32_levels_forced_to_global_scratch():
    import polardecoding_amd as pa
    from polardecoding_amd import testing
    u, llr, want = _pac128(F32)
    dec = testing.select_kernel(pa.PAC(128, 64, L=256, dtype=F32), testing.KERNEL_GENERIC_SPILL)
    assert dec.kernel_name.startswith("k_scl_wide<")
    got = _run(dec, llr, F32, 128)
    dec.close()
    _same(got, want)


# ---- 5, 6: CA-SCL at L = 64 against the oracle -------------------------------------------------------------------------
def _oracle_case(oracle, N, K, taps, B, seed, dbs):
    code = oracle.Code(N, K, taps)
    per = B // len(dbs)
    llr = np.concatenate([F.oracle_llr(oracle, code, per, seed + i, db) for i, db in enumerate(dbs)])
    ref, ref_pm, ties = oracle.decode(code, llr, "CASCL", L=64)
    return code, llr, ref, ref_pm, ties == 0


def test_cascl128_l64_against_the_oracle(oracle):
    """CRC-6: the pass mask on the final choice; the batch at 0 dB holds frames where no path passes"""
    import polardecoding_amd as pa
    N, K, B = 128, 58, 64
    code, llr, ref, ref_pm, keep = _oracle_case(oracle, N, K, M.CRC6, B, 500, (1.5, 0.0))
    assert keep.sum() >= B * 3 // 4
    dec = pa.CASCL(N, K, L=64, crc_taps=M.CRC6)
    assert dec.kernel_name.startswith("k_scl_wide<double,L=64>")
    u, pm, fl = _run(dec, llr, F64, N)
    assert np.array_equal(u[keep], ref[keep])
    assert np.array_equal(pm[keep], ref_pm[keep])
    assert not (fl[keep] & M.FLAG_TIE).any()
    passed = (fl & M.FLAG_CRC_PASS) != 0
    assert passed.any() and not passed.all()
    # polar_cascl_decode_device reports the list size; every frame equals the model too, ties included
    import torch
    ls = torch.zeros(B, dtype=torch.int32, device="cuda")
    bits = dec.decode_cascl_device(_cuda(llr), list_size=ls)
    dec.synchronize()
    assert np.array_equal(_unpack(bits.cpu().numpy(), N), u) and (ls.cpu().numpy() == 64).all()
    dec.close()
    _same((u, pm, fl), M.dscl_model(code.frozen, None, llr, 64, crc=(code.info_order, M.CRC6), oracle=oracle))


def test_n1024_l64_crc24c_against_the_oracle(oracle):
    """log2 L * log2 N = 60 bits of pointer table; the levels live in global scratch"""
    import polardecoding_amd as pa
    N, K, B = 1024, 512, 8
    code, llr, ref, ref_pm, keep = _oracle_case(oracle, N, K, CRC24C, B, 600, (1.5, 1.0))
    assert keep.sum() >= B * 3 // 4
    dec = pa.CASCL(N, K, L=64, crc_taps=CRC24C)
    assert dec.kernel_name.startswith("k_scl_wide<")
    u, pm, fl = _run(dec, llr, F64, N)
    dec.close()
    assert np.array_equal(u[keep], ref[keep])
    assert np.array_equal(pm[keep], ref_pm[keep])
    assert ref[keep].any()


# ---- 7, 8: the pointer table at 63 and 64 bits --------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,dtype", [(512, 128, F32), (256, 256, F64)], ids=["N512-L128-63bits", "N256-L256-64bits"])
def test_full_pointer_table(N, L, dtype):
    import polardecoding_amd as pa
    B = 4
    io = _info(N, N // 2)
    u, llr = M.make_frames(N, io, None, B, 700 + N, dbs=(1.0, 1.5))
    llr = _rows_for(dtype, llr)
    want = M.dscl_model(_frozen(N, io), None, llr, L, dtype=_np_dtype(dtype))
    dec = pa.SCLdecode(N, N // 2, L=L, dtype=dtype)
    assert dec.kernel_name.startswith("k_scl_wide<")
    got = _run(dec, llr, dtype, N)
    dec.close()
    _same(got, want)
    assert got[0].any()


# ---- 9: the work queue ----------------------------------------------------------------------------------------------------
def test_work_queue_launch_equals_small_launches():
    """8192 frames in one launch (more than the resident workgroups) against the same rows in launches of 64, three times
    over (every launch leaves the counter at zero); the first 64 against the model"""
    import torch
    import polardecoding_amd as pa
    io, u, rows, want = _n32(16, F64)
    B = 8192
    rng = np.random.default_rng(9)
    llr = np.concatenate([rows["awgn"], 2.0 * rng.standard_normal((B - 64, 32)) + 1.0])
    dec = pa.SCLdecode(32, 16, L=64)
    assert dec.kernel_name.startswith("k_scl_wide<")
    d_in = _cuda(llr)

    def run(chunk):
        bits = torch.full((B, 1), -1, dtype=torch.int32, device="cuda")
        pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
        fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        for o in range(0, B, chunk):
            dec.decode_device(d_in[o:o + chunk], out_bits=bits[o:o + chunk], pm=pm[o:o + chunk], flags=fl[o:o + chunk])
        dec.synchronize()
        return bits.cpu().numpy(), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)

    small = run(64)
    for rep in range(3):
        _same(run(B), small)
    dec.close()
    assert (small[1] >= 0).all() and (small[2] <= 3).all()              # every frame was written
    _same((_unpack(small[0][:64], 32), small[1][:64], small[2][:64]), want["awgn"])


# ---- 10, 11, 12: input forms -----------------------------------------------------------------------------------------------
def test_input_forms():
    """an f64 ctx given y and sigma, given f32 rows, and through the host buffers of decode_batch / decode_batch_y / decode"""
    import polardecoding_amd as pa
    N, K, L, B = 32, 16, 64, 64
    io, u, rows, want = _n32(K, F64)
    fz = _frozen(N, io)
    dec = pa.SCLdecode(N, K, L=L)
    sigma = 0.8
    y = np.random.default_rng(5).standard_normal((B, N)) * sigma + (1.0 - 2.0 * M.encode(u))
    w_y = M.dscl_model(fz, None, 2 * y / sigma / sigma, L)
    import torch
    pm = torch.zeros(B, dtype=torch.float64, device="cuda")
    fl = torch.zeros(B, dtype=torch.int32, device="cuda")
    bits = dec.decode_device(_cuda(y), sigma=sigma, pm=pm, flags=fl)          # 10: y and sigma, formed in the kernel
    dec.synchronize()
    _same((_unpack(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)), w_y)
    l32 = rows["awgn"].astype(np.float32)                                      # 11: f32 rows into f64 arithmetic
    w32 = M.dscl_model(fz, None, l32.astype(np.float64), L)
    bits = dec.decode_device(_cuda(l32), pm=pm, flags=fl)
    dec.synchronize()
    _same((_unpack(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)), w32)
    _same(dec.decode_batch(rows["awgn"]), want["awgn"])                        # 12: host buffers
    _same(dec.decode_batch_y(y, sigma), w_y)
    assert np.array_equal(dec(y[3], sigma), w_y[0][3])
    dec.close()
    f32dec = pa.SCLdecode(N, K, L=L, dtype=F32)                                # an f32 ctx takes the host's f64 rows
    g32 = F.grid(rows["awgn"], *F.GRIDS[1])
    _same(f32dec.decode_batch(g32), M.dscl_model(fz, None, g32, L, dtype=np.float32))
    f32dec.close()


# ---- 13: what the wide list is for -----------------------------------------------------------------------------------------
def test_pac128_l128_has_fewer_block_errors_than_l32():
    """PAC(128, 64) at 1.5 dB over the same 16 384 generated frames (CPU model: 79 against 124 block errors in 2 000)"""
    import polardecoding_amd as pa
    errs = {}
    for L in (32, 128):
        dec = pa.PAC(128, 64, L=L, dtype=F32)
        errs[L] = dec.fer_batch(77, 0, 1.5, 16384)
        assert dec.kernel_name.startswith("k_scl_wide<" if L > 32 else "k_scl_dyn<")
        dec.close()
    print("block / bit errors by L:", errs)
    assert 0 < errs[128][0] < errs[32][0]


# ---- 14: refusals on the device --------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable():
    import polardecoding_amd as pa
    N, K = 128, 58
    dec = pa.CASCL(N, K, L=64, crc_taps=M.CRC6)
    for stages in ((8, 64), (1, 64), (1, 8, 32, 64)):
        with pytest.raises(pa.PolarError):
            dec.set_cascl_stages(stages)
    assert dec.kernel_name.startswith("k_scl_wide<")
    uh, pm, fl, ls = dec.decode_cascl_batch(6.0 * np.ones((3, N)))
    assert not uh.any() and (ls == 64).all() and (fl & M.FLAG_CRC_PASS).all()
    dec.close()
    with pytest.raises(pa.PolarError):
        pa.SCLdecode(64, 32, L=64, dtype=pa.Q8)
    with pytest.raises(pa.PolarError):
        pa.SCLdecode(64, 32, L=512)
    with pytest.raises(pa.PolarError):
        pa.SCLdecode(512, 256, L=256)                    # POLAR_ENOKERNEL
    with pytest.raises(pa.PolarError):
        pa.decode(np.ones(64), np.zeros(64, dtype=np.uint8), 64, 64)
