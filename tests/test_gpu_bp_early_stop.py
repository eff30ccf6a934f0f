"""GPU: BP early termination, stop rule G (polar_bp_set_stop; include/polar_hip.h).

Every frame's stop point and decisions against the numpy restatement of the reference's BP
(tests/test_bp_early_stop_host.py, itself checked against the oracle) and the oracle's fixed-iteration decoder, on all
three BP kernels: k_bp_w128 (N = 128), k_bp_r4 (N = 1024), k_bp (N = 512, rows in LDS; N = 2048, rows in global
scratch).  Then: f32 against the library's own fixed-iteration f32 decode, the default rule untouched, the work queue
under frames of varying length, the consumers of the rule and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bp_early_stop_host import stop_points  # noqa: E402

ITER_MAX = 40
DBS = (1.0, 1.5, 2.0, 2.5, 3.0)
# N, K, frames per Eb/N0 point, kernel the ctx must pick
SHAPES = [(128, 64, 40, "k_bp_w128<"), (1024, 512, 20, "k_bp_r4<"), (512, 256, 30, "k_bp<"), (2048, 1024, 10, "k_bp<")]


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


_CACHE = {}


def _case(N, oracle):
    """Frames over 1 to 3 dB for one block length, the decoder's frozen set, and the restatement's per-frame answers."""
    if N in _CACHE:
        return _CACHE[N]
    import polardecoding_amd as pa
    K, per = next((k, p) for n, k, p, _ in SHAPES if n == N)
    dec = pa.BP(N, K, iterMax=ITER_MAX)
    io = dec.info_order
    rest = [j for j in range(N) if j not in set(io.tolist())]
    code = oracle.Code(N, K, None, Q=rest + io.tolist())   # the decoder's information set (N > 1024: no 5G table)
    llr, ys, sigs = [], [], []
    for k, db in enumerate(DBS):
        sim = oracle.Sim(3100 + N + k)
        sig = oracle.sigma_from_db(db)
        _, y = sim.frames(code, sig, per)
        ys += list(y)
        sigs += [sig] * per
        llr += [oracle.llr_from_y(v, sig) for v in y]
    llr = np.stack(llr)
    t_stop, conv, out = stop_points(llr, code.frozen, ITER_MAX)
    c = dict(K=K, code=code, llr=llr, ys=np.stack(ys), sigs=np.array(sigs), t=t_stop, conv=conv, out=out)
    _CACHE[N] = c
    return c


def _run(dec, llr, dtype=None):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    if dtype is not None:
        d = d.to(dtype)
    B = d.shape[0]
    it = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fills are done before the ctx stream reads the buffers
    bits = dec.decode_bp_device(d, iters=it, flags=fl)
    dec.synchronize()
    return _unpack(bits.cpu().numpy(), dec.N), it.cpu().numpy().astype(np.int64), fl.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("N,K,per,kname", SHAPES)
def test_stop_points_f64(N, K, per, kname, oracle):
    """iters[b] is the first round trip at which u_hat F == x_hat (or iterMax), the flag says which, and u_hat is the
    oracle's (= the reference's BP()) with iterMax = iters[b]."""
    import polardecoding_amd as pa
    c = _case(N, oracle)
    dec = pa.BP(N, K, iterMax=ITER_MAX, early_stop="g")
    assert dec.kernel_name.startswith(kname) and "stop rule G" in dec.kernel_name
    uh, it, fl = _run(dec, c["llr"])
    assert np.array_equal(it, c["t"])
    assert np.array_equal(fl, np.where(c["conv"], pa.FLAG_BP_CONVERGED, 0))
    assert np.array_equal(uh, c["out"])
    assert c["conv"].any() and (it < ITER_MAX).any()
    for t in np.unique(it):
        sel = it == t
        ref, _, _ = oracle.decode(c["code"], c["llr"][sel], "BP", bp_iters=int(t))
        assert np.array_equal(uh[sel], ref), t


@pytest.mark.parametrize("N,K,per,kname", SHAPES[:3])
def test_stop_points_f32_equal_fixed_iteration_f32(N, K, per, kname, oracle):
    """f32: the frames that ran t round trips are bit-identical to the same library's f32 decode with bp_iters = t."""
    import torch
    import polardecoding_amd as pa
    c = _case(N, oracle)
    dec = pa.BP(N, K, iterMax=ITER_MAX, early_stop="g", dtype=pa.F32)
    uh, it, fl = _run(dec, c["llr"], torch.float32)
    assert it.min() >= 1 and it.max() <= ITER_MAX
    assert (fl[it < ITER_MAX] == pa.FLAG_BP_CONVERGED).all()   # a frame that stopped early converged
    assert (it < ITER_MAX).sum() > len(it) // 4
    x32 = torch.from_numpy(c["llr"]).cuda().float()
    for t in np.unique(it):
        sel = np.flatnonzero(it == t)
        fix = pa.BP(N, K, iterMax=int(t), dtype=pa.F32)
        xs = x32[torch.from_numpy(sel).cuda()].contiguous()
        torch.cuda.synchronize()
        bits = fix.decode_device(xs)
        fix.synchronize()
        assert np.array_equal(uh[sel], _unpack(bits.cpu().numpy(), N)), t


@pytest.mark.parametrize("N,K,per,kname", SHAPES[:3])
def test_none_rule_is_the_fixed_decoder(N, K, per, kname, oracle):
    """POLAR_BP_STOP_NONE on the new entry point: polar_decode_device's decisions, iters = iterMax, flags = 0; a ctx
    switched G -> NONE returns to the fixed result."""
    import torch
    import polardecoding_amd as pa
    c = _case(N, oracle)
    dec = pa.BP(N, K, iterMax=ITER_MAX)
    d = torch.from_numpy(c["llr"]).cuda()
    torch.cuda.synchronize()
    bits = dec.decode_device(d)
    dec.synchronize()
    ref = _unpack(bits.cpu().numpy(), N)
    uh, it, fl = _run(dec, c["llr"])
    assert np.array_equal(uh, ref)
    assert (it == ITER_MAX).all() and (fl == 0).all()
    dec.set_bp_stop("g")
    ug, _, _ = _run(dec, c["llr"])
    assert np.array_equal(ug, c["out"])
    dec.set_bp_stop(None)
    assert "stop" not in dec.kernel_name
    un, it2, fl2 = _run(dec, c["llr"])
    assert np.array_equal(un, ref) and (it2 == ITER_MAX).all() and (fl2 == 0).all()


@pytest.mark.parametrize("N", [1024, 128, 512])
def test_work_queue_with_frames_of_varying_length(N, oracle):
    """B = 1, B below the resident count, a B that is no multiple of anything, and a queued launch well above the resident
    count (the base frames tiled), twice back to back on one ctx: every frame gets its own answer, none is skipped or
    repeated."""
    import torch
    import polardecoding_amd as pa
    c = _case(N, oracle)
    dec = pa.BP(N, c["K"], iterMax=ITER_MAX, early_stop="g")
    nb = len(c["t"])
    for B in (1, 37, 1000 + 7, 20000 + 13):
        idx = (np.arange(B) * 7 + 3) % nb
        d = torch.from_numpy(c["llr"][idx]).cuda()
        outs = []
        for _ in range(2):   # two launches queued on the ctx stream before one synchronisation
            it = torch.zeros(B, dtype=torch.int32, device="cuda")
            fl = torch.zeros(B, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            outs.append((dec.decode_bp_device(d, iters=it, flags=fl), it, fl))
        dec.synchronize()
        for bits, it, fl in outs:
            assert np.array_equal(_unpack(bits.cpu().numpy(), N), c["out"][idx]), B
            assert np.array_equal(it.cpu().numpy(), c["t"][idx]), B
            assert np.array_equal(fl.cpu().numpy() != 0, c["conv"][idx]), B


def test_consumers_honour_the_rule(oracle):
    """polar_fer_batch under G = generate + polar_bp_decode_device + polar_count_errors_device on the same frames;
    polar_decode_batch_y, polar_bp_decode_batch and polar_decode (one frame) give the restatement's decisions."""
    import torch
    import polardecoding_amd as pa
    N, K = 1024, 512
    dec = pa.BP(N, K, iterMax=50, early_stop="g")
    B, seed, first, snr = 6000, 77, 1000, 2.0
    blk, bits = dec.fer_batch(seed, first, snr, B)
    llr = torch.empty((B, N), dtype=torch.float64, device="cuda")
    u = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dec.generate_device(seed, first, snr, llr, u)
    uh = dec.decode_bp_device(llr, iters=it)
    dec.count_errors_device(uh, u, cnt)
    dec.synchronize()
    assert (blk, bits) == tuple(int(x) for x in cnt.cpu().numpy())
    assert it.float().mean().item() < 45   # at 2 dB most frames stop early

    c = _case(N, oracle)
    d2 = pa.BP(N, K, iterMax=ITER_MAX, early_stop="g")
    for sig in np.unique(c["sigs"]):
        sel = c["sigs"] == sig
        uy, _, fy = d2.decode_batch_y(c["ys"][sel], sig)
        assert np.array_equal(uy, c["out"][sel])
        assert np.array_equal(fy != 0, c["conv"][sel])
    ub, ib, fb2 = d2.decode_bp_batch(c["llr"])
    assert np.array_equal(ub, c["out"]) and np.array_equal(ib, c["t"]) and np.array_equal(fb2 != 0, c["conv"])
    b = int(np.argmin(c["t"]))
    assert np.array_equal(d2(c["ys"][b], c["sigs"][b]), c["out"][b])


def test_refusals():
    import torch
    import polardecoding_amd as pa
    EINVAL = -1
    scl = pa.SCLdecode(128, 64, L=8)
    assert scl._lib.polar_bp_set_stop(scl._h, pa.BP_STOP_G) == EINVAL
    with pytest.raises(pa.PolarError):
        scl.set_bp_stop("g")
    dec = pa.BP(128, 64, iterMax=20)
    assert dec._lib.polar_bp_set_stop(dec._h, 7) == EINVAL
    with pytest.raises(ValueError):
        dec.set_bp_stop("crc")
    assert dec._lib.polar_bp_decode_device(scl._h, None, 0, 0.0, 0, None, None, None) == EINVAL
    dec.set_bp_stop("g")
    B = 4
    x = torch.zeros((B, 128), dtype=torch.float64, device="cuda")
    u = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    E = torch.zeros((1, 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cp = (C.c_int * 1)(10)
    rc = dec._lib.polar_bp_readout_device(dec._h, C.c_void_p(x.data_ptr()), 0, 0.0, B, C.c_void_p(u.data_ptr()), cp, 1,
                                          C.c_void_p(E.data_ptr()), None)
    assert rc == EINVAL
    dec.set_bp_stop(pa.BP_STOP_NONE)
    dec.bp_readout_device(x, u, [10], E)   # accepted again
    dec.synchronize()
