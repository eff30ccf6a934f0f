"""GPU: dynamic frozen bits (k_scl_dyn, k_generate_dyn) against the numpy model of tests/test_dyn_host.py.

Per frame: u_hat bit for bit, the metric by ==, the flags word equal, in f64 and in f32, at the smallest shapes where each
mechanism first appears (N = 32: the history is one register; 64: first multi-word history and mask; 128: the working PAC
size; 1024 with L = 32 in f64: the global-scratch variant; 1024 with L = 1: more lanes than words).  The work queue needs
more frames than resident workgroups (N = 1024, L = 16, f64: one per CU): that launch is held to launches too small to queue,
and both to the model on every frame, on Gaussian rows and on a grid where nearly every frame ties.
Then the input forms, the generator, polar_fer_batch, the PAC round trip, the stop rule, graph capture and the refusals."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_dyn_host as M  # noqa: E402

F64, F32 = 0, 1


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


def _code(kind, N, arg):
    """(info_order, dyn, crc taps or None, algo) of a test code"""
    import polardecoding_amd as pa
    if kind == "pac":                                   # PAC(N, N/2), g = 0o133, rm profile
        io = pa.pac_info_order(N, N // 2, "rm")
        return io, pa.dyn_pac(N, io, M.G133), None, pa.ALGO_SCL
    if kind == "pc":                                    # PC-CA-polar (N, K + r = arg[0]), CRC-6, n_pc = 3, n_pc_wm = arg[1]
        q = pa.q_sequence(N)
        pos, sets, io = pa.dyn_pc5g(N, q[N - (arg[0] + 3):], 3, arg[1])
        return io, (pos, sets), M.CRC6, pa.ALGO_CASCL
    q = pa.q_sequence(N)
    if kind == "random":                                # random frozen subset, random sparse sets with chains
        io = np.asarray(q[N // 2:], dtype=np.int32)
        return io, M.random_dyn(N, _frozen(N, io), arg), (M.CRC6 if arg % 2 else None), (pa.ALGO_CASCL if arg % 2 else pa.ALGO_SCL)
    raise ValueError(kind)


# (kind, N, arg, L, dtype, B, seed)
CASES = [
    ("pac", 32, None, 2, F64, 1, 11), ("pac", 32, None, 2, F32, 65, 12), ("pac", 32, None, 32, F64, 300, 13),
    ("pac", 32, None, 1, F64, 65, 14),
    ("pac", 64, None, 8, F64, 300, 21), ("pac", 64, None, 8, F32, 65, 22), ("pac", 64, None, 1, F32, 300, 23),
    ("pac", 128, None, 32, F64, 65, 31), ("pac", 128, None, 32, F32, 300, 32), ("pac", 128, None, 2, F64, 300, 33),
    ("pac", 1024, None, 32, F64, 65, 41), ("pac", 1024, None, 1, F64, 65, 43),
    ("pac", 1024, None, 8, F32, 65, 44),
    ("pc", 64, (20, 0), 8, F64, 300, 51), ("pc", 64, (20, 1), 8, F32, 65, 52), ("pc", 64, (20, 1), 2, F64, 65, 53),
    ("pc", 256, (18, 0), 8, F32, 65, 54), ("pc", 256, (18, 1), 8, F64, 300, 55), ("pc", 256, (18, 0), 32, F64, 65, 56),
    ("random", 64, 3, 8, F64, 300, 61), ("random", 64, 4, 32, F32, 65, 62), ("random", 128, 5, 2, F32, 300, 63),
    ("random", 128, 6, 8, F64, 65, 64), ("random", 32, 7, 1, F64, 65, 65),
]
# every case must hold frames with decision errors: Eb/N0 as if the rate were 1/2 (sigma = 10^(-dB/20)), lower for the
# low-rate PC codes
CASE_DBS = (0.0, 1.0, 1.5, 2.0)
PC_DBS = {64: (-5.0, -4.0, -3.0, -2.0), 256: (-9.0, -8.0, -7.0, -6.0)}


def case_inputs(case):
    """(info_order, dyn, taps, algo, u [B][N], llr [B][N] f64, model outputs (u_hat, pm, flags)) -- also run on the CPU when
    the seeds were chosen: the model reports a median tie on no frame of any case (tests/test_gpu_dyn_families.py has the ties)"""
    import polardecoding_amd as pa
    kind, N, arg, L, dtype, B, seed = case
    io, dyn, taps, algo = _code(kind, N, arg)
    if L == 1 and taps is None:
        algo = pa.ALGO_SC
    u, llr = M.make_frames(N, io, dyn, B, seed, dbs=PC_DBS[N] if kind == "pc" else CASE_DBS, crc=taps)
    if dtype == F32:
        llr = llr.astype(np.float32).astype(np.float64)      # the f32 decoder reads exactly these values
    want = M.dscl_model(_frozen(N, io), dyn, llr, L, crc=(io, taps) if taps else None,
                        dtype=np.float32 if dtype == F32 else np.float64, sc=(algo == pa.ALGO_SC))
    return io, dyn, taps, algo, u, llr, want


def _decoder(case, io, dyn, taps, algo, **kw):
    import polardecoding_amd as pa
    _, N, _, L, dtype, _, _ = case
    K = len(io) - (max(taps) if taps else 0)
    return pa.Decoder(N, K, algo, L=L, crc_taps=taps, dtype=dtype, info_order=io, dyn=dyn, **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[1]}-{c[2]}-L{c[3]}-{'f32' if c[4] else 'f64'}-B{c[5]}")
def test_decisions_metrics_flags_equal_the_model(case):
    import torch
    kind, N, arg, L, dtype, B, seed = case
    io, dyn, taps, algo, u, llr, (w_u, w_pm, w_fl) = case_inputs(case)
    dec = _decoder(case, io, dyn, taps, algo)
    assert "k_scl_dyn<" in dec.kernel_name and np.array_equal(dec.dyn_positions, dyn[0])
    d_in = _cuda(llr.astype(np.float32) if dtype == F32 else llr)
    pm = torch.zeros(B, dtype=torch.float64, device="cuda")
    fl = torch.zeros(B, dtype=torch.int32, device="cuda")
    bits = dec.decode_device(d_in, pm=pm, flags=fl)
    dec.synchronize()
    g_u, g_pm, g_fl = _unpack(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)
    dec.close()
    assert np.array_equal(g_u, w_u)                     # every frame, a median tie or not
    assert np.array_equal(g_pm, w_pm)
    assert np.array_equal(g_fl, w_fl)
    # the case shows something: dynamic bits equal to 1 in the outputs, and (beyond a single frame) decision errors
    assert g_u[:, dyn[0]].any()
    if B > 1:
        assert (g_u != u).any(axis=1).any()


@pytest.mark.parametrize("algo_name,taps", [("SC", None), ("SCL", None), ("CASCL", M.CRC6)])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_empty_sets_are_the_plain_decoder_and_the_oracle(algo_name, taps, dtype, oracle):
    import polardecoding_amd as pa
    N, K, L = 128, 64, 1 if algo_name == "SC" else 8
    code = oracle.Code(N, K - (6 if taps else 0), taps)
    llr = M._oracle_frames(oracle, code, 30, 900)
    if dtype == F32:
        llr = llr.astype(np.float32).astype(np.float64)
    ref, ref_pm, ties = oracle.decode(code, llr, algo_name, L=L, dtype="f32" if dtype == F32 else "f64")
    keep = ties == 0
    assert keep.sum() >= 100
    fz = np.flatnonzero(code.frozen).astype(np.int32)
    algo = {"SC": pa.ALGO_SC, "SCL": pa.ALGO_SCL, "CASCL": pa.ALGO_CASCL}[algo_name]
    plain = pa.Decoder(N, code.K, algo, L=L, crc_taps=taps, dtype=dtype)
    want = plain.decode_batch(llr)
    for dyn in (((), ()), (fz[1::2], [np.zeros(0, dtype=np.int32)] * len(fz[1::2]))):
        dec = pa.Decoder(N, code.K, algo, L=L, crc_taps=taps, dtype=dtype, dyn=dyn)
        assert "k_scl_dyn<" in dec.kernel_name
        got = dec.decode_batch(llr)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)             # identity with the plain context, ties included
        assert np.array_equal(got[0][keep], ref[keep])
        assert np.array_equal(got[1][keep], ref_pm[keep].astype(np.float64))
        dec.close()
    plain.close()
    assert (ref != 0).any()


def test_work_queue_launch_equals_small_launches():
    """N = 1024, L = 16, f64 keeps one workgroup per CU resident, so B = 600 frames are handed out by the work queue; the
    same frames in launches of 100 are taken by index alone.  Both are held to the model on all 600 frames (bits, metric,
    flags; the model takes a few seconds for them), once on Gaussian rows and once on the (0.5, 15) grid of
    tests/llr_families.py, where nearly every frame has a median tie (582 of 600 with the model), so that refills are in
    flight while the queue hands out frames."""
    import torch
    import llr_families as F
    case = ("pac", 1024, None, 16, F64, 12, 42)
    io, dyn, taps, algo, u, llr, _ = case_inputs(case)
    B = 600
    _, more = M.make_frames(1024, io, dyn, B - 12, 43, dbs=CASE_DBS)
    gauss = np.concatenate([llr, more])
    dec = _decoder(case, io, dyn, taps, algo)
    for rows, min_ties in ((gauss, 0), (F.grid(gauss, 0.5, 15), 500)):
        w_u, w_pm, w_fl = M.dscl_model(_frozen(1024, io), dyn, rows, 16)
        assert ((w_fl & M.FLAG_TIE) != 0).sum() >= min_ties
        d_in = _cuda(rows)
        outs = []
        for chunks in ((B,), (100,) * 6):
            bits = torch.zeros((B, 32), dtype=torch.int32, device="cuda")
            pm = torch.zeros(B, dtype=torch.float64, device="cuda")
            fl = torch.zeros(B, dtype=torch.int32, device="cuda")
            o = 0
            for nb in chunks:
                dec.decode_device(d_in[o:o + nb], out_bits=bits[o:o + nb], pm=pm[o:o + nb], flags=fl[o:o + nb])
                o += nb
            dec.synchronize()
            outs.append((bits.cpu().numpy(), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)))
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
        assert np.array_equal(_unpack(outs[0][0], 1024), w_u)
        assert np.array_equal(outs[0][1], w_pm) and np.array_equal(outs[0][2], w_fl)
        assert outs[0][0].any(axis=1).all()             # no frame was left undecoded
    dec.close()


PAC64 = ("pac", 64, None, 8, F64, 65, 71)


def test_input_forms():
    """f32 input on an f64 ctx; y with sigma; polar_decode and polar_decode_batch(_y); a frozen_mask override is refused"""
    import polardecoding_amd as pa
    io, dyn, taps, algo, u, llr, _ = case_inputs(PAC64)
    N, L, B = 64, 8, 65
    fz = _frozen(N, io)
    dec = _decoder(PAC64, io, dyn, taps, algo)
    l32 = llr.astype(np.float32)
    w_u, w_pm, w_fl = M.dscl_model(fz, dyn, l32.astype(np.float64), L)
    assert not (w_fl & M.FLAG_TIE).any()
    bits = dec.decode_device(_cuda(l32))
    dec.synchronize()
    assert np.array_equal(_unpack(bits.cpu().numpy(), N), w_u)
    # y with sigma: llr = 2 * y / sigma / sigma, formed in the kernel
    sigma = 0.8
    y = np.random.default_rng(5).standard_normal((B, N)) * sigma + (1.0 - 2.0 * M.encode(u))
    w2 = M.dscl_model(fz, dyn, 2 * y / sigma / sigma, L)
    assert not (w2[2] & M.FLAG_TIE).any()
    got = dec.decode_batch_y(y, sigma)
    for g, w in zip(got, w2):
        assert np.array_equal(g, w)
    assert np.array_equal(dec(y[3], sigma), w2[0][3])
    got = dec.decode_batch(2 * y / sigma / sigma)
    for g, w in zip(got, w2):
        assert np.array_equal(g, w)
    with pytest.raises(pa.PolarError):
        dec.decode_batch(llr, frozen_mask=fz)
    dec.close()


@pytest.mark.parametrize("case,snr", [(("pac", 128, None, 8, F64, 300, 81), 1.5), (("pc", 64, (20, 1), 8, F32, 300, 82), -3.0),
                                      (("random", 1024, 9, 2, F32, 65, 83), 1.5)], ids=["pac128", "pc64", "random1024"])
def test_generator_and_fer_batch(case, snr):
    """every generated u row satisfies every constraint; the information bits are the plain context's for the same seed;
    polar_fer_batch's counters equal generate -> decode -> count run by hand"""
    import torch
    import polardecoding_amd as pa
    kind, N, arg, L, dtype, B, seed = case
    io, dyn, taps, algo = _code(kind, N, arg)
    dec = _decoder(case, io, dyn, taps, algo)
    K = len(io) - (max(taps) if taps else 0)
    plain = pa.Decoder(N, K, algo, L=L, crc_taps=taps, dtype=dtype, info_order=io)
    tdt = torch.float32 if dtype == F32 else torch.float64
    out = torch.empty((B, N), dtype=tdt, device="cuda")
    ub = torch.zeros((B, N // 32), dtype=torch.int32, device="cuda")
    out_p, ub_p = torch.empty_like(out), torch.zeros_like(ub)
    dec.generate_device(seed, 1000, snr, out, ub)
    plain.generate_device(seed, 1000, snr, out_p, ub_p)
    dec.synchronize()
    plain.synchronize()
    u, up = _unpack(ub.cpu().numpy(), N), _unpack(ub_p.cpu().numpy(), N)
    assert np.array_equal(u[:, io], up[:, io]) and u[:, io].any()
    pos, sets = dyn
    assert u[:, pos].any()
    want = M.fill_dynamic(np.where(np.isin(np.arange(N), io), u, 0).astype(np.int64), dyn)
    assert np.array_equal(u, want)                     # every constraint holds, plain frozen positions are 0
    # the noise is the plain context's: the rows differ exactly by the sign flips of the codeword bits
    x, xp = M.encode(u), M.encode(up)
    sig = 10.0 ** (-snr / 20.0)
    diff = out.cpu().numpy().astype(np.float64) - out_p.cpu().numpy().astype(np.float64)
    assert np.allclose(diff, (xp.astype(np.float64) - x) * 2.0 * 2.0 / sig / sig, rtol=1e-5, atol=1e-4)
    # fer_batch == generate -> decode -> count
    bits = dec.decode_device(out)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    dec.count_errors_device(bits, ub, cnt)
    dec.synchronize()
    hand = tuple(int(v) for v in cnt.cpu().numpy())
    assert dec.fer_batch(seed, 1000, snr, B) == hand
    uh = _unpack(bits.cpu().numpy(), N)
    assert hand == (int((uh[:, io] != u[:, io]).any(axis=1).sum()), int((uh[:, io] != u[:, io]).sum()))
    assert hand[0] > 0
    dec.close()
    plain.close()


def test_pac_round_trip():
    """pac_unprecode of decoded noiseless frames returns the payload"""
    import polardecoding_amd as pa
    N, K = 128, 64
    for L in (1, 32):
        dec = pa.PAC(N, K, L=L)
        io = dec.info_order
        rng = np.random.default_rng(L)
        v = np.zeros((40, N), dtype=np.int32)
        v[:, io] = rng.integers(0, 2, (40, K))
        u = pa.pac_precode(v)
        assert u[:, dec.dyn_positions].any()
        uh, _, _ = dec.decode_batch(6.0 * (1.0 - 2.0 * M.encode(u)))
        assert np.array_equal(uh, u)
        assert np.array_equal(pa.pac_unprecode(uh)[:, io], v[:, io])
        dec.close()
    dec = pa.PCCASCL(64, 14, n_pc=3, n_pc_wm=1, L=8)
    assert dec.A == 20 and len(dec.dyn_positions) == 3
    dec.close()


def test_stop_rule_agrees_with_a_loop_over_the_models_decisions():
    io, dyn, taps, algo, u, llr, _ = case_inputs(PAC64)
    N, L, B = 64, 8, 65
    sigma = 10.0 ** (-1.0 / 20.0)
    y = np.random.default_rng(17).standard_normal((B, N)) * sigma + (1.0 - 2.0 * M.encode(u))
    w_u, _, w_fl = M.dscl_model(_frozen(N, io), dyn, 2 * y / sigma / sigma, L)
    assert not (w_fl & M.FLAG_TIE).any()
    err = (w_u[:, io] != u[:, io]).sum(axis=1)
    assert (err > 0).sum() >= 3
    dec = _decoder(PAC64, io, dyn, taps, algo)
    for need, min_frames in ((1, 0), (3, 0), (10 ** 6, 0), (1, 40)):
        used = blk = bits = 0
        for f in range(B):                               # main()'s loop: stop WITH the frame that reaches `need`
            used += 1
            blk += int(err[f] > 0)
            bits += int(err[f])
            if blk >= need and used >= min_frames:
                break
        assert dec.stop_rule_batch_y(y, sigma, u, need, min_frames) == (used, blk, bits)
    dec.close()


def test_graph_capture():
    import torch
    case = ("pac", 128, None, 8, F32, 300, 91)
    io, dyn, taps, algo, u, llr, (w_u, w_pm, w_fl) = case_inputs(case)
    assert not (w_fl & M.FLAG_TIE).any()
    dec = _decoder(case, io, dyn, taps, algo)
    d_in = _cuda(llr.astype(np.float32))
    bits = torch.zeros((300, 4), dtype=torch.int32, device="cuda")
    pm = torch.zeros(300, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dec.use_torch_stream()
        dec.decode_device(d_in, out_bits=bits, pm=pm)    # warm-up at the same B
        stream.synchronize()
        bits.zero_()
        pm.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            dec.use_torch_stream()
            dec.decode_device(d_in, out_bits=bits, pm=pm)
        bits.zero_()
        for _ in range(2):
            g.replay()
        stream.synchronize()
    assert np.array_equal(_unpack(bits.cpu().numpy(), 128), w_u)
    assert np.array_equal(pm.cpu().numpy(), w_pm)
    del g
    dec.close()


def test_refusals_on_the_device():
    import ctypes as C
    import torch
    import polardecoding_amd as pa
    io, dyn, taps, algo = _code("pc", 64, (20, 0))
    dec = pa.PCCASCL(64, 14, L=8)
    assert dec.algo == pa.ALGO_CASCL and "k_scl_dyn<double,L=8>" in dec.kernel_name
    assert np.array_equal(dec.dyn_positions, dyn[0]) and np.array_equal(dec.info_order, io)
    llr = np.ones((2, 64))
    with pytest.raises(pa.PolarError):
        dec.set_cascl_stages((1, 8))
    with pytest.raises(pa.PolarError):
        dec.decode_cascl_batch(llr)
    with pytest.raises(pa.PolarError):
        dec.decode_cascl_device(_cuda(llr))
    for fn in (dec.set_scf_flips, dec.set_scan_iters):
        with pytest.raises(pa.PolarError):
            fn(2)
    with pytest.raises(pa.PolarError):
        dec.set_bp_stop("g")
    for fn in (dec.decode_bp_batch, dec.decode_scf_batch, dec.decode_scan_batch):
        with pytest.raises(pa.PolarError):
            fn(llr)
    # the context is still usable, and a plain context reports no dynamic positions
    uh, _, _ = dec.decode_batch(llr)
    assert uh.shape == (2, 64)
    dec.close()
    plain = pa.SCLdecode(64, 32, L=2)
    assert plain.dyn_positions is None and "dyn" not in plain.kernel_name
    plain.close()
    with pytest.raises(pa.PolarError):
        pa.Decoder(2048, 1024, pa.ALGO_SCL, L=2, dyn=((0,), [[]]))       # POLAR_ENOKERNEL
    with pytest.raises(pa.PolarError):
        pa.Decoder(64, 32, pa.ALGO_BP, dyn=((0,), [[]]))
    with pytest.raises(pa.PolarError):
        pa.Decoder(64, 32, pa.ALGO_SCL, L=2, dyn=((63,), [[]]))          # unfrozen under the cfg
    # the genie calls work on any ctx
    d = pa.PAC(64, 32, L=2)
    cnt = torch.zeros((2, 64), dtype=torch.int64, device="cuda")
    d.construct_batch(1, 0, 0.8, 64, cnt)
    d.synchronize()
    assert int(cnt.sum()) > 0
    d.close()
