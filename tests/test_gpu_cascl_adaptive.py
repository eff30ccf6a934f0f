"""GPU: adaptive CA-SCL (polar_cascl_set_stages; include/polar_hip.h).

Every frame's decisions, metric, flags and deciding list size against the rule's composition (tests/
test_cascl_adaptive_host.py compose()) of the oracle's SC and fixed-L CA-SCL decoders, with the pass bits from the numpy
CRC syndrome, on every stage kernel: k_sc_lanes, k_scl_fast2 and k_scl_big (N = 1024, stages 1, 8, 32); k_scl_generic
and k_scl_fast (N = 128, stages 1, 2, 8); N = 2048 with an explicit reliability order (stages 2, 16).  Then: f32 and the
large batch against the library's own fixed-L contexts, the input forms, the edges (all pass, all fail, single-stage and
cleared rules, CRC-file and systematic contexts), the consumers of the rule and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_cascl_adaptive_host import CRC6, CRC24C, FLAG_CRC_PASS, compose, syndrome  # noqa: E402

FLAG_TIE, FLAG_RERANK = 1, 4
DBS = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0)


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _beta_order(N):
    """polarization-weight reliability order (ascending), an explicit Q for N > 1024"""
    n = int(np.log2(N))
    beta = 2.0 ** 0.25
    w = [sum(beta ** b for b in range(n) if (i >> b) & 1) for i in range(N)]
    return [int(i) for i in np.argsort(np.array(w), kind="stable")]


def _frames(oracle, code, per, seed, dbs=DBS):
    llr, ys, sigs, us = [], [], [], []
    for k, db in enumerate(dbs):
        sim = oracle.Sim(seed + k)
        sig = oracle.sigma_from_db(db)
        u, y = sim.frames(code, sig, per)
        us += list(u)
        ys += list(y)
        sigs += [sig] * per
        llr += [oracle.llr_from_y(v, sig) for v in y]
    return np.stack(llr), np.stack(ys), np.array(sigs), np.stack(us)


def _adaptive(dec, x, sigma=0.0):
    """decode_cascl_device on a host array (float64 or float32) -> (u_hat, pm, flags, list)"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    B = d.shape[0]
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ls = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fills are done before the ctx stream reads the buffers
    bits = dec.decode_cascl_device(d, sigma=sigma, pm=pm, flags=fl, list_size=ls)
    dec.synchronize()
    return (_unpack(bits.cpu().numpy(), dec.N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32).astype(np.int64),
            ls.cpu().numpy().astype(np.int64))


def _fixed(dec, x, sigma=0.0):
    """polar_decode_device of a fixed context -> (u_hat, pm, flags)"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    B = d.shape[0]
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_device(d, sigma=sigma, pm=pm, flags=fl)
    dec.synchronize()
    return _unpack(bits.cpu().numpy(), dec.N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32).astype(np.int64)


def _lib_composition(N, K, taps, stages, x, sigma=0.0, **kw):
    """The rule's output from the library's own fixed contexts (SC over I[0..K+r) for L = 1)."""
    import polardecoding_amd as pa
    top = pa.CASCL(N, K, L=stages[-1], crc_taps=taps, **kw)
    io = top.info_order
    outs, passes = [], []
    for L in stages:
        if L == 1:
            sc = pa.Decoder(N, top.A, pa.ALGO_SC, L=1, dtype=kw.get("dtype", pa.F64), info_order=io)
            uh, pm, fl = _fixed(sc, x, sigma)
            ok = syndrome(uh, io, taps) == 0
            fl = fl | np.where(ok, FLAG_CRC_PASS, 0)
        else:
            uh, pm, fl = _fixed(top if L == stages[-1] else pa.CASCL(N, K, L=L, crc_taps=taps, **kw), x, sigma)
            ok = (fl & FLAG_CRC_PASS) != 0
        outs.append((L, uh, pm, fl))
        passes.append(ok)
    return compose(outs, passes)


def _oracle_composition(oracle, code, taps, stages, llr, dtype="f64"):
    """The rule's output from the oracle: SC of the code with the CRC positions as information bits, CA-SCL with L_s;
    flags = TIE from the oracle's ties, CRC_PASS from the syndrome of the chosen path.  dtype "f32": the oracle in float
    (the metrics are floats, returned widened)."""
    io = code.info_order
    outs, passes = [], []
    for L in stages:
        if L == 1:
            q = [j for j in range(code.N) if j not in set(io.tolist())] + io.tolist()
            sc = oracle.Code(code.N, code.A, None, Q=q)
            uh, _, _ = oracle.decode(sc, llr, "SC", dtype=dtype)
            pm, ties = np.zeros(len(llr)), np.zeros(len(llr), dtype=np.int64)
        else:
            uh, pm, ties = oracle.decode(code, llr, "CASCL", L=L, dtype=dtype)
        ok = syndrome(uh, io, taps) == 0
        fl = np.where(ties > 0, FLAG_TIE, 0) | np.where(ok, FLAG_CRC_PASS, 0)
        outs.append((L, uh, np.asarray(pm, dtype=np.float64), fl))
        passes.append(ok)
    return compose(outs, passes)


def _same(got, want, label="", rerank_free=True):
    uh, pm, fl, ls = got
    wu, wpm, wfl, wls = want
    assert np.array_equal(uh, wu), label
    assert np.array_equal(pm.view(np.uint64), np.asarray(wpm, dtype=np.float64).view(np.uint64)), label   # bitwise
    mask = ~FLAG_RERANK if rerank_free else ~0
    assert np.array_equal(fl & mask, wfl & mask), label
    assert np.array_equal(ls, wls), label


# N, K, taps, stages, frames per Eb/N0 point, stage kernels the ctx must name, explicit Q
SHAPES = [(1024, 512, CRC24C, (1, 8, 32), 40, ("k_sc_lanes", "k_scl_fast2", "k_scl_big"), False),
          (128, 64, CRC6, (1, 2, 8), 60, ("k_sc_lanes", "k_scl_generic", "k_scl_fast<"), False),
          (2048, 1024, CRC24C, (2, 16), 12, ("k_scl_big", "k_scl_big"), True)]


@pytest.mark.parametrize("N,K,taps,stages,per,knames,explicit_q", SHAPES)
def test_oracle_parity_every_stage_kernel(N, K, taps, stages, per, knames, explicit_q, oracle):
    import polardecoding_amd as pa
    q = _beta_order(N) if explicit_q else None
    code = oracle.Code(N, K, taps, Q=q)
    kw = dict(info_order=code.info_order) if explicit_q else {}
    dec = pa.CASCL(N, K, L=stages[-1], crc_taps=taps, stages=stages, **kw)
    assert np.array_equal(dec.info_order, code.info_order)
    name = dec.kernel_name
    assert name.startswith("adaptive CA-SCL")
    pos = [name.find(k) for k in knames]
    assert all(p >= 0 for p in pos) and pos == sorted(pos), name
    llr, _, _, _ = _frames(oracle, code, per, 4100 + N)
    got = _adaptive(dec, llr)
    want = _oracle_composition(oracle, code, taps, stages, llr)
    _same(got, want, f"N={N}", rerank_free=True)
    ls = got[3]
    for L in stages:   # every stage decides some frames
        assert (ls == L).any(), (L, np.unique(ls, return_counts=True))
    assert (got[2] & FLAG_CRC_PASS).any() and not (got[2] & FLAG_CRC_PASS).all()


@pytest.mark.parametrize("N,K,taps,stages", [(1024, 512, CRC24C, (1, 8, 32)), (128, 64, CRC6, (1, 2, 8))])
def test_f32_equals_fixed_f32_contexts(N, K, taps, stages, oracle):
    import polardecoding_amd as pa
    code = oracle.Code(N, K, taps)
    llr, _, _, _ = _frames(oracle, code, 40, 5200 + N)
    dec = pa.CASCL(N, K, L=stages[-1], crc_taps=taps, stages=stages, dtype=pa.F32)
    for x in (llr, llr.astype(np.float32)):
        _same(_adaptive(dec, x), _lib_composition(N, K, taps, stages, x, dtype=pa.F32), str(x.dtype), rerank_free=False)


@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_input_forms_and_small_batches(B, oracle):
    """LLR f64 and y with sigma: the oracle composition; LLR f32: the library's fixed contexts on the same input."""
    import polardecoding_amd as pa
    N, K, stages = 1024, 512, (1, 8, 32)
    code = oracle.Code(N, K, CRC24C)
    sim = oracle.Sim(600 + B)
    sig = oracle.sigma_from_db(1.75)
    _, ys = sim.frames(code, sig, B)
    llr = np.stack([oracle.llr_from_y(y, sig) for y in ys])
    dec = pa.CASCL(N, K, L=32, stages=stages)
    want = _oracle_composition(oracle, code, CRC24C, stages, llr)
    _same(_adaptive(dec, llr), want, "llr f64", rerank_free=True)
    _same(_adaptive(dec, ys, sigma=sig), want, "y", rerank_free=True)
    x32 = llr.astype(np.float32)
    _same(_adaptive(dec, x32), _lib_composition(N, K, CRC24C, stages, x32), "llr f32", rerank_free=False)
    # the host-buffer form
    uh, pm, fl, ls = dec.decode_cascl_batch(llr)
    _same((uh, pm, fl.astype(np.int64), ls.astype(np.int64)), want, "batch", rerank_free=True)


def test_large_batch_equals_fixed_contexts():
    import torch
    import polardecoding_amd as pa
    N, K, stages, B = 1024, 512, (1, 8, 32), 200000
    dec = pa.CASCL(N, K, L=32, stages=stages)
    x = torch.empty((B, N), dtype=torch.float64, device="cuda")
    dec.generate_device(11, 0, 1.5, x)
    dec.synchronize()
    llr = x.cpu().numpy()
    del x
    got = _adaptive(dec, llr)
    _same(got, _lib_composition(N, K, CRC24C, stages, llr), "B=200000", rerank_free=False)
    assert all((got[3] == L).any() for L in stages)


def test_all_pass_batch_is_the_sc_context(oracle):
    import polardecoding_amd as pa
    N, K = 1024, 512
    code = oracle.Code(N, K, CRC24C)
    llr, _, _, _ = _frames(oracle, code, 300, 77, dbs=(8.0,))
    dec = pa.CASCL(N, K, L=32, stages=(1, 8, 32))
    uh, pm, fl, ls = _adaptive(dec, llr)
    assert (ls == 1).all()
    sc = pa.Decoder(N, dec.A, pa.ALGO_SC, info_order=dec.info_order)
    su, spm, sfl = _fixed(sc, llr)
    assert np.array_equal(uh, su) and (pm == 0.0).all() and np.array_equal(spm, pm)
    assert np.array_equal(fl, sfl | FLAG_CRC_PASS)


def test_all_fail_batch_is_fixed_lmax():
    import polardecoding_amd as pa
    N, K = 1024, 512
    llr = np.random.default_rng(3).normal(0.0, 2.0, size=(500, N))   # pure noise
    dec = pa.CASCL(N, K, L=32, stages=(1, 8, 32))
    got = _adaptive(dec, llr)
    fu, fpm, ffl = _fixed(pa.CASCL(N, K, L=32), llr)
    assert not (ffl & FLAG_CRC_PASS).any()
    _same(got, (fu, fpm, ffl, np.full(len(llr), 32)), "noise", rerank_free=False)


def test_single_stage_and_cleared_rule_are_the_default(oracle):
    import polardecoding_amd as pa
    N, K = 1024, 512
    code = oracle.Code(N, K, CRC24C)
    llr, _, _, _ = _frames(oracle, code, 30, 900)
    ref = _fixed(pa.CASCL(N, K, L=8), llr)
    dec = pa.CASCL(N, K, L=8)
    default_name = dec.kernel_name
    for rule in ((8,), (1, 8), None, ()):
        dec.set_cascl_stages(rule)
        if rule == (1, 8):
            assert dec.kernel_name != default_name
            continue
        assert dec.kernel_name == default_name
        assert dec.cascl_stages == ()
        uh, pm, fl, ls = _adaptive(dec, llr)
        _same((uh, pm, fl, ls), ref + (np.full(len(llr), 8),), str(rule), rerank_free=False)
        assert np.array_equal(_fixed(dec, llr)[0], ref[0])


def test_crc_file_and_systematic_contexts(oracle, tmp_path):
    import polardecoding_amd as pa
    path = str(tmp_path / "CRC_6.dat")
    pa.save_crc_matrix(path, 64, CRC6)
    code = oracle.Code(128, 64, CRC6)
    llr, _, _, _ = _frames(oracle, code, 60, 1300)
    dec = pa.CASCL(128, 64, L=8, crc_file=path, stages=(1, 2, 8))
    _same(_adaptive(dec, llr), _oracle_composition(oracle, code, CRC6, (1, 2, 8), llr), "crc file", rerank_free=True)
    scode = oracle.Code(1024, 512, CRC24C, systematic=True)
    llr, _, _, _ = _frames(oracle, scode, 30, 1400)
    dec = pa.CASCL(1024, 512, L=8, systematic=True, stages=(1, 8))
    _same(_adaptive(dec, llr), _oracle_composition(oracle, scode, CRC24C, (1, 8), llr), "systematic", rerank_free=True)


def test_fer_batch_honours_the_rule():
    """polar_fer_batch's block and bit errors equal those of the composition on the polar_generate_device frames (B above
    the size at which the fixed decoder splits the batch over two streams)."""
    import torch
    import polardecoding_amd as pa
    N, K, stages, B, db, seed = 1024, 512, (1, 8, 32), 40000, 1.5, 21
    dec = pa.CASCL(N, K, L=32, stages=stages)
    x = torch.empty((B, N), dtype=torch.float64, device="cuda")
    ub = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    dec.generate_device(seed, 1000, db, x, u_bits=ub)
    dec.synchronize()
    llr, u = x.cpu().numpy(), _unpack(ub.cpu().numpy(), N)
    del x
    uh = _lib_composition(N, K, CRC24C, stages, llr)[0]
    io = dec.info_order
    err = (uh[:, io] != u[:, io]).sum(axis=1)
    blk, bits = dec.fer_batch(seed, 1000, db, B)
    assert (blk, bits) == (int((err > 0).sum()), int(err.sum()))
    assert blk > 0


def test_decode_and_stop_rule_honour_the_rule(oracle):
    import polardecoding_amd as pa
    N, K, stages = 1024, 512, (1, 8, 32)
    code = oracle.Code(N, K, CRC24C)
    sig = oracle.sigma_from_db(1.0)
    us, ys = oracle.Sim(31).frames(code, sig, 200)
    llr = np.stack([oracle.llr_from_y(y, sig) for y in ys])
    want = _lib_composition(N, K, CRC24C, stages, llr)
    dec = pa.CASCL(N, K, L=32, stages=stages)
    for b in (0, 1, 2):
        assert np.array_equal(dec(ys[b], sig), want[0][b])
    uh, pm, fl = dec.decode_batch_y(ys, sig)
    assert np.array_equal(uh, want[0]) and np.array_equal(pm, want[1])
    io = code.info_order
    err = (want[0][:, io] != us[:, io]).sum(axis=1)
    assert (err > 0).sum() >= 2
    need = int((err > 0).sum()) // 2
    cut = int(np.flatnonzero(np.cumsum(err > 0) >= need)[0]) + 1
    used, blk, bits = dec.stop_rule_batch_y(ys, sig, us, need)
    assert (used, blk, bits) == (cut, int((err[:cut] > 0).sum()), int(err[:cut].sum()))
    assert (want[3] > 1).any()


def test_refusals_leave_the_ctx_usable(oracle):
    import torch
    import polardecoding_amd as pa
    N, K = 1024, 512
    code = oracle.Code(N, K, CRC24C)
    llr, _, _, _ = _frames(oracle, code, 20, 2000, dbs=(1.5,))
    dec = pa.CASCL(N, K, L=32, stages=(1, 8, 32))
    ref = _adaptive(dec, llr)
    with pytest.raises(pa.PolarError):
        pa.SCLdecode(N, K, L=8).set_cascl_stages((1, 8))
    for bad in ((8, 1, 32), (1, 6, 32), (1, 8, 16), (1, 8, 32, 64), (1, 2, 4, 8, 16, 32, 32), (8, 8, 32), (0, 32)):
        with pytest.raises(pa.PolarError):
            dec.set_cascl_stages(bad)
    assert dec.cascl_stages == (1, 8, 32)
    _same(_adaptive(dec, llr), ref, "after refused rules", rerank_free=False)
    # a call while the ctx stream is capturing: POLAR_EINVAL, nothing captured
    d = torch.from_numpy(llr).cuda()
    out = torch.empty((len(llr), N // 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    refused = False
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dec.use_torch_stream()
        with torch.cuda.graph(g, stream=s):
            out.zero_()
            try:
                dec.decode_cascl_device(d, out_bits=out)
            except pa.PolarError:
                refused = True
    torch.cuda.synchronize()
    dec.use_torch_stream()
    assert refused
    del g
    _same(_adaptive(dec, llr), ref, "after the capture", rerank_free=False)


def test_polar_sim_stages():
    sim = os.path.join(REPO, "polardecoding_amd", "lib", "polar_sim")
    base = [sim, "--algo", "cascl", "--N", "1024", "--K", "512", "--L", "32", "--crc", "24c", "--fast", "--snr", "2.5:2.5:0.5",
            "--ble", "5", "--batch", "16384"]
    r = subprocess.run(base + ["--stages", "1,8,32"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "2.5" in r.stdout
    r = subprocess.run(base + ["--stages", "1,8,32", "--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--stages" in r.stderr
    r = subprocess.run(base + ["--stages", "1,8,16"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--stages" in r.stderr
