"""GPU: soft-output SCAN (POLAR_ALGO_SCAN; include/polar_hip.h).

Every frame's decisions, u-bit LLRs and extrinsic code-bit LLRs against scan_model() of tests/test_scan_host.py (the numpy
restatement of the definition on the oracle's check node): u_hat bit for bit, llr_u and ext_x equal by ==, the infinities
in the same places, in f64 and in f32 (against the model run in np.float32).  Then the input forms, rate-matched contexts,
the consumers of the decoder (FER, stop rule, polar_sim), graph capture and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_scan_host import breaking_mask, scan_model  # noqa: E402

DBS = (1.0, 1.5, 2.0, 2.5)


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _frames(oracle, code, B, seed, dbs=DBS):
    """B oracle frames spread over the Eb/N0 points: (llr [B][N], y [B][N], sigma [B], u [B][N])"""
    per = -(-B // len(dbs))
    llr, ys, sig, us = [], [], [], []
    for k, db in enumerate(dbs):
        s = oracle.sigma_from_db(db)
        u, y = oracle.Sim(seed + k).frames(code, s, per)
        us.append(u)
        ys.append(y)
        sig += [s] * per
        llr += [oracle.llr_from_y(v, s) for v in y]
    return np.stack(llr)[:B], np.concatenate(ys)[:B], np.array(sig)[:B], np.concatenate(us)[:B]


def _scan(dec, x, sigma=0.0, soft=True):
    """decode_scan_device on a host array (float64 or float32) -> (u_hat, llr_u, ext_x)"""
    import torch
    import polardecoding_amd as pa
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    B = d.shape[0]
    ty = torch.float32 if dec.dtype == pa.F32 else torch.float64
    lu = torch.full((B, dec.N), float("nan"), dtype=ty, device="cuda") if soft else None
    ex = torch.full((B, dec.N), float("nan"), dtype=ty, device="cuda") if soft else None
    torch.cuda.synchronize()   # torch's fills are done before the ctx stream reads the buffers
    bits = dec.decode_scan_device(d, sigma=sigma, llr_u=lu, ext_x=ex)
    dec.synchronize()
    return (_unpack(bits.cpu().numpy(), dec.N), lu.cpu().numpy() if soft else None, ex.cpu().numpy() if soft else None)


def _same(got, want, label=""):
    uh, lu, ex = got
    wu, wlu, wex = want
    assert np.array_equal(uh, wu), (label, "u_hat", np.flatnonzero((uh != wu).any(axis=1))[:10])
    for name, g, w in (("llr_u", lu, wlu), ("ext_x", ex, wex)):
        assert g.dtype == w.dtype, (label, name)
        assert not np.isnan(g).any(), (label, name, "NaN", np.argwhere(np.isnan(g))[:5])
        assert np.array_equal(np.isinf(g), np.isinf(w)), (label, name, "infinities")
        bad = g != w
        assert not bad.any(), (label, name, int(bad.sum()), np.argwhere(bad)[:5])


# N, K, I, B
CASES = [(128, 64, I, B) for I in (1, 2, 4, 8) for B in (1, 63, 64, 65, 4177)] + \
        [(N, K, I, 300) for N, K in ((32, 16), (256, 100), (512, 256)) for I in (1, 2, 4, 8)] + \
        [(1024, 512, 1, 65), (1024, 512, 2, 200), (1024, 512, 4, 321), (1024, 512, 8, 64)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N,K,I,B", CASES)
def test_library_equals_model(N, K, I, B, dtype, oracle):
    import polardecoding_amd as pa
    code = oracle.Code(N, K)
    f32 = dtype == "f32"
    dec = pa.SCAN(N, K, iters=I, dtype=pa.F32 if f32 else pa.F64)
    assert np.array_equal(dec.info_order, code.info_order) and dec.L == 1
    assert "k_scan_lanes" in dec.kernel_name and f"I={I}" in dec.kernel_name
    llr, _, _, _ = _frames(oracle, code, B, 2000 + 7 * I + B)
    want = scan_model(code.frozen, llr, I, dtype=np.float32 if f32 else np.float64, oracle=oracle, skip=True)
    _same(_scan(dec, llr), want, f"N={N} I={I} B={B} {dtype}")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("which", ["rate_0.9", "rate_0.1", "breaking_128", "breaking_1024"])
def test_extra_codes(which, dtype, oracle):
    import polardecoding_amd as pa
    f32 = dtype == "f32"
    rng = np.random.default_rng(11)
    if which.startswith("rate"):
        N, K = 256, (230 if which == "rate_0.9" else 26)
        dec = pa.SCAN(N, K, dtype=pa.F32 if f32 else pa.F64)
        fz = np.asarray(oracle.Code(N, K).frozen)
    else:
        N = int(which.split("_")[1])
        fz = breaking_mask(N, 77 + N)
        info = np.flatnonzero(fz == 0).astype(np.int32)
        dec = pa.Decoder(N, len(info), pa.ALGO_SCAN, info_order=info, dtype=pa.F32 if f32 else pa.F64)
    sig = 0.8
    llr = 2 * (1 + sig * rng.normal(size=(150, N))) / sig / sig
    for I in (1, 4):
        dec.set_scan_iters(I)
        want = scan_model(fz, llr, I, dtype=np.float32 if f32 else np.float64, oracle=oracle, skip=True)
        _same(_scan(dec, llr), want, f"{which} I={I} {dtype}")


def test_input_forms(oracle):
    import torch
    import polardecoding_amd as pa
    N, K, I, B = 128, 64, 4, 300
    code = oracle.Code(N, K)
    llr, ys, sig, _ = _frames(oracle, code, B, 3100, dbs=(1.5,))
    dec = pa.SCAN(N, K)
    assert dec.scan_iters is None and "I=4" in dec.kernel_name   # the default
    want = scan_model(code.frozen, llr, I, oracle=oracle)
    _same(_scan(dec, llr), want, "llr")
    _same(_scan(dec, ys, sigma=sig[0]), want, "y with sigma")
    x32 = llr.astype(np.float32)
    _same(_scan(dec, x32), scan_model(code.frozen, x32.astype(np.float64), I, oracle=oracle), "f64 ctx, f32 input")
    d32 = pa.SCAN(N, K, dtype=pa.F32)
    _same(_scan(d32, x32), scan_model(code.frozen, x32, I, dtype=np.float32, oracle=oracle), "f32 ctx, f32 input")
    # NULL soft buffers, then NULL decisions
    assert np.array_equal(_scan(dec, llr, soft=False)[0], want[0])
    d = torch.from_numpy(llr).cuda()
    ex = torch.full((B, N), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert dec.decode_scan_device(d, out_bits=False, ext_x=ex) is None
    dec.synchronize()
    assert np.array_equal(ex.cpu().numpy(), want[2])
    # the host-buffer forms
    uh, lu, ex = dec.decode_scan_batch(llr)
    _same((uh, lu, ex), want, "polar_scan_decode_batch")
    uh, pm, fl = dec.decode_batch(llr)   # polar_decode_batch
    assert np.array_equal(uh, want[0]) and (pm == 0.0).all() and (fl == 0).all()
    uh, pm, fl = dec.decode_batch_y(ys, sig[0])
    assert np.array_equal(uh, want[0])
    for b in (0, 1, 7):   # polar_decode, the reference call shape
        assert np.array_equal(dec(ys[b], sig[b]), want[0][b]), b
    # a frozen_mask override, as for SC
    other = oracle.Code(N, 40)
    uh, _, _ = dec.decode_batch(llr, frozen_mask=other.frozen)
    assert np.array_equal(uh, scan_model(other.frozen, llr, I, oracle=oracle)[0])
    assert np.array_equal(dec.decode_batch(llr)[0], want[0])


@pytest.mark.parametrize("E", [864, 700, 1500])
def test_rate_matched_context(E, oracle):
    import torch
    import polardecoding_amd as pa
    N, K, B = 1024, 350, 130
    dec = pa.Decoder(N, K, pa.ALGO_SCAN, E=E)
    assert dec.E == E and dec.rm_mode == {864: pa.RM_PUNCTURE, 700: pa.RM_SHORTEN, 1500: pa.RM_REPEAT}[E]
    rng = np.random.default_rng(E)
    sig = 0.7
    x = 2 * (1 + sig * rng.normal(size=(B, E))) / sig / sig
    d = torch.from_numpy(x).cuda()
    rows = torch.empty((B, N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dec.rm_recover_device(d, out=rows)
    dec.synchronize()
    fz = np.ones(N, dtype=np.uint8)
    fz[dec.info_order] = 0
    want = scan_model(fz, rows.cpu().numpy(), 4, oracle=oracle, skip=True)
    _same(_scan(dec, x), want, f"E={E}")
    assert want[2].shape == (B, N)


def test_fer_batch_stop_rule_and_sc(oracle):
    import torch
    import polardecoding_amd as pa
    N, K, B, db, seed = 1024, 512, 1 << 16, 2.0, 21
    errs = {}
    for I in (1, 4):
        dec = pa.SCAN(N, K, iters=I)
        x = torch.empty((B, N), dtype=torch.float64, device="cuda")
        ub = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        dec.generate_device(seed, 1000, db, x, u_bits=ub)
        dec.synchronize()
        torch.cuda.synchronize()
        bits = dec.decode_scan_device(x)
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        dec.count_errors_device(bits, ub, cnt)
        dec.synchronize()
        want = tuple(cnt.cpu().tolist())
        got = dec.fer_batch(seed, 1000, db, B)
        print(f"SCAN I={I}: block errors {got[0]}, bit errors {got[1]} of {B}")
        assert got == want
        errs[I] = got[0]
        del x, ub, bits
    sc = pa.SCdecode(N, K)
    errs["sc"] = sc.fer_batch(seed, 1000, db, B)[0]
    print(f"SC: block errors {errs['sc']} of {B}")
    assert errs[4] < errs[1]
    assert errs[4] < errs["sc"]
    # the stop rule on host buffers against a literal loop
    dec = pa.SCAN(N, K)
    code = oracle.Code(N, K)
    sig = oracle.sigma_from_db(1.5)
    us, ys = oracle.Sim(31).frames(code, sig, 300)
    llr = np.stack([oracle.llr_from_y(y, sig) for y in ys])
    uh = scan_model(code.frozen, llr, 4, oracle=oracle, skip=True)[0]
    io = code.info_order
    err = (uh[:, io] != us[:, io]).sum(axis=1)
    assert (err > 0).sum() >= 2
    need = int((err > 0).sum()) // 2
    cut = int(np.flatnonzero(np.cumsum(err > 0) >= need)[0]) + 1
    assert dec.stop_rule_batch_y(ys, sig, us, need) == (cut, int((err[:cut] > 0).sum()), int(err[:cut].sum()))


def test_graph_capture_replays_the_same_bits(oracle):
    import torch
    import polardecoding_amd as pa
    N, K, B = 1024, 512, 2000
    code = oracle.Code(N, K)
    llr, _, _, _ = _frames(oracle, code, B, 7100, dbs=(1.5, 2.0))
    dec = pa.SCAN(N, K)
    ref = _scan(dec, llr)   # the warm-up at the same B
    d = torch.from_numpy(llr).cuda()
    out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    lu = torch.empty((B, N), dtype=torch.float64, device="cuda")
    ex = torch.empty((B, N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dec.use_torch_stream()
        with torch.cuda.graph(g, stream=s):
            dec.decode_scan_device(d, out_bits=out, llr_u=lu, ext_x=ex)
    torch.cuda.synchronize()
    for _ in range(2):
        out.zero_()
        lu.fill_(float("nan"))
        ex.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same((_unpack(out.cpu().numpy(), N), lu.cpu().numpy(), ex.cpu().numpy()), ref, "replay")
    dec.use_torch_stream()
    del g


def test_refusals_leave_the_ctx_usable(oracle, tmp_path):
    import torch
    import polardecoding_amd as pa
    N, K = 128, 64
    code = oracle.Code(N, K)
    llr, _, _, _ = _frames(oracle, code, 200, 6100, dbs=(1.5,))
    dec = pa.SCAN(N, K, iters=2)
    ref = _scan(dec, llr)
    d = torch.from_numpy(llr).cuda()
    for bad in (0, -1, 65, 1000):
        with pytest.raises(pa.PolarError) as e:
            dec.set_scan_iters(bad)
        assert "rc=-1" in str(e.value)
    assert "I=2" in dec.kernel_name
    for other in (pa.SCdecode(N, K), pa.BP(N, K, iterMax=5), pa.CASCL(N, K, L=8, crc_taps=pa.CRC6_TAPS)):
        with pytest.raises(pa.PolarError) as e:
            other.set_scan_iters(4)
        assert "rc=-1" in str(e.value)
        with pytest.raises(pa.PolarError) as e:
            other.decode_scan_device(d)
        assert "rc=-1" in str(e.value)
        with pytest.raises(pa.PolarError):
            other.decode_scan_batch(llr)
    for call in (lambda: dec.set_bp_stop("g"), lambda: dec.decode_bp_device(d), lambda: dec.decode_bp_batch(llr),
                 lambda: dec.set_cascl_stages((1, 8)), lambda: dec.decode_cascl_device(d), lambda: dec.decode_cascl_batch(llr),
                 lambda: dec.set_scf_flips(4), lambda: dec.decode_scf_device(d), lambda: dec.decode_scf_batch(llr)):
        with pytest.raises(pa.PolarError) as e:
            call()
        assert "rc=-1" in str(e.value)
    path = str(tmp_path / "CRC_6.dat")
    pa.save_crc_matrix(path, K, pa.CRC6_TAPS)
    with pytest.raises(pa.PolarError) as e:   # polar_create_crc_file
        pa.Decoder(N, K, pa.ALGO_SCAN, crc_file=path)
    assert "rc=-1" in str(e.value)
    with pytest.raises(pa.PolarError) as e:   # no kernel above N = 1024
        pa.SCAN(2048, 1024)
    assert "rc=-4" in str(e.value)
    _same(_scan(dec, llr), ref, "after refusals")


def test_polar_sim_scan():
    sim = os.path.join(REPO, "polardecoding_amd", "lib", "polar_sim")
    base = [sim, "--algo", "scan", "--N", "1024", "--K", "512", "--snr", "2.0:2.5:0.5", "--ble", "5"]
    for extra in (["--fast", "--batch", "16384"], ["--batch", "2048"]):   # polar_fer_batch; polar_stop_rule_batch_y
        r = subprocess.run(base + extra + ["--iters", "2"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = [ln for ln in r.stdout.splitlines() if "bSNR = " in ln]
        assert len(lines) == 2 and "error block" in lines[0] and "BLER" in lines[0], r.stdout
    r = subprocess.run(base + ["--iters", "65"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--iters" in r.stderr
