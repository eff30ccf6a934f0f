"""GPU: dynamic SC-Flip (polar_scf_set_dynamic; include/polar_hip.h).

Every frame's decisions, flags, attempts and reported flip set against dscf_model() of tests/dscf_model.py (the numpy
restatement of rules 1-8 on the oracle's check node) by ==: CRC-6 / N = 128 and CRC-24C / N = 1024, budgets (1, 1), (8, 8),
(4, 4, 4), (32, 32) and (8) with c = 1.5, c in {0, 1.5}, tau = 5, batches of 1, 63, 64 and one large one, oracle frames at
1.0 - 2.5 dB.  The seeds were chosen with the model so that every multi-level case has a frame decided at each level and
one that fails them all; the tests assert it.  Then f32, the input forms, N = 2048 (two wavefronts per workgroup), quantised
rows with tied keys at a list boundary, the identities of rule 8, the static rule restored, refusals and the consumers."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_cascl_adaptive_host import CRC6, CRC24C, FLAG_CRC_PASS, syndrome  # noqa: E402
from dscf_model import dscf_model, sc_run_sets  # noqa: E402

DBS = (1.0, 1.5, 2.0, 2.5)
TAU = 5.0
SHAPE = {128: (64, CRC6, 1500, 4100), 1024: (512, CRC24C, 600, 4204)}   # N: K, taps, frames, seed
_memo = {}


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


def _shape(oracle, N):
    """the frames of a shape, computed once: (code, llr, failing [B] bool of attempt 0)"""
    if N not in _memo:
        K, taps, B, seed = SHAPE[N]
        code = oracle.Code(N, K, taps)
        llr, _, _, _ = _frames(oracle, code, B, seed)
        u0, _ = sc_run_sets(oracle, code.frozen, llr)
        _memo[N] = (code, llr, syndrome(u0, code.info_order, taps) != 0)
    return _memo[N]


def _rows(oracle, N, budgets):
    """the rows a case decodes: all of the shape's, but at N >= 1024 with a budget of 32 about 100 failing frames"""
    code, llr, fail = _shape(oracle, N)
    if N >= 1024 and max(budgets) == 32:
        pick = np.sort(np.concatenate([np.flatnonzero(fail)[:100], np.flatnonzero(~fail)[:40]]))
        llr = llr[pick]
    return code, llr


def _want(oracle, N, budgets, c, dtype=np.float64):
    key = (N, budgets, c, dtype)
    if key not in _memo:
        code, llr = _rows(oracle, N, budgets)
        _memo[key] = dscf_model(code, llr, budgets, c, TAU, dtype=dtype, oracle=oracle)
    return _memo[key]


def levels_decided(res, budgets):
    """per level the number of frames it decided, and the number of frames no attempt decided"""
    passed = (res.flags & FLAG_CRC_PASS) != 0
    edges = np.concatenate([[0], np.cumsum(budgets)])
    per = [int((passed & (res.attempts > edges[k]) & (res.attempts <= edges[k + 1])).sum()) for k in range(len(budgets))]
    return per, int((~passed).sum())


def _dscf(dec, x, sigma=0.0):
    """decode_scf_sets_device on a host array (float64 or float32) -> (u_hat, flags, attempts, sets)"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    B = d.shape[0]
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    at = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    st = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fills are done before the ctx stream reads the buffers
    bits = dec.decode_scf_sets_device(d, sigma=sigma, flags=fl, attempts=at, sets=st)
    dec.synchronize()
    return (_unpack(bits.cpu().numpy(), dec.N), fl.cpu().numpy().view(np.uint32).astype(np.int64),
            at.cpu().numpy().astype(np.int64), st.cpu().numpy().astype(np.int64))


def _same(got, want, label="", rows=slice(None)):
    uh, fl, at, st = got
    assert np.array_equal(uh, want.u[rows]), (label, np.flatnonzero((uh != want.u[rows]).any(axis=1))[:10])
    assert np.array_equal(fl, want.flags[rows]), label
    assert np.array_equal(at, want.attempts[rows]), (label, np.flatnonzero(at != want.attempts[rows])[:10])
    assert np.array_equal(st, want.sets[rows]), (label, np.flatnonzero((st != want.sets[rows]).any(axis=1))[:10])


CASES = [(N, b, c) for N in (128, 1024) for b in ((1, 1), (8, 8), (4, 4, 4), (32, 32)) for c in (0.0, 1.5)] + \
        [(N, (8,), 1.5) for N in (128, 1024)]


@pytest.mark.parametrize("N,budgets,c", CASES)
def test_library_equals_model(N, budgets, c, oracle):
    import polardecoding_amd as pa
    K, taps, _, _ = SHAPE[N]
    code, llr = _rows(oracle, N, budgets)
    want = _want(oracle, N, budgets, c)
    per, none = levels_decided(want, budgets)
    assert all(p > 0 for p in per) and none > 0, (per, none)   # every level decides a frame, and a frame fails them all
    dec = pa.DSCFlip(N, K, budgets=budgets, c=c, tau=TAU, crc_taps=taps)
    assert np.array_equal(dec.info_order, code.info_order)
    assert dec.get_scf_dynamic() == (budgets, c, TAU)
    nm = dec.kernel_name
    assert "k_scf_lanes" in nm and f"omega={len(budgets)}" in nm and "T=" + ",".join(map(str, budgets)) in nm
    assert f"c={c:g}" in nm and "tau=5" in nm
    _same(_dscf(dec, llr), want, f"N={N} {budgets} c={c}")
    # batches of 1, 63 and 64, starting at a frame that the last level decided or that nothing decided
    s = int(np.flatnonzero(want.attempts > sum(budgets[:-1]))[0])
    s = max(0, min(s, len(llr) - 64))
    for B in (1, 63, 64):
        _same(_dscf(dec, llr[s:s + B]), want, f"N={N} {budgets} c={c} B={B}", rows=slice(s, s + B))


def test_f32_and_input_forms(oracle):
    import polardecoding_amd as pa
    N, budgets, c = 1024, (8, 8), 1.5
    K, taps, _, _ = SHAPE[N]
    code = oracle.Code(N, K, taps)
    llr, ys, sig, _ = _frames(oracle, code, 300, 4300, dbs=(1.5,))
    want32 = dscf_model(code, llr, budgets, c, TAU, dtype=np.float32, oracle=oracle)
    per, none = levels_decided(want32, budgets)
    assert all(p > 0 for p in per) and none > 0, (per, none)
    dec = pa.DSCFlip(N, K, budgets=budgets, c=c, tau=TAU, dtype=pa.F32)
    _same(_dscf(dec, llr), want32, "f32 ctx, f64 input")
    _same(_dscf(dec, llr.astype(np.float32)), want32, "f32 ctx, f32 input")
    d64 = pa.DSCFlip(N, K, budgets=budgets, c=c, tau=TAU)
    want = dscf_model(code, llr, budgets, c, TAU, oracle=oracle)
    _same(_dscf(d64, ys, sigma=sig[0]), want, "y with sigma")
    x32 = llr.astype(np.float32)
    _same(_dscf(d64, x32), dscf_model(code, x32.astype(np.float64), budgets, c, TAU, oracle=oracle), "f64 ctx, f32 input")
    two = int(np.flatnonzero(want.attempts > budgets[0])[0])
    for b in (0, two):   # polar_decode, the reference call shape
        assert np.array_equal(d64(ys[b], sig[b]), want.u[b]), b
    uh, pm, fl = d64.decode_batch(llr)   # polar_decode_batch
    assert np.array_equal(uh, want.u) and (pm == 0.0).all() and np.array_equal(fl.astype(np.int64), want.flags)
    uh, fl, at = d64.decode_scf_batch(llr)   # polar_scf_decode_batch
    assert np.array_equal(uh, want.u) and np.array_equal(at.astype(np.int64), want.attempts)
    uh, fl, at, st = d64.decode_scf_sets_batch(llr)   # polar_scf_decode_sets_batch
    _same((uh, fl.astype(np.int64), at.astype(np.int64), st.astype(np.int64)), want, "sets batch")


def test_n2048_two_waves_per_workgroup(oracle):
    import polardecoding_amd as pa
    N, K, budgets = 2048, 1024, (32, 32)   # the lists of the recording policies: 24 KiB per wavefront in f64
    dec = pa.DSCFlip(N, K, budgets=budgets, c=1.5, tau=TAU)
    io = dec.info_order.tolist()
    q = [j for j in range(N) if j not in set(io)] + io
    code = oracle.Code(N, K, CRC24C, Q=q)
    assert np.array_equal(code.info_order, dec.info_order)
    llr, _, _, _ = _frames(oracle, code, 96, 2050, dbs=(1.5, 2.0))
    want = dscf_model(code, llr, budgets, 1.5, TAU, oracle=oracle)
    per, none = levels_decided(want, budgets)
    assert all(p > 0 for p in per) and none > 0 and (want.attempts == 0).any(), (per, none)
    _same(_dscf(dec, llr), want, "N=2048")


def test_quantised_rows_tie_at_a_list_boundary(oracle):
    import polardecoding_amd as pa
    N, budgets = 128, (4, 4, 4)
    K, taps, _, _ = SHAPE[N]
    code, llr, _ = _shape(oracle, N)
    q = np.clip(np.round(llr[:700] * 4) / 4, -8.0, 8.0)
    for c, dtype, dt in ((1.5, np.float64, pa.F64), (0.0, np.float32, pa.F32)):
        want = dscf_model(code, q, budgets, c, TAU, dtype=dtype, oracle=oracle)
        assert all(len(t) > 0 for t in want.ties), [len(t) for t in want.ties]   # equal keys at the end of a list, every level
        per, none = levels_decided(want, budgets)
        assert all(p > 0 for p in per) and none > 0, (per, none)
        dec = pa.DSCFlip(N, K, budgets=budgets, c=c, tau=TAU, crc_taps=taps, dtype=dt)
        _same(_dscf(dec, q), want, f"quantised c={c}")


def test_order_one_without_penalty_is_the_static_decoder(oracle):
    import polardecoding_amd as pa
    N = 1024
    K, taps, _, _ = SHAPE[N]
    code, llr, _ = _shape(oracle, N)
    static = pa.SCFlip(N, K, T=8)
    ref = _dscf(static, llr)   # decode_scf_sets_device on a static ctx: at most one entry per set
    assert (ref[3][:, 1:] == -1).all() and (ref[3][:, 0] >= 0).any()
    assert np.array_equal(ref[3][:, 0] >= 0, (ref[2] >= 1) & ((ref[1] & FLAG_CRC_PASS) != 0))
    hit = ref[3][:, 0] >= 0
    assert np.isin(ref[3][hit, 0], code.info_order).all()
    dyn = pa.DSCFlip(N, K, budgets=(8,), c=0.0, tau=TAU)
    got = _dscf(dyn, llr)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    want = _want(oracle, N, (8, 8), 0.0)
    one = want.attempts <= 8   # rule 8: a frame decided at level 1 has the same output for every omega
    one &= (want.flags & FLAG_CRC_PASS) != 0
    assert np.array_equal(got[0][one], want.u[one]) and np.array_equal(got[3][one], want.sets[one])
    # omega = 0 restores the static rule and keeps T; set_scf_flips changes T_1 only
    name = static.kernel_name
    dyn.set_scf_dynamic((4, 4), 1.5, TAU)
    assert dyn.kernel_name != name and dyn.get_scf_dynamic() == ((4, 4), 1.5, TAU)
    dyn.set_scf_flips(8)
    assert dyn.get_scf_dynamic() == ((8, 4), 1.5, TAU)
    dyn.set_scf_dynamic(None)
    assert dyn.get_scf_dynamic() == ((), 0.0, 0.0) and dyn.kernel_name == name
    for a, b in zip(_dscf(dyn, llr), ref):
        assert np.array_equal(a, b)
    import torch
    d = torch.from_numpy(llr).cuda()
    at = torch.zeros(len(llr), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dyn.decode_scf_device(d, attempts=at)   # the existing entry point, the existing kernels
    dyn.synchronize()
    assert np.array_equal(_unpack(bits.cpu().numpy(), N), ref[0]) and np.array_equal(at.cpu().numpy(), ref[2])


def test_refusals_leave_the_ctx_unchanged(oracle):
    import torch
    import polardecoding_amd as pa
    N = 128
    K, taps, _, _ = SHAPE[N]
    code, llr, _ = _shape(oracle, N)
    llr = llr[:200]
    dec = pa.DSCFlip(N, K, budgets=(4, 4), c=1.5, tau=TAU, crc_taps=taps)
    ref = _dscf(dec, llr)
    state = dec.get_scf_dynamic()
    bad = [((4, 4, 4, 4), 1.5, TAU), ((0,), 1.5, TAU), ((4, 33), 1.5, TAU), ((4, 0), 1.5, TAU), ((33,), 0.0, 0.0),
           ((4, 4), -1.0, TAU), ((4, 4), 1.5, -0.5), ((4, 4), float("nan"), TAU), ((4, 4), 1.5, float("inf")),
           ((4, -1, 4), 1.5, TAU)]
    for b, c, tau in bad:
        with pytest.raises(pa.PolarError):
            dec.set_scf_dynamic(b, c, tau)
        assert dec.get_scf_dynamic() == state
    small = pa.SCFlip(32, 4, crc_taps=CRC6)   # A = 10: T_1 <= 10, later budgets up to 32
    small.set_scf_dynamic((10, 32), 0.0, 0.0)
    with pytest.raises(pa.PolarError):
        small.set_scf_dynamic((11, 4), 0.0, 0.0)
    with pytest.raises(pa.PolarError):
        pa.CASCL(1024, 512, L=8).set_scf_dynamic((4, 4), 1.5, TAU)
    with pytest.raises(pa.PolarError):
        pa.CASCL(1024, 512, L=8).get_scf_dynamic()
    with pytest.raises(pa.PolarError):
        pa.SCdecode(N, K).decode_scf_sets_device(torch.from_numpy(llr).cuda())
    for a, b in zip(_dscf(dec, llr), ref):
        assert np.array_equal(a, b)
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
                dec.decode_scf_sets_device(d, out_bits=out)
            except pa.PolarError:
                refused = True
    torch.cuda.synchronize()
    dec.use_torch_stream()
    assert refused
    del g
    for a, b in zip(_dscf(dec, llr), ref):
        assert np.array_equal(a, b)


def test_short_lists_on_a_tiny_code(oracle):
    """A = 10 information positions: a level-1 set whose position is the last one has no extension, so level 2 has fewer
    than T_2 candidates; the absent sets never pass and attempts of an undecided frame is still T_1 + T_2"""
    import polardecoding_amd as pa
    dec = pa.SCFlip(32, 4, crc_taps=CRC6)
    budgets = (2, 32)
    dec.set_scf_dynamic(budgets, 0.0, TAU)
    io = dec.info_order.tolist()
    q = [j for j in range(32) if j not in set(io)] + io
    code = oracle.Code(32, 4, CRC6, Q=q)
    assert np.array_equal(code.info_order, dec.info_order)
    llr, _, _, _ = _frames(oracle, code, 400, 3200, dbs=(0.0, 1.0))
    want = dscf_model(code, llr, budgets, 0.0, TAU, oracle=oracle)
    assert any(len(lst) < 32 for lst in want.lists[1].values())
    per, none = levels_decided(want, budgets)
    assert all(p > 0 for p in per) and none > 0, (per, none)
    _same(_dscf(dec, llr), want, "tiny code")


def test_rule_8_on_generated_frames(oracle):
    import torch
    import polardecoding_amd as pa
    N, K, B, db, seed = 1024, 512, 1 << 14, 2.0, 11
    one = pa.DSCFlip(N, K, budgets=(8,))
    two = pa.DSCFlip(N, K, budgets=(8, 16))
    x = torch.empty((B, N), dtype=torch.float64, device="cuda")
    ub = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    one.generate_device(seed, 0, db, x, u_bits=ub)
    one.synchronize()
    u = _unpack(ub.cpu().numpy(), N)
    io = one.info_order
    res = []
    for dec in (one, two):
        at = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        bits = dec.decode_scf_device(x, attempts=at)
        dec.synchronize()
        res.append((_unpack(bits.cpu().numpy(), N), at.cpu().numpy()))
    (u1, a1), (u2, a2) = res
    w1 = (u1[:, io] != u[:, io]).any(axis=1)
    w2 = (u2[:, io] != u[:, io]).any(axis=1)
    lvl1 = (a2 >= 1) & (a2 <= 8)
    assert lvl1.any() and np.array_equal(u1[a2 <= 8], u2[a2 <= 8]) and np.array_equal(a1[a2 <= 8], a2[a2 <= 8])
    assert not (w2 & ~w1).any()
    assert w2.sum() < w1.sum(), (w2.sum(), w1.sum())
    # the model agrees on a sample of the frames that only the pairs repaired, and on some that nothing did
    code = oracle.Code(N, K, CRC24C)
    pick = np.concatenate([np.flatnonzero(w1 & ~w2)[:24], np.flatnonzero(w2)[:8]])
    llr = x[torch.from_numpy(pick).cuda()].cpu().numpy()
    m1 = dscf_model(code, llr, (8,), 1.5, TAU, oracle=oracle)
    m2 = dscf_model(code, llr, (8, 16), 1.5, TAU, oracle=oracle)
    assert np.array_equal(m1.u, u1[pick]) and np.array_equal(m2.u, u2[pick]) and np.array_equal(m2.attempts, a2[pick])
    mw1 = (m1.u[:, io] != u[pick][:, io]).any(axis=1)
    mw2 = (m2.u[:, io] != u[pick][:, io]).any(axis=1)
    assert mw1.all() and mw2.sum() == min(8, int(w2.sum())) and mw2.sum() < mw1.sum()


def test_fer_batch_and_polar_sim_run_the_dynamic_rule():
    import torch
    import polardecoding_amd as pa
    N, K, B, db, seed = 1024, 512, 40000, 2.0, 21
    dec = pa.DSCFlip(N, K, budgets=(8, 8), c=0.0, tau=0.0)   # c = 0: rule 8 makes its wrong frames a subset of T = 8's
    x = torch.empty((B, N), dtype=torch.float64, device="cuda")
    ub = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    dec.generate_device(seed, 1000, db, x, u_bits=ub)
    bits = dec.decode_device(x)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    dec.count_errors_device(bits, ub, cnt)
    dec.synchronize()
    want = tuple(cnt.cpu().tolist())
    assert want[0] > 0
    assert dec.fer_batch(seed, 1000, db, B) == want
    static = pa.SCFlip(N, K, T=8)
    assert static.fer_batch(seed, 1000, db, B)[0] > want[0]   # the pairs repair frames the single flips leave wrong
    sim = os.path.join(REPO, "polardecoding_amd", "lib", "polar_sim")
    base = [sim, "--algo", "scf", "--N", "1024", "--K", "512", "--crc", "24c", "--snr", "2.0:2.0:0.5", "--ble", "5", "--fast",
            "--batch", "16384"]
    r = subprocess.run(base + ["--flips", "8,8", "--scf-metric", "1.5,5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "bSNR = " in ln]
    assert len(lines) == 1 and "error block" in lines[0] and "BLER" in lines[0], r.stdout
    r = subprocess.run(base + ["--flips", "8,40"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--flips" in r.stderr
