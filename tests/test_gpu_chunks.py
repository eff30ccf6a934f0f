"""GPU: every chunked host loop of csrc/polar_hip.hip and csrc/h_*.hip across its pass boundaries, at small shapes.

The loops cut a batch into passes of at most 256 MiB of rows and offset every input, output and list pointer per pass; a
slipped offset changes every frame beyond the first pass and nothing else.  polardecoding_amd.testing.chunk_bytes() lowers
the cap of one context, so that the cases of tests/chunk_cases.py (held to their conditions by tests/test_chunks_host.py)
make three and more passes with a few hundred frames.  Every case runs four decodes on one context: uncapped on a small
batch, capped on the whole batch, uncapped on the whole batch, capped again (the scratch buffers shrink and grow in between);
every per-frame output of the entry point, pre-filled with a sentinel, must equal the reference by ==: the numpy models for
Q8, SC-Flip, dynamic SC-Flip, BPL and the genie counters, the oracle composition for the adaptive rule, and for a
rate-matched context a plain uncapped context on test_rm_host.recover()'s rows.  No capped context outlives its test."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import chunk_cases as CC  # noqa: E402
import test_construct_host as GM  # noqa: E402
import test_gpu_bpl as BT  # noqa: E402
import test_gpu_cascl_adaptive as AD  # noqa: E402
import test_gpu_dscf as DS  # noqa: E402
import test_gpu_q8 as Q8T  # noqa: E402
import test_gpu_scf as ST  # noqa: E402
import test_rm_host as RM  # noqa: E402
from test_cascl_adaptive_host import CRC6  # noqa: E402

SMALL = CC.B_SMALL


def _cap(dec, nbytes):
    from polardecoding_amd import testing as T
    return T.chunk_bytes(dec, nbytes)


def _cut(want, n):
    return tuple(np.asarray(a)[:n] for a in want)


def _four(dec, cap, run, same, x, want, label, small=SMALL):
    """the four decodes of a case, on one context; leaves the context capped"""
    _cap(dec, 0)   # the context moves into the test library before its first decode
    same(run(dec, x[:small]), _cut(want, small), f"{label}: uncapped, B = {small}")
    _cap(dec, cap)
    same(run(dec, x), want, f"{label}: capped at {cap} bytes")
    _cap(dec, 0)
    same(run(dec, x), want, f"{label}: uncapped")
    _cap(dec, cap)
    same(run(dec, x), want, f"{label}: capped again")


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def test_setter_refuses_a_null_context_and_zero_restores():
    import ctypes as C
    import polardecoding_amd as pa
    lib = pa.load_library(testing=True)
    lib.polar_testing_chunk_bytes.argtypes = [C.c_void_p, C.c_size_t]
    assert lib.polar_testing_chunk_bytes(None, 64) == -1   # POLAR_EINVAL
    dec = pa.SCdecode(64, 32, dtype=pa.Q8)
    try:
        assert _cap(dec, 1) is dec and dec._chunk_bytes == 1
        assert _cap(dec, 0)._chunk_bytes == 0
    finally:
        dec.close()


# ---- q8_decode_rows ---------------------------------------------------------------------------------------------------------
def _q8_dec(ctx):
    import polardecoding_amd as pa
    s = CC.Q8_CTX[ctx]
    if s["sc"]:
        return pa.SCdecode(CC.Q8_N, s["K"], dtype=pa.Q8)
    if s["taps"]:
        return pa.CASCL(CC.Q8_N, s["K"], L=s["L"], crc_taps=s["taps"], dtype=pa.Q8)
    return pa.SCLdecode(CC.Q8_N, s["K"], L=s["L"], dtype=pa.Q8)


@pytest.mark.parametrize("ctx", list(CC.Q8_CTX))
def test_q8_rows(ctx):
    import torch
    s = CC.Q8_CTX[ctx]
    dec = _q8_dec(ctx)
    try:
        assert dec.quant == (2.0, 8, 8)
        assert np.array_equal(dec.info_order, CC.info_order(CC.Q8_N, dec.A))
        for family in ("gauss", "ternary"):
            x, want = CC.q8_rows(family), CC.q8_want(ctx, family)
            _four(dec, CC.ROW_CAP, lambda d, r: Q8T._float_device(d, r, np.float64), Q8T._same, x, want, f"{ctx} {family} double rows")
            # capped from here on: float rows, the other batch sizes, no pm and no flags
            Q8T._same(Q8T._float_device(dec, x, np.float32), want, f"{ctx} {family} float rows")
            for B in (CC.B_EVEN, CC.B_SMALL):
                Q8T._same(Q8T._float_device(dec, x[:B], np.float64), _cut(want, B), f"{ctx} {family} B={B}")
            for dt in (np.float64, np.float32):
                bits = torch.full((len(x), dec.NW), -1, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                dec.decode_device(_cuda(x.astype(dt)), out_bits=bits)
                dec.synchronize()
                assert np.array_equal(Q8T._unpack(bits.cpu().numpy(), dec.N), want[0]), (ctx, family, dt, "bits only")
        if s["taps"]:   # y rows with sigma, and the CA-SCL entry point with its list size
            want = CC.q8_want(ctx, "gauss", y=True)
            Q8T._same(Q8T._float_device(dec, CC.q8_y("gauss"), np.float64, sigma=CC.Q8_SIGMA), want, "y rows")
            x, want = CC.q8_rows("ternary"), CC.q8_want(ctx, "ternary")
            B = len(x)
            pm = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
            fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
            ls = torch.full((B,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            bits = dec.decode_cascl_device(_cuda(x), pm=pm, flags=fl, list_size=ls)
            dec.synchronize()
            Q8T._same((Q8T._unpack(bits.cpu().numpy(), dec.N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)), want,
                      "polar_cascl_decode_device")
            assert (ls.cpu().numpy() == s["L"]).all()
    finally:
        dec.close()


# ---- the rate-matched loop --------------------------------------------------------------------------------------------------
def _ints(B, n=1, fill=-1):
    import torch
    return [torch.full((B,), fill, dtype=torch.int32, device="cuda") for _ in range(n)]


def _host(bits, N, *outs):
    return (Q8T._unpack(bits.cpu().numpy(), N),) + tuple(o.cpu().numpy() for o in outs)


def _run_fixed(dec, x):
    import torch
    d = _cuda(x)
    pm = torch.full((len(x),), -1.0, dtype=torch.float64, device="cuda")
    fl, = _ints(len(x))
    torch.cuda.synchronize()
    bits = dec.decode_device(d, pm=pm, flags=fl)
    dec.synchronize()
    return _host(bits, dec.N, pm, fl)


def _run_cascl(dec, x):
    import torch
    d = _cuda(x)
    pm = torch.full((len(x),), -1.0, dtype=torch.float64, device="cuda")
    fl, ls = _ints(len(x), 2)
    torch.cuda.synchronize()
    bits = dec.decode_cascl_device(d, pm=pm, flags=fl, list_size=ls)
    dec.synchronize()
    return _host(bits, dec.N, pm, fl, ls)


def _run_sets(dec, x):
    import torch
    d = _cuda(x)
    fl, at = _ints(len(x), 2)
    st = torch.full((len(x), 3), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_scf_sets_device(d, flags=fl, attempts=at, sets=st)
    dec.synchronize()
    return _host(bits, dec.N, fl, at, st)


def _run_bp(dec, x):
    import torch
    d = _cuda(x)
    it, fl = _ints(len(x), 2)
    torch.cuda.synchronize()
    bits = dec.decode_bp_device(d, iters=it, flags=fl)
    dec.synchronize()
    return _host(bits, dec.N, it, fl)


def _run_bpl(dec, x):
    import torch
    d = _cuda(x)
    outs = _ints(len(x), 4)
    torch.cuda.synchronize()
    bits = dec.decode_bpl_device(d, iters=outs[0], flags=outs[1], graph=outs[2], total_iters=outs[3])
    dec.synchronize()
    return _host(bits, dec.N, *outs)


def _run_scan(dec, x):
    import torch
    import polardecoding_amd as pa
    d = _cuda(x)
    soft = torch.float32 if dec.dtype == pa.F32 else torch.float64
    lu = torch.full((len(x), dec.N), -12345.0, dtype=soft, device="cuda")
    ex = torch.full((len(x), dec.N), -12345.0, dtype=soft, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_scan_device(d, llr_u=lu, ext_x=ex)
    dec.synchronize()
    return _host(bits, dec.N, lu, ex)


def _bitwise(got, want, label):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (label, k)
        bad = np.flatnonzero((g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(axis=1))
        assert bad.size == 0, f"{label}: output {k} differs at frames {bad[:8]} ({bad.size} in all)"


def _rm_decoders(E, ibil):
    """(label, rate-matched context, plain context with the rate-matched order, the run that returns every output)"""
    import polardecoding_amd as pa
    N, K = CC.RM_N, CC.RM_K
    io, ioK = pa.rm_info_order(N, K + 6, E), pa.rm_info_order(N, K, E)
    kw = dict(E=E, ibil=ibil)
    yield "SC", pa.SCdecode(N, K, **kw), pa.SCdecode(N, K, info_order=ioK), _run_fixed
    yield "SCL8", pa.SCLdecode(N, K, L=8, **kw), pa.SCLdecode(N, K, L=8, info_order=ioK), _run_fixed
    yield "CASCL8", pa.CASCL(N, K, L=8, crc_taps=CRC6, **kw), pa.CASCL(N, K, L=8, crc_taps=CRC6, info_order=io), _run_cascl
    yield ("adaptive", pa.CASCL(N, K, L=8, crc_taps=CRC6, stages=CC.AD_STAGES, **kw),
           pa.CASCL(N, K, L=8, crc_taps=CRC6, stages=CC.AD_STAGES, info_order=io), _run_cascl)
    yield "SCF8", pa.SCFlip(N, K, T=8, crc_taps=CRC6, **kw), pa.SCFlip(N, K, T=8, crc_taps=CRC6, info_order=io), _run_sets
    yield ("DSCF(4,4)", pa.DSCFlip(N, K, budgets=(4, 4), crc_taps=CRC6, **kw),
           pa.DSCFlip(N, K, budgets=(4, 4), crc_taps=CRC6, info_order=io), _run_sets)
    yield ("BPstop", pa.BP(N, K, iterMax=30, early_stop="g", **kw), pa.BP(N, K, iterMax=30, early_stop="g", info_order=ioK),
           _run_bp)
    yield "BPL", pa.BPL(N, K, iterMax=12, **kw), pa.BPL(N, K, iterMax=12, info_order=ioK), _run_bpl
    yield "SCAN", pa.SCAN(N, K, **kw), pa.SCAN(N, K, info_order=ioK), _run_scan


@pytest.mark.parametrize("E,ibil,mode", CC.RM_E)
def test_rate_matched_rows(E, ibil, mode):
    x = CC.rm_rows(E)
    for label, rm, plain, run in _rm_decoders(E, ibil):
        try:
            assert rm.rm_mode == mode and rm.E == E and rm.ibil == ibil
            assert np.array_equal(rm.info_order, plain.info_order)
            inputs = [x] + ([x.astype(np.float32)] if label == "SCAN" else [])   # SCAN: an f64 ctx on float rows as well
            for xin in inputs:
                what = f"E={E} {label} {xin.dtype}"
                want = run(plain, RM.recover(xin, CC.RM_N, rm.A, int(ibil)))
                if label in ("SCF8", "DSCF(4,4)"):   # the pass loop inside a pass runs: frames fail, and flips decide some
                    assert (want[2] >= 1).sum() > 3 * 8 and (want[3][:, 0] >= 0).any(), what
                _four(rm, CC.RM_CAP, run, _bitwise, xin, want, what)
                for B in (CC.B_EVEN, CC.B_SMALL):
                    _bitwise(run(rm, xin[:B]), _cut(want, B), f"{what} B={B}")
        finally:
            rm.close()
            plain.close()


# ---- cascl_adaptive ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.AD_CASES, ids=lambda c: c.name)
def test_adaptive_later_stages(case, oracle):
    import torch
    import polardecoding_amd as pa
    dt, kind = case.spec
    x, want = CC.ad_rows(oracle, kind, dt), CC.ad_want(oracle, kind, dt)
    dec = pa.CASCL(CC.AD_N, CC.AD_K, L=CC.AD_STAGES[-1], crc_taps=CRC6, stages=CC.AD_STAGES, dtype=pa.F32 if dt == "f32" else pa.F64)
    try:
        assert np.array_equal(dec.info_order, CC.ad_code(oracle).info_order)
        xin = x.astype(np.float32) if dt == "f32" else x
        _four(dec, case.cap, AD._adaptive, lambda g, w, label: AD._same(g, w, label, rerank_free=True), xin, want, case.name)
        if dt == "f64":   # a float input on the f64 context: the rows are exact in float32
            AD._same(AD._adaptive(dec, x.astype(np.float32)), want, case.name + " float rows", rerank_free=True)
        # without pm (and without flags and list size): the decisions alone
        bits = torch.full((len(x), dec.NW), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_cascl_device(_cuda(xin), out_bits=bits)
        dec.synchronize()
        assert np.array_equal(AD._unpack(bits.cpu().numpy(), dec.N), want[0]), case.name + " bits only"
    finally:
        dec.close()


# ---- scf_decode, static pass B ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.SCF_CASES, ids=lambda c: c.name)
def test_static_flip_pass_b(case, oracle):
    import polardecoding_amd as pa
    T, dtype, kind = case.spec
    x = CC.scf_rows(oracle, case)
    u, flags, attempts, sets, fail = CC.scf_want(oracle, case)
    dec = pa.SCFlip(CC.SCF_N, CC.SCF_K, T=T, crc_taps=CRC6, dtype=pa.F32 if dtype == np.float32 else pa.F64)
    try:
        small = min(CC.B_SMALL, len(x) - 1)
        # polar_scf_decode_device resolves with k_scf_resolve, polar_scf_decode_sets_device with k_scf_resolve_sets
        _four(dec, case.cap, ST._scf, ST._same, x, (u, flags, attempts), case.name + " k_scf_resolve", small=small)
        _four(dec, case.cap, DS._dscf, _exact, x, (u, flags, attempts, sets), case.name + " k_scf_resolve_sets", small=small)
    finally:
        dec.close()


def _exact(got, want, label):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        bad = np.flatnonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1)) if g.shape == w.shape else None
        assert bad is not None and bad.size == 0, f"{label}: output {k} differs at frames {bad[:8] if bad is not None else 'shape'}"


# ---- scf_decode, the levels of the dynamic rule -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.DSCF_CASES, ids=lambda c: c.name)
def test_dynamic_flip_levels(case, oracle):
    import polardecoding_amd as pa
    N, budgets, c, dtype, _ = case.spec
    K, taps, _, _ = DS.SHAPE[N]
    x, want = CC.dscf_rows(oracle, case), CC.dscf_want(oracle, case)
    dec = pa.DSCFlip(N, K, budgets=budgets, c=c, tau=CC.TAU, crc_taps=taps, dtype=pa.F32 if dtype == np.float32 else pa.F64)
    try:
        assert dec.get_scf_dynamic() == (budgets, c, CC.TAU)
        _four(dec, case.cap, DS._dscf, _exact, x, (want.u, want.flags, want.attempts, want.sets), case.name,
              small=min(CC.B_SMALL, len(x) - 1))
        assert dec.get_scf_dynamic() == (budgets, c, CC.TAU)   # the rule came along into the test library
    finally:
        dec.close()


# ---- bpl_decode -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.BPL_CASES, ids=lambda c: c.name)
def test_bpl_attempts(case, oracle):
    import torch
    import polardecoding_amd as pa
    N, K, iters, which, taps = case.spec[:5]
    x, res = CC.bpl_rows(oracle, case), CC.bpl_want(oracle, case)
    code = CC.bpl_code(oracle, case)
    graphs = CC.bpl_graphs(code.n, which)
    dec = pa.BPL(N, K, iterMax=iters, graphs=None if which == "default" else graphs, crc_taps=taps)
    try:
        assert np.array_equal(dec.info_order, code.info_order) and np.array_equal(dec.bpl_graphs, np.asarray(graphs))
        want = BT._of_model(res)
        _four(dec, case.cap, BT._bpl, BT._same, x, want, case.name, small=min(CC.B_SMALL, len(x) - 1))
        assert np.array_equal(dec.bpl_graphs, np.asarray(graphs))   # the list came along into the test library
        BT._same(BT._bpl(dec, x.astype(np.float32)), want, case.name + " float rows")   # capped; the rows are exact in float32
        # the decisions alone: every optional pointer null
        for dt in (np.float64, np.float32):
            bits = torch.full((len(x), dec.NW), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            dec.decode_bpl_device(_cuda(x.astype(dt)), out_bits=bits)
            dec.synchronize()
            assert np.array_equal(BT._unpack(bits.cpu().numpy(), N), res.bits), (case.name, dt, "bits only")
    finally:
        dec.close()


# ---- polar_construct_batch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", [(32, np.float64), (128, np.float32)])
def test_construct_batch_first_frame_per_pass(N, dtype, oracle):
    import torch
    import polardecoding_amd as pa
    seed, first, sigma, B = 77, 5_000_000_000, 0.9, CC.B_RAGGED
    dec = pa.SCdecode(N, N // 2, dtype=pa.F32 if dtype == np.float32 else pa.F64)
    try:
        _cap(dec, 0)
        rows = torch.empty((B, N), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
        dec.genie_rows_device(seed, first, sigma, rows)
        dec.synchronize()
        xh = rows.cpu().numpy()
        models = {}
        for n in (CC.B_RAGGED, CC.B_EVEN, CC.B_SMALL):
            err, tie, _, _ = GM.genie_model(oracle, xh[:n], dtype)
            models[n] = np.stack([err, tie]).astype(np.uint64)
        assert models[B][0].sum() > 0 and not np.array_equal(models[B], models[CC.B_EVEN])

        def counts(n):
            c = torch.zeros((2, N), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            dec.construct_batch(seed, first, sigma, n, c)
            dec.synchronize()
            return c.cpu().numpy().view(np.uint64)

        assert np.array_equal(counts(CC.B_SMALL), models[CC.B_SMALL]), "uncapped, small"
        for cap in (CC.ROW_CAP, 0, CC.ROW_CAP):
            _cap(dec, cap)
            assert np.array_equal(counts(B), models[B]), f"cap {cap}"
        for n in (CC.B_EVEN, CC.B_SMALL):   # capped
            assert np.array_equal(counts(n), models[n]), n
    finally:
        dec.close()


# ---- polar_fer_batch: the rate-matched loop on both lanes ---------------------------------------------------------------------
def test_fer_batch_across_the_lanes():
    import polardecoding_amd as pa
    N, K, E, B, db = CC.FER_CASE.spec
    dec = pa.SCLdecode(N, K, L=8, E=E, ibil=True)
    try:
        _cap(dec, 0)
        want = dec.fer_batch(7, 0, db, B)
        assert want[0] > 0, want
        _cap(dec, CC.FER_CASE.cap)
        assert dec.fer_batch(7, 0, db, B) == want
        _cap(dec, 0)
        assert dec.fer_batch(7, 0, db, B) == want
    finally:
        dec.close()
