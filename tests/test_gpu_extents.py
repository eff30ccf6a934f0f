"""GPU: every device entry point writes inside its outputs, at batch sizes around a group of frames (tests/extents.py).

For every case of extents.CASES and every batch size one call runs with all outputs carved from one Arena: views at the
natural alignment of their type and no more, a guard of at least one whole group of rows (and 4096 bytes) on both sides.
Then: no guard byte changed; every output equals, with ==, the reference the kernel's own test uses (the CPU oracle, or the
numpy model of the decoder) on all B frames; the input rows are byte-identical to a snapshot taken before the call; the
context names the expected kernel.  The call is repeated on a fresh arena with each nullable output null, and with all of
them null: the remaining outputs must equal the first run.  Then the chunked host loops across a pass boundary against
their uncapped run, and the host-buffer forms with their outputs in a numpy arena against the device forms.

Rows are the all-zero codeword over BPSK + AWGN at 1.5 dB, rounded through float32; one seeded batch per row width.
tests/test_extents_host.py holds the Arena and the table to their conditions.  Reads beyond the inputs are not covered."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bpl_model as BM  # noqa: E402
import chunk_cases as CC  # noqa: E402
import extents as X  # noqa: E402
import q8_model as QM  # noqa: E402
import test_construct_host as GM  # noqa: E402
import test_dyn_host as DM  # noqa: E402
import test_encode_host as EM  # noqa: E402
import test_gpu_bpl as BT  # noqa: E402
import test_gpu_cascl_adaptive as AD  # noqa: E402
import test_gpu_chunks as CT  # noqa: E402
import test_gpu_encode as GE  # noqa: E402
import test_gpu_llr_families as LF  # noqa: E402
import test_rm_host as RM  # noqa: E402
from dscf_model import dscf_model  # noqa: E402
from test_bp_early_stop_host import stop_points  # noqa: E402
from test_cascl_adaptive_host import FLAG_CRC_PASS, syndrome  # noqa: E402
from test_gpu_stoprule import _host_cut  # noqa: E402
from test_scan_host import scan_model  # noqa: E402
from test_scf_host import scf_model  # noqa: E402

FLAG_TIE, FLAG_RERANK, FLAG_BP_CONVERGED = 1, 4, 8
SIGMA = 10.0 ** (-1.5 / 20.0)
BY_NAME = {c.name: c for c in X.CASES}
_rows, _refs = {}, {}


def rows(width, y=False):
    """the seeded batch of a row width: LLRs 2 y / sigma / sigma of y = 1 + sigma z at 1.5 dB, rounded through float32 (y=True:
    the observations themselves, rounded through float32)"""
    if width not in _rows:
        z = np.random.default_rng(1500 + width).standard_normal((320, width))
        yy = 1.0 + SIGMA * z
        _rows[width] = (CC.f32_exact(2.0 * yy / SIGMA / SIGMA), CC.f32_exact(yy))
    for a in _rows[width]:
        a.setflags(write=False)
    return _rows[width][1 if y else 0]


def _cuda(x, shift=0):
    """a device copy of x; shift: it starts that many elements beyond an allocation's start"""
    import torch
    x = np.array(x, order="C")   # a writable copy: the cached rows are read-only
    flat = torch.empty(x.size + 4, dtype=torch.from_numpy(x[:0].reshape(-1)).dtype, device="cuda")
    t = flat[shift:shift + x.size].view(x.shape)
    t.copy_(torch.from_numpy(x))
    return t


def _frozen(N, io):
    f = np.ones(N, dtype=np.uint8)
    f[np.asarray(io)] = 0
    return f


class Ref:
    """inputs(B) -> dict(t={name: tensor}, f32=, sigma=, ...); want(B) -> {output name: array}; cmp: {name: f(got, want)}"""

    def __init__(self, inputs, full, cut=None, cmp=None):
        self.inputs, self._full, self._cut, self.cmp, self._memo = inputs, full, cut, cmp or {}, None

    def want(self, B):
        if self._cut is None:
            return self._full(B)
        if self._memo is None:
            self._memo = self._full()
            for a in self._memo.values():
                np.asarray(a).setflags(write=False)
        return {k: v[:B] for k, v in self._memo.items()}


def _words(u):
    return EM.pack(u)


# ---- the references, one builder per kind -----------------------------------------------------------------------------------
def _b_list(case, dec, oracle):
    """SC / SCL / CA-SCL through polar_decode_device or polar_time_decode_device against the oracle"""
    import polardecoding_amd as pa
    c, kw, op = case.ctx, case.ctx["kw"], case.opts
    N, K, taps, L, dt = c["N"], c["K"], kw.get("crc_taps"), kw.get("L", 1), kw.get("dtype", "f64")
    algo = c["kind"]
    Bm = max(case.batches)
    code = LF._code_of(oracle, dec, K, taps)
    sigma = SIGMA if op.get("from_y") else 0.0
    if "E" in kw:
        x_in = rows(kw["E"])
        llr = RM.recover(x_in[:Bm], N, dec.A, 0)
        assert dec.rm_mode != pa.RM_NONE and np.array_equal(dec.info_order, pa.rm_info_order(N, dec.A, kw["E"]))
    elif sigma:
        x_in = rows(N, y=True)
        llr = np.stack([oracle.llr_from_y(v, sigma) for v in x_in[:Bm]])
    else:
        x_in, llr = rows(N), rows(N)[:Bm]
    in32 = op.get("in_dtype") == "f32"

    def inputs(B):
        return dict(t={"in": _cuda(x_in[:B].astype(np.float32 if in32 else np.float64), op.get("shift", 0))}, f32=int(in32), sigma=sigma)

    def full():
        uh, pm, ties, st = LF._oracle(oracle, code, llr.astype(LF._np(dt)), algo, L=L, dtype=dt)
        fl = np.where(ties > 0, FLAG_TIE, 0)
        if taps:
            fl = fl | np.where(syndrome(uh, code.info_order, taps) == 0, FLAG_CRC_PASS, 0)
        if algo == "SC":
            pm, fl = np.zeros(Bm), np.zeros(Bm, dtype=np.int64)
        return {"d_uhat_bits": _words(uh), "d_pm": pm, "d_flags": fl.astype(np.uint32), "rerank": st[:, 0] > 0}

    def same_pm(g, w):
        return np.array_equal(g.astype(np.float32), w) if dt == "f32" else np.array_equal(g, w)

    return Ref(inputs, full, cut=True, cmp={"d_pm": same_pm, "d_flags": lambda g, w: np.array_equal(g & ~np.uint32(FLAG_RERANK), w)})


def _b_dyn(case, dec, oracle):
    """k_scl_dyn and k_scl_wide against dscl_model"""
    import polardecoding_amd as pa
    c = case.ctx
    N, K, L = c["N"], c["K"], c["kw"]["L"]
    io = dec.info_order
    dyn = pa.dyn_pac(N, pa.pac_info_order(N, K, "rm"), DM.G133) if c["kind"] == "PAC" else None
    x = rows(N)

    def full():
        u, pm, fl = DM.dscl_model(_frozen(N, io), dyn, x[:max(case.batches)], L, oracle=oracle)
        return {"d_uhat_bits": _words(u), "d_pm": pm, "d_flags": fl}
    return Ref(lambda B: dict(t={"in": _cuda(x[:B])}), full, cut=True)


def _b_q8(case, dec, oracle):
    c, kw = case.ctx, case.ctx["kw"]
    N, taps = c["N"], kw.get("crc_taps")
    io = dec.info_order
    q = QM.quantize(rows(N))

    def full():
        u, pm, fl = QM.decode_rows(q[:max(case.batches)], _frozen(N, io), kw.get("L", 1), crc=(io, taps) if taps else None, sc=c["kind"] == "SC")
        return {"d_uhat_bits": _words(u), "d_pm": pm, "d_flags": fl}
    return Ref(lambda B: dict(t={"in": _cuda(q[:B])}), full, cut=True)


def _b_quantise(case, dec, oracle):
    x = rows(case.ctx["N"])[:max(case.batches)]
    return Ref(lambda B: dict(t={"in": _cuda(x[:B])}), lambda: {"d_out": QM.quantize(x)}, cut=True)


def _code(case, dec, oracle):
    c = case.ctx
    code = oracle.Code(c["N"], c["K"], c["kw"].get("crc_taps"))
    assert np.array_equal(code.info_order, dec.info_order)
    return code


def _b_scf(case, dec, oracle):
    code, kw = _code(case, dec, oracle), case.ctx["kw"]
    x = rows(code.N)[:max(case.batches)]

    def full():
        if case.ref == "dscf":
            r = dscf_model(code, x, kw["budgets"], kw["c"], kw["tau"], oracle=oracle)
            u, fl, at, sets = r.u, r.flags, r.attempts, r.sets
        else:
            u, fl, at = scf_model(code, x, kw["T"], oracle=oracle)[:3]
            sets = np.zeros((len(u), 3))
        assert (at > 0).any() and (at == 0).any()   # flips ran, and some frames needed none
        return {"d_uhat_bits": _words(u), "d_flags": fl.astype(np.uint32), "d_attempts": at.astype(np.uint32),
                "d_sets": np.asarray(sets).astype(np.int32)}
    return Ref(lambda B: dict(t={"in": _cuda(x[:B])}), full, cut=True)


def _b_scan(case, dec, oracle):
    code = _code(case, dec, oracle)
    x = rows(code.N)[:max(case.batches)]

    def full():
        u, lu, ex = scan_model(code.frozen, x, case.ctx["kw"]["iters"], oracle=oracle, skip=True)
        return {"d_uhat_bits": _words(u), "d_llr_u": lu, "d_ext_x": ex}
    return Ref(lambda B: dict(t={"in": _cuda(x[:B])}), full, cut=True)   # soft outputs by value: == takes +inf and either zero


def _b_bp(case, dec, oracle):
    c, kw = case.ctx, case.ctx["kw"]
    code = LF._code_of(oracle, dec, c["K"], None)
    xa = rows(c["N"])
    x = xa[:max(case.batches)]
    it = kw["iterMax"]

    def full():
        if kw.get("early_stop"):
            t, conv, u = stop_points(x, code.frozen, it)
            fl = np.where(conv, FLAG_BP_CONVERGED, 0)
        else:
            u = oracle.decode(code, x, "BP", bp_iters=it)[0]
            t, fl = np.full(len(x), it), np.zeros(len(x), dtype=np.int64)
        return {"d_uhat_bits": _words(u), "d_iters": t.astype(np.uint32), "d_flags": fl.astype(np.uint32)}
    return Ref(lambda B: dict(t={"in": _cuda(xa[:B])}), full, cut=True)


def _b_readout(case, dec, oracle):
    c = case.ctx
    code = LF._code_of(oracle, dec, c["K"], None)
    x = rows(c["N"])
    cp = case.opts["checkpoints"]
    cps = np.asarray(cp, dtype=np.int32)

    def inputs(B):
        return dict(t={"in": _cuda(x[:B]), "u_bits": _cuda(np.zeros((B, c["N"] // 32), dtype=np.int32))},
                    cp=cps.ctypes.data_as(C.POINTER(C.c_int)), ncp=len(cp), keep=cps)

    def want(B):   # the sent word is the all-zero one; E is summed over the B frames of the call
        uh, E = oracle.bp_readout(code, x[:B], np.zeros((B, c["N"]), dtype=np.int32), c["kw"]["iterMax"], cp)
        return {"d_E": E.astype(np.uint64).reshape(-1), "d_uhat_bits": _words(uh)}
    return Ref(inputs, want)


def _b_bpl(case, dec, oracle):
    c, kw = case.ctx, case.ctx["kw"]
    code = _code(case, dec, oracle)
    P = min(code.n, 8)
    edge = case.opts.get("rows") == "compaction edge"   # tests/test_gpu_bpl.py: the one frame of the second block is an open one
    x = BT._edge_rows()[2] if edge else rows(c["N"])[:max(case.batches)]
    assert len(x) == max(case.batches)

    def full():
        r = BM.bpl_decode(x, code.frozen, code.info_order, BM.cyclic_graphs(code.n, P), kw["iterMax"], kw.get("crc_taps"))
        assert len(r.attempts) > 1 and len(r.attempts[1]["frames"]) >= 1   # frames are open after attempt 0
        if edge:   # graph 0, a later graph and none each decide frames, and the second compaction block has a frame to write
            assert min(BM.classes(r, P)) >= 1 and r.attempts[1]["frames"][-1] == X.AD_CHUNK
        return {"d_uhat_bits": _words(r.bits), "d_iters": r.iters.astype(np.uint32), "d_flags": r.flags.astype(np.uint32),
                "d_graph": r.graph.astype(np.uint32), "d_total_iters": r.total.astype(np.uint32)}
    return Ref(lambda B: dict(t={"in": _cuda(x[:B])}), full, cut=True)


def _b_adaptive(case, dec, oracle):
    code, kw = _code(case, dec, oracle), case.ctx["kw"]
    x = rows(code.N)[:max(case.batches)]

    def full():
        u, pm, fl, ls = AD._oracle_composition(oracle, code, kw["crc_taps"], kw["stages"], x)
        assert len(set(ls.tolist())) == len(kw["stages"])   # every stage decided some frame
        return {"d_uhat_bits": _words(u), "d_pm": pm, "d_flags": fl.astype(np.uint32), "d_list": ls.astype(np.uint32)}
    return Ref(lambda B: dict(t={"in": _cuda(x[:B])}), full, cut=True,
               cmp={"d_flags": lambda g, w: np.array_equal(g & ~np.uint32(FLAG_RERANK), w)})


def _b_recover(case, dec, oracle):
    c = case.ctx
    x = rows(c["kw"]["E"])[:max(case.batches)]
    return Ref(lambda B: dict(t={"in": _cuda(x[:B])}), lambda: {"d_out": RM.recover(x, c["N"], dec.A, 0)}, cut=True)


def _b_count(case, dec, oracle):
    N = case.ctx["N"]
    io = dec.info_order
    rng = np.random.default_rng(77)
    Bm = max(case.batches)
    u = rng.integers(0, 2, (Bm, N)).astype(np.uint8)
    uh = u ^ ((rng.random((Bm, N)) < 0.03) & (rng.random((Bm, 1)) < 0.6)).astype(np.uint8)
    a, b = (EM.transform(uh), EM.transform(u)) if case.ctx["kw"].get("sys_polar") else (uh, u)
    per = (a[:, io] != b[:, io]).sum(axis=1)
    assert (per[:3] != 0).any() and (per == 0).any()

    def want(B):
        return {"d_counters": np.array([(per[:B] != 0).sum(), per[:B].sum()], dtype=np.uint64), "d_frame_err": per[:B].astype(np.uint32)}
    return Ref(lambda B: dict(t={"uhat": _cuda(_words(uh[:B]).view(np.int32)), "u_bits": _cuda(_words(u[:B]).view(np.int32))}), want)


def _b_cut(case, dec, oracle):
    rng = np.random.default_rng(78)
    fe = ((rng.random(max(case.batches)) < 0.3) * rng.integers(1, 40, max(case.batches))).astype(np.uint32)
    fe[0] = 5
    return Ref(lambda B: dict(t={"in": _cuda(fe[:B].view(np.int32))}, need=2, min_frames=0),
               lambda B: {"d_out": np.array(_host_cut(fe[:B], 2), dtype=np.uint64)})


def _b_genie(case, dec, oracle):
    x = rows(case.ctx["N"])[:max(case.batches)]

    def want(B):
        err, tie, _, _ = GM.genie_model(oracle, x[:B])
        return {"d_counts": np.concatenate([err, tie]).astype(np.uint64)}
    return Ref(lambda B: dict(t={"in": _cuda(x[:B])}), want)


def _b_encode(case, dec, oracle):
    """transform, encode and payload against the models of tests/test_encode_host.py"""
    Bm, N, K = max(case.batches), dec.N, dec.K
    rng = np.random.default_rng(79 + N)
    v = rng.integers(0, 2, (Bm, K)).astype(np.uint8)
    w = EM.pack(v).copy()
    if K % 32:
        w[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(K % 32)   # garbage above bit K: it must be ignored
    u_any = rng.integers(0, 2, (Bm, N)).astype(np.uint8)
    want_u, want_x = GE._model(dec, None, v)
    if case.ref == "transform":
        return Ref(lambda B: dict(t={"in": _cuda(_words(u_any[:B]).view(np.int32))}), lambda: {"d_out": _words(EM.transform(u_any))}, cut=True)
    if case.ref == "encode":
        return Ref(lambda B: dict(t={"in": _cuda(w[:B].view(np.int32))}), lambda: {"d_u_bits": _words(want_u), "d_x_bits": _words(want_x)},
                   cut=True)
    return Ref(lambda B: dict(t={"in": _cuda(_words(want_u[:B]).view(np.int32))}),
               lambda: {"d_payload": EM.pack(v), "d_crc_ok": np.ones(Bm, dtype=np.uint32)}, cut=True)


BUILD = {"list": _b_list, "sc": _b_list, "rm": _b_list, "dyn": _b_dyn, "q8": _b_q8, "quantise": _b_quantise, "scf": _b_scf,
         "dscf": _b_scf, "scan": _b_scan, "bp": _b_bp, "readout": _b_readout, "bpl": _b_bpl, "adaptive": _b_adaptive,
         "recover": _b_recover, "count": _b_count, "cut": _b_cut, "genie": _b_genie, "transform": _b_encode, "encode": _b_encode,
         "payload": _b_encode}


def ref_of(case, dec, oracle):
    if case.name not in _refs:
        _refs[case.name] = BUILD[case.ref](case, dec, oracle)
    return _refs[case.name]


# ---- one call with its outputs in an arena ----------------------------------------------------------------------------------
def _std(p, i, B):
    return p("in"), i.get("f32", 0), float(i.get("sigma", 0.0)), B


def _rows_only(p, i, B):
    return p("in"), B


# entry point -> the arguments between the context and the output pointers (p(name): the device pointer of an input tensor)
BEFORE = {
    "polar_decode_device": _std, "polar_bp_decode_device": _std, "polar_cascl_decode_device": _std,
    "polar_scf_decode_device": _std, "polar_scf_decode_sets_device": _std, "polar_bpl_decode_device": _std,
    "polar_scan_decode_device": _std, "polar_q8_quantize_device": _std, "polar_genie_count_device": _std,
    "polar_rm_recover_device": _std, "polar_time_decode_device": _std,
    "polar_q8_decode_device": _rows_only, "polar_transform_device": _rows_only, "polar_encode_device": _rows_only,
    "polar_payload_device": _rows_only,
    "polar_bp_readout_device": lambda p, i, B: (p("in"), 0, 0.0, B, p("u_bits"), i["cp"], i["ncp"]),
    "polar_count_errors_device": lambda p, i, B: (p("uhat"), p("u_bits"), B),
    "polar_stop_rule_cut_device": lambda p, i, B: (p("in"), B, i["need"], i["min_frames"]),
    "polar_construct_batch": lambda p, i, B: (i["seed"], i["first"], i["sigma"], B),
}
# entry point -> the arguments behind the output pointers: polar_time_decode_device takes reps and a host float
AFTER = {"polar_time_decode_device": lambda: (1, C.byref(C.c_float(-1.0)))}


def _call(entry, dec, inp, B, ptrs):
    def p(k):
        return C.c_void_p(inp["t"][k].data_ptr())
    after = AFTER[entry]() if entry in AFTER else ()
    return getattr(dec._lib, entry)(dec._h, *BEFORE[entry](p, inp, B), *ptrs, *after)


def run(case, dec, B, inp, null=()):
    """one call of the case's entry point with every output (but those named in `null`) carved from a fresh arena; asserts
    the return code, the guards and the inputs; returns {output name: flat host array}"""
    import torch
    live = [o for o in case.outputs if o.name not in null]
    specs = {o.name: (o.dtype, X.elems(o, case.ctx, B), case.group, X.row_elems(o, case.ctx)) for o in live}
    arena = X.Arena("torch", X.Arena.need(specs.values()))
    views = {}
    for o in live:
        views[o.name] = arena.carve(o.name, *specs[o.name])
        assert views[o.name].data_ptr() % 16 == np.dtype(o.dtype).itemsize % 16
        if o.acc:
            views[o.name].zero_()
    snaps = {k: X.snapshot(t) for k, t in inp["t"].items()}
    torch.cuda.synchronize()   # torch's fills and copies are done before the ctx stream runs
    ptrs = [C.c_void_p(views[o.name].data_ptr()) if o.name in views else None for o in case.outputs]
    rc = _call(case.entry, dec, inp, B, ptrs)
    dec.synchronize()
    torch.cuda.synchronize()
    assert rc == 0, (case.name, B, null, rc, dec._lib.polar_last_error(dec._h).decode())
    assert arena.check() == [], (case.name, B, null)
    for k, t in inp["t"].items():
        assert X.unchanged(t, snaps[k]), (case.name, B, f"input {k} was written")
    return {o.name: views[o.name].cpu().numpy().view(np.dtype(o.dtype)) for o in live}


def _null_sets(case):
    nullable = [o.name for o in case.outputs if o.nullable]
    sets = [(n,) for n in nullable]
    if len(nullable) > 1 and not case.opts.get("not_all_null"):
        sets.append(tuple(nullable))
    return sets


PAIRS = [(c, B) for c in X.CASES for B in c.batches]


@pytest.mark.parametrize("case,B", PAIRS, ids=[f"{c.name}-B{B}" for c, B in PAIRS])
def test_outputs_stay_inside_their_extents(case, B, oracle):
    from polardecoding_amd import testing as T
    dec = X.make_ctx(case.ctx)
    try:
        if case.opts.get("cap"):
            T.chunk_bytes(dec, case.opts["cap"])
        # the name belongs to the context, not to the launch: polar_kernel_name() names the family chosen for a batch of 64,
        # so below 64 frames k_sc_lanes contexts (SC, stage 0 of the adaptive rule) launch the kernel their name gives second
        assert dec.kernel_name.startswith(case.prefix), dec.kernel_name
        ref = ref_of(case, dec, oracle)
        inp = ref.inputs(B)
        if case.opts.get("shift"):
            assert inp["t"]["in"].data_ptr() % 16 != 0
        got = run(case, dec, B, inp)
        want = ref.want(B)
        for o in case.outputs:
            g, w = got[o.name], np.asarray(want[o.name])
            g = g.reshape(w.shape)
            same = ref.cmp.get(o.name, np.array_equal)(g, w)
            assert same, (case.name, B, o.name, np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:8])
        if "rerank" in want and case.ctx["kw"].get("dtype", "f64") == "f64" and "d_flags" in got:   # as tests/test_gpu_llr_families.py
            rr = (got["d_flags"] & FLAG_RERANK) != 0
            assert not rr.any() if "k_scl_generic" in dec.kernel_name or case.ref != "list" else np.array_equal(rr, want["rerank"])
        for null in _null_sets(case):
            again = run(case, dec, B, inp, null=null)
            for name, a in again.items():
                assert np.array_equal(a, got[name]), (case.name, B, "null:", null, name)
    finally:
        dec.close()


# ---- the chunked host loops across a pass boundary ---------------------------------------------------------------------------
def _ragged(loop):
    return next(c for c in CC.CASES if c.loop == loop and c.kind == "ragged")


def _loop(loop, oracle):
    """(context, entry point, outputs, rows or None, cap, extra inputs) of the first ragged case of a loop in tests/chunk_cases.py"""
    import polardecoding_amd as pa
    case = _ragged(loop)
    if loop == "q8":
        return CT._q8_dec(case.spec[0]), "polar_decode_device", X.LIST3, CC.q8_rows("gauss"), case.cap
    if loop == "rm":
        E, ibil = case.spec[:2]
        return pa.SCLdecode(CC.RM_N, CC.RM_K, L=8, E=E, ibil=ibil), "polar_decode_device", X.LIST3, CC.rm_rows(E), case.cap
    if loop == "adaptive":
        dec = pa.CASCL(CC.AD_N, CC.AD_K, L=CC.AD_STAGES[-1], crc_taps=X.CRC6, stages=CC.AD_STAGES)
        return dec, "polar_cascl_decode_device", BY_NAME["adaptive (1,2,8) N=128"].outputs, CC.ad_rows(oracle, "ragged"), case.cap
    if loop == "scf":
        dec = pa.SCFlip(CC.SCF_N, CC.SCF_K, T=case.spec[0], crc_taps=X.CRC6)
        return dec, "polar_scf_decode_device", X.SCF3, CC.scf_rows(oracle, case), case.cap
    if loop == "dscf":
        N, budgets, c = case.spec[:3]
        K, taps, _, _ = CT.DS.SHAPE[N]
        dec = pa.DSCFlip(N, K, budgets=budgets, c=c, tau=CC.TAU, crc_taps=taps)
        return dec, "polar_scf_decode_sets_device", BY_NAME["dscf (4,4,4) N=128"].outputs, CC.dscf_rows(oracle, case), case.cap
    if loop == "bpl":
        N, K, iters = case.spec[:3]
        return pa.BPL(N, K, iterMax=iters), "polar_bpl_decode_device", BY_NAME["bpl N=128"].outputs, CC.bpl_rows(oracle, case), case.cap
    assert loop == "construct"
    N = case.spec[0]
    return pa.SCdecode(N, N // 2), "polar_construct_batch", BY_NAME["genie count N=128"].outputs, None, case.cap


@pytest.mark.parametrize("loop", ["q8", "rm", "adaptive", "scf", "dscf", "bpl", "construct"])
def test_chunked_loops(loop, oracle):
    """the capped run (three passes and more, a partial last one) writes what the uncapped run writes and nothing else"""
    from polardecoding_amd import testing as T
    dec, entry, outputs, x, cap = _loop(loop, oracle)
    try:
        width = dec.E if x is not None else dec.N
        case = X.Case(f"chunked {loop}", entry, X.ctx("", dec.N, dec.K, E=width), "", CC.ROW_FLOOR, (), outputs, "", {})
        B = len(x) if x is not None else CC.B_RAGGED
        inp = dict(t={"in": _cuda(x)}) if x is not None else dict(t={}, seed=77, first=5_000_000_000, sigma=0.9)
        T.chunk_bytes(dec, 0)
        plain = run(case, dec, B, inp)
        T.chunk_bytes(dec, cap)
        capped = run(case, dec, B, inp)
        for name, a in capped.items():
            assert np.array_equal(a, plain[name]), (loop, name)
        assert any(a.any() for a in plain.values())
    finally:
        dec.close()


# ---- the host-buffer forms: outputs in a numpy arena, == the device form ---------------------------------------------------------
def _host_views(B, spec):
    """spec: [(name, dtype, elements per frame)] -> (numpy arena, {name: view}), the guards sized for 64 rows"""
    specs = [(dt, per * B, 64, per) for _, dt, per in spec]
    arena = X.Arena("numpy", X.Arena.need(specs))
    return arena, {name: arena.carve(name, *s) for (name, _, _), s in zip(spec, specs)}


def _cast(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


def _as_arg(fn, k, a):
    """a numpy array as argument k of a bound library function (its declared pointer type)"""
    return C.cast(C.c_void_p(a.ctypes.data), fn.argtypes[k])


def _device(name, B, oracle, dec):
    case = BY_NAME[name]
    inp = ref_of(case, dec, oracle).inputs(B)
    return case, inp, run(case, dec, B, inp)


def _bits(words, B, n):
    return EM.unpack(np.ascontiguousarray(words).reshape(B, -1), n).astype(np.int32)


UHAT = ("u_hat", "int32", "N", "d_uhat_bits")
H_PM, H_FLAGS = ("pm", "float64", 1, "d_pm"), ("flags", "uint32", 1, "d_flags")
# host entry point -> (device case, arguments between the input rows and B, outputs as (name, dtype, per frame, device output))
# every one is f(ctx, rows, [extra], B, outputs...)
HOST = {
    "polar_decode_batch": ("fast N=128", (None,), [UHAT, H_PM, H_FLAGS]),                 # no frozen_mask override
    "polar_decode_batch_y": ("fast2_y CASCL f64", (SIGMA,), [UHAT, H_PM, H_FLAGS]),
    "polar_bp_decode_batch": ("k_bp_w128 N=128 stop g", (), [UHAT, ("iters", "uint32", 1, "d_iters"), H_FLAGS]),
    "polar_cascl_decode_batch": ("adaptive (1,2,8) N=128", (), [UHAT, H_PM, H_FLAGS, ("list", "uint32", 1, "d_list")]),
    "polar_scf_decode_batch": ("scf T=8 N=128", (), [UHAT, H_FLAGS, ("attempts", "uint32", 1, "d_attempts")]),
    "polar_scf_decode_sets_batch": ("dscf (4,4,4) N=128", (), [UHAT, H_FLAGS, ("attempts", "uint32", 1, "d_attempts"),
                                                               ("sets", "int32", 3, "d_sets")]),
    "polar_scan_decode_batch": ("scan N=128 I=2", (), [UHAT, ("llr_u", "float64", "N", "d_llr_u"), ("ext_x", "float64", "N", "d_ext_x")]),
    "polar_bpl_decode_batch": ("bpl N=128", (), [UHAT, ("iters", "uint32", 1, "d_iters"), H_FLAGS, ("graph", "uint32", 1, "d_graph"),
                                                 ("total_iters", "uint32", 1, "d_total_iters")]),
    "polar_q8_decode_batch": ("q8 CASCL N=64 L=8", (), [UHAT, ("pm", "int32", 1, "d_pm"), H_FLAGS]),
}
# the host entry points with a test of their own below
HOST_BY_HAND = {
    "polar_decode": "test_single_frame_host_forms", "polar_decode_llr": "test_single_frame_host_forms",
    "polar_encode_batch": "test_encoder_side_host_forms", "polar_payload_batch": "test_encoder_side_host_forms",
    "polar_bp_readout_batch": "test_bp_readout_host_form",
}


def _host_call(entry, dec, x, extra, B, views):
    fn = getattr(dec._lib, entry)
    k = 2 + len(extra) + 1   # ctx, rows, extra, B
    return fn(dec._h, _as_arg(fn, 1, x), *extra, B, *[_as_arg(fn, k + j, v) for j, v in enumerate(views)])


@pytest.mark.parametrize("B", X.HOST_BATCHES)
@pytest.mark.parametrize("entry", list(HOST))
def test_host_buffer_forms(entry, B, oracle):
    name, extra, spec = HOST[entry]
    case = BY_NAME[name]
    assert X.HOST_CASES[entry] == case.entry
    dec = X.make_ctx(case.ctx)
    try:
        _, inp, dev = _device(name, B, oracle, dec)
        x = np.ascontiguousarray(inp["t"]["in"].cpu().numpy())
        snap = X.snapshot(x)
        d = X.dims(case.ctx)
        arena, views = _host_views(B, [(n, dt, per if isinstance(per, int) else d[per]) for n, dt, per, _ in spec])
        rc = _host_call(entry, dec, x, extra, B, list(views.values()))
        assert rc == 0, (entry, B, rc)
        assert arena.check() == [] and X.unchanged(x, snap), (entry, B)
        for n, dt, per, dname in spec:
            want = _bits(dev[dname], B, case.ctx["N"]).reshape(-1) if n == "u_hat" else dev[dname]
            assert views[n].dtype == want.dtype and np.array_equal(views[n], want), (entry, B, n)
    finally:
        dec.close()


@pytest.mark.parametrize("B", X.HOST_BATCHES)
def test_single_frame_host_forms(B, oracle):
    """polar_decode (y and sigma) and polar_decode_llr (LLRs and a frozen mask), frame by frame into one arena"""
    import polardecoding_amd as pa
    case = BY_NAME["fast2_y CASCL f64"]
    dec = X.make_ctx(case.ctx)
    try:
        _, inp, dev = _device(case.name, B, oracle, dec)
        y = np.ascontiguousarray(inp["t"]["in"].cpu().numpy())
        snap = X.snapshot(y)
        arena, views = _host_views(B, [("u_hat", "int32", dec.N)])
        uh = views["u_hat"].reshape(B, dec.N)
        for b in range(B):
            assert dec._lib.polar_decode(dec._h, _cast(y[b], C.c_double), SIGMA, _cast(uh[b], C.c_int)) == 0
        assert arena.check() == [] and X.unchanged(y, snap)
        assert np.array_equal(uh, _bits(dev["d_uhat_bits"], B, dec.N))
    finally:
        dec.close()
    case = BY_NAME["generic N=64 L=8"]
    dec = X.make_ctx(case.ctx)
    try:
        _, inp, dev = _device(case.name, B, oracle, dec)
        x = np.ascontiguousarray(inp["t"]["in"].cpu().numpy())
        mask = _frozen(dec.N, dec.info_order)
        snap, msnap = X.snapshot(x), X.snapshot(mask)
        arena, views = _host_views(B, [("u_hat", "int32", dec.N)])
        uh = views["u_hat"].reshape(B, dec.N)
        lib = pa.load_library()
        for b in range(B):
            assert lib.polar_decode_llr(_cast(x[b], C.c_double), _cast(mask, C.c_ubyte), dec.N, 8, _cast(uh[b], C.c_int)) == 0
        assert arena.check() == [] and X.unchanged(x, snap) and X.unchanged(mask, msnap)
        assert np.array_equal(uh, _bits(dev["d_uhat_bits"], B, dec.N))
    finally:
        dec.close()


HOST_CHUNK = 16384   # host_batch() of csrc/polar_hip.hip: frames per chunk while a chunk's rows stay below 128 MiB


@pytest.mark.parametrize("B", [2049, HOST_CHUNK + 1, 6 * HOST_CHUNK + 1])
def test_decode_batch_across_the_chunks_of_the_host_pipeline(B, oracle):
    """polar_decode_batch cuts a batch into chunks and computes the copy-back and the unpacking per chunk (u_hat + (f0 + f) N,
    pm + f0, nf NW words).  At N = 32 a chunk takes 16384 frames: B = 2049 is one chunk; B = 16385 makes two, the second of one
    frame; from 6 x 16384 frames on the chunks ramp (2048, 4096, 8192, 16384 ..., 8192, 4096, 2048) and are staged through
    pinned buffers, so B = 98305 makes eleven, the first of 2048 frames and a ragged one of 4097 in the middle."""
    N = 32
    case = X.Case("host N=32", "polar_decode_device", X.ctx("SCL", N, 16, L=2), "", 64, (B,), X.LIST3, "", {})
    dec = X.make_ctx(case.ctx)
    try:
        rng = np.random.default_rng(1532)   # a random word per frame, so that a frame written to another's place shows
        u = np.zeros((B, N), dtype=np.uint8)
        u[:, dec.info_order] = rng.integers(0, 2, (B, dec.A))
        x = CC.f32_exact(2.0 * ((1.0 - 2.0 * EM.transform(u)) + SIGMA * rng.standard_normal((B, N))) / SIGMA / SIGMA)
        dev = run(case, dec, B, dict(t={"in": _cuda(x)}))
        u_dev = _bits(dev["d_uhat_bits"], B, N)
        edges = {2049: [], HOST_CHUNK + 1: [HOST_CHUNK],
                 6 * HOST_CHUNK + 1: [2048, 6144, 14336, 30720, 47104, 63488, 79872, 83969, 92161, 96257]}[B]   # first frame of each later chunk
        assert all((u_dev[b - 1] != u_dev[b]).any() for b in edges)   # the frames on both sides of a boundary differ
        snap = X.snapshot(x)
        arena, views = _host_views(B, [("u_hat", "int32", N), ("pm_out", "float64", 1), ("flags", "uint32", 1)])
        rc = _host_call("polar_decode_batch", dec, x, (None,), B, list(views.values()))
        assert rc == 0 and arena.check() == [] and X.unchanged(x, snap)
        bad = np.flatnonzero((views["u_hat"].reshape(B, N) != u_dev).any(axis=1))
        assert bad.size == 0, f"u_hat differs from frame {bad[0]} on ({bad.size} frames)"
        assert np.array_equal(views["pm_out"], dev["d_pm"]) and np.array_equal(views["flags"], dev["d_flags"])
    finally:
        dec.close()


def test_scf_sets_batch_across_the_chunks_of_the_host_pipeline(oracle):
    """polar_scf_decode_sets_batch at 16385 frames of N = 32 (two host chunks, the second of one frame): `sets` is the one
    output of the host pipeline whose rows are wider than a word (3 positions per frame), so its slice per chunk and its
    copy-back are held to the device form on the same rows here.  Dynamic SC-Flip (4, 4, 4) on random valid codewords at
    Eb/N0 = 3 dB, where a minority of the frames reports a set and the case takes well under a second; the last frame, alone
    in the second chunk, is one whose reported set is not empty."""
    N, K, B = 32, 16, HOST_CHUNK + 1
    sigma = 10.0 ** (-3.0 / 20.0)
    case = X.Case("host dscf N=32", "polar_scf_decode_sets_device",
                  X.ctx("DSCF", N, K, budgets=(4, 4, 4), c=1.5, tau=5.0, crc_taps=X.CRC6), "", 64, (B,),
                  BY_NAME["dscf (4,4,4) N=128"].outputs, "", {})
    dec = X.make_ctx(case.ctx)
    try:
        io = dec.info_order.tolist()
        code = oracle.Code(N, K, X.CRC6, Q=[j for j in range(N) if j not in set(io)] + io)
        assert np.array_equal(code.info_order, dec.info_order)
        basis, _ = oracle.Sim(1533).frames(code, sigma, 32)   # valid words u; the code and its CRC are linear, so are their sums
        rng = np.random.default_rng(1533)
        u = ((rng.integers(0, 2, (B, 32)) @ np.asarray(basis, dtype=np.int64)) & 1).astype(np.uint8)
        x = CC.f32_exact(2.0 * ((1.0 - 2.0 * EM.transform(u)) + sigma * rng.standard_normal((B, N))) / sigma / sigma)
        sets = run(case, dec, B, dict(t={"in": _cuda(x)}))["d_sets"].reshape(B, 3)
        assert (sets[:, 0] >= 0).any(), "no frame flipped"
        j = int(np.flatnonzero(sets[:, 0] >= 0)[0])
        x[[j, B - 1]] = x[[B - 1, j]]   # a frame that flips goes last: the only frame of the second chunk
        dev = run(case, dec, B, dict(t={"in": _cuda(x)}))
        sets = dev["d_sets"].reshape(B, 3)
        assert sets[B - 1, 0] >= 0 and (sets[:HOST_CHUNK, 0] >= 0).any() and (sets[:HOST_CHUNK, 0] < 0).any()
        snap = X.snapshot(x)
        arena, views = _host_views(B, [("u_hat", "int32", N), ("flags", "uint32", 1), ("attempts", "uint32", 1), ("sets", "int32", 3)])
        rc = _host_call("polar_scf_decode_sets_batch", dec, x, (), B, list(views.values()))
        assert rc == 0 and arena.check() == [] and X.unchanged(x, snap)
        bad = np.flatnonzero((views["u_hat"].reshape(B, N) != _bits(dev["d_uhat_bits"], B, N)).any(axis=1))
        assert bad.size == 0, f"u_hat differs from frame {bad[0]} on ({bad.size} frames)"
        for n, dname in (("flags", "d_flags"), ("attempts", "d_attempts"), ("sets", "d_sets")):
            assert views[n].dtype == dev[dname].dtype and np.array_equal(views[n], dev[dname]), n
    finally:
        dec.close()


@pytest.mark.parametrize("B", X.HOST_BATCHES)
def test_encoder_side_host_forms(B, oracle):
    """polar_encode_batch (u only, x only, both) and polar_payload_batch at N = 32 against the device forms"""
    enc, pay = BY_NAME["encode N=32"], BY_NAME["payload N=32"]
    dec = X.make_ctx(enc.ctx)
    try:
        N, K = dec.N, dec.K
        _, inp, dev = _device(enc.name, B, oracle, dec)
        v = EM.unpack(inp["t"]["in"].cpu().numpy().view(np.uint32), K).astype(np.int32)
        v = np.ascontiguousarray(v)
        snap = X.snapshot(v)
        want_u, want_x = _bits(dev["d_u_bits"], B, N), _bits(dev["d_x_bits"], B, N)
        for use in (("u", "x"), ("u",), ("x",)):
            arena, views = _host_views(B, [(n, "int32", N) for n in use])
            rc = dec._lib.polar_encode_batch(dec._h, _cast(v, C.c_int), B, _cast(views["u"], C.c_int) if "u" in use else None,
                                             _cast(views["x"], C.c_int) if "x" in use else None)
            assert rc == 0 and arena.check() == [] and X.unchanged(v, snap), use
            for n in use:
                assert np.array_equal(views[n].reshape(B, N), want_u if n == "u" else want_x), (use, n)
        _, pinp, pdev = _device(pay.name, B, oracle, dec)
        uh = np.ascontiguousarray(_bits(pinp["t"]["in"].cpu().numpy().view(np.uint32), B, N))
        snap = X.snapshot(uh)
        for with_ok in (True, False):
            arena, views = _host_views(B, [("payload", "int32", K)] + ([("crc_ok", "uint32", 1)] if with_ok else []))
            rc = dec._lib.polar_payload_batch(dec._h, _cast(uh, C.c_int), B, _cast(views["payload"], C.c_int),
                                              _cast(views["crc_ok"], C.c_uint) if with_ok else None)
            assert rc == 0 and arena.check() == [] and X.unchanged(uh, snap)
            assert np.array_equal(views["payload"].reshape(B, K), EM.unpack(pdev["d_payload"].reshape(B, -1), K))
            if with_ok:
                assert np.array_equal(views["crc_ok"], pdev["d_crc_ok"])
    finally:
        dec.close()


@pytest.mark.parametrize("B", X.HOST_BATCHES)
def test_bp_readout_host_form(B, oracle):
    case = BY_NAME["bp readout N=128"]
    dec = X.make_ctx(case.ctx)
    try:
        N, n = dec.N, dec.N.bit_length() - 1
        _, inp, dev = _device(case.name, B, oracle, dec)
        x = np.ascontiguousarray(inp["t"]["in"].cpu().numpy())
        u = np.zeros((B, N), dtype=np.int32)
        snap, usnap = X.snapshot(x), X.snapshot(u)
        for with_uhat in (True, False):
            specs = [("uint64", inp["ncp"] * (n + 1), 1, 1)] + ([("int32", B * N, 64, N)] if with_uhat else [])
            arena = X.Arena("numpy", X.Arena.need(specs))
            E = arena.carve("E", *specs[0])
            E[...] = 0   # the call adds
            uh = arena.carve("u_hat", *specs[1]) if with_uhat else None
            rc = dec._lib.polar_bp_readout_batch(dec._h, _cast(x, C.c_double), 0.0, B, _cast(u, C.c_int), inp["cp"], inp["ncp"],
                                                 _cast(E, C.c_ulonglong), _cast(uh, C.c_int) if with_uhat else None)
            assert rc == 0 and arena.check() == [] and X.unchanged(x, snap) and X.unchanged(u, usnap)
            assert np.array_equal(E, dev["d_E"])
            if with_uhat:
                assert np.array_equal(uh.reshape(B, N), _bits(dev["d_uhat_bits"], B, N))
    finally:
        dec.close()
