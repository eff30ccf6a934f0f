"""GPU: a reused, reconfigured context against a freshly created one (the scripts of tests/ctx_sequences.py).

One test per script and library.  The script runs on ONE context; at every observation a fresh context is built from the
recipe (the constructor plus the final value of every setting, no history), runs the same call once and is closed, and every
output of the two calls is compared byte for byte: packed decisions, path metrics as bit patterns, flags, iters / list_size /
attempts / sets / graph / total_iters, soft outputs with their infinities, counters, kernel_name, and in the testing library
the launch plan.  No tolerance exists anywhere in this file.

The anchor: the first observation after the script's last change (the first one where a script has no change) is also held
to the CPU model that the decoder's feature test uses (ctx_sequences.model), on its first ANCHOR_CAP frames, so that the
reused and the fresh context cannot both be wrong in the same way unnoticed.

Changes without a CPU model (kernel selection, the cap on the resident grid, stream switches) leave the outputs as they
were; there the test asserts that the change was in effect: kernel_name moved, the launch plan shows the capped grid and the
work queue, polar_get_stream returns the torch stream's handle.

In the shipped library a script runs without its hook changes (Script.without_hooks); every other step is the same.
Every device call is followed by dec.synchronize() before the read-back; before a call, torch.cuda.synchronize() so that
torch's fills are done before the context's stream reads them."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctx_sequences as S  # noqa: E402

pytestmark = pytest.mark.gpu

ANCHOR_CAP = 48
NAN = float("nan")
PLAN_ENTRIES = ("decode_device", "decode_cascl_device", "decode_bp_device", "decode_scf_device", "decode_scf_sets_device",
                "decode_scan_device", "decode_bpl_device", "decode_q8_device")   # their last launch plan is their own


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _pack(bits):
    b = np.asarray(bits, dtype=np.uint8)
    return np.packbits(b, axis=1, bitorder="little").view(np.uint32).view(np.int32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _full(shape, fill, dtype):
    import torch
    return torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device="cuda")


def _np(t):
    return t.cpu().numpy()


def _library(which):
    import polardecoding_amd as pa
    return pa.load_library(testing=(which == "testing"))


def _create(script, which):
    import polardecoding_amd as pa
    kw = dict(script.kw)
    if kw.get("dtype") == "Q8":
        kw["dtype"] = pa.Q8
    return getattr(pa, script.ctor)(*script.args, _library=_library(which), **kw)


def _change(dec, chg, streams):
    """one change on a live context"""
    import torch
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    what, v = chg
    if what in S.HOOKS:
        getattr(T, what)(dec, v)
    elif what == "stream":
        with torch.cuda.stream(streams[v]):
            dec.use_torch_stream()
    elif what == "sys_polar":
        dec.set_systematic(v)
    elif what == "stages":
        dec.set_cascl_stages(v)
    elif what == "bp_stop":
        dec.set_bp_stop(v)
    elif what == "scf_flips":
        dec.set_scf_flips(v)
    elif what == "scf_dynamic":
        dec.set_scf_dynamic(*v) if v is not None else dec.set_scf_dynamic(None)
    elif what == "scan_iters":
        dec.set_scan_iters(v)
    elif what == "bpl_graphs":
        n = dec.N.bit_length() - 1
        dec.set_bpl_graphs(pa.bpl_cyclic_graphs(n, v if v is not None else min(n, 8)))
    elif what == "quant":
        dec.set_quant(*v)
    else:
        assert what == "frozen_mask", what   # per call: the next polar_decode_batch takes it


def _fresh(script, settings, which, streams):
    dec = _create(script, which)
    for chg in S.recipe(settings):
        _change(dec, chg, streams)
    return dec


# ---- the entries: one call (or a short chain) with all of its outputs ----------------------------------------------------------
def _run(dec, script, w, x):
    """observation w.step on dec with the inputs x -> {name: numpy array}; the names are ctx_sequences.OUTPUTS"""
    import torch
    import polardecoding_amd as pa
    ob, st = w.step, w.settings
    e, B, N, NW = ob.entry, ob.B, dec.N, dec.NW
    i32, f64 = torch.int32, torch.float64
    seed, first = script.seed, 1000 * w.nobs
    host = {"decode_batch": lambda: dec.decode_batch(x.llr, frozen_mask=script.masks[st["frozen_mask"]] if st["frozen_mask"] else None),
            "decode_batch_y": lambda: dec.decode_batch_y(x.y, x.sigma),
            "decode": lambda: (dec(x.y[0], x.sigma).reshape(1, N),),
            "stop_rule_batch_y": lambda: tuple(np.asarray([v]) for v in dec.stop_rule_batch_y(x.y, x.sigma, x.u, 2)),
            "fer_batch": lambda: tuple(np.asarray([v]) for v in dec.fer_batch(seed, first, script.db, B)),
            "decode_bp_batch": lambda: dec.decode_bp_batch(x.llr),
            "decode_scf_batch": lambda: dec.decode_scf_batch(x.llr),
            "decode_scf_sets_batch": lambda: dec.decode_scf_sets_batch(x.llr),
            "decode_scan_batch": lambda: dec.decode_scan_batch(x.llr),
            "decode_bpl_batch": lambda: dec.decode_bpl_batch(x.llr),
            "encode_batch": lambda: dec.encode_batch(np.random.default_rng(seed + w.nobs).integers(0, 2, (B, dec.K)))}
    if e in host:
        return dict(zip(S.outputs_of(ob), (np.asarray(v) for v in host[e]())))

    def call(fn, *outs):
        """torch's fills first, then the call on the context's stream, then its synchronize()"""
        torch.cuda.synchronize()
        r = fn()
        dec.synchronize()
        return r

    d = _dev(x.llr) if e not in S.GENERATED and e not in ("encode_payload",) else None
    fl, it = _full(B, -1, i32), _full(B, -1, i32)
    if e == "decode_device":
        pm = _full(B, NAN, f64)
        bits = call(lambda: dec.decode_device(d, pm=pm, flags=fl))
        return {"uh": _unpack(_np(bits), N), "pm": _np(pm), "flags": _np(fl)}
    if e == "decode_cascl_device":
        pm, ls = _full(B, NAN, f64), _full(B, -1, i32)
        bits = call(lambda: dec.decode_cascl_device(d, pm=pm, flags=fl, list_size=ls))
        return {"uh": _unpack(_np(bits), N), "pm": _np(pm), "flags": _np(fl), "list_size": _np(ls)}
    if e == "decode_bp_device":
        bits = call(lambda: dec.decode_bp_device(d, iters=it, flags=fl))
        return {"uh": _unpack(_np(bits), N), "iters": _np(it), "flags": _np(fl)}
    if e == "bp_readout":
        cp = (3, 6, 12)
        E, out, ub = _full((len(cp), N.bit_length()), 0, torch.int64), _full((B, NW), 0, i32), _dev(_pack(x.u))
        try:
            call(lambda: dec.bp_readout_device(d, ub, cp, E, out_bits=out))
            refused = 0
        except pa.PolarError:
            refused = 1
        return {"refused": np.asarray([refused]), "E": _np(E), "uh": _unpack(_np(out), N)}
    if e in ("decode_scf_device", "decode_scf_sets_device"):
        if e == "decode_scf_device":
            bits = call(lambda: dec.decode_scf_device(d, flags=fl, attempts=it))
            return {"uh": _unpack(_np(bits), N), "flags": _np(fl), "attempts": _np(it)}
        sets = _full((B, 3), -7, i32)
        bits = call(lambda: dec.decode_scf_sets_device(d, flags=fl, attempts=it, sets=sets))
        return {"uh": _unpack(_np(bits), N), "flags": _np(fl), "attempts": _np(it), "sets": _np(sets)}
    if e == "decode_scan_device":
        soft = ob.opt["soft"]
        lu = _full((B, N), NAN, f64) if soft else None
        ex = _full((B, N), NAN, f64) if soft else None
        bits = call(lambda: dec.decode_scan_device(d, llr_u=lu, ext_x=ex))
        out = {"uh": _unpack(_np(bits), N)}
        return dict(out, llr_u=_np(lu), ext_x=_np(ex)) if soft else out
    if e == "decode_bpl_device":
        gr, tot = _full(B, -1, i32), _full(B, -1, i32)
        bits = call(lambda: dec.decode_bpl_device(d, iters=it, flags=fl, graph=gr, total_iters=tot))
        return {"uh": _unpack(_np(bits), N), "iters": _np(it), "flags": _np(fl), "graph": _np(gr), "total_iters": _np(tot)}
    if e == "decode_q8_device":
        q = _dev(pa.q8_quantize(x.llr, *S.DEFAULTS["quant"][:2]))   # quantised under the quantiser the context was created with
        pm = _full(B, -7, i32)
        bits = call(lambda: dec.decode_q8_device(q, pm=pm, flags=fl))
        return {"uh": _unpack(_np(bits), N), "pm": _np(pm), "flags": _np(fl)}
    if e == "rm_recover":
        out = _full((B, N), NAN, f64)
        call(lambda: dec.rm_recover_device(d, out=out))
        return {"rows": _np(out)}
    if e == "list_decode":
        masks = _dev(np.asarray([0, 1, 5], dtype=np.int32))
        paths, pm, rem, count, flags = call(lambda: dec.decode_list_device(d))
        idx = call(lambda: dec.list_select_device(rem, count, masks))
        got = call(lambda: dec.list_gather_device(paths, idx[:, 0]))
        paths, pm, rem, count = _np(paths), _np(pm), _np(rem), _np(count)
        dead = np.arange(dec.L)[None, :] >= count[:, None]   # ranks behind the live paths are not written
        paths[dead], pm[dead], rem[dead] = 0, 0.0, 0
        return {"paths": paths, "pm": pm, "rem": rem, "count": count, "flags": _np(flags), "idx": _np(idx), "gathered": _np(got)}
    if e == "construct_batch":
        counts = _full((2, N), 0, torch.int64)
        call(lambda: dec.construct_batch(seed, first, x.sigma, B, counts))
        return {"counts": _np(counts)}
    if e == "generate_count":
        llr, ub = _full((B, script.W), NAN, f64), _full((B, NW), -1, i32)
        cnt, fe = _full(2, 0, torch.int64), _full(B, -1, i32)
        call(lambda: dec.generate_device(seed, first, script.db, llr, ub))
        bits = call(lambda: dec.decode_device(llr))
        call(lambda: dec.count_errors_device(bits, ub, cnt, frame_err=fe))
        return {"llr": _np(llr), "u_bits": _np(ub), "uh": _unpack(_np(bits), N), "counters": _np(cnt), "frame_err": _np(fe)}
    if e == "encode_payload":
        KW = (dec.K + 31) // 32
        bits = np.random.default_rng(seed + w.nobs).integers(0, 2, (B, KW * 32), dtype=np.uint8)
        bits[:, dec.K:] = 0
        u, xx = call(lambda: dec.encode_device(_dev(_pack(bits))))
        pay, ok = call(lambda: dec.payload_device(u))
        return {"u": _np(u), "x": _np(xx), "payload": _np(pay), "crc_ok": _np(ok)}
    raise KeyError(e)


def _observe(dec, script, w, x, which):
    out = _run(dec, script, w, x)
    assert tuple(out) == S.outputs_of(w.step), (w.step.entry, tuple(out))
    out["kernel_name"] = np.frombuffer(dec.kernel_name.encode(), dtype=np.uint8)
    if which == "testing" and w.step.entry in PLAN_ENTRIES:
        from polardecoding_amd import testing as T
        out["plan"] = np.asarray(T.last_plan(dec))
    return out


def _same(reused, fresh, where):
    assert list(reused) == list(fresh), where
    for k in reused:
        a, b = np.ascontiguousarray(reused[k]), np.ascontiguousarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (where, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            if k == "kernel_name":
                raise AssertionError(f"{where}: kernel_name {a.tobytes().decode()!r} on the reused context, {b.tobytes().decode()!r} on the fresh one")
            rows = np.flatnonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))
            raise AssertionError(f"{where}: output {k!r} of the reused context differs from the fresh one's at {rows.size} of {len(a)} "
                                 f"rows, first {rows[:8].tolist()}")


def _anchor(script, w, x, out, oracle):
    m = S.model(script, w.settings, w.step, x, oracle, cap=ANCHOR_CAP)
    assert m is not None, f"{script.name}: no CPU model for the anchor {w.step.entry}"
    keys = [k for k in m if not k.startswith("_")]
    assert keys
    for k in keys:
        want = np.asarray(m[k])
        got = np.asarray(out[k])[:len(want)]
        if want.dtype.kind == "f":
            assert got.dtype == want.dtype, (script.name, k)
            assert np.array_equal(np.isinf(got), np.isinf(want)), (script.name, k, "infinities")
            assert not np.isnan(got).any(), (script.name, k, "NaN")
        bad = (got != want).reshape(len(want), -1).any(axis=1)
        assert not bad.any(), f"{script.name}: anchor {w.step.entry} at step {w.i}: {k!r} differs from the model at frames {np.flatnonzero(bad)[:8].tolist()}"


def _in_effect(dec, script, chg, out, prev, streams):
    """a change without a CPU model was in effect during the observation that follows it"""
    what, v = chg.step
    if what == "stream":
        assert dec._lib.polar_get_stream(dec._h) == streams[v].cuda_stream, (script.name, chg.i)
    elif what == "select_kernel" and what not in script.quiet:
        assert prev is not None and out["kernel_name"].tobytes() != prev["kernel_name"].tobytes(), (script.name, chg.i, dec.kernel_name)
    elif what == "resident_blocks":
        grid, jobs, per, queued = (int(t) for t in out["plan"])
        if v:
            assert grid <= v and queued == 1 and jobs > grid * per, (script.name, chg.i, out["plan"])
        else:
            assert queued == 0 and jobs <= grid * per, (script.name, chg.i, out["plan"])


CASES = [pytest.param(s, "testing", id=f"{s.name}-testing") for s in S.SCRIPTS] + \
        [pytest.param(s.without_hooks(), "shipped", id=f"{s.name}-shipped") for s in S.SCRIPTS]


@pytest.mark.parametrize("script,which", CASES)
def test_reused_context_equals_a_fresh_one(script, which, oracle):
    import torch
    streams = {"A": torch.cuda.Stream(), "B": torch.cuda.Stream()}
    ws = list(S.walk(script))
    changes = [k for k, w in enumerate(ws) if isinstance(w.step, S.Chg)]
    anchor = (changes[-1] + 1) if changes else 0
    dec = _create(script, which)
    prev = None
    try:
        for k, w in enumerate(ws):
            if isinstance(w.step, S.Chg):
                _change(dec, w.step, streams)
                continue
            where = f"{script.name} ({which} library), step {w.i}: {w.step.entry} B={w.step.B} under {S.recipe(w.settings)}" + \
                (f", frozen_mask {w.settings['frozen_mask']}" if w.step.entry in S.TAKES_MASK and w.settings["frozen_mask"] else "")
            x = S.inputs(script, w.nobs, w.step.B, w.settings["sys_polar"]) if w.step.entry not in S.GENERATED else S.inputs(script, 0, 1)
            out = _observe(dec, script, w, x, which)
            other = _fresh(script, w.settings, which, streams)
            try:
                _same(out, _observe(other, script, w, x, which), where)
            finally:
                other.close()
            if w.step.entry == "bp_readout":
                assert int(out["refused"][0]) == (1 if w.settings["bp_stop"] == "g" else 0), where
            if k and isinstance(ws[k - 1].step, S.Chg) and ws[k - 1].step.what in S.NO_MODEL:
                _in_effect(dec, script, ws[k - 1], out, prev, streams)
            if k == anchor:
                _anchor(script, w, x, out, oracle)
            prev = out
    finally:
        dec.close()


def test_reused_codebook_equals_a_fresh_one():
    """polar_codebook_set_stream, the one setter of the header that is not a polar_ctx's: one code book through batches of
    5, 70, 5, 70 frames on its own stream, torch stream A, B and A again; every call against a fresh book on the same stream, the
    last one also against the members' own decode_device (what a book promises for every frame)."""
    import torch
    import polardecoding_amd as pa
    rng = np.random.default_rng(31)
    rows = 2.0 + 2.5 * rng.standard_normal((70, 128))
    code = rng.integers(0, 2, 70).astype(np.int32)
    streams = {"A": torch.cuda.Stream(), "B": torch.cuda.Stream()}

    def book(stream):
        decs = [pa.SCLdecode(128, 64, L=8), pa.SCLdecode(64, 32, L=8)]
        cb = pa.Codebook(decs)
        for d in decs:
            d.close()   # the codes were copied
        if stream is not None:
            with torch.cuda.stream(streams[stream]):
                cb.use_torch_stream()
        return cb

    def decode(cb, idx):
        d, c = _dev(rows[idx]), _dev(code[idx])
        pm, fl = _full(len(idx), NAN, torch.float64), _full(len(idx), -1, torch.int32)
        torch.cuda.synchronize()
        bits = cb.decode_device(d, c, pm=pm, flags=fl)
        cb.synchronize()
        return {"bits": _np(bits), "pm": _np(pm), "flags": _np(fl), "kernel_name": np.frombuffer(cb.kernel_name.encode(), dtype=np.uint8)}

    cb = book(None)
    try:
        for i, (stream, B) in enumerate(((None, 5), ("A", 70), ("B", 5), ("A", 70))):
            if stream is not None:
                with torch.cuda.stream(streams[stream]):
                    cb.use_torch_stream()
                assert cb._lib.polar_codebook_get_stream(cb._h) == streams[stream].cuda_stream
            idx = (37 * i + np.arange(B)) % 70
            out = decode(cb, idx)
            other = book(stream)
            try:
                _same(out, decode(other, idx), f"code book, call {i}: B={B} on stream {stream}")
            finally:
                other.close()
        for c, N in ((0, 128), (1, 64)):   # the anchor: every frame is what its member decodes
            sel = idx[code[idx] == c]
            dec = pa.SCLdecode(N, N // 2, L=8)
            d = _dev(rows[sel][:, :N])
            pm, fl = _full(len(sel), NAN, torch.float64), _full(len(sel), -1, torch.int32)
            torch.cuda.synchronize()
            bits = dec.decode_device(d, pm=pm, flags=fl)
            dec.synchronize()
            at = np.flatnonzero(code[idx] == c)
            assert len(sel) > 10
            assert np.array_equal(out["bits"][at][:, :N // 32], _np(bits)) and np.array_equal(out["pm"][at], _np(pm))
            assert np.array_equal(out["flags"][at], _np(fl))
            dec.close()
    finally:
        cb.close()


def test_group_of_a_crc_file_decoder_equals_the_group_of_its_taps():
    """A decoder made from a generator-matrix file hands its real g(D) to polar_group_create and polar_fer_multi_gpu (its cfg
    used to keep crc_r = 0 and both refused it): one rank of each gives what the decoder's own polar_fer_batch gives."""
    import polardecoding_amd as pa
    path = os.path.join(HERE, "golden", "CRC_6.dat")
    assert tuple(pa.load_crc_matrix(path)[0]) == tuple(pa.CRC6_TAPS)
    a = pa.CASCL(128, 64, L=8, crc_file=path)
    b = pa.CASCL(128, 64, L=8, crc_taps=pa.CRC6_TAPS)
    assert (a._cfg.crc_r, a._cfg.n_taps, [a._cfg.crc_taps[i] for i in range(3)]) == (6, 3, list(pa.CRC6_TAPS))
    seed, first, snr, n = 77, 4096, 1.0, 3000
    ga, gb = pa.Group(a, 1), pa.Group(b, 1)
    try:
        ra, rb, rd = ga.fer_batch(seed, first, snr, n)[:2], gb.fer_batch(seed, first, snr, n)[:2], a.fer_batch(seed, first, snr, n)
        assert ra == rb == rd and rd[0] > 0, (ra, rb, rd)
        assert a.fer_multi_gpu(1, seed, first, snr, n)[:2] == rd
    finally:
        ga.close()
        gb.close()
        a.close()
        b.close()
