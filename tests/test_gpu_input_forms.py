"""GPU: the load stage of every decode kernel, for every row type, y form and alignment (tests/input_forms.py).

For every case (one context per kernel instantiation family, at the smallest shape that selects it) and every form (R, IN,
sigma, shift): the base rows as IN, placed `shift` elements into a 16-byte-aligned allocation that is NaN everywhere else,
are decoded with sigma, and every per-frame output of the entry point -- bits, metric, flags, round trips, attempts, list
size, graph, flip sets, list rows, SCAN soft outputs, genie counters, pre-filled with a sentinel -- must equal with == the CPU
reference on form_rows(): oracle.decode in R for SC, SCL, CA-SCL and BP, the numpy models for the rest.  The flags of the
oracle's list decoders are compared bit by bit as tests/test_gpu_llr_families.py::_check_list does: POLAR_FLAG_TIE and
POLAR_FLAG_CRC_PASS always, POLAR_FLAG_RERANK against the oracle's count in f64 (never set by k_scl_generic) and not at all
in f32.  Afterwards the allocation's NaN frame and the rows are unchanged, and all forms of one (R, LLR-or-y) pair agree
among themselves byte for byte (POLAR_FLAG_RERANK aside: a diagnostic of the kernel that ran, and the kernel may depend on
IN).  A cell whose DISPATCH entry is None must return POLAR_ENOKERNEL and write nothing; tests/test_input_forms_host.py
shows why no cell is one today.

BP returns bits and round trips only: its cells catch gross errors (a wrong element, a wrong width, a missing sigma), not
single roundings.  A HIP runtime error in a decode ends the session: nothing more is started on a device that has faulted."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import input_forms as IF  # noqa: E402
import list_model as LM  # noqa: E402

IDS = [c.name for c in IF.CASES]
SENT = -7   # every output starts as this (bits: all ones)


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _ints(*shape):
    import torch
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda")


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


_LAST = []   # the output tensors of the call in flight, and their bytes before it


def _go(tens, call):
    _LAST[:] = [(t, t.cpu().numpy().tobytes()) for t in tens]
    call()


def _run(case, dec, d, sigma):
    """the case's entry point on device rows d -> ({output name: host array}, the device tensors it was given)"""
    import torch
    B, N = d.shape
    bits = _ints(B, dec.NW)
    pm = torch.full((B,), float(SENT), dtype=torch.float64, device="cuda")
    fl = _ints(B)
    e = case.entry
    del _LAST[:]
    torch.cuda.synchronize()   # torch's fills are done before the ctx stream reads and writes the buffers
    if e == "polar_decode_device":
        outs, tens = dict(pm=pm, flags=fl), (bits, pm, fl)
        _go(tens, lambda: dec.decode_device(d, sigma=sigma, out_bits=bits, pm=pm, flags=fl))
    elif e == "polar_time_decode_device":
        outs, tens = {}, (bits,)
        _go(tens, lambda: dec.time_decode_device(d, bits, 2, sigma=sigma))
    elif e == "polar_bp_decode_device":
        it = _ints(B)
        outs, tens = dict(iters=it, flags=fl), (bits, it, fl)
        _go(tens, lambda: dec.decode_bp_device(d, sigma=sigma, out_bits=bits, iters=it, flags=fl))
    elif e == "polar_bp_readout_device":
        E = torch.zeros((len(case.opts["checkpoints"]), dec.N.bit_length()), dtype=torch.int64, device="cuda")
        u = torch.from_numpy(_pack(IF.sent_bits(case))).cuda()
        torch.cuda.synchronize()
        outs, tens = dict(E=E), (bits, E)
        _go(tens, lambda: dec.bp_readout_device(d, u, case.opts["checkpoints"], E, out_bits=bits, sigma=sigma))
    elif e == "polar_cascl_decode_device":
        ls = _ints(B)
        outs, tens = dict(pm=pm, flags=fl, list=ls), (bits, pm, fl, ls)
        _go(tens, lambda: dec.decode_cascl_device(d, sigma=sigma, out_bits=bits, pm=pm, flags=fl, list_size=ls))
    elif e == "polar_scf_decode_device":
        at = _ints(B)
        outs, tens = dict(flags=fl, attempts=at), (bits, fl, at)
        _go(tens, lambda: dec.decode_scf_device(d, sigma=sigma, out_bits=bits, flags=fl, attempts=at))
    elif e == "polar_scf_decode_sets_device":
        at, st = _ints(B), _ints(B, 3)
        outs, tens = dict(flags=fl, attempts=at, sets=st), (bits, fl, at, st)
        _go(tens, lambda: dec.decode_scf_sets_device(d, sigma=sigma, out_bits=bits, flags=fl, attempts=at, sets=st))
    elif e == "polar_scan_decode_device":
        ty = torch.float32 if dec.dtype == 1 else torch.float64
        lu = torch.full((B, N), float("nan"), dtype=ty, device="cuda")
        ex = torch.full((B, N), float("nan"), dtype=ty, device="cuda")
        torch.cuda.synchronize()
        outs, tens = dict(llr_u=lu, ext_x=ex), (bits, lu, ex)
        _go(tens, lambda: dec.decode_scan_device(d, sigma=sigma, out_bits=bits, llr_u=lu, ext_x=ex))
    elif e == "polar_bpl_decode_device":
        it, gr, tot = _ints(B), _ints(B), _ints(B)
        outs, tens = dict(iters=it, flags=fl, graph=gr, total=tot), (bits, it, fl, gr, tot)
        _go(tens, lambda: dec.decode_bpl_device(d, sigma=sigma, out_bits=bits, iters=it, flags=fl, graph=gr, total_iters=tot))
    elif e == "polar_genie_count_device":
        cnt = torch.zeros((2, N), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        _go((cnt,), lambda: dec.genie_count_device(d, cnt, sigma=sigma))
        dec.synchronize()
        return dict(counts=cnt.cpu().numpy()), (cnt,)
    elif e == "polar_list_decode":
        paths, lpm, rem, count, lfl = dec.decode_list_device(d, sigma=sigma)
        dec.synchronize()
        return dict(paths=LM.unpack(paths.cpu().numpy(), N), pm=lpm.cpu().numpy(), rem=_u32(rem), count=_u32(count),
                    flags=_u32(lfl)), (paths, lpm, rem, count, lfl)
    else:
        raise ValueError(e)
    dec.synchronize()
    got = dict(bits=_unpack(bits.cpu().numpy(), N))
    for k, t in outs.items():
        got[k] = _u32(t) if t.dtype == torch.int32 and k == "flags" else t.cpu().numpy()
        if got[k].dtype == np.int32:
            got[k] = got[k].astype(np.int64)
    return got, tens


def _pack(u):
    B, N = u.shape
    w = (u.reshape(B, N // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return w.astype(np.uint32).view(np.int32)


def _same(case, got, want, family, R, label):
    """every output against the reference, =="""
    want = dict(want)
    if case.entry == "polar_time_decode_device":
        want = dict(bits=want["bits"])
    if case.ref in IF.LIST_REFS and "flags" in got:   # the oracle's list decoders: the flags word bit by bit
        fl = got["flags"]
        assert not (fl & ~np.int64(7)).any(), (label, "unknown flag bits")
        assert np.array_equal((fl & IF.FLAG_TIE) != 0, want.pop("tie")), (label, "FLAG_TIE")
        if "crc_pass" in want:
            assert np.array_equal((fl & IF.FLAG_CRC_PASS) != 0, want.pop("crc_pass")), (label, "FLAG_CRC_PASS")
        else:
            assert not (fl & IF.FLAG_CRC_PASS).any(), (label, "FLAG_CRC_PASS without a CRC")
        rerank = want.pop("rerank")
        if R == "f64":
            if family == "k_scl_generic":
                assert not (fl & IF.FLAG_RERANK).any(), (label, "FLAG_RERANK from k_scl_generic")
            else:   # kernels that pre-rank on the metrics' high words
                assert np.array_equal((fl & IF.FLAG_RERANK) != 0, rerank), (label, "FLAG_RERANK")
    if case.ref == "adaptive":
        got = dict(got, flags=got["flags"] & ~np.int64(IF.FLAG_RERANK))
    for k in ("tie", "crc_pass", "rerank"):
        want.pop(k, None)
    assert set(want) <= set(got), (label, sorted(want), sorted(got))
    for k, w in want.items():
        g, w = np.asarray(got[k]), np.asarray(w)
        if k in ("llr_u", "ext_x"):
            assert g.dtype == w.dtype and not np.isnan(g).any(), (label, k)
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{label}: {k} differs from the reference at {bad[:8]} ({bad.size} of {len(g)})"


def _bytes_of(got):
    out = {}
    for k, v in got.items():
        v = np.asarray(v)
        if k == "flags":
            v = v & ~np.int64(IF.FLAG_RERANK)
        out[k] = np.ascontiguousarray(v).tobytes()
    return out


@pytest.mark.parametrize("R", ["f64", "f32"])
@pytest.mark.parametrize("case", IF.CASES, ids=IDS)
def test_every_form_equals_the_reference(case, R, oracle):
    import polardecoding_amd as pa
    x = IF.base_rows(case)
    dec = IF.make_dec(case, R)
    try:
        io = IF.code_of(case)[0]
        assert np.array_equal(dec.info_order, io), case.name
        own = IF.families_of(IF.DISPATCH[case.name][(R, R)])
        name = dec.kernel_name
        assert any(re.search(re.escape({"k_bp_global": "k_bp", "k_scl_list": "k_scl_generic", "k_bp_readout": "k_bp_w128",
                                        "k_genie_lanes": "k_sc_lanes"}.get(f, f)) + r"<", name) for f in own), (case.name, name)
        print(f"KERNEL input forms {case.name} {R}: {name}")
        refs, first = {}, {}
        for form in (f for f in IF.FORMS if f.R == R):
            label = f"{case.name}: {IF.form_id(form)}"
            cell = IF.DISPATCH[case.name][(R, form.IN)]
            xin = x.astype(IF.NP[form.IN])
            p = IF.place(xin, form.shift, backend="torch")
            assert p.rows.data_ptr() % 16 == (form.shift * xin.itemsize) % 16 and p.rows.is_contiguous()
            if cell is None:   # the library refuses the pair: the documented code, and nothing is written
                with pytest.raises(pa.PolarError, match=rf"rc={IF.ENOKERNEL}\)"):
                    _run(case, dec, p.rows, form.sigma)
                dec.synchronize()
                assert _LAST and all(t.cpu().numpy().tobytes() == before for t, before in _LAST), f"{label}: a refused call wrote"
                assert IF.frame_intact(p, xin), label
                continue
            key = form.sigma > 0
            if key not in refs:
                refs[key] = IF.reference(case, R, IF.form_rows(x, form.IN, form.sigma, R), oracle)
            try:
                got, _ = _run(case, dec, p.rows, form.sigma)
            except pa.PolarError as err:
                if "rc=-3)" in str(err):   # a HIP runtime error: nothing more is started on this device
                    pytest.exit(f"{label}: {err}", returncode=3)
                raise
            fams = IF.families_of(cell)
            _same(case, got, refs[key], fams[0] if len(fams) == 1 else None, R, label)
            assert IF.frame_intact(p, xin), f"{label}: the rows or the NaN frame around them changed"
            b = _bytes_of(got)
            if key not in first:
                first[key] = (label, b)
            else:
                for k in b:
                    assert b[k] == first[key][1][k], f"{label}: {k} differs from {first[key][0]}"
        assert set(refs) == {False, True}
    finally:
        dec.close()


def test_a_refused_pair_writes_nothing():
    """what a None cell of DISPATCH asserts, on a call the library does refuse: polar_bp_readout_device beyond its largest N
    returns POLAR_ENOKERNEL and leaves the outputs as they were"""
    import torch
    import polardecoding_amd as pa
    dec = pa.BP(2048, 1024, iterMax=2, info_order=np.asarray(IF._beta_order(2048)[1024:], dtype=np.int32))
    try:
        p = IF.place(np.ones((3, 2048), dtype=np.float32), 1, backend="torch")
        bits = _ints(3, dec.NW)
        E = torch.full((1, 12), SENT, dtype=torch.int64, device="cuda")
        u = torch.zeros((3, dec.NW), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(pa.PolarError, match=rf"rc={IF.ENOKERNEL}\)"):
            dec.bp_readout_device(p.rows, u, (2,), E, out_bits=bits)
        dec.synchronize()
        assert (bits.cpu().numpy() == SENT).all() and (E.cpu().numpy() == SENT).all()
        assert IF.frame_intact(p, np.ones((3, 2048), dtype=np.float32))
    finally:
        dec.close()
