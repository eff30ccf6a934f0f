"""GPU: the sent-path trace (include/polar_hip.h, "Sent-path trace") against the numpy model of tests/trace_model.py, everything
by ==.

The cases are those of tests/trace_cases.py, the smallest shapes at which each mechanism first exists: N = 32 (the whole history
and the match flag's bits in one register word), N = 64 (history rows in LDS; a CRC), N = 128 with L = 2 and 32 (S = 32 and 2
lanes per path), L = 1, L = 64 and 128 (the wide kernel: the matching slot found inside one wavefront and across two), a PAC and a
random dynamic context, a rate-matched, a systematic and a CRC-file context.  Every pool is held to the condition of
trace_cases.py on the model before anything is compared.  Then the identities with polar_list_decode and polar_decode_device,
which need no model, ragged batches and capped grids (a wavefront's second frame sees what the first left behind), the extents
of every output, the refusals, the host form and graph capture."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import extents as X  # noqa: E402
import list_model as LM  # noqa: E402
import trace_cases as TC  # noqa: E402
import trace_model as TM  # noqa: E402

F64, F32 = 0, 1
EINVAL, ENOKERNEL = -1, -4
FLAG_RERANK_MASK = 0xFFFFFFFB
OUTS = ("loss_leaf", "loss_rank", "rank", "chosen", "flags")
NP_DTYPE = {F64: np.float64, F32: np.float32}


def _cuda(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()          # a copy: the pools are read-only


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(name, dtype, sl=slice(None)):
    """device rows (of the case's input width) and packed sent words of the pool's frames sl"""
    u, llr, rows, _ = TC.pool(name)
    r = rows[sl]
    return _cuda(r.astype(np.float32) if dtype == F32 else r), _cuda(TM.pack(u[sl]).view(np.int32))


def _host(t):
    """trace_list_device's tuple -> numpy in the model's dtypes"""
    kinds = (np.int32, np.uint32, np.int32, np.int32, np.uint32)
    return tuple(a.cpu().numpy().view(k) if a is not None else None for a, k in zip(t, kinds))


def _trace(dec, name, dtype, sl=slice(None), **want):
    d_in, d_u = _inputs(name, dtype, sl)
    t = dec.trace_list_device(d_in, d_u, **want)
    dec.synchronize()
    return _host(t), t, d_in, d_u


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """(device result, model result) of a case, computed once and shared; nothing in it is written afterwards"""
    want = TC.model(name, NP_DTYPE[dtype])
    TC.check_condition(name, want)                                        # before any comparison
    dec = TC.decoder(name, dtype)
    try:
        assert np.array_equal(dec.info_order, TC.case_code(name)[0])
        got, tens, d_in, d_u = _trace(dec, name, dtype)
        kernel = dec.kernel_name
    finally:
        dec.close()
    return dict(got=got, want=want, tens=tens, kernel=kernel)


def _assert_equal(got, want, what=""):
    for g, w, n in zip(got, want, OUTS):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what} {n} differs from frame {bad[0]} on ({bad.size} frames): {g[bad[:4]]} != {w[bad[:4]]}"


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(TC.CASES))
def test_trace_equals_the_model(name, dtype):
    c = _case(name, dtype)
    _assert_equal(c["got"], c["want"], name)
    N, L = TC.CASES[name][1], TC.CASES[name][3]
    loss_leaf, loss_rank, rank, chosen, flags = c["got"]
    assert np.array_equal(loss_leaf == N, rank >= 0)                      # rule 5, stated again on the device output
    assert (loss_rank > L).any()                                          # a frame lost at a ranking leaf
    j0 = TC.pool(name)[3]
    assert loss_leaf[-2] == j0 and loss_rank[-2] == 0 and loss_leaf[-1] == N and rank[-1] == chosen[-1]   # the planted rows


@pytest.mark.parametrize("name", ["n32-l4", "n64-crc6-l4", "wide-n64-l128", "rm-n64-e48-l8"])
def test_count_equals_bincount_and_adds(name):
    import torch
    N = TC.CASES[name][1]
    c = _case(name, F64)
    loss_leaf, loss_rank, rank, chosen, flags = c["got"]
    t_ll, _, t_rank, t_chosen, _ = c["tens"]
    B = loss_leaf.size
    want = np.zeros(N + 4, dtype=np.int64)
    want[:N] = np.bincount(loss_leaf[loss_leaf < N], minlength=N)
    want[N:N + 3] = np.bincount(TM.classes(rank, chosen), minlength=3)
    want[N + 3] = B
    assert np.array_equal(want.astype(np.uint64), TM.count(N, loss_leaf, rank, chosen))
    dec = TC.decoder(name)
    try:
        hist = torch.zeros(N + 4, dtype=torch.int64, device="cuda")
        dec.trace_count_device(t_ll, t_rank, t_chosen, hist)
        dec.synchronize()
        assert np.array_equal(hist.cpu().numpy(), want)
        dec.trace_count_device(t_ll, t_rank, t_chosen, hist)              # it ADDS
        dec.trace_count_device(t_ll[:37], t_rank[:37], t_chosen[:37], hist)   # and a ragged third call: less than a wavefront
        dec.synchronize()
        third = TM.count(N, loss_leaf[:37], rank[:37], chosen[:37]).astype(np.int64)
        assert np.array_equal(hist.cpu().numpy(), 2 * want + third)
        # guard words around the histogram
        arena = X.Arena("torch", X.Arena.need([("int64", N + 4, 2, N + 4)]))
        h = arena.carve("hist", "int64", N + 4, 2, N + 4)
        h.zero_()
        assert dec._lib.polar_list_trace_count(dec._h, _ptr(t_ll), _ptr(t_rank), _ptr(t_chosen), B, _ptr(h)) == 0
        dec.synchronize()
        torch.cuda.synchronize()
        assert arena.check() == [] and np.array_equal(h.cpu().numpy(), want)
        for k in range(4):                                                # every pointer is required
            args = [_ptr(t_ll), _ptr(t_rank), _ptr(t_chosen), B, _ptr(hist)]
            args[k if k < 3 else 4] = None
            assert dec._lib.polar_list_trace_count(dec._h, *args) == EINVAL
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["n32-l4", "n64-crc6-l4", "n128-l32", "wide-n64-l64", "pac64-l8", "rm-n64-e48-l8", "sys-n64-crc6-l4",
                                  "crcfile-n64-l8"])
def test_identities_with_the_existing_entry_points(name):
    """no model: paths[f][rank[f]] of polar_list_decode is the sent row where rank >= 0 and no row is where rank < 0; class 0 <=>
    polar_decode_device returns the sent u; flags are the decode's"""
    import torch
    kind, N, K, L, taps, seed = TC.CASES[name]
    loss_leaf, loss_rank, rank, chosen, flags = _case(name, F64)["got"]
    u = TC.pool(name)[0]
    B = u.shape[0]
    dec = TC.decoder(name)
    try:
        d_in, _ = _inputs(name, F64)
        paths, pm, rem, count, l_flags = dec.decode_list_device(d_in)
        p_fl = torch.zeros(B, dtype=torch.int32, device="cuda")
        bits = dec.decode_device(d_in, flags=p_fl)
        dec.synchronize()
    finally:
        dec.close()
    paths = LM.unpack(paths.cpu().numpy(), N)
    count = count.cpu().numpy()
    hit = (paths == u[:, None, :]).all(-1) & (np.arange(L)[None, :] < count[:, None])
    f = np.arange(B)
    assert hit[f[rank >= 0], rank[rank >= 0]].all() and not hit[rank < 0].any()
    assert np.array_equal(chosen, LM.kstar(rem.cpu().numpy().view(np.uint32), count, taps is not None))
    correct = (LM.unpack(bits.cpu().numpy(), N) == u).all(1)
    assert np.array_equal(TM.classes(rank, chosen) == 0, correct)
    assert np.array_equal(flags, l_flags.cpu().numpy().view(np.uint32))
    assert np.array_equal(flags, p_fl.cpu().numpy().view(np.uint32) & FLAG_RERANK_MASK)


@pytest.mark.parametrize("name", ["n32-l4", "n64-l8", "wide-n64-l128", "rm-n64-e48-l8"])
def test_ragged_batches_and_later_jobs(name):
    """B = 1, 63, 65 on one context, then the whole pool under a grid of 1 and of 3 blocks: every block decodes many frames one
    after the other, and a frame's match flags, loss leaf and history start clean"""
    from polardecoding_amd import testing as T
    want = TC.model(name)
    dec = TC.decoder(name)
    try:
        for B in (1, 63, 65, 1):
            got, _, _, _ = _trace(dec, name, F64, slice(0, B))
            _assert_equal(got, [w[:B] for w in want], f"{name} B={B}")
        got, _, _, _ = _trace(dec, name, F64, slice(97, 98))              # the noiseless row alone
        _assert_equal(got, [w[97:98] for w in want], name)
        for cap in (1, 3):
            T.resident_blocks(dec, cap)
            # the planted lost frame first: what it leaves behind meets a frame that is not lost
            order = np.r_[96, 97, 0:96]
            u, llr, rows, _ = TC.pool(name)
            d_in, d_u = _cuda(rows[order]), _cuda(TM.pack(u[order]).view(np.int32))
            t = dec.trace_list_device(d_in, d_u)
            dec.synchronize()
            got = _host(t)
            assert T.last_plan(dec)[0] == cap
            _assert_equal(got, [w[order] for w in want], f"{name} cap={cap}")
    finally:
        dec.close()


def _arena(B):
    specs = [("int32", B, 2, 1)] * 5
    arena = X.Arena("torch", X.Arena.need(specs))
    return arena, {n: arena.carve(n, *s) for n, s in zip(OUTS, specs)}


@pytest.mark.parametrize("name", ["n32-l4", "n128-l32", "wide-n64-l64", "rm-n64-e48-l8"])
def test_outputs_stay_inside_their_extents(name):
    import torch
    dec = TC.decoder(name)
    try:
        for B in (1, 67):
            want = [w[:B] for w in TC.model(name)]
            d_in, d_u = _inputs(name, F64, slice(0, B))
            snap_in, snap_u = X.snapshot(d_in), X.snapshot(d_u)
            arena, v = _arena(B)
            rc = dec._lib.polar_list_trace(dec._h, _ptr(d_in), 0, 0.0, _ptr(d_u), B, *[_ptr(v[n]) for n in OUTS])
            dec.synchronize()
            torch.cuda.synchronize()
            assert rc == 0 and arena.check() == [] and X.unchanged(d_in, snap_in) and X.unchanged(d_u, snap_u), (name, B)
            _assert_equal(_host([v[n] for n in OUTS]), want, f"{name} B={B}")
            # every output alone, the others NULL: the same values, nothing else written
            for k, n in enumerate(OUTS):
                arena, v = _arena(B)
                args = [_ptr(v[m]) if m == n else None for m in OUTS]
                rc = dec._lib.polar_list_trace(dec._h, _ptr(d_in), 0, 0.0, _ptr(d_u), B, *args)
                dec.synchronize()
                assert rc == 0 and arena.check() == [], (name, B, n)
                h = arena.host()
                for m in OUTS:
                    _, _, start, end, _ = arena.span(m)
                    if m != n:
                        assert (h[start:end] == X.FILL).all(), (name, B, n, m)
                assert np.array_equal(v[n].cpu().numpy().view(want[k].dtype), want[k]), (name, B, n)
        assert dec._lib.polar_list_trace(dec._h, _ptr(d_in), 0, 0.0, _ptr(d_u), 1, None, None, None, None, None) == EINVAL
        assert dec._lib.polar_list_trace(dec._h, _ptr(d_in), 0, 0.0, None, 1, *[_ptr(v[n]) for n in OUTS]) == EINVAL
        assert dec._lib.polar_list_trace(dec._h, None, 0, 0.0, _ptr(d_u), 1, *[_ptr(v[n]) for n in OUTS]) == EINVAL
        got, _, _, _ = _trace(dec, name, F64, slice(0, 5))                # and it still works
        _assert_equal(got, [w[:5] for w in TC.model(name)], name)
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["n64-crc6-l4", "wide-n64-l64", "pac64-l8"])
def test_global_scratch_variant_gives_the_same_trace(name):
    """the GA instantiations (LLR levels in global scratch: what N = 1024 with L = 32 in f64 runs), forced at a small shape"""
    from polardecoding_amd import testing as T
    dec = T.select_kernel(TC.decoder(name), T.KERNEL_GENERIC_SPILL)
    try:
        got, _, _, _ = _trace(dec, name, F64)
    finally:
        dec.close()
    _assert_equal(got, TC.model(name), name)


def test_n1024_crc24_l8_identities():
    """N = 1024, K = 512, CRC-24C, L = 8, where the ordinary decode is the pair kernel: class 0 <=> it returns the sent word,
    chosen and rank against polar_list_decode, and four frames against the model"""
    import polardecoding_amd as pa
    import torch
    from oracle import oracle_py as O
    N, K, L, B = 1024, 512, 8, 48
    code = O.Code(N, K, X.CRC24C)
    sig = O.sigma_from_db(1.25)
    u, ys = O.Sim(31).frames(code, sig, B)
    rows = np.stack([O.llr_from_y(y, sig) for y in ys])
    dec = pa.CASCL(N, K, L=L)
    try:
        d_in, d_u = _cuda(rows), _cuda(TM.pack(u).view(np.int32))
        t = dec.trace_list_device(d_in, d_u)
        paths, pm, rem, count, l_flags = dec.decode_list_device(d_in)
        bits = dec.decode_device(d_in)
        dec.synchronize()
        loss_leaf, loss_rank, rank, chosen, flags = _host(t)
        io = dec.info_order
    finally:
        dec.close()
    paths = LM.unpack(paths.cpu().numpy(), N)
    hit = (paths == u[:, None, :]).all(-1)
    assert np.array_equal(rank, np.where(hit.any(1), hit.argmax(1), -1)) and np.array_equal(loss_leaf == N, rank >= 0)
    assert np.array_equal(chosen, LM.kstar(rem.cpu().numpy().view(np.uint32), count.cpu().numpy(), True))
    cls = TM.classes(rank, chosen)
    assert np.array_equal(cls == 0, (LM.unpack(bits.cpu().numpy(), N) == u).all(1)) and (cls == 0).any() and (cls == 2).any()
    pick = np.r_[np.flatnonzero(cls == 2)[:2], np.flatnonzero(cls == 0)[:2]]
    frozen = np.ones(N, dtype=np.uint8)
    frozen[io] = 0
    want = TM.trace_model(frozen, None, rows[pick], u[pick], L, crc=(io, X.CRC24C))
    _assert_equal([a[pick] for a in (loss_leaf, loss_rank, rank, chosen, flags)], want, "n1024")


def test_host_form_equals_the_device_form():
    for name in ("n64-crc6-l4", "rm-n64-e48-l8"):
        u, llr, rows, _ = TC.pool(name)
        dec = TC.decoder(name)
        try:
            got = dec.trace_list_batch(rows[90:], u[90:])
            rk = np.full(8, 77, dtype=np.int32)                          # one output alone
            h_rows, h_u = np.ascontiguousarray(rows[90:]), np.ascontiguousarray(u[90:])
            rc = dec._lib.polar_list_trace_host(dec._h, h_rows.ctypes.data_as(C.POINTER(C.c_double)),
                                                h_u.ctypes.data_as(C.POINTER(C.c_int)), 8, None, None,
                                                rk.ctypes.data_as(C.POINTER(C.c_int)), None, None)
            assert rc == 0
        finally:
            dec.close()
        _assert_equal(got, [w[90:] for w in TC.model(name)], name)
        assert np.array_equal(rk, TC.model(name)[2][90:])


def test_graph_capture_of_trace_and_count():
    """rule 9: after a warm-up at the same B the two calls, one linear chain, are captured into a graph and replayed"""
    import torch
    name = "n64-crc6-l4"
    N = TC.CASES[name][1]
    c = _case(name, F64)
    dec = TC.decoder(name)
    try:
        d_in, d_u = _inputs(name, F64)
        B = d_in.shape[0]
        t = {n: torch.zeros(B, dtype=torch.int32, device="cuda") for n in OUTS}
        hist = torch.zeros(N + 4, dtype=torch.int64, device="cuda")
        lib, h = dec._lib, dec._h

        def chain():
            dec.use_torch_stream()
            rc = [lib.polar_list_trace(h, _ptr(d_in), 0, 0.0, _ptr(d_u), B, *[_ptr(t[n]) for n in OUTS]),
                  lib.polar_list_trace_count(h, _ptr(t["loss_leaf"]), _ptr(t["rank"]), _ptr(t["chosen"]), B, _ptr(hist))]
            assert rc == [0, 0], rc

        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            chain()                                                       # warm-up at the same B
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                chain()
            for n in OUTS:
                t[n].zero_()
            hist.zero_()
            for _ in range(2):
                g.replay()
            stream.synchronize()
        _assert_equal(_host([t[n] for n in OUTS]), c["got"], "replay")
        loss_leaf, _, rank, chosen, _ = c["got"]
        assert np.array_equal(hist.cpu().numpy().view(np.uint64), 2 * TM.count(N, loss_leaf, rank, chosen))
        del g
    finally:
        dec.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _refused(dec, code):
    import torch
    B, NW, N = 2, dec.NW, dec.N
    d_in = torch.zeros((B, dec.E), dtype=torch.float64, device="cuda")
    d_u = torch.zeros((B, NW), dtype=torch.int32, device="cuda")
    o = [torch.zeros(B, dtype=torch.int32, device="cuda") for _ in OUTS]
    hist = torch.zeros(N + 4, dtype=torch.int64, device="cuda")
    lib, h = dec._lib, dec._h
    assert lib.polar_list_trace(h, _ptr(d_in), 0, 0.0, _ptr(d_u), B, *[_ptr(x) for x in o]) == code
    assert lib.polar_list_trace_count(h, _ptr(o[0]), _ptr(o[2]), _ptr(o[3]), B, _ptr(hist)) == code
    host, hu, out = np.zeros((B, dec.E)), np.zeros((B, N), dtype=np.int32), np.zeros(B, dtype=np.int32)
    assert lib.polar_list_trace_host(h, host.ctypes.data_as(C.POINTER(C.c_double)), hu.ctypes.data_as(C.POINTER(C.c_int)), B,
                                     out.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, None) == code
    assert not hist.cpu().numpy().any() and not any(x.cpu().numpy().any() for x in o)
    bits = dec.decode_device(d_in + 1.0)                                  # the context still decodes
    dec.synchronize()
    assert not bits.cpu().numpy().any()


@pytest.mark.parametrize("kind", ["SC", "BP", "Q8", "staged", "N2048"])
def test_refusals_leave_the_context_usable(kind):
    import polardecoding_amd as pa
    CRC6 = TC.CRC6
    make = {"SC": lambda: pa.SCdecode(64, 32), "BP": lambda: pa.BP(64, 32, iterMax=4),
            "Q8": lambda: pa.CASCL(64, 26, L=8, crc_taps=CRC6, dtype=pa.Q8),
            "staged": lambda: pa.CASCL(64, 26, L=8, crc_taps=CRC6, stages=(2, 8)),
            "N2048": lambda: pa.SCLdecode(2048, 1024, L=2)}[kind]
    dec = make()
    try:
        _refused(dec, ENOKERNEL if kind == "N2048" else EINVAL)
        if kind == "staged":                                             # the rule is a state, not a property
            dec.set_cascl_stages(None)
            u, llr, rows, _ = TC.pool("crcfile-n64-l8")
            got = dec.trace_list_batch(rows[:4], u[:4])
            _assert_equal(got, [w[:4] for w in TC.model("crcfile-n64-l8")], "staged")
    finally:
        dec.close()
