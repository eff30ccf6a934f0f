"""GPU: BP list decoding over permuted factor graphs (POLAR_ALGO_BPL; include/polar_hip.h).

Bits, iters, graph, flags and total_iters of every frame against the numpy model (tests/bpl_model.py, held to the oracle in
tests/test_bpl_host.py) in f64, and against the composition by rules 4-6 of the library's own BP contexts built on the
permuted codes, in f64 and f32 with both input types, on every BP kernel (k_bp_w128, k_bp, k_bp_r4, k_bp_global).  Then the
CRC-aided decoder, custom lists, the identity, the edges of the compaction, the consumers of the decoder and the refusals."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bpl_model as M  # noqa: E402

CRC6 = (0, 5, 6)
FLAG_CRC_PASS, FLAG_BP_CONVERGED = 2, 8
AD_CHUNK = 2048   # frames per compaction block (csrc/adaptive_kernel.h)


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _beta_order(N):
    """polarization-weight reliability order (ascending), an explicit Q for N > 1024"""
    n = int(np.log2(N))
    beta = 2.0 ** 0.25
    w = [sum(beta ** b for b in range(n) if (i >> b) & 1) for i in range(N)]
    return [int(i) for i in np.argsort(np.array(w), kind="stable")]


def _bpl(dec, x, sigma=0.0):
    """decode_bpl_device on a host array or a CUDA tensor -> (u_hat, iters, flags, graph, total_iters)"""
    import torch
    d = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    B = d.shape[0]
    outs = [torch.full((B,), -1, dtype=torch.int32, device="cuda") for _ in range(4)]
    bits = torch.full((B, dec.N // 32), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fills are done before the ctx stream reads the buffers
    dec.decode_bpl_device(d, sigma=sigma, out_bits=bits, iters=outs[0], flags=outs[1], graph=outs[2], total_iters=outs[3])
    dec.synchronize()
    return (_unpack(bits.cpu().numpy(), dec.N),) + tuple(o.cpu().numpy().astype(np.int64) for o in outs)


def _same(got, want, what=""):
    for name, g, w in zip(("bits", "iters", "flags", "graph", "total_iters"), got, want):
        assert np.array_equal(g, w), f"{what}: {name} differ at frames {np.flatnonzero((np.asarray(g) != np.asarray(w)).reshape(len(g), -1).any(axis=1))[:8]}"


def _of_model(res):
    return res.bits, res.iters, res.flags, res.graph, res.total


def _sim_frames(oracle, code, seed, per, dbs):
    llr, ys, sigs, us = [], [], [], []
    for k, db in enumerate(dbs):
        sig = oracle.sigma_from_db(db)
        u, y = oracle.Sim(seed + k).frames(code, sig, per)
        us += list(u)
        ys += list(y)
        sigs += [sig] * per
        llr += [oracle.llr_from_y(v, sig) for v in y]
    return np.stack(llr), np.stack(ys), np.array(sigs), np.stack(us)


@functools.lru_cache(maxsize=None)
def _model_set(N, seed, B, iter_max, crc=False):
    """frames of oracle.Sim (half at 1.0 dB, half at 1.5 dB), the model's result on the default list; computed once"""
    from oracle import oracle_py as oracle
    code = oracle.Code(N, N // 2, CRC6 if crc else None)
    llr, ys, sigs, us = _sim_frames(oracle, code, seed, B // 2, (1.0, 1.5))
    n = code.n
    P = min(n, 8)
    res = M.bpl_decode(llr, code.frozen, code.info_order, M.cyclic_graphs(n, P), iter_max, CRC6 if crc else None)
    return code, llr, ys, sigs, us, res, P


# ---- model parity, f64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,iter_max,seed", [(32, 200, 10, 4132), (64, 200, 12, 4164), (128, 200, 20, 4228), (512, 60, 20, 4612)])
def test_default_list_equals_the_model(N, B, iter_max, seed, oracle):
    import polardecoding_amd as pa
    code, llr, ys, sigs, us, res, P = _model_set(N, seed, B, iter_max)
    cls = M.classes(res, P)
    print("classes (graph 0, graph >= 1, none):", cls)
    assert min(cls) >= 1, cls
    dec = pa.BPL(N, N // 2, iterMax=iter_max)
    assert np.array_equal(dec.bpl_graphs, np.asarray(M.cyclic_graphs(code.n, P)))
    _same(_bpl(dec, llr), _of_model(res), f"N={N}")
    # y input: the permutation moves the y values, the kernel forms the LLR (one sigma per call)
    half = B // 2
    _same(_bpl(dec, ys[:half], sigma=float(sigs[0])), tuple(a[:half] for a in _of_model(res)), f"N={N} from y")


# ---- composition parity against the library's own BP contexts ------------------------------------------------------------
def _compose(per_graph, P):
    """rules 4-6 (no CRC) from per-graph (u_hat, t, flags) of every frame"""
    B = len(per_graph[0][1])
    bits, it, fl = (np.array(a, copy=True) for a in per_graph[0])
    graph = np.full(B, P, dtype=np.int64)
    total = np.zeros(B, dtype=np.int64)
    open_ = np.ones(B, dtype=bool)
    for p, (u, t, f) in enumerate(per_graph):
        total[open_] += t[open_]
        acc = open_ & ((f & FLAG_BP_CONVERGED) != 0)
        bits[acc], it[acc], fl[acc], graph[acc] = u[acc], t[acc], f[acc], p
        open_ &= ~acc
    return bits, it, fl, graph, total


COMPOSE_CASES = [(N, dt, in32, 4, B) for N, B in ((128, 4096), (512, 2048), (1024, 3072)) for dt in ("f64", "f32") for in32 in (0, 1)]
COMPOSE_CASES.append((2048, "f64", 0, 3, 2048))


@pytest.mark.parametrize("N,dt,in32,P,B", COMPOSE_CASES)
def test_composition_of_plain_bp_contexts(N, dt, in32, P, B):
    import torch
    import polardecoding_amd as pa
    K, iter_max = N // 2, 30
    dtype = pa.F32 if dt == "f32" else pa.F64
    n = N.bit_length() - 1
    io = _beta_order(N)[N - K:] if N > 1024 else None
    dec = pa.BPL(N, K, iterMax=iter_max, graphs=P, dtype=dtype, info_order=io)
    name = dec.kernel_name
    want_kernel = {128: "k_bp_w128", 512: "k_bp<", 1024: "k_bp_r4", 2048: "k_bp<"}[N]
    assert want_kernel in name and f"x {P} graphs" in name and "k_bpl_gather" in name, name
    d = torch.empty((B, N), dtype=torch.float64, device="cuda")
    dec.generate_device(20 + N, 0, 2.0, d)
    dec.synchronize()
    if in32:
        d = d.to(torch.float32)
    x = d.cpu().numpy()
    I = dec.info_order
    per_graph = []
    for pi in M.cyclic_graphs(n, P):
        s = M.sigma(pi, N)
        sinv = np.argsort(s)
        bp = pa.BP(N, K, iterMax=iter_max, early_stop="g", dtype=dtype, info_order=sinv[I])
        rows = np.ascontiguousarray(x[:, s])
        if in32:
            it = torch.zeros(B, dtype=torch.int32, device="cuda")
            fl = torch.zeros(B, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            bits = bp.decode_bp_device(torch.from_numpy(rows).cuda(), iters=it, flags=fl)
            bp.synchronize()
            up, t, f = _unpack(bits.cpu().numpy(), N), it.cpu().numpy().astype(np.int64), fl.cpu().numpy().astype(np.int64)
        else:
            up, t, f = bp.decode_bp_batch(rows)
            t, f = t.astype(np.int64), f.astype(np.int64)
        u = np.zeros_like(up)
        u[:, s] = up
        per_graph.append((u, t, f))
        bp.close()
    want = _compose(per_graph, P)
    cls = (int((want[3] == 0).sum()), int(((want[3] >= 1) & (want[3] < P)).sum()), int((want[3] == P).sum()))
    print("classes (graph 0, graph >= 1, none):", cls)
    assert min(cls) >= 1, cls
    _same(_bpl(dec, d), want, f"N={N} {dt} in32={in32}")


# ---- CRC-aided -------------------------------------------------------------------------------------------------------------
def test_crc_aided_equals_the_model(oracle):
    import polardecoding_amd as pa
    code, llr, ys, sigs, us, res, P = _model_set(128, 5300, 200, 20, crc=True)
    a0 = res.attempts[0]
    later = a0["conv"] & ~a0["crcok"] & (res.graph >= 1) & (res.graph < P)
    fallback = (res.graph == P) & ((res.flags & FLAG_BP_CONVERGED) != 0) & ((res.flags & FLAG_CRC_PASS) == 0)
    print("converged, failed the CRC, accepted later:", int(later.sum()), " fallback converged without CRC:", int(fallback.sum()))
    assert later.sum() >= 1 and fallback.sum() >= 1
    dec = pa.BPL(128, 64, iterMax=20, crc_taps=CRC6)
    assert dec.A == 70 and "CRC-aided" in dec.kernel_name
    assert np.array_equal(dec.info_order, code.info_order)
    _same(_bpl(dec, llr), _of_model(res), "CRC-aided")


# ---- custom lists ----------------------------------------------------------------------------------------------------------
def _custom_lists():
    rng = np.random.default_rng(3)
    rev7, id7 = list(range(7))[::-1], list(range(7))
    yield "reversal first", 128, [rev7, id7, [(b + 2) % 7 for b in range(7)]]
    low_fixed = [[0, 1, 2, 3, 4] + list(5 + rng.permutation(2)) for _ in range(2)] + [[0, 1, 2, 3, 4, 6, 5]]
    crossing = [[5, 1, 2, 3, 4, 0, 6], [0, 6, 2, 3, 4, 5, 1]]
    randoms = [list(rng.permutation(7)) for _ in range(3)]
    yield "bits 0-4 fixed, bits crossing 5, random", 128, [low_fixed[2], crossing[0], randoms[0], low_fixed[0], crossing[1], randoms[1], randoms[2]]
    yield "P = 32", 64, [list(rng.permutation(6)) for _ in range(32)]


@pytest.mark.parametrize("what,N,graphs", list(_custom_lists()), ids=lambda v: v if isinstance(v, str) else None)
def test_custom_lists_equal_the_model(what, N, graphs, oracle):
    import polardecoding_amd as pa
    seed, it = {128: (4228, 20), 64: (4164, 12)}[N]
    code, llr, *_ = _model_set(N, seed, 200, it)
    llr = llr[:120]
    res = M.bpl_decode(llr, code.frozen, code.info_order, graphs, it)
    P = len(graphs)
    cls = M.classes(res, P)
    print("classes:", cls)
    assert min(cls) >= 1, cls
    assert list(graphs[0]) != list(range(code.n))   # the fallback goes through the un-permute
    dec = pa.BPL(N, N // 2, iterMax=it, graphs=graphs)
    assert np.array_equal(dec.bpl_graphs, np.asarray(graphs))
    _same(_bpl(dec, llr), _of_model(res), what)


# ---- identity (rule 7) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dt", [(128, "f64"), (1024, "f64"), (512, "f32")])
def test_one_identity_graph_is_bp_with_rule_g(N, dt):
    import torch
    import polardecoding_amd as pa
    dtype = pa.F32 if dt == "f32" else pa.F64
    n = N.bit_length() - 1
    bp = pa.BP(N, N // 2, iterMax=25, early_stop="g", dtype=dtype)
    dec = pa.BPL(N, N // 2, iterMax=25, graphs=[list(range(n))], dtype=dtype)
    B = 1500
    d = torch.empty((B, N), dtype=torch.float64, device="cuda")
    bp.generate_device(9, 0, 1.5, d)
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    fl = torch.zeros(B, dtype=torch.int32, device="cuda")
    bp.synchronize()
    torch.cuda.synchronize()
    bits = bp.decode_bp_device(d, iters=it, flags=fl)
    bp.synchronize()
    t, f = it.cpu().numpy().astype(np.int64), fl.cpu().numpy().astype(np.int64)
    conv = (f & FLAG_BP_CONVERGED) != 0
    assert 0 < conv.sum() < B
    _same(_bpl(dec, d), (_unpack(bits.cpu().numpy(), N), t, f, np.where(conv, 0, 1), t), f"identity N={N} {dt}")
    # only the decisions asked for: the path without any glue kernel
    out = dec.decode_bpl_device(d)
    dec.synchronize()
    assert torch.equal(out, bits)


# ---- compaction edges, N = 32 ----------------------------------------------------------------------------------------------
def _awgn_rows(rng, B, N, db):
    sig = 10.0 ** (-db / 20.0)
    return 2.0 * (1.0 + sig * rng.standard_normal((B, N))) / sig / sig


@functools.lru_cache(maxsize=None)
def _edge_rows():
    rng = np.random.default_rng(17)
    clean = _awgn_rows(rng, 300, 32, 8.0)
    weak = 0.05 * rng.standard_normal((300, 32))
    mixed = _awgn_rows(rng, AD_CHUNK + 1, 32, 1.0)
    # of the weak rows, those that no graph of the default list settles within two round trips (by the model, row by row)
    from oracle import oracle_py as oracle
    code = oracle.Code(32, 16)
    res = M.bpl_decode(weak, code.frozen, code.info_order, M.cyclic_graphs(5, 5), 2)
    weak = weak[res.graph == 5][:200]
    assert len(weak) == 200
    # the one frame of the second compaction block is an open one
    tail = M.bpl_decode(mixed[-65:], code.frozen, code.info_order, M.cyclic_graphs(5, 5), 10)
    k = len(mixed) - 65 + int(np.flatnonzero(tail.graph >= 1)[-1])
    mixed[[k, -1]] = mixed[[-1, k]]
    return clean, weak, mixed


@pytest.mark.parametrize("case", ["B = 1", "B = AD_CHUNK + 1", "none open", "all open", "only the last open"])
def test_compaction_edges(case, oracle):
    import polardecoding_amd as pa
    N, K, n = 32, 16, 5
    code = oracle.Code(N, K)
    clean, weak, mixed = _edge_rows()
    it = 10
    if case == "B = 1":
        llr = mixed[:1]
    elif case == "B = AD_CHUNK + 1":
        llr = mixed
    elif case == "none open":
        llr = clean
    elif case == "all open":
        llr, it = weak, 2
    else:
        llr, it = np.concatenate([clean[:199], weak[:1]]), 2
    graphs = M.cyclic_graphs(n, n)
    res = M.bpl_decode(llr, code.frozen, code.info_order, graphs, it)
    if case == "none open":
        assert (res.graph == 0).all() and len(res.attempts) == 1
    if case == "all open":
        assert (res.graph == n).all() and (res.total == n * it).all()
    if case == "only the last open":
        assert (res.graph[:-1] == 0).all() and res.graph[-1] == n and res.attempts[1]["frames"].tolist() == [199]
    if case == "B = AD_CHUNK + 1":
        assert res.attempts[1]["frames"][-1] == AD_CHUNK and min(M.classes(res, n)) >= 1
    dec = pa.BPL(N, K, iterMax=it)
    _same(_bpl(dec, llr), _of_model(res), case)


# ---- consumers ---------------------------------------------------------------------------------------------------------------
def test_consumers_agree_with_the_bpl_entry_point(oracle):
    import torch
    import polardecoding_amd as pa
    N, K = 128, 64
    code, llr, ys, sigs, us, res, P = _model_set(N, 4228, 200, 20)
    dec = pa.BPL(N, K, iterMax=20)
    want = _bpl(dec, llr)
    _same(want, _of_model(res), "decode_bpl_device")
    uh, it, fl, gr, tot = dec.decode_bpl_batch(llr)
    _same((uh, it, fl, gr, tot), want, "decode_bpl_batch")
    uh, pm, fl = dec.decode_batch(llr)
    assert np.array_equal(uh, want[0]) and np.array_equal(fl, want[2]) and not pm.any()
    half, sig = 100, float(sigs[0])
    uh, pm, fl = dec.decode_batch_y(ys[:half], sig)
    assert np.array_equal(uh, want[0][:half]) and np.array_equal(fl, want[2][:half])
    open_frame = int(np.flatnonzero(res.graph[:half] >= 1)[0])
    for b in (0, open_frame):
        assert np.array_equal(dec(ys[b], sig), want[0][b])
    d = torch.from_numpy(llr).cuda()
    pmd = torch.full((200,), -1.0, dtype=torch.float64, device="cuda")
    fld = torch.full((200,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_device(d, pm=pmd, flags=fld)
    dec.synchronize()
    assert np.array_equal(_unpack(bits.cpu().numpy(), N), want[0]) and np.array_equal(fld.cpu().numpy(), want[2])
    assert not pmd.cpu().numpy().any()
    # the stop rule on host buffers
    io = code.info_order
    err = (want[0][:half][:, io] != us[:half][:, io]).sum(axis=1)
    assert (err > 0).sum() >= 2
    need = int((err > 0).sum()) // 2
    cut = int(np.flatnonzero(np.cumsum(err > 0) >= need)[0]) + 1
    assert dec.stop_rule_batch_y(ys[:half], sig, us[:half], need) == (cut, int((err[:cut] > 0).sum()), int(err[:cut].sum()))
    # fer_batch == generate -> decode -> count
    B = 6000
    blk, bit = dec.fer_batch(5, 0, 1.5, B)
    g = torch.empty((B, N), dtype=torch.float64, device="cuda")
    ub = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dec.generate_device(5, 0, 1.5, g, u_bits=ub)
    out = dec.decode_bpl_device(g)
    dec.count_errors_device(out, ub, cnt)
    dec.synchronize()
    assert (blk, bit) == tuple(int(v) for v in cnt.cpu().numpy()) and 0 < blk < B
    ms = dec.time_decode_device(g, out, 2)
    assert ms > 0
    # kernel name and ctx info
    assert "k_bp_w128<double> (stop rule G) x 7 graphs; glue k_bpl_gather, k_bpl_scatter" in dec.kernel_name
    vals = [C.c_int() for _ in range(6)]
    assert dec._lib.polar_ctx_info(dec._h, *[C.byref(v) for v in vals]) == 0
    assert [v.value for v in vals] == [N, K, K, 1, pa.ALGO_BPL, pa.F64]
    assert np.array_equal(dec.info_order, code.info_order)


def test_crc_aided_generator_and_counters_are_those_of_cascl():
    import torch
    import polardecoding_amd as pa
    N, K, B = 128, 64, 4000
    dec = pa.BPL(N, K, iterMax=20, crc_taps=CRC6)
    ca = pa.CASCL(N, K, L=8, crc_taps=CRC6)
    g1, g2 = (torch.empty((B, N), dtype=torch.float64, device="cuda") for _ in range(2))
    u1, u2 = (torch.empty((B, N // 32), dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    dec.generate_device(3, 0, 2.0, g1, u_bits=u1)
    ca.generate_device(3, 0, 2.0, g2, u_bits=u2)
    dec.synchronize()
    ca.synchronize()
    assert torch.equal(g1, g2) and torch.equal(u1, u2)
    uh, it, fl, gr, tot = _bpl(dec, g1)
    ok = (fl & FLAG_CRC_PASS) != 0
    assert ((gr < 7) == (ok & ((fl & FLAG_BP_CONVERGED) != 0))).all() and 0 < ok.sum() < B
    blk, bit = dec.fer_batch(3, 0, 2.0, B)
    sent = _unpack(u1.cpu().numpy(), N)
    io = dec.info_order
    err = (uh[:, io] != sent[:, io]).sum(axis=1)
    assert (blk, bit) == (int((err > 0).sum()), int(err.sum()))


def test_rate_matched_context_decodes_the_recovered_row():
    import torch
    import polardecoding_amd as pa
    N, K, E, B = 128, 40, 100, 3000
    dec = pa.BPL(N, K, iterMax=20, E=E)
    assert dec.rm_mode != pa.RM_NONE and dec.kernel_name.startswith("k_rm_recover, then ")
    plain = pa.BPL(N, K, iterMax=20, info_order=dec.info_order)
    g = torch.empty((B, E), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dec.generate_device(8, 0, 1.0, g)
    rows = dec.rm_recover_device(g)
    dec.synchronize()
    want = _bpl(plain, rows)
    assert min((want[3] == 0).sum(), ((want[3] >= 1) & (want[3] < 7)).sum()) >= 1
    _same(_bpl(dec, g), want, "rate matched")


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable(oracle):
    import torch
    import polardecoding_amd as pa
    N, K, n = 128, 64, 7
    code, llr, ys, sigs, us, res, P = _model_set(N, 4228, 200, 20)
    dec = pa.BPL(N, K, iterMax=20)
    d = torch.from_numpy(llr).cuda()
    refused = [lambda: dec.set_bp_stop("g"), lambda: dec.set_bp_stop(None), lambda: dec.decode_bp_device(d),
               lambda: dec.decode_bp_batch(llr), lambda: dec.set_cascl_stages((1, 8)), lambda: dec.decode_cascl_device(d),
               lambda: dec.decode_cascl_batch(llr), lambda: dec.set_scf_flips(4), lambda: dec.decode_scf_device(d),
               lambda: dec.decode_scf_batch(llr), lambda: dec.set_scan_iters(2), lambda: dec.decode_scan_device(d),
               lambda: dec.decode_scan_batch(llr), lambda: dec.set_quant(2.0), lambda: dec.quant,
               lambda: dec.decode_q8_device(torch.zeros((4, N), dtype=torch.int8, device="cuda")),
               lambda: dec.set_systematic(True), lambda: dec.decode_batch(llr, frozen_mask=code.frozen),
               lambda: dec.bp_readout_device(d, torch.zeros((200, N // 32), dtype=torch.int32, device="cuda"), [3],
                                             torch.zeros((1, n + 1), dtype=torch.int64, device="cuda"))]
    for k, call in enumerate(refused):
        with pytest.raises(pa.PolarError):
            call()
            pytest.fail(f"call {k} was not refused")
    # malformed lists: the ctx keeps its list
    before = dec.bpl_graphs
    ident = list(range(n))
    for bad in ([[0, 1, 2, 3, 4, 5, 5]], [[0, 1, 2, 3, 4, 5, 7]], [[-1, 1, 2, 3, 4, 5, 6]], [ident, [1, 1, 2, 3, 4, 5, 6]],
                np.zeros((0, n), dtype=np.int32), [ident] * 33):
        with pytest.raises(pa.PolarError):
            dec.set_bpl_graphs(bad)
    assert np.array_equal(dec.bpl_graphs, before)
    # polar_bpl_* on other contexts; contexts that cannot be BPL
    bp = pa.BP(N, K, iterMax=20, early_stop="g")
    for call in (lambda: bp.set_bpl_graphs([ident]), lambda: bp.bpl_graphs, lambda: bp.decode_bpl_device(d),
                 lambda: bp.decode_bpl_batch(llr), lambda: pa.SCLdecode(N, K).decode_bpl_batch(llr)):
        with pytest.raises(pa.PolarError):
            call()
    with pytest.raises(pa.PolarError):
        pa.BPL(N, K, dtype=pa.Q8)
    with pytest.raises(pa.PolarError):
        pa.BPL(N, K, iterMax=0)
    with pytest.raises(pa.PolarError):
        pa.Decoder(N, K, pa.ALGO_BPL, dyn=([0], [[]]))
    with pytest.raises(pa.PolarError):
        pa.Decoder(N, K, pa.ALGO_BPL, crc_file=os.path.join(HERE, "golden", "CRC_6.dat"))
    _same(_bpl(dec, llr), _of_model(res), "after the refusals")
    # a call while the ctx stream is capturing: POLAR_EINVAL, nothing captured
    out = torch.empty((len(llr), N // 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    was_refused = False
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dec.use_torch_stream()
        with torch.cuda.graph(g, stream=s):
            out.zero_()
            try:
                dec.decode_bpl_device(d, out_bits=out)
            except pa.PolarError:
                was_refused = True
    torch.cuda.synchronize()
    dec.use_torch_stream()
    assert was_refused
    del g
    _same(_bpl(dec, llr), _of_model(res), "after the capture")


def test_polar_sim_bpl():
    """the C harness: --algo bpl with and without --fast, --graphs and --crc; BLER falls with the list"""
    import re
    import subprocess
    sim = os.path.join(os.path.dirname(HERE), "polardecoding_amd", "lib", "polar_sim")
    base = [sim, "--algo", "bpl", "--N", "128", "--K", "64", "--bp-iters", "30", "--snr", "2.0:2.0:0.5", "--ble", "300",
            "--batch", "8192", "--fast"]
    bler = {}
    for P in ("1", "7"):
        r = subprocess.run(base + ["--graphs", P], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        bler[P] = float(re.search(r"BLER = ([0-9.e+-]+)", r.stdout).group(1))
    assert 0 < bler["7"] < bler["1"] < 0.5, bler
    r = subprocess.run(base[:-1] + ["--graphs", "4", "--crc", "6", "--ble", "20"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "BLER" in r.stdout, r.stderr
    r = subprocess.run(base + ["--graphs", "33"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--graphs" in r.stderr
    r = subprocess.run([sim, "--algo", "bp", "--N", "128", "--K", "64", "--graphs", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--graphs" in r.stderr
