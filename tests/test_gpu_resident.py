"""GPU: every persistent kernel's second, third and ragged last job at small batches, frame for frame against its model.

polardecoding_amd.testing.resident_blocks() caps the grid of one context, so that the rows of tests/resident_cases.py (held to
their conditions by tests/test_resident_host.py) put a few dozen frames through a wavefront's later jobs: state that was not
initialised again, a scratch line still cached from the frame before, a ragged last job that arrives through the counter, a
counter that does not return to zero.  For every row and cap, on one context:

  the cap took effect   polar_testing_last_plan reports grid == cap, the row's jobs per block, and the work queue exactly when
                        there are more jobs than slots (never for the fixed-stride kernels, which then have jobs > slots)
  every frame of every output of the three batch sizes equals the model (the oracle, or the kernel's numpy model), by ==
  position independence the largest batch in reversed order returns the reversed outputs
  counter reset         the largest batch three times with nothing in between, and an uncapped launch of 7 frames between the
                        first and the second
  output bounds         the outputs are views into a guarded arena (tests/extents.py)

Then one capped k_scan_lanes launch captured in a graph and replayed, and the hook itself."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import extents as X  # noqa: E402
import resident_cases as RC  # noqa: E402

FLAG_TIE = 1
WRAPPED = ("scf", "dscf")   # the last plan of these decodes is a later pass over the failing frames, not the whole batch


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _make(row):
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    s = row.spec
    kw = {"dtype": pa.F32 if s.get("f32") else pa.F64}
    taps = RC.taps_of(row)
    if s.get("own_order"):
        kw["info_order"] = RC.info_order(row.N, row.K + (max(taps) if taps else 0))
    if row.kind == "fam":
        _, c, made = RC.family_case(row)
        algo = {"SC": pa.ALGO_SC, "SCL": pa.ALGO_SCL, "CASCL": pa.ALGO_CASCL}[c.algo]
        K = made.order.size - (max(made.taps) if made.taps else 0)
        dec = pa.Decoder(c.N, K, algo, L=c.L, crc_taps=made.taps, info_order=made.order, dyn=made.dyn, **kw)
        assert np.array_equal(dec.info_order, made.order)
    elif row.kind in ("list", "listout"):
        dec = pa.CASCL(row.N, row.K, L=s["L"], crc_taps=taps, **kw) if taps else pa.SCLdecode(row.N, row.K, L=s["L"], **kw)
    elif row.kind == "sc":
        dec = pa.SCdecode(row.N, row.K, **kw)
    elif row.kind in ("bp", "bpstop"):
        dec = pa.BP(row.N, row.K, iterMax=s["iters"], early_stop="g" if row.kind == "bpstop" else None, **kw)
    elif row.kind == "scan":
        dec = pa.SCAN(row.N, row.K, iters=s["I"], **kw)
    elif row.kind == "scf":
        dec = pa.SCFlip(row.N, row.K, T=s["T"], crc_taps=taps, **kw)
    elif row.kind == "dscf":
        dec = pa.DSCFlip(row.N, row.K, budgets=s["budgets"], c=s["c"], tau=RC.TAU, crc_taps=taps, **kw)
    elif row.kind == "q8":
        dec = pa.CASCL(row.N, row.K, L=s["L"], crc_taps=taps, dtype=pa.Q8)
    else:
        raise ValueError(row.kind)
    if "variant" in s:
        T.select_kernel(dec, s["variant"])
    return dec


def _outputs(row, B):
    """(name, dtype, elements per frame) of the entry point's per-frame outputs"""
    NW, soft = row.N // 32, ("float32" if row.spec.get("f32") else "float64")
    bits = ("bits", "int32", NW)
    L = row.spec.get("L", 0)
    return {"fam": [bits, ("pm", "float64", 1), ("flags", "int32", 1)],
            "listout": [("paths", "int32", L * NW), ("pm", "float64", L), ("rem", "int32", L), ("count", "int32", 1), ("flags", "int32", 1)],
            "list": [bits, ("pm", "float64", 1), ("flags", "int32", 1)], "q8": [bits, ("pm", "float64", 1), ("flags", "int32", 1)],
            "sc": [bits], "bp": [bits], "bpstop": [bits, ("iters", "int32", 1), ("flags", "int32", 1)],
            "scan": [bits, ("llr_u", soft, row.N), ("ext_x", soft, row.N)],
            "scf": [bits, ("flags", "int32", 1), ("attempts", "int32", 1)],
            "dscf": [bits, ("flags", "int32", 1), ("attempts", "int32", 1), ("sets", "int32", 3)]}[row.kind]


def _run(row, dec, x):
    """one launch on rows x: the model's tuple from outputs carved out of a guarded arena, and the arena's verdict"""
    import torch
    import polardecoding_amd as pa
    B = len(x)
    outs = _outputs(row, B)
    group = max(row.u, 1)
    arena = X.Arena("torch", X.Arena.need([(dt, B * per, group, per) for _, dt, per in outs]))
    t = {}
    for name, dt, per in outs:
        v = arena.carve(name, dt, B * per, group, per)
        t[name] = v.view(B, per) if per > 1 else v
    if "bits" in t:
        t["bits"] = t["bits"].view(B, row.N // 32)
    d = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32 if row.spec.get("f32") else np.float64)).cuda()
    sigma = row.spec.get("sigma", 0.0)
    torch.cuda.synchronize()
    if row.kind == "listout":   # polar_list_decode on the arena's views
        rc = dec._lib.polar_list_decode(dec._h, C.c_void_p(d.data_ptr()), 0, 0.0, B,
                                        *[C.c_void_p(t[k].data_ptr()) for k in ("paths", "pm", "rem", "count", "flags")])
        assert rc == 0, rc
    elif row.kind in ("list", "q8", "fam"):
        dec.decode_device(d, sigma=sigma, out_bits=t["bits"], pm=t["pm"], flags=t["flags"])
    elif row.kind in ("sc", "bp"):
        dec.decode_device(d, out_bits=t["bits"])
    elif row.kind == "bpstop":
        dec.decode_bp_device(d, out_bits=t["bits"], iters=t["iters"], flags=t["flags"])
    elif row.kind == "scan":
        dec.decode_scan_device(d, out_bits=t["bits"], llr_u=t["llr_u"], ext_x=t["ext_x"])
    elif row.kind == "scf":
        dec.decode_scf_device(d, out_bits=t["bits"], flags=t["flags"], attempts=t["attempts"])
    else:
        dec.decode_scf_sets_device(d, out_bits=t["bits"], flags=t["flags"], attempts=t["attempts"], sets=t["sets"])
    dec.synchronize()
    h = {k: v.cpu().numpy() for k, v in t.items()}
    uh = _unpack(h["bits"], row.N) if "bits" in h else None
    if row.kind == "listout":
        L = row.spec["L"]
        got = (_unpack(h["paths"], row.N).reshape(B, L, row.N), h["pm"], h["rem"].view(np.uint32), h["count"].view(np.uint32),
               h["flags"].view(np.uint32))
    elif row.kind == "fam":
        got = (uh, h["pm"], h["flags"].view(np.uint32))
    elif row.kind == "list":
        pm = h["pm"].astype(np.float32) if row.spec.get("f32") else h["pm"]
        got = (uh, pm, (h["flags"].view(np.uint32) & FLAG_TIE) != 0)
    elif row.kind == "q8":
        got = (uh, h["pm"].astype(np.int64), h["flags"].view(np.uint32))
    elif row.kind in ("sc", "bp"):
        got = (uh,)
    elif row.kind == "bpstop":
        got = (uh, h["iters"].astype(np.int64), h["flags"].view(np.uint32) == pa.FLAG_BP_CONVERGED)
    elif row.kind == "scan":
        got = (uh, h["llr_u"], h["ext_x"])
    elif row.kind == "scf":
        got = (uh, h["flags"].view(np.uint32).astype(np.int64), h["attempts"].astype(np.int64))
    else:
        got = (uh, h["flags"].view(np.uint32).astype(np.int64), h["attempts"].astype(np.int64), h["sets"].astype(np.int64))
    return got, arena.check()


def _same(got, want, label):
    assert len(got) == len(want), label
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        if g.dtype.kind == "f":
            assert g.dtype == w.dtype, (label, k, g.dtype, w.dtype)
            assert not np.isnan(g).any(), (label, k, "NaN")
            assert np.array_equal(np.isinf(g), np.isinf(w)), (label, k, "infinities")
        bad = np.flatnonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1))
        assert bad.size == 0, f"{label}: output {k} differs from the model at frames {bad[:10]} ({bad.size} of {len(g)})"


def _cut(want, n, rev=False):
    return tuple(np.asarray(a)[:n][::-1] if rev else np.asarray(a)[:n] for a in want)


def _stride_holds(dec, cap, need=None, label=""):
    """the last fixed-stride launch that sizes its own grid took the cap; need given: the blocks its work needs, more than cap"""
    from polardecoding_amd import testing as T
    grid, blocks = T.last_stride(dec)
    assert blocks >= 1 and grid == min(cap, blocks), (label, grid, blocks)
    if need is not None:
        assert blocks == need and need > cap, (label, grid, blocks, need)


def _plan_holds(row, dec, cap, B, label):
    from polardecoding_amd import testing as T
    grid, jobs, jpb, queued = T.last_plan(dec)
    print(f"PLAN {label}: (grid {grid}, jobs {jobs}, jobs_per_block {jpb}, queued {queued})")
    assert jpb == row.jpb, (label, "jobs per block", jpb)
    if row.kind in WRAPPED:
        assert jobs >= 1 and grid == min(cap, -(-jobs // jpb)), (label, grid, jobs)   # pass B: (failing frame, flip) pairs
        _stride_holds(dec, cap, label=label + " k_scf_resolve")
    else:
        assert jobs == RC.jobs(row, B), (label, jobs)
        assert grid == cap, (label, "grid", grid)
        if "bp_global" in row.name and B > cap:
            _stride_holds(dec, cap, need=B, label=label)
    more = jobs > grid * jpb
    assert queued == (1 if more and row.queue else 0), (label, "queued", queued)
    return more


@pytest.mark.parametrize("cap", RC.CAPS)
@pytest.mark.parametrize("row", RC.ROWS, ids=[r.name for r in RC.ROWS])
def test_later_jobs_equal_the_model(row, cap, oracle):
    from polardecoding_amd import testing as T
    x, want = RC.pool(oracle, row), RC.want(oracle, row)
    dec = _make(row)
    try:
        if row.N <= 1024 and row.kind != "fam":
            assert np.array_equal(dec.info_order, RC.code_of(oracle, row).info_order)
        T.resident_blocks(dec, cap)
        B0, B1, B2 = RC.batches(row, cap)
        for B in (B0, B1, B2):
            label = f"{row.name} cap {cap} B {B}"
            got, stray = _run(row, dec, x[:B])
            assert dec.kernel_name.startswith(row.prefix), (label, dec.kernel_name)
            more = _plan_holds(row, dec, cap, B, label)
            if row.kind not in WRAPPED:
                assert more == (B > B0), label
            assert stray == [], (label, "a store outside the outputs", stray)
            _same(got, _cut(want, B), label)
        got, stray = _run(row, dec, x[:B2][::-1])
        assert stray == []
        _same(got, _cut(want, B2, rev=True), f"{row.name} cap {cap} reversed")
        for rep in range(3):   # every launch leaves the counter at zero for the next one
            got, stray = _run(row, dec, x[:B2])
            assert stray == []
            _same(got, _cut(want, B2), f"{row.name} cap {cap} launch {rep}")
            if rep == 0:
                T.resident_blocks(dec, 0)
                got, _ = _run(row, dec, x[:7])
                _same(got, _cut(want, 7), f"{row.name} uncapped B 7")
                T.resident_blocks(dec, cap)
    finally:
        dec.close()


def test_a_captured_capped_scan_launch_replays(oracle):
    """one capped k_scan_lanes launch (three rounds and a ragged job on one workgroup) captured in a graph: every replay
    returns the model's outputs, so the queue is back at zero without a host-side step"""
    import torch
    from polardecoding_amd import testing as T
    row = next(r for r in RC.SCAN_ROWS if r.N == 128 and not r.spec.get("f32"))
    B = RC.batches(row, 1)[2]
    x, want = RC.pool(oracle, row)[:B], _cut(RC.want(oracle, row), B)
    dec = T.resident_blocks(_make(row), 1)
    try:
        d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dec.use_torch_stream()
            bits = torch.full((B, row.N // 32), -1, dtype=torch.int32, device="cuda")
            lu = torch.full((B, row.N), float("nan"), dtype=torch.float64, device="cuda")
            ex = torch.full((B, row.N), float("nan"), dtype=torch.float64, device="cuda")
            dec.decode_scan_device(d, out_bits=bits, llr_u=lu, ext_x=ex)   # every allocation is done before the capture
            s.synchronize()
            assert T.last_plan(dec) == (1, RC.jobs(row, B), row.jpb, 1)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                dec.use_torch_stream()
                dec.decode_scan_device(d, out_bits=bits, llr_u=lu, ext_x=ex)
            for rep in range(3):
                bits.fill_(-1)
                lu.fill_(float("nan"))
                ex.fill_(float("nan"))
                g.replay()
                torch.cuda.synchronize()
                _same((_unpack(bits.cpu().numpy(), row.N), lu.cpu().numpy(), ex.cpu().numpy()), want, f"replay {rep}")
    finally:
        dec.close()


# ---- the hook itself --------------------------------------------------------------------------------------------------------
def test_setter_and_getter_refuse_null_and_negative_and_zero_restores(oracle):
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    lib = pa.load_library(testing=True)
    lib.polar_testing_resident_blocks.argtypes = [C.c_void_p, C.c_int]
    lib.polar_testing_last_plan.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    assert lib.polar_testing_resident_blocks(None, 1) == -1   # POLAR_EINVAL
    assert lib.polar_testing_last_plan(None, None, None, None, None) == -1
    row = RC.SC_ROWS[2]
    x, want = RC.pool(oracle, row), RC.want(oracle, row)
    dec = _make(row)
    try:
        T.resident_blocks(dec, 2)
        assert lib.polar_testing_resident_blocks(dec._h, -1) == -1
        assert lib.polar_testing_last_plan(dec._h, None, None, None, None) == 0   # every pointer may be null
        B = RC.batches(row, 2)[2]
        _same(_run(row, dec, x[:B])[0], _cut(want, B), "cap 2")
        assert T.last_plan(dec) == (2, RC.jobs(row, B), row.jpb, 1)           # the refused value changed nothing
        assert T.resident_blocks(dec, 0)._resident_blocks == 0
        _same(_run(row, dec, x[:B])[0], _cut(want, B), "restored")
        grid, jobs, jpb, queued = T.last_plan(dec)
        assert (grid, jobs, jpb, queued) == (-(-RC.jobs(row, B) // row.jpb), RC.jobs(row, B), row.jpb, 0)   # a block per four jobs
    finally:
        dec.close()


def test_cap_survives_a_context_re_creation_and_changes_no_result(oracle):
    """the cap is set while the context still lives in the product library: resident_blocks() re-creates it inside the test
    library, and select_kernel() after it keeps it; the same frames at caps 1, 2, 5, 64 and none return the same outputs"""
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    row = RC.LIST_ROWS[0]
    x, want = RC.pool(oracle, row), RC.want(oracle, row)
    B = RC.pool_size(row)
    dec = pa.CASCL(row.N, row.K, L=row.spec["L"], crc_taps=RC.taps_of(row))
    try:
        assert dec._lib is pa.load_library()
        T.resident_blocks(dec, 1)
        assert dec._lib is pa.load_library(testing=True) and dec._resident_blocks == 1
        _same(_run(row, dec, x)[0], want, "cap 1")
        assert T.last_plan(dec) == (1, B, row.jpb, 1)
        with pytest.raises(pa.PolarError, match="test-only cap"):   # the product library has no hook to apply the cap with
            dec._rebind(pa.load_library())
        assert dec._lib is pa.load_library(testing=True)            # refused before anything was closed
        T.resident_blocks(dec, 0)
        dec._rebind(pa.load_library())
        _same(_run(row, dec, x)[0], want, "product library")
        dec._resident_blocks = 3
        T.select_kernel(dec, T.KERNEL_AUTO)      # re-created in the test library: api.py applies the cap again
        _same(_run(row, dec, x)[0], want, "cap 3 after a re-creation")
        assert T.last_plan(dec) == (3, B, row.jpb, 1)
        for cap in (2, 5, 64, 0):
            T.resident_blocks(dec, cap)
            _same(_run(row, dec, x)[0], want, f"cap {cap}")
            grid = T.last_plan(dec)[0]
            assert grid == (min(cap, -(-B // row.jpb)) if cap else -(-B // row.jpb)), (cap, grid)
    finally:
        dec.close()


# ---- kernels whose output is a sum over the batch ---------------------------------------------------------------------------
@pytest.mark.parametrize("cap", RC.CAPS)
def test_genie_counters_under_the_cap(cap, oracle):
    """k_genie_lanes (jobs of 64 frames, four per block) and k_genie_rows (fixed stride): the leaf-sign counters of three
    rounds and a ragged job against the counting model of tests/test_construct_host.py on the device's own design rows,
    which are the uncapped launch's rows value for value"""
    import torch
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    import test_construct_host as GM
    N, seed, first, sigma = 128, 77, 5_000_000_000, 0.9
    B = 3 * cap * 4 * 64 + 64 + 37
    dec = pa.SCdecode(N, N // 2)
    try:
        T.resident_blocks(dec, 0)
        rows = torch.empty((B, N), dtype=torch.float64, device="cuda")
        dec.genie_rows_device(seed, first, sigma, rows)
        dec.synchronize()
        xh = rows.cpu().numpy()
        T.resident_blocks(dec, cap)
        rows.fill_(-1.0)
        torch.cuda.synchronize()
        dec.genie_rows_device(seed, first, sigma, rows)   # 128 B / 2 pairs on cap * 256 threads: many trips of the stride loop
        dec.synchronize()
        assert np.array_equal(rows.cpu().numpy(), xh)
        err, tie, _, _ = GM.genie_model(oracle, xh, np.float64)
        want = np.stack([err, tie]).astype(np.uint64)
        assert want[0].sum() > 0
        for rep in range(3):
            c = torch.zeros((2, N), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            dec.genie_count_device(rows, c)
            dec.synchronize()
            assert T.last_plan(dec) == (cap, -(-B // 64), 4, 1)
            assert np.array_equal(c.cpu().numpy().view(np.uint64), want), rep
        c = torch.zeros((2, N), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        dec.construct_batch(seed, first, sigma, B, c)
        dec.synchronize()
        _stride_holds(dec, cap, need=-(-B * N // 2 // 256), label="k_genie_rows")   # a thread per pair of values
        assert np.array_equal(c.cpu().numpy().view(np.uint64), want)
    finally:
        dec.close()


def _pack(u):
    u = np.asarray(u, dtype=np.uint32)
    B, N = u.shape
    return (u.reshape(B, N // 32, 32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64).astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("cap", RC.CAPS)
def test_bp_readout_under_the_cap(cap, oracle):
    """k_bp_readout (one frame per block, fixed stride) at N = 128: decisions frame for frame and the read-out table summed
    over the batch against oracle.bp_readout"""
    import torch
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    N, K, iters, cp = 128, 64, 12, [1, 4, 12]
    B = 3 * cap + 1
    code = oracle.Code(N, K)
    us, llr = [], []
    for k, db in enumerate((-1.0, 1.0, 3.0)):
        sig = oracle.sigma_from_db(db)
        u, ys = oracle.Sim(4220 + k).frames(code, sig, -(-B // 3))
        us += list(u)
        llr += [oracle.llr_from_y(y, sig) for y in ys]
    us, llr = np.stack(us)[:B], np.stack(llr)[:B]
    ref_uh, ref_E = oracle.bp_readout(code, llr, us, iters, cp)
    wrong = (ref_uh != us).any(axis=1)
    assert wrong.any() and not wrong.all() and ref_E.any()
    dec = T.resident_blocks(pa.BP(N, K, iterMax=iters), cap)
    try:
        for rep in range(2):
            E = torch.zeros(len(cp), code.n + 1, dtype=torch.int64, device="cuda")
            out = torch.full((B, N // 32), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            dec.bp_readout_device(torch.from_numpy(llr).cuda(), torch.from_numpy(_pack(us)).cuda(), cp, E, out_bits=out)
            dec.synchronize()
            assert T.last_plan(dec) == (cap, B, 1, 0)
            _stride_holds(dec, cap, need=B, label="k_bp_readout")
            assert np.array_equal(E.cpu().numpy(), ref_E), rep
            assert np.array_equal(_unpack(out.cpu().numpy(), N), ref_uh), rep
    finally:
        dec.close()


# ---- wrappers and glue: the assertions of their own modules, with the cap set -------------------------------------------------
@pytest.mark.parametrize("cap", RC.CAPS)
def test_adaptive_cascl_under_the_cap(cap, oracle):
    """stages (1, 2, 8) at N = 128 on the frames of tests/chunk_cases.py: the SC stage, the L = 2 stage context and the
    context's own L = 8 decoder run capped (the cap is copied to the stage contexts), with k_ad_crc_check, k_ad_gather and
    k_ad_scatter on a capped grid.  A stage context's plan is read through its owner: after the whole batch that is the
    L = 8 stage on the frames that reached it, after a batch that ends at an earlier stage that stage's"""
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    import chunk_cases as CC
    import test_gpu_cascl_adaptive as AD
    x, want = CC.ad_rows(oracle, "ragged"), CC.ad_want(oracle, "ragged")
    last = int(CC.ad_stage_fails(oracle, x, "f64")[-1].sum())
    assert last > 3 * cap * 4
    dec = pa.CASCL(CC.AD_N, CC.AD_K, L=CC.AD_STAGES[-1], crc_taps=CC.CRC6, stages=CC.AD_STAGES)
    try:
        T.resident_blocks(dec, cap)
        assert dec.cascl_stages == CC.AD_STAGES
        for rep in range(2):
            AD._same(AD._adaptive(dec, x), want, f"cap {cap} launch {rep}", rerank_free=True)
            assert T.last_plan(dec) == (cap, last, 4, 1)   # k_scl_fast<N=128>: one frame per wavefront, four per block
            _stride_holds(dec, cap, label="k_ad_scatter")
        # the stage contexts: a batch that ends after stage 0, or after stage 1, leaves that stage's plan as the last one
        fails = CC.ad_stage_fails(oracle, x, "f64")
        pass0, only1 = np.flatnonzero(~fails[0]), np.flatnonzero(fails[0] & ~fails[1])
        n1 = 3 * cap + 1
        assert pass0.size >= n1 and only1.size >= n1
        few = pass0[:n1]                                   # below 64 frames the SC stage is k_scl_generic: one job per block
        lanes = np.resize(pass0, 3 * cap * 4 * 64 + 64 + 37)   # k_sc_lanes: jobs of 64 frames, four per block
        mixed = np.sort(np.concatenate([pass0[:5], only1[:n1]]))
        for idx, plan, what in ((few, (cap, n1, 1, 1), "SC stage, k_scl_generic"),
                                (lanes, (cap, -(-lanes.size // 64), 4, 1), "SC stage, k_sc_lanes"),
                                (mixed, (cap, n1, 1, 1), "L = 2 stage")):
            AD._same(AD._adaptive(dec, x[idx]), tuple(np.asarray(w)[idx] for w in want), f"cap {cap} {what}", rerank_free=True)
            assert T.last_plan(dec) == plan, (what, T.last_plan(dec))
    finally:
        dec.close()


@pytest.mark.parametrize("cap", RC.CAPS)
def test_bpl_under_the_cap(cap, oracle):
    """BPL at N = 128 with CRC-6 (tests/chunk_cases.py): k_bp_w128 on gathered rows, k_bpl_gather and k_bpl_scatter capped"""
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    import chunk_cases as CC
    import test_gpu_bpl as BT
    case = CC.BPL_CASES[-1]
    N, K, iters, which, taps = case.spec[:5]
    x, res = CC.bpl_rows(oracle, case), CC.bpl_want(oracle, case)
    open_frames = [len(a["frames"]) for a in res.attempts]
    assert len(open_frames) > 2 and open_frames[1] > 3 * cap * 4   # attempt 1 runs three rounds and more on gathered rows
    dec = pa.BPL(N, K, iterMax=iters, crc_taps=taps)
    try:
        T.resident_blocks(dec, cap)
        for rep in range(2):
            BT._same(BT._bpl(dec, x), BT._of_model(res), f"cap {cap} launch {rep}")
            grid, jobs, jpb, queued = T.last_plan(dec)
            assert jobs == open_frames[-1] and jpb == 4, (grid, jobs, jpb, queued)   # the last attempt's launch
            assert grid == min(cap, -(-jobs // 4)) and queued == (jobs > grid * 4), (grid, jobs, jpb, queued)
            _stride_holds(dec, cap, label="k_bpl_scatter")
    finally:
        dec.close()


@pytest.mark.parametrize("cap", RC.CAPS)
def test_rate_matched_decode_under_the_cap(cap, oracle):
    """E = 100 at N = 128: k_rm_recover (one frame per block, fixed stride) in front of a capped SCL decode, against the oracle
    on test_rm_host.recover()'s rows"""
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    import test_rm_host as RM
    N, K, E, L = 128, 40, 100, 8
    B = 3 * cap * 4 + 1
    rng = np.random.default_rng(100)
    sig = 10.0 ** (-rng.uniform(0.0, 3.0, size=(B, 1)) / 20.0)
    x = RC.f32_exact(2.0 * (1.0 + sig * rng.standard_normal((B, E))) / sig / sig)
    x[2::3] = RC.f32_exact(rng.normal(0.0, 2.0, size=x[2::3].shape))
    dec = pa.SCLdecode(N, K, L=L, E=E)
    try:
        io = pa.rm_info_order(N, K, E)
        assert np.array_equal(dec.info_order, io)
        code = oracle.Code(N, K, None, Q=[j for j in range(N) if j not in set(io.tolist())] + io.tolist())
        wide = RM.recover(x, N, dec.A, 0)
        uh, pm, ties = oracle.decode(code, wide, "SCL", L=L)
        assert np.unique(pm).size > B // 2
        T.resident_blocks(dec, cap)
        row = RC.LIST_ROWS[0]._replace(N=N)   # the outputs and the comparison of a list row
        for rep in range(2):
            got, stray = _run(row, dec, x)
            assert stray == []
            _same(got, (uh, pm, ties > 0), f"cap {cap} launch {rep}")
            assert T.last_plan(dec) == (cap, B, 4, 1)
            _stride_holds(dec, cap, need=B, label="k_rm_recover")   # one frame per block
    finally:
        dec.close()


@pytest.mark.parametrize("cap", RC.CAPS)
@pytest.mark.parametrize("cid", ["crc6-128-65", "pac-128-64", "shorten-128-40-E100"])
def test_generators_under_the_cap(cid, cap):
    """k_generate, k_generate_dyn and k_generate_rm (four frames per block, fixed stride): u bits by == and every value within
    the bound of tests/gen_model.py, three trips of the frame loop and a ragged one, across frame 2^32"""
    from polardecoding_amd import testing as T
    import test_gpu_generator_values as GV
    c = GV.Case(cid)
    try:
        T.resident_blocks(c.dec, cap)
        B = 3 * cap * 4 + 5
        seed, first = GV.EDGES[0][0], 2 ** 32 - 3
        frames = GV.G.frames_of(first, B)
        u, x = c.bits(seed, frames)
        for f32, out_is_y, snr in ((False, False, 1.5), (True, True, -3.0)):
            got, du = c.run(seed, first, B, snr, f32=f32, out_is_y=out_is_y)
            assert np.array_equal(du, u), (cid, "u bits")
            ref, bound = GV.G.channel(x, c.z(seed, frames), GV.G.sigma_of(snr), out_is_y)
            GV._check_values(c.kernel, got, ref, bound, (cid, "cap", cap, snr))
            _stride_holds(c.dec, cap, need=-(-B // 4), label=c.kernel)   # four frames per block
    finally:
        c.dec.close()


@pytest.mark.parametrize("cap", RC.CAPS)
def test_count_errors_under_the_cap(cap):
    """k_count_errors (one frame per wavefront, fixed stride over the grid's wavefronts) against a numpy count"""
    import torch
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    N, K = 128, 64
    B = 3 * cap * 4 + 3
    rng = np.random.default_rng(cap)
    u = (rng.random((B, N)) < 0.5).astype(np.uint32)
    uh = u ^ ((rng.random((B, N)) < 0.02) & (np.arange(B)[:, None] % 3 != 0)).astype(np.uint32)
    dec = T.resident_blocks(pa.SCdecode(N, K), cap)
    try:
        info = np.zeros(N, dtype=bool)
        info[dec.info_order] = True
        per = ((u != uh) & info[None, :]).sum(axis=1)
        assert (per > 0).any() and (per == 0).any()
        for rep in range(2):
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            fe = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            dec.count_errors_device(torch.from_numpy(_pack(uh)).cuda(), torch.from_numpy(_pack(u)).cuda(), cnt, frame_err=fe)
            dec.synchronize()
            assert np.array_equal(fe.cpu().numpy(), per), rep
            _stride_holds(dec, cap, need=-(-B // 4), label="k_count_errors")   # four frames per block
            assert cnt.cpu().tolist() == [int((per > 0).sum()), int(per.sum())], rep
    finally:
        dec.close()


@pytest.mark.parametrize("cap", RC.CAPS)
def test_list_glue_under_the_cap(cap, oracle):
    """k_list_soft (one frame per block, fixed stride) capped; k_list_select and k_list_gather have one thread per element and
    keep their grids.  All three against tests/list_model.py on the device's own list, which equals the model's"""
    import torch
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    import list_model as LM
    N, K, L = 64, 32, 8
    B = 3 * cap + 1
    code = oracle.Code(N, K, RC.CRC6)
    sig = oracle.sigma_from_db(1.0)
    _, ys = oracle.Sim(640).frames(code, sig, B)
    x = RC.f32_exact(np.stack([oracle.llr_from_y(y, sig) for y in ys]))
    paths, pm, rem, count, flags = LM.list_model(code.frozen, None, x, L, crc=(code.info_order, RC.CRC6), oracle=oracle)
    dec = pa.CASCL(N, K, L=L, crc_taps=RC.CRC6)
    try:
        assert np.array_equal(dec.info_order, code.info_order)
        T.resident_blocks(dec, cap)
        t = dec.decode_list_device(torch.from_numpy(x).cuda())
        dec.synchronize()
        assert T.last_plan(dec) == (cap, B, 1, 1)   # k_scl_list: three rounds and one job
        assert np.array_equal(LM.unpack(t[0].cpu().numpy(), N), paths) and np.array_equal(t[1].cpu().numpy(), pm)
        assert np.array_equal(t[2].cpu().numpy().view(np.uint32), rem) and np.array_equal(t[3].cpu().numpy().view(np.uint32), count)
        present = int(rem[B - 1, 1])
        masks = np.array([0, present, 0x3F], dtype=np.int32)
        idx = dec.list_select_device(t[2], t[3], torch.from_numpy(masks).cuda())
        row = dec.list_gather_device(t[0], idx[:, 0])
        soft = dec.list_soft_device(t[0], t[1], t[3], rem=t[2], want_rem=0, domain=1, clamp=16.0)
        dec.synchronize()
        assert T.last_plan(dec) == (cap, B, 1, 0)   # k_list_soft
        idx = idx.cpu().numpy()
        assert np.array_equal(idx, LM.select(rem, count, masks.view(np.uint32))) and (idx[:, 0] >= 0).any()
        assert np.array_equal(LM.unpack(row.cpu().numpy(), N), LM.gather(paths, idx[:, 0]))
        assert np.array_equal(soft.cpu().numpy(), LM.soft(paths, pm, count, rem, 0, 1, 16.0))
    finally:
        dec.close()
