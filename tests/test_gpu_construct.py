"""GPU: Monte-Carlo code construction (include/polar_hip.h rules 1-4) against the numpy model of tests/test_construct_host.py.

The gate is exactness: k_genie_lanes' counters equal the model's, counter for counter, in f64 and in f32, for LLR and y rows,
at every block length.  Then: counters add (calls, non-zero buffers, queued launches, graph replays), polar_construct_batch is
its two halves, the design rows depend only on (seed, frame) and have the moments of rule 3, refusals leave the ctx usable,
and a constructed frozen set decodes no worse than the polarization-weight order it replaces."""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import test_construct_host as M  # noqa: E402


def _torch_dtype(dtype):
    import torch
    return torch.float32 if dtype == np.float32 else torch.float64


def _ctx(N, dtype=np.float64):
    import polardecoding_amd as pa
    dec = pa.SCdecode(N, N // 2, dtype=pa.F32 if dtype == np.float32 else pa.F64)
    dec.use_torch_stream()
    return dec


def _zeros(N):
    import torch
    return torch.zeros((2, N), dtype=torch.int64, device="cuda")


def _host(counts):
    return counts.cpu().numpy().view(np.uint64)


def _count(dec, rows, sigma=0.0, counts=None):
    import torch
    counts = _zeros(dec.N) if counts is None else counts
    dec.genie_count_device(torch.from_numpy(np.ascontiguousarray(rows)).cuda(), counts, sigma=sigma)
    dec.synchronize()
    return _host(counts)


@pytest.mark.parametrize("dtype", M.EXACT_DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", M.EXACT_CASES, ids=lambda c: "N%d-s%g-B%d" % c[:3])
def test_counters_equal_the_model_exactly(case, dtype, oracle):
    N, sigma, B, seed = case
    llr = M.design_rows(N, B, sigma, seed).astype(dtype)    # ctx dtype == row dtype
    err, tie, _, _ = M.genie_model(oracle, llr, dtype)
    dec = _ctx(N, dtype)
    got = _count(dec, llr)
    print(f"N={N} B={B} {np.dtype(dtype).name}: model err sum {int(err.sum())} tie sum {int(tie.sum())}; "
          f"differing counters {int((got[0] != err).sum())} + {int((got[1] != tie).sum())}")
    assert np.array_equal(got[0], err) and np.array_equal(got[1], tie)
    # the same frames given as observations y with sigma > 0: llr = 2*y/sigma/sigma in double, then rounded to the ctx dtype
    y = (1 + sigma * np.random.default_rng(seed).standard_normal((B, N))).astype(dtype)
    llr_y = oracle.llr_from_y(y.astype(np.float64), sigma).reshape(B, N).astype(dtype)
    err, tie, _, _ = M.genie_model(oracle, llr_y, dtype)
    got = _count(dec, y, sigma=sigma)
    assert np.array_equal(got[0], err) and np.array_equal(got[1], tie)


@pytest.mark.parametrize("dtype", M.EXACT_DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("N", [32, 128, 1024, 4096])
def test_zero_rows_tie_and_huge_rows_stay_finite(N, dtype, oracle):
    dec = _ctx(N, dtype)
    B = 64 + 37
    got = _count(dec, np.zeros((B, N), dtype=dtype))
    assert (got[1] == B).all() and not got[0].any()
    got = _count(dec, -np.zeros((B, N), dtype=dtype))
    assert (got[1] == B).all() and not got[0].any()
    mixed = np.full((B, N), 1e30, dtype=dtype)
    mixed[1::2] = M.design_rows(N, B, 0.8, 90 + N).astype(dtype)[1::2]
    mixed[0] = 0
    err, tie, lam, _ = M.genie_model(oracle, mixed, dtype)
    assert np.isfinite(lam).all() and tie.min() >= 1
    got = _count(dec, mixed)
    assert np.array_equal(got[0], err) and np.array_equal(got[1], tie)


def test_counters_accumulate_over_calls_and_buffers(oracle):
    import torch
    N, B = 512, 64 * 6 + 11
    llr = M.design_rows(N, B, 0.8, 77)
    err, tie, _, _ = M.genie_model(oracle, llr)
    dec = _ctx(N)
    whole = _count(dec, llr)
    assert np.array_equal(whole[0], err) and np.array_equal(whole[1], tie)
    c = _zeros(N)
    _count(dec, llr[:200], counts=c)
    halves = _count(dec, llr[200:], counts=c)
    assert np.array_equal(halves, whole)
    start = np.random.default_rng(3).integers(0, 2 ** 62, size=(2, N)).astype(np.uint64)
    c = torch.from_numpy(start.view(np.int64).copy()).cuda()
    assert np.array_equal(_count(dec, llr, counts=c), start + whole)    # adds to a non-zero buffer, 64-bit sums


@pytest.mark.parametrize("N,dtype", [(1024, np.float64), (2048, np.float32)])
def test_one_big_queued_launch_equals_small_launches(N, dtype):
    """More batches of 64 than resident wavefronts: the jobs beyond the first round come from the work queue.  Integer sums
    cannot depend on who takes which batch."""
    import torch
    dec = _ctx(N, dtype)
    B, chunk = (1 << 19) + 777, 16384
    rows = torch.empty((B, N), dtype=torch.float32, device="cuda")
    dec.genie_rows_device(9, 0, 0.8, rows)
    big = _zeros(N)
    for _ in range(2):   # twice on the same context: the queue counter is back at zero after a launch
        dec.genie_count_device(rows, big)
    small = _zeros(N)
    for off in range(0, B, chunk):
        dec.genie_count_device(rows[off:off + chunk], small)
    dec.synchronize()
    big, small = _host(big), _host(small)
    assert small[0].sum() > 0 and np.array_equal(big, 2 * small)


def test_captured_call_replays_and_adds_again():
    import torch
    N, B = 1024, (1 << 18) + 5     # with the work queue
    dec = _ctx(N)
    rows = torch.empty((B, N), dtype=torch.float32, device="cuda")
    dec.genie_rows_device(4, 0, 0.8, rows)
    once = _zeros(N)
    dec.genie_count_device(rows, once)    # warm-up at the same B: scratch and queue exist
    dec.construct_batch(4, 0, 0.8, 4096, _zeros(N))
    dec.synchronize()
    once = _host(once)
    c = _zeros(N)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dec.use_torch_stream()
        with torch.cuda.graph(g, stream=s):
            dec.genie_count_device(rows, c)
    torch.cuda.synchronize()
    c.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    dec.use_torch_stream()
    assert once[0].sum() > 0 and np.array_equal(_host(c), 3 * once)
    del g


@pytest.mark.parametrize("N,dtype,B", [(4096, np.float64, 8192 + 1000), (128, np.float32, 70001), (32, np.float64, 1000)])
def test_construct_batch_is_rows_then_count(N, dtype, B):
    """B spans more than one 256 MiB chunk at N = 4096 f64 (8192 rows per chunk)."""
    import torch
    dec = _ctx(N, dtype)
    seed, first, sigma = 1234, 5_000_000_000, 0.9
    a = _zeros(N)
    dec.construct_batch(seed, first, sigma, B, a)
    rows = torch.empty((B, N), dtype=_torch_dtype(dtype), device="cuda")
    dec.genie_rows_device(seed, first, sigma, rows)
    b = _zeros(N)
    dec.genie_count_device(rows, b)
    # rows depend only on (seed, frame index): the range cut differently gives the same counters
    c = _zeros(N)
    cuts = [0, 1, 64, B // 3, B - 7, B]
    for lo, hi in zip(cuts, cuts[1:]):
        dec.construct_batch(seed, first + lo, sigma, hi - lo, c)
    dec.synchronize()
    a, b, c = _host(a), _host(b), _host(c)
    assert a[0].sum() > 0
    assert np.array_equal(a, b) and np.array_equal(a, c)
    part = torch.empty((7, N), dtype=_torch_dtype(dtype), device="cuda")
    dec.genie_rows_device(seed, first + B - 7, sigma, part)
    assert torch.equal(part, rows[B - 7:])
    other = _zeros(N)
    dec.construct_batch(seed + 1, first, sigma, B, other)
    dec.synchronize()
    assert not np.array_equal(_host(other), a)


@pytest.mark.parametrize("dtype", M.EXACT_DTYPES, ids=["f64", "f32"])
def test_design_row_statistics(dtype):
    """Rule 3: LLR = 2*(1 + sigma z)/sigma^2 has mean 2/sigma^2 and variance 4/sigma^2.  Over n = 2^16 * N samples the mean is
    within 4 standard errors sqrt(var/n), the variance within 4 standard errors var*sqrt(2/(n-1)) (normal samples)."""
    import torch
    N, B, sigma = 128, 1 << 16, 0.8
    dec = _ctx(N, dtype)
    rows = torch.empty((B, N), dtype=_torch_dtype(dtype), device="cuda")
    dec.genie_rows_device(31, 0, sigma, rows)
    dec.synchronize()
    x = rows.cpu().numpy().astype(np.float64)
    n = x.size
    mean, var = 2 / sigma ** 2, 4 / sigma ** 2
    print(f"mean {x.mean():.6f} (want {mean:.6f}, se {math.sqrt(var / n):.2e}); var {x.var():.6f} (want {var:.6f}, se {var * math.sqrt(2 / (n - 1)):.2e})")
    assert abs(x.mean() - mean) <= 4 * math.sqrt(var / n)
    assert abs(x.var() - var) <= 4 * var * math.sqrt(2 / (n - 1))
    # element e takes normal (e & 1) of its pair's Philox block: the two normals of a pair are uncorrelated
    z = (x * sigma ** 2 / 2 - 1) / sigma
    assert abs((z[:, 0::2] * z[:, 1::2]).mean()) <= 4 / math.sqrt(n / 2)


def test_refusals_leave_the_ctx_usable(oracle):
    import torch
    import polardecoding_amd as pa
    N = 128
    dec = _ctx(N)
    rows = torch.empty((64, N), dtype=torch.float64, device="cuda")
    c = _zeros(N)
    lib, h = dec._lib, dec._h
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.polar_genie_rows_device(h, 1, 0, sigma, 64, rows.data_ptr(), 0) == -1
        assert lib.polar_construct_batch(h, 1, 0, sigma, 64, c.data_ptr()) == -1
    assert lib.polar_genie_rows_device(h, 1, 0, 0.8, 64, None, 0) == -1
    assert lib.polar_construct_batch(h, 1, 0, 0.8, 64, None) == -1
    assert lib.polar_genie_count_device(h, None, 0, 0.0, 64, c.data_ptr()) == -1
    assert lib.polar_genie_count_device(h, rows.data_ptr(), 0, 0.0, 64, None) == -1
    assert lib.polar_genie_count_device(h, rows.data_ptr(), 0, 0.0, 1 << 31, c.data_ptr()) == -1
    assert lib.polar_construct_batch(h, 1, 0, 0.8, 1 << 31, c.data_ptr()) == -1
    assert lib.polar_genie_rows_device(h, 1, 0, 0.8, 1 << 31, rows.data_ptr(), 0) == -1
    assert lib.polar_genie_count_device(None, rows.data_ptr(), 0, 0.0, 64, c.data_ptr()) == -1
    rm = pa.Decoder(N, 40, pa.ALGO_SC, E=100)
    with pytest.raises(pa.PolarError):
        rm.genie_count_device(rows, c)
    with pytest.raises(pa.PolarError):
        rm.genie_rows_device(1, 0, 0.8, rows)
    with pytest.raises(pa.PolarError):
        rm.construct_batch(1, 0, 0.8, 64, c)
    dec.synchronize()
    assert not _host(c).any()
    llr = M.design_rows(N, 100, 0.8, 8)
    err, tie, _, _ = M.genie_model(oracle, llr)
    got = _count(dec, llr)
    assert np.array_equal(got[0], err) and np.array_equal(got[1], tie)
    assert lib.polar_genie_count_device(h, rows.data_ptr(), 0, 0.0, 0, c.data_ptr()) == 0   # B = 0: nothing to do


def _fer(dec, seed, snr_db, frames, batch=1 << 16):
    blk = 0
    for first in range(0, frames, batch):
        blk += dec.fer_batch(seed, first, snr_db, min(batch, frames - first))[0]
    return blk


MC_FRAMES = 1 << 23    # construction frames of the end-to-end test (N = 2048 f64)
FER_FRAMES = 1 << 20


def test_constructed_set_decodes_no_worse_than_the_polarization_weight_order():
    """N = 2048, K = 1024, SC, design and evaluation at 2.0 dB (sigma = 10^(-2/20)).  Condition: FER(constructed) <=
    FER(polarization weight) + 3 binomial standard errors of the latter, over the same 2^20 generated frame indices."""
    import polardecoding_amd as pa
    N, K, db = 2048, 1024, 2.0
    sigma = 10 ** (-db / 20)
    pa.construct_mc(N, sigma, 1 << 16, seed=2)   # warm-up: code objects, scratch
    t0 = time.time()
    order, counts = pa.construct_mc(N, sigma, MC_FRAMES, seed=1)
    sec = time.time() - t0
    assert sorted(order.tolist()) == list(range(N))
    base = pa.SCdecode(N, K)
    mc = pa.SCdecode(N, K, info_order=order[N - K:])
    assert mc.info_order.tolist() == order[N - K:].tolist()
    overlap = len(set(order[N - K:].tolist()) & set(base.info_order.tolist()))
    e_base = _fer(base, 77, db, FER_FRAMES)
    e_mc = _fer(mc, 77, db, FER_FRAMES)
    p = e_base / FER_FRAMES
    se = math.sqrt(p * (1 - p) / FER_FRAMES)
    print("CONSTRUCT_RESULT " + json.dumps({
        "N": N, "K": K, "algo": "SC", "design_db": db, "eval_db": db, "mc_frames": MC_FRAMES, "mc_seconds": round(sec, 3),
        "fer_frames": FER_FRAMES, "fer_constructed": e_mc / FER_FRAMES, "fer_base": p, "base": "polarization weight",
        "block_errors_constructed": e_mc, "block_errors_base": e_base, "info_set_overlap": overlap}))
    assert e_base > 0
    assert e_mc / FER_FRAMES <= p + 3 * se


def test_polar_sim_construct_then_q_file(tmp_path):
    sim = os.path.join(REPO, "polardecoding_amd", "lib", "polar_sim")
    q = str(tmp_path / "q2048.txt")
    base = [sim, "--algo", "sc", "--N", "2048", "--K", "1024", "--fast", "--snr", "2.0:2.5:0.5", "--ble", "50", "--batch", "16384"]
    a = subprocess.run(base + ["--construct", "1000000", "--design-snr", "2.0", "--q-out", q], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0, a.stderr
    vals = [int(x) for x in open(q).read().split()]
    assert sorted(vals) == list(range(2048))
    b = subprocess.run(base + ["--q", q], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    la = [ln for ln in a.stdout.splitlines() if "bSNR = " in ln]
    lb = [ln for ln in b.stdout.splitlines() if "bSNR = " in ln]
    assert len(la) == 2 and la == lb, (a.stdout, b.stdout)
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert [ln for ln in plain.stdout.splitlines() if "bSNR = " in ln] != la    # the constructed order is in use
    r = subprocess.run(base + ["--construct", "1000"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--design-snr" in r.stderr
