"""GPU: k_scl_dyn and k_generate_dyn on the constraint families of tests/dyn_families.py, against dscl_model
(tests/test_dyn_host.py) in f64 and in f32.

Every comparison is == on every frame, median-tie frames included: u_hat bit for bit, the metric, the flags word.  There is
no `keep` mask and no tolerance; the kernel is deterministic and the model implements the slot-level survivor and refill rule.
tests/test_dyn_families_host.py holds the conditions: the model equals the oracle on every mask used here, the cases tie
(a third of the frames and more on the grids at L >= 8), err and set dynamic bits.  Each test asserts "k_scl_dyn<" in the
kernel name of every context it makes.

  N = 32    the history is the register h0 alone: L = 1 (SC), 2, 32, nine constraint families x eight input batches (three
            grids, hard, each again with mixed zero signs and degenerate rows planted), B = 65 and 300
  N = 64    the first LDS history word, copied on fork and refill: L = 2 and 8, f64 and f32, nine families, each case on the
            default variant and on the global-scratch variant (GA = true, through the testing library's spill selection):
            both equal the model, and so each other
  N = 128   the 30 masks of tests/frozen_patterns.py x bern_half / alternate / dyn_chain: SC, SCL L = 8 and 32, CA-SCL with
            CRC-6 at permuted positions, 16 frames per case at 1 and 3 dB on the grids and `hard` in turn
  N = 1024  all_prev / word0_only / own_word_only / word_edges on the PAC rm mask, an islands and a leaf0 mask: L = 32 f64
            (GA by size), L = 32 f32 (LDS; S = 2, sixteen strided words per lane), L = 8, L = 1 in SC mode (S = 64 > N / 32)
  k_generate_dyn with D = N / 2 dense rows; y + sigma input and f32 input on an f64 context on a grid.

205 cases from dyn_families.cases(), the 36 of N = 64 on both variants, plus one input-form and four generator cases.  The
model takes about 28 s of CPU time for all of them (17 s of it at N = 1024); the wall time on an MI355X has not been measured:
no device was available when this file was written, and nothing in it has run on one yet."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dyn_families as D  # noqa: E402
import test_dyn_host as M  # noqa: E402

GROUPS = {g: [c for c in D.cases() if c.group == g] for g in ("n32", "n64", "n128", "n128crc", "n1024")}


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _decoder(c, made, spill=False):
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    algo = {"SC": pa.ALGO_SC, "SCL": pa.ALGO_SCL, "CASCL": pa.ALGO_CASCL}[c.algo]
    K = made.order.size - (max(made.taps) if made.taps else 0)
    dec = pa.Decoder(c.N, K, algo, L=c.L, crc_taps=made.taps, dtype=pa.F32 if c.dtype == "f32" else pa.F64,
                     info_order=made.order, dyn=made.dyn)
    if spill:
        T.select_kernel(dec, T.KERNEL_GENERIC_SPILL)
    assert "k_scl_dyn<" in dec.kernel_name, (D.tag(c), dec.kernel_name)
    assert np.array_equal(dec.dyn_positions, made.dyn[0]) and np.array_equal(dec.info_order, made.order), D.tag(c)
    return dec


def _decode(dec, rows, sigma=0.0):
    """polar_decode_device -> (u_hat, pm float64, flags uint32); the buffers start from values no decode writes"""
    import torch
    d = _cuda(rows)
    B = d.shape[0]
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_device(d, sigma=sigma, pm=pm, flags=fl)
    dec.synchronize()
    return _unpack(bits.cpu().numpy(), dec.N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


def _same(got, want, label):
    """bits, metric and flags by == on every frame; the message names the first differing frame and leaf"""
    (g_u, g_pm, g_fl), (w_u, w_pm, w_fl) = got, want
    bad = np.flatnonzero((g_u != w_u).any(axis=1))
    if bad.size:
        f = int(bad[0])
        j = int(np.flatnonzero(g_u[f] != w_u[f])[0])
        tie = bool(w_fl[f] & M.FLAG_TIE)
        assert False, (label, f"u_hat differs in {bad.size} frames, first frame {f} at leaf {j} (word {j >> 5}); the model "
                       f"flags a tie there: {tie}; pm {g_pm[f]!r} against {w_pm[f]!r}")
    bad = np.flatnonzero(g_pm != w_pm)
    assert bad.size == 0, (label, f"pm differs in {bad.size} frames, first {int(bad[0])}: {g_pm[bad[0]]!r} against {w_pm[bad[0]]!r}")
    bad = np.flatnonzero(g_fl != w_fl)
    assert bad.size == 0, (label, f"flags differ in {bad.size} frames, first {int(bad[0])}: {g_fl[bad[0]]} against {w_fl[bad[0]]}")


def _run(c, spill=False):
    """case c on every one of its input batches; returns the number of batches compared"""
    made, ref = D.materialise(c), D.reference(c)
    dec = _decoder(c, made, spill)
    for name, rows in made.batches.items():
        _same(_decode(dec, rows), ref[name], f"{D.tag(c)} {name}{' GA' if spill else ''} {dec.kernel_name}")
    dec.close()
    return len(made.batches)


@pytest.mark.parametrize("L,dtype,B", D.N32_CONFIGS, ids=lambda v: str(v))
def test_n32_register_history(L, dtype, B):
    cs = [c for c in GROUPS["n32"] if (c.L, c.dtype, c.B) == (L, dtype, B)]
    assert [c.fam for c in cs] == list(D.FAMILIES)
    assert sum(_run(c) for c in cs) == 9 * 8


@pytest.mark.parametrize("L,dtype", D.N64_CONFIGS, ids=lambda v: str(v))
def test_n64_lds_history_default_and_global_scratch(L, dtype):
    """the same cases on both variants; each equals the model on every frame, hence the two are identical"""
    cs = [c for c in GROUPS["n64"] if (c.L, c.dtype) == (L, dtype)]
    assert [c.fam for c in cs] == list(D.FAMILIES)
    assert sum(_run(c) + _run(c, spill=True) for c in cs) == 9 * 3 * 2


@pytest.mark.parametrize("L,dtype", D.N128_SCL, ids=lambda v: str(v))
def test_n128_frozen_patterns(L, dtype):
    cs = [c for c in GROUPS["n128"] if (c.L, c.dtype) == (L, dtype)]
    assert len(cs) == 15 and len({c.mask for c in cs}) == 15 and {c.fam for c in cs} == set(D.N128_FAMS)
    assert sum(_run(c) for c in cs) == 15


@pytest.mark.parametrize("L,dtype", D.N128_CASCL, ids=lambda v: str(v))
def test_n128_frozen_patterns_cascl(L, dtype):
    cs = [c for c in GROUPS["n128crc"] if (c.L, c.dtype) == (L, dtype)]
    assert len(cs) in (6, 7) and all(c.algo == "CASCL" for c in cs)
    assert sum(_run(c) for c in cs) == len(cs)


@pytest.mark.parametrize("L,dtype", D.N1024_CONFIGS, ids=lambda v: str(v))
def test_n1024_dense_rows(L, dtype):
    cs = [c for c in GROUPS["n1024"] if (c.L, c.dtype) == (L, dtype)]
    assert {c.fam for c in cs if c.mask == "rm"} == set(D.N1024_FAMS) and {c.mask for c in cs} == set(D.N1024_MASKS)
    assert sum(_run(c) for c in cs) == len(cs) >= 6


def test_all_cases_are_run():
    assert sum(len(v) for v in GROUPS.values()) == len(D.cases()) == 205


# ---- other input forms ---------------------------------------------------------------------------------------------------
def test_y_sigma_and_f32_input_on_an_f64_context():
    """one grid batch each: y with sigma = 0.5 (llr = 8 y, formed in the kernel, exact), and float32 rows into an f64 context"""
    c = next(c for c in GROUPS["n64"] if (c.fam, c.L, c.dtype) == ("bern_half", 8, "f64"))
    made, ref = D.materialise(c), D.reference(c)
    rows, want = made.batches["grid2x3"], ref["grid2x3"]
    assert (want[2] & M.FLAG_TIE).sum() * 3 >= c.B
    dec = _decoder(c, made)
    _same(_decode(dec, rows / 8.0, sigma=0.5), want, "y + sigma")
    _same(_decode(dec, rows.astype(np.float32)), want, "f32 input on an f64 context")
    got = dec.decode_batch_y(rows / 8.0, 0.5)
    _same((got[0], got[1], np.asarray(got[2]).view(np.uint32)), want, "decode_batch_y")
    dec.close()


# ---- k_generate_dyn --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["all_prev", "bern_half"])
@pytest.mark.parametrize("N", [64, 1024])
def test_generator_fills_dense_rows(N, fam):
    """D = N / 2 dense rows (test_gpu_dyn.py::test_generator_and_fer_batch has PAC, three PC bits and a sparse set): every
    constraint holds by fill_dynamic, the information bits are the plain context's, fer_batch equals the hand count"""
    import torch
    import polardecoding_amd as pa
    mask, io = D.mask_of(N, "rm")
    dyn = D.constraint_families(N, mask, 5)[fam]
    assert dyn[0].size == N // 2
    L, B, seed, snr = 8, 300 if N == 64 else 65, 1234 + N, 1.5
    dec = pa.Decoder(N, N // 2, pa.ALGO_SCL, L=L, info_order=io, dyn=dyn)
    plain = pa.Decoder(N, N // 2, pa.ALGO_SCL, L=L, info_order=io)
    assert "k_scl_dyn<" in dec.kernel_name
    out = torch.empty((B, N), dtype=torch.float64, device="cuda")
    ub = torch.zeros((B, N // 32), dtype=torch.int32, device="cuda")
    out_p, ub_p = torch.empty_like(out), torch.zeros_like(ub)
    dec.generate_device(seed, 1000, snr, out, ub)
    plain.generate_device(seed, 1000, snr, out_p, ub_p)
    dec.synchronize()
    plain.synchronize()
    u, up = _unpack(ub.cpu().numpy(), N), _unpack(ub_p.cpu().numpy(), N)
    assert np.array_equal(u[:, io], up[:, io]) and u[:, io].any()
    assert u[:, dyn[0]].any()
    want = M.fill_dynamic(np.where(mask == 0, u, 0).astype(np.int64), dyn)
    bad = np.argwhere(u != want)
    assert bad.size == 0, f"{bad.shape[0]} bits differ from fill_dynamic, first (frame, leaf) {bad[0].tolist()}"
    x, xp = M.encode(u), M.encode(up)
    sig = 10.0 ** (-snr / 20.0)
    diff = out.cpu().numpy() - out_p.cpu().numpy()
    assert np.allclose(diff, (xp.astype(np.float64) - x) * 2.0 * 2.0 / sig / sig, rtol=1e-5, atol=1e-4)
    bits = dec.decode_device(out)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    dec.count_errors_device(bits, ub, cnt)
    dec.synchronize()
    hand = tuple(int(v) for v in cnt.cpu().numpy())
    assert dec.fer_batch(seed, 1000, snr, B) == hand
    uh = _unpack(bits.cpu().numpy(), N)
    assert hand == (int((uh[:, io] != u[:, io]).any(axis=1).sum()), int((uh[:, io] != u[:, io]).sum()))
    # the decode of the generated rows is the model's too
    w_u, _, _ = M.dscl_model(mask, dyn, out.cpu().numpy()[:16], L)
    assert np.array_equal(uh[:16], w_u)
    dec.close()
    plain.close()
