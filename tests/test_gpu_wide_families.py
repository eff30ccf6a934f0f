"""GPU: k_scl_wide (csrc/scl_wide.h) at L = 128 and 256, where a list spans 2 and 4 wavefronts, on tied and degenerate rows,
frozen sets outside the 5G order and dense constraint sets, against dscl_model (tests/test_dyn_host.py) in f64 and in f32.

Every comparison is == on every frame: u_hat bit for bit, the metric, the flags word; no `keep` mask, no tolerance.  The
pm / flags buffers start from values no decode writes, and every wide context asserts kernel_name.startswith("k_scl_wide<")
(behind "k_rm_recover, then " on the rate-matched contexts of group 8, which name their recovery kernel first).
tests/test_wide_families_host.py holds the conditions on the CPU: on these rows the model ties, leaves dead slots
un-refilled, refills across 64-slot groups and meets leaves whose 2L candidates are all equal -- none of which happens on
the Gaussian rows of tests/test_gpu_wide.py.  The cases are those of tests/wide_families.py:

   1  N = 32, L = 128 / 256, f64 / f32: state in registers only, 2 / 4 wavefronts; dense_all, leaf0, bern_0.5, sparse_5_half,
      and all_prev / prev_only constraints on bern_0.5; the eight LLR families
   2  N = 64, L = 128 on the 27 frozen patterns, default variant and forced to global scratch (GA, through the testing
      library's spill selection): both equal the model, hence each other; L = 256 (f32 and f64, both LDS) on three masks
   3  N = 128, L = 256 on the 30 frozen patterns, mask m on configuration m % 2 of (f32: levels in LDS, f64: GA by size)
   4  CA-SCL, N = 128, CRC-6 at permuted positions: L = 128 f32 on the 25 masks that can carry it, L = 256 f64 (GA by size)
      on three; FLAG_CRC_PASS is set on some frames and clear on others at each L
   5  constraint families at (64, 128) f64 / f32 and (128, 256) f32 LDS / f64 GA by size; PCCASCL(64, 24, n_pc = 3, n_pc_wm = 1,
      L = 128) and a bern_half CA-SCL case at (128, 256)
   6  ties at the pointer-table extremes (1024, 64) f64, (512, 128) f32, (256, 256) f64, all GA by size
   7  lists that never fill (K <= 5): L = 128 / 256 against L = 32 (not k_scl_wide) device against device, and both against the model
   8  rate matching: shortened, punctured (exact zeros) and repeated rows into CA-SCL L = 128, with and without the channel
      interleaver, and plain SCL at L = 256 punctured
   9  the frozen-mask override of decode_batch on a wide SCL context
  10  the work queue at four wavefronts, default and GA: 8192 rows in one launch against launches of 64

Dropped against the plan, for the model's CPU time: group 1 runs 18 frames per batch, not 66 (every batch still holds each
degenerate row; the kernel decodes one frame per workgroup, so a batch above 64 frames reaches nothing more).  No mask and
no mechanism is dropped.

Also dropped: group 7 runs 32 Gaussian and 32 mixed rows per mask, not 64 and 64 (the model at L = 256 steps all 256 slots
through every leaf of a list that holds at most 32 paths).

A record, not a gate: the model takes about 88 s of CPU time for the whole file on the machine it was written on (group 5: 26 s,
group 3: 15 s, group 1: 13 s, group 7: 12 s, group 2: 11 s, groups 4 and 8: 8 s each).  On one MI355X this file, tests/test_gpu_wide.py
and tests/test_gpu_dyn_families.py together (87 tests) took 57 s of wall time, the model on that host's CPU included; the first
34 tests of this file (groups 1 to 7) took 27.6 s of it, and no test of this file more than 2.5 s.  The file was not timed
alone."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frozen_patterns as P  # noqa: E402
import llr_families as F  # noqa: E402
import test_dyn_host as M  # noqa: E402
import test_rm_host as RM  # noqa: E402
import wide_families as W  # noqa: E402
from test_gpu_dyn_families import _cuda, _decode, _same, _unpack  # noqa: E402

GROUPS = {g: [c for c in W.cases() if c.group == g] for g in W.GROUPS}
CRC6 = W.CRC6


def _pa_dtype(dtype):
    import polardecoding_amd as pa
    return pa.F32 if dtype == "f32" else pa.F64


def _decoder(c, made, spill=False):
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    K = made.order.size - (max(made.taps) if made.taps else 0)
    dec = pa.Decoder(c.N, K, pa.ALGO_CASCL if made.taps else pa.ALGO_SCL, L=c.L, crc_taps=made.taps, dtype=_pa_dtype(c.dtype),
                     info_order=made.order, dyn=made.dyn)
    if spill:
        T.select_kernel(dec, T.KERNEL_GENERIC_SPILL)
    assert dec.kernel_name.startswith("k_scl_wide<") == (c.L > 32) and dec.L == c.L, (W.tag(c), dec.kernel_name)
    assert np.array_equal(dec.info_order, made.order), W.tag(c)
    if made.dyn is not None:
        assert np.array_equal(dec.dyn_positions, made.dyn[0]) and "dynamic" in dec.kernel_name
    return dec


def _run(c, spill=False, note=""):
    """case c on every one of its input batches; returns what the device gave, name -> (u_hat, pm, flags)"""
    made, (ref, _) = W.materialise(c), W.reference(c)
    dec = _decoder(c, made, spill)
    got = {}
    for name, rows in made.batches.items():
        got[name] = _decode(dec, rows)
        _same(got[name], ref[name], f"{W.tag(c)} {name}{' forced GA' if spill else ''}{note} {dec.kernel_name}")
    dec.close()
    return got


# ---- 1: registers only, several wavefronts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("L,dtype", W.W1_CONFIGS, ids=lambda v: str(v))
def test_n32_register_state_across_wavefronts(L, dtype):
    cs = [c for c in GROUPS["w1"] if (c.L, c.dtype) == (L, dtype)]
    assert [(c.mask, c.fam) for c in cs] == [(m, W.NONE) for m in W.W1_MASKS] + [("bern_0.5", f) for f in W.W1_CONSTRAINTS]
    assert sum(len(_run(c)) for c in cs) == 6 * 8


# ---- 2: the first LDS words, two wavefronts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_n64_l128_every_frozen_pattern_default_and_forced_ga(dtype):
    """the same cases on both variants; each equals the model on every frame, hence the two are identical"""
    cs = [c for c in GROUPS["w2"] if (c.L, c.dtype) == (128, dtype)]
    assert [c.mask for c in cs] == list(P.families(64)) and len(cs) == 27
    for c in cs:
        _run(c)
        _run(c, spill=True)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_n64_l256_levels_in_lds(dtype):
    cs = [c for c in GROUPS["w2"] if (c.L, c.dtype) == (256, dtype)]
    assert [c.mask for c in cs] == list(W.W2_L256_MASKS)
    for c in cs:
        _run(c, note=" LDS")


# ---- 3: four wavefronts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1], ids=["f32-lds", "f64-ga-by-size"])
def test_n128_l256_every_frozen_pattern(k):
    L, dtype = W.W3_CONFIGS[k]
    cs = [c for c in GROUPS["w3"] if (c.L, c.dtype) == (L, dtype)]
    assert [c.mask for c in cs] == list(P.families(128))[k::2] and len(cs) == 15
    for c in cs:
        _run(c, note=" GA by size" if dtype == "f64" else " LDS")


# ---- 4: CA-SCL across wavefronts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,dtype", [(128, "f32"), (256, "f64")], ids=["L128-f32", "L256-f64-ga-by-size"])
def test_cascl_crc_mask_across_wavefronts(L, dtype):
    cs = [c for c in GROUPS["w4"] if (c.L, c.dtype) == (L, dtype)]
    want = list(P.with_crc(P.families(128), 128)) if L == 128 else list(W.W4_L256_MASKS)
    assert [c.mask for c in cs] == want
    passed = np.concatenate([(_run(c)["cycle"][2] & M.FLAG_CRC_PASS) != 0 for c in cs])
    assert passed.any() and not passed.all()          # the pass mask decided some frames; in others no slot passed


# ---- 5: constraints at wide L -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", W.W5_MASKS)
@pytest.mark.parametrize("N,L,dtype,B", W.W5_CONFIGS, ids=lambda v: str(v))
def test_constraint_families(N, L, dtype, B, mask):
    cs = [c for c in GROUPS["w5"] if (c.N, c.L, c.dtype, c.B, c.algo, c.mask) == (N, L, dtype, B, "SCL", mask)]
    assert [c.fam for c in cs] == list(W.W5_FAMS)
    for c in cs:
        _run(c, note=" GA by size" if (N, dtype) == (128, "f64") else " LDS")


def test_cascl_with_constraints():
    """5G parity-check bits under CA-SCL at (64, 128), and a bern_half set under CA-SCL at (128, 256)"""
    import polardecoding_amd as pa
    (c,) = [c for c in GROUPS["w5"] if c.algo == "CASCL"]
    fl = _run(c)["cycle"][2]
    N, K, L, B = 64, 24, 128, 16
    pos, sets, io = pa.dyn_pc5g(N, pa.q_sequence(N)[N - (K + 6 + 3):], 3, 1)
    mask = np.ones(N, dtype=np.uint8)
    mask[io] = 0
    u, llr = M.make_frames(N, io, (pos, sets), B, 64128, dbs=W.DBS2, crc=CRC6)
    rows = W.input_batch(llr, "cycle", 64128, np.float64)
    want = W.model_on(mask, (pos, sets), rows, L, "f64", crc=(io, CRC6))
    assert (want[2] & M.FLAG_TIE).any()
    dec = pa.PCCASCL(N, K, n_pc=3, n_pc_wm=1, L=L)
    assert dec.kernel_name.startswith("k_scl_wide<double,L=128>") and "dynamic" in dec.kernel_name
    assert np.array_equal(dec.dyn_positions, pos) and np.array_equal(dec.info_order, io)
    got = _decode(dec, rows)
    dec.close()
    _same(got, want, f"PCCASCL(64, 24) L=128 {dec.kernel_name}")
    assert ((np.concatenate([fl, got[2]]) & M.FLAG_CRC_PASS) != 0).any()


# ---- 6: ties at the pointer-table extremes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,dtype", W.W6_SHAPES, ids=lambda v: str(v))
def test_ties_at_the_pointer_table_extremes(N, L, dtype):
    (c,) = [c for c in GROUPS["w6"] if (c.N, c.L, c.dtype) == (N, L, dtype)]
    ref, tr = W.reference(c)
    (name,) = ref
    assert (ref[name][2] & M.FLAG_TIE).all()
    assert L == 64 or tr[name]["cross"].all()          # above one wavefront every frame refills across wavefronts
    _run(c, note=" GA by size")


# ---- 7: lists that never fill ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 128])
def test_lists_that_never_fill_equal_l32(N):
    """2^K <= 32 live paths on either side and no ranking: the wide kernel and the L = 32 kernel give the same bits and metric"""
    for mask in W.W7_MASKS[N]:
        cs = {c.L: c for c in GROUPS["w7"] if (c.N, c.mask) == (N, mask)}
        assert sorted(cs) == [32, 128, 256]
        made = W.materialise(cs[32])
        assert int((made.mask == 0).sum()) <= 5
        for L in (128, 256):
            assert all(np.array_equal(a, b) for a, b in zip(W.materialise(cs[L]).batches.values(), made.batches.values()))
        got = {L: _run(c) for L, c in cs.items()}        # each against the model; L = 32 is not k_scl_wide (_decoder)
        for name in made.batches:
            for L in (128, 256):
                _same(got[L][name], got[32][name], f"{N} {mask} {name}: L = {L} against L = 32 on the device")
            assert not got[32][name][2].any()


# ---- 8: rate matching ---------------------------------------------------------------------------------------------------------
RM_PREFIX = "k_rm_recover, then "
RM_CASES = {"shortened": (60, 100, RM.SHORTEN), "punctured": (36, 100, RM.PUNCTURE), "repeated": (40, 160, RM.REPEAT)}


@functools.lru_cache(maxsize=None)
def _rm_rows(A, E, ibil, crc, B=32):
    """(info_order, frozen mask, received rows [2 B][E] float64: B Gaussian rows, then the same on grid(1, 7))"""
    N = 128
    io = RM.info_order(N, A, E)
    mask = np.ones(N, dtype=np.uint8)
    mask[io] = 0
    u, _ = M.make_frames(N, io, None, B, 800 + A + E, crc=CRC6 if crc else None)
    sent = RM.transmit(RM.encode(u), E, A, ibil)
    rng = np.random.default_rng([A, E, int(ibil)])
    sig = 10.0 ** (-np.array([1.0, 3.0])[np.arange(B) % 2] / 20.0)[:, None]
    rx = 2.0 * ((1.0 - 2.0 * sent) + sig * rng.standard_normal((B, E))) / sig / sig
    rows = np.concatenate([rx, F.grid(rx, 1.0, 7)])
    rows.setflags(write=False)
    return io, mask, rows


def _rm_case(A, E, mode, ibil, dtype, L, crc):
    import polardecoding_amd as pa
    N = 128
    assert RM.mode_of(N, A, E) == mode
    io, mask, rows = _rm_rows(A, E, ibil, crc)
    rows = rows.astype(np.float32 if dtype == "f32" else np.float64)
    want = W.model_on(mask, None, RM.recover(rows, N, A, ibil), L, dtype, crc=(io, CRC6) if crc else None)
    dec = pa.Decoder(N, A - (6 if crc else 0), pa.ALGO_CASCL if crc else pa.ALGO_SCL, L=L, crc_taps=CRC6 if crc else None,
                     dtype=_pa_dtype(dtype), E=E, ibil=ibil)
    # a rate-matched context names its recovery kernel first: "k_rm_recover, then k_scl_wide<...>"
    assert dec.kernel_name.startswith(RM_PREFIX + "k_scl_wide<") and (dec.E, dec.rm_mode, dec.ibil) == (E, mode, ibil)
    assert np.array_equal(dec.info_order, io)
    got = _decode(dec, rows)
    dec.close()
    _same(got, want, f"rate matching A={A} E={E} ibil={ibil} {dtype} L={L} {dec.kernel_name}")
    return want


@pytest.mark.parametrize("ibil", [False, True], ids=["plain", "ibil"])
@pytest.mark.parametrize("case", list(RM_CASES))
def test_rate_matched_cascl_l128(case, ibil):
    A, E, mode = RM_CASES[case]
    want = _rm_case(A, E, mode, ibil, "f64", 128, True)
    if mode != RM.REPEAT:
        assert (want[2][32:] & M.FLAG_TIE).any()       # the grid rows with planted zeros / 2^20 tie
    if mode == RM.SHORTEN:
        _rm_case(A, E, mode, ibil, "f32", 128, True)


def test_rate_matched_scl_l256_punctured():
    A, E, mode = RM_CASES["punctured"]
    _rm_case(A, E, mode, False, "f64", 256, False)


# ---- 9: the frozen-mask override -----------------------------------------------------------------------------------------
def test_frozen_mask_override_on_a_wide_context():
    import polardecoding_amd as pa
    dec = pa.SCLdecode(64, 32, L=128)                   # the 5G set; every decode below overrides it
    assert dec.kernel_name.startswith("k_scl_wide<double,L=128>")
    for mask in ("islands_32_a", "leaf0", "bern_0.5"):
        (c,) = [c for c in GROUPS["w2"] if (c.mask, c.L, c.dtype) == (mask, 128, "f64")]
        made, (ref, _) = W.materialise(c), W.reference(c)
        own = _decoder(c, made)
        for name, rows in made.batches.items():
            got = dec.decode_batch(rows, frozen_mask=made.mask)
            got = (got[0], got[1], np.asarray(got[2]).view(np.uint32))
            mine = own.decode_batch(rows)
            _same(got, (mine[0], mine[1], np.asarray(mine[2]).view(np.uint32)), f"override {mask}: against the context made with it")
            _same(got, ref[name], f"override {mask}: against the model")
        own.close()
    dec.close()


# ---- 10: the work queue, four wavefronts, both variants ------------------------------------------------------------------
@pytest.mark.parametrize("spill", [False, True], ids=["default", "forced-ga"])
def test_work_queue_four_wavefronts(spill):
    """8192 rows in one launch (more than the 8 x 256 workgroups the GA variant may keep resident, so every scratch slice is
    reused from frame to frame) against the same rows in launches of 64, three times over; the first 64 against the model"""
    import torch
    (c,) = GROUPS["w10"]
    made, (ref, _) = W.materialise(c), W.reference(c)
    B, N = 8192, c.N
    rng = np.random.default_rng(10)
    llr = np.concatenate([made.batches["mixed"], 2.0 * rng.standard_normal((B - c.B, N)) + 1.0])
    dec = _decoder(c, made, spill)
    d_in = _cuda(llr)

    def run(chunk):
        bits = torch.full((B, N // 32), -1, dtype=torch.int32, device="cuda")
        pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
        fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for o in range(0, B, chunk):
            dec.decode_device(d_in[o:o + chunk], out_bits=bits[o:o + chunk], pm=pm[o:o + chunk], flags=fl[o:o + chunk])
        dec.synchronize()
        return _unpack(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)

    small = run(64)
    for rep in range(3):
        _same(run(B), small, f"one launch of {B}, repeat {rep}, against launches of 64")
    dec.close()
    assert (small[0][:, 3] == 0).all() and (small[1] >= 0).all() and (small[2] <= 1).all()   # every output was written
    _same(tuple(a[:c.B] for a in small), ref["mixed"], "the first 64 rows against the model")


def test_all_cases_are_run():
    """every case of wide_families.cases() belongs to a group a test above runs whole"""
    assert sum(len(v) for v in GROUPS.values()) == len(W.cases())
    assert all(GROUPS[g] for g in W.GROUPS)
