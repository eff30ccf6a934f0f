"""CPU: the model of the "List output" section (tests/list_model.py) held to what already stands.

  * the existing model: entry k* of rule 5 of list_model() equals tests/test_dyn_host.dscl_model's (u_hat, pm, flags), at
    N = 32 and 64, L = 4, 8 and 64, with and without CRC-6, plain and with random dynamic sets, on AWGN rows and on grid rows
    where metrics tie; the list itself obeys rule 3 (sorted, padded, count);
  * the reference: in f64 on tie-free frames the sorted metrics of the list equal the path metrics of the oracle's literal
    model of the reference's node records, sorted (N = 128, K = 64, CRC-6, L = 8: a shape of tests/test_oracle_ties.py);
  * rules 8, 10 and 11-13 restated on hand-made lists: the all-agree +-clamp case, the want_rem fallback, padding never
    selected, the x domain against test_dyn_host.encode;
  * include/polar_hip.h documents the section and declares the five entry points; the library exports them."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import list_model as LM  # noqa: E402
import llr_families as F  # noqa: E402
import test_dyn_host as M  # noqa: E402

CRC6 = M.CRC6
ENTRY_POINTS = ("polar_list_decode", "polar_list_decode_host", "polar_list_select", "polar_list_gather",
                "polar_list_soft")


def _rows(oracle, code, B, seed, kind):
    llr = F.oracle_llr(oracle, code, B, seed, 1.5)
    return F.grid(llr, 1.0, 7) if kind == "grid" else llr


# (N, K, crc, L, dynamic seed or None)
MODEL_CASES = [(32, 16, None, 4, None), (32, 16, None, 8, 3), (32, 10, CRC6, 4, None), (32, 16, None, 64, None),
               (64, 32, None, 8, None), (64, 26, CRC6, 8, 5), (64, 26, CRC6, 4, None), (64, 32, None, 64, 7), (64, 26, CRC6, 64, None)]


@pytest.mark.parametrize("kind", ["awgn", "grid"])
@pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: f"N{c[0]}-K{c[1]}-{'crc6' if c[2] else 'nocrc'}-L{c[3]}-dyn{c[4]}")
def test_entry_kstar_is_the_existing_model(case, kind, oracle):
    N, K, taps, L, dseed = case
    code = oracle.Code(N, K, taps)
    dyn = M.random_dyn(N, code.frozen, dseed) if dseed is not None else None
    crc = (code.info_order, taps) if taps else None
    B = 12 if L == 64 else 24
    llr = _rows(oracle, code, B, 100 + N + L, kind)
    for dtype in (np.float64, np.float32):
        x = llr.astype(dtype).astype(np.float64)
        w_u, w_pm, w_fl = M.dscl_model(code.frozen, dyn, x, L, crc=crc, dtype=dtype, sc=False, oracle=oracle)
        paths, pm, rem, count, flags = LM.list_model(code.frozen, dyn, x, L, crc=crc, dtype=dtype, oracle=oracle)
        ks = LM.kstar(rem, count, taps is not None)
        f = np.arange(B)
        assert np.array_equal(paths[f, ks], w_u) and np.array_equal(pm[f, ks], w_pm) and np.array_equal(flags, w_fl)
        # rule 3
        act = min(L, 1 << (N - int(code.frozen.sum())))
        assert (count == act).all()
        assert (np.diff(pm[:, :act], axis=1) >= 0).all() and np.isfinite(pm[:, :act]).all()
        assert np.isposinf(pm[:, act:]).all() and not paths[:, act:].any() and not rem[:, act:].any()
        if taps is None:
            assert not rem.any() and (ks == 0).all()
        if kind == "grid" and dtype is np.float64:
            assert (pm[:, :act - 1] == pm[:, 1:act]).any(), "the grid rows must tie two live metrics somewhere"


def test_sorted_metrics_are_the_references(oracle):
    code = oracle.Code(128, 64, oracle.CRC6_TAPS)
    sim, sig = oracle.Sim(5), oracle.sigma_from_db(1.5)
    lit = oracle.Literal(code, 8, crc=True)
    seen = 0
    for _ in range(16):
        _, y = sim.frame(code, sig)
        llr = oracle.llr_from_y(y, sig)
        uh, pm_ref, d = lit.decode(llr)
        if d != [0, 0, 0]:
            continue
        ref = np.sort(lit.path_metrics())
        paths, pm, rem, count, flags = LM.list_model(code.frozen, None, llr[None, :], 8, crc=(code.info_order, oracle.CRC6_TAPS),
                                                     oracle=oracle)
        assert count[0] == 8 and not (flags[0] & M.FLAG_TIE)
        assert np.array_equal(pm[0], ref)
        k = LM.kstar(rem, count, True)[0]
        assert np.array_equal(paths[0, k], uh) and pm[0, k] == pm_ref
        seen += 1
    assert seen >= 8


# ---- rules 8, 10, 11-13 on a hand-made list --------------------------------------------------------------------------------
def _toy():
    # two frames, L = 4, N = 32.  Frame 0: count 3 (one padding rank), frame 1: count 4
    rng = np.random.default_rng(1)
    paths = rng.integers(0, 2, (2, 4, 32)).astype(np.int32)
    paths[:, :, 5] = 0               # every path agrees on 0 at position 5
    paths[:, :, 9] = 1               # and on 1 at position 9
    paths[0, :, 11] = (0, 1, 1, 0)
    paths[0, 3] = 0                  # padding
    pm = np.array([[1.0, 2.5, 4.0, np.inf], [0.5, 0.5, 3.0, 100.0]])
    rem = np.array([[7, 0, 7, 0], [1, 2, 2, 0]], dtype=np.uint32)
    count = np.array([3, 4], dtype=np.uint32)
    return paths, pm, rem, count


def test_select_and_gather_rules():
    paths, pm, rem, count = _toy()
    idx = LM.select(rem, count, [0, 7, 2, 9])
    assert idx.tolist() == [[1, 0, -1, -1], [3, -1, 1, -1]]
    # padding is never selected: frame 0's rank 3 has rem 0 and is the only other entry with it
    assert LM.select(rem[:, ::-1][:, :4], np.array([0, 0]), [0]).tolist() == [[-1], [-1]]
    g = LM.gather(paths, idx[:, 2])
    assert np.array_equal(g[0], paths[0, 0]) and np.array_equal(g[1], paths[1, 1])     # -1 -> rank 0


def test_soft_rules():
    paths, pm, rem, count = _toy()
    s = LM.soft(paths, pm, count, clamp=3.0)
    assert (s[:, 5] == 3.0).all() and (s[:, 9] == -3.0).all()                          # all agree: +-clamp
    assert s[0, 11] == 2.5 - 1.0                                                       # m_1 - m_0 over ranks 0..2
    # frame 1: the large metric difference is clamped; ties in pm give an exact 0 where ranks 0 and 1 differ
    j = int(np.flatnonzero(paths[1, 0] != paths[1, 1])[0])
    assert s[1, j] == 0.0 and np.abs(s).max() == 3.0
    # want_rem: only the matching ranks; frame 0 keeps ranks 0 and 2 (rem 7), frame 1 has no rem 7 and falls back to all ranks
    s7 = LM.soft(paths, pm, count, rem=rem, want_rem=7, clamp=64.0)
    sub = LM.soft(paths[:1, [0, 2]], pm[:1, [0, 2]], np.array([2]), clamp=64.0)
    assert np.array_equal(s7[0], sub[0])
    assert np.array_equal(s7[1], LM.soft(paths, pm, count, clamp=64.0)[1])
    assert s7[0, 11] == 4.0 - 1.0
    # x domain: the same rule on the codewords
    enc = np.stack([M.encode(paths[f]) for f in range(2)]).astype(np.int32)
    assert np.array_equal(LM.soft(paths, pm, count, domain=1, clamp=8.0), LM.soft(enc, pm, count, domain=0, clamp=8.0))
    # an empty list says "bit 0" everywhere
    assert (LM.soft(paths, pm, np.array([0, 0]), clamp=2.0) == 2.0).all()


# ---- the header and the library ----------------------------------------------------------------------------------------------
def test_header_documents_the_section():
    text = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    m = re.search(r"/\* --- List output.*?\*/", text, re.S)
    assert m, "no 'List output' section"
    sec = m.group(0)
    for k in range(1, 14):
        assert re.search(rf"^ \* +{k}\. ", sec, re.M), f"rule {k} is missing"
    for word in ("ascending (PM, slot)", "padding", "+inf", "POLAR_FLAG_RERANK", "POLAR_ENOKERNEL", "POLAR_EINVAL", "matches nothing",
                 "D^i mod g(D) = D^i", "positive means bit 0", "k_scl_list", "Out of scope"):
        assert word in sec, word
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"^int {name}\(polar_ctx \*ctx,", code, re.M), name


def test_library_exports_the_entry_points():
    import polardecoding_amd as pa
    lib = pa.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    for name in ("decode_list_device", "decode_list_batch", "list_select_device", "list_gather_device", "list_soft_device"):
        assert callable(getattr(pa.Decoder, name)), name
