"""CPU: the conditions that make tests/test_gpu_frozen_patterns.py meaningful (tests/frozen_patterns.py).

Coverage: over the N = 1024 families all 256 octet masks occur, leaf 0 is information in some and the last leaf frozen in
some, the leading all-frozen run is 0, 14, 15, 16 and 17 octets (and 15 octets plus 3 leaves), and for every span size
8 .. 256 an aligned all-frozen span follows an aligned all-information one and the reverse.  The sets cut from the 5G order
fail every one of these: over all A = 1 .. N - 1 at N = 1024 they reach 13 octet masks, 25 half-block and 54 block masks
(10, 21 and 42 at N = 128), leaf 0 is never information and the last leaf never frozen.

The reference: the CPU oracle reads frozen[j] leaf by leaf; here it is held to the independent numpy list decoder
dscl_model (tests/test_dyn_host.py) on every family -- decisions, metric and tie flag by ==, no frame left out -- for SC,
SCL and CA-SCL (CRC-6) at L = 1, 2, 8, 32 in f64 and f32 at N = 128 (12 frames each, 3 dB), and at N = 1024 for SC and for
SCL / CA-SCL (CRC-24C) with L = 8 (4 frames each).  The CRC positions I[0..r) are a seeded permutation's first entries, so
they lie anywhere in the set.  SC-Flip's model (tests/test_scf_host.py) needs no second model: its run without a flip is
held to the oracle's SC.  Frames with a median tie that the oracle reported on these frames (f64 and f32 runs counted
separately): none at N = 128 (0 of 2880 SCL and 0 of 2400 CA-SCL frame decodes); at N = 1024, 6 of 304 SCL frame decodes --
one each in octets_hi, islands_128_a, tail_32, tail_quarter, dense_all, anti5g -- and 13 of 264 CA-SCL ones -- two in
lead_15, one each in islands_16_a, islands_256_a, lead_14, lead_16, leaf0_run, tail_1, tail_8, dense_but_last, bern_0.1,
bern_0.5, anti5g.  Decisions, metric and flag of the model equal the oracle's on those frames too.

Refusals that need no device: polar_create answers POLAR_EINVAL for an info_order with a duplicate or an out-of-range
entry, and accepts every family (A == N included) up to the missing device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frozen_patterns as P  # noqa: E402
from test_dyn_host import FLAG_TIE, dscl_model  # noqa: E402
from test_scf_host import sc_run  # noqa: E402

CRC6 = (0, 5, 6)
CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)
TAPS = {128: CRC6, 1024: CRC24C}


# ---- coverage --------------------------------------------------------------------------------------------------------
def test_families_are_deterministic_masks():
    for N in (32, 64, 128, 256, 512, 1024, 2048):
        a, b = P.families(N), P.families(N)
        assert list(a) == list(b) and len(a) >= 23
        for name in a:
            assert np.array_equal(a[name], b[name]), name
            assert a[name].dtype == np.uint8 and a[name].shape == (N,) and set(np.unique(a[name])) <= {0, 1}
            assert (a[name] == 0).any(), name
            o1, o2 = P.order_of(a[name], 5), P.order_of(a[name], 5)
            assert np.array_equal(o1, o2) and sorted(o1.tolist()) == np.flatnonzero(a[name] == 0).tolist()
            q = P.q_of(a[name], o1)
            assert sorted(q) == list(range(N))
    assert len(P.families(1024)) == 38 and len(P.families(128)) == 30


def test_every_octet_mask_occurs():
    fam = P.families(1024)
    lo, hi = set(P.octets_of(fam["octets_lo"]).tolist()), set(P.octets_of(fam["octets_hi"]).tolist())
    assert lo == set(range(0, 128)) and hi == set(range(128, 256))
    seen = set()
    for m in fam.values():
        seen |= set(P.octets_of(m).tolist())
    assert seen == set(range(256))
    assert P.octets_of(fam["octets_hi"])[0] != 0xFF and P.octets_of(fam["octets_lo"])[0] != 0xFF
    small = P.families(128)
    have = set(P.octets_of(small["octets_lo"]).tolist()) | set(P.octets_of(small["octets_hi"]).tolist())
    assert {0x80, 0xFE, 0x7F, 0xFF, 0x00, 0x55} <= have and len(have) == 32


def test_first_and_last_leaf_take_both_values():
    for N in (128, 1024):
        fam = P.families(N)
        assert {int(m[0]) for m in fam.values()} == {0, 1}
        assert {int(m[-1]) for m in fam.values()} == {0, 1}
        assert (fam["leaf0"][:4] == [0, 0, 0, 1]).all() and not fam["leaf0_run"][:40].any()
        assert fam["tail_1"][-1] == 1 and fam["tail_8"][-8:].all() and fam["tail_32"][-32:].all()
        assert fam["tail_quarter"][-N // 4:].all() and not fam["dense_all"].any()
        for name, info in (("sparse_last", [N - 1]), ("sparse_first", [0]), ("sparse_5_half", [5, N // 2]),
                           ("sparse_1_2_penult", [1, 2, N - 2])):
            assert np.flatnonzero(fam[name] == 0).tolist() == info
        assert np.flatnonzero(fam["anti5g"] == 0).tolist() == sorted(P.q5g(N)[:N // 2])


def test_leading_runs():
    fam = P.families(1024)
    runs = {name: P.leading_frozen_octets(m) for name, m in fam.items()}
    assert {0, 14, 15, 16, 17, 127} <= set(runs.values())
    for p in (14, 15, 16, 17, 127):
        assert runs[f"lead_{p}"] == p and fam[f"lead_{p}"][8 * p] == 0
    first_info = int(np.flatnonzero(fam["lead_mid"] == 0)[0])
    assert first_info == 8 * 15 + 3 and runs["lead_mid"] == 15
    small = P.families(128)
    assert P.leading_frozen_octets(small["lead_14"]) == 14 and P.leading_frozen_octets(small["lead_15"]) == 15


def _span_transitions(mask, s):
    """(an aligned all-frozen span of s leaves directly after an aligned all-information one, the reverse)"""
    spans = np.asarray(mask).reshape(-1, s)
    fz, inf = spans.all(axis=1), ~spans.any(axis=1)
    return bool((inf[:-1] & fz[1:]).any()), bool((fz[:-1] & inf[1:]).any())


def test_spans_alternate_at_every_size():
    fam = P.families(1024)
    for s in P.ISLAND_SPANS:
        for ph in ("a", "b"):
            assert _span_transitions(fam[f"islands_{s}_{ph}"], s) == (True, True), (s, ph)
        assert fam[f"islands_{s}_a"][0] == 0 and fam[f"islands_{s}_b"][0] == 1
        # both phases inside one parent span too: the left child all-information and the right all-frozen, and the reverse
        pairs = {(bool(sp[:s].all()), bool(sp[s:].all())) for ph in ("a", "b") for sp in fam[f"islands_{s}_{ph}"].reshape(-1, 2 * s)}
        assert pairs == {(False, True), (True, False)}


def _masks_5g(N, w):
    q = P.q5g(N)
    seen = set()
    for A in range(1, N):
        m = np.ones(N, dtype=np.uint8)
        m[q[N - A:]] = 0
        seen |= {bytes(b) for b in m.reshape(-1, w)}
    return seen


def test_the_5g_sets_fail_the_same_checks():
    """the gap the families close, as figures"""
    assert [len(_masks_5g(1024, w)) for w in (8, 16, 32)] == [13, 25, 54]
    assert [len(_masks_5g(128, w)) for w in (8, 16, 32)] == [10, 21, 42]
    octs = sorted(int(P.octets_of(np.frombuffer(b, dtype=np.uint8))[0]) for b in _masks_5g(1024, 8))
    assert octs == [0x00, 0x01, 0x03, 0x05, 0x07, 0x17, 0x1F, 0x37, 0x3F, 0x57, 0x5F, 0x7F, 0xFF]
    q = P.q5g(1024)
    assert q[0] == 0 and q[-1] == 1023       # leaf 0 is the last to become information, leaf N - 1 the last to be frozen
    for A in range(1, 1024):
        m = np.ones(1024, dtype=np.uint8)
        m[q[1024 - A:]] = 0
        assert m[0] == 1 and m[-1] == 0
        for s in (64, 128, 256):             # above 32 leaves no all-frozen span ever follows an all-information one
            assert _span_transitions(m, s)[0] is False


def test_no_crc_lists_are_the_small_families():
    for N, r in P.CRC_R.items():
        fam = P.families(N)
        assert tuple(k for k, m in fam.items() if int((m == 0).sum()) <= r) == P.NO_CRC[N]
        assert list(P.with_crc(fam, N)) == [k for k in fam if k not in P.NO_CRC[N]]
        assert len(P.with_crc(fam, N)) == len(fam) - 5


# ---- the oracle against a second model ---------------------------------------------------------------------------------
def _frames(oracle, code, B, seed, db):
    sig = oracle.sigma_from_db(db)
    _, ys = oracle.Sim(seed).frames(code, sig, B)
    return np.stack([oracle.llr_from_y(y, sig) for y in ys])


def _against_model(oracle, N, name, mask, algo, Ls, B, seed):
    """oracle.decode == dscl_model on B frames of family `name`, f64 and f32; returns (frames compared, tie frames)"""
    taps = TAPS[N] if algo == "CASCL" else None
    r = max(taps) if taps else 0
    A = int((mask == 0).sum())
    order = P.order_of(mask, seed)
    code = oracle.Code(N, A - r, taps, Q=P.q_of(mask, order))
    assert np.array_equal(code.frozen, mask) and np.array_equal(code.info_order, order)
    llr = _frames(oracle, code, B, seed, 3.0)
    done = ties_seen = 0
    for dtype, ds in ((np.float64, "f64"), (np.float32, "f32")):
        for L in Ls:
            ref, ref_pm, ties = oracle.decode(code, llr, algo, L=L, dtype=ds)
            u, pm, fl = dscl_model(mask, None, llr, L, crc=(order, taps) if taps else None, dtype=dtype, sc=(algo == "SC"),
                                   oracle=oracle)
            tag = (N, name, algo, L, ds)
            assert np.array_equal(u, ref), tag
            if algo != "SC":
                assert np.array_equal(pm, np.asarray(ref_pm).astype(np.float64)), tag
                assert np.array_equal((fl & FLAG_TIE) != 0, ties > 0), tag
            done += B
            ties_seen += int((ties > 0).sum())
    return done, ties_seen


def _over_families(oracle, N, fam, algo, Ls, B, seed):
    """_against_model over the families: (frames compared, tie frames); prints the families with tie frames"""
    res = [_against_model(oracle, N, name, mask, algo, Ls, B, seed + k) for k, (name, mask) in enumerate(fam.items())]
    tied = {name: t for name, (_, t) in zip(fam, res) if t}
    if tied:
        print(f"N={N} {algo}: tie frames per family {tied}")
    return sum(d for d, _ in res), sum(t for _, t in res)


@pytest.mark.parametrize("algo", ["SC", "SCL", "CASCL"])
def test_oracle_equals_the_model_on_every_family_n128(algo, oracle):
    fam = P.families(128)
    if algo == "CASCL":
        fam = P.with_crc(fam, 128)
    done, ties = _over_families(oracle, 128, fam, algo, (1,) if algo == "SC" else (1, 2, 8, 32), 12, 900)
    print(f"N=128 {algo}: {len(fam)} families, {done} frames compared, {ties} with a median tie")
    assert done == len(fam) * 12 * 2 * (1 if algo == "SC" else 4)
    assert ties == 0                                         # the figure of the module docstring


@pytest.mark.parametrize("algo", ["SC", "SCL", "CASCL"])
def test_oracle_equals_the_model_on_every_family_n1024(algo, oracle):
    fam = P.families(1024)
    if algo == "CASCL":
        fam = P.with_crc(fam, 1024)
    done, ties = _over_families(oracle, 1024, fam, algo, (1,) if algo == "SC" else (8,), 4, 1900)
    print(f"N=1024 {algo}: {len(fam)} families, {done} frames compared, {ties} with a median tie")
    assert done == len(fam) * 4 * 2
    assert ties == {"SC": 0, "SCL": 6, "CASCL": 13}[algo]    # the figures of the module docstring


@pytest.mark.parametrize("N", [128, 1024])
def test_scf_models_run_without_a_flip_is_the_oracles_sc(N, oracle):
    for k, (name, mask) in enumerate(P.with_crc(P.families(N), N).items()):
        order = P.order_of(mask, 40 + k)
        sc = oracle.Code(N, order.size, None, Q=P.q_of(mask, order))
        llr = _frames(oracle, sc, 6, 300 + k, 2.0)
        for dtype, ds in ((np.float64, "f64"), (np.float32, "f32")):
            u, lam = sc_run(oracle, mask, llr, dtype=dtype)
            ref, _, _ = oracle.decode(sc, llr, "SC", dtype=ds)
            assert np.array_equal(u, ref), (N, name, ds)
            assert not u[:, mask != 0].any()


# ---- refusals that need no device ----------------------------------------------------------------------------------------
def _create(pa, N, order, algo, taps=None, L=8):
    lib = pa.load_library()
    cfg = pa.api._Cfg()
    t = np.asarray(taps if taps else [0], dtype=np.int32)
    io = np.ascontiguousarray(order, dtype=np.int32)
    r = max(taps) if taps else 0
    cfg.N, cfg.K, cfg.L, cfg.algo = N, io.size - r, L, algo
    cfg.crc_r, cfg.n_taps = r, (len(taps) if taps else 0)
    cfg.crc_taps = t.ctypes.data_as(C.POINTER(C.c_int)) if taps else None
    cfg.info_order = io.ctypes.data_as(C.POINTER(C.c_int))
    cfg.bp_iters, cfg.dtype, cfg.device = 5, pa.F64, 1 << 20   # no such device: a valid request ends in POLAR_EDEVICE
    h = C.c_void_p()
    rc = lib.polar_create(C.byref(cfg), C.byref(h))
    assert not h.value
    return rc


def test_polar_create_checks_the_information_set_before_the_device():
    import polardecoding_amd as pa
    EINVAL, EDEVICE = -1, -3
    for N in (128, 1024):
        fam = P.families(N)
        for k, (name, mask) in enumerate(fam.items()):
            order = P.order_of(mask, k)
            for algo in (pa.ALGO_SC, pa.ALGO_SCL, pa.ALGO_BP, pa.ALGO_SCAN):
                assert _create(pa, N, order, algo) == EDEVICE, (N, name, algo)      # A == N included (dense_all)
            if name not in P.NO_CRC[N]:
                for algo in (pa.ALGO_CASCL, pa.ALGO_SCF):
                    assert _create(pa, N, order, algo, TAPS[N]) == EDEVICE, (N, name, algo)
            else:                                                                   # K = A - r < 1
                assert _create(pa, N, order, pa.ALGO_CASCL, TAPS[N]) == EINVAL, (N, name)
        order = P.order_of(fam["bern_0.5"], 1)
        dup = order.copy()
        dup[-1] = dup[0]
        assert _create(pa, N, dup, pa.ALGO_SCL) == EINVAL
        for bad in (-1, N, N + 5):
            oob = order.copy()
            oob[3] = bad
            assert _create(pa, N, oob, pa.ALGO_SCL) == EINVAL, bad
            assert _create(pa, N, oob, pa.ALGO_SC) == EINVAL, bad
        assert _create(pa, N, order, pa.ALGO_SCL) == EDEVICE
