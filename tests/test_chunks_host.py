"""CPU: the cases of tests/chunk_cases.py do what they are there for, from the models alone.

tests/test_gpu_chunks.py runs the chunked host loops of csrc/polar_hip.hip and csrc/h_*.hip across pass boundaries and compares with ==.  It
can only see a slipped offset if the frames really spread over several passes and if the frames of the later passes have
something to get wrong: a frame decided at every level, lists built from the sets of the level before, open frames of every
class.  Those conditions are asserted here, not assumed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bpl_model as BM  # noqa: E402
import chunk_cases as CC  # noqa: E402
import q8_model as QM  # noqa: E402
import test_gpu_dscf as DS  # noqa: E402
import test_rm_host as RM  # noqa: E402

FLAG_CRC_PASS = 2


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.name)
def test_frames_spread_over_the_passes(case, oracle):
    ps = CC.passes(case, oracle)
    print(case.name, ps)
    assert ps
    if case.kind == "even":
        what, n, ch = ps[0]
        assert n == 2 * ch, ps
        return
    if case.kind == "small":   # a row loop: one full pass and a frame; the later attempts of BPL: less than one pass
        assert all(n < ch if case.loop == "bpl" else ch < n < 2 * ch for _, n, ch in ps), ps
        return
    assert case.kind == "ragged"
    for k, (what, n, ch) in enumerate(ps):
        # the adaptive rule's last stage: more than one pass and a partial one (its frames are those that failed twice)
        least = ch if (case.loop == "adaptive" and k > 0) else 2 * ch
        assert n > least, (what, n, ch)
        assert ch == 1 or n % ch != 0, (what, n, ch)
        assert 1 <= ch <= 64


def test_every_loop_has_a_ragged_and_an_even_case():
    for loop in CC.LOOPS:
        kinds = {c.kind for c in CC.CASES if c.loop == loop}
        assert {"ragged", "even"} <= kinds, (loop, kinds)
    assert len({c.name for c in CC.CASES}) == len(CC.CASES)
    # the SC-Flip loops run with 1 <= CH <= 12, and one case with CH = 1
    chs = [ch for c in CC.DSCF_CASES for ch in CC.dscf_ch(c)]
    assert min(chs) == 1 and max(chs) <= 12 and len(set(chs)) >= 4, chs
    for c in CC.SCF_CASES:
        assert 2 <= CC.rows_per_pass(c.cap, CC.pair_bytes(CC.SCF_N) * c.spec[0], CC.SCF_FLOOR) <= 12
    # the row loops: one byte is below every row, RM_CAP below a row of the rate-matched shapes in either input type
    assert CC.rows_per_pass(CC.ROW_CAP, 1, CC.ROW_FLOOR) == 64 and CC.rows_per_pass(CC.RM_CAP, CC.RM_N * 4, CC.ROW_FLOOR) == 64
    assert CC.rows_per_pass(CC.RM_CAP, CC.pair_bytes(CC.RM_N) * 8, CC.SCF_FLOOR) == 3    # SC-Flip T = 8 inside a pass
    assert CC.rows_per_pass(CC.RM_CAP, CC.pair_bytes(CC.RM_N) * 4, CC.SCF_FLOOR) == 6    # dynamic (4, 4) inside a pass
    N, K, E, B, _ = CC.FER_CASE.spec
    half = (B // 2 + 63) // 64 * 64   # fer_batch_impl's two lanes
    assert half > 2 * 64 and B - half > 2 * 64


def test_rate_matched_shapes_are_one_of_each_mode():
    assert sorted(m for _, _, m in CC.RM_E) == sorted((RM.PUNCTURE, RM.SHORTEN, RM.REPEAT))
    assert sum(ibil for _, ibil, _ in CC.RM_E) >= 1
    for E, _, mode in CC.RM_E:
        for A in (CC.RM_K, CC.RM_K + 6):   # without and with CRC-6
            assert RM.mode_of(CC.RM_N, A, E) == mode, (E, A)
            assert RM.info_order(CC.RM_N, A, E) is not None
        x = CC.rm_rows(E)
        assert x.shape == (CC.B_RAGGED, E) and np.array_equal(x, x.astype(np.float32).astype(np.float64))


def test_q8_ternary_rows_tie_in_every_frame():
    want = CC.q8_want("scl4", "ternary")
    assert (want[2] & QM.FLAG_TIE).all()
    assert np.abs(CC.q8_rows("ternary") * 2).max() == 1
    x = CC.q8_rows("gauss")
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))   # a float input quantises to the same rows


@pytest.mark.parametrize("case", [c for c in CC.AD_CASES if c.kind == "ragged"], ids=lambda c: c.name)
def test_adaptive_every_list_size_decides_a_frame(case, oracle):
    dt, kind = case.spec
    (_, n1, ch), (_, n2, _) = CC.passes(case, oracle)
    assert n1 > 2 * ch and n2 > ch
    uh, pm, fl, ls = CC.ad_want(oracle, kind, dt)
    assert all((ls == L).any() for L in CC.AD_STAGES), np.unique(ls, return_counts=True)
    assert (fl & FLAG_CRC_PASS).any() and not (fl & FLAG_CRC_PASS).all()


@pytest.mark.parametrize("case", CC.SCF_CASES, ids=lambda c: c.name)
def test_static_flip_cases_decide_and_fail(case, oracle):
    u, flags, attempts, sets, fail = CC.scf_want(oracle, case)
    passed = (flags & FLAG_CRC_PASS) != 0
    assert (attempts == 0).any() and (passed[fail]).any() and (~passed).any()
    assert np.array_equal(sets[:, 0] >= 0, passed & (attempts >= 1)) and (sets[:, 1:] == -1).all()
    if case.kind == "ragged":   # flips decide frames of the middle passes and one of the last, partial pass
        ch = CC.passes(case, oracle)[0][2]
        hit = np.flatnonzero(passed[fail])
        assert (hit >= ch).sum() > 10 and hit.max() >= len(fail) - len(fail) % ch


@pytest.mark.parametrize("case", [c for c in CC.DSCF_CASES if c.kind == "ragged"], ids=lambda c: c.name)
def test_dynamic_flip_cases(case, oracle):
    N, budgets, c, dtype, rows = case.spec
    want = CC.dscf_want(oracle, case)
    per, none = DS.levels_decided(want, budgets)
    print(case.name, "decided per level", per, "by none", none, "frames per level", [len(l) for l in want.lists])
    assert all(p > 0 for p in per) and none > 0, (per, none)
    chs = CC.dscf_ch(case)
    if len(set(budgets)) > 1:
        assert len(set(chs)) == len(set(budgets)), chs   # CH differs from level to level
    if rows == "quantised":
        assert all(len(t) > 0 for t in want.ties), [len(t) for t in want.ties]   # equal keys at the end of a list, every level
    # a frame that sits in a later pass at level k and at level k + 1, whose level-(k + 1) list extends level-k sets: the
    # lists its pairs wrote at level k were found through the per-pass offsets, and k_scf_merge read them across passes
    found = 0
    for k in range(1, len(budgets)):
        slot_a = {f: s for s, f in enumerate(want.lists[k - 1])}
        for s, (f, lst) in enumerate(want.lists[k].items()):
            if s >= chs[k] and slot_a[f] >= chs[k - 1] and lst and all(len(e[3]) == k + 1 for e in lst):
                assert all(e[3][:k] == want.lists[k - 1][f][e[1]][3] for e in lst)   # entry q extends set q of the level before
                found += 1
    assert found > 0


def test_dynamic_flip_unequal_budgets_case_is_there():
    assert any(len(set(c.spec[1])) == 3 for c in CC.DSCF_CASES)
    assert any(c.spec[3] == np.float32 for c in CC.DSCF_CASES) and any(c.spec[0] == 1024 for c in CC.DSCF_CASES)


def test_bpl_cases(oracle):
    later_big = later_small = False
    for case in CC.BPL_CASES:
        res = CC.bpl_want(oracle, case)
        code = CC.bpl_code(oracle, case)
        P = len(CC.bpl_graphs(code.n, case.spec[3]))
        counts = [len(a["frames"]) for a in res.attempts]
        cls = BM.classes(res, P)
        print(case.name, "frames per attempt", counts, "classes (graph 0, graph >= 1, none)", cls)
        assert min(cls) >= 1, (case.name, cls)
        later_big |= any(n > 2 * CC.ROW_FLOOR for n in counts[1:])
        later_small |= any(0 < n < CC.ROW_FLOOR for n in counts[1:])
        if case.spec[4]:   # CRC-aided: a frame that converges at attempt 0, fails the CRC and is accepted by a later graph
            a0 = res.attempts[0]
            later = a0["conv"] & ~a0["crcok"] & (res.graph >= 1) & (res.graph < P)
            assert later.sum() >= 1
        first_is_identity = CC.bpl_graphs(code.n, case.spec[3])[0] == list(range(code.n))
        assert first_is_identity == (case.loop == "bpl")   # "bpl0": attempt 0 goes through the staged loop
    assert later_big and later_small
    assert any(c.spec[4] for c in CC.BPL_CASES)
