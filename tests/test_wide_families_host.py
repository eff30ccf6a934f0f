"""CPU: the conditions that make tests/test_gpu_wide_families.py meaningful (tests/wide_families.py), on the model and the
oracle alone.

The device file compares k_scl_wide with dscl_model (tests/test_dyn_host.py) at L = 128 and 256.  What is new there is the
code that crosses wavefronts: the rank of a dead slot over the wavefronts below it, the walk over the per-wavefront lists of
both-survivors, the un-refilled dead slot, the tie flag from counts summed over wavefronts.  dscl_model's `trace` reports per
frame whether a phase-2 leaf had

  tie         fewer than L candidates survive (FLAG_TIE)
  cross       a refilled slot whose source slot lies in another group of 64 slots (another wavefront of the kernel)
  unrefilled  a dead slot that is not refilled (rank >= n_both) and continues as its 0-branch
  all_equal   all 2L candidates equal: every slot dead, n_both = 0

and the floors below are asserted on the mixed and `cycle` batches of groups 2 to 5 (w2 .. w5), case by case, for every
mask that is rate 1/2 or denser: tie and unrefilled in at least half of the frames, cross in at least a quarter, and at least
one all_equal frame per group and configuration.  Measured here (frames of 24 / 12 / 16 / 8):

  w2  N = 64,  L = 128, 24 frames   tie = unrefilled 20 .. 24, cross 11 .. 20, all_equal 4 .. 10
      N = 64,  L = 256, 12 frames   tie = unrefilled 12,       cross 8 .. 9,   all_equal 4 .. 5
  w3  N = 128, L = 256, 12 frames   tie = unrefilled 12,       cross 6 .. 11,  all_equal 2 .. 9
  w4  CA-SCL,  L = 128, 16 frames   tie = unrefilled 14 .. 16, cross 9 .. 16,  all_equal 1 .. 12;  L = 256: 15 .. 16, 15 .. 16, 1 .. 12
  w5  (64, 128), 16 frames          tie = unrefilled 14 .. 16, cross 12 .. 16, all_equal 0 .. 4
      (128, 256), 8 frames          tie = unrefilled 8,        cross 7 .. 8,   all_equal 0 .. 6
On the Gaussian rows of group 7 the model flags no tie at all.

EXEMPT lists, by name and with the reason, the masks too sparse for the per-case floors (the device file compares them like
all others); at most a third of the masks of a length may be exempt.  Also here: the case table, the mixed batch against
the one of tests/test_gpu_llr_families.py, the model against the oracle at L = 64 on three of the masks, and that every
constraint case sets dynamic bits and errs.  The model runs of this file take about a minute."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frozen_patterns as P  # noqa: E402
import llr_families as F  # noqa: E402
import test_dyn_host as M  # noqa: E402
import wide_families as W  # noqa: E402

# masks below rate 1/2, or with so few information leaves behind the point where the list is full that fewer than half of the
# frames rank at all: no per-case floor
EXEMPT = {
    "sparse_last": "K = 1: the list never fills, no phase 2",
    "sparse_first": "K = 1: the list never fills, no phase 2",
    "sparse_5_half": "K = 2: the list never fills, no phase 2",
    "sparse_1_2_penult": "K = 3: the list never fills, no phase 2",
    "lead_7": "N = 64, K = 4: the list never fills",
    "lead_14": "N = 128, K = 8 <= log2 L: at most one ranking leaf",
    "lead_15": "N = 128, K = 4: the list never fills",
    "bern_0.9": "rate 1/8: K = 8 at N = 64, 13 at N = 128, few ranking leaves",
    "tail_32": "N = 64: K = 11 with the last 32 leaves frozen, four ranking leaves at L = 128",
}
GROUP_SIZES = {"w1": 24, "w2": 60, "w3": 30, "w4": 28, "w5": 97, "w6": 3, "w7": 30, "w10": 1}
# (group, L, dtype) of the floors: every configuration of groups 2 to 5
CONFIGS = [("w2", 128, "f64"), ("w2", 128, "f32"), ("w2", 256, "f32"), ("w2", 256, "f64"), ("w3", 256, "f32"), ("w3", 256, "f64"),
           ("w4", 128, "f32"), ("w4", 256, "f64"), ("w5", 128, "f64"), ("w5", 128, "f32"), ("w5", 256, "f32"), ("w5", 256, "f64")]


def _group(name):
    return [c for c in W.cases() if c.group == name]


def test_case_table():
    cs = W.cases()
    assert {g: len(_group(g)) for g in W.GROUPS} == GROUP_SIZES and len(cs) == sum(GROUP_SIZES.values())
    assert len({W.tag(c) for c in cs}) == len(cs)
    assert {(c.group, c.L, c.dtype) for c in cs if c.group in ("w2", "w3", "w4", "w5")} == set(CONFIGS)
    assert all(c.L >= 128 for c in cs if c.group != "w7" and c.group != "w6") and {c.L for c in _group("w7")} == {32, 128, 256}
    for dt in ("f64", "f32"):
        assert [c.mask for c in _group("w2") if (c.L, c.dtype) == (128, dt)] == list(P.families(64))
    assert len(P.families(64)) == 27 and len(P.families(128)) == 30
    for m, c in enumerate(_group("w3")):
        assert (c.mask, (c.L, c.dtype)) == (list(P.families(128))[m], W.W3_CONFIGS[m % 2])
    assert [c.mask for c in _group("w4") if c.L == 128] == list(P.with_crc(P.families(128), 128))
    assert set(W.RESEED) <= {W.tag(c) for c in cs}
    # what the masks are for: leaf 0 information, the list full before the first frozen leaf, a frozen last leaf, rate 1
    f64m, f128m = P.families(64), P.families(128)
    assert f128m["leaf0"][0] == 0 and not f64m["leaf0_run"][:40].any() and f128m["tail_1"][-1] == 1 and not f128m["dense_all"].any()
    # at most a third of the masks of a length without a floor
    for fam in (f64m, f128m):
        assert 3 * sum(name in EXEMPT for name in fam) <= len(fam)
    for N, masks in W.W7_MASKS.items():
        assert all(int((P.families(N)[m] == 0).sum()) <= 5 for m in masks)       # 2^K <= 32: never a ranking leaf
        assert [m for m, v in P.families(N).items() if int((v == 0).sum()) <= 5] == sorted(masks, key=list(P.families(N)).index)


def test_mixed_batch_is_the_one_of_the_llr_families_tests():
    import test_gpu_llr_families as G
    llr = np.random.default_rng(3).standard_normal((24, 64)) * 3.0
    for dtype in ("f64", "f32"):
        a = W.mixed(llr, 5, np.float32 if dtype == "f32" else np.float64, copies=3)
        b = G._mixed(llr, 5, dtype)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    x = W.mixed(llr, 5, np.float64)
    names = {name: row for name, row in F.degenerate_rows(64, np.float64, 5, c=2.0)}
    for name, row in names.items():                    # planted once each
        assert sum(np.array_equal(r.view(np.uint64), row.view(np.uint64)) for r in x) >= 1, name
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()


@pytest.mark.parametrize("group,L,dtype", CONFIGS, ids=lambda v: str(v))
def test_cases_tie_leave_dead_slots_and_refill_across_wavefronts(group, L, dtype):
    cs = [c for c in _group(group) if (c.L, c.dtype) == (L, dtype)]
    assert cs
    all_equal = 0
    for c in cs:
        ref, tr = W.reference(c)
        (name,) = ref
        t = {k: int(v.sum()) for k, v in tr[name].items()}
        assert np.array_equal(tr[name]["tie"], (ref[name][2] & M.FLAG_TIE) != 0), W.tag(c)
        print(f"{W.tag(c)}: of {c.B} frames {t}{'  (exempt)' if c.mask in EXEMPT else ''}")
        all_equal += t["all_equal"]
        if c.mask in EXEMPT:
            continue
        assert 2 * t["tie"] >= c.B and 2 * t["unrefilled"] >= c.B and 4 * t["cross"] >= c.B, (W.tag(c), t)
    assert all_equal >= 1


def test_pointer_table_extremes_tie_in_every_frame():
    for c in _group("w6"):
        ref, tr = W.reference(c)
        (name,) = ref
        assert tr[name]["tie"].all() and tr[name]["unrefilled"].all(), W.tag(c)
        assert tr[name]["cross"].all() == (c.L > 64), W.tag(c)     # one wavefront at L = 64: nothing to cross


def test_constraint_cases_set_dynamic_bits_and_err():
    for c in _group("w5"):
        made, (ref, _) = W.materialise(c), W.reference(c)
        u = ref["cycle"][0]
        assert u[:, made.dyn[0]].any(), W.tag(c)
        assert (u != made.u).any(), W.tag(c)


@pytest.mark.parametrize("mask", ["leaf0", "islands_16_a", "dense_but_block"])
def test_model_at_L64_is_the_oracle_on_the_new_masks(mask, oracle):
    """48 AWGN frames at N = 128; frames on which the oracle reports a median tie are left out (its tie rule is not the
    library's), at most a quarter of them"""
    N, B, L = 128, 48, 64
    fz, order = W.mask_of(N, mask)
    code = oracle.Code(N, order.size, None, Q=P.q_of(fz, order))
    assert np.array_equal(code.frozen, fz) and np.array_equal(code.info_order, order)
    llr = F.oracle_llr(oracle, code, B, 900 + order.size, 3.0 if order.size > 64 else 1.5)
    ref, ref_pm, ties = oracle.decode(code, llr, "SCL", L=L)
    keep = ties == 0
    assert keep.sum() >= B * 3 // 4
    trace = {}
    u, pm, fl = M.dscl_model(fz, None, llr, L, oracle=oracle, trace=trace)
    assert np.array_equal(u[keep], ref[keep])
    assert np.array_equal(pm[keep], ref_pm[keep].astype(np.float64))
    assert not (fl[keep] & M.FLAG_TIE).any() and np.array_equal(trace["tie"], (fl & M.FLAG_TIE) != 0)
    assert not trace["cross"].any()                    # L = 64: one group of slots
    assert ref[keep].any()


def test_trace_leaves_the_results_unchanged():
    c = next(c for c in _group("w2") if (c.mask, c.L, c.dtype) == ("bern_0.5", 128, "f64"))
    made, (ref, tr) = W.materialise(c), W.reference(c)
    plain = M.dscl_model(made.mask, None, np.asarray(made.batches["mixed"], dtype=np.float64), c.L)
    for a, b in zip(plain, ref["mixed"]):
        assert np.array_equal(a, b)
    assert set(tr["mixed"]) == {"tie", "cross", "unrefilled", "all_equal"}
