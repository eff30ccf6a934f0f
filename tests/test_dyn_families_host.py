"""CPU: the conditions that make tests/test_gpu_dyn_families.py meaningful (tests/dyn_families.py), on the model and the
oracle alone.

The device file compares k_scl_dyn with dscl_model (tests/test_dyn_host.py) on every frame, median-tie frames included.
That can only fail where the cases reach the kernel's history machinery -- the refill of phase 2 runs only under the tie
rule or when a path dies -- so for every case of dyn_families.cases() the following is asserted here, not assumed:

  * the model with every set empty equals the oracle on every mask the cases use (decisions, metric, tie flag; no frame
    left out), so the model's survivor and refill rule is the oracle's on these masks;
  * frames with FLAG_TIE: at least one in every list case (L >= 2), and at least a third of the batch on every grid batch
    at L >= 8 (N = 32, 64), on the `split` batch at N = 1024 and over the N = 128 cases together;
  * at least one frame with a decision error, and some dynamic bit equal to 1 in the model's output;
  * fill_dynamic -> encode -> the model on the noiseless rows returns u exactly, for every case;
  * the structural claims about the constraint families (test_structure).

Cases that cannot meet a condition are listed in EXCEPTIONS with the conditions they miss; the table is asserted to be exact
(no case missing from it, none in it without cause), and it excuses the "shows something" assertions only -- the device file
compares those cases like all others.  Why they miss: word_edges at N = 32 refers to leaf 0 alone (a dynamic leaf with an
empty set); the first 32 leaves of the rm mask at N = 1024 are all frozen, so word0_only sums zeros there (the islands
mask carries word0_only instead); the dynamic leaves of islands_64_b, dense_but_first and sparse_last precede every
information leaf; dense_all has no frozen leaf at all (D = 0); the sparse_* masks have at most three information leaves, so
a list of 8 or 32 never fills (no phase 2, no tie), and lead_15 with L = 32 is the same; sparse_*, lead_14, lead_15 and, under
CRC-6 with L = 32, bern_0.9 decode most of their 16 frames at 1 and 3 dB without an error.

Measured with the model (frames with FLAG_TIE / frames in error / dynamic bits equal to 1, smallest .. largest over the
cases of the row; exceptions included):

  N = 32, 9 families x 8 input batches    L = 1 (SC), B = 65:   no flags / 197 .. 242 of 520 / 0 .. 1981
                                          L = 2 f32, B = 300:   591 .. 731 of 2400 (least batch 11) / 625 .. 693 / 0 .. 10715
                                          L = 32 f64, B = 300:  1707 .. 1844 of 2400 (least grid batch 135 of 300) / 588 .. 691 / 0 .. 10519
  N = 64, 9 families x 3 batches of 65    L = 2:   88 .. 108 of 195 (least batch 8) / 82 .. 106 / 87 .. 1642
                                          L = 8:   134 .. 152 of 195 (least grid batch 33 of 65) / 84 .. 114 / 91 .. 1723
  N = 128, 30 masks x 3 families, B = 16  SC: 30 cases, SCL L = 8 and L = 32: 30 cases each, CA-SCL: 25 cases; 0 .. 16 ties per
                                          case, 1088 tie frames in the 1216 frames of the list cases that tie at all
  N = 1024, B = 65 (`split`)              L = 32: 14 cases, 64 .. 65 ties / 34 .. 65 / 0 .. 16113
                                          L = 8:  6 cases, 54 .. 65 ties / 37 .. 65 / 0 .. 15566
                                          L = 1 (SC): 7 cases, no flags / 52 .. 65 / 0 .. 6509
The model runs take about half a minute for the whole file."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dyn_families as D  # noqa: E402
import frozen_patterns as P  # noqa: E402
from test_dyn_host import FLAG_TIE, dscl_model, encode, fill_dynamic  # noqa: E402

# case tag -> the conditions it cannot meet: "tie" (a list case without a tie frame), "err" (no decision error),
# "dyn1" (no dynamic bit equal to 1).  The reasons are in the module docstring.
EXCEPTIONS = {
    "32-rm-word_edges-L1-f64-SC-B65": "dyn1",
    "32-rm-word_edges-L2-f32-SCL-B300": "dyn1",
    "32-rm-word_edges-L32-f64-SCL-B300": "dyn1",
    "128-islands_64_b-bern_half-L1-f32-SC-B16": "dyn1",
    "128-islands_64_b-alternate-L32-f32-SCL-B16": "dyn1",
    "128-islands_64_b-dyn_chain-L8-f32-SCL-B16": "dyn1",
    "128-lead_14-bern_half-L8-f64-SCL-B16": "err",
    "128-lead_14-dyn_chain-L32-f64-SCL-B16": "err",
    "128-lead_15-bern_half-L32-f32-SCL-B16": "tie err",
    "128-lead_15-alternate-L8-f32-SCL-B16": "err",
    "128-lead_15-dyn_chain-L1-f32-SC-B16": "err",
    "128-sparse_last-bern_half-L1-f64-SC-B16": "err dyn1",
    "128-sparse_last-alternate-L32-f64-SCL-B16": "tie err dyn1",
    "128-sparse_last-dyn_chain-L8-f64-SCL-B16": "tie err dyn1",
    "128-sparse_first-bern_half-L8-f32-SCL-B16": "tie err",
    "128-sparse_first-dyn_chain-L32-f32-SCL-B16": "tie err",
    "128-sparse_5_half-bern_half-L32-f64-SCL-B16": "tie err",
    "128-sparse_5_half-alternate-L8-f64-SCL-B16": "tie err",
    "128-sparse_1_2_penult-alternate-L32-f32-SCL-B16": "tie err",
    "128-sparse_1_2_penult-dyn_chain-L8-f32-SCL-B16": "tie",
    "128-dense_all-bern_half-L8-f64-SCL-B16": "dyn1",
    "128-dense_all-alternate-L1-f64-SC-B16": "dyn1",
    "128-dense_all-dyn_chain-L32-f64-SCL-B16": "dyn1",
    "128-dense_but_first-bern_half-L32-f32-SCL-B16": "dyn1",
    "128-dense_but_first-alternate-L8-f32-SCL-B16": "dyn1",
    "128-dense_but_first-dyn_chain-L1-f32-SC-B16": "dyn1",
    "128-islands_64_b-bern_half-L32-f32-CASCL-B16": "dyn1",
    "128-lead_14-alternate-L8-f32-CASCL-B16": "err",
    "128-dense_all-dyn_chain-L32-f32-CASCL-B16": "dyn1",
    "128-dense_but_first-bern_half-L8-f32-CASCL-B16": "dyn1",
    "128-bern_0.9-dyn_chain-L32-f64-CASCL-B16": "err",
    "1024-rm-word0_only-L32-f64-SCL-B65": "dyn1",
    "1024-rm-word0_only-L32-f32-SCL-B65": "dyn1",
    "1024-rm-word0_only-L8-f64-SCL-B65": "dyn1",
    "1024-rm-word0_only-L1-f64-SC-B65": "dyn1",
}
GROUPS = ("n32", "n64", "n128", "n128crc", "n1024")
GROUP_SIZES = {"n32": 27, "n64": 36, "n128": 90, "n128crc": 25, "n1024": 27}


def _group(name):
    return [c for c in D.cases() if c.group == name]


def test_case_table():
    cs = D.cases()
    assert {g: len(_group(g)) for g in GROUPS} == GROUP_SIZES and len(cs) == sum(GROUP_SIZES.values())
    tags = {D.tag(c) for c in cs}
    assert set(EXCEPTIONS) <= tags
    # every N = 128 mask meets three SCL configurations, every constraint family all six
    for name in P.families(128):
        assert len({(c.L, c.dtype) for c in _group("n128") if c.mask == name}) == 3
    for f in D.N128_FAMS:
        assert len({(c.L, c.dtype) for c in _group("n128") if c.fam == f}) == 6
    for f in D.N1024_FAMS:
        assert {(c.L, c.dtype) for c in _group("n1024") if c.fam == f and c.mask == "rm"} == set(D.N1024_CONFIGS)
        assert all(any(c.fam == f and c.mask == m for c in _group("n1024")) for m in D.N1024_MASKS)
    assert {(c.L, c.dtype) for c in _group("n1024") if (c.mask, c.fam) == ("islands_16_a", "word0_only")} == set(D.N1024_CONFIGS)


# ---- the constraint families ---------------------------------------------------------------------------------------------
def _words(N, dyn):
    """[D][N/32] mask words of the sets"""
    return D.M.dyn_masks(N, dyn)[1]


def test_structure():
    rm1024, _ = D.mask_of(1024, "rm")
    fam = D.constraint_families(1024, rm1024, 5)
    again = D.constraint_families(1024, rm1024, 5)
    assert list(fam) == list(D.FAMILIES)
    for name in fam:
        assert np.array_equal(fam[name][0], again[name][0])
        assert all(np.array_equal(a, b) for a, b in zip(fam[name][1], again[name][1])), name
    fz = np.flatnonzero(rm1024)
    for name in fam:
        want = fz[::2] if name == "alternate" else fz
        assert np.array_equal(fam[name][0], want), name               # every frozen position dynamic (alternate: every second)
    # all_prev: every word below j >> 5 full in every row; on the islands mask (frozen up to leaf 1023; the rm mask ends in
    # word 29) rows with all 32 words non-zero -- the case that runs it is L = 32 in f32: S = 2, sixteen words per lane
    isl, _ = D.mask_of(1024, "islands_16_a")
    fam_isl = D.constraint_families(1024, isl, 5)
    for f in (fam, fam_isl):
        w = _words(1024, f["all_prev"])
        for d, j in enumerate(f["all_prev"][0]):
            assert (w[d, :j >> 5] == 0xFFFFFFFF).all() and not w[d, (j >> 5) + 1:].any()
    assert ((_words(1024, fam_isl["all_prev"]) != 0).sum(axis=1) == 32).sum() == 16
    assert any((c.mask, c.fam, c.L, c.dtype) == ("islands_16_a", "all_prev", 32, "f32") for c in D.cases())
    # word0_only: words 1 .. 31 are zero in every row; on the islands mask rows at j >= 992 with word 0 non-zero
    for f in (fam, fam_isl):
        assert not _words(1024, f["word0_only"])[:, 1:].any()
    late = fam_isl["word0_only"][0] >= 992
    assert late.sum() == 16 and (_words(1024, fam_isl["word0_only"])[late, 0] != 0).all()
    assert rm1024[:32].all() and (isl[:16] == 0).all()                 # word 0: all frozen on rm, information on the islands
    # own_word_only: only word j >> 5, the last one the kernel's loop reads
    w = _words(1024, fam["own_word_only"])
    for d, j in enumerate(fam["own_word_only"][0]):
        assert not np.delete(w[d], j >> 5).any() and int(w[d, j >> 5]) == (1 << (int(j) & 31)) - 1
    # prev_only: rows at j % 32 == 0 -- the one bit read is bit 31 of the word before
    pos, sets = fam["prev_only"]
    edge = [d for d, j in enumerate(pos) if j % 32 == 0 and j]
    assert len(edge) >= 8 and all(sets[d].tolist() == [pos[d] - 1] for d in edge) and sets[0].size == 0 and pos[0] == 0
    # word_edges: bits 0 and 31 of every word below j
    w = _words(1024, fam["word_edges"])
    assert set(np.unique(w).tolist()) <= {0, 1, 0x80000001}
    # dyn_chain refers to earlier dynamic bits (and to nothing else but one information bit)
    pos, sets = D.constraint_families(128, P.families(128)["bern_0.5"], 5)["dyn_chain"]
    mask = P.families(128)["bern_0.5"]
    assert max(s.size for s in sets) == 3 and any(mask[s].sum() == 2 for s in sets)
    assert all(mask[s].sum() <= 2 and (mask[s] == 0).sum() <= 1 for s in sets)
    # alternate: a plain frozen leaf and a dynamic leaf inside one octet
    pos, _ = D.constraint_families(128, mask, 5)["alternate"]
    plain = np.setdiff1d(np.flatnonzero(mask), pos)
    assert np.intersect1d(pos // 8, plain // 8).size >= 4
    # position 0 is dynamic in some masks, information in others
    lead = [D.mask_of(c.N, c.mask)[0][0] for c in D.cases()]
    assert {int(x) for x in lead} == {0, 1}
    assert D.mask_of(1024, "leaf0")[0][0] == 0 and rm1024[0] == 1 and fam["all_prev"][0][0] == 0
    # dense_all has no frozen position: D = 0
    assert D.constraint_families(128, P.families(128)["dense_all"], 5)["bern_half"][0].size == 0


# ---- the model with empty sets against the oracle ------------------------------------------------------------------------
def _frames(oracle, code, B, seed, db):
    sig = oracle.sigma_from_db(db)
    _, ys = oracle.Sim(seed).frames(code, sig, B)
    return np.stack([oracle.llr_from_y(y, sig) for y in ys])


def test_model_with_empty_sets_is_the_oracle_on_every_mask(oracle):
    """every (N, mask, L, dtype, algorithm) of the cases, the constraint positions of the case with every set emptied, on
    grid rows: ties included"""
    seen = set()
    frames = ties_seen = 0
    for c in D.cases():
        key = (c.N, c.mask, c.L, c.dtype, c.algo)
        if key in seen:
            continue
        seen.add(key)
        mask, order = D.mask_of(c.N, c.mask)
        taps = D.CRC6 if c.algo == "CASCL" else None
        code = oracle.Code(c.N, order.size - (6 if taps else 0), taps, Q=P.q_of(mask, order))
        assert np.array_equal(code.frozen, mask) and np.array_equal(code.info_order, order)
        B = 4 if c.N == 1024 else 8
        llr = D.F.grid(_frames(oracle, code, B, 700 + len(seen), 2.0), 0.5, 15)
        pos = D.constraint_families(c.N, mask, 5)["alternate" if c.fam == "alternate" else "all_prev"][0]
        empties = (pos, [np.zeros(0, dtype=np.int32)] * len(pos))
        ref, ref_pm, ties = oracle.decode(code, llr, c.algo, L=c.L, dtype=c.dtype)
        u, pm, fl = dscl_model(mask, empties, llr, c.L, crc=(order, taps) if taps else None, dtype=D.np_dtype(c),
                               sc=(c.algo == "SC"), oracle=oracle)
        assert np.array_equal(u, ref), key
        if c.algo != "SC":
            assert np.array_equal(pm, np.asarray(ref_pm).astype(np.float64)), key
            assert np.array_equal((fl & FLAG_TIE) != 0, ties > 0), key
            ties_seen += int((ties > 0).sum())
        frames += B
    print(f"{len(seen)} (mask, L, dtype, algorithm) compared with the oracle on {frames} frames, {ties_seen} with a median tie")
    assert len(seen) >= 130 and ties_seen * 4 >= frames


# ---- the conditions, case by case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_cases_tie_err_and_set_dynamic_bits(group):
    found = {}
    tie_frames = list_frames = 0
    for c in _group(group):
        made, ref = D.materialise(c), D.reference(c)
        ties = {k: int(((fl & FLAG_TIE) != 0).sum()) for k, (_, _, fl) in ref.items()}
        err = sum(int((u != made.u).any(axis=1).sum()) for u, _, _ in ref.values())
        dyn1 = sum(int(u[:, made.dyn[0]].sum()) for u, _, _ in ref.values())
        print(f"{D.tag(c)}: ties {ties}, frames in error {err}, dynamic ones {dyn1}")
        miss = []
        if c.algo == "SC":
            assert not any(fl.any() or pm.any() for _, pm, fl in ref.values())
        elif sum(ties.values()) == 0:
            miss.append("tie")
        if err == 0:
            miss.append("err")
        if dyn1 == 0:
            miss.append("dyn1")
        if miss:
            found[D.tag(c)] = " ".join(miss)
        if c.L >= 8 and "tie" not in miss:
            for name, t in ties.items():
                if name.startswith("grid") or name in ("split", "hard"):
                    assert group.startswith("n128") or 3 * t >= c.B, (D.tag(c), name, t)
            tie_frames += sum(ties.values())
            list_frames += c.B * len(ties)
        if c.L == 2:
            assert all(t >= 1 for t in ties.values()), (D.tag(c), ties)
    assert found == {k: v for k, v in EXCEPTIONS.items() if k in {D.tag(c) for c in _group(group)}}
    print(f"{group}: {tie_frames} tie frames in {list_frames} frames of the L >= 8 cases")
    assert 3 * tie_frames >= list_frames


@pytest.mark.parametrize("group", GROUPS)
def test_noiseless_frames_decode_to_u(group):
    """fill_dynamic -> encode -> the model: u exactly, so the sets, the frames and the model agree on every family"""
    for c in _group(group):
        made = D.materialise(c)
        u = made.u[:4]
        filled = fill_dynamic(np.where(made.mask == 0, u, 0).astype(np.int64), made.dyn)
        assert np.array_equal(filled, u), D.tag(c)
        got, _, _ = D.model(c, made, 8.0 * (1.0 - 2.0 * encode(u)))
        assert np.array_equal(got, u), D.tag(c)
