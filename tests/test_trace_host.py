"""CPU: the numpy model of the "Sent-path trace" section (tests/trace_model.py) against what already stands -- the list model
of tests/list_model.py and its kstar() -- the cases of tests/trace_cases.py against the condition that keeps them from passing
vacuously, and the C ABI: the header documents the section and declares the three entry points, polar_hip.map exports them."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
import list_model as LM  # noqa: E402
import trace_cases as TC  # noqa: E402
import trace_model as TM  # noqa: E402

HOST_CASES = ["n32-l4", "n64-l8", "n64-crc6-l4", "n128-l2", "n32-l1", "wide-n64-l64", "pac64-l8", "rdyn64-l4", "rm-n64-e48-l8",
              "sys-n64-crc6-l4"]


def _frozen(name):
    N = TC.CASES[name][1]
    io, dyn, crc = TC.case_code(name)
    frozen = np.ones(N, dtype=np.uint8)
    frozen[io] = 0
    return frozen, dyn, crc


@pytest.mark.parametrize("name", HOST_CASES)
def test_rank_and_chosen_are_the_row_comparison_on_the_list_model(name):
    """rules 5 and 6 as they are written: rank by comparing the rows of list_model()'s output with the sent word, chosen by
    kstar(); and loss_leaf == N <=> rank >= 0"""
    kind, N, K, L, taps, seed = TC.CASES[name]
    frozen, dyn, crc = _frozen(name)
    u, llr, _, _ = TC.pool(name)
    loss_leaf, loss_rank, rank, chosen, flags = TC.model(name)
    paths, pm, rem, count, l_flags = LM.list_model(frozen, dyn, llr, L, crc=crc)
    hit = (paths == u[:, None, :]).all(-1) & (np.arange(L)[None, :] < count[:, None])
    assert (hit.sum(1) <= 1).all()                                        # rule 2: at most one live slot matches
    assert np.array_equal(rank, np.where(hit.any(1), hit.argmax(1), -1))
    assert np.array_equal(chosen, LM.kstar(rem, count, crc is not None))
    assert np.array_equal(flags, l_flags)
    assert np.array_equal(loss_leaf == N, rank >= 0)
    assert (loss_rank[loss_leaf == N] == 0).all()
    assert ((loss_rank == 0) | (loss_rank > L)).all() and (loss_rank <= 2 * L).all()   # rule 4: the sent candidate failed the test


@pytest.mark.parametrize("name", list(TC.CASES))
def test_cases_meet_the_condition(name):
    """no pool passes vacuously: every class and at least three loss leaves are there, on the model alone; the planted rows do
    what they were planted for"""
    N = TC.CASES[name][1]
    res = TC.model(name)
    TC.check_condition(name, res)
    loss_leaf, loss_rank, rank, chosen, flags = res
    j0 = TC.pool(name)[3]
    assert loss_leaf[-2] == j0 and loss_rank[-2] == 0 and rank[-2] == -1    # a forced bit the sent word disagrees with
    assert loss_leaf[-1] == N and rank[-1] == chosen[-1]                     # the noiseless row: correct


def test_issue_counts():
    """the class counts of the oracle frames the cases were chosen by: 96 frames each, the first 64 at N = 128"""
    want = {"n32-l4": (80, 9, 7), "n64-l8": (72, 14, 10), "n128-l2": (45, 2, 17), "n64-crc6-l4": (66, 0, 30),
            "n64-crc6-l8": (77, 0, 19), "n32-l1": (66, 0, 30)}
    for name, w in want.items():
        res = TC.model(name)
        B = 64 if name == "n128-l2" else TC.FRAMES
        n = np.bincount(TM.classes(res[2][:B], res[3][:B]), minlength=3)
        assert tuple(n) == w, (name, n)


def test_a_list_that_cannot_prune_never_loses():
    """N = 32 with six information leaves and L = 64 = 2^6: the list holds every word of the code"""
    import polardecoding_amd as pa
    N, K, L, B = 32, 6, 64, 24
    io = np.asarray(pa.q_sequence(N)[N - K:], dtype=np.int32)
    frozen = np.ones(N, dtype=np.uint8)
    frozen[io] = 0
    u, llr = TC.M.make_frames(N, io, None, B, 3, dbs=(-7.0,))
    loss_leaf, loss_rank, rank, chosen, flags = TM.trace_model(frozen, None, llr, u, L)
    assert (loss_leaf == N).all() and (loss_rank == 0).all() and (rank >= 0).all() and (chosen == 0).all()
    assert (rank > 0).any()                                              # at -7 dB the sent word is not always the best one


def test_a_one_on_a_frozen_leaf_is_lost_there():
    kind, N, K, L, taps, seed = TC.CASES["n64-l8"]
    frozen, dyn, crc = _frozen("n64-l8")
    u, llr, _, _ = TC.pool("n64-l8")
    for j0 in np.flatnonzero(frozen)[[0, 5, -1]]:
        v = u[-1:].copy()
        v[0, j0] = 1
        loss_leaf, loss_rank, rank, chosen, flags = TM.trace_model(frozen, dyn, llr[-1:], v, L)
        assert loss_leaf[0] == j0 and loss_rank[0] == 0 and rank[0] == -1


def test_count_model():
    res = TC.model("n64-l8")
    N = 64
    h = TM.count(N, res[0], res[2], res[3])
    assert h[N + 3] == res[0].size and h[N:N + 3].sum() == h[N + 3] and h[:N].sum() == h[N + 2]
    assert np.array_equal(TM.count(N, res[0], res[2], res[3], hist=h), 2 * h)


def test_pack_inverts_unpack():
    u = TC.pool("n128-l2")[0]
    assert np.array_equal(LM.unpack(TM.pack(u), 128), u)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
NAMES = ("polar_list_trace", "polar_list_trace_count", "polar_list_trace_host")


def test_trace_abi_is_declared_documented_and_exported():
    import ctypes as C
    hdr = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    assert "Sent-path trace" in hdr
    sec = hdr[hdr.index("--- Sent-path trace"):]
    assert hdr.index("--- List output") < hdr.index("--- Sent-path trace") < hdr.index("--- Code books")
    for k in range(1, 10):                                                 # the numbered rules
        assert re.search(r"^ \*   %d\. " % k, sec, re.M), k
    for n in NAMES:
        assert re.search(r"^int %s\(polar_ctx \*" % n, hdr, re.M), n
    assert "polar_list_trace" in open(os.path.join(REPO, "polardecoding_amd", "csrc", "polar_hip.map")).read()
    import polardecoding_amd as pa
    lib = pa.load_library()
    for n in NAMES:
        assert hasattr(lib, n), n
    # refusals that touch no device
    assert lib.polar_list_trace(None, None, 0, C.c_double(0.0), None, 0, None, None, None, None, None) == -1
    assert lib.polar_list_trace_count(None, None, None, None, 0, None) == -1
    assert lib.polar_list_trace_host(None, None, None, 0, None, None, None, None, None) == -1
