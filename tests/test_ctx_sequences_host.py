"""CPU: the table of the reused-context tests (tests/ctx_sequences.py) against include/polar_hip.h and against its own rules.

Every setter the header declares must be a change of some script (a setter added later fails here until a script uses it);
the batch sizes of every script must go small, large, small and back to the first large one; every change must be followed by
an observation, every setter must take three values in the pattern a, b, a; and -- sensitivity -- for every change whose two
states have a CPU model, the models must differ on the frames of the observation that follows it, in an output that the GPU
test compares: an observation that cannot tell the new state from the old one proves nothing.  Where two models agree, the
script's seed or Eb/N0 is what changes, never this criterion."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctx_sequences as S  # noqa: E402
import extents as X  # noqa: E402

IDS = [s.name for s in S.SCRIPTS]
SETTER_RE = re.compile(r"^polar_(set_\w+|\w+_set_\w+)$")
CAP = 24   # frames of an observation that the sensitivity check puts through the models


def header_setters(text=None):
    return sorted(n for n in X.prototypes(text) if SETTER_RE.match(n))


def setters_without_a_script(text=None, scripts=S.SCRIPTS):
    used = {S.SETTERS[st.what] for s in scripts for st in s.steps if isinstance(st, S.Chg) and st.what in S.SETTERS}
    return [n for n in header_setters(text) if n not in used and n not in S.ELSEWHERE]


def test_every_setter_of_the_header_is_a_change_of_some_script():
    names = header_setters()
    assert len(names) >= 10 and set(S.SETTERS.values()) <= set(names), names
    assert not (set(S.SETTERS.values()) & set(S.ELSEWHERE))
    assert setters_without_a_script() == []
    for where in S.ELSEWHERE.values():
        path, test = where.split("::")
        with open(os.path.join(S.REPO, path)) as f:
            assert re.search(rf"^def {test}\(", f.read(), re.M), where


def test_a_setter_without_a_script_is_found():
    with open(os.path.join(S.REPO, "include", "polar_hip.h")) as f:
        text = f.read()
    more = text.replace("int polar_set_stream(", "int polar_scan_set_damping(polar_ctx *ctx, double d);\nint polar_set_stream(")
    assert setters_without_a_script(more) == ["polar_scan_set_damping"]
    less = [s for s in S.SCRIPTS if s.name != "q8_128"]
    assert setters_without_a_script(None, less) == ["polar_q8_set_quant"]


def test_the_minimum_set_of_scripts_is_there():
    assert IDS == ["sc128", "scl128", "scl1024", "cascl1024", "cascl128", "bp128", "bp256", "scf128", "scan128", "bpl128", "q8_128",
                   "rm128", "dyn128", "wide128"]
    assert len({s.seed for s in S.SCRIPTS}) == len(S.SCRIPTS)


@pytest.mark.parametrize("script", S.SCRIPTS, ids=IDS)
def test_batches_go_small_large_small_and_back(script):
    for sc in (script, script.without_hooks()):
        bs = [st.B for st in sc.steps if isinstance(st, S.Obs)]
        assert any(bs[i] < bs[j] > bs[k] and bs[l] == bs[j]
                   for j in range(len(bs)) for i in range(j) for k in range(j + 1, len(bs)) for l in range(k + 1, len(bs))), bs
        assert all(b <= S.B_MAX or b in S.BIG_B for b in bs), bs


@pytest.mark.parametrize("script", S.SCRIPTS, ids=IDS)
def test_every_change_is_followed_by_an_observation_that_sees_it(script):
    steps = script.steps
    assert isinstance(steps[-1], S.Obs)
    for i, st in enumerate(steps):
        if not isinstance(st, S.Chg):
            continue
        assert st.what in S.SETTERS or st.what in S.HOOKS or st.what == "frozen_mask", st
        nxt = steps[i + 1]
        assert isinstance(nxt, S.Obs), (i, st)
        if st.what == "frozen_mask":
            assert nxt.entry in S.TAKES_MASK and st.value in script.mask_fns, (i, st)
    for w in S.walk(script):   # a change changes something
        if isinstance(w.step, S.Chg):
            assert w.before != w.settings, (w.i, w.step)


def _values(script, what):
    out = [S.DEFAULTS[what]]
    for w in S.walk(script):
        if isinstance(w.step, S.Chg) and w.step.what == what:
            out.append(w.settings[what])
    return out


@pytest.mark.parametrize("what", sorted(S.SETTERS) + ["frozen_mask", "select_kernel", "resident_blocks"])
def test_every_setting_goes_a_b_a(what):
    def aba(v):
        return any(v[i] == v[k] != v[j] for j in range(len(v)) for i in range(j) for k in range(j + 1, len(v)))
    seqs = [_values(s, what) for s in S.SCRIPTS]
    if what == "frozen_mask":   # the mask is per call: none, A, B, none is the sequence of the calls
        seqs = [[w.settings["frozen_mask"] for w in S.walk(s) if isinstance(w.step, S.Obs) and w.step.entry in S.TAKES_MASK]
                for s in S.SCRIPTS]
    assert any(aba(v) for v in seqs), seqs


def test_the_recipe_holds_what_the_context_holds():
    fin = [w for w in S.walk(S.BY_NAME["scf128"])][-1]
    assert S.recipe(fin.settings) == [S.Chg("scf_flips", 4)]          # T stays at the first dynamic budget
    fin = [w for w in S.walk(S.BY_NAME["cascl1024"])][-1]
    assert S.recipe(fin.settings) == []
    mid = [w for w in S.walk(S.BY_NAME["cascl1024"]) if isinstance(w.step, S.Obs)][7]
    assert S.recipe(mid.settings) == [S.Chg("sys_polar", True), S.Chg("stages", (1, 8))]
    for s in S.SCRIPTS:   # a consumed mask is gone
        last = [w for w in S.walk(s)][-1]
        assert "frozen_mask" not in [c.what for c in S.recipe(last.settings)]


def test_the_three_masks_of_scl1024_end_the_fill_phase_at_three_leaves():
    import fill_phase_codes as F
    import polardecoding_amd as pa
    s = S.BY_NAME["scl1024"]
    info = {k: [int(j) for j in np.flatnonzero(np.asarray(m) == 0)] for k, m in s.masks.items()}
    info["own"] = [int(j) for j in s.info_order()]
    ends = {k: F.rule(v) for k, v in info.items()}
    assert ends == {"A": 256, "B": 128, "own": 192}
    if os.path.exists(pa.lib_path()):   # the library's own answer
        lib = pa.load_library()
        lib.polar_fill_phase_end.restype = C.c_int
        lib.polar_fill_phase_end.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
        for k, v in info.items():
            io = np.asarray(v, dtype=np.int32)
            assert lib.polar_fill_phase_end(1024, io.ctypes.data_as(C.POINTER(C.c_int)), len(io)) == ends[k], k


def test_consecutive_observations_read_different_rows():
    for s in S.SCRIPTS:
        n = s.bmax()
        a, b = S.frame_index(s, 0, min(5, n)), S.frame_index(s, 1, min(5, n))
        assert not np.array_equal(a, b) and np.unique(S.rows(s).llr, axis=0).shape[0] == n


# ---- sensitivity -------------------------------------------------------------------------------------------------------------
def _pairs():
    """(script, index of the change, index of the observation after it) for every change that has a CPU model"""
    out = []
    for s in S.SCRIPTS:
        ws = list(S.walk(s))
        for k, w in enumerate(ws):
            if isinstance(w.step, S.Chg) and w.step.what not in S.NO_MODEL:
                out.append(pytest.param(s, k, id=f"{s.name}-{w.i}-{w.step.what}"))
    return out


def _differ(a, b):
    keys = [k for k in a if k in b]
    assert keys
    return [k for k in keys if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


@pytest.mark.parametrize("script,k", _pairs())
def test_the_observation_after_a_change_tells_the_two_states_apart(script, k, oracle):
    ws = list(S.walk(script))
    chg, ob = ws[k], ws[k + 1]
    x = S.inputs(script, ob.nobs, ob.step.B, ob.settings["sys_polar"])
    new = S.model(script, ob.settings, ob.step, x, oracle, cap=CAP)
    old = S.model(script, chg.before, ob.step, x, oracle, cap=CAP)
    assert new is not None and old is not None, "a change with a CPU model is observed through an entry that has none"
    assert _differ(old, new), f"{script.name}: step {chg.i} ({chg.step.what} -> {chg.step.value!r}) leaves every modelled output of the next call as it was"
