"""CPU: the helper of the load-stage tests (tests/input_forms.py) against include/polar_hip.h and the dispatchers.

Completeness: every entry point of the header with a `const void *d_in, int in_is_f32` pair is a case or is named in EXEMPT.
Dispatch: DISPATCH is checked by a grep of the instantiation lines the dispatcher units spell out (launch_*<double, float>
and the like): a cell runs a pair its unit spells, and every pair a unit spells is reached by a cell.  The tuned L = 8
launchers (k_fast.hip, k_fast2.hip, k_fast4.hip) return POLAR_ENOKERNEL for an f64 context on float rows, but fast_ok() in
polar_hip.hip sends those rows to k_scl_big (N = 1024) or k_scl_generic (N = 128) first, the forced test variants included:
the refusals are not reachable through the C ABI, and no cell of DISPATCH is None.

What the references can tell apart.  For every case whose reference is the oracle's list decoder, the path metrics on
form_rows() differ, in some frame of the batch, from those on rows formed by each of three wrong rules: 2*y/(sigma*sigma),
the product formed in float, LLRs rounded to float before an f64 context.  BP returns bits (and round trips) only: its cells
catch gross errors -- a wrong element, a wrong width, a missing sigma -- and not single roundings; the y form is asserted
against a rule that omits sigma, so that at least this much is shown."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import input_forms as IF  # noqa: E402

IDS = [c.name for c in IF.CASES]
LIST_CASES = [c for c in IF.CASES if c.ref in IF.LIST_REFS and c.entry == "polar_decode_device"]
BP_CASES = [c for c in IF.CASES if c.ref in ("bp", "bpl", "readout")]


# ---- completeness -------------------------------------------------------------------------------------------------------------
def _row_entry_points(text=None):
    """the functions of the header that take `const void *d_in, int in_is_f32`"""
    out = []
    for name, p in IF.EX.prototypes(text).items():
        decls = [d for d, _ in p.params]
        if "const void *d_in" in decls and "int in_is_f32" in decls:
            out.append(name)
    return out


def _uncovered(text=None):
    have = {c.entry for c in IF.CASES} | set(IF.EXEMPT)
    return [n for n in _row_entry_points(text) if n not in have]


def test_every_row_entry_point_is_a_case_or_exempt():
    names = _row_entry_points()
    assert len(names) >= 15 and "polar_decode_device" in names and "polar_list_decode" in names
    assert _uncovered() == []
    for c in IF.CASES:
        assert c.entry in names, c.name
    assert set(IF.EXEMPT) <= {"polar_rm_recover_device", "polar_q8_quantize_device", "polar_codebook_decode",
                              "polar_codebook_list_decode"}
    for name, where in IF.EXEMPT.items():
        assert name in names and os.path.exists(os.path.join(IF.REPO, where)), name
        with open(os.path.join(IF.REPO, where)) as f:
            assert re.search(r"data_ptr\(\) %|misaligned", f.read()), where   # that file does place rows off a 16-byte boundary


def test_a_new_row_entry_point_without_a_case_is_found():
    with open(IF.EX.HEADER) as f:
        text = f.read()
    new = ("int polar_new_decode_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B,\n"
           "                            uint32_t *d_uhat_bits);\n")
    at = text.index("int polar_count_errors_device")
    assert _uncovered(text[:at] + new + text[at:]) == ["polar_new_decode_device"]


def test_header_states_the_rule_once_and_the_entry_points_refer_to_it():
    protos = IF.EX.prototypes()
    main = " ".join(protos["polar_decode_device"].comment.split())
    for phrase in ("Input rows", "2 * v / sigma / sigma", "alignment of its element type", "k_scl_big", "k_scl_generic"):
        assert phrase in main, phrase
    for name in _row_entry_points():
        if name not in ("polar_decode_device", "polar_codebook_decode", "polar_codebook_list_decode"):
            assert "Input rows" in protos[name].comment, name


# ---- the dispatch table -------------------------------------------------------------------------------------------------------
def _units():
    return sorted(f for f in os.listdir(IF.CSRC) if re.fullmatch(r"k_\w+\.hip", f))


def _pairs_of(family):
    """the (R, IN) pairs the dispatcher of a kernel family spells out"""
    units, launcher = IF.FAMILY_SRC[family]
    pairs = set()
    for u in units:
        with open(os.path.join(IF.CSRC, u)) as f:
            assert launcher in f.read(), (family, u)
        src = "k_scl_launch.h" if launcher == "launch_scl_types" else u
        want = "launch_scl_l" if launcher == "launch_scl_types" else launcher
        pairs |= {(R, IN) for name, R, IN in IF.spelled(src) if name == want}
    return pairs


def test_every_cell_runs_a_pair_its_dispatcher_spells_out():
    assert set(IF.DISPATCH) == set(IDS)
    for c in IF.CASES:
        assert set(IF.DISPATCH[c.name]) == set(IF.PAIRS), c.name
        for pair, cell in IF.DISPATCH[c.name].items():
            for fam in IF.families_of(cell):
                assert pair in _pairs_of(fam), (c.name, pair, fam)


def test_every_spelled_instantiation_is_reached_by_a_cell():
    reached = {(IF.FAMILY_SRC[fam][1], pair) for c in IF.CASES for pair, cell in IF.DISPATCH[c.name].items()
               for fam in IF.families_of(cell)}
    known = {launcher for _, launcher in IF.FAMILY_SRC.values()}
    seen = 0
    for u in _units() + ["k_scl_launch.h"]:
        if u in IF.EXEMPT_UNITS:
            continue
        for name, R, IN in IF.spelled(u):
            if name == "launch_scl_l":
                name = "launch_scl_types"
            assert name in known, f"{u} spells out {name}<{R}, {IN}>: add its kernel family to tests/input_forms.py"
            assert (name, (R, IN)) in reached, f"{u}: {name}<{R}, {IN}> is reached by no cell of DISPATCH"
            seen += 1
    assert seen >= 4 * 12
    # a made-up pair of a made-up dispatcher would be found
    assert ("launch_new_kernel", ("f64", "f32")) not in reached


def test_an_f64_context_on_float_rows_leaves_the_tuned_l8_kernels():
    """fast_ok() refuses the pair before a tuned launcher sees it, so the POLAR_ENOKERNEL lines of those launchers are not
    reachable and the cells run k_scl_big (N = 1024) or k_scl_generic (N = 128)"""
    with open(os.path.join(IF.CSRC, "polar_hip.hip")) as f:
        text = f.read()
    body = text[text.index("bool fast_ok("):text.index("enum class Family")]
    assert "if (g.dtype == POLAR_F64 && in_is_f32) return false;" in body
    family = text[text.index("Family kernel_family("):text.index("int q8_decode_rows(")]
    assert family.index("if (fast_ok(c, in_is_f32)) {") < family.index("Family::FAST4") < family.index("return Family::BIG")
    for unit, launcher in (("k_fast.hip", "launch_fast_n"), ("k_fast2.hip", "launch_fast2"), ("k_fast4.hip", "launch_fast4")):
        assert (launcher, "f64", "f32") not in IF.spelled(unit)
        with open(os.path.join(IF.CSRC, unit)) as f:
            assert "POLAR_ENOKERNEL" in f.read()
    tuned = [c for c in IF.CASES if any(f in ("k_scl_fast", "k_scl_fast2", "k_scl_fast4") for f in IF.families_of(c.family[("f64", "f64")]))]
    assert len(tuned) >= 6
    for c in tuned:
        want = "k_scl_big" if c.ctx["N"] == 1024 else "k_scl_generic"
        assert want in IF.families_of(IF.DISPATCH[c.name][("f64", "f32")]), c.name
    assert not [c.name for c in IF.CASES if None in IF.DISPATCH[c.name].values()]


# ---- the forms and the rule ---------------------------------------------------------------------------------------------------
def test_forms_are_the_product_of_the_four_axes():
    assert len(IF.FORMS) == len(set(IF.FORMS)) == 2 * 2 * (2 + 3)
    assert {f.shift for f in IF.FORMS if f.IN == "f64"} == {0, 1} and {f.shift for f in IF.FORMS if f.IN == "f32"} == {0, 1, 2}
    assert {f.sigma for f in IF.FORMS} == {0.0, IF.SIGMA} and IF.SIGMA == 10 ** (-1.5 / 20)
    m, e = np.frexp(IF.SIGMA)
    assert m != 0.5   # not a power of two


@pytest.mark.parametrize("case", IF.CASES, ids=IDS)
def test_base_rows_are_exact_in_float_so_two_references_serve_a_context(case):
    x = IF.base_rows(case)
    assert x.shape == (case.B, case.ctx["N"]) and x.dtype == np.float64 and np.isfinite(x).all()
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    for R in ("f64", "f32"):
        for sigma in (0.0, IF.SIGMA):
            a, b = IF.form_rows(x, "f64", sigma, R), IF.form_rows(x, "f32", sigma, R)
            assert a.dtype == IF.NP[R] and a.tobytes() == b.tobytes()
    assert case.B % 2 == 1 and (case.B >= 67 if "lanes" in str(case.family[("f64", "f64")]) else True)


def test_form_rows_is_the_rule_and_differs_from_its_neighbours():
    x = IF.base_rows(IF.CASES[0])
    s = IF.SIGMA
    y = IF.form_rows(x, "f32", s, "f64")
    assert np.array_equal(y, 2 * x / s / s)
    assert np.array_equal(IF.form_rows(x, "f64", 0.0, "f32"), x.astype(np.float32))
    for which in IF.WRONG_RULES:
        w = IF.wrong_rows(x, s, which)
        assert w.dtype == np.float64 and (w != y).mean() > 0.05, which
        assert np.allclose(w, y, rtol=1e-6, atol=0)
    # with a power of two the three agree with the rule: the generic sigma is what tells them apart
    for which in ("assoc", "float product"):
        assert np.array_equal(IF.wrong_rows(x, 0.5, which), IF.form_rows(x, "f32", 0.5, "f64")), which


@pytest.mark.parametrize("case", LIST_CASES, ids=[c.name for c in LIST_CASES])
def test_the_oracles_path_metrics_tell_the_rules_apart(case, oracle):
    x = IF.base_rows(case)
    right = IF.reference(case, "f64", IF.form_rows(x, "f32", IF.SIGMA, "f64"), oracle)
    for which in IF.WRONG_RULES:
        wrong = IF.reference(case, "f64", IF.wrong_rows(x, IF.SIGMA, which), oracle)
        assert (wrong["pm"] != right["pm"]).any(), (case.name, which)
    # and the two forms of one batch are two different problems
    llr = IF.reference(case, "f64", IF.form_rows(x, "f64", 0.0, "f64"), oracle)
    assert (llr["pm"] != right["pm"]).all()


@pytest.mark.parametrize("case", BP_CASES, ids=[c.name for c in BP_CASES])
def test_bp_cells_see_a_missing_sigma(case, oracle):
    x = IF.base_rows(case)
    right = IF.reference(case, "f64", IF.form_rows(x, "f64", IF.SIGMA, "f64"), oracle)
    wrong = IF.reference(case, "f64", IF.wrong_rows(x, IF.SIGMA, "no sigma"), oracle)
    assert any((np.asarray(right[k]) != np.asarray(wrong[k])).any() for k in right), case.name


# ---- the typed restatements of BP with the stop rule and of BP list decoding ----------------------------------------------------
def test_typed_bp_is_the_oracles_bp_in_both_types(oracle):
    case = next(c for c in IF.CASES if c.name == "k_bp N=256 stop g")
    code = IF.oracle_code(case, oracle)
    x = IF.base_rows(case)
    for R in ("f64", "f32"):
        rows = IF.form_rows(x, "f32", IF.SIGMA, R)
        for t, (u_hat, _) in enumerate(IF.typed_bp_rounds(oracle, rows, code.frozen, 4, IF.NP[R]), start=1):
            ref, _, _ = oracle.decode(code, rows, "BP", bp_iters=t, dtype=R)
            assert np.array_equal(u_hat, ref), (R, t)


@pytest.mark.parametrize("name", ["k_bp_w128 N=128 stop g", "bpl P=2 N=128", "bpl reversal first N=128 chunked"])
def test_typed_stop_rule_and_list_are_the_f64_models(name, oracle):
    case = next(c for c in IF.CASES if c.name == name)
    io, _, taps, fz = IF.code_of(case)
    x = IF.base_rows(case)
    for sigma in (0.0, IF.SIGMA):
        rows = IF.form_rows(x, "f64", sigma, "f64")
        if case.ref == "bp":
            want = IF.stop_points(rows, fz, 12)
            got = IF.typed_stop_points(oracle, rows, fz, 12, np.float64)
            assert want[1].any() and not want[1].all()
        else:
            it = case.ctx["kw"]["iterMax"]
            res = IF.BM.bpl_decode(rows, fz, io, IF.bpl_graphs(case), it, taps)
            want = (res.bits, res.iters, res.flags, res.graph, res.total)
            got = IF.typed_bpl(oracle, rows, fz, io, IF.bpl_graphs(case), it, taps, np.float64)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (name, sigma)


# ---- what the chunked cases are there for ---------------------------------------------------------------------------------------
def test_chunked_cases_cross_a_pass_boundary(oracle):
    floor = 64   # chunk_rows(): the row loops never take fewer rows per pass
    for case in (c for c in IF.CASES if "cap" in c.opts):
        x = IF.base_rows(case)
        for R in ("f64", "f32"):
            for sigma in (0.0, IF.SIGMA):
                ref = IF.reference(case, R, IF.form_rows(x, "f32", sigma, R), oracle)
                if case.ref == "adaptive":   # stage 1 takes the frames that fail SC: more than one pass of 64
                    assert (ref["list"] > 1).sum() > floor, (case.name, R, sigma, int((ref["list"] > 1).sum()))
                    assert {1, 2, 8} == set(np.unique(ref["list"]).tolist())
                elif case.ref == "scf":      # a cap of one byte: every failing frame is a pass
                    assert (ref["attempts"] > 0).sum() >= 8 and (ref["sets"][:, 0] >= 0).sum() >= 2, (case.name, R, sigma)
                else:                        # attempt 0 is staged: the whole batch in passes of 64
                    assert case.B > floor and IF.bpl_graphs(case)[0] != list(range(7))
                    assert (ref["graph"] == 0).any() and (ref["graph"] > 0).any(), (case.name, R, sigma)


# ---- place() ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_place_starts_at_the_stated_residue_inside_a_nan_frame(dtype):
    x = np.arange(3 * 32, dtype=dtype).reshape(3, 32) - 7
    for shift in (0, 1, 2):
        p = IF.place(x, shift)
        isz = np.dtype(dtype).itemsize
        assert IF.address(p.whole) % 16 == 0 and IF.address(p.rows) % 16 == (shift * isz) % 16
        assert p.rows.shape == x.shape and p.rows.dtype == x.dtype and p.rows.flags["C_CONTIGUOUS"] and np.array_equal(p.rows, x)
        assert np.shares_memory(p.rows, p.whole) and len(p.whole) - shift - x.size >= 64
        assert IF.frame_intact(p, x)
        p.whole[shift + x.size] = 0          # one element behind the last row
        assert not IF.frame_intact(p, x)
        p.whole[shift + x.size] = np.nan
        if shift:
            p.whole[shift - 1] = 1
            assert not IF.frame_intact(p, x)
            p.whole[shift - 1] = np.nan
        p.rows[1, 5] += 1                    # a changed row
        assert not IF.frame_intact(p, x)
    assert (2 * np.dtype(np.float32).itemsize) % 16 == 8   # shift 2 of float rows: 8-byte aligned, not 16
