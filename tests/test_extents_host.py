"""CPU: the helper of the output-extent tests (tests/extents.py) and its table against include/polar_hip.h.

The Arena must find a one-byte change in either guard of any output and name it, and stay silent when only the outputs were
written; every guard must be large enough for a whole phantom group of its case; every batch list must straddle a multiple
of its group width; and every `*_device` and host-buffer entry point of the header must be in the table or be named with the
test that already guards it, with the number of outputs and their nullable marks as the header declares them."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import extents as X  # noqa: E402

IDS = [c.name for c in X.CASES]


def _arena():
    a = X.Arena("numpy", capacity=X.Arena.need([("uint32", 96, 64, 4), ("float64", 3, 2, 1), ("int8", 130, 64, 64)]))
    views = [a.carve("bits", "uint32", 96, 64, 4), a.carve("pm", "float64", 3, 2, 1), a.carve("q", "int8", 130, 64, 64)]
    return a, views


def test_views_are_exact_naturally_aligned_and_never_16_byte_aligned():
    a, views = _arena()
    for v, (dt, n) in zip(views, (("uint32", 96), ("float64", 3), ("int8", 130))):
        isz = np.dtype(dt).itemsize
        assert v.dtype == np.dtype(dt) and v.shape == (n,)
        assert v.ctypes.data % 16 == isz % 16 and v.ctypes.data % isz == 0 and v.ctypes.data % 16 != 0
        assert (v.view(np.uint8) == X.FILL).all()
    for (_, front, start, end, back), g in zip(a.spans, (4096, 4096, 64 * 64)):
        assert start - front >= g and back - end >= g
    assert a.spans[0][4] <= a.spans[1][1] and a.spans[1][4] <= a.spans[2][1] and a.cursor <= a.capacity   # no guard is shared


def test_arena_is_silent_when_only_the_outputs_are_written():
    a, views = _arena()
    assert a.check() == []
    for v in views:
        v[...] = 0
    assert a.check() == []


@pytest.mark.parametrize("where", ["directly in front", "directly behind", "far end of the front guard", "far end of the back guard",
                                   "an unrelated guard"])
def test_arena_finds_one_planted_byte(where):
    a, views = _arena()
    for v in views:
        v[...] = 1
    _, front, start, end, back = a.span("pm")
    at, want = {"directly in front": (start - 1, ("pm", "front")), "directly behind": (end, ("pm", "behind")),
                "far end of the front guard": (front, ("pm", "front")), "far end of the back guard": (back - 1, ("pm", "behind")),
                "an unrelated guard": (a.span("q")[3] + 1000, ("q", "behind"))}[where]
    a.buf[at] ^= 0x01
    assert a.check() == [want + (at,)]
    a.buf[at] = X.FILL
    assert a.check() == []


def test_arena_reports_the_tail_and_refuses_to_overflow():
    a = X.Arena("numpy", capacity=3 * 4096)
    a.carve("x", "uint32", 8)
    a.buf[-1] = 0
    assert a.check() == [("", "tail", a.capacity - 1)]
    with pytest.raises(ValueError):
        a.carve("y", "uint32", 4096)


def test_snapshot_sees_one_changed_byte():
    x = np.arange(24, dtype=np.float64).reshape(3, 8)
    snap = X.snapshot(x)
    assert X.unchanged(x, snap)
    x.view(np.uint8)[2, 5] ^= 0x80
    assert not X.unchanged(x, snap)


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_every_guard_covers_a_whole_group(case):
    for B in case.batches:
        specs = [(o.dtype, X.elems(o, case.ctx, B), case.group, X.row_elems(o, case.ctx)) for o in case.outputs]
        a = X.Arena("numpy", capacity=X.Arena.need(specs))
        for o, (dt, n, g, r) in zip(case.outputs, specs):
            v = a.carve(o.name, dt, n, g, r)
            assert v.size == n
            _, front, start, end, back = a.span(o.name)
            need = max(4096, case.group * r * np.dtype(dt).itemsize)
            assert start - front >= need and back - end >= need, (case.name, o.name)
        assert a.cursor <= a.capacity


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_batches_lie_on_both_sides_of_a_group_boundary(case):
    bs, G = case.batches, case.group
    assert len(set(bs)) == len(bs) and min(bs) >= 1
    if len(bs) == 1:   # the one case that is there for a single size: one frame beyond a full block
        assert bs[0] == G + 1
        return
    assert any(b % G for b in bs), "no ragged batch"
    assert any(m * G - G < lo < m * G < hi for m in range(1, max(bs) // G + 2) for lo in bs for hi in bs), (case.name, bs, G)


def test_table_names_are_unique():
    assert len(set(IDS)) == len(IDS)


# ---- the header -----------------------------------------------------------------------------------------------------------------
def test_parser_reads_a_prototype_and_its_comment():
    text = """/* d_a (nullable) [B], d_b [B] (may be NULL); d_c and d_d are nullable. */
int polar_x_device(polar_ctx *ctx, const void *d_in, size_t B, uint32_t *d_a, uint32_t *d_b,
                   int32_t *d_c /* [3] */, int *d_d, const int *d_e, uint32_t *d_f);
/* no such word */
int polar_y_device(polar_ctx *ctx, size_t B, void *d_out, float *ms);"""
    p = X.prototypes(text)
    assert list(p) == ["polar_x_device", "polar_y_device"]
    assert X.device_outputs(p["polar_x_device"]) == ["d_a", "d_b", "d_c", "d_d", "d_f"]
    assert X.nullable_in_comment(p["polar_x_device"]) == ["d_a", "d_b", "d_c", "d_d"]
    assert X.device_outputs(p["polar_y_device"]) == ["d_out"] and X.nullable_in_comment(p["polar_y_device"]) == []


def test_every_device_entry_point_is_in_the_table_or_guarded_elsewhere():
    protos = X.prototypes()
    device = {n for n in protos if n.endswith("_device")}
    assert len(device) >= 20, sorted(device)
    covered = {c.entry for c in X.CASES}
    assert covered <= device, covered - device
    assert not (covered & set(X.ELSEWHERE))
    missing = device - covered - set(X.ELSEWHERE)
    assert not missing, f"entry points with no output-extent case: {sorted(missing)}"
    assert sorted(X.ELSEWHERE) == ["polar_generate_device", "polar_genie_rows_device"]
    for name, where in X.ELSEWHERE.items():
        path, test = where.split("::")
        with open(os.path.join(X.REPO, path)) as f:
            assert re.search(rf"^def {test}\(", f.read(), re.M), where


def test_every_host_buffer_entry_point_is_in_the_table():
    protos = X.prototypes()
    host = {n for n in protos if n.endswith("_batch") or n.endswith("_batch_y")} | {"polar_decode", "polar_decode_llr"}
    assert set(X.HOST_CASES) <= host and not (set(X.HOST_CASES) & set(X.HOST_ELSEWHERE))
    missing = host - set(X.HOST_CASES) - set(X.HOST_ELSEWHERE)
    assert not missing, f"host-buffer entry points with no output-extent case: {sorted(missing)}"
    assert all(dev in protos for dev in X.HOST_CASES.values())
    assert len(X.HOST_CASES) == 14


def test_every_host_buffer_entry_point_is_run_by_a_gpu_test():
    """a key of HOST_CASES is either a row of the GPU file's HOST table, which test_host_buffer_forms is parametrised over, or
    is named with a test of that file whose source calls it"""
    import inspect
    import test_gpu_extents as G   # imports no GPU package at module level
    assert not (set(G.HOST) & set(G.HOST_BY_HAND))
    assert set(G.HOST) | set(G.HOST_BY_HAND) == set(X.HOST_CASES)
    for entry, (name, _, spec) in G.HOST.items():
        assert G.BY_NAME[name].entry == X.HOST_CASES[entry], entry
        assert [o[3] for o in spec] == [o.name for o in G.BY_NAME[name].outputs], entry   # every device output has a host one
    for entry, test in G.HOST_BY_HAND.items():
        assert re.search(rf"\b{entry}\(", inspect.getsource(getattr(G, test))), (entry, test)


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_outputs_agree_with_the_header(case):
    proto = X.prototypes()[case.entry]
    names = X.device_outputs(proto)
    assert [o.name for o in case.outputs] == names, case.entry
    assert [o.name for o in case.outputs if o.nullable] == X.nullable_in_comment(proto), case.entry
