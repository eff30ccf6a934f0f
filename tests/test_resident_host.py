"""CPU: the table of tests/resident_cases.py checked with the references alone, so that tests/test_gpu_resident.py cannot pass
vacuously: every row's largest batch makes three rounds and a ragged last job at either cap; the frames that only a later job
decodes (index >= S u) differ among themselves, hold frames that do not decode to the sent word and, per kind, frames with a
positive path metric, frames that need an attempt beyond the first, or differing iteration counts; and every planted
degenerate row is decoded by a later job of its wavefront at one cap at least.  Seeds and Eb/N0 points of the table were
picked here until the references met these conditions; the conditions are fixed.  Also: the hook is declared."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import resident_cases as RC  # noqa: E402

IDS = [r.name for r in RC.ROWS]


def test_names_are_unique_and_shapes_are_the_issue_s():
    assert len(set(IDS)) == len(IDS)
    for row in RC.ROWS:
        assert row.u in RC.RAGGED and row.jpb >= 1
        assert RC.batches(row, 1) == (row.jpb * row.u, row.jpb * row.u + 1, 3 * row.jpb * row.u + row.u + RC.RAGGED[row.u])


@pytest.mark.parametrize("row", RC.ROWS, ids=IDS)
def test_largest_batch_makes_three_rounds_and_a_ragged_job(row):
    for cap in RC.CAPS:
        S = RC.slots(row, cap)
        B0, B1, B2 = RC.batches(row, cap)
        assert RC.jobs(row, B0) == S and B0 % row.u == 0                       # the control: one job per slot
        assert RC.jobs(row, B1) == S + 1 and (row.u == 1 or B1 % row.u == 1)   # one queued job, ragged
        assert RC.jobs(row, B2) >= 3 * S + 1
        assert row.u == 1 or B2 % row.u != 0
    assert RC.pool_size(row) == RC.batches(row, RC.CAPS[-1])[2]


@pytest.mark.parametrize("row", RC.ROWS, ids=IDS)
def test_queued_part_of_every_largest_batch_is_not_trivial(row, oracle):
    want, sent = RC.want(oracle, row), RC.sent(oracle, row)
    assert all(len(w) == RC.pool_size(row) for w in want)
    degenerate = [p for pos in RC.planted(oracle, row).values() for p in pos] if row.spec.get("plant", True) else []
    for cap in RC.CAPS:
        lo, hi = RC.slots(row, cap) * row.u, RC.batches(row, cap)[2]
        q = [np.asarray(w)[lo:hi] for w in want]
        assert any((a.reshape(len(a), -1) != a.reshape(len(a), -1)[0]).any() for a in q), "the model's outputs are all equal"
        best = q[0] if q[0].ndim == 2 else q[0][:, 0]   # list output: the path of rank 0
        wrong = (best != sent[lo:hi]).any(axis=1)
        wrong[[p - lo for p in degenerate if lo <= p < hi]] = False   # a planted row carries no word: it does not count
        assert wrong.any(), "every queued frame decodes to the sent word"
        assert not wrong.all()
        if row.kind in ("list", "q8", "fam", "listout"):
            assert (np.isfinite(q[1]) & (q[1] > 0)).any(), "no positive path metric"
        if row.kind in ("scf", "dscf"):
            assert (q[2] > 1).any() if row.kind == "dscf" else (q[2] >= 1).any(), "no attempt beyond the first"
            assert (q[1] & RC.FLAG_CRC_PASS != 0).any() and (q[1] & RC.FLAG_CRC_PASS == 0).any()
        if row.kind == "bpstop":
            assert np.unique(q[1]).size > 1, "constant iteration counts"


@pytest.mark.parametrize("row", [r for r in RC.ROWS if r.spec.get("plant", True)], ids=lambda r: r.name)
def test_every_planted_row_meets_a_later_job(row, oracle):
    where = RC.planted(oracle, row)
    assert where, "nothing planted"
    names = [n for n, _ in RC.degenerate(row.N, np.float64, 0)]
    assert list(where)[:min(3, len(where))] == names[:min(3, len(where))]   # zero, 2^20, subnormal come first
    for name, pos in where.items():
        ok = any(RC.slots(row, cap) * row.u <= p < RC.batches(row, cap)[2] for p in pos for cap in RC.CAPS)
        assert ok, (name, pos)
    if RC.pool_size(row) >= 60:
        assert {"zero+", "2^20", "subnormal"} <= set(where)


def test_hook_is_declared():
    text = open(os.path.join(REPO, "include", "polar_hip_testing.h")).read()
    assert re.search(r"int polar_testing_resident_blocks\(polar_ctx \*ctx, int blocks\);", text)
    assert re.search(r"int polar_testing_last_plan\(const polar_ctx \*ctx, int \*grid, long long \*jobs, int \*jobs_per_block, "
                     r"int \*queued\);", text)
    assert re.search(r"int polar_testing_last_stride\(const polar_ctx \*ctx, int \*grid, long long \*need\);", text)
