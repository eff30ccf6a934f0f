"""CPU: the pair kernel's LDS layout functions (csrc/fast2_lds.h) and the bank model that chose them
(tools/lds_bank_model.py).

  * The header compiles for the host, so its static_asserts -- rows 16-byte aligned and apart, a 32-lane group's own rows in
    banks of their own at every word and word window, rows by pointer no worse than 2-way -- are exercised without a GPU;
    a small program prints the offsets and they are the ones the model uses.
  * The model on a fixed seed: per access class the new row layout is never worse than the old one, conflict-free on the
    own rows (2 cycles for the two 32-lane groups) and within 2-way (4 cycles) on pointer rows, where the old one was 8-way.
  * The table layouts the model compares (48-byte cells, kept; three arrays, measured slower on the GPU) are printed; the
    only assertion on them is what the model is for: `arrays` has no more array cycles than `cells` in any class."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import lds_bank_model as M  # noqa: E402

PROG = r"""
#include <cstdio>
#include "fast2_lds.h"
int main()
{
    using namespace polar::fast2_lds;
    std::printf("%d %d %d %d %d\n", NW, SLOTS, ROW_STRIDE, CW_BASE, ROWS_WORDS);
    for (int c = 0; c < CWS; ++c)
        for (int s = 0; s < SLOTS; ++s) std::printf("%d ", cw_base(c) + row(s));
    std::printf("\n%d\n", pointer_rows_worst());
    return 0;
}
"""


def test_header_compiles_for_the_host_and_matches_the_model(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "layout.cpp"
    src.write_text(PROG)
    exe = tmp_path / "layout"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "polardecoding_amd", "csrc"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(v) for v in out[0].split()] == [M.NW, M.SLOTS, M.ROW_STRIDE, M.CW_BASE, M.CW_BASE + M.SLOTS * M.ROW_STRIDE]
    assert [int(v) for v in out[1].split()] == [M.ROWS["new"](c, s) for c in range(2) for s in range(M.SLOTS)]
    assert int(out[2]) == 2


def test_cycles_of_known_accesses():
    """the model's instruction table on accesses whose cycles are known by construction"""
    assert M.cycles("b32", [4 * l for l in range(64)]) == 2                       # consecutive words
    assert M.cycles("b32", [128 * l for l in range(64)]) == 64                    # one bank, 32 addresses per group
    assert M.cycles("b32", [128 * (l // 8) for l in range(64)]) == 8              # one bank, 4 addresses per group
    assert M.cycles("b32", [0] * 64) == 2                                         # broadcast
    assert M.cycles("b64", [8 * l for l in range(64)]) == 2
    assert M.cycles("b64", [256 * l for l in range(64)]) == 64
    assert M.cycles("b128", [16 * l for l in range(64)]) == 4
    assert M.cycles("b128", [48 * (l % 32) for l in range(64)]) == 4 * 1          # cells 0 .. 15 per 16-lane group: apart
    assert M.cycles("b128", [48 * 16 * (l % 2) for l in range(64)]) == 4 * 2      # cells 16 apart share their banks
    assert M.cycles("b32", [-1] * 63 + [0]) == 2


def test_new_row_layout_is_never_worse():
    res = M.rows_model(np.random.default_rng(20), 200)
    for cls, v in res.items():
        print(f"{cls:28s} old {v['old']:6.2f}   new {v['new']:6.2f}")
        assert v["new"] <= v["old"], cls
    assert res["own row, one word"] == {"old": 16.0, "new": 2.0}
    assert res["own row, window w0 + pos"] == {"old": 16.0, "new": 2.0}
    assert res["pointer row, one word"]["new"] <= 4.0 and res["pointer row, window"]["new"] <= 4.0


@pytest.mark.parametrize("dtype,es", [("f64", 8), ("f32", 4)])
def test_table_layouts_in_the_model(dtype, es):
    ops = M.sample_frames(16, 20, dtype)
    res = M.table_model(ops, np.random.default_rng(21), 200, es)
    for cls, v in res.items():
        print(f"{dtype} {cls:16s} cells {v[('cells', 0)]:6.2f}   arrays {v[('arrays', 0)]:6.2f}")
        assert v[("arrays", 0)] <= v[("cells", 0)], (dtype, cls)
