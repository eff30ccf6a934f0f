"""CPU: the order of the elements inside the pair kernel's level-7 / level-8 scratch rows (csrc/fast2_scratch.h).

  * The header compiles for the host, so its static_asserts -- sigma a bijection on a row, a lane's passes 2m / 2m + 1 one
    aligned pair, a path's four lanes on 8 consecutive elements, the + 8k strides passing through, rows starting at
    multiples of two elements -- are exercised without a GPU; a small program prints sigma and the row offsets.
  * `sigma` below restates the order in Python and is held to the header value by value; the bijection and the pair
    property are then checked on the printed values for both row lengths, every pos and every pair of passes."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (128, 256)

PROG = r"""
#include <cstdio>
#include "fast2_scratch.h"
int main()
{
    using namespace polar::fast2_scratch;
    std::printf("%d %d %d %d %d %d\n", ROW7, ROW8, SC_L8, SC_L7, SC_TL, SCRATCH_CW);
    for (unsigned e = 0; e < (unsigned)ROW8; ++e) std::printf("%u ", sigma(e));
    std::printf("\n");
    for (unsigned pos = 0; pos < 4; ++pos)
        for (unsigned m = 0; m < (unsigned)ROW8 / 8; ++m) std::printf("%u ", pair_at(pos, m));
    std::printf("\n");
    return 0;
}
"""


def sigma(e):
    """storage index of element e: inside a block of 8, the pass bit (4) goes below the two bits of pos"""
    return (e & ~7) | ((e & 3) << 1) | ((e >> 2) & 1)


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("scratch_order")
    src, exe = d / "order.cpp", d / "order"
    src.write_text(PROG)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "polardecoding_amd", "csrc"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    consts = [int(v) for v in out[0].split()]
    return consts, [int(v) for v in out[1].split()], [int(v) for v in out[2].split()]


def test_python_restatement_is_the_header(header):
    consts, sig, _ = header
    assert consts[:2] == list(ROWS)
    assert len(sig) == 256
    assert sig == [sigma(e) for e in range(256)]


@pytest.mark.parametrize("n", ROWS)
def test_bijection(header, n):
    sig = header[1][:n]
    assert sorted(sig) == list(range(n))   # a row's elements stay inside the row, each index taken once


@pytest.mark.parametrize("n", ROWS)
def test_pair_property(header, n):
    """lane pos, passes 2m and 2m + 1 (elements pos + 8m, pos + 8m + 4): adjacent, first index even, at pair_at(pos, m);
    the four lanes of a path together: the 8 elements of block m"""
    _, sig, pair = header
    for m in range(n // 8):
        block = []
        for pos in range(4):
            a, b = sig[pos + 8 * m], sig[pos + 8 * m + 4]
            assert b == a + 1 and a % 2 == 0, (n, pos, m)
            assert a == pair[pos * 32 + m] == 8 * m + 2 * pos, (n, pos, m)
            block += [a, b]
        assert sorted(block) == list(range(8 * m, 8 * m + 8)), (n, m)


@pytest.mark.parametrize("n", ROWS)
def test_strides_pass_through(header, n):
    """the readers' + 64k (level 8), + 64 (level 7) and + 32k (prefix, fill phase) strides are multiples of 8"""
    sig = header[1]
    for e in range(n):
        for stride in (32, 64, 128):
            if e + stride < n:
                assert sig[e + stride] == sig[e] + stride, (n, e, stride)


def test_rows_start_at_pairs(header):
    consts = header[0]
    row7, row8, sc_l8, sc_l7, sc_tl, scratch_cw = consts
    for v in (row7, row8, sc_l8, sc_l7, scratch_cw):
        assert v % 2 == 0
    # the rows of the two levels and the top-left level do not overlap
    assert sc_l7 >= sc_l8 + 8 * row8 and sc_tl >= sc_l7 + 8 * row7 and scratch_cw == sc_tl + 512
