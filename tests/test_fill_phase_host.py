"""CPU: where the pair kernel's list-filling phase ends (polar_fill_phase_end, include/polar_hip.h) -- the library's answer
against the rule restated in tests/fill_phase_codes.py, on the codes tests/test_gpu_fast2_fill_phase.py decodes, so that the
GPU file provably has codes on both sides of every condition: the two BASELINE codes (192), a code that fills its list at
leaves 254 / 255 (256), and the near misses -- an information leaf at 189, four information leaves below 192, two of them in
front of the block at 192, the first information leaf at 63 (the 5G order for K = 768), every leaf information, and the 5G
order for K = 256."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_phase_codes as FP  # noqa: E402


def _lib():
    import polardecoding_amd as pa
    if not os.path.exists(pa.lib_path()):
        import __graft_entry__ as g
        g.build()
    lib = pa.load_library()
    lib.polar_fill_phase_end.restype = C.c_int
    lib.polar_fill_phase_end.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    return lib


def _end(lib, info, N=FP.N):
    io = np.ascontiguousarray(info, dtype=np.int32)
    return lib.polar_fill_phase_end(N, io.ctypes.data_as(C.POINTER(C.c_int)), len(io))


def test_the_information_leaves_the_cases_stand_on():
    c = FP.codes()
    low = {name: sorted(j for j in v[2] if j < 256) for name, v in c.items()}
    assert low["headline"][:4] == [127, 190, 191, 219]
    assert low["scl512"][:3] == [127, 191, 221]
    assert low["e256"] == [127, 254, 255] and low["one_path"] == [254, 255] and low["k256"] == low["k256_scl"] == [255]
    assert min(c["k768"][2]) == 63
    for name, v in c.items():
        assert len(set(v[2])) == len(v[2]), name
        assert len(v[2]) > (24 if v[1] else 0), name


@pytest.mark.parametrize("name", list(FP.codes()))
def test_the_library_and_the_rule_agree(name):
    _, _, info, want = FP.codes()[name]
    got = _end(_lib(), info)
    assert got == FP.rule(info), name
    assert got == want, name


def test_every_value_is_on_both_sides():
    ends = {name: FP.rule(v[2]) for name, v in FP.codes().items()}
    assert {0, 128, 192, 256} <= set(ends.values())


def test_every_5g_code_follows_the_rule():
    lib = _lib()
    q = FP.q5g()
    seen = set()
    for A in range(1, FP.N + 1):
        got = _end(lib, q[FP.N - A:])
        assert got == FP.rule(q[FP.N - A:]), A
        seen.add(got)
    assert 192 in seen and 0 in seen


def test_other_lengths_and_bad_arguments():
    lib = _lib()
    assert _end(lib, [127, 255, 511], N=512) == 0 and _end(lib, list(range(2048, 4096)), N=4096) == 0
    io = (C.c_int * 2)(5, 1024)
    assert lib.polar_fill_phase_end(1024, io, 2) < 0 and lib.polar_fill_phase_end(1000, io, 1) < 0
    assert lib.polar_fill_phase_end(1024, None, 1) < 0 and lib.polar_fill_phase_end(1024, io, 0) < 0
