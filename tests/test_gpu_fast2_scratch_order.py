"""GPU: the pair kernel (k_scl_fast2 / k_scl_fast2_y, csrc/scl_fast2.h) where the order of its level-7 / level-8 scratch
rows (csrc/fast2_scratch.h) decides what it reads.  Every writer of such a row (from_top's left, right and g steps, from_l8,
the frozen prefix, the fill phase's first block) and every reader (from_l8, from_l7, both fill blocks) must agree on where
an element lies, also when a row is read through another slot's pointer after a fork.

N is fixed at 1024 for this kernel, so the small dimension is the batch: 1 frame (the second codeword of the wavefront
idle), 2, 3 (a lone codeword in the last pair) and 33 frames at 0.75 dB, where most information leaves rank and paths fork.
Information sets with E = 0, 128, 192 and 256 (tests/fill_phase_codes.py) take the frame through every step: E = 0 starts
with the frozen prefix's registers and the octet heads, E = 128 enters from_l8 behind the prefix, E = 192 runs the fill
phase's level-8 block and E = 256 its level-7 block as well.  Four forms: f64 with CRC-24C, f64 without CRC, f32 (against
the f32 oracle; its rows are in element order, read and written by the same code through sg() / sg2()) and the y form
(sigma > 0).  Decisions, path metrics and flags are compared with == against the oracle for
every frame; the smaller batches are the first frames of the 33, so the oracle decodes each set once per form.

One more case decodes the 33 frames, then the same frames in reverse order, then the first order again in one context:
the first and the third output are identical (nothing stale in the rows between frames or launches)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_phase_codes as FP  # noqa: E402
from test_gpu_fast2_lds_layout import VARIANTS, _code, _np, _reference  # noqa: E402

pytestmark = pytest.mark.gpu

N, L, NROWS = 1024, 8, 33
BATCHES = (1, 2, 3, 33)
SETS = {"k768": 0, "pair_126_127": 128, "headline": 192, "e256": 256}   # name in fill_phase_codes -> E
_cache = {}


def _frames(oracle, name):
    """33 frames at 0.75 dB on the set's information leaves: (y, sigma, llr), read-only"""
    if name not in _cache:
        info = FP.codes()[name][2]
        assert FP.rule(info) == SETS[name], name
        sig = oracle.sigma_from_db(0.75)
        _, ys = oracle.Sim(2150 + SETS[name]).frames(_code(oracle, info, False), sig, NROWS)
        y = np.stack(ys)
        llr = np.stack([oracle.llr_from_y(r, sig) for r in ys])
        y.setflags(write=False)
        llr.setflags(write=False)
        _cache[name] = (y, sig, llr)
    return _cache[name]


def _case(oracle, name, variant):
    """(code, algo, dtype, rows for the device, sigma for the device, the oracle's (u_hat, pm, flags)) of a set and form"""
    if (name, variant) not in _cache:
        algo, crc, dtype, from_y = VARIANTS[variant]
        y, sig, llr = _frames(oracle, name)
        llr = llr.astype(_np(dtype))
        code = _code(oracle, FP.codes()[name][2], crc)
        ref = _reference(oracle, code, llr, algo, dtype)
        for r in ref:
            r.setflags(write=False)
        _cache[(name, variant)] = (code, algo, dtype, (y if from_y else llr), (sig if from_y else 0.0), ref)
    return _cache[(name, variant)]


def _decoder(code, algo, dtype, E):
    import polardecoding_amd as pa
    dec = pa.Decoder(N, code.K, pa.ALGO_CASCL if algo == "CASCL" else pa.ALGO_SCL, L=L, crc_taps=code.taps if algo == "CASCL" else None,
                     info_order=code.info_order, dtype=pa.F64 if dtype == "f64" else pa.F32)
    lib = pa.load_library()
    lib.polar_fill_phase_end.restype = C.c_int
    lib.polar_fill_phase_end.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    io = np.ascontiguousarray(dec.info_order, dtype=np.int32)
    assert lib.polar_fill_phase_end(N, io.ctypes.data_as(C.POINTER(C.c_int)), len(io)) == E
    return dec


def _decode(dec, rows, sigma):
    """one launch of the pair kernel: (u_hat, pm, flags) on the host; the outputs start out as -1"""
    import torch
    from conftest import unpack_bits
    x = torch.from_numpy(np.array(rows)).cuda()
    B = x.shape[0]
    bits = torch.full((B, N // 32), -1, dtype=torch.int32, device="cuda")
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_device(x, sigma=sigma, out_bits=bits, pm=pm, flags=fl)
    dec.synchronize()
    assert dec.kernel_name.startswith("k_scl_fast2<"), dec.kernel_name   # the name of both forms (k_fast2.hip)
    return unpack_bits(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


def _assert_equal(got, ref, what):
    uh, pm, fl = got
    o_uh, o_pm, o_fl = ref
    bad = np.nonzero((uh != o_uh).any(axis=1))[0]
    assert bad.size == 0, f"{what}: decisions differ from the oracle's in frames {bad[:8]}"
    assert np.array_equal(pm.astype(o_pm.dtype), o_pm), f"{what}: path metrics differ in frames {np.nonzero(pm.astype(o_pm.dtype) != o_pm)[0][:8]}"
    assert np.array_equal(fl, o_fl), f"{what}: flags {fl[fl != o_fl][:8]} for {o_fl[fl != o_fl][:8]}"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SETS))
def test_scratch_rows_at_small_batches(name, variant, oracle):
    code, algo, dtype, rows, sigma, ref = _case(oracle, name, variant)
    dec = _decoder(code, algo, dtype, SETS[name])
    try:
        for B in BATCHES:
            got = _decode(dec, rows[:B], sigma)
            _assert_equal(got, tuple(r[:B] for r in ref), f"{name}, {variant}, B = {B}")
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["headline", "e256"])
def test_nothing_stale_between_launches(name, oracle):
    code, algo, dtype, rows, sigma, ref = _case(oracle, name, "f64_crc")
    dec = _decoder(code, algo, dtype, SETS[name])
    try:
        first = _decode(dec, rows, sigma)
        other = _decode(dec, rows[::-1], sigma)    # other frames in every wavefront's rows
        again = _decode(dec, rows, sigma)
    finally:
        dec.close()
    _assert_equal(first, ref, f"{name}: first launch")
    _assert_equal(other, tuple(r[::-1] for r in ref), f"{name}: reversed frames")
    for a, b, what in zip(first, again, ("decisions", "path metrics", "flags")):
        assert np.array_equal(a, b), f"{name}: {what} of the same frames differ between two launches of one context"


def test_the_sets_cover_every_end():
    assert set(SETS.values()) == {0, 128, 192, 256}
