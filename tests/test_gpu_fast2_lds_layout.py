"""GPU: the pair kernel (k_scl_fast2 / k_scl_fast2_y, csrc/scl_fast2.h) where its LDS layout decides what it reads: the
staircase table's cells and the partial-sum rows (csrc/fast2_lds.h).  Every case compares decisions, path metric and flags
with == against the oracle, N = 1024, L = 8, in four variants: f64 with CRC-24C, f64 without CRC, f32 (against the f32
oracle) and the y form (sigma > 0).

Table: 16 rows on the code in which every leaf is an information leaf (no frozen run, no list-filling phase: octet 0 goes
through the narrow chains of octet()).  A check node reads the table at |a + b| and |a - b|.
  * Rows 0 and 1 are a frame at 1 dB whose first pairs (e, e + 512) -- the operands of the root step, a wide step -- are
    replaced by pairs built for the cells.
  * Rows 2 .. 15 hold the built pairs at elements (i, i + 4), i < 4, and +64 .. +128 everywhere else.  CHK(v, big) is v
    itself (both table values are T = 0 and the minimum is |v|), so the six wide steps above octet 0 hand elements 0 .. 7
    down unchanged and the level-2 check node of octet 0 -- the head of a narrow chain -- reads the table at the built
    operands.  `_level3` restates the tree in numpy and the test asserts that the hand-down is exact.
  The built pairs: (t, +0) reads the table at t twice; ((s + d) / 2, (s - d) / 2) reads it at s and d, exact for the cell
  centres (five mantissa bits) and for s, d = thr -+ 1 ulp.  Both sets of operands are asserted to hold every one of the 50
  cells, both clamps (below 0.125, at and above 8), zero (the wide steps: +0 and -0; a check node's own result is never -0,
  so a narrow chain meets -0 only behind a g step) and each of the seven thresholds at -1 ulp, exact and +1 ulp.

Rows: 33 frames at 0.75 dB -- most information leaves rank, paths fork, pointer rows are shared; the odd count leaves a
lone codeword in the last pair -- on the information sets of the headline code (K + r = 536, E = 192), of SCL K = 512
(E = 192) and of tests/fill_phase_codes.py with E = 0, 128 and 256: the list-filling phase writes the partial-sum rows.

The oracle decodes each set of rows once per variant (about 2 ms a frame)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_phase_codes as FP  # noqa: E402

pytestmark = pytest.mark.gpu

N, L, NROWS = 1024, 8, 33
THR = (0.196, 0.433, 0.71, 1.05, 1.508, 2.252, 4.5)
TV = (0.65, 0.55, 0.45, 0.35, 0.25, 0.15, 0.05, 0.0)
#            algo     CRC    dtype  y form
VARIANTS = {
    "f64_crc": ("CASCL", True, "f64", False),
    "f64_nocrc": ("SCL", False, "f64", False),
    "f32": ("CASCL", True, "f32", False),
    "y": ("SCL", False, "f64", True),
}
# information sets of the rows cases: name in fill_phase_codes (its algo and taps are not used here), expected E
SETS = {"headline": 192, "scl512": 192, "k768": 0, "pair_126_127": 128, "e256": 256}
_cache = {}


def _np(dtype):
    return np.float64 if dtype == "f64" else np.float32


def cell_of(x):
    """the table cell of |x| (csrc/polar_lut.h Cell<R>::raw, Lut<R>::index_of): 0 below 0.125, 1 .. 48, 49 from 8 up"""
    x = np.asarray(x)
    if x.dtype == np.float64:
        raw = ((x.view(np.uint64) >> np.uint64(32 + 17)) & np.uint64(0x3FFF)).astype(np.int64)
        bias = 0x3FC00000 >> 17
    else:
        raw = ((x.view(np.uint32) >> np.uint32(20)) & np.uint32(0x7FF)).astype(np.int64)
        bias = 0x3E000000 >> 20
    return np.clip(raw, bias - 1, bias + 48) - (bias - 1)


def built_pairs(dt):
    """(a, b) pairs whose a + b and a - b are exact and, together, hold every cell, zero and threshold neighbour"""
    centre = [dt(0.0625)] + [dt(2.0 ** ((k - 1) // 8 - 3) * (1 + ((k - 1) % 8 + 0.5) / 8)) for k in range(1, 49)] + [dt(12)]
    assert cell_of(np.array(centre, dtype=dt)).tolist() == list(range(50))
    pairs = [(dt(0), dt(0)), (dt(-0.0), dt(0)), (dt(0), dt(-0.0)), (dt(-0.0), dt(-0.0))]
    for t in THR:
        t = dt(t)
        lo, hi = np.nextafter(t, dt(0)), np.nextafter(t, dt(16))
        pairs += [(t, dt(0)), ((lo + hi) / dt(2), (lo - hi) / dt(2)), (-(lo + hi) / dt(2), (lo - hi) / dt(2))]
    for k in range(0, 50, 2):
        s, d = centre[k], centre[k + 1]
        pairs += [((s + d) / dt(2), (s - d) / dt(2))]
    pairs += [(dt(8), dt(0)), (np.nextafter(dt(8), dt(0)), dt(-0.0)), (dt(0.125), dt(0))]   # the edges of the two clamps
    return pairs


def assert_covers(a, b, what, minus_zero=True):
    """the operands |a + b|, |a - b| hold all 50 cells, both zeros and every threshold at -1 ulp, exact, +1 ulp"""
    dt = a.dtype.type
    ops = np.concatenate([a + b, a - b])
    assert sorted(set(cell_of(ops).tolist())) == list(range(50)), what
    assert (ops == 0).any() and not np.signbit(ops[ops == 0]).all(), what
    assert np.signbit(ops[ops == 0]).any() or not minus_zero, what
    mag = set(np.abs(ops).tolist())
    for t in THR:
        t = dt(t)
        assert {float(np.nextafter(t, dt(0))), float(t), float(np.nextafter(t, dt(16)))} <= mag, (what, t)
    assert float(dt(8)) in mag and float(np.nextafter(dt(8), dt(0))) in mag and float(dt(0.125)) in mag, what


def _chk(a, b):
    """CHK as the decoders compute it: sign * min + (T(|a + b|) - T(|a - b|)), each operation rounded once"""
    dt = a.dtype.type
    thr, tv = np.array(THR, dtype=dt), np.array(TV, dtype=dt)
    T = lambda x: tv[np.searchsorted(thr, np.abs(x), side="right")]  # noqa: E731
    sign = np.where(np.signbit(a) ^ np.signbit(b), dt(-1), dt(1))
    return sign * np.minimum(np.abs(a), np.abs(b)) + (T(a + b) - T(a - b))


def _level3(rows):
    """elements 0 .. 7 of the level-3 node above octet 0: six check-node steps below the root step"""
    x = rows
    while x.shape[1] > 8:
        h = x.shape[1] // 2
        x = _chk(x[:, :h], x[:, h:])
    return x


def table_rows(oracle, dtype):
    """the 16 rows of the table case (read-only)"""
    key = ("table", dtype)
    if key not in _cache:
        dt = _np(dtype)
        pairs = built_pairs(dt)
        rng = np.random.default_rng(2001)
        rows = np.empty((16, N), dtype=dt)
        # wide: the root step's pairs (e, e + 512)
        code = oracle.Code(N, 512, None)
        sig = oracle.sigma_from_db(1.0)
        _, ys = oracle.Sim(2002).frames(code, sig, 2)
        for r in range(2):
            rows[r] = oracle.llr_from_y(ys[r], sig).astype(dt)
            for k, (a, b) in enumerate(pairs):
                e = (5 * k + 3 * r) % 512 if r else k     # row 1: the same pairs at other elements (other lanes), swapped
                rows[r, e], rows[r, e + 512] = (b, a) if r else (a, b)
        assert len(set((5 * k + 3) % 512 for k in range(len(pairs)))) == len(pairs)
        # narrow: elements (i, i + 4) of the level-3 node above octet 0
        slots = [pairs[k % len(pairs)] for k in range(14 * 4)]
        assert len(pairs) <= len(slots)
        rows[2:] = rng.choice(np.array([64, 96, 128], dtype=dt), size=(14, N))
        for k, (a, b) in enumerate(slots):
            rows[2 + k // 4, k % 4], rows[2 + k // 4, k % 4 + 4] = a, b
        rows.setflags(write=False)
        _cache[key] = rows
    return _cache[key]


def _code(oracle, info, crc):
    taps = oracle.CRC24C_TAPS if crc else None
    s = set(info)
    code = oracle.Code(N, len(info) - (max(taps) if taps else 0), taps, Q=[j for j in range(N) if j not in s] + list(info))
    assert code.info_order.tolist() == list(info)
    return code


def _reference(oracle, code, rows, algo, dtype):
    """the oracle's (u_hat, pm, flags word) for LLR rows"""
    import polardecoding_amd as pa
    from test_cascl_adaptive_host import syndrome
    st = np.zeros((len(rows), 2), dtype=np.int32)
    uh, pm, ties = oracle.decode(code, np.array(rows), algo, L=L, dtype=dtype, stats=st)
    fl = np.where(ties > 0, pa.FLAG_TIE, 0)
    if algo == "CASCL":
        fl = fl | np.where(syndrome(uh, code.info_order, code.taps) == 0, pa.FLAG_CRC_PASS, 0)
    if dtype == "f64":   # the f32 keys are the whole metric: no re-rank there
        fl = fl | np.where(st[:, 0] > 0, pa.FLAG_RERANK, 0)
    return uh, pm, fl.astype(np.uint32)


def _decode_and_compare(oracle, code, algo, dtype, rows, sigma, ref, E, what):
    """one launch of the pair kernel on rows (LLRs, or y with sigma > 0) against ref"""
    import torch
    import polardecoding_amd as pa
    from conftest import unpack_bits
    dec = pa.Decoder(N, code.K, pa.ALGO_CASCL if algo == "CASCL" else pa.ALGO_SCL, L=L, crc_taps=code.taps if algo == "CASCL" else None,
                     info_order=code.info_order, dtype=pa.F64 if dtype == "f64" else pa.F32)
    lib = pa.load_library()
    lib.polar_fill_phase_end.restype = C.c_int
    lib.polar_fill_phase_end.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    io = np.ascontiguousarray(dec.info_order, dtype=np.int32)
    assert lib.polar_fill_phase_end(N, io.ctypes.data_as(C.POINTER(C.c_int)), len(io)) == E, what
    x = torch.from_numpy(np.array(rows)).cuda()
    B = x.shape[0]
    bits = torch.full((B, N // 32), -1, dtype=torch.int32, device="cuda")
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_device(x, sigma=sigma, out_bits=bits, pm=pm, flags=fl)
    dec.synchronize()
    name = dec.kernel_name
    dec.close()
    assert name.startswith("k_scl_fast2<"), name   # the name of both forms; sigma > 0 selects k_scl_fast2_y (k_fast2.hip)
    uh, pm, fl = unpack_bits(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)
    o_uh, o_pm, o_fl = ref
    bad = np.nonzero((uh != o_uh).any(axis=1))[0]
    assert bad.size == 0, f"{what}: decisions differ from the oracle's in frames {bad[:8]}"
    assert np.array_equal(pm.astype(o_pm.dtype), o_pm), f"{what}: path metrics differ in frames {np.nonzero(pm.astype(o_pm.dtype) != o_pm)[0][:8]}"
    assert np.array_equal(fl, o_fl), f"{what}: flags {fl[fl != o_fl][:8]} for {o_fl[fl != o_fl][:8]}"


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_table_cells(variant, oracle):
    algo, crc, dtype, from_y = VARIANTS[variant]
    rows = table_rows(oracle, dtype)
    assert_covers(rows[0, :512], rows[0, 512:], "wide steps")
    assert_covers(rows[1, :512], rows[1, 512:], "wide steps, second row")
    l3 = _level3(np.array(rows[2:]))
    assert np.array_equal(l3, rows[2:, :8]), "the wide steps do not hand elements 0 .. 7 down unchanged"
    # a check node's zero is +0, so -0 reaches a narrow chain only behind a g step (-d of a zero difference: the zero pairs)
    assert_covers(l3[:, :4].ravel(), l3[:, 4:].ravel(), "narrow chains", minus_zero=False)
    code = _code(oracle, list(range(N)), crc)
    ref = _reference(oracle, code, rows, algo, dtype)
    # y with sigma = 1: the kernel's 2 y / sigma / sigma is the row exactly
    x, sigma = (np.array(rows) / _np(dtype)(2), 1.0) if from_y else (rows, 0.0)
    _decode_and_compare(oracle, code, algo, dtype, x, sigma, ref, 0, "table rows, " + variant)


def _row_frames(oracle, name):
    """33 frames at 0.75 dB of a code on the set's information leaves: (y, sigma, llr), read-only"""
    key = ("frames", name)
    if key not in _cache:
        info = FP.codes()[name][2]
        assert FP.rule(info) == SETS[name], name
        sig = oracle.sigma_from_db(0.75)
        _, ys = oracle.Sim(2100 + len(name)).frames(_code(oracle, info, False), sig, NROWS)
        y = np.stack(ys)
        llr = np.stack([oracle.llr_from_y(r, sig) for r in ys])
        y.setflags(write=False)
        llr.setflags(write=False)
        _cache[key] = (y, sig, llr)
    return _cache[key]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SETS))
def test_partial_sum_rows(name, variant, oracle):
    algo, crc, dtype, from_y = VARIANTS[variant]
    y, sig, llr = _row_frames(oracle, name)
    llr = llr.astype(_np(dtype))
    code = _code(oracle, FP.codes()[name][2], crc)
    ref = _reference(oracle, code, llr, algo, dtype)
    if variant == "f64_crc":
        print(f"{name}: E = {SETS[name]}, frames with a tie {int((ref[2] & 1).astype(bool).sum())}, whose CRC passes {int((ref[2] & 2).astype(bool).sum())}")
    _decode_and_compare(oracle, code, algo, dtype, y if from_y else llr, sig if from_y else 0.0, ref, SETS[name],
                        f"{name}, {variant}")


def test_the_row_cases_cover_every_end():
    assert set(SETS.values()) == {0, 128, 192, 256}
