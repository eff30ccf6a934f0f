"""GPU: the pair kernel (k_scl_fast2 / k_scl_fast2_y, csrc/scl_fast2.h) where the narrow check nodes of an octet look the
staircase up ONCE (chk_narrow()): the lower lane of a pair computes s = x + y, the upper lane y - x = -d with the partner's
sign flipped, one look-up serves both and the lower lane fetches T(|d|) from its neighbour.  What can go wrong is narrow:
the flip lands in a lane that is read, T(|s|) and T(|d|) are swapped or come from the wrong lane, a slot refilled at a fork
keeps its own T(|d|) instead of its source's.  Every case compares decisions, path metric and flags with == against the
oracle, N = 1024, L = 8, in the four variants of tests/test_gpu_fast2_lds_layout.py (f64 with CRC-24C, f64 without CRC, f32
against the f32 oracle, the y form); the frames, codes and the comparison are that module's.

Frames: 33 frames at 0.75 dB -- most information leaves rank and paths fork -- on the information sets of
tests/fill_phase_codes.py with E = 0, 128, 192 and 256.  One decoder decodes the first 1, 2 and 3 of them (a lone codeword,
one pair, a pair and a lone codeword) and then all 33 three times; every launch is compared.

Crafted rows, on the code in which every leaf is an information leaf (octet 0 goes through the narrow chains of octet(),
every leaf ranks).  A row holds +64 .. +128 everywhere but at a few elements of the level-3 node above octet 0, so the wide
steps hand those elements down unchanged (CHK(v, big) is v), the other elements of the node stay big, and
  * a level-1 row has (x, y) at elements 0, 2 and a second pair at elements 1, 3 (big at 4 .. 7): the operands of the two
    level-1 nodes of octet 0's first chain, in pos 0 and pos 1 (partners in pos 2, 3);
  * a level-0 row has (x, y) at elements 0, 1 (big at 2 .. 7): the operands of the level-0 node above leaves 0 and 1.
`_nodes` restates the tree in numpy and the test asserts, before it decodes, that the hand-down is exact and that at each of
the two node kinds every case occurs: x - y at each of the seven thresholds at -1 ulp, exact and +1 ulp while x + y lies in
another table cell, the mirror image with x + y at the thresholds, each for the four sign combinations of (s, d), and
x == y, x == -y.  From the second threshold up the other operand also has another table VALUE than both sides of the
threshold, so that swapped look-ups change the node's result (at the first, 0.196, it cannot: operands whose difference
is exactly 0.196 +- 1 ulp lie below 0.25 each, which keeps the other operand below 0.304, under the second threshold)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_phase_codes as FP  # noqa: E402
import test_gpu_fast2_lds_layout as LL  # noqa: E402

pytestmark = pytest.mark.gpu

N, L = LL.N, LL.L
VARIANTS = LL.VARIANTS
SETS = {"k768": 0, "pair_126_127": 128, "headline": 192, "e256": 256}
COUNTS = (1, 2, 3, 33, 33, 33)
_cache = {}


def _T(x):
    dt = x.dtype.type
    return np.array(LL.TV, dtype=dt)[np.searchsorted(np.array(LL.THR, dtype=dt), np.abs(x), side="right")]


class _Launches:
    """one decoder, several launches, each compared with the oracle's rows"""

    def __init__(self, code, algo, dtype):
        import polardecoding_amd as pa
        self.dec = pa.Decoder(N, code.K, pa.ALGO_CASCL if algo == "CASCL" else pa.ALGO_SCL, L=L,
                              crc_taps=code.taps if algo == "CASCL" else None, info_order=code.info_order,
                              dtype=pa.F64 if dtype == "f64" else pa.F32)

    def compare(self, rows, sigma, ref, what):
        import torch
        from conftest import unpack_bits
        x = torch.from_numpy(np.array(rows)).cuda()
        B = x.shape[0]
        bits = torch.full((B, N // 32), -1, dtype=torch.int32, device="cuda")
        pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
        fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.dec.decode_device(x, sigma=sigma, out_bits=bits, pm=pm, flags=fl)
        self.dec.synchronize()
        assert self.dec.kernel_name.startswith("k_scl_fast2<"), self.dec.kernel_name
        uh, pm, fl = unpack_bits(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)
        o_uh, o_pm, o_fl = (r[:B] for r in ref)
        bad = np.nonzero((uh != o_uh).any(axis=1))[0]
        assert bad.size == 0, f"{what}: decisions differ from the oracle's in frames {bad[:8]}"
        assert np.array_equal(pm.astype(o_pm.dtype), o_pm), f"{what}: path metrics differ in frames {np.nonzero(pm.astype(o_pm.dtype) != o_pm)[0][:8]}"
        assert np.array_equal(fl, o_fl), f"{what}: flags {fl[fl != o_fl][:8]} for {o_fl[fl != o_fl][:8]}"

    def close(self):
        self.dec.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SETS))
def test_frames(name, variant, oracle):
    algo, crc, dtype, from_y = VARIANTS[variant]
    assert FP.rule(FP.codes()[name][2]) == SETS[name], name
    y, sig, llr = LL._row_frames(oracle, name)
    llr = llr.astype(LL._np(dtype))
    code = LL._code(oracle, FP.codes()[name][2], crc)
    ref = LL._reference(oracle, code, llr, algo, dtype)
    if variant == "f64_crc":
        print(f"{name}: E = {SETS[name]}, frames with a tie {int((ref[2] & 1).astype(bool).sum())}, re-ranked {int((ref[2] & 4).astype(bool).sum())}")
    run = _Launches(code, algo, dtype)
    try:
        for k, B in enumerate(COUNTS):
            run.compare((y if from_y else llr)[:B], sig if from_y else 0.0, ref, f"{name}, {variant}, launch {k}: {B} frames")
    finally:
        run.close()


def test_the_frame_cases_cover_every_end():
    assert set(SETS.values()) == {0, 128, 192, 256} and set(COUNTS) == {1, 2, 3, 33} and COUNTS.count(33) == 3


# ---- crafted rows ----
def _targets(dt):
    """the 21 threshold neighbours: (threshold index, -1 / 0 / +1 ulp, value)"""
    out = []
    for k, t in enumerate(LL.THR):
        t = dt(t)
        out += [(k, -1, np.nextafter(t, dt(0))), (k, 0, t), (k, 1, np.nextafter(t, dt(16)))]
    return out


def _other(dt, t, sign):
    """an operand u = sign * |u| for the other look-up of a node whose one look-up is at t > 0: (u + t) / 2 and (u - t) / 2
    are exact, so are their sum and difference, and |u| lies in another table cell -- where possible with a table value
    that differs from those on both sides of t's threshold"""
    centre = [dt(2.0 ** ((k - 1) // 8 - 3) * (1 + ((k - 1) % 8 + 0.5) / 8)) for k in range(1, 49)] + [dt(12), dt(0.0625), dt(0.03125)]
    cand = []
    for c in centre:
        cand += [c, np.nextafter(c, dt(16))]
    near = {float(_T(np.nextafter(t, dt(0)))), float(_T(t)), float(_T(np.nextafter(t, dt(16))))}
    cand.sort(key=lambda c: float(_T(c)) in near)   # stable: the candidates with another table value first
    for c in cand:
        u = dt(sign) * c
        a, b = (u + t) / dt(2), (u - t) / dt(2)
        if a + b == u and a - b == t and LL.cell_of(np.array([u]))[0] != LL.cell_of(np.array([t]))[0]:
            return u
    raise AssertionError(f"no exact partner for {t!r}")


def crafted_pairs(dt):
    """(x, y) per case of a narrow node, in a fixed order"""
    pairs = []
    for _, _, t in _targets(dt):
        for st in (1, -1):
            for su in (1, -1):
                d, s = dt(st) * t, _other(dt, t, su)         # x - y at the threshold, x + y in another cell
                pairs.append(((s + d) / dt(2), (s - d) / dt(2)))
                s, d = dt(st) * t, _other(dt, t, su)         # the mirror image
                pairs.append(((s + d) / dt(2), (s - d) / dt(2)))
    for a in (dt(0.3), dt(-0.3), dt(2.252), dt(-5.0)):
        pairs += [(a, a), (a, -a)]                           # x == y: d = +0; x == -y: s = +0
    return pairs


def crafted_rows(dtype):
    """the rows (read-only) and, per row, the node kind it serves: 1 (two level-1 nodes) or 0 (one level-0 node)"""
    key = ("rows", dtype)
    if key not in _cache:
        dt = LL._np(dtype)
        pairs = crafted_pairs(dt)
        assert len(pairs) % 2 == 0
        n1 = len(pairs) // 2
        rng = np.random.default_rng(2201)
        rows = rng.choice(np.array([64, 96, 128], dtype=dt), size=(n1 + len(pairs), N))
        for k, (a, b) in enumerate(pairs):
            r, i = k // 2, k % 2
            rows[r, i], rows[r, i + 2] = a, b                # level 1: elements (0, 2) and (1, 3)
            rows[n1 + k, 0], rows[n1 + k, 1] = a, b          # level 0: elements (0, 1)
        kind = np.array([1] * n1 + [0] * len(pairs))
        rows.setflags(write=False)
        _cache[key] = (rows, kind)
    return _cache[key]


def _nodes(l3):
    """the operands (x, y) of the narrow nodes of octet 0's first chain, from elements 0 .. 7 of the level-3 node:
    the two level-1 nodes [rows][2] and the level-0 node [rows]"""
    v2 = LL._chk(l3[:, :4], l3[:, 4:])
    v1 = LL._chk(v2[:, :2], v2[:, 2:])
    return (v2[:, :2], v2[:, 2:]), (v1[:, 0], v1[:, 1])


def assert_cases(x, y, what):
    """every case of the docstring occurs among the nodes with operands (x, y)"""
    dt = x.dtype.type
    s, d = x + y, x - y
    other_cell = LL.cell_of(s) != LL.cell_of(d)
    for k, u, t in _targets(dt):
        near = [_T(np.nextafter(t, dt(0))), _T(t), _T(np.nextafter(t, dt(16)))]
        for at, ot, name in ((d, s, "x - y"), (s, d, "x + y")):
            for st in (1, -1):
                for so in (1, -1):
                    hit = (at == dt(st) * t) & (np.sign(ot) == so) & other_cell
                    assert hit.any(), f"{what}: {name} = {st} * (threshold {k} {u:+d} ulp), other operand's sign {so}"
                    # from the second threshold up the other look-up has a value of its own: swapped look-ups show
                    assert k == 0 or (hit & ~np.isin(_T(ot), near)).any(), (what, name, k, u, st, so)
    assert ((x == y) & (x != 0)).any() and ((x == -y) & (x != 0)).any(), what


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_crafted_rows(variant, oracle):
    algo, crc, dtype, from_y = VARIANTS[variant]
    rows, kind = crafted_rows(dtype)
    l3 = LL._level3(np.array(rows))
    # the wide steps hand the built elements down unchanged and leave the others big (a check node of two big values
    # takes up to 0.65 off the smaller one, seven times)
    assert np.array_equal(l3[kind == 1, :4], rows[kind == 1, :4]) and np.array_equal(l3[kind == 0, :2], rows[kind == 0, :2])
    assert (l3[kind == 1, 4:] >= 59).all() and (l3[kind == 0, 2:] >= 59).all()
    (x1, y1), (x0, y0) = _nodes(l3)
    assert np.array_equal(x1[kind == 1], rows[kind == 1, 0:2]) and np.array_equal(y1[kind == 1], rows[kind == 1, 2:4])
    assert np.array_equal(x0[kind == 0], rows[kind == 0, 0]) and np.array_equal(y0[kind == 0], rows[kind == 0, 1])
    assert_cases(x1[kind == 1].ravel(), y1[kind == 1].ravel(), "level-1 nodes")
    assert_cases(x0[kind == 0], y0[kind == 0], "level-0 nodes")
    code = LL._code(oracle, list(range(N)), crc)
    key = ("ref", algo, dtype)
    if key not in _cache:
        _cache[key] = LL._reference(oracle, code, rows, algo, dtype)
    x, sigma = (np.array(rows) / LL._np(dtype)(2), 1.0) if from_y else (rows, 0.0)
    run = _Launches(code, algo, dtype)
    try:
        run.compare(x, sigma, _cache[key], "crafted rows, " + variant)
    finally:
        run.close()
