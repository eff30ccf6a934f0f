"""GPU: the pair kernel's list-filling phase (csrc/scl_fast2.h fill_phase()) against the oracle.

Below the leaf E that polar_fill_phase_end names, k_scl_fast2 decodes breadth-first: the first 128 leaves as one butterfly,
every further 64-leaf block as two, one per distinct path, and the information leaves at the end of a block fork without
ranking.  The octet loops take over at octet E / 8 from the state the phase leaves (metrics, partial-sum rows, the level-7
rows of the two paths).  Every case compares decisions, path metric and the flags word with == against the oracle on every
frame; the codes are those of tests/fill_phase_codes.py (tests/test_fill_phase_host.py holds their E on the CPU), built with
info_order= and asserted to run the pair kernel with the E the case is about.

  * the headline code (CRC-24C, K = 512: E = 192, the list full at leaf 191), LLR rows, f64: 48 frames at 2 dB and 48 at
    0 dB (closer fork metrics at leaves 127 / 190 / 191), and B = 1, 2, 3, 65 from both ends of the set: both halves of a
    pair, the odd tail, the second job of a wavefront;
  * the other ends: SCL K = 512 (E = 192 left with four paths), E = 256, E = 128 after a fork at leaves 126 and
    127, E = 128 with leaf 189 information, with one path up to leaf 254 and for the 5G order at K = 256, (c)'s near miss
    at 192, and two codes without the phase (E = 0: the 5G order at K = 768, every leaf information);
  * the y form (sigma > 0), f32 against the f32 oracle;
  * tied, quantised, all-zero and constant rows (tests/llr_families.py) on the headline code: a lambda of +-0 at leaves
    127 / 190 / 191 forks and adds PHI as the per-leaf branch does;
  * two contexts, one with the phase and one without, launched in turn: nothing is carried in the scratch or in LDS.

The oracle decodes every set of frames once (about 2 ms a frame)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_phase_codes as FP  # noqa: E402
import llr_families as F  # noqa: E402

pytestmark = pytest.mark.gpu

N, L = FP.N, 8
_cache = {}


def _code(oracle, name):
    """(oracle code, algo, taps, E) of a code of fill_phase_codes"""
    key = ("code", name)
    if key not in _cache:
        algo, taps, info, _ = FP.codes()[name]
        A = len(info)
        s = set(info)
        code = oracle.Code(N, A - (max(taps) if taps else 0), taps, Q=[j for j in range(N) if j not in s] + list(info))
        assert code.info_order.tolist() == list(info)
        _cache[key] = (code, algo, taps, FP.rule(info))
    return _cache[key]


def _decoder(oracle, name, dtype="f64"):
    import polardecoding_amd as pa
    code, algo, taps, E = _code(oracle, name)
    dec = pa.Decoder(N, code.K, pa.ALGO_CASCL if algo == "CASCL" else pa.ALGO_SCL, L=L, crc_taps=taps,
                     info_order=code.info_order, dtype=pa.F64 if dtype == "f64" else pa.F32)
    assert dec.kernel_name.startswith("k_scl_fast2<"), dec.kernel_name
    lib = pa.load_library()
    lib.polar_fill_phase_end.restype = C.c_int
    lib.polar_fill_phase_end.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    io = np.ascontiguousarray(dec.info_order, dtype=np.int32)
    assert lib.polar_fill_phase_end(N, io.ctypes.data_as(C.POINTER(C.c_int)), len(io)) == E, name
    return dec


def _crc_pass(code, uh):
    r = code.r
    glow = sum(1 << t for t in code.taps if t < r)
    tab = np.zeros(N, dtype=np.uint32)
    rem = 1
    for j in code.info_order:
        tab[j] = rem
        rem <<= 1
        if rem >> r:
            rem = (rem ^ (1 << r)) ^ glow
    return np.bitwise_xor.reduce(np.where(uh.astype(bool), tab[None, :], np.uint32(0)), axis=1) == 0


def _reference(oracle, name, rows, dtype="f64"):
    """the oracle's (u_hat, pm, flags word) for LLR rows"""
    import polardecoding_amd as pa
    code, algo, _, _ = _code(oracle, name)
    st = np.zeros((len(rows), 2), dtype=np.int32)
    uh, pm, ties = oracle.decode(code, rows, algo, L=L, dtype=dtype, stats=st)
    fl = np.where(ties > 0, pa.FLAG_TIE, 0)
    if algo == "CASCL":
        fl = fl | np.where(_crc_pass(code, uh), pa.FLAG_CRC_PASS, 0)
    if dtype == "f64":   # the f32 keys are the whole metric: no re-rank there
        fl = fl | np.where(st[:, 0] > 0, pa.FLAG_RERANK, 0)
    out = (uh, pm, fl.astype(np.uint32))
    for a in out:
        a.setflags(write=False)
    return out


def _frames(oracle, name, seed, db, B):
    """(y [B][N], sigma, llr [B][N]) of B frames of the oracle's transmit chain"""
    sig = oracle.sigma_from_db(db)
    _, ys = oracle.Sim(seed).frames(_code(oracle, name)[0], sig, B)
    y = np.stack(ys)
    return y, sig, np.stack([oracle.llr_from_y(r, sig) for r in ys])


def _run(dec, rows, sigma=0.0):
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
    assert dec.kernel_name.startswith("k_scl_fast2"), dec.kernel_name
    return unpack_bits(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    uh, pm, fl = got
    o_uh, o_pm, o_fl = want
    bad = np.nonzero((uh != o_uh).any(axis=1))[0]
    assert bad.size == 0, f"{what}: decisions differ from the oracle's in frames {bad[:8]}"
    assert np.array_equal(pm.astype(o_pm.dtype), o_pm), f"{what}: path metrics differ in frames {np.nonzero(pm.astype(o_pm.dtype) != o_pm)[0][:8]}"
    assert np.array_equal(fl, o_fl), f"{what}: flags {fl[fl != o_fl][:8]} for {o_fl[fl != o_fl][:8]}"


def _headline(oracle, dtype="f64"):
    """96 frames of the headline code, 48 at 2 dB then 48 at 0 dB: (y, sigma of each half, llr, reference)"""
    key = ("headline", dtype)
    if key not in _cache:
        y2, s2, l2 = _frames(oracle, "headline", 4201, 2.0, 48)
        y0, s0, l0 = _frames(oracle, "headline", 4202, 0.0, 48)
        llr = np.concatenate([l2, l0])
        if dtype == "f32":
            llr = llr.astype(np.float32)
        llr.setflags(write=False)
        _cache[key] = (np.concatenate([y2, y0]), (s2, s0), llr, _reference(oracle, "headline", llr, dtype))
    return _cache[key]


def test_headline_code_all_frames(oracle):
    _, _, llr, ref = _headline(oracle)
    dec = _decoder(oracle, "headline")
    _same(_run(dec, llr), ref, "96 frames")
    dec.close()


@pytest.mark.parametrize("B", [1, 2, 3, 65])
def test_headline_code_batch_sizes(B, oracle):
    _, _, llr, ref = _headline(oracle)
    dec = _decoder(oracle, "headline")
    n = len(llr)
    _same(_run(dec, llr[:B]), tuple(a[:B] for a in ref), f"first {B}")
    _same(_run(dec, llr[n - B:]), tuple(a[n - B:] for a in ref), f"last {B}")
    dec.close()


@pytest.mark.parametrize("name,db", [("scl512", 1.0), ("e256", 2.0), ("one_path", 1.0), ("pair_126_127", 2.0),
                                     ("leaf_189", 2.0), ("two_before_192", 1.0), ("k768", 5.0), ("all_info", 9.0), ("k256", -1.5)])
def test_other_ends(name, db, oracle):
    assert _code(oracle, name)[3] == FP.codes()[name][3]
    _, _, llr = _frames(oracle, name, 4300 + len(name), db, 33)
    ref = _reference(oracle, name, llr)
    dec = _decoder(oracle, name)
    print(f"{name}: E = {_code(oracle, name)[3]}, {int((ref[0] != 0).any(axis=1).sum())} frames with a non-zero decision")
    _same(_run(dec, llr), ref, name)
    _same(_run(dec, llr[::-1]), tuple(a[::-1] for a in ref), name + ", reversed")
    dec.close()


def test_the_cases_cover_every_end(oracle):
    names = ["headline", "scl512", "e256", "one_path", "pair_126_127", "leaf_189", "two_before_192", "k768", "all_info", "k256"]
    ends = [_code(oracle, n)[3] for n in names]
    assert {0, 128, 192, 256} <= set(ends) and ends.count(0) >= 2, ends


def test_y_form(oracle):
    y, (s2, s0), _, ref = _headline(oracle)
    dec = _decoder(oracle, "headline")
    _same(_run(dec, y[:48], s2), tuple(a[:48] for a in ref), "y rows, 2 dB")
    _same(_run(dec, y[48:][:47], s0), tuple(a[48:][:47] for a in ref), "y rows, 0 dB, odd batch")
    dec.close()
    yy, sig, llr = _frames(oracle, "scl512", 4401, 1.0, 9)
    dec = _decoder(oracle, "scl512")
    _same(_run(dec, yy, sig), _reference(oracle, "scl512", llr), "SCL, y rows")
    dec.close()


@pytest.mark.parametrize("name", ["headline", "scl512", "e256"])
def test_f32_against_the_f32_oracle(name, oracle):
    if name == "headline":
        _, _, llr, ref = _headline(oracle, "f32")
    else:
        llr = _frames(oracle, name, 4500, 1.5, 33)[2].astype(np.float32)
        ref = _reference(oracle, name, llr, "f32")
    dec = _decoder(oracle, name, "f32")
    _same(_run(dec, llr), ref, name + " f32")
    _same(_run(dec, llr[:63]), tuple(a[:63] for a in ref), name + " f32, B = 63")
    dec.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_degenerate_rows(dtype, oracle):
    """the grids, the hard rows, mixed zero signs and the planted all-zero / constant / huge / subnormal rows"""
    llr = _headline(oracle)[2][32:64]   # 16 frames at 2 dB, 16 at 0 dB
    np_dt = np.float64 if dtype == "f64" else np.float32
    fam = F.families(np.array(llr), 4600, np_dt)
    x = np.concatenate(list(fam.values()))
    assert (x == 0).all(axis=1).any() and np.signbit(x[(x == 0).all(axis=1)]).any()
    ref = _reference(oracle, "headline", x, dtype)
    import polardecoding_amd as pa
    assert (ref[2] & pa.FLAG_TIE).any()
    dec = _decoder(oracle, "headline", dtype)
    _same(_run(dec, x), ref, "families " + dtype)
    _same(_run(dec, x[::-1]), tuple(a[::-1] for a in ref), "families reversed " + dtype)
    dec.close()


def test_alternating_launches(oracle):
    """a context with the phase and one without take turns: same results every time"""
    _, _, llr, ref = _headline(oracle)
    _, _, llr0 = _frames(oracle, "k768", 4700, 5.0, 33)
    ref0 = _reference(oracle, "k768", llr0)
    a, b = _decoder(oracle, "headline"), _decoder(oracle, "k768")
    for turn in range(3):
        _same(_run(a, llr[turn:]), tuple(r[turn:] for r in ref), f"with the phase, turn {turn}")
        _same(_run(b, llr0), ref0, f"without the phase, turn {turn}")
    a.close()
    b.close()
