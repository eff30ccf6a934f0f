"""GPU: every decoder kernel on frozen sets outside the 5G reliability order (tests/frozen_patterns.py) against the CPU
oracle -- and, where the repository has one, the decoder's numpy model (scf_model, scan_model, the BP stop-point restatement,
the adaptive rule's composition).  tests/test_frozen_patterns_host.py holds the conditions: the families reach all 256 octet
masks, both values of "leaf 0 information" and "last leaf frozen", leading runs of 0, 14, 15, 16, 17 octets, alternating
all-frozen / all-information spans of every size -- none of which a set cut from the 5G order has -- and the oracle equals a
second list-decoder model on every family.

Every comparison is == : decisions, the path metric (list decoders; f32 metrics compared as float32), FLAG_TIE, and for
CA-SCL FLAG_CRC_PASS from the syndrome of the oracle's chosen path.  No frame is left out.  The decoders are built from
info_order = a seeded permutation of the family's information positions (the CRC positions I[0..r) lie anywhere in the
set), and the library's info_order must return it.  Frames: the oracle's transmit chain on the same code, half at 1.0 dB
and half at 4.0 dB, LLRs rounded through float32; four families are run again on the (1, 7) grid of tests/llr_families.py,
where magnitudes tie.  Each test asserts the kernel it reached and the number of family batches it ran."""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frozen_patterns as P  # noqa: E402
import llr_families as F  # noqa: E402
from test_bp_early_stop_host import stop_points  # noqa: E402
from test_cascl_adaptive_host import CRC6, CRC24C, FLAG_CRC_PASS, syndrome  # noqa: E402
from test_gpu_cascl_adaptive import _oracle_composition  # noqa: E402
from test_gpu_llr_families import _bp, _cuda, _fixed, _np, _oracle, _pa, _same_pm, _same_scf, _scf, _unpack  # noqa: E402
from test_scan_host import scan_model  # noqa: E402
from test_scf_host import scf_model  # noqa: E402

FLAG_TIE = 1
DTYPES = ["f64", "f32"]
GRID_FAMILIES = ("octets_lo", "islands_32_a", "leaf0", "sparse_5_half")
TAPS = {128: CRC6, 1024: CRC24C}
ALGO = {"SC": 0, "BP": 1, "SCL": 2, "CASCL": 3, "SCF": 4, "SCAN": 5}


def _seed(N, name):
    return 1000 + N + zlib.crc32(name.encode()) % 100000


def _code(oracle, N, name, mask, taps=None):
    """(oracle code, info_order) of family `name`: K = A - r payload bits, the CRC at a seeded permutation's first r entries"""
    r = max(taps) if taps else 0
    order = P.order_of(mask, _seed(N, name))
    code = oracle.Code(N, order.size - r, taps, Q=P.q_of(mask, order))
    assert np.array_equal(code.frozen, mask) and np.array_equal(code.info_order, order), name
    return code, order


def _dec(N, mask, order, algo, L=1, taps=None, dtype="f64", **kw):
    """a library context on the same set; the frozen array of its info_order must be the family's mask"""
    import polardecoding_amd as pa
    r = max(taps) if taps else 0
    dec = pa.Decoder(N, order.size - r, ALGO[algo], L=L, crc_taps=taps, dtype=_pa(dtype), info_order=order, **kw)
    got = dec.info_order
    assert np.array_equal(got, order), "info_order does not return what went in"
    fz = np.ones(N, dtype=np.uint8)
    fz[got] = 0
    assert np.array_equal(fz, mask), "the library's frozen set is not the family's"
    assert dec.A == order.size and dec.N == N
    return dec


def _llr(oracle, code, B, seed, grid=False):
    """B frames of the code's own transmit chain, half at 1.0 dB and half at 4.0 dB, through float32"""
    h = B // 2
    x = np.concatenate([F.oracle_llr(oracle, code, h, seed, 1.0), F.oracle_llr(oracle, code, B - h, seed + 1, 4.0)])
    x = x.astype(np.float32).astype(np.float64)
    return F.grid(x, 1.0, 7) if grid else x


def _batches(fam):
    """(family, grid?) in running order: every family on Gaussian rows, the GRID_FAMILIES among them again on the grid"""
    return [(k, False) for k in fam] + [(k, True) for k in GRID_FAMILIES if k in fam]


_REFS = {}


def _list_ref(oracle, N, name, mask, algo, L, dtype, B, grid):
    """(order, rows, oracle's (u_hat, pm, ties, stats), CRC pass of the oracle's path): computed once, shared by the kernels
    that decode the same shape, never modified"""
    key = (N, name, algo, L, dtype, B, grid)
    if key not in _REFS:
        taps = TAPS[N] if algo == "CASCL" else None
        code, order = _code(oracle, N, name, mask, taps)
        x = _llr(oracle, code, B, _seed(N, name), grid).astype(_np(dtype))
        ref = _oracle(oracle, code, x, algo, L=L, dtype=dtype)
        ok = syndrome(ref[0], order, taps) == 0 if taps else None
        for a in (order,) + tuple(ref):
            a.setflags(write=False)
        _REFS[key] = (order, x, ref, ok)
    return _REFS[key]


def _check_list(dec, x, ref, ok, dtype, label):
    uh, pm, fl = _fixed(dec, x)
    o_uh, o_pm, o_ties, _ = ref
    bad = np.flatnonzero((uh != o_uh).any(axis=1))
    if bad.size:
        j = int(np.flatnonzero(uh[bad[0]] != o_uh[bad[0]])[0])
        assert False, (label, dec.kernel_name, "u_hat differs in frames", bad[:8], "first leaf", j, "of frame", int(bad[0]))
    _same_pm(pm, o_pm, dtype, (label, dec.kernel_name, "pm"))
    assert np.array_equal((fl & FLAG_TIE) != 0, o_ties > 0), (label, dec.kernel_name, "FLAG_TIE")
    if ok is not None:
        assert np.array_equal((fl & FLAG_CRC_PASS) != 0, ok), (label, dec.kernel_name, "FLAG_CRC_PASS")


def _run_list(oracle, N, fam, algo, L, dtype, B, kernel, variant=None, grids=True):
    """every family of `fam` through one list kernel; returns the number of batches run"""
    from polardecoding_amd import testing as T
    ran = 0
    for name, grid in (_batches(fam) if grids else [(k, False) for k in fam]):
        order, x, ref, ok = _list_ref(oracle, N, name, fam[name], algo, L, dtype, B, grid)
        dec = _dec(N, fam[name], order, algo, L=L, taps=TAPS[N] if algo == "CASCL" else None, dtype=dtype)
        if variant is not None:
            T.select_kernel(dec, variant)
        assert dec.kernel_name.startswith(kernel), (name, dec.kernel_name)
        _check_list(dec, x, ref, ok, dtype, f"{name}{' grid' if grid else ''} {algo} N={N} L={L} {dtype}")
        dec.close()
        ran += 1
    return ran


def _families(N, algo, *prefixes):
    fam = P.families(N)
    if algo in ("CASCL", "SCF"):
        fam = P.with_crc(fam, N)
    return P.select(fam, *prefixes) if prefixes else fam


# ---- the tuned L = 8 kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("algo", ["SCL", "CASCL"])
def test_pair_kernel_on_every_family(algo, dtype, oracle):
    """k_scl_fast2, N = 1024, L = 8, 37 frames (odd: the last wavefront has one idle half)"""
    fam = _families(1024, algo)
    ran = _run_list(oracle, 1024, fam, algo, 8, dtype, 37, "k_scl_fast2<")
    assert ran == (38 + 4 if algo == "SCL" else 33 + 3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("algo", ["SCL", "CASCL"])
def test_one_per_wave_kernel_n128_on_every_family(algo, dtype, oracle):
    """k_scl_fast, N = 128, L = 8 (CRC-6)"""
    fam = _families(128, algo)
    ran = _run_list(oracle, 128, fam, algo, 8, dtype, 37, "k_scl_fast<")
    assert ran == (30 + 4 if algo == "SCL" else 25 + 3)


@pytest.mark.parametrize("algo", ["SCL", "CASCL"])
@pytest.mark.parametrize("variant,kernel", [("KERNEL_ONE_PER_WAVE", "k_scl_fast<"), ("KERNEL_FOUR_PER_WAVE", "k_scl_fast4<")])
def test_selectable_kernels_n1024(variant, kernel, algo, oracle):
    """k_scl_fast and k_scl_fast4 at N = 1024 (37 frames: one of four codewords live in the last wavefront) on the octet,
    lead and leaf0 families (fast4: and the sparse ones); the references are those of the pair-kernel test"""
    from polardecoding_amd import testing as T
    pre = ("octets_", "lead_", "leaf0") + (("sparse_",) if kernel == "k_scl_fast4<" else ())
    fam = _families(1024, algo, *pre)
    ran = _run_list(oracle, 1024, fam, algo, 8, "f64", 37, kernel, variant=getattr(T, variant))
    want = {("k_scl_fast<", "SCL"): 10 + 2, ("k_scl_fast<", "CASCL"): 9 + 2, ("k_scl_fast4<", "SCL"): 14 + 3,
            ("k_scl_fast4<", "CASCL"): 9 + 2}
    assert ran == want[(kernel, algo)]


# ---- k_scl_big -------------------------------------------------------------------------------------------------------------
BIG_SHAPES = [(512, 2, None), (512, 32, None), (1024, 4, None), (1024, 8, "KERNEL_BIG"), (2048, 4, None)]


@pytest.mark.parametrize("N,L,variant", BIG_SHAPES)
def test_big_kernel(N, L, variant, oracle):
    """k_scl_big: the per-leaf frozen word at N = 512 (L = 2, 32), 1024 (L = 4; L = 8 selected) and 2048 (upper levels in
    scratch) on the octet, islands, leaf0, sparse and dense families, 9 frames; CA-SCL too at N = 1024"""
    from polardecoding_amd import testing as T
    pre = ("octets_", "islands_", "leaf0", "sparse_", "dense_")
    fam = _families(N, "SCL", *pre)
    ran = _run_list(oracle, N, fam, "SCL", L, "f64", 9, "k_scl_big<", variant=getattr(T, variant) if variant else None)
    assert ran == 2 + 12 + 2 + 4 + 4 + 4
    if N == 1024:
        fam = _families(N, "CASCL", *pre)
        ran = _run_list(oracle, N, fam, "CASCL", L, "f32" if L == 4 else "f64", 9, "k_scl_big<",
                        variant=getattr(T, variant) if variant else None)
        assert ran == 2 + 12 + 2 + 4 + 3


# ---- k_scl_generic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 8, 32])
@pytest.mark.parametrize("N", [32, 64, 256])
def test_generic_kernel_on_every_family(N, L, oracle):
    fam = _families(N, "SCL")
    ran = _run_list(oracle, N, fam, "SCL", L, "f64", 13, "k_scl_generic<")
    assert ran == {32: 23 + 3, 64: 27 + 4, 256: 36 + 4}[N]     # islands_32_a, a grid family, needs N > 32


def _run_sc(oracle, N, dtype, B, expect):
    import polardecoding_amd as pa
    fam = P.families(N)
    ran = 0
    for name, grid in _batches(fam):
        code, order = _code(oracle, N, name, fam[name])
        x = _llr(oracle, code, B, _seed(N, name), grid).astype(_np(dtype))
        ref = _oracle(oracle, code, x, "SC", dtype=dtype)[0]
        dec = _dec(N, fam[name], order, "SC", dtype=dtype)
        assert expect in dec.kernel_name, dec.kernel_name
        uh, _, _ = _fixed(dec, x)
        bad = np.flatnonzero((uh != ref).any(axis=1))
        assert bad.size == 0, (name, grid, N, dtype, dec.kernel_name, "frames", bad[:8], "first leaf",
                               int(np.flatnonzero(uh[bad[0]] != ref[bad[0]])[0]))
        dec.close()
        ran += 1
    assert ran == len(fam) + (3 if N == 32 else 4) and pa.ALGO_SC == 0
    return ran


@pytest.mark.parametrize("N", [32, 64, 256])
def test_generic_kernel_sc_below_64_frames(N, oracle):
    _run_sc(oracle, N, "f64", 13, "k_scl_generic below")


# ---- one codeword per lane ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [32, 128, 1024, 2048])
def test_sc_lanes_on_every_family(N, dtype, oracle):
    """k_sc_lanes, 131 frames (two full wavefronts plus three lanes)"""
    ran = _run_sc(oracle, N, dtype, 131, "k_sc_lanes<")
    assert ran == {32: 23 + 3, 128: 30 + 4, 1024: 38 + 4, 2048: 37 + 4}[N]


SCF_PARTS = [(128, 0, 1)] + [(1024, k, 5) for k in range(5)]


@pytest.mark.parametrize("N,part,parts", SCF_PARTS)
def test_scf_lanes_on_every_family_with_a_crc(N, part, parts, oracle):
    """k_scf_lanes, T = 8, 131 frames, against scf_model; the N = 1024 families in five parts (the model is slow)"""
    names = list(_families(N, "SCF"))
    assert len(names) == {128: 25, 1024: 33}[N]
    fam = P.families(N)
    ran = 0
    for name in names[part::parts]:
        code, order = _code(oracle, N, name, fam[name], TAPS[N])
        x = _llr(oracle, code, 131, _seed(N, name))
        want = scf_model(code, x, 8, oracle=oracle)
        dec = _dec(N, fam[name], order, "SCF", taps=TAPS[N])
        assert dec.kernel_name.startswith("k_scf_lanes<") and "T=8" in dec.kernel_name, dec.kernel_name
        _same_scf(_scf(dec, x), want, (name, N))
        dec.close()
        ran += 1
    assert ran == len(names[part::parts]) and ran >= 6


@pytest.mark.parametrize("name", ["bern_0.5", "islands_64_a", "leaf0"])
def test_adaptive_cascl_1_8_32(name, oracle):
    """stages (1, 8, 32) at N = 1024: k_sc_lanes, k_scl_fast2 and k_scl_big with the glue kernels, 131 frames"""
    import torch
    N, B, stages = 1024, 131, (1, 8, 32)
    code, order = _code(oracle, N, name, P.families(N)[name], CRC24C)
    x = _llr(oracle, code, B, _seed(N, name))
    dec = _dec(N, P.families(N)[name], order, "CASCL", L=32, taps=CRC24C)
    dec.set_cascl_stages(stages)
    for k in ("k_sc_lanes<", "k_scl_fast2<", "k_scl_big<"):
        assert k in dec.kernel_name, dec.kernel_name
    parts = [_oracle_composition(oracle, code, CRC24C, stages, x[i:i + 33]) for i in range(0, B, 33)]
    wu, wpm, wfl, wls = (np.concatenate([p[k] for p in parts]) for k in range(4))
    d = _cuda(x)
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ls = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_cascl_device(d, pm=pm, flags=fl, list_size=ls)
    dec.synchronize()
    uh, pm = _unpack(bits.cpu().numpy(), N), pm.cpu().numpy()
    fl, ls = fl.cpu().numpy().view(np.uint32).astype(np.int64), ls.cpu().numpy().astype(np.int64)
    print(f"adaptive {name}: frames decided per list size {dict(zip(*np.unique(wls, return_counts=True)))}")
    assert np.array_equal(ls, wls), (name, np.unique(ls, return_counts=True), np.unique(wls, return_counts=True))
    assert np.array_equal(uh, wu), name
    assert np.array_equal(pm, wpm), name
    assert np.array_equal(fl & (FLAG_TIE | FLAG_CRC_PASS), wfl), name


# ---- BP and SCAN ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,kernel", [(128, "k_bp_w128<"), (1024, "k_bp_r4<"), (256, "k_bp<")])
def test_bp_priors_on_custom_sets(N, kernel, oracle):
    """5 round trips, with and without stop rule G, 9 frames, on the octet, Bernoulli, all-information and sparse families"""
    import polardecoding_amd as pa
    fam = P.select(P.families(N), "octets_", "bern_", "dense_all", "sparse_")
    iters, ran = 5, 0
    for name, mask in fam.items():
        code, order = _code(oracle, N, name, mask)
        x = _llr(oracle, code, 9, _seed(N, name))
        dec = _dec(N, mask, order, "BP", bp_iters=iters)
        assert dec.kernel_name.startswith(kernel) and "stop rule" not in dec.kernel_name, dec.kernel_name
        ref, _, _ = oracle.decode(code, x, "BP", bp_iters=iters)
        uh, _, _ = _fixed(dec, x, meta=False)
        assert np.array_equal(uh, ref), (name, N, "fixed")
        dec.set_bp_stop("g")
        assert dec.kernel_name.startswith(kernel) and "stop rule G" in dec.kernel_name, dec.kernel_name
        t_stop, conv, out = stop_points(x, mask, iters)
        uh, it, fl = _bp(dec, x)
        assert np.array_equal(it, t_stop), (name, N, it, t_stop)
        assert np.array_equal(fl, np.where(conv, pa.FLAG_BP_CONVERGED, 0)), (name, N)
        assert np.array_equal(uh, out), (name, N, "stop rule G")
        for t in np.unique(it):
            sel = it == t
            r2, _, _ = oracle.decode(code, x[sel], "BP", bp_iters=int(t))
            assert np.array_equal(uh[sel], np.atleast_2d(r2)), (name, N, int(t))
        dec.close()
        ran += 1
    assert ran == 2 + 3 + 1 + 4


@pytest.mark.parametrize("N", [128, 1024])
def test_scan_on_islands_and_octets(N, oracle):
    """k_scan_lanes, I = 2, 70 frames, against scan_model(skip=True): soft outputs by == as well"""
    import torch
    fam = P.select(P.families(N), "islands_", "octets_")
    ran = 0
    for name, mask in fam.items():
        code, order = _code(oracle, N, name, mask)
        x = _llr(oracle, code, 70, _seed(N, name))
        dec = _dec(N, mask, order, "SCAN")
        dec.set_scan_iters(2)
        assert dec.kernel_name.startswith("k_scan_lanes<") and "I=2" in dec.kernel_name, dec.kernel_name
        want = scan_model(mask, x, 2, oracle=oracle, skip=True)
        lu = torch.full((70, N), float("nan"), dtype=torch.float64, device="cuda")
        ex = torch.full((70, N), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        bits = dec.decode_scan_device(_cuda(x), llr_u=lu, ext_x=ex)
        dec.synchronize()
        assert np.array_equal(_unpack(bits.cpu().numpy(), N), want[0]), (name, N, "u_hat")
        for nm, g, w in (("llr_u", lu.cpu().numpy(), want[1]), ("ext_x", ex.cpu().numpy(), want[2])):
            assert not np.isnan(g).any() and np.array_equal(np.isinf(g), np.isinf(w)), (name, N, nm)
            assert (g == w).all(), (name, N, nm)
        dec.close()
        ran += 1
    assert ran == {128: 8, 1024: 12}[N] + 2


# ---- the other ways a set comes in -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["islands_32_a", "leaf0", "bern_0.5"])
def test_frozen_mask_override_equals_the_info_order_context(name, oracle):
    """a context built on the 5G set, decode_batch(llr, frozen_mask=mask): the result of the context built from info_order
    (and the oracle's); a later call without the override gives the 5G result again.  SC with 131 frames (k_sc_lanes), SCL
    L = 8 (k_scl_fast2) and BP at N = 1024."""
    import polardecoding_amd as pa
    N = 1024
    mask = P.families(N)[name]
    code, order = _code(oracle, N, name, mask)
    code5g = oracle.Code(N, 512)
    for algo, B, make, kernel in (("SC", 131, lambda: pa.SCdecode(N, 512), "k_sc_lanes<"),
                                  ("SCL", 37, lambda: pa.SCLdecode(N, 512, L=8), "k_scl_fast2<"),
                                  ("BP", 9, lambda: pa.BP(N, 512, iterMax=5), "k_bp_r4<")):
        x = _llr(oracle, code, B, _seed(N, name) + 7)
        base = make()
        assert base.kernel_name.startswith(kernel), base.kernel_name
        own = _dec(N, mask, order, algo, L=8 if algo == "SCL" else 1, **({"bp_iters": 5} if algo == "BP" else {}))
        ref = _oracle(oracle, code, x, algo, L=8, iters=5)
        ref5g = _oracle(oracle, code5g, x, algo, L=8, iters=5)
        before = base.decode_batch(x)
        got = base.decode_batch(x, frozen_mask=mask)
        assert base.kernel_name.startswith(kernel), base.kernel_name   # the dispatch does not depend on the mask
        mine = own.decode_batch(x)
        after = base.decode_batch(x)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(mine[0], ref[0]), (name, algo)
        assert np.array_equal(before[0], ref5g[0]) and np.array_equal(after[0], ref5g[0]), (name, algo)
        assert not np.array_equal(ref[0], ref5g[0])
        if algo == "SCL":
            for r, want in ((got, ref), (mine, ref), (before, ref5g), (after, ref5g)):
                assert np.array_equal(r[1], want[1]), (name, "pm")
                assert np.array_equal((r[2] & FLAG_TIE) != 0, want[2] > 0), (name, "FLAG_TIE")
        base.close()
        own.close()


@pytest.mark.parametrize("name", ["islands_32_a", "tail_quarter", "sparse_last"])
def test_no_output_word_is_left_unwritten(name, oracle):
    """decode_device into out_bits full of ones and pm / flags full of a sentinel: afterwards every frozen bit is 0, every
    decision the oracle's, and no sentinel is left -- k_sc_lanes, k_scl_fast2 and k_scl_big (L = 4) at N = 1024"""
    import torch
    N = 1024
    mask = P.families(N)[name]
    code, order = _code(oracle, N, name, mask)
    for algo, L, B, kernel in (("SC", 1, 131, "k_sc_lanes<"), ("SCL", 8, 37, "k_scl_fast2<"), ("SCL", 4, 9, "k_scl_big<")):
        x = _llr(oracle, code, B, _seed(N, name) + L)
        ref = _oracle(oracle, code, x, algo, L=L)
        dec = _dec(N, mask, order, algo, L=L)
        assert dec.kernel_name.startswith(kernel), dec.kernel_name
        bits = torch.full((B, N // 32), -1, dtype=torch.int32, device="cuda")
        pm = torch.full((B,), -12345.0, dtype=torch.float64, device="cuda")
        fl = torch.full((B,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_device(_cuda(x), out_bits=bits, pm=pm, flags=fl)
        dec.synchronize()
        uh = _unpack(bits.cpu().numpy(), N)
        assert not uh[:, mask != 0].any(), (name, kernel, "a frozen bit is set")
        assert np.array_equal(uh, ref[0]), (name, kernel)
        pm, fl = pm.cpu().numpy(), fl.cpu().numpy()
        assert not (pm == -12345.0).any() and not (fl == 0x5A5A5A5A).any(), (name, kernel, "sentinel left")
        if algo == "SCL":
            assert np.array_equal(pm, ref[1]) and np.array_equal((fl & FLAG_TIE) != 0, ref[2] > 0), (name, kernel)
        else:
            assert not pm.any() and not fl.any(), (name, kernel)
        dec.close()


@pytest.mark.parametrize("L", [1, 8])
def test_decode_llr_cache_crosses_an_eviction(L, oracle):
    """polar_decode_llr keeps eight contexts: ten distinct N = 128 masks in turn, then the first again"""
    import polardecoding_amd as pa
    N = 128
    fam = P.families(N)
    names = ["octets_lo", "octets_hi", "islands_8_b", "islands_32_a", "lead_14", "leaf0", "tail_quarter", "sparse_5_half",
             "dense_all", "bern_0.5"]
    for k, name in enumerate(names + names[:1]):
        code, _ = _code(oracle, N, name, fam[name])
        x = _llr(oracle, code, 2, _seed(N, name) + k)
        for row in x:
            ref, _, _ = oracle.decode(code, row, "SC" if L == 1 else "SCL", L=L)
            assert np.array_equal(pa.decode(row, fam[name], N, L), ref), (name, k, L)


def test_refusals_and_creations():
    """CA-SCL and SC-Flip refuse a frozen_mask override; every algorithm is created on every family the header allows (A == N
    included), and info_order returns what went in (_dec asserts it)"""
    import polardecoding_amd as pa
    made = 0
    for N in (128, 1024):
        fam = P.families(N)
        for k, (name, mask) in enumerate(fam.items()):
            order = P.order_of(mask, k)
            for algo in ("SC", "SCL", "BP", "SCAN") + (("CASCL", "SCF") if name not in P.NO_CRC[N] else ()):
                dec = _dec(N, mask, order, algo, L=8 if algo in ("SCL", "CASCL") else 1,
                           taps=TAPS[N] if algo in ("CASCL", "SCF") else None)
                assert dec.kernel_name
                if algo in ("CASCL", "SCF") and name == "bern_0.5":
                    with pytest.raises(pa.PolarError):
                        dec.decode_batch(np.zeros((2, N)), frozen_mask=mask)
                dec.close()
                made += 1
            if name in P.NO_CRC[N]:
                with pytest.raises(pa.PolarError):
                    _dec(N, mask, order, "CASCL", L=8, taps=TAPS[N])
    assert made == (30 + 38) * 4 + (25 + 33) * 2
