"""GPU: every decoder on quantised, tied and degenerate LLR rows (tests/llr_families.py) against the references the
repository already has -- the oracle for SC / SCL / CA-SCL / BP, scf_model, scan_model, the BP stop-point restatement, the
adaptive rule's composition, the rate-matching model and the genie model.  Everything is compared with == or array_equal,
in f64 and in f32 (f32 against the oracle or model run in float32).

On Gaussian rows two magnitudes almost never coincide; on these rows they coincide all the time
(tests/test_llr_families_host.py holds the conditions: median ties and full-width re-ranks in most CA-SCL frames, flip
lists whose tie rule decides outputs, exact-zero leaves).  A "mixed" batch takes its rows in turn from the three grids and
the hard family, with -0.0 and +0.0 mixed, and has every degenerate row planted three times (in at most half of the batch),
the wavefront boundaries 0, 63, 64, 127, 128, ... and last first.  The kernels that decode one codeword per lane (SC, SC-Flip,
SCAN, genie, and the rate-matched forms of these) get batches of 322 frames or more, where every degenerate row sits on a
boundary; the list kernels put 1, 2 or 4 codewords in a wavefront, and their reversed second pass moves other rows there.
List batches are run twice, the second time reversed.  Each test prints the kernel it exercised (KERNEL lines)."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import llr_families as F  # noqa: E402
import test_construct_host as MC  # noqa: E402
from test_gpu_cascl_adaptive import _oracle_composition  # noqa: E402
import test_rm_host as RM  # noqa: E402
from test_bp_early_stop_host import stop_points  # noqa: E402
from test_cascl_adaptive_host import CRC6, CRC24C  # noqa: E402
from test_llr_families_host import SCF_CASES, SEED  # noqa: E402
from test_scan_host import scan_model  # noqa: E402
from test_scf_host import scf_model  # noqa: E402

FLAG_TIE, FLAG_RERANK = 1, 4
DTYPES = ["f64", "f32"]


def _np(dtype):
    return np.float32 if dtype == "f32" else np.float64


def _pa(dtype):
    import polardecoding_amd as pa
    return pa.F32 if dtype == "f32" else pa.F64


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _code_of(oracle, dec, K, taps):
    """the oracle's code with the decoder's information set (N > 1024 has no 5G table)"""
    io = dec.info_order.tolist()
    s = set(io)
    code = oracle.Code(dec.N, K, taps, Q=[j for j in range(dec.N) if j not in s] + io)
    assert np.array_equal(code.info_order, dec.info_order)
    return code


def _mixed(llr, seed, dtype, degenerate=True):
    """rows in turn from grid(1, 7), grid(0.5, 15), grid(2, 3) and hard, zero signs mixed, degenerate rows planted"""
    dt = np.dtype(_np(dtype))
    B, width = llr.shape
    parts = [F.grid(llr, s, m) for s, m in F.GRIDS] + [F.hard(llr, 2.0)]
    x = np.empty_like(llr)
    for k, p in enumerate(parts):
        x[k::4] = p[k::4]
    x = F.mix_zero_signs(x, seed).astype(dt)
    if degenerate:
        x = F.plant(x, F.degenerate_rows(width, dt, seed, c=2.0), start=seed)
    return x


def _oracle(oracle, code, x, algo, L=1, dtype="f64", iters=20, workers=8):
    """oracle.decode over the rows of x on several host threads (ctypes releases the GIL): (u_hat, pm, ties, stats)"""
    parts = [p for p in np.array_split(np.arange(len(x)), min(len(x), workers * 2)) if len(p)]

    def run(idx):
        st = np.zeros((len(idx), 2), dtype=np.int32)
        uh, pm, ties = oracle.decode(code, x[idx], algo, L=L, bp_iters=iters, dtype=dtype,
                                     stats=st if algo in ("SCL", "CASCL") else None)
        return uh, np.atleast_1d(pm), np.atleast_1d(ties), st

    with ThreadPoolExecutor(workers) as ex:
        res = list(ex.map(run, parts))
    return tuple(np.concatenate([r[k] for r in res]) for k in range(4))


def _fixed(dec, x, sigma=0.0, meta=True):
    """polar_decode_device -> (u_hat, pm float64, flags); meta=False passes no pm / flags buffers (BP)"""
    import torch
    d = x if isinstance(x, torch.Tensor) else _cuda(x)
    B = d.shape[0]
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fills are done before the ctx stream reads the buffers
    bits = dec.decode_device(d, sigma=sigma, pm=pm, flags=fl) if meta else dec.decode_device(d, sigma=sigma)
    dec.synchronize()
    return _unpack(bits.cpu().numpy(), dec.N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32).astype(np.int64)


def _same_pm(pm, want, dtype, label):
    if dtype == "f32":
        assert np.array_equal(pm.astype(np.float32), want), label
    else:
        assert np.array_equal(pm, want), label


def _check_list(dec, x, ref, dtype, label):
    """a list context against the oracle's (u_hat, pm, ties, stats) on batch x, forwards and reversed"""
    o_uh, o_pm, o_ties, st = ref
    name = dec.kernel_name
    for order in (np.arange(len(x)), np.arange(len(x))[::-1]):
        uh, pm, fl = _fixed(dec, x[order])
        inv = np.argsort(order)
        uh, pm, fl = uh[inv], pm[inv], fl[inv]
        bad = np.flatnonzero((uh != o_uh).any(axis=1))
        assert bad.size == 0, (label, name, "u_hat", bad[:10])
        _same_pm(pm, o_pm, dtype, (label, name, "pm"))
        assert np.array_equal((fl & FLAG_TIE) != 0, o_ties > 0), (label, name, "FLAG_TIE")
        if dtype == "f64":
            if "k_scl_generic" in name:
                assert not (fl & FLAG_RERANK).any(), (label, name)
            else:   # kernels that pre-rank on the metrics' high words
                assert np.array_equal((fl & FLAG_RERANK) != 0, st[:, 0] > 0), (label, name, "FLAG_RERANK")


# ---- list decoders: the list part of tools/stress_parity.py ----------------------------------------------------------------
LIST_SHAPES = []
for _N in (512, 1024, 2048, 4096):
    for _L in (2, 4, 8, 16, 32):
        for _K, _taps in ((_N // 2, CRC24C), (_N // 4, None), (3 * _N // 4, CRC6)):
            if _N == 4096 and _L >= 16 and _K != _N // 2:
                continue
            LIST_SHAPES.append((_N, _K, _L, _taps))
for _N in (32, 64, 128, 256):
    for _L in (1, 2, 8, 32):
        LIST_SHAPES.append((_N, _N // 2, _L, None))


def _list_dec(N, K, L, taps, dtype):
    import polardecoding_amd as pa
    if taps:
        return pa.CASCL(N, K, L=L, crc_taps=taps, dtype=_pa(dtype))
    return pa.SCLdecode(N, K, L=L, dtype=_pa(dtype))


def _frames_for(N, L):
    return 66 if N * L < 32768 else 32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,L,taps", LIST_SHAPES, ids=lambda v: "crc%d" % max(v) if isinstance(v, tuple) else str(v))
def test_list_decoders_match_the_oracle(N, K, L, taps, dtype, oracle):
    dec = _list_dec(N, K, L, taps, dtype)
    code = _code_of(oracle, dec, K, taps)
    B = _frames_for(N, L)
    llr = F.oracle_llr(oracle, code, B, SEED + N + L, 1.5 if K * 2 <= N else 3.5)
    x = _mixed(llr, N + L, dtype)
    algo = "CASCL" if taps else "SCL"
    ref = _oracle(oracle, code, x, algo, L=L, dtype=dtype)
    print(f"KERNEL list {algo} N={N} K={K} L={L} {dtype}: {dec.kernel_name}; frames {B}, with ties {(ref[2] > 0).sum()}, "
          f"with re-rank {(ref[3][:, 0] > 0).sum()}")
    _check_list(dec, x, ref, dtype, f"{algo} N={N} K={K} L={L} {dtype}")
    if N <= 256 and L == 8:   # the spilled generic kernel at small N
        from polardecoding_amd import testing as T
        T.select_kernel(dec, T.KERNEL_GENERIC_SPILL)
        assert "k_scl_generic" in dec.kernel_name
        print(f"KERNEL list spilled N={N} L={L} {dtype}: {dec.kernel_name}")
        _check_list(dec, x, ref, dtype, f"spilled {algo} N={N} L={L} {dtype}")
    dec.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,taps", [(512, CRC24C), (256, None)])
def test_every_selectable_kernel_at_n1024_l8(K, taps, dtype, oracle):
    from polardecoding_amd import testing as T
    N, L, B = 1024, 8, 130
    code = oracle.Code(N, K, taps)
    llr = F.oracle_llr(oracle, code, B, SEED, 2.0)
    x = _mixed(llr, 1024 + K, dtype)
    algo = "CASCL" if taps else "SCL"
    ref = _oracle(oracle, code, x, algo, L=L, dtype=dtype)
    assert (ref[2] > 0).sum() >= B // 4 and (ref[3][:, 0] > 0).sum() >= B // 4
    variants = [("auto", T.KERNEL_AUTO, "k_scl_fast"), ("one_per_wave", T.KERNEL_ONE_PER_WAVE, "k_scl_fast<"),
                ("four_per_wave", T.KERNEL_FOUR_PER_WAVE, "k_scl_fast4"), ("big", T.KERNEL_BIG, "k_scl_big"),
                ("generic", T.KERNEL_GENERIC, "k_scl_generic"), ("generic_spill", T.KERNEL_GENERIC_SPILL, "k_scl_generic")]
    for label, variant, expect in variants:
        dec = _list_dec(N, K, L, taps, dtype)
        T.select_kernel(dec, variant)
        assert expect in dec.kernel_name, (label, dec.kernel_name)
        print(f"KERNEL select {label} {algo} {dtype}: {dec.kernel_name}")
        _check_list(dec, x, ref, dtype, f"{label} {algo} {dtype}")
        dec.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [8, 32])
def test_every_big_split(L, dtype, oracle):
    from polardecoding_amd import testing as T
    N, K, B = 1024, 512, (130 if L == 8 else 24)
    code = oracle.Code(N, K, CRC24C)
    llr = F.oracle_llr(oracle, code, B, SEED + L, 2.0)
    x = _mixed(llr, 77 + L, dtype)
    ref = _oracle(oracle, code, x, "CASCL", L=L, dtype=dtype)
    assert (ref[2] > 0).sum() >= B // 4
    for split in (35, 46, 57, 351, 371):
        dec = _list_dec(N, K, L, CRC24C, dtype)
        T.select_kernel(dec, T.KERNEL_BIG)
        T.big_split(dec, split)
        assert "k_scl_big" in dec.kernel_name
        print(f"KERNEL big split {split} L={L} {dtype}: {dec.kernel_name}")
        _check_list(dec, x, ref, dtype, f"split {split} L={L} {dtype}")
        dec.close()


# ---- SC ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [32, 128, 1024, 2048])
def test_sc_both_kernels_and_a_misaligned_buffer(N, dtype, oracle):
    import torch
    import polardecoding_amd as pa
    K = N // 2
    dec = pa.SCdecode(N, K, dtype=_pa(dtype))
    code = _code_of(oracle, dec, K, None)
    for B in (40, 64 * 5 + 11):   # k_scl_generic below 64 frames, k_sc_lanes from 64 on
        llr = F.oracle_llr(oracle, code, B, SEED + N + B, 2.0)
        x = _mixed(llr, N + B, dtype)
        ref = _oracle(oracle, code, x, "SC", dtype=dtype)[0]
        uh, _, _ = _fixed(dec, x)
        print(f"KERNEL SC N={N} B={B} {dtype}: {dec.kernel_name}")
        assert np.array_equal(uh, ref), (N, B, dtype)
        # the rows one element past a 16-byte boundary: the scalar read path
        flat = torch.empty(B * N + 4, dtype=torch.float32 if dtype == "f32" else torch.float64, device="cuda")
        d = flat[1:1 + B * N].view(B, N)
        d.copy_(_cuda(x))
        assert d.is_contiguous() and d.data_ptr() % 16 != 0
        uh, _, _ = _fixed(dec, d)
        assert np.array_equal(uh, ref), (N, B, dtype, "misaligned")
    assert N != 1024 or "k_sc_lanes" in dec.kernel_name


# ---- SC-Flip ---------------------------------------------------------------------------------------------------------------
def _scf(dec, x, sigma=0.0):
    import torch
    d = _cuda(x)
    B = d.shape[0]
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    at = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_scf_device(d, sigma=sigma, flags=fl, attempts=at)
    dec.synchronize()
    return (_unpack(bits.cpu().numpy(), dec.N), fl.cpu().numpy().view(np.uint32).astype(np.int64),
            at.cpu().numpy().astype(np.int64))


def _same_scf(got, want, label):
    uh, fl, at = got
    bad = np.flatnonzero((uh != want[0]).any(axis=1) | (at != want[2]))
    assert bad.size == 0, (label, "u_hat / attempts differ on frames", bad[:10], len(bad))
    assert np.array_equal(fl, want[1]), label


_SCF_REFS = {}


def _scf_case(oracle, N, K, taps, T, B, dtype):
    """(code, x, scf_model's answer): the frames of the host conditions (seed 5, 1.5 dB) on grid (1, 7) followed by the same
    frames on grid (2, 3), in f64 and in f32; computed when first asked for"""
    key = (N, T, dtype)
    if key not in _SCF_REFS:
        code = oracle.Code(N, K, taps)
        llr = F.oracle_llr(oracle, code, B, SEED, 1.5)
        x = np.concatenate([F.grid(llr, 1.0, 7), F.grid(llr, 2.0, 3)])
        _SCF_REFS[key] = (code, x, scf_model(code, x.astype(_np(dtype)), T, dtype=_np(dtype), oracle=oracle))
    return _SCF_REFS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,taps,T,B", SCF_CASES)
def test_scf_equals_the_model_where_ties_decide(N, K, taps, T, B, dtype, oracle):
    import polardecoding_amd as pa
    code, x, want = _scf_case(oracle, N, K, taps, T, B, dtype)
    dec = pa.SCFlip(N, K, T=T, crc_taps=taps, dtype=_pa(dtype))
    assert np.array_equal(dec.info_order, code.info_order)
    print(f"KERNEL SC-Flip N={N} T={T} {dtype}: {dec.kernel_name}; {len(want[4])} of {len(x)} frames fail attempt 0")
    assert len(want[4]) > 100
    _same_scf(_scf(dec, x.astype(_np(dtype))), want, f"N={N} T={T} {dtype} llr")
    _same_scf(_scf(dec, x), want, f"N={N} T={T} {dtype} f64 input")
    # y with sigma = 1: 2 * y / 1 / 1 is the same grid value
    _same_scf(_scf(dec, x / 2, sigma=1.0), want, f"N={N} T={T} {dtype} y with sigma")


@pytest.mark.parametrize("dtype", DTYPES)
def test_scf_on_every_family(dtype, oracle):
    import polardecoding_amd as pa
    N, K, T = 128, 64, 8
    code = oracle.Code(N, K, CRC6)
    llr = F.oracle_llr(oracle, code, 130, SEED + 1, 1.5)
    dec = pa.SCFlip(N, K, T=T, crc_taps=CRC6, dtype=_pa(dtype))
    x = np.concatenate(list(F.families(llr, SEED, _np(dtype), degenerate=False).values()))
    x = F.plant(x, F.degenerate_rows(N, _np(dtype), SEED, c=2.0))   # 1040 frames: every degenerate row on a wavefront boundary
    want = scf_model(code, x, T, dtype=_np(dtype), oracle=oracle)
    _same_scf(_scf(dec, x), want, f"families {dtype}")


def test_scf_n2048_t32_record_list_with_fewer_waves(oracle):
    import polardecoding_amd as pa
    N, K, T, B = 2048, 1024, 32, 150
    dec = pa.SCFlip(N, K, T=T)
    code = _code_of(oracle, dec, K, CRC24C)
    llr = F.oracle_llr(oracle, code, B, SEED, 1.5)
    x = np.concatenate([F.grid(llr[:B // 2], 1.0, 7), F.grid(llr[B // 2:], 2.0, 3)])
    want = scf_model(code, x, T, oracle=oracle)
    print(f"KERNEL SC-Flip N={N} T={T} f64: {dec.kernel_name}; {len(want[4])} of {B} frames fail attempt 0")
    assert len(want[4]) >= 20
    _same_scf(_scf(dec, x), want, "N=2048 T=32")


# ---- SCAN ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,per", [(128, 64, 70), (1024, 512, 66)])
def test_scan_equals_the_model_on_every_family(N, K, per, dtype, oracle):
    import torch
    import polardecoding_amd as pa
    code = oracle.Code(N, K)
    llr = F.oracle_llr(oracle, code, per, SEED, 1.5)
    fam = F.families(llr, SEED, _np(dtype), degenerate=False)
    x = np.concatenate(list(fam.values()))   # rows are independent: one model run for all families
    x = F.plant(x, F.degenerate_rows(N, _np(dtype), SEED, c=2.0))   # 8 * per frames: every degenerate row on a wavefront boundary
    names = [f"{k}[{b}]" for k in fam for b in range(per)]
    dec = pa.SCAN(N, K, dtype=_pa(dtype))
    ty = torch.float32 if dtype == "f32" else torch.float64
    for I in (1, 4):
        dec.set_scan_iters(I)
        want = scan_model(code.frozen, x, I, dtype=_np(dtype), oracle=oracle, skip=True)
        for B in (len(x), 63, 65):   # the whole batch, and batches on both sides of 64
            d = _cuda(x[:B])
            lu = torch.full((B, N), float("nan"), dtype=ty, device="cuda")
            ex = torch.full((B, N), float("nan"), dtype=ty, device="cuda")
            torch.cuda.synchronize()
            bits = dec.decode_scan_device(d, llr_u=lu, ext_x=ex)
            dec.synchronize()
            uh = _unpack(bits.cpu().numpy(), N)
            bad = np.flatnonzero((uh != want[0][:B]).any(axis=1))
            assert bad.size == 0, (I, dtype, "u_hat", [names[b] for b in bad[:8]])
            for nm, g, w in (("llr_u", lu.cpu().numpy(), want[1][:B]), ("ext_x", ex.cpu().numpy(), want[2][:B])):
                assert g.dtype == w.dtype and not np.isnan(g).any(), (I, dtype, nm)
                assert np.array_equal(np.isinf(g), np.isinf(w)) and not (g == -np.inf).any(), (I, dtype, nm, "infinities")
                bad = np.flatnonzero((g != w).any(axis=1))
                assert bad.size == 0, (I, dtype, nm, [names[b] for b in bad[:8]])
        print(f"KERNEL SCAN N={N} I={I} {dtype}: {dec.kernel_name}")


# ---- BP --------------------------------------------------------------------------------------------------------------------
BP_SHAPES = [(128, 64, 20, "k_bp_w128<"), (1024, 512, 8, "k_bp_r4<"), (512, 256, 11, "k_bp<"), (2048, 1024, 5, "k_bp<")]


def _bp(dec, x):
    import torch
    d = _cuda(x)
    B = d.shape[0]
    it = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_bp_device(d, iters=it, flags=fl)
    dec.synchronize()
    return _unpack(bits.cpu().numpy(), dec.N), it.cpu().numpy().astype(np.int64), fl.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,iters,kname", BP_SHAPES)
def test_bp_fixed_iterations_match_the_oracle(N, K, iters, kname, dtype, oracle):
    import polardecoding_amd as pa
    dec = pa.BP(N, K, iterMax=iters, dtype=_pa(dtype))
    assert dec.kernel_name.startswith(kname), dec.kernel_name
    code = _code_of(oracle, dec, K, None)
    llr = F.oracle_llr(oracle, code, 70, SEED + N, 2.0)
    x = _mixed(llr, N, dtype)
    ref = _oracle(oracle, code, x, "BP", dtype=dtype, iters=iters)[0]
    uh, _, _ = _fixed(dec, x, meta=False)
    print(f"KERNEL BP N={N} it={iters} {dtype}: {dec.kernel_name}")
    bad = np.flatnonzero((uh != ref).any(axis=1))
    assert bad.size == 0, (N, dtype, bad[:10])


@pytest.mark.parametrize("N,K,iters,kname", BP_SHAPES)
def test_bp_stop_rule_g_matches_the_restatement(N, K, iters, kname, oracle):
    import polardecoding_amd as pa
    iter_max = 40
    dec = pa.BP(N, K, iterMax=iter_max, early_stop="g")
    assert dec.kernel_name.startswith(kname) and "stop rule G" in dec.kernel_name
    code = _code_of(oracle, dec, K, None)
    llr = F.oracle_llr(oracle, code, 70, SEED + N, 2.5)
    x = _mixed(llr, N, "f64")
    t_stop, conv, out = stop_points(x, code.frozen, iter_max)
    uh, it, fl = _bp(dec, x)
    print(f"KERNEL BP stop rule N={N} f64: {dec.kernel_name}; converged {conv.sum()} of {len(x)}, iters {np.unique(t_stop)[:8]}")
    assert conv.any() and not conv.all()
    assert np.array_equal(it, t_stop), np.flatnonzero(it != t_stop)[:10]
    assert np.array_equal(fl, np.where(conv, pa.FLAG_BP_CONVERGED, 0))
    assert np.array_equal(uh, out)
    for t in np.unique(it):   # and the oracle's fixed-iteration decoder at the stop point
        sel = it == t
        ref, _, _ = oracle.decode(code, x[sel], "BP", bp_iters=int(t))
        assert np.array_equal(uh[sel], np.atleast_2d(ref)), t
    # f32: the frames that ran t round trips against the f32 oracle with bp_iters = t
    d32 = pa.BP(N, K, iterMax=iter_max, early_stop="g", dtype=pa.F32)
    x32 = x.astype(np.float32)
    uh, it, fl = _bp(d32, x32)
    assert it.min() >= 1 and it.max() <= iter_max and (fl[it < iter_max] == pa.FLAG_BP_CONVERGED).all()
    for t in np.unique(it):
        sel = it == t
        ref, _, _ = oracle.decode(code, x32[sel], "BP", bp_iters=int(t), dtype="f32")
        assert np.array_equal(uh[sel], np.atleast_2d(ref)), ("f32", t)


# ---- adaptive CA-SCL -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,taps,stages,B", [(1024, 512, CRC24C, (1, 8, 32), 130), (128, 64, CRC6, (1, 2, 8), 330)])
def test_adaptive_cascl_matches_the_oracle_composition(N, K, taps, stages, B, dtype, oracle):
    import torch
    import polardecoding_amd as pa
    code = oracle.Code(N, K, taps)
    llr = F.oracle_llr(oracle, code, B, SEED + N, 1.5)
    x = _mixed(llr, N + 1, dtype)
    dec = pa.CASCL(N, K, L=stages[-1], crc_taps=taps, stages=stages, dtype=_pa(dtype))
    print(f"KERNEL adaptive N={N} {stages} {dtype}: {dec.kernel_name}")
    wu, wpm, wfl, wls = _oracle_composition(oracle, code, taps, stages, x, dtype)
    d = _cuda(x)
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ls = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_cascl_device(d, pm=pm, flags=fl, list_size=ls)
    dec.synchronize()
    uh, pm = _unpack(bits.cpu().numpy(), N), pm.cpu().numpy()
    fl, ls = fl.cpu().numpy().view(np.uint32).astype(np.int64), ls.cpu().numpy().astype(np.int64)
    assert np.array_equal(ls, wls), (np.unique(ls, return_counts=True), np.unique(wls, return_counts=True))
    assert np.array_equal(uh, wu)
    _same_pm(pm, wpm.astype(_np(dtype)), dtype, "pm")
    assert np.array_equal(fl & ~FLAG_RERANK, wfl)
    for L in stages:
        assert (ls == L).any(), L


# ---- rate matching -----------------------------------------------------------------------------------------------------------
# N, K, E: puncturing, shortening, repetition with two copies of every position, repetition with three copies of some
RM_CASES = [(1024, 200, 864), (1024, 512, 864), (1024, 400, 2048), (1024, 300, 2500)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,E", RM_CASES)
def test_rate_matched_decoders_on_grid_rows(N, K, E, dtype, oracle):
    import torch
    import polardecoding_amd as pa
    B = 330
    dt = _np(dtype)
    base = _mixed(MC.design_rows(E, B, 0.8, E + 1), E, dtype)           # E-wide rows: sums of copies tie exactly
    perm = RM.channel_perm(E)
    algos = [("SC", lambda kw: pa.SCdecode(N, K, **kw), None), ("CASCL8", lambda kw: pa.CASCL(N, K, L=8, **kw), CRC24C),
             ("SCF8", lambda kw: pa.SCFlip(N, K, T=8, **kw), CRC24C), ("SCAN4", lambda kw: pa.Decoder(N, K, pa.ALGO_SCAN, **kw), None)]
    for label, make, taps in algos:
        want = None
        for ibil in (0, 1):
            dec = make(dict(dtype=_pa(dtype), E=E, ibil=bool(ibil)))
            A = dec.A
            assert dec.rm_mode == RM.mode_of(N, A, E) and np.array_equal(dec.info_order, RM.info_order(N, A, E))
            x = base[:, perm] if ibil else base                  # sent[t] = e[perm[t]]: the same recovered rows either way
            rows = RM.recover(x, N, A, ibil, out_dtype=dt)
            out = torch.full((B, N), 12345.0, dtype=torch.float32 if dtype == "f32" else torch.float64, device="cuda")
            torch.cuda.synchronize()
            dec.rm_recover_device(_cuda(x), out=out)
            dec.synchronize()
            bits = np.uint32 if dtype == "f32" else np.uint64
            assert np.array_equal(out.cpu().numpy().view(bits), rows.view(bits)), (label, E, ibil, "recovery")
            if ibil:
                assert np.array_equal(rows.view(bits), rows0.view(bits))
            rows0 = rows
            if E == 2500 and not ibil:
                mult = np.array([len(range(k, E, N)) for k in range(N)])
                assert mult.max() == 3 and mult.min() == 2
            if want is None:   # the reference on the recovered rows, once per decoder
                code = _code_of(oracle, dec, K, taps)
                if label == "SC":
                    want = (_oracle(oracle, code, rows, "SC", dtype=dtype)[0],)
                elif label == "CASCL8":
                    want = _oracle(oracle, code, rows, "CASCL", L=8, dtype=dtype)
                elif label == "SCF8":
                    want = scf_model(code, rows, 8, dtype=dt, oracle=oracle)
                else:
                    want = scan_model(code.frozen, rows, 4, dtype=dt, oracle=oracle, skip=True)
                print(f"KERNEL rate-matched {label} N={N} K={K} E={E} mode {dec.rm_mode} {dtype}: {dec.kernel_name}")
            tag = (label, E, ibil, dtype)
            if label == "SC":
                assert np.array_equal(_fixed(dec, x)[0], want[0]), tag
            elif label == "CASCL8":
                uh, pm, fl = _fixed(dec, x)
                assert np.array_equal(uh, want[0]), tag
                _same_pm(pm, want[1], dtype, tag)
                assert np.array_equal((fl & FLAG_TIE) != 0, want[2] > 0), tag
            elif label == "SCF8":
                _same_scf(_scf(dec, x), want, tag)
            else:
                ty = torch.float32 if dtype == "f32" else torch.float64
                lu = torch.full((B, N), float("nan"), dtype=ty, device="cuda")
                ex = torch.full((B, N), float("nan"), dtype=ty, device="cuda")
                torch.cuda.synchronize()
                b = dec.decode_scan_device(_cuda(x), llr_u=lu, ext_x=ex)
                dec.synchronize()
                assert np.array_equal(_unpack(b.cpu().numpy(), N), want[0]), tag
                for g, w in ((lu.cpu().numpy(), want[1]), (ex.cpu().numpy(), want[2])):
                    assert not np.isnan(g).any() and np.array_equal(np.isinf(g), np.isinf(w)) and (g == w).all(), tag
            dec.close()


# ---- construction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,B", [(128, 64 * 5 + 37), (1024, 64 * 5 + 10)])
def test_genie_counters_on_grid_rows(N, B, dtype, oracle):
    import torch
    import polardecoding_amd as pa
    dt = _np(dtype)
    x = _mixed(MC.design_rows(N, B, 0.8, 50 + N), N + 2, dtype)
    err, tie, lam, _ = MC.genie_model(oracle, x, dt)
    print(f"KERNEL genie N={N} B={B} {dtype}: err sum {int(err.sum())}, tie sum {int(tie.sum())}, tie min {int(tie.min())} "
          f"max {int(tie.max())}")
    assert not np.isnan(lam).any()
    assert tie.any() and tie.min() != tie.max() and err.any()       # tie[] non-zero and not all equal
    dec = pa.SCdecode(N, N // 2, dtype=_pa(dtype))
    dec.use_torch_stream()
    counts = torch.zeros((2, N), dtype=torch.int64, device="cuda")
    dec.genie_count_device(_cuda(x), counts)
    dec.synchronize()
    got = counts.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[0], err), np.flatnonzero(got[0] != err)[:10]
    assert np.array_equal(got[1], tie), np.flatnonzero(got[1] != tie)[:10]
