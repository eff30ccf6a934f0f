"""GPU: every kernel that forms or checks a CRC against its model on the single-bit frames of tests/crc_cases.py, for the
polynomial family r = 1, 6, 11, 16, 24, 25, 31, 32.  Every comparison is == against the reference.

Frame i of a case carries a word whose CRC remainder is exactly 1 << i (tests/test_crc_cases_host.py holds that and what the
references do with it): a kernel that loses remainder bit i -- a mask row skipped, a shift by 32, a 31-bit compare -- returns
the flipped word where the reference returns the sent one, or reports POLAR_FLAG_CRC_PASS where the reference clears it.  A
case has B = r frames: odd batches and idle half-wavefronts.  The decoders: k_scl_fast2 (LLR and y form), k_scl_fast,
k_scl_fast4, k_scl_big, k_scl_generic (LDS-resident and spilled), k_scl_dyn, k_scl_wide, k_scl_q8, the list output and its
masked selection, a code book, k_scf_lanes (static and dynamic), k_ad_crc_check behind adaptive CA-SCL (N = 4096: two words
per lane) and behind BP list decoding.  The encoder side (k_place, k_extract) runs for every polynomial with plain and
systematic CRC at K = 1, A = N, K < r, K a multiple of 32 and N = 4096, against tests/test_encode_host.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import crc_cases as CC  # noqa: E402
import list_model as LM  # noqa: E402
import test_encode_host as E  # noqa: E402
from test_gpu_llr_families import _cuda, _fixed, _pa, _same_scf, _scf, _unpack  # noqa: E402

KEEP = CC.FLAG_TIE | CC.FLAG_CRC_PASS


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same_list(got, want, dtype, rerank, label):
    """(u_hat, pm, flags) of decode_device against crc_cases.ref_list; rerank: None (not compared), False (the kernel never
    sets it) or True (from the oracle's counts, f64 only)"""
    uh, pm, fl = got
    w_uh, w_pm, w_fl, w_rr = want
    bad = np.flatnonzero((uh != w_uh).any(axis=1))
    assert bad.size == 0, (label, "u_hat differs on frames (= remainder bits)", bad.tolist())
    if dtype == "f32":
        assert np.array_equal(pm.astype(np.float32), w_pm), (label, "pm")
    else:
        assert np.array_equal(pm, w_pm), (label, "pm")
    assert np.array_equal(fl & KEEP, w_fl), (label, "TIE / CRC_PASS", np.flatnonzero((fl & KEEP) != w_fl).tolist())
    if dtype == "f64" and rerank is not None:
        assert np.array_equal((fl & CC.FLAG_RERANK) != 0, w_rr if rerank else np.zeros_like(w_rr)), (label, "RERANK")


# ---- the list decoders behind polar_decode_device --------------------------------------------------------------------------
@pytest.mark.parametrize("case,r,dtype", CC.list_case_ids(), ids=lambda v: v.label if isinstance(v, tuple) else str(v))
def test_list_kernel_sees_every_remainder_bit(case, r, dtype, oracle):
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    N, K, L = case.N, case.K, case.L
    code = CC.code_of(N, K, r)
    dec = pa.CASCL(N, K, L=L, crc_taps=CC.POLYS[r], dtype=_pa(dtype))
    try:
        if case.variant:
            T.select_kernel(dec, getattr(T, case.variant))
        assert case.kernel in dec.kernel_name, dec.kernel_name
        assert np.array_equal(dec.info_order, code.info_order)
        weak = CC.frames(N, K, r)[3].astype(CC.np_dtype(dtype))
        want = CC.ref_list(N, K, r, L, dtype)
        rerank = None if "k_scl_wide" in case.kernel else "k_scl_generic" not in case.kernel
        for form in case.forms:
            got = _fixed(dec, weak) if form == "llr" else _fixed(dec, CC.y_of(weak).astype(weak.dtype), sigma=CC.SIGMA)
            _same_list(got, want, dtype, rerank, f"{case.label} r={r} {dtype} {form} {dec.kernel_name}")
    finally:
        dec.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("r", CC.DYN_RS)
def test_dyn_kernel_sees_every_remainder_bit(r, dtype, oracle):
    import polardecoding_amd as pa
    io, dyn, _ = CC.dyn_code(r)
    dec = pa.PCCASCL(CC.DYN_N, CC.DYN_K, n_pc=CC.DYN_NPC, L=CC.DYN_L, crc_taps=CC.POLYS[r], dtype=_pa(dtype))
    try:
        assert "k_scl_dyn<" in dec.kernel_name and np.array_equal(dec.info_order, io)
        assert np.array_equal(dec.dyn_positions, dyn[0])
        w_uh, w_pm, w_fl = CC.ref_dyn(r, dtype)
        uh, pm, fl = _fixed(dec, CC.dyn_frames(r)[3].astype(CC.np_dtype(dtype)))
        bad = np.flatnonzero((uh != w_uh).any(axis=1))
        assert bad.size == 0, ("u_hat differs on frames", bad.tolist())
        assert np.array_equal(pm, w_pm) and np.array_equal(fl & KEEP, w_fl)
    finally:
        dec.close()


@pytest.mark.parametrize("r", CC.Q8_RS)
@pytest.mark.parametrize("N,K,L", CC.Q8_SHAPES)
def test_q8_kernel_sees_every_remainder_bit(N, K, L, r, oracle):
    import torch
    import polardecoding_amd as pa
    code = CC.code_of(N, K, r)
    dec = pa.CASCL(N, K, L=L, crc_taps=CC.POLYS[r], dtype=pa.Q8)
    try:
        assert "k_scl_q8<" in dec.kernel_name and np.array_equal(dec.info_order, code.info_order)
        q = CC.q8_of(CC.frames(N, K, r)[3])
        pm = torch.full((r,), -1, dtype=torch.int32, device="cuda")
        fl = torch.full((r,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        bits = dec.decode_q8_device(_cuda(q), pm=pm, flags=fl)
        dec.synchronize()
        w_uh, w_pm, w_fl = CC.ref_q8(N, K, r, L)
        uh = _unpack(bits.cpu().numpy(), N)
        bad = np.flatnonzero((uh != w_uh).any(axis=1))
        assert bad.size == 0, ("u_hat differs on frames", bad.tolist())
        assert np.array_equal(pm.cpu().numpy(), w_pm) and np.array_equal(_u32(fl), w_fl)
    finally:
        dec.close()


# ---- list output: the one place where the remainder's value is visible ----------------------------------------------------
def _list_outputs(dec, rows):
    t = dec.decode_list_device(_cuda(rows))
    dec.synchronize()
    return (LM.unpack(t[0].cpu().numpy(), dec.N), t[1].cpu().numpy(), _u32(t[2]), _u32(t[3]), _u32(t[4])), t


@pytest.mark.parametrize("N,K,L", CC.PATHS_SHAPES)
def test_list_output_and_masked_selection(N, K, L, oracle):
    import polardecoding_amd as pa
    for r in CC.fits(N, K):
        code = CC.code_of(N, K, r)
        u, uf, _, weak = CC.frames(N, K, r)
        dec = pa.CASCL(N, K, L=L, crc_taps=CC.POLYS[r])
        try:
            assert np.array_equal(dec.info_order, code.info_order)
            got, tens = _list_outputs(dec, weak)
            want = CC.ref_all_paths(N, K, r, L)
            for g, w, what in zip(got, want, ("paths", "pm", "rem", "count", "flags")):
                bad = np.flatnonzero((g != w).reshape(r, -1).any(axis=1))
                assert bad.size == 0, (N, r, what, "differs on frames", bad.tolist())
            paths, pm, rem, count, flags = got
            bit = (np.uint64(1) << np.arange(r, dtype=np.uint64)).astype(np.uint32)
            at = (paths == uf[:, None, :]).all(axis=2)                      # the rank that holds u'
            assert (at.sum(axis=1) == 1).all() and np.array_equal(rem[at], bit)
            # masks [0, 1 << 0, .., 1 << (r-1)] in one call: column 1 + i of frame i must be the rank of u', column 0 that of u
            masks = np.concatenate([[0], bit]).astype(np.uint32)
            idx = dec.list_select_device(tens[2], tens[3], _cuda(masks.view(np.int32)))
            dec.synchronize()
            idx = idx.cpu().numpy()
            assert np.array_equal(idx, LM.select(rem, count, masks)), (N, r)
            f = np.arange(r)
            assert np.array_equal(idx[f, 1 + f], at.argmax(axis=1))
            has_u = (paths == u[:, None, :]).all(axis=2)
            assert np.array_equal(idx[:, 0], np.where(has_u.any(axis=1), has_u.argmax(axis=1), -1)) and 2 * has_u.any(axis=1).sum() >= r
        finally:
            dec.close()


def test_code_book_list_equals_its_members_own_lists(oracle):
    """N = 64 with CRC-11 and N = 128 with CRC-32 in one launch, frames interleaved"""
    import polardecoding_amd as pa
    decs = [pa.CASCL(N, K, L=L, crc_taps=CC.POLYS[r]) for N, K, L, r in CC.BOOK_MEMBERS]
    cb = pa.Codebook(decs)
    try:
        assert cb.kernel_name.startswith("k_scl_book<double") and cb.C == 2
        NWm = cb.N_max // 32
        sizes = [r for _, _, _, r in CC.BOOK_MEMBERS]
        code = np.random.default_rng(5).permutation(np.repeat(np.arange(2), sizes)).astype(np.int32)
        B = code.size
        rows = np.full((B, cb.W_max), np.nan)
        want = (np.zeros((B, 8, NWm), dtype=np.uint32), np.zeros((B, 8)), np.zeros((B, 8), dtype=np.uint32),
                np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32))
        for c, (d, (N, K, L, r)) in enumerate(zip(decs, CC.BOOK_MEMBERS)):
            f = np.flatnonzero(code == c)
            weak = CC.frames(N, K, r)[3]
            rows[f, :N] = weak
            ml = d.decode_list_device(_cuda(weak))
            d.synchronize()
            want[0][f, :, :N // 32] = _u32(ml[0])
            for k in (1, 2, 3, 4):
                want[k][f] = ml[k].cpu().numpy().view(np.uint32 if k > 1 else np.float64)
            # and the members' own lists are the model's
            own = (LM.unpack(ml[0].cpu().numpy(), N), want[1][f], want[2][f], want[3][f], want[4][f])
            for g, w in zip(own, CC.ref_all_paths(N, K, r, L)):
                assert np.array_equal(g, w)
        t = cb.decode_list_device(_cuda(rows), _cuda(code))
        cb.synchronize()
        got = (_u32(t[0]), t[1].cpu().numpy(), _u32(t[2]), _u32(t[3]), _u32(t[4]))
        for g, w, what in zip(got, want, ("paths", "pm", "rem", "count", "flags")):
            if what == "flags":
                g, w = g & ~np.uint32(CC.FLAG_RERANK), w & ~np.uint32(CC.FLAG_RERANK)
            bad = np.flatnonzero((g != w).reshape(B, -1).any(axis=1))
            assert bad.size == 0, (what, "differs on frames", bad.tolist(), code[bad].tolist())
    finally:
        cb.close()
        for d in decs:
            d.close()


# ---- kernels whose first pass is SC: plain rows -----------------------------------------------------------------------------
@pytest.mark.parametrize("r", CC.SCF_RS)
def test_scf_lanes_static_and_dynamic(r, oracle):
    import polardecoding_amd as pa
    from test_gpu_dscf import _dscf, _same
    N, K = CC.SCF_N, CC.SCF_K
    code = CC.code_of(N, K, r)
    plain = CC.frames(N, K, r)[2]
    dec = pa.SCFlip(N, K, T=CC.SCF_T, crc_taps=CC.POLYS[r])
    try:
        assert "k_scf_lanes<" in dec.kernel_name and np.array_equal(dec.info_order, code.info_order)
        want = CC.ref_scf(N, K, r, CC.SCF_T)
        got = _scf(dec, plain)
        _same_scf(got, want, f"static r={r}")
        assert (got[2] >= 1).all() and len(want[4]) == r, "attempt 0 failed in every frame"
        dec.set_scf_flips(0)                         # SC plus the CRC flag: the verdict on u' itself
        uh, fl, at = _scf(dec, plain)
        assert np.array_equal(uh, CC.frames(N, K, r)[1]) and not fl.any() and not at.any()
    finally:
        dec.close()
    dec = pa.DSCFlip(N, K, budgets=CC.SCF_BUDGETS, c=CC.SCF_C, tau=CC.SCF_TAU, crc_taps=CC.POLYS[r])
    try:
        assert "k_scf_lanes<" in dec.kernel_name
        got = _dscf(dec, plain)
        _same(got, CC.ref_dscf(N, K, r, CC.SCF_BUDGETS), f"dynamic r={r}")
        assert (got[2] >= 1).all(), "attempt 0 failed in every frame"
    finally:
        dec.close()


ADAPTIVE = [(N, K, st, r) for N, K, st, rs in CC.ADAPTIVE_CASES for r in CC.fits(N, K, rs)]


@pytest.mark.parametrize("N,K,stages,r", ADAPTIVE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_adaptive_crc_check_sees_every_remainder_bit(N, K, stages, r, oracle):
    import polardecoding_amd as pa
    from test_gpu_cascl_adaptive import _adaptive, _same
    code = CC.code_of(N, K, r)
    dec = pa.CASCL(N, K, L=stages[-1], crc_taps=CC.POLYS[r], stages=stages)
    try:
        assert "k_ad_crc_check" in dec.kernel_name and np.array_equal(dec.info_order, code.info_order)
        want = CC.ref_adaptive(N, K, r, stages)
        got = _adaptive(dec, CC.frames(N, K, r)[2])
        assert (got[3] == stages[-1]).all(), "stage 1 failed the CRC in every frame"
        _same(got, want, f"N={N} r={r}")
    finally:
        dec.close()


def test_bpl_crc_check_at_r32(oracle):
    import polardecoding_amd as pa
    from test_gpu_bpl import _bpl, _of_model, _same
    N, K, r, iters, P = CC.BPL_CASE
    code = CC.code_of(N, K, r)
    dec = pa.BPL(N, K, iterMax=iters, graphs=P, crc_taps=CC.POLYS[r])
    try:
        assert "CRC-aided" in dec.kernel_name and np.array_equal(dec.info_order, code.info_order)
        got = _bpl(dec, CC.frames(N, K, r)[2])
        _same(got, _of_model(CC.ref_bpl(N, K, r, iters, P)), "BPL r=32")
        assert (got[3] >= 1).all(), "graph 0 converged to u' and failed the CRC in every frame"
    finally:
        dec.close()


# ---- the encoder side -------------------------------------------------------------------------------------------------------
def _words(bits):
    return _cuda(E.pack(bits).view(np.int32))


def _bits(t, n):
    return E.unpack(t.cpu().numpy().view(np.uint32), n)


def _enc_decoder(N, K, r, crc_sys):
    import polardecoding_amd as pa
    return pa.CASCL(N, K, L=2, crc_taps=CC.POLYS[r], systematic=crc_sys)


@pytest.mark.parametrize("crc_sys", [False, True], ids=["plain", "syscrc"])
@pytest.mark.parametrize("r", CC.ALL_R)
def test_encode_and_payload_equal_the_model(r, crc_sys):
    taps = CC.POLYS[r]
    for N, K in CC.enc_shapes(r):
        dec = _enc_decoder(N, K, r, crc_sys)
        try:
            info = dec.info_order
            assert np.array_equal(info, CC.enc_info(N, K + r))
            for B in CC.ENC_BS:
                label = (r, crc_sys, N, K, B)
                v = np.random.default_rng([r, N, K, B]).integers(0, 2, (B, K)).astype(np.uint8)
                w = E.pack(v).copy()
                if K % 32:   # garbage above bit K in the last payload word must be ignored
                    w[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(K % 32)
                want_u = E.place(v, N, info, taps, crc_sys)
                want_x = E.transform(want_u)
                d_u, d_x = dec.encode_device(_cuda(w.view(np.int32)))
                d_back, d_ok = dec.payload_device(d_u)
                dec.synchronize()
                assert np.array_equal(_bits(d_u, N), want_u), label
                assert np.array_equal(_bits(d_x, N), want_x), label
                assert np.array_equal(_u32(d_back), E.pack(v)), label        # bit for bit, zero at and above K
                assert (d_ok.cpu().numpy() == 1).all(), label
                # one flipped bit among the first r information positions: remainder 1 << i
                bad_u = want_u.copy()
                bad_u[np.arange(B), info[np.arange(B) % r]] ^= 1
                want_v, want_ok = E.extract(bad_u, info, taps, crc_sys)
                d_back, d_ok = dec.payload_device(_words(bad_u))
                dec.synchronize()
                assert not want_ok.any() and np.array_equal(_u32(d_ok), want_ok), label
                assert np.array_equal(_u32(d_back), E.pack(np.ascontiguousarray(want_v))), label
        finally:
            dec.close()


PAYLOAD_SHAPES = sorted({(N, K, r) for (N, K, _), rs in CC.weak_shapes().items() for r in rs} |
                        {(N, K, r) for (N, K), rs in CC.plain_shapes().items() for r in rs})


@pytest.mark.parametrize("crc_sys", [False, True], ids=["plain", "syscrc"])
def test_payload_of_the_single_bit_words(crc_sys, oracle):
    """polar_payload_device on the words of the decoder cases: crc_ok = 1 on u, 0 on u' in every frame (remainder 1 << i), the
    payload the model's"""
    for N, K, r in PAYLOAD_SHAPES:
        taps = CC.POLYS[r]
        dec = _enc_decoder(N, K, r, crc_sys)
        try:
            info = dec.info_order
            u, uf = CC.frames(N, K, r)[:2]
            assert np.array_equal(info, CC.code_of(N, K, r).info_order)
            for words, ok in ((u, 1), (uf, 0)):
                want_v, want_ok = E.extract(words, info, taps, crc_sys)
                d_back, d_ok = dec.payload_device(_words(words))
                dec.synchronize()
                assert (want_ok == ok).all() and np.array_equal(_u32(d_ok), want_ok), (N, K, r, ok)
                assert np.array_equal(_u32(d_back), E.pack(np.ascontiguousarray(want_v))), (N, K, r, ok)
        finally:
            dec.close()


@pytest.mark.parametrize("crc_sys", [False, True], ids=["plain", "syscrc"])
def test_round_trip_with_the_generator_at_r32(crc_sys):
    """generate_device at 60 dB, payload_device, encode_device: the generator's own CRC-32 words come back bit for bit"""
    import torch
    import polardecoding_amd as pa
    N, K, B = 128, 33, 65
    dec = pa.CASCL(N, K, L=8, crc_taps=CC.POLYS[32], systematic=crc_sys)
    try:
        y = torch.empty((B, N), dtype=torch.float64, device="cuda")
        u_bits = torch.empty((B, dec.NW), dtype=torch.int32, device="cuda")
        dec.generate_device(11, 0, 60.0, y, u_bits=u_bits, out_is_y=True)
        d_pay, d_ok = dec.payload_device(u_bits)
        d_u, d_x = dec.encode_device(d_pay)
        dec.synchronize()
        assert (d_ok.cpu().numpy() == 1).all() and d_pay.cpu().numpy().any()
        assert np.array_equal(d_u.cpu().numpy(), u_bits.cpu().numpy())
        assert np.array_equal(_bits(d_x, N), (y.cpu().numpy() < 0).astype(np.uint8))
        want_v, want_ok = E.extract(_bits(u_bits, N), dec.info_order, CC.POLYS[32], crc_sys)
        assert want_ok.all() and np.array_equal(_u32(d_pay), E.pack(np.ascontiguousarray(want_v)))
    finally:
        dec.close()
