"""GPU: list output (include/polar_hip.h, "List output") against the numpy model of tests/list_model.py, everything by ==.

The shapes are the smallest at which each mechanism first exists: N = 32 (the whole history in the register h0, S = 16 lanes
per path, tied grid rows so that the slot tie-break of rule 3 runs), K = 2 (the list never fills: padding), N = 64 with L = 32
(S = 2, history words in LDS, a CRC), PAC(64, 32) (a dynamic context), L = 64 and 128 (the wide kernel, the ranking inside one
wavefront and across two), a rate-matched context, and N = 1024, K = 512, CRC-24C, L = 8, where the ordinary decode is the pair
kernel and rule 5 ties the two together.  Then the extents of every output at ragged batches, NULL outputs, the host form,
masked selection with the transmit convention of rule 9, soft output in both domains, and the refusals."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import extents as X  # noqa: E402
import list_model as LM  # noqa: E402
import llr_families as F  # noqa: E402
import test_dyn_host as M  # noqa: E402

F64, F32 = 0, 1
CRC6, CRC24C = X.CRC6, X.CRC24C
EINVAL, ENOKERNEL = -1, -4
FLAG_RERANK_MASK = 0xFFFFFFFB  # every flag but POLAR_FLAG_RERANK: what rule 5 compares


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# name -> (kind, N, K, L, taps, dtype, B); kind "plain" | "pac" | "rm"
CASES = {
    "n32-l4-f64": ("plain", 32, 16, 4, None, F64, 32),
    "n32-l4-f32": ("plain", 32, 16, 4, None, F32, 32),
    "n32-k2-l8": ("plain", 32, 2, 8, None, F64, 16),
    "n64-crc6-l32": ("plain", 64, 32, 32, CRC6, F64, 32),
    "n64-crc6-l32-f32": ("plain", 64, 32, 32, CRC6, F32, 16),
    "pac64-l8": ("pac", 64, 32, 8, None, F64, 32),
    "wide-n128-l64": ("plain", 128, 64, 64, None, F64, 16),
    "wide-n64-l128": ("plain", 64, 32, 128, CRC6, F32, 16),
    "wide-pac64-l64": ("pac", 64, 32, 64, None, F64, 8),
    "rm-n64-e48-crc6-l8": ("rm", 64, 16, 8, CRC6, F64, 32),
}


def _decoder(name):
    import polardecoding_amd as pa
    kind, N, K, L, taps, dtype, B = CASES[name]
    if kind == "pac":
        return pa.PAC(N, K, L=L, dtype=dtype)
    algo = pa.ALGO_CASCL if taps else pa.ALGO_SCL
    return pa.Decoder(N, K, algo, L=L, crc_taps=taps, dtype=dtype, E=48 if kind == "rm" else None)


def _case_code(name):
    """(information positions in the library's order, dyn) of a case, from the host helpers alone"""
    import polardecoding_amd as pa
    kind, N, K, L, taps, dtype, B = CASES[name]
    A = K + (max(taps) if taps else 0)
    if kind == "pac":
        io = pa.pac_info_order(N, K, "rm")
        return io, pa.dyn_pac(N, io, M.G133)
    if kind == "rm":
        return np.asarray(pa.rm_info_order(N, A, 48), dtype=np.int32), None
    return np.asarray(pa.q_sequence(N)[N - A:], dtype=np.int32), None


def _case_rows(name):
    """([B][width] float64 rows exact in the case's dtype: half AWGN, a quarter on a grid and a quarter of one magnitude, where
    metrics tie; dyn; positions)"""
    kind, N, K, L, taps, dtype, B = CASES[name]
    io, dyn = _case_code(name)
    _, llr = M.make_frames(N, io, dyn, B, 7 + N + L, dbs=(0.0, 1.0, 2.0, 3.0), crc=taps)
    llr[B // 2:] = F.grid(llr[B // 2:], 1.0, 7)
    llr[3 * B // 4:] = F.hard(llr[3 * B // 4:], 1.0)
    if kind == "rm":
        llr = llr[:, :48]                    # any E values are a valid received row
    if dtype == F32:
        llr = llr.astype(np.float32).astype(np.float64)
    return llr, dyn, io


def _run(dec, rows, dtype, **want):
    """decode_list_device on host rows -> numpy (paths [B][L][N], pm, rem, count, flags) and the device tensors"""
    d_in = _cuda(rows.astype(np.float32) if dtype == F32 else rows)
    t = dec.decode_list_device(d_in, **want)
    dec.synchronize()
    paths, pm, rem, count, flags = t
    out = (LM.unpack(paths.cpu().numpy(), dec.N) if paths is not None else None, pm.cpu().numpy() if pm is not None else None,
           _u32(rem) if rem is not None else None, _u32(count) if count is not None else None,
           _u32(flags) if flags is not None else None)
    return out, t, d_in


@functools.lru_cache(maxsize=None)
def _case(name):
    """(rows, N-wide rows the model read, dyn, device result, device tensors, model result, ordinary decode) of a case,
    computed once and shared by the tests; nothing in it is written afterwards"""
    import torch
    kind, N, K, L, taps, dtype, B = CASES[name]
    dec = _decoder(name)
    try:
        rows, dyn, io = _case_rows(name)
        assert np.array_equal(dec.info_order, io)
        got, tens, d_in = _run(dec, rows, dtype)
        wide = rows
        if kind == "rm":
            wide = dec.rm_recover_device(d_in).cpu().numpy().astype(np.float64)
        pm = torch.zeros(B, dtype=torch.float64, device="cuda")
        fl = torch.zeros(B, dtype=torch.int32, device="cuda")
        bits = dec.decode_device(d_in, pm=pm, flags=fl)
        dec.synchronize()
        plain = (LM.unpack(bits.cpu().numpy(), N), pm.cpu().numpy(), _u32(fl))
        frozen = np.ones(N, dtype=np.uint8)
        frozen[dec.info_order] = 0
        want = LM.list_model(frozen, dyn, wide, L, crc=(dec.info_order, taps) if taps else None,
                             dtype=np.float32 if dtype == F32 else np.float64)
        return dict(rows=rows, dyn=dyn, got=got, tens=tens, want=want, plain=plain, kernel=dec.kernel_name)
    finally:
        dec.close()


@pytest.mark.parametrize("name", list(CASES))
def test_list_equals_the_model(name):
    kind, N, K, L, taps, dtype, B = CASES[name]
    c = _case(name)
    for g, w, what in zip(c["got"], c["want"], ("paths", "pm", "rem", "count", "flags")):
        bad = np.flatnonzero((g != w).reshape(B, -1).any(axis=1))
        assert bad.size == 0, f"{what} differs from frame {bad[0]} on ({bad.size} frames)"
    paths, pm, rem, count, flags = c["got"]
    act = int(count[0])
    assert act == min(L, 1 << K if K < 20 else L)
    # rule 3 padding, stated again on the device output
    assert np.isposinf(pm[:, act:]).all() and not paths[:, act:].any() and not rem[:, act:].any()
    # the rows tie: two live slots of one frame with equal PM, so the slot tie-break decided an order (not at K = 2: the four
    # paths of a frame differ in bits that thirty positions repeat, and no two metrics of these rows coincide)
    if name != "n32-k2-l8":
        assert (pm[:, :act - 1] == pm[:, 1:act]).any()
    if kind == "pac":
        assert paths[:, 0][:, c["dyn"][0]].any(), "bits at dynamic positions are b, not 0"
    if taps:
        assert (flags & 2).any() and (rem[:, :act] != 0).any()
    assert ("k_scl_wide<" in c["kernel"]) == (L > 32)


@pytest.mark.parametrize("name", list(CASES))
def test_rule5_identity_with_the_ordinary_decode(name):
    kind, N, K, L, taps, dtype, B = CASES[name]
    c = _case(name)
    paths, pm, rem, count, flags = c["got"]
    u, p_pm, p_fl = c["plain"]
    ks = LM.kstar(rem, count, taps is not None)
    f = np.arange(B)
    assert np.array_equal(paths[f, ks], u) and np.array_equal(pm[f, ks], p_pm)
    assert np.array_equal(flags, p_fl & FLAG_RERANK_MASK)


def test_list_never_fills_at_k2():
    paths, pm, rem, count, flags = _case("n32-k2-l8")["got"]
    assert (count == 4).all() and np.isfinite(pm[:, :4]).all() and np.isposinf(pm[:, 4:]).all()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_n1024_against_the_pair_kernel_and_the_model(dtype):
    """N = 1024, K = 512, CRC-24C, L = 8: rule 5 against decode_device (k_scl_fast2) on 48 AWGN rows at 1.5 dB and 16 tied
    rows, and 8 frames (4 + 4) against the model"""
    import polardecoding_amd as pa
    import torch
    from oracle import oracle_py as O
    N, K, L, B = 1024, 512, 8, 64
    code = O.Code(N, K, CRC24C)
    rows = F.oracle_llr(O, code, B, 21, 1.5)
    rows[48:] = F.grid(rows[48:], 1.0, 7)
    if dtype == F32:
        rows = rows.astype(np.float32).astype(np.float64)
    dec = pa.CASCL(N, K, L=L, dtype=dtype)
    try:
        assert "k_scl_fast2<" in dec.kernel_name
        (paths, pm, rem, count, flags), _, d_in = _run(dec, rows, dtype)
        p_pm = torch.zeros(B, dtype=torch.float64, device="cuda")
        p_fl = torch.zeros(B, dtype=torch.int32, device="cuda")
        bits = dec.decode_device(d_in, pm=p_pm, flags=p_fl)
        dec.synchronize()
        io = dec.info_order
    finally:
        dec.close()
    ks = LM.kstar(rem, count, True)
    f = np.arange(B)
    assert np.array_equal(paths[f, ks], LM.unpack(bits.cpu().numpy(), N))
    assert np.array_equal(pm[f, ks], p_pm.cpu().numpy())
    assert np.array_equal(flags, _u32(p_fl) & FLAG_RERANK_MASK)
    assert (flags & 2).any() and (flags & 1).any()                        # frames that pass the CRC, frames with a median tie
    pick = np.r_[0:4, 48:52]
    frozen = np.ones(N, dtype=np.uint8)
    frozen[io] = 0
    want = LM.list_model(frozen, None, rows[pick], L, crc=(io, CRC24C), dtype=np.float32 if dtype == F32 else np.float64)
    for g, w in zip((paths, pm, rem, count, flags), want):
        assert np.array_equal(g[pick], w)


def test_systematic_context_keeps_rule5():
    """polar_set_systematic: the remainders are those of tab_sys, and k* is still the ordinary decode's choice"""
    import polardecoding_amd as pa
    import torch
    N, K, L, B = 64, 32, 8, 32
    dec = pa.CASCL(N, K, L=L, crc_taps=CRC6, sys_polar=True)
    try:
        _, rows = M.make_frames(N, dec.info_order, None, B, 5, crc=CRC6)
        (paths, pm, rem, count, flags), _, d_in = _run(dec, rows, F64)
        p_pm = torch.zeros(B, dtype=torch.float64, device="cuda")
        p_fl = torch.zeros(B, dtype=torch.int32, device="cuda")
        bits = dec.decode_device(d_in, pm=p_pm, flags=p_fl)
        dec.synchronize()
    finally:
        dec.close()
    ks = LM.kstar(rem, count, True)
    f = np.arange(B)
    assert np.array_equal(paths[f, ks], LM.unpack(bits.cpu().numpy(), N)) and np.array_equal(pm[f, ks], p_pm.cpu().numpy())
    assert np.array_equal(flags, _u32(p_fl) & FLAG_RERANK_MASK) and (flags & 2).any() and (ks > 0).any()


@pytest.mark.parametrize("name", ["n64-crc6-l32", "wide-n64-l128", "wide-pac64-l64"])
def test_global_scratch_variant_gives_the_same_list(name):
    """the GA instantiations (LLR levels in global scratch: what N = 1024 with L = 32 in f64 runs), forced at a small shape"""
    from polardecoding_amd import testing as T
    c = _case(name)
    dec = T.select_kernel(_decoder(name), T.KERNEL_GENERIC_SPILL)
    try:
        got, _, _ = _run(dec, c["rows"], CASES[name][5])
    finally:
        dec.close()
    for g, w in zip(got, c["got"]):
        assert np.array_equal(g, w)


def test_rate_matched_rows_across_a_chunk_boundary():
    """the recovered rows go through ctx scratch in chunks: with a cap of a few rows per pass the outputs of every pass land at
    their own offsets"""
    from polardecoding_amd import testing as T
    name = "rm-n64-e48-crc6-l8"
    c = _case(name)
    dec = _decoder(name)
    try:
        T.chunk_bytes(dec, 3 * 64 * 8)
        rows = np.tile(c["rows"], (3, 1))                                  # 96 rows: the least chunk is 64 rows
        got, _, _ = _run(dec, rows, F64)
    finally:
        dec.close()
    for g, w in zip(got, c["got"]):
        assert np.array_equal(g, np.tile(w, (3,) + (1,) * (w.ndim - 1)))


# ---- extents: guard words around every output, ragged batches, a second call, NULL outputs ------------------------------------
LIST_OUTS = (("d_paths", "uint32", "LNW"), ("d_pm", "float64", "L"), ("d_rem", "uint32", "L"), ("d_count", "uint32", 1),
             ("d_flags", "uint32", 1))


def _arena(outs, dims, B):
    specs = [(dt, (per if isinstance(per, int) else dims[per]) * B, 2, per if isinstance(per, int) else dims[per]) for _, dt, per in outs]
    arena = X.Arena("torch", X.Arena.need(specs))
    return arena, {name: arena.carve(name, *s) for (name, _, _), s in zip(outs, specs)}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("name", ["n32-l4-f64", "n64-crc6-l32", "wide-n64-l128", "rm-n64-e48-crc6-l8"])
def test_ragged_batches_stay_inside_their_outputs(name):
    import torch
    kind, N, K, L, taps, dtype, _ = CASES[name]
    dec = _decoder(name)
    try:
        dims = {"LNW": L * N // 32, "L": L}
        rows67 = np.tile(_case_rows(name)[0], (5, 1))[:67]
        for B in (1, 67, 1):                                            # the third pass: a second call at the first size
            rows = rows67[:B]
            want, _, d_in = _run(dec, rows, dtype)
            snap = X.snapshot(d_in)
            arena, v = _arena(LIST_OUTS, dims, B)
            rc = dec._lib.polar_list_decode(dec._h, _ptr(d_in), int(dtype == F32), 0.0, B, *[_ptr(v[n]) for n, _, _ in LIST_OUTS])
            dec.synchronize()
            torch.cuda.synchronize()
            assert rc == 0 and arena.check() == [] and X.unchanged(d_in, snap), (name, B)
            got = (LM.unpack(v["d_paths"].cpu().numpy().reshape(B, L, N // 32), N), v["d_pm"].cpu().numpy().reshape(B, L),
                   _u32(v["d_rem"]).reshape(B, L), _u32(v["d_count"]), _u32(v["d_flags"]))
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (name, B)
            # every output alone, the others NULL: the same values, nothing else written
            for k, (n, _, _) in enumerate(LIST_OUTS):
                arena, v = _arena(LIST_OUTS, dims, B)
                args = [_ptr(v[m]) if m == n else None for m, _, _ in LIST_OUTS]
                rc = dec._lib.polar_list_decode(dec._h, _ptr(d_in), int(dtype == F32), 0.0, B, *args)
                dec.synchronize()
                assert rc == 0 and arena.check() == [], (name, B, n)
                h = arena.host()
                for m, _, _ in LIST_OUTS:
                    _, _, start, end, _ = arena.span(m)
                    if m != n:
                        assert (h[start:end] == X.FILL).all(), (name, B, n, m)
                one = v[n].cpu().numpy()
                ref = (want[0], want[1], want[2], want[3], want[4])[k]
                if n == "d_paths":
                    one = LM.unpack(one.reshape(B, L, N // 32), N)
                assert np.array_equal(one.view(ref.dtype).reshape(ref.shape) if n != "d_paths" else one, ref), (name, B, n)
        assert dec._lib.polar_list_decode(dec._h, _ptr(d_in), int(dtype == F32), 0.0, 1, None, None, None, None, None) == EINVAL
    finally:
        dec.close()


def test_list_kernels_stay_inside_their_outputs():
    """polar_list_select, polar_list_gather and polar_list_soft at B = 1 and 67 with guards around their
    outputs, against the model"""
    import torch
    name = "n64-crc6-l32"
    kind, N, K, L, taps, dtype, _ = CASES[name]
    dec = _decoder(name)
    try:
        rows67 = np.tile(_case_rows(name)[0], (3, 1))[:67]
        masks = np.array([0, 5, 63], dtype=np.int32)
        for B in (1, 67):
            (paths, pm, rem, count, flags), (t_paths, t_pm, t_rem, t_count, _), _ = _run(dec, rows67[:B], dtype)
            outs = (("d_idx", "int32", 3), ("d_uhat_bits", "uint32", N // 32), ("d_out", "float64", N))
            arena, v = _arena(outs, {}, B)
            lib, h = dec._lib, dec._h
            assert lib.polar_list_select(h, _ptr(t_rem), _ptr(t_count), B, _ptr(_cuda(masks)), 3, _ptr(v["d_idx"])) == 0
            assert lib.polar_list_gather(h, _ptr(t_paths), C.c_void_p(v["d_idx"].data_ptr() + 4), 3, B, _ptr(v["d_uhat_bits"])) == 0
            assert lib.polar_list_soft(h, _ptr(t_paths), _ptr(t_pm), _ptr(t_count), _ptr(t_rem), 5, 1, 16.0, B, _ptr(v["d_out"])) == 0
            dec.synchronize()
            torch.cuda.synchronize()
            assert arena.check() == [], B
            idx = v["d_idx"].cpu().numpy().reshape(B, 3)
            assert np.array_equal(idx, LM.select(rem, count, masks))
            assert np.array_equal(LM.unpack(v["d_uhat_bits"].cpu().numpy().reshape(B, N // 32), N), LM.gather(paths, idx[:, 1]))
            assert np.array_equal(v["d_out"].cpu().numpy().reshape(B, N), LM.soft(paths, pm, count, rem, 5, 1, 16.0))
    finally:
        dec.close()


def test_host_form_equals_the_device_form():
    name = "n64-crc6-l32"
    dec = _decoder(name)
    try:
        rows = _case(name)["rows"][:3]
        got = dec.decode_list_batch(rows)
    finally:
        dec.close()
    for g, w in zip(got, _case(name)["got"]):
        assert np.array_equal(g, w[:3])


def test_graph_capture_of_the_whole_chain():
    """rule 7: list decode, select, gather and soft output read nothing back; after a warm-up at the same B the four calls are
    captured into one graph and replayed"""
    import torch
    name = "n64-crc6-l32"
    kind, N, K, L, taps, dtype, B = CASES[name]
    c = _case(name)
    paths, pm, rem, count, flags = c["got"]
    dec = _decoder(name)
    try:
        d_in = _cuda(c["rows"])
        i32 = dict(dtype=torch.int32, device="cuda")
        t = dict(paths=torch.zeros((B, L, N // 32), **i32), pm=torch.zeros((B, L), dtype=torch.float64, device="cuda"),
                 rem=torch.zeros((B, L), **i32), count=torch.zeros(B, **i32), flags=torch.zeros(B, **i32),
                 idx=torch.zeros((B, 1), **i32), row=torch.zeros((B, N // 32), **i32),
                 soft=torch.zeros((B, N), dtype=torch.float64, device="cuda"), masks=torch.zeros(1, **i32))
        lib, h = dec._lib, dec._h

        def chain():
            dec.use_torch_stream()
            rc = [lib.polar_list_decode(h, _ptr(d_in), 0, 0.0, B, _ptr(t["paths"]), _ptr(t["pm"]), _ptr(t["rem"]),
                                               _ptr(t["count"]), _ptr(t["flags"])),
                  lib.polar_list_select(h, _ptr(t["rem"]), _ptr(t["count"]), B, _ptr(t["masks"]), 1, _ptr(t["idx"])),
                  lib.polar_list_gather(h, _ptr(t["paths"]), _ptr(t["idx"]), 1, B, _ptr(t["row"])),
                  lib.polar_list_soft(h, _ptr(t["paths"]), _ptr(t["pm"]), _ptr(t["count"]), _ptr(t["rem"]), 0, 1, 32.0, B,
                                             _ptr(t["soft"]))]
            assert rc == [0, 0, 0, 0], rc

        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            chain()                                                       # warm-up at the same B
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                chain()
            for k in ("paths", "pm", "rem", "count", "flags", "idx", "row", "soft"):
                t[k].zero_()
            for _ in range(2):
                g.replay()
            stream.synchronize()
        assert np.array_equal(LM.unpack(t["paths"].cpu().numpy(), N), paths) and np.array_equal(t["pm"].cpu().numpy(), pm)
        assert np.array_equal(_u32(t["rem"]), rem) and np.array_equal(_u32(t["count"]), count) and np.array_equal(_u32(t["flags"]), flags)
        assert np.array_equal(LM.unpack(t["row"].cpu().numpy(), N), c["plain"][0])
        assert np.array_equal(t["soft"].cpu().numpy(), LM.soft(paths, pm, count, rem, 0, 1, 32.0))
        del g
    finally:
        dec.close()


# ---- masked-CRC selection --------------------------------------------------------------------------------------------------------
def test_mask_zero_reproduces_the_ca_scl_choice():
    import polardecoding_amd as pa
    for name in ("n64-crc6-l32", "wide-n64-l128"):
        kind, N, K, L, taps, dtype, B = CASES[name]
        c = _case(name)
        paths, pm, rem, count, flags = c["got"]
        t_paths, _, t_rem, t_count, _ = c["tens"]
        dec = _decoder(name)
        try:
            idx = dec.list_select_device(t_rem, t_count, _cuda(np.zeros(1, dtype=np.int32)))
            bits = dec.list_gather_device(t_paths, idx[:, 0])
            dec.synchronize()
        finally:
            dec.close()
        idx = idx.cpu().numpy()[:, 0]
        passed = (flags & 2) != 0
        assert passed.any() and not passed.all()
        assert np.array_equal(idx[passed], LM.kstar(rem, count, True)[passed]) and (idx[~passed] == -1).all()
        assert np.array_equal(LM.unpack(bits.cpu().numpy(), N), c["plain"][0])       # -1 -> rank 0: the ordinary decode's row


@pytest.mark.parametrize("crc_systematic", [False, True], ids=["crc-nonsys", "crc-sys"])
def test_blind_detection_with_three_masks(crc_systematic):
    """rule 9: frames sent with mask m_2 XORed into u[I[i]], i < r, at high SNR select m_2 and give -1 for the other masks
    (24 CRC bits: a chance match of one of the other 7 list members is 2^-21 per frame), and the gathered row's payload is
    the sent one in both CRC conventions"""
    import polardecoding_amd as pa
    N, K, L, B, r = 128, 64, 8, 16, 24
    masks = np.array([0x00A5A5A5, 0x00123456, 0x00FEDCBA], dtype=np.int32)
    rng = np.random.default_rng(9)
    dec = pa.CASCL(N, K, L=L, crc_taps=CRC24C, systematic=crc_systematic)
    try:
        payload = rng.integers(0, 2, (B, K)).astype(np.int32)
        u, _ = dec.encode_batch(payload)
        io = dec.info_order
        for i in range(r):
            u[:, io[i]] ^= (int(masks[1]) >> i) & 1
        x = M.encode(u)
        rows = 8.0 * (1.0 - 2.0 * x) + 0.5 * rng.standard_normal((B, N))
        (paths, pm, rem, count, flags), (t_paths, _, t_rem, t_count, _), _ = _run(dec, rows, F64)
        idx = dec.list_select_device(t_rem, t_count, _cuda(masks))
        row = dec.list_gather_device(t_paths, idx[:, 1])
        pay, ok = dec.payload_device(row)
        absent = dec.list_select_device(t_rem, t_count, _cuda(np.array([0x01000000, 0x00A5A5A5], dtype=np.int32)))
        dec.synchronize()
    finally:
        dec.close()
    idx = idx.cpu().numpy()
    assert np.array_equal(idx, LM.select(rem, count, masks))
    assert (idx[:, 1] >= 0).all() and (idx[:, 0] == -1).all() and (idx[:, 2] == -1).all()
    assert np.array_equal(LM.unpack(row.cpu().numpy(), N), u)
    got = LM.unpack(pay.cpu().numpy(), ((K + 31) // 32) * 32)[:, :K]
    assert np.array_equal(got, payload) and not ok.cpu().numpy().any()
    assert not (flags & 2).any()                                          # no list member has remainder 0
    assert (absent.cpu().numpy() == -1).all()                             # a bit at crc_r matches nothing; neither does an absent mask


def test_padding_is_never_selected():
    c = _case("n32-k2-l8")
    _, _, t_rem, t_count, _ = c["tens"]
    dec = _decoder("n32-k2-l8")
    try:
        idx = dec.list_select_device(t_rem, t_count, _cuda(np.array([0, 1], dtype=np.int32)))
        dec.synchronize()
    finally:
        dec.close()
    idx = idx.cpu().numpy()
    assert (idx[:, 0] == 0).all() and (idx[:, 1] == -1).all()            # rem is 0 everywhere, padding included: rank 0, never 4..7
    import torch
    dec = _decoder("n32-k2-l8")
    try:
        none = dec.list_select_device(t_rem, torch.zeros_like(t_count), _cuda(np.array([0], dtype=np.int32)))
        dec.synchronize()
    finally:
        dec.close()
    assert (none.cpu().numpy() == -1).all()


# ---- soft output -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n32-l4-f64", "n64-crc6-l32", "wide-n64-l128", "n32-k2-l8"])
@pytest.mark.parametrize("domain", [0, 1], ids=["u", "x"])
def test_soft_output_equals_the_model(name, domain):
    kind, N, K, L, taps, dtype, B = CASES[name]
    c = _case(name)
    paths, pm, rem, count, flags = c["got"]
    t_paths, t_pm, t_rem, t_count, _ = c["tens"]
    present = int(rem[0, 1]) if taps else 0
    dec = _decoder(name)
    try:
        outs = [(dec.list_soft_device(t_paths, t_pm, t_count, domain=domain, clamp=512.0), (None, 0)),
                (dec.list_soft_device(t_paths, t_pm, t_count, rem=t_rem, want_rem=0, domain=domain, clamp=512.0), (rem, 0)),
                (dec.list_soft_device(t_paths, t_pm, t_count, rem=t_rem, want_rem=present, domain=domain, clamp=0.75), (rem, present)),
                (dec.list_soft_device(t_paths, t_pm, t_count, rem=t_rem, want_rem=0x40, domain=domain, clamp=512.0), (rem, 0x40))]
        dec.synchronize()
    finally:
        dec.close()
    clamps = (512.0, 512.0, 0.75, 512.0)
    for (t, (r_, w_)), cl in zip(outs, clamps):
        assert np.array_equal(t.cpu().numpy(), LM.soft(paths, pm, count, r_, w_, domain, cl))
    s = outs[0][0].cpu().numpy()
    assert (np.abs(s) < 512.0).any()                                      # a position with both values present
    if domain == 0:
        assert (s[:, 0] == 512.0).all()                                    # all paths agree: u_0 is frozen in every case, no path has a 1
    assert np.array_equal(outs[3][0].cpu().numpy(), s)                    # 0x40 is no 6-bit remainder: the fallback to all ranks
    assert (np.abs(outs[2][0].cpu().numpy()) <= 0.75).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(dec, code):
    import torch
    B, L, NW, N = 2, max(dec.L, 1), dec.NW, dec.N
    d_in = torch.zeros((B, dec.E), dtype=torch.float64, device="cuda")
    paths = torch.zeros((B, L, NW), dtype=torch.int32, device="cuda")
    pm = torch.zeros((B, L), dtype=torch.float64, device="cuda")
    rem = torch.zeros((B, L), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros((B, N), dtype=torch.float64, device="cuda")
    lib, h = dec._lib, dec._h
    assert lib.polar_list_decode(h, _ptr(d_in), 0, 0.0, B, _ptr(paths), _ptr(pm), _ptr(rem), _ptr(cnt), None) == code
    assert lib.polar_list_select(h, _ptr(rem), _ptr(cnt), B, _ptr(cnt), 1, _ptr(rem)) == code
    assert lib.polar_list_gather(h, _ptr(paths), _ptr(cnt), 1, B, _ptr(paths)) == code
    assert lib.polar_list_soft(h, _ptr(paths), _ptr(pm), _ptr(cnt), None, 0, 0, 1.0, B, _ptr(out)) == code
    host, hpm = np.zeros((B, dec.E)), np.zeros((B, L))
    dp = C.POINTER(C.c_double)
    assert lib.polar_list_decode_host(h, host.ctypes.data_as(dp), B, None, hpm.ctypes.data_as(dp), None, None, None) == code
    # the context still decodes
    bits = dec.decode_device(d_in + 1.0)
    dec.synchronize()
    assert not bits.cpu().numpy().any()


@pytest.mark.parametrize("kind", ["SC", "BP", "SCF", "SCAN", "BPL", "Q8", "staged", "N2048"])
def test_refusals_leave_the_context_usable(kind):
    import polardecoding_amd as pa
    make = {"SC": lambda: pa.SCdecode(64, 32), "BP": lambda: pa.BP(64, 32, iterMax=4), "SCF": lambda: pa.SCFlip(64, 32, crc_taps=CRC6),
            "SCAN": lambda: pa.SCAN(64, 32), "BPL": lambda: pa.BPL(64, 32, iterMax=4),
            "Q8": lambda: pa.CASCL(64, 26, L=8, crc_taps=CRC6, dtype=pa.Q8),
            "staged": lambda: pa.CASCL(64, 26, L=8, crc_taps=CRC6, stages=(2, 8)),
            "N2048": lambda: pa.SCLdecode(2048, 1024, L=2)}[kind]
    dec = make()
    try:
        _refused(dec, ENOKERNEL if kind == "N2048" else EINVAL)
        if kind == "staged":                                             # the rule is a state, not a property: without it the list is there
            dec.set_cascl_stages(None)
            assert dec.decode_list_batch(np.ones((1, 64)))[3][0] == 8
    finally:
        dec.close()


def test_bad_arguments():
    import torch
    name = "n32-l4-f64"
    c = _case(name)
    t_paths, t_pm, t_rem, t_count, _ = c["tens"]
    dec = _decoder(name)
    try:
        lib, h, B = dec._lib, dec._h, t_count.shape[0]
        out = torch.zeros((B, 32), dtype=torch.float64, device="cuda")
        for clamp in (0.0, -1.0, float("inf"), float("nan")):
            assert lib.polar_list_soft(h, _ptr(t_paths), _ptr(t_pm), _ptr(t_count), None, 0, 0, clamp, B, _ptr(out)) == EINVAL
        assert lib.polar_list_soft(h, _ptr(t_paths), _ptr(t_pm), _ptr(t_count), None, 0, 2, 1.0, B, _ptr(out)) == EINVAL
        for Mn in (0, 65):
            assert lib.polar_list_select(h, _ptr(t_rem), _ptr(t_count), B, _ptr(t_rem), Mn, _ptr(out)) == EINVAL
        assert lib.polar_list_gather(h, _ptr(t_paths), _ptr(t_count), 0, B, _ptr(out)) == EINVAL
        again, _, _ = _run(dec, c["rows"], F64)                            # and it still works
        for g, w in zip(again, c["got"]):
            assert np.array_equal(g, w)
    finally:
        dec.close()
