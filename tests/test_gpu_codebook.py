"""GPU: code books (include/polar_hip.h, "Code books").  Every comparison is == against the member's own context: rule 4 says a
frame of a code-book call gets what polar_decode_device / polar_list_decode on members[c] return for its row, and those kernels
are already held to the oracle and the models.

Rows are built per member (test_dyn_host.make_frames for a plain or dynamic member; a rate-matched member takes E values of the
same kind: any E values are a valid received row), made exact in the case's dtype and interleaved by a fixed permutation, so
that neighbouring frames have different codes.  The input's row stride is W_max + 5 and every element of a row beyond the
member's width is NaN: a kernel that read one would lose the identity.  B = 16 384 is twice the largest resident grid of a
one-wavefront kernel (32 workgroups x 256 CUs), so wavefronts take several frames of different codes back to back; with the
levels in global scratch the grid is at most 8 x 256, so B = 4096 there.  Every case is computed once and shared."""
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
import test_dyn_host as M  # noqa: E402

F64, F32 = 0, 1
CRC6, CRC24C = X.CRC6, X.CRC24C
EINVAL, ENOKERNEL = -1, -4
NO_CODE = 0x10
NOT_RERANK = 0xFFFFFFFB   # every flag but POLAR_FLAG_RERANK: what rule 4 compares
PAD = 5                   # ld = W_max + PAD
MASK9 = 0b000101          # the identity mask sent by rule 9 of "List output" on half of the CRC member's frames

# book -> (L, B, members); a member is (kind, N, K, taps, E, ibil), kind "sc" | "scl" | "cascl" | "pac"
BOOKS = {
    "mixed": (4, 16384, [("scl", 32, 16, None, None, 0), ("cascl", 64, 32, CRC6, None, 0), ("scl", 128, 64, None, None, 0),
                         ("scl", 32, 2, None, None, 0)]),
    "rm": (8, 16384, [("scl", 32, 8, None, 40, 0), ("scl", 64, 16, None, 44, 1), ("cascl", 64, 16, CRC6, 48, 0),
                      ("scl", 64, 32, None, None, 0)]),
    "dyn": (8, 16384, [("pac", 64, 32, None, None, 0), ("scl", 64, 32, None, None, 0), ("scl", 32, 16, None, None, 0)]),
    "sc": (1, 16384, [("sc", 32, 16, None, None, 0), ("sc", 64, 32, None, None, 0), ("sc", 128, 64, None, None, 0)]),
    "ga": (32, 4096, [("cascl", 1024, 512, CRC24C, None, 0), ("scl", 256, 128, None, None, 0)]),
    "one": (8, 4096, [("cascl", 64, 32, CRC6, None, 0)]),
}


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _member(spec, L, dtype):
    import polardecoding_amd as pa
    kind, N, K, taps, E, ibil = spec
    if kind == "pac":
        return pa.PAC(N, K, L=L, dtype=dtype)
    algo = {"sc": pa.ALGO_SC, "scl": pa.ALGO_SCL, "cascl": pa.ALGO_CASCL}[kind]
    return pa.Decoder(N, K, algo, L=L, crc_taps=taps, dtype=dtype, E=E, ibil=bool(ibil))


def _members(book, dtype):
    L, B, specs = BOOKS[book]
    return [_member(s, L, dtype) for s in specs]


def _close(decs):
    for d in decs:
        d.close()


def _member_rows(dec, spec, Bm, seed, masked=False):
    """[Bm][W] float64 rows of one member: frames of its code at 0 .. 3 dB; a rate-matched member takes the first E values of
    frames of a code of length >= E.  masked: the second half of the frames is sent with MASK9 XORed into u[I[i]], i < r."""
    import polardecoding_amd as pa
    kind, N, K, taps, E, ibil = spec
    dbs = (0.0, 1.0, 2.0, 3.0)
    if E is not None:
        Nw = max(N, 64)
        _, llr = M.make_frames(Nw, np.arange(Nw // 2, Nw), None, Bm, seed, dbs=dbs)
        return np.ascontiguousarray(llr[:, :E]) if E <= Nw else np.concatenate([llr, llr[:, :E - Nw]], axis=1)
    io = dec.info_order
    dyn = pa.dyn_pac(N, io, M.G133) if kind == "pac" else None
    u, llr = M.make_frames(N, io, dyn, Bm, seed, dbs=dbs, crc=taps)
    if masked and taps:
        rng = np.random.default_rng(seed + 1)
        h = Bm // 2
        um = u[h:].copy()
        for i in range(max(taps)):
            um[:, io[i]] ^= (MASK9 >> i) & 1
        sig = 10.0 ** (-np.asarray(dbs)[np.arange(Bm - h) % 4] / 20.0)[:, None]
        y = (1.0 - 2.0 * M.encode(um)) + sig * rng.standard_normal((Bm - h, N))
        llr[h:] = 2.0 * y / sig / sig
    return llr


def _codes(B, Cn, seed=5):
    """code index per frame: every member B / C times (or once more), in a fixed permutation"""
    return np.random.default_rng(seed).permutation(np.arange(B) % Cn).astype(np.int32)


def _np_in(rows, in32):
    return rows.astype(np.float32) if in32 else rows


def _zext(words, NW):
    out = np.zeros(words.shape[:-1] + (NW,), dtype=np.uint32)
    out[..., :words.shape[-1]] = words
    return out


@functools.lru_cache(maxsize=None)
def _case(book, dtype=F64, in32=False, sigma=0.0, want_list=False):
    """One code-book call and the members' own calls on the same rows, as numpy arrays; computed once, never written after.
    Keys: code, rows (the [B][ld] input as float64), got = (bits, pm, flags) and want = the same assembled from the members;
    with want_list: lgot / lwant = (paths, pm, rem, count, flags), and tens = the device tensors of the list call."""
    import torch
    import polardecoding_amd as pa
    L, B, specs = BOOKS[book]
    decs = _members(book, dtype)
    cb = pa.Codebook(decs)
    try:
        Cn, NWm, ld = len(specs), cb.N_max // 32, cb.W_max + PAD
        assert cb.members == [(d.N, d.E, d.A) for d in decs] and cb.L == L and cb.C == Cn and cb.dtype == dtype
        assert cb.kernel_name.startswith("k_scl_book<" + ("float" if dtype == F32 else "double"))
        code = _codes(B, Cn)
        rows = np.full((B, ld), np.nan)
        per = []
        for c, (d, s) in enumerate(zip(decs, specs)):
            f = np.flatnonzero(code == c)
            r = _member_rows(d, s, f.size, 100 + 7 * c + L, masked=want_list)
            if sigma > 0:
                r = r * (sigma * sigma / 2.0)          # the same frames as observations y
            if dtype == F32 or in32:
                r = r.astype(np.float32).astype(np.float64)
            rows[f, :d.E] = r
            per.append((f, r))
        d_in, d_code = _cuda(_np_in(rows, in32)), _cuda(code)
        pm = torch.zeros(B, dtype=torch.float64, device="cuda")
        fl = torch.zeros(B, dtype=torch.int32, device="cuda")
        bits = cb.decode_device(d_in, d_code, sigma=sigma, pm=pm, flags=fl)
        cb.synchronize()
        out = dict(code=code, rows=rows, ld=ld, got=(_u32(bits), pm.cpu().numpy(), _u32(fl)))
        wb, wp, wf = np.zeros((B, NWm), dtype=np.uint32), np.zeros(B), np.zeros(B, dtype=np.uint32)
        if want_list:
            t = cb.decode_list_device(d_in, d_code, sigma=sigma)
            cb.synchronize()
            out["tens"] = t
            out["lgot"] = (_u32(t[0]), t[1].cpu().numpy(), _u32(t[2]), _u32(t[3]), _u32(t[4]))
            lw = (np.zeros((B, L, NWm), dtype=np.uint32), np.zeros((B, L)), np.zeros((B, L), dtype=np.uint32),
                  np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32))
        for d, (f, r) in zip(decs, per):
            m_in = _cuda(_np_in(r, in32))
            mp = torch.zeros(f.size, dtype=torch.float64, device="cuda")
            mf = torch.zeros(f.size, dtype=torch.int32, device="cuda")
            mb = d.decode_device(m_in, sigma=sigma, pm=mp, flags=mf)
            d.synchronize()
            wb[f], wp[f], wf[f] = _zext(_u32(mb), NWm), mp.cpu().numpy(), _u32(mf)
            if want_list:
                ml = d.decode_list_device(m_in, sigma=sigma)
                d.synchronize()
                lw[0][f] = _zext(_u32(ml[0]), NWm)
                for k in (1, 2, 3, 4):
                    lw[k][f] = ml[k].cpu().numpy().view(np.uint32 if k > 1 else np.float64)
        out["want"] = (wb, wp, wf)
        if want_list:
            out["lwant"] = lw
        return out
    finally:
        cb.close()
        _close(decs)


def _same(got, want, B, names, code):
    for g, w, what in zip(got, want, names):
        if what == "flags":
            g, w = g & NOT_RERANK, w & NOT_RERANK
        bad = np.flatnonzero((g != w).reshape(B, -1).any(axis=1))
        assert bad.size == 0, f"{what} differs from frame {bad[0]} on (code {code[bad[0]]}; {bad.size} frames)"


DECODE_CASES = [("mixed", F64, False, 0.0), ("mixed", F32, True, 0.0), ("mixed", F64, True, 0.0), ("rm", F64, False, 0.0),
                ("rm", F32, True, 0.0), ("rm", F64, False, 0.8), ("rm", F32, True, 0.8), ("dyn", F64, False, 0.0),
                ("sc", F64, False, 0.0), ("ga", F64, False, 0.0), ("one", F64, False, 0.0)]


@pytest.mark.parametrize("book,dtype,in32,sigma", DECODE_CASES)
def test_decode_equals_every_members_own_decode(book, dtype, in32, sigma):
    """rule 4 with rule 5's zero words: bits, metric and flags of every frame, mixed lengths back to back in one wavefront,
    stale LDS of a longer previous frame, CRC next to no CRC, recovery in the load stage, SC against k_sc_lanes, the
    global-scratch layout; the NaN tail of every row is never read"""
    c = _case(book, dtype, in32, sigma, book in ("mixed", "rm"))
    B = BOOKS[book][1]
    _same(c["got"], c["want"], B, ("bits", "pm", "flags"), c["code"])
    assert np.isfinite(c["got"][1]).all()
    if book != "sc":
        assert (c["got"][2] & 2).any() == any(s[3] for s in BOOKS[book][2])   # CRC passes exactly where a member has a CRC


@pytest.mark.parametrize("book,dtype,in32,sigma", [k for k in DECODE_CASES if k[0] in ("mixed", "rm")])
def test_list_equals_every_members_own_list(book, dtype, in32, sigma):
    """the list call: all five outputs, padding included, zero words above N_c / 32 in every rank"""
    c = _case(book, dtype, in32, sigma, True)
    _same(c["lgot"], c["lwant"], BOOKS[book][1], ("paths", "pm", "rem", "count", "flags"), c["code"])


def test_rm_members_are_what_the_issue_names():
    """the three bit-selection modes and the interleaver are all in the rate-matching book"""
    import polardecoding_amd as pa
    decs = _members("rm", F64)
    try:
        assert [(d.rm_mode, d.ibil) for d in decs] == [(pa.RM_REPEAT, False), (pa.RM_PUNCTURE, True), (pa.RM_SHORTEN, False),
                                                       (pa.RM_NONE, False)]
    finally:
        _close(decs)


def test_plain_members_against_the_oracle(oracle):
    """the first 16 frames of each plain f64 member of the mixed-N book against the CPU oracle, so that this file does not rest
    on the library alone"""
    c = _case("mixed", F64, False, 0.0, True)
    L, B, specs = BOOKS["mixed"]
    bits, pm, _ = c["got"]
    for k, (kind, N, K, taps, E, ibil) in enumerate(specs):
        if kind != "scl":
            continue
        f = np.flatnonzero(c["code"] == k)[:16]
        uh, rpm, _ = oracle.decode(oracle.Code(N, K), c["rows"][f, :N], "SCL", L=L)
        got = ((bits[f][:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(f.size, -1)[:, :N]
        assert np.array_equal(got, uh) and np.array_equal(pm[f], rpm), (N, K)


def test_select_and_gather_through_the_longest_member():
    """rule 8: polar_list_select / polar_list_gather on the book's list outputs, called on the N_max member, return each
    member's own selection; mask MASK9 was sent by rule 9 of "List output" on half of the CRC member's frames"""
    import torch
    c = _case("mixed", F64, False, 0.0, True)
    L, B, specs = BOOKS["mixed"]
    decs = _members("mixed", F64)
    try:
        big = max(decs, key=lambda d: d.N)
        paths, pm, rem, count, flags = c["tens"]
        masks = _cuda(np.array([0, MASK9], dtype=np.int32))
        idx = big.list_select_device(rem, count, masks)
        rows = [big.list_gather_device(paths, idx[:, m]) for m in (0, 1)]
        big.synchronize()
        idx_h = idx.cpu().numpy()
        for k, d in enumerate(decs):
            f = np.flatnonzero(c["code"] == k)
            sel = torch.from_numpy(f).cuda()
            m_paths = paths[sel][:, :, :d.NW].contiguous()
            m_idx = d.list_select_device(rem[sel].contiguous(), count[sel].contiguous(), masks)
            assert np.array_equal(idx_h[f], m_idx.cpu().numpy()), k
            for m in (0, 1):
                own = d.list_gather_device(m_paths, m_idx[:, m].contiguous())
                d.synchronize()
                assert np.array_equal(_u32(rows[m])[f], _zext(_u32(own), big.NW)), (k, m)
        f = np.flatnonzero(c["code"] == 1)                    # the CRC-6 member: the masked half is found under MASK9
        h = f.size // 2
        # a list of L = 4 words holds a given 6-bit remainder by chance on at most 4 / 64 of the frames; the sent word is
        # in the list far more often than that at 0 .. 3 dB
        assert (idx_h[f[h:], 1] >= 0).mean() > 0.2 and (idx_h[f[:h], 0] >= 0).mean() > 0.2
    finally:
        _close(decs)


def test_c_1024_repeats_one_member():
    """C = 1024, the same member at every index: indices 0, 511 and 1023 give what C = 1 gives"""
    import polardecoding_amd as pa
    c = _case("one", F64, False, 0.0, False)
    L, B, specs = BOOKS["one"]
    decs = _members("one", F64)
    cb = pa.Codebook(decs * 1024)
    try:
        assert cb.C == 1024
        n = 192
        code = np.array([0, 511, 1023] * (n // 3), dtype=np.int32)
        rows = c["rows"][:n]
        bits = cb.decode_device(_cuda(rows), _cuda(code))
        cb.synchronize()
        assert np.array_equal(_u32(bits), c["got"][0][:n])
    finally:
        cb.close()
        _close(decs)


def test_misaligned_input_and_destroyed_members():
    """d_in one element off a 16-byte boundary gives the same result, and so does a code book whose members were destroyed
    right after it was made (rule 2)"""
    import torch
    import polardecoding_amd as pa
    c = _case("rm", F32, True, 0.0, True)
    L, B, specs = BOOKS["rm"]
    decs = _members("rm", F32)
    cb = pa.Codebook(decs)
    _close(decs)
    try:
        n = 1024
        flat = torch.empty(n * c["ld"] + 1, dtype=torch.float32, device="cuda")
        d_in = flat[1:].view(n, c["ld"])
        d_in.copy_(_cuda(c["rows"][:n].astype(np.float32)))
        assert d_in.data_ptr() % 16 == 4
        pm = torch.zeros(n, dtype=torch.float64, device="cuda")
        fl = torch.zeros(n, dtype=torch.int32, device="cuda")
        bits = cb.decode_device(d_in, _cuda(c["code"][:n]), pm=pm, flags=fl)
        cb.synchronize()
        _same((_u32(bits), pm.cpu().numpy(), _u32(fl)), [w[:n] for w in c["got"]], n, ("bits", "pm", "flags"), c["code"])
    finally:
        cb.close()


def test_bad_index():
    """rule 6: frames with code = C and 0xFFFFFFFF get exactly the stated outputs, their neighbours are unaffected, the call
    returns POLAR_OK and the stream synchronises clean"""
    import torch
    import polardecoding_amd as pa
    c = _case("mixed", F64, False, 0.0, True)
    L, B, specs = BOOKS["mixed"]
    n = 512
    code = c["code"][:n].copy()
    bad = np.array([0, 7, 8, 255, 300, n - 1])
    code[bad[::2]] = len(specs)
    code[bad[1::2]] = -1                                        # 0xFFFFFFFF
    good = np.setdiff1d(np.arange(n), bad)
    decs = _members("mixed", F64)
    cb = pa.Codebook(decs)
    try:
        d_in, d_code = _cuda(c["rows"][:n]), _cuda(code)
        pm = torch.zeros(n, dtype=torch.float64, device="cuda")
        fl = torch.zeros(n, dtype=torch.int32, device="cuda")
        bits = cb.decode_device(d_in, d_code, pm=pm, flags=fl)
        lst = cb.decode_list_device(d_in, d_code)
        cb.synchronize()
        torch.cuda.synchronize()
        bits, pm, fl = _u32(bits), pm.cpu().numpy(), _u32(fl)
        assert (bits[bad] == 0).all() and np.isposinf(pm[bad]).all() and (fl[bad] == NO_CODE).all()
        _same((bits[good], pm[good], fl[good]), [w[:n][good] for w in c["got"]], good.size, ("bits", "pm", "flags"), code[good])
        paths, lpm, rem, count, lfl = _u32(lst[0]), lst[1].cpu().numpy(), _u32(lst[2]), _u32(lst[3]), _u32(lst[4])
        assert (paths[bad] == 0).all() and np.isposinf(lpm[bad]).all() and (rem[bad] == 0).all()
        assert (count[bad] == 0).all() and (lfl[bad] == NO_CODE).all()
        _same((paths[good], lpm[good], rem[good], count[good], lfl[good]), [w[:n][good] for w in c["lgot"]], good.size,
              ("paths", "pm", "rem", "count", "flags"), code[good])
    finally:
        cb.close()
        _close(decs)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
def test_output_extents(B):
    """rule 5: guard words (tests/extents.py) around every output of both device calls at ragged batches, every output NULL
    in turn, and all outputs NULL is POLAR_EINVAL"""
    import torch
    import polardecoding_amd as pa
    c = _case("mixed", F64, False, 0.0, True)
    L, _, specs = BOOKS["mixed"]
    decs = _members("mixed", F64)
    cb = pa.Codebook(decs)
    try:
        NW = cb.NW
        d_in, d_code = _cuda(c["rows"][:B]), _cuda(c["code"][:B])
        lib, h = cb._lib, cb._h
        dec_outs = (("bits", "uint32", NW), ("pm", "float64", 1), ("flags", "uint32", 1))
        lst_outs = (("paths", "uint32", L * NW), ("pm", "float64", L), ("rem", "uint32", L), ("count", "uint32", 1),
                    ("flags", "uint32", 1))
        for outs, fn, ref in ((dec_outs, lib.polar_codebook_decode, c["got"]), (lst_outs, lib.polar_codebook_list_decode, c["lgot"])):
            for null in [None] + [o[0] for o in outs]:
                a = X.Arena("torch", capacity=X.Arena.need([(dt, B * per, 2, per) for _, dt, per in outs]))
                views = [a.carve(nm, dt, B * per, 2, per) if nm != null else None for nm, dt, per in outs]
                rc = fn(h, _p(d_in), 0, c["ld"], _p(d_code), 0.0, B, *[_p(v) for v in views])
                cb.synchronize()
                assert rc == 0 and a.check() == [], (null, rc, a.check())
                for v, w in zip(views, ref):
                    if v is not None:
                        assert np.array_equal(v.cpu().numpy().view(w.dtype).reshape(w[:B].shape), w[:B]), null
            assert fn(h, _p(d_in), 0, c["ld"], _p(d_code), 0.0, B, *([None] * len(outs))) == EINVAL
    finally:
        cb.close()
        _close(decs)


def test_host_form_equals_the_device_form():
    import polardecoding_amd as pa
    c = _case("mixed", F64, False, 0.0, True)
    n = 300
    decs = _members("mixed", F64)
    cb = pa.Codebook(decs)
    try:
        rows = np.nan_to_num(c["rows"][:n], nan=0.0)            # a host array of doubles; the tail is still never read
        uh, pm, fl = cb.decode_batch(rows, c["code"][:n].view(np.uint32))
        bits, wpm, wfl = c["got"]
        want = ((bits[:n][:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, -1)
        assert np.array_equal(uh, want) and np.array_equal(pm, wpm[:n]) and np.array_equal(fl, wfl[:n])
    finally:
        cb.close()
        _close(decs)


def test_graph_capture():
    """rule 7: after one warm-up call a decode is captured on the code book's stream and replayed twice"""
    import torch
    import polardecoding_amd as pa
    c = _case("mixed", F64, False, 0.0, True)
    L, B, specs = BOOKS["mixed"]
    decs = _members("mixed", F64)
    cb = pa.Codebook(decs)
    try:
        d_in, d_code = _cuda(c["rows"]), _cuda(c["code"])
        bits = torch.zeros((B, cb.NW), dtype=torch.int32, device="cuda")
        pm = torch.zeros(B, dtype=torch.float64, device="cuda")
        fl = torch.zeros(B, dtype=torch.int32, device="cuda")

        def call():
            cb.use_torch_stream()
            cb.decode_device(d_in, d_code, out_bits=bits, pm=pm, flags=fl)

        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            call()                                                # warm-up
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                call()
            for t in (bits, pm, fl):
                t.zero_()
            for _ in range(2):
                g.replay()
            stream.synchronize()
        _same((_u32(bits), pm.cpu().numpy(), _u32(fl)), c["got"], B, ("bits", "pm", "flags"), c["code"])
        del g
    finally:
        cb.close()
        _close(decs)


def test_refusals_leave_the_members_usable():
    """rule 9, each refusal followed by one good decode on the same members"""
    import torch
    import polardecoding_amd as pa
    c = _case("mixed", F64, False, 0.0, True)
    L, _, specs = BOOKS["mixed"]
    decs = _members("mixed", F64)
    n = 64
    d_in, d_code = _cuda(c["rows"][:n]), _cuda(c["code"][:n])

    def good():
        cb = pa.Codebook(decs)
        try:
            bits = cb.decode_device(d_in, d_code)
            cb.synchronize()
            assert np.array_equal(_u32(bits), c["got"][0][:n])
        finally:
            cb.close()

    def refused(members, rc=EINVAL):
        lib = decs[0]._lib
        arr = (C.c_void_p * len(members))(*[m._h.value if m is not None else None for m in members])
        h = C.c_void_p(1)
        assert lib.polar_codebook_create(arr, len(members), C.byref(h)) == rc and not h.value
        good()

    others = {
        "dtype": lambda: pa.SCLdecode(64, 32, L=L, dtype=pa.F32),
        "L": lambda: pa.SCLdecode(64, 32, L=2 * L),
        "sc with list": lambda: pa.SCdecode(64, 32),
        "bp": lambda: pa.BP(64, 32, iterMax=4),
        "q8": lambda: pa.SCLdecode(64, 32, L=L, dtype=pa.Q8),
        "systematic": lambda: pa.Decoder(64, 32, pa.ALGO_SCL, L=L, sys_polar=True),
        "stages": lambda: pa.CASCL(64, 32, L=L, crc_taps=CRC6, stages=(1, L)),
        "long": lambda: pa.SCLdecode(2048, 1024, L=L),
    }
    try:
        refused(decs[:1] + [None])
        for what, make in others.items():
            o = make()
            try:
                refused(decs + [o], ENOKERNEL if what == "long" else EINVAL)
            finally:
                o.close()
        wide = [pa.SCLdecode(64, 32, L=64)]
        try:
            refused(wide)
        finally:
            _close(wide)
        cb = pa.Codebook(decs)
        try:
            lib, h = cb._lib, cb._h
            bits = torch.zeros((n, cb.NW), dtype=torch.int32, device="cuda")
            args = lambda ld, B, p_in=d_in.data_ptr(): (h, C.c_void_p(p_in), 0, ld, _p(d_code), 0.0, B, _p(bits), None, None)  # noqa: E731
            assert lib.polar_codebook_decode(*args(cb.W_max - 1, n)) == EINVAL
            assert lib.polar_codebook_decode(*args(c["ld"], 1 << 31)) == EINVAL
            assert lib.polar_codebook_decode(*args(c["ld"], n, d_in.data_ptr() + 4)) == EINVAL
            assert lib.polar_codebook_decode(*args(c["ld"], 0)) == 0 and not bits.any()
            assert lib.polar_codebook_decode(*args(c["ld"], n)) == 0
            cb.synchronize()
            assert np.array_equal(_u32(bits), c["got"][0][:n])
        finally:
            cb.close()
    finally:
        _close(decs)
