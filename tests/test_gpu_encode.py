"""GPU: the encoder side (k_transform, k_place, k_extract, k_dyn_fill, k_rm_select, k_count_sys) and systematic polar mode
against the numpy models of tests/test_encode_host.py, bit for bit.

B is 1, 65 or 300: no launch is a whole number of workgroups.  N = 32 is one word (in-word stages only), 64 the first stage
across lanes, 4096 the size with two words per lane.  The generator (k_generate and its rate-matched and dynamic forms) is the
oracle that is independent of the new code: at 60 dB no sign of y can differ from the sent bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_dyn_host as D  # noqa: E402
import test_encode_host as M  # noqa: E402
import test_rm_host as R  # noqa: E402

F64, F32 = 0, 1
FLAG_CRC_PASS = 0x2
CRC32 = (0, 1, 2, 4, 5, 7, 8, 10, 11, 12, 16, 22, 23, 26, 32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _tsync():
    """torch fills and copies run on torch's stream, the library on the context's own: order them"""
    import torch
    torch.cuda.synchronize()


def _words(bits):
    """rows of 0/1 -> int32 CUDA tensor of packed words"""
    return _cuda(M.pack(bits).view(np.int32))


def _bits(t, n):
    return M.unpack(t.cpu().numpy().view(np.uint32), n)


def _taps(dec):
    return tuple(int(t) for t in dec._cfg_keep[0]) if dec._cfg.n_taps else None


def _make(name):
    """a decoder of the named test code and its dynamic constraints (or None)"""
    import polardecoding_amd as pa
    if name == "sc32":
        return pa.SCdecode(32, 13), None
    if name == "cascl128":
        return pa.CASCL(128, 64, L=8, crc_taps=pa.CRC6_TAPS), None
    if name == "cascl128-syscrc":
        return pa.CASCL(128, 64, L=8, crc_taps=pa.CRC6_TAPS, systematic=True), None
    if name == "cascl1024":
        return pa.CASCL(1024, 500, L=8, crc_taps=pa.CRC24C_TAPS), None
    if name == "cascl128-crc32":   # r = 32: the tap-32 branch, a shift by a whole word
        return pa.CASCL(128, 33, L=8, crc_taps=CRC32), None
    if name == "cascl1024-syscrc":
        return pa.CASCL(1024, 500, L=8, crc_taps=pa.CRC24C_TAPS, systematic=True), None
    if name == "scl4096":
        return pa.SCLdecode(4096, 2048, L=2), None
    if name == "pac128":
        io = pa.pac_info_order(128, 64, "rm")
        dyn = pa.dyn_pac(128, io, D.G133)
        return pa.Decoder(128, 64, pa.ALGO_SCL, L=8, info_order=io, dyn=dyn), dyn
    if name == "pc64":
        q = pa.q_sequence(64)
        pos, sets, io = pa.dyn_pc5g(64, q[64 - 23:], 3, 0)
        return pa.Decoder(64, 14, pa.ALGO_CASCL, L=8, crc_taps=pa.CRC6_TAPS, info_order=io, dyn=(pos, sets)), (pos, sets)
    if name == "rm-repeat":      # E = 160 at N = 128
        dec = pa.Decoder(128, 40, pa.ALGO_SC, E=160)
        assert dec.rm_mode == pa.RM_REPEAT
        return dec, None
    if name == "rm-puncture":    # 16 A <= 7 E
        dec = pa.Decoder(128, 40, pa.ALGO_SC, E=100, ibil=True)
        assert dec.rm_mode == pa.RM_PUNCTURE
        return dec, None
    if name == "rm-shorten":     # A = 64 + 6 = 70
        dec = pa.Decoder(128, 64, pa.ALGO_CASCL, L=8, crc_taps=pa.CRC6_TAPS, E=100)
        assert dec.rm_mode == pa.RM_SHORTEN and dec.A == 70
        return dec, None
    raise ValueError(name)


def _model(dec, dyn, v, sys_polar=False):
    """(u [B][N], sent bits [B][E]) of payload rows v for the code of `dec`"""
    import polardecoding_amd as pa
    info = dec.info_order
    z = M.place(v, dec.N, info, _taps(dec), dec.systematic)
    if dyn is not None:
        z = D.fill_dynamic(z.astype(np.int64), dyn).astype(np.uint8)
    if sys_polar:
        return M.sys_encode(z, info)
    x = M.transform(z)
    if dec.rm_mode != pa.RM_NONE:
        x = R.transmit(x, dec.E, dec.A, dec.ibil)
    return z, x


def _payload(dec, B, seed):
    """random payload rows and their packed words, with garbage above bit K in the last word (it must be ignored)"""
    v = np.random.default_rng(seed).integers(0, 2, (B, dec.K)).astype(np.uint8)
    w = M.pack(v).copy()
    if dec.K % 32:
        w[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(dec.K % 32)
    return v, _cuda(w.view(np.int32))


# ---- transform ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 65, 300])
@pytest.mark.parametrize("N", [32, 64, 1024, 4096])
def test_transform_equals_the_model(N, B):
    import polardecoding_amd as pa
    dec = pa.SCdecode(N, N // 2)
    u = np.random.default_rng(N + B).integers(0, 2, (B, N)).astype(np.uint8)
    d_u = _words(u)
    d_x = dec.transform_device(d_u)
    d_back = dec.transform_device(d_x)
    d_inplace = d_u.clone()
    _tsync()
    dec.transform_device(d_inplace, out=d_inplace)
    dec.synchronize()
    assert np.array_equal(_bits(d_x, N), M.transform(u))
    assert np.array_equal(_bits(d_inplace, N), M.transform(u))
    assert np.array_equal(_bits(d_back, N), u)
    dec.close()


# ---- encode and payload ------------------------------------------------------------------------------------------------
ENCODE_CASES = [("sc32", 65), ("cascl128", 300), ("cascl128-syscrc", 65), ("cascl1024", 65), ("cascl1024-syscrc", 300),
                ("scl4096", 65), ("scl4096", 1), ("pac128", 300), ("pc64", 65), ("rm-repeat", 65), ("rm-puncture", 300),
                ("rm-shorten", 65)]


@pytest.mark.parametrize("name,B", ENCODE_CASES, ids=lambda c: str(c))
def test_encode_equals_the_model(name, B):
    dec, dyn = _make(name)
    v, d_pay = _payload(dec, B, 7 * B + len(name))
    want_u, want_x = _model(dec, dyn, v)
    d_u, d_x = dec.encode_device(d_pay)
    _, d_x_only = dec.encode_device(d_pay, want_u=False)       # u goes to context scratch
    d_u_only, _ = dec.encode_device(d_pay, want_x=False)
    d_back, d_ok = dec.payload_device(d_u)
    dec.synchronize()
    assert np.array_equal(_bits(d_u, dec.N), want_u)
    assert np.array_equal(_bits(d_x, dec.E), want_x)
    assert np.array_equal(d_x.cpu().numpy(), d_x_only.cpu().numpy()) and np.array_equal(d_u.cpu().numpy(), d_u_only.cpu().numpy())
    assert np.array_equal(d_x.cpu().numpy().view(np.uint32), M.pack(want_x))          # the bits at or above E are zero
    assert np.array_equal(d_back.cpu().numpy().view(np.uint32), M.pack(v))            # and those at or above K
    assert (d_ok.cpu().numpy() == 1).all()
    if dyn is not None:
        assert want_u[:, np.asarray(dyn[0])].any()
    # the host-buffer forms
    hu, hx = dec.encode_batch(v[:5])
    hv, hok = dec.payload_batch(hu)
    assert np.array_equal(hu, want_u[:5]) and np.array_equal(hx, want_x[:5])
    assert np.array_equal(hv, v[:5]) and (hok == 1).all()
    dec.close()


@pytest.mark.parametrize("name", ["cascl128", "cascl128-syscrc", "cascl1024", "pac128", "pc64", "rm-repeat", "rm-puncture",
                                  "rm-shorten", "cascl128-crc32"])
def test_encode_reproduces_the_generator(name):
    import torch
    dec, _ = _make(name)
    B = 300
    y = torch.empty((B, dec.E), dtype=torch.float64, device="cuda")
    u_bits = torch.empty((B, dec.NW), dtype=torch.int32, device="cuda")
    dec.generate_device(11, 0, 60.0, y, u_bits=u_bits, out_is_y=True)
    d_pay, d_ok = dec.payload_device(u_bits)
    d_u, d_x = dec.encode_device(d_pay)
    dec.synchronize()
    assert (d_ok.cpu().numpy() == 1).all()
    assert d_pay.cpu().numpy().any()
    assert np.array_equal(d_u.cpu().numpy(), u_bits.cpu().numpy())
    assert np.array_equal(_bits(d_x, dec.E), (y.cpu().numpy() < 0).astype(np.uint8))
    dec.close()


def _algo_decoder(algo, dtype, N=128, K=64):
    import polardecoding_amd as pa
    kw = dict(dtype=dtype)
    return {"sc": lambda: pa.SCdecode(N, K, **kw), "scl": lambda: pa.SCLdecode(N, K, L=8, **kw),
            "cascl": lambda: pa.CASCL(N, K, L=8, crc_taps=pa.CRC6_TAPS, **kw),
            "scf": lambda: pa.SCFlip(N, K, crc_taps=pa.CRC6_TAPS, **kw), "bp": lambda: pa.BP(N, K, **kw),
            "scan": lambda: pa.SCAN(N, K, **kw)}[algo]()


@pytest.mark.parametrize("sys_polar", [False, True], ids=["plain", "sys"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("algo", ["sc", "scl", "cascl", "scf", "bp", "scan"])
def test_round_trip_through_a_decoder(algo, dtype, sys_polar):
    import torch
    dec = _algo_decoder(algo, dtype)
    if sys_polar:
        dec.set_systematic(True)
    assert dec.sys_polar == sys_polar
    v, d_pay = _payload(dec, 65, 3)
    _, d_x = dec.encode_device(d_pay)
    dec.synchronize()
    x = torch.from_numpy(_bits(d_x, dec.N).astype(np.float64)).cuda()
    llr = (1.0 - 2.0 * x) * 4.0
    llr = llr.float() if dtype == F32 else llr
    _tsync()
    bits = dec.decode_device(llr)
    d_back, d_ok = dec.payload_device(bits)
    dec.synchronize()
    assert np.array_equal(d_back.cpu().numpy().view(np.uint32), M.pack(v))
    assert (d_ok.cpu().numpy() == 1).all()
    dec.close()


@pytest.mark.parametrize("crc_sys", [False, True], ids=["plain", "syscrc"])
@pytest.mark.parametrize("sys_polar", [False, True], ids=["u", "sys"])
def test_crc_verdict_and_quotient_on_wrong_decisions(crc_sys, sys_polar):
    """SC decisions (SC-Flip with T = 0) of rows with f % 16 inverted LLR signs: verdict and payload equal the model's on that
    u_hat, for frames that pass and frames that fail"""
    import polardecoding_amd as pa
    dec = pa.SCFlip(128, 64, T=0, crc_taps=pa.CRC6_TAPS, systematic=crc_sys, sys_polar=sys_polar)
    B = 300
    v, d_pay = _payload(dec, B, 5)
    _, d_x = dec.encode_device(d_pay)
    dec.synchronize()
    llr = (1.0 - 2.0 * _bits(d_x, 128).astype(np.float64)) * 4.0
    rng = np.random.default_rng(9)
    for f in range(B):
        llr[f, rng.permutation(128)[:f % 16]] *= -1.0
    bits = dec.decode_device(_cuda(llr))
    d_back, d_ok = dec.payload_device(bits)
    dec.synchronize()
    uh = _bits(bits, 128)
    row = M.transform(uh) if sys_polar else uh
    want_v, want_ok = M.extract(row, dec.info_order, pa.CRC6_TAPS, crc_sys)
    ok = d_ok.cpu().numpy().view(np.uint32)
    assert np.array_equal(ok, want_ok) and ok.any() and not ok.all()
    assert np.array_equal(_bits(d_back, 64), want_v)
    dec.close()


# ---- systematic mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("sc32", 65), ("cascl128", 300), ("cascl128-syscrc", 65), ("cascl1024", 65), ("scl4096", 65)])
def test_systematic_encode_equals_the_two_pass_model(name, B):
    dec, _ = _make(name)
    dec.set_systematic(True)
    v, d_pay = _payload(dec, B, B + 1)
    want_u, want_x = _model(dec, None, v, sys_polar=True)
    d_u, d_x = dec.encode_device(d_pay)
    d_back, d_ok = dec.payload_device(d_u)
    dec.synchronize()
    assert np.array_equal(_bits(d_u, dec.N), want_u) and np.array_equal(_bits(d_x, dec.N), want_x)
    info = dec.info_order
    assert np.array_equal(want_x[:, info], M.crc_word(v, _taps(dec), dec.systematic))   # the codeword carries the CRC word
    assert np.array_equal(d_back.cpu().numpy().view(np.uint32), M.pack(v)) and (d_ok.cpu().numpy() == 1).all()
    dec.close()


def _noisy(dec, B, snr_db, seed=21):
    import torch
    llr = torch.empty((B, dec.N), dtype=torch.float64, device="cuda")
    u_bits = torch.empty((B, dec.NW), dtype=torch.int32, device="cuda")
    dec.generate_device(seed, 0, snr_db, llr, u_bits=u_bits)
    dec.synchronize()   # other contexts, on their own streams, read these rows
    return llr, u_bits


def _decode(dec, llr):
    import torch
    B = llr.shape[0]
    pm = torch.zeros(B, dtype=torch.float64, device="cuda")
    fl = torch.zeros(B, dtype=torch.int32, device="cuda")
    _tsync()
    bits = dec.decode_device(llr, pm=pm, flags=fl)
    dec.synchronize()
    return bits, pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("N,K,taps,snr_db", [(128, 64, M.CRC6, 1.5), (1024, 512, M.CRC24C, 1.0)])
def test_systematic_cascl_is_the_plain_list_with_the_systematic_crc(N, K, taps, snr_db):
    """The list kernels are untouched: the L paths, their metrics and the frame-level flags are those of the plain context on
    the same LLRs, and only the table the final choice tests differs.  With the mode on the chosen path is the best-metric
    path whose tab_sys syndrome is 0, or the best-metric path if none is.  Held here through the plain SCL context of the same
    information set (its output is the best-metric path of the same list):
      - FLAG_CRC_PASS equals the model's CRC verdict on x_hat = u_hat F, frame for frame, and payload_device's verdict;
      - if the best-metric path has syndrome 0, or FLAG_CRC_PASS is clear, output and metric equal that path's, bit for bit;
      - otherwise the output has syndrome 0 and a metric that is not better;
      - the flags other than FLAG_CRC_PASS equal those of the plain CA-SCL context."""
    import polardecoding_amd as pa
    B = 300
    sysd = pa.CASCL(N, K, L=8, crc_taps=taps, sys_polar=True)
    info = sysd.info_order
    plain = pa.CASCL(N, K, L=8, crc_taps=taps, info_order=info)
    scl = pa.SCLdecode(N, K + max(taps), L=8, info_order=info)
    llr, u_bits = _noisy(sysd, B, snr_db)
    b_s, pm_s, fl_s = _decode(sysd, llr)
    b_p, pm_p, fl_p = _decode(plain, llr)
    b_0, pm_0, fl_0 = _decode(scl, llr)
    _, d_ok = sysd.payload_device(b_s)
    sysd.synchronize()
    uh_s, uh_0 = _bits(b_s, N), _bits(b_0, N)
    tab = M.crc_table_sys(N, info, taps)
    syn_s, syn_0 = M.syndrome(tab, uh_s), M.syndrome(tab, uh_0)
    passed = (fl_s & FLAG_CRC_PASS) != 0
    verdict = M.extract(M.transform(uh_s), info, taps)[1].astype(bool)
    assert np.array_equal(passed, verdict) and np.array_equal(passed, syn_s == 0)
    assert np.array_equal(d_ok.cpu().numpy().astype(bool), verdict)
    assert passed.any() and not passed.all()
    same = (syn_0 == 0) | ~passed
    assert np.array_equal(uh_s[same], uh_0[same]) and np.array_equal(pm_s[same], pm_0[same])
    assert (pm_s[~same] >= pm_0[~same]).all() and (~same).any()
    assert np.array_equal(fl_s & ~np.uint32(FLAG_CRC_PASS), fl_p & ~np.uint32(FLAG_CRC_PASS))
    # the sent frames were systematic codewords: the frames decoded correctly carry the payload on x_hat[I]
    good = (b_s.cpu().numpy() == u_bits.cpu().numpy()).all(axis=1)
    assert good.any() and passed[good].all()
    for d in (sysd, plain, scl):
        d.close()


@pytest.mark.parametrize("crc_sys", [False, True], ids=["plain", "syscrc"])
def test_systematic_error_counts_are_on_the_codeword(crc_sys):
    import torch
    import polardecoding_amd as pa
    B, N = 300, 128
    dec = pa.CASCL(N, 64, L=8, crc_taps=pa.CRC6_TAPS, systematic=crc_sys, sys_polar=True)
    llr, u_bits = _noisy(dec, B, 1.0, seed=33)
    bits = dec.decode_device(llr)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    ferr = torch.zeros(B, dtype=torch.int32, device="cuda")
    _tsync()
    dec.count_errors_device(bits, u_bits, cnt, frame_err=ferr)
    dec.synchronize()
    pos = dec.info_order[6:] if crc_sys else dec.info_order
    diff = M.transform(_bits(bits, N))[:, pos] != M.transform(_bits(u_bits, N))[:, pos]
    per = diff.sum(axis=1)
    assert per.any()
    assert np.array_equal(ferr.cpu().numpy(), per)
    assert cnt.cpu().numpy().tolist() == [int((per != 0).sum()), int(per.sum())]
    assert dec.fer_batch(33, 0, 1.0, B) == (int((per != 0).sum()), int(per.sum()))
    dec.close()


def test_systematic_sc_has_fewer_bit_errors_at_the_same_fer():
    """Arikan 2011: the same decoder, about the same FER (same payloads and noise, another codeword), fewer bit errors.  The
    Eb/N0 is the highest of the list at which 20 000 frames hold at least 200 block errors in both modes.  Measured on an
    MI355X: 3.0 dB, FER 0.0223 plain and 0.0219 systematic, 7359 against 3274 bit errors (ratio 0.445)."""
    import polardecoding_amd as pa
    plain, sysd = pa.SCdecode(128, 64), pa.SCdecode(128, 64, sys_polar=True)
    for db in (3.0, 2.5, 2.0, 1.5, 1.0):
        blk_p, bit_p = plain.fer_batch(1, 0, db, 20000)
        blk_s, bit_s = sysd.fer_batch(1, 0, db, 20000)
        print(f"SC(128,64) {db} dB: plain FER {blk_p / 20000:.4f} bit errors {bit_p}; systematic FER {blk_s / 20000:.4f} "
              f"bit errors {bit_s}; ratio {bit_s / max(bit_p, 1):.3f}")
        if blk_p >= 200 and blk_s >= 200:
            break
    else:
        pytest.fail("no Eb/N0 of the list gives 200 block errors in 20 000 frames")
    assert bit_s < bit_p
    plain.close()
    sysd.close()


# ---- refusals, mode off ------------------------------------------------------------------------------------------------
def _refused_and_unchanged(dec, llr):
    import polardecoding_amd as pa
    def decisions():
        bits = dec.decode_device(llr)
        dec.synchronize()
        return bits.cpu().numpy()
    before = decisions()
    with pytest.raises(pa.PolarError):
        dec.set_systematic(True)
    assert dec.sys_polar is False
    assert np.array_equal(decisions(), before)
    dec.close()


def test_set_systematic_refusals():
    import polardecoding_amd as pa
    rng = np.random.default_rng(2)
    pac, _ = _make("pac128")
    _refused_and_unchanged(pac, _cuda(rng.standard_normal((65, 128)) * 3))
    rm, _ = _make("rm-shorten")
    _refused_and_unchanged(rm, _cuda(rng.standard_normal((65, 100)) * 3))
    rnd = pa.CASCL(64, 26, L=8, crc_taps=pa.CRC6_TAPS, info_order=M.random_set())
    _refused_and_unchanged(rnd, _cuda(rng.standard_normal((65, 64)) * 3))


def test_null_buffers_are_refused():
    import torch
    import polardecoding_amd as pa
    dec = pa.SCdecode(64, 32)
    L, h = dec._lib, dec._h
    buf = C.c_void_p(torch.zeros(64, dtype=torch.int32, device="cuda").data_ptr())
    assert L.polar_transform_device(h, None, 1, buf) == -1 and L.polar_transform_device(h, buf, 1, None) == -1
    assert L.polar_encode_device(h, None, 1, buf, buf) == -1
    assert L.polar_encode_device(h, buf, 1, None, None) == -1          # both outputs NULL
    assert L.polar_payload_device(h, None, 1, buf, None) == -1 and L.polar_payload_device(h, buf, 1, None, None) == -1
    assert L.polar_encode_batch(h, None, 1, None, None) == -1 and L.polar_payload_batch(h, None, 1, None, None) == -1
    assert L.polar_set_systematic(None, 1) == -1 and L.polar_set_systematic(h, 2) == -1 and L.polar_get_systematic(None) == 0
    assert L.polar_encode_device(h, buf, 0, buf, buf) == 0             # B = 0
    dec.close()


@pytest.mark.parametrize("stages", [None, (1, 2, 8)], ids=["fixed", "adaptive"])
def test_mode_off_is_the_fresh_context(stages):
    import torch
    import polardecoding_amd as pa
    B = 300
    make = lambda: pa.CASCL(128, 64, L=8, crc_taps=pa.CRC6_TAPS, stages=stages)   # noqa: E731
    fresh, dec = make(), make()
    dec.set_systematic(True)
    llr_on, _ = _noisy(dec, B, 1.5)
    b_on, _, fl_on = _decode(dec, llr_on)
    d_ok = dec.payload_device(b_on)[1]
    dec.synchronize()
    ok_on = d_ok.cpu().numpy().astype(bool)
    assert np.array_equal((fl_on & FLAG_CRC_PASS) != 0, ok_on)      # the stages, too, test the systematic CRC
    dec.set_systematic(False)
    assert dec.sys_polar is False
    outs = []
    for d in (fresh, dec):
        llr, u_bits = _noisy(d, B, 1.5)
        bits, pm, fl = _decode(d, llr)
        outs.append((llr.cpu().numpy(), u_bits.cpu().numpy(), bits.cpu().numpy(), pm, fl, d.fer_batch(5, 0, 1.5, B)))
        d.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert not np.array_equal(llr_on.cpu().numpy(), outs[0][0])     # the mode did change what was sent
