"""GPU: fixed-point min-sum SC / SCL / CA-SCL (dtype POLAR_Q8, csrc/scl_q8.h) against tests/q8_model.py, the numpy statement
of rules 1-6 of include/polar_hip.h.  Integer arithmetic has no rounding: bits, the int32 metric and the flags word are
compared with ==, nowhere a tolerance."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import frozen_patterns as FP  # noqa: E402
import q8_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
CRC6 = (0, 5, 6)


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _frozen(dec):
    fz = np.ones(dec.N, dtype=np.uint8)
    fz[dec.info_order] = 0
    return fz


def _model(dec, q, crc_taps=None, sc=False):
    sc_, qc, qi = dec.quant
    crc = (dec.info_order, crc_taps) if crc_taps else None
    return M.decode_rows(q, _frozen(dec), dec.L, crc=crc, qc=qc, qi=qi, sc=sc)


def _q8_device(dec, q):
    """polar_q8_decode_device on int8 rows -> (u_hat, pm int32, flags)"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(q, dtype=np.int8)).cuda()
    B = d.shape[0]
    pm = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_q8_device(d, pm=pm, flags=fl)
    dec.synchronize()
    return _unpack(bits.cpu().numpy(), dec.N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


def _float_device(dec, x, dtype, sigma=0.0):
    """polar_decode_device on float rows of a Q8 ctx (rule 7) -> (u_hat, pm double, flags)"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()
    B = d.shape[0]
    pm = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bits = dec.decode_device(d, sigma=sigma, pm=pm, flags=fl)
    dec.synchronize()
    return _unpack(bits.cpu().numpy(), dec.N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: bits differ in frames {np.flatnonzero((got[0] != want[0]).any(axis=1))[:8]}"
    assert np.array_equal(np.asarray(got[1]).astype(np.int64), np.asarray(want[1]).astype(np.int64)), f"{what}: metrics differ"
    assert np.array_equal(got[2], want[2]), f"{what}: flags differ"


def _rows(rng, B, N, amp=24.0):
    """float rows whose quantised values spread over the int8 range with many small ones (ties and zeros included)"""
    return rng.normal(0.0, amp, size=(B, N)) * (rng.random((B, 1)) < 0.7) + rng.normal(0.0, 1.5, size=(B, N))


# ---- shapes: SC and SCL, every list size, both entry points -----------------------------------------------------------------
@pytest.mark.parametrize("N", [32, 64, 256])
@pytest.mark.parametrize("L", [0, 1, 2, 4, 8, 32])   # 0: POLAR_ALGO_SC
def test_shapes_against_the_model(N, L):
    import polardecoding_amd as pa
    B = 65 if N <= 64 else 9          # more frames than one pass of a small grid takes by index (B = 65 at N <= 64)
    rng = np.random.default_rng([N, L])
    x = _rows(rng, B, N)
    dec = pa.SCdecode(N, N // 2, dtype=pa.Q8) if L == 0 else pa.SCLdecode(N, N // 2, L=L, dtype=pa.Q8)
    assert dec.kernel_name == f"k_scl_q8<L={max(L, 1)}>" and dec.quant == (2.0, 8, 8)
    q = dec.quantize(x)
    assert np.array_equal(q, M.quantize(x))
    want = _model(dec, q, sc=(L == 0))
    if L == 0:
        assert not want[1].any() and not want[2].any()
    _same(_q8_device(dec, q), want, "polar_q8_decode_device")
    _same(_q8_device(dec, q[:1]), [w[:1] for w in want], "B = 1")
    _same(_float_device(dec, x, np.float64), want, "polar_decode_device, double rows (rule 7)")
    xf = x.astype(np.float32)
    _same(_float_device(dec, xf, np.float32), _model(dec, M.quantize(xf), sc=(L == 0)), "polar_decode_device, float rows")
    _same(dec.decode_q8_batch(q), want, "polar_q8_decode_batch")
    uh, pm, fl = dec.decode_batch(x)
    _same((uh, pm, fl), want, "polar_decode_batch")
    # y rows: 2*y/sigma/sigma inside the quantiser
    sig = 0.84
    y = x * sig * sig / 2
    qy = M.quantize(y, sigma=sig)
    _same(_float_device(dec, y, np.float64, sigma=sig), _model(dec, qy, sc=(L == 0)), "y rows")


# ---- CA-SCL ---------------------------------------------------------------------------------------------------------------
def test_cascl_128():
    import polardecoding_amd as pa
    N, K, B = 128, 64, 40
    dec = pa.CASCL(N, K, L=8, crc_taps=CRC6, dtype=pa.Q8)
    x = _rows(np.random.default_rng(128), B, N, amp=10.0)
    q = dec.quantize(x)
    want = _model(dec, q, crc_taps=CRC6)
    assert (want[2] & M.FLAG_CRC_PASS).any() and not (want[2] & M.FLAG_CRC_PASS).all()   # both outcomes of rule 6
    _same(_q8_device(dec, q), want, "N=128 CA-SCL")
    _same(_float_device(dec, x, np.float64), want, "N=128 CA-SCL, float entry")


@pytest.mark.parametrize("L", [8, 32])
def test_cascl_1024_generated_frames(L):
    import torch
    import polardecoding_amd as pa
    N, K, B = 1024, 512, 32
    dec = pa.CASCL(N, K, L=L, dtype=pa.Q8)
    x = torch.empty((B, N), dtype=torch.float32, device="cuda")
    ub = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    dec.generate_device(5, 100, 2.0, x, u_bits=ub)
    dec.synchronize()
    xh = x.cpu().numpy()
    q = M.quantize(xh)
    dq = dec.quantize_device(x)
    dec.synchronize()
    assert np.array_equal(dq.cpu().numpy(), q)                 # polar_q8_quantize_device is rule 1
    want = _model(dec, q, crc_taps=pa.CRC24C_TAPS)
    _same(_q8_device(dec, q), want, f"N=1024 CA-SCL L={L}")
    _same(_float_device(dec, xh, np.float32), want, f"N=1024 CA-SCL L={L}, float entry")
    sent = _unpack(ub.cpu().numpy(), N)
    assert (want[0] == sent).all(axis=1).sum() >= B // 2       # at 2.0 dB most frames decode


# ---- row families: the smallest inputs that reach each branch ------------------------------------------------------------------
def _family_rows(name, B, N, rng):
    if name == "ternary":
        return rng.integers(-1, 2, size=(B, N)).astype(np.int8)
    if name == "pm127":
        return (127 * (1 - 2 * rng.integers(0, 2, size=(B, N)))).astype(np.int8)
    if name == "pm15":
        return rng.integers(-15, 16, size=(B, N)).astype(np.int8)
    if name == "minus128":
        q = rng.integers(-128, 128, size=(B, N)).astype(np.int8)
        q[:, ::7] = -128
        return q
    assert name == "zero"
    return np.zeros((B, N), dtype=np.int8)


@pytest.mark.parametrize("name", ["ternary", "pm127", "pm15", "minus128", "zero"])
def test_row_families(name):
    import polardecoding_amd as pa
    N, K, B = 128, 64, 24
    rng = np.random.default_rng(len(name))
    q = _family_rows(name, B, N, rng)
    quant = (2.0, 5, 5) if name == "pm15" else (2.0, 8, 8)      # qi = 5: the internal clamp (15) is narrower than int8
    for mk, taps in ((lambda: pa.SCLdecode(N, K, L=4, dtype=pa.Q8, quant=quant), None),
                     (lambda: pa.CASCL(N, K, L=8, crc_taps=CRC6, dtype=pa.Q8, quant=quant), CRC6),
                     (lambda: pa.SCdecode(N, K, dtype=pa.Q8, quant=quant), None)):
        dec = mk()
        assert dec.quant == quant
        sc = dec.algo == pa.ALGO_SC
        want = _model(dec, q, crc_taps=taps, sc=sc)
        _same(_q8_device(dec, q), want, f"{name} L={dec.L}")
        if name in ("ternary", "zero") and not sc:
            assert (want[2] & M.FLAG_TIE).all()                # a tie in every frame, and the library agrees on it
    if name == "pm15":
        dec = pa.SCLdecode(N, K, L=4, dtype=pa.Q8, quant=(2.0, 5, 8))
        a, b = _model(dec, q), M.decode_rows(q, _frozen(dec), 4, qc=5, qi=5)
        assert not np.array_equal(a[1], b[1])                  # the narrower internal clamp changes metrics: the case bites
        _same(_q8_device(dec, q), a, "qc=5 qi=8")
    if name == "minus128":
        dec = pa.SCLdecode(N, K, L=4, dtype=pa.Q8, quant=(2.0, 6, 8))
        _same(_q8_device(dec, q), _model(dec, q), "int8 rows clamped to Cc = 31 on load")


# ---- frozen sets outside the 5G order -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["leaf0", "islands_8_a", "islands_64_b", "lead_16"])
def test_frozen_patterns(name):
    import polardecoding_amd as pa
    N, L, B = 256, 4, 12
    mask = FP.families(N)[name]
    if name == "lead_16":
        assert FP.leading_frozen_octets(mask) == 16
    order = FP.order_of(mask, 3)
    dec = pa.SCLdecode(N, order.size, L=L, info_order=order, dtype=pa.Q8)
    assert np.array_equal(_frozen(dec), mask)
    x = _rows(np.random.default_rng(len(name)), B, N, amp=12.0)
    q = dec.quantize(x)
    _same(_q8_device(dec, q), _model(dec, q), name)


# ---- noise-free rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sc", "scl", "cascl"])
def test_noise_free_rows_return_the_sent_word(algo):
    import polardecoding_amd as pa
    N, K, B = 256, 128, 20
    dec = {"sc": lambda: pa.SCdecode(N, K, dtype=pa.Q8), "scl": lambda: pa.SCLdecode(N, K, L=8, dtype=pa.Q8),
           "cascl": lambda: pa.CASCL(N, K, L=8, crc_taps=CRC6, dtype=pa.Q8)}[algo]()
    payload = np.random.default_rng(9).integers(0, 2, size=(B, K)).astype(np.int32)
    u, x = dec.encode_batch(payload)
    q = (127 * (1 - 2 * x)).astype(np.int8)
    uh, pm, fl = _q8_device(dec, q)
    assert np.array_equal(uh, u) and not pm.any()
    assert (fl & M.FLAG_CRC_PASS).all() if algo == "cascl" else not (fl & M.FLAG_CRC_PASS).any()


# ---- polar_fer_batch is generate -> quantise -> decode -> count ----------------------------------------------------------------
def test_fer_batch_is_the_chain_by_hand():
    import torch
    import polardecoding_amd as pa
    N, K, B, db, seed = 128, 64, 4096, 2.0, 77
    dec = pa.CASCL(N, K, L=8, crc_taps=CRC6, dtype=pa.Q8)
    x = torch.empty((B, N), dtype=torch.float32, device="cuda")
    ub = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    dec.generate_device(seed, 500, db, x, u_bits=ub)
    q = dec.quantize_device(x)
    bits = dec.decode_q8_device(q)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    dec.synchronize()
    torch.cuda.synchronize()
    dec.count_errors_device(bits, ub, cnt)
    dec.synchronize()
    want = tuple(cnt.cpu().tolist())
    got = dec.fer_batch(seed, 500, db, B)
    print(f"Q8 CA-SCL N=128 L=8 at {db} dB: block errors {got[0]}, bit errors {got[1]} of {B}")
    assert got == want and 0 < got[0] < B // 2
    # the same chain on the host: the stop rule on y rows
    sig = 10 ** (-db / 20)
    y = (x.cpu().numpy().astype(np.float64) * sig * sig / 2)[:256]
    sent = _unpack(ub.cpu().numpy(), N)[:256]
    uh = _model(dec, M.quantize(y, sigma=sig), crc_taps=CRC6)[0]
    io = dec.info_order
    err = (uh[:, io] != sent[:, io]).sum(axis=1)
    assert dec.stop_rule_batch_y(y, sig, sent, need=10 ** 6) == (256, int((err > 0).sum()), int(err.sum()))


# ---- graph capture ------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_same_bits():
    import torch
    import polardecoding_amd as pa
    N, K, B = 256, 128, 700
    dec = pa.CASCL(N, K, L=8, crc_taps=CRC6, dtype=pa.Q8)
    q = dec.quantize(_rows(np.random.default_rng(5), B, N, amp=8.0))
    ref = _q8_device(dec, q)               # the warm-up at the same B
    d = torch.from_numpy(q).cuda()
    out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    pm = torch.empty(B, dtype=torch.int32, device="cuda")
    fl = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dec.use_torch_stream()
        with torch.cuda.graph(g, stream=s):    # one linear stream, no parallel branches
            dec.decode_q8_device(d, out_bits=out, pm=pm, flags=fl)
    torch.cuda.synchronize()
    out.zero_()
    pm.fill_(-1)
    fl.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _same((_unpack(out.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)), ref, "replay")
    dec.use_torch_stream()
    del g


# ---- the quantiser of a ctx, refusals ---------------------------------------------------------------------------------------
def test_set_quant_and_refusals_leave_the_ctx_usable():
    import torch
    import polardecoding_amd as pa
    N, K = 128, 64
    dec = pa.CASCL(N, K, L=8, crc_taps=CRC6, dtype=pa.Q8)
    x = _rows(np.random.default_rng(2), 30, N, amp=10.0)
    ref = _float_device(dec, x, np.float64)
    for bad in ((0.0, 8, 8), (-2.0, 8, 8), (float("inf"), 8, 8), (float("nan"), 8, 8), (2.0, 1, 8), (2.0, 6, 5), (2.0, 8, 9), (2.0, 9, 9)):
        with pytest.raises(pa.PolarError) as e:
            dec.set_quant(*bad)
        assert "rc=-1" in str(e.value)
        assert dec.quant == (2.0, 8, 8)
    d = torch.from_numpy(x).cuda()
    for call in (lambda: dec.set_systematic(True), lambda: dec.set_cascl_stages((1, 8)), lambda: dec.set_bp_stop("g"),
                 lambda: dec.decode_bp_device(d), lambda: dec.set_scf_flips(2), lambda: dec.decode_scf_device(d),
                 lambda: dec.set_scan_iters(2), lambda: dec.decode_scan_device(d),
                 lambda: dec.genie_count_device(d, torch.zeros((2, N), dtype=torch.int64, device="cuda")),
                 lambda: dec.genie_rows_device(1, 0, 0.7, torch.empty((4, N), dtype=torch.float64, device="cuda")),
                 lambda: dec.construct_batch(1, 0, 0.7, 64, torch.zeros((2, N), dtype=torch.int64, device="cuda"))):
        with pytest.raises(pa.PolarError) as e:
            call()
        assert "rc=-1" in str(e.value)
    with pytest.raises(pa.PolarError) as e:   # a frozen_mask override
        pa.SCLdecode(N, K, L=2, dtype=pa.Q8).decode_batch(x, frozen_mask=np.ones(N, dtype=np.uint8))
    assert "rc=-1" in str(e.value)
    # polar_q8_* on a ctx of another dtype
    f32 = pa.CASCL(N, K, L=8, crc_taps=CRC6, dtype=pa.F32)
    dq = torch.zeros((4, N), dtype=torch.int8, device="cuda")
    for call in (lambda: f32.set_quant(2.0, 8, 8), lambda: f32.quant, lambda: f32.quantize_device(d),
                 lambda: f32.decode_q8_device(dq), lambda: f32.decode_q8_batch(np.zeros((4, N), dtype=np.int8))):
        with pytest.raises(pa.PolarError) as e:
            call()
        assert "rc=-1" in str(e.value)
    _same(_float_device(dec, x, np.float64), ref, "after refusals")
    # a new quantiser takes effect, and polar_create_crc_file makes the same decoder
    dec.set_quant(1.0, 5, 6)
    assert dec.quant == (1.0, 5, 6)
    want = M.decode_rows(M.quantize(x, 1.0, 5), _frozen(dec), 8, crc=(dec.info_order, CRC6), qc=5, qi=6)
    _same(_float_device(dec, x, np.float64), want, "scale 1, qc 5, qi 6")
    import ctypes as C
    dt = C.c_int()
    dec._lib.polar_ctx_info(dec._h, None, None, None, None, None, C.byref(dt))
    assert dt.value == 2


def test_crc_file_context(tmp_path):
    import polardecoding_amd as pa
    N, K = 128, 64
    path = str(tmp_path / "CRC_6.dat")
    pa.save_crc_matrix(path, K, CRC6)
    a = pa.CASCL(N, K, L=8, crc_file=path, dtype=pa.Q8)
    b = pa.CASCL(N, K, L=8, crc_taps=CRC6, dtype=pa.Q8)
    q = a.quantize(_rows(np.random.default_rng(4), 30, N, amp=10.0))
    _same(_q8_device(a, q), _q8_device(b, q), "polar_create_crc_file")
    _same(_q8_device(a, q), _model(b, q, crc_taps=CRC6), "polar_create_crc_file against the model")


def test_polar_sim_q8():
    import subprocess
    sim = os.path.join(REPO, "polardecoding_amd", "lib", "polar_sim")
    base = [sim, "--algo", "cascl", "--N", "128", "--K", "64", "--crc", "6", "--snr", "2.0:2.5:0.5", "--ble", "5", "--dtype", "q8"]
    for extra in (["--fast", "--batch", "4096"], ["--batch", "1024", "--quant", "1,5,6"]):   # polar_fer_batch; polar_stop_rule_batch_y
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [ln for ln in r.stdout.splitlines() if "bSNR = " in ln]
        assert len(lines) == 2 and "error block" in lines[0], r.stdout
    r = subprocess.run(base + ["--quant", "2,9,9"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--quant" in r.stderr


# ---- the float contexts are untouched ---------------------------------------------------------------------------------------
def test_float_contexts_after_a_q8_one_equal_the_oracle(oracle):
    import polardecoding_amd as pa
    code = oracle.Code(1024, 512, oracle.CRC24C_TAPS)
    sig = oracle.sigma_from_db(1.5)
    us, ys = oracle.Sim(7).frames(code, sig, 16)          # the 16 frames of smoke()
    llr = np.stack([oracle.llr_from_y(y, sig) for y in ys])
    q8 = pa.CASCL(1024, 512, L=8, dtype=pa.Q8)
    q8.decode_batch(llr)
    for dtype, name in ((pa.F64, "f64"), (pa.F32, "f32")):
        ref, ref_pm, _ = oracle.decode(code, llr, "CASCL", L=8, dtype=name)
        dec = pa.CASCL(1024, 512, L=8, dtype=dtype)
        uh, pm, fl = dec.decode_batch(llr)
        assert np.array_equal(uh, ref), name
        assert np.array_equal(pm.astype(np.float32 if name == "f32" else np.float64), ref_pm), name
        assert "q8" not in dec.kernel_name
