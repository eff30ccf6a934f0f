"""GPU: k_scl_q8 and k_q8_quantize (csrc/scl_q8.h, csrc/k_q8.hip) against tests/q8_model.py on the table of tests/q8_cases.py.

Integer arithmetic has no rounding: u_hat bit for bit, the int32 metric (and the double one of the float entry, compared as
doubles) and the flags word are compared with == on every frame; the quantiser's int8 values with == on every element.  The
pm / flags buffers start from values no decode writes.  Every context asserts kernel_name == "k_scl_q8<L=..>", its
info_order and its quantiser.  tests/test_q8_cases_host.py holds on the CPU what each group is there for.

  A  every (N, L) of N = 32 .. 1024 x L = SC, 1, 2, 4, 8, 16, 32 (L = 16 is the only instantiation with S = 4) through
     polar_q8_decode_device on 12 rows, one L per N (and every CA-SCL case) also through polar_decode_device on double rows;
     CA-SCL at L = 2, 16 with CRC-6 / CRC-11 / CRC-24C
  B  every frozen pattern of tests/frozen_patterns.py at N = 128 (L = 2, 8, 16, 32; CA-SCL L = 8 where the mask can carry
     CRC-6) and at N = 1024 (L = 8, 32), the lists that never fill among them
  C  all 28 clamp pairs at N = 128 as SCL L = 8, CA-SCL L = 8 and SC; three of them also through the float entry at scales 0.5, 2.0, 3.7
  D  polar_q8_quantize_device on constructed values, double and float input at an address aligned to the element size and
     no more, the output at an odd address inside a buffer of markers; B = 9 and 73 rows of N = 32
  E  metrics above 2^13 through the int32 and the double metric path

Records, not gates.  With the 5G order the model ties (FLAG_TIE) on these frames of the 12 of group A, L = 2, 4, 8, 16, 32:
N = 128: 7, 12, 10, 12, 12; N = 256: 9, 11, 10, 12, 12; N = 512: 8, 10, 12, 12, 12; N = 1024: 11, 12, 12, 12, 12; in the CA-SCL
cases 8 to 12 of 12.  FLAG_CRC_PASS is set on these of the 6 spread rows, L = 2 / 16: N = 64: 2 / 2; 128: 3 / 4; 256: 2 / 4;
512: 1 / 2; 1024: 1 / 3.
The model's CPU time on the machine this was written on: group A 10.5 s (N = 1024, L = 32: 1.0 s for its 12 frames), B 26 s
(N = 128: 7 s, N = 1024: 19 s), C 7 s, D and E below 1 s each.  On one MI355X the 168 tests of this file took 21.3 s of wall
time, that host's model time included; no test more than 0.5 s but the first, which loads the library (2.1 s).
No comparison failed when the file was written: no change to csrc/scl_q8.h or csrc/k_q8.hip came of it."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import q8_cases as Q  # noqa: E402
import q8_model as M  # noqa: E402
from test_gpu_q8 import _float_device, _q8_device, _same  # noqa: E402

NEVER = -128          # the quantiser never writes -128: the marker around its output and under it


def _decoder(ctx):
    import polardecoding_amd as pa
    K = ctx.order.size - (max(ctx.taps) if ctx.taps else 0)
    kw = dict(dtype=pa.Q8)
    if ctx.given:
        kw["info_order"] = ctx.order
    if ctx.quant != Q.DEFAULT_QUANT:
        kw["quant"] = ctx.quant
    if ctx.sc:
        dec = pa.SCdecode(ctx.N, K, **kw)
    elif ctx.taps:
        dec = pa.CASCL(ctx.N, K, L=ctx.L, crc_taps=ctx.taps, **kw)
    else:
        dec = pa.SCLdecode(ctx.N, K, L=ctx.L, **kw)
    assert dec.kernel_name == f"k_scl_q8<L={max(ctx.L, 1)}>" and dec.L == max(ctx.L, 1)
    assert np.array_equal(dec.info_order, ctx.order) and dec.quant == ctx.quant
    return dec


def _same_f64(got, want, what):
    """the float entry: bits and flags as _same, the metric a double equal to the model's integer"""
    _same(got, want, what)
    assert got[1].dtype == np.float64 and np.array_equal(got[1], want[1].astype(np.float64)), f"{what}: double metrics differ"


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,crc", Q.a_cases(), ids=lambda v: str(int(v)))
def test_a_every_shape(N, L, crc):
    ctx = Q.a_ctx(N, L, crc)
    x, q = Q.a_rows(N, L, crc)
    want = Q.a_want(N, L, crc)
    dec = _decoder(ctx)
    if L == 16:
        assert dec.kernel_name == "k_scl_q8<L=16>"
    tag = f"N={N} L={L}{' CA-SCL' if crc else ''}"
    _same(_q8_device(dec, q), want, f"{tag} polar_q8_decode_device")
    if crc or Q.A_FLOAT_L[N] == L:
        _same_f64(_float_device(dec, x, np.float64), want, f"{tag} polar_decode_device, double rows (rule 7)")
    dec.close()


# ---- B ------------------------------------------------------------------------------------------------------------------
def _b_run(N, name):
    q = Q.b_rows(N, name)
    for L in Q.B_LS[N]:
        dec = _decoder(Q.b_ctx(N, name, L))
        _same(_q8_device(dec, q), Q.b_want(N, name, L), f"N={N} {name} L={L}")
        dec.close()


@pytest.mark.parametrize("name", Q.b_masks(128))
def test_b_frozen_patterns_128(name):
    _b_run(128, name)
    if name in Q.b_crc_masks():
        dec = _decoder(Q.b_ctx(128, name, Q.B_CRC_L, True))
        _same(_q8_device(dec, Q.b_rows(128, name)), Q.b_want(128, name, Q.B_CRC_L, True), f"N=128 {name} CA-SCL L={Q.B_CRC_L}")
        dec.close()


@pytest.mark.parametrize("name", Q.b_masks(1024))
def test_b_frozen_patterns_1024(name):
    _b_run(1024, name)


# ---- C ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qc,qi", Q.C_PAIRS)
def test_c_every_clamp_pair(qc, qi):
    for kind in Q.C_KINDS:
        q, want = Q.c_rows(kind), Q.c_want(kind, qc, qi)
        dec = _decoder(Q.c_ctx(kind, qc, qi))
        _same(_q8_device(dec, q), want, f"{kind} qc={qc} qi={qi}")
        dec.close()
        for scale in Q.C_FLOAT_SCALES if (qc, qi) in Q.C_FLOAT_PAIRS else ():
            dec = _decoder(Q.c_ctx(kind, qc, qi, scale))
            x = Q.float_rows_of(q, scale)
            for dtype in (np.float64, np.float32):
                _same_f64(_float_device(dec, x.astype(dtype), dtype), want, f"{kind} qc={qc} qi={qi} scale={scale} {np.dtype(dtype).name} rows")
            dec.close()


# ---- D ------------------------------------------------------------------------------------------------------------------
def _quantize_device(dec, rows, sigma=0.0, off=37):
    """polar_q8_quantize_device on rows [B][32]: the input one element into its allocation, the output `off` (odd) bytes into a
    buffer of markers -> int8 [B][32].  Asserts that the markers around the output are intact."""
    import torch
    B, n, esz = rows.shape[0], rows.size, rows.dtype.itemsize
    src = torch.zeros(n + 1, dtype=torch.float64 if esz == 8 else torch.float32, device="cuda")
    src[1:] = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)).cuda()
    d_in = src[1:].view(B, Q.D_N)
    assert d_in.data_ptr() % (2 * esz) == esz and d_in.is_contiguous()
    buf = torch.full((n + 2 * off + 1,), NEVER, dtype=torch.int8, device="cuda")
    out = buf[off:off + n]
    assert out.data_ptr() % 2 == 1
    torch.cuda.synchronize()
    dec.quantize_device(d_in, sigma=sigma, out=out)
    dec.synchronize()
    got = buf.cpu().numpy()
    assert (got[:off] == NEVER).all() and (got[off + n:] == NEVER).all(), "the quantiser wrote outside its output"
    return got[off:off + n].reshape(B, Q.D_N)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("scale", Q.D_SCALES)
def test_d_quantiser_on_constructed_values(scale, dtype):
    dec = _decoder(Q.d_ctx())
    for qc in Q.D_QCS:
        dec.set_quant(scale, qc, 8)
        for B, small in zip(Q.D_BS, (True, False)):
            rows = Q.d_pad(Q.d_values(scale, dtype, small=small), B)
            assert rows.dtype == dtype and (B * Q.D_N) % 256
            got = _quantize_device(dec, rows)
            want = M.quantize(rows, scale, qc)
            bad = np.flatnonzero((got != want).ravel())
            assert bad.size == 0, (f"scale={scale} qc={qc} B={B}: {bad.size} values differ, first at {bad[:4]}: in "
                                   f"{rows.ravel()[bad[:4]]!r} got {got.ravel()[bad[:4]]} want {want.ravel()[bad[:4]]}")
    dec.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("sigma,scale", Q.D_Y)
def test_d_quantiser_on_y_values(sigma, scale, dtype):
    dec = _decoder(Q.d_ctx())
    for qc in (8, 5):
        dec.set_quant(scale, qc, 8)
        rows = Q.d_pad(Q.d_y_values(sigma, scale, dtype), 73)
        got = _quantize_device(dec, rows, sigma=sigma)
        want = M.quantize(rows, scale, qc, sigma=sigma)
        bad = np.flatnonzero((got != want).ravel())
        assert bad.size == 0, f"sigma={sigma} scale={scale} qc={qc}: {bad.size} values differ, first at {bad[:4]}"
    dec.close()


@pytest.mark.parametrize("dtype,scale,qc", [(np.float64, 2.0, 8), (np.float32, 3.7, 5)], ids=["double", "float"])
def test_d_float_entry_is_quantise_then_decode(dtype, scale, qc):
    """polar_decode_device on the constructed rows = polar_q8_decode_device on the model's int8 rows = the model"""
    ctx = Q.d_ctx()._replace(quant=(scale, qc, 8))
    dec = _decoder(ctx)
    rows = Q.d_pad(Q.d_values(scale, dtype), 73)
    q = M.quantize(rows, scale, qc)
    assert q.max() == M.clamp_of(qc) and q.min() == -M.clamp_of(qc)
    want = Q.model(ctx, q)
    _same_f64(_float_device(dec, rows, dtype), want, "polar_decode_device")
    _same(_q8_device(dec, q), want, "polar_q8_decode_device")
    dec.close()


# ---- E ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", Q.E_LS)
@pytest.mark.parametrize("name", Q.E_MASKS)
def test_e_large_metrics(name, L):
    q, want = Q.e_rows(name), Q.e_want(name, L)
    assert want[1].max() >= Q.E_FLOOR
    dec = _decoder(Q.e_ctx(name, L))
    got = _q8_device(dec, q)
    assert got[1].dtype == np.int32
    _same(got, want, f"{name} L={L} int32 metric")
    _same_f64(_float_device(dec, Q.float_rows_of(q, 2.0), np.float64), want, f"{name} L={L} double metric")
    dec.close()
