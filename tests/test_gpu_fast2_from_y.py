"""GPU: the two forms of the pair kernel -- k_scl_fast2 (the rows are LLRs, sigma = 0) and k_scl_fast2_y (the rows are
channel observations y, converted with sigma > 0 at every channel read) -- on the same frames.

CA-SCL and SCL at N = 1024, K = 512, L = 8, f64 and f32.  Frames from the oracle's simulator at 1.5 dB go through both forms:
as y with sigma, and as the LLRs 2 y / sigma^2 computed on the host.  In f64 both must equal the CPU oracle bit for bit --
decisions, path metric, the tie and re-rank flags -- and each other in every flag; in f32 they must equal each other (for
float input rows as well: the LLRs are then formed from the rounded y, as the kernel forms them).  The rows of
tests/golden/ties_CASCL_1024_L8.npz go through the LLR form.

Batch sizes: 2 (one pair of frames, no work queue), 63 (odd: the idle half of the last wavefront decodes the last frame once
more) and 2 * 6144 + 2 (more pairs than resident wavefronts in f64 and f32: the rest comes through the work queue).  The big
batches repeat the 49 simulated frames, so the oracle decodes each frame once."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K, L = 1024, 512, 8
NSIM = 49
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def _taps(algo):
    import polardecoding_amd as pa
    return pa.CRC24C_TAPS if algo == "CASCL" else None


def _frames(oracle, algo):
    """49 simulated frames of the algorithm's code at 1.5 dB and what the f64 oracle makes of them (computed once)."""
    if algo not in _cache:
        code = oracle.Code(N, K, _taps(algo))
        sig = oracle.sigma_from_db(1.5)
        _, ys = oracle.Sim(1300 + (algo == "SCL")).frames(code, sig, NSIM)
        y = np.stack(ys)
        llr = np.stack([oracle.llr_from_y(r, sig) for r in y])
        st = np.zeros((NSIM, 2), dtype=np.int32)
        uh, pm, ties = oracle.decode(code, llr, algo, L=L, stats=st)
        for a in (y, llr, uh, pm, ties, st):
            a.setflags(write=False)
        _cache[algo] = (sig, y, llr, uh, pm, ties, st)
    return _cache[algo]


def _decoder(algo, dtype):
    import polardecoding_amd as pa
    dt = pa.F64 if dtype == "f64" else pa.F32
    dec = pa.CASCL(N, K, L=L, dtype=dt) if algo == "CASCL" else pa.SCLdecode(N, K, L=L, dtype=dt)
    assert dec.kernel_name.startswith("k_scl_fast2<"), dec.kernel_name
    return dec


def _run(dec, rows, sigma):
    """rows [B][N] (numpy) through polar_decode_device -> u_hat [B][N], pm [B], flags [B]"""
    import torch
    from conftest import unpack_bits
    x = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    B = x.shape[0]
    bits = torch.full((B, N // 32), -1, dtype=torch.int32, device="cuda")
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    dec.decode_device(x, sigma=sigma, out_bits=bits, pm=pm, flags=fl)
    dec.synchronize()
    assert dec.kernel_name.startswith("k_scl_fast2<"), dec.kernel_name
    return unpack_bits(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("B", [2, 63, 6144 * 2 + 2])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("algo", ["CASCL", "SCL"])
def test_y_with_sigma_equals_llr_rows(algo, dtype, B, oracle):
    import polardecoding_amd as pa
    sig, y, llr, o_uh, o_pm, o_ties, o_st = _frames(oracle, algo)
    idx = np.arange(B) % NSIM
    dec = _decoder(algo, dtype)
    uh_y, pm_y, fl_y = _run(dec, y[idx], sig)
    uh_l, pm_l, fl_l = _run(dec, llr[idx], 0.0)
    bad = np.nonzero((uh_y != uh_l).any(axis=1))[0]
    assert bad.size == 0, f"decisions of the two forms differ in frames {bad[:8]}"
    assert np.array_equal(pm_y.view(np.int64), pm_l.view(np.int64))
    assert np.array_equal(fl_y, fl_l)
    if dtype == "f64":
        for uh, pm, fl in ((uh_y, pm_y, fl_y), (uh_l, pm_l, fl_l)):
            bad = np.nonzero((uh != o_uh[idx]).any(axis=1))[0]
            assert bad.size == 0, f"decisions differ from the oracle's in frames {bad[:8]}"
            assert np.array_equal(pm, o_pm[idx])
            assert np.array_equal((fl & pa.FLAG_TIE) != 0, o_ties[idx] > 0)
            assert np.array_equal((fl & pa.FLAG_RERANK) != 0, o_st[idx, 0] > 0)
    else:
        # float input rows: y rounded to float, the LLRs formed from the rounded y in double and then rounded, as chv() does
        y32 = y[idx].astype(np.float32)
        llr32 = np.stack([oracle.llr_from_y(r.astype(np.float64), sig) for r in y32[:NSIM]]).astype(np.float32)[idx]
        uh_y, pm_y, fl_y = _run(dec, y32, sig)
        uh_l, pm_l, fl_l = _run(dec, llr32, 0.0)
        assert np.array_equal(uh_y, uh_l)
        assert np.array_equal(pm_y.view(np.int64), pm_l.view(np.int64))
        assert np.array_equal(fl_y, fl_l)
    if B == 2:   # the one-frame entry (polar_decode: y and sigma)
        assert np.array_equal(dec(y[0], sig), uh_l[0])
    dec.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("algo", ["CASCL", "SCL"])
def test_tie_rows_through_the_llr_form(algo, dtype, oracle):
    """the 14 rows with median ties, as LLRs, 63 frames (the rows repeated; odd tail) against the oracle of the same
    arithmetic type: decisions, path metric, tie flag; in f64 the re-rank flag as well"""
    import polardecoding_amd as pa
    z = np.load(os.path.join(GOLD, "ties_CASCL_1024_L8.npz"))
    llr = np.stack([oracle.llr_from_y(r, float(z["sigma"])) for r in z["y"]])
    code = oracle.Code(N, K, _taps(algo))
    st = np.zeros((len(llr), 2), dtype=np.int32)
    o_uh, o_pm, o_ties = oracle.decode(code, llr, algo, L=L, dtype=dtype, stats=st)
    idx = np.arange(63) % len(llr)
    dec = _decoder(algo, dtype)
    uh, pm, fl = _run(dec, llr[idx], 0.0)
    assert np.array_equal(uh, o_uh[idx])
    assert np.array_equal(pm.astype(o_pm.dtype), o_pm[idx])
    assert np.array_equal((fl & pa.FLAG_TIE) != 0, o_ties[idx] > 0)
    if dtype == "f64":
        assert np.array_equal((fl & pa.FLAG_RERANK) != 0, st[idx, 0] > 0)
    dec.close()
