"""GPU: 5G NR rate matching (include/polar_hip.h rules 1-7) against the numpy model of tests/test_rm_host.py.

The recovery kernel bit for bit in every mode, with and without the channel interleaver, f64 / f32, LLR / y input, odd E and
misaligned rows; decoding on a rate-matched context against a plain context with the rate-matched order fed the model's
rows, for every decoder; the generator against the model; polar_fer_batch end to end; the refusals and polar_sim."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import test_rm_host as M  # noqa: E402

CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)
CRC6 = (0, 5, 6)


def _unpack(words, N):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, N).astype(np.int32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# (N, K, E) per mode, E odd where it can be; A = K (no CRC) for the recovery tests
RECOVER_CASES = [(32, 10, 25), (32, 20, 27), (32, 16, 101),
                 (128, 30, 99), (128, 80, 111), (128, 64, 389),
                 (512, 120, 301), (512, 300, 433), (512, 256, 1537),
                 (1024, 200, 865), (1024, 536, 863), (1024, 512, 2049), (1024, 100, 8191)]


@pytest.mark.parametrize("N,K,E", RECOVER_CASES)
def test_recover_matches_the_model(N, K, E):
    import torch
    import polardecoding_amd as pa
    rng = np.random.default_rng(N * 7 + E)
    for ibil in (0, 1):
        dec = pa.SCdecode(N, K, E=E, ibil=bool(ibil))
        assert dec.E == E and dec.ibil == bool(ibil) and dec.rm_mode == M.mode_of(N, K, E)
        for B in (1, 63, 4177 if E < 4096 else 700):
            for dt in (np.float64, np.float32):
                x = (rng.standard_normal((B, E)) * 3).astype(dt)
                x[:, ::7] = -0.0
                tdt = torch.float64 if dt == np.float64 else torch.float32
                for sigma in (0.0, 0.8):
                    # rows start one element into the buffer: the head / tail path of every row
                    buf = torch.empty(B * E + 1, dtype=tdt, device="cuda")
                    buf[1:] = _cuda(x.reshape(-1))
                    d_in = buf[1:].view(B, E)
                    out = torch.full((B * N + 333,), 12345.0, dtype=tdt, device="cuda")
                    torch.cuda.synchronize()
                    dec.rm_recover_device(d_in, sigma=sigma, out=out)
                    dec.synchronize()
                    got = out.cpu().numpy()
                    want = M.recover(x, N, K, ibil, sigma=sigma, out_dtype=dt)
                    assert np.array_equal(got[:B * N].reshape(B, N).view(np.uint64 if dt == np.float64 else np.uint32),
                                          want.view(np.uint64 if dt == np.float64 else np.uint32)), (ibil, B, dt, sigma)
                    assert np.all(got[B * N:] == 12345.0)
        dec.close()


def _decoders(N, K, E, ibil, dtype):
    """(rate-matched decoder, plain decoder with the rate-matched order, label) for every algo"""
    import polardecoding_amd as pa
    A = K + 24
    io = pa.rm_info_order(N, A, E)
    ioK = pa.rm_info_order(N, K, E)
    kw = dict(dtype=dtype, E=E, ibil=ibil)
    pk = dict(dtype=dtype)
    out = [(pa.SCdecode(N, K, **kw), pa.SCdecode(N, K, info_order=ioK, **pk), "SC"),
           (pa.SCLdecode(N, K, L=8, **kw), pa.SCLdecode(N, K, L=8, info_order=ioK, **pk), "SCL8"),
           (pa.SCLdecode(N, K, L=32, **kw), pa.SCLdecode(N, K, L=32, info_order=ioK, **pk), "SCL32"),
           (pa.CASCL(N, K, L=8, **kw), pa.CASCL(N, K, L=8, info_order=io, **pk), "CASCL8"),
           (pa.CASCL(N, K, L=32, stages=(1, 8, 32), **kw), pa.CASCL(N, K, L=32, stages=(1, 8, 32), info_order=io, **pk), "adaptive"),
           (pa.SCFlip(N, K, T=8, **kw), pa.SCFlip(N, K, T=8, info_order=io, **pk), "SCF8"),
           (pa.BP(N, K, iterMax=30, **kw), pa.BP(N, K, iterMax=30, info_order=ioK, **pk), "BP"),
           (pa.BP(N, K, iterMax=30, early_stop="g", **kw), pa.BP(N, K, iterMax=30, early_stop="g", info_order=ioK, **pk), "BPstop")]
    return out


def _run(dec, x, label):
    """all per-frame outputs of a device decode: (u_hat, pm, flags, extra)"""
    import torch
    d = _cuda(x)
    B = d.shape[0]
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ex = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if label.startswith("BP"):
        bits = dec.decode_bp_device(d, iters=ex, flags=fl)
    elif label == "SCF8":
        bits = dec.decode_scf_device(d, flags=fl, attempts=ex)
    elif label in ("CASCL8", "adaptive"):
        bits = dec.decode_cascl_device(d, pm=pm, flags=fl, list_size=ex)
    else:
        bits = dec.decode_device(d, pm=pm, flags=fl)
    dec.synchronize()
    return _unpack(bits.cpu().numpy(), dec.N), pm.cpu().numpy(), fl.cpu().numpy(), ex.cpu().numpy()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("E,ibil", [(864, 0), (864, 1), (1153, 1)])
def test_decode_is_the_plain_decoder_on_the_recovered_rows(E, ibil, dtype):
    import torch
    import polardecoding_amd as pa
    N, K, B = 1024, 512, 700
    gen = pa.CASCL(N, K, L=8, E=E, ibil=bool(ibil))
    y = torch.empty((B, E), dtype=torch.float64, device="cuda")
    gen.generate_device(11, 0, 1.5, y, out_is_y=True)
    gen.synchronize()
    yh = y.cpu().numpy()
    sigma = 10 ** (-1.5 / 20)
    xin = yh.astype(np.float32) if dtype else yh
    llr = 2 * xin / xin.dtype.type(sigma) / xin.dtype.type(sigma)   # E-value LLR rows
    for rm, plain, label in _decoders(N, K, E, bool(ibil), dtype):
        A = rm.A
        got = _run(rm, llr, label)
        want = _run(plain, M.recover(llr, N, A, ibil), label)
        for g, w, nm in zip(got, want, ("u_hat", "pm", "flags", "extra")):
            assert np.array_equal(g, w), (label, nm, E, ibil, dtype)
        # the y form: recovery forms 2y/sigma/sigma per term
        d = _cuda(xin)
        if label.startswith("BP"):
            bits = rm.decode_bp_device(d, sigma=sigma)
            pbits = plain.decode_bp_device(_cuda(M.recover(xin, N, A, ibil, sigma=sigma)))
        else:
            bits = rm.decode_device(d, sigma=sigma)
            pbits = plain.decode_device(_cuda(M.recover(xin, N, A, ibil, sigma=sigma)))
        rm.synchronize()
        plain.synchronize()
        assert np.array_equal(bits.cpu().numpy(), pbits.cpu().numpy()), (label, "y input")
        rm.close()
        plain.close()


def test_sc_f64_equals_the_oracle_check_node(oracle):
    from test_scf_host import sc_run
    import polardecoding_amd as pa
    N, K = 128, 40
    for E in (100, 111, 300):
        rng = np.random.default_rng(E)
        llr = rng.standard_normal((64, E)) * 2 + 1.0
        rows = M.recover(llr, N, K, 0)
        frozen = np.ones(N, dtype=np.uint8)
        frozen[M.info_order(N, K, E)] = 0
        want, _ = sc_run(oracle, frozen, rows)
        dec = pa.SCdecode(N, K, E=E)
        uh, _, _ = dec.decode_batch(llr)
        assert np.array_equal(uh, want), E


GEN_CASES = [(1024, 512, 24, 864), (1024, 512, 24, 2051), (1024, 200, 24, 864), (1024, 200, 24, 641), (128, 40, 6, 100),
             (64, 20, 0, 45)]


@pytest.mark.parametrize("N,K,r,E", GEN_CASES)
def test_generator_against_the_model(N, K, r, E):
    import torch
    import polardecoding_amd as pa
    B = 512
    for ibil in (0, 1):
        if r:
            taps = CRC24C if r == 24 else CRC6
            rm = pa.CASCL(N, K, L=8, crc_taps=taps, E=E, ibil=bool(ibil))
            plain = pa.CASCL(N, K, L=8, crc_taps=taps, info_order=pa.rm_info_order(N, K + r, E))
        else:
            rm = pa.SCdecode(N, K, E=E, ibil=bool(ibil))
            plain = pa.SCdecode(N, K, info_order=pa.rm_info_order(N, K, E))
        A = rm.A
        out = torch.empty((B, E), dtype=torch.float64, device="cuda")
        ub = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        rm.generate_device(5, 100, 60.0, out, u_bits=ub, out_is_y=True)
        rm.synchronize()
        pout = torch.empty((B, N), dtype=torch.float64, device="cuda")
        pub = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        plain.generate_device(5, 100, 60.0, pout, u_bits=pub, out_is_y=True)
        plain.synchronize()
        assert torch.equal(ub, pub)
        u = _unpack(ub.cpu().numpy(), N)
        e = M.transmit(M.encode(u), E, A, ibil)
        y = out.cpu().numpy()
        assert np.array_equal(y < 0, e.astype(bool)), ibil
        # 0 dB: y - (1 - 2e) is N(0, 1) (sigma = 1)
        y0 = torch.empty((B, E), dtype=torch.float64, device="cuda")
        u0 = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        rm.generate_device(9, 0, 0.0, y0, u_bits=u0, out_is_y=True)
        rm.synchronize()
        e0 = M.transmit(M.encode(_unpack(u0.cpu().numpy(), N)), E, A, ibil)
        z = y0.cpu().numpy() - (1.0 - 2.0 * e0)
        n = z.size
        assert abs(z.mean()) < 5 / np.sqrt(n)
        assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / n)
        # sharding: frames [0, B) = [0, B/2) + [B/2, B); the LLR form in f32 too
        for tdt in (torch.float64, torch.float32):
            whole = torch.empty((B, E), dtype=tdt, device="cuda")
            rm.generate_device(3, 7, 1.0, whole)
            a = torch.empty((B // 2, E), dtype=tdt, device="cuda")
            b = torch.empty((B - B // 2, E), dtype=tdt, device="cuda")
            rm.generate_device(3, 7, 1.0, a)
            rm.generate_device(3, 7 + B // 2, 1.0, b)
            rm.synchronize()
            assert torch.equal(whole, torch.cat([a, b]))
        rm.close()
        plain.close()


FER_CASES = [(1024, 512, 1024), (1024, 512, 864), (1024, 512, 2048), (1024, 200, 864), (1024, 200, 640), (128, 40, 99)]


@pytest.mark.parametrize("N,K,E", FER_CASES)
def test_fer_batch_at_20_db_is_error_free(N, K, E):
    import polardecoding_amd as pa
    for ibil in (False, True):
        for dec in (pa.SCdecode(N, K, E=E, ibil=ibil), pa.SCLdecode(N, K, L=8, E=E, ibil=ibil),
                    pa.CASCL(N, K, L=8, E=E, ibil=ibil, dtype=pa.F32), pa.CASCL(N, K, L=32, stages=(1, 8, 32), E=E, ibil=ibil),
                    pa.SCFlip(N, K, E=E, ibil=ibil), pa.BP(N, K, iterMax=40, early_stop="g", E=E, ibil=ibil)):
            blk, bits = dec.fer_batch(1, 0, 20.0, 40000)
            assert (blk, bits) == (0, 0), (dec.kernel_name, E, ibil)
            dec.close()


def test_fer_at_E_equal_N_matches_the_plain_code():
    import polardecoding_amd as pa
    B = 1 << 16
    plain = pa.CASCL(1024, 512, L=8)
    pb, _ = plain.fer_batch(21, 0, 1.5, B)
    for ibil in (False, True):
        rm = pa.CASCL(1024, 512, L=8, E=1024, ibil=ibil)
        assert np.array_equal(rm.info_order, plain.info_order)
        rb, _ = rm.fer_batch(21, 0, 1.5, B)
        p = (pb + rb) / (2 * B)
        se = np.sqrt(2 * p * (1 - p) / B)
        assert abs(pb - rb) / B <= 4 * se + 1e-12, (pb, rb, ibil)
        assert rb > 0


def test_host_entry_points_and_refusals():
    import torch
    import polardecoding_amd as pa
    N, K, E = 128, 40, 99
    dec = pa.SCLdecode(N, K, L=8, E=E, ibil=True)
    plain = pa.SCLdecode(N, K, L=8, info_order=pa.rm_info_order(N, K, E))
    rng = np.random.default_rng(3)
    y = rng.standard_normal((300, E)) + 1.0
    uh, pm, fl = dec.decode_batch_y(y, 0.9)
    rows = M.recover(y, N, K, 1, sigma=0.9)
    uh2, pm2, fl2 = plain.decode_batch(rows)
    assert np.array_equal(uh, uh2) and np.array_equal(pm, pm2) and np.array_equal(fl, fl2)
    assert np.array_equal(dec(y[0], 0.9), uh2[0])
    u = uh2.copy()
    u[::3, plain.info_order[0]] ^= 1   # every third frame: one bit error on an information position
    assert dec.stop_rule_batch_y(y, 0.9, u, 10 ** 6) == (300, 100, 100)
    with pytest.raises(pa.PolarError):
        dec.decode_batch(y, frozen_mask=np.zeros(N, dtype=np.uint8))
    with pytest.raises(ValueError):
        dec.decode_batch(rng.standard_normal((3, N)))
    bp = pa.BP(N, K, iterMax=10, E=E)
    Et = torch.zeros((1, 8), dtype=torch.int64, device="cuda")
    with pytest.raises(pa.PolarError):
        bp.bp_readout_device(torch.zeros((4, E), dtype=torch.float64, device="cuda"),
                             torch.zeros((4, N // 32), dtype=torch.int32, device="cuda"), [5], Et)
    with pytest.raises(pa.PolarError):
        plain.rm_recover_device(torch.zeros((4, N), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        pa.CASCL(1024, 512, L=8, crc_file="CRC_6.dat", E=864)
    t = torch.zeros((4, E), dtype=torch.float64, device="cuda")
    assert dec.time_decode_device(t, torch.empty((4, N // 32), dtype=torch.int32, device="cuda"), 2) > 0


def test_polar_sim_fast_rate_matched():
    sim = os.path.join(REPO, "polardecoding_amd", "lib", "polar_sim")
    r = subprocess.run([sim, "--algo", "cascl", "--N", "1024", "--K", "512", "--L", "8", "--E", "864", "--ibil", "--fast",
                        "--snr", "3.0:3.0:1", "--ble", "20", "--batch", "16384"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [x for x in r.stdout.splitlines() if x.startswith("L = 8")][0]
    bler = float(line.split("BLER = ")[1].split()[0])
    assert 0 < bler < 0.5, line
