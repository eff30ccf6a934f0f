"""GPU: every value the device-side transmit chain produces, against tests/gen_model.py -- an independent numpy statement of
the documented rule (Philox4x32-10 with counter (frame lo, frame hi, block, stream) and key (seed lo, seed hi), Box-Muller on
53-bit uniforms, y = +-1 + sigma z, LLR = 2 * y / sigma / sigma).  The kernels: k_generate, k_generate_dyn, k_generate_rm
(polar_generate_device) and k_genie_rows (polar_genie_rows_device).

Exact, by ==: the reported u bits against the model's u, for every code variant of the chain; the sign of y against x at 60 dB,
where sigma |z| <= 1e-3 * 8.66 < 1 for every z the generator can produce.
By value: f64 outputs within gen_model.f64_bound (per-operation error bounds propagated through the chain, a function of the
model's sigma |z| and |y|; the per-operation figures are assumed, see DESIGN.md "Generator values"); f32 outputs within one
ulp32 of float32(model), and equal to it wherever the model value is further than the f64 bound from a rounding midpoint.
Every case runs over the counter edges: a seed with a high word, a batch across frame 2^32, frames above 2^40, B = 1, B = 5.
Each test prints the largest observed error in units of the bound."""
import os

import numpy as np
import pytest

import gen_model as G
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LD = np.longdouble
CRC6 = (0, 5, 6)
CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)
CRC32 = (0, 1, 2, 4, 5, 7, 8, 10, 11, 12, 16, 22, 23, 26, 32)
GUARD = 1024            # elements behind every output that the kernel must leave alone
SNRS = (0.0, 1.5, -3.0)   # sigma = 1 exactly, < 1, > 1
# (seed, first_frame, B): a seed with a high word and a batch across the carry into the counter's second word; frames above
# 2^40 and a batch that is no multiple of a workgroup's four waves; one frame
EDGES = ((0x9E3779B97F4A7C15, 2 ** 32 - 3, 8), (0xC0FFEE, 2 ** 40 + 12345, 5), (0x1F00000002, 2 ** 63 + 1, 1))
WORST = {}              # kernel -> largest |device - model| / bound seen, f64


# ---- the code variants --------------------------------------------------------------------------------------------------------
# id -> (kernel, constructor, model keywords).  K below 32, a multiple of 32 and one past it; N = 64 (one element per lane,
# the second normal of a block unused), 128, 1024, 4096 (all 64 bits of the lane word).
def _cases():
    import polardecoding_amd as pa
    c = {}

    def plain(name, make, **kw):
        c[name] = ("k_generate", make, kw)

    plain("nocrc-64-20", lambda: pa.SCLdecode(64, 20, L=8))
    plain("nocrc-128-64", lambda: pa.SCLdecode(128, 64, L=8))
    plain("nocrc-1024-513", lambda: pa.SCLdecode(1024, 513, L=8))
    plain("nocrc-4096-2048", lambda: pa.SCLdecode(4096, 2048, L=8))
    plain("crc6-64-24", lambda: pa.CASCL(64, 24, L=8, crc_taps=CRC6), taps=CRC6)
    plain("crc6-128-65", lambda: pa.CASCL(128, 65, L=8, crc_taps=CRC6), taps=CRC6)
    plain("crc24c-1024-512", lambda: pa.CASCL(1024, 512, L=8), taps=CRC24C)
    plain("crc24c-4096-2049", lambda: pa.CASCL(4096, 2049, L=8), taps=CRC24C)
    plain("crc32-128-33", lambda: pa.CASCL(128, 33, L=8, crc_taps=CRC32), taps=CRC32)          # the tap-32 branch
    plain("crc32-1024-480", lambda: pa.CASCL(1024, 480, L=8, crc_taps=CRC32), taps=CRC32)
    plain("syscrc6-64-20", lambda: pa.CASCL(64, 20, L=8, crc_taps=CRC6, systematic=True), taps=CRC6, systematic=True)
    plain("syscrc24c-1024-512", lambda: pa.CASCL(1024, 512, L=8, systematic=True), taps=CRC24C, systematic=True)
    plain("syscrc24c-1024-97", lambda: pa.CASCL(1024, 97, L=8, systematic=True), taps=CRC24C, systematic=True)
    plain("syscrc32-128-64", lambda: pa.CASCL(128, 64, L=8, crc_taps=CRC32, systematic=True), taps=CRC32, systematic=True)
    plain("crcfile-128-64", lambda: pa.CASCL(128, 64, L=8, crc_file=os.path.join(GOLDEN, "CRC_6.dat"), systematic=True),
          crc_file=True)
    plain("syspolar-64-20", lambda: pa.SCdecode(64, 20, sys_polar=True), sys_polar=True)
    plain("syspolar-128-65", lambda: pa.CASCL(128, 65, L=8, crc_taps=CRC6, sys_polar=True), taps=CRC6, sys_polar=True)
    plain("syspolar-1024-512", lambda: pa.CASCL(1024, 512, L=8, sys_polar=True), taps=CRC24C, sys_polar=True)
    plain("syspolar-4096-2048", lambda: pa.SCLdecode(4096, 2048, L=8, sys_polar=True), sys_polar=True)

    def dyn(name, make, **kw):
        c[name] = ("k_generate_dyn", make, dict(kw, dyn=True))

    dyn("pac-64-31", lambda: pa.PAC(64, 31, L=8))
    dyn("pac-128-64", lambda: pa.PAC(128, 64, L=8))
    dyn("pac-1024-513", lambda: pa.PAC(1024, 513, L=8))
    dyn("pc5g-64-14", lambda: pa.PCCASCL(64, 14, n_pc=3, n_pc_wm=1, L=8), taps=CRC6)
    dyn("pc5g-1024-512", lambda: pa.PCCASCL(1024, 512, L=8, crc_taps=CRC24C), taps=CRC24C)

    def rm(name, N, K, taps, E):
        for ibil in (False, True):
            kw = dict(E=E, ibil=ibil)
            make = (lambda kw=kw: pa.CASCL(N, K, L=8, crc_taps=taps, **kw)) if taps else (lambda kw=kw: pa.SCdecode(N, K, **kw))
            c[f"{name}-{N}-{K}-E{E}" + ("-ibil" if ibil else "")] = ("k_generate_rm", make, dict(taps=taps, rm=(E, ibil)))

    rm("repeat", 64, 20, None, 97)           # E odd: the last block's second normal unused
    rm("repeat", 1024, 512, CRC24C, 2051)
    rm("puncture", 128, 33, None, 100)
    rm("puncture", 1024, 200, CRC24C, 864)
    rm("shorten", 64, 20, None, 45)
    rm("shorten", 128, 40, CRC6, 100)
    rm("shorten", 1024, 513, CRC24C, 865)
    for N, K in ((64, 20), (1024, 512)):      # E = N: the rows of test_the_two_box_muller_copies_agree (not in CASE_IDS)
        c[f"copy-{N}-{K}"] = ("k_generate_rm", lambda N=N, K=K: pa.SCdecode(N, K, E=N), dict(taps=None, rm=(N, False)))
    return c


CASE_IDS = ["nocrc-64-20", "nocrc-128-64", "nocrc-1024-513", "nocrc-4096-2048", "crc6-64-24", "crc6-128-65", "crc24c-1024-512",
            "crc24c-4096-2049", "crc32-128-33", "crc32-1024-480", "syscrc6-64-20", "syscrc24c-1024-512", "syscrc24c-1024-97",
            "syscrc32-128-64", "crcfile-128-64", "syspolar-64-20", "syspolar-128-65", "syspolar-1024-512", "syspolar-4096-2048",
            "pac-64-31", "pac-128-64", "pac-1024-513", "pc5g-64-14", "pc5g-1024-512"]
CASE_IDS += [f"{n}{s}" for n in ("repeat-64-20-E97", "repeat-1024-512-E2051", "puncture-128-33-E100", "puncture-1024-200-E864",
                                 "shorten-64-20-E45", "shorten-128-40-E100", "shorten-1024-513-E865") for s in ("", "-ibil")]


class Case:
    """one decoder and what the model needs to know about it"""

    def __init__(self, cid):
        import polardecoding_amd as pa
        from polardecoding_amd import crcfile
        self.kernel, make, kw = _cases()[cid]
        self.dec = make()
        d = self.dec
        self.N, self.K, self.W = d.N, d.K, d.E
        self.model = dict(taps=kw.get("taps"), systematic=kw.get("systematic", False), sys_polar=kw.get("sys_polar", False))
        if kw.get("crc_file"):
            self.model["Gc"] = crcfile.load(os.path.join(GOLDEN, "CRC_6.dat"))
        if kw.get("dyn"):
            pos = d.dyn_positions
            if hasattr(d, "pac_g"):
                self.model["dyn"] = pa.dyn_pac(d.N, d.info_order, d.pac_g)
            else:
                r = max(kw["taps"])
                q = pa.q_sequence(d.N)
                p, sets, io = pa.dyn_pc5g(d.N, q[d.N - (d.K + r + len(pos)):], len(pos), 1 if self.N == 64 else 0)
                assert np.array_equal(io, d.info_order)
                self.model["dyn"] = (p, sets)
            assert np.array_equal(self.model["dyn"][0], pos)
        self.rm = kw.get("rm")
        self.kind = "rows" if self.rm else "plain"
        self._z = {}

    def bits(self, seed, frames):
        """(u [B][N], sent bits [B][W])"""
        u = G.u_rows(seed, frames, self.N, self.K, self.dec.info_order, **self.model)
        x = G.encode(u)
        if self.rm:
            x = G.RM.transmit(x, self.rm[0], self.dec.A, self.rm[1])
        return u, x

    def z(self, seed, frames):
        key = (seed, frames.tobytes())
        if key not in self._z:
            self._z[key] = G.noise(seed, frames, self.kind, self.W)
        return self._z[key]

    def run(self, seed, first, B, snr_db, f32=False, out_is_y=False, want_u=True):
        """polar_generate_device -> (out [B][W], u bits [B][N] or None); the guard behind the output is checked"""
        import torch
        tdt = torch.float32 if f32 else torch.float64
        buf = torch.full((B * self.W + GUARD,), 12345.0, dtype=tdt, device="cuda")
        ub = torch.zeros((B, self.N // 32), dtype=torch.int32, device="cuda") if want_u else None
        self.dec.generate_device(seed, first, snr_db, buf[:B * self.W].view(B, self.W), ub, out_is_y=out_is_y)
        self.dec.synchronize()
        h = buf.cpu().numpy()
        assert (h[B * self.W:] == 12345.0).all(), "the generator wrote beyond its output"
        u = None
        if want_u:
            w = ub.cpu().numpy().view(np.uint32)
            u = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, self.N).astype(np.uint8)
        return h[:B * self.W].reshape(B, self.W), u


def _check_values(kernel, got, ref, bound, what):
    """f64: |got - ref| <= bound per element; f32: one ulp32, and equality away from the rounding midpoints"""
    if got.dtype == np.float64:
        ratio = np.abs(got.astype(LD) - ref) / bound
        worst = float(ratio.max())
        WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        assert worst <= 1.0, (kernel, what, "element", i, "got", float(got[i]), "model", float(ref[i]), "error / bound", worst)
        return worst
    within, need, ok = G.f32_check(got, ref, bound)
    assert within.all(), (kernel, what, "more than one ulp32 off at", np.argwhere(~within)[:4].tolist())
    bad = need & ~ok
    assert not bad.any(), (kernel, what, "float32(model) required at", np.argwhere(bad)[:4].tolist())
    assert need.mean() > 0.999          # nearly every element is held to equality
    return None


@pytest.mark.parametrize("cid", CASE_IDS)
def test_generator_bits_and_values(cid):
    """u bits by ==, sign of y by == at 60 dB, and every value in the y and LLR forms, f64 and f32, at three sigmas, each
    combination on one of the counter edges (every edge sees f64 and f32, y and LLR)"""
    c = Case(cid)
    worst, run = 0.0, 0
    for seed, first, B in EDGES:
        frames = G.frames_of(first, B)
        u, x = c.bits(seed, frames)
        y, du = c.run(seed, first, B, 60.0, out_is_y=True)
        assert np.array_equal(du, u), (cid, "u bits", hex(seed), first)
        assert np.array_equal(y < 0, x.astype(bool)), (cid, "sign of y", hex(seed), first)
    for out_is_y in (True, False):
        for f32 in (False, True):
            for snr in SNRS:
                seed, first, B = EDGES[run % len(EDGES)]
                run += 1
                frames = G.frames_of(first, B)
                u, x = c.bits(seed, frames)
                ref, bound = G.channel(x, c.z(seed, frames), G.sigma_of(snr), out_is_y)
                got, du = c.run(seed, first, B, snr, f32=f32, out_is_y=out_is_y, want_u=(run % 2 == 0))
                assert du is None or np.array_equal(du, u)
                w = _check_values(c.kernel, got, ref, bound, (cid, snr, "y" if out_is_y else "llr", hex(seed), first, B))
                worst = max(worst, w or 0.0)
    print(f"\n{c.kernel} {cid}: largest f64 error {worst:.3f} of the bound (kernel so far {WORST[c.kernel]:.3f})")
    c.dec.close()


def test_sigma_is_exact_at_0_db_and_the_llr_order_is_kept():
    """sigma = 10^(-0/20) = 1: y and the LLR are y and 2 y exactly, so the two forms of one frame differ by the doubling alone"""
    c = Case("crc24c-1024-512")
    assert G.sigma_of(0.0) == 1.0
    seed, first, B = EDGES[0]
    y, _ = c.run(seed, first, B, 0.0, out_is_y=True)
    llr, _ = c.run(seed, first, B, 0.0, out_is_y=False)
    assert np.array_equal(llr, 2 * y)
    # the documented order 2 * y / sigma / sigma, in binary64, from the device's own y
    s = np.float64(G.sigma_of(1.5))
    y, _ = c.run(seed, first, B, 1.5, out_is_y=True)
    llr, _ = c.run(seed, first, B, 1.5, out_is_y=False)
    assert np.array_equal(llr, 2 * y / s / s)
    c.dec.close()


def test_n_below_64_stays_einval():
    import torch
    import polardecoding_amd as pa
    dec = pa.SCdecode(32, 16)
    out = torch.zeros((4, 32), dtype=torch.float64, device="cuda")
    with pytest.raises(pa.PolarError, match=r"rc=-1\)"):
        dec.generate_device(1, 0, 1.0, out)
    dec.synchronize()
    assert not out.any()
    dec.close()


@pytest.mark.parametrize("cid", ["crc6-64-24", "pc5g-64-14", "shorten-64-20-E45-ibil"])
def test_grid_stride_second_trip(cid):
    """N = 64 and a batch just above num_cu * 8 workgroups * 4 waves: the last frames are a workgroup's second trip through the
    frame loop.  The first frames (across frame 2^32), the frames round the boundary and the last frames are compared."""
    import torch
    c = Case(cid)
    per_trip = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4
    B = per_trip + 5
    seed, first = EDGES[0][0], 2 ** 32 - 3
    got, du = c.run(seed, first, B, 1.5)
    got32, _ = c.run(seed, first, B, -3.0, f32=True, out_is_y=True, want_u=False)
    sel = np.array(sorted(set(list(range(8)) + list(range(per_trip - 4, B)))))
    frames = G.frames_of(first, B)[sel]
    u, x = c.bits(seed, frames)
    assert np.array_equal(du[sel], u)
    z = c.z(seed, frames)
    ref, bound = G.channel(x, z, G.sigma_of(1.5), False)
    w = _check_values(c.kernel, got[sel], ref, bound, (cid, "second trip"))
    ref, bound = G.channel(x, z, G.sigma_of(-3.0), True)
    _check_values(c.kernel, got32[sel], ref, bound, (cid, "second trip, f32 y"))
    print(f"\n{c.kernel} {cid} B = {B}: largest f64 error {w:.3f} of the bound")
    c.dec.close()


# ---- design rows -------------------------------------------------------------------------------------------------------------
def _genie(dec, seed, first, sigma, B, f32):
    import torch
    N = dec.N
    buf = torch.full((B * N + GUARD,), 12345.0, dtype=torch.float32 if f32 else torch.float64, device="cuda")
    dec.genie_rows_device(seed, first, sigma, buf[:B * N].view(B, N))
    dec.synchronize()
    h = buf.cpu().numpy()
    assert (h[B * N:] == 12345.0).all(), "k_genie_rows wrote beyond its output"
    return h[:B * N].reshape(B, N)


@pytest.mark.parametrize("N", [64, 128, 1024])
def test_genie_rows_values(N):
    """k_genie_rows: element e of frame f is 2 * (1 + sigma z) / sigma / sigma, z = normal (e & 1) of block e >> 1, stream 2"""
    import polardecoding_amd as pa
    dec = pa.SCdecode(N, N // 2)
    worst, run = 0.0, 0
    for sigma in (1.0, 0.8):
        for f32 in (False, True):
            seed, first, B = EDGES[run % len(EDGES)]
            run += 1
            frames = G.frames_of(first, B)
            ref, bound = G.channel(np.zeros((B, N), dtype=np.uint8), G.noise(seed, frames, "rows", N), sigma, False)
            w = _check_values("k_genie_rows", _genie(dec, seed, first, sigma, B, f32), ref, bound, (N, sigma, hex(seed), first))
            worst = max(worst, w or 0.0)
    print(f"\nk_genie_rows N = {N}: largest f64 error {worst:.3f} of the bound")
    dec.close()


def test_genie_rows_grid_stride_second_trip():
    """more pairs than num_cu * 16 workgroups * 256 threads: the last frames are written on a thread's second trip"""
    import torch
    import polardecoding_amd as pa
    N = 1024
    dec = pa.SCdecode(N, N // 2)
    per_trip = torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256 // (N // 2)
    B = per_trip + 3
    seed, first = EDGES[0][0], 2 ** 32 - 3
    got = _genie(dec, seed, first, 0.8, B, False)
    sel = np.array(sorted(set(list(range(6)) + list(range(per_trip - 3, B)))))
    frames = G.frames_of(first, B)[sel]
    ref, bound = G.channel(np.zeros((len(sel), N), dtype=np.uint8), G.noise(seed, frames, "rows", N), 0.8, False)
    w = _check_values("k_genie_rows", got[sel], ref, bound, "second trip")
    print(f"\nk_genie_rows B = {B}: largest f64 error {w:.3f} of the bound")
    dec.close()


@pytest.mark.parametrize("N,K", [(64, 20), (1024, 512)])
def test_the_two_box_muller_copies_agree(N, K):
    """At E = N the sent position t of k_generate_rm and element t of k_genie_rows take the same normal ((t & 1) of block
    t >> 1, stream 2) from two copies of the Box-Muller.  Both are held to the model; as f64 LLRs at the same sigma they are
    equal by == wherever the sent bit is 0 (the design row is the all-zero codeword; the payload of a generated frame cannot
    be set, so the positions that carry a 1 are compared through the model only)."""
    import polardecoding_amd as pa
    rm = Case(f"copy-{N}-{K}")
    assert rm.dec.rm_mode == pa.RM_REPEAT and rm.W == N
    plain = pa.SCdecode(N, K)
    for (seed, first, B), snr in zip(EDGES, SNRS):
        sigma = G.sigma_of(snr)
        frames = G.frames_of(first, B)
        u, e = rm.bits(seed, frames)
        z = rm.z(seed, frames)
        a, du = rm.run(seed, first, B, snr)
        b = _genie(plain, seed, first, sigma, B, False)
        assert np.array_equal(du, u)
        ref, bound = G.channel(e, z, sigma, False)
        _check_values("k_generate_rm", a, ref, bound, ("copy", N, snr))
        ref0, bound0 = G.channel(np.zeros_like(e), z, sigma, False)
        _check_values("k_genie_rows", b, ref0, bound0, ("copy", N, snr))
        zero = e == 0
        assert zero.any() and (~zero).any()
        assert np.array_equal(a[zero], b[zero]), (N, snr)
    rm.dec.close()
    plain.close()
