"""CPU: adaptive CA-SCL (polar_cascl_set_stages, include/polar_hip.h).

A numpy restatement of the CRC syndrome of a decision -- XOR over {j : u_j = 1} of crc_tab[j], crc_tab[I[i]] = D^i mod g(D)
-- checked against the sent u of the oracle's transmit chain (non-systematic and systematic, CRC-24C and the CRC-6 of
CASCL_128.c), and compose(), the rule's definition of a frame's output from the outputs of its stages.
tests/test_gpu_cascl_adaptive.py reuses both.  Also: the new C ABI is declared and exported."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_CRC_PASS = 2
CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)
CRC6 = (0, 5, 6)


def crc_table(N, info_order, taps):
    """crc_tab[N]: D^i mod g(D) at position I[i] (bit k = coefficient of D^k), 0 at the other positions."""
    r = max(taps)
    glow = sum(1 << t for t in taps if t < r)
    tab = np.zeros(N, dtype=np.uint64)
    rem = 1
    for j in info_order:
        tab[int(j)] = rem
        rem <<= 1
        if rem >> r:
            rem ^= (1 << r) | glow
    return tab


def syndrome(u, info_order, taps):
    """CRC syndrome of decisions u ([N] or [B][N], 0/1): 0 iff the CRC passes."""
    u = np.asarray(u)
    tab = crc_table(u.shape[-1], info_order, taps)
    return np.bitwise_xor.reduce(np.where(u != 0, tab, np.uint64(0)), axis=-1)


def compose(stage_outputs, passes):
    """The rule's output.  stage_outputs: per stage (L, u_hat [B][N], pm [B], flags [B]) over ALL frames; passes: per stage
    bool [B].  A frame takes the outputs of the first stage it passes, else those of the last.
    Returns (u_hat, pm, flags, list size)."""
    L0, uh, pm, fl = stage_outputs[0]
    uh, pm, fl = np.array(uh), np.array(pm), np.array(fl)
    ls = np.full(len(pm), L0, dtype=np.int64)
    todo = ~np.asarray(passes[0], dtype=bool)
    for (L, u_s, pm_s, fl_s), p in zip(stage_outputs[1:], passes[1:]):
        uh[todo], pm[todo], fl[todo], ls[todo] = np.asarray(u_s)[todo], np.asarray(pm_s)[todo], np.asarray(fl_s)[todo], L
        todo &= ~np.asarray(p, dtype=bool)
    return uh, pm, fl, ls


CODES = [(1024, 512, CRC24C, False), (1024, 512, CRC24C, True), (128, 64, CRC6, False), (128, 64, CRC6, True)]


@pytest.mark.parametrize("N,K,taps,sys_", CODES)
def test_syndrome_is_zero_on_sent_frames(N, K, taps, sys_, oracle):
    code = oracle.Code(N, K, taps, systematic=sys_)
    sim = oracle.Sim(77 + N + int(sys_))
    us, _ = sim.frames(code, oracle.sigma_from_db(2.0), 20)
    assert us.any()
    assert (syndrome(us, code.info_order, taps) == 0).all()


@pytest.mark.parametrize("N,K,taps,sys_", CODES)
def test_syndrome_sees_every_single_flip(N, K, taps, sys_, oracle):
    code = oracle.Code(N, K, taps, systematic=sys_)
    sim = oracle.Sim(91 + N)
    u, _ = sim.frame(code, oracle.sigma_from_db(2.0))
    flips = np.repeat(u[None, :], code.A, axis=0)
    flips[np.arange(code.A), code.info_order] ^= 1
    assert (syndrome(flips, code.info_order, taps) != 0).all()


def test_crc_table_is_the_oracles_division(oracle):
    """The table restates the reference's CRcheck (long division of C[i] = u[I[i]] by g): on the oracle's CA-SCL decisions
    of noisy frames the syndrome is zero on every frame it decoded correctly."""
    code = oracle.Code(128, 64, CRC6)
    sim = oracle.Sim(5)
    sig = oracle.sigma_from_db(1.0)
    us, ys = sim.frames(code, sig, 60)
    llr = np.stack([oracle.llr_from_y(y, sig) for y in ys])
    uh, _, _ = oracle.decode(code, llr, "CASCL", L=2)
    s = syndrome(uh, code.info_order, CRC6)
    ok = (uh == us).all(axis=1)
    assert (s[ok] == 0).all() and ok.any() and (~ok).any()


def test_compose():
    B, N = 6, 4
    st = [(1, np.zeros((B, N), int), np.zeros(B), np.array([2, 0, 0, 2, 0, 0])),
          (8, np.ones((B, N), int), np.full(B, 8.0), np.array([2, 2, 0, 2, 0, 0])),
          (32, np.full((B, N), 3), np.full(B, 32.0), np.array([0, 2, 2, 0, 0, 1]))]
    passes = [(s[3] & FLAG_CRC_PASS) != 0 for s in st]
    uh, pm, fl, ls = compose(st, passes)
    assert ls.tolist() == [1, 8, 32, 1, 32, 32]
    assert pm.tolist() == [0.0, 8.0, 32.0, 0.0, 32.0, 32.0]
    assert fl.tolist() == [2, 2, 2, 2, 0, 1]
    assert (uh[1] == 1).all() and (uh[4] == 3).all() and (uh[0] == 0).all()


def test_adaptive_abi_is_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    for name in ("polar_cascl_set_stages", "polar_cascl_decode_device", "polar_cascl_decode_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    lib = os.path.join(REPO, "polardecoding_amd", "lib", "libpolar_hip.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build())"
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in ("polar_cascl_set_stages", "polar_cascl_decode_device", "polar_cascl_decode_batch"):
        assert re.search(r"\b" + name + r"\b", out), name
