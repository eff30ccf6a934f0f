"""Frozen sets outside the 5G reliability order (a plain helper module, imported by tests/test_frozen_patterns_host.py,
tests/test_gpu_frozen_patterns.py and tools/stress_parity.py --patterns).

The library takes any information set (polar_cfg.info_order, the frozen_mask override, polar_decode_llr), and the tuned
kernels take their control flow from the set alone: the leading all-frozen run and the per-octet form of the list kernels,
frozen_span / live / fuse / below and the block tests of the one-codeword-per-lane kernels, the per-leaf frozen word of
k_scl_big, the priors of BP.  Sets cut from the 5G order reach 13 of the 256 octet masks, never unfreeze leaf 0 and never
freeze the last leaf (tests/test_frozen_patterns_host.py asserts these figures).  families(N) makes the other shapes:

  octets_lo, octets_hi    N >= 1024: seeded shuffles of the octet masks 0x00..0x7F and 0x80..0xFF (bit k of a mask = leaf
                          8 o + k frozen), one shuffle per 128 octets; together every mask value occurs.  Below, a seeded
                          sample of N / 8 masks of each half that holds 0x00, 0x55, 0x7F (lo) and 0x80, 0xFE, 0xFF (hi).
                          Octet 0 is never 0xFF.
  islands_s_a, islands_s_b  s = 8 .. 256 while s < N: (j // s) & 1 and its complement -- all-information and all-frozen
                          spans alternate in both phases at every level.
  lead_P                  P = 14, 15, 16, 17 and N / 8 - 1 (where below N / 8): exactly P leading all-frozen octets, leaf 8 P
                          information, the rest Bernoulli(0.5).  lead_mid (N >= 256): the run ends at leaf 8 * 15 + 3.
  leaf0, leaf0_run        leaves 0, 1, 2 information and leaf 3 frozen / the first 40 leaves information (N >= 64); the
                          rest Bernoulli(0.5).  The list forks before the first frozen leaf and fills in the first octets.
  tail_1, tail_8, tail_32 (N >= 64), tail_quarter   the last leaf / octet / 32-leaf block / quarter frozen, the rest
                          Bernoulli(0.5).
  sparse_last, sparse_first, sparse_5_half, sparse_1_2_penult   information sets {N-1}, {0}, {5, N/2}, {1, 2, N-2}: fewer
                          forks than log2 L for the larger lists, so the list never fills.
  dense_all, dense_but_first, dense_but_last, dense_but_block   everything information / all but leaf 0 / all but leaf
                          N - 1 / all but the 32-leaf block at N / 2.
  bern_0.1, bern_0.5, bern_0.9   every leaf frozen with that probability.
  anti5g                  (N <= 1024) the N / 2 LEAST reliable positions of the 5G order as the information set.

Every mask is uint8 [N] (1 = frozen) with at least one information leaf, and a function of (N, name) alone.
order_of(mask, seed) is a seeded permutation of the information positions (an info_order: the CRC positions I[0..r) land
anywhere in the set); q_of(mask, order) the reliability order that makes oracle.Code reproduce it.  NO_CRC[N] lists the
families whose A = K + r unfrozen leaves cannot carry the CRC used at that N (A <= r); CRC_R[N] is that r."""
import os
import zlib
from collections import OrderedDict

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ISLAND_SPANS = (8, 16, 32, 64, 128, 256)
LEADS = (14, 15, 16, 17)
CRC_R = {128: 6, 1024: 24}   # CRC-6 of CASCL_128.c at N = 128, CRC-24C at N = 1024
# families with A <= r there: no CA-SCL, no SC-Flip (tests/test_frozen_patterns_host.py holds the lists to the masks)
NO_CRC = {
    128: ("lead_15", "sparse_last", "sparse_first", "sparse_5_half", "sparse_1_2_penult"),
    1024: ("lead_127", "sparse_last", "sparse_first", "sparse_5_half", "sparse_1_2_penult"),
}


def _rng(N, name):
    return np.random.default_rng([N, zlib.crc32(name.encode())])


def _bern(N, name, p=0.5):
    return (_rng(N, name).random(N) < p).astype(np.uint8)


def from_octets(octets):
    """octet masks [N/8] (bit k = leaf 8 o + k frozen) -> frozen mask uint8 [N]"""
    o = np.asarray(octets, dtype=np.uint8)
    return ((o[:, None] >> np.arange(8, dtype=np.uint8)) & 1).astype(np.uint8).reshape(-1)


def octets_of(mask):
    """frozen mask [N] -> its N/8 octet masks"""
    m = np.asarray(mask, dtype=np.uint8).reshape(-1, 8)
    return (m << np.arange(8, dtype=np.uint8)).sum(axis=1).astype(np.uint8)


def leading_frozen_octets(mask):
    o = octets_of(mask)
    lead = 0
    while lead < o.size and o[lead] == 0xFF:
        lead += 1
    return lead


def _octet_family(N, name, lo, must):
    rng = _rng(N, name)
    half = np.arange(lo, lo + 128)
    count = N // 8
    if count >= 128:
        out = np.concatenate([rng.permutation(half) for _ in range(count // 128)])
    else:
        rest = rng.permutation(np.setdiff1d(half, must))[:count - len(must)]
        out = rng.permutation(np.concatenate([np.asarray(must), rest]))
    if out[0] == 0xFF:   # the leading run stays 0 here: lead_P has the runs
        k = int(np.flatnonzero(out != 0xFF)[0])
        out[0], out[k] = out[k], out[0]
    return from_octets(out)


def q5g(N):
    """the 5G reliability order restricted to < N (ascending reliability); N <= 1024"""
    vals = []
    with open(os.path.join(REPO, "polardecoding_amd", "data", "q5g_nmax1024.txt")) as f:
        for line in f:
            if not line.startswith("#"):
                vals += [int(x) for x in line.split()]
    return [x for x in vals if x < N]


def families(N):
    """OrderedDict name -> frozen mask uint8 [N] (1 = frozen); see the module docstring"""
    assert N >= 32 and N & (N - 1) == 0
    j = np.arange(N)
    fam = OrderedDict()
    fam["octets_lo"] = _octet_family(N, "octets_lo", 0x00, (0x00, 0x55, 0x7F))
    fam["octets_hi"] = _octet_family(N, "octets_hi", 0x80, (0x80, 0xFE, 0xFF))
    for s in ISLAND_SPANS:
        if s < N:
            fam[f"islands_{s}_a"] = ((j // s) & 1).astype(np.uint8)
            fam[f"islands_{s}_b"] = (1 - ((j // s) & 1)).astype(np.uint8)
    for P in sorted(set(p for p in LEADS + (N // 8 - 1,) if 0 < p < N // 8)):
        m = _bern(N, f"lead_{P}")
        m[:8 * P] = 1
        m[8 * P] = 0
        fam[f"lead_{P}"] = m
    if N >= 256:
        m = _bern(N, "lead_mid")
        m[:8 * 15 + 3] = 1
        m[8 * 15 + 3] = 0
        fam["lead_mid"] = m
    m = _bern(N, "leaf0")
    m[:3] = 0
    m[3] = 1
    fam["leaf0"] = m
    if N >= 64:
        m = _bern(N, "leaf0_run")
        m[:40] = 0
        fam["leaf0_run"] = m
    for name, w in (("tail_1", 1), ("tail_8", 8), ("tail_32", 32), ("tail_quarter", N // 4)):
        if w < N:
            m = _bern(N, name)
            m[N - w:] = 1
            fam[name] = m
    for name, info in (("sparse_last", (N - 1,)), ("sparse_first", (0,)), ("sparse_5_half", (5, N // 2)),
                       ("sparse_1_2_penult", (1, 2, N - 2))):
        m = np.ones(N, dtype=np.uint8)
        m[list(info)] = 0
        fam[name] = m
    fam["dense_all"] = np.zeros(N, dtype=np.uint8)
    for name, sl in (("dense_but_first", slice(0, 1)), ("dense_but_last", slice(N - 1, N)),
                     ("dense_but_block", slice(N // 2, N // 2 + 32))):
        m = np.zeros(N, dtype=np.uint8)
        m[sl] = 1
        fam[name] = m
    for p in (0.1, 0.5, 0.9):
        fam[f"bern_{p}"] = _bern(N, f"bern_{p}", p)
    if N <= 1024:
        m = np.ones(N, dtype=np.uint8)
        m[q5g(N)[:N // 2]] = 0
        fam["anti5g"] = m
    for name, m in fam.items():
        assert m.dtype == np.uint8 and m.shape == (N,) and m.max() <= 1 and (m == 0).any(), name
    return fam


def select(fam, *prefixes):
    """the families whose name starts with one of the prefixes, in order"""
    return OrderedDict((k, v) for k, v in fam.items() if k.startswith(prefixes))


def with_crc(fam, N):
    """the families that can carry the CRC used at N (all but NO_CRC[N])"""
    return OrderedDict((k, v) for k, v in fam.items() if k not in NO_CRC[N])


def order_of(mask, seed):
    """a seeded permutation of the information positions of `mask`: an info_order (int32 [A])"""
    info = np.flatnonzero(np.asarray(mask) == 0)
    return np.random.default_rng([int(seed), info.size]).permutation(info).astype(np.int32)


def q_of(mask, order):
    """reliability order [N] for oracle.Code(N, A - r, taps, Q=...): the frozen positions, then `order`"""
    return np.flatnonzero(np.asarray(mask) != 0).tolist() + [int(x) for x in order]
