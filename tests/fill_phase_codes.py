"""The codes of the pair kernel's list-filling phase (csrc/scl_fast2.h fill_phase()) and the rule that chooses where the
phase ends, restated.  tests/test_fill_phase_host.py holds polar_fill_phase_end to the restatement on every code here;
tests/test_gpu_fast2_fill_phase.py decodes them.

The rule (N = 1024; csrc/h_code.hip fill_phase_end): E is the largest of 256, 192, 128 with
  (a) at most three information leaves below E,
  (b) each of them one of the last two leaves of its 64-leaf block, and none below leaf 126,
  (c) for E > 128, exactly one of them below leaf 128 and no other one below E - 64 (exactly two paths enter every block
      behind leaf 128),
and 0 if there is none or E <= 8 * lead, lead = min(15, leading all-frozen octets).  (b) and (c) are narrower than "every
information leaf below E is one of the last two leaves of its 64-leaf block": the first 128 leaves are one butterfly, and a
later block is decoded for two paths.

A code is (name, algo, crc taps or None, information leaves in the order the CRC table takes them, expected E)."""
import numpy as np

N = 1024


def rule(info):
    frozen = np.ones(N, dtype=bool)
    frozen[np.asarray(info)] = False
    lead = 0
    while lead < 15 and frozen[8 * lead:8 * lead + 8].all():
        lead += 1
    for E in (256, 192, 128):
        below = [j for j in range(E) if not frozen[j]]
        ok = all(j % 64 >= 62 and j >= 126 for j in below) and len(below) <= 3
        if E > 128 and not (sum(j < 128 for j in below) == 1 and sum(j < E - 64 for j in below) == 1):
            ok = False
        if ok and E > 8 * lead:
            return E
    return 0


def q5g():
    import polardecoding_amd as pa
    return [int(j) for j in pa.q_sequence(N)]


def from_5g(A):
    """the A most reliable leaves of the 5G order, ascending reliability"""
    return q5g()[N - A:]


def with_low(low, A=536):
    """the 5G set of size A with its leaves below 256 replaced by `low` (ascending reliability kept for the rest)"""
    return sorted(low) + [j for j in from_5g(A) if j >= 256]


def codes():
    """name -> (algo, taps, info leaves, E)"""
    import polardecoding_amd as pa
    CRC24C = tuple(pa.CRC24C_TAPS)
    return {
        "headline": ("CASCL", CRC24C, from_5g(536), 192),                       # 127, 190, 191, then 219
        "scl512": ("SCL", None, from_5g(512), 192),                             # 127, 191, then 221: logact = 2 at E
        "e256": ("CASCL", CRC24C, with_low([127, 254, 255]), 256),
        "one_path": ("SCL", None, with_low([254, 255]), 128),                   # one path up to leaf 254: (c) stops 192 and 256
        "pair_126_127": ("CASCL", CRC24C, with_low([126, 127, 190, 191]), 128),   # four information leaves below 192
        "leaf_189": ("CASCL", CRC24C, with_low([127, 189, 191]), 128),          # 189 in place of 190
        "third_at_189": ("SCL", None, with_low([126, 127, 189]), 128),
        "two_before_192": ("SCL", None, with_low([127, 191, 255]), 192),        # (c) stops 256
        "k768": ("SCL", None, from_5g(768), 0),                                 # first information leaf: 63
        "all_info": ("SCL", None, list(range(N)), 0),
        "k256": ("CASCL", CRC24C, from_5g(280), 128),                           # 255 alone below 256: one path, (c)
        "k256_scl": ("SCL", None, from_5g(256), 128),
    }
