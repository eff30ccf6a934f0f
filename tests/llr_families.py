"""Input families for the decoders' tie, zero and degenerate-row paths (a plain helper module, imported by
tests/test_llr_families_host.py and tests/test_gpu_llr_families.py).

A receiver hands a decoder fixed-point LLRs: magnitudes coincide all the time, sums cancel to exact zeros, and rate
matching plants constants.  The functions here make such rows from Gaussian LLR rows (the oracle's frames, or any seeded rows where the width is
not N), in float64 and float32:

  grid(llr, step, maxq)   clip(rint(llr / step), -maxq, maxq) * step; GRIDS lists the three (step, maxq) in use.  Every value
                          is a small multiple of a power of two, so the float32 copy is exact.
  hard(llr, c)            +-c with the channel sign: one magnitude everywhere.
  mix_zero_signs(x, seed) a copy with the sign bit set on a seeded half of the exact zeros (-0.0 and +0.0 mixed).
  degenerate_rows(...)    all +0, all -0, all +c, all -c, alternating +-c, one non-zero entry, magnitude 2^20 (the value rate
                          matching plants at a shortened position), magnitude 1e30 (finite after 4096 additions in f32) and
                          subnormal magnitudes (1e-40 as f32, 1e-310 as f64).  No infinities, no NaN.
  plant(x, rows, start)   a copy of batch x with every degenerate row in it a few times (three, in at most half of the
                          batch).  The first copies go to the wavefront boundaries of a kernel that decodes one codeword per
                          lane -- batch positions 0, 63, 64, 127, 128, ... and last -- starting with row `start`; from 322
                          frames on there are more such positions than rows, so every row sits on one.
"""
import numpy as np

GRIDS = ((1.0, 7), (0.5, 15), (2.0, 3))
SHORT_LLR = 1048576.0          # POLAR_RM_SHORT_LLR = 2^20
HUGE = 1e30
SUBNORMAL = {np.dtype(np.float32): 1e-40, np.dtype(np.float64): 1e-310}


def oracle_llr(oracle, code, B, seed, db):
    """the LLRs [B][N] (float64) of B frames of the oracle's transmit chain at `db`"""
    sig = oracle.sigma_from_db(db)
    _, ys = oracle.Sim(seed).frames(code, sig, B)
    return np.stack([oracle.llr_from_y(y, sig) for y in ys])


def grid(llr, step, maxq):
    return np.clip(np.rint(np.asarray(llr, dtype=np.float64) / step), -maxq, maxq) * step


def hard(llr, c=1.0):
    return np.where(np.signbit(llr), -c, c).astype(np.float64)


def mix_zero_signs(x, seed):
    x = np.array(x, copy=True)
    zero = np.flatnonzero(x.ravel() == 0)
    pick = zero[np.random.default_rng(seed).random(zero.size) < 0.5]
    flat = x.reshape(-1)
    flat[zero] = 0.0
    flat[pick] = -0.0
    return x


def degenerate_rows(width, dtype, seed, c=1.0):
    """[(name, row [width] of dtype)]: the degenerate rows of the module docstring; random signs where a row has any."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(width) < 0.5, -1.0, 1.0)
    alt = np.where(np.arange(width) % 2 == 0, c, -c)
    one = np.zeros(width)
    one[int(rng.integers(width))] = -c
    rows = [("zero+", np.zeros(width)), ("zero-", -np.zeros(width)), ("all+c", np.full(width, c)), ("all-c", np.full(width, -c)),
            ("alternating", alt), ("one_nonzero", one), ("2^20", sign * SHORT_LLR), ("1e30", sign * HUGE),
            ("subnormal", sign * SUBNORMAL[dtype])]
    out = [(name, r.astype(dtype)) for name, r in rows]
    for name, r in out:
        assert np.isfinite(r).all(), name
    assert (out[-1][1] != 0).all() and np.signbit(out[1][1]).all()
    return out


def edge_positions(B):
    """0, 63, 64, 127, 128, ... and B - 1: the first and last lane of every batch of 64"""
    e = [0]
    for k in range(64, B, 64):
        e += [k - 1, k]
    e.append(B - 1)
    return list(dict.fromkeys(p for p in e if 0 <= p < B))


def plant(x, rows, start=0, copies=3):
    """x [B][width] with the degenerate rows planted `copies` times each (in at most half of the batch), the wavefront
    boundaries first"""
    x = np.array(x, copy=True)
    B, k = len(x), len(rows)
    edges = edge_positions(B)
    taken = set(edges)
    slots = edges + [p for p in range(B) if p not in taken]
    for i in range(min(copies * k, B // 2)):
        x[slots[i]] = rows[(start + i) % k][1]
    return x


def families(llr, seed, dtype, degenerate=True):
    """{name: batch of dtype} from Gaussian rows llr [B][width]: the three grids, hard, each again with mixed zero signs and
    (degenerate=True) the degenerate rows planted."""
    dtype = np.dtype(dtype)
    width = llr.shape[1]
    out = {}
    base = [(f"grid{step:g}x{maxq}", grid(llr, step, maxq)) for step, maxq in GRIDS] + [("hard", hard(llr, 1.0))]
    for k, (name, x) in enumerate(base):
        out[name] = x.astype(dtype)
        y = mix_zero_signs(x, seed + k).astype(dtype)
        if degenerate:
            y = plant(y, degenerate_rows(width, dtype, seed + 10 * k, c=1.0 if name == "hard" else 2.0), start=2 * k)
        out[name + "_mixed"] = y
    return out
