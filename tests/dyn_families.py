"""Constraint sets for dynamic frozen bits, and the cases built from them (a plain helper module, imported by
tests/test_dyn_families_host.py, tests/test_gpu_dyn_families.py and tools/stress_parity.py --dyn).

k_scl_dyn (csrc/scl_dyn.h) keeps a per-path history -- word 0 in a register that is shuffled on every fork and refill, words
1.. in LDS, copied on every fork and refill -- and reduces AND / popcount / XOR over the S = 64 / L lanes of a path, lane
`pos` taking the words pos, pos + S, ... up to j >> 5.  PAC rows, three 5G parity-check bits and sparse random sets reach
little of that.  constraint_families(N, frozen_mask, seed) makes the other shapes, name -> (pos, sets); every frozen position
of the mask is dynamic unless stated:

  all_prev        S_j = {0 .. j-1}: every mask word up to j >> 5 is full (N = 1024, L = 32: sixteen strided words per lane)
  bern_half       each i < j with probability 1/2
  prev_only       S_j = {j-1} (empty for j = 0): at j % 32 == 0 the one bit read is the last one written to the word before
  word0_only      each i < min(j, 32) with probability 1/2: the register word alone, whatever word j is in
  own_word_only   S_j = {i : 32 (j >> 5) <= i < j}: the last word the loop reads, alone
  word_edges      S_j = {i < j : i % 32 in (0, 31)}: the first and the last bit of every word
  dyn_chain       S_j = the nearest earlier information position and the two nearest earlier dynamic positions
  alternate       every second frozen position dynamic with bern_half sets, the others plain frozen
  pac             polar_dyn_pac with g = 0o133 on the mask's information set
  none            (a Case's family only, not in FAMILIES) no constraints: dyn = None, a plain context (tests/wide_families.py)

Every set obeys the ABI: i < j, ascending, position frozen under the cfg; a set may hold information, dynamic and plain
frozen positions.  Everything is a function of (N, mask, seed) alone.

cases() lists what the device file runs and the host file holds the conditions for: a Case names (N, mask, constraint
family, L, dtype, algorithm, frames, input batches); materialise(case) makes its code and rows, reference(case) the model's
outputs on them (computed once per process, never modified).  Input batches are those of tests/llr_families.py (three grids,
`hard`, each again `_mixed`: zero signs mixed and the degenerate rows planted) and two mixtures of them:
  cycle    frame i is on GRIDS[k] for k = (i // 2) % 4 < 3, `hard` for k = 3 -- every kind at both Eb/N0 of a two-point batch
  split    the first half (rounded up) on the (0.5, 15) grid, the rest `hard`
The grids and `hard` are exact in float32, and an f32 case's rows are made in float32, so the f32 model reads what the f32
kernel reads."""
import os
import sys
import zlib
from collections import OrderedDict, namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frozen_patterns as P  # noqa: E402
import llr_families as F  # noqa: E402
import test_dyn_host as M  # noqa: E402

G133 = 0o133
CRC6 = (0, 5, 6)
NONE = "none"
FAMILIES = ("all_prev", "bern_half", "prev_only", "word0_only", "own_word_only", "word_edges", "dyn_chain", "alternate", "pac")


def _rng(N, seed, name):
    return np.random.default_rng([int(seed), N, zlib.crc32(name.encode())])


def _i32(x):
    return np.asarray(x, dtype=np.int32).reshape(-1)


def constraint_families(N, frozen_mask, seed):
    """OrderedDict name -> (pos int32 [D] ascending, sets: D ascending int32 arrays); see the module docstring"""
    mask = np.asarray(frozen_mask)
    assert mask.shape == (N,)
    fz = np.flatnonzero(mask != 0)
    info = np.flatnonzero(mask == 0)

    def bern(name, j, lim=None):
        r = _rng(N, seed, f"{name}{j}")
        return np.flatnonzero(r.random(j if lim is None else min(j, lim)) < 0.5)

    def chain(j):
        d = fz[fz < j][-2:]
        i = info[info < j][-1:]
        return np.sort(np.concatenate([d, i]))

    fam = OrderedDict()
    fam["all_prev"] = (fz, [np.arange(j) for j in fz])
    fam["bern_half"] = (fz, [bern("bern_half", j) for j in fz])
    fam["prev_only"] = (fz, [np.arange(j - 1, j) if j else np.zeros(0) for j in fz])
    fam["word0_only"] = (fz, [bern("word0_only", j, 32) for j in fz])
    fam["own_word_only"] = (fz, [np.arange(32 * (j >> 5), j) for j in fz])
    fam["word_edges"] = (fz, [np.flatnonzero(np.isin(np.arange(j) % 32, (0, 31))) for j in fz])
    fam["dyn_chain"] = (fz, [chain(j) for j in fz])
    fam["alternate"] = (fz[::2], [bern("alternate", j) for j in fz[::2]])
    if fz.size and info.size:
        import polardecoding_amd as pa
        fam["pac"] = pa.dyn_pac(N, info.astype(np.int32), G133)
    out = OrderedDict()
    for name, (pos, sets) in fam.items():
        pos, sets = _i32(pos), [_i32(s) for s in sets]
        assert len(sets) == pos.size and (np.diff(pos) > 0).all() and mask[pos].all(), name
        for j, s in zip(pos, sets):
            assert (np.diff(s) > 0).all() and (s.size == 0 or (s[0] >= 0 and s[-1] < j)), (name, j)
        out[name] = (pos, sets)
    return out


# ---- input batches ----------------------------------------------------------------------------------------------------
def input_batch(llr, name, seed, dtype):
    """the batch `name` (module docstring) of Gaussian rows llr [B][N], as dtype"""
    B = len(llr)
    if name == "cycle":
        kinds = [F.grid(llr, s, q) for s, q in F.GRIDS] + [F.hard(llr, 1.0)]
        k = (np.arange(B) // 2) % 4
        x = np.stack([kinds[k[i]][i] for i in range(B)])
    elif name == "split":
        h = (B + 1) // 2
        x = np.concatenate([F.grid(llr[:h], 0.5, 15), F.hard(llr[h:], 1.0)])
    else:
        x = F.families(llr, seed, dtype)[name]
    x = x.astype(dtype)
    assert np.isfinite(x).all()
    return x


LLR_FAMILIES = ("grid1x7", "grid1x7_mixed", "grid0.5x15", "grid0.5x15_mixed", "grid2x3", "grid2x3_mixed", "hard", "hard_mixed")

# ---- the cases ----------------------------------------------------------------------------------------------------------
# group: the device test that runs it; mask: "rm" (the PAC rate profile, K = N / 2) or a family of frozen_patterns;
# algo: "SC" (L = 1), "SCL", "CASCL" (CRC-6, the CRC positions anywhere in the set)
Case = namedtuple("Case", "group N mask fam L dtype algo B dbs inputs")


def tag(c):
    return f"{c.N}-{c.mask}-{c.fam}-L{c.L}-{c.dtype}-{c.algo}-B{c.B}"


def _seed(c):
    return 1 + zlib.crc32(tag(c).encode()) % 1000003


N32_CONFIGS = [(1, "f64", 65), (2, "f32", 300), (32, "f64", 300)]            # (L, dtype, B)
N64_CONFIGS = [(2, "f64"), (2, "f32"), (8, "f64"), (8, "f32")]
N64_INPUTS = ("grid2x3", "grid0.5x15_mixed", "hard")
N128_SCL = [(1, "f64"), (8, "f32"), (32, "f64"), (1, "f32"), (8, "f64"), (32, "f32")]
N128_CASCL = [(8, "f64"), (32, "f32"), (8, "f32"), (32, "f64")]
N128_FAMS = ("bern_half", "alternate", "dyn_chain")
N1024_CONFIGS = [(32, "f64"), (32, "f32"), (8, "f64"), (1, "f64")]
N1024_FAMS = ("all_prev", "word0_only", "own_word_only", "word_edges")
N1024_MASKS = ("rm", "islands_16_a", "leaf0")
DBS2 = (1.0, 3.0)
DBS4 = (0.0, 1.0, 1.5, 2.0)


def cases():
    """every case of tests/test_gpu_dyn_families.py, in running order"""
    out = []
    # N = 32: the history is the register alone.  Every constraint family on every input family, one-per-wave batch sizes.
    for L, dt, B in N32_CONFIGS:
        out += [Case("n32", 32, "rm", f, L, dt, "SC" if L == 1 else "SCL", B, DBS4, LLR_FAMILIES) for f in FAMILIES]
    # N = 64: the first LDS history word; default and global-scratch variant on the same cases
    for L, dt in N64_CONFIGS:
        out += [Case("n64", 64, "rm", f, L, dt, "SCL", 65, DBS4, N64_INPUTS) for f in FAMILIES]
    # N = 128: every frozen pattern x three constraint families; mask m with family f runs SCL configuration (m + 2 f) % 6 (so a mask
    # meets L = 1, 8 and 32 and a constraint family all six configurations), and every mask that can carry CRC-6 one CA-SCL configuration
    masks = list(P.families(128))
    for m, name in enumerate(masks):
        for f, famname in enumerate(N128_FAMS):
            L, dt = N128_SCL[(m + 2 * f) % 6]
            out.append(Case("n128", 128, name, famname, L, dt, "SC" if L == 1 else "SCL", 16, DBS2, ("cycle",)))
    for m, name in enumerate(P.with_crc(P.families(128), 128)):
        L, dt = N128_CASCL[m % 4]
        out.append(Case("n128crc", 128, name, N128_FAMS[m % 3], L, dt, "CASCL", 16, DBS2, ("cycle",)))
    # N = 1024: dense rows.  The rm mask meets every configuration; the islands and leaf0 masks one each per family, and
    # word0_only every configuration on the islands mask too: the first 32 leaves of the rm mask are all frozen, so there
    # the register word of the history stays 0.
    for m, name in enumerate(N1024_MASKS):
        for f, famname in enumerate(N1024_FAMS):
            for c, (L, dt) in enumerate(N1024_CONFIGS):
                if name == "rm" or c == (f + m) % 4 or (name, famname) == ("islands_16_a", "word0_only"):
                    out.append(Case("n1024", 1024, name, famname, L, dt, "SC" if L == 1 else "SCL", 65, DBS2, ("split",)))
    assert len({tag(c) for c in out}) == len(out)
    return out


def np_dtype(c):
    return np.float32 if c.dtype == "f32" else np.float64


def mask_of(N, name):
    """(frozen mask uint8 [N], info_order) of a case's mask"""
    if name == "rm":
        import polardecoding_amd as pa
        order = pa.pac_info_order(N, N // 2, "rm")
        mask = np.ones(N, dtype=np.uint8)
        mask[order] = 0
        return mask, order
    mask = P.families(N)[name]
    return mask, P.order_of(mask, 77)


Made = namedtuple("Made", "mask order dyn taps u batches")
_MADE, _REFS = {}, {}


def materialise(c):
    """Made(mask, info_order, (pos, sets), CRC taps or None, u [B][N], OrderedDict input name -> rows [B][N] of the dtype)"""
    if c not in _MADE:
        mask, order = mask_of(c.N, c.mask)
        dyn = None if c.fam == NONE else constraint_families(c.N, mask, 5)[c.fam]
        taps = CRC6 if c.algo == "CASCL" else None
        u, llr = M.make_frames(c.N, order, dyn, c.B, _seed(c), dbs=c.dbs, crc=taps)
        batches = OrderedDict((k, input_batch(llr, k, _seed(c), np_dtype(c))) for k in c.inputs)
        for a in (mask, order, u) + tuple(batches.values()):
            a.setflags(write=False)
        _MADE[c] = Made(mask, order, dyn, taps, u, batches)
    return _MADE[c]


def model(c, made, rows, oracle=None):
    """dscl_model on rows [B][N] of case c: (u_hat, pm float64, flags)"""
    return M.dscl_model(made.mask, made.dyn, np.asarray(rows, dtype=np.float64), c.L, crc=(made.order, made.taps) if made.taps else None,
                        dtype=np_dtype(c), sc=(c.algo == "SC"), oracle=oracle)


def reference(c):
    """OrderedDict input name -> the model's (u_hat, pm, flags) on that batch; one model run over all batches of the case"""
    if c not in _REFS:
        made = materialise(c)
        res = model(c, made, np.concatenate(list(made.batches.values())))
        out = OrderedDict()
        for k, name in enumerate(made.batches):
            part = tuple(np.ascontiguousarray(r[k * c.B:(k + 1) * c.B]) for r in res)
            for a in part:
                a.setflags(write=False)
            out[name] = part
        _REFS[c] = out
    return _REFS[c]
