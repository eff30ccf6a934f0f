"""The cases that hold k_scl_wide (csrc/scl_wide.h, L = 64 / 128 / 256) to dscl_model where a list spans wavefronts (a plain
helper module, imported by tests/test_wide_families_host.py, tests/test_gpu_wide_families.py and tools/stress_parity.py
--wide).

At L >= 128 the ranking, the refill of dead slots, the exchange of path state and the final choice cross wavefronts through
LDS.  That code runs only when a path dies or candidates tie, and on Gaussian rows the model flags no tie at all; so the cases
here put the tie inputs of tests/llr_families.py, the frozen sets of tests/frozen_patterns.py and the constraint families of
tests/dyn_families.py on shapes with 2 and 4 wavefronts.  A case is a dyn_families.Case (family "none": no constraints, a
plain context); its group names the device test that runs it:

  w1   N = 32, L = 128 / 256: history and partial sums all in registers, yet 2 / 4 wavefronts; the eight LLR families
  w2   N = 64, L = 128 on every frozen pattern (the first LDS words, two wavefronts), L = 256 on three of them
  w3   N = 128, L = 256 on every frozen pattern, f32 (levels in LDS) and f64 (global scratch by size) in turn
  w4   CA-SCL at N = 128 with CRC-6 at permuted positions, L = 128 f32 on every mask that can carry it, L = 256 f64 on three
  w5   the constraint families at (64, 128) and (128, 256), one CA-SCL case with constraints at (128, 256)
  w6   the three shapes that fill the 64-bit pointer table, on a grid with mixed zero signs (mask "5g": the 5G order)
  w7   masks with K <= 5 at L = 128 / 256 and at L = 32: the list never fills; one set of rows per (N, mask) for all three L
  w10  N = 32, L = 256: the 64 model-checked rows of the work-queue test

Input batches beyond those of dyn_families.input_batch:
  mixed             rows in turn from grid(1, 7), grid(0.5, 15), grid(2, 3) and hard(2.0), zero signs mixed, the degenerate
                    rows of llr_families planted once each (in at most half of the batch), starting with row `seed`: what
                    tests/test_gpu_llr_families.py calls a mixed batch, with one copy per row for the small batches here
  grid0.5x15_signs  the (0.5, 15) grid with -0.0 and +0.0 mixed, nothing planted
  awgn              the Gaussian rows themselves (rounded to float32 for an f32 case)
reference(case) runs the model once per process with a trace (dscl_model's `trace`) and keeps both; nothing is modified
afterwards.  SEED shifts every case's frames (tools/stress_parity.py --wide sets it; the tests leave it 0)."""
import os
import sys
import zlib
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dyn_families as D  # noqa: E402
import frozen_patterns as P  # noqa: E402
import llr_families as F  # noqa: E402
import test_dyn_host as M  # noqa: E402

Case, tag, np_dtype, NONE, CRC6 = D.Case, D.tag, D.np_dtype, D.NONE, D.CRC6
SEED = 0
DBS2 = (1.0, 3.0)
DBS_CRC = (0.0, 3.0)

W1_CONFIGS = [(128, "f64"), (128, "f32"), (256, "f64"), (256, "f32")]
W1_MASKS = ("dense_all", "leaf0", "bern_0.5", "sparse_5_half")
W1_CONSTRAINTS = ("all_prev", "prev_only")              # on bern_0.5
W1_B = 12                                               # frames per batch: every degenerate row in two of the four mixed batches
W2_L256_MASKS = ("dense_all", "leaf0_run", "tail_32")
W3_CONFIGS = [(256, "f32"), (256, "f64")]               # levels in LDS; global scratch by size
W4_L256_MASKS = ("bern_0.5", "leaf0", "islands_32_a")
W5_CONFIGS = [(64, 128, "f64", 16), (64, 128, "f32", 16), (128, 256, "f32", 8), (128, 256, "f64", 8)]   # (N, L, dtype, B)
W5_MASKS = ("rm", "leaf0", "islands_16_a", "bern_0.5")
W5_FAMS = ("all_prev", "bern_half", "word_edges", "own_word_only", "dyn_chain", "pac")
W6_SHAPES = [(1024, 64, "f64"), (512, 128, "f32"), (256, 256, "f64")]
W7_MASKS = {64: ("sparse_last", "sparse_first", "sparse_5_half", "sparse_1_2_penult", "lead_7"),
            128: ("sparse_last", "sparse_first", "sparse_5_half", "sparse_1_2_penult", "lead_15")}
# cases whose first seed gave no frame in error (tests/test_wide_families_host.py asks for one): tag -> seed shift
RESEED = {"128-rm-all_prev-L256-f32-SCL-B8": 2, "128-rm-pac-L256-f32-SCL-B8": 2}
GROUPS = ("w1", "w2", "w3", "w4", "w5", "w6", "w7", "w10")


def cases():
    """every Case of tests/test_gpu_wide_families.py, in running order"""
    out = []
    for L, dt in W1_CONFIGS:
        out += [Case("w1", 32, m, NONE, L, dt, "SCL", W1_B, D.DBS4, D.LLR_FAMILIES) for m in W1_MASKS]
        out += [Case("w1", 32, "bern_0.5", f, L, dt, "SCL", W1_B, D.DBS4, D.LLR_FAMILIES) for f in W1_CONSTRAINTS]
    for dt in ("f64", "f32"):
        out += [Case("w2", 64, m, NONE, 128, dt, "SCL", 24, DBS2, ("mixed",)) for m in P.families(64)]
    for dt in ("f32", "f64"):
        out += [Case("w2", 64, m, NONE, 256, dt, "SCL", 12, DBS2, ("mixed",)) for m in W2_L256_MASKS]
    for k, m in enumerate(P.families(128)):
        L, dt = W3_CONFIGS[k % 2]
        out.append(Case("w3", 128, m, NONE, L, dt, "SCL", 12, DBS2, ("mixed",)))
    crc_masks = list(P.with_crc(P.families(128), 128))
    out += [Case("w4", 128, m, NONE, 128, "f32", "CASCL", 16, DBS_CRC, ("cycle",)) for m in crc_masks]
    out += [Case("w4", 128, m, NONE, 256, "f64", "CASCL", 16, DBS_CRC, ("cycle",)) for m in W4_L256_MASKS]
    for N, L, dt, B in W5_CONFIGS:
        out += [Case("w5", N, m, f, L, dt, "SCL", B, DBS2, ("cycle",)) for m in W5_MASKS for f in W5_FAMS]
    out.append(Case("w5", 128, "bern_0.5", "bern_half", 256, "f32", "CASCL", 8, DBS2, ("cycle",)))
    out += [Case("w6", N, "5g", NONE, L, dt, "SCL", 4, (1.0, 1.5), ("grid0.5x15_signs",)) for N, L, dt in W6_SHAPES]
    for N, masks in W7_MASKS.items():
        out += [Case("w7", N, m, NONE, L, "f64", "SCL", 32, DBS2, ("awgn", "mixed")) for m in masks for L in (128, 256, 32)]
    out.append(Case("w10", 32, "leaf0", NONE, 256, "f64", "SCL", 64, D.DBS4, ("mixed",)))
    assert len({tag(c) for c in out}) == len(out)
    return out


def mask_of(N, name):
    """dyn_families.mask_of, and "5g": the N / 2 most reliable positions of the 5G order"""
    if name == "5g":
        import polardecoding_amd as pa
        order = np.asarray(pa.q_sequence(N)[N // 2:], dtype=np.int32)
        mask = np.ones(N, dtype=np.uint8)
        mask[order] = 0
        return mask, order
    return D.mask_of(N, name)


def _seed(c):
    """one set of frames per case; in w7 per (N, mask), so that the three list sizes decode the same rows"""
    key = tag(c._replace(L=0)) if c.group == "w7" else tag(c)
    return 1 + (zlib.crc32(key.encode()) + 7919 * SEED + RESEED.get(tag(c), 0)) % 1000003


def mixed(llr, seed, dtype, copies=1):
    """the mixed batch of the module docstring from Gaussian rows llr [B][width]"""
    dt = np.dtype(dtype)
    parts = [F.grid(llr, s, m) for s, m in F.GRIDS] + [F.hard(llr, 2.0)]
    x = np.empty_like(llr)
    for k, p in enumerate(parts):
        x[k::4] = p[k::4]
    x = F.mix_zero_signs(x, seed).astype(dt)
    return F.plant(x, F.degenerate_rows(llr.shape[1], dt, seed, c=2.0), start=seed, copies=copies)


def input_batch(llr, name, seed, dtype):
    if name == "mixed":
        x = mixed(llr, seed, dtype)
    elif name == "grid0.5x15_signs":
        x = F.mix_zero_signs(F.grid(llr, 0.5, 15), seed).astype(dtype)
    elif name == "awgn":
        x = llr.astype(dtype)
    else:
        return D.input_batch(llr, name, seed, dtype)
    assert np.isfinite(x).all()
    return x


_MADE, _REFS = {}, {}


def materialise(c):
    """dyn_families.Made of a case; as dyn_families.materialise, with the masks and input batches of this module"""
    if c not in _MADE:
        mask, order = mask_of(c.N, c.mask)
        dyn = None if c.fam == NONE else D.constraint_families(c.N, mask, 5)[c.fam]
        taps = CRC6 if c.algo == "CASCL" else None
        u, llr = M.make_frames(c.N, order, dyn, c.B, _seed(c), dbs=c.dbs, crc=taps)
        batches = OrderedDict((k, input_batch(llr, k, _seed(c), np_dtype(c))) for k in c.inputs)
        for a in (mask, order, u) + tuple(batches.values()):
            a.setflags(write=False)
        _MADE[c] = D.Made(mask, order, dyn, taps, u, batches)
    return _MADE[c]


def model_on(mask, dyn, rows, L, dtype, crc=None, trace=None):
    """dscl_model on rows [B][N] in the arithmetic `dtype` ("f64" / "f32")"""
    return M.dscl_model(mask, dyn, np.asarray(rows, dtype=np.float64), L, crc=crc, dtype=np.float32 if dtype == "f32" else np.float64,
                        trace=trace)


def reference(c):
    """(OrderedDict input name -> the model's (u_hat, pm, flags), OrderedDict input name -> trace dict of bool [B]); one model
    run over all batches of the case"""
    if c not in _REFS:
        made = materialise(c)
        trace = {}
        res = model_on(made.mask, made.dyn, np.concatenate(list(made.batches.values())), c.L, c.dtype,
                       crc=(made.order, made.taps) if made.taps else None, trace=trace)
        out, tr = OrderedDict(), OrderedDict()
        for k, name in enumerate(made.batches):
            sl = slice(k * c.B, (k + 1) * c.B)
            out[name] = tuple(np.ascontiguousarray(r[sl]) for r in res)
            tr[name] = {key: np.ascontiguousarray(v[sl]) for key, v in trace.items()}
            for a in out[name] + tuple(tr[name].values()):
                a.setflags(write=False)
        _REFS[c] = (out, tr)
    return _REFS[c]
