"""The cases that run the chunked host loops of csrc/polar_hip.hip and csrc/h_*.hip across a pass boundary (a plain helper module, imported by
tests/test_chunks_host.py and tests/test_gpu_chunks.py).

Seven loops cut a batch into passes of at most 256 MiB of rows (chunk_rows) and offset every input, output and list pointer
by hand for the second and later passes: q8_decode_rows, the rate-matched loop (for_rm_chunks, which decode_device_impl and
polar_list_decode share; each offsets its own outputs in the loop's body), the later stages of cascl_adaptive, pass B of
scf_decode, the levels of its dynamic rule, the attempts of bpl_decode (attempt 0 through the staging buffers when the first
graph is not the identity, and every later attempt) and polar_construct_batch.  At 256 MiB a
second pass takes batches no model can follow; polardecoding_amd.testing.chunk_bytes() lowers the cap of one context, and
the cases here are the rows, contexts and caps at which a few hundred frames of N = 32 .. 128 make three and more passes.

A Case names its loop, its kind and its cap in bytes; passes(case, oracle) lists, from the models alone, the frames that
enter every pass loop of the decode (per level, stage or attempt) beside the rows per pass CH that follow from the cap:
  ragged  every pass loop of the case takes more than 2 CH frames and not a multiple of CH: three passes or more and a
          partial last one (with CH = 1 there is no partial pass; such a case only has to make more than two)
  even    the first pass loop of the case takes exactly 2 CH frames: no partial pass
  small   a further batch size of a ragged case (B = 65: one full pass and one frame)
tests/test_chunks_host.py asserts these and what else a case is there for; tests/test_gpu_chunks.py decodes.  The row
loops (floor 64 rows) run with a cap of 1 byte, so CH = 64, on B = 229 = 64 + 64 + 64 + 37, B = 128 and B = 65; the SC-Flip
loops have floor 1 and get caps that make CH = 1 .. 12.  A rate-matched SC-Flip or BPL context has a pass loop inside every
pass of the rate-matched loop; those run with RM_CAP, which is below one row (CH = 64) and a few SC-Flip frames.

Every reference comes from what the suite already has and is computed once per process: q8_model, dscf_model with the
frames of tests/test_gpu_dscf.py, scf_model, bpl_model, the oracle composition of the adaptive rule, test_rm_host.recover
and the genie model.  Float rows are rounded to float32 first, so that a double and a float input share one reference."""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bpl_model as BM  # noqa: E402
import q8_model as QM  # noqa: E402
import test_gpu_cascl_adaptive as AD  # noqa: E402  (_frames, _oracle_composition: the oracle composition of the rule)
import test_gpu_dscf as DS  # noqa: E402  (_shape, _rows: the frames of the dynamic rule's tests)
import test_gpu_q8 as Q8T  # noqa: E402  (_rows, _family_rows)
import test_rm_host as RM  # noqa: E402
from dscf_model import dscf_model  # noqa: E402
from test_cascl_adaptive_host import CRC6, FLAG_CRC_PASS, syndrome  # noqa: E402
from test_scf_host import scf_model  # noqa: E402

ROW_FLOOR, SCF_FLOOR = 64, 1          # chunk_rows' floor argument: the row loops, the two SC-Flip loops
ROW_CAP = 1                           # bytes: every row loop runs on its floor
RM_CAP = 400                          # bytes: below a row of N = 128 (512 / 1024 bytes), 3 frames of SC-Flip T = 8, 6 of (4, 4)
B_RAGGED, B_EVEN, B_SMALL = 229, 128, 65
ROW_BATCHES = {"ragged": B_RAGGED, "even": B_EVEN, "small": B_SMALL}
TAU = DS.TAU

Case = namedtuple("Case", "name loop kind cap spec")
_memo = {}


def rows_per_pass(cap, unit_bytes, floor):
    """chunk_rows() before its min(B, .): the rows per pass a cap gives"""
    return max(floor, cap // unit_bytes)


def pair_bytes(N):
    return (N // 32) * 4


def once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def f32_exact(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def info_order(N, A):
    """the A most reliable positions of the 5G order restricted to < N: what polar_create derives"""
    return np.asarray(RM.q_order(N)[N - A:], dtype=np.int32)


# ---- q8_decode_rows ---------------------------------------------------------------------------------------------------------
Q8_N = 64
Q8_CTX = {"cascl8": dict(K=26, L=8, taps=CRC6, sc=False), "scl4": dict(K=32, L=4, taps=None, sc=False),
          "sc": dict(K=32, L=1, taps=None, sc=True)}
Q8_SIGMA = 0.84


def q8_rows(family):
    """[229][64] float64 rows, exact in float32: test_gpu_q8's spread rows, or its ternary rows over the scale (ties in
    every frame, so equal metrics sit on both sides of every pass boundary)"""
    def make():
        rng = np.random.default_rng([Q8_N, len(family)])
        if family == "ternary":
            return Q8T._family_rows("ternary", B_RAGGED, Q8_N, rng).astype(np.float64) * 0.5
        return f32_exact(Q8T._rows(rng, B_RAGGED, Q8_N))
    return once(("q8 rows", family), make)


def q8_want(ctx, family, y=False):
    """(u_hat, pm, flags) of q8_model for the rows of a family; y: the rows given as y = llr sigma^2 / 2 with Q8_SIGMA"""
    def make():
        s = Q8_CTX[ctx]
        x = q8_rows(family)
        q = QM.quantize(q8_y(family), sigma=Q8_SIGMA) if y else QM.quantize(x)
        A = s["K"] + (max(s["taps"]) if s["taps"] else 0)
        io = info_order(Q8_N, A)
        fz = np.ones(Q8_N, dtype=np.uint8)
        fz[io] = 0
        return QM.decode_rows(q, fz, s["L"], crc=(io, s["taps"]) if s["taps"] else None, sc=s["sc"])
    return once(("q8 want", ctx, family, y), make)


def q8_y(family):
    return q8_rows(family) * Q8_SIGMA * Q8_SIGMA / 2


# ---- the rate-matched loop --------------------------------------------------------------------------------------------------
RM_N, RM_K = 128, 40
RM_E = [(111, True, RM.PUNCTURE), (80, False, RM.SHORTEN), (389, False, RM.REPEAT)]   # E, ibil, the mode for A = 40 and 46


def rm_rows(E):
    """[229][E] LLR rows, exact in float32: the all-zero codeword at 0 .. 3 dB, every fourth row pure noise (frames that fail
    a CRC, flip lists, BP attempts that do not converge: the pass loops inside a pass run)"""
    def make():
        rng = np.random.default_rng(1000 + E)
        sig = 10.0 ** (-rng.uniform(0.0, 3.0, size=(B_RAGGED, 1)) / 20.0)
        x = 2.0 * (1.0 + sig * rng.standard_normal((B_RAGGED, E))) / sig / sig
        x[3::4] = rng.normal(0.0, 2.0, size=x[3::4].shape)
        return f32_exact(x)
    return once(("rm rows", E), make)


# ---- cascl_adaptive ---------------------------------------------------------------------------------------------------------
AD_N, AD_K, AD_STAGES = 128, 64, (1, 2, 8)


def ad_code(oracle):
    return once("ad code", lambda: oracle.Code(AD_N, AD_K, CRC6))


def _ad_all(oracle):
    def make():
        rng = np.random.default_rng(11)
        noise = rng.normal(0.0, 2.0, size=(120, AD_N))
        fr, _, _, _ = AD._frames(oracle, ad_code(oracle), 280, 900, dbs=(2.0,))
        x = np.concatenate([noise, fr])
        np.random.default_rng(5).shuffle(x)
        return f32_exact(x)
    return once("ad all", make)


def ad_stage_fails(oracle, rows, dtype):
    """per later stage the frames that enter it: bool [B] failing every stage before"""
    code = ad_code(oracle)
    io = code.info_order
    out, todo = [], np.ones(len(rows), dtype=bool)
    for L in AD_STAGES[:-1]:
        if L == 1:
            q = [j for j in range(code.N) if j not in set(io.tolist())] + io.tolist()
            uh, _, _ = oracle.decode(oracle.Code(code.N, code.A, None, Q=q), rows, "SC", dtype=dtype)
        else:
            uh, _, _ = oracle.decode(code, rows, "CASCL", L=L, dtype=dtype)
        todo = todo & (syndrome(uh, io, CRC6) != 0)
        out.append(todo)
    return out


def ad_rows(oracle, kind, dtype="f64"):
    """ragged: 120 pure-noise rows and 280 frames at 2 dB, shuffled; even: of those, the first 128 that fail stage 0 in
    `dtype` and 37 that pass it"""
    x = _ad_all(oracle)
    if kind == "ragged":
        return x

    def make():
        f0 = ad_stage_fails(oracle, x, dtype)[0]
        return x[np.sort(np.concatenate([np.flatnonzero(f0)[:2 * ROW_FLOOR], np.flatnonzero(~f0)[:37]]))]
    return once(("ad even", dtype), make)


def ad_want(oracle, kind, dtype="f64"):
    return once(("ad want", kind, dtype),
                lambda: AD._oracle_composition(oracle, ad_code(oracle), CRC6, AD_STAGES, ad_rows(oracle, kind, dtype), dtype=dtype))


# ---- scf_decode, static pass B ----------------------------------------------------------------------------------------------
SCF_N, SCF_K = 128, 64


def _scf_all(oracle):
    code, llr, _ = DS._shape(oracle, SCF_N)
    return code, llr[:600]


def scf_rows(oracle, case):
    code, llr = _scf_all(oracle)
    T, dtype, kind = case.spec
    if kind == "ragged":
        return llr

    def make():
        fail = np.zeros(len(llr), dtype=bool)
        fail[scf_model(code, llr, T, dtype=dtype, oracle=oracle)[4]] = True
        n = 2 * rows_per_pass(case.cap, pair_bytes(SCF_N) * T, SCF_FLOOR)
        return llr[np.sort(np.concatenate([np.flatnonzero(fail)[:n], np.flatnonzero(~fail)[:21]]))]
    return once(("scf even", case.name), make)


def scf_want(oracle, case):
    """(u_hat, flags, attempts, sets [B][3], failing frames): scf_model, and the set a static context reports (the flipped
    position of the attempt that passed, else none)"""
    def make():
        code, _ = _scf_all(oracle)
        T, dtype, _ = case.spec
        u, flags, attempts, flips, fail = scf_model(code, scf_rows(oracle, case), T, dtype=dtype, oracle=oracle)
        sets = np.full((len(u), 3), -1, dtype=np.int64)
        for k, f in enumerate(fail):
            if flags[f] & FLAG_CRC_PASS:
                sets[f, 0] = flips[k][attempts[f] - 1]
        return u, flags, attempts, sets, fail
    return once(("scf want", case.name), make)


# ---- scf_decode, the levels of the dynamic rule -----------------------------------------------------------------------------
def dscf_code(oracle, N):
    return DS._shape(oracle, N)[0]


def dscf_rows(oracle, case):
    N, budgets, c, dtype, rows = case.spec
    code, llr, fail = DS._shape(oracle, N)
    if rows == "shape":
        return llr
    if rows == "quantised":   # the rows of test_quantised_rows_tie_at_a_list_boundary
        return np.clip(np.round(llr[:700] * 4) / 4, -8.0, 8.0)

    def make():
        if rows == "even":   # exactly 2 CH frames fail attempt 0
            n = 2 * rows_per_pass(case.cap, pair_bytes(N) * budgets[0], SCF_FLOOR)
            return llr[np.sort(np.concatenate([np.flatnonzero(fail)[:n], np.flatnonzero(~fail)[:30]]))]
        # "picked" (N = 1024): the frames of the shape that level 2 decides, the first failing ones up to 100, 40 that pass
        full = dscf_model(code, llr, budgets, c, TAU, dtype=dtype, oracle=oracle)
        two = np.flatnonzero((full.attempts > budgets[0]) & ((full.flags & FLAG_CRC_PASS) != 0))
        rest = np.setdiff1d(np.flatnonzero(fail), two)[:100 - len(two)]
        return llr[np.sort(np.concatenate([two, rest, np.flatnonzero(~fail)[:40]]))]
    return once(("dscf rows", case.name), make)


def dscf_want(oracle, case):
    N, budgets, c, dtype, _ = case.spec
    return once(("dscf want", case.name),
                lambda: dscf_model(dscf_code(oracle, N), dscf_rows(oracle, case), budgets, c, TAU, dtype=dtype, oracle=oracle))


def dscf_ch(case):
    N, budgets = case.spec[:2]
    return [rows_per_pass(case.cap, pair_bytes(N) * T, SCF_FLOOR) for T in budgets]


# ---- bpl_decode -------------------------------------------------------------------------------------------------------------
def bpl_graphs(n, which):
    if which == "default":
        return BM.cyclic_graphs(n, min(n, 8))
    return [list(range(n))[::-1]] + BM.cyclic_graphs(n, 3)   # the reversal first: attempt 0 goes through the staging buffers


def _awgn(rng, B, N, db):
    sig = 10.0 ** (-db / 20.0)
    return 2.0 * (1.0 + sig * rng.standard_normal((B, N))) / sig / sig


def bpl_code(oracle, case):
    N, K, _, _, taps = case.spec[:5]
    return once(("bpl code", N, K, taps), lambda: oracle.Code(N, K, taps))


def _bpl_all(oracle, case):
    """293 = 229 + 64 rows, exact in float32: two thirds at the lower Eb/N0 of the shape and one third at the higher, shuffled"""
    N, K, iters, which, taps, dbs = case.spec[:6]

    def make():
        rng = np.random.default_rng(5)
        B = B_RAGGED + ROW_FLOOR
        x = np.concatenate([_awgn(rng, B - B // 3, N, dbs[0]), _awgn(rng, B // 3, N, dbs[1])])
        rng.shuffle(x)
        return f32_exact(x)
    return once(("bpl all", N, dbs), make)


def _bpl_model(oracle, case, x):
    N, K, iters, which, taps = case.spec[:5]
    code = bpl_code(oracle, case)
    return BM.bpl_decode(x, code.frozen, code.info_order, bpl_graphs(code.n, which), iters, taps)


def bpl_rows(oracle, case):
    x = _bpl_all(oracle, case)
    sel = case.spec[6]
    if isinstance(sel, int):
        return x[:sel]
    if sel == "all":
        return x

    def make():   # "open128": exactly 2 CH frames are open after attempt 0
        res = _bpl_model(oracle, case, x)
        opened = np.zeros(len(x), dtype=bool)
        opened[res.attempts[1]["frames"]] = True
        return x[np.sort(np.concatenate([np.flatnonzero(opened)[:2 * ROW_FLOOR], np.flatnonzero(~opened)[:37]]))]
    return once(("bpl rows", case.name), make)


def bpl_want(oracle, case):
    return once(("bpl want", case.name), lambda: _bpl_model(oracle, case, bpl_rows(oracle, case)))


# ---- the cases --------------------------------------------------------------------------------------------------------------
def _row_cases(loop, names):
    return [Case(f"{loop} {nm} B={ROW_BATCHES[kind]}", loop, kind, ROW_CAP, (nm, ROW_BATCHES[kind]))
            for nm in names for kind in ("ragged", "even", "small")]


Q8_CASES = _row_cases("q8", list(Q8_CTX))
RM_CASES = [Case(f"rm E={E} ibil={int(ibil)} B={ROW_BATCHES[kind]}", "rm", kind, RM_CAP, (E, ibil, mode, ROW_BATCHES[kind]))
            for E, ibil, mode in RM_E for kind in ("ragged", "even", "small")]
CONSTRUCT_CASES = _row_cases("construct", [32, 128])
AD_CASES = [Case(f"adaptive {dt} {kind}", "adaptive", kind, ROW_CAP, (dt, kind)) for dt in ("f64", "f32") for kind in ("ragged", "even")]
# T, dtype, kind; the caps make CH = 3 (T = 8: 128 bytes per frame) and CH = 5 (T = 32: 512 bytes)
SCF_CASES = [Case(f"scf T={T} {np.dtype(dt).name} {kind}", "scf", kind, cap, (T, dt, kind))
             for T, cap in ((8, 400), (32, 2600)) for dt in (np.float64, np.float32) for kind in ("ragged",)] + \
            [Case("scf T=8 float64 even", "scf", "even", 400, (8, np.float64, "even"))]
# N, budgets, c, dtype, rows.  pair_bytes is 16 at N = 128: a cap of 400 bytes gives CH = 6 for T = 4, 3 for T = 8, 12 for
# T = 2; 700 bytes give CH = 5 for T = 8; 1 byte gives CH = 1.  At N = 1024 a frame of T = 8 takes 1024 bytes: 7500 bytes give CH = 7.
DSCF_CASES = [Case("dscf (4,4,4) c=1.5", "dscf", "ragged", 400, (128, (4, 4, 4), 1.5, np.float64, "shape")),
              Case("dscf (8,2,4) c=1.5", "dscf", "ragged", 400, (128, (8, 2, 4), 1.5, np.float64, "shape")),
              Case("dscf (8,8) c=0", "dscf", "ragged", 700, (128, (8, 8), 0.0, np.float64, "shape")),
              Case("dscf (32,32) CH=1", "dscf", "ragged", 1, (128, (32, 32), 1.5, np.float64, "shape")),
              Case("dscf (4,4,4) f32", "dscf", "ragged", 400, (128, (4, 4, 4), 1.5, np.float32, "shape")),
              Case("dscf quantised c=1.5", "dscf", "ragged", 400, (128, (4, 4, 4), 1.5, np.float64, "quantised")),
              Case("dscf quantised c=0 f32", "dscf", "ragged", 400, (128, (4, 4, 4), 0.0, np.float32, "quantised")),
              Case("dscf N=1024 (8,8)", "dscf", "ragged", 7500, (1024, (8, 8), 1.5, np.float64, "picked")),
              Case("dscf (4,4) even", "dscf", "even", 400, (128, (4, 4), 1.5, np.float64, "even"))]
# N, K, iterMax, graph list, CRC, the two Eb/N0 points, rows.  loop "bpl0": the staged attempt 0; "bpl": the later attempts
BPL32 = (32, 16, 6, "default", None, (-1.0, 1.0))
BPL32R = (32, 16, 6, "reversal", None, (-1.0, 1.0))
BPL128 = (128, 64, 12, "default", CRC6, (0.0, 1.5))
BPL_CASES = [Case("bpl N=32 default", "bpl", "ragged", ROW_CAP, BPL32 + ("all",)),
             Case("bpl N=32 default open=128", "bpl", "even", ROW_CAP, BPL32 + ("open128",)),
             Case("bpl N=32 default B=65", "bpl", "small", ROW_CAP, BPL32 + (B_SMALL,)),
             Case("bpl N=32 reversal first", "bpl0", "ragged", ROW_CAP, BPL32R + ("all",)),
             Case("bpl N=32 reversal first B=128", "bpl0", "even", ROW_CAP, BPL32R + (B_EVEN,)),
             Case("bpl N=128 CRC-6", "bpl", "ragged", ROW_CAP, BPL128 + (B_RAGGED,))]
FER_CASE = Case("fer rm SCL8", "rm", "lanes", ROW_CAP, (128, 40, 111, 40000, 1.5))   # N, K, E, B, Eb/N0: two lanes of the batch

CASES = Q8_CASES + RM_CASES + CONSTRUCT_CASES + AD_CASES + SCF_CASES + DSCF_CASES + BPL_CASES
LOOPS = ("q8", "rm", "adaptive", "scf", "dscf", "bpl0", "bpl", "construct")


def passes(case, oracle):
    """[(what, frames entering the pass loop, CH)] for every pass loop the case's decode runs, from the models alone"""
    if case.loop in ("q8", "rm", "construct"):
        return [("batch", case.spec[-1], ROW_FLOOR)]
    if case.loop == "adaptive":
        dt, kind = case.spec
        fails = ad_stage_fails(oracle, ad_rows(oracle, kind, dt), dt)
        return [(f"stage {s + 1}", int(f.sum()), ROW_FLOOR) for s, f in enumerate(fails)]
    if case.loop == "scf":
        T = case.spec[0]
        return [("pass B", len(scf_want(oracle, case)[4]), rows_per_pass(case.cap, pair_bytes(SCF_N) * T, SCF_FLOOR))]
    if case.loop == "dscf":
        want = dscf_want(oracle, case)
        return [(f"level {k + 1}", len(want.lists[k]), ch) for k, ch in enumerate(dscf_ch(case))]
    res = bpl_want(oracle, case)
    out = [("attempt 0", len(res.attempts[0]["frames"]), ROW_FLOOR)] if case.loop == "bpl0" else []
    return out + [(f"attempt {p}", len(a["frames"]), ROW_FLOOR) for p, a in enumerate(res.attempts) if p >= 1]
