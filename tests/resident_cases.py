"""The rows that put every persistent kernel through its second, third and ragged last job at small batches (a plain helper
module, imported by tests/test_resident_host.py and tests/test_gpu_resident.py).

Every decoder kernel starts only as many blocks as stay resident at once; a wavefront (or block) takes its first job by its
index and every further one from a counter (csrc/polar_host.h plan_launch(), csrc/polar_params.h next_job_*).  On an MI355X
the resident set is thousands of wavefronts, so a second job on the same wavefront needs batches no model can follow.
polardecoding_amd.testing.resident_blocks() caps the grid of one context; with `cap` blocks of `jpb` jobs each there are
S = cap * jpb slots, and a row of this table runs at caps 1 (one block strictly in sequence: the most carry-over) and 3
(three blocks contend for the counter) on three prefixes of one pool of frames:

  S u              every slot takes one job, no queue: the control
  S u + 1          one queued job, and it is ragged
  3 S u + u + r    r = 1 for pairs, 3 for quads, 37 for jobs of 64 frames, 0 for single frames

A Row names its decoder (`make`), the kernel-name prefix the context must report, the frames per job u, the jobs per block
jpb (the kernel's Cfg::WAVES; the GPU test reads it back with polar_testing_last_plan, so a changed WAVES fails there),
whether the kernel takes its later jobs from the work queue (False: a fixed stride) and the model that every frame of every
output is held to.  The pool holds oracle frames of three Eb/N0 points in turn, rounded to float32 (one pool serves a double
and a float context), with the degenerate rows of llr_families planted behind the first S u frames of cap 1: an all-zero, a
2^20 and a subnormal row come first, directly before and after ordinary rows in one wavefront's job sequence.  A planted row
that lies inside cap 1's largest batch is in a later job there; one beyond it is at an index >= 3 S u of cap 1, which is
S u of cap 3.  Models are computed once per process on the whole pool; a batch is a prefix."""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import llr_families as F  # noqa: E402
from test_bp_early_stop_host import stop_points  # noqa: E402
from test_cascl_adaptive_host import FLAG_CRC_PASS  # noqa: E402
from test_scan_host import scan_model  # noqa: E402
from test_scf_host import scf_model  # noqa: E402
from dscf_model import dscf_model  # noqa: E402
import q8_model as QM  # noqa: E402
import dyn_families as DF  # noqa: E402
import wide_families as WF  # noqa: E402
import list_model as LM  # noqa: E402
import test_rm_host as RM  # noqa: E402

CRC6 = (0, 1, 6)
CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)
CAPS = (1, 3)
RAGGED = {1: 0, 2: 1, 4: 3, 64: 37}
AUTO, GENERIC, GENERIC_SPILL, BIG, ONE_PER_WAVE, FOUR_PER_WAVE = range(6)   # polardecoding_amd.testing.KERNEL_*
TAU = 5.0

# name; kind (which model and which entry point); N, K; constructor arguments in `spec`; kernel-name prefix; u; jpb; queue
Row = namedtuple("Row", "name kind N K spec prefix u jpb queue dbs seed")
_memo = {}


def once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def slots(row, cap):
    return cap * row.jpb


def batches(row, cap):
    """(control, one ragged queued job, three rounds and a ragged rest)"""
    su = slots(row, cap) * row.u
    return su, su + 1, 3 * su + row.u + RAGGED[row.u]


def pool_size(row):
    return batches(row, CAPS[-1])[2]


def jobs(row, B):
    return -(-B // row.u)


def f32_exact(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def info_order(N, A):
    """the A most reliable positions, ascending reliability: the 5G order restricted to < N as polar_create derives it; above
    N = 1024 (no 5G table) the beta-expansion order with beta = 2^(1/4), handed to the decoder as its info_order"""
    if N <= 1024:
        return np.asarray(RM.q_order(N)[N - A:], dtype=np.int32)
    j = np.arange(N)
    w = sum(((j >> b) & 1) * 2.0 ** (b / 4.0) for b in range(N.bit_length() - 1))
    return np.argsort(w, kind="stable")[N - A:].astype(np.int32)


def taps_of(row):
    return row.spec.get("taps")


def code_of(oracle, row):
    def make():
        taps = taps_of(row)
        A = row.K + (max(taps) if taps else 0)
        io = info_order(row.N, A).tolist()
        s = set(io)
        code = oracle.Code(row.N, row.K, taps, Q=[j for j in range(row.N) if j not in s] + io)
        assert code.info_order.tolist() == io
        return code
    return once(("code", row.N, row.K, taps_of(row)), make)


def degenerate(width, dtype, seed):
    """llr_families.degenerate_rows with the all-zero, the 2^20 and the subnormal row first"""
    rows = dict(F.degenerate_rows(width, dtype, seed, c=2.0))
    first = ["zero+", "2^20", "subnormal"]
    return [(k, rows[k]) for k in first] + [(k, v) for k, v in rows.items() if k not in first]


def planted_from(row):
    return batches(row, CAPS[0])[0]


def plant(x, rows, lanes):
    """llr_families.plant() for the kernels that decode one codeword per lane (it puts the rows on the wavefront boundaries
    first); for the others it would fill the few frames of cap 1's later jobs with degenerate rows alone, so there every
    second frame (offsets 1, 3, 5, ...) takes the next degenerate row, once"""
    if lanes:
        return F.plant(x, rows)
    x = np.array(x, copy=True)
    for i, p in enumerate(range(1, len(x), 2)):
        if i < len(rows):
            x[p] = rows[i][1]
    return x


def family_case(row):
    """(module, Case, Made) of a row on a case of tests/dyn_families.py or tests/wide_families.py"""
    mod = DF if row.spec["module"] == "dyn" else WF
    c = mod.Case(*row.spec["case"])
    return mod, c, mod.materialise(c)


def _planted_pool(row, x):
    x = np.array(x[:pool_size(row)], dtype=np.float64)
    assert len(x) == pool_size(row)
    if row.spec.get("plant", True):
        dt = np.float32 if row.spec.get("f32") else np.float64
        p0 = planted_from(row)
        x[p0:] = plant(x[p0:], degenerate(row.N, dt, row.seed), row.u == 64).astype(np.float64)
    x.setflags(write=False)
    return x


def pool(oracle, row):
    """[pool_size][N] float64, exact in float32: frames of the row's three Eb/N0 points in turn; the degenerate rows planted
    behind cap 1's first round.  With spec["y"] the rows are channel observations for spec["sigma"]."""
    def make():
        if row.kind == "fam":   # the family's own rows (its frames carry its dynamic bits), the first input batch of the case
            _, c, made = family_case(row)
            return _planted_pool(row, made.batches[c.inputs[0]][row.spec.get("offset", 0):])
        code = code_of(oracle, row)
        B = pool_size(row)
        per = -(-B // len(row.dbs))
        x = np.empty((per * len(row.dbs), row.N))
        for k, db in enumerate(row.dbs):
            sig = oracle.sigma_from_db(db)
            _, ys = oracle.Sim(row.seed + k).frames(code, sig, per)
            x[k::len(row.dbs)] = ys if row.spec.get("y") else np.stack([oracle.llr_from_y(y, sig) for y in ys])
        return _planted_pool(row, f32_exact(x))
    return once(("pool", row.name), make)


def planted(oracle, row):
    """{name: [pool positions]} of the degenerate rows that pool() planted"""
    x = pool(oracle, row)
    dt = np.float32 if row.spec.get("f32") else np.float64
    out = {}
    for name, r in degenerate(row.N, dt, row.seed):
        hit = np.flatnonzero((x.view(np.uint64) == r.astype(np.float64).view(np.uint64)[None, :]).all(axis=1))
        if hit.size:
            out[name] = hit.tolist()
    return out


def _llr_rows(oracle, row, x):
    """the LLR rows the kernel decodes: x itself, or from observations as the kernel forms them (in double from the row as
    the context reads it, rounded to the arithmetic type)"""
    if not row.spec.get("y"):
        return x
    llr = np.stack([oracle.llr_from_y(r, row.spec["sigma"]) for r in x])
    return llr.astype(np.float32).astype(np.float64) if row.spec.get("f32") else llr


def want(oracle, row):
    """the model's outputs for the whole pool, a tuple of arrays with one entry per frame each"""
    def make():
        if row.kind == "fam":
            mod, c, made = family_case(row)
            if mod is DF:
                u, pm, flags = DF.model(c, made, pool(oracle, row), oracle=oracle)
            else:
                u, pm, flags = WF.model_on(made.mask, made.dyn, pool(oracle, row), c.L, c.dtype, crc=(made.order, made.taps) if made.taps else None)
            return u, np.asarray(pm, dtype=np.float64), np.asarray(flags).astype(np.uint32)
        x, code = pool(oracle, row), code_of(oracle, row)
        f32 = bool(row.spec.get("f32"))
        dts, dtn = ("f32" if f32 else "f64"), (np.float32 if f32 else np.float64)
        if row.kind == "list":
            uh, pm, ties = oracle.decode(code, _llr_rows(oracle, row, x), "CASCL" if taps_of(row) else "SCL", L=row.spec["L"], dtype=dts)
            return uh, pm, ties > 0
        if row.kind == "sc":
            return (oracle.decode(code, x, "SC", dtype=dts)[0],)
        if row.kind == "bp":
            return (oracle.decode(code, x, "BP", bp_iters=row.spec["iters"], dtype=dts)[0],)
        if row.kind == "bpstop":
            t, conv, out = stop_points(x, code.frozen, row.spec["iters"])
            return out, np.asarray(t, dtype=np.int64), np.asarray(conv, dtype=bool)
        if row.kind == "scan":
            return scan_model(code.frozen, x.astype(dtn), row.spec["I"], dtype=dtn, oracle=oracle, skip=True)
        if row.kind == "scf":
            u, flags, attempts, _, _ = scf_model(code, x, row.spec["T"], dtype=dtn, oracle=oracle)
            return u, np.asarray(flags, dtype=np.int64), np.asarray(attempts, dtype=np.int64)
        if row.kind == "dscf":
            m = dscf_model(code, x, row.spec["budgets"], row.spec["c"], TAU, dtype=dtn, oracle=oracle)
            return m.u, np.asarray(m.flags, dtype=np.int64), np.asarray(m.attempts, dtype=np.int64), np.asarray(m.sets, dtype=np.int64)
        if row.kind == "q8":
            q = QM.quantize(x)
            u, pm, flags = QM.decode_rows(q, code.frozen, row.spec["L"], crc=(code.info_order, taps_of(row)) if taps_of(row) else None,
                                          sc=False)
            return u, np.asarray(pm).astype(np.int64), np.asarray(flags).astype(np.uint32)
        if row.kind == "listout":
            paths, pm, rem, count, flags = LM.list_model(code.frozen, None, x, row.spec["L"], crc=(code.info_order, taps_of(row)) if taps_of(row) else None,
                                                         dtype=dtn, oracle=oracle)
            return (np.asarray(paths), np.asarray(pm, dtype=np.float64), np.asarray(rem).astype(np.uint32), np.asarray(count).astype(np.uint32),
                    np.asarray(flags).astype(np.uint32))
        raise ValueError(row.kind)
    return once(("want", row.name), make)


def sent(oracle, row):
    """the words the pool's frames carry ([pool_size][N]; the planted rows carry none and count as not decoded to it)"""
    def make():
        if row.kind == "fam":
            o = row.spec.get("offset", 0)
            return np.asarray(family_case(row)[2].u[o:o + pool_size(row)], dtype=np.int32)
        code = code_of(oracle, row)
        B = pool_size(row)
        per = -(-B // len(row.dbs))
        u = np.empty((per * len(row.dbs), row.N), dtype=np.int32)
        for k, db in enumerate(row.dbs):
            u[k::len(row.dbs)] = oracle.Sim(row.seed + k).frames(code, oracle.sigma_from_db(db), per)[0]
        return u[:B]
    return once(("sent", row.name), make)


def _r(name, kind, N, K, prefix, u, jpb, dbs, seed, queue=True, **spec):
    return Row(name, kind, N, K, spec, prefix, u, jpb, queue, dbs, seed)


LOW = (0.5, 1.5, 2.5)
MID = (1.0, 2.0, 3.0)
SIGMA_Y = 0.84

LIST_ROWS = [
    _r("fast128 f64", "list", 128, 64, "k_scl_fast<double,N=128", 1, 4, MID, 1100, L=8, taps=CRC6),
    # the float N = 128 kernel loops by a fixed stride (k_fast.hip)
    _r("fast128 f32", "list", 128, 64, "k_scl_fast<float,N=128", 1, 4, MID, 101, queue=False, L=8, taps=CRC6, f32=True),
    _r("fast1024 one per wave", "list", 1024, 512, "k_scl_fast<double,N=1024", 1, 4, LOW, 102, L=8, taps=CRC24C, variant=ONE_PER_WAVE),
    _r("fast2 f64", "list", 1024, 512, "k_scl_fast2<double", 2, 4, LOW, 103, L=8, taps=CRC24C),
    _r("fast2 f32", "list", 1024, 512, "k_scl_fast2<float", 2, 4, LOW, 104, L=8, taps=CRC24C, f32=True),
    _r("fast2_y f64", "list", 1024, 512, "k_scl_fast2<double", 2, 4, LOW, 105, L=8, taps=CRC24C, y=True, sigma=SIGMA_Y),
    _r("fast2_y f32", "list", 1024, 512, "k_scl_fast2<float", 2, 4, LOW, 106, L=8, taps=CRC24C, f32=True, y=True, sigma=SIGMA_Y),
    _r("fast4", "list", 1024, 512, "k_scl_fast4<double", 4, 4, LOW, 107, L=8, taps=CRC24C, variant=FOUR_PER_WAVE),
    _r("big L32 f64", "list", 1024, 512, "k_scl_big<double,L=32", 1, 4, LOW, 108, L=32),
    _r("big L32 f32", "list", 1024, 512, "k_scl_big<float,L=32", 1, 4, LOW, 109, L=32, f32=True),
    _r("big chain N2048 L16", "list", 2048, 1024, "k_scl_big<double,L=16", 1, 4, LOW, 110, L=16, taps=CRC24C, own_order=True),
    _r("generic L4", "list", 256, 128, "k_scl_generic<double,L=4", 1, 1, MID, 1112, L=4),
    _r("generic spill L8", "list", 128, 64, "k_scl_generic<double,L=8", 1, 1, MID, 1116, L=8, variant=GENERIC_SPILL),
]
SC_ROWS = [
    _r("SC below 64 frames", "sc", 128, 64, "k_scl_generic<double,L=1", 1, 1, MID, 1123, variant=GENERIC),
    _r("sc_lanes N64", "sc", 64, 20, "k_sc_lanes<double", 64, 4, (0.0, 2.0, 4.0), 121),
    _r("sc_lanes N128", "sc", 128, 64, "k_sc_lanes<double", 64, 4, MID, 122),
]
SCAN_ROWS = [
    _r(f"scan N{N} I{I} {'f32' if f32 else 'f64'}", "scan", N, K, "k_scan_lanes<" + ("float" if f32 else "double"), 64, 4, MID,
       130 + N + f32, I=I, f32=f32)
    for N, K, I in ((32, 16, 3), (128, 64, 2)) for f32 in (False, True)
]
BP_SEED = {("bp_w128", False): 1268, ("bp_w128", True): 1270, ("bp N256", False): 1396, ("bp N256", True): 1396}
BP_ROWS = [
    _r(f"{nm}{' stop' if stop else ''}", "bpstop" if stop else "bp", N, N // 2, prefix, 1, jpb, (1.0, 2.5, 4.0), BP_SEED.get((nm, stop), 140 + N), queue=q,
       iters=it, own_order=N > 1024)
    for nm, N, prefix, jpb, it, q in (("bp_w128", 128, "k_bp_w128<double", 4, 12, True), ("bp N256", 256, "k_bp<double", 1, 10, True),
                                       ("bp_r4", 1024, "k_bp_r4<double", 1, 5, True),
                                       ("bp_global N2048", 2048, "k_bp<double", 1, 3, False))
    for stop in (False, True)
]
SCF_ROWS = [
    _r("scf T4", "scf", 128, 64, "k_scf_lanes<double", 64, 4, MID, 150, T=4, taps=CRC6),
    _r("dscf omega2", "dscf", 128, 64, "k_scf_lanes<double", 64, 4, MID, 151, budgets=(4, 4), c=1.5, taps=CRC6),
]
Q8_ROWS = [
    _r("q8 L8", "q8", 128, 64, "k_scl_q8", 1, 1, MID, 160, L=8, taps=CRC6),
]
# dyn_families / wide_families Case fields: group, N, mask, constraint family, L, dtype, algo, frames, Eb/N0 points, inputs
FAM_ROWS = [
    _r("dyn N32 L2 f32", "fam", 32, 16, "k_scl_dyn<float,L=2", 1, 1, None, 170, f32=True, module="dyn", offset=10,
       case=("n32", 32, "rm", "bern_half", 2, "f32", "SCL", 300, DF.DBS4, DF.LLR_FAMILIES)),
    _r("wide L64", "fam", 64, 0, "k_scl_wide<double,L=64", 1, 1, None, 171, module="wide", offset=9,
       case=("resident", 64, "sparse_5_half", WF.NONE, 64, "f64", "SCL", 64, WF.DBS2, ("awgn",))),
    _r("wide L256 global scratch", "fam", 128, 0, "k_scl_wide<double,L=256", 1, 1, None, 172, module="wide",
       case=("resident", 128, "bern_0.5", WF.NONE, 256, "f64", "SCL", 12, WF.DBS2, ("awgn",))),
]
LISTOUT_ROWS = [
    _r("k_scl_list L4", "listout", 32, 16, "k_scl_generic<double,L=4", 1, 1, (1.0, 3.0, 5.0), 1180, L=4),
    _r("wide LIST L64", "listout", 128, 64, "k_scl_wide<double,L=64", 1, 1, MID, 181, L=64),
]
ROWS = LIST_ROWS + FAM_ROWS + LISTOUT_ROWS + SC_ROWS + SCAN_ROWS + BP_ROWS + SCF_ROWS + Q8_ROWS
