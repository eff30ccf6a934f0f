"""The load stage of every decode kernel: row type, y form and alignment (a plain helper module, imported by
tests/test_input_forms_host.py and tests/test_gpu_input_forms.py; no GPU is touched at import).

Every decode kernel starts by turning element i of the caller's row into a working LLR, and include/polar_hip.h ("Input rows")
states the rule once:

    v = (double)row[i];  if (sigma > 0) v = 2 * v / sigma / sigma;  working value = (R)v

R is the context's arithmetic type, IN the type of the rows; each of the four (R, IN) pairs is a template instantiation of
its own, the y form is a third axis and the address of the rows a fourth (a row needs the alignment of its element type
only).  form_rows() is the numpy statement of the rule, FORMS the product of the four axes, place() puts rows at a chosen
residue modulo 16 inside a NaN frame, CASES lists one context per kernel instantiation family at the smallest shape that
selects it, DISPATCH names the kernel family each (case, R, IN) cell runs, and EXEMPT the entry points whose load stage
another file already holds at a shifted address.

Base rows are Gaussian at 1 to 2 dB and rounded to float32 first, so that double and float rows carry the same values and a
(case, R) needs two references only: the LLR form and the y form.  The sigma of the y form is generic on purpose: with a
power of two 2*y/(sigma*sigma), float arithmetic and the rule all agree, with SIGMA they do not
(tests/test_input_forms_host.py shows the path metrics that separate them).

reference() is the CPU answer of a case on rows formed by form_rows(): oracle.decode for SC, SCL, CA-SCL and BP, and the
numpy models the suite already has for the rest (scf_model, dscf_model, scan_model, list_model, bpl_model, dscl_model for
dynamic frozen bits and wide lists, genie_model, the oracle composition of the adaptive rule, stop_points).  bpl_model and
stop_points are written in binary64; typed_stop_points() and typed_bpl() restate them for either type on the oracle's CHK
and are held to them (f64) and to the oracle's fixed-iteration BP (f32) by the host file."""
import ctypes as C
import os
import re
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (HERE, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import bpl_model as BM  # noqa: E402
import extents as EX  # noqa: E402  (ctx, make_ctx, prototypes: the header parser of the output-extent tests)
import list_model as LM  # noqa: E402
import test_construct_host as MC  # noqa: E402
import test_dyn_host as DM  # noqa: E402
import test_gpu_cascl_adaptive as AD  # noqa: E402  (_oracle_composition; imports no GPU package)
from dscf_model import dscf_model  # noqa: E402
from test_bp_early_stop_host import stop_points  # noqa: E402
from test_cascl_adaptive_host import CRC6, CRC24C, FLAG_CRC_PASS, syndrome  # noqa: E402
from test_gpu_bpl import _beta_order  # noqa: E402
from test_scan_host import scan_model  # noqa: E402
from test_scf_host import scf_model  # noqa: E402

CSRC = os.path.join(REPO, "polardecoding_amd", "csrc")
NP = {"f64": np.float64, "f32": np.float32}
C_NAME = {"f64": "double", "f32": "float"}
SIGMA = 10 ** (-1.5 / 20)          # 1.5 dB at rate 1/2: not a power of two
FLAG_TIE, FLAG_RERANK, FLAG_BP_CONVERGED = 1, 4, 8
ENOKERNEL = -4
PAD = 64                           # elements of NaN behind the last row, at least


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def form_rows(x, in_dtype, sigma, r_dtype):
    """the working LLRs of rows x handed in as in_dtype with sigma, in a context of arithmetic type r_dtype"""
    v = np.asarray(x).astype(NP[in_dtype]).astype(np.float64)
    if sigma > 0:
        v = 2 * v / sigma / sigma
    return v.astype(NP[r_dtype])


def wrong_rows(x, sigma, which):
    """rows of an f64 context formed by a rule that is not the library's, for a y form (sigma > 0):
    "assoc" 2*y/(sigma*sigma); "float product" the same steps as the rule, in float on float rows; "rounded" the LLRs of
    the rule rounded to float before the f64 context takes them"""
    x = np.asarray(x)
    if which == "assoc":
        return (2 * x.astype(np.float64) / (sigma * sigma)).astype(np.float64)
    if which == "float product":
        s = np.float32(sigma)
        return (np.float32(2) * x.astype(np.float32) / s / s).astype(np.float64)
    if which == "rounded":
        return form_rows(x, "f64", sigma, "f64").astype(np.float32).astype(np.float64)
    if which == "no sigma":
        return x.astype(np.float64)
    raise ValueError(which)


WRONG_RULES = ("assoc", "float product", "rounded")

Form = namedtuple("Form", "R IN sigma shift")
FORMS = [Form(R, IN, sigma, shift) for R in ("f64", "f32") for IN in ("f64", "f32") for sigma in (0.0, SIGMA)
         for shift in ((0, 1) if IN == "f64" else (0, 1, 2))]


def form_id(f):
    return f"R={f.R} IN={f.IN} {'y' if f.sigma > 0 else 'llr'} shift={f.shift}"


# ---- placement ------------------------------------------------------------------------------------------------------------------
Placed = namedtuple("Placed", "rows whole shift")


def place(x, shift, backend="numpy"):
    """Placed(rows, whole, shift): `rows` is a view with x's values that starts `shift` elements into `whole`, a fresh
    16-byte-aligned allocation of x's type whose every other element is NaN, PAD or more of them behind the last row.
    backend "numpy" (host) or "torch" (a CUDA tensor)."""
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float64, np.float32) and shift >= 0
    total = shift + x.size + PAD
    if backend == "torch":
        import torch
        whole = torch.full((total,), float("nan"), dtype=torch.float32 if x.dtype == np.float32 else torch.float64, device="cuda")
        assert whole.data_ptr() % 16 == 0
        rows = whole[shift:shift + x.size].view(x.shape)
        rows.copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        return Placed(rows, whole, shift)
    raw = np.empty(total * x.itemsize + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    whole = raw[off:off + total * x.itemsize].view(x.dtype)
    whole[:] = np.nan
    rows = whole[shift:shift + x.size].reshape(x.shape)
    rows[...] = x
    return Placed(rows, whole, shift)


def address(t):
    return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def frame_intact(p, x):
    """the rows of a placement still hold x bit for bit, and every element of the allocation outside them is NaN"""
    whole = p.whole if isinstance(p.whole, np.ndarray) else p.whole.cpu().numpy()
    x = np.ascontiguousarray(x)
    inside = whole[p.shift:p.shift + x.size]
    return bool(np.isnan(whole[:p.shift]).all() and np.isnan(whole[p.shift + x.size:]).all() and
                len(whole) >= p.shift + x.size + PAD and inside.tobytes() == x.tobytes())


# ---- the cases ------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name entry ctx B ref family opts")
PAIRS = [(R, IN) for R in ("f64", "f32") for IN in ("f64", "f32")]


def _case(name, entry, c, B, ref, family, f64_on_float=None, **opts):
    """family: the kernel family (or a tuple of them, for a decoder of several launches) that every (R, IN) runs;
    f64_on_float: what an f64 context runs on float rows where fast_ok() sends them elsewhere"""
    fam = {p: family for p in PAIRS}
    if f64_on_float is not None:
        fam[("f64", "f32")] = f64_on_float
    return Case(name, entry, c, B, ref, fam, opts)


def _cases():
    ctx = EX.ctx
    DEV, BPD = "polar_decode_device", "polar_bp_decode_device"
    c1024 = dict(L=8, crc_taps=CRC24C)
    io2048 = tuple(_beta_order(2048)[1024:])   # the 5G table stops at 1024: one explicit order for the library and the oracle
    out = [
        # one codeword per lane: 64 frames and more
        _case("sc_lanes N=128", DEV, ctx("SC", 128, 64), 67, "sc", "k_sc_lanes"),
        # the generic list kernel, and its levels in global scratch
        _case("generic N=64 L=1", DEV, ctx("SCL", 64, 32, L=1), 7, "scl", "k_scl_generic"),
        _case("generic N=64 L=4", DEV, ctx("SCL", 64, 32, L=4), 7, "scl", "k_scl_generic"),
        _case("generic N=64 L=32", DEV, ctx("SCL", 64, 32, L=32), 7, "scl", "k_scl_generic", seed=4109),
        _case("generic spill N=64 L=8", DEV, ctx("SCL", 64, 32, "KERNEL_GENERIC_SPILL", L=8), 7, "scl", "k_scl_generic"),
        # L = 8 at N = 128 and N = 1024: an f64 context on float rows leaves the tuned kernels (fast_ok, polar_hip.hip)
        _case("fast N=128 CRC-6", DEV, ctx("CASCL", 128, 64, L=8, crc_taps=CRC6), 9, "cascl", "k_scl_fast", "k_scl_generic"),
        _case("fast N=1024 one per wave", DEV, ctx("CASCL", 1024, 512, "KERNEL_ONE_PER_WAVE", **c1024), 5, "cascl", "k_scl_fast",
              "k_scl_big"),
        _case("fast2 N=1024 SCL", DEV, ctx("SCL", 1024, 512, L=8), 5, "scl", "k_scl_fast2", "k_scl_big"),
        _case("fast2 N=1024 CA-SCL", DEV, ctx("CASCL", 1024, 512, **c1024), 5, "cascl", "k_scl_fast2", "k_scl_big"),
        _case("fast2 N=1024 CA-SCL timed", "polar_time_decode_device", ctx("CASCL", 1024, 512, **c1024), 5, "cascl", "k_scl_fast2",
              "k_scl_big"),
        _case("fast4 N=1024 four per wave", DEV, ctx("CASCL", 1024, 512, "KERNEL_FOUR_PER_WAVE", **c1024), 5, "cascl", "k_scl_fast4",
              "k_scl_big"),
        _case("big N=512 L=2", DEV, ctx("SCL", 512, 256, L=2), 5, "scl", "k_scl_big"),
        _case("big N=1024 L=32", DEV, ctx("CASCL", 1024, 512, L=32, crc_taps=CRC24C), 5, "cascl", "k_scl_big"),
        _case("big N=2048 L=4 spilled levels", DEV, ctx("SCL", 2048, 1024, L=4, info_order=io2048), 5, "scl", "k_scl_big"),
        _case("dyn PAC(64, 32) L=8", DEV, ctx("PAC", 64, 32, L=8), 7, "dyn", "k_scl_dyn"),
        _case("wide N=32 L=64", DEV, ctx("SCL", 32, 16, L=64), 5, "dyn", "k_scl_wide"),
        _case("list N=64 L=8", "polar_list_decode", ctx("CASCL", 64, 32, L=8, crc_taps=CRC6), 7, "list", "k_scl_list"),
    ]
    # BP: two or three round trips, the stop rule off and on; the messages of N = 2048 do not fit a CU's LDS
    for fam, N, it in (("k_bp_w128", 128, 3), ("k_bp_r4", 1024, 2), ("k_bp", 256, 3), ("k_bp_global", 2048, 2)):
        for rule in (None, "g"):
            kw = dict(iterMax=it, early_stop=rule)
            if N == 2048:
                kw["info_order"] = io2048
            out.append(_case(f"{fam} N={N} stop {rule or 'none'}", BPD, ctx("BP", N, N // 2, **kw), 5, "bp", fam))
    out += [
        _case("bp readout N=128", "polar_bp_readout_device", ctx("BP", 128, 64, iterMax=4), 5, "readout", "k_bp_readout",
              checkpoints=(2, 4)),
        _case("scf T=2 N=128", "polar_scf_decode_device", ctx("SCF", 128, 64, T=2, crc_taps=CRC6), 67, "scf", "k_scf_lanes"),
        _case("dscf (2,2) N=128", "polar_scf_decode_sets_device", ctx("DSCF", 128, 64, budgets=(2, 2), c=1.5, tau=5.0, crc_taps=CRC6),
              67, "dscf", "k_scf_lanes"),
        _case("scan N=128 I=2", "polar_scan_decode_device", ctx("SCAN", 128, 64, iters=2), 67, "scan", "k_scan_lanes"),
        _case("genie N=128", "polar_genie_count_device", ctx("SC", 128, 64), 67, "genie", "k_genie_lanes"),
        # a later stage with fewer than 64 open frames runs SC on the generic kernel
        _case("adaptive (1,2,8) N=128", "polar_cascl_decode_device", ctx("CASCL", 128, 64, L=8, crc_taps=CRC6, stages=(1, 2, 8)), 67,
              "adaptive", ("k_sc_lanes", "k_scl_generic", "k_scl_fast"), ("k_sc_lanes", "k_scl_generic")),
        _case("bpl P=2 N=128", "polar_bpl_decode_device", ctx("BPL", 128, 64, iterMax=12, graphs=2, crc_taps=CRC6), 13, "bpl",
              ("k_bp_w128",)),
        # the chunked passes (polardecoding_amd.testing.chunk_bytes): stage 1 of the adaptive rule takes more than 64 open
        # frames, every failing SC-Flip frame is a pass of its own, and attempt 0 of a list that starts with the stage
        # reversal is staged in passes of 64 frames, the second one from d_in + 64 rows
        _case("adaptive (1,2,8) N=128 chunked", "polar_cascl_decode_device",
              ctx("CASCL", 128, 64, L=8, crc_taps=CRC6, stages=(1, 2, 8)), 197, "adaptive",
              ("k_sc_lanes", "k_scl_generic", "k_scl_fast"), ("k_sc_lanes", "k_scl_generic"), cap=1),
        _case("scf T=2 N=128 chunked", "polar_scf_decode_sets_device", ctx("SCF", 128, 64, T=2, crc_taps=CRC6), 67, "scf",
              "k_scf_lanes", cap=1),
        _case("bpl reversal first N=128 chunked", "polar_bpl_decode_device",
              ctx("BPL", 128, 64, iterMax=12, graphs=((6, 5, 4, 3, 2, 1, 0), (1, 2, 3, 4, 5, 6, 0))), 67, "bpl", ("k_bp_w128",), cap=1),
    ]
    return out


CASES = _cases()
DISPATCH = {c.name: dict(c.family) for c in CASES}

# the d_in, in_is_f32 entry points whose load stage another file already holds at a shifted address
EXEMPT = {
    "polar_rm_recover_device": "tests/test_gpu_rm.py",
    "polar_q8_quantize_device": "tests/test_gpu_q8_cases.py",
    "polar_codebook_decode": "tests/test_gpu_codebook.py",
    "polar_codebook_list_decode": "tests/test_gpu_codebook.py",
}

# kernel family -> (the k_*.hip units that dispatch it, the launcher whose instantiations they spell out).  The units that
# go through launch_scl_types name no type themselves: the four pairs stand in k_scl_launch.h (launch_scl_l).
FAMILY_SRC = {
    "k_sc_lanes": (("k_sc.hip",), "launch_sc_lanes"),
    "k_scl_generic": (("k_generic.hip",), "launch_scl_types"),
    "k_scl_dyn": (("k_dyn.hip",), "launch_scl_types"),
    "k_scl_fast": (("k_fast.hip",), "launch_fast_n"),
    "k_scl_fast2": (("k_fast2.hip",), "launch_fast2"),
    "k_scl_fast4": (("k_fast4.hip",), "launch_fast4"),
    "k_scl_big": (("k_big_f64.hip", "k_big_f32.hip"), "launch_big_l"),
    "k_scl_wide": (("k_wide.hip",), "launch_wide_l"),
    "k_scl_list": (("k_list.hip",), "launch_list_l"),
    "k_bp_w128": (("k_bp.hip",), "launch_bp"),
    "k_bp_r4": (("k_bp.hip",), "launch_bp"),
    "k_bp": (("k_bp.hip",), "launch_bp"),
    "k_bp_global": (("k_bp.hip",), "launch_bp"),
    "k_bp_readout": (("k_bp.hip",), "launch_bp_readout"),
    "k_scf_lanes": (("k_scf.hip",), "launch_scf_lanes"),
    "k_scan_lanes": (("k_scan.hip",), "launch_scan_lanes"),
    "k_genie_lanes": (("k_genie.hip",), "launch_genie_lanes"),
}
# units whose d_in entry points are EXEMPT (the code book) or that have no float rows at all (Q8 decodes int8)
EXEMPT_UNITS = ("k_book.hip", "k_q8.hip", "k_rm.hip")
_SPELLED = re.compile(r"\b(launch_\w+)<(?:\w+, )?(double|float), (double|float)\b")


def spelled(unit):
    """{(launcher, R, IN)} of the instantiation lines a dispatcher unit spells out"""
    with open(os.path.join(CSRC, unit)) as f:
        text = f.read()
    names = {"double": "f64", "float": "f32"}
    return {(m.group(1), names[m.group(2)], names[m.group(3)]) for m in _SPELLED.finditer(text)}


def families_of(cell):
    return () if cell is None else (cell,) if isinstance(cell, str) else tuple(cell)


# ---- codes and rows -------------------------------------------------------------------------------------------------------------
_memo = {}


def once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def taps_of(case):
    t = case.ctx["kw"].get("crc_taps")
    return tuple(t) if t else None


def code_of(case):
    """(info_order [A], dyn or None, taps or None, frozen [N]) of a case's context, from the host helpers alone"""
    def make():
        import polardecoding_amd as pa
        N, K, kw = case.ctx["N"], case.ctx["K"], case.ctx["kw"]
        taps = taps_of(case)
        A = K + (max(taps) if taps else 0)
        dyn = None
        if case.ctx["kind"] == "PAC":
            io = pa.pac_info_order(N, K, "rm")
            dyn = pa.dyn_pac(N, io, DM.G133)
        elif "info_order" in kw:
            io = np.asarray(kw["info_order"], dtype=np.int32)
        else:
            io = np.asarray(pa.q_sequence(N)[N - A:], dtype=np.int32)
        assert len(io) == A
        fz = np.ones(N, dtype=np.uint8)
        fz[io] = 0
        return io, dyn, taps, fz
    return once(("code", case.name), make)


def oracle_code(case, oracle):
    """the oracle's code with the case's information set (an explicit reliability order: N = 2048 has no 5G table)"""
    def make():
        io, _, taps, _ = code_of(case)
        N, K = case.ctx["N"], case.ctx["K"]
        s = set(io.tolist())
        code = oracle.Code(N, K, taps, Q=[j for j in range(N) if j not in s] + io.tolist())
        assert np.array_equal(code.info_order, io)
        return code
    return once(("oracle code", case.name), make)


def base_rows(case):
    """[B][N] float64 rows, exact in float32: 0.7 times the channel LLRs of codewords of the case's code at 1, 1.5 and 2 dB (as
    LLRs they are a pessimistic receiver's, as y values with SIGMA an optimistic one's: frames fail in both forms, and BP
    converges on some frames in both); the genie rows are the design rows of the all-zero codeword.  opts["seed"]: the seed
    of a case whose default batch does not separate the rules (tests/test_input_forms_host.py)."""
    def make():
        N, seed = case.ctx["N"], case.opts.get("seed", 4000 + CASES.index(case))
        if case.ref == "genie":
            llr = MC.design_rows(N, case.B, 0.8, seed)
        else:
            io, dyn, taps, _ = code_of(case)
            _, llr = DM.make_frames(N, io, dyn, case.B, seed, dbs=(1.0, 1.5, 2.0), crc=taps)
        return (0.7 * llr).astype(np.float32).astype(np.float64)
    return once(("rows", case.name), make)


def sent_bits(case):
    """[B][N] 0/1: the bits the read-out of a BP context compares with (any bits do: the table counts mismatches)"""
    return np.random.default_rng(77).integers(0, 2, (case.B, case.ctx["N"])).astype(np.int32)


def make_dec(case, R):
    """the library context of a case in arithmetic type R, with its test-only kernel choice and chunk cap (the caller closes it)"""
    c = dict(case.ctx, kw=dict(case.ctx["kw"], dtype=R))
    if "info_order" in c["kw"]:
        c["kw"]["info_order"] = np.asarray(c["kw"]["info_order"], dtype=np.int32)
    if "graphs" in c["kw"] and not isinstance(c["kw"]["graphs"], int):
        c["kw"]["graphs"] = [list(g) for g in c["kw"]["graphs"]]
    dec = EX.make_ctx(c)
    if "cap" in case.opts:
        from polardecoding_amd import testing as T
        T.chunk_bytes(dec, case.opts["cap"])
    return dec


# ---- BP with the stop rule and BP list decoding, in either type -------------------------------------------------------------------
def typed_bp_rounds(oracle, llr, frozen, iters, dtype):
    """bp_rounds of tests/test_bp_early_stop_host.py in `dtype`, the check node from the oracle (po_math): yields (u_hat, x_hat)
    after each round trip"""
    llr = np.ascontiguousarray(llr, dtype=dtype)
    B, N = llr.shape
    n = N.bit_length() - 1
    fz = np.asarray(frozen, dtype=bool)

    def chk(a, b):
        return oracle.math(0, a.ravel(), b.ravel(), dtype=dtype).reshape(a.shape)

    l = np.zeros((n + 1, B, N), dtype=dtype)
    r = np.zeros((n + 1, B, N), dtype=dtype)
    l[n] = llr
    r[0] = np.where(fz, dtype(999.0), dtype(0.0))[None, :]
    upper = [np.array([k for k in range(N) if not k & (1 << i)]) for i in range(n)]
    for _ in range(iters):
        for i in range(n):
            s, j = 1 << i, upper[i]
            a = chk(r[i][:, j], l[i + 1][:, j + s] + r[i][:, j + s])
            b = r[i][:, j + s] + chk(r[i][:, j], l[i + 1][:, j])
            r[i + 1][:, j], r[i + 1][:, j + s] = a, b
        for i in range(n - 1, -1, -1):
            s, j = 1 << i, upper[i]
            a = chk(l[i + 1][:, j], l[i + 1][:, j + s] + r[i][:, j + s])
            b = l[i + 1][:, j + s] + chk(r[i][:, j], l[i + 1][:, j])
            l[i][:, j], l[i][:, j + s] = a, b
        assert l.dtype == dtype and r.dtype == dtype
        u_hat = np.where(fz[None, :], 0, np.where(l[0] + r[0] >= 0, 0, 1)).astype(np.int32)
        yield u_hat, np.where(l[n] + r[n] >= 0, 0, 1).astype(np.int32)


def typed_stop_points(oracle, llr, frozen, iter_max, dtype):
    """stop_points in `dtype`: (round trips run [B], converged [B], decisions [B][N])"""
    B, N = np.asarray(llr).shape
    t_stop = np.full(B, iter_max, dtype=np.int64)
    conv = np.zeros(B, dtype=bool)
    out = np.zeros((B, N), dtype=np.int32)
    for t, (u_hat, x_hat) in enumerate(typed_bp_rounds(oracle, llr, frozen, iter_max, dtype), start=1):
        hold = ~conv & np.all(BM.encode(u_hat) == x_hat, axis=1)
        t_stop[hold] = t
        out[hold] = u_hat[hold]
        conv |= hold
        if t == iter_max:
            out[~conv] = u_hat[~conv]
    return t_stop, conv, out


def typed_bpl(oracle, llr, frozen, info_order, graphs, iter_max, taps, dtype):
    """bpl_model.bpl_decode (rules 1-6 of the header) with the attempts run in `dtype`: (bits, iters, flags, graph, total)"""
    llr = np.asarray(llr)
    B, N = llr.shape
    frozen = np.asarray(frozen)
    P = len(graphs)
    bits = np.zeros((B, N), dtype=np.int32)
    iters, flags, total = (np.zeros(B, dtype=np.int64) for _ in range(3))
    graph = np.full(B, P, dtype=np.int64)
    open_ = np.arange(B)
    for p, pi in enumerate(graphs):
        if open_.size == 0:
            break
        s = BM.sigma(pi, N)
        t, conv, u_perm = typed_stop_points(oracle, llr[open_][:, s], frozen[s], iter_max, dtype)
        u_hat = np.zeros_like(u_perm)
        u_hat[:, s] = u_perm
        crcok = BM.crc_remainder_is_zero(u_hat, info_order, taps) if taps else np.ones(open_.size, dtype=bool)
        acc = conv & crcok
        fl = np.where(conv, FLAG_BP_CONVERGED, 0) | (np.where(crcok, FLAG_CRC_PASS, 0) if taps else 0)
        total[open_] += t
        put = np.ones(open_.size, dtype=bool) if p == 0 else acc
        bits[open_[put]], iters[open_[put]], flags[open_[put]] = u_hat[put], t[put], fl[put]
        graph[open_[acc]] = p
        open_ = open_[~acc]
    return bits, iters, flags, graph, total


def typed_readout(oracle, code, llr, u, iters, checkpoints, dtype):
    """oracle.bp_readout in either type: (u_hat [B][N], E [len(checkpoints)][n+1] summed over the rows)"""
    if dtype == np.float64:
        return oracle.bp_readout(code, llr, u, iters, checkpoints)
    fn = oracle.lib().po_bpr_decode_f32
    ip = C.POINTER(C.c_int)
    fn.argtypes = [C.POINTER(oracle._Code), C.POINTER(C.c_float), C.c_int, ip, C.c_int, ip, C.POINTER(C.c_long), ip]
    llr = np.ascontiguousarray(llr, dtype=np.float32).reshape(-1, code.N)
    u = np.ascontiguousarray(u, dtype=np.int32).reshape(-1, code.N)
    cp = np.asarray(checkpoints, dtype=np.int32)
    E = np.zeros((len(cp), code.n + 1), dtype=np.int64)
    uh = np.zeros_like(u)
    for b in range(len(llr)):
        rc = fn(code._h, llr[b].ctypes.data_as(C.POINTER(C.c_float)), iters, cp.ctypes.data_as(ip), len(cp),
                u[b].ctypes.data_as(ip), E.ctypes.data_as(C.POINTER(C.c_long)), uh[b].ctypes.data_as(ip))
        assert rc == 0
    return uh, E


def bpl_graphs(case):
    g = case.ctx["kw"]["graphs"]
    n = case.ctx["N"].bit_length() - 1
    return BM.cyclic_graphs(n, g) if isinstance(g, int) else [list(p) for p in g]


# ---- the references ---------------------------------------------------------------------------------------------------------------
def reference(case, R, rows, oracle):
    """{output name: array} of the case's decoder on working LLRs `rows` (form_rows) in arithmetic type R.  The list decoders
    of the oracle report their flags bit by bit: "tie", "crc_pass" (CA-SCL) and "rerank" (per frame, whether some leaf needs
    more than the 32-bit ranking keys: what an f64 kernel that pre-ranks on them reports as POLAR_FLAG_RERANK)."""
    dt = NP[R]
    rows = np.ascontiguousarray(rows, dtype=dt)
    io, dyn, taps, fz = code_of(case)
    kw, N, B = case.ctx["kw"], case.ctx["N"], len(rows)
    if case.ref == "sc":
        uh, _, _ = oracle.decode(oracle_code(case, oracle), rows, "SC", dtype=R)
        return dict(bits=uh, pm=np.zeros(B), flags=np.zeros(B, dtype=np.int64))
    if case.ref in ("scl", "cascl"):
        st = np.zeros((B, 2), dtype=np.int32)
        uh, pm, ties = oracle.decode(oracle_code(case, oracle), rows, case.ref.upper(), L=kw["L"], dtype=R, stats=st)
        out = dict(bits=uh, pm=np.asarray(pm, dtype=np.float64), tie=np.atleast_1d(ties) > 0, rerank=st[:, 0] > 0)
        if case.ref == "cascl":
            out["crc_pass"] = syndrome(uh, io, taps) == 0
        return out
    if case.ref == "dyn":
        uh, pm, fl = DM.dscl_model(fz, dyn, rows.astype(np.float64), kw["L"], crc=(io, taps) if taps else None, dtype=dt)
        return dict(bits=uh, pm=np.asarray(pm, dtype=np.float64), flags=np.asarray(fl).astype(np.int64))
    if case.ref == "list":
        paths, pm, rem, count, fl = LM.list_model(fz, dyn, rows, kw["L"], crc=(io, taps) if taps else None, dtype=dt, oracle=oracle)
        return dict(paths=paths, pm=pm, rem=rem.astype(np.int64), count=count.astype(np.int64), flags=fl.astype(np.int64))
    if case.ref == "bp":
        it = kw["iterMax"]
        if kw["early_stop"] is None:
            uh, _, _ = oracle.decode(oracle_code(case, oracle), rows, "BP", bp_iters=it, dtype=R)
            return dict(bits=uh, iters=np.full(B, it, dtype=np.int64), flags=np.zeros(B, dtype=np.int64))
        t, conv, uh = stop_points(rows, fz, it) if R == "f64" else typed_stop_points(oracle, rows, fz, it, dt)
        return dict(bits=uh, iters=t, flags=np.where(conv, FLAG_BP_CONVERGED, 0).astype(np.int64))
    if case.ref == "readout":
        uh, E = typed_readout(oracle, oracle_code(case, oracle), rows, sent_bits(case), kw["iterMax"], case.opts["checkpoints"], dt)
        return dict(bits=uh, E=E)
    if case.ref == "scf":
        u, fl, at, flips, fail = scf_model(oracle_code(case, oracle), rows, kw["T"], dtype=dt, oracle=oracle)
        out = dict(bits=u, flags=fl, attempts=at)
        if case.entry == "polar_scf_decode_sets_device":   # a static context reports the flipped position of a passing attempt
            sets = np.full((B, 3), -1, dtype=np.int64)
            for k, f in enumerate(fail):
                if fl[f] & FLAG_CRC_PASS:
                    sets[f, 0] = flips[k][at[f] - 1]
            out["sets"] = sets
        return out
    if case.ref == "dscf":
        res = dscf_model(oracle_code(case, oracle), rows, kw["budgets"], kw["c"], kw["tau"], dtype=dt, oracle=oracle)
        return dict(bits=res.u, flags=res.flags, attempts=res.attempts, sets=res.sets)
    if case.ref == "scan":
        u, lu, ex = scan_model(fz, rows, kw["iters"], dtype=dt, oracle=oracle, skip=True)
        return dict(bits=u, llr_u=lu, ext_x=ex)
    if case.ref == "genie":
        err, tie, _, _ = MC.genie_model(oracle, rows, dt)
        return dict(counts=np.stack([err, tie]).astype(np.int64))
    if case.ref == "adaptive":
        u, pm, fl, ls = AD._oracle_composition(oracle, oracle_code(case, oracle), taps, kw["stages"], rows, dtype=R)
        return dict(bits=u, pm=np.asarray(pm, dtype=np.float64), flags=np.asarray(fl).astype(np.int64), list=ls)
    if case.ref == "bpl":
        if R == "f64":
            res = BM.bpl_decode(rows, fz, io, bpl_graphs(case), kw["iterMax"], taps)
            got = (res.bits, res.iters, res.flags, res.graph, res.total)
        else:
            got = typed_bpl(oracle, rows, fz, io, bpl_graphs(case), kw["iterMax"], taps, dt)
        return dict(zip(("bits", "iters", "flags", "graph", "total"), got))
    raise ValueError(case.ref)


LIST_REFS = ("scl", "cascl")   # the cases whose reference is the oracle's list decoder: path metrics, bit-wise flags
