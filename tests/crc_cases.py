"""The cases that hold every kernel that forms or checks a CRC to its model for r = 1 .. 32 (a plain helper module, imported by
tests/test_crc_cases_host.py and tests/test_gpu_crc_cases.py; it touches no GPU).

The list decoders read a path's CRC remainder as XOR over {j : u_j = 1} of crc_tab[j], crc_tab[I[i]] = D^i mod g(D).  For
i < r that entry is exactly 1 << i, so a code word u with the bit at I[i] inverted (u') has the remainder 1 << i: one bit.
Frame i of a case, i = 0 .. r-1, is built on that (single_bit_frames):

  plain row   +2.0 / -2.0 by x' = u' F^{(x)n}: the noise-free word of u'.  SC returns u', which fails the CRC in bit i alone.
  weak row    the plain row with magnitude 0.25 wherever x = u F^{(x)n} and x' differ: u' stays the best path of plain SCL,
              u is a close second, and CA-SCL has to see remainder bit i to prefer u (or to clear POLAR_FLAG_CRC_PASS where
              u fell out of the list).

Both rows are exact in float32; with sigma = 0.5 the y form is y = llr / 8, also exact.  A kernel that is blind to remainder
bit i returns u' on frame i where the reference returns u, or sets POLAR_FLAG_CRC_PASS where the reference clears it.
tests/test_crc_cases_host.py asserts on the CPU that the references behave as this text says.

A case has B = r frames.  The tables below name, per kernel, the shapes and the polynomials; every reference is the oracle's
or the numpy model the repository already has for that decoder, computed once per process (once())."""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_encode_host as E  # noqa: E402
from test_cascl_adaptive_host import syndrome  # noqa: E402

FLAG_TIE, FLAG_CRC_PASS, FLAG_RERANK = 1, 2, 4
SIGMA = 0.5                      # y = llr * SIGMA^2 / 2 = llr / 8
HI, LO = 2.0, 0.25               # the two magnitudes of a row
Q8_HI, Q8_LO = 16, 2             # the same rows as int8, handed to k_scl_q8 directly
SEED = 1

# the polynomial family, by r: taps as in polar_cfg (exponents of g(D), 0 and r included)
POLYS = {
    1: (0, 1),                                                        # D + 1
    6: (0, 5, 6),                                                     # CRC-6 of CASCL_128.c
    11: (0, 5, 9, 10, 11),                                            # CRC-11 of 5G NR
    16: (0, 5, 12, 16),                                               # CRC-16: D^16 + D^12 + D^5 + 1
    24: (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24),              # CRC-24C
    25: (0, 3, 25),                                                   # D^25 + D^3 + 1
    31: (0, 3, 31),                                                   # D^31 + D^3 + 1
    32: (0, 1, 2, 4, 5, 7, 8, 10, 11, 12, 16, 22, 23, 26, 32),        # CRC-32
}
ALL_R = tuple(POLYS)
# rows of the pair kernel's mask loop, rows = (crc_r + 3) & ~3, per polynomial
FAST2_ROWS = {1: 4, 6: 8, 11: 12, 16: 16, 24: 24, 25: 28, 31: 32, 32: 32}

_memo = {}


def once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _oracle():
    from oracle import oracle_py
    return oracle_py


def fits(N, K, rs=ALL_R):
    return tuple(r for r in rs if K + r <= N)


def code_of(N, K, r):
    """the oracle's code on the library's information set: the 5G order up to N = 1024, the library's own order above"""
    def make():
        O = _oracle()
        return O.Code(N, K, POLYS[r], Q=None if N <= 1024 else [int(j) for j in E.default_order(N)])
    return once(("code", N, K, r), make)


def sc_code_of(code):
    """SC over I[0 .. K+r): the CRC positions as information bits, the same frozen set"""
    io = code.info_order.tolist()
    s = set(io)
    return _oracle().Code(code.N, code.A, None, Q=[j for j in range(code.N) if j not in s] + io)


def rows_of(x, xf):
    """(plain, weak) float64 rows of code words x (sent) and xf (with the flipped bit)"""
    plain = HI * (1.0 - 2.0 * np.asarray(xf, dtype=np.float64))
    weak = np.where(np.asarray(x) != np.asarray(xf), plain * (LO / HI), plain)
    return plain, weak


def single_bit_frames(code):
    """(u, u_flipped, plain, weak), r frames each: u from the oracle's transmit chain (CRC attached), u_flipped = u with the
    bit at I[i] inverted in frame i, and the two rows of the module text"""
    def make():
        O = _oracle()
        r = code.r
        u, _ = O.Sim(SEED).frames(code, SIGMA, r)
        uf = u.copy()
        uf[np.arange(r), code.info_order[:r]] ^= 1
        plain, weak = rows_of(E.transform(u), E.transform(uf))
        return u, uf, plain, weak
    return once(("frames", code.N, code.K, code.r), make)


def frames(N, K, r):
    return single_bit_frames(code_of(N, K, r))


def y_of(llr):
    return np.asarray(llr) * (SIGMA * SIGMA / 2.0)


def q8_of(llr):
    """the int8 form of a row: +-16 / +-2"""
    return (np.asarray(llr) * (Q8_HI / HI)).astype(np.int8)


def np_dtype(dtype):
    return np.float32 if dtype == "f32" else np.float64


# ---- references -------------------------------------------------------------------------------------------------------------
def ref_list(N, K, r, L, dtype="f64", algo="CASCL", rows="weak"):
    """the oracle's list decoder on a case's rows: (u_hat, pm, flags without RERANK, rerank bool [B])"""
    def make():
        O = _oracle()
        code = code_of(N, K, r)
        x = frames(N, K, r)[3 if rows == "weak" else 2]
        st = np.zeros((len(x), 2), dtype=np.int32)
        uh, pm, ties = O.decode(code, x, algo, L=L, dtype=dtype, stats=st)
        ok = syndrome(uh, code.info_order, code.taps) == 0
        fl = np.where(np.atleast_1d(ties) > 0, FLAG_TIE, 0)
        if algo == "CASCL":
            fl = fl | np.where(ok, FLAG_CRC_PASS, 0)
        return uh, np.atleast_1d(pm), fl.astype(np.int64), st[:, 0] > 0
    return once(("list", N, K, r, L, dtype, algo, rows), make)


def ref_sc(N, K, r, dtype="f64"):
    """the oracle's SC over I[0 .. K+r) on the plain rows"""
    def make():
        code = code_of(N, K, r)
        return _oracle().decode(sc_code_of(code), frames(N, K, r)[2], "SC", dtype=dtype)[0]
    return once(("sc", N, K, r, dtype), make)


def ref_adaptive(N, K, r, stages, dtype="f64"):
    """_oracle_composition on the plain rows: (u_hat, pm, flags, list size)"""
    def make():
        from test_gpu_cascl_adaptive import _oracle_composition
        code = code_of(N, K, r)
        x = frames(N, K, r)[2]
        return _oracle_composition(_oracle(), code, code.taps, stages, x.astype(np_dtype(dtype)), dtype)
    return once(("adaptive", N, K, r, stages, dtype), make)


def ref_scf(N, K, r, T, dtype="f64"):
    def make():
        from test_scf_host import scf_model
        code = code_of(N, K, r)
        return scf_model(code, frames(N, K, r)[2].astype(np_dtype(dtype)), T, dtype=np_dtype(dtype), oracle=_oracle())
    return once(("scf", N, K, r, T, dtype), make)


def ref_dscf(N, K, r, budgets):
    def make():
        from dscf_model import dscf_model
        code = code_of(N, K, r)
        return dscf_model(code, frames(N, K, r)[2], budgets, SCF_C, SCF_TAU, oracle=_oracle())
    return once(("dscf", N, K, r, budgets), make)


def ref_q8(N, K, r, L):
    """q8_model on the int8 weak rows: (u_hat, pm int32, flags uint32)"""
    def make():
        import q8_model
        code = code_of(N, K, r)
        q = q8_of(frames(N, K, r)[3])
        out = [q8_model.decode(row, code.frozen, L, crc=(code.info_order, code.taps)) for row in q]
        return (np.stack([o[0] for o in out]), np.asarray([o[1] for o in out], dtype=np.int32),
                np.asarray([o[2] for o in out], dtype=np.uint32))
    return once(("q8", N, K, r, L), make)


def ref_all_paths(N, K, r, L, dtype="f64"):
    """list_model on the weak rows: (paths, pm, rem, count, flags)"""
    def make():
        import list_model
        code = code_of(N, K, r)
        return list_model.list_model(code.frozen, None, frames(N, K, r)[3], L, crc=(code.info_order, code.taps),
                                     dtype=np_dtype(dtype), oracle=_oracle())
    return once(("paths", N, K, r, L, dtype), make)


def ref_bpl(N, K, r, iter_max, P):
    def make():
        import bpl_model
        code = code_of(N, K, r)
        n = N.bit_length() - 1
        return bpl_model.bpl_decode(frames(N, K, r)[2], code.frozen, code.info_order, bpl_model.cyclic_graphs(n, P), iter_max,
                                    crc_taps=code.taps)
    return once(("bpl", N, K, r, iter_max, P), make)


# ---- the dynamic code: 5G PC-CA-SCL ----------------------------------------------------------------------------------------
DYN_N, DYN_K, DYN_L, DYN_NPC = 128, 33, 8, 3
DYN_RS = (11, 24, 32)


def dyn_code(r):
    """(info_order, (pos, sets), frozen incl. the PC positions) of PCCASCL(128, 33, n_pc = 3) with polynomial r"""
    def make():
        import polardecoding_amd as pa
        q = pa.q_sequence(DYN_N)
        pos, sets, io = pa.dyn_pc5g(DYN_N, q[DYN_N - (DYN_K + r + DYN_NPC):], DYN_NPC, 0)
        frozen = np.ones(DYN_N, dtype=np.uint8)
        frozen[io] = 0
        return np.asarray(io, dtype=np.int32), (pos, sets), frozen
    return once(("dyn code", r), make)


def dyn_frames(r):
    """single_bit_frames for the dynamic code: the parity-check bits are filled again after the flip, so both u and
    u_flipped are words of the code without its CRC"""
    def make():
        import test_dyn_host as D
        io, dyn, _ = dyn_code(r)
        v = np.random.default_rng([SEED, r]).integers(0, 2, (r, DYN_K)).astype(np.uint8)
        u = np.zeros((r, DYN_N), dtype=np.int64)
        u[:, io] = E.crc_word(v, POLYS[r])
        uf = u.copy()
        uf[np.arange(r), io[:r]] ^= 1
        u, uf = D.fill_dynamic(u, dyn), D.fill_dynamic(uf, dyn)
        plain, weak = rows_of(E.transform(u), E.transform(uf))
        return u.astype(np.int32), uf.astype(np.int32), plain, weak
    return once(("dyn frames", r), make)


def ref_dyn(r, dtype="f64", crc=True):
    """dscl_model on the weak rows (crc=False: the plain list decoder over the same constraints)"""
    def make():
        import test_dyn_host as D
        io, dyn, frozen = dyn_code(r)
        return D.dscl_model(frozen, dyn, dyn_frames(r)[3], DYN_L, crc=(io, POLYS[r]) if crc else None, dtype=np_dtype(dtype),
                            sc=False, oracle=_oracle())
    return once(("dyn", r, dtype, crc), make)


# ---- the case tables --------------------------------------------------------------------------------------------------------
# decode_device on weak rows against ref_list.  variant: a name of polardecoding_amd.testing (KERNEL_*), None: the default
# choice; kernel: what dec.kernel_name must contain; forms: "llr", "y" (y = llr / 8 with sigma = 0.5)
ListCase = namedtuple("ListCase", "label N K L rs dtypes variant kernel forms")
R_EDGE = (1, 25, 32)
R_BIG = (6, 25, 32)
LIST_CASES = [
    ListCase("fast2", 1024, 480, 8, ALL_R, ("f64", "f32"), None, "k_scl_fast2<", ("llr", "y")),
    ListCase("fast-n128", 128, 33, 8, ALL_R, ("f64",), None, "k_scl_fast<", ("llr",)),
    ListCase("fast-n1024", 1024, 480, 8, R_EDGE, ("f64",), "KERNEL_ONE_PER_WAVE", "k_scl_fast<", ("llr",)),
    ListCase("fast4", 1024, 480, 8, R_EDGE, ("f64",), "KERNEL_FOUR_PER_WAVE", "k_scl_fast4<", ("llr",)),
    ListCase("big-n512-l2", 512, 200, 2, R_BIG, ("f64", "f32"), "KERNEL_BIG", "k_scl_big<", ("llr",)),
    ListCase("big-n512-l32", 512, 200, 32, R_BIG, ("f64", "f32"), "KERNEL_BIG", "k_scl_big<", ("llr",)),
    ListCase("big-n1024-l32", 1024, 480, 32, R_BIG, ("f64", "f32"), None, "k_scl_big<", ("llr",)),
    ListCase("generic-n64", 64, 20, 8, ALL_R, ("f64",), "KERNEL_GENERIC", "k_scl_generic<", ("llr",)),
    ListCase("generic-spill-n64", 64, 20, 8, ALL_R, ("f64",), "KERNEL_GENERIC_SPILL", "k_scl_generic<", ("llr",)),
    ListCase("generic-n32-l2", 32, 15, 2, (1, 6, 11), ("f64",), "KERNEL_GENERIC", "k_scl_generic<", ("llr",)),
    ListCase("wide-n64-l64", 64, 20, 64, (6, 32), ("f64",), None, "k_scl_wide<", ("llr",)),
]


def list_case_ids():
    """[(case, r, dtype)] over the table, every polynomial that fits the shape"""
    return [(c, r, dt) for c in LIST_CASES for r in fits(c.N, c.K, c.rs) for dt in c.dtypes]


# the shapes (N, K, L) whose weak rows feed some list decoder, with the polynomials each is run with: the host conditions
# cover all of them
Q8_SHAPES = ((64, 20, 8), (128, 33, 8))
Q8_RS = (6, 24, 32)
PATHS_SHAPES = ((64, 20, 8), (128, 33, 8))         # polar_list_decode / polar_list_select, every polynomial
BOOK_MEMBERS = ((64, 20, 8, 11), (128, 33, 8, 32))  # N, K, L, r of the two-member code book


def weak_shapes():
    """{(N, K, L): set of r}"""
    out = {}
    for c in LIST_CASES:
        out.setdefault((c.N, c.K, c.L), set()).update(fits(c.N, c.K, c.rs))
    for N, K, L in Q8_SHAPES:
        out.setdefault((N, K, L), set()).update(Q8_RS)
    for N, K, L in PATHS_SHAPES:
        out.setdefault((N, K, L), set()).update(fits(N, K))
    for N, K, L, r in BOOK_MEMBERS:
        out.setdefault((N, K, L), set()).add(r)
    return out


# kernels whose first pass is SC, on plain rows
SCF_N, SCF_K, SCF_T, SCF_BUDGETS = 128, 33, 4, (2, 2)
SCF_C, SCF_TAU = 0.0, 5.0                            # the dynamic rule without its penalty term
SCF_RS = (6, 16, 32)
# adaptive CA-SCL: N, K, stages, polynomials.  N = 4096: a lane of k_ad_crc_check takes two words
ADAPTIVE_CASES = [(128, 33, (1, 8), ALL_R), (1024, 480, (1, 8), ALL_R), (4096, 2048, (1, 2), (24, 32))]
BPL_CASE = (128, 33, 32, 20, 4)                     # N, K, r, iterMax, graphs


def plain_shapes():
    """{(N, K): set of r} of the cases that rely on SC returning u_flipped on the plain row"""
    out = {(SCF_N, SCF_K): set(SCF_RS)}
    for N, K, _, rs in ADAPTIVE_CASES:
        out.setdefault((N, K), set()).update(fits(N, K, rs))
    return out


# ---- the encoder side ------------------------------------------------------------------------------------------------------
ENC_BS = (1, 65)


def enc_shapes(r):
    """(N, K) of the encoder cases of polynomial r: K = 1, A = N, K < r or K >= r, K a multiple of 32 with a CRC, and the sizes
    with one word, several words and two words per lane"""
    out = [(32, 1)] if r < 32 else []
    if r < 32:
        out.append((32, 32 - r))
    out += [(64, 20), (128, 32), (128, 33), (128, 64), (1024, 480), (1024, 512)]
    if r in (24, 32):
        out.append((4096, 2048))
    return [(N, K) for N, K in dict.fromkeys(out) if K >= 1 and K + r <= N]


def enc_cases():
    """[(r, N, K, crc_systematic)]"""
    return [(r, N, K, s) for r in ALL_R for N, K in enc_shapes(r) for s in (False, True)]


def enc_info(N, A):
    return np.asarray(E.default_order(N)[N - A:], dtype=np.int32)


def long_division(w, taps):
    """bit-serial long division of one row w (coefficient of D^i at i) by g(D), most significant coefficient first, with
    python integers: (quotient bits [A - r], remainder bits [r])"""
    r = max(taps)
    g = sum(1 << t for t in taps)
    val = sum(int(b) << i for i, b in enumerate(w))
    A = len(w)
    quo = 0
    for i in range(A - 1, r - 1, -1):
        if (val >> i) & 1:
            val ^= g << (i - r)
            quo |= 1 << (i - r)
    return [(quo >> i) & 1 for i in range(A - r)], [(val >> i) & 1 for i in range(r)]
