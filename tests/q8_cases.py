"""The cases that hold k_scl_q8 and k_q8_quantize (csrc/scl_q8.h, csrc/k_q8.hip) to tests/q8_model.py at every shape (a plain
helper module, imported by tests/test_q8_cases_host.py and tests/test_gpu_q8_cases.py).

k_scl_q8 shares no body with the other list decoders: its own int8 LDS rows of N + 4 S bytes, its lane split S = 64 / L, dword
loops stepped by 4 S, ranking by counting 32-bit keys, a run-time internal clamp Ci in every g step, and a quantiser kernel
of its own.  Five groups, each a table of contexts (Ctx) and rows; every expected output is q8_model's, computed once per
process (once()):

  A  every (N, L): N = 32 .. 1024 x L = SC, 1, 2, 4, 8, 16, 32 on the 5G set with K = N / 2 and the default quantiser; 12 rows
     (6 spread rows of test_gpu_q8._rows, 3 ternary, 3 uniform over int8 with -128 planted).  CA-SCL at L = 2 and 16 with
     CRC-6 (N = 64, 128), CRC-11 (256) and CRC-24C (512, 1024): there the 6 spread rows are a codeword of the code at
     magnitude A_SIGNAL plus the spread noise of amplitude A_CRC_AMP[(N, L)], scaled per row by A_GAINS, so that
     FLAG_CRC_PASS takes both values.
  B  frozen sets outside the 5G order (tests/frozen_patterns.py) through a seeded info_order: all 30 masks at N = 128 with
     L = 2, 8, 16, 32 on 6 rows, all 38 at N = 1024 with L = 8, 32 on 3 rows, and the 25 masks that can carry CRC-6 as CA-SCL
     with L = 8.
  C  all 28 clamp pairs 2 <= qc <= qi <= 8 at N = 128 as SCL L = 8, CA-SCL L = 8 with CRC-6, and SC, on 16 rows: 8 uniform over
     int8 with -128 planted and 8 "flipped hard" rows (a codeword at magnitude 127 with 3 % to 20 % of the signs flipped, so
     that g sums grow to Cc 2^t and meet Ci: 5 rows with the flips at random positions, 3 with 16 flips on the support of
     the rows of F^{(x)n} of the frozen leaves 15 and 23).  Three pairs also through the float entry at scales 0.5, 2.0, 3.7.
  D  the device quantiser on constructed values: t = v * scale on every half-integer and integer of -130 .. 130 and their
     neighbours, the clamp edges, huge values, infinities, NaN and signed zeros, for double and float input; and y values
     on whose half-integers 2*y/sigma/sigma*scale lands, where another operation order rounds differently.
  E  large metrics: sparse_last and sparse_first at N = 1024 on rows over {-127, +127}: metrics above 2^13.

tests/test_q8_cases_host.py asserts on the CPU what each group is there for."""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frozen_patterns as FP  # noqa: E402
import q8_model as M  # noqa: E402
import test_gpu_q8 as Q8T  # noqa: E402  (_rows, _family_rows)

CRC6 = (0, 5, 6)
CRC11 = (0, 5, 9, 10, 11)
CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)
DEFAULT_QUANT = (2.0, 8, 8)

# N, L (0: POLAR_ALGO_SC), sc, CRC taps or None, info_order int32 [A], given (the order is passed to polar_create; False: the
# library derives it from the 5G order and the test asserts that it is this one), (scale, qc, qi)
Ctx = namedtuple("Ctx", "N L sc taps order given quant")
_memo = {}


def once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def order_5g(N, A):
    """the A most reliable positions of the 5G order restricted to < N, ascending reliability: what polar_create derives"""
    return np.asarray(FP.q5g(N)[N - A:], dtype=np.int32)


def frozen_of(ctx):
    fz = np.ones(ctx.N, dtype=np.uint8)
    fz[ctx.order] = 0
    return fz


def crc_of(ctx):
    return (ctx.order, ctx.taps) if ctx.taps else None


def model(ctx, q, decode=M.decode):
    """q8_model (or a copy of it with the same signature) on int8 rows [B][N] -> (u_hat, pm int32, flags uint32)"""
    scale, qc, qi = ctx.quant
    fz, crc = frozen_of(ctx), crc_of(ctx)
    out = [decode(r, fz, max(ctx.L, 1), crc=crc, qc=qc, qi=qi, sc=ctx.sc) for r in np.asarray(q).reshape(-1, ctx.N)]
    return (np.stack([o[0] for o in out]), np.asarray([o[1] for o in out], dtype=np.int32),
            np.asarray([o[2] for o in out], dtype=np.uint32))


def want(key, ctx, q):
    return once(("want", key), lambda: model(ctx, q))


# ---- row builders -----------------------------------------------------------------------------------------------------------
def transform(u):
    """x = u F^{(x)n} over the last axis (natural order: the left half of every block is left ^ right)"""
    x = np.array(u, dtype=np.int64)
    B, N = x.shape
    h = 1
    while h < N:
        x = x.reshape(B, N // (2 * h), 2, h)
        x[:, :, 0, :] ^= x[:, :, 1, :]
        x = x.reshape(B, N)
        h *= 2
    return x


def codewords(rng, B, ctx):
    """(u [B][N], x [B][N]): random words of the code of ctx; with a CRC, the bits at I[0 .. r) make the remainder 0"""
    N, order = ctx.N, ctx.order
    r = max(ctx.taps) if ctx.taps else 0
    u = np.zeros((B, N), dtype=np.int64)
    u[:, order[r:]] = rng.integers(0, 2, size=(B, order.size - r))
    if r:
        tab = M.crc_table(N, order, ctx.taps)
        assert [tab[int(j)] for j in order[:r]] == [1 << i for i in range(r)]
        for b in range(B):
            rem = 0
            for j in np.flatnonzero(u[b]):
                rem ^= tab[int(j)]
            u[b, order[:r]] = [(rem >> i) & 1 for i in range(r)]
    return u, transform(u)


def ternary(rng, B, N):
    return Q8T._family_rows("ternary", B, N, rng)


def minus128(rng, B, N):
    """uniform over int8 with -128 at every seventh position"""
    return Q8T._family_rows("minus128", B, N, rng)


def pm127(rng, B, N):
    return Q8T._family_rows("pm127", B, N, rng)


def flip_counts(B, N, lo=0.03, hi=0.20):
    return [int(round(share * N)) for share in np.linspace(lo, hi, B)]


def flipped_hard(rng, B, ctx, bursts=()):
    """(q int8 [B + len(bursts)][N], x [..][N] the codewords): random words of ctx's code at magnitude 127.  Row b < B has a
    share of 3 % .. 20 % (evenly spaced over the rows) of its signs flipped at random positions.  Each further row takes its
    flips from one entry of `bursts`, a tuple of leaves: the signs at the support of those rows of F^{(x)n} are flipped, so
    the row is the noise-free word of u ^ e_leaves, and an SC walk forced back to u pays the whole magnitude Cc 2^popcount(leaf)
    of such a leaf at once -- 16 flips in one block of 16 for leaf 15."""
    N = ctx.N
    _, x = codewords(rng, B + len(bursts), ctx)
    q = 127 * (1 - 2 * x)
    for b, k in enumerate(flip_counts(B, N)):
        q[b, rng.permutation(N)[:k]] *= -1
    for b, leaves in enumerate(bursts, start=B):
        e = np.zeros((1, N), dtype=np.int64)
        e[0, list(leaves)] = 1
        q[b, transform(e)[0] == 1] *= -1
    return q.astype(np.int8), x


def float_rows_of(q, scale):
    """double rows whose quantisation with `scale` and qc = 8 is q with -128 clamped to -127 (which every decode does on load)"""
    return np.asarray(q, dtype=np.float64) / scale


# ---- group A: every (N, L) --------------------------------------------------------------------------------------------------
A_NS = (32, 64, 128, 256, 512, 1024)
A_LS = (0, 1, 2, 4, 8, 16, 32)
A_CRC = {64: CRC6, 128: CRC6, 256: CRC11, 512: CRC24C, 1024: CRC24C}
A_CRC_LS = (2, 16)
A_FLOAT_L = {32: 16, 64: 2, 128: 0, 256: 32, 512: 16, 1024: 4}   # the L per N that also runs through polar_decode_device
# The spread rows of a CA-SCL case: a codeword at LLR magnitude A_SIGNAL plus test_gpu_q8._rows of amplitude A_CRC_AMP[(N, L)]
# scaled per row by A_GAINS.  Row 0 is nearly clean and passes the CRC, rows 4 and 5 drown and fail it; one amplitude turned
# out to give both outcomes in all ten cases (tests/test_q8_cases_host.py::test_a_cascl holds that).
A_SIGNAL = 2.0
A_CRC_AMP = {(N, L): 24.0 for N in A_CRC for L in A_CRC_LS}
A_GAINS = (0.02, 0.1, 0.3, 1.0, 1.5, 2.0)
A_SPREAD, A_TERNARY, A_MINUS = 6, 3, 3


def a_ctx(N, L, crc=False):
    taps = A_CRC[N] if crc else None
    A = N // 2 + (max(taps) if taps else 0)
    return Ctx(N, L, L == 0, taps, order_5g(N, A), False, DEFAULT_QUANT)


def a_cases():
    """[(N, L, crc)]: 42 shapes and 10 CA-SCL cases"""
    return [(N, L, False) for N in A_NS for L in A_LS] + [(N, L, True) for N in A_CRC for L in A_CRC_LS]


def a_rows(N, L, crc=False):
    """(x float64 [12][N], q int8 [12][N]): x quantises to q up to -128 / -127.  In a CA-SCL case the spread rows carry a
    codeword: on pure noise no path ever passes a CRC of 6 bits or more often enough to show both outcomes on six rows."""
    def make():
        ctx = a_ctx(N, L, crc)
        rng = np.random.default_rng([N, L, int(crc)])
        if crc:
            _, cw = codewords(rng, A_SPREAD, ctx)
            xs = A_SIGNAL * (1 - 2 * cw) + np.asarray(A_GAINS)[:, None] * Q8T._rows(rng, A_SPREAD, N, amp=A_CRC_AMP[(N, L)])
        else:
            xs = Q8T._rows(rng, A_SPREAD, N)
        q = np.concatenate([M.quantize(xs), ternary(rng, A_TERNARY, N), minus128(rng, A_MINUS, N)])
        x = np.concatenate([xs, float_rows_of(q[A_SPREAD:], DEFAULT_QUANT[0])])
        return x, q
    return once(("a rows", N, L, crc), make)


def a_want(N, L, crc=False):
    return want(("a", N, L, crc), a_ctx(N, L, crc), a_rows(N, L, crc)[1])


# ---- group B: frozen sets outside the 5G order ------------------------------------------------------------------------------
B_LS = {128: (2, 8, 16, 32), 1024: (8, 32)}
B_ROWS = {128: (3, 3), 1024: (2, 1)}          # spread rows, ternary rows
B_CRC_L = 8
B_SEED = 3
B_AMP = 12.0


def b_masks(N):
    return list(FP.families(N))


def b_crc_masks():
    return list(FP.with_crc(FP.families(128), 128))


def b_ctx(N, name, L, crc=False):
    order = FP.order_of(FP.families(N)[name], B_SEED)
    return Ctx(N, L, False, CRC6 if crc else None, order, True, DEFAULT_QUANT)


def b_rows(N, name):
    def make():
        rng = np.random.default_rng([N, len(name), sum(name.encode())])
        ns, nt = B_ROWS[N]
        return np.concatenate([M.quantize(Q8T._rows(rng, ns, N, amp=B_AMP)), ternary(rng, nt, N)])
    return once(("b rows", N, name), make)


def b_want(N, name, L, crc=False):
    return want(("b", N, name, L, crc), b_ctx(N, name, L, crc), b_rows(N, name))


def b_never_fills(N, name, L):
    """fewer information leaves than log2 L: the list ends with act = 2^A < L"""
    return (1 << int((FP.families(N)[name] == 0).sum())) < L


# ---- group C: every clamp pair ----------------------------------------------------------------------------------------------
C_N, C_L = 128, 8
C_PAIRS = [(qc, qi) for qc in range(2, 9) for qi in range(qc, 9)]
C_KINDS = ("scl", "cascl", "sc")
C_FLOAT_PAIRS = ((2, 2), (4, 6), (8, 8))     # these also run through the float entry, at each of C_FLOAT_SCALES
C_FLOAT_SCALES = (0.5, 2.0, 3.7)
C_UNIFORM, C_FLIPPED = 8, 8
# The burst rows of the flipped block (flipped_hard).  Leaves 15 and 23 are frozen in both codes (A = 64 and A = 70) and have
# four 1-bits, the most of any frozen leaf: every path pays min(16 Cc, Ci) there at once.  Each entry flips 16 signs (12.5 %;
# rows 15 and 23 of F^{(x)7} share 8 columns).
C_BURSTS = ((15,), (23,), (15, 23))


def c_ctx(kind, qc, qi, scale=2.0):
    taps = CRC6 if kind == "cascl" else None
    A = C_N // 2 + (6 if taps else 0)
    return Ctx(C_N, 0 if kind == "sc" else C_L, kind == "sc", taps, order_5g(C_N, A), False, (scale, qc, qi))


def c_flipped(kind):
    """(q int8 [8][128], codewords [8][128]): 5 rows with random flips, 3 burst rows"""
    def make():
        return flipped_hard(np.random.default_rng([C_N, len(kind), 1]), C_FLIPPED - len(C_BURSTS), c_ctx(kind, 8, 8), C_BURSTS)
    return once(("c flipped", kind), make)


def c_rows(kind):
    """int8 [16][128]: the rows depend on the code (its codewords), not on the clamp pair"""
    def make():
        rng = np.random.default_rng([C_N, len(kind)])
        return np.concatenate([minus128(rng, C_UNIFORM, C_N), c_flipped(kind)[0]])
    return once(("c rows", kind), make)


def c_want(kind, qc, qi):
    return want(("c", kind, qc, qi), c_ctx(kind, qc, qi), c_rows(kind))


# ---- group D: the device quantiser ------------------------------------------------------------------------------------------
D_N = 32
D_BS = (9, 73)
D_SCALES = (0.5, 1.0, 2.0, 3.7)
D_QCS = tuple(range(2, 9))
D_Y = ((0.84, 2.0), (0.7, 3.7), (1.3, 1.0))   # (sigma, scale)
D_SPECIAL = (127.49, 127.5, -127.5, 128.0, 1e3, -1e3, 1e30, -1e30, 1e308, -1e308, np.inf, -np.inf, np.nan, 0.0, -0.0)


def d_targets():
    """the values t = v * scale is to land on: every integer and half-integer of -130 .. 130, then the specials"""
    return np.arange(-260, 261) / 2.0, np.asarray(D_SPECIAL)


def d_values(scale, dtype, small=False):
    """1-D array of `dtype`: targets / scale (rounded to dtype), the neighbours of the first kind on both sides in dtype,
    and the specials / scale (without 1e308 in float32, where it is an infinity).  small: the subset for B = 9 (|t| <= 2 or
    |t| >= 126, and the specials)."""
    grid, special = d_targets()
    if small:
        grid = grid[(np.abs(grid) <= 2) | (np.abs(grid) >= 126)]
    if dtype == np.float32:
        special = special[np.abs(special) != 1e308]
    with np.errstate(over="ignore"):
        g = (grid / scale).astype(dtype)
        s = (special / scale).astype(dtype)
    inf = np.asarray(np.inf, dtype=dtype)
    return np.concatenate([g, s, np.nextafter(g, inf), np.nextafter(g, -inf)])


def d_y_values(sigma, scale, dtype):
    """y0 = (k + 0.5) / scale * sigma^2 / 2 for k = -126 .. 125 and the 4 nextafter steps on either side: 2268 values"""
    y0 = ((np.arange(-126, 126) + 0.5) / scale * sigma * sigma / 2).astype(dtype)
    inf = np.asarray(np.inf, dtype=dtype)
    out, up, dn = [y0], y0, y0
    for _ in range(4):
        up, dn = np.nextafter(up, inf), np.nextafter(dn, -inf)
        out += [up, dn]
    return np.concatenate(out)


def d_pad(v, B):
    """v laid into [B][32] rows, the last one padded with zeros"""
    assert v.size <= B * D_N, (v.size, B)
    out = np.zeros(B * D_N, dtype=v.dtype)
    out[:v.size] = v
    return out.reshape(B, D_N)


def d_ctx(L=4):
    return Ctx(D_N, L, False, None, order_5g(D_N, D_N // 2), False, DEFAULT_QUANT)


# ---- group E: large metrics -------------------------------------------------------------------------------------------------
E_N = 1024
E_MASKS = ("sparse_last", "sparse_first")
E_LS = (8, 32)
E_ROWS = 6
E_FLOOR = 8192


def e_ctx(name, L):
    return b_ctx(E_N, name, L)


def e_rows(name):
    return once(("e rows", name), lambda: pm127(np.random.default_rng([E_N, len(name)]), E_ROWS, E_N))


def e_want(name, L):
    return want(("e", name, L), e_ctx(name, L), e_rows(name))
