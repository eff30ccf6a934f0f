"""Fixed-point min-sum SC / SCL / CA-SCL (dtype POLAR_Q8) as include/polar_hip.h defines it, rules 1-6, in plain numpy and
Python integers, one frame at a time (a helper module: tests/test_q8_host.py checks it against an exhaustive search,
tests/test_gpu_q8.py holds the library to it with ==).  Nothing here is written from the kernel: the list is kept in rank
order, the candidates are sorted with sorted() on the triple (PM_c, b, r), and L may be any positive integer."""
import numpy as np

FLAG_TIE, FLAG_CRC_PASS = 1, 2


def clamp_of(q):
    """C = 2^(q-1) - 1"""
    return (1 << (int(q) - 1)) - 1


def quantize(v, scale=2.0, qc=8, sigma=0.0):
    """rule 1: float values (any shape) -> int8"""
    v = np.asarray(v)
    if v.dtype != np.float64:
        v = v.astype(np.float64)          # a float input is converted to double first
    if sigma > 0:
        v = 2 * v / sigma / sigma         # in that order
    with np.errstate(over="ignore", invalid="ignore"):
        t = v * np.float64(scale)         # one rounding
        q = np.clip(np.rint(t), -clamp_of(qc), clamp_of(qc))   # rint: ties to even
    return np.where(np.isnan(t), 0.0, q).astype(np.int8)


def crc_table(N, info_order, taps):
    """crc_tab[I[i]] = D^i mod g(D) (bit t = coefficient of D^t); 0 at frozen positions"""
    r = max(taps)
    glow = sum(1 << t for t in taps if t < r)
    tab = [0] * N
    rem = 1
    for j in info_order:
        tab[int(j)] = rem
        rem <<= 1
        if rem >> r & 1:
            rem = (rem ^ (1 << r)) ^ glow
    return tab


def f(a, b):
    """rule 2 on integer arrays"""
    s = np.where((a < 0) != (b < 0), -1, 1)
    return s * np.minimum(np.abs(a), np.abs(b))


def g(a, b, u, Ci):
    return np.clip(b + np.where(u != 0, -a, a), -Ci, Ci)


def decode(q_row, frozen, L, crc=None, qc=8, qi=8, sc=False):
    """rules 2-6 on one int8 row.  frozen [N] (1 = frozen); crc = (info_order, taps) or None; sc: POLAR_ALGO_SC.
    Returns (u_hat [N] int32, PM int, flags int).
    The list is held in rank order: row r of every array below belongs to the path of rank r.  alpha[t] [m][2^t] are the LLR
    levels, beta[t] [m][2^t] the partial sums returned by the left child at level t, u [m][N] the bits, pm [m] the metrics."""
    frozen = np.asarray(frozen)
    N = frozen.size
    n = N.bit_length() - 1
    Cc, Ci = clamp_of(qc), clamp_of(qi)
    ch = np.clip(np.asarray(q_row, dtype=np.int64), -Cc, Cc)      # clamped on load: -128 becomes -Cc
    tab = crc_table(N, *crc) if crc is not None else None
    alpha = [None] * n + [ch[None, :]]
    beta = [None] * (n + 1)
    u = np.zeros((1, N), dtype=np.int64)
    pm = np.zeros(1, dtype=np.int64)
    flags = 0
    for j in range(N):
        # lambda of leaf j: g at the level where j turns right, f below it (SC's schedule)
        if j == 0:
            top = n
        else:
            d = (j & -j).bit_length() - 1
            h = 1 << d
            alpha[d] = g(alpha[d + 1][:, :h], alpha[d + 1][:, h:], beta[d], Ci)
            top = d
        for t in range(top - 1, -1, -1):
            h = 1 << t
            alpha[t] = f(alpha[t + 1][:, :h], alpha[t + 1][:, h:])
        lam = alpha[0][:, 0]
        if sc:
            bits = np.zeros(1, dtype=np.int64) if frozen[j] else (lam < 0).astype(np.int64)
        elif frozen[j]:                               # rule 4
            pm = pm + np.where(lam < 0, -lam, 0)
            bits = np.zeros(pm.size, dtype=np.int64)
        else:                                         # rule 5
            cand = []
            for r in range(pm.size):
                l = int(lam[r])
                for b in (0, 1):
                    cand.append((int(pm[r]) + (abs(l) if b != int(l < 0) else 0), b, r))
            cand.sort()
            if len(cand) > L and cand[L - 1][0] == cand[L][0]:
                flags |= FLAG_TIE
            keep = cand[:L]
            par = np.asarray([r for _, _, r in keep])
            alpha = [a[par] if a is not None else None for a in alpha]
            beta = [a[par] if a is not None else None for a in beta]
            u = u[par]
            pm = np.asarray([c for c, _, _ in keep], dtype=np.int64)
            bits = np.asarray([b for _, b, _ in keep], dtype=np.int64)
        u[:, j] = bits
        cur = bits[:, None]                           # partial sums after leaf j
        t = 0
        while t < n and (j >> t) & 1:
            cur = np.concatenate([beta[t] ^ cur, cur], axis=1)
            t += 1
        if t < n:
            beta[t] = cur
    if sc:
        return u[0].astype(np.int32), 0, 0
    order = list(range(pm.size))                      # rule 6: smallest (PM, r)
    if tab is not None:
        def rem(r):
            x = 0
            for j in np.flatnonzero(u[r]):
                x ^= tab[int(j)]
            return x
        ok = [r for r in order if rem(r) == 0]
        if ok:
            order = ok
            flags |= FLAG_CRC_PASS
    best = min(order, key=lambda r: (int(pm[r]), r))
    return u[best].astype(np.int32), int(pm[best]), flags


def decode_rows(q_rows, frozen, L, **kw):
    """decode() over [B][N] rows -> (u_hat [B][N] int32, pm [B] int32, flags [B] uint32)"""
    q_rows = np.asarray(q_rows).reshape(-1, np.asarray(frozen).size)
    out = [decode(r, frozen, L, **kw) for r in q_rows]
    return (np.stack([o[0] for o in out]), np.asarray([o[1] for o in out], dtype=np.int32),
            np.asarray([o[2] for o in out], dtype=np.uint32))


def forced_metric(q_row, frozen, bits, qc=8, qi=8):
    """PM of the word `bits` [N] (0 at frozen positions) by an SC walk with every bit given: rules 2 and 4, an information
    leaf paying |lambda| when its given bit is not [lambda < 0].  Independent of decode(): plain recursion over the tree.
    Returns (PM, [PM right after each information leaf])."""
    frozen = np.asarray(frozen)
    Cc, Ci = clamp_of(qc), clamp_of(qi)
    ch = np.clip(np.asarray(q_row, dtype=np.int64), -Cc, Cc)
    pm = 0
    at_info = []

    def walk(alpha, lo):
        nonlocal pm
        if alpha.size == 1:
            l, b = int(alpha[0]), int(bits[lo])
            assert not (frozen[lo] and b)
            if b != int(l < 0):
                pm += abs(l)
            if not frozen[lo]:
                at_info.append(pm)
            return np.array([b], dtype=np.int64)
        h = alpha.size // 2
        left = walk(f(alpha[:h], alpha[h:]), lo)
        right = walk(g(alpha[:h], alpha[h:], left, Ci), lo + h)
        return np.concatenate([left ^ right, right])

    walk(ch, 0)
    return pm, at_info
