"""Numpy model of BP list decoding over permuted factor graphs (POLAR_ALGO_BPL, include/polar_hip.h rules 1-6).

Built on the restated BP of tests/test_bp_early_stop_host.py (stop_points: the G-matrix stop rule; encode: u F^{(x)n}).  The
model shares nothing with the library but the header's text: sigma is formed bit by bit, the CRC is a polynomial division
of w(D), w[i] = u_hat[I[i]], and an attempt is stop_points on the permuted row with the permuted frozen mask."""
import numpy as np

from test_bp_early_stop_host import encode, stop_points  # noqa: F401  (encode is re-exported for the tests)

FLAG_CRC_PASS, FLAG_BP_CONVERGED = 2, 8


def sigma(pi, N):
    """sigma_pi(j) = sum over b of ((j >> b) & 1) << pi[b], for j = 0 .. N-1"""
    j = np.arange(N, dtype=np.int64)
    out = np.zeros(N, dtype=np.int64)
    for b, t in enumerate(pi):
        out |= ((j >> b) & 1) << int(t)
    return out


def cyclic_graphs(n, P):
    return [[(b + s) % n for b in range(n)] for s in range(P)]


def crc_remainder_is_zero(u_hat, info_order, taps):
    """w(D) = sum of u_hat[I[i]] D^i; True where w(D) mod g(D) == 0 (long division over GF(2), one row at a time)"""
    r = max(taps)
    w = np.array(np.asarray(u_hat)[..., np.asarray(info_order)], dtype=np.int64, copy=True).reshape(-1, len(info_order))
    for d in range(w.shape[1] - 1, r - 1, -1):
        hit = w[:, d] == 1
        for t in taps:
            w[hit, d - r + t] ^= 1
    return ~w[:, :r].any(axis=1)


class Result:
    """bits [B][N], iters, graph, flags, total [B]; attempts: per graph p a dict with the frames it ran (`frames`, indices),
    their rows `row`, masks `frozen`, decisions in the attempt's order `u_perm`, un-permuted `u_hat`, `t`, `conv`, `crcok`."""


def bpl_decode(llr, frozen, info_order, graphs, iter_max, crc_taps=None):
    llr = np.asarray(llr, dtype=np.float64)
    B, N = llr.shape
    frozen = np.asarray(frozen)
    P = len(graphs)
    res = Result()
    res.bits = np.zeros((B, N), dtype=np.int32)
    res.iters = np.zeros(B, dtype=np.int64)
    res.flags = np.zeros(B, dtype=np.int64)
    res.graph = np.full(B, P, dtype=np.int64)
    res.total = np.zeros(B, dtype=np.int64)
    res.attempts = []
    open_ = np.arange(B)
    for p, pi in enumerate(graphs):
        if open_.size == 0:
            break
        s = sigma(pi, N)
        row = llr[open_][:, s]                       # rule 1: row_p[j] = l[sigma_p(j)]
        fz = frozen[s]                               #         fz_p[j] = fz[sigma_p(j)]
        t, conv, u_perm = stop_points(row, fz, iter_max)
        u_hat = np.zeros_like(u_perm)
        u_hat[:, s] = u_perm                         #         u_hat_p[sigma_p(j)] = u'_p[j]
        crcok = crc_remainder_is_zero(u_hat, info_order, crc_taps) if crc_taps else np.ones(open_.size, dtype=bool)
        acc = conv & crcok                           # rule 4
        fl = np.where(conv, FLAG_BP_CONVERGED, 0) | (np.where(crcok, FLAG_CRC_PASS, 0) if crc_taps else 0)
        res.attempts.append(dict(frames=open_.copy(), row=row, frozen=fz, u_perm=u_perm, u_hat=u_hat, t=t, conv=conv,
                                 crcok=crcok))
        res.total[open_] += t                        # rule 6
        put = np.ones(open_.size, dtype=bool) if p == 0 else acc   # rule 5: attempt 0 is the fallback
        res.bits[open_[put]] = u_hat[put]
        res.iters[open_[put]] = t[put]
        res.flags[open_[put]] = fl[put]
        res.graph[open_[acc]] = p
        open_ = open_[~acc]
    return res


def classes(res, P):
    """(decided by graph 0, by a graph >= 1, by none)"""
    return int((res.graph == 0).sum()), int(((res.graph >= 1) & (res.graph < P)).sum()), int((res.graph == P).sum())
