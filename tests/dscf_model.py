"""Dynamic SC-Flip (polar_scf_set_dynamic, include/polar_hip.h) restated in numpy: rules 1-8 of the header section.

sc_run_sets() is test_scf_host.sc_run (po_sc_decode's leaf loop on the oracle's check node) with up to three inverted
leaves per row.  dscf_model() builds the level lists from the metric in the stated operation order, in `dtype`, runs every
set and resolves the attempts.  tests/test_dscf_host.py checks the model's own properties; tests/test_gpu_dscf.py holds
the library to it by ==."""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_cascl_adaptive_host import FLAG_CRC_PASS, syndrome  # noqa: E402

MAX_ORDER = 3

Result = namedtuple("Result", "u flags attempts sets lists ties")
# lists[k] (k = 0 .. omega-1, level k + 1): {frame index: [(M, q, i, set tuple), ...] in list order}, for the frames
# that reached the level; ties[k]: the frames whose level-(k + 1) list ends on a key M that the first candidate left
# out shares (the order (M, q, i) alone decided which of the two went in)


def sc_run_sets(oracle, frozen, llr, sets=None, dtype=np.float64):
    """po_sc_decode over the rows of llr [B][N] in `dtype`; the decisions at the leaves sets[b] (int [B][3], -1 padded)
    of row b inverted.  Returns (u_hat [B][N] int32, lambda [B][N]: the leaf LLR that decided each u_hat_j)."""
    llr = np.ascontiguousarray(llr, dtype=dtype)
    B, N = llr.shape
    n = N.bit_length() - 1
    sets = np.full((B, MAX_ORDER), -1) if sets is None else np.asarray(sets).reshape(B, MAX_ORDER)
    alpha = np.zeros((B, 2 * N), dtype=dtype)
    alpha[:, N:] = llr   # alpha[2^t + i]: level t; level n is the channel
    bl = np.zeros((B, N), dtype=np.uint8)
    u = np.zeros((B, N), dtype=np.int32)
    lam = np.zeros((B, N), dtype=dtype)

    def chk(a, b):
        return oracle.math(0, a.ravel(), b.ravel(), dtype=dtype).reshape(a.shape)

    for j in range(N):
        if j == 0:
            tf = n - 1
        else:
            d = (j & -j).bit_length() - 1
            h = 1 << d
            src = alpha[:, 2 * h:4 * h]
            alpha[:, h:2 * h] = np.where(bl[:, h:2 * h] != 0, src[:, h:] - src[:, :h], src[:, h:] + src[:, :h])
            tf = d - 1
        for t in range(tf, -1, -1):
            h = 1 << t
            src = alpha[:, 2 * h:4 * h]
            alpha[:, h:2 * h] = chk(src[:, :h], src[:, h:])
        lj = alpha[:, 1]
        lam[:, j] = lj
        bit = np.zeros(B, dtype=np.uint8) if frozen[j] else ((lj < 0) ^ (sets == j).any(axis=1)).astype(np.uint8)
        u[:, j] = bit
        cur = bit[:, None]
        t = 0
        while t < n and (j >> t) & 1:
            h = 1 << t
            cur = np.concatenate([bl[:, h:2 * h] ^ cur, cur], axis=1)
            t += 1
        if t < n:
            bl[:, 1 << t:2 << t] = cur
    return u, lam


def metric(lam, pos, E, c, tau, dtype=np.float64):
    """Rules 2 and 3 for one run: lam [N] its leaf LLRs, pos the information positions ascending, E the run's set (a tuple,
    ascending).  Returns M(E, i) for every i of pos (dtype) and the mask i > max(E)."""
    c, tau = dtype(c), dtype(tau)
    a = np.abs(np.asarray(lam, dtype=dtype)[pos])   # fabs in the arithmetic type: +0 == -0
    cnt = np.cumsum(a <= tau)                       # covers flipped leaves and i itself
    S = c * cnt.astype(dtype)
    if len(E) == 0:
        M = a + S
    else:
        F = None
        for j in E:                                  # ascending j, starting from the first term
            v = np.abs(dtype(lam[j]))
            F = v if F is None else dtype(F + v)
        M = (F + a) + S
    assert M.dtype == dtype
    return M, pos > (max(E) if len(E) else -1)


def next_list(lams, Es, pos, T, c, tau, dtype=np.float64):
    """Rules 4 and 5 for one frame: lams[q] the leaf LLRs of run(Es[q]).  The T candidates (q, i) of smallest
    (M(E_q, i), q, i): [(M, q, i, E_q + (i,)), ...]."""
    Ms, qs, js = [], [], []
    for q, (lam, E) in enumerate(zip(lams, Es)):
        M, ok = metric(lam, pos, E, c, tau, dtype)
        Ms.append(M[ok])
        js.append(pos[ok])
        qs.append(np.full(int(ok.sum()), q))
    if not Ms:
        return []
    M, q, j = np.concatenate(Ms), np.concatenate(qs), np.concatenate(js)
    order = np.lexsort((j, q, M))[:T]
    return [(M[o], int(q[o]), int(j[o]), tuple(Es[q[o]]) + (int(j[o]),)) for o in order]


def dscf_model(code, llr, budgets, c, tau, dtype=np.float64, oracle=None):
    """The decoder's output for budgets (T_1 .. T_omega), penalty c and threshold tau: Result(u_hat [B][N], flags [B],
    attempts [B], sets [B][3] ascending and -1 padded, the per-level lists)."""
    if oracle is None:
        from oracle import oracle_py as oracle
    budgets = tuple(int(t) for t in budgets)
    omega = len(budgets)
    assert 1 <= omega <= MAX_ORDER
    llr = np.ascontiguousarray(llr).reshape(-1, code.N)
    B = len(llr)
    io, taps = code.info_order, code.taps
    pos = np.sort(np.asarray(io))
    u0, lam0 = sc_run_sets(oracle, code.frozen, llr, dtype=dtype)
    ok0 = syndrome(u0, io, taps) == 0
    u = u0.copy()
    flags = np.where(ok0, FLAG_CRC_PASS, 0).astype(np.int64)
    attempts = np.where(ok0, 0, sum(budgets)).astype(np.int64)
    sets = np.full((B, MAX_ORDER), -1, dtype=np.int64)
    lists = [dict() for _ in range(omega)]
    ties = [set() for _ in range(omega)]
    # the runs whose extensions make the next level's list: per open frame the leaf LLRs and the set of each
    open_frames = [int(f) for f in np.flatnonzero(~ok0)]
    runs = {f: ([lam0[f]], [()]) for f in open_frames}
    base = 0
    for k, T in enumerate(budgets):
        if not open_frames:
            break
        rows, rsets, owner = [], [], []
        for f in open_frames:
            lst = next_list(runs[f][0], runs[f][1], pos, T + 1, c, tau, dtype)
            if len(lst) > T and lst[T - 1][0] == lst[T][0]:
                ties[k].add(f)
            lst = lst[:T]
            lists[k][f] = lst
            for r, (_, _, _, E) in enumerate(lst):
                rows.append(llr[f])
                rsets.append(list(E) + [-1] * (MAX_ORDER - len(E)))
                owner.append((f, r))
        if not rows:
            break
        ut, lamt = sc_run_sets(oracle, code.frozen, np.stack(rows), np.array(rsets), dtype=dtype)
        okt = syndrome(ut, io, taps) == 0
        still, nruns, done = [], {}, set()
        for row, (f, r) in enumerate(owner):
            if f in done:
                continue
            if okt[row]:   # rows of a frame are in list order: the first passing one has the smallest number
                done.add(f)
                u[f] = ut[row]
                flags[f] |= FLAG_CRC_PASS
                attempts[f] = base + r + 1
                sets[f] = rsets[row]
        for row, (f, r) in enumerate(owner):
            if f not in done:
                nruns.setdefault(f, ([], []))
                nruns[f][0].append(lamt[row])
                nruns[f][1].append(lists[k][f][r][3])
        still = [f for f in open_frames if f not in done]
        for f in still:
            nruns.setdefault(f, ([], []))
        open_frames, runs = still, nruns
        base += T
    return Result(u, flags, attempts, sets, lists, ties)
