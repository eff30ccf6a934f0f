"""Numpy model of the "Sent-path trace" section of include/polar_hip.h, shared by tests/test_trace_host.py (CPU) and
tests/test_gpu_trace.py.

trace_model() is the loop of tests/list_model.list_model -- the same state, the same leaf rules, the oracle's arithmetic -- with
one flag per slot: the slot's decided bits 0 .. j equal the sent ones (rule 2).  The flag moves with the path wherever the
history moves, the leaf after whose decision no live slot carries it is the loss leaf (rule 3), and at a ranking leaf the count
#{m : c_m <= c_sent} of the survivor test is kept for it (rule 4).  rank is read off the flag, not off a row comparison;
test_trace_host.py holds it to the row comparison on list_model()'s output.  count() restates rule 8."""
import numpy as np

from list_model import kstar
from test_dyn_host import FLAG_CRC_PASS, FLAG_TIE, _parity32, crc_table, dyn_masks


def pack(u):
    """[..., N] of 0/1 -> [..., N/32] uint32, bit j & 31 of word j >> 5"""
    u = np.asarray(u).astype(np.uint32)
    w = u.reshape(*u.shape[:-1], u.shape[-1] // 32, 32) << np.arange(32, dtype=np.uint32)
    return np.bitwise_or.reduce(w, axis=-1).astype(np.uint32)


def trace_model(frozen, dyn, llr, u, L, crc=None, dtype=np.float64, oracle=None):
    """frozen, dyn, llr, L, crc, dtype as list_model; u [B][N] of 0/1, the sent word.
    Returns (loss_leaf [B] int32, loss_rank [B] uint32, rank [B] int32, chosen [B] int32, flags [B] uint32)."""
    if oracle is None:
        from oracle import oracle_py as oracle
    frozen = np.asarray(frozen)
    N = frozen.size
    n = N.bit_length() - 1
    NW = N // 32
    llr = np.ascontiguousarray(llr, dtype=dtype).reshape(-1, N)
    B = llr.shape[0]
    u = np.asarray(u).reshape(B, N).astype(np.uint8)
    row, mask = dyn_masks(N, dyn)
    if crc is None:
        ctab = None
    elif isinstance(crc, tuple):
        ctab = crc_table(N, *crc)
    else:
        ctab = np.asarray(crc, dtype=np.uint64)

    def chk(a, b):
        return oracle.math(0, a.ravel(), b.ravel(), dtype=dtype).reshape(a.shape)

    def phi(lam, bit):
        return oracle.math(2, lam.ravel(), bit.astype(dtype).ravel(), dtype=dtype).reshape(lam.shape)

    slot = np.arange(L)
    alpha = np.zeros((B, L, N), dtype=dtype)
    pa = np.zeros((B, L, n + 1), dtype=np.int64)
    bl = np.zeros((B, L, N), dtype=np.uint8)
    pb = np.zeros((B, L, n + 1), dtype=np.int64)
    hist = np.zeros((B, L, NW), dtype=np.uint32)
    crcr = np.zeros((B, L), dtype=np.uint64)
    PM = np.zeros((B, L), dtype=dtype)
    tie = np.zeros(B, dtype=bool)
    act = 1
    match = np.zeros((B, L), dtype=bool)   # rule 2; before leaf 0 the one live slot has decided nothing
    match[:, 0] = True
    loss_leaf = np.full(B, N, dtype=np.int32)
    loss_rank = np.zeros(B, dtype=np.uint32)

    def level(buf, ptr, t):
        if t == n:
            return np.broadcast_to(llr[:, None, :], (B, L, N))
        return np.take_along_axis(buf[:, :, 1 << t:2 << t], ptr[:, :, t][:, :, None], axis=1)

    for j in range(N):
        if j == 0:
            tf = n - 1
        else:
            d = (j & -j).bit_length() - 1
            h = 1 << d
            src = level(alpha, pa, d + 1)
            bits = level(bl, pb, d)
            alpha[:, :, h:2 * h] = np.where(bits != 0, src[:, :, h:] - src[:, :, :h], src[:, :, h:] + src[:, :, :h])
            pa[:, :, d] = slot
            tf = d - 1
        for t in range(tf, -1, -1):
            h = 1 << t
            src = level(alpha, pa, t + 1)
            alpha[:, :, h:2 * h] = chk(np.ascontiguousarray(src[:, :, :h]), np.ascontiguousarray(src[:, :, h:]))
            pa[:, :, t] = slot
        lam = np.ascontiguousarray(alpha[:, :, 1])

        bit = np.zeros((B, L), dtype=np.uint8)
        sg = None
        sent_count = np.zeros(B, dtype=np.uint32)   # rule 4: the count of c_sent at a ranking leaf, 0 at every other leaf
        if row[j] >= 0:
            w = (j >> 5) + 1
            bit = _parity32(np.bitwise_xor.reduce(hist[:, :, :w] & mask[row[j], :w], axis=-1))
            PM = PM + phi(lam, bit)
        elif frozen[j]:
            PM = PM + phi(lam, bit)
        elif act < L:
            c0 = PM + phi(lam, np.zeros_like(bit))
            c1 = PM + phi(lam, np.ones_like(bit))
            sg = np.broadcast_to(np.where((slot >= act) & (slot < 2 * act), slot - act, slot), (B, L))
            PM = c0.copy()
            PM[:, act:2 * act] = c1[:, :act]
            bit[:, act:2 * act] = 1
            act *= 2
        else:
            c0 = PM + phi(lam, np.zeros_like(bit))
            c1 = PM + phi(lam, np.ones_like(bit))
            cand = np.concatenate([c0, c1], axis=1)
            n0 = (cand[:, None, :] <= c0[:, :, None]).sum(-1)
            n1 = (cand[:, None, :] <= c1[:, :, None]).sum(-1)
            s0, s1 = n0 <= L, n1 <= L
            m = match.argmax(1)                                       # the slot that matched after leaf j - 1, if any
            f = np.arange(B)
            sent_count = np.where(match.any(1), np.where(u[:, j] != 0, n1[f, m], n0[f, m]), 0).astype(np.uint32)
            tie |= (s0.sum(1) + s1.sum(1)) < L
            both, dead = s0 & s1, ~s0 & ~s1
            both_slots = np.argsort(~both, axis=1, kind="stable")
            rank = np.cumsum(dead, axis=1) - 1
            refill = dead & (rank < both.sum(1)[:, None])
            sg = np.where(refill, np.take_along_axis(both_slots, np.clip(rank, 0, L - 1), axis=1), slot[None, :])
            c1_s = np.take_along_axis(c1, sg, axis=1)
            bit = np.where(refill, 1, np.where(s0, 0, np.where(s1, 1, 0))).astype(np.uint8)
            PM = np.where(refill, c1_s, np.where(s0, c0, np.where(s1, c1, c0)))
        if sg is not None:
            pa = np.take_along_axis(pa, sg[:, :, None], axis=1)
            pb = np.take_along_axis(pb, sg[:, :, None], axis=1)
            hist = np.take_along_axis(hist, sg[:, :, None], axis=1)
            crcr = np.take_along_axis(crcr, sg, axis=1)
            match = np.take_along_axis(match, sg, axis=1)

        # rules 2 and 3
        match = match & (bit == u[:, j, None]) & (slot < act)[None, :]
        lost = (loss_leaf == N) & ~match.any(1)
        loss_leaf[lost] = j
        loss_rank[lost] = sent_count[lost]

        hist[:, :, j >> 5] |= bit.astype(np.uint32) << np.uint32(j & 31)
        if ctab is not None:
            crcr ^= bit.astype(np.uint64) * ctab[j]
        cur = bit[:, :, None]
        t = 0
        while t < n and (j >> t) & 1:
            cur = np.concatenate([level(bl, pb, t) ^ cur, cur], axis=-1)
            t += 1
        if t < n:
            bl[:, :, 1 << t:2 << t] = cur
            pb[:, :, t] = slot

    # rules 5 and 6 on the order of "List output" rule 3
    live = slot < act
    key = np.where(live[None, :], PM, np.inf)
    order = np.argsort(key[:, :act], axis=1, kind="stable")
    hit = np.take_along_axis(match[:, :act], order, axis=1)
    rank = np.where(hit.any(1), hit.argmax(1), -1).astype(np.int32)
    rem = np.take_along_axis(crcr[:, :act], order, axis=1)
    chosen = kstar(rem, np.full(B, act), ctab is not None).astype(np.int32)
    anyp = (rem == 0).any(1) if ctab is not None else np.zeros(B, dtype=bool)
    flags = (tie.astype(np.uint32) * FLAG_TIE) | (anyp.astype(np.uint32) * FLAG_CRC_PASS)
    return loss_leaf, loss_rank, rank, chosen, flags


def classes(rank, chosen):
    """rule 6: 0 correct, 1 selection error, 2 list loss"""
    rank, chosen = np.asarray(rank), np.asarray(chosen)
    return np.where(rank < 0, 2, np.where(rank == chosen, 0, 1))


def count(N, loss_leaf, rank, chosen, hist=None):
    """rule 8: hist [N + 4] uint64, added to"""
    out = np.zeros(N + 4, dtype=np.uint64) if hist is None else np.array(hist, dtype=np.uint64)
    ll = np.asarray(loss_leaf)
    out[:N] += np.bincount(ll[ll < N], minlength=N).astype(np.uint64)
    out[N:N + 3] += np.bincount(classes(rank, chosen), minlength=3).astype(np.uint64)
    out[N + 3] += np.uint64(ll.size)
    return out
