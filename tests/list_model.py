"""Numpy model of the "List output" section of include/polar_hip.h, shared by tests/test_list_host.py (CPU) and
tests/test_gpu_list.py.

list_model() runs the list decoder of tests/test_dyn_host.dscl_model -- the same state (per-slot level rows behind pointer
tables, bit-packed history, CRC remainder, metric), the same leaf rules, the oracle's arithmetic -- but keeps every slot to the
end and returns the whole list by rule 3: the live slots in ascending (PM, slot), padding behind them.  test_list_host.py holds
entry k* of rule 5 to dscl_model itself and the sorted metrics to the reference's.  select(), gather() and soft() restate
rules 8, 10 and 11-13."""
import numpy as np

from test_dyn_host import FLAG_CRC_PASS, FLAG_TIE, _parity32, crc_table, dyn_masks, encode


def unpack(words, N):
    """[..., N/32] uint32 -> [..., N] int32 of 0/1"""
    w = np.asarray(words).view(np.uint32) if np.asarray(words).dtype == np.int32 else np.asarray(words, dtype=np.uint32)
    return ((w[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(*w.shape[:-1], N).astype(np.int32)


def list_model(frozen, dyn, llr, L, crc=None, dtype=np.float64, oracle=None):
    """frozen [N] (1 = frozen under the cfg, dynamic positions included), dyn = (pos, sets) or None, llr [B][N], list size L,
    crc = (info_order, taps), a ready table [N] (tab_sys of the systematic mode) or None, arithmetic dtype.
    Returns (paths [B][L][N] int32, pm [B][L] float64, rem [B][L] uint32, count [B] uint32, flags [B] uint32)."""
    if oracle is None:
        from oracle import oracle_py as oracle
    frozen = np.asarray(frozen)
    N = frozen.size
    n = N.bit_length() - 1
    NW = N // 32
    llr = np.ascontiguousarray(llr, dtype=dtype).reshape(-1, N)
    B = llr.shape[0]
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
            s0 = (cand[:, None, :] <= c0[:, :, None]).sum(-1) <= L
            s1 = (cand[:, None, :] <= c1[:, :, None]).sum(-1) <= L
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

    # rule 3: the live slots in ascending (PM, slot) -- a stable sort of the metrics, the dead slots last
    live = slot < act
    key = np.where(live[None, :], PM, np.inf)
    order = np.argsort(key[:, :act], axis=1, kind="stable")
    order = np.concatenate([order, np.broadcast_to(slot[act:], (B, L - act))], axis=1)
    pm = np.take_along_axis(key, order, axis=1).astype(np.float64)
    rem = np.where(live[None, :], np.take_along_axis(crcr, order, axis=1), 0).astype(np.uint32)
    words = np.where(live[None, :, None], np.take_along_axis(hist, order[:, :, None], axis=1), 0).astype(np.uint32)
    count = np.full(B, act, dtype=np.uint32)
    anyp = ((rem == 0) & live[None, :]).any(1) if ctab is not None else np.zeros(B, dtype=bool)
    flags = (tie.astype(np.uint32) * FLAG_TIE) | (anyp.astype(np.uint32) * FLAG_CRC_PASS)
    return unpack(words, N), pm, rem, count, flags


def kstar(rem, count, has_crc):
    """rule 5: the smallest k < count with rem[k] = 0 if the code has a CRC and such a k exists, else 0"""
    rem = np.asarray(rem)
    B, L = rem.shape
    ok = (rem == 0) & (np.arange(L)[None, :] < np.asarray(count)[:, None])
    if not has_crc:
        return np.zeros(B, dtype=np.int64)
    return np.where(ok.any(1), ok.argmax(1), 0)


def select(rem, count, masks):
    """rule 8: idx [B][M], the smallest k < count[f] with rem[f][k] == masks[m], else -1"""
    rem = np.asarray(rem).astype(np.uint32)
    masks = np.asarray(masks).astype(np.uint32)
    B, L = rem.shape
    hit = (rem[:, None, :] == masks[None, :, None]) & (np.arange(L)[None, None, :] < np.asarray(count)[:, None, None])
    return np.where(hit.any(2), hit.argmax(2), -1).astype(np.int32)


def gather(paths, idx):
    """rule 10: row f = paths[f][idx[f]], -1 -> rank 0"""
    idx = np.asarray(idx)
    return np.asarray(paths)[np.arange(len(idx)), np.where(idx < 0, 0, idx)]


def soft(paths, pm, count, rem=None, want_rem=0, domain=0, clamp=64.0):
    """rules 11-13: paths [B][L][N] of 0/1, pm [B][L], count [B] -> [B][N] float64"""
    paths = np.asarray(paths)
    pm = np.asarray(pm, dtype=np.float64)
    B, L, N = paths.shape
    out = np.empty((B, N), dtype=np.float64)
    for f in range(B):
        c = int(count[f])
        cand = np.arange(c)
        if rem is not None:
            m = np.flatnonzero(np.asarray(rem[f][:c]).astype(np.uint32) == np.uint32(want_rem))
            if m.size:
                cand = m
        bits = paths[f, cand]
        if domain == 1:
            bits = encode(bits)
        v = pm[f, cand][:, None]
        m0 = np.where(bits == 0, v, np.inf).min(0, initial=np.inf)
        m1 = np.where(bits == 1, v, np.inf).min(0, initial=np.inf)
        has0, has1 = (bits == 0).any(0), (bits == 1).any(0)
        with np.errstate(invalid="ignore"):
            d = np.minimum(np.maximum(m1 - m0, -clamp), clamp)
        out[f] = np.where(~has1, clamp, np.where(~has0, -clamp, d))
    return out
