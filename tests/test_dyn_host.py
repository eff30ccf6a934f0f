"""CPU: dynamic frozen bits (include/polar_hip.h, "Dynamic frozen bits"): PAC codes and the parity-check bits of 5G PC-polar.

dscl_model() is a numpy list decoder for the rule of the header, vectorised over frames and list slots.  Its arithmetic is
the oracle's (CHK and PHI through oracle.math, in f64 and f32); its slot assignment and tie rule are written from the comments
of csrc/scl_generic.h: phase 1 clones slot k into slot k + act, phase 2 keeps the candidates c with #{m : c_m <= c} <= L, the
m-th both-survivor (ascending slot) forks into the m-th dead slot, an un-refilled dead slot continues as its 0-branch, the
chosen path is the first slot of least metric among those that pass the CRC (among all if none does).  With no constraint,
and with constraints whose sets are all empty, it equals the oracle's SC / SCL / CA-SCL; tests/test_gpu_dyn.py holds the
library to it.  Also here: the host helpers (PAC rows against a brute-force GF(2) inverse, the 5G PC rule against a literal
restatement of the standard), the refusals of polar_create_dyn (no device needed) and the exported ABI."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

CRC6 = (0, 5, 6)
FLAG_TIE, FLAG_CRC_PASS = 1, 2
G133 = 0o133


# ---- the model ------------------------------------------------------------------------------------------------------
def crc_table(N, info_order, taps):
    """crc_tab[I[i]] = D^i mod g(D) (bit t = coefficient of D^t); 0 at frozen positions"""
    r = max(taps)
    glow = sum(1 << t for t in taps if t < r)
    tab = np.zeros(N, dtype=np.uint64)
    rem = 1
    for j in info_order:
        tab[j] = rem
        rem <<= 1
        if rem >> r & 1:
            rem = (rem ^ (1 << r)) ^ glow
    return tab


def dyn_masks(N, dyn):
    """(row [N]: constraint row of leaf j or -1, mask [D][N/32] uint32)"""
    row = np.full(N, -1, dtype=np.int64)
    pos, sets = dyn if dyn is not None else ((), ())
    mask = np.zeros((max(len(pos), 1), N // 32), dtype=np.uint32)
    for d, j in enumerate(pos):
        row[j] = d
        for i in sets[d]:
            assert 0 <= i < j
            mask[d, i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return row, mask


def _parity32(x):
    x = x ^ (x >> np.uint32(16))
    x = x ^ (x >> np.uint32(8))
    x = x ^ (x >> np.uint32(4))
    x = x ^ (x >> np.uint32(2))
    x = x ^ (x >> np.uint32(1))
    return (x & np.uint32(1)).astype(np.uint8)


def dscl_model(frozen, dyn, llr, L, crc=None, dtype=np.float64, sc=None, oracle=None, trace=None):
    """frozen [N] (1 = frozen under the cfg, dynamic positions included), dyn = (pos, sets) or None, llr [B][N], list size
    L, crc = (info_order, taps) or None, arithmetic dtype.  sc: SC decisions (no metric, no flags); default L == 1 without a
    CRC.  Returns (u_hat [B][N] int32, pm [B] float64, flags [B] uint32).
    trace: a dict that receives four bool arrays [B], each true where some phase-2 leaf of the frame had the property --
    "tie" (fewer than L candidates survive), "cross" (a refilled slot and its source slot lie in different groups of 64
    slots), "unrefilled" (a dead slot is not refilled), "all_equal" (the 2L candidates are all equal).  The results do not
    depend on it."""
    if oracle is None:
        from oracle import oracle_py as oracle
    frozen = np.asarray(frozen)
    N = frozen.size
    n = N.bit_length() - 1
    NW = N // 32
    llr = np.ascontiguousarray(llr, dtype=dtype).reshape(-1, N)
    B = llr.shape[0]
    if sc is None:
        sc = L == 1 and crc is None
    row, mask = dyn_masks(N, dyn)
    ctab = crc_table(N, *crc) if crc is not None else None

    def chk(a, b):
        return oracle.math(0, a.ravel(), b.ravel(), dtype=dtype).reshape(a.shape)

    def phi(lam, bit):
        return oracle.math(2, lam.ravel(), bit.astype(dtype).ravel(), dtype=dtype).reshape(lam.shape)

    slot = np.arange(L)
    alpha = np.zeros((B, L, N), dtype=dtype)          # level t < n at [2^t, 2^(t+1)) of the slot's own row
    pa = np.zeros((B, L, n + 1), dtype=np.int64)      # which slot's row holds level t of path p (the kernel's ptrA)
    bl = np.zeros((B, L, N), dtype=np.uint8)          # saved left-child partial sums, same layout
    pb = np.zeros((B, L, n + 1), dtype=np.int64)
    hist = np.zeros((B, L, NW), dtype=np.uint32)      # decided bits of the path
    crcr = np.zeros((B, L), dtype=np.uint64)
    PM = np.zeros((B, L), dtype=dtype)
    tie = np.zeros(B, dtype=bool)
    act = 1
    if trace is not None:
        trace.update({k: np.zeros(B, dtype=bool) for k in ("tie", "cross", "unrefilled", "all_equal")})

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
        sg = None                                     # source slot of every slot, when paths move
        if row[j] >= 0:
            w = (j >> 5) + 1
            bit = _parity32(np.bitwise_xor.reduce(hist[:, :, :w] & mask[row[j], :w], axis=-1))
            if not sc:
                PM = PM + phi(lam, bit)
        elif sc:
            bit = ((lam < 0) & (frozen[j] == 0)).astype(np.uint8)
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
            both_slots = np.argsort(~both, axis=1, kind="stable")      # the both-survivors first, ascending slot
            rank = np.cumsum(dead, axis=1) - 1
            refill = dead & (rank < both.sum(1)[:, None])
            sg = np.where(refill, np.take_along_axis(both_slots, np.clip(rank, 0, L - 1), axis=1), slot[None, :])
            c1_s = np.take_along_axis(c1, sg, axis=1)
            bit = np.where(refill, 1, np.where(s0, 0, np.where(s1, 1, 0))).astype(np.uint8)
            PM = np.where(refill, c1_s, np.where(s0, c0, np.where(s1, c1, c0)))
            if trace is not None:
                trace["tie"] |= (s0.sum(1) + s1.sum(1)) < L
                trace["cross"] |= (refill & ((sg >> 6) != (slot[None, :] >> 6))).any(1)
                trace["unrefilled"] |= (dead & ~refill).any(1)
                trace["all_equal"] |= cand.min(1) == cand.max(1)
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

    if sc:
        best = np.zeros(B, dtype=np.int64)
        pm = np.zeros(B)
        flags = np.zeros(B, dtype=np.uint32)
    else:
        live = np.broadcast_to(slot < act, (B, L))
        ok = (crcr == 0) & live if ctab is not None else np.zeros((B, L), dtype=bool)
        anyp = ok.any(1)
        ok = np.where(anyp[:, None], ok, live)
        best = np.where(ok, PM, np.inf).argmin(1)     # the first slot of least metric
        pm = PM[np.arange(B), best].astype(np.float64)
        flags = (tie.astype(np.uint32) * FLAG_TIE) | (anyp.astype(np.uint32) * FLAG_CRC_PASS)
    w = hist[np.arange(B), best]
    u_hat = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, N).astype(np.int32)
    return u_hat, pm, flags


# ---- codes and frames shared with tests/test_gpu_dyn.py --------------------------------------------------------------
def encode(u):
    """x = u F^{(x)n}, natural order, rows of 0/1"""
    x = np.array(u, dtype=np.uint8)
    N = x.shape[-1]
    h = 1
    while h < N:
        v = x.reshape(x.shape[0], N // (2 * h), 2, h)
        v[:, :, 0, :] ^= v[:, :, 1, :]
        h *= 2
    return x


def fill_dynamic(u, dyn):
    """u rows with their information bits set -> the dynamic bits filled in ascending position"""
    pos, sets = dyn
    for d, j in enumerate(pos):
        u[:, j] = u[:, np.asarray(sets[d], dtype=np.int64)].sum(axis=1) & 1 if len(sets[d]) else 0
    return u


def make_frames(N, info, dyn, B, seed, dbs=(1.0, 1.5, 2.0, 2.5), crc=None):
    """B frames of the code (information positions `info`, constraints dyn), Eb/N0 cycling over dbs at rate 1/2:
    (u [B][N], llr [B][N] float64).  crc = taps: the bits at info[0..A) are a multiple of g(D) in that order."""
    rng = np.random.default_rng(seed)
    info = np.asarray(info)
    u = np.zeros((B, N), dtype=np.int64)
    if crc is None:
        u[:, info] = rng.integers(0, 2, (B, info.size))
    else:
        r = max(crc)
        v = rng.integers(0, 2, (B, info.size - r))
        w = np.zeros((B, info.size), dtype=np.int64)
        for t in crc:
            w[:, t:t + v.shape[1]] ^= v
        u[:, info] = w
    if dyn is not None:
        fill_dynamic(u, dyn)
    x = encode(u)
    sig = 10.0 ** (-np.asarray(dbs)[np.arange(B) % len(dbs)] / 20.0)
    y = (1.0 - 2.0 * x) + sig[:, None] * rng.standard_normal((B, N))
    return u.astype(np.int32), 2.0 * y / sig[:, None] / sig[:, None]


def random_dyn(N, frozen, seed, frac=0.5, max_set=6):
    """random sparse sets on a random subset of the frozen positions; sets refer to information bits AND earlier dynamic ones"""
    rng = np.random.default_rng(seed)
    fz = np.flatnonzero(frozen)
    pos = np.sort(rng.choice(fz, size=max(1, int(len(fz) * frac)), replace=False))
    sets = []
    for j in pos:
        k = int(min(j, rng.integers(0, max_set + 1)))
        s = set(rng.choice(j, size=k, replace=False).tolist()) if k else set()
        earlier = [p for p in pos if p < j]
        if earlier and rng.integers(0, 2):
            s.add(int(earlier[-1]))                    # a chain through an earlier dynamic position
        sets.append(np.array(sorted(s), dtype=np.int32))
    return pos.astype(np.int32), sets


# ---- model against the oracle ---------------------------------------------------------------------------------------
def _oracle_frames(oracle, code, per, seed, dbs=(1.0, 1.5, 2.0, 2.5)):
    out = []
    for k, db in enumerate(dbs):
        sig = oracle.sigma_from_db(db)
        _, y = oracle.Sim(seed + k).frames(code, sig, per)
        out += [oracle.llr_from_y(v, sig) for v in y]
    return np.stack(out)


@pytest.mark.parametrize("N", [32, 64, 128])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_model_without_constraints_is_the_oracle(N, dtype, oracle):
    ds = "f32" if dtype == np.float32 else "f64"
    K = N // 2
    checked = 0
    for algo, taps in (("SC", None), ("SCL", None), ("CASCL", CRC6)):
        code = oracle.Code(N, K - (6 if taps else 0), taps)
        llr = _oracle_frames(oracle, code, 6, 40 + N)
        fz = np.flatnonzero(code.frozen)
        empties = (fz[::2].astype(np.int32), [np.zeros(0, dtype=np.int32)] * len(fz[::2]))
        for L in ((1,) if algo == "SC" else (1, 2, 8, 32)):
            ref, ref_pm, ties = oracle.decode(code, llr, algo, L=L, dtype=ds)
            keep = ties == 0
            assert keep.sum() >= len(llr) * 3 // 4
            crc = (code.info_order, taps) if taps else None
            for dyn in (None, ((), ()), empties):      # no dyn, D = 0, D > 0 with every S_j empty
                u, pm, fl = dscl_model(code.frozen, dyn, llr, L, crc=crc, dtype=dtype, sc=(algo == "SC"), oracle=oracle)
                assert np.array_equal(u[keep], ref[keep]), (algo, L)
                assert np.array_equal(pm[keep], ref_pm[keep].astype(np.float64)), (algo, L)
                assert not (fl[keep] & FLAG_TIE).any()
                checked += int(keep.sum())
    assert checked > 200


def test_model_applies_a_constraint():
    """a noiseless PAC frame decodes to itself under SC and SCL; the same frame with the constraints dropped does not"""
    import polardecoding_amd as pa
    N, K = 64, 32
    io = pa.pac_info_order(N, K)
    dyn = pa.dyn_pac(N, io, G133)
    frozen = np.ones(N, dtype=np.uint8)
    frozen[io] = 0
    u, _ = make_frames(N, io, dyn, 24, 5)
    assert u[:, dyn[0]].any()
    llr = 8.0 * (1.0 - 2.0 * encode(u))
    for L in (1, 4):
        got, pm, fl = dscl_model(frozen, dyn, llr, L)
        assert np.array_equal(got, u)
        plain, _, _ = dscl_model(frozen, None, llr, L)
        assert not np.array_equal(plain, u)


# ---- host helpers ------------------------------------------------------------------------------------------------------
def _gf2_inverse(T):
    n = T.shape[0]
    a = np.concatenate([T.copy() & 1, np.eye(n, dtype=np.uint8)], axis=1)
    for c in range(n):
        p = c + int(np.flatnonzero(a[c:, c])[0])
        a[[c, p]] = a[[p, c]]
        for r in np.flatnonzero(a[:, c]):
            if r != c:
                a[r] ^= a[c]
    return a[:, n:]


@pytest.mark.parametrize("N,K,g", [(32, 16, G133), (64, 20, 0o133), (128, 64, 0o133), (64, 32, (0, 1, 4))])
def test_dyn_pac_rows_are_the_inverse_toeplitz_matrix(N, K, g):
    import polardecoding_amd as pa
    taps = pa.pac_taps(g)
    if g == 0o133:
        assert taps == (0, 2, 3, 5, 6)
    T = np.zeros((N, N), dtype=np.uint8)
    for i in range(N):
        for t in taps:
            if i + t < N:
                T[i, i + t] = 1                       # T_ij = g_{j-i}
    Ti = _gf2_inverse(T)
    io = pa.pac_info_order(N, K)
    assert len(set(io.tolist())) == K
    pos, sets = pa.dyn_pac(N, io, g)
    assert pos.tolist() == sorted(set(range(N)) - set(io.tolist()))
    for d, j in enumerate(pos):
        # v_j = sum_i u_i Tinv[i][j] = 0  <=>  u_j = XOR of u_i over i < j with Tinv[i][j] = 1
        assert sets[d].tolist() == np.flatnonzero(Ti[:j, j]).tolist()
    rng = np.random.default_rng(N)
    v = np.zeros((50, N), dtype=np.int32)
    v[:, io] = rng.integers(0, 2, (50, K))
    u = pa.pac_precode(v, g)
    assert np.array_equal(u, (v.astype(np.int64) @ T) & 1)
    for d, j in enumerate(pos):
        assert np.array_equal(u[:, sets[d]].sum(axis=1) & 1, u[:, j])
    assert np.array_equal(pa.pac_unprecode(u, g), v)
    assert np.array_equal(fill_dynamic(np.where(np.isin(np.arange(N), io), u, 0), (pos, sets)), u)


def test_pac_rm_profile():
    import polardecoding_amd as pa
    full = pa.pac_info_order(128, 64, "rm")              # RM(3, 7): every position of weight >= 4
    assert sorted(full.tolist()) == [j for j in range(128) if bin(j).count("1") >= 4]
    io = pa.pac_info_order(128, 50, "rm")
    w = np.array([bin(j).count("1") for j in io])
    out = np.array([bin(j).count("1") for j in sorted(set(range(128)) - set(io.tolist()))])
    assert w.min() >= out.max() and (w >= 4).all() and (w == 4).sum() == 50 - 29
    q = pa.q_sequence(128)
    rel = {j: i for i, j in enumerate(q)}
    assert [rel[j] for j in io] == sorted(rel[j] for j in io)
    # among the weight-4 positions the more reliable ones were taken
    kept = [rel[j] for j in io if bin(j).count("1") == 4]
    dropped = [rel[j] for j in range(128) if bin(j).count("1") == 4 and j not in set(io.tolist())]
    assert min(kept) > max(dropped)
    assert pa.pac_info_order(128, 64, "5g").tolist() == q[64:]


def _pc5g_literal(N, q_i, n_pc, n_pc_wm, payload):
    """38.212 5.3.1.2 as written: the PC positions, and u produced by the 5-stage cyclic register from the payload bits"""
    q_i = list(q_i)
    q_pc = q_i[:n_pc - n_pc_wm]
    tilde = q_i[n_pc:]                                  # the |Q_I| - n_PC most reliable
    if n_pc_wm:
        wmin = min(bin(j).count("1") for j in tilde)
        same = [j for j in tilde if bin(j).count("1") == wmin]   # ascending reliability
        assert len(same) >= n_pc_wm
        q_pc += same[len(same) - n_pc_wm:]              # the indices of highest reliability among them
    u = np.zeros(N, dtype=np.int64)
    y = [0, 0, 0, 0, 0]
    k = 0
    for nn in range(N):
        y = y[1:] + y[:1]
        if nn in q_i:
            if nn in q_pc:
                u[nn] = y[0]
            else:
                u[nn] = payload[k]
                k += 1
                y[0] ^= int(u[nn])
    assert k == len(payload)
    return sorted(q_pc), u


@pytest.mark.parametrize("N,A", [(32, 20), (64, 20), (128, 25), (256, 18)])
@pytest.mark.parametrize("wm", [0, 1])
def test_dyn_pc5g_is_the_standards_register(N, A, wm):
    import polardecoding_amd as pa
    n_pc = 3
    q = pa.q_sequence(N)
    q_i = q[N - (A + n_pc):]
    pos, sets, info = pa.dyn_pc5g(N, q_i, n_pc, wm)
    rng = np.random.default_rng(N + wm)
    seen_one = False
    for _ in range(40):
        payload = rng.integers(0, 2, A)
        want_pc, want_u = _pc5g_literal(N, q_i, n_pc, wm, payload)
        assert pos.tolist() == want_pc
        assert info.tolist() == [j for j in q_i if j not in set(want_pc)]
        u = np.zeros((1, N), dtype=np.int64)
        u[0, np.sort(info)] = payload                  # the register takes the payload in ascending position
        fill_dynamic(u, (pos, sets))
        assert np.array_equal(u[0], want_u)
        seen_one |= bool(u[0, pos].any())
    assert seen_one
    for d, j in enumerate(pos):
        assert all(i < j and i % 5 == j % 5 and i in set(info.tolist()) for i in sets[d])


# ---- refusals (no device is touched) and the ABI ------------------------------------------------------------------------
def _create_dyn(lib, pa, N=64, K=32, algo=None, pos=(0, 1), ptr=(0, 0, 1), idx=(0,), L=4, dyn_null=False, taps=None,
                ptr_null=False):
    cfg = pa.api._Cfg()
    t = np.asarray(taps if taps else [0], dtype=np.int32)
    cfg.N, cfg.K, cfg.L, cfg.algo = N, K, L, pa.ALGO_SCL if algo is None else algo
    cfg.crc_r, cfg.n_taps, cfg.crc_taps = (max(taps), len(taps), t.ctypes.data_as(C.POINTER(C.c_int))) if taps else (0, 0, None)
    cfg.bp_iters, cfg.dtype, cfg.device = 10, pa.F64, 1 << 20          # no such device: a valid request ends in EDEVICE
    p, q, x = (np.asarray(a, dtype=np.int32) for a in (pos, ptr, idx))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    d = pa.api._Dyn(len(p), ip(p), None if ptr_null else ip(q), ip(x))
    h = C.c_void_p()
    rc = lib.polar_create_dyn(C.byref(cfg), None if dyn_null else C.byref(d), C.byref(h))
    assert not h.value or rc == 0
    if h.value:
        lib.polar_destroy(h)
    return rc


def test_create_dyn_refusals():
    import polardecoding_amd as pa
    lib = pa.load_library()
    EINVAL, EDEVICE, ENOKERNEL = -1, -3, -4
    q = pa.q_sequence(64)
    unfrozen = q[-1]
    assert q[0] == 0 and q[1] == 1                      # positions 0 and 1 are frozen under (64, 32)
    assert _create_dyn(lib, pa) == EDEVICE              # everything valid: only the device is missing
    assert _create_dyn(lib, pa, pos=(), ptr=(0,), idx=()) == EDEVICE   # D = 0 is allowed
    assert _create_dyn(lib, pa, dyn_null=True) == EINVAL
    assert _create_dyn(lib, pa, ptr_null=True) == EINVAL
    assert _create_dyn(lib, pa, ptr=(1, 1, 2)) == EINVAL                    # ptr[0] != 0
    assert _create_dyn(lib, pa, ptr=(0, 1, 0)) == EINVAL                    # rows not monotone
    assert _create_dyn(lib, pa, pos=(1, 0)) == EINVAL                       # positions not ascending
    assert _create_dyn(lib, pa, pos=(1, 1)) == EINVAL
    assert _create_dyn(lib, pa, pos=(0, 64)) == EINVAL                      # out of range
    assert _create_dyn(lib, pa, pos=(0, 1), ptr=(0, 0, 1), idx=(1,)) == EINVAL   # an entry not below its position
    assert _create_dyn(lib, pa, pos=(0, 2), ptr=(0, 0, 2), idx=(1, 0)) == EINVAL  # a row not ascending
    assert _create_dyn(lib, pa, pos=(0, 2), ptr=(0, 0, 2), idx=(1, 1)) == EINVAL
    assert _create_dyn(lib, pa, pos=(0, unfrozen), ptr=(0, 0, 0), idx=()) == EINVAL   # unfrozen under the cfg
    for algo in (pa.ALGO_BP, pa.ALGO_SCF, pa.ALGO_SCAN, 9):
        assert _create_dyn(lib, pa, algo=algo, taps=CRC6 if algo == pa.ALGO_SCF else None) == EINVAL
    for algo, taps in ((pa.ALGO_SC, None), (pa.ALGO_CASCL, CRC6)):
        assert _create_dyn(lib, pa, algo=algo, taps=taps) == EDEVICE
    assert _create_dyn(lib, pa, N=2048, K=1024) == ENOKERNEL
    assert _create_dyn(lib, pa, N=48) == EINVAL


def test_dyn_abi_is_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    names = ("polar_create_dyn", "polar_dyn_info", "polar_dyn_pac", "polar_pac_precode", "polar_pac_unprecode",
             "polar_dyn_pc5g")
    assert re.search(r"typedef\s+struct\s+polar_dyn\s*\{", hdr)
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    lib = os.path.join(REPO, "polardecoding_amd", "lib", "libpolar_hip.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in names:
        assert re.search(r"\b" + name + r"\b", out), name
    import polardecoding_amd as pa
    for f in ("PAC", "PCCASCL", "dyn_pac", "dyn_pc5g", "pac_precode", "pac_unprecode"):
        assert callable(getattr(pa, f)), f
    assert isinstance(pa.Decoder.dyn_positions, property)
