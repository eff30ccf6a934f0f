"""CPU: BP early termination (polar_bp_set_stop, include/polar_hip.h).

A numpy restatement of the reference's BP (BP_1024.c:372-427, CHK :311-342) that also yields r[n] -- the row the
fixed-iteration decoder never needs -- so that the stop point of the G-matrix criterion (u_hat F == x_hat) can be found
for every frame.  Its fixed-iteration decisions are checked against the oracle here; tests/test_gpu_bp_early_stop.py
then takes the stop points from it.  Also: the new C ABI is declared and exported."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# CHK's staircase (BP_1024.c:318-333): delta = T(|L1 + L2|) - T(|L1 - L2|), thresholds and levels as written
_THR = (0.196, 0.433, 0.71, 1.05, 1.508, 2.252, 4.5)
_LVL = (0.65, 0.55, 0.45, 0.35, 0.25, 0.15, 0.05)


def _stair(x):
    out = np.zeros_like(x)
    done = np.zeros(x.shape, dtype=bool)
    for t, v in zip(_THR, _LVL):
        hit = ~done & (x < t)
        out[hit] = v
        done |= hit
    return out


def chk(L1, L2):
    """CHK(L1, L2), BP_1024.c:311-342, element-wise and in the reference's operation order."""
    sAbs = np.abs(L1 + L2)
    dAbs = np.abs(L1 - L2)
    delta = _stair(sAbs)
    delta = delta - _stair(dAbs)   # `delta -= ...`; with no threshold hit it stays as it was (x - 0 == x)
    A1, A2 = np.abs(L1), np.abs(L2)
    s = np.where(L1 >= 0, 1.0, -1.0) * np.where(L2 >= 0, 1.0, -1.0)   # s1 * s2: +-1, exact
    return np.where(A1 > A2, s * A2 + delta, s * A1 + delta)


def encode(u):
    """x = u F^{(x)n} over GF(2), natural order (SCL_1024.c:242-250): x[j] ^= x[j + s] for j with bit s clear."""
    x = np.array(u, dtype=np.int32, copy=True)
    N = x.shape[-1]
    s = 1
    while s < N:
        v = x.reshape(x.shape[:-1] + (N // (2 * s), 2, s))
        v[..., 0, :] ^= v[..., 1, :]
        s *= 2
    return x


def bp_rounds(llr, frozen, iters):
    """Reference BP on a batch llr [B][N] (f64), frozen [N] 0/1.  Yields, after each round trip t = 1..iters, the pair
    (u_hat [B][N], x_hat [B][N]) of include/polar_hip.h: u_hat from l[0] + r[0] (frozen -> 0), x_hat from l[n] + r[n]."""
    llr = np.asarray(llr, dtype=np.float64)
    B, N = llr.shape
    n = N.bit_length() - 1
    fz = np.asarray(frozen, dtype=bool)
    l = np.zeros((n + 1, B, N))
    r = np.zeros((n + 1, B, N))
    l[n] = llr                                     # BP_1024.c:381-382
    r[0] = np.where(fz, 999.0, 0.0)[None, :]       # :386-391
    upper = [np.array([k for k in range(N) if not k & (1 << i)]) for i in range(n)]   # j with bit i clear
    for _ in range(iters):
        for i in range(n):                         # R sweep, :395-404
            s = 1 << i
            j = upper[i]
            a = chk(r[i][:, j], l[i + 1][:, j + s] + r[i][:, j + s])
            b = r[i][:, j + s] + chk(r[i][:, j], l[i + 1][:, j])
            r[i + 1][:, j] = a
            r[i + 1][:, j + s] = b
        for i in range(n - 1, -1, -1):             # L sweep, :406-415
            s = 1 << i
            j = upper[i]
            a = chk(l[i + 1][:, j], l[i + 1][:, j + s] + r[i][:, j + s])
            b = l[i + 1][:, j + s] + chk(r[i][:, j], l[i + 1][:, j])
            l[i][:, j] = a
            l[i][:, j + s] = b
        u_hat = np.where(fz[None, :], 0, np.where(l[0] + r[0] >= 0, 0, 1)).astype(np.int32)   # :417-425
        x_hat = np.where(l[n] + r[n] >= 0, 0, 1).astype(np.int32)
        yield u_hat, x_hat


def stop_points(llr, frozen, iter_max):
    """Per frame: the first round trip t <= iter_max with u_hat F == x_hat (converged = True), else iter_max (False), and
    the decisions at that round trip."""
    B, N = np.asarray(llr).shape
    t_stop = np.full(B, iter_max, dtype=np.int64)
    conv = np.zeros(B, dtype=bool)
    out = np.zeros((B, N), dtype=np.int32)
    for t, (u_hat, x_hat) in enumerate(bp_rounds(llr, frozen, iter_max), start=1):
        hold = ~conv & np.all(encode(u_hat) == x_hat, axis=1)
        t_stop[hold] = t
        out[hold] = u_hat[hold]
        conv |= hold
        if t == iter_max:
            out[~conv] = u_hat[~conv]
        elif conv.all():
            break
    return t_stop, conv, out


def test_encode_is_the_generator_matrix():
    """encode() against the rows of F^{(x)n} built as a Kronecker power (SCL_1024.c:184-197 builds Fn the same way)."""
    F = np.array([[1, 0], [1, 1]], dtype=np.int32)
    Fn = F
    for _ in range(4):
        Fn = np.kron(Fn, F)
    rng = np.random.default_rng(1)
    u = rng.integers(0, 2, (20, 32)).astype(np.int32)
    assert np.array_equal(encode(u), (u @ Fn) % 2)


@pytest.mark.parametrize("N,K", [(128, 64), (256, 128)])
def test_restated_bp_equals_the_oracle(N, K, oracle):
    """The restatement's fixed-iteration decisions equal the oracle's po_bp_decode_f64 (= the reference's BP()) for
    t = 1, 2, 7, 30 round trips, over 1 to 3 dB."""
    code = oracle.Code(N, K)
    frames = []
    for k, db in enumerate((1.0, 2.0, 3.0)):
        sim = oracle.Sim(700 + N + k)
        sig = oracle.sigma_from_db(db)
        _, ys = sim.frames(code, sig, 12)
        frames += [oracle.llr_from_y(y, sig) for y in ys]
    llr = np.stack(frames)
    want = {1, 2, 7, 30}
    for t, (u_hat, x_hat) in enumerate(bp_rounds(llr, code.frozen, 30), start=1):
        if t in want:
            ref, _, _ = oracle.decode(code, llr, "BP", bp_iters=t)
            assert np.array_equal(u_hat, ref), t
    # x_hat is a hard decision of the channel side: at 3 dB after 30 round trips most frames are codewords
    t_stop, conv, out = stop_points(llr, code.frozen, 30)
    assert conv[-12:].sum() >= 6
    for b in np.flatnonzero(conv):
        ref, _, _ = oracle.decode(code, llr[b], "BP", bp_iters=int(t_stop[b]))
        assert np.array_equal(out[b], ref)


NEW_SYMBOLS = ["polar_bp_set_stop", "polar_bp_decode_device", "polar_bp_decode_batch"]


def test_stop_rule_abi_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "polar_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    full = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    for macro, val in (("POLAR_BP_STOP_NONE", "0"), ("POLAR_BP_STOP_G", "1"), ("POLAR_FLAG_BP_CONVERGED", "0x8u")):
        assert re.search(r"#define\s+" + macro + r"\s+" + re.escape(val) + r"\b", full), macro
    import polardecoding_amd as pa
    lib = pa.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert (pa.BP_STOP_NONE, pa.BP_STOP_G, pa.FLAG_BP_CONVERGED) == (0, 1, 8)
