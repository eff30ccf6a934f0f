"""CPU: 5G NR rate matching (TS 38.212 5.4.1, include/polar_hip.h rules 1-6).

The model below is written from 38.212, not from the library: the sub-block interleaver (5.4.1.1), bit selection
(5.4.1.2), the triangular channel interleaver (5.4.1.3), the pre-frozen set Q_F,tmp of 5.3.1.2, the choice of N (5.3.1) and
the receiver's recovery.  It is checked for its own properties here, the library's host functions are checked against it,
and tests/test_gpu_rm.py checks the kernels against it."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

P32 = [0, 1, 2, 4, 3, 5, 6, 7, 8, 16, 9, 17, 10, 18, 11, 19, 12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31]
REPEAT, PUNCTURE, SHORTEN = 1, 2, 3
SHORT_LLR = 1048576.0


def q_order(N):
    """the 5G reliability sequence restricted to < N, ascending reliability (38.212 Table 5.3.1.2-1)"""
    vals = []
    with open(os.path.join(REPO, "polardecoding_amd", "data", "q5g_nmax1024.txt")) as f:
        for line in f:
            if not line.startswith("#"):
                vals += [int(x) for x in line.split()]
    return [x for x in vals if x < N]


def sub_block_J(N):
    """5.4.1.1: J(n) = P(i) (N/32) + n mod (N/32), i = floor(32 n / N)"""
    n = np.arange(N)
    return np.array([P32[(32 * k) // N] * (N // 32) + k % (N // 32) for k in n])


def mode_of(N, A, E):
    """5.4.1.2"""
    if E >= N:
        return REPEAT
    return PUNCTURE if 16 * A <= 7 * E else SHORTEN


def channel_perm(E):
    """5.4.1.3: sent[t] = e[perm[t]]: written row by row into the upper triangle, read column by column"""
    T = 0
    while T * (T + 1) // 2 < E:
        T += 1
    v = [[None] * T for _ in range(T)]
    k = 0
    for i in range(T):
        for j in range(T - i):
            if k < E:
                v[i][j] = k
            k += 1
    out = []
    for j in range(T):
        for i in range(T - j):
            if v[i][j] is not None:
                out.append(v[i][j])
    return np.array(out)


def pre_frozen(N, A, E):
    """Q_F,tmp of 5.3.1.2 (n_PC = 0)"""
    J = sub_block_J(N)
    q = set()
    if E < N:
        if 16 * A <= 7 * E:
            q |= set(J[:N - E].tolist())
            t = -(-(3 * N - 2 * E) // 4) if 4 * E >= 3 * N else -(-(9 * N - 4 * E) // 16)
            q |= set(range(t))
        else:
            q |= set(J[E:].tolist())
    return q


def info_order(N, A, E):
    """rule 4: the A most reliable positions outside Q_F,tmp, ascending reliability; None if fewer are left"""
    pre = pre_frozen(N, A, E)
    keep = [x for x in q_order(N) if x not in pre]
    return np.array(keep[-A:]) if len(keep) >= A else None


def select_n(A, E, n_max):
    """5.3.1"""
    cl = int(np.ceil(np.log2(E)))
    if E <= (9 / 8) * 2 ** (cl - 1) and 16 * A < 9 * E:
        n1 = cl - 1
    else:
        n1 = cl
    n2 = int(np.ceil(np.log2(8 * A)))
    return 2 ** max(min(n1, n2, n_max), 5)


def encode(u):
    """d = u F^{(x)n} over rows of u [B][N]"""
    x = np.array(u, dtype=np.uint8)
    N = x.shape[-1]
    h = 1
    while h < N:
        x = x.reshape(x.shape[0], -1, 2, h)
        x[:, :, 0, :] ^= x[:, :, 1, :]
        x = x.reshape(x.shape[0], N)
        h *= 2
    return x


def transmit(d, E, A, ibil):
    """rules 1-3 on codewords d [B][N]: the sent bits [B][E]"""
    N = d.shape[-1]
    y = d[:, sub_block_J(N)]
    m = mode_of(N, A, E)
    k = np.arange(E)
    e = y[:, k % N] if m == REPEAT else y[:, k + N - E] if m == PUNCTURE else y[:, k]
    return e[:, channel_perm(E)] if ibil else e


def recover(rx, N, A, ibil, sigma=0.0, out_dtype=None):
    """rule 6: received rows rx [B][E] -> decoder rows [B][N] (double accumulation, one rounding to out_dtype)"""
    rx = np.asarray(rx)
    out_dtype = out_dtype or rx.dtype
    B, E = rx.shape
    t = rx.astype(np.float64)
    if sigma > 0:
        t = 2 * t / sigma / sigma
    if ibil:
        e = np.empty_like(t)
        e[:, channel_perm(E)] = t
    else:
        e = t
    m = mode_of(N, A, E)
    yv = np.empty((B, N), dtype=np.float64)
    if m == REPEAT:
        yv[:] = e[:, :N]
        for s in range(N, E, N):
            c = min(N, E - s)
            yv[:, :c] = yv[:, :c] + e[:, s:s + c]
    elif m == PUNCTURE:
        yv[:, :N - E] = 0.0
        yv[:, N - E:] = e
    else:
        yv[:, :E] = e
        yv[:, E:] = SHORT_LLR
    out = np.empty((B, N), dtype=np.float64)
    out[:, sub_block_J(N)] = yv
    return out.astype(out_dtype)


# ---- the model's own properties ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [32, 64, 128, 256, 512, 1024])
def test_J_is_a_permutation(N):
    assert sorted(sub_block_J(N).tolist()) == list(range(N))


@pytest.mark.parametrize("E", [1, 2, 3, 10, 63, 64, 65, 500, 864, 1700, 8192])
def test_channel_interleaver_is_a_permutation(E):
    p = channel_perm(E)
    assert sorted(p.tolist()) == list(range(E))
    if E == 10:   # T = 4: columns (0,4,7,9), (1,5,8), (2,6), (3)
        assert p.tolist() == [0, 4, 7, 9, 1, 5, 8, 2, 6, 3]


@pytest.mark.parametrize("N,A,E", [(1024, 536, 864), (1024, 536, 1000), (512, 300, 400), (128, 60, 100), (32, 20, 25)])
def test_shortened_bits_are_zero(N, A, E):
    assert mode_of(N, A, E) == SHORTEN
    I = info_order(N, A, E)
    rng = np.random.default_rng(N + E)
    u = np.zeros((64, N), dtype=np.uint8)
    u[:, I] = rng.integers(0, 2, (64, A))
    d = encode(u)
    J = sub_block_J(N)
    assert not d[:, J[E:]].any()


@pytest.mark.parametrize("N,A,E", [(1024, 224, 864), (1024, 224, 640), (512, 100, 300), (64, 20, 50), (32, 8, 24)])
def test_puncturing_prefreezes_the_stated_ranges(N, A, E):
    assert mode_of(N, A, E) == PUNCTURE
    J = sub_block_J(N)
    t = -(-(3 * N - 2 * E) // 4) if 4 * E >= 3 * N else -(-(9 * N - 4 * E) // 16)
    assert pre_frozen(N, A, E) == set(J[:N - E].tolist()) | set(range(t))


@pytest.mark.parametrize("N", [32, 128, 1024])
def test_no_prefreezing_at_or_above_N(N):
    A = N // 2
    for E in (N, N + 1, 3 * N, 8192):
        assert pre_frozen(N, A, E) == set()
        assert info_order(N, A, E).tolist() == q_order(N)[-A:]


@pytest.mark.parametrize("A,E,n9,n10", [(18, 54, 64, 64), (20, 140, 128, 128), (41, 200, 256, 256), (75, 600, 512, 1024),
                                        (164, 864, 512, 1024), (524, 1700, 512, 1024)])
def test_select_n_hand_worked(A, E, n9, n10):
    assert select_n(A, E, 9) == n9
    assert select_n(A, E, 10) == n10


def test_recover_inverts_transmit():
    """recovering the sent LLRs of a noiseless row gives each codeword position its sign (or the stated fills)"""
    for N, A, E in [(64, 20, 50), (64, 40, 50), (64, 20, 200), (1024, 536, 864)]:
        rng = np.random.default_rng(E)
        d = rng.integers(0, 2, (3, N)).astype(np.uint8)
        for ibil in (0, 1):
            tx = 1.0 - 2.0 * transmit(d, E, A, ibil)
            r = recover(tx, N, A, ibil)
            m = mode_of(N, A, E)
            known = r != 0.0 if m == PUNCTURE else r != SHORT_LLR
            assert np.array_equal(np.sign(r[known]), (1.0 - 2.0 * d)[known])
            if m == REPEAT:
                mult = np.array([len(range(n, E, N)) for n in range(N)])
                assert np.array_equal(np.abs(r[:, sub_block_J(N)]), np.broadcast_to(mult, (3, N)))


# ---- the library's host functions against the model ------------------------------------------------------------------

def _lib():
    import polardecoding_amd as pa
    if not os.path.exists(pa.lib_path()):
        import __graft_entry__ as g
        g.build()
    return pa.load_library()


def _pairs(N):
    """(A, E) on every side of 16A = 7E and 4E = 3N, and E in {N-1, N, N+1, 8192}"""
    out = set()
    for E in sorted({max(1, N // 4), N // 2, (3 * N) // 4 - 1, (3 * N) // 4, (3 * N + 3) // 4, N - 1, N, N + 1, 2 * N + 3,
                     8192}):
        for A in {1, 2, max(1, (7 * E) // 16 - 1), max(1, (7 * E) // 16), (7 * E) // 16 + 1, min(E, N // 2), min(E, N - 1),
                  min(E, N)}:
            if 1 <= A <= E:
                out.add((A, E))
    return sorted(out)


@pytest.mark.parametrize("N", [32, 64, 128, 256, 512, 1024])
def test_info_order_matches_the_model(N):
    lib = _lib()
    for A, E in _pairs(N):
        want = info_order(N, A, E)
        out = np.full(A, -7, dtype=np.int32)
        rc = lib.polar_rm_info_order(N, A, E, out.ctypes.data_as(C.POINTER(C.c_int)))
        if want is None:
            assert rc == -1, (N, A, E)
        else:
            assert rc == 0, (N, A, E)
            assert out.tolist() == want.tolist(), (N, A, E)


def test_select_n_matches_the_model():
    lib = _lib()
    for A in (1, 12, 18, 20, 41, 75, 164, 200, 524, 1000):
        for E in sorted({A, A + 1, 2 * A, 54, 140, 200, 600, 864, 1700, 4000, 8192}):
            if A <= E <= 8192:
                for nm in (9, 10):
                    assert lib.polar_rm_select_n(A, E, nm) == select_n(A, E, nm), (A, E, nm)
    assert lib.polar_rm_select_n(10, 9, 10) == -1
    assert lib.polar_rm_select_n(10, 8193, 10) == -1
    assert lib.polar_rm_select_n(10, 100, 8) == -1
    import polardecoding_amd as pa
    assert pa.rm_select_n(164, 864, 9) == 512 and pa.rm_select_n(164, 864) == 1024


def test_info_order_refusals():
    lib = _lib()
    out = np.zeros(2048, dtype=np.int32)
    p = out.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.polar_rm_info_order(2048, 100, 2048, p) == -1    # N > 1024
    assert lib.polar_rm_info_order(96, 10, 96, p) == -1         # not a power of two
    assert lib.polar_rm_info_order(16, 4, 16, p) == -1          # N < 32
    assert lib.polar_rm_info_order(64, 10, 9, p) == -1          # E < A
    assert lib.polar_rm_info_order(64, 10, 8193, p) == -1       # E > 8192
    assert lib.polar_rm_info_order(64, 0, 10, p) == -1          # A < 1
    assert lib.polar_rm_info_order(64, 10, 10, None) == -1


def test_create_rm_refuses_before_touching_a_device():
    import polardecoding_amd as pa
    lib = _lib()
    taps = np.array(pa.CRC24C_TAPS, dtype=np.int32)
    order = np.arange(536, dtype=np.int32)

    def cfg(N=1024, K=512, algo=pa.ALGO_CASCL, io=None):
        g = pa.api._Cfg()
        g.N, g.K, g.crc_r, g.n_taps = N, K, 24, len(taps)
        g.crc_taps = taps.ctypes.data_as(C.POINTER(C.c_int))
        g.L, g.algo, g.bp_iters, g.dtype, g.device = 8, algo, 50, pa.F64, 0
        if io is not None:
            g.info_order = io.ctypes.data_as(C.POINTER(C.c_int))
        return g

    h = C.c_void_p()
    for g, E, ibil in [(cfg(io=order), 864, 0),            # caller's info_order
                       (cfg(N=2048, K=512), 2048, 0),      # N > 1024
                       (cfg(N=16, K=4, algo=pa.ALGO_SC), 16, 0),
                       (cfg(), 535, 0),                     # E < A = 536
                       (cfg(), 8193, 0),                    # E > 8192
                       (cfg(), 864, 2),                     # ibil
                       (cfg(N=32, K=40, algo=pa.ALGO_SC), 64, 0)]:   # A > N - |Q_F,tmp| (repetition: A > N)
        assert lib.polar_create_rm(C.byref(g), E, ibil, C.byref(h)) == -1
        assert not h.value
    assert info_order(32, 40, 64) is None
    with pytest.raises(ValueError):
        pa.CASCL(1024, 512, L=8, crc_file="whatever.dat", E=864)


def test_rm_abi_is_declared_and_exported():
    lib = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "polar_hip.h")).read(), flags=re.S)
    for name in ("polar_rm_select_n", "polar_rm_info_order", "polar_create_rm", "polar_rm_info", "polar_rm_recover_device"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name)
    for d, v in (("POLAR_RM_NONE", "0"), ("POLAR_RM_REPEAT", "1"), ("POLAR_RM_PUNCTURE", "2"), ("POLAR_RM_SHORTEN", "3"),
                 ("POLAR_RM_SHORT_LLR", "1048576.0")):
        assert re.search(r"#define\s+" + d + r"\s+" + re.escape(v) + r"\b", hdr), d
    import polardecoding_amd as pa
    out = subprocess.run(["nm", "-D", "--defined-only", pa.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "polar_create_rm" in out and "polar_rm_recover_device" in out
    assert np.float32(SHORT_LLR) == SHORT_LLR   # exact in f32


def test_polar_sim_refuses_E_without_fast():
    sim = os.path.join(REPO, "polardecoding_amd", "lib", "polar_sim")
    if not os.path.exists(sim):
        _lib()
        import __graft_entry__ as g
        g.build()
    r = subprocess.run([sim, "--algo", "cascl", "--N", "1024", "--K", "512", "--E", "864", "--snr", "1:1:1"],
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "--fast" in r.stderr
