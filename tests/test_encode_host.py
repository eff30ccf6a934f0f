"""Host: numpy models of the encoder side (include/polar_hip.h "Encoder, payload extraction, systematic polar codes") and
polar_systematic_check against them.  tests/test_gpu_encode.py holds the kernels to these models.

Models, all on rows of 0/1: transform (x = u F^{(x)n}), crc_word / place / extract (CRC word by polynomial multiplication or
systematic cyclic encoding, long division on the way back), sys_encode (the two-pass systematic polar encoder), crc_table and
crc_table_sys (the N-entry CRC tables of the list decoders in the two modes)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

CRC6 = (0, 5, 6)
CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)


def _lib():
    import polardecoding_amd as pa
    if not os.path.exists(pa.lib_path()):
        import __graft_entry__ as g
        g.build()
    return pa.load_library()


# ---- models ----------------------------------------------------------------------------------------------------------------
def transform(u):
    """x = u F^{(x)n}, natural order: element j with bit s clear takes element j + 2^s, for every s"""
    x = np.array(u, dtype=np.uint8).reshape(-1, np.shape(u)[-1])
    N = x.shape[1]
    h = 1
    while h < N:
        v = x.reshape(x.shape[0], N // (2 * h), 2, h)
        v[:, :, 0, :] ^= v[:, :, 1, :]
        h *= 2
    return x


def poly_divmod(w, taps):
    """rows w [B][A] (coefficient of D^i at i) divided by g(D): (quotient [B][A-r], remainder [B][r])"""
    w = np.array(w, dtype=np.uint8)
    r = max(taps)
    q = np.zeros((w.shape[0], w.shape[1] - r), dtype=np.uint8)
    for i in range(w.shape[1] - 1, r - 1, -1):
        c = w[:, i].copy()
        q[:, i - r] = c
        for t in taps:
            w[:, i - r + t] ^= c
    return q, w[:, :r]


def crc_word(v, taps, crc_systematic=False):
    """payload rows v [B][K] -> w [B][K+r]: v(D) g(D), or (D^r v mod g, v)"""
    v = np.array(v, dtype=np.uint8)
    if not taps:
        return v
    B, K = v.shape
    r = max(taps)
    if crc_systematic:
        sh = np.concatenate([np.zeros((B, r), dtype=np.uint8), v], axis=1)
        return np.concatenate([poly_divmod(sh, taps)[1], v], axis=1)
    w = np.zeros((B, K + r), dtype=np.uint8)
    for t in taps:
        w[:, t:t + K] ^= v
    return w


def place(v, N, info, taps=None, crc_systematic=False):
    z = np.zeros((np.shape(v)[0], N), dtype=np.uint8)
    z[:, np.asarray(info)] = crc_word(v, taps, crc_systematic)
    return z


def extract(z, info, taps=None, crc_systematic=False):
    """N-bit rows -> (payload [B][K], ok [B])"""
    w = np.asarray(z, dtype=np.uint8)[:, np.asarray(info)]
    if not taps:
        return w, np.ones(w.shape[0], dtype=np.uint32)
    q, rem = poly_divmod(w, taps)
    ok = (~rem.any(axis=1)).astype(np.uint32)
    return (w[:, max(taps):] if crc_systematic else q), ok


def sys_encode(z, info):
    """the two-pass systematic encoder on placed rows z: (u, x)"""
    frozen = np.ones(z.shape[1], dtype=bool)
    frozen[np.asarray(info)] = False
    t = transform(z)
    t[:, frozen] = 0
    x = transform(t)
    return transform(x), x


def sys_check(N, info):
    info = np.asarray(info)
    z = np.zeros((info.size, N), dtype=np.uint8)
    z[np.arange(info.size), info] = 1
    u, x = sys_encode(z, info)
    frozen = np.ones(N, dtype=bool)
    frozen[info] = False
    return bool(np.array_equal(x[:, info], np.eye(info.size, dtype=np.uint8)) and not u[:, frozen].any())


def crc_table(N, info, taps):
    """tab[I[i]] = D^i mod g(D) as an r-bit integer, 0 at frozen positions"""
    r = max(taps)
    glow = sum(1 << t for t in taps if t < r)
    tab = np.zeros(N, dtype=np.uint64)
    rem = 1
    for j in info:
        tab[j] = rem
        rem <<= 1
        if rem >> r:
            rem = (rem ^ (1 << r)) ^ glow
    return tab


def crc_table_sys(N, info, taps):
    """tab_sys[j] = XOR over {i : (j & I[i]) == I[i]} of tab[I[i]] at unfrozen j, 0 at frozen j"""
    tab = crc_table(N, info, taps)
    info = np.asarray(info)
    out = np.zeros(N, dtype=np.uint64)
    for j in info:
        sub = info[(j & info) == info]
        out[j] = np.bitwise_xor.reduce(tab[sub])
    return out


def syndrome(tab, u):
    """XOR over {j : u_j = 1} of tab[j], per row"""
    return np.array([np.bitwise_xor.reduce(tab[row.astype(bool)], initial=np.uint64(0)) for row in np.asarray(u)], dtype=np.uint64)


def pack(bits):
    """rows of 0/1 [B][n] -> uint32 words [B][ceil(n/32)], bit k & 31 of word k >> 5 = element k"""
    b = np.asarray(bits, dtype=np.uint8)
    n = b.shape[1]
    pad = np.zeros((b.shape[0], -n % 32), dtype=np.uint8)
    return np.packbits(np.concatenate([b, pad], axis=1), axis=1, bitorder="little").view(np.uint32)


def unpack(words, n):
    w = np.ascontiguousarray(words).view(np.uint8).reshape(np.shape(words)[0], -1)
    return np.unpackbits(w, axis=1, bitorder="little")[:, :n]


def default_order(N):
    """the library's reliability order: the 5G sequence up to 1024, polarization weight (beta = 2^(1/4)) above"""
    import polardecoding_amd as pa
    if N <= 1024:
        return np.asarray(pa.q_sequence(N), dtype=np.int32)
    j = np.arange(N)
    w = sum(((j >> b) & 1) * 2.0 ** (b / 4) for b in range(N.bit_length() - 1))
    return np.argsort(w, kind="stable").astype(np.int32)


def random_set(N=64, A=32, seed=20):
    """a seeded random information set: the two-pass encoder is not systematic on it"""
    return np.sort(np.random.default_rng(seed).permutation(N)[:A]).astype(np.int32)


# ---- the model checks itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [32, 64, 1024])
def test_transform_is_an_involution_and_the_kronecker_power(N):
    rng = np.random.default_rng(N)
    u = rng.integers(0, 2, (7, N)).astype(np.uint8)
    assert np.array_equal(transform(transform(u)), u)
    j = np.arange(N)
    G = ((j[:, None] & j[None, :]) == j[None, :]).astype(np.int64)   # G[j][c] = 1 iff c is a subset of j
    assert np.array_equal(transform(u), (u.astype(np.int64) @ G) & 1)


@pytest.mark.parametrize("taps", [CRC6, CRC24C], ids=["crc6", "crc24c"])
@pytest.mark.parametrize("crc_sys", [False, True], ids=["plain", "syscrc"])
@pytest.mark.parametrize("N,K", [(128, 64), (1024, 500), (64, 13)])
def test_extract_inverts_place(N, K, taps, crc_sys):
    import polardecoding_amd as pa
    A = K + max(taps)
    info = np.asarray(pa.q_sequence(N)[N - A:])
    rng = np.random.default_rng(K)
    v = rng.integers(0, 2, (20, K)).astype(np.uint8)
    z = place(v, N, info, taps, crc_sys)
    got, ok = extract(z, info, taps, crc_sys)
    assert np.array_equal(got, v) and ok.all()
    # one flipped information bit is always caught (a single bit is no multiple of g)
    z[np.arange(20), info[rng.integers(0, A, 20)]] ^= 1
    assert not extract(z, info, taps, crc_sys)[1].any()
    if crc_sys:
        w = z[:, info]
        assert np.array_equal(w[:, max(taps):], extract(z, info, taps, True)[0])


@pytest.mark.parametrize("N,K,taps", [(32, 13, None), (128, 64, CRC6), (1024, 500, CRC24C)])
def test_two_pass_encoder_is_systematic(N, K, taps):
    import polardecoding_amd as pa
    A = K + (max(taps) if taps else 0)
    info = np.asarray(pa.q_sequence(N)[N - A:])
    v = np.random.default_rng(N).integers(0, 2, (30, K)).astype(np.uint8)
    z = place(v, N, info, taps)
    u, x = sys_encode(z, info)
    frozen = np.ones(N, dtype=bool)
    frozen[info] = False
    assert np.array_equal(x[:, info], z[:, info]) and not u[:, frozen].any()
    assert np.array_equal(transform(u), x)
    if taps:   # the systematic table on u is the plain table on the CRC word carried by x
        z_as_u = np.zeros_like(z)
        z_as_u[:, info] = x[:, info]
        assert np.array_equal(syndrome(crc_table_sys(N, info, taps), u), syndrome(crc_table(N, info, taps), z_as_u))
        assert not syndrome(crc_table_sys(N, info, taps), u).any()
        u[:, info[3]] ^= 1
        assert np.array_equal(syndrome(crc_table_sys(N, info, taps), u),
                              syndrome(crc_table(N, info, taps), np.where(frozen, 0, transform(u))))


# ---- polar_systematic_check against the model --------------------------------------------------------------------------
def _check(N, info):
    import ctypes as C
    io = np.ascontiguousarray(info, dtype=np.int32)
    return _lib().polar_systematic_check(N, io.ctypes.data_as(C.POINTER(C.c_int)), io.size)


@pytest.mark.parametrize("N", [32, 64])
def test_check_every_A_of_the_5g_order(N):
    import polardecoding_amd as pa
    q = pa.q_sequence(N)
    for A in range(1, N + 1):
        assert sys_check(N, q[N - A:])
        assert _check(N, q[N - A:]) == 1


@pytest.mark.parametrize("N,As", [(1024, (1, 37, 512, 524, 1000, 1024)), (4096, (1, 100, 2048, 3000))])
def test_check_sampled_A_of_the_default_order(N, As):
    q = default_order(N)
    for A in As:
        assert sys_check(N, q[N - A:]) and _check(N, q[N - A:]) == 1


def test_check_rejects_a_random_set():
    info = random_set()
    assert not sys_check(64, info)
    assert _check(64, info) == 0
    import polardecoding_amd as pa
    assert pa.systematic_check(64, info) is False and pa.systematic_check(64, pa.q_sequence(64)[32:]) is True


def test_check_refusals():
    q = np.arange(32, dtype=np.int32)
    assert _check(48, q) < 0 and _check(16, q[:8]) < 0 and _check(8192, q) < 0
    assert _check(32, np.array([1, 1], dtype=np.int32)) < 0 and _check(32, np.array([32], dtype=np.int32)) < 0
    assert _lib().polar_systematic_check(32, None, 4) < 0


def test_encode_abi_is_declared_and_exported():
    lib = _lib()
    hdr = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    for name in ("polar_transform_device", "polar_encode_device", "polar_payload_device", "polar_encode_batch",
                 "polar_payload_batch", "polar_set_systematic", "polar_get_systematic", "polar_systematic_check"):
        assert name + "(" in hdr
        assert getattr(lib, name) is not None
