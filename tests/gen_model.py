"""A numpy statement of the device-side transmit chain (include/polar_hip.h, "device-side transmit chain"; the kernels are
k_generate, k_generate_rm, k_generate_dyn and k_genie_rows), written from the documented rule and not from the kernels:

  Philox4x32-10, counter (frame lo, frame hi, block, stream), key (seed lo, seed hi);
  payload word w = c[0] of (block w, stream 0), K bits, the last word masked when K & 31;
  CRC multiply w = v g, or the systematic rows (w[0..r) = v(D) D^r mod g, w[r..K+r) = v); placement u[I[i]] = w[i];
  systematic polar mode u = (z F) with the frozen positions cleared; dynamic bits in ascending position; x = u F;
  two normals per block: u0, u1 = ((top 53 bits of c0:c1, c2:c3) + 0.5) 2^-53, r = sqrt(-2 log u0), (r cos 2 pi u1, r sin 2 pi u1);
  element -> (block, normal, stream): k_generate / k_generate_dyn  j -> ((j & 63) + 64 (j >> 7), (j >> 6) & 1, 1),
                                      k_generate_rm sent position t -> (t >> 1, t & 1, 2),  k_genie_rows e -> (e >> 1, e & 1, 2);
  y = +-1 + sigma z, LLR = 2 * y / sigma / sigma.

The integer steps and the uniforms are exact (the uniforms are IEEE binary64 basic operations, reproduced bit for bit); the
Box-Muller and everything after it is evaluated in np.longdouble (64-bit mantissa) from those binary64 uniforms, with the
angle reduced exactly in integers first.  tests/test_gen_model_host.py checks this file against the Random123 known-answer
vectors and against mpmath; tests/test_gpu_generator_values.py holds the kernels to it.  Nothing here imports the package's
kernels: the information order, the dynamic sets and a CRC generator matrix are arguments."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_dyn_host as DYN  # noqa: E402  (fill_dynamic: the dynamic-bit model of the decoder tests)
import test_rm_host as RM  # noqa: E402  (transmit: rules 1-3 of rate matching, written from 38.212)

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs a long double with a 64-bit mantissa"
# from a string: a Python float literal would carry 53 bits
PI = LD("3.14159265358979323846264338327950288419716939937510582097494459")

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = U64(0xD2511F53), U64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
STREAM_PAYLOAD, STREAM_NOISE, STREAM_ROWS = 0, 1, 2
EPS = 2.0 ** -52       # one ulp of a binary64 value, relative to it, at most
Z_MAX = float(np.sqrt(2 * 54 * np.log(2.0)))   # u0 >= 2^-54: no normal is larger than sqrt(2 * 54 * ln 2) = 8.65


# ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key, rounds=10, m0=PHILOX_M0):
    """counter: four uint64 arrays holding 32-bit words (broadcast against each other), key: two -> the four output words.
    (rounds and m0 are arguments so that the tests can show that a wrong constant is seen.)"""
    c = [np.asarray(x, dtype=U64) & M32 for x in np.broadcast_arrays(*[np.asarray(x, dtype=U64) for x in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = m0 * c[0]              # 32 x 32 bits: fits 64
        p1 = PHILOX_M1 * c[2]
        c = [((p1 >> U64(32)) ^ c[1] ^ U64(k0)) & M32, p1 & M32, ((p0 >> U64(32)) ^ c[3] ^ U64(k1)) & M32, p0 & M32]
        k0 = (k0 + PHILOX_W0) & 0xFFFFFFFF
        k1 = (k1 + PHILOX_W1) & 0xFFFFFFFF
    return c


def frame_block(seed, frames, blocks, stream, **kw):
    """the output words [4] of arrays [B][nb] for frames [B] (uint64 frame indices, taken mod 2^64) x blocks [nb]"""
    f = np.asarray(frames, dtype=U64).reshape(-1, 1)
    b = np.asarray(blocks, dtype=U64).reshape(1, -1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((f & M32, f >> U64(32), b, U64(stream)), (seed & 0xFFFFFFFF, seed >> 32), **kw)


def frames_of(first_frame, B):
    """frame indices first_frame .. first_frame + B - 1 as uint64"""
    return np.array([(int(first_frame) + i) & 0xFFFFFFFFFFFFFFFF for i in range(int(B))], dtype=U64)


# ---- uniforms and Box-Muller -------------------------------------------------------------------------------------------------
def k53(hi, lo):
    """the top 53 bits of hi:lo"""
    return ((np.asarray(hi, dtype=U64) << U64(32)) | np.asarray(lo, dtype=U64)) >> U64(11)


def uniform(k):
    """(double(k) + 0.5) * 2^-53 in binary64, as written: for k >= 2^52 the sum is not representable and rounds to even, so the
    result lies in (0, 1]: 1.0 is reached (k = 2^53 - 1), 0 is not."""
    return (np.asarray(k, dtype=U64).astype(np.float64) + np.float64(0.5)) * np.float64(2.0 ** -53)


def box_muller(u0, u1):
    """binary64 uniforms -> (r cos 2 pi u1, r sin 2 pi u1), r = sqrt(-2 log u0), in long double.
    2 u1 = m 2^-53 with m an integer <= 2^54: m is split into the nearest multiple q of 2^52 (a quarter turn) and a remainder
    of at most 2^51 in magnitude, so that sin and cos are only taken of |angle| <= pi / 4 and the quadrant is exact."""
    u0 = np.asarray(u0, dtype=np.float64)
    u1 = np.asarray(u1, dtype=np.float64)
    r = np.sqrt(LD(-2) * np.log(u0.astype(LD)))
    r = np.where(u0 == 1.0, LD(0), r)              # log 1 = 0 exactly; no -0 from the product
    m = (u1 * np.float64(2.0 ** 54)).astype(np.int64)
    assert np.array_equal(m.astype(np.float64) * 2.0 ** -54, u1), "u1 is not a multiple of 2^-54"
    q = (m + (np.int64(1) << np.int64(51))) >> np.int64(52)
    rem = m - (q << np.int64(52))
    a = rem.astype(LD) * LD(2.0 ** -53) * PI
    s, c = np.sin(a), np.cos(a)
    q = q & 3
    cs = np.choose(q, [c, -s, -c, s])
    sn = np.choose(q, [s, c, -s, -c])
    return r * cs, r * sn


def normals(seed, frames, blocks, stream, variant=None):
    """(z0, z1) long double [B][nb]: the two normals of every (frame, block).  variant (for the tests that show that the
    tolerance bites): "swap_cs" (cos and sin exchanged), "swap_u" (u0 and u1 exchanged), "stream" (stream 1 <-> 2)."""
    if variant == "stream":
        stream = {STREAM_NOISE: STREAM_ROWS, STREAM_ROWS: STREAM_NOISE}[stream]
    c = frame_block(seed, frames, blocks, stream)
    u0, u1 = uniform(k53(c[0], c[1])), uniform(k53(c[2], c[3]))
    if variant == "swap_u":
        u0, u1 = u1, u0
    z0, z1 = box_muller(u0, u1)
    return (z1, z0) if variant == "swap_cs" else (z0, z1)


# ---- the bits ----------------------------------------------------------------------------------------------------------------
def payload(seed, frames, K):
    """v [B][K]: bit b of word w is payload bit 32 w + b"""
    kw = (K + 31) // 32
    words = frame_block(seed, frames, np.arange(kw), STREAM_PAYLOAD)[0]
    bits = (words[:, :, None] >> np.arange(32, dtype=U64)[None, None, :]) & U64(1)
    return bits.reshape(len(words), kw * 32)[:, :K].astype(np.uint8)


def crc_multiply(v, taps):
    """w(D) = v(D) g(D): K + r bits"""
    K, r = v.shape[1], max(taps)
    w = np.zeros((v.shape[0], K + r), dtype=np.uint8)
    for t in taps:
        w[:, t:t + K] ^= v
    return w


def crc_systematic(v, taps):
    """w[0..r) = v(D) D^r mod g(D) (by long division), w[r..K+r) = v: a multiple of g(D) that carries the payload"""
    K, r = v.shape[1], max(taps)
    rem = np.concatenate([np.zeros((v.shape[0], r), dtype=np.uint8), v], axis=1)
    for i in range(K + r - 1, r - 1, -1):
        rows = rem[:, i] == 1
        for t in taps:
            rem[rows, i - r + t] ^= 1
    return np.concatenate([rem[:, :r], v], axis=1)


def crc_systematic_matrix(v, Gc):
    """the same from a generator matrix Gc [K][r] (the layout of the reference's CRC_6.dat): w[0..r) = v Gc"""
    par = (v.astype(np.int64) @ np.asarray(Gc, dtype=np.int64)) & 1
    return np.concatenate([par.astype(np.uint8), v], axis=1)


def encode(u):
    """x = u F^{(x)n}, natural order"""
    x = np.array(u, dtype=np.uint8)
    N, h = x.shape[1], 1
    while h < N:
        t = x.reshape(x.shape[0], N // (2 * h), 2, h)
        t[:, :, 0, :] ^= t[:, :, 1, :]
        h *= 2
    return x


def u_rows(seed, frames, N, K, info_order, taps=None, systematic=False, Gc=None, sys_polar=False, dyn=None):
    """u [B][N] as polar_generate_device reports it in d_u_bits"""
    v = payload(seed, frames, K)
    if Gc is not None:
        w = crc_systematic_matrix(v, Gc)
    elif taps and systematic:
        w = crc_systematic(v, taps)
    elif taps:
        w = crc_multiply(v, taps)
    else:
        w = v
    io = np.asarray(info_order, dtype=np.int64)
    assert w.shape[1] == io.size
    u = np.zeros((v.shape[0], N), dtype=np.uint8)
    u[:, io] = w
    if sys_polar:
        frozen = np.ones(N, dtype=bool)
        frozen[io] = False
        u = encode(u)
        u[:, frozen] = 0
    if dyn is not None:
        u = DYN.fill_dynamic(u.astype(np.int64), dyn).astype(np.uint8)
    return u


# ---- the channel -------------------------------------------------------------------------------------------------------------
def sigma_of(snr_db):
    """sigma = 10^(-snr_db / 20), the library's expression in binary64"""
    return float(10.0 ** (float(snr_db) / -20.0))


def element_map(kind, n):
    """(block [n], normal [n], stream) of the n elements of a row: kind "plain" (k_generate, k_generate_dyn) or "rows"
    (k_generate_rm's sent positions, k_genie_rows)"""
    j = np.arange(n)
    if kind == "plain":
        return (j & 63) + 64 * (j >> 7), (j >> 6) & 1, STREAM_NOISE
    assert kind == "rows"
    return j >> 1, j & 1, STREAM_ROWS


def noise(seed, frames, kind, n, variant=None):
    """z [B][n] long double: the normal of every element"""
    blk, nrm, stream = element_map(kind, n)
    ub, inv = np.unique(blk, return_inverse=True)
    z0, z1 = normals(seed, frames, ub, stream, variant)
    return np.where(nrm[None, :] == 0, z0[:, inv], z1[:, inv])


def channel(bits, z, sigma, out_is_y):
    """(ref, bound) long double [B][n]: the value of every element, y = (1 - 2 bit) + sigma z or 2 * y / sigma / sigma, and the
    largest error a binary64 evaluation may make in it (f64_bound)"""
    s = LD(sigma)
    y = (LD(1) - LD(2) * bits.astype(LD)) + s * z
    ref = y if out_is_y else LD(2) * y / s / s
    return ref, f64_bound(np.abs(s * z), np.abs(y), sigma, out_is_y)


# per-operation error of the device's binary64 functions, in ulp.  ROCm ships no accuracy table for the HIP math functions on
# the test machines, so these are ASSUMED ("Generator values"): log and sincospi 2 ulp, sqrt 1 ulp; the basic
# operations (multiply, add, divide; no contraction: the library is built with -ffp-contract=off) are correctly rounded.
ULP_LOG, ULP_SINCOSPI, ULP_SQRT, MARGIN = 2.0, 2.0, 1.0, 2.0


def f64_bound(sz, ay, sigma, out_is_y):
    """|device - exact| allowed for an element with sigma |z| = sz and |y| = ay, to first order in EPS = 2^-52:
       r = sqrt(-2 log u0):  log contributes ULP_LOG, halved by the root; the root ULP_SQRT          -> (ULP_LOG / 2 + ULP_SQRT) EPS
       z = r * cs:           + ULP_SINCOSPI for cs, + 1/2 for the product                           -> relative error of z
       sigma * z:            + 1/2                                                                  -> relative error of sigma z
       y = +-1 + sigma z:    absolute error of sigma z, + 1/2 ulp of y
       2 * y / sigma / sigma: the doubling is exact, each division adds 1/2 ulp of the quotient
    times MARGIN.  A function of the model's own quantities only."""
    rel_sz = (ULP_LOG / 2 + ULP_SQRT + ULP_SINCOSPI + 0.5 + 0.5) * EPS
    by = rel_sz * sz + 0.5 * EPS * ay
    if out_is_y:
        return MARGIN * by
    s = LD(sigma)
    return MARGIN * (LD(2) * by / s / s + 2 * 0.5 * EPS * (LD(2) * ay / s / s))


def f32_check(got, ref, bound):
    """got float32 [..] against the long double values: (within, exact_needed, exact_ok) -- within: |got - float32(ref)| <= 1
    ulp32 (got is float32(ref) or one of its two neighbours); exact_needed: ref lies further than `bound` from both rounding
    midpoints next to float32(ref), so that any binary64 value within the bound rounds to float32(ref); exact_ok: got equals it"""
    got = np.asarray(got, dtype=np.float32)
    r32 = ref.astype(np.float32)
    lo, hi = np.nextafter(r32, np.float32(-np.inf)), np.nextafter(r32, np.float32(np.inf))
    within = (got == r32) | (got == lo) | (got == hi)
    m_lo, m_hi = (r32.astype(LD) + lo.astype(LD)) / 2, (r32.astype(LD) + hi.astype(LD)) / 2
    dist = np.minimum(ref - m_lo, m_hi - ref)
    return within, dist > bound, got == r32
