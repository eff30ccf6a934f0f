"""CPU: the numpy model of the device-side transmit chain (tests/gen_model.py) against what it must itself be held to --
the Random123 known-answer vectors of philox4x32-10, mpmath at 120 bits for the Box-Muller, the binary64 edge cases of the
uniforms, and model variants (cos / sin swapped, u0 / u1 swapped, stream 1 <-> 2, one constant off by one) that must differ
from the model by far more than the tolerance tests/test_gpu_generator_values.py grants the kernels."""
import numpy as np
import pytest

import gen_model as G

LD = np.longdouble


def _hex(words):
    return " ".join(f"{int(np.asarray(w).ravel()[0]):08x}" for w in words)


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert _hex(G.philox4x32_10(counter, key)) == want


def test_philox_is_vectorised_and_frame_block_maps_the_counter():
    """frame_block(seed, frame, block, stream) is counter (frame lo, frame hi, block, stream), key (seed lo, seed hi)"""
    seed, frames, blocks = 0x299f31d0a4093822, [0x85a308d3243f6a88, 5, 2 ** 32 - 1, 2 ** 32], [0x13198a2e, 0, 7]
    c = G.frame_block(seed, frames, blocks, 0x03707344)
    assert c[0].shape == (4, 3)
    assert _hex([w[0, 0] for w in c]) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    for i, f in enumerate(frames):
        for j, b in enumerate(blocks):
            one = G.philox4x32_10((f & 0xffffffff, f >> 32, b, 0x03707344), (0xa4093822, 0x299f31d0))
            assert [int(w[i, j]) for w in c] == [int(np.asarray(w).ravel()[0]) for w in one]
    # the high word of the frame and of the seed reach the generator
    lo = G.frame_block(seed & 0xffffffff, frames, blocks, 1)
    assert not np.array_equal(lo[0], G.frame_block(seed, frames, blocks, 1)[0])
    assert not np.array_equal(G.frame_block(7, [2 ** 32 + 5], [0], 1)[0], G.frame_block(7, [5], [0], 1)[0])
    assert G.frames_of(2 ** 32 - 3, 8).tolist() == [2 ** 32 - 3 + i for i in range(8)]


def test_uniform_edges():
    """(double(k) + 0.5) 2^-53: exact below 2^52, round-to-even above: (0, 1], 1.0 included, 0 excluded"""
    k = np.array([0, 1, 2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 53 - 2, 2 ** 53 - 1], dtype=np.uint64)
    u = G.uniform(k)
    assert u.dtype == np.float64
    assert u[0] == 2.0 ** -54 and u[1] == 1.5 * 2.0 ** -53
    assert u[2] == (2.0 ** 52 - 0.5) * 2.0 ** -53                       # still exact: 2^52 - 1/2 has 53 bits
    assert u[3] == 0.5 and u[4] == (2.0 ** 52 + 2) * 2.0 ** -53         # k + 1/2 ties to the even neighbour
    assert u[5] == (2.0 ** 53 - 2) * 2.0 ** -53 and u[6] == 1.0
    assert (u > 0).all() and (u <= 1).all()
    assert int(G.k53(0xffffffff, 0xffffffff)) == 2 ** 53 - 1 and int(G.k53(0, 0x7ff)) == 0 and int(G.k53(0, 0x800)) == 1
    assert int(G.k53(0x80000000, 0)) == 2 ** 52
    # u0 = 1 gives z = 0; the smallest u0 gives the largest radius, below Z_MAX
    z0, z1 = G.box_muller(np.array([1.0, 2.0 ** -54]), np.array([0.25, 1.0]))
    assert z0[0] == 0 and z1[0] == 0
    assert float(z0[1]) == pytest.approx(G.Z_MAX, rel=1e-15) and z1[1] == 0
    assert G.Z_MAX == pytest.approx(8.6522, abs=1e-4)


def _forced_k1():
    ks = [0, 1, 2 ** 53 - 2, 2 ** 53 - 1]
    for q in range(1, 8):                      # every eighth of a turn: the zeros of cos and sin, and the quadrant seams
        for d in (-2, -1, 0, 1):
            ks.append(q * 2 ** 50 + d)
    return ks


def test_box_muller_against_mpmath():
    """both normals to a relative 2^-60 against mpmath at 120 bits, on random operands and on the forced ones: k1 at and next
    to every quarter (and eighth) turn, k0 at both ends"""
    import mpmath as mp
    mp.mp.prec = 120
    rng = np.random.default_rng(2026)
    k0 = rng.integers(0, 2 ** 53, 300).tolist()
    k1 = rng.integers(0, 2 ** 53, 300).tolist()
    forced1, forced0 = _forced_k1(), [0, 1, 2 ** 53 - 2, 2 ** 53 - 1]
    for a in forced0 + k0[:6]:
        for b in forced1:
            k0.append(a)
            k1.append(b)
    for a in forced0:
        for b in k1[:6]:
            k0.append(a)
            k1.append(b)
    u0 = G.uniform(np.array(k0, dtype=np.uint64))
    u1 = G.uniform(np.array(k1, dtype=np.uint64))
    z0, z1 = G.box_muller(u0, u1)
    assert np.abs(z0).max() <= G.Z_MAX and np.abs(z1).max() <= G.Z_MAX
    worst = 0.0
    for i in range(len(k0)):
        a, b = mp.mpf(float(u0[i])), mp.mpf(float(u1[i]))      # the binary64 uniforms, exactly
        r = mp.sqrt(-2 * mp.log(a))
        for got, want in ((z0[i], r * mp.cospi(2 * b)), (z1[i], r * mp.sinpi(2 * b))):
            g = mp.mpf(float(got))                            # long double -> mpmath exactly, in two binary64 pieces
            g += mp.mpf(float(got - LD(float(got))))
            if want == 0:
                assert g == 0, (k0[i], k1[i])
                continue
            err = abs((g - want) / want)
            worst = max(worst, float(err))
            assert err <= mp.mpf(2) ** -60, (k0[i], k1[i], float(err))
    print(f"box_muller vs mpmath: worst relative error 2^{np.log2(worst):.1f} over {len(k0)} pairs")


def test_pi_is_long_double_pi():
    import mpmath as mp
    mp.mp.prec = 120
    g = mp.mpf(float(G.PI)) + mp.mpf(float(G.PI - LD(float(G.PI))))
    assert abs(g - mp.pi) / mp.pi < mp.mpf(2) ** -64
    assert abs(mp.mpf(float(np.pi)) - mp.pi) / mp.pi > mp.mpf(2) ** -56      # what a float literal would have given


def test_element_maps():
    """k_generate's lane layout (lane l holds elements l + 64 k; one block per pair of a lane's elements), written out for N = 256,
    and the pair rule of the rate-matched and design rows; no (block, normal) is used twice in a row"""
    blk, nrm, st = G.element_map("plain", 256)
    assert st == 1
    assert blk[:64].tolist() == list(range(64)) and blk[64:128].tolist() == list(range(64))
    assert blk[128:192].tolist() == list(range(64, 128)) and blk[192:].tolist() == list(range(64, 128))
    assert nrm[:64].tolist() == [0] * 64 and nrm[64:128].tolist() == [1] * 64 and nrm[128:192].tolist() == [0] * 64
    for n in (64, 128, 1024, 4096):
        blk, nrm, _ = G.element_map("plain", n)
        assert len(set(zip(blk.tolist(), nrm.tolist()))) == n
        assert blk.max() == max(n // 2, 64) - 1
    blk, nrm, _ = G.element_map("plain", 64)
    assert not nrm.any()                                       # N = 64: the second normal of every block is unused
    blk, nrm, st = G.element_map("rows", 7)
    assert st == 2 and blk.tolist() == [0, 0, 1, 1, 2, 2, 3] and nrm.tolist() == [0, 1, 0, 1, 0, 1, 0]


def test_payload_and_crc_models():
    seed, frames = 0x1234567890, G.frames_of(2 ** 32 - 2, 4)
    for K in (20, 64, 65):
        v = G.payload(seed, frames, K)
        assert v.shape == (4, K)
        full = G.payload(seed, frames, ((K + 31) // 32) * 32)
        assert np.array_equal(v, full[:, :K])                  # the last word is masked, not redrawn
        w0 = int(G.frame_block(seed, frames[:1], [0], 0)[0][0, 0])
        assert v[0, :min(K, 32)].tolist() == [(w0 >> b) & 1 for b in range(min(K, 32))]
        for taps in ((0, 5, 6), (0, 1, 2, 4, 5, 7, 8, 10, 11, 12, 16, 22, 23, 26, 32)):
            r = max(taps)
            ws = G.crc_systematic(v, taps)
            assert np.array_equal(ws[:, r:], v)
            # both words are multiples of g(D): the remainder of the long division is zero
            for w in (ws, G.crc_multiply(v, taps)):
                rem = w.copy()
                for i in range(K + r - 1, r - 1, -1):
                    rows = rem[:, i] == 1
                    for t in taps:
                        rem[rows, i - r + t] ^= 1
                assert not rem.any()
            # the generator-matrix form with rows D^(r+k) mod g is the same word
            Gc = G.crc_systematic(np.eye(K, dtype=np.uint8), taps)[:, :r]
            assert np.array_equal(G.crc_systematic_matrix(v, Gc), ws)


def test_sys_polar_and_dynamic_rows():
    N, K = 64, 20
    io = np.arange(N - K, N)                                   # a set for which the two-pass systematic encoder is valid
    frames = G.frames_of(0, 6)
    z = G.u_rows(3, frames, N, K, io)
    u = G.u_rows(3, frames, N, K, io, sys_polar=True)
    assert not u[:, :N - K].any()
    assert np.array_equal(G.encode(u)[:, io], z[:, io])       # x = u F carries the placed row on the information set
    dyn = (np.array([3, 50]), [np.array([], dtype=np.int32), np.array([44, 45, 49])])
    io2 = np.array([j for j in range(N - K - 1, N) if j != 50])
    ud = G.u_rows(3, frames, N, K, io2, dyn=dyn)
    assert not ud[:, 3].any() and np.array_equal(ud[:, 50], ud[:, 44] ^ ud[:, 45] ^ ud[:, 49])


@pytest.mark.parametrize("out_is_y", [True, False])
@pytest.mark.parametrize("sigma", [1.0, G.sigma_of(1.5), G.sigma_of(-3.0)])
def test_variants_differ_by_far_more_than_the_tolerance(sigma, out_is_y):
    """cos / sin swapped, u0 / u1 swapped and stream 1 <-> 2 move nearly every element by more than 10^6 times the f64 bound
    (and by far more than one f32 ulp), for both element maps; so does one Philox multiplier off by one or nine rounds"""
    frames = G.frames_of(2 ** 40 + 1, 4)
    for kind, n in (("plain", 256), ("rows", 255)):
        bits = np.zeros((4, n), dtype=np.uint8)
        ref, bound = G.channel(bits, G.noise(11, frames, kind, n), sigma, out_is_y)
        assert (bound > 0).all() and (bound < 1e-13 * (1 + np.abs(ref))).all()
        for variant in ("swap_cs", "swap_u", "stream"):
            other, _ = G.channel(bits, G.noise(11, frames, kind, n, variant), sigma, out_is_y)
            far = np.abs(other - ref) > 1e6 * bound
            assert far.mean() > 0.99, (kind, variant, float(far.mean()))
            assert (np.abs(other - ref) > 4 * np.abs(ref) * 2.0 ** -23).mean() > 0.99
    a = G.frame_block(11, frames, np.arange(8), 1)
    for kw in (dict(m0=G.PHILOX_M0 + np.uint64(1)), dict(rounds=9)):
        b = G.frame_block(11, frames, np.arange(8), 1, **kw)
        assert (a[0] != b[0]).all() and (a[2] != b[2]).all()


def test_f32_check_rules():
    """float32(ref) and its neighbours pass `within`; equality is demanded away from the midpoints only"""
    ref = np.array([LD(1) + LD(2.0 ** -24) + LD(2.0 ** -60), LD(1.25), LD(-3) - LD(2.0 ** -30)])
    bound = np.full(3, LD(2.0 ** -50))
    r32 = ref.astype(np.float32)
    within, need, ok = G.f32_check(r32, ref, bound)
    assert within.all() and ok.all() and need.tolist() == [False, True, True]
    up = np.nextafter(r32, np.float32(np.inf))
    within, need, ok = G.f32_check(up, ref, bound)
    assert within.all() and not ok.any()
    within, _, _ = G.f32_check(np.nextafter(up, np.float32(np.inf)), ref, bound)
    assert not within.any()


def test_bound_is_a_function_of_the_models_quantities():
    """the propagated bound, written out once by hand: sigma |z| = 2, |y| = 3, sigma = 0.5"""
    e = 2.0 ** -52
    by = (1 + 1 + 2 + 0.5 + 0.5) * e * 2 + 0.5 * e * 3
    assert float(G.f64_bound(LD(2), LD(3), 0.5, True)) == pytest.approx(2 * by, rel=1e-12)
    assert float(G.f64_bound(LD(2), LD(3), 0.5, False)) == pytest.approx(2 * (8 * by + e * 24), rel=1e-12)
