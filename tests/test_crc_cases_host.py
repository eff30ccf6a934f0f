"""CPU: the conditions tests/test_gpu_crc_cases.py relies on, for every case of tests/crc_cases.py, from the references alone.

Per frame i of a case: crc_tab[I[i]] = 1 << i, the syndrome of u' is exactly 1 << i and that of u is 0, the plain list
decoder's best path on the weak row is u', and SC returns u' on the plain row wherever a kernel's first pass is SC.  Per
case: CA-SCL returns the sent word in at least half of the frames, and every polynomial with r >= 11 has a frame in which no
path of the list passes (there the reference returns u' with POLAR_FLAG_CRC_PASS clear).  Then the encoder model of
tests/test_encode_host.py against bit-serial long division for every polynomial of the family, r = 32 included."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import crc_cases as CC  # noqa: E402
import test_encode_host as E  # noqa: E402
from test_cascl_adaptive_host import crc_table, syndrome  # noqa: E402

WEAK = sorted(CC.weak_shapes().items())
PLAIN = sorted(CC.plain_shapes().items())


def _bits_of_frames(r):
    return np.uint64(1) << np.arange(r, dtype=np.uint64)


def _frame_conditions(u, uf, info, taps):
    r = max(taps)
    tab = crc_table(u.shape[1], info, taps)
    assert [int(tab[int(j)]) for j in info[:r]] == [1 << i for i in range(r)]
    assert not syndrome(u, info, taps).any()
    assert np.array_equal(syndrome(uf, info, taps), _bits_of_frames(r))
    assert ((u != uf).sum(axis=1) >= 1).all()


@pytest.mark.parametrize("shape,rs", WEAK, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_weak_rows(shape, rs, oracle):
    """Observed with SEED = 1 -- frames where CA-SCL returns u / frames where no path passes, of r:
    (32, 15, 2): r=1 1/0, r=6 5/1, r=11 10/1.  (64, 20, 8): r=1..16 all/0, r=24 22/2, r=25 23/2, r=31 20/11, r=32 20/12.
    (64, 20, 64): r=6 6/0, r=32 30/2.  (128, 33, 8): r=1..16 all/0, r=24 23/1, r=25 24/1, r=31 29/2, r=32 30/2.
    (512, 200, 2): r=6 5/1, r=25 23/2, r=32 29/3.  (512, 200, 32): r=6 6/0, r=25 24/1, r=32 30/2.
    (1024, 480, 8): r=1 1/0, r=6 6/0, r=11 10/1, r=16 12/4, r=24 19/5, r=25 20/5, r=31 23/8, r=32 24/8.
    (1024, 480, 32): r=6 6/0, r=25 22/3, r=32 24/8."""
    N, K, L = shape
    for r in sorted(rs):
        code = CC.code_of(N, K, r)
        u, uf, plain, weak = CC.frames(N, K, r)
        assert len(u) == r
        _frame_conditions(u, uf, code.info_order, code.taps)
        assert np.array_equal(weak.astype(np.float32).astype(np.float64), weak) and set(np.abs(weak).ravel()) <= {CC.HI, CC.LO}
        assert np.array_equal(np.sign(weak), np.sign(plain)) and (np.abs(plain) == CC.HI).all()
        assert np.array_equal(CC.y_of(weak) * 8.0, weak)
        scl = CC.ref_list(N, K, r, L, algo="SCL")[0]
        assert np.array_equal(scl, uf), (shape, r, "plain SCL's best path is not the flipped word")
        ca, _, fl, _ = CC.ref_list(N, K, r, L)
        is_u = (ca == u).all(axis=1)
        passed = (fl & CC.FLAG_CRC_PASS) != 0
        print(f"N={N} K={K} L={L} r={r}: CA-SCL returns u in {is_u.sum()} of {r} frames, no path passes in {(~passed).sum()}")
        assert 2 * is_u.sum() >= r, (shape, r)
        assert np.array_equal(is_u, passed)                         # a passing path is the sent word, in every frame
        assert (ca[~passed] == uf[~passed]).all()                   # and where none passes the reference returns u'


def test_the_family_reaches_every_row_count_of_the_pair_kernels_mask_loop():
    assert {r: (r + 3) & ~3 for r in CC.ALL_R} == CC.FAST2_ROWS
    assert sorted(CC.FAST2_ROWS.values()) == [4, 8, 12, 16, 24, 28, 32, 32]
    assert all(max(t) == r and t[0] == 0 and list(t) == sorted(set(t)) for r, t in CC.POLYS.items())


@pytest.mark.parametrize("r", [r for r in CC.ALL_R if r >= 11])
def test_every_long_polynomial_has_a_frame_where_no_path_passes(r, oracle):
    n = 0
    for (N, K, L), rs in WEAK:
        if r in rs:
            n += int(((CC.ref_list(N, K, r, L)[2] & CC.FLAG_CRC_PASS) == 0).sum())
    assert n >= 1, r


@pytest.mark.parametrize("shape,rs", PLAIN, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_plain_rows(shape, rs, oracle):
    """SC over I[0 .. K+r) returns the flipped word on the plain row, in every frame: attempt 0 of SC-Flip and stage 1 of
    adaptive CA-SCL fail the CRC in bit i alone"""
    N, K = shape
    for r in sorted(rs):
        code = CC.code_of(N, K, r)
        u, uf, plain, _ = CC.frames(N, K, r)
        _frame_conditions(u, uf, code.info_order, code.taps)
        assert np.array_equal(CC.ref_sc(N, K, r), uf), (shape, r)


@pytest.mark.parametrize("r", CC.SCF_RS)
def test_flip_decoders_fail_attempt_zero(r, oracle):
    """Attempt 0 fails in every frame.  All magnitudes of a plain row are equal, so many |lambda| tie and the flip list goes
    to the smaller positions: the models recover few frames (observed, static T = 4 / dynamic (2, 2): r = 6: 3 / 2 of 6,
    r = 16: 1 / 1 of 16, r = 32: 0 / 0 of 32).  Every further attempt is one more word whose remainder the kernel has to find
    non-zero, or zero, exactly where the model does."""
    N, K = CC.SCF_N, CC.SCF_K
    u, uf, _, _ = CC.frames(N, K, r)
    uh, fl, at, flips, fail = CC.ref_scf(N, K, r, CC.SCF_T)
    assert len(fail) == r and (at >= 1).all()
    ok = (fl & CC.FLAG_CRC_PASS) != 0
    print(f"SC-Flip N={N} r={r}: {ok.sum()} of {r} frames recovered, attempts {np.unique(at)}")
    assert np.array_equal(uh[ok], u[ok]) and np.array_equal(uh[~ok], uf[~ok])
    res = CC.ref_dscf(N, K, r, CC.SCF_BUDGETS)
    ok = (res.flags & CC.FLAG_CRC_PASS) != 0
    print(f"dynamic SC-Flip N={N} r={r}: {ok.sum()} of {r} frames recovered, attempts {np.unique(res.attempts)}")
    assert (res.attempts >= 1).all()


@pytest.mark.parametrize("r", CC.DYN_RS)
def test_dynamic_code_weak_rows(r, oracle):
    """Observed: the model returns u in 11 of 11 (r = 11), 23 of 24 (r = 24) and 29 of 32 (r = 32) frames"""
    io, dyn, frozen = CC.dyn_code(r)
    u, uf, plain, weak = CC.dyn_frames(r)
    _frame_conditions(u, uf, io, CC.POLYS[r])
    pos, sets = dyn
    for w in (u, uf):   # both are words of the code without its CRC
        for d, j in enumerate(pos):
            assert np.array_equal(w[:, j], w[:, np.asarray(sets[d], dtype=np.int64)].sum(axis=1) & 1 if len(sets[d]) else 0 * w[:, j])
    assert np.array_equal(CC.ref_dyn(r, crc=False)[0], uf)
    ca, _, fl = CC.ref_dyn(r)
    is_u = (ca == u).all(axis=1)
    print(f"PC-CA-SCL N=128 r={r}: the model returns u in {is_u.sum()} of {r} frames")
    assert 2 * is_u.sum() >= r and np.array_equal(is_u, (fl & CC.FLAG_CRC_PASS) != 0)


@pytest.mark.parametrize("N,K,L", CC.Q8_SHAPES)
def test_q8_weak_rows(N, K, L, oracle):
    """the int8 rows +-16 / +-2 under q8_model: the list decoder without a CRC returns u', with it u in at least half of the
    frames.  Observed: (64, 20): 6/6, 22/24, 23/32; (128, 33): 6/6, 24/24, 31/32"""
    import q8_model
    for r in CC.Q8_RS:
        code = CC.code_of(N, K, r)
        u, uf, _, weak = CC.frames(N, K, r)
        q = CC.q8_of(weak)
        assert set(np.abs(q.astype(int)).ravel()) <= {CC.Q8_HI, CC.Q8_LO} and np.array_equal(q < 0, weak < 0)
        scl = np.stack([q8_model.decode(row, code.frozen, L)[0] for row in q])
        assert np.array_equal(scl, uf), (N, r)
        ca, _, fl = CC.ref_q8(N, K, r, L)
        is_u = (ca == u).all(axis=1)
        print(f"q8 N={N} r={r}: the model returns u in {is_u.sum()} of {r} frames")
        assert 2 * is_u.sum() >= r and np.array_equal(is_u, (fl & CC.FLAG_CRC_PASS) != 0)


@pytest.mark.parametrize("N,K,L", CC.PATHS_SHAPES)
def test_the_list_holds_the_flipped_word_with_its_one_bit_remainder(N, K, L, oracle):
    import list_model
    for r in CC.fits(N, K):
        u, uf, _, _ = CC.frames(N, K, r)
        paths, pm, rem, count, flags = CC.ref_all_paths(N, K, r, L)
        assert np.array_equal(paths[:, 0], uf) and np.array_equal(rem[:, 0].astype(np.uint64), _bits_of_frames(r))
        idx = list_model.select(rem, count, np.array([0], dtype=np.uint32))[:, 0]
        has = idx >= 0
        assert 2 * has.sum() >= r and np.array_equal(paths[has, idx[has]], u[has])


def test_bpl_case(oracle):
    """attempt 0 converges to u' (the noise-free word) and fails the CRC in every frame.  Observed: no later graph finds a
    word that passes, the frames end with graph = P"""
    N, K, r, iters, P = CC.BPL_CASE
    u, uf, _, _ = CC.frames(N, K, r)
    res = CC.ref_bpl(N, K, r, iters, P)
    a0 = res.attempts[0]
    assert a0["conv"].all() and not a0["crcok"].any() and np.array_equal(a0["u_hat"], uf)
    print(f"BPL: graphs {np.unique(res.graph)}, flags {np.unique(res.flags)}")


# ---- the encoder model against bit-serial long division --------------------------------------------------------------------
@pytest.mark.parametrize("crc_sys", [False, True], ids=["plain", "syscrc"])
@pytest.mark.parametrize("r", CC.ALL_R)
def test_encoder_model_is_long_division(r, crc_sys):
    taps = CC.POLYS[r]
    rng = np.random.default_rng(r)
    for K in (1, 5, 31, 32, 33, 64, 97):
        v = rng.integers(0, 2, (6, K)).astype(np.uint8)
        v[0] = 1
        w = E.crc_word(v, taps, crc_sys)
        assert w.shape == (6, K + r)
        for b in range(6):
            quo, rem = CC.long_division(w[b], taps)
            assert not any(rem)
            if crc_sys:   # (D^r v mod g, v): the remainder of D^r v(D) is the low part
                assert list(w[b, r:]) == list(v[b])
                assert CC.long_division([0] * r + list(v[b]), taps)[1] == list(w[b, :r])
            else:
                assert quo == list(v[b])
        # extract on arbitrary words: quotient, remainder and verdict
        N = 256
        info = CC.enc_info(N, K + r)
        z = np.zeros((6, N), dtype=np.uint8)
        z[:, info] = rng.integers(0, 2, (6, K + r))
        z[0, info] = w[0]
        pay, ok = E.extract(z, info, taps, crc_sys)
        for b in range(6):
            quo, rem = CC.long_division(z[b, info], taps)
            assert int(ok[b]) == int(not any(rem))
            assert list(pay[b]) == (list(z[b, info[r:]]) if crc_sys else quo)
        assert ok[0] == 1
        assert np.array_equal(E.place(v, N, info, taps, crc_sys)[:, info], w)


def test_encoder_cases_cover_what_they_are_there_for():
    cases = CC.enc_cases()
    assert {r for r, _, _, _ in cases} == set(CC.ALL_R)
    assert any(K + r == N for r, N, K, _ in cases) and any(K < r for r, N, K, _ in cases)
    assert any(K % 32 == 0 and r == 32 for r, N, K, _ in cases) and (32, 4096, 2048, True) in cases
    assert all(1 <= K and K + r <= N for r, N, K, _ in cases)
