"""CPU: BP list decoding over permuted factor graphs (POLAR_ALGO_BPL, include/polar_hip.h).

The numpy model of tests/bpl_model.py is held to the CPU oracle here: an attempt on graph pi is the oracle's BP on the code
whose reliability order is the 5G order mapped through sigma_pi^-1, fed with the permuted row.  The oracle knows nothing of
sigma, so this pins the direction of the permutation.  tests/test_gpu_bpl.py then holds the library to the model.  Also the
host helpers and the C ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bpl_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _frames(oracle, code, seed, per=12, dbs=(1.0, 2.0, 3.0)):
    out = []
    for k, db in enumerate(dbs):
        sim = oracle.Sim(seed + k)
        sig = oracle.sigma_from_db(db)
        _, ys = sim.frames(code, sig, per)
        out += [oracle.llr_from_y(y, sig) for y in ys]
    return np.stack(out)


@pytest.mark.parametrize("N,K", [(128, 64), (256, 128)])
def test_model_attempts_equal_the_oracle_on_the_permuted_code(N, K, oracle):
    """Every frame of a 36-frame set (1 .. 3 dB), on the identity, the reversal and two cyclic shifts: the model's attempt,
    un-permuted, is the oracle's BP with bp_iters = t_p on Code(N, K, Q = sigma_p^-1(5G order)) and the permuted row."""
    n = N.bit_length() - 1
    code = oracle.Code(N, K)
    llr = _frames(oracle, code, 900 + N)
    assert llr.shape[0] == 36
    q = np.asarray(oracle.q_for(N))
    for pi in (list(range(n)), list(range(n))[::-1], [(b + 1) % n for b in range(n)], [(b + 3) % n for b in range(n)]):
        s = M.sigma(pi, N)
        sinv = np.argsort(s)
        permuted = oracle.Code(N, K, Q=sinv[q])
        assert np.array_equal(permuted.frozen, code.frozen[s])
        res = M.bpl_decode(llr, code.frozen, code.info_order, [pi], 30)
        att = res.attempts[0]
        assert np.array_equal(att["frames"], np.arange(36))
        for b in range(36):
            ref, _, _ = oracle.decode(permuted, att["row"][b], "BP", bp_iters=int(att["t"][b]))
            un = np.zeros(N, dtype=np.int32)
            un[s] = ref
            assert np.array_equal(res.bits[b], un), (pi, b)
        assert att["conv"].sum() >= 12   # most of the 2 and 3 dB frames settle: the stop points are not all iterMax


def test_sigma_is_a_bijection_that_commutes_with_the_encoder():
    """sigma_pi permutes 0 .. N-1, and encode(u)[sigma] == encode(u[sigma]): permuting the index bits of the positions maps
    codewords to codewords, which is what makes an attempt on a permuted row a decoder of the same code."""
    rng = np.random.default_rng(11)
    for N in (32, 128, 1024):
        n = N.bit_length() - 1
        for _ in range(6):
            pi = rng.permutation(n)
            s = M.sigma(pi, N)
            assert np.array_equal(np.sort(s), np.arange(N))
            u = rng.integers(0, 2, (5, N)).astype(np.int32)
            assert np.array_equal(M.encode(u)[:, s], M.encode(u[:, s]))
    assert np.array_equal(M.sigma([1, 2, 0, 3, 4], 32)[:9], [0, 2, 4, 6, 1, 3, 5, 7, 8])   # bit 0 -> 1, 1 -> 2, 2 -> 0


def test_crc_division_is_the_table_of_the_list_kernels():
    """w(D) mod g(D) by long division == XOR of crc_tab[I[i]] = D^i mod g over the set bits (the header's rule 3)."""
    taps, r, A = (0, 5, 6), 6, 70
    rng = np.random.default_rng(5)
    info = rng.permutation(128)[:A]
    tab, rem = {}, 1
    for i in range(A):
        tab[int(info[i])] = rem
        rem <<= 1
        if rem >> r & 1:
            rem ^= sum(1 << t for t in taps)
    u = rng.integers(0, 2, (300, 128)).astype(np.int32)
    u[:, np.setdiff1d(np.arange(128), info)] = 0
    u[0] = 0
    want = np.array([np.bitwise_xor.reduce([tab[j] for j in np.flatnonzero(row)] + [0]) == 0 for row in u])
    assert np.array_equal(M.crc_remainder_is_zero(u, info, taps), want)
    assert want[0] and 1 <= want.sum() < 60


def test_cyclic_graphs_and_refusals_without_a_context():
    import polardecoding_amd as pa
    lib = pa.load_library()
    for n, P in ((5, 1), (7, 7), (10, 8), (12, 32)):
        g = pa.bpl_cyclic_graphs(n, P)
        assert g.shape == (P, n) and g.dtype == np.int32
        assert np.array_equal(g, np.asarray(M.cyclic_graphs(n, P)))
    buf = (C.c_int * (32 * 12))()
    for n, P in ((4, 1), (13, 1), (7, 0), (7, 33)):
        assert lib.polar_bpl_cyclic_graphs(n, P, buf) == EINVAL, (n, P)
    assert lib.polar_bpl_cyclic_graphs(7, 4, None) == EINVAL
    # no context: every polar_bpl_* entry point that takes one refuses (the refusals on live contexts: test_gpu_bpl.py)
    ident = (C.c_int * 7)(*range(7))
    for P in (0, 1, 33):
        assert lib.polar_bpl_set_graphs(None, ident, P) == EINVAL
    assert lib.polar_bpl_get_graphs(None, None, None) == EINVAL
    assert lib.polar_bpl_decode_device(None, None, 0, 0.0, 0, None, None, None, None, None) == EINVAL
    assert lib.polar_bpl_decode_batch(None, None, 0, None, None, None, None, None) == EINVAL


NEW_SYMBOLS = ["polar_bpl_set_graphs", "polar_bpl_get_graphs", "polar_bpl_cyclic_graphs", "polar_bpl_decode_device",
               "polar_bpl_decode_batch"]


def test_bpl_abi_is_declared_and_exported():
    full = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"#define\s+POLAR_ALGO_BPL\s+6\b", full)
    import polardecoding_amd as pa
    lib = pa.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert pa.ALGO_BPL == 6
    for name in ("BPL", "bpl_cyclic_graphs"):
        assert callable(getattr(pa, name)) and name in pa.__all__
    for name in ("set_bpl_graphs", "bpl_graphs", "decode_bpl_device", "decode_bpl_batch"):
        assert hasattr(pa.Decoder, name), name
    # the build list names the new translation unit
    import __graft_entry__ as g
    assert "k_bpl" in g.KERNEL_TUS
