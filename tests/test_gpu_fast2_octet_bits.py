"""GPU: the partial sums inside an octet of the pair kernel (k_scl_fast2 / k_scl_fast2_y, csrc/scl_fast2.h) against the CPU
oracle.

Bits 0..7 of a path's word bl0 hold the octet's decided bits as they are; the level-1 g steps before leaves 2 and 6, the
level-2 g step before leaf 4 and the octet's level-3 word at leaf 7 form their sums from them on read (csrc/octet_bits.h,
which also holds the rule to the stored-sum form by static_assert).  A frozen leaf writes nothing, a fork copies the source's
raw bits, and what a reader sees depends on which of the leaves in front of it were information leaves.  So the cases are
frozen sets in which every one of the 256 octet masks occurs, N = 1024, L = 8, LLR rows and f64 unless said otherwise:

    masks_crc    128 shuffled octet masks, CRC-24C at a seeded choice of the information leaves, 0.5 dB
    masks_nocrc  the other 128 masks, no CRC, 0.5 dB
    masks_f32    the first set with f32 rows against the f32 oracle, 1 dB
    masks_y      the second set as channel observations with sigma > 0 (k_scl_fast2_y), 1 dB
    headline     the 5G order, K + r = 536 with CRC-24C, 1 dB: the list-filling phase hands over at octet 24 (E = 192)
    scl512       the 5G order, K = 512 without CRC, 0 dB: the same hand-over with four paths

At 0 - 1 dB most information leaves rank their candidates and forks are frequent.  Batch sizes 1 (the idle half-wave
re-decodes the frame), 2 (one pair), 5 (odd tail) and 64 (several pairs per block).  Decisions, path metric (bit pattern)
and the tie / re-rank / CRC flags must equal the oracle's frame for frame.  The oracle decodes each case's 64 frames once."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frozen_patterns as P  # noqa: E402

N, L, NF = 1024, 8, 64
MASK_SEED = 1901
#            set   CRC    dB   seed  dtype  y form
CASES = {
    "masks_crc": (0, True, 0.5, 1911, "f64", False),
    "masks_nocrc": (1, False, 0.5, 1912, "f64", False),
    "masks_f32": (0, True, 1.0, 1913, "f32", False),
    "masks_y": (1, False, 1.0, 1914, "f64", True),
    "headline": (None, True, 1.0, 1915, "f64", False),
    "scl512": (None, False, 0.0, 1916, "f64", False),
}
_cache = {}


def octet_sets():
    """two frozen masks [N] whose 2 x 128 octets are one seeded shuffle of the 256 octet masks"""
    perm = np.random.default_rng(MASK_SEED).permutation(256)
    return P.from_octets(perm[:128]), P.from_octets(perm[128:])


def _case(oracle, name):
    """the case's code, rows and what the oracle makes of them (computed once, read-only)"""
    if name not in _cache:
        from test_cascl_adaptive_host import syndrome
        which, crc, db, seed, dtype, from_y = CASES[name]
        taps = oracle.CRC24C_TAPS if crc else None
        if which is None:
            code, order, mask = oracle.Code(N, 512, taps), None, None
        else:
            mask = octet_sets()[which]
            order = P.order_of(mask, MASK_SEED + which)
            code = oracle.Code(N, order.size - (max(taps) if taps else 0), taps, Q=P.q_of(mask, order))
            assert np.array_equal(code.frozen, mask) and np.array_equal(code.info_order, order), name
        sig = oracle.sigma_from_db(db)
        _, ys = oracle.Sim(seed).frames(code, sig, NF)
        y = np.stack(ys)
        llr = np.stack([oracle.llr_from_y(r, sig) for r in y])
        if dtype == "f32":
            llr = llr.astype(np.float32)
        st = np.zeros((NF, 2), dtype=np.int32)
        uh, pm, ties = oracle.decode(code, llr, "CASCL" if crc else "SCL", L=L, dtype=dtype, stats=st)
        ok = (syndrome(uh, code.info_order, taps) == 0) if crc else np.zeros(NF, dtype=bool)
        for a in (y, llr, uh, pm, ties, st, ok):
            a.setflags(write=False)
        _cache[name] = dict(code=code, order=order, mask=mask, rows=y if from_y else llr, sigma=sig if from_y else 0.0,
                            uh=uh, pm=pm, ties=ties, st=st, ok=ok)
    return _cache[name]


def test_cases_are_not_vacuous(oracle):
    """from the oracle alone: the two sets hold all 256 octet masks; in every case the decisions at the information leaves
    = K (mod 8) hold a 0 and a 1 for every K (so every raw bit of an octet is seen set and clear, and every reader sees both
    values of every sum); leaves where the 32-bit keys do not decide occur in the f64 mask batches; the two 5G codes are
    the ones whose list fills at leaf 191"""
    a, b = octet_sets()
    assert sorted(P.octets_of(a).tolist() + P.octets_of(b).tolist()) == list(range(256))
    for name in CASES:
        c = _case(oracle, name)
        info = np.flatnonzero(np.asarray(c["code"].frozen) == 0)
        for K in range(8):
            u = c["uh"][:, info[info % 8 == K]]
            assert u.size and (u == 0).any() and (u == 1).any(), (name, K)
        # a leaf of each parity class is also frozen somewhere (the mask sets: every combination of neighbours)
        if c["mask"] is not None:
            assert all(c["mask"][K::8].any() and not c["mask"][K::8].all() for K in range(8)), name
    for name in ("masks_crc", "masks_nocrc"):
        c = _case(oracle, name)
        assert int(c["st"][:, 0].sum()) > 0, (name, "no leaf at which the keys are not enough")
        print(f"{name}: re-ranked leaves {int(c['st'][:, 0].sum())}, frames with a tie {int((c['ties'] > 0).sum())}, "
              f"frames whose CRC passes {int(c['ok'].sum())}")
    assert _case(oracle, "headline")["code"].A == 536 and _case(oracle, "scl512")["code"].A == 512
    for name in ("headline", "scl512"):
        assert sorted(int(j) for j in _case(oracle, name)["code"].info_order if j < 192)[-1] == 191, name


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 5, 64])
@pytest.mark.parametrize("name", list(CASES))
def test_octet_bits_vs_oracle(name, B, oracle):
    import torch
    import polardecoding_amd as pa
    from conftest import unpack_bits
    c = _case(oracle, name)
    crc, dtype = CASES[name][1], CASES[name][4]
    code = c["code"]
    dec = pa.Decoder(N, code.K, pa.ALGO_CASCL if crc else pa.ALGO_SCL, L=L, crc_taps=oracle.CRC24C_TAPS if crc else None,
                     dtype=pa.F64 if dtype == "f64" else pa.F32, **({} if c["order"] is None else {"info_order": c["order"]}))
    assert np.array_equal(np.sort(dec.info_order), np.flatnonzero(np.asarray(code.frozen) == 0)), name
    x = torch.from_numpy(np.array(c["rows"][:B])).cuda()   # a writable copy: the cached rows are read-only
    bits = torch.full((B, N // 32), -1, dtype=torch.int32, device="cuda")
    pm = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_device(x, sigma=c["sigma"], out_bits=bits, pm=pm, flags=fl)
    dec.synchronize()
    assert dec.kernel_name.startswith("k_scl_fast2<"), dec.kernel_name
    uh, pm, fl = unpack_bits(bits.cpu().numpy(), N), pm.cpu().numpy(), fl.cpu().numpy().view(np.uint32)
    dec.close()
    bad = np.nonzero((uh != c["uh"][:B]).any(axis=1))[0]
    assert bad.size == 0, f"decisions differ from the oracle's in frames {bad[:8]}"
    want = c["pm"][:B]
    if dtype == "f64":
        assert np.array_equal(pm.view(np.int64), want.view(np.int64))
    else:   # the f32 kernels return the float32 metric widened
        assert np.array_equal(pm.astype(np.float32).view(np.int32), want.astype(np.float32).view(np.int32))
        assert np.array_equal(pm, pm.astype(np.float32).astype(np.float64))
    assert np.array_equal((fl & pa.FLAG_TIE) != 0, c["ties"][:B] > 0)
    if dtype == "f64":   # the f32 keys are the whole metric: no re-rank there
        assert np.array_equal((fl & pa.FLAG_RERANK) != 0, c["st"][:B, 0] > 0)
    else:
        assert not (fl & pa.FLAG_RERANK).any()
    assert np.array_equal((fl & pa.FLAG_CRC_PASS) != 0, c["ok"][:B])
    assert not (fl & ~np.uint32(pa.FLAG_TIE | pa.FLAG_RERANK | pa.FLAG_CRC_PASS)).any()
