"""CPU: the input families of tests/llr_families.py do their job, on the models and the oracle alone.

tests/test_gpu_llr_families.py compares the kernels with the references on quantised, tied and degenerate rows.  That
comparison can only fail where the inputs reach the code that decides ties, so the conditions are held here first:
  * CA-SCL L = 8 on every grid: at least 50 of 200 frames with a median tie, at least 50 with the re-rank statistic raised;
  * SC-Flip: scf_model with flip_list as it is and with ties resolved to the LARGER j give different outputs on at least
    5 frames in each of the four cases, on the grids (1.0, 7) and (2.0, 3);
  * SCAN: the skipping form of scan_model equals the plain form on every family, with no invalid operation;
  * leaf zeros: on each grid some information-leaf LLR of SC is exactly zero at N = 1024.
Each minimum is a condition; the counts are printed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import llr_families as F  # noqa: E402
import test_scf_host as SCF  # noqa: E402
from test_construct_host import design_rows  # noqa: E402
from test_cascl_adaptive_host import CRC6, CRC24C  # noqa: E402
from test_scan_host import scan_model  # noqa: E402

SEED = 5


def test_family_values():
    llr = design_rows(128, 70, 0.8, 3)
    for step, maxq in F.GRIDS:
        g = F.grid(llr, step, maxq)
        assert np.array_equal(g, np.rint(g / step) * step) and np.abs(g).max() == step * maxq
        assert np.array_equal(g.astype(np.float32).astype(np.float64), g)          # exact in f32
        assert (np.sign(g) * np.sign(llr) >= 0).all()
    h = F.hard(llr, 1.5)
    assert set(np.unique(h).tolist()) == {-1.5, 1.5} and np.array_equal(h < 0, llr < 0)
    z = F.grid(llr, 2.0, 3)
    m = F.mix_zero_signs(z, 9)
    assert np.array_equal(m, z)                                                      # -0.0 == +0.0
    neg = np.signbit(m[z == 0])
    assert (z == 0).sum() > 50 and 0.3 < neg.mean() < 0.7
    for dt in (np.float64, np.float32):
        rows = F.degenerate_rows(128, dt, 4)
        names = [n for n, _ in rows]
        assert names == ["zero+", "zero-", "all+c", "all-c", "alternating", "one_nonzero", "2^20", "1e30", "subnormal"]
        d = dict(rows)
        assert all(r.dtype == dt and np.isfinite(r).all() for r in d.values())
        assert not np.signbit(d["zero+"]).any() and np.signbit(d["zero-"]).all()
        assert (d["one_nonzero"] != 0).sum() == 1
        assert (np.abs(d["2^20"]) == 2.0 ** 20).all()
        tiny = np.abs(d["subnormal"])
        assert (tiny > 0).all() and (tiny < np.finfo(dt).tiny).all()                 # subnormal, not flushed by the host
        assert np.isfinite(np.abs(d["1e30"]).astype(dt).sum(dtype=dt) * dt(32))      # 4096 additions stay finite
        x = F.plant(F.grid(llr, 1.0, 7).astype(dt), rows, start=3)
        placed = [x[0], x[63], x[64], x[-1]]
        for p, k in zip(placed, (3, 4, 5, 6)):
            assert np.array_equal(p.view(np.uint8), rows[k][1].view(np.uint8))
        for _, r in rows:                                                            # every row three times
            assert sum(np.array_equal(x[b].view(np.uint8), r.view(np.uint8)) for b in range(len(x))) >= 3
        assert F.edge_positions(66) == [0, 63, 64, 65] and F.edge_positions(130) == [0, 63, 64, 127, 128, 129]
        big = F.plant(np.full((322, 128), 5.0, dtype=dt), rows)
        for _, r in rows:                                                            # 322 frames: every row on a boundary
            assert any(np.array_equal(big[b].view(np.uint8), r.view(np.uint8)) for b in F.edge_positions(322))
        assert len(F.edge_positions(322)) >= len(rows) and (big == 5).all(axis=1).sum() == 322 - 27
        fam = F.families(llr, 1, dt)
        assert len(fam) == 8 and all(v.dtype == dt and v.shape == llr.shape for v in fam.values())
        assert not any(np.isnan(v).any() or np.isinf(v).any() for v in fam.values())


@pytest.mark.parametrize("step,maxq", F.GRIDS)
@pytest.mark.parametrize("N,K,taps", [(1024, 512, CRC24C), (128, 64, CRC6)])
def test_cascl_grids_are_dense_with_ties(N, K, taps, step, maxq, oracle):
    code = oracle.Code(N, K, taps)
    llr = F.oracle_llr(oracle, code, 200, SEED, 2.0)
    x = F.grid(llr, step, maxq)
    st = np.zeros((200, 2), dtype=np.int32)
    _, _, ties = oracle.decode(code, x, "CASCL", L=8, stats=st)
    print(f"CA-SCL N={N} L=8 grid({step:g}, {maxq}): frames with ties {(ties > 0).sum()}, with re-rank {(st[:, 0] > 0).sum()} of 200")
    assert (ties > 0).sum() >= 50
    assert (st[:, 0] > 0).sum() >= 50


def _flip_list_larger_j(lam, info_order, T):
    """flip_list of tests/test_scf_host.py with ties resolved to the LARGER j (the mutant)"""
    a = np.abs(lam[:, info_order])
    j = np.broadcast_to(np.asarray(info_order), a.shape)
    order = np.lexsort((-j, a), axis=-1)
    return np.take_along_axis(j, order, axis=-1)[:, :T]


SCF_CASES = [(128, 64, CRC6, 8, 3000), (128, 64, CRC6, 32, 3000), (1024, 512, CRC24C, 8, 1500), (1024, 512, CRC24C, 32, 1500)]


@pytest.mark.parametrize("step,maxq", [(1.0, 7), (2.0, 3)])
@pytest.mark.parametrize("N,K,taps,T,B", SCF_CASES)
def test_scf_tie_rule_decides_outputs(N, K, taps, T, B, step, maxq, oracle, monkeypatch):
    code = oracle.Code(N, K, taps)
    llr = F.oracle_llr(oracle, code, B, SEED, 1.5)
    x = F.grid(llr, step, maxq)
    a = SCF.scf_model(code, x, T, oracle=oracle)
    monkeypatch.setattr(SCF, "flip_list", _flip_list_larger_j)
    b = SCF.scf_model(code, x, T, oracle=oracle)
    monkeypatch.undo()
    assert np.array_equal(a[4], b[4])                                  # the same failing frames
    lists = int((a[3] != b[3]).any(axis=1).sum())
    differ = int(((a[0] != b[0]).any(axis=1) | (a[2] != b[2])).sum())
    print(f"SC-Flip N={N} T={T} B={B} grid({step:g}, {maxq}): {len(a[4])} failing frames, {lists} flip lists differ, "
          f"{differ} frames differ in u_hat or attempts")
    assert differ >= 5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N,K,B", [(128, 64, 70), (1024, 512, 66)])
def test_scan_skipping_form_on_every_family(N, K, B, dtype, oracle):
    code = oracle.Code(N, K)
    llr = F.oracle_llr(oracle, code, B, SEED, 1.5)
    for name, x in F.families(llr, SEED, dtype).items():
        for iters in (1, 4):
            with np.errstate(invalid="raise"):
                a = scan_model(code.frozen, x, iters, dtype=dtype, oracle=oracle, skip=False)
                b = scan_model(code.frozen, x, iters, dtype=dtype, oracle=oracle, skip=True)
            for u, v in zip(a, b):
                assert not np.isnan(u).any() and (u == v).all(), (name, iters)


@pytest.mark.parametrize("step,maxq", F.GRIDS)
def test_grids_reach_exact_zero_leaves(step, maxq, oracle):
    N, K = 1024, 512
    code = oracle.Code(N, K, CRC24C)
    llr = F.oracle_llr(oracle, code, 200, SEED, 1.5)
    for dtype in (np.float64, np.float32):
        _, lam = SCF.sc_run(oracle, code.frozen, F.grid(llr, step, maxq), dtype=dtype)
        zeros = int((lam[:, code.info_order] == 0).sum())
        print(f"SC N={N} grid({step:g}, {maxq}) {np.dtype(dtype).name}: {zeros} information-leaf LLRs exactly zero in 200 frames")
        assert zeros >= 1
