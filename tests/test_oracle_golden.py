"""CPU: the oracle restatement against the committed golden vectors (made from the compiled reference)
and, when oracle/_ref is present (build container / travelled to the box), against the real reference."""
import numpy as np
import pytest

from conftest import load_golden

PROGRAMS = ["SC_128", "SC_1024", "BP_128", "BP_1024", "BP_1024_it50", "SCL_128", "SCL_1024", "CASCL_128", "CASCL_1024_L8",
            "CASCL_1024_sys"]  # the last one decodes on the bit-reversed graph: same decisions


@pytest.mark.parametrize("name", PROGRAMS)
def test_oracle_matches_golden(name, oracle):
    N, K, taps, algo, L = oracle.REF_PROGRAMS[name]
    code = oracle.Code(N, K, taps, systematic=name in oracle.SYSTEMATIC_PROGRAMS)
    g = load_golden(name)
    n = len(g["sigma"]) if N == 128 or algo != "BP" else 4
    for i in range(n):
        llr = oracle.llr_from_y(g["y"][i], float(g["sigma"][i]))
        uh, pm, ties = oracle.decode(code, llr, algo, L=L, bp_iters=oracle.BP_ITERS.get(name, 100))
        assert np.array_equal(uh, g["u_hat"][i].astype(np.int32)), f"{name} frame {i}"
        if algo in ("SCL", "CASCL"):
            assert pm == g["pm"][i]
            assert ties == 0


@pytest.mark.parametrize("name", PROGRAMS)
def test_oracle_matches_compiled_reference(name, oracle):
    """Seeded AWGN frames (oracle.Sim(4242), 1.0 and 2.5 dB) with the compiled reference's answers on them, stored as
    tests/golden/sim4242_<name>.npz (make_golden.py: make_sim4242).  Where oracle/_ref is built, the reference itself is
    asked again, frame after frame as the fixture was made, and must still give the stored answers."""
    N, K, taps, algo, L = oracle.REF_PROGRAMS[name]
    code = oracle.Code(N, K, taps, systematic=name in oracle.SYSTEMATIC_PROGRAMS)
    g = load_golden(f"sim4242_{name}")
    ref = oracle.Ref(name) if oracle.ref_available(name) else None
    for i in range(len(g["sigma"])):
        y, s = g["y"][i], float(g["sigma"][i])
        uh_ref, pm_ref = g["u_hat"][i].astype(np.int32), g["pm"][i]
        if ref is not None:
            uh_live, pm_live = ref.decode(y, s)
            assert np.array_equal(uh_live, uh_ref) and pm_live == pm_ref, f"{name} frame {i}: oracle/_ref vs fixture"
        uh, pm, _ = oracle.decode(code, oracle.llr_from_y(y, s), algo, L=L, bp_iters=oracle.BP_ITERS.get(name, 100))
        assert np.array_equal(uh, uh_ref), f"{name} frame {i}"
        if algo in ("SCL", "CASCL"):
            assert pm == pm_ref


def test_golden_inputs_are_consistent(oracle):
    """y in the fixtures is what the restated transmit chain produces for the recorded seed order."""
    g = load_golden("CASCL_1024_L8")
    code = oracle.Code(1024, 512, oracle.CRC24C_TAPS)
    # u is a valid CRC codeword placed on the information set, frozen positions are zero
    for i in range(4):
        u = g["u"][i].astype(np.int32)
        assert not u[code.frozen == 1].any()
        w = u[code.info_order]
        c = w.copy()
        for k in range(code.A - 1, code.r - 1, -1):
            if c[k]:
                for t in oracle.CRC24C_TAPS:
                    c[k - code.r + t] ^= 1
        assert not c[:code.r].any()


def test_systematic_fixture_words_are_systematic_codewords(oracle):
    """CASCL_1024_sys.c:776-789: w[r..K+r) is the payload itself, w[0..r) the remainder that makes w(D) a
    multiple of g(D) (checked with the long division of CRcheck, :1100-1125)."""
    g = load_golden("CASCL_1024_sys")
    code = oracle.Code(1024, 512, oracle.CRC24C_TAPS, systematic=True)
    sim = oracle.Sim(20261004 + 1024 + len("CASCL_1024_sys"))   # the fixture's seed (make_golden.py)
    for i in range(6):
        u_again, _ = sim.frame(code, float(g["sigma"][i]))
        u = g["u"][i].astype(np.int32)
        assert np.array_equal(u, u_again)
        w = u[code.info_order]
        c = w.copy()
        for k in range(code.A - 1, code.r - 1, -1):
            if c[k]:
                for t in oracle.CRC24C_TAPS:
                    c[k - code.r + t] ^= 1
        assert not c[:code.r].any()
    # the K true info bits are the only ones the error metric looks at (:820-821)
    u = g["u"][0].astype(np.int32)
    uh = u.copy()
    uh[code.info_order[0]] ^= 1          # a parity position
    assert oracle.count_bit_errors(code, u, uh) == 0
    uh[code.info_order[code.r]] ^= 1     # the first payload position
    assert oracle.count_bit_errors(code, u, uh) == 1


def test_oracle_bp_readouts_match_compiled_bpr(oracle):
    """BPr_128.c (BP with per-stage read-outs): decisions and the per-frame E[6][n+1] of the fixture,
    which the compiled program produced."""
    g = load_golden("BPr_128")
    code = oracle.Code(128, 64)
    iters, cp = int(g["iters"]), g["checkpoints"].tolist()
    assert (iters, cp) == (90, [3, 6, 10, 20, 40, 80])
    for i in range(len(g["sigma"])):
        llr = oracle.llr_from_y(g["y"][i], float(g["sigma"][i]))
        uh, E = oracle.bp_readout(code, llr, g["u"][i].astype(np.int32), iters, cp)
        assert np.array_equal(uh[0], g["u_hat"][i].astype(np.int32)), i
        assert np.array_equal(E, g["E"][i]), i


def test_crc6_dat_semantics():
    """CRC_6.dat format: 64x6 0/1 rows, row i = D^(6+i) mod (D^6+D^5+1), column j = coefficient
    of D^j.  The loader/generator lives in polardecoding_amd.crcfile; the expected rows are regenerated here."""
    from polardecoding_amd import crcfile
    m = crcfile.systematic_parity_matrix(64, (0, 5, 6))
    assert m.shape == (64, 6)
    # D^6 mod g = D^5 + 1
    assert m[0].tolist() == [1, 0, 0, 0, 0, 1]
    text = crcfile.dumps(m)
    back = crcfile.loads(text)
    assert np.array_equal(back, m)
    assert text[:2] == b"\xff\xfe" and b"\r\x00\n\x00" in text


def test_crc6_dat_file_is_reproduced_byte_for_byte():
    """tests/golden/CRC_6.dat is the reference's data file (data, not code)."""
    import os
    from conftest import GOLDEN
    from polardecoding_amd import crcfile
    with open(os.path.join(GOLDEN, "CRC_6.dat"), "rb") as f:
        ref = f.read()
    m = crcfile.systematic_parity_matrix(64, (0, 5, 6))
    assert np.array_equal(crcfile.loads(ref), m)
    assert crcfile.dumps(m) == ref
