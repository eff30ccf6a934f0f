"""The leaf schedule of the pair kernel (k_scl_fast2) against the CPU oracle on frozen patterns the golden vectors do not
have.  The goldens use one code (K + r = 536: a leading frozen run of 15 octets); which octet heads, which partial-sum
carries and which octet forms (frozen prefix / generic) the kernel runs depends on the pattern alone, so the schedule code
is exercised here with other info-set sizes: a leading frozen run of 0, 1, 7 and 15 octets, and a high-rate code in which
no octet after the first takes the frozen-prefix form.  Random frames at 1.5 dB; decisions, path metric and tie flag of
every frame must equal the oracle's; the batch sizes are odd, so the last wavefront decodes with one idle half."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024
# A = number of unfrozen leaves (K + 24 CRC bits with CA-SCL, K with SCL) -> leading all-frozen octets (5G sequence):
#   A >= 1000: 0    948..999: 1    697..837: 7    442..620: 15 (the kernel's prefix form covers at most 15)
# A = 999 has no octet of the frozen-prefix form (seven frozen leaves, then one more) after the leading one.
CASES = [(1008, 0), (960, 1), (760, 7), (536, 15), (999, 1)]


def leading_frozen_octets(code):
    fr = np.asarray(code.frozen).reshape(N // 8, 8)
    lead = 0
    while lead < N // 8 and fr[lead].all():
        lead += 1
    return lead


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("algo", ["CASCL", "SCL"])
@pytest.mark.parametrize("A,lead", CASES)
def test_pair_kernel_schedule_vs_oracle(A, lead, algo, dtype, oracle):
    import polardecoding_amd as pa
    taps = pa.CRC24C_TAPS if algo == "CASCL" else None
    K = A - 24 if algo == "CASCL" else A
    assert K >= 896 or A < 948   # the two shortest runs are also the high-rate cases
    code = oracle.Code(N, K, taps)
    assert min(leading_frozen_octets(code), 15) == lead
    dt = pa.F64 if dtype == "f64" else pa.F32
    dec = pa.CASCL(N, K, L=8, dtype=dt) if algo == "CASCL" else pa.SCLdecode(N, K, L=8, dtype=dt)
    assert dec.kernel_name.startswith("k_scl_fast2"), dec.kernel_name
    B = 131 if A != 536 else 201   # odd: the last pair of frames has one live codeword
    sim = oracle.Sim(7000 + A + (1 if algo == "SCL" else 0))
    sig = oracle.sigma_from_db(1.5)
    _, ys = sim.frames(code, sig, B)
    llr = np.stack([oracle.llr_from_y(y, sig) for y in ys]).astype(np.float32).astype(np.float64)
    ref_uh, ref_pm, ref_t = oracle.decode(code, llr, algo, L=8, dtype=dtype)
    uh, pm, fl = dec.decode_batch(llr)
    assert uh.shape == ref_uh.shape and len(pm) == B and len(fl) == B
    bad = np.nonzero((uh != ref_uh).any(axis=1))[0]
    assert bad.size == 0, f"decisions differ in frames {bad[:8]}"
    assert np.array_equal(pm.astype(np.float32 if dtype == "f32" else np.float64), ref_pm)
    assert np.array_equal((fl & pa.FLAG_TIE) != 0, ref_t > 0)
