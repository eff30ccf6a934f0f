"""GPU: a context gives back everything it took.  polar_destroy has no list of its own: every stream, event, pinned
buffer, table and scratch buffer of a polar_ctx is a member of an owning type (csrc/dev_owned.h), and the two lanes of
polar_fer_batch are exchanged by one function.  These tests create, use and destroy one context of every kind that owns more
than the base set and watch the device's free memory, and check that the lane exchange leaves a ctx as it found it.

The leak criterion.  One round = every kind of KINDS created, used once and destroyed.  After a warm-up round the free
memory of the device (hipMemGetInfo) is read, four more rounds run, and it is read again: it must not have dropped by more
than SLACK.  SLACK comes from the parent commit (hand-written polar_destroy), measured three times on one MI355X with this
file: its loss over the same four rounds was 0, 0 and 0 bytes (MEASURED_PARENT_LOSS), and one allocation granule of the
runtime is 2 MiB (GRANULE: free memory moved by 35, 137 and 545 times 2 MiB for the SCAN context at 1024, 4096 and 16384
frames, and by nothing smaller); SLACK = max(loss) + GRANULE = 2 MiB.  This commit lost 0 bytes in the same run.  So that
the test cannot pass vacuously, the free memory read while the largest context of the set is alive (SCAN at N = 1024, f64,
SCAN_B frames: its scratch is 4.25 MiB per resident wavefront; measured 274 MiB below the baseline) must be at least
10 * SLACK below the baseline: a context of that size that was never freed would fail the criterion at once.  The runtime
hands out small allocations from granules it keeps, so the criterion sees a leaked table only once the leak crosses a
granule; the owning types themselves are checked allocation by allocation in tests/native/owned_selftest.cpp.

Free memory is a figure of the whole device: an allocation by another tenant of the GPU during the four rounds can fail
test_four_rounds_leak_nothing falsely."""
import hashlib

import numpy as np
import pytest
import torch

import polardecoding_amd as pa

pytestmark = pytest.mark.gpu

MEASURED_PARENT_LOSS = (0, 0, 0)   # bytes, three runs of four rounds on the parent commit
GRANULE = 2 << 20                  # bytes, read off the same runs
SLACK = max(MEASURED_PARENT_LOSS) + GRANULE
SCAN_B = 4096                      # 64 resident wavefronts of SCAN scratch: 274 MiB of free memory
FER_B = 32768                      # polar_fer_batch splits into two lanes from here


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


_llr_cache = {}


def _llr(B, W):
    """all-zero codeword over BPSK + AWGN at 2 dB as LLRs, [B][W] float64 (host); built once per shape"""
    if (B, W) not in _llr_cache:
        rng = np.random.default_rng(100 + W)
        sigma = 10 ** (-2.0 / 20)
        _llr_cache[(B, W)] = 2 * (1.0 + sigma * rng.standard_normal((B, W))) / sigma / sigma
    return _llr_cache[(B, W)]


def _dev(B, W):
    key = ("dev", B, W)
    if key not in _llr_cache:
        _llr_cache[key] = torch.from_numpy(_llr(B, W)).cuda()
    return _llr_cache[key]


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return h.hexdigest()


def _device_decode(dec, B):
    pm = torch.zeros(B, dtype=torch.float64, device="cuda")
    fl = torch.zeros(B, dtype=torch.int32, device="cuda")
    bits = dec.decode_device(_dev(B, dec.E), pm=pm, flags=fl)
    dec.synchronize()
    return _sha(bits, pm, fl)


def _host_pipeline(probe):
    dec = pa.CASCL(1024, 512, L=8)          # pinned buffers, copy stream, six events, ping-pong device buffers
    out = _sha(*dec.decode_batch(_llr(256, 1024)))
    dec.close()
    return out


def _stages(probe):
    dec = pa.CASCL(1024, 512, L=8, stages=[1, 2, 8])   # two stage contexts on the parent's stream, the ad_* buffers
    out = _device_decode(dec, 256)
    dec.close()
    return out


def _rate_matched(probe):
    dec = pa.CASCL(1024, 200, L=8, E=864, ibil=True)   # the interleaver tables, rm_rows
    out = _device_decode(dec, 128)
    dec.close()
    return out


def _dynamic(probe):
    N, K = 64, 32
    io = np.asarray(pa.q_sequence(N)[N - K:], dtype=np.int32)
    frozen = np.setdiff1d(np.arange(N), io)
    pos = [int(j) for j in frozen[frozen > io.min()][:3]]   # D = 3
    sets = [np.arange(j % 3, j, 3) for j in pos]
    dec = pa.Decoder(N, K, pa.ALGO_SCL, L=8, info_order=io, dyn=(pos, sets))
    assert len(dec.dyn_positions) == 3
    out = _device_decode(dec, 64)
    dec.close()
    return out


def _scflip(probe):
    dec = pa.SCFlip(1024, 512)
    bits = dec.decode_scf_device(_dev(256, 1024))
    dec.synchronize()
    out = _sha(bits)
    dec.close()
    return out


def _scan(probe):
    dec = pa.SCAN(1024, 512)                # the largest context of the set
    bits = dec.decode_scan_device(_dev(SCAN_B, 1024))
    dec.synchronize()
    out = _sha(bits)
    if probe is not None:
        probe.append(_free())
    dec.close()
    return out


def _q8(probe):
    dec = pa.CASCL(1024, 512, L=8, dtype=pa.Q8)         # q8_rows, q8_pm
    out = _device_decode(dec, 256)
    dec.close()
    return out


def _systematic_encode(probe):
    dec = pa.SCLdecode(128, 64, L=8)
    dec.set_systematic(True)                            # then the three encoder tables and its scratch rows
    payload = (np.arange(64 * 64).reshape(64, 64) * 7 // 3) & 1
    out = _sha(*dec.encode_batch(payload))
    dec.close()
    return out


def _fer_two_lanes(probe):
    dec = pa.CASCL(128, 64, L=8)                        # stream_b, ev_b, both lanes' scratch
    out = repr(dec.fer_batch(11, 0, 2.0, FER_B))
    dec.close()
    return out


KINDS = (_host_pipeline, _stages, _rate_matched, _dynamic, _scflip, _scan, _q8, _systematic_encode, _fer_two_lanes)


def one_round(probe=None):
    return [kind(probe) for kind in KINDS]


def four_round_loss():
    """(bytes of free memory lost over four rounds, baseline - free memory with the SCAN context alive, smallest nonzero
    step of free memory seen); the caller has run the warm-up round"""
    base = _free()
    probe, seen = [], [base]
    for _ in range(4):
        one_round(probe)
        seen.append(_free())
    steps = [abs(a - b) for a, b in zip(seen, seen[1:]) if a != b] + [abs(base - p) for p in probe if p != base]
    return base - seen[-1], base - min(probe), min(steps) if steps else 0


@pytest.fixture(scope="module")
def warm():
    return one_round()


def test_create_decode_destroy_every_kind(warm):
    """a context made after the first of its kind was destroyed computes what the first did"""
    assert one_round() == warm


def test_four_rounds_leak_nothing(warm):
    lost, largest, step = four_round_loss()
    print(f"free memory lost over four rounds: {lost} bytes; SCAN context alive: {largest} bytes below the baseline; "
          f"smallest step {step} bytes; slack {SLACK}")
    assert largest >= 10 * SLACK, "the largest context is too small for the slack: the criterion would pass vacuously"
    assert lost <= SLACK


def test_lane_exchange_leaves_the_ctx_as_it_was():
    """polar_fer_batch with two lanes twice on one ctx: the same counters; a plain decode on that ctx afterwards (its own
    stream, its own scratch again) equals the same decode on a fresh ctx"""
    dec = pa.CASCL(128, 64, L=8)
    first = dec.fer_batch(5, 0, 1.0, FER_B)
    assert dec.fer_batch(5, 0, 1.0, FER_B) == first
    assert first[0] > 0   # frames in error at 1 dB: the counters count
    B = 40000             # above the resident count: the decode uses the scratch buffer's work queue
    after = _device_decode(dec, B)
    dec.close()
    fresh = pa.CASCL(128, 64, L=8)
    assert _device_decode(fresh, B) == after
    fresh.close()
