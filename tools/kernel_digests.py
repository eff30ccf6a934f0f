"""Developer tool: a SHA-256 per case of what k_scl_generic, k_scl_dyn, k_scl_q8, k_scl_wide and the three generators
(k_generate, k_generate_rm, k_generate_dyn) write, for comparing two builds more finely than the tests do.

    python3 tools/kernel_digests.py [ROOT] > A.txt
    python3 tools/kernel_digests.py [OTHER_ROOT] > B.txt     (same box, same session)
    diff A.txt B.txt

ROOT is the checkout whose package and libraries are used (default: this one).  Decoders: decisions, metrics and flags of
one batch below and one above the resident count, N = 32 / 64 / 128, L = 1 / 2 / 8 / 32, f64 and f32, LDS and global-scratch
variant, SC / SCL / CA-SCL (CRC-6) and PAC / PC-CA-polar / random-mask dynamic sets; a quarter of the rows sits on a grid so
that metrics tie.  k_scl_q8 (float rows into a POLAR_Q8 context): SCL / CA-SCL, L = 1 / 8 / 32 at the same N; k_scl_wide:
L = 64 at N = 32 / 64, f64 and f32, SCL / CA-SCL / PAC.  Generators: LLR and y rows, f64 and f32, with u_bits.  Generator digests depend on the ROCm math library
(log, sincospi), so they compare builds on one installation and are not pinned anywhere."""
import hashlib
import os
import sys

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch
import polardecoding_amd as pa
from polardecoding_amd import testing as T

CRC24C, CRC6 = pa.CRC24C_TAPS, pa.CRC6_TAPS
B_SMALL, B_LARGE = 37, 40011    # below / above the resident job count of a 64-thread block with at most 160 KiB of LDS
_rows = {}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def rows(N, f32):
    """all-zero codeword over BPSK + AWGN at 1 dB (rate 1/2) as LLRs; every fourth row rounded to halves, so candidates tie"""
    if (N, f32) not in _rows:
        rng = np.random.default_rng(1000 + N)
        sigma = 10 ** (-1.0 / 20)
        x = 2 * (1.0 + sigma * rng.standard_normal((B_LARGE, N))) / sigma / sigma
        x[3::4] = np.round(x[3::4] * 2) / 2
        _rows[(N, f32)] = torch.from_numpy(x.astype(np.float32 if f32 else np.float64)).cuda()
    return _rows[(N, f32)]


def decode(label, dec, variant=None):
    """variant None: the context keeps the kernel it chose (k_scl_q8, k_scl_wide)"""
    if variant is not None:
        T.select_kernel(dec, variant)
    f32 = dec.dtype == pa.F32
    for B in (B_SMALL, B_LARGE):
        x = rows(dec.N, f32)[:B]
        pm = torch.zeros(B, dtype=torch.float64, device="cuda")
        fl = torch.zeros(B, dtype=torch.int32, device="cuda")
        bits = dec.decode_device(x, pm=pm, flags=fl)
        dec.synchronize()
        print(f"{label} {'-' if variant is None else 'GA' if variant == T.KERNEL_GENERIC_SPILL else 'LDS'} B={B} {dec.kernel_name} "
              f"ties={int((fl & 1).sum())} {sha(bits, pm, fl)}", flush=True)
    dec.close()


def generate(label, mk, B=777):
    for dt, tdt in ((pa.F64, torch.float64), (pa.F32, torch.float32)):
        for is_y in (False, True):
            try:
                dec = mk(dt)
            except pa.PolarError as e:      # a combination the library does not offer: the same line from both builds
                print(f"{label} not created: {e}", flush=True)
                continue
            out = torch.zeros((B, dec.E), dtype=tdt, device="cuda")
            ub = torch.zeros((B, dec.N // 32), dtype=torch.int32, device="cuda")
            dec.generate_device(4242, 17, 1.5, out, ub, out_is_y=is_y)
            dec.synchronize()
            print(f"{label} mode={dec.rm_mode} {'f32' if dt else 'f64'} {'y' if is_y else 'llr'} "
                  f"ones={int(torch.count_nonzero(ub))} {sha(out, ub)}", flush=True)
            dec.close()


def dyn_sets(N, K):
    """a random-mask dynamic set: every second frozen position after the first information bit takes a sparse set of
    earlier positions, earlier dynamic positions among them"""
    rng = np.random.default_rng(N)
    io = np.asarray(pa.q_sequence(N)[N - K:], dtype=np.int32)
    frozen = np.setdiff1d(np.arange(N), io)
    pos = [int(j) for j in frozen[frozen > io.min()][::2]]
    return io, (pos, [np.sort(rng.choice(j, size=min(j, 5), replace=False)) for j in pos])


for N in (64, 1024):
    K = N // 2 - 8
    for name, kw in (("crc", {}), ("syscrc", {"systematic": True}), ("syspolar", {"sys_polar": True})):
        generate(f"k_generate N={N} {name}", lambda dt: pa.CASCL(N, K, L=8, crc_taps=CRC6 if N == 64 else CRC24C, dtype=dt, **kw))
    generate(f"k_generate N={N} sc", lambda dt: pa.SCdecode(N, N // 2, dtype=dt))
for K, E in ((512, 2048), (200, 864), (512, 864)):     # repeat, puncture, shorten
    for ibil in (False, True):
        generate(f"k_generate_rm K={K} E={E} ibil={int(ibil)}", lambda dt: pa.CASCL(1024, K, L=8, E=E, ibil=ibil, dtype=dt))
generate("k_generate_rm syscrc E=700", lambda dt: pa.CASCL(1024, 300, L=8, E=700, systematic=True, dtype=dt))
generate("k_generate_dyn pac128", lambda dt: pa.PAC(128, 64, L=8, dtype=dt))
generate("k_generate_dyn pac1024", lambda dt: pa.PAC(1024, 512, L=8, dtype=dt))
generate("k_generate_dyn pc64", lambda dt: pa.PCCASCL(64, 14, L=8, dtype=dt))
generate("k_generate_dyn pc256", lambda dt: pa.PCCASCL(256, 18, n_pc_wm=1, L=8, dtype=dt))

for variant in (T.KERNEL_GENERIC, T.KERNEL_GENERIC_SPILL):
    for dt in (pa.F64, pa.F32):
        d = "f32" if dt else "f64"
        for N in (32, 64, 128):
            K = N // 2
            decode(f"generic sc N={N} {d}", pa.SCdecode(N, K, dtype=dt), variant)
            decode(f"dyn pac N={N} L=1 {d}", pa.PAC(N, K, L=1, dtype=dt), variant)
            for L in (1, 2, 8, 32):
                decode(f"generic scl N={N} L={L} {d}", pa.SCLdecode(N, K, L=L, dtype=dt), variant)
                decode(f"generic cascl N={N} L={L} {d}", pa.CASCL(N, K - 6, L=L, crc_taps=CRC6, dtype=dt), variant)
                if L > 1:
                    decode(f"dyn pac N={N} L={L} {d}", pa.PAC(N, K, L=L, dtype=dt), variant)
                decode(f"dyn pc N={N} L={L} {d}", pa.PCCASCL(N, K - 9, n_pc_wm=1, L=L, dtype=dt), variant)
                io, dyn = dyn_sets(N, K)
                decode(f"dyn random N={N} L={L} {d}", pa.Decoder(N, K, pa.ALGO_SCL, L=L, dtype=dt, info_order=io, dyn=dyn), variant)
for N in (32, 64, 128):
    K = N // 2
    for L in (1, 8, 32):
        decode(f"q8 scl N={N} L={L}", pa.SCLdecode(N, K, L=L, dtype=pa.Q8))
        decode(f"q8 cascl N={N} L={L}", pa.CASCL(N, K - 6, L=L, crc_taps=CRC6, dtype=pa.Q8))
for dt in (pa.F64, pa.F32):
    d = "f32" if dt else "f64"
    for N in (32, 64):
        K = N // 2
        decode(f"wide scl N={N} L=64 {d}", pa.SCLdecode(N, K, L=64, dtype=dt))
        decode(f"wide cascl N={N} L=64 {d}", pa.CASCL(N, K - 6, L=64, crc_taps=CRC6, dtype=dt))
        decode(f"wide pac N={N} L=64 {d}", pa.PAC(N, K, L=64, dtype=dt))
print("done", flush=True)
