#!/usr/bin/env python3
"""CRC-aided SC-Flip (POLAR_ALGO_SCF) against SC and fixed CA-SCL, on one GPU (developer tool).

N = 1024 / K = 512 / CRC-24C, f64 and f32 (--dtype), Eb/N0 = 1.0 .. 3.0 dB, on the same resident frames from
polar_generate_device: frames/s of one decode call (wall time of call + stream sync, mean over --reps calls after one
warm-up) and FER of SC-Flip with T = 4, 8, 16, 32, of SC over I[0..K+r) (k_sc_lanes) and of CA-SCL with L = 2, 4, 8.  Also
SC-Flip's pass A alone (T = 0: SC plus the CRC check) against SC, and the histogram of the attempt that decided each frame
(0 = plain SC; T counts the frames where no attempt passed).  One JSON line per (dtype, Eb/N0)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402

N, K = 1024, 512
TS = (4, 8, 16, 32)
LS = (2, 4, 8)
DBS = (1.0, 1.5, 2.0, 2.5, 3.0)


def timed(fn, dec, reps):
    fn()   # warm-up
    dec.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        dec.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def fer(dec, out, u, cnt):
    cnt.zero_()
    torch.cuda.synchronize()
    dec.count_errors_device(out, u, cnt)
    dec.synchronize()
    return int(cnt[0].item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f64,f32")
    ap.add_argument("--dbs", default=",".join(str(d) for d in DBS))
    ap.add_argument("--frames", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    args = ap.parse_args()
    dbs = [float(v) for v in args.dbs.split(",")]
    B = args.frames
    for dts in args.dtype.split(","):
        dt = pa.F64 if dts == "f64" else pa.F32
        tdt = torch.float64 if dts == "f64" else torch.float32
        scf = {T: pa.SCFlip(N, K, T=T, dtype=dt) for T in (0,) + TS}
        top = scf[TS[0]]
        sc = pa.Decoder(N, top.A, pa.ALGO_SC, dtype=dt, info_order=top.info_order)
        cascl = {L: pa.CASCL(N, K, L=L, dtype=dt) for L in LS}
        x = torch.empty((B, N), dtype=tdt, device="cuda")
        u = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        at = torch.empty(B, dtype=torch.int32, device="cuda")
        fl = torch.empty(B, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for db in dbs:
            top.generate_device(args.seed, 0, db, x, u)
            top.synchronize()
            row = {"dtype": dts, "N": N, "K": K, "crc": "24C", "frames": B, "ebn0_db": db, "kernel_scf": top.kernel_name}
            ms = timed(lambda: sc.decode_device(x, out_bits=out), sc, args.reps)
            row["frames_per_s_sc"] = B / ms * 1e3
            row["fer_sc"] = fer(sc, out, u, cnt) / B
            ms = timed(lambda: scf[0].decode_scf_device(x, out_bits=out), scf[0], args.reps)
            row["frames_per_s_scf_pass_a"] = B / ms * 1e3
            row["pass_a_over_sc"] = row["frames_per_s_sc"] / row["frames_per_s_scf_pass_a"]
            for T in TS:
                dec = scf[T]
                ms = timed(lambda: dec.decode_scf_device(x, out_bits=out, flags=fl, attempts=at), dec, args.reps)
                row[f"frames_per_s_scf_T{T}"] = B / ms * 1e3
                row[f"fer_scf_T{T}"] = fer(dec, out, u, cnt) / B
                h = torch.bincount(at.to(torch.int64), minlength=T + 1).cpu().tolist()
                nopass = int(((fl & pa.FLAG_CRC_PASS) == 0).sum().item())
                h[T] -= nopass
                row[f"attempts_scf_T{T}"] = h   # h[t]: frames decided by attempt t (passing)
                row[f"no_pass_scf_T{T}"] = nopass
            for L, dec in cascl.items():
                ms = timed(lambda: dec.decode_device(x, out_bits=out), dec, args.reps)
                row[f"frames_per_s_cascl_L{L}"] = B / ms * 1e3
                row[f"fer_cascl_L{L}"] = fer(dec, out, u, cnt) / B
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
