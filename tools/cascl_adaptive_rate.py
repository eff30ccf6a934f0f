#!/usr/bin/env python3
"""Adaptive CA-SCL (polar_cascl_set_stages) against the fixed-list decoders, on one GPU (developer tool).

For N = 1024 / K = 512 / CRC-24C with stages (1, 8, 32) and (8, 32), and N = 4096 / K = 2048 with stages (1, 8, 32) and
(8, 32) (BASELINE config 5), in f64 (and f32 with --dtype), at Eb/N0 = 1.0 .. 3.0 dB: frames/s of one polar_cascl_decode_device
call and of the fixed decoders (L_max, and L = 8 for N = 1024) on the same resident frames from polar_generate_device
(wall time of call + stream sync, mean over --reps calls, after one warm-up), the fraction of frames decided at each stage
and the FER of every decoder.  One JSON line per (config, dtype, Eb/N0)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402

# name, N, K, stages, fixed list sizes to compare with, frames
CONFIGS = [("CASCL_1024_1-8-32", 1024, 512, (1, 8, 32), (32, 8), 1 << 16),
           ("CASCL_1024_8-32", 1024, 512, (8, 32), (32, 8), 1 << 16),
           ("CASCL_4096_1-8-32", 4096, 2048, (1, 8, 32), (32,), 1 << 14),
           ("CASCL_4096_8-32", 4096, 2048, (8, 32), (32,), 1 << 14)]
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
    ap.add_argument("--only", default="")
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--dbs", default=",".join(str(d) for d in DBS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    args = ap.parse_args()
    dbs = [float(v) for v in args.dbs.split(",")]
    for name, N, K, stages, fixed, B in CONFIGS:
        if args.only and args.only not in name:
            continue
        for dts in args.dtype.split(","):
            dt = pa.F64 if dts == "f64" else pa.F32
            tdt = torch.float64 if dts == "f64" else torch.float32
            ad = pa.CASCL(N, K, L=stages[-1], stages=stages, dtype=dt)
            fx = {L: pa.CASCL(N, K, L=L, dtype=dt) for L in fixed}
            x = torch.empty((B, N), dtype=tdt, device="cuda")
            u = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
            out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
            ls = torch.empty(B, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            for db in dbs:
                ad.generate_device(args.seed, 0, db, x, u)
                ad.synchronize()
                row = {"config": name, "dtype": dts, "N": N, "K": K, "stages": list(stages), "frames": B, "ebn0_db": db,
                       "kernel_adaptive": ad.kernel_name}
                ms = timed(lambda: ad.decode_cascl_device(x, out_bits=out, list_size=ls), ad, args.reps)
                row["ms_adaptive"] = ms
                row["frames_per_s_adaptive"] = B / ms * 1e3
                row["fer_adaptive"] = fer(ad, out, u, cnt) / B
                row["frac_decided"] = {str(L): (ls == L).to(torch.float64).mean().item() for L in stages}
                for L, dec in fx.items():
                    ms = timed(lambda: dec.decode_device(x, out_bits=out), dec, args.reps)
                    row[f"frames_per_s_fixed_L{L}"] = B / ms * 1e3
                    row[f"fer_fixed_L{L}"] = fer(dec, out, u, cnt) / B
                row["speedup_vs_fixed_Lmax"] = row["frames_per_s_adaptive"] / row[f"frames_per_s_fixed_L{stages[-1]}"]
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
