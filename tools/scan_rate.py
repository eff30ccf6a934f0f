#!/usr/bin/env python3
"""Soft-output SCAN (POLAR_ALGO_SCAN) against BP (50 round trips) and SC, on one GPU (developer tool).

N = 1024 / K = 512 and N = 128 / K = 64, no CRC, f64 and f32 (--dtype), on the same resident frames from
polar_generate_device: frames/s from polar_time_decode_device (device events around --reps decodes after one warm-up) and
FER of SCAN with I = 1, 2, 4 iterations, of BP with 50 round trips and of SC.  One JSON line per (N, dtype, Eb/N0)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402

ITERS = (1, 2, 4)
SHAPES = ((1024, 512), (128, 64))


def measure(dec, x, out, u, cnt, reps):
    dec.decode_device(x, out_bits=out)   # warm-up: scratch allocation, first launch
    dec.synchronize()
    ms = dec.time_decode_device(x, out, reps)
    cnt.zero_()
    torch.cuda.synchronize()
    dec.count_errors_device(out, u, cnt)
    dec.synchronize()
    B = x.shape[0]
    return B / ms * 1e3, int(cnt[0].item()) / B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f64,f32")
    ap.add_argument("--dbs", default="2.0")
    ap.add_argument("--frames", type=int, default=1 << 17)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bp-iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=2026)
    args = ap.parse_args()
    B = args.frames
    for N, K in SHAPES:
        for dts in args.dtype.split(","):
            dt = pa.F64 if dts == "f64" else pa.F32
            tdt = torch.float64 if dts == "f64" else torch.float32
            scan = {i: pa.SCAN(N, K, iters=i, dtype=dt) for i in ITERS}
            bp = pa.BP(N, K, iterMax=args.bp_iters, dtype=dt)
            sc = pa.SCdecode(N, K, dtype=dt)
            x = torch.empty((B, N), dtype=tdt, device="cuda")
            u = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
            out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            for db in (float(v) for v in args.dbs.split(",")):
                sc.generate_device(args.seed, 0, db, x, u)
                sc.synchronize()
                row = {"dtype": dts, "N": N, "K": K, "frames": B, "ebn0_db": db, "kernel_scan": scan[ITERS[-1]].kernel_name}
                row["frames_per_s_sc"], row["fer_sc"] = measure(sc, x, out, u, cnt, args.reps)
                row[f"frames_per_s_bp{args.bp_iters}"], row[f"fer_bp{args.bp_iters}"] = measure(bp, x, out, u, cnt, args.reps)
                for i in ITERS:
                    row[f"frames_per_s_scan_I{i}"], row[f"fer_scan_I{i}"] = measure(scan[i], x, out, u, cnt, args.reps)
                print(json.dumps(row), flush=True)
            del x, u, out, scan, bp, sc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
