#!/usr/bin/env python3
"""BP early termination (stop rule G, polar_bp_set_stop) against the fixed-iteration decoder, on one GPU (developer tool).

For N = 1024 / K = 512 with iterMax 50 and 100 and N = 128 / K = 64 with iterMax 100, in f64 and f32, and at Eb/N0 = 1.0 ..
3.0 dB: frames/s of one polar_bp_decode_device launch with POLAR_BP_STOP_NONE and with POLAR_BP_STOP_G (HIP events,
mean over --reps launches on the same resident frames), the mean and maximum round trips per frame under G, and the FER
of both rules.  Inputs come from polar_generate_device (random payloads, BPSK + AWGN), as in tools/bench_configs.py.
One JSON line per (config, dtype, Eb/N0).  per_round_trip_cost = (ms_G / mean iterations) / (ms_NONE / iterMax) - 1: what
the check adds to one round trip once the shorter frames are accounted for."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402

CONFIGS = [("BP_1024_50it", 1024, 512, 50, 1 << 16), ("BP_1024_100it", 1024, 512, 100, 1 << 16),
           ("BP_128_100it", 128, 64, 100, 1 << 18)]
DBS = (1.0, 1.5, 2.0, 2.5, 3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--dtype", default="f64,f32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    for name, N, K, iters, B in CONFIGS:
        if args.only and args.only not in name:
            continue
        for dts in args.dtype.split(","):
            dt = pa.F64 if dts == "f64" else pa.F32
            tdt = torch.float64 if dts == "f64" else torch.float32
            dec = pa.BP(N, K, iterMax=iters, dtype=dt)
            x = torch.empty((B, N), dtype=tdt, device="cuda")
            u = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
            out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
            it = torch.empty(B, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            for db in DBS:
                dec.generate_device(args.seed, 0, db, x, u)
                row = {"config": name, "dtype": dts, "N": N, "K": K, "iterMax": iters, "frames": B, "ebn0_db": db}
                for rule in ("none", "g"):
                    dec.set_bp_stop(rule)
                    dec.decode_bp_device(x, out_bits=out, iters=it)   # warm-up, and the decisions counted below
                    cnt.zero_()
                    torch.cuda.synchronize()
                    dec.count_errors_device(out, u, cnt)
                    dec.synchronize()
                    blk = int(cnt[0].item())
                    ms = dec.time_decode_device(x, out, args.reps)
                    row[f"kernel_{rule}"] = dec.kernel_name
                    row[f"ms_{rule}"] = ms
                    row[f"frames_per_s_{rule}"] = B / ms * 1e3
                    row[f"fer_{rule}"] = blk / B
                    if rule == "g":
                        itc = it.to(torch.float64)
                        row["mean_iters_g"] = itc.mean().item()
                        row["max_iters_g"] = int(it.max().item())
                        row["frac_stopped_early"] = (it < iters).to(torch.float64).mean().item()
                row["speedup_g"] = row["frames_per_s_g"] / row["frames_per_s_none"]
                row["per_round_trip_cost"] = (row["ms_g"] / row["mean_iters_g"]) / (row["ms_none"] / iters) - 1
                dec.set_bp_stop(None)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
