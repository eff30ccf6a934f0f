#!/usr/bin/env python3
"""Monte-Carlo construction (polar_genie_count_device, polar_construct_batch) on one GPU (developer tool).

Rates: for N in --sizes, f64 and f32, --frames design rows at --sigma: M frames/s of genie_count_device alone (rows
resident, of the ctx dtype), of construct_batch (rows generated into ctx scratch, then counted) and of the SC decoder of a
K = N/2 context (default order) on the same rows.  Wall time of call + stream sync, median over --reps calls after a warm-up.
One JSON line per (N, dtype).

--fer: frozen sets in use.  For each (algo, N, Eb/N0) of FER_POINTS: construct at that point with --mc-frames frames, then
FER over --fer-frames generated frames with the constructed information set and with the library's default order.  One JSON
line per point (block errors, FERs, overlap of the two information sets, seconds of the construction)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FER_POINTS = (("sc", 2048, 2.0), ("sc", 1024, 2.0), ("cascl8", 4096, 1.25))


def timed(fn, sync, reps):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def rates(args):
    import torch
    import polardecoding_amd as pa
    B = args.frames
    for N in args.sizes:
        for dname, dtype, tdt in (("f64", pa.F64, torch.float64), ("f32", pa.F32, torch.float32)):
            if dname not in args.dtypes:
                continue
            d = pa.SCdecode(N, N // 2, dtype=dtype)
            rows = torch.empty((B, N), dtype=tdt, device="cuda")
            d.genie_rows_device(1, 0, args.sigma, rows)
            cnt = torch.zeros((2, N), dtype=torch.int64, device="cuda")
            bits = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
            t_cnt = timed(lambda: d.genie_count_device(rows, cnt), d.synchronize, args.reps)
            t_all = timed(lambda: d.construct_batch(1, 0, args.sigma, B, cnt), d.synchronize, args.reps)
            t_row = timed(lambda: d.genie_rows_device(1, 0, args.sigma, rows), d.synchronize, args.reps)
            t_sc = timed(lambda: d.decode_device(rows, out_bits=bits), d.synchronize, args.reps)
            emit({"what": "rate", "N": N, "dtype": dname, "frames": B, "sigma": args.sigma, "reps": args.reps,
                  "mframes_per_s_genie_count": B / t_cnt / 1e6, "mframes_per_s_construct_batch": B / t_all / 1e6,
                  "mframes_per_s_genie_rows": B / t_row / 1e6, "mframes_per_s_sc_decode_K_half": B / t_sc / 1e6,
                  "genie_over_sc": t_sc / t_cnt, "sc_kernel": d.kernel_name}, args.out)
            d.close()
            del rows, bits


def fer(args):
    import polardecoding_amd as pa
    for algo, N, db in FER_POINTS:
        K = N // 2
        sigma = 10 ** (-db / 20)
        pa.construct_mc(N, sigma, 1 << 16, seed=2)
        t0 = time.perf_counter()
        order, _ = pa.construct_mc(N, sigma, args.mc_frames, seed=1)
        sec = time.perf_counter() - t0
        mk = (lambda **kw: pa.SCdecode(N, K, **kw)) if algo == "sc" else (lambda **kw: pa.CASCL(N, K, L=8, **kw))
        base = mk()
        A = base.A
        mc = mk(info_order=order[N - A:])
        rec = {"what": "fer", "algo": algo, "N": N, "K": K, "A": A, "design_db": db, "eval_db": db, "mc_frames": args.mc_frames,
               "mc_seconds": sec, "fer_frames": args.fer_frames, "base": "5G sequence" if N <= 1024 else "polarization weight",
               "info_set_overlap": len(set(order[N - A:].tolist()) & set(base.info_order.tolist()))}
        for name, dec in (("base", base), ("constructed", mc)):
            blk = 0
            for first in range(0, args.fer_frames, 1 << 16):
                blk += dec.fer_batch(77, first, db, min(1 << 16, args.fer_frames - first))[0]
            rec["block_errors_" + name] = blk
            rec["fer_" + name] = blk / args.fer_frames
            dec.close()
        emit(rec, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sigma", type=float, default=0.7943282347242815, help="design noise (default: 2.0 dB at rate 1/2)")
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--fer", action="store_true")
    ap.add_argument("--mc-frames", type=int, default=1 << 23)
    ap.add_argument("--fer-frames", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    args.sizes = [int(v) for v in args.sizes.split(",")]
    args.dtypes = args.dtypes.split(",")
    (fer if args.fer else rates)(args)


if __name__ == "__main__":
    main()
