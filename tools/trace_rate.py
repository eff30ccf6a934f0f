#!/usr/bin/env python3
"""Sent-path trace (include/polar_hip.h, "Sent-path trace") on one GPU (developer tool).  One JSON line per configuration.

On generated frames (generate_device -> trace_list_device -> trace_count_device) at --db: the class split (correct, selection
error, list loss), the ten leaves with most losses, the rate of the trace next to polar_list_decode of the same context (events
on the decoder's stream over --reps launches after a warm-up), and the host-side comparison of tools/list_rate.py --fer on the
same frames (the whole list copied out and compared row by row), which the trace's class 2 count must equal.
Configurations: PAC(128, 64) at L = 32, 64, 128, 256 and CA-SCL N = 1024, K = 512, CRC-24C, L = 8."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402


def configs(dt):
    out = [("pac128_L%d" % L, (lambda L=L: pa.PAC(128, 64, L=L, dtype=dt))) for L in (32, 64, 128, 256)]
    return out + [("cascl1024_L8", lambda: pa.CASCL(1024, 512, L=8, dtype=dt))]


def timed(dec, fn, reps):
    """milliseconds per call of fn() on the decoder's stream (torch's current stream)"""
    fn()
    dec.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--frames", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--db", type=float, default=2.0)
    ap.add_argument("--only", default=None, help="comma-separated config names")
    args = ap.parse_args()
    B = args.frames
    for dts in args.dtype.split(","):
        dt = pa.F64 if dts == "f64" else pa.F32
        tdt = torch.float64 if dts == "f64" else torch.float32
        for name, make in configs(dt):
            if args.only and name not in args.only.split(","):
                continue
            dec = make()
            dec.use_torch_stream()
            N, L, NW = dec.N, dec.L, dec.NW
            x = torch.empty((B, N), dtype=tdt, device="cuda")
            u = torch.empty((B, NW), dtype=torch.int32, device="cuda")
            dec.generate_device(args.seed, 0, args.db, x, u)
            hist = torch.zeros(N + 4, dtype=torch.int64, device="cuda")
            loss_leaf, loss_rank, rank, chosen, flags = dec.trace_list_device(x, u)
            dec.trace_count_device(loss_leaf, rank, chosen, hist)
            dec.synchronize()
            h = hist.cpu().numpy()
            top = sorted(((int(h[j]), j) for j in range(N) if h[j]), reverse=True)[:10]
            row = {"config": name, "dtype": dts, "N": N, "K": dec.K, "L": L, "frames": B, "ebn0_db": args.db, "reps": args.reps,
                   "correct": int(h[N]), "selection_error": int(h[N + 1]), "list_loss": int(h[N + 2]),
                   "top_loss_leaves": [[j, c] for c, j in top]}
            lost = loss_rank[loss_leaf < N].float()
            row["mean_loss_rank_over_L"] = float((lost[lost > 0] / L).mean()) if (lost > 0).any() else None
            # the same statistic the slow way: the whole list to the host, rows compared there
            paths, _, _, count, _ = dec.decode_list_device(x, want_pm=False, want_rem=False, want_flags=False)
            dec.synchronize()
            hp, hu, hc = paths.cpu(), u.cpu(), count.cpu()
            member = ((hp == hu[:, None, :]).all(dim=2) & (torch.arange(L)[None, :] < hc[:, None])).any(dim=1)
            row["host_list_miss"] = int((~member).sum())
            row["host_bytes_per_frame"] = L * N // 8
            row["trace_bytes_per_frame"] = 20
            row["agree"] = row["host_list_miss"] == row["list_loss"]
            ms_list = timed(dec, lambda: dec.decode_list_device(x), args.reps)
            ms_trace = timed(dec, lambda: dec.trace_list_device(x, u), args.reps)
            ms_count = timed(dec, lambda: dec.trace_count_device(loss_leaf, rank, chosen, hist), args.reps)
            row["list_frames_per_s"] = B / ms_list * 1e3
            row["trace_frames_per_s"] = B / ms_trace * 1e3
            row["trace_over_list"] = ms_list / ms_trace
            row["count_us"] = ms_count * 1e3
            print(json.dumps(row), flush=True)
            dec.close()


if __name__ == "__main__":
    main()
