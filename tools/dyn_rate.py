#!/usr/bin/env python3
"""Dynamic frozen bits (k_scl_dyn) next to the plain decoder, on one GPU (developer tool).

Throughput: on the same resident frames, polar_time_decode_device of k_scl_generic (forced through the testing library's
generic selection) against k_scl_dyn with D = 0 and with the PAC constraint set, for (N, L) = (128, 32) and (1024, 8), f64 and
f32 (--dtype).  The frames are the PAC code's, so the plain kernels decode them as if the constraints were not there: the
work per leaf is what is compared, not the decisions.

FER (--fer): polar_fer_batch over --frames frames per point, Eb/N0 = 1.0 .. 3.0 dB, of PAC(128, 64) L = 32 (rm profile),
5G polar (128, 64) SCL L = 32 and CA-SCL L = 32 with CRC-6.  One JSON line per row.

Wide lists (--L 32,64,128,256): instead of the rows above, PAC(128, 64) per list size -- frames/s of the context's own kernel
(k_scl_dyn up to L = 32, k_scl_wide above) on the same resident frames, and with --fer its FER at --dbs on identical frames
(the generator does not depend on L)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402
from polardecoding_amd import testing  # noqa: E402

SHAPES = ((128, 32), (1024, 8))
DBS = (1.0, 1.5, 2.0, 2.5, 3.0)


def wide_lists(args):
    N, K = 128, 64
    Ls = [int(v) for v in args.L.split(",")]
    for dts in args.dtype.split(","):
        dt = pa.F64 if dts == "f64" else pa.F32
        tdt = torch.float64 if dts == "f64" else torch.float32
        decs = {L: pa.PAC(N, K, L=L, dtype=dt) for L in Ls}
        B = args.rate_frames
        x = torch.empty((B, N), dtype=tdt, device="cuda")
        out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        decs[Ls[0]].generate_device(args.seed, 0, 2.0, x, None)
        decs[Ls[0]].synchronize()
        for L, dec in decs.items():
            dec.time_decode_device(x, out, 1)   # warm-up
            ms = dec.time_decode_device(x, out, args.reps)
            print(json.dumps({"dtype": dts, "N": N, "K": K, "L": L, "frames": B, "ebn0_db": 2.0, "kernel": dec.kernel_name,
                              "frames_per_s": B / ms * 1e3}), flush=True)
        if args.fer:
            for db in (float(v) for v in args.dbs.split(",")):
                row = {"dtype": dts, "N": N, "K": K, "frames": args.frames, "ebn0_db": db}
                for L, dec in decs.items():
                    blk, _ = dec.fer_batch(args.seed, 0, db, args.frames)
                    row[f"block_errors_L{L}"] = blk
                    row[f"fer_L{L}"] = blk / args.frames
                print(json.dumps(row), flush=True)
        for d in decs.values():
            d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f64,f32")
    ap.add_argument("--frames", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--fer", action="store_true")
    ap.add_argument("--L", default=None, help="list sizes, e.g. 32,64,128,256: PAC(128, 64) per list size")
    ap.add_argument("--dbs", default="1.5,2.0,2.5", help="Eb/N0 points of --L --fer")
    ap.add_argument("--rate-frames", type=int, default=1 << 14, help="resident frames of the --L rate rows")
    args = ap.parse_args()
    B = args.frames
    if args.L:
        return wide_lists(args)
    for dts in args.dtype.split(","):
        dt = pa.F64 if dts == "f64" else pa.F32
        tdt = torch.float64 if dts == "f64" else torch.float32
        for N, L in SHAPES:
            K = N // 2
            io = pa.pac_info_order(N, K)
            pac = pa.PAC(N, K, L=L, dtype=dt)
            d0 = pa.Decoder(N, K, pa.ALGO_SCL, L=L, dtype=dt, info_order=io, dyn=((), ()))
            gen = pa.Decoder(N, K, pa.ALGO_SCL, L=L, dtype=dt, info_order=io)
            testing.select_kernel(gen, testing.KERNEL_GENERIC)
            x = torch.empty((B, N), dtype=tdt, device="cuda")
            out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
            pac.generate_device(args.seed, 0, 2.0, x, None)
            pac.synchronize()
            row = {"dtype": dts, "N": N, "K": K, "L": L, "frames": B, "ebn0_db": 2.0}
            for name, dec in (("generic", gen), ("dyn_D0", d0), ("dyn_pac", pac)):
                dec.time_decode_device(x, out, 1)   # warm-up
                ms = dec.time_decode_device(x, out, args.reps)
                row[f"kernel_{name}"] = dec.kernel_name
                row[f"frames_per_s_{name}"] = B / ms * 1e3
            row["dyn_D0_over_generic"] = row["frames_per_s_dyn_D0"] / row["frames_per_s_generic"]
            row["dyn_pac_over_generic"] = row["frames_per_s_dyn_pac"] / row["frames_per_s_generic"]
            print(json.dumps(row), flush=True)
            for d in (pac, d0, gen):
                d.close()
        if args.fer:
            decs = {"pac_rm_L32": pa.PAC(128, 64, L=32, dtype=dt), "scl_5g_L32": pa.SCLdecode(128, 64, L=32, dtype=dt),
                    "cascl_crc6_L32": pa.CASCL(128, 64, L=32, crc_taps=pa.CRC6_TAPS, dtype=dt)}
            for db in DBS:
                row = {"dtype": dts, "N": 128, "K": 64, "frames": B, "ebn0_db": db}
                for name, dec in decs.items():
                    blk, _ = dec.fer_batch(args.seed, 0, db, B)
                    row[f"fer_{name}"] = blk / B
                print(json.dumps(row), flush=True)
            for d in decs.values():
                d.close()


if __name__ == "__main__":
    main()
