#!/usr/bin/env python3
"""Fixed-point min-sum (dtype Q8) against the f32 context of the same cfg, on one GPU (developer tool).

(a) frames/s from polar_time_decode_device (device events around --reps decodes after a warm-up) at B = --frames resident
    f32 rows of polar_generate_device at 2.0 dB, for SC N = 1024, SCL L = 32 N = 1024, CA-SCL L = 8 N = 1024 (CRC-24C) and
    CA-SCL L = 8 N = 128 (CRC-6).  The Q8 figure includes the quantiser kernel (rule 7: float rows in).  f32 and Q8 are
    timed alternately, --rounds times; the line carries the median and the extremes of each.
(b) FER of CA-SCL L = 8 N = 1024 at --dbs with --fer-frames frames per point (polar_fer_batch), for f32 and for Q8 with the
    default quantiser, scale 1 / 2 / 4 and (qc, qi) = (5, 6) / (6, 8).
One JSON line per configuration (a) and per (Eb/N0, decoder) (b)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402

RATE_CFGS = (
    ("sc_1024", lambda dt: pa.SCdecode(1024, 512, dtype=dt)),
    ("scl_1024_l32", lambda dt: pa.SCLdecode(1024, 512, L=32, dtype=dt)),
    ("cascl_1024_l8", lambda dt: pa.CASCL(1024, 512, L=8, dtype=dt)),
    ("cascl_128_l8", lambda dt: pa.CASCL(128, 64, L=8, crc_taps=pa.CRC6_TAPS, dtype=dt)),
)
QUANTS = (("q8 default (2,8,8)", None), ("q8 scale 1", (1.0, 8, 8)), ("q8 scale 2", (2.0, 8, 8)), ("q8 scale 4", (4.0, 8, 8)),
          ("q8 (qc,qi)=(5,6)", (2.0, 5, 6)), ("q8 (qc,qi)=(6,8)", (2.0, 6, 8)))


def rates(args):
    B = args.frames
    for name, mk in RATE_CFGS:
        f32, q8 = mk(pa.F32), mk(pa.Q8)
        N = f32.N
        x = torch.empty((B, N), dtype=torch.float32, device="cuda")
        u = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f32.generate_device(args.seed, 0, 2.0, x, u)
        f32.synchronize()
        for dec in (f32, q8):      # warm-up: scratch, first launch
            dec.decode_device(x, out_bits=out)
            dec.synchronize()
        fps = {"f32": [], "q8": []}
        for _ in range(args.rounds):
            for key, dec in (("f32", f32), ("q8", q8)):
                fps[key].append(B / dec.time_decode_device(x, out, args.reps) * 1e3)
        row = {"part": "rate", "cfg": name, "frames": B, "reps": args.reps, "rounds": args.rounds,
               "kernel_f32": f32.kernel_name, "kernel_q8": q8.kernel_name}
        for key in ("f32", "q8"):
            row[f"frames_per_s_{key}"] = statistics.median(fps[key])
            row[f"frames_per_s_{key}_min_max"] = [min(fps[key]), max(fps[key])]
        row["q8_over_f32"] = row["frames_per_s_q8"] / row["frames_per_s_f32"]
        print(json.dumps(row), flush=True)
        del x, u, out, f32, q8
        torch.cuda.empty_cache()


def fers(args):
    decs = [("f32", pa.CASCL(1024, 512, L=8, dtype=pa.F32))]
    for label, quant in QUANTS:
        decs.append((label, pa.CASCL(1024, 512, L=8, dtype=pa.Q8, quant=quant)))
    for db in (float(v) for v in args.dbs.split(",")):
        for label, dec in decs:
            blk = bits = 0
            done = 0
            while done < args.fer_frames:      # every decoder sees the same frames: (seed, frame index)
                nb = min(args.batch, args.fer_frames - done)
                b0, b1 = dec.fer_batch(args.seed, done, db, nb)
                blk, bits, done = blk + b0, bits + b1, done + nb
            print(json.dumps({"part": "fer", "cfg": "cascl_1024_l8", "decoder": label, "ebn0_db": db, "frames": done,
                              "block_errors": blk, "fer": blk / done, "bit_errors": bits}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dbs", default="1.5,2.0,2.5")
    ap.add_argument("--fer-frames", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=1 << 17)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--skip", default="", help="rate or fer")
    args = ap.parse_args()
    if args.skip != "rate":
        rates(args)
    if args.skip != "fer":
        fers(args)


if __name__ == "__main__":
    main()
