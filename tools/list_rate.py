#!/usr/bin/env python3
"""List output (include/polar_hip.h, "List output") on one GPU (developer tool).  One JSON line per row.

Rates, on resident frames, timed with events on the decoder's stream over --reps launches after a warm-up:
  * polar_list_decode next to the ordinary decode of the same context and next to the ordinary decode of the dynamic
    (D = 0 where the code has no dynamic bits) context of the same cfg, which runs the same kernel body with the one-path
    epilogue: N = 1024, K = 512, CRC-24C, L = 8; PAC(128, 64) with L = 32 and L = 128;
  * polar_list_select (M = 4), polar_list_gather and polar_list_soft (both domains) on the lists.
Containment (--fer): per Eb/N0 in --dbs, the share of frames whose sent word is a member of the list, next to the frame error
rate of the ordinary decode on the same frames."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402


def configs(dt):
    q = pa.q_sequence(1024)
    return [
        ("cascl1024_L8", lambda: pa.CASCL(1024, 512, L=8, dtype=dt),
         lambda: pa.Decoder(1024, 512, pa.ALGO_CASCL, L=8, crc_taps=pa.CRC24C_TAPS, dtype=dt, info_order=q[1024 - 536:], dyn=((), ()))),
        ("pac128_L32", lambda: pa.PAC(128, 64, L=32, dtype=dt), None),
        ("pac128_L128", lambda: pa.PAC(128, 64, L=128, dtype=dt), None),
    ]


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
    ap.add_argument("--fer", action="store_true")
    ap.add_argument("--dbs", default="1.0,1.5,2.0,2.5")
    ap.add_argument("--only", default=None, help="comma-separated config names")
    args = ap.parse_args()
    B = args.frames
    for dts in args.dtype.split(","):
        dt = pa.F64 if dts == "f64" else pa.F32
        tdt = torch.float64 if dts == "f64" else torch.float32
        for name, make, make_dyn in configs(dt):
            if args.only and name not in args.only.split(","):
                continue
            dec = make()
            dec.use_torch_stream()
            N, L, NW = dec.N, dec.L, dec.NW
            x = torch.empty((B, N), dtype=tdt, device="cuda")
            u = torch.empty((B, NW), dtype=torch.int32, device="cuda")
            out = torch.empty((B, NW), dtype=torch.int32, device="cuda")
            dec.generate_device(args.seed, 0, 2.0, x, u)
            dec.synchronize()
            row = {"config": name, "dtype": dts, "N": N, "K": dec.K, "L": L, "frames": B, "ebn0_db": 2.0, "kernel": dec.kernel_name}
            row["decode_frames_per_s"] = B / timed(dec, lambda: dec.decode_device(x, out_bits=out), args.reps) * 1e3
            if make_dyn is not None:
                d0 = make_dyn()
                d0.use_torch_stream()
                row["dyn_kernel"] = d0.kernel_name
                row["dyn_decode_frames_per_s"] = B / timed(d0, lambda: d0.decode_device(x, out_bits=out), args.reps) * 1e3
                d0.close()
            else:
                row["dyn_decode_frames_per_s"] = row["decode_frames_per_s"]   # the context is the dynamic one
            last = {}

            def run_list():
                last["out"] = dec.decode_list_device(x)
            ms = timed(dec, run_list, args.reps)
            row["list_frames_per_s"] = B / ms * 1e3
            row["list_over_dyn_decode"] = row["list_frames_per_s"] / row["dyn_decode_frames_per_s"]
            row["list_bytes_per_frame"] = L * N // 8 + 12 * L + 8
            paths, pm, rem, count, flags = last["out"]
            masks = torch.arange(4, dtype=torch.int32, device="cuda")
            idx = dec.list_select_device(rem, count, masks)
            row["select_M4_frames_per_s"] = B / timed(dec, lambda: dec.list_select_device(rem, count, masks), args.reps) * 1e3
            row["gather_frames_per_s"] = B / timed(dec, lambda: dec.list_gather_device(paths, idx[:, 0]), args.reps) * 1e3
            for dom, key in ((0, "soft_u"), (1, "soft_x")):
                ms = timed(dec, lambda: dec.list_soft_device(paths, pm, count, domain=dom, clamp=64.0), args.reps)
                row[key + "_frames_per_s"] = B / ms * 1e3
                row[key + "_out_GB_per_s"] = B * N * 8 / ms / 1e6
            print(json.dumps(row), flush=True)
            if args.fer:
                for db in (float(v) for v in args.dbs.split(",")):
                    dec.generate_device(args.seed + 1, 0, db, x, u)
                    paths, _, _, count, _ = dec.decode_list_device(x, want_pm=False, want_rem=False, want_flags=False)
                    dec.decode_device(x, out_bits=out)
                    dec.synchronize()
                    live = torch.arange(L, device="cuda")[None, :] < count[:, None]
                    member = ((paths == u[:, None, :]).all(dim=2) & live).any(dim=1)
                    err = (out != u).any(dim=1)
                    print(json.dumps({"config": name, "dtype": dts, "ebn0_db": db, "frames": B,
                                      "sent_word_in_list": float(member.float().mean()), "list_miss_rate": float(1 - member.float().mean()),
                                      "fer": float(err.float().mean())}), flush=True)
            dec.close()


if __name__ == "__main__":
    main()
