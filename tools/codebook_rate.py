#!/usr/bin/env python3
"""Code books (include/polar_hip.h, "Code books") on one GPU (developer tool).  One JSON line per row.

Everything runs on torch's current stream and is timed with events over --reps calls after a warm-up, end to end (every
launch of a call counts):
  (a) the cost of the per-frame descriptor: a C = 1 code book against the dynamic-context kernel (k_scl_dyn, D = 0) and the
      list call against polar_list_decode of the same cfg: N = 1024, K = 512, CRC-24C, L = 8, --frames frames, f32 and f64;
  (b) a search-space mix: A = 40 + 24 (CRC-24C) at E = 108, 216, 432, 864, 1728 (N by polar_rm_select_n(A, E, 9)), L = 8, f32,
      44 k frames for k in --slots split 16 / 12 / 8 / 4 / 4 over the five codes: one code-book call against five
      polar_decode_device calls (each member's own kernel behind k_rm_recover);
  (c) the recovery in the load stage against k_rm_recover followed by the same kernel on N-wide rows: C = 1 books of one
      rate-matched member (N = 512, E = 864 and E = 432, ibil on) and of the plain member with the same information set."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402


def timed(fn, reps):
    """milliseconds per call of fn() on torch's current stream"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def part_a(args):
    q = pa.q_sequence(1024)
    B = args.frames
    for dts in ("f32", "f64"):
        dt, tdt = (pa.F32, torch.float32) if dts == "f32" else (pa.F64, torch.float64)
        dec = pa.CASCL(1024, 512, L=8, dtype=dt)
        dyn = pa.Decoder(1024, 512, pa.ALGO_CASCL, L=8, crc_taps=pa.CRC24C_TAPS, dtype=dt, info_order=q[1024 - 536:], dyn=((), ()))
        cb = pa.Codebook([dec])
        for o in (dec, dyn, cb):
            o.use_torch_stream()
        x = torch.empty((B, 1024), dtype=tdt, device="cuda")
        out = torch.empty((B, 32), dtype=torch.int32, device="cuda")
        code = torch.zeros(B, dtype=torch.int32, device="cuda")
        dec.generate_device(args.seed, 0, 2.0, x, None)
        row = {"part": "a", "dtype": dts, "frames": B, "kernel": cb.kernel_name, "dyn_kernel": dyn.kernel_name}
        row["dyn_decode_frames_per_s"] = B / timed(lambda: dyn.decode_device(x, out_bits=out), args.reps) * 1e3
        row["book_decode_frames_per_s"] = B / timed(lambda: cb.decode_device(x, code, out_bits=out), args.reps) * 1e3
        row["list_frames_per_s"] = B / timed(lambda: dec.decode_list_device(x), args.reps) * 1e3
        row["book_list_frames_per_s"] = B / timed(lambda: cb.decode_list_device(x, code), args.reps) * 1e3
        row["book_over_dyn"] = row["book_decode_frames_per_s"] / row["dyn_decode_frames_per_s"]
        row["book_list_over_list"] = row["book_list_frames_per_s"] / row["list_frames_per_s"]
        print(json.dumps(row), flush=True)
        for o in (cb, dyn, dec):
            o.close()


def part_b(args):
    Es, share = (108, 216, 432, 864, 1728), (16, 12, 8, 4, 4)
    decs = [pa.Decoder(pa.rm_select_n(64, E, 9), 40, pa.ALGO_CASCL, L=8, crc_taps=pa.CRC24C_TAPS, dtype=pa.F32, E=E) for E in Es]
    cb = pa.Codebook(decs)
    for o in decs + [cb]:
        o.use_torch_stream()
    for k in (int(v) for v in args.slots.split(",")):
        B = 44 * k
        code_h = np.random.default_rng(args.seed).permutation(np.repeat(np.arange(5), [s * k for s in share])).astype(np.int32)
        rows = torch.zeros((B, cb.W_max), dtype=torch.float32, device="cuda")
        own, outs = [], []
        for c, d in enumerate(decs):
            n = share[c] * k
            x = torch.empty((n, d.E), dtype=torch.float32, device="cuda")
            d.generate_device(args.seed + c, 0, 2.0, x, None)
            rows[torch.from_numpy(np.flatnonzero(code_h == c)).cuda(), :d.E] = x
            own.append(x)
            outs.append(torch.empty((n, d.NW), dtype=torch.int32, device="cuda"))
        code = torch.from_numpy(code_h).cuda()
        out = torch.empty((B, cb.NW), dtype=torch.int32, device="cuda")

        def five():
            for d, x, o in zip(decs, own, outs):
                d.decode_device(x, out_bits=o)
        ms_five = timed(five, args.reps)
        ms_book = timed(lambda: cb.decode_device(rows, code, out_bits=out), args.reps)
        print(json.dumps({"part": "b", "slots": k, "frames": B, "N": [d.N for d in decs], "E": list(Es),
                          "member_kernels": [d.kernel_name for d in decs], "kernel": cb.kernel_name,
                          "five_calls_us": ms_five * 1e3, "book_call_us": ms_book * 1e3, "five_over_book": ms_five / ms_book}),
              flush=True)
    for o in [cb] + decs:
        o.close()


def part_c(args):
    B = args.frames
    for E in (864, 432):
        rm = pa.Decoder(512, 40, pa.ALGO_CASCL, L=8, crc_taps=pa.CRC24C_TAPS, dtype=pa.F32, E=E, ibil=True)
        plain = pa.Decoder(512, 40, pa.ALGO_CASCL, L=8, crc_taps=pa.CRC24C_TAPS, dtype=pa.F32, info_order=rm.info_order)
        cb_rm, cb_plain = pa.Codebook([rm]), pa.Codebook([plain])
        for o in (rm, plain, cb_rm, cb_plain):
            o.use_torch_stream()
        x = torch.empty((B, E), dtype=torch.float32, device="cuda")
        rm.generate_device(args.seed, 0, 2.0, x, None)
        code = torch.zeros(B, dtype=torch.int32, device="cuda")
        out = torch.empty((B, 16), dtype=torch.int32, device="cuda")
        wide = rm.rm_recover_device(x)

        def two():
            rm.rm_recover_device(x, out=wide)
            cb_plain.decode_device(wide, code, out_bits=out)
        ms_two = timed(two, args.reps)
        ms_fused = timed(lambda: cb_rm.decode_device(x, code, out_bits=out), args.reps)
        ms_plain = timed(lambda: cb_plain.decode_device(wide, code, out_bits=out), args.reps)
        print(json.dumps({"part": "c", "N": 512, "E": E, "mode": rm.rm_mode, "ibil": True, "frames": B,
                          "recover_then_book_us": ms_two * 1e3, "fused_book_us": ms_fused * 1e3, "plain_book_us": ms_plain * 1e3,
                          "two_over_fused": ms_two / ms_fused}), flush=True)
        for o in (cb_rm, cb_plain, plain, rm):
            o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--slots", default="1,16,256")
    ap.add_argument("--parts", default="a,b,c")
    args = ap.parse_args()
    for p in args.parts.split(","):
        {"a": part_a, "b": part_b, "c": part_c}[p](args)


if __name__ == "__main__":
    main()
