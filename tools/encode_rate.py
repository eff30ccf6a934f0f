#!/usr/bin/env python3
"""Encoder side and systematic polar mode on one GPU (developer tool).

  rates   frames/s of polar_transform_device, polar_encode_device and polar_payload_device at N = 128, 1024, 4096 (CA-SCL
          contexts, CRC-24C, K = N / 2; wall time of call + stream sync, mean over --reps calls after a warm-up), and the
          transform's bytes/s over the 2 N / 8 bytes per frame it must move;
  fer     frames/s of polar_fer_batch with systematic mode off and on (CA-SCL N = 1024 L = 8);
  curves  FER and BER of both modes for SC N = 1024 K = 512 and CA-SCL L = 8 at 1.0 .. 2.5 dB, --curve-frames per point.
One JSON line per measurement.  The kernels' own times come from `rocprofv3 --kernel-trace --stats -- python
tools/encode_rate.py --only rates`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, sync, reps):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def rates(args, out):
    import torch
    import polardecoding_amd as pa
    B = args.frames
    for N in (128, 1024, 4096):
        K = N // 2
        for sys_polar in (False, True):
            d = pa.CASCL(N, K, L=8, sys_polar=sys_polar)
            pay = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, (K + 31) // 32), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()   # torch's stream filled the payload; the context runs on its own
            u, x = d.encode_device(pay)
            t_enc = timed(lambda: d._lib.polar_encode_device(d._h, pay.data_ptr(), B, u.data_ptr(), x.data_ptr()),
                          d.synchronize, args.reps)
            back = torch.empty_like(pay)
            ok = torch.empty(B, dtype=torch.int32, device="cuda")
            t_pay = timed(lambda: d._lib.polar_payload_device(d._h, u.data_ptr(), B, back.data_ptr(), ok.data_ptr()),
                          d.synchronize, args.reps)
            rec = {"what": "rates", "N": N, "K": K, "crc": "24c", "sys_polar": int(sys_polar), "frames": B,
                   "encode_frames_per_s": B / t_enc, "payload_frames_per_s": B / t_pay,
                   "round_trip_ok": bool(torch.equal(back, pay) and bool((ok == 1).all()))}
            if not sys_polar:
                t_x = timed(lambda: d._lib.polar_transform_device(d._h, u.data_ptr(), B, x.data_ptr()), d.synchronize, args.reps)
                rec["transform_frames_per_s"] = B / t_x
                rec["transform_bytes_per_s"] = B * 2 * N / 8 / t_x
            emit(rec, out)
            d.close()


def fer(args, out):
    import polardecoding_amd as pa
    B = args.frames
    for sys_polar in (False, True):
        d = pa.CASCL(1024, 512, L=8, sys_polar=sys_polar)
        t = timed(lambda: d.fer_batch(1, 0, 2.0, B), d.synchronize, args.reps)
        emit({"what": "fer_batch", "N": 1024, "K": 512, "L": 8, "sys_polar": int(sys_polar), "frames": B,
              "frames_per_s": B / t}, out)
        d.close()


def curves(args, out):
    import polardecoding_amd as pa
    F = args.curve_frames
    for algo, make in (("sc", lambda s: pa.SCdecode(1024, 512, sys_polar=s)), ("cascl", lambda s: pa.CASCL(1024, 512, L=8, sys_polar=s))):
        decs = {s: make(s) for s in (False, True)}
        for db in (1.0, 1.5, 2.0, 2.5):
            rec = {"what": "curve", "algo": algo, "N": 1024, "K": 512, "snr_db": db, "frames": F}
            for s, d in decs.items():
                blk, bits = d.fer_batch(7, 0, db, F)
                tag = "sys" if s else "plain"
                rec["fer_" + tag] = blk / F
                rec["ber_" + tag] = bits / (F * d.A)   # bit errors over the K + r positions compared
            rec["ber_ratio"] = rec["ber_sys"] / rec["ber_plain"] if rec["ber_plain"] else None
            emit(rec, out)
        for d in decs.values():
            d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 16)
    ap.add_argument("--curve-frames", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="rates,fer,curves")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    for name in args.only.split(","):
        {"rates": rates, "fer": fer, "curves": curves}[name](args, out)


if __name__ == "__main__":
    main()
