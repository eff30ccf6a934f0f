#!/usr/bin/env python3
"""5G rate matching (polar_create_rm) against the plain decoder, on one GPU (developer tool).

N = 1024, CA-SCL L = 8 / CRC-24C and SC, f64 and f32, channel interleaver off and on, at the (K, E) points
  K = 512: E = 1024 (repetition, one term: the plain code's order), 864 (shortening), 2048 (repetition, two terms);
  K = 200: E = 864 (puncturing, 4E >= 3N), 640 (puncturing, 4E < 3N).
Frames come from polar_generate_device at --snr (the rate-matched generator writes [B][E]).  Per point: frames/s of one
decode call (wall time of call + stream sync, mean over --reps calls after a warm-up), the same for the plain context of
that K and CRC at E = N, frames/s of polar_rm_recover_device alone, and the FER.  One JSON line per (dtype, algo, K, E,
ibil).

--stats DB --points K:E: read the rocpd database that `rocprofv3 --kernel-trace --stats -o NAME` wrote for a run of this
tool at that one point and print one JSON line with the times of k_rm_recover<double / float>, k_generate_rm and
k_generate, and the recovery's achieved bandwidth over the bytes it must move, (E + N) * sizeof(IN) per frame."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 1024
POINTS = ((512, 1024), (512, 864), (512, 2048), (200, 864), (200, 640))


def timed(fn, sync, reps):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        sync()
    return (time.perf_counter() - t0) / reps


def make(pa, algo, K, dtype, **kw):
    if algo == "cascl":
        return pa.CASCL(N, K, L=8, dtype=dtype, **kw)
    return pa.SCdecode(N, K, dtype=dtype, **kw)


def run(args):
    import torch
    import polardecoding_amd as pa
    B = args.frames
    out = open(args.out, "a") if args.out else None
    for dname, dtype, tdt in (("f64", pa.F64, torch.float64), ("f32", pa.F32, torch.float32)):
        if dname not in args.dtypes:
            continue
        for algo in args.algos:
            plain_rate = {}
            for K, E in args.points:
                if K not in plain_rate:
                    p = make(pa, algo, K, dtype)
                    x = torch.empty((B, N), dtype=tdt, device="cuda")
                    p.generate_device(1, 0, args.snr, x)
                    bits = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
                    t = timed(lambda: p.decode_device(x, out_bits=bits), p.synchronize, args.reps)
                    plain_rate[K] = (B / t, p.kernel_name)
                    p.close()
                    del x
                for ibil in (False, True):
                    d = make(pa, algo, K, dtype, E=E, ibil=ibil)
                    x = torch.empty((B, E), dtype=tdt, device="cuda")
                    u = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
                    d.generate_device(1, 0, args.snr, x, u_bits=u)
                    bits = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
                    rows = torch.empty((B, N), dtype=tdt, device="cuda")
                    t_dec = timed(lambda: d.decode_device(x, out_bits=bits), d.synchronize, args.reps)
                    t_rec = timed(lambda: d.rm_recover_device(x, out=rows), d.synchronize, args.reps)
                    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
                    d.decode_device(x, out_bits=bits)
                    d.count_errors_device(bits, u, cnt)
                    d.synchronize()
                    rec = {"dtype": dname, "algo": algo, "N": N, "K": K, "E": E, "ibil": int(ibil), "mode": d.rm_mode,
                           "frames": B, "snr_db": args.snr, "kernel": d.kernel_name,
                           "frames_per_s_rm": B / t_dec, "frames_per_s_plain_E_eq_N": plain_rate[K][0],
                           "rm_over_plain": (B / t_dec) / plain_rate[K][0],
                           "frames_per_s_recover_only": B / t_rec,
                           "recover_wall_bytes_per_s": B * (E + N) * (8 if dname == "f64" else 4) / t_rec,
                           "fer": int(cnt[0].item()) / B}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
                    d.close()
                    del x, rows


def stats(args):
    """per-launch times from the rocpd database of `rocprofv3 --kernel-trace -o NAME` (its `kernels` view); launches of the
    same kernel are told apart by their frame count through the LDS size and by the chunk the decode path uses"""
    import sqlite3
    (K, E), = args.points
    db = sqlite3.connect(args.stats)
    rec = {"source": "rocprofv3 --kernel-trace (rocpd kernels view)", "K": K, "E": E, "N": N, "frames": args.frames}
    for k, esz in (("k_rm_recover<double>", 8), ("k_rm_recover<float>", 4), ("k_generate_rm", 0), ("k_generate(", 0)):
        d = sorted(r[0] for r in db.execute("select duration from kernels where name like ?", ("%" + k + "%",)))
        if not d:
            continue
        med = d[len(d) // 2]
        rec[k.rstrip("(") + "_median_ns"] = med
        rec[k.rstrip("(") + "_min_ns"] = d[0]
        rec[k.rstrip("(") + "_launches"] = len(d)
        if esz:   # the decode path's chunks hold min(B, 256 MiB / (N * esz)) frames
            chunk = min(args.frames, (256 << 20) // (N * esz))
            rec[k + "_frames_per_chunk"] = chunk
            rec[k + "_chunk_bytes_per_s"] = chunk * (E + N) * esz / (d[0] * 1e-9)
            rec[k + "_ns_per_frame"] = d[0] / chunk
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--snr", type=float, default=2.0)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--algos", default="cascl,sc")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--stats", default=None, help="rocpd database of a profiled run: print kernel times instead")
    ap.add_argument("--points", default=None, help="K:E,K:E,... instead of the default points")
    args = ap.parse_args()
    args.algos = args.algos.split(",")
    args.dtypes = args.dtypes.split(",")
    args.points = [tuple(int(v) for v in p.split(":")) for p in args.points.split(",")] if args.points else list(POINTS)
    if args.stats:
        stats(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
