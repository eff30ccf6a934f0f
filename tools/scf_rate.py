#!/usr/bin/env python3
"""CRC-aided SC-Flip (POLAR_ALGO_SCF) against SC and fixed CA-SCL, on one GPU (developer tool).

N = 1024 / K = 512 / CRC-24C, f64 and f32 (--dtype), Eb/N0 = 1.0 .. 3.0 dB, on the same resident frames from
polar_generate_device: frames/s of one decode call (wall time of call + stream sync, mean over --reps calls after one
warm-up) and FER of SC-Flip with T = 4, 8, 16, 32, of SC over I[0..K+r) (k_sc_lanes) and of CA-SCL with L = 2, 4, 8.  Also
SC-Flip's pass A alone (T = 0: SC plus the CRC check) against SC, and the histogram of the attempt that decided each frame
(0 = plain SC; T counts the frames where no attempt passed).  One JSON line per (dtype, Eb/N0).

--budgets "8;8,16;8,16,32" adds dynamic SC-Flip (polar_scf_set_dynamic) with each budget list, once per --metric "c,tau"
pair ("1.5,5;0,0"): frames/s, FER and, per level, how many frames each rank of the level decided.  --ts picks the static T."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import polardecoding_amd as pa  # noqa: E402

N, K = 1024, 512
TS = (4, 8, 16, 32)
LS = (2, 4, 8)
DBS = (1.0, 1.5, 2.0, 2.5, 3.0)


def timed(fn, dec, reps):
    fn()   # warm-up
    dec.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        dec.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def fer(dec, out, u, cnt):
    cnt.zero_()
    torch.cuda.synchronize()
    dec.count_errors_device(out, u, cnt)
    dec.synchronize()
    return int(cnt[0].item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f64,f32")
    ap.add_argument("--dbs", default=",".join(str(d) for d in DBS))
    ap.add_argument("--frames", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--ts", default=",".join(str(t) for t in TS), help="static flip budgets")
    ap.add_argument("--budgets", default="", help="dynamic budget lists, ';' between lists: 8;8,16;8,16,32")
    ap.add_argument("--metric", default="1.5,5", help="c,tau pairs of the dynamic rule, ';' between pairs")
    args = ap.parse_args()
    ts = tuple(int(t) for t in args.ts.split(",") if t)
    budgets = [tuple(int(t) for t in b.split(",")) for b in args.budgets.split(";") if b]
    metrics = [tuple(float(v) for v in m.split(",")) for m in args.metric.split(";") if m]
    dbs = [float(v) for v in args.dbs.split(",")]
    B = args.frames
    for dts in args.dtype.split(","):
        dt = pa.F64 if dts == "f64" else pa.F32
        tdt = torch.float64 if dts == "f64" else torch.float32
        scf = {T: pa.SCFlip(N, K, T=T, dtype=dt) for T in (0,) + ts}
        top = scf[ts[0] if ts else 0]
        dyn = {(b, m): pa.DSCFlip(N, K, budgets=b, c=m[0], tau=m[1], dtype=dt) for b in budgets for m in metrics}
        sc = pa.Decoder(N, top.A, pa.ALGO_SC, dtype=dt, info_order=top.info_order)
        cascl = {L: pa.CASCL(N, K, L=L, dtype=dt) for L in LS}
        x = torch.empty((B, N), dtype=tdt, device="cuda")
        u = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
        at = torch.empty(B, dtype=torch.int32, device="cuda")
        fl = torch.empty(B, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for db in dbs:
            top.generate_device(args.seed, 0, db, x, u)
            top.synchronize()
            row = {"dtype": dts, "N": N, "K": K, "crc": "24C", "frames": B, "ebn0_db": db, "kernel_scf": top.kernel_name}
            ms = timed(lambda: sc.decode_device(x, out_bits=out), sc, args.reps)
            row["frames_per_s_sc"] = B / ms * 1e3
            row["fer_sc"] = fer(sc, out, u, cnt) / B
            ms = timed(lambda: scf[0].decode_scf_device(x, out_bits=out), scf[0], args.reps)
            row["frames_per_s_scf_pass_a"] = B / ms * 1e3
            row["pass_a_over_sc"] = row["frames_per_s_sc"] / row["frames_per_s_scf_pass_a"]
            for T in ts:
                dec = scf[T]
                ms = timed(lambda: dec.decode_scf_device(x, out_bits=out, flags=fl, attempts=at), dec, args.reps)
                row[f"frames_per_s_scf_T{T}"] = B / ms * 1e3
                row[f"fer_scf_T{T}"] = fer(dec, out, u, cnt) / B
                h = torch.bincount(at.to(torch.int64), minlength=T + 1).cpu().tolist()
                nopass = int(((fl & pa.FLAG_CRC_PASS) == 0).sum().item())
                h[T] -= nopass
                row[f"attempts_scf_T{T}"] = h   # h[t]: frames decided by attempt t (passing)
                row[f"no_pass_scf_T{T}"] = nopass
            for (b, (c, tau)), dec in dyn.items():
                tag = "dscf_" + "_".join(str(t) for t in b) + f"_c{c:g}_tau{tau:g}"
                ms = timed(lambda: dec.decode_scf_device(x, out_bits=out, flags=fl, attempts=at), dec, args.reps)
                row[f"frames_per_s_{tag}"] = B / ms * 1e3
                row[f"fer_{tag}"] = fer(dec, out, u, cnt) / B
                nopass = int(((fl & pa.FLAG_CRC_PASS) == 0).sum().item())
                h = torch.bincount(at.to(torch.int64), minlength=sum(b) + 1).cpu().tolist()
                h[sum(b)] -= nopass
                lv, lo = [], 1
                for t in b:   # per level: frames decided by its ranks 0 .. T_k - 1
                    lv.append(h[lo:lo + t])
                    lo += t
                row[f"attempts_{tag}"] = {"attempt0": h[0], "levels": lv, "no_pass": nopass}
            for L, dec in cascl.items():
                ms = timed(lambda: dec.decode_device(x, out_bits=out), dec, args.reps)
                row[f"frames_per_s_cascl_L{L}"] = B / ms * 1e3
                row[f"fer_cascl_L{L}"] = fer(dec, out, u, cnt) / B
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
