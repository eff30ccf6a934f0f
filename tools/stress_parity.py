#!/usr/bin/env python3
"""Differential sweep GPU (through the C ABI) vs the CPU oracle over many shapes: every kernel family, list sizes,
code lengths, rates, CRCs, both arithmetic types, ragged batch sizes.  Developer tool (tests/ holds the fixed cases).
--patterns: every configuration on a frozen set of tests/frozen_patterns.py (picked by the tool's rng) instead of the 5G set.
--dyn FAMILY: instead of the sweep above, k_scl_dyn against the numpy model of tests/test_dyn_host.py (bits, metric, flags by
==, tie frames included) on a constraint family of tests/dyn_families.py, at larger B than tests/test_gpu_dyn_families.py.
--wide: instead of the sweep above, k_scl_wide at L = 128 / 256 against the same model on the cases of tests/wide_families.py
(groups w1 .. w7) with the seed given here and --wide-scale times the frames of tests/test_gpu_wide_families.py."""
import argparse, itertools, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import polardecoding_amd as pa
from oracle import oracle_py as O
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import frozen_patterns as FP

ap = argparse.ArgumentParser()
ap.add_argument("seed", nargs="?", type=int, default=2026, help="another seed: other batch sizes and frames")
ap.add_argument("--inputs", choices=("gaussian", "grid", "hard"), default="gaussian",
                help="grid: LLRs rounded to step 1, clipped to +-7; hard: +-1 with the channel sign (dense with ties)")
ap.add_argument("--patterns", action="store_true",
                help="a frozen set outside the 5G order (tests/frozen_patterns.py) per configuration, K = its size less the CRC")
ap.add_argument("--dyn", choices=("pac", "all_prev", "bern_half"), default=None,
                help="dynamic frozen bits: this constraint family on the PAC rm mask, against the numpy model")
ap.add_argument("--wide", action="store_true",
                help="wide lists: the cases of tests/wide_families.py with this seed, against the numpy model")
ap.add_argument("--wide-scale", type=int, default=4, help="--wide: frames per case, as a multiple of the test's")
ap.add_argument("--wide-groups", default="w1,w2,w3,w4,w5,w6,w7", help="--wide: the groups to run")
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
bad = 0
t0 = time.time()


def dyn_sweep(family):
    """k_scl_dyn == dscl_model on every frame, N = 32 .. 1024, L = 1 .. 32, f64 and f32"""
    global bad
    import dyn_families as DF
    for N, L, dtype in itertools.product((32, 64, 128, 1024), (1, 2, 8, 32), ("f64", "f32")):
        mask, io = DF.mask_of(N, "rm")
        dyn = DF.constraint_families(N, mask, args.seed)[family]
        B = int(rng.integers(40, 90)) if N == 1024 else int(rng.integers(300, 1200))
        _, llr = DF.M.make_frames(N, io, dyn, B, int(rng.integers(1, 1 << 30)), dbs=(0.0, 1.0, 2.0, 3.0))
        llr = llr.astype(np.float32).astype(np.float64)
        if args.inputs == "grid":
            llr = np.clip(np.rint(llr), -7, 7)
        elif args.inputs == "hard":
            llr = np.where(np.signbit(llr), -1.0, 1.0)
        npdt = np.float32 if dtype == "f32" else np.float64
        want = DF.M.dscl_model(mask, dyn, llr, L, dtype=npdt)
        dec = pa.Decoder(N, N // 2, pa.ALGO_SC if L == 1 else pa.ALGO_SCL, L=L, dtype=pa.F32 if dtype == "f32" else pa.F64,
                         info_order=io, dyn=dyn)
        uh, pm, fl = dec.decode_batch(llr)
        ok = np.array_equal(uh, want[0]) and np.array_equal(pm, want[1]) and np.array_equal(np.asarray(fl).view(np.uint32), want[2])
        ties = int((want[2] & 1).sum())
        print(f"{'ok ' if ok else 'BAD'} dyn {family:9s} N={N:4d} L={L:2d} {dtype} {dec.kernel_name[:30]:30s} B={B:4d} tie-frames={ties}",
              flush=True)
        bad += (not ok)
        dec.close()


def wide_sweep(scale):
    """k_scl_wide == dscl_model on every frame of every case of wide_families.cases() but the work-queue rows"""
    global bad
    import wide_families as WF
    WF.SEED = args.seed
    for c in WF.cases():
        if c.group not in args.wide_groups.split(","):
            continue
        c = c._replace(B=c.B * scale)
        made, (ref, tr) = WF.materialise(c), WF.reference(c)
        K = made.order.size - (max(made.taps) if made.taps else 0)
        dec = pa.Decoder(c.N, K, pa.ALGO_CASCL if made.taps else pa.ALGO_SCL, L=c.L, crc_taps=made.taps,
                         dtype=pa.F32 if c.dtype == "f32" else pa.F64, info_order=made.order, dyn=made.dyn)
        for name, rows in made.batches.items():
            uh, pm, fl = dec.decode_batch(np.asarray(rows, dtype=np.float64))
            want = ref[name]
            ok = np.array_equal(uh, want[0]) and np.array_equal(pm, want[1]) and np.array_equal(np.asarray(fl).view(np.uint32), want[2])
            t = tr[name]
            print(f"{'ok ' if ok else 'BAD'} wide {WF.tag(c):52s} {name:16s} {dec.kernel_name[:28]:28s} tie={int(t['tie'].sum())} "
                  f"unrefilled={int(t['unrefilled'].sum())} cross={int(t['cross'].sum())} all-equal={int(t['all_equal'].sum())}", flush=True)
            bad += (not ok)
        dec.close()


if args.wide:
    wide_sweep(args.wide_scale)
    print(f"{bad} mismatching batches, {time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)

if args.dyn:
    dyn_sweep(args.dyn)
    print(f"{bad} mismatching configurations, {time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)


def q_of(dec, N, K, taps):
    io = dec.info_order.tolist()
    s = set(io)
    return [j for j in range(N) if j not in s] + io


def pat(N, K, taps=None):
    """(K, constructor keywords, tag suffix): unchanged by default; --patterns: a family that can carry the CRC"""
    if not args.patterns:
        return K, {}, ""
    r = max(taps) if taps else 0
    fam = [(k, m) for k, m in FP.families(N).items() if int((m == 0).sum()) > r]
    name, mask = fam[int(rng.integers(len(fam)))]
    order = FP.order_of(mask, args.seed)
    return order.size - r, {"info_order": order}, " " + name


def check(tag, dec, code, algo, L, B, db, dtype, iters=20):
    global bad
    sim = O.Sim(int(rng.integers(1, 1 << 30)))
    sig = O.sigma_from_db(db)
    us, ys = sim.frames(code, sig, B)
    llr = np.stack([O.llr_from_y(y, sig) for y in ys]).astype(np.float32).astype(np.float64)
    if args.inputs == "grid":
        llr = np.clip(np.rint(llr), -7, 7)
    elif args.inputs == "hard":
        llr = np.where(np.signbit(llr), -1.0, 1.0)
    ref, rpm, _ = O.decode(code, llr, algo, L=L, bp_iters=iters, dtype=dtype)
    uh, pm, fl = dec.decode_batch(llr)
    ok = np.array_equal(uh, ref) and (dtype == "f32" or algo in ("SC", "BP") or np.array_equal(pm, rpm))
    nerr = int((uh != us).any(axis=1).sum())
    print(f"{'ok ' if ok else 'BAD'} {tag:48s} {dec.kernel_name[:34]:34s} B={B:4d} frames-in-error={nerr}", flush=True)
    bad += (not ok)


for dtype in ("f64", "f32"):
    dt = pa.F64 if dtype == "f64" else pa.F32
    # list decoders
    for N, L in itertools.product((512, 1024, 2048, 4096), (2, 4, 8, 16, 32)):
        for K, taps in ((N // 2, pa.CRC24C_TAPS), (N // 4, None), (3 * N // 4, pa.CRC6_TAPS)):
            if N == 4096 and L >= 16 and K != N // 2:
                continue
            K, kw, fam = pat(N, K, taps)
            dec = pa.CASCL(N, K, L=L, crc_taps=taps, dtype=dt, **kw) if taps else pa.SCLdecode(N, K, L=L, dtype=dt, **kw)
            code = O.Code(N, K, taps, Q=q_of(dec, N, K, taps))
            B = int(rng.integers(3, 9)) if N * L >= 32768 else int(rng.integers(5, 20))
            check(f"{'CASCL' if taps else 'SCL'} N={N} K={K} L={L} r={max(taps) if taps else 0} {dtype}{fam}", dec, code,
                  "CASCL" if taps else "SCL", L, B, 1.5 if K * 2 <= N else 3.5, dtype)
    for N, L in itertools.product((32, 64, 128, 256), (1, 2, 8, 32)):
        K, kw, fam = pat(N, N // 2)
        dec = pa.SCLdecode(N, K, L=L, dtype=dt, **kw)
        code = O.Code(N, K, None, Q=q_of(dec, N, K, None))
        check(f"SCL N={N} K={K} L={L} {dtype}{fam}", dec, code, "SCL", L, int(rng.integers(5, 40)), 2.0, dtype)
    # SC: lanes kernel (B >= 64) and the generic one (B < 64)
    for N in (32, 64, 128, 256, 512, 1024, 2048):
        for K in (max(1, N // 8), N // 2, N - N // 8):
            K, kw, fam = pat(N, K)
            dec = pa.SCdecode(N, K, dtype=dt, **kw)
            code = O.Code(N, K, None, Q=q_of(dec, N, K, None))
            for B in (int(rng.integers(1, 63)), int(rng.integers(64, 200))):
                check(f"SC N={N} K={K} {dtype}{fam}", dec, code, "SC", 1, B, 2.0 if K * 2 <= N else 5.0, dtype)
    # the four tuned L = 8 kernels for N = 1024 side by side (one, two, four codewords per wavefront; big-list kernel)
    from polardecoding_amd import testing as T
    for variant in ("AUTO", "ONE_PER_WAVE", "FOUR_PER_WAVE", "BIG"):
        for K, taps in ((512, pa.CRC24C_TAPS), (256, None), (768, pa.CRC6_TAPS), (1000, None), (24, None)):
            K, kw, fam = pat(1024, K, taps)
            dec = pa.CASCL(1024, K, L=8, crc_taps=taps, dtype=dt, **kw) if taps else pa.SCLdecode(1024, K, L=8, dtype=dt, **kw)
            T.select_kernel(dec, getattr(T, "KERNEL_" + variant))
            code = O.Code(1024, K, taps, Q=q_of(dec, 1024, K, taps))
            check(f"{variant} N=1024 K={K} r={max(taps) if taps else 0} {dtype}{fam}", dec, code, "CASCL" if taps else "SCL", 8,
                  int(rng.integers(1, 40)), 1.5 if K <= 512 else 4.5, dtype)
    # BP (N = 1024: the register-blocked kernel, several rates and iteration counts)
    for N, K, it in ((32, 16, 7), (128, 64, 20), (512, 256, 11), (1024, 512, 6), (1024, 200, 13), (1024, 900, 50), (2048, 1024, 4),
                     (4096, 2048, 3)):   # above 1024: rows in global scratch
        K, kw, fam = pat(N, K)
        dec = pa.BP(N, K, iterMax=it, dtype=dt, **kw)
        code = O.Code(N, K, None, Q=q_of(dec, N, K, None))
        check(f"BP N={N} K={K} it={it} {dtype}{fam}", dec, code, "BP", 1, int(rng.integers(3, 12)), 2.0 if K * 2 <= N else 5.0, dtype, iters=it)
print(f"{bad} mismatching configurations, {time.time() - t0:.0f} s")
sys.exit(1 if bad else 0)
