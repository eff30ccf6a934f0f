"""Developer tool: the launch shapes of the persistent kernels (csrc/polar_host.h plan_launch()), for comparing two builds.

    rocprofv3 --kernel-trace --output-format csv -d OUT_A -- python3 tools/launch_shapes.py [ROOT_A]
    rocprofv3 --kernel-trace --output-format csv -d OUT_B -- python3 tools/launch_shapes.py [ROOT_B]
    python3 tools/launch_shapes.py --compare OUT_A OUT_B

The first form decodes, for every launcher that goes through plan_launch(), one batch below the resident job count and one
above it (without and with the work queue), from the checkout at ROOT (default: this one).  --compare reads the two kernel
traces and compares them dispatch by dispatch: kernel name, grid, workgroup, LDS_Block_Size (profiles/r10_launch_shapes.txt)."""
import csv
import glob
import os
import sys


def load(d):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    assert len(f) == 1, (d, f)
    rows = list(csv.DictReader(open(f[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"]),
             int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"]), int(r["LDS_Block_Size"])) for r in rows]


def compare(da, db):
    a, b = load(da), load(db)
    diff = sum(1 for x, y in zip(a, b) if x != y) + abs(len(a) - len(b))
    ours = [x for x in a if "polar::" in x[0]]
    print(f"A: {len(a)} dispatches, B: {len(b)}; of the library's kernels {len(ours)}; differing dispatches: {diff}")
    print("kernel | grid (work-items) | workgroup | LDS_Block_Size   -- the library's dispatches in order")
    for x, y in zip(a, b):
        if "polar::" in x[0] or "polar::" in y[0]:
            nm = x[0].replace("void ", "")
            nm = nm[:nm.index("(")] if "(" in nm else nm
            print(f"{nm} | {x[1]} | {x[2]} | {x[3]}" + ("" if x == y else f"   != {y}"))
    return 1 if diff else 0


if len(sys.argv) > 1 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch
import polardecoding_amd as pa
from polardecoding_amd import testing as T

CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)
CRC6 = (0, 1, 6)
rng = np.random.default_rng(11)
_base = {}


def rows(B, N, f32=False, snr_db=1.0):
    """all-zero codeword over BPSK + AWGN as LLRs: 2048 host rows tiled on the device"""
    key = (N, f32)
    if key not in _base:
        sigma = 10 ** (-snr_db / 20)
        x = 2 * (1.0 + sigma * rng.standard_normal((2048, N))) / sigma / sigma
        _base[key] = torch.from_numpy(x.astype(np.float32 if f32 else np.float64)).cuda()
    b = _base[key]
    return b.repeat((B + 2047) // 2048, 1)[:B].contiguous()


def run(label, dec, Bs, variant=None, f32_in=False, how="decode_device"):
    if variant is not None:
        T.select_kernel(dec, variant)
    for B in Bs:
        x = rows(B, dec.N, f32_in)
        getattr(dec, how)(x)
        dec.synchronize()
        torch.cuda.synchronize()
        print(f"{label} B={B} {dec.kernel_name}", flush=True)
    dec.close()


F32 = pa.F32
# launch_fast
run("fast128_f64", pa.CASCL(128, 64, L=8, crc_taps=CRC6), (7, 70001))
run("fast128_f32", pa.CASCL(128, 64, L=8, crc_taps=CRC6, dtype=F32), (7, 70001), f32_in=True)
run("fast128_f32_in64", pa.SCLdecode(128, 64, L=8, dtype=F32), (7, 70001))
run("fast1024_one", pa.CASCL(1024, 512, L=8), (7, 6144 * 3 + 5), variant=T.KERNEL_ONE_PER_WAVE)
# launch_fast2
run("fast2_f64", pa.CASCL(1024, 512, L=8), (7, 6144 * 3 + 5))
run("fast2_f32", pa.SCLdecode(1024, 512, L=8, dtype=F32), (7, 6144 * 5 + 5), f32_in=True)
# launch_fast4
run("fast4_f64", pa.CASCL(1024, 512, L=8), (7, 6144 * 6 + 5), variant=T.KERNEL_FOUR_PER_WAVE)
run("fast4_f32", pa.CASCL(1024, 512, L=8, dtype=F32), (7, 6144 * 8 + 5), variant=T.KERNEL_FOUR_PER_WAVE, f32_in=True)
# launch_big_v, both translation units
run("big_f64_L32", pa.SCLdecode(1024, 512, L=32), (9, 4096 * 2 + 333))
run("big_f32_L32", pa.SCLdecode(1024, 512, L=32, dtype=F32), (9, 4096 * 3 + 333), f32_in=True)
run("big_f64_N2048", pa.CASCL(2048, 1024, L=32), (9, 3072 * 2 + 77))
run("big_f32_N2048", pa.CASCL(2048, 1024, L=32, dtype=F32), (9, 3072 * 3 + 77))
run("big_f64_L8", pa.CASCL(1024, 512, L=8), (9, 20011), variant=T.KERNEL_BIG)
run("big_f64_L2_N512", pa.SCLdecode(512, 256, L=2), (9, 60011))
# launch_sc_lanes
run("sc_f64", pa.SCdecode(1024, 512), (100, (1 << 18) + 777))
run("sc_f32_N256", pa.SCdecode(256, 128, dtype=F32), (100, (1 << 19) + 777), f32_in=True)
# launch_scf_lanes: pass A, record, pass B (frames at 1 dB fail SC often)
run("scf_f64", pa.SCFlip(1024, 512, T=8), (300, 200001), how="decode_scf_device")
run("scf_f32_T32", pa.SCFlip(2048, 1024, T=32, dtype=F32), (300,), how="decode_scf_device", f32_in=True)
# launch_genie_lanes
for dt, B in ((pa.F64, 100), (pa.F64, (1 << 18) + 777), (F32, 100)):
    dec = pa.SCdecode(1024, 512, dtype=dt)
    counts = torch.zeros(2, 1024, dtype=torch.int64, device="cuda")
    dec.genie_count_device(rows(B, 1024), counts)
    dec.synchronize()
    print(f"genie B={B}", flush=True)
    dec.close()
# launch_scan_lanes
run("scan_f64", pa.SCAN(1024, 512, iters=2), (100, 80001), how="decode_scan_device")
run("scan_f32_N128", pa.SCAN(128, 64, iters=2, dtype=F32), (100, 300001), how="decode_scan_device", f32_in=True)
# launch_scl_v: LDS and global-scratch variants
run("generic_L4", pa.SCLdecode(256, 128, L=4), (5, 30011))
run("generic_sc_small", pa.SCdecode(1024, 512), (5,))
run("generic_GA_L8", pa.CASCL(1024, 512, L=8), (5, 3001), variant=T.KERNEL_GENERIC_SPILL)
run("generic_GA_f32_L32", pa.SCLdecode(1024, 512, L=32, dtype=F32), (5, 3001), variant=T.KERNEL_GENERIC_SPILL, f32_in=True)
run("generic_N4096_L32", pa.CASCL(4096, 2048, L=32), (5,), variant=T.KERNEL_GENERIC)
# launch_dyn_v
run("dyn_pac128", pa.PAC(128, 64, L=32), (5, 30011))
run("dyn_pac1024_GA", pa.PAC(1024, 512, L=8), (5, 3001), variant=T.KERNEL_GENERIC_SPILL)
run("dyn_pc", pa.PCCASCL(64, 14, L=8, dtype=F32), (5, 100001), f32_in=True)
# launch_bp_r4, launch_bp_w128, launch_bp (LDS branch), with and without the stop rule
run("bp_r4", pa.BP(1024, 512, iterMax=5), (5, 768 * 4 + 19))
run("bp_r4_stop_f32", pa.BP(1024, 512, iterMax=5, early_stop="g", dtype=F32), (5, 768 * 8 + 19), f32_in=True)
run("bp_w128", pa.BP(128, 64, iterMax=5), (5, 4096 * 6 + 3))
run("bp_w128_stop", pa.BP(128, 64, iterMax=5, early_stop="g"), (5, 4096 * 6 + 3))
run("bp_lds_256", pa.BP(256, 128, iterMax=5), (5, 9001))
run("bp_lds_256_stop", pa.BP(256, 128, iterMax=5, early_stop="g"), (5, 9001))
run("bp_lds_1024_generic", pa.BP(1024, 512, iterMax=5), (5, 2001), variant=T.KERNEL_GENERIC)
print("done", flush=True)
