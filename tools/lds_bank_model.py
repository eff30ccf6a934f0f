#!/usr/bin/env python3
"""Developer tool: LDS-array cycles per access of the pair kernel's LDS layouts (csrc/fast2_lds.h), on the CPU.

    python tools/lds_bank_model.py [--frames 64] [--samples 2000] [--seed 20] > profiles/r20_lds_bank_model.txt

The model is the banking rule of gfx950: a wave64 LDS instruction is served in fixed lane groups, one cycle per group, and
every further distinct address on a busy bank costs the group one more cycle (lanes with the same address broadcast).
    ds_read_b32 / ds_write_b32   2 groups of 32 lanes (0-31, 32-63)          bank = (a / 4) mod 32
    ds_read_b64                  2 groups of 32 lanes                        bank = (a / 4) mod 64, two dwords
    ds_read_b128                 4 groups of 16 lanes (0-3 12-15 20-27, 4-11 16-19 28-31, and the same + 32), four dwords
A lane of the pair kernel is lane = 8 p + 4 c + pos: slot p, codeword c, pos 0..3.

Rows (partial sums, [codeword][slot][32 words]): the old layout (every row at a multiple of 32 words) against
fast2_lds::row / cw_base, for the access classes of the kernel: the own row at one word, the own row at the window w0 + pos,
and a row by pointer (pb(t)) at one word / at a window, with the pointers of a list in which half of the slots were
re-filled by a fork from a random slot.

Table (staircase, 50 cells): a look-up reads thr and {T_lo, T_hi} of the cell of |x|.  The cells are sampled from the
check-node operands |a + b|, |a - b| of frames of the oracle's transmit chain at 2 dB, decoded with the oracle's decisions
as partial sums, in f64 and f32 arithmetic.  Wide steps (the levels 3 and up: a lane holds element pos + 4 r of its path's
node) and narrow chains (levels 2, 1, 0 inside an octet: 4, 2 and 1 distinct elements per path) separately.  The sixteen
paths of a wavefront are sixteen independent frames -- paths of one list share most of their values and broadcast more, so
the cycles of BOTH layouts are upper bounds.
    cells    48-byte cells, thr (8 / 4 bytes) at +0 and {T_lo, T_hi} (16 / 8 bytes) at +32            (polar_lut.h)
    arrays   thr[c], T_lo[c], T_hi[c], three reads of one element each, the arrays 257 elements apart (out of reach of a
             two-address read, so each stays a read of its own)
One instruction reads one array, so the base of an array only renames its banks: the tool prints the cycles over shifts of
the arrays against each other to show it.  The model counts LDS-array cycles only -- not the issue slot and the return of
a third instruction per look-up, which is why `arrays` wins here and lost on the GPU: the kernel
keeps `cells`."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

THR = (0.196, 0.433, 0.71, 1.05, 1.508, 2.252, 4.5)
TV = (0.65, 0.55, 0.45, 0.35, 0.25, 0.15, 0.05, 0.0)
G32 = [list(range(0, 32)), list(range(32, 64))]
_g16 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
G16 = _g16 + [[l + 32 for l in g] for g in _g16]
#        groups, banks, dwords
INSTR = {"b32": (G32, 32, 1), "b64": (G32, 64, 2), "b128": (G16, 64, 4)}

# ---- the layouts (csrc/fast2_lds.h; tests/test_fast2_lds_layout_host.py holds these to the header) ----
NW, SLOTS = 32, 8
ROW_STRIDE, CW_BASE = 36, 8 * 36 + 16
ROWS = {"old": lambda c, s: c * SLOTS * NW + s * NW, "new": lambda c, s: c * CW_BASE + s * ROW_STRIDE}
ARRAY_ELEMS = 257


def table_reads(layout, es):
    """[(instruction, byte offset of cell c -> address)] of one look-up; es = sizeof(R)"""
    if layout == "cells":
        return [("b64" if es == 8 else "b32", lambda c: 48 * c), ("b128" if es == 8 else "b64", lambda c: 48 * c + 32)]
    rd = "b64" if es == 8 else "b32"
    return [(rd, lambda c: es * c), (rd, lambda c: es * (ARRAY_ELEMS + c)), (rd, lambda c: es * (2 * ARRAY_ELEMS + c))]


def cycles(instr, addr):
    """LDS-array cycles of one wave instruction; addr[lane] = byte address, or -1 for a lane that takes no part"""
    groups, banks, dwords = INSTR[instr]
    total = 0
    for g in groups:
        per_bank = {}
        for lane in g:
            if addr[lane] < 0:
                continue
            for k in range(dwords):
                w = addr[lane] // 4 + k
                per_bank.setdefault(w % banks, set()).add(w)
        total += max([len(v) for v in per_bank.values()] + [1])
    return total


# ---- rows ----
def rows_model(rng, samples):
    """access class -> {layout: mean cycles of a ds_read_b32}"""
    out = {}
    lanes = [(l >> 3, (l >> 2) & 1, l & 3) for l in range(64)]
    for cls in ("own row, one word", "own row, window w0 + pos", "pointer row, one word", "pointer row, window"):
        res = {k: [] for k in ROWS}
        for _ in range(samples):
            w0 = int(rng.integers(0, NW - 3))
            ptr = np.tile(np.arange(SLOTS), (2, 1))
            refill = rng.random((2, SLOTS)) < 0.5
            ptr = np.where(refill, rng.integers(0, SLOTS, size=(2, SLOTS)), ptr)
            for k, row in ROWS.items():
                a = []
                for p, c, pos in lanes:
                    s = p if cls.startswith("own") else int(ptr[c, p])
                    a.append(4 * (row(c, s) + w0 + (pos if "window" in cls else 0)))
                res[k].append(cycles("b32", a))
        out[cls] = {k: float(np.mean(v)) for k, v in res.items()}
    return out


# ---- table ----
def cell_of(x):
    x = np.asarray(x)
    if x.dtype == np.float64:
        raw = ((x.view(np.uint64) >> np.uint64(49)) & np.uint64(0x3FFF)).astype(np.int64)
        bias = 0x3FC00000 >> 17
    else:
        raw = ((x.view(np.uint32) >> np.uint32(20)) & np.uint32(0x7FF)).astype(np.int64)
        bias = 0x3E000000 >> 20
    return np.clip(raw, bias - 1, bias + 48) - (bias - 1)


def chk(a, b):
    dt = a.dtype.type
    thr, tv = np.array(THR, dtype=dt), np.array(TV, dtype=dt)
    T = lambda x: tv[np.searchsorted(thr, np.abs(x), side="right")]  # noqa: E731
    sign = np.where(np.signbit(a) ^ np.signbit(b), dt(-1), dt(1))
    return sign * np.minimum(np.abs(a), np.abs(b)) + (T(a + b) - T(a - b))


def operands(llr, u):
    """level t -> [cells of |a + b|, cells of |a - b|], each [nodes][2^t] in leaf order, of the f steps that produce level t"""
    lev = {}

    def node(x, lo):
        n = len(x)
        if n == 1:
            return np.array([u[lo]], dtype=np.uint8)
        a, b = x[:n // 2], x[n // 2:]
        t = n.bit_length() - 2
        lev.setdefault(t, [[], []])
        lev[t][0].append(cell_of(a + b))
        lev[t][1].append(cell_of(a - b))
        xl = node(chk(a, b), lo)
        xr = node(np.where(xl == 1, b - a, b + a), lo + n // 2)
        return np.concatenate([xl ^ xr, xr])

    node(llr, 0)
    return {t: [np.stack(v[0]), np.stack(v[1])] for t, v in lev.items()}


def sample_frames(frames, seed, dtype):
    from oracle import oracle_py as O
    code = O.Code(1024, 512, O.CRC24C_TAPS)
    sig = O.sigma_from_db(2.0)
    _, ys = O.Sim(seed).frames(code, sig, frames)
    llr = np.stack([O.llr_from_y(y, sig) for y in ys]).astype(np.float64 if dtype == "f64" else np.float32)
    uh = O.decode(code, llr, "CASCL", L=8, dtype=dtype)[0]
    return [operands(llr[i], uh[i]) for i in range(frames)]


def table_model(ops, rng, samples, es, shifts=(0,)):
    """step class -> {layout: mean cycles per look-up (all its reads)}"""
    lanes = [(l >> 3, (l >> 2) & 1, l & 3) for l in range(64)]
    out = {}
    for cls, levels in (("wide steps", list(range(3, 10))), ("narrow chains", [2, 1, 0])):
        res = {}
        for _ in range(samples):
            t = int(rng.choice(levels))
            fr = rng.choice(len(ops), size=16, replace=False)
            which = int(rng.integers(0, 2))
            nn, width = ops[0][t][0].shape
            nd = int(rng.integers(0, nn))
            r = int(rng.integers(0, max(1, width // 4)))
            cells = []
            for p, c, pos in lanes:
                e = (4 * r + pos) if width >= 4 else (pos & (width - 1))
                cells.append(int(ops[fr[2 * p + c]][t][which][nd, e]))
            for lay in ("cells", "arrays"):
                for sh in shifts:
                    tot = 0
                    for k, (ins, f) in enumerate(table_reads(lay, es)):
                        tot += cycles(ins, [f(c) + 8 * sh * k for c in cells])
                    res.setdefault((lay, sh), []).append(tot)
        out[cls] = {k: float(np.mean(v)) for k, v in res.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    print(f"# tools/lds_bank_model.py --frames {args.frames} --samples {args.samples} --seed {args.seed}")
    print("## partial-sum rows: LDS-array cycles of one 4-byte access of the wavefront (2 = conflict-free)")
    for cls, v in rows_model(rng, args.samples).items():
        print(f"{cls:28s} old {v['old']:6.2f}   new {v['new']:6.2f}")
    for dtype, es in (("f64", 8), ("f32", 4)):
        ops = sample_frames(args.frames, args.seed, dtype)
        base = sum(INSTR[i][0].__len__() for i, _ in table_reads("cells", es)), sum(len(INSTR[i][0]) for i, _ in table_reads("arrays", es))
        print(f"## staircase table, {dtype}: LDS-array cycles of one look-up (conflict-free: cells {base[0]}, arrays {base[1]})")
        res = table_model(ops, rng, args.samples, es, shifts=tuple(range(0, 32, 4)))
        for cls, v in res.items():
            arr = [v[("arrays", sh)] for sh in range(0, 32, 4)]
            print(f"{cls:28s} cells {v[('cells', 0)]:6.2f}   arrays {v[('arrays', 0)]:6.2f}   (arrays shifted against each other by 0 .. 224 bytes: "
                  f"{min(arr):.2f} .. {max(arr):.2f})")


if __name__ == "__main__":
    main()
