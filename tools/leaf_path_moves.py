#!/usr/bin/env python3
"""Developer tool: what the trivial-prune exit of every leaf of the pair kernel (csrc/scl_fast2.h) executes besides its
arithmetic -- register copies and scalar branches -- read from the ISA.

    python3 tools/leaf_path_moves.py [--kernel SUBSTR ...] [--asm FILE.s] [--src k_fast2] [--verbose]

Compiles csrc/k_fast2.hip with __graft_entry__.HIPCC_FLAGS (-S --cuda-device-only; or reads --asm), and in every kernel whose
mangled name contains one of SUBSTR (default: the two f64 LLR kernels, IddLb1E and IddLb0E of k_scl_fast2) finds the prune
sites: each v_permlane32_swap is the last step of trivial_prune()'s maximum, the conditional branch on vcc behind it is the
prune test.  From the side of that branch taken when no lane objects (vcc == 0) it walks the blocks up to the leaf's CRC
update (the first v_xor_b32) or the first bit-field instruction of its partial-sum update, whichever comes first, and counts

    VALU       vector ALU instructions on the path
    mov        v_mov_b32 / v_mov_b64 without DPP (a DPP move carries data between lanes and is not counted), of which
    b64        v_mov_b64, and
    copies     moves whose source is a register (the rest load constants)
    back       pairs "x <- y ... y <- x" on the path: a value copied away and back
    sbr        scalar branch instructions on the path

Branches whose condition is a flag register set to 0 / -1 earlier on the path (the structurizer's "Flow" blocks) are
followed as the flag says; at any other conditional branch both sides are walked and the side with more moves is reported
(marked "?").  Sites are listed in text order with the header of the loop that holds them; the kernel's totals (static
instructions, code bytes, VGPRs, spilled VGPRs, scratch accesses inside the octet loops) follow the table."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BR = re.compile(r"^(s_branch|s_cbranch_\w+)\s+(\S+)")
FLAGSET = re.compile(r"^s_mov_b64\s+(s\[\d+:\d+\]),\s*(0|-1)$")
FLAGTEST = re.compile(r"^s_(andn2|and)_b64\s+vcc,\s*exec,\s*(s\[\d+:\d+\])$")
BITFIELD = ("v_and_or_b32", "v_or3_b32", "v_bitop3_b32", "v_lshl_or_b32", "v_bfi_b32", "v_and_b32", "v_or_b32")


class Block:
    def __init__(self, name):
        self.name, self.ins, self.succ, self.loop = name, [], [], ""


def kernels(txt):
    """{mangled name: lines of its text}"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        out[m.group(1)] = m.group(2).splitlines()
    return out


def blocks_of(lines):
    """basic blocks in text order; an instruction is (line number in the kernel's text, text)"""
    blocks = [Block("entry")]
    for n, raw in enumerate(lines):
        s = raw.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        fall = re.match(r"^; %bb\.(\d+):", s)
        if m or fall:
            b = Block(m.group(1) if m else "bb." + fall.group(1))
            lm = re.search(r"Header=(BB\d+_\d+) Depth=(\d+)", s)
            if lm:
                b.loop = f"{lm.group(1)}/d{lm.group(2)}"
            blocks.append(b)
            continue
        if not s or s.startswith(";") or s.startswith("."):
            continue
        blocks[-1].ins.append((n, s.split(";")[0].strip()))
        if BR.match(blocks[-1].ins[-1][1]):     # a branch ends its block, label behind it or not
            blocks.append(Block(f"after.{n}"))
            blocks[-1].loop = blocks[-2].loop
    for i, b in enumerate(blocks):
        nxt = blocks[i + 1].name if i + 1 < len(blocks) else None
        b.succ = [nxt] if nxt else []
        for _, t in b.ins:
            m = BR.match(t)
            if m:
                b.succ = [m.group(2)] if m.group(1) == "s_branch" else [m.group(2), nxt]
            elif t.startswith("s_endpgm"):
                b.succ = []
    return blocks


def is_end(t, crc):
    # leaf 7's CRC update may be scheduled behind its partial-sum update: whichever comes first ends the path
    return t.startswith(BITFIELD) or (crc and t.startswith("v_xor_b32"))


def flags_before(blocks, b):
    """flag registers set to a constant on the way into block b: up the chain of single predecessors"""
    preds = {}
    for x in blocks:
        for s in x.succ:
            preds.setdefault(s, []).append(x)
    chain = []
    cur = b
    for _ in range(12):
        ps = preds.get(cur.name, [])
        if len(ps) != 1:
            break
        cur = ps[0]
        chain.append(cur)
    flags = {}
    for x in reversed(chain):
        for _, t in x.ins:
            m = FLAGSET.match(t)
            if m:
                flags[m.group(1)] = m.group(2)
            else:
                m = re.match(r"^s_\w+\s+(s\[\d+:\d+\])", t)
                if m and not FLAGTEST.match(t):
                    flags.pop(m.group(1), None)
    return flags


def walk(byname, start, crc, flags0, limit=40):
    """all paths from block `start` to the end marker; returns (path instructions, ambiguous) of the one with most moves"""
    best = None
    stack = [(start, [], dict(flags0), False, 0)]
    while stack:
        name, acc, flags, amb, depth = stack.pop()
        if name is None or depth > limit:
            continue
        b = byname[name]
        acc = list(acc)
        flags = dict(flags)
        test = None
        done = False
        for _, t in b.ins:
            acc.append(t)
            if is_end(t, crc):
                done = True
                break
            m = FLAGSET.match(t)
            if m:
                flags[m.group(1)] = m.group(2)
            elif re.match(r"^s_\w+\s+(s\[\d+:\d+\])", t) and not FLAGTEST.match(t):
                flags.pop(re.match(r"^s_\w+\s+(s\[\d+:\d+\])", t).group(1), None)
            m = FLAGTEST.match(t)
            if m:
                test = (m.group(1), flags.get(m.group(2)))
            elif re.match(r"^(v_cmp|s_cmp|s_bit|s_and|s_or|s_xor)", t) and not m:
                if re.search(r"\b(vcc|scc)\b", t) or t.startswith(("s_cmp", "s_bit", "v_cmp")):
                    test = None
        if done:
            nm = sum(1 for t in acc if plain_mov(t))
            if best is None or nm > best[2]:
                best = (acc, amb, nm)
            continue
        last = b.ins[-1][1] if b.ins else ""
        m = BR.match(last)
        if m and m.group(1) in ("s_cbranch_vccnz", "s_cbranch_vccz") and test and test[1] is not None:
            # vcc = exec & flag (and) or exec & ~flag (andn2)
            nz = (test[1] == "-1") if test[0] == "and" else (test[1] == "0")
            taken = nz if m.group(1) == "s_cbranch_vccnz" else not nz
            stack.append((b.succ[0] if taken else b.succ[1], acc, flags, amb, depth + 1))
        elif m and m.group(1) != "s_branch":
            for s in b.succ:
                stack.append((s, acc, flags, True, depth + 1))
        else:
            for s in b.succ:
                stack.append((s, acc, flags, amb, depth + 1))
    return best


def plain_mov(t):
    return re.match(r"^v_mov_b(32|64)(_e32|_e64)?\s", t) is not None


def site_rows(lines, crc):
    blocks = blocks_of(lines)
    byname = {b.name: b for b in blocks}
    rows = []
    for b in blocks:
        for k, (n, t) in enumerate(b.ins):
            if not t.startswith("v_permlane32_swap"):
                continue
            tail = [x for _, x in b.ins[k:]]
            br = BR.match(tail[-1])
            cmp_ = next((x for x in tail if x.startswith("v_cmp")), "?")
            if not br or br.group(1) not in ("s_cbranch_vccz", "s_cbranch_vccnz"):
                rows.append((n, b.loop, cmp_, None))
                continue
            start = b.succ[0] if br.group(1) == "s_cbranch_vccz" else b.succ[1]
            rows.append((n, b.loop, cmp_ + " ; " + tail[-1], walk(byname, start, crc, flags_before(blocks, b))))
    return rows


def report(name, lines, meta, verbose):
    crc = "Lb1E" in name
    print(f"{name}   (path ends at {'the CRC update or ' if crc else ''}the first bit-field instruction of the partial-sum update)")
    print(f"  {'site':>4} {'line':>6} {'loop':>12} {'VALU':>5} {'mov':>4} {'b64':>4} {'copies':>6} {'back':>4} {'sbr':>4}")
    for i, (n, loop, how, res) in enumerate(site_rows(lines, crc)):
        if res is None:
            print(f"  {i + 1:4d} {n:6d} {loop:>12}   no path found ({how})")
            continue
        acc, amb, _ = res
        movs = [t for t in acc if plain_mov(t)]
        pairs = []
        for t in movs:
            m = re.match(r"^\S+\s+(v\[\d+:\d+\]|v\d+),\s*(v\[\d+:\d+\]|v\d+)$", t)
            if m:
                pairs.append((m.group(1), m.group(2)))
        back = sum(1 for k, (d, s) in enumerate(pairs) if (s, d) in pairs[:k])
        print(f"  {i + 1:4d} {n:6d} {loop:>12} {sum(1 for t in acc if t.startswith('v_')):5d} {len(movs):4d} "
              f"{sum(1 for t in movs if t.startswith('v_mov_b64')):4d} {len(pairs):6d} {back:4d} "
              f"{sum(1 for t in acc if BR.match(t)):4d}{' ?' if amb else ''}")
        if verbose:
            print(f"         prune test: {how}")
            for t in acc:
                print("           " + t)
    ins = [t.strip().split(";")[0].strip() for t in lines]
    ins = [t for t in ins if t and not t.startswith((".", ";")) and not re.match(r"^\S+:$", t)]
    sl, ss = sum(t.startswith("scratch_load") for t in ins), sum(t.startswith("scratch_store") for t in ins)
    # the octet loops: the loops that hold prune sites
    loops = {loop.split("/")[0] for _, loop, _, _ in site_rows(lines, crc) if loop}
    inl = [0, 0]
    cur = ""
    for raw in lines:
        s = raw.strip()
        lm = re.search(r"Header=(BB\d+_\d+) Depth", s)
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", s):
            cur = lm.group(1) if lm else ""
        elif cur in loops and s.startswith("scratch_load"):
            inl[0] += 1
        elif cur in loops and s.startswith("scratch_store"):
            inl[1] += 1
    print(f"  instructions {len(ins)}, code bytes {meta.get('size', '?')}, vgpr {meta.get('vgpr', '?')}, "
          f"spilled {meta.get('spill', '?')}, scratch_load / scratch_store {sl} / {ss}, inside the loops of the prune "
          f"sites ({', '.join(sorted(loops))}) {inl[0]} / {inl[1]}, plain v_mov {sum(plain_mov(t) for t in ins)} "
          f"(b64 {sum(t.startswith('v_mov_b64') for t in ins)})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="append", help="substring of the mangled kernel name (repeatable)")
    ap.add_argument("--asm", help="read this .s instead of compiling")
    ap.add_argument("--src", default="k_fast2", help="translation unit in csrc/ (without .hip)")
    ap.add_argument("--verbose", action="store_true", help="print the instructions of every path")
    args = ap.parse_args()
    subs = args.kernel or ["11k_scl_fast2IddLb1E", "11k_scl_fast2IddLb0E"]
    if args.asm:
        txt = open(args.asm).read()
    else:
        import __graft_entry__ as g
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k.s")
            subprocess.check_call([g._hipcc()] + g.HIPCC_FLAGS + ["-S", "--cuda-device-only", "-o", out,
                                                                  os.path.join(g.CSRC, args.src + ".hip")], cwd=g.CSRC)
            txt = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt):
        meta[m.group(1)] = {"vgpr": m.group(2), "spill": m.group(3)}
    names = list(kernels(txt).items())
    sizes = re.findall(r"^; codeLenInByte = (\d+)", txt, re.M)
    for (name, lines), size in zip(names, sizes + ["?"] * len(names)):
        if any(s in name for s in subs):
            report(name, lines, dict(meta.get(name, {}), size=size), args.verbose)


if __name__ == "__main__":
    main()
