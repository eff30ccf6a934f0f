"""Output extents of the device and host-buffer entry points (a plain helper module, imported by tests/test_extents_host.py,
tests/test_gpu_extents.py and tests/test_gpu_queue.py; no GPU is touched at import).

Every kernel that puts several frames into one wavefront or workgroup has a hand-written rule for the ragged last group.
A store for a frame at or beyond B lands in the slack of a 512-byte-rounded allocation or in a neighbouring tensor, and a
test that reads back rows [0, B) never sees it.  Here every output of a call is a view into one Arena: a flat byte buffer
filled with 0xA5, each view at the natural alignment of its element type and no more, with a guard in front and a guard
behind that is at least as large as one whole group of frames (and at least 4096 bytes).  A kernel that stored a phantom
group hits a guard and stays inside the arena's allocation.  CASES lists, per (entry point, kernel), the context, the
group width, the batch sizes around it and the outputs with their nullable marks; HOST_CASES the host-buffer forms.
Reads beyond the inputs are not covered: they cannot be seen without a fault."""
import os
import re
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_bpl import AD_CHUNK  # noqa: E402  (frames per compaction block, csrc/adaptive_kernel.h; imports no GPU package)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "polar_hip.h")

FILL = 0xA5
MIN_GUARD = 4096
CRC6 = (0, 5, 6)
CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)


def guard_bytes(dtype, rows_in_group, row_elems):
    """the least size of each guard of an output: a whole group of rows, and never below 4096 bytes"""
    return max(MIN_GUARD, int(rows_in_group) * int(row_elems) * np.dtype(dtype).itemsize)


def _torch_dtype(dtype):
    import torch
    name = {"uint32": "int32", "uint64": "int64"}.get(np.dtype(dtype).name, np.dtype(dtype).name)   # same bytes
    return getattr(torch, name)


class Arena:
    """One flat byte buffer filled with 0xA5; carve() hands out views with a guard on both sides, check() lists the guard
    bytes that changed.  backend "numpy" (host) or "torch" (uint8 on `device`)."""

    def __init__(self, backend="numpy", capacity=1 << 20, device="cuda"):
        self.backend, self.capacity = backend, int(capacity)
        if backend == "torch":
            import torch
            self.buf = torch.full((self.capacity,), FILL, dtype=torch.uint8, device=device)
            self.base = self.buf.data_ptr()
        elif backend == "numpy":
            self.buf = np.full(self.capacity, FILL, dtype=np.uint8)
            self.base = self.buf.ctypes.data
        else:
            raise ValueError(backend)
        self.cursor = 0
        self.spans = []   # (name, start of the front guard, start of the view, end of the view, end of the back guard)

    @staticmethod
    def need(specs):
        """capacity for carve(name, dtype, elems, rows_in_group, row_elems) over specs of (dtype, elems, rows_in_group,
        row_elems)"""
        return sum(2 * guard_bytes(d, g, r) + int(e) * np.dtype(d).itemsize + 32 for d, e, g, r in specs) + 32

    def carve(self, name, dtype, elems, rows_in_group=1, row_elems=1):
        """A view of exactly `elems` elements of `dtype`.  Its address is congruent to the element size modulo 16 (so it is
        aligned for its type and neither 16- nor 256-byte aligned); in front of it and behind it lie at least
        max(4096, rows_in_group * row_elems * itemsize) bytes of guard, shared with no other view."""
        dt = np.dtype(dtype)
        g = guard_bytes(dt, rows_in_group, row_elems)
        front = self.cursor
        start = front + g
        start += (dt.itemsize - (self.base + start)) % 16
        end = start + int(elems) * dt.itemsize
        if end + g > self.capacity:
            raise ValueError(f"arena of {self.capacity} bytes is too small for {name}")
        self.spans.append((name, front, start, end, end + g))
        self.cursor = end + g
        if self.backend == "numpy":
            return self.buf[start:end].view(dt)
        return self.buf[start:end].view(_torch_dtype(dt))

    def host(self):
        return self.buf if self.backend == "numpy" else self.buf.cpu().numpy()

    def check(self):
        """[(name, side, first byte offset)] for every guard with a byte other than 0xA5 ("front" / "behind"; the bytes beyond
        the last guard count as ("", "tail", offset)); empty when only the views were written"""
        h = self.host()
        out = []
        for name, front, start, end, back in self.spans:
            for side, a, b in (("front", front, start), ("behind", end, back)):
                bad = np.flatnonzero(h[a:b] != FILL)
                if bad.size:
                    out.append((name, side, a + int(bad[0])))
        bad = np.flatnonzero(h[self.cursor:] != FILL)
        if bad.size:
            out.append(("", "tail", self.cursor + int(bad[0])))
        return out

    def span(self, name):
        return next(s for s in self.spans if s[0] == name)


def snapshot(t):
    """the bytes of a numpy array or a torch tensor, copied to the host"""
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t).reshape(-1).view(np.uint8).copy()
    return t.contiguous().reshape(-1).cpu().numpy().view(np.uint8).copy()


def unchanged(t, snap):
    return np.array_equal(snapshot(t), snap)


Arena.snapshot = staticmethod(snapshot)
Arena.unchanged = staticmethod(unchanged)


# ---- the table ----------------------------------------------------------------------------------------------------------------
Out = namedtuple("Out", "name dtype per unit nullable acc")
Case = namedtuple("Case", "name entry ctx prefix group batches outputs ref opts")


def O(name, dtype, per, unit="frame", nullable=False, acc=False):
    """an output: `per` elements per frame (unit "frame") or per call ("call"); per is a number or a key of dims();
    acc: the call adds to what the buffer holds, so it is zeroed first"""
    return Out(name, dtype, per, unit, nullable, acc)


def ctx(kind, N, K, variant=None, **kw):
    return dict(kind=kind, N=N, K=K, variant=variant, kw=kw)


def dims(c):
    """the sizes an output may name, from the context's description alone"""
    N, K = c["N"], c["K"]
    E = c["kw"].get("E", N)
    n = N.bit_length() - 1
    return {"N": N, "NW": N // 32, "2N": 2 * N, "KW": (K + 31) // 32, "EW": (E + 31) // 32, "E_tab": 2 * (n + 1)}


def elems(out, c, B):
    per = out.per if isinstance(out.per, int) else dims(c)[out.per]
    return per * (B if out.unit == "frame" else 1)


def row_elems(out, c):
    return out.per if isinstance(out.per, int) else dims(c)[out.per]


def batches_of(G):
    """1, G - 1, G + 1, 2 G - 1 without duplicates and zeros"""
    return tuple(sorted({b for b in (1, G - 1, G + 1, 2 * G - 1) if b > 0}))


def make_ctx(c):
    """the library context of a description (the caller closes it)"""
    import polardecoding_amd as pa
    from polardecoding_amd import testing as T
    kw = dict(c["kw"])
    dt = kw.pop("dtype", "f64")
    kw["dtype"] = {"f64": pa.F64, "f32": pa.F32, "q8": pa.Q8}[dt]
    sys_polar = kw.pop("sys_polar", False)
    kind, N, K = c["kind"], c["N"], c["K"]
    if kind == "PAC":
        dec = pa.PAC(N, K, **kw)
    else:
        dec = {"SC": pa.SCdecode, "SCL": pa.SCLdecode, "CASCL": pa.CASCL, "BP": pa.BP, "SCF": pa.SCFlip, "DSCF": pa.DSCFlip,
               "BPL": pa.BPL, "SCAN": pa.SCAN}[kind](N, K, **kw)
    if c["variant"]:
        T.select_kernel(dec, getattr(T, c["variant"]))
    if sys_polar:
        dec.set_systematic(True)
    return dec


U4, I4, F8, F4, U8, I1 = "uint32", "int32", "float64", "float32", "uint64", "int8"
BITS = O("d_uhat_bits", U4, "NW")
PM = O("d_pm", F8, 1, nullable=True)
FLAGS = O("d_flags", U4, 1, nullable=True)
LIST3 = (BITS, PM, FLAGS)
BP3 = (BITS, O("d_iters", U4, 1, nullable=True), FLAGS)
SCF3 = (BITS, FLAGS, O("d_attempts", U4, 1, nullable=True))
ENC2 = (O("d_u_bits", U4, "NW", nullable=True), O("d_x_bits", U4, "EW", nullable=True))
PAY2 = (O("d_payload", U4, "KW"), O("d_crc_ok", U4, 1, nullable=True))


def _dev(name, c, prefix, group, batches, ref, outputs=LIST3, entry="polar_decode_device", **opts):
    return Case(name, entry, c, prefix, group, tuple(batches), tuple(outputs), ref, opts)


def _cases():
    out = []
    # the pair kernel: two frames per wavefront
    c1024 = dict(L=8, crc_taps=CRC24C)
    for algo, kw in (("CASCL", c1024), ("SCL", dict(L=8))):
        out.append(_dev(f"fast2 {algo} f64", ctx(algo, 1024, 512, **kw), "k_scl_fast2<", 2, (1, 3, 7), "list"))
        out.append(_dev(f"fast2_y {algo} f64", ctx(algo, 1024, 512, **kw), "k_scl_fast2<", 2, (1, 3, 7), "list", from_y=True))
    out.append(_dev("fast2 CASCL f32 on f32 rows", ctx("CASCL", 1024, 512, dtype="f32", **c1024), "k_scl_fast2<float", 2, (1, 3, 7),
                    "list", in_dtype="f32"))
    out.append(_dev("fast2 CASCL f32 on f64 rows", ctx("CASCL", 1024, 512, dtype="f32", **c1024), "k_scl_fast2<float", 2, (1, 3, 7),
                    "list"))
    out.append(_dev("fast4 CASCL", ctx("CASCL", 1024, 512, "KERNEL_FOUR_PER_WAVE", **c1024), "k_scl_fast4<", 4, (1, 2, 3, 5, 7), "list"))
    # one frame per wavefront, four wavefronts per workgroup
    out.append(_dev("fast N=128", ctx("CASCL", 128, 64, L=8, crc_taps=CRC6), "k_scl_fast<", 4, (1, 3, 5), "list"))
    out.append(_dev("fast N=1024", ctx("CASCL", 1024, 512, "KERNEL_ONE_PER_WAVE", **c1024), "k_scl_fast<", 4, (1, 3, 5), "list"))
    # one frame per wavefront or workgroup: the group is taken as 2, an odd batch beside a single frame
    out.append(_dev("big N=512 L=2", ctx("SCL", 512, 256, L=2), "k_scl_big<", 2, (1, 3), "list"))
    out.append(_dev("big N=2048 L=4", ctx("SCL", 2048, 1024, L=4), "k_scl_big<", 2, (1, 3), "list"))
    out.append(_dev("generic N=64 L=8", ctx("SCL", 64, 32, L=8), "k_scl_generic<", 2, (1, 3), "list"))
    out.append(_dev("generic spill N=64 L=8", ctx("SCL", 64, 32, "KERNEL_GENERIC_SPILL", L=8), "k_scl_generic<", 2, (1, 3), "list"))
    out.append(_dev("dyn PAC N=32 L=2", ctx("PAC", 32, 16, L=2), "k_scl_dyn<", 2, (1, 3), "dyn"))
    out.append(_dev("wide N=64 L=64", ctx("SCL", 64, 32, L=64), "k_scl_wide<", 2, (1, 3), "dyn"))
    q8pm = (BITS, O("d_pm", I4, 1, nullable=True), FLAGS)
    out.append(_dev("q8 CASCL N=64 L=8", ctx("CASCL", 64, 26, L=8, crc_taps=CRC6, dtype="q8"), "k_scl_q8<", 2, (1, 3), "q8",
                    q8pm, "polar_q8_decode_device"))
    out.append(_dev("q8 SC N=64", ctx("SC", 64, 32, dtype="q8"), "k_scl_q8<", 2, (1, 3), "q8", q8pm, "polar_q8_decode_device"))
    out.append(_dev("q8 quantise N=64", ctx("SC", 64, 32, dtype="q8"), "k_scl_q8<", 64, (1, 3, 65), "quantise",
                    (O("d_out", I1, "N"),), "polar_q8_quantize_device"))
    # 64 frames per wavefront
    out.append(_dev("sc_lanes N=128", ctx("SC", 128, 64), "k_sc_lanes<", 64, (64, 65, 127, 129), "sc"))
    out.append(_dev("sc_lanes N=128 misaligned rows", ctx("SC", 128, 64), "k_sc_lanes<", 64, (64, 65, 127, 129), "sc", shift=1))
    out.append(_dev("scf T=8 N=128", ctx("SCF", 128, 64, T=8, crc_taps=CRC6), "k_scf_lanes<", 64, (1, 63, 65, 129), "scf", SCF3,
                    "polar_scf_decode_device"))
    out.append(_dev("dscf (4,4,4) N=128", ctx("DSCF", 128, 64, budgets=(4, 4, 4), c=1.5, tau=5.0, crc_taps=CRC6), "k_scf_lanes<",
                    64, (1, 63, 65, 129), "dscf", SCF3 + (O("d_sets", I4, 3, nullable=True),), "polar_scf_decode_sets_device"))
    out.append(_dev("scan N=128 I=2", ctx("SCAN", 128, 64, iters=2), "k_scan_lanes<", 64, (1, 63, 65), "scan",
                    (O("d_uhat_bits", U4, "NW", nullable=True), O("d_llr_u", F8, "N", nullable=True),
                     O("d_ext_x", F8, "N", nullable=True)), "polar_scan_decode_device"))
    # BP: four frames per workgroup at most
    for kname, N, it in (("k_bp_w128<", 128, 8), ("k_bp_r4<", 1024, 8), ("k_bp<", 256, 8), ("k_bp<", 2048, 3)):
        for rule in (None, "g"):
            what = "k_bp_global" if N == 2048 else kname[:-1]
            out.append(_dev(f"{what} N={N} stop {rule or 'none'}", ctx("BP", N, N // 2, iterMax=it, early_stop=rule), kname, 4,
                            (1, 3, 5), "bp", BP3, "polar_bp_decode_device"))
    out.append(_dev("bp readout N=128", ctx("BP", 128, 64, iterMax=8), "k_bp_w128<", 4, (1, 3, 5), "readout",
                    (O("d_E", U8, "E_tab", "call", acc=True), O("d_uhat_bits", U4, "NW", nullable=True)), "polar_bp_readout_device",
                    checkpoints=(3, 8)))
    bpl5 = (BITS, O("d_iters", U4, 1, nullable=True), FLAGS, O("d_graph", U4, 1, nullable=True),
            O("d_total_iters", U4, 1, nullable=True))
    out.append(_dev("bpl N=128", ctx("BPL", 128, 64, iterMax=12, crc_taps=CRC6),
                    "k_bp_w128<double> (stop rule G) x 7 graphs (CRC-aided)", 64, (1, 65, 257), "bpl", bpl5,
                    "polar_bpl_decode_device"))
    out.append(_dev("bpl N=32 capped, AD_CHUNK + 1 frames", ctx("BPL", 32, 16, iterMax=10),
                    "k_bp<double> (stop rule G) x 5 graphs", AD_CHUNK, (AD_CHUNK + 1,), "bpl", bpl5, "polar_bpl_decode_device", cap=1,
                    rows="compaction edge"))
    # k_ad_crc_check holds 64 / (N / 32) = 16 frames per wavefront at N = 128
    out.append(_dev("adaptive (1,2,8) N=128", ctx("CASCL", 128, 64, L=8, crc_taps=CRC6, stages=(1, 2, 8)), "adaptive CA-SCL", 16,
                    (1, 15, 17, 63, 65, 257), "adaptive", LIST3 + (O("d_list", U4, 1, nullable=True),), "polar_cascl_decode_device"))
    rm = ctx("SCL", 64, 20, L=8, E=50)
    out.append(_dev("rate-matched decode A=20 E=50", rm, "k_rm_recover", 64, (1, 3, 65), "rm"))
    out.append(_dev("rate-matched recover A=20 E=50", rm, "k_rm_recover", 64, (1, 3, 65), "recover", (O("d_out", F8, "N"),),
                    "polar_rm_recover_device"))
    cnt = (O("d_counters", U8, 2, "call", acc=True), O("d_frame_err", U4, 1, nullable=True))
    cc = dict(L=8, crc_taps=CRC6)
    out.append(_dev("count errors", ctx("CASCL", 128, 64, **cc), "", 64, (1, 3, 65), "count", cnt, "polar_count_errors_device"))
    out.append(_dev("count errors systematic", ctx("CASCL", 128, 64, sys_polar=True, **cc), "", 64, (1, 3, 65), "count", cnt,
                    "polar_count_errors_device"))
    out.append(_dev("stop rule cut", ctx("CASCL", 128, 64, **cc), "", 64, (1, 3, 65), "cut", (O("d_out", U8, 3, "call"),),
                    "polar_stop_rule_cut_device"))
    out.append(_dev("genie count N=128", ctx("SC", 128, 64), "", 64, (1, 3, 65), "genie", (O("d_counts", U8, "2N", "call", acc=True),),
                    "polar_genie_count_device"))
    # the encoder side: a frame group of 1 << enc_log_group(NW) lanes, 64 frames per wavefront at N = 32, one at N = 4096
    for label, c, G, bs in (("N=32", ctx("SC", 32, 13), 64, (1, 63, 65, 257)), ("N=4096", ctx("SCL", 4096, 2048, L=2), 2, (1, 3)),
                            ("rate-matched", ctx("CASCL", 128, 64, L=8, crc_taps=CRC6, E=100), 16, (1, 3, 65))):
        out.append(_dev(f"transform {label}", c, "", G, bs, "transform", (O("d_out", U4, "NW"),), "polar_transform_device"))
        out.append(_dev(f"encode {label}", c, "", G, bs, "encode", ENC2, "polar_encode_device", not_all_null=True))
        out.append(_dev(f"payload {label}", c, "", G, bs, "payload", PAY2, "polar_payload_device"))
    out.append(_dev("time decode CASCL N=1024", ctx("CASCL", 1024, 512, **c1024), "k_scl_fast2<", 2, (1, 3, 7), "list", (BITS,),
                    "polar_time_decode_device"))
    return out


CASES = _cases()

# entry points with outputs that an existing test already holds to their extents
ELSEWHERE = {
    "polar_generate_device": "tests/test_gpu_generator_values.py::test_generator_bits_and_values",
    "polar_genie_rows_device": "tests/test_gpu_generator_values.py::test_genie_rows_values",
}

# ---- the host-buffer forms (part 4): entry point -> the device form its result must equal ----------------------------------------
HOST_BATCHES = (1, 3, 65)
HOST_CASES = {
    "polar_decode": "polar_decode_device",
    "polar_decode_llr": "polar_decode_device",
    "polar_decode_batch": "polar_decode_device",
    "polar_decode_batch_y": "polar_decode_device",
    "polar_bp_decode_batch": "polar_bp_decode_device",
    "polar_cascl_decode_batch": "polar_cascl_decode_device",
    "polar_scf_decode_batch": "polar_scf_decode_device",
    "polar_scf_decode_sets_batch": "polar_scf_decode_sets_device",
    "polar_scan_decode_batch": "polar_scan_decode_device",
    "polar_bpl_decode_batch": "polar_bpl_decode_device",
    "polar_q8_decode_batch": "polar_q8_decode_device",
    "polar_encode_batch": "polar_encode_device",
    "polar_payload_batch": "polar_payload_device",
    "polar_bp_readout_batch": "polar_bp_readout_device",
}
# host-buffer forms that return a few numbers through scalar pointers, and the chunked loop with a device buffer
HOST_ELSEWHERE = {
    "polar_fer_batch": "two host counters; no caller buffer",
    "polar_stop_rule_batch_y": "three host scalars; no caller buffer",
    "polar_group_fer_batch": "needs more than one GPU",
    "polar_group_stop_rule_batch": "needs more than one GPU",
    "polar_construct_batch": "tests/test_gpu_extents.py::test_chunked_loops[construct]",
}


# ---- the header ---------------------------------------------------------------------------------------------------------------
Proto = namedtuple("Proto", "name params comment")
_PROTO = re.compile(r"^(?:int|void|const char \*|void \*)\s*(polar_\w+)\(([^;{]*?)\);", re.M | re.S)
_COMMENT = re.compile(r"/\*.*?\*/", re.S)


def prototypes(text=None):
    """{name: Proto} of include/polar_hip.h: params as (declaration, name) pairs, comment = the comment block that ends right
    above the prototype (through the prototypes of one group that share it)"""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    comments = [(m.start(), m.end(), m.group(0)) for m in _COMMENT.finditer(text)]
    out = {}
    for m in _PROTO.finditer(text):
        if any(a <= m.start() < b for a, b, _ in comments):
            continue
        params = []
        for p in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(","):
            p = " ".join(p.split())
            params.append((p, re.split(r"[\s*]+", p)[-1]))
        above = [c for c in comments if c[1] <= m.start()]
        out[m.group(1)] = Proto(m.group(1), params, above[-1][2] if above else "")
    return out


def device_outputs(proto):
    """the names of the non-const device pointer parameters after B"""
    names = [n for _, n in proto.params]
    after = proto.params[names.index("B") + 1:] if "B" in names else []
    return [n for d, n in after if "*" in d and not d.startswith("const") and n.startswith("d_")]


def nullable_in_comment(proto):
    """the outputs a prototype's comment declares nullable: `name (nullable`, `name (may be NULL`, `a, b and c are nullable`,
    and every output for `each of the three may be NULL` / `either output nullable`"""
    outs = device_outputs(proto)
    text = " ".join(proto.comment.replace("*", " ").split())
    found = set(re.findall(r"(\w+)\s*(?:\[[^\]]*\])*\s*\((?:nullable|may be NULL)", text))
    for m in re.finditer(r"((?:\w+(?:,\s*|\s+and\s+))+\w+)\s+are nullable", text):
        found |= set(re.split(r",\s*|\s+and\s+", m.group(1)))
    if re.search(r"each of the \w+ may be NULL|[Ee]ither output nullable", text):
        found |= set(outs)
    return [n for n in outs if n in found]
