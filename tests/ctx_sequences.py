"""The scripts of the reused-context tests: what one polar_ctx is put through, call after call, and for every call the recipe
of the fresh context that must give the same outputs.  Pure Python and numpy: tests/test_ctx_sequences_host.py checks the
table itself on the CPU, tests/test_gpu_ctx_sequences.py runs it.

The statement held: the outputs of call k on a context depend on its current configuration and on the call's own inputs,
and on nothing that calls 1 .. k-1 left behind (staging buffers that only grow, tables built on first use, the per-call
frozen mask and its phase end, tables and sub-contexts swapped by the setters, the lane exchange of polar_fer_batch).

A script is a context kind (constructor of polardecoding_amd and its arguments), a seed with an Eb/N0, and an ordered list of
steps.  A step is a change, Chg(what, value), or an observation, Obs(entry, B, opt):

  change       `what` is a key of SETTERS (a setter of include/polar_hip.h), of HOOKS (a hook of include/polar_hip_testing.h:
               the step exists only where the context lives in the testing library) or "frozen_mask" (the mask of the next
               polar_decode_batch, by name in the script's `masks`; that call consumes it).
  observation  `entry` is a key of the GPU file's ENTRIES: one entry point (or a short chain of them) with its batch and all
               of its outputs.

walk(script) yields every step with the settings in force: for an observation that is the recipe of the fresh context --
the constructor plus the final value of each setting that differs from its default, each set once, in the order of
SETTING_ORDER, with no history.  A setting's value is what the context holds afterwards, not what was passed: dynamic
SC-Flip leaves its first budget behind as the flip budget T when it is switched off (polar_scf_set_dynamic), so the recipe of
the observations after that names T.

Inputs.  rows(script) draws one random codeword per frame (all-zero codewords for the rate-matched and the PAC script, whose
encoders are not restated here: their Eb/N0 is low enough that most frames hold decision errors), BPSK + AWGN.  Observation
i of a script reads the frames (37 i + b) mod BMAX, b < B: two consecutive calls never see the same rows at the same index, so
a row or a result left in a staging buffer by the earlier call is not the right answer of the later one.

model(script, settings, obs, x, oracle) is the CPU model of an observation where the feature test of that decoder has one
(the oracle, scan_model, scf_model / dscf_model, bpl_model, q8_model, the BP stop rule of test_bp_early_stop_host, the oracle
composition of the stage rule, dscl_model for PAC and wide lists, the recovery of test_rm_host).  The host test uses it for the
sensitivity of every change (old and new settings must differ on the observation's own frames), the GPU test for the anchor
of every script.  Keys that begin with "_" are verdicts of the model that no entry point returns."""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

CRC6 = (0, 5, 6)
CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)
AD_CHUNK = 2048          # frames per compaction block (csrc/adaptive_kernel.h)
FER_SPLIT = 32768        # polar_fer_batch runs two lanes from here (csrc/h_fer.hip)
FLAG_TIE, FLAG_CRC_PASS, FLAG_RERANK, FLAG_BP_CONVERGED = 1, 2, 4, 8
KERNEL_AUTO, KERNEL_GENERIC_SPILL, KERNEL_BIG, KERNEL_ONE_PER_WAVE = 0, 2, 3, 4   # polardecoding_amd/testing.py
B_MAX = 300              # no batch above it unless the threshold it crosses is the point (BIG_B names those)
BIG_B = {FER_SPLIT + 65: "two lanes of polar_fer_batch, ragged second half", 40000: "two lanes of polar_fer_batch (rm_rows is per lane)",
         AD_CHUNK + 1: "one frame beyond a compaction block"}

Chg = namedtuple("Chg", "what value")
Obs = namedtuple("Obs", "entry B opt")


def obs(entry, B, **opt):
    return Obs(entry, B, opt)


# setting -> the setter of include/polar_hip.h that a change of it calls
SETTERS = {"stream": "polar_set_stream", "bp_stop": "polar_bp_set_stop", "stages": "polar_cascl_set_stages",
           "scf_flips": "polar_scf_set_flips", "scf_dynamic": "polar_scf_set_dynamic", "scan_iters": "polar_scan_set_iters",
           "bpl_graphs": "polar_bpl_set_graphs", "sys_polar": "polar_set_systematic", "quant": "polar_q8_set_quant"}
# setters of the header that are not setters of a polar_ctx, with the test that runs them
ELSEWHERE = {"polar_codebook_set_stream": "tests/test_gpu_ctx_sequences.py::test_reused_codebook_equals_a_fresh_one"}
HOOKS = ("select_kernel", "big_split", "resident_blocks", "chunk_bytes")
# the order in which a fresh context receives its settings; the values a context is created with
SETTING_ORDER = HOOKS + ("stream", "sys_polar", "stages", "bp_stop", "scf_flips", "scf_dynamic", "scan_iters", "bpl_graphs", "quant")
DEFAULTS = {"select_kernel": KERNEL_AUTO, "big_split": 0, "resident_blocks": 0, "chunk_bytes": 0, "stream": None,
            "sys_polar": False, "stages": (), "bp_stop": "none", "scf_flips": 8, "scf_dynamic": None, "scan_iters": 4,
            "bpl_graphs": None, "quant": (2.0, 8, 8), "frozen_mask": None}
# changes without a CPU model: identical outputs are the expected result, the GPU test asserts that they were in effect
NO_MODEL = HOOKS + ("stream",)
# entries that take the per-call mask
TAKES_MASK = ("decode_batch",)


class Script:
    def __init__(self, name, ctor, args, kw, seed, db, steps, crosses, masks=None, zero=False, quiet=()):
        self.name, self.ctor, self.args, self.kw, self.seed, self.db = name, ctor, tuple(args), dict(kw), seed, db
        self.steps, self.crosses, self.mask_fns, self.zero = list(steps), crosses, dict(masks or {}), zero
        self._masks = None   # built on first use (they read the 5G table)
        self.quiet = tuple(quiet)   # hooks whose effect neither kernel_name nor the launch plan shows on this context
        self.N, self.K = self.args[0], self.args[1]
        self.taps = tuple(self.kw["crc_taps"]) if self.kw.get("crc_taps") else None
        self.A = self.K + (max(self.taps) if self.taps else 0)
        self.W = self.kw.get("E", self.N)           # values per input row
        self.L = self.kw.get("L", 1)

    def uses_hooks(self):
        return any(isinstance(s, Chg) and s.what in HOOKS for s in self.steps)

    def without_hooks(self):
        """the same script for a context in the shipped library: every step but the hook changes"""
        return Script(self.name, self.ctor, self.args, self.kw, self.seed, self.db,
                      [s for s in self.steps if not (isinstance(s, Chg) and s.what in HOOKS)], self.crosses, self.mask_fns, self.zero,
                      self.quiet)

    @property
    def masks(self):
        if self._masks is None:
            self._masks = {k: f() for k, f in self.mask_fns.items()}
        return self._masks

    def info_order(self):
        """I[0..A) of the context in ascending reliability: the 5G order (every script has N <= 1024)"""
        import polardecoding_amd as pa
        return np.asarray(pa.q_sequence(self.N)[self.N - self.A:], dtype=np.int32)

    def frozen(self, mask=None):
        if mask is not None:
            return np.asarray(self.masks[mask], dtype=np.uint8)
        fz = np.ones(self.N, dtype=np.uint8)
        fz[self.info_order()] = 0
        return fz

    def bmax(self):
        return max(s.B for s in self.steps if isinstance(s, Obs) and s.entry not in GENERATED)


# what every entry returns, by the names the GPU file and model() share ("soft": only where the observation asks for them)
OUTPUTS = {"decode_batch": ("uh", "pm", "flags"), "decode": ("uh",), "decode_batch_y": ("uh", "pm", "flags"),
           "decode_device": ("uh", "pm", "flags"), "construct_batch": ("counts",), "stop_rule_batch_y": ("used", "blk", "bits"),
           "generate_count": ("llr", "u_bits", "uh", "counters", "frame_err"), "fer_batch": ("blk", "bits"),
           "decode_cascl_device": ("uh", "pm", "flags", "list_size"), "encode_payload": ("u", "x", "payload", "crc_ok"),
           "list_decode": ("paths", "pm", "rem", "count", "flags", "idx", "gathered"),
           "decode_bp_device": ("uh", "iters", "flags"), "decode_bp_batch": ("uh", "iters", "flags"),
           "bp_readout": ("refused", "E", "uh"),
           "decode_scf_device": ("uh", "flags", "attempts"), "decode_scf_batch": ("uh", "flags", "attempts"),
           "decode_scf_sets_device": ("uh", "flags", "attempts", "sets"), "decode_scf_sets_batch": ("uh", "flags", "attempts", "sets"),
           "decode_scan_device": ("uh", "llr_u", "ext_x"), "decode_scan_batch": ("uh", "llr_u", "ext_x"),
           "decode_bpl_device": ("uh", "iters", "flags", "graph", "total_iters"),
           "decode_bpl_batch": ("uh", "iters", "flags", "graph", "total_iters"),
           "decode_q8_device": ("uh", "pm", "flags"), "rm_recover": ("rows",), "encode_batch": ("u", "x")}


def outputs_of(ob):
    names = OUTPUTS[ob.entry]
    if ob.entry == "decode_scan_device" and not ob.opt.get("soft"):
        names = ("uh",)
    return names


# entries whose frames come from the device generator (seed, first frame, Eb/N0), not from rows()
GENERATED = ("fer_batch", "generate_count", "construct_batch")


def apply(settings, chg):
    """the settings after a change: what the context holds, which is not always what was passed"""
    s = dict(settings)
    if chg.what == "scf_dynamic":
        s["scf_dynamic"] = chg.value
        if chg.value is not None:
            s["scf_flips"] = chg.value[0][0]       # budgets[0] becomes T and stays when the rule is switched off
    elif chg.what == "scf_flips":
        s["scf_flips"] = chg.value
        if s["scf_dynamic"] is not None:
            (b, c, tau) = s["scf_dynamic"]
            s["scf_dynamic"] = ((chg.value,) + tuple(b[1:]), c, tau)
    elif chg.what == "stages":
        s["stages"] = tuple(chg.value) if len(chg.value) > 1 else ()
    else:
        assert chg.what in DEFAULTS, chg.what
        s[chg.what] = chg.value
    return s


def recipe(settings):
    """the changes that make a fresh context of these settings, one per setting that is not at its default"""
    return [Chg(k, settings[k]) for k in SETTING_ORDER if settings[k] != DEFAULTS[k]]


Step = namedtuple("Step", "i step before settings nobs")   # settings: in force at the step (after it, for a change)


def walk(script):
    """every step with the settings before and at it; an observation that takes the per-call mask consumes it"""
    settings = dict(DEFAULTS)
    nobs = 0
    for i, st in enumerate(script.steps):
        before = settings
        if isinstance(st, Chg):
            settings = apply(settings, st)
            yield Step(i, st, before, settings, nobs)
        else:
            yield Step(i, st, before, settings, nobs)
            nobs += 1
            if st.entry in TAKES_MASK and settings["frozen_mask"] is not None:
                settings = dict(settings, frozen_mask=None)


def frame_index(script, nobs, B):
    return (37 * nobs + np.arange(B)) % script.bmax()


Inputs = namedtuple("Inputs", "llr y sigma u")
_rows = {}


def rows(script, sys_polar=False):
    """Inputs of bmax() frames: llr = 2 y / sigma^2 [.][W], y [.][W], sigma, the sent u [.][N].  sys_polar: the same payloads
    sent as systematic polar codewords (what a context in that mode is meant to decode: the CRC of a plain codeword fails
    there on every frame, and every stage rule would end at its last stage)."""
    key = (script.name, bool(sys_polar))
    if key in _rows:
        return _rows[key]
    from test_encode_host import place, sys_encode, transform
    rng = np.random.default_rng(script.seed)
    n, N = script.bmax(), script.N
    sigma = float(np.sqrt(1.0 / (2.0 * (script.K / script.W) * 10.0 ** (script.db / 10.0))))
    if script.zero:
        u = np.zeros((n, N), dtype=np.uint8)
        x = np.zeros((n, script.W), dtype=np.uint8)
    else:
        v = rng.integers(0, 2, (n, script.K), dtype=np.uint8)
        u = place(v, N, script.info_order(), script.taps, bool(script.kw.get("systematic")))
        if sys_polar:
            u = sys_encode(u, script.info_order())[0]
        x = transform(u)
    y = (1.0 - 2.0 * x) + sigma * rng.standard_normal(x.shape)
    _rows[key] = Inputs(2 * y / sigma / sigma, y, sigma, u.astype(np.int32))
    return _rows[key]


def inputs(script, nobs, B, sys_polar=False):
    r, idx = rows(script, sys_polar), frame_index(script, nobs, B)
    return Inputs(np.ascontiguousarray(r.llr[idx]), np.ascontiguousarray(r.y[idx]), r.sigma, np.ascontiguousarray(r.u[idx]))


def cyclic_graphs(n, P):
    return [[(b + s) % n for b in range(n)] for s in range(P)]


# ---- the scripts -------------------------------------------------------------------------------------------------------------
def _mask(N, A):
    """the A most reliable leaves of the 5G order unfrozen"""
    import polardecoding_amd as pa
    m = np.ones(N, dtype=np.uint8)
    m[pa.q_sequence(N)[N - A:]] = 0
    return m


def _mask1024(low):
    """the 512 most reliable leaves with those below 256 replaced by `low` (tests/fill_phase_codes.py with_low)"""
    import fill_phase_codes as F
    m = np.ones(1024, dtype=np.uint8)
    m[F.with_low(low, 512)] = 0
    return m


DEV, HOST = "decode_device", "decode_batch"
DYN2, DYN3 = ((4, 16), 1.5, 5.0), ((4, 16, 4), 1.5, 5.0)


def _scripts():
    S = []

    S.append(Script("sc128", "SCdecode", (128, 64), {}, 11, 2.0, [
        obs(HOST, 5), obs(DEV, 130),
        Chg("frozen_mask", "A"), obs(HOST, 5),
        obs("construct_batch", 130),
        Chg("frozen_mask", "B"), obs(HOST, 130),
        obs(HOST, 5), obs("decode", 1), obs(DEV, 130)],
        "c->in / bits / pm / flags between k_scl_generic (B < 64) and k_sc_lanes; d_frozen_override of two masks and of none; "
        "genie_rows of polar_construct_batch between them", masks={"A": lambda: _mask(128, 72), "B": lambda: _mask(128, 56)}))

    S.append(Script("scl128", "SCLdecode", (128, 64), {"L": 8}, 12, 2.0, [
        obs(DEV, 5),
        Chg("resident_blocks", 2), obs(DEV, 300),
        Chg("resident_blocks", 0), obs(DEV, 5),
        obs(HOST, 70), obs("stop_rule_batch_y", 70), obs(HOST, 7),
        obs("generate_count", 40), obs("fer_batch", FER_SPLIT + 65), obs(DEV, 300),
        Chg("stream", "A"), obs(DEV, 5),
        Chg("stream", "B"), obs(DEV, 300),
        Chg("stream", "A"), obs(HOST, 7)],
        "the queue counter of c->scratch (allocated under the cap, unused after it); c->flags as error counts "
        "(polar_stop_rule_batch_y) and then as flags; gen_u / gen_cnt / c->bits of polar_fer_batch, lane_b with its stream and "
        "event, swap_lane(); two caller streams in turn"))

    S.append(Script("scl1024", "SCLdecode", (1024, 512), {"L": 8}, 13, 2.0, [
        obs(DEV, 3),
        Chg("frozen_mask", "A"), obs(HOST, 40),
        Chg("frozen_mask", "B"), obs(HOST, 3),
        obs(HOST, 40), obs(DEV, 3),
        Chg("select_kernel", KERNEL_BIG), obs(DEV, 40),
        Chg("select_kernel", KERNEL_GENERIC_SPILL), obs(DEV, 3),
        Chg("select_kernel", KERNEL_ONE_PER_WAVE), obs(DEV, 40),
        Chg("select_kernel", KERNEL_AUTO), obs(DEV, 3)],
        "fill_end_override of the pair kernel: 256 (mask A), 128 (mask B), then the context's own 192 through the same "
        "pointer comparison of decode_fixed(); c->scratch sized by k_scl_big, k_scl_generic (global scratch), k_scl_fast and "
        "k_scl_fast2 in turn",
        # B has an information leaf in the middle of block 128 .. 191: a phase end left over from A would decode it as frozen
        masks={"A": lambda: _mask1024([127, 254, 255]), "B": lambda: _mask1024([180, 254, 255])}))

    ad = "decode_cascl_device"
    S.append(Script("cascl1024", "CASCL", (1024, 512), {"L": 8, "crc_taps": CRC24C}, 14, 1.5, [
        obs(ad, 5), obs("encode_payload", 9),
        Chg("stages", (1, 8)), obs(ad, 300),
        Chg("stages", (2, 8)), obs(ad, 5),
        Chg("stages", (1, 2, 4, 8)), obs(ad, 300),
        Chg("stages", ()), obs(ad, 5),
        Chg("sys_polar", True), obs(ad, 40),
        Chg("stages", (1, 8)), obs(ad, 300),
        Chg("stages", (2, 8)), obs(ad, 5),
        Chg("sys_polar", False), obs(ad, 40),
        Chg("sys_polar", True), obs(ad, 5),
        Chg("sys_polar", False), obs(ad, 40),
        Chg("stages", ()), obs(ad, 300),
        obs("encode_payload", 9)],
        "stage contexts created and destroyed under the live context (they borrow its stream); the ad_* buffers; d_crc_tab / "
        "d_crc_mask of the context and of its stages through polar_set_systematic in both orders with polar_cascl_set_stages; "
        "h_crc_tab_sys, enc_tables and info_order_table built lazily in either mode"))

    lst = "list_decode"
    S.append(Script("cascl128", "CASCL", (128, 64), {"L": 8, "crc_taps": CRC6, "systematic": True}, 15, 2.0, [
        obs(DEV, 5), obs(lst, 130), obs(DEV, 5),
        Chg("sys_polar", True), obs(lst, 130),
        Chg("sys_polar", False), obs(DEV, 5), obs(lst, 130)],
        "the D = 0 list tables (d_list_mask / d_list_row) built on first use, c->scratch between k_scl_fast and k_scl_list; the "
        "CRC tables of both modes under the list kernel"))

    for N in (128, 256):
        S.append(Script(f"bp{N}", "BP", (N, N // 2), {"iterMax": 12}, 16 + N, 2.0, [
            obs("decode_bp_device", 5),
            Chg("bp_stop", "g"), obs("decode_bp_device", 130), obs("bp_readout", 5),
            Chg("bp_stop", "none"), obs("decode_bp_device", 5), obs("bp_readout", 5),
            Chg("bp_stop", "g"), obs("decode_bp_batch", 130),
            Chg("frozen_mask", "A"), obs(HOST, 5)],
            "iters / flags written by the kernel (rule G) or by memset (rule NONE); bp_iters and c->flags of the host forms; the "
            "priors of a mask override (d_frozen_override) after the context's own", masks={"A": lambda N=N: _mask(N, N // 2 + 8)}))

    S.append(Script("scf128", "SCFlip", (128, 64), {"crc_taps": CRC6}, 17, 1.0, [
        obs("decode_scf_device", 5),
        Chg("scf_flips", 1), obs("decode_scf_device", 130),
        Chg("scf_flips", 32), obs("decode_scf_batch", 5),
        Chg("scf_flips", 8), obs("decode_scf_sets_device", 130),
        Chg("scf_dynamic", DYN2), obs("decode_scf_sets_device", 5),
        Chg("scf_dynamic", DYN3), obs("decode_scf_sets_batch", 130),
        Chg("scf_dynamic", None), obs("decode_scf_device", 5), obs("decode_scf_batch", 130)],
        "scf_flips / scf_pass / scf_bits sized by T = 1, 32, 8; scf_sets / scf_l* / scf_spass / scf_surv of the dynamic rule "
        "at order 2 and 3 and their leftovers under the static rule (T = 4, the first dynamic budget, stays); scf_hsets"))

    S.append(Script("scan128", "SCAN", (128, 64), {}, 18, 1.0, [
        obs("decode_scan_device", 5, soft=True),
        Chg("scan_iters", 1), obs("decode_scan_device", 130, soft=False),
        Chg("scan_iters", 8), obs("decode_scan_device", 5, soft=True),
        Chg("scan_iters", 4), obs("decode_scan_batch", 130),
        obs(HOST, 5),
        Chg("frozen_mask", "A"), obs(HOST, 130)],
        "the stored betas in c->scratch between iteration counts; scan_llr / scan_ext staging and null soft outputs in turn; "
        "c->in / c->bits between polar_scan_decode_batch and polar_decode_batch; d_frozen_override",
        masks={"A": lambda: _mask(128, 72)}))

    S.append(Script("bpl128", "BPL", (128, 64), {"iterMax": 12, "crc_taps": CRC6}, 19, 2.0, [
        obs("decode_bpl_device", 9),
        Chg("bpl_graphs", 2), obs("decode_bpl_device", AD_CHUNK + 1),
        Chg("bpl_graphs", 7), obs("decode_bpl_device", 9),
        Chg("bpl_graphs", 1), obs("decode_bpl_batch", AD_CHUNK + 1),
        Chg("bpl_graphs", None), obs("decode_bpl_device", AD_CHUNK + 1)],
        "d_bpl_sigma / d_bpl_sinv / d_bpl_frozen / d_bpl_crc reallocated for 2, 7, 1 and the default number of graphs; the open-frame "
        "lists (ad_idx, ad_blk of two compaction blocks after one), bpl_siters, bpl_graph / bpl_total"))

    S.append(Script("q8_128", "CASCL", (128, 64), {"L": 8, "dtype": "Q8", "crc_taps": CRC24C}, 20, 2.5, [
        obs(DEV, 5), obs(DEV, 300),
        Chg("quant", (1.0, 5, 6)), obs(DEV, 5), obs("decode_q8_device", 300),
        Chg("quant", (2.0, 8, 8)), obs(DEV, 5), obs("decode_q8_device", 300)],
        "q8_rows (per lane) and q8_pm between the float entry and polar_q8_decode_device on rows quantised under the first "
        "quantiser; scale, qc and qi read at every launch"))

    S.append(Script("rm128", "SCLdecode", (128, 40), {"L": 8, "E": 99, "ibil": True}, 21, 0.0, [
        obs("rm_recover", 5), obs(DEV, 5), obs(DEV, 300), obs(DEV, 5),
        obs("decode_batch_y", 70), obs("fer_batch", 40000), obs("encode_batch", 9), obs(DEV, 300)],
        "rm_rows of both lanes (polar_fer_batch swaps them), gen_llr at E values per row, enc_x / enc_io of the host encoder", zero=True))

    S.append(Script("dyn128", "PAC", (128, 64), {}, 22, 1.0, [
        obs(DEV, 5), obs(lst, 130), obs("generate_count", 40), obs("fer_batch", FER_SPLIT + 65), obs(DEV, 5), obs(DEV, 130)],
        "c->scratch between k_scl_dyn and k_scl_list with the dynamic tables; the generator's dynamic fill; both lanes", zero=True))

    S.append(Script("wide128", "SCLdecode", (128, 64), {"L": 64}, 23, 2.0, [
        obs(DEV, 5), obs(lst, 70),
        Chg("select_kernel", KERNEL_GENERIC_SPILL), obs(DEV, 5),
        Chg("select_kernel", KERNEL_AUTO), obs(DEV, 70)],
        "c->scratch of k_scl_wide with its levels in LDS and in global scratch, and of its list epilogue",
        quiet=("select_kernel",)))   # k_scl_wide keeps its name and its plan in either variant
    return S


SCRIPTS = _scripts()
BY_NAME = {s.name: s for s in SCRIPTS}


# ---- the CPU models ----------------------------------------------------------------------------------------------------------
def _mask_code(oracle, N, frozen):
    fz = np.asarray(frozen) != 0
    q = [int(j) for j in np.flatnonzero(fz)] + [int(j) for j in np.flatnonzero(~fz)]
    return oracle.Code(N, int((~fz).sum()), None, Q=q)


def _verdict(tab, uh):
    from test_encode_host import syndrome
    return syndrome(tab, uh) == 0


def model(script, settings, ob, x, oracle, cap=None):
    """_model() cut down to the outputs the entry returns (and the model's own verdicts)"""
    m = _model(script, settings, ob, x, oracle, cap)
    if m is None:
        return None
    return {k: v for k, v in m.items() if k.startswith("_") or k in outputs_of(ob)}


def _model(script, settings, ob, x, oracle, cap=None):
    """CPU model of observation `ob` under `settings` on the frames x (the first `cap` of them): a dict of outputs by the names
    the GPU file uses, or None where the decoder's feature test has no model for the entry."""
    s, N = script, script.N
    n = len(x.llr) if cap is None else min(cap, len(x.llr))
    llr = x.llr[:n]
    mask = settings["frozen_mask"] if ob.entry in TAKES_MASK else None
    fz = s.frozen(mask)
    e = ob.entry
    if s.ctor == "BP":
        if e not in ("decode_bp_device", "decode_bp_batch", HOST):
            return None
        if settings["bp_stop"] == "g":
            from test_bp_early_stop_host import stop_points
            t, conv, out = stop_points(llr, fz, s.kw["iterMax"])
            return {"uh": out, "iters": t, "flags": np.where(conv, FLAG_BP_CONVERGED, 0)}
        uh, _, _ = oracle.decode(_mask_code(oracle, N, fz), llr, "BP", bp_iters=s.kw["iterMax"])
        return {"uh": uh, "iters": np.full(n, s.kw["iterMax"]), "flags": np.zeros(n, dtype=np.int64)}
    if s.ctor == "SCAN":
        if e not in ("decode_scan_device", "decode_scan_batch", HOST):
            return None
        from test_scan_host import scan_model
        uh, lu, ex = scan_model(fz, llr, settings["scan_iters"], oracle=oracle, skip=True)
        return {"uh": uh, "llr_u": lu, "ext_x": ex}
    if s.ctor == "SCFlip":
        code = oracle.Code(N, s.K, s.taps)
        if settings["scf_dynamic"] is not None:
            from dscf_model import dscf_model
            b, c, tau = settings["scf_dynamic"]
            r = dscf_model(code, llr, b, c, tau, oracle=oracle)
            return {"uh": r.u, "flags": r.flags, "attempts": r.attempts, "sets": r.sets}
        from test_scf_host import scf_model
        uh, fl, at = scf_model(code, llr, settings["scf_flips"], oracle=oracle)[:3]
        return {"uh": uh, "flags": fl, "attempts": at}
    if s.ctor == "BPL":
        import bpl_model as M
        nb = N.bit_length() - 1
        P = settings["bpl_graphs"] if settings["bpl_graphs"] is not None else min(nb, 8)
        r = M.bpl_decode(llr, fz, s.info_order(), M.cyclic_graphs(nb, P), s.kw["iterMax"], s.taps)
        return {"uh": r.bits, "iters": r.iters, "flags": r.flags, "graph": r.graph, "total_iters": r.total}
    if s.kw.get("dtype") == "Q8":
        import q8_model as Q
        scale, qc, qi = settings["quant"]
        if e == DEV:
            q = Q.quantize(llr, scale, qc)
        elif e == "decode_q8_device":
            q = Q.quantize(llr, *DEFAULTS["quant"][:2])     # rows quantised under the quantiser the context was created with
        else:
            return None
        uh, pm, fl = Q.decode_rows(q, fz, s.L, crc=(s.info_order(), s.taps), qc=qc, qi=qi)
        return {"uh": uh, "pm": pm, "flags": fl}
    if "E" in s.kw:
        if e != "rm_recover":
            return None
        from test_rm_host import recover
        return {"rows": recover(llr, N, s.A, s.kw["ibil"])}
    if s.ctor == "PAC" or s.L > 32:
        if e != DEV:
            return None
        from test_dyn_host import dscl_model
        dyn = None
        if s.ctor == "PAC":
            import polardecoding_amd as pa
            io = pa.pac_info_order(N, s.K)
            dyn = pa.dyn_pac(N, io)
            fz = np.ones(N, dtype=np.uint8)
            fz[io] = 0
        uh, pm, fl = dscl_model(fz, dyn, llr, 32 if s.ctor == "PAC" else s.L, oracle=oracle)
        return {"uh": uh, "pm": pm}
    # SC / SCL / CA-SCL with L <= 32 on the oracle
    algo = {"SCdecode": "SC", "SCLdecode": "SCL", "CASCL": "CASCL"}[s.ctor]
    if e == "decode_cascl_device":
        from test_encode_host import crc_table, crc_table_sys
        code = oracle.Code(N, s.K, s.taps)
        io = s.info_order()
        if settings["sys_polar"]:
            # the systematic mode: the verdict of its table on the words as sent; the list size that decides a frame where
            # the first of at most two stages has a model (SC on the oracle, L = 2 on list_model with that table)
            tab = crc_table_sys(N, io, s.taps)
            out = {"_verdict": _verdict(tab, x.u[:n])}
            st = settings["stages"]
            if not st:
                out["list_size"] = np.full(n, s.L)
            elif len(st) == 2 and st[0] == 1:
                sc = _mask_code(oracle, N, s.frozen())
                out["list_size"] = np.where(_verdict(tab, oracle.decode(sc, llr, "SC")[0]), 1, s.L)
            elif len(st) == 2 and st[0] == 2:
                import list_model as LM
                fl = LM.list_model(s.frozen(), None, llr, 2, crc=tab, oracle=oracle)[4]
                out["list_size"] = np.where((fl & FLAG_CRC_PASS) != 0, 2, s.L)
            return out
        if settings["stages"]:
            from test_gpu_cascl_adaptive import _oracle_composition
            uh, pm, fl, ls = _oracle_composition(oracle, code, s.taps, settings["stages"], llr)
        else:
            uh, pm, _ = oracle.decode(code, llr, "CASCL", L=s.L)
            ls = np.full(n, s.L)
        return {"uh": uh, "pm": pm, "list_size": ls, "_verdict": _verdict(crc_table(N, io, s.taps), x.u[:n])}
    if e == "list_decode" and s.ctor == "CASCL":
        import list_model as LM
        from test_encode_host import crc_table_sys
        crc = crc_table_sys(N, s.info_order(), s.taps) if settings["sys_polar"] else (s.info_order(), s.taps)
        paths, pm, rem, count, fl = LM.list_model(fz, None, llr, s.L, crc=crc, oracle=oracle)
        return {"paths": paths, "pm": pm, "rem": rem, "count": count, "flags": fl}
    if e not in (DEV, HOST, "decode_batch_y"):
        return None
    if settings["sys_polar"]:   # CA-SCL with the systematic mode's table: the list model's choice
        if s.ctor != "CASCL" or N > 128:
            return None
        import list_model as LM
        from test_encode_host import crc_table_sys
        paths, pm, rem, count, fl = LM.list_model(fz, None, llr, s.L, crc=crc_table_sys(N, s.info_order(), s.taps), oracle=oracle)
        k = LM.kstar(rem, count, True)
        return {"uh": paths[np.arange(n), k], "pm": pm[np.arange(n), k],
                "_verdict": _verdict(crc_table_sys(N, s.info_order(), s.taps), x.u[:n])}
    code = _mask_code(oracle, N, fz) if mask is not None else oracle.Code(N, s.K, s.taps)
    uh, pm, _ = oracle.decode(code, llr, algo, L=s.L)
    out = {"uh": uh} if algo == "SC" else {"uh": uh, "pm": pm}
    if algo == "CASCL" and mask is None:   # FLAG_CRC_PASS of a frame decoded as sent
        from test_encode_host import crc_table
        out["_verdict"] = _verdict(crc_table(N, s.info_order(), s.taps), x.u[:n])
    return out
