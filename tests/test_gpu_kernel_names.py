"""GPU: polar_kernel_name() of a context, string for string.

Some forty assertions elsewhere in the suite take `dec.kernel_name` as evidence that a given kernel ran.  The name is
formatted from the same choice decode_fixed() launches by (csrc/polar_hip.hip kernel_family(), csrc/k_bp.hip bp_variant());
this table pins every string, the wrappers of the decoders around the fixed one and the order in which they override one
another included.  Contexts are created and never decode."""
import pytest

pytestmark = pytest.mark.gpu

CRC24C = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)
CRC6 = (0, 1, 6)

SC_LANES = "k_sc_lanes<%s> (batches of 64+; k_scl_generic below)"
GLUE = "; glue k_ad_crc_check, k_ad_fail_count/scan/write, k_ad_gather, k_ad_scatter"
SCF = "k_scf_lanes<%s> (SC-Flip, T=%d; pass A, k_ad_fail_count/scan/write, record, pass B, k_scf_resolve)"

# polardecoding_amd.testing: KERNEL_AUTO .. KERNEL_FOUR_PER_WAVE
AUTO, GENERIC, GENERIC_SPILL, BIG, ONE_PER_WAVE, FOUR_PER_WAVE = range(6)
VARIANTS = ("auto", "generic", "generic_spill", "big", "one_per_wave", "four_per_wave")


def _make(kind, N, K, kw):
    import polardecoding_amd as pa
    kw = dict(kw)
    if kw.pop("f32", False):
        kw["dtype"] = pa.F32
    return {"SC": pa.SCdecode, "SCL": pa.SCLdecode, "CASCL": pa.CASCL, "BP": pa.BP, "SCF": pa.SCFlip, "SCAN": pa.SCAN,
            "PAC": pa.PAC, "PCCASCL": pa.PCCASCL}[kind](N, K, **kw)


def _lists(ty):
    """SCL and CA-SCL at N = 128 / 1024, L = 8: the name per polar_testing_select_kernel variant"""
    rows = []
    for kind, taps in (("SCL", None), ("CASCL", True)):
        for N in (1024, 128):
            kw = {"L": 8, "f32": True} if ty == "float" else {"L": 8}
            if taps:
                kw["crc_taps"] = CRC24C if N == 1024 else CRC6
            generic = f"k_scl_generic<{ty},L=8>"
            fast = f"k_scl_fast<{ty},N={N},L=8>"
            if N == 1024:
                names = (f"k_scl_fast2<{ty},N=1024,L=8>", generic, generic, f"k_scl_big<{ty},L=8>", fast,
                         f"k_scl_fast4<{ty},N=1024,L=8>")
            else:   # no pair or quad kernel and no k_scl_big below N = 512
                names = (fast, generic, generic, generic, fast, fast)
            rows.append((kind, N, N // 2, kw, names))
    return rows


SC_1024 = (SC_LANES % "double", "k_scl_generic<double,L=1>", "k_scl_generic<double,L=1>", SC_LANES % "double",
           SC_LANES % "double", SC_LANES % "double")
# stages (1, 8, 32) at N = 1024: the SC context, the L = 8 context and the context's own L = 32 decoder
ADAPTIVE = tuple("adaptive CA-SCL: L=1 %s -> L=8 %s -> L=32 %s" % st + GLUE for st in (
    (SC_LANES % "double", "k_scl_fast2<double,N=1024,L=8>", "k_scl_big<double,L=32>"),
    ("k_scl_generic<double,L=1>", "k_scl_generic<double,L=8>", "k_scl_generic<double,L=32>"),
    ("k_scl_generic<double,L=1>", "k_scl_generic<double,L=8>", "k_scl_generic<double,L=32>"),
    (SC_LANES % "double", "k_scl_big<double,L=8>", "k_scl_big<double,L=32>"),
    (SC_LANES % "double", "k_scl_fast<double,N=1024,L=8>", "k_scl_big<double,L=32>"),
    (SC_LANES % "double", "k_scl_fast4<double,N=1024,L=8>", "k_scl_big<double,L=32>")))
RM = "k_rm_recover, then "

# kind, N, K, constructor arguments, the name per variant (one string: the same under every variant)
TABLE = [
    ("SC", 1024, 512, {}, SC_1024),
    ("SC", 1024, 512, {"f32": True}, (SC_LANES % "float", "k_scl_generic<float,L=1>", "k_scl_generic<float,L=1>",
                                      SC_LANES % "float", SC_LANES % "float", SC_LANES % "float")),
    ("SC", 4096, 2048, {}, "k_scl_generic<double,L=1>"),
    *_lists("double"),
    *_lists("float"),
    ("SCL", 1024, 512, {"L": 32}, ("k_scl_big<double,L=32>", "k_scl_generic<double,L=32>", "k_scl_generic<double,L=32>",
                                   "k_scl_big<double,L=32>", "k_scl_big<double,L=32>", "k_scl_big<double,L=32>")),
    ("SCL", 256, 128, {"L": 4}, "k_scl_generic<double,L=4>"),
    ("SCL", 1024, 512, {"L": 1}, "k_scl_generic<double,L=1>"),
    ("BP", 1024, 512, {"iterMax": 10}, ("k_bp_r4<double>", "k_bp<double>", "k_bp<double>", "k_bp_r4<double>", "k_bp_r4<double>",
                                        "k_bp_r4<double>")),
    ("BP", 1024, 512, {"iterMax": 10, "early_stop": "g", "f32": True},
     ("k_bp_r4<float> (stop rule G)", "k_bp<float> (stop rule G)", "k_bp<float> (stop rule G)", "k_bp_r4<float> (stop rule G)",
      "k_bp_r4<float> (stop rule G)", "k_bp_r4<float> (stop rule G)")),
    ("BP", 128, 64, {"iterMax": 10}, ("k_bp_w128<double>", "k_bp<double>", "k_bp<double>", "k_bp_w128<double>",
                                      "k_bp_w128<double>", "k_bp_w128<double>")),
    ("BP", 128, 64, {"iterMax": 10, "early_stop": "g"},
     ("k_bp_w128<double> (stop rule G)", "k_bp<double> (stop rule G)", "k_bp<double> (stop rule G)",
      "k_bp_w128<double> (stop rule G)", "k_bp_w128<double> (stop rule G)", "k_bp_w128<double> (stop rule G)")),
    ("BP", 256, 128, {"iterMax": 10}, "k_bp<double>"),
    ("BP", 256, 128, {"iterMax": 10, "early_stop": "g"}, "k_bp<double> (stop rule G)"),
    ("SCF", 1024, 512, {"T": 8}, SCF % ("double", 8)),
    ("SCF", 128, 64, {"T": 3, "crc_taps": CRC6, "f32": True}, SCF % ("float", 3)),
    ("SCAN", 1024, 512, {"iters": 2}, "k_scan_lanes<double> (SCAN, I=2)"),
    ("CASCL", 1024, 512, {"L": 32, "stages": (1, 8, 32)}, ADAPTIVE),
    ("SC", 1024, 512, {"E": 2049}, tuple(RM + s for s in SC_1024)),
    ("CASCL", 1024, 512, {"L": 8, "E": 2049},
     (RM + "k_scl_fast2<double,N=1024,L=8>", RM + "k_scl_generic<double,L=8>", RM + "k_scl_generic<double,L=8>",
      RM + "k_scl_big<double,L=8>", RM + "k_scl_fast<double,N=1024,L=8>", RM + "k_scl_fast4<double,N=1024,L=8>")),
    ("CASCL", 1024, 512, {"L": 32, "stages": (1, 8, 32), "E": 2049}, tuple(RM + s for s in ADAPTIVE)),
    ("PCCASCL", 64, 14, {"L": 8}, "k_scl_dyn<double,L=8> (D=3 dynamic frozen bits)"),
    ("PAC", 128, 64, {"L": 32, "f32": True}, "k_scl_dyn<float,L=32> (D=64 dynamic frozen bits)"),
    ("PAC", 1024, 512, {"L": 8}, "k_scl_dyn<double,L=8> (D=512 dynamic frozen bits)"),
]


def _id(row):
    kind, N, K, kw, _ = row
    return "-".join([f"{kind}{N}"] + [f"{k}{'' if v is True else v}".replace(" ", "") for k, v in kw.items() if k != "crc_taps"])


@pytest.mark.parametrize("row", TABLE, ids=_id)
def test_kernel_name_is_exactly(row):
    from polardecoding_amd import testing as T
    kind, N, K, kw, names = row
    by_variant = names if isinstance(names, tuple) else (names,) * 6
    dec = _make(kind, N, K, kw)
    assert dec.kernel_name == by_variant[AUTO], "product library"
    for variant in (GENERIC, GENERIC_SPILL, BIG, ONE_PER_WAVE, FOUR_PER_WAVE, AUTO):   # the test library; back to auto last
        T.select_kernel(dec, variant)
        assert dec.kernel_name == by_variant[variant], VARIANTS[variant]
    dec.close()
