"""The cases of the sent-path trace tests, shared by tests/test_trace_host.py (CPU: the condition below, on the model) and
tests/test_gpu_trace.py (the kernels against the model), built from host code alone.

A case is a code, a list size and a pool of rows with their sent words: 96 frames of the transmit chain at 1.0 dB (0.0 dB with
a CRC) -- oracle.Sim(seed).frames for the 5G-ordered codes, tests/test_dyn_host.make_frames for the others -- and two planted
rows behind them, both noiseless: a sent u with a 1 on a frozen leaf (on the PAC case, where every frozen leaf is dynamic, with
a wrong dynamic bit), and an untouched one.  The seeds were chosen on the CPU so that the model alone meets the condition on
the 96 frames, the planted rows left out: a case without a CRC and with L >= 2 holds at least 5 frames of class 0, 2 of class 1 and 5 of class
2, a CRC case and the L = 1 case at least 5 each of classes 0 and 2, and every case at least 3 distinct loss leaves."""
import functools
import os

import numpy as np

import test_dyn_host as M
import test_encode_host as EH
import test_rm_host as RM
import trace_model as TM

HERE = os.path.dirname(os.path.abspath(__file__))
CRC6 = M.CRC6
FRAMES = 96

# name -> (kind, N, K, L, taps, seed); kind "plain" | "pac" | "rdyn" | "rm" | "sys" | "crcfile"
# K counts the payload bits; with a CRC the code has A = K + 6 information positions
CASES = {
    "n32-l4": ("plain", 32, 16, 4, None, 1),           # all history in the one-word register path
    "n64-l8": ("plain", 64, 32, 8, None, 2),           # the history rows in LDS
    "n64-crc6-l4": ("plain", 64, 26, 4, CRC6, 3),
    "n64-crc6-l8": ("plain", 64, 26, 8, CRC6, 4),
    "n128-l2": ("plain", 128, 64, 2, None, 5),         # S = 32 lanes per path
    "n128-l32": ("plain", 128, 64, 32, None, 1),       # S = 2
    "n32-l1": ("plain", 32, 16, 1, None, 6),
    "wide-n64-l64": ("plain", 64, 44, 64, None, 3),    # one wavefront
    "wide-n64-l128": ("plain", 64, 44, 128, None, 4),  # two wavefronts
    "pac64-l8": ("pac", 64, 32, 8, None, 1),
    "rdyn64-l4": ("rdyn", 64, 32, 4, None, 2),
    "rm-n64-e48-l8": ("rm", 64, 24, 8, None, 2),
    "sys-n64-crc6-l4": ("sys", 64, 26, 4, CRC6, 1),
    "crcfile-n64-l8": ("crcfile", 64, 26, 8, CRC6, 4),
}
E_RM = 48
CRC_FILE = os.path.join(HERE, "golden", "CRC_6.dat")


def case_db(name):
    return 0.0 if CASES[name][4] else 1.0


def case_code(name):
    """(information positions in the library's order, dyn or None, the model's crc argument or None)"""
    import polardecoding_amd as pa
    kind, N, K, L, taps, seed = CASES[name]
    A = K + (max(taps) if taps else 0)
    if kind == "pac":
        io = pa.pac_info_order(N, K, "rm")
        return io, pa.dyn_pac(N, io, M.G133), None
    if kind == "rm":
        return np.asarray(pa.rm_info_order(N, A, E_RM), dtype=np.int32), None, None
    io = np.asarray(pa.q_sequence(N)[N - A:], dtype=np.int32)
    if kind == "rdyn":
        frozen = np.ones(N, dtype=np.uint8)
        frozen[io] = 0
        return io, M.random_dyn(N, frozen, 5), None
    if kind == "sys":
        return io, None, EH.crc_table_sys(N, io, taps)
    return io, None, (io, taps) if taps else None


def decoder(name, dtype=0):
    import polardecoding_amd as pa
    kind, N, K, L, taps, seed = CASES[name]
    if kind == "pac":
        return pa.PAC(N, K, L=L, dtype=dtype)
    algo = pa.ALGO_CASCL if taps else pa.ALGO_SCL
    if kind == "crcfile":
        return pa.CASCL(N, K, L=L, crc_file=CRC_FILE, dtype=dtype)
    if kind == "rdyn":
        io, dyn, _ = case_code(name)
        return pa.Decoder(N, K, algo, L=L, dtype=dtype, dyn=dyn)
    return pa.Decoder(N, K, algo, L=L, crc_taps=taps, dtype=dtype, E=E_RM if kind == "rm" else None,
                      sys_polar=(kind == "sys"))


@functools.lru_cache(maxsize=None)
def pool(name):
    """(u [B][N] int32, llr [B][N] float64: the N-wide rows the decode works on, rows: what the entry point is given, j0: the
    planted frozen leaf): FRAMES frames, then the two planted rows.  rows is llr itself but on the rate-matched case, where it
    is [B][E_RM] and llr is its recovery by tests/test_rm_host.recover."""
    from oracle import oracle_py as O
    kind, N, K, L, taps, seed = CASES[name]
    io, dyn, _ = case_code(name)
    db = case_db(name)
    if kind == "plain":
        code = O.Code(N, K, taps)
        assert np.array_equal(code.info_order, io)
        sig = O.sigma_from_db(db)
        u, ys = O.Sim(seed).frames(code, sig, FRAMES)
        llr = np.stack([O.llr_from_y(y, sig) for y in ys])
    elif kind == "sys":
        rng = np.random.default_rng(seed)
        z = EH.place(rng.integers(0, 2, (FRAMES, K)).astype(np.uint8), N, io, taps)
        u, x = EH.sys_encode(z, io)
        sig = 10.0 ** (-db / 20.0)
        llr = 2.0 * ((1.0 - 2.0 * x) + sig * rng.standard_normal((FRAMES, N))) / sig / sig
    else:
        u, llr = M.make_frames(N, io, dyn, FRAMES, seed, dbs=(db,), crc=taps)
    u = np.asarray(u, dtype=np.int32)
    frozen = np.ones(N, dtype=bool)
    frozen[io] = False
    if dyn is not None:
        frozen[np.asarray(dyn[0])] = False
    forced = np.flatnonzero(frozen) if frozen.any() else np.asarray(dyn[0])   # PAC: every frozen leaf is dynamic
    j0 = int(forced[forced.size // 2])                                        # a forced leaf in the middle of the set
    planted_u = np.stack([u[0], u[1]])
    planted_u[0, j0] ^= 1
    planted_llr = 16.0 * (1.0 - 2.0 * M.encode(u[:2]).astype(np.float64))     # both noiseless: the first is lost at j0 alone
    u = np.concatenate([u, planted_u])
    llr = np.concatenate([llr, planted_llr])
    rows = llr
    if kind == "rm":
        # the E_RM sent values of every row, and what the decoder makes of them
        rows = np.ascontiguousarray(RM.transmit(llr, E_RM, K, False))
        llr = RM.recover(rows, N, K, False)
    for a in (u, llr, rows):
        a.setflags(write=False)
    return u, llr, rows, j0


@functools.lru_cache(maxsize=None)
def model(name, dtype=np.float64):
    """trace_model on the case's pool, once: (loss_leaf, loss_rank, rank, chosen, flags)"""
    kind, N, K, L, taps, seed = CASES[name]
    io, dyn, crc = case_code(name)
    u, llr, _, _ = pool(name)
    frozen = np.ones(N, dtype=np.uint8)
    frozen[io] = 0
    rows = llr
    if dtype == np.float32:
        rows = llr.astype(np.float32).astype(np.float64)
        if kind == "rm":
            rows = RM.recover(pool(name)[2].astype(np.float32).astype(np.float64), N, K, False, out_dtype=np.float32).astype(np.float64)
    out = TM.trace_model(frozen, dyn, rows, u, L, crc=crc, dtype=dtype)
    for a in out:
        a.setflags(write=False)
    return out


def check_condition(name, res):
    """the pool does not pass vacuously (the module docstring): counted over the FRAMES noisy frames, not the planted rows"""
    kind, N, K, L, taps, seed = CASES[name]
    loss_leaf, loss_rank, rank, chosen, flags = [a[:FRAMES] for a in res]
    n = np.bincount(TM.classes(rank, chosen), minlength=3)
    if taps or L == 1:
        assert n[0] >= 5 and n[2] >= 5, (name, n)
    else:
        assert n[0] >= 5 and n[1] >= 2 and n[2] >= 5, (name, n)
    assert np.unique(loss_leaf[loss_leaf < N]).size >= 3, name
    return n
