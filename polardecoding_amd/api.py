"""ctypes binding of libpolar_hip.so and the host-side mirror of the reference decode functions.

Reference call shape (SCL_1024.c:134, :263, :547):  ``void SCLdecode(double *y, int *u_hat)`` with
``N, K, n, L`` as #defines and ``std``, ``inI[]`` as globals.  Here the #defines/globals become the
constructor arguments of a decoder object and the call keeps its two data arguments::

    dec = SCLdecode(N=1024, K=512, L=8)       # SCL_1024.c:13-16
    u_hat = dec(y, sigma)                     # == std = sigma; SCLdecode(y, u_hat)

No CPU fallback exists: a missing library raises PolarError.
"""
import ctypes as C
import os

import numpy as np

ALGO_SC, ALGO_BP, ALGO_SCL, ALGO_CASCL, ALGO_SCF, ALGO_SCAN, ALGO_BPL = 0, 1, 2, 3, 4, 5, 6
F64, F32, Q8 = 0, 1, 2   # Q8: fixed-point min-sum on int8 LLRs (SC / SCL / CA-SCL, N <= 1024)
FLAG_TIE, FLAG_CRC_PASS, FLAG_RERANK, FLAG_BP_CONVERGED = 1, 2, 4, 8
FLAG_NO_CODE = 16   # code-book decodes only: the frame's code index was >= C
RM_NONE, RM_REPEAT, RM_PUNCTURE, RM_SHORTEN = 0, 1, 2, 3   # polar_rm_info modes (5G rate matching)
RM_SHORT_LLR = 1048576.0   # POLAR_RM_SHORT_LLR: the recovered value at a shortened position
BP_STOP_NONE, BP_STOP_G = 0, 1   # polar_bp_set_stop: iterMax round trips / stop at the first with u_hat F == x_hat
_BP_STOP_RULES = {None: BP_STOP_NONE, "none": BP_STOP_NONE, "g": BP_STOP_G, BP_STOP_NONE: BP_STOP_NONE, BP_STOP_G: BP_STOP_G}
CRC6_TAPS = (0, 5, 6)  # g(D) = D^6 + D^5 + 1 (CASCL_128.c:3)
CRC24C_TAPS = (0, 1, 2, 4, 8, 12, 13, 15, 17, 20, 21, 23, 24)  # CASCL_1024_L8.c:2-4

_HERE = os.path.dirname(os.path.abspath(__file__))


class PolarError(RuntimeError):
    pass


class _Cfg(C.Structure):
    _fields_ = [("N", C.c_int), ("K", C.c_int), ("crc_r", C.c_int), ("crc_taps", C.POINTER(C.c_int)),
                ("n_taps", C.c_int), ("L", C.c_int), ("algo", C.c_int), ("bp_iters", C.c_int),
                ("info_order", C.POINTER(C.c_int)), ("dtype", C.c_int), ("device", C.c_int),
                ("crc_systematic", C.c_int)]


class _Dyn(C.Structure):
    _fields_ = [("D", C.c_int), ("pos", C.POINTER(C.c_int)), ("ptr", C.POINTER(C.c_int)), ("idx", C.POINTER(C.c_int))]


class _CrcMatrix(C.Structure):
    _fields_ = [("K", C.c_int), ("r", C.c_int), ("n_taps", C.c_int), ("taps", C.c_int * 33),
                ("rows", C.POINTER(C.c_uint32))]


def lib_path(testing=False):
    return os.path.join(_HERE, "lib", "libpolar_hip_testing.so" if testing else "libpolar_hip.so")


_libs = {}


def load_library(testing=False):
    """Load libpolar_hip.so (built by __graft_entry__.build()).  Raises if absent: there is no fallback.
    testing=True: libpolar_hip_testing.so, the same sources plus the test-only entry points of
    include/polar_hip_testing.h (polardecoding_amd/testing.py; never used by the product)."""
    if testing in _libs:
        return _libs[testing]
    # torch bundles its own HIP runtime: it must be the first one loaded in the process, or torch later
    # finds "No HIP GPUs".  torch is only plumbing here (device buffers, streams, distributed).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    path = lib_path(testing)
    if not os.path.exists(path):
        raise PolarError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(path)
    vp, dp, ip, up = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint)
    L.polar_create.argtypes = [C.POINTER(_Cfg), C.POINTER(vp)]
    L.polar_destroy.argtypes = [vp]
    L.polar_create_crc_file.argtypes = [C.POINTER(_Cfg), C.c_char_p, C.POINTER(vp)]
    L.polar_crc_matrix_load.argtypes = [C.c_char_p, C.POINTER(_CrcMatrix)]
    L.polar_crc_matrix_free.argtypes = [C.POINTER(_CrcMatrix)]
    L.polar_crc_matrix_save.argtypes = [C.c_char_p, C.c_int, ip, C.c_int]
    L.polar_strerror.restype = C.c_char_p
    L.polar_strerror.argtypes = [C.c_int]
    L.polar_last_error.restype = C.c_char_p
    L.polar_last_error.argtypes = [vp]
    L.polar_decode.argtypes = [vp, dp, C.c_double, ip]
    L.polar_decode_llr.argtypes = [dp, C.POINTER(C.c_ubyte), C.c_int, C.c_int, ip]
    L.polar_decode_batch.argtypes = [vp, dp, C.POINTER(C.c_ubyte), C.c_size_t, ip, dp, up]
    L.polar_decode_batch_y.argtypes = [vp, dp, C.c_double, C.c_size_t, ip, dp, up]
    L.polar_decode_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, vp, vp]
    L.polar_count_errors_device.argtypes = [vp, vp, vp, C.c_size_t, vp, vp]
    L.polar_stop_rule_cut_device.argtypes = [vp, vp, C.c_size_t, C.c_uint, C.c_size_t, vp]
    L.polar_stop_rule_batch_y.argtypes = [vp, dp, C.c_double, vp, C.c_size_t, C.c_uint, C.c_size_t, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.polar_bp_set_stop.argtypes = [vp, C.c_int]
    L.polar_bp_decode_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, vp, vp]
    L.polar_bp_decode_batch.argtypes = [vp, dp, C.c_size_t, ip, up, up]
    L.polar_bp_readout_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, ip, C.c_int, vp, vp]
    L.polar_bp_readout_batch.argtypes = [vp, dp, C.c_double, C.c_size_t, ip, ip, C.c_int, C.POINTER(C.c_ulonglong), ip]
    L.polar_cascl_set_stages.argtypes = [vp, ip, C.c_int]
    L.polar_cascl_decode_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, vp, vp, vp]
    L.polar_cascl_decode_batch.argtypes = [vp, dp, C.c_size_t, ip, dp, up, up]
    L.polar_scf_set_flips.argtypes = [vp, C.c_int]
    L.polar_scf_decode_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, vp, vp]
    L.polar_scf_decode_batch.argtypes = [vp, dp, C.c_size_t, ip, up, up]
    L.polar_scf_set_dynamic.argtypes = [vp, ip, C.c_int, C.c_double, C.c_double]
    L.polar_scf_get_dynamic.argtypes = [vp, ip, ip, dp, dp]
    L.polar_scf_decode_sets_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, vp, vp, vp]
    L.polar_scf_decode_sets_batch.argtypes = [vp, dp, C.c_size_t, ip, up, up, ip]
    L.polar_bpl_set_graphs.argtypes = [vp, ip, C.c_int]
    L.polar_bpl_get_graphs.argtypes = [vp, ip, ip]
    L.polar_bpl_cyclic_graphs.argtypes = [C.c_int, C.c_int, ip]
    L.polar_bpl_decode_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, vp, vp, vp, vp]
    L.polar_bpl_decode_batch.argtypes = [vp, dp, C.c_size_t, ip, up, up, up, up]
    L.polar_scan_set_iters.argtypes = [vp, C.c_int]
    L.polar_scan_decode_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, vp, vp]
    L.polar_scan_decode_batch.argtypes = [vp, dp, C.c_size_t, ip, vp, vp]
    L.polar_generate_device.argtypes = [vp, C.c_ulonglong, C.c_ulonglong, C.c_double, C.c_size_t, vp, C.c_int,
                                        C.c_int, vp]
    L.polar_fer_batch.argtypes = [vp, C.c_ulonglong, C.c_ulonglong, C.c_double, C.c_size_t, C.POINTER(C.c_ulonglong),
                                  C.POINTER(C.c_ulonglong)]
    L.polar_fer_multi_gpu.argtypes = [C.POINTER(_Cfg), C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_double, C.c_size_t,
                                      C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)]
    L.polar_group_create.argtypes = [C.POINTER(_Cfg), C.c_int, C.POINTER(vp)]
    L.polar_group_destroy.argtypes = [vp]
    L.polar_group_size.argtypes = [vp]
    L.polar_group_fer_batch.argtypes = [vp, C.c_ulonglong, C.c_ulonglong, C.c_double, C.c_size_t, C.POINTER(C.c_ulonglong),
                                        C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)]
    L.polar_group_stop_rule_batch.argtypes = [vp, C.c_ulonglong, C.c_ulonglong, C.c_double, C.c_size_t, C.c_uint, C.c_size_t,
                                              C.POINTER(C.c_size_t), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.polar_set_stream.argtypes = [vp, vp]
    L.polar_get_stream.restype = vp
    L.polar_get_stream.argtypes = [vp]
    L.polar_synchronize.argtypes = [vp]
    L.polar_time_decode_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, C.c_int,
                                           C.POINTER(C.c_float)]
    L.polar_ctx_info.argtypes = [vp, ip, ip, ip, ip, ip, ip]
    L.polar_info_order.argtypes = [vp, ip, C.c_int]
    L.polar_rm_select_n.argtypes = [C.c_int, C.c_int, C.c_int]
    L.polar_rm_info_order.argtypes = [C.c_int, C.c_int, C.c_int, ip]
    L.polar_create_rm.argtypes = [C.POINTER(_Cfg), C.c_int, C.c_int, C.POINTER(vp)]
    L.polar_rm_info.argtypes = [vp, ip, ip, ip]
    L.polar_rm_recover_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp]
    L.polar_genie_count_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp]
    L.polar_genie_rows_device.argtypes = [vp, C.c_ulonglong, C.c_ulonglong, C.c_double, C.c_size_t, vp, C.c_int]
    L.polar_construct_batch.argtypes = [vp, C.c_ulonglong, C.c_ulonglong, C.c_double, C.c_size_t, vp]
    L.polar_construct_order.argtypes = [C.c_int, C.POINTER(C.c_uint64), ip, ip]
    L.polar_create_dyn.argtypes = [C.POINTER(_Cfg), C.POINTER(_Dyn), C.POINTER(vp)]
    L.polar_dyn_info.argtypes = [vp, ip, ip]
    L.polar_dyn_pac.argtypes = [C.c_int, ip, C.c_int, ip, C.c_int, ip, ip, ip, C.c_int, ip]
    L.polar_pac_precode.argtypes = [C.c_int, ip, C.c_int, ip, C.c_size_t, ip]
    L.polar_pac_unprecode.argtypes = [C.c_int, ip, C.c_int, ip, C.c_size_t, ip]
    L.polar_dyn_pc5g.argtypes = [C.c_int, ip, C.c_int, C.c_int, C.c_int, ip, ip, ip, C.c_int, ip, ip]
    L.polar_transform_device.argtypes = [vp, vp, C.c_size_t, vp]
    L.polar_encode_device.argtypes = [vp, vp, C.c_size_t, vp, vp]
    L.polar_payload_device.argtypes = [vp, vp, C.c_size_t, vp, vp]
    L.polar_encode_batch.argtypes = [vp, ip, C.c_size_t, ip, ip]
    L.polar_payload_batch.argtypes = [vp, ip, C.c_size_t, ip, up]
    L.polar_set_systematic.argtypes = [vp, C.c_int]
    L.polar_get_systematic.argtypes = [vp]
    L.polar_systematic_check.argtypes = [C.c_int, ip, C.c_int]
    L.polar_q8_set_quant.argtypes = [vp, C.c_double, C.c_int, C.c_int]
    L.polar_q8_get_quant.argtypes = [vp, dp, ip, ip]
    L.polar_q8_quantize_host.argtypes = [dp, C.c_size_t, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int8)]
    L.polar_q8_quantize_device.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp]
    L.polar_q8_decode_device.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
    L.polar_q8_decode_batch.argtypes = [vp, C.POINTER(C.c_int8), C.c_size_t, ip, C.POINTER(C.c_int32), up]
    L.polar_list_decode.argtypes = [vp, vp, C.c_int, C.c_double, C.c_size_t, vp, vp, vp, vp, vp]
    L.polar_list_decode_host.argtypes = [vp, dp, C.c_size_t, ip, dp, up, up, up]
    L.polar_list_select.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_int, vp]
    L.polar_list_gather.argtypes = [vp, vp, vp, C.c_int, C.c_size_t, vp]
    L.polar_list_soft.argtypes = [vp, vp, vp, vp, vp, C.c_uint, C.c_int, C.c_double, C.c_size_t, vp]
    L.polar_list_trace.argtypes = [vp, vp, C.c_int, C.c_double, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.polar_list_trace_count.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    L.polar_list_trace_host.argtypes = [vp, dp, ip, C.c_size_t, ip, up, ip, ip, up]
    L.polar_codebook_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp)]
    L.polar_codebook_destroy.argtypes = [vp]
    L.polar_codebook_destroy.restype = None
    L.polar_codebook_info.argtypes = [vp, ip, ip, ip, ip, ip]
    L.polar_codebook_member.argtypes = [vp, C.c_int, ip, ip, ip]
    L.polar_codebook_set_stream.argtypes = [vp, vp]
    L.polar_codebook_get_stream.restype = vp
    L.polar_codebook_get_stream.argtypes = [vp]
    L.polar_codebook_synchronize.argtypes = [vp]
    L.polar_codebook_kernel_name.restype = C.c_char_p
    L.polar_codebook_kernel_name.argtypes = [vp]
    L.polar_codebook_last_error.restype = C.c_char_p
    L.polar_codebook_last_error.argtypes = [vp]
    L.polar_codebook_decode.argtypes = [vp, vp, C.c_int, C.c_size_t, vp, C.c_double, C.c_size_t, vp, vp, vp]
    L.polar_codebook_list_decode.argtypes = [vp, vp, C.c_int, C.c_size_t, vp, C.c_double, C.c_size_t, vp, vp, vp, vp, vp]
    L.polar_codebook_decode_host.argtypes = [vp, dp, C.c_size_t, C.POINTER(C.c_uint32), C.c_double, C.c_size_t, ip, dp, up]
    L.polar_kernel_name.restype = C.c_char_p
    L.polar_kernel_name.argtypes = [vp]
    L.polar_version.restype = C.c_char_p
    _libs[testing] = L
    return L


def load_crc_matrix(path):
    """polar_crc_matrix_load: the reference's CRC_6.dat / Gc[K][r] generator-matrix file -> (taps of g(D), [K][r] uint8
    matrix).  Raises PolarError if the file is not such a matrix (a row that is not D^(r+i) mod g, ragged, not 0/1)."""
    lib = load_library()
    m = _CrcMatrix()
    rc = lib.polar_crc_matrix_load(os.fsencode(path), C.byref(m))
    if rc != 0:
        raise PolarError(f"polar_crc_matrix_load({path}): {lib.polar_strerror(rc).decode()} (rc={rc})")
    try:
        rows = np.ctypeslib.as_array(m.rows, shape=(m.K,)).copy()
        taps = tuple(int(m.taps[i]) for i in range(m.n_taps))
        mat = ((rows[:, None] >> np.arange(m.r, dtype=np.uint32)) & 1).astype(np.uint8)
    finally:
        lib.polar_crc_matrix_free(C.byref(m))
    return taps, mat


def save_crc_matrix(path, K, taps):
    """polar_crc_matrix_save: the K x r generator matrix of g(D) in the bytes of the reference's CRC_6.dat."""
    lib = load_library()
    t = np.asarray(list(taps), dtype=np.int32)
    rc = lib.polar_crc_matrix_save(os.fsencode(path), int(K), _ptr(t, C.c_int), len(t))
    if rc != 0:
        raise PolarError(f"polar_crc_matrix_save: {lib.polar_strerror(rc).decode()} (rc={rc})")


def q_sequence(N):
    """5G reliability order restricted to < N (what the reference hard-codes, SC_1024.c:42-91)."""
    vals = []
    with open(os.path.join(_HERE, "data", "q5g_nmax1024.txt")) as f:
        for line in f:
            if not line.startswith("#"):
                vals += [int(x) for x in line.split()]
    return [x for x in vals if x < N]


def _ptr(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


def q8_quantize(values, scale=2.0, qc=8, sigma=0.0):
    """polar_q8_quantize_host (include/polar_hip.h, fixed-point min-sum, rule 1): values of any shape -> int8 of that shape,
    rint(v * scale) clamped to +-(2^(qc-1) - 1), v = 2*y/sigma/sigma when sigma > 0.  Host only."""
    lib = load_library()
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = np.empty(v.shape, dtype=np.int8)
    rc = lib.polar_q8_quantize_host(_ptr(v, C.c_double), v.size, float(sigma), float(scale), int(qc), _ptr(out, C.c_int8))
    if rc != 0:
        raise PolarError(f"polar_q8_quantize_host: {lib.polar_strerror(rc).decode()} (rc={rc})")
    return out


def bpl_cyclic_graphs(n, P):
    """polar_bpl_cyclic_graphs: the cyclic shifts pi_s[b] = (b + s) mod n, s = 0 .. P-1, as an int32 array [P][n] (the default
    list of a BPL decoder is bpl_cyclic_graphs(n, min(n, 8))).  Host only."""
    lib = load_library()
    out = np.zeros((max(int(P), 1), max(int(n), 1)), dtype=np.int32)
    rc = lib.polar_bpl_cyclic_graphs(int(n), int(P), _ptr(out, C.c_int))
    if rc != 0:
        raise PolarError(f"polar_bpl_cyclic_graphs({n}, {P}): {lib.polar_strerror(rc).decode()} (rc={rc})")
    return out


def rm_select_n(A, E, n_max=10):
    """polar_rm_select_n: the block length 38.212 5.3.1 picks for A = K + r encoder bits sent as E values."""
    lib = load_library()
    rc = lib.polar_rm_select_n(int(A), int(E), int(n_max))
    if rc < 0:
        raise PolarError(f"polar_rm_select_n({A}, {E}, {n_max}): {lib.polar_strerror(rc).decode()} (rc={rc})")
    return rc


def rm_info_order(N, A, E):
    """polar_rm_info_order: I[0..A) of the rate-matched frozen set (include/polar_hip.h rule 4), ascending reliability."""
    lib = load_library()
    out = np.zeros(max(int(A), 1), dtype=np.int32)
    rc = lib.polar_rm_info_order(int(N), int(A), int(E), _ptr(out, C.c_int))
    if rc != 0:
        raise PolarError(f"polar_rm_info_order({N}, {A}, {E}): {lib.polar_strerror(rc).decode()} (rc={rc})")
    return out[:int(A)]


def systematic_check(N, info_order):
    """polar_systematic_check: True if the two-pass systematic polar encoder is valid for the information set `info_order`
    (every unit vector on it is encoded to a codeword that equals it on the set).  Host only."""
    io = np.ascontiguousarray(info_order, dtype=np.int32).ravel()
    rc = load_library().polar_systematic_check(int(N), _ptr(io, C.c_int), int(io.size))
    if rc < 0:
        raise PolarError(f"polar_systematic_check: rc={rc}")
    return bool(rc)


def pac_taps(g):
    """Exponents of a PAC generator polynomial.  An int is read as the usual octal shorthand with its most significant bit
    as g_0 (0o133 = 1011011 -> g_0 g_1 .. g_6 = 1,0,1,1,0,1,1 -> exponents 0, 2, 3, 5, 6); a sequence is taken as exponents."""
    if isinstance(g, (int, np.integer)):
        bits = bin(int(g))[2:]
        return tuple(i for i, c in enumerate(bits) if c == "1")
    return tuple(int(t) for t in g)


def _csr_sets(pos, ptr, idx):
    return [idx[ptr[d]:ptr[d + 1]].copy() for d in range(len(pos))]


def dyn_pac(N, info_order, g=0o133):
    """polar_dyn_pac: the dynamic frozen bits of the PAC code with information set `info_order` and precoder polynomial g
    (pac_taps) -> (pos, sets): every position outside the information set, and per position the earlier positions whose
    decided bits it is the XOR of.  Feeds ``Decoder(..., dyn=(pos, sets))``.  Host only."""
    lib = load_library()
    io = np.ascontiguousarray(info_order, dtype=np.int32)
    t = np.asarray(pac_taps(g), dtype=np.int32)
    D = int(N) - io.size
    pos = np.zeros(max(D, 1), dtype=np.int32)
    ptr = np.zeros(D + 1, dtype=np.int32)
    nnz = C.c_int(0)
    args = (int(N), _ptr(io, C.c_int), io.size, _ptr(t, C.c_int), t.size, _ptr(pos, C.c_int), _ptr(ptr, C.c_int))
    rc = lib.polar_dyn_pac(*args, None, 0, C.byref(nnz))
    idx = np.zeros(max(nnz.value, 1), dtype=np.int32)
    if rc == 0:
        rc = lib.polar_dyn_pac(*args, _ptr(idx, C.c_int), idx.size, None)
    if rc != 0:
        raise PolarError(f"polar_dyn_pac: {lib.polar_strerror(rc).decode()} (rc={rc})")
    return pos[:D], _csr_sets(pos[:D], ptr, idx)


def _pac_rows(fn, N, g, rows):
    lib = load_library()
    a = np.ascontiguousarray(rows, dtype=np.int32)
    if a.ndim == 0 or a.shape[-1] != N:
        raise ValueError(f"rows must have {N} bits")
    t = np.asarray(pac_taps(g), dtype=np.int32)
    out = np.zeros_like(a)
    rc = getattr(lib, fn)(int(N), _ptr(t, C.c_int), t.size, _ptr(a, C.c_int), a.size // N, _ptr(out, C.c_int))
    if rc != 0:
        raise PolarError(f"{fn}: {lib.polar_strerror(rc).decode()} (rc={rc})")
    return out


def pac_precode(v, g=0o133):
    """polar_pac_precode: bit rows [..][N], u = v T (T_ij = g_{j-i}); v is zero outside the information set."""
    return _pac_rows("polar_pac_precode", np.shape(v)[-1], g, v)


def pac_unprecode(u, g=0o133):
    """polar_pac_unprecode: bit rows [..][N], v = u T^-1: the payload of a decoded PAC row sits at the information positions."""
    return _pac_rows("polar_pac_unprecode", np.shape(u)[-1], g, u)


def dyn_pc5g(N, q_i, n_pc=3, n_pc_wm=0):
    """polar_dyn_pc5g (38.212 5.3.1.2): q_i = Q_I in ascending reliability (K + n_pc entries, K counting the CRC) ->
    (pos, sets, info_order): the PC positions, their sets, and Q_I without them in ascending reliability (what
    ``Decoder(info_order=...)`` takes).  Host only."""
    lib = load_library()
    q = np.ascontiguousarray(q_i, dtype=np.int32)
    D = int(n_pc)
    pos = np.zeros(max(D, 1), dtype=np.int32)
    ptr = np.zeros(D + 1, dtype=np.int32)
    info = np.zeros(max(q.size - D, 1), dtype=np.int32)
    nnz = C.c_int(0)
    args = (int(N), _ptr(q, C.c_int), q.size, D, int(n_pc_wm), _ptr(pos, C.c_int), _ptr(ptr, C.c_int))
    rc = lib.polar_dyn_pc5g(*args, None, 0, C.byref(nnz), _ptr(info, C.c_int))
    idx = np.zeros(max(nnz.value, 1), dtype=np.int32)
    if rc == 0:
        rc = lib.polar_dyn_pc5g(*args, _ptr(idx, C.c_int), idx.size, None, _ptr(info, C.c_int))
    if rc != 0:
        raise PolarError(f"polar_dyn_pc5g: {lib.polar_strerror(rc).decode()} (rc={rc})")
    return pos[:D], _csr_sets(pos[:D], ptr, idx), info[:q.size - D]


def construct_order(N, counts, base_order=None):
    """polar_construct_order (include/polar_hip.h, Monte-Carlo construction rule 4): counts [2][N] (err row, tie row) -> the
    N positions in ascending reliability (descending 2*err + tie, equal scores in `base_order`; None: the library's own order
    for N).  ``order[N - A:]`` is an ``info_order`` for A unfrozen positions.  Host only."""
    lib = load_library()
    cnt = np.ascontiguousarray(counts, dtype=np.uint64)
    if cnt.shape != (2, int(N)):
        raise ValueError(f"counts must have shape (2, {N})")
    base = None
    if base_order is not None:
        base = np.ascontiguousarray(base_order, dtype=np.int32)
        if base.shape != (int(N),):
            raise ValueError(f"base_order must have shape ({N},)")
    out = np.zeros(int(N), dtype=np.int32)
    rc = lib.polar_construct_order(int(N), _ptr(cnt, C.c_uint64), _ptr(base, C.c_int) if base is not None else None,
                                   _ptr(out, C.c_int))
    if rc != 0:
        raise PolarError(f"polar_construct_order({N}): {lib.polar_strerror(rc).decode()} (rc={rc})")
    return out


def construct_mc(N, sigma, frames, seed=0, dtype=F64, device=0, base_order=None, batch=1 << 16):
    """Monte-Carlo construction for design noise `sigma`: genie-aided SC of `frames` all-zero codewords on the device
    (Decoder.construct_batch, `batch` frames per call) -> (order, counts).  order: the N positions in ascending reliability
    (``order[N - A:]`` feeds ``SCLdecode(N, K, info_order=...)`` and the others); counts: uint64 [2][N] (err row, tie row)."""
    import torch
    dec = Decoder(N, N // 2, ALGO_SC, dtype=dtype, device=device)
    try:
        d_counts = torch.zeros((2, N), dtype=torch.int64, device=f"cuda:{device}")
        done = 0
        while done < frames:
            nb = min(int(batch), int(frames) - done)
            dec.construct_batch(seed, done, sigma, nb, d_counts)
            done += nb
        dec.synchronize()
        counts = d_counts.cpu().numpy().view(np.uint64)
    finally:
        dec.close()
    return construct_order(N, counts, base_order), counts


class Decoder:
    """One polar_ctx: a (N, K, CRC, L, algo, dtype) configuration bound to one GPU."""

    def __init__(self, N, K, algo, L=1, crc_taps=None, bp_iters=100, dtype=F64, device=0, info_order=None,
                 systematic=False, crc_file=None, E=None, ibil=False, dyn=None, sys_polar=False, quant=None, _library=None):
        """quant = (scale, qc, qi): the quantiser of a dtype=Q8 decoder (polar_q8_set_quant; None: scale 2.0, 8 and 8 bits).
        dyn = (pos, sets): dynamic frozen bits (polar_create_dyn): pos ascending frozen positions, sets[d] the earlier
        positions whose decided bits u_hat[pos[d]] is the XOR of (SC / SCL / CA-SCL only; see dyn_pac, dyn_pc5g).
        E: 5G rate matching (polar_create_rm): every decode takes rows of E channel values and generate_device writes
        them; ibil: with the channel interleaver (uplink).
        sys_polar: systematic polar code (polar_set_systematic; not to be confused with `systematic`, the systematic CRC)."""
        self._h = C.c_void_p()
        if E is not None and crc_file is not None:
            raise ValueError("E (rate matching) and crc_file exclude each other: polar_create_crc_file takes no E")
        if dyn is not None and (E is not None or crc_file is not None):
            raise ValueError("dyn (dynamic frozen bits) excludes E and crc_file")
        self._lib = _library if _library is not None else load_library()
        self.N, self.K, self.algo, self.dtype, self.device = N, K, algo, dtype, device
        taps = np.asarray(list(crc_taps) if crc_taps else [0], dtype=np.int32)
        cfg = _Cfg()
        cfg.N, cfg.K = N, K
        cfg.crc_r = int(max(taps)) if crc_taps else 0
        cfg.crc_taps = _ptr(taps, C.c_int)
        cfg.n_taps = len(taps) if crc_taps else 0
        cfg.L, cfg.algo, cfg.bp_iters, cfg.dtype, cfg.device = L, algo, bp_iters, dtype, device
        cfg.crc_systematic = 1 if systematic else 0   # CASCL_1024_sys.c: encoder and error metric only
        self.systematic = bool(systematic)
        io = None
        if info_order is not None:
            io = np.ascontiguousarray(info_order, dtype=np.int32)
            cfg.info_order = _ptr(io, C.c_int)
        self._crc_file = os.fsencode(crc_file) if crc_file is not None else None   # g(D) and r from a generator-matrix file
        self._cfg, self._cfg_keep = cfg, (taps, io)   # kept for polar_fer_multi_gpu (the arrays the struct points to must stay alive)
        self.bp_stop = BP_STOP_NONE
        self.cascl_stages = ()
        self.scf_flips = None   # None: the library's default (min(8, K + r))
        self.scf_dynamic = None   # None: the static rule; else (budgets, c, tau) of set_scf_dynamic
        self.scan_iters = None  # None: the library's default (4)
        self._bpl_graphs = None # None: the library's default list (min(n, 8) cyclic shifts)
        self._chunk_bytes = 0   # test-only cap of the chunked passes (testing.chunk_bytes); 0: the library's 256 MiB
        self._resident_blocks = 0   # test-only cap of the resident grid (testing.resident_blocks); 0: the library's choice
        self._rm = (int(E), 1 if ibil else 0) if E is not None else None
        self._dyn = None
        if dyn is not None:
            dpos = np.ascontiguousarray(dyn[0], dtype=np.int32).ravel()
            sets = [np.asarray(s, dtype=np.int32).ravel() for s in dyn[1]]
            if len(sets) != dpos.size:
                raise ValueError("dyn = (pos, sets) needs one set per position")
            dptr = np.zeros(dpos.size + 1, dtype=np.int32)
            dptr[1:] = np.cumsum([s.size for s in sets])
            didx = np.ascontiguousarray(np.concatenate(sets + [np.zeros(0, dtype=np.int32)]), dtype=np.int32)
            self._dyn = (dpos, dptr, didx)
        self._create()
        if crc_file is not None:
            # g(D) lives only inside polar_create_crc_file: every other consumer of the cfg (polar_group_create,
            # polar_fer_multi_gpu) must see it too
            ftaps = np.asarray(load_crc_matrix(crc_file)[0], dtype=np.int32)
            cfg.crc_r, cfg.crc_taps, cfg.n_taps = int(ftaps.max()), _ptr(ftaps, C.c_int), int(ftaps.size)
            self._cfg_keep = (ftaps, io)
        A, Lr = C.c_int(), C.c_int()
        self._lib.polar_ctx_info(self._h, None, None, C.byref(A), C.byref(Lr), None, None)
        self.A, self.L = A.value, Lr.value
        self.NW = N // 32
        e, mode, il = C.c_int(), C.c_int(), C.c_int()
        self._lib.polar_rm_info(self._h, C.byref(e), C.byref(mode), C.byref(il))
        self.E, self.rm_mode, self.ibil = e.value, mode.value, bool(il.value)   # plain: E = N, RM_NONE
        self._w = self.E   # values per input row of every decode entry point
        self._sys_polar = False
        if sys_polar:
            self.set_systematic(True)
        self._quant = None
        if quant is not None:
            self.set_quant(*quant)

    def _create(self):
        if self._dyn is not None:
            dpos, dptr, didx = self._dyn
            d = _Dyn(dpos.size, _ptr(dpos, C.c_int), _ptr(dptr, C.c_int), _ptr(didx, C.c_int))
            rc = self._lib.polar_create_dyn(C.byref(self._cfg), C.byref(d), C.byref(self._h))
        elif self._rm is not None:
            rc = self._lib.polar_create_rm(C.byref(self._cfg), self._rm[0], self._rm[1], C.byref(self._h))
        elif self._crc_file is not None:
            rc = self._lib.polar_create_crc_file(C.byref(self._cfg), self._crc_file, C.byref(self._h))
        else:
            rc = self._lib.polar_create(C.byref(self._cfg), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise PolarError(f"polar_create: {self._lib.polar_strerror(rc).decode()} (rc={rc})")

    def _rebind(self, lib):
        """Re-create this decoder's context inside another build of the library (polardecoding_amd/testing.py)."""
        if lib is self._lib:
            return
        if (self._chunk_bytes or self._resident_blocks) and not hasattr(lib, "polar_testing_resident_blocks"):
            raise PolarError("this decoder carries a test-only cap (testing.chunk_bytes / testing.resident_blocks): set it to 0 "
                             "before moving the decoder into a library without the test entry points")
        self.close()
        self._lib = lib
        self._create()
        if self.bp_stop != BP_STOP_NONE:
            self.set_bp_stop(self.bp_stop)
        if self.cascl_stages:
            self.set_cascl_stages(self.cascl_stages)
        if self.scf_flips is not None:
            self.set_scf_flips(self.scf_flips)
        if self.scf_dynamic is not None:
            self.set_scf_dynamic(*self.scf_dynamic)
        if self.scan_iters is not None:
            self.set_scan_iters(self.scan_iters)
        if self._bpl_graphs is not None:
            self.set_bpl_graphs(self._bpl_graphs)
        if self._sys_polar:
            self._sys_polar = False
            self.set_systematic(True)
        if self._quant is not None:
            self.set_quant(*self._quant)
        if self._chunk_bytes:   # only a test library has the setter
            lib.polar_testing_chunk_bytes.argtypes = [C.c_void_p, C.c_size_t]
            self._check(lib.polar_testing_chunk_bytes(self._h, self._chunk_bytes), "polar_testing_chunk_bytes")
        if self._resident_blocks:
            lib.polar_testing_resident_blocks.argtypes = [C.c_void_p, C.c_int]
            self._check(lib.polar_testing_resident_blocks(self._h, self._resident_blocks), "polar_testing_resident_blocks")

    @property
    def info_order(self):
        """I[0..A): unfrozen positions in reliability order (the reference's global I[])."""
        out = np.zeros(self.A, dtype=np.int32)
        self._check(self._lib.polar_info_order(self._h, _ptr(out, C.c_int), self.A), "polar_info_order")
        return out

    @property
    def dyn_positions(self):
        """polar_dyn_info: the dynamic frozen positions (ascending), or None on a decoder made without dyn."""
        D = C.c_int()
        self._check(self._lib.polar_dyn_info(self._h, C.byref(D), None), "polar_dyn_info")
        if D.value < 0:
            return None
        out = np.zeros(max(D.value, 1), dtype=np.int32)
        self._check(self._lib.polar_dyn_info(self._h, None, _ptr(out, C.c_int)), "polar_dyn_info")
        return out[:D.value]

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.polar_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.polar_strerror(rc).decode()
            det = self._lib.polar_last_error(self._h).decode()
            raise PolarError(f"{what}: {msg} {det} (rc={rc})")

    def set_bp_stop(self, rule):
        """BP early termination (polar_bp_set_stop): None / "none" / BP_STOP_NONE runs iterMax round trips (the reference),
        "g" / BP_STOP_G stops a frame at the first round trip whose decisions form a codeword (u_hat F == x_hat)."""
        if rule not in _BP_STOP_RULES:
            raise ValueError(f"unknown BP stop rule {rule!r}: None, 'none' or 'g'")
        code = _BP_STOP_RULES[rule]
        self._check(self._lib.polar_bp_set_stop(self._h, code), "polar_bp_set_stop")
        self.bp_stop = code

    def set_cascl_stages(self, stages):
        """Adaptive CA-SCL (polar_cascl_set_stages): decode with the first list size, re-decode only the frames whose chosen
        path fails the CRC with the next, up to cfg.L (stages[-1] must equal L; 1 = SC).  () or None restores the default."""
        st = np.asarray(list(stages) if stages else [], dtype=np.int32)
        self._check(self._lib.polar_cascl_set_stages(self._h, _ptr(st, C.c_int) if st.size else None, int(st.size)),
                    "polar_cascl_set_stages")
        self.cascl_stages = tuple(int(x) for x in st) if st.size > 1 else ()

    def set_scf_flips(self, T):
        """SC-Flip flip budget (polar_scf_set_flips): up to T single-flip attempts per CRC-failing frame, 0 <= T <=
        min(32, K + r); T = 0 is SC plus the CRC flag."""
        self._check(self._lib.polar_scf_set_flips(self._h, int(T)), "polar_scf_set_flips")
        self.scf_flips = int(T)
        if self.scf_dynamic is not None:   # T_1 of the dynamic rule
            b, c, tau = self.scf_dynamic
            self.scf_dynamic = ((int(T),) + tuple(b[1:]), c, tau)

    def set_scf_dynamic(self, budgets, c=0.0, tau=0.0):
        """Dynamic SC-Flip (polar_scf_set_dynamic): flip sets of up to len(budgets) <= 3 positions, budgets[k] sets of size
        k + 1 per CRC-failing frame (each 1 .. 32), ranked by M = |lambda| sums + c * (count of |lambda| <= tau).  budgets[0]
        becomes the flip budget T.  None or () restores the static rule and keeps T."""
        b = np.asarray(list(budgets) if budgets is not None else [], dtype=np.int32)
        self._check(self._lib.polar_scf_set_dynamic(self._h, _ptr(b, C.c_int) if b.size else None, int(b.size), float(c),
                                                    float(tau)), "polar_scf_set_dynamic")
        if b.size:
            self.scf_dynamic = (tuple(int(x) for x in b), float(c), float(tau))
            self.scf_flips = int(b[0])
        else:
            self.scf_dynamic = None

    def get_scf_dynamic(self):
        """polar_scf_get_dynamic: (budgets, c, tau) with budgets a tuple of omega entries; ((), 0.0, 0.0) on the static rule."""
        om = C.c_int()
        b = np.zeros(3, dtype=np.int32)
        c, tau = C.c_double(), C.c_double()
        self._check(self._lib.polar_scf_get_dynamic(self._h, C.byref(om), _ptr(b, C.c_int), C.byref(c), C.byref(tau)),
                    "polar_scf_get_dynamic")
        return tuple(int(x) for x in b[:om.value]), c.value, tau.value

    def set_scan_iters(self, iters):
        """SCAN iteration count (polar_scan_set_iters): 1 <= iters <= 64, default 4."""
        self._check(self._lib.polar_scan_set_iters(self._h, int(iters)), "polar_scan_set_iters")
        self.scan_iters = int(iters)

    def set_bpl_graphs(self, graphs):
        """BP list decoding (polar_bpl_set_graphs): the ordered list of factor graphs, [P][n] permutations of 0 .. n-1 with
        1 <= P <= 32; pi[b] is the index bit that bit b of a position moves to.  Refused (PolarError, decoder unchanged) on a
        decoder that is not BPL and for a row that is not a permutation."""
        n = self.N.bit_length() - 1
        g = np.ascontiguousarray(graphs, dtype=np.int32)
        if g.ndim != 2 or g.shape[1] != n:
            raise ValueError(f"graphs must have shape [P][{n}]")
        self._check(self._lib.polar_bpl_set_graphs(self._h, _ptr(g, C.c_int), int(g.shape[0])), "polar_bpl_set_graphs")
        self._bpl_graphs = g.copy()

    @property
    def bpl_graphs(self):
        """polar_bpl_get_graphs: the list of a BPL decoder as an int32 array [P][n]"""
        P = C.c_int()
        self._check(self._lib.polar_bpl_get_graphs(self._h, C.byref(P), None), "polar_bpl_get_graphs")
        out = np.zeros((P.value, self.N.bit_length() - 1), dtype=np.int32)
        self._check(self._lib.polar_bpl_get_graphs(self._h, None, _ptr(out, C.c_int)), "polar_bpl_get_graphs")
        return out

    def set_systematic(self, on):
        """Systematic polar code (polar_set_systematic): the codeword carries the CRC word on the information set.  Refused
        (PolarError, decoder unchanged) on dynamic and rate-matched decoders and when systematic_check fails."""
        self._check(self._lib.polar_set_systematic(self._h, 1 if on else 0), "polar_set_systematic")
        self._sys_polar = bool(on)

    def set_quant(self, scale, qc=8, qi=8):
        """polar_q8_set_quant (dtype=Q8 decoders): scale > 0, 2 <= qc <= qi <= 8 bits for the channel / the internal LLRs."""
        self._check(self._lib.polar_q8_set_quant(self._h, float(scale), int(qc), int(qi)), "polar_q8_set_quant")
        self._quant = (float(scale), int(qc), int(qi))

    @property
    def quant(self):
        """polar_q8_get_quant: (scale, qc, qi) of a dtype=Q8 decoder"""
        sc, qc, qi = C.c_double(), C.c_int(), C.c_int()
        self._check(self._lib.polar_q8_get_quant(self._h, C.byref(sc), C.byref(qc), C.byref(qi)), "polar_q8_get_quant")
        return sc.value, qc.value, qi.value

    def quantize(self, rows, sigma=0.0):
        """rule 1 with this decoder's quantiser on host values (q8_quantize): rows of LLRs, or of y when sigma > 0 -> int8"""
        sc, qc, _ = self.quant
        return q8_quantize(rows, sc, qc, sigma)

    def quantize_device(self, d_in, sigma=0.0, out=None):
        """polar_q8_quantize_device: d_in [B][N] float64 / float32 CUDA tensor -> int8 tensor [B][N].  Asynchronous."""
        import torch
        B = self._dev_rows(d_in)
        if d_in.dtype not in (torch.float64, torch.float32):
            raise ValueError("input must be float64 or float32")
        if out is None:
            out = torch.empty((B, self.N), dtype=torch.int8, device=d_in.device)
        if out.dtype != torch.int8 or not out.is_contiguous() or out.numel() < B * self.N:
            raise ValueError("out must be a contiguous int8 tensor with B * N elements")
        self._check(self._lib.polar_q8_quantize_device(self._h, C.c_void_p(d_in.data_ptr()), 1 if d_in.dtype == torch.float32 else 0,
                                                       float(sigma), B, C.c_void_p(out.data_ptr())), "polar_q8_quantize_device")
        return out

    def decode_q8_device(self, d_q, out_bits=None, pm=None, flags=None):
        """polar_q8_decode_device: d_q int8 CUDA tensor [B][N] -> out_bits int32 [B][N/32]; pm (int32 [B]) and flags (int32
        [B]) are optional tensors.  Asynchronous, no read-back."""
        import torch
        B = self._dev_rows(d_q)
        if d_q.dtype != torch.int8:
            raise ValueError("input must be int8")
        if out_bits is None:
            out_bits = torch.empty((B, self.NW), dtype=torch.int32, device=d_q.device)
        for t in (pm, flags):
            if t is not None and (t.numel() < B or t.element_size() != 4 or not t.is_contiguous()):
                raise ValueError("pm / flags must be contiguous 32-bit tensors of at least B elements")
        self._check(self._lib.polar_q8_decode_device(
            self._h, C.c_void_p(d_q.data_ptr()), B, C.c_void_p(out_bits.data_ptr()),
            C.c_void_p(pm.data_ptr()) if pm is not None else None,
            C.c_void_p(flags.data_ptr()) if flags is not None else None), "polar_q8_decode_device")
        return out_bits

    def decode_q8_batch(self, q):
        """polar_q8_decode_batch: q int8 [B][N] -> (u_hat [B][N] int32, pm [B] int32, flags [B] uint32)"""
        q = np.ascontiguousarray(q, dtype=np.int8)
        if q.ndim == 0 or q.shape[-1] != self.N:
            raise ValueError(f"rows must have {self.N} values (shape [B][{self.N}])")
        q = q.reshape(-1, self.N)
        B = q.shape[0]
        uh = np.empty((B, self.N), dtype=np.int32)
        pm = np.zeros(B, dtype=np.int32)
        fl = np.zeros(B, dtype=np.uint32)
        self._check(self._lib.polar_q8_decode_batch(self._h, _ptr(q, C.c_int8), B, _ptr(uh, C.c_int), _ptr(pm, C.c_int32),
                                                    _ptr(fl, C.c_uint)), "polar_q8_decode_batch")
        return uh, pm, fl

    @property
    def sys_polar(self):
        return bool(self._lib.polar_get_systematic(self._h))

    @property
    def kernel_name(self):
        return self._lib.polar_kernel_name(self._h).decode()

    def _rows(self, x):
        """host rows of this decoder's width (N, or E on a rate-matched decoder) as float64 [B][width]"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim == 0 or x.shape[-1] != self._w:
            raise ValueError(f"rows must have {self._w} values (shape [B][{self._w}])")
        return x.reshape(-1, self._w)

    def _dev_rows(self, d):
        if not (d.is_cuda and d.is_contiguous()) or d.dim() == 0 or d.shape[-1] != self._w:
            raise ValueError(f"device rows must be a contiguous CUDA tensor of shape [B][{self._w}]")
        return d.numel() // self._w

    # ---- host buffers -------------------------------------------------------------------------------
    def __call__(self, y, sigma):
        """Reference call shape: channel observations y[N] and sigma (the global ``std``) -> u_hat[N]."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (self._w,):
            raise ValueError(f"y must have shape ({self._w},)")
        uh = np.empty(self.N, dtype=np.int32)
        self._check(self._lib.polar_decode(self._h, _ptr(y, C.c_double), float(sigma), _ptr(uh, C.c_int)),
                    "polar_decode")
        return uh

    def decode_batch(self, llr, frozen_mask=None, want_pm=True, out=None):
        """out: optional int32 [B][N] array to receive u_hat (a caller that keeps its buffers, as the reference does, pays
        no page faults for a fresh half-gigabyte array per call)."""
        llr = self._rows(llr)
        B = llr.shape[0]
        if out is not None:
            if out.dtype != np.int32 or out.shape != (B, self.N) or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous int32 array of shape (B, N)")
            uh = out
        else:
            uh = np.empty((B, self.N), dtype=np.int32)
        pm = np.zeros(B, dtype=np.float64)
        fl = np.zeros(B, dtype=np.uint32)
        fm = None
        if frozen_mask is not None:
            fm = np.ascontiguousarray(frozen_mask, dtype=np.uint8)
        self._check(self._lib.polar_decode_batch(self._h, _ptr(llr, C.c_double),
                                                 _ptr(fm, C.c_ubyte) if fm is not None else None, B,
                                                 _ptr(uh, C.c_int), _ptr(pm, C.c_double), _ptr(fl, C.c_uint)),
                    "polar_decode_batch")
        return uh, pm, fl

    def decode_batch_y(self, y, sigma):
        y = self._rows(y)
        B = y.shape[0]
        uh = np.empty((B, self.N), dtype=np.int32)
        pm = np.zeros(B, dtype=np.float64)
        fl = np.zeros(B, dtype=np.uint32)
        self._check(self._lib.polar_decode_batch_y(self._h, _ptr(y, C.c_double), float(sigma), B,
                                                   _ptr(uh, C.c_int), _ptr(pm, C.c_double), _ptr(fl, C.c_uint)),
                    "polar_decode_batch_y")
        return uh, pm, fl

    # ---- device buffers (torch tensors on this ctx's GPU) ---------------------------------------------
    def use_torch_stream(self):
        """Run on torch's current stream so that torch ops and decodes are ordered."""
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.polar_set_stream(self._h, C.c_void_p(s)), "polar_set_stream")

    def decode_device(self, d_in, sigma=0.0, out_bits=None, pm=None, flags=None):
        """d_in: torch CUDA tensor [B][N] float64 or float32 (LLRs, or y if sigma > 0).
        Returns out_bits: int32 tensor [B][N/32] (bit j&31 of word j>>5 = u_hat[j])."""
        import torch
        B = self._dev_rows(d_in)
        if out_bits is None:
            out_bits = torch.empty((B, self.NW), dtype=torch.int32, device=d_in.device)
        f32 = 1 if d_in.dtype == torch.float32 else 0
        if not f32 and d_in.dtype != torch.float64:
            raise ValueError("input must be float64 or float32")
        self._check(self._lib.polar_decode_device(
            self._h, C.c_void_p(d_in.data_ptr()), f32, float(sigma), B, C.c_void_p(out_bits.data_ptr()),
            C.c_void_p(pm.data_ptr()) if pm is not None else None,
            C.c_void_p(flags.data_ptr()) if flags is not None else None), "polar_decode_device")
        return out_bits

    def decode_bp_device(self, d_in, sigma=0.0, out_bits=None, iters=None, flags=None):
        """polar_bp_decode_device: like decode_device, plus per frame the round trips run (`iters`, int32 [B]) and
        FLAG_BP_CONVERGED (`flags`, int32 [B]); both optional tensors.  Returns out_bits."""
        import torch
        B = self._dev_rows(d_in)
        if out_bits is None:
            out_bits = torch.empty((B, self.NW), dtype=torch.int32, device=d_in.device)
        f32 = 1 if d_in.dtype == torch.float32 else 0
        if not f32 and d_in.dtype != torch.float64:
            raise ValueError("input must be float64 or float32")
        for t in (iters, flags):
            if t is not None and (t.numel() < B or t.element_size() != 4 or not t.is_contiguous()):
                raise ValueError("iters / flags must be contiguous 32-bit tensors of at least B elements")
        self._check(self._lib.polar_bp_decode_device(
            self._h, C.c_void_p(d_in.data_ptr()), f32, float(sigma), B, C.c_void_p(out_bits.data_ptr()),
            C.c_void_p(iters.data_ptr()) if iters is not None else None,
            C.c_void_p(flags.data_ptr()) if flags is not None else None), "polar_bp_decode_device")
        return out_bits

    def decode_cascl_device(self, d_in, sigma=0.0, out_bits=None, pm=None, flags=None, list_size=None):
        """polar_cascl_decode_device: like decode_device, plus per frame the list size of the stage that decided it
        (`list_size`, int32 [B], 1 = SC); pm (float64 [B]), flags and list_size are optional tensors.  Returns out_bits."""
        import torch
        B = self._dev_rows(d_in)
        if out_bits is None:
            out_bits = torch.empty((B, self.NW), dtype=torch.int32, device=d_in.device)
        f32 = 1 if d_in.dtype == torch.float32 else 0
        if not f32 and d_in.dtype != torch.float64:
            raise ValueError("input must be float64 or float32")
        for t in (flags, list_size):
            if t is not None and (t.numel() < B or t.element_size() != 4 or not t.is_contiguous()):
                raise ValueError("flags / list_size must be contiguous 32-bit tensors of at least B elements")
        if pm is not None and (pm.numel() < B or pm.dtype != torch.float64 or not pm.is_contiguous()):
            raise ValueError("pm must be a contiguous float64 tensor of at least B elements")
        self._check(self._lib.polar_cascl_decode_device(
            self._h, C.c_void_p(d_in.data_ptr()), f32, float(sigma), B, C.c_void_p(out_bits.data_ptr()),
            C.c_void_p(pm.data_ptr()) if pm is not None else None,
            C.c_void_p(flags.data_ptr()) if flags is not None else None,
            C.c_void_p(list_size.data_ptr()) if list_size is not None else None), "polar_cascl_decode_device")
        return out_bits

    def decode_cascl_batch(self, llr):
        """polar_cascl_decode_batch: llr [B][N] -> (u_hat [B][N] int32, pm [B] float64, flags [B] uint32,
        list size [B] uint32)."""
        llr = self._rows(llr)
        B = llr.shape[0]
        uh = np.empty((B, self.N), dtype=np.int32)
        pm = np.zeros(B, dtype=np.float64)
        fl = np.zeros(B, dtype=np.uint32)
        ls = np.zeros(B, dtype=np.uint32)
        self._check(self._lib.polar_cascl_decode_batch(self._h, _ptr(llr, C.c_double), B, _ptr(uh, C.c_int),
                                                       _ptr(pm, C.c_double), _ptr(fl, C.c_uint), _ptr(ls, C.c_uint)),
                    "polar_cascl_decode_batch")
        return uh, pm, fl, ls

    def decode_scf_device(self, d_in, sigma=0.0, out_bits=None, flags=None, attempts=None):
        """polar_scf_decode_device: like decode_device, plus per frame the attempt that decided it (`attempts`, int32 [B]:
        0 = plain SC, T when none passed); flags and attempts are optional tensors.  Returns out_bits."""
        import torch
        B = self._dev_rows(d_in)
        if out_bits is None:
            out_bits = torch.empty((B, self.NW), dtype=torch.int32, device=d_in.device)
        f32 = 1 if d_in.dtype == torch.float32 else 0
        if not f32 and d_in.dtype != torch.float64:
            raise ValueError("input must be float64 or float32")
        for t in (flags, attempts):
            if t is not None and (t.numel() < B or t.element_size() != 4 or not t.is_contiguous()):
                raise ValueError("flags / attempts must be contiguous 32-bit tensors of at least B elements")
        self._check(self._lib.polar_scf_decode_device(
            self._h, C.c_void_p(d_in.data_ptr()), f32, float(sigma), B, C.c_void_p(out_bits.data_ptr()),
            C.c_void_p(flags.data_ptr()) if flags is not None else None,
            C.c_void_p(attempts.data_ptr()) if attempts is not None else None), "polar_scf_decode_device")
        return out_bits

    def decode_scf_batch(self, llr):
        """polar_scf_decode_batch: llr [B][N] -> (u_hat [B][N] int32, flags [B] uint32, attempts [B] uint32)."""
        llr = self._rows(llr)
        B = llr.shape[0]
        uh = np.empty((B, self.N), dtype=np.int32)
        fl = np.zeros(B, dtype=np.uint32)
        at = np.zeros(B, dtype=np.uint32)
        self._check(self._lib.polar_scf_decode_batch(self._h, _ptr(llr, C.c_double), B, _ptr(uh, C.c_int),
                                                     _ptr(fl, C.c_uint), _ptr(at, C.c_uint)), "polar_scf_decode_batch")
        return uh, fl, at

    def decode_scf_sets_device(self, d_in, sigma=0.0, out_bits=None, flags=None, attempts=None, sets=None):
        """polar_scf_decode_sets_device: decode_scf_device plus `sets` (optional int32 tensor [B][3]): the positions the
        reported attempt inverted, ascending, -1 padded.  Returns out_bits."""
        import torch
        B = self._dev_rows(d_in)
        if out_bits is None:
            out_bits = torch.empty((B, self.NW), dtype=torch.int32, device=d_in.device)
        f32 = 1 if d_in.dtype == torch.float32 else 0
        if not f32 and d_in.dtype != torch.float64:
            raise ValueError("input must be float64 or float32")
        for t, m in ((flags, 1), (attempts, 1), (sets, 3)):
            if t is not None and (t.numel() < m * B or t.element_size() != 4 or not t.is_contiguous()):
                raise ValueError("flags / attempts / sets must be contiguous 32-bit tensors of at least B (sets: 3 B) elements")
        self._check(self._lib.polar_scf_decode_sets_device(
            self._h, C.c_void_p(d_in.data_ptr()), f32, float(sigma), B, C.c_void_p(out_bits.data_ptr()),
            C.c_void_p(flags.data_ptr()) if flags is not None else None,
            C.c_void_p(attempts.data_ptr()) if attempts is not None else None,
            C.c_void_p(sets.data_ptr()) if sets is not None else None), "polar_scf_decode_sets_device")
        return out_bits

    def decode_scf_sets_batch(self, llr):
        """polar_scf_decode_sets_batch: llr [B][N] -> (u_hat [B][N] int32, flags [B] uint32, attempts [B] uint32,
        sets [B][3] int32)."""
        llr = self._rows(llr)
        B = llr.shape[0]
        uh = np.empty((B, self.N), dtype=np.int32)
        fl = np.zeros(B, dtype=np.uint32)
        at = np.zeros(B, dtype=np.uint32)
        st = np.full((B, 3), -1, dtype=np.int32)
        self._check(self._lib.polar_scf_decode_sets_batch(self._h, _ptr(llr, C.c_double), B, _ptr(uh, C.c_int),
                                                          _ptr(fl, C.c_uint), _ptr(at, C.c_uint), _ptr(st, C.c_int)),
                    "polar_scf_decode_sets_batch")
        return uh, fl, at, st

    def decode_bpl_device(self, d_in, sigma=0.0, out_bits=None, iters=None, flags=None, graph=None, total_iters=None):
        """polar_bpl_decode_device: like decode_device, plus per frame (optional int32 tensors [B]) the round trips of the
        reported attempt (`iters`), FLAG_BP_CONVERGED / FLAG_CRC_PASS (`flags`), the graph that decided the frame (`graph`, P
        when none did) and the round trips of every attempt run for it (`total_iters`).  Returns out_bits."""
        import torch
        B = self._dev_rows(d_in)
        if out_bits is None:
            out_bits = torch.empty((B, self.NW), dtype=torch.int32, device=d_in.device)
        f32 = 1 if d_in.dtype == torch.float32 else 0
        if not f32 and d_in.dtype != torch.float64:
            raise ValueError("input must be float64 or float32")
        for t in (iters, flags, graph, total_iters):
            if t is not None and (t.numel() < B or t.element_size() != 4 or not t.is_contiguous()):
                raise ValueError("iters / flags / graph / total_iters must be contiguous 32-bit tensors of at least B elements")
        opt = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (iters, flags, graph, total_iters)]
        self._check(self._lib.polar_bpl_decode_device(
            self._h, C.c_void_p(d_in.data_ptr()), f32, float(sigma), B, C.c_void_p(out_bits.data_ptr()), *opt),
            "polar_bpl_decode_device")
        return out_bits

    def decode_bpl_batch(self, llr):
        """polar_bpl_decode_batch: llr [B][N] -> (u_hat [B][N] int32, iters, flags, graph, total_iters: [B] uint32 each)."""
        llr = self._rows(llr)
        B = llr.shape[0]
        uh = np.empty((B, self.N), dtype=np.int32)
        it, fl, gr, tot = (np.zeros(B, dtype=np.uint32) for _ in range(4))
        self._check(self._lib.polar_bpl_decode_batch(self._h, _ptr(llr, C.c_double), B, _ptr(uh, C.c_int), _ptr(it, C.c_uint),
                                                     _ptr(fl, C.c_uint), _ptr(gr, C.c_uint), _ptr(tot, C.c_uint)),
                    "polar_bpl_decode_batch")
        return uh, it, fl, gr, tot

    def decode_scan_device(self, d_in, sigma=0.0, out_bits=None, llr_u=None, ext_x=None):
        """polar_scan_decode_device: soft-output SCAN.  llr_u and ext_x are optional tensors [B][N] of the decoder's dtype
        (float64 or float32) on d_in's device: the LLR of every u bit (+inf at frozen positions) and the extrinsic LLR of
        every code bit.  out_bits=False skips the hard decisions; None allocates them.  Returns out_bits (or None)."""
        import torch
        B = self._dev_rows(d_in)
        if out_bits is None:
            out_bits = torch.empty((B, self.NW), dtype=torch.int32, device=d_in.device)
        elif out_bits is False:
            out_bits = None
        f32 = 1 if d_in.dtype == torch.float32 else 0
        if not f32 and d_in.dtype != torch.float64:
            raise ValueError("input must be float64 or float32")
        want = torch.float32 if self.dtype == F32 else torch.float64
        for t in (llr_u, ext_x):
            if t is not None and (t.numel() < B * self.N or t.dtype != want or not t.is_contiguous()):
                raise ValueError(f"llr_u / ext_x must be contiguous {want} tensors of at least B*N elements")
        self._check(self._lib.polar_scan_decode_device(
            self._h, C.c_void_p(d_in.data_ptr()), f32, float(sigma), B,
            C.c_void_p(out_bits.data_ptr()) if out_bits is not None else None,
            C.c_void_p(llr_u.data_ptr()) if llr_u is not None else None,
            C.c_void_p(ext_x.data_ptr()) if ext_x is not None else None), "polar_scan_decode_device")
        return out_bits

    def decode_scan_batch(self, llr):
        """polar_scan_decode_batch: llr [B][N] -> (u_hat [B][N] int32, llr_u [B][N], ext_x [B][N]), the soft outputs in the
        decoder's dtype."""
        llr = self._rows(llr)
        B = llr.shape[0]
        uh = np.empty((B, self.N), dtype=np.int32)
        soft = np.float32 if self.dtype == F32 else np.float64
        lu = np.empty((B, self.N), dtype=soft)
        ex = np.empty((B, self.N), dtype=soft)
        self._check(self._lib.polar_scan_decode_batch(self._h, _ptr(llr, C.c_double), B, _ptr(uh, C.c_int),
                                                      C.c_void_p(lu.ctypes.data), C.c_void_p(ex.ctypes.data)),
                    "polar_scan_decode_batch")
        return uh, lu, ex

    def decode_bp_batch(self, llr):
        """polar_bp_decode_batch: llr [B][N] -> (u_hat [B][N] int32, iters [B] uint32, flags [B] uint32)."""
        llr = self._rows(llr)
        B = llr.shape[0]
        uh = np.empty((B, self.N), dtype=np.int32)
        it = np.zeros(B, dtype=np.uint32)
        fl = np.zeros(B, dtype=np.uint32)
        self._check(self._lib.polar_bp_decode_batch(self._h, _ptr(llr, C.c_double), B, _ptr(uh, C.c_int),
                                                    _ptr(it, C.c_uint), _ptr(fl, C.c_uint)), "polar_bp_decode_batch")
        return uh, it, fl

    # ---- list output (include/polar_hip.h, "List output") -------------------------------------------------
    def decode_list_device(self, d_in, sigma=0.0, want_paths=True, want_pm=True, want_rem=True, want_count=True,
                           want_flags=True):
        """polar_list_decode: d_in as decode_device -> (paths [B][L][N/32] int32, pm [B][L] float64, rem [B][L] int32,
        count [B] int32, flags [B] int32), rank k of a frame = its k-th live path in ascending (PM, slot); an output not
        asked for is None and is not computed (at least one must be asked for)."""
        import torch
        B = self._dev_rows(d_in)
        f32 = 1 if d_in.dtype == torch.float32 else 0
        if not f32 and d_in.dtype != torch.float64:
            raise ValueError("input must be float64 or float32")
        dev, i32 = d_in.device, torch.int32
        paths = torch.empty((B, self.L, self.NW), dtype=i32, device=dev) if want_paths else None
        pm = torch.empty((B, self.L), dtype=torch.float64, device=dev) if want_pm else None
        rem = torch.empty((B, self.L), dtype=i32, device=dev) if want_rem else None
        count = torch.empty(B, dtype=i32, device=dev) if want_count else None
        flags = torch.empty(B, dtype=i32, device=dev) if want_flags else None
        self._check(self._lib.polar_list_decode(
            self._h, C.c_void_p(d_in.data_ptr()), f32, float(sigma), B,
            *[C.c_void_p(t.data_ptr()) if t is not None else None for t in (paths, pm, rem, count, flags)]),
            "polar_list_decode")
        return paths, pm, rem, count, flags

    def decode_list_batch(self, llr):
        """polar_list_decode_host: host rows -> (paths [B][L][N] int32 0/1, pm [B][L], rem [B][L] uint32, count [B] uint32,
        flags [B] uint32)."""
        llr = self._rows(llr)
        B = llr.shape[0]
        paths = np.empty((B, self.L, self.N), dtype=np.int32)
        pm = np.empty((B, self.L), dtype=np.float64)
        rem = np.empty((B, self.L), dtype=np.uint32)
        count = np.empty(B, dtype=np.uint32)
        flags = np.empty(B, dtype=np.uint32)
        self._check(self._lib.polar_list_decode_host(self._h, _ptr(llr, C.c_double), B, _ptr(paths, C.c_int),
                                                      _ptr(pm, C.c_double), _ptr(rem, C.c_uint), _ptr(count, C.c_uint),
                                                      _ptr(flags, C.c_uint)), "polar_list_decode_host")
        return paths, pm, rem, count, flags

    @staticmethod
    def _list_t(t, shape, dtype, what):
        if not (t.is_cuda and t.is_contiguous()) or t.dtype != dtype or tuple(t.shape[1:]) != tuple(shape):
            raise ValueError(f"{what} must be a contiguous CUDA {dtype} tensor of shape [B]{list(shape)}")
        return t.shape[0]

    def list_select_device(self, rem, count, masks):
        """polar_list_select: rem [B][L], count [B], masks [M] (int32 CUDA tensors, 1 <= M <= 64) -> idx [B][M] int32:
        the least-metric rank whose remainder equals the mask, -1 if the list has none."""
        import torch
        B = self._list_t(rem, (self.L,), torch.int32, "rem")
        if self._list_t(count, (), torch.int32, "count") != B:
            raise ValueError("count must have one entry per frame")
        if not (masks.is_cuda and masks.is_contiguous()) or masks.dtype != torch.int32 or masks.dim() != 1:
            raise ValueError("masks must be a contiguous CUDA int32 tensor of shape [M]")
        M = masks.shape[0]
        idx = torch.empty((B, M), dtype=torch.int32, device=rem.device)
        self._check(self._lib.polar_list_select(self._h, C.c_void_p(rem.data_ptr()), C.c_void_p(count.data_ptr()), B,
                                                       C.c_void_p(masks.data_ptr()), M, C.c_void_p(idx.data_ptr())),
                    "polar_list_select")
        return idx

    def list_gather_device(self, paths, idx):
        """polar_list_gather: paths [B][L][N/32], idx [B] or a column idx[:, m] of list_select_device's result (int32;
        -1 takes rank 0) -> bits [B][N/32] int32."""
        import torch
        B = self._list_t(paths, (self.L, self.NW), torch.int32, "paths")
        if not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 1 or idx.shape[0] != B or (B > 1 and idx.stride(0) < 1):
            raise ValueError("idx must be a CUDA int32 tensor of shape [B] (a column of a [B][M] tensor will do)")
        stride = idx.stride(0) if B > 1 else 1
        out = torch.empty((B, self.NW), dtype=torch.int32, device=paths.device)
        self._check(self._lib.polar_list_gather(self._h, C.c_void_p(paths.data_ptr()), C.c_void_p(idx.data_ptr()),
                                                       stride, B, C.c_void_p(out.data_ptr())), "polar_list_gather")
        return out

    def list_soft_device(self, paths, pm, count, rem=None, want_rem=0, domain=0, clamp=64.0):
        """polar_list_soft: max-log LLRs over the list -> [B][N] float64, positive = bit 0; domain 0: u, 1: x.  rem
        given: only the ranks with remainder want_rem count, unless there is none."""
        import torch
        B = self._list_t(paths, (self.L, self.NW), torch.int32, "paths")
        if self._list_t(pm, (self.L,), torch.float64, "pm") != B or self._list_t(count, (), torch.int32, "count") != B:
            raise ValueError("pm and count must have one row per frame")
        if rem is not None and self._list_t(rem, (self.L,), torch.int32, "rem") != B:
            raise ValueError("rem must have one row per frame")
        out = torch.empty((B, self.N), dtype=torch.float64, device=paths.device)
        self._check(self._lib.polar_list_soft(
            self._h, C.c_void_p(paths.data_ptr()), C.c_void_p(pm.data_ptr()), C.c_void_p(count.data_ptr()),
            C.c_void_p(rem.data_ptr()) if rem is not None else None, int(want_rem) & 0xFFFFFFFF, int(domain), float(clamp), B,
            C.c_void_p(out.data_ptr())), "polar_list_soft")
        return out

    # ---- encoder side ---------------------------------------------------------------------------------
    @staticmethod
    def _words(t, width, what):
        import torch
        if not (t.is_cuda and t.is_contiguous()) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != width:
            raise ValueError(f"{what} must be a contiguous CUDA int32 tensor of shape [B][{width}]")
        return t.shape[0]

    def transform_device(self, bits, out=None):
        """polar_transform_device: rows [B][N/32] int32 -> their transform by F^{(x)n} (out may be `bits`)."""
        import torch
        B = self._words(bits, self.NW, "bits")
        if out is None:
            out = torch.empty_like(bits)
        self._words(out, self.NW, "out")
        self._check(self._lib.polar_transform_device(self._h, C.c_void_p(bits.data_ptr()), B, C.c_void_p(out.data_ptr())),
                    "polar_transform_device")
        return out

    def encode_device(self, payload, want_u=True, want_x=True):
        """polar_encode_device: payload [B][ceil(K/32)] int32 (bit k of the row = payload bit k) -> (u_bits [B][N/32],
        x_bits [B][N/32], or [B][ceil(E/32)] on a rate-matched decoder); an output not asked for is None."""
        import torch
        B = self._words(payload, (self.K + 31) // 32, "payload")
        u = torch.empty((B, self.NW), dtype=torch.int32, device=payload.device) if want_u else None
        x = torch.empty((B, (self.E + 31) // 32), dtype=torch.int32, device=payload.device) if want_x else None
        self._check(self._lib.polar_encode_device(self._h, C.c_void_p(payload.data_ptr()), B,
                                                  C.c_void_p(u.data_ptr()) if want_u else None,
                                                  C.c_void_p(x.data_ptr()) if want_x else None), "polar_encode_device")
        return u, x

    def payload_device(self, uhat_bits):
        """polar_payload_device: decisions [B][N/32] -> (payload [B][ceil(K/32)] int32, crc_ok [B] int32)."""
        import torch
        B = self._words(uhat_bits, self.NW, "uhat_bits")
        pay = torch.empty((B, (self.K + 31) // 32), dtype=torch.int32, device=uhat_bits.device)
        ok = torch.empty(B, dtype=torch.int32, device=uhat_bits.device)
        self._check(self._lib.polar_payload_device(self._h, C.c_void_p(uhat_bits.data_ptr()), B, C.c_void_p(pay.data_ptr()),
                                                   C.c_void_p(ok.data_ptr())), "polar_payload_device")
        return pay, ok

    def encode_batch(self, payload):
        """polar_encode_batch: payload [B][K] of 0/1 -> (u [B][N], x [B][N] or [B][E]) int32."""
        p = np.ascontiguousarray(payload, dtype=np.int32)
        if p.ndim != 2 or p.shape[1] != self.K:
            raise ValueError(f"payload must have shape [B][{self.K}]")
        B = p.shape[0]
        u = np.empty((B, self.N), dtype=np.int32)
        x = np.empty((B, self.E), dtype=np.int32)
        self._check(self._lib.polar_encode_batch(self._h, _ptr(p, C.c_int), B, _ptr(u, C.c_int), _ptr(x, C.c_int)),
                    "polar_encode_batch")
        return u, x

    def payload_batch(self, u_hat):
        """polar_payload_batch: decisions [B][N] of 0/1 -> (payload [B][K] int32, crc_ok [B] uint32)."""
        uh = np.ascontiguousarray(u_hat, dtype=np.int32)
        if uh.ndim != 2 or uh.shape[1] != self.N:
            raise ValueError(f"u_hat must have shape [B][{self.N}]")
        B = uh.shape[0]
        pay = np.empty((B, self.K), dtype=np.int32)
        ok = np.empty(B, dtype=np.uint32)
        self._check(self._lib.polar_payload_batch(self._h, _ptr(uh, C.c_int), B, _ptr(pay, C.c_int), _ptr(ok, C.c_uint)),
                    "polar_payload_batch")
        return pay, ok

    def generate_device(self, seed, first_frame, snr_db, out, u_bits=None, out_is_y=False):
        """Device-side transmit chain (throughput mode): fills `out` [B][N] ([B][E] on a rate-matched decoder; float64/float32
        LLRs, or y) and `u_bits` [B][N/32] int32 for frames first_frame .. first_frame + B - 1 of stream `seed`."""
        import torch
        B = self._dev_rows(out) if self.rm_mode != RM_NONE else out.numel() // self.N
        self._check(self._lib.polar_generate_device(
            self._h, int(seed), int(first_frame), float(snr_db), B, C.c_void_p(out.data_ptr()),
            1 if out.dtype == torch.float32 else 0, 1 if out_is_y else 0,
            C.c_void_p(u_bits.data_ptr()) if u_bits is not None else None), "polar_generate_device")
        return out

    def fer_batch(self, seed, first_frame, snr_db, B):
        """generate -> decode -> count for B frames on the device; returns (block_errors, bit_errors)."""
        blk, bits = C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.polar_fer_batch(self._h, int(seed), int(first_frame), float(snr_db), int(B),
                                              C.byref(blk), C.byref(bits)), "polar_fer_batch")
        return blk.value, bits.value

    def fer_multi_gpu(self, ngpus, seed, first_frame, snr_db, frames_per_gpu):
        """polar_fer_batch over the GPUs of this node (one shard of frames_per_gpu frames each, own context and host thread
        per GPU, RCCL all-reduce of the two counters): returns (block_errors, bit_errors, seconds of the slowest GPU)."""
        blk, bits, sec = C.c_ulonglong(0), C.c_ulonglong(0), C.c_double(0)
        self._check(self._lib.polar_fer_multi_gpu(C.byref(self._cfg), int(ngpus), int(seed), int(first_frame), float(snr_db),
                                                  int(frames_per_gpu), C.byref(blk), C.byref(bits), C.byref(sec)),
                    "polar_fer_multi_gpu")
        return blk.value, bits.value, sec.value

    def count_errors_device(self, uhat_bits, u_bits, counters, frame_err=None):
        B = uhat_bits.shape[0]
        self._check(self._lib.polar_count_errors_device(
            self._h, C.c_void_p(uhat_bits.data_ptr()), C.c_void_p(u_bits.data_ptr()), B,
            C.c_void_p(counters.data_ptr()),
            C.c_void_p(frame_err.data_ptr()) if frame_err is not None else None), "polar_count_errors_device")

    def stop_rule_cut_device(self, frame_err, need, out, min_frames=0):
        """The reference's sequential stop rule (SCL_1024.c:228) on the per-frame error counts of a batch: out (int64
        CUDA tensor [3]) <- frames consumed, block errors, bit errors among them.  Asynchronous on the ctx stream."""
        self._check(self._lib.polar_stop_rule_cut_device(self._h, C.c_void_p(frame_err.data_ptr()), frame_err.numel(),
                                                         int(need), int(min_frames), C.c_void_p(out.data_ptr())),
                    "polar_stop_rule_cut_device")

    def stop_rule_batch_y(self, y, sigma, u, need, min_frames=0):
        """One batch of main()'s loop on host buffers: y [B][N] observations, u [B][N] sent bits (0/1).  Returns
        (frames consumed, block errors, bit errors) under the stop rule with `need` block errors still missing."""
        y = self._rows(y)
        ub = np.packbits(np.ascontiguousarray(u, dtype=np.uint8).reshape(-1, self.N), axis=1, bitorder="little")
        ub = np.ascontiguousarray(ub).view(np.uint32)
        used, blk, bits = C.c_size_t(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.polar_stop_rule_batch_y(self._h, _ptr(y, C.c_double), float(sigma), ub.ctypes.data, y.shape[0],
                                                      int(need), int(min_frames), C.byref(used), C.byref(blk), C.byref(bits)),
                    "polar_stop_rule_batch_y")
        return used.value, blk.value, bits.value

    def bp_readout_device(self, d_in, u_bits, checkpoints, E, out_bits=None, sigma=0.0):
        """BPr_128.c: BP with per-stage read-outs.  d_in [B][N] LLR (or y with sigma), u_bits [B][N/32] int32 sent
        bits, E int64 [len(checkpoints)][n+1] accumulated on the device, out_bits optional [B][N/32]."""
        import torch
        B = d_in.numel() // self.N
        cp = (C.c_int * len(checkpoints))(*[int(x) for x in checkpoints])
        self._check(self._lib.polar_bp_readout_device(
            self._h, C.c_void_p(d_in.data_ptr()), 1 if d_in.dtype == torch.float32 else 0, float(sigma), B,
            C.c_void_p(u_bits.data_ptr()), cp, len(checkpoints), C.c_void_p(E.data_ptr()),
            C.c_void_p(out_bits.data_ptr()) if out_bits is not None else None), "polar_bp_readout_device")

    def time_decode_device(self, d_in, out_bits, reps, sigma=0.0):
        import torch
        B = d_in.numel() // self._w
        ms = C.c_float()
        self._check(self._lib.polar_time_decode_device(
            self._h, C.c_void_p(d_in.data_ptr()), 1 if d_in.dtype == torch.float32 else 0, float(sigma), B,
            C.c_void_p(out_bits.data_ptr()), int(reps), C.byref(ms)), "polar_time_decode_device")
        return ms.value

    def rm_recover_device(self, d_in, sigma=0.0, out=None):
        """polar_rm_recover_device (rate-matched decoders): d_in [B][E] float64/float32 LLRs (or y with sigma > 0) -> the
        [B][N] rows of the same dtype that the decoder reads (include/polar_hip.h rule 6).  Asynchronous on the ctx stream."""
        import torch
        if self.rm_mode == RM_NONE:
            raise PolarError("rm_recover_device: not a rate-matched decoder (pass E=...)")
        B = self._dev_rows(d_in)
        if d_in.dtype not in (torch.float64, torch.float32):
            raise ValueError("input must be float64 or float32")
        if out is None:
            out = torch.empty((B, self.N), dtype=d_in.dtype, device=d_in.device)
        if out.dtype != d_in.dtype or not out.is_contiguous() or out.numel() < B * self.N:
            raise ValueError("out must be a contiguous tensor of the input's dtype with B * N elements")
        self._check(self._lib.polar_rm_recover_device(self._h, C.c_void_p(d_in.data_ptr()), 1 if d_in.dtype == torch.float32 else 0,
                                                      float(sigma), B, C.c_void_p(out.data_ptr())), "polar_rm_recover_device")
        return out

    # ---- sent-path trace (include/polar_hip.h, "Sent-path trace") ---------------------------------------------------
    def trace_list_device(self, d_in, u_bits, sigma=0.0, want_loss_leaf=True, want_loss_rank=True, want_rank=True,
                          want_chosen=True, want_flags=True):
        """polar_list_trace: d_in as decode_device, u_bits [B][N/32] int32 (the sent u, packed like decode_device's output)
        -> (loss_leaf, loss_rank, rank, chosen, flags), int32 CUDA tensors [B]: the leaf where the sent path left the list (N:
        it never did), the sent candidate's count among the 2L candidates there, its rank in the final list (-1: not there),
        the rank of the path the ordinary decode returns, and that decode's flags.  An output not asked for is None and is not
        computed (at least one must be asked for)."""
        import torch
        B = self._dev_rows(d_in)
        f32 = 1 if d_in.dtype == torch.float32 else 0
        if not f32 and d_in.dtype != torch.float64:
            raise ValueError("input must be float64 or float32")
        if self._list_t(u_bits, (self.NW,), torch.int32, "u_bits") != B:
            raise ValueError("u_bits and the rows disagree on B")
        outs = [torch.empty(B, dtype=torch.int32, device=d_in.device) if w else None
                for w in (want_loss_leaf, want_loss_rank, want_rank, want_chosen, want_flags)]
        self._check(self._lib.polar_list_trace(
            self._h, C.c_void_p(d_in.data_ptr()), f32, float(sigma), C.c_void_p(u_bits.data_ptr()), B,
            *[C.c_void_p(t.data_ptr()) if t is not None else None for t in outs]), "polar_list_trace")
        return tuple(outs)

    def trace_count_device(self, loss_leaf, rank, chosen, hist):
        """polar_list_trace_count: loss_leaf, rank, chosen [B] as trace_list_device returned them; adds per leaf the frames
        lost there (hist[:N]), the frames of class 0 (correct), 1 (selection error), 2 (list loss) (hist[N:N+3]) and B
        (hist[N+3]).  hist: int64 CUDA tensor [N + 4] holding the library's uint64 counters.  Asynchronous on the ctx stream."""
        import torch
        B = self._list_t(loss_leaf, (), torch.int32, "loss_leaf")
        if self._list_t(rank, (), torch.int32, "rank") != B or self._list_t(chosen, (), torch.int32, "chosen") != B:
            raise ValueError("loss_leaf, rank and chosen disagree on B")
        if not (hist.is_cuda and hist.is_contiguous() and hist.dtype == torch.int64 and hist.numel() == self.N + 4):
            raise ValueError("hist must be a contiguous int64 CUDA tensor of N + 4 elements")
        self._check(self._lib.polar_list_trace_count(self._h, C.c_void_p(loss_leaf.data_ptr()), C.c_void_p(rank.data_ptr()),
                                                     C.c_void_p(chosen.data_ptr()), B, C.c_void_p(hist.data_ptr())),
                    "polar_list_trace_count")
        return hist

    def trace_list_batch(self, llr, u):
        """polar_list_trace_host: host rows and the sent u [B][N] of 0/1 -> (loss_leaf int32, loss_rank uint32, rank int32,
        chosen int32, flags uint32), each [B]."""
        llr = self._rows(llr)
        B = llr.shape[0]
        u = np.ascontiguousarray(u, dtype=np.int32)
        if u.shape != (B, self.N):
            raise ValueError(f"u must have shape [{B}][{self.N}]")
        loss_leaf = np.empty(B, dtype=np.int32)
        loss_rank = np.empty(B, dtype=np.uint32)
        rank = np.empty(B, dtype=np.int32)
        chosen = np.empty(B, dtype=np.int32)
        flags = np.empty(B, dtype=np.uint32)
        self._check(self._lib.polar_list_trace_host(self._h, _ptr(llr, C.c_double), _ptr(u, C.c_int), B, _ptr(loss_leaf, C.c_int),
                                                    _ptr(loss_rank, C.c_uint), _ptr(rank, C.c_int), _ptr(chosen, C.c_int),
                                                    _ptr(flags, C.c_uint)), "polar_list_trace_host")
        return loss_leaf, loss_rank, rank, chosen, flags

    # ---- Monte-Carlo construction (include/polar_hip.h: genie-aided SC, rules 1-3) -----------------------------------
    @staticmethod
    def _counts(counts, N):
        import torch
        if not (counts.is_cuda and counts.is_contiguous() and counts.dtype == torch.int64 and counts.numel() == 2 * N):
            raise ValueError("counts must be a contiguous int64 CUDA tensor of shape [2][N] (err row, tie row)")
        return C.c_void_p(counts.data_ptr())

    def genie_count_device(self, d_in, counts, sigma=0.0):
        """polar_genie_count_device: d_in [B][N] float64/float32 LLRs (or y with sigma > 0); adds per leaf the frames whose
        genie-aided SC leaf LLR is negative (counts[0]) or zero (counts[1]).  counts: int64 CUDA tensor [2][N] holding the
        library's uint64 counters.  Asynchronous on the ctx stream."""
        import torch
        if d_in.dtype not in (torch.float64, torch.float32):
            raise ValueError("input must be float64 or float32")
        if not (d_in.is_cuda and d_in.is_contiguous()) or d_in.dim() == 0 or d_in.shape[-1] != self.N:
            raise ValueError(f"device rows must be a contiguous CUDA tensor of shape [B][{self.N}]")
        B = d_in.numel() // self.N
        self._check(self._lib.polar_genie_count_device(self._h, C.c_void_p(d_in.data_ptr()), 1 if d_in.dtype == torch.float32 else 0,
                                                       float(sigma), B, self._counts(counts, self.N)), "polar_genie_count_device")
        return counts

    def genie_rows_device(self, seed, first_frame, sigma, out):
        """polar_genie_rows_device: fills out [B][N] (float64 or float32 CUDA tensor) with the design rows of frames
        first_frame .. first_frame + B - 1: the all-zero codeword over BPSK + AWGN of standard deviation sigma, as LLRs."""
        import torch
        if out.dtype not in (torch.float64, torch.float32):
            raise ValueError("out must be float64 or float32")
        if not (out.is_cuda and out.is_contiguous()) or out.dim() == 0 or out.shape[-1] != self.N:
            raise ValueError(f"out must be a contiguous CUDA tensor of shape [B][{self.N}]")
        self._check(self._lib.polar_genie_rows_device(self._h, int(seed), int(first_frame), float(sigma), out.numel() // self.N,
                                                      C.c_void_p(out.data_ptr()), 1 if out.dtype == torch.float32 else 0),
                    "polar_genie_rows_device")
        return out

    def construct_batch(self, seed, first_frame, sigma, B, counts):
        """polar_construct_batch: design rows of B frames (ctx dtype, ctx scratch) -> genie-aided SC -> counts (as
        genie_count_device).  Exactly genie_rows_device followed by genie_count_device on the same frames."""
        self._check(self._lib.polar_construct_batch(self._h, int(seed), int(first_frame), float(sigma), int(B),
                                                    self._counts(counts, self.N)), "polar_construct_batch")
        return counts

    def synchronize(self):
        self._check(self._lib.polar_synchronize(self._h), "polar_synchronize")


class Group:
    """polar_group: one context per GPU of this node (devices 0 .. ngpus-1) for the configuration of `dec`, plus the RCCL
    communicators; frames are sharded contiguously, RCCL carries only the final counters (or, for the exact stop rule,
    the per-frame error counts)."""

    def __init__(self, dec, ngpus):
        self._lib, self._dec = dec._lib, dec
        self._h = C.c_void_p()
        rc = self._lib.polar_group_create(C.byref(dec._cfg), int(ngpus), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise PolarError(f"polar_group_create: {self._lib.polar_strerror(rc).decode()} (rc={rc})")

    @property
    def size(self):
        return self._lib.polar_group_size(self._h)

    def fer_batch(self, seed, first_frame, snr_db, frames_per_gpu):
        blk, bits, sec = C.c_ulonglong(0), C.c_ulonglong(0), C.c_double(0)
        rc = self._lib.polar_group_fer_batch(self._h, int(seed), int(first_frame), float(snr_db), int(frames_per_gpu),
                                             C.byref(blk), C.byref(bits), C.byref(sec))
        if rc != 0:
            raise PolarError(f"polar_group_fer_batch: {self._lib.polar_strerror(rc).decode()} (rc={rc})")
        return blk.value, bits.value, sec.value

    def stop_rule_batch(self, seed, first_frame, snr_db, frames_per_gpu, need, min_frames=0):
        """(frames consumed, block errors, bit errors) of the reference's stop rule over the sharded batch."""
        used, blk, bits = C.c_size_t(0), C.c_ulonglong(0), C.c_ulonglong(0)
        rc = self._lib.polar_group_stop_rule_batch(self._h, int(seed), int(first_frame), float(snr_db), int(frames_per_gpu),
                                                   int(need), int(min_frames), C.byref(used), C.byref(blk), C.byref(bits))
        if rc != 0:
            raise PolarError(f"polar_group_stop_rule_batch: {self._lib.polar_strerror(rc).decode()} (rc={rc})")
        return used.value, blk.value, bits.value

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.polar_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Codebook:
    """polar_codebook: C decoders' codes behind one launch (include/polar_hip.h, "Code books").  Every frame of a call names
    its code by an index into `decoders`; its bits, metric and flags are what that decoder's own decode_device returns.  The
    codes are copied at construction: the decoders may be closed afterwards."""

    def __init__(self, decoders):
        decoders = list(decoders)
        if not decoders:
            raise ValueError("a code book needs at least one decoder")
        self._lib = decoders[0]._lib
        self._h = C.c_void_p()
        arr = (C.c_void_p * len(decoders))(*[d._h.value for d in decoders])
        rc = self._lib.polar_codebook_create(arr, len(decoders), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise PolarError(f"polar_codebook_create: {self._lib.polar_strerror(rc).decode()} (rc={rc})")
        c, n, w, l, dt = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._lib.polar_codebook_info(self._h, C.byref(c), C.byref(n), C.byref(w), C.byref(l), C.byref(dt))
        self.C, self.N_max, self.W_max, self.L, self.dtype = c.value, n.value, w.value, l.value, dt.value
        self.NW = self.N_max // 32
        self.device = decoders[0].device
        self.members = []
        for i in range(self.C):
            self._lib.polar_codebook_member(self._h, i, C.byref(n), C.byref(w), C.byref(c))
            self.members.append((n.value, w.value, c.value))

    @property
    def kernel_name(self):
        return self._lib.polar_codebook_kernel_name(self._h).decode()

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.polar_codebook_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.polar_strerror(rc).decode()
            det = self._lib.polar_codebook_last_error(self._h).decode()
            raise PolarError(f"{what}: {msg} {det} (rc={rc})")

    def use_torch_stream(self):
        """Run on torch's current stream so that torch ops and decodes are ordered."""
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.polar_codebook_set_stream(self._h, C.c_void_p(s)), "polar_codebook_set_stream")

    def synchronize(self):
        self._check(self._lib.polar_codebook_synchronize(self._h), "polar_codebook_synchronize")

    def _dev_args(self, d_in, code):
        """(B, ld, in_is_f32) of rows d_in [B][>= W_max] (unit stride inside a row, any row stride) and code [B] int32"""
        import torch
        if not d_in.is_cuda or d_in.dim() != 2 or d_in.shape[1] < self.W_max or (d_in.shape[1] > 1 and d_in.stride(1) != 1):
            raise ValueError(f"device rows must be a CUDA tensor of shape [B][>= {self.W_max}] with unit stride inside a row")
        if d_in.dtype not in (torch.float32, torch.float64):
            raise ValueError("input must be float64 or float32")
        B = d_in.shape[0]
        ld = d_in.stride(0) if B > 1 else d_in.shape[1]
        if not (code.is_cuda and code.is_contiguous()) or code.dtype != torch.int32 or tuple(code.shape) != (B,):
            raise ValueError("code must be a contiguous CUDA int32 tensor of shape [B]")
        return B, ld, 1 if d_in.dtype == torch.float32 else 0

    def decode_device(self, d_in, code, sigma=0.0, out_bits=None, pm=None, flags=None):
        """polar_codebook_decode: d_in [B][ld] float64 or float32 (the row stride is read from d_in.stride(0)), code [B] int32
        (the bits of an unsigned index).  Returns out_bits: int32 [B][N_max/32]; pm (float64 [B]) and flags (int32 [B]) are
        optional tensors."""
        import torch
        B, ld, f32 = self._dev_args(d_in, code)
        if out_bits is None:
            out_bits = torch.empty((B, self.NW), dtype=torch.int32, device=d_in.device)
        self._check(self._lib.polar_codebook_decode(
            self._h, C.c_void_p(d_in.data_ptr()), f32, ld, C.c_void_p(code.data_ptr()), float(sigma), B,
            C.c_void_p(out_bits.data_ptr()), C.c_void_p(pm.data_ptr()) if pm is not None else None,
            C.c_void_p(flags.data_ptr()) if flags is not None else None), "polar_codebook_decode")
        return out_bits

    def decode_list_device(self, d_in, code, sigma=0.0, want_paths=True, want_pm=True, want_rem=True, want_count=True,
                           want_flags=True):
        """polar_codebook_list_decode -> (paths [B][L][N_max/32] int32, pm [B][L] float64, rem [B][L] int32, count [B] int32,
        flags [B] int32) as Decoder.decode_list_device; an output not asked for is None and is not computed."""
        import torch
        B, ld, f32 = self._dev_args(d_in, code)
        dev, i32 = d_in.device, torch.int32
        paths = torch.empty((B, self.L, self.NW), dtype=i32, device=dev) if want_paths else None
        pm = torch.empty((B, self.L), dtype=torch.float64, device=dev) if want_pm else None
        rem = torch.empty((B, self.L), dtype=i32, device=dev) if want_rem else None
        count = torch.empty(B, dtype=i32, device=dev) if want_count else None
        flags = torch.empty(B, dtype=i32, device=dev) if want_flags else None
        self._check(self._lib.polar_codebook_list_decode(
            self._h, C.c_void_p(d_in.data_ptr()), f32, ld, C.c_void_p(code.data_ptr()), float(sigma), B,
            *[C.c_void_p(t.data_ptr()) if t is not None else None for t in (paths, pm, rem, count, flags)]),
            "polar_codebook_list_decode")
        return paths, pm, rem, count, flags

    def decode_batch(self, rows, code, sigma=0.0):
        """polar_codebook_decode_host: host rows [B][ld >= W_max] and code [B] -> (u_hat [B][N_max] int32 0/1, pm [B], flags
        [B] uint32)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        code = np.ascontiguousarray(code, dtype=np.uint32)
        if rows.ndim != 2 or rows.shape[1] < self.W_max or code.shape != (rows.shape[0],):
            raise ValueError(f"rows must have shape [B][>= {self.W_max}] and code shape [B]")
        B, ld = rows.shape
        uh = np.empty((B, self.N_max), dtype=np.int32)
        pm = np.zeros(B, dtype=np.float64)
        fl = np.zeros(B, dtype=np.uint32)
        self._check(self._lib.polar_codebook_decode_host(self._h, _ptr(rows, C.c_double), ld, _ptr(code, C.c_uint32), float(sigma), B,
                                                         _ptr(uh, C.c_int), _ptr(pm, C.c_double), _ptr(fl, C.c_uint)),
                    "polar_codebook_decode_host")
        return uh, pm, fl


# ---- mirrors of the reference entry points (same names, same argument meaning) -----------------------

def SCdecode(N, K, **kw):
    """SC_128.c:395 / SC_1024.c:434 -- ``SCdecode(y, u_hat)``."""
    return Decoder(N, K, ALGO_SC, L=1, **kw)


def BP(N, K, iterMax=100, early_stop=None, **kw):
    """BP_1024.c:372 -- ``BP(y, u_hat)``; iterMax is BP_1024.c:16.  early_stop="g": stop a frame at the first round trip
    whose decisions form a codeword (Decoder.set_bp_stop); None: iterMax round trips, as the reference."""
    dec = Decoder(N, K, ALGO_BP, L=1, bp_iters=iterMax, **kw)
    if early_stop is not None:
        dec.set_bp_stop(early_stop)
    return dec


def SCLdecode(N, K, L=8, **kw):
    """SCL_1024.c:547 -- ``SCLdecode(y, u_hat)``; L is SCL_1024.c:16.  L: a power of two up to 32, or a wide list of 64, 128
    or 256 while N * L <= 65536 (include/polar_hip.h, "Wide lists"; not with dtype=Q8)."""
    return Decoder(N, K, ALGO_SCL, L=L, **kw)


def CASCL(N, K, L=8, crc_taps=CRC24C_TAPS, crc_file=None, stages=None, **kw):
    """CASCL_1024_L8.c:601 -- ``CASCL(y, u_hat)``; r and g(D) are CASCL_1024_L8.c:2-4, :19.
    ``systematic=True`` is CASCL_1024_sys.c: same decoder, systematic CRC in the generator, K-bit error metric.
    ``crc_file``: r and g(D) from a generator-matrix file instead (the reference's CRC_6.dat; ``Gc`` of
    CASCL_1024_sys.c:48-561 in the same layout) -- polar_create_crc_file.
    ``stages``: adaptive CA-SCL, e.g. ``CASCL(1024, 512, L=32, stages=(1, 8, 32))`` (Decoder.set_cascl_stages);
    None: every frame decoded with list size L.  L = 64, 128, 256 (N * L <= 65536): a wide list; no ``stages`` then."""
    if crc_file is not None:
        dec = Decoder(N, K, ALGO_CASCL, L=L, crc_taps=None, crc_file=crc_file, **kw)
    else:
        dec = Decoder(N, K, ALGO_CASCL, L=L, crc_taps=crc_taps, **kw)
    if stages is not None:
        dec.set_cascl_stages(stages)
    return dec


def SCFlip(N, K, T=8, crc_taps=CRC24C_TAPS, crc_file=None, **kw):
    """CRC-aided SC-Flip (include/polar_hip.h, POLAR_ALGO_SCF): SC over the K + r unfrozen positions; a frame that fails
    the CRC is decoded again with one of its T least reliable decisions inverted, up to T times, until one passes.
    ``crc_taps`` / ``crc_file`` / ``systematic`` as for CASCL."""
    if crc_file is not None:
        dec = Decoder(N, K, ALGO_SCF, L=1, crc_taps=None, crc_file=crc_file, **kw)
    else:
        dec = Decoder(N, K, ALGO_SCF, L=1, crc_taps=crc_taps, **kw)
    if T != 8:
        dec.set_scf_flips(T)
    return dec


def DSCFlip(N, K, budgets=(8, 16), c=1.5, tau=5.0, crc_taps=CRC24C_TAPS, crc_file=None, **kw):
    """Dynamic SC-Flip (include/polar_hip.h, polar_scf_set_dynamic): SCFlip whose attempts invert sets of up to len(budgets)
    decisions, budgets[k] sets of size k + 1, ranked by the multiplier-free metric with penalty ``c`` and threshold ``tau``
    (defaults: the constants of Ercan et al., 2020; DESIGN.md 4.6 has what they measured here)."""
    dec = SCFlip(N, K, T=8, crc_taps=crc_taps, crc_file=crc_file, **kw)
    dec.set_scf_dynamic(budgets, c, tau)
    return dec


def BPL(N, K, iterMax=100, graphs=None, crc_taps=None, **kw):
    """BP list decoding over permuted factor graphs (include/polar_hip.h, POLAR_ALGO_BPL): BP with the G-matrix stop rule and
    iterMax round trips per attempt; a frame that does not converge (or, with ``crc_taps``, converges to a word that fails the
    CRC) is decoded again on the next graph of the list.  ``graphs``: None (the default list, min(n, 8) cyclic shifts), an
    int P (the first P cyclic shifts) or a list of permutations of 0 .. n-1 (Decoder.set_bpl_graphs)."""
    dec = Decoder(N, K, ALGO_BPL, L=1, bp_iters=iterMax, crc_taps=crc_taps, **kw)
    if graphs is not None:
        n = int(N).bit_length() - 1
        dec.set_bpl_graphs(bpl_cyclic_graphs(n, graphs) if isinstance(graphs, (int, np.integer)) else graphs)
    return dec


def SCAN(N, K, iters=4, **kw):
    """Soft-output SCAN (include/polar_hip.h, POLAR_ALGO_SCAN): BP's message arithmetic on SC's schedule, ``iters``
    iterations; Decoder.decode_scan_device / decode_scan_batch return an LLR for every u bit and every code bit."""
    dec = Decoder(N, K, ALGO_SCAN, L=1, **kw)
    if iters != 4:
        dec.set_scan_iters(iters)
    return dec


def pac_info_order(N, K, profile="rm"):
    """Information set of a PAC code in ascending reliability.  "rm": the K positions of largest popcount(j) (the
    Reed-Muller rate profile), ties to the more reliable in the library's order; "5g": the K most reliable."""
    q = q_sequence(N)
    if profile == "5g":
        return np.asarray(q[N - K:], dtype=np.int32)
    if profile != "rm":
        raise ValueError("profile must be 'rm' or '5g'")
    rel = {j: i for i, j in enumerate(q)}
    best = sorted(range(N), key=lambda j: (bin(j).count("1"), rel[j]))[N - K:]
    return np.asarray(sorted(best, key=lambda j: rel[j]), dtype=np.int32)


def PAC(N, K, g=0o133, L=32, profile="rm", **kw):
    """Polarization-adjusted convolutional code under list decoding (include/polar_hip.h, dynamic frozen bits): SCL (SC for
    L = 1) over the rate profile `profile` (pac_info_order) with every other position a dynamic frozen bit of the precoder g.
    Decisions are u-domain rows; ``pac_unprecode(u_hat, g)[..., dec.info_order]`` is the payload.  L = 64, 128 or 256 (a wide
    list, N * L <= 65536) is where PAC(128, 64) gains over the default of 32."""
    io = pac_info_order(N, K, profile)
    dec = Decoder(N, K, ALGO_SCL if L > 1 else ALGO_SC, L=L, info_order=io, dyn=dyn_pac(N, io, g), **kw)
    dec.pac_g = pac_taps(g)
    return dec


def PCCASCL(N, K, n_pc=3, n_pc_wm=0, L=8, crc_taps=CRC6_TAPS, **kw):
    """5G parity-check CRC-aided polar code at E = N (38.212 5.3.1.2): Q_I = the K + r + n_pc most reliable positions, n_pc
    of them parity-check bits (dyn_pc5g), CA-SCL over the rest.  L up to 32, or a wide list of 64, 128 or 256."""
    r = int(max(crc_taps))
    q = q_sequence(N)
    pos, sets, io = dyn_pc5g(N, q[N - (K + r + n_pc):], n_pc, n_pc_wm)
    return Decoder(N, K, ALGO_CASCL, L=L, crc_taps=crc_taps, info_order=io, dyn=(pos, sets), **kw)


def decode(llr_in, frozen_mask, N, L):
    """BASELINE.json north_star call shape ``decode(llr_in, frozen_mask, N, L)`` -> u_hat[N]."""
    lib = load_library()
    llr = np.ascontiguousarray(llr_in, dtype=np.float64)
    fm = np.ascontiguousarray(frozen_mask, dtype=np.uint8)
    if llr.shape != (N,) or fm.shape != (N,):
        raise ValueError("llr_in and frozen_mask must have shape (N,)")
    uh = np.empty(N, dtype=np.int32)
    rc = lib.polar_decode_llr(_ptr(llr, C.c_double), _ptr(fm, C.c_ubyte), N, L, _ptr(uh, C.c_int))
    if rc != 0:
        raise PolarError(f"polar_decode_llr: {lib.polar_strerror(rc).decode()} (rc={rc})")
    return uh
