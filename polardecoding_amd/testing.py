"""ctypes binding of include/polar_hip_testing.h -- the TEST-ONLY entry points (kernel selection for cross-checks, the
kernels' scalar arithmetic on chosen operands).  They live in libpolar_hip_testing.so, a second build of the same sources
with -DPOLAR_TESTING; the product library libpolar_hip.so does not export them.  A decoder handed to select_kernel /
big_split is re-created inside the test library first.  Used by tests/ and tools/, never by the product."""
import ctypes as C

import numpy as np

from .api import PolarError, load_library

KERNEL_AUTO, KERNEL_GENERIC, KERNEL_GENERIC_SPILL, KERNEL_BIG, KERNEL_ONE_PER_WAVE, KERNEL_FOUR_PER_WAVE = 0, 1, 2, 3, 4, 5
OP_CHK, OP_CHK_LUT, OP_CHK_LUT1, OP_TABV, OP_PHI, OP_PHI_LUT, OP_CHK_CNT, OP_CHK_IDX, OP_CHK_TAB = 0, 1, 2, 3, 4, 5, 6, 7, 8


def select_kernel(dec, variant):
    """dec: a polardecoding_amd Decoder.  Returns dec (its kernel_name reflects the choice)."""
    lib = load_library(testing=True)
    dec._rebind(lib)
    lib.polar_testing_select_kernel.argtypes = [C.c_void_p, C.c_int]
    rc = lib.polar_testing_select_kernel(dec._h, int(variant))
    if rc != 0:
        raise PolarError(f"polar_testing_select_kernel rc={rc}")
    return dec


def big_split(dec, split):
    lib = load_library(testing=True)
    dec._rebind(lib)
    lib.polar_testing_big_split.argtypes = [C.c_void_p, C.c_int]
    rc = lib.polar_testing_big_split(dec._h, int(split))
    if rc != 0:
        raise PolarError(f"polar_testing_big_split rc={rc}")
    return dec


def chunk_bytes(dec, nbytes):
    """The byte cap of the chunked host loops (polar_testing_chunk_bytes): a pass takes at most nbytes of rows, so a few
    hundred frames cross pass boundaries.  0 restores 256 MiB.  The decoder keeps the cap across a later rebind."""
    lib = load_library(testing=True)
    dec._rebind(lib)
    lib.polar_testing_chunk_bytes.argtypes = [C.c_void_p, C.c_size_t]
    rc = lib.polar_testing_chunk_bytes(dec._h, int(nbytes))
    if rc != 0:
        raise PolarError(f"polar_testing_chunk_bytes rc={rc}")
    dec._chunk_bytes = int(nbytes)
    return dec


def resident_blocks(dec, blocks):
    """The cap on the resident grid (polar_testing_resident_blocks): every launch of dec whose kernel loops over its jobs
    starts at most `blocks` blocks, so a few dozen frames reach a wavefront's later jobs.  0 restores the library's choice.
    The decoder keeps the cap across a later rebind."""
    lib = load_library(testing=True)
    dec._rebind(lib)
    lib.polar_testing_resident_blocks.argtypes = [C.c_void_p, C.c_int]
    rc = lib.polar_testing_resident_blocks(dec._h, int(blocks))
    if rc != 0:
        raise PolarError(f"polar_testing_resident_blocks rc={rc}")
    dec._resident_blocks = int(blocks)
    return dec


def last_plan(dec):
    """(grid, jobs, jobs_per_block, queued) of dec's most recent decoder-kernel launch (polar_testing_last_plan)."""
    lib = load_library(testing=True)
    dec._rebind(lib)
    lib.polar_testing_last_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int)]
    g, j, p, q = C.c_int(), C.c_longlong(), C.c_int(), C.c_int()
    rc = lib.polar_testing_last_plan(dec._h, C.byref(g), C.byref(j), C.byref(p), C.byref(q))
    if rc != 0:
        raise PolarError(f"polar_testing_last_plan rc={rc}")
    return g.value, j.value, p.value, q.value


def last_stride(dec):
    """(grid, blocks the work needs) of dec's most recent fixed-stride launch that sizes its own grid
    (polar_testing_last_stride)"""
    lib = load_library(testing=True)
    dec._rebind(lib)
    lib.polar_testing_last_stride.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    g, n = C.c_int(), C.c_longlong()
    rc = lib.polar_testing_last_stride(dec._h, C.byref(g), C.byref(n))
    if rc != 0:
        raise PolarError(f"polar_testing_last_stride rc={rc}")
    return g.value, n.value


def math(op, a, b, dtype=np.float64, device=0):
    """The device functions of csrc/polar_math.h / polar_lut.h applied element-wise on the GPU."""
    lib = load_library(testing=True)
    lib.polar_testing_math.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.ascontiguousarray(a, dtype=dtype).ravel()
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=dtype), a.shape), dtype=dtype).ravel()
    out = np.empty_like(a)
    rc = lib.polar_testing_math(int(op), 1 if dtype == np.float32 else 0, a.ctypes.data, b.ctypes.data,
                                out.ctypes.data, a.size, device)
    if rc != 0:
        raise PolarError(f"polar_testing_math rc={rc}")
    return out
