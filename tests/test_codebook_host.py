"""CPU: code books (include/polar_hip.h, "Code books"): the symbols resolve with the argtypes the Python mirror declares, and
the refusals that need no device return before one is touched."""
import ctypes as C

import pytest


def _lib():
    import polardecoding_amd as pa
    return pa.load_library()


def test_symbols_resolve_with_the_declared_argtypes():
    lib = _lib()
    n_args = {"polar_codebook_create": 3, "polar_codebook_destroy": 1, "polar_codebook_info": 6, "polar_codebook_member": 5,
              "polar_codebook_set_stream": 2, "polar_codebook_get_stream": 1, "polar_codebook_synchronize": 1,
              "polar_codebook_kernel_name": 1, "polar_codebook_last_error": 1, "polar_codebook_decode": 10,
              "polar_codebook_list_decode": 12, "polar_codebook_decode_host": 9}
    for name, n in n_args.items():
        assert len(getattr(lib, name).argtypes) == n, name
    assert lib.polar_codebook_kernel_name.restype is C.c_char_p and lib.polar_codebook_get_stream.restype is C.c_void_p


def test_refusals_that_touch_no_device():
    lib = _lib()
    EINVAL = -1
    one = (C.c_void_p * 1)(None)
    for members, n in ((None, 1), (one, 0), (one, 1025), (one, -1), (one, 1)):   # NULL list, C out of range, a NULL member
        h = C.c_void_p(1)
        assert lib.polar_codebook_create(members, n, C.byref(h)) == EINVAL and not h.value
    assert lib.polar_codebook_create(one, 1, None) == EINVAL
    lib.polar_codebook_destroy(None)
    assert lib.polar_codebook_info(None, None, None, None, None, None) == EINVAL
    assert lib.polar_codebook_member(None, 0, None, None, None) == EINVAL
    assert lib.polar_codebook_synchronize(None) == EINVAL and lib.polar_codebook_set_stream(None, None) == EINVAL
    assert lib.polar_codebook_get_stream(None) is None
    assert lib.polar_codebook_kernel_name(None) == b"" and lib.polar_codebook_last_error(None) == b""
    assert lib.polar_codebook_decode(None, None, 0, 0, None, 0.0, 1, None, None, None) == EINVAL
    assert lib.polar_codebook_list_decode(None, None, 0, 0, None, 0.0, 1, None, None, None, None, None) == EINVAL
    assert lib.polar_codebook_decode_host(None, None, 0, None, 0.0, 1, None, None, None) == EINVAL


def test_an_empty_code_book_raises():
    import polardecoding_amd as pa
    with pytest.raises(ValueError):
        pa.Codebook([])


def test_the_flag_is_the_headers():
    import os
    import re
    import polardecoding_amd as pa
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "polar_hip.h")).read()
    assert int(re.search(r"#define POLAR_FLAG_NO_CODE (0x[0-9a-f]+)u", hdr).group(1), 16) == pa.FLAG_NO_CODE
