"""CPU: the owning types behind polar_ctx and polar_group (csrc/dev_owned.h) against a stub HIP runtime, under
AddressSanitizer + UBSan + LeakSanitizer.  tests/native/owned_selftest.cpp is a program of its own (never loaded into
Python): construct-destroy, moves onto live objects, std::swap of two Bufs, reset() twice, a borrowed stream, and
DevMem::upload with the allocation and with the copy failing; a double free, a leak or an unbalanced stub counter fails it."""
import os
import subprocess

from conftest import REPO


def test_owning_types_under_asan_ubsan():
    native = os.path.join(REPO, "tests", "native")
    out_dir = os.path.join(REPO, "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "owned_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(native, "hip_stub"),
                           "-o", exe, os.path.join(native, "owned_selftest.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "owned_selftest: ok" in out.stdout
