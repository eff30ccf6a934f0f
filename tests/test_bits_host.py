"""CPU: the word-level steps every list kernel takes from csrc/polar_bits.h, as a program of its own (never loaded into
Python).  tests/native/bits_selftest.cpp holds polar_word_transform and polar_word_transform_n (n = 0 .. 5) to x = u F^{(x)n}
written out over GF(2) on all 2^16 words with an empty upper half, on their images shifted left by 16 and on 10 000 random
words, checks the involution, and runs scl_generic.h's partial-sum update with ps_fold0 / ps_save0 on every bit sequence of
N = 16 and on 10 000 random ones of N = 32 beside updateBit on plain arrays, compared at every leaf and, at the last one,
with the encoding."""
import os
import subprocess

from conftest import REPO


def test_word_transform_and_word0_partial_sums():
    native = os.path.join(REPO, "tests", "native")
    out_dir = os.path.join(REPO, "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "bits_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(native, "bits_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "bits_selftest: ok" in out.stdout
