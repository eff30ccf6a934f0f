/* CPU self-test of csrc/polar_bits.h, a program of its own (tests/test_bits_host.py compiles and runs it).
 *
 * polar_word_transform / polar_word_transform_n against x = u F^{(x)n} written out over GF(2) (x[j] = sum of the u[i] whose
 * index contains j bitwise), and the involution; ps_fold0 / ps_save0 by running scl_generic.h's partial-sum update of one
 * path with them and comparing, at every leaf, with updateBit on plain arrays (one uint8_t per element per level). */
#define __host__
#define __device__
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../polardecoding_amd/csrc/polar_bits.h"

using polar::polar_word_transform;
using polar::polar_word_transform_n;
using polar::ps_fold0;
using polar::ps_save0;

static long failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond) && failures++ < 10) {                 \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

// x = u F^{(x)n} on every aligned group of 2^n bits of the word, element by element
static uint32_t naive_transform(uint32_t u, int n)
{
    const int g = 1 << n;
    uint32_t x = 0;
    for (int base = 0; base < 32; base += g)
        for (int j = 0; j < g; ++j) {
            uint32_t s = 0;
            for (int i = 0; i < g; ++i)
                if ((i & j) == j) s ^= (u >> (base + i)) & 1u;
            x |= s << (base + j);
        }
    return x;
}

static void check_word(uint32_t w)
{
    const uint32_t x = polar_word_transform(w);
    CHECK(x == naive_transform(w, 5), "polar_word_transform(%08x) = %08x, naive %08x", w, x, naive_transform(w, 5));
    CHECK(polar_word_transform(x) == w, "polar_word_transform is no involution at %08x", w);
    for (int n = 0; n <= 5; ++n) {
        const uint32_t low = (n == 5) ? w : w & ((1u << (1 << n)) - 1u);   // the whole row of an N = 2^n code
        CHECK(polar_word_transform_n(low, n) == naive_transform(low, n), "polar_word_transform_n(%08x, %d) = %08x, naive %08x",
              low, n, polar_word_transform_n(low, n), naive_transform(low, n));
        CHECK(polar_word_transform_n(w, n) == naive_transform(w, n), "polar_word_transform_n(%08x, %d), every group", w, n);
    }
}

// One path of a code of N = 2^n <= 32 bits decides u (bit j = leaf j): the packed update of scl_generic.h beside updateBit
// (SCL_1024.c:424-448) on arrays; left[t][e] = saved left-child sums of level t, cur[e] = the working sums.
static void check_sequence(uint32_t u, int n)
{
    const int N = 1 << n;
    uint8_t left[5][16], cur[32], nxt[32];
    std::memset(left, 0, sizeof left);
    uint32_t bl0 = 0, cur0 = 0;
    for (int j = 0; j < N; ++j) {
        const uint32_t bit = (u >> j) & 1u;
        // packed
        cur0 = bit;
        int t = 0;
        while (t < n && ((j >> t) & 1)) {
            cur0 = ps_fold0(bl0, cur0, t);
            ++t;
        }
        if (t < n) bl0 = ps_save0(bl0, cur0, t);
        // arrays
        cur[0] = (uint8_t)bit;
        int s = 0;
        while (s < n && ((j >> s) & 1)) {
            const int h = 1 << s;
            for (int e = 0; e < h; ++e) {
                nxt[e] = left[s][e] ^ cur[e];
                nxt[e + h] = cur[e];
            }
            std::memcpy(cur, nxt, 2 * h);
            ++s;
        }
        if (s < n) std::memcpy(left[s], cur, 1 << s);
        // level t, element e <-> bit 2^t + e of bl0; the working sums from bit 0 of cur0
        uint32_t want_bl = 0, want_cur = 0;
        for (int lv = 0; lv < n; ++lv)
            for (int e = 0; e < (1 << lv); ++e) want_bl |= (uint32_t)left[lv][e] << ((1 << lv) + e);
        for (int e = 0; e < (1 << s); ++e) want_cur |= (uint32_t)cur[e] << e;
        CHECK(t == s && bl0 == want_bl, "n=%d u=%08x leaf %d: bl0 %08x, arrays %08x", n, u, j, bl0, want_bl);
        CHECK(cur0 == want_cur, "n=%d u=%08x leaf %d: cur0 %08x, arrays %08x", n, u, j, cur0, want_cur);
    }
    const uint32_t row = (n == 5) ? u : u & ((1u << N) - 1u);
    CHECK(cur0 == naive_transform(row, n), "n=%d u=%08x: root sums %08x, encoding %08x", n, u, cur0, naive_transform(row, n));
}

int main()
{
    std::mt19937 rng(20240611u);
    for (uint32_t w = 0; w < (1u << 16); ++w) {
        check_word(w);
        check_word(polar_word_transform(w) << 16);
        check_sequence(w, 4);
    }
    for (int i = 0; i < 10000; ++i) check_word((uint32_t)rng());
    for (int i = 0; i < 10000; ++i) check_sequence((uint32_t)rng(), 5);
    if (failures) {
        std::printf("bits_selftest: %ld failures\n", failures);
        return 1;
    }
    std::printf("bits_selftest: ok\n");
    return 0;
}
