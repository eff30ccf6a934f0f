// book_desc.h -- code books (include/polar_hip.h, "Code books"): what scl_generic_body<..., BOOK> reads per frame.
//   BookCode      one member's tables and shape, 64 bytes, 64-byte aligned: the kernel loads it as 16 wave-uniform words
//   BookArgs      the [C] table of them, the per-frame code indices and the row stride of the input
//   book_code()   the descriptor of code c as a wave-uniform value
//   book_rm_load  the load stage of a rate-matched member: ch[i], i < N, from the frame's E input values (rule 6 of "5G NR
//                 rate matching"), k_rm_recover's arithmetic without its [B][N] rows in global memory
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "polar_math.h"

namespace polar {

constexpr int BOOK_RM_NONE = 0, BOOK_RM_REPEAT = 1, BOOK_RM_PUNCTURE = 2, BOOK_RM_SHORTEN = 3;   // POLAR_RM_*
constexpr double BOOK_RM_SHORT_LLR = 1048576.0;                                                  // POLAR_RM_SHORT_LLR
constexpr uint32_t BOOK_FLAG_NO_CODE = 0x10u;                                                    // POLAR_FLAG_NO_CODE
constexpr int BOOK_MAX_N = 1024, BOOK_MAX_C = 1024;

struct alignas(64) BookCode {
    const uint32_t *frozen;     // [N/32] bit j = leaf j frozen
    const uint32_t *crc_tab;    // [N], or null: no CRC
    const uint32_t *dyn_mask;   // [D][N/32]; a member without constraints: one zero row
    const int *dyn_row;         // [N]: row of leaf j, or -1
    const uint16_t *ilv;        // [E] sent-row position of e_k (ibil), or null
    int N, n;
    int E, logS, rm_mode;       // BOOK_RM_*; E and logS (N / 32 = 2^logS) are read on a rate-matched member only
    int sc_mode;
};
static_assert(sizeof(BookCode) == 64, "one descriptor is sixteen words");

struct BookArgs {
    const BookCode *codes;      // [C]
    const uint32_t *code;       // [B] code index of frame f; >= C: BOOK_FLAG_NO_CODE
    uint32_t C;
    size_t ld;                  // row stride of the input in elements, >= every member's row width
};

// the inverse of the sub-block interleaver pattern P of 38.212 Table 5.4.1.1-1 (rm_kernel.h kRmP): inv[P[t]] = t
#define POLAR_BOOK_RM_PINV 0, 1, 2, 4, 3, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22, 9, 11, 13, 15, 17, 19, 21, 23, 24, 25, 26, 28, 27, 29, 30, 31
constexpr bool book_rm_pinv_ok()
{
    constexpr unsigned char P[32] = {0, 1, 2, 4, 3, 5, 6, 7, 8, 16, 9, 17, 10, 18, 11, 19,
                                     12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31};
    constexpr unsigned char inv[32] = {POLAR_BOOK_RM_PINV};
    for (int t = 0; t < 32; ++t)
        if (inv[P[t]] != t) return false;
    return true;
}
static_assert(book_rm_pinv_ok(), "the table below inverts 38.212 Table 5.4.1.1-1");
__device__ __forceinline__ int book_rm_pinv(int b)
{
    constexpr unsigned char inv[32] = {POLAR_BOOK_RM_PINV};
    return inv[b];
}

// c is wave-uniform and below C: every lane reads the same sixteen words, and readfirstlane makes them scalar values
__device__ __forceinline__ BookCode book_code(const BookCode *codes, uint32_t c)
{
    const uint32_t *q = reinterpret_cast<const uint32_t *>(codes + c);
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)q[i]);
    BookCode d;
    __builtin_memcpy(&d, w, sizeof d);
    return d;
}

// Decoder position i holds y_m with J(m) = i.  The terms are gathered from the row in global memory (it is at most 8 KiB
// and stays in the vector L1 for the frame's load stage); they are summed in double in ascending k, rounded once to IN,
// then converted to R: what k_rm_recover followed by the plain load computes.  Only src[0 .. E) is read.
template <typename R, typename IN>
__device__ __forceinline__ void book_rm_load(R *ch, const IN *src, const BookCode &d, double sigma, int lane)
{
    const int N = d.N, E = d.E, S1 = (1 << d.logS) - 1;
    const bool y = sigma > 0;
    auto term = [&](int k) -> double {
        const double v = (double)src[d.ilv ? (int)d.ilv[k] : k];
        return y ? llr_from_y(v, sigma) : v;
    };
    for (int i = lane; i < N; i += 64) {
        const int m = (book_rm_pinv(i >> d.logS) << d.logS) | (i & S1);
        double v;
        if (d.rm_mode == BOOK_RM_REPEAT) {
            v = term(m);
            for (int k = m + N; k < E; k += N) v += term(k);
        } else if (d.rm_mode == BOOK_RM_PUNCTURE) {
            v = (m < N - E) ? 0.0 : term(m - (N - E));
        } else {
            v = (m < E) ? term(m) : BOOK_RM_SHORT_LLR;
        }
        ch[i] = (R)(IN)v;
    }
}

}  // namespace polar
