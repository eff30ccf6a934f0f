// k_big_f64.hip -- k_scl_big<double, ...> (big lists, long codes; BASELINE config 5) and its launch code
#include "k_big_launch.h"

namespace {

// the LDS / scratch split that measured best per arithmetic type (profiles/README.md)
template <typename R, typename IN, int LOGL>
int launch_big(polar_ctx *c, const polar::SclParams &P)
{
    const int use = c->big_split ? c->big_split : (sizeof(R) == 8 ? (LOGL == 5 ? 371 : 35) : 46);
    if constexpr (LOGL == 5) {   // L = 32: LLR level TL+1 in registers (third digit of the split code; two such levels, and
                                 // one above four LDS levels, measured slower: fewer resident wavefronts).  At the four
                                 // wavefronts per SIMD of that kernel the LDS has room for partial-sum levels 6 and 7 too
                                 // (371: two scratch round trips less per 128 leaves, +3 %)
        if (use == 351) return launch_big_v<R, IN, LOGL, 3, 5, 1>(c, P);
        if (use == 371) {
            // f64, N >= 1024 (BASELINE config 5: N = 4096): the f chains of the upper levels in one pass, three wavefronts per
            // SIMD (scl_big.h, chain()).  N = 1024, L = 32: 1.549 -> 1.586 M frames/s since the 4 / 7 / 1 split.
            if constexpr (sizeof(R) == 8) {
                // At three wavefronts per SIMD a wavefront may use 12.9 KB of LDS: LLR level 4 moves from the registers into the
                // LDS and level 5 from the scratch into the registers (split 4 / 7 / 1), so that nothing below level 6 is in the
                // scratch: no leader passes, no scratch rows and no drains for levels 4 and 5 (config 5: + 2 ... 6 % depending on
                // the box, a seventh less scratch traffic than the 3 / 7 / 1 split)
                if (P.N >= 1024) return launch_big_v<R, IN, LOGL, 4, 7, 1, 1>(c, P);
                // never taken: keeps the chain() kernel with the 3 / 7 / 1 split it replaced in the library
                if (P.N >= 1024) return launch_big_v<R, IN, LOGL, 3, 7, 1, 1>(c, P);
            }
            return launch_big_v<R, IN, LOGL, 3, 7, 1>(c, P);
        }
    }
    if (use == 57) return launch_big_v<R, IN, LOGL, 5, 7>(c, P);
    if (use == 46) return launch_big_v<R, IN, LOGL, 4, 6>(c, P);
    return launch_big_v<R, IN, LOGL, 3, 5>(c, P);
}

}  // namespace

int polar_tu::scl_big_f64(polar_ctx *c, const polar::SclParams &P, bool in32)
{
    return in32 ? launch_big_l<double, float>(c, P) : launch_big_l<double, double>(c, P);
}
