// scl_book.h -- code books (include/polar_hip.h, "Code books"): one launch decodes frames of different codes.
//
// k_scl_book is scl_generic.h's scl_generic_body with DYN = BOOK = true, k_scl_book_list the same with LIST = true: the
// texts of k_scl_dyn and k_scl_list with a per-frame choice of the tables (book_desc.h).  What BOOK adds at the top of the
// frame loop: the frame's code index (wave-uniform, range-checked before it addresses anything), that member's 64-byte
// descriptor, and on a rate-matched member the recovery of the N decoder values from the frame's E input values in the
// load stage.  The LDS layout, the dynamic LDS bytes, the choice between LDS-resident and global-scratch levels and the
// scratch slice are those of the largest member (SclParams::N), so a launch runs at that member's occupancy.
#pragma once
#include "scl_dyn.h"

namespace polar {

struct BookParams {
    SclParams s;   // N, n: the largest member's; frozen, crc_tab, sc_mode are not read
    BookArgs k;
    ListOut o;     // k_scl_book_list only
};

template <typename R, typename IN, int LOGL, bool GA>
__global__ __launch_bounds__(64) void k_scl_book(BookParams BP)
{
    scl_generic_body<R, IN, LOGL, GA, true, false, true>(BP.s, nullptr, nullptr, nullptr, &BP.k);
}

template <typename R, typename IN, int LOGL, bool GA>
__global__ __launch_bounds__(64) void k_scl_book_list(BookParams BP)
{
    scl_generic_body<R, IN, LOGL, GA, true, true, true>(BP.s, nullptr, nullptr, &BP.o, &BP.k);
}

}  // namespace polar
