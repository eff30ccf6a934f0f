// list_out.h -- where the LIST epilogue of scl_generic_body / k_scl_wide writes a frame's whole list (include/polar_hip.h,
// "List output", rules 2 and 3): rank k = the live slots in ascending (PM, slot), padding behind them.
#pragma once
#include <stdint.h>

namespace polar {

struct ListOut {
    uint32_t *paths;   // [B][L][N/32] or null
    double *pm;        // [B][L] or null
    uint32_t *rem;     // [B][L] or null
    uint32_t *count;   // [B] or null
};

}  // namespace polar
