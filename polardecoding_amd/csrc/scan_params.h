// scan_params.h -- argument block of the SCAN kernel (scan_lanes.h), shared with the host layer
#pragma once
#include <stdint.h>

namespace polar {

struct ScanParams {
    const void *in;            // [B][N] double or float: LLRs, or y when sigma > 0
    double sigma;
    uint32_t *out_bits;        // [B][N/32] or null
    void *llr_u;               // [B][N] of the arithmetic type, or null
    void *ext_x;               // [B][N] of the arithmetic type, or null
    const uint32_t *frozen;    // [N/32] bit j = leaf j frozen
    int N, n, B, iters;
    void *scratch;
    unsigned *queue;           // polar_host.h work_queue(); null = jobs by a fixed stride
};

constexpr int SCAN_MAX_ITERS = 64;   // polar_scan_set_iters
constexpr int SCAN_MAX_N = 1024;     // the frozen mask is one word per lane, the stored betas n*N/2 values per codeword

}  // namespace polar
