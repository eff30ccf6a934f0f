// scf_params.h -- the argument block of the SC-Flip kernels (scf_lanes.h), shared with the host layer.
#pragma once
#include <stdint.h>

namespace polar {

enum { SCF_CHECK = 0, SCF_RECORD = 1, SCF_FLIP = 2 };   // leaf policies of k_scf_lanes
constexpr uint32_t SCF_CRC_PASS = 0x2u;                 // POLAR_FLAG_CRC_PASS
constexpr int SCF_MAX_T = 32;                           // flip budget: at most 32 attempts per frame

struct ScfParams {
    const void *in;           // [frames][N] double or float: LLRs, or y when sigma > 0
    double sigma;
    uint32_t *out_bits;       // CHECK: [B][N/32] per frame; FLIP: [B][N/32] per pair; RECORD: unused
    double *pm;               // CHECK: [B] or null (0.0)
    uint32_t *flags;          // CHECK: [B] flags word; FLIP: [B] 1 = the pair passed the CRC
    uint32_t *attempts;       // CHECK: [B] or null: 0 on a pass, T otherwise
    const uint32_t *frozen;   // [N/32]
    const uint32_t *crc_tab;  // [N]
    const uint32_t *idx;      // RECORD: item q is frame idx[q]; FLIP: item q is frame idx[q / T]; CHECK: null (item = frame)
    uint16_t *flips;          // RECORD: written [B][T]; FLIP: flips[q] = the leaf pair q inverts
    int N, n;
    int B;                    // items
    int T;
    void *scratch;            // per wavefront: ScLanesCfg<R>::scratch_bytes(N)
    unsigned *queue;
};

}  // namespace polar
