// scf_params.h -- the argument block of the SC-Flip kernels (scf_lanes.h), shared with the host layer.
#pragma once
#include <stdint.h>

namespace polar {

enum { SCF_CHECK = 0, SCF_RECORD = 1, SCF_FLIP = 2 };   // leaf policies of k_scf_lanes
// leaf policies of the dynamic rule (polar_scf_set_dynamic): the record pass on the metric M(0, i), run(E) of a flip set,
// and run(E) that also keeps the lane's T_{k+1} best extensions of E
enum { SCF_RECORD_M = 3, SCF_FLIPSET = 4, SCF_FLIPREC = 5 };
constexpr uint32_t SCF_CRC_PASS = 0x2u;                 // POLAR_FLAG_CRC_PASS
constexpr int SCF_MAX_T = 32;                           // flip budget: at most 32 attempts per frame (and per level)
constexpr int SCF_MAX_ORDER = 3;                        // POLAR_SCF_MAX_ORDER: positions per flip set
constexpr uint16_t SCF_NO_POS = 0xFFFFu;                // padding of a flip set; a set that starts with it is absent

struct ScfParams {
    const void *in;           // [frames][N] double or float: LLRs, or y when sigma > 0
    double sigma;
    uint32_t *out_bits;       // CHECK: [B][N/32] per frame; FLIP, FLIPSET, FLIPREC: [B][N/32] per pair; else unused
    double *pm;               // CHECK: [B] or null (0.0)
    uint32_t *flags;          // CHECK: [B] flags word; FLIP, FLIPSET, FLIPREC: [B] 1 = the pair passed the CRC
    uint32_t *attempts;       // CHECK: [B] or null: 0 on a pass, T otherwise
    const uint32_t *frozen;   // [N/32]
    const uint32_t *crc_tab;  // [N]
    const uint32_t *idx;      // RECORD(_M): item q is frame idx[q]; FLIP*: item q is frame idx[q / T]; CHECK: null (item = frame)
    uint16_t *flips;          // RECORD: written [B][T]; FLIP: flips[q] = the leaf pair q inverts;
                              // FLIPSET, FLIPREC: flips[3 q .. 3 q + 3) = the set of pair q, ascending, SCF_NO_POS padded
    int N, n;
    int B;                    // items
    int T;
    void *scratch;            // per wavefront: ScLanesCfg<R>::scratch_bytes(N)
    unsigned *queue;
    // the dynamic rule (RECORD_M, FLIPREC; unused by the other policies)
    int Tn;                   // length of the list an item keeps
    double mc, tau;           // penalty c and threshold tau, rounded to R in the kernel
    void *lkey;               // written [B][Tn] R: the keys M(E, i) of the item's list, ascending (key, i)
    uint16_t *lpos;           // written [B][Tn]: their i
    uint32_t *lcnt;           // written [B]: entries of the list (< Tn when fewer positions lie above max(E))
};

}  // namespace polar
