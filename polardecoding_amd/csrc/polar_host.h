// polar_host.h -- internal: the context object behind the C ABI and the launcher each kernel translation unit exports.
// The library is built from several translation units (one per kernel family, compiled in parallel; see
// __graft_entry__.py): polar_hip.hip and h_*.hip hold the C ABI and the host logic, k_*.hip the kernels with their launch code.
#pragma once
#include "../../include/polar_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "book_desc.h"
#include "dev_owned.h"
#include "polar_params.h"

namespace polar {
struct TraceOut;    // trace_out.h
struct ScfParams;   // scf_params.h
struct GenParams;   // gen_common.h
struct ScanParams;  // scan_lanes.h
}

// What belongs to one stream of a ctx.  The rule: a buffer that a decode on c->stream writes and that the two halves of
// fer_batch_impl (h_fer.hip) would share belongs here, beside the stream.  A polar_ctx IS its current lane (c->stream,
// c->scratch, ... are the names the k_*.hip launchers read) and holds a second one, lane_b; swap_lane() below is the only
// code that exchanges the two, so a member added here is swapped without another line.
// Deliberately outside the lane: the ad_* / scf_* buffers (fer_batch_impl does not split for adaptive CA-SCL or SC-Flip)
// and q8_pm (fer_batch_impl passes no d_pm, so the halves never touch it).
struct Lane {
    Stream stream;    // before the buffers: they are released first
    Buf scratch;      // per-wave scratch of the persistent kernels, with their work queue
    Buf rm_rows;      // polar_create_rm: the recovered N-wide rows of one chunk
    Buf q8_rows;      // POLAR_Q8: the quantised rows of the float entry points, one chunk
};

constexpr size_t kChunkBytes = (size_t)256 << 20;   // a chunked pass takes at most this many bytes of rows

// Every device resource of a ctx is a member of an owning type (dev_owned.h): polar_destroy only synchronises and deletes.
// The streams are declared before the buffers, so that the buffers are released first.
struct polar_ctx : Lane {
    polar_cfg cfg{};
    int n = 0, A = 0, NW = 0, logL = 0;
    std::vector<int> info_order;          // I[]
    std::vector<unsigned char> frozen;    // [N]
    std::vector<int> taps;
    std::vector<uint32_t> h_crc_tab;      // [N]
    Stream copy_stream;                   // host -> device copies overlap the decode of the previous chunk
    Lane lane_b;                          // polar_fer_batch runs its two halves on two streams: the second one's lane
    Event ev_b;
    Event ev_in[2], ev_free[2], ev_out[2];   // chunked host pipeline
    Event ev0, ev1;                       // polar_time_decode_device
    DevMem<uint32_t> d_frozen;            // [NW] bit = frozen
    DevMem<uint32_t> d_info;              // [NW] bit = unfrozen
    DevMem<uint32_t> d_crc_tab;           // [N] or empty
    DevMem<uint32_t> d_crc_mask;          // [CRC_MASK_ROWS][NW] the same table as masks over x_hat (make_crc_masks), or empty
    DevMem<uint32_t> d_gc_rows;           // [K] systematic CRC generator rows (D^(r+k) mod g), or empty
    DevMem<uint32_t> d_frozen_override;
    int fill_end = 0, fill_end_override = 0;   // fill_phase_end() of the mask in d_frozen / d_frozen_override (pair kernel)
    DevMem<int> d_info_order;             // [A] for the device-side generator and the encoder (info_order_table)
    int num_cu = 0;
    Buf in, bits, pm, flags;              // staging for the host-pointer entry points
    Buf bp_iters;                         // polar_bp_decode_batch: round trips per frame
    int bp_stop = POLAR_BP_STOP_NONE;     // polar_bp_set_stop
    // adaptive CA-SCL (polar_cascl_set_stages): list sizes of the stages (empty = the fixed decoder) and one context per
    // stage (an SC context for L = 1, null for L = cfg.L: this context's own fixed decoder); they borrow this ctx's stream
    std::vector<int> cascl_stages;
    std::vector<polar_ctx *> stage_ctx;
    Buf ad_flags;                         // per-frame flags when the caller passes none
    Buf ad_idx[2], ad_blk, ad_cnt;        // failing-frame lists (ping-pong), compaction block counts, device count
    Buf ad_in, ad_bits, ad_pm, ad_sflags; // a later stage's gathered input and outputs
    // SC-Flip (POLAR_ALGO_SCF): flip budget T (polar_scf_set_flips), the failing frames' flip positions, pass B's pairs
    int scf_T = 8;
    Buf scf_flips, scf_pass, scf_bits;
    // its dynamic rule (polar_scf_set_dynamic): order (0: the static rule), budgets T_2, T_3 (T_1 is scf_T), c and tau; the
    // flip sets of the level that runs and of the next one, the pairs' lists (keys, leaves, lengths), per failing frame
    // whether a pair passed, and the slots of the frames that go on to the next level
    int scf_omega = 0, scf_Tk[3] = {0, 0, 0};
    double scf_c = 0.0, scf_tau = 0.0;
    Buf scf_sets[2], scf_lkey, scf_lpos, scf_lcnt, scf_spass, scf_surv;
    Buf scf_hsets;                        // polar_scf_decode_sets_batch: staging of the reported sets
    // BP list decoding (POLAR_ALGO_BPL): the graphs pi_p[b] (polar_bpl_set_graphs), per graph whether it is the identity,
    // and on the device sigma_p, its inverse, the permuted frozen masks and (with a CRC) the permuted CRC tables; the
    // attempts' round trips per open frame, and graph / total_iters of the host-pointer entry points.  The open-frame lists
    // and the gathered rows are the ad_* buffers above
    std::vector<int> bpl_perms;           // [P][n]
    std::vector<unsigned char> bpl_ident; // [P]
    DevMem<uint16_t> d_bpl_sigma, d_bpl_sinv;   // [P][N]
    DevMem<uint32_t> d_bpl_frozen;        // [P][NW]
    DevMem<uint32_t> d_bpl_crc;           // [P][N] or empty
    Buf bpl_siters, bpl_graph, bpl_total;
    int scan_I = 4;                       // SCAN (POLAR_ALGO_SCAN): iterations (polar_scan_set_iters)
    Buf scan_llr, scan_ext;               // polar_scan_decode_batch: staging of the soft outputs
    // 5G rate matching (polar_create_rm): E, POLAR_RM_* mode (POLAR_RM_NONE: a plain ctx), channel interleaver, its tables
    // (sent-row position of e_k, and the inverse); the recovered rows are the lane's rm_rows
    int rm_E = 0, rm_mode = POLAR_RM_NONE, rm_ibil = 0;
    DevMem<uint16_t> d_rm_ilv, d_rm_ilv_inv;
    Buf genie_rows;                       // polar_construct_batch: one chunk of design rows
    // dynamic frozen bits (polar_create_dyn): positions (ascending), dense constraint rows [D][NW] and the row index of
    // every leaf (-1: not dynamic) on the device
    bool is_dyn = false;
    std::vector<int> dyn_pos;
    DevMem<uint32_t> d_dyn_mask;
    DevMem<int> d_dyn_row, d_dyn_pos;
    // encoder side (polar_encode_device, polar_payload_device, polar_set_systematic): i with I[i] = j per position
    // (0xFFFF = frozen), D^i mod g(D) for i < A, both built on first use; the two CRC tables of CA-SCL / SC-Flip (the plain
    // one of make_crc_table and the systematic-mode one, whichever is live sits in d_crc_tab); scratch rows of the encoder
    bool sys_polar = false;
    DevMem<uint16_t> d_enc_inv;
    DevMem<uint32_t> d_enc_rtab;
    std::vector<uint32_t> h_crc_tab_sys;
    Buf enc_u, enc_x, enc_io;
    // fixed-point min-sum (dtype POLAR_Q8): the quantiser (polar_q8_set_quant) and the int32 metrics behind the double d_pm
    // of the float entry points; their quantised rows are the lane's q8_rows
    double q8_scale = 2.0;
    int q8_qc = 8, q8_qi = 8;
    Buf q8_pm;
    Buf in2[2], bits2[2];                // chunked host pipeline: ping-pong device buffers
    PinnedMem<uint32_t> h_bits[2];       // pinned host copies of the packed decisions
    PinnedMem<double> h_in[2];           // pinned staging of the caller's (pageable) input chunks, big batches only
    Buf gen_llr, gen_u, gen_cnt;          // polar_fer_batch
    std::string last_error;
    std::string kernel_name;
    // kernel selection overrides, set only through include/polar_hip_testing.h (cross-checks of the tuned kernels)
    bool force_generic = false;
    bool use_fast2 = true;      // false: one codeword per wavefront (k_scl_fast) instead of two at N = 1024
    bool use_fast4 = false;     // four codewords per wavefront (k_scl_fast4) at N = 1024
    bool force_spill = false;   // no tuned L = 8 kernel; with force_generic: the global-scratch variant of k_scl_generic
    int big_split = 0;          // 35 | 46 | 57: LDS / scratch split of k_scl_big; 0 = the measured best
    size_t chunk_bytes = kChunkBytes;   // bytes of rows per pass of the chunked loops (chunk_rows, polar_hip.hip)
    int resident_blocks = 0;    // at most this many blocks per launch (cap_grid below); 0: the launcher's own choice
    struct {
        int grid;
        long long jobs;
        int jobs_per_block;
        int queued;
    } last_plan{};              // what record_plan() saw last (polar_testing_last_plan)
    struct {
        int grid;
        long long need;
    } last_stride{};            // what stride_grid() saw last (polar_testing_last_stride)
    // list output (polar_list_decode): the D = 0 constraint tables a ctx without dynamic bits runs k_scl_list with
    // (row = -1 at every leaf, one zero mask row), built on first use; staging of polar_list_decode_host, and of
    // polar_list_trace_host (u in list_paths, loss_leaf in list_cnt, loss_rank in list_rem, rank and chosen in list_pm)
    DevMem<uint32_t> d_list_mask;
    DevMem<int> d_list_row;
    Buf list_paths, list_pm, list_rem, list_cnt;
};

// c's lane <-> c->lane_b: work enqueued through c afterwards runs on the other stream with the other stream's buffers
inline void swap_lane(polar_ctx *c) { std::swap(static_cast<Lane &>(*c), c->lane_b); }

// c works on its other lane while this object lives, and on its own again on every way out of the scope
struct OtherLane {
    polar_ctx *c;
    explicit OtherLane(polar_ctx *ctx) : c(ctx) { swap_lane(c); }
    ~OtherLane() { swap_lane(c); }
    OtherLane(const OtherLane &) = delete;
    OtherLane &operator=(const OtherLane &) = delete;
};

// Every entry point that allocates or launches runs on the ctx's device whatever the calling thread had current,
// and leaves the thread's current device as it found it.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

inline int fail(polar_ctx *c, hipError_t e, const char *what)
{
    if (c) c->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return POLAR_EDEVICE;
}

#define HIP_TRY(c, expr)                                   \
    do {                                                   \
        hipError_t e_ = (expr);                            \
        if (e_ != hipSuccess) return fail(c, e_, #expr);   \
    } while (0)

inline int ensure(polar_ctx *c, Buf &b, size_t bytes)
{
    if (b.cap >= bytes) return POLAR_OK;
    if (b.p) HIP_TRY(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    HIP_TRY(c, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return POLAR_OK;
}

// ensure() where the caller chooses the size freely (encoder rows, SCAN scratch, the groups' receive buffers): running out
// of device memory is POLAR_ENOMEM, the runtime's error is cleared and the ctx stays usable; any other failure is
// POLAR_EDEVICE.
inline int ensure_nomem(polar_ctx *c, Buf &b, size_t bytes, const char *what)
{
    if (b.cap >= bytes) return POLAR_OK;
    if (b.p) HIP_TRY(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        b.p = nullptr;
        c->last_error = std::string(what) + ": out of device memory";
        return POLAR_ENOMEM;
    }
    if (e != hipSuccess) return fail(c, e, what);
    b.cap = bytes;
    return POLAR_OK;
}

// Work queue of a persistent kernel.  The resident wavefronts take their first job by their index and every further one
// from a counter (atomic add), so a wavefront that gets fewer issue slots simply takes fewer jobs: a launch ends when the
// work does, not when the slowest statically assigned wavefront does.  One counter per scratch buffer
// (the buffer and its counter belong to one stream at a time); the kernel leaves it at zero (polar_params.h job_fetch).
inline int work_queue(polar_ctx *c, Buf &scratch, unsigned **counter)
{
    if (!scratch.queue) {
        HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&scratch.queue), 256));
        HIP_TRY(c, hipMemsetAsync(scratch.queue, 0, 256, c->stream));
    }
    *counter = scratch.queue;
    return POLAR_OK;
}

// The test-only cap on the resident grid (include/polar_hip_testing.h, polar_testing_resident_blocks): every launcher whose
// kernel loops over its jobs, by the work queue (plan_launch) or by a fixed stride (stride_grid), passes its grid through
// here, so that a few dozen frames reach a wavefront's second and later jobs.  Launchers with one thread per element and no loop (k_q8_quantize,
// k_q8_pm_f64, the encoder kernels, k_list_select / k_list_gather, the compaction of adaptive CA-SCL) do not.
inline long long cap_grid(const polar_ctx *c, long long grid)
{
    if (c->resident_blocks) grid = std::min<long long>(grid, c->resident_blocks);
    return std::max<long long>(grid, 1);
}

// Grid of a launcher that sizes it itself for a kernel that loops by a fixed stride: the `need` blocks of the work, at most
// `limit` (what the launcher allows itself) and at most the cap; kept for polar_testing_last_stride (need > grid: the loop
// makes a second trip)
inline int stride_grid(polar_ctx *c, long long need, long long limit)
{
    const long long grid = cap_grid(c, std::min(need, limit));
    c->last_stride = {(int)grid, need};
    return (int)grid;
}

// The plan of a decoder kernel's launch, kept for polar_testing_last_plan
inline void record_plan(polar_ctx *c, long long grid, long long jobs, int jobs_per_block, bool queued)
{
    c->last_plan = {(int)grid, jobs, jobs_per_block, queued ? 1 : 0};
}

// Launch of a persistent kernel: as many blocks as are resident at once (or as the jobs need, if fewer), each block's
// slice of c->scratch, and the work queue when there are more jobs than the resident blocks take by their index.  A
// k_*.hip launcher states what is particular to its kernel in a LaunchShape; plan_launch() does the rest.
struct LaunchShape {
    int threads;                        // block size
    size_t lds;                         // dynamic LDS bytes per block
    long long jobs;                     // codewords, or groups of 2 / 4 / 64 of them: what one wavefront (or block) takes at a time
    int jobs_per_block;
    size_t scratch_per_block = 0;       // bytes of c->scratch per block; 0: the kernel uses none
    int occ_cap = 0;                    // at most this many blocks per CU; 0: what fits
    long long grid_cap = 0;             // at most this many blocks; 0: no limit
    bool set_lds_attr = true;           // raise the kernel's dynamic-LDS limit to lds first
    bool use_queue = true;              // false: fixed stride even with more jobs than resident slots
    const char *nomem_what = nullptr;   // set: c->scratch grows with ensure_nomem(..., nomem_what), else with ensure()
};
struct LaunchPlan {
    int grid;
    void *scratch;     // c->scratch.p, or null without scratch_per_block
    unsigned *queue;   // the counter of c->scratch, or null: every job has a resident slot
};

inline int plan_launch(polar_ctx *c, const void *kern, const LaunchShape &s, LaunchPlan *out)
{
    if (s.set_lds_attr) HIP_TRY(c, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds));
    int occ = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, s.threads, s.lds));
    if (occ < 1) occ = 1;
    if (s.occ_cap && occ > s.occ_cap) occ = s.occ_cap;
    long long grid = std::min<long long>((s.jobs + s.jobs_per_block - 1) / s.jobs_per_block, (long long)occ * c->num_cu);
    if (s.grid_cap) grid = std::min(grid, s.grid_cap);
    grid = cap_grid(c, grid);
    const bool queued = s.use_queue && s.jobs > grid * s.jobs_per_block;
    record_plan(c, grid, s.jobs, s.jobs_per_block, queued);
    *out = LaunchPlan{(int)grid, nullptr, nullptr};
    if (s.scratch_per_block) {
        const size_t bytes = s.scratch_per_block * (size_t)grid;
        int rc = s.nomem_what ? ensure_nomem(c, c->scratch, bytes, s.nomem_what) : ensure(c, c->scratch, bytes);
        if (rc) return rc;
        out->scratch = c->scratch.p;
    }
    if (queued) return work_queue(c, c->scratch, &out->queue);
    return POLAR_OK;
}

// Launchers exported by the kernel translation units.  r32 / in32: arithmetic type / input type is float (else double).
namespace polar_tu {
int scl_generic(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32);             // k_generic.hip (uses c->logL, c->force_spill)
int scl_big_f64(polar_ctx *c, const polar::SclParams &P, bool in32);                       // k_big_f64.hip
int scl_big_f32(polar_ctx *c, const polar::SclParams &P, bool in32);                       // k_big_f32.hip
int sc_lanes(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32);                // k_sc.hip
int scl_fast(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32, bool crc);      // k_fast.hip: N = 128, N = 1024 one codeword per wave
int scl_fast2(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32, bool crc);     // k_fast2.hip: N = 1024, two per wave (headline)
int bp(polar_ctx *c, const polar::BpParams &P, bool r32, bool in32);                       // k_bp.hip
enum { BP_R4, BP_W128, BP_PLAIN };   // bp()'s kernel for this ctx: k_bp_r4, k_bp_w128, or k_bp / k_bp_global
int bp_variant(const polar_ctx *c);                                                        // k_bp.hip
int bp_readout(polar_ctx *c, const polar::BpReadoutParams &P, bool r32, bool in32);        // k_bp.hip
// k_adaptive.hip: the glue of the adaptive CA-SCL decoder (adaptive_kernel.h)
int ad_crc_check(polar_ctx *c, const uint32_t *d_bits, const uint32_t *d_crc_tab, uint32_t *d_flags, size_t B);   // CRC syndrome of packed decisions
size_t ad_blocks(size_t n);                                                               // compaction blocks for n frames
int ad_compact(polar_ctx *c, const uint32_t *d_flags, const uint32_t *d_idx_in, size_t n, uint32_t need, uint32_t *d_blk,
               uint32_t *d_idx_out, uint32_t *d_count);   // frames with (flags & need) != need; d_blk: 2 * ad_blocks(n) words
int ad_gather(polar_ctx *c, const void *d_src, void *d_dst, const uint32_t *d_idx, size_t n, size_t row_bytes);
int ad_scatter(polar_ctx *c, const uint32_t *s_bits, const double *s_pm, const uint32_t *s_flags, const uint32_t *d_idx,
               size_t n, uint32_t *d_bits, double *d_pm, uint32_t *d_flags, uint32_t *d_list, int L);
// k_bpl.hip: the glue of the BP list decoder (bpl_kernel.h)
int bpl_gather(polar_ctx *c, const void *d_src, bool in32, void *d_dst, const uint32_t *d_idx, size_t base,
               const uint16_t *d_sigma, size_t n);
int bpl_scatter(polar_ctx *c, const uint32_t *s_bits, const uint32_t *s_iters, const uint32_t *s_flags, const uint32_t *d_idx,
                size_t base, size_t n, const uint16_t *d_sinv, uint32_t need, int p, int P, bool all, uint32_t *d_bits,
                uint32_t *d_iters, uint32_t *d_flags, uint32_t *d_graph, uint32_t *d_total);
// k_scf.hip: SC-Flip (scf_lanes.h); mode = polar::SCF_CHECK | SCF_RECORD | SCF_FLIP, and SCF_RECORD_M | SCF_FLIPSET |
// SCF_FLIPREC of the dynamic rule
int scf_lanes(polar_ctx *c, const polar::ScfParams &P, int mode, bool r32, bool in32);
int scf_resolve(polar_ctx *c, const uint32_t *d_pass, const uint32_t *d_pbits, const uint32_t *d_idx, size_t n, int T,
                uint32_t *d_bits, uint32_t *d_flags, uint32_t *d_attempts);
int scf_resolve_sets(polar_ctx *c, const uint32_t *d_pass, const uint32_t *d_pbits, const uint32_t *d_idx, size_t n, int T,
                     const uint16_t *d_sets_in, int stride, int width, int base, uint32_t *d_bits, uint32_t *d_flags,
                     uint32_t *d_attempts, int32_t *d_sets, uint32_t *d_slot_pass);
int scf_merge(polar_ctx *c, bool r32, const void *d_lkey, const uint16_t *d_lpos, const uint32_t *d_lcnt,
              const uint16_t *d_psets, const uint32_t *d_surv, const uint32_t *d_idx_in, size_t n, int Tk, int Tn,
              uint16_t *d_out_sets, uint32_t *d_idx_out);
// k_rm.hip: 5G rate matching (rm_kernel.h): recovery [B][E] -> [B][N] of the input type, generator [B][E]
int rm_recover(polar_ctx *c, const void *d_in, bool in32, double sigma, size_t B, void *d_out);
int rm_generate(polar_ctx *c, const polar::GenParams &G);
// k_genie.hip: Monte-Carlo construction (genie_lanes.h): leaf-sign counters of genie-aided SC (the ctx's N and dtype), design rows
int genie_count(polar_ctx *c, const void *d_in, bool in32, double sigma, size_t B, unsigned long long *d_counts);
int genie_rows(polar_ctx *c, unsigned long long seed, unsigned long long first_frame, double sigma, size_t B, void *d_out,
               bool out32);
// k_scan.hip: SCAN (scan_lanes.h), 32 <= N <= 1024
int scan_lanes(polar_ctx *c, const polar::ScanParams &P, bool r32, bool in32);
// k_dyn.hip: dynamic frozen bits (scl_dyn.h): SC / SCL / CA-SCL with c->d_dyn_mask / d_dyn_row, the generator with them
int scl_dyn(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32);
int dyn_generate(polar_ctx *c, const polar::GenParams &G);
// k_wide.hip: SCL / CA-SCL with L = 64 / 128 / 256 (scl_wide.h), plain or with c->d_dyn_mask / d_dyn_row (uses c->logL, c->force_spill)
int scl_wide(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32);
// k_enc.hip: the encoder side on packed rows (enc_kernel.h)
int enc_transform(polar_ctx *c, const uint32_t *d_in, const uint32_t *d_in2, bool clear_frozen, size_t B, uint32_t *d_out);
int enc_place(polar_ctx *c, const uint32_t *d_payload, size_t B, uint32_t *d_z);                      // needs d_enc_inv, d_enc_rtab
int enc_extract(polar_ctx *c, const uint32_t *d_z, bool xform, size_t B, uint32_t *d_payload, uint32_t *d_ok);   // d_info_order, d_enc_rtab
int enc_dyn_fill(polar_ctx *c, uint32_t *d_z, size_t B);
int enc_rm_select(polar_ctx *c, const uint32_t *d_x, size_t B, uint32_t *d_e);
int enc_count_sys(polar_ctx *c, const uint32_t *d_uhat, const uint32_t *d_u, size_t B, unsigned long long *d_counters,
                  uint32_t *d_frame_err);
// k_q8.hip: fixed-point min-sum SC / SCL / CA-SCL (scl_q8.h) with the quantiser of c (q8_scale, q8_qc, q8_qi)
int q8_decode(polar_ctx *c, const int8_t *d_q, size_t B, uint32_t *d_bits, int32_t *d_pm, uint32_t *d_flags);
int q8_quantize(polar_ctx *c, const void *d_in, bool in32, double sigma, size_t count, int8_t *d_out);   // count < 2^32 * 256
int q8_pm_f64(polar_ctx *c, const int32_t *d_pm, size_t B, double *d_out);
void q8_quantize_host(const double *in, size_t n, double sigma, double scale, int Cc, int8_t *out);
// k_list.hip: list output (list_kernel.h): the LIST epilogue of scl_generic_body / k_scl_wide with the given constraint
// tables (uses c->logL, c->force_spill), and the three kernels that work on a list
int list_decode(polar_ctx *c, const polar::SclParams &P, const uint32_t *d_mask, const int *d_row, bool r32, bool in32,
                uint32_t *d_paths, double *d_pm, uint32_t *d_rem, uint32_t *d_count);
int list_select(polar_ctx *c, const uint32_t *d_rem, const uint32_t *d_count, size_t B, const uint32_t *d_masks, int M, int32_t *d_idx);
int list_gather(polar_ctx *c, const uint32_t *d_paths, const int32_t *d_idx, int idx_stride, size_t B, uint32_t *d_out);
int list_soft(polar_ctx *c, const uint32_t *d_paths, const double *d_pm, const uint32_t *d_count, const uint32_t *d_rem,
              uint32_t want_rem, int domain, double clamp, size_t B, double *d_out);
// k_trace.hip: sent-path trace (trace_out.h): the list decode of list_decode with the TRACE hook and epilogue, and the reduce
int list_trace(polar_ctx *c, const polar::SclParams &P, const uint32_t *d_mask, const int *d_row, bool r32, bool in32,
               const polar::TraceOut &T);
int trace_count(polar_ctx *c, const int32_t *d_loss_leaf, const int32_t *d_rank, const int32_t *d_chosen, size_t B,
                unsigned long long *d_hist);
// k_book.hip: code books (scl_book.h): c is the book's internal context (the largest member's N, the book's L); P.N / P.n
// are that member's, K names the descriptors, the frames' code indices and the input's row stride
int book_decode(polar_ctx *c, const polar::SclParams &P, const polar::BookArgs &K, bool r32, bool in32);
int book_list(polar_ctx *c, const polar::SclParams &P, const polar::BookArgs &K, bool r32, bool in32, uint32_t *d_paths,
              double *d_pm, uint32_t *d_rem, uint32_t *d_count);
#ifdef POLAR_TESTING
int scl_fast4(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32, bool crc);     // k_fast4.hip (libpolar_hip_testing.so only)
#endif
}  // namespace polar_tu
