/*
 * polar_hip_testing.h -- TEST-ONLY entry points of libpolar_hip.so.
 *
 * Not part of the drop-in boundary (include/polar_hip.h): nothing here corresponds to a reference interface.
 * The parity tests use these to run the SAME inputs through every kernel that can decode a configuration
 * (the tuned kernel polar_create picks, and the slower ones it would pick for other shapes) and to put single
 * operands through the kernels' check-node / metric arithmetic.  The product never calls them; the library reads
 * no environment variable.
 */
#ifndef POLAR_HIP_TESTING_H
#define POLAR_HIP_TESTING_H

#include "polar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which kernel a list / SC context launches */
#define POLAR_TEST_KERNEL_AUTO 0           /* polar_create's choice (default)                                      */
#define POLAR_TEST_KERNEL_GENERIC 1        /* k_scl_generic, every LLR level in LDS (if it fits, else as 2)          */
#define POLAR_TEST_KERNEL_GENERIC_SPILL 2  /* k_scl_generic, every LLR level in global scratch                       */
#define POLAR_TEST_KERNEL_BIG 3            /* k_scl_big (N >= 512, L >= 2) also where a tuned L = 8 kernel exists    */
#define POLAR_TEST_KERNEL_ONE_PER_WAVE 4   /* N = 1024, L = 8: k_scl_fast (one codeword per wavefront), not the pair */
#define POLAR_TEST_KERNEL_FOUR_PER_WAVE 5  /* N = 1024, L = 8: k_scl_fast4 (four codewords per wavefront)            */
int polar_testing_select_kernel(polar_ctx *ctx, int variant);

/* k_scl_big: LLR levels <= TL and partial-sum levels <= TB in LDS, written as the two digits TL TB:
 * 35, 46 or 57; 351 / 371 = 35 / 37 with LLR level 4 in the registers of the path's own lanes (L = 32 only; elsewhere 35);
 * 0 = the measured best for the arithmetic type and list size. */
int polar_testing_big_split(polar_ctx *ctx, int split);

/* Seven host loops cut a batch into passes of at most 256 MiB of rows and offset every input, output and list pointer per
 * pass (q8 rows, rate-matched rows, the later stages of adaptive CA-SCL, SC-Flip's pass B and the levels of its dynamic
 * rule, BP list attempts, polar_construct_batch).  At that size a second pass needs batches no model can follow.  This
 * sets the cap in bytes for ctx (and its stage contexts), so that the tests reach the second and later passes with a few
 * hundred short frames; each loop's own floor (64 rows, or 1 frame for the SC-Flip loops) still holds.  0 restores
 * 256 MiB.  The kernels and what they compute per frame do not depend on it. */
int polar_testing_chunk_bytes(polar_ctx *ctx, size_t bytes);

/* Every decoder kernel is persistent: a launch starts as many blocks as stay resident at once, a wavefront (or block) takes
 * its first job by its index and every further one from a counter.  On an MI355X that resident set is thousands of
 * wavefronts, so a second job on the same wavefront needs batches no model can follow.  This caps the grid of every launch
 * of ctx (and of its stage contexts) whose kernel loops over its jobs, by the work queue or by a fixed stride, at `blocks`
 * blocks, so that a few dozen frames reach the second, third and ragged last job.  Kernels with one thread per element and
 * no loop keep their grid.  0 restores the library's own choice.  What a kernel computes per frame does not depend on it. */
int polar_testing_resident_blocks(polar_ctx *ctx, int blocks);

/* The most recent launch plan of a decoder kernel of ctx (plan_launch(), and the two fixed-stride BP launchers): its grid, its
 * jobs (codewords, or groups of 2 / 4 / 64 of them), the jobs a block takes at a time, and whether the kernel was handed the
 * work queue (jobs > grid * jobs_per_block on a kernel that uses it).  Adaptive CA-SCL copies the plan of a stage context here
 * after each stage: a batch that ends at a stage leaves that stage's plan.  Any of the four pointers may be NULL. */
int polar_testing_last_plan(const polar_ctx *ctx, int *grid, long long *jobs, int *jobs_per_block, int *queued);

/* The most recent launch of ctx whose launcher sizes the grid itself for a kernel that loops by a fixed stride (k_bp_global,
 * k_bp_readout, k_rm_recover, the generators, k_genie_rows, k_count_errors, the SC-Flip, adaptive and BPL glue): its grid and
 * the blocks the work needs; need > grid means that the loop made a second trip.  Either pointer may be NULL. */
int polar_testing_last_stride(const polar_ctx *ctx, int *grid, long long *need);

/* The kernels' scalar arithmetic on caller-chosen operands, one thread per element, through the SAME device
 * functions the decoders inline (csrc/polar_math.h, csrc/polar_lut.h):
 *   op 0  chk(a, b)        compare chain, CHK of SCL_1024.c:343-374
 *   op 1  chk_lut(a, b)    table form (one compare per look-up)
 *   op 2  chk_lut1(a, b)   table form, one LDS round trip
 *   op 3  tabv(|a|)        T of SCL_1024.c:352-359 from the table      (b ignored)
 *   op 4  phi(a, u = (b != 0))      compare chain, PHI of SCL_1024.c:481-502
 *   op 5  phi_lut(a, u = (b != 0))  the form the list kernels inline: tabv(a) + max(+-a, 0)
 *   op 6  chk_cnt(a, b)    staircase counted on the VALU from the signs of |x| - threshold
 *   op 7  chk_idx(a, b)    prefix popcount over 26 cells + one threshold read (the BP kernel)
 *   op 8  chk_tab(a, b)    the same with the prefix count read from a byte table (measured alternative, not used)
 * is_f32 = 0: a, b, out are double[n]; 1: float[n].  Host pointers. */
int polar_testing_math(int op, int is_f32, const void *a, const void *b, void *out, size_t n, int device);

#ifdef __cplusplus
}
#endif
#endif
