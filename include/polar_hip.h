/*
 * polar_hip.h -- C ABI of libpolar_hip.so: MI355X-native (gfx950) polar decoders.
 *
 * Drop-in boundary for the per-frame decode functions of CHEBSB/PolarDecoding.  The reference has no
 * plugin/FFI layer; its boundary is a C function symbol plus file-scope globals:
 *
 *     void SCdecode (double *y, int *u_hat);   SC_128.c:78, :395     (N,K,n #define; std, inI[] global)
 *     void BP       (double *y, int *u_hat);   BP_1024.c:114, :372   (+ iterMax)
 *     void SCLdecode(double *y, int *u_hat);   SCL_1024.c:134, :547  (+ L; PM, PMcand, surviv global)
 *     void CASCL    (double *y, int *u_hat);   CASCL_1024_L8.c:141, :601 (+ r, CRC taps inline)
 *
 * Every entry point below names the reference interface it replaces.  Plain pointers and sizes only;
 * no C++ or torch types.  All functions return 0 on success or a negative POLAR_E* code; nothing is
 * printed (the reference's printf diagnostics "Oops!" / "Wrong propagation order!" / "Error!",
 * SCL_1024.c:418, :622, :651, become the per-frame flags word).
 *
 * Thread-safety: a polar_ctx is bound to one GPU and one HIP stream and is not re-entrant (neither is
 * the reference: all its scratch is global).  Use one ctx per host thread / per GPU.
 */
#ifndef POLAR_HIP_H
#define POLAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* algo */
#define POLAR_ALGO_SC 0    /* SCdecode   SC_128.c:395-460                      */
#define POLAR_ALGO_BP 1    /* BP         BP_1024.c:372-427                     */
#define POLAR_ALGO_SCL 2   /* SCLdecode  SCL_1024.c:547-680                    */
#define POLAR_ALGO_CASCL 3 /* CASCL      CASCL_1024_L8.c:601-761               */
#define POLAR_ALGO_SCF 4   /* CRC-aided SC-Flip (no reference counterpart; polar_scf_set_flips below) */
#define POLAR_ALGO_SCAN 5  /* soft-output SCAN (no reference counterpart; polar_scan_set_iters below) */
#define POLAR_ALGO_BPL 6   /* BP list decoding over permuted factor graphs (polar_bpl_set_graphs below) */

/* dtype: the arithmetic type the message passing runs in */
#define POLAR_F64 0 /* IEEE binary64 like the reference: bit-identical decisions (the parity gate) */
#define POLAR_F32 1 /* binary32: same operation order, FER-equivalent, not bit-identical           */
#define POLAR_Q8 2  /* fixed-point min-sum on int8 LLRs (SC / SCL / CA-SCL, N <= 1024): the section below */

/* error codes */
#define POLAR_OK 0
#define POLAR_EINVAL (-1)   /* bad argument / unsupported configuration        */
#define POLAR_ENOMEM (-2)   /* host or device allocation failed                */
#define POLAR_EDEVICE (-3)  /* HIP runtime error (see polar_last_error)        */
#define POLAR_ENOKERNEL (-4)/* no kernel instantiation for this (N, L, dtype)  */

/* per-frame flags word */
#define POLAR_FLAG_TIE 0x1u      /* a median tie occurred (reference prints "Oops!", SCL_1024.c:621-622) */
#define POLAR_FLAG_CRC_PASS 0x2u /* CASCL: the chosen path passed the CRC (CASCL_1024_L8.c:738-746); SCF: an attempt did */
#define POLAR_FLAG_RERANK 0x4u   /* diagnostic, no reference counterpart: at some information leaf the high 32 bits of
                                    the 2L candidate metrics did not single out L survivors and the kernel ranked on
                                    the full doubles (f64 list kernels that pre-rank on 32-bit keys; same result either
                                    way -- the bit lets the tests see that rare path run)                              */
#define POLAR_FLAG_BP_CONVERGED 0x8u /* BP: the stop criterion held at the last round trip run (polar_bp_set_stop)       */

typedef struct polar_ctx polar_ctx;

/* Replaces the reference's compile-time configuration (#define N K n L r iterMax, CASCL_1024_L8.c:16-21;
 * the Q-table derived I[] / inI[], :209-217; the CRC taps written inline at :253-265 and :581-593). */
typedef struct polar_cfg {
    int N;                 /* block length, power of two, 32..4096 (BP above 1024: the messages no longer fit one
                              CU's LDS and live in global scratch -- complete, not fast)                     */
    int K;                 /* payload bits                                                               */
    int crc_r;             /* CRC length r (0 = none)                                                    */
    const int *crc_taps;   /* exponents of g(D) incl. 0 and r, e.g. {0,5,6} (CASCL_128.c:212-214)        */
    int n_taps;
    int L;                 /* list size, power of two 1..32 (SC: 1); SCL / CA-SCL in F64 / F32 also 64,  *
                            * 128, 256 while N * L <= 65536 ("Wide lists" below)                          */
    int algo;              /* POLAR_ALGO_*                                                               */
    int bp_iters;          /* BP round trips (reference: iterMax = 100, BP_1024.c:16)                    */
    const int *info_order; /* I[0..K+crc_r): unfrozen positions in reliability order (I[i] = Q[N-(K+r)+i]).
                              NULL -> built from the 5G sequence like the reference does.                 */
    int dtype;             /* POLAR_F64 | POLAR_F32 | POLAR_Q8                                           */
    int device;            /* HIP device ordinal                                                         */
    int crc_systematic;    /* 0: the CRC word is v(D) g(D) (CASCL_1024_L8.c:251-266).  1: CASCL_1024_sys.c:
                              systematic cyclic encoding, w[0..r) = D^r v(D) mod g, w[r..K+r) = v (:776-789), and
                              the error counters look at the K payload bits only (:820-821).  The decoder is the
                              same: that program's bit-reversed graph fed with y[bRev[j]] makes the decisions of
                              the natural-order graph fed with y.  Used by polar_generate_device,
                              polar_count_errors_device and polar_fer_batch; ignored without a CRC.            */
} polar_cfg;

int polar_create(const polar_cfg *cfg, polar_ctx **out);
void polar_destroy(polar_ctx *ctx);
const char *polar_strerror(int code);
/* text of the last HIP error seen by this ctx ("" if none) */
const char *polar_last_error(const polar_ctx *ctx);

/* --- CRC generator-matrix file ------------------------------------------------------------------------
 * The reference's CRC_6.dat (K = 64 rows x r = 6 entries, 0/1; row i = D^(r+i) mod g(D), column j = coefficient of
 * D^j; UTF-16LE with BOM, CRLF, single spaces, no final newline) and, in the same layout, the literal
 * `const int Gc[K][r]` of CASCL_1024_sys.c:48-561 that its systematic encoder sums at :776-789.  The loader takes
 * the file's encoding as it is (also UTF-8 / ASCII, also with the braces and commas of the C literal), derives
 * g(D) = D^r + row 0 and REJECTS the file (POLAR_EINVAL) unless every row i equals D^(r+i) mod g, g has a D^0
 * term, all rows have the same 1..32 entries and every entry is 0 or 1. */
typedef struct polar_crc_matrix {
    int K;            /* rows = payload bits the matrix serves                                     */
    int r;            /* columns = CRC length                                                      */
    int n_taps;       /* number of exponents of g(D)                                               */
    int taps[33];     /* exponents of g(D), ascending, incl. 0 and r: what polar_cfg.crc_taps wants */
    uint32_t *rows;   /* [K] bit j of rows[i] = entry (i, j); malloc'ed, release with ..._free     */
} polar_crc_matrix;
int polar_crc_matrix_load(const char *path, polar_crc_matrix *out);
void polar_crc_matrix_free(polar_crc_matrix *m);
/* writes the K x r matrix of g(D) in the reference's encoding, byte for byte what CRC_6.dat holds for K = 64, {0,5,6} */
int polar_crc_matrix_save(const char *path, int K, const int *taps, int n_taps);
/* polar_create with r and g(D) taken from such a file (cfg->crc_r / crc_taps / n_taps are ignored; cfg->algo must be
 * POLAR_ALGO_CASCL or POLAR_ALGO_SCF; cfg->K <= the file's row count).  cfg->crc_systematic = 1 is the encoder the matrix belongs to. */
int polar_create_crc_file(const polar_cfg *cfg, const char *path, polar_ctx **out);

/* --- reference-shaped single-frame call -------------------------------------------------------------
 * Identical result to  std = sigma; X(y, u_hat);  for X = SCdecode / BP / SCLdecode / CASCL
 * (SCL_1024.c:263: the per-frame call in main()).  y: N channel observations (not LLRs: the LLR
 * 2*y/std/std is formed inside, SCL_1024.c:574-578).  u_hat: N ints, fully overwritten, frozen = 0. */
int polar_decode(polar_ctx *ctx, const double *y, double sigma, int *u_hat);

/* --- north-star call shape: decode(llr_in, frozen_mask, N, L) ----------------------------------------
 * One frame of channel LLRs and a frozen mask (1 = frozen; the reference's !inI[], SCL_1024.c:198-206).
 * Plain SCL (L > 1) or SC (L == 1) in f64.  Contexts are cached per (N, L, mask). */
int polar_decode_llr(const double *llr_in, const unsigned char *frozen_mask, int N, int L, int *u_hat);

/* --- batched, host buffers ---------------------------------------------------------------------------
 * B frames.  llr_in [B][N] row-major channel LLRs (double).  frozen_mask: NULL (use cfg) or [N] override
 * for SC/BP/SCL (CASCL needs cfg's info_order for the CRC).  u_hat [B][N] ints 0/1.
 * pm_out (nullable) [B]: metric of the chosen path (SCL/CASCL; 0 otherwise).  flags (nullable) [B]. */
int polar_decode_batch(polar_ctx *ctx, const double *llr_in, const unsigned char *frozen_mask, size_t B,
                       int *u_hat, double *pm_out, unsigned *flags);

/* Same, but the input is channel observations y and the kernel forms 2*y/sigma/sigma on load
 * (SCL_1024.c:576, operation order kept). */
int polar_decode_batch_y(polar_ctx *ctx, const double *y, double sigma, size_t B, int *u_hat,
                         double *pm_out, unsigned *flags);

/* --- batched, device buffers (the measured path; asynchronous on the ctx stream) ---------------------
 * d_in: [B][N] of double (in_is_f32 = 0) or float (in_is_f32 = 1), LLRs, or y when sigma > 0.
 * d_uhat_bits: [B][N/32] uint32, bit (j & 31) of word j >> 5 = u_hat[j].
 * d_pm (nullable): [B] double.  d_flags (nullable): [B] uint32.
 * Input rows -- the one rule for every entry point that takes `d_in, in_is_f32` (each refers to this paragraph).  With R the
 * arithmetic type of the ctx (cfg.dtype) and row the frame's N values, the decoder works on
 *     v = (double)row[i];  if (sigma > 0) v = 2 * v / sigma / sigma;  working value = (R)v
 * for every i: the conversion and both divisions are done in double, in that order (SCL_1024.c:576), and the result is rounded
 * once to R.  A float row on an F64 ctx is therefore exact, a double row on an F32 ctx is rounded once, and a y row is never
 * scaled in float.  (A Q8 ctx quantises v instead: rule 1 of its section.)
 * d_in needs the alignment of its element type only (4 bytes for float, 8 for double): rows need not start on a 16-byte
 * boundary, and a kernel that reads several elements at once does so only after testing the address.  No result depends on
 * anything outside the B rows.
 * The kernel that runs may depend on in_is_f32, while the result obeys the rule above all the same: an F64 ctx with L = 8 on
 * float rows does not run its tuned kernel but k_scl_big<double, float> at N = 1024 (instead of k_scl_fast2) and
 * k_scl_generic<double, float> at N = 128 (instead of k_scl_fast); polar_kernel_name names the kernel for rows of the ctx's own
 * type.  tests/input_forms.py lists a case per kernel, tests/test_gpu_input_forms.py holds each to the rule. */
int polar_decode_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B,
                        uint32_t *d_uhat_bits, double *d_pm, uint32_t *d_flags);

/* --- error accounting on device (main()'s compare loop, CASCL_1024_L8.c:296-305) ---------------------
 * d_u_bits: [B][N/32] transmitted u.  Adds to d_counters[0] (block errors) and d_counters[1] (bit errors on
 * the K + r unfrozen positions).  d_frame_err (nullable): [B] uint32 bit errors per frame (needed to cut at
 * the reference's sequential stop rule). */
int polar_count_errors_device(polar_ctx *ctx, const uint32_t *d_uhat_bits, const uint32_t *d_u_bits, size_t B,
                              unsigned long long *d_counters, uint32_t *d_frame_err);

/* --- the sequential stop rule on a batch (`for (run = 0; errBlock < BLE; run++)`, SCL_1024.c:228, :264-275) -------
 * The reference ends an Eb/N0 point WITH the frame that brings the block errors to BLE; generator state and PN phase
 * carry on from there.  For a batch decoded as a whole that is a prefix count over polar_count_errors_device's
 * d_frame_err, done on the device: d_out[0] = frames consumed (position of the `need`-th erroneous frame + 1, or B if
 * the batch holds fewer), d_out[1] / d_out[2] = block / bit errors among the consumed frames.
 * min_frames: the rule behind the published L = 32 logs (myResult_1024.zip:CASCL_L32.dat, "error block = 487 run =
 * 2000"), `errBlock < BLE || run < 2000`: consume at least min_frames frames (0 = the plain rule); with
 * min_frames > 0, need may be 0 (BLE already reached, the minimum not yet). */
int polar_stop_rule_cut_device(polar_ctx *ctx, const uint32_t *d_frame_err, size_t B, unsigned need, size_t min_frames,
                               unsigned long long *d_out /* [3] */);

/* Host-buffer form, one iteration of main()'s loop over a batch: y [B][N] observations, sigma = std, u_bits [B][N/32]
 * the sent u packed like the decisions.  Decode, compare on the unfrozen positions (:266-272; payload only with
 * crc_systematic) and cut, all on the device; only three numbers come back. */
int polar_stop_rule_batch_y(polar_ctx *ctx, const double *y, double sigma, const uint32_t *u_bits, size_t B,
                            unsigned need, size_t min_frames, size_t *consumed, unsigned long long *block_errors,
                            unsigned long long *bit_errors);

/* --- BP with per-stage read-outs (BPr_128.c:373-575: `BPr(y, u_hat, u)` and its table E[7][n+1]) -----------------
 * ctx must be a POLAR_ALGO_BP context (its bp_iters = the program's iterMax, 90 in BPr_128.c:16).  After each of the
 * iteration counts checkpoints[0..ncp) (ascending, <= 8; the program uses 3, 6, 10, 20, 40, 80, :18-23) the hard
 * decisions of l + r at every stage i = 0..n are carried back to the u side and compared with the sent bits on the
 * information set; d_E[c*(n+1) + i] accumulates the mismatches over the B frames (the program's E[c][i], :437).
 * d_u_bits: [B][N/32] sent bits; d_uhat_bits (may be NULL): [B][N/32] final decisions.  N <= 512 (f64), 1024 (f32).
 * d_in: "Input rows" at polar_decode_device. */
int polar_bp_readout_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B,
                            const uint32_t *d_u_bits, const int *checkpoints, int ncp, unsigned long long *d_E,
                            uint32_t *d_uhat_bits);
/* Host-buffer form, the shape of BPr_128.c's frame loop (:213): y [B][N] observations (sigma > 0) or LLRs (sigma = 0),
 * u [B][N] sent bits (0/1 ints), E [ncp][n+1] accumulated (+=), u_hat [B][N] (may be NULL). */
int polar_bp_readout_batch(polar_ctx *ctx, const double *in, double sigma, size_t B, const int *u,
                           const int *checkpoints, int ncp, unsigned long long *E, int *u_hat);

/* --- BP early termination (opt-in; the reference always runs iterMax round trips, BP_1024.c:393) -------------------
 * One round trip t (1-based) is one R sweep followed by one L sweep (BP_1024.c:393-416).  After round trip t:
 *   u_hat_j = the reference's final decision (BP_1024.c:417-425): 0 at a frozen position, else 0 if l[0][j] + r[0][j] >= 0,
 *             else 1;
 *   x_hat_j = 0 if l[n][j] + r[n][j] >= 0, else 1, where l[n] is the channel LLR in the message type and r[n] is what the
 *             R sweep of round trip t writes at stage n (operand order as written).
 * Rule POLAR_BP_STOP_G (the G-matrix criterion of Yuan & Parhi) stops a frame after the first t at which
 * u_hat F^{(x)n} == x_hat over GF(2), F^{(x)n} in natural order (the encoder of SCL_1024.c:242-250); the frame's output is
 * that u_hat.  A frame with no such t <= iterMax runs iterMax round trips and its output is exactly that of
 * POLAR_BP_STOP_NONE.  The rows the check reads (r[n], l[0]) are read by no message update, so a frame that stops after t
 * has the decisions of the fixed-iteration decoder with bp_iters = t, bit for bit (in f64 those of the reference's BP()
 * with iterMax = t; in f32 the same operations in float).
 * The rule belongs to the ctx and is honoured by polar_decode, polar_decode_batch(_y), polar_decode_device,
 * polar_fer_batch and polar_stop_rule_batch_y; in polar_decode_batch(_y)'s flags it sets POLAR_FLAG_BP_CONVERGED.
 * polar_bp_readout_* return POLAR_EINVAL while a rule is set (their checkpoints need every round trip).  polar_group_* and
 * polar_fer_multi_gpu build their contexts from a polar_cfg and always run POLAR_BP_STOP_NONE. */
#define POLAR_BP_STOP_NONE 0 /* default: iterMax round trips (the reference)                          */
#define POLAR_BP_STOP_G 1    /* stop at the first round trip with u_hat F == x_hat (above)             */
/* POLAR_EINVAL: not a BP ctx, or an unknown rule */
int polar_bp_set_stop(polar_ctx *ctx, int rule);
/* polar_decode_device for a BP ctx, plus per frame: d_iters (nullable) [B] round trips run, d_flags (nullable) [B]
 * POLAR_FLAG_BP_CONVERGED or 0.  With POLAR_BP_STOP_NONE d_iters is filled with iterMax and d_flags with 0.  d_in: "Input rows"
 * at polar_decode_device. */
int polar_bp_decode_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B,
                           uint32_t *d_uhat_bits, uint32_t *d_iters, uint32_t *d_flags);
/* Host-buffer form: llr_in [B][N] LLRs, u_hat [B][N], iters / flags (nullable) [B]. */
int polar_bp_decode_batch(polar_ctx *ctx, const double *llr_in, size_t B, int *u_hat, unsigned *iters, unsigned *flags);

/* --- adaptive CA-SCL (opt-in; Li, Chen and Liu, 2012): re-decode only the CRC-failing frames with larger lists ----------
 * A rule belongs to a POLAR_ALGO_CASCL context, including ones made by polar_create_crc_file and ones with crc_systematic
 * set.  The rule is a list of list sizes stages[0] < stages[1] < ... < stages[m-1] = cfg.L: each stage is a power of two,
 * 1 <= m <= 6, and cfg.L >= 2 whenever m > 1.  Each stage s defines a decision for every frame:
 *   L_s >= 2: the decision, path metric and flags of the fixed CA-SCL decoder of this context with list size L_s -- bit for
 *             bit what polar_create returns with the same cfg and L = L_s.  The frame passes if POLAR_FLAG_CRC_PASS is set.
 *   L_s = 1 (first stage only): the decision of POLAR_ALGO_SC with the same info_order[0 .. K+r), the CRC positions treated
 *             as information bits.  The frame passes if XOR over {j : u_hat_j = 1} of crc_tab[j] is 0 (crc_tab[I[i]] =
 *             D^i mod g(D)), the same test the list kernels apply.  The reported metric is 0.0; the reported flags are the
 *             SC context's flags, with POLAR_FLAG_CRC_PASS added on a pass.
 * A frame's output is the output of the first stage at which it passes.  A frame that passes at no stage takes the output
 * of the last stage (L_max), with its flags, so POLAR_FLAG_CRC_PASS is clear.  A frame that is not re-decoded is never
 * touched again.  The single-stage rule {cfg.L} is exactly the default decoder; so is clearing the rule (n = 0); in both
 * cases no new kernel runs.  dtype POLAR_F32 runs every stage in f32 (compare with the library's own fixed-L f32 contexts).
 * The rule is honoured by polar_decode, polar_decode_batch(_y), polar_decode_device, polar_fer_batch,
 * polar_stop_rule_batch_y and polar_time_decode_device.  polar_group_* and polar_fer_multi_gpu build their contexts from a
 * polar_cfg and always run the default decoder.
 * Between stages the host reads the count of failing frames (one 4-byte copy and a stream sync per stage) and stops after a
 * stage with zero failures; a decode with a rule set while the ctx stream is capturing a graph returns POLAR_EINVAL. */
/* POLAR_EINVAL: not a CA-SCL ctx, or a malformed list.  n = 0 restores the default. */
int polar_cascl_set_stages(polar_ctx *ctx, const int *stages, int n);
/* polar_decode_device for a CA-SCL ctx, plus per frame d_list (nullable) [B]: the list size of the stage that decided it
 * (1 for SC; cfg.L without a rule).  d_pm, d_flags, d_list are nullable.  d_in: "Input rows" at polar_decode_device; a later
 * stage reads the rows of its frames from d_in again. */
int polar_cascl_decode_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B,
                              uint32_t *d_uhat_bits, double *d_pm, uint32_t *d_flags, uint32_t *d_list);
/* Host-buffer form: llr_in [B][N] LLRs, u_hat [B][N]; pm, flags, list (nullable) [B]. */
int polar_cascl_decode_batch(polar_ctx *ctx, const double *llr_in, size_t B, int *u_hat, double *pm, unsigned *flags,
                             unsigned *list);

/* --- CRC-aided SC-Flip (Afisiadis, Balatsoukas-Stimming and Burg, 2014) ---------------------------------------------------
 * A POLAR_ALGO_SCF context takes the cfg of CA-SCL: crc_r >= 1 with its taps (or polar_create_crc_file), crc_systematic
 * honoured by the generator and the error counters; cfg.L is ignored and reported as 1.  32 <= N <= 2048 (N = 4096:
 * POLAR_ENOKERNEL).  With A = K + r unfrozen positions I[0..A) (info_order, as for CA-SCL), flip budget T and the dtype's
 * arithmetic type R, a frame's output is:
 *   1. attempt 0: the decisions of POLAR_ALGO_SC over I[0..A), the CRC positions decoded as information bits.  lambda_j is
 *      the leaf LLR that decides u_hat_j (u_hat_j = 1 iff lambda_j < 0).
 *   2. an attempt passes if XOR over {j : u_hat_j = 1} of crc_tab[j] is 0, crc_tab[I[i]] = D^i mod g(D) (the test of the
 *      list kernels and of the adaptive rule, systematic or not).
 *   3. if attempt 0 passes it is the output, attempts = 0.
 *   4. otherwise the flip list p_1..p_T holds the T positions of I[0..A) with the smallest |lambda_j| of attempt 0, in
 *      ascending |lambda_j| (fabs in R: +0 == -0), ties to the smaller j.
 *   5. attempt t (1 <= t <= T) is SC with the decision at leaf p_t inverted (u_hat = 1 - [lambda < 0] there); every later
 *      leaf uses the inverted bit in its partial sums; nothing else is forced.
 *   6. the output is the first attempt t that passes (attempts = t, POLAR_FLAG_CRC_PASS set); if none passes, attempt 0
 *      with attempts = T and POLAR_FLAG_CRC_PASS clear.
 *   7. the metric (d_pm / pm_out) is 0.0; the flags word is SC's with POLAR_FLAG_CRC_PASS added on a pass.
 * A frame that passes at attempt 0 is never touched again, so the frames SCF decodes wrongly are a subset of those SC does.
 * The decoder is honoured by polar_decode, polar_decode_batch(_y) (no frozen_mask override), polar_decode_device,
 * polar_fer_batch, polar_stop_rule_batch_y, polar_time_decode_device and polar_kernel_name.  polar_group_* and
 * polar_fer_multi_gpu build their contexts from a polar_cfg and run SCF with the default T = 8.
 * The host reads the count of failing frames (one 4-byte copy and a stream sync per decode): a decode while the ctx stream
 * is capturing a graph returns POLAR_EINVAL.  polar_cascl_set_stages refuses SCF contexts. */
/* T: 0 <= T <= min(32, K + r); default 8 (min(8, K + r)).  T = 0 is SC plus the CRC flag.  POLAR_EINVAL (ctx unchanged):
 * not an SCF ctx, or T out of range. */
int polar_scf_set_flips(polar_ctx *ctx, int T);
/* polar_decode_device for an SCF ctx, plus per frame d_attempts (nullable) [B]: the attempt that decided it (0 = plain SC;
 * T when no attempt passed).  d_flags and d_attempts are nullable.  d_in: "Input rows" at polar_decode_device; every attempt
 * reads its frame's row from d_in. */
int polar_scf_decode_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B,
                            uint32_t *d_uhat_bits, uint32_t *d_flags, uint32_t *d_attempts);
/* Host-buffer form: llr_in [B][N] LLRs, u_hat [B][N]; flags, attempts (nullable) [B]. */
int polar_scf_decode_batch(polar_ctx *ctx, const double *llr_in, size_t B, int *u_hat, unsigned *flags,
                           unsigned *attempts);

/* --- Dynamic SC-Flip: flip sets ranked by a metric (Chandesris, Savin and Declercq, 2018; the multiplier-free metric of
 * Ercan, Tonnellier, Doan and Gross, 2020) -----------------------------------------------------------------------------
 * Opt-in on a POLAR_ALGO_SCF context (polar_scf_set_dynamic).  An attempt inverts a SET of up to omega decisions, and the
 * sets are ranked by a metric that charges an early, fairly reliable decision less than |lambda| alone would.
 * A declared departure from the paper: the paper's decoder is serial (one attempt, its extensions into a priority list,
 * pop, repeat: T SC latencies back to back).  Here the rule is layered: all sets of size k of a frame run at once, their
 * extensions are ranked together and give the sets of size k + 1, omega + 1 SC latencies in all.  The sets tried are
 * therefore not the paper's, and neither is the metric's log-sum form (the multiplier-free one is used, reproducible
 * bit for bit).
 * Setting: order omega in {1, 2, 3}, budgets T_1 .. T_omega (each 1 .. 32, T_1 <= A), a penalty c >= 0 and a threshold
 * tau >= 0, finite doubles rounded once to R.  Rules 1-3 and 7 of the section above stay (attempt 0, the CRC test, the
 * untouched passing frames, the metric 0.0, the flags).
 *   1. run(E), E a set of information positions: SC with the decision inverted at every leaf of E (rule 5 above at each
 *      member; later leaves see the inverted bits).  lambda^E_j is the leaf LLR at information leaf j in that run.
 *      run(empty) is attempt 0.
 *   2. counter: cnt^E_i = #{ j in I[0..A) : j <= i and |lambda^E_j| <= tau }, an integer; it covers flipped leaves and i
 *      itself; the comparison is done in R, fabs as in rule 4 above.
 *   3. metric of extending E by an information position i > max(E) (max(empty) = -1):
 *        M(E, i) = (F_E + |lambda^E_i|) + S,  S = c * (R)cnt^E_i,
 *      F_empty absent (M(empty, i) = |lambda_i| + S), F_E the sum of |lambda^E_j| over j in E in ascending j starting
 *      from the first term; every + and the one * rounded once in R, no contraction.  With c = 0, M(empty, i) = |lambda_i|.
 *   4. level-1 list: the T_1 positions i of I[0..A) with the smallest (M(empty, i), i), ascending (c = 0: rule 4 above).
 *   5. level-(k+1) list (k < omega), built only for frames where no attempt of levels <= k passed: with E_0 .. E_{T_k - 1}
 *      the frame's level-k sets in list order, the candidates are all (q, i), i in I[0..A), i > max(E_q); the key is
 *      (M(E_q, i), q, i), lexicographic, lambda taken from run(E_q); the list is the T_{k+1} candidates of smallest key,
 *      ascending; candidate (q, i) stands for the set E_q + {i} (distinct by construction).  Fewer candidates: a shorter list.
 *   6. attempts are numbered globally: rank q (0-based) of level k is attempt T_1 + .. + T_{k-1} + q + 1.
 *   7. the output is the passing attempt of smallest number (attempts = that number, POLAR_FLAG_CRC_PASS, the reported set
 *      is its E); if none passes, attempt 0 with attempts = T_1 + .. + T_omega, the flag clear and an empty set.  A frame
 *      that passes at some level is not run at a later level.
 *   8. identities: omega = 1 with c = 0 is the static decoder above bit for bit, attempts included; with c, tau and T_1
 *      fixed, a frame decoded at level 1 has the same output for every omega, so the wrong frames of (T_1, T_2) are a
 *      subset of those of (T_1).
 *   9. the Python convenience constructor alone defaults to c = 1.5, tau = 5.0 (the constants Ercan et al. give; a choice,
 *      see DESIGN.md 4.6 for what this library measured).  A fresh context runs the static rule.
 * Honoured by everything that honours SCF: polar_decode, polar_decode_batch(_y), polar_decode_device, polar_scf_decode_*,
 * polar_fer_batch, polar_stop_rule_batch_y, polar_time_decode_device, polar_kernel_name, CRC-file, systematic and
 * rate-matched contexts.  polar_group_* and polar_fer_multi_gpu keep running the static default.  The host reads one count
 * per level (a 4-byte copy and a stream sync each); a decode during stream capture stays POLAR_EINVAL. */
#define POLAR_SCF_MAX_ORDER 3
/* budgets[0..omega) = T_1 .. T_omega; budgets[0] becomes T (a later polar_scf_set_flips changes T_1 only).  omega = 0
 * clears the rule and leaves T as it is (budgets, c, tau ignored).  POLAR_EINVAL (ctx unchanged): not an SCF ctx, omega
 * outside 0 .. 3, a budget out of range, c or tau negative or not finite. */
int polar_scf_set_dynamic(polar_ctx *ctx, const int *budgets, int omega, double c, double tau);
/* Every output is nullable.  budgets [3]: T_1 (the ctx's T), T_2, T_3, 0 beyond omega; omega = 0, c = tau = 0: the static rule. */
int polar_scf_get_dynamic(const polar_ctx *ctx, int *omega, int *budgets, double *c, double *tau);
/* polar_scf_decode_device plus d_sets (nullable) [B][3]: the reported set in ascending order, -1 padded (all -1: attempt 0
 * is the output).  On a static ctx it holds at most one entry, the flipped position.  d_flags, d_attempts and d_sets are
 * nullable.  d_in: "Input rows" at polar_decode_device. */
int polar_scf_decode_sets_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B,
                                 uint32_t *d_uhat_bits, uint32_t *d_flags, uint32_t *d_attempts, int32_t *d_sets);
/* Host-buffer form: sets (nullable) [B][3]. */
int polar_scf_decode_sets_batch(polar_ctx *ctx, const double *llr_in, size_t B, int *u_hat, unsigned *flags,
                                unsigned *attempts, int *sets);

/* --- Soft-output SCAN (soft cancellation; Fayyaz and Barry, IEEE JSAC 2014) ----------------------------------------------
 * SCAN is BP's message arithmetic driven by SC's schedule: a serial walk over the tree that carries LLRs upwards instead of
 * hard partial sums, and returns an LLR for every u bit and every code bit.  A POLAR_ALGO_SCAN context takes the cfg of a BP
 * context (crc_r as BP accepts it; cfg.L is ignored and reported as 1; bp_iters is ignored).  32 <= N <= 1024 (above:
 * POLAR_ENOKERNEL).
 * Setting: N = 2^n, a frozen mask, the dtype's arithmetic type R, one row l[0..N) of finite channel LLRs (2*y/sigma/sigma
 * when sigma > 0, as for the other decoders), I >= 1 iterations.
 *   CHK-inf(a, b): if b = +inf the result is a; otherwise, if a = +inf, it is b; otherwise it is the check node chk<R>(a, b)
 *   (csrc/polar_math.h).  This is chk's own value for a finite partner up to the sign of a zero; it is spelled out so that
 *   (+inf, +inf) gives +inf and no inf - inf is ever evaluated.  The only infinity that can arise is +inf, and no
 *   subtraction occurs anywhere in the decoder.
 *   A node at level t covers the leaves s .. s + 2^t - 1, h = 2^(t-1); it receives alpha[0..2^t) and returns beta[0..2^t).
 *   The root is the node at level n with s = 0 and alpha = l.
 *   1. leaf (t = 0): lambda_s = alpha[0]; beta[0] = +inf if leaf s is frozen, else 0.
 *   2. stored state: each right child (t-1, s+h) keeps the beta it returned, for the next iteration.  Before iteration 1
 *      that stored beta is +inf in every element if all of the child's leaves are frozen, and 0 otherwise (a declared
 *      difference from the paper, which starts internal nodes at 0: the stored beta of an all-frozen right child is a
 *      constant that needs no memory; for frozen sets that respect the partial order no decision changes).
 *   3. left child: alpha_l[e] = CHK-inf(alpha[e], alpha[e+h] + beta_r_prev[e]), e < h; beta_l = visit(left child, alpha_l).
 *   4. right child: alpha_r[e] = alpha[e+h] + CHK-inf(alpha[e], beta_l[e]); beta_r = visit(right child, alpha_r); this
 *      beta_r replaces beta_r_prev.
 *   5. upwards: beta[e] = CHK-inf(beta_l[e], beta_r[e] + alpha[e+h]); beta[e+h] = beta_r[e] + CHK-inf(beta_l[e], alpha[e]).
 *   6. one iteration is one visit of the root; iterations 1..I run back to back; the stored right-child betas are the only
 *      state carried over between them.
 *   7. outputs, all from iteration I: u_hat_j = 0 if j is frozen, else [lambda_j < 0]; llr_u[j] = lambda_j at unfrozen j
 *      and +inf at frozen j; ext_x[e] = the root's beta[e], the extrinsic LLR of code bit e (the caller forms
 *      l[e] + ext_x[e]; +inf where the frozen set fixes the bit); the metric is 0.0 and the flags word is 0.
 *   8. every sum and every chk is rounded once in R, no contraction.  Soft outputs are compared by value: the sign of a
 *      zero is not pinned.
 * Consequences a kernel may use (each preserves every value above): an all-frozen subtree returns +inf everywhere and its
 * lambdas are not reported, so it is never entered; an all-information subtree returns exactly 0 everywhere, so it is
 * entered in iteration I only, downwards only (alpha_l = chk(a, b), alpha_r = b); whether an element of a beta is +inf
 * depends on the frozen mask only.
 * The decoder is honoured by polar_decode, polar_decode_batch(_y) (a frozen_mask override works as for SC),
 * polar_decode_device, polar_fer_batch, polar_stop_rule_batch_y, polar_time_decode_device, polar_kernel_name and
 * polar_ctx_info.  On a polar_create_rm context the recovered N-wide row is the input l; ext_x stays N wide, in decoder
 * order.  polar_group_* and polar_fer_multi_gpu run the default I = 4.  polar_bp_*, polar_cascl_*, polar_scf_* and
 * polar_create_crc_file return POLAR_EINVAL on (or for) a SCAN ctx.  A decode that cannot get its scratch memory returns
 * POLAR_ENOMEM and leaves the ctx usable. */
/* I: 1 <= I <= 64; default 4.  POLAR_EINVAL (ctx unchanged): not a SCAN ctx, or I out of range. */
int polar_scan_set_iters(polar_ctx *ctx, int I);
/* d_uhat_bits [B][N/32], d_llr_u and d_ext_x [B][N] of the ctx dtype (double or float); each of the three may be NULL.
 * Asynchronous on the ctx stream, no host read-back: after a warm-up at the same B it can be captured into a graph.
 * d_in: "Input rows" at polar_decode_device. */
int polar_scan_decode_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B,
                             uint32_t *d_uhat_bits, void *d_llr_u, void *d_ext_x);
/* Host-buffer form: llr_in [B][N] LLRs (E per row on a rate-matched ctx); u_hat [B][N], llr_u and ext_x [B][N] of the ctx
 * dtype; each of the three outputs may be NULL. */
int polar_scan_decode_batch(polar_ctx *ctx, const double *llr_in, size_t B, int *u_hat, void *llr_u, void *ext_x);

/* --- BP list decoding over permuted factor graphs (Elkelesh, Ebada, Cammerer and ten Brink, 2018) --------------------------
 * A polar code of length N = 2^n has n! factor graphs, one per ordering of its n stages.  A frame whose messages do not
 * settle on one graph often settles on another.  A permutation of the stages is a permutation of the bits of the position
 * index (Doan, Hashemi, Mondelli and Gross, GLOBECOM 2018), so every attempt below is the BP decoder of this library,
 * unchanged, on a permuted row with a permuted frozen mask.  (The reference's BP_128_fag.c is the graph with the stage order
 * reversed.)
 * Context.  A POLAR_ALGO_BPL context takes the cfg of a BP context, bp_iters = iterMax of one attempt.  A CRC is optional:
 * crc_r = 0 means none; crc_r >= 1 with its taps works as for CA-SCL: A = K + r positions are unfrozen, and the generator and
 * the error counters treat the CRC exactly as they do for POLAR_ALGO_CASCL, crc_systematic included.  (POLAR_ALGO_BP ignores
 * crc_r as before.)  cfg.L is ignored and reported as 1.  dtypes POLAR_F64 and POLAR_F32 and every N the BP kernels take;
 * POLAR_Q8 returns POLAR_ENOKERNEL, as for BP.
 * Graphs.  A graph is a permutation pi of {0 .. n-1}.  It maps positions by
 *       sigma_pi(j) = sum over b of ((j >> b) & 1) << pi[b],
 * which moves index bit b to bit pi[b].  A context holds an ordered list pi_0 .. pi_{P-1}, 1 <= P <= 32.
 * Rules, for a context with frozen mask fz, CRC table crc_tab (crc_tab[I[i]] = D^i mod g(D), the table the list kernels use)
 * and one input row l[0..N) (LLRs, or y with sigma > 0, left as they are):
 *   1. attempt p is POLAR_ALGO_BP with POLAR_BP_STOP_G and the same bp_iters and dtype, run on row_p[j] = l[sigma_p(j)] with
 *      frozen mask fz_p[j] = fz[sigma_p(j)].  It yields decisions u'_p, round trips t_p and converged flag c_p, bit for bit
 *      what a BP context built on that permuted code returns for that row.  Then u_hat_p[sigma_p(j)] = u'_p[j].
 *   2. with sigma > 0 the permutation moves the y values, and the BP kernel forms 2*y/sigma/sigma on load as it does today.
 *   3. crcok_p = (XOR over {j : u_hat_p[j] = 1} of crc_tab[j]) == 0.  It is defined only with a CRC.
 *   4. attempt p is accepted iff c_p, and with a CRC also crcok_p.  An attempt that converges and then fails the CRC is
 *      over: it is not iterated further.
 *   5. the output is the first accepted attempt, graph = p.  If none is accepted the output is attempt 0 with graph = P.  A
 *      frame accepted at attempt p is never touched again.
 *   6. with q the reported attempt (graph, or 0 on fallback): iters = t_q; the flags word has POLAR_FLAG_BP_CONVERGED iff c_q
 *      and POLAR_FLAG_CRC_PASS iff the context has a CRC and crcok_q; total_iters is the sum of t_p over every attempt run
 *      for the frame; the metric is 0.0.
 *   7. identity: P = 1, pi_0 = identity and no CRC is a BP context with POLAR_BP_STOP_G, bit for bit, iters included.
 *   8. if pi_p is the identity, no permutation kernel needs to run for that attempt.
 * Default list: the cyclic shifts pi_s[b] = (b + s) mod n, s = 0 .. P-1, with P = min(n, 8).  This is a choice; no FER stands
 * behind it yet.
 * Honoured by polar_decode, polar_decode_batch(_y) (a frozen_mask override returns POLAR_EINVAL, as for SCF),
 * polar_decode_device, polar_fer_batch, polar_stop_rule_batch_y, polar_time_decode_device, polar_kernel_name, polar_ctx_info
 * and polar_info_order.  A polar_create_rm context decodes the recovered N-wide row.  polar_group_* and polar_fer_multi_gpu
 * run the default list.
 * The host reads the count of open frames between attempts: one 4-byte copy and a stream sync per attempt run after the
 * first, and it stops after an attempt that leaves no frame open.  A decode while the ctx stream is capturing a graph returns
 * POLAR_EINVAL, as for the adaptive rule.
 * Refused with POLAR_EINVAL, the ctx staying usable: polar_bp_*, polar_cascl_*, polar_scf_*, polar_scan_* and polar_q8_* on a
 * BPL context; polar_bpl_* (but polar_bpl_cyclic_graphs) on any other context; polar_set_systematic(ctx, 1), polar_create_dyn
 * and polar_create_crc_file with a BPL cfg.
 * Out of scope: choosing among non-converged candidates by Euclidean distance; searching for good permutations; BPL on
 * systematic or CRC-file contexts; the reference's *_fag.c programs as a second oracle. */
/* perms [P][n], row p = pi_p.  POLAR_EINVAL, with the ctx unchanged: not a BPL ctx, P outside 1..32, or a row that is not a
 * permutation of 0 .. n-1. */
int polar_bpl_set_graphs(polar_ctx *ctx, const int *perms, int P);
/* the list of the ctx: *P and perms [P][n]; both outputs nullable */
int polar_bpl_get_graphs(const polar_ctx *ctx, int *P, int *perms);
/* the cyclic shifts out[s][b] = (b + s) mod n, s = 0 .. P-1; 5 <= n <= 12, 1 <= P <= 32.  Host only. */
int polar_bpl_cyclic_graphs(int n, int P, int *out);
/* polar_decode_device for a BPL ctx, plus per frame ([B] uint32 each): d_iters and d_flags of rule 6, d_graph of rule 5
 * and d_total_iters of rule 6.  d_iters, d_flags, d_graph and d_total_iters are nullable.  d_in: "Input rows" at
 * polar_decode_device; a permuted attempt gathers the elements of a row one by one. */
int polar_bpl_decode_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_uhat_bits,
                            uint32_t *d_iters, uint32_t *d_flags, uint32_t *d_graph, uint32_t *d_total_iters);
/* Host-buffer form: llr_in [B][N] LLRs (E per row on a rate-matched ctx), u_hat [B][N]; iters, flags, graph, total_iters
 * (nullable) [B]. */
int polar_bpl_decode_batch(polar_ctx *ctx, const double *llr_in, size_t B, int *u_hat, unsigned *iters, unsigned *flags,
                           unsigned *graph, unsigned *total_iters);

/* --- 5G NR rate matching (TS 38.212 5.4.1; no reference counterpart) -------------------------------------------------
 * A rate-matched context sends E channel values per codeword instead of N.  Notation of 38.212: A = K + r bits enter the
 * encoder (r = 0 for SC / BP / SCL), N is the context's block length, 32 <= N <= 1024, A <= E <= 8192, d = u F^{(x)n} is the
 * codeword.
 *   1. sub-block interleaver (5.4.1.1): P = {0,1,2,4,3,5,6,7,8,16,9,17,10,18,11,19,12,20,13,21,14,22,15,23,24,25,26,28,27,29,
 *      30,31}, J(n) = P[floor(32n/N)] (N/32) + (n mod N/32), y_n = d_{J(n)}.
 *   2. bit selection (5.4.1.2): repetition when E >= N, e_k = y_{k mod N}; else puncturing when 16 A <= 7 E,
 *      e_k = y_{k+N-E}; else shortening, e_k = y_k.
 *   3. channel interleaver (5.4.1.3, ibil = 1, the uplink case): T = the least integer with T(T+1)/2 >= E; e is written row
 *      by row into the upper triangle v_{i,j}, i = 0..T-1, j = 0..T-1-i, NULL after E, and read column by column,
 *      j = 0..T-1, i = 0..T-1-j, skipping the NULLs.  ibil = 0: the row sent is e.
 *   4. frozen set (5.3.1.2 with n_PC = 0): Q_F,tmp is empty for E >= N.  Puncturing adds J(n) for n < N-E and then
 *      {0 .. ceil((3N-2E)/4)-1} if 4E >= 3N, else {0 .. ceil((9N-4E)/16)-1}.  Shortening adds J(n) for E <= n < N.
 *      I[0..A) = the A most reliable positions of the context's reliability order (the 5G sequence restricted to < N) that
 *      are not in Q_F,tmp, in ascending reliability: the library's own convention (CRC word w[i] -> u[I[i]]).  The 38.212
 *      placement of payload and CRC bits inside the information set, the input interleaver (I_IL), PC bits, distributed
 *      CRC and code-block segmentation are NOT part of this (PC bits at E = N: polar_create_dyn / polar_dyn_pc5g below).
 *   5. N selection (5.3.1), a helper: n1 = ceil(log2 E) - 1 if E <= (9/8) 2^(ceil(log2 E)-1) and 16 A < 9 E, else
 *      ceil(log2 E); n2 = ceil(log2 (8A)); n = max(min(n1, n2, n_max), 5), n_max = 9 or 10.
 *   6. recovery (receiver): a row of E received values becomes the N-wide row the decoders read.  The channel interleaver is
 *      undone (ibil = 1), then the value at decoder position J(n) is: repetition, the sum over k = n (mod N), k < E, in
 *      ascending k; puncturing, +0.0 for n < N-E and e_{n-(N-E)} otherwise; shortening, e_n for n < E and
 *      POLAR_RM_SHORT_LLR otherwise.  With sigma > 0 every term is 2*y/sigma/sigma (that order).  Terms are accumulated in
 *      double and rounded once to the input's type (f32 input gives an f32 row).  POLAR_RM_SHORT_LLR = 2^20 is finite on
 *      purpose (two infinities meet in g = cL - cU and give NaN), exact in f32, and 2^20 summed over 2^12 leaves stays far
 *      below FLT_MAX; the table-driven check node clamps by exponent, so large finite values are safe there.
 *   7. a decode on a rate-matched context IS the decoder of the same cfg with info_order = rule 4, applied to the rule 6 row
 *      with sigma = 0.  Outputs stay in the u domain, [B][N]: bits, pm, flags, iterations, attempts, error counters.
 * On a rate-matched context every decode entry point takes rows of E values instead of N (polar_decode,
 * polar_decode_batch(_y), polar_decode_device, polar_bp_ / polar_cascl_ / polar_scf_decode_device and _batch,
 * polar_stop_rule_batch_y, polar_time_decode_device); the recovery runs once per call into context-owned scratch (chunks of
 * at most 256 MiB of recovered rows).  A frozen_mask override and polar_bp_readout_* return POLAR_EINVAL.
 * polar_generate_device writes [B][E]: the payload stream of a plain context with the same info_order and seed (d_u_bits
 * equal), encoded, rules 1-3, then BPSK + AWGN with sigma = 10^(-snr_db/20); element t of the sent row takes normal (t & 1) of
 * Philox(seed, frame, t >> 1, stream 2) by Box-Muller.  polar_fer_batch chains generate -> recover -> decode -> count.
 * polar_create_crc_file, polar_group_* and polar_fer_multi_gpu take no E.  The recovery scratch grows with B on first use:
 * warm a context at its largest B before capturing its stream into a graph. */
#define POLAR_RM_NONE 0      /* ctx not made by polar_create_rm */
#define POLAR_RM_REPEAT 1
#define POLAR_RM_PUNCTURE 2
#define POLAR_RM_SHORTEN 3
#define POLAR_RM_SHORT_LLR 1048576.0
/* rule 5: N for (A, E), n_max 9 or 10; POLAR_EINVAL for A < 1, E < A, E > 8192 or another n_max.  Host only. */
int polar_rm_select_n(int A, int E, int n_max);
/* rule 4: out[0..A) = I for (N, A, E); POLAR_EINVAL for N not a power of two in 32..1024, A < 1, E < A, E > 8192 or
 * A > N - |Q_F,tmp|.  Host only, touches no device. */
int polar_rm_info_order(int N, int A, int E, int *out);
/* polar_create with info_order = rule 4 for E and a channel interleaver if ibil = 1.  Refuses (POLAR_EINVAL, before any
 * device is touched) a non-NULL cfg->info_order, N outside 32..1024, E < A, E > 8192, ibil not 0 / 1 and
 * A > N - |Q_F,tmp|; every algo and dtype is accepted.  polar_info_order returns the rate-matched order. */
int polar_create_rm(const polar_cfg *cfg, int E, int ibil, polar_ctx **out);
/* E, POLAR_RM_* mode and ibil of a ctx (each nullable); a plain ctx reports E = N, POLAR_RM_NONE, 0. */
int polar_rm_info(const polar_ctx *ctx, int *E, int *mode, int *ibil);
/* rule 6 on the ctx stream: d_in [B][E] double (in_is_f32 = 0) or float, LLRs or y when sigma > 0 -> d_out [B][N] of the
 * same type.  POLAR_EINVAL on a ctx not made by polar_create_rm.  Alignment and the y form as in "Input rows" at
 * polar_decode_device; the type the sums are rounded to is rule 6's. */
int polar_rm_recover_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B, void *d_out);

/* --- Monte-Carlo code construction: genie-aided SC on the device (Arikan 2009, section IX) ---------------------------
 * A frozen set designed for an operating point, for any N: send the all-zero codeword, run SC with a genie that feeds the
 * true bits into the partial sums, and count per leaf how often its LLR has the wrong sign.  For a block length N = 2^n,
 * 32 <= N <= 4096, arithmetic type R (the ctx dtype) and one input row l[0..N) of channel LLRs:
 *  1. lambda_j, j = 0..N-1, is the leaf LLR of POLAR_ALGO_SC at leaf j when EVERY leaf is frozen: all decisions are 0, every
 *     g step is cL + cU, every f step is the library's check node, in SC's operation order.  No subtree is skipped.  The
 *     ctx's own frozen set plays no part.
 *  2. A frame adds to two counters per leaf: err[j] += (lambda_j < 0), tie[j] += (lambda_j == 0) (comparisons in R; -0.0 is a
 *     tie; a NaN counts as neither).  Counters are uint64_t [2][N] (err row, then tie row) in device memory, and a call ADDS
 *     to what the buffer holds, so calls and GPUs can be summed.  Integer sums: the result does not depend on launch shape,
 *     chunking or order.
 *  3. Design rows: frame f, element e is 2*y/sigma/sigma (that order) with y = 1 + sigma * z (bit 0 is sent as +1),
 *     z = normal (e & 1) of Philox(seed, first_frame + f, e >> 1, stream 2) by the generator's Box-Muller
 *     (sqrt(-2 log u0), sincospi(2 u1)); rounded to float for an F32 ctx.
 *  4. Order: score[j] = 2*err[j] + tie[j].  out[0..N) lists the positions in ASCENDING reliability = descending score; equal
 *     scores keep the order of a caller-given base order (ascending reliability; NULL = the library's own order for N: the
 *     5G sequence, or polarization weight above 1024).  With all counters zero the result is the base order, and
 *     out + N - A is directly a polar_cfg.info_order for A unfrozen positions.
 * The entry points work on any ctx (they use its N, dtype, device, stream, scratch and work queue; an SC ctx is the natural
 * choice) and return POLAR_EINVAL on a ctx made by polar_create_rm (its rows are E wide), for NULL buffers, B > 0x7fffffff
 * and, in the two design-row calls, sigma <= 0; the ctx stays usable.  All three are asynchronous on the ctx stream and can
 * be captured into a graph after a warm-up call at the same B.
 * Out of scope: Gaussian-approximation / density-evolution construction, soft statistics (sums of 1/(1+e^lambda): float
 * sums depend on order), rate-matched construction, polar_group_* wrappers (counters add, so a caller can shard frames over
 * GPUs by first_frame and sum). */
/* rules 1-2 on caller rows d_in [B][N] (double, or float when in_is_f32; LLRs, or y when sigma > 0: "Input rows" at
 * polar_decode_device) */
int polar_genie_count_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B, uint64_t *d_counts);
/* rule 3: d_out [B][N] double, or float when out_is_f32 */
int polar_genie_rows_device(polar_ctx *ctx, unsigned long long seed, unsigned long long first_frame, double sigma, size_t B,
                            void *d_out, int out_is_f32);
/* rule 3 rows of the ctx dtype into ctx-owned scratch in chunks of at most 256 MiB, rules 1-2 on each chunk: exactly the
 * counters of polar_genie_rows_device followed by polar_genie_count_device on the same frames */
int polar_construct_batch(polar_ctx *ctx, unsigned long long seed, unsigned long long first_frame, double sigma, size_t B,
                          uint64_t *d_counts);
/* rule 4 on host counters [2][N].  Host only, touches no device.  POLAR_EINVAL for N not a power of two in 32..4096, NULL
 * counts / out, or a base order that is not a permutation of 0..N-1. */
int polar_construct_order(int N, const uint64_t *counts, const int *base_order, int *out);

/* --- Dynamic frozen bits: PAC codes, the parity-check bits of 5G PC-polar codes (no reference counterpart) ----------------
 * A frozen position need not carry the constant 0: a dynamic frozen bit carries a GF(2) linear function of earlier decided
 * bits of the same path.  That one mechanism covers polarization-adjusted convolutional (PAC) codes (Arikan 2019), the
 * parity-check bits of TS 38.212 5.3.1.2 (n_PC > 0: the uplink cases 18 <= K <= 25), eBCH-polar subcodes and any
 * lower-triangular precoding.  A dynamic context is the plain decoder of its polar_cfg plus a set Dyn of positions and a set
 * S_j for every j in Dyn:
 *   1. algo is POLAR_ALGO_SC, POLAR_ALGO_SCL or POLAR_ALGO_CASCL; L a power of two in 1..32, or a wide list ("Wide lists"
 *      below); both dtypes; 32 <= N <= 1024.
 *   2. Dyn is a set of positions that are frozen under the cfg.  S_j is a subset of {0 .. j-1}; a member may be an
 *      information position, a plain frozen one (always 0) or an earlier dynamic one.
 *   3. At leaf j, for every live path, u_hat_0 .. u_hat_{j-1} are that path's decided bits and lambda its leaf LLR.  An
 *      information or plain frozen leaf is handled exactly as in the plain decoder.
 *   4. j in Dyn: b = XOR over i in S_j of u_hat_i, and u_hat_j = b.  In SC nothing else happens.  In SCL and CA-SCL
 *      PM = PM + PHI(lambda, b): the expression and the single rounding an information leaf uses for its branch with bit b
 *      (T(|lambda|) + max(-lambda, 0) for b = 0, T(|lambda|) + max(lambda, 0) for b = 1, then one addition to PM).  No
 *      fork, no ranking, no tie flag.  The partial sums proceed with b.
 *   5. The CRC remainder takes no contribution from any frozen position, dynamic ones included.
 *   6. Outputs: u_hat carries b at dynamic positions, not 0.  Path choice, metric and flags are otherwise those of the plain
 *      decoder.
 *   7. Identity: with every S_j empty, bits, metric and flags equal those of the plain context of the same cfg, bit for bit.
 *   8. Everything is decoded in the u domain.  For a PAC code the payload is v = u T^-1 on the information positions: a host
 *      step (polar_pac_unprecode), not a kernel step.  polar_count_errors_device keeps counting on the K + r unfrozen u
 *      positions: block errors are those of the payload (the map is a bijection), bit errors are u-domain bit errors.
 *   9. polar_generate_device on a dynamic context: payload, CRC and their placement are the plain context's for the same seed
 *      and frame, then the dynamic bits are filled in ascending position, then encode and channel with the plain context's
 *      noise.  d_u_bits carries the dynamic bits.
 * Honoured by polar_decode, polar_decode_batch(_y) (a frozen_mask override returns POLAR_EINVAL), polar_decode_device,
 * polar_generate_device, polar_fer_batch, polar_stop_rule_batch_y, polar_time_decode_device, polar_kernel_name
 * ("k_scl_dyn<...>"; "k_scl_wide<...>" for L > 32), polar_ctx_info, polar_info_order and the polar_genie_* calls (which work on any ctx and ignore the
 * constraints).  polar_cascl_*, polar_bp_*, polar_scf_* and polar_scan_* return POLAR_EINVAL on a dynamic ctx.
 * Out of scope: dynamic bits on polar_create_rm / polar_create_crc_file contexts (so 5G PC-polar is covered at E = N only),
 * polar_group_* and polar_fer_multi_gpu (they build plain contexts from a polar_cfg), a CRC in the v domain for PAC, Fano or
 * sequential decoding. */
typedef struct polar_dyn {
    int D;           /* number of dynamic positions (0 is allowed: the same kernel with no constraint)            */
    const int *pos;  /* [D] strictly ascending, each frozen under the cfg                                        */
    const int *ptr;  /* [D+1] CSR row starts, ptr[0] = 0                                                         */
    const int *idx;  /* [ptr[D]] row d = S_{pos[d]}: strictly ascending, every entry < pos[d]                    */
} polar_dyn;
/* polar_create plus the constraints.  POLAR_EINVAL: a NULL or malformed dyn, a position that is unfrozen under the cfg, an
 * algo other than SC / SCL / CA-SCL; POLAR_ENOKERNEL: N > 1024.  Both before any device is touched. */
int polar_create_dyn(const polar_cfg *cfg, const polar_dyn *dyn, polar_ctx **out);
/* D and the positions of a dynamic ctx (pos nullable, [D]); a ctx not made by polar_create_dyn reports D = -1. */
int polar_dyn_info(const polar_ctx *ctx, int *D, int *pos);
/* Host-only helpers that fill caller arrays in the polar_dyn layout (touch no device).  pos [D], ptr [D+1], idx [idx_cap];
 * *nnz (nullable) = entries of idx needed.  idx may be NULL to ask for the sizes only; a non-NULL idx with idx_cap < *nnz is
 * POLAR_EINVAL.
 * PAC: the rate-1 convolutional precoder u = v T, T_ij = g_{j-i}, g given by its exponents g_taps (g_0 = 1 required), v zero
 * outside the information set info_order[0..A).  Every position outside the information set becomes dynamic, D = N - A,
 * with S_j = {i < j : h_{j-i} = 1}, h = 1 / g(D) mod D^N. */
int polar_dyn_pac(int N, const int *info_order, int A, const int *g_taps, int n_taps, int *pos, int *ptr, int *idx,
                  int idx_cap, int *nnz);
/* bit rows [B][N] of 0/1 ints: u = v T and v = u T^-1 (u and v must not overlap) */
int polar_pac_precode(int N, const int *g_taps, int n_taps, const int *v, size_t B, int *u);
int polar_pac_unprecode(int N, const int *g_taps, int n_taps, const int *u, size_t B, int *v);
/* 38.212 5.3.1.2: q_i[0..n_qi) = Q_I in ascending reliability, n_qi = K + n_PC (K counting the CRC).  The first
 * n_pc - n_pc_wm PC positions are the least reliable members of Q_I; the other n_pc_wm are the members of minimum row weight
 * 2^popcount(j) among the n_qi - n_pc most reliable, equal weights to the higher reliability.  The value rule is the
 * standard's 5-stage cyclic register; as sets, S_j = {i < j : i in Q_I \ Q_PC, i = j (mod 5)}.  Fills pos [n_pc],
 * ptr [n_pc+1], idx, and info_order [n_qi - n_pc]: Q_I \ Q_PC in ascending reliability, which is what cfg.info_order takes. */
int polar_dyn_pc5g(int N, const int *q_i, int n_qi, int n_pc, int n_pc_wm, int *pos, int *ptr, int *idx, int idx_cap,
                   int *nnz, int *info_order);

/* --- Wide lists: L = 64, 128, 256 (no reference counterpart) ------------------------------------------------------------------
 * Short codes under dynamic frozen bits (PAC(128, 64) is the main example) approach the finite-length bounds only with lists
 * of 128 to 256.  polar_create, polar_create_dyn, polar_create_crc_file and polar_create_rm accept L = 64, 128 and 256
 *   - for POLAR_ALGO_SCL and POLAR_ALGO_CASCL,
 *   - with dtype POLAR_F64 or POLAR_F32,
 *   - when N * L <= 65536:
 *         L =  64:  N <= 1024
 *         L = 128:  N <= 512
 *         L = 256:  N <= 256
 * A larger N returns POLAR_ENOKERNEL before any device is touched.  The rule is unchanged: decisions, metric and flags are
 * what the decoder for L <= 32 is specified to give, for a larger L (phase 1 clones slot k into slot k + act; phase 2 keeps
 * the candidates c with #{m : c_m <= c} <= L; the m-th both-survivor in ascending slot order forks into the m-th dead slot; an
 * un-refilled dead slot continues as its 0-branch; POLAR_FLAG_TIE iff fewer than L candidates survive at some leaf; rules
 * 3-6 of the dynamic frozen bits; the first slot of least metric among the live slots that pass the CRC, among all live slots
 * if none passes or there is no CRC), with the same arithmetic in the same operation order.  In f64 the results are
 * bit-identical to the CPU oracle where it reaches (L = 64) on frames without a median tie.
 * One kernel serves plain and dynamic contexts: polar_kernel_name starts with "k_scl_wide<".  Every entry point works on
 * such a ctx: polar_decode, polar_decode_batch(_y), polar_decode_device, polar_cascl_decode_device / _batch (d_list = L),
 * polar_fer_batch, polar_stop_rule_batch_y, polar_time_decode_device, the generator, the error counters, the encoder side.
 * POLAR_EINVAL as before: L = 512 and above, L not a power of two, L > 32 with POLAR_Q8, a stage above 32 in
 * polar_cascl_set_stages (so no adaptive decoder on a wide ctx), L > 32 in polar_decode_llr, and polar_group_create /
 * polar_fer_multi_gpu with L > 32. */

/* --- Encoder, payload extraction, systematic polar codes (no reference counterpart as functions of their own) ----------------
 * The transmit side for a caller's own bits, and the way back from a decoder's N-wide u_hat to the K payload bits.  All rows
 * are bit-packed: bit (j & 31) of word j >> 5 is element j, the layout of d_uhat_bits.  KW = ceil(K / 32), A = K + r.
 *   1. transform: out = in F^{(x)n} over GF(2), natural order (the encoder of SCL_1024.c:242-250), rows [B][N/32].  It is an
 *      involution; d_out may equal d_in.
 *   2. place: payload rows [B][KW] (bit k = v_k; bits at or above K of the last word are ignored) become the CRC word w of A
 *      bits: w(D) = v(D) g(D), or with crc_systematic w[0..r) = D^r v mod g, w[r..A) = v (both exactly polar_generate_device's);
 *      w = v without a CRC.  Then z[I[i]] = w[i], zero elsewhere.
 *   3. extract, the inverse: w[i] = z[I[i]]; with crc_systematic v = w[r..A), otherwise v is the quotient of w(D) by g(D).
 *      crc_ok = 1 iff w(D) mod g(D) = 0 (for crc_systematic that is w[0..r) = D^r v mod g); always 1 without a CRC.  The
 *      payload rows are written with the bits at or above K zero.
 *   4. polar_encode_device: u = place(payload); on a dynamic context the dynamic bits are then filled in ascending position
 *      (rule 9 of that section); x = u F^{(x)n}.  On a rate-matched context d_x_bits is the sent row e of E bits (rules 1-3 of
 *      that section), [B][ceil(E/32)] words with the bits at or above E zero.  Either output may be NULL, not both.
 *   5. polar_payload_device: extract on d_uhat_bits (u domain, [B][N/32] on every context); d_crc_ok (nullable) [B].  For a
 *      PAC code the payload is in the v domain: polar_pac_unprecode stays a host step.
 * All device calls are asynchronous on the ctx stream, read nothing back and work on every ctx of every algo.  Their small
 * tables are built on the first call (one synchronous copy): warm a ctx before capturing its stream into a graph.
 *
 * Systematic polar coding (Arikan 2011), opt-in by polar_set_systematic(ctx, 1): the codeword carries the CRC word on the
 * information set, x[I[i]] = w[i], instead of u.  With F the complement of I:
 *      z = place(payload);  t = z F^{(x)n};  t_F = 0;  x = t F^{(x)n};  u = x F^{(x)n}
 * (u equals t, the transform being an involution, so the library runs two transforms).  This gives x[I[i]] = w[i] with
 * u_F = 0 exactly when polar_systematic_check(N, I, A) = 1: the two-pass encoder maps every unit vector on I to a codeword
 * that is that unit vector on I (A host transforms).  It holds for the library's default orders and fails for arbitrary sets.
 * The decoders are unchanged: they decide u_hat.  While the mode is on,
 *   - polar_encode_device produces the u and x above;
 *   - polar_payload_device extracts from x_hat = u_hat F^{(x)n} (formed in registers, no scratch);
 *   - polar_generate_device sends the systematic codeword of the same Philox payload with the same noise, and d_u_bits is the
 *     u actually encoded;
 *   - polar_count_errors_device, and through it polar_fer_batch and polar_stop_rule_batch_y, count the bit errors of x_hat
 *     against x on I (with crc_systematic: on the K payload positions), block errors by the same comparison;
 *   - CA-SCL, its adaptive stages and SC-Flip test the CRC of x_hat[I]: their N-entry table crc_tab (crc_tab[I[i]] =
 *     D^i mod g) is replaced by tab_sys[j] = XOR over {i < A : (j & I[i]) == I[i]} of crc_tab[I[i]] at unfrozen j, 0 at frozen
 *     j, and restored when the mode is turned off.  Path metrics, ties and every decision that does not depend on the CRC are
 *     those of the plain context.
 * polar_set_systematic(ctx, 1) returns POLAR_EINVAL and leaves the ctx unchanged when the check fails, on a dynamic ctx and on
 * a rate-matched ctx (dynamic bits and punctured systematic positions would need a definition of their own).  The default is
 * off, and with it off every entry point behaves bit for bit as before.  polar_group_* and polar_fer_multi_gpu build their
 * contexts from a polar_cfg and stay non-systematic.  The switch synchronizes the ctx stream. */
/* x = u F^{(x)n} on packed rows [B][N/32]; d_out may equal d_in */
int polar_transform_device(polar_ctx *ctx, const uint32_t *d_in, size_t B, uint32_t *d_out);
/* payload [B][KW] -> u [B][N/32] and / or the sent bits [B][N/32] ([B][ceil(E/32)] on a rate-matched ctx); either output
 * nullable, not both.  POLAR_ENOMEM (ctx usable) if the scratch rows a NULL d_u_bits or a rate-matched ctx needs cannot be had. */
int polar_encode_device(polar_ctx *ctx, const uint32_t *d_payload, size_t B, uint32_t *d_u_bits, uint32_t *d_x_bits);
/* decisions [B][N/32] -> payload [B][KW] and the per-frame CRC verdict d_crc_ok [B] (nullable) */
int polar_payload_device(polar_ctx *ctx, const uint32_t *d_uhat_bits, size_t B, uint32_t *d_payload, uint32_t *d_crc_ok);
/* host-buffer forms: payload [B][K], u [B][N], x [B][N] ([B][E] on a rate-matched ctx), all 0/1 ints; u or x may be NULL */
int polar_encode_batch(polar_ctx *ctx, const int *payload, size_t B, int *u, int *x);
int polar_payload_batch(polar_ctx *ctx, const int *u_hat, size_t B, int *payload, unsigned *crc_ok);
int polar_set_systematic(polar_ctx *ctx, int on);
int polar_get_systematic(const polar_ctx *ctx);
/* host only, touches no device: 1 if the two-pass encoder is systematic on info_order[0..A), 0 if not; POLAR_EINVAL for N not a
 * power of two in 32..4096, A outside 1..N, or positions that are out of range or repeated */
int polar_systematic_check(int N, const int *info_order, int A);
/* host only, touches no device: the two forms of the CRC test of a code with information positions info_order[0..A) (A = K +
 * crc_r, ascending reliability) and the CRC crc_taps (as in polar_cfg).  crc_tab [N] (nullable) is the table the list decoders
 * apply leaf by leaf, crc_tab[I[i]] = D^i mod g(D) (systematic != 0: tab_sys above).  masks [32][N/32] is the same test on
 * the root partial sums x_hat = u_hat F^{(x)n}, which the two-codewords-per-wavefront CA-SCL kernel (N = 1024, L = 8) applies
 * once per frame: bit i of XOR over {j : u_hat_j = 1} of crc_tab[j] is the parity of x_hat AND masks[i] (bit k & 31 of word
 * k >> 5 = position k); masks crc_r .. 31 are zero.  POLAR_EINVAL for N not a power of two in 32..4096, A outside 1..N,
 * crc_r outside 1..32, positions out of range, fewer than two taps or masks NULL. */
int polar_crc_masks(int N, const int *info_order, int A, int crc_r, const int *crc_taps, int n_taps, int systematic,
                    uint32_t *crc_tab, uint32_t *masks);
/* host only, touches no device: where the list-filling phase of the two-codewords-per-wavefront SCL / CA-SCL kernel (N = 1024,
 * L = 8) ends for the code with information positions info_order[0..A): 128, 192 or 256 when the leaves below it are decoded
 * breadth-first (at most three information leaves below it, each one of the last two leaves of its 64-leaf block and none
 * below leaf 126; for 192 and 256 exactly one of them below leaf 128 and no other in front of the last 64-leaf block), 0
 * when the kernel decodes every leaf in order, which includes every N other than 1024.  The outputs are the same either
 * way.  POLAR_EINVAL as polar_systematic_check. */
int polar_fill_phase_end(int N, const int *info_order, int A);

/* --- List output: all L paths, masked-CRC selection, list soft output (no reference counterpart) ---------------------------
 * Every list decoder ends a frame with its live paths, their metrics and their CRC remainders, and the decodes above return
 * one of them.  polar_list_decode returns them all; k_list_select, k_list_gather and k_list_soft work on what it wrote.
 * tests/list_model.py restates the rules below in numpy; tests/test_gpu_list.py holds the kernels to it with ==.
 *   1. which decoder: the context's own SCL or CA-SCL rule -- for L <= 32 the rule the oracle states, for larger L the rule of
 *      "Wide lists", on a dynamic context with rules 3-6 of "Dynamic frozen bits".  Leaf by leaf the list is the one the
 *      ordinary decode of the same context has.
 *   2. the live list: after leaf N - 1 there are `act` live slots (act = min(L, 2^#information leaves)).  Each has its decided
 *      bits u_hat (frozen = 0, dynamic = b), its metric PM in the context's arithmetic type R, and its remainder
 *      rem = XOR over {j : u_hat_j = 1} of the context's CRC table (crc_tab[I[i]] = D^i mod g(D); tab_sys in systematic mode;
 *      rem = 0 for POLAR_ALGO_SCL, which has no CRC).
 *   3. output order: rank k = 0, 1, ... lists the live slots in ascending (PM, slot), compared in R.  d_count[f] = act.  The
 *      entries k >= act are padding: bits 0, pm = +inf, rem = 0.  d_pm holds the R value widened to double (exact).
 *   4. flags: d_flags is the flags word of the ordinary decode: POLAR_FLAG_TIE and POLAR_FLAG_CRC_PASS.
 *   5. identity: let k* be the smallest k < count with rem[k] = 0 if the context has a CRC and such a k exists, else k* = 0.
 *      Then paths[k*], pm[k*] and flags equal what polar_decode_device on the same context returns for the same row, bit for
 *      bit (POLAR_FLAG_RERANK excluded: it is a diagnostic of other kernels), also where the ordinary decode runs a tuned
 *      kernel (k_scl_fast2, k_scl_fast, k_scl_big).
 *   6. where it works: POLAR_ALGO_SCL and POLAR_ALGO_CASCL, POLAR_F64 and POLAR_F32, 32 <= N <= 1024, every L the context was
 *      created with (1 .. 256); plain, dynamic, CRC-file, systematic and rate-matched contexts (rows of E values are
 *      recovered first, as everywhere else).
 *   7. refusals and launch behaviour: POLAR_ENOKERNEL for N > 1024; POLAR_EINVAL, the ctx staying usable, for any other algo,
 *      for POLAR_Q8, and while a polar_cascl_set_stages rule with more than one stage is set (a frame's list would be that
 *      of whichever stage decided it).  The calls are asynchronous on the ctx stream and read nothing back: after a warm-up
 *      at the same B (which builds the tables of a context without dynamic bits and, on a rate-matched context, sizes the
 *      scratch rows) they can be captured into a graph.  The kernels are scl_generic_body<..., DYN, LIST> (k_scl_list) and
 *      k_scl_wide<..., DYN, LIST>: the decode of k_scl_dyn / k_scl_wide with another epilogue, a context without dynamic
 *      bits being the D = 0 case.  polar_kernel_name keeps naming the ordinary decode's kernel.
 * Masked-CRC selection (blind detection):
 *   8. d_idx[f][m] = the smallest k < count[f] with rem[f][k] == masks[m], -1 if there is none.  By rule 3 that k is the
 *      least-metric member of the list with that remainder.  Padding entries are never selected, whatever the mask.  Bits
 *      of a mask at or above crc_r must be zero: d_masks is device memory and the call reads nothing back, so the library
 *      does not check it -- such a mask matches nothing, every remainder being below 2^crc_r.
 *   9. transmit convention: a transmitter that XORs mask bit i into u[I[i]] for i < crc_r sends a word whose remainder is
 *      exactly the mask, because crc_tab[I[i]] = D^i mod g(D) = D^i for i < crc_r (with crc_systematic those are the
 *      parity bits w[0..r)).  polar_payload_device on the gathered row returns the sent payload in both
 *      CRC conventions (non-systematic: the quotient of v g + m by g is v; crc_systematic: the payload is w[r..A)); its
 *      crc_ok is 0 for a mask m != 0, as it must be.
 *  10. gather: row f of the output is paths[f][d_idx[f * idx_stride]]; an index of -1 (or outside 0 .. L - 1) takes rank 0,
 *      so "the masked match, else the best path" is one call on column m of rule 8's d_idx (idx_stride = M).
 * List soft output (max-log over the list):
 *  11. candidates: the ranks k < count; with d_rem non-NULL only those with rem == want_rem, unless none of them matches, in
 *      which case all ranks k < count are used.
 *  12. domain 0 takes the path bits themselves, domain 1 each path's codeword x = u F^{(x)n} (formed inside the kernel).
 *  13. value at position j, with m_b = the least pm over the candidates whose bit j is b: +clamp if no candidate has bit 1,
 *      -clamp if none has bit 0, else min(max(m_1 - m_0, -clamp), clamp) -- one subtraction in binary64.  The sign is the
 *      library's: positive means bit 0.  clamp must be > 0 and finite (POLAR_EINVAL).  The output is always double and every
 *      value is exact.
 * Out of scope: list output from the tuned kernels (their lists are the same lists by rule 5, their epilogues are not
 * touched), N > 1024, POLAR_Q8, polar_group_*, log-sum soft output, 38.212 bit placement of the RNTI, early termination of
 * blind decodes.
 * Names: the four calls on device pointers are polar_list_decode, _select, _gather and _soft; polar_list_decode_host is the
 * host-buffer form of the first.  Their output extents (guard words around every output at ragged batches, NULL outputs) are
 * held by tests/test_gpu_list.py. */
/* d_in as polar_decode_device ("Input rows" there; [B][E] on a rate-matched ctx).  Outputs, each nullable but not all:
 * d_paths [B][L][N/32], d_pm [B][L], d_rem [B][L], d_count [B], d_flags [B]. */
int polar_list_decode(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B, uint32_t *d_paths,
                      double *d_pm, uint32_t *d_rem, uint32_t *d_count, uint32_t *d_flags);
/* host-buffer form: llr_in [B][N] ([B][E]), paths [B][L][N] ints 0/1, pm and rem [B][L], count and flags [B]; each output
 * nullable, not all.  POLAR_ENOMEM (ctx usable) if the device buffers cannot be had. */
int polar_list_decode_host(polar_ctx *ctx, const double *llr_in, size_t B, int *paths, double *pm, unsigned *rem,
                           unsigned *count, unsigned *flags);
/* rule 8: d_rem [B][L], d_count [B], d_masks [M] (device), 1 <= M <= 64 -> d_idx [B][M] */
int polar_list_select(polar_ctx *ctx, const uint32_t *d_rem, const uint32_t *d_count, size_t B, const uint32_t *d_masks,
                      int M, int32_t *d_idx);
/* rule 10: d_paths [B][L][N/32], d_idx read at [f * idx_stride] (idx_stride >= 1) -> d_uhat_bits [B][N/32] */
int polar_list_gather(polar_ctx *ctx, const uint32_t *d_paths, const int32_t *d_idx, int idx_stride, size_t B,
                      uint32_t *d_uhat_bits);
/* rules 11-13: d_rem nullable; domain 0 = u, 1 = x -> d_out [B][N] double */
int polar_list_soft(polar_ctx *ctx, const uint32_t *d_paths, const double *d_pm, const uint32_t *d_count,
                    const uint32_t *d_rem, uint32_t want_rem, int domain, double clamp, size_t B, double *d_out);

/* --- Sent-path trace: where the list loses the sent word (no reference counterpart) ----------------------------------------
 * A list decoder ends a frame correct (the sent word is in the list and is chosen), with a selection error (it is in the list,
 * another path is chosen) or with a list loss (it was pruned at some leaf).  polar_list_trace is a genie-aided list decode: it
 * takes the rows and the sent u and says, per frame, which of the three happened, at which leaf the sent path left the list
 * and how far from surviving it was.  polar_list_trace_count adds that into a loss-per-leaf histogram and three class counters.
 * tests/trace_model.py restates the rules below in numpy; tests/test_gpu_trace.py holds the kernels to it with ==.
 * Setting: a context that polar_list_decode accepts (rule 6 of "List output"): POLAR_ALGO_SCL or POLAR_ALGO_CASCL, POLAR_F64 or
 * POLAR_F32, 32 <= N <= 1024, every L the context was created with (1 .. 256); plain, dynamic, CRC-file, systematic and
 * rate-matched contexts (rows of E values are recovered first, as everywhere else).  The refusals are those of rule 7 of "List
 * output", plus POLAR_EINVAL for a NULL d_u_bits.
 * Inputs: d_rows follows "Input rows" at polar_decode_device (rows_are_f32 is in_is_f32 there).  d_u_bits [B][N/32] holds the
 * sent u, packed like d_uhat_bits: what
 * polar_generate_device / polar_encode_device write, dynamic bits included.
 *   1. the decode is the context's own: leaf by leaf the list is that of polar_list_decode (rule 1 there).  Tracing changes no
 *      decision, metric or flag.
 *   2. match: after the decision at leaf j a live slot matches iff its decided bits 0 .. j equal the sent bits 0 .. j at every
 *      position, frozen, dynamic or information.  At most one live slot matches.
 *   3. loss leaf: loss_leaf is the smallest j after whose decision no live slot matches, N if there is none.  A sent u that
 *      disagrees with a forced bit (a 1 at a plain frozen leaf, a wrong dynamic bit) is lost at that leaf: defined behaviour,
 *      not an error.
 *   4. loss rank: where the loss leaf is a ranking leaf -- an information leaf reached with act == L, where the 2L candidates c
 *      are formed -- let c_sent be the candidate of the slot that matched after leaf j - 1, with the sent bit.  Then
 *      loss_rank = #{m < 2L : c_m <= c_sent}, compared in R: the count the survivor test compares with L (so loss_rank > L).
 *      Otherwise (never lost, or lost at a frozen or dynamic leaf) loss_rank = 0.
 *   5. final rank: rank is the smallest k below count whose row in list-output order (rule 3 of "List output": ascending
 *      (PM, slot)) equals the sent u, -1 if there is none.  loss_leaf == N <=> rank >= 0.
 *   6. chosen rank and class: chosen is k* of rule 5 of "List output".  Class 0 (correct): rank == chosen.  Class 1 (selection
 *      error): rank >= 0 and rank != chosen.  Class 2 (list loss): rank < 0.
 *   7. flags: d_flags is the flags word of the ordinary decode, as rule 4 of "List output".
 *   8. reduce: polar_list_trace_count adds into d_hist, uint64_t [N + 4]: hist[j] += the frames with loss_leaf == j for j < N,
 *      hist[N + c] += the frames of class c, hist[N + 3] += B.  It ADDS to what the buffer holds; the sums are integers, so
 *      the result does not depend on launch shape or order, and calls and GPUs add.
 *   9. asynchronous: every call runs on the ctx stream and reads nothing back (graph capture as rule 7 of "List output").
 *      Every per-frame output is nullable, but not all at once.  Nothing outside [B] per output is written.
 * The kernels are scl_generic_body<..., DYN, TRACE> (k_scl_trace) and k_scl_wide<..., DYN, false, TRACE>: the
 * decode of k_scl_list / k_scl_wide with one flag per slot and another epilogue, under the same limit (POLAR_ENOKERNEL where
 * log2(L) * log2(N) > 64), and k_trace_count.  polar_kernel_name keeps naming the ordinary decode's kernel.
 * Out of scope: tracing in the tuned kernels (their lists are the same lists by rule 5 of "List output"), code books, POLAR_Q8,
 * polar_group_* (the counters add: a caller shards the frames and sums), N > 1024, a rank histogram of the live path. */
/* d_rows, rows_are_f32, sigma as d_in, in_is_f32, sigma of polar_decode_device ("Input rows" there; [B][E] on a rate-matched
 * ctx), d_u_bits [B][N/32].  Outputs [B], each nullable but not all.  tests/test_gpu_trace_rows.py holds the load stage. */
int polar_list_trace(polar_ctx *ctx, const void *d_rows, int rows_are_f32, double sigma, const uint32_t *d_u_bits, size_t B,
                     int32_t *d_loss_leaf, uint32_t *d_loss_rank, int32_t *d_rank, int32_t *d_chosen, uint32_t *d_flags);
/* rule 8: d_loss_leaf, d_rank, d_chosen [B] as polar_list_trace wrote them (all required) -> d_hist [N + 4], added to */
int polar_list_trace_count(polar_ctx *ctx, const int32_t *d_loss_leaf, const int32_t *d_rank, const int32_t *d_chosen,
                           size_t B, uint64_t *d_hist);
/* host-buffer form: llr_in [B][N] ([B][E]), u [B][N] ints 0/1; outputs [B], each nullable, not all.  POLAR_ENOMEM (ctx usable)
 * if the device buffers cannot be had. */
int polar_list_trace_host(polar_ctx *ctx, const double *llr_in, const int *u, size_t B, int *loss_leaf, unsigned *loss_rank,
                          int *rank, int *chosen, unsigned *flags);

/* --- Code books: one launch decodes frames of different codes (no reference counterpart) -----------------------------------
 * Every decode above binds one launch to one context, that is to one (N, frozen set, CRC, E) for all B frames.  A receiver
 * sees a few dozen candidates per slot at several lengths and payload sizes.  A code book holds C contexts' codes; each frame
 * of a call names its code by an index, and one persistent kernel (k_scl_book: the text of k_scl_dyn / k_scl_list with a
 * per-frame choice of the tables) decodes them all.  tests/test_gpu_codebook.py holds every rule below with == against the
 * members' own contexts.
 *   1. members: C contexts, 1 <= C <= 1024, all on one device, all of one dtype (POLAR_F64 or POLAR_F32), all of one L (a power
 *      of two in 1..32); either every member is POLAR_ALGO_SC, or every member is POLAR_ALGO_SCL or POLAR_ALGO_CASCL (those two
 *      mix: an SCL member has no CRC table).  They may differ in N (32..1024), K, info_order, CRC (r, taps, crc_systematic),
 *      dynamic frozen bits (polar_create_dyn), rate matching (polar_create_rm: E, mode, ibil) and CRC-file origin.
 *   2. snapshot: polar_codebook_create copies what a decode reads from each member into device memory the code book owns: the
 *      frozen mask, the CRC table or none, the dynamic mask rows and row index (the D = 0 tables for a member without
 *      constraints), N, n, E, the rate-matching mode and interleaver table, and whether the member is SC.  Members may be
 *      changed or destroyed afterwards; the code book does not notice.  It has its own stream, scratch and work queue.
 *   3. input: d_in is [B][ld] of double or float, ld the row stride in elements, ld >= W_max.  Frame f uses code
 *      c = d_code[f] and reads d_in[f*ld .. f*ld + W_c), W_c = E_c on a rate-matched member and N_c otherwise; the elements
 *      of the row beyond W_c are never read.  d_in needs the alignment of its element type only.  One sigma per call;
 *      sigma > 0 means the input is y, as everywhere else.
 *   4. identity -- the whole specification of the decode: for a frame with c < C the bits, the metric and the flags word are
 *      bit for bit what polar_decode_device(members[c], row_f, in_is_f32, sigma, 1, ...) returns for that row, and for the
 *      list call what polar_list_decode(members[c], ...) returns, all five outputs, padding included (POLAR_FLAG_RERANK
 *      excluded, as in rule 5 of "List output").  On a rate-matched member the value at decoder position J(n) is rule 6 of
 *      "5G NR rate matching": terms accumulated in double, rounded once to the input's type, then converted to the
 *      arithmetic type; the recovery runs in the kernel's load stage, with no second kernel and no scratch rows.
 *   5. output extents: d_uhat_bits is [B][N_max/32]; frame f writes all N_max/32 words, the words at or above N_c/32 as 0.
 *      d_paths is [B][L][N_max/32] with the same rule per rank.  d_pm, d_rem, d_count and d_flags are as in the per-context
 *      calls.  Every output is nullable, but not all of them at once.  Nothing outside these extents is written at any B.
 *   6. bad index: a frame with d_code[f] >= C gets, from the decode, bits all 0, pm = +inf, flags = POLAR_FLAG_NO_CODE, and
 *      from the list call count 0, every rank padding (bits 0, pm = +inf, rem 0), flags = POLAR_FLAG_NO_CODE.  The index is
 *      device memory: the kernel compares it with C before it forms any address from it, so a bad index reads nothing.
 *   7. asynchronous: both device calls run on the code book's stream and read nothing back; nothing grows with B (no chunk
 *      loop, no scratch rows).  After one warm-up call they can be captured into a graph at any B.
 *   8. composition with the list helpers: polar_list_select, polar_list_gather and polar_list_soft read only L, and N/32 for
 *      the gather, so they work unchanged on a code book's list outputs when called on a member context with N = N_max (and
 *      the book's L).  polar_list_soft in the x domain is only meaningful for frames whose N_c = N_max.
 *   9. refusals, POLAR_EINVAL with nothing leaked and the members untouched: a NULL or empty list, C out of range, a NULL
 *      member, mixed device, dtype or L, SC mixed with the list algos, any other algo, POLAR_Q8, L > 32, a member with
 *      polar_set_systematic on, a member with a polar_cascl_set_stages rule of more than one stage; in a call ld < W_max,
 *      B > 2^31 - 1, all outputs NULL, a misaligned d_in, a NULL d_in or d_code, the list call on a book of SC members.  A
 *      member with N > 1024 gives POLAR_ENOKERNEL.  B == 0 returns POLAR_OK and touches nothing.
 * Occupancy: the LDS layout, the choice between LDS-resident and global-scratch levels and the scratch slice are fixed once
 * per launch from N_max, so a code book that mixes N = 32 with N = 1024 runs its short frames at the long frames' occupancy.
 * Where rates matter, make one code book per N.
 * Out of scope: wide lists (L > 32), POLAR_Q8, BP / SCF / SCAN / BPL members, systematic-polar members, adaptive stages, a
 * per-frame sigma (callers with per-frame noise pass LLRs), generator, error-counter and fer_batch forms, polar_group_*,
 * sorting or bucketing frames by code inside the library.
 * Names: the two calls on device pointers are polar_codebook_decode and polar_codebook_list_decode;
 * polar_codebook_decode_host is the host-buffer form of the first.  Their output extents (guard words around every output
 * at ragged batches, NULL outputs) are held by tests/test_gpu_codebook.py. */
typedef struct polar_codebook polar_codebook;
#define POLAR_FLAG_NO_CODE 0x10u /* code-book decodes only: the frame's code index was >= C */
int polar_codebook_create(polar_ctx *const *members, int C, polar_codebook **out);
void polar_codebook_destroy(polar_codebook *cb);
/* each output nullable: C, largest N, largest row width, L, dtype */
int polar_codebook_info(const polar_codebook *cb, int *C, int *N_max, int *W_max, int *L, int *dtype);
/* member c: N, row width W (E on a rate-matched member, else N), A; each nullable */
int polar_codebook_member(const polar_codebook *cb, int c, int *N, int *W, int *A);
int polar_codebook_set_stream(polar_codebook *cb, void *hip_stream);
void *polar_codebook_get_stream(polar_codebook *cb);
int polar_codebook_synchronize(polar_codebook *cb);
const char *polar_codebook_kernel_name(const polar_codebook *cb); /* "k_scl_book<...>" */
const char *polar_codebook_last_error(const polar_codebook *cb);
/* rules 3-7: d_in [B][ld], d_code [B] -> d_uhat_bits [B][N_max/32], d_pm [B], d_flags [B]; each output nullable, not all */
int polar_codebook_decode(polar_codebook *cb, const void *d_in, int in_is_f32, size_t ld, const uint32_t *d_code,
                          double sigma, size_t B, uint32_t *d_uhat_bits, double *d_pm, uint32_t *d_flags);
/* the list form: d_paths [B][L][N_max/32], d_pm [B][L], d_rem [B][L], d_count [B], d_flags [B]; each nullable, not all */
int polar_codebook_list_decode(polar_codebook *cb, const void *d_in, int in_is_f32, size_t ld, const uint32_t *d_code,
                               double sigma, size_t B, uint32_t *d_paths, double *d_pm, uint32_t *d_rem,
                               uint32_t *d_count, uint32_t *d_flags);
/* host-buffer form: in [B][ld] doubles, code [B], u_hat [B][N_max] ints 0/1, pm / flags (nullable) [B].  POLAR_ENOMEM (code
 * book usable) if the device buffers cannot be had. */
int polar_codebook_decode_host(polar_codebook *cb, const double *in, size_t ld, const uint32_t *code, double sigma,
                               size_t B, int *u_hat, double *pm, unsigned *flags);

/* --- Fixed-point min-sum decoding: int8 SC / SCL / CA-SCL (dtype POLAR_Q8; no reference counterpart) ----------------------
 * The decoder of hardware papers and 5G receivers: quantised LLRs, a check node that is a sign and a minimum, integer path
 * metrics.  Integer arithmetic has no rounding, so everything below is exact and is tested with == against a numpy model.
 * A Q8 context has a quantiser (scale, qc, qi): scale > 0 and finite, 2 <= qc <= qi <= 8, Cc = 2^(qc-1) - 1 the clamp of
 * the channel values and Ci = 2^(qi-1) - 1 the clamp of the internal values.  The defaults scale = 2.0, qc = qi = 8 are a
 * choice: they have not been tuned and no FER stands behind them.
 *   1. quantiser: for an input value v, t = v * scale in double with one rounding (a float input is converted to double
 *      first; with sigma > 0, v = 2*y/sigma/sigma in that order); q = rint(t), ties to even, then clamped to [-Cc, Cc];
 *      NaN gives 0.  Rows handed in as int8 directly are clamped to [-Cc, Cc] on load, so -128 becomes -Cc.
 *   2. node arithmetic, all in integers: f(a, b) = s * min(|a|, |b|) with s = -1 iff (a < 0) != (b < 0);
 *      g(a, b, u) = clamp(b + (u ? -a : a), -Ci, Ci).  The schedule is SC's: leaf j's LLR lambda comes from the channel row
 *      through f on left branches and g, with the path's partial sums, on right branches: the tree of every decoder here.
 *   3. list order: the live paths form an ordered list; a path's position in it is its rank r.  At the start there is one
 *      path, rank 0, PM = 0.  PM is int32.
 *   4. frozen leaf: the bit is 0; PM += |lambda| if lambda < 0; ranks are unchanged.
 *   5. information leaf with m live paths: the 2m candidates (p, b) have PM_c = PM_p + (b != [lambda_p < 0] ? |lambda_p| : 0).
 *      They are sorted ascending by the triple (PM_c, b, r_p) and the first min(2m, L) are kept; the new ranks are the
 *      positions in that order.  PM <= N * Ci < 2^17, so (PM_c << 6) | (b << 5) | r_p is a 32-bit key, no two equal, and
 *      ranking by counting on it is exact.  POLAR_FLAG_TIE is set iff at some leaf with 2m > L the candidates at sorted
 *      positions L - 1 and L have equal PM_c.
 *   6. output.  POLAR_ALGO_SCL: the path with the smallest (PM, r).  POLAR_ALGO_CASCL: among the paths whose CRC remainder
 *      (XOR over {j : u_hat_j = 1} of crc_tab[j], crc_tab[I[i]] = D^i mod g(D), as in the float decoders) is 0 the smallest
 *      (PM, r), with POLAR_FLAG_CRC_PASS set; if no path passes, the smallest (PM, r) overall with the flag clear.
 *      POLAR_ALGO_SC: L = 1, u_hat_j = [lambda < 0] at information leaves, metric 0, flags 0.  u_hat is 0 at frozen
 *      positions.  The metric is PM (exact also where an entry point stores it as a double).
 *   7. composition: a decode of float or double rows on a Q8 context IS rule 1 followed by rules 2-6.
 * polar_create with dtype POLAR_Q8 accepts POLAR_ALGO_SC, POLAR_ALGO_SCL and POLAR_ALGO_CASCL with 32 <= N <= 1024 and L a
 * power of two in 1..32 (SC: 1), and returns POLAR_ENOKERNEL, before any device is touched, for N > 1024 and for
 * POLAR_ALGO_BP, POLAR_ALGO_SCF and POLAR_ALGO_SCAN.  polar_create_crc_file works (it only supplies g(D)).
 * Honoured through rule 7, the quantised rows in ctx-owned scratch (chunks of at most 256 MiB): polar_decode,
 * polar_decode_batch(_y) (a frozen_mask override returns POLAR_EINVAL), polar_decode_device, polar_cascl_decode_device /
 * _batch (d_list = cfg.L), polar_fer_batch (it generates f32 rows, quantises, decodes and counts), polar_stop_rule_batch_y
 * and polar_time_decode_device (which therefore times the quantiser too).  polar_kernel_name is "k_scl_q8<L=...>",
 * polar_ctx_info reports dtype 2.  Type-independent calls work unchanged: polar_generate_device, polar_count_errors_device,
 * the encode / payload / transform calls.  The scratch grows with B on first use: warm a ctx at its largest B before
 * capturing its stream into a graph.
 * POLAR_EINVAL, the ctx staying usable: polar_create_rm, polar_create_dyn, polar_group_create and polar_fer_multi_gpu with a
 * Q8 cfg; polar_set_systematic(ctx, 1), polar_cascl_set_stages, polar_genie_*, polar_construct_batch, polar_bp_*,
 * polar_scf_* and polar_scan_* on a Q8 ctx; polar_q8_* (but polar_q8_quantize_host) on a ctx of another dtype.
 * Out of scope: a one-codeword-per-lane int8 SC kernel (SC is L = 1 of the list kernel), N > 1024, rate-matched, dynamic,
 * systematic and adaptive Q8 contexts, PM saturation or normalisation, offset or normalised min-sum. */
/* POLAR_EINVAL with the ctx unchanged: not a Q8 ctx, or values out of range */
int polar_q8_set_quant(polar_ctx *ctx, double scale, int qc, int qi);
int polar_q8_get_quant(const polar_ctx *ctx, double *scale, int *qc, int *qi);   /* each output nullable */
/* rule 1 on n host values.  Host only, touches no device.  POLAR_EINVAL: scale or qc out of range, a NaN sigma. */
int polar_q8_quantize_host(const double *in, size_t n, double sigma, double scale, int qc, int8_t *out);
/* rule 1 with the ctx's quantiser, asynchronous on the ctx stream: d_in [B][N] double (in_is_f32 = 0) or float -> d_out [B][N].
 * Alignment and the y form as in "Input rows" at polar_decode_device; rule 1 takes the place of the rounding to R. */
int polar_q8_quantize_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B, int8_t *d_out);
/* rules 2-6 on quantised rows d_q [B][N] (4-byte aligned).  Asynchronous on the ctx stream, no read-back: after a warm-up at
 * the same B it can be captured into a graph.  d_uhat_bits [B][N/32]; d_pm (nullable) [B] int32; d_flags (nullable) [B]. */
int polar_q8_decode_device(polar_ctx *ctx, const int8_t *d_q, size_t B, uint32_t *d_uhat_bits, int32_t *d_pm, uint32_t *d_flags);
/* host-buffer form: q [B][N], u_hat [B][N] ints 0/1, pm and flags (nullable) [B] */
int polar_q8_decode_batch(polar_ctx *ctx, const int8_t *q, size_t B, int *u_hat, int32_t *pm, unsigned *flags);

/* --- device-side transmit chain, throughput mode (the frame loop of main(), CASCL_1024_L8.c:245-292) -----------
 * Fills B frames: random payload -> CRC multiply by g(D) -> u[I[i]] -> x = u F^{(x)n} -> BPSK + AWGN at
 * Eb/N0 = snr_db (sigma = 10^(-snr_db/20), rate 1/2 as in the reference, :237) -> d_out[B][N] (double, or float
 * when out_is_f32; channel LLRs 2y/sigma/sigma, or y when out_is_y) and d_u_bits[B][N/32] (nullable).
 * Counter-based generator: frame (first_frame + f) depends only on (seed, frame index), so batches can be cut
 * and sharded over GPUs freely.  This is NOT the reference's sequential Ranq1 stream (that one stays on the
 * host: polar_sim.c); use it for throughput / FER runs, not for reproducing published run counts.
 * The generator, by value (tests/gen_model.py restates it; tests/test_gpu_generator_values.py holds the kernels to it):
 *   Philox4x32-10 with counter (frame lo, frame hi, block, stream), frame = first_frame + f, and key (seed lo, seed hi).
 *   payload: word w of the K payload bits (bit b of the word = payload bit 32 w + b; the last word masked when K & 31) is
 *     output word 0 of (block w, stream 0).
 *   uniforms: u0 = (k0 + 0.5) 2^-53, u1 = (k1 + 0.5) 2^-53 in binary64, k0 / k1 the top 53 bits of output words 0:1 / 2:3;
 *     they lie in (0, 1] (k + 0.5 rounds to even from 2^52 on; u0 = 1 gives a normal of 0).
 *   normals: one block gives two, r cos(2 pi u1) (normal 0) and r sin(2 pi u1) (normal 1), r = sqrt(-2 log u0); |z| < 8.66.
 *   noise on a plain or dynamic context: element j of a row takes normal (j >> 6) & 1 of block (j & 63) + 64 (j >> 7),
 *     stream 1 (N = 64: normal 0 of block j; the second normal is not used).  Rate-matched rows and design rows take
 *     stream 2 (see there).
 *   y = (1 - 2 x) + sigma z and the LLR is 2 * y / sigma / sigma, evaluated in that order in binary64; a float output is
 *     that binary64 value rounded once.  N >= 64 (POLAR_EINVAL below). */
int polar_generate_device(polar_ctx *ctx, unsigned long long seed, unsigned long long first_frame, double snr_db,
                          size_t B, void *d_out, int out_is_f32, int out_is_y, uint32_t *d_u_bits);

/* One throughput-mode Monte-Carlo batch entirely on the device: generate (as polar_generate_device) -> decode ->
 * count (main()'s loop body, CASCL_1024_L8.c:245-305, B times).  Adds the batch's block and bit errors to
 * *block_errors / *bit_errors (host counters).  Buffers are owned and reused by the ctx. */
int polar_fer_batch(polar_ctx *ctx, unsigned long long seed, unsigned long long first_frame, double snr_db, size_t B,
                    unsigned long long *block_errors, unsigned long long *bit_errors);

/* The same over the GPUs of one node (frames are independent, so the range first_frame .. first_frame +
 * ngpus * frames_per_gpu is cut into contiguous shards, one per GPU, each decoded by its own context on its own host thread;
 * no data-path collective).  The only exchange is the sum of the two counters, one ncclAllReduce of 2 x uint64 over RCCL /
 * xGMI per call; RCCL is loaded with dlopen() on first use (POLAR_EDEVICE if the machine has none or fewer than ngpus
 * devices).  Frame f of the range is the same frame whatever ngpus is (counter-based generator): the totals equal
 * polar_fer_batch over the whole range on one GPU.  seconds (nullable): the slowest GPU's time for its shard.
 * A polar_group holds the ngpus contexts (devices 0 .. ngpus-1; cfg->device is ignored) and the RCCL communicators, so that a
 * sweep pays for their creation once; polar_fer_multi_gpu is create + one batch + destroy. */
typedef struct polar_group polar_group;
int polar_group_create(const polar_cfg *cfg, int ngpus, polar_group **out);
void polar_group_destroy(polar_group *grp);
int polar_group_size(const polar_group *grp);
int polar_group_fer_batch(polar_group *grp, unsigned long long seed, unsigned long long first_frame, double snr_db,
                          size_t frames_per_gpu, unsigned long long *block_errors, unsigned long long *bit_errors,
                          double *seconds);
/* main()'s stop rule `for (run = 0; errBlock < BLE; run++)` (SCL_1024.c:228) over a batch decoded in shards: generate ->
 * decode -> count on every GPU as above, then ONE ncclAllGather of the per-frame error counts (4 bytes per frame) into frame
 * order and the cut of polar_stop_rule_cut_device on GPU 0.  *frames_used = frames consumed up to and including the one that
 * brings the block errors to `need` (all ngpus * frames_per_gpu if the batch holds fewer; at least min_frames),
 * *block_errors / *bit_errors = the counters over those frames (set, not added).  Independent of ngpus by construction.
 * polar_group_create runs the two collectives on known values first and refuses the group if RCCL answers differently. */
int polar_group_stop_rule_batch(polar_group *grp, unsigned long long seed, unsigned long long first_frame, double snr_db,
                                size_t frames_per_gpu, unsigned need, size_t min_frames, size_t *frames_used,
                                unsigned long long *block_errors, unsigned long long *bit_errors);
int polar_fer_multi_gpu(const polar_cfg *cfg, int ngpus, unsigned long long seed, unsigned long long first_frame,
                        double snr_db, size_t frames_per_gpu, unsigned long long *block_errors,
                        unsigned long long *bit_errors, double *seconds);

/* stream plumbing: the ctx owns a stream by default; a host framework may hand in its own
 * (hipStream_t passed as void*). */
int polar_set_stream(polar_ctx *ctx, void *hip_stream);
void *polar_get_stream(polar_ctx *ctx);
int polar_synchronize(polar_ctx *ctx);

/* Time `reps` launches of the decode kernel on B resident frames with HIP events on the ctx stream
 * (bench.py's roofline leg).  Returns average milliseconds per launch in *ms_per_launch.  d_in: "Input rows" at
 * polar_decode_device. */
int polar_time_decode_device(polar_ctx *ctx, const void *d_in, int in_is_f32, double sigma, size_t B,
                             uint32_t *d_uhat_bits, int reps, float *ms_per_launch);

/* introspection */
/* I[0..A): the unfrozen positions in reliability order this ctx uses (the reference's global I[],
 * CASCL_1024_L8.c:99, :214-217); n must be >= A. */
int polar_info_order(const polar_ctx *ctx, int *out, int n);
int polar_ctx_info(const polar_ctx *ctx, int *N, int *K, int *A, int *L, int *algo, int *dtype);
/* name of the kernel instantiation this ctx launches (for matching rocprofv3 output) */
const char *polar_kernel_name(const polar_ctx *ctx);
/* library build id string */
const char *polar_version(void);

#ifdef __cplusplus
}
#endif
#endif
