// scl_fast2.h -- CA-SCL / SCL, L = 8, N = 1024: TWO codewords per wavefront.
//
// k_scl_fast (scl_fast.h) is VALU-issue bound at 4 waves/SIMD, and most of its instructions -- the three
// narrowest LLR levels and the whole per-leaf decision (PHI, candidate ranking, fork bookkeeping) -- carry
// useful data in 8 of 64 lanes.  Here a path owns 4 lanes instead of 8 and the other half of every 8-lane
// path group belongs to a second, independent codeword:
//
//     lane = p*8 + c*4 + pos        p = path slot 0..7, c = codeword 0/1, pos = 0..3
//
// so every narrow-level and decision instruction serves two codewords.  Level t >= 2 holds 2^t/4 registers
// per lane (element e = pos + 4r, level t at A[2^t/4 ...]); levels 7, 8, the top-left level and the channel
// vector are in the per-wave global scratch / the input exactly as in k_scl_fast.  Everything that was
// wave-uniform scalar logic there and differs per codeword (survivor masks, fork matching) is per-lane here;
// the leaf schedule (frozen pattern) is the same for both codewords, so control flow stays uniform.
// Arithmetic is the same as k_scl_fast / the reference, operation for operation.
#pragma once
#include "fast2_lds.h"
#include "fast2_scratch.h"
#include "octet_bits.h"
#include "scl_fast.h"

namespace polar {

template <typename R>
struct Fast2Cfg {
    static constexpr int NLOG = 10, N = 1024, NW = 32, TOP = 9, HI = 8, L = 8;
    // levels 2..6 in registers (keeping level 6 in the scratch as well, 32 fewer VGPRs in f64, lost its A/B run)
    static constexpr int NA = 32;   // level t at offset 2^t/4
    static constexpr int WAVES = 4;
    static constexpr int MIN_WAVES_PER_SIMD = sizeof(R) == 8 ? 3 : 4;
    static constexpr int NFA = HI - 3;  // pointer fields: LLR levels 4..8, then partial-sum levels 5..9
    // per-codeword scratch (elements of R); the elements of a level-7 / level-8 row lie in the order of fast2_scratch.h
    static constexpr size_t sc_l8 = fast2_scratch::SC_L8;
    static constexpr size_t sc_l7 = fast2_scratch::SC_L7;   // behind 8 rows of 256
    static constexpr size_t sc_l6 = fast2_scratch::SC_L6;   // behind 8 rows of 128; level 6 rows: not used (level 6 is in registers)
    static constexpr size_t sc_tl = fast2_scratch::SC_TL;   // behind 8 rows of 64
    static constexpr size_t scratch_cw = fast2_scratch::SCRATCH_CW;   // the top-left level: 512
    static constexpr size_t scratch_elems = 2 * scratch_cw;  // per wave
    // f64: the level-7 / level-8 rows in the order of fast2_scratch.h, a lane's passes 2m, 2m + 1 in one 16-byte access.
    // f32 keeps the rows in element order and one access per element: the permuted order measured 1.4 % slower there,
    // with 8-byte paired accesses and without
    static constexpr bool PAIRED = sizeof(R) == 8;
    // from_top() reads its partial-sum words once per eight passes and keeps them in registers.  f64 only: in f32, at
    // 128 VGPRs, the twelve words cost 4 to 18 more spilled registers and the kernel measured slower (DESIGN.md 4.0,
    // round 22)
    static constexpr bool TOP_WORDS_ONCE = sizeof(R) == 8;
    // block-shared LDS
    static constexpr size_t off_lut = 0;
    static constexpr size_t off_frz = off_lut + ((Lut<R>::bytes + 15) / 16) * 16;
    static constexpr size_t off_msk = off_frz + 4 * NW;     // CRC masks over x_hat [CRC_MASK_ROWS][pos][8]: mask i, words pos + 4j
    static constexpr size_t off_kth = off_msk + 4 * CRC_MASK_ROWS * NW;   // kth[mask][k] = index of the k-th set bit of mask (u8)
    static constexpr size_t off_stair = off_kth + 256 * 8;  // room for a Stair<R> (chk_idx): not used
    static constexpr size_t shared_bytes = off_stair + ((Stair<R>::bytes + 15) / 16) * 16;
    // per-wave LDS
    // partial-sum rows: row slot of codeword c at word cw_base(c) + row(slot) (fast2_lds.h: a 32-lane group's rows in
    // banks of their own)
    static constexpr size_t off_bl = 0;                                    // saved partial sums
    static constexpr size_t off_cw = off_bl + 4 * fast2_lds::ROWS_WORDS;   // working partial sums
    static constexpr size_t off_cd = off_cw + 4 * fast2_lds::ROWS_WORDS;   // candidates [2][16]
    static constexpr size_t off_ky = off_cd + sizeof(R) * 32;  // keys [2][16]
    static constexpr size_t off_sg = off_ky + 128;             // top-level staging [2][256]
    static constexpr size_t per_wave = off_sg + sizeof(R) * 512;
    static constexpr size_t total = shared_bytes + WAVES * per_wave;
    static_assert(off_cw % 16 == 0 && off_cd % 16 == 0 && per_wave % 16 == 0 && shared_bytes % 16 == 0, "LDS regions are 16-byte aligned");
};
// LDS never becomes what limits occupancy: three workgroups per CU in f64, four in f32, of 160 KiB
static_assert(3 * Fast2Cfg<double>::total <= 163840 && 4 * Fast2Cfg<float>::total <= 163840, "the pair kernel's LDS limits its occupancy");

template <int QP>
__device__ __forceinline__ double quadp(double x) { return quad_lanes<QP>(x); }
template <int QP>
__device__ __forceinline__ float quadp(float x) { return quad_lanes<QP>(x); }

// The channel vector is LLRs (FROM_Y = false: the device-resident callers, the benchmark) or channel observations y that
// every read converts with sigma (FROM_Y = true).  Only the second form has the member sigma and the f64 divisions of
// llr_from_y at its channel reads (the root step, from_top's two prefetches): the first form's chv() is the bare load.
template <bool FROM_Y>
struct Fast2Sigma { double sigma; };
template <>
struct Fast2Sigma<false> {};

template <typename R, typename IN, bool CRC_ON, bool FROM_Y>
struct Fast2Dec : Fast2Sigma<FROM_Y> {
    using C = Fast2Cfg<R>;
    static constexpr int N = C::N, NW = C::NW, TOP = C::TOP, HI = C::HI, L = 8, NFA = C::NFA;

    R A[C::NA];      // levels 2..6
    R a1;            // level 1 (pos 0, 1)
    R bp_s, bp_d, bp_ts, bp_td;   // by-products of the last level-0 check node: x + y, x - y, T(|x + y|), T(|x - y|)
    R PM;            // valid at pos 0
    uint32_t ptr, bl0, fl;
    int logact;
    int p, c, pos, lane, gl;   // gl = c*4 + pos: lane offset inside a path group
    int own_addr, oth_addr;    // rank network: byte addresses into keys[]
    uint32_t pos0_mask;        // ~0 in the lane that holds its path's metric (pos 0), else 0
    int cand_addr;
    Lut<R> lut;
    R *cand, *stg;
    uint32_t *blw, *curw, *keys;   // this lane's codeword slice of the per-wave arrays
    const unsigned char *kth;
    // Scratch and input rows are read and written through buffer instructions: a wave-uniform resource descriptor
    // (4 SGPRs) plus a 32-bit per-lane byte offset.  The two codewords of a wavefront differ by a constant offset, so no
    // lane holds a 64-bit address: round 2's per-lane pointers were spilled and re-loaded from the stack in front of every
    // load of the scratch-level steps (a dependent memory round trip per load, in the same in-order vmcnt queue).
    __amdgpu_buffer_rsrc_t rs_scr;   // this wavefront's scratch (both codewords)
    __amdgpu_buffer_rsrc_t rs_in;    // the input rows of the wavefront's two codewords
    unsigned cscr;                   // element offset of the lane's codeword in the scratch: c * scratch_cw
    unsigned csrc;                   // element offset of the lane's codeword's input row: 0 or N
    static __device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, unsigned bytes)
    {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
    }
    typedef unsigned u2_t __attribute__((ext_vector_type(2)));
    // scratch rows: sc1 loads (not served from a stale L1 line: other lanes of the wavefront wrote them), plain stores
    static __device__ __forceinline__ double ld_buf(__amdgpu_buffer_rsrc_t r, unsigned eoff, double, int aux)
    {
        return aux ? __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, eoff * 8u, 0, 16))
                   : __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, eoff * 8u, 0, 0));
    }
    static __device__ __forceinline__ float ld_buf(__amdgpu_buffer_rsrc_t r, unsigned eoff, float, int aux)
    {
        return aux ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, eoff * 4u, 0, 16))
                   : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, eoff * 4u, 0, 0));
    }
    static __device__ __forceinline__ void st_buf(__amdgpu_buffer_rsrc_t r, unsigned eoff, double v)
    {
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2_t, v), r, eoff * 8u, 0, 0);
    }
    static __device__ __forceinline__ void st_buf(__amdgpu_buffer_rsrc_t r, unsigned eoff, float v)
    {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, eoff * 4u, 0, 0);
    }
    // f64: two adjacent elements from an even element offset in one 16-byte access (a lane's passes 2m, 2m + 1 of a
    // level-7 / level-8 row: fast2_scratch.h); same descriptors, same sc1 policy
    typedef unsigned u4_t __attribute__((ext_vector_type(4)));
    struct R2 {
        R a, b;
    };
    static __device__ __forceinline__ R2 ld_buf2(__amdgpu_buffer_rsrc_t r, unsigned eoff, int aux)
    {
        static_assert(sizeof(R2) == 16, "paired accesses are for f64");
        return aux ? __builtin_bit_cast(R2, __builtin_amdgcn_raw_buffer_load_b128(r, eoff * 8u, 0, 16))
                   : __builtin_bit_cast(R2, __builtin_amdgcn_raw_buffer_load_b128(r, eoff * 8u, 0, 0));
    }
    static __device__ __forceinline__ void st_buf2(__amdgpu_buffer_rsrc_t r, unsigned eoff, R2 v)
    {
        static_assert(sizeof(R2) == 16, "paired accesses are for f64");
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4_t, v), r, eoff * 8u, 0, 0);
    }
    // "pointer" into the wavefront's scratch: an element offset; q + k, q[k] = v and ld_sc(q) read like the pointer code
    struct SPtr {
        const Fast2Dec *d;
        unsigned off;
        struct Ref {
            const Fast2Dec *d;
            unsigned off;
            __device__ __forceinline__ void operator=(R v) const { st_buf(d->rs_scr, off, v); }
        };
        __device__ __forceinline__ SPtr operator+(int k) const { return SPtr{d, off + (unsigned)k}; }
        __device__ __forceinline__ Ref operator[](int k) const { return Ref{d, off + (unsigned)k}; }
    };
    static __device__ __forceinline__ R ld_sc(SPtr q) { return ld_buf(q.d->rs_scr, q.off, R(0), 1); }
    // where an element of a level-7 / level-8 row lies behind l7() / l8(): every reader and writer of the rows asks here,
    // where it uses the row.  sg(e): element e; sg2(pos, m): the first of the pair (pos + 8m, pos + 8m + 4), a lane's
    // passes 2m and 2m + 1; the second lies sg(4) behind it (PAIRED: 1)
    static __device__ __forceinline__ int sg(int e) { return C::PAIRED ? (int)fast2_scratch::sigma((unsigned)e) : e; }
    static __device__ __forceinline__ int sg2(int pos, int m) { return C::PAIRED ? (int)fast2_scratch::pair_at((unsigned)pos, (unsigned)m) : pos + 8 * m; }
    // a lane's pair at q = row + sg2(pos, m): one access where the order makes it adjacent, else one per element
    static __device__ __forceinline__ R2 ld_sc2(SPtr q)
    {
        if constexpr (C::PAIRED) return ld_buf2(q.d->rs_scr, q.off, 1);
        else return R2{ld_sc(q), ld_sc(q + sg(4))};
    }
    static __device__ __forceinline__ void st_sc2(SPtr q, R a, R b)
    {
        if constexpr (C::PAIRED) st_buf2(q.d->rs_scr, q.off, R2{a, b});
        else {
            q[0] = a;
            q[sg(4)] = b;
        }
    }

    // word offset of a slot's row in blw / curw: every reader and writer of the rows asks here, where it uses the row
    static __device__ __forceinline__ int row(int slot) { return fast2_lds::row(slot); }
    __device__ __forceinline__ int pa(int t) const { return (ptr >> (3 * (t - 4))) & 7; }
    __device__ __forceinline__ void set_pa(int t, int v) { ptr = (ptr & ~(7u << (3 * (t - 4)))) | ((uint32_t)v << (3 * (t - 4))); }
    __device__ __forceinline__ int pb(int t) const { return (ptr >> (3 * (NFA + t - 5))) & 7; }
    __device__ __forceinline__ void set_pb(int t, int v) { ptr = (ptr & ~(7u << (3 * (NFA + t - 5)))) | ((uint32_t)v << (3 * (NFA + t - 5))); }
    // wide steps: the one-round-trip table form, as in the serial chains.  Round 2 had the compact two-round-trip form
    // here in f64; with the by-product octets (octet()) the one-round-trip form measures +2.2 % (same-box A/B, round 3),
    // without them +-0; in f32 it was already +2.4 %.
    __device__ __forceinline__ R chk(R a, R b) const { return chk_lut1<R>(a, b, lut); }
    // the narrow levels inside an octet are serial chains: the one-round-trip table form (four more issue slots,
    // one LDS latency less) measured +1.8 % there against the compact form
    __device__ __forceinline__ R chks(R a, R b) const { return chk_lut1<R>(a, b, lut); }
    __device__ __forceinline__ R chv(int e) const
    {
        double v = (double)ld_buf(rs_in, csrc + (unsigned)e, IN(0), 0);
        if constexpr (FROM_Y) v = llr_from_y(v, this->sigma);
        return (R)v;
    }
    // The row addresses are recomputed where they are used (a few instructions, 16 times per frame) instead of
    // being hoisted out of the frame loop into long-lived 64-bit registers: the empty asm stops the hoisting.
    static __device__ __forceinline__ unsigned fresh(unsigned off)
    {
        __asm__ volatile("" : "+v"(off));
        return off;
    }
    __device__ __forceinline__ SPtr l8(int slot) const { return SPtr{this, fresh(cscr + (unsigned)(C::sc_l8 + slot * 256))}; }
    __device__ __forceinline__ SPtr l7(int slot) const { return SPtr{this, fresh(cscr + (unsigned)(C::sc_l7 + slot * 128))}; }
    __device__ __forceinline__ SPtr tls() const { return SPtr{this, fresh(cscr + (unsigned)C::sc_tl)}; }

    // ---- register levels: f on own data ----
    template <int T>  // T in [2, 5]: level T from level T+1
    __device__ __forceinline__ void f_reg()
    {
        constexpr int RO = (1 << T) / 4;
#pragma unroll
        for (int r = 0; r < RO; ++r) A[RO + r] = chk(A[2 * RO + r], A[3 * RO + r]);
        if constexpr (T >= 4) set_pa(T, p);
    }
    // ---- register levels: g from the owner's level T+1 (bpermute), T in {4, 5} ----
    template <int T>
    __device__ __forceinline__ void g_reg()
    {
        constexpr int RO = (1 << T) / 4;
        const int sl = pa(T + 1) * 8 + gl;
        uint32_t w;
        if constexpr (T == 5) w = blw[row(pb(5)) + 1] >> pos;   // level 5: word 1, bit e = pos + 4r
        else w = bl0 >> (16 + pos);                              // level 4: bits 16 + e
#pragma unroll
        for (int r = 0; r < RO; ++r) {
            const R x = __shfl(A[2 * RO + r], sl), y = __shfl(A[3 * RO + r], sl);
            A[RO + r] = g_bit<R>(x, y, w, 4 * r);
        }
        set_pa(T, p);
    }
    __device__ __forceinline__ void g3()  // level 3 (eager) from the owner's level 4
    {
        const int sl = pa(4) * 8 + gl;
        const uint32_t w = bl0 >> (8 + pos);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const R x = __shfl(A[4 + r], sl), y = __shfl(A[6 + r], sl);
            A[2 + r] = g_bit<R>(x, y, w, 4 * r);
        }
    }

    // ---- scratch levels ----
    // The level-6 value of pass rr (element pos + 4 rr).  Registers: the 16 level-6 registers act as a shift
    // register -- after the 16 passes of a step the value of pass rr sits in A[16 + rr] -- so the pass loops can
    // stay rolled without a dynamically indexed register and without a round trip through memory.
    __device__ __forceinline__ void push_l6(R v)
    {
#pragma unroll
        for (int r = 16; r < 31; ++r) A[r] = A[r + 1];
        A[31] = v;
    }
    __device__ __forceinline__ void load_l6() { set_pa(6, p); }
    // d >= 8 (octets 0, 32, 64, 96): level 8 from the top level (f, or g when gstep), f down to level 6.
    // Pass rr: level-8 elements e0 + 64k (k < 4), level-7 elements e0, e0 + 64, level-6 element e0 = pos + 4 rr.
    // The top-level operands are the same for all eight paths of a codeword, so the codeword's 32 lanes fetch
    // them once per chunk of 4 passes (16 segments of 16 consecutive elements), park them in an LDS staging
    // buffer and every path reads them from there; the next chunk's loads are in flight during the compute.
    __device__ __forceinline__ R top_src(bool right, int idx, int q) const
    {
        // staging index idx = seg*16 + within; seg = k + 4*h: right: h selects ch offset {0,256,512,768};
        // left: h in {0,1} selects tl offset {0,256}
        const int seg = idx >> 4, within = idx & 15;
        const int e = 16 * q + within + 64 * (seg & 3) + 256 * (seg >> 2);
        return right ? chv(e) : ld_sc(tls() + e);
    }
    __device__ __forceinline__ void from_top(bool right, bool gstep)
    {
        vm_drain();
        const uint32_t *bt = blw + row(pb(TOP)) + 16;  // beta_9: words 16..31
        const uint32_t *bh = blw + row(pb(HI)) + 8;    // beta_8: words 8..15
        const SPtr o8 = l8(p), o7 = l7(p);
        const int w32 = (int)fresh((unsigned)(p * 4 + pos));   // lane index inside the codeword (recomputed here: the staged
                                                               // elements' offsets are not worth a register each across the frame loop)
        const int nld = right ? 8 : 4;                 // staged elements per lane and chunk
        R *pre = A + 4;    // levels 2..5 are dead during this step (recomputed below): reuse their registers
#pragma unroll
        for (int m = 0; m < 8; ++m) pre[m] = (m < nld) ? top_src(right, w32 + 32 * m, 0) : R(0);
        // the step's partial-sum words, shifted to the lane's bits.  Pass rr reads word wq = rr >> 3 of each, so with
        // TOP_WORDS_ONCE they are read once per eight passes (two chunks), else in every pass
        uint32_t wt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wh[4] = {0, 0, 0, 0};
        for (int q = 0; q < 4; ++q) {
            lds_fence();
#pragma unroll
            for (int m = 0; m < 8; ++m)
                if (m < nld) stg[w32 + 32 * m] = pre[m];
            if (C::TOP_WORDS_ONCE && (q & 1) == 0) {
                const int wq = q >> 1;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (right) {
                        wt[k] = bt[2 * k + wq] >> pos;
                        wt[4 + k] = bt[8 + 2 * k + wq] >> pos;
                    }
                    if (gstep) wh[k] = bh[2 * k + wq] >> pos;
                }
            }
            lds_fence();
            if (q < 3) {
#pragma unroll
                for (int m = 0; m < 8; ++m) pre[m] = (m < nld) ? top_src(right, w32 + 32 * m, q + 1) : R(0);
            }
#pragma unroll 1
            for (int i = 0; i < 4; ++i) {
                const int rr = 4 * q + i;
                const int s0 = sg(pos + 4 * rr);   // where element e0 = pos + 4 rr lies in a level-8 / level-7 row
                const int sh = 4 * (rr & 7);
                const int wq = rr >> 3;
                const int wi = 4 * i + pos;  // position inside a staged segment
                R *v8 = A + 12;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    R x, y;
                    if (right) {
                        const uint32_t w0 = C::TOP_WORDS_ONCE ? wt[k] : bt[2 * k + wq] >> pos;
                        const uint32_t w1 = C::TOP_WORDS_ONCE ? wt[4 + k] : bt[8 + 2 * k + wq] >> pos;
                        x = g_bit<R>(stg[(k + 0) * 16 + wi], stg[(k + 8) * 16 + wi], w0, sh);    // ch[e], ch[e+512]
                        y = g_bit<R>(stg[(k + 4) * 16 + wi], stg[(k + 12) * 16 + wi], w1, sh);   // ch[e+256], ch[e+768]
                    } else {
                        x = stg[(k + 0) * 16 + wi];   // tl[e]
                        y = stg[(k + 4) * 16 + wi];   // tl[e+256]
                    }
                    if (gstep) v8[k] = g_bit<R>(x, y, C::TOP_WORDS_ONCE ? wh[k] : bh[2 * k + wq] >> pos, sh);
                    else v8[k] = chk(x, y);
                    o8[s0 + 64 * k] = v8[k];   // element e0 + 64 k
                }
                const R v70 = chk(v8[0], v8[2]), v71 = chk(v8[1], v8[3]);
                o7[s0] = v70;
                o7[s0 + 64] = v71;
                push_l6(chk(v70, v71));
            }
        }
        set_pa(8, p);
        set_pa(7, p);
        load_l6();
    }
    // d == 7: g to level 7 from the owner's level 8, f to level 6.  Four passes per chunk: their 16 loads go out
    // together into the (dead at this point) level-6 registers.
    __device__ __forceinline__ void from_l8()
    {
        vm_drain();
        const SPtr s8 = l8(pa(8));
        const uint32_t *b7 = blw + row(pb(7)) + 4;  // beta_7: words 4..7
        const SPtr o7 = l7(p);
        // passes per chunk; the passes 2m, 2m + 1 share their four paired loads and two paired stores.  In bytes per lane
        // a chunk is what it was with 8-byte accesses (f64: 64, the measured optimum), in half the instructions
        constexpr int CP = sizeof(R) == 8 ? 2 : 4;
        static_assert(CP % 2 == 0 && 4 * CP <= 16, "a chunk is whole pairs of passes and fits the dead registers");
        for (int q = 0; q < 16 / CP; ++q) {
            R *in = A;       // levels 2..5: dead here, recomputed by the f chain below
#pragma unroll
            for (int j = 0; j < CP / 2; ++j) {
                const int m = CP / 2 * q + j;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const R2 v = ld_sc2(s8 + sg2(pos, m) + 64 * k);
                    in[8 * j + k] = v.a;       // pass 2m
                    in[8 * j + 4 + k] = v.b;   // pass 2m + 1
                }
            }
#pragma unroll
            for (int j = 0; j < CP / 2; ++j) {
                const int m = CP / 2 * q + j;
                R v70[2], v71[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int i = 2 * j + h;
                    const int rr = CP * q + i;
                    const int sh = 4 * (rr & 7);
                    const int wq = rr >> 3;
                    v70[h] = g_bit<R>(in[4 * i], in[4 * i + 2], b7[wq] >> pos, sh);
                    v71[h] = g_bit<R>(in[4 * i + 1], in[4 * i + 3], b7[2 + wq] >> pos, sh);
                }
                st_sc2(o7 + sg2(pos, m), v70[0], v70[1]);
                st_sc2(o7 + sg2(pos, m) + 64, v71[0], v71[1]);
                push_l6(chk(v70[0], v71[0]));
                push_l6(chk(v70[1], v71[1]));
            }
        }
        set_pa(7, p);
        load_l6();
    }
    __device__ __forceinline__ void from_l7()  // d == 6
    {
        vm_drain();
        const SPtr s7 = l7(pa(7));
        const uint32_t *b6 = blw + row(pb(6)) + 2;  // beta_6: words 2, 3
        const uint32_t w0 = b6[0] >> pos, w1 = b6[1] >> pos;
#pragma unroll
        for (int m = 0; m < 8; ++m) {   // passes r = 2m, 2m + 1: elements pos + 4r and + 64, one paired load each
            const R2 x = ld_sc2(s7 + sg2(pos, m)), y = ld_sc2(s7 + sg2(pos, m) + 64);
            const int r = 2 * m;
            A[16 + r] = g_bit<R>(x.a, y.a, r < 8 ? w0 : w1, 4 * (r & 7));
            A[17 + r] = g_bit<R>(x.b, y.b, r < 8 ? w0 : w1, 4 * ((r + 1) & 7));
        }
        set_pa(6, p);
    }

    // head of octet o: g at level d = ctz(8o) (root f for o = 0), f chain down to level 3 (A[2], A[3])
    __device__ __forceinline__ void octet_head(int o)
    {
        const int d = (o == 0) ? 10 : 3 + __builtin_ctz((unsigned)o);
        if (d >= 8) from_top(/*right=*/o >= N / 16, /*gstep=*/d == 8);
        else if (d == 7) from_l8();
        else if (d == 6) from_l7();
        else if (d == 5) g_reg<5>();
        else if (d == 4) g_reg<4>();
        else g3();
        if (d > 5) f_reg<5>();
        if (d > 4) f_reg<4>();
        if (d > 3) f_reg<3>();
    }
    // the same for an octet inside a group of eight (o & 7 != 0, d <= 5): only the register levels 2..5 change
    __device__ __forceinline__ void octet_head_reg(int o)
    {
        const int d = 3 + __builtin_ctz((unsigned)o);
        if (d == 5) g_reg<5>();
        else if (d == 4) g_reg<4>();
        else g3();
        if (d > 4) f_reg<4>();
        if (d > 3) f_reg<3>();
    }

    // ---- partial sums (identical per path to k_scl_fast) ----
    // Bits 0..7 of bl0: the decided bits u_0 .. u_7 of the current octet as they are, 0 at the head of every octet; a frozen
    // leaf writes nothing.  The sums over them are formed where they are read (octet(), octet_bits.h); leaf 7 turns the
    // byte into the octet's eight level-3 sums, clears it and carries on.  Bits 8..15: level 3, bits 16..31: level 4.
    template <int K>
    __device__ __forceinline__ void set_bit_k(int o, uint32_t bit)
    {
        if constexpr (K < 7) {
            bl0 |= bit << K;
        } else {
            const uint32_t c3 = octet_bits::level3((bl0 & 0x7Fu) | (bit << 7));
            bl0 &= ~0xFFu;
            set_bit7(o, c3);
        }
    }
    // Leaf 7 of octet o closes the octet: j = 8o + 7, so the combine steps at levels 0..2 are the same at every octet
    // (the caller does them with constant masks and passes c3, the octet's eight level-3 partial sums); how far the
    // carry runs beyond that depends on o alone, which is wave-uniform.
    __device__ __forceinline__ void set_bit7(int o, uint32_t c3)
    {
        if ((o & 1) == 0) {
            bl0 = (bl0 & ~0xFF00u) | (c3 << 8);
            return;
        }
        const uint32_t c4 = (((bl0 >> 8) & 0xFFu) ^ c3) | (c3 << 8);
        if ((o & 2) == 0) {
            bl0 = (bl0 & 0xFFFFu) | (c4 << 16);
            return;
        }
        set_bit_lds(8 * o + 7, ((bl0 >> 16) ^ c4) | (c4 << 16));
    }
    // levels >= 5 (words in LDS); cur = the 32 level-5 partial sums that end at leaf j, j = 31 mod 32
    __device__ __forceinline__ void set_bit_lds(int j, uint32_t cur)
    {
        // the slot's row offset is recomputed here (one instruction) rather than kept across the frame loop: as a
        // loop invariant it was spilled and re-loaded from the stack at every carry step
        const int own = (int)fresh((unsigned)row(p));
        lds_fence();
        if (pos == 0) curw[own] = cur;
        lds_fence();
        int t = 5;
        while (t < 10 && ((j >> t) & 1)) {
            const int nw = 1 << (t - 5);
            const int sb = pb(t);
            for (int w = pos; w < nw; w += 4) {
                const uint32_t cc = curw[own + w];
                const uint32_t l = blw[row(sb) + nw + w];
                curw[own + w] = l ^ cc;
                curw[own + w + nw] = cc;
            }
            lds_fence();
            ++t;
        }
        if (t < 10) {
            const int nw = 1 << (t - 5);
            for (int w = pos; w < nw; w += 4) blw[own + nw + w] = curw[own + w];
            set_pb(t, p);
            lds_fence();
        }
    }

    // ---- survivors (SCL_1024.c:612-633) for both codewords; returns this lane's codeword's 16-bit mask ----
    // Rows 0,1 of the wave rank codeword 0, rows 2,3 codeword 1: row h of a pair compares its 16 keys with the
    // row rotated by 8h .. 8h+7; permlane16_swap adds the two partial counts.
    __device__ __forceinline__ uint32_t survivors(R c0, R c1)
    {
        lds_fence();
        if (pos == 0) {
            keys[2 * p] = metric_key(c0);
            keys[2 * p + 1] = metric_key(c1);
        }
        lds_fence();
        const unsigned char *kb = reinterpret_cast<const unsigned char *>(keys) - 64 * c;  // wave base of keys[2][16]
        const uint32_t own = *reinterpret_cast<const uint32_t *>(kb + own_addr);
        const uint32_t oth = *reinterpret_cast<const uint32_t *>(kb + oth_addr);
        // key_m - key_own - 1 is negative iff key_m <= key_own (keys < 2^31); one v_alignbit shifts that sign
        // bit into the accumulator: two full-rate instructions per comparison instead of cmp + addc
        const uint32_t own1 = own + 1u;
        uint32_t acc = (oth - own1) >> 31;
        acc = __builtin_amdgcn_alignbit(acc, (uint32_t)dpp_i<0x121>((int)oth) - own1, 31);
        acc = __builtin_amdgcn_alignbit(acc, (uint32_t)dpp_i<0x122>((int)oth) - own1, 31);
        acc = __builtin_amdgcn_alignbit(acc, (uint32_t)dpp_i<0x123>((int)oth) - own1, 31);
        acc = __builtin_amdgcn_alignbit(acc, (uint32_t)dpp_i<0x124>((int)oth) - own1, 31);
        acc = __builtin_amdgcn_alignbit(acc, (uint32_t)dpp_i<0x125>((int)oth) - own1, 31);
        acc = __builtin_amdgcn_alignbit(acc, (uint32_t)dpp_i<0x126>((int)oth) - own1, 31);
        acc = __builtin_amdgcn_alignbit(acc, (uint32_t)dpp_i<0x127>((int)oth) - own1, 31);
        uint32_t cnt = __popc(acc);
        {
            auto r = __builtin_amdgcn_permlane16_swap(cnt, cnt, false, false);
            cnt = r[0] + r[1];
        }
        uint64_t b = __ballot(cnt <= (uint32_t)L);
        uint32_t m_a = (uint32_t)b & 0xFFFFu, m_b = (uint32_t)(b >> 32) & 0xFFFFu;
        if (sizeof(R) == 8 && (__popc(m_a) != L || __popc(m_b) != L)) {
            // a key tie across the boundary (or a true median tie) in either codeword: decide on the full metrics
            if (__popc(c ? m_b : m_a) != L) fl |= 0x4u;   // POLAR_FLAG_RERANK, this lane's codeword
            lds_fence();
            if (pos == 0) {
                cand[p] = c0;
                cand[8 + p] = c1;
            }
            lds_fence();
            const R *cb = reinterpret_cast<const R *>(reinterpret_cast<const unsigned char *>(cand) - (int)sizeof(R) * 16 * c);
            const R *mycand = reinterpret_cast<const R *>(reinterpret_cast<const unsigned char *>(cb) + cand_addr);
            const R mine = mycand[lane & 15];
            int n = 0;
#pragma unroll
            for (int m = 0; m < 16; ++m) n += (mycand[m] <= mine) ? 1 : 0;
            b = __ballot(n <= L);
            m_a = (uint32_t)b & 0xFFFFu;
            m_b = (uint32_t)(b >> 32) & 0xFFFFu;
        }
        return c ? m_b : m_a;
    }

    // ---- "every path keeps the branch its lambda favours" (see decide): true if so for BOTH codewords ----
    // cb / cw = the path's metric with the favoured / the other branch, cb <= cw, valid at pos 0.
    __device__ __forceinline__ bool trivial_prune(R cb, R cw) const
    {
        // the largest favoured key of the lane's codeword (the other lanes of a path take no part: 0), then ONE compare per
        // path: "max favoured < min other" <=> every path's other key is above that maximum
        uint32_t mx = metric_key(cb) & pos0_mask;
        mx = max(mx, (uint32_t)dpp_i<0x128>((int)mx));   // row_ror:8: the other path of this row of 16 lanes
        {
            auto a = __builtin_amdgcn_permlane16_swap(mx, mx, false, false);
            mx = max(a[0], a[1]);
        }
        {
            auto a = __builtin_amdgcn_permlane32_swap(mx, mx, false, false);
            mx = max(a[0], a[1]);
        }
        return __ballot(mx >= (metric_key(cw) | ~pos0_mask)) == 0ull;
    }
    static __device__ __forceinline__ uint32_t sign_bit(double x) { return (uint32_t)__double2hiint(x) >> 31; }
    static __device__ __forceinline__ uint32_t sign_bit(float x) { return (uint32_t)__float_as_int(x) >> 31; }

    // ---- decision at leaf j = 8o + K; lambda valid at pos 0 ----
    // FULL: the list is full (logact == 3: at and behind the third information leaf), known at compile time -- the code
    // that fills the list, its metric select and its merge with the full-list paths do not exist in those instantiations
    template <int K, bool FULL>
    __device__ __forceinline__ void decide(int o, bool frozen, R lam) { decide_t<K, FULL>(o, frozen, lam, lut.tabv(lam)); }
    // tt = T(|lambda|) (SCL_1024.c:352-359), looked up by the caller -- or, at the odd leaves, a by-product of the
    // check node that produced the even leaf's lambda (see octet())
    template <int K, bool FULL>
    __device__ __forceinline__ void decide_t(int o, bool frozen, R lam, R tt)
    {
        // The exits of a leaf share no merged state beyond what each of them writes.  A frozen leaf touches PM and bl0
        // and is done.  At an information leaf the outcome of the trivial prune (bit, metric) is computed in front of
        // the prune test and the ranked path is an `if` without `else` that overrides it: the values a fork permutes
        // (ptr, bl0, A[1..3], a1, bp_d, bp_td) have the fork block as their only writer, so where the paths meet
        // they merge with the unchanged registers and not with copies made on the trivial side.  (With `if (trivial)
        // ... else ...` the structurised merge took every such value through a second register set: 13-17 moves on
        // the trivial exit, and as many back where the frozen exit joins; profiles/r15_ab.txt.)
        if (frozen) {
            PM += tt + negmax(lam);  // PHI(.,0)
            set_bit_k<K>(o, 0u);
            return;
        }
        uint32_t bit;
        R pm;
        if (!FULL && logact < 3) {
            const R ph0 = tt + negmax(lam), ph1 = tt + posmax(lam);  // PHI(.,0), PHI(.,1)
            bit = (p >> logact) & 1;
            pm = PM + (bit ? ph1 : ph0);
            ++logact;
        } else {
            // PHI of the branch lambda favours is T(|lambda|), of the other one T(|lambda|) + |lambda|
            // (SCL_1024.c:481-502; T + 0 is T, so these ARE c0 / c1 in the order the sign of lambda says).
            const uint32_t lneg = sign_bit(lam);   // lambda = +-0: cb == cw, never trivial, c0 == c1 below
            const R cb = PM + tt, cw = PM + (tt + absr(lam));
            // Most information leaves (85 % at 1-3 dB) prune trivially: every path keeps its favoured branch.
            // That is certain when the largest of the eight favoured keys is below the smallest of the eight
            // others (the 8 favoured candidates are then the 8 smallest of the 16, all strictly below the median
            // of SCL_1024.c:619-633), and three max/min steps over the path lanes show it -- without the key
            // exchange through LDS, the rank network and the fork bookkeeping.  Both codewords must qualify.
            bit = (uint32_t)dpp_i<0x00>((int)lneg);   // quad_perm [0,0,0,0]: pos 0 holds lambda
            pm = cb;
            if (!trivial_prune(cb, cw)) ranked<K>(lneg, cb, cw, bit, pm);
        }
        PM = pm;
        set_bit_k<K>(o, bit);
    }
    // the leaf's decision by ranking the 16 candidates; bit / pm come in as the trivial outcome and leave as the ranked one
    template <int K>
    __device__ __forceinline__ void ranked(uint32_t lneg, R cb, R cw, uint32_t &bit, R &pm)
    {
        const R c0 = lneg ? cw : cb, c1 = lneg ? cb : cw;
        const uint32_t mask = survivors(c0, c1);
        const uint32_t m0 = mask & 0xFFu, m1 = mask >> 8;
        const uint32_t m_both = m0 & m1, m_dead = ~(m0 | m1) & 0xFFu;
        if (__popc(mask) < L) fl |= 0x1u;  // median tie in this lane's codeword
        const bool s0 = (m0 >> p) & 1, s1 = (m1 >> p) & 1;
        // a slot keeps its surviving branch; one with both keeps 0 (its 1-branch moves to a dead slot); tie rule: a dead
        // slot that is not refilled continues as its 0-branch
        bit = (!s0 && s1) ? 1u : 0u;
        pm = bit ? c1 : c0;
        if (__ballot(m_dead != 0u) == 0ull) return;  // no codeword forks
        // m-th both-survivor (ascending slot) forks into the m-th dead slot (:636-661), per codeword
        const bool dead = !s0 && !s1;
        const int myrank = __popc(m_dead & ((1u << p) - 1u));
        const bool refilled = dead && (myrank < __popc(m_both));
        const int src = (int)kth[m_both * 8 + myrank];   // myrank <= 7: inside the table for every lane
        const int sg = refilled ? src : p;
        const int sl = sg * 8 + gl;
        const R c1s = __shfl(c1, sl);
        ptr = __shfl(ptr, sl);
        bl0 = __shfl(bl0, sl);
        // what the lower-node steps still to come in this octet read: the sum / difference pairs of the
        // check nodes above them (octet())
        if constexpr ((K & 4) == 0) { A[2] = __shfl(A[2], sl); A[3] = __shfl(A[3], sl); }  // s2, d2: g at level 2 (leaf 4)
        if constexpr ((K & 2) == 0) { A[1] = __shfl(A[1], sl); a1 = __shfl(a1, sl); }       // s1, d1: g at level 1
        if constexpr ((K & 1) == 0) { bp_d = __shfl(bp_d, sl); bp_td = __shfl(bp_td, sl); } // a forked copy continues with bit 1: -d0, T(|d0|)
        bit = refilled ? 1u : bit;
        pm = refilled ? c1s : pm;
    }

    // ---- the leading run of P all-frozen octets (leaves 0 .. 8P-1; 1 <= P <= 15), instead of octets 0 .. P-1 ----
    // Nothing has been decided yet, so every partial sum below the first level-7 node is 0 and BOTH children of
    // every node are known the moment the node is: f(x, y) and y + x.  The whole 128-leaf subtree is therefore
    // evaluated as seven butterfly stages over one 128-element array per codeword (32 lanes, two butterflies per
    // lane and stage) instead of octet by octet on eight replicated paths.  The values are those of the lazy
    // recursion, operation for operation; the path metric adds PHI(lambda_j, 0) for j = 0 .. 8P-1 in that order
    // (SCL_1024.c:601-604).  Afterwards the registers hold the nodes that contain leaf 8P at levels 4..6.
    // Levels 8 and 7 above it are computed once, by the codeword's 32 lanes together, into slot 0's scratch rows,
    // and every slot points there (the eight slots are replicas of one path until the first information leaf).
    // fill_phase() runs the same tree for all 128 leaves: it asks for the metric of the first nphi leaves only
    // (nphi = 8P otherwise), takes no registers (regs = false: the head at octet E/8 rebuilds them) and wants the
    // level-1 pair above leaves 126 / 127 (xl, yl), which the last stage overwrites.
    __device__ __forceinline__ void frozen_prefix(int P, int nphi, bool regs, R &xl, R &yl)
    {
        const int w32 = p * 4 + pos, j0 = 8 * P;
        vm_drain();   // the top-left level written by the root step
        {
            const SPtr tl = tls();
            const SPtr o8 = l8(0) + sg(w32), o7 = l7(0) + sg(w32);   // element w32 + 32 k lies at sg(w32) + 32 k
            R v8[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = w32 + 32 * k;
                v8[k] = chk(ld_sc(tl + e), ld_sc(tl + e + 256));
                o8[32 * k] = v8[k];
            }
            lds_fence();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const R v7 = chk(v8[k], v8[k + 4]);   // elements e and e + 128 of level 8
                o7[32 * k] = v7;
                stg[w32 + 32 * k] = v7;
            }
            set_pa(8, 0);
            set_pa(7, 0);
        }
        lds_fence();
#pragma unroll
        for (int t = 6; t >= 0; --t) {
            const int h = 1 << t;
            int idx[2];
            R x[2], y[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int b = w32 + 32 * i;
                idx[i] = ((b >> t) << (t + 1)) | (b & (h - 1));
                x[i] = stg[idx[i]];
                y[i] = stg[idx[i] + h];
            }
            if (t == 0) {
                xl = stg[126];
                yl = stg[127];
            }
            lds_fence();
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                stg[idx[i]] = chk(x[i], y[i]);
                stg[idx[i] + h] = y[i] + x[i];
            }
            lds_fence();
            if (t >= 4 && regs) {   // node of level t that holds leaf j0: elements pos + 4r
                const R *node = stg + ((j0 >> t) << t) + pos;
#pragma unroll
                for (int r = 0; r < h / 4; ++r) A[h / 4 + r] = node[4 * r];
            }
        }
        // PHI(lambda_j, 0) of all 128 leaves, then the metric in leaf order
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const R lam = stg[w32 + 32 * k];
            stg[128 + w32 + 32 * k] = lut.tabv(lam) + negmax(lam);
        }
        lds_fence();
        R pm = PM;
#pragma unroll 8
        for (int j = 0; j < nphi; ++j) pm += stg[128 + j];
        PM = pm;
        lds_fence();
    }

    // ---- the list-filling phase: leaves 0 .. E-1, E in {128, 192, 256} (the host's choice, polar_fill_phase_end) ----
    // Below E every information leaf is one of the last two leaves of its 64-leaf block, and for E > 128 exactly one of
    // them lies in front of the last block, below leaf 128.  Inside a block all partner bits are therefore 0 up to its
    // last pair, two distinct paths enter it (slot s continues path s & 1: the forks go by slot bits, decide()), and
    // the block is two 64-element butterflies per codeword instead of eight octets on eight slots.  The last two leaves are frozen
    // (PHI(., 0)) or fork without ranking, exactly as decide() does while logact < 3.  Every slot keeps its own metric
    // and writes its own partial-sum rows, so pb() stays as the frame set it; the level-7 rows of the two paths go to
    // the scratch rows of slots 0 and 1.  The head at octet E/8 (from_l8 / from_l7 / from_top) rebuilds every register.
    // bit0 / bit1 of f2: leaf frozen.  lam0: the even leaf's lambda; (xl, yl): the level-1 pair above the two leaves.
    // Returns the block's partial sums, which are the same in every 32-bit word: u = bit at the last-but-one leaf gives
    // the even positions, u = bit at the last leaf gives all of them.
    __device__ __forceinline__ uint32_t fill_tail(uint32_t f2, R lam0, R xl, R yl)
    {
        uint32_t b0 = 0, b1 = 0;
        if (!(f2 & 1u)) {
            b0 = (p >> logact) & 1;
            ++logact;
        }
        PM += lut.tabv(lam0) + (b0 ? posmax(lam0) : negmax(lam0));   // PHI(lambda, bit)
        const R lam1 = b0 ? -(xl - yl) : yl + xl;   // g with the bit just decided: the single rounding of leaf_pair()
        if (!(f2 & 2u)) {
            b1 = (p >> logact) & 1;
            ++logact;
        }
        PM += lut.tabv(lam1) + (b1 ? posmax(lam1) : negmax(lam1));
        return (b0 ? 0x55555555u : 0u) ^ (b1 ? 0xFFFFFFFFu : 0u);
    }
    __device__ __forceinline__ void fill_phase(int E, const uint32_t *frz, R xl, R yl)
    {
        const int w32 = (int)fresh((unsigned)(p * 4 + pos));
        const int qb = (p & 1) * 64;   // the slot's path inside the staging buffer
        const uint32_t wv0 = fill_tail(frz[3] >> 30, stg[126], xl, yl);
        uint32_t wv1 = 0;
        lds_fence();
        blw[row(p) + 4 + pos] = wv0;   // beta_7
        lds_fence();
#pragma unroll 1
        for (int S = 128; S < E; S += 64) {
            // the block's level-6 node for paths 0 and 1, elements w32 and w32 + 32, at stg[64 q + .]
            vm_drain();
            const uint32_t wsel = S == 128 ? wv0 : wv1;   // beta_7 (S = 128) / beta_6 (S = 192) of the slot ...
            uint32_t wq[2];                               // ... and of slots 0 and 1 at bit w32 & 31 = e & 31
            wq[0] = (uint32_t)__shfl((int)wsel, gl) >> w32;
            wq[1] = (uint32_t)__shfl((int)wsel, 8 + gl) >> w32;
            if (S == 128) {   // g at level 7 from slot 0's level-8 row (the prefix's), f to level 6
                const SPtr s8 = l8(0) + sg(w32);   // element w32 + 32 k of a row lies at sg(w32) + 32 k
                R v8[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v8[k] = ld_sc(s8 + 32 * k);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const SPtr o7 = l7(q) + sg(w32);
                    R v7[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v7[k] = g_bit<R>(v8[k], v8[k + 4], wq[q], 0);
                        o7[32 * k] = v7[k];
                    }
                    stg[64 * q + w32] = chk(v7[0], v7[2]);
                    stg[64 * q + w32 + 32] = chk(v7[1], v7[3]);
                }
                set_pa(7, p & 1);
            } else {          // g at level 6 from the path's level-7 row
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const SPtr s7 = l7(q) + sg(w32);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        stg[64 * q + w32 + 32 * i] = g_bit<R>(ld_sc(s7 + 32 * i), ld_sc(s7 + 32 * i + 64), wq[q], 0);
                }
            }
            lds_fence();
#pragma unroll
            for (int t = 5; t >= 0; --t) {   // six stages, both paths: 64 butterflies, two per lane
                const int h = 1 << t;
                int idx[2];
                R x[2], y[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int b = w32 + 32 * i;
                    idx[i] = ((b >> t) << (t + 1)) | (b & (h - 1));
                    x[i] = stg[idx[i]];
                    y[i] = stg[idx[i] + h];
                }
                if (t == 0) {
                    xl = stg[qb + 62];
                    yl = stg[qb + 63];
                }
                lds_fence();
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    stg[idx[i]] = chk(x[i], y[i]);
                    stg[idx[i] + h] = y[i] + x[i];
                }
                lds_fence();
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const R lam = stg[w32 + 32 * k];
                stg[128 + w32 + 32 * k] = lut.tabv(lam) + negmax(lam);
            }
            lds_fence();
            R pm = PM;
#pragma unroll 2
            for (int j = 0; j < 62; ++j) pm += stg[128 + qb + j];
            PM = pm;
            const uint32_t wv = fill_tail(frz[(S + 62) >> 5] >> 30, stg[qb + 62], xl, yl);
            lds_fence();
            if (S == 128) {
                wv1 = wv;
                if (pos < 2) blw[row(p) + 2 + pos] = wv;   // beta_6
            } else {          // beta_8 = (beta_7 ^ b, b), b = the partial sums of leaves 128 .. 255 = (wv1 ^ wv, wv)
                const uint32_t b = pos < 2 ? wv1 ^ wv : wv;
                blw[row(p) + 8 + pos] = wv0 ^ b;
                blw[row(p) + 12 + pos] = b;
            }
            lds_fence();
        }
    }

    // ---- octets whose first seven leaves are frozen: breadth-first (all partner bits are 0) ----
    template <bool FULL>
    __device__ __forceinline__ void octet_frozen_prefix(int o, bool last_frozen)
    {
        // level 2: f half (leaves 0..3) and g half (leaves 4..7), element pos each
        R xf = chks(A[2], A[3]), xg = A[3] + A[2];
        // level 1: lanes pos 0,1 = f results, lanes 2,3 = g results, for both halves
        R yf = quadp<0x4E>(xf), yg = quadp<0x4E>(xg);  // lane ^ 2
        {
            const R ff = chks(xf, yf), gf = xf + yf, fg = chks(xg, yg), gg = xg + yg;
            xf = (pos & 2) ? gf : ff;
            xg = (pos & 2) ? gg : fg;
        }
        // level 0: lambda_k in lane pos = k & 3 of (k < 4 ? xf : xg)
        yf = quadp<0xB1>(xf); yg = quadp<0xB1>(xg);    // lane ^ 1
        R lf, lg;
        {
            const R ff = chks(xf, yf), gf = xf + yf, fg = chks(xg, yg), gg = xg + yg;
            lf = (pos & 1) ? gf : ff;
            lg = (pos & 1) ? gg : fg;
        }
        const R pf = lut.tabv(lf) + negmax(lf), pg = lut.tabv(lg) + negmax(lg);  // PHI(lambda_k, 0)
        PM += pf;
        PM += quadp<0x55>(pf);  // lane 1 of the quad
        PM += quadp<0xAA>(pf);  // lane 2
        PM += quadp<0xFF>(pf);  // lane 3
        PM += pg;
        PM += quadp<0x55>(pg);
        PM += quadp<0xAA>(pg);
        if (last_frozen) {
            PM += quadp<0xFF>(pg);
            set_bit7(o, 0u);   // bits 0..7 of bl0 are 0 as at the head of every octet (set_bit_k): c3 = 0
        } else {
            decide<7, FULL>(o, false, quadp<0xFF>(lg));
        }
    }

    // Check node that keeps what it computed on the way: CHK(x, y) = sgn min + (T(|s|) - T(|d|)) with s = x + y,
    // d = x - y (SCL_1024.c:350-373).  The lower-node update of the same pair is cL +- cU = y +- x (:412-416), i.e.
    // s for partner bit 0 and y - x = -d for bit 1 -- same operands, one rounding, so the value is the one g_bit()
    // computes (a zero may come out as -0 where y - x gives +0; a zero lambda decides nothing: PHI adds no penalty
    // either way, it never prunes trivially, and c0 == c1 in the ranking).  T(|s|), T(|d|) are the staircase values the
    // odd leaf's PHI needs.  So inside an octet every g step and every second table look-up is a by-product.
    struct ChkBp { R v, s, d, ts, td; };
    // s or -d by the partner bit at position sh of w.  The selects of the by-product g steps go by sign mask + v_bfi_b32
    // rather than v_cmp + v_cndmask: +-0 while the wavefronts took their jobs by a fixed stride
    // (profiles/r03_ab_experiments.txt run 24), + 1.3 % since the work queue (run 34).
    static __device__ __forceinline__ R g_sel(R sum, R dif, uint32_t w, int sh)
    {
        // bit -> all-ones mask (one v_bfe_i32), then v_bfi per word: no compare, no v_cndmask
        const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)w, sh, 1);
        return Lut<R>::sel_mask(m, -dif, sum);
    }
    // The node itself.  Only the lower lane of each pair (lane, lane ^ B) is read: B = 1 at level 0 (QP = 0xB1, data in
    // pos 0), B = 2 at level 1 (QP = 0x4E, data in pos 0, 1).  The upper lane holds the partner operand and would look up
    // values nobody reads, so it takes the lower lane's second look-up instead: with the sign of ITS partner flipped, the
    // one addition gives s = x + y in the lower lane and y - x = -d in the upper one, and T(|-d|) is T(|d|) bit for bit
    // (tabv() reads exponent and mantissa bits and compares |.|).  One tabv() then serves both; the lower lane takes
    // T(|d|) from its neighbour.  In the lower lane the flip is zero, so x, y, s, d, v and both table values there are
    // those of two look-ups in the lane; d is computed in the lane, never taken from the neighbour (-0 for +0).
    // (-12 LDS and -24 VALU instructions per octet.)
    static __device__ __forceinline__ double flip_sign(double y, uint32_t m) { return __hiloint2double(__double2hiint(y) ^ (int)m, __double2loint(y)); }
    static __device__ __forceinline__ float flip_sign(float y, uint32_t m) { return __int_as_float(__float_as_int(y) ^ (int)m); }
    template <int QP>
    __device__ __forceinline__ ChkBp chk_narrow(R x) const
    {
        static_assert(QP == 0xB1 || QP == 0x4E, "partner in lane ^ 1 or lane ^ 2");
        // the sign bit in the upper lane of a pair: the compiler keeps it as a lane constant per level and folds the flip
        // into the partner's DPP move (v_xor_b32 with a DPP source)
        const uint32_t up = QP == 0xB1 ? (uint32_t)pos << 31 : ((uint32_t)pos << 30) & 0x80000000u;
        const R y = flip_sign(quadp<QP>(x), up);
        ChkBp r;
        r.s = x + y;
        r.d = x - y;
        r.ts = lut.tabv(r.s);
        r.td = quadp<QP>(r.ts);
        r.v = xor_sign(minabs(x, y), x, y) + (r.ts - r.td);
        return r;
    }
    template <int K, bool FULL>   // leaves K (even) and K + 1 from the level-1 pair in a1 (pos 0: x, pos 1: y)
    __device__ __forceinline__ void leaf_pair(int o, uint32_t fm, R x1)
    {
        const ChkBp q = chk_narrow<0xB1>(x1);
        bp_d = q.d;
        bp_td = q.td;
        decide<K, FULL>(o, (fm >> K) & 1, q.v);
        // leaf K + 1: g0 with the bit just decided (bit K of bl0, set_bit_k<K>); a slot refilled by a fork took
        // bp_d / bp_td of its source and continues with bit 1, every other slot still has its own q.s / q.ts
        const uint32_t m1 = (uint32_t)__builtin_amdgcn_sbfe((int)bl0, K, 1);
        decide_t<K + 1, FULL>(o, (fm >> (K + 1)) & 1, Lut<R>::sel_mask(m1, -bp_d, q.s), Lut<R>::sel_mask(m1, bp_td, q.ts));
    }
    template <bool FULL>
    __device__ __forceinline__ void octet(int o, uint32_t fm)
    {
        // level 2: f of (A[2], A[3]); its sum / difference stay in A[2], A[3] for the g step at leaf 4
        {
            const R s2 = A[2] + A[3], d2 = A[2] - A[3];
            const R v2 = xor_sign(minabs(A[2], A[3]), A[2], A[3]) + (lut.tabv(s2) - lut.tabv(d2));
            A[2] = s2;
            A[3] = d2;
            // level 1: f; sum / difference in (A[1], a1) for the g steps at leaves 2 and 6 (read at pos 0, 1)
            const ChkBp q1 = chk_narrow<0x4E>(v2);
            A[1] = q1.s;
            a1 = q1.d;
            leaf_pair<0, FULL>(o, fm, q1.v);
        }
        // the partner sums of the g steps come from the octet's raw bits (bits 0..7 of bl0) where they are read
        leaf_pair<2, FULL>(o, fm, g_sel(A[1], a1, octet_bits::level1_lo(bl0), pos));
        {
            const R v2 = g_sel(A[2], A[3], octet_bits::level2(bl0), pos);   // level 2, g
            const ChkBp q1 = chk_narrow<0x4E>(v2);
            A[1] = q1.s;
            a1 = q1.d;
            leaf_pair<4, FULL>(o, fm, q1.v);
        }
        leaf_pair<6, FULL>(o, fm, g_sel(A[1], a1, octet_bits::level1_hi(bl0), pos));
    }
};

// One group: the octets from o to the next multiple of eight.  Returns that multiple.
template <typename D, bool FULL>
__device__ __forceinline__ int octet_group(D &s, const uint32_t *frz, uint32_t &fword, int o)
{
    s.octet_head(o);   // the first octet after the frozen run, then octets 8, 16, ...
    for (;;) {
        if ((o & 3) == 0) fword = frz[o >> 2];
        const uint32_t fm = (fword >> (8 * (o & 3))) & 0xFFu;
        if ((fm & 0x7Fu) != 0x7Fu) s.template octet<FULL>(o, fm);
        else s.template octet_frozen_prefix<FULL>(o, fm == 0xFFu);
        ++o;
        if ((o & 7) == 0) break;
        s.octet_head_reg(o);
    }
    return o;
}

template <typename R, typename IN, bool CRC_ON, bool FROM_Y>
__device__ __forceinline__ void scl_fast2_body(const SclParams &P)
{
    using D = Fast2Dec<R, IN, CRC_ON, FROM_Y>;
    using C = Fast2Cfg<R>;
    constexpr int N = C::N, NW = C::NW, L = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the per-wave LDS base is scalar
    unsigned char *base = smem + C::shared_bytes + (size_t)wave * C::per_wave;
    uint32_t *frz = reinterpret_cast<uint32_t *>(smem + C::off_frz);
    uint32_t *msk = reinterpret_cast<uint32_t *>(smem + C::off_msk);
    unsigned char *kth = smem + C::off_kth;

    Lut<R>::build(smem + C::off_lut, threadIdx.x, blockDim.x);
    for (int i = threadIdx.x; i < NW; i += blockDim.x) frz[i] = P.frozen[i];
    if (CRC_ON)   // mask i, word pos + 4j at [i][pos][j]: a lane's eight words of a mask are two 16-byte reads
        for (int i = threadIdx.x; i < CRC_MASK_ROWS * NW; i += blockDim.x)
            msk[i] = P.crc_mask[(i & ~(NW - 1)) + ((i >> 3) & 3) + 4 * (i & 7)];
    for (int i = threadIdx.x; i < 256 * 8; i += blockDim.x) {
        int m = i >> 3, k = i & 7, idx = 0, seen = 0;
        for (int b = 0; b < 8; ++b)
            if ((m >> b) & 1) {
                if (seen == k) idx = b;
                ++seen;
            }
        kth[i] = (unsigned char)idx;
    }
    __syncthreads();

    D s;
    s.lane = threadIdx.x & 63;
    s.p = s.lane >> 3;
    s.c = (s.lane >> 2) & 1;
    s.pos = s.lane & 3;
    s.pos0_mask = s.pos == 0 ? 0xFFFFFFFFu : 0u;
    s.gl = s.lane & 7;
    s.lut.bind(smem + C::off_lut);
    s.kth = kth;
    s.blw = reinterpret_cast<uint32_t *>(base + C::off_bl) + fast2_lds::cw_base(1) * s.c;
    s.curw = reinterpret_cast<uint32_t *>(base + C::off_cw) + fast2_lds::cw_base(1) * s.c;
    s.cand = reinterpret_cast<R *>(base + C::off_cd) + s.c * 16;
    s.keys = reinterpret_cast<uint32_t *>(base + C::off_ky) + s.c * 16;
    s.stg = reinterpret_cast<R *>(base + C::off_sg) + s.c * 256;
    if constexpr (FROM_Y) s.sigma = P.sigma;
    {   // rank network: lane (row, i): rows 0,1 -> codeword 0, rows 2,3 -> codeword 1; candidate i is
        // (slot i & 7, branch i >> 3) stored at keys[cw][2*slot + branch]
        const int i = s.lane & 15, row = s.lane >> 4, cwr = row >> 1, h = row & 1;
        const int jj = (i + 8 * h) & 15;
        s.own_addr = 64 * cwr + 4 * (2 * (i & 7) + (i >> 3));
        s.oth_addr = 64 * cwr + 4 * (2 * (jj & 7) + (jj >> 3));
        s.cand_addr = (int)sizeof(R) * 16 * cwr;
    }
    const int lane = s.lane, p = s.p, c = s.c, pos = s.pos;
    const int wave_global = blockIdx.x * C::WAVES + wave;
    const int waves_total = gridDim.x * C::WAVES;
    R *scr_wave = reinterpret_cast<R *>(P.scratch) + (size_t)wave_global * C::scratch_elems;
    s.rs_scr = D::make_rsrc(scr_wave, (unsigned)(C::scratch_elems * sizeof(R)));
    s.cscr = (unsigned)c * (unsigned)C::scratch_cw;

    // leading all-frozen octets (at most 15: the run must end inside the first 128-leaf subtree)
    int lead = 0;
    while (lead < 15 && ((frz[lead >> 2] >> (8 * (lead & 3))) & 0xFFu) == 0xFFu) ++lead;
    lead = __builtin_amdgcn_readfirstlane(lead);
    const int E = P.fill_end;   // 0: the frozen run and the octets from `lead`; else fill_phase() and the octets from E / 8

    // jobs (pairs of frames): the first one by the wavefront's index, the others from the launch's work queue
    for (int pair = wave_global; 2 * pair < P.B;) {
        const int frame_raw = 2 * pair + c;
        const bool live = frame_raw < P.B;
        const int frame = live ? frame_raw : P.B - 1;  // odd tail: the idle half re-decodes the last frame, no store
        s.rs_in = D::make_rsrc(reinterpret_cast<const IN *>(P.in) + (size_t)(2 * pair) * N, (unsigned)(2 * N * sizeof(IN)));
        s.csrc = (unsigned)(frame - 2 * pair) * (unsigned)N;
        {   // root f, single path per codeword: lanes of codeword c are w = p*4 + pos = 0..31
            const auto t = s.tls();
            const int w = p * 4 + pos;
#pragma unroll 2
            for (int e = w; e < N / 2; e += 32) t[e] = s.chk(s.chv(e), s.chv(e + N / 2));
        }
#pragma unroll
        for (int j = 0; j < NW / 4; ++j) s.blw[D::row(p) + pos + 4 * j] = 0;   // the slot's own row, four lanes to a row
        lds_fence();

        s.PM = R(0);
        s.ptr = 0;
        for (int t = 4; t <= 8; ++t) s.set_pa(t, p);
        for (int t = 5; t <= 9; ++t) s.set_pb(t, p);
        s.bl0 = 0;
        s.a1 = R(0);
#pragma unroll
        for (int r = 0; r < C::NA; ++r) s.A[r] = R(0);
        s.fl = 0;
        s.logact = 0;
        uint32_t fword = 0;

        int o_first = 0;
        if (E > 0 || lead > 0) {
            R xl, yl;
            s.frozen_prefix(E > 0 ? 15 : lead, E > 0 ? 126 : 8 * lead, E == 0, xl, yl);
            o_first = lead;
            if (E > 0) {
                s.fill_phase(E, frz, xl, yl);
                o_first = E >> 3;
            }
            fword = frz[o_first >> 2];
        }
        // Groups of eight octets: level 6 (and the scratch levels) change only at the head of a group, so the inner
        // loop does not carry the 16 level-6 registers as loop-variant values.  (With one loop over all octets the
        // compiler kept them in one register set at the loop header and another behind the head, and copied all of
        // them twice per octet.)
        // The list fills at the third information leaf and stays full.  The groups up to and including that leaf's run
        // the body that can still fill it (a few groups per frame: compiled once, rolled); every group behind them runs
        // the full-list body, in which logact is not read at all.
        int o = o_first;
#pragma unroll 1
        while (o < N / 8 && s.logact < 3) o = octet_group<D, false>(s, frz, fword, o);
        while (o < N / 8) o = octet_group<D, true>(s, frz, fword, o);

        // ---- choose the path, per codeword (SCL_1024.c:667-674; CASCL_1024_L8.c:725-755) ----
        // The CRC remainder is read once, here, so it is computed once, here: it is linear in u_hat = x_hat F^{(x)n}, and
        // every slot's x_hat is in curw since leaf 1023 carried to the root.  Bit i of the remainder is the parity of
        // x_hat AND mask i (h_code.hip make_crc_masks); a lane takes its eight words pos + 4j of the slot's row, and the
        // four lanes of the slot add their parities.  Masks come four at a time (the ones from crc_r up are zero).
        bool pass = false;
        if constexpr (CRC_ON) {
            lds_fence();
            uint32_t x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = s.curw[D::row(p) + pos + 4 * j];
            typedef uint32_t u4_t __attribute__((ext_vector_type(4)));
            const u4_t *mk = reinterpret_cast<const u4_t *>(msk + 8 * pos);
            const int rows = (P.crc_r + 3) & ~3;
            uint32_t rem = 0;
#pragma unroll 1
            for (int i = 0; i < rows; i += 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const u4_t a = mk[(i + k) * (NW / 4)], b = mk[(i + k) * (NW / 4) + 1];
                    const uint32_t acc = (x[0] & a.x) ^ (x[1] & a.y) ^ (x[2] & a.z) ^ (x[3] & a.w) ^ (x[4] & b.x) ^
                                         (x[5] & b.y) ^ (x[6] & b.z) ^ (x[7] & b.w);
                    rem |= (uint32_t)(__popc(acc) & 1) << (i + k);
                }
            }
            rem ^= (uint32_t)dpp_i<0xB1>((int)rem);   // quad_perm [1,0,3,2]
            rem ^= (uint32_t)dpp_i<0x4E>((int)rem);   // quad_perm [2,3,0,1]
            pass = rem == 0u;
        }
        const uint64_t bp_ = __ballot(pass && pos == 0);
        // lanes of codeword c at pos 0 are lanes p*8 + 4c: bits 4c, 8+4c, ...
        const uint64_t cwmask = 0x0101010101010101ull << (4 * c);
        const bool any = (bp_ & cwmask) != 0ull;
        int best = -1;
        R best_pm = R(0);
        for (int q = 0; q < L; ++q) {
            const R pq = __shfl(s.PM, q * 8 + 4 * c);
            const int okq = __shfl((int)(any ? pass : true), q * 8 + 4 * c);
            if (okq && (best < 0 || pq < best_pm)) {
                best = q;
                best_pm = pq;
            }
        }
        uint32_t fl = s.fl;
        if (any) fl |= 0x2u;
        // x_hat = root partial sums of the winner; u_hat = x_hat F^{(x)n}; word index w = p*4 + pos per codeword
        lds_fence();
        {
            const int w = p * 4 + pos;
            uint32_t x = s.curw[D::row(best) + w];
            x = polar_word_transform(x);
#pragma unroll
            for (int hw = 1; hw < NW; hw <<= 1) {
                const int wo = w ^ hw;  // partner word; the lower one of the pair absorbs the upper one
                const uint32_t ov = __shfl(x, (wo >> 2) * 8 + 4 * c + (wo & 3));
                if (!(w & hw)) x ^= ov;
            }
            if (live) P.out_bits[(size_t)frame * NW + w] = x;
        }
        if (live && p == 0 && pos == 0) {
            if (P.pm) P.pm[frame] = (double)best_pm;
            if (P.flags) P.flags[frame] = fl;
        }
        lds_fence();
        pair = next_job_wave(P.queue, pair, waves_total, (P.B + 1) >> 1);
    }
}

// k_scl_fast2: the input rows are LLRs (P.sigma is not read).  k_scl_fast2_y: they are y, P.sigma > 0.  The host picks by
// P.sigma (k_fast2.hip).
template <typename R, typename IN, bool CRC_ON>
__global__ __launch_bounds__(256, (Fast2Cfg<R>::MIN_WAVES_PER_SIMD)) void k_scl_fast2(SclParams P)
{
    scl_fast2_body<R, IN, CRC_ON, false>(P);
}
template <typename R, typename IN, bool CRC_ON>
__global__ __launch_bounds__(256, (Fast2Cfg<R>::MIN_WAVES_PER_SIMD)) void k_scl_fast2_y(SclParams P)
{
    scl_fast2_body<R, IN, CRC_ON, true>(P);
}

}  // namespace polar
