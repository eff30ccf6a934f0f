// k_trace.hip -- sent-path trace (include/polar_hip.h, "Sent-path trace"): the TRACE instantiations of scl_generic_body
// (k_scl_trace) and k_scl_wide, the reduce kernel k_trace_count and their launch code.  The decode is the list decode of
// k_list.hip: the same ladder over L, the same LDS sizes, the same limit of the 64-bit pointer table.
#include "k_scl_launch.h"
#include "scl_wide.h"

namespace polar {

template <typename R, typename IN, int LOGL, bool GA>
__global__ __launch_bounds__(64) void k_scl_trace(TraceParams TP)
{
    scl_generic_body<R, IN, LOGL, GA, true, false, false, true>(TP.d.s, TP.d.mask, TP.d.row, nullptr, nullptr, &TP.t);
}

// Rule 8.  One thread per frame: hist[loss_leaf] += 1 for a lost frame, hist[N + class] and hist[N + 3] by one atomic per
// wavefront and counter.  Every thread of a block reaches the ballots; a thread past B contributes nothing.  loss_leaf comes
// from device memory: it is compared with N before an address is formed from it.
__global__ __launch_bounds__(256) void k_trace_count(const int32_t *loss_leaf, const int32_t *rank, const int32_t *chosen, int N,
                                                     size_t B, unsigned long long *hist)
{
    const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = f < B;
    const int32_t ll = in ? loss_leaf[f] : N;
    const int32_t rk = in ? rank[f] : 0;
    const int32_t ch = in ? chosen[f] : 0;
    if (in && ll >= 0 && ll < N) atomicAdd(&hist[ll], 1ull);
    const int cls = rk < 0 ? 2 : (rk == ch ? 0 : 1);
    const unsigned long long n0 = (unsigned long long)__popcll(__ballot(in && cls == 0));
    const unsigned long long n1 = (unsigned long long)__popcll(__ballot(in && cls == 1));
    const unsigned long long n2 = (unsigned long long)__popcll(__ballot(in && cls == 2));
    if ((threadIdx.x & 63) == 0) {
        if (n0) atomicAdd(&hist[N + 0], n0);
        if (n1) atomicAdd(&hist[N + 1], n1);
        if (n2) atomicAdd(&hist[N + 2], n2);
        if (n0 + n1 + n2) atomicAdd(&hist[N + 3], n0 + n1 + n2);
    }
}

}  // namespace polar

namespace {

// the reduction words of the wide kernel sit in WideLds::MISC_WORDS, which the LIST kernels carry too
struct WideTraceKernel {
    using Params = polar::TraceParams;
    template <typename R, typename IN, int LOGL, bool GA>
    static auto kernel() { return polar::k_scl_wide<R, IN, LOGL, GA, true, false, true>; }
    template <typename R, int LOGL>
    static constexpr size_t lds_bytes(int N, bool ga) { return polar::WideLds<R, LOGL, true>::bytes(N, ga); }
    static polar::SclParams &scl(Params &P) { return P.d.s; }
};

struct TraceKernel {
    using Params = polar::TraceParams;
    using Wide = WideTraceKernel;   // launch_scl_l's ladder goes on to L = 64, 128, 256
    template <typename R, typename IN, int LOGL, bool GA>
    static auto kernel() { return polar::k_scl_trace<R, IN, LOGL, GA>; }
    template <typename R, int LOGL>
    static constexpr size_t lds_bytes(int N, bool ga) { return polar::scl_dyn_lds_bytes<R, LOGL>(N, ga); }
    static polar::SclParams &scl(Params &P) { return P.d.s; }
};

}  // namespace

int polar_tu::list_trace(polar_ctx *c, const polar::SclParams &S, const uint32_t *d_mask, const int *d_row, bool r32, bool in32,
                         const polar::TraceOut &T)
{
    if ((long long)c->logL * c->n > 64) return POLAR_ENOKERNEL;   // the 64-bit pointer table holds LOGL bits per level
    polar::TraceParams P{};
    P.d.s = S;
    P.d.mask = d_mask;
    P.d.row = d_row;
    P.t = T;
    return launch_scl_types<TraceKernel>(c, P, r32, in32);
}

int polar_tu::trace_count(polar_ctx *c, const int32_t *d_loss_leaf, const int32_t *d_rank, const int32_t *d_chosen, size_t B,
                          unsigned long long *d_hist)
{
    const int blocks = (int)((B + 255) / 256);
    hipLaunchKernelGGL(polar::k_trace_count, dim3(blocks), dim3(256), 0, c->stream, d_loss_leaf, d_rank, d_chosen, c->cfg.N, B,
                       d_hist);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
