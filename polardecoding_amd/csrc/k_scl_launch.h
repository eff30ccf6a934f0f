// k_scl_launch.h -- launch code of scl_generic_body's kernels and of k_scl_wide, shared by k_generic.hip (k_scl_generic),
// k_dyn.hip (k_scl_dyn), k_wide.hip (k_scl_wide: its own ladder over L, launch_scl below it) and k_list.hip (their LIST
// instantiations), one translation unit each, compiled in parallel.  Each names its kernel in a trait K:
//     K::Params                                  the kernel's parameter struct
//     K::kernel<R, IN, LOGL, GA>()               the instantiation
//     K::lds_bytes<R, LOGL>(N, ga)               its dynamic LDS
//     K::scl(Params &)                           the SclParams inside the parameter struct
//     K::Wide (optional)                         the trait of the k_scl_wide instantiation that takes L = 64, 128, 256 for K
// The parameter struct travels down the ladder by value; launch_scl_v fills in scratch and queue.
#pragma once
#include "polar_host.h"

#include <type_traits>

namespace {

template <typename K, typename R, typename IN, int LOGL, bool GA>
int launch_scl_v(polar_ctx *c, typename K::Params Q)
{
    auto kern = K::template kernel<R, IN, LOGL, GA>();
    polar::SclParams &S = K::scl(Q);
    const size_t lds = K::template lds_bytes<R, LOGL>(S.N, GA);
    if (lds > 160 * 1024) return POLAR_ENOKERNEL;
    constexpr int threads = LOGL > 6 ? 1 << LOGL : 64;   // one wavefront; k_scl_wide: one thread per path
    LaunchShape s{threads, lds, S.B, 1};
    if (GA) {   // the levels in global scratch: at most 8 blocks per CU
        s.scratch_per_block = sizeof(R) * (size_t)((1 << LOGL) + 1) * S.N;
        s.occ_cap = 8;
    }
    LaunchPlan pl;
    int rc = plan_launch(c, reinterpret_cast<const void *>(kern), s, &pl);
    if (rc) return rc;
    if (GA) S.scratch = pl.scratch;
    S.queue = pl.queue;   // the counter hangs off c->scratch with or without scratch bytes
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(threads), lds, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

template <typename K, typename R, typename IN, int LOGL>
int launch_scl(polar_ctx *c, typename K::Params P)
{
    if (K::template lds_bytes<R, LOGL>(K::scl(P).N, false) <= 160 * 1024 && !c->force_spill)
        return launch_scl_v<K, R, IN, LOGL, false>(c, P);
    return launch_scl_v<K, R, IN, LOGL, true>(c, P);
}

template <typename K, typename = void>
struct WideOf {
    static constexpr bool present = false;
};
template <typename K>
struct WideOf<K, std::void_t<typename K::Wide>> {
    static constexpr bool present = true;
};

template <typename K, typename R, typename IN>
int launch_scl_l(polar_ctx *c, typename K::Params P)
{
    if constexpr (WideOf<K>::present) {
        switch (c->logL) {
        case 6: return launch_scl<typename K::Wide, R, IN, 6>(c, P);
        case 7: return launch_scl<typename K::Wide, R, IN, 7>(c, P);
        case 8: return launch_scl<typename K::Wide, R, IN, 8>(c, P);
        }
    }
    switch (c->logL) {
    case 0: return launch_scl<K, R, IN, 0>(c, P);
    case 1: return launch_scl<K, R, IN, 1>(c, P);
    case 2: return launch_scl<K, R, IN, 2>(c, P);
    case 3: return launch_scl<K, R, IN, 3>(c, P);
    case 4: return launch_scl<K, R, IN, 4>(c, P);
    case 5: return launch_scl<K, R, IN, 5>(c, P);
    }
    return POLAR_ENOKERNEL;
}

template <typename K>
int launch_scl_types(polar_ctx *c, typename K::Params P, bool r32, bool in32)
{
    if (r32) return in32 ? launch_scl_l<K, float, float>(c, P) : launch_scl_l<K, float, double>(c, P);
    return in32 ? launch_scl_l<K, double, float>(c, P) : launch_scl_l<K, double, double>(c, P);
}

}  // namespace
