// k_wide.hip -- wide lists, L = 64 / 128 / 256: k_scl_wide (scl_wide.h), plain and with dynamic frozen bits, and its launch code
#include "k_scl_launch.h"
#include "scl_wide.h"

namespace {

template <bool DYN>
struct WideKernel {
    using Params = polar::DynParams;
    template <typename R, typename IN, int LOGL, bool GA>
    static auto kernel() { return polar::k_scl_wide<R, IN, LOGL, GA, DYN>; }
    template <typename R, int LOGL>
    static constexpr size_t lds_bytes(int N, bool ga) { return polar::WideLds<R, LOGL, DYN>::bytes(N, ga); }
    static polar::SclParams &scl(Params &P) { return P.s; }
};

template <typename K, typename R, typename IN>
int launch_wide_l(polar_ctx *c, typename K::Params P)
{
    switch (c->logL) {
    case 6: return launch_scl<K, R, IN, 6>(c, P);
    case 7: return launch_scl<K, R, IN, 7>(c, P);
    case 8: return launch_scl<K, R, IN, 8>(c, P);
    }
    return POLAR_ENOKERNEL;
}

template <typename K>
int launch_wide_types(polar_ctx *c, typename K::Params P, bool r32, bool in32)
{
    if (r32) return in32 ? launch_wide_l<K, float, float>(c, P) : launch_wide_l<K, float, double>(c, P);
    return in32 ? launch_wide_l<K, double, float>(c, P) : launch_wide_l<K, double, double>(c, P);
}

}  // namespace

int polar_tu::scl_wide(polar_ctx *c, const polar::SclParams &S, bool r32, bool in32)
{
    if ((long long)c->logL * c->n > 64) return POLAR_ENOKERNEL;   // the 64-bit pointer table holds LOGL bits per level
    polar::DynParams P{};
    P.s = S;
    if (c->is_dyn) {
        P.mask = c->d_dyn_mask;
        P.row = c->d_dyn_row;
        return launch_wide_types<WideKernel<true>>(c, P, r32, in32);
    }
    return launch_wide_types<WideKernel<false>>(c, P, r32, in32);
}
