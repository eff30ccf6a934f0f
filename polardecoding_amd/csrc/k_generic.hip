// k_generic.hip -- k_scl_generic (correctness baseline, short codes, single-frame SC) and its launch code
#include "k_scl_launch.h"
#include "scl_generic.h"

namespace {

struct GenericKernel {
    using Params = polar::SclParams;
    template <typename R, typename IN, int LOGL, bool GA>
    static auto kernel() { return polar::k_scl_generic<R, IN, LOGL, GA>; }
    template <typename R, int LOGL>
    static constexpr size_t lds_bytes(int N, bool ga) { return polar::scl_generic_lds_bytes<R, LOGL>(N, ga); }
    static polar::SclParams &scl(Params &P) { return P; }
};

}  // namespace

int polar_tu::scl_generic(polar_ctx *c, const polar::SclParams &P, bool r32, bool in32)
{
    return launch_scl_types<GenericKernel>(c, P, r32, in32);
}
