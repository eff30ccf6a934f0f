// k_book.hip -- code books (include/polar_hip.h, "Code books"): k_scl_book and k_scl_book_list (scl_book.h) and their launch
// code.  c is the code book's internal context: the largest member's N and the book's L, stream, scratch and work queue.
#include "k_scl_launch.h"
#include "scl_book.h"

namespace {

struct BookKernel {
    using Params = polar::BookParams;
    template <typename R, typename IN, int LOGL, bool GA>
    static auto kernel() { return polar::k_scl_book<R, IN, LOGL, GA>; }
    template <typename R, int LOGL>
    static constexpr size_t lds_bytes(int N, bool ga) { return polar::scl_dyn_lds_bytes<R, LOGL>(N, ga); }
    static polar::SclParams &scl(Params &P) { return P.s; }
};

struct BookListKernel {
    using Params = polar::BookParams;
    template <typename R, typename IN, int LOGL, bool GA>
    static auto kernel() { return polar::k_scl_book_list<R, IN, LOGL, GA>; }
    template <typename R, int LOGL>
    static constexpr size_t lds_bytes(int N, bool ga) { return polar::scl_dyn_lds_bytes<R, LOGL>(N, ga); }
    static polar::SclParams &scl(Params &P) { return P.s; }
};

}  // namespace

int polar_tu::book_decode(polar_ctx *c, const polar::SclParams &S, const polar::BookArgs &K, bool r32, bool in32)
{
    polar::BookParams P{};
    P.s = S;
    P.k = K;
    return launch_scl_types<BookKernel>(c, P, r32, in32);
}

int polar_tu::book_list(polar_ctx *c, const polar::SclParams &S, const polar::BookArgs &K, bool r32, bool in32, uint32_t *d_paths,
                        double *d_pm, uint32_t *d_rem, uint32_t *d_count)
{
    polar::BookParams P{};
    P.s = S;
    P.k = K;
    P.o = polar::ListOut{d_paths, d_pm, d_rem, d_count};
    return launch_scl_types<BookListKernel>(c, P, r32, in32);
}
