// k_rm.hip -- 5G NR rate matching kernels (rm_kernel.h) and their launch code
#include "polar_host.h"
#include "rm_kernel.h"

namespace {

template <typename IN>
int launch_recover(polar_ctx *c, const polar::RmParams &P)
{
    auto kern = polar::k_rm_recover<IN>;
    const size_t lds = polar::rm_recover_lds(P.E, P.ilv != nullptr, sizeof(IN));
    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    int occ = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, polar::RM_THREADS, lds));
    if (occ < 1) occ = 1;
    const int grid = stride_grid(c, P.B, (long long)occ * c->num_cu);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(polar::RM_THREADS), lds, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}

int log2i(int v)
{
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

}  // namespace

int polar_tu::rm_recover(polar_ctx *c, const void *d_in, bool in32, double sigma, size_t B, void *d_out)
{
    if (B == 0) return POLAR_OK;
    polar::RmParams P{};
    P.in = d_in; P.out = d_out; P.ilv = c->rm_ibil ? c->d_rm_ilv : nullptr;
    P.sigma = sigma;
    P.N = c->cfg.N; P.logS = log2i(c->cfg.N / 32); P.E = c->rm_E; P.B = (int)B;
    P.mode = c->rm_mode;
    P.out_vec = (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
    return in32 ? launch_recover<float>(c, P) : launch_recover<double>(c, P);
}

int polar_tu::rm_generate(polar_ctx *c, const polar::GenParams &G)
{
    polar::GenRmParams R{};
    R.g = G;
    R.ilv_inv = c->rm_ibil ? c->d_rm_ilv_inv : nullptr;
    R.E = c->rm_E; R.logS = log2i(c->cfg.N / 32); R.mode = c->rm_mode;
    const int waves = 4;
    const size_t lds = (size_t)waves * (G.N + 2 * 1024);
    const int grid = stride_grid(c, ((long long)G.B + waves - 1) / waves, (long long)c->num_cu * 8);
    hipLaunchKernelGGL(polar::k_generate_rm, dim3(grid), dim3(64 * waves), lds, c->stream, R);
    HIP_TRY(c, hipGetLastError());
    return POLAR_OK;
}
