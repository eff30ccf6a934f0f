// k_probe.hip -- polar_testing_math: the kernels' scalar arithmetic on caller-chosen operands.  TEST LIBRARY ONLY
// (libpolar_hip_testing.so, include/polar_hip_testing.h).
#include "polar_host.h"
#include "../../include/polar_hip_testing.h"
#include "probe_kernel.h"

#ifndef POLAR_TESTING
#error "k_probe.hip belongs to libpolar_hip_testing.so (-DPOLAR_TESTING)"
#endif

extern "C" {

int polar_testing_math(int op, int is_f32, const void *a, const void *b, void *out, size_t n, int device)
{
    if (op < 0 || op > polar::PROBE_CHK_TAB || !a || !b || !out) return POLAR_EINVAL;
    if (n == 0) return POLAR_OK;
    DeviceGuard guard(device);
    const size_t es = is_f32 ? 4 : 8;
    DevMem<char> da, db, d_out;
    int rc = POLAR_OK;
    if (da.alloc(n * es) != hipSuccess || db.alloc(n * es) != hipSuccess || d_out.alloc(n * es) != hipSuccess) rc = POLAR_ENOMEM;
    if (!rc && (hipMemcpy(da, a, n * es, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(db, b, n * es, hipMemcpyHostToDevice) != hipSuccess))
        rc = POLAR_EDEVICE;
    if (!rc) {
        const int grid = (int)std::min<size_t>((n + 255) / 256, 1024);
        if (is_f32)
            hipLaunchKernelGGL(polar::k_probe_math<float>, dim3(grid), dim3(256), polar::Lut<float>::bytes + 16 + 64 * sizeof(float) + polar::Stair<float>::bytes, 0, op,
                               (const float *)da.get(), (const float *)db.get(), (float *)d_out.get(), n);
        else
            hipLaunchKernelGGL(polar::k_probe_math<double>, dim3(grid), dim3(256), polar::Lut<double>::bytes + 16 + 64 * sizeof(double) + polar::Stair<double>::bytes, 0, op,
                               (const double *)da.get(), (const double *)db.get(), (double *)d_out.get(), n);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out, d_out, n * es, hipMemcpyDeviceToHost) != hipSuccess)
            rc = POLAR_EDEVICE;
    }
    return rc;
}

}  // extern "C"
