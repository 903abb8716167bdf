// tests/support/tanf_probe.hip -- TEST INFRASTRUCTURE: the device's gf_tanf (icar_amd/csrc/glibc_flt32_tan.h) evaluated on an
// array of REAL(4) arguments, for tests/test_gpu_tanf_math.py.  Built by tests/support/build_tanf_probe.py with the product's
// compile flags.
#include <hip/hip_runtime.h>
#include "glibc_flt32_tan.h"

__global__ void k_tanf_probe(size_t n, const float *__restrict__ x, float *__restrict__ y)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    y[t] = gf_tanf(x[t]);
}

// x, y: host arrays of n floats.  Returns 0 or the HIP error code.
extern "C" int icar_tanf_probe(long n, const float *x, float *y)
{
    if (n <= 0 || !x || !y) return -1;
    float *dx = nullptr, *dy = nullptr;
    hipError_t e = hipMalloc(&dx, (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dy, (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tanf_probe, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, 0, (size_t)n, dx, dy);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(y, dy, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    if (dx) hipFree(dx);
    if (dy) hipFree(dy);
    return (int)e;
}
