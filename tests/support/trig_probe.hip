// tests/support/trig_probe.hip -- TEST INFRASTRUCTURE: the device's gf_sinf / gf_cosf / gf_asinf (icar_amd/csrc/glibc_flt32_trig.h)
// evaluated on an array of REAL(4) arguments, for tests/test_gpu_trig_math.py.  Built by tests/support/build_trig_probe.py with
// the product's compile flags.
#include <hip/hip_runtime.h>
#include "glibc_flt32_trig.h"

__global__ void k_trig_probe(int op, size_t n, const float *__restrict__ x, float *__restrict__ y)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const float v = x[t];
    y[t] = op == 0 ? gf_sinf(v) : op == 1 ? gf_cosf(v) : gf_asinf(v);
}

// op: 0 sinf, 1 cosf, 2 asinf; x, y: host arrays of n floats.  Returns 0 or the HIP error code.
extern "C" int icar_trig_probe(int op, long n, const float *x, float *y)
{
    if (op < 0 || op > 2 || n <= 0 || !x || !y) return -1;
    float *dx = nullptr, *dy = nullptr;
    hipError_t e = hipMalloc(&dx, (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dy, (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_trig_probe, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, 0, op, (size_t)n, dx, dy);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(y, dy, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    if (dx) hipFree(dx);
    if (dy) hipFree(dy);
    return (int)e;
}
