/* tests/support/tanf_host.c -- TEST INFRASTRUCTURE: the host C library's tanf on an array of REAL(4) arguments: what the
   compiled reference's TAN evaluates to, for tests/test_gpu_tanf_math.py.  Built by tests/support/build_tanf_probe.py. */
#include <math.h>

void icar_tanf_host(long n, const float *x, float *y)
{
    for (long i = 0; i < n; ++i) y[i] = tanf(x[i]);
}
