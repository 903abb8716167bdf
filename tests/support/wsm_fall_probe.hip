// tests/support/wsm_fall_probe.hip -- TEST INFRASTRUCTURE, NOT PRODUCT: the semi-Lagrangian fall of WSM3 / WSM6
// (icar_amd/csrc/wsm_fall.h: the very header mp_wsm3.hip and mp_wsm6.hip compile) on independent columns, in either of its forms,
// so that tests/test_gpu_wsm_fall.py can compare each form with the oracle's fall (oracle/wsm6_oracle.c: orc_wsm_fall_column) and
// with the other one, column by column.  The refinement of the speed is the oracle's probe_speed: +, *, / and sqrt only.
#include <hip/hip_runtime.h>
#include "wsm_fall.h"

namespace {
template <int NF>
struct ProbeSpeed {
    __device__ __forceinline__ float operator()(const float *q, float den, float denfac, float tk) const
    {
        const float q2 = NF == 2 ? q[NF - 1] : 0.0f;
        const float s = q[0] + (q2 + q2);
        return denfac * 60.f * sqrtf(sqrtf(s * den)) * (tk / 273.f);
    }
};

// column c of an array of ncol columns of km levels sits at [c * km, (c + 1) * km); field f of rql / out at f * ncol * km
template <int NF>
__global__ void __launch_bounds__(64)
k_probe_fall_serial(int ncol, int km, int iter, const float *__restrict__ den, const float *__restrict__ denfac, const float *__restrict__ tk,
                    const float *__restrict__ dz, const float *__restrict__ ww, const float *__restrict__ dt, float *__restrict__ out,
                    float *__restrict__ precip)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncol) return;
    const size_t c0 = (size_t)c * km, nf = (size_t)ncol * km;
    float *rql[NF]; float pr[NF];
    for (int f = 0; f < NF; ++f) rql[f] = out + f * nf + c0;
    wsm_fall_column<NF>(km, 1, den + c0, denfac + c0, tk + c0, dz + c0, ww + c0, rql, dt[c], iter, ProbeSpeed<NF>{}, pr);
    for (int f = 0; f < NF; ++f) precip[f * ncol + c] = pr[f];
}

// zi of the wave form: the running sum of dz, as wsm_zi_column forms it (zi[k] = height of interface k + 1)
__global__ void __launch_bounds__(64)
k_probe_zi(int ncol, int km, const float *__restrict__ dz, float *__restrict__ zi)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncol) return;
    float run = 0.0f;
    for (int k = 0; k < km; ++k) { run = run + dz[(size_t)c * km + k]; zi[(size_t)c * km + k] = run; }
}

// one wave per column, four columns per block; the operands reach the lanes as in k_w6_fall_tile / k_wsm3_fall_tile
template <int NF>
__global__ void __launch_bounds__(256)
k_probe_fall_wave(int ncol, int km, int iter, const float *__restrict__ den, const float *__restrict__ denfac, const float *__restrict__ tk,
                  const float *__restrict__ dz, const float *__restrict__ ww, const float *__restrict__ zi_, const float *__restrict__ dt,
                  float *__restrict__ out, float *__restrict__ precip)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + wave;
    if (c >= ncol) return;                                           // wave-uniform
    const size_t c0 = (size_t)c * km, nf = (size_t)ncol * km;
    const int kl = lane < km ? lane : km - 1;                        // lanes beyond the column read a valid level (values unused)
    const int kz = (lane <= km ? lane : km) - 1;
    const float zi = lane == 0 ? 0.0f : zi_[c0 + kz];
    float rql[NF], qn[NF], pr[NF];
    for (int f = 0; f < NF; ++f) rql[f] = out[f * nf + c0 + kl];
    wsm_fall_wave<NF>(km, lane, dz[c0 + kl], den[c0 + kl], denfac[c0 + kl], tk[c0 + kl], ww[c0 + kl], rql, zi, dt[c], iter, ProbeSpeed<NF>{}, qn, pr);
    for (int f = 0; f < NF; ++f) {
        if (lane < km) out[f * nf + c0 + lane] = qn[f];
        if (lane == 0) precip[f * ncol + c] = pr[f];
    }
}
#define CKF(x) do { if ((x) != hipSuccess) { rc = 2; goto done; } } while (0)
}  // namespace

extern "C" {
// form 0: wsm_fall_column (one thread per column, 3 .. 64 levels), 1: wsm_fall_wave (one wave per column, 3 .. 63 levels: km + 1
// interfaces on 64 lanes).  Host arrays: den, denfac, tk, dz, ww [ncol][km]; rql, out [nf][ncol][km] (den*q before and after);
// dt [ncol]; precip [nf][ncol].  Returns 0, 1 (bad arguments), 2 (HIP error) or 3 (km outside the form's range: nothing is
// launched and the outputs are not written).
int icar_probe_wsm_fall(int form, int ncol, int km, int nf, int iter, const float *den, const float *denfac, const float *tk, const float *dz,
                        const float *ww, const float *rql, const float *dt, float *out, float *precip)
{
    if (form < 0 || form > 1 || nf < 1 || nf > 2 || iter < 0 || iter > 1 || ncol < 0 || !den || !denfac || !tk || !dz || !ww || !rql || !dt || !out || !precip) return 1;
    if (km < 3 || km > (form == 1 ? 63 : WSM_MAXK)) return 3;
    if (ncol == 0) return 0;
    const size_t n = (size_t)ncol * km * sizeof(float);
    float *d[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, *dout = nullptr, *dpr = nullptr;   // den denfac tk dz ww zi dt
    const float *h[5] = {den, denfac, tk, dz, ww};
    int rc = 0;
    for (int a = 0; a < 5; ++a) { CKF(hipMalloc(&d[a], n)); CKF(hipMemcpy(d[a], h[a], n, hipMemcpyHostToDevice)); }
    if (form == 1) CKF(hipMalloc(&d[5], n));                 // zi: the wave form alone reads it
    CKF(hipMalloc(&d[6], ncol * sizeof(float))); CKF(hipMemcpy(d[6], dt, ncol * sizeof(float), hipMemcpyHostToDevice));
    CKF(hipMalloc(&dout, nf * n)); CKF(hipMemcpy(dout, rql, nf * n, hipMemcpyHostToDevice));
    CKF(hipMalloc(&dpr, (size_t)nf * ncol * sizeof(float))); CKF(hipMemset(dpr, 0, (size_t)nf * ncol * sizeof(float)));
    if (form == 0) {
        const dim3 g((ncol + 63) / 64), b(64);
        if (nf == 1) hipLaunchKernelGGL(k_probe_fall_serial<1>, g, b, 0, 0, ncol, km, iter, d[0], d[1], d[2], d[3], d[4], d[6], dout, dpr);
        else         hipLaunchKernelGGL(k_probe_fall_serial<2>, g, b, 0, 0, ncol, km, iter, d[0], d[1], d[2], d[3], d[4], d[6], dout, dpr);
    } else {
        hipLaunchKernelGGL(k_probe_zi, dim3((ncol + 63) / 64), dim3(64), 0, 0, ncol, km, d[3], d[5]);
        const dim3 g((ncol + 3) / 4), b(256);
        if (nf == 1) hipLaunchKernelGGL(k_probe_fall_wave<1>, g, b, 0, 0, ncol, km, iter, d[0], d[1], d[2], d[3], d[4], d[5], d[6], dout, dpr);
        else         hipLaunchKernelGGL(k_probe_fall_wave<2>, g, b, 0, 0, ncol, km, iter, d[0], d[1], d[2], d[3], d[4], d[5], d[6], dout, dpr);
    }
    CKF(hipGetLastError()); CKF(hipDeviceSynchronize());
    CKF(hipMemcpy(out, dout, nf * n, hipMemcpyDeviceToHost));
    CKF(hipMemcpy(precip, dpr, (size_t)nf * ncol * sizeof(float), hipMemcpyDeviceToHost));
done:
    for (float *p : d) if (p) (void)hipFree(p);
    if (dout) (void)hipFree(dout);
    if (dpr) (void)hipFree(dpr);
    return rc;
}
}
