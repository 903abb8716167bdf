// icar_amd/csrc/cfl.hip -- row T2: the CFL reductions of compute_dt (time_step.f90:238-305) and the bookkeeping of the
// maximum that is taken ahead of time (icar_hip_max_courant_prefetch).  Consumers: timestep.hip and the icar_hip_max_* entry points.
#include "ctx.h"
#include "comm.h"
#include <cstring>

// ------------------------------------------------------------------------------------------------
// T2: compute_dt strictness-3 reduction (time_step.f90:264-289)
// ------------------------------------------------------------------------------------------------
// One thread per (i, j) column, levels marched in registers (|w| of the level below is carried), raw buffer loads with scalar
// row / level offsets: at most 16 VGPRs (the attribute counts half of the unified file), so that the prefetched reduction
// finds a wave slot on EVERY SIMD beside the MPDATA launch it is issued next to (whose persistent blocks leave 16 registers per
// SIMD; the former grid-stride kernel needed 61 and ran on the 13 idle CUs only: 0.38 ms in the advection's shadow).
__global__ void __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(8)))
k_max_courant(Dims d, const float *__restrict__ u, const float *__restrict__ v,
              const float *__restrict__ w, const float *__restrict__ dzl, float dx,
              unsigned *__restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    typedef __amdgpu_buffer_rsrc_t rsrc_t;
    auto mk = [](const float *p) { return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, -1, 0x00020000); };
    const rsrc_t ru = mk(u), rv = mk(v), rw = mk(w);
    auto ld = [](rsrc_t r, int voff, int soff) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0)); };
    float cur = 0.0f;
    bool nan_wind = false;                                       // (a lane mask: scalar registers)
    if (i < d.nx) {
        const int vi = 4 * i, nxu = d.nx + 1;
        float wbelow = 0.0f;
#pragma unroll 1
        for (int k = 0; k < d.nz; ++k) {
            const int sc = 4 * d.idx(0, k, j), scu = 4 * (nxu * (k + d.nz * j));     // wave-uniform
            const float u0 = fabsf(ld(ru, vi, scu)), u1 = fabsf(ld(ru, vi, scu + 4));
            const float v0 = fabsf(ld(rv, vi, sc)), v1 = fabsf(ld(rv, vi, sc + 4 * d.sj));
            const float au = fmaxf(u0, u1);
            const float av = fmaxf(v0, v1);
            const float aw0 = fabsf(ld(rw, vi, sc));
            const float aw = (k == 0) ? aw0 : fmaxf(aw0, wbelow);                     // (level 0 looks at itself, :281)
            const float cw = au / dx + av / dx + aw / dzl[k];
            cur = fmaxf(cur, cw);
            wbelow = aw0;
            // fmaxf returns its other argument when one is NaN (as the reference's MAX does): a NaN wind would leave no trace in
            // the maximum.  A sum of magnitudes is NaN exactly when one of them is (inf + inf is inf)
            const float probe = (u0 + u1) + (v0 + v1) + aw0;
            nan_wind |= probe != probe;
        }
    }
    // non-negative floats order like unsigned ints, and the quiet NaN lies above +inf: a column with a NaN wind makes the maximum NaN
    // (compute_dt reports it)
    unsigned b = nan_wind ? 0x7fc00000u : __float_as_uint(cur);
    for (int o = 32; o > 0; o >>= 1) { const unsigned x = __shfl_down(b, o); b = x > b ? x : b; }
    if (threadIdx.x == 0) atomicMax(out, b);
}

// out != nullptr: the maximum is copied to the host (one stream synchronisation).  d_out != nullptr: it is left in device
// memory at d_out (a REAL(4) the caller owns) and nothing waits -- the caller all-reduces it on the device (co_min of
// time_step.f90:413 as max over images of the Courant sum: dt = factor / max is monotone, so min(dt) == factor / max).
// A maximum taken ahead of time (icar_hip_max_courant_prefetch, typically on the second stream beside the advection) is
// handed out instead of a new reduction as long as no entry point has written u, v or w since and the arguments are the same.
static bool cfl_prefetched(icar_hip_ctx *c, float dx, const float *dz_levels)
{
    return c->cfl_pre.valid && !c->wind_ptr_escaped && c->cfl_pre.ver == c->wind_version && c->cfl_pre.dx == dx
        && (int)c->cfl_pre.dzl.size() == c->d.nz && memcmp(c->cfl_pre.dzl.data(), dz_levels, sizeof(float) * c->d.nz) == 0;
}

int icar_max_courant_run(icar_hip_ctx *c, float dx, const float *dz_levels, float *out, float *d_out)
{
    if (cfl_prefetched(c, dx, dz_levels) && !c->cfl_pre.reduced) {      // (a value already reduced over the images is not this tile's)
        c->cfl_pre.valid = false;
        if (out) { HIPCHK(hipEventSynchronize(c->cfl_ev)); *out = *c->h_cfl_pre; }
        else {
            HIPCHK(hipStreamWaitEvent(c->stream, c->cfl_ev, 0));
            HIPCHK(hipMemcpyAsync(d_out, c->d_red + 8, sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        }
        return 0;
    }
    c->cfl_pre.valid = false;
    const float *u = icar_field_f(c, ICAR_F_U), *v = icar_field_f(c, ICAR_F_V), *w = icar_field_f(c, ICAR_F_W);
    if (!u || !v || !w) return 1;
    float *dzl = c->d_red + 16;
    if ((int)c->dzl_host.size() != c->d.nz || memcmp(c->dzl_host.data(), dz_levels, sizeof(float) * c->d.nz) != 0) {
        c->dzl_host.assign(dz_levels, dz_levels + c->d.nz);      // the copy source must outlive the async copy
        HIPCHK(hipMemcpyAsync(dzl, c->dzl_host.data(), sizeof(float) * c->d.nz, hipMemcpyHostToDevice, c->stream));
    }
    float *red = d_out ? d_out : c->d_red;
    HIPCHK(hipMemsetAsync(red, 0, sizeof(float), c->stream));
    if ((size_t)(c->d.nx + 1) * c->d.nz * (c->d.ny + 1) * sizeof(float) >= ((size_t)1 << 31)) { icar_set_error("max_courant: a field of 2 GiB or more is not supported (32-bit buffer offsets)"); return 1; }
    dim3 g((c->d.nx + 63) / 64, c->d.ny), b(64);
    ScopedTimer t(c, "cfl");
    hipLaunchKernelGGL(k_max_courant, g, b, 0, c->stream, c->d, u, v, w, dzl, dx, (unsigned *)red);
    HIPCHK(hipGetLastError());
    if (out) {
        HIPCHK(hipMemcpyAsync(out, red, sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// the prefetched maximum, if it is still valid AND was already reduced over the images on the device (allreduce = true below):
// consumes it; the host waits for the second stream's copy only
bool icar_cfl_prefetch_waiting(icar_hip_ctx *c)
{
    return c->step.configured && cfl_prefetched(c, c->step.cfg.dx, c->step.dz_levels.data());
}

bool icar_cfl_prefetched_global(icar_hip_ctx *c, float dx, const float *dz_levels, float *value)
{
    if (!cfl_prefetched(c, dx, dz_levels) || !c->cfl_pre.reduced) return false;
    c->cfl_pre.valid = false;
    // (a failed wait is an error of this image alone; falling back to a fresh reduction here would issue an all-reduce the other
    // images do not pair -- the value is handed out as NaN and compute_dt reports it)
    if (hipEventSynchronize(c->cfl_ev) != hipSuccess) { *value = __builtin_nanf(""); c->cfl_wait_failed = true; return true; }
    *value = *c->h_cfl_pre;
    return true;
}

// allreduce: with the RCCL transport the tile maximum is all-reduced (MAX) over the images right here, on the current (second)
// stream in the advection's shadow, so that the next update_dt finds the GLOBAL maximum waiting instead of paying an
// all-reduce + two copies on the critical path.  Every image takes the same decisions (SPMD), so the collective calls pair.
int icar_max_courant_prefetch_run(icar_hip_ctx *c, float dx, const float *dz_levels, bool allreduce)
{
    c->cfl_pre.valid = false;
    if (!c->h_cfl_pre) { HIPCHK(hipHostMalloc((void **)&c->h_cfl_pre, sizeof(float), hipHostMallocDefault)); HIPCHK(hipEventCreateWithFlags(&c->cfl_ev, hipEventDisableTiming)); }
    if (icar_max_courant_run(c, dx, dz_levels, nullptr, c->d_red + 8)) return 1;             // on the current stream, nothing waits
    if (allreduce && icar_comm_max_device(c, c->d_red + 8) != 0) return 1;
    HIPCHK(hipMemcpyAsync(c->h_cfl_pre, c->d_red + 8, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->cfl_ev, c->stream));
    c->cfl_pre.reduced = allreduce;
    c->cfl_pre.valid = true; c->cfl_pre.ver = c->wind_version; c->cfl_pre.dx = dx; c->cfl_pre.dzl.assign(dz_levels, dz_levels + c->d.nz);
    return 0;
}

// maxval(abs(u)), maxval(abs(v)), maxval(abs(w)) of the other cfl_strictness settings (time_step.f90:238-259, :293-305)
__global__ void __launch_bounds__(256)
k_max_abs3(size_t nu, size_t nv, size_t nw, const float *__restrict__ u, const float *__restrict__ v,
           const float *__restrict__ w, unsigned *__restrict__ out)
{
    const float *x = blockIdx.y == 0 ? u : blockIdx.y == 1 ? v : w;
    const size_t n = blockIdx.y == 0 ? nu : blockIdx.y == 1 ? nv : nw;
    float cur = 0.0f;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (size_t)gridDim.x * 256) cur = fmaxf(cur, fabsf(x[t]));
    for (int o = 32; o > 0; o >>= 1) cur = fmaxf(cur, __shfl_down(cur, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out + blockIdx.y, __float_as_uint(cur));
}

int icar_max_abs_winds_run(icar_hip_ctx *c, float *out3)
{
    const float *u = icar_field_f(c, ICAR_F_U), *v = icar_field_f(c, ICAR_F_V), *w = icar_field_f(c, ICAR_F_W);
    if (!u || !v || !w) return 1;
    HIPCHK(hipMemsetAsync(c->d_red, 0, 3 * sizeof(float), c->stream));
    ScopedTimer t(c, "cfl");
    hipLaunchKernelGGL(k_max_abs3, dim3(512, 3), dim3(256), 0, c->stream, icar_field_count(c, ICAR_F_U), icar_field_count(c, ICAR_F_V),
                       icar_field_count(c, ICAR_F_W), u, v, w, (unsigned *)c->d_red);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out3, c->d_red, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
