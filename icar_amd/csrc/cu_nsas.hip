// icar_amd/csrc/cu_nsas.hip -- the NSAS convection scheme on gfx950: the call of cu_nsas (src/physics/cu_driver.f90:354-417,
// src/physics/cu_nsas.f90) that convect makes for convection = kCU_NSAS.  The column code is nsas_column.h, which also says what is
// not built (tend%u / tend%v) and why a column may leave as soon as its own cnvflg falls.
//
//   k_nsas_limits   one wave per row: kbmax, kbm, kmax of nsas2d (:619-632), the maxima over the row's columns its..ite
//   k_nsas_deep     ONE THREAD PER COLUMN of its..ite, lanes along i: cu_nsas's row arrays (:169-209) and nsas2d into the workspace
//   k_nsas_shallow  nscv2d on the same t1, q1, qc2, qi2, kbot, ktop, icps
//   k_nsas_finish   the two rains, HBOT / HTOP and the four tendencies (:255-303)
// The level arrays live in a device workspace laid out [array][level][column] (every access of a wave is one coalesced line, nothing
// of a column sits in scratch); the five scalars a column carries from launch to launch (the two rains, kbot, ktop, icps) in a second,
// small one.  The tile is walked in chunks of rows that fit the workspace.  A column that stops convecting returns inside its kernel; the
// shallow scheme starts only where icps = 0 and sflx > 0.  REAL(4) throughout in the reference's operation order: no contraction,
// IEEE division and square root; expf and powf are glibc's, restated in glibc_flt32.h.
//
// hpbl: init_convection fills domain%hpbl with 1000 unless the boundary layer is YSU (cu_driver.f90:180-186); with YSU initialised the
// scheme reads the hpbl YSU wrote (ICAR_YSU_HPBL), otherwise its own array (ICAR_NSAS_HPBL).
//
// Levels: kts = 1 (the scheme names level 1 literally: prsi(i,1), zi(i,2), eta(i,1)); kte - kts >= NSAS_MIN_LEVELS scheme levels
// (with one, cu_nsas.f90:2456 reads xlamue(i,0)) and at most NSAS_MAX_LEVELS; all refused before any launch.
#include "cu_state.h"
#include "glibc_flt32.h"
#include <cmath>
#include <cstdio>

#define NSAS_FN __device__ static __forceinline__
#define NSAS_EXPF gf_expf
#define NSAS_POWF gf_powf
#define NSAS_SQRTF sqrtf
#include "nsas_column.h"

namespace {
constexpr size_t kWsColumns = (size_t)1 << 15;       // columns per launch (a tile row always fits)
enum { NSAS_NCOL = 5 };                              // rain of nsas2d, kbot, ktop, icps, rain of nscv2d

struct NsasArgs {
    Dims d;
    int i0, nxt, j0, k0, n, dxf;
    float dt, dx;
    size_t stride, nl;
    const float *t, *qv, *qc, *qi, *pi, *rho, *w, *dz, *p, *pint, *u, *v, *hpbl, *hfx, *lh;
    const int *land_mask, *limits;
    float *tend_th, *tend_qv, *tend_qc, *tend_qi, *raincv, *pratec, *hbot, *htop, *ws, *col;
};

__device__ __forceinline__ NsasIn column_of(const NsasArgs &a, int i, int j)
{
    const size_t at = (size_t)a.d.idx(i, a.k0, j);
    return {a.t + at, a.qv + at, a.qc + at, a.qi + at, a.pi + at, a.rho + at, a.w + at, a.dz + at, a.p + at, a.pint + at, a.u + at, a.v + at,
            (size_t)a.d.sk};
}

__device__ __forceinline__ float xland_of(const NsasArgs &a, int i, int j)
{
    const int lm = a.land_mask ? a.land_mask[(size_t)a.d.nx * j + i] : 1;
    return (lm == 0 || lm == 2) ? 2.0f : (float)lm;                               // cu_driver.f90:139-140
}

// limits[3 j .. 3 j + 2] = the row's kbmax, kbm, kmax; block = one wave, grid = rows
__global__ void __launch_bounds__(64)
k_nsas_limits(NsasArgs a, int j0, int *__restrict__ limits)
{
    const int j = j0 + blockIdx.x;
    int kbmax = 0, kbm = 0, kmax = 0;
    for (int ii = threadIdx.x; ii < a.nxt; ii += 64) {
        int x, y, z;
        nsas_row_limits(column_of(a, a.i0 + ii, j), a.n, &x, &y, &z);
        kbmax = max(kbmax, x); kbm = max(kbm, y); kmax = max(kmax, z);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        kbmax = max(kbmax, __shfl_xor(kbmax, m, 64)); kbm = max(kbm, __shfl_xor(kbm, m, 64)); kmax = max(kmax, __shfl_xor(kmax, m, 64));
    }
    if (threadIdx.x == 0) { limits[3 * j] = min(kbmax, a.n); limits[3 * j + 1] = min(kbm, a.n); limits[3 * j + 2] = min(kmax, a.n); }
}

__global__ void __launch_bounds__(64)
k_nsas_deep(NsasArgs a)
{
    const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y;
    if (ii >= a.nxt) return;
    const size_t col = (size_t)jj * a.nxt + ii;
    const int i = a.i0 + ii, j = a.j0 + jj;
    NsasIn in = column_of(a, i, j);
    const int *lim = a.limits + 3 * j;
    NsasOut o;
    o.rain2 = 0.f;
    // the workspace's extents and the level stride are pinned to vector registers: as wave-uniform values they (and the 36 array
    // offsets made from them) would sit in scalar registers, which the scheme's nested divergent control flow needs for its exec masks
    size_t stride = a.stride, nl = a.nl, ls = in.ls;
    float *cs = a.col + col, *ws = a.ws + col;
    asm volatile("" : "+v"(stride), "+v"(nl), "+v"(ls), "+v"(cs), "+v"(ws));
    in.ls = ls;
    nsas_setup(in, a.n, ws, stride, nl);
    nsas_deep(in, a.n, lim[0], lim[1], lim[2], xland_of(a, i, j), a.dt, a.dx, a.dxf, ws, stride, nl, &o, nullptr);
    cs[0] = o.rain1; ((int *)cs)[stride] = o.kbot; ((int *)cs)[2 * stride] = o.ktop; ((int *)cs)[3 * stride] = o.icps;
}

__global__ void __launch_bounds__(64)
k_nsas_shallow(NsasArgs a)
{
    const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y;
    if (ii >= a.nxt) return;
    const size_t col = (size_t)jj * a.nxt + ii;
    const int i = a.i0 + ii, j = a.j0 + jj;
    NsasIn in = column_of(a, i, j);
    const size_t c2 = (size_t)a.d.nx * j + i;
    size_t stride = a.stride, nl = a.nl, ls = in.ls;                              // in vector registers: see k_nsas_deep
    const float *cs = a.col + col;
    float *ws = a.ws + col;
    asm volatile("" : "+v"(stride), "+v"(nl), "+v"(ls), "+v"(cs), "+v"(ws));
    in.ls = ls;
    NsasOut o;
    o.rain1 = cs[0]; o.kbot = ((const int *)cs)[stride]; o.ktop = ((const int *)cs)[2 * stride]; o.icps = ((const int *)cs)[3 * stride];
    const float qfx = a.lh[c2] / 2260000.0f;                                      // latent_heat / LH_vaporization, cu_driver.f90:394
    nsas_shallow(in, a.n, xland_of(a, i, j), a.hpbl[c2], a.hfx[c2], qfx, a.dt, ws, stride, nl, &o, nullptr);
    float *co = a.col + col;
    ((int *)co)[stride] = o.kbot; ((int *)co)[2 * stride] = o.ktop; co[4 * stride] = o.rain2;
}

__global__ void __launch_bounds__(64)
k_nsas_finish(NsasArgs a)
{
    const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y;
    if (ii >= a.nxt) return;
    const size_t col = (size_t)jj * a.nxt + ii;
    const int i = a.i0 + ii, j = a.j0 + jj;
    const NsasIn in = column_of(a, i, j);
    const size_t at = (size_t)a.d.idx(i, a.k0, j), c2 = (size_t)a.d.nx * j + i;
    const float *cs = a.col + col;
    NsasOut o;
    o.rain1 = cs[0]; o.kbot = ((const int *)cs)[a.stride]; o.ktop = ((const int *)cs)[2 * a.stride]; o.icps = 0; o.rain2 = cs[4 * a.stride];
    nsas_finish(in, a.n, a.dt, a.ws + col, a.stride, a.nl, &o, a.tend_th + at, a.tend_qv + at, a.tend_qc + at, a.tend_qi + at, a.raincv + c2,
                a.pratec + c2, a.hbot + c2, a.htop + c2);
}

__global__ void k_nsas_fill(float *p, size_t n, float v) { const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; if (t < n) p[t] = v; }

bool is3d(int which) { return which == ICAR_NSAS_TEND_QC || which == ICAR_NSAS_TEND_QI; }
size_t count(const icar_hip_ctx *c, int which) { return is3d(which) ? c->n3 : (size_t)c->d.nx * c->d.ny; }

const float *need(icar_hip_ctx *c, int f, const char *member)
{
    if (c->field[f]) return (const float *)c->field[f];
    char b[200]; snprintf(b, sizeof b, "cu_nsas: domain%%%s (field %d) is not on the device", member, f);
    icar_set_error(b);
    return nullptr;
}
}  // namespace

void icar_nsas_free(CuState *s)
{
    for (float *&p : s->nsas) { if (p) hipFree(p); p = nullptr; }
    if (s->nsas_ws) hipFree(s->nsas_ws);
    if (s->nsas_col) hipFree(s->nsas_col);
    if (s->nsas_limits) hipFree(s->nsas_limits);
    s->nsas_ws = s->nsas_col = nullptr; s->nsas_limits = nullptr;
}

// kts..kte of the call: the levels the scheme can run on (see the header)
int icar_nsas_levels_ok(icar_hip_ctx *c, int kts, int kte)
{
    char b[400];
    const CuState *s = c->cu;
    if (!s || !s->nsas_ws) { icar_set_error("cu_nsas: the scheme is not initialised (icar_hip_convection_init with convection = 4)"); return 1; }
    if (kts < c->kms || kte > c->kme) { icar_set_error("cu_nsas: kts..kte outside the levels of the context"); return 1; }
    if (kts != 1) {
        snprintf(b, sizeof b, "cu_nsas: kts = %d: nsas2d and nscv2d name level 1 literally (prsi(i,1), zi(i,2), eta(i,1), heo(i,1), "
                 "cu_nsas.f90:624-626, :699, :908-914, :2431); only kts = 1 is built", kts);
        icar_set_error(b); return 1;
    }
    const int n = kte - kts;
    if (n < NSAS_MIN_LEVELS) {
        snprintf(b, sizeof b, "cu_nsas: %d levels (kts..kte): at least %d.  The scheme runs on kts..kte-1; with one scheme level km1 = 0 and the "
                 "reference reads xlamue(i,km1) = xlamue(i,0) below the array (cu_nsas.f90:2456)", kte - kts + 1, NSAS_MIN_LEVELS + 1);
        icar_set_error(b); return 1;
    }
    if (n > NSAS_MAX_LEVELS || n + 2 > s->nsas_levels) {
        snprintf(b, sizeof b, "cu_nsas: %d levels (kts..kte): at most %d (the column workspace is sized for kte - kts <= %d)", kte - kts + 1,
                 NSAS_MAX_LEVELS + 1, NSAS_MAX_LEVELS);
        icar_set_error(b); return 1;
    }
    return 0;
}

// init_convection for kCU_NSAS (cu_driver.f90:173-202): tend%qc, tend%qi (nsasinit's zeroing), PRATEC, HBOT, HTOP, hpbl and the workspace
int icar_nsas_init_device(icar_hip_ctx *c, float dx)
{
    if (icar_cu_common_init(c)) return 1;
    CuState *s = c->cu;
    const int nz = c->d.nz;
    const size_t n2 = (size_t)c->d.nx * c->d.ny;
    if (!s->nsas_ws) {
        for (int w = 0; w < ICAR_NSAS_N; ++w) HIPCHK(hipMalloc(&s->nsas[w], count(c, w) * sizeof(float)));
        HIPCHK(hipMalloc(&s->nsas_limits, sizeof(int) * 3 * c->d.ny));
        s->nsas_cols = n2 < kWsColumns ? n2 : kWsColumns;
        if (s->nsas_cols < (size_t)c->d.nx) s->nsas_cols = c->d.nx;
        const int n = nz - 1 < NSAS_MAX_LEVELS ? nz - 1 : NSAS_MAX_LEVELS;
        s->nsas_levels = (n < 1 ? 1 : n) + 2;
        HIPCHK(hipMalloc(&s->nsas_col, sizeof(float) * NSAS_NCOL * s->nsas_cols));
        HIPCHK(hipMalloc(&s->nsas_ws, sizeof(float) * NSAS_NARR * (size_t)s->nsas_levels * s->nsas_cols));
        HIPCHK(hipMemsetAsync(s->nsas[ICAR_NSAS_HPBL], 0, n2 * sizeof(float), c->stream));
    }
    for (int w = 0; w < ICAR_NSAS_N; ++w)
        if (w != ICAR_NSAS_HPBL) HIPCHK(hipMemsetAsync(s->nsas[w], 0, count(c, w) * sizeof(float), c->stream));
    HIPCHK(hipMemsetAsync(s->nsas_limits, 0, sizeof(int) * 3 * c->d.ny, c->stream));
    if (c->step.boundarylayer != ICAR_PBL_YSU) {                                  // cu_driver.f90:180-186
        hipLaunchKernelGGL(k_nsas_fill, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, c->stream, s->nsas[ICAR_NSAS_HPBL], n2, 1000.0f);
        HIPCHK(hipGetLastError());
    }
    s->nsas_dx = dx;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// cu_nsas on its..ite, jts..jte, kts..kte-1 (cu_driver.f90:354-417)
int icar_nsas_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte)
{
    if (icar_nsas_levels_ok(c, kts, kte)) return 1;
    CuState *s = c->cu;
    if (its < c->ims || ite > c->ime || jts < c->jms || jte > c->jme) { icar_set_error("cu_nsas: tile outside memory bounds"); return 1; }
    if (jte - jts + 1 > 65535) { icar_set_error("cu_nsas: more than 65535 rows are not supported"); return 1; }
    if (ite < its || jte < jts) return 0;
    NsasArgs a;
    a.t = need(c, ICAR_F_TEMPERATURE, "temperature"); a.qv = need(c, ICAR_F_WATER_VAPOR, "water_vapor");
    a.qc = need(c, ICAR_F_CLOUD_WATER, "cloud_water_mass"); a.qi = need(c, ICAR_F_CLOUD_ICE, "cloud_ice_mass");
    a.pi = need(c, ICAR_F_EXNER, "exner"); a.rho = need(c, ICAR_F_DENSITY, "density"); a.w = need(c, ICAR_F_W_REAL, "w_real");
    a.dz = need(c, ICAR_F_DZ_INTERFACE, "dz_interface"); a.p = need(c, ICAR_F_PRESSURE, "pressure");
    a.pint = need(c, ICAR_F_PRESSURE_INTERFACE, "pressure_interface");
    a.u = need(c, ICAR_F_U_MASS, "u_mass"); a.v = need(c, ICAR_F_V_MASS, "v_mass");
    a.hfx = need(c, ICAR_F_SENSIBLE_HEAT, "sensible_heat"); a.lh = need(c, ICAR_F_LATENT_HEAT, "latent_heat");
    if (!a.t || !a.qv || !a.qc || !a.qi || !a.pi || !a.rho || !a.w || !a.dz || !a.p || !a.pint || !a.u || !a.v || !a.hfx || !a.lh) return 1;
    a.land_mask = (const int *)c->field[ICAR_F_LAND_MASK];            // never uploaded = all land
    const float *ysu_hpbl = icar_ysu_hpbl(c);
    a.hpbl = ysu_hpbl ? ysu_hpbl : s->nsas[ICAR_NSAS_HPBL];
    a.limits = s->nsas_limits;
    a.d = c->d; a.i0 = its - c->ims; a.nxt = ite - its + 1; a.k0 = kts - c->kms; a.n = kte - kts; a.dt = dt;
    a.dx = s->nsas_dx; a.dxf = s->nsas_dx <= 1000.0f ? 1 : 2;         // cu_driver.f90:357-361
    a.tend_th = s->arr[ICAR_CU_TEND_TH]; a.tend_qv = s->arr[ICAR_CU_TEND_QV]; a.raincv = s->arr[ICAR_CU_RAINCV];
    a.tend_qc = s->nsas[ICAR_NSAS_TEND_QC]; a.tend_qi = s->nsas[ICAR_NSAS_TEND_QI]; a.pratec = s->nsas[ICAR_NSAS_PRATEC];
    a.hbot = s->nsas[ICAR_NSAS_HBOT]; a.htop = s->nsas[ICAR_NSAS_HTOP];
    a.ws = s->nsas_ws; a.col = s->nsas_col;
    const int rows_per = (int)(s->nsas_cols / (size_t)a.nxt);         // >= 1: nsas_cols >= nx
    // [array][level][column] with the column count of one launch: (array nl + level) stride + column < NSAS_NARR nsas_levels nsas_cols
    a.stride = (size_t)rows_per * a.nxt;
    a.nl = (size_t)s->nsas_levels;
    ScopedTimer timer(c, "cu_nsas");
    a.j0 = 0;
    hipLaunchKernelGGL(k_nsas_limits, dim3(jte - jts + 1), dim3(64), 0, c->stream, a, jts - c->jms, s->nsas_limits);
    for (int j = jts; j <= jte; j += rows_per) {
        const int rows = jte - j + 1 < rows_per ? jte - j + 1 : rows_per;
        const dim3 grid((a.nxt + 63) / 64, rows), block(64);
        a.j0 = j - c->jms;
        hipLaunchKernelGGL(k_nsas_deep, grid, block, 0, c->stream, a);
        hipLaunchKernelGGL(k_nsas_shallow, grid, block, 0, c->stream, a);
        hipLaunchKernelGGL(k_nsas_finish, grid, block, 0, c->stream, a);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int icar_nsas_copy(icar_hip_ctx *c, int which, void *host, bool to_device)
{
    CuState *s = c->cu;
    if (!s || !s->nsas_ws) { icar_set_error("nsas_upload / _download: the scheme is not initialised (icar_hip_convection_init with convection = 4)"); return 1; }
    if (which < 0 || which >= ICAR_NSAS_N) { icar_set_error("nsas_upload / _download: `which` is one of ICAR_NSAS_*"); return 1; }
    const size_t bytes = count(c, which) * sizeof(float);
    if (to_device) HIPCHK(hipMemcpyAsync(s->nsas[which], host, bytes, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(hipMemcpyAsync(host, s->nsas[which], bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
