// icar_amd/csrc/sfc_basic.hip -- the surface-flux slot (row L1) on gfx950: lsm(domain, options, dt) as it runs for
// landsurface = kLSM_BASIC with watersurface 0, 1 or kWATER_SIMPLE, and the 10 m diagnostics of diagnostic_update it consumes.
//
// Reference algorithm: src/physics/lsm_driver.f90 -- lsm :1005-1554 (the gate :1016-1023, windspd :1028, water_simple's call
// :1056-1072, apply_fluxes' call :1550-1552), apply_fluxes :361-423, calc_exchange_coefficient :244-265 (of which only
// `where(wind==0) wind=1e-5`, :251, is visible on this path: its result CHS is read by Noah alone and is not built), lsm_init
// :522-611, :991-1000; src/physics/water_simple.f90 -- water_simple :83-136, sat_mr :18-55, calc_exchange_coefficient :58-72,
// ocean_roughness :74-81; src/main/time_step.f90:143-161 (u_10m, v_10m, ustar).
//
//   k_diag_10m      one thread per (i,j) of ims+1:ime-1, jms+1:jme-1: the log-law factors from roughness_z0 and the first level's
//                   height, u_10m = (u_mass currw) lastw with the product rounded in between (it passes through ustar), v_10m
//                   likewise, ustar = sqrt(u_mass**2 + v_mass**2) currw.  Launched only when roughness_z0 is on the device (the
//                   reference's `associated`).
//   k_water_simple  one thread per (i,j) of the same interior: windspd = sqrt(u_10m**2 + v_10m**2) with the zero replacement
//                   (windspd is a module array nobody else reads on this path, so it stays in a register and the halo ring's
//                   values are never formed), then water_simple where land_mask == kLC_WATER: QSFC, Z0 -> roughness_z0 (read by the
//                   next k_diag_10m: the loop carried from call to call), the bulk coefficients with the Ri < 0 / Ri >= 0 branch,
//                   sensible_heat, QFX, latent_heat, skin_temperature.  Land cells are not touched.
//   k_apply_fluxes  one thread per (i,j) of the memory rectangle, marching k over the WHOLE column: one read of qv per cell, the
//                   flux updates of theta and qv on its:ite, jts:jte and k <= kts + nz with the running sum of dz in the
//                   reference's form (a plain REAL(4) loop from kts: that is how this flang lowers sum(dz(i,kts:k-1,j)),
//                   tests/golden/make_golden_sfc.py), then the floor where(qv < 1e-10) on every level of every column, halo
//                   included; qv is stored only where its bits changed.
//   k_level_max     maxval(dz_interface(:,k,:)) of every level as a maximum of bit patterns (dz_interface is positive); the host
//                   finishes apply_fluxes' search for nz (:370-376) in REAL(4), once per context and again when dz_interface or
//                   the options are rewritten.
// Lanes along i (F1 of SURVEY.md), no LDS, no barrier.  REAL(4) throughout in the reference's operation order (no contraction:
// the compiled reference has none on this path; IEEE division and square root); exp / log are the C library's expf / logf bit
// for bit (glibc_flt32.h); 75*karman**2 is the product flang folds, 75 x fl(0.41 x 0.41) in REAL(4).
#include "ctx.h"
#include "glibc_flt32.h"
#include <cstdio>
#include <vector>

namespace {
constexpr float karman = 0.41f, gravity = 9.81f, LH_vaporization = 2260000.0f, cp = 1012.0f;   // icar_constants.f90:389-397
constexpr float SMALL_QV = 1e-10f;                                                              // lsm_driver.f90:87
constexpr float k75 = 75 * (karman * karman);                                                   // water_simple.f90:121
constexpr int kLC_WATER = 2;

typedef __amdgpu_buffer_rsrc_t rsrc_t;
// raw buffer accesses as in step.hip: descriptor + per-lane byte offset (the column) + wave-uniform byte offset (row and level)
__device__ __forceinline__ rsrc_t mk(const void *p) { return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, -1, 0x00020000); }
__device__ __forceinline__ float ld(rsrc_t r, int voff, int soff) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0)); }
__device__ __forceinline__ int ldi(rsrc_t r, int voff, int soff) { return __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0); }
__device__ __forceinline__ void st(float x, rsrc_t r, int voff, int soff) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, x), r, voff, soff, 0); }

// time_step.f90:143-161
__global__ void __launch_bounds__(64)
k_diag_10m(Dims d, const float *__restrict__ z, const float *__restrict__ terrain, const float *__restrict__ z0, const float *__restrict__ u_mass,
           const float *__restrict__ v_mass, float *__restrict__ u10, float *__restrict__ v10, float *__restrict__ ustar)
{
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y;
    if (i >= d.nx - 1) return;
    const int vi = 4 * i, s2 = 4 * d.nx * j, s3 = 4 * d.idx(0, 0, j);                // level kms
    const float zo = ld(mk(z0), vi, s2);
    const float currw = karman / gf_logf((ld(mk(z), vi, s3) - ld(mk(terrain), vi, s2)) / zo);       // :146
    const float lastw = gf_logf(10.0f / zo) / karman;                                                // :148
    const float um = ld(mk(u_mass), vi, s3), vm = ld(mk(v_mass), vi, s3);
    float t = um * currw;                                                                            // :152, rounded in domain%ustar
    st(t * lastw, mk(u10), vi, s2);                                                                  // :153
    t = vm * currw;
    st(t * lastw, mk(v10), vi, s2);                                                                  // :154-155
    st(sqrtf(um * um + vm * vm) * currw, mk(ustar), vi, s2);                                         // :160
}

__device__ __forceinline__ float sat_mr(float t, float p)                                           // water_simple.f90:18-55
{
    const bool ice = t < 273.15f;
    const float a = ice ? 21.8745584f : 17.2693882f, b = ice ? 7.66f : 35.86f;
    float e_s = 610.78f * gf_expf(a * (t - 273.16f) / (t - b));
    if ((p - e_s) <= 0) e_s = p * 0.99999f;
    return 0.6219907f * e_s / (p - e_s);
}

struct WaterArgs {
    Dims d;
    const float *u10, *v10, *sst, *psfc, *ustar, *qv, *temperature, *z, *terrain;
    const int *land_mask;
    float *sensible, *latent, *z0, *qsfc, *qfx, *tskin;
};

// lsm_driver.f90:1028, :251 and water_simple.f90:83-136 on 2..nx-1, 2..ny-1 of the memory rectangle
__global__ void __launch_bounds__(64)
k_water_simple(WaterArgs a)
{
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y;
    if (i >= a.d.nx - 1) return;
    const int vi = 4 * i, s2 = 4 * a.d.nx * j, s3 = 4 * a.d.idx(0, 0, j);
    if (ldi(mk(a.land_mask), vi, s2) != kLC_WATER) return;
    const float u = ld(mk(a.u10), vi, s2), v = ld(mk(a.v10), vi, s2);
    float wind = sqrtf(u * u + v * v);                                                               // :1028
    if (wind == 0) wind = 1e-5f;                                                                     // :251
    const float tsk = ld(mk(a.sst), vi, s2);
    const float qsfc = 0.98f * sat_mr(tsk, ld(mk(a.psfc), vi, s2));                                  // :116
    const float Z0 = 8e-6f / fmaxf(ld(mk(a.ustar), vi, s2), 1e-7f);                                  // :80
    const float zz = ld(mk(a.z), vi, s3) - ld(mk(a.terrain), vi, s2);                                // z_atm, lsm_driver.f90:992
    const float r = (zz + Z0) / Z0;
    float lnz = gf_logf(r);                                                                          // :120
    const float base = (k75 * sqrtf(r)) / (lnz * lnz);                                               // :121
    const float q = karman / lnz;
    lnz = q * q;                                                                                     // :122
    const float airt = ld(mk(a.temperature), vi, s3);
    const float Ri = gravity / airt * (airt - tsk) * zz / (wind * wind);                             // :65
    float C;
    if (Ri < 0) C = lnz * (1.0f - (15.0f * Ri) / (1.0f + (base * sqrtf((-1.0f) * Ri))));             // :68
    else        C = lnz * 1.0f / ((1.0f + 15.0f * Ri) * sqrtf(1.0f + 5.0f * Ri));                    // :70
    const float qfx = C * wind * (qsfc - ld(mk(a.qv), vi, s3));                                      // :128
    st(qsfc, mk(a.qsfc), vi, s2);
    st(Z0, mk(a.z0), vi, s2);
    st(C * wind * (tsk - airt), mk(a.sensible), vi, s2);                                             // :127
    st(qfx, mk(a.qfx), vi, s2);
    st(qfx * LH_vaporization, mk(a.latent), vi, s2);                                                 // :129
    st(tsk, mk(a.tskin), vi, s2);                                                                    // :130
}

struct FluxArgs {
    Dims d;
    int i0, i1, j0, j1, k0, klast;      // 0-based, inclusive; klast = k0 + nz of apply_fluxes
    float dt, sh, lh, thick;
};

__device__ __forceinline__ void floor_store(float q_old, float q, rsrc_t rq, int vi, int sc)
{
    if (q < SMALL_QV) q = SMALL_QV;                                                                  // :419
    if (__builtin_bit_cast(int, q) != __builtin_bit_cast(int, q_old)) st(q, rq, vi, sc);
}

// apply_fluxes :378-421
__global__ void __launch_bounds__(64)
k_apply_fluxes(FluxArgs a, float *__restrict__ th, float *__restrict__ qv, const float *__restrict__ density, const float *__restrict__ pii,
               const float *__restrict__ dz, const float *__restrict__ sensible, const float *__restrict__ latent)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= a.d.nx) return;
    const int vi = 4 * i, sk = 4 * a.d.sk;
    const rsrc_t rq = mk(qv);
    int k = 0, sc = 4 * a.d.idx(0, 0, j);
    if (i >= a.i0 && i <= a.i1 && j >= a.j0 && j <= a.j1) {
        const rsrc_t rt = mk(th), rr = mk(density), rp = mk(pii), rz = mk(dz);
        const int s2 = 4 * a.d.nx * j;
        const float sens = ld(mk(sensible), vi, s2), lat = ld(mk(latent), vi, s2);
        for (; k < a.k0; ++k, sc += sk) { const float q = ld(rq, vi, sc); floor_store(q, q, rq, vi, sc); }   // (levels below kts: the floor alone)
        float below = 0.0f, dz_prev = 0.0f;                          // sum(dz(i,kts:k-1,j)), a plain loop in the reference
#pragma unroll 1
        for (; k <= a.klast; ++k, sc += sk) {
            const float q = ld(rq, vi, sc), t = ld(rt, vi, sc), rho = ld(rr, vi, sc), p = ld(rp, vi, sc), dzk = ld(rz, vi, sc);
            float lf;
            if (k == a.k0) lf = fminf(1.0f, a.thick / dzk);                                          // :393
            else {
                below = below + dz_prev;
                lf = (a.thick - below) / dzk;                                                        // :395
                lf = lf < 1.0f ? lf : 1.0f;
                lf = lf > 0.0f ? lf : 0.0f;
            }
            dz_prev = dzk;
            const float dTemp = (a.sh * sens * a.dt / cp) / (rho * a.thick);                         // :400
            st(t + (dTemp / p) * lf, rt, vi, sc);                                                    // :403
            const float lhdQV = (a.lh * lat / LH_vaporization * a.dt) / (rho * a.thick);             // :407
            floor_store(q, q + lhdQV * lf, rq, vi, sc);                                              // :410, :419
        }
    }
    // the rest of the column (all of it outside the tile): four levels' loads in flight
    for (; k + 3 < a.d.nz; k += 4, sc += 4 * sk) {
        float q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = ld(rq, vi, sc + u * sk);
#pragma unroll
        for (int u = 0; u < 4; ++u) floor_store(q[u], q[u], rq, vi, sc + u * sk);
    }
    for (; k < a.d.nz; ++k, sc += sk) { const float q = ld(rq, vi, sc); floor_store(q, q, rq, vi, sc); }
}

// maxval(dz_interface(:,k,:)) of every level: bit patterns of positive floats order like unsigned integers (cfl.hip)
__global__ void __launch_bounds__(256)
k_level_max(Dims d, const float *__restrict__ dz, unsigned *__restrict__ out)
{
    const int k = blockIdx.y, n2 = d.nx * d.ny;
    float cur = 0.0f;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n2; t += gridDim.x * 256) cur = fmaxf(cur, dz[d.idx(t % d.nx, k, t / d.nx)]);
    for (int o = 32; o > 0; o >>= 1) cur = fmaxf(cur, __shfl_down(cur, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out + k, __float_as_uint(cur));
}

__global__ void k_sfc_fill(float *p, int n, float v) { const int t = blockIdx.x * blockDim.x + threadIdx.x; if (t < n) p[t] = v; }
__global__ void k_sfc_first_level(Dims d, const float *__restrict__ q, float *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < d.nx * d.ny) out[t] = q[d.idx(t % d.nx, 0, t / d.nx)];
}

float *need(icar_hip_ctx *c, int f, const char *who, const char *member)
{
    if (c->field[f]) return (float *)c->field[f];
    char b[200]; snprintf(b, sizeof b, "%s: domain%%%s (field %d) is not on the device", who, member, f);
    icar_set_error(b);
    return nullptr;
}

bool too_large(icar_hip_ctx *c, const char *who)
{
    if (c->n3 * sizeof(float) < ((size_t)1 << 31)) return false;
    icar_set_error(std::string(who) + ": a field of 2 GiB or more is not supported (32-bit offsets)");
    return true;
}

// a 2-D result the library owns: created on first use with the reference's initial value
float *own2d(icar_hip_ctx *c, int f, float init)
{
    const bool fresh = !c->field[f];
    float *p = icar_field_f(c, f, false);                             // zero-filled
    if (p && fresh && init != 0.0f) {
        const int n2 = c->d.nx * c->d.ny;
        hipLaunchKernelGGL(k_sfc_fill, dim3((n2 + 255) / 256), dim3(256), 0, c->stream, p, n2, init);
    }
    return p;
}
}  // namespace

// the 10 m winds and ustar of diagnostic_update (time_step.f90:143-161); needs roughness_z0 (the caller tests for it)
int icar_sfc_diag_10m_run(icar_hip_ctx *c)
{
    const float *z0 = need(c, ICAR_F_ROUGHNESS_Z0, "diag_10m", "roughness_z0"), *z = need(c, ICAR_F_Z, "diag_10m", "z");
    const float *ter = need(c, ICAR_F_TERRAIN, "diag_10m", "terrain"), *um = need(c, ICAR_F_U_MASS, "diag_10m", "u_mass"), *vm = need(c, ICAR_F_V_MASS, "diag_10m", "v_mass");
    if (!z0 || !z || !ter || !um || !vm || too_large(c, "diag_10m")) return 1;
    // outside ims+1:ime-1, jms+1:jme-1 u_10m / v_10m keep their initial 0 and ustar its initial 0.1 (domain_obj.f90:419, :1950-51)
    float *u10 = own2d(c, ICAR_F_U_10M, 0.0f), *v10 = own2d(c, ICAR_F_V_10M, 0.0f), *us = own2d(c, ICAR_F_USTAR, 0.1f);
    if (!u10 || !v10 || !us) return 1;
    if (c->d.ny - 2 > 65535) { icar_set_error("diag_10m: more than 65535 rows are not supported"); return 1; }
    ScopedTimer timer(c, "diag_10m");
    hipLaunchKernelGGL(k_diag_10m, dim3((c->d.nx - 2 + 63) / 64, c->d.ny - 2), dim3(64), 0, c->stream, c->d, z, ter, z0, um, vm, u10, v10, us);
    HIPCHK(hipGetLastError());
    return 0;
}

// QSFC = domain%water_vapor%data_3d(:,kms,:) of lsm_init (:568), once
static int qsfc_init(icar_hip_ctx *c)
{
    if (c->field[ICAR_F_QSFC]) return 0;
    const float *qv = need(c, ICAR_F_WATER_VAPOR, "lsm_init", "water_vapor");
    float *qs = qv ? icar_field_f(c, ICAR_F_QSFC, false) : nullptr;
    if (!qs) return 1;
    const int n2 = c->d.nx * c->d.ny;
    hipLaunchKernelGGL(k_sfc_first_level, dim3((n2 + 255) / 256), dim3(256), 0, c->stream, c->d, qv, qs);
    HIPCHK(hipGetLastError());
    return 0;
}

// the gated block of lsm with watersurface = kWATER_SIMPLE (lsm_driver.f90:1028-1073)
int icar_sfc_water_simple_run(icar_hip_ctx *c)
{
    static const char *who = "water_simple";
    WaterArgs a;
    a.d = c->d;
    a.land_mask = (const int *)c->field[ICAR_F_LAND_MASK];
    if (!a.land_mask) { icar_set_error("water_simple: domain%land_mask (field 46) is not on the device"); return 1; }
    a.u10 = need(c, ICAR_F_U_10M, who, "u_10m"); a.v10 = need(c, ICAR_F_V_10M, who, "v_10m"); a.ustar = need(c, ICAR_F_USTAR, who, "ustar");
    a.sst = need(c, ICAR_F_SST, who, "sst"); a.psfc = need(c, ICAR_F_SURFACE_PRESSURE, who, "surface_pressure");
    a.qv = need(c, ICAR_F_WATER_VAPOR, who, "water_vapor"); a.temperature = need(c, ICAR_F_TEMPERATURE, who, "temperature");
    a.z = need(c, ICAR_F_Z, who, "z"); a.terrain = need(c, ICAR_F_TERRAIN, who, "terrain");
    a.z0 = need(c, ICAR_F_ROUGHNESS_Z0, who, "roughness_z0");
    if (!a.u10 || !a.v10 || !a.ustar || !a.sst || !a.psfc || !a.qv || !a.temperature || !a.z || !a.terrain || !a.z0 || too_large(c, who)) return 1;
    if (qsfc_init(c)) return 1;
    a.qsfc = (float *)c->field[ICAR_F_QSFC];
    a.sensible = own2d(c, ICAR_F_SENSIBLE_HEAT, 0.0f); a.latent = own2d(c, ICAR_F_LATENT_HEAT, 0.0f);
    a.qfx = own2d(c, ICAR_F_QFX, 0.0f); a.tskin = own2d(c, ICAR_F_SKIN_TEMPERATURE, 0.0f);
    if (!a.sensible || !a.latent || !a.qfx || !a.tskin) return 1;
    if (c->d.ny - 2 > 65535) { icar_set_error("water_simple: more than 65535 rows are not supported"); return 1; }
    ScopedTimer timer(c, "lsm_water");
    hipLaunchKernelGGL(k_water_simple, dim3((c->d.nx - 2 + 63) / 64, c->d.ny - 2), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// nz of apply_fluxes (:370-376) for kts..kte: the last level, absolute and 1-based in the context's index space, at which the running
// sum of maxval(dz_interface(:,k,:)) is still below sfc_layer_thickness (0: none).  Kept until dz_interface or the options change.
int icar_sfc_layers(icar_hip_ctx *c, int kts, int kte, int *nz_out)
{
    if (kts < c->kms || kte > c->kme || kte < kts) { icar_set_error("apply_fluxes: kts..kte outside the levels of the context"); return 1; }
    const float thick = c->step.sfc_layer_thickness;
    if (c->sfc_nz_valid && c->sfc_nz_kts == kts && c->sfc_nz_kte == kte && c->sfc_nz_thick == thick) { *nz_out = c->sfc_nz; return 0; }
    const float *dz = need(c, ICAR_F_DZ_INTERFACE, "apply_fluxes", "dz_interface");
    if (!dz) return 1;
    const int nz = c->d.nz;
    if (nz > 65535) { icar_set_error("apply_fluxes: more than 65535 levels are not supported"); return 1; }
    if (!c->sfc_levelmax) HIPCHK(hipMalloc(&c->sfc_levelmax, nz * sizeof(unsigned)));
    unsigned *d_max = c->sfc_levelmax;
    HIPCHK(hipMemsetAsync(d_max, 0, nz * sizeof(unsigned), c->stream));
    const int n2 = c->d.nx * c->d.ny;
    int nb = (n2 + 255) / 256; if (nb > 64) nb = 64;
    hipLaunchKernelGGL(k_level_max, dim3(nb, nz), dim3(256), 0, c->stream, c->d, dz, d_max);
    HIPCHK(hipGetLastError());
    std::vector<float> m(nz);
    HIPCHK(hipMemcpyAsync(m.data(), d_max, nz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int found = 0;
    float layer = 0.0f;
    for (int k = kts; k <= kte; ++k) {
        layer = m[k - c->kms] + layer;                                // :373
        if (layer < thick) found = k;                                 // :374
    }
    c->sfc_nz = found; c->sfc_nz_kts = kts; c->sfc_nz_kte = kte; c->sfc_nz_thick = thick; c->sfc_nz_valid = true;
    *nz_out = found;
    return 0;
}

// apply_fluxes(domain, dt) (:361-423) on the tile its..jte, levels kts .. kts+nz
int icar_sfc_apply_fluxes_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte)
{
    static const char *who = "apply_fluxes";
    if (its < c->ims || ite > c->ime || jts < c->jms || jte > c->jme || kts < c->kms || kte > c->kme) { icar_set_error("apply_fluxes: tile outside memory bounds"); return 1; }
    int nz;
    if (icar_sfc_layers(c, kts, kte, &nz)) return 1;
    if (kts + nz > kte) {
        char b[256];
        snprintf(b, sizeof b, "apply_fluxes: the surface layer reaches kte: its loop runs k = kts .. kts+nz = %d .. %d, one level more than the nz = %d "
                 "levels below sfc_layer_thickness, past kte = %d (the reference reads out of bounds there, lsm_driver.f90:389)", kts, kts + nz, nz, kte);
        icar_set_error(b);
        return 1;
    }
    float *th = need(c, ICAR_F_POTENTIAL_TEMPERATURE, who, "potential_temperature"), *qv = need(c, ICAR_F_WATER_VAPOR, who, "water_vapor");
    const float *rho = need(c, ICAR_F_DENSITY, who, "density"), *pii = need(c, ICAR_F_EXNER, who, "exner"), *dz = need(c, ICAR_F_DZ_INTERFACE, who, "dz_interface");
    const float *sh = need(c, ICAR_F_SENSIBLE_HEAT, who, "sensible_heat"), *lh = need(c, ICAR_F_LATENT_HEAT, who, "latent_heat");
    if (!th || !qv || !rho || !pii || !dz || !sh || !lh || too_large(c, who)) return 1;
    if (c->d.ny > 65535) { icar_set_error("apply_fluxes: more than 65535 rows are not supported"); return 1; }
    FluxArgs a;
    a.d = c->d; a.i0 = its - c->ims; a.i1 = ite - c->ims; a.j0 = jts - c->jms; a.j1 = jte - c->jms; a.k0 = kts - c->kms; a.klast = a.k0 + nz;
    a.dt = dt; a.sh = c->step.sh_feedback_fraction; a.lh = c->step.lh_feedback_fraction; a.thick = c->step.sfc_layer_thickness;
    ScopedTimer timer(c, "lsm_fluxes");
    hipLaunchKernelGGL(k_apply_fluxes, dim3((c->d.nx + 63) / 64, c->d.ny), dim3(64), 0, c->stream, a, th, qv, rho, pii, dz, sh, lh);
    HIPCHK(hipGetLastError());
    return 0;
}

// lsm(domain, options, dt) (:1005-1554) on the tile of icar_hip_step_configure
int icar_lsm_run(icar_hip_ctx *c, float dt)
{
    IcarStepState &s = c->step;
    if (s.landsurface == 0) return 0;                                 // :1014, whatever watersurface is
    const bool noah = s.landsurface == ICAR_LSM_NOAH;
    if (noah && !icar_lsm_noah_coupled(c)) {                          // (coupled: icar_hip_lsm_noah_couple, lsm_noah_driver.hip)
        icar_set_error("lsm: the Noah branch of lsm() (lsm_driver.f90:1177-1291: CHS, QGH, current_precipitation, the statements after the call, "
                       "soil_totalmoisture, surface_diagnostics) is not built: Noah runs through icar_hip_lsm_noah only");
        return 1;
    }
    const double now = s.model_time, upd = (double)s.lsm_update_interval;
    if (s.lsm_last_model_time == -999.0) s.lsm_last_model_time = now - upd;                          // :1016-1018
    if ((now - s.lsm_last_model_time) >= upd) {                                                      // :1021
        const float lsm_dt = (float)(now - s.lsm_last_model_time);                                   // :1022
        if (noah && !(lsm_dt > 0)) { icar_set_error("lsm: lsm_dt = 0 (update_interval = 0 at the first call): lsm_noah divides by it (PRCP = RAINBL / DT, lsm_noahdrv.f90:692)"); return 1; }
        s.lsm_last_model_time = now;                                                                 // :1023
        if (noah) { if (icar_lsm_noah_gated_run(c, lsm_dt)) return 1; }                              // :1028-1546, water_simple inside
        else if (s.watersurface == ICAR_WATER_SIMPLE && icar_sfc_water_simple_run(c)) return 1;           // :1051-1073
    }
    const icar_hip_step_config &g = s.cfg;
    return icar_sfc_apply_fluxes_run(c, dt, g.its, g.ite, g.jts, g.jte, g.kts, g.kte);               // :1550-1552
}

// lsm_init's part on the device: QSFC (:568) when water_vapor is already there
int icar_lsm_init_device(icar_hip_ctx *c)
{
    if (c->step.landsurface == 0 || !c->field[ICAR_F_WATER_VAPOR]) return 0;
    return qsfc_init(c);
}
