// icar_amd/csrc/pbl_simple.hip -- the simple boundary-layer scheme (HP96, row P1) on gfx950.
//
// Reference algorithm: src/physics/pbl_simple.f90 -- simple_pbl :69-141, diffuse_variable :143-163, pbl_diffusion :165-211,
// calc_shear :213-224, calc_virt_pot_temp_zgradient :227-248, calc_pbl_stability_function :251-274,
// calc_richardson_gradient :278-291; called by pbl(domain, options, dt) (src/physics/pbl_driver.f90:197-221).
//
// The scheme is two passes separated by a reduction: the sub-step count of the explicit diffusion is
//     nsubsteps = ceiling(2 * maxval(Kq / dz))  over its:ite, kts:kte of ONE ROW j of the tile            (:194)
// so every column of a row waits for the row's largest coefficient (and an N-image run differs from a one-image run: the
// rows of a tile are shorter.  Reproduced, not repaired).
//   k_pbl_coef     one thread per half level (lanes along i): the clipped Kq of :100-132 plus the 10*dz cap of :191-192,
//                  stored to the context's scratch; the row maximum of Kq/dz as a maximum of BIT PATTERNS (the quotient is
//                  positive, so unsigned order == float order): block-reduced, then one atomicMax per block and row --
//                  exact and independent of the order of arrival.
//   k_pbl_diffuse  one LEVEL per thread, 2^n whole columns per block (thread = level * cpb + column): the six scalars of a
//                  level live in registers through all sub-steps of the row, the neighbours' values go through LDS (two
//                  buffers, one barrier per sub-step for all six scalars).  A column is read once and written once however
//                  many sub-steps its row takes.  flux(k-1) is recomputed by the thread of level k from the same operands in
//                  the same order as the thread of level k-1 computes it, so both hold the same bits.
// REAL(4) throughout in the reference's operation order (no contraction: build.py's -ffp-contract=off; IEEE division and
// square root; exp() is the C library's expf bit for bit, glibc_flt32.h): 0 differing bits against the compiled reference.
#include "ctx.h"
#include "glibc_flt32.h"
#include <algorithm>
#include <cstdio>

namespace {
constexpr float gravity = 9.81f, karman = 0.41f;                      // icar_constants.f90; pbl_simple.f90:57
constexpr float pr_upper_limit = 4.0f, pr_lower_limit = 0.25f;        // :59-60
constexpr float asymp_length_scale = 1 / 250.0f;                      // :61
constexpr float N_substeps = 10.0f, diffusion_reduction = 2.0f;       // :64-65
constexpr int kLC_WATER = 2;                                          // icar_constants.f90 (land_mask: land = 1, water = 2)

struct PblTile { int i0, i1, j0, k0, k1; };     // 0-based, inclusive; k0..k1 are the HALF levels (between k and k+1), k1 + 1 <= nz - 1

__global__ void __launch_bounds__(256)
k_pbl_coef(Dims d, PblTile t, float dt, const float *__restrict__ th, const float *__restrict__ qv, const float *__restrict__ qc,
           const float *__restrict__ qi, const float *__restrict__ qr, const float *__restrict__ qs,
           const float *__restrict__ um, const float *__restrict__ vm, const float *__restrict__ pii,
           const float *__restrict__ z, const float *__restrict__ dz, const float *__restrict__ terrain,
           const int *__restrict__ land_mask, float *__restrict__ Kq, unsigned *__restrict__ rowmax)
{
    __shared__ unsigned part[4];
    const int i = t.i0 + blockIdx.x * 64 + threadIdx.x, k = t.k0 + blockIdx.y * 4 + threadIdx.y, j = t.j0 + blockIdx.z;
    unsigned r = 0u;
    if (i <= t.i1 && k <= t.k1) {
        const int a = d.idx(i, k, j), b = a + d.sk, c2 = i + d.nx * j;
        const float dza = dz[a], dzb = dz[b];
        // calc_shear :219-223
        const float du = um[b] - um[a], dv = vm[b] - vm[a];
        float shear = sqrtf(du * du + dv * dv) / ((dza + dzb) * 0.5f);
        if (shear < 1e-5f) shear = 1e-5f;
        // calc_virt_pot_temp_zgradient :241-246
        const float tha = th[a], thb = th[b];
        const float v1 = tha * (1 + 0.61f * qv[a] - (qc[a] + qi[a] + qr[a] + qs[a]));
        const float v2 = thb * (1 + 0.61f * qv[b] - (qc[b] + qi[b] + qr[b] + qs[b]));
        const float grad = (v2 - v1) / ((dza + dzb) * 0.5f);
        // calc_richardson_gradient :286-289
        const float temperature = (tha * pii[a] + thb * pii[b]) / 2;
        float rig = gravity / temperature * grad * 1 / (shear * shear);
        if (rig < -100.0f) rig = -100.0f;
        // calc_pbl_stability_function :255-269
        float stability = 0.0f;
        if (rig > 0) stability = gf_expf(-8.5f * rig) + 0.15f / (rig + 3);
        if (rig <= 0) stability = 1 / sqrtf(1 - 1.6f * rig);
        float prandtl = 1.5f + 3.08f * rig;
        if (prandtl > pr_upper_limit) prandtl = pr_upper_limit;
        else if (prandtl < pr_lower_limit) prandtl = pr_lower_limit;
        // simple_pbl :108-131
        const float l = 1 / (1 / (karman * (z[a] - terrain[c2])) + asymp_length_scale);
        const float K = l * l * stability * shear;
        float kq = K / prandtl;
        kq = kq * dt / ((dza + dzb) / 2);
        if (kq > 1000) kq = 1000;
        else if (kq < 1) kq = 1;
        if (land_mask && land_mask[c2] == kLC_WATER) kq = kq / 1000.0f;
        kq = kq / diffusion_reduction;
        // pbl_diffusion :191-194
        if (kq > N_substeps * dza) kq = dza * N_substeps;
        Kq[a] = kq;
        r = __float_as_uint(kq / dza);
    }
    for (int o = 32; o > 0; o >>= 1) r = max(r, (unsigned)__shfl_down((int)r, o));
    if (threadIdx.x == 0) part[threadIdx.y] = r;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        r = max(max(part[0], part[1]), max(part[2], part[3]));
        if (r) atomicMax(rowmax + j, r);
    }
}

// levels k0 .. k1+1 of cpb columns per block; nl = k1 - k0 + 2 levels; blockDim.x >= cpb * nl (a multiple of 64)
__global__ void __launch_bounds__(1024)
k_pbl_diffuse(Dims d, PblTile t, int cpb, int nl, const float *__restrict__ Kq, const unsigned *__restrict__ rowmax,
              const float *__restrict__ rho, const float *__restrict__ dz, float *__restrict__ qv, float *__restrict__ th,
              float *__restrict__ qc, float *__restrict__ qi, float *__restrict__ qs, float *__restrict__ qr)
{
    extern __shared__ float lds_pbl[];               // [2][6][blockDim.x]
    const int nt = blockDim.x, tid = threadIdx.x;
    const int col = tid % cpb, lev = tid / cpb;
    const int i = t.i0 + blockIdx.x * cpb + col, j = t.j0 + blockIdx.y, k = t.k0 + lev;
    const bool active = i <= t.i1 && lev < nl;
    const bool bottom = lev == 0, top = lev == nl - 1;
    // :194 (a row of finite fields gives 1 .. 21; the bound only keeps a row of Inf / NaN from looping for minutes)
    const int nsubsteps = min((int)ceilf(2 * __uint_as_float(rowmax[j])), 1 << 10);
    float *q_g[6] = {qv, th, qc, qi, qs, qr};        // the order of pbl_diffusion :196-209 (the scalars do not interact)
    float q[6] = {0, 0, 0, 0, 0, 0};
    float kr = 0.0f, krb = 0.0f, rho_dz = 1.0f;      // Kq * rhomean of this half level and of the one below; dz * rho (:181-182)
    int c = 0;
    if (active) {
        c = d.idx(i, k, j);
        const float rc = rho[c];
        if (!top) { kr = (Kq[c] / nsubsteps) * ((rc + rho[c + d.sk]) / 2); rho_dz = dz[c] * rc; }           // :195, :182, :181
        if (!bottom) { const float rb = rho[c - d.sk]; krb = (Kq[c - d.sk] / nsubsteps) * ((rb + rc) / 2); if (top) rho_dz = dz[c - d.sk] * rb; }   // :161 divides by rho_dz(kte)
#pragma unroll
        for (int s = 0; s < 6; ++s) q[s] = q_g[s][c];
    }
    for (int n = 0; n < nsubsteps; ++n) {
        float *buf = lds_pbl + (n & 1) * 6 * nt;
#pragma unroll
        for (int s = 0; s < 6; ++s) buf[s * nt + tid] = q[s];
        __syncthreads();
        if (active) {
#pragma unroll
            for (int s = 0; s < 6; ++s) {                                                 // diffuse_variable :151-161
                const float f = top ? 0.0f : kr * (q[s] - buf[s * nt + tid + cpb]);       // fluxes(k)
                const float fb = bottom ? 0.0f : krb * (buf[s * nt + tid - cpb] - q[s]);  // fluxes(k-1)
                if (bottom) q[s] = q[s] - f / rho_dz;
                else if (top) q[s] = q[s] + fb / rho_dz;
                else q[s] = q[s] - (f - fb) / rho_dz;
            }
        }
    }
    if (active && nsubsteps > 0) {
#pragma unroll
        for (int s = 0; s < 6; ++s) q_g[s][c] = q[s];
    }
}

const float *need(icar_hip_ctx *c, int f, const char *member)
{
    if (c->field[f]) return (const float *)c->field[f];
    char b[160]; snprintf(b, sizeof b, "pbl_simple: domain%%%s (field %d) is not on the device", member, f);
    icar_set_error(b);
    return nullptr;
}
}  // namespace

// columns per block and threads of k_pbl_diffuse for nl levels (2 .. 1024): the largest power of two of whole columns that
// fits 1024 threads, at most a wave's width
static void pbl_geometry(int nl, int &cpb, int &nt)
{
    cpb = 64;
    while (cpb > 1 && cpb * nl > 1024) cpb >>= 1;
    nt = (cpb * nl + 63) / 64 * 64;
}

int icar_pbl_simple_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte_in)
{
    if (its < c->ims || ite > c->ime || jts < c->jms || jte > c->jme || kts < c->kms || kte_in > c->kme) { icar_set_error("pbl_simple: tile outside memory bounds"); return 1; }
    if (c->d.nz > 1024) { icar_set_error("pbl_simple: more than 1024 levels are not supported"); return 1; }
    const int kte = std::min(c->kme - 1, kte_in);                                                            // :92
    if (c->d.nz < 2 || kte < kts) {
        icar_set_error("pbl_simple: needs at least two levels (kts..min(kme-1, kte) is empty: the maxval of pbl_simple.f90:194 has nothing to look at)");
        return 1;
    }
    if (ite < its || jte < jts) return 0;
    float *th = (float *)need(c, ICAR_F_POTENTIAL_TEMPERATURE, "potential_temperature"), *qv = (float *)need(c, ICAR_F_WATER_VAPOR, "water_vapor");
    float *qc = (float *)need(c, ICAR_F_CLOUD_WATER, "cloud_water_mass"), *qi = (float *)need(c, ICAR_F_CLOUD_ICE, "cloud_ice_mass");
    float *qr = (float *)need(c, ICAR_F_RAIN, "rain_mass"), *qs = (float *)need(c, ICAR_F_SNOW, "snow_mass");
    if (!th || !qv || !qc || !qi || !qr || !qs) return 1;
    const float *um = need(c, ICAR_F_U_MASS, "u_mass"), *vm = need(c, ICAR_F_V_MASS, "v_mass"), *pii = need(c, ICAR_F_EXNER, "exner");
    const float *rho = need(c, ICAR_F_DENSITY, "density"), *z = need(c, ICAR_F_Z, "z"), *dz = need(c, ICAR_F_DZ_MASS, "dz_mass");
    const float *terrain = need(c, ICAR_F_TERRAIN, "terrain");
    if (!um || !vm || !pii || !rho || !z || !dz || !terrain) return 1;
    const int *land = (const int *)c->field[ICAR_F_LAND_MASK];          // never uploaded: every cell is land (kLC_LAND)
    // scratch of the context, allocated on first use: Kq (4 B per cell) and the row maxima (4 B per row)
    if (!c->pbl_kq) HIPCHK(hipMalloc(&c->pbl_kq, c->n3 * sizeof(float)));
    if (!c->pbl_rowmax) HIPCHK(hipMalloc(&c->pbl_rowmax, (size_t)c->d.ny * sizeof(unsigned)));
    PblTile t;
    t.i0 = its - c->ims; t.i1 = ite - c->ims; t.j0 = jts - c->jms; t.k0 = kts - c->kms; t.k1 = kte - c->kms;
    const int ni = t.i1 - t.i0 + 1, nj = jte - jts + 1, nk = t.k1 - t.k0 + 1;
    if (nj > 65535) { icar_set_error("pbl_simple: more than 65535 rows per call are not supported"); return 1; }
    int cpb, nt;
    pbl_geometry(nk + 1, cpb, nt);
    ScopedTimer timer(c, "pbl");
    HIPCHK(hipMemsetAsync(c->pbl_rowmax, 0, (size_t)c->d.ny * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(k_pbl_coef, dim3((ni + 63) / 64, (nk + 3) / 4, nj), dim3(64, 4), 0, c->stream, c->d, t, dt,
                       th, qv, qc, qi, qr, qs, um, vm, pii, z, dz, terrain, land, c->pbl_kq, c->pbl_rowmax);
    hipLaunchKernelGGL(k_pbl_diffuse, dim3((ni + cpb - 1) / cpb, nj), dim3(nt), (size_t)2 * 6 * nt * sizeof(float), c->stream, c->d, t, cpb, nk + 1,
                       c->pbl_kq, c->pbl_rowmax, rho, dz, qv, th, qc, qi, qs, qr);
    HIPCHK(hipGetLastError());
    return 0;
}

// pbl(domain, options, dt) (pbl_driver.f90:197-354): the configured scheme on the tile of icar_hip_step_configure
int icar_pbl_run(icar_hip_ctx *c, float dt)
{
    if (c->step.boundarylayer == ICAR_PBL_YSU) return icar_ysu_pbl_run(c, dt);      // :223-354, pbl_ysu.hip
    if (c->step.boundarylayer != ICAR_PBL_SIMPLE) return 0;            // (kPBL_BASIC: the reference's driver has no branch for it)
    const icar_hip_step_config &g = c->step.cfg;
    return icar_pbl_simple_run(c, dt, g.its, g.ite, g.jts, g.jte, g.kts, g.kte);
}

// the rows' sub-step counts of the last call (test and measurement helper behind icar_hip_pbl_nsubsteps)
int icar_pbl_nsubsteps_copy(icar_hip_ctx *c, int *out, int n)
{
    if (!c->pbl_rowmax) { icar_set_error("pbl_nsubsteps: pbl_simple has not run on this context"); return 1; }
    if (n != c->d.ny) { icar_set_error("pbl_nsubsteps: one value per row jms..jme"); return 1; }
    std::vector<float> m(n);
    HIPCHK(hipMemcpyAsync(m.data(), c->pbl_rowmax, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int j = 0; j < n; ++j) out[j] = (int)ceilf(2 * m[j]);
    return 0;
}
