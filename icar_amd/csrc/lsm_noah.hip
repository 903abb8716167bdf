// icar_amd/csrc/lsm_noah.hip -- the Noah land-surface model on gfx950 (landsurface = kLSM_NOAH = 3): lsm_init's Noah part
// (src/physics/lsm_driver.f90:619-711 with allocate_noah_data :425-520 and LSM_NOAH_INIT, src/physics/lsm_noahdrv.f90:1021-1193) and
// the call of lsm_noah (lsm_driver.f90:1210-1278; lsm_noahdrv.f90:36-1018 with SFLX, src/physics/lsm_noahlsm.f90).  The cell code is
// noah_column.h, which also says what is not built and what a land-ice cell leaves alone.
//
//   k_noah        ONE THREAD PER CELL (i, j) of its..ite x jts..jte, lanes along i: the every-call water block, the land-ice arm and
//                 SFLX in the same launch.  A cell has no neighbour and no level loop: four soil layers, all in registers.
//   k_noah_init   LSM_NOAH_INIT's per-cell part on the same grid
//   k_noah_mask   lsm_driver.f90:710: land_mask = kLC_WATER where veg_type is the water or the lake category
//
// The tables.  REDPRM and LSM_NOAH_INIT index the vegetation and soil tables with the cell's own category, which differs from lane to
// lane: a scalar load needs an address that is the same in every lane of the wave, so the scalar cache cannot serve them.  The
// tables are 1 047 REAL(4) (4.2 KB) in device memory, packed in the order of the NP_* offsets below; every block copies them into LDS once
// (16 or 17 coalesced dwords per thread of a 64-thread block, one barrier) and the cell code reads them there through NoahTables' pointers:
// a ds_read_b32 per parameter with lanes on arbitrary banks (at most one extra LDS cycle per lane that shares a bank, no global gather,
// no dependence on what the vector cache still holds).  The 39 parameters a cell reads are nothing beside SFLX's arithmetic.
//
// REAL(4) throughout in the reference's operation order: no contraction, IEEE division; expf, exp2f, logf, log10f and powf are
// glibc's, restated in glibc_flt32.h.
#include "ctx.h"
#include "glibc_flt32.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define NOAH_FN __device__ static __forceinline__
#define NOAH_EXPF gf_expf
#define NOAH_EXP2F gf_exp2f
#define NOAH_LOGF gf_logf
#define NOAH_LOG10F gf_log10f
#define NOAH_POWF gf_powf
__device__ static __forceinline__ float noah_opaque(float x) { asm volatile("" : "+v"(x)); return x; }
#define NOAH_OPAQUE(x) noah_opaque(x)
#include "noah_column.h"

// the tables on the device: every array of icar_hip_noah_tables_t with the reference's extent, then the scalars
enum { NP_NROTBL = 0, NP_VEG = NP_NROTBL + NOAH_NLUS, NP_SOIL = NP_VEG + 13 * NOAH_NLUS, NP_SLOPE = NP_SOIL + 10 * NOAH_NSLTYPE,
       NP_GEN = NP_SLOPE + NOAH_NSLOPE, NP_INT = NP_GEN + 13, NP_N = NP_INT + 4 };

// The ICAR_NOAH_* arrays are planes of ONE allocation, array w at plane_of(w) (the four soil arrays, of four planes each, last): a
// kernel then needs one base pointer and forms every address from constants.  Passed as 48 separate pointers, the arrays' addresses
// alone took 96 scalar registers from the first load to the last store and the compiler spilled 153 of them.
enum { NOAH_PLANES = ICAR_NOAH_SOIL_WATER_CONTENT + NOAH_NSOIL * (ICAR_NOAH_N - ICAR_NOAH_SOIL_WATER_CONTENT) };
__host__ __device__ constexpr int plane_of(int w) { return w < ICAR_NOAH_SOIL_WATER_CONTENT ? w : ICAR_NOAH_SOIL_WATER_CONTENT + NOAH_NSOIL * (w - ICAR_NOAH_SOIL_WATER_CONTENT); }

struct NoahState {
    float *slab = nullptr;                   // NOAH_PLANES planes of nx ny words
    float *arr[ICAR_NOAH_N] = {nullptr};     // ... and where each array starts in it
    bool uploaded[ICAR_NOAH_N] = {false};
    float *tab = nullptr;                    // NP_N words
    bool tables = false, initialised = false;
    int lucats = 0, slcats = 0;
    icar_hip_noah_options_t opt;
};

namespace {
bool is_soil(int w) { return w >= ICAR_NOAH_SOIL_WATER_CONTENT && w <= ICAR_NOAH_SMCREL; }
size_t count(const icar_hip_ctx *c, int w) { return (size_t)c->d.nx * c->d.ny * (is_soil(w) ? NOAH_NSOIL : 1); }

struct NoahArgs {
    int nx, nz, i0, nxt, j0, k0;
    float dt;
    int isurban, isice, lucats, slcats;
    const float *tab;
    const float *qv, *p8w, *t;
    const int *land_mask, *veg, *soiltyp;
    float *slab;                             // the ICAR_NOAH_* arrays, n2 words per plane
    size_t n2;
    float *ext[8];                           // the context's fields among lsm_noah's arguments, by EXT_*
};

// where lsm_noah's arguments live, in the order of NOAH_IN_FIELDS and NOAH_IO_FIELDS: an ICAR_NOAH_* array, or ~EXT_* for a field of the context
enum { EXT_SHORTWAVE = 0, EXT_LONGWAVE, EXT_SKIN_TEMPERATURE, EXT_SENSIBLE_HEAT, EXT_QFX, EXT_LATENT_HEAT, EXT_ROUGHNESS_Z0, EXT_QSFC };
__device__ constexpr int kIn[12] = {ICAR_NOAH_QGH, ~EXT_SHORTWAVE, ~EXT_LONGWAVE, ICAR_NOAH_SOIL_DEEP_TEMPERATURE, ICAR_NOAH_VEGFRAC, ICAR_NOAH_SHDMIN,
                                    ICAR_NOAH_SHDMAX, ICAR_NOAH_SNOALB, ICAR_NOAH_CURRENT_PRECIPITATION, ICAR_NOAH_CQS2, ICAR_NOAH_CHS, ICAR_NOAH_RI};
__device__ constexpr int kIo[32] = {~EXT_SKIN_TEMPERATURE, ~EXT_SENSIBLE_HEAT, ~EXT_QFX, ~EXT_LATENT_HEAT, ICAR_NOAH_GROUND_HEAT_FLUX, ICAR_NOAH_SMSTAV,
                                    ICAR_NOAH_SOIL_TOTALMOISTURE, ICAR_NOAH_SFCRUNOFF, ICAR_NOAH_UDRUNOFF, ICAR_NOAH_ALBEDO, ICAR_NOAH_ALBBCK, ~EXT_ROUGHNESS_Z0,
                                    ICAR_NOAH_Z0, ICAR_NOAH_EMISS, ICAR_NOAH_SNOWC, ~EXT_QSFC, ICAR_NOAH_SNOW_WATER_EQUIVALENT, ICAR_NOAH_SNOW_HEIGHT,
                                    ICAR_NOAH_CANOPY_WATER, ICAR_NOAH_CHS2, ICAR_NOAH_CHKLOWQ, ICAR_NOAH_LAI, ICAR_NOAH_SNOTIME, ICAR_NOAH_ACSNOM,
                                    ICAR_NOAH_ACSNOW, ICAR_NOAH_SNOPCX, ICAR_NOAH_POTEVP, ICAR_NOAH_NOAHRES, ICAR_NOAH_FLX4, ICAR_NOAH_FVB, ICAR_NOAH_FBUR,
                                    ICAR_NOAH_FGSN};
__device__ constexpr int kSoil[4] = {ICAR_NOAH_SOIL_WATER_CONTENT, ICAR_NOAH_SOIL_TEMPERATURE, ICAR_NOAH_SH2O, ICAR_NOAH_SMCREL};
__device__ __forceinline__ float *where(const NoahArgs &a, int w) { return w >= 0 ? a.slab + (size_t)plane_of(w) * a.n2 : a.ext[~w]; }

__device__ __forceinline__ void tables_to_lds(const float *tab, float *lds, NoahTables *T)
{
    for (int n = threadIdx.x; n < NP_N; n += 64) lds[n] = tab[n];
    __syncthreads();
    T->nrotbl = (const int *)(lds + NP_NROTBL);
    const float *v = lds + NP_VEG, *s = lds + NP_SOIL, *g = lds + NP_GEN;
    T->snuptbl = v; T->rstbl = v + NOAH_NLUS; T->rgltbl = v + 2 * NOAH_NLUS; T->hstbl = v + 3 * NOAH_NLUS; T->maxalb = v + 4 * NOAH_NLUS;
    T->emissmintbl = v + 5 * NOAH_NLUS; T->emissmaxtbl = v + 6 * NOAH_NLUS; T->laimintbl = v + 7 * NOAH_NLUS; T->laimaxtbl = v + 8 * NOAH_NLUS;
    T->z0mintbl = v + 9 * NOAH_NLUS; T->z0maxtbl = v + 10 * NOAH_NLUS; T->albedomintbl = v + 11 * NOAH_NLUS; T->albedomaxtbl = v + 12 * NOAH_NLUS;
    T->bb = s; T->drysmc = s + NOAH_NSLTYPE; T->f11 = s + 2 * NOAH_NSLTYPE; T->maxsmc = s + 3 * NOAH_NSLTYPE; T->refsmc = s + 4 * NOAH_NSLTYPE;
    T->satpsi = s + 5 * NOAH_NSLTYPE; T->satdk = s + 6 * NOAH_NSLTYPE; T->satdw = s + 7 * NOAH_NSLTYPE; T->wltsmc = s + 8 * NOAH_NSLTYPE;
    T->qtz = s + 9 * NOAH_NSLTYPE;
    T->slope_data = lds + NP_SLOPE;
    T->topt_data = g[0]; T->cmcmax_data = g[1]; T->cfactr_data = g[2]; T->rsmax_data = g[3]; T->sbeta_data = g[4]; T->fxexp_data = g[5];
    T->csoil_data = g[6]; T->salp_data = g[7]; T->refdk_data = g[8]; T->refkdt_data = g[9]; T->frzk_data = g[10]; T->zbot_data = g[11];
    T->lvcoef_data = g[12];
    const int *n = (const int *)(lds + NP_INT);
    T->bare = n[0]; T->lucats = n[1]; T->slcats = n[2]; T->slpcats = n[3];
}

// a cell's categories must name a row of the tables that was read.  icar_hip_lsm_init checks every cell (k_noah_check) before it writes
// anything and fails otherwise, and new categories or new tables need a new init, so k_noah's own guard is never taken: it only keeps a
// land cell with such a category away from the tables should that ever change
__device__ __forceinline__ bool categories_ok(const NoahArgs &a, int veg, int soil) { return veg >= 1 && veg <= a.lucats && soil >= 1 && soil <= a.slcats; }

__global__ void __launch_bounds__(64)
k_noah(NoahArgs a)
{
    __shared__ float lds[NP_N];
    NoahTables T;
    tables_to_lds(a.tab, lds, &T);
    const int ii = blockIdx.x * 64 + threadIdx.x;
    if (ii >= a.nxt) return;
    const int i = a.i0 + ii, j = a.j0 + blockIdx.y;
    const size_t at = (size_t)a.nx * j + i, at3 = (size_t)a.nx * ((size_t)a.nz * j + a.k0) + i, ats = (size_t)a.nx * ((size_t)NOAH_NSOIL * j) + i;
    NoahCell c;
    c.qv = a.qv[at3]; c.p8w1 = a.p8w[at3]; c.p8w2 = a.p8w[at3 + a.nx]; c.t = a.t[at3];
    c.xland = a.land_mask ? (float)a.land_mask[at] : 1.0f;                          // real(domain%land_mask); never uploaded = all land
    c.ivgtyp = a.veg[at]; c.isltyp = a.soiltyp[at];
    if ((c.xland - 1.5f) < 0.f && !categories_ok(a, c.ivgtyp, c.isltyp)) return;
    int n = 0;
#define NOAH_X(name) c.name = where(a, kIn[n++])[at];
    NOAH_IN_FIELDS(NOAH_X)
#undef NOAH_X
    n = 0;
#define NOAH_X(name) c.name = where(a, kIo[n++])[at];
    NOAH_IO_FIELDS(NOAH_X)
#undef NOAH_X
    n = 0;
#define NOAH_X(name) { const float *p = where(a, kSoil[n++]) + ats; for (int s = 0; s < NOAH_NSOIL; ++s) c.name[s] = p[(size_t)s * a.nx]; }
    NOAH_SOIL_FIELDS(NOAH_X)
#undef NOAH_X
    noah_cell(&T, &c, a.dt, a.isurban, a.isice);
    n = 0;
#define NOAH_X(name) where(a, kIo[n++])[at] = c.name;
    NOAH_IO_FIELDS(NOAH_X)
#undef NOAH_X
    n = 0;
#define NOAH_X(name) { float *p = where(a, kSoil[n++]) + ats; for (int s = 0; s < NOAH_NSOIL; ++s) p[(size_t)s * a.nx] = c.name[s]; }
    NOAH_SOIL_FIELDS(NOAH_X)
#undef NOAH_X
}

// every cell of the memory has categories that name a row of the tables, or the flag is raised; nothing else is written
__global__ void k_noah_check(size_t n, const int *__restrict__ veg, const int *__restrict__ soiltyp, int lucats, int slcats, int *__restrict__ flag)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && !(veg[t] >= 1 && veg[t] <= lucats && soiltyp[t] >= 1 && soiltyp[t] <= slcats)) atomicOr(flag, 1);
}

// LSM_NOAH_INIT :1095-1188.  A DEVIATION, on cells no result depends on: the reference runs it on the tile its .. min(ite, ide-1),
// jts .. min(jte, jde-1) that lsm_init takes from domain%grid (lsm_driver.f90:550-553, :705), so the halo cells of an image keep SH2O = 0.25
// and SNOALB = 0.8 and their SNOW_HEIGHT is not re-derived; here every cell of the memory is initialised (icar_hip_lsm_init takes no
// tile, and a later icar_hip_lsm_noah may name any tile of the memory), and a halo cell's category is checked like an owned one's.  lsm_noah
// reads no neighbour, so no owned cell differs.
__global__ void __launch_bounds__(64)
k_noah_init(NoahArgs a, int fndsnowh, const float *__restrict__ tslb, const float *__restrict__ smois, float *__restrict__ sh2o,
            float *__restrict__ snoalb, const float *__restrict__ snow, float *__restrict__ snowh, float *__restrict__ canwat)
{
    __shared__ float lds[NP_N];
    NoahTables T;
    tables_to_lds(a.tab, lds, &T);
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= a.nx) return;
    const size_t at = (size_t)a.nx * j + i, ats = (size_t)a.nx * ((size_t)NOAH_NSOIL * j) + i;
    const int veg = a.veg[at], soil = a.soiltyp[at];
    if (!categories_ok(a, veg, soil)) return;                                      // (k_noah_check has refused the call)
    float st[NOAH_NSOIL], sm[NOAH_NSOIL], sw[NOAH_NSOIL];
    for (int s = 0; s < NOAH_NSOIL; ++s) { st[s] = tslb[ats + (size_t)s * a.nx]; sm[s] = smois[ats + (size_t)s * a.nx]; sw[s] = sh2o[ats + (size_t)s * a.nx]; }
    noah_init_cell(&T, veg, soil, st, sm, sw, &snoalb[at], snow[at], &snowh[at], &canwat[at], fndsnowh);
    for (int s = 0; s < NOAH_NSOIL; ++s) sh2o[ats + (size_t)s * a.nx] = sw[s];
}

__global__ void k_noah_mask(size_t n, const int *__restrict__ veg, int iswater, int islake, int *__restrict__ land_mask)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && (veg[t] == iswater || veg[t] == islake)) land_mask[t] = 2;
}

// :674-675: where(x < floor) x = floor
__global__ void k_noah_floor(size_t n, float *__restrict__ x, float floor_)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && x[t] < floor_) x[t] = floor_;
}

__global__ void k_noah_fill(size_t n, float *__restrict__ x, float v)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) x[t] = v;
}

int fill(icar_hip_ctx *c, NoahState *s, int w, float v)
{
    const size_t n = count(c, w);
    hipLaunchKernelGGL(k_noah_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, s->arr[w], v);
    HIPCHK(hipGetLastError());
    return 0;
}

// the categories of every cell against the tables, before icar_hip_lsm_init writes anything
int categories_refused(icar_hip_ctx *c, NoahState *s)
{
    const size_t n2 = (size_t)c->d.nx * c->d.ny;
    int *flag = c->d_flag + 8, h = 0;
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_noah_check, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, c->stream, n2, (const int *)s->arr[ICAR_NOAH_VEG_TYPE],
                       (const int *)s->arr[ICAR_NOAH_SOIL_TYPE], s->lucats, s->slcats, flag);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h) {
        icar_set_error(std::string("lsm_init") + ": a cell's veg_type or soil_type names no row of the tables (1 .. LUCATS, 1 .. SLCATS): the reference reads rows "
                       "that SOIL_VEG_GEN_PARM never filled");
        return 1;
    }
    return 0;
}

void base_args(icar_hip_ctx *c, NoahState *s, NoahArgs *a)
{
    a->nx = c->d.nx; a->nz = c->d.nz; a->tab = s->tab; a->slab = s->slab; a->n2 = (size_t)c->d.nx * c->d.ny; a->lucats = s->lucats; a->slcats = s->slcats;
    a->veg = (const int *)s->arr[ICAR_NOAH_VEG_TYPE]; a->soiltyp = (const int *)s->arr[ICAR_NOAH_SOIL_TYPE];
    a->land_mask = (const int *)c->field[ICAR_F_LAND_MASK];
}

NoahState *state(icar_hip_ctx *c, const char *who)
{
    if (!c->noah || !c->noah->tables) { icar_set_error(std::string(who) + ": the Noah tables are not on the device (icar_hip_noah_tables first)"); return nullptr; }
    return c->noah;
}
}  // namespace

void icar_noah_free(icar_hip_ctx *c)
{
    if (!c->noah) return;
    if (c->noah->slab) hipFree(c->noah->slab);
    if (c->noah->tab) hipFree(c->noah->tab);
    delete c->noah;
    c->noah = nullptr;
}

extern "C" int icar_hip_noah_tables(icar_hip_ctx *c, const icar_hip_noah_tables_t *t)
{
    // the values are looked at first
    if (!t) { icar_set_error("noah_tables: null argument"); return 1; }
    if (t->lucats < 1 || t->lucats > NOAH_NLUS || t->slcats < 1 || t->slcats > NOAH_NSLTYPE || t->slpcats < 1 || t->slpcats > NOAH_NSLOPE) {
        icar_set_error("noah_tables: LUCATS is 1 .. 50 (NLUS), SLCATS 1 .. 30 (NSLTYPE), SLPCATS 1 .. 30 (NSLOPE): module_sf_noahlsm's extents");
        return 1;
    }
    const void *arrays[25] = {t->nrotbl, t->snuptbl, t->rstbl, t->rgltbl, t->hstbl, t->maxalb, t->emissmintbl, t->emissmaxtbl, t->laimintbl, t->laimaxtbl,
                              t->z0mintbl, t->z0maxtbl, t->albedomintbl, t->albedomaxtbl, t->bb, t->drysmc, t->f11, t->maxsmc, t->refsmc, t->satpsi,
                              t->satdk, t->satdw, t->wltsmc, t->qtz, t->slope_data};
    for (const void *p : arrays)
        if (!p) { icar_set_error("noah_tables: a table's pointer is null: every array of icar_hip_noah_tables_t is needed"); return 1; }
    for (int v = 0; v < t->lucats; ++v)
        if (t->nrotbl[v] < 0 || t->nrotbl[v] > NOAH_NSOIL) { icar_set_error("noah_tables: NROTBL is 0 .. 4 (the soil layers of allocate_noah_data)"); return 1; }
    if (t->bare < 1 || t->bare > t->lucats) { icar_set_error("noah_tables: BARE is one of the 1 .. LUCATS categories"); return 1; }
    if (!c) { icar_set_error("noah_tables: null ctx"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    std::vector<float> h(NP_N, 0.0f);
    memcpy(&h[NP_NROTBL], t->nrotbl, sizeof(int) * NOAH_NLUS);
    const float *veg[13] = {t->snuptbl, t->rstbl, t->rgltbl, t->hstbl, t->maxalb, t->emissmintbl, t->emissmaxtbl, t->laimintbl, t->laimaxtbl,
                            t->z0mintbl, t->z0maxtbl, t->albedomintbl, t->albedomaxtbl};
    const float *soil[10] = {t->bb, t->drysmc, t->f11, t->maxsmc, t->refsmc, t->satpsi, t->satdk, t->satdw, t->wltsmc, t->qtz};
    for (int n = 0; n < 13; ++n) memcpy(&h[NP_VEG + n * NOAH_NLUS], veg[n], sizeof(float) * NOAH_NLUS);
    for (int n = 0; n < 10; ++n) memcpy(&h[NP_SOIL + n * NOAH_NSLTYPE], soil[n], sizeof(float) * NOAH_NSLTYPE);
    memcpy(&h[NP_SLOPE], t->slope_data, sizeof(float) * NOAH_NSLOPE);
    const float gen[13] = {t->topt_data, t->cmcmax_data, t->cfactr_data, t->rsmax_data, t->sbeta_data, t->fxexp_data, t->csoil_data, t->salp_data,
                           t->refdk_data, t->refkdt_data, t->frzk_data, t->zbot_data, t->lvcoef_data};
    memcpy(&h[NP_GEN], gen, sizeof gen);
    const int ints[4] = {t->bare, t->lucats, t->slcats, t->slpcats};
    memcpy(&h[NP_INT], ints, sizeof ints);
    if (!c->noah) c->noah = new NoahState();
    NoahState *s = c->noah;
    if (!s->tab) {
        const size_t n2 = (size_t)c->d.nx * c->d.ny;
        HIPCHK(hipMalloc(&s->tab, sizeof(float) * NP_N));
        HIPCHK(hipMalloc(&s->slab, sizeof(float) * NOAH_PLANES * n2));
        HIPCHK(hipMemsetAsync(s->slab, 0, sizeof(float) * NOAH_PLANES * n2, c->stream));     // a domain array that is never uploaded is 0, as domain_t allocates it
        for (int w = 0; w < ICAR_NOAH_N; ++w) s->arr[w] = s->slab + (size_t)plane_of(w) * n2;
    }
    HIPCHK(hipMemcpyAsync(s->tab, h.data(), sizeof(float) * NP_N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->tables = true; s->lucats = t->lucats; s->slcats = t->slcats;
    s->initialised = false;                                                        // the categories were checked against the tables before these
    return 0;
}

static int noah_copy(icar_hip_ctx *c, const char *who, int which, void *host, bool to_device)
{
    NoahState *s = state(c, who);
    if (!s) return 1;
    if (which < 0 || which >= ICAR_NOAH_N) { icar_set_error(std::string(who) + ": `which` is one of ICAR_NOAH_*"); return 1; }
    const size_t bytes = count(c, which) * sizeof(float);
    if (to_device) HIPCHK(hipMemcpyAsync(s->arr[which], host, bytes, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(hipMemcpyAsync(host, s->arr[which], bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (to_device) {
        s->uploaded[which] = true;
        // the categories are checked against the tables by icar_hip_lsm_init: new ones need it again
        if (which == ICAR_NOAH_VEG_TYPE || which == ICAR_NOAH_SOIL_TYPE) s->initialised = false;
    }
    return 0;
}

extern "C" int icar_hip_noah_upload(icar_hip_ctx *c, int which, const void *host)
{
    if (icar_enter(c, "noah_upload", host != nullptr)) return 1;
    return noah_copy(c, "noah_upload", which, const_cast<void *>(host), true);
}

extern "C" int icar_hip_noah_download(icar_hip_ctx *c, int which, void *host)
{
    if (icar_enter(c, "noah_download", host != nullptr)) return 1;
    return noah_copy(c, "noah_download", which, host, false);
}

// lsm_init (lsm_driver.f90:522-711).  landsurface 0 or 1: icar_hip_lsm_configure.  3: the Noah part :619-711
extern "C" int icar_hip_lsm_init(icar_hip_ctx *c, int landsurface, int watersurface, int update_interval, float sh_feedback_fraction,
                                 float lh_feedback_fraction, float sfc_layer_thickness, const icar_hip_noah_options_t *o)
{
    if (landsurface != ICAR_LSM_NOAH) {
        if (landsurface == 4) { icar_set_error("lsm_init: landsurface = 4 (kLSM_NOAHMP) is not built; 0, 1 (kLSM_BASIC) or 3 (kLSM_NOAH)"); return 1; }
        const int rc = icar_hip_lsm_configure(c, landsurface, watersurface, update_interval, sh_feedback_fraction, lh_feedback_fraction, sfc_layer_thickness);
        const std::string e = rc ? icar_hip_last_error() : "";
        if (e.rfind("lsm_configure: ", 0) == 0) icar_set_error("lsm_init: " + e.substr(15));       // a refusal names the entry point that was called
        return rc;
    }
    // the values are looked at first: a host learns what is not built without a device
    if (watersurface == 3) { icar_set_error("lsm_init: watersurface = 3 (kWATER_LAKE) is not built; 0, 1 (kWATER_BASIC, nothing runs) or 2 (kWATER_SIMPLE)"); return 1; }
    if (watersurface < 0 || watersurface > 3) { icar_set_error("lsm_init: watersurface is 0, 1 (kWATER_BASIC, nothing runs) or 2 (kWATER_SIMPLE)"); return 1; }
    if (update_interval < 0 || !(sfc_layer_thickness > 0)) { icar_set_error("lsm_init: update_interval >= 0 seconds and a positive sfc_layer_thickness"); return 1; }
    if (!o) { icar_set_error("lsm_init: landsurface = 3 (kLSM_NOAH) needs options%lsm_options (icar_hip_noah_options_t)"); return 1; }
    if (o->monthly_vegfrac || o->monthly_albedo) {
        icar_set_error("lsm_init: monthly_vegfrac / monthly_albedo (lsm_driver.f90:655-668, :1188-1198) are not built: the host uploads the month's "
                       "ICAR_NOAH_VEGFRAC / ICAR_NOAH_ALBEDO itself");
        return 1;
    }
    if (o->urban_category < 1 || o->ice_category < 1 || o->water_category < 1) {
        icar_set_error("lsm_init: urban_category, ice_category and water_category are categories of LU_Categories (>= 1); lake_category may be -1");
        return 1;
    }
    if (!(o->max_swe > 0)) { icar_set_error("lsm_init: max_swe is positive (options%lsm_options%max_swe)"); return 1; }
    if (!c) { icar_set_error("lsm_init: null ctx"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    NoahState *s = state(c, "lsm_init");
    if (!s) return 1;
    static const struct { int w; const char *member; } must[] = {
        {ICAR_NOAH_VEG_TYPE, "veg_type"}, {ICAR_NOAH_SOIL_TYPE, "soil_type"}, {ICAR_NOAH_VEGFRAC, "vegetation_fraction"}, {ICAR_NOAH_ALBEDO, "albedo"},
        {ICAR_NOAH_SOIL_DEEP_TEMPERATURE, "soil_deep_temperature"}, {ICAR_NOAH_SOIL_WATER_CONTENT, "soil_water_content"},
        {ICAR_NOAH_SOIL_TEMPERATURE, "soil_temperature"}};
    for (const auto &m : must)
        if (!s->uploaded[m.w]) {
            char b[200]; snprintf(b, sizeof b, "lsm_init: domain%%%s (ICAR_NOAH array %d) is not on the device: icar_hip_noah_upload it first", m.member, m.w);
            icar_set_error(b); return 1;
        }
    if (c->d.ny > 65535) { icar_set_error("lsm_init: more than 65535 rows are not supported"); return 1; }
    if (categories_refused(c, s)) return 1;                                        // the last refusal: from here on the state is written
    const size_t n2 = (size_t)c->d.nx * c->d.ny;
    // allocate_noah_data :425-520: the module's own arrays
    static const struct { int w; float v; } init[] = {
        {ICAR_NOAH_SMSTAV, 0.5f}, {ICAR_NOAH_SFCRUNOFF, 0.f}, {ICAR_NOAH_UDRUNOFF, 0.f}, {ICAR_NOAH_SNOWC, 0.f}, {ICAR_NOAH_ACSNOW, 0.f},
        {ICAR_NOAH_ACSNOM, 0.f}, {ICAR_NOAH_SNOALB, 0.8f}, {ICAR_NOAH_QGH, 0.02f}, {ICAR_NOAH_ALBBCK, 0.17f}, {ICAR_NOAH_EMISS, 0.99f},
        {ICAR_NOAH_CHKLOWQ, 0.f}, {ICAR_NOAH_FLX4, 0.f}, {ICAR_NOAH_FVB, 0.f}, {ICAR_NOAH_FBUR, 0.f}, {ICAR_NOAH_FGSN, 0.f}, {ICAR_NOAH_SHDMIN, 0.f},
        {ICAR_NOAH_SHDMAX, 100.f}, {ICAR_NOAH_SNOTIME, 0.f}, {ICAR_NOAH_SNOPCX, 0.f}, {ICAR_NOAH_POTEVP, 0.f}, {ICAR_NOAH_SMCREL, 0.f}, {ICAR_NOAH_RI, 0.f},
        {ICAR_NOAH_NOAHRES, 0.f}, {ICAR_NOAH_SH2O, 0.25f}, {ICAR_NOAH_CHS2, 0.f}, {ICAR_NOAH_CURRENT_PRECIPITATION, 0.f}};
    for (const auto &m : init) if (fill(c, s, m.w, m.v)) return 1;
    // :674-675
    const size_t ns = n2 * NOAH_NSOIL;
    hipLaunchKernelGGL(k_noah_floor, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, ns, s->arr[ICAR_NOAH_SOIL_TEMPERATURE], 200.0f);
    hipLaunchKernelGGL(k_noah_floor, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, ns, s->arr[ICAR_NOAH_SOIL_WATER_CONTENT], 0.0001f);
    HIPCHK(hipGetLastError());
    // :672, :707: canopy_water is kept across LSM_NOAH_INIT, which zeroes it
    float *keep = s->arr[ICAR_NOAH_CQS2];
    HIPCHK(hipMemcpyAsync(keep, s->arr[ICAR_NOAH_CANOPY_WATER], n2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    NoahArgs a{};
    base_args(c, s, &a);
    hipLaunchKernelGGL(k_noah_init, dim3((c->d.nx + 63) / 64, c->d.ny), dim3(64), 0, c->stream, a, o->fndsnowh ? 1 : 0, s->arr[ICAR_NOAH_SOIL_TEMPERATURE],
                       s->arr[ICAR_NOAH_SOIL_WATER_CONTENT], s->arr[ICAR_NOAH_SH2O], s->arr[ICAR_NOAH_SNOALB], s->arr[ICAR_NOAH_SNOW_WATER_EQUIVALENT],
                       s->arr[ICAR_NOAH_SNOW_HEIGHT], s->arr[ICAR_NOAH_CANOPY_WATER]);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->arr[ICAR_NOAH_CANOPY_WATER], keep, n2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (fill(c, s, ICAR_NOAH_CQS2, 0.01f)) return 1;                                // :708
    // :710
    const bool fresh = !c->field[ICAR_F_LAND_MASK];
    int *lm = (int *)icar_field_f(c, ICAR_F_LAND_MASK, false);
    if (!lm) return 1;
    if (fresh) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)lm, 1, n2, c->stream));      // never uploaded = all land (kLC_LAND)
    hipLaunchKernelGGL(k_noah_mask, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, c->stream, n2, (const int *)s->arr[ICAR_NOAH_VEG_TYPE], o->water_category,
                       o->lake_category, lm);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    s->opt = *o;
    s->initialised = true;
    icar_lsm_uncouple(c);                                                          // icar_hip_lsm_noah_couple comes after this call
    IcarStepState &st = c->step;
    st.landsurface = landsurface; st.watersurface = watersurface; st.lsm_update_interval = update_interval;
    st.sh_feedback_fraction = sh_feedback_fraction; st.lh_feedback_fraction = lh_feedback_fraction; st.sfc_layer_thickness = sfc_layer_thickness;
    st.lsm_last_model_time = -999.0;                                               // lsm_driver.f90:1000
    c->sfc_nz_valid = false;
    return 0;
}

// what lsm_noah_driver.hip needs of the state above
bool icar_noah_ready(const icar_hip_ctx *c) { return c->noah && c->noah->tables && c->noah->initialised; }
float *icar_noah_array(icar_hip_ctx *c, int w) { return c->noah->arr[w]; }
float icar_noah_max_swe(const icar_hip_ctx *c) { return c->noah->opt.max_swe; }

// the call of lsm_noah alone (lsm_driver.f90:1210-1278) on its..ite, jts..jte with RAINBL = ICAR_NOAH_CURRENT_PRECIPITATION
extern "C" int icar_hip_lsm_noah(icar_hip_ctx *c, float lsm_dt, int its, int ite, int jts, int jte)
{
    if (!(lsm_dt > 0)) { icar_set_error("lsm_noah: lsm_dt is positive (PRCP = RAINBL / DT, lsm_noahdrv.f90:692)"); return 1; }
    if (icar_enter(c, "lsm_noah")) return 1;
    return icar_noah_run(c, true, lsm_dt, its, ite, jts, jte);
}

// chs_from_host: CHS is the host's (icar_hip_lsm_noah); false: the coupled lsm() has just computed it (lsm_noah_driver.hip)
int icar_noah_run(icar_hip_ctx *c, bool chs_from_host, float lsm_dt, int its, int ite, int jts, int jte)
{
    NoahState *s = state(c, "lsm_noah");
    if (!s) return 1;
    if (!s->initialised) { icar_set_error("lsm_noah: the scheme is not initialised (icar_hip_lsm_init with landsurface = 3, again after new veg_type / soil_type or new tables)"); return 1; }
    if (chs_from_host && !s->uploaded[ICAR_NOAH_CHS]) {
        icar_set_error("lsm_noah: CHS (ICAR_NOAH_CHS) is not on the device: calc_exchange_coefficient (lsm_driver.f90:1028-1030) is not built, the host "
                       "uploads its result before the call");
        return 1;
    }
    if (its < c->ims || ite > c->ime || jts < c->jms || jte > c->jme) { icar_set_error("lsm_noah: tile outside memory bounds"); return 1; }
    if (jte - jts + 1 > 65535) { icar_set_error("lsm_noah: more than 65535 rows are not supported"); return 1; }
    const int kts = c->step.configured ? c->step.cfg.kts : c->kms;
    if (kts != 1 || c->kme < 2) {
        icar_set_error("lsm_noah: lsm_noah names level 1 literally (QV3D(i,1,j), T3D(i,1,j), P8W3D(i,1,j) beside P8W3D(i,kts+1,j), lsm_noahdrv.f90:655-673): "
                       "only kts = 1 with at least two levels is built");
        return 1;
    }
    if (ite < its || jte < jts) return 0;
    NoahArgs a{};
    base_args(c, s, &a);
    a.i0 = its - c->ims; a.nxt = ite - its + 1; a.j0 = jts - c->jms; a.k0 = kts - c->kms; a.dt = lsm_dt;
    a.isurban = s->opt.urban_category; a.isice = s->opt.ice_category;
    static const struct { int f; const char *member; } fields[] = {
        {ICAR_F_WATER_VAPOR, "water_vapor"}, {ICAR_F_PRESSURE_INTERFACE, "pressure_interface"}, {ICAR_F_TEMPERATURE, "temperature"},
        {ICAR_F_SHORTWAVE, "shortwave"}, {ICAR_F_LONGWAVE, "longwave"}, {ICAR_F_SKIN_TEMPERATURE, "skin_temperature"},
        {ICAR_F_SENSIBLE_HEAT, "sensible_heat"}, {ICAR_F_LATENT_HEAT, "latent_heat"}, {ICAR_F_ROUGHNESS_Z0, "roughness_z0"}};
    for (const auto &m : fields)
        if (!c->field[m.f]) {
            char b[200]; snprintf(b, sizeof b, "lsm_noah: domain%%%s (field %d) is not on the device", m.member, m.f);
            icar_set_error(b); return 1;
        }
    float *qfx = icar_field_f(c, ICAR_F_QFX, false), *qsfc = icar_field_f(c, ICAR_F_QSFC, false);      // lsm_driver.f90's own arrays
    if (!qfx || !qsfc) return 1;
    a.qv = (const float *)c->field[ICAR_F_WATER_VAPOR]; a.p8w = (const float *)c->field[ICAR_F_PRESSURE_INTERFACE]; a.t = (const float *)c->field[ICAR_F_TEMPERATURE];
    const int ext[8] = {ICAR_F_SHORTWAVE, ICAR_F_LONGWAVE, ICAR_F_SKIN_TEMPERATURE, ICAR_F_SENSIBLE_HEAT, ICAR_F_QFX, ICAR_F_LATENT_HEAT, ICAR_F_ROUGHNESS_Z0,
                        ICAR_F_QSFC};                                               // EXT_*
    for (int n = 0; n < 8; ++n) a.ext[n] = (float *)c->field[ext[n]];
    ScopedTimer timer(c, "lsm_noah");
    hipLaunchKernelGGL(k_noah, dim3((a.nxt + 63) / 64, jte - jts + 1), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}
