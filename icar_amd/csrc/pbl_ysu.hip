// icar_amd/csrc/pbl_ysu.hip -- the YSU boundary-layer scheme (Hong, Noh and Dudhia 2006; row P2) on gfx950: pbl_init and
// pbl(domain, options, dt) as they run for boundarylayer = kPBL_YSU.
//
// Reference algorithm: src/physics/pbl_driver.f90 -- pbl_init's YSU branch :127-194 (z_atm, gz1oz0, zol = 10, hol = 1000, xland_real,
// the six tendencies zeroed over the memory; ysuinit does nothing else), pbl's YSU branch :223-354 (the 10 m wind speed with its
// 1e-5 floor :227-228, calc_Richardson_nr, atm_utilities.f90:1131-1139, da_sfc_wtq over the whole memory :234-254, ysu on its..ite,
// jts..jte, kts..kte-1 :257-323, the four updates and the six resets over the whole memory :343-354); the cell and column code is
// ysu_column.h, which also says what of the reference is not built and which form each ** takes.  The u / v tendencies are computed
// and thrown away as in the reference (the statements that would apply them are commented out there).
//
//   k_ysu_init     one thread per (i, j) of the memory: z_atm = z(:,kts,:) - terrain, gz1oz0 = log(z_atm / roughness_z0), zol, hol
//   k_ysu_sfc      one thread per (i, j) of the memory: windspd, Ri, and da_sfc_wtq's regime, psim, psih.  Its u10, v10, t2, q2 are
//                  dummies of the driver that nothing reads: not computed.
//   k_ysu_column   ONE THREAD PER COLUMN of its..ite, lanes along i: ysu2d with tridin and the division of ysu :254-259.  The 19
//                  level arrays the scheme keeps (ysu_column.h) live in a device workspace laid out [array][level][column], so that
//                  every access of a wave is one coalesced line and nothing of a column sits in scratch; the column scalars are
//                  registers.  The tile is walked in chunks of rows that fit the workspace (2^17 columns: at 40 levels 400 MB; the
//                  whole of a 512 x 512 tile would take 800 MB, and a launch of 2^17 columns already puts two waves on every SIMD).
//                  The inputs are read from the fields where the scheme reads them (each level a coalesced line), not staged.
//   k_ysu_apply    one thread per cell of the memory: x = x + tend dt for water vapor, cloud water, potential temperature and
//                  cloud ice, then the six tendencies to zero.  Where a tendency is zero (the top level, the halo) this is
//                  x + 0 dt: the identity except that -0.0 becomes +0.0; a field is stored only where its bits change, a tendency
//                  only where it is not zero already.
// REAL(4) throughout in the reference's operation order: no contraction, IEEE division and square root, the C library's expf /
// logf / powf / atanf bit for bit (glibc_flt32.h): 0 differing bits against the compiled reference.
//
// Levels: ysu2d names level 1 literally, so kts /= 1 is refused; with fewer than three model levels kts..kte the scheme's kte-1 is 1,
// its height search `do k = 2,klpbl` never runs and hpbl reads za(i,k-1) = za(i,0) below the array (pbl_ysu.f90:655): refused;
// more than YSU_MAX_LEVELS + 1 = 129 levels: refused (the workspace).
#include "ctx.h"
#include "glibc_flt32.h"
#include <cmath>
#include <cstdio>

#define YSU_FN __device__ static __forceinline__
#define YSU_EXPF gf_expf
#define YSU_LOGF gf_logf
#define YSU_POWF gf_powf
#define YSU_ATANF gf_atanf
#define YSU_SQRTF sqrtf
#include "ysu_column.h"

struct YsuState {
    float *arr[ICAR_YSU_N] = {nullptr};
    float *ws = nullptr;                 // YSU_NARR x ws_levels x ws_cols
    size_t ws_cols = 0;
    int ws_levels = 0;
};

const float *icar_ysu_hpbl(const icar_hip_ctx *c) { return c->ysu ? c->ysu->arr[ICAR_YSU_HPBL] : nullptr; }

namespace {
constexpr size_t kWsColumns = (size_t)1 << 17;       // columns per launch of k_ysu_column (a tile row always fits)

__global__ void __launch_bounds__(256)
k_ysu_init(int n2, int sj, size_t z_at, const float *__restrict__ z, const float *__restrict__ terrain, const float *__restrict__ z0,
           int nx, float *__restrict__ z_atm, float *__restrict__ gz1oz0, float *__restrict__ zol, float *__restrict__ hol)
{
    const int c2 = blockIdx.x * 256 + threadIdx.x;
    if (c2 >= n2) return;
    const int i = c2 % nx, j = c2 / nx;
    const float za = z[z_at + (size_t)sj * j + i] - terrain[c2];                  // pbl_driver.f90:136
    z_atm[c2] = za;
    zol[c2] = 10.0f;                                                              // :138
    hol[c2] = 1000.0f;                                                            // :140
    gz1oz0[c2] = gf_logf(za / z0[c2]);                                            // :151
}

struct SfcArgs {
    int n2, nx, sj;
    size_t at1;                          // offset of (0, level 1, 0) in a 3-D field
    float dx;
    const float *u10, *v10, *t, *tskin, *z_atm, *psfc, *tg, *p, *qc, *um, *vm, *z0, *ustar;
    const int *land;
    float *windspd, *ri, *psim, *psih, *regime;
};

// pbl_driver.f90:227-254 over the memory
__global__ void __launch_bounds__(256)
k_ysu_sfc(SfcArgs a)
{
    const int c2 = blockIdx.x * 256 + threadIdx.x;
    if (c2 >= a.n2) return;
    const int i = c2 % a.nx, j = c2 / a.nx;
    const size_t at = a.at1 + (size_t)a.sj * j + i;
    const float u = a.u10[c2], v = a.v10[c2];
    float w = sqrtf(u * u + v * v);                                               // :227
    if (w == 0) w = 1e-5f;                                                        // :228
    a.windspd[c2] = w;
    const float t = a.t[at], za = a.z_atm[c2];
    a.ri[c2] = 9.81f / t * (t - a.tskin[c2]) * za / (w * w);                      // atm_utilities.f90:1138
    float regime, psim, psih;
    ysu_sfc_cell(a.psfc[c2], a.tg[c2], a.p[at], t, a.qc[at], a.um[at], a.vm[at], za, a.z0[c2], (float)a.land[c2], a.dx, a.ustar[c2],
                 &regime, &psim, &psih);
    a.regime[c2] = regime; a.psim[c2] = psim; a.psih[c2] = psih;
}

struct ColArgs {
    Dims d;
    int i0, nxt, j0, k0, n, nl;          // first column / row (0-based), columns per row, first level, scheme levels, workspace levels
    float dt;
    size_t stride;
    const float *ux, *vx, *tx, *qx, *qcx, *qix, *p, *pint, *pi, *dz;
    float *tu, *tv, *tth, *tqv, *tqc, *tqi, *exch;
    const float *psfc, *znt, *ust, *hfx, *lh, *tsk, *gz1oz0, *wspd, *br, *psim, *psih, *u10, *v10;
    const int *land;
    float *hol, *hpbl, *ws;
    int *kpbl;
};

// call ysu(...) (pbl_driver.f90:257-323) on the rows j0 .. j0+gridDim.y-1
__global__ void __launch_bounds__(64)
k_ysu_column(ColArgs a)
{
    const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y;
    if (ii >= a.nxt) return;
    const int i = a.i0 + ii, j = a.j0 + jj;
    const size_t at = (size_t)a.d.idx(i, a.k0, j), c2 = (size_t)a.d.nx * j + i;
    // the column's addresses are formed now and pinned to vector registers: as wave-uniform bases they would sit in scalar registers
    // across the whole scheme, whose nested divergent control flow needs those for its exec masks (as one set of 35 bases: 66 spilled)
    YsuCol c = {a.ux + at, a.vx + at, a.tx + at, a.qx + at, a.qcx + at, a.qix + at, a.p + at, a.pint + at, a.pi + at, a.dz + at,
                a.tu + at, a.tv + at, a.tth + at, a.tqv + at, a.tqc + at, a.tqi + at, a.exch + at};
    asm volatile("" : "+v"(c.ux), "+v"(c.vx), "+v"(c.tx), "+v"(c.qx), "+v"(c.qcx), "+v"(c.qix), "+v"(c.p2d), "+v"(c.p2di), "+v"(c.pi2d), "+v"(c.dz8w));
    asm volatile("" : "+v"(c.utnp), "+v"(c.vtnp), "+v"(c.ttnp), "+v"(c.qtnp), "+v"(c.qctnp), "+v"(c.qitnp), "+v"(c.exch_h));
    const YsuSfc s = {a.psfc[c2], a.znt[c2], a.ust[c2], (float)a.land[c2], a.hfx[c2], a.lh[c2] / YSU_XLV, a.tsk[c2], a.gz1oz0[c2], a.wspd[c2],
                      a.br[c2], a.psim[c2], a.psih[c2], a.u10[c2], a.v10[c2]};
    float *ph = a.hol + c2, *pp = a.hpbl + c2, *ws = a.ws + ((size_t)jj * a.nxt + ii);
    int *pk = a.kpbl + c2;
    asm volatile("" : "+v"(ph), "+v"(pp), "+v"(pk), "+v"(ws));
    YsuOut o;
    ysu_column(c, (size_t)a.d.sk, a.n, a.dt, s, &o, ws, a.stride, a.nl, nullptr);
    *ph = o.hol; *pp = o.hpbl; *pk = o.kpbl;
}

struct ApplyArgs {
    size_t n3;
    float dt;
    float *qv, *qc, *th, *qi, *tqv, *tqc, *tth, *tqi, *tu, *tv;
};

__device__ __forceinline__ void add_tend(float *x, float *tend, size_t at, float dt)
{
    const float t = tend[at], v = x[at], y = v + t * dt;
    if (__builtin_bit_cast(int, y) != __builtin_bit_cast(int, v)) x[at] = y;
    if (__builtin_bit_cast(int, t) != 0) tend[at] = 0.0f;
}

// pbl_driver.f90:343-354 over the memory
__global__ void __launch_bounds__(256)
k_ysu_apply(ApplyArgs a)
{
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= a.n3) return;
    add_tend(a.qv, a.tqv, at, a.dt);
    add_tend(a.qc, a.tqc, at, a.dt);
    add_tend(a.th, a.tth, at, a.dt);
    add_tend(a.qi, a.tqi, at, a.dt);
    if (__builtin_bit_cast(int, a.tu[at]) != 0) a.tu[at] = 0.0f;
    if (__builtin_bit_cast(int, a.tv[at]) != 0) a.tv[at] = 0.0f;
}

bool is3d(int which) { return which == ICAR_YSU_EXCH_H || which >= ICAR_YSU_TEND_TH; }
size_t count(const icar_hip_ctx *c, int which) { return is3d(which) ? c->n3 : (size_t)c->d.nx * c->d.ny; }

float *need(icar_hip_ctx *c, int f, const char *who, const char *member)
{
    if (c->field[f]) return (float *)c->field[f];
    char b[200]; snprintf(b, sizeof b, "%s: domain%%%s (field %d) is not on the device", who, member, f);
    icar_set_error(b);
    return nullptr;
}

YsuState *state(icar_hip_ctx *c, const char *who)
{
    if (c->ysu) return c->ysu;
    icar_set_error(std::string(who) + ": the YSU scheme is not initialised (icar_hip_pbl_init with boundarylayer = 3)");
    return nullptr;
}

// kts..kte of the call (the model's: ysu runs on kts..kte-1): the levels the scheme can run on (see the header)
int levels_ok(icar_hip_ctx *c, const YsuState *s, int kts, int kte)
{
    char b[360];
    if (kts < c->kms || kte > c->kme) { icar_set_error("ysu: kts..kte outside the levels of the context"); return 1; }
    if (kts != 1) {
        snprintf(b, sizeof b, "ysu: kts = %d: ysu2d names level 1 literally (tx(i,1), zq(i,1), do k = 2,klpbl, pbl_ysu.f90:515-634) and da_sfc_wtq is handed "
                 "level 1 of the memory: only kts = 1 makes sense", kts);
        icar_set_error(b); return 1;
    }
    const int n = kte - kts;
    if (n < YSU_MIN_LEVELS) {
        snprintf(b, sizeof b, "ysu: %d levels (kts..kte): at least %d.  ysu runs on kts..kte-1; with one scheme level its height search `do k = 2,klpbl` "
                 "never runs and hpbl reads za(i,k-1) = za(i,0) below the array (pbl_ysu.f90:655)", kte - kts + 1, YSU_MIN_LEVELS + 1);
        icar_set_error(b); return 1;
    }
    if (n > YSU_MAX_LEVELS || n + 1 > s->ws_levels) {
        snprintf(b, sizeof b, "ysu: %d levels (kts..kte): at most %d (the column workspace is sized for kte - kts <= %d)", kte - kts + 1,
                 YSU_MAX_LEVELS + 1, YSU_MAX_LEVELS);
        icar_set_error(b); return 1;
    }
    return 0;
}

int tile_ok(icar_hip_ctx *c, const char *who, int its, int ite, int jts, int jte)
{
    if (its < c->ims || ite > c->ime || jts < c->jms || jte > c->jme) { icar_set_error(std::string(who) + ": tile outside memory bounds"); return 1; }
    if (jte - jts + 1 > 65535) { icar_set_error(std::string(who) + ": more than 65535 rows are not supported"); return 1; }
    return 0;
}
}  // namespace

void icar_ysu_free(icar_hip_ctx *c)
{
    YsuState *s = c->ysu;
    if (!s) return;
    for (float *p : s->arr) if (p) hipFree(p);
    if (s->ws) hipFree(s->ws);
    delete s;
    c->ysu = nullptr;
}

// pbl_init (pbl_driver.f90:127-194) for kPBL_YSU: the slot's arrays, what it derives from z, terrain and roughness_z0, the workspace
int icar_ysu_init_device(icar_hip_ctx *c)
{
    static const char *who = "pbl_init";
    const float *z = need(c, ICAR_F_Z, who, "z"), *terrain = need(c, ICAR_F_TERRAIN, who, "terrain");
    const float *z0 = need(c, ICAR_F_ROUGHNESS_Z0, who, "roughness_z0");
    // xland_real = real(land_mask) (:156) is not stored: the kernels convert land_mask per cell; here only its presence is checked
    if (!need(c, ICAR_F_LAND_MASK, who, "land_mask") || !z || !terrain || !z0) return 1;
    if (c->kms > 1 || c->kme < 1) { icar_set_error("pbl_init: level 1 (kts of the YSU scheme) is not among the levels of the context"); return 1; }
    YsuState *s = c->ysu;
    if (!s) {
        // built aside and handed to the context only when complete: a failed allocation leaves the context without the scheme
        YsuState *t = new YsuState();
        const size_t n2 = (size_t)c->d.nx * c->d.ny;
        t->ws_cols = n2 < kWsColumns ? n2 : kWsColumns;
        if (t->ws_cols < (size_t)c->d.nx) t->ws_cols = c->d.nx;
        t->ws_levels = c->d.nz < YSU_MAX_LEVELS + 1 ? c->d.nz : YSU_MAX_LEVELS + 1;     // the scheme's n + 1 interfaces, n = kte - kts <= nz - 1
        if (t->ws_levels < 2) t->ws_levels = 2;
        bool ok = true;
        for (int w = 0; w < ICAR_YSU_N && ok; ++w) ok = !icar_hip_check(hipMalloc(&t->arr[w], count(c, w) * sizeof(float)), "hipMalloc of a YSU array");
        ok = ok && !icar_hip_check(hipMalloc(&t->ws, sizeof(float) * YSU_NARR * (size_t)t->ws_levels * t->ws_cols), "hipMalloc of the YSU workspace");
        ok = ok && !icar_hip_check(hipMemsetAsync(t->arr[ICAR_YSU_GROUND_SURF_TEMPERATURE], 0, count(c, ICAR_YSU_GROUND_SURF_TEMPERATURE) * sizeof(float), c->stream),
                                   "hipMemsetAsync");
        if (!ok) {
            for (float *p : t->arr) if (p) hipFree(p);
            if (t->ws) hipFree(t->ws);
            delete t;
            return 1;
        }
        c->ysu = s = t;
    }
    // what the reference allocates without a value (psim, psih, regime, windspd, Ri) and domain%hpbl, %kpbl, %coeff_heat_exchange_3d start
    // at zero here; the six tendencies are zeroed as :163-176 zeroes them
    for (int w = ICAR_YSU_HPBL; w < ICAR_YSU_N; ++w) HIPCHK(hipMemsetAsync(s->arr[w], 0, count(c, w) * sizeof(float), c->stream));
    const int n2 = c->d.nx * c->d.ny;
    hipLaunchKernelGGL(k_ysu_init, dim3((n2 + 255) / 256), dim3(256), 0, c->stream, n2, c->d.sj, (size_t)c->d.idx(0, 1 - c->kms, 0), z, terrain, z0,
                       c->d.nx, s->arr[ICAR_YSU_Z_ATM], s->arr[ICAR_YSU_GZ1OZ0], s->arr[ICAR_YSU_ZOL], s->arr[ICAR_YSU_HOL]);
    HIPCHK(hipGetLastError());
    return 0;
}

// pbl_driver.f90:227-254 alone
int icar_ysu_sfc_run(icar_hip_ctx *c, float dx)
{
    static const char *who = "ysu_sfc";
    YsuState *s = state(c, who);
    if (!s) return 1;
    SfcArgs a;
    a.u10 = need(c, ICAR_F_U_10M, who, "u_10m"); a.v10 = need(c, ICAR_F_V_10M, who, "v_10m"); a.t = need(c, ICAR_F_TEMPERATURE, who, "temperature");
    a.tskin = need(c, ICAR_F_SKIN_TEMPERATURE, who, "skin_temperature"); a.psfc = need(c, ICAR_F_SURFACE_PRESSURE, who, "surface_pressure");
    a.p = need(c, ICAR_F_PRESSURE, who, "pressure"); a.qc = need(c, ICAR_F_CLOUD_WATER, who, "cloud_water_mass");
    a.um = need(c, ICAR_F_U_MASS, who, "u_mass"); a.vm = need(c, ICAR_F_V_MASS, who, "v_mass"); a.z0 = need(c, ICAR_F_ROUGHNESS_Z0, who, "roughness_z0");
    a.ustar = need(c, ICAR_F_USTAR, who, "ustar"); a.land = (const int *)need(c, ICAR_F_LAND_MASK, who, "land_mask");
    if (!a.u10 || !a.v10 || !a.t || !a.tskin || !a.psfc || !a.p || !a.qc || !a.um || !a.vm || !a.z0 || !a.ustar || !a.land) return 1;
    a.n2 = c->d.nx * c->d.ny; a.nx = c->d.nx; a.sj = c->d.sj; a.at1 = (size_t)c->d.idx(0, 1 - c->kms, 0); a.dx = dx;
    a.z_atm = s->arr[ICAR_YSU_Z_ATM]; a.tg = s->arr[ICAR_YSU_GROUND_SURF_TEMPERATURE];
    a.windspd = s->arr[ICAR_YSU_WINDSPD]; a.ri = s->arr[ICAR_YSU_RI]; a.psim = s->arr[ICAR_YSU_PSIM]; a.psih = s->arr[ICAR_YSU_PSIH];
    a.regime = s->arr[ICAR_YSU_REGIME];
    ScopedTimer timer(c, "ysu_sfc");
    hipLaunchKernelGGL(k_ysu_sfc, dim3((a.n2 + 255) / 256), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// call ysu(...) (pbl_driver.f90:257-323) on its..ite, jts..jte, kts..kte-1; the tendencies stay where ysu leaves them
int icar_ysu_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte)
{
    static const char *who = "ysu";
    YsuState *s = state(c, who);
    if (!s || levels_ok(c, s, kts, kte) || tile_ok(c, who, its, ite, jts, jte)) return 1;
    if (ite < its || jte < jts) return 0;
    ColArgs a;
    a.ux = need(c, ICAR_F_U_MASS, who, "u_mass"); a.vx = need(c, ICAR_F_V_MASS, who, "v_mass"); a.tx = need(c, ICAR_F_TEMPERATURE, who, "temperature");
    a.qx = need(c, ICAR_F_WATER_VAPOR, who, "water_vapor"); a.qcx = need(c, ICAR_F_CLOUD_WATER, who, "cloud_water_mass");
    a.qix = need(c, ICAR_F_CLOUD_ICE, who, "cloud_ice_mass"); a.p = need(c, ICAR_F_PRESSURE, who, "pressure");
    a.pint = need(c, ICAR_F_PRESSURE_INTERFACE, who, "pressure_interface"); a.pi = need(c, ICAR_F_EXNER, who, "exner");
    a.dz = need(c, ICAR_F_DZ_INTERFACE, who, "dz_interface"); a.psfc = need(c, ICAR_F_SURFACE_PRESSURE, who, "surface_pressure");
    a.znt = need(c, ICAR_F_ROUGHNESS_Z0, who, "roughness_z0"); a.ust = need(c, ICAR_F_USTAR, who, "ustar");
    a.hfx = need(c, ICAR_F_SENSIBLE_HEAT, who, "sensible_heat"); a.lh = need(c, ICAR_F_LATENT_HEAT, who, "latent_heat");
    a.tsk = need(c, ICAR_F_SKIN_TEMPERATURE, who, "skin_temperature"); a.u10 = need(c, ICAR_F_U_10M, who, "u_10m"); a.v10 = need(c, ICAR_F_V_10M, who, "v_10m");
    a.land = (const int *)need(c, ICAR_F_LAND_MASK, who, "land_mask");
    if (!a.ux || !a.vx || !a.tx || !a.qx || !a.qcx || !a.qix || !a.p || !a.pint || !a.pi || !a.dz || !a.psfc || !a.znt || !a.ust || !a.hfx || !a.lh ||
        !a.tsk || !a.u10 || !a.v10 || !a.land) return 1;
    a.tu = s->arr[ICAR_YSU_TEND_U]; a.tv = s->arr[ICAR_YSU_TEND_V]; a.tth = s->arr[ICAR_YSU_TEND_TH]; a.tqv = s->arr[ICAR_YSU_TEND_QV];
    a.tqc = s->arr[ICAR_YSU_TEND_QC]; a.tqi = s->arr[ICAR_YSU_TEND_QI]; a.exch = s->arr[ICAR_YSU_EXCH_H];
    a.gz1oz0 = s->arr[ICAR_YSU_GZ1OZ0]; a.wspd = s->arr[ICAR_YSU_WINDSPD]; a.br = s->arr[ICAR_YSU_RI]; a.psim = s->arr[ICAR_YSU_PSIM];
    a.psih = s->arr[ICAR_YSU_PSIH]; a.hol = s->arr[ICAR_YSU_HOL]; a.hpbl = s->arr[ICAR_YSU_HPBL]; a.kpbl = (int *)s->arr[ICAR_YSU_KPBL];
    a.ws = s->ws;
    a.d = c->d; a.i0 = its - c->ims; a.nxt = ite - its + 1; a.k0 = kts - c->kms; a.n = kte - kts; a.nl = s->ws_levels; a.dt = dt;
    const int rows_per = (int)(s->ws_cols / (size_t)a.nxt);          // >= 1: ws_cols >= nx
    // [array][level][column] with the column count of one launch: (array nl + level) stride + column < YSU_NARR ws_levels ws_cols
    a.stride = (size_t)rows_per * a.nxt;
    ScopedTimer timer(c, "ysu");
    for (int j = jts; j <= jte; j += rows_per) {
        const int rows = jte - j + 1 < rows_per ? jte - j + 1 : rows_per;
        a.j0 = j - c->jms;
        hipLaunchKernelGGL(k_ysu_column, dim3((a.nxt + 63) / 64, rows), dim3(64), 0, c->stream, a);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// pbl_driver.f90:343-354 over the memory
static int ysu_apply_run(icar_hip_ctx *c, YsuState *s, float dt)
{
    static const char *who = "pbl";
    ApplyArgs a;
    a.qv = need(c, ICAR_F_WATER_VAPOR, who, "water_vapor"); a.qc = need(c, ICAR_F_CLOUD_WATER, who, "cloud_water_mass");
    a.th = need(c, ICAR_F_POTENTIAL_TEMPERATURE, who, "potential_temperature"); a.qi = need(c, ICAR_F_CLOUD_ICE, who, "cloud_ice_mass");
    if (!a.qv || !a.qc || !a.th || !a.qi) return 1;
    a.n3 = c->n3; a.dt = dt;
    a.tqv = s->arr[ICAR_YSU_TEND_QV]; a.tqc = s->arr[ICAR_YSU_TEND_QC]; a.tth = s->arr[ICAR_YSU_TEND_TH]; a.tqi = s->arr[ICAR_YSU_TEND_QI];
    a.tu = s->arr[ICAR_YSU_TEND_U]; a.tv = s->arr[ICAR_YSU_TEND_V];
    ScopedTimer timer(c, "ysu_apply");
    hipLaunchKernelGGL(k_ysu_apply, dim3((unsigned)((a.n3 + 255) / 256)), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// pbl(domain, options, dt) for kPBL_YSU (pbl_driver.f90:223-354) on the tile of icar_hip_step_configure
int icar_ysu_pbl_run(icar_hip_ctx *c, float dt)
{
    YsuState *s = state(c, "pbl");
    if (!s) return 1;
    const icar_hip_step_config &g = c->step.cfg;
    if (levels_ok(c, s, g.kts, g.kte) || tile_ok(c, "pbl", g.its, g.ite, g.jts, g.jte)) return 1;     // before any launch
    if (!need(c, ICAR_F_POTENTIAL_TEMPERATURE, "pbl", "potential_temperature")) return 1;
    if (icar_ysu_sfc_run(c, g.dx)) return 1;
    if (icar_ysu_run(c, dt, g.its, g.ite, g.jts, g.jte, g.kts, g.kte)) return 1;
    return ysu_apply_run(c, s, dt);
}

int icar_ysu_copy(icar_hip_ctx *c, int which, void *host, size_t n, bool to_device)
{
    const char *who = to_device ? "ysu_upload" : "ysu_download";
    YsuState *s = state(c, who);
    if (!s) return 1;
    if (which < 0 || which >= ICAR_YSU_N) { icar_set_error(std::string(who) + ": `which` is one of ICAR_YSU_*"); return 1; }
    if (n != count(c, which)) {
        char b[200]; snprintf(b, sizeof b, "%s: array %d holds %zu values, not %zu", who, which, count(c, which), n);
        icar_set_error(b); return 1;
    }
    const size_t bytes = n * sizeof(float);
    if (to_device) HIPCHK(hipMemcpyAsync(s->arr[which], host, bytes, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(hipMemcpyAsync(host, s->arr[which], bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
