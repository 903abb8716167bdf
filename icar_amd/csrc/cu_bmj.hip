// icar_amd/csrc/cu_bmj.hip -- the convection slot (row C1) on gfx950: convect(domain, options, dt) as it runs for convection = kCU_BMJ
// (and, around the schemes of cu_tiedtke.hip and cu_nsas.hip, for convection = kCU_TIEDTKE and kCU_NSAS: the zeroing and the tendency loop are shared).
//
// Reference algorithm: src/physics/cu_driver.f90 -- init_convection :97-253 (XLAND :139-140, lowlyr = 1, bmj_rad_feedback, the call of
// BMJINIT :230-243), convect :255-514 (the zeroing :272-282, the call of BMJDRV :434-465 on its..ite, jts..jte, kts..kte-1, the
// tendencies and the two precipitation sums :483-500); src/physics/cu_bmj.f90 -- the column code, restated in bmj_column.h (which
// also says what of it is not built: the radiation-feedback cloud arrays).  W0AVG (:286-298) is read by no branch of BMJ and is not
// made; stochastic_cu /= kNO_STOCHASTIC draws from random_number and is refused.
//
//   k_cu_zero    one thread per (i, j) of ims..ime, jts..jte marching k over the whole column: tend%th = tend%qv = 0, RAINCV = 0
//                (tend%qs, %qr, %u, %v stay zero and are not materialised; tend%qc and %qi likewise with BMJ -- with Tiedtke,
//                cu_tiedtke.hip, they exist and are zeroed here and applied by k_cu_apply like the other two)
//   k_cu_load, k_cu_search, k_cu_bmj, k_cu_store
//                ONE THREAD PER COLUMN of its..ite, lanes along i: the flipped column into the workspace (a streaming kernel), the
//                buoyancy search and then the adjustment on the workspace, the two tendencies out of it (streaming) -- four launches, so that the scheme's kernels
//                carry none of the fields' pointers through their control flow (as one kernel it spilled scalar registers).  The ~35 level arrays of the scheme (16 of them stored, see
//                bmj_column.h) live in a device workspace laid out [array][level][column], so that every access of a wave is one
//                coalesced line and nothing of a column sits in scratch; the column scalars are registers.  The tile is walked in
//                chunks of rows that fit the workspace.  Nine columns in ten leave after the buoyancy search and have touched
//                only the inputs and the search's four arrays.
//   k_cu_apply   one thread per (i, j) of ims..ime, jts..jte marching k: x = x + (tend dt) fraction for water_vapor,
//                potential_temperature and -- with tend = 0: the identity except that -0.0 becomes +0.0 -- cloud water and cloud ice
//                (stored only where the bits change), then accumulated_precipitation (REAL(8)) and accumulated_convective_pcp
//                += RAINCV.
// The tables of BMJINIT are built once on the host by the same header (the C library's expf / powf, which glibc_flt32.h restates
// for the device) when the slot is configured, and kept in device memory.  REAL(4) throughout in the reference's operation order:
// no contraction, IEEE division.  A wave per column (lane = level) is the obvious later form for <= 64 levels; it is not this one.
//
// Levels: BMJDRV flips with KFLIP = KTE+1-K, which maps K = KTS..KTE onto KTS..KTE only for KTS = 1, and takes PSFC from
// PINT(i,1,j): kts /= 1 is refused (with kts = 2 the reference reads DTDT(1) below the array's lower bound, cu_bmj.f90:248).
// kte - kts >= 2 (three levels; with one scheme level the reference reads PRSMID(LBOT+1) = PRSMID(2) past the column, :755) and
// kte - kts <= BMJ_MAX_LEVELS.
#include "ctx.h"
#include "glibc_flt32.h"
#include <cmath>
#include <cstdio>
#include <vector>

#define BMJ_FN __host__ __device__ static __forceinline__
#ifdef __HIP_DEVICE_COMPILE__
#define BMJ_EXPF gf_expf
#define BMJ_POWF gf_powf
#else
#define BMJ_EXPF expf
#define BMJ_POWF powf
#endif
#define BMJ_HOST_EXPF expf
#define BMJ_HOST_POWF powf
#define BMJ_WITH_TABLES
#include "bmj_column.h"

#include "cu_state.h"

namespace {
constexpr size_t kWsColumns = (size_t)1 << 16;       // columns per launch of k_cu_bmj (a tile row always fits)

struct CuArgs {                           // the fields of k_cu_load / k_cu_store
    Dims d;
    int i0, nxt, j0, k0, n;              // first column / row (0-based), columns per row, first level, scheme levels
    size_t stride;
    const float *t, *qv, *pmid, *pi, *rho, *dz, *cutop, *cubot;
    float *tend_th, *tend_qv, *ws;
};

struct ColArgs {                          // k_cu_bmj: the workspace, the tables and the column's scalars
    int nx, i0, nxt, j0, n;
    float dt;
    size_t stride, psfc_at;              // psfc_at: offset of (0, kts, 0) in pressure_interface, sj: its row stride
    int sj;
    const float *tables, *pint;
    const int *land_mask;
    float *cldefi, *raincv, *cutop, *cubot, *ws;
    float *found;                        // BmjSearch of every column of the launch: 7 arrays of `stride` values
};

__device__ __forceinline__ BmjCol column_of(const CuArgs &a, int i, int j)
{
    const size_t at = (size_t)a.d.idx(i, a.k0, j);
    return {a.t + at, a.qv + at, a.pmid + at, nullptr, a.pi + at, a.rho + at, a.dz + at, a.tend_th + at, a.tend_qv + at};
}

// BMJDRV :206-216: the flipped column into the workspace
__global__ void __launch_bounds__(64)
k_cu_load(CuArgs a)
{
    const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y;
    if (ii >= a.nxt) return;
    bmj_col_load(column_of(a, a.i0 + ii, a.j0 + jj), (size_t)a.d.sk, a.n, a.ws + ((size_t)jj * a.nxt + ii), a.stride);
}

// BMJ :496-882 on the workspace: the buoyancy search
__global__ void __launch_bounds__(64)
k_cu_search(ColArgs a)
{
    const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y;
    if (ii >= a.nxt) return;
    const size_t col = (size_t)jj * a.nxt + ii;
    const BmjTables tb = bmj_tables_at(a.tables);
    const BmjSearch f = bmj_search(a.ws + col, a.stride, a.n, a.n, &tb);
    float *o = a.found + col;
    o[0] = f.psp; o[a.stride] = f.thbt; o[2 * a.stride] = f.thesp;
    int *oi = (int *)o;
    oi[3 * a.stride] = f.lbot; oi[4 * a.stride] = f.ltop; oi[5 * a.stride] = f.pair; oi[6 * a.stride] = f.found;
}

// BMJ :888-1739 on the workspace: the quick exit (nine columns in ten), deep and shallow convection
__global__ void __launch_bounds__(64)
k_cu_bmj(ColArgs a)
{
    const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y;
    if (ii >= a.nxt) return;
    const size_t col = (size_t)jj * a.nxt + ii;
    BmjSearch f;
    {
        const float *o = a.found + col;
        const int *oi = (const int *)o;
        f.psp = o[0]; f.thbt = o[a.stride]; f.thesp = o[2 * a.stride];
        f.lbot = oi[3 * a.stride]; f.ltop = oi[4 * a.stride]; f.pair = oi[5 * a.stride]; f.found = oi[6 * a.stride];
    }
    const int i = a.i0 + ii, j = a.j0 + jj;
    const size_t c2 = (size_t)a.nx * j + i;
    const int lm = a.land_mask ? a.land_mask[c2] : 1;
    const float xland = lm == 0 ? 2.0f : (float)lm;                                                   // cu_driver.f90:139-140
    const float psfc = a.pint[a.psfc_at + (size_t)a.sj * j + i];                                      // PINT(i,1,j), cu_bmj.f90:195
    // the four result addresses are formed now and pinned to vector registers: as wave-uniform pointers they would sit in
    // scalar registers across the whole scheme, whose nested divergent control flow needs those for its exec masks
    float *pc = a.cldefi + c2, *pr = a.raincv + c2, *pt = a.cutop + c2, *pb = a.cubot + c2;
    size_t stride = a.stride;                 // (likewise the workspace's column count)
    asm volatile("" : "+v"(pc), "+v"(pr), "+v"(pt), "+v"(pb), "+v"(stride));
    float cld = *pc, rain, top, bot;
    const BmjTables tb = bmj_tables_at(a.tables);
    bmj_col_adjust(a.n, a.dt, xland, psfc, &cld, &rain, &top, &bot, a.ws + col, stride, &tb, f);
    *pc = cld; *pr = rain; *pt = top; *pb = bot;
}

// BMJDRV :246-253: the tendencies of the column from the workspace
__global__ void __launch_bounds__(64)
k_cu_store(CuArgs a)
{
    const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y;
    if (ii >= a.nxt) return;
    const int i = a.i0 + ii, j = a.j0 + jj;
    const size_t c2 = (size_t)a.d.nx * j + i;
    bmj_col_store(column_of(a, i, j), (size_t)a.d.sk, a.n, a.cutop[c2], a.cubot[c2], a.ws + ((size_t)jj * a.nxt + ii), a.stride);
}

// cu_driver.f90:272-282 on the rows j0 .. j0+gridDim.y-1
__global__ void __launch_bounds__(64)
k_cu_zero(Dims d, int j0, float *__restrict__ tend_th, float *__restrict__ tend_qv, float *__restrict__ raincv, float *__restrict__ tend_qc,
          float *__restrict__ tend_qi)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = j0 + blockIdx.y;
    if (i >= d.nx) return;
    raincv[(size_t)d.nx * j + i] = 0.0f;
    size_t at = (size_t)d.idx(i, 0, j);
    if (tend_qc) {                                                        // Tiedtke: tend%qc and tend%qi exist
        for (int k = 0; k < d.nz; ++k, at += d.sk) { tend_th[at] = 0.0f; tend_qv[at] = 0.0f; tend_qc[at] = 0.0f; tend_qi[at] = 0.0f; }
        return;
    }
    for (int k = 0; k < d.nz; ++k, at += d.sk) { tend_th[at] = 0.0f; tend_qv[at] = 0.0f; }
}

struct ApplyArgs {
    Dims d;
    int j0;
    float dt, f_qv, f_qc, f_th, f_qi;    // a fraction <= 0 (or tendency_fraction <= 0): that field is left alone
    float *qv, *qc, *th, *qi;
    const float *tend_qv, *tend_th, *raincv;
    const float *tend_qc, *tend_qi;      // null with BMJ, which leaves them at 0
    double *acc;
    float *acc_conv;
};

__device__ __forceinline__ void add_zero(float *p, size_t at, float dt, float f)
{
    const float x = p[at], y = x + 0.0f * dt * f;
    if (__builtin_bit_cast(int, y) != __builtin_bit_cast(int, x)) p[at] = y;
}

// cu_driver.f90:483-500 on the rows j0 .. j0+gridDim.y-1
__global__ void __launch_bounds__(64)
k_cu_apply(ApplyArgs a)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = a.j0 + blockIdx.y;
    if (i >= a.d.nx) return;
    size_t at = (size_t)a.d.idx(i, 0, j);
    if (a.tend_qc) {                                                                                  // Tiedtke: all four tendencies
        for (int k = 0; k < a.d.nz; ++k, at += a.d.sk) {
            if (a.f_qv > 0) a.qv[at] = a.qv[at] + a.tend_qv[at] * a.dt * a.f_qv;                      // :489
            if (a.f_qc > 0) a.qc[at] = a.qc[at] + a.tend_qc[at] * a.dt * a.f_qc;                      // :490
            if (a.f_th > 0) a.th[at] = a.th[at] + a.tend_th[at] * a.dt * a.f_th;                      // :491
            if (a.f_qi > 0) a.qi[at] = a.qi[at] + a.tend_qi[at] * a.dt * a.f_qi;                      // :492
        }
    } else
    for (int k = 0; k < a.d.nz; ++k, at += a.d.sk) {
        if (a.f_qv > 0) a.qv[at] = a.qv[at] + a.tend_qv[at] * a.dt * a.f_qv;                          // :489
        if (a.f_qc > 0) add_zero(a.qc, at, a.dt, a.f_qc);                                             // :490, tend%qc == 0
        if (a.f_th > 0) a.th[at] = a.th[at] + a.tend_th[at] * a.dt * a.f_th;                          // :491
        if (a.f_qi > 0) add_zero(a.qi, at, a.dt, a.f_qi);                                             // :492, tend%qi == 0
    }
    const size_t c2 = (size_t)a.d.nx * j + i;
    const float r = a.raincv[c2];
    a.acc[c2] = a.acc[c2] + (double)r;                                                                // :499
    a.acc_conv[c2] = a.acc_conv[c2] + r;                                                              // :500
}

__global__ void k_cu_fill(float *p, size_t n, float v) { const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; if (t < n) p[t] = v; }

bool is3d(int which) { return which == ICAR_CU_TEND_TH || which == ICAR_CU_TEND_QV; }
size_t count(const icar_hip_ctx *c, int which) { return is3d(which) ? c->n3 : (size_t)c->d.nx * c->d.ny; }

float *need(icar_hip_ctx *c, int f, const char *who, const char *member)
{
    if (c->field[f]) return (float *)c->field[f];
    char b[200]; snprintf(b, sizeof b, "%s: domain%%%s (field %d) is not on the device", who, member, f);
    icar_set_error(b);
    return nullptr;
}

CuState *state(icar_hip_ctx *c, const char *who)
{
    if (c->cu) return c->cu;
    icar_set_error(std::string(who) + ": the convection slot is not configured (icar_hip_cu_configure with convection = 5, icar_hip_cu_init or icar_hip_convection_init)");
    return nullptr;
}

int fill(icar_hip_ctx *c, float *p, size_t n, float v)
{
    hipLaunchKernelGGL(k_cu_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, p, n, v);
    HIPCHK(hipGetLastError());
    return 0;
}

// kts..kte of the call: the levels the scheme can run on (see the header)
int levels_ok(icar_hip_ctx *c, const CuState *s, int kts, int kte)
{
    char b[320];
    if (kts < c->kms || kte > c->kme) { icar_set_error("cu_bmj: kts..kte outside the levels of the context"); return 1; }
    if (kts != 1) {
        snprintf(b, sizeof b, "cu_bmj: kts = %d: BMJDRV flips with KFLIP = KTE+1-K, which maps K = KTS..KTE onto KTS..KTE only for KTS = 1 (with kts = 2 "
                 "the reference reads DTDT(KTE+1-K) = DTDT(1) below the array's lower bound, cu_bmj.f90:248)", kts);
        icar_set_error(b); return 1;
    }
    const int n = kte - kts;
    if (n < 2) {
        snprintf(b, sizeof b, "cu_bmj: %d levels (kts..kte): at least 3.  BMJ runs on kts..kte-1; with one level LBOT = LMH = 1 and the reference reads "
                 "PRSMID(LBOT+1) = PRSMID(2) past the column (cu_bmj.f90:755)", kte - kts + 1);
        icar_set_error(b); return 1;
    }
    if (n > BMJ_MAX_LEVELS || n > s->ws_levels) {
        snprintf(b, sizeof b, "cu_bmj: %d levels (kts..kte): at most %d (the column workspace is sized for kte - kts <= %d)", kte - kts + 1,
                 BMJ_MAX_LEVELS + 1, BMJ_MAX_LEVELS);
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

void icar_cu_free(icar_hip_ctx *c)
{
    CuState *s = c->cu;
    if (!s) return;
    for (float *p : s->arr) if (p) hipFree(p);
    if (s->tables) hipFree(s->tables);
    if (s->ws) hipFree(s->ws);
    if (s->found) hipFree(s->found);
    icar_tiedtke_free(s);
    icar_nsas_free(s);
    delete s;
    c->cu = nullptr;
}

// init_convection (cu_driver.f90:97-253) for kCU_BMJ: the slot's arrays, BMJINIT's tables, the column workspace
// the slot's own arrays (ICAR_CU_*), shared by both schemes
int icar_cu_common_init(icar_hip_ctx *c)
{
    if (c->cu) return 0;
    CuState *s = new CuState();
    c->cu = s;
    for (int w = 0; w < ICAR_CU_N; ++w) {
        const size_t bytes = count(c, w) * sizeof(float);
        HIPCHK(hipMalloc(&s->arr[w], bytes));
        HIPCHK(hipMemsetAsync(s->arr[w], 0, bytes, c->stream));
    }
    return fill(c, s->arr[ICAR_CU_CLDEFI], count(c, ICAR_CU_CLDEFI), BMJ_AVGEFI);                     // BMJINIT :1880-1884
}

int icar_cu_init_device(icar_hip_ctx *c)
{
    if (c->cu && c->cu->tables) return 0;
    if (icar_cu_common_init(c)) return 1;
    CuState *s = c->cu;
    std::vector<float> block(BMJ_TABLE_FLOATS);
    BmjTables h;
    bmj_build_tables(block.data(), &h);
    HIPCHK(hipMalloc(&s->tables, sizeof(float) * BMJ_TABLE_FLOATS));
    HIPCHK(hipMemcpyAsync(s->tables, block.data(), sizeof(float) * BMJ_TABLE_FLOATS, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t n2 = (size_t)c->d.nx * c->d.ny;
    s->ws_cols = n2 < kWsColumns ? n2 : kWsColumns;
    if (s->ws_cols < (size_t)c->d.nx) s->ws_cols = c->d.nx;
    s->ws_levels = c->d.nz - 1 < BMJ_MAX_LEVELS ? c->d.nz - 1 : BMJ_MAX_LEVELS;
    if (s->ws_levels < 1) s->ws_levels = 1;
    HIPCHK(hipMalloc(&s->ws, sizeof(float) * BMJ_NARR * (size_t)s->ws_levels * s->ws_cols));
    HIPCHK(hipMalloc(&s->found, sizeof(float) * 7 * s->ws_cols));
    return 0;
}

// BMJDRV on its..ite, jts..jte, kts..kte-1 (cu_driver.f90:434-465)
int icar_cu_bmj_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte)
{
    static const char *who = "cu_bmj";
    CuState *s = state(c, who);
    if (s && !s->tables) { icar_set_error("cu_bmj: BMJ is not configured (icar_hip_cu_configure with convection = 5)"); return 1; }
    if (!s || levels_ok(c, s, kts, kte) || tile_ok(c, who, its, ite, jts, jte)) return 1;
    if (ite < its || jte < jts) return 0;
    CuArgs a;
    ColArgs q;
    a.t = need(c, ICAR_F_TEMPERATURE, who, "temperature"); a.qv = need(c, ICAR_F_WATER_VAPOR, who, "water_vapor");
    a.pmid = need(c, ICAR_F_PRESSURE, who, "pressure"); q.pint = need(c, ICAR_F_PRESSURE_INTERFACE, who, "pressure_interface");
    a.pi = need(c, ICAR_F_EXNER, who, "exner"); a.rho = need(c, ICAR_F_DENSITY, who, "density");
    a.dz = need(c, ICAR_F_DZ_INTERFACE, who, "dz_interface");
    if (!a.t || !a.qv || !a.pmid || !q.pint || !a.pi || !a.rho || !a.dz) return 1;
    q.land_mask = (const int *)c->field[ICAR_F_LAND_MASK];            // never uploaded = all land, as in pbl_simple
    a.d = c->d; a.i0 = its - c->ims; a.nxt = ite - its + 1; a.k0 = kts - c->kms; a.n = kte - kts;
    a.ws = s->ws; a.cutop = s->arr[ICAR_CU_CUTOP]; a.cubot = s->arr[ICAR_CU_CUBOT];
    a.tend_th = s->arr[ICAR_CU_TEND_TH]; a.tend_qv = s->arr[ICAR_CU_TEND_QV];
    const int rows_per = (int)(s->ws_cols / (size_t)a.nxt);          // >= 1: ws_cols >= nx
    // [array][level][column] with the column count of one launch: (array n + level) stride + column < BMJ_NARR ws_levels ws_cols
    a.stride = (size_t)rows_per * a.nxt;
    q.nx = c->d.nx; q.i0 = a.i0; q.nxt = a.nxt; q.n = a.n; q.dt = dt; q.stride = a.stride; q.tables = s->tables; q.ws = s->ws; q.found = s->found;
    q.psfc_at = (size_t)c->d.idx(0, a.k0, 0); q.sj = c->d.sj;
    q.cldefi = s->arr[ICAR_CU_CLDEFI]; q.raincv = s->arr[ICAR_CU_RAINCV]; q.cutop = s->arr[ICAR_CU_CUTOP]; q.cubot = s->arr[ICAR_CU_CUBOT];
    ScopedTimer timer(c, "cu_bmj");
    for (int j = jts; j <= jte; j += rows_per) {
        const int rows = jte - j + 1 < rows_per ? jte - j + 1 : rows_per;
        const dim3 grid((a.nxt + 63) / 64, rows), block(64);
        a.j0 = q.j0 = j - c->jms;
        hipLaunchKernelGGL(k_cu_load, grid, block, 0, c->stream, a);
        hipLaunchKernelGGL(k_cu_search, grid, block, 0, c->stream, q);
        hipLaunchKernelGGL(k_cu_bmj, grid, block, 0, c->stream, q);
        hipLaunchKernelGGL(k_cu_store, grid, block, 0, c->stream, a);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// convect(domain, options, dt) (cu_driver.f90:255-514) on the tile of icar_hip_step_configure
int icar_convect_run(icar_hip_ctx *c, float dt)
{
    static const char *who = "convect";
    IcarStepState &st = c->step;
    if (st.convection == 0) return 0;                                 // :264
    CuState *s = state(c, who);
    if (!s) return 1;
    const icar_hip_step_config &g = st.cfg;
    const bool tdk = st.convection == ICAR_CU_TIEDTKE, nsas = st.convection == ICAR_CU_NSAS;
    float *const tend_qc = tdk ? s->tdk[ICAR_TIEDTKE_TEND_QC] : nsas ? s->nsas[ICAR_NSAS_TEND_QC] : nullptr;
    float *const tend_qi = tdk ? s->tdk[ICAR_TIEDTKE_TEND_QI] : nsas ? s->nsas[ICAR_NSAS_TEND_QI] : nullptr;
    if ((tdk ? icar_tiedtke_levels_ok(c, g.kts, g.kte) : nsas ? icar_nsas_levels_ok(c, g.kts, g.kte) : levels_ok(c, s, g.kts, g.kte)) || tile_ok(c, who, g.its, g.ite, g.jts, g.jte)) return 1;
    if (g.jte < g.jts) return 0;
    ApplyArgs a;
    const bool on = st.cu_tendency_fraction > 0;                      // :484
    a.f_qv = on ? st.cu_tend_qv_fraction : 0.0f; a.f_qc = on ? st.cu_tend_qc_fraction : 0.0f;
    a.f_th = on ? st.cu_tend_th_fraction : 0.0f; a.f_qi = on ? st.cu_tend_qi_fraction : 0.0f;
    a.qv = a.f_qv > 0 ? need(c, ICAR_F_WATER_VAPOR, who, "water_vapor") : nullptr;
    a.qc = a.f_qc > 0 ? need(c, ICAR_F_CLOUD_WATER, who, "cloud_water_mass") : nullptr;
    a.th = a.f_th > 0 ? need(c, ICAR_F_POTENTIAL_TEMPERATURE, who, "potential_temperature") : nullptr;
    a.qi = a.f_qi > 0 ? need(c, ICAR_F_CLOUD_ICE, who, "cloud_ice_mass") : nullptr;
    if ((a.f_qv > 0 && !a.qv) || (a.f_qc > 0 && !a.qc) || (a.f_th > 0 && !a.th) || (a.f_qi > 0 && !a.qi)) return 1;
    a.acc = (double *)icar_field_f(c, ICAR_F_PRECIPITATION, false);
    if (!a.acc) return 1;
    const dim3 grid((c->d.nx + 63) / 64, g.jte - g.jts + 1), block(64);
    {
        ScopedTimer timer(c, "cu_stream");
        hipLaunchKernelGGL(k_cu_zero, grid, block, 0, c->stream, c->d, g.jts - c->jms, s->arr[ICAR_CU_TEND_TH], s->arr[ICAR_CU_TEND_QV], s->arr[ICAR_CU_RAINCV],
                           tend_qc, tend_qi);
        HIPCHK(hipGetLastError());
    }
    if (tdk ? icar_tiedtke_run(c, dt, g.its, g.ite, g.jts, g.jte, g.kts, g.kte) : nsas ? icar_nsas_run(c, dt, g.its, g.ite, g.jts, g.jte, g.kts, g.kte)
            : icar_cu_bmj_run(c, dt, g.its, g.ite, g.jts, g.jte, g.kts, g.kte)) return 1;
    a.tend_qc = tend_qc; a.tend_qi = tend_qi;
    a.d = c->d; a.j0 = g.jts - c->jms; a.dt = dt;
    a.tend_qv = s->arr[ICAR_CU_TEND_QV]; a.tend_th = s->arr[ICAR_CU_TEND_TH]; a.raincv = s->arr[ICAR_CU_RAINCV];
    a.acc_conv = s->arr[ICAR_CU_ACC_CONV_PCP];
    ScopedTimer timer(c, "cu_stream");
    hipLaunchKernelGGL(k_cu_apply, grid, block, 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

int icar_cu_copy(icar_hip_ctx *c, int which, void *host, bool to_device)
{
    CuState *s = state(c, to_device ? "cu_upload" : "cu_download");
    if (!s) return 1;
    if (which < 0 || which >= ICAR_CU_N) { icar_set_error("cu_upload / cu_download: `which` is one of ICAR_CU_*"); return 1; }
    const size_t bytes = count(c, which) * sizeof(float);
    if (to_device) HIPCHK(hipMemcpyAsync(s->arr[which], host, bytes, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(hipMemcpyAsync(host, s->arr[which], bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int icar_cu_reset_run(icar_hip_ctx *c)
{
    CuState *s = state(c, "cu_reset");
    if (!s) return 1;
    if (fill(c, s->arr[ICAR_CU_CLDEFI], count(c, ICAR_CU_CLDEFI), BMJ_AVGEFI)) return 1;
    return fill(c, s->arr[ICAR_CU_ACC_CONV_PCP], count(c, ICAR_CU_ACC_CONV_PCP), 0.0f);
}

int icar_cu_tables_copy(icar_hip_ctx *c, float *out, size_t capacity, size_t *n_out)
{
    if (n_out) *n_out = BMJ_TABLE_FLOATS;
    if (!out) return 0;
    CuState *s = state(c, "cu_tables");
    if (!s) return 1;
    if (!s->tables) { icar_set_error("cu_tables: BMJ is not configured (icar_hip_cu_configure with convection = 5)"); return 1; }
    if (capacity < (size_t)BMJ_TABLE_FLOATS) { icar_set_error("cu_tables: buffer too small"); return 1; }
    HIPCHK(hipMemcpyAsync(out, s->tables, sizeof(float) * BMJ_TABLE_FLOATS, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
