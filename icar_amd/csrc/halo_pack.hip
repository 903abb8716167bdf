// icar_amd/csrc/halo_pack.hip -- row H1: the two packers every message is made of.
//
//   icar_halo_pack_dirs   the halo faces of the exchangeable scalars (exchangeable_obj.f90:248-356), any subset of the four
//                         directions in one launch.  Buffer layout per direction, field after field:
//                         N / S = [h][nz][nx] (verbatim planes), E / W = [ny][nz][h].
//                           put_north sends rows ny-2h..ny-h-1 ; put_south rows h..2h-1          (exchangeable_obj.f90:263,280)
//                           retrieve_north fills rows ny-h..ny-1 ; retrieve_south rows 0..h-1    (:290,:300)
//                           put_east sends cols nx-2h..nx-h-1 ; put_west cols h..2h-1            (:317,:335)
//                           retrieve_east fills cols nx-h..nx-1 ; retrieve_west cols 0..h-1
//                         Corner cells: E / W win over N / S (k_halo_dirs says why); a call without an E / W direction
//                         writes whole rows.
//   icar_box_copy         one box of a field <-> a contiguous buffer [nj][nz][ni]: the staggered faces of exchange_u /
//                         exchange_v (:158-229, planned in comm.hip) and icar_hip_box_pack / _unpack.
#include "ctx.h"
#include <algorithm>

struct HaloArgs { float *f[ICAR_MAX_ADV]; };

// all directions of one halo_send / halo_retrieve in ONE launch (blockIdx.z = direction): a step of an image with four
// neighbours issues 2 launches instead of 8 -- small tiles are host-launch-bound
struct HaloDirs { int n, ns[4], start[4], skip_w, skip_e; float *buf[4]; };
template <bool UNPACK>
__global__ void k_halo_dirs(Dims d, HaloArgs a, int h, HaloDirs hd)
{
    const int z = blockIdx.z, m = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    float *__restrict__ buf = hd.buf[z];
    if (hd.ns[z]) {                                                // N/S: h contiguous rows
        const size_t per = (size_t)d.nx * d.nz * h;
        if (t >= per) return;
        const size_t src = (size_t)hd.start[z] * d.sj + t;
        if (UNPACK) {
            // the corner cells belong to both an N/S row and an E/W column; the reference retrieves N, S, E, W in that
            // order (exchangeable_obj.f90:138-151), so E/W win: with them in the same launch the rows leave the corners alone
            const int i = (int)(t % d.nx);
            if ((hd.skip_w && i < h) || (hd.skip_e && i >= d.nx - h)) return;
            a.f[m][src] = buf[(size_t)m * per + t];
        } else buf[(size_t)m * per + t] = a.f[m][src];
    } else {                                                       // E/W: h columns of every (k, j) line
        const size_t per = (size_t)h * d.nz * d.ny;
        if (t >= per) return;
        const int x = (int)(t % h); const size_t line = t / h;
        const size_t src = line * d.nx + hd.start[z] + x;
        if (UNPACK) a.f[m][src] = buf[(size_t)m * per + t]; else buf[(size_t)m * per + t] = a.f[m][src];
    }
}

int icar_halo_pack_dirs(icar_hip_ctx *c, int ndir, const int *dirs, int h, const int *fields, int n, void *const *bufs, bool unpack)
{
    if (n <= 0 || ndir <= 0) return 0;
    if (ndir > 4) { icar_set_error("halo: at most 4 directions per call"); return 1; }
    if (n > ICAR_MAX_ADV) { icar_set_error("halo: too many fields"); return 1; }
    if (h < 1 || 2 * h > c->d.nx || 2 * h > c->d.ny) { icar_set_error("halo: bad halo width"); return 1; }
    HaloArgs a;
    for (int m = 0; m < n; ++m) {
        if (fields[m] < 0 || fields[m] >= ICAR_N_ADVECTABLE) { icar_set_error("halo: only exchangeable scalars"); return 1; }
        a.f[m] = icar_field_f(c, fields[m]);
        if (!a.f[m]) return 1;
    }
    const Dims &d = c->d;
    HaloDirs hd; hd.n = ndir; hd.skip_w = hd.skip_e = 0;
    size_t permax = 0;
    for (int z = 0; z < ndir; ++z) {
        const int dir = dirs[z];
        if (dir < 0 || dir > 3 || !bufs[z]) { icar_set_error("halo: dir must be 0..3 with a buffer"); return 1; }
        hd.ns[z] = (dir < 2); hd.buf[z] = (float *)bufs[z];
        if (dir == 2) hd.skip_e = 1;
        if (dir == 3) hd.skip_w = 1;
        // put sends the h rows / columns next to the halo, retrieve fills the outermost h (the header's table)
        if (dir < 2) hd.start[z] = !unpack ? (dir == 0 ? d.ny - 2 * h : h) : (dir == 0 ? d.ny - h : 0);
        else         hd.start[z] = !unpack ? (dir == 2 ? d.nx - 2 * h : h) : (dir == 2 ? d.nx - h : 0);
        permax = std::max(permax, dir < 2 ? (size_t)d.nx * d.nz * h : (size_t)h * d.nz * d.ny);
    }
    ScopedTimer t(c, "halo");
    dim3 g((unsigned)((permax + 255) / 256), n, ndir), b(256);
    if (unpack) hipLaunchKernelGGL(k_halo_dirs<true>, g, b, 0, c->stream, d, a, h, hd);
    else        hipLaunchKernelGGL(k_halo_dirs<false>, g, b, 0, c->stream, d, a, h, hd);
    HIPCHK(hipGetLastError());
    return 0;
}

namespace {
// box <-> contiguous buffer [nj][nz][ni]
template <bool UNPACK>
__global__ void k_box(int X, int nz, int i0, int ni, int j0, int nj, float *__restrict__ f, float *__restrict__ buf)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y, jj = blockIdx.z;
    if (t >= ni) return;
    const size_t a = (size_t)(i0 + t) + (size_t)X * (k + (size_t)nz * (j0 + jj));
    const size_t b = (size_t)t + (size_t)ni * (k + (size_t)nz * jj);
    if (UNPACK) f[a] = buf[b]; else buf[b] = f[a];
}
}  // namespace

int icar_box_copy(icar_hip_ctx *c, int field, int which, int i0, int ni, int j0, int nj, float *buf, bool unpack)
{
    if (field < 0 || field >= ICAR_N_FIELD_SLOTS || icar_hip_field_elem_size(field) != 4) { icar_set_error("box: REAL(4) fields only"); return 1; }
    const int nx = c->d.nx, nz = c->d.nz, ny = c->d.ny;
    if (icar_field_count(c, field) < (size_t)nx * nz * ny) { icar_set_error("box: 3-D fields only"); return 1; }
    const int X = (field == ICAR_F_U || field == ICAR_F_JACOBIAN_U || field == ICAR_F_DZDX || field == ICAR_F_ZR_U) ? nx + 1 : nx;
    const int Y = (field == ICAR_F_V || field == ICAR_F_JACOBIAN_V || field == ICAR_F_DZDY || field == ICAR_F_ZR_V) ? ny + 1 : ny;
    if (i0 < 0 || ni < 1 || i0 + ni > X || j0 < 0 || nj < 1 || j0 + nj > Y) { icar_set_error("box: range outside the field"); return 1; }
    float *f = which ? c->dqdt[field] : icar_field_f(c, field);
    if (!f) { if (which) icar_set_error("box: dqdt_3d of this field is not on the device"); return 1; }
    ScopedTimer t(c, "halo");
    const dim3 g((ni + 63) / 64, nz, nj), b(64);
    if (unpack) hipLaunchKernelGGL(k_box<true>, g, b, 0, c->stream, X, nz, i0, ni, j0, nj, f, buf);
    else        hipLaunchKernelGGL(k_box<false>, g, b, 0, c->stream, X, nz, i0, ni, j0, nj, f, buf);
    HIPCHK(hipGetLastError());
    return 0;
}
