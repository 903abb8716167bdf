// tests/support/mpdata_probe.hip -- TEST INFRASTRUCTURE, NOT PRODUCT (built into tests/support/libicar_probe.so).
// The fused MPDATA kernel (icar_amd/csrc/mpdata.hip) never writes the field after its donor-cell pass (q2) to memory, and q2 has to
// be bit-identical to the reference's: next to the ring the flux limiter turns one ulp of q2 into a whole antidiffusive flux
// (adv_mpdata_FCT_core.f90:80-113 with fin = fout = 0).  With the nine antidiffusive coefficient arrays of the context zeroed every
// pseudo-velocity is zero, every corrective flux is zero, and the kernel's output IS q2: tests/test_gpu_advect.py compares that with
// the oracle's donor-cell pass bit for bit.
//
// icar_probe_mpdata_geometry: the launch layout icar_mpdata_fused_run() chooses for a tile and a scalar count, and the march schedule
// of each of its y chunks, from the product's own header (icar_amd/csrc/mpdata_geometry.h).  Host code only, no device needed.
#include <hip/hip_runtime.h>
#include "ctx.h"
#include "mpdata_geometry.h"

// out[0..7] = ntile, nkr, kstore, kb, nw, nchunk, clen, exact; then 7 ints per chunk: ja, jb, P0, s0, s1, npair, generic tail steps.
// The caller provides 8 + 7 * max(1, (ny - 2) / 16 + 1) ints (the chunk count never exceeds max(1, rows / 16)).
extern "C" int icar_probe_mpdata_geometry(int nx, int nz, int ny, int nv, int *out)
{
    if (!out || nx < 3 || ny < 3 || nz < 1 || nv < 1) return 1;
    const MpLayout L = mpdata_layout(nx, nz, ny, nv);
    if (L.nchunk > std::max(1, (ny - 2) / 16 + 1)) return 2;
    const int head[8] = {L.ntile, L.nkr, L.kstore, L.kb, L.nw, L.nchunk, L.clen, L.exact ? 1 : 0};
    for (int t = 0; t < 8; ++t) out[t] = head[t];
    for (int ch = 0; ch < L.nchunk; ++ch) {
        int ja, jb;
        mpdata_chunk_rows(ny, L.clen, ch, ja, jb);
        const MpMarch M = mpdata_march(ny, ja, jb);
        const int v[7] = {M.ja, M.jb, M.P0, M.s0, M.s1, M.npair, M.ntail};
        for (int t = 0; t < 7; ++t) out[8 + 7 * ch + t] = v[t];
    }
    return 0;
}

extern "C" int icar_probe_mpdata_zero_antidiffusion(void *ctx)
{
    icar_hip_ctx *c = (icar_hip_ctx *)ctx;
    if (!c || !c->mpc) return 1;
    static_assert(MPC_CWV == 8 && MPC_GH == 9, "the antidiffusive coefficients are arrays 0..8 of icar_hip_ctx::mpc");
    if (hipSetDevice(c->device) != hipSuccess) return 2;
    if (hipMemsetAsync(c->mpc, 0, c->n3 * sizeof(float) * MPC_GH, c->stream) != hipSuccess) return 2;
    return hipStreamSynchronize(c->stream) == hipSuccess ? 0 : 2;
}
