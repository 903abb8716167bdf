// icar_amd/csrc/mpdata_geometry.h -- the launch layout of the fused MPDATA kernel (mpdata.hip) as a function of the tile's shape and
// the number of scalars, and the march schedule of one y chunk.  Host code only: icar_mpdata_fused_run() calls mpdata_layout(), and
// the tests read both functions through tests/support/mpdata_probe.hip, so that what they say about tiles, chunks and march classes
// is what the product launches.
#pragma once
#include <algorithm>
#include <cmath>

#define MP_HL 3                       // halo lanes per side
#define MP_XOUT (64 - 2 * MP_HL)      // outputs per 64-lane tile
#define MP_NW 8                       // waves per block at most: two per SIMD, ~250 VGPRs each (12 x 3 levels at three per SIMD: no faster, profiles/r05_steps.md)
#define MP_KB 5                       // levels per thread at most
#define MP_ZH 2                       // halo levels of a level range: a fake edge corrupts the outputs of the 2 levels next to it

struct MpLayout {
    int ntile;          // x tiles of MP_XOUT outputs
    int nkr, kstore;    // level ranges and the levels each of them stores
    int kb, nw;         // levels per thread (the kernel's KB) and waves per block
    int nchunk, clen;   // y chunks and the rows of each (the last one takes what is left)
    bool exact;         // the waves hold exactly the column (the kernel's EXACT)
};

// the layout of one corrective iteration over an nx x nz x ny tile (nx, ny >= 3) and nv scalars
inline MpLayout mpdata_layout(int nx, int nz, int ny, int nv)
{
    MpLayout L;
    L.ntile = std::max(1, (nx - 2 + MP_XOUT - 1) / MP_XOUT);
    // levels: one block holds at most MP_NW x MP_KB = 40; taller columns are cut into level ranges with MP_ZH halo levels.  Every
    // range's block computes its kstore levels and MP_ZH halo levels on either side, so it is those kstore + 2 MP_ZH that must fit
    // (counting the halos once per cut let nz = 73..76, 109..112, ... through with 6 levels per thread: no such kernel)
    const int cap_lv = MP_NW * MP_KB;
    int nkr = 1;
    while ((nz + nkr - 1) / nkr + (nkr > 1 ? 2 * MP_ZH : 0) > cap_lv) ++nkr;
    const int kstore = (nz + nkr - 1) / nkr;
    const int blk_lv = std::min(nz, kstore + (nkr > 1 ? 2 * MP_ZH : 0));       // levels a block computes
    const int kb = (blk_lv + MP_NW - 1) / MP_NW, nw = (blk_lv + kb - 1) / kb;
    // y chunks: a block keeps a whole CU, so the work items (tiles x chunks x ranges x scalars) should fill a whole number of
    // rounds of the 256 CUs; each chunk pays ~3.5 warm-up planes.  Pick the chunk count with the best product of the two.
    const int rows = ny - 2, per = L.ntile * nkr * nv;
    int nchunk = 1; double best = -1.0;
    for (int n = 1; n <= std::max(1, rows / 16); ++n) {
        const int cl = (rows + n - 1) / n, nn = (rows + cl - 1) / cl;
        const double items = (double)per * nn, rounds = std::ceil(items / 256.0);
        const double eff = items / (256.0 * rounds) * cl / (cl + 3.5);
        if (eff > best + 1e-9) { best = eff; nchunk = nn; }
    }
    const int clen = (rows + nchunk - 1) / nchunk;
    nchunk = (rows + clen - 1) / clen;
    L.nkr = nkr; L.kstore = kstore; L.kb = kb; L.nw = nw; L.nchunk = nchunk; L.clen = clen;
    L.exact = (nkr == 1) && (kb * nw == nz);          // the waves hold exactly the column: no per-slot level tests
    return L;
}

// The march of one y chunk, rows ja .. jb of a tile of ny rows: generic steps P0 .. s0-1 (warm-up), steady steps s0 .. s0+2 npair-1
// in pairs, then ntail generic steps up to jb+1.  A RESTATEMENT for the host of what k_mpdata_fused computes for itself -- `P0 = ja - 3`
// above its rolling state and the three lines `s0 = ja + 1, s1 = ...`, `npair = ..., s1p = ...`, `lo = ..., hi = ...` at the head
// of its march loop: the kernel keeps its own lines (it has no register to spare, tests/test_kernel_resources.py), and whoever
// changes them changes these.
struct MpMarch { int ja, jb, P0, s0, s1, npair, ntail; };
inline void mpdata_chunk_rows(int ny, int clen, int chunk, int &ja, int &jb) { ja = 1 + chunk * clen; jb = std::min(ja + clen - 1, ny - 2); }
inline MpMarch mpdata_march(int ny, int ja, int jb)
{
    MpMarch M;
    M.ja = ja; M.jb = jb;
    M.P0 = ja - 3;
    M.s0 = ja + 1; M.s1 = std::max(std::min(jb + 1, ny - 4), M.s0 - 1);
    M.npair = (M.s1 - M.s0 + 1) / 2;
    const int s1p = M.s0 + 2 * M.npair - 1;
    M.ntail = jb + 1 - s1p;                   // generic steps s1p+1 .. jb+1
    return M;
}
