// icar_amd/csrc/cu_state.h -- what the convection slot keeps on the device, shared by cu_bmj.hip (the slot's driver and BMJ) and
// cu_tiedtke.hip (the Tiedtke scheme) and cu_nsas.hip (the NSAS scheme).
#pragma once
#include "ctx.h"

struct CuState {
    float *arr[ICAR_CU_N] = {nullptr};
    float *tables = nullptr;             // BMJ_TABLE_FLOATS (null until convection = 5 is configured)
    float *ws = nullptr;                 // BMJ_NARR x ws_levels x ws_cols
    float *found = nullptr;              // 7 x ws_cols: what the search hands to the adjustment (BmjSearch)
    size_t ws_cols = 0;
    int ws_levels = 0;
    // Tiedtke (null until icar_hip_cu_init with convection = 1)
    float *tdk[ICAR_TIEDTKE_N] = {nullptr};   // tend%qc, tend%qi (nx,nz,ny), PRATEC (nx,ny), KTYPE (nx,ny) INTEGER(4)
    float *tdk_znu = nullptr;            // znu(kms:kme)
    float *tdk_ws = nullptr;             // TDK_NARR x tdk_levels x tdk_cols
    float *tdk_col = nullptr;            // TDK_NCOL x tdk_cols: the scalars a column carries between the launches
    int *tdk_leveltop = nullptr;         // ny: the row's leveltop
    size_t tdk_cols = 0;
    int tdk_levels = 0;                  // levels of the workspace (scheme levels + 2)
    // NSAS (null until icar_hip_convection_init with convection = 4)
    float *nsas[ICAR_NSAS_N] = {nullptr};     // tend%qc, tend%qi (nx,nz,ny), PRATEC, HBOT, HTOP, hpbl (nx,ny)
    float *nsas_ws = nullptr;            // NSAS_NARR x nsas_levels x nsas_cols
    float *nsas_col = nullptr;           // NSAS_NCOL x nsas_cols: what a column carries from nsas2d to nscv2d
    int *nsas_limits = nullptr;          // 3 x ny: the row's kbmax, kbm, kmax
    size_t nsas_cols = 0;
    int nsas_levels = 0;                 // levels of the workspace (scheme levels + 2)
    float nsas_dx = 0.0f;                // domain%dx
};

// cu_bmj.hip
int icar_cu_common_init(icar_hip_ctx *c);
// cu_tiedtke.hip
void icar_tiedtke_free(CuState *s);
int icar_tiedtke_levels_ok(icar_hip_ctx *c, int kts, int kte);
// cu_nsas.hip
void icar_nsas_free(CuState *s);
int icar_nsas_levels_ok(icar_hip_ctx *c, int kts, int kte);
