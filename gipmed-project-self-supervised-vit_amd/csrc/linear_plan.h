// Which kernel runs a product, how K is split and how much scratch it takes -- gv_linear, gv_linear_dw_group and the full-row
// entry points (include/gipvit.h).  This is the ONE place where that selection is stated: the entry points validate their
// arguments, ask for a plan and launch what it says; gv_workspace_bytes validates, asks for the same plan and returns its
// slab_bytes.  Pure host C++17, no HIP: the header compiles with a plain g++ (tests/linear_plan_main.cc pins every predicate's
// edges against tests/traces/linear_plans.json).  The compute-unit budget (gv_cu_budget(), gv_common.h) is an argument.
#pragma once
#include "../../include/gipvit.h"
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace gvplan {

// ---- geometry the selection depends on (gemm.hip / panel.hip static_assert each against the Cfg value it mirrors)
constexpr int BM = 128, BN = 128, BK = 64;              // the tile kernel: output tile, K-step
constexpr int WGS_PER_CU = 2;                           // ... and its resident workgroups per CU (two-stage ring)
constexpr int DW8_P = 128, DW8_Q = 384, DW8_BK = 64;    // the ping-pong dW kernel's tile (gemm_dw8.h)
constexpr int DW8_MIN_K = 2048, DW8_MAX_TILES = 256;
constexpr int PN = 384;                                 // the full-row kernels' column block: the model width they are built for (ViT-S)
constexpr int PANEL_NW = 8, PANEL_BK = 64;              // ... their waves and K-step (the only instantiated geometry)
constexpr int FM_SET8[] = {4, 7, 9, 11, 12};            // ... and their supported 16-row fragments per workgroup
constexpr int64_t WORKSPACE_BYTES = 128L << 20;         // gv_linear_workspace_bytes(): the scratch a caller offers

enum Family { DW8, DW8_SWAPPED, WIDE, TILE, TILE_DEEP, DW8_GROUP, TILE_GROUP };
enum After { AFTER_NONE, AFTER_REDUCE, AFTER_EPILOGUE, AFTER_GROUP_REDUCE };      // what follows the product
// panel_kernel's MODE and its MODE_WIDE epilogues (the GV_EPI_* combinations of the hot path's wide products)
// EP_BIAS_RESID: f32 output = (A W^T + bias) * row_scale + resid -- x + proj(a) / x + fc2(h) of the widths that have no fused
// LayerNorm kernel (ViT-B: N = 768)
enum { MODE_FWD = 0, MODE_BWD = 1, MODE_WIDE = 2 };
enum { EP_NONE = 0, EP_BIAS = 1, EP_BIAS_GELU = 2, EP_BIAS_GELU_SAVE = 3, EP_DGELU = 4, EP_BIAS_RESID = 5 };
constexpr int EP_MLP = 1;           // (MODE_FWD only: the fused-MLP variant of the forward kernel)

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// S slices over `steps` K-steps: ceil(steps / S) steps per slice, and the slices that are then not empty
struct Slices { int per, count; };
inline Slices split_slices(int steps, int S) {
    const int per = (steps + S - 1) / S;
    return {per, (steps + per - 1) / per};
}

// ---- full-row kernels
// rows per workgroup for M rows: the smallest supported FM that covers M in as few full rounds of `cus` workgroups as possible
inline int pick_fm(int M, int cus) {
    const int m16 = (M + 15) / 16;
    const int rounds = (m16 + cus * 12 - 1) / (cus * 12);
    const int need = (m16 + cus * rounds - 1) / (cus * rounds);
    for (int fm : FM_SET8) if (fm >= need) return fm;
    return 12;
}
// MODE_WIDE launch geometry (see the kernel's id mapping): groups of ncb sibling workgroups, ceil(groups / 8) per XCD
inline int wide_grid(int M, int BM_, int ncb) {
    const int P = (M + BM_ - 1) / BM_, groups = (P + ncb - 1) / ncb;
    return 8 * ncb * ((groups + 7) / 8);
}
// ... and the smallest supported FM whose WORKING workgroups (ncb per group of panels; the grid's padding to 8 ncb exits at once)
// fit one round of the CU budget; 12 (several rounds) for larger M
inline int pick_fm_wide(int M, int ncb, int cus) {
    for (int fm : FM_SET8) {
        const int P = (M + 16 * fm - 1) / (16 * fm), groups = (P + ncb - 1) / ncb;
        if (groups * ncb <= cus && wide_grid(M, 16 * fm, ncb) <= 256) return fm;
    }
    return 12;
}
// the fused MLP: 112-row panels, 64 for short M
inline int pick_fm_mlp(int M, int cus) { return M <= cus * 64 ? 4 : 7; }
// the ping-pong k-loop walks K-tiles in pairs (static ring stage): K % 128 == 0; other depths keep the one-stage-ahead loop
inline bool panel_pingpong(int K) { return K % 128 == 0; }
// the timing-row name of a full-row kernel: the instantiation as rocprofv3 prints it
inline void panel_kernel_name(char* out, size_t n, int fm, bool tb, int mode, int ep, bool pp) {
    snprintf(out, n, "panel_kernel<%d, %d, %d, %s, %d, %d, %d>", fm, PANEL_NW, PANEL_BK, tb ? "true" : "false", mode, ep, pp ? 1 : 0);
}

// ---- split policies (three, each with its own reasoning; none of them is tuned here)
// (1) pure ACCUM on the tile kernel (dW over tens of thousands of tokens, the 65536-class DINO head's dX, the grouped dW): as many
// k-slices as fill the resident workgroup slots once -- one more workgroup would run a second round alone -- and at least 512
// rows per slice.  (Halving the slices -- 16 MB of slab instead of 32 -- measured 80 vs 63 us per launch.)
inline int accum_slices(int tiles, int ksteps) {
    constexpr int SLOTS = 256 * WGS_PER_CU;
    const int want = SLOTS / tiles > 0 ? SLOTS / tiles : 1;
    const int maxs = ksteps / (512 / BK) > 0 ? ksteps / (512 / BK) : 1;
    return want < maxs ? want : maxs;
}
// (2) few rows with a fused epilogue (the DINO head's 2048-wide layers, the CLS-only tail's fc2 at 128 / 640 rows: 15 - 80 workgroups
// with 24 - 32 serial K-steps of ~1 us): split K over the idle CUs as well -- >= 4 K-steps per slice, at most one workgroup per CU
inline int few_row_slices(int tiles, int ksteps, int cus) {
    if (!(tiles <= 96 && ksteps >= 16)) return 1;
    return cus / tiles < ksteps / 4 ? cus / tiles : ksteps / 4;
}
// (3) the ping-pong dW kernel: k-slices for `tiles` one-per-CU workgroups over `ktiles` 64-deep K-tiles: the S that minimises
// rounds of `cus` workgroups x K-tiles per slice  (ViT-S block: 36 tiles -> S = 7, one round; ViT-B block: 144 tiles -> S = 3, two
// rounds of 2/3 the depth of S = 1), smallest S on ties, at least four K-tiles per slice, slabs within the workspace
inline int dw8_pick_slices(int tiles, int ktiles, long mn_floats, long workspace_bytes, int cus) {
    int best = 1; long best_cost = -1;
    for (int S = 1; S <= 64; ++S) {
        if (S > 1 && (ktiles / S < 4 || (long)S * mn_floats * 4 > workspace_bytes)) break;
        const long cost = (long)((tiles * S + cus - 1) / cus) * ((ktiles + S - 1) / S);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = S; }
    }
    return best;
}
// 128 x 384 pieces of a Pn x Qn weight gradient; 0: it does not tile
inline int dw8_tiles(int Pn, int Qn) { return (Pn > 0 && Qn > 0 && Pn % DW8_P == 0 && Qn % DW8_Q == 0) ? (Pn / DW8_P) * (Qn / DW8_Q) : 0; }

// ---- gv_linear
struct LinearPlan {
    Family family;
    int wide_ep, fm;                  // WIDE: panel_kernel's EP and FM (the grid follows from FM: wide_grid)
    int ksplit, k_per_split;          // DW8 / TILE: k-slices and their depth (ksplit == 1: no split)
    bool atomic, out_f32;             // TILE: the kernel's ATOMIC (every split launch: partial tiles) and whether its OutT is float
    int epi;                          // TILE: the epilogue mask the kernel is specialised for, -1: the runtime-mask build
    int64_t slab_bytes;               // scratch taken from the workspace, 0: none (a split without a slab meets in C through f32 atomics)
    After after;
};

// the epilogue masks of the hot path that have a kernel of their own, per operand form (anything else, and any N % 8 != 0, runs
// the runtime-mask build)
constexpr int E_B = GV_EPI_BIAS, E_BGS = GV_EPI_BIAS | GV_EPI_GELU | GV_EPI_SAVE_PRE, E_BG = GV_EPI_BIAS | GV_EPI_GELU, E_BR = GV_EPI_BIAS | GV_EPI_RESID,
              E_BP = GV_EPI_BIAS | GV_EPI_POS, E_DG = GV_EPI_DGELU, E_ACC = GV_EPI_ACCUM;
inline bool tile_specialised(bool ta, bool tb, bool c_f32, int e) {
    if (ta && tb) return c_f32 && (e == 0 || e == E_ACC);
    if (tb) return !c_f32 && (e == 0 || e == E_DG);
    return c_f32 ? (e == 0 || e == E_B || e == E_BR || e == E_BP) : (e == 0 || e == E_B || e == E_BGS || e == E_BG);
}

// dW over many token rows on the 8-wave ping-pong kernel (gemm_dw8.h): C = [P x Q] tiles of 128 x 384, or the swapped orientation
inline bool plan_dw8(const gv_linear_args& a, int cus, LinearPlan& pl) {
    if (!(a.trans_a && a.trans_b && a.c_is_f32 && a.epilogue == GV_EPI_ACCUM && a.workspace && aligned16(a.workspace))) return false;
    if (a.alpha != 0.f && a.alpha != 1.f) return false;
    if (a.K < DW8_MIN_K) return false;
    const int normal = dw8_tiles(a.M, a.N);
    const int swapped = normal || (a.colsum_a && a.N / DW8_P < 12) ? 0 : dw8_tiles(a.N, a.M);      // (column sums: >= 12 P tiles, gemm_dw8.h)
    const int tiles = normal ? normal : swapped;
    if (!tiles || tiles > DW8_MAX_TILES) return false;
    const int ktiles = (a.K + DW8_BK - 1) / DW8_BK;
    const long mn = (long)a.M * a.N;
    const Slices sl = split_slices(ktiles, dw8_pick_slices(tiles, ktiles, mn, a.workspace_bytes, cus));
    if (sl.count * mn * 4 > a.workspace_bytes) return false;
    pl.family = normal ? DW8 : DW8_SWAPPED;
    pl.ksplit = sl.count; pl.k_per_split = sl.per * DW8_BK;
    pl.slab_bytes = sl.count * mn * 4; pl.after = AFTER_REDUCE;
    return true;
}

// wide products on the full-row kernel: C[M, N] = epilogue(A W^T) with N a multiple of 384, K a multiple of 128 and one of the
// hot path's epilogues -- row panels sized for ONE round of workgroups, 768-B row segments out; these kernels take no scratch
inline bool plan_wide(const gv_linear_args& a, int cus, LinearPlan& pl) {
    if (a.trans_a || a.N % PN != 0 || !panel_pingpong(a.K) || a.M < 2048 || a.ldc % 2 != 0) return false;
    if (a.alpha != 0.f && a.alpha != 1.f) return false;
    const int e = a.epilogue;
    int ep = -1;
    if (a.c_is_f32) {      // x + Linear(a) with an f32 residual stream, where no fused LayerNorm kernel exists for the width
        if (a.trans_b || e != E_BR || a.ldr % 2 != 0) return false;
        if ((const void*)a.resid == (const void*)a.C) return false;      // in place: the rows the last two panels share would be updated twice
        ep = EP_BIAS_RESID;
    } else {
        if (a.ld_aux % 2 != 0) return false;
        if (!a.trans_b) ep = e == E_B ? EP_BIAS : e == E_BG ? EP_BIAS_GELU : e == E_BGS ? EP_BIAS_GELU_SAVE : -1;
        else ep = e == 0 ? EP_NONE : e == E_DG ? EP_DGELU : -1;
        if (ep < 0) return false;
    }
    pl.family = WIDE; pl.wide_ep = ep;
    pl.fm = pick_fm_wide(a.M, a.N / PN, cus);
    return true;
}

// the 128x128-tile kernel, two-stage ring or -- few workgroups, a long reduction -- four-stage
inline void plan_tile(const gv_linear_args& a, int cus, LinearPlan& pl) {
    const int e = a.epilogue;
    const bool ta = a.trans_a != 0, tb = a.trans_b != 0;
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN), ksteps = (a.K + BK - 1) / BK;
    const long mn = (long)a.M * a.N;
    Slices sl{ksteps, 1};
    // Split K when the output grid alone cannot fill 256 CUs.  Partial sums meet in C through f32 atomics (or a slab + reduce),
    // which needs pure ACCUM semantics (C already holds the value to add to).
    if (a.c_is_f32 && e == GV_EPI_ACCUM && tiles < 192 * WGS_PER_CU && (a.N & 7) == 0) {
        const int S = accum_slices(tiles, ksteps);
        if (S > 1) sl = split_slices(ksteps, S);
    }
    // Few tiles, a long reduction and an epilogue other than ACCUM: with a caller's scratch, split K and let ONE pass sum the partial
    // tiles and apply the epilogue
    bool epi_split = false;
    if (sl.count == 1 && !ta && !(e & (GV_EPI_ACCUM | GV_EPI_POS)) && (a.N & 7) == 0 && a.workspace && aligned16(a.workspace) && !a.colsum_a &&
        (!(e & (GV_EPI_DGELU | GV_EPI_SAVE_PRE)) || a.ld_aux % 4 == 0)) {
        const int S = few_row_slices(tiles, ksteps, cus);
        if (S >= 2) {
            const Slices fs = split_slices(ksteps, S);
            if (fs.count * mn * 4 <= a.workspace_bytes) { sl = fs; epi_split = true; }
        }
    }
    pl.ksplit = sl.count; pl.k_per_split = sl.per * BK;
    pl.atomic = sl.count > 1;
    // a slab that does not fit the scratch is not used (atomics)
    const bool slab = pl.atomic && a.workspace && sl.count * mn * 4 <= a.workspace_bytes && aligned16(a.workspace);
    pl.slab_bytes = slab ? sl.count * mn * 4 : 0;
    pl.after = !slab ? AFTER_NONE : epi_split ? AFTER_EPILOGUE : AFTER_REDUCE;
    pl.out_f32 = pl.atomic || a.c_is_f32;
    pl.epi = pl.atomic ? (int)GV_EPI_ACCUM : ((a.N & 7) == 0 && tile_specialised(ta, tb, a.c_is_f32 != 0, e)) ? e : -1;
    // at most one workgroup per CU anyway and >= 8 K-steps per workgroup: the four-stage ring
    const bool deep = tiles * sl.count <= cus && (pl.atomic ? pl.k_per_split : a.K) >= 8 * BK;
    pl.family = deep ? TILE_DEEP : TILE;
}

inline LinearPlan plan_linear(const gv_linear_args& a, int cu_budget) {
    LinearPlan pl{};
    pl.ksplit = 1;
    if (!plan_dw8(a, cu_budget, pl) && !plan_wide(a, cu_budget, pl)) plan_tile(a, cu_budget, pl);
    return pl;
}

// the timing-row name of the product kernel, as gv_linear_timing_read reports it
inline void linear_kernel_name(const LinearPlan& pl, const gv_linear_args& a, char* out, size_t n) {
    const auto tf = [](bool b) { return b ? "true" : "false"; };
    switch (pl.family) {
        case DW8: case DW8_SWAPPED: snprintf(out, n, "dw8_kernel<%s>", tf(pl.family == DW8_SWAPPED)); break;
        case WIDE: panel_kernel_name(out, n, pl.fm, a.trans_b != 0, MODE_WIDE, pl.wide_ep, true); break;
        default:
            snprintf(out, n, "gemm_%skernel<%s, %s, %s, %s, %d>", pl.family == TILE_DEEP ? "deep_" : "", tf(a.trans_a != 0), tf(a.trans_b != 0),
                     pl.out_f32 ? "float" : "bf16", tf(pl.atomic), pl.epi);
    }
}

// ---- gv_linear_dw_group: one launch over the weight-gradient products that reduce over the same token rows, one reduce for all
struct DwGroupPlan {
    Family family;                    // DW8_GROUP when every problem tiles into 128 x 384 pieces, else TILE_GROUP
    int total_tiles, ksplit, k_per_split;
    int64_t slab_bytes;
    After after;
};
inline DwGroupPlan plan_dw_group(const gv_linear_dw_group_args& a, int cu_budget) {
    DwGroupPlan pl{};
    pl.after = AFTER_GROUP_REDUCE;
    long mn = 0;
    int tiles8 = 0, tiles = 0;
    bool ok8 = a.K >= DW8_MIN_K;
    for (int q = 0; q < a.n; ++q) {
        const int M = a.prob[q].M, N = a.prob[q].N;
        mn += (long)M * N;
        tiles += ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
        const int t8 = dw8_tiles(M, N);
        ok8 = ok8 && t8 > 0;
        tiles8 += t8;
    }
    if (ok8 && tiles8 <= DW8_MAX_TILES) {
        const int ktiles = (a.K + DW8_BK - 1) / DW8_BK;
        const Slices sl = split_slices(ktiles, dw8_pick_slices(tiles8, ktiles, mn, a.workspace_bytes, cu_budget));
        if (sl.count * mn * 4 <= a.workspace_bytes) {
            pl.family = DW8_GROUP; pl.total_tiles = tiles8;
            pl.ksplit = sl.count; pl.k_per_split = sl.per * DW8_BK; pl.slab_bytes = sl.count * mn * 4;
            return pl;
        }
    }
    const int ksteps = (a.K + BK - 1) / BK;
    const Slices sl = split_slices(ksteps, accum_slices(tiles, ksteps));
    pl.family = TILE_GROUP; pl.total_tiles = tiles;
    pl.ksplit = sl.count; pl.k_per_split = sl.per * BK; pl.slab_bytes = sl.count * mn * 4;      // (may exceed the workspace: the entry point refuses)
    return pl;
}
inline const char* group_kernel_name(const DwGroupPlan& pl) { return pl.family == DW8_GROUP ? "dw8_group_kernel" : "gemm_dw_group_kernel"; }

}  // namespace gvplan
