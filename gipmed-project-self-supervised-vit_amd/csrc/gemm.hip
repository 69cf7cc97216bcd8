// bf16 MFMA GEMM for gfx950 with fused epilogues -- gv_linear (include/gipvit.h).
//
// Replaces the ATen addmm / mm calls behind nn.Linear forward and backward in the
// reference's ViT blocks, patch embedding and DINOHead (vit.pyc@L98-104, L119-131,
// L167-170, L326-330; reference train.py:1045 forward, :1071 backward).
//
// The path's GEMMs are skinny: tens of thousands of token rows against K = 384..2048 (6..32
// k-steps per tile), or -- for the weight gradients -- a tiny output reduced over all tokens.
// Design (MI355X_MICROARCH / cdna_hip_programming section 5; geometry, ring depth and schedule
// were chosen with tools/gemm_lab.hip on MI355X, numbers in DESIGN.md):
//   * one 256-thread workgroup (2x2 waves, 64x64 per wave = 4x4 v_mfma_f32_16x16x32_bf16 per
//     32-deep k-step) per 128x128 output tile, 2 workgroups per CU: the partner workgroup's
//     k-loop covers this one's prologue / epilogue.  BK = 64, 2-stage LDS ring (64 KiB).
//   * the ring is filled by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction, issued
//     from inline asm so hipcc's waitcnt pass does not drain it) one k-step ahead of the MFMAs,
//     behind a hand-counted s_waitcnt vmcnt(N) and ONE raw s_barrier per k-step.
//   * the LDS image is lane-linear, so bank swizzles are applied to the per-lane SOURCE address
//     and again on the read (rule 21):
//       "natural" operand (reduction index contiguous, x[M,K], W[N,K]): 128-B rows, 16-B chunk
//        index XOR (row & 7) -> conflict-free ds_read_b128;
//       "transposed" operand (reduction index strided: dY[tokens,N] for dW, W[N,K] for dX):
//        [64 k][128 cols] image, 32-B chunk index XOR f(k), fragments by two
//        ds_read_b64_tr_b16 (hardware transpose) -- no transposed copies in HBM.
//   * MFMA roles are swapped (weight fragment as the A operand) so each lane ends up with 4
//     consecutive output columns; the accumulators then pass through a per-wave LDS image so
//     that bias / residual / saved-activation loads and all stores are whole 128..256-B row
//     segments.  Epilogue operands (residual, pos-embed, dGELU input, bias) are fetched BEFORE
//     the k-loop; the epilogue mask is a template parameter (a runtime mask cost a load + wait
//     per element).  GELU / GELU' are clamped odd polynomials (gv_common.h), no transcendentals.
//   * split-K (dW over tens of thousands of tokens, dX of the 65536-class head): partial tiles
//     go to a caller-provided slab with plain row stores and a reduce kernel adds them into C
//     (f32 atomics run at ~1.3 TB/s on this part; they remain the fallback without a workspace).
//     The bias gradient (column sums of dY) rides along as one extra MFMA per A fragment
//     against a ones fragment.
//   * workgroup -> tile map is XCD-aware: each XCD's workgroups walk a contiguous band of tiles.
#ifndef GV_GEMM_BM
#define GV_GEMM_BM 128
#define GV_GEMM_BN 128
#define GV_GEMM_BK 64
#define GV_GEMM_WM 2
#define GV_GEMM_WN 2
#define GV_GEMM_NSTAGE 2
#endif
#include "gemm_core.h"
#include "gemm_dw8.h"
#include "linear_plan.h"
#include "timing.h"
#include <type_traits>
#include <stdlib.h>
#include <mutex>
#include <vector>
#include <string.h>

namespace {

using namespace gvgemm;
using namespace gvplan;

// production geometry (chosen with tools/gemm_lab.hip on MI355X); linear_plan.h sizes its launches
using PCfg = Cfg<GV_GEMM_BM, GV_GEMM_BN, GV_GEMM_BK, GV_GEMM_WM, GV_GEMM_WN, GV_GEMM_NSTAGE>;
static_assert(BM == PCfg::BM && BN == PCfg::BN && BK == PCfg::BK, "linear_plan.h: tile geometry");
static_assert(WGS_PER_CU == ((160 * 1024 / PCfg::LDS) < 2 ? 1 : ((160 * 1024 / PCfg::LDS) >= 3 ? 3 : 2)), "linear_plan.h: resident workgroups per CU");
static_assert(DW8_STAGE == (DW8_P + DW8_Q) * DW8_BK * 2 && DW8_IMG == DW8_P * DW8_BK * 2, "linear_plan.h: dw8 tile");

template <bool TA, bool TB, typename OutT, bool ATOMIC, int EPI>
__global__ __launch_bounds__(PCfg::THREADS, PCfg::THREADS * WGS_PER_CU / 256) void gemm_kernel(const GemmP g) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    gemm_body<PCfg, TA, TB, OutT, ATOMIC, EPI>(g, (GV_LDS char*)smem_raw);
}

// Few tiles, long reduction (the DINO head's 2048-wide layers and the CLS-only tail at 128 / 640 rows: 15 - 80 workgroups, 24 - 32
// K-steps each): with one workgroup per CU and a two-stage ring every K-step pays a whole L2 / HBM round trip, ~1 us -- 34 us for
// K = 2048 whatever M is.  The same body on a FOUR-stage ring (128 KB of LDS, three K-steps in flight): same tiles, same
// accumulation order, bit-identical results.
using DCfg = Cfg<GV_GEMM_BM, GV_GEMM_BN, GV_GEMM_BK, GV_GEMM_WM, GV_GEMM_WN, 4>;
static_assert(DCfg::LDS <= 160 * 1024, "deep ring");
template <bool TA, bool TB, typename OutT, bool ATOMIC, int EPI>
__global__ __launch_bounds__(DCfg::THREADS, 1) void gemm_deep_kernel(const GemmP g) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    gemm_body<DCfg, TA, TB, OutT, ATOMIC, EPI>(g, (GV_LDS char*)smem_raw);
}

// the tile kernel the plan names (pl.family: two- or four-stage ring), one workgroup per (tile, k-slice) -- measured
// (tools/gemm_lab): with K = 384..2048 one workgroup per item beats a persistent walk
template <bool TA, bool TB, typename OutT, bool ATOMIC, int EPI = -1>
int launch(const GemmP& p, const LinearPlan& pl, const gv_linear_args& a, hipStream_t s) {
    const int grid = p.tiles_m * p.tiles_n * p.ksplit;
    const bool deep = pl.family == TILE_DEEP;
    auto kern = deep ? gemm_deep_kernel<TA, TB, OutT, ATOMIC, EPI> : gemm_kernel<TA, TB, OutT, ATOMIC, EPI>;
    const int lds = deep ? DCfg::LDS : PCfg::LDS;
    static GvLdsOptIn opt_in[2];     // > 64 KiB of dynamic LDS: once per kernel instantiation and device
    if (int rc = gv_lds_opt_in(opt_in[deep], (const void*)kern, lds, "gemm")) return rc;
    int th = -1;
    if (gvtime::enabled()) {      // algorithmic bytes: operands once, output once, epilogue operands once
        const int e = EPI >= 0 ? EPI : p.epi;
        const double mn = (double)p.M * p.N;
        double bytes = 2.0 * p.K * ((double)p.M + p.N) + mn * sizeof(OutT);
        if (e & GV_EPI_ACCUM) bytes += mn * 4;
        if (e & GV_EPI_RESID) bytes += mn * 4;
        if (e & GV_EPI_DGELU) bytes += mn * 2;
        if (e & GV_EPI_SAVE_PRE) bytes += mn * 2;
        char name[96];
        linear_kernel_name(pl, a, name, sizeof(name));
        th = gvtime::begin(name, 2.0 * p.M * p.N * p.K, bytes, s);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PCfg::THREADS), lds, s, p);
    gvtime::end(th, s);
    GV_LAUNCH_CHECK("gv_linear");
    return GV_OK;
}

// C[m][n] += sum_s slab[s][m][n]  (split-K reduce; 16 B per lane, fully coalesced)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slab, float* __restrict__ C, long MN4, int S, int N4, long ldc4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < MN4; i += (long)gridDim.x * 256) {
        // four slab loads in flight per thread (the slabs are independent streams; a rolled loop keeps one)
        f32x4 acc = ((const f32x4*)slab)[i];
        int s2 = 1;
        for (; s2 + 3 < S; s2 += 4) {
            const f32x4 a0 = ((const f32x4*)slab)[(long)s2 * MN4 + i], a1 = ((const f32x4*)slab)[(long)(s2 + 1) * MN4 + i];
            const f32x4 a2 = ((const f32x4*)slab)[(long)(s2 + 2) * MN4 + i], a3 = ((const f32x4*)slab)[(long)(s2 + 3) * MN4 + i];
            acc += (a0 + a1) + (a2 + a3);
        }
        for (; s2 < S; ++s2) acc += ((const f32x4*)slab)[(long)s2 * MN4 + i];
        const long m = i / N4, n4 = i - m * N4;
        f32x4* dst = (f32x4*)C + m * ldc4 + n4;
        *dst = *dst + acc;
    }
}

// split-K with an epilogue other than ACCUM: C = epilogue(sum_s slab[s]) -- the epilogue of gemm_core.h in its order (alpha is in the
// partial tiles already; bias, saved pre-activation, GELU, GELU' of the saved input, row factor + residual), 16 B of output columns per lane
struct SplitEpiP {
    const float* slab; void* C; const float* bias; const float* resid; const bf16* aux_in; bf16* aux_out; const float* row_scale;
    long ldc, ldr, ld_aux; int M, N, S, epi;
};
template <typename OutT>
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const SplitEpiP q) {
    const int N4 = q.N >> 2;
    const long MN = (long)q.M * q.N, MN4 = MN >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < MN4; i += (long)gridDim.x * 256) {
        const int m = (int)(i / N4), n = (int)(i - (long)m * N4) * 4;
        f32x4 v = *(const f32x4*)(q.slab + i * 4);
        for (int s2 = 1; s2 < q.S; ++s2) v += *(const f32x4*)(q.slab + (long)s2 * MN + i * 4);
        if (q.epi & GV_EPI_BIAS) v += *(const f32x4*)(q.bias + n);
        if (q.epi & GV_EPI_SAVE_PRE) *(bf16x4*)(q.aux_out + (long)m * q.ld_aux + n) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
        if (q.epi & GV_EPI_GELU) { v[0] = gelu_f(v[0]); v[1] = gelu_f(v[1]); v[2] = gelu_f(v[2]); v[3] = gelu_f(v[3]); }
        if (q.epi & GV_EPI_DGELU) {
            const bf16x4 a = *(const bf16x4*)(q.aux_in + (long)m * q.ld_aux + n);
            v[0] *= dgelu_f((float)a[0]); v[1] *= dgelu_f((float)a[1]); v[2] *= dgelu_f((float)a[2]); v[3] *= dgelu_f((float)a[3]);
        }
        if (q.epi & GV_EPI_RESID) {
            if (q.row_scale) v *= q.row_scale[m];
            v += *(const f32x4*)(q.resid + (long)m * q.ldr + n);
        }
        if constexpr (sizeof(OutT) == 4) *(f32x4*)((float*)q.C + (long)m * q.ldc + n) = v;
        else *(bf16x4*)((bf16*)q.C + (long)m * q.ldc + n) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    }
}

// one launch over up to GV_DW_GROUP_MAX weight-gradient products that reduce over the same token rows: every workgroup
// runs ONE (problem, tile, k-slice) item of the split-K dW kernel, partial tiles go to the shared slab, one reduce
// launch folds all problems.  Items are slice-major over the concatenated tile lists, XCD-contiguous like make_walk.
struct GroupP { GemmP prob[GV_DW_GROUP_MAX]; int n, total_tiles; int tile_base[GV_DW_GROUP_MAX + 1]; };

__global__ __launch_bounds__(PCfg::THREADS, PCfg::THREADS * WGS_PER_CU / 256) void gemm_dw_group_kernel(const GroupP G) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int nb = gridDim.x, xcd = blockIdx.x & 7, lw = blockIdx.x >> 3;
    const int qd = nb >> 3, rm = nb & 7;
    const int b = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + lw;      // bijective XCD-contiguous remap
    const int slice = b / G.total_tiles, tg = b - slice * G.total_tiles;
    int q = 0;
#pragma unroll
    for (int i = 1; i < GV_DW_GROUP_MAX; ++i) q += (i < G.n && tg >= G.tile_base[i]) ? 1 : 0;
    const GemmP& g = G.prob[q];
    Walk wk;
    wk.first = slice * (g.tiles_m * g.tiles_n) + (tg - G.tile_base[q]); wk.stride = 1 << 30; wk.count = 1; wk.mlo = 0; wk.mcnt = g.tiles_m;
    gemm_body_w<PCfg, true, true, float, true, GV_EPI_ACCUM>(g, (GV_LDS char*)smem_raw, wk);
}

struct ReduceGroupP { const float* slab[GV_DW_GROUP_MAX]; float* C[GV_DW_GROUP_MAX]; long MN4[GV_DW_GROUP_MAX]; int N4[GV_DW_GROUP_MAX]; long ldc4[GV_DW_GROUP_MAX]; int S; };
__global__ __launch_bounds__(256) void splitk_reduce_group_kernel(const ReduceGroupP R) {
    const int q = blockIdx.y;
    const float* __restrict__ slab = R.slab[q];
    const long MN4 = R.MN4[q];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < MN4; i += (long)gridDim.x * 256) {
        f32x4 acc = ((const f32x4*)slab)[i];
        int s2 = 1;
        for (; s2 + 1 < R.S; s2 += 2) acc += ((const f32x4*)slab)[(long)s2 * MN4 + i] + ((const f32x4*)slab)[(long)(s2 + 1) * MN4 + i];
        for (; s2 < R.S; ++s2) acc += ((const f32x4*)slab)[(long)s2 * MN4 + i];
        const long m = i / R.N4[q], n4 = i - m * R.N4[q];
        f32x4* dst = (f32x4*)R.C[q] + m * R.ldc4[q] + n4;
        *dst = *dst + acc;
    }
}

// C += sum of the S partial slabs: the reduce launch of every single-product split (dw8 slices, the tile kernel's ACCUM split)
int launch_splitk_reduce(const float* slab, const gv_linear_args& a, int S, hipStream_t s, const char* what) {
    const long MN4 = (long)a.M * a.N / 4;
    long blocks = (MN4 + 255) / 256; if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, slab, (float*)a.C, MN4, S, a.N / 4, a.ldc / 4);
    GV_LAUNCH_CHECK(what);
    return GV_OK;
}

// dW_q += sum of problem q's S partial slabs, all problems of a group in one launch; the slabs lie in the workspace in problem order
int launch_group_reduce(const gv_linear_dw_group_args& a, int S, hipStream_t s, const char* what) {
    ReduceGroupP R{};
    long max4 = 0, slab_floats = 0;
    for (int q = 0; q < a.n; ++q) {
        const auto& pr = a.prob[q];
        R.slab[q] = a.workspace + slab_floats; R.C[q] = pr.dW; R.MN4[q] = (long)pr.M * pr.N / 4; R.N4[q] = pr.N / 4; R.ldc4[q] = pr.ldw / 4;
        slab_floats += (long)S * pr.M * pr.N;
        if (R.MN4[q] > max4) max4 = R.MN4[q];
    }
    R.S = S;
    long blocks = (max4 + 255) / 256; if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(splitk_reduce_group_kernel, dim3((unsigned)blocks, a.n), dim3(256), 0, s, R);
    GV_LAUNCH_CHECK(what);
    return GV_OK;
}

// a group's concatenated tile list (GroupP / Dw8GroupP): problem q's tiles start at tile_base[q]
template <class GP, class F>
void fill_tile_base(GP& G, int n, F tiles_of) {
    int tb = 0;
    for (int q = 0; q < n; ++q) { G.tile_base[q] = tb; tb += tiles_of(q); }
    for (int q = n; q <= GV_DW_GROUP_MAX; ++q) G.tile_base[q] = tb;
    G.n = n; G.total_tiles = tb;
}

// dW over many token rows on the 8-wave ping-pong kernel (gemm_dw8.h), then the slab reduce
template <bool SWAP>
int launch_dw8(const Dw8P& q, const gv_linear_args& a, hipStream_t s) {
    auto kern = dw8_kernel<SWAP>;
    static GvLdsOptIn opt_in;
    if (int rc = gv_lds_opt_in(opt_in, (const void*)kern, DW8_LDS, "gemm(dw8)")) return rc;
    const int th = gvtime::enabled() ? gvtime::begin(SWAP ? "dw8_kernel<true>" : "dw8_kernel<false>", 2.0 * a.M * a.N * q.K, 2.0 * q.K * ((double)a.M + a.N) + 8.0 * a.M * a.N, s) : -1;
    hipLaunchKernelGGL(kern, dim3(q.tiles_p * q.tiles_q * q.ksplit), dim3(512), DW8_LDS, s, q);
    gvtime::end(th, s);
    GV_LAUNCH_CHECK("gv_linear(dw8)");
    return launch_splitk_reduce(q.slab, a, q.ksplit, s, "gv_linear(dw8 reduce)");
}

int run_dw8(const gv_linear_args* a, const LinearPlan& pl, hipStream_t s) {
    const bool normal = pl.family == DW8;
    Dw8P q;
    q.K = a->K; q.slab = (float*)a->workspace; q.colsum = a->colsum_a;
    if (normal) { q.P = (const bf16*)a->A; q.ldp = a->lda; q.Pn = a->M; q.Q = (const bf16*)a->B; q.ldq = a->ldb; q.Qn = a->N; }
    else { q.P = (const bf16*)a->B; q.ldp = a->ldb; q.Pn = a->N; q.Q = (const bf16*)a->A; q.ldq = a->lda; q.Qn = a->M; }
    q.tiles_p = q.Pn / DW8_P; q.tiles_q = q.Qn / DW8_Q;
    q.ksplit = pl.ksplit; q.k_per_split = pl.k_per_split;
    return normal ? launch_dw8<false>(q, *a, s) : launch_dw8<true>(q, *a, s);
}

// C = epilogue(sum of the S partial slabs): the pass behind the few-row split
int launch_splitk_epilogue(const float* slab, const gv_linear_args& a, int S, hipStream_t s) {
    SplitEpiP q{slab, a.C, a.bias, a.resid, (const bf16*)a.aux_in, (bf16*)a.aux_out, a.row_scale, a.ldc, a.ldr, a.ld_aux, a.M, a.N, S, a.epilogue};
    const long MN4 = (long)a.M * a.N / 4;
    long blocks = (MN4 + 255) / 256; if (blocks > 2048) blocks = 2048;
    if (a.c_is_f32) hipLaunchKernelGGL(splitk_epilogue_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, q);
    else hipLaunchKernelGGL(splitk_epilogue_kernel<bf16>, dim3((unsigned)blocks), dim3(256), 0, s, q);
    GV_LAUNCH_CHECK("gv_linear(splitk_epilogue)");
    return GV_OK;
}

// gv_linear's argument checks, then the plan of the call (linear_plan.h)
int checked_plan(const gv_linear_args* a, LinearPlan* pl) {
    GV_REQUIRE(a && a->A && a->B && a->C, GV_E_NULL, "gv_linear: null operand");
    GV_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, GV_E_SHAPE, "gv_linear: M,N,K must be > 0 (got %d,%d,%d)", a->M, a->N, a->K);
    const bool ta = a->trans_a != 0, tb = a->trans_b != 0;
    GV_REQUIRE(!(ta && !tb), GV_E_UNSUPPORTED, "gv_linear: (trans_a=1, trans_b=0) is not built");
    if (!ta || !tb)
        GV_REQUIRE(a->K % 32 == 0, GV_E_SHAPE, "gv_linear: K=%d must be a multiple of 32 when an operand is k-contiguous", a->K);
    if (ta) GV_REQUIRE(a->M % 8 == 0, GV_E_SHAPE, "gv_linear: M=%d must be a multiple of 8 with trans_a", a->M);
    if (tb) GV_REQUIRE(a->N % 8 == 0, GV_E_SHAPE, "gv_linear: N=%d must be a multiple of 8 with trans_b", a->N);
    GV_REQUIRE(a->lda % 8 == 0 && a->ldb % 8 == 0, GV_E_ALIGN, "gv_linear: lda/ldb must be multiples of 8 elements");
    GV_REQUIRE(gv_aligned(a->A, 16) && gv_aligned(a->B, 16) && gv_aligned(a->C, 16), GV_E_ALIGN, "gv_linear: A/B/C must be 16-byte aligned");
    const int e = a->epilogue;
    GV_REQUIRE((e & ~GV_EPI_ALL) == 0, GV_E_UNSUPPORTED, "gv_linear: epilogue 0x%x has bits outside the GV_EPI_* mask 0x%x", e, GV_EPI_ALL);
    if (e & GV_EPI_BIAS) GV_REQUIRE(a->bias && gv_aligned(a->bias, 16), GV_E_NULL, "gv_linear: BIAS needs an aligned bias");
    if (e & GV_EPI_RESID) GV_REQUIRE(a->resid && a->ldr % 4 == 0, GV_E_NULL, "gv_linear: RESID needs resid with ldr %% 4 == 0");
    if (e & GV_EPI_DGELU) GV_REQUIRE(a->aux_in && a->ld_aux % 4 == 0, GV_E_NULL, "gv_linear: DGELU needs aux_in");
    if (e & GV_EPI_SAVE_PRE) GV_REQUIRE(a->aux_out && a->ld_aux % 4 == 0, GV_E_NULL, "gv_linear: SAVE_PRE needs aux_out");
    if (e & GV_EPI_POS) GV_REQUIRE(a->pos && a->P > 0, GV_E_NULL, "gv_linear: POS needs pos and P");
    if (e & GV_EPI_ACCUM) GV_REQUIRE(a->c_is_f32, GV_E_UNSUPPORTED, "gv_linear: ACCUM needs an f32 C");
    GV_REQUIRE(a->ldc % 4 == 0, GV_E_ALIGN, "gv_linear: ldc must be a multiple of 4");
    *pl = plan_linear(*a, gv_cu_budget());
    // (the full-row kernel does not read colsum_a; the ping-pong kernel runs with trans_a only)
    if (a->colsum_a && (pl->family == TILE || pl->family == TILE_DEEP))
        GV_REQUIRE(ta, GV_E_UNSUPPORTED, "gv_linear: colsum_a needs trans_a (it sums the dW product's A operand)");
    return GV_OK;
}

// gv_linear_dw_group's argument checks, then the plan of the call
int checked_group_plan(const gv_linear_dw_group_args* a, DwGroupPlan* pl) {
    GV_REQUIRE(a && a->n >= 1 && a->n <= GV_DW_GROUP_MAX, GV_E_SHAPE, "gv_linear_dw_group: 1..%d problems", GV_DW_GROUP_MAX);
    GV_REQUIRE(a->K > 0 && a->workspace && gv_aligned(a->workspace, 16), GV_E_NULL, "gv_linear_dw_group: K > 0 and an aligned workspace are required");
    for (int q = 0; q < a->n; ++q) {
        const auto& pr = a->prob[q];
        GV_REQUIRE(pr.dY && pr.X && pr.dW, GV_E_NULL, "gv_linear_dw_group: null operand in problem %d", q);
        GV_REQUIRE(pr.M > 0 && pr.N > 0 && pr.M % 8 == 0 && pr.N % 8 == 0, GV_E_SHAPE, "gv_linear_dw_group: M, N must be positive multiples of 8 (problem %d: %d x %d)", q, pr.M, pr.N);
        GV_REQUIRE(pr.ldy % 8 == 0 && pr.ldx % 8 == 0 && pr.ldw % 4 == 0, GV_E_ALIGN, "gv_linear_dw_group: leading dimensions misaligned (problem %d)", q);
        GV_REQUIRE(gv_aligned(pr.dY, 16) && gv_aligned(pr.X, 16) && gv_aligned(pr.dW, 16), GV_E_ALIGN, "gv_linear_dw_group: operands must be 16-byte aligned");
    }
    *pl = plan_dw_group(*a, gv_cu_budget());
    return GV_OK;
}

}  // namespace

// panel.hip: the wide products plan_wide admits, on the full-row kernel
int gv_panel_wide(const gv_linear_args* a, const gvplan::LinearPlan& pl, hipStream_t s);

extern "C" int64_t gv_linear_workspace_bytes(void) { return WORKSPACE_BYTES; }

// the scratch the call would take "as if the full scratch were offered": the entry point's own checks and its own plan, nothing launched
extern "C" int64_t gv_workspace_bytes(int32_t op, const void* args) {
    if (!args) { gv_set_error("gv_workspace_bytes: null args"); return -1; }
    float* const offered = (float*)(uintptr_t)256;      // (aligned, never dereferenced)
    if (op == GV_OP_LINEAR) {
        gv_linear_args a = *(const gv_linear_args*)args;
        a.workspace = offered; a.workspace_bytes = WORKSPACE_BYTES;
        LinearPlan pl;
        return checked_plan(&a, &pl) == GV_OK ? pl.slab_bytes : -1;
    }
    if (op == GV_OP_LINEAR_DW_GROUP) {
        gv_linear_dw_group_args a = *(const gv_linear_dw_group_args*)args;
        a.workspace = offered; a.workspace_bytes = WORKSPACE_BYTES;
        DwGroupPlan pl;
        return checked_group_plan(&a, &pl) == GV_OK ? pl.slab_bytes : -1;
    }
    gv_set_error("gv_workspace_bytes: op %d takes no scratch query (GV_OP_LINEAR, GV_OP_LINEAR_DW_GROUP)", op);
    return -1;
}

// ---- live per-kernel timing (timing.h; gv_linear_timing / gv_linear_timing_read of include/gipvit.h)
namespace {
struct TimingRec { char name[96]; hipEvent_t e0, e1; double flops, bytes; };      // (the name is copied: callers format it on their stack)
struct Timing {
    std::mutex mu;
    bool on = false;
    std::vector<TimingRec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};
Timing& timing() { static Timing t; return t; }
}  // namespace

bool gvtime::enabled() { return timing().on; }
int gvtime::begin(const char* kernel_name, double flops, double bytes, hipStream_t s) {
    Timing& tm = timing();
    std::lock_guard<std::mutex> lk(tm.mu);
    if (!tm.on) return -1;
    TimingRec r{{0}, tm.get(), tm.get(), flops, bytes};
    strncpy(r.name, kernel_name, sizeof(r.name) - 1);
    (void)hipEventRecord(r.e0, s);
    tm.recs.push_back(r);
    return (int)tm.recs.size() - 1;
}
void gvtime::end(int handle, hipStream_t s) {
    if (handle < 0) return;
    Timing& tm = timing();
    std::lock_guard<std::mutex> lk(tm.mu);
    if (handle < (int)tm.recs.size()) (void)hipEventRecord(tm.recs[handle].e1, s);
}

extern "C" int gv_linear_timing(int enable) {
    Timing& tm = timing();
    std::lock_guard<std::mutex> lk(tm.mu);
    if (enable) {
        for (auto& r : tm.recs) { tm.pool.push_back(r.e0); tm.pool.push_back(r.e1); }
        tm.recs.clear();
    }
    tm.on = enable != 0;
    return GV_OK;
}

extern "C" int gv_linear_timing_read(gv_linear_timing_row* rows, int max_rows) {
    GV_REQUIRE(rows && max_rows > 0, GV_E_NULL, "gv_linear_timing_read: null rows");
    Timing& tm = timing();
    std::lock_guard<std::mutex> lk(tm.mu);
    int n = 0;
    for (auto& r : tm.recs) {
        hipError_t e = hipEventSynchronize(r.e1);
        if (e != hipSuccess) { gv_set_error("gv_linear_timing_read: %s", hipGetErrorString(e)); return (int)e; }
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, r.e0, r.e1);
        if (e != hipSuccess) { gv_set_error("gv_linear_timing_read: %s", hipGetErrorString(e)); return (int)e; }
        int i = 0;
        while (i < n && strcmp(rows[i].name, r.name) != 0) ++i;
        if (i == n) {
            if (n == max_rows) continue;
            memset(&rows[n], 0, sizeof(rows[n]));
            strncpy(rows[n].name, r.name, sizeof(rows[n].name) - 1);
            ++n;
        }
        rows[i].launches += 1; rows[i].seconds += ms * 1e-3; rows[i].flops += r.flops; rows[i].bytes += r.bytes;
    }
    return n;
}

extern "C" int gv_linear(const gv_linear_args* a, void* stream) {
    LinearPlan pl;
    if (int rc = checked_plan(a, &pl)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (pl.family == DW8 || pl.family == DW8_SWAPPED) return run_dw8(a, pl, s);
    if (pl.family == WIDE) return gv_panel_wide(a, pl, s);

    const bool ta = a->trans_a != 0, tb = a->trans_b != 0;
    const int e = a->epilogue;
    GemmP p;
    p.A = (const bf16*)a->A; p.B = (const bf16*)a->B; p.C = a->C;
    p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc;
    p.epi = e; p.bias = a->bias; p.resid = a->resid; p.ldr = a->ldr;
    p.aux_in = (const bf16*)a->aux_in; p.ld_aux = a->ld_aux; p.aux_out = (bf16*)a->aux_out;
    p.pos = a->pos; p.P = a->P; p.alpha = a->alpha == 0.f ? 1.f : a->alpha;
    p.tiles_m = (a->M + BM - 1) / BM; p.tiles_n = (a->N + BN - 1) / BN;
    p.ksplit = pl.ksplit; p.k_per_split = pl.k_per_split;
    p.order = 0;
    p.colsum_a = a->colsum_a;
    p.row_scale = a->row_scale;
    p.slab = pl.slab_bytes ? a->workspace : nullptr;      // (a split without a slab: f32 atomics into C)

    // the instantiations: every split launch is <float, ATOMIC, ACCUM> (partial tiles); else the plan's specialised mask or -1
    const bool f32 = pl.out_f32;
    const int E = pl.epi;
    int rc;
    if (ta && tb) {
        if (pl.atomic) rc = launch<true, true, float, true, E_ACC>(p, pl, *a, s);
        else if (f32 && E == 0) rc = launch<true, true, float, false, 0>(p, pl, *a, s);
        else if (f32 && E == E_ACC) rc = launch<true, true, float, false, E_ACC>(p, pl, *a, s);
        else if (f32) rc = launch<true, true, float, false>(p, pl, *a, s);
        else rc = launch<true, true, bf16, false>(p, pl, *a, s);
    } else if (tb) {
        if (pl.atomic) rc = launch<false, true, float, true, E_ACC>(p, pl, *a, s);
        else if (f32) rc = launch<false, true, float, false>(p, pl, *a, s);
        else if (E == 0) rc = launch<false, true, bf16, false, 0>(p, pl, *a, s);
        else if (E == E_DG) rc = launch<false, true, bf16, false, E_DG>(p, pl, *a, s);
        else rc = launch<false, true, bf16, false>(p, pl, *a, s);
    } else {
        if (pl.atomic) rc = launch<false, false, float, true, E_ACC>(p, pl, *a, s);
        else if (f32 && E == 0) rc = launch<false, false, float, false, 0>(p, pl, *a, s);
        else if (f32 && E == E_B) rc = launch<false, false, float, false, E_B>(p, pl, *a, s);
        else if (f32 && E == E_BR) rc = launch<false, false, float, false, E_BR>(p, pl, *a, s);
        else if (f32 && E == E_BP) rc = launch<false, false, float, false, E_BP>(p, pl, *a, s);
        else if (f32) rc = launch<false, false, float, false>(p, pl, *a, s);
        else if (E == 0) rc = launch<false, false, bf16, false, 0>(p, pl, *a, s);
        else if (E == E_B) rc = launch<false, false, bf16, false, E_B>(p, pl, *a, s);
        else if (E == E_BGS) rc = launch<false, false, bf16, false, E_BGS>(p, pl, *a, s);
        else if (E == E_BG) rc = launch<false, false, bf16, false, E_BG>(p, pl, *a, s);
        else rc = launch<false, false, bf16, false>(p, pl, *a, s);
    }
    if (rc != GV_OK || pl.after == AFTER_NONE) return rc;
    if (pl.after == AFTER_REDUCE) return launch_splitk_reduce((const float*)p.slab, *a, p.ksplit, s, "gv_linear(splitk_reduce)");
    return launch_splitk_epilogue((const float*)p.slab, *a, p.ksplit, s);
}

extern "C" int gv_linear_dw_group(const gv_linear_dw_group_args* a, void* stream) {
    DwGroupPlan pl;
    if (int rc = checked_group_plan(a, &pl)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int S = pl.ksplit;
    double flops = 0, bytes = 0;
    for (int q = 0; q < a->n; ++q) {
        const auto& pr = a->prob[q];
        flops += 2.0 * pr.M * pr.N * a->K; bytes += 2.0 * a->K * ((double)pr.M + pr.N) + 8.0 * pr.M * pr.N;
    }
    long slab_floats = 0;
    if (pl.family == DW8_GROUP) {      // the ping-pong kernel (gemm_dw8.h): every problem tiles into 128 x 384 pieces
        Dw8GroupP G8{};
        for (int q = 0; q < a->n; ++q) {
            const auto& pr = a->prob[q];
            Dw8P& d = G8.prob[q];
            d.P = (const bf16*)pr.dY; d.ldp = pr.ldy; d.Pn = pr.M; d.Q = (const bf16*)pr.X; d.ldq = pr.ldx; d.Qn = pr.N;
            d.K = a->K; d.tiles_p = pr.M / DW8_P; d.tiles_q = pr.N / DW8_Q; d.ksplit = S; d.k_per_split = pl.k_per_split;
            d.slab = a->workspace + slab_floats; d.colsum = pr.colsum_dy;
            slab_floats += (long)S * pr.M * pr.N;
        }
        fill_tile_base(G8, a->n, [&](int q) { return G8.prob[q].tiles_p * G8.prob[q].tiles_q; });
        static GvLdsOptIn opt_in8;
        if (int rc = gv_lds_opt_in(opt_in8, (const void*)dw8_group_kernel, DW8_LDS, "gv_linear_dw_group")) return rc;
        const int th = gvtime::enabled() ? gvtime::begin(group_kernel_name(pl), flops, bytes, s) : -1;
        hipLaunchKernelGGL(dw8_group_kernel, dim3(pl.total_tiles * S), dim3(512), DW8_LDS, s, G8);
        gvtime::end(th, s);
        GV_LAUNCH_CHECK("gv_linear_dw_group(dw8)");
        return launch_group_reduce(*a, S, s, "gv_linear_dw_group(dw8 reduce)");
    }
    GV_REQUIRE(pl.slab_bytes <= a->workspace_bytes, GV_E_SHAPE, "gv_linear_dw_group: workspace too small (%ld bytes needed)", (long)pl.slab_bytes);
    GroupP G{};
    for (int q = 0; q < a->n; ++q) {
        const auto& pr = a->prob[q];
        GemmP& p = G.prob[q];
        p.A = (const bf16*)pr.dY; p.B = (const bf16*)pr.X; p.C = pr.dW;
        p.M = pr.M; p.N = pr.N; p.K = a->K; p.lda = pr.ldy; p.ldb = pr.ldx; p.ldc = pr.ldw;
        p.epi = GV_EPI_ACCUM; p.bias = nullptr; p.resid = nullptr; p.ldr = 0; p.aux_in = nullptr; p.ld_aux = 0; p.aux_out = nullptr;
        p.pos = nullptr; p.P = 0; p.alpha = 1.f;
        p.tiles_m = (pr.M + BM - 1) / BM; p.tiles_n = (pr.N + BN - 1) / BN;
        p.order = 0; p.colsum_a = pr.colsum_dy; p.row_scale = nullptr;
        p.k_per_split = pl.k_per_split; p.ksplit = S;
        p.slab = a->workspace + slab_floats;
        slab_floats += (long)S * p.M * p.N;
    }
    fill_tile_base(G, a->n, [&](int q) { return G.prob[q].tiles_m * G.prob[q].tiles_n; });
    static GvLdsOptIn opt_in;
    if (int rc = gv_lds_opt_in(opt_in, (const void*)gemm_dw_group_kernel, PCfg::LDS, "gv_linear_dw_group")) return rc;
    const int th = gvtime::enabled() ? gvtime::begin(group_kernel_name(pl), flops, bytes, s) : -1;
    hipLaunchKernelGGL(gemm_dw_group_kernel, dim3(pl.total_tiles * S), dim3(PCfg::THREADS), PCfg::LDS, s, G);
    gvtime::end(th, s);
    GV_LAUNCH_CHECK("gv_linear_dw_group");
    return launch_group_reduce(*a, S, s, "gv_linear_dw_group(reduce)");
}
