// Streaming attention probabilities for sequences past one workgroup's LDS (N <= GV_ATTN_STREAM_MAX_N, head_dim 64):
// gv_attention_probs without the sequence resident, so that attention maps exist for tiles up to 512 px (1 025 tokens).  It reads the
// packed qkv and the lse that gv_attention_fwd_stream left; P = exp(scale q.k - lse[q]) is attn_probs_tile.h's, the expression of
// gv_attention_probs -- given the same lse the two calls write the same bits.
//
// Row form (q_rows <= PROBS_ROW_Q, the CLS row): a GEMV per (image, head) pair that reads every K element once, straight from
// global.  The pair's 16-key tiles are dealt to the workgroup's waves in chunks; the loads of a chunk are issued before its first
// MFMA.  No LDS, no barrier.
//
// Block form (more rows): a workgroup = one pair x one block of GV_ATTN_STREAM_QBLOCK query rows -- 4 waves of 32 queries, Q
// fragments (and the rows' lse) in registers.  K passes through LDS in 64-key blocks, double buffered by LDS-DMA with ONE barrier per
// key block, as attn_fwd_stream_kernel stages it.  There is no V, no row reduction and no running state: each 16 x 16 tile is stored
// as soon as its two MFMAs are done.  Only the query blocks that hold a row < q_rows are launched.
//
// Plain launches: no atomics, nothing shared between workgroups.
#include "gv_common.h"
#include "attn_plan.h"    // ProbsStreamCfg: both forms' workgroup shape, LDS and launch geometry
#include <type_traits>

namespace {

#include "attn_tiles.h"
#include "attn_probs_tile.h"

using C = gvattn::ProbsStreamCfg;

__global__ __launch_bounds__(C::ROW_THREADS, C::ROW_OCC) void attn_probs_stream_row_kernel(gv_attention_probs_args a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N, H = a.H;
    const long ld = 3L * H * 64, pair = blockIdx.x;
    const int img = (int)(pair / H), h = (int)(pair - (long)img * H);
    const bf16* qbase = (const bf16*)a.qkv + (long)img * N * ld + h * 64;
    const int li = lane & 15, g = lane >> 4;
    const int nkt = (N + 15) >> 4;
    if (wave * C::ROW_CH >= nkt) return;                       // a short sequence leaves waves without a chunk
    const ProbsRows t = probs_rows(a, qbase, ld, pair, 0, li, g);
    for (int kt0 = wave * C::ROW_CH; kt0 < nkt; kt0 += C::ROW_NW * C::ROW_CH) {
        // key rows >= N are read as row N - 1 (in bounds) and never stored
        bf16x8 kreg[C::ROW_CH][2];
#pragma unroll
        for (int j = 0; j < C::ROW_CH; ++j) {
            int key = (kt0 + j) * 16 + li;
            key = key < N ? key : N - 1;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) kreg[j][ks] = *(const bf16x8*)(qbase + H * 64 + (long)key * ld + ks * 32 + g * 8);
        }
#pragma unroll
        for (int j = 0; j < C::ROW_CH; ++j) probs_keys(t, N, (kt0 + j) * 16, li, kreg[j][0], kreg[j][1]);
    }
}

constexpr int PQT = C::QB / (16 * C::NW);        // 16-query tiles per wave
constexpr int PKT = C::KB / 16;                  // 16-key tiles per key block

__global__ __launch_bounds__(C::THREADS, C::OCC) void attn_probs_stream_kernel(gv_attention_probs_args a, int nqb) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    GV_LDS char* const smem = (GV_LDS char*)smem_raw;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N, H = a.H;
    const long ld = 3L * H * 64;
    // query blocks of one pair are neighbours in the grid: they read the same K while it is hot in L2
    const int pair = blockIdx.x / nqb, qb = blockIdx.x - pair * nqb;
    const int img = pair / H, h = pair - img * H;
    const bf16* base = (const bf16*)a.qkv + (long)img * N * ld + h * 64;
    const int nkb = (N + C::KB - 1) / C::KB;
    const int li = lane & 15, g = lane >> 4;

    auto stage = [&](int kb) {
        const int k0 = kb * C::KB;
        stage_rows(base + H * 64 + (long)k0 * ld, ld, N - k0, C::KB, smem + (kb & 1) * C::IMG, wave, C::NW, lane);
    };
    stage(0);

    // a wave whose 32 rows all lie behind q_rows (last query block) stages and meets the barriers, nothing else
    const int q0 = qb * C::QB + wave * (16 * PQT);
    const bool live = q0 < a.q_rows;
    ProbsRows t[PQT];
    if (live) {
#pragma unroll
        for (int qt = 0; qt < PQT; ++qt) t[qt] = probs_rows(a, base, ld, pair, q0 + qt * 16, li, g);
    }

    for (int kb = 0; kb < nkb; ++kb) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kb + 1 < nkb) stage(kb + 1);
        if (!live) continue;
        GV_LDS char* const Kimg = smem + (kb & 1) * C::IMG;
#pragma unroll
        for (int kt = 0; kt < PKT; ++kt) {
            const bf16x8 k0 = read_nat(Kimg, kt * 16 + li, g), k1 = read_nat(Kimg, kt * 16 + li, 4 + g);
#pragma unroll
            for (int qt = 0; qt < PQT; ++qt) probs_keys(t[qt], N, kb * C::KB + kt * 16, li, k0, k1);
        }
    }
}

}  // namespace

extern "C" int gv_attention_probs_stream(const gv_attention_probs_args* a, void* stream) {
    if (int rc = attn_check("gv_attention_probs_stream", a, a && a->qkv && a->lse && a->p, GV_ATTN_STREAM_MAX_N, true)) return rc;
    GV_REQUIRE(a->q_rows >= 1 && a->q_rows <= a->N, GV_E_SHAPE, "gv_attention_probs_stream: need 1 <= q_rows <= N (got q_rows = %d, N = %d)", a->q_rows, a->N);
    // the lse this call reads is the streaming forward's, which needs scale > 0
    GV_REQUIRE(a->scale > 0.f, GV_E_SHAPE, "gv_attention_probs_stream: scale must be > 0 (got %g)", (double)a->scale);
    if (int rc = attn_aligned("gv_attention_probs_stream", "qkv", {a->qkv})) return rc;
    const gvattn::Launch l = C::launch(a->n_img, a->H, a->q_rows);
    GV_REQUIRE(l.grid <= 0x7fffffffL, GV_E_SHAPE, "gv_attention_probs_stream: n_img * H * query blocks = %ld exceeds the grid", l.grid);
    if (C::by_row(a->q_rows)) {
        hipLaunchKernelGGL(attn_probs_stream_row_kernel, dim3((unsigned)l.grid), dim3(l.block), 0, (hipStream_t)stream, *a);
    } else {
        static GvLdsOptIn opt_in;
        if (int rc = gv_lds_opt_in(opt_in, (const void*)attn_probs_stream_kernel, l.lds_bytes, "gv_attention_probs_stream")) return rc;
        hipLaunchKernelGGL(attn_probs_stream_kernel, dim3((unsigned)l.grid), dim3(l.block), l.lds_bytes, (hipStream_t)stream, *a,
                           C::query_blocks(a->q_rows));
    }
    GV_LAUNCH_CHECK("gv_attention_probs_stream");
    return GV_OK;
}
