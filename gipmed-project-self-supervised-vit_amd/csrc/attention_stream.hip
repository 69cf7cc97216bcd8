// Streaming attention forward for sequences past one workgroup's LDS (N <= GV_ATTN_STREAM_MAX_N, head_dim 64): the forward of
// attention.hip with K / V passed through LDS in 64-key blocks and an online softmax, so that inference runs on tiles up to
// 512 px (1 025 tokens).  Its backward is attention_stream_bwd.hip (gv_attention_bwd_stream), which reads the o / lse left here.
//
// A workgroup = one (image, head) pair x one block of GV_ATTN_STREAM_QBLOCK = 128 query rows: 4 waves of 32 queries, Q fragments
// in registers.  K / V key blocks are double buffered in the swizzled image of attn_tiles.h, filled by LDS-DMA: block j + 1 is
// in flight while block j is computed, ONE barrier per key block (it says both "block j has landed" and "nobody reads the
// buffer block j + 1 goes to any more").  32 KB of LDS, 127 registers: four workgroups per CU cover each other's barriers.
//
// Per key block, as attn_fwd_body: S^T = K Q^T (keys on MFMA rows, queries on lanes), so a query's running max m, running sum l
// and its O^T column live in ITS lanes -- the rescale is in-lane:
//     m' = max(m, max_j s_j)            alpha = exp2((m - m') c)        (c = scale log2 e; alpha = 1 exactly when m stays)
//     p_j = exp2(s_j c - m' c)          l' = l alpha + sum_j p_j        (f32; l is a per-lane partial, summed over the 4 lane
//     O' = O alpha + V^T bf16(p)                                         groups once, at the end -- alpha is the same in all 4)
// Every block multiplies by alpha (there is no "max did not move" branch to get wrong), keys >= N of the last block score -inf,
// one division at the end, lse = m scale + log l.  No atomics, nothing shared between workgroups.
#include "gv_common.h"
#include "attn_plan.h"    // StreamCfg: the workgroup's shape, its LDS and the launch geometry
#include <type_traits>

namespace {

#include "attn_tiles.h"

using S = gvattn::StreamCfg;
constexpr int SQB = S::QB, SNW = S::NW, SKB = S::KB, SIMG = S::IMG;
constexpr int SQT = SQB / (16 * SNW);           // 16-query tiles per wave
constexpr int SKT = SKB / 16;                   // 16-key tiles per key block
static_assert(SQB % 32 == 0 && SQT == 2 && SKT % 2 == 0, "4 waves x 32 queries, 32-key P V slabs");

__global__ __launch_bounds__(S::THREADS, S::OCC) void attn_fwd_stream_kernel(gv_attention_fwd_args a, int nqb) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    GV_LDS char* const smem = (GV_LDS char*)smem_raw;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N, H = a.H;
    const long ld = 3L * H * 64;
    // query blocks of one pair are neighbours in the grid: they read the same K / V while it is hot in L2
    const int pair = blockIdx.x / nqb, qb = blockIdx.x - pair * nqb;
    const int img = pair / H, h = pair - img * H;
    const bf16* base = (const bf16*)a.qkv + (long)img * N * ld + h * 64;
    const int nkb = (N + SKB - 1) / SKB;
    const int li = lane & 15, g = lane >> 4, q4 = li >> 2, p4 = li & 3;
    const float c = a.scale * 1.4426950408889634f;

    auto stage = [&](int kb) {
        const int k0 = kb * SKB;
        GV_LDS char* buf = smem + (kb & 1) * 2 * SIMG;
        stage_rows(base + H * 64 + (long)k0 * ld, ld, N - k0, SKB, buf, wave, SNW, lane);
        stage_rows(base + 2 * H * 64 + (long)k0 * ld, ld, N - k0, SKB, buf + SIMG, wave, SNW, lane);
    };
    stage(0);

    // a wave whose 32 rows all lie behind N (last query block) stages and meets the barriers, nothing else
    const int q0 = qb * SQB + wave * (16 * SQT);
    const bool live = q0 < N;
    bf16x8 qf[SQT][2];
#pragma unroll
    for (int qt = 0; qt < SQT; ++qt) {
        int qrow = q0 + qt * 16 + li;
        qrow = qrow < N ? qrow : N - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[qt][ks] = *(const bf16x8*)(base + (long)qrow * ld + ks * 32 + g * 8);
    }
    float m[SQT], l[SQT];
    f32x4 o[4][SQT];
#pragma unroll
    for (int qt = 0; qt < SQT; ++qt) {
        m[qt] = -INFINITY; l[qt] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int kb = 0; kb < nkb; ++kb) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kb + 1 < nkb) stage(kb + 1);
        if (!live) continue;
        GV_LDS char* const Kimg = smem + (kb & 1) * 2 * SIMG;
        GV_LDS char* const Vimg = Kimg + SIMG;
        const int k0 = kb * SKB;
        f32x4 s[SKT][SQT];
#pragma unroll
        for (int kt = 0; kt < SKT; ++kt) {
#pragma unroll
            for (int qt = 0; qt < SQT; ++qt) s[kt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 kf = read_nat(Kimg, kt * 16 + li, ks * 4 + g);
#pragma unroll
                for (int qt = 0; qt < SQT; ++qt) s[kt][qt] = MFMA16(kf, qf[qt][ks], s[kt][qt]);
            }
        }
        // key = k0 + kt*16 + 4g + r lives in (kt, r) of lanes {li, li+16, li+32, li+48}; only the last block has keys >= N
        // (and its first key is < N: every block leaves a finite max)
        if (k0 + SKB > N) {
#pragma unroll
            for (int kt = 0; kt < SKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = k0 + kt * 16 + 4 * g + r < N;
#pragma unroll
                    for (int qt = 0; qt < SQT; ++qt) s[kt][qt][r] = ok ? s[kt][qt][r] : -INFINITY;
                }
        }
#pragma unroll
        for (int qt = 0; qt < SQT; ++qt) {
            float bm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < SKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) bm = fmaxf(bm, s[kt][qt][r]);
            bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
            bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
            const float mn = fmaxf(m[qt], bm);
            const float alpha = __builtin_amdgcn_exp2f((m[qt] - mn) * c);       // first block: exp2(-inf) = 0 on o = l = 0
            const float mxc = -mn * c;
            float bs = 0.f;
#pragma unroll
            for (int kt = 0; kt < SKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][qt][r], c, mxc));
                    s[kt][qt][r] = p;
                    bs += p;
                }
            l[qt] = fmaf(l[qt], alpha, bs);
            m[qt] = mn;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt][qt] *= alpha;
        }
        // keep the V reads of the P V phase behind the softmax: hoisted into it they cost 8 registers (135 instead of 127), i.e. the
        // fourth workgroup of a CU -- measured 728 -> 669 us at (256 images, 6 heads, 1 025 tokens)
        __builtin_amdgcn_sched_barrier(0);
        // O^T[d][q] += sum_key V[key][d] bf16(P^T[key][q])
#pragma unroll
        for (int u = 0; u < SKT / 2; ++u) {
            bf16x8 pf[SQT];
#pragma unroll
            for (int qt = 0; qt < SQT; ++qt) pf[qt] = pack8(s[2 * u][qt], s[2 * u + 1][qt]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const bf16x8 vf = cat8(read_tr(Vimg, (2 * u) * 16 + 4 * g + q4, dt, p4),
                                       read_tr(Vimg, (2 * u + 1) * 16 + 4 * g + q4, dt, p4));
#pragma unroll
                for (int qt = 0; qt < SQT; ++qt) o[dt][qt] = MFMA16(vf, pf[qt], o[dt][qt]);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int qt = 0; qt < SQT; ++qt) {
        float sum = l[qt];
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const int q = q0 + qt * 16 + li;
        if (q < N) {
            const float inv = 1.0f / sum;
            bf16* dst = (bf16*)a.o + ((long)img * N + q) * (H * 64) + h * 64 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *(bf16x4*)(dst + dt * 16) = bf16x4{(bf16)(o[dt][qt][0] * inv), (bf16)(o[dt][qt][1] * inv),
                                                   (bf16)(o[dt][qt][2] * inv), (bf16)(o[dt][qt][3] * inv)};
            if (g == 0) a.lse[((long)img * H + h) * N + q] = m[qt] * a.scale + __logf(sum);
        }
    }
}

}  // namespace

extern "C" int gv_attention_fwd_stream(const gv_attention_fwd_args* a, void* stream) {
    if (int rc = attn_check("gv_attention_fwd_stream", a, a && a->qkv && a->o && a->lse, GV_ATTN_STREAM_MAX_N, true)) return rc;
    // the running max is taken over the raw scores and alpha = exp2((-inf - m') c) must be 0 on the first block: both need c > 0
    GV_REQUIRE(a->scale > 0.f, GV_E_SHAPE, "gv_attention_fwd_stream: scale must be > 0 (got %g)", (double)a->scale);
    if (int rc = attn_aligned("gv_attention_fwd_stream", "qkv/o", {a->qkv, a->o})) return rc;
    const gvattn::Launch l = S::launch(a->n_img, a->H, a->N, a->q_limit);
    GV_REQUIRE(l.grid <= 0x7fffffffL, GV_E_SHAPE, "gv_attention_fwd_stream: n_img * H * query blocks = %ld exceeds the grid", l.grid);
    static GvLdsOptIn opt_in;
    if (int rc = gv_lds_opt_in(opt_in, (const void*)attn_fwd_stream_kernel, l.lds_bytes, "gv_attention_fwd_stream")) return rc;
    hipLaunchKernelGGL(attn_fwd_stream_kernel, dim3((unsigned)l.grid), dim3(l.block), l.lds_bytes, (hipStream_t)stream, *a, S::query_blocks(a->N, a->q_limit));
    GV_LAUNCH_CHECK("gv_attention_fwd_stream");
    return GV_OK;
}
