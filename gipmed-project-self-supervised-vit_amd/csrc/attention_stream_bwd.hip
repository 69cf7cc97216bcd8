// Streaming attention backward for sequences past one workgroup's LDS (N <= GV_ATTN_STREAM_MAX_N, head_dim 64): the backward of
// attention.hip on the o / lse that attention_stream.hip left, so that training runs on tiles up to 512 px (1 025 tokens).
//
// Two launches, both the streaming forward's body transposed (attn_tiles.h serves them; no tile crosses LDS to be transposed):
//
//   attn_bwd_stream_dq   a workgroup = one (image, head) pair x one block of 128 query rows, 4 waves of 32 queries.  Q and dO
//                        fragments in registers; delta[q] = sum_d dO[q][d] O[q][d] in-lane, summed over the 4 lane groups and stored
//                        for the second launch.  K / V key blocks double buffered by LDS-DMA, ONE barrier per block.  Per block
//                        S^T = K Q^T and dP^T = V dO^T (keys on MFMA rows, the query on the lane: lse / delta are per-lane scalars),
//                        dS^T = P^T (dP^T - delta) scale packed like the forward's P, dQ^T += K^T dS^T with K read transposed from the
//                        same image -- exactly where the forward reads V.  Writes the q third of dqkv.
//   attn_bwd_stream_dkv  a workgroup = one pair x one block of 128 keys, 4 waves of 32 keys.  K and V fragments in registers; blocks
//                        of 64 Q / dO rows with their lse / delta double buffered the same way.  Per 32 queries it is phase A of
//                        attn_bwd_kernel: S = Q K^T, dP = dO V^T (the key on the lane), dV^T += dO^T P, dK^T += Q^T dS with the
//                        staged Q / dO read transposed.  Writes the k and v thirds.
//
// Seven MFMA products where the fused backward has five; they buy a backward with no sum across workgroups: every dQ row and
// every dK / dV row is accumulated in f32 by ONE wave over all blocks and rounded once, at its store.  No atomics, nothing waits on
// another workgroup, the only dependency between workgroups (delta) is the launch boundary.  Rounding points are attn_bwd_kernel's.
#include "gv_common.h"
#include "attn_plan.h"    // StreamBwdCfg: both workgroup shapes, their LDS and the launch geometry
#include <type_traits>

namespace {

#include "attn_tiles.h"

using B = gvattn::StreamBwdCfg;
constexpr int NW = B::NW, QB = B::QB, KB = B::KB, IMG = B::IMG;
constexpr int KEYS = B::KEYS, QS = B::QS, QIMG = B::QIMG, STAGE = B::STAGE;
constexpr float LOG2E = 1.4426950408889634f;

// one 4-byte LDS-DMA per lane: 64 consecutive f32 land at dst (wave-uniform)
__device__ __forceinline__ void glds4(const void* src, GV_LDS char* dst) {
    __builtin_amdgcn_global_load_lds((const GV_GLOBAL void*)src, (GV_LDS void*)dst, 4, 0, 0);
}

// ---------------------------------------------------------------------------------
// launch 1: delta and dQ
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(B::THREADS, B::OCC_DQ) void attn_bwd_stream_dq_kernel(gv_attention_bwd_stream_args a, int nqb, int QE) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    GV_LDS char* const smem = (GV_LDS char*)smem_raw;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N, H = a.H;
    const long ld = 3L * H * 64, ldo = (long)H * 64;
    const int pair = blockIdx.x / nqb, qb = blockIdx.x - pair * nqb;
    const int img = pair / H, h = pair - img * H;
    const bf16* base = (const bf16*)a.qkv + (long)img * N * ld + h * 64;
    bf16* dq_base = (bf16*)a.dqkv + (long)img * N * ld + h * 64;

    // a query block behind q_limit: d_o is zero there, dQ = 0 (128 rows x 8 pieces of 16 bytes over 256 threads); nothing is read
    if (qb * QB >= QE) {
        for (int i = threadIdx.x; i < QB * 8; i += B::THREADS) {
            const int q = qb * QB + (i >> 3);
            if (q < N) *(bf16x8*)(dq_base + (long)q * ld + (i & 7) * 8) = bf16x8{};
        }
        return;
    }
    const int nkb = (N + KB - 1) / KB;
    const int li = lane & 15, g = lane >> 4, q4 = li >> 2, p4 = li & 3;
    const float c = a.scale * LOG2E;

    auto stage = [&](int kb) {
        const int k0 = kb * KB;
        GV_LDS char* buf = smem + (kb & 1) * 2 * IMG;
        stage_rows(base + H * 64 + (long)k0 * ld, ld, N - k0, KB, buf, wave, NW, lane);
        stage_rows(base + 2 * H * 64 + (long)k0 * ld, ld, N - k0, KB, buf + IMG, wave, NW, lane);
    };
    stage(0);

    // a wave whose 32 rows all lie behind N (last query block) stages and meets the barriers, nothing else.  Rows of a live block are
    // < QE wherever they are < N (QE is N or a multiple of the block), so the clamp to N - 1 keeps every read inside [0, QE)
    const int q0 = qb * QB + wave * 32;
    const bool live = q0 < N;
    bf16x8 qf[2][2], dof[2][2];
    float nl[2], nd[2];                 // -lse log2(e) and -delta scale of this lane's query
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + li;
        const int qrow = q < N ? q : N - 1;
        const bf16* orow = (const bf16*)a.o + ((long)img * N + qrow) * ldo + h * 64;
        const bf16* drow = (const bf16*)a.d_o + ((long)img * N + qrow) * ldo + h * 64;
        float d = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[qt][ks] = *(const bf16x8*)(base + (long)qrow * ld + ks * 32 + g * 8);
            dof[qt][ks] = *(const bf16x8*)(drow + ks * 32 + g * 8);
            const bf16x8 of = *(const bf16x8*)(orow + ks * 32 + g * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) d = fmaf((float)of[j], (float)dof[qt][ks][j], d);
        }
        d += __shfl_xor(d, 16, 64);
        d += __shfl_xor(d, 32, 64);
        const long row = ((long)img * H + h) * N + qrow;
        if (live && g == 0 && q < N) a.delta[row] = d;
        nl[qt] = -a.lse[row] * LOG2E;
        nd[qt] = -d * a.scale;
    }
    f32x4 dq[4][2];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) dq[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < nkb; ++kb) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kb + 1 < nkb) stage(kb + 1);
        if (!live) continue;
        GV_LDS char* const Kimg = smem + (kb & 1) * 2 * IMG;
        GV_LDS char* const Vimg = Kimg + IMG;
        const int k0 = kb * KB;
        // 32 keys at a time: the scores are not needed beyond their own dS (no running max), which keeps the registers of a slab
#pragma unroll
        for (int u = 0; u < KB / 32; ++u) {
            f32x4 s[2][2], dp[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) { s[t][qt] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[t][qt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 kf = read_nat(Kimg, (2 * u + t) * 16 + li, ks * 4 + g);
                    const bf16x8 vf = read_nat(Vimg, (2 * u + t) * 16 + li, ks * 4 + g);
#pragma unroll
                    for (int qt = 0; qt < 2; ++qt) {
                        s[t][qt] = MFMA16(kf, qf[qt][ks], s[t][qt]);
                        dp[t][qt] = MFMA16(vf, dof[qt][ks], dp[t][qt]);
                    }
                }
            }
            // P^T = exp(scale S^T - lse[q]); dS^T = P^T (dP^T - delta[q]) scale.  rows key = k0 + 32 u + 16 t + 4 g + r, col q = li
            bf16x8 sb[2];
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                f32x4 ds[2];
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool ok = k0 + (2 * u + t) * 16 + 4 * g + r < N;
                        const float p = ok ? __builtin_amdgcn_exp2f(fmaf(s[t][qt][r], c, nl[qt])) : 0.f;
                        ds[t][r] = p * fmaf(dp[t][qt][r], a.scale, nd[qt]);
                    }
                sb[qt] = pack8(ds[0], ds[1]);
            }
            // dQ^T[d][q] += sum_key K[key][d] dS^T[key][q]
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const bf16x8 ka = cat8(read_tr(Kimg, (2 * u) * 16 + 4 * g + q4, dt, p4),
                                       read_tr(Kimg, (2 * u + 1) * 16 + 4 * g + q4, dt, p4));
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) dq[dt][qt] = MFMA16(ka, sb[qt], dq[dt][qt]);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + li;
        if (q < N) {
            bf16* dst = dq_base + (long)q * ld + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *(bf16x4*)(dst + dt * 16) = bf16x4{(bf16)dq[dt][qt][0], (bf16)dq[dt][qt][1], (bf16)dq[dt][qt][2], (bf16)dq[dt][qt][3]};
        }
    }
}

// ---------------------------------------------------------------------------------
// launch 2: dK and dV
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(B::THREADS, B::OCC_DKV) void attn_bwd_stream_dkv_kernel(gv_attention_bwd_stream_args a, int nkb, int QE) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    GV_LDS char* const smem = (GV_LDS char*)smem_raw;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N, H = a.H;
    const long ld = 3L * H * 64, ldo = (long)H * 64;
    const int pair = blockIdx.x / nkb, kb = blockIdx.x - pair * nkb;
    const int img = pair / H, h = pair - img * H;
    const bf16* base = (const bf16*)a.qkv + (long)img * N * ld + h * 64;
    const bf16* dobase = (const bf16*)a.d_o + (long)img * N * ldo + h * 64;
    const float* lse = a.lse + ((long)img * H + h) * N;
    const float* delta = a.delta + ((long)img * H + h) * N;
    const int nqs = (QE + QS - 1) / QS;
    const int li = lane & 15, g = lane >> 4, q4 = li >> 2, p4 = li & 3;
    const float c = a.scale * LOG2E;

    // rows >= QE of a stage are zero filled and their lse / delta come from the zero page: they are never read from the caller's buffers
    auto stage = [&](int qs) {
        const int r0 = qs * QS;
        GV_LDS char* buf = smem + (qs & 1) * STAGE;
        stage_rows(base + (long)r0 * ld, ld, QE - r0, QS, buf, wave, NW, lane);
        stage_rows(dobase + (long)r0 * ldo, ldo, QE - r0, QS, buf + QIMG, wave, NW, lane);
        if (wave < 2) {
            const float* v = wave == 0 ? lse : delta;
            const int q = r0 + lane;
            glds4(q < QE ? (const void*)(v + q) : (const void*)attn_zero_page, buf + 2 * QIMG + wave * (QS * 4));
        }
    };
    stage(0);

    // this wave's K and V fragments (B operands: lane = key, 8 consecutive d); a wave whose keys all lie behind N only stages
    const int key0 = kb * KEYS + wave * 32;
    const bool live = key0 < N;
    bf16x8 kf[2][2], vf[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + kt * 16 + li;
        const bf16* krow = base + (long)(key < N ? key : N - 1) * ld + H * 64;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kf[kt][ks] = *(const bf16x8*)(krow + ks * 32 + g * 8);
            vf[kt][ks] = *(const bf16x8*)(krow + H * 64 + ks * 32 + g * 8);
        }
    }
    f32x4 dv[4][2], dk[4][2];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) { dv[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    for (int qs = 0; qs < nqs; ++qs) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (qs + 1 < nqs) stage(qs + 1);
        if (!live) continue;
        GV_LDS char* const Qimg = smem + (qs & 1) * STAGE;
        GV_LDS char* const Dimg = Qimg + QIMG;
        GV_LDS float* const lse_s = (GV_LDS float*)(Qimg + 2 * QIMG);
        GV_LDS float* const delta_s = lse_s + QS;
#pragma unroll
        for (int qc = 0; qc < QS / 32; ++qc) {
            if (qs * QS + qc * 32 >= QE) break;
            // S, dP for [32 q] x [this wave's 32 keys]
            f32x4 s[2][2], dp[2][2];
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const int qrow = qc * 32 + qt * 16 + li;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) { s[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 qa = read_nat(Qimg, qrow, ks * 4 + g);
                    const bf16x8 da = read_nat(Dimg, qrow, ks * 4 + g);
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt) {
                        s[qt][kt] = MFMA16(qa, kf[kt][ks], s[qt][kt]);
                        dp[qt][kt] = MFMA16(da, vf[kt][ks], dp[qt][kt]);
                    }
                }
            }
            // P = exp(scale S - lse[q]); dS = P (dP - delta[q]) scale.  rows q = 4 g + r, col key = li
            f32x4 pv[2][2], ds[2][2];
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const int ql = qc * 32 + qt * 16 + 4 * g;
                f32x4 l4 = *(GV_LDS f32x4*)(lse_s + ql), d4 = *(GV_LDS f32x4*)(delta_s + ql);
                l4 *= -LOG2E;
                d4 *= -a.scale;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    const bool kok = key0 + kt * 16 + li < N;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool ok = kok && (qs * QS + ql + r < QE);
                        const float p = ok ? __builtin_amdgcn_exp2f(fmaf(s[qt][kt][r], c, l4[r])) : 0.f;
                        pv[qt][kt][r] = p;
                        ds[qt][kt][r] = p * fmaf(dp[qt][kt][r], a.scale, d4[r]);
                    }
                }
            }
            // dV^T += dO^T P ; dK^T += Q^T dS   (reduction over the chunk's 32 queries)
            bf16x8 pb[2], sb[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) { pb[kt] = pack8(pv[0][kt], pv[1][kt]); sb[kt] = pack8(ds[0][kt], ds[1][kt]); }
            const int r0 = qc * 32 + 4 * g + q4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const bf16x8 dot = cat8(read_tr(Dimg, r0, dt, p4), read_tr(Dimg, r0 + 16, dt, p4));
                const bf16x8 qtt = cat8(read_tr(Qimg, r0, dt, p4), read_tr(Qimg, r0 + 16, dt, p4));
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    dv[dt][kt] = MFMA16(dot, pb[kt], dv[dt][kt]);
                    dk[dt][kt] = MFMA16(qtt, sb[kt], dk[dt][kt]);
                }
            }
        }
    }
    if (!live) return;
    // lane = key, rows d = 16 dt + 4 g + r
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + kt * 16 + li;
        if (key < N) {
            bf16* dst = (bf16*)a.dqkv + ((long)img * N + key) * ld + h * 64 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                *(bf16x4*)(dst + H * 64 + dt * 16) = bf16x4{(bf16)dk[dt][kt][0], (bf16)dk[dt][kt][1], (bf16)dk[dt][kt][2], (bf16)dk[dt][kt][3]};
                *(bf16x4*)(dst + 2 * H * 64 + dt * 16) = bf16x4{(bf16)dv[dt][kt][0], (bf16)dv[dt][kt][1], (bf16)dv[dt][kt][2], (bf16)dv[dt][kt][3]};
            }
        }
    }
}

}  // namespace

extern "C" int gv_attention_bwd_stream(const gv_attention_bwd_stream_args* a, void* stream) {
    const char* const name = "gv_attention_bwd_stream";
    if (int rc = attn_check(name, a, a && a->qkv && a->o && a->d_o && a->lse && a->dqkv && a->delta, GV_ATTN_STREAM_MAX_N, true)) return rc;
    GV_REQUIRE(a->scale > 0.f, GV_E_SHAPE, "gv_attention_bwd_stream: scale must be > 0 (got %g)", (double)a->scale);
    if (int rc = attn_aligned(name, "buffers", {a->qkv, a->o, a->d_o, a->dqkv})) return rc;
    const gvattn::Launch lq = B::launch_dq(a->n_img, a->H, a->N), lk = B::launch_dkv(a->n_img, a->H, a->N);
    GV_REQUIRE(lq.grid <= 0x7fffffffL && lk.grid <= 0x7fffffffL, GV_E_SHAPE, "gv_attention_bwd_stream: n_img * H * blocks = %ld exceeds the grid",
               lq.grid > lk.grid ? lq.grid : lk.grid);
    static GvLdsOptIn opt_dq, opt_dkv;
    if (int rc = gv_lds_opt_in(opt_dq, (const void*)attn_bwd_stream_dq_kernel, lq.lds_bytes, name)) return rc;
    if (int rc = gv_lds_opt_in(opt_dkv, (const void*)attn_bwd_stream_dkv_kernel, lk.lds_bytes, name)) return rc;
    const int QE = B::query_end(a->N, a->q_limit);
    hipLaunchKernelGGL(attn_bwd_stream_dq_kernel, dim3((unsigned)lq.grid), dim3(lq.block), lq.lds_bytes, (hipStream_t)stream, *a,
                       gvattn::ceil_div(a->N, B::QB), QE);
    GV_LAUNCH_CHECK(name);
    hipLaunchKernelGGL(attn_bwd_stream_dkv_kernel, dim3((unsigned)lk.grid), dim3(lk.block), lk.lds_bytes, (hipStream_t)stream, *a,
                       gvattn::ceil_div(a->N, B::KEYS), QE);
    GV_LAUNCH_CHECK(name);
    return GV_OK;
}
