// What the attention-MIL probe (mil.hip) and the survival probe (survival.hip) share: the launch parameters, the bag test, the gate
// and update kernels, the block reductions, the two halves every pool kernel has (bag_softmax_pool: scores, softmax and z;
// bag_score_grad: from a vector to ds and dbw), the argument and Adam checks, the workspace layout and the step driver's pieces
// (mil_set_step, mil_each_group, the gate and update launches).  A head's own file keeps its pool kernel's middle (logits and
// loss, or the risk), its other launches and its entry points.  See mil.hip for the step.
#pragma once
#include "gv_common.h"
#include <math.h>

namespace {

constexpr int MT = 64, MBK = 64, MLD = 80;           // row tile, k step, operand image row stride (80 mod 32 = 16)
constexpr int MNA = MBK / 16, MNB = MBK / 32;
constexpr int MFS = 32, MBLD = 48;                   // update: columns of F per workgroup, their image's row stride
constexpr int MCH = 32, MMAXCH = 8;                  // hidden units per gate workgroup; chunks at L = 256
constexpr int MMAXC = 32, MMAXF = 4096, MMAXL = 256, MMAXBAG = 4096, MMAXBATCH = 64;

struct MilP {
    const float* x; long ldx;
    const int* bag_ptr; const int* labels; const int* bags;
    const float* time; const int* event;      // the survival probe's per-bag time and event flag (NULL in the MIL probe)
    int off, m;               // this step's bags: bags[off .. off + m)  (bags NULL: bag off + j)
    int N, F, L, C, n_all, max_bag, nch;
    float *P, *Pm, *Pv;       // packed parameters and moments
    long oWc, oB;             // offsets: Wc; bv | bu | w | bc | bw
    float *T, *G, *SP, *DS, *Z, *DL, *LOSS, *DBW, *WS;      // workspace
    float *EV;                // survival probe: the step's event count, written by its Cox launch
    float *prob, *loss, *attn, *score;
    int accumulate, need_label;
    float step_size, rsq_bc2, wd, beta1, beta2, eps;        // lr lr_scale / (1 - beta1^t), 1 / sqrt(1 - beta2^t)
};

// bag j of the step: its first row, row count and label; false for a bad bag (nothing of it is then used as an index)
__device__ __forceinline__ bool mil_bag(const MilP& p, int j, int& start, int& n, int& y) {
    start = 0; n = 0; y = -1;
    if (j < 0 || j >= p.m) return false;
    const int bag = p.bags ? p.bags[p.off + j] : p.off + j;
    if (bag < 0 || bag >= p.n_all) return false;
    const int s = p.bag_ptr[bag], e = p.bag_ptr[bag + 1];
    if (s < 0 || e > p.N || e <= s || e - s > p.max_bag) return false;
    if (p.labels) {
        const int lab = p.labels[bag];
        if (lab >= 0 && lab < p.C) y = lab;
    }
    if (p.need_label && y < 0) return false;
    if (p.time) {                                    // survival: a time that is not finite or negative, a flag outside {0, 1}
        const float tm = p.time[bag];
        const int ev = p.event[bag];
        if (!(isfinite(tm) && tm >= 0.f) || (ev != 0 && ev != 1)) return false;
    }
    start = s; n = e - s;
    return true;
}

__device__ __forceinline__ float mil_pick(const f32x4& v, int e) { return e == 0 ? v[0] : e == 1 ? v[1] : e == 2 ? v[2] : v[3]; }

__device__ __forceinline__ void mil_adam(const MilP& p, long o, float grad) {
    const float w = p.P[o];
    const float g = grad + p.wd * w;
    const float m = p.beta1 * p.Pm[o] + (1.f - p.beta1) * g;
    const float v = p.beta2 * p.Pv[o] + (1.f - p.beta2) * g * g;
    p.Pm[o] = m;
    p.Pv[o] = v;
    p.P[o] = w - p.step_size * (m / (sqrtf(v) * p.rsq_bc2 + p.eps));
}

// (a) 64 rows of one bag against 32 rows of V and the same 32 of U
template <bool TRAIN>
__global__ __launch_bounds__(256) void mil_gate_kernel(MilP p) {
    __shared__ __attribute__((aligned(16))) float sm[2 * MBK * MLD];
    float* As = sm;
    float* Bs = sm + MBK * MLD;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, g = lane >> 4;
    const int F = p.F, L = p.L;
    const int j0 = blockIdx.x * MT, b = blockIdx.y, l0 = blockIdx.z * MCH;
    int start, n, y;
    if (!mil_bag(p, b, start, n, y) || j0 >= n) return;                // (uniform: a bad bag, a tile past the bag's end)
    // a thread loads MNA 16-byte pieces of feature row (t >> 2) and of weight row (t >> 2): k quads (t & 3) + 4 jj
    const int lrow = t >> 2, lq = t & 3;
    const float* xp = j0 + lrow < n ? p.x + (long)(start + j0 + lrow) * p.ldx : nullptr;
    const int wl = l0 + (lrow & 31);                                   // columns 0..31: V rows, 32..63: the same rows of U
    const float* wp = wl < L ? p.P + (long)((lrow < 32 ? 0 : L) + wl) * F : nullptr;
    f32x4 ra[MNA], rb[MNA];
    auto load = [&](int k0) {
#pragma unroll
        for (int jj = 0; jj < MNA; ++jj) {
            const int k = k0 + (lq + 4 * jj) * 4;
            ra[jj] = (xp && k < F) ? *(const f32x4*)(xp + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            rb[jj] = (wp && k < F) ? *(const f32x4*)(wp + k) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store = [&](float* S, const f32x4 (&v)[MNA]) {                // k-major image S[k][row], rotated as in linprobe.hip
#pragma unroll
        for (int jj = 0; jj < MNA; ++jj)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = (i + lq) & 3;
                S[((lq + 4 * jj) * 4 + e) * MLD + lrow] = mil_pick(v[jj], e);
            }
    };
    f32x4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    load(0);
    for (int k0 = 0; k0 < F; k0 += MBK) {
        __syncthreads();
        store(As, ra);
        store(Bs, rb);
        __syncthreads();
        if (k0 + MBK < F) load(k0 + MBK);
        // 32 products are one fmaf chain from zero, the chains are then added in order (as in linprobe.hip)
#pragma unroll
        for (int kc = 0; kc < MBK / 32; ++kc) {
            f32x4 part[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) part[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = kc * 8; kk < kc * 8 + 8; ++kk) {
                const float af = As[(kk * 4 + g) * MLD + wave * 16 + li];
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
                    part[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, Bs[(kk * 4 + g) * MLD + cb * 16 + li], part[cb], 0, 0, 0);
            }
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) acc[cb] += part[cb];
        }
    }
    // accumulator fragment: row 4g + r of the wave's 16, column cb * 16 + li: blocks 0, 1 are V's units, 2, 3 the same units of U
    const float* bv = p.P + p.oB;
    const float* bu = bv + L;
    const float* w = bu + L;
    float sc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int l = l0 + cb * 16 + li;
        if (l >= L) continue;
        const float bvl = bv[l], bul = bu[l], wl_ = w[l];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + wave * 16 + g * 4 + r;
            const float tv = tanhf(acc[cb][r] + bvl);
            const float gv = 1.f / (1.f + expf(-(acc[cb + 2][r] + bul)));
            sc[r] = fmaf(wl_, tv * gv, sc[r]);
            if (TRAIN && j < n) {
                const long o = ((long)b * p.max_bag + j) * L + l;
                p.T[o] = tv;
                p.G[o] = gv;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                    // the chunk's share of the score: a fixed tree over the 16 lanes of a row
        float s = sc[r];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const int j = j0 + wave * 16 + g * 4 + r;
        if (li == 0 && j < n) p.SP[((long)b * p.max_bag + j) * MMAXCH + blockIdx.z] = s;
    }
}

__device__ __forceinline__ float mil_block_sum(float v, float* red, int t) {       // a fixed tree over the 256 threads
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ float mil_block_max(float v, float* red, int t) {
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] = fmaxf(red[t], red[t + o]);
        __syncthreads();
    }
    return red[0];
}

// (b), the front of a pool kernel, one workgroup of 256 per good bag: the scores (the gate's partials added in chunk order, plus
// bw), a_i = softmax over the bag's own rows, left in sS, and z = sum_i a_i x_i, left in sZ.  Predict stores score / attn where
// they are asked for, training stores z.  LDS: sS [MMAXBAG], sZ [MMAXF] and zpart [4 * 256] 16-byte aligned, red [256].
template <bool TRAIN>
__device__ __forceinline__ void bag_softmax_pool(const MilP& p, int b, int start, int n, float bw, float* sS, float* sZ, float* zpart,
                                                 float* red) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int F = p.F;
    const long slot0 = (long)b * p.max_bag;
    float mx = -INFINITY;
    for (int i = t; i < n; i += 256) {
        float s = bw;
        for (int ch = 0; ch < p.nch; ++ch) s += p.SP[(slot0 + i) * MMAXCH + ch];
        sS[i] = s;
        mx = fmaxf(mx, s);
        if (!TRAIN && p.score) p.score[start + i] = s;
    }
    mx = mil_block_max(mx, red, t);
    float ps = 0.f;
    for (int i = t; i < n; i += 256) {               // rows past the bag are not in the sum
        const float e = expf(sS[i] - mx);
        sS[i] = e;
        ps += e;
    }
    const float den = mil_block_sum(ps, red, t);
    for (int i = t; i < n; i += 256) {
        const float a = sS[i] / den;
        sS[i] = a;
        if (!TRAIN && p.attn) p.attn[start + i] = a;
    }
    __syncthreads();
    // z = sum_i a_i x_i: 256 columns at a time, wave w the rows w, w + 4, .. in order, the four waves' sums then added in order
    for (int c0 = 0; c0 < F; c0 += 256) {
        const int col = c0 + lane * 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (col < F) {
            const float* xp = p.x + (long)start * p.ldx + col;
#pragma unroll 4
            for (int i = wave; i < n; i += 4) {
                const f32x4 xv = *(const f32x4*)(xp + (long)i * p.ldx);
                const float a = sS[i];
                acc[0] = fmaf(a, xv[0], acc[0]); acc[1] = fmaf(a, xv[1], acc[1]);
                acc[2] = fmaf(a, xv[2], acc[2]); acc[3] = fmaf(a, xv[3], acc[3]);
            }
        }
        *(f32x4*)(zpart + wave * 256 + lane * 4) = acc;
        __syncthreads();
        if (c0 + t < F) sZ[c0 + t] = ((zpart[t] + zpart[256 + t]) + zpart[512 + t]) + zpart[768 + t];
        __syncthreads();
    }
    if (TRAIN)
        for (int f = t; f < F; f += 256) p.Z[(long)b * F + f] = sZ[f];
}

// (b), the back of a training pool kernel: with a vector d in sZ (its stores fenced by the caller's barrier), sV[i] = d . x_i
// per row (sV [MMAXBAG]), then ds_i = a_i (sV[i] - sum_j a_j sV[j]) into DS and their sum into DBW[b]
__device__ __forceinline__ void bag_score_grad(const MilP& p, int b, int start, int n, const float* sS, float* sV, const float* sZ, float* red) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int F = p.F;
    const long slot0 = (long)b * p.max_bag;
    for (int i = wave; i < n; i += 4) {
        const float* xp = p.x + (long)(start + i) * p.ldx;
        float acc = 0.f;
        for (int f = lane * 4; f < F; f += 256) {
            const f32x4 xv = *(const f32x4*)(xp + f);
            acc = fmaf(sZ[f], xv[0], acc); acc = fmaf(sZ[f + 1], xv[1], acc);
            acc = fmaf(sZ[f + 2], xv[2], acc); acc = fmaf(sZ[f + 3], xv[3], acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) sV[i] = acc;
    }
    __syncthreads();
    float pd = 0.f;
    for (int i = t; i < n; i += 256) pd = fmaf(sS[i], sV[i], pd);
    const float dot = mil_block_sum(pd, red, t);
    float pb = 0.f;
    for (int i = t; i < n; i += 256) {
        const float ds = sS[i] * (sV[i] - dot);
        p.DS[slot0 + i] = ds;
        pb += ds;
    }
    const float dbw = mil_block_sum(pb, red, t);
    if (t == 0) p.DBW[b] = dbw;
}

// (c) the weight gradients of one (F slice, hidden block) and their Adam step.  SURV (survival.hip): C = 1, DL[b] is the Cox
// d theta_b, a step without an event changes nothing, the risk bias gets a gradient of exactly zero (the partial likelihood does
// not depend on it) and loss_sum[1] counts the events.
template <bool SURV>
__global__ __launch_bounds__(256) void mil_update_kernel(MilP p) {
    __shared__ __attribute__((aligned(16))) float As[MBK * MLD];          // [k = row of the step][hidden column of the block]
    __shared__ __attribute__((aligned(16))) float Bs[MBK * MBLD];         // [k][column of the slice]
    __shared__ int sst[MMAXBATCH], sn[MMAXBATCH];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, g = lane >> 4;
    const int F = p.F, L = p.L, C = p.C, m = p.m;
    if (t < MMAXBATCH) { int s_, n_, y_; mil_bag(p, t, s_, n_, y_); sst[t] = s_; sn[t] = n_; }
    __syncthreads();
    int good = 0;
    for (int j = 0; j < MMAXBATCH; ++j) good += sn[j] > 0;
    if (good == 0) return;                           // a step without a good bag changes nothing
    if (SURV && p.EV[0] == 0.f) return;
    const int f0 = blockIdx.x * MFS;
    const int ny = (3 * L + MT - 1) / MT;
    if ((int)blockIdx.y == ny) {
        // dWc = sum_b dl_b z_b^T for the slice, bags in order
        for (int i = 0; i < 4; ++i) {
            const int idx = t + 256 * i, c = idx >> 5, f = f0 + (idx & 31);
            if (c >= C || f >= F) continue;
            float acc = 0.f;
            for (int b = 0; b < m; ++b)
                if (sn[b] > 0) acc = fmaf(p.DL[b * MMAXC + c], p.Z[(long)b * F + f], acc);
            mil_adam(p, p.oWc + (long)c * F + f, acc);
        }
        if (blockIdx.x == 0) {
            if (t < C) {
                float s = 0.f;
                for (int b = 0; b < m; ++b)
                    if (sn[b] > 0) s += p.DL[b * MMAXC + t];
                mil_adam(p, p.oB + 3 * L + t, SURV ? 0.f : s);
            } else if (t == 64) {
                float s = 0.f;
                for (int b = 0; b < m; ++b)
                    if (sn[b] > 0) s += p.DBW[b];
                mil_adam(p, p.oB + 3 * L + C, s);
            } else if (t == 128) {
                float s = p.loss[0];
                for (int b = 0; b < m; ++b)
                    if (sn[b] > 0) s += p.LOSS[b];
                p.loss[0] = s;
            } else if (SURV && t == 192) {
                p.loss[1] += p.EV[0];
            }
        }
        return;
    }
    const int c0 = blockIdx.y * MT;                  // the block's first column of [dt (L) | dg (L) | du (L)]
    const bool gemm = c0 < 2 * L, sums = blockIdx.x == 0;
    if (!gemm && !sums) return;
    // this thread's pieces of the hidden image: rows (t >> 4) + 16 jj of a k step, columns c0 + 4 (t & 15) .. + 3 (one kind: L is
    // a multiple of 16)
    const int ak = t >> 4, acol = c0 + (t & 15) * 4;
    const int kind = acol < L ? 0 : acol < 2 * L ? 1 : acol < 3 * L ? 2 : 3;
    const int al = acol - kind * L;
    const f32x4 w4 = kind < 3 ? *(const f32x4*)(p.WS + al) : f32x4{0.f, 0.f, 0.f, 0.f};
    const int bk = t >> 3, bcol = f0 + (t & 7) * 4;
    f32x4 ra[MNA], rb[MNB];
    auto load = [&](int b, int j0) {
        const int n = sn[b];
#pragma unroll
        for (int jj = 0; jj < MNA; ++jj) {
            const int j = j0 + ak + 16 * jj;
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            if (kind < 3 && j < n) {
                const long slot = (long)b * p.max_bag + j;
                const f32x4 tv = *(const f32x4*)(p.T + slot * L + al), gv = *(const f32x4*)(p.G + slot * L + al);
                const float ds = p.DS[slot];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    o[e] = kind == 0 ? ds * w4[e] * gv[e] * (1.f - tv[e] * tv[e])
                         : kind == 1 ? ds * w4[e] * tv[e] * gv[e] * (1.f - gv[e])
                                     : ds * tv[e] * gv[e];
            }
            ra[jj] = o;
        }
        if (gemm) {
#pragma unroll
            for (int jj = 0; jj < MNB; ++jj) {
                const int j = j0 + bk + 32 * jj;
                rb[jj] = (j < n && bcol < F) ? *(const f32x4*)(p.x + (long)(sst[b] + j) * p.ldx + bcol) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    // the k steps: good bags in step order, 64 rows at a time
    auto next = [&](int& b, int& j0) {
        if (b >= 0) {
            j0 += MBK;
            if (j0 < sn[b]) return true;
        }
        for (++b; b < m; ++b)
            if (sn[b] > 0) { j0 = 0; return true; }
        return false;
    };
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const bool live = c0 + wave * 16 < 2 * L;        // this wave's 16 hidden columns are rows of V or U
    float cs = 0.f;
    int b = -1, j0 = 0;
    bool have = next(b, j0);
    if (have) load(b, j0);
    while (have) {
        __syncthreads();                             // the previous step's fragment reads are done
#pragma unroll
        for (int jj = 0; jj < MNA; ++jj) *(f32x4*)(As + (ak + 16 * jj) * MLD + (t & 15) * 4) = ra[jj];
        if (gemm) {
#pragma unroll
            for (int jj = 0; jj < MNB; ++jj) *(f32x4*)(Bs + (bk + 32 * jj) * MBLD + (t & 7) * 4) = rb[jj];
        }
        __syncthreads();
        have = next(b, j0);
        if (have) load(b, j0);
        if (gemm && live) {
#pragma unroll
            for (int kk = 0; kk < MBK / 4; ++kk) {
                const float af = As[(kk * 4 + g) * MLD + wave * 16 + li];
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
                    acc[jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, Bs[(kk * 4 + g) * MBLD + jb * 16 + li], acc[jb], 0, 0, 0);
            }
        }
        if (sums && t < MT)                          // the image's column sums, rows in order: dbv | dbu | dw
            for (int k = 0; k < MBK; ++k) cs += As[k * MLD + t];
    }
    // accumulator fragment: row (= hidden column) 4g + r of the wave's block, column li
    if (gemm && live) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int hc = c0 + wave * 16 + g * 4 + r;
            if (hc >= 2 * L) continue;
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const int f = f0 + jb * 16 + li;
                if (f < F) mil_adam(p, (long)hc * F + f, acc[jb][r]);
            }
        }
    }
    if (sums && t < MT && c0 + t < 3 * L) mil_adam(p, p.oB + c0 + t, cs);
}

int mil_check_shape(const char* who, int batch, int max_bag, int L, int C, int F) {
    GV_REQUIRE(F >= 4 && F % 4 == 0 && F <= MMAXF, GV_E_SHAPE, "%s: need F a multiple of 4, 4 <= F <= %d (got %d)", who, MMAXF, F);
    GV_REQUIRE(L >= 16 && L % 16 == 0 && L <= MMAXL, GV_E_SHAPE, "%s: need L a multiple of 16, 16 <= L <= %d (got %d)", who, MMAXL, L);
    GV_REQUIRE(C >= 1 && C <= MMAXC, GV_E_SHAPE, "%s: need 1 <= C <= %d (got %d)", who, MMAXC, C);
    GV_REQUIRE(batch >= 1 && batch <= MMAXBATCH, GV_E_SHAPE, "%s: need 1 <= batch <= %d (got %d)", who, MMAXBATCH, batch);
    GV_REQUIRE(max_bag >= 1 && max_bag <= MMAXBAG, GV_E_SHAPE, "%s: need 1 <= max_bag <= %d (got %d)", who, MMAXBAG, max_bag);
    return GV_OK;
}

// workspace, in floats: T [R, L] | G [R, L] | SP [R, 8] | DS [R] | Z [batch, F] | DL [batch, 32] | LOSS [batch] | DBW [batch] | WS [256]
// with R = batch * max_bag rounded up to a multiple of 4 (every part starts 16-byte aligned: batch is padded to 64 in the small ones)
struct MilWs { int64_t T, G, SP, DS, Z, DL, LOSS, DBW, WS, total; };
MilWs mil_workspace(int batch, int max_bag, int L, int F) {
    const int64_t R = ((int64_t)batch * max_bag + 3) / 4 * 4;
    MilWs w;
    w.T = 0;
    w.G = w.T + R * L;
    w.SP = w.G + R * L;
    w.DS = w.SP + R * MMAXCH;
    w.Z = w.DS + R;
    w.DL = w.Z + (int64_t)batch * F;
    w.LOSS = w.DL + (int64_t)MMAXBATCH * MMAXC;
    w.DBW = w.LOSS + MMAXBATCH;
    w.WS = w.DBW + MMAXBATCH;
    w.total = w.WS + MMAXL;
    return w;
}

// wsfn: the function that tells this caller's workspace size, named in the two workspace messages
int mil_check_common(const char* who, const char* wsfn, const float* x, int64_t ldx, int F, int N, int n_all, int n_bags, const void* params,
                     const void* ws, int64_t have, int64_t need) {
    GV_REQUIRE(N >= 1 && n_all >= 1 && n_bags >= 1, GV_E_SHAPE, "%s: need N >= 1, n_all_bags >= 1 and n_bags >= 1 (got N = %d, n_all_bags = %d, n_bags = %d)",
               who, N, n_all, n_bags);
    GV_REQUIRE(ldx >= F, GV_E_SHAPE, "%s: need ldx >= F (got ldx = %lld, F = %d)", who, (long long)ldx, F);
    GV_REQUIRE(ldx % 4 == 0, GV_E_ALIGN, "%s: ldx must be a multiple of 4 (got %lld)", who, (long long)ldx);
    GV_REQUIRE(gv_aligned(x, 16), GV_E_ALIGN, "%s: x must be 16-byte aligned", who);
    GV_REQUIRE(gv_aligned(params, 16), GV_E_ALIGN, "%s: params must be 16-byte aligned", who);
    GV_REQUIRE(ws, GV_E_NULL, "%s: null workspace (%lld bytes needed, %s)", who, (long long)need, wsfn);
    GV_REQUIRE(have >= need, GV_E_SHAPE, "%s: workspace of %lld bytes, %lld needed (%s)", who, (long long)have, (long long)need, wsfn);
    GV_REQUIRE(gv_aligned(ws, 16), GV_E_ALIGN, "%s: workspace must be 16-byte aligned", who);
    return GV_OK;
}

int mil_check_adam(const char* who, const float* m, const float* v, int step0, float lr, float lr_scale, float wd, float beta1, float beta2,
                   float eps) {
    GV_REQUIRE(gv_aligned(m, 16) && gv_aligned(v, 16), GV_E_ALIGN, "%s: m and v must be 16-byte aligned", who);
    GV_REQUIRE(step0 >= 0, GV_E_SHAPE, "%s: need step0 >= 0 (got %d)", who, step0);
    GV_REQUIRE(isfinite(lr) && lr > 0.f, GV_E_SHAPE, "%s: need lr finite and > 0 (got %g)", who, (double)lr);
    GV_REQUIRE(isfinite(lr_scale) && lr_scale >= 0.f, GV_E_SHAPE, "%s: need lr_scale finite and >= 0 (got %g)", who, (double)lr_scale);
    GV_REQUIRE(isfinite(wd) && wd >= 0.f, GV_E_SHAPE, "%s: need wd finite and >= 0 (got %g)", who, (double)wd);
    GV_REQUIRE(beta1 >= 0.f && beta1 < 1.f, GV_E_SHAPE, "%s: need 0 <= beta1 < 1 (got %g)", who, (double)beta1);
    GV_REQUIRE(beta2 >= 0.f && beta2 < 1.f, GV_E_SHAPE, "%s: need 0 <= beta2 < 1 (got %g)", who, (double)beta2);
    GV_REQUIRE(isfinite(eps) && eps > 0.f, GV_E_SHAPE, "%s: need eps finite and > 0 (got %g)", who, (double)eps);
    return GV_OK;
}

// Adam step `step` (1-based): the bias corrections in double (beta as the float the kernel multiplies by)
void mil_set_step(MilP& p, float lr, float lr_scale, float beta1, float beta2, int64_t step) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    p.step_size = (float)((double)lr * (double)lr_scale / (bc1 > 0.0 ? bc1 : 1.0));
    p.rsq_bc2 = (float)(1.0 / sqrt(bc2 > 0.0 ? bc2 : 1.0));
}

// predict: groups of at most 64 bags share the workspace
int mil_predict_group(int n_bags) { return n_bags < MMAXBATCH ? (n_bags < 1 ? 1 : n_bags) : MMAXBATCH; }

// the bags [0, n_bags) of a call in groups of `batch` (the last group takes the bags that are left): p.off and p.m, then launch()
template <class Fn>
void mil_each_group(MilP& p, int n_bags, int batch, Fn launch) {
    for (int s0 = 0; s0 < n_bags; s0 += batch) {
        p.off = s0;
        p.m = n_bags - s0 < batch ? n_bags - s0 : batch;
        launch();
    }
}

template <bool TRAIN>
void mil_launch_gate(const MilP& p, void* stream) {
    hipLaunchKernelGGL(mil_gate_kernel<TRAIN>, dim3((unsigned)((p.max_bag + MT - 1) / MT), (unsigned)p.m, (unsigned)p.nch), dim3(256), 0,
                       (hipStream_t)stream, p);
}

// (c)'s grid: 32-column slices of F by the 64-column blocks of [dt | dg | du] and one more row for dWc, the biases and the loss
template <bool SURV>
void mil_launch_update(const MilP& p, void* stream) {
    const int ny = (3 * p.L + MT - 1) / MT;
    hipLaunchKernelGGL(mil_update_kernel<SURV>, dim3((unsigned)((p.F + MFS - 1) / MFS), (unsigned)(ny + 1)), dim3(256), 0, (hipStream_t)stream, p);
}

void mil_fill(MilP& p, const float* x, int64_t ldx, const int* bag_ptr, const int* labels, const int* bags, int N, int F, int L, int C,
              int n_all, int max_bag, float* params, void* workspace, const MilWs& w) {
    p.x = x; p.ldx = (long)ldx; p.bag_ptr = bag_ptr; p.labels = labels; p.bags = bags;
    p.N = N; p.F = F; p.L = L; p.C = C; p.n_all = n_all; p.max_bag = max_bag; p.nch = (L + MCH - 1) / MCH;
    p.P = params;
    p.oWc = (long)2 * L * F;
    p.oB = (long)(2 * L + C) * F;
    float* ws = (float*)workspace;
    p.T = ws + w.T; p.G = ws + w.G; p.SP = ws + w.SP; p.DS = ws + w.DS; p.Z = ws + w.Z; p.DL = ws + w.DL; p.LOSS = ws + w.LOSS;
    p.DBW = ws + w.DBW; p.WS = ws + w.WS;
}

}  // namespace
