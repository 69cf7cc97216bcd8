// Linear probe on frozen features (gv_linprobe_train / gv_linprobe_predict): DINO's eval_linear as a grid of H linear heads
// trained in one pass over the feature bank -- every head shares one read of every feature row.
//   z[h, j, c] = b[h, c] + sum_f W[h, c, f] x[r_j, f];  p = softmax_c(z);  g = (p - onehot(y_j)) / m
//   dW = g^T x + wd W;  mW = mu mW + dW;  W -= lr[h] lr_scale mW       (same for b): torch.optim.SGD(momentum, weight_decay)
// A step is two launches, every dependency a launch boundary (no grid barrier, no atomics):
//   lp_fwd_kernel     one workgroup per 64 minibatch rows: the rows are gathered through `rows`, the [64, H C] logits come off the
//                     f32 MFMA (v_mfma_f32_16x16x4_f32, k-major LDS operand images as in knn.hip, row stride 80: lane groups of a
//                     fragment read hit 32 different banks), then one thread per (row, head) does the softmax; g goes to the
//                     workspace with the tile's column sums of g and its per-head loss sums.
//   lp_update_kernel  one workgroup per 32 columns of F: dW = g^T x for its slice over all m rows (g rows and gathered x rows ARE the
//                     k-major operand images), momentum update in the epilogue -- dW never reaches HBM.  Workgroup 0 also sums the
//                     tiles' partials in tile order: the bias update and loss_sum.
// Every sum has a fixed order that does not depend on the grid: a logit is the in-order sum of its 32-product fmaf chains, a dW
// element one fmaf chain in minibatch order, the partials are per 64-row tile whatever the launch looks like.  The result,
// loss_sum included, is bitwise the same run to run.
// Loads are bounds-checked by construction: a padded lane (row >= m, k >= F, column >= H C, a row index outside [0, N), k-step
// rows past the minibatch) is zero-filled in BOTH operands, never read.  A label outside [0, C) is never used as an index: its
// row contributes nothing.
#include "gv_common.h"
#include <math.h>

namespace {

constexpr int LT = 64, LBK = 64, LLD = 80;          // row tile, k step, operand image row stride (80 mod 32 = 16)
constexpr int LNA = LBK / 16, LNB = LBK / 32;        // 16-byte pieces per thread of a 64-wide / a 32-wide k-step image
constexpr int LHC = 64, LZ = LHC + 1;                // H C limit = logit tile width; logit tile row stride (lane = row: 32 banks)
constexpr int LFS = 32, LBLD = 48;                   // update: columns of F per workgroup, their image's row stride (48 mod 32 = 16)
constexpr int LMAXC = 32, LMAXF = 4096, LMAXM = 4096;
constexpr int LPART = 2 * LHC;                       // floats per row tile: 64 column sums of g, then up to 64 per-head loss sums

struct LpP {
    const float* x; long ldx;
    const int* labels;        // may be NULL (predict without a loss)
    const int* rows;          // this step's row indices; NULL: row j of the launch is row row0 + j
    int row0, m, N, F, H, C, HC, n_tiles;
    float *W, *b, *mW, *mb;
    const float *lr, *wd;
    float lr_scale, mu, inv_m;
    float *G, *part;          // workspace: g [n_tiles * 64, 64], partials [n_tiles, 128]
    float *prob, *loss;       // predict: [Q, H C] and [H]; train: loss = loss_sum
    int accumulate;           // predict's loss: add to what is there (chunks after the first)
};

__device__ __forceinline__ float lp_pick(const f32x4& v, int e) { return e == 0 ? v[0] : e == 1 ? v[1] : e == 2 ? v[2] : v[3]; }

// (a) logits, softmax, g / probabilities and the tile's partial sums
template <bool TRAIN>
__global__ __launch_bounds__(256) void lp_fwd_kernel(LpP p) {
    __shared__ __attribute__((aligned(16))) float sm[2 * LBK * LLD];      // operand images; after the k loop the (row, head) losses
    __shared__ float Z[LT * LZ];
    __shared__ int srow[LT], slab[LT];
    float* As = sm;
    float* Bs = sm + LBK * LLD;
    float* Ls = sm;                                                      // [64][65] <= 2 * LBK * 80
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, g = lane >> 4;
    const int F = p.F, HC = p.HC, C = p.C;
    const int j0 = blockIdx.x * LT;
    if (t < LT) {
        const int j = j0 + t;
        int r = -1, y = -1;
        if (j < p.m) {
            r = p.rows ? p.rows[j] : p.row0 + j;
            if (r < 0 || r >= p.N) r = -1;
            else if (p.labels) { y = p.labels[r]; if (y < 0 || y >= C) y = -1; }
        }
        srow[t] = r;
        slab[t] = y;
    }
    __syncthreads();
    // a thread loads LNA 16-byte pieces of feature row (t >> 2) and of weight row (t >> 2): k quads (t & 3) + 4 jj
    const int lrow = t >> 2, lq = t & 3;
    const float* xp = srow[lrow] >= 0 ? p.x + (long)srow[lrow] * p.ldx : nullptr;
    const float* wp = lrow < HC ? p.W + (long)lrow * F : nullptr;
    f32x4 ra[LNA], rb[LNA];
    auto load = [&](int k0) {
#pragma unroll
        for (int jj = 0; jj < LNA; ++jj) {
            const int k = k0 + (lq + 4 * jj) * 4;
            ra[jj] = (xp && k < F) ? *(const f32x4*)(xp + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            rb[jj] = (wp && k < F) ? *(const f32x4*)(wp + k) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    // k-major image S[k][row]; the four elements of a piece go out rotated by lq, so the 32 lanes of a store group (8 rows x 4
    // quads) spread over 16 banks, two lanes each (a 2-way store conflict costs nothing) instead of 8 banks, four lanes each
    auto store = [&](float* S, const f32x4 (&v)[LNA]) {
#pragma unroll
        for (int jj = 0; jj < LNA; ++jj)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = (i + lq) & 3;
                S[((lq + 4 * jj) * 4 + e) * LLD + lrow] = lp_pick(v[jj], e);
            }
    };
    const int ncb = (HC + 15) >> 4;                  // 16-column blocks that hold a head
    f32x4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    load(0);
    for (int k0 = 0; k0 < F; k0 += LBK) {
        __syncthreads();                             // the previous step's fragment reads are done
        store(As, ra);
        store(Bs, rb);
        __syncthreads();
        if (k0 + LBK < F) load(k0 + LBK);            // next tile's loads fly under this tile's MFMAs
        // 32 products are one fmaf chain from zero, the chains are then added in order: F / 32 roundings at the logit's
        // magnitude instead of F (3840 features: a quarter of the rounding error of one long chain)
#pragma unroll
        for (int kc = 0; kc < LBK / 32; ++kc) {
            f32x4 part[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) part[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = kc * 8; kk < kc * 8 + 8; ++kk) {
                const float af = As[(kk * 4 + g) * LLD + wave * 16 + li];
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
                    if (cb < ncb) part[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, Bs[(kk * 4 + g) * LLD + cb * 16 + li], part[cb], 0, 0, 0);
            }
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) acc[cb] += part[cb];
        }
    }
    // park the logits (accumulator fragment: row 4g + r, column li) with the bias
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        const int col = cb * 16 + li;
        const float bias = col < HC ? p.b[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) Z[(wave * 16 + g * 4 + r) * LZ + col] = acc[cb][r] + bias;
    }
    __syncthreads();                                 // (also: every fragment read of sm is done, Ls may take its place)
    // one thread per (row, head): max-subtracted softmax over the head's C logits, in place
    {
        const int row = t & 63, y = slab[row];
        for (int h = t >> 6; h < p.H; h += 4) {
            float* z = Z + row * LZ + h * C;
            float mx = z[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) s += expf(z[c] - mx);
            const float loss = y >= 0 ? logf(s) - (z[y] - mx) : 0.f;
            for (int c = 0; c < C; ++c) {
                const float pc = expf(z[c] - mx) / s;
                z[c] = TRAIN ? (y >= 0 ? (pc - (c == y ? 1.f : 0.f)) * p.inv_m : 0.f) : pc;
            }
            Ls[row * LZ + h] = loss;
        }
    }
    __syncthreads();
    if (TRAIN) {
#pragma unroll 4
        for (int i = 0; i < LT * LHC / 256; ++i) {
            const int idx = t + 256 * i, row = idx >> 6, col = idx & 63;
            p.G[(long)(j0 + row) * LHC + col] = Z[row * LZ + col];          // rows >= m and columns >= H C are zeros
        }
    } else {
        for (int i = 0; i < LT * LHC / 256; ++i) {
            const int idx = t + 256 * i, row = idx >> 6, col = idx & 63;
            if (col < HC && j0 + row < p.m && srow[row] >= 0) p.prob[((long)p.row0 + j0 + row) * HC + col] = Z[row * LZ + col];
        }
    }
    if (t < LHC) {                                   // column sums of g over the tile's rows, in row order
        float s = 0.f;
        if (TRAIN)
            for (int row = 0; row < LT; ++row) s += Z[row * LZ + t];
        p.part[(long)blockIdx.x * LPART + t] = s;
    } else if (t < 2 * LHC) {                        // per-head loss sums, in row order
        const int h = t - LHC;
        float s = 0.f;
        if (h < p.H)
            for (int row = 0; row < LT; ++row) s += Ls[row * LZ + h];
        p.part[(long)blockIdx.x * LPART + t] = s;
    }
}

// (b) dW = g^T x for 32 columns of F over all m rows, momentum update in the epilogue; workgroup 0: bias and loss
__global__ __launch_bounds__(256) void lp_update_kernel(LpP p) {
    __shared__ __attribute__((aligned(16))) float As[LBK * LLD];          // [k = minibatch row][h c]
    __shared__ __attribute__((aligned(16))) float Bs[LBK * LBLD];         // [k = minibatch row][column of the slice]
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, g = lane >> 4;
    const int F = p.F, HC = p.HC, m = p.m;
    const int f0 = blockIdx.x * LFS;
    const int bk = t >> 3, bc = f0 + (t & 7) * 4;    // this thread's pieces of the x image: k-step rows bk + 32 jj, first column
    auto row_of = [&](int j) {
        if (j >= m) return -1;
        const int r = p.rows[j];
        return (r < 0 || r >= p.N) ? -1 : r;
    };
    f32x4 ra[LNA], rb[LNB];
    auto load = [&](int j0, const int (&r)[LNB]) {
#pragma unroll
        for (int jj = 0; jj < LNA; ++jj) {
            const int idx = t + 256 * jj, j = j0 + (idx >> 4);
            ra[jj] = j < m ? *(const f32x4*)(p.G + (long)j * LHC + (idx & 15) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int jj = 0; jj < LNB; ++jj)
            rb[jj] = (r[jj] >= 0 && bc < F) ? *(const f32x4*)(p.x + (long)r[jj] * p.ldx + bc) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const bool live = wave * 16 < HC;                // this wave's 16 rows of [H C] hold a head
    int r_next[LNB];                                 // row indices run one k step ahead of the rows themselves
#pragma unroll
    for (int jj = 0; jj < LNB; ++jj) r_next[jj] = row_of(bk + 32 * jj);
    load(0, r_next);
#pragma unroll
    for (int jj = 0; jj < LNB; ++jj) r_next[jj] = row_of(LBK + bk + 32 * jj);
    for (int j0 = 0; j0 < m; j0 += LBK) {
        __syncthreads();                             // the previous step's fragment reads are done
#pragma unroll
        for (int jj = 0; jj < LNA; ++jj) {
            const int idx = t + 256 * jj;
            *(f32x4*)(As + (idx >> 4) * LLD + (idx & 15) * 4) = ra[jj];
        }
#pragma unroll
        for (int jj = 0; jj < LNB; ++jj) *(f32x4*)(Bs + (bk + 32 * jj) * LBLD + (t & 7) * 4) = rb[jj];
        __syncthreads();
        if (j0 + LBK < m) {
            load(j0 + LBK, r_next);
#pragma unroll
            for (int jj = 0; jj < LNB; ++jj) r_next[jj] = row_of(j0 + 2 * LBK + bk + 32 * jj);
        }
        if (live) {
#pragma unroll
            for (int kk = 0; kk < LBK / 4; ++kk) {
                const float af = As[(kk * 4 + g) * LLD + wave * 16 + li];
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
                    acc[jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, Bs[(kk * 4 + g) * LBLD + jb * 16 + li], acc[jb], 0, 0, 0);
            }
        }
    }
    // accumulator fragment: row (= h c) 4g + r of the wave's block, column li
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int hc = wave * 16 + g * 4 + r;
        if (hc >= HC) continue;
        const int h = hc / p.C;
        const float wd = p.wd[h], step = p.lr[h] * p.lr_scale;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            const int f = f0 + jb * 16 + li;
            if (f >= F) continue;
            const long o = (long)hc * F + f;
            const float w = p.W[o];
            const float mom = p.mu * p.mW[o] + (acc[jb][r] + wd * w);
            p.mW[o] = mom;
            p.W[o] = w - step * mom;
        }
    }
    if (blockIdx.x == 0) {
        if (t < HC) {                                // bias: the tiles' column sums of g in tile order
            float s = 0.f;
            for (int i = 0; i < p.n_tiles; ++i) s += p.part[(long)i * LPART + t];
            const int h = t / p.C;
            const float bv = p.b[t];
            const float mom = p.mu * p.mb[t] + (s + p.wd[h] * bv);
            p.mb[t] = mom;
            p.b[t] = bv - p.lr[h] * p.lr_scale * mom;
        } else if (t >= LHC && t - LHC < p.H) {      // loss_sum: the tiles' loss sums in tile order
            float s = 0.f;
            for (int i = 0; i < p.n_tiles; ++i) s += p.part[(long)i * LPART + t];
            p.loss[t - LHC] += s;
        }
    }
}

// predict's loss: the tiles' loss sums of one chunk in tile order
__global__ __launch_bounds__(64) void lp_loss_kernel(LpP p) {
    const int h = threadIdx.x;
    if (h >= p.H) return;
    float s = 0.f;
    for (int i = 0; i < p.n_tiles; ++i) s += p.part[(long)i * LPART + LHC + h];
    p.loss[h] = p.accumulate ? p.loss[h] + s : s;
}

int lp_check_shape(const char* who, int M, int H, int C, int F) {
    GV_REQUIRE(C >= 1 && C <= LMAXC, GV_E_SHAPE, "%s: need 1 <= C <= %d (got %d)", who, LMAXC, C);
    GV_REQUIRE(H >= 1 && (int64_t)H * C <= LHC, GV_E_SHAPE, "%s: need H >= 1 and H * C <= %d (got H = %d, C = %d)", who, LHC, H, C);
    GV_REQUIRE(F >= 4 && F % 4 == 0 && F <= LMAXF, GV_E_SHAPE, "%s: need F a multiple of 4, 4 <= F <= %d (got %d)", who, LMAXF, F);
    GV_REQUIRE(M >= 1 && M <= LMAXM, GV_E_SHAPE, "%s: need 1 <= batch <= %d (got %d)", who, LMAXM, M);
    return GV_OK;
}

int64_t lp_workspace(int M) {
    const int64_t tiles = (M + LT - 1) / LT;
    return tiles * (LT * LHC + LPART) * 4;
}

int lp_check_x(const char* who, const float* x, int64_t ldx, int F) {
    GV_REQUIRE(ldx >= F, GV_E_SHAPE, "%s: need ldx >= F (got ldx = %lld, F = %d)", who, (long long)ldx, F);
    GV_REQUIRE(ldx % 4 == 0, GV_E_ALIGN, "%s: ldx must be a multiple of 4 (got %lld)", who, (long long)ldx);
    GV_REQUIRE(gv_aligned(x, 16), GV_E_ALIGN, "%s: x must be 16-byte aligned", who);
    return GV_OK;
}

int lp_check_workspace(const char* who, const void* ws, int64_t have, int64_t need) {
    GV_REQUIRE(ws, GV_E_NULL, "%s: null workspace (%lld bytes needed, gv_linprobe_workspace_bytes)", who, (long long)need);
    GV_REQUIRE(have >= need, GV_E_SHAPE, "%s: workspace of %lld bytes, %lld needed (gv_linprobe_workspace_bytes)", who, (long long)have,
               (long long)need);
    GV_REQUIRE(gv_aligned(ws, 16), GV_E_ALIGN, "%s: workspace must be 16-byte aligned", who);
    return GV_OK;
}

}  // namespace

extern "C" int64_t gv_linprobe_workspace_bytes(int32_t M, int32_t H, int32_t C, int32_t F) {
    if (lp_check_shape("gv_linprobe_workspace_bytes", M, H, C, F) != GV_OK) return -1;
    return lp_workspace(M);
}

extern "C" int gv_linprobe_train(const gv_linprobe_train_args* a, void* stream) {
    const char* who = "gv_linprobe_train";
    GV_REQUIRE(a && a->W && a->b && a->mW && a->mb && a->lr && a->wd && a->x && a->labels && a->rows && a->loss_sum, GV_E_NULL,
               "%s: null pointer (W, b, mW, mb, lr, wd, x, labels, rows and loss_sum are required)", who);
    int rc = lp_check_shape(who, a->batch, a->H, a->C, a->F);
    if (rc != GV_OK) return rc;
    GV_REQUIRE(a->N >= 1 && a->n_rows >= 1, GV_E_SHAPE, "%s: need N >= 1 and n_rows >= 1 (got N = %d, n_rows = %d)", who, a->N, a->n_rows);
    if ((rc = lp_check_x(who, a->x, a->ldx, a->F)) != GV_OK) return rc;
    GV_REQUIRE(gv_aligned(a->W, 16), GV_E_ALIGN, "%s: W must be 16-byte aligned", who);
    GV_REQUIRE(isfinite(a->lr_scale) && a->lr_scale >= 0.f, GV_E_SHAPE, "%s: need lr_scale finite and >= 0 (got %g)", who, (double)a->lr_scale);
    GV_REQUIRE(a->momentum >= 0.f && a->momentum < 1.f, GV_E_SHAPE, "%s: need 0 <= momentum < 1 (got %g)", who, (double)a->momentum);
    const int M = a->batch;
    if ((rc = lp_check_workspace(who, a->workspace, a->workspace_bytes, lp_workspace(M))) != GV_OK) return rc;
    LpP p = {};
    p.x = a->x; p.ldx = (long)a->ldx; p.labels = a->labels;
    p.N = a->N; p.F = a->F; p.H = a->H; p.C = a->C; p.HC = a->H * a->C;
    p.W = a->W; p.b = a->b; p.mW = a->mW; p.mb = a->mb; p.lr = a->lr; p.wd = a->wd;
    p.lr_scale = a->lr_scale; p.mu = a->momentum;
    p.G = (float*)a->workspace;
    p.part = p.G + (int64_t)((M + LT - 1) / LT) * LT * LHC;
    p.loss = a->loss_sum;
    for (int s0 = 0; s0 < a->n_rows; s0 += M) {      // the last step takes the rows that are left and averages over their count
        p.rows = a->rows + s0;
        p.m = a->n_rows - s0 < M ? a->n_rows - s0 : M;
        p.inv_m = 1.0f / (float)p.m;
        p.n_tiles = (p.m + LT - 1) / LT;
        hipLaunchKernelGGL(lp_fwd_kernel<true>, dim3((unsigned)p.n_tiles), dim3(256), 0, (hipStream_t)stream, p);
        hipLaunchKernelGGL(lp_update_kernel, dim3((unsigned)((p.F + LFS - 1) / LFS)), dim3(256), 0, (hipStream_t)stream, p);
    }
    GV_LAUNCH_CHECK(who);
    return GV_OK;
}

extern "C" int gv_linprobe_predict(const gv_linprobe_predict_args* a, void* stream) {
    const char* who = "gv_linprobe_predict";
    GV_REQUIRE(a && a->W && a->b && a->x && a->prob, GV_E_NULL, "%s: null pointer (W, b, x and prob are required)", who);
    GV_REQUIRE(!a->loss || a->labels, GV_E_NULL, "%s: null labels with a loss output (the loss is the sum of -log p[label])", who);
    GV_REQUIRE(a->Q >= 1, GV_E_SHAPE, "%s: need Q >= 1 (got %d)", who, a->Q);
    const int M = a->Q < LMAXM ? a->Q : LMAXM;       // chunks of at most 4096 rows share the workspace
    int rc = lp_check_shape(who, M, a->H, a->C, a->F);
    if (rc != GV_OK) return rc;
    if ((rc = lp_check_x(who, a->x, a->ldx, a->F)) != GV_OK) return rc;
    GV_REQUIRE(gv_aligned(a->W, 16), GV_E_ALIGN, "%s: W must be 16-byte aligned", who);
    if ((rc = lp_check_workspace(who, a->workspace, a->workspace_bytes, lp_workspace(M))) != GV_OK) return rc;
    LpP p = {};
    p.x = a->x; p.ldx = (long)a->ldx; p.labels = a->loss ? a->labels : nullptr;
    p.N = a->Q; p.F = a->F; p.H = a->H; p.C = a->C; p.HC = a->H * a->C;
    p.W = const_cast<float*>(a->W); p.b = const_cast<float*>(a->b);
    p.G = (float*)a->workspace;
    p.part = p.G + (int64_t)((M + LT - 1) / LT) * LT * LHC;
    p.prob = a->prob; p.loss = a->loss;
    for (int s0 = 0; s0 < a->Q; s0 += M) {
        p.row0 = s0;
        p.m = a->Q - s0 < M ? a->Q - s0 : M;
        p.n_tiles = (p.m + LT - 1) / LT;
        p.accumulate = s0 > 0;
        hipLaunchKernelGGL(lp_fwd_kernel<false>, dim3((unsigned)p.n_tiles), dim3(256), 0, (hipStream_t)stream, p);
        if (a->loss) hipLaunchKernelGGL(lp_loss_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p);
    }
    GV_LAUNCH_CHECK(who);
    return GV_OK;
}
