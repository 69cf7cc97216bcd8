// The two loss-level terms of DINOv2 that need no change of architecture (include/gipvit.h has the contract):
//   * Sinkhorn-Knopp centring of the teacher, in the log domain.  Its result is handed to gv_dino_loss as the centre:
//     softmax((t - c) / tau) with c_k = -tau a_k IS the Sinkhorn-Knopp assignment, so only a = log u is computed here.
//   * the KoLeo regulariser on the student's CLS features of every global crop, forward and backward.
// Every dependency between workgroups is a launch boundary; there is no atomic and every sum has a fixed order, so both terms are
// bitwise the same run to run.  expf / logf / sqrtf and true divisions throughout: the Sinkhorn result feeds an exponent.
#include "gv_common.h"
#include <float.h>

namespace {

// ---------------------------------------------------------------------------------------------------------------- Sinkhorn-Knopp
constexpr int SK_NT = 256, SK_TILE = SK_NT * 4;     // threads, and columns (four per thread, one 16-B load), of a column workgroup
constexpr int SK_BLOCKS = 1024;                     // workgroups a pass aims for (four per CU)

__device__ __forceinline__ float sk_inv_tau(const gv_sinkhorn_args& a) { return 1.0f / (a.hyper ? a.hyper[GV_HYP_TEACHER_TEMP] : a.teacher_temp); }

// logit * (1 / tau), rounded on its own (as gv_dino_loss_f32 forms it): contracted into an FMA with the "- shift" that follows, the
// passes would each see a differently rounded exponent
__device__ __forceinline__ float sk_scaled(float t, float inv_t) {
#pragma clang fp contract(off)
    return t * inv_t;
}

// sum of the workgroup's values in a fixed order: lanes by butterfly, waves one after the other.  Valid in thread 0.
template <int NT> __device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < NT / 64; ++w) s += red[w];
    return s;
}

// rows [r0, r1) of the workgroup's slice, columns in 16-B pieces: the slice's largest raw logit -> partial[block]
__global__ __launch_bounds__(SK_NT) void sk_max_kernel(gv_sinkhorn_args a, long n4, float* partial) {
    __shared__ float red[SK_NT / 64];
    float m = -INFINITY;
    for (long i = (long)blockIdx.x * SK_NT + threadIdx.x; i < n4; i += (long)gridDim.x * SK_NT) {
        const f32x4 v = *(const f32x4*)(a.teacher + i * 4);
        m = fmaxf(m, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// shift = max(T) * (1 / tau): rounding is monotone and 1 / tau > 0, so this is the largest scaled logit as the passes form it
__global__ __launch_bounds__(SK_NT) void sk_max_final_kernel(gv_sinkhorn_args a, int n, const float* partial) {
    __shared__ float red[SK_NT / 64];
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += SK_NT) m = fmaxf(m, partial[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) a.shift[0] = sk_scaled(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), sk_inv_tau(a));
}

// grid (column tiles, row slices): out[slice, k] = sum over the slice's rows, in row order, of exp(T_rk / tau - shift + a_k + b_r)
__global__ __launch_bounds__(SK_NT) void sk_cols_kernel(gv_sinkhorn_args a, int r_per, float* out) {
    const int k = (blockIdx.x * SK_NT + threadIdx.x) * 4;
    if (k >= a.K) return;
    const int r0 = blockIdx.y * r_per, r1 = min(a.R, r0 + r_per);
    const float inv_t = sk_inv_tau(a), shift = a.shift[0];
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 ak = a.first ? zero : *(const f32x4*)(a.a + k);
    f32x4 s = zero;
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        const f32x4 t = *(const f32x4*)(a.teacher + (long)r * a.K + k);
        const float br = a.first ? 0.f : a.b[r];
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += expf(((sk_scaled(t[e], inv_t) - shift) + ak[e]) + br);
    }
    *(f32x4*)(out + (long)blockIdx.y * a.K + k) = s;
}

// colsum[k] = the slices' partial sums, added in slice order
__global__ __launch_bounds__(SK_NT) void sk_cols_combine_kernel(gv_sinkhorn_args a, int n_slices, const float* partial) {
    const int k = (blockIdx.x * SK_NT + threadIdx.x) * 4;
    if (k >= a.K) return;
    f32x4 s = *(const f32x4*)(partial + k);
    for (int y = 1; y < n_slices; ++y) s += *(const f32x4*)(partial + (long)y * a.K + k);
    *(f32x4*)(a.colsum + k) = s;
}

// a_k -= log(max(s_k, FLT_MIN)) (a_k = 0 before the first pass); with a centre to write, sk_center[k] = -tau a_k
__global__ __launch_bounds__(SK_NT) void sk_fold_kernel(gv_sinkhorn_args a, int finish) {
    const int k = (blockIdx.x * SK_NT + threadIdx.x) * 4;
    if (k >= a.K) return;
    const f32x4 s = *(const f32x4*)(a.colsum + k);
    f32x4 ak = a.first ? f32x4{0.f, 0.f, 0.f, 0.f} : *(const f32x4*)(a.a + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) ak[e] -= logf(fmaxf(s[e], FLT_MIN));
    *(f32x4*)(a.a + k) = ak;
    if (finish) {
        const float tau = a.hyper ? a.hyper[GV_HYP_TEACHER_TEMP] : a.teacher_temp;
        *(f32x4*)(a.sk_center + k) = f32x4{-tau * ak[0], -tau * ak[1], -tau * ak[2], -tau * ak[3]};
    }
}

// one workgroup per row: b_r = -log sum_k exp(T_rk / tau - shift + a_k)
template <int NT>
__global__ __launch_bounds__(NT) void sk_rows_kernel(gv_sinkhorn_args a) {
    __shared__ float red[NT / 64];
    const int row = blockIdx.x;
    const float* x = a.teacher + (long)row * a.K;
    const float inv_t = sk_inv_tau(a), shift = a.shift[0];
    float s = 0.f;
    for (int k = threadIdx.x * 4; k < a.K; k += NT * 4) {
        const f32x4 t = *(const f32x4*)(x + k);
        const f32x4 ak = *(const f32x4*)(a.a + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += expf((sk_scaled(t[e], inv_t) - shift) + ak[e]);
    }
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) a.b[row] = -logf(s);
}

// the column pass's geometry: row slices so that tiles x slices reaches SK_BLOCKS workgroups (64 tiles of 1024 columns at K = 65536
// would leave three quarters of the chip idle)
struct SkPlan { int ktiles, r_per, slices; };
SkPlan sk_plan(int R, int K) {
    SkPlan p;
    p.ktiles = (K + SK_TILE - 1) / SK_TILE;
    int slices = (SK_BLOCKS + p.ktiles - 1) / p.ktiles;
    if (slices > R) slices = R;
    p.r_per = (R + slices - 1) / slices;
    p.slices = (R + p.r_per - 1) / p.r_per;
    return p;
}

long sk_workspace_floats(int R, int K) {
    const SkPlan p = sk_plan(R, K);
    const long cols = p.slices > 1 ? (long)p.slices * K : 0;
    return cols > SK_BLOCKS ? cols : SK_BLOCKS;
}

bool sk_shape_ok(int R, int K) { return R >= 1 && R <= 65535 && K >= 4 && K % 4 == 0; }

// which: 0 shift, 1 cols, 2 rows, 3 finish
int sk_check(const gv_sinkhorn_args* a, const char* who, int which) {
    GV_REQUIRE(a, GV_E_NULL, "%s: null argument struct", who);
    GV_REQUIRE(a->teacher && a->shift && a->a && a->b && a->colsum && a->workspace, GV_E_NULL, "%s: null pointer", who);
    GV_REQUIRE(which != 3 || a->sk_center, GV_E_NULL, "%s: null pointer (sk_center)", who);
    GV_REQUIRE(sk_shape_ok(a->R, a->K), GV_E_SHAPE, "%s: need 1 <= R <= 65535 and K a positive multiple of 4 (got R=%d K=%d)", who, a->R, a->K);
    GV_REQUIRE(a->teacher_temp > 0.f, GV_E_SHAPE, "%s: the teacher temperature must be > 0", who);
    GV_REQUIRE(gv_aligned(a->teacher, 16) && gv_aligned(a->a, 16) && gv_aligned(a->colsum, 16) && gv_aligned(a->workspace, 16) &&
               (which != 3 || gv_aligned(a->sk_center, 16)), GV_E_ALIGN, "%s: teacher, a, colsum, sk_center and workspace must be 16-byte aligned", who);
    const long need = sk_workspace_floats(a->R, a->K) * 4;
    GV_REQUIRE(a->workspace_bytes >= need, GV_E_SHAPE, "%s: workspace of %lld bytes, %ld needed (gv_sinkhorn_workspace_bytes)", who,
               (long long)a->workspace_bytes, need);
    return GV_OK;
}

// ------------------------------------------------------------------------------------------------------------------------- KoLeo
constexpr int KL_NT = 256, KL_MAX_D = 768, KL_MAX_B = 1024, KL_MAX_G = 4;
constexpr float KL_EPS = 1e-8f;

struct KlWs { float* y; float* inv; float* dist; float* term; };
__host__ __device__ inline KlWs kl_ws(void* ws, int rows, int D) {
    KlWs w;
    w.y = (float*)ws;
    w.inv = w.y + (long)rows * D;
    w.dist = w.inv + rows;
    w.term = w.dist + rows;
    return w;
}
long kl_workspace_bytes(int G, int B, int D) { return (((long)G * B * (D + 3)) * 4 + 15) & ~15L; }

// one wave per row: y = x / max(||x||, eps), inv = 1 / max(||x||, eps)
template <typename T>
__global__ __launch_bounds__(KL_NT) void koleo_norm_kernel(gv_koleo_args a) {
    const int rows = a.G * a.B, row = blockIdx.x * (KL_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const KlWs w = kl_ws(a.workspace, rows, a.D);
    const T* x = (const T*)a.feats + (long)row * a.ld;
    float v[KL_MAX_D / 64], ss = 0.f;
#pragma unroll
    for (int c = 0; c < KL_MAX_D / 64; ++c) {
        v[c] = c * 64 < a.D ? (float)x[c * 64 + lane] : 0.f;
        ss += v[c] * v[c];
    }
    const float nrm = fmaxf(sqrtf(wave_sum(ss)), KL_EPS);
#pragma unroll
    for (int c = 0; c < KL_MAX_D / 64; ++c)
        if (c * 64 < a.D) w.y[(long)row * a.D + c * 64 + lane] = v[c] / nrm;
    if (lane == 0) w.inv[row] = 1.0f / nrm;
}

// one workgroup per row i: its four waves share the crop's other rows j, a wave keeps the best dot it meets going up (strictly
// greater replaces: the lowest index wins a tie), the waves' candidates are merged the same way; then delta_i = y_i - y_I + eps,
// d_i = ||delta_i|| and the row's loss term -log(d_i + eps)
__global__ __launch_bounds__(KL_NT) void koleo_nn_kernel(gv_koleo_args a) {
    __shared__ float best_v[KL_NT / 64], red[KL_NT / 64];
    __shared__ int best_j[KL_NT / 64];
    const int rows = a.G * a.B, row = blockIdx.x, g = row / a.B, i = row - g * a.B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const KlWs w = kl_ws(a.workspace, rows, a.D);
    const float* yc = w.y + (long)g * a.B * a.D;
    const float* yi = yc + (long)i * a.D;
    float v[KL_MAX_D / 64];
#pragma unroll
    for (int c = 0; c < KL_MAX_D / 64; ++c) v[c] = c * 64 < a.D ? yi[c * 64 + lane] : 0.f;
    float bv = -INFINITY;
    int bj = -1;
    for (int j = wave; j < a.B; j += KL_NT / 64) {
        if (j == i) continue;
        const float* yj = yc + (long)j * a.D;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < KL_MAX_D / 64; ++c)
            if (c * 64 < a.D) dot = fmaf(v[c], yj[c * 64 + lane], dot);
        dot = wave_sum(dot);
        if (dot > bv) { bv = dot; bj = j; }
    }
    if (lane == 0) { best_v[wave] = bv; best_j[wave] = bj; }
    __syncthreads();
    bv = -INFINITY; bj = -1;
    for (int q = 0; q < KL_NT / 64; ++q) {      // every thread merges the same way
        const float qv = best_v[q];
        const int qj = best_j[q];
        if (qj >= 0 && (bj < 0 || qv > bv || (qv == bv && qj < bj))) { bv = qv; bj = qj; }
    }
    const float* yn = yc + (long)bj * a.D;
    float ss = 0.f;
    for (int c = threadIdx.x; c < a.D; c += KL_NT) {
        const float d = (yi[c] - yn[c]) + KL_EPS;
        ss += d * d;
    }
    __syncthreads();                             // red is free: nothing else uses it before
    ss = block_sum<KL_NT>(ss, red);
    if (threadIdx.x == 0) {
        const float d = sqrtf(ss);
        a.nn[row] = bj;
        w.dist[row] = d;
        w.term[row] = -logf(d + KL_EPS);
    }
}

// koleo = sum over the crops, in order, of the mean of the crop's terms (each summed in a fixed order)
__global__ __launch_bounds__(KL_NT) void koleo_sum_kernel(gv_koleo_args a) {
    __shared__ float red[KL_NT / 64];
    const KlWs w = kl_ws(a.workspace, a.G * a.B, a.D);
    float total = 0.f;
    for (int g = 0; g < a.G; ++g) {
        float s = 0.f;
        for (int i = threadIdx.x; i < a.B; i += KL_NT) s += w.term[g * a.B + i];
        s = block_sum<KL_NT>(s, red);
        total += s / (float)a.B;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.koleo[0] = total;
}

// one workgroup per row i (a gather: no atomics): gy_i = -w_i delta_i + sum over the crop's rows i', in order, with I_i' = i of
// w_i' delta_i';  gx_i = (gy_i - y_i (y_i . gy_i)) / max(||x_i||, eps);  dfeats_i = round(float(dfeats_i) + scale gx_i)
template <typename T>
__global__ __launch_bounds__(KL_NT) void koleo_bwd_kernel(gv_koleo_args a) {
    __shared__ float red[KL_NT / 64];
    __shared__ float dot_all;
    const int rows = a.G * a.B, row = blockIdx.x, g = row / a.B, i = row - g * a.B;
    const KlWs w = kl_ws(a.workspace, rows, a.D);
    const float* yc = w.y + (long)g * a.B * a.D;
    const float* yi = yc + (long)i * a.D;
    const float invB = 1.0f / (float)a.B;
    constexpr int PER = KL_MAX_D / KL_NT;       // elements of the row per thread
    float y[PER], gy[PER];
    {
        const float d = w.dist[row];
        const float wi = invB / (d * (d + KL_EPS));
        const float* yn = yc + (long)min(max(a.nn[row], 0), a.B - 1) * a.D;      // never an index outside the crop, whatever nn holds
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int c = p * KL_NT + threadIdx.x;
            y[p] = c < a.D ? yi[c] : 0.f;
            gy[p] = c < a.D ? -wi * ((y[p] - yn[c]) + KL_EPS) : 0.f;
        }
    }
    for (int j = 0; j < a.B; ++j) {
        if (a.nn[g * a.B + j] != i) continue;   // uniform over the workgroup
        const float d = w.dist[g * a.B + j];
        const float wj = invB / (d * (d + KL_EPS));
        const float* yj = yc + (long)j * a.D;
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int c = p * KL_NT + threadIdx.x;
            if (c < a.D) gy[p] += wj * ((yj[c] - y[p]) + KL_EPS);
        }
    }
    float dot = 0.f;
#pragma unroll
    for (int p = 0; p < PER; ++p) dot += y[p] * gy[p];
    dot = block_sum<KL_NT>(dot, red);
    if (threadIdx.x == 0) dot_all = dot;
    __syncthreads();
    dot = dot_all;
    float scale = a.weight * w.inv[row];
    if (a.loss_scale) scale *= a.loss_scale[0];
    T* dst = (T*)a.dfeats + (long)row * a.ld;
#pragma unroll
    for (int p = 0; p < PER; ++p) {
        const int c = p * KL_NT + threadIdx.x;
        if (c < a.D) dst[c] = (T)((float)dst[c] + scale * (gy[p] - y[p] * dot));
    }
}

const char* kl_shape_error(int G, int B, int D) {
    if (G < 1 || G > KL_MAX_G) return "1 <= G <= 4";
    if (B < 2 || B > KL_MAX_B) return "2 <= B <= 1024";
    if (D < 64 || D > KL_MAX_D || D % 64) return "D a multiple of 64 up to 768";
    return nullptr;
}

int kl_check(const gv_koleo_args* a, const char* who, bool bwd, int elt) {
    GV_REQUIRE(a, GV_E_NULL, "%s: null argument struct", who);
    GV_REQUIRE(a->workspace && a->nn && (bwd ? a->dfeats != nullptr : (a->feats && a->koleo)), GV_E_NULL, "%s: null pointer", who);
    const char* bad = kl_shape_error(a->G, a->B, a->D);
    GV_REQUIRE(!bad, GV_E_SHAPE, "%s: need %s (got G=%d B=%d D=%d)", who, bad, a->G, a->B, a->D);
    GV_REQUIRE(a->ld >= a->D, GV_E_SHAPE, "%s: need ld >= D (got ld=%lld D=%d)", who, (long long)a->ld, a->D);
    GV_REQUIRE(gv_aligned(a->workspace, 16) && gv_aligned(bwd ? a->dfeats : a->feats, elt), GV_E_ALIGN, "%s: workspace must be 16-byte aligned", who);
    const long need = kl_workspace_bytes(a->G, a->B, a->D);
    GV_REQUIRE(a->workspace_bytes >= need, GV_E_SHAPE, "%s: workspace of %lld bytes, %ld needed (gv_koleo_workspace_bytes)", who,
               (long long)a->workspace_bytes, need);
    if (bwd) GV_REQUIRE(a->weight == a->weight && a->weight >= 0.f && a->weight <= FLT_MAX, GV_E_SHAPE, "%s: weight must be finite and >= 0", who);
    return GV_OK;
}

template <typename T> int koleo_fwd_launch(const gv_koleo_args* a, void* stream, const char* who) {
    const int rc = kl_check(a, who, false, sizeof(T));
    if (rc != GV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int rows = a->G * a->B;
    hipLaunchKernelGGL(koleo_norm_kernel<T>, dim3((rows + KL_NT / 64 - 1) / (KL_NT / 64)), dim3(KL_NT), 0, s, *a);
    GV_LAUNCH_CHECK("gv_koleo_fwd(norm)");
    hipLaunchKernelGGL(koleo_nn_kernel, dim3(rows), dim3(KL_NT), 0, s, *a);
    GV_LAUNCH_CHECK("gv_koleo_fwd(nn)");
    hipLaunchKernelGGL(koleo_sum_kernel, dim3(1), dim3(KL_NT), 0, s, *a);
    GV_LAUNCH_CHECK("gv_koleo_fwd(sum)");
    return GV_OK;
}

template <typename T> int koleo_bwd_launch(const gv_koleo_args* a, void* stream, const char* who) {
    const int rc = kl_check(a, who, true, sizeof(T));
    if (rc != GV_OK) return rc;
    hipLaunchKernelGGL(koleo_bwd_kernel<T>, dim3(a->G * a->B), dim3(KL_NT), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_koleo_bwd");
    return GV_OK;
}

}  // namespace

extern "C" int64_t gv_sinkhorn_workspace_bytes(int32_t R, int32_t K) {
    if (!sk_shape_ok(R, K)) { gv_set_error("gv_sinkhorn_workspace_bytes: need 1 <= R <= 65535 and K a positive multiple of 4 (got R=%d K=%d)", R, K); return -1; }
    return sk_workspace_floats(R, K) * 4;
}

extern "C" int gv_sinkhorn_shift(const gv_sinkhorn_args* a, void* stream) {
    const int rc = sk_check(a, "gv_sinkhorn_shift", 0);
    if (rc != GV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long n4 = (long)a->R * a->K / 4;
    long nb = (n4 + SK_NT * 4 - 1) / (SK_NT * 4);
    if (nb > SK_BLOCKS) nb = SK_BLOCKS;
    hipLaunchKernelGGL(sk_max_kernel, dim3((int)nb), dim3(SK_NT), 0, s, *a, n4, (float*)a->workspace);
    GV_LAUNCH_CHECK("gv_sinkhorn_shift(max)");
    hipLaunchKernelGGL(sk_max_final_kernel, dim3(1), dim3(SK_NT), 0, s, *a, (int)nb, (const float*)a->workspace);
    GV_LAUNCH_CHECK("gv_sinkhorn_shift(final)");
    return GV_OK;
}

extern "C" int gv_sinkhorn_cols(const gv_sinkhorn_args* a, void* stream) {
    const int rc = sk_check(a, "gv_sinkhorn_cols", 1);
    if (rc != GV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const SkPlan p = sk_plan(a->R, a->K);
    float* out = p.slices > 1 ? (float*)a->workspace : a->colsum;
    hipLaunchKernelGGL(sk_cols_kernel, dim3(p.ktiles, p.slices), dim3(SK_NT), 0, s, *a, p.r_per, out);
    GV_LAUNCH_CHECK("gv_sinkhorn_cols");
    if (p.slices > 1) {
        hipLaunchKernelGGL(sk_cols_combine_kernel, dim3(p.ktiles), dim3(SK_NT), 0, s, *a, p.slices, (const float*)a->workspace);
        GV_LAUNCH_CHECK("gv_sinkhorn_cols(combine)");
    }
    return GV_OK;
}

extern "C" int gv_sinkhorn_rows(const gv_sinkhorn_args* a, void* stream) {
    const int rc = sk_check(a, "gv_sinkhorn_rows", 2);
    if (rc != GV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sk_fold_kernel, dim3((a->K + SK_TILE - 1) / SK_TILE), dim3(SK_NT), 0, s, *a, 0);
    GV_LAUNCH_CHECK("gv_sinkhorn_rows(fold)");
    if (a->K >= 8192) hipLaunchKernelGGL(sk_rows_kernel<1024>, dim3(a->R), dim3(1024), 0, s, *a);
    else hipLaunchKernelGGL(sk_rows_kernel<256>, dim3(a->R), dim3(256), 0, s, *a);
    GV_LAUNCH_CHECK("gv_sinkhorn_rows");
    return GV_OK;
}

extern "C" int gv_sinkhorn_finish(const gv_sinkhorn_args* a, void* stream) {
    const int rc = sk_check(a, "gv_sinkhorn_finish", 3);
    if (rc != GV_OK) return rc;
    hipLaunchKernelGGL(sk_fold_kernel, dim3((a->K + SK_TILE - 1) / SK_TILE), dim3(SK_NT), 0, (hipStream_t)stream, *a, 1);
    GV_LAUNCH_CHECK("gv_sinkhorn_finish");
    return GV_OK;
}

extern "C" int64_t gv_koleo_workspace_bytes(int32_t G, int32_t B, int32_t D) {
    const char* bad = kl_shape_error(G, B, D);
    if (bad) { gv_set_error("gv_koleo_workspace_bytes: need %s (got G=%d B=%d D=%d)", bad, G, B, D); return -1; }
    return kl_workspace_bytes(G, B, D);
}

extern "C" int gv_koleo_fwd(const gv_koleo_args* a, void* stream) { return koleo_fwd_launch<bf16>(a, stream, "gv_koleo_fwd"); }
extern "C" int gv_koleo_fwd_f32(const gv_koleo_args* a, void* stream) { return koleo_fwd_launch<float>(a, stream, "gv_koleo_fwd_f32"); }
extern "C" int gv_koleo_bwd(const gv_koleo_args* a, void* stream) { return koleo_bwd_launch<bf16>(a, stream, "gv_koleo_bwd"); }
extern "C" int gv_koleo_bwd_f32(const gv_koleo_args* a, void* stream) { return koleo_bwd_launch<float>(a, stream, "gv_koleo_bwd_f32"); }
