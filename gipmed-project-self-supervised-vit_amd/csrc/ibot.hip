// The row kernels of the iBOT masked-patch term (DINOv2's iBOTPatchLoss.forward_masked; include/gipvit.h has the contract):
//   * gv_mask_tokens_fwd / _bwd: the learned mask token in place of the marked patch embeddings, and its gradient;
//   * gv_rows_gather / gv_rows_scatter: the pair around gv_layernorm_fwd / _bwd that runs the final norm on a row table;
//   * gv_ibot_loss: softmax((t - c_p) / tau_t) against log_softmax(s / tau_s) over the marked rows, each with its own weight;
//   * gv_patch_center_update: the EMA of c_p, with the row count read from the device.
// A row table is device data, so no entry point can check it: every kernel skips an entry outside [0, n_rows) (and, where the table
// names patch rows, a CLS row) instead of following it.  Sums over rows are stored per slice and added in slice order by a second
// launch: no atomics, bitwise the same run to run.  The f32 operand mode uses expf / logf, the 16-bit path the fast forms, far below
// the rounding of its gradient; both round logit * (1 / tau) on its own, as gv_dino_loss_f32 does.
#include "gv_common.h"
#include <float.h>

namespace {

constexpr int IB_NT = 256;
constexpr int MT_ROWS = 64;                 // table entries one workgroup of gv_mask_tokens_bwd sums
constexpr int IB_BLOCKS = 1024;             // workgroups the loss pass aims for (four per CU)
constexpr int IB_MAX_SLICES = 1024;

template <typename T> __device__ __forceinline__ void st4(T* p, f32x4 v);
template <> __device__ __forceinline__ void st4<float>(float* p, f32x4 v) { *(f32x4*)p = v; }
template <> __device__ __forceinline__ void st4<bf16>(bf16* p, f32x4 v) { *(bf16x4*)p = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]}; }

// ------------------------------------------------------------------------------------------------------------------ mask token
// grid (M): x[rows[i]] = mask_token + pos[rows[i] mod N]
__global__ __launch_bounds__(IB_NT) void mask_tokens_fwd_kernel(gv_mask_tokens_fwd_args a) {
    const int r = a.rows[blockIdx.x];
    if (r < 0 || r >= a.n_rows) return;
    const int t = r % a.N;
    if (t == 0) return;
    for (int c = threadIdx.x * 4; c < a.D; c += IB_NT * 4)
        *(f32x4*)(a.x + (long)r * a.D + c) = *(const f32x4*)(a.mask_token + c) + *(const f32x4*)(a.pos + (long)t * a.D + c);
}

// grid (slices of MT_ROWS entries), D / 4 threads: partial[slice] = sum of g over the slice's entries in table order, and the
// entries' rows of the compact patch gradient set to zero
template <typename PT>
__global__ __launch_bounds__(IB_NT) void mask_tokens_bwd_kernel(gv_mask_tokens_bwd_args a) {
    const int c = threadIdx.x * 4;
    if (c >= a.D) return;
    const int i0 = blockIdx.x * MT_ROWS, i1 = min(a.M, i0 + MT_ROWS);
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 s = zero;
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        const int r = a.rows[i];
        if (r < 0 || r >= a.n_rows) continue;
        const int img = r / a.N, t = r - img * a.N;
        if (t == 0) continue;
        s += *(const f32x4*)(a.g + (long)r * a.D + c);
        st4((PT*)a.gpatch + ((long)img * (a.N - 1) + (t - 1)) * a.D + c, zero);
    }
    *(f32x4*)(a.workspace + (long)blockIdx.x * a.D + c) = s;
}

// dmask_token (+)= the slices' partial sums, in slice order
__global__ __launch_bounds__(IB_NT) void mask_tokens_sum_kernel(gv_mask_tokens_bwd_args a, int n_slices) {
    const int c = threadIdx.x * 4;
    if (c >= a.D) return;
    f32x4 s = *(const f32x4*)(a.workspace + c);
    for (int y = 1; y < n_slices; ++y) s += *(const f32x4*)(a.workspace + (long)y * a.D + c);
    if (a.accumulate) s += *(const f32x4*)(a.dmask_token + c);
    *(f32x4*)(a.dmask_token + c) = s;
}

int mt_slices(int M) { return (M + MT_ROWS - 1) / MT_ROWS; }
bool mt_shape_ok(int M, int D) { return M >= 1 && D >= 4 && D <= IB_NT * 4 && D % 4 == 0; }

// ---------------------------------------------------------------------------------------------------------- gather and scatter
// grid (M): out[i] = x[rows[i]] (zeros for an entry outside the buffer), scale_out[i] = scale[rows[i]]
__global__ __launch_bounds__(IB_NT) void rows_gather_kernel(gv_rows_gather_args a) {
    const int i = blockIdx.x, r = a.rows[i];
    const bool ok = r >= 0 && r < a.n_rows;
    for (int c = threadIdx.x * 4; c < a.D; c += IB_NT * 4)
        *(f32x4*)(a.out + (long)i * a.D + c) = ok ? *(const f32x4*)(a.x + (long)r * a.x_stride + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x == 0 && a.scale_out) a.scale_out[i] = ok ? a.scale[r] : 0.f;
}

// grid (M): g[rows[i]] = g_src[i], gb[rows[i]] = gb_src[i]
template <typename T>
__global__ __launch_bounds__(IB_NT) void rows_scatter_kernel(gv_rows_scatter_args a) {
    const int i = blockIdx.x, r = a.rows[i];
    if (r < 0 || r >= a.n_rows) return;
    for (int c = threadIdx.x * 4; c < a.D; c += IB_NT * 4) {
        *(f32x4*)(a.g + (long)r * a.g_stride + c) = *(const f32x4*)(a.g_src + (long)i * a.D + c);
        if (a.gb) {
            if constexpr (sizeof(T) == 4) *(f32x4*)((float*)a.gb + (long)r * a.gb_stride + c) = *(const f32x4*)((const float*)a.gb_src + (long)i * a.D + c);
            else *(bf16x4*)((bf16*)a.gb + (long)r * a.gb_stride + c) = *(const bf16x4*)((const bf16*)a.gb_src + (long)i * a.D + c);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ loss
template <typename DT> __device__ __forceinline__ float ex(float x) { if constexpr (sizeof(DT) == 4) return expf(x); else return __expf(x); }
template <typename DT> __device__ __forceinline__ float lg(float x) { if constexpr (sizeof(DT) == 4) return logf(x); else return __logf(x); }
// logit * (1 / tau), rounded on its own in both operand modes: contracted into an FMA with the "- max" that follows, the second
// pass would see another exponent than the first (csrc/dino_loss.hip) -- and a row of one class would not come out as exactly p = 1
template <typename DT> __device__ __forceinline__ float scaled(float x, float inv_t) {
#pragma clang fp contract(off)
    return x * inv_t;
}

// VEC consecutive f32 (VEC = 4: one 16-byte load; VEC = 1 serves a K that is no multiple of 4, whose rows are not 16-byte aligned)
template <int VEC> __device__ __forceinline__ f32x4 ldv(const float* p, float fill) {
    if constexpr (VEC == 4) return *(const f32x4*)p;
    else return f32x4{p[0], fill, fill, fill};
}

// workspace: [0, 4 M) row statistics (maximum and log-sum-exp of the scaled row: student rows, then teacher rows), then the loss
// partials of the second pass [ktiles * slices], then, 16-byte aligned, the column-sum partials [slices, K]
struct IbPlan { int vec, ktiles, r_per, slices; long loss_off, cols_off, floats; };
IbPlan ib_plan(int M, int K) {
    IbPlan p;
    p.vec = K % 4 == 0 ? 4 : 1;
    const int tile = IB_NT * p.vec;
    p.ktiles = (K + tile - 1) / tile;
    int slices = (IB_BLOCKS + p.ktiles - 1) / p.ktiles;
    if (slices > IB_MAX_SLICES) slices = IB_MAX_SLICES;
    if (slices > M) slices = M;
    p.r_per = (M + slices - 1) / slices;
    p.slices = (M + p.r_per - 1) / p.r_per;
    p.loss_off = 4L * M;
    p.cols_off = (p.loss_off + (long)p.ktiles * p.slices + 3) & ~3L;
    p.floats = p.cols_off + (long)p.slices * K;
    return p;
}

struct IbTemps { float inv_ts, inv_tt; };
__device__ __forceinline__ IbTemps ib_temps(const gv_ibot_loss_args& a) {
    const float ts = a.hyper ? a.hyper[GV_HYP_STUDENT_TEMP] : a.student_temp, tt = a.hyper ? a.hyper[GV_HYP_TEACHER_TEMP] : a.teacher_temp;
    return IbTemps{1.0f / ts, 1.0f / tt};
}

// one workgroup per logits row (student rows, then teacher rows): the running maximum and sum of exponentials of the scaled row
template <typename DT, int VEC>
__global__ __launch_bounds__(IB_NT) void ib_row_stats_kernel(gv_ibot_loss_args a) {
    __shared__ float red_m[IB_NT / 64], red_s[IB_NT / 64];
    const int row = blockIdx.x;
    const bool teacher = row >= a.M;
    const IbTemps tp = ib_temps(a);
    const float* x = teacher ? a.teacher + (long)(row - a.M) * a.K : a.student + (long)row * a.K;
    const float inv_t = teacher ? tp.inv_tt : tp.inv_ts;
    float m = -INFINITY, s = 0.f;
    for (int k = threadIdx.x * VEC; k < a.K; k += IB_NT * VEC) {
        f32x4 v = ldv<VEC>(x + k, 0.f);
        if (teacher) v -= ldv<VEC>(a.center + k, 0.f);
        float lm = -INFINITY;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { v[e] = scaled<DT>(v[e], inv_t); lm = fmaxf(lm, v[e]); }
        if (lm > m) { s *= ex<DT>(m - lm); m = lm; }
#pragma unroll
        for (int e = 0; e < VEC; ++e) s += ex<DT>(v[e] - m);
    }
    const float wm = wave_max(m);
    s = (m == -INFINITY) ? 0.f : s * ex<DT>(m - wm);   // idle lanes when K < VEC * IB_NT
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) { red_m[threadIdx.x >> 6] = wm; red_s[threadIdx.x >> 6] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float Mx = red_m[0];
        for (int w = 1; w < IB_NT / 64; ++w) Mx = fmaxf(Mx, red_m[w]);
        float S = 0.f;
        for (int w = 0; w < IB_NT / 64; ++w) S += red_m[w] == -INFINITY ? 0.f : red_s[w] * ex<DT>(red_m[w] - Mx);
        a.workspace[2 * row] = Mx;
        a.workspace[2 * row + 1] = lg<DT>(S);
    }
}

// grid (column tiles, row slices); a thread owns VEC consecutive classes and walks its slice's rows in order: the gradient row
// pieces, its share of the weighted loss, and the raw teacher column sums of the slice
template <typename DT, int VEC>
__global__ __launch_bounds__(IB_NT) void ib_loss_grad_kernel(gv_ibot_loss_args a, IbPlan p) {
    __shared__ float red[IB_NT / 64];
    const int k = (blockIdx.x * IB_NT + threadIdx.x) * VEC;
    const int r0 = blockIdx.y * p.r_per, r1 = min(a.M, r0 + p.r_per);
    const IbTemps tp = ib_temps(a);
    float coef = a.ibot_weight * (a.grad_scale == 0.f ? 1.f : a.grad_scale) * tp.inv_ts;
    if (a.loss_scale) coef *= a.loss_scale[0];
    float loss = 0.f;
    if (k < a.K) {
        const f32x4 c = ldv<VEC>(a.center + k, 0.f);
        f32x4 csum = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int r = r0; r < r1; ++r) {
            const f32x4 sv = ldv<VEC>(a.student + (long)r * a.K + k, 0.f), raw = ldv<VEC>(a.teacher + (long)r * a.K + k, 0.f);
            const float sm = a.workspace[2 * r], sl = a.workspace[2 * r + 1];
            const float tm = a.workspace[2 * (a.M + r)], tl = a.workspace[2 * (a.M + r) + 1];
            const float w = a.weight[r];
            csum += raw;
            f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
            if (w != 0.f) {         // a row of weight 0: no loss, an exactly zero gradient row, whatever its logits hold
                float rl = 0.f;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float pt = ex<DT>(scaled<DT>(raw[e] - c[e], tp.inv_tt) - tm - tl);
                    const float logp = scaled<DT>(sv[e], tp.inv_ts) - sm - sl;
                    rl -= pt * logp;
                    g[e] = (w * coef) * (ex<DT>(logp) - pt);
                }
                loss += w * rl;
            }
            DT* dst = (DT*)a.dstudent + (long)r * a.K + k;
            if constexpr (VEC == 4) st4<DT>(dst, g);
            else dst[0] = (DT)g[0];
        }
        float* out = a.workspace + p.cols_off + (long)blockIdx.y * a.K + k;
        if constexpr (VEC == 4) *(f32x4*)out = csum;
        else out[0] = csum[0];
    }
    loss = wave_sum(loss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = loss;
    __syncthreads();
    if (threadIdx.x == 0) a.workspace[p.loss_off + (long)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// center_sum[k] = the slices' column sums in slice order; the workgroup behind the column tiles adds the loss partials in their
// order and writes the row count
template <int VEC>
__global__ __launch_bounds__(IB_NT) void ib_finish_kernel(gv_ibot_loss_args a, IbPlan p) {
    __shared__ float red[IB_NT / 64];
    if ((int)blockIdx.x == p.ktiles) {
        float s = 0.f;
        for (int i = threadIdx.x; i < p.ktiles * p.slices; i += IB_NT) s += a.workspace[p.loss_off + i];
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) { a.loss[0] = (red[0] + red[1]) + (red[2] + red[3]); a.center_sum[a.K] = (float)a.M; }
        return;
    }
    const int k = (blockIdx.x * IB_NT + threadIdx.x) * VEC;
    if (k >= a.K) return;
    const float* part = a.workspace + p.cols_off + k;
    f32x4 s = ldv<VEC>(part, 0.f);
    for (int y = 1; y < p.slices; ++y) s += ldv<VEC>(part + (long)y * a.K, 0.f);
    if constexpr (VEC == 4) *(f32x4*)(a.center_sum + k) = s;
    else a.center_sum[k] = s[0];
}

const char* ib_shape_error(int M, int K) {
    if (M < 1 || M > (1 << 20)) return "1 <= M <= 1048576";
    if (K < 1 || K > (1 << 20)) return "1 <= K <= 1048576";
    return nullptr;
}

template <typename DT, int VEC> int ibot_loss_run(const gv_ibot_loss_args* a, const IbPlan& p, hipStream_t s, const char* who) {
    hipLaunchKernelGGL((ib_row_stats_kernel<DT, VEC>), dim3(2 * a->M), dim3(IB_NT), 0, s, *a);
    GV_LAUNCH_CHECK("gv_ibot_loss(row_stats)");
    hipLaunchKernelGGL((ib_loss_grad_kernel<DT, VEC>), dim3(p.ktiles, p.slices), dim3(IB_NT), 0, s, *a, p);
    GV_LAUNCH_CHECK("gv_ibot_loss(loss_grad)");
    hipLaunchKernelGGL(ib_finish_kernel<VEC>, dim3(p.ktiles + 1), dim3(IB_NT), 0, s, *a, p);
    GV_LAUNCH_CHECK("gv_ibot_loss(finish)");
    (void)who;
    return GV_OK;
}

template <typename DT> int ibot_loss_launch(const gv_ibot_loss_args* a, void* stream, const char* who) {
    GV_REQUIRE(a, GV_E_NULL, "%s: null argument struct", who);
    GV_REQUIRE(a->student && a->teacher && a->center && a->weight && a->dstudent && a->loss && a->center_sum && a->workspace, GV_E_NULL,
               "%s: null pointer", who);
    const char* bad = ib_shape_error(a->M, a->K);
    GV_REQUIRE(!bad, GV_E_SHAPE, "%s: need %s (got M=%d K=%d)", who, bad, a->M, a->K);
    GV_REQUIRE(a->student_temp > 0.f && a->teacher_temp > 0.f, GV_E_SHAPE, "%s: temperatures must be > 0", who);
    GV_REQUIRE(a->ibot_weight == a->ibot_weight && a->ibot_weight >= 0.f && a->ibot_weight <= FLT_MAX, GV_E_SHAPE, "%s: ibot_weight must be finite and >= 0", who);
    const IbPlan p = ib_plan(a->M, a->K);
    const size_t al = p.vec == 4 ? 16 : 4;
    GV_REQUIRE(gv_aligned(a->student, al) && gv_aligned(a->teacher, al) && gv_aligned(a->center, al) && gv_aligned(a->center_sum, al) &&
               gv_aligned(a->workspace, 16) && gv_aligned(a->dstudent, p.vec == 4 ? 4 * sizeof(DT) : sizeof(DT)) && gv_aligned(a->weight, 4) && gv_aligned(a->loss, 4),
               GV_E_ALIGN, "%s: student, teacher, center, center_sum and workspace must be 16-byte aligned (4-byte when K is no multiple of 4)", who);
    GV_REQUIRE(a->workspace_bytes >= p.floats * 4, GV_E_SHAPE, "%s: workspace of %lld bytes, %ld needed (gv_ibot_loss_workspace_bytes)", who,
               (long long)a->workspace_bytes, p.floats * 4);
    hipStream_t s = (hipStream_t)stream;
    return p.vec == 4 ? ibot_loss_run<DT, 4>(a, p, s, who) : ibot_loss_run<DT, 1>(a, p, s, who);
}

// ---------------------------------------------------------------------------------------------------------------- patch centre
__global__ __launch_bounds__(IB_NT) void patch_center_update_kernel(gv_patch_center_update_args a) {
    const int k = blockIdx.x * IB_NT + threadIdx.x;
    const float n = a.center_sum[a.K];
    if (k >= a.K || !(n > 0.f)) return;
    a.center[k] = a.center[k] * a.momentum + (a.center_sum[k] / n) * (1.0f - a.momentum);
}

int rows_check(const char* who, const void* rows, int M, int D, int n_rows) {
    GV_REQUIRE(rows, GV_E_NULL, "%s: null pointer (rows)", who);
    GV_REQUIRE(M >= 1 && D >= 4 && D % 4 == 0 && n_rows >= 1, GV_E_SHAPE, "%s: need M >= 1, n_rows >= 1 and D a positive multiple of 4 (got M=%d D=%d n_rows=%d)",
               who, M, D, n_rows);
    GV_REQUIRE(gv_aligned(rows, 4), GV_E_ALIGN, "%s: rows must be 4-byte aligned", who);
    return GV_OK;
}

template <typename PT> int mask_tokens_bwd_launch(const gv_mask_tokens_bwd_args* a, void* stream, const char* who) {
    GV_REQUIRE(a, GV_E_NULL, "%s: null argument struct", who);
    GV_REQUIRE(a->g && a->gpatch && a->dmask_token && a->workspace, GV_E_NULL, "%s: null pointer", who);
    const int rc = rows_check(who, a->rows, a->M, a->D, a->n_rows);
    if (rc != GV_OK) return rc;
    GV_REQUIRE(a->D <= IB_NT * 4 && a->N >= 2 && a->n_rows % a->N == 0, GV_E_SHAPE, "%s: need D <= %d, N >= 2 and n_rows a multiple of N (got D=%d N=%d n_rows=%d)", who,
               IB_NT * 4, a->D, a->N, a->n_rows);
    GV_REQUIRE(gv_aligned(a->g, 16) && gv_aligned(a->dmask_token, 16) && gv_aligned(a->workspace, 16) && gv_aligned(a->gpatch, 4 * sizeof(PT)), GV_E_ALIGN,
               "%s: g, gpatch, dmask_token and workspace must be 16-byte aligned (gpatch: 8-byte in a 16-bit format)", who);
    const int n_slices = mt_slices(a->M);
    const long need = (long)n_slices * a->D * 4;
    GV_REQUIRE(a->workspace_bytes >= need, GV_E_SHAPE, "%s: workspace of %lld bytes, %ld needed (gv_mask_tokens_workspace_bytes)", who,
               (long long)a->workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mask_tokens_bwd_kernel<PT>, dim3(n_slices), dim3(IB_NT), 0, s, *a);
    GV_LAUNCH_CHECK("gv_mask_tokens_bwd");
    hipLaunchKernelGGL(mask_tokens_sum_kernel, dim3(1), dim3(IB_NT), 0, s, *a, n_slices);
    GV_LAUNCH_CHECK("gv_mask_tokens_bwd(sum)");
    return GV_OK;
}

template <typename T> int rows_scatter_launch(const gv_rows_scatter_args* a, void* stream, const char* who) {
    GV_REQUIRE(a, GV_E_NULL, "%s: null argument struct", who);
    GV_REQUIRE(a->g_src && a->g && (!a->gb == !a->gb_src), GV_E_NULL, "%s: null pointer (gb and gb_src go together)", who);
    const int rc = rows_check(who, a->rows, a->M, a->D, a->n_rows);
    if (rc != GV_OK) return rc;
    GV_REQUIRE(a->g_stride >= a->D && a->g_stride % 4 == 0 && (!a->gb || (a->gb_stride >= a->D && a->gb_stride % 4 == 0)), GV_E_SHAPE,
               "%s: strides must be multiples of 4 and >= D (got g_stride=%lld gb_stride=%lld D=%d)", who, (long long)a->g_stride, (long long)a->gb_stride, a->D);
    GV_REQUIRE(gv_aligned(a->g_src, 16) && gv_aligned(a->g, 16) && gv_aligned(a->gb_src, 4 * sizeof(T)) && gv_aligned(a->gb, 4 * sizeof(T)), GV_E_ALIGN,
               "%s: g_src and g must be 16-byte aligned, gb_src and gb to four elements", who);
    hipLaunchKernelGGL(rows_scatter_kernel<T>, dim3(a->M), dim3(IB_NT), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_rows_scatter");
    return GV_OK;
}

}  // namespace

extern "C" int gv_mask_tokens_fwd(const gv_mask_tokens_fwd_args* a, void* stream) {
    const char* who = "gv_mask_tokens_fwd";
    GV_REQUIRE(a, GV_E_NULL, "%s: null argument struct", who);
    GV_REQUIRE(a->x && a->mask_token && a->pos, GV_E_NULL, "%s: null pointer", who);
    const int rc = rows_check(who, a->rows, a->M, a->D, a->n_rows);
    if (rc != GV_OK) return rc;
    GV_REQUIRE(a->N >= 2 && a->n_rows % a->N == 0, GV_E_SHAPE, "%s: need N >= 2 and n_rows a multiple of N (got N=%d n_rows=%d)", who, a->N, a->n_rows);
    GV_REQUIRE(gv_aligned(a->x, 16) && gv_aligned(a->mask_token, 16) && gv_aligned(a->pos, 16), GV_E_ALIGN, "%s: x, mask_token and pos must be 16-byte aligned", who);
    hipLaunchKernelGGL(mask_tokens_fwd_kernel, dim3(a->M), dim3(IB_NT), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_mask_tokens_fwd");
    return GV_OK;
}

extern "C" int gv_mask_tokens_bwd(const gv_mask_tokens_bwd_args* a, void* stream) { return mask_tokens_bwd_launch<bf16>(a, stream, "gv_mask_tokens_bwd"); }
extern "C" int gv_mask_tokens_bwd_f32(const gv_mask_tokens_bwd_args* a, void* stream) { return mask_tokens_bwd_launch<float>(a, stream, "gv_mask_tokens_bwd_f32"); }

extern "C" int64_t gv_mask_tokens_workspace_bytes(int32_t M, int32_t D) {
    if (!mt_shape_ok(M, D)) { gv_set_error("gv_mask_tokens_workspace_bytes: need M >= 1 and D a multiple of 4 up to %d (got M=%d D=%d)", IB_NT * 4, M, D); return -1; }
    return (int64_t)mt_slices(M) * D * 4;
}

extern "C" int gv_rows_gather(const gv_rows_gather_args* a, void* stream) {
    const char* who = "gv_rows_gather";
    GV_REQUIRE(a, GV_E_NULL, "%s: null argument struct", who);
    GV_REQUIRE(a->x && a->out && (!a->scale == !a->scale_out), GV_E_NULL, "%s: null pointer (scale and scale_out go together)", who);
    const int rc = rows_check(who, a->rows, a->M, a->D, a->n_rows);
    if (rc != GV_OK) return rc;
    GV_REQUIRE(a->x_stride >= a->D && a->x_stride % 4 == 0, GV_E_SHAPE, "%s: x_stride must be a multiple of 4 and >= D (got %lld, D=%d)", who, (long long)a->x_stride, a->D);
    GV_REQUIRE(gv_aligned(a->x, 16) && gv_aligned(a->out, 16) && gv_aligned(a->scale, 4) && gv_aligned(a->scale_out, 4), GV_E_ALIGN, "%s: x and out must be 16-byte aligned", who);
    hipLaunchKernelGGL(rows_gather_kernel, dim3(a->M), dim3(IB_NT), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_rows_gather");
    return GV_OK;
}

extern "C" int gv_rows_scatter(const gv_rows_scatter_args* a, void* stream) { return rows_scatter_launch<bf16>(a, stream, "gv_rows_scatter"); }
extern "C" int gv_rows_scatter_f32(const gv_rows_scatter_args* a, void* stream) { return rows_scatter_launch<float>(a, stream, "gv_rows_scatter_f32"); }

extern "C" int gv_ibot_loss(const gv_ibot_loss_args* a, void* stream) { return ibot_loss_launch<bf16>(a, stream, "gv_ibot_loss"); }
extern "C" int gv_ibot_loss_f32(const gv_ibot_loss_args* a, void* stream) { return ibot_loss_launch<float>(a, stream, "gv_ibot_loss_f32"); }

extern "C" int64_t gv_ibot_loss_workspace_bytes(int32_t M, int32_t K) {
    const char* bad = ib_shape_error(M, K);
    if (bad) { gv_set_error("gv_ibot_loss_workspace_bytes: need %s (got M=%d K=%d)", bad, M, K); return -1; }
    return ib_plan(M, K).floats * 4;
}

extern "C" int gv_patch_center_update(const gv_patch_center_update_args* a, void* stream) {
    const char* who = "gv_patch_center_update";
    GV_REQUIRE(a, GV_E_NULL, "%s: null argument struct", who);
    GV_REQUIRE(a->center && a->center_sum, GV_E_NULL, "%s: null pointer", who);
    GV_REQUIRE(a->K >= 1, GV_E_SHAPE, "%s: K must be >= 1 (got %d)", who, a->K);
    GV_REQUIRE(a->momentum >= 0.f && a->momentum <= 1.f, GV_E_SHAPE, "%s: momentum must lie in [0, 1]", who);
    hipLaunchKernelGGL(patch_center_update_kernel, dim3((a->K + IB_NT - 1) / IB_NT), dim3(IB_NT), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_patch_center_update");
    return GV_OK;
}
