// Mean pooling of the patch tokens (timm VisionTransformer global_pool='avg': x[:, 1:].mean(dim=1), the CLS row excluded) in
// front of fc_norm, forward and backward.  Both kernels are HBM-bound row kernels: a workgroup owns (image, 64-column slab);
// its 256 threads are 16 column lanes of four columns x 16 row lanes strided over the tokens: the f32 traffic (x, pooled, dpool, g,
// and gb in the fp32 mode) is one 16-byte access per lane, a wave touching four rows of 256 contiguous bytes; the 16-bit gb of the
// backward is the same four columns, an 8-byte store per lane and four rows of 128 bytes per wave (eight columns per lane would
// make that store 16 bytes and halve the workgroups: not built, the backward runs at the forward's rate).
// Pooling is independent per column: no atomics, and the summation order (a row lane's tokens in ascending order, then the 16
// row lanes in ascending order) does not depend on the grid.
//   fwd bytes / image: (N - 1) * D * 4 in, D * 4 out;   bwd bytes / image: D * 4 in, N * D * (4 + 2) out (16-bit gb).
#include "gv_common.h"

namespace {

constexpr int POOL_COLS = 64;      // columns of a workgroup's slab (16 lanes x 4)
constexpr int POOL_ROWS = 16;      // row lanes

__global__ __launch_bounds__(256) void token_mean_fwd_kernel(gv_token_mean_fwd_args a, int slabs) {
    __shared__ f32x4 red[POOL_ROWS][POOL_COLS / 4];
    const int img = blockIdx.x / slabs, slab = blockIdx.x - img * slabs;
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = slab * POOL_COLS + cl * 4;
    const bool live = c < a.D;                   // D % 4 == 0: a lane's four columns are inside together
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const float* x = a.x + (long)img * a.N * a.D + c;
        int t = 1 + rl;
        // four rows in flight per lane, added in token order
        for (; t + 3 * POOL_ROWS < a.N; t += 4 * POOL_ROWS) {
            const f32x4 v0 = *(const f32x4*)(x + (long)t * a.D);
            const f32x4 v1 = *(const f32x4*)(x + (long)(t + POOL_ROWS) * a.D);
            const f32x4 v2 = *(const f32x4*)(x + (long)(t + 2 * POOL_ROWS) * a.D);
            const f32x4 v3 = *(const f32x4*)(x + (long)(t + 3 * POOL_ROWS) * a.D);
            acc += v0; acc += v1; acc += v2; acc += v3;
        }
        for (; t < a.N; t += POOL_ROWS) acc += *(const f32x4*)(x + (long)t * a.D);
    }
    red[rl][cl] = acc;
    __syncthreads();
    if (rl == 0 && live) {
        f32x4 s = red[0][cl];
#pragma unroll
        for (int r = 1; r < POOL_ROWS; ++r) s += red[r][cl];
        const float n = (float)(a.N - 1);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = s[j] / n;
        *(f32x4*)(a.pooled + (long)img * a.D + c) = o;
    }
}

// F32IO: gb is f32 (the fp32 operand mode), else the build's 16-bit format
template <bool F32IO>
__global__ __launch_bounds__(256) void token_mean_bwd_kernel(gv_token_mean_bwd_args a, int slabs) {
    const int img = blockIdx.x / slabs, slab = blockIdx.x - img * slabs;
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = slab * POOL_COLS + cl * 4;
    if (c >= a.D) return;
    const f32x4 d = *(const f32x4*)(a.dpool + (long)img * a.D + c);
    const float n = (float)(a.N - 1);
    const float gs = a.gb_scale ? a.gb_scale[img] : 1.0f;
    f32x4 gv, zero = {0.f, 0.f, 0.f, 0.f};
    float gbv[4], gbz[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) { gv[j] = d[j] / n; gbv[j] = gv[j] * gs; }
    bf16x4 hb, hz;
#pragma unroll
    for (int j = 0; j < 4; ++j) { hb[j] = (bf16)gbv[j]; hz[j] = (bf16)0.f; }
    const long row0 = (long)img * a.N;
    for (int t = rl; t < a.N; t += POOL_ROWS) {
        const long o = (row0 + t) * a.D + c;
        *(f32x4*)(a.g + o) = t ? gv : zero;            // row 0 of every image: the CLS token does not reach the pooled feature
        if constexpr (F32IO) {
            f32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = t ? gbv[j] : gbz[j];
            *(f32x4*)((float*)a.gb + o) = w;
        } else {
            *(bf16x4*)((bf16*)a.gb + o) = t ? hb : hz;
        }
    }
}

int pool_shape(const char* name, int n_img, int N, int D) {
    GV_REQUIRE(n_img > 0 && N >= 2, GV_E_SHAPE, "%s: n_img=%d N=%d: need n_img > 0 and at least one patch token (N >= 2)", name, n_img, N);
    GV_REQUIRE(D > 0 && D % 4 == 0, GV_E_SHAPE, "%s: D=%d must be a positive multiple of 4", name, D);
    const long slabs = (D + POOL_COLS - 1) / POOL_COLS;
    GV_REQUIRE((long)n_img * slabs <= 0x7fffffffL && (long)n_img * N <= 0x7fffffffL, GV_E_SHAPE, "%s: n_img=%d N=%d D=%d: too many rows / workgroups", name, n_img, N, D);
    return GV_OK;
}

}  // namespace

extern "C" int gv_token_mean_fwd(const gv_token_mean_fwd_args* a, void* stream) {
    GV_REQUIRE(a && a->x && a->pooled, GV_E_NULL, "gv_token_mean_fwd: null pointer");
    if (int rc = pool_shape("gv_token_mean_fwd", a->n_img, a->N, a->D)) return rc;
    GV_REQUIRE(gv_aligned(a->x, 16) && gv_aligned(a->pooled, 16), GV_E_ALIGN, "gv_token_mean_fwd: x and pooled must be 16-byte aligned");
    const int slabs = (a->D + POOL_COLS - 1) / POOL_COLS;
    hipLaunchKernelGGL(token_mean_fwd_kernel, dim3(a->n_img * slabs), dim3(256), 0, (hipStream_t)stream, *a, slabs);
    GV_LAUNCH_CHECK("gv_token_mean_fwd");
    return GV_OK;
}

template <bool F32IO> static int token_mean_bwd_launch(const gv_token_mean_bwd_args* a, void* stream) {
    GV_REQUIRE(a && a->dpool && a->g && a->gb, GV_E_NULL, "gv_token_mean_bwd: null pointer");
    if (int rc = pool_shape("gv_token_mean_bwd", a->n_img, a->N, a->D)) return rc;
    GV_REQUIRE(gv_aligned(a->dpool, 16) && gv_aligned(a->g, 16) && gv_aligned(a->gb, F32IO ? 16 : 8), GV_E_ALIGN,
               "gv_token_mean_bwd: dpool / g must be 16-byte aligned, gb %d-byte", F32IO ? 16 : 8);
    const int slabs = (a->D + POOL_COLS - 1) / POOL_COLS;
    hipLaunchKernelGGL(token_mean_bwd_kernel<F32IO>, dim3(a->n_img * slabs), dim3(256), 0, (hipStream_t)stream, *a, slabs);
    GV_LAUNCH_CHECK("gv_token_mean_bwd");
    return GV_OK;
}
extern "C" int gv_token_mean_bwd(const gv_token_mean_bwd_args* a, void* stream) { return token_mean_bwd_launch<false>(a, stream); }
extern "C" int gv_token_mean_bwd_f32(const gv_token_mean_bwd_args* a, void* stream) { return token_mean_bwd_launch<true>(a, stream); }
