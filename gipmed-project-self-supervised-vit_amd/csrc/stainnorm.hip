// Macenko stain normalisation at inference: the three estimation passes over a slide's sample tiles and gv_stain_apply
// (include/gipvit.h; gipvit/stainnorm.py holds the host steps between the passes and the fp64 restatement).
//
// The passes read each sampled pixel once (3 B) and keep everything else on chip: HBM-bound, n h w 3 bytes per pass plus the
// partials.  They compute in fp64 from a per-block table of the 256 od values and share one launch shape that depends on the
// SHAPE only: G = clamp(ceil(n h w / 256), 1, 512) workgroups of 256 threads walk the pixels with stride G * 256, reduce in a
// fixed order (lane tree, then the four waves left to right) and write one partial each; a second launch sums the partials in
// a fixed order.  Histogram bins are integer adds in LDS.  No floating-point atomic: bitwise reproducible on any device.
#include "gv_common.h"
#include "stain_px.h"

#pragma clang fp contract(off)

namespace {

constexpr int ST_MAXG = 512, ST_MIN_BINS = 256, ST_MAX_BINS = 4096;
typedef unsigned long long u64;

inline int stain_groups(u64 npx) {
    const u64 g = (npx + 255) / 256;
    return (int)(g < 1 ? 1 : (g > (u64)ST_MAXG ? (u64)ST_MAXG : g));
}

// the block's table of od values in fp64 (as stain_px.h builds its f32 one)
__device__ __forceinline__ void fill_od(double* odt) {
    odt[threadIdx.x] = -log((double)(threadIdx.x + 1) * (1.0 / 256.0));
    __syncthreads();
}

// pixel p of [n, h, w]: tile p / hw, pixel p % hw
__device__ __forceinline__ const uint8_t* pixel(const uint8_t* tiles, int64_t stride, u64 hw, u64 p) {
    const u64 t = p / hw;
    return tiles + (int64_t)t * stride + (int64_t)(p - t * hw) * 3;
}

// ---- pass 1: n, sum od, sum od_i od_j over tissue pixels.  Partial g: 10 x 8 bytes = {u64 n, f64 s[9]}
__global__ __launch_bounds__(256) void stain_stats_kernel(gv_stain_stats_args a, u64 npx) {
    __shared__ double odt[256];
    __shared__ double red[4][9];
    __shared__ u64 redn[4];
    fill_od(odt);
    const u64 hw = (u64)a.h * (u64)a.w;
    double s[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    u64 cnt = 0;
    for (u64 p = (u64)blockIdx.x * 256 + threadIdx.x; p < npx; p += (u64)gridDim.x * 256) {
        const uint8_t* q = pixel(a.tiles, a.img_stride, hw, p);
        const int r = q[0], g = q[1], b = q[2];
        if (r <= a.v_max && g <= a.v_max && b <= a.v_max) {
            const double o0 = odt[r], o1 = odt[g], o2 = odt[b];
            ++cnt;
            s[0] += o0; s[1] += o1; s[2] += o2;
            s[3] += o0 * o0; s[4] += o0 * o1; s[5] += o0 * o2;
            s[6] += o1 * o1; s[7] += o1 * o2; s[8] += o2 * o2;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] += __shfl_xor(s[k], o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        redn[wave] = cnt;
#pragma unroll
        for (int k = 0; k < 9; ++k) red[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64* pn = (u64*)a.workspace + (u64)blockIdx.x * 10;
        double* ps = (double*)(pn + 1);
        pn[0] = redn[0] + redn[1] + redn[2] + redn[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) ps[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// one wave: lane l takes partials l, l + 64, ... in order, then the lane tree
__global__ __launch_bounds__(64) void stain_stats_sum_kernel(const void* ws, int G, void* out) {
    const u64* part = (const u64*)ws;
    u64 cnt = 0;
    double s[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    for (int g = threadIdx.x; g < G; g += 64) {
        cnt += part[(u64)g * 10];
        const double* ps = (const double*)(part + (u64)g * 10 + 1);
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] += ps[k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] += __shfl_xor(s[k], o, 64);
    }
    if (threadIdx.x == 0) {
        ((u64*)out)[0] = cnt;
#pragma unroll
        for (int k = 0; k < 9; ++k) ((double*)out)[1 + k] = s[k];
    }
}

// ---- passes 2 and 3: per-workgroup histograms in LDS (integer adds), written out whole as the workgroup's partial
__device__ __forceinline__ void hist_clear(unsigned* hist, int len) {
    for (int i = threadIdx.x; i < len; i += 256) hist[i] = 0u;
    __syncthreads();
}
__device__ __forceinline__ void hist_store(const unsigned* hist, int len, void* ws) {
    __syncthreads();
    unsigned* part = (unsigned*)ws + (u64)blockIdx.x * len;
    for (int i = threadIdx.x; i < len; i += 256) part[i] = hist[i];
}

__global__ __launch_bounds__(256) void stain_angle_hist_kernel(gv_stain_angle_hist_args a, u64 npx) {
    __shared__ double odt[256];
    __shared__ unsigned hist[ST_MAX_BINS];
    const int NB = a.n_bins;
    hist_clear(hist, NB);
    fill_od(odt);
    const u64 hw = (u64)a.h * (u64)a.w;
    const double pi = 3.14159265358979323846;
    for (u64 p = (u64)blockIdx.x * 256 + threadIdx.x; p < npx; p += (u64)gridDim.x * 256) {
        const uint8_t* q = pixel(a.tiles, a.img_stride, hw, p);
        const int r = q[0], g = q[1], b = q[2];
        if (r <= a.v_max && g <= a.v_max && b <= a.v_max) {
            const double o0 = odt[r], o1 = odt[g], o2 = odt[b];
            const double t0 = o0 * a.V[0] + o1 * a.V[2] + o2 * a.V[4];
            const double t1 = o0 * a.V[1] + o1 * a.V[3] + o2 * a.V[5];
            const double f = floor((atan2(t1, t0) + pi) * (double)NB / (2.0 * pi));
            int bin = f < 0. ? 0 : (f >= (double)NB ? NB - 1 : (int)f);      // (a NaN compares false twice: bin 0 after the cast's clamp)
            bin = bin < 0 ? 0 : (bin >= NB ? NB - 1 : bin);
            atomicAdd(&hist[bin], 1u);
        }
    }
    hist_store(hist, NB, a.workspace);
}

__global__ __launch_bounds__(256) void stain_conc_hist_kernel(gv_stain_conc_hist_args a, u64 npx) {
    __shared__ double odt[256];
    __shared__ unsigned hist[2 * (ST_MAX_BINS + 1)];
    const int NB = a.n_bins, len = 2 * (NB + 1);
    hist_clear(hist, len);
    fill_od(odt);
    const u64 hw = (u64)a.h * (u64)a.w;
    for (u64 p = (u64)blockIdx.x * 256 + threadIdx.x; p < npx; p += (u64)gridDim.x * 256) {
        const uint8_t* q = pixel(a.tiles, a.img_stride, hw, p);
        const double o0 = odt[q[0]], o1 = odt[q[1]], o2 = odt[q[2]];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double c = o0 * a.pinv[3 * k] + o1 * a.pinv[3 * k + 1] + o2 * a.pinv[3 * k + 2];
            int bin = NB;                                                    // the underflow count
            if (!(c < 0.)) {
                const double f = floor(c * (double)NB / a.cmax[k]);
                bin = f >= (double)NB ? NB - 1 : (int)f;
                bin = bin < 0 ? 0 : (bin >= NB ? NB - 1 : bin);
            }
            atomicAdd(&hist[k * (NB + 1) + bin], 1u);
        }
    }
    hist_store(hist, len, a.workspace);
}

// out[i] = sum over the G partials of entry i (integers: any order gives the same sum; this one is g = 0 .. G - 1)
__global__ __launch_bounds__(256) void stain_hist_sum_kernel(const void* ws, int G, int len, int64_t* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const unsigned* part = (const unsigned*)ws;
    int64_t s = 0;
    for (int g = 0; g < G; ++g) s += (int64_t)part[(u64)g * len + i];
    out[i] = s;
}

__global__ __launch_bounds__(256) void stain_apply_kernel(gv_stain_apply_args a) {
    __shared__ float odt[256];
    const int tile = blockIdx.y;
    const gv_stain_params st = a.stain[tile];
    if (st.on) odt[threadIdx.x] = stain_od_entry(threadIdx.x);               // (st.on is the block's: the barrier is uniform)
    __syncthreads();
    const long hw = (long)a.h * a.w;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const uint8_t* src = a.tiles + (long)tile * a.img_stride + i * 3;
    uint8_t* dst = a.out + ((long)tile * hw + i) * 3;
    Px p{src[0], src[1], src[2]};
    if (st.on) p = stain_px(p, st, odt);
    dst[0] = (uint8_t)p.r; dst[1] = (uint8_t)p.g; dst[2] = (uint8_t)p.b;
}

// what the three passes check alike; -> npx
int pass_check(const char* name, const uint8_t* tiles, int64_t stride, int n, int h, int w, const void* ws, const void* out, u64* npx) {
    GV_REQUIRE(tiles && ws && out, GV_E_NULL, "%s: null pointer", name);
    GV_REQUIRE(gv_aligned(ws, 8) && gv_aligned(out, 8), GV_E_ALIGN, "%s: workspace / out must be 8-byte aligned", name);
    GV_REQUIRE(n > 0 && h > 0 && w > 0, GV_E_SHAPE, "%s: bad shape %d x %d x %d", name, n, h, w);
    const u64 hw = (u64)h * (u64)w;
    GV_REQUIRE(hw < (1ull << 32) && (u64)n * hw < (1ull << 32), GV_E_SHAPE, "%s: n * h * w = %d * %d * %d must stay below 2^32", name, n, h, w);
    GV_REQUIRE(stride >= (int64_t)(hw * 3), GV_E_SHAPE, "%s: img_stride %ld is less than a tile (%ld bytes)", name, (long)stride, (long)(hw * 3));
    *npx = (u64)n * hw;
    return GV_OK;
}

int bins_check(const char* name, int nb) {
    GV_REQUIRE(nb >= ST_MIN_BINS && nb <= ST_MAX_BINS, GV_E_SHAPE, "%s: n_bins=%d must be in %d .. %d", name, nb, ST_MIN_BINS, ST_MAX_BINS);
    return GV_OK;
}

}  // namespace

extern "C" int gv_stain_stats(const gv_stain_stats_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_stain_stats: null pointer");
    u64 npx = 0;
    if (const int rc = pass_check("gv_stain_stats", a->tiles, a->img_stride, a->n, a->h, a->w, a->workspace, a->out, &npx)) return rc;
    GV_REQUIRE(a->v_max >= 0 && a->v_max <= 255, GV_E_SHAPE, "gv_stain_stats: v_max=%d must be a byte value", a->v_max);
    const int G = stain_groups(npx);
    hipLaunchKernelGGL(stain_stats_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, *a, npx);
    GV_LAUNCH_CHECK("gv_stain_stats");
    hipLaunchKernelGGL(stain_stats_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const void*)a->workspace, G, a->out);
    GV_LAUNCH_CHECK("gv_stain_stats(sum)");
    return GV_OK;
}

extern "C" int gv_stain_angle_hist(const gv_stain_angle_hist_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_stain_angle_hist: null pointer");
    u64 npx = 0;
    if (const int rc = pass_check("gv_stain_angle_hist", a->tiles, a->img_stride, a->n, a->h, a->w, a->workspace, a->out, &npx)) return rc;
    if (const int rc = bins_check("gv_stain_angle_hist", a->n_bins)) return rc;
    GV_REQUIRE(a->v_max >= 0 && a->v_max <= 255, GV_E_SHAPE, "gv_stain_angle_hist: v_max=%d must be a byte value", a->v_max);
    const int G = stain_groups(npx), len = a->n_bins;
    hipLaunchKernelGGL(stain_angle_hist_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, *a, npx);
    GV_LAUNCH_CHECK("gv_stain_angle_hist");
    hipLaunchKernelGGL(stain_hist_sum_kernel, dim3((len + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const void*)a->workspace, G, len, a->out);
    GV_LAUNCH_CHECK("gv_stain_angle_hist(sum)");
    return GV_OK;
}

extern "C" int gv_stain_conc_hist(const gv_stain_conc_hist_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_stain_conc_hist: null pointer");
    u64 npx = 0;
    if (const int rc = pass_check("gv_stain_conc_hist", a->tiles, a->img_stride, a->n, a->h, a->w, a->workspace, a->out, &npx)) return rc;
    if (const int rc = bins_check("gv_stain_conc_hist", a->n_bins)) return rc;
    GV_REQUIRE(a->cmax[0] > 0. && a->cmax[1] > 0., GV_E_SHAPE, "gv_stain_conc_hist: cmax must be > 0");
    const int G = stain_groups(npx), len = 2 * (a->n_bins + 1);
    hipLaunchKernelGGL(stain_conc_hist_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, *a, npx);
    GV_LAUNCH_CHECK("gv_stain_conc_hist");
    hipLaunchKernelGGL(stain_hist_sum_kernel, dim3((len + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const void*)a->workspace, G, len, a->out);
    GV_LAUNCH_CHECK("gv_stain_conc_hist(sum)");
    return GV_OK;
}

extern "C" int gv_stain_apply(const gv_stain_apply_args* a, void* stream) {
    GV_REQUIRE(a && a->tiles && a->out && a->stain, GV_E_NULL, "gv_stain_apply: null pointer");
    GV_REQUIRE(gv_aligned(a->stain, 4), GV_E_ALIGN, "gv_stain_apply: stain misaligned");
    GV_REQUIRE(a->n > 0 && a->n <= 65535 && a->h > 0 && a->w > 0, GV_E_SHAPE, "gv_stain_apply: bad shape %d x %d x %d (at most 65535 tiles per call)", a->n, a->h, a->w);
    const long hw = (long)a->h * a->w;
    GV_REQUIRE(hw < (1L << 31) && a->img_stride >= hw * 3, GV_E_SHAPE, "gv_stain_apply: img_stride %ld is less than a tile (%ld bytes)", (long)a->img_stride, hw * 3);
    hipLaunchKernelGGL(stain_apply_kernel, dim3((unsigned)((hw + 255) / 256), a->n), dim3(256), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_stain_apply");
    return GV_OK;
}
