// Fused AdamW + teacher EMA + bf16 weight refresh over a flat parameter arena.
// Replaces optimizer.step() (reference train.py:1078; torch.optim.AdamW semantics) and
// the EMA update (train.py:1080-1081 ModelEmaV2 / DINO teacher) with one
// HBM-bound pass: per element 20 B read (g, p, m, v, teacher) + 20 B written
// (p, m, v, teacher, two bf16 copies).
#include "gv_common.h"

namespace {

// The two optimizer kernels below must agree BIT FOR BIT (with every range scale 1 the range kernel has to reproduce the plain
// one), and the plain one must keep the bits it has always produced.  Left to the compiler, which products and sums contract
// into FMAs depends on the code around the inlined copy, so contraction is switched off in the shared functions and every
// FMA is written out -- exactly those the plain kernel has been built with so far.
__device__ __forceinline__ f32x4 fma4(const f32x4 a, const f32x4 b, const f32x4 c) {
    return f32x4{__builtin_fmaf(a[0], b[0], c[0]), __builtin_fmaf(a[1], b[1], c[1]), __builtin_fmaf(a[2], b[2], c[2]), __builtin_fmaf(a[3], b[3], c[3])};
}
__device__ __forceinline__ f32x4 fma4(const f32x4 a, const float b, const f32x4 c) { return fma4(a, f32x4{b, b, b, b}, c); }

// What one launch resolves before it touches an element: the schedule values (by value or from `hyper`), the loss-scaled skip,
// the applied-step bias corrections and the global-norm clip.  A is gv_adamw_ema_args or gv_adamw_ema_ranges_args: the two
// carry the same fields under the same names.
struct adam_step { float gscale, lr, weight_decay, bias_corr1, bias_corr2, teacher_momentum; int mode; };

template <class A>
__device__ __forceinline__ adam_step adam_resolve(A a) {
#pragma clang fp contract(off)
    if (a.hyper) {
        a.lr = a.hyper[GV_HYP_LR]; a.weight_decay *= a.hyper[GV_HYP_WD];   // by-value wd is a 0/1 multiplier here
        a.bias_corr1 = a.hyper[GV_HYP_BC1]; a.bias_corr2 = a.hyper[GV_HYP_BC2];
        a.teacher_momentum = a.hyper[GV_HYP_TEACHER_MOM]; a.grad_scale = a.hyper[GV_HYP_GRAD_SCALE];
    }
    float gscale = a.grad_scale;
    if (a.loss_scale) {                                    // fp16 loss scaling: unscale; a non-finite gradient skips the step
        gscale /= a.loss_scale[0];
        if (!isfinite(*a.gnorm_sq)) a.mode = 3;
        // a skipped step is no optimizer step: Adam's bias corrections count the APPLIED steps (state[3]), not the host's calls
        const float t = a.loss_scale[3] + 1.0f;
        a.bias_corr1 = 1.0f - powf(a.beta1, t); a.bias_corr2 = 1.0f - powf(a.beta2, t);
    }
    if (a.clip_norm > 0.f && a.mode != 3) {
        const float c = a.clip_norm / __builtin_fmaf(sqrtf(*a.gnorm_sq), fabsf(gscale), 1e-6f);      // clip / (||g|| + 1e-6)
        if (c < 1.0f) gscale *= c;
    }
    return adam_step{gscale, a.lr, a.weight_decay, a.bias_corr1, a.bias_corr2, a.teacher_momentum, a.mode};
}

// THE per-element update of both optimizer kernels: f32x4 units i0, i0 + stride, ... < i1 of the buffers in `a` are stepped at
// rate `lr` with weight decay `weight_decay` (uniform over the units of one call); everything else comes from `s`.
template <class A>
__device__ __forceinline__ void adam_update(const A& a, const adam_step& s, const float lr, const float weight_decay,
                                            const long i0, const long i1, const long stride) {
#pragma clang fp contract(off)
    const float decay = __builtin_fmaf(-lr, weight_decay, 1.0f);       // 1 - lr * wd
    const float step = lr / s.bias_corr1;
    const float inv_sqrt_bc2 = 1.0f / sqrtf(s.bias_corr2);
    const float om = 1.0f - s.teacher_momentum;
    for (long i = i0; i < i1; i += stride) {
        f32x4 g = s.mode == 3 ? f32x4{0.f, 0.f, 0.f, 0.f} : ((const f32x4*)a.grad)[i] * s.gscale;
        if (a.clip_value > 0.f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = fminf(fmaxf(g[j], -a.clip_value), a.clip_value);
        }
        f32x4 p = ((f32x4*)a.p)[i], m = ((f32x4*)a.m)[i], v = ((f32x4*)a.v)[i];
        if (s.mode == 3) {
            // frozen range (no gradient: the optimizer skips the parameter); only the EMA below runs
        } else if (s.mode == 0) {
            p *= decay;
        } else {
            g = fma4(p, weight_decay, g);                   // L2 decay rides on the gradient
        }
        if (s.mode == 3) {
        } else if (s.mode == 2) {                                  // SGD, Nesterov momentum (torch.optim.SGD semantics)
            m = m * a.beta1 + g;
            p = fma4(fma4(m, a.beta1, g), -lr, p);          // p -= (g + m * beta1) * lr
        } else {
            m = fma4(g, 1.0f - a.beta1, m * a.beta1);
            v = fma4(v, a.beta2, g * g * (1.0f - a.beta2));
            // sqrt(v) / sqrt(bc2) + eps: one FMA in lanes 0 and 1, product and sum rounded separately in lanes 2 and 3 (see above)
            p[0] -= step * m[0] / __builtin_fmaf(sqrtf(v[0]), inv_sqrt_bc2, a.eps);
            p[1] -= step * m[1] / __builtin_fmaf(sqrtf(v[1]), inv_sqrt_bc2, a.eps);
            p[2] -= step * m[2] / (sqrtf(v[2]) * inv_sqrt_bc2 + a.eps);
            p[3] -= step * m[3] / (sqrtf(v[3]) * inv_sqrt_bc2 + a.eps);
        }
        if (s.mode != 3) { ((f32x4*)a.p)[i] = p; ((f32x4*)a.m)[i] = m; ((f32x4*)a.v)[i] = v; }
        if (a.p_bf16) ((bf16x4*)a.p_bf16)[i] = bf16x4{(bf16)p[0], (bf16)p[1], (bf16)p[2], (bf16)p[3]};
        if (a.teacher) {
            f32x4 t = fma4(p, om, ((f32x4*)a.teacher)[i] * s.teacher_momentum);
            ((f32x4*)a.teacher)[i] = t;
            if (a.teacher_bf16) ((bf16x4*)a.teacher_bf16)[i] = bf16x4{(bf16)t[0], (bf16)t[1], (bf16)t[2], (bf16)t[3]};
        }
    }
}

__global__ __launch_bounds__(256) void adamw_ema_kernel(gv_adamw_ema_args a) {
    const adam_step s = adam_resolve(a);
    adam_update(a, s, s.lr, s.weight_decay, (long)blockIdx.x * 256 + threadIdx.x, a.n >> 2, (long)gridDim.x * 256);
}

// The same pass over a RANGE TABLE (include/gipvit.h gv_adamw_ema_ranges): a workgroup takes whole rows {range, lo, hi} of the
// block table, so the range's rate and decay are uniform over the workgroup (two scalar loads per row) and the element
// traffic is the 16-byte loads and stores of the kernel above.  A row that does not lie inside [0, n) or names no range is skipped.
__global__ __launch_bounds__(256) void adamw_ema_ranges_kernel(gv_adamw_ema_ranges_args a) {
    const adam_step s = adam_resolve(a);
    for (int row = blockIdx.x; row < a.n_blocks; row += gridDim.x) {
        const int r = a.blocks[3 * row], lo = a.blocks[3 * row + 1], hi = a.blocks[3 * row + 2];
        if (r < 0 || r >= a.n_ranges || lo < 0 || hi > a.n || lo >= hi) continue;
        const float lr = s.lr * a.ranges[2 * r], wd = s.weight_decay * a.ranges[2 * r + 1];
        adam_update(a, s, lr, wd, (long)(lo >> 2) + threadIdx.x, (long)(hi >> 2), 256L);
    }
}

__global__ void loss_scale_update_kernel(gv_loss_scale_update_args a) {
    float S = a.state[0], good = a.state[1];
    if (!isfinite(*a.gnorm_sq)) { S *= a.backoff_factor; good = 0.f; a.state[2] += 1.f; }
    else {
        a.state[3] += 1.f;
        if (++good >= (float)a.growth_interval) { S *= a.growth_factor; good = 0.f; }
    }
    a.state[0] = S; a.state[1] = good;
}

// adaptive gradient clipping: one wave per unit (include/gipvit.h gv_agc)
__global__ __launch_bounds__(256) void agc_kernel(gv_agc_args a) {
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (u >= a.n_units) return;
    const int off = a.units[2 * u], len = a.units[2 * u + 1];
    const float* p = a.p + off; float* g = a.grad + off;
    float sp = 0.f, sg = 0.f;
    for (int i = lane; i < len; i += 64) { const float pv = p[i], gv = g[i] * a.grad_scale; sp += pv * pv; sg += gv * gv; }
    sp = wave_sum(sp); sg = wave_sum(sg);
    const float max_norm = fmaxf(sqrtf(sp), a.eps) * a.clip_factor, gn = sqrtf(sg);
    if (gn < max_norm) return;
    const float c = max_norm / fmaxf(gn, 1e-6f);
    for (int i = lane; i < len; i += 64) g[i] *= c;
}

// LAMB, both phases (include/gipvit.h gv_lamb).  One workgroup per table entry: a slice of ONE tensor.
__global__ __launch_bounds__(256) void lamb_kernel(gv_lamb_args a) {
    const int tensor = a.blocks[blockIdx.x * 3], lo = a.blocks[blockIdx.x * 3 + 1], hi = a.blocks[blockIdx.x * 3 + 2];
    float gscale = a.grad_scale;
    {
        float nrm = sqrtf(*a.gnorm_sq) * fabsf(a.grad_scale);
        if (a.clip_norm > 0.f) { const float c = a.clip_norm / (nrm + 1e-6f); if (c < 1.0f) { gscale *= c; nrm *= c; } }
        if (a.max_grad_norm > 0.f && nrm > a.max_grad_norm) gscale *= a.max_grad_norm / nrm;
    }
    const float inv_bc1 = 1.0f / a.bias_corr1, inv_sqrt_bc2 = 1.0f / sqrtf(a.bias_corr2);
    float trust = 1.0f;
    if (a.phase == 1 && a.weight_decay != 0.f) {
        const float wn = sqrtf(a.stats[2 * tensor]), un = sqrtf(a.stats[2 * tensor + 1]);
        trust = (wn > 0.f && un > 0.f) ? wn / un : 1.0f;
    }
    const float om = 1.0f - a.teacher_momentum;
    const float lr = a.lr_scale ? a.lr * a.lr_scale[tensor] : a.lr;   // --layer-decay: the tensor's own rate
    float sp = 0.f, su = 0.f;
    for (long i = (lo >> 2) + threadIdx.x; i < (hi >> 2); i += 256) {
        f32x4 p = ((f32x4*)a.p)[i], m = ((f32x4*)a.m)[i], v = ((f32x4*)a.v)[i];
        if (a.phase == 0) {
            const f32x4 g = ((const f32x4*)a.grad)[i] * gscale;
            m = m * a.beta1 + g * (1.0f - a.beta1);
            v = v * a.beta2 + g * g * (1.0f - a.beta2);
            ((f32x4*)a.m)[i] = m; ((f32x4*)a.v)[i] = v;
        }
        f32x4 u;
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = (m[j] * inv_bc1) / (sqrtf(v[j]) * inv_sqrt_bc2 + a.eps) + a.weight_decay * p[j];
        if (a.phase == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { sp += p[j] * p[j]; su += u[j] * u[j]; }
        } else {
            p -= u * (lr * trust);
            ((f32x4*)a.p)[i] = p;
            if (a.p_bf16) ((bf16x4*)a.p_bf16)[i] = bf16x4{(bf16)p[0], (bf16)p[1], (bf16)p[2], (bf16)p[3]};
            if (a.teacher) {
                f32x4 t = ((f32x4*)a.teacher)[i] * a.teacher_momentum + p * om;
                ((f32x4*)a.teacher)[i] = t;
                if (a.teacher_bf16) ((bf16x4*)a.teacher_bf16)[i] = bf16x4{(bf16)t[0], (bf16)t[1], (bf16)t[2], (bf16)t[3]};
            }
        }
    }
    if (a.phase == 0) {
        sp = wave_sum(sp); su = wave_sum(su);
        __shared__ float red[8];
        if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = sp; red[4 + (threadIdx.x >> 6)] = su; }
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicAdd(a.stats + 2 * tensor, red[0] + red[1] + red[2] + red[3]);
            atomicAdd(a.stats + 2 * tensor + 1, red[4] + red[5] + red[6] + red[7]);
        }
    }
}

}  // namespace

extern "C" int gv_loss_scale_update(const gv_loss_scale_update_args* a, void* stream) {
    GV_REQUIRE(a && a->state && a->gnorm_sq, GV_E_NULL, "gv_loss_scale_update: null pointer");
    GV_REQUIRE(a->growth_factor >= 1.f && a->backoff_factor > 0.f && a->backoff_factor <= 1.f && a->growth_interval > 0, GV_E_SHAPE,
               "gv_loss_scale_update: need growth_factor >= 1, 0 < backoff_factor <= 1, growth_interval > 0");
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_loss_scale_update");
    return GV_OK;
}

extern "C" int gv_agc(const gv_agc_args* a, void* stream) {
    GV_REQUIRE(a && a->p && a->grad && a->units, GV_E_NULL, "gv_agc: null pointer");
    GV_REQUIRE(a->n_units > 0 && a->clip_factor > 0.f && a->eps > 0.f, GV_E_SHAPE, "gv_agc: need n_units > 0, clip_factor > 0, eps > 0");
    hipLaunchKernelGGL(agc_kernel, dim3((a->n_units + 3) / 4), dim3(256), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_agc");
    return GV_OK;
}

extern "C" int gv_lamb(const gv_lamb_args* a, void* stream) {
    GV_REQUIRE(a && a->p && a->grad && a->m && a->v && a->blocks && a->stats && a->gnorm_sq, GV_E_NULL, "gv_lamb: null pointer");
    GV_REQUIRE(a->phase == 0 || a->phase == 1, GV_E_UNSUPPORTED, "gv_lamb: phase must be 0 (moments + norms) or 1 (apply)");
    GV_REQUIRE(a->n_blocks > 0, GV_E_SHAPE, "gv_lamb: empty block table");
    GV_REQUIRE(gv_aligned(a->p, 16) && gv_aligned(a->grad, 16) && gv_aligned(a->m, 16) && gv_aligned(a->v, 16), GV_E_ALIGN,
               "gv_lamb: buffers must be 16-byte aligned");
    GV_REQUIRE(a->bias_corr1 > 0.f && a->bias_corr2 > 0.f, GV_E_SHAPE, "gv_lamb: bias corrections must be > 0");
    hipLaunchKernelGGL(lamb_kernel, dim3((unsigned)a->n_blocks), dim3(256), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_lamb");
    return GV_OK;
}

extern "C" int gv_adamw_ema(const gv_adamw_ema_args* a, void* stream) {
    GV_REQUIRE(a && a->p && a->grad && a->m && a->v, GV_E_NULL, "gv_adamw_ema: null pointer");
    GV_REQUIRE(a->mode >= 0 && a->mode <= 3, GV_E_UNSUPPORTED, "gv_adamw_ema: mode must be 0 (AdamW), 1 (Adam+L2), 2 (SGD Nesterov) or 3 (frozen: EMA only)");
    GV_REQUIRE(a->n > 0 && a->n % 4 == 0, GV_E_SHAPE, "gv_adamw_ema: n=%ld must be a positive multiple of 4 (pad the arena)", (long)a->n);
    GV_REQUIRE(gv_aligned(a->p, 16) && gv_aligned(a->grad, 16) && gv_aligned(a->m, 16) && gv_aligned(a->v, 16), GV_E_ALIGN,
               "gv_adamw_ema: buffers must be 16-byte aligned");
    if (a->clip_norm > 0.f) GV_REQUIRE(a->gnorm_sq, GV_E_NULL, "gv_adamw_ema: clip_norm needs gnorm_sq");
    if (a->loss_scale) GV_REQUIRE(a->gnorm_sq, GV_E_NULL, "gv_adamw_ema: loss_scale needs gnorm_sq (the finite check)");
    GV_REQUIRE(!(a->clip_norm > 0.f && a->clip_value > 0.f), GV_E_UNSUPPORTED, "gv_adamw_ema: clip_norm and clip_value exclude each other (--clip-mode norm | value)");
    if (!a->hyper) GV_REQUIRE(a->bias_corr1 > 0.f && a->bias_corr2 > 0.f, GV_E_SHAPE, "gv_adamw_ema: bias corrections must be > 0");
    long blocks = (a->n / 4 + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(adamw_ema_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_adamw_ema");
    return GV_OK;
}

extern "C" int gv_adamw_ema_ranges(const gv_adamw_ema_ranges_args* a, void* stream) {
    GV_REQUIRE(a && a->p && a->grad && a->m && a->v, GV_E_NULL, "gv_adamw_ema_ranges: null pointer");
    GV_REQUIRE(a->blocks && a->ranges, GV_E_NULL, "gv_adamw_ema_ranges: null table (blocks / ranges)");
    GV_REQUIRE(a->n_blocks > 0 && a->n_ranges > 0, GV_E_SHAPE, "gv_adamw_ema_ranges: empty table (n_blocks=%d, n_ranges=%d)", (int)a->n_blocks, (int)a->n_ranges);
    GV_REQUIRE(a->mode >= 0 && a->mode <= 2, GV_E_UNSUPPORTED, "gv_adamw_ema_ranges: mode must be 0 (AdamW), 1 (Adam+L2) or 2 (SGD Nesterov); a frozen range is left out of the table");
    GV_REQUIRE(a->n > 0 && a->n % 4 == 0 && a->n <= 0x7fffffffL, GV_E_SHAPE, "gv_adamw_ema_ranges: n=%ld must be a positive multiple of 4 below 2^31 (the table holds int32 offsets)", (long)a->n);
    GV_REQUIRE(gv_aligned(a->p, 16) && gv_aligned(a->grad, 16) && gv_aligned(a->m, 16) && gv_aligned(a->v, 16), GV_E_ALIGN,
               "gv_adamw_ema_ranges: buffers must be 16-byte aligned");
    GV_REQUIRE(gv_aligned(a->p_bf16, 8) && gv_aligned(a->teacher, 16) && gv_aligned(a->teacher_bf16, 8) && gv_aligned(a->blocks, 4) && gv_aligned(a->ranges, 4), GV_E_ALIGN,
               "gv_adamw_ema_ranges: teacher must be 16-byte, the 16-bit copies 8-byte, the tables 4-byte aligned");
    if (a->clip_norm > 0.f) GV_REQUIRE(a->gnorm_sq, GV_E_NULL, "gv_adamw_ema_ranges: clip_norm needs gnorm_sq");
    if (a->loss_scale) GV_REQUIRE(a->gnorm_sq, GV_E_NULL, "gv_adamw_ema_ranges: loss_scale needs gnorm_sq (the finite check)");
    GV_REQUIRE(!(a->clip_norm > 0.f && a->clip_value > 0.f), GV_E_UNSUPPORTED, "gv_adamw_ema_ranges: clip_norm and clip_value exclude each other (--clip-mode norm | value)");
    if (!a->hyper) GV_REQUIRE(a->bias_corr1 > 0.f && a->bias_corr2 > 0.f, GV_E_SHAPE, "gv_adamw_ema_ranges: bias corrections must be > 0");
    const int blocks = a->n_blocks > 4096 ? 4096 : a->n_blocks;
    hipLaunchKernelGGL(adamw_ema_ranges_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_adamw_ema_ranges");
    return GV_OK;
}
