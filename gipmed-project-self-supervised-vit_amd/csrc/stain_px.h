// The optical-density map of one pixel (gv_stain_params, include/gipvit.h): the ONE place it is evaluated, for the crop pass
// (augment.hip: stain jitter), gv_stain_apply (stainnorm.hip) and gv_patchify_stain (patch.hip: stain normalisation), so the
// three produce the same byte for the same record.
#pragma once
#include "gv_common.h"

namespace {

struct Px { int r, g, b; };

// entry v of a block's 256-entry table of -ln((v + 1) / 256): the fp64 value, rounded once to f32
__device__ __forceinline__ float stain_od_entry(int v) { return (float)(-log((double)(v + 1) * (1.0 / 256.0))); }

// od comes from `odt`, the block's table; od' is summed left to right without contraction, exp is the accurate library
// function: a result is off the fp64 one by less than 1e-4 of a grey level, so the rounded byte differs only within that
// distance of a tie.
__device__ __forceinline__ Px stain_px(const Px p, const gv_stain_params& s, const float* odt) {
#pragma clang fp contract(off)
    const float od[3] = {odt[p.r], odt[p.g], odt[p.b]};
    int c3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = od[0] * s.A[c] + od[1] * s.A[3 + c] + od[2] * s.A[6 + c] + s.b[c];
        c3[c] = (int)fminf(fmaxf(rintf(256.0f * expf(-t) - 1.0f), 0.f), 255.f);
    }
    return Px{c3[0], c3[1], c3[2]};
}

}  // namespace
