// The attention kernels' common LDS image and fragment helpers, and their entry points' common checks (attention.hip,
// attention_stream.hip, attention_stream_bwd.hip, attention_probs_stream.hip; each includes attn_plan.h first).
//
// LDS image: [rows = tokens][64 d] bf16, 128-B rows, 16-B chunk index XOR (row & 7).  Filled by LDS-DMA with the swizzle on
// the per-lane SOURCE address.  The same image serves k-contiguous fragment reads (ds_read_b128) and hardware-transposed
// reads (ds_read_b64_tr_b16: 4 rows x 16 columns per 16-lane group), both conflict-free.
//
// Included inside each file's anonymous namespace: every translation unit has its own copy (and its own zero page).
#pragma once
#include <initializer_list>

// What every entry point checks first, in the order it always has: pointers, then the shape against the limit `max_n` of
// include/gipvit.h.  full_text: the wording of gv_attention_probs and the streaming calls, which name every condition.
template <class A> int attn_check(const char* name, const A* a, bool pointers_ok, int max_n, bool full_text) {
    GV_REQUIRE(pointers_ok, GV_E_NULL, "%s: null pointer", name);
    GV_REQUIRE(gvattn::shape_ok(a->n_img, a->H, a->N, max_n), GV_E_SHAPE,
               full_text ? "%s: need n_img > 0, H > 0, 0 < N <= %d (got N = %d)" : "%s: need 0 < N <= %d (got %d)", name, max_n, a->N);
    return GV_OK;
}
// ... and last: the buffers the kernels read and write in 16-byte pieces
inline int attn_aligned(const char* name, const char* what, std::initializer_list<const void*> buffers) {
    for (const void* p : buffers) GV_REQUIRE(gv_aligned(p, 16), GV_E_ALIGN, "%s: %s must be 16-byte aligned", name, what);
    return GV_OK;
}

__device__ __attribute__((aligned(256))) unsigned short attn_zero_page[128];

__device__ __forceinline__ void glds16(const void* src, GV_LDS char* dst) {
    __builtin_amdgcn_global_load_lds((const GV_GLOBAL void*)src, (GV_LDS void*)dst, 16, 0, 0);
}

// stage rows [0, nrows_pad) of a [token][64] slice; rows >= nvalid are zero filled
__device__ __forceinline__ void stage_rows(const bf16* __restrict__ gbase, long ld, int nvalid, int nrows_pad,
                                           GV_LDS char* img, int wave, int nwaves, int lane) {
    const int pieces = nrows_pad >> 3;
    for (int piece = wave; piece < pieces; piece += nwaves) {
        const int r = piece * 8 + (lane >> 3);
        const int slot = lane & 7;
        const int c = slot ^ (r & 7);
        const bf16* src = r < nvalid ? gbase + (long)r * ld + c * 8 : (const bf16*)attn_zero_page + slot * 8;
        glds16(src, img + __builtin_amdgcn_readfirstlane(piece * 1024));
    }
}

__device__ __forceinline__ bf16x8 read_nat(GV_LDS char* img, int row, int chunk) {
    return *(GV_LDS bf16x8*)(img + row * 128 + ((chunk ^ (row & 7)) << 4));
}
// transposed read: this lane addresses `row`, 16-column block dt, quarter p (0..3)
__device__ __forceinline__ bf16x4 read_tr(GV_LDS char* img, int row, int dt, int p) {
    const int c16 = 2 * dt + (p >> 1);
    return GV_DS_READ_TR16(img + row * 128 + ((c16 ^ (row & 7)) << 4) + 8 * (p & 1));
}
__device__ __forceinline__ bf16x8 cat8(bf16x4 lo, bf16x4 hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ bf16x8 pack8(f32x4 a, f32x4 b) {
    return bf16x8{(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
}
template <int LO, int HI, class F>
__device__ __forceinline__ void attn_static_for(F&& f) {
    if constexpr (LO < HI) { f(std::integral_constant<int, LO>{}); attn_static_for<LO + 1, HI>(f); }
}
#define MFMA16(a, b, c) GV_MFMA_16x16x32((a), (b), (c))
