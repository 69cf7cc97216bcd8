// patchify: NHWC uint8 tile crop windows -> normalised bf16 patch rows.
// Replaces the im2col half of PatchEmbed's Conv2d(3, D, 16, 16) (vit.pyc@L167-170)
// fused with the reference's ToTensor + Normalize (transformations.py:124-128) and
// the crop slicing of the multi-crop input contract.
//
// HBM-bound.  One thread per (image, patch, pixel row): reads the 48 contiguous
// bytes of 16 RGB pixels and writes three 32-B runs (one per channel) so that a
// patch row is laid out k = c*256 + py*16 + px, the flatten order of the conv
// weight [D, 3, 16, 16].  A wave covers 4 horizontally adjacent patches x 16 pixel
// rows: reads are 192-B contiguous per pixel row, writes 512-B contiguous per
// (patch, channel).   algorithmic bytes / image: crop^2 * 3 in + (crop/16)^2 * 1536 out.
#include "gv_common.h"
#include "stain_px.h"

namespace {

struct norm_consts { float s0, s1, s2, o0, o1, o2; };

// n(tile, y, x .. x + 15, c): the normalised f32 values of one 16-pixel run of a tile (with its fill box applied) -- the ONE
// place the value is computed, for the plain, the mixing and the stain kernel alike, so all contract it the same way.
// STAIN (gv_patchify_stain): a record `st` with on != 0 maps the run's 16 pixels byte to byte (stain_px, table `odt`) between the
// load and the normalisation; the instantiation without it is the code as it was.
template <bool STAIN = false>
__device__ __forceinline__ void norm_run(const gv_patchify_args& a, const norm_consts& k, int tile, int y, int x, float (&px)[3][16],
                                         const gv_stain_params* st = nullptr, const float* odt = nullptr) {
    const float s0 = k.s0, s1 = k.s1, s2 = k.s2, o0 = k.o0, o1 = k.o1, o2 = k.o2;
    const uint8_t* src = a.tiles + (long)tile * a.img_stride + ((long)y * a.tile_w + x) * 3;

    // 48 bytes at arbitrary alignment -> 12 aligned dwords (+ up to 3 tail bytes)
    const uintptr_t addr = (uintptr_t)src;
    const uint32_t* w = (const uint32_t*)(addr & ~(uintptr_t)3);
    const int mis = (int)(addr & 3);
    uint32_t d[13];
#pragma unroll
    for (int i = 0; i < 12; ++i) d[i] = w[i];
    d[12] = 0;
    if (mis) {
        const uint8_t* tail = (const uint8_t*)(w + 12);
        for (int i = 0; i < mis; ++i) d[12] |= (uint32_t)tail[i] << (8 * i);
    }
    uint32_t u[12];
    if (mis == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) u[i] = d[i];
    } else {
        const int sh = mis * 8;
#pragma unroll
        for (int i = 0; i < 12; ++i) u[i] = (d[i] >> sh) | (d[i + 1] << (32 - sh));
    }
    if constexpr (STAIN) {
        if (st->on) {
            uint32_t v[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = 3 * i;
                const Px q = stain_px(Px{(int)((u[j >> 2] >> (8 * (j & 3))) & 0xFF), (int)((u[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFF),
                                         (int)((u[(j + 2) >> 2] >> (8 * ((j + 2) & 3))) & 0xFF)}, *st, odt);
                v[j >> 2] |= (uint32_t)q.r << (8 * (j & 3));
                v[(j + 1) >> 2] |= (uint32_t)q.g << (8 * ((j + 1) & 3));
                v[(j + 2) >> 2] |= (uint32_t)q.b << (8 * ((j + 2) & 3));
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) u[i] = v[i];
        }
    }
    // byte j of the run = pixel j/3, channel j%3
#pragma unroll
    for (int j = 0; j < 48; ++j) {
        const float v = (float)((u[j >> 2] >> (8 * (j & 3))) & 0xFF);
        const int c = j % 3;
        px[c][j / 3] = v * (c == 0 ? s0 : c == 1 ? s1 : s2) + (c == 0 ? o0 : c == 1 ? o1 : o2);
    }
    if (a.fill) {
        const float* f = a.fill + (long)tile * 8;
        if (f[7] != 0.f && (float)y >= f[0] && (float)y < f[1]) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if ((float)(x + i) >= f[2] && (float)(x + i) < f[3]) { px[0][i] = f[4]; px[1][i] = f[5]; px[2][i] = f[6]; }
        }
    }
}

// one pixel row of one patch: three runs of 16 values (one per channel) at k = c*256 + py*16
template <bool F32OUT> __device__ __forceinline__ void store_run(void* patches, long ip, int py, const float (&px)[3][16]) {
    if constexpr (F32OUT) {
        float* out = (float*)patches + ip * 768 + py * 16;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 16; i += 4) *(f32x4*)(out + c * 256 + i) = f32x4{px[c][i], px[c][i + 1], px[c][i + 2], px[c][i + 3]};
    } else {
        bf16* out = (bf16*)patches + ip * 768 + py * 16;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            bf16x8 lo, hi;
#pragma unroll
            for (int i = 0; i < 8; ++i) { lo[i] = (bf16)px[c][i]; hi[i] = (bf16)px[c][8 + i]; }
            *(bf16x8*)(out + c * 256) = lo;
            *(bf16x8*)(out + c * 256 + 8) = hi;
        }
    }
}

// ---- random erasing (gv_erase_row): the part the u8 and the NCHW kernels share.  The table and the step's seed travel as one
// kernel argument; the instantiations without ERASE never look at it.
struct erase_in { const gv_erase_row* tab; uint32_t seed; };
// A row as the kernels use it: anything that is not a well-formed value / noise row has no boxes.
struct erase_desc { const gv_erase_row* r; int mode, nb; };
__device__ __forceinline__ erase_desc load_erase(const gv_erase_row* tab, int img) {
    const gv_erase_row* r = tab + img;
    const int mode = r->mode, nb = r->n_box;
    const bool ok = (mode == GV_ERASE_VALUE || mode == GV_ERASE_NOISE) && nb >= 0 && nb <= GV_ERASE_MAX_BOXES;
    return erase_desc{r, ok ? mode : GV_ERASE_OFF, ok ? nb : 0};
}
// bit i set: pixel wx + i (i < N <= 16) of window row wy lies in box b.  The pixels of a run all lie in the window, so the box
// is clamped to it by construction.
template <int N> __device__ __forceinline__ unsigned erase_bits(const gv_erase_row* r, int b, int wy, int wx) {
    const int yl = r->box[b][0], yh = r->box[b][1], xl = r->box[b][2], xh = r->box[b][3];
    if (wy < yl || wy >= yh) return 0u;
    const int lo = max(xl, wx), hi = min(xh, wx + N);
    if (hi <= lo) return 0u;
    return ((1u << (hi - wx)) - 1u) & ~((1u << (lo - wx)) - 1u);
}
template <int N> __device__ __forceinline__ unsigned erase_mask(const erase_desc& e, int wy, int wx) {
    unsigned m = 0u;
    for (int b = 0; b < e.nb; ++b) m |= erase_bits<N>(e.r, b, wy, wx);
    return m;
}
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {      // murmur3 finaliser, as drop_keep (rowops.hip)
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
// z(idx): Box-Muller on two hashes of the pixel's index, f32 with the accurate logf / cosf / sqrtf (gipvit.h)
__device__ __forceinline__ float erase_noise(uint32_t seed, uint32_t idx) {
    const uint32_t h1 = fmix32(seed + 0x9E3779B9u * (idx + 1u));
    const uint32_t h2 = fmix32(h1 + 0x6D2B79F5u);
    const float u1 = (float)((h1 >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(h2 >> 8) * 0x1p-24f;
    return sqrtf(-2.0f * logf(u1)) * cosf(6.2831853f * u2);
}
// The erased pixels (bits of `mask`) of NC channels c0 .. of one run: v[j][i] = channel c0 + j, pixel wx + i of window row wy.
template <int NC, int N>
__device__ __forceinline__ void erase_apply(const erase_desc& e, uint32_t seed, int img, int c0, int S, int wy, int wx, unsigned mask, float (&v)[NC][N]) {
    if (e.mode == GV_ERASE_NOISE) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const uint32_t idx = (((uint32_t)img * 3u + (uint32_t)(c0 + j)) * (uint32_t)S + (uint32_t)wy) * (uint32_t)S + (uint32_t)wx;
#pragma unroll
            for (int i = 0; i < N; ++i)
                if ((mask >> i) & 1u) v[j][i] = erase_noise(seed, idx + (uint32_t)i);
        }
    } else {
        for (int b = 0; b < e.nb; ++b) {        // in order: a later box overwrites an earlier one
            const unsigned bits = erase_bits<N>(e.r, b, wy, wx);
            if (!bits) continue;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const float val = e.r->value[b][c0 + j];
#pragma unroll
                for (int i = 0; i < N; ++i)
                    if ((bits >> i) & 1u) v[j][i] = val;
            }
        }
    }
}

// ERASE (gv_patchify_erase without a mix table, n_win == 1): the run's erased pixels are overwritten after normalise + fill; a
// run wholly inside erased boxes reads nothing.
template <bool F32OUT, bool ERASE = false>      // F32OUT: fp32 parity mode, f32 patch rows (f32path.hip)
__global__ __launch_bounds__(256) void patchify_kernel(gv_patchify_args a, int P, int side, norm_consts k, erase_in er) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)a.n_img * P * 16;
    if (t >= total) return;
    const int py = (int)(t & 15);
    const long ip = t >> 4;
    const int patch = (int)(ip % P);
    const int img = (int)(ip / P);
    const int tile = img % a.n_tiles, win = img / a.n_tiles;
    const int prow = patch / side, pcol = patch - prow * side;
    const int y = a.win_y[win] + prow * 16 + py, x = a.win_x[win] + pcol * 16;
    float px[3][16];
    if constexpr (ERASE) {
        const int wy = prow * 16 + py, wx = pcol * 16;       // window coordinates: the boxes' frame
        const erase_desc e = load_erase(er.tab, img);
        const unsigned em = erase_mask<16>(e, wy, wx);
        if (em != 0xFFFFu) norm_run(a, k, tile, y, x, px);
        if (em) erase_apply<3, 16>(e, er.seed, img, 0, a.crop, wy, wx, em, px);
    } else {
        norm_run(a, k, tile, y, x, px);
    }
    store_run<F32OUT>(a.patches, ip, py, px);
}

// ---- patchify_stain (gv_patchify_stain): patchify_kernel with tile t's bytes mapped through record stain[t] first.  Same thread
// mapping and stores; the new work is 48 table look-ups and 48 expf per thread of a tile whose record is on.  The od table is the
// same for every record, so a workgroup builds it once if any of its threads needs it (a workgroup may span tiles); one whose
// tiles are all off takes the barrier and nothing else.
template <bool F32OUT>
__global__ __launch_bounds__(256) void patchify_stain_kernel(gv_patchify_args a, const gv_stain_params* stain, int P, int side, norm_consts k) {
    __shared__ float odt[256];
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)a.n_img * P * 16;
    const bool live = t < total;
    const int py = (int)(t & 15);
    const long ip = t >> 4;
    const int patch = (int)(ip % P);
    const int img = (int)(ip / P);
    const int tile = img % a.n_tiles, win = img / a.n_tiles;
    gv_stain_params st;
    st.on = 0;
    if (live) st = stain[tile];
    if (__syncthreads_or(st.on != 0)) {
        odt[threadIdx.x] = stain_od_entry(threadIdx.x);
        __syncthreads();
    }
    if (!live) return;
    const int prow = patch / side, pcol = patch - prow * side;
    const int y = a.win_y[win] + prow * 16 + py, x = a.win_x[win] + pcol * 16;
    float px[3][16];
    norm_run<true>(a, k, tile, y, x, px, &st, odt);
    store_run<F32OUT>(a.patches, ip, py, px);
}

// mixup's two products and their sum, each rounded on its own (torch: x.mul(lam).add(x.flip(0).mul(1 - lam))): no FMA
__device__ __forceinline__ float mix_blend(float vi, float vj, float lam, float oml) {
#pragma clang fp contract(off)
    const float a = vi * lam;
    const float b = vj * oml;
    return a + b;
}

// A mix row as the kernels use it: anything that is not a well-formed blend / paste row is a copy row.
struct mix_desc { int partner, mode; float lam, oml; int yl, yh, xl, xh; };
__device__ __forceinline__ mix_desc load_mix(const gv_mix_row* mix, int img, int n_tiles) {
    const gv_mix_row r = mix[img];
    mix_desc m{r.partner, r.mode, r.lam, r.one_minus_lam, r.yl, r.yh, r.xl, r.xh};
    if ((unsigned)m.partner >= (unsigned)n_tiles || (m.mode != GV_MIX_BLEND && m.mode != GV_MIX_PASTE)) m.mode = GV_MIX_COPY;
    return m;
}

// ---- patchify_mix: patchify with timm's Mixup applied to the batch inside the same pass (gv_patchify_mix_args).  Same
// thread mapping and store pattern as patchify_kernel; the only new traffic is the partner tile's 48 bytes per thread, read
// by blend rows and by the threads of a paste row whose run meets the box (a run wholly inside it skips its own tile instead).
// ERASE: as in patchify_kernel, after the mixing; a run wholly inside erased boxes reads neither source.
template <bool F32OUT, bool ERASE = false>
__global__ __launch_bounds__(256) void patchify_mix_kernel(gv_patchify_args a, const gv_mix_row* mix, int P, int side, norm_consts k, erase_in er) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)a.n_img * P * 16;
    if (t >= total) return;
    const int py = (int)(t & 15);
    const long ip = t >> 4;
    const int patch = (int)(ip % P);
    const int img = (int)(ip / P);                       // n_win == 1: image = tile
    const int prow = patch / side, pcol = patch - prow * side;
    const int wy = prow * 16 + py, wx = pcol * 16;       // window coordinates: the box's frame
    const int y = a.win_y[0] + wy, x = a.win_x[0] + wx;
    const mix_desc m = load_mix(mix, img, a.n_tiles);
    // a paste row's run: outside the box, wholly inside it (the partner alone is read), or cut by one of its sides
    const bool meets = m.mode == GV_MIX_PASTE && wy >= m.yl && wy < m.yh && wx < m.xh && wx + 16 > m.xl;
    const bool whole = meets && wx >= m.xl && wx + 16 <= m.xh;
    const bool blend = m.mode == GV_MIX_BLEND;
    float px[3][16];
    erase_desc e{nullptr, GV_ERASE_OFF, 0};
    unsigned em = 0u;
    if constexpr (ERASE) {
        e = load_erase(er.tab, img);
        em = erase_mask<16>(e, wy, wx);
    }
    if (!ERASE || em != 0xFFFFu) {
        norm_run(a, k, whole ? m.partner : img, y, x, px);
        if (blend || (meets && !whole)) {
            float pj[3][16];
            norm_run(a, k, m.partner, y, x, pj);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool in = wx + i >= m.xl && wx + i < m.xh;
#pragma unroll
                for (int c = 0; c < 3; ++c) px[c][i] = blend ? mix_blend(px[c][i], pj[c][i], m.lam, m.oml) : (in ? pj[c][i] : px[c][i]);
            }
        }
    }
    if constexpr (ERASE) {
        if (em) erase_apply<3, 16>(e, er.seed, img, 0, a.crop, wy, wx, em, px);
    }
    store_run<F32OUT>(a.patches, ip, py, px);
}

// ---- random-resized-crop (+ horizontal flip) of NHWC u8 tiles: the DINO multi-crop input
// stage.  Semantics = torchvision's tensor-mode resized_crop with
// antialias off: the box (y0, x0, h, w) of the tile is resampled to out x out with
// F.interpolate(float32, mode='bilinear', align_corners=False), rounded half-to-even and
// clamped to u8; flip mirrors the OUTPUT columns.  One thread per 4 output pixels (12
// contiguous bytes); float32 arithmetic in the oracle's association, no FMA contraction,
// so the bytes are reproducible against the CPU restatement.
__global__ __launch_bounds__(256) void crop_resize_kernel(gv_crop_resize_args a) {
#pragma clang fp contract(off)
    const int out = a.out_size, q = out >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)a.n_crops * out * q;
    if (t >= total) return;
    const int xq = (int)(t % q);
    const int oy = (int)((t / q) % out);
    const int n = (int)(t / ((long)q * out));
    const int* bx = a.boxes + n * 6;
    const int tile = bx[0], y0 = bx[1], x0 = bx[2], h = bx[3], w = bx[4], flip = bx[5];
    const uint8_t* src = a.tiles + (long)tile * a.tile_h * a.tile_w * 3;
    const float sy = (float)h / (float)out, sx = (float)w / (float)out;
    float fy = sy * ((float)oy + 0.5f) - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    const int iy0 = (int)fy, iy1 = iy0 + (iy0 < h - 1 ? 1 : 0);
    const float ly = fy - (float)iy0, ly0 = 1.0f - ly;
    const uint8_t* r0 = src + ((long)(y0 + iy0) * a.tile_w + x0) * 3;
    const uint8_t* r1 = src + ((long)(y0 + iy1) * a.tile_w + x0) * 3;
    uint32_t pk[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int oxo = xq * 4 + i;                       // output column
        const int ox = flip ? out - 1 - oxo : oxo;        // column of the un-flipped resample
        float fx = sx * ((float)ox + 0.5f) - 0.5f;
        fx = fx < 0.f ? 0.f : fx;
        const int ix0 = (int)fx, ix1 = ix0 + (ix0 < w - 1 ? 1 : 0);
        const float lx = fx - (float)ix0, lx0 = 1.0f - lx;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = lx0 * (float)r0[ix0 * 3 + c] + lx * (float)r0[ix1 * 3 + c];
            const float bot = lx0 * (float)r1[ix0 * 3 + c] + lx * (float)r1[ix1 * 3 + c];
            float v = __builtin_rintf(ly0 * top + ly * bot);
            v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
            const int b = i * 3 + c;
            pk[b >> 2] |= (uint32_t)v << (8 * (b & 3));
        }
    }
    uint32_t* dst = (uint32_t*)(a.out + ((long)n * out * out + (long)oy * out + xq * 4) * 3);
    dst[0] = pk[0]; dst[1] = pk[1]; dst[2] = pk[2];
}


// ---- patchify_nchw: crop windows of an ALREADY NORMALISED float32 NCHW batch -> patch rows (the reference's own
// input, Data [B, 3, H, W] after ToTensor + Normalize, train.py:1027-1033).  Same output layout as patchify; no mean / std:
// the value is only rounded to the build's 16-bit format (RNE, the hardware convert: bit-equal to torch's .to()) or copied
// (f32 rows).  HBM-bound: algorithmic bytes / image crop^2 * 12 in + (crop/16)^2 * 768 * sizeof(out) out.
//
// One workgroup per strip of up to 16 patches of one patch row: phase 1 reads its 3 channels x 16 pixel rows with 16-B loads
// (a row segment is contiguous in W; NCHW_U loads in flight per lane) and stores them converted into an LDS image
// [c][py][x]; phase 2 writes the strip's patch rows -- one contiguous run of n_patch * 768 elements -- with 16-B stores, each
// lane's 16 B being 16 B of one LDS image row.  A row segment that does not start 16-B aligned (a window at an odd column, an
// odd stride) takes four 4-B loads per item instead.
constexpr int NCHW_MAXP = 16, NCHW_U = 6;

__device__ __forceinline__ f32x4 nchw_load4(const float* src) {
    if (((uintptr_t)src & 15) == 0) return *(const f32x4*)src;
    return f32x4{src[0], src[1], src[2], src[3]};
}

// bit i set: pixel wx + i of window row wy lies in a paste row's box (0 for copy and blend rows)
__device__ __forceinline__ int paste_mask4(const mix_desc& m, int wy, int wx) {
    int mask = 0;
    if (m.mode == GV_MIX_PASTE && wy >= m.yl && wy < m.yh) {
#pragma unroll
        for (int i = 0; i < 4; ++i) mask |= (wx + i >= m.xl && wx + i < m.xh) ? 1 << i : 0;
    }
    return mask;
}

// MIX (gv_patchify_nchw_mix, n_win == 1): phase 1 takes each 4-pixel item from the image, from its partner or from both, as
// the image's mix row says; everything else is the plain kernel.
// ERASE (gv_patchify_nchw_erase, n_win == 1): the image's erase row is the workgroup's; a strip that meets none of its boxes runs
// the loop of the kernel without it, in one that does an item wholly inside erased boxes loads nothing and the erased pixels are
// overwritten after the combine.
template <typename OT, bool MIX, bool ERASE = false>
__global__ __launch_bounds__(256) void patchify_nchw_kernel(gv_patchify_nchw_args a, int side, int n_chunk, const gv_mix_row* mix, erase_in er) {
    constexpr int V = 16 / (int)sizeof(OT);                       // elements per 16-B store
    // items per lane and round: MIX holds two sources per item, so half as many keep the loads in flight (and the registers,
    // hence the workgroups per CU that overlap one strip's loads with another's stores) where the plain kernel has them
    constexpr int U = MIX ? NCHW_U / 2 : NCHW_U;
    constexpr int ROW = NCHW_MAXP * 16 + 16 / (int)sizeof(OT);    // LDS image row (+16 B: rows start on different banks)
    __shared__ __attribute__((aligned(16))) OT img_lds[3 * 16 * ROW];
    const int bid = blockIdx.x;
    const int chunk = bid % n_chunk, prow = (bid / n_chunk) % side, img = bid / (n_chunk * side);
    const int tile = img % a.n_tiles, win = img / a.n_tiles;
    const int p0 = chunk * NCHW_MAXP, np = min(NCHW_MAXP, side - p0);
    const int y0 = a.win_y[win] + prow * 16, x0 = a.win_x[win] + p0 * 16;
    const float* base = a.images + (long)tile * a.stride_n + (long)y0 * a.stride_h + x0;
    // phase 1: item = (channel, pixel row, 4-pixel group); 48 row segments of np * 16 pixels
    const int q = np * 4, n_items = 48 * q;
    mix_desc m{0, GV_MIX_COPY, 1.f, 0.f, 0, 0, 0, 0};
    long pdelta = 0;                                                // partner image - this image, in elements
    if constexpr (MIX) {
        m = load_mix(mix, img, a.n_tiles);
        if (m.mode != GV_MIX_COPY) pdelta = (long)(m.partner - tile) * a.stride_n;
    }
    erase_desc e{nullptr, GV_ERASE_OFF, 0};
    if constexpr (ERASE) {
        e = load_erase(er.tab, img);
        bool hit = false;                                           // does a box meet this strip's 16 rows x np * 16 columns?
        for (int b = 0; b < e.nb; ++b) {
            const int* bx = e.r->box[b];
            hit |= bx[0] < prow * 16 + 16 && bx[1] > prow * 16 && bx[2] < (p0 + np) * 16 && bx[3] > p0 * 16 && bx[0] < bx[1] && bx[2] < bx[3];
        }
        if (!hit) e.nb = 0;
    }
    for (int b0 = threadIdx.x; b0 < n_items; b0 += 256 * U) {
        f32x4 v[U];
        unsigned em[ERASE ? U : 1];                                 // ERASE: which of the item's 4 pixels are erased
        // MIX: w = the partner's 4 pixels, pm = which of the 4 a paste row takes from it.  Every load of the batch of items is
        // issued before the first value is used (the combine waits for the second loop), as in the plain kernel.
        f32x4 w[MIX ? U : 1];
        int pm[MIX ? U : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int it = b0 + u * 256;
            if (it < n_items) {
                const int seg = it / q, g = it - seg * q;
                const float* src = base + (long)(seg >> 4) * a.stride_c + (long)(seg & 15) * a.stride_h + g * 4;
                bool live = true;                                   // false: all 4 pixels are erased, nothing is read
                if constexpr (ERASE) {
                    em[u] = erase_mask<4>(e, prow * 16 + (seg & 15), p0 * 16 + g * 4);
                    live = em[u] != 15u;
                }
                if constexpr (!MIX) {
                    if constexpr (ERASE) v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (live) v[u] = nchw_load4(src);
                } else {
                    pm[u] = paste_mask4(m, prow * 16 + (seg & 15), p0 * 16 + g * 4);
                    const bool blend = m.mode == GV_MIX_BLEND;
                    v[u] = w[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (live && (blend || pm[u] != 15)) v[u] = nchw_load4(src);
                    if (live && (blend || pm[u] != 0)) w[u] = nchw_load4(src + pdelta);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int it = b0 + u * 256;
            if (it < n_items) {
                const int seg = it / q, g = it - seg * q;
                if constexpr (MIX) {
                    if (m.mode == GV_MIX_BLEND) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[u][i] = mix_blend(v[u][i], w[u][i], m.lam, m.oml);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[u][i] = ((pm[u] >> i) & 1) ? w[u][i] : v[u][i];
                    }
                }
                if constexpr (ERASE) {
                    if (em[u]) {
                        float t[1][4] = {{v[u][0], v[u][1], v[u][2], v[u][3]}};
                        erase_apply<1, 4>(e, er.seed, img, seg >> 4, a.crop, prow * 16 + (seg & 15), p0 * 16 + g * 4, em[u], t);
                        v[u] = f32x4{t[0][0], t[0][1], t[0][2], t[0][3]};
                    }
                }
                OT* d = img_lds + seg * ROW + g * 4;
                if constexpr (sizeof(OT) == 4) {
                    *(f32x4*)d = v[u];
                } else {
                    bf16x4 o;
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] = (bf16)v[u][i];
                    *(bf16x4*)d = o;
                }
            }
        }
    }
    __syncthreads();
    // phase 2: the strip's rows [(img * side + prow) * side + p0, + np) x 768, contiguous; element e = p*768 + c*256 + py*16 + px
    OT* out = (OT*)a.patches + ((long)(img * side + prow) * side + p0) * 768;
    const int n_out = np * 768 / V;
    for (int o = threadIdx.x; o < n_out; o += 256) {
        const int e = o * V;
        const int p = e / 768, k = e - p * 768;
        const int c = k >> 8, py = (k >> 4) & 15, px = k & 15;
        const OT* s = img_lds + (c * 16 + py) * ROW + p * 16 + px;
        if constexpr (sizeof(OT) == 4) {
            *(f32x4*)(out + e) = *(const f32x4*)s;
        } else {
            *(bf16x8*)(out + e) = *(const bf16x8*)s;
        }
    }
}

}  // namespace

extern "C" int gv_crop_resize(const gv_crop_resize_args* a, void* stream) {
    GV_REQUIRE(a && a->tiles && a->out && a->boxes, GV_E_NULL, "gv_crop_resize: null pointer");
    GV_REQUIRE(a->n_crops > 0 && a->n_tiles > 0 && a->tile_h > 0 && a->tile_w > 0, GV_E_SHAPE, "gv_crop_resize: bad shape");
    GV_REQUIRE(a->out_size > 0 && a->out_size % 4 == 0, GV_E_SHAPE, "gv_crop_resize: out_size=%d must be a positive multiple of 4", a->out_size);
    GV_REQUIRE(gv_aligned(a->out, 4) && gv_aligned(a->boxes, 4), GV_E_ALIGN, "gv_crop_resize: out / boxes must be 4-byte aligned");
    const long total = (long)a->n_crops * a->out_size * (a->out_size / 4);
    hipLaunchKernelGGL(crop_resize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    GV_LAUNCH_CHECK("gv_crop_resize");
    return GV_OK;
}

// What an entry point with an erase table adds to the checks of the plain / mix launch (`crop` is validated by the caller first).
static int erase_check(const char* name, const gv_mix_row* mix, const erase_in* er, int n_win, int n_img, int crop) {
    GV_REQUIRE(er->tab, GV_E_NULL, "%s: null erase table", name);
    GV_REQUIRE(gv_aligned(er->tab, 4), GV_E_ALIGN, "%s: the erase table must be 4-byte aligned", name);
    GV_REQUIRE(gv_aligned(mix, 4), GV_E_ALIGN, "%s: the mix table must be 4-byte aligned", name);
    GV_REQUIRE(n_win == 1, GV_E_SHAPE, "%s: n_win=%d, one window only (the boxes are in the window's coordinates)", name, n_win);
    GV_REQUIRE((long)n_img * 3 * crop * crop < (1L << 32), GV_E_SHAPE,
               "%s: n_img * 3 * crop^2 = %ld, the noise generator's pixel index needs < 2^32", name, (long)n_img * 3 * crop * crop);
    return GV_OK;
}

// mix == nullptr: gv_patchify; else gv_patchify_mix (has_mix says which was called: a NULL table is then an error).  er: the call
// is gv_patchify_erase, with or without a mix table.
// stain: the call is gv_patchify_stain (has_stain says so: a NULL table is then an error), without mix / erase tables.
template <bool F32OUT> static int patchify_launch(const gv_patchify_args* a, void* stream, const gv_mix_row* mix = nullptr, bool has_mix = false,
                                                  const erase_in* er = nullptr, const gv_stain_params* stain = nullptr, bool has_stain = false) {
    GV_REQUIRE(a && a->tiles && a->patches, GV_E_NULL, "gv_patchify: null pointer");
    if (has_stain) {
        GV_REQUIRE(stain, GV_E_NULL, "gv_patchify_stain: null stain table");
        GV_REQUIRE(gv_aligned(stain, 4), GV_E_ALIGN, "gv_patchify_stain: the stain table must be 4-byte aligned");
    }
    if (has_mix) {
        GV_REQUIRE(mix, GV_E_NULL, "gv_patchify_mix: null mix table");
        GV_REQUIRE(gv_aligned(mix, 4), GV_E_ALIGN, "gv_patchify_mix: the mix table must be 4-byte aligned");
        GV_REQUIRE(a->n_win == 1, GV_E_SHAPE, "gv_patchify_mix: n_win=%d, one window only (the batch is mixed as a whole)", a->n_win);
    }
    GV_REQUIRE(a->crop > 0 && a->crop % 16 == 0, GV_E_SHAPE, "gv_patchify: crop=%d must be a positive multiple of 16", a->crop);
    GV_REQUIRE(a->n_win >= 1 && a->n_win <= 16 && a->n_tiles >= 1 && a->n_img == a->n_win * a->n_tiles, GV_E_SHAPE,
               "gv_patchify: n_img (%d) must equal n_win (%d) * n_tiles (%d), n_win <= 16", a->n_img, a->n_win, a->n_tiles);
    for (int w = 0; w < a->n_win; ++w)
        GV_REQUIRE(a->win_y[w] >= 0 && a->win_x[w] >= 0 && a->win_y[w] + a->crop <= a->tile_h && a->win_x[w] + a->crop <= a->tile_w,
                   GV_E_SHAPE, "gv_patchify: window %d (%d,%d)+%d leaves the %dx%d tile", w, a->win_y[w], a->win_x[w], a->crop, a->tile_h, a->tile_w);
    GV_REQUIRE(gv_aligned(a->patches, 16), GV_E_ALIGN, "gv_patchify: patches must be 16-byte aligned");
    for (int c = 0; c < 3; ++c) GV_REQUIRE(a->std[c] > 0.f, GV_E_SHAPE, "gv_patchify: std must be > 0");
    const int side = a->crop / 16, P = side * side;
    const long total = (long)a->n_img * P * 16;
    const float s0 = 1.0f / (255.0f * a->std[0]), s1 = 1.0f / (255.0f * a->std[1]), s2 = 1.0f / (255.0f * a->std[2]);
    const float o0 = -a->mean[0] / a->std[0], o1 = -a->mean[1] / a->std[1], o2 = -a->mean[2] / a->std[2];
    const norm_consts k{s0, s1, s2, o0, o1, o2};
    const dim3 grid((unsigned)((total + 255) / 256));
    if (has_stain) {
        hipLaunchKernelGGL((patchify_stain_kernel<F32OUT>), grid, dim3(256), 0, (hipStream_t)stream, *a, stain, P, side, k);
        GV_LAUNCH_CHECK("gv_patchify_stain");
        return GV_OK;
    }
    if (er) {
        if (const int rc = erase_check("gv_patchify_erase", mix, er, a->n_win, a->n_img, a->crop)) return rc;
        if (mix)
            hipLaunchKernelGGL((patchify_mix_kernel<F32OUT, true>), grid, dim3(256), 0, (hipStream_t)stream, *a, mix, P, side, k, *er);
        else
            hipLaunchKernelGGL((patchify_kernel<F32OUT, true>), grid, dim3(256), 0, (hipStream_t)stream, *a, P, side, k, *er);
        GV_LAUNCH_CHECK("gv_patchify_erase");
        return GV_OK;
    }
    if (has_mix) {
        hipLaunchKernelGGL((patchify_mix_kernel<F32OUT, false>), grid, dim3(256), 0, (hipStream_t)stream, *a, mix, P, side, k, erase_in{nullptr, 0u});
        GV_LAUNCH_CHECK("gv_patchify_mix");
        return GV_OK;
    }
    hipLaunchKernelGGL((patchify_kernel<F32OUT, false>), grid, dim3(256), 0, (hipStream_t)stream, *a, P, side, k, erase_in{nullptr, 0u});
    GV_LAUNCH_CHECK("gv_patchify");
    return GV_OK;
}
extern "C" int gv_patchify_erase(const gv_patchify_erase_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_erase: null pointer");
    const erase_in er{a->erase, a->seed};
    return patchify_launch<false>(&a->p, stream, a->mix, false, &er);
}
extern "C" int gv_patchify_erase_f32(const gv_patchify_erase_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_erase_f32: null pointer");
    const erase_in er{a->erase, a->seed};
    return patchify_launch<true>(&a->p, stream, a->mix, false, &er);
}
extern "C" int gv_patchify_stain(const gv_patchify_stain_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_stain: null pointer");
    return patchify_launch<false>(&a->p, stream, nullptr, false, nullptr, a->stain, true);
}
extern "C" int gv_patchify_stain_f32(const gv_patchify_stain_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_stain_f32: null pointer");
    return patchify_launch<true>(&a->p, stream, nullptr, false, nullptr, a->stain, true);
}
extern "C" int gv_patchify(const gv_patchify_args* a, void* stream) { return patchify_launch<false>(a, stream); }
extern "C" int gv_patchify_f32(const gv_patchify_args* a, void* stream) { return patchify_launch<true>(a, stream); }
extern "C" int gv_patchify_mix(const gv_patchify_mix_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_mix: null pointer");
    return patchify_launch<false>(&a->p, stream, a->mix, true);
}
extern "C" int gv_patchify_mix_f32(const gv_patchify_mix_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_mix_f32: null pointer");
    return patchify_launch<true>(&a->p, stream, a->mix, true);
}

template <typename OT> static int patchify_nchw_launch(const gv_patchify_nchw_args* a, void* stream, const char* name,
                                                       const gv_mix_row* mix = nullptr, bool has_mix = false, const erase_in* er = nullptr) {
    GV_REQUIRE(a && a->images && a->patches, GV_E_NULL, "%s: null pointer", name);
    if (has_mix) {
        GV_REQUIRE(mix, GV_E_NULL, "%s: null mix table", name);
        GV_REQUIRE(gv_aligned(mix, 4), GV_E_ALIGN, "%s: the mix table must be 4-byte aligned", name);
        GV_REQUIRE(a->n_win == 1, GV_E_SHAPE, "%s: n_win=%d, one window only (the batch is mixed as a whole)", name, a->n_win);
    }
    GV_REQUIRE(a->crop > 0 && a->crop % 16 == 0, GV_E_SHAPE, "%s: crop=%d must be a positive multiple of 16", name, a->crop);
    GV_REQUIRE(a->n_win >= 1 && a->n_win <= 16 && a->n_tiles >= 1 && a->n_img == a->n_win * a->n_tiles, GV_E_SHAPE,
               "%s: n_img (%d) must equal n_win (%d) * n_tiles (%d), 1 <= n_win <= 16", name, a->n_img, a->n_win, a->n_tiles);
    GV_REQUIRE(a->img_h > 0 && a->img_w > 0 && a->stride_n >= 0 && a->stride_c >= 0 && a->stride_h >= 0, GV_E_SHAPE,
               "%s: bad image shape %dx%d or negative stride", name, a->img_h, a->img_w);
    for (int w = 0; w < a->n_win; ++w)
        GV_REQUIRE(a->win_y[w] >= 0 && a->win_x[w] >= 0 && a->win_y[w] + a->crop <= a->img_h && a->win_x[w] + a->crop <= a->img_w,
                   GV_E_SHAPE, "%s: window %d (%d,%d)+%d leaves the %dx%d image", name, w, a->win_y[w], a->win_x[w], a->crop, a->img_h, a->img_w);
    GV_REQUIRE(gv_aligned(a->images, 4), GV_E_ALIGN, "%s: images must be 4-byte aligned", name);
    GV_REQUIRE(gv_aligned(a->patches, 16), GV_E_ALIGN, "%s: patches must be 16-byte aligned", name);
    const int side = a->crop / 16, n_chunk = (side + NCHW_MAXP - 1) / NCHW_MAXP;
    const long blocks = (long)a->n_img * side * n_chunk;
    GV_REQUIRE(blocks < (1L << 31), GV_E_SHAPE, "%s: %ld workgroups exceed the grid", name, blocks);
    const dim3 grid((unsigned)blocks);
    const erase_in none{nullptr, 0u};
    if (er) {
        if (const int rc = erase_check(name, mix, er, a->n_win, a->n_img, a->crop)) return rc;
        if (mix)
            hipLaunchKernelGGL((patchify_nchw_kernel<OT, true, true>), grid, dim3(256), 0, (hipStream_t)stream, *a, side, n_chunk, mix, *er);
        else
            hipLaunchKernelGGL((patchify_nchw_kernel<OT, false, true>), grid, dim3(256), 0, (hipStream_t)stream, *a, side, n_chunk, mix, *er);
    } else if (has_mix) {
        hipLaunchKernelGGL((patchify_nchw_kernel<OT, true, false>), grid, dim3(256), 0, (hipStream_t)stream, *a, side, n_chunk, mix, none);
    } else {
        hipLaunchKernelGGL((patchify_nchw_kernel<OT, false, false>), grid, dim3(256), 0, (hipStream_t)stream, *a, side, n_chunk, mix, none);
    }
    GV_LAUNCH_CHECK(name);
    return GV_OK;
}
extern "C" int gv_patchify_nchw_erase(const gv_patchify_nchw_erase_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_nchw_erase: null pointer");
    const erase_in er{a->erase, a->seed};
    return patchify_nchw_launch<bf16>(&a->p, stream, "gv_patchify_nchw_erase", a->mix, false, &er);
}
extern "C" int gv_patchify_nchw_erase_f32(const gv_patchify_nchw_erase_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_nchw_erase_f32: null pointer");
    const erase_in er{a->erase, a->seed};
    return patchify_nchw_launch<float>(&a->p, stream, "gv_patchify_nchw_erase_f32", a->mix, false, &er);
}
extern "C" int gv_patchify_nchw_mix(const gv_patchify_nchw_mix_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_nchw_mix: null pointer");
    return patchify_nchw_launch<bf16>(&a->p, stream, "gv_patchify_nchw_mix", a->mix, true);
}
extern "C" int gv_patchify_nchw_mix_f32(const gv_patchify_nchw_mix_args* a, void* stream) {
    GV_REQUIRE(a, GV_E_NULL, "gv_patchify_nchw_mix_f32: null pointer");
    return patchify_nchw_launch<float>(&a->p, stream, "gv_patchify_nchw_mix_f32", a->mix, true);
}
extern "C" int gv_patchify_nchw(const gv_patchify_nchw_args* a, void* stream) { return patchify_nchw_launch<bf16>(a, stream, "gv_patchify_nchw"); }
extern "C" int gv_patchify_nchw_f32(const gv_patchify_nchw_args* a, void* stream) {
    return patchify_nchw_launch<float>(a, stream, "gv_patchify_nchw_f32");
}
