/*
 * gipvit.h -- C ABI of libgipvit_hip.so: the MI355X (gfx950) implementation of the
 * ViT-encoder + DINO multi-crop training hot path of
 * noam-mosh/GipMed-Project-Self-Supervised-ViT.
 *
 * The reference has no FFI of its own for this path: the arithmetic is reached
 * through ATen library calls issued by timm's VisionTransformer
 * (reference train.py:482-495 create_model, train.py:1044-1078 step) and by the
 * orphaned nn_encoder_arch ViT / DINOHead bytecode (cited
 * below as vit.pyc@L<n>).  Each entry point names the reference call it replaces.
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (tensor.data_ptr());
 *     the library allocates nothing, keeps no reference after return, and only
 *     enqueues kernels on `stream` (a hipStream_t passed as void*); it never
 *     synchronises, so every call is hipGraph-capturable;
 *   - return 0 on success, <0 = GV_E_* argument error (message in
 *     gv_last_error(), thread local), >0 = hipError_t of a failed launch;
 *   - "bf16" buffers hold the library build's 16-bit format (uint16_t patterns): bfloat16 in libgipvit_hip.so, IEEE
 *     half in libgipvit_hip_f16.so -- the same sources built with -DGV_ACT_F16 for the reference's
 *     --amp --amp-dtype float16 (train.py:452-465); gv_act_format() says which.  "f32" is IEEE float;
 *   - matrices are row-major with an explicit leading dimension in ELEMENTS.
 */
#ifndef GIPVIT_H
#define GIPVIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GV_ABI_VERSION 9
enum { GV_HYP_LR = 0, GV_HYP_WD, GV_HYP_BC1, GV_HYP_BC2, GV_HYP_TEACHER_MOM, GV_HYP_GRAD_SCALE,
       GV_HYP_TEACHER_TEMP, GV_HYP_STUDENT_TEMP, GV_HYP_COUNT };

enum {
    GV_OK = 0,
    GV_E_SHAPE = -1,      /* unsupported / inconsistent shape            */
    GV_E_ALIGN = -2,      /* pointer or leading dimension misaligned     */
    GV_E_NULL = -3,       /* required pointer is NULL                    */
    GV_E_UNSUPPORTED = -4 /* flag / dtype combination not built          */
};

/* ---- library ---------------------------------------------------------- */
int gv_version(void);
const char* gv_last_error(void);
/* name of the gfx target the kernels were compiled for ("gfx950") */
const char* gv_target(void);
/* the 16-bit operand / activation format this library was built for */
enum { GV_ACT_FORMAT_BF16 = 0, GV_ACT_FORMAT_F16 = 1 };
int gv_act_format(void);

/* ---- patchify: replaces PatchEmbed's Conv2d im2col on the reference input
 * contract (vit.pyc@L167-170; datasets.py:614-631 -> transformations.py:124-128
 * ToTensor + Normalize).  Reads crop windows of NHWC uint8 tiles, applies
 * (u8/255 - mean[c]) / std[c] and writes bf16 patch rows [n_img*P, 768] with
 * k = c*256 + py*16 + px (the flatten order of Conv2d weight [D,3,16,16]). */
typedef struct {
    const uint8_t* tiles; /* [n_img, tile_h, tile_w, 3] u8 (NHWC)             */
    void* patches;        /* bf16 [n_img * (crop/16)^2, 768]                  */
    int32_t n_img;        /* images in this crop group                        */
    int32_t tile_h, tile_w;
    int64_t img_stride;   /* bytes between consecutive images                 */
    int32_t n_win;        /* crop windows per tile (images = tiles x windows) */
    int32_t win_y[16], win_x[16]; /* window origin per window index           */
    int32_t crop;         /* window side, multiple of 16                      */
    float mean[3], std[3];
    /* image index i -> tile i % n_tiles, window i / n_tiles (crop-major)     */
    int32_t n_tiles;
    /* optional device f32 [n_tiles][8] = {y0, y1, x0, x1, v_r, v_g, v_b, on}: pixels of tile t inside the box take the
     * NORMALISED value v_c -- Cutout applied after Normalize (transformations.py:206-207: zeros) and
     * MyMeanPixelRegularization (91-100: the whole tile becomes one colour) are not uint8 pixel values          */
    const float* fill;
} gv_patchify_args;
int gv_patchify(const gv_patchify_args* a, void* stream);

/* ---- patchify_nchw: the same patch rows from the reference's own hot-path input, Data [B, 3, H, W] float32 ALREADY
 * normalised by ToTensor + Normalize (train.py:1027-1033, datasets.py:614-621, transformations.py:124-128), or a
 * user hook's FloatTensor[3, H, W] (transformations.py:199-200).  No mean / std: each value is only rounded to the
 * build's 16-bit format, round-to-nearest-even (bit-identical to torch's .to(bfloat16) / .to(float16) for finite
 * input; NaN stays NaN, +-Inf stays +-Inf).  Windows may start at any pixel; strides let a slice of a larger batch in
 * without a copy.  Same image order, rows and column order k = c*256 + py*16 + px as gv_patchify. */
typedef struct {
    const float* images;          /* [n_tiles, 3, img_h, img_w] f32, strides below (elements); the W stride is 1 */
    void* patches;                /* 16-bit (f32 for _f32) [n_img * (crop/16)^2, 768], 16-byte aligned          */
    int32_t n_img, n_tiles, img_h, img_w;
    int64_t stride_n, stride_c, stride_h;
    /* image index i -> tile i % n_tiles, window i / n_tiles (crop-major); crop multiple of 16 */
    int32_t n_win, win_y[16], win_x[16], crop;
} gv_patchify_nchw_args;
int gv_patchify_nchw(const gv_patchify_nchw_args* a, void* stream);

/* ---- mixup / cutmix inside the patchify pass (reference train.py:752-771 builds timm's Mixup, 1037-1040 applies it to
 * the batch: `input, target = mixup_fn(input, target)`).  One row of the device mix table per image i of the batch:
 * partner index j, the weights (BOTH rounded on the host from the double the sampler drew: the kernel never computes
 * 1 - lam), a box [yl, yh) x [xl, xh) in window coordinates and a mode.  With n(t, y, x, c) the value the unmixed
 * kernel writes for tile t:
 *   GV_MIX_COPY   n(i)                                  the row is bit-identical to the unmixed kernel's; j is not read
 *   GV_MIX_BLEND  n(i) * lam + n(j) * one_minus_lam     (mixup) each product and the sum rounded separately, no FMA,
 *                                                       then rounded once to the 16-bit format (kept f32 for _f32)
 *   GV_MIX_PASTE  n(j) inside the box, n(i) outside     (cutmix)
 * Sources are always the ORIGINAL tiles (timm mixes from x.flip(0) / copies), nothing is mixed in place.  A row whose
 * partner is outside [0, n_tiles) or whose mode is unknown is treated as GV_MIX_COPY. */
enum { GV_MIX_COPY = 0, GV_MIX_BLEND = 1, GV_MIX_PASTE = 2 };
typedef struct {
    int32_t partner, mode;
    float lam, one_minus_lam;
    int32_t yl, yh, xl, xh;
} gv_mix_row;
/* gv_patchify with a mix table: one window only (n_win == 1, the supervised step's top-left img_size window); `fill`
 * is applied per SOURCE tile, as the unmixed kernel applies it. */
typedef struct {
    gv_patchify_args p;
    const gv_mix_row* mix;        /* device [p.n_tiles], 4-byte aligned */
} gv_patchify_mix_args;
int gv_patchify_mix(const gv_patchify_mix_args* a, void* stream);
/* gv_patchify_nchw with a mix table (n_win == 1): blend is x[i] * lam + x[j] * one_minus_lam with the same separate
 * roundings -- bit-identical to torch's x.mul(lam).add(x.flip(0).mul(1 - lam)) followed by .to(16-bit). */
typedef struct {
    gv_patchify_nchw_args p;
    const gv_mix_row* mix;        /* device [p.n_tiles], 4-byte aligned */
} gv_patchify_nchw_mix_args;
int gv_patchify_nchw_mix(const gv_patchify_nchw_mix_args* a, void* stream);

/* ---- random erasing inside the patchify pass (--reprob / --remode / --recount: timm's RandomErasing as its PrefetchLoader
 * builds it -- the reference's timm_train.py:621-624 passes the flags to timm's loader, its train.py:788-791 has the same
 * call commented out).  One row of the device erase table per image i of the batch: up to GV_ERASE_MAX_BOXES boxes
 * [yl, yh) x [xl, xh) in window coordinates (clamped to the window), applied in order on the NORMALISED values the
 * network sees, after the mix table and after `fill`, so an erased pixel depends on no source pixel:
 *   GV_ERASE_OFF    the row is bit-identical to the kernel without the table
 *   GV_ERASE_VALUE  pixels of box b take value[b][c] (timm mode 'const': zeros; 'rand': one N(0,1) draw per box and
 *                   channel, made on the host); a later box overwrites an earlier one
 *   GV_ERASE_NOISE  pixels of every box take z(i, c, y, x) (timm mode 'pixel'), a counter-based N(0,1) deviate keyed by the
 *                   pixel, not by the box or the launch geometry -- the u8 and the NCHW kernel, both output widths and
 *                   gipvit.erasing.noise_reference agree.  With S = crop, idx = ((i * 3 + c) * S + y) * S + x as uint32 and
 *                   fmix32 the murmur3 finaliser of gv_dropout:
 *                       h1 = fmix32(seed + 0x9E3779B9 * (idx + 1));   h2 = fmix32(h1 + 0x6D2B79F5)
 *                       u1 = ((h1 >> 8) + 1) * 2^-24;                 u2 = (h2 >> 8) * 2^-24
 *                       z  = sqrtf(-2 * logf(u1)) * cosf(6.2831853f * u2)       (f32, the accurate library functions)
 * In every mode the value is rounded once to the 16-bit format (kept f32 for _f32).  A row with an unknown mode or n_box
 * outside 0 .. GV_ERASE_MAX_BOXES is treated as GV_ERASE_OFF.  A 16-pixel run (u8) or 4-pixel item (NCHW) wholly inside
 * erased boxes loads nothing, neither from its image nor from its mix partner. */
enum { GV_ERASE_OFF = 0, GV_ERASE_VALUE = 1, GV_ERASE_NOISE = 2 };
#define GV_ERASE_MAX_BOXES 8
typedef struct {
    int32_t mode, n_box;
    int32_t box[GV_ERASE_MAX_BOXES][4];   /* {yl, yh, xl, xh} */
    float value[GV_ERASE_MAX_BOXES][3];   /* GV_ERASE_VALUE: normalised value per box and channel */
} gv_erase_row;
/* gv_patchify / gv_patchify_mix with an erase table: one window only (n_win == 1); n_img * 3 * crop^2 < 2^32. */
typedef struct {
    gv_patchify_args p;
    const gv_mix_row* mix;        /* device [p.n_tiles], 4-byte aligned, or NULL: no mixing */
    const gv_erase_row* erase;    /* device [p.n_tiles], 4-byte aligned */
    uint32_t seed;                /* GV_ERASE_NOISE: one value per step */
} gv_patchify_erase_args;
int gv_patchify_erase(const gv_patchify_erase_args* a, void* stream);
typedef struct {
    gv_patchify_nchw_args p;
    const gv_mix_row* mix;        /* device [p.n_tiles], 4-byte aligned, or NULL: no mixing */
    const gv_erase_row* erase;    /* device [p.n_tiles], 4-byte aligned */
    uint32_t seed;
} gv_patchify_nchw_erase_args;
int gv_patchify_nchw_erase(const gv_patchify_nchw_erase_args* a, void* stream);

/* ---- random-resized crops of the tiles (DINO multi-crop input stage; absent from the
 * reference, whose tiles are augmented on the CPU by transformations.py:103-209 -- SURVEY 8f rank 1).
 * For crop n: box (y0, x0, h, w) of tile `tile` is resampled to out_size x out_size with
 * torchvision's tensor-mode semantics (float32 bilinear, align_corners=False, no antialias,
 * round half to even, clamp) and mirrored left-right when flip != 0.
 * boxes: device int32 [n_crops][6] = {tile, y0, x0, h, w, flip}; the box must lie inside the
 * tile (the caller checks: the values are device-resident).  out: u8 [n_crops, out, out, 3].   */
typedef struct {
    const uint8_t* tiles;  /* [n_tiles, tile_h, tile_w, 3] u8 (NHWC) */
    uint8_t* out;
    const int32_t* boxes;
    int32_t n_crops, n_tiles, tile_h, tile_w, out_size;
} gv_crop_resize_args;
int gv_crop_resize(const gv_crop_resize_args* a, void* stream);

/* ---- DINO view augmentation fused behind the random-resized crop: ONE pass over the tiles writes every augmented view
 * (DINO's DataAugmentationDINO -- absent from the reference; its pixel operations are the ones the reference applies to
 * whole tiles on the CPU, transformations.py:140-147: torchvision ColorJitter on PIL images + GaussianBlur(3)).  Per crop,
 * with that crop's own draws (made on the host):
 *   random-resized crop + flip (exactly gv_crop_resize's arithmetic)  ->  ColorJitter ops in `order` (n_color = 0: the
 *   RandomApply missed)  ->  RandomGrayscale (PIL "L", replicated)  ->  Gaussian blur 3x3 on the jittered view (float32,
 *   reflect padding, round half to even)  ->  solarise (PIL ImageOps.solarize: v >= threshold -> 255 - v).
 * ColorJitter's contrast blends with the mean grey of the VIEW as it is when the operation runs: a first kernel takes it
 * per crop (`stats`, device uint64 [n_crops], scratch).  The resized crop itself never exists in HBM.                      */
typedef struct {
    int32_t n_color;             /* colour operations applied (0..4)                                            */
    int32_t order[4];            /* 0 brightness, 1 contrast, 2 saturation, 3 hue, in application order          */
    float bf, cf, sf;            /* ImageEnhance factors                                                        */
    int32_t hue;                 /* added to the H byte (mod 256)                                               */
    int32_t gray;                /* 1: grayscale view                                                           */
    int32_t blur; float kc, ks;  /* 3x3 Gaussian: centre / side weight of the normalised 1-D kernel             */
    int32_t solar;               /* solarise threshold (DINO: 128), < 0: off                                    */
} gv_view_params;
typedef struct {
    const uint8_t* tiles;        /* [n_tiles, tile_h, tile_w, 3] u8 (NHWC)                                      */
    uint8_t* out;                /* [n_crops, out_size, out_size, 3] u8                                         */
    const int32_t* boxes;        /* device int32 [n_crops][6] = {tile, y0, x0, h, w, flip} (as gv_crop_resize)  */
    const gv_view_params* params; /* device [n_crops]                                                           */
    uint64_t* stats;
    int32_t n_crops, n_tiles, tile_h, tile_w, out_size;
} gv_crop_augment_args;
int gv_crop_augment(const gv_crop_augment_args* a, void* stream);

/* ---- gv_crop_augment with an H&E stain jitter (Tellez et al. 2018 / 2019, "HED" augmentation; absent from the reference) in
 * the same pass.  Per crop: random-resized crop + flip (exactly gv_crop_resize's arithmetic)  ->  stain transform  ->  the
 * chain of gv_crop_augment (colour ops in `order`, grayscale, blur, solarise); contrast blends with the mean grey of the
 * STAINED view.  With M the stain matrix (rows H, E, D: Ruifrok & Johnston's vectors, each normalised to unit length), a
 * pixel with bytes v_c goes through
 *     od_c  = -ln((v_c + 1) / 256)                        (>= 0, finite for v = 0)
 *     s     = od . M^-1                                   (stain concentrations, not clamped)
 *     s'_k  = alpha_k * s_k + beta_k                      (k = H, E, D)
 *     od'   = s' . M
 *     v'_c  = clamp(rint(256 * exp(-od'_c) - 1), 0, 255)  (round half to even)
 * The map is affine in od, so the host (gipvit.stain.stain_record) folds a crop's draw into A = M^-1 diag(alpha) M and
 * b = beta M, both taken in fp64 and rounded to f32, and the kernel evaluates od'_c = sum_k od_k * A[k][c] + b[c] in f32
 * (od from a 256-entry table of the fp64 values rounded once, the accurate expf).  on = 0: the crop's pixels pass through
 * untouched; alpha = 1, beta = 0 is the identity on every byte.  Checks, launches and `stats` as gv_crop_augment.          */
typedef struct {
    int32_t on;                  /* 0: no stain transform for this crop                                         */
    float A[9];                  /* row-major [k][c]                                                            */
    float b[3];
} gv_stain_params;
typedef struct {
    gv_crop_augment_args v;
    const gv_stain_params* stain; /* device [v.n_crops], 4-byte aligned                                         */
} gv_crop_augment_stain_args;
int gv_crop_augment_stain(const gv_crop_augment_stain_args* a, void* stream);

/* ---- Macenko stain normalisation at inference (Macenko et al., ISBI 2009; absent from the reference).  Per slide, from a
 * sample of its tiles (u8 NHWC, already cut to the window the encoder sees), the slide's own haematoxylin / eosin vectors
 * HE [3][2] and their 99th-percentile concentrations maxC [2] are estimated and the slide is mapped onto a fixed target
 * (HE_t, maxC_t).  Optical density is this library's, od_c = -ln((v_c + 1) / 256), NOT the -ln(v / 240) of the usual scripts:
 * a slide whose estimate equals the target maps onto itself.  The map is linear in od,
 *     od' = od . A,   A = (HE_t diag(maxC_t / maxC) pinv(HE))^T   (fp64, rounded to f32; b = 0, on = 1)
 * i.e. one gv_stain_params record per slide, evaluated exactly as the crop pass evaluates a jitter record.  The estimate
 * (gipvit.stainnorm restates it in fp64 numpy) takes three passes over the sample with small host steps between them:
 *   tissue mask   pixel p is tissue iff all three bytes are <= v_max, v_max = floor(256 exp(-beta)) - 1 (beta = 0.15: 219);
 *                 an integer test, no floating-point comparison on the device
 *   pass 1        gv_stain_stats over tissue pixels: the count n, sum od (3) and sum od_i od_j (6, upper triangle), fp64.
 *                 Host: covariance (S2 - n mu mu^T) / (n - 1), eigh, the two leading eigenvectors V [3][2] (largest first,
 *                 each flipped so that its component sum is >= 0)
 *   pass 2        gv_stain_angle_hist over tissue pixels: t = od . V, phi = atan2(t1, t0), bin floor((phi + pi) NB / 2 pi)
 *                 clamped to [0, NB).  Host: phi_lo / phi_hi = the alpha-th / (100 - alpha)-th percentile of the histogram,
 *                 v = V (cos phi, sin phi); the vector with the larger first component is H, the other E
 *   pass 3        gv_stain_conc_hist over ALL pixels: c = pinv(HE) od, one histogram per stain over [0, cmax_k),
 *                 cmax_k = ln 256 * sum_j max(pinv_kj, 0) (an upper bound: od >= 0; a value past it lands in the last
 *                 bin); c_k < 0 goes to an underflow count that still counts for the rank.  Host: maxC_k = the 99th percentile
 * A percentile read from a histogram has the resolution of one bin width.  All three passes compute in fp64 from a per-block
 * table of the 256 od values and share one launch shape: G = clamp(ceil(n h w / 256), 1, 512) workgroups -- a function of the
 * shape only, never of the device -- write per-workgroup partials into `workspace`, a second launch sums them in a fixed
 * order.  No floating-point atomic anywhere (histogram bins are integer adds in LDS): results are bitwise the same run to run
 * and box to box.  workspace bytes:  gv_stain_stats G * 80;  gv_stain_angle_hist G * NB * 4;  gv_stain_conc_hist
 * G * 2 * (NB + 1) * 4.  Refused before any launch: a null pointer (GV_E_NULL), tiles-independent pointers not 8-byte aligned
 * (GV_E_ALIGN), NB outside 256 .. 4096, v_max outside 0 .. 255, n h w >= 2^32 or img_stride < h w 3 (GV_E_SHAPE).         */
typedef struct {
    const uint8_t* tiles;        /* [n, h, w, 3] u8 (NHWC), img_stride bytes between tiles                      */
    int64_t img_stride;
    int32_t n, h, w;
    int32_t v_max;               /* tissue: every byte <= v_max                                                 */
    void* workspace;             /* 8-byte aligned, see above                                                   */
    void* out;                   /* 8-byte aligned: uint64 n, then f64 {s_r, s_g, s_b, s_rr, s_rg, s_rb, s_gg, s_gb, s_bb} */
} gv_stain_stats_args;
int gv_stain_stats(const gv_stain_stats_args* a, void* stream);
typedef struct {
    const uint8_t* tiles;
    int64_t img_stride;
    int32_t n, h, w;
    int32_t v_max;
    int32_t n_bins;              /* NB                                                                          */
    double V[6];                 /* row-major [3][2]                                                            */
    void* workspace;
    int64_t* out;                /* [NB] counts, 8-byte aligned                                                 */
} gv_stain_angle_hist_args;
int gv_stain_angle_hist(const gv_stain_angle_hist_args* a, void* stream);
typedef struct {
    const uint8_t* tiles;
    int64_t img_stride;
    int32_t n, h, w;
    int32_t n_bins;              /* NB                                                                          */
    double pinv[6];              /* row-major [2][3]: pinv(HE)                                                  */
    double cmax[2];              /* > 0                                                                         */
    void* workspace;
    int64_t* out;                /* [2][NB + 1]: stain k's bins, then its underflow count; 8-byte aligned       */
} gv_stain_conc_hist_args;
int gv_stain_conc_hist(const gv_stain_conc_hist_args* a, void* stream);

/* ---- gv_stain_apply: u8 tiles -> u8 tiles through one gv_stain_params record per tile (what a pathologist looks at for QA).
 * Every pixel goes through the crop pass's own function (csrc/stain_px.h); a tile whose record has on = 0 is copied bit for
 * bit.  out is contiguous [n, h, w, 3] and must not overlap tiles' other tiles (in place, out == tiles with the same stride,
 * is fine: a pixel depends on itself only).  n <= 65535.                                                                    */
typedef struct {
    const uint8_t* tiles;        /* [n, h, w, 3] u8 (NHWC), img_stride bytes between tiles                      */
    uint8_t* out;                /* [n, h, w, 3] u8, contiguous                                                 */
    const gv_stain_params* stain; /* device [n], 4-byte aligned                                                 */
    int64_t img_stride;
    int32_t n, h, w;
} gv_stain_apply_args;
int gv_stain_apply(const gv_stain_apply_args* a, void* stream);

/* ---- gv_patchify_stain: gv_patchify with the stain map inside the same pass (no extra pass over the pixels).  The bytes of
 * tile t go through record stain[t] first (the same function as gv_stain_apply), then through the n(tile, y, x, c) of the plain
 * kernel computed from the stained BYTE, `fill` applied after the stain as it is applied after Normalize: the rows are
 * bit-identical to gv_patchify over gv_stain_apply's output.  A workgroup none of whose tiles has on != 0 builds no table and
 * evaluates no exponential.  No mix / erase combination (those are training tables), no NCHW form.  Checks as gv_patchify,
 * plus: a null table GV_E_NULL, a table that is not 4-byte aligned GV_E_ALIGN.                                              */
typedef struct {
    gv_patchify_args p;
    const gv_stain_params* stain; /* device [p.n_tiles], 4-byte aligned                                         */
} gv_patchify_stain_args;
int gv_patchify_stain(const gv_patchify_stain_args* a, void* stream);

/* ---- tile augmentation on the device (replaces the CPU / PIL recipes of transformations.py:131-197 on tiles that are
 * already in HBM).  One parameter record per tile, drawn on the host; operations in reference order:
 *   colour ops in `order` (0 brightness, 1 contrast, 2 saturation, 3 hue: torchvision ColorJitter on PIL images, PIL's
 *   float32 blend with truncation; hue = +`hue` on the H byte of PIL's HSV image) -> Gaussian blur 3x3 (float32, reflect
 *   padding, round half to even; kc / ks = centre / side weight of the 1-D kernel) -> Gaussian noise x/255 + sigma * z,
 *   clip, (255 x) truncated (transformations.py:71-88; z = ztable[murmur3(seed, pixel, channel) >> 22]) -> dihedral element
 *   d4 (bit 0 transpose, bit 1 mirror rows, bit 2 mirror columns: any sequence of flips / MyRotation, 48-56) -> NEAREST
 *   zoom about the centre in 16.16 fixed point (RandomAffine(degrees=0, scale), PIL semantics) -> black box `cut`
 *   (Cutout on the [0, 1] tensor, 10-45).  Byte-exact against oracle/augment_oracle.py.
 * stats: device scratch u64 [n] (zeroed by the call); ztable: device f32 [1024], quantiles of N(0, 1).                  */
typedef struct {
    int32_t n_color; int32_t order[4];
    float bf, cf, sf; int32_t hue;
    int32_t blur; float kc, ks;
    float sigma; uint32_t seed;
    int32_t d4;
    int32_t zoom, a0, a2;
    int32_t cut[4];              /* y0, y1, x0, x1 in output coordinates; empty when y0 >= y1            */
} gv_augment_params;
typedef struct {
    const uint8_t* tiles; uint8_t* out;       /* u8 [n, H, W, 3] NHWC, out != tiles                     */
    const gv_augment_params* params;          /* device [n]                                             */
    uint64_t* stats; const float* ztable;
    int32_t n, H, W;
} gv_augment_args;
int gv_augment(const gv_augment_args* a, void* stream);

/* ---- LayerNorm (nn.LayerNorm(D, eps=1e-6); vit.pyc@L138,142,195) -------
 * fwd: x f32 rows -> y bf16 rows (+ mean, rstd f32 per row).
 * D must be 192, 384 or 768.  Row r of x lives at x + r*x_stride.        */
typedef struct {
    const float* x; int64_t x_stride;
    const float* gamma; const float* beta;
    void* y;              /* bf16 [rows, D] compact                         */
    float* mean; float* rstd; /* [rows]                                      */
    int32_t rows, D; float eps;
} gv_layernorm_fwd_args;
int gv_layernorm_fwd(const gv_layernorm_fwd_args* a, void* stream);

/* bwd: g[r] (f32, the residual-stream gradient, stride g_stride) += dLN/dx;
 * gb[r] = bf16(g[r]); partial column sums of dy*xhat, dy and new g are left
 * in `partials` [GV_LN_PARTIAL_BLOCKS, 3, D] f32 for gv_colsum_finalize.   */
#define GV_LN_PARTIAL_BLOCKS 1024
typedef struct {
    const void* dy;       /* bf16 [rows, D] compact                         */
    const float* x; int64_t x_stride;
    const float* mean; const float* rstd; const float* gamma;
    float* g; int64_t g_stride;   /* in/out                                  */
    void* gb; int64_t gb_stride;  /* bf16 out (may be NULL)                  */
    float* partials;
    int32_t rows, D;
    int32_t g_init;       /* 1: g is treated as 0 on input (g = dx)          */
    const float* gb_scale; /* optional [rows]: gb[r] = bf16(g[r] * gb_scale[r]) -- the gradient entering a branch whose
                            * output was scaled by stochastic depth; NULL = 1  */
} gv_layernorm_bwd_args;
int gv_layernorm_bwd(const gv_layernorm_bwd_args* a, void* stream);

/* out[c] (+)= sum_b partials[b, which, c] for b < n_blocks                 */
typedef struct {
    const float* partials; int32_t n_blocks, n_which, which, C;
    float* out; int32_t accumulate;
} gv_colsum_finalize_args;
int gv_colsum_finalize(const gv_colsum_finalize_args* a, void* stream);

/* all three column sums of a LayerNorm-backward partial buffer in one launch:
 * out_w[c] += sum_b partials[b, w, c] for w = 0..2 (NULL outputs are skipped).  Always
 * accumulates (row-split blocks meet in the outputs through f32 atomics).             */
typedef struct {
    const float* partials; int32_t n_blocks, C;
    float* out0; float* out1; float* out2;
} gv_ln_finalize_args;
int gv_ln_finalize(const gv_ln_finalize_args* a, void* stream);

/* column sums of a bf16 or f32 matrix [rows, C] -> out[C] f32 (bias grads,
 * train.py:1071 backward of nn.Linear bias).  workspace >= 64*C floats.    */
typedef struct {
    const void* x; int32_t x_is_f32; int64_t ld;
    int32_t rows, C;
    float* workspace; float* out; int32_t accumulate;
} gv_colsum_args;
int gv_colsum(const gv_colsum_args* a, void* stream);

/* ---- linear / GEMM (nn.Linear fwd + both backward products; vit.pyc@L98-104,
 * L119-131, L326-330).  C[M,N] = op(A) . op(B) with bf16 operands, f32 MFMA
 * accumulation (v_mfma_f32_16x16x32_bf16):
 *    trans_a = 0: A stored [M,K];  1: A stored [K,M]
 *    trans_b = 0: B stored [N,K] (torch Linear weight);  1: B stored [K,N]
 * forward  y = x W^T      : (0,0)        dX = dY W : (0,1)     dW = dY^T X : (1,1)
 * Epilogue, applied in this order to the f32 accumulator v at (m,n):
 *    BIAS: v += bias[n];  SAVE_PRE: aux_out[m,n] = bf16(v);  GELU: v = gelu(v);
 *    DGELU: v *= gelu'(aux_in[m,n]);  RESID: v += resid[m,n] (f32);
 *    POS: token-row remap m -> m + m/P + 1 and v += pos[(m%P)+1, n] (patch embed);
 *    ACCUM: v += C[m,n] (f32 out only);  then C[m,n] = v (bf16 or f32).       */
enum {
    GV_EPI_BIAS = 1, GV_EPI_GELU = 2, GV_EPI_RESID = 4, GV_EPI_DGELU = 8,
    GV_EPI_ACCUM = 16, GV_EPI_POS = 32, GV_EPI_SAVE_PRE = 64,
    GV_EPI_ALL = 127      /* any other bit is rejected with GV_E_UNSUPPORTED */
};
typedef struct {
    const void* A; const void* B; void* C;
    int32_t M, N, K;
    int64_t lda, ldb, ldc;
    int32_t trans_a, trans_b;
    int32_t c_is_f32;
    int32_t epilogue;           /* GV_EPI_* bitmask                          */
    const float* bias;          /* [N] f32                                   */
    const float* resid; int64_t ldr;   /* f32 [M,N]                          */
    const void* aux_in; int64_t ld_aux; /* bf16 [M,N] pre-activation (DGELU) */
    void* aux_out;              /* bf16 [M,N], ld = ld_aux (SAVE_PRE)        */
    const float* pos; int32_t P; /* POS: pos f32 [(P+1), N]                  */
    float alpha;                /* scales the accumulator before the epilogue*/
    /* trans_a only: colsum_a[m] += sum_k A[k,m] (f32, atomics) -- the bias gradient of the
     * Linear whose weight gradient this launch computes, from the tiles it stages anyway */
    float* colsum_a;
    /* optional split-K scratch (f32, caller-owned, gv_linear_workspace_bytes() big): when given,
     * split-K partial tiles are stored as slabs and summed into C by a second kernel instead of
     * meeting in C through f32 atomics (the atomic volume is ~33 MB per launch at full occupancy
     * and runs at ~1.3 TB/s; slab stores + reduce move the same bytes at HBM speed).           */
    float* workspace; int64_t workspace_bytes;
    /* RESID only, optional: v *= row_scale[m] before the residual add -- stochastic depth (timm DropPath, train.py:283-288
     * --drop-path: keep / (1 - p) of the token's image, see gv_expand_rows); NULL = 1                                  */
    const float* row_scale;
} gv_linear_args;
/* upper bound of the split-K scratch gv_linear can use for any shape */
int64_t gv_linear_workspace_bytes(void);
/* Scratch ONE call would use if the full gv_linear_workspace_bytes() were offered (`gv_workspace_bytes(op, shape)`):
 * op = GV_OP_LINEAR with a gv_linear_args, GV_OP_LINEAR_DW_GROUP with a gv_linear_dw_group_args -- shapes, flags, leading
 * dimensions and operand ALIGNMENT as in the real call (pointers are checked for alignment, never dereferenced; the
 * workspace fields are ignored).  The entry point's own checks and kernel selection answer, nothing is launched: 0 = the call
 * takes no scratch (e.g. the full-row kernels), -1 = the arguments would be rejected (gv_last_error()).  Every other entry
 * point takes caller-sized buffers named in its struct and needs no query.                                                  */
#define GV_OP_LINEAR 0
#define GV_OP_LINEAR_DW_GROUP 1
int64_t gv_workspace_bytes(int32_t op, const void* args);
int gv_linear(const gv_linear_args* a, void* stream);

/* Weight gradients of several Linears that reduce over the SAME token rows (one transformer block: attn.qkv, attn.proj,
 * mlp.fc1, mlp.fc2; autograd of vit.pyc@L98-104, L119-131) in ONE launch:  dW_q[M_q, N_q] += dY_q^T X_q over K rows, and
 * colsum_dy_q[m] += sum_k dY_q[k, m] (the bias gradient) where given.  Split-K fills the chip ONCE for the whole group
 * instead of once per product: 108 tiles x 4 slices for a ViT-S block instead of 4 x (9..36 tiles x 14..56 slices), so the
 * partial-tile slab traffic drops from 4 x 32 MB to 28 MB and one reduce launch serves all products.
 * workspace: f32 scratch, gv_linear_workspace_bytes() big.                                                             */
#define GV_DW_GROUP_MAX 4
typedef struct {
    const void* dY; int64_t ldy;     /* bf16 [K, M]  (rows = tokens)                         */
    const void* X;  int64_t ldx;     /* bf16 [K, N]                                          */
    float* dW; int64_t ldw;          /* f32 [M, N], accumulated into                         */
    float* colsum_dy;                /* f32 [M] or NULL, accumulated into                    */
    int32_t M, N;
} gv_dw_problem;
typedef struct {
    gv_dw_problem prob[GV_DW_GROUP_MAX];
    int32_t n, K;
    float* workspace; int64_t workspace_bytes;
} gv_linear_dw_group_args;
int gv_linear_dw_group(const gv_linear_dw_group_args* a, void* stream);

/* Live per-kernel timing of the GEMM-class launches (gv_linear, gv_linear_ln_fwd, gv_linear_ln_bwd; bench.py's
 * roofline leg): while enabled, every such launch is bracketed by two HIP events on the launch stream.
 * gv_linear_timing(1) clears earlier records and starts recording, gv_linear_timing(0) stops.  _read synchronises
 * on the recorded events and folds them into one row per kernel (name = the kernel instantiation as rocprofv3
 * prints it, e.g. "gemm_kernel<true, true, float, true, 16>"); returns the number of rows written (<= max_rows)
 * or an error.                                                                                                  */
typedef struct {
    char name[96];
    int32_t launches;
    double seconds, flops;   /* summed over the launches */
    double bytes;            /* algorithmic HBM bytes summed over the launches: every operand read once, every output written once */
} gv_linear_timing_row;
int gv_linear_timing(int enable);
int gv_linear_timing_read(gv_linear_timing_row* rows, int max_rows);

/* ---- full-row Linear fused with the LayerNorm around it (ViT-S width: N must be 384) --------------------------
 * One workgroup owns whole output rows, so the row-wise LayerNorm work happens in the GEMM epilogue and the f32
 * residual row makes one HBM round trip instead of two (csrc/panel.hip).
 *
 * fwd -- replaces `x = x + Linear(a)` of Block.forward (attn.proj / mlp.fc2, vit.pyc@L146-152) TOGETHER WITH the
 * LayerNorm that reads the new x next (norm2 of the block / norm1 of the next block, vit.pyc@L138,142):
 *     out[m,:] = A[m,:] . W^T + bias + resid[m,:]          (f32; W is the Linear weight [N, K], bf16)
 *     y[m,:]   = bf16( (out[m,:] - mean[m]) * rstd[m] * gamma + beta ),  mean / rstd of out[m,:] (eps inside the sqrt)
 * gamma == NULL skips the LayerNorm outputs (last block: the final norm reads CLS rows only); bias / resid optional. */
typedef struct {
    const void* A; const void* W;        /* bf16 [M, K] (lda), bf16 [N, K] (ldw)            */
    int32_t M, N, K; int64_t lda, ldw;
    const float* bias;                   /* [N] or NULL                                     */
    const float* resid; int64_t ldr;     /* f32 [M, N] or NULL                              */
    float* out; int64_t ldo;             /* f32 [M, N]                                      */
    const float* gamma; const float* beta; float eps;
    void* y;                             /* bf16 [M, N] compact                             */
    float* mean; float* rstd;            /* [M]                                             */
    const float* row_scale;              /* optional [M]: out = resid + row_scale[m] * (A W^T + bias) (stochastic depth)    */
} gv_linear_ln_fwd_args;
int gv_linear_ln_fwd(const gv_linear_ln_fwd_args* a, void* stream);

/* Fused MLP forward (vit.pyc@L98-104 Mlp.forward inside Block.forward L146-152, for passes that save nothing: the DINO teacher,
 * inference):  out = resid + row_scale * (GELU(A W1^T + bias1) W2^T + bias2)  [f32],  and -- with gamma -- y / mean / rstd =
 * LayerNorm(out) as gv_linear_ln_fwd leaves them.  A bf16 [M, K], W1 bf16 [hidden, K], W2 bf16 [N, hidden]; N = 384,
 * K % 64 == 0, hidden % 256 == 0.  The [M, hidden] activation lives in LDS, 256 columns at a time (a K-slice of fc2);
 * results are bit-identical to gv_linear(BIAS | GELU) followed by gv_linear_ln_fwd.                                          */
typedef struct {
    const void* A; const void* W1; const float* bias1; const void* W2; const float* bias2;
    int32_t M, N, K, hidden; int64_t lda, ldw1, ldw2;
    const float* resid; int64_t ldr; float* out; int64_t ldo;
    const float* gamma; const float* beta; float eps; void* y; float* mean; float* rstd;
    const float* row_scale;
} gv_mlp_ln_fwd_args;
int gv_mlp_ln_fwd(const gv_mlp_ln_fwd_args* a, void* stream);

/* bwd -- replaces the dX product of the Linear that CONSUMED a LayerNorm output (mlp.fc1 / attn.qkv:
 * dXn = dY . W with W the Linear weight stored [K = its out features, N = 384]) together with that LayerNorm's
 * backward (autograd of vit.pyc@L138,142; gv_layernorm_bwd's contract with dy = dXn kept in f32):
 *     g[m,:] (+)= dLN/dx(dXn[m,:]; x[m,:], mean[m], rstd[m], gamma);   gb[m,:] = bf16(g[m,:])
 *     partials[b, 0..2, :] = column sums over workgroup b's rows of dXn*xhat, dXn, new g   (gv_ln_finalize folds them:
 *     dgamma, dbeta, bias gradient of the Linear in front of the residual add)
 * partials must hold gv_linear_ln_blocks(M) blocks of [3, N] f32.                                                   */
typedef struct {
    const void* A; const void* W;        /* bf16 dY [M, K] (lda), bf16 W [K, N] (ldw)       */
    int32_t M, N, K; int64_t lda, ldw;
    const float* x; int64_t ldx;         /* f32 [M, N]: the LayerNorm's input rows          */
    const float* mean; const float* rstd; const float* gamma;
    float* g; int64_t ldg;               /* f32 [M, N] in/out: residual-stream gradient     */
    void* gb; int64_t ldgb;              /* bf16 out (may be NULL)                          */
    float* partials; int32_t partial_blocks;
    int32_t g_init;                      /* 1: g is treated as 0 on input                   */
    const float* gb_scale;               /* optional [M]: gb[m,:] = bf16(g[m,:] * gb_scale[m]) (stochastic depth)           */
} gv_linear_ln_bwd_args;
int gv_linear_ln_bwd(const gv_linear_ln_bwd_args* a, void* stream);
/* workgroups (= partial blocks) a gv_linear_ln_* launch over M rows uses */
int gv_linear_ln_blocks(int32_t M);

/* ---- stochastic depth (timm DropPath behind --drop-path, train.py:283-288; vit.pyc@L66-74): n_rep sets of per-image
 * factors keep / (1 - p) (one set per residual branch) expanded to one factor per token row of a multi-crop row space:
 * rows[r*T + t] = per_img[r*n_img + row_img[t]],  row_img[t] = the image token row t belongs to.                   */
typedef struct { const float* per_img; const int32_t* row_img; float* rows; int32_t n_rep, n_img, T; } gv_expand_rows_args;
int gv_expand_rows(const gv_expand_rows_args* a, void* stream);

/* ---- attention (vit.pyc@L119-131): softmax(q k^T * scale) v per (image, head)
 * on packed qkv bf16 [n_img*N, 3, H, 64] -> o bf16 [n_img*N, H, 64];
 * lse f32 [n_img, H, N] (natural-log sum-exp of the scaled scores).
 * head_dim is fixed at 64 (ViT-T/S/B); N <= GV_ATTN_MAX_N (a whole sequence
 * sits in one workgroup's LDS; the _f32 entry points: N <= GV_ATTN_F32_MAX_N). */
typedef struct {
    const void* qkv; void* o; float* lse;
    int32_t n_img, N, H; float scale;
    int32_t q_limit;      /* > 0: only the first q_limit query rows of every image are needed (rounded up to 32): o / lse rows behind
                           * them are left untouched.  The last block of a ViT whose forward returns the CLS row (vit.pyc@L248-253)
                           * asks for 1.  0 = every query.  (The _f32 entry point computes every query.)                            */
} gv_attention_fwd_args;
int gv_attention_fwd(const gv_attention_fwd_args* a, void* stream);

/* Streaming forward for sequences past the GV_ATTN_MAX_N of gv_attention_fwd (tiles up to 512 px at patch 16: 1 025 tokens).  Inputs and
 * outputs are those of gv_attention_fwd -- qkv 16-bit [n_img*N, 3, H, 64], o 16-bit [n_img*N, H, 64], lse f32 [n_img, H, N] (the
 * natural-log sum-exp of the scaled scores), head_dim 64 -- for 1 <= N <= GV_ATTN_STREAM_MAX_N (65 key tiles of 16); any other N
 * returns GV_E_SHAPE with the limit in gv_last_error(), a null pointer GV_E_NULL, both before any launch.  scale must be > 0
 * (GV_E_SHAPE otherwise: the running max is taken over the unscaled scores).
 * K / V pass through LDS in key blocks under an online softmax: running max and running sum per query row in f32, an f32 O
 * accumulator rescaled when the max moves, P rounded to the 16-bit format before P V (as gv_attention_fwd does), one division at
 * the end, lse = max + log(sum).  Keys >= N of the last block are never counted, query rows >= N never stored.
 * q_limit > 0: only whole blocks of GV_ATTN_STREAM_QBLOCK query rows that hold a row < q_limit are computed; o / lse rows behind
 * the last such block are left untouched (the CLS-only last block asks for 1).  0 = every query.
 * No atomics: the result of an (image, head) pair depends neither on the launch geometry nor on the other pairs of the launch.
 * One plain launch (no cooperative launch, nothing waits on another workgroup), 32 KB of LDS.  Its backward is gv_attention_bwd_stream
 * (below), its attention maps are gv_attention_probs_stream's.  There is no _f32 form: the fp32 operand mode keeps its limit.        */
#define GV_ATTN_MAX_N 288            /* gv_attention_fwd / _bwd / _probs and the varlen calls */
#define GV_ATTN_F32_MAX_N 260        /* the _f32 entry points */
#define GV_ATTN_STREAM_MAX_N 1040
#define GV_ATTN_STREAM_QBLOCK 128
int gv_attention_fwd_stream(const gv_attention_fwd_args* a, void* stream);

/* Varlen forward (the `cu_seqlens` form): the token-concatenated row space of a multi-crop pass -- segment i
 * holds n_img[i] images of N[i] tokens, its rows start where segment i - 1 ends, qkv / o cover all segments, lse[i] is
 * segment i's f32 [n_img[i], H, N[i]].  A long (128 < N <= 224) + a short (32 < N <= 64) segment run as ONE launch
 * (the short pairs fill the long launch's last, half-empty round of workgroups); any other mix runs one launch per segment.
 * (gv_attention_bwd_varlen below takes the same segment table.)                                                              */
#define GV_ATTN_MAX_SEG 4
typedef struct {
    const void* qkv; void* o;
    int32_t n_seg; int32_t n_img[GV_ATTN_MAX_SEG]; int32_t N[GV_ATTN_MAX_SEG];
    float* lse[GV_ATTN_MAX_SEG];
    int32_t H; float scale;
    int32_t q_limit;      /* as gv_attention_fwd_args.q_limit, for every segment */
} gv_attention_fwd_varlen_args;
int gv_attention_fwd_varlen(const gv_attention_fwd_varlen_args* a, void* stream);

typedef struct {
    const void* qkv; const void* o; const void* d_o; const float* lse;
    void* dqkv;           /* bf16 [n_img*N, 3, H, 64]                        */
    int32_t n_img, N, H; float scale;
    int32_t q_limit;      /* > 0: d_o is zero behind the first q_limit query rows of every image (the caller guarantees it for the rows
                           * up to the next multiple of 32; rows behind that are not read): those queries are skipped and their dQ rows
                           * are written as zeros.  qkv / o / lse must be valid for the rows up to that multiple of 32 (what
                           * gv_attention_fwd with the same q_limit leaves).  0 = every query.                                      */
} gv_attention_bwd_args;
int gv_attention_bwd(const gv_attention_bwd_args* a, void* stream);

/* Streaming backward: gv_attention_bwd for 1 <= N <= GV_ATTN_STREAM_MAX_N, on the o / lse that gv_attention_fwd_stream left (16-bit
 * operands, head_dim 64; there is no _f32 form).  Checks, their order and their wording are the streaming forward's: a null pointer
 * (delta included) GV_E_NULL, any other N GV_E_SHAPE with the limit in gv_last_error(), scale <= 0 GV_E_SHAPE, a buffer that is not
 * 16-byte aligned GV_E_ALIGN -- all before any launch.
 * Two plain launches on the stream, the second behind the first:
 *   1. per (pair, block of GV_ATTN_STREAM_QBLOCK query rows): delta[q] = sum_d dO[q][d] O[q][d] in f32, stored to `delta`; K / V stream
 *      through LDS in key blocks; dQ accumulates in f32 over all key blocks and is rounded once, at the store (the q third of dqkv);
 *   2. per (pair, block of 128 keys): Q / dO rows stream through LDS with their lse / delta; dK and dV accumulate in f32 over all
 *      query rows and are rounded once, at the store (the k and v thirds).
 * Both recompute P = exp(scale q.k - lse[q]) from the f32 lse and round P and dS = P (dP - delta) scale to the 16-bit format before
 * their products, as gv_attention_bwd does.  Keys >= N are never counted, query rows >= N never read or stored.
 * No atomics, no cooperative launch, nothing waits on another workgroup: the only dependency between workgroups (delta) is the launch
 * boundary.  The result of an (image, head) pair depends neither on the launch geometry nor on the other pairs; a second call on the
 * same buffers gives the same bits.
 * q_limit > 0: with qe = min(N, q_limit rounded up to GV_ATTN_STREAM_QBLOCK), only query rows < qe are read (qkv's q, o, d_o, lse --
 * what gv_attention_fwd_stream with the same q_limit leaves); the caller guarantees d_o is zero in [q_limit, qe).  dQ rows >= qe are
 * written as zeros, dK / dV are the sums over the rows < qe.  0 = every query.                                                 */
typedef struct {
    const void* qkv; const void* o; const void* d_o; const float* lse;
    void* dqkv;           /* 16-bit [n_img*N, 3, H, 64] */
    float* delta;         /* scratch f32 [n_img, H, N]: written, then read, inside the call */
    int32_t n_img, N, H; float scale;
    int32_t q_limit;
} gv_attention_bwd_stream_args;
int gv_attention_bwd_stream(const gv_attention_bwd_stream_args* a, void* stream);

/* Varlen backward: the segment table of gv_attention_fwd_varlen (segment i: n_img[i] images of N[i] tokens, rows back to back in
 * qkv / o / d_o / dqkv; lse[i] as the forward left it).  One CALL for the multi-crop row space; inside, each length class runs as
 * its own launch: the long class (N > 64) holds a CU's LDS alone (114 - 142 KB per (image, head) pair) while the short classes
 * run 4 - 5 workgroups per CU, so a shared launch geometry would cost the short pairs their occupancy.  */
typedef struct {
    const void* qkv; const void* o; const void* d_o; void* dqkv;
    int32_t n_seg; int32_t n_img[GV_ATTN_MAX_SEG]; int32_t N[GV_ATTN_MAX_SEG];
    const float* lse[GV_ATTN_MAX_SEG];
    int32_t H; float scale;
    int32_t q_limit;      /* as gv_attention_bwd_args.q_limit, for every segment */
} gv_attention_bwd_varlen_args;
int gv_attention_bwd_varlen(const gv_attention_bwd_varlen_args* a, void* stream);

/* ---- attention probabilities: the softmax matrix of Attention.forward (vit.pyc@L119-131) that the reference returns from
 * get_last_selfattention (vit.pyc@L255-262: blocks[:-1], then the last block with return_attention=True, L146-152).
 * gv_attention_fwd never writes it; this call recomputes it from the same q / k and the lse that forward left:
 *     p[img, h, q, key] = exp(scale * q.k - lse[img, h, q])     for q < q_rows, key < N
 * so P is exactly the softmax that produced o (one pass, no row reduction).  p is compact and need not be aligned: at N = 257 a
 * row is 1 028 bytes.  q_rows = 1 is the CLS row (a forward with q_limit = 1 leaves lse valid for it); q_rows = N needs a
 * forward with q_limit = 0.  N <= GV_ATTN_MAX_N, head_dim 64 (the _f32 entry point: N <= GV_ATTN_F32_MAX_N, every 16-bit buffer
 * as f32).                                                                                                                   */
typedef struct {
    const void*  qkv;   /* 16-bit [n_img*N, 3, H, 64], as gv_attention_fwd read it                          */
    const float* lse;   /* f32 [n_img, H, N], as gv_attention_fwd left it: rows [0, q_rows) must be valid */
    float*       p;     /* f32 [n_img, H, q_rows, N] compact: p = exp(q.k * scale - lse[q])               */
    int32_t n_img, N, H; float scale;
    int32_t q_rows;     /* 1..N: query rows 0..q_rows-1 of every image (1 = the CLS row)                  */
} gv_attention_probs_args;
int gv_attention_probs(const gv_attention_probs_args* a, void* stream);
int gv_attention_probs_f32(const gv_attention_probs_args* a, void* stream);   /* every 16-bit buffer as f32 */

/* Streaming probabilities: gv_attention_probs for 1 <= N <= GV_ATTN_STREAM_MAX_N, on the qkv and the lse that gv_attention_fwd_stream
 * left (16-bit operands, head_dim 64; there is no _f32 form).  Same argument struct, same contract:
 *     p[img, h, q, key] = exp(scale * q.k - lse[img, h, q])     for q < q_rows, key < N,   1 <= q_rows <= N
 * p is f32 [n_img, H, q_rows, N], compact, no alignment assumed (at N = 1 025 a row is 4 100 bytes: 4-byte stores).
 * Checks, their order and their wording are the streaming forward's: a null pointer GV_E_NULL, any other N GV_E_SHAPE with the limit
 * in gv_last_error(), q_rows outside 1..N GV_E_SHAPE, scale <= 0 GV_E_SHAPE, a qkv that is not 16-byte aligned GV_E_ALIGN -- all
 * before any launch.
 * Only lse rows [0, q_rows) are read: the rows behind them may hold anything (after a forward with q_limit = 1 they do; that forward
 * computes the first GV_ATTN_STREAM_QBLOCK rows, so q_rows up to that many are served by it).  Keys >= N are never written, nothing
 * before p[0] or behind p[n_img*H*q_rows*N - 1] is touched.
 * The arithmetic is gv_attention_probs': s = the f32 result of two 16x16x32 MFMAs (d = 0..31, then 32..63), p = exp2(fma(s,
 * scale log2e, -lse log2e)).  Given the same lse buffer the two calls write the same bits at every N <= GV_ATTN_MAX_N, and a row of p
 * depends neither on q_rows, nor on which of the two forms ran, nor on the launch geometry, nor on the other pairs of the launch:
 *   q_rows <= 16 (the CLS row): a workgroup per (image, head) pair reads every K element once, straight from global; no LDS;
 *   more rows: a workgroup per (pair, block of GV_ATTN_STREAM_QBLOCK query rows), of which only ceil(q_rows / QBLOCK) are launched;
 *              K streams through LDS in key blocks (16 KB), each 16 x 16 tile is stored as soon as it is computed.
 * One plain launch: no atomics, no cooperative launch, nothing waits on another workgroup.                                     */
int gv_attention_probs_stream(const gv_attention_probs_args* a, void* stream);

/* ---- token assembly (vit.pyc@L235-246 prepare_tokens: CLS row) ---------
 * x[i*N + 0, :] = cls[:] + pos[0, :] for every image i.                    */
typedef struct { float* x; const float* cls; const float* pos; int32_t n_img, N, D; } gv_cls_rows_args;
int gv_cls_rows(const gv_cls_rows_args* a, void* stream);

/* backward of token assembly: from g f32 [n_img*N, D] produce
 *   gpatch bf16 [n_img*P, D] (compact patch rows, A operand of dW_patch),
 *   dpos f32 [N, D] (+)= sum_i g[i*N + t]  (dcls = dpos row 0 before the add
 *   is also written to dcls (+)=).                                           */
typedef struct {
    const float* g; void* gpatch; float* dpos; float* dcls;
    int32_t n_img, N, D; int32_t accumulate;
} gv_tokens_bwd_args;
int gv_tokens_bwd(const gv_tokens_bwd_args* a, void* stream);

/* small strided matmul C[m,n] (+)= sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] (+ bias[n]);
 * element strides, each operand f32 or bf16.  For the tiny products of the path: the
 * bicubic pos-embed resampling (vit.pyc@L213-233) as a fixed linear map, and the
 * supervised classifier head Linear(D, num_classes) (train.py:482-495, num_classes=2). */
typedef struct {
    const void* A; int32_t a_is_bf16; int64_t sam, sak;
    const void* B; int32_t b_is_bf16; int64_t sbk, sbn;
    void* C; int32_t c_is_bf16; int64_t ldc;
    const float* bias;
    int32_t M, N, K; int32_t accumulate;
} gv_small_matmul_args;
int gv_small_matmul(const gv_small_matmul_args* a, void* stream);

/* ---- DINOHead tail (vit.pyc@L326-330) ---------------------------------
 * l2norm fwd: y bf16 = x / max(||x||, 1e-12), inv_norm f32 [rows] saved.    */
typedef struct { const float* x; void* y; float* inv_norm; int32_t rows, C; } gv_l2norm_fwd_args;
int gv_l2norm_fwd(const gv_l2norm_fwd_args* a, void* stream);
/* bwd: dx bf16 = (dy - y (y.dy)) * inv_norm  (dy f32, y bf16)               */
typedef struct { const float* dy; const void* y; const float* inv_norm; void* dx; int32_t rows, C; } gv_l2norm_bwd_args;
int gv_l2norm_bwd(const gv_l2norm_bwd_args* a, void* stream);
/* weight_norm: w bf16 [K,C] = g[k] * v[k,:] / ||v[k,:]||                    */
typedef struct { const float* v; const float* g; void* w; int32_t rows, C; } gv_weightnorm_fwd_args;
int gv_weightnorm_fwd(const gv_weightnorm_fwd_args* a, void* stream);
/* bwd: dv (+)= g/||v|| (dw - vhat (vhat.dw)); dg (+)= vhat.dw (dg may be NULL) */
typedef struct {
    const float* dw; const float* v; const float* g; float* dv; float* dg;
    int32_t rows, C; int32_t accumulate;
} gv_weightnorm_bwd_args;
int gv_weightnorm_bwd(const gv_weightnorm_bwd_args* a, void* stream);

/* ---- DINO loss (paper Alg. 1; absent from the reference)
 * student f32 [V*B, K] crop-major, teacher f32 [G*B, K] crop-major.
 * Writes loss (scalar f32, mean over the G*(V-1)... pairs and B), dstudent
 * bf16 [V*B, K] = d loss / d student * grad_scale, and center_sum f32 [K] =
 * sum over teacher rows of the raw teacher logits.
 * workspace: f32 [2 * (V+G) * B] row stats.                                 */
typedef struct {
    const float* student; const float* teacher; const float* center;
    void* dstudent; float* loss; float* center_sum; float* workspace;
    int32_t B, V, G, K;
    float student_temp, teacher_temp, grad_scale;
    const float* hyper;   /* optional device vector (see gv_adamw_ema_args): temps */
    const float* loss_scale; /* optional DEVICE scalar: dstudent is multiplied by it (fp16 loss scaling, gv_loss_scale_update) */
} gv_dino_loss_args;
int gv_dino_loss(const gv_dino_loss_args* a, void* stream);

/* center <- m * center + (1-m) * center_sum / n_rows (after the all-reduce) */
typedef struct { float* center; const float* center_sum; int32_t K; float momentum; float inv_rows; } gv_center_update_args;
int gv_center_update(const gv_center_update_args* a, void* stream);

/* ---- supervised head loss (train.py:1046 softmax, :1053 LabelSmoothingCE on
 * the soft-maxed output, gather index target[B,1] per train_instruct.txt:3-7).
 * logits f32 [B,C] (C <= 64), target i64 [B]; loss scalar; dlogits f32 [B,C].*/
typedef struct {
    const float* logits; const int64_t* target; float* loss; float* dlogits; float* prob;
    int32_t B, C; float smoothing;
    const float* loss_scale; /* optional DEVICE scalar: dlogits is multiplied by it (fp16 loss scaling); the loss itself is not */
} gv_softmax_lsce_args;
int gv_softmax_lsce(const gv_softmax_lsce_args* a, void* stream);

/* ---- supervised head loss on mixed / soft targets (train.py:832-842: timm SoftTargetCrossEntropy or BinaryCrossEntropy
 * once mixup / cutmix is active or --bce-loss is given; :1046 softmax first, so the loss sees the SOFT-MAXED output p).
 * The dense target of timm's mixup_target is built in registers, never in memory:
 *     off = smoothing / C;  on = 1 - smoothing + off
 *     t[b, c] = lam[b] * (c == y[b] ? on : off) + (1 - lam[b]) * (c == y[partner[b]] ? on : off)
 *     has_threshold:  t = t > threshold ? 1 : 0                                        (GV_MIX_LOSS_BCE only)
 *   GV_MIX_LOSS_SOFT_CE  loss = mean_b sum_c -t * log_softmax(p)
 *   GV_MIX_LOSS_BCE      loss = mean_{b,c} binary_cross_entropy_with_logits(p, t)
 * logits f32 [B, C] (C <= 64), target i64 [B]; loss scalar; dlogits f32 [B, C] = d loss / d logits (through both the
 * softmax and the loss).  partner NULL: no mixing (timm's one-hot-with-smoothing branch); lam NULL: 1.  A partner
 * outside [0, B) counts as the row itself. */
enum { GV_MIX_LOSS_SOFT_CE = 0, GV_MIX_LOSS_BCE = 1 };
typedef struct {
    const float* logits; const int64_t* target; const int32_t* partner; const float* lam;
    float* loss; float* dlogits; float* prob;
    int32_t B, C; float smoothing;
    int32_t kind, has_threshold; float threshold;
    const float* loss_scale; /* optional DEVICE scalar: dlogits is multiplied by it (fp16 loss scaling); the loss itself is not */
} gv_softmax_mix_loss_args;
int gv_softmax_mix_loss(const gv_softmax_mix_loss_args* a, void* stream);

/* ---- gather / scatter of CLS rows: y[i,:] = x[i*N, :] (f32 -> bf16) -------*/
typedef struct { const float* x; void* y; int32_t n_img, N, D; } gv_gather_cls_args;
int gv_gather_cls(const gv_gather_cls_args* a, void* stream);

/* ---- mean pooling of the patch tokens (`--gp avg`, reference train.py:490 -> timm global_pool='avg': x[:, 1:].mean(dim=1) in
 * front of fc_norm; the CLS row is excluded).  x f32 [n_img * N, D] compact (the residual stream), pooled f32 [n_img, D]:
 *   fwd: pooled[i, :] = sum over t = 1 .. N-1 of x[i*N + t, :], divided by N - 1.  f32 accumulation, no atomics; the summation
 *        order is fixed by (N, D) alone, so the result is bitwise reproducible.
 *   bwd: for every row t >= 1 of image i: g[i*N + t, :] = dpool[i, :] / (N - 1) (f32, the residual-stream gradient) and
 *        gb[i*N + t, :] = bf16(g * gb_scale[i]); row t = 0 (CLS) is written as zeros in both.  Every row of g and gb is written.
 * N < 2 or D % 4 != 0: GV_E_SHAPE, a null pointer (gb_scale excepted): GV_E_NULL, both before any launch.                   */
typedef struct { const float* x; float* pooled; int32_t n_img, N, D; } gv_token_mean_fwd_args;
int gv_token_mean_fwd(const gv_token_mean_fwd_args* a, void* stream);
typedef struct {
    const float* dpool;    /* f32 [n_img, D]                                                                       */
    float* g;              /* f32 [n_img * N, D] out                                                               */
    void* gb;              /* bf16 [n_img * N, D] out (f32 in gv_token_mean_bwd_f32)                               */
    const float* gb_scale; /* optional [n_img]: the stochastic-depth factor of the branch gb enters; NULL = 1      */
    int32_t n_img, N, D;
} gv_token_mean_bwd_args;
int gv_token_mean_bwd(const gv_token_mean_bwd_args* a, void* stream);

/* dst[i] = vals[i] for i < n <= 16: per-step schedule values (gv_adamw_ema_args.hyper)
 * delivered as KERNEL ARGUMENTS of a stream-ordered launch rather than by a memcpy.     */
typedef struct { float* dst; float vals[16]; int32_t n; } gv_store_f32_args;
int gv_store_f32(const gv_store_f32_args* a, void* stream);

/* f32 -> bf16 cast of a flat buffer (weight arena refresh)                  */
typedef struct { const float* src; void* dst; int64_t n; } gv_cast_bf16_args;
int gv_cast_bf16(const gv_cast_bf16_args* a, void* stream);

/* sum of squares of a flat f32 buffer -> out[0] (+)= ; workspace >= 1024 f32 */
typedef struct { const float* x; int64_t n; float* workspace; float* out; int32_t accumulate; } gv_sumsq_args;
int gv_sumsq(const gv_sumsq_args* a, void* stream);

/* ---- fused AdamW + teacher EMA + bf16 refresh over a flat parameter arena
 * (train.py:1078 optimizer.step; :1080-1081 model_ema.update).
 *   if clip_norm > 0: scale = min(1, clip_norm / (sqrt(*gnorm_sq) + 1e-6))
 *   g = grad * grad_scale * scale;  p *= 1 - lr*wd;  m,v Adam;  p -= ...
 *   p_bf16 = bf16(p);  if teacher: t = mom*t + (1-mom)*p; t_bf16 = bf16(t)   */
typedef struct {
    float* p; const float* grad; float* m; float* v; void* p_bf16;
    float* teacher; void* teacher_bf16;
    int64_t n;
    float lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2;
    float grad_scale, clip_norm; const float* gnorm_sq;
    float teacher_momentum;
    /* optional DEVICE vector; when non-NULL it overrides the by-value scalars (except
     * weight_decay, which then MULTIPLIES hyper[GV_HYP_WD]: 1 = decayed, 0 = not) so a
     * captured hipGraph can be replayed with new schedules:
     * [GV_HYP_LR, GV_HYP_WD, GV_HYP_BC1, GV_HYP_BC2, GV_HYP_TEACHER_MOM, GV_HYP_GRAD_SCALE,
     *  GV_HYP_TEACHER_TEMP, GV_HYP_STUDENT_TEMP] */
    const float* hyper;
    /* 0 = AdamW (decoupled decay, torch.optim.AdamW); 1 = Adam with L2 decay folded into the
     * gradient (timm --opt adam, the documented runs: train_instruct.txt:23); 2 = SGD with
     * Nesterov momentum beta1 and L2 decay (timm --opt sgd, the reference default, train.py:161);
     * `m` is the momentum buffer, `v` is unused in mode 2; 3 = frozen range: p, m, v are left
     * untouched (a parameter without a gradient is skipped by torch optimizers: reference
     * train.py:497-503 --no-grad, DINO's frozen last layer) and only the teacher EMA / bf16
     * refresh run.                                                                           */
    int32_t mode;
    /* > 0: every gradient element (after grad_scale) is clamped to [-clip_value, clip_value] -- `--clip-mode value`,
     * torch.nn.utils.clip_grad_value_ (reference train.py:1072-1077 dispatch_clip_grad); use instead of clip_norm */
    float clip_value;
    /* optional: the DEVICE state vector of gv_loss_scale_update, [S, .., .., applied steps] (fp16 loss scaling,
     * torch.cuda.amp.GradScaler as driven by timm's NativeScaler: reference train.py:585-602, 1061-1070).  The gradient was
     * produced from S * loss, so g = grad * grad_scale / S (the clip norm is that of the unscaled gradient); when *gnorm_sq
     * (required then) is not finite the call leaves p, m, v untouched -- GradScaler.step() skips optimizer.step() -- while the
     * teacher / --model-ema update and the 16-bit refresh still run; and Adam's bias corrections are taken at step
     * state[3] + 1 (the optimizer's own count of applied steps) instead of the by-value / hyper ones.                        */
    const float* loss_scale;
} gv_adamw_ema_args;
int gv_adamw_ema(const gv_adamw_ema_args* a, void* stream);

/* ---- the same pass over a RANGE TABLE: per-range learning-rate scale and weight-decay multiplier in ONE launch
 * (`--layer-decay`, reference train.py:175 -> optimizer_kwargs -> timm create_optimizer_v2 -> param_groups_layer_decay: one
 * parameter group per (layer, decay | no-decay), each at lr * lr_scale, the scheduler multiplying every group's rate by its
 * lr_scale -- SURVEY Appendix B).  Every field gv_adamw_ema_args carries keeps its meaning; range r is stepped with
 *     lr_r = lr * ranges[r][0]  (formed once, in f32; `lr` is hyper[GV_HYP_LR] when hyper is given)
 *     wd_r = weight_decay * ranges[r][1]          (weight_decay after the hyper[GV_HYP_WD] multiplication)
 * and the global-norm / value clip, the loss-scaled skip on a non-finite *gnorm_sq (p, m, v untouched in every range, the
 * EMA copy still moves), the applied-step bias corrections, the EMA copy and both 16-bit refreshes are gv_adamw_ema's:
 * both kernels call one per-element device function, so with lr_scale = 1 the results are bit-identical to gv_adamw_ema
 * calls over the same ranges.  mode 0 / 1 / 2 only: a frozen range is simply left out of the table.
 *   blocks: device int32 [n_blocks][3] = {range, lo, hi}: elements [lo, hi) of the buffers, all of range `range`, taken by
 *           one workgroup -- rows of bounded length that never cross a range (the ranges differ in size by three orders
 *           of magnitude), lo / hi multiples of 4, 0 <= lo < hi <= n; a row outside [0, n) or naming no range is skipped;
 *   ranges: device f32 [n_ranges][2] = {lr_scale, wd_multiplier}.
 * Elements no row covers are not touched at all (no 16-bit refresh, no EMA).                                          */
typedef struct {
    float* p; const float* grad; float* m; float* v; void* p_bf16;
    float* teacher; void* teacher_bf16;
    int64_t n;                   /* length of the buffers in elements: the bound every table row is checked against */
    float lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2;
    float grad_scale, clip_norm; const float* gnorm_sq;
    float teacher_momentum;
    const float* hyper;
    int32_t mode;                /* 0 AdamW, 1 Adam + L2, 2 SGD Nesterov */
    float clip_value;
    const float* loss_scale;
    const int32_t* blocks; int32_t n_blocks;
    const float* ranges; int32_t n_ranges;
} gv_adamw_ema_ranges_args;
int gv_adamw_ema_ranges(const gv_adamw_ema_ranges_args* a, void* stream);

/* ---- GradScaler.update() (torch.cuda.amp.GradScaler: init_scale 65536, growth_factor 2, backoff_factor 0.5, growth_interval
 * 2000): state[0] = S, state[1] = number of consecutive finite steps, state[2] = number of skipped steps so far (for the log),
 * state[3] = number of applied optimizer steps.
 * *gnorm_sq = sum of squares of the scaled gradient arena (after the data-parallel all-reduce, so every rank decides alike):
 *   not finite:  S *= backoff_factor, state[1] = 0, state[2] += 1
 *   finite:      state[3] += 1;  if ++state[1] == growth_interval: S *= growth_factor, state[1] = 0
 * One thread, stream-ordered behind the optimizer launches that read S; nothing returns to the host.                         */
typedef struct {
    float* state; const float* gnorm_sq;
    float growth_factor, backoff_factor; int32_t growth_interval;
} gv_loss_scale_update_args;
int gv_loss_scale_update(const gv_loss_scale_update_args* a, void* stream);

/* ---- dropout (`--drop`, reference train.py:283-284 -> create_model(drop_rate): nn.Dropout after the pos-embed add, after attn.proj,
 * after the MLP activation and after mlp.fc2; vit.pyc@L98-104, L119-131, L235-246).  Counter-based masks, so that the backward
 * regenerates what the forward used and the oracle can restate it: element i of a site is KEPT iff
 *   fmix32(seed + 0x9E3779B9 * (i + 1)) >= threshold,   threshold = floor(p * 2^32)   (murmur3 finaliser)
 * and kept values are scaled by `scale` = 1 / (1 - p).  `seed` is the site's own (host: one per step, layer and site).
 * gv_dropout: in place on x (bf16, or f32 with x_is_f32) -- an activation in the forward, the gradient entering the same site
 * in the backward.  gv_dropout_add: out[m, :] = resid[m, :] + row_scale[m] * dropout(t[m, :]) for the two residual branches
 * (t = the branch's Linear output incl. bias, f32; row_scale: stochastic depth, may be NULL).  Element index = m * cols + c.
 * These run only when --drop > 0 (the step then takes the unfused Linear / LayerNorm kernels); the default path is untouched. */
typedef struct { void* x; int32_t x_is_f32; int64_t n; uint32_t seed, threshold; float scale; } gv_dropout_args;
int gv_dropout(const gv_dropout_args* a, void* stream);
typedef struct {
    const float* t; const float* resid; float* out; const float* row_scale;
    int32_t rows, cols; uint32_t seed, threshold; float scale;
} gv_dropout_add_args;
int gv_dropout_add(const gv_dropout_add_args* a, void* stream);

/* ---- adaptive gradient clipping (`--clip-mode agc`, reference train.py:1072-1077 -> timm.utils.adaptive_clip_grad): per UNIT
 * (a row of a matrix / conv filter = dim 0 of the parameter; a whole tensor for 1-D parameters and for tensors whose dim 0 is 1)
 *   g_u <- g_u * min(1, clip_factor * max(||p_u||, eps) / max(||g_u||, 1e-6)),   g_u = grad_u * grad_scale for the norms
 * in place on the (unscaled) gradient arena, before the optimizer pass.  units: device int32 [n_units][2] = {offset, length}
 * into p / grad (offsets multiples of 4 are not required).  One wave per unit.                                            */
typedef struct {
    const float* p; float* grad; const int32_t* units; int32_t n_units;
    float clip_factor, eps, grad_scale;
} gv_agc_args;
int gv_agc(const gv_agc_args* a, void* stream);

/* ---- LAMB (timm `--opt lamb`, reference train.py:161 -> create_optimizer_v2 -> timm.optim.Lamb; named in SURVEY 8f-4) over the
 * same flat arena, two launches per range (a per-TENSOR trust ratio needs every tensor's norms before its update):
 *   phase 0:  g = grad * grad_scale * c, c = the global-norm clips (clip_norm as in gv_adamw_ema, then Lamb's own
 *             max_grad_norm: g /= max(||g|| / max_grad_norm, 1));  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
 *             u = (m / bias_corr1) / (sqrt(v) / sqrt(bias_corr2) + eps) + weight_decay * p;
 *             stats[2 t] += ||p||^2, stats[2 t + 1] += ||u||^2 over tensor t  (the caller zeroes `stats` first)
 *   phase 1:  p -= lr * r_t * u with r_t = ||p|| / ||u|| if weight_decay != 0 and both norms > 0, else 1 (timm:
 *             always_adapt = False);  bf16 refresh + teacher / --model-ema EMA as in gv_adamw_ema.
 * `blocks`: device int32 [n_blocks][3] = {tensor, lo, hi}: element range [lo, hi) of the arena range handled by one
 * workgroup, never crossing a tensor (built once by the host from the arena layout; lo, hi multiples of 4).            */
typedef struct {
    float* p; const float* grad; float* m; float* v; void* p_bf16;
    float* teacher; void* teacher_bf16;
    const int32_t* blocks; int32_t n_blocks;
    float* stats;                /* f32 [2 * n_tensors]                                                              */
    float lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2;
    float grad_scale, clip_norm, max_grad_norm; const float* gnorm_sq;     /* gnorm_sq: sum of squares of the raw gradient */
    float teacher_momentum;
    int32_t phase;
    /* optional: device f32 [n_tensors], tensor t is stepped at lr * lr_scale[t] in phase 1 (`--layer-decay`; the trust ratio and
     * both clips do not depend on the rate).  NULL = every tensor at lr                                                */
    const float* lr_scale;
} gv_lamb_args;
int gv_lamb(const gv_lamb_args* a, void* stream);

/* ---- fp32 operand mode (SURVEY 8d fp32 column; the reference's default arithmetic, train.py without --amp) -------
 * The same entry points with EVERY bf16 buffer of the argument struct read / written as f32 instead (activations,
 * GEMM operands incl. the weights, aux_in / aux_out, attention q/k/v/o/dO/dqkv, LayerNorm y / dy / gb, patch rows);
 * f32 fields keep their meaning.  Linear: v_mfma_f32_16x16x4_f32, any M / N / K, exact erf GELU and GELU', c_is_f32
 * must be 1, workspace ignored (pure-ACCUM launches with few output tiles split K through f32 atomics).
 * Attention: N <= GV_ATTN_F32_MAX_N.  A parity mode: it holds the 1e-4 logits / loss and 1e-3 gradient-norm gates against the fp32
 * oracle (tests/test_fp32_gpu.py); the training path stays bf16.                                                   */
int gv_linear_f32(const gv_linear_args* a, void* stream);
int gv_attention_fwd_f32(const gv_attention_fwd_args* a, void* stream);
int gv_attention_bwd_f32(const gv_attention_bwd_args* a, void* stream);
int gv_layernorm_fwd_f32(const gv_layernorm_fwd_args* a, void* stream);
int gv_layernorm_bwd_f32(const gv_layernorm_bwd_args* a, void* stream);
int gv_patchify_f32(const gv_patchify_args* a, void* stream);
int gv_patchify_nchw_f32(const gv_patchify_nchw_args* a, void* stream);    /* exact copy into f32 patch rows */
int gv_patchify_mix_f32(const gv_patchify_mix_args* a, void* stream);
int gv_patchify_nchw_mix_f32(const gv_patchify_nchw_mix_args* a, void* stream);
int gv_patchify_erase_f32(const gv_patchify_erase_args* a, void* stream);
int gv_patchify_stain_f32(const gv_patchify_stain_args* a, void* stream);
int gv_patchify_nchw_erase_f32(const gv_patchify_nchw_erase_args* a, void* stream);
int gv_tokens_bwd_f32(const gv_tokens_bwd_args* a, void* stream);
int gv_token_mean_bwd_f32(const gv_token_mean_bwd_args* a, void* stream);      /* gb f32 */
/* DINO head: zn / dz (l2norm), the weight-normalised last-layer matrix, and the student-logit gradient as f32 */
int gv_l2norm_fwd_f32(const gv_l2norm_fwd_args* a, void* stream);
int gv_l2norm_bwd_f32(const gv_l2norm_bwd_args* a, void* stream);
int gv_weightnorm_fwd_f32(const gv_weightnorm_fwd_args* a, void* stream);
int gv_dino_loss_f32(const gv_dino_loss_args* a, void* stream);

/* ---- weighted k-NN vote on frozen features: DINO's knn_classifier, the training monitor of a --dino run (gipvit/knn.py).
 * For query row q and bank row b, both already L2-normalised (gv_l2norm_fwd_f32):
 *     sim = q . b in f32;  the k largest sim over the whole bank;
 *     votes[q, c] = sum over those k of exp(sim_j * inv_temp) * [labels[idx_j] == c].
 * The Q x Nb similarity matrix is never written: one launch walks the bank in 128-row chunks on the f32 MFMA and keeps a sorted
 * (sim, idx) list of length k per query on chip, per bank split; a second small launch merges the n_split lists and votes.
 * f32 only (both library builds), no atomics: the result is the same run to run.
 * Order, part of the contract: similarity descending and, among equal similarities, the smaller bank index first -- for every
 * split count; top_sim is bitwise the same for every split count.  A label outside [0, C) votes for no class and is never used
 * as an index.  Limits: Q >= 1, 1 <= k <= 64, k <= Nb, D a multiple of 4 and <= 1024, 1 <= C <= 32, ldq / ldb multiples of 4
 * and >= D, q / bank 16-byte aligned, 0 <= n_split <= min(32, Nb), workspace_bytes >= gv_knn_workspace_bytes(Q, Nb, k, n_split). */
typedef struct {
    const float*   q;        /* f32 [Q, D], row stride ldq                                              */
    const float*   bank;     /* f32 [Nb, D], row stride ldb                                             */
    const int32_t* labels;   /* i32 [Nb]                                                                */
    float*         votes;    /* f32 [Q, C]                                                              */
    float*         top_sim;  /* f32 [Q, k], non-increasing; may be NULL                                 */
    int32_t*       top_idx;  /* i32 [Q, k], bank rows of top_sim; may be NULL                           */
    void*          workspace; int64_t workspace_bytes;   /* caller-owned scratch: the per-split lists   */
    int32_t Q, Nb, D, k, C;
    int32_t n_split;         /* 0: the library chooses (a workgroup per CU); > 0: that many bank splits */
    int64_t ldq, ldb;        /* row strides in elements                                                 */
    float   inv_temp;        /* 1 / temperature (DINO: 1 / 0.07)                                        */
} gv_knn_vote_args;
int gv_knn_vote(const gv_knn_vote_args* a, void* stream);
/* scratch bytes of one gv_knn_vote call (n_split as in the call; 0 resolves as the call would); -1 with gv_last_error() set
 * for arguments the call would refuse.  Touches no GPU.                                                                    */
int64_t gv_knn_workspace_bytes(int32_t Q, int32_t Nb, int32_t k, int32_t n_split);

/* ---- linear probe on frozen features: DINO's eval_linear as H linear heads over F features and C classes, trained together so
 * that every head shares one read of every feature row (gipvit/linprobe.py; a grid of learning rates in one pass over the bank).
 * State, caller-owned f32: W [H, C, F], b [H, C], momentum buffers mW / mb of the same shapes, lr [H], wd [H].
 * gv_linprobe_train performs ceil(n_rows / batch) SGD steps over x[rows[...]], all enqueued on the stream; the last step takes the
 * n_rows % batch rows that are left and averages over that count.  One step on the rows r_0 .. r_{m-1}, per head h, in f32:
 *     z[h,j,c] = b[h,c] + sum_f W[h,c,f] x[r_j,f];  p = softmax_c(z) (max-subtracted);  loss_sum[h] += sum_j -log p[h,j,y_j]
 *     g[h,j,c] = (p[h,j,c] - [c == y_j]) / m
 *     dW[h,c,:] = sum_j g[h,j,c] x[r_j,:] + wd[h] W[h,c,:];   db[h,c] = sum_j g[h,j,c] + wd[h] b[h,c]
 *     mW = momentum mW + dW;  W -= lr[h] lr_scale mW          (same for b)
 * -- torch.optim.SGD(momentum, weight_decay) on nn.Linear heads under a mean cross-entropy loss.  loss_sum is accumulated across
 * calls (the caller zeroes it).  A step is two launches: logits on the f32 MFMA per 64-row tile (g and per-tile partial sums go to
 * the workspace), then dW = g^T x per 32 columns of F with the update in the epilogue (dW never reaches memory).  No grid barrier,
 * no atomics, every sum in a fixed order that does not depend on the grid: the result, loss_sum included, is bitwise the same run
 * to run.  Every load is bounds-checked (padding is zero-filled, never read).  A label outside [0, C) or a row index outside
 * [0, N) is never used as an index: that row contributes nothing (the step still divides by m).
 * Limits: 1 <= C <= 32, H >= 1, H * C <= 64, F a multiple of 4 and <= 4096, ldx >= F and a multiple of 4, x and W 16-byte aligned,
 * 1 <= batch <= 4096, n_rows >= 1, N >= 1, lr_scale finite and >= 0, 0 <= momentum < 1,
 * workspace (16-byte aligned) of gv_linprobe_workspace_bytes(batch, H, C, F) bytes. */
typedef struct {
    float*         W;        /* f32 [H, C, F]                                                            */
    float*         b;        /* f32 [H, C]                                                               */
    float*         mW;       /* f32 [H, C, F] momentum buffer                                            */
    float*         mb;       /* f32 [H, C]    momentum buffer                                            */
    const float*   lr;       /* f32 [H]                                                                  */
    const float*   wd;       /* f32 [H]                                                                  */
    const float*   x;        /* f32 [N, F], row stride ldx                                               */
    const int32_t* labels;   /* i32 [N]                                                                  */
    const int32_t* rows;     /* i32 [n_rows]: the visiting order, any multiset of row indices            */
    float*         loss_sum; /* f32 [H], accumulated                                                     */
    void*          workspace; int64_t workspace_bytes;
    int64_t ldx;
    int32_t N, F, H, C, n_rows, batch;
    float   lr_scale;        /* the schedule's factor for these steps                                    */
    float   momentum;        /* SGD momentum (DINO: 0.9)                                                 */
} gv_linprobe_train_args;
int gv_linprobe_train(const gv_linprobe_train_args* a, void* stream);
/* prob[q, h, c] = softmax_c of the same logits for every row of x [Q, F]; with labels and loss non-NULL also loss[h] = the sum
 * over q of -log prob[q, h, labels[q]] (overwritten; a label outside [0, C) adds nothing).  Same limits; any Q >= 1 (chunks of
 * 4096 rows), workspace of gv_linprobe_workspace_bytes(min(Q, 4096), H, C, F) bytes.                                          */
typedef struct {
    const float*   W;        /* f32 [H, C, F]                                                            */
    const float*   b;        /* f32 [H, C]                                                               */
    const float*   x;        /* f32 [Q, F], row stride ldx                                               */
    const int32_t* labels;   /* i32 [Q]; may be NULL when loss is                                        */
    float*         prob;     /* f32 [Q, H, C]                                                            */
    float*         loss;     /* f32 [H]; may be NULL                                                     */
    void*          workspace; int64_t workspace_bytes;
    int64_t ldx;
    int32_t Q, F, H, C;
} gv_linprobe_predict_args;
int gv_linprobe_predict(const gv_linprobe_predict_args* a, void* stream);
/* scratch bytes of a gv_linprobe_train call with this batch (gv_linprobe_predict: batch = min(Q, 4096)); -1 with gv_last_error()
 * set for arguments the call would refuse.  Touches no GPU.                                                                    */
int64_t gv_linprobe_workspace_bytes(int32_t batch, int32_t H, int32_t C, int32_t F);

/* ---- attention-MIL probe on frozen features: gated-attention ABMIL (Ilse et al. 2018) over bags of feature rows, one bag per
 * slide (gipvit/mil.py).  Bag b holds the rows bag_ptr[b] .. bag_ptr[b + 1] - 1 of x (a CSR over rows), its label is labels[b].
 * State, caller-owned f32, ONE packed vector of P = (2 L + C) F + 3 L + C + 1 values, the Adam moments m and v in the same layout:
 *     VU [2 L, F] (rows 0 .. L-1: V, rows L .. 2L-1: U) | Wc [C, F] | bv [L] | bu [L] | w [L] | bc [C] | bw [1]
 * The model, per bag of rows x_1 .. x_n, in f32:
 *     t_i = tanh(V x_i + bv);  g_i = sigmoid(U x_i + bu);  s_i = w . (t_i * g_i) + bw;  a = softmax_i(s) (max-subtracted)
 *     z = sum_i a_i x_i;  logits = Wc z + bc;  p = softmax_c(logits);  the bag's loss is -log p[label]
 * gv_mil_train performs ceil(n_bags / batch) steps over the bags bags[0 .. n_bags), all enqueued on the stream; the last step
 * takes the bags that are left.  A step is torch.optim.Adam(lr lr_scale, (beta1, beta2), eps, weight_decay = wd) on every
 * parameter under the mean of the step's bag losses: the decay is added to the gradient, step k of the call (k = 0 ..) is Adam's
 * step step0 + k + 1, its bias corrections 1 - beta^t are computed on the host in double.  loss_sum is accumulated (the caller
 * zeroes it): the sum of the bag losses.  A step is three launches, every dependency a launch boundary (no grid barrier, no
 * atomics): the gate (64 rows of a bag x 32 hidden units per workgroup on the f32 MFMA; t, g and partial scores go to the
 * workspace), the pool (a workgroup per bag: softmax, z, logits, loss, and the backward down to ds_i), the update (dV | dU =
 * (dt | dg)^T x per 64 hidden columns x 32 columns of F with Adam in the epilogue; no weight gradient reaches memory).  Every sum
 * has an order fixed by the data layout: the result, loss_sum included, is bitwise the same run to run.  Every load is
 * bounds-checked (padding is zero-filled, never read); rows of x that no bag covers are never read.
 * A BAD BAG contributes nothing and is never used as an index: an index in `bags` outside [0, n_all_bags), an empty bag, one
 * longer than max_bag, a bag_ptr range outside [0, N], a label outside [0, C).  A step averages over its good bags; a step
 * without a good bag changes nothing (Adam's step count still advances).
 * Limits: F a multiple of 4 in 4..4096, L a multiple of 16 in 16..256, 1 <= C <= 32, 1 <= batch <= 64, 1 <= max_bag <= 4096,
 * N >= 1, n_all_bags >= 1, n_bags >= 1, step0 >= 0, ldx >= F and a multiple of 4, x and params / m / v 16-byte aligned, lr_scale
 * finite and >= 0, lr > 0 and finite, wd >= 0, 0 <= beta1 < 1, 0 <= beta2 < 1, eps > 0, workspace (16-byte aligned) of
 * gv_mil_workspace_bytes(batch, max_bag, L, C, F) bytes. */
typedef struct {
    float*         params;   /* f32 [P], the layout above                                                */
    float*         m;        /* f32 [P] Adam's first moment                                              */
    float*         v;        /* f32 [P] Adam's second moment                                             */
    const float*   x;        /* f32 [N, F], row stride ldx                                               */
    const int32_t* bag_ptr;  /* i32 [n_all_bags + 1]                                                     */
    const int32_t* labels;   /* i32 [n_all_bags]                                                         */
    const int32_t* bags;     /* i32 [n_bags]: the visiting order, any multiset of bag indices            */
    float*         loss_sum; /* f32 [1], accumulated                                                     */
    void*          workspace; int64_t workspace_bytes;
    int64_t ldx;
    int32_t N, F, L, C, n_all_bags, n_bags, batch, max_bag;
    int32_t step0;           /* Adam steps taken before this call                                        */
    float   lr, lr_scale, wd, beta1, beta2, eps;
} gv_mil_train_args;
int gv_mil_train(const gv_mil_train_args* a, void* stream);
/* prob[j, :] = p of bag bags[j] (bags NULL: of bag j) for j < n_bags, zeros for a bad bag; optionally attn[r] = a_i and
 * score[r] = s_i for every row r of those bags (other rows are left as they are); with loss non-NULL (labels required) loss[0] =
 * the sum over the bags, in order, of -log p[label] -- a label outside [0, C) adds nothing -- overwritten, or added to what is
 * there with accumulate != 0 (two calls over two halves of a list then give the bits of one call over the list).  Same limits;
 * any n_bags >= 1 (groups of 64 bags), workspace of gv_mil_workspace_bytes(min(n_bags, 64), max_bag, L, C, F) bytes.            */
typedef struct {
    const float*   params;   /* f32 [P]                                                                  */
    const float*   x;        /* f32 [N, F], row stride ldx                                               */
    const int32_t* bag_ptr;  /* i32 [n_all_bags + 1]                                                     */
    const int32_t* labels;   /* i32 [n_all_bags]; may be NULL when loss is                               */
    const int32_t* bags;     /* i32 [n_bags]; may be NULL                                                */
    float*         prob;     /* f32 [n_bags, C]                                                          */
    float*         loss;     /* f32 [1]; may be NULL                                                     */
    float*         attn;     /* f32 [N]; may be NULL                                                     */
    float*         score;    /* f32 [N]; may be NULL                                                     */
    void*          workspace; int64_t workspace_bytes;
    int64_t ldx;
    int32_t N, F, L, C, n_all_bags, n_bags, max_bag;
    int32_t accumulate;
} gv_mil_predict_args;
int gv_mil_predict(const gv_mil_predict_args* a, void* stream);
/* scratch bytes of a gv_mil_train call (gv_mil_predict: batch = min(n_bags, 64)); -1 with gv_last_error() set for arguments the
 * call would refuse.  Touches no GPU.                                                                                          */
int64_t gv_mil_workspace_bytes(int32_t batch, int32_t max_bag, int32_t L, int32_t C, int32_t F);

/* ---- slide-level survival probe on frozen features (gipvit/survival.py, csrc/survival.hip): the ABMIL body above with one
 * risk output, trained on Cox's partial likelihood with right-censoring.
 * MODEL: gv_mil_train's at C = 1.  Per bag t_i, g_i, s_i, a, z as above; the bag's RISK is theta = Wc . z + bc.  The packed
 * layout is the MIL one at C = 1: P = (2 L + 1) F + 3 L + 2 values,  VU [2 L, F] | Wc [1, F] | bv [L] | bu [L] | w [L] | bc | bw.
 * STEP LOSS: Cox partial likelihood, Breslow ties.  G = the step's good bags in step order, e_i in {0, 1} (1 = the event was
 * observed, 0 = censored), t_i the time as f32, E = #{i in G : e_i = 1}:
 *     l        = (1/E) sum_{i in G, e_i = 1} [ log sum_{j in G, t_j >= t_i} exp(theta_j) - theta_i ]
 *     dtheta_k = (1/E) [ sum_{i in G, e_i = 1, t_i <= t_k} exp(theta_k - M) / S_i  -  e_k ]
 *     S_i = sum_{j in G, t_j >= t_i} exp(theta_j - M),   M = max_{j in G} theta_j
 * in f32 with expf / logf, the sums over j and over i in step order.  Times are compared exactly as given; equal times are in
 * each other's risk set; a bag listed twice is two tied entries.  A step with E = 0 changes nothing (parameters and moments
 * keep their bits, Adam's step count still advances) and adds nothing to loss_sum.  loss_sum is f32 [2], accumulated (the
 * caller zeroes it): {sum of the event terms log S_i + M - theta_i, E}; the epoch loss is their quotient.
 * THE RISK BIAS bc: l does not depend on bc, so its loss gradient is identically zero, and the step gives it a gradient of
 * EXACTLY zero (not the sum of the dtheta_k, rounding noise that Adam would normalise to +-lr): with wd = 0 bc keeps its bits,
 * with decay it only decays.  bw is treated as the MIL probe treats it.
 * ADAM is gv_mil_train's: the decay is added to the gradient, step k of the call is Adam's step step0 + k + 1, the bias
 * corrections are computed on the host in double, lr lr_scale is the rate.
 * gv_surv_train performs ceil(n_bags / batch) steps over bags[], all enqueued on the stream.  A step is four launches, every
 * dependency a launch boundary (no grid barrier, no atomics): the MIL gate; a pool launch (a workgroup per bag) that stops at
 * theta_b and z_b and, because dz_b = dtheta_b Wc at C = 1, leaves the unit-gradient ds~_i = a_i (u_i - sum_j a_j u_j), u_i =
 * Wc . x_i, and dbw~ = sum_i ds~_i; the Cox launch (a workgroup per bag: l and dtheta from the step's <= 64 risks, then the
 * bag's ds~ rows and dbw~ scaled by dtheta_b); the MIL update with dl_b = dtheta_b and the gradient of bc forced to zero.  Every
 * sum has an order fixed by the data layout: results are bitwise the same run to run.  Every load is bounds-checked, padding is
 * zero-filled, rows of x that no bag covers are never read.
 * A BAD BAG contributes nothing and is never used as an index: any of gv_mil_train's conditions on geometry, a time that is
 * not finite or is negative, an event flag outside {0, 1}.
 * Limits: gv_mil_train's at C = 1 (F a multiple of 4 in 4..4096, L a multiple of 16 in 16..256, 1 <= batch <= 64, 1 <= max_bag
 * <= 4096, the same alignment rules), workspace of gv_surv_workspace_bytes(batch, max_bag, L, F) bytes. */
typedef struct {
    float*         params;   /* f32 [P], the layout above                                                */
    float*         m;        /* f32 [P] Adam's first moment                                              */
    float*         v;        /* f32 [P] Adam's second moment                                             */
    const float*   x;        /* f32 [N, F], row stride ldx                                               */
    const int32_t* bag_ptr;  /* i32 [n_all_bags + 1]                                                     */
    const float*   time;     /* f32 [n_all_bags]: time to the event or to censoring                      */
    const int32_t* event;    /* i32 [n_all_bags]: 1 = event observed, 0 = censored                       */
    const int32_t* bags;     /* i32 [n_bags]: the visiting order, any multiset of bag indices            */
    float*         loss_sum; /* f32 [2], accumulated: {sum of the event terms, events}                   */
    void*          workspace; int64_t workspace_bytes;
    int64_t ldx;
    int32_t N, F, L, n_all_bags, n_bags, batch, max_bag;
    int32_t step0;           /* Adam steps taken before this call                                        */
    float   lr, lr_scale, wd, beta1, beta2, eps;
} gv_surv_train_args;
int gv_surv_train(const gv_surv_train_args* a, void* stream);
/* risk[j] = theta of bag bags[j] (bags NULL: of bag j) for j < n_bags, 0 for a bad bag (geometry only: no time is read);
 * optionally attn[r] = a_i and score[r] = s_i for every row r of those bags, as gv_mil_predict writes them.  Any n_bags >= 1
 * (groups of 64 bags), workspace of gv_surv_workspace_bytes(min(n_bags, 64), max_bag, L, F) bytes.                            */
typedef struct {
    const float*   params;   /* f32 [P]                                                                  */
    const float*   x;        /* f32 [N, F], row stride ldx                                               */
    const int32_t* bag_ptr;  /* i32 [n_all_bags + 1]                                                     */
    const int32_t* bags;     /* i32 [n_bags]; may be NULL                                                */
    float*         risk;     /* f32 [n_bags]                                                             */
    float*         attn;     /* f32 [N]; may be NULL                                                     */
    float*         score;    /* f32 [N]; may be NULL                                                     */
    void*          workspace; int64_t workspace_bytes;
    int64_t ldx;
    int32_t N, F, L, n_all_bags, n_bags, max_bag;
} gv_surv_predict_args;
int gv_surv_predict(const gv_surv_predict_args* a, void* stream);
/* scratch bytes of a gv_surv_train call (gv_surv_predict: batch = min(n_bags, 64)); -1 with gv_last_error() set for arguments
 * the call would refuse.  Touches no GPU.                                                                                     */
int64_t gv_surv_workspace_bytes(int32_t batch, int32_t max_bag, int32_t L, int32_t F);
/* COHORT EVALUATION over any risk f32 [n], time f32 [n], event i32 [n], 1 <= n <= 65536.  An entry with a non-finite risk, a
 * time that is not finite or is negative, or a flag outside {0, 1} is excluded and counted.  Over the valid entries:
 *   loss[0] = sum_{e_i = 1} [ log S_i + M - theta_i ] IN FP64 (exp / log in double), S_i and M as above.  A row's sum S_i is
 *     taken by one workgroup of 256 threads, thread t adding the entries t, t + 256, .. in order and the 256 partial sums going
 *     through one fixed tree: the order depends on n alone, not on the launch geometry.  The rows' terms are stored and then
 *     added in index order.
 *   CONCORDANCE (Harrell) over ordered pairs (i, j) of valid entries: a pair is COMPARABLE iff e_i = 1 and t_i < t_j (strict),
 *     and then concordant / discordant / tied as theta_i >, <, = theta_j;  C = (concordant + tied / 2) / comparable.  Pairs
 *     with equal times are NOT counted, whichever of the two had the event -- this differs from lifelines' concordance_index,
 *     which counts an equal-time pair when exactly one of the two is an event.
 *   counts int64 [6] = events, comparable, concordant, discordant, tied, excluded: exact integers.
 * Two calls give the same bits.  Workspace (8-byte aligned) of gv_cox_eval_workspace_bytes(n) bytes.                          */
typedef struct {
    const float*   risk;     /* f32 [n]                                                                  */
    const float*   time;     /* f32 [n]                                                                  */
    const int32_t* event;    /* i32 [n]                                                                  */
    double*        loss;     /* f64 [1]: the sum of the event terms                                      */
    int64_t*       counts;   /* i64 [6]: events, comparable, concordant, discordant, tied, excluded      */
    void*          workspace; int64_t workspace_bytes;
    int32_t n;
} gv_cox_eval_args;
int gv_cox_eval(const gv_cox_eval_args* a, void* stream);
int64_t gv_cox_eval_workspace_bytes(int32_t n);

/* ---- DINOv2 loss options (csrc/dinov2_terms.hip): Sinkhorn-Knopp centring of the teacher and the KoLeo regulariser.
 *
 * Sinkhorn-Knopp over the teacher logits T f32 [R, K] (R = G * B local rows), in the log domain: a [K] (= log u) and b [R] start
 * at 0, tau is hyper[GV_HYP_TEACHER_TEMP] when hyper is given (teacher_temp otherwise), shift = max(T / tau) over all ranks' rows;
 * for it = 0 .. n-1:   s_k = sum_r exp(T_rk / tau - shift + a_k + b_r) over all ranks' rows;  a_k -= log(max(s_k, FLT_MIN));
 *                      unless it is the last:  b_r = -log sum_k exp(T_rk / tau - shift + a_k)
 * and sk_center[k] = -tau a_k: gv_dino_loss with sk_center in place of its centre computes softmax((t - c) / tau), which is
 * the Sinkhorn-Knopp assignment (its per-sample normalisation is the softmax's).  One entry point per dependency between rows and
 * columns, so that the caller can all-reduce between them -- 2 n + 1 calls:
 *     gv_sinkhorn_shift    shift[0] = the LOCAL maximum (the caller takes the maximum over the ranks)
 *     gv_sinkhorn_cols     colsum[k] = the LOCAL s_k (the caller adds the ranks' sums); first != 0: a and b are read as 0
 *     gv_sinkhorn_rows     a_k -= log(max(colsum[k], FLT_MIN)) (first != 0: a is read as 0), then b
 *     gv_sinkhorn_finish   the same fold of the last colsum, and sk_center
 * Each call but the last is two kernel launches (partial maxima + their fold; row-sliced partial sums + their combination, one launch
 * when there is a single slice; the fold of a + the rows): 4 n + 1 launches for n iterations, 13 at n = 3.
 * No atomics and every sum in an order fixed by (R, K): bitwise the same run to run.  Every dependency between workgroups is a
 * launch boundary.  expf / logf, 16-byte loads.  Limits: 1 <= R <= 65535, K a positive multiple of 4, teacher_temp > 0; teacher, a,
 * colsum, sk_center and workspace 16-byte aligned; workspace of gv_sinkhorn_workspace_bytes(R, K) bytes.  A refused call
 * returns GV_E_* before any launch.                                                                                          */
typedef struct {
    const float* teacher;    /* f32 [R, K]                                                               */
    float*       shift;      /* f32 [1]                                                                  */
    float*       a;          /* f32 [K]                                                                  */
    float*       b;          /* f32 [R]                                                                  */
    float*       colsum;     /* f32 [K]                                                                  */
    float*       sk_center;  /* f32 [K]; gv_sinkhorn_finish only, may be NULL elsewhere                  */
    void*        workspace; int64_t workspace_bytes;
    const float* hyper;      /* optional device vector (see gv_adamw_ema_args): the teacher temperature  */
    int32_t R, K;
    int32_t first;           /* != 0: a and b hold nothing yet (the first column pass and the fold after it) */
    float   teacher_temp;
} gv_sinkhorn_args;
int gv_sinkhorn_shift(const gv_sinkhorn_args* a, void* stream);
int gv_sinkhorn_cols(const gv_sinkhorn_args* a, void* stream);
int gv_sinkhorn_rows(const gv_sinkhorn_args* a, void* stream);
int gv_sinkhorn_finish(const gv_sinkhorn_args* a, void* stream);
/* scratch bytes of the four calls; -1 with gv_last_error() set for a shape they would refuse.  Touches no GPU. */
int64_t gv_sinkhorn_workspace_bytes(int32_t R, int32_t K);

/* KoLeo (Sablayrolles et al. 2019, as DINOv2 applies it) on the rows x_i of feats [>= G * B, D], 16-bit activations (f32 for the
 * _f32 entry points), crop g = rows g B .. g B + B - 1, computed in f32 with eps = 1e-8:
 *     y_i = x_i / max(||x_i||, eps);  I_i = argmax_{j != i} y_i . y_j within the crop (the lowest index wins a tie)
 *     delta_i = y_i - y_I + eps;  d_i = ||delta_i||;  koleo = sum_g -(1 / B) sum_i log(d_i + eps)
 * gv_koleo_fwd writes koleo[0], nn[i] = I_i (index within the crop) and y, 1 / max(||x||, eps), d into the workspace.
 * gv_koleo_bwd, from that workspace and nn, with I held constant and w_i = 1 / (B d_i (d_i + eps)):
 *     gy_i = -w_i delta_i + sum_{i': I_i' = i} w_i' delta_i';  gx_i = (gy_i - y_i (y_i . gy_i)) / max(||x_i||, eps)
 *     dfeats_i = round(float(dfeats_i) + weight [* loss_scale[0]] * gx_i) in place for the rows [0, G * B); no other row is touched.
 * The backward gathers (row i scans its crop for I_i' == i): no atomics, bitwise the same run to run.
 * Limits: 1 <= G <= 4, 2 <= B <= 1024, D a multiple of 64 up to 768, ld >= D, weight finite and >= 0, workspace 16-byte aligned
 * and of gv_koleo_workspace_bytes(G, B, D) bytes.  A refused call returns GV_E_* before any launch.                          */
typedef struct {
    const void*  feats;      /* [>= G * B, D], row stride ld (forward)                                   */
    void*        dfeats;     /* [>= G * B, D], row stride ld (backward)                                  */
    void*        workspace; int64_t workspace_bytes;
    int32_t*     nn;         /* i32 [G * B]                                                              */
    float*       koleo;      /* f32 [1] (forward)                                                        */
    const float* loss_scale; /* optional DEVICE scalar that multiplies the gradient (fp16 loss scaling)  */
    int64_t ld;
    int32_t G, B, D;
    float   weight;          /* koleo_weight (backward)                                                  */
} gv_koleo_args;
int gv_koleo_fwd(const gv_koleo_args* a, void* stream);
int gv_koleo_bwd(const gv_koleo_args* a, void* stream);
int gv_koleo_fwd_f32(const gv_koleo_args* a, void* stream);
int gv_koleo_bwd_f32(const gv_koleo_args* a, void* stream);
/* scratch bytes of gv_koleo_fwd / _bwd; -1 with gv_last_error() set for a shape they would refuse.  Touches no GPU. */
int64_t gv_koleo_workspace_bytes(int32_t G, int32_t B, int32_t D);

/* ---- iBOT masked-patch term (csrc/ibot.hip; DINOv2's iBOTPatchLoss.forward_masked and the mask token of its student).
 *
 * A ROW TABLE is an int32 device vector of M token rows of a [n_rows, D] token buffer, row = image * N + token (N tokens per
 * image, token 0 the CLS row).  It is device data, so no call can check it: every kernel skips an entry outside [0, n_rows)
 * -- and, in the two mask-token calls, a CLS row -- instead of following it.  The entries must be unique (each call writes a row
 * once per entry, in no order between entries).  Every sum over rows is stored per slice and added in slice order by a second
 * launch: no atomics, bitwise the same run to run.  Every refused call returns GV_E_* before any launch.
 *
 * gv_mask_tokens_fwd: x[rows[i], :] = mask_token[:] + pos[rows[i] mod N, :], f32 (one addition: exact to the bit against any
 * other f32 evaluation).  Runs behind the patch-embedding product and gv_cls_rows; no other row of x is touched.
 * gv_mask_tokens_bwd (behind gv_tokens_bwd, which has already added the rows into dpos):
 *     dmask_token[:] (+)= sum_i g[rows[i], :]        64 entries per workgroup in table order, then the workgroups' sums in order
 *     gpatch[image * (N - 1) + token - 1, :] = 0     for every entry: the patch embedding gets nothing from a masked patch
 * Limits: M >= 1, N >= 2, n_rows a multiple of N, D a multiple of 4 (up to 1024 in the backward); x, g, mask_token, pos,
 * dmask_token and workspace 16-byte aligned; workspace of gv_mask_tokens_workspace_bytes(M, D) bytes.                          */
typedef struct {
    float*         x;           /* f32 [n_rows, D]                                                          */
    const float*   mask_token;  /* f32 [D]                                                                  */
    const float*   pos;         /* f32 [N, D]                                                               */
    const int32_t* rows;        /* i32 [M]                                                                  */
    int32_t M, N, D, n_rows;
} gv_mask_tokens_fwd_args;
int gv_mask_tokens_fwd(const gv_mask_tokens_fwd_args* a, void* stream);
typedef struct {
    const float*   g;           /* f32 [n_rows, D]: the gradient of the token buffer                        */
    void*          gpatch;      /* [n_rows / N * (N - 1), D] compact patch rows, as gv_tokens_bwd wrote them */
    float*         dmask_token; /* f32 [D]                                                                  */
    const int32_t* rows;        /* i32 [M]                                                                  */
    float*         workspace; int64_t workspace_bytes;
    int32_t M, N, D, n_rows;
    int32_t accumulate;         /* != 0: dmask_token += the sum                                             */
} gv_mask_tokens_bwd_args;
int gv_mask_tokens_bwd(const gv_mask_tokens_bwd_args* a, void* stream);
int gv_mask_tokens_bwd_f32(const gv_mask_tokens_bwd_args* a, void* stream);   /* gpatch as f32 */
/* scratch bytes of gv_mask_tokens_bwd; -1 with gv_last_error() set for a shape it would refuse.  Touches no GPU. */
int64_t gv_mask_tokens_workspace_bytes(int32_t M, int32_t D);

/* The final norm on a row table is gv_layernorm_fwd / _bwd between a gather and a scatter (the same kernels on the same values:
 * bit-equal to the norm of the rows taken on their own):
 *   gv_rows_gather    out[i, :] = x[rows[i], :] (f32, row stride x_stride; zeros for a skipped entry) and, with scale given,
 *                     scale_out[i] = scale[rows[i]] (the rows' stochastic-depth factors, gv_layernorm_bwd's gb_scale)
 *   gv_rows_scatter   g[rows[i], :] = g_src[i, :] (f32) and, with gb given, gb[rows[i], :] = gb_src[i, :] (16-bit; f32 for _f32):
 *                     the residual gradient and the last block's MLP-half dY at the marked rows; a plain store, the rows are unique
 * Limits: M >= 1, D a positive multiple of 4, strides multiples of 4 and >= D, the f32 buffers 16-byte aligned.               */
typedef struct {
    const float*   x; int64_t x_stride;
    const int32_t* rows;        /* i32 [M]                                                                  */
    float*         out;         /* f32 [M, D]                                                               */
    const float*   scale;       /* optional f32 [n_rows]                                                    */
    float*         scale_out;   /* f32 [M], given exactly when scale is                                     */
    int32_t M, D, n_rows;
} gv_rows_gather_args;
int gv_rows_gather(const gv_rows_gather_args* a, void* stream);
typedef struct {
    const float*   g_src;       /* f32 [M, D]                                                               */
    float*         g; int64_t g_stride;
    const void*    gb_src;      /* optional [M, D]                                                          */
    void*          gb; int64_t gb_stride;   /* given exactly when gb_src is                                 */
    const int32_t* rows;        /* i32 [M]                                                                  */
    int32_t M, D, n_rows;
} gv_rows_scatter_args;
int gv_rows_scatter(const gv_rows_scatter_args* a, void* stream);
int gv_rows_scatter_f32(const gv_rows_scatter_args* a, void* stream);         /* gb_src / gb as f32 */

/* gv_ibot_loss on the head's logits of the M marked rows, student and teacher f32 [M, K] in table order, with the patch centre
 * c [K], the rows' weights w [M] (1 / (n_j J) for a row of image j) and tau_s / tau_t as gv_dino_loss takes them (hyper included):
 *     p_i = softmax((t_i - c) / tau_t);  loss[0] = -sum_i w_i sum_k p_ik log_softmax(s_i / tau_s)_k     (ibot_weight NOT applied)
 *     dstudent[i, :] = w_i (softmax(s_i / tau_s) - p_i) / tau_s * ibot_weight * grad_scale [* loss_scale[0]]   (16-bit; f32 for _f32)
 *     center_sum[k] = sum_i t_ik for k < K (raw logits, every row whatever its weight);  center_sum[K] = (float)M
 * so that one [K + 1] vector carries sums and count through the all-reduce.  A row of weight 0 adds nothing to the loss and gets a
 * gradient row of exact zeros, whatever its logits hold.  Two passes, each reading every logit once (16-byte loads when K is a
 * multiple of 4, 4-byte loads otherwise): row maxima and log-sum-exps; then column tiles x row slices, which write the gradient
 * and store their loss and column-sum partials, added in a fixed order by a last small launch.  grad_scale 0 reads as 1.
 * Limits: 1 <= M, K <= 2^20, temperatures > 0, ibot_weight finite and >= 0; workspace 16-byte aligned and of
 * gv_ibot_loss_workspace_bytes(M, K) bytes; student, teacher, center and center_sum 16-byte aligned when K is a multiple of 4. */
typedef struct {
    const float* student; const float* teacher; const float* center; const float* weight;
    void* dstudent; float* loss; float* center_sum;
    float* workspace; int64_t workspace_bytes;
    int32_t M, K;
    float student_temp, teacher_temp, ibot_weight, grad_scale;
    const float* hyper;      /* optional device vector (see gv_adamw_ema_args): temps                       */
    const float* loss_scale; /* optional DEVICE scalar that multiplies the gradient (fp16 loss scaling)     */
} gv_ibot_loss_args;
int gv_ibot_loss(const gv_ibot_loss_args* a, void* stream);
int gv_ibot_loss_f32(const gv_ibot_loss_args* a, void* stream);
/* scratch bytes of gv_ibot_loss; -1 with gv_last_error() set for a shape it would refuse.  Touches no GPU. */
int64_t gv_ibot_loss_workspace_bytes(int32_t M, int32_t K);

/* center[k] <- m center[k] + (1 - m) center_sum[k] / center_sum[K] for k < K, with the (all-reduced) row count read from the
 * device vector's last slot: no host synchronisation.  A count that is not > 0 leaves the centre unchanged.                   */
typedef struct { float* center; const float* center_sum; int32_t K; float momentum; } gv_patch_center_update_args;
int gv_patch_center_update(const gv_patch_center_update_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIPVIT_H */
