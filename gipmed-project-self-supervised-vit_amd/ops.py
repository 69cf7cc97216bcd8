"""Tensor-level wrappers over the C ABI: pass ``tensor.data_ptr()`` + the current
HIP stream.  PyTorch is plumbing here (device memory, streams); all arithmetic
runs in libgipvit_hip.so.  Every function launches asynchronously."""
from __future__ import annotations

import functools
from typing import Optional, Sequence

import torch

from . import _lib as L

# the 16-bit tensor dtype of this process's library build (_lib.ACT_FORMAT): bfloat16 by default, float16 for the -DGV_ACT_F16
# library (--amp --amp-dtype float16); the name follows the default build
bf16, f32 = (torch.bfloat16 if L.ACT_FORMAT == "bf16" else torch.float16), torch.float32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _sfx(t: torch.Tensor) -> str:
    """Entry-point suffix of the fp32 operand mode: chosen by the dtype of the buffer that is bf16 on the training path."""
    if t.dtype == f32:
        return "_f32"
    if t.dtype != bf16:
        raise TypeError(f"expected a bf16 (training path) or f32 (fp32 parity mode) tensor, got {t.dtype}")
    return ""


def _chk(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype or not t.is_cuda:
        raise TypeError(f"{name}: expected a {dtype} device tensor, got {t.dtype} on {t.device}")


def augment(tiles_u8: torch.Tensor, params: torch.Tensor, stats: torch.Tensor, ztable: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Apply one augmentation record per tile on the device (gv_augment).  params: uint8 device tensor holding n packed
    gv_augment_params records (gipvit.augment packs them); stats: int64 device scratch [n]; ztable: f32 [1024]."""
    _chk(tiles_u8, torch.uint8, "tiles")
    n, H, W, _ = tiles_u8.shape
    assert params.is_cuda and params.dtype == torch.uint8 and params.numel() == n * C_sizeof_augment_params() and stats.numel() >= n
    if out is None:
        out = torch.empty_like(tiles_u8)
    a = L.gv_augment_args(tiles_u8.data_ptr(), out.data_ptr(), params.data_ptr(), stats.data_ptr(), ztable.data_ptr(), n, H, W)
    L.call("gv_augment", a, _stream())
    return out


def C_sizeof_augment_params() -> int:
    import ctypes
    return ctypes.sizeof(L.gv_augment_params)


def _mix_table(mix: torch.Tensor, n_tiles: int, windows) -> int:
    """Pointer of a device mix table: uint8 [n_tiles * sizeof(gv_mix_row)] (gipvit.mixup.MixPlan.table)."""
    import ctypes
    if not (mix.is_cuda and mix.dtype == torch.uint8 and mix.is_contiguous() and mix.numel() == n_tiles * ctypes.sizeof(L.gv_mix_row)):
        raise ValueError(f"mix: expected a contiguous uint8 device tensor of {n_tiles} gv_mix_row records, got {mix.dtype} {tuple(mix.shape)} on {mix.device}")
    if len(windows) != 1:
        raise ValueError("mix: the batch is mixed as a whole -- one crop window only")
    return mix.data_ptr()


def _erase_table(erase, n_tiles: int, windows):
    """(pointer, seed) of ``erase`` = (device erase table: uint8 [n_tiles * sizeof(gv_erase_row)], the step's 32-bit seed) --
    gipvit.erasing.ErasePlan's ``table`` and ``seed``."""
    import ctypes
    tab, seed = erase
    if not (tab.is_cuda and tab.dtype == torch.uint8 and tab.is_contiguous() and tab.numel() == n_tiles * ctypes.sizeof(L.gv_erase_row)):
        raise ValueError(f"erase: expected a contiguous uint8 device tensor of {n_tiles} gv_erase_row records, got {tab.dtype} {tuple(tab.shape)} on {tab.device}")
    if len(windows) != 1:
        raise ValueError("erase: the boxes are in the window's coordinates -- one crop window only")
    if not 0 <= int(seed) < (1 << 32):
        raise ValueError(f"erase: the seed is one 32-bit value, got {seed}")
    return tab.data_ptr(), int(seed)


def patchify(tiles_u8: torch.Tensor, windows: Sequence[Sequence[int]], crop: int, mean, std,
             out: Optional[torch.Tensor] = None, fill: Optional[torch.Tensor] = None, mix: Optional[torch.Tensor] = None, erase=None,
             stain: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tiles_u8 [n_tiles, H, W, 3] u8 NHWC; windows [(y0, x0)] of side ``crop``.
    Returns bf16 patches [(len(windows) * n_tiles) * (crop/16)^2, 768], images crop-major.
    ``mix``: a device mix table (gipvit.mixup) -- the batch is mixed in the same pass (gv_patchify_mix), one window only.
    ``erase``: (device erase table, seed) of a gipvit.erasing.ErasePlan -- random erasing in the same pass, after ``fill`` and
    ``mix`` (gv_patchify_erase), one window only.
    ``stain``: n_tiles packed gv_stain_params records on the device (gipvit.stainnorm) -- each tile's bytes go through its record
    inside the same pass (gv_patchify_stain), ``fill`` after it; not with ``mix`` / ``erase`` (training tables)."""
    _chk(tiles_u8, torch.uint8, "tiles")
    assert tiles_u8.dim() == 4 and tiles_u8.shape[-1] == 3 and tiles_u8.is_contiguous()
    n_tiles, H, W, _ = tiles_u8.shape
    n_img = n_tiles * len(windows)
    P = (crop // 16) ** 2
    if out is None:
        out = torch.empty(n_img * P, 768, dtype=bf16, device=tiles_u8.device)
    a = L.gv_patchify_args()
    a.tiles, a.patches, a.n_img, a.tile_h, a.tile_w = tiles_u8.data_ptr(), out.data_ptr(), n_img, H, W
    a.img_stride, a.n_win, a.crop, a.n_tiles = H * W * 3, len(windows), crop, n_tiles
    for i, (y, x) in enumerate(windows):
        a.win_y[i], a.win_x[i] = int(y), int(x)
    for c in range(3):
        a.mean[c], a.std[c] = float(mean[c]), float(std[c])
    if fill is not None:        # f32 [n_tiles, 8] device: normalised fill boxes (Cutout after Normalize, MeanPixelRegularization)
        assert fill.is_cuda and fill.dtype == f32 and fill.shape == (n_tiles, 8) and fill.is_contiguous()
        a.fill = fill.data_ptr()
    if stain is not None:
        if mix is not None or erase is not None:
            raise ValueError("stain: inference-time normalisation does not combine with the training tables mix / erase")
        L.call("gv_patchify_stain" + _sfx(out), L.gv_patchify_stain_args(a, _stain_table(stain, n_tiles, tiles_u8.device)), _stream())
        return out
    if erase is not None:
        L.call("gv_patchify_erase" + _sfx(out), L.gv_patchify_erase_args(a, None if mix is None else _mix_table(mix, n_tiles, windows),
                                                                         *_erase_table(erase, n_tiles, windows)), _stream())
        return out
    if mix is not None:
        L.call("gv_patchify_mix" + _sfx(out), L.gv_patchify_mix_args(a, _mix_table(mix, n_tiles, windows)), _stream())
        return out
    L.call("gv_patchify" + _sfx(out), a, _stream())
    return out


def patchify_nchw(images_f32: torch.Tensor, windows: Sequence[Sequence[int]], crop: int, out: Optional[torch.Tensor] = None,
                  mix: Optional[torch.Tensor] = None, erase=None) -> torch.Tensor:
    """images_f32 [n_tiles, 3, H, W] f32 NCHW, already normalised (any N / C / H strides, W stride 1); windows [(y0, x0)] of
    side ``crop``.  Returns patches [(len(windows) * n_tiles) * (crop/16)^2, 768] in the build's 16-bit format (the value
    rounded, no mean / std), or exact f32 rows when ``out`` is f32; images crop-major as ``patchify``.
    ``mix``: a device mix table (gipvit.mixup): gv_patchify_nchw_mix, one window only.
    ``erase``: (device erase table, seed) of a gipvit.erasing.ErasePlan: gv_patchify_nchw_erase, after ``mix``, one window only."""
    _chk(images_f32, f32, "images")
    if images_f32.dim() != 4 or images_f32.shape[1] != 3 or images_f32.stride(-1) != 1:
        raise ValueError(f"images: expected float32 [n, 3, H, W] with W stride 1, got shape {tuple(images_f32.shape)} "
                         f"strides {images_f32.stride()}")
    n_tiles, _, H, W = images_f32.shape
    n_img = n_tiles * len(windows)
    P = (crop // 16) ** 2
    if out is None:
        out = torch.empty(n_img * P, 768, dtype=bf16, device=images_f32.device)
    sfx = _sfx(out)
    if out.numel() < n_img * P * 768 or not out.is_contiguous():
        raise ValueError(f"out: need a contiguous buffer of {n_img * P} x 768, got {tuple(out.shape)}")
    a = L.gv_patchify_nchw_args()
    a.images, a.patches, a.n_img, a.n_tiles, a.img_h, a.img_w = images_f32.data_ptr(), out.data_ptr(), n_img, n_tiles, H, W
    a.stride_n, a.stride_c, a.stride_h = images_f32.stride(0), images_f32.stride(1), images_f32.stride(2)
    a.n_win, a.crop = len(windows), crop
    for i, (y, x) in enumerate(windows):
        a.win_y[i], a.win_x[i] = int(y), int(x)
    if erase is not None:
        L.call("gv_patchify_nchw_erase" + sfx, L.gv_patchify_nchw_erase_args(a, None if mix is None else _mix_table(mix, n_tiles, windows),
                                                                             *_erase_table(erase, n_tiles, windows)), _stream())
        return out
    if mix is not None:
        L.call("gv_patchify_nchw_mix" + sfx, L.gv_patchify_nchw_mix_args(a, _mix_table(mix, n_tiles, windows)), _stream())
        return out
    L.call("gv_patchify_nchw" + sfx, a, _stream())
    return out


def crop_resize(tiles_u8: torch.Tensor, boxes: torch.Tensor, out_size: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Random-resized crops on the device: tiles_u8 [n_tiles, H, W, 3] u8, boxes int32 [n, 6] =
    (tile, y0, x0, h, w, flip) on the same device -> u8 [n, out_size, out_size, 3]; see gv_crop_resize."""
    _chk(tiles_u8, torch.uint8, "tiles")
    assert tiles_u8.dim() == 4 and tiles_u8.shape[-1] == 3 and tiles_u8.is_contiguous()
    assert boxes.dtype == torch.int32 and boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.is_contiguous() and boxes.device == tiles_u8.device
    n = boxes.shape[0]
    if out is None:
        out = torch.empty(n, out_size, out_size, 3, dtype=torch.uint8, device=tiles_u8.device)
    a = L.gv_crop_resize_args(tiles_u8.data_ptr(), out.data_ptr(), boxes.data_ptr(), n, tiles_u8.shape[0], tiles_u8.shape[1],
                              tiles_u8.shape[2], out_size)
    L.call("gv_crop_resize", a, _stream())
    return out


_VIEW_PARAMS_BYTES = __import__("ctypes").sizeof(L.gv_view_params)      # one packed gv_view_params record


def crop_augment(tiles_u8: torch.Tensor, boxes: torch.Tensor, params: torch.Tensor, stats: torch.Tensor, out_size: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """DINO views in one pass: the random-resized crop of ``crop_resize`` with each crop's ColorJitter / grayscale / 3x3 blur /
    solarise applied before the single store.  ``params``: uint8 device tensor holding n packed gv_view_params records
    (multicrop.ViewAugmentSampler.pack); ``stats``: int64 device scratch [>= n]; see gv_crop_augment."""
    _chk(tiles_u8, torch.uint8, "tiles")
    assert tiles_u8.dim() == 4 and tiles_u8.shape[-1] == 3 and tiles_u8.is_contiguous()
    assert boxes.dtype == torch.int32 and boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.is_contiguous() and boxes.device == tiles_u8.device
    n = boxes.shape[0]
    assert params.dtype == torch.uint8 and params.numel() == n * _VIEW_PARAMS_BYTES and params.device == tiles_u8.device
    assert stats.dtype == torch.int64 and stats.numel() >= n and stats.device == tiles_u8.device
    if out is None:
        out = torch.empty(n, out_size, out_size, 3, dtype=torch.uint8, device=tiles_u8.device)
    a = L.gv_crop_augment_args(tiles_u8.data_ptr(), out.data_ptr(), boxes.data_ptr(), params.data_ptr(), stats.data_ptr(), n, tiles_u8.shape[0],
                               tiles_u8.shape[1], tiles_u8.shape[2], out_size)
    L.call("gv_crop_augment", a, _stream())
    return out


_STAIN_PARAMS_BYTES = __import__("ctypes").sizeof(L.gv_stain_params)    # one packed gv_stain_params record


def crop_augment_stain(tiles_u8: torch.Tensor, boxes: torch.Tensor, params: torch.Tensor, stains: torch.Tensor, stats: torch.Tensor,
                       out_size: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``crop_augment`` with each crop's H&E stain jitter applied to the resized crop before the view chain, in the same pass.
    ``stains``: uint8 device tensor holding n packed gv_stain_params records (stain.StainJitterSampler.pack); see
    gv_crop_augment_stain."""
    _chk(tiles_u8, torch.uint8, "tiles")
    assert tiles_u8.dim() == 4 and tiles_u8.shape[-1] == 3 and tiles_u8.is_contiguous()
    assert boxes.dtype == torch.int32 and boxes.dim() == 2 and boxes.shape[1] == 6 and boxes.is_contiguous() and boxes.device == tiles_u8.device
    n = boxes.shape[0]
    assert params.dtype == torch.uint8 and params.numel() == n * _VIEW_PARAMS_BYTES and params.device == tiles_u8.device
    assert stains.dtype == torch.uint8 and stains.numel() == n * _STAIN_PARAMS_BYTES and stains.device == tiles_u8.device
    assert stats.dtype == torch.int64 and stats.numel() >= n and stats.device == tiles_u8.device
    if out is None:
        out = torch.empty(n, out_size, out_size, 3, dtype=torch.uint8, device=tiles_u8.device)
    a = L.gv_crop_augment_args(tiles_u8.data_ptr(), out.data_ptr(), boxes.data_ptr(), params.data_ptr(), stats.data_ptr(), n, tiles_u8.shape[0],
                               tiles_u8.shape[1], tiles_u8.shape[2], out_size)
    L.call("gv_crop_augment_stain", L.gv_crop_augment_stain_args(a, stains.data_ptr()), _stream())
    return out


def _stain_table(stain: torch.Tensor, n: int, device) -> int:
    """Pointer of a device table of ``n`` packed gv_stain_params records (uint8)."""
    if not (isinstance(stain, torch.Tensor) and stain.is_cuda and stain.device == device and stain.dtype == torch.uint8 and stain.is_contiguous()
            and stain.numel() == n * _STAIN_PARAMS_BYTES):
        raise ValueError(f"stain: expected a contiguous uint8 device tensor of {n} gv_stain_params records ({n * _STAIN_PARAMS_BYTES} bytes)")
    return stain.data_ptr()


def _stain_tiles(tiles_u8: torch.Tensor):
    """(n, h, w, bytes between tiles) of u8 NHWC tiles whose images are dense (a slice along the first dimension is fine)."""
    _chk(tiles_u8, torch.uint8, "tiles")
    if tiles_u8.dim() != 4 or tiles_u8.shape[-1] != 3 or tiles_u8.shape[0] < 1:
        raise ValueError(f"tiles: expected uint8 [n, h, w, 3], got {tuple(tiles_u8.shape)}")
    n, h, w, _ = tiles_u8.shape
    if tuple(tiles_u8.stride()[1:]) != (3 * w, 3, 1) or (n > 1 and tiles_u8.stride(0) < 3 * h * w):
        raise ValueError(f"tiles: every image must be dense NHWC (strides {tiles_u8.stride()})")
    return n, h, w, (tiles_u8.stride(0) if n > 1 else 3 * h * w)


def _stain_groups(n_pixels: int) -> int:
    """Workgroups (= partials) of the three estimation passes: clamp(ceil(n h w / 256), 1, 512), a function of the shape only."""
    return max(1, min(512, -(-int(n_pixels) // 256)))


def stain_stats(tiles_u8: torch.Tensor, v_max: int):
    """Pass 1 of the Macenko estimate (gv_stain_stats) over tissue pixels (every byte <= ``v_max``) -> (n int64 [1], sums f64 [9] =
    sum od_r, od_g, od_b, then sum od_i od_j for rr, rg, rb, gg, gb, bb), device tensors."""
    n, h, w, stride = _stain_tiles(tiles_u8)
    ws = torch.empty(_stain_groups(n * h * w) * 10, dtype=torch.int64, device=tiles_u8.device)
    out = torch.empty(10, dtype=torch.int64, device=tiles_u8.device)
    L.call("gv_stain_stats", L.gv_stain_stats_args(tiles_u8.data_ptr(), stride, n, h, w, int(v_max), ws.data_ptr(), out.data_ptr()), _stream())
    return out[:1], out[1:].view(torch.float64)


def stain_angle_hist(tiles_u8: torch.Tensor, V, v_max: int, bins: int = 4096) -> torch.Tensor:
    """Pass 2 (gv_stain_angle_hist): histogram of atan2(od . V[:, 1], od . V[:, 0]) over tissue pixels, ``bins`` bins over
    [-pi, pi) -> int64 [bins] on the device.  ``V``: host [3, 2] floats."""
    n, h, w, stride = _stain_tiles(tiles_u8)
    bins = int(bins)
    a = L.gv_stain_angle_hist_args()
    a.tiles, a.img_stride, a.n, a.h, a.w, a.v_max, a.n_bins = tiles_u8.data_ptr(), stride, n, h, w, int(v_max), bins
    for i in range(3):
        for k in range(2):
            a.V[i * 2 + k] = float(V[i][k])
    ws = torch.empty(_stain_groups(n * h * w) * max(bins, 1), dtype=torch.int32, device=tiles_u8.device)
    out = torch.empty(max(bins, 1), dtype=torch.int64, device=tiles_u8.device)
    a.workspace, a.out = ws.data_ptr(), out.data_ptr()
    L.call("gv_stain_angle_hist", a, _stream())
    return out


def stain_conc_hist(tiles_u8: torch.Tensor, pinv, cmax, bins: int = 4096) -> torch.Tensor:
    """Pass 3 (gv_stain_conc_hist): per stain k the histogram of c_k = pinv[k] . od over ALL pixels, ``bins`` bins over
    [0, cmax[k]) -> int64 [2, bins + 1] on the device, the last column the count of c_k < 0.  ``pinv``: host [2, 3]."""
    n, h, w, stride = _stain_tiles(tiles_u8)
    bins = int(bins)
    a = L.gv_stain_conc_hist_args()
    a.tiles, a.img_stride, a.n, a.h, a.w, a.n_bins = tiles_u8.data_ptr(), stride, n, h, w, bins
    for k in range(2):
        a.cmax[k] = float(cmax[k])
        for j in range(3):
            a.pinv[k * 3 + j] = float(pinv[k][j])
    ws = torch.empty(_stain_groups(n * h * w) * 2 * (max(bins, 1) + 1), dtype=torch.int32, device=tiles_u8.device)
    out = torch.empty(2, max(bins, 1) + 1, dtype=torch.int64, device=tiles_u8.device)
    a.workspace, a.out = ws.data_ptr(), out.data_ptr()
    L.call("gv_stain_conc_hist", a, _stream())
    return out


def stain_apply(tiles_u8: torch.Tensor, stains: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """u8 tiles -> u8 tiles through one gv_stain_params record per tile (gv_stain_apply): ``stains`` holds n packed records
    (uint8, device); a tile whose record has on = 0 is copied."""
    n, h, w, stride = _stain_tiles(tiles_u8)
    if out is None:
        out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=tiles_u8.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous() or out.device != tiles_u8.device:
        raise ValueError(f"out: expected a contiguous uint8 [{n}, {h}, {w}, 3] on {tiles_u8.device}")
    L.call("gv_stain_apply", L.gv_stain_apply_args(tiles_u8.data_ptr(), out.data_ptr(), _stain_table(stains, n, tiles_u8.device), stride, n, h, w), _stream())
    return out


def layernorm_fwd(x, gamma, beta, rows: int, D: int, x_stride: Optional[int] = None, eps: float = 1e-6,
                  y=None, mean=None, rstd=None):
    _chk(x, f32, "x")
    dev = x.device
    y = torch.empty(rows, D, dtype=bf16, device=dev) if y is None else y
    mean = torch.empty(rows, dtype=f32, device=dev) if mean is None else mean
    rstd = torch.empty(rows, dtype=f32, device=dev) if rstd is None else rstd
    a = L.gv_layernorm_fwd_args(x.data_ptr(), D if x_stride is None else x_stride, gamma.data_ptr(), beta.data_ptr(),
                                y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, D, eps)
    L.call("gv_layernorm_fwd" + _sfx(y), a, _stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, g, gb, partials, rows: int, D: int, x_stride=None, g_stride=None,
                  gb_stride=None, g_init: bool = False, gb_scale=None):
    """``gb_scale`` f32 [rows]: gb = bf16(g * gb_scale[row]) (stochastic depth of the branch in front of this residual add)."""
    a = L.gv_layernorm_bwd_args(dy.data_ptr(), x.data_ptr(), D if x_stride is None else x_stride, mean.data_ptr(),
                                rstd.data_ptr(), gamma.data_ptr(), g.data_ptr(), D if g_stride is None else g_stride,
                                _p(gb), D if gb_stride is None else gb_stride, partials.data_ptr(), rows, D, int(g_init), _p(gb_scale))
    if gb is not None and gb.dtype != dy.dtype:
        raise TypeError(f"layernorm_bwd: dy is {dy.dtype} but gb is {gb.dtype}")
    L.call("gv_layernorm_bwd" + _sfx(dy), a, _stream())


def colsum_finalize(partials, n_blocks: int, n_which: int, which: int, C: int, out, accumulate: bool):
    a = L.gv_colsum_finalize_args(partials.data_ptr(), n_blocks, n_which, which, C, out.data_ptr(), int(accumulate))
    L.call("gv_colsum_finalize", a, _stream())


def ln_finalize(partials, n_blocks: int, C: int, out0, out1, out2):
    """out_w += column sums of partials[:, w, :] (w = 0, 1, 2); None outputs are skipped."""
    L.call("gv_ln_finalize", L.gv_ln_finalize_args(partials.data_ptr(), n_blocks, C, _p(out0), _p(out1), _p(out2)), _stream())


def colsum(x, rows: int, C: int, workspace, out, accumulate: bool = False, ld: Optional[int] = None):
    a = L.gv_colsum_args(x.data_ptr(), int(x.dtype == f32), C if ld is None else ld, rows, C, workspace.data_ptr(),
                         out.data_ptr(), int(accumulate))
    L.call("gv_colsum", a, _stream())


def linear(A, B, C, M: int, N: int, K: int, *, trans_a=False, trans_b=False, epilogue=0, bias=None, resid=None,
           aux_in=None, aux_out=None, pos=None, P=0, alpha=1.0, lda=None, ldb=None, ldc=None, ldr=None, ld_aux=None,
           colsum_a=None, workspace=None, row_scale=None):
    """C[M,N] = op(A) op(B) (+ epilogue); see include/gipvit.h gv_linear."""
    a = L.gv_linear_args()
    a.A, a.B, a.C, a.M, a.N, a.K = A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K
    a.lda = (M if trans_a else K) if lda is None else lda
    a.ldb = (N if trans_b else K) if ldb is None else ldb
    a.ldc = N if ldc is None else ldc
    a.trans_a, a.trans_b, a.c_is_f32, a.epilogue = int(trans_a), int(trans_b), int(C.dtype == f32), epilogue
    a.bias, a.resid, a.ldr = _p(bias), _p(resid), (N if ldr is None else ldr)
    a.aux_in, a.ld_aux, a.aux_out = _p(aux_in), (N if ld_aux is None else ld_aux), _p(aux_out)
    a.pos, a.P, a.alpha, a.colsum_a, a.row_scale = _p(pos), P, alpha, _p(colsum_a), _p(row_scale)
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if A.dtype == f32:      # fp32 operand mode: A, B, C and the aux buffers are all f32
        for t in (B, C, aux_in, aux_out):
            if t is not None and t.dtype != f32:
                raise TypeError(f"linear: f32 A with a {t.dtype} operand (the fp32 mode is f32 throughout)")
    else:
        for t in (B, aux_in, aux_out):
            if t is not None and t.dtype != bf16:
                raise TypeError(f"linear: bf16 A with a {t.dtype} operand")
    L.call("gv_linear" + _sfx(A), a, _stream())
    return C


def linear_timing(enable: bool):
    """Start (True) / stop (False) HIP-event timing of every GEMM launch inside gv_linear."""
    rc = L.lib.gv_linear_timing(int(enable))
    if rc != 0:
        raise L.GipvitError(f"gv_linear_timing: {rc}")


def linear_timing_read():
    """Rows {kernel, launches, seconds, flops, bytes} per GEMM-class kernel since linear_timing(True)."""
    rows = (L.gv_linear_timing_row * 64)()
    n = L.lib.gv_linear_timing_read(rows, 64)
    if n < 0 or n > 64:
        raise L.GipvitError(f"gv_linear_timing_read: {n}: {L.lib.gv_last_error().decode()}")
    return [{"kernel": r.name.decode(), "launches": r.launches, "seconds": r.seconds, "flops": r.flops, "bytes": r.bytes} for r in rows[:n]]


def linear_ln_fwd(A, W, out, M: int, K: int, *, bias=None, resid=None, gamma=None, beta=None, y=None, mean=None, rstd=None, eps: float = 1e-6,
                  N: int = 384, row_scale=None, lda=None, ldw=None, ldr=None, ldo=None):
    """out = A W^T + bias + resid (f32) and, with gamma, y / mean / rstd = LayerNorm of the new row; see gv_linear_ln_fwd.
    Leading dimensions (elements) default to the compact widths."""
    a = L.gv_linear_ln_fwd_args(A.data_ptr(), W.data_ptr(), M, N, K, K if lda is None else lda, K if ldw is None else ldw, _p(bias), _p(resid),
                                N if ldr is None else ldr, out.data_ptr(), N if ldo is None else ldo,
                                _p(gamma), _p(beta), eps, _p(y), _p(mean), _p(rstd), _p(row_scale))
    L.call("gv_linear_ln_fwd", a, _stream())


def mlp_ln_fwd(A, W1, b1, W2, out, M: int, K: int, hidden: int, *, bias2=None, resid=None, gamma=None, beta=None, y=None, mean=None, rstd=None,
               eps: float = 1e-6, N: int = 384, row_scale=None, lda=None, ldw1=None, ldw2=None, ldr=None, ldo=None):
    """out = resid + row_scale (GELU(A W1^T + b1) W2^T + bias2) (f32) and, with gamma, y / mean / rstd = LayerNorm of the new row, in one
    launch; the hidden activation is not stored (forward-only passes); see gv_mlp_ln_fwd.  Leading dimensions (elements) default to
    the compact widths."""
    a = L.gv_mlp_ln_fwd_args(A.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), _p(bias2), M, N, K, hidden, K if lda is None else lda,
                             K if ldw1 is None else ldw1, hidden if ldw2 is None else ldw2,
                             _p(resid), N if ldr is None else ldr, out.data_ptr(), N if ldo is None else ldo, _p(gamma), _p(beta), eps, _p(y), _p(mean), _p(rstd), _p(row_scale))
    L.call("gv_mlp_ln_fwd", a, _stream())


def linear_ln_bwd(dY, W, x, mean, rstd, gamma, g, gb, partials, M: int, K: int, *, g_init: bool = False, N: int = 384, gb_scale=None,
                  lda=None, ldw=None, ldx=None, ldg=None, ldgb=None) -> int:
    """dXn = dY W (W stored [K, N]) fused with the LayerNorm backward it feeds; returns the number of partial blocks
    written (the n_blocks argument of ln_finalize); see gv_linear_ln_bwd.  Leading dimensions (elements) default to the compact widths."""
    a = L.gv_linear_ln_bwd_args(dY.data_ptr(), W.data_ptr(), M, N, K, K if lda is None else lda, N if ldw is None else ldw, x.data_ptr(),
                                N if ldx is None else ldx, mean.data_ptr(), rstd.data_ptr(),
                                gamma.data_ptr(), g.data_ptr(), N if ldg is None else ldg, _p(gb), N if ldgb is None else ldgb, partials.data_ptr(), partials.shape[0], int(g_init), _p(gb_scale))
    L.call("gv_linear_ln_bwd", a, _stream())
    return L.lib.gv_linear_ln_blocks(M)


def linear_dw_group(problems, K: int, workspace):
    """problems: [(dY [K, M] bf16, X [K, N] bf16, dW [M, N] f32 (accumulated), colsum_dy [M] f32 or None), ...] (at most 4) that
    reduce over the same K token rows -- one split-K launch + one reduce for all of them; see gv_linear_dw_group.  The matrices may be
    2-D views of wider buffers: a matrix's leading dimension is its .stride(0)."""
    a = L.gv_linear_dw_group_args()
    a.n, a.K = len(problems), K
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    for q, (dY, X, dW, cs) in enumerate(problems):
        pr = a.prob[q]
        pr.dY, pr.ldy, pr.X, pr.ldx, pr.dW, pr.ldw = dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0), dW.data_ptr(), dW.stride(0)
        pr.colsum_dy, pr.M, pr.N = _p(cs), dY.shape[1], X.shape[1]
    L.call("gv_linear_dw_group", a, _stream())


def _attention_fwd(name, entry, qkv, n_img, N, H, scale, o, lse, q_limit):
    """attention_fwd / attention_fwd_stream: the same buffers and argument struct through the entry point ``entry``"""
    dev = qkv.device
    o = torch.empty(n_img * N, H * 64, dtype=qkv.dtype, device=dev) if o is None else o
    lse = torch.empty(n_img, H, N, dtype=f32, device=dev) if lse is None else lse
    a = L.gv_attention_fwd_args(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), n_img, N, H, scale, q_limit)
    if o.dtype != qkv.dtype:
        raise TypeError(f"{name}: qkv is {qkv.dtype} but o is {o.dtype}")
    L.call(entry, a, _stream())
    return o, lse


def attention_fwd(qkv, n_img: int, N: int, H: int, scale: float, o=None, lse=None, q_limit: int = 0):
    return _attention_fwd("attention_fwd", "gv_attention_fwd" + _sfx(qkv), qkv, n_img, N, H, scale, o, lse, q_limit)


def attention_fwd_stream(qkv, n_img: int, N: int, H: int, scale: float, o=None, lse=None, q_limit: int = 0):
    """``attention_fwd`` for N up to ``_lib.GV_ATTN_STREAM_MAX_N`` tokens (gv_attention_fwd_stream: K / V streamed through LDS under
    an online softmax).  Forward only and 16-bit only: the fp32 operand mode keeps its ``_lib.GV_ATTN_F32_MAX_N``.  ``q_limit`` > 0:
    whole blocks of ``_lib.GV_ATTN_STREAM_QBLOCK`` query rows that hold a row < q_limit are computed, o / lse behind them are left
    untouched."""
    if qkv.dtype != bf16:
        raise TypeError(f"attention_fwd_stream: qkv must be {bf16}, got {qkv.dtype} (there is no fp32 operand form: that mode stops at "
                        f"N = {L.GV_ATTN_F32_MAX_N})")
    return _attention_fwd("attention_fwd_stream", "gv_attention_fwd_stream", qkv, n_img, N, H, scale, o, lse, q_limit)


def _attention_probs(name, entry, qkv, lse, n_img, N, H, scale, q_rows, p):
    """attention_probs / attention_probs_stream: the same buffers and argument struct through the entry point ``entry``"""
    if p is None:
        p = torch.empty(n_img, H, q_rows, N, dtype=f32, device=qkv.device)
    if p.dtype != f32 or lse.dtype != f32:
        raise TypeError(f"{name}: p and lse must be float32, got {p.dtype} / {lse.dtype}")
    if not p.is_contiguous() or p.numel() != n_img * H * q_rows * N:
        raise ValueError(f"{name}: p must be a contiguous buffer of {n_img} x {H} x {q_rows} x {N}, got {tuple(p.shape)}")
    if qkv.numel() < n_img * N * 3 * H * 64 or lse.numel() < n_img * H * N:
        raise ValueError(f"{name}: qkv / lse are smaller than n_img * N rows")
    a = L.gv_attention_probs_args(qkv.data_ptr(), lse.data_ptr(), p.data_ptr(), n_img, N, H, scale, q_rows)
    L.call(entry, a, _stream())
    return p


def attention_probs(qkv, lse, n_img: int, N: int, H: int, scale: float, q_rows: int, p=None):
    """The softmax matrix of the attention that ``attention_fwd`` computed from the same ``qkv`` and left ``lse`` for:
    f32 [n_img, H, q_rows, N], query rows 0..q_rows-1 of every image (1 = the CLS row; lse must be valid for them); see
    gv_attention_probs.  ``p``: a caller buffer of that many elements (contiguous), written in place."""
    return _attention_probs("attention_probs", "gv_attention_probs" + _sfx(qkv), qkv, lse, n_img, N, H, scale, q_rows, p)


def attention_probs_stream(qkv, lse, n_img: int, N: int, H: int, scale: float, q_rows: int, p=None):
    """``attention_probs`` for N up to ``_lib.GV_ATTN_STREAM_MAX_N`` tokens, on the ``lse`` that ``attention_fwd_stream`` left
    (gv_attention_probs_stream: the sequence is never resident; the same bits as ``attention_probs`` given the same lse).  16-bit
    only: there is no ``_f32`` form, the fp32 operand mode keeps its ``_lib.GV_ATTN_F32_MAX_N``."""
    if qkv.dtype == f32:
        raise ValueError(f"attention_probs_stream: there is no gv_attention_probs_stream_f32 form (the fp32 operand mode stops at "
                         f"N = {L.GV_ATTN_F32_MAX_N}: use attention_probs)")
    if qkv.dtype != bf16:
        raise TypeError(f"attention_probs_stream: qkv must be {bf16}, got {qkv.dtype}")
    return _attention_probs("attention_probs_stream", "gv_attention_probs_stream", qkv, lse, n_img, N, H, scale, q_rows, p)


def _varlen(entry, a, fields, segments, H, scale, q_limit, per_segment, mismatch):
    """attention_fwd_varlen / attention_bwd_varlen.  ``a``: the entry point's argument struct, ``fields``: its buffers {field: tensor},
    qkv first.  f32 operands, or a table past GV_ATTN_MAX_SEG: ``per_segment(row slice, n_img, N, lse)`` for every segment."""
    bufs = list(fields.values())
    rows = 0
    if bufs[0].dtype != bf16 or len(segments) > L.GV_ATTN_MAX_SEG:
        for n_img, N, lse in segments:
            per_segment(slice(rows, rows + n_img * N), n_img, N, lse)
            rows += n_img * N
        return
    if any(t.dtype != bufs[0].dtype for t in bufs):
        raise TypeError(mismatch)
    for k, t in fields.items():
        setattr(a, k, t.data_ptr())
    a.n_seg, a.H, a.scale, a.q_limit = len(segments), H, scale, q_limit
    for i, (n_img, N, lse) in enumerate(segments):
        assert lse.dtype == f32 and lse.numel() >= n_img * H * N
        a.n_img[i], a.N[i], a.lse[i] = n_img, N, lse.data_ptr()
        rows += n_img * N
    assert all(t.shape[0] >= rows and t.is_contiguous() for t in bufs)
    L.call(entry, a, _stream())


def attention_fwd_varlen(qkv, o, segments, H: int, scale: float, q_limit: int = 0):
    """All segments of a token-concatenated row space in one call: ``segments`` = [(n_img, N, lse f32 [n_img, H, N]), ...] in row
    order; qkv [T, 3 H 64], o [T, H 64].  bf16: gv_attention_fwd_varlen (a long + a short segment share ONE launch); the fp32
    operand mode runs one call per segment."""
    _varlen("gv_attention_fwd_varlen", L.gv_attention_fwd_varlen_args(), dict(qkv=qkv, o=o), segments, H, scale, q_limit,
            lambda r, n_img, N, lse: attention_fwd(qkv[r], n_img, N, H, scale, o=o[r], lse=lse, q_limit=q_limit),
            f"attention_fwd_varlen: qkv is {qkv.dtype} but o is {o.dtype}")


def attention_bwd(qkv, o, d_o, lse, n_img: int, N: int, H: int, scale: float, dqkv=None, q_limit: int = 0):
    """``q_limit`` > 0: d_o is zero behind the first q_limit query rows of every image -- those queries are skipped (gv_attention_bwd)."""
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    a = L.gv_attention_bwd_args(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), n_img, N, H, scale, q_limit)
    if not (o.dtype == d_o.dtype == dqkv.dtype == qkv.dtype):
        raise TypeError("attention_bwd: qkv / o / d_o / dqkv must share one dtype")
    L.call("gv_attention_bwd" + _sfx(qkv), a, _stream())
    return dqkv


def attention_bwd_stream(qkv, o, d_o, lse, n_img: int, N: int, H: int, scale: float, dqkv=None, delta=None, q_limit: int = 0):
    """``attention_bwd`` for N up to ``_lib.GV_ATTN_STREAM_MAX_N`` tokens, on the o / lse that ``attention_fwd_stream`` left
    (gv_attention_bwd_stream: a dQ launch over query blocks, then a dK / dV launch over key blocks).  16-bit only.  ``delta``: f32
    scratch of n_img * H * N elements, allocated when none is given.  ``q_limit`` > 0: d_o is zero behind the first q_limit query
    rows; only the whole blocks of ``_lib.GV_ATTN_STREAM_QBLOCK`` query rows that hold a row < q_limit are read, dQ behind them is
    zero."""
    if qkv.dtype != bf16:
        raise TypeError(f"attention_bwd_stream: qkv must be {bf16}, got {qkv.dtype} (there is no fp32 operand form: that mode stops at "
                        f"N = {L.GV_ATTN_F32_MAX_N})")
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    if not (o.dtype == d_o.dtype == dqkv.dtype == qkv.dtype):
        raise TypeError("attention_bwd_stream: qkv / o / d_o / dqkv must share one dtype")
    delta = torch.empty(n_img * H * N, dtype=f32, device=qkv.device) if delta is None else delta
    if delta.dtype != f32 or lse.dtype != f32 or delta.numel() < n_img * H * N:
        raise TypeError(f"attention_bwd_stream: lse and delta must be float32, delta of at least {n_img * H * N} elements")
    a = L.gv_attention_bwd_stream_args(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), delta.data_ptr(),
                                       n_img, N, H, scale, q_limit)
    L.call("gv_attention_bwd_stream", a, _stream())
    return dqkv


def attention_bwd_varlen(qkv, o, d_o, dqkv, segments, H: int, scale: float, q_limit: int = 0):
    """Backward of all segments of a token-concatenated row space in one call: ``segments`` = [(n_img, N, lse), ...] as for
    attention_fwd_varlen; qkv / dqkv [T, 3 H 64], o / d_o [T, H 64].  bf16: gv_attention_bwd_varlen; the fp32 operand mode runs
    one call per segment."""
    _varlen("gv_attention_bwd_varlen", L.gv_attention_bwd_varlen_args(), dict(qkv=qkv, o=o, d_o=d_o, dqkv=dqkv), segments, H, scale, q_limit,
            lambda r, n_img, N, lse: attention_bwd(qkv[r], o[r], d_o[r], lse, n_img, N, H, scale, dqkv=dqkv[r], q_limit=q_limit),
            "attention_bwd_varlen: qkv / o / d_o / dqkv must share one dtype")
    return dqkv


def expand_rows(per_img, row_img, rows, n_rep: int, n_img: int, T: int):
    """rows[r, t] = per_img[r, row_img[t]]: per-image stochastic-depth factors -> one factor per token row (n_rep branches)."""
    L.call("gv_expand_rows", L.gv_expand_rows_args(per_img.data_ptr(), row_img.data_ptr(), rows.data_ptr(), n_rep, n_img, T), _stream())


def cls_rows(x, cls, pos, n_img: int, N: int, D: int):
    L.call("gv_cls_rows", L.gv_cls_rows_args(x.data_ptr(), cls.data_ptr(), pos.data_ptr(), n_img, N, D), _stream())


def tokens_bwd(g, gpatch, dpos, dcls, n_img: int, N: int, D: int, accumulate: bool):
    a = L.gv_tokens_bwd_args(g.data_ptr(), gpatch.data_ptr(), dpos.data_ptr(), _p(dcls), n_img, N, D, int(accumulate))
    L.call("gv_tokens_bwd" + _sfx(gpatch), a, _stream())


def small_matmul(A, B, C, M: int, N: int, K: int, *, sam, sak, sbk, sbn, ldc=None, bias=None, accumulate=False):
    """C[m,n] (+)= sum_k A[m*sam + k*sak] B[k*sbk + n*sbn] (+ bias[n]); element strides."""
    a = L.gv_small_matmul_args(A.data_ptr(), int(A.dtype == bf16), sam, sak, B.data_ptr(), int(B.dtype == bf16), sbk, sbn,
                               C.data_ptr(), int(C.dtype == bf16), N if ldc is None else ldc, _p(bias), M, N, K, int(accumulate))
    L.call("gv_small_matmul", a, _stream())


def l2norm_fwd(x, y, inv_norm, rows: int, C: int):
    L.call("gv_l2norm_fwd" + _sfx(y), L.gv_l2norm_fwd_args(x.data_ptr(), y.data_ptr(), inv_norm.data_ptr(), rows, C), _stream())


def l2norm_bwd(dy, y, inv_norm, dx, rows: int, C: int):
    if dx.dtype != y.dtype:
        raise TypeError(f"l2norm_bwd: y is {y.dtype} but dx is {dx.dtype}")
    L.call("gv_l2norm_bwd" + _sfx(y), L.gv_l2norm_bwd_args(dy.data_ptr(), y.data_ptr(), inv_norm.data_ptr(), dx.data_ptr(), rows, C), _stream())


_KINDS = ("knn", "linprobe", "mil", "surv", "cox_eval")
_workspaces = {k: {} for k in _KINDS}    # kind -> {device -> uint8 scratch of that kind's calls, grown on demand and kept}


def _scratch(kind: str, dev, *dims):
    """The per-device scratch of ``kind`` (one of _KINDS), at least gv_<kind>_workspace_bytes(*dims) bytes."""
    need = getattr(L.lib, f"gv_{kind}_workspace_bytes")(*dims)
    if need < 0:
        raise L.GipvitError(f"gv_{kind}_workspace_bytes: {L.lib.gv_last_error().decode()}")
    kept = _workspaces[kind]
    ws = kept.get(dev)
    if ws is None or ws.numel() < need:
        ws = kept[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


# the names the buffers and their helpers had when every kind kept its own: the same dicts, _scratch with the kind filled in
_knn_workspace, _linprobe_workspace, _mil_workspace, _surv_workspace, _cox_workspace = (_workspaces[k] for k in _KINDS)
_linprobe_scratch, _mil_scratch, _surv_scratch, _cox_scratch = (functools.partial(_scratch, k) for k in _KINDS[1:])


def knn_vote(q, bank, labels, k: int, temp: float, C: int, *, n_split: int = 0, want_topk: bool = False):
    """Weighted k-NN vote (gv_knn_vote): q f32 [Q, D] and bank f32 [Nb, D], rows L2-normalised (row stride free, a multiple of 4;
    unit column stride), labels int32 [Nb] -> votes f32 [Q, C] with votes[q, c] = sum over the k most similar bank rows of
    exp(sim / temp) * [label == c]; with ``want_topk`` also (top_sim f32 [Q, k] non-increasing, top_idx int32 [Q, k]).
    ``n_split``: 0 = the library chooses, > 0 forces that many bank splits (same result)."""
    _chk(q, f32, "q"); _chk(bank, f32, "bank"); _chk(labels, torch.int32, "labels")
    if q.dim() != 2 or bank.dim() != 2 or q.shape[1] != bank.shape[1] or q.stride(1) != 1 or bank.stride(1) != 1:
        raise ValueError(f"knn_vote: expected q [Q, D] and bank [Nb, D] with unit column stride, got {tuple(q.shape)} strides {q.stride()} "
                         f"and {tuple(bank.shape)} strides {bank.stride()}")
    if bank.device != q.device or labels.device != q.device:
        raise TypeError("knn_vote: q, bank and labels must live on one device")
    if labels.dim() != 1 or labels.shape[0] != bank.shape[0] or not labels.is_contiguous():
        raise ValueError(f"knn_vote: labels must be a contiguous int32 [{bank.shape[0]}], got {tuple(labels.shape)}")
    if not temp > 0:
        raise ValueError(f"knn_vote: temp must be > 0 (got {temp})")
    (Q, D), Nb = q.shape, bank.shape[0]
    ws = _scratch("knn", q.device, Q, Nb, k, n_split)
    votes = torch.empty(Q, C, dtype=f32, device=q.device)
    top_sim = torch.empty(Q, k, dtype=f32, device=q.device) if want_topk else None
    top_idx = torch.empty(Q, k, dtype=torch.int32, device=q.device) if want_topk else None
    a = L.gv_knn_vote_args(q.data_ptr(), bank.data_ptr(), labels.data_ptr(), votes.data_ptr(), _p(top_sim), _p(top_idx), ws.data_ptr(), ws.numel(),
                           Q, Nb, D, k, C, n_split, q.stride(0), bank.stride(0), 1.0 / temp)
    L.call("gv_knn_vote", a, _stream())
    return (votes, top_sim, top_idx) if want_topk else votes


def _linprobe_heads(who: str, W, b, x):
    """Shapes of the heads against the features -> (H, C, F)."""
    _chk(W, f32, "W"); _chk(b, f32, "b"); _chk(x, f32, "x")
    if W.dim() != 3 or b.dim() != 2 or tuple(b.shape) != tuple(W.shape[:2]) or not (W.is_contiguous() and b.is_contiguous()):
        raise ValueError(f"{who}: expected contiguous W [H, C, F] and b [H, C], got {tuple(W.shape)} and {tuple(b.shape)}")
    if x.dim() != 2 or x.shape[1] != W.shape[2] or x.stride(1) != 1:
        raise ValueError(f"{who}: expected x [N, {W.shape[2]}] with unit column stride, got {tuple(x.shape)} strides {x.stride()}")
    if W.device != x.device or b.device != x.device:
        raise TypeError(f"{who}: W, b and x must live on one device")
    return tuple(W.shape)


def linprobe_train(W, b, mW, mb, lr, wd, x, labels, rows, loss_sum, batch: int, lr_scale: float = 1.0, momentum: float = 0.9):
    """SGD steps of H linear heads on frozen features (gv_linprobe_train), in place: W / mW f32 [H, C, F], b / mb f32 [H, C],
    lr / wd f32 [H], x f32 [N, F] (row stride free, a multiple of 4), labels int32 [N], rows int32 [n_rows] (the visiting order:
    ceil(n_rows / batch) steps, the last one over the rows that are left), loss_sum f32 [H] (accumulated: sum of -log p[label]).
    The step is torch.optim.SGD(lr[h] * lr_scale, momentum, weight_decay=wd[h]) under a mean cross-entropy loss."""
    H, C, F = _linprobe_heads("linprobe_train", W, b, x)
    for t, shape, nm in ((mW, (H, C, F), "mW"), (mb, (H, C), "mb"), (lr, (H,), "lr"), (wd, (H,), "wd"), (loss_sum, (H,), "loss_sum")):
        _chk(t, f32, nm)
        if tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"linprobe_train: {nm} must be a contiguous f32 {list(shape)} on {x.device}, got {tuple(t.shape)} on {t.device}")
    _chk(labels, torch.int32, "labels"); _chk(rows, torch.int32, "rows")
    if labels.dim() != 1 or labels.shape[0] != x.shape[0] or not labels.is_contiguous() or labels.device != x.device:
        raise ValueError(f"linprobe_train: labels must be a contiguous int32 [{x.shape[0]}] on {x.device}, got {tuple(labels.shape)}")
    if rows.dim() != 1 or not rows.is_contiguous() or rows.device != x.device:
        raise ValueError(f"linprobe_train: rows must be a contiguous int32 vector on {x.device}, got {tuple(rows.shape)}")
    ws = _scratch("linprobe", x.device, batch, H, C, F)
    a = L.gv_linprobe_train_args(W.data_ptr(), b.data_ptr(), mW.data_ptr(), mb.data_ptr(), lr.data_ptr(), wd.data_ptr(), x.data_ptr(),
                                 labels.data_ptr(), rows.data_ptr(), loss_sum.data_ptr(), ws.data_ptr(), ws.numel(), x.stride(0),
                                 x.shape[0], F, H, C, rows.shape[0], batch, lr_scale, momentum)
    L.call("gv_linprobe_train", a, _stream())


def linprobe_predict(W, b, x, labels=None):
    """Softmax of the H heads' logits (gv_linprobe_predict): W f32 [H, C, F], b f32 [H, C], x f32 [Q, F] -> prob f32 [Q, H, C];
    with ``labels`` int32 [Q] also -> (prob, loss f32 [H]), loss[h] = sum over q of -log prob[q, h, labels[q]]."""
    H, C, F = _linprobe_heads("linprobe_predict", W, b, x)
    Q = x.shape[0]
    if labels is not None:
        _chk(labels, torch.int32, "labels")
        if labels.dim() != 1 or labels.shape[0] != Q or not labels.is_contiguous() or labels.device != x.device:
            raise ValueError(f"linprobe_predict: labels must be a contiguous int32 [{Q}] on {x.device}, got {tuple(labels.shape)}")
    ws = _scratch("linprobe", x.device, max(1, min(Q, 4096)), H, C, F)
    prob = torch.empty(Q, H, C, dtype=f32, device=x.device)
    loss = torch.empty(H, dtype=f32, device=x.device) if labels is not None else None
    a = L.gv_linprobe_predict_args(W.data_ptr(), b.data_ptr(), x.data_ptr(), _p(labels), prob.data_ptr(), _p(loss), ws.data_ptr(), ws.numel(),
                                   x.stride(0), Q, F, H, C)
    L.call("gv_linprobe_predict", a, _stream())
    return prob if labels is None else (prob, loss)


def _mil_inputs(who: str, params, x, bag_ptr, labels, bags, Lh: int, C: int):
    """Shapes of the packed parameters against the features and the bag table -> (F, n_all_bags)."""
    _chk(params, f32, "params"); _chk(x, f32, "x"); _chk(bag_ptr, torch.int32, "bag_ptr")
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError(f"{who}: expected x [N, F] with unit column stride, got {tuple(x.shape)} strides {x.stride()}")
    F = x.shape[1]
    P = (2 * Lh + C) * F + 3 * Lh + C + 1
    if params.dim() != 1 or params.shape[0] != P or not params.is_contiguous():
        raise ValueError(f"{who}: params must be a contiguous f32 [{P}] ((2 L + C) F + 3 L + C + 1 with L = {Lh}, C = {C}, F = {F}), got {tuple(params.shape)}")
    if bag_ptr.dim() != 1 or bag_ptr.shape[0] < 2 or not bag_ptr.is_contiguous():
        raise ValueError(f"{who}: bag_ptr must be a contiguous int32 [n_bags + 1], got {tuple(bag_ptr.shape)}")
    n_all = bag_ptr.shape[0] - 1
    for t, nm, n in ((labels, "labels", n_all), (bags, "bags", None)):
        if t is None:
            continue
        _chk(t, torch.int32, nm)
        if t.dim() != 1 or not t.is_contiguous() or (n is not None and t.shape[0] != n) or not t.shape[0]:
            raise ValueError(f"{who}: {nm} must be a contiguous int32 vector{'' if n is None else f' [{n}]'}, got {tuple(t.shape)}")
    for t, nm in ((params, "params"), (bag_ptr, "bag_ptr"), (labels, "labels"), (bags, "bags")):
        if t is not None and t.device != x.device:
            raise TypeError(f"{who}: {nm} must live on {x.device}")
    return F, n_all


def _mil_state(who: str, params, m, v, loss_sum, width: int, dev):
    """The moments against the packed parameters, and the loss_sum row of ``width`` sums."""
    for t, nm, shape in ((m, "m", tuple(params.shape)), (v, "v", tuple(params.shape)), (loss_sum, "loss_sum", (width,))):
        _chk(t, f32, nm)
        if tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: {nm} must be a contiguous f32 {list(shape)} on {dev}, got {tuple(t.shape)} on {t.device}")


def _tile_outputs(out: dict, x, want_attn: bool, want_score: bool):
    """The tail of a predict's dict: attn / score f32 [N] zeros where asked for, after what ``out`` already holds -> (attn, score)."""
    for nm, want in (("attn", want_attn), ("score", want_score)):
        if want:
            out[nm] = torch.zeros(x.shape[0], dtype=f32, device=x.device)
    return out.get("attn"), out.get("score")


def mil_train(params, m, v, x, bag_ptr, labels, bags, loss_sum, hidden: int, num_classes: int, batch: int, max_bag: int, step0: int, lr: float,
              lr_scale: float = 1.0, wd: float = 0.0, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
    """Adam steps of the gated-attention MIL model on frozen features (gv_mil_train), in place: params / m / v f32 [P] packed as
    include/gipvit.h lays them out, x f32 [N, F] (row stride free, a multiple of 4), bag_ptr int32 [n_all + 1] (bag b = rows
    bag_ptr[b] .. bag_ptr[b + 1] - 1), labels int32 [n_all], bags int32 [n_bags] (the visiting order: ceil(n_bags / batch)
    steps), loss_sum f32 [1] (accumulated: the sum of the bag losses).  ``step0``: Adam steps taken before this call."""
    F, n_all = _mil_inputs("mil_train", params, x, bag_ptr, labels, bags, hidden, num_classes)
    if labels is None or bags is None:
        raise ValueError("mil_train: labels and bags are required")
    _mil_state("mil_train", params, m, v, loss_sum, 1, x.device)
    ws = _scratch("mil", x.device, batch, max_bag, hidden, num_classes, F)
    a = L.gv_mil_train_args(params.data_ptr(), m.data_ptr(), v.data_ptr(), x.data_ptr(), bag_ptr.data_ptr(), labels.data_ptr(), bags.data_ptr(),
                            loss_sum.data_ptr(), ws.data_ptr(), ws.numel(), x.stride(0), x.shape[0], F, hidden, num_classes, n_all, bags.shape[0],
                            batch, max_bag, step0, lr, lr_scale, wd, beta1, beta2, eps)
    L.call("gv_mil_train", a, _stream())


def mil_predict(params, x, bag_ptr, hidden: int, num_classes: int, max_bag: int, labels=None, bags=None, want_attn: bool = False,
                want_score: bool = False, loss=None):
    """The model's bag probabilities (gv_mil_predict) -> dict(prob f32 [n_bags, C]; with ``labels`` int32 [n_all] also loss f32
    [1], the sum of -log p[label]; with ``want_attn`` / ``want_score`` attn / score f32 [N]: a_i after and s_i before the bag's
    softmax, zero in rows no predicted bag covers).  ``bags`` int32: the bags to predict, default all in order.  ``loss``: an f32
    [1] from an earlier call, to which this call's sum is added."""
    F, n_all = _mil_inputs("mil_predict", params, x, bag_ptr, labels, bags, hidden, num_classes)
    n_bags = n_all if bags is None else bags.shape[0]
    if loss is not None:
        _chk(loss, f32, "loss")
        if labels is None or tuple(loss.shape) != (1,) or loss.device != x.device:
            raise ValueError("mil_predict: an accumulated loss is an f32 [1] on the features' device and needs labels")
    accumulate = loss is not None
    if labels is not None and loss is None:
        loss = torch.empty(1, dtype=f32, device=x.device)
    ws = _scratch("mil", x.device, max(1, min(n_bags, 64)), max_bag, hidden, num_classes, F)
    prob = torch.empty(n_bags, num_classes, dtype=f32, device=x.device)
    out = dict(prob=prob) if loss is None else dict(prob=prob, loss=loss)
    attn, score = _tile_outputs(out, x, want_attn, want_score)
    a = L.gv_mil_predict_args(params.data_ptr(), x.data_ptr(), bag_ptr.data_ptr(), _p(labels), _p(bags), prob.data_ptr(), _p(loss), _p(attn), _p(score),
                              ws.data_ptr(), ws.numel(), x.stride(0), x.shape[0], F, hidden, num_classes, n_all, n_bags, max_bag, int(accumulate))
    L.call("gv_mil_predict", a, _stream())
    return out


def _surv_table(who: str, time, event, n: int, dev):
    _chk(time, f32, "time"); _chk(event, torch.int32, "event")
    for t, nm in ((time, "time"), (event, "event")):
        if t.dim() != 1 or t.shape[0] != n or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: {nm} must be a contiguous vector [{n}] on {dev}, got {tuple(t.shape)} on {t.device}")


def surv_train(params, m, v, x, bag_ptr, time, event, bags, loss_sum, hidden: int, batch: int, max_bag: int, step0: int, lr: float,
               lr_scale: float = 1.0, wd: float = 0.0, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
    """Adam steps of the gated-attention survival model on frozen features under Cox's partial likelihood (gv_surv_train), in
    place: params / m / v f32 [P] packed as the MIL probe's at C = 1, x f32 [N, F], bag_ptr int32 [n_all + 1], time f32 [n_all],
    event int32 [n_all] (1 = observed, 0 = censored), bags int32 [n_bags] (the visiting order), loss_sum f32 [2] (accumulated:
    the sum of the event terms, the events).  ``step0``: Adam steps taken before this call."""
    F, n_all = _mil_inputs("surv_train", params, x, bag_ptr, None, bags, hidden, 1)
    if time is None or event is None or bags is None:
        raise ValueError("surv_train: time, event and bags are required")
    _surv_table("surv_train", time, event, n_all, x.device)
    _mil_state("surv_train", params, m, v, loss_sum, 2, x.device)
    ws = _scratch("surv", x.device, batch, max_bag, hidden, F)
    a = L.gv_surv_train_args(params.data_ptr(), m.data_ptr(), v.data_ptr(), x.data_ptr(), bag_ptr.data_ptr(), time.data_ptr(), event.data_ptr(),
                             bags.data_ptr(), loss_sum.data_ptr(), ws.data_ptr(), ws.numel(), x.stride(0), x.shape[0], F, hidden, n_all, bags.shape[0],
                             batch, max_bag, step0, lr, lr_scale, wd, beta1, beta2, eps)
    L.call("gv_surv_train", a, _stream())


def surv_predict(params, x, bag_ptr, hidden: int, max_bag: int, bags=None, want_attn: bool = False, want_score: bool = False):
    """The model's bag risks (gv_surv_predict) -> dict(risk f32 [n_bags], 0 for a bad bag; with ``want_attn`` / ``want_score``
    attn / score f32 [N]: a_i after and s_i before the bag's softmax, zero in rows no predicted bag covers)."""
    F, n_all = _mil_inputs("surv_predict", params, x, bag_ptr, None, bags, hidden, 1)
    n_bags = n_all if bags is None else bags.shape[0]
    ws = _scratch("surv", x.device, max(1, min(n_bags, 64)), max_bag, hidden, F)
    out = dict(risk=torch.empty(n_bags, dtype=f32, device=x.device))
    attn, score = _tile_outputs(out, x, want_attn, want_score)
    a = L.gv_surv_predict_args(params.data_ptr(), x.data_ptr(), bag_ptr.data_ptr(), _p(bags), out["risk"].data_ptr(), _p(attn), _p(score),
                               ws.data_ptr(), ws.numel(), x.stride(0), x.shape[0], F, hidden, n_all, n_bags, max_bag)
    L.call("gv_surv_predict", a, _stream())
    return out


def cox_eval(risk, time, event):
    """Cohort evaluation (gv_cox_eval) of risk f32 [n], time f32 [n], event int32 [n] -> (loss f64 [1]: the sum of the event
    terms of Cox's partial likelihood in fp64, counts int64 [6]: events, comparable, concordant, discordant, tied, excluded)."""
    _chk(risk, f32, "risk")
    if risk.dim() != 1 or not risk.shape[0] or not risk.is_contiguous():
        raise ValueError(f"cox_eval: risk must be a contiguous f32 vector, got {tuple(risk.shape)}")
    n = risk.shape[0]
    _surv_table("cox_eval", time, event, n, risk.device)
    ws = _scratch("cox_eval", risk.device, n)
    loss = torch.empty(1, dtype=torch.float64, device=risk.device)
    counts = torch.empty(6, dtype=torch.int64, device=risk.device)
    a = L.gv_cox_eval_args(risk.data_ptr(), time.data_ptr(), event.data_ptr(), loss.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), n)
    L.call("gv_cox_eval", a, _stream())
    return loss, counts


def weightnorm_fwd(v, g, w, rows: int, C: int):
    L.call("gv_weightnorm_fwd" + _sfx(w), L.gv_weightnorm_fwd_args(v.data_ptr(), g.data_ptr(), w.data_ptr(), rows, C), _stream())


def weightnorm_bwd(dw, v, g, dv, dg, rows: int, C: int, accumulate: bool):
    a = L.gv_weightnorm_bwd_args(dw.data_ptr(), v.data_ptr(), g.data_ptr(), dv.data_ptr(), _p(dg), rows, C, int(accumulate))
    L.call("gv_weightnorm_bwd", a, _stream())


def dino_loss(student, teacher, center, dstudent, loss, center_sum, workspace, B: int, V: int, G: int, K: int,
              student_temp: float, teacher_temp: float, grad_scale: float = 1.0, hyper=None, loss_scale=None):
    """``loss_scale``: device f32 scalar (LossScaler.state) that multiplies the gradient -- fp16 loss scaling."""
    a = L.gv_dino_loss_args(student.data_ptr(), teacher.data_ptr(), center.data_ptr(), dstudent.data_ptr(), loss.data_ptr(),
                            center_sum.data_ptr(), workspace.data_ptr(), B, V, G, K, student_temp, teacher_temp, grad_scale, _p(hyper),
                            _p(loss_scale))
    L.call("gv_dino_loss" + _sfx(dstudent), a, _stream())


def center_update(center, center_sum, K: int, momentum: float, inv_rows: float):
    L.call("gv_center_update", L.gv_center_update_args(center.data_ptr(), center_sum.data_ptr(), K, momentum, inv_rows), _stream())


def _sinkhorn(entry: str, teacher, shift, a, b, colsum, workspace, R: int, K: int, teacher_temp: float, hyper, first: bool, sk_center=None):
    args = L.gv_sinkhorn_args(teacher.data_ptr(), shift.data_ptr(), a.data_ptr(), b.data_ptr(), colsum.data_ptr(), _p(sk_center), workspace.data_ptr(),
                              workspace.numel() * workspace.element_size(), _p(hyper), R, K, int(first), teacher_temp)
    L.call(entry, args, _stream())


def sinkhorn_shift(teacher, shift, a, b, colsum, workspace, R: int, K: int, teacher_temp: float, hyper=None):
    """Sinkhorn-Knopp centring of the teacher logits f32 [R, K] (include/gipvit.h), first of its 2 n + 1 calls: shift f32 [1] =
    this rank's largest logit / tau (the caller takes the maximum over the ranks).  a / colsum f32 [K], b f32 [R] and the
    workspace (gv_sinkhorn_workspace_bytes) are the state all four functions share; ``hyper`` carries tau as for dino_loss."""
    _sinkhorn("gv_sinkhorn_shift", teacher, shift, a, b, colsum, workspace, R, K, teacher_temp, hyper, False)


def sinkhorn_cols(teacher, shift, a, b, colsum, workspace, R: int, K: int, teacher_temp: float, hyper=None, first: bool = False):
    """colsum[k] = this rank's sum_r exp(T_rk / tau - shift + a_k + b_r) (the caller adds the ranks' sums); ``first``: a = b = 0."""
    _sinkhorn("gv_sinkhorn_cols", teacher, shift, a, b, colsum, workspace, R, K, teacher_temp, hyper, first)


def sinkhorn_rows(teacher, shift, a, b, colsum, workspace, R: int, K: int, teacher_temp: float, hyper=None, first: bool = False):
    """a_k -= log colsum[k] (``first``: from a = 0), then b_r = -log sum_k exp(T_rk / tau - shift + a_k)."""
    _sinkhorn("gv_sinkhorn_rows", teacher, shift, a, b, colsum, workspace, R, K, teacher_temp, hyper, first)


def sinkhorn_finish(teacher, shift, a, b, colsum, workspace, sk_center, R: int, K: int, teacher_temp: float, hyper=None, first: bool = False):
    """The fold of the last column sums, and sk_center f32 [K] = -tau a: dino_loss's ``center`` under Sinkhorn-Knopp centring."""
    _sinkhorn("gv_sinkhorn_finish", teacher, shift, a, b, colsum, workspace, R, K, teacher_temp, hyper, first, sk_center)


def koleo_fwd(feats, workspace, nn, koleo, G: int, B: int, D: int):
    """KoLeo on rows [0, G * B) of feats [>= G * B, D] (16-bit, or f32 in the fp32 operand mode), per crop of B rows: koleo f32 [1]
    = sum_g L_g, nn int32 [G * B] = every row's nearest neighbour within its crop; y, norms and distances stay in the workspace
    (gv_koleo_workspace_bytes) for koleo_bwd."""
    a = L.gv_koleo_args(feats.data_ptr(), None, workspace.data_ptr(), workspace.numel() * workspace.element_size(), nn.data_ptr(), koleo.data_ptr(),
                        None, feats.stride(0), G, B, D, 0.0)
    L.call("gv_koleo_fwd" + _sfx(feats), a, _stream())


def koleo_bwd(dfeats, workspace, nn, G: int, B: int, D: int, weight: float, loss_scale=None):
    """dfeats[0 : G * B] += weight [* loss_scale] * d koleo / d feats, in place, from the workspace and nn koleo_fwd left."""
    a = L.gv_koleo_args(None, dfeats.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size(), nn.data_ptr(), None,
                        _p(loss_scale), dfeats.stride(0), G, B, D, weight)
    L.call("gv_koleo_bwd" + _sfx(dfeats), a, _stream())


def _row_table(who: str, rows, M: int):
    if rows.dtype != torch.int32 or rows.numel() < M or not rows.is_contiguous() or M < 1:
        raise ValueError(f"{who}: rows must be a contiguous int32 tensor of at least M = {M} >= 1 entries, got {rows.dtype} {tuple(rows.shape)}")


def mask_tokens_fwd(x, mask_token, pos, rows, M: int, N: int, D: int):
    """x[rows[i]] = mask_token + pos[rows[i] mod N] for the first M entries of the int32 row table (iBOT's masked student input);
    x f32 [n_img * N, D] contiguous, behind the patch-embedding product and cls_rows; see gv_mask_tokens_fwd."""
    _row_table("mask_tokens_fwd", rows, M)
    if x.dtype != f32 or not x.is_contiguous() or x.numel() % (N * D) or mask_token.numel() != D or pos.numel() < N * D:
        raise ValueError(f"mask_tokens_fwd: need contiguous f32 x [n_img * {N}, {D}], mask_token [{D}] and pos [{N}, {D}], got {tuple(x.shape)}, "
                         f"{tuple(mask_token.shape)}, {tuple(pos.shape)}")
    a = L.gv_mask_tokens_fwd_args(x.data_ptr(), mask_token.data_ptr(), pos.data_ptr(), rows.data_ptr(), M, N, D, x.numel() // D)
    L.call("gv_mask_tokens_fwd", a, _stream())


def mask_tokens_bwd(g, gpatch, dmask_token, rows, workspace, M: int, N: int, D: int, accumulate: bool):
    """dmask_token (+)= sum_i g[rows[i]] in a fixed order, and the marked rows of the compact patch gradient set to exact zeros;
    behind tokens_bwd (dpos keeps the rows' share).  workspace: f32, gv_mask_tokens_workspace_bytes(M, D); see gv_mask_tokens_bwd."""
    _row_table("mask_tokens_bwd", rows, M)
    n_rows = g.numel() // D
    if g.dtype != f32 or not (g.is_contiguous() and gpatch.is_contiguous()) or n_rows % N or gpatch.numel() < n_rows // N * (N - 1) * D:
        raise ValueError(f"mask_tokens_bwd: need contiguous f32 g [n_img * {N}, {D}] and gpatch [n_img * {N - 1}, {D}], got {tuple(g.shape)}, {tuple(gpatch.shape)}")
    a = L.gv_mask_tokens_bwd_args(g.data_ptr(), gpatch.data_ptr(), dmask_token.data_ptr(), rows.data_ptr(), workspace.data_ptr(),
                                  workspace.numel() * workspace.element_size(), M, N, D, n_rows, int(accumulate))
    L.call("gv_mask_tokens_bwd" + _sfx(gpatch), a, _stream())


def rows_gather(x, rows, out, M: int, D: int, n_rows: int, x_stride: Optional[int] = None, scale=None, scale_out=None):
    """out[i] = x[rows[i]] (f32 [M, D] compact) and, with ``scale`` f32 [n_rows], scale_out[i] = scale[rows[i]]: the front half of
    the final norm on a row table (layernorm_fwd on ``out`` is the norm of those rows); see gv_rows_gather."""
    _row_table("rows_gather", rows, M)
    xs = D if x_stride is None else x_stride
    if x.dtype != f32 or out.dtype != f32 or out.numel() < M * D or x.numel() < (n_rows - 1) * xs + D or (scale is None) != (scale_out is None):
        raise ValueError(f"rows_gather: need f32 x of {n_rows} rows (stride {xs}) and f32 out [{M}, {D}], scale and scale_out together; got "
                         f"{tuple(x.shape)} {x.dtype}, {tuple(out.shape)} {out.dtype}")
    if scale is not None and (scale.dtype != f32 or scale.numel() < n_rows or scale_out.dtype != f32 or scale_out.numel() < M):
        raise ValueError(f"rows_gather: scale f32 [{n_rows}] and scale_out f32 [{M}], got {tuple(scale.shape)} and {tuple(scale_out.shape)}")
    L.call("gv_rows_gather", L.gv_rows_gather_args(x.data_ptr(), xs, rows.data_ptr(), out.data_ptr(), _p(scale), _p(scale_out), M, D, n_rows), _stream())


def rows_scatter(g_src, g, rows, M: int, D: int, n_rows: int, g_stride: Optional[int] = None, gb_src=None, gb=None, gb_stride: Optional[int] = None):
    """g[rows[i]] = g_src[i] (f32) and, when given, gb[rows[i]] = gb_src[i] (the build's 16-bit format, or f32 in the fp32 operand
    mode): the back half of the final norm's backward on a row table; see gv_rows_scatter."""
    _row_table("rows_scatter", rows, M)
    gs, gbs = D if g_stride is None else g_stride, D if gb_stride is None else gb_stride
    if g_src.dtype != f32 or g.dtype != f32 or g_src.numel() < M * D or g.numel() < (n_rows - 1) * gs + D or (gb is None) != (gb_src is None):
        raise ValueError(f"rows_scatter: need f32 g_src [{M}, {D}] and f32 g of {n_rows} rows (stride {gs}), gb and gb_src together")
    if gb is not None and (gb.dtype != gb_src.dtype or gb_src.numel() < M * D or gb.numel() < (n_rows - 1) * gbs + D):
        raise ValueError(f"rows_scatter: gb_src [{M}, {D}] and gb of {n_rows} rows (stride {gbs}) in one format, got {gb_src.dtype} and {gb.dtype}")
    a = L.gv_rows_scatter_args(g_src.data_ptr(), g.data_ptr(), gs, _p(gb_src), _p(gb), gbs, rows.data_ptr(), M, D, n_rows)
    L.call("gv_rows_scatter" + ("" if gb is None else _sfx(gb)), a, _stream())


def ibot_loss(student, teacher, center, weight, dstudent, loss, center_sum, workspace, M: int, K: int, student_temp: float, teacher_temp: float,
              ibot_weight: float, grad_scale: float = 1.0, hyper=None, loss_scale=None):
    """The iBOT masked-patch term on the first M rows of student / teacher f32 [>= M, K]: loss f32 [1] (unweighted by
    ``ibot_weight``), dstudent [>= M, K] (16-bit, or f32 in the fp32 operand mode) and center_sum f32 [K + 1] = the raw teacher
    column sums with M in the last slot; ``weight`` f32 [M] holds 1 / (n_j J) per row.  See gv_ibot_loss."""
    for t, nm in ((student, "student"), (teacher, "teacher"), (dstudent, "dstudent")):
        if t.numel() < M * K or not t.is_contiguous():
            raise ValueError(f"ibot_loss: {nm} must be contiguous and hold [{M}, {K}], got {tuple(t.shape)}")
    if student.dtype != f32 or teacher.dtype != f32 or weight.dtype != f32 or weight.numel() < M or center.numel() < K or center_sum.numel() < K + 1:
        raise ValueError(f"ibot_loss: need f32 logits, weight [{M}], center [{K}] and center_sum [{K + 1}], got {student.dtype}, {tuple(weight.shape)}, "
                         f"{tuple(center.shape)}, {tuple(center_sum.shape)}")
    a = L.gv_ibot_loss_args(student.data_ptr(), teacher.data_ptr(), center.data_ptr(), weight.data_ptr(), dstudent.data_ptr(), loss.data_ptr(),
                            center_sum.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size(), M, K, student_temp, teacher_temp,
                            ibot_weight, grad_scale, _p(hyper), _p(loss_scale))
    L.call("gv_ibot_loss" + _sfx(dstudent), a, _stream())


def patch_center_update(center, center_sum, K: int, momentum: float):
    """center <- m center + (1 - m) center_sum[:K] / center_sum[K]; the count is read on the device, 0 leaves the centre as it is."""
    if center.numel() < K or center_sum.numel() < K + 1:
        raise ValueError(f"patch_center_update: center [{K}] and center_sum [{K + 1}], got {tuple(center.shape)} and {tuple(center_sum.shape)}")
    L.call("gv_patch_center_update", L.gv_patch_center_update_args(center.data_ptr(), center_sum.data_ptr(), K, momentum), _stream())


def softmax_lsce(logits, target, loss, dlogits, prob, B: int, C: int, smoothing: float, loss_scale=None):
    a = L.gv_softmax_lsce_args(logits.data_ptr(), target.data_ptr(), loss.data_ptr(), dlogits.data_ptr(), _p(prob), B, C, smoothing,
                               _p(loss_scale))
    L.call("gv_softmax_lsce", a, _stream())


def softmax_mix_loss(logits, target, loss, dlogits, prob, B: int, C: int, smoothing: float, kind: str, partner=None, lam=None,
                     threshold: Optional[float] = None, loss_scale=None):
    """softmax -> timm SoftTargetCrossEntropy (``kind`` "soft_ce") or BinaryCrossEntropy ("bce") on the mixup target built
    from ``target`` i64 [B], ``partner`` i32 [B] (None: no mixing) and ``lam`` f32 [B] (None: 1); see gv_softmax_mix_loss."""
    kinds = {"soft_ce": L.MIX_LOSS_SOFT_CE, "bce": L.MIX_LOSS_BCE}
    if kind not in kinds:
        raise ValueError(f"kind {kind!r}: 'soft_ce' or 'bce'")
    for t, dt, nm in ((partner, torch.int32, "partner"), (lam, f32, "lam")):
        if t is not None and (t.dtype != dt or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f"{nm}: expected a contiguous {dt} tensor of {B} elements, got {t.dtype} {tuple(t.shape)}")
    a = L.gv_softmax_mix_loss_args(logits.data_ptr(), target.data_ptr(), _p(partner), _p(lam), loss.data_ptr(), dlogits.data_ptr(), _p(prob),
                                   B, C, smoothing, kinds[kind], int(threshold is not None), 0.0 if threshold is None else float(threshold),
                                   _p(loss_scale))
    L.call("gv_softmax_mix_loss", a, _stream())


def gather_cls(x, y, n_img: int, N: int, D: int):
    L.call("gv_gather_cls", L.gv_gather_cls_args(x.data_ptr(), y.data_ptr(), n_img, N, D), _stream())


def token_mean_fwd(x, pooled, n_img: int, N: int, D: int):
    """pooled[i] = mean of rows 1 .. N-1 of image i of x f32 [n_img * N, D] (the CLS row excluded; global_pool='avg'); see
    gv_token_mean_fwd."""
    _chk(x, f32, "x"); _chk(pooled, f32, "pooled")
    if x.numel() < n_img * N * D or pooled.numel() < n_img * D or not (x.is_contiguous() and pooled.is_contiguous()):
        raise ValueError(f"token_mean_fwd: need contiguous x [{n_img * N}, {D}] and pooled [{n_img}, {D}], got {tuple(x.shape)} and {tuple(pooled.shape)}")
    L.call("gv_token_mean_fwd", L.gv_token_mean_fwd_args(x.data_ptr(), pooled.data_ptr(), n_img, N, D), _stream())
    return pooled


def token_mean_bwd(dpool, g, gb, n_img: int, N: int, D: int, gb_scale=None):
    """The backward of ``token_mean_fwd`` into the residual gradient: rows t >= 1 of image i get g = dpool[i] / (N - 1) (f32) and
    gb = g * gb_scale[i] in gb's format (the build's 16-bit one, or f32 in the fp32 operand mode); row 0 is zeros in both; see
    gv_token_mean_bwd."""
    _chk(dpool, f32, "dpool"); _chk(g, f32, "g")
    if gb_scale is not None:
        _chk(gb_scale, f32, "gb_scale")
        if gb_scale.numel() < n_img or not gb_scale.is_contiguous():
            raise ValueError(f"token_mean_bwd: gb_scale holds one contiguous factor per image ({n_img}), got {tuple(gb_scale.shape)}")
    sfx = _sfx(gb)
    if not gb.is_cuda:
        raise TypeError(f"gb: expected a device tensor, got one on {gb.device}")
    if dpool.numel() < n_img * D or g.numel() < n_img * N * D or gb.numel() < n_img * N * D or not (dpool.is_contiguous() and g.is_contiguous() and gb.is_contiguous()):
        raise ValueError(f"token_mean_bwd: need contiguous dpool [{n_img}, {D}] and g / gb [{n_img * N}, {D}], got {tuple(dpool.shape)}, "
                         f"{tuple(g.shape)}, {tuple(gb.shape)}")
    L.call("gv_token_mean_bwd" + sfx, L.gv_token_mean_bwd_args(dpool.data_ptr(), g.data_ptr(), gb.data_ptr(), _p(gb_scale), n_img, N, D), _stream())


def store_f32(dst, vals):
    """dst[i] = vals[i] (n <= 16) by a stream-ordered kernel whose arguments carry the values."""
    a = L.gv_store_f32_args()
    a.dst, a.n = dst.data_ptr(), len(vals)
    for i, v in enumerate(vals):
        a.vals[i] = float(v)
    L.call("gv_store_f32", a, _stream())


def cast_bf16(src, dst, n: Optional[int] = None):
    L.call("gv_cast_bf16", L.gv_cast_bf16_args(src.data_ptr(), dst.data_ptr(), src.numel() if n is None else n), _stream())


def sumsq(x, workspace, out, accumulate: bool = False, n: Optional[int] = None):
    a = L.gv_sumsq_args(x.data_ptr(), x.numel() if n is None else n, workspace.data_ptr(), out.data_ptr(), int(accumulate))
    L.call("gv_sumsq", a, _stream())


def adamw_ema(p, grad, m, v, p_bf16, teacher, teacher_bf16, n: int, *, lr, beta1, beta2, eps, weight_decay, step: int,
              grad_scale=1.0, clip_norm=0.0, gnorm_sq=None, teacher_momentum=0.0, hyper=None, mode=0, clip_value=0.0, loss_scale=None):
    """``loss_scale``: device f32 scalar S; the gradient is divided by it and a non-finite ``gnorm_sq`` skips the update (GradScaler.step)."""
    a = L.gv_adamw_ema_args(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), _p(p_bf16), _p(teacher), _p(teacher_bf16), n,
                            lr, beta1, beta2, eps, weight_decay, 1.0 - beta1 ** step, 1.0 - beta2 ** step,
                            grad_scale, clip_norm, _p(gnorm_sq), teacher_momentum, _p(hyper), mode, clip_value, _p(loss_scale))
    L.call("gv_adamw_ema", a, _stream())


def range_block_table(ranges, chunk: int = 1 << 12) -> torch.Tensor:
    """Block table of gv_adamw_ema_ranges for ranges = [(lo, hi), ...] (element ranges of the flat buffers, multiples of 4, in
    range-id order): int32 [n_blocks, 3] = (range, lo, hi), rows of at most ``chunk`` elements that never cross a range -- one
    workgroup's work, so a 768-element range and a 1.77 M-element one load the chip alike (as lamb_block_table)."""
    assert chunk > 0 and chunk % 4 == 0
    return lamb_block_table(ranges, chunk)


def adamw_ema_ranges(p, grad, m, v, p_bf16, teacher, teacher_bf16, n: int, blocks, ranges, *, lr, beta1, beta2, eps, weight_decay, step: int,
                     grad_scale=1.0, clip_norm=0.0, gnorm_sq=None, teacher_momentum=0.0, hyper=None, mode=0, clip_value=0.0, loss_scale=None):
    """gv_adamw_ema over a range table in ONE launch: ``blocks`` device int32 [n_blocks, 3] = (range, lo, hi) (range_block_table),
    ``ranges`` device f32 [n_ranges, 2] = (lr_scale, wd_multiplier); range r steps at ``lr * lr_scale[r]`` with weight decay
    ``weight_decay * wd_multiplier[r]``.  Everything else as adamw_ema."""
    if not (blocks.dtype == torch.int32 and blocks.is_contiguous() and blocks.dim() == 2 and blocks.shape[1] == 3):
        raise TypeError("blocks: contiguous int32 [n_blocks, 3]")
    if not (ranges.dtype == f32 and ranges.is_contiguous() and ranges.dim() == 2 and ranges.shape[1] == 2):
        raise TypeError("ranges: contiguous float32 [n_ranges, 2]")
    if blocks.device != p.device or ranges.device != p.device:
        raise TypeError("blocks / ranges must live on the device of the buffers")
    a = L.gv_adamw_ema_ranges_args(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), _p(p_bf16), _p(teacher), _p(teacher_bf16), n,
                                   lr, beta1, beta2, eps, weight_decay, 1.0 - beta1 ** step, 1.0 - beta2 ** step,
                                   grad_scale, clip_norm, _p(gnorm_sq), teacher_momentum, _p(hyper), mode, clip_value, _p(loss_scale),
                                   blocks.data_ptr(), blocks.shape[0], ranges.data_ptr(), ranges.shape[0])
    L.call("gv_adamw_ema_ranges", a, _stream())


class LossScaler:
    """torch.cuda.amp.GradScaler as timm's NativeScaler drives it (reference train.py:585-602, 1061-1070), kept on the device:
    ``state`` = f32 [S, consecutive finite steps, skipped steps, applied steps].  The loss kernels multiply their gradient by S, gv_adamw_ema divides
    it out and skips the update when the gradient's sum of squares is not finite, ``update`` is GradScaler.update().  Nothing comes
    back to the host; ``state_dict`` (checkpoints: timm's 'amp_scaler' entry) synchronises."""

    def __init__(self, device, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000):
        self.state = torch.tensor([init_scale, 0.0, 0.0, 0.0], dtype=f32, device=device)
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval

    @property
    def scale(self):        # what the kernels take: the loss kernels read [0], gv_adamw_ema [0] and [3]
        return self.state

    def update(self, gnorm_sq):
        a = L.gv_loss_scale_update_args(self.state.data_ptr(), gnorm_sq.data_ptr(), self.growth_factor, self.backoff_factor, self.growth_interval)
        L.call("gv_loss_scale_update", a, _stream())

    def state_dict(self):
        s = self.state.tolist()
        return {"scale": s[0], "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(s[1]), "skipped_steps": int(s[2]), "applied_steps": int(s[3])}

    def load_state_dict(self, d):
        self.growth_factor, self.backoff_factor = float(d["growth_factor"]), float(d["backoff_factor"])
        self.growth_interval = int(d["growth_interval"])
        self.state.copy_(torch.tensor([float(d["scale"]), float(d["_growth_tracker"]), float(d.get("skipped_steps", 0)),
                                       float(d.get("applied_steps", 0))], dtype=f32))


def lamb_block_table(tensors, chunk: int = 1 << 16) -> torch.Tensor:
    """Block table of gv_lamb for tensors = [(lo, hi), ...] (element ranges of a flat buffer, multiples of 4, in tensor-id order):
    int32 [n_blocks, 3] = (tensor, lo, hi), slices of at most ``chunk`` elements that never cross a tensor."""
    rows = []
    for t, (lo, hi) in enumerate(tensors):
        assert lo % 4 == 0 and hi % 4 == 0 and hi > lo
        for a in range(lo, hi, chunk):
            rows.append((t, a, min(hi, a + chunk)))
    return torch.tensor(rows, dtype=torch.int32)


def lamb(p, grad, m, v, p_bf16, teacher, teacher_bf16, blocks, stats, gnorm_sq, *, phase: int, lr, beta1, beta2, eps, weight_decay, step: int,
         grad_scale=1.0, clip_norm=0.0, max_grad_norm=1.0, teacher_momentum=0.0, lr_scale=None):
    """One phase of LAMB over the tensors of ``blocks`` (device int32 [n, 3], offsets relative to the buffers passed); see gv_lamb.
    ``lr_scale``: optional device f32 [n_tensors], tensor t steps at ``lr * lr_scale[t]`` (--layer-decay)."""
    assert lr_scale is None or (lr_scale.dtype == f32 and lr_scale.is_contiguous() and lr_scale.device == p.device)
    assert blocks.dtype == torch.int32 and blocks.is_contiguous() and stats.dtype == f32
    a = L.gv_lamb_args(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), _p(p_bf16), _p(teacher), _p(teacher_bf16), blocks.data_ptr(),
                       blocks.shape[0], stats.data_ptr(), lr, beta1, beta2, eps, weight_decay, 1.0 - beta1 ** step, 1.0 - beta2 ** step,
                       grad_scale, clip_norm, max_grad_norm, gnorm_sq.data_ptr(), teacher_momentum, phase, _p(lr_scale))
    L.call("gv_lamb", a, _stream())


def agc_units(tensors) -> torch.Tensor:
    """Unit table of gv_agc for tensors = [(offset, shape), ...]: one unit per index of dim 0 (timm unitwise_norm: the norm over all
    other dims), the whole tensor for 1-D parameters; int32 [n_units, 2] = (offset, length)."""
    rows = []
    for off, shape in tensors:
        n = 1
        for d in shape:
            n *= d
        if len(shape) <= 1:
            rows.append((off, n))
        else:
            per = n // shape[0]
            rows.extend((off + r * per, per) for r in range(shape[0]))
    return torch.tensor(rows, dtype=torch.int32)


def agc(p, grad, units, clip_factor: float, eps: float = 1e-3, grad_scale: float = 1.0):
    """Adaptive gradient clipping in place on ``grad`` (units: device int32 [n, 2] from agc_units); see gv_agc."""
    assert units.dtype == torch.int32 and units.is_contiguous() and units.device == grad.device
    L.call("gv_agc", L.gv_agc_args(p.data_ptr(), grad.data_ptr(), units.data_ptr(), units.shape[0], clip_factor, eps, grad_scale), _stream())


def dropout_threshold(p: float) -> int:
    """keep iff hash >= floor(p * 2^32) (gv_dropout)."""
    return min(int(p * 4294967296.0), 4294967295)


def dropout_site_seed(seed: int, layer: int, site: int) -> int:
    """The seed of one dropout site of one step: murmur3 finaliser of (step seed, layer, site); sites: 0 pos-embed, 1 attn.proj,
    2 MLP activation, 3 mlp.fc2.  (Restated in oracle/vit_oracle.py for the checker.)"""
    h = (seed ^ (0x85EBCA6B * (layer * 8 + site + 1))) & 0xFFFFFFFF
    h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF; h ^= h >> 16
    return h


def dropout(x, seed: int, p: float, n: Optional[int] = None):
    """In place on a contiguous bf16 / f32 tensor: nn.Dropout(p) with the counter-based mask of (seed, element index); see gv_dropout."""
    assert x.is_contiguous() and x.dtype in (bf16, f32)
    a = L.gv_dropout_args(x.data_ptr(), int(x.dtype == f32), x.numel() if n is None else n, seed, dropout_threshold(p), 1.0 / (1.0 - p))
    L.call("gv_dropout", a, _stream())


def dropout_add(t, resid, out, rows: int, cols: int, seed: int, p: float, row_scale=None):
    """out = resid + row_scale * dropout(t) (all f32 [rows, cols]); see gv_dropout_add."""
    assert t.dtype == f32 and resid.dtype == f32 and out.dtype == f32
    a = L.gv_dropout_add_args(t.data_ptr(), resid.data_ptr(), out.data_ptr(), _p(row_scale), rows, cols, seed, dropout_threshold(p), 1.0 / (1.0 - p))
    L.call("gv_dropout_add", a, _stream())
