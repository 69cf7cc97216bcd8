"""Host-side sequencing of the hot path over the C ABI (no autograd, no torch math).

Mirrors, for this path only, what the reference reaches through timm's
``VisionTransformer`` + ``loss.backward()`` + ``optimizer.step()``
(reference train.py:1044-1078) and what the orphaned DINO ViT / DINOHead
bytecode specifies (``vit.pyc@L..``):

  * ``Arena``     -- every parameter of (backbone [+ head]) in ONE flat f32 buffer with
                     matching flat gradient / Adam-moment / bf16 / teacher buffers, so the
                     optimizer + EMA + bf16 refresh is one fused pass and the data-parallel
                     reduction is a few large RCCL calls over contiguous ranges.  Weight-decayed
                     matrices come first, in the order their gradients complete in backward.
  * ``VitGroup``  -- activations of one network pass: the crop groups are ``Segment``s of one
                     token-concatenated row space (multi-crop wrapper, row D1).
  * ``VitRunner`` -- forward / backward of the encoder as explicit launch sequences.
  * ``DinoEngine`` / ``SupervisedEngine`` -- one training step (rows S1, D1-D5, L1, O1).

The critical path is launched on the caller's current stream with static buffers; work that
feeds nothing downstream (teacher forward, weight-gradient GEMMs, LayerNorm-gradient finalize)
goes to one side stream ordered by events.
"""
from __future__ import annotations

import dataclasses
import math
import os
import weakref
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import ops
from .archs import ARCHS  # noqa: F401  (vit.pyc@L275-293; plain data, kept where the driver can read it before the library loads)
from .layer_decay import LayerDecayPlan

bf16, f32 = ops.bf16, torch.float32      # ops.bf16: the 16-bit dtype of the loaded library build (float16 under GIPVIT_ACT_FORMAT=f16)

MEAN_RON = (0.8998, 0.8253, 0.9357)   # transformations.py:106
STD_RON = (0.1125, 0.1751, 0.0787)    # transformations.py:113
PAD = 64                              # arena offsets are multiples of 64 elements


_POISON_POOL: List["weakref.ref"] = []      # the tensors _empty handed out under GIPVIT_POISON=1 (repoison refills the live ones)


def _poison(t: torch.Tensor):
    t.fill_(float("nan") if t.dtype.is_floating_point else 255)


def _empty(shape, dt, device, carried: bool = False):
    """torch.empty, or NaN / 0xFF-poisoned memory when GIPVIT_POISON=1 (debug: any read of a
    buffer before it was written then shows up as NaN in the loss / gradients).  This is scratch: nothing may read it before the
    same step / pass wrote it, and a poisoned one is registered for ``repoison`` (``carried``: it is not -- ``_carried``).
    Float types and uint8 only: all-ones in a wider integer would be a wild index, and index tables are built from their
    values (torch.cat / torch.tensor), never allocated empty."""
    if not (dt.is_floating_point or dt == torch.uint8):
        raise TypeError(f"_empty / _carried: {dt} -- float types and uint8 only (poison in a wider integer would be a wild index)")
    t = torch.empty(shape, dtype=dt, device=device)
    if os.environ.get("GIPVIT_POISON"):
        _poison(t)
        if not carried:
            _POISON_POOL.append(weakref.ref(t))
    return t


def _carried(shape, dt, device):
    """``_empty`` for a buffer that legitimately holds values from one step to the next: poisoned when allocated (a read before
    its FIRST write still shows) and never refilled.  Every call site names who writes it and when."""
    return _empty(shape, dt, device, carried=True)


def repoison() -> int:
    """Refill every live ``_empty`` buffer that was allocated under GIPVIT_POISON=1 (NaN, all-ones for uint8) and return how
    many there were: 0 with poison off.  Called between steps / passes it shows a read of what the PREVIOUS one left behind.
    The fills are queued on the current stream, so the caller synchronises the device first (the last step's side-stream work
    may still be using the buffers)."""
    live = [(r, r()) for r in _POISON_POOL]
    _POISON_POOL[:] = [r for r, t in live if t is not None]
    n = 0
    for _, t in live:
        if t is not None:
            _poison(t)
            n += 1
    return n


def input_form(x, n: Optional[int], hw: Optional[Tuple[int, int]], float_extras: Sequence[Tuple[str, object]] = ()) -> str:
    """The two image forms every engine entry point takes: ``"u8"`` for uint8 NHWC tiles [n, H, W, 3] (ToTensor + Normalize
    fused into gv_patchify, the fast path) or ``"f32"`` for float32 NCHW [n, 3, H, W] already normalised (the reference's
    ``Data``, train.py:1027-1033: gv_patchify_nchw, W stride 1).  Float input must have ``n`` images of ``hw`` = (H, W) (either
    None: not checked; uint8 tiles keep their callers' own checks); ``float_extras``: (name, value) of the arguments that
    belong to the u8 pipeline -- any of them set with float input is a ValueError."""
    u8 = isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] == 3
    fl = isinstance(x, torch.Tensor) and x.dtype == f32 and x.dim() == 4 and x.shape[1] == 3 and x.stride(-1) == 1
    if not (u8 or fl):
        got = f"{x.dtype} {tuple(x.shape)} strides {x.stride()}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise TypeError("images: expected uint8 NHWC tiles [n, H, W, 3] or float32 NCHW [n, 3, H, W] already normalised "
                        f"(W stride 1), got {got}")
    if fl:
        want = (x.shape[0] if n is None else n, 3) + (tuple(x.shape[2:]) if hw is None else tuple(hw))
        if tuple(x.shape) != want:
            raise ValueError(f"images: expected float32 NCHW of shape {want}, got {tuple(x.shape)}")
        for name, v in float_extras:
            if v is not None:
                raise ValueError(f"{name}= works on uint8 tiles (its boxes / crops are u8-pipeline objects): not with float32 NCHW input")
    return "u8" if u8 else "f32"


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


@dataclasses.dataclass(frozen=True)
class EngineSwitches:
    """The engine's runtime switches, read from the environment once, when a runner / engine is built: field ``x`` is
    ``GIPVIT_X`` (a boolean is off at "0").  Every default is the fast path; the others exist for A/B runs (README)."""
    fused_ln: bool = True          # full-row Linear + LayerNorm kernels (csrc/panel.hip) at the ViT-S width
    group_dw: bool = True          # a block's four weight gradients as one launch
    cls_only_last: bool = True     # the last block's projection / MLP on the CLS rows only
    fused_mlp: bool = True         # forward-only passes: the MLP as one launch
    cls_qlimit: bool = True        # under cls_only_last, that block's attention for the CLS queries only
    varlen_attn: bool = True       # the crop lengths of a multi-crop pass in one attention launch
    dw_stream: bool = True         # work that feeds nothing downstream on a side stream
    side_priority: int = 0         # that stream's priority
    teacher_side: bool = True      # the teacher's forward on the side stream, beside the student's
    bucket_mb: int = 25            # size of the gradient all-reduce ranges (dist.reduction_plan)

    @classmethod
    def from_env(cls) -> "EngineSwitches":
        kw = {}
        for f in dataclasses.fields(cls):
            v = os.environ.get("GIPVIT_" + f.name.upper())
            if v is not None:
                kw[f.name] = v != "0" if isinstance(f.default, bool) else int(v)
        return cls(**kw)


class SideStream:
    """Work that feeds nothing downstream, queued on a side stream beside the main stream (the caller's current stream when
    the helper is made) and ordered by events.  ``run(fn)``: the side stream waits for what main has
    queued so far, ``fn()`` is queued there and the event that marks its end is returned; ``join(ev)``: main waits for it
    before it overwrites what ``fn`` still reads; ``then(fn)``: ``fn()`` behind the side stream's own work only (no events).
    With no side stream ``fn`` runs inline and ``run`` returns None.  Events come from ``pool``, a list its owner keeps
    across steps, in the order they are asked for (a step asks for the same ones every time)."""

    def __init__(self, side, pool: list):
        self.main = torch.cuda.current_stream() if side is not None else None
        self.side, self.pool, self.n = side, pool, 0

    def _event(self):
        if self.n == len(self.pool):
            self.pool.append(torch.cuda.Event())
        self.n += 1
        return self.pool[self.n - 1]

    def run(self, fn):
        if self.side is None:
            fn()
            return None
        e0 = self._event(); e0.record(self.main); self.side.wait_event(e0)
        with torch.cuda.stream(self.side):
            fn()
            e1 = self._event(); e1.record(self.side)
        return e1

    def then(self, fn):
        with torch.cuda.stream(self.side):      # (a no-op context without a side stream)
            fn()

    def join(self, ev):
        if ev is not None:
            self.main.wait_event(ev)


# --------------------------------------------------------------------------- #
# parameter inventory (timm / DINO state_dict names)
# --------------------------------------------------------------------------- #
POOLS = ("token", "avg")


def resolve_pool(global_pool: Optional[str]) -> str:
    """The reference's ``--gp`` (train.py:122, handed to create_model at train.py:490) -> "token" | "avg".  None is the model's
    default, "token" (timm treats an unset --gp so).  "" is refused: timm then applies the head to every token and the
    reference's loss breaks on the [B, N, C] logits; "max" / "avgmax" / anything else is not a pooling of timm's ViT."""
    if global_pool is None:
        return "token"
    if global_pool not in POOLS:
        raise ValueError(f"global_pool {global_pool!r}: 'token' (the CLS token, the default) or 'avg' (mean of the patch tokens + fc_norm)"
                         + ("; '' would hand every token to the head (no pooling), which the reference's loss cannot take" if global_pool == "" else ""))
    return global_pool


def vit_param_specs(arch: str, img_size: int, num_classes: int = 0, global_pool: str = "token") -> "OrderedDict[str, Tuple[int, ...]]":
    """``global_pool`` "avg" (timm 0.8 VisionTransformer): the final ``norm`` is Identity and ``fc_norm``, a
    LayerNorm over the mean of the patch tokens, takes its place in the order."""
    a = ARCHS[arch]
    fnorm = "fc_norm." if resolve_pool(global_pool) == "avg" else "norm."
    D, depth = a["embed_dim"], a["depth"]
    P = (img_size // 16) ** 2
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["cls_token"] = (1, 1, D)
    s["pos_embed"] = (1, P + 1, D)
    s["patch_embed.proj.weight"] = (D, 3, 16, 16)
    s["patch_embed.proj.bias"] = (D,)
    for i in range(depth):
        b = f"blocks.{i}."
        s[b + "norm1.weight"] = (D,); s[b + "norm1.bias"] = (D,)
        s[b + "attn.qkv.weight"] = (3 * D, D); s[b + "attn.qkv.bias"] = (3 * D,)
        s[b + "attn.proj.weight"] = (D, D); s[b + "attn.proj.bias"] = (D,)
        s[b + "norm2.weight"] = (D,); s[b + "norm2.bias"] = (D,)
        s[b + "mlp.fc1.weight"] = (4 * D, D); s[b + "mlp.fc1.bias"] = (4 * D,)
        s[b + "mlp.fc2.weight"] = (D, 4 * D); s[b + "mlp.fc2.bias"] = (D,)
    s[fnorm + "weight"] = (D,); s[fnorm + "bias"] = (D,)
    if num_classes > 0:
        s["head.weight"] = (num_classes, D); s["head.bias"] = (num_classes,)
    return s


def dino_head_specs(in_dim: int, out_dim: int, hidden: int = 2048, bottleneck: int = 256):
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()   # vit.pyc@L296-318
    s["mlp.0.weight"] = (hidden, in_dim); s["mlp.0.bias"] = (hidden,)
    s["mlp.2.weight"] = (hidden, hidden); s["mlp.2.bias"] = (hidden,)
    s["mlp.4.weight"] = (bottleneck, hidden); s["mlp.4.bias"] = (bottleneck,)
    s["last_layer.weight_g"] = (out_dim, 1)
    s["last_layer.weight_v"] = (out_dim, bottleneck)
    return s


def no_weight_decay(name: str, shape) -> bool:
    """timm create_optimizer_v2 filter: 1-D, *.bias, pos_embed, cls_token -- and iBOT's mask_token (DINOv2 lists it
    with them)."""
    base = name.split(".", 1)[1] if name.startswith(("backbone.", "head.")) else name
    return len(shape) <= 1 or name.endswith(".bias") or base in ("pos_embed", "cls_token", "mask_token") or name.endswith("weight_g")


class Arena:
    """Flat parameter storage.  ``order`` lists names in arena order."""

    def __init__(self, specs: "OrderedDict[str, Tuple[int, ...]]", device, teacher: bool):
        decay = [n for n, s in specs.items() if not no_weight_decay(n, s)]
        nodecay = [n for n, s in specs.items() if no_weight_decay(n, s)]
        decay.reverse()                      # gradients complete head-first, block 11 .. 0, patch embed last
        self.specs, self.order = specs, decay + nodecay
        self.off: Dict[str, int] = {}
        o = 0
        for n in decay:
            self.off[n] = o
            o += _round_up(math.prod(specs[n]), PAD)
        self.n_decay = o
        for n in nodecay:
            self.off[n] = o
            o += _round_up(math.prod(specs[n]), PAD)
        self.n = o
        z = lambda dt: torch.zeros(self.n, dtype=dt, device=device)
        self.p, self.g, self.m, self.v, self.pb = z(f32), z(f32), z(f32), z(f32), z(bf16)
        self.t, self.tb = (z(f32), z(bf16)) if teacher else (None, None)

    def view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        shape = self.specs[name]
        o = self.off[name]
        return buf[o:o + math.prod(shape)].view(shape)

    def span(self, name: str) -> Tuple[int, int]:
        """[lo, hi) of one parameter in the flat buffers, padding included."""
        return self.off[name], self.off[name] + _round_up(math.prod(self.specs[name]), PAD)

    def load(self, state: Dict[str, torch.Tensor], buf: Optional[torch.Tensor] = None):
        buf = self.p if buf is None else buf
        for n in self.specs:
            self.view(buf, n).copy_(state[n].to(f32))

    def state_dict(self, buf=None, prefix: str = "") -> "OrderedDict[str, torch.Tensor]":
        buf = self.p if buf is None else buf
        return OrderedDict((n[len(prefix):], self.view(buf, n).detach().clone()) for n in self.specs if n.startswith(prefix))


class Weights:
    """Accessor over one weight set of an arena (student or teacher) with a name prefix."""

    def __init__(self, arena: Arena, prefix: str, teacher: bool = False, fp32: bool = False):
        self.a, self.prefix, self.teacher, self.fp32 = arena, prefix, teacher, fp32

    def w(self, name):      # matrix used as a GEMM operand: the bf16 copy (the f32 master itself in the fp32 operand mode)
        if self.fp32:
            return self.f(name)
        return self.a.view(self.a.tb if self.teacher else self.a.pb, self.prefix + name)

    def f(self, name):      # f32 parameter (bias, LN, pos, cls)
        return self.a.view(self.a.t if self.teacher else self.a.p, self.prefix + name)

    def g(self, name):      # f32 gradient
        return self.a.view(self.a.g, self.prefix + name)


# --------------------------------------------------------------------------- #
# bicubic pos-embed resampling as a fixed linear map (vit.pyc@L213-233)
# --------------------------------------------------------------------------- #
def pos_interp_matrix(n_src_side: int, crop: int) -> torch.Tensor:
    """[P_dst, P_src] matrix M with interpolate(pos) = M @ pos, built by pushing the
    identity basis through the exact torch call the reference makes."""
    import torch.nn.functional as F
    Ns = n_src_side * n_src_side
    w0 = crop // 16 + 0.1
    eye = torch.eye(Ns, dtype=torch.float64).reshape(1, n_src_side, n_src_side, Ns).permute(0, 3, 1, 2)
    out = F.interpolate(eye, scale_factor=(w0 / n_src_side, w0 / n_src_side), mode="bicubic")
    side = crop // 16
    assert out.shape[-1] == side and out.shape[-2] == side
    return out.permute(0, 2, 3, 1).reshape(side * side, Ns).to(torch.float32).contiguous()


# --------------------------------------------------------------------------- #
# activations of a crop group: one or more SEGMENTS (crop resolutions) whose tokens are
# concatenated -- every token-wise op (LayerNorm, all GEMMs, dW) then runs ONCE over all rows;
# only attention, patch embedding and the CLS handling run per segment (multi-crop wrapper, row D1)
# --------------------------------------------------------------------------- #
class Segment:
    def __init__(self, arch, n_img, crop, img_size, row0, img0, device, save, depth, H, act=bf16):
        D = ARCHS[arch]["embed_dim"]
        self.n_img, self.crop, self.row0, self.img0 = n_img, crop, row0, img0
        self.P = (crop // 16) ** 2
        self.N = self.P + 1
        self.T = n_img * self.N
        e = lambda shape, dt: _empty(shape, dt, device)
        nb = depth if save else 1
        self.patches = e((n_img * self.P, 768), act)
        self.lse = [e((n_img, H, self.N), f32) for _ in range(nb)]
        self.fstats = [e((n_img,), f32) for _ in range(2)]
        self.pos = None if crop == img_size else e((self.N, D), f32)
        self.interp = None if crop == img_size else pos_interp_matrix(img_size // 16, crop).to(device)
        if save:
            self.gpatch = e((n_img * self.P, D), act)
            self.dpos = e((self.N, D), f32)

    def rows(self, t: torch.Tensor) -> torch.Tensor:
        return t[self.row0:self.row0 + self.T]


class VitGroup:
    def __init__(self, arch: str, segments, img_size: int, device, save: bool, act=bf16, pool: str = "token", stream_bwd: bool = False,
                 stream_maps: bool = False):
        """segments: [(n_img, crop), ...] in feature-row order.  ``act``: element type of the activation / gradient buffers
        that feed GEMMs and attention -- bf16 on the training path, f32 in the fp32 operand mode (csrc/f32path.hip).
        ``pool``: "token" (the feature is the CLS row) or "avg" (the mean of the patch tokens, then fc_norm: every token of the
        last block is computed and differentiated).  ``stream_bwd`` (the engines' ``long_seq``): the backward of a segment past
        GV_ATTN_MAX_N tokens runs gv_attention_bwd_stream instead of being refused (VitRunner.require_trainable).  ``stream_maps``
        (FeatureExtractor's ``long_maps``): the attention maps of such a segment come from gv_attention_probs_stream instead of
        being refused (VitRunner.require_attention_maps)."""
        assert act in (bf16, f32) and pool in POOLS
        self.act, self.pool = act, pool
        self.stream_bwd = bool(stream_bwd)
        self.stream_maps = bool(stream_maps)
        a = ARCHS[arch]
        D, depth, H = a["embed_dim"], a["depth"], a["num_heads"]
        self.save = save
        self.segs: List[Segment] = []
        row0 = img0 = 0
        for n_img, crop in segments:
            sg = Segment(arch, n_img, crop, img_size, row0, img0, device, save, depth, H, act)
            self.segs.append(sg)
            row0 += sg.T
            img0 += n_img
        self.T, self.n_img = row0, img0
        T, nb = self.T, (depth if save else 1)
        e = lambda shape, dt: _empty(shape, dt, device)
        self.x = [e((T, D), f32) for _ in range(2 * depth + 1 if save else 3)]
        self.xn1 = [e((T, D), act) for _ in range(nb)]
        self.xn2 = [e((T, D), act) for _ in range(nb)]
        self.qkv = [e((T, 3 * D), act) for _ in range(nb)]
        self.o = [e((T, D), act) for _ in range(nb)]
        self.hp = [e((T, 4 * D), act) for _ in range(nb)]
        self.h = [e((T, 4 * D), act) for _ in range(nb)]
        self.stats = [[e((T,), f32) for _ in range(4)] for _ in range(nb)]   # mean1, rstd1, mean2, rstd2
        if save:   # backward scratch
            self.g, self.gb, self.gb2 = e((T, D), f32), e((T, D), act), e((T, D), act)
            self.dh = e((T, 4 * D), act)
            self.dxn = e((T, D), act)
            self.dqkv = e((T, 3 * D), act)
            self.do = e((T, D), act)
            # a block's weight gradients are one side-stream item that runs while the NEXT block's dX chain does: the dY
            # buffers alternate between two sets by block parity, so a block's set stays untouched until that item has run
            self.gb3, self.gb4 = e((T, D), act), e((T, D), act)
            self.dh_b, self.dqkv_b = e((T, 4 * D), act), e((T, 3 * D), act)
            # gv_attention_bwd_stream's delta scratch (written, then read, inside each call), sized for the longest long segment
            long = [sg.n_img * H * sg.N for sg in self.segs if sg.N > L.GV_ATTN_MAX_N]
            if self.stream_bwd and long:
                self.delta = e((max(long),), f32)

        if pool == "avg":      # the pooled rows in front of fc_norm (its statistics: the segments' fstats) and their gradient
            self.pooled = e((self.n_img, D), f32)
            if save:
                self.dpool = e((self.n_img, D), f32)
        self.depth, self.device = depth, device
        # CLS-only last block (VitRunner.cls_last): buffers over the n_img CLS rows, allocated on first use (alloc_cls)
        self.c_o = None
        self.D_ = D
        self.prepared = False     # VitRunner.prepare_backward has zeroed this group's backward scratch for the coming backward
        self.dropout, self.tmp = None, None   # --drop: (p, step seed) and the f32 branch-output buffer of the unfused residual adds (set_dropout)
        self.rs = None            # stochastic depth: f32 [depth, 2, T] row factors of the attention / MLP branch (set_drop)
        self.all_tokens = False   # iBOT: patch rows of the last block reach the head, so the CLS-only tail is off (VitRunner._cls_tail)
        self.drop_img = None      # ... and the per-image factors they were expanded from
        self._row_img = None

    def set_drop(self, per_img: Optional[torch.Tensor]):
        """Stochastic depth (timm DropPath, vit.pyc@L66-74) for the next forward / backward of this group: ``per_img`` f32
        [depth, 2, n_img] on the device = keep / (1 - p) per image for each block's attention and MLP branch (images in
        segment order), or None to switch it off.  Expanded to one factor per token row in one launch."""
        self.drop_img = per_img
        if per_img is None:
            self.rs = None
            return
        assert per_img.dtype == f32 and tuple(per_img.shape) == (self.depth, 2, self.n_img), (per_img.shape, (self.depth, 2, self.n_img))
        if self._row_img is None:
            m = torch.cat([sg.img0 + torch.arange(sg.T, dtype=torch.int32) // sg.N for sg in self.segs])
            self._row_img = m.to(self.device)
            self._rs_buf = _carried((self.depth, 2, self.T), f32, self.device)      # written by every set_drop (below), valid until the next one
        ops.expand_rows(per_img.contiguous(), self._row_img, self._rs_buf, self.depth * 2, self.n_img, self.T)
        self.rs = self._rs_buf

    def set_dropout(self, p: float, seed: int):
        """Dropout (--drop, nn.Dropout after the pos-embed add, attn.proj, the MLP activation and mlp.fc2; vit.pyc@L98-131, L235-246) for
        the next forward / backward of this group: probability ``p`` and this step's 32-bit ``seed`` (the masks are counter-based:
        the backward regenerates them), or p = 0 to switch it off.  The step then runs the unfused Linear / LayerNorm kernels."""
        if not p:
            self.dropout = None
            return
        if not 0.0 < p < 1.0:
            raise ValueError(f"dropout probability {p}: need 0 <= p < 1")
        assert self.save, "dropout belongs to a training pass"
        if self.T * 4 * self.x[0].shape[1] >= 1 << 32:
            raise ValueError("dropout: a site has more than 2^32 elements")
        self.dropout = (float(p), int(seed) & 0xFFFFFFFF)
        if self.tmp is None:
            self.tmp = _empty(tuple(self.x[0].shape), f32, self.device)

    def alloc_cls(self):
        """Buffers of the last block's CLS-only tail: n_img rows instead of T (one per crop image, images in segment order)."""
        if self.c_o is not None:
            return
        n, D, act = self.n_img, self.D_, self.act
        e = lambda shape, dt: _empty(shape, dt, self.device)
        self.c_o, self.c_xn2 = e((n, D), act), e((n, D), act)
        self.c_xa, self.c_xb, self.c_xc = e((n, D), f32), e((n, D), f32), e((n, D), f32)
        self.c_h, self.c_hp = e((n, 4 * D), act), e((n, 4 * D), act)
        self.c_stats = [e((n,), f32), e((n,), f32)]                      # mean2, rstd2
        if self.save:
            self.c_g, self.c_gb, self.c_gb_att = e((n, D), f32), e((n, D), act), e((n, D), act)
            self.c_dh, self.c_dxn, self.c_do = e((n, 4 * D), act), e((n, D), act), e((n, D), act)

    def gather_cls(self, src: torch.Tensor, dst: torch.Tensor):
        """dst[image] = src[the image's CLS row] (strided copies, one per segment)."""
        for sg in self.segs:
            dst[sg.img0:sg.img0 + sg.n_img].copy_(sg.rows(src).view(sg.n_img, sg.N, -1)[:, 0])

    def scatter_cls(self, src: torch.Tensor, dst: torch.Tensor):
        """dst[the image's CLS row] = src[image]; the other rows of dst are left as they are."""
        for sg in self.segs:
            sg.rows(dst).view(sg.n_img, sg.N, -1)[:, 0].copy_(src[sg.img0:sg.img0 + sg.n_img])

    def xbuf(self, j):
        return self.x[j] if self.save else self.x[j % 3]

    def slot(self, i):
        return i if self.save else 0


@dataclasses.dataclass
class Capture:
    """Extra outputs of one forward-only pass (``VitRunner.forward(capture=...)``; the reference's get_last_selfattention /
    get_intermediate_layers, vit.pyc@L255-272), written into caller buffers on the pass's stream.  ``attn``: f32 [n_img, H,
    attn_rows, N], the last block's softmax for query rows 0..attn_rows-1 (1 = the CLS row: the pass keeps its CLS-only tail and
    q_limit; more rows run that block's attention for every query).  ``tokens``: n f32 [T, D] buffers, the final norm over every
    token after each of the last n blocks (the CLS-only tail is off for that pass); ``stats``: f32 [2, T] scratch for their
    LayerNorm statistics.  One segment (single-crop groups) only."""
    attn: Optional[torch.Tensor] = None
    attn_rows: int = 1
    tokens: Sequence[torch.Tensor] = ()
    stats: Optional[torch.Tensor] = None


class VitRunner:
    def __init__(self, arch: str, img_size: int, device, fp32: bool = False, sw: Optional[EngineSwitches] = None):
        """``sw``: the switches of the engine that owns this runner (read from the environment when not given)."""
        a = ARCHS[arch]
        self.arch, self.D, self.depth, self.H, self.img_size = arch, a["embed_dim"], a["depth"], a["num_heads"], img_size
        self.fp32 = fp32    # fp32 operand mode: one f32 kernel per op (no fused Linear + LayerNorm, no grouped dW launch)
        self.scale = 64 ** -0.5
        self.sw = sw = EngineSwitches.from_env() if sw is None else sw
        # full-row Linear + LayerNorm kernels (csrc/panel.hip) exist for the ViT-S width; GIPVIT_FUSED_LN=0 keeps the
        # round-1 pair (128x128-tile GEMM + stand-alone LayerNorm pass) for A/B runs
        self.fused = self.D == 384 and not fp32 and sw.fused_ln
        # the four weight-gradient products of a block as ONE split-K launch (gv_linear_dw_group): a quarter of the slab
        # traffic and four times longer k-loops than four launches (ViT-S: 165 us per block at 950 TFLOP/s against
        # 4 x (51 + 7) us).  GIPVIT_GROUP_DW=0 (and the fp32 operand mode) runs the same schedule with four gv_linear
        # launches in the block's side-stream item instead of the one, for A/B runs.
        self.group_dw = not fp32 and sw.group_dw
        # Only the CLS row of the last block's output feeds the head (vit.pyc@L248-253: forward returns x[:, 0]), so that block's
        # attention projection, MLP and residual adds for the other tokens -- and their whole backward except the K / V path --
        # are dead values: the last block runs them on the n_img CLS rows only (same loss and gradients; ~5.7 % fewer FLOPs of a
        # ViT-S DINO step).  GIPVIT_CLS_ONLY_LAST=0 computes every token of every block, as the reference's module + autograd do.
        self.cls_last = sw.cls_only_last
        # forward-only passes (teacher, inference) run the MLP as one launch; GIPVIT_FUSED_MLP=0 keeps fc1 / fc2 apart (A/B runs)
        self.fused_mlp = sw.fused_mlp
        self.partials_ring = [_empty((L.LN_PARTIAL_BLOCKS, 3, self.D), f32, device) for _ in range(3)]
        self.cs_ws = _empty((64 * 4 * self.D,), f32, device)
        self.one = torch.ones(1, dtype=f32, device=device)
        # split-K slabs per stream: the weight gradients' (on the side stream, or inline when there is none) and those of the
        # few-row products of the CLS-only tail queued on the main stream.  gv_linear picks its split count from the size.
        self.ws_side = _empty((L.lib.gv_linear_workspace_bytes() // 4,), f32, device)
        self.ws_main = _empty((16 << 20) // 4, f32, device)
        self.side = None
        if torch.device(device).type == "cuda" and sw.dw_stream:
            self.side = torch.cuda.Stream(device, priority=sw.side_priority)
        self._events: List[torch.cuda.Event] = []

    # ---- forward: tiles -> CLS features written into feats[row_off + seg.img0 ...]
    def forward(self, W: Weights, G: VitGroup, tiles_u8, windows, mean, std, feats, row_off: int = 0, fill=None, on_side: bool = False,
                capture: Optional[Capture] = None, mix: Optional[torch.Tensor] = None, erase=None, masks=None, patch=None, stain=None):
        """windows: one list of (y0, x0) crop origins per segment; tiles_u8: one NHWC u8 tensor for all
        segments, or one per segment (pre-cut crops: each with the single window (0, 0)).  A float32 NCHW source (already
        normalised, engine.input_form) goes through gv_patchify_nchw instead, without mean / std.
        ``fill`` / ``mix`` / ``erase`` / ``masks`` / ``stain``: optional inputs of the first stage (``_embed``).
        ``on_side``: the call is queued on the side stream (the teacher beside the student): its split-K products take that
        stream's scratch.  ``capture``: extra outputs of a forward-only pass (``Capture``); None issues exactly the default launches.
        ``patch``: (MaskPlan, PatchRows) -- the final norm also runs on the plan's rows of the first segment, into
        ``PatchRows.hb.feats`` (gv_rows_gather + gv_layernorm_fwd); the group must have ``all_tokens`` set.  Either None, or a
        plan without a marked patch, issues exactly the default launches."""
        D, T, H = self.D, G.T, self.H
        if (masks is not None or patch is not None) and not G.all_tokens:
            raise ValueError("masks / patch: the group must run its last block on every token (VitGroup.all_tokens)")
        cap = capture
        if cap is not None:
            assert not G.save and len(G.segs) == 1, "capture: forward-only single-crop groups"
        tok0 = self.depth - len(cap.tokens) if cap is not None else self.depth        # first block whose normed tokens are captured
        cls_tail = self._cls_tail(G) and tok0 == self.depth
        all_q = cap is not None and cap.attn is not None and cap.attn_rows > 1
        streams = any(sg.N > L.GV_ATTN_MAX_N for sg in G.segs)       # the fused varlen call holds whole sequences in LDS
        if cap is not None and cap.attn is not None:
            self.require_attention_maps(G)
        E = L
        self._embed(W, G, tiles_u8, windows, mean, std, fill, mix, erase, masks, stain)
        # --drop: counter-based masks at the four nn.Dropout sites (gv_dropout / gv_dropout_add); the residual adds then run unfused
        dp = G.dropout
        dseed = (lambda layer, site: ops.dropout_site_seed(dp[1], layer, site)) if dp else None
        if dp:
            ops.dropout(G.xbuf(0), dseed(0, 0), dp[0], n=T * D)                           # pos_drop
        # D = 384 (ViT-S): proj / fc2 run as full-row products with the residual add AND the LayerNorm that reads the new
        # row next fused into the epilogue (gv_linear_ln_fwd) -- only block 0's norm1 is a stand-alone pass
        fused = self.fused and dp is None

        def norm_args(i, k):
            """Block i's norm1 / norm2 (k = 1 / 2) as the arguments of the launch that writes the row it reads; all None past the last block."""
            if i == self.depth:
                return dict(gamma=None, beta=None, y=None, mean=None, rstd=None)
            n, s = f"blocks.{i}.norm{k}.", G.slot(i)
            return dict(gamma=W.f(n + "weight"), beta=W.f(n + "bias"), y=(G.xn1, G.xn2)[k - 1][s], mean=G.stats[s][2 * k - 2], rstd=G.stats[s][2 * k - 1])

        def residual(i, site, a, name, K, resid, out, row_scale, ln):
            """out = resid + row_scale * dropout(a W^T + bias), the residual add behind block i's ``name`` (attn.proj: dropout site 1,
            mlp.fc2: site 3), then the LayerNorm ``ln`` of the new row (None: it is not computed here)."""
            w, bias = W.w(f"blocks.{i}.{name}.weight"), W.f(f"blocks.{i}.{name}.bias")
            if fused:
                ops.linear_ln_fwd(a, w, out, T, K, bias=bias, resid=resid, row_scale=row_scale, **ln)
                return
            if dp:
                ops.linear(a, w, G.tmp, T, D, K, epilogue=E.EPI_BIAS, bias=bias)
                ops.dropout_add(G.tmp, resid, out, T, D, dseed(i, site), dp[0], row_scale=row_scale)
            else:
                ops.linear(a, w, out, T, D, K, epilogue=E.EPI_BIAS | E.EPI_RESID, bias=bias, resid=resid, row_scale=row_scale)
            if ln is not None:
                ops.layernorm_fwd(out, ln["gamma"], ln["beta"], T, D, y=ln["y"], mean=ln["mean"], rstd=ln["rstd"])

        for i in range(self.depth):
            b, s = f"blocks.{i}.", G.slot(i)
            xa, xb, xc = G.xbuf(2 * i), G.xbuf(2 * i + 1), G.xbuf(2 * i + 2)
            st = G.stats[s]
            rs_a, rs_m = (G.rs[i, 0], G.rs[i, 1]) if G.rs is not None else (None, None)      # stochastic depth of the two branches
            if not fused or i == 0:
                ops.layernorm_fwd(xa, W.f(b + "norm1.weight"), W.f(b + "norm1.bias"), T, D, y=G.xn1[s], mean=st[0], rstd=st[1])
            ops.linear(G.xn1[s], W.w(b + "attn.qkv.weight"), G.qkv[s], T, 3 * D, D, epilogue=E.EPI_BIAS, bias=W.f(b + "attn.qkv.bias"))
            # the last block under the CLS-only tail: only the CLS query's attention output is used (row 0 of every image)
            ql = 1 if (cls_tail and i == self.depth - 1 and self.sw.cls_qlimit and not all_q) else 0
            if len(G.segs) > 1 and self.sw.varlen_attn and not streams:
                # the crop lengths of a multi-crop pass in ONE call (gv_attention_fwd_varlen: the 37-token pairs fill the 197-token
                # launch's half-empty last round); GIPVIT_VARLEN_ATTN=0 keeps one launch per segment for A/B runs
                ops.attention_fwd_varlen(G.qkv[s], G.o[s], [(sg.n_img, sg.N, sg.lse[s]) for sg in G.segs], H, self.scale, q_limit=ql)
            else:
                # a segment past one workgroup's LDS (N > GV_ATTN_MAX_N: tiles above 256 px) streams K / V instead (gv_attention_fwd_stream)
                for sg in G.segs:
                    attn_fwd = ops.attention_fwd_stream if sg.N > L.GV_ATTN_MAX_N else ops.attention_fwd
                    attn_fwd(sg.rows(G.qkv[s]), sg.n_img, sg.N, H, self.scale, o=sg.rows(G.o[s]), lse=sg.lse[s], q_limit=ql)
            if cap is not None and cap.attn is not None and i == self.depth - 1:
                # past GV_ATTN_MAX_N (a ``stream_maps`` group: require_attention_maps) the map comes from the streaming call, on the lse
                # the streaming forward has just left (q_limit = 1 leaves the first GV_ATTN_STREAM_QBLOCK rows: the CLS row is among them)
                sg = G.segs[0]
                attn_probs = ops.attention_probs_stream if sg.N > L.GV_ATTN_MAX_N else ops.attention_probs
                attn_probs(G.qkv[s], sg.lse[s], sg.n_img, sg.N, H, self.scale, cap.attn_rows, p=cap.attn)
            if cls_tail and i == self.depth - 1:
                self._last_block_tail_fwd(W, G, i, xa, on_side)
                break
            residual(i, 1, G.o[s], "attn.proj", D, xa, xb, rs_a, norm_args(i, 2))
            # fused: the launch that ends the block also runs the NEXT block's norm1 on the row it has just written
            ln_next = norm_args(i + 1, 1) if fused else None
            if fused and self.fused_mlp and not G.save:
                # a pass that keeps no activations (the teacher, inference): fc1 -> GELU -> fc2 -> + residual -> the next norm1 in ONE
                # launch (gv_mlp_ln_fwd); the [T, 4 D] activation never reaches HBM
                ops.mlp_ln_fwd(G.xn2[s], W.w(b + "mlp.fc1.weight"), W.f(b + "mlp.fc1.bias"), W.w(b + "mlp.fc2.weight"), xc, T, D, 4 * D,
                               bias2=W.f(b + "mlp.fc2.bias"), resid=xb, row_scale=rs_m, **ln_next)
            else:
                ops.linear(G.xn2[s], W.w(b + "mlp.fc1.weight"), G.h[s], T, 4 * D, D,
                           epilogue=E.EPI_BIAS | E.EPI_GELU | (E.EPI_SAVE_PRE if G.save else 0),   # a forward-only group keeps no pre-activation
                           bias=W.f(b + "mlp.fc1.bias"), aux_out=G.hp[s] if G.save else None)
                if dp:
                    ops.dropout(G.h[s], dseed(i, 2), dp[0], n=T * 4 * D)
                residual(i, 3, G.h[s], "mlp.fc2", 4 * D, xb, xc, rs_m, ln_next)
            if i >= tok0:     # capture: the final norm over every token of this block's output
                ops.layernorm_fwd(xc, W.f("norm.weight"), W.f("norm.bias"), T, D, y=cap.tokens[i - tok0], mean=cap.stats[0], rstd=cap.stats[1])
        self._final_norm(W, G, feats, row_off, cls_tail, patch)

    def _embed(self, W: Weights, G: VitGroup, tiles_u8, windows, mean, std, fill, mix, erase, masks, stain):
        """The first stage of ``forward``, per segment: patchify, the segment's pos embedding, CLS rows, the patch-embedding product
        and iBOT's mask tokens -> the segment's rows of ``G.xbuf(0)``.  Its optional inputs, and what it refuses of them before anything is launched:
        ``fill``: per-tile normalised fill boxes of the augmentation (gipvit.augment: Cutout after Normalize,
        MeanPixelRegularization), f32 [n_tiles, 8].
        ``mix``: a device mix table (gipvit.mixup.MixPlan.table) -- the single-segment, single-window batch is mixed inside the
        patchify pass (gv_patchify_mix / gv_patchify_nchw_mix); None issues exactly the default launches.
        ``erase``: (device erase table, seed) of a gipvit.erasing.ErasePlan -- random erasing in that same pass, after ``fill`` and
        ``mix`` (gv_patchify_erase / gv_patchify_nchw_erase); None issues exactly the default launches.
        ``masks``: a gipvit.masking.MaskPlan over the images of the FIRST segment (iBOT: the student's global crops) -- the marked
        patch embeddings are replaced by ``mask_token`` (+ pos) behind the patch-embedding product (gv_mask_tokens_fwd).
        ``stain``: one packed gv_stain_params record per tile on the device (gipvit.stainnorm: stain normalisation at inference) --
        the uint8 tiles of a forward-only single-segment group go through it inside the patchify pass (gv_patchify_stain); None
        issues exactly the default launches."""
        D, E = self.D, L
        if stain is not None and (G.save or len(G.segs) != 1 or mix is not None or erase is not None):
            raise ValueError("stain: inference only -- a forward-only single-segment group without mix / erase tables (training is never normalised)")
        for name, table in (("mix", mix), ("erase", erase)):
            if table is not None and (len(G.segs) != 1 or len(windows[0]) != 1):
                raise ValueError(f"{name}: the supervised step's one window of one segment only")
        # (these two keywords exist for a step with a plan / a pass with a record only: without one the patchify call is the one it always was)
        okw = {k: v for k, v in (("erase", erase), ("stain", stain)) if v is not None}
        pos_full = W.f("pos_embed").view(-1, D)
        x0 = G.xbuf(0)
        for k, (sg, wins) in enumerate(zip(G.segs, windows)):
            src = tiles_u8[k] if isinstance(tiles_u8, (list, tuple)) else tiles_u8
            if src.dtype == f32:
                if fill is not None:
                    raise ValueError("fill= works on uint8 tiles: not with float32 NCHW input")
                if stain is not None:
                    raise ValueError("stain= works on uint8 tiles: float32 NCHW input is already normalised, its bytes are gone")
                ops.patchify_nchw(src, wins, sg.crop, out=sg.patches, mix=mix, **okw)
            else:
                ops.patchify(src, wins, sg.crop, mean, std, out=sg.patches, fill=fill, mix=mix, **okw)
            if sg.pos is None:
                pos = pos_full
            else:   # interpolate_pos_encoding: row 0 = cls pos, rows 1.. = M @ pos[1:]
                pos = sg.pos
                Ps = pos_full.shape[0] - 1
                ops.small_matmul(self.one, pos_full, pos, 1, D, 1, sam=0, sak=0, sbk=0, sbn=1)
                ops.small_matmul(sg.interp, pos_full[1:], pos[1:], sg.P, D, Ps, sam=Ps, sak=1, sbk=D, sbn=1)
            xs = sg.rows(x0)
            ops.cls_rows(xs, W.f("cls_token").view(-1), pos, sg.n_img, sg.N, D)
            ops.linear(sg.patches, W.w("patch_embed.proj.weight").view(D, 768), xs, sg.n_img * sg.P, D, 768,
                       epilogue=E.EPI_BIAS | E.EPI_POS, bias=W.f("patch_embed.proj.bias"), pos=pos, P=sg.P)
            if masks is not None and k == 0 and masks.M > 0:
                masks_fit(masks, sg)
                ops.mask_tokens_fwd(xs, W.f("mask_token").view(-1), pos, masks.rows, masks.M, sg.N, D)

    def _final_norm(self, W: Weights, G: VitGroup, feats, row_off: int, cls_tail: bool, patch):
        """The last stage of ``forward``: the pooled / CLS-only / strided-CLS final norm of every segment into ``feats``, and iBOT's
        marked rows (``patch``) through the same norm into their own head buffers."""
        D, xl = self.D, G.xbuf(2 * self.depth)
        for sg in G.segs:
            im, r0 = slice(sg.img0, sg.img0 + sg.n_img), row_off + sg.img0
            out = dict(y=feats[r0:r0 + sg.n_img], mean=sg.fstats[0], rstd=sg.fstats[1])
            if G.pool == "avg":     # mean of the patch tokens -> fc_norm (timm global_pool='avg': the final norm is Identity)
                ops.token_mean_fwd(sg.rows(xl), G.pooled[im], sg.n_img, sg.N, D)
                ops.layernorm_fwd(G.pooled[im], W.f("fc_norm.weight"), W.f("fc_norm.bias"), sg.n_img, D, **out)
            elif cls_tail:         # the last block left its output for the CLS rows only, contiguous
                ops.layernorm_fwd(G.c_xc[im], W.f("norm.weight"), W.f("norm.bias"), sg.n_img, D, **out)
            else:
                ops.layernorm_fwd(sg.rows(xl), W.f("norm.weight"), W.f("norm.bias"), sg.n_img, D, x_stride=sg.N * D, **out)
        if patch is not None and patch[0].M > 0:
            # iBOT: the final norm on the marked rows of the first segment, compact and in table order, for the head's second pass
            plan, pr = patch
            sg, M = G.segs[0], plan.M
            masks_fit(plan, sg, pr)
            rs_last = G.rs[self.depth - 1, 1] if (G.rs is not None and G.save) else None
            ops.rows_gather(sg.rows(xl), plan.rows, pr.x, M, D, sg.T, scale=rs_last, scale_out=pr.scale if rs_last is not None else None)
            ops.layernorm_fwd(pr.x, W.f("norm.weight"), W.f("norm.bias"), M, D, y=pr.hb.feats, mean=pr.mean, rstd=pr.rstd)

    @staticmethod
    def require_trainable(G: VitGroup):
        """gv_attention_bwd holds a whole sequence in LDS: a group with a segment past GV_ATTN_MAX_N tokens runs forward only
        (gv_attention_fwd_stream) -- unless it was built with ``stream_bwd`` (the engines' ``long_seq=True``), whose backward streams
        (gv_attention_bwd_stream) up to GV_ATTN_STREAM_MAX_N tokens.  Raised before anything is launched."""
        long = [sg.N for sg in G.segs if sg.N > L.GV_ATTN_MAX_N]
        if long and getattr(G, "stream_bwd", False):
            if max(long) > L.GV_ATTN_STREAM_MAX_N:
                raise ValueError(f"backward: {max(long)} tokens per image is past the {L.GV_ATTN_STREAM_MAX_N}-token limit of the streaming "
                                 f"attention (images up to 512 px at patch 16)")
            return
        if long:
            raise ValueError(f"backward: {long[0]} tokens per image ({G.segs[0].crop if len(G.segs) == 1 else 'multi-crop'} px) is past the "
                             f"{L.GV_ATTN_MAX_N}-token limit of the attention backward (images up to 256 px at patch 16); "
                             f"larger images run forward-only (inference, feature extraction)")

    @staticmethod
    def require_attention_maps(G: VitGroup):
        """gv_attention_probs stops at GV_ATTN_MAX_N tokens, as the kernels it restates -- unless the group was built with
        ``stream_maps`` (FeatureExtractor's ``long_maps=True``), whose maps come from gv_attention_probs_stream up to
        GV_ATTN_STREAM_MAX_N tokens.  Raised before anything is launched."""
        long = [sg.N for sg in G.segs if sg.N > L.GV_ATTN_MAX_N]
        if long and getattr(G, "stream_maps", False):
            if max(long) > L.GV_ATTN_STREAM_MAX_N:
                raise ValueError(f"attention maps: {max(long)} tokens per image is past the {L.GV_ATTN_STREAM_MAX_N}-token limit of "
                                 f"gv_attention_probs_stream (images up to 512 px at patch 16)")
            return
        if long:
            raise ValueError(f"attention maps: {long[0]} tokens per image is past the {L.GV_ATTN_MAX_N}-token limit of gv_attention_probs "
                             f"(images up to 256 px at patch 16); features and intermediate layers work up to {L.GV_ATTN_STREAM_MAX_N} tokens")

    def _cls_tail(self, G: VitGroup) -> bool:
        """Does this group run the last block's projection / MLP on the CLS rows only?  (Training groups: on the grouped
        weight-gradient path and without --drop, whose backward this build restates for that case.)  Never for a mean-pooled
        group: every token of the last block reaches the feature."""
        return G.pool != "avg" and not G.all_tokens and self.cls_last and G.dropout is None and (not G.save or self.group_dw)

    def _last_block_tail_fwd(self, W: Weights, G: VitGroup, i: int, xa: torch.Tensor, on_side: bool):
        """x + proj(attention) -> norm2 -> MLP -> residual of block i for the CLS rows only (vit.pyc@L146-152 on the rows that
        VisionTransformer.forward returns, L248-253): n_img rows through the tiled GEMM and a LayerNorm pass (a full-row kernel
        streams a whole weight matrix per workgroup at this row count)."""
        G.alloc_cls()
        D, n, s, E, b = self.D, G.n_img, G.slot(i), L, f"blocks.{i}."
        rs_a, rs_m = (G.drop_img[i, 0], G.drop_img[i, 1]) if G.rs is not None else (None, None)       # per image = per CLS row
        G.gather_cls(G.o[s], G.c_o)
        G.gather_cls(xa, G.c_xa)
        ops.linear(G.c_o, W.w(b + "attn.proj.weight"), G.c_xb, n, D, D, epilogue=E.EPI_BIAS | E.EPI_RESID,
                   bias=W.f(b + "attn.proj.bias"), resid=G.c_xa, row_scale=rs_a)
        ops.layernorm_fwd(G.c_xb, W.f(b + "norm2.weight"), W.f(b + "norm2.bias"), n, D, y=G.c_xn2, mean=G.c_stats[0], rstd=G.c_stats[1])
        ops.linear(G.c_xn2, W.w(b + "mlp.fc1.weight"), G.c_h, n, 4 * D, D, epilogue=E.EPI_BIAS | E.EPI_GELU | (E.EPI_SAVE_PRE if G.save else 0),
                   bias=W.f(b + "mlp.fc1.bias"), aux_out=G.c_hp if G.save else None)
        # (a few hundred rows, a 4 D-deep reduction: gv_linear splits K when handed a scratch -- the one of the stream this pass is queued on)
        ops.linear(G.c_h, W.w(b + "mlp.fc2.weight"), G.c_xc, n, D, 4 * D, epilogue=E.EPI_BIAS | E.EPI_RESID,
                   bias=W.f(b + "mlp.fc2.bias"), resid=G.c_xb, row_scale=rs_m, workspace=self.ws_side if on_side else self.ws_main)

    def prepare_backward(self, G: VitGroup):
        """Zero the backward scratch that is accumulated into or only partly written: the residual gradient (the final norm's backward
        writes the CLS rows), and the attention-output gradient of the CLS-only last block / the first dY buffer otherwise.  Stream-
        ordered fills with no input: an engine may issue them early on its side stream (DinoEngine does, beside the forward pass).
        A mean-pooled group needs none: gv_token_mean_bwd writes every row of both."""
        if G.pool == "avg":
            G.prepared = True
            return
        G.g.zero_()
        if self._cls_tail(G):
            G.alloc_cls()
            G.do.zero_()
        else:
            (G.gb3 if (self.depth - 1) & 1 else G.gb).zero_()      # the last block's MLP-half dY (backward: sets[parity][0])
        G.prepared = True

    # ---- backward from d(CLS features) bf16 [G.n_img, D]; gradients ACCUMULATE into the arena
    def backward(self, W: Weights, G: VitGroup, dfeat: torch.Tensor, on_block_done=None, patch=None):
        """``on_block_done(i)`` is called once block i's parameter gradients are complete
        (data-parallel engines start that block's all-reduce there).  ``patch``: the (MaskPlan, PatchRows) the forward was given --
        the head's gradient of the marked rows (``PatchRows.hb.dfeats``) goes back through the final norm into those rows of the
        residual gradient and of the last block's MLP-half dY, and ``mask_token`` gets its gradient behind gv_tokens_bwd."""
        self.require_trainable(G)
        if patch is not None and patch[0].M == 0:
            patch = None
        D, T, H = self.D, G.T, self.H
        E = L
        ACC = E.EPI_ACCUM
        # --drop: the gradient entering a dropout site carries that site's mask (regenerated from the step seed); the bias gradients
        # of attn.proj / mlp.fc2 are then column sums of the MASKED gradient, not LayerNorm backward's third sum
        dp = G.dropout
        dseed = (lambda layer, site: ops.dropout_site_seed(dp[1], layer, site)) if dp else None
        fused_b = self.fused and dp is None

        def drop_branch_grad(gb, layer, site, bias_grad):
            ops.dropout(gb, dseed(layer, site), dp[0], n=T * D)
            ops.colsum(gb, T, D, self.cs_ws, bias_grad, accumulate=True)
        sets = ((G.gb, G.gb2, G.dh, G.dqkv), (G.gb3, G.gb4, G.dh_b, G.dqkv_b))      # per block parity: dY of the MLP / attention half, dh, dqkv
        gb_first = sets[(self.depth - 1) & 1][0]
        cls_tail = self._cls_tail(G)          # the last block ran its projection / MLP on the CLS rows only (forward): so does its backward
        if not G.prepared:
            self.prepare_backward(G)
        G.prepared = False
        # stochastic depth: the bf16 gradient handed to a branch carries that branch's row factor (rs[i, 0] attention, rs[i, 1] MLP)
        rs = G.rs
        ring = self.partials_ring
        self._final_norm_bwd(W, G, dfeat, gb_first, cls_tail, patch)
        # The weight-gradient GEMMs are off the critical path (nothing in backward consumes dW):
        # they run on a side stream beside the dX chain, so their tiles fill the tail of every
        # main-stream kernel (a 345 x 3-tile GEMM occupies 2.02 rounds of the 512 workgroup slots).
        # join(ev): main waits for a side event before it overwrites a buffer a dW product still reads (gb / dh / dqkv).
        sx = SideStream(self.side if G.g.is_cuda else None, self._events)
        join = sx.join

        # LayerNorm backward leaves per-block column sums in a partials buffer; folding them into the gamma / beta /
        # bias gradients (ln_finalize) is parameter-gradient work too, so it also goes to the side stream.  Three
        # partials buffers rotate; one is rewritten only after the finalize that read it (three calls ago) has run.
        fin_ev, ring_i, last_fin = [None, None, None], 0, None

        def ln_bwd(dy, x, mean, rstd, gamma, gb, d0, d1, d2, dx_of=None, gb_scale=None, rows=None, g=None):
            """LayerNorm backward into the residual gradient.  ``dx_of = (dY, W, K)``: the dX product that produces ``dy``
            runs fused with it (gv_linear_ln_bwd) and ``dy`` never exists in HBM.  ``rows`` / ``g``: a row count and residual
            gradient other than the group's T rows / G.g (the last block's CLS-only tail: the unfused pair)."""
            nonlocal ring_i, last_fin
            k = ring_i
            ring_i = (k + 1) % 3
            join(fin_ev[k])
            M_, g_ = (T if rows is None else rows), (G.g if g is None else g)
            if dx_of is not None and fused_b and rows is None:
                nblk = ops.linear_ln_bwd(dx_of[0], dx_of[1], x, mean, rstd, gamma, g_, gb, ring[k], M_, dx_of[2], gb_scale=gb_scale)
            else:
                if dx_of is not None:
                    ops.linear(dx_of[0], dx_of[1], dy, M_, D, dx_of[2], trans_b=True, workspace=self.ws_main if rows is not None else None)
                ops.layernorm_bwd(dy, x, mean, rstd, gamma, g_, gb, ring[k], M_, D, gb_scale=gb_scale)
                nblk = L.LN_PARTIAL_BLOCKS
            fin_ev[k] = last_fin = sx.run(lambda: ops.ln_finalize(ring[k], nblk, D, d0, d1, d2))

        def report(i):
            if on_block_done is not None:
                # the block's weight gradients are produced by the side stream: report the block from
                # there, so a data-parallel all-reduce queues behind the dW products and main never waits
                sx.then(lambda: on_block_done(i))

        def block_dw(probs):
            """The block's four weight gradients dW (+)= dY^T X (bias gradient: the column sums of dY), one side-stream item."""
            if self.group_dw:
                ops.linear_dw_group(probs, T, self.ws_side)
                return
            for dY, X, dW, cs in probs:
                ops.linear(dY, X, dW, dY.shape[1], X.shape[1], T, trans_a=True, trans_b=True, epilogue=ACC, colsum_a=cs, workspace=self.ws_side)

        streams = any(sg.N > L.GV_ATTN_MAX_N for sg in G.segs)

        def attn_bwd(i, dqkv, segs, **ql):
            """Block i's attention backward (``ql``: its q_limit keyword, if any): the varlen call over all segments -- or, when a segment is past
            GV_ATTN_MAX_N tokens, one call per segment as the forward makes them: gv_attention_bwd_stream for a long one,
            gv_attention_bwd for a short one."""
            if not streams:
                ops.attention_bwd_varlen(G.qkv[i], G.o[i], G.do, dqkv, segs, H, self.scale, **ql)
                return
            for sg in G.segs:
                bufs = (sg.rows(G.qkv[i]), sg.rows(G.o[i]), sg.rows(G.do), sg.lse[i], sg.n_img, sg.N, H, self.scale)
                if sg.N > L.GV_ATTN_MAX_N:
                    ops.attention_bwd_stream(*bufs, dqkv=sg.rows(dqkv), delta=G.delta, **ql)
                else:
                    ops.attention_bwd(*bufs, dqkv=sg.rows(dqkv), **ql)

        done_grp = [None, None]
        for i in reversed(range(self.depth)):
            b, st = f"blocks.{i}.", G.stats[i]
            par = i & 1
            gb_mlp, gb_att, dh, dqkv = sets[par]
            gb_next = sets[par ^ 1][0]                    # dY of block i - 1's MLP half
            segs = [(sg.n_img, sg.N, sg.lse[i]) for sg in G.segs]
            join(done_grp[par])                           # block i + 2's weight gradients read this parity's buffers
            if cls_tail and i == self.depth - 1:
                # ---- last block, CLS rows only (forward: _last_block_tail_fwd): MLP and projection backward over n_img rows; the
                # attention backward and the qkv product's dX + norm1 backward then run over all tokens as in every block, with
                # dO and the residual gradient zero outside the CLS rows (only K and V of the other tokens reached the output)
                n = G.n_img
                ops.linear(G.c_gb, W.w(b + "mlp.fc2.weight"), G.c_dh, n, 4 * D, D, trans_b=True, epilogue=E.EPI_DGELU, aux_in=G.c_hp)
                ln_bwd(G.c_dxn, G.c_xb, G.c_stats[0], G.c_stats[1], W.f(b + "norm2.weight"), G.c_gb_att,
                       W.g(b + "norm2.weight"), W.g(b + "norm2.bias"), W.g(b + "attn.proj.bias"),
                       dx_of=(G.c_dh, W.w(b + "mlp.fc1.weight"), 4 * D), gb_scale=None if rs is None else G.drop_img[i, 0], rows=n, g=G.c_g)
                ops.linear(G.c_gb_att, W.w(b + "attn.proj.weight"), G.c_do, n, D, D, trans_b=True)
                G.scatter_cls(G.c_do, G.do)           # (G.do was zeroed by prepare_backward)
                G.scatter_cls(G.c_g, G.g)                 # (G.g was zeroed above)
                # dO is zero behind every image's CLS row: the attention backward skips the other queries (their dQ rows come out zero)
                attn_bwd(i, dqkv, segs, q_limit=1 if self.sw.cls_qlimit else 0)
                ln_bwd(G.dxn, G.x[2 * i], st[0], st[1], W.f(b + "norm1.weight"), gb_next,
                       W.g(b + "norm1.weight"), W.g(b + "norm1.bias"), W.g(f"blocks.{i - 1}.mlp.fc2.bias") if i > 0 else None,
                       dx_of=(dqkv, W.w(b + "attn.qkv.weight"), 3 * D), gb_scale=None if (rs is None or i == 0) else rs[i - 1, 1])

                def tail_dw():
                    # three weight gradients reduce over the n CLS rows, the qkv one over all tokens
                    ops.linear(G.c_gb, G.c_h, W.g(b + "mlp.fc2.weight"), D, 4 * D, n, trans_a=True, trans_b=True, epilogue=ACC, workspace=self.ws_side)
                    ops.linear(G.c_dh, G.c_xn2, W.g(b + "mlp.fc1.weight"), 4 * D, D, n, trans_a=True, trans_b=True, epilogue=ACC,
                               colsum_a=W.g(b + "mlp.fc1.bias"), workspace=self.ws_side)
                    ops.linear(G.c_gb_att, G.c_o, W.g(b + "attn.proj.weight"), D, D, n, trans_a=True, trans_b=True, epilogue=ACC, workspace=self.ws_side)
                    ops.linear_dw_group([(dqkv, G.xn1[i], W.g(b + "attn.qkv.weight"), W.g(b + "attn.qkv.bias"))], T, self.ws_side)
                done_grp[par] = sx.run(tail_dw)
                report(i)
                continue
            if dp:
                drop_branch_grad(gb_mlp, i, 3, W.g(b + "mlp.fc2.bias"))
            ops.linear(gb_mlp, W.w(b + "mlp.fc2.weight"), dh, T, 4 * D, D, trans_b=True, epilogue=E.EPI_DGELU, aux_in=G.hp[i])
            if dp:
                ops.dropout(dh, dseed(i, 2), dp[0], n=T * 4 * D)
            ln_bwd(G.dxn, G.x[2 * i + 1], st[2], st[3], W.f(b + "norm2.weight"), gb_att,
                   W.g(b + "norm2.weight"), W.g(b + "norm2.bias"), None if dp else W.g(b + "attn.proj.bias"),
                   dx_of=(dh, W.w(b + "mlp.fc1.weight"), 4 * D), gb_scale=None if rs is None else rs[i, 0])
            if dp:
                drop_branch_grad(gb_att, i, 1, W.g(b + "attn.proj.bias"))
            ops.linear(gb_att, W.w(b + "attn.proj.weight"), G.do, T, D, D, trans_b=True)
            attn_bwd(i, dqkv, segs)
            # the block's four dY operands are final once the attention backward has run: its weight gradients go to the side stream
            # BEFORE the last kernel of the block's dX chain (which only reads dqkv), one kernel earlier than the chain's end
            probs = [(gb_mlp, G.h[i], W.g(b + "mlp.fc2.weight"), None),
                     (dh, G.xn2[i], W.g(b + "mlp.fc1.weight"), W.g(b + "mlp.fc1.bias")),
                     (gb_att, G.o[i], W.g(b + "attn.proj.weight"), None),
                     (dqkv, G.xn1[i], W.g(b + "attn.qkv.weight"), W.g(b + "attn.qkv.bias"))]
            done_grp[par] = sx.run(lambda: block_dw(probs))
            join(done_grp[par ^ 1])                       # block i + 1's weight gradients read gb_next (its MLP-half dY)
            ln_bwd(G.dxn, G.x[2 * i], st[0], st[1], W.f(b + "norm1.weight"), gb_next,
                   W.g(b + "norm1.weight"), W.g(b + "norm1.bias"), W.g(f"blocks.{i - 1}.mlp.fc2.bias") if (i > 0 and not dp) else None,
                   dx_of=(dqkv, W.w(b + "attn.qkv.weight"), 3 * D), gb_scale=None if (rs is None or i == 0) else rs[i - 1, 1])
            report(i)
        join(done_grp[0]); join(done_grp[1])    # every dW product is in (the side stream runs them in order); ws_side is free again
        join(last_fin)          # ... and the last finalize
        if dp:
            ops.dropout(G.g, dseed(0, 0), dp[0], n=T * D)                                 # pos_drop's mask on the token gradient
        self._embed_bwd(W, G, patch)

    def _final_norm_bwd(self, W: Weights, G: VitGroup, dfeat: torch.Tensor, gb_first: torch.Tensor, cls_tail: bool, patch):
        """The first stage of ``backward``: the final norm's backward of every segment (``_final_norm``'s three forms) and of iBOT's
        marked rows, into the residual gradient ``G.g`` and ``gb_first``, the last block's MLP-half dY."""
        D, dp, rs, ring, xl = self.D, G.dropout, G.rs, self.partials_ring, G.x[2 * self.depth]
        fc2_bias = W.g(f"blocks.{self.depth - 1}.mlp.fc2.bias")      # its gradient is the third column sum of these launches (not under --drop)
        for sg in G.segs:
            # (the final norm touches the CLS rows only, one per image: the per-image factors are its row factors)
            im = slice(sg.img0, sg.img0 + sg.n_img)
            gs = None if rs is None else G.drop_img[self.depth - 1, 1, im]
            if G.pool == "avg":
                # fc_norm backward over the pooled rows -> dpool, spread over the patch rows of the residual gradient and of the
                # last block's MLP-half dY (the CLS rows: zeros).  The last mlp.fc2.bias gradient is the column sum of that dY's
                # f32 source over every token row, sum_img gb_scale[img] * dpool[img]: the third sum of this launch
                ops.layernorm_bwd(dfeat[im], G.pooled[im], sg.fstats[0], sg.fstats[1], W.f("fc_norm.weight"), G.dpool[im], None, ring[0],
                                  sg.n_img, D, g_init=True, gb_scale=gs)
                ops.ln_finalize(ring[0], L.LN_PARTIAL_BLOCKS, D, W.g("fc_norm.weight"), W.g("fc_norm.bias"), None if dp else fc2_bias)
                ops.token_mean_bwd(G.dpool[im], sg.rows(G.g), sg.rows(gb_first), sg.n_img, sg.N, D, gb_scale=gs)
                continue
            if cls_tail:
                ops.layernorm_bwd(dfeat[im], G.c_xc[im], sg.fstats[0], sg.fstats[1], W.f("norm.weight"), G.c_g[im], G.c_gb[im], ring[0],
                                  sg.n_img, D, g_init=True, gb_scale=gs)
            else:
                ops.layernorm_bwd(dfeat[im], sg.rows(xl), sg.fstats[0], sg.fstats[1], W.f("norm.weight"), sg.rows(G.g),
                                  sg.rows(gb_first), ring[0], sg.n_img, D, x_stride=sg.N * D, g_stride=sg.N * D, gb_stride=sg.N * D, g_init=True,
                                  gb_scale=gs)
            ops.ln_finalize(ring[0], L.LN_PARTIAL_BLOCKS, D, W.g("norm.weight"), W.g("norm.bias"), None if dp else fc2_bias)
        if patch is not None:
            # the marked rows (unique, never a CLS row): the norm's backward on the compact copy, its three column sums next to the
            # CLS rows' share, then a plain store into the rows prepare_backward left at zero
            assert not cls_tail and G.pool != "avg" and dp is None
            plan, pr = patch
            sg, M = G.segs[0], plan.M
            ops.layernorm_bwd(pr.hb.dfeats, pr.x, pr.mean, pr.rstd, W.f("norm.weight"), pr.g, pr.gb, ring[0], M, D, g_init=True,
                              gb_scale=None if rs is None else pr.scale)
            ops.ln_finalize(ring[0], L.LN_PARTIAL_BLOCKS, D, W.g("norm.weight"), W.g("norm.bias"), fc2_bias)
            ops.rows_scatter(pr.g, sg.rows(G.g), plan.rows, M, D, sg.T, gb_src=pr.gb, gb=sg.rows(gb_first))

    def _embed_bwd(self, W: Weights, G: VitGroup, patch):
        """The last stage of ``backward``, per segment: token assembly and the patch embedding's gradients (``_embed``'s mirror)."""
        D, ACC = self.D, L.EPI_ACCUM
        gpos = W.g("pos_embed").view(-1, D)
        for k, sg in enumerate(G.segs):
            ops.tokens_bwd(sg.rows(G.g), sg.gpatch, sg.dpos, None, sg.n_img, sg.N, D, accumulate=False)
            if patch is not None and k == 0:
                # a masked patch's token is mask_token + pos: its gradient goes to mask_token (and stays in dpos), the patch embedding
                # gets nothing from it -- zero rows of gpatch for the weight, and its share taken back out of the bias's column sum
                pr = patch[1]
                ops.mask_tokens_bwd(sg.rows(G.g), sg.gpatch, pr.dmask, patch[0].rows, pr.mt_ws, patch[0].M, sg.N, D, accumulate=False)
                ops.small_matmul(self.one, pr.dmask, W.g("mask_token").view(1, D), 1, D, 1, sam=0, sak=0, sbk=0, sbn=1, accumulate=True)
                ops.small_matmul(pr.minus_one, pr.dmask, W.g("patch_embed.proj.bias").view(1, D), 1, D, 1, sam=0, sak=0, sbk=0, sbn=1, accumulate=True)
            # d cls_token = sum over images of the CLS-row gradient = dpos row 0
            ops.small_matmul(self.one, sg.dpos, W.g("cls_token").view(1, D), 1, D, 1, sam=0, sak=0, sbk=0, sbn=1, accumulate=True)
            ops.linear(sg.gpatch, sg.patches, W.g("patch_embed.proj.weight").view(D, 768), D, 768, sg.n_img * sg.P,
                       trans_a=True, trans_b=True, epilogue=ACC, workspace=self.ws_side)
            ops.colsum(sg.dpos[1:], sg.P, D, self.cs_ws, W.g("patch_embed.proj.bias"), accumulate=True)
            if sg.pos is None:
                ops.small_matmul(self.one, sg.dpos, gpos, 1, sg.N * D, 1, sam=0, sak=0, sbk=0, sbn=1, accumulate=True)
            else:
                Ps = gpos.shape[0] - 1
                ops.small_matmul(self.one, sg.dpos, gpos, 1, D, 1, sam=0, sak=0, sbk=0, sbn=1, accumulate=True)
                ops.small_matmul(sg.interp, sg.dpos[1:], gpos[1:], Ps, D, sg.P, sam=1, sak=Ps, sbk=D, sbn=1, accumulate=True)


# --------------------------------------------------------------------------- #
# DINO head (vit.pyc@L296-330) forward / backward over R rows
# --------------------------------------------------------------------------- #
class HeadBuffers:
    def __init__(self, R: int, D: int, K: int, hidden: int, bott: int, device, save: bool, act=bf16):
        e = lambda shape, dt: _empty(shape, dt, device)
        self.R = R
        self.feats = e((R, D), act)
        self.h1p, self.h1 = e((R, hidden), act), e((R, hidden), act)
        self.h2p, self.h2 = e((R, hidden), act), e((R, hidden), act)
        self.z, self.zn, self.inv = e((R, bott), f32), e((R, bott), act), e((R,), f32)
        self.logits = e((R, K), f32)
        if save:
            self.dlogits = e((R, K), act)
            self.dzn, self.dz = e((R, bott), f32), e((R, bott), act)
            self.dh2, self.dh1 = e((R, hidden), act), e((R, hidden), act)
            self.dfeats = e((R, D), act)
            self.dwn = e((K, bott), f32)


class PatchRows:
    """Buffers of iBOT's marked rows for one network: the head buffers of up to ``R`` rows (``hb``), the compact f32 copy of the
    rows in front of the final norm with its statistics and -- for the student (``save``) -- the norm's backward outputs, the rows'
    stochastic-depth factors and the scratch of gv_mask_tokens_bwd."""

    def __init__(self, R: int, D: int, K: int, hidden: int, bott: int, device, save: bool, act=bf16):
        e = lambda shape, dt: _empty(shape, dt, device)
        self.R = R
        self.hb = HeadBuffers(R, D, K, hidden, bott, device, save, act)
        self.x, self.mean, self.rstd = e((R, D), f32), e((R,), f32), e((R,), f32)
        if save:
            self.g, self.gb, self.scale = e((R, D), f32), e((R, D), act), e((R,), f32)
            self.dmask = e((D,), f32)
            self.mt_ws = e((_ws_bytes("gv_mask_tokens_workspace_bytes", R, D) // 4,), f32)
            self.minus_one = torch.full((1,), -1.0, dtype=f32, device=device)


def masks_fit(plan, sg: Segment, pr: Optional["PatchRows"] = None):
    """A MaskPlan against the segment it indexes (and the buffers its rows go to): a ValueError before anything is launched."""
    if plan.J != sg.n_img or plan.P != sg.P:
        raise ValueError(f"masks: a plan for {plan.J} images of {plan.P} patches, the global crops are {sg.n_img} images of {sg.P}")
    if pr is not None and plan.M > pr.R:
        raise ValueError(f"masks: {plan.M} marked patches, the iBOT head buffers hold {pr.R} rows (ibot_mask_ratio / ibot_mask_prob size them)")


class HeadRunner:
    def __init__(self, D: int, K: int, hidden: int, bott: int, device):
        self.D, self.K, self.hidden, self.bott = D, K, hidden, bott
        self.cs_ws = _empty((64 * max(hidden, bott),), f32, device)
        # split-K slabs per stream (a few hundred rows against 2048-deep reductions: gv_linear splits K when handed a scratch)
        self.ws_main = _empty((L.lib.gv_linear_workspace_bytes() // 4,), f32, device)
        self.ws_side = _empty((L.lib.gv_linear_workspace_bytes() // 4,), f32, device)

    def forward(self, W: Weights, wn: torch.Tensor, hb: HeadBuffers, on_side: bool = False, rows: Optional[int] = None):
        """``on_side``: the call is queued on the engine's side stream (the teacher's head beside the student's forward): its
        split-K products then take the side stream's scratch.  ``rows``: the first so many rows of the buffers only (iBOT's marked
        rows: the buffers are sized once, every step has its own count)."""
        R, D, Hd, Bt, K, E = (hb.R if rows is None else rows), self.D, self.hidden, self.bott, self.K, L
        ws = self.ws_side if on_side else self.ws_main
        ops.linear(hb.feats, W.w("mlp.0.weight"), hb.h1, R, Hd, D, epilogue=E.EPI_BIAS | E.EPI_GELU | E.EPI_SAVE_PRE,
                   bias=W.f("mlp.0.bias"), aux_out=hb.h1p)
        ops.linear(hb.h1, W.w("mlp.2.weight"), hb.h2, R, Hd, Hd, epilogue=E.EPI_BIAS | E.EPI_GELU | E.EPI_SAVE_PRE,
                   bias=W.f("mlp.2.bias"), aux_out=hb.h2p, workspace=ws)
        ops.linear(hb.h2, W.w("mlp.4.weight"), hb.z, R, Bt, Hd, epilogue=E.EPI_BIAS, bias=W.f("mlp.4.bias"), workspace=ws)
        ops.l2norm_fwd(hb.z, hb.zn, hb.inv, R, Bt)
        ops.linear(hb.zn, wn, hb.logits, R, K, Bt)

    def backward(self, W: Weights, wn: torch.Tensor, hb: HeadBuffers, train_last_layer: bool, sx: SideStream, rows: Optional[int] = None):
        """The weight-gradient products (they feed nothing in backward) go through ``sx``, the engine's side stream: each is
        queued there once its operands are ready, with the scratch of the stream it runs on.  ``rows``: as in ``forward``."""
        R, D, Hd, Bt, K, E = (hb.R if rows is None else rows), self.D, self.hidden, self.bott, self.K, L
        ACC = E.EPI_ACCUM
        ws = self.ws_side if sx.side is not None else self.ws_main

        def dw_last():     # dW_n = dlogits^T zn, then through weight_norm (g frozen: norm_last_layer)
            ops.linear(hb.dlogits, hb.zn, hb.dwn, K, Bt, R, trans_a=True, trans_b=True)
            ops.weightnorm_bwd(hb.dwn, W.f("last_layer.weight_v"), W.f("last_layer.weight_g").view(-1),
                               W.g("last_layer.weight_v"), None, K, Bt, accumulate=True)
        if train_last_layer:
            sx.run(dw_last)
        hb.dzn.zero_()         # split-K over the K=65536 classes accumulates with atomics
        ops.linear(hb.dlogits, wn, hb.dzn, R, Bt, K, trans_b=True, epilogue=ACC, workspace=self.ws_main)
        ops.l2norm_bwd(hb.dzn, hb.zn, hb.inv, hb.dz, R, Bt)
        sx.run(lambda: ops.linear(hb.dz, hb.h2, W.g("mlp.4.weight"), Bt, Hd, R, trans_a=True, trans_b=True, epilogue=ACC,
                                  colsum_a=W.g("mlp.4.bias"), workspace=ws))
        ops.linear(hb.dz, W.w("mlp.4.weight"), hb.dh2, R, Hd, Bt, trans_b=True, epilogue=E.EPI_DGELU, aux_in=hb.h2p)
        sx.run(lambda: ops.linear(hb.dh2, hb.h1, W.g("mlp.2.weight"), Hd, Hd, R, trans_a=True, trans_b=True, epilogue=ACC,
                                  colsum_a=W.g("mlp.2.bias"), workspace=ws))
        ops.linear(hb.dh2, W.w("mlp.2.weight"), hb.dh1, R, Hd, Hd, trans_b=True, epilogue=E.EPI_DGELU, aux_in=hb.h1p, workspace=self.ws_main)
        sx.run(lambda: ops.linear(hb.dh1, hb.feats, W.g("mlp.0.weight"), Hd, D, R, trans_a=True, trans_b=True, epilogue=ACC,
                                  colsum_a=W.g("mlp.0.bias"), workspace=ws))
        ops.linear(hb.dh1, W.w("mlp.0.weight"), hb.dfeats, R, D, Hd, trans_b=True, workspace=self.ws_main)


# --------------------------------------------------------------------------- #
# data-parallel reduction hooks (engine stays importable without torch.distributed)
# --------------------------------------------------------------------------- #
class NoReducer:
    world = 1

    def reduce_range(self, buf, lo, hi):
        pass

    def reduce_tensor(self, t):
        pass

    def reduce_max(self, t):
        pass

    def finish(self):
        pass


def _ws_bytes(query: str, *shape) -> int:
    """A workspace query of the library (gv_*_workspace_bytes); the shape it refuses is a ValueError with the library's words."""
    n = getattr(L.lib, query)(*shape)
    if n < 0:
        raise ValueError(L.lib.gv_last_error().decode())
    return n


def operand_mode(precision: str):
    """``precision`` "bf16" | "fp32" -> (fp32 operand mode?, element type of the activation buffers)."""
    if precision not in ("bf16", "fp32"):
        raise ValueError(f"precision {precision!r}: 'bf16' or 'fp32'")
    return precision == "fp32", (f32 if precision == "fp32" else bf16)


def _prefixed(backbone: Dict[str, torch.Tensor], head: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The two state dicts of a DINO network under their arena names."""
    st = {"backbone." + k: v for k, v in backbone.items()}
    st.update({"head." + k: v for k, v in head.items()})
    return st


def _check_ibot(weight, ratio, prob, gsize: int, drop: float, centering: str) -> float:
    """The iBOT options an engine is built with (the driver's check_supported says the same before any GPU work) -> the weight."""
    from .masking import check_mask_options
    if not (isinstance(weight, (int, float)) and math.isfinite(weight) and weight >= 0):
        raise ValueError(f"ibot_weight {weight}: finite and >= 0")
    check_mask_options(ratio, prob)
    if weight > 0:
        if gsize < 64:
            raise ValueError(f"ibot_weight > 0 needs global crops of at least 64 px (a 4 x 4 patch grid), got {gsize}")
        if drop and drop > 0:
            raise ValueError("ibot_weight > 0 with drop > 0 is not built (the dropout path has no all-token last block with a row table)")
        if centering == "sinkhorn_knopp":
            raise ValueError("ibot_weight > 0 with centering 'sinkhorn_knopp' is not built: Sinkhorn-Knopp over a patch-row count that varies per "
                             "rank is missing, and the EMA patch centre in its place would be a silent substitution")
    return float(weight)


def accumulate_micro(acc: Dict[torch.Tensor, torch.Tensor], table, j: int, n: int):
    """Gradient accumulation of a step's outputs: micro-batch ``j`` of ``n`` has just written every tensor of ``table``, rows of
    (tensor, mean).  Their running sums are kept in ``acc`` (a clone on the first micro-batch), and the last micro-batch leaves in
    the tensor the mean over the n values (``mean``: the loss terms) or their sum (the centre sums).  n = 1: nothing is touched."""
    if n == 1:
        return
    for t, mean in table:
        acc[t] = t.clone() if j == 0 else acc[t] + t
        if j == n - 1:
            t.copy_(acc[t] / n if mean else acc[t])


def check_long_seq(long_seq: bool, precision: str, crops: Sequence[int]) -> bool:
    """The engines' ``long_seq`` keyword (train.py --train-long-seq): training crops past GV_ATTN_MAX_N tokens, their attention
    backward streamed (gv_attention_bwd_stream).  What it cannot do is refused here, before any device work."""
    if not long_seq:
        return False
    if precision == "fp32":
        raise ValueError(f"long_seq=True with precision='fp32': the streaming attention has no fp32 operand form (that mode stops at "
                         f"{L.GV_ATTN_F32_MAX_N} tokens); long sequences train in the 16-bit mode")
    for crop in crops:
        n_tok = (crop // 16) ** 2 + 1
        if n_tok > L.GV_ATTN_STREAM_MAX_N:
            raise ValueError(f"long_seq=True with a {crop}-px crop: {n_tok} tokens per image is past the {L.GV_ATTN_STREAM_MAX_N}-token "
                             f"limit of the streaming attention (images up to 512 px at patch 16)")
    return True


class TrainEngine:
    """What the two training engines share: the precision / clip-mode arguments and the loss scaler, the gradients handed out,
    and the clip / loss-scale part of the optimizer's arguments."""

    def _set_modes(self, precision: str, clip_mode: str, clip_modes: Sequence[str], dev):
        """-> (fp32, act) of ``operand_mode``; sets ``precision``, ``clip_mode`` (train.py:1072-1077) and ``scaler``."""
        if clip_mode not in clip_modes:
            raise ValueError(f"clip_mode {clip_mode!r}: one of {', '.join(clip_modes)} (train.py:1072-1077)")
        fp32, act = operand_mode(precision)
        self.precision, self.clip_mode = precision, clip_mode
        # the float16 library build (--amp --amp-dtype float16) trains under dynamic loss scaling: torch's GradScaler on the device
        # (via timm NativeScaler, reference train.py:585-602, 1061-1070)
        self.scaler = ops.LossScaler(dev) if (L.ACT_FORMAT == "f16" and not fp32) else None
        return fp32, act

    @property
    def loss_scale(self) -> Optional[torch.Tensor]:
        """The ``loss_scale`` argument of the loss and optimizer launches: the scaler's device scale, None without loss scaling."""
        return self.scaler.scale if self.scaler is not None else None

    def grads(self) -> Dict[str, torch.Tensor]:
        """Copies of the parameter gradients of the last forward_backward.  Under float16 loss scaling the arena holds S x gradient:
        the copies are divided by the scale in force (call before optimizer_step, whose scaler update may change S)."""
        inv = None if self.scaler is None else 1.0 / self.scaler.state[0]
        return {n: self.arena.view(self.arena.g, n).detach().clone() if inv is None else self.arena.view(self.arena.g, n).detach() * inv
                for n in self.arena.specs}

    def _clip_args(self) -> dict:
        """The optimizer launches' clip_norm / gnorm_sq / clip_value / loss_scale arguments; queues the gradient's sum of squares
        when they need it (under loss scaling it is also the finite check of GradScaler.step())."""
        by_norm = self.clip > 0 and self.clip_mode == "norm"
        need_norm = by_norm or self.scaler is not None
        if need_norm:
            ops.sumsq(self.arena.g, self.red_ws, self.gnorm_sq)
        return dict(clip_norm=self.clip if by_norm else 0.0, gnorm_sq=self.gnorm_sq if need_norm else None,
                    clip_value=self.clip if (self.clip > 0 and self.clip_mode == "value") else 0.0,
                    loss_scale=self.loss_scale)


# --------------------------------------------------------------------------- #
# one DINO multi-crop training step (paper Alg. 1)
# --------------------------------------------------------------------------- #
class DinoEngine(TrainEngine):
    def __init__(self, arch="vit_small", img_size=224, out_dim=65536, batch=64, tile=256, n_global=2, n_local=8,
                 gsize=224, lsize=96, hidden=2048, bottleneck=256, lr=5e-4, weight_decay=0.04, betas=(0.9, 0.999), eps=1e-8,
                 momentum_teacher=0.996, student_temp=0.1, teacher_temp=0.04, center_momentum=0.9, clip_grad: float = 0.0,
                 mean=MEAN_RON, std=STD_RON, windows=None, device="cuda:0", reducer=None, precision: str = "bf16", clip_mode: str = "norm",
                 centering: str = "center", sinkhorn_iters: int = 3, koleo_weight: float = 0.0, ibot_weight: float = 0.0,
                 ibot_mask_ratio: Tuple[float, float] = (0.1, 0.5), ibot_mask_prob: float = 0.5, drop: float = 0.0,
                 long_seq: bool = False):
        """``precision``: "bf16" (the training path) or "fp32" (every GEMM / attention operand, the head activations, the
        weight-normalised prototype matrix and the logit gradient in f32 -- the verification mode of SURVEY 8d's fp32 column).
        ``clip_mode``: "norm" (global norm, the reference default) or "value" (element-wise clamp), train.py:1072-1077.
        ``centering``: "center" (the EMA centre of DINO) or "sinkhorn_knopp" (DINOv2: ``sinkhorn_iters`` Sinkhorn-Knopp iterations
        over the teacher logits of all ranks, handed to the loss as ``sk_center``; the EMA centre keeps running beside it).
        ``koleo_weight`` > 0 adds that multiple of the KoLeo regulariser on the student's features of every global crop (DINOv2 uses
        0.1): ``koleo`` is its unweighted value, local to the rank, ``loss`` stays the DINO term.
        ``ibot_weight`` > 0 adds that multiple of the iBOT masked-patch term (DINOv2 uses 1.0): every step then takes a
        gipvit.masking.MaskPlan (``masks=``) over its global crops, the student sees ``backbone.mask_token`` in place of the marked
        patches, both networks run their last block on every token and the marked rows go through the same head a second time
        against the second EMA centre ``patch_center``.  ``ibot`` is the term's unweighted value, ``loss`` stays the DINO term.
        ``ibot_mask_ratio`` / ``ibot_mask_prob`` size the patch-row buffers (masking.max_rows).  ``drop``: the run's --drop, only
        so that the combination is refused here.
        ``long_seq``: crops past GV_ATTN_MAX_N tokens (above 256 px) may be trained on: the student's attention backward of such a
        segment streams (gv_attention_bwd_stream, up to 512 px).  Groups without such a segment launch exactly what they do without it."""
        self.long_seq = check_long_seq(long_seq, precision, (gsize,) + ((lsize,) if n_local else ()))
        self.ibot_weight = _check_ibot(ibot_weight, ibot_mask_ratio, ibot_mask_prob, gsize, drop, centering)
        if centering not in ("center", "sinkhorn_knopp"):
            raise ValueError(f"centering {centering!r}: 'center' or 'sinkhorn_knopp'")
        if not 1 <= int(sinkhorn_iters) <= 8:
            raise ValueError(f"sinkhorn_iters {sinkhorn_iters}: 1..8")
        if not (math.isfinite(koleo_weight) and koleo_weight >= 0):
            raise ValueError(f"koleo_weight {koleo_weight}: finite and >= 0")
        if koleo_weight > 0 and batch < 2:
            raise ValueError("koleo_weight > 0 needs a batch of at least 2: the nearest neighbour is taken among the other tiles of the crop")
        dev = torch.device(device)
        fp32, act = self._set_modes(precision, clip_mode, ("norm", "value"), dev)
        self.dev, self.arch, self.B, self.tile = dev, arch, batch, tile
        D = ARCHS[arch]["embed_dim"]
        self.D, self.K, self.G, self.V = D, out_dim, n_global, n_global + n_local
        self.mean, self.std = tuple(mean), tuple(std)
        self.gsize, self.lsize = gsize, lsize
        self._gcrops = self._lcrops = self._vstats = None       # crop buffers of the random-resized-crop path (allocated on first use)
        if windows is None:   # deterministic crop windows of SURVEY 8(d): (y0, x0)
            windows = [(16 * g, 16 * g) for g in range(n_global)] + [(20 * l, 160 - 20 * l) for l in range(n_local)]
        self.gwins, self.lwins = list(windows[:n_global]), list(windows[n_global:])
        specs = OrderedDict(("backbone." + k, v) for k, v in vit_param_specs(arch, img_size, 0).items())
        specs.update(("head." + k, v) for k, v in dino_head_specs(D, out_dim, hidden, bottleneck).items())
        if self.ibot_weight > 0:      # last of the no-decay part of the arena (every other offset is that of a run without iBOT)
            specs["backbone.mask_token"] = (1, D)
        self.arena = Arena(specs, dev, teacher=True)
        self.sW, self.tW = Weights(self.arena, "backbone.", fp32=fp32), Weights(self.arena, "backbone.", teacher=True, fp32=fp32)
        self.sH, self.tH = Weights(self.arena, "head.", fp32=fp32), Weights(self.arena, "head.", teacher=True, fp32=fp32)
        self.sw = EngineSwitches.from_env()
        self.vit = VitRunner(arch, img_size, dev, fp32=fp32, sw=self.sw)
        self.head = HeadRunner(D, out_dim, hidden, bottleneck, dev)
        B = batch
        segs = [(n_global * B, gsize)] + ([(n_local * B, lsize)] if n_local else [])
        self.g_stu = VitGroup(arch, segs, img_size, dev, save=True, act=act, stream_bwd=self.long_seq)   # all student crops, tokens concatenated
        self.g_teach = VitGroup(arch, [(n_global * B, gsize)], img_size, dev, save=False, act=act)
        self.s_wins = [self.gwins] + ([self.lwins] if n_local else [])
        self.hb_s = HeadBuffers(self.V * B, D, out_dim, hidden, bottleneck, dev, save=True, act=act)
        self.hb_t = HeadBuffers(n_global * B, D, out_dim, hidden, bottleneck, dev, save=False, act=act)
        self.wn_s = _carried((out_dim, bottleneck), act, dev)      # written by _refresh_wn: at load_state and behind every optimizer step
        self.wn_t = _carried((out_dim, bottleneck), act, dev)      # written by _refresh_wn, as wn_s
        self.center = torch.zeros(out_dim, dtype=f32, device=dev)
        self.center_sum = torch.zeros(out_dim, dtype=f32, device=dev)
        self.loss = torch.zeros(1, dtype=f32, device=dev)
        self.loss_ws = _empty((2 * (self.V + self.G) * B,), f32, dev)
        self.centering, self.sinkhorn_iters, self.koleo_weight = centering, int(sinkhorn_iters), float(koleo_weight)
        self.sk_center = self.koleo = self.koleo_nn = None
        if centering == "sinkhorn_knopp":       # written by every step's _sinkhorn before the loss reads sk_center
            R = n_global * B
            self.sk_center, self.sk_a, self.sk_colsum = (_empty((out_dim,), f32, dev) for _ in range(3))
            self.sk_b, self.sk_shift = _empty((R,), f32, dev), _empty((1,), f32, dev)
            self.sk_ws = _empty((_ws_bytes("gv_sinkhorn_workspace_bytes", R, out_dim) // 4,), f32, dev)
        if koleo_weight > 0:
            self.koleo = _empty((1,), f32, dev)           # written by every forward's gv_koleo_fwd
            # an index table: _empty refuses wide integers (all-ones poison would be a wild index).  gv_koleo_fwd writes every entry
            # before gv_koleo_bwd reads one, and the backward clamps what it reads into the crop
            self.koleo_nn = torch.zeros(n_global * B, dtype=torch.int32, device=dev)
            self.koleo_ws = _empty((_ws_bytes("gv_koleo_workspace_bytes", n_global, B, D) // 4,), f32, dev)
        self.ibot = self.patch_center = self.patch_center_sum = self.pr_s = self.pr_t = None
        if self.ibot_weight > 0:
            from .masking import max_rows
            if L.ACT_FORMAT == "f16" and not fp32:
                raise ValueError("ibot_weight > 0 is not built for the float16 library (--amp needs --amp-dtype bfloat16)")
            self.g_stu.all_tokens = self.g_teach.all_tokens = True
            R = max(1, max_rows(n_global * B, (gsize // 16) ** 2, ibot_mask_ratio, ibot_mask_prob))
            self.ibot_rows = R
            self.pr_s = PatchRows(R, D, out_dim, hidden, bottleneck, dev, save=True, act=act)
            self.pr_t = PatchRows(R, D, out_dim, hidden, bottleneck, dev, save=False, act=act)
            self.ibot = torch.zeros(1, dtype=f32, device=dev)
            self.patch_center = torch.zeros(out_dim, dtype=f32, device=dev)
            # [K + 1]: the teacher's column sums and, in the last slot, the row count -- one vector through the all-reduce
            self.patch_center_sum = torch.zeros(out_dim + 1, dtype=f32, device=dev)
            self.ibot_ws = _empty((_ws_bytes("gv_ibot_loss_workspace_bytes", R, out_dim) // 4,), f32, dev)
        self.gnorm_sq = torch.zeros(1, dtype=f32, device=dev)
        self.red_ws = _empty((1024,), f32, dev)
        self.hyper = torch.zeros(L.HYP_COUNT, dtype=f32, device=dev)
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.m_teacher, self.ts, self.tt, self.cm, self.clip = momentum_teacher, student_temp, teacher_temp, center_momentum, clip_grad
        self.train_last_layer = True
        self.t = 0
        self.reducer = reducer if reducer is not None else NoReducer()
        self._n_micro = 1
        self._drop = None             # set_dropout: (p, step seed) of the student's --drop
        self._acc: Dict[torch.Tensor, torch.Tensor] = {}       # running sums of the step's outputs over its micro-batches (accumulate_micro)
        self._plan = None             # gradient all-reduce ranges (dist.reduction_plan), built on first use
        self._events: List[torch.cuda.Event] = []       # the SideStream pool of forward_backward
        # contiguous arena range of every block's weight-decayed matrices (arena order = backward order)
        self._block_range = {}
        for i in range(ARCHS[arch]["depth"]):
            spans = [self.arena.span(n) for n in self.arena.order if n.startswith(f"backbone.blocks.{i}.") and self.arena.off[n] < self.arena.n_decay]
            self._block_range[i] = (min(lo for lo, _ in spans), max(hi for _, hi in spans))

    # ---- parameters ----------------------------------------------------------------
    def _with_mask_token(self, backbone: Dict[str, torch.Tensor], what: str) -> Dict[str, torch.Tensor]:
        """iBOT on, and a state from a run without it: ``mask_token`` starts at zeros (DINOv2's initial value), and says so."""
        if self.ibot_weight > 0 and "mask_token" not in backbone:
            print(f"ibot: the {what} state has no mask_token: it starts at zeros", flush=True)
            backbone = dict(backbone, mask_token=torch.zeros(1, self.D))
        elif self.ibot_weight == 0 and "mask_token" in backbone:
            print(f"the {what} state holds iBOT's mask_token, this run has no iBOT term (ibot_weight 0): mask_token is dropped", flush=True)
        return backbone

    def load_state(self, backbone: Dict[str, torch.Tensor], head: Dict[str, torch.Tensor]):
        backbone = self._with_mask_token(backbone, "student")
        self.arena.load(_prefixed(backbone, head))
        self.arena.t.copy_(self.arena.p)            # teacher starts as a copy of the student
        self.refresh_bf16()

    def load_teacher_state(self, backbone: Dict[str, torch.Tensor], head: Dict[str, torch.Tensor], center: Optional[torch.Tensor] = None):
        """Restore the EMA teacher (and the centre) of a saved run: without it a resumed run would restart the
        teacher from the student while the momentum schedule is already near 1."""
        self.arena.load(_prefixed(self._with_mask_token(backbone, "teacher"), head), self.arena.t)
        if center is not None:
            self.center.copy_(center.to(self.center.device, f32).view(-1))
        self.refresh_bf16()

    def refresh_bf16(self):
        a = self.arena
        ops.cast_bf16(a.p, a.pb); ops.cast_bf16(a.t, a.tb)
        self._refresh_wn()

    def _refresh_wn(self):
        bt = self.head.bott
        ops.weightnorm_fwd(self.sH.f("last_layer.weight_v"), self.sH.f("last_layer.weight_g").view(-1), self.wn_s, self.K, bt)
        ops.weightnorm_fwd(self.tH.f("last_layer.weight_v"), self.tH.f("last_layer.weight_g").view(-1), self.wn_t, self.K, bt)

    def backbone_state_dict(self, teacher: bool = False):
        return self.arena.state_dict(self.arena.t if teacher else self.arena.p, "backbone.")

    def head_state_dict(self, teacher: bool = False):
        return self.arena.state_dict(self.arena.t if teacher else self.arena.p, "head.")

    # ---- the step --------------------------------------------------------------------
    def set_drop_path(self, per_img: Optional[torch.Tensor]):
        """Stochastic depth for the STUDENT's next steps (the teacher runs without, as in DINO): f32 [depth, 2, V * B] on the
        device, keep / (1 - p) per crop image (global crops first, crop-major like the feature rows), or None."""
        self.g_stu.set_drop(per_img)

    def set_dropout(self, p: float, seed: int = 0):
        """--drop for the STUDENT's next step (the teacher runs in eval mode): probability and this step's 32-bit seed; p = 0 switches it off.
        Under gradient accumulation every micro-batch of the step derives its own seed from this one (forward_backward)."""
        if p and self.ibot_weight > 0:
            raise ValueError("--drop with the iBOT term is not built (ibot_weight > 0)")
        self._drop = (float(p), int(seed) & 0xFFFFFFFF) if p else None
        self.g_stu.set_dropout(p, seed)

    def set_hyper(self, lr=None, wd=None, momentum_teacher=None, teacher_temp=None, n_micro: int = 1):
        """Put the per-step schedule values into the device hyper vector with a tiny stream-ordered
        kernel whose ARGUMENTS carry them.  Not a memcpy: the host runs several steps ahead of the
        GPU, and a pinned staging buffer would be rewritten before the queued steps consumed it."""
        self.t += 1
        vals = [0.0] * L.HYP_COUNT
        vals[L.HYP_LR] = self.lr if lr is None else lr
        vals[L.HYP_WD] = self.wd if wd is None else wd
        vals[L.HYP_BC1] = 1.0 - self.betas[0] ** self.t
        vals[L.HYP_BC2] = 1.0 - self.betas[1] ** self.t
        vals[L.HYP_TEACHER_MOM] = self._cur_mom = self.m_teacher if momentum_teacher is None else momentum_teacher
        vals[L.HYP_GRAD_SCALE] = 1.0 / (self.reducer.world * n_micro)
        vals[L.HYP_TEACHER_TEMP] = self.tt if teacher_temp is None else teacher_temp
        vals[L.HYP_STUDENT_TEMP] = self.ts
        ops.store_f32(self.hyper, vals)

    def forward_backward(self, tiles_u8: torch.Tensor, micro: Tuple[int, int] = (0, 1), boxes=None, fill=None, views=None, masks=None, stains=None):
        """teacher fwd (global crops) -> student fwd (all crops) -> loss -> backward.
        Leaves gradients in arena.g, loss in self.loss, center_sum.  ``micro = (j, n)``: this is
        micro-batch j of n (gradient accumulation): gradients, loss and centre sums add up over
        the n calls and the data-parallel reduction is issued from the last one only.
        ``views``: (global, local) packed per-crop records of multicrop.ViewAugmentSampler.sample -- with ``boxes``, every crop
        gets its own colour jitter / grayscale / blur / solarisation in the pass that cuts it (gv_crop_augment).
        ``stains``: (global, local) packed per-crop records of stain.StainJitterSampler.sample -- with ``views``, every crop's
        H&E stain jitter is applied in that same pass, ahead of the view chain (gv_crop_augment_stain).
        ``tiles_u8``: uint8 [B, tile, tile, 3] or float32 NCHW [B, 3, tile, tile] already normalised (engine.input_form): float
        input runs the fixed crop windows only (no ``boxes`` / ``views`` / ``stains`` / ``fill``).
        ``masks``: this micro-batch's gipvit.masking.MaskPlan over the G * B global crops (crop-major, like the feature rows) --
        given exactly when ``ibot_weight`` > 0."""
        B, G, V = self.B, self.G, self.V
        self._check_step(tiles_u8, boxes, fill, views, masks, stains)
        M = 0 if masks is None else masks.M
        patch_t, patch_s = (None, None) if masks is None else ((masks, self.pr_t), (masks, self.pr_s))
        mj, mn = micro
        first, last = mj == 0, mj == mn - 1
        if mn > 1 and self._drop:      # micro-batches of one step must not share their dropout masks
            self.g_stu.set_dropout(self._drop[0], ops.dropout_site_seed(self._drop[1], 15, mj))
        t_src, t_win, s_src, s_win = self._cut_crops(tiles_u8, boxes, views, stains)
        sx = SideStream(self.vit.side if tiles_u8.is_cuda else None, self._events)

        def fills():
            # fills nothing in the forward depends on (the gradient arena, the backward's zero-initialised scratch): on the side
            # stream, beside the forward pass (without one, the backward zeroes its scratch when it starts)
            if first:
                self.arena.g.zero_()
            if sx.side is not None:
                self.vit.prepare_backward(self.g_stu)

        # the teacher's forward shares nothing with the student's until the loss: it runs on the
        # side stream beside the student forward (fills the tail of each other's kernels)
        t_side = sx.side is not None and self.sw.teacher_side

        def teacher():
            self.vit.forward(self.tW, self.g_teach, t_src, t_win, self.mean, self.std, self.hb_t.feats, fill=fill, on_side=t_side, patch=patch_t)
            self.head.forward(self.tH, self.wn_t, self.hb_t, on_side=t_side)
            if M > 0:
                self.head.forward(self.tH, self.wn_t, self.pr_t.hb, on_side=t_side, rows=M)
        ev_zero = sx.run(fills)
        ev_teacher = sx.run(teacher) if t_side else teacher()
        self.vit.forward(self.sW, self.g_stu, s_src, s_win, self.mean, self.std, self.hb_s.feats, fill=fill, masks=masks, patch=patch_s)
        if self.koleo_weight > 0:
            ops.koleo_fwd(self.hb_s.feats, self.koleo_ws, self.koleo_nn, self.koleo, G, B, self.D)
        self.head.forward(self.sH, self.wn_s, self.hb_s)
        if M > 0:
            self.head.forward(self.sH, self.wn_s, self.pr_s.hb, rows=M)
        sx.join(ev_teacher)
        center = self.center if self.centering == "center" else self._sinkhorn()
        ops.dino_loss(self.hb_s.logits, self.hb_t.logits, center, self.hb_s.dlogits, self.loss, self.center_sum,
                      self.loss_ws, B, V, G, self.K, self.ts, self.tt, hyper=self.hyper, loss_scale=self.loss_scale)
        if masks is not None:
            if M > 0:
                ops.ibot_loss(self.pr_s.hb.logits, self.pr_t.hb.logits, self.patch_center, masks.weight, self.pr_s.hb.dlogits, self.ibot,
                              self.patch_center_sum, self.ibot_ws, M, self.K, self.ts, self.tt, self.ibot_weight, hyper=self.hyper,
                              loss_scale=self.loss_scale)
            else:       # no marked patch on this rank: no patch launch, the term is 0 and the rank adds nothing to the centre
                self.ibot.zero_(); self.patch_center_sum.zero_()
            # the mean over the micro-batches like the loss; sums and count add up like the CLS centre's
            accumulate_micro(self._acc, ((self.ibot, True), (self.patch_center_sum, False)), mj, mn)
            if last:
                self.reducer.reduce_tensor(self.patch_center_sum)
        accumulate_micro(self._acc, ((self.loss, True), (self.center_sum, False)) + (((self.koleo, True),) if self.koleo_weight > 0 else ()), mj, mn)
        if last:
            self.reducer.reduce_tensor(self.center_sum)
        sx.join(ev_zero)
        self.head.backward(self.sH, self.wn_s, self.hb_s, self.train_last_layer, sx)
        if M > 0:       # the marked rows through the same head: its weight gradients accumulate behind the CLS rows'
            self.head.backward(self.sH, self.wn_s, self.pr_s.hb, self.train_last_layer, sx, rows=M)
        if self.koleo_weight > 0:       # into the global crops' rows of the feature gradient, under the loss scale the DINO term carries
            ops.koleo_bwd(self.hb_s.dfeats, self.koleo_ws, self.koleo_nn, G, B, self.D, self.koleo_weight, loss_scale=self.loss_scale)
        # The gradient all-reduce goes out as a few contiguous arena ranges, each as soon as it is final (dist.reduction_plan):
        # the head's matrices when the head backward ends, then coalesced block ranges of >= 25 MB from the side stream (the
        # block's weight gradients are produced there), then block 0 + patch embed + the no-decay tail as ONE message when
        # backward ends -- RCCL's stream runs beside the remaining backward (reference: NativeDDP's buckets, train.py:634, 1071)
        if last:        # (before the last micro-batch gradients keep accumulating locally)
            sx.then(lambda: self._release("head"))     # behind the head's weight gradients, which were queued on the side stream
        self.vit.backward(self.sW, self.g_stu, self.hb_s.dfeats, on_block_done=self._release if last else None, patch=patch_s)
        if last:
            self._release("end")
            self.reducer.finish()

    def _check_step(self, tiles_u8, boxes, fill, views, masks, stains):
        """Everything ``forward_backward`` refuses, raised before its first launch."""
        self.vit.require_trainable(self.g_stu)
        if (masks is not None) != (self.ibot_weight > 0):
            raise ValueError("masks= goes with ibot_weight > 0: " + ("this engine was built without the iBOT term" if masks is not None else
                                                                       "an engine with the iBOT term needs a MaskPlan for every micro-batch"))
        if masks is not None:
            masks_fit(masks, self.g_stu.segs[0], self.pr_s)
        input_form(tiles_u8, self.B, (self.tile, self.tile), (("fill", fill), ("boxes", boxes), ("views", views), ("stains", stains)))
        if boxes is not None and fill is not None:
            raise ValueError("fill boxes are tile coordinates: they cannot be combined with re-cut random crops (boxes)")
        if views is not None and boxes is None:
            raise ValueError("views (per-crop augmentation draws) need boxes: the views are produced by the pass that cuts the crops")
        if stains is not None and views is None:
            raise ValueError("stains (per-crop stain jitter draws) need views: the jitter runs inside the view-augmentation pass")
        if boxes is not None:
            bg, bl = boxes
            assert bg.shape[0] == self.G * self.B and (self.V == self.G or bl.shape[0] == (self.V - self.G) * self.B)

    def _cut_crops(self, tiles_u8, boxes, views, stains):
        """-> (t_src, t_win, s_src, s_win), the sources and windows of the teacher's and the student's ``VitRunner.forward``: the
        tiles under the fixed windows, or with ``boxes`` the crops cut here."""
        if boxes is None:
            return tiles_u8, [self.gwins], tiles_u8, self.s_wins
        # random-resized crops (multicrop.MultiCropSampler): cut on the device, then every crop is its own
        # "tile" with the single window (0, 0); rows stay crop-major like the fixed windows
        B, n_local = self.B, self.V - self.G
        if self._gcrops is None:
            self._gcrops = _empty((self.G * B, self.gsize, self.gsize, 3), torch.uint8, self.dev)
            self._lcrops = _empty((n_local * B, self.lsize, self.lsize, 3), torch.uint8, self.dev) if n_local else None
        if views is not None and self._vstats is None:
            self._vstats = torch.zeros(max(self.G, n_local) * B, dtype=torch.int64, device=self.dev)

        def cut(k, size, out):      # crop group k (0 global, 1 local): plain, with every crop's view chain, or with its stain jitter ahead of that
            if views is None:
                ops.crop_resize(tiles_u8, boxes[k], size, out=out)
            elif stains is None:
                ops.crop_augment(tiles_u8, boxes[k], views[k], self._vstats, size, out=out)
            else:
                ops.crop_augment_stain(tiles_u8, boxes[k], views[k], stains[k], self._vstats, size, out=out)
            return out
        crops = [cut(0, self.gsize, self._gcrops)] + ([cut(1, self.lsize, self._lcrops)] if n_local else [])
        return crops[0], [[(0, 0)]], crops, [[(0, 0)]] * len(crops)

    def _release(self, trigger):
        """Queue the all-reduce of the plan's ranges that ``trigger`` ("head", a block number, "end") completes."""
        if self.reducer.world > 1 or getattr(self.reducer, "always", False):
            for trg, lo, hi in self._reduction_plan():
                if trg == trigger:
                    self.reducer.reduce_range(self.arena.g, lo, hi)

    def _sinkhorn(self) -> torch.Tensor:
        """Sinkhorn-Knopp centring of this step's teacher logits (include/gipvit.h), 2 n + 1 calls (4 n + 1 kernel launches) on the
        main stream: the shift is the maximum and every column pass the sum over all ranks.  -> ``sk_center``, the loss's centre."""
        R, n = self.G * self.B, self.sinkhorn_iters
        state = (self.hb_t.logits, self.sk_shift, self.sk_a, self.sk_b, self.sk_colsum, self.sk_ws)
        ops.sinkhorn_shift(*state, R, self.K, self.tt, hyper=self.hyper)
        self.reducer.reduce_max(self.sk_shift)
        self.reducer.finish()
        for it in range(n):
            ops.sinkhorn_cols(*state, R, self.K, self.tt, hyper=self.hyper, first=it == 0)
            self.reducer.reduce_tensor(self.sk_colsum)
            self.reducer.finish()
            if it < n - 1:
                ops.sinkhorn_rows(*state, R, self.K, self.tt, hyper=self.hyper, first=it == 0)
        ops.sinkhorn_finish(*state, self.sk_center, R, self.K, self.tt, hyper=self.hyper, first=n == 1)
        return self.sk_center

    def _reduction_plan(self):
        if self._plan is None:
            from .dist import reduction_plan
            a = self.arena
            head_names = [n for n in a.order if n.startswith("head.") and a.off[n] < a.n_decay]
            head_span = (min(a.off[n] for n in head_names), max(a.span(n)[1] for n in head_names)) if head_names else None
            self._plan = reduction_plan(head_span, self._block_range, a.n, bucket_bytes=self.sw.bucket_mb << 20)
        return self._plan

    def optimizer_step(self):
        a = self.arena
        kw = dict(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, step=max(self.t, 1), hyper=self.hyper, **self._clip_args())
        lo = 0
        if not self.train_last_layer:
            # the head's last layer is frozen for the first epochs (DINO cancel_gradients_last_layer sets its grad to
            # None, so the optimizer SKIPS it: no decay, no moment update) -- only the teacher EMA runs over its range
            lo, hi = a.span("head.last_layer.weight_v")
            assert lo == 0, "the last layer opens the arena (backward-completion order)"
            sl = slice(lo, hi)
            ops.adamw_ema(a.p[sl], a.g[sl], a.m[sl], a.v[sl], a.pb[sl], a.t[sl], a.tb[sl], hi - lo, lr=0.0, beta1=self.betas[0],
                          beta2=self.betas[1], eps=self.eps, weight_decay=0.0, step=1, hyper=self.hyper, mode=3)
            lo = hi
        sl = slice(lo, a.n_decay)
        ops.adamw_ema(a.p[sl], a.g[sl], a.m[sl], a.v[sl], a.pb[sl], a.t[sl], a.tb[sl], a.n_decay - lo, weight_decay=1.0, **kw)
        if a.n > a.n_decay:   # biases / LN / pos / cls: same schedules, weight-decay multiplier 0
            sl = slice(a.n_decay, a.n)
            ops.adamw_ema(a.p[sl], a.g[sl], a.m[sl], a.v[sl], a.pb[sl], a.t[sl], a.tb[sl], a.n - a.n_decay, weight_decay=0.0, **kw)
        if self.scaler is not None:
            self.scaler.update(self.gnorm_sq)
        self._refresh_wn()
        ops.center_update(self.center, self.center_sum, self.K, self.cm, 1.0 / (self.G * self.B * self.reducer.world * self._n_micro))
        if self.ibot_weight > 0:      # the patch centre, where the CLS centre is updated; the count comes with the sums
            ops.patch_center_update(self.patch_center, self.patch_center_sum, self.K, self.cm)

    def step_micro(self, tile_batches: Sequence[torch.Tensor], masks=None, **sched) -> torch.Tensor:
        """One optimizer step over ``len(tile_batches)`` micro-batches of B tiles each (gradient
        accumulation; BASELINE config 5 reaches 512 tiles per GPU this way).  Equals ``step`` on the
        concatenated batch up to summation order."""
        n = len(tile_batches)
        if masks is not None and len(masks) != n:
            raise ValueError(f"masks: one MaskPlan per micro-batch ({n}), got {len(masks)}")
        self.set_hyper(n_micro=n, **sched)
        for j, tb in enumerate(tile_batches):
            if input_form(tb, self.B, (self.tile, self.tile)) == "u8":
                assert tb.shape == (self.B, self.tile, self.tile, 3)
            self.forward_backward(tb, micro=(j, n), masks=None if masks is None else masks[j])
        self._n_micro = n
        try:
            self.optimizer_step()
        finally:
            self._n_micro = 1
        return self.loss

    def step(self, tiles_u8: torch.Tensor, boxes=None, fill=None, views=None, masks=None, stains=None, **sched) -> torch.Tensor:
        """One full training step on [B, tile, tile, 3] uint8 NHWC tiles (or float32 NCHW [B, 3, tile, tile] already normalised,
        on the fixed windows).  Returns the (device, un-synchronised) loss tensor.  ``boxes``: (global, local) int32 device tensors
        from multicrop.MultiCropSampler.sample -- random-resized crops instead of the fixed parity windows; ``views`` / ``stains``:
        the per-crop augmentation records of forward_backward."""
        if input_form(tiles_u8, self.B, (self.tile, self.tile), (("fill", fill), ("boxes", boxes), ("views", views), ("stains", stains))) == "u8":
            assert tiles_u8.shape == (self.B, self.tile, self.tile, 3)
        self.set_hyper(**sched)
        self.forward_backward(tiles_u8, boxes=boxes, fill=fill, views=views, masks=masks, stains=stains)
        self.optimizer_step()
        return self.loss


# --------------------------------------------------------------------------- #
# supervised single-crop step (reference train.py:1044-1078; BASELINE config 1)
# --------------------------------------------------------------------------- #
class SupervisedEngine(TrainEngine):
    """ViT + Linear head, softmax -> LabelSmoothingCE (the reference's actual loss path); with a mix plan (gipvit.mixup) the batch
    is mixed inside the patchify pass and the loss is SoftTargetCE / BCE on the mixup target (train.py:832-842, 1037-1040)."""

    def __init__(self, arch="vit_tiny", img_size=64, num_classes=2, batch=8, lr=1e-3, weight_decay=0.0, betas=(0.9, 0.999),
                 eps=1e-8, smoothing=0.1, clip_grad: float = 0.0, mean=MEAN_RON, std=STD_RON, device="cuda:0", reducer=None,
                 opt: str = "adamw", momentum: float = 0.9, train_backbone: bool = True, model_ema_decay: Optional[float] = None,
                 precision: str = "bf16", clip_mode: str = "norm", loss: str = "lsce", bce_target_thresh: Optional[float] = None,
                 layer_decay: Optional[float] = None, global_pool: Optional[str] = "token", long_seq: bool = False):
        """``long_seq``: images past GV_ATTN_MAX_N tokens (above 256 px) may be trained on: the attention backward streams
        (gv_attention_bwd_stream, up to 512 px).  An engine at a smaller image launches exactly what it does without it.
        ``global_pool`` (train.py:122 --gp -> create_model, train.py:490): "token" (None: the same) = the CLS token through the
        final norm; "avg" = timm's mean-pooled model: no final norm, the mean of the patch tokens through ``fc_norm``, so
        ``feats`` is the pooled, normalised feature and the last block runs on every token (gv_token_mean_fwd / _bwd).
        ``precision``: "bf16" (the training path: bf16 GEMM / attention operands, f32 accumulation and residual stream) or
        "fp32" (the reference's default arithmetic: every operand f32, csrc/f32path.hip -- the mode the 1e-4 parity gates
        of SURVEY 8d are stated for; an order of magnitude slower, kept for verification).
        ``loss`` (train.py:832-842): "lsce" LabelSmoothingCrossEntropy (gv_softmax_lsce, the default path), "soft_ce" timm
        SoftTargetCrossEntropy or "bce" timm BinaryCrossEntropy (``bce_target_thresh``: its target_threshold) on the mixup
        target of the step's ``mix`` plan (gv_softmax_mix_loss); ``smoothing`` goes into that target.
        ``layer_decay`` (train.py:175 --layer-decay -> timm param_groups_layer_decay, restated in gipvit.layer_decay): None = one
        rate for every layer, the two-launch optimizer pass.  A number (1.0 included) gives layer ``id`` the rate
        ``lr * layer_decay ** (depth + 2 - id)`` and makes ``optimizer_step`` ONE gv_adamw_ema_ranges launch over a range table
        (adamw / adam / sgd) or hands gv_lamb a per-tensor rate; ``layer_scales`` / ``mean_lr`` show the result."""
        self.pool = resolve_pool(global_pool)
        self.long_seq = check_long_seq(long_seq, precision, (img_size,))
        if loss not in ("lsce", "soft_ce", "bce"):
            raise ValueError(f"loss {loss!r}: 'lsce', 'soft_ce' or 'bce' (train.py:832-842)")
        if bce_target_thresh is not None and loss != "bce":
            raise ValueError("bce_target_thresh goes with loss='bce' (timm BinaryCrossEntropy's target_threshold)")
        self.loss_kind, self.bce_target_thresh = loss, bce_target_thresh
        if clip_mode == "value" and opt == "lamb":
            raise ValueError("--clip-mode value with --opt lamb is not built (Lamb's own global-norm clip needs the norm of the clamped gradient)")
        dev = torch.device(device)
        fp32, act = self._set_modes(precision, clip_mode, ("norm", "value", "agc"), dev)
        if self.scaler is not None and (opt == "lamb" or clip_mode == "agc"):
            raise ValueError("float16 loss scaling is built for adamw / adam / sgd with --clip-mode norm | value; "
                             "--opt lamb and --clip-mode agc run with --amp-dtype bfloat16")
        self.dev, self.arch, self.B, self.img, self.C = dev, arch, batch, img_size, num_classes
        D = ARCHS[arch]["embed_dim"]
        self.D = D
        self.mean, self.std = tuple(mean), tuple(std)
        # --model-ema (train.py:615-622, ModelEmaV2): the EMA copy lives in the arena's teacher slot and is
        # updated by the same fused optimizer pass (train.py:1080-1081)
        self.ema_decay = model_ema_decay
        self.arena = Arena(vit_param_specs(arch, img_size, num_classes, self.pool), dev, teacher=model_ema_decay is not None)
        self.W = Weights(self.arena, "", fp32=fp32)
        self.Wema = Weights(self.arena, "", teacher=True, fp32=fp32) if model_ema_decay is not None else None
        self.vit = VitRunner(arch, img_size, dev, fp32=fp32)
        self.grp = VitGroup(arch, [(batch, img_size)], img_size, dev, save=True, act=act, pool=self.pool, stream_bwd=self.long_seq)
        e = lambda shape, dt: _empty(shape, dt, dev)
        self.feats, self.dfeats = e((batch, D), act), e((batch, D), act)
        self.logits, self.dlogits, self.prob = e((batch, num_classes), f32), e((batch, num_classes), f32), e((batch, num_classes), f32)
        self.loss = torch.zeros(1, dtype=f32, device=dev)
        self.ones = torch.ones(batch, dtype=f32, device=dev)
        self.gnorm_sq = torch.zeros(1, dtype=f32, device=dev)
        self.red_ws = _empty((1024,), f32, dev)
        self.lr, self.wd, self.betas, self.eps, self.smoothing, self.clip = lr, weight_decay, betas, eps, smoothing, clip_grad
        self.t = 0
        self.reducer = reducer if reducer is not None else NoReducer()
        if opt not in ("adamw", "adam", "sgd", "lamb"):
            raise ValueError(f"--opt {opt}: this build fuses adamw / adam / sgd (nesterov) / lamb only")
        self.opt = opt
        self.opt_mode = {"adamw": 0, "adam": 1, "sgd": 2, "lamb": -1}[opt]
        if opt == "sgd":
            self.betas = (momentum, betas[1])
        if clip_mode == "agc" and clip_grad > 0:
            # adaptive gradient clipping (timm adaptive_clip_grad; the reference excludes the classifier: model_parameters(exclude_head=True))
            a = self.arena
            self._agc_units = ops.agc_units([(a.off[n], a.specs[n]) for n in a.order if not n.startswith("head.")]).to(dev)
        if opt == "lamb":
            # timm.optim.Lamb (reference train.py:161, 583): per-tensor trust ratio -> every tensor's norms are needed before its
            # update: two launches per arena segment over a block table that never crosses a tensor (gv_lamb)
            a = self.arena
            self._lamb_names = list(a.order)
            spans = [a.span(n) for n in self._lamb_names]
            self._lamb_tab = ops.lamb_block_table(spans).to(dev)
            self._lamb_decay = torch.tensor([0.0 if no_weight_decay(n, a.specs[n]) else 1.0 for n in self._lamb_names])
            # decayed tensors open the arena (Arena layout): two sub-tables, one per weight-decay value
            nd = sum(1 for n in self._lamb_names if not no_weight_decay(n, a.specs[n]))
            tid = self._lamb_tab[:, 0]
            self._lamb_tabs = (self._lamb_tab[tid < nd].contiguous(), self._lamb_tab[tid >= nd].contiguous())
            self._lamb_stats = torch.zeros(2 * len(self._lamb_names), dtype=f32, device=dev)
            self.lamb_max_grad_norm = 1.0          # timm Lamb default
        self.train_backbone = train_backbone      # False = --no-grad head-only fine-tune (train.py:497-503)
        self.layer_decay = layer_decay
        if layer_decay is not None:
            # built once for both settings of train_backbone (the driver's model object may flip it after construction):
            # the whole arena, and the classifier's two tensors alone (the optimizer never sees a frozen parameter)
            a, depth = self.arena, ARCHS[arch]["depth"]
            plans = {True: LayerDecayPlan(a, depth, layer_decay), False: LayerDecayPlan(a, depth, layer_decay, names=("head.weight", "head.bias"))}
            self._ld = {k: (pl, pl.block_table().to(dev), pl.range_rows().to(dev)) for k, pl in plans.items()}
            if opt == "lamb":
                self._lamb_lr_scale = torch.tensor([plans[True].scales[n] for n in self._lamb_names], dtype=f32).to(dev)

    @property
    def layer_scales(self) -> Optional[Dict[str, float]]:
        """--layer-decay: name -> rate scale of every parameter the optimizer steps (None without the flag)."""
        return None if self.layer_decay is None else dict(self._ld[bool(self.train_backbone)][0].scales)

    def mean_lr(self, lr: float) -> float:
        """The rate the reference logs for a scheduled rate ``lr``: the mean over the optimizer's parameter groups (train.py:1088-1089,
        959-965) -- with --layer-decay ``lr`` times the mean scale of the (layer, decay) groups that hold a trainable parameter,
        else ``lr`` itself."""
        return lr if self.layer_decay is None else self._ld[bool(self.train_backbone)][0].mean_lr(lr)

    def load_state(self, state: Dict[str, torch.Tensor], ema_state: Optional[Dict[str, torch.Tensor]] = None):
        self.arena.load(state)
        ops.cast_bf16(self.arena.p, self.arena.pb)
        if self.arena.t is not None:       # ModelEmaV2 starts as a deep copy of the model; a resumed run restores it
            if ema_state is not None:
                self.arena.load(ema_state, self.arena.t)
            else:
                self.arena.t.copy_(self.arena.p)
            ops.cast_bf16(self.arena.t, self.arena.tb)

    def state_dict(self, ema: bool = False):
        return self.arena.state_dict(self.arena.t if ema else None)

    def set_drop_path(self, per_img: Optional[torch.Tensor]):
        """Stochastic depth (--drop-path) for the next training steps: f32 [depth, 2, batch] on the device = keep / (1 - p)
        per image and residual branch, or None (evaluation: ``forward`` with it set would scale the branches too)."""
        self.grp.set_drop(per_img)

    def set_dropout(self, p: float, seed: int = 0):
        """--drop for the next training steps' forward / backward: probability and the step's 32-bit seed (evaluation: p = 0)."""
        self.grp.set_dropout(p, seed)

    def forward(self, tiles_u8, ema: bool = False, fill=None, mix=None):
        """Inference / features: returns (logits f32 [B,C], CLS features bf16 [B,D]); ``ema``: with the EMA weights.
        ``tiles_u8``: uint8 NHWC [B, H, W, 3] or float32 NCHW [B, 3, H, W] already normalised (engine.input_form); the
        image is its top-left img_size window.  ``mix``: a training step's gipvit.mixup.MixPlan (forward_backward).  Never
        erases: random erasing belongs to the training step alone."""
        return self._forward(tiles_u8, ema, fill, mix, None)

    def _forward(self, tiles_u8, ema, fill, mix, erase):
        B, C, D, W = self.B, self.C, self.D, (self.Wema if ema else self.W)
        input_form(tiles_u8, B, None, (("fill", fill),))
        self.vit.forward(W, self.grp, tiles_u8, [[(0, 0)]], self.mean, self.std, self.feats, fill=fill, mix=None if mix is None else mix.table,
                         erase=None if erase is None else (erase.table, erase.seed))
        ops.small_matmul(self.feats, W.f("head.weight"), self.logits, B, C, D, sam=D, sak=1, sbk=1, sbn=D, bias=W.f("head.bias"))
        return self.logits, self.feats

    def forward_backward(self, tiles_u8, target, fill=None, mix=None, erase=None):
        """``mix``: this step's gipvit.mixup.MixPlan (on the device) or None.  With a plan the batch is mixed inside the patchify
        pass and the loss takes the plan's partner / lam (train.py:1037-1040); ``self.prob`` is the softmax of the MIXED batch.
        ``erase``: this step's gipvit.erasing.ErasePlan (on the device) or None: random erasing of the normalised batch inside the
        same pass, after ``fill`` and ``mix`` (timm's prefetcher order); the labels and every loss are unchanged by it."""
        B, C, D, W = self.B, self.C, self.D, self.W
        if mix is not None and self.loss_kind == "lsce":
            raise ValueError("mix= needs loss='soft_ce' or 'bce': label-smoothing cross-entropy takes hard labels (train.py:832-842)")
        self.vit.require_trainable(self.grp)
        self.arena.g.zero_()
        self._forward(tiles_u8, False, fill, mix, erase)
        if self.loss_kind == "lsce":
            ops.softmax_lsce(self.logits, target.view(-1), self.loss, self.dlogits, self.prob, B, C, self.smoothing, loss_scale=self.loss_scale)
        else:
            ops.softmax_mix_loss(self.logits, target.view(-1), self.loss, self.dlogits, self.prob, B, C, self.smoothing, self.loss_kind,
                                 partner=None if mix is None else mix.partner, lam=None if mix is None else mix.lam,
                                 threshold=self.bce_target_thresh, loss_scale=self.loss_scale)
        # head backward: dW = dlogits^T f, db = colsum(dlogits), df = dlogits W
        ops.small_matmul(self.dlogits, self.feats, W.g("head.weight"), C, D, B, sam=1, sak=C, sbk=D, sbn=1, accumulate=True)
        ops.small_matmul(self.ones, self.dlogits, W.g("head.bias").view(1, C), 1, C, B, sam=0, sak=1, sbk=C, sbn=1, accumulate=True)
        ops.small_matmul(self.dlogits, W.f("head.weight"), self.dfeats, B, D, C, sam=C, sak=1, sbk=D, sbn=1)
        if self.train_backbone:
            self.vit.backward(W, self.grp, self.dfeats)
        self.reducer.reduce_range(self.arena.g, 0, self.arena.n)
        self.reducer.finish()

    def optimizer_step(self, lr=None):
        a = self.arena
        self.t += 1
        if self.clip > 0 and self.clip_mode == "agc":
            ops.agc(a.p, a.g, self._agc_units, self.clip, 1e-3, 1.0 / self.reducer.world)
        kw = dict(lr=self.lr if lr is None else lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, step=self.t,
                  grad_scale=1.0 / self.reducer.world, mode=self.opt_mode, teacher_momentum=self.ema_decay or 0.0, **self._clip_args())
        tt = (lambda sl: (a.t[sl], a.tb[sl])) if a.t is not None else (lambda sl: (None, None))
        if self.opt_mode < 0:
            if not self.train_backbone:
                raise ValueError("--opt lamb with --no-grad (head-only fine-tune) is not built: use adamw / adam / sgd")
            ops.sumsq(a.g, self.red_ws, self.gnorm_sq)              # Lamb clips by the global norm itself (max_grad_norm = 1)
            self._lamb_stats.zero_()
            kl = dict(lr=kw["lr"], beta1=kw["beta1"], beta2=kw["beta2"], eps=self.eps, step=self.t, grad_scale=kw["grad_scale"],
                      clip_norm=kw["clip_norm"], max_grad_norm=self.lamb_max_grad_norm, teacher_momentum=self.ema_decay or 0.0)
            for phase in (0, 1):
                for tab, wd in zip(self._lamb_tabs, (self.wd, 0.0)):
                    if tab.shape[0]:
                        ops.lamb(a.p, a.g, a.m, a.v, a.pb, a.t, a.tb, tab, self._lamb_stats, self.gnorm_sq, phase=phase, weight_decay=wd,
                                 lr_scale=self._lamb_lr_scale if self.layer_decay is not None else None, **kl)
            return
        if self.layer_decay is not None:
            # --layer-decay: every (layer, decay | no-decay) range at its own rate, one launch (gv_adamw_ema_ranges)
            _, blocks, rows = self._ld[bool(self.train_backbone)]
            ops.adamw_ema_ranges(a.p, a.g, a.m, a.v, a.pb, a.t, a.tb, a.n, blocks, rows, weight_decay=self.wd, **kw)
            if self.scaler is not None:
                self.scaler.update(self.gnorm_sq)
            return
        if self.train_backbone:
            ranges = [(0, a.n_decay, self.wd), (a.n_decay, a.n, 0.0)]
        else:
            # --no-grad (train.py:497-503): the encoder has requires_grad=False, so the optimizer never sees it -- no
            # weight decay, no moments; only the classifier's two tensors are stepped (the EMA of the frozen part
            # stays equal to the model it was copied from)
            ranges = [a.span("head.weight") + (self.wd,), a.span("head.bias") + (0.0,)]
        for lo, hi, wd in ranges:
            sl = slice(lo, hi)
            ops.adamw_ema(a.p[sl], a.g[sl], a.m[sl], a.v[sl], a.pb[sl], *tt(sl), hi - lo, weight_decay=wd, **kw)
        if self.scaler is not None:
            self.scaler.update(self.gnorm_sq)

    def step(self, tiles_u8, target, lr=None, fill=None, mix=None, erase=None):
        assert target.dtype == torch.int64
        self.forward_backward(tiles_u8, target, fill=fill, mix=mix, erase=erase)
        self.optimizer_step(lr)
        return self.loss


# --------------------------------------------------------------------------- #
# forward-only encoder: slide-level inference / feature extraction
# --------------------------------------------------------------------------- #
class FeatureExtractor:
    """The encoder run forward-only on the same kernels: per-tile CLS features (what the reference's
    ``validate()`` writes to ``<slide>_features.pt``, train.py:1281-1282) and, with a classifier head,
    per-tile logits / positive-class scores (train.py:1186-1343).  Nothing is saved for a backward pass:
    the group rotates three residual buffers and the fc1 epilogue skips the pre-activation store.

    ``weights``: a ``Weights`` view of another engine's arena (student, EMA or DINO teacher) -- the
    extractor then evaluates those live parameters instead of owning a copy (validation between epochs)."""

    def __init__(self, arch="vit_small", img_size=256, batch=256, num_classes=0, mean=MEAN_RON, std=STD_RON, device="cuda:0",
                 weights: Optional[Weights] = None, precision: str = "bf16", global_pool: Optional[str] = "token", long_maps: bool = False):
        """``precision``: as for the engines; with ``weights`` it follows the owning engine's mode.  ``global_pool``: as
        SupervisedEngine's -- "avg" returns the mean of the patch tokens through ``fc_norm`` (the weights must be an avg
        model's); the attention maps do not change with it, ``intermediate_layers`` is refused (no final norm).
        ``long_maps``: ``run_with_attention`` and ``last_selfattention`` also work past GV_ATTN_MAX_N tokens (above 256 px, up to
        512 px), through gv_attention_probs_stream; at or below that limit the keyword changes no launch.  Mind the size of a
        full map: N x N f32 is 4.2 MB per head and tile at 512 px (1 025 tokens; ViT-S: 25 MB per tile) -- ``cls_only`` /
        ``run_with_attention`` return 4.1 KB per head and tile.  precision='fp32' keeps its construction-time limit."""
        self.pool = resolve_pool(global_pool)
        fp32, act = operand_mode(precision)
        if weights is not None:
            fp32, act = weights.fp32, (f32 if weights.fp32 else bf16)
        n_tok = (img_size // 16) ** 2 + 1
        if img_size % 16 or not 16 <= img_size or n_tok > L.GV_ATTN_STREAM_MAX_N:
            raise ValueError(f"img_size {img_size}: a multiple of 16 up to 512 ({L.GV_ATTN_STREAM_MAX_N} tokens, gv_attention_fwd_stream)")
        if fp32 and n_tok > L.GV_ATTN_F32_MAX_N:
            raise ValueError(f"precision='fp32' with img_size {img_size}: {n_tok} tokens per image, the fp32 operand mode's attention "
                             f"stops at {L.GV_ATTN_F32_MAX_N} (256-px images); larger images run in the 16-bit mode")
        dev = torch.device(device)
        self.dev, self.arch, self.B, self.img, self.C = dev, arch, batch, img_size, num_classes
        self.D = ARCHS[arch]["embed_dim"]
        self.mean, self.std = tuple(mean), tuple(std)
        if weights is None:
            self.arena = Arena(vit_param_specs(arch, img_size, num_classes, self.pool), dev, teacher=False)
            self.W = Weights(self.arena, "", fp32=fp32)
        else:
            self.arena, self.W = weights.a, weights
        self.vit = VitRunner(arch, img_size, dev, fp32=fp32)
        self.vit.side = None                       # a forward-only pass has nothing to put on a side stream
        has_fc_norm = self.W.prefix + "fc_norm.weight" in self.arena.specs
        if has_fc_norm != (self.pool == "avg"):
            raise ValueError(f"global_pool={self.pool!r} over the weights of a {'mean-pooled' if has_fc_norm else 'CLS-token'} model")
        self.long_maps = bool(long_maps)
        self.grp = VitGroup(arch, [(batch, img_size)], img_size, dev, save=False, act=act, pool=self.pool, stream_maps=self.long_maps)
        self.feats = _empty((batch, self.D), act, dev)
        self.logits = _empty((batch, num_classes), f32, dev) if num_classes else None
        self._pad: Dict[str, torch.Tensor] = {}          # the zero-padded last batch per input form (_batches)
        self._scratch: Dict[str, torch.Tensor] = {}      # capture buffers of a padded last batch, token statistics (_scratch_buf)
        self._stain = self._stain_buf = None               # set_stain: B copies of the slide's gv_stain_params record, device

    def set_stain(self, record) -> None:
        """Stain normalisation of the current slide (gipvit.stainnorm): ``record`` is ONE gv_stain_params record (the structured
        numpy array of ``stainnorm.normaliser_record`` / ``SlideStain.record``, or its 52 packed bytes as a uint8 tensor).  While
        set, every pass of this extractor (``forward``, ``run``, ``run_with_attention``, ``last_selfattention``,
        ``intermediate_layers``, ``probe_features``; padded last batches and precision="fp32" included) patchifies through
        gv_patchify_stain with the record broadcast over the batch; float32 NCHW input then raises ValueError.  None: off."""
        if record is None:
            self._stain = None
            return
        from .stainnorm import pack_record
        one = record if isinstance(record, torch.Tensor) else pack_record(record)
        if one.dtype != torch.uint8 or one.numel() != ops._STAIN_PARAMS_BYTES:
            raise ValueError(f"set_stain: expected one gv_stain_params record ({ops._STAIN_PARAMS_BYTES} bytes)")
        if self._stain_buf is None:
            self._stain_buf = torch.empty(self.B * ops._STAIN_PARAMS_BYTES, dtype=torch.uint8, device=self.dev)
        self._stain_buf.view(self.B, -1).copy_(one.reshape(1, -1).to(self.dev))
        self._stain = self._stain_buf

    def load_state(self, state: Dict[str, torch.Tensor]):
        if "mask_token" in state:       # an iBOT student / teacher: the token stands in for masked patches in training only
            print("FeatureExtractor: the state holds iBOT's mask_token; inference masks nothing: mask_token is dropped", flush=True)
        self.arena.load(state)
        ops.cast_bf16(self.arena.p, self.arena.pb)

    def forward(self, tiles_u8: torch.Tensor, capture: Optional[Capture] = None):
        """tiles_u8 [B, img, img, 3] u8 NHWC, or float32 NCHW [B, 3, img, img] already normalised -> (CLS features bf16 [B, D],
        logits f32 [B, C] or None).  ``capture``: attention / token outputs of the same pass (``Capture``)."""
        if input_form(tiles_u8, self.B, (self.img, self.img)) == "u8":
            assert tiles_u8.shape == (self.B, self.img, self.img, 3)
        elif self._stain is not None:
            raise ValueError("a stain record is set (set_stain): float32 NCHW input is already normalised and cannot be stain-normalised")
        self.vit.forward(self.W, self.grp, tiles_u8, [[(0, 0)]], self.mean, self.std, self.feats, capture=capture, stain=self._stain)
        if self.C:
            ops.small_matmul(self.feats, self.W.f("head.weight"), self.logits, self.B, self.C, self.D, sam=self.D, sak=1, sbk=1, sbn=self.D,
                             bias=self.W.f("head.bias"))
        return self.feats, self.logits

    def _batches(self, tiles_u8: torch.Tensor):
        """(lo, hi, batch) over any number of tiles: batches of B, the last one padded (its rows >= hi - lo are zeros)."""
        form = input_form(tiles_u8, None, (self.img, self.img))
        n = tiles_u8.shape[0]
        for lo in range(0, n, self.B):
            hi = min(n, lo + self.B)
            part = tiles_u8[lo:hi]
            if hi - lo < self.B:
                if form not in self._pad:
                    shape = (self.B, self.img, self.img, 3) if form == "u8" else (self.B, 3, self.img, self.img)
                    self._pad[form] = torch.zeros(shape, dtype=tiles_u8.dtype, device=self.dev)
                self._pad[form][: hi - lo].copy_(part)
                part = self._pad[form]
            yield lo, hi, part

    def run(self, tiles_u8: torch.Tensor):
        """Any number of tiles (one chunk of a slide, datasets.py:699-700 ``tiles_per_iter``), uint8 NHWC or float32 NCHW as
        ``forward``: batches of B, the last one padded.  -> (features f32 [n, D], logits f32 [n, C] or None), device tensors
        owned by the caller."""
        return self._run(tiles_u8, None)

    def run_with_attention(self, tiles_u8: torch.Tensor):
        """As ``run``, plus the CLS query's attention over every token in the last block, from the same forward (one extra small
        launch per batch) -> (features, logits, attention f32 [n, H, N]).  ``attention[:, :, 1:]`` reshaped to
        (img / 16, img / 16) is DINO's attention map of each head."""
        self._check_size(tiles_u8)
        self.vit.require_attention_maps(self.grp)
        attn = torch.empty(tiles_u8.shape[0], self.vit.H, self.grp.segs[0].N, dtype=f32, device=self.dev)
        return (*self._run(tiles_u8, attn), attn)

    def _run(self, tiles_u8, attn):
        n = tiles_u8.shape[0]
        feats = torch.empty(n, self.D, dtype=f32, device=self.dev)
        logits = torch.empty(n, self.C, dtype=f32, device=self.dev) if self.C else None
        outs = [] if attn is None else [("_cls_attn", attn)]
        for lo, hi, f, l in self._captured(tiles_u8, outs, lambda bufs: Capture(attn=bufs[0], attn_rows=1) if bufs else None):
            feats[lo:hi].copy_(f[: hi - lo])
            if logits is not None:
                logits[lo:hi].copy_(l[: hi - lo])
        return feats, logits

    def _captured(self, tiles_u8, outs, capture):
        """The batched pass of every entry point over any number of tiles.  Per batch (``_batches``): a capture buffer for each (scratch
        name, [n, ...] output) of ``outs`` -- the output's rows themselves when the batch is full, else a B-row scratch --, ``forward`` with
        ``capture(buffers)``, a yield of (lo, hi, features, logits), then the rows of a partial batch copied from the scratch to the outputs."""
        for lo, hi, part in self._batches(tiles_u8):
            full = hi - lo == self.B
            bufs = [out[lo:hi] if full else self._scratch_buf(name, (self.B,) + tuple(out.shape[1:])) for name, out in outs]
            yield (lo, hi) + self.forward(part, capture(bufs))
            if not full:
                for (_, out), b in zip(outs, bufs):
                    out[lo:hi].copy_(b[: hi - lo])

    def _scratch_buf(self, name: str, shape) -> torch.Tensor:
        """The f32 scratch ``name`` of ``shape`` (allocated on first use and kept, again when the shape changes)."""
        buf = self._scratch.get(name)
        if buf is None or tuple(buf.shape) != tuple(shape):
            buf = self._scratch[name] = torch.empty(tuple(shape), dtype=f32, device=self.dev)
        return buf

    def _token_capture(self, bufs) -> Capture:
        """The ``Capture`` of the final norm's tokens into ``bufs`` (f32 [B, N, D] each), with the LayerNorm statistics scratch they share."""
        T = self.grp.T
        return Capture(tokens=[b.view(T, self.D) for b in bufs], stats=self._scratch_buf("_tok_stats", (2, T)))

    def _check_size(self, tiles_u8: torch.Tensor):
        form = input_form(tiles_u8, None, (self.img, self.img))       # (float32 NCHW of another size: ValueError there)
        if form == "u8" and tuple(tiles_u8.shape[1:3]) != (self.img, self.img):
            raise ValueError(f"images: expected {self.img} x {self.img} tiles, got {tuple(tiles_u8.shape[1:3])} (no pos-embed "
                             "interpolation at inference)")

    def last_selfattention(self, tiles_u8: torch.Tensor, cls_only: bool = False) -> torch.Tensor:
        """The reference's get_last_selfattention (vit.pyc@L255-262) over any number of tiles (batched and padded as ``run``):
        the last block's softmax attention f32 [n, H, N, N], or only the CLS query's row, [n, H, 1, N], with ``cls_only``."""
        self._check_size(tiles_u8)
        self.vit.require_attention_maps(self.grp)
        N, H = self.grp.segs[0].N, self.vit.H
        q = 1 if cls_only else N
        out = torch.empty(tiles_u8.shape[0], H, q, N, dtype=f32, device=self.dev)
        for _ in self._captured(tiles_u8, [("_attn_buf", out)], lambda bufs: Capture(attn=bufs[0], attn_rows=q)):
            pass        # (the capture is the output)
        return out

    def intermediate_layers(self, tiles_u8: torch.Tensor, n: int = 1) -> List[torch.Tensor]:
        """The reference's get_intermediate_layers (vit.pyc@L264-272) over any number of tiles: ``norm(x)`` over every token after
        each of the last ``n`` blocks, in block order -- a list of n f32 [n_tiles, N, D].  Not for a global_pool='avg' model."""
        if self.pool == "avg":
            raise ValueError("intermediate_layers: the reference applies the final norm to every token there, and a "
                             "global_pool='avg' model has none (its fc_norm normalises the pooled vector)")
        self._check_size(tiles_u8)
        if not 1 <= n <= self.vit.depth:
            raise ValueError(f"intermediate_layers: n = {n}, need 1 <= n <= depth = {self.vit.depth}")
        outs = [torch.empty(tiles_u8.shape[0], self.grp.segs[0].N, self.D, dtype=f32, device=self.dev) for _ in range(n)]
        for _ in self._captured(tiles_u8, [(f"_tok_buf{k}", o) for k, o in enumerate(outs)], self._token_capture):
            pass        # (the capture is the output)
        return outs

    def probe_features(self, tiles_u8: torch.Tensor, n_last: int = 4, avgpool: bool = False) -> torch.Tensor:
        """The input of DINO's eval_linear over any number of tiles: the CLS rows of ``norm(x)`` after each of the last ``n_last``
        blocks, concatenated in block order, with ``avgpool`` followed by the mean of the last block's normalised patch tokens
        -- f32 [n_tiles, n_last * D (+ D)].  Built on the token capture of ``intermediate_layers`` one batch at a time: the
        scratch is n_last x B x N x D whatever the number of tiles.  Not for a global_pool='avg' model."""
        if self.pool == "avg":
            raise ValueError("probe_features: the probe reads the final norm's tokens, and a global_pool='avg' model has no "
                             "final norm (its fc_norm normalises the pooled vector)")
        self._check_size(tiles_u8)
        if not 1 <= n_last <= self.vit.depth:
            raise ValueError(f"probe_features: n_last = {n_last}, need 1 <= n_last <= depth = {self.vit.depth}")
        N, D, T, B = self.grp.segs[0].N, self.D, self.grp.T, self.B
        out = torch.empty(tiles_u8.shape[0], (n_last + bool(avgpool)) * D, dtype=f32, device=self.dev)
        bufs = [self._scratch_buf(f"_tok_buf{k}", (B, N, D)) for k in range(n_last)]       # (every batch through the scratch: no [n, N, D] output)
        pooled = self._scratch_buf("_probe_pool", (B, D)) if avgpool else None
        for lo, hi, _, _ in self._captured(tiles_u8, [], lambda _: self._token_capture(bufs)):
            for k, b in enumerate(bufs):
                out[lo:hi, k * D:(k + 1) * D].copy_(b[: hi - lo, 0, :])          # the CLS rows: a strided copy
            if avgpool:
                ops.token_mean_fwd(bufs[-1].view(T, D), pooled, B, N, D)
                out[lo:hi, n_last * D:].copy_(pooled[: hi - lo])
        return out
