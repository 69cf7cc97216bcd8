"""Host side of supervised mixup / cutmix (reference train.py:752-771 builds timm's ``Mixup`` from --mixup / --cutmix /
--cutmix-minmax / --mixup-prob / --mixup-switch-prob / --mixup-mode; 1037-1040 applies it): the per-step DRAWS, restated from
timm 0.8.x (``timm/data/mixup.py``: Mixup._params_per_batch / _params_per_elem, rand_bbox, rand_bbox_minmax,
cutmix_bbox_and_lam with correct_lam).  timm is not installed here and the reference does not pin a version: the
restatement is pinned by nothing but itself.  The pixels and the loss are the device's work -- a ``MixPlan`` carries the mix
table of gv_patchify_mix / gv_patchify_nchw_mix and the ``partner`` / ``lam`` vectors of gv_softmax_mix_loss.

Draws come from numpy's ``default_rng`` like the other host streams (timm uses the global numpy state), so the SAME
distributions, not the same numbers.  Order of draws per decision (one per batch, per image, or per pair):
``u < prob`` or no mixing; with both alphas > 0 ``cut = (u < switch_prob)``; ``lam ~ Beta(a, a)`` with the chosen alpha;
then the box of a cutmix decision (centre y, x -- or with min / max: height, width, top, left)."""
from __future__ import annotations

import json
from typing import Optional, Sequence

import numpy as np
import torch

MIX_COPY, MIX_BLEND, MIX_PASTE = 0, 1, 2      # gipvit.h GV_MIX_*
# gv_mix_row (gipvit.h / _lib.gv_mix_row): 32 bytes
ROW_DT = np.dtype([("partner", "<i4"), ("mode", "<i4"), ("lam", "<f4"), ("one_minus_lam", "<f4"),
                   ("yl", "<i4"), ("yh", "<i4"), ("xl", "<i4"), ("xh", "<i4")])
MODES = ("batch", "pair", "elem")


class MixPlan:
    """One step's mixing: ``rows`` (host, ROW_DT [B]) and, once on a device, ``table`` uint8 [B * 32] (the gv_mix_row records),
    ``partner`` int32 [B] and ``lam`` float32 [B] (the weight of each image's own label in the target)."""

    def __init__(self, rows: np.ndarray, device=None):
        assert rows.dtype == ROW_DT and rows.ndim == 1
        self.rows = rows
        self.table = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy())
        self.partner = torch.from_numpy(rows["partner"].astype(np.int32))
        self.lam = torch.from_numpy(rows["lam"].astype(np.float32))
        if device is not None:
            self.table, self.partner, self.lam = (t.to(device, non_blocking=True) for t in (self.table, self.partner, self.lam))

    @staticmethod
    def make_rows(B: int) -> np.ndarray:
        """B copy rows, partner B - 1 - i (timm pairs image i with x.flip(0)[i])."""
        rows = np.zeros(B, ROW_DT)
        rows["partner"] = B - 1 - np.arange(B)
        rows["lam"], rows["one_minus_lam"] = 1.0, 0.0
        return rows

    @staticmethod
    def set_row(rows: np.ndarray, i: int, lam: float, box: Optional[Sequence[int]]):
        """Row i from a decision: ``lam`` the double the sampler drew (after correct_lam for a box); lam == 1 stays a copy row.
        Both weights are rounded here, from the double: the kernels never compute 1 - lam."""
        if lam == 1.0:
            return
        rows["lam"][i], rows["one_minus_lam"][i] = np.float32(lam), np.float32(1.0 - lam)
        if box is None:
            rows["mode"][i] = MIX_BLEND
        else:
            rows["mode"][i] = MIX_PASTE
            rows["yl"][i], rows["yh"][i], rows["xl"][i], rows["xh"][i] = box


class MixSampler:
    """timm ``Mixup``'s draws.  ``sample(device)`` -> MixPlan, or None while ``enabled`` is False (--mixup-off-epoch: no draw
    is consumed then)."""

    def __init__(self, mixup_alpha: float = 1.0, cutmix_alpha: float = 0.0, cutmix_minmax=None, prob: float = 1.0, switch_prob: float = 0.5,
                 mode: str = "batch", batch: int = 8, img_size: int = 224, seed: int = 0):
        if mode not in MODES:
            raise ValueError(f"mixup mode {mode!r}: one of {MODES}")
        if batch < 2 or batch % 2:
            raise ValueError(f"mixup pairs image i with image B - 1 - i: the batch size must be even, got {batch}")
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError("mixup / cutmix alpha must be >= 0")
        if cutmix_minmax is not None:
            if len(cutmix_minmax) != 2:
                raise ValueError(f"cutmix_minmax needs two values (min, max), got {list(cutmix_minmax)}")
            lo, hi = float(cutmix_minmax[0]), float(cutmix_minmax[1])
            if not (0.0 < lo < hi <= 1.0) or int(img_size * lo) >= int(img_size * hi):
                raise ValueError(f"cutmix_minmax {list(cutmix_minmax)}: need 0 < min < max <= 1 with distinct box sizes at {img_size} px")
            cutmix_minmax = (lo, hi)
            cutmix_alpha = 1.0                      # timm: "force cutmix alpha == 1.0 when minmax active"
        if mixup_alpha == 0 and cutmix_alpha == 0:
            raise ValueError("one of mixup_alpha / cutmix_alpha / cutmix_minmax must be set")
        self.mixup_alpha, self.cutmix_alpha, self.minmax = float(mixup_alpha), float(cutmix_alpha), cutmix_minmax
        self.prob, self.switch_prob, self.mode, self.B, self.img = float(prob), float(switch_prob), mode, batch, img_size
        self.rng = np.random.default_rng(seed)
        self.enabled = True

    # ---- one decision: (lam, box or None); lam == 1 means "not mixed"
    def _decide(self):
        r = self.rng
        if not r.random() < self.prob:
            return 1.0, None
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = bool(r.random() < self.switch_prob)
        else:
            cut = self.cutmix_alpha > 0
        a = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(r.beta(a, a))
        if not cut:
            return lam, None
        H = W = self.img
        if self.minmax is None:                     # timm rand_bbox (margin 0)
            ratio = np.sqrt(1.0 - lam)
            cut_h, cut_w = int(H * ratio), int(W * ratio)
            cy, cx = int(r.integers(0, H)), int(r.integers(0, W))
            yl, yh = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
            xl, xh = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
        else:                                       # timm rand_bbox_minmax
            cut_h = int(r.integers(int(H * self.minmax[0]), int(H * self.minmax[1])))
            cut_w = int(r.integers(int(W * self.minmax[0]), int(W * self.minmax[1])))
            yl, xl = int(r.integers(0, H - cut_h)), int(r.integers(0, W - cut_w))
            yh, xh = yl + cut_h, xl + cut_w
        lam = 1.0 - (yh - yl) * (xh - xl) / float(H * W)       # correct_lam
        return lam, (yl, yh, xl, xh)

    def sample_host(self) -> Optional[np.ndarray]:
        if not self.enabled:
            return None
        B = self.B
        rows = MixPlan.make_rows(B)
        if self.mode == "batch":
            lam, box = self._decide()
            for i in range(B):
                MixPlan.set_row(rows, i, lam, box)
        elif self.mode == "elem":
            for i in range(B):
                MixPlan.set_row(rows, i, *self._decide())
        else:                                       # pair: drawn for the first half, mirrored onto the second
            for i in range(B // 2):
                lam, box = self._decide()
                MixPlan.set_row(rows, i, lam, box)
                MixPlan.set_row(rows, B - 1 - i, lam, box)
        return rows

    def sample(self, device=None) -> Optional[MixPlan]:
        rows = self.sample_host()
        return None if rows is None else MixPlan(rows, device)

    def state_dict(self):
        """Plain strings / bools (loads with weights_only=True): the bit generator's state as JSON, as the driver's host_rng entries."""
        return {"rng": json.dumps(self.rng.bit_generator.state), "enabled": bool(self.enabled)}

    def load_state_dict(self, sd):
        self.rng.bit_generator.state = json.loads(sd["rng"])
        self.enabled = bool(sd.get("enabled", self.enabled))


assert ROW_DT.itemsize == 32
