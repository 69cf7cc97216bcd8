"""Host side of the iBOT masked-patch term: which patches of which global crop the student does not see.

``MaskSampler`` restates DINOv2's collate (``collate_data_and_cast``) and its ``MaskingGenerator`` from their description -- the
source is not here, so the restatement is pinned by nothing but itself.  Of the J = G * B global-crop images of a micro-batch,
``int(J * prob)`` are masked.  The i-th of those n draws its target count ``int(P * u)`` with u uniform in the i-th of n equal
sub-intervals of ``ratio``; blocks are added until the target is met.  A block draws an area uniform in [4, min(remaining, 0.5 P)]
and a log-uniform aspect ratio in [0.3, 1 / 0.3], h = round(sqrt(area * aspect)), w = round(sqrt(area / aspect)), and a position; it is
accepted if h < H, w < W and it adds between 1 and ``remaining`` new patches.  Ten tries per block; the image stops at the first
block that fails all of them, so a count may stay below its target (DINOv2 does not top it up either).  The order of masked and
unmasked images is then shuffled.

Draws come from numpy's ``default_rng``, seeded per rank, like the other host streams: the SAME distributions as DINOv2's
``random`` / ``np.random`` calls, not the same numbers -- the stream is not bit-compatible with Python's ``random``.

The device's part is ``MaskPlan``: an ascending int32 table of token rows (row = j * N + 1 + p; the student's global segment and
the teacher's group both start at row 0, so one table serves both) and the weight 1 / (n_j J) of each row.
"""
from __future__ import annotations

import json
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

MIN_BLOCK = 4                 # DINOv2 MaskingGenerator: min_num_patches
MAX_ASPECT = 1.0 / 0.3        # ... min_aspect 0.3, max_aspect 1 / 0.3
TRIES = 10


class MaskPlan:
    """One micro-batch's masks: ``masks`` bool [J, P] on the host, ``M`` marked patches in all, ``counts`` [J], and -- on ``device``
    once given -- ``rows`` int32 [M] ascending and ``weight`` float32 [M] = 1 / (n_j J).  Both are empty tensors when M = 0."""

    def __init__(self, masks: np.ndarray, device=None):
        masks = np.ascontiguousarray(masks)
        if masks.dtype != np.bool_ or masks.ndim != 2:
            raise ValueError(f"masks: a boolean [J, P] array, got {masks.dtype} {masks.shape}")
        self.masks = masks
        self.J, self.P = masks.shape
        self.N = self.P + 1
        self.counts = masks.sum(1).astype(np.int64)
        j, p = np.nonzero(masks)                                    # row-major: ascending in j, then p
        self.M = int(j.size)
        self.rows_host = (j * self.N + 1 + p).astype(np.int32)
        self.weight_host = (1.0 / (self.counts[j].astype(np.float64) * self.J)).astype(np.float32)
        self.rows, self.weight = torch.from_numpy(self.rows_host), torch.from_numpy(self.weight_host)
        if device is not None:
            self.rows, self.weight = self.rows.to(device, non_blocking=True), self.weight.to(device, non_blocking=True)

    @classmethod
    def from_masks(cls, masks, device=None) -> "MaskPlan":
        """A plan from explicit masks: anything ``np.asarray`` turns into a boolean [J, P] array (a torch tensor included)."""
        if isinstance(masks, torch.Tensor):
            masks = masks.cpu().numpy()
        return cls(np.asarray(masks, dtype=np.bool_), device)

    @property
    def n_masked_images(self) -> int:
        return int((self.counts > 0).sum())


def check_mask_options(ratio: Sequence[float], prob: float):
    """0 < lo <= hi < 1 and 0 < prob <= 1, or a ValueError that names the option."""
    if len(ratio) != 2 or not all(math.isfinite(float(r)) for r in ratio) or not 0.0 < float(ratio[0]) <= float(ratio[1]) < 1.0:
        raise ValueError(f"ibot mask ratio {list(ratio)}: need 0 < LO <= HI < 1")
    if not (math.isfinite(float(prob)) and 0.0 < float(prob) <= 1.0):
        raise ValueError(f"ibot mask probability {prob}: need 0 < P <= 1")


def max_rows(n_images: int, P: int, ratio: Sequence[float], prob: float) -> int:
    """The most rows a sampled plan can mark: int(J * prob) images of at most int(hi * P) patches (the head buffers' size)."""
    return int(n_images * prob) * int(ratio[1] * P)


class MaskSampler:
    """``sample(device)`` -> MaskPlan for ``n_images`` global-crop images of a ``grid`` x ``grid`` patch grid."""

    def __init__(self, grid: int, n_images: int, ratio: Tuple[float, float] = (0.1, 0.5), prob: float = 0.5, seed: int = 0):
        check_mask_options(ratio, prob)
        if grid < 4:
            raise ValueError(f"ibot masking needs a patch grid of at least 4 x 4 (a global crop of 64 px), got {grid} x {grid}")
        if n_images < 1:
            raise ValueError(f"n_images {n_images}: at least 1")
        self.grid, self.J, self.P = int(grid), int(n_images), int(grid) * int(grid)
        self.ratio, self.prob = (float(ratio[0]), float(ratio[1])), float(prob)
        self.rng = np.random.default_rng(seed)
        self.max_block = 0.5 * self.P
        self.last_targets: Optional[np.ndarray] = None       # the targets of the last sample, in the shuffled image order (0: unmasked)

    def _block(self, mask: np.ndarray, remaining: int) -> int:
        """Try to add one block of at most ``remaining`` new patches; -> how many it added (0: all tries failed)."""
        r, H = self.rng, self.grid
        hi = min(float(remaining), self.max_block)
        for _ in range(TRIES):
            area = MIN_BLOCK + (hi - MIN_BLOCK) * r.random()      # (fewer than 4 left: between the two, as random.uniform(4, remaining) gives)
            aspect = math.exp(r.uniform(math.log(1.0 / MAX_ASPECT), math.log(MAX_ASPECT)))
            h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if not (0 < h < H and 0 < w < H):
                continue
            top, left = int(r.integers(0, H - h + 1)), int(r.integers(0, H - w + 1))
            new = h * w - int(mask[top:top + h, left:left + w].sum())
            if 0 < new <= remaining:
                mask[top:top + h, left:left + w] = True
                return new
        return 0

    def _one(self, target: int) -> np.ndarray:
        mask = np.zeros((self.grid, self.grid), np.bool_)
        count = 0
        while count < target:
            new = self._block(mask, target - count)
            if new == 0:
                break
            count += new
        return mask.reshape(-1)

    def sample_host(self) -> np.ndarray:
        J, P, (lo, hi) = self.J, self.P, self.ratio
        n = int(J * self.prob)
        masks, targets = np.zeros((J, P), np.bool_), np.zeros(J, np.int64)
        edges = np.linspace(lo, hi, n + 1)
        for i in range(n):
            targets[i] = int(P * self.rng.uniform(edges[i], edges[i + 1]))
            masks[i] = self._one(int(targets[i]))
        order = self.rng.permutation(J)
        self.last_targets = targets[order]
        return masks[order]

    def sample(self, device=None) -> MaskPlan:
        return MaskPlan(self.sample_host(), device)

    def state_dict(self):
        """Plain strings (loads with weights_only=True): the bit generator's state as JSON, as the driver's host_rng entries."""
        return {"rng": json.dumps(self.rng.bit_generator.state)}

    def load_state_dict(self, sd):
        self.rng.bit_generator.state = json.loads(sd["rng"])
