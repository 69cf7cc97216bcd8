"""Host side of random erasing (--reprob / --remode / --recount): the per-step DRAWS of timm's ``RandomErasing`` as its
``PrefetchLoader`` constructs it (``timm/data/random_erasing.py``; device-side, per image of the batch, on the normalised
batch, after the collate mixup), restated.  The reference's timm_train.py:621-624 passes the three flags to timm's loader; its
train.py:788-791 has the same call commented out.  timm is not installed here and the reference does not pin a version: the
restatement is pinned by nothing but itself.  The pixels are the device's work -- an ``ErasePlan`` carries the erase table and
the seed of gv_patchify_erase / gv_patchify_nchw_erase (include/gipvit.h), which erase inside the patchify pass.

Per image, on the supervised step's img_size window of side S: ``u > prob`` leaves it untouched; ``count`` is 1 or uniform in
[1, recount]; each of the ``count`` boxes takes up to 10 attempts at ``area = U(0.02, 1/3) * S^2 / count``, ``aspect =
exp(U(ln 0.3, ln(1/0.3)))``, ``h = int(round(sqrt(area * aspect)))``, ``w = int(round(sqrt(area / aspect)))``, accepted when
``h < S and w < S`` with ``top ~ randint[0, S - h]``, ``left ~ randint[0, S - w]``.  Fill: 'const' zeros, 'rand' one N(0, 1)
value per channel and box (drawn here), 'pixel' one N(0, 1) value per pixel and channel (generated in the kernel from the
step's seed; ``noise_reference`` restates the generator).  Boxes are applied in order.

Draws come from numpy's ``default_rng`` like the other host streams (timm uses python's ``random`` and torch's generator), so the
SAME distributions, not the same numbers."""
from __future__ import annotations

import json
import math
from typing import Optional, Sequence

import numpy as np
import torch

ERASE_OFF, ERASE_VALUE, ERASE_NOISE = 0, 1, 2      # gipvit.h GV_ERASE_*
MAX_BOXES = 8                                      # gipvit.h GV_ERASE_MAX_BOXES
# gv_erase_row (gipvit.h / _lib.gv_erase_row): 232 bytes
ROW_DT = np.dtype([("mode", "<i4"), ("n_box", "<i4"), ("box", "<i4", (MAX_BOXES, 4)), ("value", "<f4", (MAX_BOXES, 3))])
MODES = ("pixel", "rand", "const")
MIN_AREA, MAX_AREA, MIN_ASPECT, ATTEMPTS = 0.02, 1.0 / 3.0, 0.3, 10      # timm RandomErasing's defaults


class ErasePlan:
    """One step's erasing: ``rows`` (host, ROW_DT [B]), ``seed`` (the 32-bit seed of the 'pixel' noise) and, once on a device,
    ``table`` uint8 [B * 232] (the gv_erase_row records)."""

    def __init__(self, rows: np.ndarray, seed: int = 0, device=None):
        assert rows.dtype == ROW_DT and rows.ndim == 1 and 0 <= int(seed) < (1 << 32)
        self.rows, self.seed = rows, int(seed)
        self.table = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy())
        if device is not None:
            self.table = self.table.to(device, non_blocking=True)

    @staticmethod
    def make_rows(B: int) -> np.ndarray:
        """B rows that erase nothing."""
        return np.zeros(B, ROW_DT)

    @staticmethod
    def add_box(rows: np.ndarray, i: int, box: Sequence[int], value=(0.0, 0.0, 0.0), mode: int = ERASE_VALUE):
        """Append box (yl, yh, xl, xh) to row i; ``value``: its fill per channel (ERASE_VALUE rows)."""
        n = int(rows["n_box"][i])
        if n >= MAX_BOXES:
            raise ValueError(f"a gv_erase_row holds {MAX_BOXES} boxes")
        rows["mode"][i] = mode
        rows["box"][i, n] = box
        rows["value"][i, n] = value
        rows["n_box"][i] = n + 1


class EraseSampler:
    """timm ``RandomErasing``'s draws.  ``sample(device)`` -> ErasePlan."""

    def __init__(self, prob: float = 0.25, mode: str = "pixel", count: int = 1, batch: int = 8, img_size: int = 224, seed: int = 0):
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f"random erasing: prob {prob} is a probability, 0 <= p <= 1")
        if mode not in MODES:
            raise ValueError(f"random erasing: mode {mode!r}: one of {MODES}")
        if not 1 <= count <= MAX_BOXES:
            raise ValueError(f"random erasing: count {count}: 1 .. {MAX_BOXES} boxes per image (GV_ERASE_MAX_BOXES)")
        self.prob, self.mode, self.count, self.B, self.img = float(prob), mode, int(count), int(batch), int(img_size)
        self.rng = np.random.default_rng(seed)

    def sample_host(self):
        """-> (rows, seed).  Order of draws: the step's seed; then per image u, the count (recount > 1), and per attempt the area,
        the aspect and -- accepted -- top, left and the 'rand' values."""
        r, S = self.rng, self.img
        seed = int(r.integers(0, 1 << 32))
        rows = ErasePlan.make_rows(self.B)
        la = math.log(MIN_ASPECT)
        for i in range(self.B):
            if r.random() > self.prob:
                continue
            rows["mode"][i] = ERASE_NOISE if self.mode == "pixel" else ERASE_VALUE
            count = 1 if self.count == 1 else int(r.integers(1, self.count + 1))
            for _ in range(count):
                for _ in range(ATTEMPTS):
                    area = float(r.uniform(MIN_AREA, MAX_AREA)) * S * S / count
                    aspect = math.exp(float(r.uniform(la, -la)))
                    h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                    if h < S and w < S:
                        top, left = int(r.integers(0, S - h + 1)), int(r.integers(0, S - w + 1))
                        value = r.standard_normal(3) if self.mode == "rand" else (0.0, 0.0, 0.0)
                        if h > 0 and w > 0:      # (an empty box erases nothing in timm either)
                            ErasePlan.add_box(rows, i, (top, top + h, left, left + w), value, int(rows["mode"][i]))
                        break
        return rows, seed

    def sample(self, device=None) -> ErasePlan:
        rows, seed = self.sample_host()
        return ErasePlan(rows, seed, device)

    def state_dict(self):
        """Plain strings (loads with weights_only=True): the bit generator's state as JSON, as the driver's host_rng entries."""
        return {"rng": json.dumps(self.rng.bit_generator.state)}

    def load_state_dict(self, sd):
        self.rng.bit_generator.state = json.loads(sd["rng"])


def _fmix32(h: np.ndarray) -> np.ndarray:
    """murmur3's finaliser on uint32 values held in uint64."""
    M = np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16)); h = (h * np.uint64(0x85EBCA6B)) & M
    h = h ^ (h >> np.uint64(13)); h = (h * np.uint64(0xC2B2AE35)) & M
    return h ^ (h >> np.uint64(16))


def noise_reference(seed: int, n_img: int, S: int) -> np.ndarray:
    """The kernels' 'pixel' noise z(img, c, y, x) for the whole window of every image, float64 [n_img, 3, S, S]: the generator of
    include/gipvit.h (GV_ERASE_NOISE) with the formula's f32 inputs -- u1, u2 and the constant 6.2831853f -- evaluated in double."""
    n = n_img * 3 * S * S
    if n >= 1 << 32:
        raise ValueError(f"n_img * 3 * S^2 = {n}: the pixel index is 32 bits")
    M = np.uint64(0xFFFFFFFF)
    idx = np.arange(n, dtype=np.uint64)
    h1 = _fmix32((np.uint64(seed) + np.uint64(0x9E3779B9) * (idx + np.uint64(1))) & M)
    h2 = _fmix32((h1 + np.uint64(0x6D2B79F5)) & M)
    u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (h2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(float(np.float32(6.2831853)) * u2)
    return z.reshape(n_img, 3, S, S)


def apply_reference(x: torch.Tensor, plan: ErasePlan) -> torch.Tensor:
    """The whole operation restated in torch, for the tests: ``x`` float32 [B, 3, S, S], the normalised (and already mixed) window
    the network would see; returns the erased copy.  ERASE_NOISE boxes take ``noise_reference`` rounded to f32 (the device
    evaluates the formula in f32: equal within the tests' 1e-5, not bit for bit)."""
    B, C, S, S2 = x.shape
    assert C == 3 and S == S2 and len(plan.rows) == B and x.dtype == torch.float32
    out = x.detach().cpu().clone()
    noise = None
    for i, r in enumerate(plan.rows):
        mode, nb = int(r["mode"]), int(r["n_box"])
        if mode not in (ERASE_VALUE, ERASE_NOISE) or not 0 <= nb <= MAX_BOXES:
            continue
        for b in range(nb):
            yl, yh, xl, xh = (min(max(int(v), 0), S) for v in r["box"][b])
            if yh <= yl or xh <= xl:
                continue
            if mode == ERASE_VALUE:
                out[i, :, yl:yh, xl:xh] = torch.from_numpy(r["value"][b].copy()).view(3, 1, 1)
            else:
                if noise is None:
                    noise = torch.from_numpy(noise_reference(plan.seed, B, S).astype(np.float32))
                out[i, :, yl:yh, xl:xh] = noise[i, :, yl:yh, xl:xh]
    return out.to(x.device)


assert ROW_DT.itemsize == 232
