"""H&E stain jitter for the DINO views (host side of gv_crop_augment_stain; ``--stain-jitter``).

Stain augmentation in optical-density space (Tellez et al. 2018 / 2019: "HED-light" sigma = 0.05, "HED-strong" sigma = 0.2) with
Ruifrok & Johnston's colour-deconvolution vectors.  The reference has nothing like it (it augments with torchvision ColorJitter
on the CPU); formula and random stream are this build's own.  With M the stain matrix (rows H, E, D, unit length), a pixel
with bytes v_c goes through

    od_c  = -ln((v_c + 1) / 256)                        (>= 0, finite for v = 0)
    s     = od . M^-1                                   (stain concentrations, not clamped)
    s'_k  = alpha_k * s_k + beta_k                      (k = H, E, D)
    od'   = s' . M
    v'_c  = clamp(rint(256 * exp(-od'_c) - 1), 0, 255)  (round half to even)

(not skimage's rgb2hed, which clamps and so cannot be inverted).  The map is affine in od: a crop's draw is folded here into
A = M^-1 diag(alpha) M and b = beta M (fp64, rounded to f32), and only that 52-byte record travels to the device, where the
pixel work happens inside the pass that cuts and augments the crop.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch


def _unit_rows(m) -> np.ndarray:
    m = np.asarray(m, np.float64)
    return m / np.linalg.norm(m, axis=1, keepdims=True)


# rows H, E, D (Ruifrok & Johnston 2001), each normalised to unit length; condition number 3.8
STAIN_MATRIX = _unit_rows([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]])
STAIN_MATRIX.setflags(write=False)

# one packed gv_stain_params record (include/gipvit.h)
DT = np.dtype([("on", "<i4"), ("A", "<f4", (3, 3)), ("b", "<f4", (3,))])


def stain_affine(alpha, beta, matrix=STAIN_MATRIX) -> Tuple[np.ndarray, np.ndarray]:
    """The draw (alpha, beta) [..., 3] folded into od' = od . A + b, in fp64: A [..., 3, 3] = M^-1 diag(alpha) M, b [..., 3] = beta M."""
    m = np.asarray(matrix, np.float64)
    alpha, beta = np.asarray(alpha, np.float64), np.asarray(beta, np.float64)
    A = np.einsum("ik,...k,kc->...ic", np.linalg.inv(m), alpha, m)
    return A, beta @ m


def stain_record(alpha, beta, matrix=STAIN_MATRIX) -> np.ndarray:
    """-> gv_stain_params record(s) (dtype ``DT``, on = 1) of the draw: ``stain_affine`` rounded to f32."""
    A, b = stain_affine(alpha, beta, matrix)
    r = np.zeros(A.shape[:-2], DT)
    r["on"], r["A"], r["b"] = 1, A, b
    return r


def stain_od(od, A, b) -> np.ndarray:
    """od' = od . A + b in fp64 (od [..., 3])."""
    return np.asarray(od, np.float64) @ np.asarray(A, np.float64) + np.asarray(b, np.float64)


def stain_reference(img_u8, A, b) -> Tuple[np.ndarray, np.ndarray]:
    """The transform of one record restated in numpy fp64, for the tests: ``img_u8`` uint8 [..., 3], ``A`` [3, 3] and ``b`` [3] as
    the record holds them.  -> (256 * exp(-od') - 1 unrounded, fp64; the bytes: that value rounded half to even and clamped)."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    od = -np.log((img.astype(np.float64) + 1.0) / 256.0)
    x = 256.0 * np.exp(-stain_od(od, A, b)) - 1.0
    return x, np.clip(np.rint(x), 0, 255).astype(np.uint8)


class StainJitterSampler:
    """Per-crop draws of the stain jitter: with probability ``prob`` a crop gets alpha_k ~ U(1 - sigma, 1 + sigma) and
    beta_k ~ U(-sigma, sigma) for k = H, E, D, otherwise ``on = 0`` (the record then carries A = I, b = 0).  Every crop consumes
    the same number of draws whether it is jittered or not.  Rows are crop-major, global crops first, like
    multicrop.ViewAugmentSampler's."""

    DT = DT

    def __init__(self, batch: int, n_global: int = 2, n_local: int = 8, sigma: float = 0.05, prob: float = 1.0, seed: int = 0, matrix=STAIN_MATRIX):
        if not (np.isfinite(sigma) and 0 <= sigma < 1):
            raise ValueError(f"sigma={sigma}: must be finite and in [0, 1) (alpha has to stay positive)")
        if not 0 < prob <= 1:
            raise ValueError(f"prob={prob}: must be in (0, 1]")
        self.B, self.G, self.Lc, self.sigma, self.prob = batch, n_global, n_local, float(sigma), float(prob)
        self.matrix = np.array(matrix, np.float64)
        self.rng = np.random.default_rng(seed)

    def _draw(self, n_crops: int):
        n, s = n_crops * self.B, self.sigma
        on = self.rng.random(n) < self.prob
        return on, self.rng.uniform(1.0 - s, 1.0 + s, (n, 3)), self.rng.uniform(-s, s, (n, 3))

    def sample_draws(self):
        """-> ((on [G*B], alpha [G*B, 3], beta [G*B, 3]), the same for the L*B local crops): the draws before they are folded."""
        return self._draw(self.G), self._draw(self.Lc)

    def _records(self, on, alpha, beta) -> np.ndarray:
        r = stain_record(np.where(on[:, None], alpha, 1.0), np.where(on[:, None], beta, 0.0), self.matrix)
        r["on"] = on
        r["A"][~on], r["b"][~on] = np.eye(3, dtype=np.float32), 0.0      # exactly I, not M^-1 M
        return r

    def sample_host(self):
        """-> (global records [G*B], local records [L*B]) as structured numpy arrays of ``DT``."""
        return tuple(self._records(*d) for d in self.sample_draws())

    @staticmethod
    def to_dicts(a: np.ndarray):
        return [dict(on=bool(r["on"]), A=np.array(r["A"]), b=np.array(r["b"])) for r in a]

    @staticmethod
    def pack(a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())

    def sample(self, device=None):
        """-> (global, local) packed gv_stain_params records as uint8 tensors on ``device``."""
        out = [self.pack(x) for x in self.sample_host()]
        return tuple(t.to(device, non_blocking=True) if device is not None else t for t in out)
