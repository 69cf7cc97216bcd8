"""Macenko stain normalisation at inference (``--stain-normalize macenko``; Macenko et al., ISBI 2009).

The training side jitters the DINO views in optical-density space (gipvit/stain.py); this is the inference side: per slide, the
slide's own haematoxylin / eosin vectors ``HE`` [3, 2] and their 99th-percentile concentrations ``maxC`` [2] are estimated from a
sample of its tiles, and the slide is mapped onto a fixed target.  The reference has nothing like it.  Optical density is this
project's, od_c = -ln((v_c + 1) / 256), and bytes come back as v'_c = clamp(rint(256 exp(-od'_c) - 1), 0, 255) -- not the
-ln(v / 240) of the usual scripts: a slide whose estimate equals the target maps onto itself.  The map is
linear in od, od' = od . A with A = (HE_t diag(maxC_t / maxC) pinv(HE))^T, i.e. one ``gv_stain_params`` record per slide that
gv_patchify_stain evaluates inside the patchify pass (no extra pass over the pixels) and gv_stain_apply writes back as bytes.

The estimate, stated in include/gipvit.h and restated here in fp64 numpy (``macenko_reference``):

    tissue   pixel p is tissue iff all three bytes are <= v_max = floor(256 exp(-beta)) - 1  (beta = 0.15: 219)
    pass 1   over tissue pixels: n, sum od, sum od_i od_j  ->  covariance (S2 - n mu mu^T) / (n - 1), eigh, the two leading
             eigenvectors V [3, 2] (largest first, each flipped so that its component sum is >= 0)
    pass 2   over tissue pixels: t = od . V, phi = atan2(t1, t0), histogram of ``bins`` bins over [-pi, pi)  ->  phi_lo, phi_hi =
             the alpha-th and (100 - alpha)-th percentile, v = V (cos phi, sin phi); larger first component: H, the other: E
    pass 3   over ALL pixels (as Macenko's code does): c = pinv(HE) od, one histogram per stain over [0, cmax_k), cmax_k =
             ln 256 * sum_j max(pinv_kj, 0) (an upper bound since od >= 0), c_k < 0 in an underflow count  ->  maxC_k = the
             99th percentile

Percentiles are read from histograms (``hist_percentile``): their resolution is one bin width, 2 pi / bins for the angles and
cmax_k / bins for the concentrations.  The slide passes through untouched (record ``on = 0``) when fewer than max(64, 1 % of the
sampled pixels) are tissue, an estimate is not finite, maxC_k <= 1e-3 or |cos angle(H, E)| > 0.999.
"""
from __future__ import annotations

import bisect
import itertools
import logging
import math
from collections import Counter
from fractions import Fraction
from typing import NamedTuple, Optional

import numpy as np
import torch

from .stain import DT

_logger = logging.getLogger("train")

LN256 = math.log(256.0)
# fallback reasons, in the order they are tested
FEW_TISSUE, NONFINITE, COLLINEAR, LOW_CONCENTRATION = "few_tissue", "nonfinite", "collinear", "low_concentration"


class MacenkoTarget:
    """The stain vectors ``HE`` [3, 2] (columns H, E) and concentrations ``maxC`` [2] every slide is mapped onto; the default is
    Macenko's published reference."""

    def __init__(self, HE=((0.5626, 0.2159), (0.7201, 0.8012), (0.4062, 0.5581)), maxC=(1.9705, 1.0308)):
        self.HE, self.maxC = np.array(HE, np.float64), np.array(maxC, np.float64)
        if self.HE.shape != (3, 2) or self.maxC.shape != (2,) or not (np.isfinite(self.HE).all() and np.isfinite(self.maxC).all() and (self.maxC > 0).all()):
            raise ValueError("MacenkoTarget: HE must be a finite [3, 2], maxC a finite positive [2]")


def check_params(beta: float, alpha: float, bins: int = 4096, max_tiles: int = 0) -> None:
    if not (math.isfinite(beta) and 0.0 < beta < LN256):
        raise ValueError(f"beta={beta}: the od threshold of the tissue mask must be in (0, ln 256)")
    if not (math.isfinite(alpha) and 0.0 < alpha < 50.0):
        raise ValueError(f"alpha={alpha}: the angle percentile must be in (0, 50)")
    if not 256 <= int(bins) <= 4096:
        raise ValueError(f"bins={bins}: must be in 256 .. 4096")
    if int(max_tiles) < 0:
        raise ValueError(f"max_tiles={max_tiles}: must be >= 0 (0: the whole first chunk)")


def tissue_v_max(beta: float) -> int:
    """A pixel is tissue iff every byte is <= this: floor(256 exp(-beta)) - 1 (219 at beta = 0.15)."""
    return int(math.floor(256.0 * math.exp(-beta))) - 1


def od_table() -> np.ndarray:
    """od of the 256 byte values, fp64."""
    return -np.log((np.arange(256, dtype=np.float64) + 1.0) / 256.0)


def hist_percentile(hist, under: int, lo: float, hi: float, p: float) -> float:
    """The p-th percentile of n = under + sum(hist) values of which ``hist[b]`` lie in bin b of len(hist) equal bins over
    [lo, hi) and ``under`` below lo, with numpy's convention: the values in ascending order, rank r = p / 100 * (n - 1), linear
    interpolation between the values of rank floor(r) and floor(r) + 1.  A histogram does not know where inside its bin a value
    lies: the i-th of the m values of a bin (i = 0 .. m - 1, in rank order) is placed at the centre of the i-th of m equal cells of
    that bin, lo + (b + (i + 1/2) / m) * width, a value of the underflow count at ``lo``.  Both interpolated positions lie in the
    bins of the values they stand for, so the result is within ONE BIN WIDTH of the exact percentile of the binned values -- that
    is the resolution, whatever the counts.  Counts, ranks and positions are exact integers / rationals; one rounding at the end."""
    under = int(under)
    if isinstance(hist, np.ndarray) and hist.dtype.kind in "iu" and hist.size and int(hist.max()) < (1 << 40):
        h = hist.reshape(-1).astype(np.int64)                 # the device's counts: int64 sums are exact (< 2^32 pixels a call)
        cum, low = np.cumsum(h), int(h.min())
        bin_of = lambda j: int(np.searchsorted(cum, j, side="right"))
    else:                                                     # any integers, however large
        h = [int(x) for x in (hist.reshape(-1).tolist() if isinstance(hist, np.ndarray) else hist)]
        cum, low = list(itertools.accumulate(h)), min(h, default=0)
        bin_of = lambda j: bisect.bisect_right(cum, j)
    n = under + (int(cum[-1]) if len(h) else 0)
    if n <= 0 or under < 0 or not len(h) or low < 0:
        raise ValueError("hist_percentile: needs non-negative counts and at least one value")
    if not 0.0 <= p <= 100.0:
        raise ValueError(f"hist_percentile: p={p} outside [0, 100]")
    flo, width = Fraction(lo), (Fraction(hi) - Fraction(lo)) / len(h)

    def position(k: int) -> Fraction:            # of the value of rank k
        if k < under:
            return flo
        b = bin_of(k - under)
        m = int(h[b])
        return flo + (b + (Fraction(k - under - (int(cum[b]) - m)) + Fraction(1, 2)) / m) * width

    r = Fraction(p) / 100 * (n - 1)
    k = r.numerator // r.denominator
    x = position(k)
    if r != k:
        x += (r - k) * (position(k + 1) - x)
    return float(x)


# ---- the host steps between the passes (shared by the fp64 restatement and the device estimator) ----------------------------
def _stain_basis(n: int, S1: np.ndarray, S2: np.ndarray) -> np.ndarray:
    """n, sum od [3], sum od od^T [3, 3] -> V [3, 2]: the two leading eigenvectors of the covariance, largest first, each flipped
    so that its component sum is >= 0."""
    mu = S1 / n
    cov = (S2 - n * np.outer(mu, mu)) / (n - 1)
    _, vec = np.linalg.eigh(cov)
    V = vec[:, [2, 1]].copy()
    for k in range(2):
        if V[:, k].sum() < 0:
            V[:, k] = -V[:, k]
    return V


def _sym(s6) -> np.ndarray:
    rr, rg, rb, gg, gb, bb = (float(x) for x in s6)
    return np.array([[rr, rg, rb], [rg, gg, gb], [rb, gb, bb]], np.float64)


def _stain_vectors(V: np.ndarray, hist, alpha: float):
    """V [3, 2], the angle histogram -> (phi_lo, phi_hi, HE [3, 2])."""
    phi = [hist_percentile(hist, 0, -math.pi, math.pi, q) for q in (alpha, 100.0 - alpha)]
    v = [V @ np.array([math.cos(f), math.sin(f)]) for f in phi]
    HE = np.stack([v[0], v[1]] if v[0][0] > v[1][0] else [v[1], v[0]], axis=1)
    return phi[0], phi[1], HE


def normaliser_record(HE, maxC, target: Optional[MacenkoTarget] = None) -> np.ndarray:
    """-> one gv_stain_params record (dtype ``stain.DT``, shape [1], on = 1, b = 0) with A = (HE_t diag(maxC_t / maxC) pinv(HE))^T
    taken in fp64 and rounded to f32: od' = od . A maps a slide with vectors ``HE`` and concentrations ``maxC`` onto ``target``."""
    target = target or MacenkoTarget()
    HE, maxC = np.asarray(HE, np.float64), np.asarray(maxC, np.float64)
    M = target.HE @ np.diag(target.maxC / maxC) @ np.linalg.pinv(HE)
    r = np.zeros(1, DT)
    r["on"], r["A"], r["b"] = 1, M.T, 0.0
    return r


def off_record() -> np.ndarray:
    """The record of a slide that passes through untouched: on = 0 (A = I, b = 0)."""
    r = np.zeros(1, DT)
    r["A"] = np.eye(3, dtype=np.float32)
    return r


def pack_record(rec: np.ndarray) -> torch.Tensor:
    """One record -> its 52 bytes as a uint8 tensor (host)."""
    rec = np.ascontiguousarray(np.asarray(rec, DT).reshape(-1))
    if rec.shape[0] != 1:
        raise ValueError(f"expected ONE gv_stain_params record, got {rec.shape[0]}")
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())


class SlideStain(NamedTuple):
    """One slide's estimate.  ``on`` False: the fallback, ``reason`` says which (HE / maxC then hold what had been estimated up to
    there, NaN otherwise) and ``record`` has on = 0."""
    HE: np.ndarray
    maxC: np.ndarray
    n_tissue: int
    n_pixels: int
    on: bool
    reason: str
    record: np.ndarray


class _Passes:
    """The three passes over one sample of tiles, as the estimate consumes them."""

    n_pixels: int

    def stats(self, v_max):                   # -> (n, S1 [3], S2 [3, 3])
        raise NotImplementedError

    def angle_hist(self, V, v_max, bins):     # -> counts [bins]
        raise NotImplementedError

    def conc_hist(self, pinv, cmax, bins):    # -> counts [2, bins + 1]
        raise NotImplementedError


def _estimate(ps: _Passes, beta: float, alpha: float, bins: int, target: MacenkoTarget, out: dict) -> SlideStain:
    """The estimate over the passes ``ps``; every intermediate goes into ``out``."""
    nan32, nan2 = np.full((3, 2), np.nan), np.full(2, np.nan)
    v_max = tissue_v_max(beta)
    out.update(v_max=v_max, n_pixels=ps.n_pixels)

    def fallback(reason, HE=nan32, maxC=nan2):
        out.update(on=False, reason=reason, record=off_record())
        return SlideStain(HE, maxC, out.get("n", 0), ps.n_pixels, False, reason, out["record"])

    n, S1, S2 = ps.stats(v_max)
    out.update(n=n, S1=S1, S2=S2)
    if n < max(64, math.ceil(0.01 * ps.n_pixels)):
        return fallback(FEW_TISSUE)
    V = _stain_basis(n, S1, S2)
    out.update(V=V)
    if not np.isfinite(V).all():
        return fallback(NONFINITE)
    hist = ps.angle_hist(V, v_max, bins)
    phi_lo, phi_hi, HE = _stain_vectors(V, hist, alpha)
    out.update(angle_hist=hist, phi_lo=phi_lo, phi_hi=phi_hi, HE=HE)
    if not np.isfinite(HE).all():
        return fallback(NONFINITE)
    cosang = float(HE[:, 0] @ HE[:, 1] / (np.linalg.norm(HE[:, 0]) * np.linalg.norm(HE[:, 1])))
    out.update(cos_angle=cosang)
    if not math.isfinite(cosang):
        return fallback(NONFINITE, HE)
    if abs(cosang) > 0.999:
        return fallback(COLLINEAR, HE)
    pinv = np.linalg.pinv(HE)
    cmax = LN256 * np.maximum(pinv, 0.0).sum(axis=1)
    out.update(pinv=pinv, cmax=cmax)
    if not (np.isfinite(pinv).all() and np.isfinite(cmax).all()):
        return fallback(NONFINITE, HE)
    if (cmax <= 1e-3).any():                  # every concentration of that stain is <= 0
        return fallback(LOW_CONCENTRATION, HE)
    ch = ps.conc_hist(pinv, cmax, bins)
    maxC = np.array([hist_percentile(ch[k, :bins], ch[k, bins], 0.0, cmax[k], 99.0) for k in range(2)])
    out.update(conc_hist=ch, maxC=maxC)
    if not np.isfinite(maxC).all():
        return fallback(NONFINITE, HE, maxC)
    if (maxC <= 1e-3).any():
        return fallback(LOW_CONCENTRATION, HE, maxC)
    rec = normaliser_record(HE, maxC, target)
    if not np.isfinite(rec["A"]).all():
        return fallback(NONFINITE, HE, maxC)
    out.update(on=True, reason="", record=rec, A=np.array(rec["A"][0], np.float64))
    return SlideStain(HE, maxC, n, ps.n_pixels, True, "", rec)


class _NumpyPasses(_Passes):
    """fp64 numpy over host tiles: the definition."""

    def __init__(self, tiles_u8: np.ndarray, out: dict):
        t = np.asarray(tiles_u8)
        if t.dtype != np.uint8 or t.ndim != 4 or t.shape[-1] != 3:
            raise ValueError(f"tiles: expected uint8 [n, h, w, 3], got {t.dtype} {t.shape}")
        self.px = t.reshape(-1, 3)
        self.od = od_table()[self.px]
        self.n_pixels, self.out = self.px.shape[0], out

    def stats(self, v_max):
        self.mask = (self.px <= v_max).all(axis=1)
        od = self.od[self.mask]
        self.out.update(mask=self.mask)
        r, g, b = od[:, 0], od[:, 1], od[:, 2]
        return int(self.mask.sum()), od.sum(axis=0), _sym([(r * r).sum(), (r * g).sum(), (r * b).sum(), (g * g).sum(), (g * b).sum(), (b * b).sum()])

    def angle_hist(self, V, v_max, bins):
        od = self.od[self.mask]
        t0 = od[:, 0] * V[0, 0] + od[:, 1] * V[1, 0] + od[:, 2] * V[2, 0]
        t1 = od[:, 0] * V[0, 1] + od[:, 1] * V[1, 1] + od[:, 2] * V[2, 1]
        phi = np.arctan2(t1, t0)
        pos = (phi + np.pi) * float(bins) / (2.0 * np.pi)          # the bin is floor(pos), clamped
        self.out.update(phi=phi, angle_pos=pos)
        return np.bincount(np.clip(np.floor(pos), 0, bins - 1).astype(np.int64), minlength=bins)

    def conc_hist(self, pinv, cmax, bins):
        od, ch = self.od, np.zeros((2, bins + 1), np.int64)
        conc, poss = [], []
        for k in range(2):
            c = od[:, 0] * pinv[k, 0] + od[:, 1] * pinv[k, 1] + od[:, 2] * pinv[k, 2]
            neg = c < 0
            pos = c * float(bins) / cmax[k]
            ch[k, :bins] = np.bincount(np.clip(np.floor(pos[~neg]), 0, bins - 1).astype(np.int64), minlength=bins)
            ch[k, bins] = int(neg.sum())
            conc.append(c); poss.append(pos)
        self.out.update(conc=np.stack(conc), conc_pos=np.stack(poss))
        return ch


def macenko_reference(tiles_u8, beta: float = 0.15, alpha: float = 1.0, bins: int = 4096, target: Optional[MacenkoTarget] = None) -> dict:
    """The definition end to end in fp64 numpy over host tiles uint8 [n, h, w, 3] -> a dict of every intermediate that exists for
    the input: v_max, n_pixels, mask, n, S1, S2, V, phi, angle_pos, angle_hist, phi_lo, phi_hi, HE, cos_angle, pinv, cmax, conc,
    conc_pos, conc_hist, maxC, A, and always on, reason, record and ``stain`` (the SlideStain)."""
    check_params(beta, alpha, bins)
    out: dict = {}
    out["stain"] = _estimate(_NumpyPasses(tiles_u8, out), beta, alpha, int(bins), target or MacenkoTarget(), out)
    return out


class _DevicePasses(_Passes):
    def __init__(self, tiles: torch.Tensor):
        self.t = tiles
        self.n_pixels = tiles.shape[0] * tiles.shape[1] * tiles.shape[2]

    def stats(self, v_max):
        from . import ops
        n, s = ops.stain_stats(self.t, v_max)
        s = s.cpu().numpy()                                           # (the copy synchronises)
        return int(n.cpu()[0]), s[:3].copy(), _sym(s[3:])

    def angle_hist(self, V, v_max, bins):
        from . import ops
        return ops.stain_angle_hist(self.t, V, v_max, bins).cpu().numpy()

    def conc_hist(self, pinv, cmax, bins):
        from . import ops
        return ops.stain_conc_hist(self.t, pinv, cmax, bins).cpu().numpy()


class MacenkoEstimator:
    """``fit(tiles)``: the estimate of one slide from device tiles uint8 [n, h, w, 3] (already cut to the window the encoder
    sees), the three passes on the device (gv_stain_stats / _angle_hist / _conc_hist) with the small host steps between them.
    ``max_tiles`` > 0: only the first ``max_tiles`` tiles are sampled."""

    def __init__(self, device, beta: float = 0.15, alpha: float = 1.0, bins: int = 4096, max_tiles: int = 0, target: Optional[MacenkoTarget] = None):
        check_params(beta, alpha, bins, max_tiles)
        self.dev, self.beta, self.alpha, self.bins, self.max_tiles = torch.device(device), float(beta), float(alpha), int(bins), int(max_tiles)
        self.target = target or MacenkoTarget()

    def fit(self, tiles_u8: torch.Tensor) -> SlideStain:
        if not (isinstance(tiles_u8, torch.Tensor) and tiles_u8.dtype == torch.uint8 and tiles_u8.dim() == 4 and tiles_u8.shape[-1] == 3 and tiles_u8.shape[0] > 0):
            raise ValueError("MacenkoEstimator.fit: expected uint8 tiles [n, h, w, 3] (float tiles cannot be stain-normalised)")
        t = tiles_u8.to(self.dev)
        if self.max_tiles:
            t = t[: self.max_tiles]
        return _estimate(_DevicePasses(t), self.beta, self.alpha, self.bins, self.target, {})


class SlideNormaliser:
    """Keeps a forward-only runner (``engine.FeatureExtractor``) on the current slide's record.  ``begin(data, first_of_slide)`` is
    called with every chunk of tiles as the loader delivers it, before the runner sees it: on a slide's first chunk the estimator
    fits on that chunk's first ``max_tiles`` tiles (0: the whole chunk), cut to the runner's centred window as the monitors cut
    them, and hands the record to the runner; on later chunks the record stays.  ``end()`` takes the record off the runner.  Every
    fallback is counted (``fallbacks``: reason -> slides) and logged once, with the slide and the reason."""

    def __init__(self, runner, estimator: MacenkoEstimator, log: Optional[logging.Logger] = None, primary: bool = True):
        self.runner, self.est, self.log, self.primary = runner, estimator, log or _logger, primary
        self.current: Optional[SlideStain] = None
        self.fallbacks: Counter = Counter()
        self.slides = 0

    def _window(self, data: torch.Tensor) -> torch.Tensor:
        if data.dim() == 5:
            data = data.squeeze(0)
        if data.dtype != torch.uint8 or data.dim() != 4 or data.shape[-1] != 3:
            raise ValueError("stain normalisation works on uint8 NHWC tiles: a transform= hook that delivers float tiles is refused")
        from .knn import centred_window
        return centred_window(data.to(self.runner.dev, non_blocking=True), self.runner.img)

    def begin(self, data: torch.Tensor, first_of_slide: bool, name: str = "") -> SlideStain:
        if first_of_slide or self.current is None:
            st = self.est.fit(self._window(data))
            self.current = st
            self.slides += 1
            if not st.on:
                self.fallbacks[st.reason] += 1
                if self.primary:
                    self.log.warning("stain normalisation: slide %s passes through untouched (%s: %d tissue pixels of %d sampled)",
                                     name or f"#{self.slides}", st.reason, st.n_tissue, st.n_pixels)
            self.runner.set_stain(st.record)
        return self.current

    def end(self) -> None:
        self.current = None
        self.runner.set_stain(None)

    def state(self) -> dict:
        """What ``<slide>_stain.pt`` holds for the current slide."""
        st = self.current
        return dict(HE=torch.from_numpy(np.array(st.HE)), maxC=torch.from_numpy(np.array(st.maxC)), n_tissue=st.n_tissue, on=bool(st.on), reason=st.reason)
