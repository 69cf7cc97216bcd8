"""Weighted k-NN monitor on frozen teacher features: the training monitor DINO's recipe comes with (``knn_classifier`` of the
paper's eval_knn), for ``--dino`` runs, whose encoder has no classifier head for ``validate()`` to score.

A bank of L2-normalised CLS features with slide labels is built from the training-fold slides, every tile of the evaluation fold
votes with its k most similar bank tiles, weighted exp(sim / temp) (``ops.knn_vote`` -> gv_knn_vote: the Nb x Q similarity
matrix stays on chip).  Reported like ``validate()``: per-tile top-1, AUC per patch and AUC per slide (slide score = mean of its
tile scores).  The features come from a forward-only ``engine.FeatureExtractor`` over the teacher backbone's live weights, so the
bank is rebuilt at every evaluation.  A tile larger than the runner's image (256-px tiles, 224-px global crops) contributes its
centred window."""
from __future__ import annotations

import logging
from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from . import ops
from .validate import _auc

_logger = logging.getLogger("train")
f32 = torch.float32


def tile_slide_metrics(prefix: str, pred: np.ndarray, score: Optional[np.ndarray], labels: np.ndarray, slide_ids) -> "OrderedDict[str, float]":
    """Per-tile predictions pred [N], positive-class scores score [N] (None: one class only), labels [N], slide_ids [N] (any
    hashable per tile; tiles of a slide share one) -> OrderedDict(<prefix>top1 in percent, and with scores <prefix>auc_per_patch,
    <prefix>auc_per_slide): the slide score is the mean of its patch scores, the slide label its first tile's.  Shared by the
    k-NN monitor and the linear probe (gipvit/linprobe.py)."""
    out = OrderedDict()
    out[prefix + "top1"] = 100.0 * float((pred == labels).mean()) if len(labels) else float("nan")
    if score is not None and len(labels):
        out[prefix + "auc_per_patch"] = _auc(labels, score)
        first, inv = {}, np.empty(len(labels), dtype=np.int64)
        for i, s in enumerate(slide_ids):                      # slides in order of first appearance
            inv[i] = first.setdefault(s if not isinstance(s, np.generic) else s.item(), len(first))
        n = len(first)
        mean = np.bincount(inv, weights=score, minlength=n) / np.bincount(inv, minlength=n)
        out[prefix + "auc_per_slide"] = _auc(labels[np.unique(inv, return_index=True)[1]], mean)      # a slide's label: its first tile's
    return out


def knn_metrics(votes: np.ndarray, labels: np.ndarray, slide_ids: np.ndarray) -> "OrderedDict[str, float]":
    """votes [N, C] (>= 0), labels [N] in [0, C), slide_ids [N] (any hashable per tile; tiles of a slide share one) ->
    OrderedDict(knn_top1 in percent, and for C > 1: knn_auc_per_patch, knn_auc_per_slide).  The predicted class is the arg-max
    of the votes, the lowest class on a tie; the patch score is votes[:, 1] / votes.sum(1), the slide score the mean of its
    patch scores, the slide label its first tile's."""
    votes = np.asarray(votes, dtype=np.float64)
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    if votes.ndim != 2 or votes.shape[0] != labels.shape[0] or len(slide_ids) != labels.shape[0]:
        raise ValueError(f"knn_metrics: votes {votes.shape}, labels {labels.shape} and {len(slide_ids)} slide ids do not match")
    score = None
    if votes.shape[1] > 1:
        tot = votes.sum(1)
        score = np.divide(votes[:, 1], tot, out=np.zeros_like(tot), where=tot > 0)
    return tile_slide_metrics("knn_", np.argmax(votes, axis=1), score, labels, slide_ids)


def centred_window(data: torch.Tensor, img: int) -> torch.Tensor:
    """The centred img x img window of larger uint8 tiles (a device slice copy); everything else goes to the runner as it is."""
    if data.dtype == torch.uint8 and data.dim() == 4 and data.shape[1] == data.shape[2] and data.shape[1] > img:
        o = (data.shape[1] - img) // 2
        return data[:, o:o + img, o:o + img, :].contiguous()
    return data


def collect_features(loader, C: int, features, who: str, normaliser=None, keep=None):
    """-> (features f32 [N, D] device, labels int64 [N], slide ordinal int64 [N], slides left out) over the slides whose label
    is inside [0, C); ``features(data)`` maps one chunk of tiles to its f32 [n, D] rows.  ``normaliser``: a
    gipvit.stainnorm.SlideNormaliser over the runner behind ``features`` -- every chunk is announced to it first (a slide begins
    behind the previous ``Is Last Batch``), so the bank and the query pass see stain-normalised tiles; None: nothing changes.
    ``keep``: a predicate over the slide's position in ``loader.image_file_names`` that decides in place of the label (the
    survival probe keeps the slides its table has); None: nothing changes."""
    if hasattr(loader, "reset_counter"):
        loader.reset_counter()
    feats, labels, slides, skipped, ordinal = [], [], [], 0, 0
    first = True
    for mb in loader:
        y = int(mb["Label"].reshape(-1)[0])
        ok = 0 <= y < C if keep is None else bool(keep(ordinal))
        if ok:
            if normaliser is not None:
                normaliser.begin(mb["Data"], first)
                first = False
            f = features(mb["Data"])
            feats.append(f)
            labels.append(np.full(f.shape[0], y, dtype=np.int64))
            slides.append(np.full(f.shape[0], ordinal, dtype=np.int64))
        if mb["Is Last Batch"]:
            skipped += not ok
            ordinal += 1
            first = True
    if normaliser is not None:
        normaliser.end()
    if not feats:
        raise ValueError(f"{who}: no slide with a label in [0, {C}) in the loader" if keep is None else f"{who}: no slide of the loader is kept")
    return torch.cat(feats), np.concatenate(labels), np.concatenate(slides), skipped


class FeatureMonitor:
    """What the k-NN monitor, the linear probe (gipvit/linprobe.py) and the MIL probe (gipvit/mil.py) share; ``fit(bank)`` then ``evaluate(queries)``."""
    prefix, metrics, auc_metrics = "", (), ()   # metric names = prefix + each of: always reported / with more than one class only
    lower_is_better, avgpool = (), False        # those of ``metrics`` where the lower value is the better one; probe_features' pooled vector

    def __init__(self, runner, num_classes: int, primary: bool, log: Optional[logging.Logger], normaliser):
        if not 1 <= num_classes <= 32:
            raise ValueError(f"{type(self).__name__}: num_classes must be in 1..32 (got {num_classes})")
        self.runner, self.C, self.primary, self.log, self.normaliser = runner, num_classes, primary, log or _logger, normaliser

    def metric_names(self):
        return [self.prefix + m for m in self.metrics + (self.auc_metrics if self.C > 1 else ())]

    def _chunk(self, data: torch.Tensor) -> torch.Tensor:      # one chunk of tiles as the runner takes it
        if data.dim() == 5:
            data = data.squeeze(0)
        return centred_window(data.to(self.runner.dev, non_blocking=True), self.runner.img)

    def features(self, data: torch.Tensor) -> torch.Tensor:
        """f32 [n, F] probe features of one chunk of tiles, on the device."""
        return self.runner.probe_features(self._chunk(data), self.n_last, self.avgpool)

    def _collect(self, loader):
        return collect_features(loader, self.C, self.features, type(self).__name__, normaliser=self.normaliser)


class KnnMonitor(FeatureMonitor):
    """``runner``: an ``engine.FeatureExtractor`` (``run(tiles) -> (features f32 [n, D], logits)``).  ``build_bank(loader)`` then
    ``evaluate(loader)``; loaders are ``data.InferTiles`` / ``data.SyntheticSlides``."""
    prefix, metrics, auc_metrics = "knn_", ("top1",), ("auc_per_patch", "auc_per_slide")

    def __init__(self, runner, k: int = 20, temp: float = 0.07, num_classes: int = 2, primary: bool = True, log: Optional[logging.Logger] = None,
                 normaliser=None):
        if not 1 <= k <= 64:
            raise ValueError(f"KnnMonitor: k must be in 1..64 (got {k})")
        if not temp > 0:
            raise ValueError(f"KnnMonitor: temp must be > 0 (got {temp})")
        super().__init__(runner, num_classes, primary, log, normaliser)
        self.k, self.temp = k, temp
        self.bank = self.bank_labels = None

    def features(self, data: torch.Tensor) -> torch.Tensor:
        """L2-normalised f32 [n, D] CLS features of one chunk of tiles, on the device."""
        feats, _ = self.runner.run(self._chunk(data))
        n, D = feats.shape
        out = torch.empty_like(feats)
        ops.l2norm_fwd(feats, out, torch.empty(n, dtype=f32, device=feats.device), n, D)
        return out

    def build_bank(self, loader) -> int:
        feats, labels, slides, skipped = self._collect(loader)
        self.bank = feats
        self.bank_labels = torch.from_numpy(labels.astype(np.int32)).to(feats.device)
        if self.primary:
            self.log.info("k-NN monitor: bank of %d tiles from %d slides (%d slides left out: label outside [0, %d))",
                          feats.shape[0], len(np.unique(slides)), skipped, self.C)
        return feats.shape[0]

    fit = build_bank                # the teacher moved: the bank is rebuilt at every evaluation

    def evaluate(self, loader) -> "OrderedDict[str, float]":
        if self.bank is None:
            raise RuntimeError("KnnMonitor.evaluate: build_bank first")
        feats, labels, slides, skipped = self._collect(loader)
        k = min(self.k, self.bank.shape[0])
        votes = ops.knn_vote(feats, self.bank, self.bank_labels, k, self.temp, self.C)
        metrics = knn_metrics(votes.cpu().numpy(), labels, slides)           # (the copy synchronises)
        if self.primary:
            self.log.info("k-NN monitor: %d query tiles from %d slides (%d left out), k %d, temp %g: %s", feats.shape[0], len(np.unique(slides)),
                          skipped, k, self.temp, "  ".join(f"{n} {v:.4f}" for n, v in metrics.items()))
        return metrics
