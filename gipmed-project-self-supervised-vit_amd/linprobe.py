"""Linear probe on frozen teacher features: the second protocol DINO features are judged by (the paper's eval_linear), next to
the weighted k-NN monitor of ``gipvit/knn.py``.

A grid of linear heads, one per learning rate, is trained with SGD (momentum 0.9, cosine schedule per epoch, rate scaled by
batch / 256) on cached features of the bank slides: the CLS rows of the final norm after each of the last ``n_last`` blocks,
concatenated (``FeatureExtractor.probe_features``).  All heads train in the same pass over the bank (``ops.linprobe_train`` ->
gv_linprobe_train: every head shares one read of every feature row).  With more than one head a share of the bank slides is held
out, by slide, and the head with the lowest mean cross-entropy on their tiles is the one reported.  Reported like ``validate()``:
per-tile top-1 and loss, AUC per patch and AUC per slide (slide score = mean of its tile scores).  Collecting follows the k-NN
monitor: a tile larger than the runner's image contributes its centred window, a slide whose label is outside [0, C) is left
out."""
from __future__ import annotations

import logging
import math
from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .knn import FeatureMonitor, tile_slide_metrics

f32 = torch.float32
MAX_HEAD_COLUMNS, MAX_FEATURES, MAX_BATCH = 64, 4096, 4096      # gv_linprobe_train's limits (include/gipvit.h)
MOMENTUM, INIT_STD = 0.9, 0.01


def holdout_slides(n_slides: int, holdout: float) -> np.ndarray:
    """bool [n_slides]: the slides that go to the selection set.  Slide ordinal i is held out when
    floor((i + 1) * holdout) > floor(i * holdout); if that selects none, the last slide is."""
    if n_slides < 2:
        raise ValueError(f"LinearProbe: choosing among heads needs at least two bank slides (one to train on, one held out), got {n_slides}")
    sel = np.array([math.floor((i + 1) * holdout) > math.floor(i * holdout) for i in range(n_slides)], dtype=bool)
    if not sel.any():
        sel[-1] = True
    return sel


def select_head(losses: Sequence[float]) -> int:
    """The head with the lowest selection loss; ties go to the lower index, a NaN loss never wins."""
    best = 0
    for h, v in enumerate(losses):
        if v < losses[best] or (losses[best] != losses[best] and v == v):
            best = h
    return best


def epoch_permutations(n: int, epochs: int, seed: int) -> np.ndarray:
    """int64 [epochs, n]: one permutation of range(n) per epoch, from numpy's PCG64(seed) -- a function of (n, epochs, seed) only."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.stack([rng.permutation(n) for _ in range(epochs)]) if epochs else np.empty((0, n), dtype=np.int64)


def lr_scale_at(epoch: int, epochs: int) -> float:
    """DINO's per-epoch CosineAnnealingLR(T_max=epochs, eta_min=0) as a factor of the base rate."""
    return 0.5 * (1.0 + math.cos(math.pi * epoch / epochs))


def init_heads(H: int, C: int, F: int, seed: int):
    """(W f32 [H, C, F], b f32 [H, C]): W ~ N(0, 0.01^2) drawn on the host from ``seed``, every head the same draw; b = 0."""
    w = np.random.Generator(np.random.PCG64([seed, 1])).standard_normal((C, F)) * INIT_STD
    return torch.from_numpy(np.broadcast_to(w.astype(np.float32), (H, C, F)).copy()), torch.zeros(H, C, dtype=f32)


def probe_metrics(prob: np.ndarray, labels: np.ndarray, slide_ids, loss: float) -> "OrderedDict[str, float]":
    """prob [N, C] of one head, labels [N] in [0, C), slide_ids [N], loss = the mean cross-entropy -> OrderedDict(linear_top1 in
    percent, linear_loss, and for C > 1: linear_auc_per_patch, linear_auc_per_slide).  The predicted class is the arg-max (the
    lowest class on a tie), the patch score prob[:, 1], the slide score the mean of its tiles', the slide label its first tile's."""
    prob = np.asarray(prob, dtype=np.float64)
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    if prob.ndim != 2 or prob.shape[0] != labels.shape[0] or len(slide_ids) != labels.shape[0]:
        raise ValueError(f"probe_metrics: prob {prob.shape}, labels {labels.shape} and {len(slide_ids)} slide ids do not match")
    m = tile_slide_metrics("linear_", np.argmax(prob, axis=1), prob[:, 1] if prob.shape[1] > 1 else None, labels, slide_ids)
    out = OrderedDict(linear_top1=m.pop("linear_top1"), linear_loss=float(loss))
    out.update(m)
    return out


class LinearProbe(FeatureMonitor):
    """``runner``: an ``engine.FeatureExtractor`` of a CLS-token model.  ``fit(bank_loader)`` then ``evaluate(query_loader)``;
    loaders are ``data.InferTiles`` / ``data.SyntheticSlides``.  ``state_dict(head)`` hands a head out as nn.Linear's."""
    prefix, metrics, auc_metrics, lower_is_better = "linear_", ("top1", "loss"), ("auc_per_patch", "auc_per_slide"), ("loss",)

    def __init__(self, runner, num_classes: int = 2, lrs: Sequence[float] = (0.001,), weight_decay: float = 0.0, epochs: int = 100,
                 batch: int = 1024, n_last: int = 4, avgpool: bool = False, holdout: float = 0.2, seed: int = 0, primary: bool = True,
                 log: Optional[logging.Logger] = None, normaliser=None):
        lrs = tuple(float(v) for v in lrs)
        super().__init__(runner, num_classes, primary, log, normaliser)
        if not lrs or not all(math.isfinite(v) and v > 0 for v in lrs):
            raise ValueError(f"LinearProbe: lrs must be a non-empty list of positive finite rates (got {lrs})")
        if len(lrs) * num_classes > MAX_HEAD_COLUMNS:
            raise ValueError(f"LinearProbe: {len(lrs)} heads x {num_classes} classes is past the kernel's {MAX_HEAD_COLUMNS} logit columns")
        if epochs < 1 or not 1 <= batch <= MAX_BATCH:
            raise ValueError(f"LinearProbe: need epochs >= 1 and 1 <= batch <= {MAX_BATCH} (got {epochs}, {batch})")
        if not weight_decay >= 0 or not 0 < holdout <= 0.5:
            raise ValueError(f"LinearProbe: need weight_decay >= 0 and 0 < holdout <= 0.5 (got {weight_decay}, {holdout})")
        depth = runner.vit.depth
        if not 1 <= n_last <= depth:
            raise ValueError(f"LinearProbe: n_last must be in 1..{depth}, the model's depth (got {n_last})")
        self.F = (n_last + bool(avgpool)) * runner.D
        if self.F > MAX_FEATURES:
            raise ValueError(f"LinearProbe: {self.F} features per tile ({n_last} layers{' + the pooled vector' if avgpool else ''} of width "
                             f"{runner.D}) is past the kernel's {MAX_FEATURES}")
        self.lrs, self.wd, self.epochs, self.batch = lrs, float(weight_decay), epochs, batch
        self.n_last, self.avgpool, self.holdout, self.seed = n_last, bool(avgpool), holdout, seed
        self.H = len(lrs)
        self.W = self.b = None
        self.head = 0
        self.selection_loss = self.train_loss = None

    def fit(self, bank_loader) -> int:
        """Train every head on the bank (minus the held-out slides when there is more than one head) and choose the head to
        report.  -> the number of training tiles."""
        feats, labels, slides, skipped = self._collect(bank_loader)
        order = np.unique(slides)                                      # ordinals of the slides that were kept, ascending
        held = np.zeros(len(labels), dtype=bool)
        if self.H > 1:
            held = np.isin(slides, order[holdout_slides(len(order), self.holdout)])
        train_idx, sel_idx = np.nonzero(~held)[0], np.nonzero(held)[0]
        self.train(feats, labels, train_idx)
        dev = feats.device
        if self.H > 1:
            sel = torch.from_numpy(sel_idx).to(dev)
            _, loss = ops.linprobe_predict(self.W, self.b, feats.index_select(0, sel), torch.from_numpy(labels[sel_idx].astype(np.int32)).to(dev))
            self.selection_loss = (loss.double().cpu().numpy() / len(sel_idx)).tolist()
            self.head = select_head(self.selection_loss)
        else:
            self.selection_loss, self.head = None, 0
        if self.primary:
            self.log.info("linear probe: %d heads x %d epochs on %d tiles from %d slides (%d slides left out: label outside [0, %d)), %d tiles "
                          "of %d slides held out; last-epoch loss %s%s", self.H, self.epochs, len(train_idx), len(order) - len(np.unique(slides[held])),
                          skipped, self.C, len(sel_idx), len(np.unique(slides[held])), " ".join(f"{v:.4f}" for v in self.train_loss[-1]),
                          "" if self.selection_loss is None else "; selection loss " + " ".join(f"{v:.4f}" for v in self.selection_loss)
                          + f" -> head {self.head} (lr {self.lrs[self.head]:g})")
        return len(train_idx)

    def train(self, feats: torch.Tensor, labels: np.ndarray, train_idx: np.ndarray):
        """The SGD run itself on device features f32 [N, F] and host labels [N] over the rows ``train_idx``: fresh heads, one
        permutation of the training rows per epoch, the cosine factor constant within an epoch.  Leaves W, b and
        ``train_loss`` ([epochs][H] mean cross-entropy per epoch)."""
        dev, H, C, F = feats.device, self.H, self.C, self.F
        if feats.shape[1] != F:
            raise ValueError(f"LinearProbe: features of width {feats.shape[1]}, expected {F}")
        labels = np.asarray(labels).reshape(-1)
        if labels.shape[0] != feats.shape[0] or (len(labels) and (labels.min() < 0 or labels.max() >= C)):
            raise ValueError(f"LinearProbe: {labels.shape[0]} labels for {feats.shape[0]} rows, all must be inside [0, {C})")
        train_idx = np.asarray(train_idx, dtype=np.int64)
        if not len(train_idx) or train_idx.min() < 0 or train_idx.max() >= feats.shape[0]:
            raise ValueError(f"LinearProbe: no training rows, or rows outside [0, {feats.shape[0]})")
        W, b = init_heads(H, C, F, self.seed)
        self.W, self.b = W.to(dev), b.to(dev)
        mW, mb = torch.zeros_like(self.W), torch.zeros_like(self.b)
        lr = torch.tensor([v * self.batch / 256.0 for v in self.lrs], dtype=f32, device=dev)
        wd = torch.full((H,), self.wd, dtype=f32, device=dev)
        rows = torch.from_numpy(train_idx[epoch_permutations(len(train_idx), self.epochs, self.seed)].astype(np.int32)).to(dev)
        y = torch.from_numpy(labels.astype(np.int32)).to(dev)
        loss = torch.zeros(self.epochs, H, dtype=f32, device=dev)      # row e: epoch e's loss_sum
        for e in range(self.epochs):
            ops.linprobe_train(self.W, self.b, mW, mb, lr, wd, feats, y, rows[e], loss[e], self.batch, lr_scale_at(e, self.epochs), MOMENTUM)
        self.train_loss = (loss.double().cpu().numpy() / len(train_idx)).tolist()      # (the copy synchronises)

    def evaluate(self, loader) -> "OrderedDict[str, float]":
        if self.W is None:
            raise RuntimeError("LinearProbe.evaluate: fit first")
        feats, labels, slides, skipped = self._collect(loader)
        prob, loss = ops.linprobe_predict(self.W, self.b, feats, torch.from_numpy(labels.astype(np.int32)).to(feats.device))
        prob, loss = prob.cpu().numpy(), loss.double().cpu().numpy() / len(labels)
        metrics = probe_metrics(prob[:, self.head], labels, slides, loss[self.head])
        if self.primary:
            top1 = [100.0 * float((np.argmax(prob[:, h], axis=1) == labels).mean()) for h in range(self.H)]
            for h in range(self.H):
                self.log.info("linear probe: head %d lr %g: selection loss %s, query top-1 %.2f%s", h, self.lrs[h],
                              "n/a" if self.selection_loss is None else f"{self.selection_loss[h]:.4f}", top1[h], "  <- reported" if h == self.head else "")
            self.log.info("linear probe: %d query tiles from %d slides (%d left out): %s", len(labels), len(np.unique(slides)), skipped,
                          "  ".join(f"{n} {v:.4f}" for n, v in metrics.items()))
        return metrics

    def state_dict(self, head: Optional[int] = None) -> "OrderedDict[str, torch.Tensor]":
        """One head as nn.Linear(F, C)'s state (host tensors): the selected head, or head ``head``."""
        if self.W is None:
            raise RuntimeError("LinearProbe.state_dict: fit first")
        h = self.head if head is None else head
        if not 0 <= h < self.H:
            raise ValueError(f"LinearProbe.state_dict: head {h}, there are {self.H}")
        return OrderedDict(weight=self.W[h].detach().cpu().clone(), bias=self.b[h].detach().cpu().clone())
