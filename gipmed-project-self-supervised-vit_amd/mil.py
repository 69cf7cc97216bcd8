"""Slide-level attention-MIL probe on frozen teacher features: the third protocol next to the weighted k-NN monitor
(``gipvit/knn.py``) and the linear probe (``gipvit/linprobe.py``), and the one that scores SLIDES rather than tiles.

A slide is a bag of its tiles' features.  Gated-attention ABMIL (Ilse et al. 2018) scores every tile, s_i = w . (tanh(V x_i + bv)
* sigmoid(U x_i + bu)) + bw, pools the bag with a = softmax_i(s), z = sum_i a_i x_i, and classifies z with one linear layer.  No
gradient reaches the features.  It is trained with Adam (cosine factor per epoch as in the linear probe, ``batch`` bags per
step, one permutation of the bags per epoch) by ``ops.mil_train`` -> gv_mil_train; the attention weights a_i and scores s_i per
tile are kept by ``tile_attention`` as the heat maps.  Collecting follows the other two monitors: a tile larger than the
runner's image contributes its centred window, a slide whose label is outside [0, C) is left out; the cached rows come slide by
slide with non-decreasing ordinals, which is the bag table."""
from __future__ import annotations

import logging
import math
from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from .knn import FeatureMonitor
from .linprobe import epoch_permutations, lr_scale_at
from .validate import _auc

f32 = torch.float32
MAX_FEATURES, MAX_HIDDEN, MAX_BATCH, MAX_BAG = 4096, 256, 64, 4096      # gv_mil_train's limits (include/gipvit.h)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def param_count(L: int, C: int, F: int) -> int:
    return (2 * L + C) * F + 3 * L + C + 1


def param_views(params: torch.Tensor, L: int, C: int, F: int) -> "OrderedDict[str, torch.Tensor]":
    """Views into a packed parameter vector (include/gipvit.h: VU | Wc | bv | bu | w | bc | bw) under nn.Linear's names."""
    if params.dim() != 1 or params.shape[0] != param_count(L, C, F):
        raise ValueError(f"param_views: {tuple(params.shape)} is not the packed vector of L = {L}, C = {C}, F = {F}")
    o = (2 * L + C) * F
    return OrderedDict([
        ("attention_V.weight", params[:L * F].view(L, F)), ("attention_V.bias", params[o:o + L]),
        ("attention_U.weight", params[L * F:2 * L * F].view(L, F)), ("attention_U.bias", params[o + L:o + 2 * L]),
        ("attention_w.weight", params[o + 2 * L:o + 3 * L].view(1, L)), ("attention_w.bias", params[o + 3 * L + C:o + 3 * L + C + 1]),
        ("classifier.weight", params[2 * L * F:o].view(C, F)), ("classifier.bias", params[o + 3 * L:o + 3 * L + C])])


def init_params(L: int, C: int, F: int, seed: int) -> torch.Tensor:
    """The packed f32 parameter vector with nn.Linear's default init, U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias,
    every tensor drawn on the host from its own numpy PCG64([seed, k]) stream (k: its place in ``param_views``)."""
    params = torch.zeros(param_count(L, C, F), dtype=f32)
    for k, (name, view) in enumerate(param_views(params, L, C, F).items()):
        fan_in = L if name.startswith("attention_w") else F
        bound = 1.0 / math.sqrt(fan_in)
        draw = np.random.Generator(np.random.PCG64([seed, k])).uniform(-bound, bound, size=tuple(view.shape))
        view.copy_(torch.from_numpy(draw.astype(np.float32)))
    return params


def bag_table(slide_ordinals) -> np.ndarray:
    """int32 [n_bags + 1]: the CSR over rows of bags that are runs of equal ordinals.  The ordinals must not decrease."""
    s = np.asarray(slide_ordinals).reshape(-1)
    if not len(s):
        raise ValueError("bag_table: no rows")
    if (np.diff(s) < 0).any():
        raise ValueError("bag_table: the slide ordinals must be non-decreasing (the rows of a slide are one contiguous bag)")
    starts = np.concatenate([[0], np.nonzero(np.diff(s) != 0)[0] + 1, [len(s)]])
    return starts.astype(np.int32)


def mil_metrics(prob: np.ndarray, labels: np.ndarray, loss: float) -> "OrderedDict[str, float]":
    """prob [n_slides, C], labels [n_slides] in [0, C), loss = the mean cross-entropy -> OrderedDict(mil_top1 in percent over
    slides, mil_loss, and for C > 1 mil_auc_per_slide with prob[:, 1] as the slide score).  Arg-max, the lowest class on a tie."""
    prob = np.asarray(prob, dtype=np.float64)
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    if prob.ndim != 2 or prob.shape[0] != labels.shape[0] or not len(labels):
        raise ValueError(f"mil_metrics: prob {prob.shape} and labels {labels.shape} do not match")
    out = OrderedDict(mil_top1=100.0 * float((np.argmax(prob, axis=1) == labels).mean()), mil_loss=float(loss))
    if prob.shape[1] > 1:
        out["mil_auc_per_slide"] = _auc(labels, prob[:, 1])
    return out


class BagProbe(FeatureMonitor):
    """What the slide-level ABMIL probes share (MilProbe below, ``gipvit/survival.py``'s SurvivalProbe): the settings and their
    refusals, the bag-table check, the Adam run's scaffold, the tile heat maps and the state dict.  A subclass gives
    ``loss_width`` (the sums of a ``loss_sum`` row), ``_epoch`` (one epoch's device call) and ``_epoch_losses`` (the epochs' sums
    -> ``train_loss``), and keeps its own ``_collect``, ``fit``, ``train``, ``predict`` and ``evaluate``; ``self.C`` is the number
    of outputs."""
    loss_width = 1

    def __init__(self, runner, num_classes, hidden, lr, weight_decay, epochs, batch, n_last, seed, primary, log, features, normaliser,
                 runner_needs: Optional[str] = None):
        """``runner_needs``: the refusal of a subclass whose runner came without something it then needs."""
        super().__init__(runner, num_classes, primary, log, normaliser)
        name = type(self).__name__
        if hidden % 16 or not 16 <= hidden <= MAX_HIDDEN:
            raise ValueError(f"{name}: hidden must be a multiple of 16 in 16..{MAX_HIDDEN} (got {hidden})")
        if not (math.isfinite(lr) and lr > 0) or not weight_decay >= 0:
            raise ValueError(f"{name}: need a positive finite lr and weight_decay >= 0 (got {lr}, {weight_decay})")
        if epochs < 1 or not 1 <= batch <= MAX_BATCH:
            raise ValueError(f"{name}: need epochs >= 1 and 1 <= batch <= {MAX_BATCH} (got {epochs}, {batch})")
        if runner is not None:
            depth = runner.vit.depth
            if not 1 <= n_last <= depth:
                raise ValueError(f"{name}: n_last must be in 1..{depth}, the model's depth (got {n_last})")
            if runner_needs:
                raise ValueError(f"{name}: {runner_needs}")
            self.F = n_last * runner.D
        elif features is None:
            raise ValueError(f"{name}: without a runner, pass features=F (the width of the saved feature rows)")
        else:
            self.F = int(features)
        if self.F % 4 or not 4 <= self.F <= MAX_FEATURES:
            raise ValueError(f"{name}: {self.F} features per tile; the kernels take a multiple of 4 in 4..{MAX_FEATURES}")
        self.L, self.lr, self.wd, self.epochs, self.batch = hidden, float(lr), float(weight_decay), epochs, batch
        self.n_last, self.seed = n_last, seed
        self.params = None
        self.train_loss = None

    def _check_bags(self, who: str, feats, bag_ptr):
        name = type(self).__name__
        if feats.dim() != 2 or feats.shape[1] != self.F:
            raise ValueError(f"{name}.{who}: features of shape {tuple(feats.shape)}, expected [N, {self.F}]")
        ptr = np.asarray(bag_ptr).reshape(-1).astype(np.int64)
        if len(ptr) < 2 or ptr[0] != 0 or ptr[-1] != feats.shape[0] or (np.diff(ptr) < 1).any():
            raise ValueError(f"{name}.{who}: bag_ptr must rise from 0 to {feats.shape[0]}, the feature rows, with no empty bag")
        if np.diff(ptr).max() > MAX_BAG:
            raise ValueError(f"{name}.{who}: a bag of {int(np.diff(ptr).max())} tiles; the kernels stop at {MAX_BAG} per slide")
        return ptr.astype(np.int32)

    def _fitted(self, who: str):
        if self.params is None:
            raise RuntimeError(f"{type(self).__name__}.{who}: fit first")

    def _run_epochs(self, feats: torch.Tensor, ptr: np.ndarray, targets):
        """The Adam run on checked inputs: ``ptr`` from ``_check_bags``, ``targets`` the host vectors [n] that ``_epoch`` takes."""
        n, dev = len(ptr) - 1, feats.device
        self.params = init_params(self.L, self.C, self.F, self.seed).to(dev)
        self.m, self.v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        order = torch.from_numpy(epoch_permutations(n, self.epochs, self.seed).astype(np.int32)).to(dev)
        ptr_d, targets = torch.from_numpy(ptr).to(dev), [torch.from_numpy(t).to(dev) for t in targets]
        loss = torch.zeros(self.epochs, self.loss_width, dtype=f32, device=dev)      # row e: epoch e's loss_sum
        max_bag, steps = int(np.diff(ptr).max()), -(-n // self.batch)
        for e in range(self.epochs):
            self._epoch(feats, ptr_d, targets, order[e], loss[e], max_bag, e * steps, lr_scale_at(e, self.epochs))
        self.train_loss = self._epoch_losses(loss.double().cpu().numpy(), n)        # (the copy synchronises)

    def tile_attention(self, loader):
        """Per slide of the loader that was kept, in order: (attn f32 [n_tiles], score f32 [n_tiles]) host tensors -- the tile
        weights after and before the slide's softmax."""
        feats, ptr = self._collect(loader)[:2]
        out = self.predict(feats, ptr, tiles=True)
        attn, score = out["attn"].cpu(), out["score"].cpu()
        return [(attn[ptr[i]:ptr[i + 1]].clone(), score[ptr[i]:ptr[i + 1]].clone()) for i in range(len(ptr) - 1)]

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """Host tensors under the names and shapes of the nn.Linear layers of an ABMIL module."""
        self._fitted("state_dict")
        return OrderedDict((k, v.clone()) for k, v in param_views(self.params.detach().cpu(), self.L, self.C, self.F).items())


class MilProbe(BagProbe):
    """``runner``: an ``engine.FeatureExtractor`` of a CLS-token model.  ``fit(bank_loader)`` then ``evaluate(query_loader)``;
    loaders are ``data.InferTiles`` / ``data.SyntheticSlides``.  ``train(feats, bag_ptr, labels)`` is the device run on its own:
    features read back from <slide>_features.pt files train without an encoder (``runner`` may then be None with ``features=F``)."""
    prefix, metrics, auc_metrics, lower_is_better = "mil_", ("top1", "loss"), ("auc_per_slide",), ("loss",)

    def __init__(self, runner, num_classes: int = 2, hidden: int = 128, lr: float = 5e-4, weight_decay: float = 1e-4, epochs: int = 50,
                 batch: int = 8, n_last: int = 1, seed: int = 0, primary: bool = True, log: Optional[logging.Logger] = None,
                 features: Optional[int] = None, normaliser=None):
        super().__init__(runner, num_classes, hidden, lr, weight_decay, epochs, batch, n_last, seed, primary, log, features, normaliser)

    def _collect(self, loader):
        """-> (features f32 [N, F] device, bag_ptr int32 [n + 1], slide labels int64 [n], slides left out)."""
        feats, labels, slides, skipped = super()._collect(loader)
        ptr = bag_table(slides)
        return feats, ptr, labels[ptr[:-1]], skipped

    def fit(self, bank_loader) -> int:
        """Train a fresh model on the bank's slides.  -> the number of training slides."""
        feats, ptr, labels, skipped = self._collect(bank_loader)
        self.train(feats, ptr, labels)
        if self.primary:
            self.log.info("MIL probe: %d epochs of %d-slide steps on %d slides, %d tiles (%d slides left out: label outside [0, %d)); epoch loss "
                          "%.4f -> %.4f", self.epochs, self.batch, len(labels), feats.shape[0], skipped, self.C, self.train_loss[0], self.train_loss[-1])
        return len(labels)

    def train(self, feats: torch.Tensor, bag_ptr, labels):
        """The Adam run itself on device features f32 [N, F], the bag table [n + 1] and host slide labels [n]: fresh parameters,
        one permutation of the bags per epoch, the cosine factor constant within an epoch.  Leaves ``params`` (packed, device),
        the moments ``m`` / ``v`` and ``train_loss`` ([epochs] mean slide loss per epoch)."""
        ptr = self._check_bags("train", feats, bag_ptr)
        labels = np.asarray(labels).reshape(-1)
        n = len(ptr) - 1
        if labels.shape[0] != n or labels.min() < 0 or labels.max() >= self.C:
            raise ValueError(f"MilProbe.train: {labels.shape[0]} labels for {n} bags, all must be inside [0, {self.C})")
        self._run_epochs(feats, ptr, [labels.astype(np.int32)])

    def _epoch(self, feats, ptr, targets, bags, loss_sum, max_bag, step0, scale):
        from . import ops
        ops.mil_train(self.params, self.m, self.v, feats, ptr, targets[0], bags, loss_sum, self.L, self.C, self.batch, max_bag, step0, self.lr,
                      scale, self.wd, BETA1, BETA2, EPS)

    def _epoch_losses(self, sums, n):
        return (sums.reshape(-1) / n).tolist()

    def predict(self, feats: torch.Tensor, bag_ptr, labels=None, tiles: bool = False):
        """-> ops.mil_predict's dict for the bags of ``feats``."""
        from . import ops
        self._fitted("predict")
        ptr = self._check_bags("predict", feats, bag_ptr)
        dev = feats.device
        y = None if labels is None else torch.from_numpy(np.asarray(labels).astype(np.int32)).to(dev)
        return ops.mil_predict(self.params, feats, torch.from_numpy(ptr).to(dev), self.L, self.C, int(np.diff(ptr).max()), labels=y,
                               want_attn=tiles, want_score=tiles)

    def evaluate(self, loader) -> "OrderedDict[str, float]":
        feats, ptr, labels, skipped = self._collect(loader)
        out = self.predict(feats, ptr, labels)
        metrics = mil_metrics(out["prob"].cpu().numpy(), labels, float(out["loss"].double().cpu()) / len(labels))
        if self.primary:
            self.log.info("MIL probe: %d query slides, %d tiles (%d left out): %s", len(labels), feats.shape[0], skipped,
                          "  ".join(f"{n} {v:.4f}" for n, v in metrics.items()))
        return metrics
