"""Slide-level survival probe on frozen teacher features: the fourth monitor of a ``--dino`` run, next to the k-NN monitor
(``gipvit/knn.py``), the linear probe (``gipvit/linprobe.py``) and the MIL probe (``gipvit/mil.py``), and the one whose target is
a censored time rather than a class -- the reference trainer's default target, ``Survival_Time``.

The model is the MIL probe's gated-attention ABMIL body with one output, the slide's risk theta = Wc . z + bc.  It is trained on
Cox's partial likelihood with right-censoring (Breslow ties) over the ``batch`` slides of a step, with Adam, one permutation of
the bags per epoch and a cosine factor per epoch (``ops.surv_train`` -> gv_surv_train), and scored on the evaluation fold by
Harrell's concordance index and the cohort's partial likelihood in fp64 (``ops.cox_eval`` -> gv_cox_eval).  A slide counts iff
the survival table has it; its class label plays no part.  Definitions: include/gipvit.h.

``cox_reference`` / ``cindex_reference`` / ``surv_metrics`` restate the cohort evaluation in fp64 numpy; the tests hold the
kernels to them.  Pairs with equal times are not comparable here, which differs from lifelines' concordance_index."""
from __future__ import annotations

import logging
import math
from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from .knn import collect_features
from .mil import BETA1, BETA2, EPS, MAX_BAG, MAX_BATCH, MAX_FEATURES, MAX_HIDDEN, BagProbe, bag_table, init_params, param_views

f32 = torch.float32
MAX_COHORT = 65536          # gv_cox_eval's largest cohort


def _valid(risk, time, event):
    risk, time, event = (np.asarray(a).reshape(-1) for a in (risk, time, event))
    if not (risk.shape == time.shape == event.shape):
        raise ValueError(f"risk {risk.shape}, time {time.shape} and event {event.shape} do not match")
    ok = np.isfinite(risk.astype(np.float64)) & np.isfinite(time.astype(np.float64)) & (time >= 0) & ((event == 0) | (event == 1))
    return risk.astype(np.float64)[ok], time.astype(np.float64)[ok], event[ok].astype(np.int64), int((~ok).sum())


def cox_reference(risk, time, event):
    """-> (the sum over the valid events of log sum_{t_j >= t_i} exp(theta_j) - theta_i in fp64, the number of events, the
    number of excluded entries).  An entry with a non-finite risk, a time that is not finite or is negative, or a flag outside
    {0, 1} is excluded."""
    th, t, e, excluded = _valid(risk, time, event)
    if not e.sum():
        return 0.0, 0, excluded
    M = th.max()
    w = np.exp(th - M)
    total = 0.0
    for i in np.nonzero(e)[0]:
        total += math.log(w[t >= t[i]].sum()) + M - th[i]
    return float(total), int(e.sum()), excluded


def cindex_reference(risk, time, event):
    """Harrell's concordance over ordered pairs of valid entries: (i, j) is comparable iff e_i = 1 and t_i < t_j (strict: a pair
    with equal times is not counted), and then concordant / discordant / tied as theta_i >, <, = theta_j.
    -> (C = (concordant + tied / 2) / comparable or nan, comparable, concordant, discordant, tied)."""
    th, t, e, _ = _valid(risk, time, event)
    comp = (e[:, None] == 1) & (t[:, None] < t[None, :])
    conc = int((comp & (th[:, None] > th[None, :])).sum())
    disc = int((comp & (th[:, None] < th[None, :])).sum())
    n = int(comp.sum())
    tied = n - conc - disc
    return ((conc + 0.5 * tied) / n if n else float("nan")), n, conc, disc, tied


def surv_metrics(risk, time, event) -> "OrderedDict[str, float]":
    """-> OrderedDict(surv_cindex, surv_loss): Harrell's C (nan without a comparable pair) and the cohort's partial likelihood
    per event (nan without an event), over the valid entries."""
    total, events, _ = cox_reference(risk, time, event)
    return OrderedDict(surv_cindex=cindex_reference(risk, time, event)[0], surv_loss=total / events if events else float("nan"))


class SurvivalProbe(BagProbe):
    """``runner``: an ``engine.FeatureExtractor`` of a CLS-token model; ``table``: slide name -> (time, event), event 1 =
    observed.  ``fit(bank_loader)`` then ``evaluate(query_loader)``.  ``train(feats, bag_ptr, time, event)`` is the device run on
    its own: features read back from <slide>_features.pt files train without an encoder (``runner`` and ``table`` may then be
    None with ``features=F``)."""
    prefix, metrics, auc_metrics, lower_is_better = "surv_", ("cindex", "loss"), (), ("loss",)
    loss_width = 2

    def __init__(self, runner, table, hidden: int = 128, lr: float = 5e-4, weight_decay: float = 1e-4, epochs: int = 50, batch: int = 32,
                 n_last: int = 1, seed: int = 0, primary: bool = True, log: Optional[logging.Logger] = None, features: Optional[int] = None,
                 normaliser=None, num_classes: int = 1):
        # (num_classes: the monitors' common keyword; one risk output)
        super().__init__(runner, 1, hidden, lr, weight_decay, epochs, batch, n_last, seed, primary, log, features, normaliser,
                         runner_needs=None if table is not None else "with a runner, pass the survival table (slide name -> (time, event))")
        self.table = dict(table or {})
        self._warned = False

    def _collect(self, loader):
        """-> (features f32 [N, F] device, bag_ptr int32 [n + 1], time f32 [n], event int32 [n], slides left out): the slides
        of the loader that the table has."""
        names = list(loader.image_file_names)
        keep = lambda k: k < len(names) and names[k] in self.table
        feats, _, slides, skipped = collect_features(loader, self.C, self.features, type(self).__name__, normaliser=self.normaliser, keep=keep)
        ptr = bag_table(slides)
        rows = [self.table[names[int(slides[s])]] for s in ptr[:-1]]
        return feats, ptr, np.array([r[0] for r in rows], dtype=np.float32), np.array([r[1] for r in rows], dtype=np.int32), skipped

    def fit(self, bank_loader) -> int:
        """Train a fresh model on the bank's slides.  -> the number of training slides."""
        feats, ptr, time, event, skipped = self._collect(bank_loader)
        self.train(feats, ptr, time, event)
        if self.primary:
            self.log.info("survival probe: %d epochs of %d-slide steps on %d slides (%d events), %d tiles (%d slides left out: not in the "
                          "survival table); epoch loss %.4f -> %.4f", self.epochs, self.batch, len(time), int(event.sum()), feats.shape[0], skipped,
                          self.train_loss[0], self.train_loss[-1])
        return len(time)

    def train(self, feats: torch.Tensor, bag_ptr, time, event):
        """The Adam run itself on device features f32 [N, F], the bag table [n + 1] and the host time / event vectors [n]: fresh
        parameters, one permutation of the bags per epoch, the cosine factor constant within an epoch.  Leaves ``params``
        (packed, device), the moments ``m`` / ``v`` and ``train_loss`` ([epochs]: the epoch's event terms over its events)."""
        ptr = self._check_bags("train", feats, bag_ptr)
        time, event = np.asarray(time, dtype=np.float32).reshape(-1), np.asarray(event).reshape(-1)
        n = len(ptr) - 1
        if time.shape[0] != n or event.shape[0] != n or not (np.isfinite(time).all() and (time >= 0).all()) or not np.isin(event, (0, 1)).all():
            raise ValueError(f"SurvivalProbe.train: need {n} finite times >= 0 and {n} event flags in {{0, 1}}")
        if not event.any():
            raise ValueError("SurvivalProbe.train: the bank has no event (every slide is censored): the partial likelihood has no term")
        self._run_epochs(feats, ptr, [time, event.astype(np.int32)])

    def _epoch(self, feats, ptr, targets, bags, loss_sum, max_bag, step0, scale):
        from . import ops
        ops.surv_train(self.params, self.m, self.v, feats, ptr, targets[0], targets[1], bags, loss_sum, self.L, self.batch, max_bag, step0, self.lr,
                       scale, self.wd, BETA1, BETA2, EPS)

    def _epoch_losses(self, sums, n):
        return [float(s / k) if k else float("nan") for s, k in sums]

    def predict(self, feats: torch.Tensor, bag_ptr, tiles: bool = False):
        """-> ops.surv_predict's dict for the bags of ``feats``."""
        from . import ops
        self._fitted("predict")
        ptr = self._check_bags("predict", feats, bag_ptr)
        return ops.surv_predict(self.params, feats, torch.from_numpy(ptr).to(feats.device), self.L, int(np.diff(ptr).max()), want_attn=tiles,
                                want_score=tiles)

    def score(self, risk: torch.Tensor, time, event) -> "OrderedDict[str, float]":
        """surv_cindex / surv_loss of device risks against host times and events (gv_cox_eval; cohorts above its limit on the host)."""
        from . import ops
        if risk.shape[0] > MAX_COHORT:
            return surv_metrics(risk.cpu().numpy(), time, event)
        dev = risk.device
        loss, counts = ops.cox_eval(risk, torch.from_numpy(np.asarray(time, dtype=np.float32)).to(dev),
                                    torch.from_numpy(np.asarray(event).astype(np.int32)).to(dev))
        events, comparable, conc, _, tied, _ = (int(c) for c in counts.cpu())
        return OrderedDict(surv_cindex=(conc + 0.5 * tied) / comparable if comparable else float("nan"),
                           surv_loss=float(loss.cpu()) / events if events else float("nan"))

    def evaluate(self, loader) -> "OrderedDict[str, float]":
        feats, ptr, time, event, skipped = self._collect(loader)
        metrics = self.score(self.predict(feats, ptr)["risk"], time, event)
        if math.isnan(metrics["surv_cindex"]) and not self._warned:
            self._warned = True
            self.log.warning("survival probe: no comparable pair among the %d query slides (an event with a later time elsewhere): surv_cindex is nan",
                             len(time))
        if self.primary:
            self.log.info("survival probe: %d query slides (%d events), %d tiles (%d left out): %s", len(time), int(event.sum()), feats.shape[0],
                          skipped, "  ".join(f"{n} {v:.4f}" for n, v in metrics.items()))
        return metrics
