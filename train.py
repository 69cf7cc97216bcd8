#!/usr/bin/env python3
"""Training driver for the MI355X hot path -- drop-in for the reference's ``train.py`` on the
ViT path only.

    python train.py --model vit_small_patch16_224 --dataset synthetic --num-classes 2 \
        --batch-size 256 --epochs 2 --opt adam --lr-base 0.001 --sched cosine --warmup-epochs 1
    torchrun --nproc_per_node=8 train.py --dino --model vit_small_patch16_224 --batch-size 64 ...

What it keeps from the reference (file:line = /root/reference/train.py):
  * the whole CLI surface (83-393, table in gipvit/cli_spec.py) + ``-c FILE`` YAML defaults (396-410);
  * step order (1037-1078): mixup / cutmix -> forward -> softmax -> LabelSmoothingCE (SoftTargetCE / BCE under mixup or --bce-loss,
    828-846) -> backward -> clip -> optimizer -> model EMA;
  * lr = lr_base * global_batch / 256 (569-581), cosine/step schedule with warm-up (881-887);
  * the ``Train: ep [i/n] Loss .. Time .. rate/s LR .. Data ..`` log line (1096-1111);
  * the epoch loop (905-977): train -> slide-level ``validate`` (933, 1146-1345) -> EMA validate (943-955) ->
    summary.csv -> checkpoint on ``--eval-metric`` (970-973); ``--extract_features`` skips training and writes
    ``./TCGA_500/<slide>_features.pt`` (906, 1281-1282);
  * output folder layout, ``args.yaml``, checkpoint file names / keys incl. ``state_dict_ema`` (854-879);
  * batch dict keys 'Data' / 'Target' (1027-1028) and the ``define_transformations`` hook.
Deliberate deviations: the device is threaded through (the reference is
hard-wired to cuda and unrunnable on CPU -- here a GPU is REQUIRED, there is no CPU fallback);
W&B is optional; the LR is stepped every update with --sched-on-updates (the reference steps it only
inside the log-interval block, 1087/1130-1137); AUC is computed at log time from device-side
probabilities instead of a per-step D2H sync (1054); tiles are sharded over ranks.
``--dino`` adds the DINO multi-crop SSL step the north-star names (absent from the reference).
Every reference flag marked ``used`` in gipvit/cli_spec.py is read below (tests/test_host.py enforces it); a value
this build cannot honour is REJECTED, never silently ignored.
"""
from __future__ import annotations

import os as _os
# The step uses three streams with cross-stream waits (main, the side stream of engine.py, RCCL's
# communication stream).  HIP maps streams onto 4 hardware queues by default and a stream's wait
# blocks everything behind it in a shared queue: measured 20.2 vs 18.2 ms/step with RCCL in the
# picture.  Must be set before the HIP runtime initialises.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import argparse
import csv
import json
import logging
import math
import os
import sys
import time
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from gipvit.checkpoint import HOST_STREAMS, CheckpointSaver, load_checkpoint_file, pack_host_rng, restore_host_rng, stream_seed  # noqa: E402
from gipvit.cli_spec import REFERENCE_FLAGS  # noqa: E402

_logger = logging.getLogger("train")
_TYPES = {"int": int, "float": float, "str": str}


def flag_dest(e) -> str:
    """argparse's dest for a cli_spec entry: explicit ``dest``, else the first long option."""
    if e.get("dest"):
        return e["dest"]
    longs = [f for f in e["flags"] if f.startswith("--")]
    return (longs[0] if longs else e["flags"][0]).lstrip("-").replace("-", "_")


def build_parser():
    cfg = argparse.ArgumentParser(add_help=False)
    cfg.add_argument("-c", "--config", default="", type=str, metavar="FILE")
    p = argparse.ArgumentParser(description="MI355X ViT / DINO trainer (reference-compatible CLI)")
    for e in REFERENCE_FLAGS:
        kw = {k: e[k] for k in ("action", "default", "nargs", "const", "dest") if k in e}
        if "type" in e:
            kw["type"] = _TYPES[e["type"]]
        kw["help"] = ("" if e["used"] else "[accepted, ignored by this build] ") + f"reference train.py:{e['ref']}"
        p.add_argument(*e["flags"], **kw)
    g = p.add_argument_group("MI355X build additions")
    g.add_argument("--dino", action="store_true", help="DINO multi-crop self-supervised step (2 global + N local crops)")
    g.add_argument("--out-dim", type=int, default=65536)
    g.add_argument("--local-crops-number", type=int, default=8)
    g.add_argument("--global-crop-size", type=int, default=224)
    g.add_argument("--local-crop-size", type=int, default=96)
    g.add_argument("--random-crops", action="store_true", help="DINO: random-resized crops + flips cut on the device every step "
                   "(gv_crop_resize); default = the fixed parity windows")
    g.add_argument("--view-augment", action="store_true", help="DINO, with --random-crops: each crop gets its own ColorJitter / grayscale / "
                   "3x3 Gaussian blur / solarisation (DINO's DataAugmentationDINO) in the pass that cuts it (gv_crop_augment)")
    g.add_argument("--color-jitter-p", type=float, default=0.8, help="--view-augment: probability of the ColorJitter(0.4, 0.4, 0.2, 0.1)")
    g.add_argument("--gray-p", type=float, default=0.2, help="--view-augment: probability of a grayscale view")
    g.add_argument("--blur-p", type=float, nargs=3, default=(1.0, 0.1, 0.5), help="--view-augment: blur probability of global crop 1 / 2 / the local crops")
    g.add_argument("--solarize-p", type=float, default=0.2, help="--view-augment: solarisation probability of global crop 2")
    g.add_argument("--stain-jitter", type=float, default=0.0, metavar="SIGMA", help="DINO, with --random-crops --view-augment: H&E stain jitter "
                   "in optical-density space on every crop, in the same pass (gv_crop_augment_stain): per stain (haematoxylin, eosin, residual) "
                   "alpha ~ U(1 - SIGMA, 1 + SIGMA), beta ~ U(-SIGMA, SIGMA); 0 = off, Tellez et al. use 0.05 (light) and 0.2 (strong)")
    g.add_argument("--stain-prob", type=float, default=1.0, metavar="P", help="--stain-jitter: probability that a crop is jittered, 0 < P <= 1")
    g.add_argument("--train-long-seq", action="store_true", help="train on crops past 288 tokens (tiles above 256 px, up to 512 px = 1 025 tokens): "
                   "the attention backward of such a crop streams K / V and Q / dO through LDS (gv_attention_bwd_stream) instead of holding the "
                   "sequence in one workgroup; covers --img-size and the DINO --global-crop-size / --local-crop-size.  16-bit mode only; "
                   "attention maps keep their 288-token limit (their own opt-in: --long-attention-maps)")
    g.add_argument("--stain-normalize", type=str, default="none", metavar="{none,macenko}", help="stain normalisation of every INFERENCE pass of the run "
                   "(validation, --extract_features, the k-NN / linear / MIL monitors' bank and query passes): per slide, Macenko's H&E vectors and "
                   "99th-percentile concentrations are estimated on the device from the slide's first chunk and the slide is mapped onto Macenko's "
                   "reference inside the patchify pass (gv_patchify_stain).  Training batches are never normalised")
    g.add_argument("--stain-norm-tiles", type=int, default=0, metavar="K", help="--stain-normalize: estimate from the first K tiles of a slide's first chunk (0 = the whole chunk)")
    g.add_argument("--stain-norm-beta", type=float, default=0.15, help="--stain-normalize: od threshold of the tissue mask, in (0, ln 256)")
    g.add_argument("--stain-norm-alpha", type=float, default=1.0, help="--stain-normalize: the angle percentiles are alpha and 100 - alpha, alpha in (0, 50)")
    g.add_argument("--global-crops-scale", type=float, nargs=2, default=(0.4, 1.0))
    g.add_argument("--local-crops-scale", type=float, nargs=2, default=(0.05, 0.4))
    g.add_argument("--momentum-teacher", type=float, default=0.996)
    g.add_argument("--teacher-temp", type=float, default=0.04)
    g.add_argument("--warmup-teacher-temp", type=float, default=0.04)
    g.add_argument("--warmup-teacher-temp-epochs", type=int, default=0)
    g.add_argument("--weight-decay-end", type=float, default=0.4)
    g.add_argument("--freeze-last-layer", type=int, default=1, help="epochs during which the head's last layer is not updated")
    g.add_argument("--centering", default="center", choices=("center", "sinkhorn_knopp"), help="DINO: how the teacher's logits are centred -- the "
                   "EMA centre of DINO, or DINOv2's Sinkhorn-Knopp iterations over the step's teacher logits of all ranks (gv_sinkhorn_*)")
    g.add_argument("--sinkhorn-iters", type=int, default=3, help="--centering sinkhorn_knopp: iterations (1..8)")
    g.add_argument("--ibot-weight", type=float, default=0.0, help="DINO: weight of the iBOT masked-patch term (gv_mask_tokens_* / gv_ibot_loss): the "
                   "student sees a learned mask token in place of the marked patches of its global crops and the marked rows go through the "
                   "head a second time; 0 = off, DINOv2 uses 1.0")
    g.add_argument("--ibot-mask-ratio", type=float, nargs=2, default=[0.1, 0.5], metavar=("LO", "HI"), help="--ibot-weight: share of a masked "
                   "image's patches that is marked, 0 < LO <= HI < 1 (DINOv2 mask_ratio_min_max)")
    g.add_argument("--ibot-mask-prob", type=float, default=0.5, help="--ibot-weight: share of the global crops that is masked, 0 < P <= 1 "
                   "(DINOv2 mask_sample_probability)")
    g.add_argument("--koleo-weight", type=float, default=0.0, help="DINO: weight of the KoLeo regulariser on the student's CLS features of "
                   "every global crop (gv_koleo_fwd / gv_koleo_bwd); 0 = off, DINOv2 uses 0.1")
    g.add_argument("--knn-monitor", action="store_true", help="DINO: weighted k-NN classifier on the teacher's frozen features as the training "
                   "monitor (bank = training-fold slides, queries = evaluation fold; gv_knn_vote): eval_knn_top1 / eval_knn_auc_per_patch / "
                   "eval_knn_auc_per_slide in summary.csv, checkpoints chosen on --eval-metric among them")
    g.add_argument("--knn-k", type=int, default=20, help="--knn-monitor: neighbours that vote (1..64)")
    g.add_argument("--knn-temp", type=float, default=0.07, help="--knn-monitor: a neighbour votes with weight exp(similarity / temp)")
    g.add_argument("--knn-bank-tiles", type=int, default=None, help="--knn-monitor: tiles per training slide in the bank (default: --num_tiles)")
    g.add_argument("--knn-rate", type=int, default=1, help="--knn-monitor: evaluate every N epochs")
    g.add_argument("--linear-probe", action="store_true", help="DINO: linear probe on the teacher's frozen features (DINO's eval_linear on cached "
                   "features: bank = training-fold slides, queries = evaluation fold; gv_linprobe_train): eval_linear_top1 / eval_linear_loss / "
                   "eval_linear_auc_per_patch / eval_linear_auc_per_slide in summary.csv")
    g.add_argument("--linprobe-lrs", type=float, nargs="+", default=[0.001], help="--linear-probe: one head per base rate, trained together (a "
                   "head's rate is lr * batch / 256); with more than one the head with the lowest loss on held-out bank slides is reported")
    g.add_argument("--linprobe-epochs", type=int, default=100, help="--linear-probe: passes over the bank (cosine schedule per epoch)")
    g.add_argument("--linprobe-batch", type=int, default=1024, help="--linear-probe: minibatch rows (1..4096)")
    g.add_argument("--linprobe-layers", type=int, default=4, help="--linear-probe: the CLS tokens of the last N blocks are the features")
    g.add_argument("--linprobe-avgpool", action="store_true", help="--linear-probe: append the mean of the last block's patch tokens")
    g.add_argument("--linprobe-wd", type=float, default=0.0, help="--linear-probe: weight decay of the heads")
    g.add_argument("--linprobe-rate", type=int, default=0, help="--linear-probe: 0 = probe after the last epoch only, N >= 1 = every N epochs and the last")
    g.add_argument("--linprobe-holdout", type=float, default=0.2, help="--linear-probe, more than one rate: share of the bank slides held out to "
                   "choose the head on (0 < share <= 0.5)")
    g.add_argument("--mil-probe", action="store_true", help="DINO: slide-level attention-MIL probe on the teacher's frozen features (gated ABMIL "
                   "over each slide's bag of tile features, trained with Adam; bank = training-fold slides, queries = evaluation fold; "
                   "gv_mil_train): eval_mil_top1 / eval_mil_loss / eval_mil_auc_per_slide in summary.csv")
    g.add_argument("--mil-hidden", type=int, default=128, help="--mil-probe: width of the gated attention (a multiple of 16 in 16..256)")
    g.add_argument("--mil-lr", type=float, default=5e-4, help="--mil-probe: Adam's rate (cosine schedule per epoch)")
    g.add_argument("--mil-wd", type=float, default=1e-4, help="--mil-probe: weight decay, added to the gradient")
    g.add_argument("--mil-epochs", type=int, default=50, help="--mil-probe: passes over the bank's slides")
    g.add_argument("--mil-batch", type=int, default=8, help="--mil-probe: slides per step (1..64)")
    g.add_argument("--mil-layers", type=int, default=1, help="--mil-probe: the CLS tokens of the last N blocks are the features")
    g.add_argument("--mil-rate", type=int, default=0, help="--mil-probe: 0 = probe after the last epoch only, N >= 1 = every N epochs and the last")
    g.add_argument("--surv-probe", action="store_true", help="DINO: slide-level survival probe on the teacher's frozen features (the MIL probe's "
                   "gated ABMIL with one risk output, trained on Cox's partial likelihood with right-censoring, gv_surv_train; time and status come "
                   "from labels.csv: time | 'Time (months)' and censored | Censored | event): eval_surv_cindex / eval_surv_loss in summary.csv")
    g.add_argument("--surv-hidden", type=int, default=128, help="--surv-probe: width of the gated attention (a multiple of 16 in 16..256)")
    g.add_argument("--surv-lr", type=float, default=5e-4, help="--surv-probe: Adam's rate (cosine schedule per epoch)")
    g.add_argument("--surv-wd", type=float, default=1e-4, help="--surv-probe: weight decay, added to the gradient")
    g.add_argument("--surv-epochs", type=int, default=50, help="--surv-probe: passes over the bank's slides")
    g.add_argument("--surv-batch", type=int, default=32, help="--surv-probe: slides per step (1..64); a step's slides are each other's risk sets")
    g.add_argument("--surv-layers", type=int, default=1, help="--surv-probe: the CLS tokens of the last N blocks are the features")
    g.add_argument("--surv-rate", type=int, default=0, help="--surv-probe: 0 = probe after the last epoch only, N >= 1 = every N epochs and the last")
    g.add_argument("--tile-size", type=int, default=256)
    g.add_argument("--batches-per-epoch", type=int, default=100, help="synthetic source only")
    g.add_argument("--synthetic-slides", type=int, default=4, help="synthetic source only: slides of the inference set")
    g.add_argument("--no-validate", action="store_true", help="skip the per-epoch slide-level validation")
    g.add_argument("--features-dir", default="./TCGA_500", help="where --extract_features writes <slide>_features.pt (train.py:1282)")
    g.add_argument("--extract-attention", action="store_true", help="with --extract_features: also write <slide>_attention.pt, f32 "
                   "[n_tiles, heads, N] = the CLS query's last-block attention over every token (get_last_selfattention row 0); "
                   "[:, :, 1:] reshaped to (img/16, img/16) is DINO's attention map")
    g.add_argument("--long-attention-maps", action="store_true", help="with --extract_features --extract-attention: attention maps of tiles above "
                   "256 px, up to 512 px = 1 025 tokens (gv_attention_probs_stream: the CLS row is recomputed from the streaming forward's "
                   "log-sum-exp without holding the sequence in one workgroup).  16-bit mode only; not for --dino --extract_features, "
                   "which extracts such maps on the supervised route from an --initial-checkpoint")
    g.add_argument("--device", default="cuda", help="must be a GPU: the hot path has no CPU fallback")
    g.add_argument("--precision", default="bf16", choices=("bf16", "fp32"), help="bf16: bf16 GEMM / attention operands, f32 accumulation, f32 "
                   "residual stream and master weights (the training path).  fp32: every operand f32 -- the reference's arithmetic "
                   "without --amp; a verification mode, an order of magnitude slower")
    return cfg, p


def parse_args(argv=None):
    cfg, p = build_parser()
    known, remaining = cfg.parse_known_args(argv)
    from_file = {}
    if known.config:
        with open(known.config) as f:
            from_file = yaml.safe_load(f) or {}
            p.set_defaults(**from_file)
    args = p.parse_args(remaining)
    # --dino (this build's addition) changes the DEFAULT of --opt from the reference's 'sgd' to the recipe's 'adamw'; an --opt the
    # user did pass is never replaced (check_supported refuses what the DINO step cannot honour)
    if args.dino and "opt" not in from_file and not any(a == "--opt" or a.startswith("--opt=") for a in remaining):
        args.opt = "adamw"
    return args, yaml.safe_dump(vars(args), default_flow_style=False)


SUPPORTED_OPTS = ("sgd", "adam", "adamw", "lamb")  # modes of gv_adamw_ema (sgd = momentum + nesterov, timm's default for 'sgd') + gv_lamb
SUPPORTED_SCHEDS = ("cosine", "step")               # gipvit/sched.py
LOWER_IS_BETTER = ("loss", "linear_loss", "mil_loss")     # train.py:866: the --eval-metric values where the lower checkpoint is the better one
SURV_LOWER_IS_BETTER = ("surv_loss",)                     # the survival probe's, consulted beside it


def dino_loss_options(args) -> dict:
    """The DINOv2 loss options of the command line as DinoEngine's keyword arguments."""
    return dict(centering=args.centering, sinkhorn_iters=args.sinkhorn_iters, koleo_weight=args.koleo_weight)


def ibot_options(args) -> dict:
    """The iBOT flags of the command line as DinoEngine's keyword arguments."""
    return dict(ibot_weight=args.ibot_weight, ibot_mask_ratio=tuple(args.ibot_mask_ratio), ibot_mask_prob=args.ibot_mask_prob, drop=args.drop or 0.0)


def check_ibot(args):
    """--ibot-weight / --ibot-mask-ratio / --ibot-mask-prob: refused before any GPU work (DinoEngine's constructor says the same)."""
    lo, hi = args.ibot_mask_ratio
    given = [f for f, on in (("--ibot-weight", args.ibot_weight != 0), ("--ibot-mask-ratio", [lo, hi] != [0.1, 0.5]),
                             ("--ibot-mask-prob", args.ibot_mask_prob != 0.5)) if on]
    if given and not args.dino:
        raise SystemExit(f"{' / '.join(given)}: the iBOT term belongs to the DINO step, it needs --dino")
    if not (math.isfinite(args.ibot_weight) and args.ibot_weight >= 0):
        raise SystemExit(f"--ibot-weight {args.ibot_weight}: a finite weight >= 0")
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi < 1.0):
        raise SystemExit(f"--ibot-mask-ratio {lo} {hi}: need 0 < LO <= HI < 1")
    if not (math.isfinite(args.ibot_mask_prob) and 0.0 < args.ibot_mask_prob <= 1.0):
        raise SystemExit(f"--ibot-mask-prob {args.ibot_mask_prob}: need 0 < P <= 1")
    if args.ibot_weight > 0:
        if args.global_crop_size < 64:
            raise SystemExit(f"--ibot-weight with --global-crop-size {args.global_crop_size}: the mask blocks need a 4 x 4 patch grid, 64 px at least")
        if args.drop:
            raise SystemExit("--ibot-weight with --drop: the dropout path has no all-token last block with a row table; not built")
        if args.amp and args.amp_dtype != "bfloat16":
            raise SystemExit("--ibot-weight with --amp --amp-dtype float16: the iBOT term is not built for the float16 library; pass --amp-dtype bfloat16")
        if args.centering == "sinkhorn_knopp":
            raise SystemExit("--ibot-weight with --centering sinkhorn_knopp: Sinkhorn-Knopp over a patch-row count that varies per rank is not built, "
                             "and the EMA patch centre in its place would be a silent substitution")


def check_supported(args, log=_logger.warning):
    """Reference flags whose value this build cannot honour are rejected loudly; the ones it maps onto its own
    arithmetic are explained once.  Returns the resolved image size (or None)."""
    if args.drop and not 0.0 <= args.drop < 1.0:
        raise SystemExit(f"--drop {args.drop}: dropout needs 0 <= rate < 1 (reference train.py:283-284, vit.pyc@L98-131)")
    if args.drop_path is not None and not 0.0 <= args.drop_path < 1.0:
        raise SystemExit(f"--drop-path {args.drop_path}: stochastic depth needs 0 <= rate < 1 (reference train.py:287-288, vit.pyc@L66-74)")
    if args.drop_connect:
        raise SystemExit("--drop-connect is the deprecated spelling of --drop-path (reference train.py:285-286): pass --drop-path")
    if args.pretrained and not args.initial_checkpoint:
        raise SystemExit("--pretrained downloads weights by URL (reference train.py:482-485): there is no network here -- "
                         "pass the file with --initial-checkpoint instead")
    if args.clip_mode not in ("norm", "value", "agc"):
        raise SystemExit(f"--clip-mode {args.clip_mode}: 'norm' (global norm, the reference default), 'value' (element-wise clamp) or 'agc' (adaptive, "
                         "per unit) -- the three modes of timm's dispatch_clip_grad (train.py:1072-1077)")
    if args.clip_mode == "agc" and args.dino:
        raise SystemExit("--clip-mode agc with --dino is not built (the reference applies it to a supervised model minus its classifier)")
    if args.clip_mode == "value" and args.opt.lower() == "lamb":
        raise SystemExit("--clip-mode value with --opt lamb is not built (Lamb's own global-norm clip needs the norm of the clamped gradient)")
    if args.opt.lower() not in SUPPORTED_OPTS:
        raise SystemExit(f"--opt {args.opt}: the fused optimizer kernel (csrc/optim.hip) implements {' / '.join(SUPPORTED_OPTS)}; timm's other "
                         "create_optimizer_v2 choices (reference train.py:161, 583) are not built and nothing is substituted for them")
    if args.dino and args.opt.lower() != "adamw":
        raise SystemExit(f"--dino --opt {args.opt}: the DINO step is AdamW with the recipe's weight-decay schedule (paper; the frozen-last-layer and "
                         "teacher-EMA ranges are fused into that pass); pass --opt adamw")
    if args.gp is not None:
        # train.py:122 -> create_model(global_pool=args.gp), train.py:490: the encoder's pooling
        if args.gp not in ("token", "avg"):
            raise SystemExit(f"--gp {args.gp!r}: 'token' (the CLS token, the default) or 'avg' (mean of the patch tokens + fc_norm); "
                             + ("'' would hand every token to the head, which the reference's loss cannot take"
                                if args.gp == "" else "timm's ViT has no other pooling"))
        if args.gp == "avg" and args.dino:
            raise SystemExit("--gp avg with --dino: the DINO step reads the CLS token; mean pooling is the supervised model's (fine-tune "
                             "a DINO checkpoint with --gp avg --initial-checkpoint)")
    if args.layer_decay is not None:
        # train.py:175 -> timm param_groups_layer_decay: every layer below the classifier at layer_decay times the rate of the one above
        if not args.layer_decay > 0:
            raise SystemExit(f"--layer-decay {args.layer_decay}: the per-layer rate scale is layer_decay ** k, it must be > 0")
        if args.dino:
            raise SystemExit("--dino --layer-decay is not built: the DINO step keeps its recipe (one rate for the student, the frozen-last-layer and "
                             "teacher-EMA ranges fused into its pass); --layer-decay is the supervised fine-tuning knob")
    if args.sched.lower() not in SUPPORTED_SCHEDS:
        raise SystemExit(f"--sched {args.sched}: this build steps the learning rate by {' / '.join(SUPPORTED_SCHEDS)} (+ linear warm-up); timm's other "
                         "create_scheduler_v2 choices (reference train.py:180, 881-887) are not built and a constant rate is not substituted")
    if args.in_chans not in (None, 3):
        raise SystemExit(f"--in-chans {args.in_chans}: the patch-embedding kernel reads 3-channel NHWC uint8 tiles")
    img = None
    if args.input_size:
        c, h, w = args.input_size
        if c != 3 or h != w or h % 16:
            raise SystemExit(f"--input-size {args.input_size}: need 3 x S x S with S a multiple of 16")
        img = h
    if args.amp and args.amp_dtype.lower() not in ("float16", "fp16", "bfloat16", "bf16"):
        raise SystemExit(f"--amp-dtype {args.amp_dtype}: 'float16' (the reference default, train.py:332) or 'bfloat16'")
    if amp_is_f16(args):
        # the same kernels built with IEEE half as the 16-bit format (libgipvit_hip_f16.so) + torch's GradScaler on the device
        if args.opt.lower() == "lamb" or args.clip_mode == "agc":
            raise SystemExit("--amp --amp-dtype float16: dynamic loss scaling is built for adamw / adam / sgd with --clip-mode norm | value; "
                             "run --opt lamb / --clip-mode agc with --amp-dtype bfloat16")
    elif not args.amp and args.precision != "fp32":
        log("no --amp: the reference would compute in fp32 (train.py:452-465); this build's GEMMs take bf16 operands with f32 "
            "accumulation, f32 residual stream and f32 master weights (the --amp --amp-dtype bfloat16 arithmetic) unless "
            "--precision fp32 is given")
    if args.amp and args.precision == "fp32":
        raise SystemExit("--amp asks for mixed precision, --precision fp32 for f32 operands throughout: pick one")
    if args.view_augment and not (args.dino and args.random_crops):
        raise SystemExit("--view-augment augments the crops that --dino --random-crops cuts on the device: pass both")
    if not (math.isfinite(args.stain_jitter) and 0 <= args.stain_jitter < 1):
        raise SystemExit(f"--stain-jitter {args.stain_jitter}: sigma must be finite and in [0, 1) (alpha ~ U(1 - sigma, 1 + sigma) has to stay positive)")
    if not 0 < args.stain_prob <= 1:
        raise SystemExit(f"--stain-prob {args.stain_prob}: the share of jittered crops, 0 < P <= 1")
    if args.stain_jitter > 0 and not (args.dino and args.random_crops and args.view_augment):
        raise SystemExit("--stain-jitter runs inside the view-augmentation pass of the crops (gv_crop_augment_stain): "
                         "pass --dino --random-crops --view-augment with it")
    if args.extract_attention and not args.extract_features:
        raise SystemExit("--extract-attention writes <slide>_attention.pt next to the features: it needs --extract_features")
    if args.knn_monitor:
        if not args.dino:
            raise SystemExit("--knn-monitor scores the DINO teacher's frozen features: it needs --dino (a supervised run has validate())")
        if not 1 <= args.knn_k <= 64:
            raise SystemExit(f"--knn-k {args.knn_k}: the vote kernel keeps 1..64 neighbours per query (gv_knn_vote)")
        if not args.knn_temp > 0:
            raise SystemExit(f"--knn-temp {args.knn_temp}: the vote weight is exp(similarity / temp), temp must be > 0")
        if args.knn_rate < 1:
            raise SystemExit(f"--knn-rate {args.knn_rate}: evaluate every N >= 1 epochs")
        if args.knn_bank_tiles is not None and args.knn_bank_tiles < 1:
            raise SystemExit(f"--knn-bank-tiles {args.knn_bank_tiles}: tiles per training slide in the bank, >= 1")
        if args.eval_metric == "loss":
            raise SystemExit("--eval-metric loss with --knn-monitor: the monitor reports top1 / auc_per_patch / auc_per_slide (no loss); "
                             "pick one of them")
        if args.test_fold in (-1, "-1"):
            raise SystemExit("--test_fold -1 with --knn-monitor: no evaluation fold is left to query the bank with")
        if args.tile_size < args.global_crop_size:
            raise SystemExit(f"--knn-monitor: the teacher sees {args.global_crop_size}-px images, the centred window of a {args.tile_size}-px "
                             "tile (--tile-size) cannot be smaller than that")
    if args.linear_probe:
        if not args.dino:
            raise SystemExit("--linear-probe scores the DINO teacher's frozen features: it needs --dino (a supervised run has validate())")
        lrs = list(args.linprobe_lrs or [])
        if not lrs or not all(math.isfinite(v) and v > 0 for v in lrs):
            raise SystemExit(f"--linprobe-lrs {lrs}: one positive finite base rate per head, at least one")
        if len(lrs) * (args.num_classes or 2) > 64:
            raise SystemExit(f"--linprobe-lrs: {len(lrs)} heads x {args.num_classes or 2} classes is past the 64 logit columns of gv_linprobe_train")
        if args.linprobe_epochs < 1:
            raise SystemExit(f"--linprobe-epochs {args.linprobe_epochs}: at least one pass over the bank")
        if not 1 <= args.linprobe_batch <= 4096:
            raise SystemExit(f"--linprobe-batch {args.linprobe_batch}: 1 .. 4096 rows per step (gv_linprobe_train)")
        from gipvit.archs import ARCHS, resolve_arch       # plain tables: nothing is loaded for them
        spec = ARCHS[resolve_arch(args.model)]
        if not 1 <= args.linprobe_layers <= spec["depth"]:
            raise SystemExit(f"--linprobe-layers {args.linprobe_layers}: the last 1 .. {spec['depth']} blocks of {args.model}")
        width = (args.linprobe_layers + bool(args.linprobe_avgpool)) * spec["embed_dim"]
        if width > 4096:
            raise SystemExit(f"--linprobe-layers {args.linprobe_layers}{' --linprobe-avgpool' if args.linprobe_avgpool else ''}: {width} features per "
                             f"tile at width {spec['embed_dim']}, gv_linprobe_train stops at 4096")
        if not args.linprobe_wd >= 0:
            raise SystemExit(f"--linprobe-wd {args.linprobe_wd}: weight decay must be >= 0")
        if args.linprobe_rate < 0:
            raise SystemExit(f"--linprobe-rate {args.linprobe_rate}: 0 = after the last epoch only, N >= 1 = every N epochs and the last")
        if not 0 < args.linprobe_holdout <= 0.5:
            raise SystemExit(f"--linprobe-holdout {args.linprobe_holdout}: the share of bank slides held out, 0 < share <= 0.5")
        if args.test_fold in (-1, "-1"):
            raise SystemExit("--test_fold -1 with --linear-probe: no evaluation fold is left to score the heads on")
        if args.tile_size < args.global_crop_size:
            raise SystemExit(f"--linear-probe: the teacher sees {args.global_crop_size}-px images, the centred window of a {args.tile_size}-px "
                             "tile (--tile-size) cannot be smaller than that")
        names = monitor_metric_names(args)
        if resolve_eval_metric(args.eval_metric, bool(args.knn_monitor), True, bool(args.mil_probe)) not in names:
            raise SystemExit(f"--eval-metric {args.eval_metric}: the monitors of this run report {names} (a bare name is the k-NN monitor's "
                             "when that is on, else the probe's)")
    if args.mil_probe:
        check_bag_probe(args, "mil", "",
                        lambda: resolve_eval_metric(args.eval_metric, bool(args.knn_monitor), bool(args.linear_probe), True))
    if getattr(args, "surv_probe", False):
        check_surv_probe(args)
    check_ibot(args)
    # the DINOv2 loss options belong to the DINO step
    if not args.dino and (args.centering != "center" or args.koleo_weight != 0):
        raise SystemExit("--centering sinkhorn_knopp / --koleo-weight change the DINO step's loss: they need --dino")
    if not (math.isfinite(args.koleo_weight) and args.koleo_weight >= 0):
        raise SystemExit(f"--koleo-weight {args.koleo_weight}: a finite weight >= 0")
    if not 1 <= args.sinkhorn_iters <= 8:
        raise SystemExit(f"--sinkhorn-iters {args.sinkhorn_iters}: 1 .. 8 iterations")
    if args.koleo_weight > 0 and args.batch_size < 2:
        raise SystemExit(f"--koleo-weight {args.koleo_weight} with --batch-size {args.batch_size}: KoLeo takes every tile's nearest neighbour among "
                         "the other tiles of its crop on this GPU, it needs at least 2")
    if args.supervised and args.dino:
        raise SystemExit("--supervised (fine-tune with labels, train.py:715-717) and --dino (self-supervised) exclude each other")
    # mixup / cutmix / BCE (train.py:752-771, 828-846): the supervised step's batch, target and loss
    given = [f for f, on in (("--mixup", args.mixup), ("--cutmix", args.cutmix), ("--cutmix-minmax", args.cutmix_minmax is not None),
                             ("--mixup-prob", args.mixup_prob != 1.0), ("--mixup-switch-prob", args.mixup_switch_prob != 0.5),
                             ("--mixup-mode", args.mixup_mode != "batch"), ("--mixup-off-epoch", args.mixup_off_epoch),
                             ("--bce-loss", args.bce_loss), ("--bce-target-thresh", args.bce_target_thresh is not None)) if on]
    if args.dino and given:
        raise SystemExit(f"{' '.join(given)} with --dino: mixup / cutmix and the soft-target / BCE losses belong to the supervised step "
                         "(train.py:752-771, 828-846); the DINO loss takes no labels")
    if args.mixup < 0 or args.cutmix < 0:
        raise SystemExit(f"--mixup {args.mixup} --cutmix {args.cutmix}: the Beta distribution's alpha must be >= 0 (0 = off)")
    if args.mixup_mode not in ("batch", "pair", "elem"):
        raise SystemExit(f"--mixup-mode {args.mixup_mode}: 'batch', 'pair' or 'elem' (train.py:275-276)")
    if args.cutmix_minmax is not None:
        mm = list(args.cutmix_minmax)
        if len(mm) != 2 or not (0.0 < mm[0] < mm[1] <= 1.0):
            raise SystemExit(f"--cutmix-minmax {mm}: two values in (0, 1], strictly ascending (min and max side of the box as a share of the image)")
    if not 0.0 <= args.mixup_prob <= 1.0 or not 0.0 <= args.mixup_switch_prob <= 1.0:
        raise SystemExit("--mixup-prob / --mixup-switch-prob are probabilities: 0 <= p <= 1")
    if mix_active(args) and args.batch_size % 2:
        raise SystemExit(f"--batch-size {args.batch_size} with mixup / cutmix: image i is mixed with image B - 1 - i, the batch size must be even")
    if args.bce_loss and not mix_active(args) and not args.smoothing:
        log("--bce-loss with --smoothing 0 and no mixup: the reference selects plain cross-entropy there (train.py:838-844); so does this build")
    # random erasing (timm_train.py:621-624 -> timm's loader; train.py:788-791 has the call commented out): the supervised step's batch
    given = [f for f, on in (("--reprob", args.reprob), ("--remode", args.remode != "pixel"), ("--recount", args.recount != 1)) if on]
    if args.dino and given:
        raise SystemExit(f"{' '.join(given)} with --dino: random erasing belongs to the supervised step (timm's loader applies it to the "
                         "labelled batch); the DINO crops have their own augmentation (--view-augment)")
    if not 0.0 <= args.reprob <= 1.0:
        raise SystemExit(f"--reprob {args.reprob} is a probability: 0 <= p <= 1 (0 = off)")
    if args.remode not in ("pixel", "rand", "const"):
        raise SystemExit(f"--remode {args.remode}: 'pixel' (per-pixel noise), 'rand' (one random colour per box) or 'const' (zeros)")
    if not 1 <= args.recount <= 8:
        raise SystemExit(f"--recount {args.recount}: 1 .. 8 boxes per image (the erase table's row holds GV_ERASE_MAX_BOXES = 8)")
    return img


ATTN_TRAIN_MAX_TOKENS = 288     # gv_attention_bwd / gv_attention_probs hold one sequence in LDS (include/gipvit.h)
ATTN_STREAM_MAX_TOKENS = 1040   # gv_attention_fwd_stream; gv_attention_bwd_stream behind --train-long-seq, gv_attention_probs_stream behind --long-attention-maps
ATTN_F32_MAX_TOKENS = 260       # the fp32 operand mode's attention


def check_stain_normalize(args):
    """--stain-normalize and its options, refused before any GPU work (main calls this ahead of the device check)."""
    if args.stain_normalize not in ("none", "macenko"):
        raise SystemExit(f"--stain-normalize {args.stain_normalize}: 'none' or 'macenko' (Vahadane is not built)")
    if not (math.isfinite(args.stain_norm_beta) and 0 < args.stain_norm_beta < math.log(256.0)):
        raise SystemExit(f"--stain-norm-beta {args.stain_norm_beta}: the od threshold of the tissue mask must be in (0, ln 256)")
    if not (math.isfinite(args.stain_norm_alpha) and 0 < args.stain_norm_alpha < 50):
        raise SystemExit(f"--stain-norm-alpha {args.stain_norm_alpha}: the angle percentile must be in (0, 50)")
    if args.stain_norm_tiles < 0:
        raise SystemExit(f"--stain-norm-tiles {args.stain_norm_tiles}: K >= 0 (0 = the whole first chunk of a slide)")


def check_token_limits(args):
    """Image sizes against the attention kernels' sequence limits, before any device work: a run that TRAINS needs every crop within
    288 tokens (256 px at patch 16); --extract_features on the supervised route is forward-only and goes up to 512 px
    (gv_attention_fwd_stream); --extract-attention, --dino --extract_features (it builds the DINO training engine) and
    --precision fp32 keep the 288- / 260-token limits.  --train-long-seq lifts the limit of a training run to 1 040 tokens (512 px:
    gv_attention_bwd_stream), in the 16-bit mode; --long-attention-maps lifts the limit of --extract-attention on the supervised route to the
    same 1 040 tokens (gv_attention_probs_stream), in the 16-bit mode; everything else keeps its limit and, without the flags, its message."""
    tokens = lambda px: (px // 16) ** 2 + 1
    long_seq = getattr(args, "train_long_seq", False)
    long_maps = getattr(args, "long_attention_maps", False)
    if long_maps and not (args.extract_features and args.extract_attention):
        raise SystemExit("--long-attention-maps lifts the limit of --extract_features --extract-attention (attention maps of tiles above 256 px): "
                         "it needs both")
    if args.dino:
        sizes = [("--global-crop-size", args.global_crop_size)] + ([("--local-crop-size", args.local_crop_size)] if args.local_crops_number else [])
    else:
        sizes = [("image size (--img-size / --input-size / --tile-size)", args.img_size or (args.input_size[1] if args.input_size else None) or args.tile_size)]
    for flag, px in sizes:
        n = tokens(px)
        if args.dino and args.extract_features and n > ATTN_TRAIN_MAX_TOKENS:
            raise SystemExit(f"--dino --extract_features with {flag} {px}: {n} tokens per image, the DINO route builds its training engine and stops at "
                             f"{ATTN_TRAIN_MAX_TOKENS} tokens (256 px at patch 16); extract features above that on the supervised route")
        if not args.extract_features and long_seq:
            if n > ATTN_STREAM_MAX_TOKENS:
                raise SystemExit(f"--train-long-seq with {flag} {px}: {n} tokens per image, the streaming attention stops at {ATTN_STREAM_MAX_TOKENS} "
                                 f"tokens (512 px at patch 16)")
            if args.precision == "fp32" and n > ATTN_F32_MAX_TOKENS:
                raise SystemExit(f"--train-long-seq --precision fp32 with {flag} {px}: {n} tokens per image, the fp32 operand mode's attention stops at "
                                 f"{ATTN_F32_MAX_TOKENS} tokens (256 px) and has no streaming form; long sequences train in the 16-bit mode")
        elif not args.extract_features and n > ATTN_TRAIN_MAX_TOKENS:
            raise SystemExit(f"{flag} {px}: {n} tokens per image, training stops at {ATTN_TRAIN_MAX_TOKENS} tokens (256 px at patch 16: the attention "
                             f"backward holds a whole sequence in LDS); larger tiles run forward-only -- --extract_features, up to 512 px")
        if long_maps and n > ATTN_STREAM_MAX_TOKENS:
            raise SystemExit(f"--long-attention-maps with {flag} {px}: {n} tokens per image, the streaming attention maps stop at "
                             f"{ATTN_STREAM_MAX_TOKENS} tokens (512 px at patch 16)")
        if args.extract_features and args.extract_attention and n > ATTN_TRAIN_MAX_TOKENS and not long_maps:
            raise SystemExit(f"--extract-attention with {flag} {px}: {n} tokens per image, attention maps stop at {ATTN_TRAIN_MAX_TOKENS} tokens "
                             f"(256 px at patch 16); the features themselves work up to 512 px")
        if args.extract_features and n > ATTN_STREAM_MAX_TOKENS:
            raise SystemExit(f"{flag} {px}: {n} tokens per image, the streaming attention forward stops at {ATTN_STREAM_MAX_TOKENS} tokens (512 px at patch 16)")
        if args.extract_features and args.precision == "fp32" and n > ATTN_F32_MAX_TOKENS:
            raise SystemExit(f"--precision fp32 with {flag} {px}: {n} tokens per image, the fp32 operand mode's attention stops at "
                             f"{ATTN_F32_MAX_TOKENS} tokens (256 px); larger tiles run in the 16-bit mode")


def check_bag_probe(args, key, metric_hint, resolve):
    """The refusals --mil-probe and --surv-probe share, all before any GPU work and in one order.  ``key``: mil | surv, the
    prefix of the probe's flags and of its gv_<key>_train; ``metric_hint``: what the --eval-metric refusal adds for this probe; ``resolve``:
    the run's --eval-metric resolved with this probe on."""
    flag, entry = f"--{key}-probe", f"gv_{key}_train"
    opt = lambda name: getattr(args, f"{key}_{name}")
    if not args.dino:
        raise SystemExit(f"{flag} scores the DINO teacher's frozen features: it needs --dino (a supervised run has validate())")
    if opt("hidden") % 16 or not 16 <= opt("hidden") <= 256:
        raise SystemExit(f"--{key}-hidden {opt('hidden')}: a multiple of 16 in 16 .. 256 ({entry})")
    if not (math.isfinite(opt("lr")) and opt("lr") > 0):
        raise SystemExit(f"--{key}-lr {opt('lr')}: a positive finite rate")
    if not opt("wd") >= 0:
        raise SystemExit(f"--{key}-wd {opt('wd')}: weight decay must be >= 0")
    if opt("epochs") < 1:
        raise SystemExit(f"--{key}-epochs {opt('epochs')}: at least one pass over the bank's slides")
    if not 1 <= opt("batch") <= 64:
        raise SystemExit(f"--{key}-batch {opt('batch')}: 1 .. 64 slides per step ({entry})")
    from gipvit.archs import ARCHS, resolve_arch       # plain tables: nothing is loaded for them
    spec, layers = ARCHS[resolve_arch(args.model)], opt("layers")
    if not 1 <= layers <= spec["depth"]:
        raise SystemExit(f"--{key}-layers {layers}: the last 1 .. {spec['depth']} blocks of {args.model}")
    if layers * spec["embed_dim"] > 4096:
        raise SystemExit(f"--{key}-layers {layers}: {layers * spec['embed_dim']} features per tile at width {spec['embed_dim']}, "
                         f"{entry} stops at 4096")
    if opt("rate") < 0:
        raise SystemExit(f"--{key}-rate {opt('rate')}: 0 = after the last epoch only, N >= 1 = every N epochs and the last")
    if args.test_fold in (-1, "-1"):
        raise SystemExit(f"--test_fold -1 with {flag}: no evaluation fold is left to score the slides of")
    if args.tile_size < args.global_crop_size:
        raise SystemExit(f"{flag}: the teacher sees {args.global_crop_size}-px images, the centred window of a {args.tile_size}-px "
                         "tile (--tile-size) cannot be smaller than that")
    if args.num_tiles > 4096:
        raise SystemExit(f"--num_tiles {args.num_tiles} with {flag}: a slide's bag holds at most 4096 tiles ({entry})")
    if args.knn_bank_tiles is not None and args.knn_bank_tiles > 4096:
        raise SystemExit(f"--knn-bank-tiles {args.knn_bank_tiles} with {flag}: a slide's bag holds at most 4096 tiles ({entry})")
    names = monitor_metric_names(args)
    if resolve() not in names:
        raise SystemExit(f"--eval-metric {args.eval_metric}: the monitors of this run report {names} (a bare name is the k-NN monitor's when that "
                         f"is on, else the linear probe's, else the MIL probe's{metric_hint})")


def check_surv_probe(args):
    """--surv-probe's refusals, all before any GPU work (the MIL probe's, and a survival table to train on)."""
    check_bag_probe(args, "surv", "; the survival probe's are surv_cindex and surv_loss",
                    lambda: resolve_eval_metric(args.eval_metric, bool(args.knn_monitor), bool(args.linear_probe), bool(args.mil_probe), surv=True))
    if args.dataset not in ("", "synthetic") and (args.dataset.startswith("tiles:") or args.data_dir) and not args.extract_features:
        from gipvit import data as D                   # (numpy and torch only: no library is loaded)
        root = args.dataset[6:] if args.dataset.startswith("tiles:") else args.data_dir
        if not D.read_survival(root):
            raise SystemExit(f"--surv-probe: {os.path.join(root, 'labels.csv')} yields no survival table (a time | 'Time (months)' column, a "
                             "censored | Censored | event column, and at least one row with valid cells)")


def monitor_metric_names(args):
    """The metrics the monitors of a --dino run report, in the fixed order of their summary.csv columns: the k-NN monitor's, then
    the linear probe's, then the MIL probe's, then the survival probe's; the AUCs only with more than one class."""
    many = (args.num_classes or 2) > 1
    knn = (["knn_top1"] + (["knn_auc_per_patch", "knn_auc_per_slide"] if many else [])) if args.knn_monitor else []
    probe = (["linear_top1", "linear_loss"] + (["linear_auc_per_patch", "linear_auc_per_slide"] if many else [])) if args.linear_probe else []
    mil = (["mil_top1", "mil_loss"] + (["mil_auc_per_slide"] if many else [])) if getattr(args, "mil_probe", False) else []
    surv = ["surv_cindex", "surv_loss"] if getattr(args, "surv_probe", False) else []
    return knn + probe + mil + surv


def summary_row(epoch, train_metrics, eval_metrics, monitor_names, lr) -> "OrderedDict":
    """One row of summary.csv.  The header is written once, so every epoch's row has the same columns in the same order:
    validate()'s metrics as they come, then one column per name in ``monitor_names`` (the k-NN monitor's, then the probe's), in
    that order whichever of them ran this epoch -- empty where a monitor did not run (--knn-rate / --linprobe-rate)."""
    row = OrderedDict(epoch=epoch, **{"train_" + k: v for k, v in train_metrics.items()})
    row.update(("eval_" + k, v) for k, v in eval_metrics.items() if k not in monitor_names)
    row.update(("eval_" + k, eval_metrics.get(k, "")) for k in monitor_names)
    row["lr"] = lr
    return row


def resolve_eval_metric(name: str, knn: bool, probe: bool, mil: bool = False, *, surv: bool = False) -> str:
    """--eval-metric among the metrics of a --dino run's monitors: a name that already starts knn_ / linear_ / mil_ / surv_ is
    taken as given, a bare one is the k-NN monitor's when that is on ('top1' -> 'knn_top1'), else the linear probe's when that is
    on, else the MIL probe's, else the survival probe's when it is the only monitor."""
    if name.startswith("knn_") or name.startswith("linear_") or name.startswith("mil_") or name.startswith("surv_"):
        return name
    return ("knn_" + name) if knn else ("linear_" + name) if probe else ("mil_" + name) if mil else ("surv_" + name) if surv else name


def mix_active(args) -> bool:
    """train.py:755."""
    return args.mixup > 0 or args.cutmix > 0.0 or args.cutmix_minmax is not None


def loss_kind(args) -> str:
    """The training loss train.py:832-844 selects, as SupervisedEngine's ``loss``: mixing active -> BinaryCrossEntropy with --bce-loss,
    else SoftTargetCrossEntropy (smoothing goes into the target); not active -> BinaryCrossEntropy with --bce-loss and a non-zero
    --smoothing, else LabelSmoothingCrossEntropy (smoothing 0: cross-entropy)."""
    if mix_active(args):
        return "bce" if args.bce_loss else "soft_ce"
    return "bce" if (args.bce_loss and args.smoothing) else "lsce"


def build_mix_sampler(args, img_size: int, rank: int = 0):
    """timm Mixup's draws from the flags (train.py:755-771), or None when mixing is off.  Seeded per rank like the other host streams."""
    if not mix_active(args):
        return None
    from gipvit.mixup import MixSampler
    return MixSampler(mixup_alpha=args.mixup, cutmix_alpha=args.cutmix, cutmix_minmax=args.cutmix_minmax, prob=args.mixup_prob,
                      switch_prob=args.mixup_switch_prob, mode=args.mixup_mode, batch=args.batch_size, img_size=img_size,
                      seed=stream_seed("mix", args.seed, rank))


def build_erase_sampler(args, img_size: int, rank: int = 0):
    """timm RandomErasing's draws from --reprob / --remode / --recount, or None at --reprob 0.  Seeded per rank like the other host streams."""
    if not args.reprob > 0:
        return None
    from gipvit.erasing import EraseSampler
    return EraseSampler(prob=args.reprob, mode=args.remode, count=args.recount, batch=args.batch_size, img_size=img_size,
                        seed=stream_seed("erase", args.seed, rank))


def amp_is_f16(args) -> bool:
    """``--amp`` with the reference's default ``--amp-dtype float16`` (train.py:332, 452-465)."""
    return bool(args.amp) and args.amp_dtype.lower() in ("float16", "fp16")


class Meter:
    def __init__(self):
        self.val = self.sum = self.n = 0.0

    def update(self, v, k=1):
        self.val, self.sum, self.n = v, self.sum + v * k, self.n + k

    @property
    def avg(self):
        return self.sum / max(self.n, 1)


def teacher_temp_at(args, epoch: int) -> float:
    """DINO's teacher-temperature schedule: linear warm-up from --warmup-teacher-temp to --teacher-temp over the first
    --warmup-teacher-temp-epochs epochs (np.linspace over those epochs), --teacher-temp afterwards -- and from step 0
    when there is no warm-up."""
    n = args.warmup_teacher_temp_epochs
    if n <= 0 or epoch >= n:
        return args.teacher_temp
    if n == 1:
        return args.warmup_teacher_temp
    return args.warmup_teacher_temp + (args.teacher_temp - args.warmup_teacher_temp) * epoch / (n - 1)


def hook_batch_format(args, transform, argv=None) -> str:
    """Batch format a caller's transform hook (``main(transform=...)``) implies, found before any GPU work by calling it on
    the first tile of the dataset: "u8_nhwc" or "f32_nchw" (the reference's normalised FloatTensor[3, H, W],
    transformations.py:199-200).  Float batches skip the uint8 pipeline, so what only exists there is refused here."""
    from gipvit import data as D, transformations as T
    if args.dataset in ("", "synthetic") or not (args.dataset.startswith("tiles:") or args.data_dir):
        raise SystemExit("main(transform=...): the hook transforms tiles read from disk -- pass --dataset tiles:<dir> (or --data_dir)")
    if isinstance(transform, T.TileTransform):
        return "u8_nhwc"
    root = args.dataset[6:] if args.dataset.startswith("tiles:") else args.data_dir
    fmt = D.probe_hook_format(D.scan_slides(root, args.target), transform, args.tile_size)
    if fmt == "f32_nchw":
        why = "the transform hook returns float32 [3, H, W] images (already normalised)"
        if args.random_crops:
            raise SystemExit(f"--random-crops: {why}; random-resized crops are cut from uint8 tiles on the device -- "
                             "run the fixed crop windows (drop the flag) or return uint8 [H, W, 3] tiles from the hook")
        if args.view_augment:
            raise SystemExit(f"--view-augment: {why}; the per-crop view augmentation works on uint8 tiles on the device")
        given = sys.argv[1:] if argv is None else list(argv)
        if any(a == "--transform_type" or a.startswith("--transform_type=") for a in given) and args.transform_type in T.DEVICE_RECIPES:
            raise SystemExit(f"--transform_type {args.transform_type}: {why}; the named recipes augment uint8 tiles on the device "
                             "and the hook replaces them -- drop the flag")
    return fmt


def select_slides(args, slides, primary=True):
    """-> (training slides, evaluation slides, whether validate() has a fold to run on)."""
    from gipvit import data as D
    want_eval = not args.no_validate and (not args.dino or args.extract_features)
    train_slides = D.select_fold(slides, args.test_fold, True)
    if args.supervised or (monitor_metric_names(args) and not args.extract_features) or (want_eval and args.test_fold not in (-1, "-1")):
        eval_slides = D.select_fold(slides, args.test_fold, False)       # raises when evaluation was asked for and no slide is in the fold
    else:
        eval_slides = []        # the reference's "no validation" setting (train.py:367, datasets.py:284-287): every fold but 'test' / 'val' trains
        if want_eval and primary:
            _logger.info("--test_fold -1: no validation fold; validate() is skipped (reference train.py:367)")
        want_eval = False
    if args.supervised:     # train.py:715-717: --supervised re-splits the TEST-fold set 80 / 20 into train / eval
        perm = np.random.default_rng(args.seed).permutation(len(eval_slides))
        k = max(1, int(len(eval_slides) * 0.8))
        train_slides, eval_slides = [eval_slides[i] for i in perm[:k]], [eval_slides[i] for i in perm[k:]] or eval_slides
    return train_slides, eval_slides, want_eval


def build_loaders(args, run, transform, hook_format):
    """-> SimpleNamespace(source, augmenter: a named recipe's; inf: validate()'s loader; bank / query: the monitors', training / evaluation fold) or Nones."""
    from gipvit import data as D, transformations as T
    B, tile, rank = run.B, run.tile, run.rank
    synthetic = args.dataset in ("", "synthetic")
    transform = T.define_transformations(transform if transform is not None else args.transform_type if not synthetic else "none", True, tile, args.c_param, "Ron")
    augmenter = None
    if getattr(transform, "device_recipe", None):      # the named recipes run on the DEVICE once the tiles are in HBM (gv_augment); the readers deliver raw tiles
        from gipvit.augment import TileAugmenter
        augmenter = TileAugmenter(transform.device_recipe, tile, transform.color_param, run.mean, run.std, seed=args.seed + 31 * rank, device=run.dev)
        transform = None
    if hook_format == "f32_nchw" and run.primary:
        _logger.info("transform hook returns float32 [3, H, W]: batches are float32 NCHW, patchified without the fused normalise")
    inf = bank = query = surv_table = None
    bank_tiles, monitors_on = args.knn_bank_tiles or args.num_tiles, bool(monitor_metric_names(args)) and not args.extract_features
    if synthetic:
        source = D.SyntheticTiles(B, tile, args.batches_per_epoch, args.num_classes or 2, seed=args.seed + rank)
        if not args.no_validate and (not args.dino or args.extract_features):
            inf = D.SyntheticSlides(args.synthetic_slides, min(args.num_tiles, 2 * B), tile, args.tiles_per_iter, seed=args.seed + 99)
        if monitors_on:      # (--extract_features runs alone)
            bank = D.SyntheticSlides(args.synthetic_slides, min(bank_tiles, 2 * B), tile, args.tiles_per_iter, seed=args.seed + 77)
            query = D.SyntheticSlides(args.synthetic_slides, min(args.num_tiles, 2 * B), tile, args.tiles_per_iter, seed=args.seed + 99)
            if getattr(args, "surv_probe", False):
                surv_table = D.synthetic_survival(bank.image_file_names, args.seed)
    elif args.dataset.startswith("tiles:") or args.data_dir:
        root = args.dataset[6:] if args.dataset.startswith("tiles:") else args.data_dir
        train_slides, eval_slides, want_eval = select_slides(args, D.scan_slides(root, args.target), run.primary)
        infer = lambda n, seed, slides: D.InferTiles(root, tile, args.tiles_per_iter, n, seed=seed, dataset_name=args.dataset, workers=args.workers, slides=slides)
        source = D.TileFolder(root, B, transform, rank, run.world, args.seed, tile, n_tiles=args.n_patches_train, workers=args.workers, slides=train_slides)
        if want_eval:
            inf = infer(args.num_tiles, args.seed, eval_slides)
        if monitors_on:      # (--extract_features runs alone)
            bank, query = infer(bank_tiles, args.seed + 1, train_slides), infer(args.num_tiles, args.seed, eval_slides)
            if getattr(args, "surv_probe", False):
                surv_table = D.read_survival(root)
    else:
        raise SystemExit(f"--dataset {args.dataset}: whole-slide datasets need openslide and are outside this build "
                         "(SURVEY section 2 #15); use 'synthetic' or 'tiles:<dir>' with pre-extracted tile_<i>.data files")
    return SimpleNamespace(source=source, augmenter=augmenter, inf=inf, bank=bank, query=query, surv_table=surv_table)


def build_engine(args, run, img_from_input_size):
    """-> (engine with its initial, --initial-checkpoint or --resume state, image size, classes (0: --dino), --model-ema's decay or None, the --resume
    checkpoint or None, the epoch to start at)."""
    from gipvit import models as M
    from gipvit.engine import DinoEngine, SupervisedEngine
    arch, B, tile = run.arch, run.B, run.tile
    common = dict(arch=arch, batch=B, lr=run.lr, weight_decay=args.weight_decay, betas=run.betas, eps=run.eps, clip_grad=args.clip_grad or 0.0,
                  mean=run.mean, std=run.std, device=run.dev, reducer=run.reducer, precision=args.precision, clip_mode=args.clip_mode,
                  long_seq=getattr(args, "train_long_seq", False))
    if common["long_seq"] and run.primary:
        _logger.info("--train-long-seq: crops past %d tokens train with the streaming attention backward (gv_attention_bwd_stream, up to %d tokens)",
                     ATTN_TRAIN_MAX_TOKENS, ATTN_STREAM_MAX_TOKENS)
    ema_decay = args.model_ema_decay if args.model_ema else None                 # train.py:615-622
    if args.dino:
        if args.model_ema and run.primary:
            _logger.warning("--model-ema with --dino: the DINO teacher IS the EMA model (momentum schedule --momentum-teacher); flag has no further effect")
        img, nc = args.global_crop_size, 0
        eng = DinoEngine(img_size=img, out_dim=args.out_dim, tile=tile, n_local=args.local_crops_number, gsize=args.global_crop_size, lsize=args.local_crop_size,
                         momentum_teacher=args.momentum_teacher, teacher_temp=args.teacher_temp, **common, **dino_loss_options(args), **ibot_options(args))
        bb = (M.load_encoder_checkpoint(args.initial_checkpoint, arch, img, mask_token=args.ibot_weight > 0) if args.initial_checkpoint
              else M.init_vit_state(arch, img, 0, seed=args.seed))
        eng.load_state(bb, M.init_dino_head_state(eng.D, args.out_dim, seed=args.seed + 1))
    else:
        img, nc = args.img_size or img_from_input_size or tile, args.num_classes or 2   # the reference patches timm's default cfg to 256 (train_instruct.txt:9-13)
        eng = SupervisedEngine(img_size=img, num_classes=nc, smoothing=args.smoothing, opt=run.opt, momentum=args.momentum, train_backbone=not args.no_grad,
                               model_ema_decay=ema_decay, loss=loss_kind(args), bce_target_thresh=args.bce_target_thresh if loss_kind(args) == "bce" else None,
                               layer_decay=args.layer_decay, global_pool=args.gp, **common)
        st = (M.load_encoder_checkpoint(args.initial_checkpoint, arch, img, nc, eng.pool) if args.initial_checkpoint
              else M.init_vit_state(arch, img, nc, seed=args.seed, global_pool=eng.pool))
        eng.load_state(st)
    if not args.resume:
        return eng, img, nc, ema_decay, None, args.start_epoch or 0
    ck = load_checkpoint_file(args.resume)        # weights, teacher / EMA copy, optimizer moments and loss scaler into the engine
    strip = lambda d: {k[7:] if k.startswith("module.") else k: v for k, v in d.items()}
    sd = strip(ck["state_dict"])
    sub = lambda d, pre: {k[len(pre):]: v for k, v in d.items() if k.startswith(pre)}
    if args.dino:
        eng.load_state(sub(sd, "backbone."), sub(sd, "head."))
        if "state_dict_ema" in ck:        # the teacher + centre: without them the run would restart the EMA from the student
            te = strip(ck["state_dict_ema"])
            eng.load_teacher_state(sub(te, "backbone."), sub(te, "head."), ck.get("dino_center"))
            if args.ibot_weight > 0 and ck.get("ibot_center") is not None:
                eng.patch_center.copy_(ck["ibot_center"].to(run.dev, torch.float32).view(-1))
        elif run.primary:
            _logger.warning("--resume: %s holds no teacher ('state_dict_ema'); the teacher restarts as a copy of the student", args.resume)
    else:
        eng.load_state(sd, strip(ck["state_dict_ema"]) if (ema_decay is not None and "state_dict_ema" in ck) else None)
    if "optimizer" in ck and not args.no_resume_opt:
        eng.arena.m.copy_(ck["optimizer"]["exp_avg"]); eng.arena.v.copy_(ck["optimizer"]["exp_avg_sq"]); eng.t = int(ck["optimizer"]["step"])
    if eng.scaler is not None and isinstance(ck.get("amp_scaler"), dict):      # timm resume_checkpoint(..., loss_scaler=...); a GradScaler state
        # written by torch itself has no count of applied steps: the optimizer's step count stands in
        eng.scaler.load_state_dict(dict({"applied_steps": eng.t}, **ck["amp_scaler"]))
    return eng, img, nc, ema_decay, ck, args.start_epoch if args.start_epoch is not None else ck.get("epoch", -1) + 1


def build_evaluation(args, args_text, run):
    """What ends an epoch -> (runners over the engine's LIVE weights: SimpleNamespace(val, ema, mon: the monitors', norm: {name: its SlideNormaliser} or {}),
    the monitors, the resolved --eval-metric, the primary's saver and output dir (train.py:854-879))."""
    from gipvit.engine import FeatureExtractor, Weights
    arch, tile, mean, std, dev, eng, img, nc = run.arch, run.tile, run.mean, run.std, run.dev, run.eng, run.img, run.nc
    eval_B = min(256, max(run.B, 32))
    teacher = lambda: Weights(eng.arena, "backbone.", teacher=True, fp32=args.precision == "fp32")
    r = SimpleNamespace(val=None, ema=None, mon=None, norm={})
    long_maps = bool(getattr(args, "long_attention_maps", False))     # --long-attention-maps: the extractors' maps past GV_ATTN_MAX_N tokens
    if run.data.inf is not None:
        if args.dino:       # features come from the teacher backbone (the model DINO users evaluate)
            r.val = FeatureExtractor(arch, tile, eval_B, 0, mean, std, dev, weights=teacher(), long_maps=long_maps)
            if tile != img:
                raise SystemExit(f"--extract_features with --dino: tile size {tile} must equal the teacher's image size {img}")
        else:
            r.val = FeatureExtractor(arch, img, eval_B, nc, mean, std, dev, weights=eng.W, global_pool=eng.pool, long_maps=long_maps)
            if run.ema_decay is not None:
                r.ema = FeatureExtractor(arch, img, eval_B, nc, mean, std, dev, weights=eng.Wema, global_pool=eng.pool, long_maps=long_maps)
    if run.data.bank is not None:   # the teacher backbone at its own image size; larger tiles contribute their centred window (gipvit/knn.py)
        r.mon = FeatureExtractor(arch, img, eval_B, 0, mean, std, dev, weights=teacher())
    if args.stain_normalize == "macenko":
        from gipvit.stainnorm import MacenkoEstimator, SlideNormaliser
        estimator = MacenkoEstimator(dev, beta=args.stain_norm_beta, alpha=args.stain_norm_alpha, max_tiles=args.stain_norm_tiles)
        r.norm = {key: SlideNormaliser(getattr(r, key), estimator, primary=run.primary) for key in ("val", "ema", "mon") if getattr(r, key) is not None}
        if run.primary:
            _logger.info("stain normalisation: macenko (beta %.3g alpha %.3g, %s of a slide's first chunk) on every inference pass%s; "
                         "training batches are not normalised", args.stain_norm_beta, args.stain_norm_alpha,
                         f"the first {args.stain_norm_tiles} tiles" if args.stain_norm_tiles else "every tile", "" if r.norm else " (this run has none)")
    monitors = build_monitors(args, r.mon, run.primary, r.norm.get("mon"), **({"surv_table": run.data.surv_table} if getattr(args, "surv_probe", False) else {}))
    eval_metric = resolve_eval_metric(args.eval_metric, *(any(m.prefix == p for m in monitors) for p in ("knn_", "linear_", "mil_")),
                                      surv=any(m.prefix == "surv_" for m in monitors))   # 'top1' -> knn_top1
    saver = output_dir = None
    if run.primary:
        exp = args.experiment or "-".join([time.strftime("%Y%m%d-%H%M%S"), args.model.replace("/", "_"), str(img)])
        output_dir = os.path.join(args.output or "./output/train", exp, args.subexperiment or "")
        decreasing = eval_metric in LOWER_IS_BETTER or eval_metric in SURV_LOWER_IS_BETTER or not (monitors or (run.data.inf is not None and not args.dino))       # train.py:866
        saver = CheckpointSaver(output_dir, args.model, vars(args), decreasing=decreasing, max_history=args.checkpoint_hist)
        with open(os.path.join(output_dir, "args.yaml"), "w") as f:
            f.write(args_text)
    return r, monitors, eval_metric, saver, output_dir


def build_monitors(args, runner, primary=True, normaliser=None, surv_table=None):
    """The run's monitors on ``runner``, in the fixed order k-NN, linear probe, MIL probe, survival probe.  ``normaliser``: the keyword exists with
    --stain-normalize only; ``surv_table``: slide name -> (time, event), with --surv-probe only."""
    if runner is None:
        return []
    from gipvit.knn import KnnMonitor as Knn            # (imported late: they load the library)
    from gipvit.linprobe import LinearProbe as Linear
    from gipvit.mil import MilProbe as Mil
    kw = dict(num_classes=args.num_classes or 2, primary=primary, **({"normaliser": normaliser} if normaliser is not None else {}))
    monitors = []
    if args.knn_monitor:
        monitors.append(Knn(runner, k=args.knn_k, temp=args.knn_temp, **kw))
    if args.linear_probe:       # heads on the same runner's last-layer CLS tokens (gipvit/linprobe.py)
        monitors.append(Linear(runner, lrs=args.linprobe_lrs, weight_decay=args.linprobe_wd, epochs=args.linprobe_epochs, batch=args.linprobe_batch,
                               n_last=args.linprobe_layers, avgpool=args.linprobe_avgpool, holdout=args.linprobe_holdout, seed=args.seed, **kw))
    if args.mil_probe:          # slide-level ABMIL on the same runner's CLS tokens, one bag per slide (gipvit/mil.py)
        monitors.append(Mil(runner, hidden=args.mil_hidden, lr=args.mil_lr, weight_decay=args.mil_wd, epochs=args.mil_epochs, batch=args.mil_batch,
                            n_last=args.mil_layers, seed=args.seed, **kw))
    if getattr(args, "surv_probe", False):      # the same body with one risk output under Cox's partial likelihood (gipvit/survival.py)
        from gipvit.survival import SurvivalProbe as Surv
        monitors.append(Surv(runner, surv_table, hidden=args.surv_hidden, lr=args.surv_lr, weight_decay=args.surv_wd, epochs=args.surv_epochs,
                             batch=args.surv_batch, n_last=args.surv_layers, seed=args.seed, **kw))
    assert [n for m in monitors for n in m.metric_names()] == monitor_metric_names(args)        # the flag-level statements the refusals and the saver use
    assert [m.prefix + x for m in monitors for x in m.lower_is_better] == [n for n in monitor_metric_names(args) if n in LOWER_IS_BETTER or n in SURV_LOWER_IS_BETTER]
    return monitors


def monitor_due(args, prefix: str, epoch: int) -> bool:
    """The monitor with this metric prefix runs after ``epoch``: k-NN every --knn-rate epochs; a probe after the last and, at a rate >= 1, every rate epochs."""
    if prefix == "knn_":
        return (epoch + 1) % args.knn_rate == 0
    rate = args.linprobe_rate if prefix == "linear_" else args.surv_rate if prefix == "surv_" else args.mil_rate
    return epoch == args.epochs - 1 or (rate >= 1 and (epoch + 1) % rate == 0)


def build_samplers(args, rank, primary, dev, img, depth, drop_rows):
    """The run's host draw streams, seeded per rank from checkpoint.HOST_STREAMS -> SimpleNamespace(samplers or None, streams: {name: Generator}, seeds)."""
    B, seed = args.batch_size, (lambda name: stream_seed(name, args.seed, rank))
    s = SimpleNamespace(crops=None, ibot=None, views=None, stain=None, drop_path=None, drop=None)
    if args.dino and args.random_crops:       # DINO recipe: random-resized crops + flips, cut on the device
        from gipvit.multicrop import MultiCropSampler
        s.crops = MultiCropSampler(B, args.tile_size, 2, args.local_crops_number, tuple(args.global_crops_scale), tuple(args.local_crops_scale), seed=seed("crops"))
    # mixup / cutmix (train.py:752-771, 1037-1040): the draws are the host's, the mixed batch is made inside the patchify pass
    s.mix = None if args.dino else build_mix_sampler(args, img, rank)
    if s.mix is not None and primary:
        _logger.info("mixup / cutmix on the device: mixup %.3g cutmix %.3g minmax %s prob %.3g switch %.3g mode %s, loss %s", args.mixup, args.cutmix,
                     args.cutmix_minmax, args.mixup_prob, args.mixup_switch_prob, args.mixup_mode, loss_kind(args))
    # random erasing (--reprob / --remode / --recount): boxes drawn on the host, erased inside the same patchify pass, after the mixing
    s.erase = None if args.dino else build_erase_sampler(args, img, rank)
    if s.erase is not None and primary:
        _logger.info("random erasing on the device: reprob %.3g remode %s recount %d (training steps only, after mixup / cutmix)", args.reprob, args.remode, args.recount)
    if args.dino and args.ibot_weight > 0:      # iBOT: which patches of which global crop the student does not see, drawn per rank
        from gipvit.masking import MaskSampler
        s.ibot = MaskSampler(args.global_crop_size // 16, 2 * B, tuple(args.ibot_mask_ratio), args.ibot_mask_prob, seed=seed("ibot"))
    if args.view_augment:
        from gipvit.multicrop import ViewAugmentSampler
        s.views = ViewAugmentSampler(B, 2, args.local_crops_number, jitter_p=args.color_jitter_p, gray_p=args.gray_p, blur_p=tuple(args.blur_p),
                                     solar_p=(0.0, args.solarize_p, 0.0), seed=seed("views"))
    if args.stain_jitter > 0:       # H&E stain jitter: folded per-crop records drawn per rank, applied in the view-augmentation pass
        from gipvit.stain import StainJitterSampler
        s.stain = StainJitterSampler(B, 2, args.local_crops_number, args.stain_jitter, prob=args.stain_prob, seed=seed("stain"))
        if primary:
            _logger.info("H&E stain jitter on the device: sigma %.3g prob %.3g (every crop, ahead of the view augmentation)", args.stain_jitter, args.stain_prob)
    if args.drop_path:      # train.py:287-288: stochastic depth on the training passes (DINO: the student's, every crop of every tile its own sample)
        from gipvit.droppath import DropPathSampler
        s.drop_path = DropPathSampler(depth, drop_rows, args.drop_path, seed("drop_path"), dev)
    if args.drop:           # train.py:283-284: nn.Dropout at the four sites of the encoder, a fresh 32-bit seed per step (counter-based masks)
        s.drop = np.random.default_rng(seed("drop"))
    s.streams = {"drop": s.drop, **{k: getattr(getattr(s, k), "rng", None) for k in ("crops", "views", "stain", "mix", "erase", "ibot")}}
    s.seeds = {k: seed(k) for k in HOST_STREAMS}
    return s


def extra_state(args, eng, ema_decay, rng_state):
    """A checkpoint's entries beside weights and optimizer; ``rng_state``: pack_host_rng's, gathered by ALL ranks at the save point."""
    ex = dict(rng_state)
    if args.dino:       # teacher (the EMA model) + centre: a DINO run cannot be resumed (or evaluated) without them
        ex.update(state_dict_ema=eng.arena.state_dict(eng.arena.t), dino_center=eng.center.detach().cpu())
        if eng.ibot_weight > 0:
            ex["ibot_center"] = eng.patch_center.detach().cpu()
    elif ema_decay is not None:
        ex["state_dict_ema"] = eng.state_dict(ema=True)     # timm CheckpointSaver key
    if eng.scaler is not None:
        ex["amp_scaler"] = eng.scaler.state_dict()          # timm CheckpointSaver(amp_scaler=loss_scaler) key, train.py:585-602
    return ex


def train_epoch(args, run, epoch):
    """The step loop (train.py:988-1143) -> the epoch's train metrics; leaves the last step's rate in ``run.cur_lr``."""
    from gipvit import sched as S
    eng, smp, dev, B, world = run.eng, run.smp, run.dev, run.B, run.world
    batch_time, data_time, losses, probs, targets = Meter(), Meter(), Meter(), [], []
    end, last_idx, total_updates = time.time(), run.updates_per_epoch - 1, args.epochs * run.updates_per_epoch
    if args.dino:
        eng.train_last_layer = epoch >= args.freeze_last_layer
    if smp.mix is not None and args.mixup_off_epoch and epoch >= args.mixup_off_epoch:
        smp.mix.enabled = False                # train.py:1005-1009: no mixing from this epoch on; the loss stays the soft-target one
    for batch_idx, mb in (enumerate(run.loader) if not args.extract_features else ()):      # train.py:906
        data, target, fill = mb["Data"], mb["Target"], None
        if run.data.augmenter is not None:      # the draws came with the batch (pinned staging); the pixel work is one launch here
            data, fill = run.data.augmenter.run(data, mb["AugParams"]), mb["Fill"]
        data_time.update(time.time() - end)
        run.cur_lr = cur_lr = run.schedule.at(epoch, batch_idx)
        if smp.drop_path is not None:
            eng.set_drop_path(smp.drop_path.sample())
        if smp.drop is not None:
            eng.set_dropout(args.drop, int(smp.drop.integers(0, 1 << 32)))
        if args.dino:
            it = epoch * run.updates_per_epoch + batch_idx
            sch = dict(lr=cur_lr, wd=S.cosine_between(args.weight_decay, args.weight_decay_end, it, total_updates),
                       momentum_teacher=S.cosine_between(args.momentum_teacher, 1.0, it, total_updates),
                       teacher_temp=teacher_temp_at(args, epoch))
            loss_t = eng.step(data, boxes=smp.crops.sample(dev) if smp.crops is not None else None, fill=fill if smp.crops is None else None,
                              views=smp.views.sample(dev) if smp.views is not None else None,
                              **({"masks": smp.ibot.sample(dev)} if smp.ibot is not None else {}),
                              **({"stains": smp.stain.sample(dev)} if smp.stain is not None else {}), **sch)
        else:
            ekw = {"erase": smp.erase.sample(dev)} if smp.erase is not None else {}
            loss_t = eng.step(data, target, lr=cur_lr, fill=fill, mix=smp.mix.sample(dev) if smp.mix is not None else None, **ekw)
            probs.append(eng.prob[:, 1].clone() if eng.C > 1 else eng.prob[:, 0].clone()); targets.append(target.view(-1).clone())
        torch.cuda.synchronize()                  # train.py:1083
        batch_time.update(time.time() - end)
        if batch_idx == last_idx or batch_idx % args.log_interval == 0:
            lv = float(loss_t)
            if world > 1:
                t = torch.tensor([lv], device=dev)
                torch.distributed.all_reduce(t)   # utils.reduce_tensor, train.py:1091-1093
                lv = float(t) / world
            losses.update(lv, B)
            if run.primary:
                _logger.info("Train: {} [{:>4d}/{} ({:>3.0f}%)]  Loss: {:#.4g} ({:#.3g})  Time: {:.3f}s, {:>7.2f}/s  ({:.3f}s, {:>7.2f}/s)  "
                             "LR: {:.3e}  Data: {:.3f} ({:.3f})".format(
                                 epoch, batch_idx, run.updates_per_epoch, 100.0 * batch_idx / max(last_idx, 1), losses.val, losses.avg,
                                 batch_time.val, B * world / batch_time.val, batch_time.avg, B * world / batch_time.avg, run.logged_lr(cur_lr),
                                 data_time.val, data_time.avg)
                             + ("  KoLeo: {:#.4g}".format(float(eng.koleo)) if args.dino and args.koleo_weight > 0 else "")
                             + ("  iBOT: {:#.4g}".format(float(eng.ibot)) if args.dino and args.ibot_weight > 0 else ""))
            if args.recovery_interval and (batch_idx + 1) % args.recovery_interval == 0:
                rng_state = pack_host_rng(smp.streams, smp.drop_path, run.gather)       # a collective: every rank, only the write is the primary's
                if run.saver is not None:
                    run.saver.save_recovery(epoch, batch_idx, eng.arena.state_dict(), extra=extra_state(args, eng, run.ema_decay, rng_state))
        end = time.time()
    train_metrics = OrderedDict(loss=losses.avg)
    if probs:
        try:
            from sklearn.metrics import roc_auc_score
            train_metrics["auc"] = float(roc_auc_score(torch.cat(targets).cpu().numpy(), torch.cat(probs).float().cpu().numpy()))
        except Exception:                       # single-class epoch etc. (the reference would raise, train.py:1054)
            train_metrics["auc"] = float("nan")
    return train_metrics


def end_of_epoch(args, run, epoch, train_metrics):
    """Slide-level validation (train.py:932-955), the monitors that are due, summary.csv, checkpoint on --eval-metric (958-973)."""
    from gipvit.validate import validate
    eng, runners, primary = run.eng, run.runners, run.primary
    norm = lambda key: {"normaliser": runners.norm[key]} if key in runners.norm else {}
    eval_metrics = OrderedDict()
    if runners.val is not None:
        eval_metrics = validate(runners.val, run.data.inf, extract_features=bool(args.extract_features), extract_attention=bool(args.extract_attention),
                                smoothing=args.smoothing, log_interval=args.log_interval, out_dir=args.features_dir, primary=primary, **norm("val"))
        if runners.ema is not None and not args.extract_features:       # train.py:943-955: the EMA model's metrics win
            eval_metrics = validate(runners.ema, run.data.inf, smoothing=args.smoothing, log_interval=args.log_interval, primary=primary,
                                    log_suffix=" (EMA)", **norm("ema"))
    for m in run.monitors:
        if monitor_due(args, m.prefix, epoch):      # the teacher moved: a fresh bank / fresh heads / a fresh model on it as it stands
            m.fit(run.data.bank)
            eval_metrics.update(m.evaluate(run.data.query))
    if args.extract_features:
        if primary:
            _logger.info(f"*** features of {int(eval_metrics.get('slides', 0))} slides written to {args.features_dir}")
        return
    rng_state = pack_host_rng(run.smp.streams, run.smp.drop_path, run.gather)       # every rank: the checkpoint holds each rank's streams
    if not primary:
        return
    # the monitors' columns stay in one order, empty for a monitor that did not run this epoch
    monitor_names = [n for m in run.monitors for n in m.metric_names()]
    row = summary_row(epoch, train_metrics, eval_metrics, monitor_names, run.logged_lr(run.cur_lr))
    fn = os.path.join(run.output_dir, "summary.csv")
    new = not os.path.exists(fn)
    with open(fn, "a") as f:
        w = csv.DictWriter(f, fieldnames=row.keys())
        if new:
            w.writeheader()
        w.writerow(row)
    if run.wandb is not None:
        run.wandb.log({k: v for k, v in row.items() if v != ""})
    optim, eval_metric = {"exp_avg": eng.arena.m, "exp_avg_sq": eng.arena.v, "step": eng.t}, run.eval_metric
    if eval_metric in eval_metrics:
        save_metric, name = eval_metrics[eval_metric], "eval " + eval_metric          # train.py:970-973
    elif eval_metric in monitor_names or (not eval_metrics and run.monitors):
        save_metric, name = None, "eval " + eval_metric                               # not evaluated this epoch (--knn-rate / --linprobe-rate / --mil-rate / --surv-rate)
    elif eval_metrics:
        who = ("validate() reports" if not run.monitors else "the k-NN monitor reports" if [m.prefix for m in run.monitors] == ["knn_"]
               else "the monitors of this run report")
        raise SystemExit(f"--eval-metric {eval_metric}: {who} {list(eval_metrics)}")
    else:
        save_metric, name = train_metrics["loss"], "train loss"
    best, best_ep = run.saver.save_checkpoint(epoch, eng.arena.state_dict(), optim, metric=save_metric, extra=extra_state(args, eng, run.ema_decay, rng_state))
    _logger.info(f"*** epoch {epoch}: " + "  ".join(f"{k} {v:.4f}" for k, v in list(train_metrics.items()) + [("eval_" + k, v) for k, v in eval_metrics.items()])
                 + (f"  (best {name} {best:.4f} @ {best_ep})" if best is not None else f"  (no {name} yet)"))


def main(argv=None, transform=None):
    """``transform``: a custom augmentation hook in place of ``--transform_type`` (the reference's "any callable is the
    transform", transformations.py:199-200), applied by the tile reader threads.  It maps a uint8 [H, W, 3] tile to a uint8
    tile of the same form, or to a float [3, H, W] image already normalised -- then the batches are float32 NCHW, no
    device augmentation runs, and --random-crops / --view-augment / a named --transform_type are refused."""
    args, args_text = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    check_token_limits(args)
    check_stain_normalize(args)
    hook_format = hook_batch_format(args, transform, argv) if transform is not None else None
    if args.stain_normalize != "none" and hook_format == "f32_nchw":
        raise SystemExit("--stain-normalize: the transform hook returns float32 [3, H, W] images (already normalised); the stain estimate "
                         "and the map work on uint8 tiles -- return uint8 [H, W, 3] tiles from the hook or drop the flag")
    if not torch.cuda.is_available() or not str(args.device).startswith("cuda"):
        raise SystemExit("train.py: an MI355X is required (device=%s, cuda available=%s); the HIP hot path has no CPU fallback"
                         % (args.device, torch.cuda.is_available()))
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", args.local_rank))
    primary = rank == 0
    img_from_input_size = check_supported(args, _logger.warning if primary else (lambda m: None))
    if amp_is_f16(args):
        # one process computes in one 16-bit format: pick the float16 build of the library before it is first loaded
        assert "gipvit._lib" not in sys.modules, "the library was loaded before the --amp-dtype was known"
        os.environ["GIPVIT_ACT_FORMAT"] = "f16"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    reducer, gather = None, (lambda obj: [obj])            # gather: pack_host_rng's collective, [rank 0's obj, rank 1's, ...]
    if world > 1:
        import torch.distributed as dist
        from gipvit.dist import RcclReducer, comm_setup
        comm = comm_setup(world)                               # CUs left to RCCL's channels; the library sizes its launches for the rest
        dist.init_process_group("nccl", device_id=dev)         # RCCL
        reducer = RcclReducer()

        def gather(obj):
            out = [None] * world
            dist.all_gather_object(out, obj)
            return out
        if primary:
            _logger.info("data parallel over %d ranks (RCCL): launches sized for %d CUs (GIPVIT_COMM_CUS=%d)", world, comm["cu_budget"], comm["comm_cus"])
    torch.manual_seed(args.seed + rank)                        # utils.random_seed(seed, rank), train.py:467
    ignored = [e["flags"][-1] for e in REFERENCE_FLAGS if not e["used"] and e["flags"][-1].startswith("-")
               and getattr(args, flag_dest(e), None) not in (e.get("default"), None, False)]
    if ignored and primary:
        _logger.warning("flags accepted for CLI compatibility but outside this build's hot path: %s", " ".join(ignored))
    wandb_run = None
    if args.log_wandb and primary:                             # train.py:447-450 (optional here; credentials from the environment only)
        try:
            import wandb
            wandb_run = wandb.init(project=args.experiment or "gipvit", group=args.group or None, config=vars(args))
        except Exception as ex:                                # not installed / offline
            _logger.warning("--log-wandb: wandb unavailable (%s); metrics go to the log and summary.csv only", ex)

    from gipvit import models as M, sched as S, data as D, transformations as T
    from gipvit.engine import ARCHS
    opt = args.opt.lower()
    run = SimpleNamespace(rank=rank, world=world, primary=primary, dev=dev, reducer=reducer, gather=gather, wandb=wandb_run, arch=M.resolve_arch(args.model),
                          B=args.batch_size, tile=args.tile_size, mean=tuple(args.mean) if args.mean else T.MEAN["Ron"],
                          std=tuple(args.std) if args.std else T.STD["Ron"], opt=opt, betas=tuple(args.opt_betas) if args.opt_betas else (0.9, 0.999),
                          lr=S.scaled_lr(args.lr, args.lr_base, args.batch_size, world, args.lr_base_size, args.lr_base_scale, opt),
                          eps=args.opt_eps if args.opt_eps is not None else (1e-6 if opt == "lamb" else 1e-8))     # timm defaults: Lamb 1e-6, Adam(W) 1e-8
    if primary:
        _logger.info(f"Learning rate ({run.lr}) calculated from base learning rate ({args.lr_base}) and global batch size ({run.B * world})")
    run.data = build_loaders(args, run, transform, hook_format)
    run.eng, run.img, run.nc, run.ema_decay, ck, start_epoch = build_engine(args, run, img_from_input_size)
    if hasattr(run.data.source, "epoch"):
        run.data.source.epoch = start_epoch        # the synthetic source seeds every epoch: a resumed run sees epoch k's tiles
    if primary:
        n_params = sum(int(torch.tensor(s).prod()) for s in run.eng.arena.specs.values())
        _logger.info(f"Model {args.model} ({run.arch}) created, param count:{n_params}" + ("" if args.dino else f", global pool: {run.eng.pool}"))
    run.runners, run.monitors, run.eval_metric, run.saver, run.output_dir = build_evaluation(args, args_text, run)
    run.updates_per_epoch = len(run.data.source)
    run.schedule = S.LrSchedule(run.lr, args.sched, args.epochs, args.warmup_epochs, args.warmup_lr, args.min_lr, run.updates_per_epoch, args.decay_epochs,
                                args.decay_rate, on_updates=args.sched_on_updates or args.dino)
    # the step's critical path runs on a high-priority stream; the engine's side stream (teacher forward,
    # weight-gradient GEMMs) fills the CU slots it leaves
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.Stream(dev, priority=-1))
    # tiles reach HBM one batch ahead of the step: pinned staging + a copy stream (replaces pin_memory workers, train.py:732)
    run.loader = D.DevicePrefetcher(run.data.source, dev, (run.B, run.tile, run.tile, 3), run.data.augmenter)
    run.smp = smp = build_samplers(args, rank, primary, dev, run.img, ARCHS[run.arch]["depth"], (run.eng.V * run.B) if args.dino else run.B)
    if args.resume:     # continue every rank's draw streams where the saved run left them (or, across a change of world size, restart them apart)
        restore_host_rng(ck, smp.streams, smp.drop_path, rank, world, start_epoch, warn=_logger.warning, seeds=smp.seeds)
    # the reference logs the MEAN rate over the parameter groups (train.py:1088-1089, 959-965): with --layer-decay cur_lr x the mean scale
    run.cur_lr, run.logged_lr = run.lr, run.eng.mean_lr if hasattr(run.eng, "mean_lr") else (lambda v: v)
    for epoch in range(start_epoch, args.epochs):      # train.py:905-977
        end_of_epoch(args, run, epoch, train_epoch(args, run, epoch))
        if args.extract_features:
            break
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
