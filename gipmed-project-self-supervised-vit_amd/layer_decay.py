"""``--layer-decay`` on the host: the layer map, the per-layer rate scales and the range table of gv_adamw_ema_ranges.

The reference hands the flag to timm (train.py:175, ``optimizer_kwargs(cfg=args)`` -> ``create_optimizer_v2`` at train.py:583).
timm is not importable here and is unpinned in the reference, so the two timm behaviours below are RESTATED from its published
source -- parity is unpinned beyond this restatement:

* ``VisionTransformer.group_matcher(coarse=False)`` = ``GROUP_MATCHER``.  ``group_parameters`` sorts the match keys -- stem
  ``(0,)``, ``blocks.i`` ``(1, i)``, ``norm`` ``(1, 99999)``, unmatched names (the classifier) last -- and numbers them, so for
  depth L: ``cls_token``, ``pos_embed``, ``patch_embed.*`` -> 0, ``blocks.i.*`` -> i + 1, ``norm.*`` -> L + 1, ``head.*`` -> L + 2.
  ``fc_norm.*`` of a ``--gp avg`` model matches none of the patterns (``^norm`` does not match it): it falls into the unmatched
  group with ``head.*``, id L + 2, scale 1.  Such a model has no ``norm.*``, so id L + 1 holds no parameter and ``mean_lr``
  averages one group fewer.
* ``param_groups_layer_decay``: ``num_layers = L + 3``, ``scale(id) = decay ** (num_layers - 1 - id)``; one parameter group per
  (layer, decay | no-decay) that holds a trainable parameter, ``lr_scale`` = the layer's scale; timm's schedulers set every
  group's rate to ``scheduled_lr * lr_scale`` at every update, warm-up included.  The decay / no-decay split inside a layer is
  ``engine.no_weight_decay``'s.
"""
from __future__ import annotations

import re
from collections import OrderedDict
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

GROUP_MATCHER = dict(stem=r"^cls_token|pos_embed|patch_embed", blocks=[(r"^blocks\.(\d+)", None), (r"^norm", (99999,))])
_STEM, _BLOCK, _NORM = (re.compile(GROUP_MATCHER["stem"]), re.compile(GROUP_MATCHER["blocks"][0][0]), re.compile(GROUP_MATCHER["blocks"][1][0]))


def group_matcher(coarse: bool = False) -> dict:
    """timm ``VisionTransformer.group_matcher`` (restated, see the module docstring); ``coarse`` groups are not built."""
    if coarse:
        raise ValueError("group_matcher(coarse=True) is not built: --layer-decay takes the per-block groups (timm's default)")
    return dict(stem=GROUP_MATCHER["stem"], blocks=list(GROUP_MATCHER["blocks"]))


def num_layers(depth: int) -> int:
    return depth + 3


def layer_id(name: str, depth: int) -> int:
    """Layer id of a parameter name of a depth-``depth`` ViT under GROUP_MATCHER (patterns are tried in timm's order)."""
    if _STEM.match(name):
        return 0
    m = _BLOCK.match(name)
    if m:
        i = int(m.group(1))
        if not 0 <= i < depth:
            raise ValueError(f"{name}: block index outside a depth-{depth} model")
        return i + 1
    if _NORM.match(name):
        return depth + 1
    return depth + 2                 # no pattern matches: the last group (the classifier)


def layer_scale(layer: int, depth: int, decay: float) -> float:
    return float(decay) ** (num_layers(depth) - 1 - layer)


class Range(NamedTuple):
    lo: int
    hi: int
    layer: int
    decayed: bool
    names: Tuple[str, ...]


def range_table(arena, depth: int, names: Optional[Sequence[str]] = None) -> List[Range]:
    """Maximal contiguous ranges [lo, hi) of the arena in which layer id and decay flag are constant, over ``names`` (default:
    every parameter, in arena order; padding belongs to the parameter in front of it).  The arena's layout makes them few:
    2 * depth + 5 for a ViT with a classifier."""
    from .engine import no_weight_decay
    picked = list(arena.order) if names is None else sorted(names, key=lambda n: arena.off[n])
    out: List[Range] = []
    for n in picked:
        lo, hi = arena.span(n)
        lay, dec = layer_id(n, depth), not no_weight_decay(n, arena.specs[n])
        if out and out[-1].hi == lo and out[-1].layer == lay and out[-1].decayed == dec:
            out[-1] = out[-1]._replace(hi=hi, names=out[-1].names + (n,))
        else:
            out.append(Range(lo, hi, lay, dec, (n,)))
    for r in out:
        assert r.lo % 4 == 0 and r.hi % 4 == 0 and r.hi > r.lo
    return out


class LayerDecayPlan:
    """Everything ``--layer-decay`` needs for one set of trainable parameters: ``ranges`` (range_table), ``scales`` (name -> rate
    scale), ``mean_scale`` (mean of the scale over the (layer, decay) groups that hold a parameter: what the reference's log
    line averages, train.py:1088-1089) and the two tables of gv_adamw_ema_ranges."""

    def __init__(self, arena, depth: int, decay: float, names: Optional[Sequence[str]] = None):
        if not decay > 0:
            raise ValueError(f"layer_decay {decay}: must be > 0")
        self.depth, self.decay = depth, float(decay)
        self.ranges = range_table(arena, depth, names)
        self.scales: "OrderedDict[str, float]" = OrderedDict(
            (n, layer_scale(r.layer, depth, decay)) for r in self.ranges for n in r.names)
        groups = sorted({(r.layer, r.decayed) for r in self.ranges})
        self.group_scales = [layer_scale(lay, depth, decay) for lay, _ in groups]
        self.mean_scale = sum(self.group_scales) / len(self.group_scales)

    def mean_lr(self, lr: float) -> float:
        return lr * self.mean_scale

    def range_rows(self) -> torch.Tensor:
        """f32 [n_ranges, 2] = (lr_scale, wd_multiplier)."""
        return torch.tensor([(layer_scale(r.layer, self.depth, self.decay), 1.0 if r.decayed else 0.0) for r in self.ranges], dtype=torch.float32)

    def block_table(self, chunk: int = 1 << 12) -> torch.Tensor:
        from . import ops
        return ops.range_block_table([(r.lo, r.hi) for r in self.ranges], chunk)
