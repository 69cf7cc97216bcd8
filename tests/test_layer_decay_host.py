"""CPU: --layer-decay on the host -- timm's layer map and scales (restated: timm is not importable here), the range table of
gv_adamw_ema_ranges over the arena, the driver's flag checks, the mean group rate the log line prints, and the new entry
point's argument checks (which answer before any launch)."""
import ctypes
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 12


def _arena(num_classes=2, arch="vit_tiny", img=64):
    from gipvit.engine import Arena, vit_param_specs
    return Arena(vit_param_specs(arch, img, num_classes), "cpu", teacher=False)


def test_layer_ids_and_scales_follow_timm():
    """vit_tiny, num_classes=2, decay 0.75: ids 0 (stem), i + 1 (blocks.i), L + 1 (norm), L + 2 (head); scale = 0.75 ** (14 - id)."""
    from gipvit import layer_decay as LD
    from gipvit.models import VitModel
    ids = {"cls_token": 0, "pos_embed": 0, "patch_embed.proj.weight": 0, "patch_embed.proj.bias": 0,
           "blocks.0.norm1.weight": 1, "blocks.0.attn.qkv.bias": 1, "blocks.0.mlp.fc2.weight": 1,
           "blocks.11.attn.proj.weight": 12, "blocks.11.norm2.bias": 12,
           "norm.weight": 13, "norm.bias": 13, "head.weight": 14, "head.bias": 14}
    for name, want in ids.items():
        assert LD.layer_id(name, DEPTH) == want, name
    assert LD.num_layers(DEPTH) == 15
    scales = {"head.weight": 1.0, "norm.weight": 0.75, "blocks.11.mlp.fc1.weight": 0.5625,
              "blocks.0.attn.qkv.weight": 0.023757264018058777, "pos_embed": 0.017817948013544083}      # 0.75 ** 13, 0.75 ** 14
    arena = _arena()
    plan = LD.LayerDecayPlan(arena, DEPTH, 0.75)
    assert set(plan.scales) == set(arena.specs)
    for name, want in scales.items():
        assert plan.scales[name] == pytest.approx(want, rel=1e-12), name
    for name in arena.specs:                     # every parameter: the closed form
        assert plan.scales[name] == pytest.approx(0.75 ** (14 - LD.layer_id(name, DEPTH)), rel=1e-12), name
    with pytest.raises(ValueError):
        LD.layer_id("blocks.12.norm1.weight", DEPTH)
    with pytest.raises(ValueError):
        LD.LayerDecayPlan(arena, DEPTH, 0.0)
    model = VitModel(types.SimpleNamespace(C=2, D=192, arena=arena), "vit_tiny")
    assert model.group_matcher() == model.group_matcher(coarse=False) == dict(
        stem=r"^cls_token|pos_embed|patch_embed", blocks=[(r"^blocks\.(\d+)", None), (r"^norm", (99999,))])


def test_range_table_tiles_the_arena():
    from gipvit import layer_decay as LD
    from gipvit.engine import no_weight_decay
    arena = _arena()
    plan = LD.LayerDecayPlan(arena, DEPTH, 0.75)
    R = plan.ranges
    assert len(R) == 2 * DEPTH + 5 == 29
    assert R[0].lo == 0 and R[-1].hi == arena.n and all(a.hi == b.lo for a, b in zip(R, R[1:]))         # no gap, no overlap
    assert all(r.lo % 4 == 0 and r.hi % 4 == 0 and r.hi > r.lo for r in R)
    seen = []
    for r in R:
        for n in r.names:
            assert LD.layer_id(n, DEPTH) == r.layer and (not no_weight_decay(n, arena.specs[n])) == r.decayed, n
            lo, hi = arena.span(n)
            assert r.lo <= lo and hi <= r.hi
            seen.append(n)
    assert seen == list(arena.order)
    assert all((a.layer, a.decayed) != (b.layer, b.decayed) for a, b in zip(R, R[1:]))                  # maximal
    assert [r.layer for r in R[:14]] == [14] + list(range(12, -1, -1)) and all(r.decayed for r in R[:14])
    assert [r.layer for r in R[14:]] == list(range(0, 15)) and not any(r.decayed for r in R[14:])
    assert R[13].hi == arena.n_decay
    rows = plan.range_rows()
    assert rows.shape == (29, 2) and rows.dtype == torch.float32
    assert rows[:, 1].tolist() == [1.0] * 14 + [0.0] * 15 and rows[0, 0] == 1.0 and float(rows[14, 0]) == pytest.approx(0.75 ** 14, rel=1e-6)
    # the block table: bounded rows that never cross a range and cover the same elements
    for chunk in (1 << 12, 1 << 16, 256):
        tab = plan.block_table(chunk)
        assert tab.dtype == torch.int32 and tab.shape[1] == 3
        covered = torch.zeros(arena.n, dtype=torch.int32)
        for r, lo, hi in tab.tolist():
            assert R[r].lo <= lo < hi <= R[r].hi and hi - lo <= chunk and lo % 4 == 0 and hi % 4 == 0
            covered[lo:hi] += 1
        assert bool((covered == 1).all())
    # --no-grad: the classifier's two tensors only, both at the full rate
    head = LD.LayerDecayPlan(arena, DEPTH, 0.75, names=("head.weight", "head.bias"))
    assert [(r.lo, r.hi) for r in head.ranges] == [arena.span("head.weight"), arena.span("head.bias")]
    assert [(r.layer, r.decayed) for r in head.ranges] == [(14, True), (14, False)]
    assert head.range_rows().tolist() == [[1.0, 1.0], [1.0, 0.0]] and head.scales == {"head.weight": 1.0, "head.bias": 1.0}


def test_flag_is_parsed_checked_and_used():
    sys.path.insert(0, ROOT)
    import train
    from gipvit.cli_spec import REFERENCE_FLAGS
    args, _ = train.parse_args(["--model", "vit_tiny", "--layer-decay", "0.75"])
    assert args.layer_decay == 0.75
    train.check_supported(args, lambda m: None)
    for bad in (["--layer-decay", "0"], ["--layer-decay", "-1"], ["--dino", "--layer-decay", "0.75"]):
        a, _ = train.parse_args(["--model", "vit_tiny"] + bad)
        with pytest.raises(SystemExit):
            train.check_supported(a, lambda m: None)
    a, _ = train.parse_args(["--model", "vit_tiny"])
    assert a.layer_decay is None
    entry = [e for e in REFERENCE_FLAGS if e["flags"] == ["--layer-decay"]]
    assert len(entry) == 1 and entry[0]["used"] is True
    from gipvit.engine import SupervisedEngine
    import inspect
    assert inspect.signature(SupervisedEngine.__init__).parameters["layer_decay"].default is None


def test_mean_group_rate():
    """The reference's log line and summary.csv print the mean rate over the optimizer's parameter groups."""
    from gipvit import layer_decay as LD
    arena = _arena()
    plan = LD.LayerDecayPlan(arena, DEPTH, 0.75)
    groups = [0.75 ** (14 - lay) for lay in range(15) for dec in (True, False) if not (lay == 13 and dec)]   # norm has no decayed tensor
    assert len(groups) == 29 and len(plan.group_scales) == 29
    want = sum(1e-3 * s for s in groups) / 29
    assert plan.mean_lr(1e-3) == pytest.approx(want, rel=1e-12) and plan.mean_lr(1e-3) < 0.3e-3
    assert LD.LayerDecayPlan(arena, DEPTH, 1.0).mean_lr(1e-3) == 1e-3
    assert LD.LayerDecayPlan(arena, DEPTH, 0.75, names=("head.weight", "head.bias")).mean_lr(1e-3) == 1e-3


def test_entry_point_is_bound_and_checks_its_arguments_without_gpu():
    from gipvit import _lib
    assert _lib.ENTRY_POINTS["gv_adamw_ema_ranges"] is _lib.gv_adamw_ema_ranges_args
    assert [f[0] for f in _lib.gv_lamb_args._fields_][-1] == "lr_scale"
    assert [f[0] for f in _lib.gv_adamw_ema_ranges_args._fields_][:len(_lib.gv_adamw_ema_args._fields_)] == [f[0] for f in _lib.gv_adamw_ema_args._fields_]

    def good():
        a = _lib.gv_adamw_ema_ranges_args()
        a.p = a.grad = a.m = a.v = a.blocks = a.ranges = 256
        a.n, a.n_blocks, a.n_ranges, a.bias_corr1, a.bias_corr2 = 64, 1, 1, 0.1, 0.001
        return a

    def fails(a, code, word):
        with pytest.raises(_lib.GipvitError, match=word):
            _lib.call("gv_adamw_ema_ranges", a, 0)
        assert _lib.lib.gv_adamw_ema_ranges(ctypes.byref(a), None) == code

    a = good(); a.blocks = None
    fails(a, -3, "null")
    a = good(); a.ranges = None
    fails(a, -3, "null")
    a = good(); a.n_blocks = 0
    fails(a, -1, "empty")
    a = good(); a.n_ranges = 0
    fails(a, -1, "empty")
    for mode in (3, -1):
        a = good(); a.mode = mode
        fails(a, -4, "mode")
    a = good(); a.clip_norm = a.clip_value = 1.0; a.gnorm_sq = 256
    fails(a, -4, "exclude")
    a = good(); a.clip_norm = 1.0
    fails(a, -3, "gnorm_sq")
    a = good(); a.p = 260
    fails(a, -2, "aligned")
    a = good(); a.n = 66
    fails(a, -1, "multiple of 4")
    fails(_lib.gv_adamw_ema_ranges_args(), -3, "null")
