"""CPU: the stream order of the data-parallel step (tests/dp_order.py over tests/launch_trace.py recordings).

A range of the gradient arena released one block early, or from the wrong stream, or a gradient write that lands behind its
range's release, is a silent gradient corruption that one rank can never show and two ranks show only sometimes.  Here every
engine configuration with a launch order of its own runs one step on the CPU with a recording reducer of world size 2, and the
trace is held to the ordering properties P1-P6 of dp_order (module docstring there).  These runs are checked by property, not
by hash: they are not part of launch_trace.CONFIGS or of the fixture.

The checker is shown to bite on four doctored recordings (the trace is edited, never the engine)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_order
import launch_trace as lt


def _masks(eng, marked):
    """A MaskPlan over the engine's G * B global crops: ``marked`` patches in the first image, none elsewhere."""
    import numpy as np
    from gipvit.masking import MaskPlan
    m = np.zeros((eng.G * eng.B, (eng.gsize // 16) ** 2), np.bool_)
    m[0, 3:3 + marked] = True
    return MaskPlan(m, "cpu")


def _dino(arch, batch=1, **kw):
    def make(red):
        return lt._dino(arch, batch=batch, reducer=red, **kw)
    return make


def _step(eng):
    eng.step(lt._tiles(eng.B, 256))


def _micro2(eng):
    eng.step_micro([lt._tiles(eng.B, 256), lt._tiles(eng.B, 256)])


def _dropout_micro2(eng):
    eng.set_dropout(0.1, 7)
    eng.set_drop_path(torch.ones(12, 2, eng.V * eng.B))
    _micro2(eng)


def _frozen_last_layer(eng):
    eng.train_last_layer = False
    _step(eng)


def _sup(**kw):
    def make(red):
        return lt._sup(reducer=red, **kw)
    return make


def _sup_step(eng):
    eng.step(lt._tiles(2, 64), torch.zeros(2, 1, dtype=torch.int64))


B1 = dict(bucket_mb=1)
# id -> (EngineSwitches fields, engine factory (reducer ->), run (engine ->))
CASES = {
    "dino_s": (B1, _dino("vit_small"), _step),
    "dino_s_bucket25": ({}, _dino("vit_small"), _step),
    "dino_s_micro2": (B1, _dino("vit_small"), _micro2),
    "dino_s_ungrouped": (dict(B1, group_dw=False), _dino("vit_small"), _step),
    "dino_s_every_token": (dict(B1, cls_only_last=False), _dino("vit_small"), _step),
    "dino_t_fp32": (B1, _dino("vit_tiny", precision="fp32"), _step),
    "dino_t_clip": (B1, _dino("vit_tiny", clip_grad=3.0), _step),
    "dino_t_teacher_main": (dict(B1, teacher_side=False), _dino("vit_tiny"), _step),
    "dino_s_sinkhorn_koleo": (B1, _dino("vit_small", batch=2, centering="sinkhorn_knopp", koleo_weight=0.1), _step),
    "dino_t_dropout_micro2": (B1, _dino("vit_tiny"), _dropout_micro2),
    "dino_t_frozen_last_layer": (B1, _dino("vit_tiny"), _frozen_last_layer),
    "dino_s_ibot": (B1, _dino("vit_small", ibot_weight=1.0), lambda eng: eng.step(lt._tiles(1, 256), masks=_masks(eng, 20))),
    "dino_s_ibot_no_marked_patch": (B1, _dino("vit_small", ibot_weight=1.0), lambda eng: eng.step(lt._tiles(1, 256), masks=_masks(eng, 0))),
    "dino_t_ibot_micro2": (B1, _dino("vit_tiny", ibot_weight=1.0),
                           lambda eng: eng.step_micro([lt._tiles(1, 256)] * 2, masks=[_masks(eng, 0), _masks(eng, 9)])),
    "sup_adamw": (B1, _sup(), _sup_step),
    "sup_lamb": (B1, _sup(opt="lamb"), _sup_step),
    "sup_agc": (B1, _sup(clip_mode="agc", clip_grad=0.01), _sup_step),
    "sup_layer_decay": (B1, _sup(arch="vit_small", layer_decay=0.75), _sup_step),
}
MIN_RANGES = {"dino_s": 13, "dino_s_bucket25": 3}      # bucket_mb = 1: a ViT-S step releases block by block (head, 11 blocks, the end message)

_cache = {}


def traced(cid) -> dp_order.Trace:
    """One recording per configuration, shared by the tests that read it (none of them changes it)."""
    if cid not in _cache:
        switches, make, run = CASES[cid]
        with lt.recording(switches) as rec:
            eng = dp_order.instrument(make(dp_order.RecordingReducer(rec)), rec)
            run(eng)
        from gipvit.dist import reduction_plan
        a = eng.arena
        g = {v: k for k, v in rec.storage_names(a).items()}["g"]
        if hasattr(eng, "_reduction_plan"):
            plan = [(lo, hi) for _, lo, hi in eng._reduction_plan()]
            # ... which is dist.reduction_plan over this arena's own layout, worked out here from the arena alone
            head = [n for n in a.order if n.startswith("head.") and a.off[n] < a.n_decay]
            blocks = {}
            for i in range(len({n.split(".")[2] for n in a.order if n.startswith("backbone.blocks.")})):
                sp = [a.span(n) for n in a.order if n.startswith(f"backbone.blocks.{i}.") and a.off[n] < a.n_decay]
                blocks[i] = (min(lo for lo, _ in sp), max(hi for _, hi in sp))
            want = reduction_plan((min(a.off[n] for n in head), max(a.span(n)[1] for n in head)), blocks, a.n,
                                  bucket_bytes=switches.get("bucket_mb", 25) << 20)
            assert plan == [(lo, hi) for _, lo, hi in want]
        else:
            plan = [(lo, hi) for _, lo, hi in reduction_plan(None, {}, a.n)]       # the supervised step: one message
        _cache[cid] = dp_order.Trace(rec.events, g, a.n, plan)
    return _cache[cid]


@pytest.mark.parametrize("cid", list(CASES))
def test_data_parallel_step_is_ordered(cid):
    """P1-P6 hold: 0 violations.  The configuration really has an active reducer (ranges released, a finish, collectives for the
    centre sums) and, with 1-MB buckets, many ranges -- so the properties were checked on something."""
    tr = traced(cid)
    names = [e[0] for e in tr.events]
    assert names.count("reduce_range") == len(tr.plan) >= MIN_RANGES.get(cid, 1) and "finish" in names
    if cid.startswith("dino"):
        assert names.count("reduce_tensor") >= 1 + ("ibot" in cid) and "side.then.begin" in names
    if "sinkhorn" in cid:
        assert names.count("reduce_max") == 1 and names.count("reduce_tensor") == 1 + 3
    bad = dp_order.check(tr)
    assert not bad, f"{len(bad)} violations, the first: {bad[0]}"


def test_accumulation_reduces_from_the_last_micro_batch_only():
    """2 micro-batches: every collective of gradients and centre sums lies behind the second ``micro`` marker, one set per step."""
    for cid in ("dino_s_micro2", "dino_t_dropout_micro2", "dino_t_ibot_micro2"):
        ev = traced(cid).events
        second = next(i for i, e in enumerate(ev) if e[0] == "micro" and e[1] == 1)
        assert [e[0] for e in ev].count("micro") == 2
        assert all(i > second for i, e in enumerate(ev) if e[0] in dp_order.COLLECTIVES)


def _flagged(tr, events, tag, *words):
    bad = dp_order.check(dp_order.Trace(events, tr.g, tr.n, tr.plan))
    hits = [b for b in bad if b.startswith(tag) and all(w in b for w in words)]
    assert hits, (tag, words, len(bad), bad[:3])
    return bad


@pytest.mark.parametrize("cid", ["dino_s", "dino_s_ungrouped", "dino_t_fp32"])
def test_checker_flags_releases_issued_from_main(cid):
    """Doctored 1: the ``side.then`` markers around every reduce_range removed.  The weight gradients are produced on the side
    stream, so a release from main overtakes them: P2, first of all the head's weight-norm backward against the head range."""
    tr = traced(cid)
    bad = _flagged(tr, dp_order.releases_from_main(tr.events), "P2", "[side]", "issued on main")
    first = next(b for b in bad if b.startswith("P2"))
    assert "weightnorm_bwd [side]" in first and f"s{tr.g}:{tr.plan[0][0]}-{tr.plan[0][1]}" in first, first
    assert len([b for b in bad if b.startswith("P2")]) >= len(tr.plan) - 2        # every side-stream release but not the end message


@pytest.mark.parametrize("cid", ["dino_s", "dino_s_ungrouped", "dino_s_every_token", "dino_t_fp32"])
def test_checker_flags_a_block_released_one_launch_early(cid):
    """Doctored 2: one block's reduce_range moved in front of the ``side.run`` that holds that block's weight-gradient launch."""
    tr = traced(cid)
    _flagged(tr, dp_order.release_one_block_early(tr), "P3", "linear", "before the next finish")


@pytest.mark.parametrize("cid", ["dino_s", "dino_t_clip", "sup_adamw", "sup_lamb", "sup_agc"])
def test_checker_flags_a_missing_finish(cid):
    """Doctored 3: the step's last ``finish`` removed: the optimizer reads gradients that are still on the wire."""
    tr = traced(cid)
    _flagged(tr, dp_order.drop_last_finish(tr.events), "P6", "pending")


@pytest.mark.parametrize("cid", ["dino_t_teacher_main", "dino_s", "dino_t_fp32"])
def test_checker_flags_the_arena_fill_left_unjoined(cid):
    """Doctored 4: the join of the arena fill removed with every later join.  With the teacher on the main stream that join is
    the only edge behind the fill: ``Tensor.zero_`` of g on the side stream races the main stream's ln_finalize into the final
    norm's gradients (P1).  With the teacher on the side stream its join, which comes first and stays, covers the fill queued in
    front of it (one FIFO stream) -- there the recording is flagged for what the later joins ordered: the side stream's weight
    gradients against the optimizer."""
    tr = traced(cid)
    if cid == "dino_t_teacher_main":
        _flagged(tr, dp_order.drop_joins_from_fill(tr), "P1", "Tensor.zero_ [side]", "ln_finalize [main]")
    else:
        _flagged(tr, dp_order.drop_joins_from_fill(tr), "P1", "[side]", "adamw_ema [main]")


def test_checker_flags_a_wrong_plan_and_a_release_before_the_last_micro_batch():
    """P4 on doctored recordings: two releases swapped, one dropped, and a release moved into the first micro-batch."""
    tr = traced("dino_s_micro2")
    ev = tr.events
    idx = [i for i, e in enumerate(ev) if e[0] == "reduce_range"]
    swapped = list(ev)
    swapped[idx[2]], swapped[idx[3]] = ev[idx[3]], ev[idx[2]]
    _flagged(tr, swapped, "P4", "the plan is")
    _flagged(tr, ev[:idx[4]] + ev[idx[4] + 1:], "P4", "does not continue the tiling")
    first = next(i for i, e in enumerate(ev) if e[0] == "micro") + 1
    _flagged(tr, ev[:first] + [ev[idx[0]]] + ev[first:idx[0]] + ev[idx[0] + 1:], "P4", "before the step's last micro-batch")


def test_checker_flags_a_centre_sum_consumed_without_a_finish():
    """P5 on a doctored recording: Sinkhorn's first ``finish`` removed -- the column pass reads a shift that is still being
    reduced -- and a centre sum rewritten while its collective is in flight."""
    tr = traced("dino_s_sinkhorn_koleo")
    ev = tr.events
    f = next(i for i, e in enumerate(ev) if e[0] == "finish")
    assert ev[f - 1][0] == "reduce_max" and ev[f + 1][0] == "sinkhorn_cols"
    _flagged(tr, ev[:f] + ev[f + 1:], "P5", "sinkhorn_cols", "reduce_max")
    c = next(i for i, e in enumerate(ev) if e[0] == "reduce_tensor" and ev[i - 1][0] == "dino_loss")
    _flagged(tr, ev[:c + 1] + [ev[c - 1]] + ev[c + 1:], "P5", "dino_loss", "before the next finish")
