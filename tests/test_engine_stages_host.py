"""CPU: the stages of ``DinoEngine.forward_backward`` and ``VitRunner.forward`` on their own -- the micro-batch accumulation
helper on plain tensors, the crop-cutting stage under the launch recorder (tests/launch_trace.py), and every refusal of the two
functions: the same exception and words as before the stages existed, raised before anything is launched."""
import pytest
import torch

import launch_trace as lt

TILES = lt._tiles(2, 256)


# ------------------------------------------------------------------ accumulate_micro
@pytest.mark.parametrize("n", [1, 2, 3])
def test_accumulate_micro_mean_and_sum(n):
    from gipvit.engine import accumulate_micro
    g = torch.Generator().manual_seed(n)
    fed = [(torch.randn(1, generator=g), torch.randn(5, generator=g)) for _ in range(n)]
    loss, csum, acc = torch.empty(1), torch.empty(5), {}
    for j, (a, b) in enumerate(fed):
        loss.copy_(a); csum.copy_(b)            # what micro-batch j's launches leave in the step's outputs
        accumulate_micro(acc, ((loss, True), (csum, False)), j, n)
        if j < n - 1:                           # untouched before the last micro-batch
            assert torch.equal(loss, a) and torch.equal(csum, b)
    if n == 1:                                  # a step without accumulation: not a bit moves, nothing is kept
        assert torch.equal(loss, fed[0][0]) and torch.equal(csum, fed[0][1]) and acc == {}
        return
    want_a, want_b = fed[0][0].clone(), fed[0][1].clone()
    for a, b in fed[1:]:                        # the engine's arithmetic: a running f32 sum in micro-batch order, one division
        want_a, want_b = want_a + a, want_b + b
    assert torch.equal(loss, want_a / n) and torch.equal(csum, want_b)
    a64, b64 = torch.stack([a for a, _ in fed]).double(), torch.stack([b for _, b in fed]).double()
    assert torch.allclose(loss.double(), a64.mean(0), rtol=0, atol=2e-7 * float(a64.abs().sum()))
    assert torch.allclose(csum.double(), b64.sum(0), rtol=0, atol=2e-7 * float(b64.abs().sum(0).max()))


def test_accumulate_micro_starts_again_with_every_step():
    from gipvit.engine import accumulate_micro
    t, acc = torch.empty(1), {}
    for step in (1.0, 10.0):                    # the sums of the step before are dropped by the first micro-batch's clone
        for j in range(2):
            t.fill_(step * (j + 1))
            accumulate_micro(acc, ((t, False),), j, 2)
        assert float(t) == 3.0 * step


# ------------------------------------------------------------------ the crop-cutting stage
def _draws(views, stains):
    from gipvit.multicrop import MultiCropSampler, ViewAugmentSampler
    from gipvit.stain import StainJitterSampler
    return (MultiCropSampler(2, 256, 2, 2, seed=1).sample(), ViewAugmentSampler(2, 2, 2, seed=2).sample() if views else None,
            StainJitterSampler(2, 2, 2, 0.2, seed=3).sample() if stains else None)


@pytest.mark.parametrize("views,stains,name", [(False, False, "crop_resize"), (True, False, "crop_augment"), (True, True, "crop_augment_stain")])
def test_cut_crops_issues_one_launch_per_crop_group(views, stains, name):
    from gipvit.engine import DinoEngine
    with lt.recording() as rec:
        eng = DinoEngine(arch="vit_tiny", img_size=224, out_dim=256, batch=2, n_local=2, device="cpu")
        t_src, t_win, s_src, s_win = eng._cut_crops(TILES, *_draws(views, stains))
    assert [e[0] for e in rec.events] == [name, name]
    number = lambda t: rec.storages[t.untyped_storage().data_ptr()]
    assert [e[2]["out"]["tensor"][0] for e in rec.events] == [number(eng._gcrops), number(eng._lcrops)]
    assert [e[1][2 + 2 * views + stains] for e in rec.events] == [eng.gsize, eng.lsize]        # (tiles, boxes[, views[, stains], stats], size)
    assert tuple(eng._gcrops.shape) == (4, 224, 224, 3) and tuple(eng._lcrops.shape) == (4, 96, 96, 3)
    assert (eng._vstats is not None) == views
    assert t_src is eng._gcrops and t_win == [[(0, 0)]] and s_win == [[(0, 0)], [(0, 0)]]
    assert len(s_src) == 2 and s_src[0] is eng._gcrops and s_src[1] is eng._lcrops


def test_cut_crops_without_local_crops_and_without_boxes():
    with lt.recording() as rec:
        eng = lt._dino("vit_tiny", n_local=0)
        bg = torch.tensor([[0, y, x, 224, 224, 0] for (y, x) in eng.gwins], dtype=torch.int32)
        t_src, t_win, s_src, s_win = eng._cut_crops(lt._tiles(1, 256), (bg, None), None, None)
        assert [e[0] for e in rec.events] == ["crop_resize"] and eng._lcrops is None
        assert t_src is eng._gcrops and len(s_src) == 1 and s_src[0] is eng._gcrops and t_win == s_win == [[(0, 0)]]
        del rec.events[:]
        tiles = lt._tiles(1, 256)
        assert eng._cut_crops(tiles, None, None, None) == (tiles, [eng.gwins], tiles, eng.s_wins) and rec.events == []       # the fixed windows


# ------------------------------------------------------------------ refusals, before anything is launched
def _refused(rec, exc, words, call):
    del rec.events[:]
    with pytest.raises(exc) as info:
        call()
    assert words in str(info.value), str(info.value)
    assert rec.events == [], rec.events[:3]


def test_forward_backward_refuses_before_the_first_launch():
    boxes, views, stains = _draws(True, True)
    with lt.recording() as rec:
        eng = lt._dino("vit_tiny", batch=2, n_local=2)
        ibot = lt._dino("vit_tiny", ibot_weight=1.0)
        fb = eng.forward_backward
        _refused(rec, ValueError, "masks= goes with ibot_weight > 0: this engine was built without the iBOT term",
                 lambda: fb(TILES, masks=lt._masks(ibot, 3)))
        _refused(rec, ValueError, "masks= goes with ibot_weight > 0: an engine with the iBOT term needs a MaskPlan for every micro-batch",
                 lambda: ibot.forward_backward(lt._tiles(1, 256)))
        _refused(rec, ValueError, "masks: a plan for 4 images of 196 patches, the global crops are 2 images of 196",
                 lambda: ibot.forward_backward(lt._tiles(1, 256), masks=lt._masks(eng, 3)))
        _refused(rec, ValueError, "fill boxes are tile coordinates: they cannot be combined with re-cut random crops (boxes)",
                 lambda: fb(TILES, boxes=boxes, fill=torch.zeros(2, 8)))
        _refused(rec, ValueError, "views (per-crop augmentation draws) need boxes: the views are produced by the pass that cuts the crops",
                 lambda: fb(TILES, views=views))
        _refused(rec, ValueError, "stains (per-crop stain jitter draws) need views: the jitter runs inside the view-augmentation pass",
                 lambda: fb(TILES, boxes=boxes, stains=stains))
        _refused(rec, ValueError, "boxes= works on uint8 tiles", lambda: fb(torch.zeros(2, 3, 256, 256), boxes=boxes))
        _refused(rec, TypeError, "images: expected uint8 NHWC tiles", lambda: fb(TILES.double()))
        _refused(rec, ValueError, "images: expected float32 NCHW of shape (2, 3, 256, 256)", lambda: fb(torch.zeros(2, 3, 224, 224)))
        with pytest.raises(AssertionError):
            fb(TILES, boxes=(boxes[0][:2], boxes[1]))
        assert rec.events == []
        eng.step(TILES, boxes=boxes, views=views, stains=stains)            # ... and the accepted combination still runs
        assert [e[0] for e in rec.events if e[0].startswith("crop")] == ["crop_augment_stain"] * 2


def test_vit_forward_refuses_before_the_first_launch():
    from gipvit.engine import FeatureExtractor
    with lt.recording() as rec:
        dino, sup = lt._dino("vit_tiny"), lt._sup()
        fx = FeatureExtractor(arch="vit_tiny", img_size=64, batch=2, device="cpu")
        one, table = [[(0, 0)]], torch.zeros(4)
        multi = lambda **kw: dino.vit.forward(dino.sW, dino.g_stu, lt._tiles(1, 256), dino.s_wins, dino.mean, dino.std, dino.hb_s.feats, **kw)
        train = lambda **kw: sup.vit.forward(sup.W, sup.grp, lt._tiles(2, 64), one, sup.mean, sup.std, sup.feats, **kw)
        infer = lambda **kw: fx.vit.forward(fx.W, fx.grp, lt._tiles(2, 64), one, fx.mean, fx.std, fx.feats, **kw)
        stain = "stain: inference only -- a forward-only single-segment group without mix / erase tables (training is never normalised)"
        _refused(rec, ValueError, stain, lambda: train(stain=table))
        _refused(rec, ValueError, stain, lambda: infer(stain=table, mix=table))
        _refused(rec, ValueError, stain, lambda: infer(stain=table, erase=(table, 1)))
        _refused(rec, ValueError, "mix: the supervised step's one window of one segment only", lambda: multi(mix=table))
        _refused(rec, ValueError, "erase: the supervised step's one window of one segment only", lambda: multi(erase=(table, 1)))
        _refused(rec, ValueError, "erase: the supervised step's one window of one segment only",
                 lambda: sup.vit.forward(sup.W, sup.grp, lt._tiles(2, 64), [[(0, 0), (0, 0)]], sup.mean, sup.std, sup.feats, erase=(table, 1)))
        words = "masks / patch: the group must run its last block on every token (VitGroup.all_tokens)"
        _refused(rec, ValueError, words, lambda: multi(masks=lt._masks(dino, 3)))
        _refused(rec, ValueError, words, lambda: train(patch=(lt._masks(dino, 3), None)))
        _refused(rec, ValueError, "fill= works on uint8 tiles: not with float32 NCHW input",
                 lambda: sup.vit.forward(sup.W, sup.grp, torch.zeros(2, 3, 64, 64), one, sup.mean, sup.std, sup.feats, fill=torch.zeros(2, 8)))
        _refused(rec, ValueError, "stain= works on uint8 tiles: float32 NCHW input is already normalised, its bytes are gone",
                 lambda: fx.vit.forward(fx.W, fx.grp, torch.zeros(2, 3, 64, 64), one, fx.mean, fx.std, fx.feats, stain=table))
        infer(stain=table)                      # ... and the accepted one carries the keyword, alone
        assert rec.events[0][0] == "patchify" and sorted(rec.events[0][2]) == ["fill", "mix", "out", "stain"]
