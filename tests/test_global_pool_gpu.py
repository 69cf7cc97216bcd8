"""GPU: ``--gp avg`` -- gv_token_mean_fwd / gv_token_mean_bwd against float64 through ``ops`` (the contracts of
tests/test_global_pool_host.py), the supervised step of a mean-pooled model against that module's reference at the gates of
tests/test_engine_gpu.py (logits 2e-2 of max |ref|, loss 1e-3, per-parameter gradient 5e-2, gradient norm 1e-2; the fp32 operand
mode: logits 1e-4, loss 1e-4, gradient norm 1e-3), what sits downstream of the pooled feature (soft-target / BCE losses with mix
and erase plans, LAMB, the clip modes, the data-parallel reducer), training, the forward-only extractor, the driver end to end and the float16
build in a process of its own."""
import math
import os
import subprocess
import sys

import pytest
import torch

import test_global_pool_host as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENT = 3, -768.0


def guarded(rows, cols, dtype, dev):
    """(whole buffer, the [rows, cols] view between GUARD sentinel rows in front of it and behind it)."""
    buf = torch.full((rows + 2 * GUARD, cols), SENT, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf, rows):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + rows:] == SENT).all())


# (n_img, N, D): a single patch row; odd sizes; the ViT widths; 256- and 512-px sequences; a width that is no multiple of the
# 64-column slab (the last slab's lanes past D stay idle)
POOL_SHAPES = [(1, 2, 192), (3, 17, 384), (5, 37, 192), (2, 257, 768), (2, 1025, 384), (4, 9, 100)]


def run_pool_kernels(ops, dev, n_img, N, D, act, with_scale):
    x, dpool, scale = H.pool_case(n_img, N, D)
    pbuf, pooled = guarded(n_img, D, torch.float32, dev)
    ops.token_mean_fwd(x.to(dev), pooled, n_img, N, D)
    again = torch.empty(n_img, D, dtype=torch.float32, device=dev)
    ops.token_mean_fwd(x.to(dev).clone(), again, n_img, N, D)
    gbuf, g = guarded(n_img * N, D, torch.float32, dev)
    bbuf, gb = guarded(n_img * N, D, act, dev)
    ops.token_mean_bwd(dpool.to(dev), g, gb, n_img, N, D, gb_scale=scale.to(dev) if with_scale else None)
    torch.cuda.synchronize()
    assert guards_intact(pbuf, n_img) and guards_intact(gbuf, n_img * N) and guards_intact(bbuf, n_img * N), "a kernel wrote outside its buffer"
    assert torch.equal(pooled, again), "two runs of the pooled mean differ"
    ratio = H.assert_pool_fwd(pooled.cpu(), x, n_img, N)
    H.assert_pool_bwd(g.cpu(), gb.cpu(), dpool, scale if with_scale else None, n_img, N)
    return ratio


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("n_img,N,D", POOL_SHAPES)
def test_token_mean_kernels(dev, n_img, N, D, with_scale):
    from gipvit import ops
    for act in (ops.bf16, torch.float32):
        ratio = run_pool_kernels(ops, dev, n_img, N, D, act, with_scale)
    print(f"[token mean {n_img}x{N}x{D}] forward error / bound {ratio:.3f}")


def test_token_mean_ops_refuse_wrong_dtypes_and_shapes(dev):
    from gipvit import _lib as L, ops
    f = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    with pytest.raises(TypeError):
        ops.token_mean_fwd(f(6, 192, dt=ops.bf16), f(2, 192), 2, 3, 192)
    with pytest.raises(TypeError):
        ops.token_mean_fwd(f(6, 192), f(2, 192, dt=torch.float64), 2, 3, 192)
    with pytest.raises(TypeError):
        ops.token_mean_bwd(f(2, 192, dt=ops.bf16), f(6, 192), f(6, 192, dt=ops.bf16), 2, 3, 192)
    with pytest.raises(TypeError):
        ops.token_mean_bwd(f(2, 192), f(6, 192), f(6, 192, dt=torch.float64), 2, 3, 192)
    with pytest.raises(TypeError):
        ops.token_mean_bwd(f(2, 192), f(6, 192), f(6, 192, dt=ops.bf16), 2, 3, 192, gb_scale=f(2, dt=torch.float64))
    with pytest.raises(ValueError):
        ops.token_mean_fwd(f(5, 192), f(2, 192), 2, 3, 192)                       # x is a row short
    with pytest.raises(L.GipvitError, match="N >= 2"):
        ops.token_mean_fwd(f(2, 192), f(2, 192), 2, 1, 192)
    with pytest.raises(L.GipvitError, match="multiple of 4"):
        ops.token_mean_bwd(f(2, 6), f(6, 6), f(6, 6, dt=ops.bf16), 2, 3, 6)


# --------------------------------------------------------------------------- #
# step parity
# --------------------------------------------------------------------------- #
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def check_grads(got, ref, named, tol=5e-2, norm_tol=1e-2):
    worst, gg, gr = [], 0.0, 0.0
    assert set(got) == set(ref)
    for k, r in ref.items():
        g = got[k]
        gg += float((g.double() ** 2).sum()); gr += float((r.double() ** 2).sum())
        if float(r.abs().max()) >= 1e-12:
            worst.append((_rel(g, r), k))
    worst.sort(reverse=True)
    assert worst[0][0] <= tol, f"gradient mismatch: {worst[:8]}"
    for k in named:
        assert float(ref[k].abs().max()) >= 1e-12 and _rel(got[k], ref[k]) <= tol, (k, _rel(got[k], ref[k]))
    gn = abs(math.sqrt(gg) - math.sqrt(gr)) / math.sqrt(gr)
    assert gn <= norm_tol, f"grad-norm rel err {gn}"
    return worst[0], gn


STEP_CONFIGS = {
    "tiny64": dict(arch="vit_tiny", img=64, B=8),
    "small96": dict(arch="vit_small", img=96, B=4),
    "small256": dict(arch="vit_small", img=256, B=2),
    "tiny64_droppath": dict(arch="vit_tiny", img=64, B=8, drop_path=0.5),
    "small96_droppath": dict(arch="vit_small", img=96, B=4, drop_path=0.5),
    "tiny64_dropout": dict(arch="vit_tiny", img=64, B=8, drop_path=0.2, dropout=(0.15, 4242)),
    "tiny64_fp32": dict(arch="vit_tiny", img=64, B=8, precision="fp32"),
}


@pytest.mark.parametrize("cid", list(STEP_CONFIGS))
def test_avg_step_parity(dev, cid):
    from gipvit.engine import SupervisedEngine
    from oracle import vit_oracle as vo
    c = STEP_CONFIGS[cid]
    arch, img, B, precision = c["arch"], c["img"], c["B"], c.get("precision", "bf16")
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    p = H.avg_params(arch, img, 2, seed=0)
    tiles = vo.synth_tiles(B, img, seed=1234)
    tgt = torch.randint(0, 2, (B, 1), generator=torch.Generator().manual_seed(5))
    drop = dropout = None
    eng = SupervisedEngine(arch=arch, img_size=img, num_classes=2, batch=B, device=dev, precision=precision, global_pool="avg")
    eng.load_state(p)
    if "drop_path" in c:
        drop = vo.drop_path_factors(12, B, c["drop_path"], torch.Generator().manual_seed(9))
        last = drop[11, 1]
        assert float(last.min()) == 0.0 and float(last.max()) > 1.0          # the pool's gb_scale drops some images and scales the others
        eng.set_drop_path(drop.to(dev))
    if "dropout" in c:
        dropout = c["dropout"]
        eng.set_dropout(*dropout)
    loss_r, grads_r, logits_r = H.avg_forward_backward(p, tiles, tgt, arch, img, drop=drop, dropout=dropout, fp64=precision == "fp32")
    eng.forward_backward(tiles.to(dev), tgt.to(dev))
    torch.cuda.synchronize()
    assert not eng.vit._cls_tail(eng.grp) and eng.vit.fused == (arch == "vit_small" and precision == "bf16")
    dlog = float((eng.logits.cpu().double() - logits_r.double()).abs().max())
    dl = abs(float(eng.loss) - float(loss_r))
    named = ("fc_norm.weight", "fc_norm.bias", "blocks.11.mlp.fc2.bias")
    got = eng.grads()
    print(f"[avg step {cid}] logits err {dlog:.2e} (max |ref| {float(logits_r.abs().max()):.3f})  |dloss| {dl:.2e}  "
          + "  ".join(f"{k} {_rel(got[k], grads_r[k]):.2e}" for k in named))
    if precision == "fp32":
        assert dlog <= 1e-4 and dl <= 1e-4, (dlog, dl)
        worst, gn = check_grads(got, grads_r, named, norm_tol=1e-3)
    else:
        assert dlog <= 2e-2 * float(logits_r.abs().max()), (dlog, float(logits_r.abs().max()))
        assert dl <= 1e-3, (float(eng.loss), float(loss_r))
        worst, gn = check_grads(got, grads_r, named)
    print(f"[avg step {cid}] worst grad {worst[0]:.2e} ({worst[1]})  grad-norm rel {gn:.2e}")


# --------------------------------------------------------------------------- #
# training
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("kw", [{}, dict(layer_decay=0.75, model_ema_decay=0.9)], ids=["plain", "layer_decay_ema"])
def test_avg_training_lowers_the_loss(dev, kw):
    from gipvit import models as M
    from gipvit.engine import SupervisedEngine
    from oracle import vit_oracle as vo
    eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, lr=1e-3, weight_decay=0.05, device=dev, global_pool="avg", **kw)
    eng.load_state(M.init_vit_state("vit_tiny", 64, 2, seed=0, global_pool="avg"))
    tiles = vo.synth_tiles(8, 64, seed=1234).to(dev)
    tgt = torch.randint(0, 2, (8, 1), generator=torch.Generator().manual_seed(5)).to(dev)
    losses = [float(eng.step(tiles, tgt)) for _ in range(20)]
    assert all(math.isfinite(l) for l in losses) and losses[-1] < losses[0] - 0.05, losses
    sd = eng.state_dict()
    assert float((sd["fc_norm.weight"] - 1).abs().max()) > 0 and float(sd["fc_norm.bias"].abs().max()) > 0
    if kw:
        assert eng.layer_scales["fc_norm.weight"] == 1.0 and eng.layer_scales["blocks.0.norm1.weight"] == 0.75 ** 13
        ema = eng.state_dict(ema=True)
        assert float((ema["fc_norm.weight"] - 1).abs().max()) > 0 and not torch.equal(ema["fc_norm.weight"], sd["fc_norm.weight"])    # the EMA copy moves


def test_avg_head_only_fine_tune_leaves_fc_norm_alone(dev):
    """--no-grad: the reference freezes every parameter and re-enables the classifier's two; fc_norm stays where it was."""
    from gipvit import models as M
    from gipvit.engine import SupervisedEngine
    from oracle import vit_oracle as vo
    eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, lr=1e-3, weight_decay=0.05, device=dev, global_pool="avg",
                           train_backbone=False)
    st = M.init_vit_state("vit_tiny", 64, 2, seed=0, global_pool="avg")
    eng.load_state(st)
    tiles = vo.synth_tiles(8, 64, seed=1234).to(dev)
    tgt = torch.randint(0, 2, (8, 1), generator=torch.Generator().manual_seed(5)).to(dev)
    for _ in range(3):
        eng.step(tiles, tgt)
    sd = eng.state_dict()
    assert torch.equal(sd["fc_norm.weight"].cpu(), st["fc_norm.weight"]) and torch.equal(sd["blocks.11.mlp.fc2.weight"].cpu(), st["blocks.11.mlp.fc2.weight"])
    assert not torch.equal(sd["head.weight"].cpu(), st["head.weight"])


# --------------------------------------------------------------------------- #
# downstream of the pooled feature: soft-target / BCE losses with mix and erase plans, LAMB, the clip modes, the DP reducer
# --------------------------------------------------------------------------- #
def _no_decay(name, shape):
    return len(shape) <= 1 or name.endswith(".bias") or name in ("pos_embed", "cls_token")


def _close(got, want, rtol=1e-5, atol=1e-6):
    got, want = got.double().cpu(), want.double().cpu()
    return bool(((got - want).abs() <= atol + rtol * want.abs()).all()), float((got - want).abs().max())


@pytest.mark.parametrize("kind,thr", [("soft_ce", None), ("bce", 0.2)])
def test_avg_step_with_mix_and_erase_plans(dev, kind, thr):
    """The mean-pooled ViT-T under timm's Mixup target and both batch plans (blend + paste rows, 'rand' erase boxes after the mix),
    against the reference on the restated batch: the gates of test_avg_step_parity."""
    import mixup_worker as mw
    from gipvit.engine import SupervisedEngine
    from gipvit.erasing import EraseSampler, apply_reference
    from gipvit.mixup import MixPlan
    from oracle import vit_oracle as vo
    B, S = 8, 64
    p = H.avg_params("vit_tiny", S, 2, seed=0)
    x = vo.normalize_window(vo.synth_tiles(B, S, seed=1234), (0, 0, S))
    tgt = torch.tensor([0, 1, 1, 0, 1, 0, 0, 0]).view(B, 1)
    rows = MixPlan.make_rows(B)
    MixPlan.set_row(rows, 0, 0.3, None); MixPlan.set_row(rows, B - 1, 0.3, None)
    MixPlan.set_row(rows, 1, 1.0 - (30 * 22) / float(S * S), (7, 37, 9, 31)); MixPlan.set_row(rows, 2, 0.85, None)
    erase = EraseSampler(0.75, "rand", 3, B, S, seed=4).sample(dev)
    assert set(rows["mode"].tolist()) == {0, 1, 2} and int((erase.rows["n_box"] > 0).sum()) > 0
    sp = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    logits_r = H.avg_logits(sp, apply_reference(mw.mix_images(x, rows), erase), "vit_tiny")
    dense = mw.mixup_target(tgt, 2, torch.from_numpy(rows["lam"].copy()), torch.from_numpy(rows["partner"].copy()), 0.1)
    loss_r = mw.mix_loss(logits_r, dense, kind, thr)
    loss_r.backward()
    grads_r, logits_r, loss_r = {k: v.grad for k, v in sp.items()}, logits_r.detach(), loss_r.detach()
    eng = SupervisedEngine(arch="vit_tiny", img_size=S, num_classes=2, batch=B, device=dev, loss=kind, bce_target_thresh=thr, global_pool="avg")
    eng.load_state(p)
    plan = MixPlan(rows, dev)
    eng.forward_backward(x.to(dev), tgt.to(dev), mix=plan, erase=erase)
    torch.cuda.synchronize()
    dlog, dl = float((eng.logits.cpu() - logits_r).abs().max()), abs(float(eng.loss) - float(loss_r))
    print(f"[avg {kind} mix + erase] logits err {dlog:.2e} (max |ref| {float(logits_r.abs().max()):.3f})  |dloss| {dl:.2e}")
    assert dlog <= 2e-2 * float(logits_r.abs().max()) and dl <= 1e-3, (dlog, dl)
    check_grads(eng.grads(), grads_r, ("fc_norm.weight", "fc_norm.bias", "blocks.11.mlp.fc2.bias"))
    assert math.isfinite(float(eng.step(x.to(dev), tgt.to(dev), mix=plan, erase=erase)))


@pytest.mark.parametrize("layer_decay", [0.75, None])
def test_avg_lamb_steps_match_oracle(dev, layer_decay):
    """opt='lamb' (with and without --layer-decay) over an arena that holds fc_norm.*: three fp32 steps against the oracle's Lamb fed the
    engine's own gradients, each tensor's update scaled by its layer's rate (fc_norm.*: the classifier's, 1) -- the tolerances of
    tests/test_layer_decay_gpu.py."""
    from gipvit.engine import SupervisedEngine
    from oracle import vit_oracle as vo
    lr, wd = 1e-3, 0.05
    eng = SupervisedEngine("vit_tiny", 64, 2, batch=8, precision="fp32", layer_decay=layer_decay, lr=lr, weight_decay=wd, opt="lamb", eps=1e-6,
                           device=dev, global_pool="avg")
    state = H.avg_params("vit_tiny", 64, 2, seed=0)
    eng.load_state(state)
    scale = {n: 1.0 for n in state}
    if layer_decay is not None:
        scale = eng.layer_scales
        assert scale["fc_norm.weight"] == scale["fc_norm.bias"] == scale["head.weight"] == 1.0 and scale["blocks.11.norm1.weight"] == 0.75 ** 2
    ref = vo.Lamb({n: q.clone().float() for n, q in state.items()}, lr=lr, wd=wd)
    for step in range(3):
        tiles = vo.synth_tiles(8, 64, seed=100 + step).to(dev)
        tgt = torch.randint(0, 2, (8, 1), generator=torch.Generator().manual_seed(step)).to(dev)
        eng.forward_backward(tiles, tgt)
        grads = {n: g.cpu() for n, g in eng.grads().items()}
        eng.optimizer_step()
        before = {n: q.clone() for n, q in ref.p.items()}
        ref.step(grads)
        for n in state:
            ref.p[n].copy_(before[n] + scale[n] * (ref.p[n] - before[n]))
        got = eng.state_dict()
        for n in state:
            ok, mx = _close(got[n], ref.p[n])
            assert ok, f"lamb step {step} {n}: max err {mx:.4g}"
    assert not torch.equal(got["fc_norm.weight"].cpu(), state["fc_norm.weight"]) and not torch.equal(got["fc_norm.bias"].cpu(), state["fc_norm.bias"])


@pytest.mark.parametrize("clip_mode", ["norm", "value", "agc"])
def test_avg_clip_modes(dev, clip_mode):
    """--clip-mode norm / value / agc over an arena that holds fc_norm.*: one fp32 adamw step against torch's AdamW on the engine's own
    gradients clipped on the CPU (clip_grad_norm_, clamp, the oracle's adaptive_clip_grad with the classifier left out), at a
    threshold that bites."""
    from gipvit.engine import SupervisedEngine
    from oracle import vit_oracle as vo
    lr, wd = 1e-3, 0.05
    clip = {"norm": 0.05, "value": 2e-4, "agc": 0.01}[clip_mode]
    eng = SupervisedEngine("vit_tiny", 64, 2, batch=8, precision="fp32", lr=lr, weight_decay=wd, opt="adamw", clip_grad=clip, clip_mode=clip_mode,
                           device=dev, global_pool="avg")
    state = H.avg_params("vit_tiny", 64, 2, seed=0)
    eng.load_state(state)
    tiles = vo.synth_tiles(8, 64, seed=100).to(dev)
    tgt = torch.randint(0, 2, (8, 1), generator=torch.Generator().manual_seed(0)).to(dev)
    eng.forward_backward(tiles, tgt)
    grads = {n: g.cpu() for n, g in eng.grads().items()}
    eng.optimizer_step()
    torch.cuda.synchronize()
    cpu = {n: q.clone().float().requires_grad_(True) for n, q in state.items()}
    if clip_mode == "agc":
        clipped = vo.adaptive_clip_grad({n: q.detach() for n, q in cpu.items()}, grads, clip, skip=("head.weight", "head.bias"))
        assert not torch.equal(clipped["blocks.11.mlp.fc2.bias"], grads["blocks.11.mlp.fc2.bias"])       # a zero bias: max_norm = clip x eps, it bites
        for n in state:        # the engine clips the arena in place
            ok, mx = _close(eng.grads()[n], clipped[n], 1e-5, 1e-7)
            assert ok, f"agc {n}: max err {mx:.4g}"
    else:
        clipped = {n: g.clone() for n, g in grads.items()}
        if clip_mode == "norm":
            total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))
            assert total > clip
            for n in clipped:
                clipped[n] *= min(1.0, clip / (total + 1e-6))
        else:
            assert float(grads["fc_norm.bias"].abs().max()) > clip
            for n in clipped:
                clipped[n].clamp_(-clip, clip)
    opt = torch.optim.AdamW([dict(params=[q], weight_decay=0.0 if _no_decay(n, q.shape) else wd) for n, q in cpu.items()], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    for n, q in cpu.items():
        q.grad = clipped[n].clone()
    opt.step()
    got = eng.state_dict()
    for n in state:
        ok, mx = _close(got[n], cpu[n].detach())
        assert ok, f"{clip_mode} {n}: max err {mx:.4g}"
    assert not torch.equal(got["fc_norm.weight"].cpu(), state["fc_norm.weight"])


DP_NAMES = ("fc_norm.weight", "fc_norm.bias", "blocks.11.mlp.fc2.bias", "blocks.0.attn.qkv.weight", "pos_embed", "head.weight")


def _dp_engine(B, reducer=None):
    from gipvit.engine import SupervisedEngine
    eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=B, lr=1e-3, weight_decay=0.05, device="cuda:0", reducer=reducer,
                           global_pool="avg")
    eng.load_state(H.avg_params("vit_tiny", 64, 2, seed=0))
    return eng


def _dp_batch():
    from oracle import vit_oracle as vo
    return vo.synth_tiles(4, 64, seed=99), torch.tensor([0, 1, 1, 0]).view(4, 1)


def _dp_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gipvit.dist import RcclReducer, shard_range
    eng = _dp_engine(2, RcclReducer())
    lo, hi = shard_range(4, rank, world)
    tiles, tgt = _dp_batch()
    tiles, tgt = tiles[lo:hi].to("cuda:0"), tgt[lo:hi].to("cuda:0")
    eng.forward_backward(tiles, tgt)
    torch.cuda.synchronize()
    gr = eng.grads()
    gsel = {k: gr[k].cpu().numpy() for k in DP_NAMES}
    loss = float(eng.loss)
    eng.optimizer_step()
    torch.cuda.synchronize()
    sd = eng.state_dict()
    q.put((rank, loss, gsel, {k: sd[k].cpu().numpy() for k in DP_NAMES}))        # numpy payloads: pickled by value
    dist.destroy_process_group()


def test_avg_two_ranks_match_single_process(dev):
    """The data-parallel reducer over an arena that holds fc_norm.* (two ranks on the one GPU over gloo, as tests/test_dp_gpu.py): the
    reduced gradient x 1 / world equals one process's gradient on the four tiles, the replicas stay identical after the step."""
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ps = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = sorted([q.get(timeout=300) for _ in ps], key=lambda t: t[0])
    [p.join(60) for p in ps]
    one = _dp_engine(4)
    tiles, tgt = _dp_batch()
    one.forward_backward(tiles.to(dev), tgt.to(dev))
    torch.cuda.synchronize()
    g1 = one.grads()
    assert abs((res[0][1] + res[1][1]) / 2 - float(one.loss)) < 1e-4
    start = H.avg_params("vit_tiny", 64, 2, seed=0)
    for k in DP_NAMES:
        assert (res[0][2][k] == res[1][2][k]).all() and (res[0][3][k] == res[1][3][k]).all(), k          # both replicas: the same arena, the same update
        r = _rel(torch.from_numpy(res[0][2][k]) * 0.5, g1[k])
        assert r < 2e-2, (k, r)                                           # bf16 noise only; a wrong 1 / world is a factor 2
        assert not (res[0][3][k] == start[k].numpy()).all(), k              # ... and the step moved it


# --------------------------------------------------------------------------- #
# extractor
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("img", [64, 272])
def test_avg_extractor_matches_the_engine_and_the_reference(dev, img):
    from gipvit.engine import FeatureExtractor, SupervisedEngine
    from oracle import vit_oracle as vo
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    B = 2
    p = H.avg_params("vit_tiny", img, 2, seed=2)
    eng = SupervisedEngine(arch="vit_tiny", img_size=img, num_classes=2, batch=B, device=dev, global_pool="avg")
    eng.load_state(p)
    tiles = vo.synth_tiles(B, img, seed=31)
    x = tiles.to(dev)
    logits, feats = eng.forward(x)
    logits, feats = logits.clone(), feats.float().clone()
    fx = FeatureExtractor("vit_tiny", img, B, 2, eng.mean, eng.std, dev, weights=eng.W, global_pool="avg")
    f2, l2 = fx.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(feats, f2.float()) and torch.equal(logits, l2)
    ref = H.avg_features(p, vo.normalize_window(tiles, (0, 0, img)), "vit_tiny")
    err = _rel(f2.float(), ref)
    print(f"[avg extractor {img} px] features rel err {err:.2e}")
    assert err <= 2e-2, err
    # run(): any number of tiles, the last batch padded
    three = torch.cat([x, x[:1]])
    fr, lr_ = fx.run(three)
    assert fr.shape == (3, 192) and torch.equal(fr[:2], feats) and torch.equal(fr[2], feats[0]) and torch.equal(lr_[:2], logits)
    with pytest.raises(ValueError, match="final norm"):
        fx.intermediate_layers(x)
    if img == 272:
        with pytest.raises(ValueError, match="288-token limit"):
            fx.last_selfattention(x)
        with pytest.raises(ValueError, match="288-token limit"):
            eng.forward_backward(x, torch.zeros(B, 1, dtype=torch.int64, device=dev))
        return
    # the attention maps involve no norm: the same as a CLS-token extractor's over the same block weights
    tok = FeatureExtractor("vit_tiny", img, B, 2, eng.mean, eng.std, dev)
    tok.load_state({k.replace("fc_norm.", "norm."): v for k, v in p.items()})
    a_avg, a_tok = fx.last_selfattention(x), tok.last_selfattention(x)
    torch.cuda.synchronize()
    assert a_avg.shape == (B, 3, 17, 17) and torch.equal(a_avg, a_tok)
    assert not torch.equal(tok.forward(x)[0].float(), feats)              # ... while the features are another function of the tokens


def test_avg_model_seam(dev):
    from gipvit import models as M
    model = M.create_model("vit_tiny_patch16_224", num_classes=2, img_size=64, batch=2, device=dev, global_pool="avg")
    assert model.engine.pool == "avg" and "fc_norm.weight" in model.state_dict() and "norm.weight" not in model.state_dict()
    assert M.create_model("vit_tiny_patch16_224", num_classes=2, img_size=64, batch=2, device=dev).engine.pool == "token"
    x = torch.zeros(2, 64, 64, 3, dtype=torch.uint8, device=dev)
    assert model(x).shape == (2, 2) and model.forward_features(x).shape == (2, 192)
    assert model.get_last_selfattention(x).shape == (2, 3, 17, 17)
    with pytest.raises(ValueError, match="final norm"):
        model.get_intermediate_layers(x)
    with pytest.raises(ValueError, match="global_pool"):
        M.create_model("vit_tiny_patch16_224", num_classes=2, img_size=64, batch=2, device=dev, global_pool="")


# --------------------------------------------------------------------------- #
# the driver
# --------------------------------------------------------------------------- #
def _driver_args(tmp_path):
    return ["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "--num-classes", "2", "--img-size", "64", "--tile-size", "64",
            "-b", "8", "--batches-per-epoch", "4", "--opt", "adamw", "--lr-base", "0.01", "--warmup-epochs", "0", "--log-interval", "2",
            "--output", str(tmp_path), "--seed", "1", "--synthetic-slides", "2", "--num_tiles", "11", "--tiles_per_iter", "4",
            "--model-ema", "--model-ema-decay", "0.9"]


def test_train_py_gp_avg_trains_and_resumes(dev, tmp_path, caplog):
    sys.path.insert(0, ROOT)
    import train
    base = _driver_args(tmp_path) + ["--gp", "avg"]
    with caplog.at_level("INFO"):
        assert train.main(base + ["--epochs", "1", "--experiment", "avg"]) == 0
    assert any("global pool: avg" in m for m in caplog.messages)
    assert not any("outside this build's hot path" in m and "--gp" in m for m in caplog.messages)
    ck = torch.load(tmp_path / "avg" / "last.pth.tar", weights_only=True)
    sd, ema = ck["state_dict"], ck["state_dict_ema"]
    assert "fc_norm.weight" in sd and "norm.weight" not in sd and set(ema) == set(sd)
    assert float((sd["fc_norm.weight"] - 1).abs().max()) > 0 and not torch.equal(ema["fc_norm.weight"], sd["fc_norm.weight"])
    # --resume restores the avg checkpoint (model, EMA copy, optimizer) and trains on
    assert train.main(base + ["--epochs", "2", "--experiment", "avg", "--resume", str(tmp_path / "avg" / "last.pth.tar")]) == 0
    ck2 = torch.load(tmp_path / "avg" / "last.pth.tar", weights_only=True)
    assert ck2["epoch"] == 1 and ck2["optimizer"]["step"] == 8 and not torch.equal(ck2["state_dict"]["fc_norm.weight"], sd["fc_norm.weight"])
    # a CLS-token model cannot take it
    with pytest.raises(KeyError, match="norm.weight"):
        train.main(_driver_args(tmp_path) + ["--epochs", "2", "--experiment", "tok", "--resume", str(tmp_path / "avg" / "last.pth.tar")])


def test_train_py_gp_avg_extracts_pooled_features(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import train
    feats = {}
    for gp in ("avg", "token"):
        fd = tmp_path / ("feats_" + gp)
        assert train.main(_driver_args(tmp_path) + ["--gp", gp, "--epochs", "1", "--experiment", "fx_" + gp, "--extract_features",
                                                    "--features-dir", str(fd)]) == 0
        assert sorted(os.listdir(fd)) == [f"synthetic_{k}_features.pt" for k in range(2)]
        feats[gp] = torch.load(fd / "synthetic_0_features.pt", weights_only=True)
        assert feats[gp].shape == (11, 192) and feats[gp].dtype == torch.float32 and bool(torch.isfinite(feats[gp]).all())
    # same seed, same weights but for the pooling: other features
    assert float((feats["avg"] - feats["token"]).abs().max()) > 0.05 and float(feats["avg"].std()) > 0.05
    with pytest.raises(SystemExit, match="--gp"):
        train.main(_driver_args(tmp_path) + ["--gp", "max", "--epochs", "1", "--experiment", "bad"])


# --------------------------------------------------------------------------- #
# float16 build
# --------------------------------------------------------------------------- #
def test_float16_build(dev):
    """tests/global_pool_f16_worker.py in a process of its own (GIPVIT_ACT_FORMAT=f16): the kernel checks at (3, 17, 384) and one
    vit_tiny avg step at the gates above."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "global_pool_f16_worker.py")], cwd=ROOT,
                       env=dict(os.environ, GIPVIT_ACT_FORMAT="f16"), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("POOL F16 OK"), (r.stdout[-2000:], r.stderr[-3000:])
