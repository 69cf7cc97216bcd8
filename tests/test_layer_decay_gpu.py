"""GPU: --layer-decay.  gv_adamw_ema_ranges against torch's optimizers with one parameter group per range and, bit for bit,
against the gv_adamw_ema launches it replaces; gv_lamb's per-tensor rates against the oracle's Lamb; SupervisedEngine(layer_decay=)
against CPU optimizers whose groups come from a layer map written here; the driver's log line and summary.csv.

Tolerances: ``close(got, ref, 1e-5, 1e-6)`` for f32 parameters and the EMA copy is the one tests/test_kernels_gpu.py::test_adamw_ema
holds this arithmetic to; 16-bit copies must EQUAL the cast of the f32 result; the LAMB figures are test_lamb_matches_oracle's."""
import csv
import math
import os
import re
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = torch.float32


def ops():
    from gipvit import ops as o
    return o


def err_report(got, ref, rtol, atol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    return int(bad.sum()), bad.numel(), float(err.max())


def close(got, ref, rtol, atol, what=""):
    nbad, n, mx = err_report(got, ref, rtol, atol)
    print(f"[layer-decay] {what}: {nbad}/{n} off, max err {mx:.4g}")
    assert nbad == 0, f"{what}: {nbad}/{n} off, max err {mx:.4g}"


def make_ranges(sizes):
    spans, off = [], 0
    for s in sizes:
        assert s % 4 == 0
        spans.append((off, off + s)); off += s
    return spans, off


# ----------------------------------------------------------------------------- 6: kernel against torch
SIZES = (4, 768, 1_200_004, 12_296, 64, 300_000, 1_536, 12)        # 8 ranges: one of 4 elements, one above 1 M
DECAYED = (True, False, True, True, False, True, False, False)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_ranges_kernel_matches_torch_param_groups(dev, mode):
    o = ops()
    spans, n = make_ranges(SIZES)
    g = torch.Generator().manual_seed(40 + mode)
    scales = [0.01 + 0.99 * float(torch.rand(1, generator=g)) for _ in SIZES]
    assert all(0.01 < s <= 1.0 for s in scales) and len(SIZES) >= 7 and min(SIZES) == 4 and max(SIZES) > 1_000_000
    lr, wd, mom = (1e-2 if mode == 2 else 1e-3), 0.04, 0.99
    p0, t0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (1.0 + 0.5 * s) for s in range(3)]          # a new gradient every step

    def reference(sc):
        ps = [p0[lo:hi].clone().requires_grad_(True) for lo, hi in spans]
        groups = [dict(params=[q], lr=lr * s, weight_decay=wd if d else 0.0) for q, s, d in zip(ps, sc, DECAYED)]
        opt = (torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8) if mode == 0 else
               torch.optim.Adam(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8) if mode == 1 else
               torch.optim.SGD(groups, lr=lr, momentum=0.9, nesterov=True))
        tref = t0.clone()
        for gr in grads:
            for q, (lo, hi) in zip(ps, spans):
                q.grad = gr[lo:hi].clone()
            opt.step()
            tref = mom * tref + (1.0 - mom) * torch.cat([q.detach() for q in ps])
        return torch.cat([q.detach() for q in ps]), tref

    p_ref, t_ref = reference(scales)
    p = p0.to(dev); m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); t = t0.to(dev)
    pb = torch.empty(n, dtype=o.bf16, device=dev); tb = torch.empty(n, dtype=o.bf16, device=dev)
    blocks = o.range_block_table(spans).to(dev)
    rows = torch.tensor([(s, 1.0 if d else 0.0) for s, d in zip(scales, DECAYED)], dtype=f32).to(dev)
    for step, gr in enumerate(grads, 1):
        o.adamw_ema_ranges(p, gr.to(dev), m, v, pb, t, tb, n, blocks, rows, lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd,
                           step=step, teacher_momentum=mom, mode=mode)
    torch.cuda.synchronize()
    close(p, p_ref, 1e-5, 1e-6, f"mode {mode} p")
    close(t, t_ref, 1e-5, 1e-6, f"mode {mode} ema")
    assert torch.equal(pb, p.to(o.bf16)) and torch.equal(tb, t.to(o.bf16))
    # the tolerance tells a per-range rate from one rate for all: the same reference with every scale forced to 1 must NOT pass
    p_one, t_one = reference([1.0] * len(SIZES))
    nbad, _, mx = err_report(p, p_one, 1e-5, 1e-6)
    print(f"[layer-decay] mode {mode} against scales == 1: {nbad} off, max err {mx:.4g}")
    assert nbad > 0 and err_report(t, t_one, 1e-5, 1e-6)[0] > 0


# ----------------------------------------------------------------------------- 7: kernel against the existing kernel, bit for bit
@pytest.mark.parametrize("variant", ["plain", "clip_norm", "clip_value", "hyper", "loss_scale"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_ranges_kernel_equals_two_range_launches_bitwise(dev, variant, mode):
    """Every scale 1, the decay flags of the two-range layout (decayed ranges first): p, m, v, the EMA copy and both 16-bit copies
    after three steps equal what two gv_adamw_ema calls leave -- both kernels run one device function."""
    o = ops()
    sizes, n_dec = (4, 70_000, 1_200_004, 768, 2_048, 12), 3
    spans, n = make_ranges(sizes)
    cut = spans[n_dec][0]
    g = torch.Generator().manual_seed(7)
    p0, t0 = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    grads = [(torch.randn(n, generator=g) * (1.0 + s)).to(dev) for s in range(3)]
    blocks = o.range_block_table(spans).to(dev)
    rows = torch.tensor([(1.0, 1.0 if i < n_dec else 0.0) for i in range(len(sizes))], dtype=f32).to(dev)
    lr, wd, mom = 1e-3, 0.05, 0.9
    ws = torch.empty(1024, device=dev)

    def run(ranged: bool):
        p, m, v, t = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), t0.clone()
        pb, tb = torch.zeros(n, dtype=o.bf16, device=dev), torch.zeros(n, dtype=o.bf16, device=dev)
        gn = torch.zeros(1, device=dev)
        scaler = o.LossScaler(dev, init_scale=8.0) if variant == "loss_scale" else None
        hyper = torch.zeros(8, device=dev) if variant == "hyper" else None
        skipped = None
        for step, gr in enumerate(grads, 1):
            kw = dict(lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, step=step, teacher_momentum=mom, mode=mode)
            if variant == "clip_norm":
                o.sumsq(gr, ws.fill_(float("nan")), gn); kw.update(clip_norm=5.0, gnorm_sq=gn)
            if variant == "clip_value":
                kw.update(clip_value=0.7, grad_scale=0.5)
            if variant == "hyper":
                o.store_f32(hyper, [lr * step, wd, 1.0 - 0.9 ** step, 1.0 - 0.999 ** step, mom, 0.25, 0.0, 0.0])
                kw.update(hyper=hyper, lr=0.0)
            if variant == "loss_scale":
                o.sumsq(gr, ws.fill_(float("nan")), gn)
                if step == 2:
                    gn.fill_(float("inf"))
                kw.update(loss_scale=scaler.scale, gnorm_sq=gn)
                before = (p.clone(), m.clone(), v.clone(), t.clone())
            wds = (1.0, 0.0) if variant == "hyper" else (wd, 0.0)           # with hyper the by-value decay is a 0 / 1 multiplier
            if ranged:
                o.adamw_ema_ranges(p, gr, m, v, pb, t, tb, n, blocks, rows, weight_decay=wds[0], **kw)
            else:
                for (lo, hi), w in zip(((0, cut), (cut, n)), wds):
                    sl = slice(lo, hi)
                    o.adamw_ema(p[sl], gr[sl], m[sl], v[sl], pb[sl], t[sl], tb[sl], hi - lo, weight_decay=w, **kw)
            if scaler is not None:
                scaler.update(gn)
                if step == 2:           # the skipped step: p, m, v untouched in every range, the EMA copy still moves
                    skipped = all(torch.equal(a, b) for a, b in zip(before[:3], (p, m, v))) and not torch.equal(before[3], t)
        torch.cuda.synchronize()
        return (p, m, v, t, pb, tb), skipped, (None if scaler is None else scaler.state.tolist())

    got, skipped, st = run(True)
    ref, skipped_ref, st_ref = run(False)
    for name, a, b in zip(("p", "m", "v", "ema", "p 16-bit", "ema 16-bit"), got, ref):
        assert torch.equal(a, b), f"{variant} mode {mode}: {name} differs in {int((a != b).sum())} of {a.numel()} elements"
    assert not torch.equal(got[0], p0) and bool(torch.isfinite(got[0]).all())
    if variant == "loss_scale":
        assert skipped is True and skipped_ref is True and st == st_ref and st[2] == 1.0 and st[3] == 2.0


# ----------------------------------------------------------------------------- 8: LAMB
def test_lamb_per_tensor_rates_match_oracle(dev):
    """The update is linear in the rate and neither the moments, the clips nor the trust ratio depend on it: the reference for tensor k
    is p_before + scale_k * (p_after_oracle_step - p_before), written back into the oracle's parameters before the next step."""
    from oracle import vit_oracle as vo
    o = ops()
    g = torch.Generator().manual_seed(21)
    shapes = {"blocks.0.mlp.fc1.weight": (96, 64), "blocks.0.attn.qkv.weight": (40, 64), "blocks.0.mlp.fc1.bias": (96,)}     # two decayed, one not
    scale = {"blocks.0.mlp.fc1.weight": 1.0, "blocks.0.attn.qkv.weight": 0.3, "blocks.0.mlp.fc1.bias": 0.05}
    params = {k: torch.randn(*sh, generator=g) * 0.3 for k, sh in shapes.items()}
    orc = vo.Lamb({k: v.clone() for k, v in params.items()}, lr=2e-3, wd=0.05)
    spans, off = [], 0
    for k, sh in shapes.items():
        n = (math.prod(sh) + 63) // 64 * 64
        spans.append((off, off + n)); off += n
    flat = lambda d: torch.cat([torch.nn.functional.pad(d[k].reshape(-1), (0, (sp[1] - sp[0]) - d[k].numel())) for k, sp in zip(shapes, spans)])
    P = flat(params).to(dev); M, V, T = torch.zeros_like(P), torch.zeros_like(P), P.clone()
    Pb, Tb = torch.zeros(off, dtype=o.bf16, device=dev), torch.zeros(off, dtype=o.bf16, device=dev)
    P1, M1, V1, T1, Pb1, Tb1 = (x.clone() for x in (P, M, V, T, Pb, Tb))          # lr_scale = NULL
    P2, M2, V2, T2, Pb2, Tb2 = (x.clone() for x in (P, M, V, T, Pb, Tb))          # lr_scale = ones
    tab = o.lamb_block_table(spans, chunk=2048).to(dev)
    tabs = (tab[tab[:, 0] < 2].contiguous(), tab[tab[:, 0] >= 2].contiguous())
    stats, gsq, ws = torch.zeros(6, device=dev), torch.zeros(1, device=dev), torch.empty(1024, device=dev)
    rates = torch.tensor([scale[k] for k in shapes], dtype=f32).to(dev)
    ones = torch.ones(3, dtype=f32, device=dev)
    t_ref = {k: v.clone() for k, v in params.items()}
    kw = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-6, teacher_momentum=0.99)
    for step in range(1, 4):
        grads = {k: torch.randn(*sh, generator=g) * (3.0 if step == 1 else 0.05) for k, sh in shapes.items()}      # step 1 triggers the global clip
        before = {k: v.clone() for k, v in orc.p.items()}
        orc.step(grads)
        for k in orc.p:
            orc.p[k].copy_(before[k] + scale[k] * (orc.p[k] - before[k]))
            t_ref[k] = 0.99 * t_ref[k] + 0.01 * orc.p[k]
        G = flat(grads).to(dev)
        o.sumsq(G, ws.fill_(float("nan")), gsq)          # the scratch as a kernel must expect it: NaN, not fresh zero pages
        for bufs, ls in (((P, M, V, Pb, T, Tb), rates), ((P1, M1, V1, Pb1, T1, Tb1), None), ((P2, M2, V2, Pb2, T2, Tb2), ones)):
            stats.zero_()
            for phase in (0, 1):
                for tb, wd in zip(tabs, (0.05, 0.0)):
                    o.lamb(bufs[0], G, bufs[1], bufs[2], bufs[3], bufs[4], bufs[5], tb, stats, gsq, phase=phase, weight_decay=wd, step=step,
                           lr_scale=ls, **kw)
    torch.cuda.synchronize()
    for (k, sh), (lo, hi) in zip(shapes.items(), spans):
        n = math.prod(sh)
        close(P[lo:lo + n].view(sh), orc.p[k], 1e-5, 1e-6, f"lamb p {k}")
        close(T[lo:lo + n].view(sh), t_ref[k], 1e-5, 1e-6, f"lamb ema {k}")
        close(Pb[lo:lo + n].view(sh), orc.p[k], 1e-2, 1e-2, f"lamb 16-bit {k}")
        close(M[lo:lo + n].view(sh), orc.m[k], 1e-5, 1e-7, f"lamb m {k}")
    # the field left NULL is today's call; a table of ones computes lr * 1
    for a, b in zip((P1, M1, V1, T1, Pb1, Tb1), (P2, M2, V2, T2, Pb2, Tb2)):
        assert torch.equal(a, b)
    assert not torch.equal(P, P1)


# ----------------------------------------------------------------------------- 9: engine
# timm's layer map for a depth-12 ViT, written out here (NOT the engine's function): VisionTransformer.group_matcher + group_parameters
STEM, BLOCK, NORM = re.compile(r"^cls_token|pos_embed|patch_embed"), re.compile(r"^blocks\.(\d+)"), re.compile(r"^norm")


def timm_layer_id(name, depth=12):
    if STEM.match(name):
        return 0
    if BLOCK.match(name):
        return int(BLOCK.match(name).group(1)) + 1
    return depth + 1 if NORM.match(name) else depth + 2


def timm_scale(name, decay, depth=12):
    return decay ** (depth + 3 - 1 - timm_layer_id(name, depth))


def timm_no_decay(name, shape):
    return len(shape) <= 1 or name.endswith(".bias") or name in ("pos_embed", "cls_token")


@pytest.mark.parametrize("opt,train_backbone", [("adamw", True), ("sgd", True), ("lamb", True), ("adamw", False)])
def test_engine_layer_decay_matches_cpu_optimizer(dev, opt, train_backbone):
    from gipvit.engine import SupervisedEngine
    from oracle import vit_oracle as vo
    lr, wd, decay = 1e-3, 0.05, 0.75
    eng = SupervisedEngine("vit_tiny", 64, 2, batch=8, precision="fp32", layer_decay=decay, lr=lr, weight_decay=wd, opt=opt,
                           eps=1e-6 if opt == "lamb" else 1e-8, train_backbone=train_backbone, device=dev)
    state = vo.init_vit("vit_tiny", 64, 2, seed=0)
    eng.load_state(state)
    names = list(state) if train_backbone else ["head.weight", "head.bias"]
    assert timm_scale("head.bias", decay) == 1.0 and abs(timm_scale("pos_embed", decay) - 0.017817948) < 1e-9
    assert eng.layer_scales == pytest.approx({n: timm_scale(n, decay) for n in names}, rel=1e-12)
    groups_seen = {(timm_layer_id(n), timm_no_decay(n, state[n].shape)) for n in names}
    assert eng.mean_lr(lr) == pytest.approx(sum(lr * decay ** (14 - lay) for lay, _ in groups_seen) / len(groups_seen), rel=1e-12)
    cpu = {n: state[n].clone().float().requires_grad_(True) for n in names}
    if opt == "lamb":
        ref = vo.Lamb({n: q.detach() for n, q in cpu.items()}, lr=lr, wd=wd)
    else:
        groups = [dict(params=[q], lr=lr * timm_scale(n, decay), weight_decay=0.0 if timm_no_decay(n, q.shape) else wd) for n, q in cpu.items()]
        ref = torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8) if opt == "adamw" else torch.optim.SGD(groups, lr=lr, momentum=0.9, nesterov=True)
    for step in range(3):
        tiles = vo.synth_tiles(8, 64, seed=100 + step).to(dev)
        tgt = torch.randint(0, 2, (8, 1), generator=torch.Generator().manual_seed(step)).to(dev)
        eng.forward_backward(tiles, tgt)
        grads = {n: gr.cpu() for n, gr in eng.grads().items()}
        eng.optimizer_step()
        if opt == "lamb":
            before = {n: q.clone() for n, q in ref.p.items()}
            ref.step({n: grads[n] for n in names})
            for n in names:
                ref.p[n].copy_(before[n] + timm_scale(n, decay) * (ref.p[n] - before[n]))
        else:
            for n in names:
                cpu[n].grad = grads[n].clone()
            ref.step()
        got = eng.state_dict()
        worst = 0.0
        for n in state:
            if n in cpu:
                want = ref.p[n] if opt == "lamb" else cpu[n].detach()
                nbad, tot, mx = err_report(got[n], want, 1e-5, 1e-6)
                worst = max(worst, mx)
                assert nbad == 0, f"{opt} step {step} {n}: {nbad}/{tot} off, max err {mx:.4g}"
            else:
                assert torch.equal(got[n].cpu(), state[n].float()), f"{n} is frozen and moved"
        print(f"[layer-decay] engine {opt} backbone={train_backbone} step {step}: max err {worst:.4g}")
    assert not torch.equal(got["head.weight"].cpu(), state["head.weight"].float())
    if train_backbone:
        assert not torch.equal(got["pos_embed"].cpu(), state["pos_embed"].float())


# ----------------------------------------------------------------------------- 10: driver
def test_driver_layer_decay_log_rate_and_resume(dev, tmp_path, caplog):
    sys.path.insert(0, ROOT)
    import train
    base = ["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "--num-classes", "2", "--img-size", "64", "--tile-size", "64",
            "-b", "8", "--batches-per-epoch", "6", "--opt", "adamw", "--lr", "0.001", "--sched", "cosine", "--warmup-epochs", "1",
            "--warmup-lr", "1e-5", "--min-lr", "0", "--log-interval", "2", "--output", str(tmp_path), "--subexperiment", "sub", "--seed", "1",
            "--synthetic-slides", "4", "--num_tiles", "12", "--tiles_per_iter", "5"]
    # cosine over E epochs stepped per epoch, one warm-up epoch from 1e-5: epoch 0 -> 1e-5, epoch e >= 1 -> 0.5 * lr * (1 + cos(pi e / E))
    sched = lambda e, E: 1e-5 if e == 0 else 0.5 * 1e-3 * (1.0 + math.cos(math.pi * e / E))
    mean_scale = sum(0.75 ** (14 - lay) for lay in range(15) for dec in (0, 1) if (lay, dec) != (13, 1)) / 29       # norm holds no decayed tensor

    def logged(messages):
        out = {}
        for msg in messages:
            mt = re.match(r"Train: (\d+) \[.*LR: (\S+)", msg)
            if mt:
                out.setdefault(int(mt.group(1)), set()).add(mt.group(2))
        return out

    with caplog.at_level("INFO"):
        assert train.main(base + ["--experiment", "ld", "--epochs", "2", "--layer-decay", "0.75"]) == 0
    lrs = logged(caplog.messages)
    assert lrs == {e: {"{:.3e}".format(sched(e, 2) * mean_scale)} for e in (0, 1)}, lrs
    rows = list(csv.DictReader(open(tmp_path / "ld" / "sub" / "summary.csv")))
    assert [int(r["epoch"]) for r in rows] == [0, 1]
    for r in rows:
        assert float(r["lr"]) == pytest.approx(sched(int(r["epoch"]), 2) * mean_scale, rel=1e-9)
        assert 0.3 < float(r["train_loss"]) < 1.2
    # a resumed run continues (the moments are per element, the decay rides in the arguments)
    caplog.clear()
    with caplog.at_level("INFO"):
        assert train.main(base + ["--experiment", "ld", "--epochs", "3", "--layer-decay", "0.75", "--resume", str(tmp_path / "ld" / "sub" / "last.pth.tar")]) == 0
    assert logged(caplog.messages) == {2: {"{:.3e}".format(sched(2, 3) * mean_scale)}}
    rows = list(csv.DictReader(open(tmp_path / "ld" / "sub" / "summary.csv")))
    assert [int(r["epoch"]) for r in rows] == [0, 1, 2] and float(rows[2]["lr"]) == pytest.approx(sched(2, 3) * mean_scale, rel=1e-9)
    ck = torch.load(tmp_path / "ld" / "sub" / "last.pth.tar", weights_only=True)
    assert ck["optimizer"]["step"] == 18
    # without the flag: the plain scheduled rate, as before
    caplog.clear()
    with caplog.at_level("INFO"):
        assert train.main(base + ["--experiment", "plain", "--epochs", "2"]) == 0
    assert logged(caplog.messages) == {e: {"{:.3e}".format(sched(e, 2))} for e in (0, 1)}
    rows = list(csv.DictReader(open(tmp_path / "plain" / "sub" / "summary.csv")))
    assert [float(r["lr"]) for r in rows] == [sched(0, 2), sched(1, 2)]
