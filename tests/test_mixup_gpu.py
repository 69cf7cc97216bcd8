"""Supervised mixup / cutmix on the device: gv_patchify_mix / gv_patchify_nchw_mix bit-exact against torch, gv_softmax_mix_loss
against timm's losses restated under autograd, the supervised step with a plan against the oracle's model, and the driver.
The restatements and the per-build kernel checks live in tests/mixup_worker.py (also run there on the float16 build)."""
import csv
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixup_worker as mw      # noqa: E402

pytestmark = pytest.mark.gpu
NINE = ("--mixup", "--cutmix", "--cutmix-minmax", "--mixup-prob", "--mixup-switch-prob", "--mixup-mode", "--mixup-off-epoch",
        "--bce-loss", "--bce-target-thresh")


def test_patchify_mix_u8_exact(dev):
    mw.check_patchify_mix_u8(dev)


def test_patchify_mix_nchw_exact(dev):
    mw.check_patchify_mix_nchw(dev)


def test_patchify_mix_copy_rows_equal_unmixed_kernel(dev):
    """An all-copy table: every row bit-identical to gv_patchify / gv_patchify_nchw, with partners that are never read."""
    from gipvit import ops
    from gipvit.mixup import MixPlan
    from oracle import vit_oracle as vo
    B = 8
    t = vo.synth_tiles(B, 64, seed=3).to(dev)
    rows = MixPlan.make_rows(B)
    rows["partner"][0] = 1 << 30          # out of range: such a row is a copy row
    rows["mode"][1] = 7                   # unknown mode: a copy row
    tab = MixPlan(rows, dev).table
    assert torch.equal(ops.patchify(t, [(0, 0)], 64, vo.MEAN_RON, vo.STD_RON, mix=tab).view(torch.int16),
                       ops.patchify(t, [(0, 0)], 64, vo.MEAN_RON, vo.STD_RON).view(torch.int16))
    x = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    assert torch.equal(ops.patchify_nchw(x, [(0, 0)], 64, mix=tab).view(torch.int16), ops.patchify_nchw(x, [(0, 0)], 64).view(torch.int16))
    with pytest.raises(ValueError, match="one crop window"):
        ops.patchify_nchw(x, [(0, 0), (0, 0)], 32, mix=tab)


def test_softmax_mix_loss(dev):
    mw.check_mix_loss(dev)


def test_softmax_mix_loss_lam1_is_lsce_and_loss_scale(dev):
    """soft_ce with lam = 1 against gv_softmax_lsce itself at test_softmax_lsce's gates; loss_scale multiplies dlogits only."""
    from gipvit import ops
    for B, C in ((8, 2), (300, 5), (64, 64)):
        g = torch.Generator().manual_seed(B + 1)
        z = torch.randn(B, C, generator=g).to(dev); tgt = torch.randint(0, C, (B,), generator=g).to(dev)
        new = lambda: (torch.empty(1, device=dev), torch.empty(B, C, device=dev), torch.empty(B, C, device=dev))
        l0, d0, p0 = new(); l1, d1, p1 = new(); l2, d2, p2 = new()
        ops.softmax_lsce(z, tgt, l0, d0, p0, B, C, 0.1)
        partner = (B - 1 - torch.arange(B)).to(torch.int32).to(dev)
        ops.softmax_mix_loss(z, tgt, l1, d1, p1, B, C, 0.1, "soft_ce", partner=partner, lam=torch.ones(B, device=dev))
        assert abs(float(l1) - float(l0)) < 1e-5
        assert torch.allclose(d1, d0, rtol=1e-4, atol=1e-6) and torch.allclose(p1, p0, rtol=1e-5, atol=1e-6)
        scale = torch.tensor([1024.0, 0.0, 0.0, 0.0], device=dev)
        for kind in ("soft_ce", "bce"):
            lam = torch.rand(B, generator=g).to(dev)
            ops.softmax_mix_loss(z, tgt, l1, d1, p1, B, C, 0.1, kind, partner=partner, lam=lam)
            ops.softmax_mix_loss(z, tgt, l2, d2, p2, B, C, 0.1, kind, partner=partner, lam=lam, loss_scale=scale)
            assert float(l2) == float(l1) and torch.equal(p1, p2)
            assert torch.allclose(d2, d1 * 1024.0, rtol=1e-6, atol=0.0)


def test_mixup_float16_build(dev):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mixup_worker.py"), "f16"], cwd=ROOT, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, GIPVIT_ACT_FORMAT="f16"))
    assert r.returncode == 0 and r.stdout.strip().endswith("MIXUP F16 OK"), (r.stdout[-2000:], r.stderr[-3000:])


# ------------------------------------------------------------------ the step
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _check_grads(got, ref, tol=5e-2):
    """The parity gates of tests/test_nchw_input_gpu.py: per-parameter relative error and the global gradient norm."""
    worst, gn_g, gn_r = [], 0.0, 0.0
    for k, r in ref.items():
        if r is None:
            continue
        g = got[k]
        gn_g += float((g.double() ** 2).sum()); gn_r += float((r.double() ** 2).sum())
        if float(r.abs().max()) >= 1e-12:
            worst.append((_rel(g, r), k))
    worst.sort(reverse=True)
    rel_norm = abs(math.sqrt(gn_g) - math.sqrt(gn_r)) / math.sqrt(gn_r)
    print(f"[grads] worst {worst[0]}, grad-norm rel err {rel_norm:.2e}")
    assert worst[0][0] <= tol, f"gradient mismatch: {worst[:8]}"
    assert rel_norm <= 1e-2, f"grad-norm rel err {rel_norm}"


def _step_plan(B=8, S=64):
    """Copy, blend and paste rows in one plan."""
    from gipvit.mixup import MixPlan
    rows = MixPlan.make_rows(B)
    MixPlan.set_row(rows, 0, 0.3, None); MixPlan.set_row(rows, B - 1, 0.3, None)
    MixPlan.set_row(rows, 1, 1.0 - (30 * 22) / float(S * S), (7, 37, 9, 31)); MixPlan.set_row(rows, B - 2, 1.0 - (30 * 22) / float(S * S), (7, 37, 9, 31))
    MixPlan.set_row(rows, 2, 0.85, None)
    assert set(rows["mode"].tolist()) == {0, 1, 2}
    return rows


def _oracle_step(orc, x, tgt, rows, kind, thr):
    from oracle import vit_oracle as vo
    sp = {k: v.detach().clone().requires_grad_(True) for k, v in orc.p.items()}
    logits = vo.vit_logits(sp, mw.mix_images(x, rows), orc.arch)
    dense = mw.mixup_target(tgt, logits.shape[1], torch.from_numpy(rows["lam"].copy()), torch.from_numpy(rows["partner"].copy()), orc.smoothing)
    loss = mw.mix_loss(logits, dense, kind, thr)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in sp.items()}, logits.detach()


@pytest.mark.parametrize("kind,thr", [("soft_ce", None), ("bce", 0.2)])
def test_supervised_step_with_plan_against_oracle(dev, kind, thr):
    """ViT-T, img 64, B = 8: the oracle mixes normalize_window(tiles) with the restated Mixup; gates of tests/test_nchw_input_gpu.py."""
    from gipvit.engine import SupervisedEngine
    from gipvit.mixup import MixPlan
    from oracle import step_oracle as so, vit_oracle as vo
    orc = so.SupervisedOracle(arch="vit_tiny", img_size=64, num_classes=2, seed=0, lr=1e-3, wd=0.05)
    tiles = vo.synth_tiles(8, 64, seed=1234)
    x = vo.normalize_window(tiles, (0, 0, 64))
    tgt = torch.tensor([0, 1, 1, 0, 1, 0, 0, 0]).view(8, 1)               # partners with the other label and with the same
    rows = _step_plan()
    plan = MixPlan(rows, dev)
    loss_r, grads_r, logits_r = _oracle_step(orc, x, tgt, rows, kind, thr)
    scale = float(logits_r.abs().max())
    for form, src in (("u8", tiles.to(dev)), ("f32", x.to(dev))):
        eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, lr=1e-3, weight_decay=0.05, device=dev, loss=kind,
                               bce_target_thresh=thr)
        eng.load_state(orc.p)
        eng.forward_backward(src, tgt.to(dev), mix=plan)
        torch.cuda.synchronize()
        dl, dloss = float((eng.logits.cpu() - logits_r).abs().max()), abs(float(eng.loss) - float(loss_r))
        print(f"[{kind} {form}] logits max-abs err {dl:.2e} (scale {scale:.2f}), loss {float(eng.loss):.5f} ref {float(loss_r):.5f}")
        assert dl <= 2e-2 * max(scale, 1.0) and dloss <= 1e-3
        _check_grads(eng.grads(), grads_r)
        assert math.isfinite(float(eng.step(src, tgt.to(dev), mix=plan)))
        e32 = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, lr=1e-3, weight_decay=0.05, device=dev, precision="fp32",
                               loss=kind, bce_target_thresh=thr)
        e32.load_state(orc.p)
        e32.forward_backward(src, tgt.to(dev), mix=plan)
        torch.cuda.synchronize()
        dl, dloss = float((e32.logits.cpu() - logits_r).abs().max()), abs(float(e32.loss) - float(loss_r))
        print(f"[{kind} {form} fp32] logits max-abs err {dl:.2e}, loss err {dloss:.2e}")
        assert dl <= 1e-4 and dloss <= 1e-4
        _check_grads(e32.grads(), grads_r, tol=1e-3)


def test_all_copy_plan_reproduces_the_unmixed_step(dev):
    """soft_ce on an all-copy plan = the mix=None, lsce step: logits bit-identical, loss within test_softmax_lsce's 1e-5;
    lsce refuses a plan; bce runs without one."""
    from gipvit.engine import SupervisedEngine
    from gipvit.mixup import MixPlan
    from oracle import step_oracle as so, vit_oracle as vo
    orc = so.SupervisedOracle(arch="vit_tiny", img_size=64, num_classes=2, seed=0)
    tiles = vo.synth_tiles(8, 64, seed=99).to(dev)
    tgt = torch.randint(0, 2, (8, 1), generator=torch.Generator().manual_seed(5)).to(dev)
    plan = MixPlan(MixPlan.make_rows(8), dev)
    out = {}
    for name, kw, mix in (("lsce", {}, None), ("soft_ce", {"loss": "soft_ce"}, plan), ("soft_ce none", {"loss": "soft_ce"}, None)):
        eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, device=dev, **kw)
        eng.load_state(orc.p)
        eng.forward_backward(tiles, tgt, mix=mix)
        torch.cuda.synchronize()
        out[name] = (eng.logits.clone(), float(eng.loss), eng.grads())
    for name in ("soft_ce", "soft_ce none"):
        assert torch.equal(out[name][0], out["lsce"][0]) and abs(out[name][1] - out["lsce"][1]) <= 1e-5, name
        assert _rel(out[name][2]["head.weight"], out["lsce"][2]["head.weight"]) < 1e-4
    eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, device=dev)
    with pytest.raises(ValueError, match="soft_ce"):
        eng.forward_backward(tiles, tgt, mix=plan)
    bce = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, device=dev, loss="bce")
    bce.load_state(orc.p)
    assert math.isfinite(float(bce.step(tiles, tgt)))
    with pytest.raises(ValueError, match="fill="):
        eng2 = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, device=dev, loss="soft_ce")
        eng2.forward_backward(torch.randn(8, 3, 64, 64, device=dev), tgt, fill=torch.zeros(8, 8, device=dev), mix=plan)


# ------------------------------------------------------------------ the driver
def test_train_mixup_through_the_driver(dev, tmp_path, caplog, monkeypatch):
    sys.path.insert(0, ROOT)
    import train
    from gipvit.engine import SupervisedEngine
    from gipvit.mixup import MixSampler

    def common(exp):          # the argument list of test_train_supervised_and_resume
        return ["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "--num-classes", "2", "--img-size", "64", "--tile-size", "64",
                "-b", "8", "--batches-per-epoch", "6", "--opt", "adam", "--lr-base", "0.001", "--sched", "cosine", "--warmup-epochs", "1",
                "--log-interval", "2", "--output", str(tmp_path), "--experiment", exp, "--subexperiment", "sub", "--seed", "1",
                "--synthetic-slides", "4", "--num_tiles", "12", "--tiles_per_iter", "5", "--model-ema", "--model-ema-decay", "0.9"]
    mixf = ["--mixup", "0.8", "--cutmix", "1.0"]
    seen = []
    orig = SupervisedEngine.step
    monkeypatch.setattr(SupervisedEngine, "step", lambda self, *a, **k: (seen.append(k.get("mix")), orig(self, *a, **k))[1])
    with caplog.at_level("INFO"):
        assert train.main(common("plain") + ["--epochs", "2"]) == 0
        assert all(m is None for m in seen) and len(seen) == 12
        del seen[:]
        assert train.main(common("mix") + mixf + ["--epochs", "2"]) == 0
    assert len(seen) == 12 and all(m is not None for m in seen)
    rows = {e: list(csv.DictReader(open(tmp_path / e / "sub" / "summary.csv"))) for e in ("plain", "mix")}
    assert all(np.isfinite(float(r["train_loss"])) and np.isfinite(float(r["eval_loss"])) for r in rows["mix"]) and len(rows["mix"]) == 2
    assert float(rows["mix"][0]["train_loss"]) != float(rows["plain"][0]["train_loss"])
    for m in caplog.messages:
        if "accepted for CLI compatibility" in m:
            assert not any(f in m.split() for f in NINE), m
    # the mix stream rides in the checkpoint: a sampler restored from it draws what one that was never interrupted draws next
    ck = torch.load(tmp_path / "mix" / "sub" / "last.pth.tar", weights_only=True)
    assert "mix" in ck["host_rng"]
    args, _ = train.parse_args(common("mix") + mixf)
    whole = train.build_mix_sampler(args, 64, 0)
    for _ in range(12):
        whole.sample_host()
    restored = MixSampler(0.8, 1.0, None, 1.0, 0.5, "batch", 8, 64, seed=12345)
    restored.load_state_dict({"rng": ck["host_rng"]["mix"]})
    for _ in range(3):
        assert np.array_equal(restored.sample_host(), whole.sample_host())
    del seen[:]
    assert train.main(common("mix") + mixf + ["--epochs", "3", "--resume", str(tmp_path / "mix" / "sub" / "last.pth.tar")]) == 0
    assert len(seen) == 6
    whole2 = train.build_mix_sampler(args, 64, 0)
    for _ in range(12):
        whole2.sample_host()
    assert np.array_equal(seen[0].rows, whole2.sample_host())              # the resumed run went on from the saved stream
    assert [int(r["epoch"]) for r in csv.DictReader(open(tmp_path / "mix" / "sub" / "summary.csv"))] == [0, 1, 2]
    # --mixup-off-epoch 1: plans in epoch 0, none from epoch 1 on
    del seen[:]
    assert train.main(common("off") + mixf + ["--epochs", "2", "--mixup-off-epoch", "1"]) == 0
    assert [m is None for m in seen] == [False] * 6 + [True] * 6
    # --bce-loss alone (no mixing): timm's one-hot-with-smoothing branch
    del seen[:]
    assert train.main(common("bce") + ["--epochs", "1", "--bce-loss"]) == 0
    assert all(m is None for m in seen)
    r = list(csv.DictReader(open(tmp_path / "bce" / "sub" / "summary.csv")))
    assert len(r) == 1 and np.isfinite(float(r[0]["train_loss"]))
    assert float(r[0]["train_loss"]) != float(rows["plain"][0]["train_loss"])
