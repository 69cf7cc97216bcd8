"""GPU: gv_linprobe_train / gv_linprobe_predict against the f64 torch.optim.SGD reference of tests/test_linprobe_host.py, one exact
step written out by hand, bitwise reproducibility (run to run, NaN row padding, repeated row indices), probe_features against
intermediate_layers, LinearProbe on a real encoder against the same procedure through the host reference, and the driver.

Measured on an MI355X, maxima over the six cases against the f64 reference (the bounds are 2e-6 on the state and on
probabilities, 4e-6 on mean losses): training W 1.1e-7, b 3.5e-8, mW 2.7e-7, mb 1.3e-7, epoch loss 2.2e-7; predict probabilities
1.3e-6 (the 3840-feature case, whose two fastest heads have diverged to logits of several hundred; 3.4e-7 on the other five),
mean loss 2.7e-7.  Every test prints its figures; DESIGN.md section 4 records these."""
import csv
import math
import os
import sys

import numpy as np
import pytest
import torch

from test_linprobe_host import (CASES, CASE_IDS, MU, case_reference, cosine_scale, probe_predict_reference, probe_reference, s_args)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
f32 = torch.float32
STATE_BOUND, LOSS_BOUND = 2e-6, 4e-6


def _poison_workspace(dev, M, H, C, F):
    """The scratch ops.linprobe_* keep per device, all-ones bit patterns (NaN) for the next call: a slot the first launch never
    wrote would show as a NaN in the result."""
    from gipvit import ops
    ops._scratch("linprobe", dev, M, H, C, F).fill_(255)                    # (grown if need be)


def _train_gpu(dev, s, x_dev=None, perms=None):
    """The epochs of a case on the device -> (W, b, mW, mb, epoch_loss [epochs, H] = loss_sum / rows), host tensors."""
    from gipvit import ops
    H, C, F = s["W0"].shape
    perms = s["perms"] if perms is None else perms
    x = s["x"].to(dev) if x_dev is None else x_dev
    W, b = s["W0"].to(dev), s["b0"].to(dev)
    mW, mb = torch.zeros_like(W), torch.zeros_like(b)
    lr, wd = torch.tensor(s["lr"], dtype=f32, device=dev), torch.tensor(s["wd"], dtype=f32, device=dev)
    y = s["labels"].to(dev, torch.int32)
    rows = torch.from_numpy(np.asarray(perms).astype(np.int32)).to(dev)
    epochs = rows.shape[0]
    loss = torch.zeros(epochs, H, dtype=f32, device=dev)
    _poison_workspace(dev, s["M"], H, C, F)
    for e in range(epochs):
        ops.linprobe_train(W, b, mW, mb, lr, wd, x, y, rows[e], loss[e], s["M"], cosine_scale(e, epochs), MU)
    torch.cuda.synchronize()
    return W.cpu(), b.cpu(), mW.cpu(), mb.cpu(), loss.cpu() / rows.shape[1]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_train_matches_the_f64_reference(dev, case):
    """W, b and the momentum buffers after all epochs within 2e-6 of torch.optim.SGD in f64, every epoch's loss_sum / N within 4e-6."""
    s, ref = case_reference(case)
    got = _train_gpu(dev, s)
    errs = [float((g.double() - r).abs().max()) for g, r in zip(got, ref)]
    print("max |gpu - f64|: W %.3e  b %.3e  mW %.3e  mb %.3e  epoch loss %.3e" % tuple(errs))
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert max(errs[:4]) <= STATE_BOUND and errs[4] <= LOSS_BOUND


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_predict_matches_the_f64_reference(dev, case):
    """Probabilities of the reference's trained heads (as f32) within 2e-6 of their f64 softmax, the mean loss within 4e-6."""
    from gipvit import ops
    s, ref = case_reference(case)
    W, b = ref[0].to(f32), ref[1].to(f32)
    H, C, F = W.shape
    want = probe_predict_reference(W, b, s["x"])
    _poison_workspace(dev, min(len(s["x"]), 4096), H, C, F)
    prob, loss = ops.linprobe_predict(W.to(dev), b.to(dev), s["x"].to(dev), s["labels"].to(dev, torch.int32))
    only = ops.linprobe_predict(W.to(dev), b.to(dev), s["x"].to(dev))              # no labels: probabilities alone
    torch.cuda.synchronize()
    assert prob.shape == (len(s["x"]), H, C) and loss.shape == (H,) and torch.equal(_bits(only), _bits(prob))
    want_loss = -torch.log(want[torch.arange(len(s["x"])), :, s["labels"]]).mean(0)
    ep, el = float((prob.cpu().double() - want).abs().max()), float((loss.cpu().double() / len(s["x"]) - want_loss).abs().max())
    print(f"max |prob - f64| {ep:.3e}, max |mean loss - f64| {el:.3e}")
    assert ep <= STATE_BOUND and el <= LOSS_BOUND


def test_predict_in_chunks_and_out_of_range_labels(dev):
    """More rows than one chunk of 4096: the loss is summed over the chunks; a label outside [0, C) adds nothing and is no index."""
    from gipvit import ops
    Q, F, H, C = 4200, 64, 2, 3
    g = torch.Generator().manual_seed(7)
    x, W, b = torch.randn(Q, F, generator=g), 0.2 * torch.randn(H, C, F, generator=g), 0.1 * torch.randn(H, C, generator=g)
    labels = torch.randint(0, C, (Q,), generator=g)
    labels[::5] = -3
    labels[1::5] = C + 1000000
    ok = (labels >= 0) & (labels < C)
    want = probe_predict_reference(W, b, x)
    want_loss = -torch.log(want[torch.arange(Q), :, labels.clamp(0, C - 1)])[ok].sum(0)
    _poison_workspace(dev, 4096, H, C, F)
    prob, loss = ops.linprobe_predict(W.to(dev), b.to(dev), x.to(dev), labels.to(dev, torch.int32))
    torch.cuda.synchronize()
    ep, el = float((prob.cpu().double() - want).abs().max()), float(((loss.cpu().double() - want_loss) / int(ok.sum())).abs().max())
    print(f"max |prob - f64| {ep:.3e}, max |mean loss - f64| {el:.3e}")
    assert ep <= STATE_BOUND and el <= LOSS_BOUND


def test_one_exact_step(dev):
    """One head, F = 4, four rows, everything on a power-of-two grid: both classes start from the same weight row, so p = 1/2
    exactly and every product and sum below is exact in f32.
        g[j, 0] = (1/2 - [y_j == 0]) / 4 = -1/8 for the rows of class 0 (rows 0, 2, 3), +1/8 for row 1;  g[j, 1] = -g[j, 0]
        sum_j g[j, 0] x_j = (x1 - x0 - x2 - x3) / 8 = [-0.5625, 0.125, -0.09375, -0.4375]
        dW[0] = that + 0.5 w = [-0.3125, 0, 0.40625, -0.375];   dW[1] = -that + 0.5 w = [0.8125, -0.25, 0.59375, 0.5]
        db = [-0.25 + 0.5 * 0.25, 0.25 + 0.5 * 0.25] = [-0.125, 0.375]
        mW = 0.5 * 1 + dW;  mb = 0.5 * [2, -2] + db = [0.875, -0.625];  step = lr * lr_scale = 0.25
        W = w - 0.25 mW;  b = 0.25 - 0.25 mb = [0.03125, 0.40625];  loss_sum = 4 ln 2"""
    from gipvit import ops
    x = torch.tensor([[1.0, 0.5, -2.0, 4.0], [-1.0, 2.0, 0.25, 0.5], [2.0, 1.0, 1.0, -1.0], [0.5, -0.5, 2.0, 1.0]])
    y = torch.tensor([0, 1, 0, 0], dtype=torch.int32)
    w = [0.5, -0.25, 1.0, 0.125]
    W, b = torch.tensor([[w, w]]).to(dev), torch.tensor([[0.25, 0.25]]).to(dev)
    mW, mb = torch.ones(1, 2, 4, device=dev), torch.tensor([[2.0, -2.0]], device=dev)
    lr, wd = torch.tensor([0.5], device=dev), torch.tensor([0.5], device=dev)
    loss = torch.zeros(1, device=dev)
    _poison_workspace(dev, 4, 1, 2, 4)
    ops.linprobe_train(W, b, mW, mb, lr, wd, x.to(dev), y.to(dev), torch.arange(4, dtype=torch.int32, device=dev), loss, 4, 0.5, 0.5)
    torch.cuda.synchronize()
    assert mW.cpu().tolist() == [[[0.1875, 0.5, 0.90625, 0.125], [1.3125, 0.25, 1.09375, 1.0]]]
    assert mb.cpu().tolist() == [[0.875, -0.625]]
    assert W.cpu().tolist() == [[[0.453125, -0.375, 0.7734375, 0.09375], [0.171875, -0.3125, 0.7265625, -0.125]]]
    assert b.cpu().tolist() == [[0.03125, 0.40625]]
    assert abs(float(loss) - 4.0 * math.log(2.0)) <= 2.4e-7                  # 4 logf(2): one f32 rounding step at 2.77
    # the same call again accumulates into loss_sum
    before = float(loss)
    ops.linprobe_train(W, b, mW, mb, lr, wd, x.to(dev), y.to(dev), torch.arange(4, dtype=torch.int32, device=dev), loss, 4, 0.5, 0.5)
    assert float(loss) > before


def test_bitwise_reproducibility(dev):
    """Two runs agree bit for bit; so does a run over features with a wider row stride and NaN in the padding, and a visiting
    order that repeats row indices gives what the same rows written out one after the other give."""
    case = CASES[0]
    s, ref = case_reference(case)
    N, F = s["x"].shape
    first, again = _train_gpu(dev, s), _train_gpu(dev, s)
    assert all(torch.equal(_bits(a), _bits(c)) for a, c in zip(first, again))
    wide = torch.full((N + 2, F + 8), float("nan"), device=dev)
    wide[1:N + 1, 4:4 + F] = s["x"].to(dev)
    xs = wide[1:N + 1, 4:4 + F]                                             # row stride F + 8, NaN on every side
    assert xs.stride() == (F + 8, 1) and xs.data_ptr() % 16 == 0
    padded = _train_gpu(dev, s, x_dev=xs)
    assert all(torch.equal(_bits(a), _bits(c)) for a, c in zip(first, padded))
    # a multiset of rows: some rows several times, some never
    rng = np.random.Generator(np.random.PCG64(11))
    multi = rng.integers(0, N, size=(2, 150))
    multi[:, 10:14] = multi[:, 9:10]                                        # one row five times in a row, inside one step
    got = _train_gpu(dev, s, perms=multi)
    flat = dict(s, x=torch.cat([s["x"][multi[0]], s["x"][multi[1]]]), labels=torch.cat([s["labels"][multi[0]], s["labels"][multi[1]]]))
    written_out = _train_gpu(dev, flat, perms=np.stack([np.arange(150), 150 + np.arange(150)]))
    assert all(torch.equal(_bits(a), _bits(c)) for a, c in zip(got, written_out))
    want = probe_reference(**dict(s_args(s), perms=multi))
    errs = [float((g.double() - r).abs().max()) for g, r in zip(got, want)]
    print("repeated rows, max |gpu - f64|: W %.3e  b %.3e  mW %.3e  mb %.3e  epoch loss %.3e" % tuple(errs))
    assert max(errs[:4]) <= STATE_BOUND and errs[4] <= LOSS_BOUND


def test_ops_refuse_bad_tensors(dev):
    from gipvit import ops
    W, b, x = torch.zeros(2, 3, 8, device=dev), torch.zeros(2, 3, device=dev), torch.zeros(5, 8, device=dev)
    with pytest.raises(TypeError):
        ops.linprobe_predict(W.double(), b, x)
    with pytest.raises(ValueError):
        ops.linprobe_predict(W, b, torch.zeros(5, 16, device=dev)[:, ::2])       # column stride 2
    with pytest.raises(ValueError):
        ops.linprobe_predict(W, torch.zeros(2, 4, device=dev), x)
    with pytest.raises(ValueError):
        ops.linprobe_predict(W, b, x, torch.zeros(4, dtype=torch.int32, device=dev))
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(ValueError):
        ops.linprobe_train(W, b, z(2, 3, 8), z(2, 3), z(2), z(3), x, torch.zeros(5, dtype=torch.int32, device=dev),
                           torch.zeros(5, dtype=torch.int32, device=dev), z(2), 4)      # wd of the wrong length
    with pytest.raises(TypeError):
        ops.linprobe_train(W, b, z(2, 3, 8), z(2, 3), z(2), z(2), x, torch.zeros(5, dtype=torch.int64, device=dev),
                           torch.zeros(5, dtype=torch.int32, device=dev), z(2), 4)      # int64 labels


# ---- probe_features
def _runner(dev, img=64, batch=8, seed=0):
    from gipvit.engine import FeatureExtractor
    from gipvit import models as M
    runner = FeatureExtractor("vit_tiny", img, batch=batch, device=dev)
    runner.load_state(M.init_vit_state("vit_tiny", img, 0, seed=seed))
    return runner


@pytest.mark.parametrize("form", ["u8", "f32_nchw"])
def test_probe_features_are_the_cls_rows_of_intermediate_layers(dev, form):
    runner = _runner(dev)
    g = torch.Generator().manual_seed(3)
    n, D = 11, 192                                                          # 8 + 3: the second batch is padded
    if form == "u8":
        tiles = torch.randint(0, 256, (n, 64, 64, 3), dtype=torch.uint8, generator=g).to(dev)
    else:
        tiles = torch.randn(n, 3, 64, 64, generator=g).to(dev)
    layers = runner.intermediate_layers(tiles, 4)
    feats = runner.probe_features(tiles, n_last=4, avgpool=True)
    plain = runner.probe_features(tiles, n_last=2)
    torch.cuda.synchronize()
    assert feats.shape == (n, 5 * D) and feats.dtype == f32 and plain.shape == (n, 2 * D)
    cls = torch.cat([o[:, 0, :] for o in layers], dim=1)
    assert torch.equal(_bits(feats[:, :4 * D]), _bits(cls)) and torch.equal(_bits(plain), _bits(cls[:, 2 * D:]))
    pooled = layers[-1][:, 1:, :].double().mean(dim=1)
    err = float((feats[:, 4 * D:].double() - pooled).abs().max())
    print(f"pooled part against the f64 mean of the last layer's patch tokens: {err:.3e}")
    assert err <= 1e-6 and float(pooled.abs().max()) > 1e-3
    with pytest.raises(ValueError):
        runner.probe_features(tiles, n_last=0)
    with pytest.raises(ValueError):
        runner.probe_features(tiles, n_last=13)
    with pytest.raises(ValueError):
        runner.probe_features(tiles[:, :48] if form == "u8" else tiles[:, :, :48], n_last=1)


def test_probe_features_at_512_px(dev):
    """Forward only, so the probe's features go up to 512-px tiles (1025 tokens, the streaming attention forward): a padded
    second batch, against intermediate_layers as above."""
    runner = _runner(dev, img=512, batch=2)
    tiles = torch.randint(0, 256, (3, 512, 512, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(dev)
    layers = runner.intermediate_layers(tiles, 2)
    feats = runner.probe_features(tiles, n_last=2, avgpool=True)
    torch.cuda.synchronize()
    assert layers[0].shape == (3, 1025, 192) and feats.shape == (3, 3 * 192)
    assert torch.equal(_bits(feats[:, :384]), _bits(torch.cat([o[:, 0, :] for o in layers], dim=1)))
    err = float((feats[:, 384:].double() - layers[-1][:, 1:, :].double().mean(dim=1)).abs().max())
    print(f"512 px, pooled part against the f64 mean of 1024 patch tokens: {err:.3e}")
    assert err <= 1e-6 and bool(torch.isfinite(feats).all())


def test_probe_features_refuse_a_mean_pooled_model(dev):
    from gipvit.engine import FeatureExtractor
    runner = FeatureExtractor("vit_tiny", 64, batch=4, device=dev, global_pool="avg")
    with pytest.raises(ValueError):
        runner.probe_features(torch.zeros(4, 64, 64, 3, dtype=torch.uint8, device=dev))


# ---- LinearProbe on a real encoder
def test_linear_probe_matches_the_host_reference_on_the_runners_features(dev):
    from gipvit import data as D
    from gipvit.linprobe import LinearProbe, epoch_permutations, holdout_slides, init_heads, probe_metrics, select_head
    runner = _runner(dev)
    lrs, epochs, batch, n_last = (0.05, 0.2, 0.8), 3, 16, 2
    probe = LinearProbe(runner, num_classes=2, lrs=lrs, epochs=epochs, batch=batch, n_last=n_last, weight_decay=1e-4, seed=5)
    bank_loader, query_loader = D.SyntheticSlides(5, 12, 64, tiles_per_iter=5, seed=11), D.SyntheticSlides(4, 9, 64, tiles_per_iter=7, seed=23)
    assert probe.fit(bank_loader) == 48                                     # slide 4 of 5 is held out
    got = probe.evaluate(query_loader)
    assert list(got) == ["linear_top1", "linear_loss", "linear_auc_per_patch", "linear_auc_per_slide"]
    sd = probe.state_dict()
    assert sd["weight"].shape == (2, n_last * 192) and sd["bias"].shape == (2,) and torch.equal(sd["weight"], probe.W[probe.head].cpu())
    assert torch.equal(probe.state_dict(head=2)["bias"], probe.b[2].cpu())

    # the same procedure through the host reference on the runner's own features
    def feats(loader):
        return torch.cat([runner.probe_features(mb["Data"].to(dev), n_last) for mb in loader]).cpu()
    fb, fq = feats(bank_loader), feats(query_loader)
    yb, yq = torch.tensor(sum(([k % 2] * 12 for k in range(5)), [])), torch.tensor(sum(([k % 2] * 9 for k in range(4)), []))
    held_np = np.repeat(holdout_slides(5, 0.2), 12)
    assert held_np.tolist() == [False] * 48 + [True] * 12
    train_idx, held = np.nonzero(~held_np)[0], torch.from_numpy(held_np)
    W0, b0 = init_heads(3, 2, n_last * 192, seed=5)
    perms = train_idx[epoch_permutations(48, epochs, seed=5)]
    W, b, mW, mb, loss = probe_reference(fb, yb, W0, b0, [v * batch / 256.0 for v in lrs], [1e-4] * 3, perms, batch)
    errs = (float((probe.W.cpu().double() - W).abs().max()), float((probe.b.cpu().double() - b).abs().max()),
            float((torch.tensor(probe.train_loss, dtype=torch.float64) - loss).abs().max()))
    print("fit against the reference: W %.3e  b %.3e  epoch loss %.3e; f64 last-epoch losses %s" % (errs + ([round(float(v), 4) for v in loss[-1]],)))
    assert errs[0] <= STATE_BOUND and errs[1] <= STATE_BOUND and errs[2] <= LOSS_BOUND
    ps = probe_predict_reference(W, b, fb[held])
    sel_loss = (-torch.log(ps[torch.arange(12), :, yb[held]]).mean(0)).tolist()
    gaps = sorted(sel_loss)
    print("selection losses", sel_loss, "probe", probe.selection_loss, "head", probe.head)
    assert min(b_ - a_ for a_, b_ in zip(gaps, gaps[1:])) >= 1e-5            # well posed: an f32 run cannot change the order
    assert max(abs(a_ - b_) for a_, b_ in zip(sel_loss, probe.selection_loss)) <= LOSS_BOUND
    assert probe.head == select_head(sel_loss)
    pq = probe_predict_reference(W, b, fq)[:, probe.head]
    want = probe_metrics(pq.numpy(), yq.numpy(), np.repeat(np.arange(4), 9), float(-torch.log(pq[torch.arange(36), yq]).mean()))
    print("probe", dict(got), "reference", dict(want))
    assert got["linear_top1"] == want["linear_top1"] and abs(got["linear_loss"] - want["linear_loss"]) <= LOSS_BOUND
    assert abs(got["linear_auc_per_patch"] - want["linear_auc_per_patch"]) <= 1e-6 and abs(got["linear_auc_per_slide"] - want["linear_auc_per_slide"]) <= 1e-6
    # one head: nothing is held out
    one = LinearProbe(runner, num_classes=2, lrs=(0.2,), epochs=1, batch=16, n_last=1)
    assert one.fit(bank_loader) == 60 and one.head == 0 and one.selection_loss is None
    with pytest.raises(ValueError):
        LinearProbe(runner, lrs=(0.1, 0.2), epochs=1, n_last=1).fit(D.SyntheticSlides(1, 6, 64, tiles_per_iter=6, seed=2))      # one slide, two heads


def test_linear_probe_feeds_the_centred_window_of_larger_tiles(dev):
    from gipvit import data as D
    from gipvit.linprobe import LinearProbe
    runner = _runner(dev)
    probe = LinearProbe(runner, lrs=(0.1,), epochs=1, batch=8, n_last=1)
    mb = next(iter(D.SyntheticSlides(1, 6, 96, tiles_per_iter=6, seed=5)))      # 96-px tiles into the 64-px runner
    manual = runner.probe_features(mb["Data"][:, 16:80, 16:80, :].contiguous().to(dev), 1)
    assert torch.equal(_bits(probe.features(mb["Data"])), _bits(manual))


# ---- the driver
def test_driver_writes_linear_metrics_and_picks_model_best_on_them(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import train
    base = ["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--out-dim", "1024", "--batches-per-epoch", "2", "--epochs", "2",
            "--lr", "1e-4", "--warmup-epochs", "0", "--log-interval", "1", "--output", str(tmp_path), "--seed", "3", "--linear-probe",
            "--linprobe-lrs", "0.1", "0.4", "--linprobe-epochs", "3", "--linprobe-batch", "16", "--linprobe-layers", "2"]
    names = ["eval_linear_top1", "eval_linear_loss", "eval_linear_auc_per_patch", "eval_linear_auc_per_slide"]
    knn = ["eval_knn_top1", "eval_knn_auc_per_patch", "eval_knn_auc_per_slide"]
    # --linprobe-rate 1: every epoch; the default --eval-metric top1 resolves to linear_top1
    assert train.main(base + ["--experiment", "every", "--linprobe-rate", "1"]) == 0
    rows = list(csv.DictReader(open(tmp_path / "every" / "summary.csv")))
    assert len(rows) == 2 and not any(k in rows[0] for k in knn)
    for r in rows:
        assert 0.0 <= float(r["eval_linear_top1"]) <= 100.0 and float(r["eval_linear_loss"]) > 0 and float(r["train_loss"]) > 0
        assert all(0.0 <= float(r[n]) <= 1.0 for n in names[2:])
    top1 = [float(r["eval_linear_top1"]) for r in rows]
    best = torch.load(tmp_path / "every" / "model_best.pth.tar", weights_only=True)
    assert best["metric"] == max(top1) and best["epoch"] == (1 if top1[1] > top1[0] else 0)      # increasing
    # the default rate with the k-NN monitor beside it: the probe runs after the last epoch only, its columns stay; model_best
    # follows --eval-metric linear_auc_per_slide, which only the last epoch has
    assert train.main(base + ["--experiment", "last", "--knn-monitor", "--knn-k", "5", "--eval-metric", "linear_auc_per_slide"]) == 0
    rows = list(csv.DictReader(open(tmp_path / "last" / "summary.csv")))
    assert len(rows) == 2 and all(rows[0][n] == "" for n in names) and all(rows[1][n] != "" for n in names)
    assert all(rows[0][n] != "" and rows[1][n] != "" for n in knn)
    best = torch.load(tmp_path / "last" / "model_best.pth.tar", weights_only=True)
    assert best["epoch"] == 1 and best["metric"] == float(rows[1]["eval_linear_auc_per_slide"])
    assert "metric" not in torch.load(tmp_path / "last" / "checkpoint-0.pth.tar", weights_only=True)
    # the monitors on different schedules (k-NN on epoch 2 of 3, the probe after the last): the header is written once and
    # every value is read back under its own name
    assert train.main(base + ["--experiment", "mixed", "--epochs", "3", "--knn-monitor", "--knn-k", "5", "--knn-rate", "2"]) == 0
    rows = list(csv.DictReader(open(tmp_path / "mixed" / "summary.csv")))
    assert len(rows) == 3 and all(r[n] == "" for r in (rows[0], rows[2]) for n in knn) and all(r[n] == "" for r in rows[:2] for n in names)
    assert 0.0 <= float(rows[1]["eval_knn_top1"]) <= 100.0 and all(0.0 <= float(rows[1][n]) <= 1.0 for n in knn[1:])
    assert 0.0 <= float(rows[2]["eval_linear_top1"]) <= 100.0 and float(rows[2]["eval_linear_loss"]) > 0
    assert all(0.0 <= float(rows[2][n]) <= 1.0 for n in names[2:]) and [int(r["epoch"]) for r in rows] == [0, 1, 2]
    best = torch.load(tmp_path / "mixed" / "model_best.pth.tar", weights_only=True)      # knn_top1: only epoch 1 has it
    assert best["epoch"] == 1 and best["metric"] == float(rows[1]["eval_knn_top1"])
    # a name neither monitor reports is refused with the other flags
    with pytest.raises(SystemExit) as e:
        train.main(base + ["--experiment", "bad", "--eval-metric", "f1"])
    assert "--eval-metric" in str(e.value)
