"""Float32 NCHW input already normalised (the reference's ``Data`` batches, train.py:1027-1033) on the device:
gv_patchify_nchw bit-exact against torch's reshape / permute / .to(), the engines against the oracle on float input with
no uint8 tile behind it, the cross-path against the fused-normalise uint8 path, the model seam and the data pipeline."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

WINDOW_SETS = ((224, [(0, 0), (16, 16)]), (96, [(20 * l, 160 - 20 * l) for l in range(8)]), (96, [(1, 3), (7, 157)]))


def ref_rows(x, wins, crop):
    """torch restatement: crop, then [n, 3, side, 16, side, 16] -> rows [n * side^2, 768] with k = c*256 + py*16 + px."""
    side, rows = crop // 16, []
    for (y0, x0) in wins:
        w = x[:, :, y0:y0 + crop, x0:x0 + crop]
        rows.append(w.reshape(w.shape[0], 3, side, 16, side, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1, 768))
    return torch.cat(rows)


def assert_bits_equal(got, ref, what):
    """Equal bit patterns, except that a NaN only has to be a NaN."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan), what
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(it)[~nan], ref.view(it)[~nan]), (what, int((got.view(it) != ref.view(it)).sum()))


def _inputs(dev):
    g = torch.Generator().manual_seed(17)
    x = (3.0 * torch.randn(3, 3, 256, 256, generator=g))
    x[0, 0, 5, 7] = float("inf"); x[1, 2, 100, 200] = float("-inf"); x[2, 1, 30, 40] = float("nan"); x[0, 1, 20, 21] = -0.0
    x[1, 0, 50, 60] = 1e30; x[2, 2, 60, 70] = 3.3895314e38        # overflow the 16-bit range: must round to +-Inf like torch
    big = torch.randn(5, 3, 262, 270, generator=g)
    sl = big[1:4, :, 3:259, 7:263]                                   # a strided slice: N / C / H strides of the big batch, odd offset
    return x.to(dev), big.to(dev)[1:4, :, 3:259, 7:263], sl


def check_patchify_nchw_exact(dev, half):
    from gipvit import ops
    act = torch.float16 if half else torch.bfloat16
    assert ops.bf16 == act
    x, xs_dev, xs_cpu = _inputs(dev)
    for src, cpu in ((x, x.cpu()), (xs_dev, xs_cpu)):
        assert src.stride(-1) == 1
        for crop, wins in WINDOW_SETS:
            ref = ref_rows(cpu, wins, crop)
            assert_bits_equal(ops.patchify_nchw(src, wins, crop).cpu(), ref.to(act), f"{act} {crop} {wins[:2]} {src.stride()}")
            out = torch.empty(ref.shape, dtype=torch.float32, device=dev)
            assert_bits_equal(ops.patchify_nchw(src, wins, crop, out=out).cpu(), ref, f"f32 {crop} {wins[:2]} {src.stride()}")
    # DINO's two crop groups and a 256-px crop (one strip of 16 patches per workgroup) on a batch of 64
    g = torch.Generator().manual_seed(3)
    b = torch.randn(64, 3, 256, 256, generator=g)
    for crop, wins in ((256, [(0, 0)]), (224, [(0, 0), (16, 16)])):
        assert_bits_equal(ops.patchify_nchw(b.to(dev), wins, crop).cpu(), ref_rows(b, wins, crop).to(act), f"B64 {crop}")


def test_patchify_nchw_exact(dev):
    check_patchify_nchw_exact(dev, half=False)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "f16"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, GIPVIT_ACT_FORMAT="f16"))
    assert r.returncode == 0 and r.stdout.strip().endswith("NCHW F16 OK"), (r.stdout[-2000:], r.stderr[-3000:])


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _check_grads(got, ref, tol=5e-2, skip=()):
    """The parity gates of tests/test_engine_gpu.py: per-parameter relative error and the global gradient norm."""
    worst, gn_g, gn_r = [], 0.0, 0.0
    for k, r in ref.items():
        if r is None or k in skip:
            continue
        g = got[k]
        gn_g += float((g.double() ** 2).sum()); gn_r += float((r.double() ** 2).sum())
        if float(r.abs().max()) >= 1e-12:
            worst.append((_rel(g, r), k))
    worst.sort(reverse=True)
    assert worst[0][0] <= tol, f"gradient mismatch: {worst[:8]}"
    rel_norm = abs(math.sqrt(gn_g) - math.sqrt(gn_r)) / math.sqrt(gn_r)
    assert rel_norm <= 1e-2, f"grad-norm rel err {rel_norm}"
    return worst[0], rel_norm


def test_cross_path_u8_and_normalised_float(dev):
    """u8 tiles t (fused normalise) against x = normalize_window(t): the same step up to one 16-bit ulp in a few patch values."""
    from gipvit import ops
    from gipvit.engine import SupervisedEngine
    from oracle import step_oracle as so, vit_oracle as vo
    orc = so.SupervisedOracle(arch="vit_tiny", img_size=64, num_classes=2, seed=0)
    eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, device=dev)
    eng.load_state(orc.p)
    t = vo.synth_tiles(8, 64, seed=1234)
    x = vo.normalize_window(t, (0, 0, 64))
    p_u8 = ops.patchify(t.to(dev), [(0, 0)], 64, eng.mean, eng.std).cpu()
    p_f = ops.patchify_nchw(x.to(dev), [(0, 0)], 64).cpu()
    d = (p_u8.view(torch.int16).int() - p_f.view(torch.int16).int()).abs()
    frac = float((d != 0).float().mean())
    print(f"[cross-path] patch values one ulp apart: {frac:.2e} of {d.numel()}")
    assert int(d.max()) <= 1 and frac < 1e-2
    tgt = torch.randint(0, 2, (8, 1), generator=torch.Generator().manual_seed(5)).to(dev)
    out = {}
    for name, src in (("u8", t.to(dev)), ("f32", x.to(dev))):
        eng.forward_backward(src, tgt)
        torch.cuda.synchronize()
        out[name] = (eng.logits.clone().cpu(), float(eng.loss))
    assert float((out["u8"][0] - out["f32"][0]).abs().max()) <= 1e-3
    assert abs(out["u8"][1] - out["f32"][1]) <= 1e-3


def _supervised_reference(orc, x, tgt):
    sp = {k: v.detach().clone().requires_grad_(True) for k, v in orc.p.items()}
    from oracle import vit_oracle as vo
    logits = vo.vit_logits(sp, x, orc.arch)
    loss = vo.softmax_lsce(logits, tgt, orc.smoothing)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in sp.items()}, logits.detach()


def test_supervised_float_input_against_oracle(dev):
    """randn NCHW input (no uint8 tile exists): ViT-T step at test_supervised_step_parity's gates, then the fp32 mode at 1e-4."""
    from gipvit.engine import SupervisedEngine
    from oracle import step_oracle as so
    orc = so.SupervisedOracle(arch="vit_tiny", img_size=64, num_classes=2, seed=0, lr=1e-3, wd=0.05)
    x = torch.randn(8, 3, 64, 64, generator=torch.Generator().manual_seed(21))
    tgt = torch.randint(0, 2, (8, 1), generator=torch.Generator().manual_seed(5))
    loss_r, grads_r, logits_r = _supervised_reference(orc, x, tgt)
    eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, lr=1e-3, weight_decay=0.05, device=dev)
    eng.load_state(orc.p)
    eng.forward_backward(x.to(dev), tgt.to(dev))
    torch.cuda.synchronize()
    scale = float(logits_r.abs().max())
    assert float((eng.logits.cpu() - logits_r).abs().max()) <= 2e-2 * max(scale, 1.0)
    assert abs(float(eng.loss) - float(loss_r)) <= 1e-3
    _check_grads(eng.grads(), grads_r)
    l = eng.step(x.to(dev), tgt.to(dev))
    assert math.isfinite(float(l))
    # fp32 operand mode: exact f32 patch rows
    e32 = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=8, lr=1e-3, weight_decay=0.05, device=dev, precision="fp32")
    e32.load_state(orc.p)
    e32.forward_backward(x.to(dev), tgt.to(dev))
    torch.cuda.synchronize()
    dl = float((e32.logits.cpu() - logits_r).abs().max())
    print(f"[fp32 float input] logits max-abs err {dl:.2e}")
    assert dl <= 1e-4 and abs(float(e32.loss) - float(loss_r)) <= 1e-4
    _check_grads(e32.grads(), grads_r, tol=1e-3)


def test_dino_float_input_against_oracle(dev):
    """randn NCHW [B, 3, 256, 256]: the fixed windows' slices of the float batch through vo.multicrop_forward / vo.dino_loss,
    at test_dino_step_parity's gates; then step and step_micro run on float batches."""
    from gipvit.engine import DinoEngine
    from oracle import step_oracle as so, vit_oracle as vo
    K, B = 4096, 2
    orc = so.DinoOracle(arch="vit_tiny", img_size=224, out_dim=K, seed=0, lr=5e-4, wd=0.04, n_local=8)
    eng = DinoEngine(arch="vit_tiny", img_size=224, out_dim=K, batch=B, n_local=8, lr=5e-4, weight_decay=0.04, device=dev)
    eng.load_state(orc.p, orc.hp)
    c = 0.05 * torch.randn(1, K, generator=torch.Generator().manual_seed(3))
    orc.center = c.clone(); eng.center.copy_(c[0])
    x = torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(8))
    crops = [x[:, :, y:y + s, x0:x0 + s] for (y, x0, s) in orc.wins]
    with torch.no_grad():
        t_out = vo.multicrop_forward(orc.tp, orc.thp, crops[:2], orc.arch)
    sp = {k: v.detach().clone().requires_grad_(True) for k, v in orc.p.items()}
    shp = {k: v.detach().clone().requires_grad_(True) for k, v in orc.hp.items()}
    s_out = vo.multicrop_forward(sp, shp, crops, orc.arch)
    loss_r, bsum = vo.dino_loss(s_out, t_out, orc.center, len(crops), 2, orc.ts, orc.tt)
    loss_r.backward()
    loss_r = loss_r.detach()
    grads_r = {**{"backbone." + k: v.grad for k, v in sp.items()}, **{"head." + k: v.grad for k, v in shp.items()}}
    eng.set_hyper()
    eng.forward_backward(x.to(dev))
    torch.cuda.synchronize()
    for got, ref, nm in ((eng.hb_t.logits, t_out, "teacher"), (eng.hb_s.logits, s_out.detach(), "student")):
        err = float((got.cpu() - ref).abs().max())
        assert err <= 2e-2 * float(ref.abs().max()), (nm, err, float(ref.abs().max()))
    assert abs(float(eng.loss) - float(loss_r)) <= 1e-3, (float(eng.loss), float(loss_r))
    assert _rel(eng.center_sum, bsum[0]) < 1e-2
    _check_grads(eng.grads(), grads_r, skip=("head.last_layer.weight_g",))
    l1 = float(eng.step(x.to(dev)))
    l2 = float(eng.step_micro([x.to(dev), x.to(dev)]))
    assert math.isfinite(l1) and math.isfinite(l2)


def test_model_seam_feature_extractor_and_errors(dev):
    from gipvit import models as M
    from gipvit.engine import FeatureExtractor
    from oracle import vit_oracle as vo
    model = M.create_model("vit_tiny_patch16_224", img_size=64, batch=8, num_classes=2, device=dev)
    x = torch.randn(8, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(dev)
    a = model(x).clone()
    b = model.engine.forward(x)[0].clone()
    assert torch.equal(a, b)
    assert torch.equal(model(x.to(memory_format=torch.channels_last)).clone(), a)
    assert torch.equal(model.forward_features(x.to(memory_format=torch.channels_last)).clone(), model.engine.forward(x)[1].clone())
    t = vo.synth_tiles(8, 64, seed=1).to(dev)
    assert model(t).shape == (8, 2)                                     # the uint8 form is unchanged
    # other dtypes / layouts and u8-pipeline arguments
    for bad in (x.half(), x.double(), x.permute(0, 2, 3, 1)):
        with pytest.raises(TypeError, match="float32 NCHW"):
            model(bad)
    with pytest.raises(TypeError):
        model.engine.forward(x.to(memory_format=torch.channels_last))
    with pytest.raises(ValueError, match="fill="):
        model.engine.forward(x, fill=torch.zeros(8, 8, device=dev))
    with pytest.raises(ValueError):
        model.engine.forward(x[:4])
    # FeatureExtractor.run on a float chunk that is not a multiple of B: the padded last batch takes a float pad buffer
    fe = FeatureExtractor("vit_tiny", 64, 8, 2, device=dev, weights=model.engine.W)
    xs = torch.randn(13, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(dev)
    feats, logits = fe.run(xs)
    f0, l0 = (v.float().clone() for v in fe.forward(xs[:8]))
    pad = torch.zeros(8, 3, 64, 64, device=dev); pad[:5] = xs[8:]
    f1, l1 = (v.float().clone() for v in fe.forward(pad))
    torch.cuda.synchronize()
    assert feats.shape == (13, fe.D) and torch.equal(feats, torch.cat([f0, f1[:5]])) and torch.equal(logits, torch.cat([l0, l1[:5]]))
    with pytest.raises(ValueError):
        fe.forward(xs[:8, :, :32, :32])


def test_dino_float_refuses_u8_pipeline_arguments(dev):
    from gipvit.engine import DinoEngine
    eng = DinoEngine(arch="vit_tiny", img_size=224, out_dim=1024, batch=2, device=dev)
    x = torch.randn(2, 3, 256, 256, device=dev)
    boxes = (torch.zeros(4, 6, dtype=torch.int32, device=dev), torch.zeros(16, 6, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="boxes="):
        eng.forward_backward(x, boxes=boxes)
    with pytest.raises(ValueError, match="fill="):
        eng.step(x, fill=torch.zeros(2, 8, device=dev))
    with pytest.raises(ValueError, match="shape"):
        eng.step(torch.randn(2, 3, 224, 224, device=dev))
    with pytest.raises(TypeError):
        eng.step(x.half())


MEAN, STD = torch.tensor([0.8998, 0.8253, 0.9357]), torch.tensor([0.1125, 0.1751, 0.0787])


def float_hook(tile):
    """ToTensor + Normalize, as the reference's hooks end (transformations.py:124-128): uint8 HWC -> float [3, H, W]."""
    x = torch.from_numpy(np.array(tile)).permute(2, 0, 1).float() / 255.0
    return (x - MEAN[:, None, None]) / STD[:, None, None]


def test_float_hook_pipeline_and_driver(dev, tmp_path):
    """TileFolder in float mode -> DevicePrefetcher (pinned f32 staging) -> device batches equal to the hook's; then the driver
    trains supervised and DINO (fixed windows) on such batches."""
    sys.path.insert(0, ROOT)
    import csv
    import train
    from gipvit import data as D
    rng = np.random.default_rng(0)
    root = tmp_path / "tiles"
    for s in range(4):
        os.makedirs(root / f"slide{s}")
        for i in range(4):
            D.write_tile_file(str(root / f"slide{s}" / f"tile_{i}.data"), rng.integers(0, 256, (256, 256, 3), dtype=np.uint8))
    (root / "labels.csv").write_text("slide,label,fold\n" + "".join(f"slide{s},{s % 2},{1 + s // 2}\n" for s in range(4)))
    src = D.TileFolder(str(root), 4, float_hook, seed=3, tile_size=64, n_tiles=4)
    ref = list(D.TileFolder(str(root), 4, float_hook, seed=3, tile_size=64, n_tiles=4))
    pf = D.DevicePrefetcher(src, dev, (4, 64, 64, 3))
    got = [(mb["Data"].cpu().clone(), mb["Target"].cpu().clone()) for mb in pf]
    assert pf.batch_format == "f32_nchw" and len(got) == len(ref) == 4
    for (d, t), r in zip(got, ref):
        assert d.dtype == torch.float32 and d.shape == (4, 3, 64, 64)
        assert torch.equal(d, r["Data"]) and torch.equal(t, r["Target"])
    rc = train.main(["--model", "vit_tiny_patch16_224", "--dataset", f"tiles:{root}", "--num-classes", "2", "--img-size", "64", "--tile-size", "64",
                     "-b", "4", "--epochs", "1", "--opt", "adamw", "--lr", "1e-4", "--warmup-epochs", "0", "--output", str(tmp_path), "--experiment", "sup",
                     "--n_patches_train", "4", "--test_fold", "2", "--workers", "3", "--num_tiles", "5", "--tiles_per_iter", "3",
                     "--eval-metric", "loss", "--log-interval", "1"], transform=float_hook)
    assert rc == 0
    rows = list(csv.DictReader(open(tmp_path / "sup" / "summary.csv")))
    assert len(rows) == 1 and np.isfinite(float(rows[0]["train_loss"])) and np.isfinite(float(rows[0]["eval_loss"]))
    rc = train.main(["--dino", "--model", "vit_tiny", "--dataset", f"tiles:{root}", "-b", "2", "--out-dim", "1024", "--lr", "1e-4", "--epochs", "1",
                     "--log-interval", "1", "--output", str(tmp_path), "--experiment", "dino", "--seed", "7", "--no-validate",
                     "--n_patches_train", "2", "--test_fold", "-1"], transform=float_hook)
    assert rc == 0
    rows = list(csv.DictReader(open(tmp_path / "dino" / "summary.csv")))
    assert len(rows) == 1 and 5.0 < float(rows[0]["train_loss"]) < 8.0


if __name__ == "__main__":          # the float16 build, in a process of its own (GIPVIT_ACT_FORMAT=f16)
    sys.path.insert(0, ROOT)
    assert sys.argv[1:] == ["f16"] and os.environ.get("GIPVIT_ACT_FORMAT") == "f16"
    check_patchify_nchw_exact(torch.device("cuda:0"), half=True)
    torch.cuda.synchronize()
    print("NCHW F16 OK")
