"""GPU: get_last_selfattention / get_intermediate_layers (vit.pyc@L255-272) -- the gv_attention_probs kernels against torch, the
model seam and FeatureExtractor against the oracle composition of tests/test_attention_maps_host.py, non-interference with the
default path and training, and the driver's --extract-attention."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import vit_oracle as vo
from test_attention_maps_host import reference_attention_and_layers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SENTINEL = -12345.0


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _torch_softmax(qkv, n_img, N, H, scale, dt=torch.float32):
    x = qkv.to(dt).view(n_img, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    return ((x[0] @ x[1].transpose(-2, -1)) * scale).softmax(-1), x[2]


def check_probs(dev, N, H, n_img, q_rows_set, spike=False, q_limit=0):
    """One shape: returns the largest |dP| and row-sum error over the q_rows cases (asserting the gates on the way)."""
    from gipvit import ops
    scale = 64 ** -0.5
    g = torch.Generator().manual_seed(N * 131 + H)
    qkv = torch.randn(n_img * N, 3 * H * 64, generator=g)
    if spike:       # one key dominates every query: q = 1, k[7] = 3 -> score 24 against O(1)
        v = qkv.view(n_img, N, 3, H, 64)
        v[:, :, 0] = 1.0
        v[:, 7, 1] = 3.0
    qkv = qkv.to(ops.bf16).to(dev)
    o, lse = ops.attention_fwd(qkv, n_img, N, H, scale, q_limit=q_limit)
    ref, vref = _torch_softmax(qkv.cpu(), n_img, N, H, scale)
    worst = [0.0, 0.0]
    for q_rows in q_rows_set:
        n = n_img * H * q_rows * N
        buf = torch.full((n + 37,), SENTINEL, dtype=torch.float32, device=dev)
        p = ops.attention_probs(qkv, lse, n_img, N, H, scale, q_rows, p=buf[:n].view(n_img, H, q_rows, N)).cpu()
        tail = buf[n:].cpu()
        assert torch.all(tail == SENTINEL), (N, H, q_rows, "wrote behind p")
        d = float((p - ref[:, :, :q_rows]).abs().max())
        s = float((p.double().sum(-1) - 1).abs().max())
        worst = [max(worst[0], d), max(worst[1], s)]
        assert d <= 1e-4 and s <= 1e-4, (N, H, n_img, q_rows, d, s)
        if q_rows == N:     # P and lse pair up: P V in fp32 is the forward's o
            pv = (p @ vref).permute(0, 2, 1, 3).reshape(n_img * N, H * 64)
            e = float((pv - o.float().cpu()).abs().max())
            assert e <= 2e-2, (N, H, e)
    return worst


def test_attention_probs_parity(dev):
    worst = [0.0, 0.0]
    for N, H, n_img in ((17, 3, 3), (37, 6, 5), (64, 12, 3), (65, 6, 3), (197, 6, 3), (257, 6, 5), (257, 12, 3), (288, 12, 3), (288, 3, 1)):
        w = check_probs(dev, N, H, n_img, (1, 5, N))
        worst = [max(a, b) for a, b in zip(worst, w)]
    w = check_probs(dev, 257, 6, 3, (1,), q_limit=1)          # the CLS-only forward leaves lse valid for row 0
    worst = [max(a, b) for a, b in zip(worst, w)]
    w = check_probs(dev, 197, 6, 3, (1, 5, 197), spike=True)
    worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"gv_attention_probs: max |dP| {worst[0]:.3e}, max |row sum - 1| {worst[1]:.3e}")


def test_attention_probs_f32_parity(dev):
    from gipvit import ops
    scale = 64 ** -0.5
    worst = 0.0
    for N, H, n_img in ((17, 3, 3), (65, 6, 3), (197, 6, 3), (257, 6, 3), (260, 3, 1)):
        qkv = torch.randn(n_img * N, 3 * H * 64, generator=torch.Generator().manual_seed(N)).to(dev)
        o, lse = ops.attention_fwd(qkv, n_img, N, H, scale)
        ref, _ = _torch_softmax(qkv.cpu(), n_img, N, H, scale, torch.float64)
        for q_rows in (1, 5, N):
            p = ops.attention_probs(qkv, lse, n_img, N, H, scale, q_rows).cpu()
            d = float((p.double() - ref[:, :, :q_rows]).abs().max())
            worst = max(worst, d)
            assert d <= 1e-6, (N, H, q_rows, d)
    print(f"gv_attention_probs_f32: max |dP| against fp64 {worst:.3e}")


def _model(dev, precision):
    from gipvit import models as M
    m = M.create_model("vit_tiny", img_size=64, batch=2, device=dev, precision=precision)
    p = vo.init_vit("vit_tiny", 64, 2, seed=0)
    m.load_state_dict(p)
    return m, p


@pytest.mark.parametrize("precision,attn_tol,layer_tol", [("bf16", 1e-2, 2e-2), ("fp32", 2e-5, 1e-4)])
def test_model_seam_against_reference(dev, precision, attn_tol, layer_tol):
    m, p = _model(dev, precision)
    t = vo.synth_tiles(2, 64, seed=5)
    xf = vo.normalize_window(t, (0, 0, 64))
    with torch.no_grad():
        ref_attn, ref_layers = reference_attention_and_layers({k: v.double() for k, v in p.items()}, xf.double(), "vit_tiny")
    for x in (t.to(dev), xf.to(dev)):
        a = m.get_last_selfattention(x)
        assert a.shape == (2, 3, 17, 17) and a.dtype == torch.float32
        da = float((a.cpu().double() - ref_attn).abs().max())
        assert da <= attn_tol, (precision, da)
        msg = [f"{precision} attention max abs {da:.2e}"]
        for n in (1, 4, 12):
            got = m.get_intermediate_layers(x, n)
            assert len(got) == n and all(g.shape == (2, 17, 192) and g.dtype == torch.float32 for g in got)
            for k, g in enumerate(got):
                r = _rel(g, ref_layers[12 - n + k])
                assert r <= layer_tol, (precision, n, k, r)
            msg.append(f"n={n} rel {max(_rel(g, ref_layers[12 - n + k]) for k, g in enumerate(got)):.2e}")
        print(", ".join(msg))
    # any batch size; images of another size are refused
    a5 = m.get_last_selfattention(vo.synth_tiles(5, 64, seed=6).to(dev))
    assert a5.shape == (5, 3, 17, 17)
    with pytest.raises(ValueError):
        m.get_last_selfattention(vo.synth_tiles(2, 32, seed=6).to(dev))
    with pytest.raises(ValueError):
        m.get_intermediate_layers(torch.zeros(2, 3, 32, 32, device=dev))


def test_feature_extractor_vit_s_256(dev):
    from gipvit.engine import FeatureExtractor
    p = vo.init_vit("vit_small", 256, 0, seed=3)
    fe = FeatureExtractor("vit_small", 256, batch=4, device=dev)
    fe.load_state(p)
    t = vo.synth_tiles(11, 256, seed=7)
    full = fe.last_selfattention(t.to(dev))
    cls = fe.last_selfattention(t.to(dev), cls_only=True)
    layers = fe.intermediate_layers(t.to(dev), 4)
    with torch.no_grad():
        ref_attn, ref_layers = reference_attention_and_layers(p, vo.normalize_window(t, (0, 0, 256)), "vit_small")
    assert full.shape == (11, 6, 257, 257) and cls.shape == (11, 6, 1, 257)
    da = float((full.cpu() - ref_attn).abs().max())
    dc = float((cls - full[:, :, :1]).abs().max())
    assert da <= 1e-2 and dc <= 1e-6, (da, dc)
    rel = [_rel(g, ref_layers[8 + k]) for k, g in enumerate(layers)]
    assert len(layers) == 4 and all(g.shape == (11, 257, 384) for g in layers) and max(rel) <= 2e-2, rel
    print(f"ViT-S 256: attention max abs {da:.2e}, cls vs row 0 {dc:.2e}, layers rel {max(rel):.2e}")


def test_non_interference(dev):
    from gipvit.engine import FeatureExtractor
    m, _ = _model(dev, "bf16")
    x = vo.synth_tiles(2, 64, seed=8).to(dev)
    f0 = m.forward_features(x).clone()
    m.get_last_selfattention(x); m.get_intermediate_layers(x, 4)
    assert torch.equal(m.forward_features(x).clone(), f0)
    # a training step with the calls between forward_backward and optimizer_step == the same step without them
    tgt = torch.tensor([0, 1], dtype=torch.int64, device=dev)
    res = []
    for calls in (False, True):
        mm, _ = _model(dev, "bf16")
        e = mm.engine
        e.forward_backward(x, tgt)
        if calls:
            mm.get_last_selfattention(x); mm.get_intermediate_layers(x, 12)
        g = e.arena.g.clone()
        e.optimizer_step(lr=1e-3)
        torch.cuda.synchronize()
        res.append((g, e.arena.p.clone(), e.arena.pb.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # FeatureExtractor.run: features bit-identical with and without the CLS-row capture
    fe = FeatureExtractor("vit_tiny", 64, 4, 2, device=dev, weights=m.engine.W)
    t = vo.synth_tiles(7, 64, seed=9).to(dev)
    fa, la = fe.run(t)
    fb, lb, attn = fe.run_with_attention(t)
    assert torch.equal(fa, fb) and torch.equal(la, lb) and attn.shape == (7, 3, 17)


def test_driver_extract_attention(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import train
    from gipvit import data as D, models as M
    from gipvit.engine import FeatureExtractor
    fd = tmp_path / "feats"
    args = ["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "--img-size", "64", "--tile-size", "64", "-b", "8", "--epochs", "1",
            "--output", str(tmp_path), "--experiment", "fx", "--extract_features", "--synthetic-slides", "3", "--num_tiles", "11",
            "--tiles_per_iter", "4", "--features-dir", str(fd), "--seed", "0"]
    assert train.main(args + ["--extract-attention"]) == 0
    files = sorted(os.listdir(fd))
    assert files == sorted([f"synthetic_{k}_features.pt" for k in range(3)] + [f"synthetic_{k}_attention.pt" for k in range(3)])
    fe = FeatureExtractor("vit_tiny", 64, 32, 2, device=dev)
    fe.load_state(M.init_vit_state("vit_tiny", 64, 2, seed=0))
    slides = {}
    for mb in D.SyntheticSlides(3, 11, 64, 4, seed=0 + 99):
        slides.setdefault(mb["Slide Filename"], []).append(mb["Data"])
    for k in range(3):
        a = torch.load(fd / f"synthetic_{k}_attention.pt", weights_only=True)
        assert a.shape == (11, 3, 17) and a.dtype == torch.float32
        assert float((a.double().sum(-1) - 1).abs().max()) <= 1e-4
        ref = fe.last_selfattention(torch.cat(slides[f"synthetic_{k}"]).to(dev), cls_only=True)[:, :, 0].cpu()
        assert float((a - ref).abs().max()) <= 1e-6
    with pytest.raises(SystemExit):
        train.main([a for a in args if a != "--extract_features"] + ["--extract-attention"])


def test_attention_probs_float16_build(dev):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch\nfrom gipvit import ops\nassert ops.bf16 == torch.float16\n"
            "import test_attention_maps_gpu as t\n"
            "w = t.check_probs(torch.device('cuda:0'), 257, 6, 3, (1, 5, 257))\n"
            "print('F16 PROBS', w)\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, GIPVIT_ACT_FORMAT="f16"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout.strip().splitlines()[-1])
