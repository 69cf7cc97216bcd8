"""Run by tests/test_dinov2_terms_gpu.py in a process of its own, for what is fixed when the library is loaded or a buffer allocated:

    poison   GIPVIT_POISON=1: two DINO steps with Sinkhorn-Knopp centring and KoLeo, every scratch buffer refilled with NaN in between
    f16      GIPVIT_ACT_FORMAT=f16: the float16 build's KoLeo gradient under a loss scale of 1024

Prints its figures and 'DINOV2 TERMS OK' at the end; any failure is an exception (non-zero exit)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dinov2_terms_cases as C                                   # noqa: E402
from bench import synth_tiles                                    # noqa: E402
from gipvit import engine, ops                                   # noqa: E402
from gipvit.models import init_dino_head_state, init_vit_state   # noqa: E402

dev = torch.device("cuda:0")
K, B, W = 1024, 4, 0.1


def make(**kw):
    eng = engine.DinoEngine(arch="vit_tiny", img_size=224, out_dim=K, batch=B, lr=1e-4, weight_decay=0.04, device=dev,
                            centering="sinkhorn_knopp", koleo_weight=W, **kw)
    eng.load_state(init_vit_state("vit_tiny", 224, 0, seed=0), init_dino_head_state(192, K, seed=1))
    return eng


def poison():
    assert os.environ.get("GIPVIT_POISON") == "1"
    eng = make()
    assert bool(torch.isnan(eng.sk_center).all()) and bool(torch.isnan(eng.koleo_ws).all()), "the new buffers are not poisoned"
    tiles = synth_tiles(B, 256, 99, dev)
    for step in range(2):
        loss = float(eng.step(tiles))
        torch.cuda.synchronize()
        kol = float(eng.koleo)
        print(f"step {step}: loss {loss:.5f} koleo {kol:.5f}")
        assert np.isfinite(loss) and np.isfinite(kol)
        assert bool(torch.isfinite(eng.sk_center).all()) and bool(torch.isfinite(eng.arena.g).all()) and bool(torch.isfinite(eng.arena.p).all())
        assert engine.repoison() > 0


def f16():
    assert ops.bf16 is torch.float16
    eng = make()
    assert eng.scaler is not None
    tiles = synth_tiles(B, 256, 99, dev)
    real, snaps = ops.koleo_bwd, []

    def spy(dfeats, *a, **kw):
        assert kw.get("loss_scale") is not None
        before = dfeats.float().cpu()
        real(dfeats, *a, **kw)
        snaps.append((before, dfeats.float().cpu()))
    ops.koleo_bwd = spy
    try:
        for scale in (1024.0, 1.0):
            eng.scaler.state[0] = scale
            eng.set_hyper()
            eng.forward_backward(tiles)
            torch.cuda.synchronize()
    finally:
        ops.koleo_bwd = real
    rows = eng.G * eng.B
    feats, nn = eng.hb_s.feats.float().cpu().numpy(), eng.koleo_nn.cpu().numpy()
    g64, g32 = C.koleo_grad(feats, eng.G, eng.B, nn), C.koleo_grad(feats, eng.G, eng.B, nn, np.float32)
    bnd = W * C.bound(g32, g64)
    (b_hi, a_hi), (b_lo, a_lo) = snaps
    for scale, before, after in ((1024.0, b_hi, a_hi), (1.0, b_lo, a_lo)):
        added = (after - before).double()[:rows]
        want = scale * W * torch.from_numpy(g64)
        allow = scale * bnd + 2.0 ** -8 * after[:rows].double().abs()
        ratio = float(((added - want).abs() / allow).max())
        print(f"loss scale {scale:g}: max |added| {float(added.abs().max()):.3e}, worst err / bound {ratio:.3f}")
        assert ratio <= 1.0
        assert torch.equal(after[rows:], before[rows:])
    unscaled = (a_lo - b_lo).double()[:rows]
    scaled = (a_hi - b_hi).double()[:rows]
    allow = 1024.0 * (bnd + 2.0 ** -8 * a_lo[:rows].double().abs()) + 2.0 ** -8 * a_hi[:rows].double().abs()
    ratio = float(((scaled - 1024.0 * unscaled).abs() / allow).max())
    print(f"1024 x the unscaled part: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0


{"poison": poison, "f16": f16}[sys.argv[1]]()
print("DINOV2 TERMS OK")
