"""The step and pass configurations of tests/test_poison_gpu.py, shared with tools/poison_spread.py (which measures how far
two CLEAN runs of each lie apart: the gate of the test).  ``run_case(name, dev, before=...)`` builds one engine, loads fixed
weights, runs the case's three steps (or the extractor's call sequence) and returns the recorded quantities as device tensors;
``before()`` is called ahead of every step / call (the poisoned run synchronises and re-poisons there)."""
import functools

import torch

STEPS = 3
K = 1024
SWITCHES = ("fused_ln", "group_dw", "cls_only_last", "fused_mlp", "cls_qlimit", "varlen_attn", "dw_stream", "teacher_side")

# name -> (family, options).  ``env``: variables set before the engine is built (EngineSwitches are read there).
CASES = {}


def _case(name, family, **kw):
    CASES[name] = (family, kw)


# ---- DinoEngine, vit_tiny, 224 / 96 px crops of 256-px tiles, B = 2, K = 1024
_case("dino_tiny_l8", "dino", arch="vit_tiny", n_local=8)
_case("dino_tiny_l0", "dino", arch="vit_tiny", n_local=0)
_case("dino_tiny_micro2", "dino", arch="vit_tiny", n_local=8, micro=2)
_case("dino_tiny_frozen_last", "dino", arch="vit_tiny", n_local=8, train_last_layer=False)
_case("dino_tiny_drop_path_once", "dino", arch="vit_tiny", n_local=8, drop_path=0.3)
_case("dino_tiny_dropout", "dino", arch="vit_tiny", n_local=8, dropout=0.1)
_case("dino_tiny_views", "dino", arch="vit_tiny", n_local=8, views=True)
_case("dino_tiny_fill", "dino", arch="vit_tiny", n_local=8, fill=True)
_case("dino_tiny_fp32", "dino", arch="vit_tiny", n_local=8, precision="fp32")
# ---- DinoEngine, vit_small: fused full-row path, CLS-only tail with q_limit, varlen attention, grouped dW, side stream
_case("dino_small", "dino", arch="vit_small", n_local=8)
for _sw in SWITCHES:
    _case(f"dino_small_no_{_sw}", "dino", arch="vit_small", n_local=8, env={"GIPVIT_" + _sw.upper(): "0"})
_case("dino_base", "dino", arch="vit_base", n_local=8)
# ---- SupervisedEngine, vit_tiny, 64 px, B = 8
_case("sup_plain", "sup")
_case("sup_avg", "sup", eng=dict(global_pool="avg"))
_case("sup_mix", "sup", eng=dict(loss="soft_ce"), mix=True)
_case("sup_erase", "sup", erase=True)
_case("sup_mix_erase", "sup", eng=dict(loss="soft_ce"), mix=True, erase=True)
_case("sup_lamb", "sup", eng=dict(opt="lamb"))
_case("sup_agc", "sup", eng=dict(clip_mode="agc", clip_grad=0.02))
_case("sup_clip_value", "sup", eng=dict(clip_mode="value", clip_grad=1e-3))
_case("sup_layer_decay_ema", "sup", eng=dict(layer_decay=0.75, model_ema_decay=0.99))
_case("sup_dropout", "sup", dropout=0.1)
_case("sup_fp32", "sup", eng=dict(precision="fp32"))
_case("sup_small224", "sup", arch="vit_small", img=224, B=2)
# ---- FeatureExtractor: forward only; 6 tiles at batch 4 make the second batch a padded one over the first one's rows
_case("fx_small256_c2", "fx", arch="vit_small", img=256, B=4, n=6, C=2)
_case("fx_small256_avg", "fx", arch="vit_small", img=256, B=4, n=6, C=2, pool="avg")
_case("fx_tiny272_stream", "fx", arch="vit_tiny", img=272, B=2, n=3, C=0, calls=("run",))
_case("fx_tiny64_fp32", "fx", arch="vit_tiny", img=64, B=4, n=6, C=2, precision="fp32")

FX_CALLS = ("run", "run_with_attention", "last_selfattention", "intermediate_layers", "run")


@functools.lru_cache(maxsize=None)
def _vit_state(arch, img, C, pool="token"):
    from gipvit.models import init_vit_state
    return init_vit_state(arch, img, C, seed=0, global_pool=pool)


@functools.lru_cache(maxsize=None)
def _head_state(D):
    from gipvit.models import init_dino_head_state
    return init_dino_head_state(D, K, seed=1)


@functools.lru_cache(maxsize=None)
def _tiles(n, size, seed):
    from oracle import vit_oracle as vo
    return vo.synth_tiles(n, size, seed=seed)


def _fill_boxes(B, dev):
    """One normalised fill box on tile 1 (gipvit.augment's record: y0, y1, x0, x1, the three values, on)."""
    fill = torch.zeros(B, 8)
    fill[1] = torch.tensor([10., 50., 20., 70., 0.5, -0.25, 1.5, 1.])
    return fill.to(dev)


def _arena_record(out, a):
    for nm in ("p", "m", "v", "t"):
        buf = getattr(a, nm, None)
        if buf is not None:
            out["arena." + nm] = buf.clone()


def _run_dino(dev, before, arch, n_local, micro=1, train_last_layer=True, drop_path=None, dropout=None, views=False, fill=False,
              precision="bf16"):
    from gipvit.engine import ARCHS, DinoEngine
    from gipvit.multicrop import MultiCropSampler, ViewAugmentSampler
    from oracle import vit_oracle as vo
    B = 2
    eng = DinoEngine(arch=arch, img_size=224, out_dim=K, batch=B, n_local=n_local, device=dev, precision=precision)
    eng.load_state(_vit_state(arch, 224, 0), _head_state(ARCHS[arch]["embed_dim"]))
    eng.train_last_layer = train_last_layer
    if drop_path:      # set ONCE: the expanded row factors are carried over the three steps (VitGroup._rs_buf)
        eng.set_drop_path(vo.drop_path_factors(12, (2 + n_local) * B, drop_path, torch.Generator().manual_seed(4)).to(dev))
    crops = MultiCropSampler(B, 256, 2, n_local, seed=2) if views else None
    augs = ViewAugmentSampler(B, 2, n_local, seed=4) if views else None
    out = {}
    for s in range(STEPS):
        batches = [_tiles(B, 256, 100 + micro * s + j).to(dev) for j in range(micro)]
        kw = {}
        if views:
            kw = dict(boxes=crops.sample(dev), views=augs.sample(dev))
        if fill:
            kw = dict(fill=_fill_boxes(B, dev))
        before()
        if dropout:
            eng.set_dropout(dropout, 7000 + s)
        loss = eng.step_micro(batches) if micro > 1 else eng.step(batches[0], **kw)
        torch.cuda.synchronize()
        out[f"loss{s}"] = loss.clone()
    _arena_record(out, eng.arena)
    out["center"] = eng.center.clone()
    return out


def _run_sup(dev, before, arch="vit_tiny", img=64, B=8, eng=None, mix=False, erase=False, dropout=None):
    from gipvit.engine import SupervisedEngine
    from gipvit.erasing import EraseSampler
    from gipvit.mixup import MixSampler
    ekw = dict(eng or {})
    pool = ekw.get("global_pool", "token")
    e = SupervisedEngine(arch=arch, img_size=img, num_classes=2, batch=B, weight_decay=0.05, device=dev, **ekw)
    e.load_state(_vit_state(arch, img, 2, pool))
    mixes = MixSampler(0.8, 1.0, None, 1.0, 0.5, "elem", B, img, seed=11) if mix else None
    erases = EraseSampler(0.75, "rand", 3, B, img, seed=4) if erase else None
    out = {}
    for s in range(STEPS):
        tiles = _tiles(B, img, 200 + s).to(dev)
        tgt = torch.randint(0, 2, (B, 1), generator=torch.Generator().manual_seed(5 + s)).to(dev)
        kw = {}
        if mix:
            kw["mix"] = mixes.sample(dev)
        if erase:
            kw["erase"] = erases.sample(dev)
        before()
        if dropout:
            e.set_dropout(dropout, 7000 + s)
        loss = e.step(tiles, tgt, **kw)
        torch.cuda.synchronize()
        out[f"loss{s}"] = loss.clone()
    _arena_record(out, e.arena)
    return out


def _run_fx(dev, before, arch, img, B, n, C, pool="token", precision="bf16", calls=FX_CALLS):
    from gipvit.engine import FeatureExtractor
    fx = FeatureExtractor(arch=arch, img_size=img, batch=B, num_classes=C, device=dev, precision=precision, global_pool=pool)
    fx.load_state(_vit_state(arch, img, C, pool))
    tiles = _tiles(n, img, 300).to(dev)
    out = {}
    for k, call in enumerate(calls):
        if call == "intermediate_layers" and pool == "avg":
            continue                                  # refused for a mean-pooled model (no final norm)
        before()
        if call == "run":
            res = fx.run(tiles)
        elif call == "run_with_attention":
            res = fx.run_with_attention(tiles)
        elif call == "last_selfattention":
            res = (fx.last_selfattention(tiles, cls_only=False),)
        else:
            res = tuple(fx.intermediate_layers(tiles, n=2))
        torch.cuda.synchronize()
        for j, t in enumerate(res):
            if t is not None:
                out[f"{k}.{call}.{j}"] = t.clone()
    return out


def run_case(name, dev, before=lambda: None, setenv=None):
    """-> {quantity: device tensor}.  ``setenv(name, value)``: how the case's environment switches are set (the test hands in
    monkeypatch.setenv; the caller undoes them)."""
    family, kw = CASES[name]
    kw = dict(kw)
    for var, val in kw.pop("env", {}).items():
        setenv(var, val)
    return {"dino": _run_dino, "sup": _run_sup, "fx": _run_fx}[family](dev, before, **kw)


def spread(a, b, name):
    """The distance the gate is stated in: |a - b| for a loss, ||a - b|| / ||b|| for a buffer."""
    a, b = a.double(), b.double()
    if name.startswith("loss"):
        return float((a - b).abs().max())
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
