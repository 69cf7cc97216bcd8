"""CPU: ``--gp avg`` (timm global_pool='avg': the final norm is Identity, the mean of the patch tokens goes through fc_norm) on the
host side -- parameter specs, layer decay, checkpoint loading, the CLI, the launch sequence of a mean-pooled engine, and the
contracts of gv_token_mean_fwd / gv_token_mean_bwd as assertion functions that tests/test_global_pool_gpu.py applies to the
kernels and that are shown here to reject four faults of a numpy model.

This module owns the reference of the mean-pooled model: ``avg_logits`` is built from the oracle's public ``prepare_tokens``,
``block`` and ``layer_norm``; gradients come from autograd; ``fp64=True`` computes in float64."""
import os
import sys

import numpy as np
import pytest
import torch

import launch_trace as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- #
# the reference
# --------------------------------------------------------------------------- #
def avg_params(arch, img_size, num_classes=2, seed=0, dtype=torch.float32):
    """The oracle's seeded ViT parameters as a mean-pooled model's: ``norm.*`` gone, ``fc_norm.*`` in its place, with a
    non-trivial gamma / beta so that their gradients and the scaling of dpool are exercised."""
    from oracle import vit_oracle as vo
    src = vo.init_vit(arch, img_size, num_classes, seed, dtype)
    D = vo.ARCHS[arch]["embed_dim"]
    g = torch.Generator().manual_seed(seed + 1000)
    p = type(src)()
    for k, v in src.items():
        if k == "norm.weight":
            p["fc_norm.weight"] = (1.0 + 0.2 * torch.randn(D, generator=g)).to(dtype)
        elif k == "norm.bias":
            p["fc_norm.bias"] = (0.1 * torch.randn(D, generator=g)).to(dtype)
        else:
            p[k] = v
    return p


def avg_features(p, x, arch, drop=None, dropout=None):
    """tokens after the last block -> mean of the patch tokens (the CLS row excluded) -> fc_norm."""
    from oracle import vit_oracle as vo
    a = vo.ARCHS[arch]
    t = vo._drop(vo.prepare_tokens(x, p), dropout, 0, 0)
    for i in range(a["depth"]):
        t = vo.block(t, p, i, a["num_heads"], None if drop is None else drop[i], dropout)
    return vo.layer_norm(t[:, 1:].mean(1), p["fc_norm.weight"], p["fc_norm.bias"])


def avg_logits(p, x, arch, drop=None, dropout=None, fp64=False):
    """The classifier on the pooled, normalised feature.  ``fp64``: parameters and input are taken to float64 first."""
    if fp64:
        p = {k: v.double() for k, v in p.items()}
        x = x.double()
    return avg_features(p, x, arch, drop, dropout) @ p["head.weight"].t() + p["head.bias"]


def avg_forward_backward(p, tiles_u8, target, arch, img_size, smoothing=0.1, drop=None, dropout=None, fp64=False):
    """One supervised forward / backward of the mean-pooled model (softmax -> LabelSmoothingCE, as SupervisedOracle) ->
    (loss, {name: gradient}, logits)."""
    from oracle import vit_oracle as vo
    dt = torch.float64 if fp64 else torch.float32
    x = vo.normalize_window(tiles_u8, (0, 0, img_size), dtype=dt)
    sp = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in p.items()}
    logits = avg_logits(sp, x, arch, drop=drop, dropout=None if dropout is None else (dropout[0], dropout[1], 0))
    loss = vo.softmax_lsce(logits, target, smoothing)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in sp.items()}, logits.detach()


# --------------------------------------------------------------------------- #
# the kernels' contracts
# --------------------------------------------------------------------------- #
ACT_MANT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}     # mantissa bits, smallest normal exponent


def ulp(v, dtype):
    """Spacing of ``dtype`` at |v| (float64 array): 2^(e - mantissa bits), e clamped at the smallest normal exponent."""
    m, emin = ACT_MANT[dtype]
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where(a > 0, np.maximum(e, emin), emin)
    return np.exp2(e - m)


def assert_pool_fwd(pooled, x, n_img, N):
    """pooled f32 [n_img, D] against the float64 mean of rows 1 .. N-1 of x f32 [n_img * N, D]:
    |pooled - ref| <= (N - 1) 2^-24 mean_rows|x| + 2^-24 |ref| per element (recursive summation in any fixed order, then one
    rounded division)."""
    D = x.shape[1]
    xs = x.double().view(n_img, N, D)[:, 1:]
    ref = xs.mean(1)
    bound = (N - 1) * 2.0 ** -24 * xs.abs().mean(1) + 2.0 ** -24 * ref.abs()
    err = (pooled.double() - ref).abs()
    worst = float((err - bound).max())
    assert tuple(pooled.shape) == (n_img, D) and worst <= 0, f"pooled mean: error exceeds the summation bound by {worst:.3e} (max err {float(err.max()):.3e})"
    return float((err / bound.clamp_min(1e-300)).max())


def assert_pool_bwd(g, gb, dpool, scale, n_img, N):
    """g f32 / gb (16-bit or f32) [n_img * N, D] against dpool f32 [n_img, D] and the per-image factors ``scale`` (None = 1)."""
    D = dpool.shape[1]
    g3, gb3 = g.view(n_img, N, D), gb.view(n_img, N, D)
    assert g.dtype == torch.float32 and bool((g3[:, 0] == 0).all()) and bool((gb3[:, 0] == 0).all()), "the CLS row's gradient must be exactly zero"
    assert torch.equal(g3[:, 1:], g3[:, 1:2].expand(-1, N - 1, -1)), "g: every patch row of an image must equal its row 1 bitwise"
    assert torch.equal(gb3[:, 1:], gb3[:, 1:2].expand(-1, N - 1, -1)), "gb: every patch row of an image must equal its row 1 bitwise"
    ref = dpool.double().numpy() / (N - 1)
    err = np.abs(g3[:, 1].double().numpy() - ref)
    assert (err <= 2 * ulp(ref, torch.float32)).all(), f"g row 1: {float((err / ulp(ref, torch.float32)).max()):.2f} f32 ulp from dpool / (N - 1)"
    s = np.ones((n_img, 1)) if scale is None else scale.double().numpy().reshape(n_img, 1)
    refb = g3[:, 1].double().numpy() * s
    errb = np.abs(gb3[:, 1].double().numpy() - refb)
    assert (errb <= ulp(refb, gb.dtype)).all(), f"gb row 1: {float((errb / ulp(refb, gb.dtype)).max()):.2f} ulp of {gb.dtype} from g * gb_scale"


def model_pool_fwd(x, n_img, N, fault=None):
    """numpy model of gv_token_mean_fwd's contract: f32 recursive summation over the patch rows, one f32 division."""
    xs = x.numpy().reshape(n_img, N, -1)
    acc = np.zeros((n_img, xs.shape[2]), np.float32)
    for t in range(0 if fault == "cls_in_mean" else 1, N):
        acc = (acc + xs[:, t]).astype(np.float32)
    return torch.from_numpy((acc / np.float32(N if fault == "div_by_n" else N - 1)).astype(np.float32))


def model_pool_bwd(dpool, scale, n_img, N, act, fault=None):
    """numpy / torch model of gv_token_mean_bwd's contract -> (g, gb)."""
    D = dpool.shape[1]
    row = (dpool.numpy() / np.float32(N if fault == "div_by_n" else N - 1)).astype(np.float32)
    g = torch.from_numpy(np.repeat(row[:, None, :], N, axis=1).copy())
    s = torch.ones(n_img) if scale is None else scale.clone()
    if fault == "neighbour_scale":
        s = s.roll(1)
    gb = (g * s.view(n_img, 1, 1)).to(act)
    if fault != "cls_grad":
        g[:, 0] = 0
        gb[:, 0] = 0
    return g.view(n_img * N, D), gb.view(n_img * N, D)


def pool_case(n_img, N, D, seed=0):
    """Inputs of one kernel-level case: x with a large CLS row and a per-column offset (a mean that forgets to skip row 0 or
    divides by N is far off), dpool, distinct per-image factors."""
    g = torch.Generator().manual_seed(seed + 7919 * N + D)
    x = torch.randn(n_img, N, D, generator=g) + torch.linspace(-2, 2, D)
    x[:, 0] = 50.0 + torch.randn(n_img, D, generator=g)
    dpool = torch.randn(n_img, D, generator=g) * 3.0
    scale = 0.5 + 0.37 * torch.arange(1, n_img + 1, dtype=torch.float32)
    return x.view(n_img * N, D).contiguous(), dpool, scale


@pytest.mark.parametrize("act", [torch.bfloat16, torch.float16, torch.float32])
def test_contract_model_passes_and_each_fault_is_rejected(act):
    n_img, N, D = 3, 17, 192
    x, dpool, scale = pool_case(n_img, N, D)
    assert_pool_fwd(model_pool_fwd(x, n_img, N), x, n_img, N)
    for sc in (scale, None):
        assert_pool_bwd(*model_pool_bwd(dpool, sc, n_img, N, act), dpool, sc, n_img, N)
    for fault in ("cls_in_mean", "div_by_n"):
        with pytest.raises(AssertionError, match="summation bound"):
            assert_pool_fwd(model_pool_fwd(x, n_img, N, fault), x, n_img, N)
    for fault, msg in (("div_by_n", "f32 ulp from dpool"), ("cls_grad", "exactly zero"), ("neighbour_scale", "from g \\* gb_scale")):
        with pytest.raises(AssertionError, match=msg):
            assert_pool_bwd(*model_pool_bwd(dpool, scale, n_img, N, act, fault), dpool, scale, n_img, N)


# --------------------------------------------------------------------------- #
# specs, layer decay, checkpoints
# --------------------------------------------------------------------------- #
def test_specs_replace_norm_by_fc_norm_in_place():
    from gipvit.engine import Arena, no_weight_decay, vit_param_specs
    tok, avg = vit_param_specs("vit_tiny", 64, 2), vit_param_specs("vit_tiny", 64, 2, "avg")
    assert list(vit_param_specs("vit_tiny", 64, 2, "token").items()) == list(tok.items())
    assert "norm.weight" in tok and "norm.bias" in tok and not any(k.startswith("fc_norm") for k in tok)
    # the default spec, key for key: the stem, 12 keys per block, the final norm, the head
    assert list(tok)[:4] == ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    assert list(tok)[-4:] == ["norm.weight", "norm.bias", "head.weight", "head.bias"] and len(tok) == 4 + 12 * 12 + 4
    assert [k.replace("fc_norm.", "norm.") for k in avg] == list(tok) and [avg[k] for k in avg] == [tok[k] for k in tok]
    assert "fc_norm.weight" in avg and "fc_norm.bias" in avg and "norm.weight" not in avg and "norm.bias" not in avg
    assert no_weight_decay("fc_norm.weight", avg["fc_norm.weight"]) and no_weight_decay("fc_norm.bias", avg["fc_norm.bias"])
    a_t, a_a = Arena(tok, "cpu", False), Arena(avg, "cpu", False)
    assert a_a.n == a_t.n and a_a.n_decay == a_t.n_decay and a_a.off["fc_norm.weight"] == a_t.off["norm.weight"] >= a_t.n_decay
    for bad in ("", "max", "avgmax"):
        with pytest.raises(ValueError, match="global_pool"):
            vit_param_specs("vit_tiny", 64, 2, bad)


def test_layer_decay_puts_fc_norm_with_the_head():
    from gipvit.engine import Arena, vit_param_specs
    from gipvit.layer_decay import LayerDecayPlan, layer_id
    assert layer_id("fc_norm.weight", 12) == layer_id("head.weight", 12) == 14 and layer_id("norm.weight", 12) == 13
    plan = LayerDecayPlan(Arena(vit_param_specs("vit_tiny", 64, 2, "avg"), "cpu", False), 12, 0.75)
    for n in ("fc_norm.weight", "fc_norm.bias", "head.weight", "head.bias"):
        assert plan.scales[n] == 1.0, n
    assert plan.scales["blocks.11.mlp.fc2.weight"] == 0.75 ** 2 and plan.scales["cls_token"] == 0.75 ** 14
    # no parameter is left in the final norm's layer: the mean over the (layer, decay) groups has one scale-0.75 group fewer
    tok = LayerDecayPlan(Arena(vit_param_specs("vit_tiny", 64, 2), "cpu", False), 12, 0.75)
    assert len(tok.group_scales) == len(plan.group_scales) + 1 and abs(sum(tok.group_scales) - sum(plan.group_scales) - 0.75) < 1e-12
    assert plan.mean_lr(2.0) == 2.0 * sum(plan.group_scales) / len(plan.group_scales)


def test_checkpoint_loading_between_token_and_avg_models(tmp_path, capsys):
    from gipvit import models as M
    tok = M.init_vit_state("vit_tiny", 64, 2, seed=3)
    avg = M.init_vit_state("vit_tiny", 64, 2, seed=3, global_pool="avg")
    assert all(torch.equal(avg[k], tok[k]) for k in tok if not k.startswith("norm."))         # the same draws elsewhere
    tok["norm.weight"] = torch.full((192,), 1.5); tok["norm.bias"] = torch.full((192,), 0.25)
    avg["fc_norm.weight"] = torch.full((192,), 0.75); avg["fc_norm.bias"] = torch.full((192,), -0.5)
    torch.save({"state_dict": tok}, tmp_path / "tok.pth.tar")
    torch.save({"state_dict": {"module." + k: v for k, v in avg.items()}}, tmp_path / "avg.pth.tar")
    # token-style file -> avg model (the fine-tuning case): norm.* dropped, fc_norm at (1, 0), one notice
    capsys.readouterr()
    got = M.load_encoder_checkpoint(str(tmp_path / "tok.pth.tar"), "vit_tiny", 64, 2, "avg")
    note = capsys.readouterr().out
    assert note.count("\n") == 1 and "fc_norm" in note and "norm.*" in note
    assert "norm.weight" not in got and bool((got["fc_norm.weight"] == 1).all()) and bool((got["fc_norm.bias"] == 0).all())
    assert all(torch.equal(got[k], tok[k]) for k in got if not k.startswith("fc_norm."))
    # avg file -> avg model: fc_norm.* loaded, nothing printed
    got = M.load_encoder_checkpoint(str(tmp_path / "avg.pth.tar"), "vit_tiny", 64, 2, "avg")
    assert capsys.readouterr().out == "" and list(got) == list(avg) and all(torch.equal(got[k], avg[k]) for k in avg)
    # avg file -> token model: there is no final norm to load
    with pytest.raises(KeyError, match="norm.weight"):
        M.load_encoder_checkpoint(str(tmp_path / "avg.pth.tar"), "vit_tiny", 64, 2)
    # token file -> token model: unchanged
    got = M.load_encoder_checkpoint(str(tmp_path / "tok.pth.tar"), "vit_tiny", 64, 2)
    assert list(got) == list(tok) and all(torch.equal(got[k], tok[k]) for k in tok)


def test_state_dict_round_trip_follows_the_specs():
    from gipvit import models as M
    from gipvit.engine import SupervisedEngine
    with lt.recording():           # (loading refreshes the 16-bit weight copy: a launch, recorded instead of run)
        eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=2, device="cpu", global_pool="avg", model_ema_decay=0.9)
        st = M.init_vit_state("vit_tiny", 64, 2, seed=5, global_pool="avg")
        st["fc_norm.weight"] = torch.full((192,), 0.75); st["fc_norm.bias"] = torch.full((192,), -0.5)
        ema = {k: v + 1.0 for k, v in st.items()}
        eng.load_state(st, ema)
        model = M.VitModel(eng, "vit_tiny")
        sd = model.state_dict()
        assert list(sd) == list(st) and all(torch.equal(sd[k], st[k]) for k in st)
        assert all(torch.equal(v, ema[k]) for k, v in eng.state_dict(ema=True).items())          # --resume restores the EMA copy too
        assert {n for n, _ in model.named_parameters()} == set(st)
        sd["fc_norm.bias"] = torch.full((192,), 2.0)
        assert model.load_state_dict(sd) == ([], [])
        assert bool((eng.W.f("fc_norm.bias") == 2.0).all())
        with pytest.raises(KeyError, match="fc_norm"):
            model.load_state_dict(M.init_vit_state("vit_tiny", 64, 2, seed=5))                    # a token state dict: strict


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def test_cli_accepts_token_and_avg_and_refuses_the_rest():
    sys.path.insert(0, ROOT)
    import train
    from gipvit.cli_spec import REFERENCE_FLAGS
    from gipvit.engine import SupervisedEngine, FeatureExtractor
    assert [e["used"] for e in REFERENCE_FLAGS if e["flags"] == ["--gp"]] == [True]
    for ok in (["--gp", "avg"], ["--gp", "token"], []):
        args, _ = train.parse_args(["--model", "vit_tiny"] + ok)
        train.check_supported(args, lambda m: None)
    for bad in (["--gp", "max"], ["--gp", ""], ["--gp", "avg", "--dino"]):
        args, _ = train.parse_args(["--model", "vit_tiny"] + bad)
        with pytest.raises(SystemExit, match="--gp"):
            train.check_supported(args, lambda m: None)
    args, _ = train.parse_args(["--model", "vit_tiny", "--gp", "token", "--dino"])
    train.check_supported(args, lambda m: None)
    for bad in ("", "max"):
        with pytest.raises(ValueError, match="global_pool"):
            SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=2, device="cpu", global_pool=bad)
        with pytest.raises(ValueError, match="global_pool"):
            FeatureExtractor(arch="vit_tiny", img_size=64, batch=2, device="cpu", global_pool=bad)
    assert SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=2, device="cpu", global_pool=None).pool == "token"
    # an extractor over another model's weights must agree with them about the pooling
    eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=2, device="cpu", global_pool="avg")
    with pytest.raises(ValueError, match="global_pool"):
        FeatureExtractor("vit_tiny", 64, 2, 0, device="cpu", weights=eng.W)
    fx = FeatureExtractor("vit_tiny", 64, 2, 0, device="cpu", weights=eng.W, global_pool="avg")
    with pytest.raises(ValueError, match="no"):
        fx.intermediate_layers(torch.zeros(2, 64, 64, 3, dtype=torch.uint8))


# --------------------------------------------------------------------------- #
# launch sequence
# --------------------------------------------------------------------------- #
def _trace_step(arch, pool, **kw):
    from gipvit import engine
    calls = []
    saved = engine.VitGroup.gather_cls, engine.VitGroup.scatter_cls
    engine.VitGroup.gather_cls = lambda self, *a: calls.append("gather_cls")
    engine.VitGroup.scatter_cls = lambda self, *a: calls.append("scatter_cls")
    try:
        with lt.recording() as rec:
            eng = engine.SupervisedEngine(arch=arch, img_size=64, num_classes=2, batch=2, device="cpu", global_pool=pool, **kw)
            eng.step(torch.zeros(2, 64, 64, 3, dtype=torch.uint8), torch.zeros(2, 1, dtype=torch.int64))
    finally:
        engine.VitGroup.gather_cls, engine.VitGroup.scatter_cls = saved
    return eng, rec.events, calls


@pytest.mark.parametrize("arch", ["vit_tiny", "vit_small"])
def test_avg_engine_launches_one_pool_each_way_and_no_cls_tail(arch):
    eng, events, calls = _trace_step(arch, "avg")
    names = [e[0] for e in events]
    assert names.count("token_mean_fwd") == 1 and names.count("token_mean_bwd") == 1
    attn = [e for e in events if e[0].startswith("attention")]
    assert len(attn) == 24 and all(e[2].get("q_limit", 0) == 0 for e in attn)
    assert calls == [] and "gather_cls" not in names
    assert eng.vit.fused == (arch == "vit_small") and names.count("linear_ln_fwd") == (24 if arch == "vit_small" else 0)
    # the pool sits between the last block and fc_norm's LayerNorm; the backward opens with that norm's backward (no dY buffer: the
    # pooled gradient is its residual output), its finalize into fc_norm.* and the last mlp.fc2.bias, then the spread
    k = names.index("token_mean_fwd")
    assert names[k + 1] == "layernorm_fwd" and names[k + 2] == "small_matmul"
    k = names.index("token_mean_bwd")
    assert names[k - 2:k] == ["layernorm_bwd", "ln_finalize"] and events[k - 2][1][6] is None
    a = eng.arena
    outs = [x["tensor"][1] for x in events[k - 1][1][3:6]]
    assert outs == [a.off["fc_norm.weight"], a.off["fc_norm.bias"], a.off["blocks.11.mlp.fc2.bias"]]
    # both backward buffers are fully written by the spread: the only fill of the step is the gradient arena's
    zeros = [e for e in events if e[0] == "Tensor.zero_"]
    assert len(zeros) == 1 and zeros[0][1][0]["tensor"][2] == [a.n]
    # the spread writes the residual gradient and the dY buffer of the last block's MLP half, whole
    T, D = eng.grp.T, eng.D
    assert [x["tensor"][2] for x in events[k][1][:3]] == [[2, D], [T, D], [T, D]]


def test_token_engine_trace_has_no_pool_launch():
    eng, events, calls = _trace_step("vit_tiny", "token")
    names = [e[0] for e in events]
    assert "token_mean_fwd" not in names and "token_mean_bwd" not in names and calls.count("gather_cls") == 2
    assert any(e[2].get("q_limit", 0) == 1 for e in events if e[0].startswith("attention"))


def test_avg_engine_with_dropout_takes_the_bias_gradient_from_the_masked_dy():
    from gipvit import engine
    with lt.recording() as rec:
        eng = engine.SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=2, device="cpu", global_pool="avg")
        eng.set_dropout(0.1, 7)
        eng.set_drop_path(torch.ones(12, 2, 2))
        eng.step(torch.zeros(2, 64, 64, 3, dtype=torch.uint8), torch.zeros(2, 1, dtype=torch.int64))
    names = [e[0] for e in rec.events]
    k = names.index("token_mean_bwd")
    assert rec.events[k - 1][0] == "ln_finalize" and rec.events[k - 1][1][5] is None            # no third sum under --drop ...
    assert names[k + 1:k + 3] == ["dropout", "colsum"]                                          # ... the masked dY's column sum instead
    assert rec.events[k + 2][1][4]["tensor"][1] == eng.arena.off["blocks.11.mlp.fc2.bias"]
    assert rec.events[k][2]["gb_scale"] is not None and rec.events[k - 2][2]["gb_scale"] is not None
