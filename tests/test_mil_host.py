"""CPU: the attention-MIL probe's specification and host side.

* ``mil_reference`` / ``mil_predict_reference``: the whole procedure in plain torch (autograd + torch.optim.Adam), fp64 by default;
  a hand-derived backward following the issue's formulas agrees with autograd to 1e-12.  The GPU tests (tests/test_mil_gpu.py)
  hold gv_mil_train / gv_mil_predict to these.
* well-posedness of the shared cases: Adam divides by sqrt(v), so a gradient of rounding-noise size is amplified.  Every case is
  also run through the same reference in torch f32; ``gap32`` = max |f32 - f64| over the parameters must stay <= 2e-5.  That is a
  condition on the inputs (seeds, scales, rates), checked here, and exported per case for the GPU file's parameter bound.
* host helpers (bag_table, init_params, mil_metrics, state_dict), struct layouts against gcc, the entry points' refusals through
  the ABI without a GPU, the driver's --mil-* flags, --eval-metric resolution and column order.
* learnability: on "needle" bags the reference reaches slide AUC 1.0 and puts most of a positive bag's attention on its needles."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8

# F, L, C, batch, bag sizes, epochs, ldx, seed, lr, wd.  Together: F in {4, 36, 192, 388}, L in {16, 128, 256}, C in {1, 2, 3},
# batch in {1, 3, 8}, bag sizes from {1, 2, 63, 64, 65, 129, 500}, a last partial step wherever batch > 1, ldx > F once.
# Every case has weight decay: the softmax over a bag is invariant to a shift of its scores, so the loss gradient of the score
# bias bw is exactly zero, and without the decay term Adam would divide f32 rounding noise by its own size (measured: gap32
# 1.9e-4 on bw alone in the last case at wd = 0, 4e-8 with it).  Steps without decay are covered by the exact probes of the GPU file.
CASES = [
    dict(F=4, L=16, C=1, batch=1, sizes=[1, 2, 63], epochs=2, ldx=4, seed=0, lr=1e-3, wd=1e-4),
    dict(F=36, L=128, C=2, batch=3, sizes=[64, 65, 1, 129, 2, 63, 64], epochs=3, ldx=40, seed=1, lr=1e-3, wd=1e-4),
    dict(F=192, L=256, C=3, batch=8, sizes=[500, 129, 65, 64, 63, 2, 1, 129, 65, 64, 2], epochs=2, ldx=192, seed=2, lr=5e-4, wd=1e-4),
    dict(F=388, L=16, C=2, batch=3, sizes=[65, 129, 2, 63, 1], epochs=2, ldx=388, seed=3, lr=5e-4, wd=1e-4),
]
CASE_IDS = ["F%d-L%d-C%d-B%d" % (c["F"], c["L"], c["C"], c["batch"]) for c in CASES]
NAMES = ["attention_V.weight", "attention_V.bias", "attention_U.weight", "attention_U.bias", "attention_w.weight", "attention_w.bias",
         "classifier.weight", "classifier.bias"]


def cosine_scale(e, epochs):
    return 0.5 * (1.0 + math.cos(math.pi * e / epochs))


def draw_params(L, C, F, seed):
    """nn.Linear-style U(-1/sqrt(fan_in), 1/sqrt(fan_in)) f32 tensors under NAMES (torch generator: the tests' own draw)."""
    g = torch.Generator().manual_seed(seed + 500)
    shapes = [(L, F), (L,), (L, F), (L,), (1, L), (1,), (C, F), (C,)]
    out = {}
    for name, shape in zip(NAMES, shapes):
        bound = 1.0 / math.sqrt(L if name.startswith("attention_w") else F)
        out[name] = (torch.rand(shape, generator=g) * 2 - 1) * bound
    return out


def pack(params, L, C, F):
    """NAMES-keyed tensors -> the packed vector of include/gipvit.h: VU | Wc | bv | bu | w | bc | bw."""
    return torch.cat([params["attention_V.weight"].reshape(-1), params["attention_U.weight"].reshape(-1), params["classifier.weight"].reshape(-1),
                      params["attention_V.bias"], params["attention_U.bias"], params["attention_w.weight"].reshape(-1), params["classifier.bias"],
                      params["attention_w.bias"]])


def case_setup(case):
    """-> dict of a case's inputs: x f32 [N, F], ptr int64 [n + 1], labels int64 [n], params0 (NAMES), perms [epochs, n]."""
    F, C, sizes, seed = case["F"], case["C"], case["sizes"], case["seed"]
    g = torch.Generator().manual_seed(seed)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = torch.randn(int(ptr[-1]), F, generator=g)
    labels = torch.tensor([i % C for i in range(len(sizes))], dtype=torch.int64)
    for b in range(len(sizes)):                      # a class direction on the bag's first row, so that there is something to learn
        x[ptr[b], labels[b] % F] += 2.0
    rng = np.random.Generator(np.random.PCG64(seed))
    perms = np.stack([rng.permutation(len(sizes)) for _ in range(case["epochs"])])
    return dict(x=x, ptr=ptr, labels=labels, params0=draw_params(case["L"], C, F, seed), perms=perms)


def mil_forward(P, xb):
    """One bag: rows xb [n, F] -> (logits [C], a [n], s [n])."""
    t = torch.tanh(xb @ P["attention_V.weight"].t() + P["attention_V.bias"])
    g = torch.sigmoid(xb @ P["attention_U.weight"].t() + P["attention_U.bias"])
    s = (t * g) @ P["attention_w.weight"].reshape(-1) + P["attention_w.bias"]
    a = torch.softmax(s, dim=0)
    z = a @ xb
    return P["classifier.weight"] @ z + P["classifier.bias"], a, s


def mil_reference(x, ptr, labels, params0, perms, batch, lr, wd, dtype=torch.float64):
    """torch.optim.Adam(lr * cosine factor, (0.9, 0.999), 1e-8, weight_decay=wd) over the model under the mean cross-entropy of a
    step's bags, the bags of an epoch visited in perms[e]'s order ``batch`` at a time.
    -> (params, m, v: NAMES-keyed dicts, epoch_loss [epochs] = mean -log p[label] over the epoch's bags), all ``dtype``."""
    P = {k: v.clone().to(dtype).requires_grad_(True) for k, v in params0.items()}
    opt = torch.optim.Adam(list(P.values()), lr=lr, betas=(BETA1, BETA2), eps=EPS, weight_decay=wd)
    xd = x.to(dtype)
    epochs = len(perms)
    epoch_loss = torch.zeros(epochs, dtype=dtype)
    for e in range(epochs):
        for grp in opt.param_groups:
            grp["lr"] = lr * cosine_scale(e, epochs)
        for s0 in range(0, len(perms[e]), batch):
            step = [int(b) for b in perms[e][s0:s0 + batch]]
            opt.zero_grad()
            total = 0.0
            for b in step:
                logits, _, _ = mil_forward(P, xd[ptr[b]:ptr[b + 1]])
                total = total + torch.nn.functional.cross_entropy(logits[None], labels[b:b + 1], reduction="sum")
            epoch_loss[e] += total.detach()
            (total / len(step)).backward()
            opt.step()
        epoch_loss[e] /= len(perms[e])
    st = lambda key: {k: opt.state[p][key].detach() if p in opt.state else torch.zeros_like(p) for k, p in P.items()}
    return {k: v.detach() for k, v in P.items()}, st("exp_avg"), st("exp_avg_sq"), epoch_loss


def mil_predict_reference(params, x, ptr, labels=None, dtype=torch.float64):
    """-> (prob [n, C], attn [N], score [N], loss = sum of -log p[label] or None), ``dtype``."""
    P = {k: v.to(dtype) for k, v in params.items()}
    xd = x.to(dtype)
    prob, attn, score = [], [], []
    for b in range(len(ptr) - 1):
        logits, a, s = mil_forward(P, xd[ptr[b]:ptr[b + 1]])
        prob.append(torch.softmax(logits, dim=0)); attn.append(a); score.append(s)
    prob = torch.stack(prob)
    loss = None if labels is None else -torch.log(prob[torch.arange(len(labels)), labels]).sum()
    return prob, torch.cat(attn), torch.cat(score), loss


def mil_hand_gradients(P, xs, ys):
    """The issue's backward formulas written out for one step over the bags xs (list of [n, F]) with labels ys -> NAMES-keyed."""
    V, bv, U, bu = P["attention_V.weight"], P["attention_V.bias"], P["attention_U.weight"], P["attention_U.bias"]
    w, Wc = P["attention_w.weight"].reshape(-1), P["classifier.weight"]
    m = len(xs)
    G = {k: torch.zeros_like(v) for k, v in P.items()}
    for xb, y in zip(xs, ys):
        t = torch.tanh(xb @ V.t() + bv)
        g = torch.sigmoid(xb @ U.t() + bu)
        u = t * g
        a = torch.softmax(u @ w + P["attention_w.bias"], dim=0)
        z = a @ xb
        p = torch.softmax(Wc @ z + P["classifier.bias"], dim=0)
        dl = p.clone()
        dl[y] -= 1.0
        dl /= m
        G["classifier.weight"] += torch.outer(dl, z)
        G["classifier.bias"] += dl
        da = xb @ (Wc.t() @ dl)
        ds = a * (da - (a * da).sum())
        G["attention_w.bias"] += ds.sum()
        G["attention_w.weight"] += (ds @ u)[None]
        dt = ds[:, None] * w * g * (1 - t * t)
        dg = ds[:, None] * w * t * g * (1 - g)
        G["attention_V.weight"] += dt.t() @ xb
        G["attention_V.bias"] += dt.sum(0)
        G["attention_U.weight"] += dg.t() @ xb
        G["attention_U.bias"] += dg.sum(0)
    return G


_ref_cache = {}


def case_reference(i):
    """(setup, f64 reference, gap32) of case i, computed once and shared by the tests of both files (never modified)."""
    if i not in _ref_cache:
        c, s = CASES[i], case_setup(CASES[i])
        kw = dict(x=s["x"], ptr=s["ptr"], labels=s["labels"], params0=s["params0"], perms=s["perms"], batch=c["batch"], lr=c["lr"], wd=c["wd"])
        ref = mil_reference(**kw)
        r32 = mil_reference(dtype=torch.float32, **kw)
        gaps = {k: float((r32[0][k].double() - ref[0][k]).abs().max()) for k in NAMES}
        _ref_cache[i] = (s, ref, max(gaps.values()), gaps)
    return _ref_cache[i]


def gap32(i):
    return case_reference(i)[2]


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_cases_are_well_posed(i):
    s, (P, m, v, loss), gap, gaps = case_reference(i)
    print(f"gap32 {gap:.3e} per tensor {{{', '.join(f'{k}: {g:.1e}' for k, g in gaps.items())}}}; f64 epoch losses {[round(float(x), 5) for x in loss]}")
    assert gap <= 2e-5
    assert all(bool(torch.isfinite(t).all()) for t in P.values()) and bool(torch.isfinite(loss).all())
    if CASES[i]["C"] > 1:
        assert float(loss[-1]) < float(loss[0])


def test_hand_backward_agrees_with_autograd():
    s = case_setup(CASES[1])
    P = {k: v.double().requires_grad_(True) for k, v in s["params0"].items()}
    xd, ptr, labels = s["x"].double(), s["ptr"], s["labels"]
    step = [0, 2, 3]
    total = sum(torch.nn.functional.cross_entropy(mil_forward(P, xd[ptr[b]:ptr[b + 1]])[0][None], labels[b:b + 1]) for b in step) / len(step)
    total.backward()
    with torch.no_grad():
        G = mil_hand_gradients({k: v.detach() for k, v in P.items()}, [xd[ptr[b]:ptr[b + 1]] for b in step], [int(labels[b]) for b in step])
    for k in NAMES:
        assert float((G[k] - P[k].grad).abs().max()) <= 1e-12, k


def test_reference_first_step_is_adam_by_hand():
    s, c = case_setup(CASES[3]), CASES[3]
    P, m, v, _ = mil_reference(s["x"], s["ptr"], s["labels"], s["params0"], np.array([[0, 1, 2]]), 3, c["lr"], 1e-2)
    P0 = {k: t.double() for k, t in s["params0"].items()}
    xd, ptr = s["x"].double(), s["ptr"]
    G = mil_hand_gradients(P0, [xd[ptr[b]:ptr[b + 1]] for b in range(3)], [int(s["labels"][b]) for b in range(3)])
    for k in NAMES:
        g = G[k] + 1e-2 * P0[k]                      # coupled weight decay
        assert float((m[k] - (1 - BETA1) * g).abs().max()) <= 1e-15 and float((v[k] - (1 - BETA2) * g * g).abs().max()) <= 1e-15
        want = P0[k] - c["lr"] * g / (g.abs() + EPS)  # m-hat / (sqrt(v-hat) + eps) at step 1, cosine factor 1
        assert float((P[k] - want).abs().max()) <= 1e-12, k


# ---- host helpers
def test_bag_table():
    from gipvit.mil import bag_table
    assert bag_table([0, 0, 0, 2, 2, 5]).tolist() == [0, 3, 5, 6] and bag_table([7]).tolist() == [0, 1]
    assert bag_table(np.array([3, 3, 4])).dtype == np.int32
    with pytest.raises(ValueError):
        bag_table([0, 1, 0])
    with pytest.raises(ValueError):
        bag_table([])


def test_init_params_depend_on_the_seed_only():
    from gipvit.mil import init_params, param_count, param_views
    L, C, F = 32, 3, 20
    a, b = init_params(L, C, F, 5), init_params(L, C, F, 5)
    assert a.dtype == torch.float32 and a.shape == (param_count(L, C, F),) and torch.equal(a, b) and not torch.equal(a, init_params(L, C, F, 6))
    views = param_views(a, L, C, F)
    assert list(views) == NAMES
    for k, (name, t) in enumerate(views.items()):
        bound = 1.0 / math.sqrt(L if name.startswith("attention_w") else F)
        assert float(t.abs().max()) <= bound
        want = np.random.Generator(np.random.PCG64([5, k])).uniform(-bound, bound, size=tuple(t.shape)).astype(np.float32)
        assert np.array_equal(t.numpy(), want), name
    assert abs(float(views["attention_V.weight"].std()) - (1 / math.sqrt(F)) / math.sqrt(3)) < 0.02
    # the views tile the vector exactly as the packed layout says
    P = {n: torch.full(tuple(t.shape), float(k + 1)) for k, (n, t) in enumerate(views.items())}
    packed = pack(P, L, C, F)
    assert all(bool((t == k + 1).all()) for k, t in enumerate(param_views(packed, L, C, F).values()))


def test_mil_metrics_hand_computed():
    from gipvit.mil import mil_metrics
    p1 = np.array([0.9, 0.4, 0.5, 0.2, 0.7])
    prob = np.stack([1 - p1, p1], axis=1)
    labels = np.array([1, 1, 0, 0, 0])
    m = mil_metrics(prob, labels, 0.375)
    assert list(m) == ["mil_top1", "mil_loss", "mil_auc_per_slide"]
    # arg-max (lowest class on the 0.5 tie): 1 0 0 0 1 -> hits 1 0 1 1 0
    assert m["mil_top1"] == 60.0 and m["mil_loss"] == 0.375
    # (pos, neg) pairs: 0.9 beats 0.5 0.2 0.7; 0.4 beats 0.2 only -> 4 of 6
    assert abs(m["mil_auc_per_slide"] - 4 / 6) < 1e-12
    assert list(mil_metrics(prob[:, :1], np.zeros(5, dtype=int), 0.0)) == ["mil_top1", "mil_loss"]
    with pytest.raises(ValueError):
        mil_metrics(prob, labels[:3], 0.0)


class _Runner:
    D, img, dev = 192, 64, "cpu"

    class vit:
        depth = 12


def test_state_dict_names_and_shapes_and_refused_settings():
    from gipvit.mil import MilProbe, init_params
    probe = MilProbe(_Runner(), num_classes=3, hidden=32, n_last=2)
    assert (probe.F, probe.L, probe.C) == (384, 32, 3)
    with pytest.raises(RuntimeError):
        probe.state_dict()
    probe.params = init_params(32, 3, 384, 0)
    sd = probe.state_dict()
    assert list(sd) == NAMES
    lin = {"attention_V": torch.nn.Linear(384, 32), "attention_U": torch.nn.Linear(384, 32), "attention_w": torch.nn.Linear(32, 1),
           "classifier": torch.nn.Linear(384, 3)}
    for name, mod in lin.items():
        assert sd[name + ".weight"].shape == mod.weight.shape and sd[name + ".bias"].shape == mod.bias.shape
        mod.load_state_dict({"weight": sd[name + ".weight"], "bias": sd[name + ".bias"]})
    for kw in (dict(num_classes=0), dict(num_classes=33), dict(hidden=8), dict(hidden=40), dict(hidden=272), dict(lr=0.0), dict(lr=float("nan")),
               dict(weight_decay=-1e-3), dict(epochs=0), dict(batch=0), dict(batch=65), dict(n_last=0), dict(n_last=13)):
        with pytest.raises(ValueError):
            MilProbe(_Runner(), **kw)
    assert MilProbe(None, features=1536).F == 1536
    with pytest.raises(ValueError):
        MilProbe(None)
    with pytest.raises(ValueError):
        MilProbe(None, features=4100)


# ---- the ABI without a GPU
def _lib():
    from gipvit import _lib as L
    return L


def test_struct_layouts_match_gcc(tmp_path):
    L = _lib()
    structs = [L.gv_mil_train_args, L.gv_mil_predict_args]
    lines = []
    for st in structs:
        lines.append(f'printf("{st.__name__} %zu\\n", sizeof({st.__name__}));')
        lines += [f'printf("{st.__name__}.{f} %zu\\n", offsetof({st.__name__}, {f}));' for f, _ in st._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gipvit.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for st in structs:
        assert int(out[st.__name__]) == ctypes.sizeof(st), st.__name__
        for f, _ in st._fields_:
            assert int(out[f"{st.__name__}.{f}"]) == getattr(st, f).offset, (st.__name__, f)


TRAIN_OK = dict(params=4096, m=8192, v=12288, x=16384, bag_ptr=20480, labels=24576, bags=28672, loss_sum=32768, workspace=36864,
                workspace_bytes=1 << 40, ldx=384, N=4000, F=384, L=128, C=2, n_all_bags=10, n_bags=10, batch=8, max_bag=500, step0=0,
                lr=5e-4, lr_scale=1.0, wd=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)      # never dereferenced


def test_mil_train_abi_errors():
    L = _lib()

    def rc(**kw):
        return L.lib.gv_mil_train(ctypes.byref(L.gv_mil_train_args(**dict(TRAIN_OK, **kw))), None)

    def err():
        return L.lib.gv_last_error().decode()
    assert L.lib.gv_mil_train(None, None) == -3
    for name in ("params", "m", "v", "x", "bag_ptr", "labels", "bags", "loss_sum", "workspace"):
        assert rc(**{name: None}) == -3 and "null" in err(), name
    for F in (0, 382, 4100):
        assert rc(F=F, ldx=4100) == -1 and "4096" in err() and "multiple of 4" in err(), F
    for Lh in (0, 8, 24, 272):
        assert rc(L=Lh) == -1 and "multiple of 16" in err() and "256" in err(), Lh
    for C in (0, 33):
        assert rc(C=C) == -1 and "1 <= C <= 32" in err(), C
    for b in (0, 65):
        assert rc(batch=b) == -1 and "1 <= batch <= 64" in err(), b
    for mb in (0, 4097):
        assert rc(max_bag=mb) == -1 and "1 <= max_bag <= 4096" in err(), mb
    assert rc(N=0) == -1 and "N >= 1" in err()
    assert rc(n_bags=0) == -1 and "n_bags >= 1" in err()
    assert rc(n_all_bags=0) == -1 and "n_all_bags >= 1" in err()
    assert rc(ldx=380) == -1 and "ldx >= F" in err()
    assert rc(ldx=386) == -2 and "multiple of 4" in err()
    assert rc(x=16384 + 4) == -2 and "16-byte aligned" in err()
    assert rc(params=4096 + 8) == -2 and "16-byte aligned" in err()
    assert rc(m=8192 + 4) == -2 and "16-byte aligned" in err()
    assert rc(step0=-1) == -1 and "step0" in err()
    for v in (0.0, -1e-3, float("inf"), float("nan")):
        assert rc(lr=v) == -1 and "lr finite and > 0" in err(), v
    for v in (-0.5, float("inf"), float("nan")):
        assert rc(lr_scale=v) == -1 and "lr_scale finite and >= 0" in err(), v
    assert rc(wd=-1e-4) == -1 and "wd" in err()
    for v in (-0.1, 1.0, float("nan")):
        assert rc(beta1=v) == -1 and "beta1" in err(), v
        assert rc(beta2=v) == -1 and "beta2" in err(), v
    for v in (0.0, -1e-8, float("nan")):
        assert rc(eps=v) == -1 and "eps" in err(), v
    need = L.lib.gv_mil_workspace_bytes(8, 500, 128, 2, 384)
    assert need > 0
    assert rc(workspace_bytes=need - 1) == -1 and str(need) in err() and "workspace" in err()
    assert rc(workspace=36864 + 4) == -2 and "workspace" in err()


def test_mil_predict_abi_errors():
    L = _lib()
    ok = dict(params=4096, x=8192, bag_ptr=12288, labels=16384, bags=None, prob=20480, loss=24576, attn=28672, score=32768, workspace=36864,
              workspace_bytes=1 << 40, ldx=384, N=4000, F=384, L=128, C=2, n_all_bags=100, n_bags=100, max_bag=500, accumulate=0)

    def rc(**kw):
        return L.lib.gv_mil_predict(ctypes.byref(L.gv_mil_predict_args(**dict(ok, **kw))), None)

    def err():
        return L.lib.gv_last_error().decode()
    assert L.lib.gv_mil_predict(None, None) == -3
    for name in ("params", "x", "bag_ptr", "prob", "workspace"):
        assert rc(**{name: None}) == -3 and "null" in err(), name
    assert rc(labels=None) == -3 and "labels" in err()                      # a loss needs labels
    assert rc(n_bags=0) == -1 and "n_bags >= 1" in err()
    assert rc(F=4100, ldx=4100) == -1 and "4096" in err()
    assert rc(L=24) == -1 and "multiple of 16" in err()
    assert rc(C=33) == -1 and "1 <= C <= 32" in err()
    assert rc(max_bag=4097) == -1 and "max_bag" in err()
    assert rc(ldx=380) == -1 and "ldx >= F" in err()
    assert rc(x=8192 + 4) == -2 and "16-byte aligned" in err()
    need = L.lib.gv_mil_workspace_bytes(64, 500, 128, 2, 384)                # more than 64 bags: groups of 64
    assert rc(workspace_bytes=need - 1) == -1 and str(need) in err()
    small = L.lib.gv_mil_workspace_bytes(5, 500, 128, 2, 384)
    assert 0 < small < need and rc(n_bags=5, workspace_bytes=small - 1) == -1 and str(small) in err()


def test_mil_workspace_bytes():
    L = _lib()
    ws = L.lib.gv_mil_workspace_bytes
    assert ws(1, 1, 16, 1, 4) > 0 and ws(64, 4096, 256, 32, 4096) > 0
    sizes = [ws(b, 500, 128, 2, 384) for b in (1, 2, 8, 64)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    assert ws(8, 500, 128, 2, 384) >= 8 * 500 * 128 * 2 * 4                  # t and g of every row at least
    for bad in ((0, 500, 128, 2, 384), (65, 500, 128, 2, 384), (8, 0, 128, 2, 384), (8, 4097, 128, 2, 384), (8, 500, 0, 2, 384), (8, 500, 24, 2, 384),
                (8, 500, 272, 2, 384), (8, 500, 128, 0, 384), (8, 500, 128, 33, 384), (8, 500, 128, 2, 0), (8, 500, 128, 2, 382), (8, 500, 128, 2, 4100)):
        assert ws(*bad) == -1 and L.lib.gv_last_error().decode().startswith("gv_mil_workspace_bytes"), bad


def test_both_builds_export_the_entry_points():
    L = _lib()
    names = ["gv_mil_train", "gv_mil_predict", "gv_mil_workspace_bytes"]
    assert all(hasattr(L.lib, n) for n in names)
    assert L.ENTRY_POINTS["gv_mil_train"] is L.gv_mil_train_args and L.ENTRY_POINTS["gv_mil_predict"] is L.gv_mil_predict_args
    assert "gv_mil_workspace_bytes" in L.PLAIN_SYMBOLS and L.lib.gv_version() == 9
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); missing = [n for n in sys.argv[2:] if not hasattr(l, n)]; assert not missing, missing; "
            "l.gv_mil_workspace_bytes.restype = ctypes.c_int64; assert l.gv_mil_workspace_bytes(8, 500, 128, 2, 384) > 0")
    for lib in ("libgipvit_hip.so", "libgipvit_hip_f16.so"):
        r = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(L.LIB_PATH), lib)] + names, capture_output=True, text=True)
        assert r.returncode == 0, (lib, r.stderr[-600:])


# ---- the driver
def _train():
    sys.path.insert(0, ROOT)
    import train
    return train


MIL = ["--dino", "--mil-probe"]


@pytest.mark.parametrize("flags,word", [
    (["--mil-probe"], "--mil-probe"),                                                         # without --dino
    (MIL + ["--mil-hidden", "8"], "--mil-hidden"),
    (MIL + ["--mil-hidden", "40"], "--mil-hidden"),
    (MIL + ["--mil-hidden", "272"], "--mil-hidden"),
    (MIL + ["--mil-lr", "0"], "--mil-lr"),
    (MIL + ["--mil-lr", "-0.001"], "--mil-lr"),
    (MIL + ["--mil-lr", "nan"], "--mil-lr"),
    (MIL + ["--mil-lr", "inf"], "--mil-lr"),
    (MIL + ["--mil-wd", "-0.001"], "--mil-wd"),
    (MIL + ["--mil-epochs", "0"], "--mil-epochs"),
    (MIL + ["--mil-batch", "0"], "--mil-batch"),
    (MIL + ["--mil-batch", "65"], "--mil-batch"),
    (MIL + ["--mil-layers", "0"], "--mil-layers"),
    (MIL + ["--mil-layers", "13"], "--mil-layers"),
    (MIL + ["--model", "vit_base_patch16_224", "--mil-layers", "6"], "--mil-layers"),          # 6 x 768 > 4096
    (MIL + ["--mil-rate", "-1"], "--mil-rate"),
    (MIL + ["--test_fold", "-1"], "--test_fold"),
    (MIL + ["--tile-size", "128"], "--tile-size"),
    (MIL + ["--num_tiles", "4097"], "--num_tiles"),
    (MIL + ["--knn-bank-tiles", "4097"], "--knn-bank-tiles"),
    (MIL + ["--eval-metric", "f1"], "--eval-metric"),                                         # mil_f1: no such metric
    (MIL + ["--eval-metric", "auc_per_patch"], "--eval-metric"),                              # slides only
    (MIL + ["--eval-metric", "linear_top1"], "--eval-metric"),                                # the linear probe is off
    (MIL + ["--knn-monitor", "--eval-metric", "mil_f1"], "--eval-metric"),
    (MIL + ["--knn-monitor", "--eval-metric", "loss"], "--eval-metric"),                      # a bare name is the k-NN monitor's
    (MIL + ["--linear-probe", "--eval-metric", "mil_auc_per_patch"], "--eval-metric"),
    (MIL + ["--num-classes", "1", "--eval-metric", "auc_per_slide"], "--eval-metric"),        # one class: no AUC
    (["--dino", "--linear-probe", "--eval-metric", "mil_top1"], "--eval-metric"),             # the MIL probe is off
])
def test_driver_refuses_before_any_gpu_work(flags, word):
    train = _train()
    args, _ = train.parse_args((["--model", "vit_tiny"] if "--model" not in flags else []) + flags)
    with pytest.raises(SystemExit) as e:
        train.check_supported(args, lambda m: None)
    assert word in str(e.value)


def test_mil_flags_are_inert_without_the_probe():
    train = _train()
    base, _ = train.parse_args(["--model", "vit_tiny", "--dino"])
    assert (base.mil_probe, base.mil_hidden, base.mil_lr, base.mil_wd, base.mil_epochs, base.mil_batch, base.mil_layers, base.mil_rate) == \
        (False, 128, 5e-4, 1e-4, 50, 8, 1, 0)
    assert train.check_supported(base, lambda m: None) is None
    bad = ["--mil-hidden", "7", "--mil-lr", "-1", "--mil-wd", "-1", "--mil-epochs", "0", "--mil-batch", "999", "--mil-layers", "50", "--mil-rate", "-3"]
    for extra in (["--dino"], []):
        off, _ = train.parse_args(["--model", "vit_tiny", "--test_fold", "-1"] + bad + extra)
        assert not off.mil_probe and train.check_supported(off, lambda m: None) is None
        ref, _ = train.parse_args(["--model", "vit_tiny", "--test_fold", "-1"] + extra)
        differ = {k for k in vars(ref) if getattr(ref, k) != getattr(off, k)}
        assert differ == {"mil_hidden", "mil_lr", "mil_wd", "mil_epochs", "mil_batch", "mil_layers", "mil_rate"}, differ
        assert train.monitor_metric_names(off) == []
    on, _ = train.parse_args(["--model", "vit_tiny"] + MIL + ["--mil-hidden", "64", "--mil-lr", "1e-3", "--mil-wd", "0", "--mil-epochs", "5", "--mil-batch",
                                                               "64", "--mil-layers", "2", "--mil-rate", "2", "--knn-monitor", "--linear-probe"])
    assert train.check_supported(on, lambda m: None) is None
    assert (on.mil_hidden, on.mil_lr, on.mil_wd, on.mil_epochs, on.mil_batch, on.mil_layers, on.mil_rate) == (64, 1e-3, 0.0, 5, 64, 2, 2)
    vb, _ = train.parse_args(["--model", "vit_base_patch16_224"] + MIL + ["--mil-layers", "5"])      # 3840 features: inside the limit
    assert train.check_supported(vb, lambda m: None) is None


@pytest.mark.parametrize("name,knn,probe,mil,want", [
    ("top1", False, False, True, "mil_top1"), ("loss", False, False, True, "mil_loss"), ("auc_per_slide", False, False, True, "mil_auc_per_slide"),
    ("mil_top1", False, False, True, "mil_top1"), ("mil_loss", True, True, True, "mil_loss"), ("mil_auc_per_slide", True, False, True, "mil_auc_per_slide"),
    ("top1", True, False, True, "knn_top1"), ("top1", False, True, True, "linear_top1"), ("top1", True, True, True, "knn_top1"),
    ("loss", False, True, True, "linear_loss"), ("linear_loss", False, True, True, "linear_loss"), ("knn_top1", True, False, True, "knn_top1"),
    ("top1", False, False, False, "top1"), ("mil_top1", False, False, False, "mil_top1"),
])
def test_eval_metric_resolution(name, knn, probe, mil, want):
    train = _train()
    assert train.resolve_eval_metric(name, knn, probe, mil) == want
    if not mil and not name.startswith("mil_"):
        assert train.resolve_eval_metric(name, knn, probe) == want           # the three-argument form is unchanged


def test_metric_names_and_accepted_eval_metrics():
    train = _train()
    mil = ["mil_top1", "mil_loss", "mil_auc_per_slide"]
    only, _ = train.parse_args(["--model", "vit_tiny"] + MIL)
    assert train.monitor_metric_names(only) == mil
    allm, _ = train.parse_args(["--model", "vit_tiny", "--knn-monitor", "--linear-probe"] + MIL)
    assert train.monitor_metric_names(allm) == ["knn_top1", "knn_auc_per_patch", "knn_auc_per_slide", "linear_top1", "linear_loss",
                                                "linear_auc_per_patch", "linear_auc_per_slide"] + mil
    one, _ = train.parse_args(["--model", "vit_tiny", "--num-classes", "1"] + MIL)
    assert train.monitor_metric_names(one) == ["mil_top1", "mil_loss"]
    for flags in (["--eval-metric", "loss"], ["--eval-metric", "auc_per_slide"], ["--eval-metric", "mil_auc_per_slide"],
                  ["--knn-monitor", "--eval-metric", "mil_loss"], ["--linear-probe", "--eval-metric", "mil_top1"],
                  ["--linear-probe", "--knn-monitor", "--eval-metric", "mil_auc_per_slide"], ["--linear-probe", "--eval-metric", "auc_per_patch"],
                  ["--num-classes", "1", "--eval-metric", "top1"]):
        args, _ = train.parse_args(["--model", "vit_tiny"] + MIL + flags)
        assert train.check_supported(args, lambda m: None) is None, flags
    row = train.summary_row(3, {"loss": 1.0}, {"mil_top1": 50.0, "mil_loss": 0.7, "mil_auc_per_slide": 0.5}, train.monitor_metric_names(allm), 1e-3)
    assert list(row)[-4:] == ["eval_mil_top1", "eval_mil_loss", "eval_mil_auc_per_slide", "lr"] and row["eval_knn_top1"] == "" and row["eval_mil_loss"] == 0.7


def test_mil_checks_load_no_library():
    code = ("import os, sys; sys.path.insert(0, %r); import train\n"
            "a, _ = train.parse_args(['--model', 'vit_base_patch16_224', '--dino', '--mil-probe', '--mil-layers', '4', '--amp'])\n"
            "assert train.check_supported(a, lambda m: None) is None\n"
            "a, _ = train.parse_args(['--model', 'vit_tiny', '--dino', '--mil-probe', '--mil-layers', '13', '--amp'])\n"
            "try:\n    train.check_supported(a, lambda m: None)\n    raise AssertionError('accepted')\nexcept SystemExit as e:\n    assert '--mil-layers' in str(e)\n"
            "assert 'gipvit._lib' not in sys.modules and 'gipvit.engine' not in sys.modules and 'gipvit.mil' not in sys.modules" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "GIPVIT_ACT_FORMAT"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-800:]


# ---- learnability of the specification
def needle_bags(n_bags, seed, F=16):
    """Bags of 16..40 rows of N(0, 1) noise; every second bag is positive: two of its rows ("needles") carry +6 along a fixed
    direction.  -> (x f32 [N, F], ptr, labels int64 [n_bags], needle mask bool [N])."""
    rng = np.random.Generator(np.random.PCG64([seed, 99]))
    direction = np.zeros(F)
    direction[:4] = 0.5                                                    # unit length
    sizes = rng.integers(16, 41, size=n_bags)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = rng.standard_normal((int(ptr[-1]), F))
    labels = np.arange(n_bags) % 2
    needle = np.zeros(int(ptr[-1]), dtype=bool)
    for b in range(n_bags):
        if labels[b]:
            rows = ptr[b] + rng.choice(sizes[b], size=2, replace=False)
            x[rows] += 6.0 * direction
            needle[rows] = True
    return torch.from_numpy(x.astype(np.float32)), ptr, torch.from_numpy(labels), needle


NEEDLE = dict(L=16, C=2, F=16, batch=4, lr=1e-2, wd=1e-4, epochs=40, seed=7)


def needle_check(prob, attn, ptr, labels, needle):
    """AUC 1.0 over the fresh bags, and more than half of every positive bag's attention on its two needles."""
    from gipvit.validate import _auc
    assert _auc(np.asarray(labels), np.asarray(prob)[:, 1]) == 1.0
    shares = [float(np.asarray(attn)[ptr[b]:ptr[b + 1]][needle[ptr[b]:ptr[b + 1]]].sum()) for b in range(len(labels)) if labels[b]]
    assert min(shares) > 0.5, shares
    return min(shares)


def test_the_specification_learns_needle_bags():
    c = NEEDLE
    x, ptr, labels, _ = needle_bags(24, c["seed"])
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    perms = np.stack([rng.permutation(24) for _ in range(c["epochs"])])
    P, _, _, loss = mil_reference(x, ptr, labels, draw_params(c["L"], c["C"], c["F"], c["seed"]), perms, c["batch"], c["lr"], c["wd"])
    xq, ptrq, yq, needle = needle_bags(12, c["seed"] + 1)
    prob, attn, _, _ = mil_predict_reference(P, xq, ptrq)
    share = needle_check(prob.numpy(), attn.numpy(), ptrq, yq.numpy(), needle)
    print(f"needle bags: epoch loss {float(loss[0]):.4f} -> {float(loss[-1]):.4f}, least attention share on the needles {share:.3f}")
