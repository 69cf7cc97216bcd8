"""CPU: the linear probe's references -- f64 torch.optim.SGD over nn.Linear heads (what the GPU tests hold gv_linprobe_train to) and
an f32 restatement of the kernel's step, with the well-posedness of the shared cases between them -- the entry points' refusals
through the ABI without a GPU, the workspace query, LinearProbe's host logic (hold-out rule, head selection, metrics,
permutations) and the driver's --linprobe-* flags (refusals before any GPU work, inert without --linear-probe, --eval-metric)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU = 0.9
# (N, F, H, C, M, epochs, seed): an F tail + an M tail (last step of 60 rows); five heads of three classes; H C at the limit of 64;
# one step per epoch with C at the limit; ViT-B width with a last step of 4 rows; 16 heads of 4 classes in steps of 33 rows.
# (The ViT-B case has six heads, not two: at 3840 randn features a 4-row step at the two largest rates, 0.3 and 0.15, overshoots
# and their loss rises from epoch to epoch; the heads from rate 0.075 down learn, which is what the well-posedness test asks of
# a case.)
CASES = [(200, 196, 3, 2, 70, 3, 0), (333, 768, 5, 3, 128, 2, 1), (150, 1536, 32, 2, 64, 2, 2), (97, 64, 1, 32, 97, 4, 3),
         (260, 3840, 6, 2, 256, 2, 4), (129, 384, 16, 4, 33, 2, 5)]
CASE_IDS = ["N%d-F%d-H%d-C%d-M%d" % c[:5] for c in CASES]


def probe_inputs(N, F, C, seed):
    """Seeded inputs: randn features f32 [N, F] and labels int64 [N] drawn from a planted linear rule plus noise (so that a
    linear head can learn them and the loss falls)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, F, generator=g)
    planted = torch.randn(C, F, generator=g) / math.sqrt(F)
    labels = (2.0 * x @ planted.t() + torch.randn(N, C, generator=g)).argmax(dim=1)
    return x, labels


def head_rates(H):
    """Per-head rate 0.3 * 0.5 ** (h mod 6), weight decay alternating 0 and 1e-3."""
    return [0.3 * 0.5 ** (h % 6) for h in range(H)], [0.0 if h % 2 == 0 else 1e-3 for h in range(H)]


def cosine_scale(e, epochs):
    return 0.5 * (1.0 + math.cos(math.pi * e / epochs))


def case_setup(case):
    """-> dict of a case's inputs: x, labels, W0 [H, C, F] (every head the same N(0, 0.01^2) draw), b0, lr, wd, perms
    [epochs, N] (numpy PCG64(seed)), M, epochs."""
    N, F, H, C, M, epochs, seed = case
    x, labels = probe_inputs(N, F, C, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    W0 = (0.01 * torch.randn(C, F, generator=g)).expand(H, C, F).contiguous()
    lr, wd = head_rates(H)
    rng = np.random.Generator(np.random.PCG64(seed))
    perms = np.stack([rng.permutation(N) for _ in range(epochs)])
    return dict(x=x, labels=labels, W0=W0, b0=torch.zeros(H, C), lr=lr, wd=wd, perms=perms, M=M, epochs=epochs)


def probe_reference(x, labels, W0, b0, lr, wd, perms, M, mu=MU, dtype=torch.float64):
    """torch.optim.SGD(momentum, weight_decay) over nn.Linear heads under CrossEntropyLoss (mean), one parameter group per head,
    the cosine factor set per epoch, the rows of an epoch visited in perms[e]'s order M at a time.
    -> (W [H, C, F], b [H, C], mW, mb, epoch_loss [epochs, H] = mean -log p[label] over the epoch's rows), all ``dtype``."""
    H, C, F = W0.shape
    xd = x.to(dtype)
    heads = [torch.nn.Linear(F, C).to(dtype) for _ in range(H)]
    with torch.no_grad():
        for h, lin in enumerate(heads):
            lin.weight.copy_(W0[h])
            lin.bias.copy_(b0[h])
    opt = torch.optim.SGD([dict(params=list(lin.parameters()), lr=lr[h], weight_decay=wd[h]) for h, lin in enumerate(heads)], lr=1.0, momentum=mu)
    ce_mean, ce_sum = torch.nn.CrossEntropyLoss(), torch.nn.CrossEntropyLoss(reduction="sum")
    epochs = len(perms)
    epoch_loss = torch.zeros(epochs, H, dtype=dtype)
    for e in range(epochs):
        for h, grp in enumerate(opt.param_groups):
            grp["lr"] = lr[h] * cosine_scale(e, epochs)
        for s in range(0, len(perms[e]), M):
            r = torch.from_numpy(np.asarray(perms[e][s:s + M]).astype(np.int64))
            opt.zero_grad()
            total = 0.0
            for h, lin in enumerate(heads):
                z = lin(xd[r])
                total = total + ce_mean(z, labels[r])
                epoch_loss[e, h] += ce_sum(z, labels[r]).detach()
            total.backward()
            opt.step()
        epoch_loss[e] /= len(perms[e])
    buf = lambda p: opt.state[p]["momentum_buffer"].detach()
    return (torch.stack([lin.weight.detach() for lin in heads]), torch.stack([lin.bias.detach() for lin in heads]),
            torch.stack([buf(lin.weight) for lin in heads]), torch.stack([buf(lin.bias) for lin in heads]), epoch_loss)


def probe_predict_reference(W, b, x):
    """softmax of the heads' logits in f64: prob [Q, H, C]."""
    z = torch.einsum("hcf,qf->qhc", W.double(), x.double()) + b.double()
    return torch.softmax(z, dim=2)


def probe_restatement_f32(x, labels, W0, b0, lr, wd, perms, M, mu=MU):
    """The step as include/gipvit.h states it, in f32 on the CPU: same returns as ``probe_reference``."""
    f32 = torch.float32
    H, C, F = W0.shape
    W, b = W0.clone().to(f32), b0.clone().to(f32)
    mW, mb = torch.zeros_like(W), torch.zeros_like(b)
    lr_t, wd_t = torch.tensor(lr, dtype=f32), torch.tensor(wd, dtype=f32)
    epochs = len(perms)
    epoch_loss = torch.zeros(epochs, H, dtype=f32)
    for e in range(epochs):
        step = lr_t * torch.tensor(cosine_scale(e, epochs), dtype=f32)
        for s in range(0, len(perms[e]), M):
            r = torch.from_numpy(np.asarray(perms[e][s:s + M]).astype(np.int64))
            xr, y, m = x[r], labels[r], len(r)
            z = torch.einsum("hcf,jf->hjc", W, xr) + b[:, None, :]
            z = z - z.max(dim=2, keepdim=True).values
            ez = z.exp()
            ssum = ez.sum(dim=2, keepdim=True)
            p = ez / ssum
            zy = z.gather(2, y.view(1, m, 1).expand(H, m, 1))
            epoch_loss[e] += (ssum.log() - zy).sum(dim=(1, 2))
            g = (p - torch.nn.functional.one_hot(y, C).to(f32)) / m
            dW = torch.einsum("hjc,jf->hcf", g, xr) + wd_t[:, None, None] * W
            db = g.sum(dim=1) + wd_t[:, None] * b
            mW = mu * mW + dW
            mb = mu * mb + db
            W = W - step[:, None, None] * mW
            b = b - step[:, None] * mb
        epoch_loss[e] /= len(perms[e])
    return W, b, mW, mb, epoch_loss


_ref_cache = {}


def case_reference(case):
    """Inputs and f64 reference of a case, computed once and shared by the tests of both files (never modified)."""
    if case not in _ref_cache:
        s = case_setup(case)
        _ref_cache[case] = (s, probe_reference(**s_args(s)))
    return _ref_cache[case]


def s_args(s):
    return {k: s[k] for k in ("x", "labels", "W0", "b0", "lr", "wd", "perms", "M")}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_cases_are_well_posed(case):
    """The f32 restatement of the step stays within 2.5e-7 of the f64 reference on W and b and within 5e-7 on the epoch losses,
    so the GPU bounds (2e-6 / 4e-6, about ten times that) leave room for another summation order and nothing else; and the loss
    falls over the epochs for at least one head."""
    s, (W, b, mW, mb, loss) = case_reference(case)
    W32, b32, mW32, mb32, loss32 = probe_restatement_f32(**s_args(s))
    ew, eb = float((W32.double() - W).abs().max()), float((b32.double() - b).abs().max())
    el = float((loss32.double() - loss).abs().max())
    print(f"f32 restatement against f64: W {ew:.3e}  b {eb:.3e}  epoch loss {el:.3e}; f64 epoch losses of head 0: {[round(float(v), 4) for v in loss[:, 0]]}")
    assert ew <= 2.5e-7 and eb <= 2.5e-7 and el <= 5e-7
    assert bool((loss[-1] < loss[0]).any())
    assert bool(torch.isfinite(W).all()) and bool(torch.isfinite(loss).all())


def test_reference_first_step_is_the_gradient():
    """One step from zero-initialised buffers: the momentum buffer equals the gradient (+ wd W) written out by hand, as in torch."""
    x, labels = probe_inputs(12, 8, 3, seed=9)
    W0 = 0.01 * torch.randn(2, 3, 8, generator=torch.Generator().manual_seed(1))
    b0 = torch.zeros(2, 3)
    lr, wd = [0.2, 0.1], [0.0, 1e-2]
    W, b, mW, mb, loss = probe_reference(x, labels, W0, b0, lr, wd, np.arange(12)[None, :], 12)
    p = probe_predict_reference(W0, b0, x)                                  # [12, 2, 3]
    g = (p - torch.nn.functional.one_hot(labels, 3).double()[:, None, :]) / 12
    dW = torch.einsum("jhc,jf->hcf", g, x.double()) + torch.tensor(wd, dtype=torch.float64)[:, None, None] * W0.double()
    assert float((mW - dW).abs().max()) <= 1e-15 and float((mb - g.sum(0)).abs().max()) <= 1e-15
    assert float((W - (W0.double() - torch.tensor(lr, dtype=torch.float64)[:, None, None] * dW)).abs().max()) <= 1e-15      # cosine factor 1 at epoch 0
    want = -torch.log(p[torch.arange(12), :, labels]).mean(0)
    assert float((loss[0] - want).abs().max()) <= 1e-14


def _lib():
    from gipvit import _lib as L
    return L


def test_linprobe_train_abi_errors():
    L = _lib()
    ok = dict(W=4096, b=8192, mW=12288, mb=16384, lr=20480, wd=24576, x=28672, labels=32768, rows=36864, loss_sum=40960, workspace=45056,
              workspace_bytes=1 << 30, ldx=768, N=1000, F=768, H=5, C=3, n_rows=1000, batch=128, lr_scale=1.0, momentum=0.9)      # never dereferenced

    def rc(**kw):
        return L.lib.gv_linprobe_train(ctypes.byref(L.gv_linprobe_train_args(**dict(ok, **kw))), None)

    def err():
        return L.lib.gv_last_error().decode()
    assert L.lib.gv_linprobe_train(None, None) == -3
    for name in ("W", "b", "mW", "mb", "lr", "wd", "x", "labels", "rows", "loss_sum", "workspace"):
        assert rc(**{name: None}) == -3 and "null" in err(), name
    for C in (0, 33):
        assert rc(C=C, H=1) == -1 and "1 <= C <= 32" in err(), C
    assert rc(H=0) == -1 and "H >= 1" in err()
    assert rc(H=22, C=3) == -1 and "H * C <= 64" in err()
    for F in (0, 766, 4100):
        assert rc(F=F, ldx=4100) == -1 and "4096" in err() and "multiple of 4" in err(), F
    assert rc(ldx=764) == -1 and "ldx >= F" in err()
    assert rc(ldx=770) == -2 and "multiple of 4" in err()
    assert rc(x=28672 + 4) == -2 and "16-byte aligned" in err()
    assert rc(W=4096 + 8) == -2 and "16-byte aligned" in err()
    for M in (0, 4097):
        assert rc(batch=M) == -1 and "1 <= batch <= 4096" in err(), M
    assert rc(n_rows=0) == -1 and "n_rows >= 1" in err()
    assert rc(N=0) == -1 and "N >= 1" in err()
    for v in (-0.5, float("inf"), float("nan")):
        assert rc(lr_scale=v) == -1 and "lr_scale finite and >= 0" in err(), v
    for v in (-0.1, 1.0, float("nan")):
        assert rc(momentum=v) == -1 and "0 <= momentum < 1" in err(), v
    need = L.lib.gv_linprobe_workspace_bytes(128, 5, 3, 768)
    assert need > 0
    assert rc(workspace_bytes=need - 1) == -1 and str(need) in err() and "workspace" in err()
    assert rc(workspace=45056 + 4) == -2 and "workspace" in err()


def test_linprobe_predict_abi_errors():
    L = _lib()
    ok = dict(W=4096, b=8192, x=12288, labels=16384, prob=20480, loss=24576, workspace=28672, workspace_bytes=1 << 30, ldx=384, Q=5000, F=384, H=16, C=4)

    def rc(**kw):
        return L.lib.gv_linprobe_predict(ctypes.byref(L.gv_linprobe_predict_args(**dict(ok, **kw))), None)

    def err():
        return L.lib.gv_last_error().decode()
    assert L.lib.gv_linprobe_predict(None, None) == -3
    for name in ("W", "b", "x", "prob", "workspace"):
        assert rc(**{name: None}) == -3 and "null" in err(), name
    assert rc(labels=None) == -3 and "labels" in err()                      # a loss needs labels
    assert rc(Q=0) == -1 and "Q >= 1" in err()
    assert rc(C=33, H=1) == -1 and "1 <= C <= 32" in err()
    assert rc(H=17) == -1 and "H * C <= 64" in err()
    assert rc(F=4100, ldx=4100) == -1 and "4096" in err()
    assert rc(ldx=380) == -1 and "ldx >= F" in err()
    assert rc(ldx=386) == -2 and "multiple of 4" in err()
    assert rc(x=12288 + 4) == -2 and "16-byte aligned" in err()
    need = L.lib.gv_linprobe_workspace_bytes(4096, 16, 4, 384)               # Q past 4096: chunks of 4096 rows
    assert rc(workspace_bytes=need - 1) == -1 and str(need) in err()
    small = L.lib.gv_linprobe_workspace_bytes(70, 16, 4, 384)
    assert 0 < small < need and rc(Q=70, workspace_bytes=small - 1) == -1 and str(small) in err()


def test_linprobe_workspace_bytes():
    L = _lib()
    ws = L.lib.gv_linprobe_workspace_bytes
    assert ws(1, 1, 1, 4) > 0 and ws(4096, 32, 2, 4096) > 0
    sizes = [ws(M, 8, 2, 1536) for M in (1, 64, 65, 1024, 4096)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4 and sizes[0] == sizes[1]      # per 64-row tile
    assert ws(1024, 8, 2, 1536) >= 1024 * 16 * 4                            # g [m, H C] at least
    for bad in ((0, 1, 2, 64), (4097, 1, 2, 64), (64, 0, 2, 64), (64, 33, 2, 64), (64, 1, 0, 64), (64, 1, 33, 64), (64, 3, 32, 64),
                (64, 1, 2, 0), (64, 1, 2, 62), (64, 1, 2, 4100)):
        assert ws(*bad) == -1 and L.lib.gv_last_error().decode().startswith("gv_linprobe_workspace_bytes"), bad


def test_both_builds_export_the_entry_points():
    L = _lib()
    names = ["gv_linprobe_train", "gv_linprobe_predict", "gv_linprobe_workspace_bytes"]
    assert all(hasattr(L.lib, n) for n in names)
    assert L.ENTRY_POINTS["gv_linprobe_train"] is L.gv_linprobe_train_args and L.ENTRY_POINTS["gv_linprobe_predict"] is L.gv_linprobe_predict_args
    assert "gv_linprobe_workspace_bytes" in L.PLAIN_SYMBOLS and L.lib.gv_version() == 9
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); missing = [n for n in sys.argv[2:] if not hasattr(l, n)]; assert not missing, missing; "
            "l.gv_linprobe_workspace_bytes.restype = ctypes.c_int64; assert l.gv_linprobe_workspace_bytes(128, 5, 3, 768) > 0")
    for lib in ("libgipvit_hip.so", "libgipvit_hip_f16.so"):
        r = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(L.LIB_PATH), lib)] + names, capture_output=True, text=True)
        assert r.returncode == 0, (lib, r.stderr[-600:])


# ---- LinearProbe's host logic
def test_holdout_rule():
    from gipvit.linprobe import holdout_slides
    with pytest.raises(ValueError):
        holdout_slides(1, 0.2)
    assert holdout_slides(2, 0.2).tolist() == [False, True]                  # floor never steps: the last slide
    assert holdout_slides(5, 0.2).tolist() == [False, False, False, False, True]
    assert holdout_slides(11, 0.2).tolist() == [False, False, False, False, True, False, False, False, False, True, False]
    assert holdout_slides(2, 0.5).tolist() == [False, True] and holdout_slides(5, 0.5).tolist() == [False, True, False, True, False]
    for n in (2, 5, 11):
        for h in (0.1, 0.2, 0.33, 0.5):
            sel = holdout_slides(n, h)
            assert sel.dtype == bool and 1 <= sel.sum() < n                  # something to choose on, something to train on
            assert holdout_slides(n, h).tolist() == sel.tolist()             # deterministic


def test_head_selection():
    from gipvit.linprobe import select_head
    assert select_head([0.7, 0.5, 0.6]) == 1
    assert select_head([0.5, 0.4, 0.4, 0.9]) == 1                            # a tie goes to the lower index
    assert select_head([0.3]) == 0
    assert select_head([float("nan"), 0.8, 0.6]) == 2 and select_head([0.8, float("nan")]) == 0


def test_probe_metrics_against_sklearn_and_hand_computed_slide_mean():
    from sklearn.metrics import roc_auc_score
    from gipvit.linprobe import probe_metrics
    p1 = np.array([0.25, 0.75, 0.5, 0.75, 0.2, 0.6, 1.0, 0.4])
    prob = np.stack([1.0 - p1, p1], axis=1)
    labels = np.array([0, 0, 0, 1, 1, 1, 1, 0])
    slides = np.array([10, 10, 10, 7, 7, 3, 3, 5])                           # slide 10 (label 0), 7 (1), 3 (1), 5 (0)
    m = probe_metrics(prob, labels, slides, 0.625)
    assert list(m) == ["linear_top1", "linear_loss", "linear_auc_per_patch", "linear_auc_per_slide"]
    # arg-max, the lowest class on a tie: predictions 0 1 0 1 0 1 1 0 -> hits 1 0 1 1 0 1 1 1
    assert m["linear_top1"] == 100.0 * 6 / 8 and m["linear_loss"] == 0.625
    assert abs(m["linear_auc_per_patch"] - roc_auc_score(labels, p1)) < 1e-12
    slide_score = [(0.25 + 0.75 + 0.5) / 3, (0.75 + 0.2) / 2, (0.6 + 1.0) / 2, 0.4]
    assert abs(m["linear_auc_per_slide"] - roc_auc_score([0, 1, 1, 0], slide_score)) < 1e-12
    assert m["linear_auc_per_slide"] == 0.75                                 # 0.5 / 0.475 / 0.8 / 0.4: one of the four (pos, neg) pairs is inverted
    assert probe_metrics(prob, labels, [f"s{v}" for v in slides], 0.625) == m
    assert list(probe_metrics(prob[:, :1], np.zeros(8, dtype=int), slides, 0.0)) == ["linear_top1", "linear_loss"]
    with pytest.raises(ValueError):
        probe_metrics(prob, labels[:5], slides, 0.0)


def test_permutations_schedule_and_initial_heads_depend_on_the_seed_only():
    from gipvit.linprobe import epoch_permutations, init_heads, lr_scale_at
    a, b = epoch_permutations(37, 4, seed=3), epoch_permutations(37, 4, seed=3)
    assert a.shape == (4, 37) and np.array_equal(a, b) and all(sorted(r) == list(range(37)) for r in a.tolist())
    assert len({tuple(r) for r in a.tolist()}) == 4                          # a new order every epoch
    assert not np.array_equal(a, epoch_permutations(37, 4, seed=4))
    assert np.array_equal(epoch_permutations(37, 6, seed=3)[:4], a)           # more epochs continue the same stream
    rng = np.random.Generator(np.random.PCG64(3))
    assert np.array_equal(a, np.stack([rng.permutation(37) for _ in range(4)]))
    assert [lr_scale_at(e, 4) for e in (0, 2)] == [1.0, 0.5 * (1.0 + math.cos(math.pi / 2))] and 0 < lr_scale_at(3, 4) < 0.5
    W, bias = init_heads(3, 2, 16, seed=5)
    assert W.shape == (3, 2, 16) and W.dtype == torch.float32 and bias.shape == (3, 2) and not bias.any()
    assert torch.equal(W[0], W[1]) and torch.equal(W[0], W[2]) and torch.equal(W, init_heads(3, 2, 16, seed=5)[0])
    assert not torch.equal(W, init_heads(3, 2, 16, seed=6)[0])
    big = init_heads(1, 32, 4096, seed=0)[0]
    assert abs(float(big.std()) - 0.01) < 2e-4 and abs(float(big.mean())) < 1e-4


def test_linear_probe_refuses_bad_settings():
    from gipvit.linprobe import LinearProbe

    class Runner:
        D, img, dev = 768, 224, "cpu"

        class vit:
            depth = 12
    ok = LinearProbe(Runner(), lrs=(0.1, 0.2), n_last=4, avgpool=True)
    assert (ok.H, ok.C, ok.F) == (2, 2, 3840)
    for kw in (dict(lrs=()), dict(lrs=(0.1, 0.0)), dict(lrs=(float("nan"),)), dict(lrs=[0.1] * 33), dict(num_classes=0), dict(num_classes=33),
               dict(epochs=0), dict(batch=0), dict(batch=4097), dict(n_last=0), dict(n_last=13), dict(n_last=5, avgpool=True), dict(weight_decay=-1e-3),
               dict(holdout=0.0), dict(holdout=0.6)):
        with pytest.raises(ValueError):
            LinearProbe(Runner(), **kw)
    with pytest.raises(RuntimeError):
        ok.state_dict()


# ---- the driver
def _train():
    sys.path.insert(0, ROOT)
    import train
    return train


PROBE = ["--dino", "--linear-probe"]


@pytest.mark.parametrize("flags,word", [
    (["--linear-probe"], "--linear-probe"),                                                   # without --dino
    (PROBE + ["--linprobe-lrs", "0"], "--linprobe-lrs"),
    (PROBE + ["--linprobe-lrs", "0.1", "-0.1"], "--linprobe-lrs"),
    (PROBE + ["--linprobe-lrs", "nan"], "--linprobe-lrs"),
    (PROBE + ["--linprobe-lrs", "inf"], "--linprobe-lrs"),
    (PROBE + ["--linprobe-lrs"] + ["0.1"] * 33, "--linprobe-lrs"),                            # 33 heads x 2 classes > 64
    (PROBE + ["--num-classes", "10", "--linprobe-lrs"] + ["0.1"] * 7, "--linprobe-lrs"),
    (PROBE + ["--linprobe-epochs", "0"], "--linprobe-epochs"),
    (PROBE + ["--linprobe-batch", "0"], "--linprobe-batch"),
    (PROBE + ["--linprobe-batch", "4097"], "--linprobe-batch"),
    (PROBE + ["--linprobe-layers", "0"], "--linprobe-layers"),
    (PROBE + ["--linprobe-layers", "13"], "--linprobe-layers"),
    (PROBE + ["--model", "vit_base_patch16_224", "--linprobe-layers", "5", "--linprobe-avgpool"], "--linprobe-layers"),      # 6 x 768 > 4096
    (PROBE + ["--linprobe-wd", "-0.001"], "--linprobe-wd"),
    (PROBE + ["--linprobe-rate", "-1"], "--linprobe-rate"),
    (PROBE + ["--linprobe-holdout", "0"], "--linprobe-holdout"),
    (PROBE + ["--linprobe-holdout", "0.51"], "--linprobe-holdout"),
    (PROBE + ["--test_fold", "-1"], "--test_fold"),
    (PROBE + ["--tile-size", "128"], "--tile-size"),
    (PROBE + ["--eval-metric", "f1"], "--eval-metric"),                                       # linear_f1: no such metric
    (PROBE + ["--knn-monitor", "--eval-metric", "linear_f1"], "--eval-metric"),
    (PROBE + ["--knn-monitor", "--eval-metric", "knn_loss"], "--eval-metric"),
    (PROBE + ["--num-classes", "1", "--eval-metric", "auc_per_slide"], "--eval-metric"),      # one class: no AUC
    (PROBE + ["--eval-metric", "knn_top1"], "--eval-metric"),                                 # the monitor is off
])
def test_driver_refuses_before_any_gpu_work(flags, word):
    train = _train()
    args, _ = train.parse_args((["--model", "vit_tiny"] if "--model" not in flags else []) + flags)
    with pytest.raises(SystemExit) as e:
        train.check_supported(args, lambda m: None)
    assert word in str(e.value)


def test_an_empty_rate_list_is_refused():
    train = _train()
    args, _ = train.parse_args(["--model", "vit_tiny"] + PROBE)
    args.linprobe_lrs = []                                                   # (a YAML config can say so; argparse's nargs="+" cannot)
    with pytest.raises(SystemExit) as e:
        train.check_supported(args, lambda m: None)
    assert "--linprobe-lrs" in str(e.value)


def test_linprobe_flags_are_inert_without_the_probe():
    train = _train()
    base, _ = train.parse_args(["--model", "vit_tiny", "--dino"])
    assert (base.linear_probe, base.linprobe_lrs, base.linprobe_epochs, base.linprobe_batch, base.linprobe_layers, base.linprobe_avgpool,
            base.linprobe_wd, base.linprobe_rate, base.linprobe_holdout) == (False, [0.001], 100, 1024, 4, False, 0.0, 0, 0.2)
    assert train.check_supported(base, lambda m: None) is None
    bad = ["--linprobe-lrs", "-1", "--linprobe-epochs", "0", "--linprobe-batch", "99999", "--linprobe-layers", "50", "--linprobe-avgpool",
           "--linprobe-wd", "-1", "--linprobe-rate", "-3", "--linprobe-holdout", "0.9"]
    for extra in (["--dino"], []):
        off, _ = train.parse_args(["--model", "vit_tiny", "--test_fold", "-1"] + bad + extra)
        assert not off.linear_probe and train.check_supported(off, lambda m: None) is None
        ref, _ = train.parse_args(["--model", "vit_tiny", "--test_fold", "-1"] + extra)
        differ = {k for k in vars(ref) if getattr(ref, k) != getattr(off, k)}
        assert differ == {"linprobe_lrs", "linprobe_epochs", "linprobe_batch", "linprobe_layers", "linprobe_avgpool", "linprobe_wd",
                          "linprobe_rate", "linprobe_holdout"}, differ
    on, _ = train.parse_args(["--model", "vit_tiny"] + PROBE + ["--linprobe-lrs", "0.1", "0.01", "--linprobe-epochs", "5", "--linprobe-batch", "64",
                                                                 "--linprobe-layers", "2", "--linprobe-avgpool", "--linprobe-wd", "1e-4",
                                                                 "--linprobe-rate", "2", "--linprobe-holdout", "0.5", "--knn-monitor"])
    assert train.check_supported(on, lambda m: None) is None
    assert (on.linprobe_lrs, on.linprobe_epochs, on.linprobe_batch, on.linprobe_layers, on.linprobe_avgpool, on.linprobe_wd, on.linprobe_rate,
            on.linprobe_holdout) == ([0.1, 0.01], 5, 64, 2, True, 1e-4, 2, 0.5)
    # ViT-B with four layers plus the pooled vector is 3840 features: inside the limit
    vb, _ = train.parse_args(["--model", "vit_base_patch16_224"] + PROBE + ["--linprobe-avgpool"])
    assert train.check_supported(vb, lambda m: None) is None


@pytest.mark.parametrize("name,knn,probe,want", [
    ("top1", True, False, "knn_top1"), ("auc_per_slide", True, False, "knn_auc_per_slide"), ("knn_top1", True, False, "knn_top1"),      # as before
    ("top1", True, True, "knn_top1"), ("auc_per_patch", True, True, "knn_auc_per_patch"), ("linear_auc_per_slide", True, True, "linear_auc_per_slide"),
    ("linear_loss", True, True, "linear_loss"), ("knn_auc_per_slide", True, True, "knn_auc_per_slide"),
    ("top1", False, True, "linear_top1"), ("loss", False, True, "linear_loss"), ("auc_per_slide", False, True, "linear_auc_per_slide"),
    ("linear_top1", False, True, "linear_top1"),
    ("top1", False, False, "top1"), ("loss", False, False, "loss"),
])
def test_eval_metric_resolution(name, knn, probe, want):
    assert _train().resolve_eval_metric(name, knn, probe) == want


def test_probe_checks_load_no_library_and_keep_the_process_clean():
    """The probe's depth and width checks read plain tables: check_supported loads no library, so a refused --amp-dtype float16
    command line has not chosen a library build for the process."""
    code = ("import os, sys; sys.path.insert(0, %r); import train\n"
            "a, _ = train.parse_args(['--model', 'vit_base_patch16_224', '--dino', '--linear-probe', '--linprobe-avgpool', '--amp'])\n"
            "assert train.check_supported(a, lambda m: None) is None\n"
            "a, _ = train.parse_args(['--model', 'vit_tiny', '--dino', '--linear-probe', '--linprobe-layers', '13', '--amp'])\n"
            "try:\n    train.check_supported(a, lambda m: None)\n    raise AssertionError('accepted')\nexcept SystemExit as e:\n    assert '--linprobe-layers' in str(e)\n"
            "assert 'gipvit._lib' not in sys.modules and 'gipvit.engine' not in sys.modules and 'GIPVIT_ACT_FORMAT' not in os.environ" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "GIPVIT_ACT_FORMAT"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-800:]
    from gipvit import archs, engine, models
    assert engine.ARCHS is archs.ARCHS and models.MODEL_REGISTRY is archs.MODEL_REGISTRY and models.resolve_arch is archs.resolve_arch


def test_eval_metric_names_accepted():
    train = _train()
    for flags in (["--eval-metric", "loss"], ["--eval-metric", "linear_auc_per_slide"], ["--knn-monitor", "--eval-metric", "auc_per_patch"],
                  ["--knn-monitor", "--eval-metric", "linear_loss"], ["--num-classes", "1", "--eval-metric", "top1"]):
        args, _ = train.parse_args(["--model", "vit_tiny"] + PROBE + flags)
        assert train.check_supported(args, lambda m: None) is None, flags
    both, _ = train.parse_args(["--model", "vit_tiny", "--knn-monitor"] + PROBE)
    assert train.monitor_metric_names(both) == ["knn_top1", "knn_auc_per_patch", "knn_auc_per_slide", "linear_top1", "linear_loss",
                                                "linear_auc_per_patch", "linear_auc_per_slide"]
    one, _ = train.parse_args(["--model", "vit_tiny", "--num-classes", "1"] + PROBE)
    assert train.monitor_metric_names(one) == ["linear_top1", "linear_loss"]


@pytest.mark.parametrize("knn_rate,probe_rate", [(2, 0), (2, 1), (1, 0), (3, 2)])
def test_summary_rows_keep_their_columns_whichever_monitor_ran(tmp_path, knn_rate, probe_rate):
    """summary.csv's header is written once: five epochs with the monitors on different schedules, written the way the driver
    writes them and read back by name, give every value under its own header and empty cells where a monitor did not run."""
    import csv
    from collections import OrderedDict
    train = _train()
    knn = ["knn_top1", "knn_auc_per_patch", "knn_auc_per_slide"]
    lin = ["linear_top1", "linear_loss", "linear_auc_per_patch", "linear_auc_per_slide"]
    fn, epochs, want = tmp_path / "summary.csv", 5, []
    for e in range(epochs):
        ev = OrderedDict()
        if (e + 1) % knn_rate == 0:
            ev.update((n, 100.0 * e + i) for i, n in enumerate(knn))
        if e == epochs - 1 or (probe_rate >= 1 and (e + 1) % probe_rate == 0):
            ev.update((n, 1000.0 * e + 50 + i) for i, n in enumerate(lin))            # (the probe reports after the monitor)
        row = train.summary_row(e, OrderedDict(loss=0.5 + e), ev, knn + lin, 1e-3)
        assert list(row) == ["epoch", "train_loss"] + ["eval_" + n for n in knn + lin] + ["lr"]
        with open(fn, "a") as f:
            w = csv.DictWriter(f, fieldnames=row.keys())
            if e == 0:
                w.writeheader()
            w.writerow(row)
        want.append(ev)
    rows = list(csv.DictReader(open(fn)))
    assert len(rows) == epochs
    for e, (r, ev) in enumerate(zip(rows, want)):
        assert int(r["epoch"]) == e and float(r["train_loss"]) == 0.5 + e and float(r["lr"]) == 1e-3
        for n in knn + lin:
            assert r["eval_" + n] == (str(ev[n]) if n in ev else ""), (e, n)
    # validate()'s metrics, which no monitor names, keep their own order in front
    sup = train.summary_row(0, OrderedDict(loss=1.0, auc=0.5), OrderedDict(loss=0.7, top1=50.0), [], 1e-3)
    assert list(sup) == ["epoch", "train_loss", "train_auc", "eval_loss", "eval_top1", "lr"]
