"""GPU: gv_mil_train / gv_mil_predict against the fp64 autograd + torch.optim.Adam reference of tests/test_mil_host.py, exact
closed-form probes (uniform attention, one-hot attention, one Adam step by hand), bitwise properties (run to run, NaN rows no bag
covers, a bag listed twice, predict split over two calls), bad bags, MilProbe on a real encoder against the same procedure
through the host reference, the needle bags, and the driver.

Bounds: Adam's moments 2e-6 and epoch mean losses 4e-6 (the linear probe's bounds: both are linear or quadratic in the
gradient); parameters max(4 * gap32(case), 2e-6), gap32 being the f32-vs-f64 gap of the reference itself (test_mil_host.py);
predict 2e-6 on prob / attn / score, 4e-6 on the mean loss.  Every test prints its figures.

Measured on an MI355X, max |gpu - f64| per case (F-L-C-batch):
    case            params (bound; gap32)            m         v         epoch loss   predict: prob     attn      score     mean loss
    4-16-1-1        4.9e-8 (2.0e-6; 4.9e-8)          5.4e-12   1.9e-16   0            0         3.1e-8    2.9e-8    0
    36-128-2-3      1.4e-7 (2.0e-6; 8.7e-8)          4.8e-8    1.4e-8    4.0e-8       4.9e-8    4.5e-9    6.6e-8    5.6e-8
    192-256-3-8     5.1e-7 (7.7e-6; 1.9e-6)          1.2e-8    3.1e-9    6.2e-8       3.2e-8    2.6e-8    8.3e-8    1.1e-8
    388-16-2-3      1.4e-8 (2.0e-6; 1.4e-7)          1.9e-8    8.2e-9    2.1e-8       2.3e-8    1.6e-8    7.2e-8    2.3e-8
The worst parameter element is attention_U.weight[133, 95] of the third case; no case needs the 4 x gap32 part of its bound.
One Adam step by hand: m and v of the classifier 0.5 ulp, the parameter 7.2e-8 (one ulp of it).  MilProbe on vit_tiny features:
parameters 1.5e-7 (gap32 3.7e-7), m 4.2e-8, epoch loss 3.1e-8.  Needle bags: AUC 1.0, least attention share 0.643 (the fp64
reference: 0.643).  DESIGN.md section 4 records these."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from probe_bits_cases import mil_train_gpu as _train_gpu, pad as _pad
from test_mil_host import (BETA1, BETA2, CASES, CASE_IDS, EPS, NAMES, NEEDLE, case_reference, cosine_scale, draw_params, mil_predict_reference,
                           mil_reference, needle_bags, needle_check, pack)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
f32 = torch.float32
STATE_BOUND, LOSS_BOUND = 2e-6, 4e-6


def _poison_workspace(dev, batch, max_bag, L, C, F):
    """The scratch ops.mil_* keep per device, all-ones bit patterns (NaN) for the next call: a slot a launch reads without an
    earlier launch having written it would show as a NaN in the result."""
    from gipvit import ops
    ops._scratch("mil", dev, batch, max_bag, L, C, F).fill_(255)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _worst(got_packed, ref, L, C, F):
    """max |gpu - f64| over the tensors of a NAMES-keyed reference dict -> (error, the tensor's name, the element's index)."""
    from gipvit.mil import param_views
    worst = (0.0, None, None)
    for k, t in param_views(got_packed, L, C, F).items():
        d = (t.double() - ref[k].reshape(t.shape)).abs()
        if float(d.max()) >= worst[0]:
            worst = (float(d.max()), k, tuple(int(i) for i in np.unravel_index(int(d.argmax()), t.shape)))
    return worst


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_train_matches_the_f64_reference(dev, i):
    c = CASES[i]
    s, (P, m, v, loss), gap, _ = case_reference(i)
    L, C, F = c["L"], c["C"], c["F"]
    got = _train_gpu(dev, s["x"], s["ptr"], s["labels"], pack(s["params0"], L, C, F), s["perms"], c["batch"], L, C, c["lr"], c["wd"], ldx=c["ldx"])
    ep, em, ev = _worst(got[0], P, L, C, F), _worst(got[1], m, L, C, F), _worst(got[2], v, L, C, F)
    el = float((got[3].double() / len(c["sizes"]) - loss).abs().max())
    bound = max(4 * gap, STATE_BOUND)
    print(f"max |gpu - f64|: params {ep[0]:.3e} at {ep[1]}{ep[2]} (bound {bound:.3e}, gap32 {gap:.3e})  m {em[0]:.3e} at {em[1]}{em[2]}  "
          f"v {ev[0]:.3e}  epoch loss {el:.3e}")
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert em[0] <= STATE_BOUND and ev[0] <= STATE_BOUND and el <= LOSS_BOUND
    assert ep[0] <= bound


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_predict_matches_the_f64_reference(dev, i):
    from gipvit import ops
    c = CASES[i]
    s, (P, _, _, _), _, _ = case_reference(i)
    L, C, F = c["L"], c["C"], c["F"]
    P32 = {k: t.to(f32) for k, t in P.items()}
    prob, attn, score, loss = mil_predict_reference(P32, s["x"], s["ptr"], s["labels"])
    n, mb = len(c["sizes"]), max(c["sizes"])
    packed = pack(P32, L, C, F).to(dev)
    x = _pad(s["x"], c["ldx"]).to(dev)[:, :F]
    ptr, y = torch.from_numpy(s["ptr"].astype(np.int32)).to(dev), s["labels"].to(dev, torch.int32)
    _poison_workspace(dev, n, mb, L, C, F)
    full = ops.mil_predict(packed, x, ptr, L, C, mb, labels=y, want_attn=True, want_score=True)
    bare = ops.mil_predict(packed, x, ptr, L, C, mb)                         # no labels, no tile outputs
    part = ops.mil_predict(packed, x, ptr, L, C, mb, labels=y, want_attn=True)
    torch.cuda.synchronize()
    assert list(bare) == ["prob"] and torch.equal(_bits(bare["prob"]), _bits(full["prob"]))
    assert torch.equal(_bits(part["prob"]), _bits(full["prob"])) and torch.equal(_bits(part["attn"]), _bits(full["attn"]))
    assert torch.equal(_bits(part["loss"]), _bits(full["loss"])) and "score" not in part
    errs = (float((full["prob"].cpu().double() - prob).abs().max()), float((full["attn"].cpu().double() - attn).abs().max()),
            float((full["score"].cpu().double() - score).abs().max()), abs(float(full["loss"].cpu().double()) - float(loss)) / n)
    print("max |gpu - f64|: prob %.3e  attn %.3e  score %.3e  mean loss %.3e" % errs)
    assert full["prob"].shape == (n, C) and full["attn"].shape == (len(s["x"]),)
    assert max(errs[:3]) <= STATE_BOUND and errs[3] <= LOSS_BOUND


# ---- exact probes
def _zero_gate(L, C, F, w=0.5, bw=0.25, wc_row=None):
    """V = U = 0 and zero gate biases: t = 0, g = 1/2, u = 0, so every score is bw.  Equal classifier rows: p = 1/C."""
    P = {"attention_V.weight": torch.zeros(L, F), "attention_V.bias": torch.zeros(L), "attention_U.weight": torch.zeros(L, F),
         "attention_U.bias": torch.zeros(L), "attention_w.weight": torch.full((1, L), w), "attention_w.bias": torch.tensor([bw]),
         "classifier.weight": (torch.zeros(F) if wc_row is None else wc_row).repeat(C, 1), "classifier.bias": torch.full((C,), 0.125)}
    return P


def _grid(n, F, seed):
    """Rows on the grid of eighths in [-2, 2]: their sums over up to 4096 rows and their power-of-two means are exact in f32."""
    return torch.randint(-16, 17, (n, F), generator=torch.Generator().manual_seed(seed)).to(f32) / 8


def _ulps(got, want):
    """|got - want| in units of the f32 spacing at want (want: float64 array of the exact values)."""
    want32 = np.asarray(want, dtype=np.float64).astype(np.float32)
    return np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_uniform_probe(dev, C):
    """a_i = 1/n: exactly for n a power of two, within 1 ulp otherwise; a pad row in the softmax denominator (a 64-row tile holds
    63, 65 - 64 or 129 - 128 live rows) would move it.  Scores are bw exactly, p = 1/C and the loss ln C within 1 ulp."""
    from gipvit import ops
    L, F = 16, 4
    sizes = [1, 2, 63, 64, 65, 128, 129]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = _grid(int(ptr[-1]), F, 1)
    P = _zero_gate(L, C, F, wc_row=torch.tensor([0.5, -1.0, 0.25, 2.0]))
    labels = torch.tensor([i % C for i in range(len(sizes))], dtype=torch.int32)
    _poison_workspace(dev, len(sizes), 129, L, C, F)
    out = ops.mil_predict(pack(P, L, C, F).to(dev), x.to(dev), torch.from_numpy(ptr).to(dev), L, C, 129, labels=labels.to(dev), want_attn=True, want_score=True)
    torch.cuda.synchronize()
    attn, score, prob = out["attn"].cpu().numpy(), out["score"].cpu().numpy(), out["prob"].cpu().numpy()
    assert (score == np.float32(0.25)).all()
    for b, n in enumerate(sizes):
        a = attn[ptr[b]:ptr[b + 1]]
        bad = np.nonzero(_ulps(a, np.full(n, 1.0 / n)) > (0 if n in (1, 2, 64, 128) else 1))[0]
        assert not len(bad), f"bag of n = {n}: row {int(bad[0])} has a = {a[bad[0]]!r}, 1/n = {1.0 / n!r}"
    assert _ulps(prob, np.full(prob.shape, 1.0 / C)).max() <= 1
    want = len(sizes) * np.log(float(C))
    print(f"C = {C}: loss sum {float(out['loss'].cpu()):.9g}, {len(sizes)} ln C = {want:.9g}")
    if C == 1:
        assert float(out["loss"].cpu()) == 0.0
    else:
        assert abs(float(out["loss"].cpu()) - want) <= len(sizes) * np.spacing(np.float32(np.log(float(C))))


def _one_step(dev, x, ptr, labels, P, L, C, bag, beta1=0.0, lr=1e-3, scale=0.0, wd=0.0):
    F = x.shape[1]
    return _train_gpu(dev, x, ptr, labels, pack(P, L, C, F), np.array([[bag]]), 1, L, C, lr, wd, beta1=beta1, scale=scale)


@pytest.mark.parametrize("n", [1, 2, 64, 128])
def test_uniform_probe_pools_the_exact_mean(dev, n):
    """With beta1 = 0 Adam's first moment is the gradient itself.  Zero classifier: p = 1/2 exactly, dl = (-1/2, +1/2), so
    m[Wc[0]] = -z / 2 and m[Wc[1]] = +z / 2 bit for bit, z the exact mean of the bag's rows on the grid of eighths."""
    from gipvit.mil import param_views
    L, C, F = 16, 2, 8
    x = _grid(n + 6, F, n)
    ptr = np.array([3, 3 + n])                                              # rows before and after the bag belong to no bag
    P = _zero_gate(L, C, F)
    _, m, _, loss = _one_step(dev, x, ptr, [0], P, L, C, 0)
    z = x[3:3 + n].double().mean(0)
    got = param_views(m, L, C, F)["classifier.weight"]
    assert torch.equal(got[0].double(), -z / 2) and torch.equal(got[1].double(), z / 2), (n, got, z)
    assert _ulps(loss.numpy(), [np.log(2.0)]).max() <= 1


@pytest.mark.parametrize("n,sel", [(1, 0), (64, 63), (65, 64), (129, 0), (129, 63), (129, 64), (129, 128), (200, 199)])
def test_selector_probe(dev, n, sel):
    """One row's score exceeds the rest by more than 200: the attention is one-hot and z is that row bit for bit (read back as
    m[Wc] = -+z / 2 with beta1 = 0 and a zero classifier).  A shifted or tile-edge row would hand back a neighbour."""
    from gipvit import ops
    from gipvit.mil import param_views
    L, C, F = 16, 2, 8
    g = torch.Generator().manual_seed(1000 * n + sel)
    x = torch.randn(n, F, generator=g)
    x[:, 0] = 0.0
    x[sel, 0] = 1.0                                                         # the flag column: tanh(20 * 1) against tanh(0)
    P = _zero_gate(L, C, F, w=400.0 / L, bw=0.0)
    P["attention_V.weight"][:, 0] = 20.0
    P["attention_U.bias"][:] = 20.0
    ptr = np.array([0, n])
    out = ops.mil_predict(pack(P, L, C, F).to(dev), x.to(dev), torch.from_numpy(ptr.astype(np.int32)).to(dev), L, C, n, want_attn=True, want_score=True)
    score, attn = out["score"].cpu(), out["attn"].cpu()
    rest = torch.cat([score[:sel], score[sel + 1:]])
    assert n == 1 or float(score[sel] - rest.max()) > 200.0
    onehot = torch.zeros(n)
    onehot[sel] = 1.0
    assert torch.equal(attn, onehot), (n, sel, attn.nonzero().reshape(-1).tolist())
    _, m, _, _ = _one_step(dev, x, ptr, [1], P, L, C, 0)
    got = param_views(m, L, C, F)["classifier.weight"]
    assert torch.equal(_bits(got[0]), _bits(0.5 * x[sel])) and torch.equal(_bits(got[1]), _bits(-0.5 * x[sel])), (n, sel)


def test_one_adam_step_by_hand(dev):
    """The uniform probe gives the gradient exactly (wd = 0): g[Wc[c]] = (1/2 - [c == y]) z, g[bc] = 1/2 - [c == y], every other
    gradient is zero (equal classifier rows: dz = 0).  m = (1 - beta1) g and v = (1 - beta2) g^2 within 1 ulp of the exact
    products, the parameter moves by lr m-hat / (sqrt(v-hat) + eps) = lr g / (|g| + eps), the rest does not move a bit."""
    from gipvit.mil import param_views
    L, C, F, n, lr = 16, 2, 8, 64, 1e-3
    x = _grid(n, F, 5)
    P = _zero_gate(L, C, F, wc_row=torch.tensor([0.5, -1.0, 0.25, 2.0, 0.0, 1.0, -0.5, 0.125]))
    p0 = pack(P, L, C, F)
    p1, m, v, _ = _train_gpu(dev, x, np.array([0, n]), [1], p0, np.array([[0]]), 1, L, C, lr, 0.0, scale=1.0)
    z = x.double().mean(0)
    g = {k: torch.zeros_like(t, dtype=torch.float64) for k, t in P.items()}
    g["classifier.weight"] = torch.stack([0.5 * z, -0.5 * z])
    g["classifier.bias"] = torch.tensor([0.5, -0.5], dtype=torch.float64)
    b1, b2 = float(np.float32(1) - np.float32(BETA1)), float(np.float32(1) - np.float32(BETA2))      # as the kernel forms them, in f32
    for k in NAMES:
        gm, gv, gp = (param_views(t, L, C, F)[k] for t in (m, v, p1))
        if k.startswith("classifier"):
            um, uv = _ulps(gm.numpy(), (b1 * g[k]).numpy()).max(), _ulps(gv.numpy(), (b2 * g[k] * g[k]).numpy())
            uv = uv[np.isfinite(uv)].max()                                  # (a zero gradient: 0 against 0)
            want = P[k].double() - lr * g[k] / (g[k].abs() + EPS)
            ep = (gp.double() - want).abs()
            print(f"{k}: m {um:.2f} ulp, v {uv:.2f} ulp, parameter {float(ep.max()):.3e}")
            assert um <= 1 and uv <= 1
            assert bool((ep <= torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64)) + 1e-6 * lr).all())
            assert bool(((gm == 0) == (g[k] == 0)).all())
        else:
            assert not gm.any() and not gv.any() and torch.equal(_bits(gp), _bits(P[k].reshape(gp.shape))), k


# ---- bitwise properties
def _small_case(seed=11, sizes=(3, 65, 2, 64, 5), F=12, L=32, C=3):
    g = torch.Generator().manual_seed(seed)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = torch.randn(int(ptr[-1]), F, generator=g)
    labels = torch.tensor([i % C for i in range(len(sizes))])
    return x, ptr, labels, draw_params(L, C, F, seed)


def test_run_to_run_and_uncovered_nan_rows(dev):
    """Two runs give the same bits, loss_sum included; so does a run over the same bags laid out between rows of NaN that no
    listed bag covers (rows in front of bag_ptr[0], whole unlisted bags, rows behind the last bag)."""
    L, C, F = 32, 3, 12
    x, ptr, labels, P0 = _small_case()
    perms = np.array([[4, 1, 0, 3, 2], [2, 3, 1, 4, 0]])
    run = lambda: _train_gpu(dev, x, ptr, labels, pack(P0, L, C, F), perms, 2, L, C, 1e-3, 1e-4)
    a, b = run(), run()
    assert all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a, b)) and all(bool(torch.isfinite(t).all()) for t in a)
    # bag k becomes bag 2k + 1 of a table whose even bags are 7 rows of NaN; 5 rows of NaN in front, 9 behind
    sizes = np.diff(ptr)
    rows, ptr2, at = [torch.full((5, F), float("nan"))], [5], 5
    for k, n in enumerate(sizes):
        rows += [torch.full((7, F), float("nan")), x[ptr[k]:ptr[k + 1]]]
        ptr2 += [at + 7, at + 7 + int(n)]
        at += 7 + int(n)
    rows.append(torch.full((9, F), float("nan")))
    labels2 = torch.zeros(len(ptr2) - 1, dtype=torch.int64)
    labels2[1::2] = labels
    c = _train_gpu(dev, torch.cat(rows), np.array(ptr2), labels2, pack(P0, L, C, F), 2 * perms + 1, 2, L, C, 1e-3, 1e-4, max_bag=65)
    assert all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a, c))


def test_a_bag_listed_twice_counts_twice(dev):
    L, C, F = 32, 3, 12
    x, ptr, labels, P0 = _small_case()
    perms = np.array([[1, 0, 1, 3, 3]])
    got = _train_gpu(dev, x, ptr, labels, pack(P0, L, C, F), perms, 3, L, C, 1e-3, 1e-4)
    P, m, v, loss = mil_reference(x, ptr, labels, P0, perms, 3, 1e-3, 1e-4)
    once = mil_reference(x, ptr, labels, P0, np.array([[1, 0, 3]]), 3, 1e-3, 1e-4)
    em, ev, el = _worst(got[1], m, L, C, F)[0], _worst(got[2], v, L, C, F)[0], abs(float(got[3][0]) / 5 - float(loss[0]))
    print(f"max |gpu - f64|: m {em:.3e}  v {ev:.3e}  mean loss {el:.3e}; listed once the moments differ by {_worst(got[1], once[1], L, C, F)[0]:.3e}")
    assert em <= STATE_BOUND and ev <= STATE_BOUND and el <= LOSS_BOUND and _worst(got[1], once[1], L, C, F)[0] > 1e-4


def test_predict_split_over_two_calls(dev):
    """70 bags (more than one group of 64): the loss of one call and of two calls over 30 + 40 bags, the second accumulating,
    have the same bits; so have the probabilities."""
    from gipvit import ops
    L, C, F = 16, 3, 8
    g = torch.Generator().manual_seed(3)
    sizes = torch.randint(1, 6, (70,), generator=g).numpy()
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    x = torch.randn(int(sizes.sum()), F, generator=g).to(dev)
    y = torch.randint(0, C, (70,), generator=g).to(dev, torch.int32)
    packed = pack(draw_params(L, C, F, 3), L, C, F).to(dev)
    bags = torch.arange(70, dtype=torch.int32, device=dev)
    _poison_workspace(dev, 64, 5, L, C, F)
    one = ops.mil_predict(packed, x, ptr, L, C, 5, labels=y)
    first = ops.mil_predict(packed, x, ptr, L, C, 5, labels=y, bags=bags[:30])
    second = ops.mil_predict(packed, x, ptr, L, C, 5, labels=y, bags=bags[30:], loss=first["loss"])
    torch.cuda.synchronize()
    assert torch.equal(_bits(second["loss"]), _bits(one["loss"])) and float(one["loss"]) > 0
    assert torch.equal(_bits(torch.cat([first["prob"], second["prob"]])), _bits(one["prob"]))
    want = mil_predict_reference(draw_params(L, C, F, 3), x.cpu(), ptr.cpu().numpy(), y.cpu().long())
    assert abs(float(one["loss"].cpu().double()) - float(want[3])) / 70 <= LOSS_BOUND


# ---- bad bags
def test_bad_bags_contribute_nothing(dev):
    """An empty bag, one longer than max_bag, one whose rows end past N, one with a label outside [0, C), and bag indices outside
    the table, mixed into the visiting order: the result has the bits of the run over the good bags alone.  (A step averages
    over its good bags; the all-bad last step changes nothing.)"""
    L, C, F = 32, 3, 12
    x, ptr, labels, P0 = _small_case()                                      # good bags of 3, 65, 2, 64, 5 rows
    clean = _train_gpu(dev, x, ptr, labels, pack(P0, L, C, F), np.array([[0, 1, 2, 3, 4]]), 3, L, C, 1e-3, 1e-4, max_bag=65)
    g = [x[ptr[k]:ptr[k + 1]] for k in range(5)]
    junk = lambda n: torch.randn(n, F, generator=torch.Generator().manual_seed(n))
    # table: g0, EMPTY, g1, LONG (70 rows), g2, BADLABEL (4 rows), g3, g4, PASTN (starts inside x, ends 50 rows past it)
    parts = [g[0], g[1], junk(70), g[2], junk(4), g[3], g[4], junk(10)]
    sizes = [3, 0, 65, 70, 2, 4, 64, 5, 60]
    ptr2 = np.concatenate([[0], np.cumsum(sizes)])
    x2 = torch.cat(parts)
    assert ptr2[-1] == x2.shape[0] + 50
    labels2 = torch.tensor([0, 0, 1, 0, 2, 7, 0, 1, 0])
    labels2[5] = 7
    order = np.array([[0, 1, 2, 4, 3, 6, 5, 7, 8, -1, 99]])                 # steps of 4: {g0 EMPTY g1 g2} {LONG g3 BADLABEL g4} {PASTN -1 99}
    dirty = _train_gpu(dev, x2, ptr2, labels2, pack(P0, L, C, F), order, 4, L, C, 1e-3, 1e-4, max_bag=65)
    assert all(bool(torch.isfinite(t).all()) for t in dirty)
    for name, a, b in zip(("params", "m", "v", "loss_sum"), clean, dirty):
        assert torch.equal(_bits(a), _bits(b)), name
    neg = labels2.clone()
    neg[5] = -1
    dirty2 = _train_gpu(dev, x2, ptr2, neg, pack(P0, L, C, F), order, 4, L, C, 1e-3, 1e-4, max_bag=65)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(clean, dirty2))


def test_predict_of_bad_bags(dev):
    """predict: a bad bag's probabilities are zeros, its rows get no attention; a label outside [0, C) only leaves the loss out."""
    from gipvit import ops
    L, C, F = 16, 2, 8
    g = torch.Generator().manual_seed(8)
    sizes = [4, 0, 9, 3]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = torch.randn(16, F, generator=g)
    P = draw_params(L, C, F, 8)
    y = torch.tensor([1, 0, 5, 0], dtype=torch.int32)
    out = ops.mil_predict(pack(P, L, C, F).to(dev), x.to(dev), torch.from_numpy(ptr).to(dev), L, C, 4, labels=y.to(dev), want_attn=True)
    prob, attn = out["prob"].cpu(), out["attn"].cpu()
    want = mil_predict_reference(P, x, ptr.astype(np.int64))
    assert not prob[1].any() and not prob[2].any() and not attn[4:13].any()             # empty; 9 rows > max_bag 4
    assert float((prob[[0, 3]].double() - want[0][[0, 3]]).abs().max()) <= STATE_BOUND
    loss = -(torch.log(want[0][0, 1]) + torch.log(want[0][3, 0]))
    assert abs(float(out["loss"].cpu()) - float(loss)) <= 2 * LOSS_BOUND


# ---- MilProbe on a real encoder
def _runner(dev, img=64, batch=8, seed=0):
    from gipvit.engine import FeatureExtractor
    from gipvit import models as M
    runner = FeatureExtractor("vit_tiny", img, batch=batch, device=dev)
    runner.load_state(M.init_vit_state("vit_tiny", img, 0, seed=seed))
    return runner


def test_mil_probe_matches_the_host_reference_on_the_runners_features(dev):
    from gipvit import data as D
    from gipvit.linprobe import epoch_permutations
    from gipvit.mil import MilProbe, init_params, mil_metrics, param_views
    runner = _runner(dev)
    L, C, F, epochs, batch, lr, wd, seed = 16, 2, 192, 3, 2, 1e-3, 1e-4, 5
    probe = MilProbe(runner, num_classes=C, hidden=L, lr=lr, weight_decay=wd, epochs=epochs, batch=batch, n_last=1, seed=seed)
    bank_loader, query_loader = D.SyntheticSlides(5, 8, 64, tiles_per_iter=5, seed=11), D.SyntheticSlides(4, 6, 64, tiles_per_iter=4, seed=23)
    assert probe.fit(bank_loader) == 5
    got = probe.evaluate(query_loader)
    assert list(got) == ["mil_top1", "mil_loss", "mil_auc_per_slide"]
    sd = probe.state_dict()
    assert list(sd) == NAMES and sd["attention_V.weight"].shape == (L, F) and sd["classifier.weight"].shape == (C, F)
    # the same procedure through the host reference on the probe's own cached features
    fb, ptrb, yb, _ = probe._collect(bank_loader)
    fq, ptrq, yq, _ = probe._collect(query_loader)
    assert ptrb.tolist() == [0, 8, 16, 24, 32, 40] and yb.tolist() == [0, 1, 0, 1, 0] and ptrq.tolist() == [0, 6, 12, 18, 24]
    P0 = {k: t.clone() for k, t in param_views(init_params(L, C, F, seed), L, C, F).items()}
    kw = dict(x=fb.cpu(), ptr=ptrb.astype(np.int64), labels=torch.from_numpy(yb), params0=P0, perms=epoch_permutations(5, epochs, seed), batch=batch,
              lr=lr, wd=wd)
    P, m, v, loss = mil_reference(**kw)
    P32 = mil_reference(dtype=f32, **kw)[0]
    gap = max(float((P32[k].double() - P[k]).abs().max()) for k in NAMES)
    ep, em = _worst(probe.params.cpu(), P, L, C, F), _worst(probe.m.cpu(), m, L, C, F)
    el = float((torch.tensor(probe.train_loss, dtype=torch.float64) - loss).abs().max())
    print(f"fit against the reference: params {ep[0]:.3e} at {ep[1]}{ep[2]} (gap32 {gap:.3e})  m {em[0]:.3e}  epoch loss {el:.3e}")
    assert gap <= 2e-5 and ep[0] <= max(4 * gap, STATE_BOUND) and em[0] <= STATE_BOUND and el <= LOSS_BOUND
    prob, attn, score, ql = mil_predict_reference(P, fq.cpu(), ptrq.astype(np.int64), torch.from_numpy(yq))
    want = mil_metrics(prob.numpy(), yq, float(ql) / 4)
    print("probe", dict(got), "reference", dict(want))
    assert got["mil_top1"] == want["mil_top1"] and abs(got["mil_loss"] - want["mil_loss"]) <= LOSS_BOUND
    assert abs(got["mil_auc_per_slide"] - want["mil_auc_per_slide"]) <= 1e-6
    tiles = probe.tile_attention(query_loader)
    assert len(tiles) == 4 and all(a.shape == (6,) and s.shape == (6,) for a, s in tiles)
    assert all(abs(float(a.double().sum()) - 1.0) <= 1e-6 for a, _ in tiles)
    assert float((torch.cat([a for a, _ in tiles]).double() - attn).abs().max()) <= 4 * STATE_BOUND
    # features read back from files train without an encoder
    alone = MilProbe(None, num_classes=C, hidden=L, lr=lr, weight_decay=wd, epochs=epochs, batch=batch, seed=seed, features=F)
    alone.train(fb, ptrb, yb)
    assert torch.equal(_bits(alone.params), _bits(probe.params))


def test_mil_probe_feeds_the_centred_window_of_larger_tiles(dev):
    from gipvit import data as D
    from gipvit.mil import MilProbe
    runner = _runner(dev)
    probe = MilProbe(runner, hidden=16, epochs=1, batch=2, n_last=2)
    mb = next(iter(D.SyntheticSlides(1, 6, 96, tiles_per_iter=6, seed=5)))      # 96-px tiles into the 64-px runner
    manual = runner.probe_features(mb["Data"][:, 16:80, 16:80, :].contiguous().to(dev), 2)
    assert probe.F == 384 and torch.equal(_bits(probe.features(mb["Data"])), _bits(manual))


# ---- needle bags on the device
def test_needle_bags_on_the_device(dev):
    from gipvit import ops
    c = NEEDLE
    L, C, F = c["L"], c["C"], c["F"]
    x, ptr, labels, _ = needle_bags(24, c["seed"])
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    perms = np.stack([rng.permutation(24) for _ in range(c["epochs"])])
    P, _, _, loss = _train_gpu(dev, x, ptr, labels, pack(draw_params(L, C, F, c["seed"]), L, C, F), perms, c["batch"], L, C, c["lr"], c["wd"])
    xq, ptrq, yq, needle = needle_bags(12, c["seed"] + 1)
    out = ops.mil_predict(P.to(dev), xq.to(dev), torch.from_numpy(ptrq.astype(np.int32)).to(dev), L, C, int(np.diff(ptrq).max()), want_attn=True)
    share = needle_check(out["prob"].cpu().numpy(), out["attn"].cpu().numpy(), ptrq, yq.numpy(), needle)
    print(f"needle bags: epoch loss {float(loss[0]) / 24:.4f} -> {float(loss[-1]) / 24:.4f}, least attention share on the needles {share:.3f}")


# ---- the driver
def test_driver_writes_mil_metrics_and_picks_model_best_on_them(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import train
    base = ["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--out-dim", "1024", "--batches-per-epoch", "2", "--epochs", "2",
            "--lr", "1e-4", "--warmup-epochs", "0", "--log-interval", "1", "--output", str(tmp_path), "--seed", "3", "--mil-probe",
            "--mil-hidden", "16", "--mil-epochs", "3", "--mil-batch", "2"]
    names = ["eval_mil_top1", "eval_mil_loss", "eval_mil_auc_per_slide"]
    knn = ["eval_knn_top1", "eval_knn_auc_per_patch", "eval_knn_auc_per_slide"]
    lin = ["eval_linear_top1", "eval_linear_loss", "eval_linear_auc_per_patch", "eval_linear_auc_per_slide"]
    # the default --mil-rate 0: after the last epoch only; model_best follows --eval-metric mil_auc_per_slide
    assert train.main(base + ["--experiment", "last", "--eval-metric", "mil_auc_per_slide"]) == 0
    with open(tmp_path / "last" / "summary.csv") as f:
        header = f.readline().strip().split(",")
    rows = list(csv.DictReader(open(tmp_path / "last" / "summary.csv")))
    assert header == ["epoch", "train_loss"] + names + ["lr"]
    assert len(rows) == 2 and all(rows[0][n] == "" for n in names) and all(rows[1][n] != "" for n in names)
    assert 0.0 <= float(rows[1]["eval_mil_top1"]) <= 100.0 and float(rows[1]["eval_mil_loss"]) > 0 and 0.0 <= float(rows[1]["eval_mil_auc_per_slide"]) <= 1.0
    best = torch.load(tmp_path / "last" / "model_best.pth.tar", weights_only=True)
    assert best["epoch"] == 1 and best["metric"] == float(rows[1]["eval_mil_auc_per_slide"])
    assert "metric" not in torch.load(tmp_path / "last" / "checkpoint-0.pth.tar", weights_only=True)
    # all three monitors: the columns keep their order, the MIL probe's last; --mil-rate 1 fills every epoch; mil_loss is decreasing
    assert train.main(base + ["--experiment", "all", "--mil-rate", "1", "--knn-monitor", "--knn-k", "3", "--linear-probe", "--linprobe-epochs", "2",
                              "--linprobe-batch", "8", "--linprobe-layers", "1", "--eval-metric", "mil_loss"]) == 0
    with open(tmp_path / "all" / "summary.csv") as f:
        header = f.readline().strip().split(",")
    assert header == ["epoch", "train_loss"] + knn + lin + names + ["lr"]
    rows = list(csv.DictReader(open(tmp_path / "all" / "summary.csv")))
    assert len(rows) == 2 and all(r[n] != "" for r in rows for n in names + knn) and all(rows[0][n] == "" for n in lin)
    losses = [float(r["eval_mil_loss"]) for r in rows]
    best = torch.load(tmp_path / "all" / "model_best.pth.tar", weights_only=True)
    assert best["metric"] == min(losses) and best["epoch"] == (1 if losses[1] < losses[0] else 0)
    # a name no monitor of the run reports is refused with the other flags
    with pytest.raises(SystemExit) as e:
        train.main(base + ["--experiment", "bad", "--eval-metric", "auc_per_patch"])
    assert "--eval-metric" in str(e.value)
