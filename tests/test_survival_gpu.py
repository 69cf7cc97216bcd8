"""GPU: gv_surv_train / gv_surv_predict / gv_cox_eval against the fp64 references of tests/test_survival_host.py, exact
closed-form probes (equal risks over power-of-two risk sets, one Adam step by hand), bitwise properties (run to run, NaN rows no
bag covers, the risk bias, a step without an event, bad bags of each kind), SurvivalProbe on a real encoder against the same
procedure through the host reference, the needle bags, and the driver.

Bounds (the MIL probe's, tests/test_mil_gpu.py): Adam's moments 2e-6, epoch losses 4e-6, parameters max(4 * gap32(case), 2e-6),
gap32 being the f32-vs-f64 gap of the reference itself; predict 2e-6 on risk / attn / score; gv_cox_eval: exact counts and the
loss within 1e-10 max(1, |loss|) of numpy fp64.  Every test prints its figures.

Measured on an MI355X, max |gpu - f64| per case (F-L-batch):
    case          params (bound; gap32)            m         v         epoch loss   predict: risk     attn      score
    4-16-2        4.1e-8 (2.0e-6; 3.7e-8)          7.8e-9    2.6e-9    2.2e-8       3.2e-8    1.3e-8    4.9e-8
    36-128-3      1.7e-6 (2.0e-6; 1.9e-7)          2.2e-8    1.1e-8    2.7e-8       5.1e-8    1.5e-8    5.9e-8
    192-256-8     2.4e-6 (7.6e-6; 1.9e-6)          3.2e-8    1.7e-8    1.1e-7       7.5e-8    4.4e-8    7.6e-8
    388-16-64     3.6e-7 (2.0e-6; 4.6e-7)          3.5e-8    3.0e-8    5.7e-7       1.0e-7    6.3e-8    6.0e-8
The worst parameter elements are attention_V.weight[59, 11] (second case) and attention_U.weight[126, 129] (third): weights whose
gradient nearly cancels, which Adam moves as far as any other; the moments agree to 3.5e-8.  With a direction planted in the
features the last case measured 3.2e-6 against a bound of 2.3e-6 while the reference's own f32 run scattered from 5.7e-7 to 4.1e-6
between two hosts; the cases' features are therefore noise alone (tests/test_survival_host.py, case_setup).
Equal-risk probe: m[Wc] exact, loss_sum {4.1588831, 4}.  One Adam step by hand: m 0.50 ulp, v 0.47 ulp, parameter 7.4e-11.
gv_cox_eval, n in {1, 2, 63, 64, 65, 1000, 4097}: the six counts exact, |loss - numpy fp64| = 0 at the printed precision.
SurvivalProbe on vit_tiny features: parameters 1.2e-7 (gap32 2.5e-7), m 1.2e-8, epoch loss 4.8e-8.  Needle bags: C-index 1.0 over
24 pairs, needle risks >= -0.47, the others <= -1.08 (the fp64 reference's figures), least attention share 0.214.  DESIGN.md
section 4 records these."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from probe_bits_cases import surv_train_gpu as _train_gpu, pad as _pad
from test_mil_host import BETA1, BETA2, EPS, NAMES, cosine_scale, draw_params, pack
from test_survival_host import (CASES, CASE_IDS, NEEDLE, case_reference, cohort, needle_perms, needle_survival, surv_predict_reference,
                                surv_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
f32 = torch.float32
STATE_BOUND, LOSS_BOUND = 2e-6, 4e-6


def _poison_workspace(dev, batch, max_bag, L, F):
    """The scratch ops.surv_* keep per device, all-ones bit patterns (NaN) for the next call: a slot a launch reads without an
    earlier launch having written it would show as a NaN in the result."""
    from gipvit import ops
    ops._scratch("surv", dev, batch, max_bag, L, F).fill_(255)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _worst(got_packed, ref, L, F):
    from gipvit.mil import param_views
    worst = (0.0, None, None)
    for k, t in param_views(got_packed, L, 1, F).items():
        d = (t.double() - ref[k].reshape(t.shape)).abs()
        if float(d.max()) >= worst[0]:
            worst = (float(d.max()), k, tuple(int(i) for i in np.unravel_index(int(d.argmax()), t.shape)))
    return worst


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_train_matches_the_f64_reference(dev, i):
    c = CASES[i]
    s, (P, m, v, loss), gap, _ = case_reference(i)
    L, F = c["L"], c["F"]
    got = _train_gpu(dev, s["x"], s["ptr"], s["time"], s["event"], pack(s["params0"], L, 1, F), s["perms"], c["batch"], L, c["lr"], c["wd"], ldx=c["ldx"])
    ep, em, ev = _worst(got[0], P, L, F), _worst(got[1], m, L, F), _worst(got[2], v, L, F)
    el = float((got[3][:, 0].double() / got[3][:, 1].double() - loss).abs().max())
    bound = max(4 * gap, STATE_BOUND)
    print(f"max |gpu - f64|: params {ep[0]:.3e} at {ep[1]}{ep[2]} (bound {bound:.3e}, gap32 {gap:.3e})  m {em[0]:.3e} at {em[1]}{em[2]}  "
          f"v {ev[0]:.3e}  epoch loss {el:.3e}")
    assert all(bool(torch.isfinite(t).all()) for t in got)
    events = sum(int(s["event"][b]) for b in range(len(c["sizes"])))
    assert got[3][:, 1].tolist() == [float(events)] * c["epochs"]
    assert em[0] <= STATE_BOUND and ev[0] <= STATE_BOUND and el <= LOSS_BOUND
    assert ep[0] <= bound


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_predict_matches_the_f64_reference(dev, i):
    from gipvit import ops
    c = CASES[i]
    s, (P, _, _, _), _, _ = case_reference(i)
    L, F = c["L"], c["F"]
    P32 = {k: t.to(f32) for k, t in P.items()}
    risk, attn, score = surv_predict_reference(P32, s["x"], s["ptr"])
    n, mb = len(c["sizes"]), max(c["sizes"])
    packed = pack(P32, L, 1, F).to(dev)
    x = _pad(s["x"], c["ldx"]).to(dev)[:, :F]
    ptr = torch.from_numpy(s["ptr"].astype(np.int32)).to(dev)
    _poison_workspace(dev, min(n, 64), mb, L, F)
    full = ops.surv_predict(packed, x, ptr, L, mb, want_attn=True, want_score=True)
    bare = ops.surv_predict(packed, x, ptr, L, mb)
    part = ops.surv_predict(packed, x, ptr, L, mb, want_attn=True)
    torch.cuda.synchronize()
    assert list(bare) == ["risk"] and torch.equal(_bits(bare["risk"]), _bits(full["risk"]))
    assert torch.equal(_bits(part["risk"]), _bits(full["risk"])) and torch.equal(_bits(part["attn"]), _bits(full["attn"])) and "score" not in part
    errs = (float((full["risk"].cpu().double() - risk).abs().max()), float((full["attn"].cpu().double() - attn).abs().max()),
            float((full["score"].cpu().double() - score).abs().max()))
    print("max |gpu - f64|: risk %.3e  attn %.3e  score %.3e" % errs)
    assert full["risk"].shape == (n,) and full["attn"].shape == (len(s["x"]),)
    assert max(errs) <= STATE_BOUND


# ---- exact probes
def _zero_gate(L, F, w=0.5, bw=0.25, wc=None, bc=0.125):
    """V = U = 0 and zero gate biases: every score is bw, the attention uniform.  Wc = 0: every risk is bc."""
    return {"attention_V.weight": torch.zeros(L, F), "attention_V.bias": torch.zeros(L), "attention_U.weight": torch.zeros(L, F),
            "attention_U.bias": torch.zeros(L), "attention_w.weight": torch.full((1, L), w), "attention_w.bias": torch.tensor([bw]),
            "classifier.weight": (torch.zeros(F) if wc is None else wc).reshape(1, F), "classifier.bias": torch.tensor([bc])}


def _grid(n, F, seed):
    """Rows on the grid of eighths in [-2, 2]: their sums over up to 4096 rows and their power-of-two means are exact in f32."""
    return torch.randint(-16, 17, (n, F), generator=torch.Generator().manual_seed(seed)).to(f32) / 8


def _ulps(got, want):
    want32 = np.asarray(want, dtype=np.float64).astype(np.float32)
    return np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


def test_equal_risks_over_power_of_two_risk_sets(dev):
    """Zero gate and Wc = 0: every risk is bc, exp(theta - M) = 1 and S_i = |R_i|.  Eight bags at times 1 1 1 1 2 2 3 4 (risk sets of
    8, 4, 2, 1 entries), events at bags 0, 4, 6, 7 (E = 4): d theta_k = (sum_{events i, t_i <= t_k} 1 / |R_i| - e_k) / 4, exact
    in f32.  With beta1 = 0 the first moment of Wc is the gradient sum_k d theta_k z_k, z_k the exact mean of bag k's 1, 2, 4, ..
    rows on the grid of eighths: within 0.5 ulp (one rounding).  loss_sum = {sum log |R_i| within 1 ulp per term, E exactly}."""
    from gipvit.mil import param_views
    L, F = 16, 8
    sizes = [1, 2, 4, 8, 16, 64, 128, 2]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    x = _grid(int(ptr[-1]), F, 3)
    time, event = [1, 1, 1, 1, 2, 2, 3, 4], [1, 0, 0, 0, 1, 0, 1, 1]
    rset = {1: 8, 2: 4, 3: 2, 4: 1}
    dth = np.array([(sum(1.0 / rset[time[i]] for i in range(8) if event[i] and time[i] <= time[k]) - event[k]) / 4 for k in range(8)])
    P = _zero_gate(L, F)
    _, m, _, loss = _train_gpu(dev, x, ptr, time, event, pack(P, L, 1, F), np.arange(8)[None], 8, L, 1e-3, 0.0, beta1=0.0, scale=0.0)
    z = torch.stack([x[ptr[k]:ptr[k + 1]].double().mean(0) for k in range(8)])
    want = (torch.from_numpy(dth)[:, None] * z).sum(0)
    got = param_views(m, L, 1, F)["classifier.weight"][0]
    u = _ulps(got.numpy(), want.numpy())
    terms = [np.log(float(rset[time[i]])) for i in range(8) if event[i]]
    print(f"d theta {dth.tolist()}; m[Wc] within {u.max():.2f} ulp; loss_sum {loss[0].tolist()}, sum log|R| = {sum(terms):.9g}")
    assert abs(dth.sum()) == 0.0 and u.max() <= 0.5
    # a term's logf is within 1 ulp of the term; each of the E additions in step order rounds to half an ulp of the running sum
    tol = sum(float(np.spacing(np.float32(t))) for t in terms) + len(terms) * 0.5 * float(np.spacing(np.float32(sum(terms))))
    assert abs(float(loss[0, 0]) - sum(terms)) <= tol and float(loss[0, 1]) == 4.0
    assert not param_views(m, L, 1, F)["classifier.bias"].any()              # the risk bias: a gradient of exactly zero


def test_one_adam_step_by_hand(dev):
    """Two bags, zero gate, Wc = 0, times 1 < 2, both events: S = (2, 1), d theta = (1/2 (1/2 - 1), 1/2 (1/2 + 1 - 1)) = (-1/4, 1/4),
    g[Wc] = (z_1 - z_0) / 4 exactly; every other gradient is zero at wd = 0 (dz = d theta Wc = 0).  m, v within 1 ulp of the
    exact products, Wc moves by lr g / (|g| + eps), the rest does not move a bit."""
    from gipvit.mil import param_views
    L, F, lr = 16, 8, 1e-3
    x = _grid(64 + 16, F, 5)
    ptr = np.array([0, 64, 80])
    P = _zero_gate(L, F)
    p1, m, v, loss = _train_gpu(dev, x, ptr, [1.0, 2.0], [1, 1], pack(P, L, 1, F), np.array([[0, 1]]), 2, L, lr, 0.0, scale=1.0)
    g = (x[64:].double().mean(0) - x[:64].double().mean(0)) / 4
    b1, b2 = float(np.float32(1) - np.float32(BETA1)), float(np.float32(1) - np.float32(BETA2))
    for k in NAMES:
        gm, gv, gp = (param_views(t, L, 1, F)[k] for t in (m, v, p1))
        if k == "classifier.weight":
            um, uv = _ulps(gm[0].numpy(), (b1 * g).numpy()).max(), _ulps(gv[0].numpy(), (b2 * g * g).numpy())
            uv = uv[np.isfinite(uv)].max()
            want = -lr * g / (g.abs() + EPS)
            ep = (gp[0].double() - want).abs()
            print(f"{k}: m {um:.2f} ulp, v {uv:.2f} ulp, parameter {float(ep.max()):.3e}")
            assert um <= 1 and uv <= 1
            assert bool((ep <= torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64)) + 1e-6 * lr).all())
        else:
            assert not gm.any() and not gv.any() and torch.equal(_bits(gp), _bits(P[k].reshape(gp.shape))), k
    assert _ulps([float(loss[0, 0])], [np.log(2.0)]).max() <= 1 and float(loss[0, 1]) == 2.0


# ---- bitwise properties
def _small_case(seed=11, sizes=(3, 65, 2, 64, 5), F=12, L=32):
    g = torch.Generator().manual_seed(seed)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = torch.randn(int(ptr[-1]), F, generator=g)
    time = np.array([2.0, 1.0, 2.0, 3.5, 1.0], dtype=np.float32)[:len(sizes)]
    event = np.array([1, 0, 1, 1, 1])[:len(sizes)]
    return x, ptr, time, event, draw_params(L, 1, F, seed)


def test_run_to_run_and_uncovered_nan_rows(dev):
    L, F = 32, 12
    x, ptr, time, event, P0 = _small_case()
    perms = np.array([[4, 1, 0, 3, 2], [2, 3, 1, 4, 0]])
    run = lambda: _train_gpu(dev, x, ptr, time, event, pack(P0, L, 1, F), perms, 2, L, 1e-3, 1e-4)
    a, b = run(), run()
    assert all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a, b)) and all(bool(torch.isfinite(t).all()) for t in a)
    # bag k becomes bag 2k + 1 of a table whose even bags are 7 rows of NaN (time NaN too); 5 rows of NaN in front, 9 behind
    sizes = np.diff(ptr)
    rows, ptr2, at = [torch.full((5, F), float("nan"))], [5], 5
    for k, n in enumerate(sizes):
        rows += [torch.full((7, F), float("nan")), x[ptr[k]:ptr[k + 1]]]
        ptr2 += [at + 7, at + 7 + int(n)]
        at += 7 + int(n)
    rows.append(torch.full((9, F), float("nan")))
    time2, event2 = np.full(len(ptr2) - 1, np.nan, dtype=np.float32), np.zeros(len(ptr2) - 1, dtype=np.int64)
    time2[1::2], event2[1::2] = time, event
    c = _train_gpu(dev, torch.cat(rows), np.array(ptr2), time2, event2, pack(P0, L, 1, F), 2 * perms + 1, 2, L, 1e-3, 1e-4, max_bag=65)
    assert all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a, c))


def test_a_bag_listed_twice_is_two_tied_entries(dev):
    L, F = 32, 12
    x, ptr, time, event, P0 = _small_case()
    perms = np.array([[1, 0, 1, 3, 3]])
    got = _train_gpu(dev, x, ptr, time, event, pack(P0, L, 1, F), perms, 3, L, 1e-3, 1e-4)
    P, m, v, loss = surv_reference(x, ptr, time, event, P0, perms, 3, 1e-3, 1e-4)
    once = surv_reference(x, ptr, time, event, P0, np.array([[1, 0, 3]]), 3, 1e-3, 1e-4)
    em, ev, el = _worst(got[1], m, L, F)[0], _worst(got[2], v, L, F)[0], abs(float(got[3][0, 0] / got[3][0, 1]) - float(loss[0]))
    print(f"max |gpu - f64|: m {em:.3e}  v {ev:.3e}  epoch loss {el:.3e}; listed once the moments differ by {_worst(got[1], once[1], L, F)[0]:.3e}")
    assert em <= STATE_BOUND and ev <= STATE_BOUND and el <= LOSS_BOUND and _worst(got[1], once[1], L, F)[0] > 1e-4
    assert float(got[3][0, 1]) == 3.0                                        # bag 0 once, bag 3 twice; bag 1 is censored


def test_the_risk_bias_keeps_its_bits_without_decay(dev):
    from gipvit.mil import param_views
    L, F = 32, 12
    x, ptr, time, event, P0 = _small_case()
    P0["classifier.bias"] = torch.tensor([0.3137])
    perms = np.array([[4, 1, 0, 3, 2], [2, 3, 1, 4, 0]])
    P, m, v, _ = _train_gpu(dev, x, ptr, time, event, pack(P0, L, 1, F), perms, 3, L, 1e-2, 0.0)
    views = [param_views(t, L, 1, F)["classifier.bias"] for t in (P, m, v)]
    assert torch.equal(_bits(views[0]), _bits(P0["classifier.bias"])) and not views[1].any() and not views[2].any()
    assert not torch.equal(param_views(P, L, 1, F)["classifier.weight"], P0["classifier.weight"])
    Pd = _train_gpu(dev, x, ptr, time, event, pack(P0, L, 1, F), perms, 3, L, 1e-2, 1e-2)[0]
    bc = float(param_views(Pd, L, 1, F)["classifier.bias"])
    assert 0.0 < bc < 0.3137                                                 # with decay it only decays


def test_a_step_without_an_event_changes_nothing_but_the_step_count(dev):
    """Bags 1 (censored) twice, then bags 0, 2: the first step leaves params, m, v and loss_sum as they were; the second is Adam's
    step 2 -- the bits of a call that starts at step0 = 1 over bags 0, 2 alone, not those of one that starts at step0 = 0."""
    L, F = 32, 12
    x, ptr, time, event, P0 = _small_case()
    p0 = pack(P0, L, 1, F)
    g = torch.Generator().manual_seed(1)
    state = (torch.randn(p0.shape, generator=g) * 1e-3, torch.rand(p0.shape, generator=g) * 1e-6)
    alone = _train_gpu(dev, x, ptr, time, event, p0, np.array([[1, 1]]), 2, L, 1e-3, 1e-4, state=state)
    assert torch.equal(_bits(alone[0]), _bits(p0)) and torch.equal(_bits(alone[1]), _bits(state[0])) and torch.equal(_bits(alone[2]), _bits(state[1]))
    assert alone[3].tolist() == [[0.0, 0.0]]
    both = _train_gpu(dev, x, ptr, time, event, p0, np.array([[1, 1, 0, 2]]), 2, L, 1e-3, 1e-4, state=state)
    second = _train_gpu(dev, x, ptr, time, event, p0, np.array([[0, 2]]), 2, L, 1e-3, 1e-4, state=state, step0=1)
    first = _train_gpu(dev, x, ptr, time, event, p0, np.array([[0, 2]]), 2, L, 1e-3, 1e-4, state=state, step0=0)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(both, second)) and not torch.equal(_bits(both[0]), _bits(first[0]))


def test_bad_bags_contribute_nothing(dev):
    """An empty bag, one longer than max_bag, one whose rows end past N, bags with a NaN / infinite / negative time, with a flag
    of 2 / -1, and bag indices outside the table, mixed into the visiting order: the bits of the run over the good bags alone."""
    L, F = 32, 12
    x, ptr, time, event, P0 = _small_case()                                 # good bags of 3, 65, 2, 64, 5 rows
    clean = _train_gpu(dev, x, ptr, time, event, pack(P0, L, 1, F), np.array([[0, 1, 2, 3, 4]]), 3, L, 1e-3, 1e-4, max_bag=65)
    g = [x[ptr[k]:ptr[k + 1]] for k in range(5)]
    junk = lambda n: torch.randn(n, F, generator=torch.Generator().manual_seed(n))
    # table: g0 EMPTY g1 LONG(70) g2 NANTIME(4) INFTIME(4) NEGTIME(4) g3 FLAG2(4) FLAGNEG(4) g4 PASTN
    parts = [g[0], g[1], junk(70), g[2], junk(4), junk(4), junk(4), g[3], junk(4), junk(4), g[4], junk(10)]
    sizes = [3, 0, 65, 70, 2, 4, 4, 4, 64, 4, 4, 5, 60]
    ptr2 = np.concatenate([[0], np.cumsum(sizes)])
    x2 = torch.cat(parts)
    assert ptr2[-1] == x2.shape[0] + 50
    time2 = np.array([time[0], 1, time[1], 1, time[2], np.nan, np.inf, -1.0, time[3], 1, 1, time[4], 1], dtype=np.float32)
    event2 = np.array([event[0], 1, event[1], 1, event[2], 1, 1, 1, event[3], 2, -1, event[4], 1])
    # steps of 6: {g0 EMPTY g1 NANTIME g2 LONG} {INFTIME g3 FLAG2 NEGTIME g4 FLAGNEG} {PASTN -1 99}: good bags 0 1 2 | 3 4, as clean's steps
    order = np.array([[0, 1, 2, 5, 4, 3, 6, 8, 9, 7, 11, 10, 12, -1, 99]])
    dirty = _train_gpu(dev, x2, ptr2, time2, event2, pack(P0, L, 1, F), order, 6, L, 1e-3, 1e-4, max_bag=65)
    assert all(bool(torch.isfinite(t).all()) for t in dirty)
    # clean ran 2 steps, dirty 3 (the last all bad): the step counts of the first two agree
    for name, a, b in zip(("params", "m", "v", "loss_sum"), clean, dirty):
        assert torch.equal(_bits(a), _bits(b)), name


def test_predict_of_bad_bags_writes_zeros(dev):
    from gipvit import ops
    L, F = 16, 8
    g = torch.Generator().manual_seed(8)
    sizes = [4, 0, 9, 3]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = torch.randn(16, F, generator=g)
    P = draw_params(L, 1, F, 8)
    _poison_workspace(dev, 6, 4, L, F)
    bags = torch.tensor([0, 1, 2, 3, -1, 9], dtype=torch.int32)
    out = ops.surv_predict(pack(P, L, 1, F).to(dev), x.to(dev), torch.from_numpy(ptr).to(dev), L, 4, bags=bags.to(dev), want_attn=True)
    risk, attn = out["risk"].cpu(), out["attn"].cpu()
    want = surv_predict_reference(P, x, ptr.astype(np.int64)[[0, 1]])[0], surv_predict_reference(P, x[13:], np.array([0, 3]))[0]
    assert risk[[1, 2, 4, 5]].tolist() == [0.0] * 4 and not attn[4:13].any()             # empty; 9 rows > max_bag 4; outside the table
    assert abs(float(risk[0]) - float(want[0][0])) <= STATE_BOUND and abs(float(risk[3]) - float(want[1][0])) <= STATE_BOUND


# ---- the cohort evaluation
@pytest.mark.parametrize("n,kind", [(1, "mixed"), (2, "mixed"), (63, "mixed"), (64, "excluded"), (65, "mixed"), (1000, "mixed"), (1000, "censored"),
                                    (1000, "single"), (1000, "excluded"), (4097, "excluded")])
def test_cox_eval(dev, n, kind):
    from gipvit import ops
    from gipvit.survival import cindex_reference, cox_reference
    risk, time, event = cohort(n, 5, kind)
    want, events, excluded = cox_reference(risk, time, event)
    _, comp, conc, disc, tied = cindex_reference(risk, time, event)
    args = [torch.from_numpy(a).to(dev) for a in (risk, time, event)]
    ops._scratch("cox_eval", dev, n).fill_(255)
    loss, counts = ops.cox_eval(*args)
    loss2, counts2 = ops.cox_eval(*args)
    torch.cuda.synchronize()
    got = float(loss.cpu())
    print(f"n {n} {kind}: counts {counts.cpu().tolist()}, loss {got!r} against numpy {want!r}: {abs(got - want):.3e}")
    assert counts.cpu().tolist() == [events, comp, conc, disc, tied, excluded]
    assert abs(got - want) <= 1e-10 * max(1.0, abs(want))
    assert torch.equal(loss.view(torch.int64), loss2.view(torch.int64)) and torch.equal(counts, counts2)


# ---- SurvivalProbe on a real encoder
def _runner(dev, img=64, batch=8, seed=0):
    from gipvit.engine import FeatureExtractor
    from gipvit import models as M
    runner = FeatureExtractor("vit_tiny", img, batch=batch, device=dev)
    runner.load_state(M.init_vit_state("vit_tiny", img, 0, seed=seed))
    return runner


def test_survival_probe_matches_the_host_reference_on_the_runners_features(dev):
    from gipvit import data as D
    from gipvit.linprobe import epoch_permutations
    from gipvit.mil import init_params, param_views
    from gipvit.survival import SurvivalProbe, surv_metrics
    runner = _runner(dev)
    L, F, epochs, batch, lr, wd, seed = 16, 192, 3, 3, 1e-3, 1e-4, 5
    bank_loader, query_loader = D.SyntheticSlides(6, 8, 64, tiles_per_iter=5, seed=11), D.SyntheticSlides(5, 6, 64, tiles_per_iter=4, seed=23)
    table = D.synthetic_survival(bank_loader.image_file_names, 2)
    del table["synthetic_1"]                                                # a slide the table does not have is left out
    probe = SurvivalProbe(runner, table, hidden=L, lr=lr, weight_decay=wd, epochs=epochs, batch=batch, n_last=1, seed=seed)
    assert probe.fit(bank_loader) == 5
    got = probe.evaluate(query_loader)
    assert list(got) == ["surv_cindex", "surv_loss"]
    sd = probe.state_dict()
    assert list(sd) == NAMES and sd["attention_V.weight"].shape == (L, F) and sd["classifier.weight"].shape == (1, F)
    fb, ptrb, tb, eb, skipped = probe._collect(bank_loader)
    fq, ptrq, tq, eq, _ = probe._collect(query_loader)
    assert ptrb.tolist() == [0, 8, 16, 24, 32, 40] and skipped == 1 and ptrq.tolist() == [0, 6, 12, 18, 24]
    assert tb.tolist() == [table[f"synthetic_{k}"][0] for k in (0, 2, 3, 4, 5)] and eb.tolist() == [1, 1, 0, 1, 0]
    P0 = {k: t.clone() for k, t in param_views(init_params(L, 1, F, seed), L, 1, F).items()}
    kw = dict(x=fb.cpu(), ptr=ptrb.astype(np.int64), time=tb, event=eb.astype(np.int64), params0=P0, perms=epoch_permutations(5, epochs, seed),
              batch=batch, lr=lr, wd=wd)
    P, m, v, loss = surv_reference(**kw)
    P32 = surv_reference(dtype=f32, **kw)[0]
    gap = max(float((P32[k].double() - P[k]).abs().max()) for k in NAMES)
    ep, em = _worst(probe.params.cpu(), P, L, F), _worst(probe.m.cpu(), m, L, F)
    el = float((torch.tensor(probe.train_loss, dtype=torch.float64) - loss).abs().max())
    print(f"fit against the reference: params {ep[0]:.3e} at {ep[1]}{ep[2]} (gap32 {gap:.3e})  m {em[0]:.3e}  epoch loss {el:.3e}")
    assert gap <= 2e-5 and ep[0] <= max(4 * gap, STATE_BOUND) and em[0] <= STATE_BOUND and el <= LOSS_BOUND
    risk, attn, _ = surv_predict_reference(P, fq.cpu(), ptrq.astype(np.int64))
    want = surv_metrics(risk.numpy(), tq, eq)
    print("probe", dict(got), "reference", dict(want))
    assert got["surv_cindex"] == want["surv_cindex"] and abs(got["surv_loss"] - want["surv_loss"]) <= LOSS_BOUND
    tiles = probe.tile_attention(query_loader)
    assert len(tiles) == 4 and all(a.shape == (6,) and s.shape == (6,) for a, s in tiles)
    assert float((torch.cat([a for a, _ in tiles]).double() - attn).abs().max()) <= 4 * STATE_BOUND
    alone = SurvivalProbe(None, table=None, hidden=L, lr=lr, weight_decay=wd, epochs=epochs, batch=batch, seed=seed, features=F)
    alone.train(fb, ptrb, tb, eb)
    assert torch.equal(_bits(alone.params), _bits(probe.params))
    # an all-censored query cohort: no comparable pair, surv_cindex is nan
    m0 = alone.score(torch.zeros(3, device=dev), [1.0, 2.0, 3.0], [0, 0, 0])
    assert np.isnan(m0["surv_cindex"]) and np.isnan(m0["surv_loss"])


def test_survival_probe_feeds_the_centred_window_of_larger_tiles(dev):
    from gipvit import data as D
    from gipvit.survival import SurvivalProbe
    runner = _runner(dev)
    probe = SurvivalProbe(runner, {}, hidden=16, epochs=1, batch=2, n_last=2)
    mb = next(iter(D.SyntheticSlides(1, 6, 96, tiles_per_iter=6, seed=5)))      # 96-px tiles into the 64-px runner
    manual = runner.probe_features(mb["Data"][:, 16:80, 16:80, :].contiguous().to(dev), 2)
    assert probe.F == 384 and torch.equal(_bits(probe.features(mb["Data"])), _bits(manual))


# ---- needle bags on the device
def test_needle_bags_on_the_device(dev):
    from gipvit import ops
    from gipvit.survival import cindex_reference
    c = NEEDLE
    L, F = c["L"], c["F"]
    x, ptr, time, event, _, _ = needle_survival(24, c["seed"])
    P, _, _, loss = _train_gpu(dev, x, ptr, time, event, pack(draw_params(L, 1, F, c["seed"]), L, 1, F), needle_perms(), c["batch"], L, c["lr"], c["wd"])
    xq, ptrq, tq, eq, needle, yq = needle_survival(12, c["seed"] + 1)
    out = ops.surv_predict(P.to(dev), xq.to(dev), torch.from_numpy(ptrq.astype(np.int32)).to(dev), L, int(np.diff(ptrq).max()), want_attn=True)
    risk = out["risk"].cpu()
    l2, counts = ops.cox_eval(out["risk"], torch.from_numpy(tq).to(dev), torch.from_numpy(eq.astype(np.int32)).to(dev))
    counts = counts.cpu().tolist()
    attn = out["attn"].cpu().numpy()
    share = min(float(attn[ptrq[b]:ptrq[b + 1]][needle[ptrq[b]:ptrq[b + 1]]].sum()) for b in range(12) if yq[b])
    print(f"needle bags: epoch loss {float(loss[0, 0] / loss[0, 1]):.4f} -> {float(loss[-1, 0] / loss[-1, 1]):.4f}, counts {counts}, needle risks >= "
          f"{float(risk[yq == 1].min()):.2f}, other risks <= {float(risk[yq == 0].max()):.2f}, least attention share {share:.3f}")
    assert counts[1] == 24 and counts[2] == 24 and cindex_reference(risk.numpy(), tq, eq)[0] == 1.0


# ---- the driver
def test_driver_writes_surv_metrics_and_picks_model_best_on_them(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import train
    base = ["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--out-dim", "1024", "--batches-per-epoch", "2", "--epochs", "2",
            "--lr", "1e-4", "--warmup-epochs", "0", "--log-interval", "1", "--output", str(tmp_path), "--seed", "3", "--surv-probe",
            "--surv-hidden", "16", "--surv-epochs", "3", "--surv-batch", "4", "--surv-rate", "1", "--mil-probe", "--mil-hidden", "16", "--mil-epochs", "2",
            "--mil-batch", "2", "--mil-rate", "1"]
    names, mil = ["eval_surv_cindex", "eval_surv_loss"], ["eval_mil_top1", "eval_mil_loss", "eval_mil_auc_per_slide"]
    assert train.main(base + ["--experiment", "c", "--eval-metric", "surv_cindex"]) == 0
    with open(tmp_path / "c" / "summary.csv") as f:
        header = f.readline().strip().split(",")
    assert header == ["epoch", "train_loss"] + mil + names + ["lr"]
    rows = list(csv.DictReader(open(tmp_path / "c" / "summary.csv")))
    assert len(rows) == 2 and all(r[n] != "" for r in rows for n in names + mil)
    cs = [float(r["eval_surv_cindex"]) for r in rows]
    assert all(0.0 <= c <= 1.0 for c in cs) and all(float(r["eval_surv_loss"]) > 0 for r in rows)
    best = torch.load(tmp_path / "c" / "model_best.pth.tar", weights_only=True)
    assert best["metric"] == max(cs) and best["epoch"] == (1 if cs[1] > cs[0] else 0)
    # the default top1 is no metric of a run whose only monitor is the survival probe
    only = [a for k, a in enumerate(base) if not a.startswith("--mil") and not (k and base[k - 1].startswith("--mil-"))]
    with pytest.raises(SystemExit) as e:
        train.main(only + ["--experiment", "bad"])
    assert "surv_cindex" in str(e.value)
