"""CPU: the survival probe's specification and host side.

* ``surv_reference`` / ``surv_predict_reference``: the whole procedure in plain torch (autograd over Cox's partial likelihood with
  Breslow ties + torch.optim.Adam, the risk bias's gradient zeroed), fp64 by default.  It is checked against the hand-written
  d theta formula of include/gipvit.h, a definition-by-loops Cox on <= 6 slides and the two-slide closed form.  The GPU tests
  (tests/test_survival_gpu.py) hold gv_surv_train / gv_surv_predict to it.
* ``gap32`` = max |f32 - f64| of the reference over the parameters, per shared case, for the GPU file's parameter bound.
* ``cox_reference`` / ``cindex_reference`` (gipvit/survival.py) against brute-force loops; read_survival, synthetic_survival;
  struct layouts against gcc, the entry points' refusals through the ABI without a GPU, the driver's --surv-* flags, --eval-metric
  resolution, column order, the direction tuple.
* learnability: on the MIL file's "needle" bags with time 1 for needle bags and 4 for the others the reference reaches a
  concordance of exactly 1.0 over the fresh bags."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_mil_host import BETA1, BETA2, EPS, NAMES, cosine_scale, draw_params, mil_forward, needle_bags, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# F, L, batch, bag sizes, epochs, ldx, seed, lr; wd = 1e-4, integer times in 1..5 (many ties), event = (b % 4 != 1).  The last
# case has a full 64-bag step and a 6-bag remainder.
CASES = [
    dict(F=4, L=16, batch=2, sizes=[1, 2, 63, 5], epochs=2, ldx=4, seed=0, lr=1e-3, wd=1e-4),
    dict(F=36, L=128, batch=3, sizes=[64, 65, 1, 129, 2, 63, 64], epochs=3, ldx=40, seed=1, lr=1e-3, wd=1e-4),
    dict(F=192, L=256, batch=8, sizes=[500, 129, 65, 64, 63, 2, 1, 129, 65, 64, 2], epochs=2, ldx=192, seed=2, lr=5e-4, wd=1e-4),
    dict(F=388, L=16, batch=64, sizes=[3, 5, 2, 7, 1] * 14, epochs=2, ldx=388, seed=3, lr=5e-4, wd=1e-4),
]
CASE_IDS = ["F%d-L%d-B%d" % (c["F"], c["L"], c["batch"]) for c in CASES]


def case_setup(case):
    """-> dict of a case's inputs: x f32 [N, F], ptr int64 [n + 1], time f32 [n], event int64 [n], params0 (NAMES), perms."""
    F, sizes, seed = case["F"], case["sizes"], case["seed"]
    g = torch.Generator().manual_seed(seed)
    n = len(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = torch.randn(int(ptr[-1]), F, generator=g)
    rng = np.random.Generator(np.random.PCG64(seed))
    time = rng.integers(1, 6, size=n).astype(np.float32)
    event = np.array([int(b % 4 != 1) for b in range(n)], dtype=np.int64)
    # The features are noise alone, on purpose.  With a planted direction (x[first row of b, 0] += 2 (3 - t_b)) the reference's own
    # f32-vs-f64 gap of the last case scattered from 2.5e-8 to 4.1e-6 over three seeds, and for one seed from 5.7e-7 to 4.1e-6
    # between two hosts' torch builds: a weight whose gradient nearly cancels is moved by Adam as far as any other, so a single f32
    # run says little about the next one.  Without it the gap stayed within 1.2e-7 .. 2.5e-7 over the same seeds.
    perms = np.stack([rng.permutation(n) for _ in range(case["epochs"])])
    return dict(x=x, ptr=ptr, time=time, event=event, params0=draw_params(case["L"], 1, F, seed), perms=perms)


def cox_step_loss(theta, time, event):
    """Cox partial likelihood with Breslow ties over one step: theta [m] (torch), time / event arrays [m] -> (the sum of the
    event terms, E)."""
    t = torch.as_tensor(np.asarray(time, dtype=np.float64))
    total, E = 0.0, 0
    for i in range(len(theta)):
        if int(event[i]) == 1:
            total = total + torch.logsumexp(theta[t >= t[i]], dim=0) - theta[i]
            E += 1
    return total, E


def surv_reference(x, ptr, time, event, params0, perms, batch, lr, wd, dtype=torch.float64):
    """torch.optim.Adam(lr * cosine factor, (0.9, 0.999), 1e-8, weight_decay=wd) over the C = 1 model under the step's Cox loss,
    the gradient of classifier.bias (the risk bias: the loss does not depend on it) zeroed before the decay is added; a step
    without an event changes nothing but advances Adam's step count.
    -> (params, m, v: NAMES-keyed dicts, epoch_loss [epochs] = the epoch's event terms over its events), all ``dtype``."""
    P = {k: v.clone().to(dtype).requires_grad_(True) for k, v in params0.items()}
    opt = torch.optim.Adam(list(P.values()), lr=lr, betas=(BETA1, BETA2), eps=EPS, weight_decay=wd)
    xd = x.to(dtype)
    epochs = len(perms)
    epoch_loss = torch.zeros(epochs, dtype=dtype)
    for e in range(epochs):
        for grp in opt.param_groups:
            grp["lr"] = lr * cosine_scale(e, epochs)
        events = 0
        for s0 in range(0, len(perms[e]), batch):
            step = [int(b) for b in perms[e][s0:s0 + batch]]
            opt.zero_grad()
            theta = torch.stack([mil_forward(P, xd[ptr[b]:ptr[b + 1]])[0][0] for b in step])
            total, E = cox_step_loss(theta, [time[b] for b in step], [event[b] for b in step])
            if E == 0:
                for p in P.values():
                    st = opt.state[p]
                    if not st:
                        st["step"], st["exp_avg"], st["exp_avg_sq"] = torch.tensor(0.0), torch.zeros_like(p), torch.zeros_like(p)
                    st["step"] += 1
                continue
            epoch_loss[e] += total.detach()
            events += E
            (total / E).backward()
            P["classifier.bias"].grad.zero_()
            opt.step()
        epoch_loss[e] /= max(events, 1)
    st = lambda key: {k: opt.state[p][key].detach() if p in opt.state else torch.zeros_like(p) for k, p in P.items()}
    return {k: v.detach() for k, v in P.items()}, st("exp_avg"), st("exp_avg_sq"), epoch_loss


def surv_predict_reference(params, x, ptr, dtype=torch.float64):
    """-> (risk [n], attn [N], score [N]), ``dtype``."""
    P = {k: v.to(dtype) for k, v in params.items()}
    xd = x.to(dtype)
    risk, attn, score = [], [], []
    for b in range(len(ptr) - 1):
        logits, a, s = mil_forward(P, xd[ptr[b]:ptr[b + 1]])
        risk.append(logits[0]); attn.append(a); score.append(s)
    return torch.stack(risk), torch.cat(attn), torch.cat(score)


def dtheta_by_hand(theta, time, event):
    """The header's formula, in the dtype of theta (numpy)."""
    theta = np.asarray(theta)
    M, E = theta.max(), int(np.sum(event))
    w = np.exp(theta - M)
    S = np.array([w[np.asarray(time) >= time[i]].sum() for i in range(len(theta))])
    return np.array([(sum(w[k] / S[i] for i in range(len(theta)) if event[i] == 1 and time[i] <= time[k]) - event[k]) / E for k in range(len(theta))])


_ref_cache = {}


def case_reference(i):
    """(setup, f64 reference, gap32, per-tensor gaps) of case i, computed once and shared by both files (never modified)."""
    if i not in _ref_cache:
        c, s = CASES[i], case_setup(CASES[i])
        kw = dict(x=s["x"], ptr=s["ptr"], time=s["time"], event=s["event"], params0=s["params0"], perms=s["perms"], batch=c["batch"], lr=c["lr"], wd=c["wd"])
        ref = surv_reference(**kw)
        r32 = surv_reference(dtype=torch.float32, **kw)
        gaps = {k: float((r32[0][k].double() - ref[0][k]).abs().max()) for k in NAMES}
        _ref_cache[i] = (s, ref, max(gaps.values()), gaps)
    return _ref_cache[i]


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_cases_are_well_posed(i):
    s, (P, m, v, loss), gap, gaps = case_reference(i)
    print(f"gap32 {gap:.3e} per tensor {{{', '.join(f'{k}: {g:.1e}' for k, g in gaps.items())}}}; f64 epoch losses {[round(float(x), 5) for x in loss]}")
    assert gap <= 2e-5
    assert all(bool(torch.isfinite(t).all()) for t in P.values()) and bool(torch.isfinite(loss).all())
    assert not m["classifier.bias"].abs().max() > CASES[i]["wd"]          # only the decay ever reaches the risk bias


def test_autograd_agrees_with_the_dtheta_formula():
    g = torch.Generator().manual_seed(4)
    for m in (2, 5, 6):
        theta = torch.randn(m, generator=g, dtype=torch.float64).requires_grad_(True)
        time = np.array([2, 1, 2, 3, 1, 2][:m], dtype=np.float32)
        event = np.array([1, 0, 1, 1, 1, 0][:m])
        total, E = cox_step_loss(theta, time, event)
        (total / E).backward()
        assert float(np.abs(theta.grad.numpy() - dtheta_by_hand(theta.detach().numpy(), time, event)).max()) <= 1e-14
        assert abs(float(theta.grad.sum())) <= 1e-14                         # the loss does not see a common shift


def test_cox_loss_by_loops_and_the_two_slide_closed_form():
    g = torch.Generator().manual_seed(9)
    theta = torch.randn(6, generator=g, dtype=torch.float64)
    time, event = [3.0, 1.0, 3.0, 2.0, 5.0, 1.0], [1, 1, 0, 1, 0, 0]
    want, E = 0.0, 0
    for i in range(6):
        if event[i]:
            want += math.log(sum(math.exp(float(theta[j])) for j in range(6) if time[j] >= time[i])) - float(theta[i])
            E += 1
    total, E2 = cox_step_loss(theta, time, event)
    assert E == E2 == 3 and abs(float(total) - want) <= 1e-13
    from gipvit.survival import cox_reference
    assert abs(cox_reference(theta.numpy(), time, event)[0] - want) <= 1e-13
    # two slides, slide 0 the earlier event, one step: l = 1/2 [log(e^th0 + e^th1) - th0] with E = ... the one event
    th = torch.tensor([0.3, -0.8], dtype=torch.float64)
    total, E = cox_step_loss(th, [1.0, 2.0], [1, 0])
    assert E == 1 and abs(float(total) - (math.log(math.exp(0.3) + math.exp(-0.8)) - 0.3)) <= 1e-15
    total, E = cox_step_loss(th, [1.0, 1.0], [1, 1])                          # tied: both in each other's risk set
    assert E == 2 and abs(float(total) / E - 0.5 * (2 * math.log(math.exp(0.3) + math.exp(-0.8)) - 0.3 + 0.8)) <= 1e-15
    total, E = cox_step_loss(th, [1.0, 2.0], [1, 1])
    assert abs(float(total) / E - 0.5 * (math.log(math.exp(0.3) + math.exp(-0.8)) - 0.3)) <= 1e-15      # the later event's term is log e^th1 - th1 = 0


def test_reference_zeroes_the_risk_bias_and_skips_eventless_steps():
    s, c = case_setup(CASES[0]), CASES[0]
    kw = dict(x=s["x"], ptr=s["ptr"], time=s["time"], params0=s["params0"], batch=2, lr=c["lr"])
    P, m, v, _ = surv_reference(event=s["event"], perms=np.array([[0, 2, 3, 1]]), wd=0.0, **kw)
    assert torch.equal(P["classifier.bias"], s["params0"]["classifier.bias"].double()) and not m["classifier.bias"].any()
    # bag 1 is censored: the step {1, 1} has no event; what follows it is Adam's step 2
    a = surv_reference(event=s["event"], perms=np.array([[1, 1, 0, 2]]), wd=1e-4, **kw)
    assert float(a[3][0]) > 0 and all(bool(torch.isfinite(t).all()) for t in a[0].values())
    g = a[1]["classifier.weight"] / (1 - BETA1)
    b = surv_reference(event=s["event"], perms=np.array([[0, 2]]), wd=1e-4, **kw)
    assert torch.allclose(g, b[1]["classifier.weight"] / (1 - BETA1), rtol=0, atol=1e-15)      # the same gradient ...
    assert not torch.equal(a[0]["classifier.weight"], b[0]["classifier.weight"])              # ... under another bias correction


# ---- the cohort evaluation's numpy restatement
def _cindex_loops(risk, time, event):
    ok = [i for i in range(len(risk)) if np.isfinite(risk[i]) and np.isfinite(time[i]) and time[i] >= 0 and event[i] in (0, 1)]
    comp = conc = disc = tied = 0
    for i in ok:
        for j in ok:
            if event[i] == 1 and time[i] < time[j]:
                comp += 1
                conc += risk[i] > risk[j]
                disc += risk[i] < risk[j]
                tied += risk[i] == risk[j]
    return comp, conc, disc, tied


def _cox_loops(risk, time, event):
    ok = [i for i in range(len(risk)) if np.isfinite(risk[i]) and np.isfinite(time[i]) and time[i] >= 0 and event[i] in (0, 1)]
    total = 0.0
    for i in ok:
        if event[i] == 1:
            total += math.log(sum(math.exp(float(risk[j])) for j in ok if time[j] >= time[i])) - float(risk[i])
    return total, sum(int(event[i]) for i in ok), len(risk) - len(ok)


def cohort(n, seed, kind="mixed"):
    """risk f32, time f32, event int32 [n] with tied times and risks; ``kind``: mixed / censored (no event) / single (one event) /
    excluded (entries of each excluded kind mixed in)."""
    rng = np.random.Generator(np.random.PCG64([seed, n]))
    risk = (rng.integers(-8, 9, size=n) / 4).astype(np.float32) if n > 2 else rng.standard_normal(n).astype(np.float32)
    time = rng.integers(1, max(2, min(n, 40)) + 1, size=n).astype(np.float32)
    event = (rng.random(n) < 0.6).astype(np.int32)
    if kind == "censored":
        event[:] = 0
    elif kind == "single":
        event[:] = 0
        event[int(np.argmin(time))] = 1
    elif kind == "excluded":
        bad = [(np.nan, None, None), (np.inf, None, None), (None, np.nan, None), (None, -1.0, None), (None, np.inf, None), (None, None, 2), (None, None, -1)]
        for k, (r, t, e) in enumerate(bad):
            i = (k * 7 + 1) % n
            if r is not None: risk[i] = r
            if t is not None: time[i] = t
            if e is not None: event[i] = e
    return risk, time, event


@pytest.mark.parametrize("n,kind", [(1, "mixed"), (2, "mixed"), (9, "mixed"), (40, "mixed"), (40, "censored"), (40, "single"), (40, "excluded"), (63, "excluded")])
def test_numpy_restatements_against_loops(n, kind):
    from gipvit.survival import cindex_reference, cox_reference, surv_metrics
    risk, time, event = cohort(n, 5, kind)
    comp, conc, disc, tied = _cindex_loops(risk, time, event)
    c, *counts = cindex_reference(risk, time, event)
    assert counts == [comp, conc, disc, tied]
    assert (math.isnan(c) and comp == 0) or c == (conc + 0.5 * tied) / comp
    total, events, excluded = _cox_loops(risk, time, event)
    got = cox_reference(risk, time, event)
    assert got[1:] == (events, excluded) and abs(got[0] - total) <= 1e-12 * max(1.0, abs(total))
    if kind == "censored":
        assert comp == 0 and events == 0 and math.isnan(surv_metrics(risk, time, event)["surv_cindex"])
    if kind == "single":
        assert events == 1 and comp > 0
    if kind == "excluded":
        assert excluded >= 5
    m = surv_metrics(risk, time, event)
    assert list(m) == ["surv_cindex", "surv_loss"] and (events == 0 or abs(m["surv_loss"] - total / events) <= 1e-12)


def test_equal_times_are_not_comparable():
    from gipvit.survival import cindex_reference
    assert cindex_reference([1.0, 0.0], [2.0, 2.0], [1, 0])[1] == 0
    assert cindex_reference([1.0, 0.0, 1.0], [1.0, 2.0, 3.0], [1, 1, 0]) == (0.5, 3, 1, 1, 1)


# ---- the tables
def test_read_survival_both_spellings_and_bad_cells(tmp_path):
    from gipvit.data import _read_labels, read_survival
    ref = tmp_path / "ref"; ref.mkdir()
    (ref / "labels.csv").write_text("slide,label,fold,Time (months),Censored\nA,Positive,1,12.5,0\nB,Negative,2,30,1\nC,1,1,,0\nD,0,1,abc,0\nE,1,1,-3,0\n"
                                    "F,1,1,nan,0\nG,1,1,inf,1\nH,1,1,7,2\nI,1,1,7,\nJ,0,test,0,1\n")
    assert read_survival(str(ref)) == {"A": (12.5, 1), "B": (30.0, 0), "J": (0.0, 0)}
    own = tmp_path / "own"; own.mkdir()
    (own / "labels.csv").write_text("slide,label,time,event\nA,0,4,1\nB,1,9.25,0\nC,1,2,x\n")
    assert read_survival(str(own)) == {"A": (4.0, 1), "B": (9.25, 0)}
    low = tmp_path / "low"; low.mkdir()
    (low / "labels.csv").write_text("slide,time,censored\nA,4,1\n")
    assert read_survival(str(low)) == {"A": (4.0, 0)}
    plain = tmp_path / "plain"; plain.mkdir()
    (plain / "labels.csv").write_text("slide,label,fold\nA,1,1\nB,0,2\n")
    assert read_survival(str(plain)) == {} and read_survival(str(tmp_path)) == {}
    assert _read_labels(str(ref), None)["A"] == (1, "1") and _read_labels(str(plain), None) == {"A": (1, "1"), "B": (0, "2")}


def test_synthetic_survival_depends_on_ordinal_and_seed_only():
    from gipvit.data import synthetic_survival
    names = [f"synthetic_{k}" for k in range(6)]
    a, b = synthetic_survival(names, 3), synthetic_survival(names, 3)
    assert a == b and list(a) == names and a != synthetic_survival(names, 4)
    assert synthetic_survival(["x", "y", "z"], 3) == {n: a[o] for n, o in zip("xyz", names)}      # the name plays no part
    assert {e for _, e in a.values()} == {0, 1} and {e for _, e in synthetic_survival(names[:2], 0).values()} == {0, 1}
    assert all(np.float32(t) == t and 1.0 <= t <= 60.0 for t, _ in a.values())
    t0 = float(np.float32(np.random.Generator(np.random.PCG64([3, 2])).uniform(1.0, 60.0)))
    assert a["synthetic_2"] == (t0, 1)


def test_collect_features_keep_predicate():
    from gipvit.knn import collect_features
    mk = lambda k, y, last: {"Data": torch.full((2, 3), float(k)), "Label": torch.tensor([y]), "Is Last Batch": last}

    class Loader:
        image_file_names = ["a", "b", "c"]

        def __iter__(self):
            return iter([mk(0, 0, False), mk(0, 0, True), mk(1, 7, True), mk(2, 1, True)])
    f, y, s, skipped = collect_features(Loader(), 2, lambda d: d, "t")
    assert s.tolist() == [0, 0, 0, 0, 2, 2] and skipped == 1
    f, y, s, skipped = collect_features(Loader(), 2, lambda d: d, "t", keep=lambda k: k != 0)       # the label plays no part
    assert s.tolist() == [1, 1, 2, 2] and skipped == 1 and f[:, 0].tolist() == [1.0, 1.0, 2.0, 2.0]
    with pytest.raises(ValueError):
        collect_features(Loader(), 2, lambda d: d, "t", keep=lambda k: False)


class _Runner:
    D, img, dev = 192, 64, "cpu"

    class vit:
        depth = 12


def test_probe_settings_state_dict_and_refusals():
    from gipvit.mil import init_params
    from gipvit.survival import SurvivalProbe
    probe = SurvivalProbe(_Runner(), {"a": (1.0, 1)}, hidden=32, n_last=2)
    assert (probe.F, probe.L, probe.C, probe.batch) == (384, 32, 1, 32)
    assert probe.metric_names() == ["surv_cindex", "surv_loss"] and probe.lower_is_better == ("loss",) and probe.prefix == "surv_"
    with pytest.raises(RuntimeError):
        probe.state_dict()
    probe.params = init_params(32, 1, 384, 0)
    sd = probe.state_dict()
    assert list(sd) == NAMES and sd["classifier.weight"].shape == (1, 384) and sd["classifier.bias"].shape == (1,)
    for kw in (dict(hidden=8), dict(hidden=40), dict(hidden=272), dict(lr=0.0), dict(lr=float("nan")), dict(weight_decay=-1e-3), dict(epochs=0),
               dict(batch=0), dict(batch=65), dict(n_last=0), dict(n_last=13)):
        with pytest.raises(ValueError):
            SurvivalProbe(_Runner(), {}, **kw)
    with pytest.raises(ValueError):
        SurvivalProbe(_Runner(), None)
    alone = SurvivalProbe(None, table=None, features=1536)
    assert alone.F == 1536
    with pytest.raises(ValueError):
        SurvivalProbe(None, table=None)
    with pytest.raises(ValueError):
        SurvivalProbe(None, table=None, features=4100)
    with pytest.raises(ValueError) as e:                                    # a bank without an event
        alone.train(torch.zeros(4, 1536), [0, 2, 4], [1.0, 2.0], [0, 0])
    assert "no event" in str(e.value)


# ---- the ABI without a GPU
def _lib():
    from gipvit import _lib as L
    return L


def test_struct_layouts_match_gcc(tmp_path):
    L = _lib()
    structs = [L.gv_surv_train_args, L.gv_surv_predict_args, L.gv_cox_eval_args]
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


TRAIN_OK = dict(params=4096, m=8192, v=12288, x=16384, bag_ptr=20480, time=24576, event=45056, bags=28672, loss_sum=32768, workspace=36864,
                workspace_bytes=1 << 40, ldx=384, N=4000, F=384, L=128, n_all_bags=10, n_bags=10, batch=8, max_bag=500, step0=0,
                lr=5e-4, lr_scale=1.0, wd=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)      # never dereferenced


def test_surv_train_abi_errors():
    L = _lib()
    rc = lambda **kw: L.lib.gv_surv_train(ctypes.byref(L.gv_surv_train_args(**dict(TRAIN_OK, **kw))), None)
    err = lambda: L.lib.gv_last_error().decode()
    assert L.lib.gv_surv_train(None, None) == -3
    for name in ("params", "m", "v", "x", "bag_ptr", "time", "event", "bags", "loss_sum", "workspace"):
        assert rc(**{name: None}) == -3 and "null" in err(), name
    for F in (0, 382, 4100):
        assert rc(F=F, ldx=4100) == -1 and "4096" in err() and "multiple of 4" in err(), F
    for Lh in (0, 8, 24, 272):
        assert rc(L=Lh) == -1 and "multiple of 16" in err() and "256" in err(), Lh
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
    need = L.lib.gv_surv_workspace_bytes(8, 500, 128, 384)
    assert need > 0
    assert rc(workspace_bytes=need - 1) == -1 and str(need) in err() and "workspace" in err() and err().startswith("gv_surv_train")
    assert "(gv_surv_workspace_bytes)" in err() and rc(workspace=None) == -3 and "gv_surv_workspace_bytes)" in err()
    assert rc(workspace=36864 + 4) == -2 and "workspace" in err()


def test_surv_predict_and_cox_eval_abi_errors():
    L = _lib()
    ok = dict(params=4096, x=8192, bag_ptr=12288, bags=None, risk=20480, attn=28672, score=32768, workspace=36864,
              workspace_bytes=1 << 40, ldx=384, N=4000, F=384, L=128, n_all_bags=100, n_bags=100, max_bag=500)
    rc = lambda **kw: L.lib.gv_surv_predict(ctypes.byref(L.gv_surv_predict_args(**dict(ok, **kw))), None)
    err = lambda: L.lib.gv_last_error().decode()
    assert L.lib.gv_surv_predict(None, None) == -3
    for name in ("params", "x", "bag_ptr", "risk", "workspace"):
        assert rc(**{name: None}) == -3 and "null" in err(), name
    assert rc(n_bags=0) == -1 and "n_bags >= 1" in err()
    assert rc(F=4100, ldx=4100) == -1 and "4096" in err()
    assert rc(L=24) == -1 and "multiple of 16" in err()
    assert rc(max_bag=4097) == -1 and "max_bag" in err()
    assert rc(ldx=380) == -1 and "ldx >= F" in err()
    assert rc(x=8192 + 4) == -2 and "16-byte aligned" in err()
    need = L.lib.gv_surv_workspace_bytes(64, 500, 128, 384)                  # more than 64 bags: groups of 64
    assert rc(workspace_bytes=need - 1) == -1 and str(need) in err() and "(gv_surv_workspace_bytes)" in err()
    small = L.lib.gv_surv_workspace_bytes(5, 500, 128, 384)
    assert 0 < small < need and rc(n_bags=5, workspace_bytes=small - 1) == -1 and str(small) in err()
    okc = dict(risk=4096, time=8192, event=12288, loss=16384, counts=20480, workspace=24576, workspace_bytes=1 << 40, n=1000)
    rcc = lambda **kw: L.lib.gv_cox_eval(ctypes.byref(L.gv_cox_eval_args(**dict(okc, **kw))), None)
    assert L.lib.gv_cox_eval(None, None) == -3
    for name in ("risk", "time", "event", "loss", "counts", "workspace"):
        assert rcc(**{name: None}) == -3 and "null" in err(), name
    for n in (0, -1, 65537):
        assert rcc(n=n) == -1 and "1 <= n <= 65536" in err(), n
    need = L.lib.gv_cox_eval_workspace_bytes(1000)
    assert rcc(workspace_bytes=need - 1) == -1 and str(need) in err()
    assert rcc(workspace=24576 + 4) == -2 and rcc(loss=16384 + 4) == -2 and "8-byte aligned" in err()


def test_workspace_bytes():
    L = _lib()
    ws, mil = L.lib.gv_surv_workspace_bytes, L.lib.gv_mil_workspace_bytes
    assert ws(1, 1, 16, 4) > 0 and ws(64, 4096, 256, 4096) > 0
    sizes = [ws(b, 500, 128, 384) for b in (1, 2, 8, 64)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4 and all(s % 16 == 0 for s in sizes)
    assert ws(8, 500, 128, 384) == mil(8, 500, 128, 1, 384) + 16            # the MIL layout and the step's event count
    for bad in ((0, 500, 128, 384), (65, 500, 128, 384), (8, 0, 128, 384), (8, 4097, 128, 384), (8, 500, 0, 384), (8, 500, 24, 384),
                (8, 500, 272, 384), (8, 500, 128, 0), (8, 500, 128, 382), (8, 500, 128, 4100)):
        assert ws(*bad) == -1 and L.lib.gv_last_error().decode().startswith("gv_surv_workspace_bytes"), bad
    cw = L.lib.gv_cox_eval_workspace_bytes
    assert cw(1) == 64 and cw(65536) == (6 * 65536 + 2) * 8 and cw(4096) >= 4096 * 8 * 2
    for bad in (0, -5, 65537):
        assert cw(bad) == -1 and L.lib.gv_last_error().decode().startswith("gv_cox_eval_workspace_bytes"), bad


def test_both_builds_export_the_entry_points():
    L = _lib()
    names = ["gv_surv_train", "gv_surv_predict", "gv_cox_eval", "gv_surv_workspace_bytes", "gv_cox_eval_workspace_bytes", "gv_mil_train", "gv_mil_predict"]
    assert all(hasattr(L.lib, n) for n in names)
    assert L.ENTRY_POINTS["gv_surv_train"] is L.gv_surv_train_args and L.ENTRY_POINTS["gv_surv_predict"] is L.gv_surv_predict_args
    assert L.ENTRY_POINTS["gv_cox_eval"] is L.gv_cox_eval_args
    assert "gv_surv_workspace_bytes" in L.PLAIN_SYMBOLS and "gv_cox_eval_workspace_bytes" in L.PLAIN_SYMBOLS
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); missing = [n for n in sys.argv[2:] if not hasattr(l, n)]; assert not missing, missing; "
            "l.gv_surv_workspace_bytes.restype = ctypes.c_int64; assert l.gv_surv_workspace_bytes(8, 500, 128, 384) > 0")
    for lib in ("libgipvit_hip.so", "libgipvit_hip_f16.so"):
        r = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(L.LIB_PATH), lib)] + names, capture_output=True, text=True)
        assert r.returncode == 0, (lib, r.stderr[-600:])


# ---- the driver
def _train():
    sys.path.insert(0, ROOT)
    import train
    return train


SURV = ["--dino", "--surv-probe", "--eval-metric", "surv_cindex"]


@pytest.mark.parametrize("flags,word", [
    (["--surv-probe", "--eval-metric", "surv_cindex"], "--surv-probe"),                        # without --dino
    (SURV + ["--surv-hidden", "8"], "--surv-hidden"),
    (SURV + ["--surv-hidden", "40"], "--surv-hidden"),
    (SURV + ["--surv-hidden", "272"], "--surv-hidden"),
    (SURV + ["--surv-lr", "0"], "--surv-lr"),
    (SURV + ["--surv-lr", "-0.001"], "--surv-lr"),
    (SURV + ["--surv-lr", "nan"], "--surv-lr"),
    (SURV + ["--surv-lr", "inf"], "--surv-lr"),
    (SURV + ["--surv-wd", "-0.001"], "--surv-wd"),
    (SURV + ["--surv-epochs", "0"], "--surv-epochs"),
    (SURV + ["--surv-batch", "0"], "--surv-batch"),
    (SURV + ["--surv-batch", "65"], "--surv-batch"),
    (SURV + ["--surv-layers", "0"], "--surv-layers"),
    (SURV + ["--surv-layers", "13"], "--surv-layers"),
    (SURV + ["--model", "vit_base_patch16_224", "--surv-layers", "6"], "--surv-layers"),       # 6 x 768 > 4096
    (SURV + ["--surv-rate", "-1"], "--surv-rate"),
    (SURV + ["--test_fold", "-1"], "--test_fold"),
    (SURV + ["--tile-size", "128"], "--tile-size"),
    (SURV + ["--num_tiles", "4097"], "--num_tiles"),
    (SURV + ["--knn-bank-tiles", "4097"], "--knn-bank-tiles"),
    (["--dino", "--surv-probe"], "surv_cindex"),                                              # the default top1: no such metric
    (["--dino", "--surv-probe", "--eval-metric", "auc_per_slide"], "--eval-metric"),
    (["--dino", "--surv-probe", "--eval-metric", "mil_top1"], "--eval-metric"),               # the MIL probe is off
    (["--dino", "--surv-probe", "--knn-monitor", "--eval-metric", "cindex"], "--eval-metric"),  # a bare name is the k-NN monitor's
    (["--dino", "--surv-probe", "--mil-probe", "--eval-metric", "surv_top1"], "--eval-metric"),
    (["--dino", "--mil-probe", "--eval-metric", "surv_cindex"], "--eval-metric"),             # the survival probe is off
])
def test_driver_refuses_before_any_gpu_work(flags, word):
    train = _train()
    args, _ = train.parse_args((["--model", "vit_tiny"] if "--model" not in flags else []) + flags)
    with pytest.raises(SystemExit) as e:
        train.check_supported(args, lambda m: None)
    assert word in str(e.value)


def test_driver_refuses_a_folder_without_a_survival_table(tmp_path):
    train = _train()
    (tmp_path / "labels.csv").write_text("slide,label,fold\nA,1,1\nB,0,test\n")
    args, _ = train.parse_args(["--model", "vit_tiny", "--dataset", f"tiles:{tmp_path}"] + SURV)
    with pytest.raises(SystemExit) as e:
        train.check_supported(args, lambda m: None)
    assert "survival table" in str(e.value) and "labels.csv" in str(e.value)
    (tmp_path / "labels.csv").write_text("slide,label,fold,Time (months),Censored\nA,1,1,12,0\nB,0,test,20,1\n")
    assert train.check_supported(args, lambda m: None) is None
    args, _ = train.parse_args(["--model", "vit_tiny", "--dataset", f"tiles:{tmp_path}", "--dino", "--mil-probe"])
    (tmp_path / "labels.csv").write_text("slide,label,fold\nA,1,1\nB,0,test\n")
    assert train.check_supported(args, lambda m: None) is None               # only --surv-probe asks for the table


def test_surv_flags_are_inert_without_the_probe():
    train = _train()
    base, _ = train.parse_args(["--model", "vit_tiny", "--dino"])
    assert (base.surv_probe, base.surv_hidden, base.surv_lr, base.surv_wd, base.surv_epochs, base.surv_batch, base.surv_layers, base.surv_rate) == \
        (False, 128, 5e-4, 1e-4, 50, 32, 1, 0)
    assert train.check_supported(base, lambda m: None) is None
    bad = ["--surv-hidden", "7", "--surv-lr", "-1", "--surv-wd", "-1", "--surv-epochs", "0", "--surv-batch", "999", "--surv-layers", "50", "--surv-rate", "-3"]
    for extra in (["--dino"], []):
        off, _ = train.parse_args(["--model", "vit_tiny", "--test_fold", "-1"] + bad + extra)
        assert not off.surv_probe and train.check_supported(off, lambda m: None) is None
        ref, _ = train.parse_args(["--model", "vit_tiny", "--test_fold", "-1"] + extra)
        differ = {k for k in vars(ref) if getattr(ref, k) != getattr(off, k)}
        assert differ == {"surv_hidden", "surv_lr", "surv_wd", "surv_epochs", "surv_batch", "surv_layers", "surv_rate"}, differ
        assert train.monitor_metric_names(off) == []
    on, _ = train.parse_args(["--model", "vit_tiny"] + SURV + ["--surv-hidden", "64", "--surv-lr", "1e-3", "--surv-wd", "0", "--surv-epochs", "5",
                                                                "--surv-batch", "64", "--surv-layers", "2", "--surv-rate", "2", "--knn-monitor",
                                                                "--linear-probe", "--mil-probe"])
    assert train.check_supported(on, lambda m: None) is None
    assert (on.surv_hidden, on.surv_lr, on.surv_wd, on.surv_epochs, on.surv_batch, on.surv_layers, on.surv_rate) == (64, 1e-3, 0.0, 5, 64, 2, 2)
    assert train.monitor_due(on, "surv_", 1) and not train.monitor_due(on, "surv_", 0) and train.monitor_due(on, "surv_", on.epochs - 1)
    skip, _ = train.parse_args(["--model", "vit_tiny", "--extract_features"] + SURV)
    assert train.check_supported(skip, lambda m: None) is None
    from gipvit import cli_spec
    assert len(cli_spec.REFERENCE_FLAGS) == 148 and not any("surv" in str(f) for f in cli_spec.REFERENCE_FLAGS)


@pytest.mark.parametrize("name,knn,probe,mil,surv,want", [
    ("cindex", False, False, False, True, "surv_cindex"), ("loss", False, False, False, True, "surv_loss"), ("top1", False, False, False, True, "surv_top1"),
    ("surv_cindex", True, True, True, True, "surv_cindex"), ("surv_loss", False, False, True, True, "surv_loss"),
    ("top1", True, False, False, True, "knn_top1"), ("loss", False, True, False, True, "linear_loss"), ("loss", False, False, True, True, "mil_loss"),
    ("mil_top1", False, False, True, True, "mil_top1"), ("surv_cindex", False, False, False, False, "surv_cindex"),
    # the old forms
    ("top1", False, False, True, False, "mil_top1"), ("top1", True, True, True, False, "knn_top1"), ("loss", False, True, False, False, "linear_loss"),
    ("top1", False, False, False, False, "top1"), ("mil_loss", True, True, True, False, "mil_loss"),
])
def test_eval_metric_resolution(name, knn, probe, mil, surv, want):
    train = _train()
    assert train.resolve_eval_metric(name, knn, probe, mil, surv=surv) == want
    if not surv:
        assert train.resolve_eval_metric(name, knn, probe, mil) == want      # the four- and three-argument forms are unchanged
        if not mil:
            assert train.resolve_eval_metric(name, knn, probe) == want


def test_metric_names_column_order_and_direction():
    train = _train()
    only, _ = train.parse_args(["--model", "vit_tiny"] + SURV)
    assert train.monitor_metric_names(only) == ["surv_cindex", "surv_loss"]
    allm, _ = train.parse_args(["--model", "vit_tiny", "--knn-monitor", "--linear-probe", "--mil-probe"] + SURV)
    assert train.monitor_metric_names(allm) == ["knn_top1", "knn_auc_per_patch", "knn_auc_per_slide", "linear_top1", "linear_loss",
                                                "linear_auc_per_patch", "linear_auc_per_slide", "mil_top1", "mil_loss", "mil_auc_per_slide",
                                                "surv_cindex", "surv_loss"]
    one, _ = train.parse_args(["--model", "vit_tiny", "--num-classes", "1", "--mil-probe"] + SURV)
    assert train.monitor_metric_names(one) == ["mil_top1", "mil_loss", "surv_cindex", "surv_loss"]
    for flags in (["--eval-metric", "cindex"], ["--eval-metric", "loss"], ["--eval-metric", "surv_loss"], ["--knn-monitor", "--eval-metric", "surv_loss"],
                  ["--knn-monitor", "--eval-metric", "top1"], ["--linear-probe", "--mil-probe", "--eval-metric", "surv_cindex"],
                  ["--mil-probe", "--eval-metric", "auc_per_slide"]):
        args, _ = train.parse_args(["--model", "vit_tiny", "--dino", "--surv-probe"] + flags)
        assert train.check_supported(args, lambda m: None) is None, flags
    row = train.summary_row(3, {"loss": 1.0}, {"surv_cindex": 0.75, "surv_loss": 1.5}, train.monitor_metric_names(allm), 1e-3)
    assert list(row)[-4:] == ["eval_mil_auc_per_slide", "eval_surv_cindex", "eval_surv_loss", "lr"] and row["eval_mil_top1"] == "" and row["eval_surv_cindex"] == 0.75
    # the direction: a tuple of its own beside the pinned one
    assert train.LOWER_IS_BETTER == ("loss", "linear_loss", "mil_loss")
    assert train.SURV_LOWER_IS_BETTER == ("surv_loss",) and "surv_cindex" not in train.SURV_LOWER_IS_BETTER


def test_build_monitors_without_the_flag_and_with_it():
    train = _train()
    off, _ = train.parse_args(["--model", "vit_tiny", "--dino", "--mil-probe", "--mil-hidden", "32"])
    assert train.build_monitors(off, None) == []
    mons = train.build_monitors(off, _Runner())
    assert [type(m).__name__ for m in mons] == ["MilProbe"] and mons[0].L == 32
    on, _ = train.parse_args(["--model", "vit_tiny", "--mil-probe", "--surv-hidden", "64", "--surv-batch", "16"] + SURV)
    mons = train.build_monitors(on, _Runner(), surv_table={"synthetic_0": (3.0, 1)})
    assert [m.prefix for m in mons] == ["mil_", "surv_"] and (mons[1].L, mons[1].batch, mons[1].table) == (64, 16, {"synthetic_0": (3.0, 1)})


def test_surv_checks_load_no_library():
    code = ("import os, sys; sys.path.insert(0, %r); import train\n"
            "a, _ = train.parse_args(['--model', 'vit_base_patch16_224', '--dino', '--surv-probe', '--surv-layers', '4', '--eval-metric', 'surv_cindex', '--amp'])\n"
            "assert train.check_supported(a, lambda m: None) is None\n"
            "a, _ = train.parse_args(['--model', 'vit_tiny', '--dino', '--surv-probe', '--surv-layers', '13', '--amp'])\n"
            "try:\n    train.check_supported(a, lambda m: None)\n    raise AssertionError('accepted')\nexcept SystemExit as e:\n    assert '--surv-layers' in str(e)\n"
            "assert 'gipvit._lib' not in sys.modules and 'gipvit.engine' not in sys.modules and 'gipvit.survival' not in sys.modules" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "GIPVIT_ACT_FORMAT"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-800:]


# ---- learnability of the specification
NEEDLE = dict(L=16, F=16, batch=8, lr=1e-2, wd=1e-4, epochs=80, seed=7)


def needle_survival(n_bags, seed):
    """The MIL file's needle bags as a survival cohort: time 1 for the needle bags and 4 for the others, event = (b % 3 != 0)."""
    x, ptr, labels, needle = needle_bags(n_bags, seed)
    time = np.where(labels.numpy() == 1, 1.0, 4.0).astype(np.float32)
    event = np.array([int(b % 3 != 0) for b in range(n_bags)], dtype=np.int64)
    return x, ptr, time, event, needle, labels.numpy()


def needle_perms():
    rng = np.random.Generator(np.random.PCG64(NEEDLE["seed"]))
    return np.stack([rng.permutation(24) for _ in range(NEEDLE["epochs"])])


def test_the_specification_learns_needle_bags():
    from gipvit.survival import cindex_reference
    c = NEEDLE
    x, ptr, time, event, _, _ = needle_survival(24, c["seed"])
    P, _, _, loss = surv_reference(x, ptr, time, event, draw_params(c["L"], 1, c["F"], c["seed"]), needle_perms(), c["batch"], c["lr"], c["wd"])
    xq, ptrq, tq, eq, needle, yq = needle_survival(12, c["seed"] + 1)
    risk, attn, _ = surv_predict_reference(P, xq, ptrq)
    cidx, comparable, *_ = cindex_reference(risk.numpy(), tq, eq)
    shares = [float(attn.numpy()[ptrq[b]:ptrq[b + 1]][needle[ptrq[b]:ptrq[b + 1]]].sum()) for b in range(12) if yq[b]]
    print(f"needle bags: epoch loss {float(loss[0]):.4f} -> {float(loss[-1]):.4f}, C-index {cidx} over {comparable} pairs, needle risks >= "
          f"{float(risk[yq == 1].min()):.2f}, other risks <= {float(risk[yq == 0].max()):.2f}, least attention share on the needles {min(shares):.3f}")
    assert comparable == 24 and cidx == 1.0
