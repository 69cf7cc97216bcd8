"""GPU: Sinkhorn-Knopp centring (gv_sinkhorn_*) and KoLeo (gv_koleo_fwd / _bwd) against the float64 specification of
tests/dinov2_terms_cases.py, and the DINO step with either or both of them against a torch restatement composed from
oracle.vit_oracle.  The kernel bounds are computed per case on the CPU (8 x the float32 restatement's deviation from float64, floor
1e-6: dinov2_terms_cases.bound); tests/test_dinov2_terms_host.py holds the conditions on the fixed inputs.  Every test prints its figures."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dinov2_terms_cases as C
from test_engine_gpu import _check_grads
from test_fp32_gpu import GNORM_TOL, GRAD_TOL, LOSS_TOL
from test_row_kernels_gpu import Measured, _dino_add, guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
f32, f64 = torch.float32, torch.float64
NAN = float("nan")


def ops():
    from gipvit import ops as o
    return o


def lib():
    from gipvit import _lib
    return _lib


# ============================================================================ Sinkhorn-Knopp
def run_sinkhorn(dev, T, tau, n, hyper_tau=None):
    """The 2 n + 1 launches on NaN-filled state (nothing may be read before it is written) -> (sk_center, a) on the CPU.
    ``hyper_tau``: tau travels in the hyper vector and the by-value temperature is another one."""
    o, L = ops(), lib()
    R, K = T.shape
    t = torch.from_numpy(T).to(dev)
    full = lambda m: guarded(dev, m, fill=NAN)
    (sb, shift), (ab, a), (bb, b), (cb, cs), (kb, skc) = full(1), full(K), full(R), full(K), full(K)
    nws = L.lib.gv_sinkhorn_workspace_bytes(R, K) // 4
    wb, ws = full(nws)
    hyper, by_value = None, tau
    if hyper_tau is not None:
        hyper = torch.zeros(L.HYP_COUNT, device=dev)
        hyper[L.HYP_TEACHER_TEMP] = hyper_tau
        by_value = 0.2
    st, kw = (t, shift, a, b, cs, ws), dict(hyper=hyper)
    o.sinkhorn_shift(*st, R, K, by_value, **kw)
    for it in range(n):
        o.sinkhorn_cols(*st, R, K, by_value, first=it == 0, **kw)
        if it < n - 1:
            o.sinkhorn_rows(*st, R, K, by_value, first=it == 0, **kw)
    o.sinkhorn_finish(*st, skc, R, K, by_value, first=n == 1, **kw)
    torch.cuda.synchronize()
    for buf, m, what in ((sb, 1, "shift"), (ab, K, "a"), (bb, R, "b"), (cb, K, "colsum"), (kb, K, "sk_center"), (wb, nws, "workspace")):
        assert bool(torch.isnan(buf[m:]).all()), f"{what}: elements behind the buffer were written"
    return skc.cpu(), a.cpu()


def _sinkhorn_check(dev, R, K, tau, n):
    c64, bnd, s_min = C.sinkhorn_reference(R, K, tau, n)
    T = C.sinkhorn_logits(R, K)
    skc, a = run_sinkhorn(dev, T, tau, n)
    again, _ = run_sinkhorn(dev, T, tau, n)
    assert torch.equal(skc, again), "two runs differ"
    via_hyper, _ = run_sinkhorn(dev, T, 0.5, n, hyper_tau=tau)
    assert torch.equal(skc, via_hyper), "tau from the hyper vector gives another result than tau by value"
    err = float(np.abs(C.gauge(skc.numpy()) - c64).max())
    print(f"[sinkhorn] R={R} K={K} tau={tau} n={n}: max |gauged centre - f64| {err:.3e}, bound {bnd:.3e} ({err / bnd:.3f}), min s_k {s_min:.2e}")
    assert s_min >= 1e-30, "a column sum reaches the clamp: the case's inputs are not fit for the comparison"
    assert bool(torch.isfinite(skc).all()) and err <= bnd
    assert float((skc + np.float32(tau) * a).abs().max()) <= 1e-6 * float(skc.abs().max())     # sk_center = -tau a


@gpu
@pytest.mark.parametrize("n", C.ITERS)
@pytest.mark.parametrize("tau", C.TAUS)
@pytest.mark.parametrize("R,K", C.SINKHORN_CASES[:3])
def test_sinkhorn_center_against_fp64(dev, R, K, tau, n):
    _sinkhorn_check(dev, R, K, tau, n)


@gpu
@pytest.mark.parametrize("R,K", C.SINKHORN_CASES[3:])
def test_sinkhorn_center_at_the_split_edges(dev, R, K):
    """The headline shape once, and one below / at / one above every edge of the column pass's tiles and row slices, the row pass's
    two workgroup sizes and the shift pass's stride (dinov2_terms_cases.SINKHORN_CASES)."""
    _sinkhorn_check(dev, R, K, 0.04, 3)


@gpu
@pytest.mark.parametrize("dt", ["16bit", "f32"])
def test_dino_loss_with_the_sinkhorn_center(dev, dt):
    """gv_dino_loss fed with sk_center: loss and student gradient of the float64 DINO loss under float64 Sinkhorn-Knopp probabilities,
    under the rule tests/test_row_kernels_gpu.py applies to the kernel (plain float32 side: the float32 restatement's centre)."""
    from oracle import vit_oracle as vo
    o = ops()
    B, V, G, K, tau, ts = 3, 4, 2, 1028, 0.04, 0.1
    T = C.sinkhorn_logits(G * B, K)
    s = torch.randn(V * B, K, generator=torch.Generator().manual_seed(5))
    a64, _ = C.sinkhorn_log(T, tau, 3)
    a32, _ = C.sinkhorn_log(T, tau, 3, np.float32)
    out = {}
    for name, d, a in (("ref", f64, a64), ("plain", f32, a32)):
        sr = s.to(d).clone().requires_grad_(True)
        center = torch.from_numpy(-np.asarray(tau, a.dtype) * a).to(d)[None]
        loss, csum = vo.dino_loss(sr, torch.from_numpy(T).to(d), center, V, G, ts, tau)
        loss.backward()
        out[name] = dict(loss=loss.detach().reshape(1), grad=sr.grad, csum=csum[0])
    # the reference's probabilities ARE the Sinkhorn-Knopp assignment
    P = torch.softmax((torch.from_numpy(T).double() + tau * torch.from_numpy(a64)) / tau, dim=-1).numpy()
    assert float(np.abs(P - C.sinkhorn_literal(T, tau, 3)).max()) < 1e-13
    skc, _ = run_sinkhorn(dev, T, tau, 3)
    dtype = f32 if dt == "f32" else o.bf16
    ds = torch.zeros(V * B, K, dtype=dtype, device=dev)
    loss, csum, ws = torch.zeros(1, device=dev), torch.zeros(K, device=dev), torch.full((2 * (V + G) * B,), NAN, device=dev)
    o.dino_loss(s.to(dev), torch.from_numpy(T).to(dev), skc.to(dev), ds, loss, csum, ws, B, V, G, K, ts, tau)
    torch.cuda.synchronize()
    m = Measured()
    _dino_add(m, f"sk_center {(B, V, G, K)}", ds.cpu(), loss.cpu(), csum.cpu(), out["ref"], out["plain"], dtype)
    m.check()


# ============================================================================ KoLeo
def run_koleo(dev, x, G, B, D, dtype, weight=1.0, d0=None, loss_scale=None):
    """forward + backward on NaN-filled scratch -> (koleo, nn, dfeats [rows + 3, D]) on the CPU; d0: what dfeats holds before."""
    o, L = ops(), lib()
    rows = G * B
    feats = torch.from_numpy(x).to(dev, dtype)
    nws = L.lib.gv_koleo_workspace_bytes(G, B, D) // 4
    wb, ws = guarded(dev, nws, fill=NAN)
    kb, kol = guarded(dev, 1, fill=NAN)
    nn = torch.full((rows + 8,), -7, dtype=torch.int32, device=dev)
    o.koleo_fwd(feats, ws, nn[:rows], kol, G, B, D)
    df = (torch.zeros(rows + 3, D) if d0 is None else d0.clone()).to(dev, dtype)
    o.koleo_bwd(df, ws, nn[:rows], G, B, D, weight, loss_scale=loss_scale)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wb[nws:]).all()) and bool(torch.isnan(kb[1:]).all()) and bool((nn[rows:] == -7).all()), "a guard was written"
    return kol.cpu(), nn[:rows].cpu(), df.float().cpu()


@gpu
@pytest.mark.parametrize("dt", ["16bit", "f32"])
@pytest.mark.parametrize("G,B,D", C.KOLEO_CASES)
def test_koleo_forward_backward(dev, G, B, D, dt):
    """nn exactly the reference's (the host test holds a gap of 1e-3 on these inputs), koleo and gx within the exported bounds, the
    in-place add into a non-zero dfeats (16-bit: plus 2^-8 of the result, one rounding of the sum doubled), rows past G B untouched
    bit for bit, two runs bitwise equal.  The inputs are bfloat16 values: both entry points see the same numbers."""
    r = C.koleo_reference(G, B, D)
    dtype = f32 if dt == "f32" else ops().bf16
    rows = G * B
    kol, nn, gx = run_koleo(dev, r["x"], G, B, D, dtype)
    assert np.array_equal(nn.numpy(), r["fwd"]["nn"]), "nearest neighbours differ from the reference's"
    ek = abs(float(kol) - float(r["fwd"]["koleo"]))
    ref = torch.from_numpy(r["gx"])
    slack = (2.0 ** -8) * ref.abs() if dt == "16bit" else 0.0
    eg = (gx[:rows].double() - ref).abs()
    print(f"[koleo {dt}] {(G, B, D)}: |koleo - f64| {ek:.3e} (bound {r['koleo_bound']:.2e}), max |gx - f64| {float(eg.max()):.3e} "
          f"(bound {r['gx_bound']:.2e}), worst err / bound {float((eg / (r['gx_bound'] + slack)).max()):.3f}")
    assert ek <= r["koleo_bound"] and bool((eg <= r["gx_bound"] + slack).all())
    assert bool((gx[rows:] == 0).all())
    # in place, into a gradient that is already there
    d0 = torch.from_numpy(C.bf16_round(0.01 * np.random.Generator(np.random.PCG64(D + B)).standard_normal((rows + 3, D)).astype(np.float32)))
    kol2, nn2, got = run_koleo(dev, r["x"], G, B, D, dtype, weight=1.0, d0=d0)
    want = d0[:rows].double() + ref
    slack = (2.0 ** -8) * want.abs() if dt == "16bit" else 0.0
    ea = (got[:rows].double() - want).abs()
    print(f"[koleo {dt}] {(G, B, D)}: in-place add, worst err / bound {float((ea / (r['gx_bound'] + slack)).max()):.3f}")
    assert bool((ea <= r["gx_bound"] + slack).all())
    assert torch.equal(got[rows:], d0[rows:]), "rows past G B were written"
    kol3, nn3, again = run_koleo(dev, r["x"], G, B, D, dtype, weight=1.0, d0=d0)
    assert torch.equal(kol2, kol3) and torch.equal(kol, kol2) and torch.equal(nn2, nn3) and torch.equal(got, again), "two runs differ"


@gpu
def test_koleo_weight_and_loss_scale_multiply_the_gradient(dev):
    """weight 0.25 with a device loss scale of 1024 (powers of two: exact) gives 256 x the unit-weight gradient, in both forms."""
    G, B, D = 2, 5, 384
    x = C.koleo_reference(G, B, D)["x"]
    ls = torch.tensor([1024.0, 0.0, 0.0, 0.0], device=dev)
    for dtype in (f32, ops().bf16):
        _, _, one = run_koleo(dev, x, G, B, D, dtype)
        _, _, scaled = run_koleo(dev, x, G, B, D, dtype, weight=0.25, loss_scale=ls)
        if dtype == f32:
            assert torch.equal(scaled, 256.0 * one)
        else:
            assert float((scaled - 256.0 * one).abs().max()) <= 2.0 ** -8 * float(scaled.abs().max())


# ============================================================================ the step
ARCH, K_OUT, B_STEP, W_KOLEO = "vit_tiny", 1024, 4, 0.1
CONFIGS = {"sinkhorn": dict(centering="sinkhorn_knopp"), "koleo": dict(koleo_weight=W_KOLEO),
           "both": dict(centering="sinkhorn_knopp", koleo_weight=W_KOLEO)}


def step_tiles():
    sys.path.insert(0, ROOT)
    import bench
    return bench.synth_tiles(B_STEP, 256, 99, "cpu")


def koleo_torch(feats, G, B, nn=None):
    """KoLeo of include/gipvit.h in torch (autograd: the index is a constant; ``nn``: a given one) -> (value, nn)."""
    total, out = 0.0, []
    for g in range(G):
        x = feats[g * B:(g + 1) * B]
        y = x / x.norm(dim=1, keepdim=True).clamp_min(C.EPS)
        if nn is None:
            dots = (y @ y.t()).detach().clone()
            dots.fill_diagonal_(-float("inf"))
            I = dots.argmax(1)
        else:
            I = torch.as_tensor(nn[g * B:(g + 1) * B], dtype=torch.long)
        d = (y - y[I] + C.EPS).norm(dim=1)
        total = total + (-torch.log(d + C.EPS)).mean()
        out.append(I)
    return total, torch.cat(out)


@functools.lru_cache(maxsize=1)
def _step_graph():
    """The DINO step's forward once on the CPU (float32, oracle.vit_oracle), its autograd graph kept."""
    from oracle import step_oracle as so, vit_oracle as vo
    orc = so.DinoOracle(arch=ARCH, img_size=224, out_dim=K_OUT, seed=0, lr=5e-4, wd=0.04, n_local=8)
    orc.center = 0.05 * torch.randn(1, K_OUT, generator=torch.Generator().manual_seed(3))
    crops = orc.crops(step_tiles())
    V, G = len(crops), orc.n_global
    with torch.no_grad():
        t_out = vo.multicrop_forward(orc.tp, orc.thp, crops[:G], ARCH)
    sp = {k: v.clone().requires_grad_(True) for k, v in orc.p.items()}
    shp = {k: v.clone().requires_grad_(True) for k, v in orc.hp.items()}
    feats = torch.cat([vo.vit_features(sp, torch.cat(crops[:G]), ARCH), vo.vit_features(sp, torch.cat(crops[G:]), ARCH)])
    s_out = vo.dino_head(shp, feats)
    leaves = {**{"backbone." + k: v for k, v in sp.items()}, **{"head." + k: v for k, v in shp.items()}}
    a, _ = C.sinkhorn_log(t_out.numpy(), orc.tt, 3)
    return dict(orc=orc, V=V, G=G, t_out=t_out, s_out=s_out, feats=feats, leaves=leaves, sk_center=torch.from_numpy(-orc.tt * a).float()[None])


@functools.lru_cache(maxsize=8)
def reference_for(config, nn=None):
    """Loss, koleo and every gradient of one configuration; ``nn`` (a tuple): the neighbour index KoLeo holds constant, default the
    reference's own arg-max.  -> dict(loss, koleo, grads, center, nn, feats)"""
    from oracle import vit_oracle as vo
    gr, kw = _step_graph(), CONFIGS[config]
    orc = gr["orc"]
    center = gr["sk_center"] if "centering" in kw else orc.center
    kol, idx = koleo_torch(gr["feats"], gr["G"], B_STEP, nn)
    loss, _ = vo.dino_loss(gr["s_out"], gr["t_out"], center, gr["V"], gr["G"], orc.ts, orc.tt)
    obj = loss + kw.get("koleo_weight", 0.0) * kol
    g = torch.autograd.grad(obj, list(gr["leaves"].values()), retain_graph=True, allow_unused=True)
    return dict(loss=float(loss.detach()), koleo=float(kol.detach()), grads=dict(zip(gr["leaves"], g)), center=center[0], nn=idx, feats=gr["feats"].detach())


def step_reference():
    """-> (oracle, {config: reference_for(config)})"""
    return _step_graph()["orc"], {name: reference_for(name) for name in CONFIGS}


def make_engine(dev, precision, **kw):
    from gipvit.engine import DinoEngine
    orc, _ = step_reference()
    eng = DinoEngine(arch=ARCH, img_size=224, out_dim=K_OUT, batch=B_STEP, n_local=8, lr=5e-4, weight_decay=0.04, device=dev, precision=precision, **kw)
    eng.load_state(orc.p, orc.hp)
    eng.center.copy_(orc.center[0])
    return eng


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _grad_gates(eng, grads_r):
    got = eng.grads()
    keys = [k for k, r in grads_r.items() if r is not None and k != "head.last_layer.weight_g"]
    gn_g = math.sqrt(sum(float((got[k].double() ** 2).sum()) for k in keys))
    gn_r = math.sqrt(sum(float((grads_r[k].double() ** 2).sum()) for k in keys))
    worst = max((_rel(got[k], grads_r[k]), k) for k in keys if float(grads_r[k].abs().max()) > 1e-12)
    return abs(gn_g - gn_r) / gn_r, worst


@gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_fp32_step_with_the_options(dev, config):
    """ViT-T, out_dim 1024, B = 4, the fp32 operand mode: loss, koleo, every parameter gradient and the gradient norm at the gates of
    tests/test_fp32_gpu.py, with Sinkhorn-Knopp centring, with KoLeo (weight 0.1), with both."""
    _, refs = step_reference()
    ref, kw = refs[config], CONFIGS[config]
    eng = make_engine(dev, "fp32", **kw)
    eng.set_hyper()
    eng.forward_backward(step_tiles().to(dev))
    torch.cuda.synchronize()
    dl = abs(float(eng.loss) - ref["loss"])
    gn, worst = _grad_gates(eng, ref["grads"])
    msg = f"[fp32 step {config}] loss err {dl:.2e}, grad-norm rel {gn:.2e}, worst parameter gradient {worst[0]:.2e} ({worst[1]})"
    if "koleo_weight" in kw:
        dk = abs(float(eng.koleo) - ref["koleo"])
        msg += f", koleo {float(eng.koleo):.5f} err {dk:.2e}"
        assert torch.equal(eng.koleo_nn.cpu().long(), ref["nn"])
        assert dk <= LOSS_TOL
    if "centering" in kw:
        dc = float(np.abs(C.gauge(eng.sk_center.cpu().numpy()) - C.gauge(ref["center"].numpy())).max())
        msg += f", gauged sk_center against the oracle's teacher logits {dc:.2e}"
    print(msg)
    assert dl <= LOSS_TOL and gn <= GNORM_TOL and worst[0] <= GRAD_TOL, msg


@gpu
def test_bf16_step_with_koleo(dev):
    """The 16-bit step with both options.  The features come from the GPU, so the neighbour check is tie-robust: every koleo_nn[i]
    has a dot within 4 D 2^-24 of the float64 maximum on the read-back features; koleo within 1e-4 relative of float64 on those
    features; what gv_koleo_bwd added to dfeats (snapshots around the call: the DINO part is the same launch's input) is the float64
    gradient for THAT index within weight x the float32 restatement's bound plus 2^-8 of the result; loss, per-parameter gradients
    and gradient norm under the gates of tests/test_engine_gpu.py as they stand (loss 1e-3; _check_grads: 5e-2 and 1e-2), against the
    oracle with KoLeo's index held at the one the GPU took (on its 16-bit features it need not be the float32 oracle's arg-max)."""
    o = ops()
    eng = make_engine(dev, "bf16", **CONFIGS["both"])
    snaps, real = [], o.koleo_bwd

    def spy(dfeats, *a, **kw):
        snaps.append(dfeats.float().cpu())
        real(dfeats, *a, **kw)
        snaps.append(dfeats.float().cpu())
    o.koleo_bwd = spy
    try:
        eng.set_hyper()
        eng.forward_backward(step_tiles().to(dev))
        torch.cuda.synchronize()
    finally:
        o.koleo_bwd = real
    G, B, D = eng.G, eng.B, eng.D
    feats = eng.hb_s.feats.float().cpu().numpy()
    nn = eng.koleo_nn.cpu().numpy()
    f64_ = C.koleo(feats, G, B)
    y = f64_["y"]
    for g in range(G):
        yc = y[g * B:(g + 1) * B]
        dots = yc @ yc.T
        np.fill_diagonal(dots, -np.inf)
        chosen = dots[np.arange(B), nn[g * B:(g + 1) * B]]
        assert bool((dots.max(1) - chosen <= 4 * D * 2.0 ** -24).all()), (g, dots.max(1) - chosen)
    mine = C.koleo(feats, G, B, nn=nn)
    rk = abs(float(eng.koleo) - float(mine["koleo"])) / abs(float(mine["koleo"]))
    g64, g32 = C.koleo_grad(feats, G, B, nn), C.koleo_grad(feats, G, B, nn, np.float32)
    bnd = W_KOLEO * C.bound(g32, g64)
    before, after = snaps
    added = (after - before).double()[:G * B]
    want = W_KOLEO * torch.from_numpy(g64)
    err = (added - want).abs()
    allow = bnd + 2.0 ** -8 * after[:G * B].double().abs()
    ref = reference_for("both", tuple(int(i) for i in nn))
    gn, worst = _grad_gates(eng, ref["grads"])
    dl = abs(float(eng.loss) - ref["loss"])
    print(f"[bf16 step] koleo {float(eng.koleo):.5f} rel err {rk:.2e}; added gradient worst err / bound {float((err / allow).max()):.3f} "
          f"(max |w gx| {float(want.abs().max()):.3e}); loss err {dl:.2e}, grad-norm rel {gn:.2e}, worst gradient {worst[0]:.2e} ({worst[1]})")
    assert rk <= 1e-4 and bool((err <= allow).all())
    assert torch.equal(after[G * B:], before[G * B:]), "KoLeo reached the local crops' rows"
    assert dl <= 1e-3, dl
    _check_grads(eng.grads(), ref["grads"], skip=("head.last_layer.weight_g",))


@gpu
def test_options_off_change_nothing(dev):
    """centering='center', koleo_weight=0 spelled out, against engines built without the arguments.  Everything the forward pass
    leaves without atomics is bit-identical (features, logits, loss, the logit gradient).  The gradient arena and the centre sum of
    this engine are not bitwise reproducible from one run to the next (the head's split-K products and gv_dino_loss's centre sum
    accumulate with f32 atomics in arrival order: profiles/poison_spread.txt, "dino_tiny_fp32"), so two engines built WITHOUT the
    arguments already differ there; the spelled-out engine must be no farther from the first of them than GATE_FACTOR = 4 x the
    largest distance of three further plain engines from it (the gate of tests/test_poison_gpu.py, over several pairs as there),
    and bit-identical whenever they all are.  That the launches and their arguments are the same is held without a GPU by
    tests/test_dinov2_terms_host.py::test_options_off_leave_the_full_trace."""
    engines = [make_engine(dev, "fp32") for _ in range(4)] + [make_engine(dev, "fp32", centering="center", sinkhorn_iters=5, koleo_weight=0.0)]
    tiles = step_tiles().to(dev)
    for e in engines:
        e.set_hyper()
        e.forward_backward(tiles)
    torch.cuda.synchronize()
    plain, others, spelled = engines[0], engines[1:4], engines[4]
    assert spelled.sk_center is None and spelled.koleo is None and spelled.koleo_nn is None
    assert torch.equal(plain.loss, spelled.loss)
    for hb in ("hb_s", "hb_t"):
        for name in ("feats", "logits"):
            assert torch.equal(getattr(getattr(plain, hb), name), getattr(getattr(spelled, hb), name)), (hb, name)
    assert torch.equal(plain.hb_s.dlogits, spelled.hb_s.dlogits)
    for what, pick in (("gradient arena", lambda e: e.arena.g), ("centre sum", lambda e: e.center_sum)):
        pairs = [_rel(pick(e), pick(plain)) for e in others]
        own, d = max(pairs), _rel(pick(spelled), pick(plain))
        print(f"[options off] {what}: plain engines differ from the first by {', '.join(f'{x:.3e}' for x in pairs)}, the spelled-out one by {d:.3e}")
        assert d <= 4.0 * own and (own > 0 or torch.equal(pick(plain), pick(spelled))), what


@gpu
def test_two_micro_batches_average_koleo(dev):
    eng = make_engine(dev, "fp32", **CONFIGS["both"])
    t1 = step_tiles().to(dev)
    t2 = t1.flip(0).contiguous().roll(7, 1)
    singles = []
    for t in (t1, t2):
        eng.set_hyper()
        eng.forward_backward(t)
        singles.append((float(eng.koleo), float(eng.loss)))
    eng.step_micro([t1, t2])
    torch.cuda.synchronize()
    want_k, want_l = (singles[0][0] + singles[1][0]) / 2, (singles[0][1] + singles[1][1]) / 2
    print(f"[micro] koleo {singles[0][0]:.6f} and {singles[1][0]:.6f} -> {float(eng.koleo):.6f}; loss {float(eng.loss):.6f} (mean {want_l:.6f})")
    assert singles[0][0] != singles[1][0]
    assert abs(float(eng.koleo) - want_k) <= 2e-7 * abs(want_k) + 1e-7 and abs(float(eng.loss) - want_l) <= 1e-6 * abs(want_l)


def _worker(mode, env=None, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in ("GIPVIT_ACT_FORMAT", "GIPVIT_POISON")}
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dinov2_terms_worker.py"), mode], env=e, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().endswith("DINOV2 TERMS OK")


@gpu
def test_poisoned_buffers_two_steps(dev):
    """GIPVIT_POISON=1 (a process of its own: the switch is read at allocation): two steps with both options on, every scratch buffer
    refilled with NaN between them -- loss, koleo, sk_center and the arena stay finite."""
    _worker("poison", {"GIPVIT_POISON": "1"})


@gpu
def test_float16_build_scales_the_koleo_gradient(dev):
    """The float16 library in a process of its own: under a loss scale of 1024 the part gv_koleo_bwd adds to dfeats is 1024 x the
    part it adds under a scale of 1, within the 16-bit bound."""
    _worker("f16", {"GIPVIT_ACT_FORMAT": "f16"})


def _rank(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gipvit.dist import RcclReducer, shard_range
    from gipvit.engine import DinoEngine
    from gipvit.models import init_vit_state, init_dino_head_state
    eng = DinoEngine(arch=ARCH, img_size=224, out_dim=K_OUT, batch=2, lr=1e-4, weight_decay=0.04, device="cuda:0", reducer=RcclReducer(), **CONFIGS["both"])
    eng.load_state(init_vit_state(ARCH, 224, 0, seed=0), init_dino_head_state(192, K_OUT, seed=1))
    lo, hi = shard_range(B_STEP, rank, world)
    loss = float(eng.step(step_tiles()[lo:hi].to("cuda:0")))
    torch.cuda.synchronize()
    q.put((rank, eng.sk_center.cpu().numpy(), eng.hb_t.logits.float().cpu().numpy(), float(eng.koleo), loss))      # numpy: pickled by value
    dist.destroy_process_group()


@gpu
def test_two_ranks_share_one_sinkhorn(dev):
    """Two ranks (gloo, both on this GPU) with two tiles each: sk_center bitwise equal on both, and -- after the gauge -- within the
    bound of the float64 iteration over ALL ranks' teacher rows (read back from both), which is what the reduction has to reproduce.
    Then ONE process on all four tiles: its own centre under the same bound on its own rows, and the two centres against each other.
    The 16-bit teacher forward of two tiles need not give the bits of the forward of four (a product may pick another kernel by its
    row count), and the bound knows nothing of that: the float64 centres of the two sets of logits say what the difference of the
    logits alone moves, and the allowance is then the two bounds plus that; when the logits agree bit for bit it is the one process's
    bound alone.  koleo is local
    to a rank by definition and is not compared across the split."""
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ps = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = sorted([q.get(timeout=300) for _ in ps], key=lambda t: t[0])
    [p.join(60) for p in ps]
    assert np.array_equal(res[0][1], res[1][1]), "the ranks hold different sk_center"
    T = np.concatenate([res[0][2], res[1][2]])
    tau = 0.04
    a64, s_min = C.sinkhorn_log(T, tau, 3)
    a32, _ = C.sinkhorn_log(T, tau, 3, np.float32)
    c64 = C.gauge(-tau * a64)
    bnd = C.bound(C.gauge(-np.float32(tau) * a32), c64)
    err = float(np.abs(C.gauge(res[0][1]) - c64).max())
    alone, _ = C.sinkhorn_log(res[0][2], tau, 3)
    print(f"[two ranks] max |gauged sk_center - f64 over all rows| {err:.3e}, bound {bnd:.3e}; a rank alone would be off by "
          f"{float(np.abs(C.gauge(-tau * alone) - c64).max()):.3e}; koleo {res[0][3]:.5f} / {res[1][3]:.5f}, loss {res[0][4]:.5f} / {res[1][4]:.5f}")
    assert s_min >= 1e-30 and err <= bnd
    assert all(math.isfinite(v) for r in res for v in r[3:])
    from gipvit.engine import DinoEngine
    from gipvit.models import init_vit_state, init_dino_head_state
    one = DinoEngine(arch=ARCH, img_size=224, out_dim=K_OUT, batch=B_STEP, lr=1e-4, weight_decay=0.04, device=dev, **CONFIGS["both"])
    one.load_state(init_vit_state(ARCH, 224, 0, seed=0), init_dino_head_state(192, K_OUT, seed=1))
    one.set_hyper()
    one.forward_backward(step_tiles().to(dev))
    torch.cuda.synchronize()
    T1 = one.hb_t.logits.float().cpu().numpy()
    b64, s1 = C.sinkhorn_log(T1, tau, 3)
    b32, _ = C.sinkhorn_log(T1, tau, 3, np.float32)
    d64 = C.gauge(-tau * b64)
    bnd1 = C.bound(C.gauge(-np.float32(tau) * b32), d64)
    c1 = C.gauge(one.sk_center.cpu().numpy())
    err1, moved = float(np.abs(c1 - d64).max()), float(np.abs(d64 - c64).max())
    direct = float(np.abs(C.gauge(res[0][1]) - c1).max())
    rows = lambda t: t.reshape(2, -1, K_OUT)       # [crop, tile, K]
    same = np.array_equal(np.concatenate([rows(res[0][2]), rows(res[1][2])], axis=1), rows(T1))
    print(f"[one process] max |gauged sk_center - f64| {err1:.3e}, bound {bnd1:.3e}; two ranks against one process {direct:.3e}; the teacher logits "
          f"{'agree bit for bit' if same else 'differ'}: their float64 centres by {moved:.3e}")
    assert s1 >= 1e-30 and err1 <= bnd1
    assert direct <= (bnd1 if same else bnd + bnd1 + moved)       # the same logits: the one process's bound, as it stands


@gpu
def test_driver_hands_the_options_to_the_engine(dev, tmp_path, monkeypatch, caplog):
    """train.py --dino with both options, one short epoch: the engine it builds receives the flags' values, the log line carries
    'KoLeo:' and summary.csv keeps its columns."""
    import csv
    import logging
    sys.path.insert(0, ROOT)
    import train
    from gipvit import engine
    seen = []

    class Spy(engine.DinoEngine):
        def __init__(self, *a, **kw):
            seen.append(kw)
            super().__init__(*a, **kw)
    monkeypatch.setattr(engine, "DinoEngine", Spy)
    base = ["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--out-dim", "1024", "--batches-per-epoch", "2", "--lr", "1e-4",
            "--epochs", "1", "--log-interval", "1", "--output", str(tmp_path), "--seed", "7", "--no-validate"]
    with caplog.at_level(logging.INFO):
        assert train.main(base + ["--experiment", "opts", "--centering", "sinkhorn_knopp", "--sinkhorn-iters", "2", "--koleo-weight", "0.1"]) == 0
    assert len(seen) == 1 and (seen[0]["centering"], seen[0]["sinkhorn_iters"], seen[0]["koleo_weight"]) == ("sinkhorn_knopp", 2, 0.1)
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Train:")]
    assert lines and all("KoLeo: " in l for l in lines), lines
    assert all(math.isfinite(float(l.split("KoLeo: ")[1].split()[0])) for l in lines)
    caplog.clear()
    with caplog.at_level(logging.INFO):
        assert train.main(base + ["--experiment", "plain"]) == 0
    assert (seen[1]["centering"], seen[1]["koleo_weight"]) == ("center", 0.0)
    assert not any("KoLeo" in r.getMessage() for r in caplog.records)
    head = lambda n: next(csv.reader(open(tmp_path / n / "summary.csv")))
    assert head("opts") == head("plain")
