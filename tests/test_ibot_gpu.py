"""GPU: the iBOT kernels (csrc/ibot.hip) one by one against fp64 torch, with poisoned outputs and guard elements behind them, then
the DINO + iBOT step against the torch-autograd restatement of tests/ibot_cases.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ibot_cases as C

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, GUARD = 12345.0, 4096


def ops():
    from gipvit import ops as o
    return o


def guarded(dev, n, dtype=f32, fill=SENT):
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[:n]


def guard_ok(buf, n, what, fill=SENT):
    assert torch.equal(buf[n:], torch.full_like(buf[n:], fill)), f"{what}: guard elements behind the output were written"


def loss_ws(M, K, dev):
    """gv_ibot_loss's scratch, NaN-filled: all of it is written before it is read"""
    from gipvit import _lib
    return torch.full((_lib.lib.gv_ibot_loss_workspace_bytes(M, K) // 4,), float("nan"), device=dev)


def rint(shape, lo, hi, seed, dtype=f32):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def table(n_img, N, M, seed, dev):
    """M unique patch rows of n_img images of N tokens, ascending, with the first and the last patch of the first and the last image
    among them when M allows."""
    must = [1, N - 1, (n_img - 1) * N + 1, n_img * N - 1][:M]
    rest = [r for r in range(n_img * N) if r % N and r not in must]
    pick = torch.randperm(len(rest), generator=torch.Generator().manual_seed(seed))[:M - len(must)].tolist()
    rows = sorted(set(must) | {rest[i] for i in pick})
    assert len(rows) == M
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(rows, dtype=torch.int32).to(dev)


# ------------------------------------------------------------------------------------------------------------------ mask tokens
@pytest.mark.parametrize("D", [192, 384, 768])
def test_mask_tokens_fwd(dev, D):
    """x[rows[i]] = mask_token + pos[rows[i] mod N]: one f32 addition, so bit-exact; every other row bit-untouched; the table holds the
    first and the last patch of the first and the last image; guard elements behind x."""
    n_img, N = 5, 17
    g = torch.Generator().manual_seed(D)
    x0, mt, pos = torch.randn(n_img * N, D, generator=g), torch.randn(D, generator=g), torch.randn(N, D, generator=g)
    for M in (1, 4, 33):
        rows, rows_d = table(n_img, N, M, M, dev)
        buf, x = guarded(dev, n_img * N * D)
        x = x.view(n_img * N, D); x.copy_(x0)
        ops().mask_tokens_fwd(x, mt.to(dev), pos.to(dev), rows_d, M, N, D)
        want = x0.clone()
        want[rows.long()] = mt + pos[rows.long() % N]
        assert torch.equal(x.cpu(), want), M
        guard_ok(buf, n_img * N * D, "x")


@pytest.mark.parametrize("D", [192, 384, 768])
@pytest.mark.parametrize("M", [1, 64, 65, 200])
def test_mask_tokens_bwd(dev, M, D):
    """On integers -2..2 (every f32 sum exact, the gate tests/test_row_kernels_gpu.py::test_tokens_bwd_exact applies to gv_tokens_bwd's
    dcls: torch.equal against the exact sum): dmask_token, with and without accumulation; the marked rows of the compact patch gradient
    exact zeros and every other row bit-equal; M = 1, one full workgroup slice (64), one more, and four slices; then on normal data two
    runs bitwise equal and the fp64 sum within f32 rounding of M terms."""
    n_img, N = 7, 37
    o = ops()
    g = rint((n_img * N, D), -2, 2, seed=M + D)
    rows, rows_d = table(n_img, N, M, M + 1, dev)
    pr = (rows.long() // N) * (N - 1) + rows.long() % N - 1
    ws = torch.full((o.L.lib.gv_mask_tokens_workspace_bytes(M, D) // 4,), float("nan"), device=dev)
    for dt in (bf16, f32):
        for acc in (False, True):
            gp0 = rint((n_img * (N - 1), D), -3, 3, seed=5)
            pbuf, gp = guarded(dev, gp0.numel(), dt); gp = gp.view(gp0.shape); gp.copy_(gp0)
            dbuf, dm = guarded(dev, D)
            if acc:
                dm.fill_(3.0)
            o.mask_tokens_bwd(g.to(dev), gp, dm, rows_d, ws, M, N, D, accumulate=acc)
            assert torch.equal(dm.cpu(), g[rows.long()].sum(0) + (3.0 if acc else 0.0)), (dt, acc)
            want = gp0.clone(); want[pr] = 0.0
            assert torch.equal(gp.float().cpu(), want), (dt, acc)
            guard_ok(pbuf, gp0.numel(), "gpatch"); guard_ok(dbuf, D, "dmask_token")
    gr = torch.randn(n_img * N, D, generator=torch.Generator().manual_seed(3))
    outs = []
    for _ in range(2):
        gp, dm = torch.zeros(n_img * (N - 1), D, dtype=bf16, device=dev), torch.full((D,), float("nan"), device=dev)
        o.mask_tokens_bwd(gr.to(dev), gp, dm, rows_d, ws, M, N, D, accumulate=False)
        outs.append(dm.cpu())
    assert torch.equal(outs[0], outs[1])
    ref = gr[rows.long()].double().sum(0)
    bound = M * 2.0 ** -24 * float(gr[rows.long()].abs().double().sum(0).max()) + 1e-30
    assert float((outs[0].double() - ref).abs().max()) <= bound


# ------------------------------------------------------------------------------------------------------- final norm on a row table
@pytest.mark.parametrize("D", [192, 384, 768])
@pytest.mark.parametrize("M", [1, 3, 257])
def test_row_table_final_norm(dev, M, D):
    """Forward: gather + gv_layernorm_fwd is bit-equal to gv_layernorm_fwd on a torch-gathered copy (features and statistics).
    Backward: gv_layernorm_bwd on the compact rows + scatter is bit-equal to gv_layernorm_bwd plus a torch scatter, residual gradient
    and the 16-bit / f32 dY with the rows' stochastic-depth factors; rows outside the table keep their bits; guards behind all."""
    from gipvit import _lib as L
    o = ops()
    n_img, N = 9, 37
    T = n_img * N
    g = torch.Generator().manual_seed(M * 1000 + D)
    x, gamma, beta = torch.randn(T, D, generator=g) * 2 + 0.3, torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    scale = (torch.rand(T, generator=g) < 0.7).float() / 0.7
    rows, rows_d = table(n_img, N, M, M, dev)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    for dt in (bf16, f32):
        xbuf, xc = guarded(dev, M * D); xc = xc.view(M, D)
        sbuf, sc = guarded(dev, M)
        o.rows_gather(xd, rows_d, xc, M, D, T, scale=scale.to(dev), scale_out=sc)
        assert torch.equal(xc.cpu(), x[rows.long()]) and torch.equal(sc.cpu(), scale[rows.long()])
        guard_ok(xbuf, M * D, "gathered x"); guard_ok(sbuf, M, "gathered scale")
        y, y2 = torch.empty(M, D, dtype=dt, device=dev), torch.empty(M, D, dtype=dt, device=dev)
        _, mean, rstd = o.layernorm_fwd(xc, gd, bd, M, D, y=y)
        _, mean2, rstd2 = o.layernorm_fwd(x[rows.long()].to(dev), gd, bd, M, D, y=y2)
        assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
        dy = torch.randn(M, D, generator=g).to(dt).to(dev)
        gc, gbc = torch.empty(M, D, device=dev), torch.empty(M, D, dtype=dt, device=dev)
        parts = torch.full((L.LN_PARTIAL_BLOCKS, 3, D), float("nan"), device=dev)
        o.layernorm_bwd(dy, xc, mean, rstd, gd, gc, gbc, parts, M, D, g_init=True, gb_scale=sc)
        g0, gb0 = torch.randn(T, D, generator=g), torch.randn(T, D, generator=g).to(dt)
        gbuf, G = guarded(dev, T * D); G = G.view(T, D); G.copy_(g0)
        bbuf, GB = guarded(dev, T * D, dt); GB = GB.view(T, D); GB.copy_(gb0)
        o.rows_scatter(gc, G, rows_d, M, D, T, gb_src=gbc, gb=GB)
        wg, wgb = g0.clone(), gb0.clone()
        wg[rows.long()] = gc.cpu(); wgb[rows.long()] = gbc.cpu()
        assert torch.equal(G.cpu(), wg) and torch.equal(GB.cpu(), wgb), dt
        guard_ok(gbuf, T * D, "g"); guard_ok(bbuf, T * D, "gb")
        # ... and the norm's backward itself against fp64 autograd on the gathered rows (the gate of test_fp32_gpu.py::test_layernorm_f32_io)
        if dt == f32:
            xr = x[rows.long()].double().requires_grad_(True)
            torch.nn.functional.layer_norm(xr, (D,), gamma.double(), beta.double(), 1e-6).backward(dy.cpu().double())
            rel = float((gc.cpu().double() - xr.grad).norm() / xr.grad.norm())
            assert rel < 2e-6, rel
            assert torch.equal(gbc.cpu(), gc.cpu() * scale[rows.long()][:, None])


# ------------------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("K", [1, 8, 1000, 65536])
@pytest.mark.parametrize("M", [1, 2, 67])
def test_ibot_loss(dev, M, K):
    """gv_ibot_loss / _f32 against fp64 torch at the gates tests/test_kernels_gpu.py::test_dino_loss applies to gv_dino_loss: the loss
    within 1e-4 max(1, |loss|), the column sums at rtol = atol = 1e-4, the gradient at rtol 1e-2 and atol 1e-2 of its largest element.
    Both operand modes are held to those gates (gv_dino_loss_f32 has no kernel-level gate of its own; the step tests below hold the
    f32 mode to tests/test_fp32_gpu.py's).  Slot K of center_sum is M exactly; center_sum and the loss are bitwise equal
    over two runs; the zero-weight row's gradient row is exact zeros; the gradient carries ibot_weight and grad_scale; guards behind
    every output, and NaN scratch."""
    o = ops()
    s, t, c, w = C.loss_inputs(M, K)
    W, gs, ts, tt = 0.5, 0.25, 0.1, 0.04
    sr = s.double().requires_grad_(True)
    loss_ref, csum_ref = C.ibot_loss_ref(sr, t.double(), c.double(), w.double(), ts, tt)
    (loss_ref * W * gs).backward()
    gmax = float(sr.grad.abs().max())
    for dt, k in ((bf16, 1.0), (f32, 1.0)):
        runs = []
        for _ in range(2):
            dbuf, ds = guarded(dev, M * K, dt, fill=float("nan")); ds = ds.view(M, K)
            lbuf, loss = guarded(dev, 1)
            cbuf, csum = guarded(dev, K + 1)
            ws = loss_ws(M, K, dev)
            o.ibot_loss(s.to(dev), t.to(dev), c.to(dev), w.to(dev), ds, loss, csum, ws, M, K, ts, tt, W, grad_scale=gs)
            runs.append((loss.cpu().clone(), csum.cpu().clone(), ds.float().cpu().clone()))
            assert torch.isnan(dbuf[M * K:]).all(); guard_ok(lbuf, 1, "loss"); guard_ok(cbuf, K + 1, "center_sum")
        (l, cs, d), (l2, cs2, _) = runs
        assert torch.equal(l, l2) and torch.equal(cs, cs2), dt
        assert float(cs[K]) == float(M)
        print(f"[ibot_loss M={M} K={K} {dt}] loss {float(l):.6f} ref {float(loss_ref):.6f}, grad max err {float((d.double() - sr.grad).abs().max()):.2e} of {gmax:.2e}")
        assert abs(float(l) - float(loss_ref)) < k * 1e-4 * max(1.0, abs(float(loss_ref)))
        assert torch.allclose(cs[:K].double(), csum_ref, rtol=1e-4, atol=1e-4)
        assert torch.allclose(d.double(), sr.grad, rtol=k * 1e-2, atol=k * 1e-2 * gmax)
        if M > 1:
            assert float(d[M // 2].abs().max()) == 0.0 and not torch.signbit(d[M // 2]).any()


def test_ibot_loss_zero_weight_row_ignores_its_logits(dev):
    """A row of weight 0 adds nothing and gets exact zeros even when its logits are not finite."""
    o = ops()
    M, K = 3, 256
    s, t, c, w = C.loss_inputs(M, K)
    s[1] = float("inf"); t[1, 0] = float("nan")
    ds, loss, csum = torch.full((M, K), float("nan"), device=dev), torch.empty(1, device=dev), torch.empty(K + 1, device=dev)
    o.ibot_loss(s.to(dev), t.to(dev), c.to(dev), w.to(dev), ds, loss, csum, loss_ws(M, K, dev), M, K, 0.1, 0.04, 1.0)
    keep = [0, 2]
    ref, _ = C.ibot_loss_ref(s[keep].double(), t[keep].double(), c.double(), w[keep].double(), 0.1, 0.04)
    assert math.isfinite(float(loss)) and abs(float(loss) - float(ref)) < 1e-5 and float(ds[1].abs().max()) == 0.0


def test_patch_center_update(dev):
    """c <- m c + (1 - m) sums / count with the count read from slot K: a count of 67, of 1, and 0 (the centre keeps its bits)."""
    o = ops()
    K = 1000
    g = torch.Generator().manual_seed(4)
    c0 = torch.randn(K, generator=g)
    for n in (67.0, 1.0, 0.0):
        tot = torch.cat([torch.randn(K, generator=g) * max(n, 1.0), torch.tensor([n])])
        buf, c = guarded(dev, K); c.copy_(c0)
        o.patch_center_update(c, tot.to(dev), K, 0.9)
        ref = C.patch_center_ref(c0.double(), tot.double(), 0.9)
        if n == 0.0:
            assert torch.equal(c.cpu(), c0)
        else:
            assert torch.allclose(c.cpu().double(), ref, rtol=1e-5, atol=1e-6)       # the gate of test_dino_loss's centre
        guard_ok(buf, K, "center")


# ------------------------------------------------------------------------------------------------------------------------ the step
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _grad_report(got, ref, skip=("head.last_layer.weight_g",)):
    keys = [k for k, r in ref.items() if r is not None and k not in skip]
    gn_g = math.sqrt(sum(float((got[k].double() ** 2).sum()) for k in keys))
    gn_r = math.sqrt(sum(float((ref[k].double() ** 2).sum()) for k in keys))
    worst = max((_rel(got[k], ref[k]), k) for k in keys if float(ref[k].abs().max()) > 1e-12)
    return worst, abs(gn_g - gn_r) / gn_r


CASES = [("vit_tiny", 64, 32, 512), ("vit_small", 96, 32, 512)]     # unfused, and the fused full-row path


@pytest.fixture(scope="module")
def refs():
    """The reference step of every case, computed once and shared."""
    out = {}

    def get(arch, gsize, lsize, K, drop=False):
        key = (arch, drop)
        if key not in out:
            torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
            orc, mt, pc, tiles = C.step_case(arch, gsize, lsize, K)
            masks = C.fixed_masks(4, (gsize // 16) ** 2)
            d = C.vo.drop_path_factors(12, 4 * 2, 0.4, torch.Generator().manual_seed(2)) if drop else None
            out[key] = (orc, mt, pc, tiles, masks, d, C.reference_step(orc, mt, tiles, masks, 1.0, pc, drop=d))
        return out[key]
    return get


@pytest.mark.parametrize("arch,gsize,lsize,K", CASES)
def test_step_fp32(dev, refs, arch, gsize, lsize, K):
    """fp32 operand mode at the gates tests/test_fp32_gpu.py::test_fp32_dino_step_gates holds the DINO step to: logits 1e-4 (of
    max(1, largest)), loss 1e-4, centre sums 1e-5 relative, gradient norm 1e-3, every gradient 1e-3 -- mask_token's and the head's
    included.  ``ibot`` and the patch rows' logits and sums are new quantities: they take the gates of their neighbours (the loss,
    the CLS logits, center_sum).  Then an optimizer step: the patch centre against the formula at 1e-4 (the gate of the CLS centre)."""
    from gipvit.masking import MaskPlan
    orc, mt, pc, tiles, masks, _, r = refs(arch, gsize, lsize, K)
    eng = C.make_engine(orc, mt, pc, K, 2, dev, precision="fp32")
    plan = MaskPlan.from_masks(masks, dev)
    eng.set_hyper()
    eng.forward_backward(tiles.to(dev), masks=plan)
    torch.cuda.synchronize()
    M = plan.M
    for got, ref, nm in ((eng.hb_t.logits, r["t_out"], "teacher"), (eng.hb_s.logits, r["s_out"], "student"),
                         (eng.pr_t.hb.logits[:M], r["tp_out"], "teacher patch"), (eng.pr_s.hb.logits[:M], r["sp_out"], "student patch")):
        err = float((got.cpu() - ref).abs().max())
        assert err <= 1e-4 * max(1.0, float(ref.abs().max())), (nm, err)
    dl, di = abs(float(eng.loss) - float(r["loss"])), abs(float(eng.ibot) - float(r["ibot"]))
    worst, gn = _grad_report(eng.grads(), r["grads"])
    print(f"[ibot fp32 {arch}] |dloss| {dl:.2e} |dibot| {di:.2e} (ibot {float(r['ibot']):.4f}) worst gradient {worst[0]:.2e} ({worst[1]}) "
          f"mask_token {_rel(eng.grads()['backbone.mask_token'], r['grads']['backbone.mask_token']):.2e} grad-norm rel {gn:.2e}")
    assert dl <= 1e-4 and di <= 1e-4
    assert _rel(eng.center_sum, r["center_sum"][0]) < 1e-5 and _rel(eng.patch_center_sum[:K], r["patch_sum"][:K]) < 1e-5
    assert float(eng.patch_center_sum[K]) == float(M)
    assert gn <= 1e-3 and worst[0] <= 1e-3, (gn, worst)
    assert float(r["grads"]["backbone.mask_token"].abs().max()) > 1e-8
    eng.optimizer_step()
    torch.cuda.synchronize()
    assert _rel(eng.patch_center, C.patch_center_ref(pc, r["patch_sum"], 0.9)) < 1e-4


@pytest.mark.parametrize("arch,gsize,lsize,K", CASES)
def test_step_bf16(dev, refs, arch, gsize, lsize, K):
    """The training path at the gates of tests/test_engine_gpu.py::test_dino_forward_backward_parity_configs: logits 2 % of the
    largest, loss 1e-3, every gradient 5 %, gradient norm 1 %, centre sums 1e-2.  ``ibot`` takes the loss's gate, the patch rows'
    logits and sums those of the CLS rows."""
    from gipvit.masking import MaskPlan
    orc, mt, pc, tiles, masks, _, r = refs(arch, gsize, lsize, K)
    eng = C.make_engine(orc, mt, pc, K, 2, dev)
    plan = MaskPlan.from_masks(masks, dev)
    eng.set_hyper()
    eng.forward_backward(tiles.to(dev), masks=plan)
    torch.cuda.synchronize()
    M = plan.M
    for got, ref, nm in ((eng.hb_t.logits, r["t_out"], "teacher"), (eng.hb_s.logits, r["s_out"], "student"),
                         (eng.pr_t.hb.logits[:M], r["tp_out"], "teacher patch"), (eng.pr_s.hb.logits[:M], r["sp_out"], "student patch")):
        err = float((got.cpu() - ref).abs().max())
        assert err <= 2e-2 * float(ref.abs().max()), (nm, err)
    dl, di = abs(float(eng.loss) - float(r["loss"])), abs(float(eng.ibot) - float(r["ibot"]))
    worst, gn = _grad_report(eng.grads(), r["grads"])
    print(f"[ibot bf16 {arch}] |dloss| {dl:.2e} |dibot| {di:.2e} worst gradient {worst[0]:.2e} ({worst[1]}) grad-norm rel {gn:.2e}")
    assert dl <= 1e-3 and di <= 1e-3
    assert _rel(eng.center_sum, r["center_sum"][0]) < 1e-2 and _rel(eng.patch_center_sum[:K], r["patch_sum"][:K]) < 1e-2
    assert worst[0] <= 5e-2 and gn <= 1e-2, (worst, gn)


def test_step_drop_path_fp32(dev, refs):
    """One step with stochastic-depth factors set (rate 0.4: several of the marked rows' images are dropped in the last block), at
    the fp32 gates: the rows' factor reaches the last block's MLP-half dY as gb_scale does for the CLS rows."""
    from gipvit.masking import MaskPlan
    arch, gsize, lsize, K = CASES[0]
    orc, mt, pc, tiles, masks, drop, r = refs(arch, gsize, lsize, K, drop=True)
    assert float(drop[11, 1, :4].min()) == 0.0 or float(drop[11, 1, :4].max()) > 1.0
    eng = C.make_engine(orc, mt, pc, K, 2, dev, precision="fp32")
    eng.set_drop_path(drop.to(dev))
    eng.set_hyper()
    eng.forward_backward(tiles.to(dev), masks=MaskPlan.from_masks(masks, dev))
    torch.cuda.synchronize()
    worst, gn = _grad_report(eng.grads(), r["grads"])
    print(f"[ibot fp32 drop-path] worst gradient {worst[0]:.2e} ({worst[1]}) grad-norm rel {gn:.2e}")
    assert abs(float(eng.loss) - float(r["loss"])) <= 1e-4 and abs(float(eng.ibot) - float(r["ibot"])) <= 1e-4
    assert gn <= 1e-3 and worst[0] <= 1e-3, (gn, worst)


def test_two_micro_batches_are_the_sum_of_their_parts(dev):
    """step_micro over two micro-batches with two plans (different M, the second with marks in the first image) against the two
    forward_backward calls on their own, fp32 operand mode: gradients add up (1e-5 relative: atomics in the weight-gradient
    products reorder sums), ``ibot`` and ``loss`` are the means, the patch sums and the count add."""
    from gipvit.masking import MaskPlan
    arch, gsize, lsize, K = CASES[0]
    orc, mt, pc, tiles, = C.step_case(arch, gsize, lsize, K)
    tiles2 = C.vo.synth_tiles(2, 256, seed=77)
    plans = [MaskPlan.from_masks(C.fixed_masks(4, 16, v), dev) for v in (0, 1)]
    assert plans[0].M != plans[1].M
    eng = C.make_engine(orc, mt, pc, K, 2, dev, precision="fp32")
    parts = []
    for tl, pl in zip((tiles, tiles2), plans):
        eng.set_hyper()
        eng.forward_backward(tl.to(dev), masks=pl)
        torch.cuda.synchronize()
        parts.append((eng.grads(), float(eng.loss), float(eng.ibot), eng.patch_center_sum.clone()))
    eng.set_hyper(n_micro=2)
    for j, (tl, pl) in enumerate(zip((tiles, tiles2), plans)):
        eng.forward_backward(tl.to(dev), micro=(j, 2), masks=pl)
    torch.cuda.synchronize()
    got = eng.grads()
    worst = max((_rel(got[k], parts[0][0][k] + parts[1][0][k]), k) for k in got if float(parts[0][0][k].abs().max()) > 1e-12)
    assert worst[0] < 1e-5, worst
    assert abs(float(eng.ibot) - 0.5 * (parts[0][2] + parts[1][2])) < 1e-6 and abs(float(eng.loss) - 0.5 * (parts[0][1] + parts[1][1])) < 1e-6
    assert _rel(eng.patch_center_sum, parts[0][3] + parts[1][3]) < 1e-6 and float(eng.patch_center_sum[K]) == plans[0].M + plans[1].M
    with pytest.raises(ValueError):
        eng.step_micro([tiles.to(dev), tiles2.to(dev)], masks=plans[:1])
    with pytest.raises(ValueError):
        eng.forward_backward(tiles.to(dev))


def test_no_marked_patch_is_the_dino_step_on_every_token(dev):
    """M = 0: no patch launch, ibot = 0, the patch centre unchanged by the optimizer step, and the DINO gradients finite."""
    from gipvit.masking import MaskPlan
    arch, gsize, lsize, K = CASES[0]
    orc, mt, pc, tiles = C.step_case(arch, gsize, lsize, K)
    eng = C.make_engine(orc, mt, pc, K, 2, dev)
    eng.step(tiles.to(dev), masks=MaskPlan.from_masks(np.zeros((4, 16), bool), dev))
    torch.cuda.synchronize()
    assert float(eng.ibot) == 0.0 and torch.equal(eng.patch_center.cpu(), pc) and math.isfinite(float(eng.loss))
    assert float(eng.grads()["backbone.mask_token"].abs().max()) == 0.0


POISON = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import ibot_cases as C
from gipvit import engine
from gipvit.masking import MaskPlan
dev = torch.device("cuda:0")
orc, mt, pc, tiles = C.step_case("vit_tiny", 64, 32, 512)
eng = C.make_engine(orc, mt, pc, 512, 2, dev)
plans = [MaskPlan.from_masks(C.fixed_masks(4, 16, v), dev) for v in (0, 1, 0)]
out = []
for pl in plans:
    out.append(float(eng.step(tiles.to(dev), masks=pl)))
    out.append(float(eng.ibot))
    torch.cuda.synchronize()
    engine.repoison()
torch.cuda.synchronize()
out.append(float(eng.backbone_state_dict()["mask_token"].double().abs().sum()))
out.append(float(eng.patch_center.double().abs().sum()))
print("VALUES", " ".join(repr(v) for v in out))
"""


def test_poison_three_steps(dev):
    """GIPVIT_POISON=1 with engine.repoison() between steps: loss, ibot, mask_token and the patch centre stay finite over three steps
    and equal those of an unpoisoned run (atomics in the weight-gradient sums: 1e-4 relative after three optimizer steps)."""
    vals = {}
    for poison in ("1", ""):
        env = dict(os.environ)
        env.pop("GIPVIT_POISON", None)
        if poison:
            env["GIPVIT_POISON"] = "1"
        r = subprocess.run([sys.executable, "-c", POISON, ROOT], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        vals[poison] = [float(v) for v in r.stdout.split("VALUES", 1)[1].split()]
    assert all(math.isfinite(v) for v in vals["1"]), vals["1"]
    assert vals["1"][-2] > 0.0 and vals["1"][-1] > 0.0
    for a, b in zip(vals["1"], vals[""]):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (vals["1"], vals[""])


# -------------------------------------------------------------------------------------------------------------------- the driver
def test_driver_run_checkpoint_resume_and_feature_extractor(dev, tmp_path, caplog, capsys):
    """train.py --dino --ibot-weight 1 on synthetic tiles, ViT-T, three batches an epoch: the log line carries ``iBOT:``, the
    checkpoint holds mask_token (student and teacher) and ibot_center, a run resumed from epoch 0's file continues the mask stream
    (same final generator state, same patch centre and teacher as the uninterrupted run, at the gates of
    tests/test_train_gpu.py::test_train_dino_checkpoint_and_resume), and FeatureExtractor loads the student, saying that it drops
    mask_token."""
    sys.path.insert(0, ROOT)
    import train
    # (train.main makes a high-priority stream the current one and leaves it so: put the caller's back, or every later test of
    # the process runs its steps under another stream topology than it was written for)
    stream = torch.cuda.current_stream()
    try:
        _driver_run(dev, tmp_path, caplog, capsys, train)
    finally:
        torch.cuda.set_stream(stream)


def _driver_run(dev, tmp_path, caplog, capsys, train):
    base = ["--dino", "--ibot-weight", "1", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--out-dim", "512", "--global-crop-size", "64",
            "--local-crop-size", "32", "--local-crops-number", "2", "--batches-per-epoch", "3", "--lr", "1e-4", "--weight-decay", "0.04",
            "--clip-grad", "3.0", "--warmup-epochs", "1", "--log-interval", "1", "--output", str(tmp_path), "--seed", "7", "--ibot-mask-prob", "1.0"]
    with caplog.at_level("INFO"):
        assert train.main(base + ["--epochs", "2", "--experiment", "full"]) == 0
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Train:")]
    assert len(lines) == 6 and all("iBOT: " in l for l in lines)
    vals = [float(l.split("iBOT: ")[1].split()[0]) for l in lines]
    assert all(math.isfinite(v) and 1.0 < v < 2 * math.log(512) for v in vals), vals           # about ln K at the start
    ck0 = torch.load(tmp_path / "full" / "checkpoint-0.pth.tar", weights_only=True)
    ck1 = torch.load(tmp_path / "full" / "last.pth.tar", weights_only=True)
    for ck in (ck0, ck1):
        assert ck["state_dict"]["backbone.mask_token"].shape == (1, 192) and ck["state_dict_ema"]["backbone.mask_token"].shape == (1, 192)
        assert ck["ibot_center"].shape == (512,) and float(ck["ibot_center"].abs().max()) > 0 and "ibot" in ck["host_rng"]
    assert float(ck1["state_dict"]["backbone.mask_token"].abs().max()) > 0                      # it started at zeros and has learned
    assert train.main(base + ["--epochs", "2", "--experiment", "res", "--resume", str(tmp_path / "full" / "checkpoint-0.pth.tar")]) == 0
    r1 = torch.load(tmp_path / "res" / "last.pth.tar", weights_only=True)
    assert r1["host_rng"]["ibot"] == ck1["host_rng"]["ibot"] != ck0["host_rng"]["ibot"]
    rel = lambda a, b: float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
    for k in ("backbone.blocks.0.attn.qkv.weight", "backbone.mask_token", "head.mlp.2.weight"):
        assert rel(r1["state_dict_ema"][k], ck1["state_dict_ema"][k]) < 1e-5, k
        assert rel(r1["state_dict"][k], ck1["state_dict"][k]) < 2e-3, k
    assert rel(r1["ibot_center"], ck1["ibot_center"]) < 1e-3
    from gipvit.engine import FeatureExtractor
    capsys.readouterr()
    fx = FeatureExtractor(arch="vit_tiny", img_size=64, batch=2, device=dev)
    fx.load_state({k[len("backbone."):]: v for k, v in ck1["state_dict"].items() if k.startswith("backbone.")})
    assert "mask_token is dropped" in capsys.readouterr().out
    feats, _ = fx.run(C.vo.synth_tiles(2, 64, seed=3).to(dev))
    torch.cuda.synchronize()
    assert torch.isfinite(feats.float()).all()


# --------------------------------------------------------------------------------------------------------------------- two ranks
DP_K = 512


def _dp_masks():
    """Rank 0 marks 5 patches, rank 1 marks 9 (and leaves other images alone): [rank][G * 2, 16]."""
    m0, m1 = C.fixed_masks(4, 16, 0), C.fixed_masks(4, 16, 1)
    assert m0.sum() != m1.sum()
    return m0, m1


def _dp_engine(B, reducer=None):
    from gipvit.engine import DinoEngine
    from gipvit.models import init_vit_state, init_dino_head_state
    eng = DinoEngine(arch="vit_tiny", img_size=64, gsize=64, lsize=32, n_local=2, out_dim=DP_K, batch=B, lr=1e-4, weight_decay=0.04, device="cuda:0",
                     reducer=reducer, ibot_weight=1.0, ibot_mask_prob=1.0)
    bb = init_vit_state("vit_tiny", 64, 0, seed=0)
    bb["mask_token"] = 0.02 * torch.randn(1, 192, generator=torch.Generator().manual_seed(5))
    eng.load_state(bb, init_dino_head_state(192, DP_K, seed=1))
    eng.patch_center.copy_(0.05 * torch.randn(DP_K, generator=torch.Generator().manual_seed(6)))
    return eng


def _dp_worker(rank, world, port, q):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gipvit.dist import RcclReducer
    from gipvit.masking import MaskPlan
    eng = _dp_engine(2, RcclReducer())
    tiles = C.vo.synth_tiles(4, 256, seed=99)[2 * rank:2 * rank + 2].to("cuda:0")
    plan = MaskPlan.from_masks(_dp_masks()[rank], "cuda:0")
    eng.set_hyper()
    eng.forward_backward(tiles, masks=plan)
    torch.cuda.synchronize()
    scale = float(eng.hyper[5])
    g = {k: (v * scale).cpu().numpy() for k, v in eng.grads().items()}
    psum = eng.patch_center_sum.cpu().numpy()
    eng.optimizer_step()
    torch.cuda.synchronize()
    q.put((rank, g, psum, eng.patch_center.cpu().numpy(), float(eng.ibot), plan.M))
    dist.destroy_process_group()


def test_two_ranks_with_different_counts_match_one_process(dev):
    """Launched as tests/test_dp_gpu.py launches its ranks (gloo, both on this GPU; that file does not skip on one GPU, nor does
    this): two ranks x B = 2 with different M against one process with B = 4 on the concatenated tiles and masks -- the reduced
    gradient x grad_scale at that file's gate (2e-2: bf16 noise; a wrong weight or 1 / world is a factor), the all-reduced
    [K + 1] sums with the exact count, and the patch centre after the update at its centre gate (1e-3)."""
    import socket
    import torch.multiprocessing as mp
    from gipvit.masking import MaskPlan
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ps = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = sorted([q.get(timeout=300) for _ in ps], key=lambda t: t[0])
    [p.join(60) for p in ps]
    m0, m1 = _dp_masks()
    # one process, crop-major rows: global crop g of tiles 0..3 = rank 0's two, then rank 1's two
    full = np.concatenate([m0[0:2], m1[0:2], m0[2:4], m1[2:4]])
    one = _dp_engine(4)
    plan = MaskPlan.from_masks(full, dev)
    assert plan.M == res[0][5] + res[1][5] and res[0][5] != res[1][5]
    one.set_hyper()
    one.forward_backward(C.vo.synth_tiles(4, 256, seed=99).to(dev), masks=plan)
    torch.cuda.synchronize()
    g1 = one.grads()
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    for k in ("backbone.mask_token", "backbone.blocks.0.attn.qkv.weight", "backbone.blocks.11.mlp.fc2.weight", "backbone.patch_embed.proj.bias",
              "backbone.norm.weight", "head.mlp.0.weight", "head.last_layer.weight_v"):
        assert (res[0][1][k] == res[1][1][k]).all(), k                # both replicas hold the same reduced arena
        assert rel(torch.from_numpy(res[0][1][k]), g1[k].cpu()) < 2e-2, (k, rel(torch.from_numpy(res[0][1][k]), g1[k].cpu()))
    assert float(res[0][2][DP_K]) == float(plan.M) == float(res[1][2][DP_K])
    assert rel(torch.from_numpy(res[0][2]), one.patch_center_sum.cpu()) < 1e-2          # (bf16 head: the gate of the CLS centre sums)
    assert abs(0.5 * (res[0][4] + res[1][4]) - float(one.ibot)) < 1e-3
    one.optimizer_step()
    torch.cuda.synchronize()
    for r in res:
        assert rel(torch.from_numpy(r[3]), one.patch_center.cpu()) < 1e-3


def test_random_crops_views_koleo_drop_path_and_micro_batches_together(dev):
    """The term beside the options it must work with.  Boxes equal to the fixed windows reproduce the window path with the same plan
    (loss and ``ibot`` to 1e-5: identical crops, the DINO loss sum itself uses atomics); then sampled boxes with per-crop view
    augmentation, KoLeo, stochastic depth and two micro-batches with two plans in one step: everything finite, mask_token moves."""
    from gipvit.masking import MaskPlan
    from gipvit.multicrop import MultiCropSampler, ViewAugmentSampler
    arch, gsize, lsize, K = CASES[0]
    orc, mt, pc, tiles = C.step_case(arch, gsize, lsize, K)
    tiles = tiles.to(dev)
    plans = [MaskPlan.from_masks(C.fixed_masks(4, 16, v), dev) for v in (0, 1)]
    a, b = (C.make_engine(orc, mt, pc, K, 2, dev, koleo_weight=0.1) for _ in range(2))
    bg = torch.tensor([[i, y, x, gsize, gsize, 0] for (y, x) in a.gwins for i in range(2)], dtype=torch.int32, device=dev)
    bl = torch.tensor([[i, y, x, lsize, lsize, 0] for (y, x) in a.lwins for i in range(2)], dtype=torch.int32, device=dev)
    la, lb = float(a.step(tiles, masks=plans[0])), float(b.step(tiles, boxes=(bg, bl), masks=plans[0]))
    torch.cuda.synchronize()
    assert abs(la - lb) <= 1e-5 and abs(float(a.ibot) - float(b.ibot)) <= 1e-5 and float(a.ibot) > 0
    crops, views = MultiCropSampler(batch=2, tile=256, n_local=2, seed=11), ViewAugmentSampler(2, 2, 2, seed=12)
    b.set_drop_path(C.vo.drop_path_factors(12, 8, 0.3, torch.Generator().manual_seed(2)).to(dev))
    before = b.backbone_state_dict()["mask_token"].clone()
    for pl in plans:
        loss = float(b.step(tiles, boxes=crops.sample(dev), views=views.sample(dev), masks=pl))
        assert math.isfinite(loss) and math.isfinite(float(b.ibot)) and math.isfinite(float(b.koleo)) and float(b.ibot) > 0
    b.set_drop_path(None)
    loss = float(b.step_micro([tiles, tiles], masks=plans))
    torch.cuda.synchronize()
    assert math.isfinite(loss) and float(b.ibot) > 0 and torch.isfinite(b.patch_center).all()
    after = b.backbone_state_dict()["mask_token"]
    assert torch.isfinite(after).all() and not torch.equal(after, before)
