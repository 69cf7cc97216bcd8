"""GPU: gv_attention_bwd_stream (the streaming attention backward, N <= 1040 tokens) on the exact probes of
tests/test_attention_probes_host.py at every streaming length, under q_limit, on replicated pairs and on the cases whose lse reaches
63; then the opt-in end to end: SupervisedEngine / DinoEngine(long_seq=True) and train.py --train-long-seq on tiles above 256 px
against the CPU oracle.  tests/test_attention_stream_bwd_host.py shows on the CPU that the assertion functions used here reject a
backward that loses a key or a query row at a block seam, takes delta from a wrong row or adds a block twice.  Every output and the
delta scratch sit in buffers with a sentinel-filled guard region behind them that must stay untouched."""
import csv
import math
import os
import subprocess
import sys

import pytest
import torch

from test_attention_probes_host import H, N_IMG, SCALE, build, check_random, closed_form, pack_qkv, pack_rows, unpack_dqkv, unpack_rows
from test_attention_probes_gpu import _all_pairs_equal_pair0, _guarded, _guards_untouched, _replicated
from test_attention_stream_host import B_NS, SHORT_NS, STREAM_NS, STREAM_QBLOCK, build_spike, build_staircase
from test_attention_stream_bwd_host import BWD_PARTS, bwd_check, step_targets

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = N_IMG * H


def _qe(N, q_limit):
    return min(N, (q_limit + STREAM_QBLOCK - 1) // STREAM_QBLOCK * STREAM_QBLOCK) if q_limit else N


def run_bwd(dev, case, n_img=N_IMG, H=H, q_limit=0, d_o=None, poison_tail=False):
    """gv_attention_fwd_stream, then gv_attention_bwd_stream on its own o / lse, all outputs and delta in guarded buffers ->
    dq, dk, dv [P, N, 64] (fp64, CPU) and the raw dqkv.  ``poison_tail``: the full forward runs, then everything the limited backward
    must not read -- rows >= qe of o, lse and d_o -- is overwritten with NaN."""
    from gipvit import ops
    N = case["N"]
    qkv = pack_qkv(case, n_img, H, bf16).to(dev)
    d_o = pack_rows(case["d_o"] if d_o is None else d_o, n_img, H, bf16).to(dev)
    obuf, out = _guarded(n_img * N, H * 64, bf16, dev)
    lbuf, lse = _guarded(n_img * H, N, f32, dev)
    gbuf, dqkv = _guarded(n_img * N, 3 * H * 64, bf16, dev)
    dbuf, delta = _guarded(n_img * H, N, f32, dev)
    lse = lse.view(n_img, H, N)
    ops.attention_fwd_stream(qkv, n_img, N, H, SCALE, o=out, lse=lse)
    qe = _qe(N, q_limit)
    if poison_tail and qe < N:
        out.view(n_img, N, H * 64)[:, qe:] = float("nan")
        d_o.view(n_img, N, H * 64)[:, qe:] = float("nan")
        lse[:, :, qe:] = float("nan")
    ops.attention_bwd_stream(qkv, out, d_o, lse, n_img, N, H, SCALE, dqkv=dqkv, delta=delta.view(-1), q_limit=q_limit)
    _guards_untouched((obuf, out), (lbuf, lse), (gbuf, dqkv), (dbuf, delta))
    dq, dk, dv = unpack_dqkv(dqkv, n_img, H)
    return dict(dq=dq, dk=dk, dv=dv, dqkv_raw=dqkv.clone())


def _probe(dev, probe, N):
    case = build(probe, N)
    got = run_bwd(dev, case)
    if probe == "D":
        print(f"stream bwd probe D N={N}: " + "  ".join(f"max |{n} err| {float((got[n] - case[n]).abs().max()):.3e}" for n in BWD_PARTS["D"]))
    bwd_check(probe)(got, case)


@pytest.mark.parametrize("probe,N", [(p, N) for p in "ACD" for N in STREAM_NS] + [("B", N) for N in B_NS])
def test_probe(dev, probe, N):
    """Probes A (selector: dV bit exact, dQ = dK ~ 0), B (two-key tie: exact nonzero dQ / dK), C (Q = 0: dK exactly zero) and D
    (randn: check_random's gradient bounds) at every streaming length, 9 pairs, on the streaming forward's own o / lse."""
    _probe(dev, probe, N)


@pytest.mark.parametrize("N", SHORT_NS)
@pytest.mark.parametrize("probe", "ABCD")
def test_probe_below_the_old_limit(dev, probe, N):
    """One key block, one partial query block, a single token: the lengths gv_attention_bwd serves too."""
    _probe(dev, probe, N)


@pytest.mark.parametrize("ql,N", [(1, 289), (33, 289), (1, 1025), (129, 1025)])
def test_q_limit(dev, ql, N):
    """Probe D under q_limit: d_o zero in [q_limit, qe), NaN behind qe in o, lse and d_o (nothing there may be read).  The result
    equals, bit for bit, the unlimited call on the same data with d_o zeroed behind q_limit; dQ rows >= qe are exactly zero."""
    case = build("D", N)
    qe = _qe(N, ql)
    assert qe == (2 if ql == 129 else 1) * STREAM_QBLOCK < N
    d_o = case["d_o"].clone()
    d_o[:, ql:] = 0
    got = run_bwd(dev, case, q_limit=ql, d_o=d_o, poison_tail=True)
    full = run_bwd(dev, case, d_o=d_o)
    assert bool(torch.isfinite(got["dqkv_raw"].float()).all()), "the limited backward read a row behind qe"
    assert torch.equal(got["dqkv_raw"], full["dqkv_raw"]), "gradients differ from the unlimited call on the zero-tailed dO"
    assert bool((got["dq"][:, qe:] == 0).all()) and bool((got["dq"][:, :ql] != 0).any())
    # ... and that result is the gradient of the zero-tailed dO
    s = case["q"] @ case["k"].transpose(-1, -2) * SCALE
    _, dq, dk, dv = closed_form(case["q"], case["k"], case["v"], d_o, s.softmax(-1), SCALE)
    check_random(got, dict(case, dq=dq, dk=dk, dv=dv), parts=("dq", "dk", "dv"))


@pytest.mark.parametrize("N", [289, 1025])
def test_replicated_pairs_and_a_second_call_are_bit_equal(dev, N):
    """One pair of probe D in every pair of the launch (513 / 171 pairs, both odd): dq / dk / dv of every pair equal pair 0 bit for
    bit -- a wave reading a stale stage, a missing barrier or another pair's delta shows as a difference -- and a second call on the
    same buffers gives the same bits.  Pair 0 itself is held to probe D's bounds."""
    from gipvit import ops
    n_img, Hh = (171, 3) if N == 289 else (57, 3)
    case1 = build("D", N, 1)
    qkv, d_o = _replicated(dev, case1, n_img, Hh)
    qkv, d_o = qkv.contiguous(), d_o.contiguous()
    T = n_img * N
    obuf, out = _guarded(T, Hh * 64, bf16, dev)
    gbuf, dqkv = _guarded(T, 3 * Hh * 64, bf16, dev)
    lbuf, lse = _guarded(n_img * Hh, N, f32, dev)
    dbuf, delta = _guarded(n_img * Hh, N, f32, dev)
    lse = lse.view(n_img, Hh, N)
    ops.attention_fwd_stream(qkv, n_img, N, Hh, SCALE, o=out, lse=lse)
    ops.attention_bwd_stream(qkv, out, d_o, lse, n_img, N, Hh, SCALE, dqkv=dqkv, delta=delta.view(-1))
    first, first_delta = dqkv.clone(), delta.clone()
    ops.attention_bwd_stream(qkv, out, d_o, lse, n_img, N, Hh, SCALE, dqkv=dqkv, delta=delta.view(-1))
    _guards_untouched((obuf, out), (gbuf, dqkv), (lbuf, lse), (dbuf, delta))
    assert torch.equal(first, dqkv) and torch.equal(first_delta, delta), "a second call on the same buffers gave other bits"
    _all_pairs_equal_pair0(f"N={N} dqkv", dqkv, n_img, Hh)
    _all_pairs_equal_pair0(f"N={N} delta", delta.view(n_img, Hh, N), n_img, Hh, lse=True)
    dq, dk, dv = unpack_dqkv(dqkv[:N].reshape(N, 3, Hh, 64)[:, :, 0].reshape(N, 192), 1, 1)
    check_random(dict(dq=dq, dk=dk, dv=dv), case1, parts=("dq", "dk", "dv"))


_GRAD_CASES = {}


def _with_gradients(kind, N):
    """a spike / staircase case of the streaming host file with d_o (randn, bf16-rounded, drawn per pair from the builder's seed
    behind the builder's own draws) and the fp64 closed-form gradients -- built once, read only"""
    if (kind, N) not in _GRAD_CASES:
        name, arg = kind.split("-")
        if name == "spike":
            case, base, extra = build_spike(N, arg), 7000 + ("first", "middle", "last").index(arg), 0
        else:
            case, base, extra = build_staircase(N, arg == "up"), 7100 + int(arg == "up"), 64
        d_o = []
        for pair in range(P):
            g = torch.Generator().manual_seed(base * 100000 + N * 10 + pair)
            torch.randn(3 * N * 64 + extra, generator=g)                    # q, k, v (and the staircase's direction)
            d_o.append(torch.randn(N, 64, generator=g).to(bf16).to(f64))
        d_o = torch.stack(d_o)
        s = case["q"] @ case["k"].transpose(-1, -2) * SCALE
        _, dq, dk, dv = closed_form(case["q"], case["k"], case["v"], d_o, s.softmax(-1), SCALE)
        _GRAD_CASES[(kind, N)] = dict(case, d_o=d_o, dq=dq, dk=dk, dv=dv)
    return _GRAD_CASES[(kind, N)]


@pytest.mark.parametrize("N", [321, 1025])
@pytest.mark.parametrize("kind", ["spike-first", "spike-middle", "spike-last", "staircase-up", "staircase-down"])
def test_forced_rescale(dev, kind, N):
    """The cases that make the forward's online softmax rescale: the backward has no running max, but lse reaches 63 there and P
    is recomputed from it.  Gradients against the closed form on the fp64 softmax at check_random's gradient bounds."""
    case = _with_gradients(kind, N)
    got = run_bwd(dev, case)
    print(f"{kind} N={N}: max lse {float(case['lse'].max()):.1f}  " + "  ".join(f"max |{n} err| {float((got[n] - case[n]).abs().max()):.3e}" for n in ("dq", "dk", "dv")))
    check_random(got, case, parts=("dq", "dk", "dv"))


# ------------------------------------------------------------------------------------------------------------ end to end
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _grad_errors(got, ref, skip=()):
    """-> (per-parameter ||g - ref|| / ||ref||, worst first, as (error, name); relative error of the global gradient norm)"""
    worst, gn_g, gn_r = [], 0.0, 0.0
    for k, r in ref.items():
        if r is None or k in skip:
            continue
        g = got[k]
        gn_g += float((g.double() ** 2).sum()); gn_r += float((r.double() ** 2).sum())
        if float(r.abs().max()) < 1e-12:
            continue
        worst.append((_rel(g, r), k))
    worst.sort(reverse=True)
    return worst, abs(math.sqrt(gn_g) - math.sqrt(gn_r)) / math.sqrt(gn_r)


def _check_grads(worst, rel_norm, tol=5e-2):
    """the gate of tests/test_engine_gpu.py: per-parameter ||g - ref|| / ||ref|| <= 5e-2, gradient norm within 1e-2"""
    assert worst[0][0] <= tol, f"gradient mismatch: {[(round(e, 4), k) for e, k in worst[:8]]}"
    assert rel_norm <= 1e-2, f"grad-norm rel err {rel_norm}"


@pytest.mark.parametrize("arch,img,pool", [("vit_tiny", 272, "token"), ("vit_small", 272, "token"), ("vit_tiny", 512, "token"), ("vit_tiny", 272, "avg")])
def test_supervised_step_parity_above_256_px(dev, arch, img, pool):
    """SupervisedEngine(long_seq=True) against the CPU oracle at the gates of tests/test_engine_gpu.py (logits 2e-2 max |ref|, loss
    1e-3, per-parameter gradient 5e-2, gradient norm 1e-2): 290 tokens (ViT-S: the fused path), 1 025 tokens, and the mean-pooled
    model, whose last block differentiates every token (no q_limit; its reference is tests/test_global_pool_host.py's).  At 272 px
    the CLS-only tail (q_limit = 1 in the last block) agrees with every token of every block at the gate of
    test_cls_only_last_block_equals_every_token.

    Both images carry one label (step_targets): tests/test_attention_stream_bwd_host.py shows on the oracle alone that with two
    opposite labels on these synthetic tiles the batch gradient is a 10- to 43-fold cancellation of the per-image gradients, so
    that one bf16 rounding of a per-image term is 5 - 10 % of it (measured with labels (1, 0): worst 8.1e-2 at 272 px, 6.5e-2 at 512
    px, 9.7e-2 on fc_norm.bias -- an fp64 attention backward of the very bf16 inputs the kernel read is off by the same amount).
    Measured on an MI355X with one label: worst per-parameter error 8.5e-3 (vit_tiny 272), 7.7e-3 (vit_small 272), 8.1e-3 (vit_tiny
    512), 5.6e-3 (avg); CLS-only tail vs every token 6.0e-8 (vit_tiny) and 4.946e-3 (vit_small; the same to 1e-7 over six runs, and
    4.938e-3 on the 256-px step through gv_attention_bwd)."""
    from gipvit.engine import SupervisedEngine
    from oracle import step_oracle as so, vit_oracle as vo
    B = 2
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    tiles = vo.synth_tiles(B, img, seed=1234)
    tgt = step_targets(B)
    if pool == "avg":
        import test_global_pool_host as GP
        p = GP.avg_params(arch, img, 2, seed=0)
        loss_r, grads_r, logits_r = GP.avg_forward_backward(p, tiles, tgt, arch, img)
    else:
        orc = so.SupervisedOracle(arch=arch, img_size=img, num_classes=2, seed=0, lr=1e-3, wd=0.05)
        p = orc.p
        loss_r, grads_r, logits_r = orc.forward_backward(tiles, tgt)

    def engine_run(cls_last):
        eng = SupervisedEngine(arch=arch, img_size=img, num_classes=2, batch=B, lr=1e-3, weight_decay=0.05, device=dev, global_pool=pool, long_seq=True)
        eng.vit.cls_last = cls_last
        eng.load_state(p)
        eng.forward_backward(tiles.to(dev), tgt.to(dev))
        torch.cuda.synchronize()
        assert eng.vit._cls_tail(eng.grp) == (cls_last and pool != "avg") and eng.grp.delta.numel() == B * eng.vit.H * ((img // 16) ** 2 + 1)
        return float(eng.loss), eng.logits.float().cpu().clone(), {n: g.clone() for n, g in eng.grads().items()}

    loss, logits, grads = engine_run(True)
    dlog, dl = float((logits.double() - logits_r.double()).abs().max()), abs(loss - float(loss_r))
    worst, gn = _grad_errors(grads, grads_r)
    print(f"[long_seq step {arch} {img} px {pool}] logits err {dlog:.2e} (max |ref| {float(logits_r.abs().max()):.3f})  |dloss| {dl:.2e}  "
          f"grad-norm rel {gn:.2e}  worst grads {[(round(e, 4), k) for e, k in worst[:4]]}")
    assert dlog <= 2e-2 * max(float(logits_r.abs().max()), 1.0), (dlog, float(logits_r.abs().max()))
    assert dl <= 1e-3, (loss, float(loss_r))
    if img == 272 and pool == "token":
        loss0, logits0, grads0 = engine_run(False)
        assert abs(loss - loss0) <= 2e-5, (loss, loss0)
        assert float((logits - logits0).abs().max()) <= 2e-3 * float(logits0.abs().max())
        worst = ("", 0.0)
        for n in grads0:
            a, b = grads[n].double(), grads0[n].double()
            if float(b.norm()) == 0.0:
                assert float(a.norm()) == 0.0, n
                continue
            rel = float((a - b).norm() / b.norm())
            worst = (n, rel) if rel > worst[1] else worst
        print(f"[long_seq step {arch} {img} px] CLS-only tail vs every token: worst grad {worst[1]:.2e} ({worst[0]})")
        assert worst[1] <= 5e-3, worst
    _check_grads(*_grad_errors(grads, grads_r))


def test_dino_step_parity_with_a_streamed_global_segment(dev):
    """DinoEngine(long_seq=True), 2 x 272-px global crops (290 tokens: streamed) + 2 x 96-px local crops (37 tokens: gv_attention_fwd /
    _bwd) of 288-px tiles, against DinoOracle with the same sizes at the gates of test_dino_step_parity."""
    from gipvit.engine import DinoEngine
    from oracle import step_oracle as so, vit_oracle as vo
    K, B = 4096, 2
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    sizes = dict(img_size=272, gsize=272, lsize=96, n_local=2)
    orc = so.DinoOracle(arch="vit_tiny", out_dim=K, seed=0, lr=5e-4, wd=0.04, **sizes)
    eng = DinoEngine(arch="vit_tiny", out_dim=K, batch=B, tile=288, lr=5e-4, weight_decay=0.04, device=dev, long_seq=True, **sizes)
    eng.load_state(orc.p, orc.hp)
    c = 0.05 * torch.randn(1, K, generator=torch.Generator().manual_seed(3))
    orc.center = c.clone(); eng.center.copy_(c[0])
    tiles = vo.synth_tiles(2, 288)
    loss_r, grads_r, s_out, t_out, bsum = orc.forward_backward(tiles)
    eng.set_hyper()
    eng.forward_backward(tiles.to(dev))
    torch.cuda.synchronize()
    assert [sg.N for sg in eng.g_stu.segs] == [290, 37]
    worst, gn = _grad_errors(eng.grads(), grads_r, skip=("head.last_layer.weight_g",))
    print(f"[long_seq dino] |dloss| {abs(float(eng.loss) - float(loss_r)):.2e}  grad-norm rel {gn:.2e}  worst grads {[(round(e, 4), k) for e, k in worst[:4]]}")
    for got, ref, nm in ((eng.hb_t.logits, t_out, "teacher"), (eng.hb_s.logits, s_out, "student")):
        err = float((got.cpu() - ref).abs().max())
        assert err <= 2e-2 * float(ref.abs().max()), (nm, err, float(ref.abs().max()))
    assert abs(float(eng.loss) - float(loss_r)) <= 1e-3, (float(eng.loss), float(loss_r))
    assert _rel(eng.center_sum, bsum[0]) < 1e-2
    _check_grads(worst, gn)


def test_poisoned_step_reads_only_what_it_wrote(dev, monkeypatch):
    """One 272-px supervised step with every scratch buffer NaN when it starts (GIPVIT_POISON=1 + repoison, as
    tests/test_poison_gpu.py): the limited last-block forward leaves o / lse rows behind the first query block NaN, and the backward
    must not read them -- loss and every gradient stay finite."""
    import gc
    from gipvit import engine
    from oracle import vit_oracle as vo
    monkeypatch.setenv("GIPVIT_POISON", "1")
    eng = None
    try:
        eng = engine.SupervisedEngine(arch="vit_tiny", img_size=272, num_classes=2, batch=2, device=dev, long_seq=True)
        eng.load_state(vo.init_vit("vit_tiny", 272, 2, seed=0))
        tiles = vo.synth_tiles(2, 272, seed=7).to(dev)
        tgt = torch.zeros(2, 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        assert engine.repoison() > 0
        assert eng.vit._cls_tail(eng.grp) and bool(torch.isnan(eng.grp.delta).all())
        eng.forward_backward(tiles, tgt)
        torch.cuda.synchronize()
        assert math.isfinite(float(eng.loss))
        bad = [n for n, g in eng.grads().items() if not bool(torch.isfinite(g).all())]
        assert not bad, bad
    finally:
        del eng
        gc.collect()


def test_train_py_trains_at_272_px_with_the_flag_only(dev, tmp_path):
    import train
    args = ["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "--num-classes", "2", "--img-size", "272", "--tile-size", "272", "-b", "2",
            "--batches-per-epoch", "2", "--epochs", "1", "--lr", "1e-4", "--output", str(tmp_path), "--experiment", "long", "--synthetic-slides", "2",
            "--num_tiles", "4", "--tiles_per_iter", "2", "--seed", "1"]
    assert train.main(args + ["--train-long-seq"]) == 0
    row = list(csv.DictReader(open(tmp_path / "long" / "summary.csv")))[0]
    assert math.isfinite(float(row["train_loss"])) and 0.1 < float(row["train_loss"]) < 2.0, row
    with pytest.raises(SystemExit, match="288 tokens"):
        train.main(args)


def test_float16_build(dev):
    """tests/attention_stream_bwd_f16_worker.py in a process of its own (GIPVIT_ACT_FORMAT=f16): probes A and D at N = 289 and 1 025."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attention_stream_bwd_f16_worker.py")], cwd=ROOT,
                       env=dict(os.environ, GIPVIT_ACT_FORMAT="f16"), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("STREAM BWD F16 OK"), (r.stdout[-2000:], r.stderr[-3000:])
