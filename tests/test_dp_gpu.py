"""GPU: the data-parallel path end to end with two ranks (gloo transport, both on the one GPU of
the test box): per-rank tile shards, ranged gradient all-reduce + centre all-reduce through
RcclReducer, 1/world folded into the optimizer.  Two ranks x B=2 must reproduce one process
with B=4 on the concatenated tiles (same mean loss, same update) up to bf16 / summation-order noise.

Three cases: ViT-T (also against the oracle), ViT-S -- the headline path: full-row fused kernels, the CLS-only last block,
the grouped dW launch, 1-MB buckets so that a step sends 13 ranges, scratch poisoned -- and ViT-T with two micro-batches of
B = 1 per rank (1 / (world x n_micro) in the optimizer and in the centre, collectives from the last micro-batch only)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 1024
NAMES = ("backbone.blocks.0.attn.qkv.weight", "backbone.blocks.11.mlp.fc2.weight", "backbone.pos_embed", "backbone.norm.weight",
         "head.mlp.0.weight", "head.last_layer.weight_v")


def _make(B, reducer=None, arch="vit_tiny"):
    from gipvit.engine import DinoEngine
    from gipvit.models import init_vit_state, init_dino_head_state
    eng = DinoEngine(arch=arch, img_size=224, out_dim=K, batch=B, lr=1e-4, weight_decay=0.04, clip_grad=3.0, device="cuda:0", reducer=reducer)
    eng.load_state(init_vit_state(arch, 224, 0, seed=0), init_dino_head_state(eng.D, K, seed=1))
    return eng


def _tiles():
    sys.path.insert(0, ROOT)
    from bench import synth_tiles
    return synth_tiles(4, 256, 99, "cpu")


def _worker(rank, world, port, q, arch="vit_tiny", B=2, n_micro=1, env=None, names=NAMES):
    """One rank: ``n_micro`` micro-batches of ``B`` tiles out of its shard of the four, ``env`` set before the engine is built."""
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), **(env or {}))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gipvit.dist import RcclReducer, shard_range
    eng = _make(B, RcclReducer(), arch)
    lo, hi = shard_range(4, rank, world)
    assert hi - lo == B * n_micro
    tiles = _tiles()[lo:hi].to("cuda:0")
    micro = [tiles[j * B:(j + 1) * B] for j in range(n_micro)]
    # gradient level first (before any optimizer step: Adam is scale-invariant and would hide a wrong 1/world):
    # the reduced arena x the grad_scale the optimizer kernel will apply = the mean gradient over all four tiles
    eng.set_hyper(n_micro=n_micro)
    for j, tb in enumerate(micro):
        eng.forward_backward(tb, micro=(j, n_micro))
    torch.cuda.synchronize()
    scale = float(eng.hyper[5])                      # GV_HYP_GRAD_SCALE, what gv_adamw_ema multiplies the arena by
    gr = eng.grads()
    gsel = {k: (gr[k] * scale).cpu().numpy() for k in names}
    gnorm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in gr.values()))) * scale
    eng.t = 0
    eng.arena.g.zero_()
    losses = [float(eng.step(tiles) if n_micro == 1 else eng.step_micro(micro)) for _ in range(2)]
    torch.cuda.synchronize()
    sd = eng.backbone_state_dict()
    # numpy payloads: pickled by value (torch tensors would travel as fds the exiting child closes)
    q.put((rank, losses, sd["blocks.0.attn.qkv.weight"].cpu().numpy(), sd["pos_embed"].cpu().numpy(),
           eng.head_state_dict()["last_layer.weight_v"][:64].cpu().numpy(), eng.center.cpu().numpy(), gsel, gnorm, scale))
    dist.destroy_process_group()


def _two_ranks(**kw):
    """Both ranks as ``spawn`` children on the one GPU -> their payloads by rank.  A rank that does not answer or does not end in
    time is terminated and the test fails: nothing is tried twice."""
    import queue
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:              # a port the kernel reports free (a pid-derived one collided now and then)
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q), kwargs=kw) for r in range(2)]
    [p.start() for p in ps]
    try:
        res = sorted([q.get(timeout=300) for _ in ps], key=lambda t: t[0])
        [p.join(60) for p in ps]
        assert not any(p.is_alive() for p in ps), "a rank did not end after it had answered"
        assert [p.exitcode for p in ps] == [0, 0], [p.exitcode for p in ps]
    except queue.Empty:
        pytest.fail(f"a rank did not answer within 300 s (exit codes {[p.exitcode for p in ps]})")
    finally:
        [p.terminate() for p in ps if p.is_alive()]
    return res


def _rel(x, y):
    return float((x.double() - y.double()).norm() / y.double().norm())


def test_two_ranks_match_single_process(dev):
    res = _two_ranks()
    # ---- gradient level: reduced gradient x grad_scale == single-process mean gradient == the oracle's
    gsel, gnorm, scale = res[0][6], res[0][7], res[0][8]
    assert scale == 0.5, scale                       # 1 / world
    for k in gsel:                                   # both replicas hold the same reduced arena
        assert (gsel[k] == res[1][6][k]).all(), k
    one = _make(4)
    one.set_hyper(); one.forward_backward(_tiles().to(dev)); torch.cuda.synchronize()
    g1 = one.grads()
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    for k, g in gsel.items():
        assert rel(torch.from_numpy(g), g1[k].cpu()) < 2e-2, (k, rel(torch.from_numpy(g), g1[k].cpu()))      # bf16 noise only; a wrong 1/world is a factor 2
    gn1 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g1.values())))
    assert abs(gnorm - gn1) / gn1 < 1e-2, (gnorm, gn1)
    from oracle import step_oracle as so
    orc = so.DinoOracle(arch="vit_tiny", img_size=224, out_dim=K, seed=0)
    orc.p.update(one.backbone_state_dict()); orc.hp.update({k: v.cpu() for k, v in one.head_state_dict().items()})
    orc.p = {k: v.cpu() for k, v in orc.p.items()}
    _, g_or, _, _, _ = orc.forward_backward(_tiles())
    for k, g in gsel.items():
        assert rel(torch.from_numpy(g), g_or[k]) < 5e-2, (k, rel(torch.from_numpy(g), g_or[k]))
    gno = so.grad_norm({k: v for k, v in g_or.items() if k != "head.last_layer.weight_g"})
    assert abs(gnorm - gno) / gno < 1e-2, (gnorm, gno)
    # replicas stay identical (same reduced gradients, same update)
    res = [(r[0], r[1]) + tuple(torch.from_numpy(x) for x in r[2:6]) for r in res]
    for a, b in zip(res[0][2:], res[1][2:]):
        assert torch.equal(a, b)
    # and equal to one process on all four tiles
    ref = _make(4)
    tiles = _tiles().to(dev)
    ref_losses = [float(ref.step(tiles)) for _ in range(2)]
    torch.cuda.synchronize()
    mean_losses = [(res[0][1][i] + res[1][1][i]) / 2 for i in range(2)]
    assert abs(mean_losses[0] - ref_losses[0]) < 1e-4, (mean_losses, ref_losses)      # same weights: only the batch split differs
    assert abs(mean_losses[1] - ref_losses[1]) < 5e-3, (mean_losses, ref_losses)      # after one (Adam) update
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    sd = ref.backbone_state_dict()
    assert rel(res[0][2], sd["blocks.0.attn.qkv.weight"].cpu()) < 5e-3
    assert rel(res[0][5], ref.center.cpu()) < 1e-3


def _check_against_one_process(dev, res, arch, ref_step, names, tag, centre_gate=1e-3):
    """The gates of test_two_ranks_match_single_process (measured values of this project) on the payloads ``res`` of two ranks
    against one process with B = 4 on the same four tiles; every figure is printed before it is held to its gate."""
    gsel, gnorm = res[0][6], res[0][7]
    for k in gsel:                                   # both replicas hold the same reduced arena
        assert (gsel[k] == res[1][6][k]).all(), k
    one = _make(4, arch=arch)
    one.set_hyper(); one.forward_backward(_tiles().to(dev)); torch.cuda.synchronize()
    g1 = one.grads()
    rels = {k: _rel(torch.from_numpy(gsel[k]), g1[k].cpu()) for k in names}
    gn1 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g1.values())))
    print(f"{tag}: gradient rel " + " ".join(f"{k.split('.', 1)[1]}={v:.2e}" for k, v in rels.items()) + f"; norm {gnorm:.6g} vs {gn1:.6g} ({abs(gnorm - gn1) / gn1:.2e})")
    for k, v in rels.items():
        assert v < 2e-2, (k, v)                      # bf16 noise only; a wrong 1 / (world x n_micro) is a factor 2
    assert abs(gnorm - gn1) / gn1 < 1e-2, (gnorm, gn1)
    # replicas stay identical (same reduced gradients, same update)
    out = [tuple(torch.from_numpy(x) for x in r[2:6]) for r in res]
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)
    # and equal to one process on all four tiles: the loss is the mean over the ranks
    ref = _make(4, arch=arch)
    tiles = _tiles().to(dev)
    ref_losses = [float(ref_step(ref, tiles)) for _ in range(2)]
    torch.cuda.synchronize()
    mean_losses = [(res[0][1][i] + res[1][1][i]) / 2 for i in range(2)]
    w_rel = _rel(out[0][0], ref.backbone_state_dict()["blocks.0.attn.qkv.weight"].cpu())
    c_rel = _rel(out[0][3], ref.center.cpu())
    print(f"{tag}: losses {mean_losses} vs {ref_losses}; weight rel {w_rel:.2e}; centre rel {c_rel:.2e}")
    assert all(map(lambda v: v == v and abs(v) < 1e4, mean_losses)), mean_losses            # (poisoned scratch that was read shows here)
    assert abs(mean_losses[0] - ref_losses[0]) < 1e-4, (mean_losses, ref_losses)      # same weights: only the batch split differs
    assert abs(mean_losses[1] - ref_losses[1]) < 5e-3, (mean_losses, ref_losses)      # after one (Adam) update
    assert w_rel < 5e-3
    assert c_rel < centre_gate, (c_rel, centre_gate)


def test_two_ranks_vit_small_match_single_process(dev):
    """ViT-S, 2 ranks x B = 2, default switches: the path a production run takes and no second rank had ever run -- full-row
    fused kernels, the CLS-only last block (``blocks.11.attn.proj.weight`` comes from its tail), the grouped dW launch -- with
    1-MB buckets (13 ranges a step instead of 5) and poisoned scratch in the workers.  Gates: those of the ViT-T test, but for
    the centre after two updates.  Measured on the reference side -- one process, the same four tiles as ``step`` (B = 4) and as
    ``step_micro`` of 2 x 2, a pure summation-order change -- that centre differs by 1.28e-3 relative at ViT-S (ViT-T: 3.8e-8;
    the ViT-S weight gradients of the two differ by 9e-5 where ViT-T's differ by 1e-7, and Adam's first update turns that into
    weights 4.6e-5 apart, which the second step's teacher logits carry into the centre).  The ViT-T gate of 1e-3 is below that
    floor, so the ViT-S centre gate is 4 x the floor, 5.1e-3: a wrong 1 / world in the centre is a factor 2, two orders of
    magnitude outside.  (Two ranks measured 1.31e-3.)  Every other figure sits inside the ViT-T gates: gradients 9e-5 (gate
    2e-2), norm 2e-6 (1e-2), losses 0 and 2.9e-4 (1e-4, 5e-3), weights 4.7e-5 (5e-3)."""
    names = NAMES + ("backbone.blocks.11.attn.proj.weight",)
    res = _two_ranks(arch="vit_small", env={"GIPVIT_BUCKET_MB": "1", "GIPVIT_POISON": "1"}, names=names)
    assert res[0][8] == 0.5 and res[1][8] == 0.5                       # 1 / world
    _check_against_one_process(dev, res, "vit_small", lambda eng, t: eng.step(t), names, "vit_small 2 x 2", centre_gate=5.1e-3)


def test_two_ranks_with_accumulation_match_single_process(dev):
    """ViT-T, 2 ranks x 2 micro-batches of B = 1 against one process ``step`` with B = 4 on the same four tiles in the same
    order (rank r, micro-batch j: tile 2 r + j): GRAD_SCALE is exactly 1 / (world x n_micro) = 0.25, the centre's
    1 / (G B world n_micro), collectives from the last micro-batch only -- together, as a run with --grad-accum on two GPUs
    has them.  Gates: those of the ViT-T test (the centre after the update at its centre gate)."""
    res = _two_ranks(B=1, n_micro=2)
    assert res[0][8] == 0.25 and res[1][8] == 0.25, (res[0][8], res[1][8])
    _check_against_one_process(dev, res, "vit_tiny", lambda eng, t: eng.step(t), NAMES, "vit_tiny 2 x (2 x 1)")
