"""GPU, one process: what the data-parallel step puts on the wire is the final gradient.

A snapshot reducer (world 1, ``always = True``, so the engine releases its ranges as a data-parallel run does) clones
``buf[lo:hi]`` inside ``reduce_range``.  The clone is queued on the stream the release is issued on -- exactly what a collective
waits for -- so it sees the range as the all-reduce would.  After the step: the ranges tile the arena once in plan order, every
snapshot is bitwise the final ``g[lo:hi]`` (nothing writes a range behind its release, nothing the release should have waited
for is missing), and the gradient is the one an engine without a reducer computes from the same input.

ViT-S (the headline path: full-row fused kernels, the CLS-only last block, the grouped dW launch, 1-MB buckets so a step
releases 13 ranges) at batch 1; ViT-T for the fp32 path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
K = 1024


class SnapshotReducer:
    world, rank, always = 1, 0, True

    def __init__(self):
        self.snaps, self.calls = [], []

    def reduce_range(self, buf, lo, hi):
        self.calls.append("range")
        self.snaps.append((lo, hi, buf[lo:hi].clone()))

    def reduce_tensor(self, t):
        self.calls.append("tensor")

    def reduce_max(self, t):
        self.calls.append("max")

    def finish(self):
        self.calls.append("finish")


def _engine(arch, reducer, **kw):
    from gipvit.engine import DinoEngine
    from gipvit.models import init_dino_head_state, init_vit_state
    eng = DinoEngine(arch=arch, img_size=224, out_dim=K, batch=1, lr=1e-4, weight_decay=0.04, device="cuda:0", reducer=reducer, **kw)
    D = eng.D
    bb = init_vit_state(arch, 224, 0, seed=0)
    eng.load_state(bb, init_dino_head_state(D, K, seed=1))
    return eng


def _tiles(n, dev):
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (n, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)


def _masks(eng, dev):
    from gipvit.masking import MaskPlan
    m = np.zeros((eng.G * eng.B, (eng.gsize // 16) ** 2), np.bool_)
    m[0, 5:42] = True
    m[1, 100:113] = True
    return MaskPlan(m, dev)


def _run(eng, tiles, n_micro, masks):
    """One step's forward_backward calls -> the scaled gradient (arena x GRAD_SCALE), after a device synchronize."""
    from gipvit import _lib as L
    eng.set_hyper(n_micro=n_micro)
    for j in range(n_micro):
        kw = {} if masks is None else dict(masks=masks)
        eng.forward_backward(tiles[j:j + 1], micro=(j, n_micro), **kw)
        if j == 0 and n_micro > 1 and isinstance(eng.reducer, SnapshotReducer):
            torch.cuda.synchronize()
            assert eng.reducer.calls == [], eng.reducer.calls          # nothing goes out before the last micro-batch
    torch.cuda.synchronize()
    return eng.arena.g * float(eng.hyper[L.HYP_GRAD_SCALE])


CASES = {
    "vit_s": ("vit_small", {}, {}, 1, False),
    "vit_s_ungrouped": ("vit_small", {"GIPVIT_GROUP_DW": "0"}, {}, 1, False),
    "vit_s_every_token": ("vit_small", {"GIPVIT_CLS_ONLY_LAST": "0"}, {}, 1, False),
    "vit_s_micro2": ("vit_small", {}, {}, 2, False),
    "vit_s_ibot": ("vit_small", {}, {"ibot_weight": 1.0}, 1, True),
    "vit_t_fp32": ("vit_tiny", {}, {"precision": "fp32"}, 1, False),
}


@pytest.mark.parametrize("cid", list(CASES))
def test_released_ranges_are_the_final_gradient(dev, monkeypatch, cid):
    arch, env, kw, n_micro, ibot = CASES[cid]
    monkeypatch.setenv("GIPVIT_BUCKET_MB", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tiles = _tiles(n_micro, dev)
    # the engine without a reducer on the same input: is it deterministic run to run?  Four runs of one engine and two of a
    # second, fresh one (what the engine with the reducer is): split-K sums go through float atomics, and in the fp32 mode a
    # pair of runs differs by 6e-9 or by 3e-7 as it happens (measured: 6.4e-09, 2.9e-07, 3.0e-07 against the first run, 2.9e-07
    # for a fresh engine), so two runs alone do not show the spread
    plain = _engine(arch, None, **kw)
    masks = _masks(plain, dev) if ibot else None
    assert masks is None or masks.M == 50
    runs = [_run(plain, tiles, n_micro, masks).clone() for _ in range(4)]
    fresh = _engine(arch, None, **kw)
    runs += [_run(fresh, tiles, n_micro, masks).clone() for _ in range(2)]
    g0 = runs[0]
    assert torch.isfinite(g0).all() and float(g0.abs().max()) > 0
    deterministic = all(torch.equal(g0, x) for x in runs[1:])
    spread = max(float((g0.double() - x.double()).norm() / g0.double().norm()) for x in runs[1:])
    print(f"{cid}: no-reducer engine run to run: {'bitwise equal' if deterministic else f'relative spread {spread:.3e}'}")
    del fresh, runs

    red = SnapshotReducer()
    eng = _engine(arch, red, **kw)
    assert torch.equal(eng.arena.p, plain.arena.p)
    g = _run(eng, tiles, n_micro, masks)
    a = eng.arena
    # the ranges tile [0, a.n) once, in plan order, and with 1-MB buckets there are many
    plan = eng._reduction_plan()
    assert [(lo, hi) for lo, hi, _ in red.snaps] == [(lo, hi) for _, lo, hi in plan]
    assert len(plan) == 13 and plan[0][1] == 0 and plan[-1][2] == a.n
    assert all(plan[i][2] == plan[i + 1][1] for i in range(len(plan) - 1))
    assert red.calls[-1] == "finish" and red.calls.count("range") == 13 and red.calls.count("tensor") == 1 + ibot
    # every snapshot is bitwise the final gradient of its range (under accumulation: the accumulated one)
    for (lo, hi, snap), (trg, _, _) in zip(red.snaps, plan):
        if not torch.equal(snap, a.g[lo:hi]):
            d = (snap != a.g[lo:hi]).nonzero()
            raise AssertionError(f"range {trg} [{lo}, {hi}): {d.numel()} elements changed behind the release, the first at {lo + int(d[0])}")
    # ... and the engine computed what the engine without a reducer computes
    if deterministic:
        assert torch.equal(g, g0), float((g.double() - g0.double()).norm() / g0.double().norm())
    else:
        got = float((g.double() - g0.double()).norm() / g0.double().norm())
        print(f"{cid}: with the snapshot reducer against the no-reducer engine: {got:.3e}")
        # the same noise drawn once more: its distance from the first run is distributed like the five distances `spread` is the
        # largest of (measured: 4.8e-09 against 4.7e-09 on ViT-S, 3.1e-07 against 3.0e-07 in the fp32 mode).  4 x is room for the
        # draw's luck; a range that is missing, doubled or written behind its release is off by 1e-2 and more
        assert got <= 4 * spread, (got, spread)
