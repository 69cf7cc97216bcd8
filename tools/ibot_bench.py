"""What the iBOT masked-patch term costs at the headline shape (ViT-S, B = 64 tiles, 2 x 224 + 8 x 96 crops, K = 65 536), by
device events on one MI355X:

  (a) the DINO step as it is (ibot_weight 0: the launches of the parent commit)
  (b) the term on with plans that mark nothing: the all-token last block of both groups, and nothing else
  (c) the term on with sampled plans (default ratio and probability, about 3 800 marked rows)
  (d) gv_ibot_loss alone on (c)'s row count, back to back on resident buffers

The three engines are built once and their windows alternate, so that drift of the shared machine lands on all of them; each
figure is the median of the windows with their spread.  (c) - (b) - (d) is the patch head's products and logits traffic (with the
row-table norm, the mask-token kernels and the centre update: a few tens of microseconds).

    python tools/ibot_bench.py [--windows 5] [--steps 10] [--out profiles/ibot.txt]
    python tools/ibot_bench.py --trace-only      # a few steps of (c) and nothing else: the run to put under rocprofv3 --kernel-trace --stats
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out-dim", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    import numpy as np
    from bench import synth_tiles
    from gipvit.engine import DinoEngine
    from gipvit.masking import MaskPlan, MaskSampler
    from gipvit.models import init_dino_head_state, init_vit_state
    from gipvit import ops
    dev = torch.device("cuda:0")
    B, K = args.batch, args.out_dim
    bb, hd = init_vit_state("vit_small", 224, 0, seed=0), init_dino_head_state(384, K, seed=1)
    tiles = synth_tiles(B, 256, 99, dev)

    def make(w):
        eng = DinoEngine(arch="vit_small", img_size=224, out_dim=K, batch=B, lr=5e-4 * B / 256, weight_decay=0.04, clip_grad=3.0, device=dev,
                         ibot_weight=w)
        eng.load_state(bb, hd)
        return eng
    sampler = MaskSampler(14, 2 * B, seed=0)
    plans = [sampler.sample(dev) for _ in range(8)]
    empty = MaskPlan.from_masks(np.zeros((2 * B, 196), bool), dev)
    Ms = [p.M for p in plans]
    variants = {"c": (make(1.0), lambda i: dict(masks=plans[i % len(plans)]))}
    if not args.trace_only:
        variants = {"a": (make(0.0), lambda i: {}), "b": (make(1.0), lambda i: dict(masks=empty)), **variants}

    def window(eng, kw, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            eng.step(tiles, lr=1e-5, **kw(i))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    for eng, kw in variants.values():          # warm-up: every shape of the timed windows
        window(eng, kw, 3)
    if args.trace_only:
        window(*variants["c"], args.steps)
        print(f"traced {args.steps} steps with the term on, M = {Ms}")
        return
    times = {k: [] for k in variants}
    for _ in range(args.windows):
        for k, (eng, kw) in variants.items():
            times[k].append(window(eng, kw, args.steps))
    # (d) the loss kernel alone
    M = int(statistics.median(Ms))
    eng = variants["c"][0]
    w = torch.full((M,), 1.0 / M, device=dev)
    s, t = eng.pr_s.hb.logits, eng.pr_t.hb.logits
    loss_t = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            ops.ibot_loss(s, t, eng.patch_center, w, eng.pr_s.hb.dlogits, eng.ibot, eng.patch_center_sum, eng.ibot_ws, M, K, 0.1, 0.04, 1.0)
        e1.record()
        torch.cuda.synchronize()
        loss_t.append(e0.elapsed_time(e1) / 50)
    med = {k: statistics.median(v) for k, v in times.items()}
    ld = statistics.median(loss_t)
    gb = M * K * (4 * 2 * 2 + 2) / 1e9
    lines = [f"iBOT term at ViT-S, B = {B}, 224 / 96 px, K = {K}; {args.windows} alternated windows of {args.steps} steps, device events, ms per step",
             f"marked rows per step (default ratio 0.1-0.5, probability 0.5): {Ms}"]
    for k, name in (("a", "(a) DINO step, term off"), ("b", "(b) term on, nothing marked"), ("c", "(c) term on, sampled plans")):
        lines.append(f"{name}: median {med[k]:.3f}  windows {min(times[k]):.3f} - {max(times[k]):.3f}  ({B / med[k] * 1e3:.0f} tiles/s)")
    lines.append(f"(d) gv_ibot_loss alone, M = {M}: median {ld * 1e3:.1f} us  windows {min(loss_t) * 1e3:.1f} - {max(loss_t) * 1e3:.1f}  "
                 f"({gb:.2f} GB algorithmic: {gb / ld:.2f} TB/s)")
    lines.append(f"split of (c) - (a) = {med['c'] - med['a']:.3f} ms: all-token last block of both groups {med['b'] - med['a']:.3f}, "
                 f"gv_ibot_loss {ld:.3f}, patch head products + logits traffic + row kernels {med['c'] - med['b'] - ld:.3f}")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
