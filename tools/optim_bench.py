"""The optimizer pass with and without a range table: (a) the two gv_adamw_ema launches of the default step (decayed range, then
the no-decay tail) against (b) ONE gv_adamw_ema_ranges launch over the 29-range --layer-decay table, on
  * the ViT-S supervised arena (vit_small, 224 px, 2 classes: 21.7 M elements, no EMA copy: 30 B per element), and
  * an arena of the DINO step's size (44.0 M elements with an EMA copy: 40 B per element) cut into 29 ranges in the same proportions.
Device events around PASSES back-to-back passes after a warm-up; (a) and (b) alternate, REPS repetitions each in this one call.
Both move the same bytes, so (b) passes when its median is not above (a)'s median by more than (a)'s own spread (max - min of
its repetitions).  ``--chunk`` adds rows for other block-table row lengths (the first one listed is the one judged).
Prints the table (profiles/layer_decay.txt); ``python tools/optim_bench.py OUT`` also writes it; exit status 1 when (b) loses."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import ops                                                    # noqa: E402
from gipvit.engine import ARCHS, Arena, vit_param_specs                   # noqa: E402
from gipvit.layer_decay import LayerDecayPlan                             # noqa: E402

dev = torch.device("cuda", 0)
PASSES, REPS, WARM = 200, 5, 20


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(PASSES):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / PASSES * 1e3          # us per pass


def bench(name, spans, cut, scales, ema, chunks, lines):
    """spans: the 29 ranges [(lo, hi)]; cut: where the decayed ranges end; scales: lr scale per range."""
    n = spans[-1][1]
    g = torch.Generator().manual_seed(3)
    rnd = lambda: (torch.randn(n, generator=g) * 0.02).to(dev)
    p, grad, m, v = rnd(), rnd(), rnd(), rnd().abs()
    pb = torch.empty(n, dtype=ops.bf16, device=dev)
    t, tb = (rnd(), torch.empty(n, dtype=ops.bf16, device=dev)) if ema else (None, None)
    rows = torch.tensor([(s, 1.0 if hi <= cut else 0.0) for s, (lo, hi) in zip(scales, spans)], dtype=torch.float32).to(dev)
    kw = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=10, teacher_momentum=0.996 if ema else 0.0)
    sl = lambda x, lo, hi: None if x is None else x[lo:hi]

    def two_launches():
        for lo, hi, wd in ((0, cut, 0.05), (cut, n, 0.0)):
            ops.adamw_ema(p[lo:hi], grad[lo:hi], m[lo:hi], v[lo:hi], pb[lo:hi], sl(t, lo, hi), sl(tb, lo, hi), hi - lo, weight_decay=wd, **kw)

    def ranged(blocks):
        return lambda: ops.adamw_ema_ranges(p, grad, m, v, pb, t, tb, n, blocks, rows, weight_decay=0.05, **kw)

    variants = [("(a) 2 x gv_adamw_ema", two_launches)]
    for c in chunks:
        tab = ops.range_block_table(spans, c).to(dev)
        variants.append((f"(b) gv_adamw_ema_ranges, rows <= {c} ({tab.shape[0]} rows)", ranged(tab)))
    for _, fn in variants:
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in variants}
    for _ in range(REPS):
        for label, fn in variants:                     # alternated: (a), (b), (a), (b), ...
            times[label].append(window(fn))
    bytes_per = 40 if ema else 30
    lines.append(f"{name}: {n / 1e6:.2f} M elements, {len(spans)} ranges ({min(hi - lo for lo, hi in spans)} .. {max(hi - lo for lo, hi in spans)} elements), "
                 f"{bytes_per} B per element = {n * bytes_per / 1e6:.0f} MB per pass")
    lines.append(f"  {'':52s} {'median us':>10s} {'min':>8s} {'max':>8s} {'spread':>8s} {'GB/s':>8s}")
    for label, _ in variants:
        ts = times[label]
        med = statistics.median(ts)
        lines.append(f"  {label:52s} {med:10.1f} {min(ts):8.1f} {max(ts):8.1f} {max(ts) - min(ts):8.1f} {n * bytes_per / med / 1e3:8.0f}")
    a, b = times[variants[0][0]], times[variants[1][0]]
    ok = statistics.median(b) <= statistics.median(a) + (max(a) - min(a))
    lines.append(f"  verdict: (b) median {statistics.median(b):.1f} us {'<=' if ok else '>'} (a) median {statistics.median(a):.1f} us + (a) spread "
                 f"{max(a) - min(a):.1f} us  ->  {'PASS' if ok else 'LOSES'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--chunk", type=int, nargs="+", default=[1 << 12], help="block-table row lengths (elements); the first is judged")
    a = ap.parse_args()
    lines = [f"# tools/optim_bench.py on {torch.cuda.get_device_name(0)}; {PASSES} back-to-back passes per window after {WARM} warm-up passes, "
             f"{REPS} windows each, (a) and (b) alternated in one call; us per pass from device events"]
    arena = Arena(vit_param_specs("vit_small", 224, 2), "cpu", teacher=False)
    plan = LayerDecayPlan(arena, ARCHS["vit_small"]["depth"], 0.75)
    spans = [(r.lo, r.hi) for r in plan.ranges]
    scales = [row[0] for row in plan.range_rows().tolist()]
    ok = bench("ViT-S supervised arena", spans, arena.n_decay, scales, False, a.chunk, lines)
    # the DINO step's arena size, cut in the same proportions (bounds rounded to multiples of 4)
    N = 44_000_000
    f = N / arena.n
    bounds = [0] + [min(N, int(round(hi * f / 4)) * 4) for _, hi in spans[:-1]] + [N]
    assert all(b1 > b0 for b0, b1 in zip(bounds, bounds[1:]))
    big = list(zip(bounds, bounds[1:]))
    ok = bench("DINO-size arena with an EMA copy", big, big[13][1], scales, True, a.chunk, lines) and ok
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
