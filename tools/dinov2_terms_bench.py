#!/usr/bin/env python3
"""The DINOv2 loss options at the headline shapes, event-timed: one Sinkhorn-Knopp centring (2 n + 1 calls of gv_sinkhorn_*, R = 128
teacher rows, K = 65536, n = 3) and one KoLeo forward + backward (G = 2, B = 64, D = 384, 16-bit features).  Every window is warmed
up, holds `--calls` repetitions (2000: a window is 15 ms for the shortest call and 150 ms for the whole centring) and is repeated
`--windows` times: the line gives the median and the spread of the windows, per
entry point as well (each in windows of its own: the sum of the parts and the whole need not agree to the microsecond).
`--step-ms`: the step the figures are set against."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gipvit import _lib as L, ops as o      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--step-ms", type=float, default=13.0)
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    """-> (median, min, max) microseconds per call of fn over the windows."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / args.calls)
    return statistics.median(out), min(out), max(out)


def line(name, t, extra=""):
    print(f"{name:<34s} {t[0]:8.1f} us  (windows {t[1]:.1f} .. {t[2]:.1f})  {100.0 * t[0] / (1000.0 * args.step_ms):5.2f} % of a {args.step_ms:g}-ms step{extra}")


# ---- Sinkhorn-Knopp: cosine logits like the weight-normalised last layer's
R, K, n, tau = 128, 65536, args.iters, 0.04
g = torch.Generator().manual_seed(0)
z = torch.nn.functional.normalize(torch.randn(R, 256, generator=g), dim=1)
W = torch.nn.functional.normalize(torch.randn(K, 256, generator=g), dim=1)
T = (z @ W.t()).to(dev)
shift, a, b, cs, skc = (torch.zeros(m, device=dev) for m in (1, K, R, K, K))
ws = torch.zeros(L.lib.gv_sinkhorn_workspace_bytes(R, K) // 4, device=dev)
st = (T, shift, a, b, cs, ws)


def sinkhorn():
    o.sinkhorn_shift(*st, R, K, tau)
    for it in range(n):
        o.sinkhorn_cols(*st, R, K, tau, first=it == 0)
        if it < n - 1:
            o.sinkhorn_rows(*st, R, K, tau, first=it == 0)
    o.sinkhorn_finish(*st, skc, R, K, tau, first=n == 1)


mb = R * K * 4 / 1e6
whole = timed(sinkhorn)
line(f"sinkhorn R={R} K={K} n={n}", whole, f"  [{2 * n} passes over {mb:.1f} MB of logits: {2 * n * mb / whole[0]:.2f} TB/s]")
sinkhorn()
for name, fn in (("  gv_sinkhorn_shift", lambda: o.sinkhorn_shift(*st, R, K, tau)), ("  gv_sinkhorn_cols", lambda: o.sinkhorn_cols(*st, R, K, tau)),
                 ("  gv_sinkhorn_rows", lambda: o.sinkhorn_rows(*st, R, K, tau)), ("  gv_sinkhorn_finish", lambda: o.sinkhorn_finish(*st, skc, R, K, tau))):
    if "rows" in name or "finish" in name:      # both fold colsum into a: keep a where the iteration left it
        keep = a.clone()
        t = timed(lambda: (a.copy_(keep), fn()))
        t0 = timed(lambda: a.copy_(keep))
        t = tuple(x - t0[0] for x in t)
    else:
        t = timed(fn)
    line(name, t, f"  [{mb / t[0]:.2f} TB/s]" if "finish" not in name else "")      # MB per us = TB/s
torch.cuda.synchronize()
assert bool(torch.isfinite(skc).all())

# ---- KoLeo
G, B, D, weight = 2, 64, 384, 0.1
feats = torch.randn(G * B + 8 * B, D, generator=g).to(dev, o.bf16)
dfeats = torch.zeros_like(feats)
kws = torch.zeros(L.lib.gv_koleo_workspace_bytes(G, B, D) // 4, device=dev)
nn, kol = torch.zeros(G * B, dtype=torch.int32, device=dev), torch.zeros(1, device=dev)
fwd = lambda: o.koleo_fwd(feats, kws, nn, kol, G, B, D)
bwd = lambda: o.koleo_bwd(dfeats, kws, nn, G, B, D, weight)
line(f"koleo fwd + bwd G={G} B={B} D={D}", timed(lambda: (fwd(), bwd())))
line("  gv_koleo_fwd", timed(fwd))
line("  gv_koleo_bwd", timed(bwd))
torch.cuda.synchronize()
print(f"koleo {float(kol):.5f}, sk_center spread {float(skc.max() - skc.min()):.4f}")
