"""gv_token_mean_fwd / gv_token_mean_bwd (`--gp avg`) at the supervised step's shapes: device events around PASSES back-to-back
launches after a warm-up, REPS repetitions, median / min and the algorithmic bytes over the median.  The launches of a window
rotate over COPIES buffer sets, inputs of the forward and outputs of the backward alike (at B = 64, ViT-S, 257 tokens: 328 MB of x,
494 MB of g + gb -- both more than the 256-MB Infinity Cache), so a repeat finds neither its input nor its output lines resident.
Prints the table (profiles/global_pool.txt); ``python tools/pool_bench.py OUT`` also writes it."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import ops                                                    # noqa: E402

dev = torch.device("cuda", 0)
PASSES, REPS, WARM, COPIES = 208, 5, 26, 13


def window(fns):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(PASSES):
        fns[k % len(fns)]()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / PASSES * 1e3          # us per launch


def main():
    lines = [f"gv_token_mean_fwd / gv_token_mean_bwd: {PASSES} launches per window over {COPIES} buffer sets, {REPS} windows, us per launch"]
    for B, N, D in ((64, 257, 384), (256, 257, 384), (64, 1025, 384), (64, 257, 768)):
        xs = [torch.randn(B * N, D, device=dev) for _ in range(COPIES)]
        pooled = torch.empty(B, D, device=dev)
        dpool = torch.randn(B, D, device=dev)
        scale = torch.rand(B, device=dev) + 0.5
        gs = [torch.empty(B * N, D, device=dev) for _ in range(COPIES)]
        gbs = [torch.empty(B * N, D, dtype=ops.bf16, device=dev) for _ in range(COPIES)]
        fwd = [lambda x=x: ops.token_mean_fwd(x, pooled, B, N, D) for x in xs]
        bwd = [lambda g=g, gb=gb: ops.token_mean_bwd(dpool, g, gb, B, N, D, gb_scale=scale) for g, gb in zip(gs, gbs)]
        for name, fns, nbytes in (("fwd", fwd, B * (N - 1) * D * 4 + B * D * 4), ("bwd", bwd, B * D * 4 + B * N * D * 6)):
            for k in range(WARM):
                fns[k % len(fns)]()
            torch.cuda.synchronize()
            t = [window(fns) for _ in range(REPS)]
            med = statistics.median(t)
            lines.append(f"  ({B:3d}, {N:4d}, {D}) {name}: median {med:7.1f}  min {min(t):7.1f}  max {max(t):7.1f}   {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e6:5.2f} TB/s")
        del xs, gs, gbs
    out = "\n".join(lines)
    print(out)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
