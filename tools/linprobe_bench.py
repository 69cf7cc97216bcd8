"""One linear probe (gipvit/linprobe.py) at a realistic size, on one GPU in one process, next to the bank extraction it follows.

Shape: a bank of N = 50000 tiles x F = 1536 features (ViT-S, the CLS tokens of the last four blocks), H = 8 heads (a grid of eight
learning rates), C = 2, batch 1024, 100 epochs: 49 steps per epoch, two launches per step (gv_linprobe_train).  The whole run is
timed from the host around a synchronise (it is thousands of launches long), after a warm-up epoch, median of the repeats; one
epoch is also timed with device events.  The baseline is the same SGD step composed from torch calls for all heads at once
(gather, matmul, softmax, matmul, the momentum update), one epoch of it.  The bank extraction is ``FeatureExtractor.probe_features``
on ViT-S at 224 px per batch of 256, scaled to the bank.

    python tools/linprobe_bench.py [OUT]        # prints the table; OUT (profiles/linprobe_bench.txt) also gets it"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import ops                                   # noqa: E402
from gipvit.linprobe import epoch_permutations, init_heads, lr_scale_at      # noqa: E402

dev = torch.device("cuda", 0)
N, F, H, C, BATCH, EPOCHS, MU = 50000, 1536, 8, 2, 1024, 100, 0.9
REPEATS = 3


def torch_epoch(W, b, mW, mb, lr, x, y64, rows, scale):
    """One epoch of the same step from torch calls, all heads at once: W [H C, F], b [H C]."""
    for s in range(0, rows.shape[0], BATCH):
        r = rows[s:s + BATCH].long()
        xr, yr, m = x[r], y64[r], r.shape[0]
        p = torch.softmax((xr @ W.t() + b).view(m, H, C), dim=2)
        p[torch.arange(m, device=dev), :, yr] -= 1.0
        g = (p / m).view(m, H * C)
        mW.mul_(MU).add_(g.t() @ xr)
        mb.mul_(MU).add_(g.sum(0))
        W.sub_(mW * (lr * scale)[:, None])
        b.sub_(mb * (lr * scale))


def main():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, F, generator=g).to(dev)
    y = torch.randint(0, C, (N,), generator=g, dtype=torch.int32).to(dev)
    lr = torch.tensor([0.001 * 2 ** h * BATCH / 256.0 for h in range(H)], dtype=torch.float32, device=dev)
    wd = torch.zeros(H, device=dev)
    rows = torch.from_numpy(epoch_permutations(N, EPOCHS, 0).astype(np.int32)).to(dev)

    def run(epochs):
        W0, b0 = init_heads(H, C, F, 0)
        W, b = W0.to(dev), b0.to(dev)
        mW, mb, loss = torch.zeros_like(W), torch.zeros_like(b), torch.zeros(EPOCHS, H, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for e in range(epochs):
            ops.linprobe_train(W, b, mW, mb, lr, wd, x, y, rows[e], loss[e], BATCH, lr_scale_at(e, EPOCHS), MU)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, loss

    run(1)                                               # warm-up
    times = []
    for _ in range(REPEATS):
        t, loss = run(EPOCHS)
        times.append(t)
    sec = statistics.median(times)
    steps = EPOCHS * ((N + BATCH - 1) // BATCH)
    # one epoch by device events
    W0, b0 = init_heads(H, C, F, 0)
    W, b = W0.to(dev), b0.to(dev)
    mW, mb, l1 = torch.zeros_like(W), torch.zeros_like(b), torch.zeros(H, device=dev)
    ev = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.linprobe_train(W, b, mW, mb, lr, wd, x, y, rows[0], l1, BATCH, 1.0, MU)
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    ms_epoch = statistics.median(ev)
    # the torch composition, one epoch
    Wt, bt = init_heads(H, C, F, 0)
    Wt, bt = Wt.view(H * C, F).to(dev), bt.view(H * C).to(dev)
    mWt, mbt, lrt, y64 = torch.zeros_like(Wt), torch.zeros_like(bt), lr.repeat_interleave(C), y.long()
    torch_epoch(Wt, bt, mWt, mbt, lrt, x, y64, rows[0], 1.0)
    torch.cuda.synchronize()
    tb = []
    for _ in range(3):
        t0 = time.perf_counter()
        torch_epoch(Wt, bt, mWt, mbt, lrt, x, y64, rows[1], 1.0)
        torch.cuda.synchronize()
        tb.append((time.perf_counter() - t0) * 1e3)
    ms_torch = statistics.median(tb)
    bytes_step = 2.0 * BATCH * F * 4                     # the minibatch rows are read by both launches
    lines = [f"# tools/linprobe_bench.py on {torch.cuda.get_device_name(0)}; N = {N}, F = {F}, H = {H}, C = {C}, batch {BATCH}, {EPOCHS} epochs "
             f"({steps} steps, {2 * steps} launches); median of {REPEATS} runs after a warm-up epoch",
             f"100-epoch probe, gv_linprobe_train               {sec:9.3f} s    runs {' '.join(f'{t:.3f}' for t in times)}",
             f"one epoch by device events                       {ms_epoch:9.3f} ms   = {1e3 * ms_epoch / (steps / EPOCHS):.1f} us per step; "
             f"{bytes_step * (steps / EPOCHS) / ms_epoch / 1e6:.1f} GB/s of feature rows (each step reads its {bytes_step / 2e6:.1f} MB twice)",
             f"one epoch of the step composed from torch calls  {ms_torch:9.3f} ms   ({ms_torch / ms_epoch:.2f} x the kernel's epoch)",
             f"last-epoch mean loss per head (random labels): {' '.join(f'{v:.4f}' for v in (loss[-1] / N).tolist())}"]
    from gipvit.engine import FeatureExtractor
    from gipvit.models import init_vit_state
    B = 256
    runner = FeatureExtractor("vit_small", 224, batch=B, device=dev)
    runner.load_state(init_vit_state("vit_small", 224, 0, seed=0))
    tiles = torch.randint(0, 256, (B, 224, 224, 3), generator=g, dtype=torch.uint8).to(dev)
    for _ in range(3):
        runner.probe_features(tiles, 4)
    torch.cuda.synchronize()
    tf = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            runner.probe_features(tiles, 4)
        e1.record()
        torch.cuda.synchronize()
        tf.append(e0.elapsed_time(e1) / 5)
    ms_f = statistics.median(tf)
    lines += [f"bank extraction, ViT-S 224 px, batch {B} (FeatureExtractor.probe_features, 4 layers, tiles resident): {ms_f:.3f} ms per batch = "
              f"{B / ms_f * 1e3:.0f} tiles/s; {N} tiles: {ms_f * N / B / 1e3:.2f} s (scaled from the batch time, tile reading not included)",
              f"the probe is {100.0 * sec / (ms_f * N / B / 1e3):.1f} % of the extraction it follows"]
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
