"""One epoch of the attention-MIL probe (gipvit/mil.py) at a representative size, on one GPU in one process.

Shape: 1000 bags x 500 tiles, F = 384 features (ViT-S CLS tokens), L = 128, C = 2, batch 8: 125 Adam steps per epoch, three
launches per step (gv_mil_train).  The epoch is timed with device events after a warm-up epoch, median of the repeats.  The
baseline is the same step in eager torch f32 on the same device: the eight bags of a step as one [8, 500, F] batch, autograd,
torch.optim.Adam.

    python tools/mil_bench.py [OUT]        # prints the table; OUT (profiles/mil_bench.txt) also gets it"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import ops                                   # noqa: E402
from gipvit.linprobe import epoch_permutations            # noqa: E402
from gipvit.mil import init_params, param_views           # noqa: E402

dev = torch.device("cuda", 0)
BAGS, TILES, F, L, C, BATCH, LR, WD = 1000, 500, 384, 128, 2, 8, 5e-4, 1e-4
REPEATS = 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(BAGS * TILES, F, generator=g).to(dev)
    y = torch.randint(0, C, (BAGS,), generator=g, dtype=torch.int32).to(dev)
    ptr = torch.arange(0, BAGS * TILES + 1, TILES, dtype=torch.int32, device=dev)
    order = torch.from_numpy(epoch_permutations(BAGS, 2, 0).astype(np.int32)).to(dev)
    steps = -(-BAGS // BATCH)

    def kernel_epoch(state, e):
        P, m, v, loss = state
        ops.mil_train(P, m, v, x, ptr, y, order[e], loss[e], L, C, BATCH, TILES, e * steps, LR, 1.0, WD)

    def fresh():
        P = init_params(L, C, F, 0).to(dev)
        return P, torch.zeros_like(P), torch.zeros_like(P), torch.zeros(2, 1, device=dev)
    ours = []
    for _ in range(REPEATS):
        st = fresh()
        kernel_epoch(st, 0)                                                # warm-up epoch
        torch.cuda.synchronize()
        ours.append(timed(lambda: kernel_epoch(st, 1)))
    loss_ours = float(st[3][1]) / BAGS

    def torch_epoch(P, opt, e):
        total = torch.zeros((), device=dev)
        xb, y64, o = x.view(BAGS, TILES, F), y.long(), order[e].long()
        for s in range(0, BAGS, BATCH):
            b = o[s:s + BATCH]
            xs = xb[b]
            t = torch.tanh(xs @ P["attention_V.weight"].t() + P["attention_V.bias"])
            gg = torch.sigmoid(xs @ P["attention_U.weight"].t() + P["attention_U.bias"])
            a = torch.softmax((t * gg) @ P["attention_w.weight"].reshape(-1) + P["attention_w.bias"], dim=1)
            z = torch.einsum("bn,bnf->bf", a, xs)
            loss = torch.nn.functional.cross_entropy(z @ P["classifier.weight"].t() + P["classifier.bias"], y64[b])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += loss.detach() * len(b)
        return total
    eager = []
    for _ in range(REPEATS):
        P = {k: t.clone().to(dev).requires_grad_(True) for k, t in param_views(init_params(L, C, F, 0), L, C, F).items()}
        opt = torch.optim.Adam(list(P.values()), lr=LR, weight_decay=WD)
        torch_epoch(P, opt, 0)
        torch.cuda.synchronize()
        out = []
        eager.append(timed(lambda: out.append(torch_epoch(P, opt, 1))))
    loss_eager = float(out[0]) / BAGS
    k, t = statistics.median(ours), statistics.median(eager)
    lines = [
        f"# tools/mil_bench.py on {torch.cuda.get_device_name(0)}; {BAGS} bags x {TILES} tiles, F = {F}, L = {L}, C = {C}, batch {BATCH}: "
        f"{steps} steps, {3 * steps} launches per epoch; device events, median of {REPEATS} after a warm-up epoch",
        f"one epoch, gv_mil_train                              {k:9.3f} ms   = {1e3 * k / steps:.1f} us per step   runs " + " ".join(f"{v:.3f}" for v in ours),
        f"one epoch of the same step in eager torch f32        {t:9.3f} ms   = {1e3 * t / steps:.1f} us per step ({t / k:.2f} x the kernels' epoch)   runs "
        + " ".join(f"{v:.3f}" for v in eager),
        f"second-epoch mean loss (random labels): kernels {loss_ours:.6f}, eager {loss_eager:.6f}",
    ]
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
