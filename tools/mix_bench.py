"""Cost of mixing inside the patchify pass: gv_patchify against gv_patchify_mix (all-blend and all-paste tables) and
gv_patchify_nchw against gv_patchify_nchw_mix at B = 256, 256 x 256, one window -- us, algorithmic MB and GB/s, and the ratio
to the plain kernel next to the ratio of algorithmic bytes (the mixed kernels read a second source: (2 in + out) / (in + out) =
1.33 for uint8 tiles, 1.67 for float32 NCHW).  Then one supervised ViT-S B = 64 step at 256 px with and without a plan (ms).
Device-event timing over repeated launches after a warm-up (median of 5 windows); the inputs stay resident, so the reads of a
repeat may hit the Infinity Cache.  Prints the table (profiles/mixup.txt); ``python tools/mix_bench.py OUT`` also writes it."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import ops                                   # noqa: E402
from gipvit.engine import MEAN_RON, STD_RON, SupervisedEngine   # noqa: E402
from gipvit.mixup import MixPlan, MixSampler             # noqa: E402

dev = torch.device("cuda", 0)
B, S = 256, 256
REPS, WINDOWS = 50, 5


def timed(fn, reps=REPS):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / reps * 1e3)       # us
    return statistics.median(per)


def table(n, kind):
    """All-blend rows, or all-paste rows with a 128 x 128 box at an odd origin (a quarter of the window comes from the partner)."""
    rows = MixPlan.make_rows(n)
    for i in range(n):
        if kind == "blend":
            MixPlan.set_row(rows, i, 0.37, None)
        else:
            MixPlan.set_row(rows, i, 0.75, (37, 165, 51, 179))
    return MixPlan(rows, dev).table


def main():
    lines = [f"# tools/mix_bench.py on {torch.cuda.get_device_name(0)}; B = {B}, {S} x {S}, one window; median of {WINDOWS} windows x {REPS} launches"]
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    f = torch.randn(B, 3, S, S, generator=g).to(dev)
    out = torch.empty(B * (S // 16) ** 2, 768, dtype=ops.bf16, device=dev)
    w = [(0, 0)]
    blend, paste = table(B, "blend"), table(B, "paste")
    px = B * S * S
    out_b = out.numel() * 2
    lines.append(f"{'kernel':34s} {'us':>8s} {'MB':>8s} {'GB/s':>8s} {'x plain':>8s} {'x bytes':>8s}")
    for name, in_b, plain, mixed in (
            ("gv_patchify (u8)", px * 3, lambda: ops.patchify(u8, w, S, MEAN_RON, STD_RON, out=out),
             lambda t: (lambda: ops.patchify(u8, w, S, MEAN_RON, STD_RON, out=out, mix=t))),
            ("gv_patchify_nchw", px * 12, lambda: ops.patchify_nchw(f, w, S, out=out), lambda t: (lambda: ops.patchify_nchw(f, w, S, out=out, mix=t)))):
        us0 = timed(plain)
        mb0 = (in_b + out_b) / 1e6
        lines.append(f"{name:34s} {us0:8.1f} {mb0:8.1f} {mb0 * 1e3 / us0:8.0f} {1.0:8.2f} {1.0:8.2f}")
        # blend reads both sources whole; the paste table reads the partner for the box only (a quarter of the pixels + the runs it cuts)
        for kind, t, mb in (("all blend", blend, (2 * in_b + out_b) / 1e6), ("all paste (128^2 box)", paste, (in_b + out_b) / 1e6)):
            us = timed(mixed(t))
            lines.append(f"{'  _mix ' + kind:34s} {us:8.1f} {mb:8.1f} {mb * 1e3 / us:8.0f} {us / us0:8.2f} {mb / mb0:8.2f}")
    # supervised ViT-S / 16 at 256 px, B = 64: one optimizer step without a plan (lsce), and with one (soft_ce; the sampler's draw and the
    # table's host-to-device copy included, as the driver pays them)
    Bs = 64
    from gipvit.models import init_vit_state
    tgt = torch.randint(0, 2, (Bs, 1), generator=g).to(dev)
    st = init_vit_state("vit_small", 256, 2, seed=0)
    e0 = SupervisedEngine(arch="vit_small", img_size=256, num_classes=2, batch=Bs, device=dev)
    e0.load_state(st)
    ms0 = timed(lambda: e0.step(u8[:Bs], tgt), reps=10) / 1e3
    lines.append(f"supervised ViT-S B=64 step, no plan (lsce)        {ms0:8.3f} ms")
    del e0
    e1 = SupervisedEngine(arch="vit_small", img_size=256, num_classes=2, batch=Bs, device=dev, loss="soft_ce")
    e1.load_state(st)
    smp = MixSampler(0.8, 1.0, None, 1.0, 0.5, "batch", Bs, 256, seed=0)
    ms1 = timed(lambda: e1.step(u8[:Bs], tgt, mix=smp.sample(dev)), reps=10) / 1e3
    lines.append(f"supervised ViT-S B=64 step, --mixup 0.8 --cutmix 1 {ms1:8.3f} ms")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
