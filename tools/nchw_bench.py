"""Float32 NCHW input against uint8 NHWC tiles: gv_patchify_nchw against gv_patchify on the two shapes of the input contract
(B = 64 at 256 px with one window; B = 64 with DINO's fixed windows, 2 x 224 + 8 x 96 per tile) in us and algorithmic GB/s,
and a supervised ViT-S B = 64 step fed u8 tiles against the same step fed float32 NCHW (ms).  Device-event timing over
repeated launches after a warm-up (median of 5 windows); the inputs stay resident, so the reads of a repeat may hit the
Infinity Cache.  Prints the table (profiles/nchw_ingest.txt); ``python tools/nchw_bench.py OUT`` also writes it to OUT."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import ops                                   # noqa: E402
from gipvit.engine import MEAN_RON, STD_RON, SupervisedEngine   # noqa: E402

dev = torch.device("cuda", 0)
B = 64
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


def main():
    lines = [f"# tools/nchw_bench.py on {torch.cuda.get_device_name(0)}; B = {B}, median of {WINDOWS} windows x {REPS} launches"]
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (B, 256, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    f = torch.randn(B, 3, 256, 256, generator=g).to(dev)
    dino = [(224, [(16 * k, 16 * k) for k in range(2)]), (96, [(20 * l, 160 - 20 * l) for l in range(8)])]
    cases = (("B=64 256^2, one window", [(256, [(0, 0)])]), ("B=64 DINO 2x224 + 8x96", dino))
    lines.append(f"{'case':28s} {'kernel':20s} {'us':>8s} {'MB':>8s} {'GB/s':>8s}")
    for name, groups in cases:
        outs = [torch.empty(B * len(w) * (c // 16) ** 2, 768, dtype=ops.bf16, device=dev) for c, w in groups]
        px = sum(B * len(w) * c * c for c, w in groups)
        out_b = sum(o.numel() * 2 for o in outs)
        for kern, in_b, fn in (
                ("gv_patchify (u8)", px * 3, lambda: [ops.patchify(u8, w, c, MEAN_RON, STD_RON, out=o) for (c, w), o in zip(groups, outs)]),
                ("gv_patchify_nchw", px * 3 * 4, lambda: [ops.patchify_nchw(f, w, c, out=o) for (c, w), o in zip(groups, outs)])):
            us = timed(fn)
            mb = (in_b + out_b) / 1e6
            lines.append(f"{name:28s} {kern:20s} {us:8.1f} {mb:8.1f} {mb * 1e3 / us:8.0f}")
    # supervised ViT-S / 16 at 256 px, B = 64: one optimizer step, u8 tiles against float32 NCHW
    eng = SupervisedEngine(arch="vit_small", img_size=256, num_classes=2, batch=B, device=dev)
    from gipvit.models import init_vit_state
    eng.load_state(init_vit_state("vit_small", 256, 2, seed=0))
    tgt = torch.randint(0, 2, (B, 1), generator=g).to(dev)
    for name, x in (("u8 NHWC", u8), ("f32 NCHW", f)):
        ms = timed(lambda: eng.step(x, tgt), reps=10) / 1e3
        lines.append(f"supervised ViT-S B=64 step, {name:9s} {ms:8.3f} ms")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
