"""gv_crop_augment_stain against gv_crop_augment at the headline shape (profiles/stain_jitter.txt): 64 tiles of 256 px, 128 crops
at 224 + 512 at 96, the same boxes and view draws, every crop jittered at sigma 0.05.  One sample = both sizes' calls, event to
event over 40 back-to-back repetitions after 20 warm-up ones; 7 samples per variant, alternating; the medians are compared.

    python tools/stain_bench.py        one JSON line
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import ops                                                # noqa: E402
from gipvit.multicrop import MultiCropSampler, ViewAugmentSampler     # noqa: E402
from gipvit.stain import StainJitterSampler                           # noqa: E402

B, REPS, SAMPLES = 64, 40, 7


def main():
    dev = torch.device("cuda:0")
    tiles = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, 256, 256, 3), dtype=np.uint8)).to(dev)
    boxes = MultiCropSampler(B, 256, 2, 8, seed=1).sample(dev)
    views = ViewAugmentSampler(B, 2, 8, seed=2).sample(dev)
    stains = StainJitterSampler(B, 2, 8, 0.05, seed=3).sample(dev)
    stats = torch.zeros(8 * B, dtype=torch.int64, device=dev)
    outs = (torch.empty(2 * B, 224, 224, 3, dtype=torch.uint8, device=dev), torch.empty(8 * B, 96, 96, 3, dtype=torch.uint8, device=dev))

    def plain():
        ops.crop_augment(tiles, boxes[0], views[0], stats, 224, out=outs[0])
        ops.crop_augment(tiles, boxes[1], views[1], stats, 96, out=outs[1])

    def stained():
        ops.crop_augment_stain(tiles, boxes[0], views[0], stains[0], stats, 224, out=outs[0])
        ops.crop_augment_stain(tiles, boxes[1], views[1], stains[1], stats, 96, out=outs[1])

    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / REPS

    for _ in range(20):
        plain(); stained()
    torch.cuda.synchronize()
    t = {"plain": [], "stain": []}
    for _ in range(SAMPLES):
        t["plain"].append(sample(plain))
        t["stain"].append(sample(stained))
    med = {k: statistics.median(v) for k, v in t.items()}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "plain_us": [round(v, 1) for v in t["plain"]], "stain_us": [round(v, 1) for v in t["stain"]],
                      "plain_median_us": round(med["plain"], 1), "stain_median_us": round(med["stain"], 1),
                      "delta_us": round(med["stain"] - med["plain"], 1)}))


if __name__ == "__main__":
    main()
