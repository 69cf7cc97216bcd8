"""Macenko stain normalisation at the headline shapes (profiles/stain_norm.txt):

  patchify   gv_patchify against gv_patchify_stain (every record on) and gv_patchify_stain with every record off, B = 256 tiles of
             256 px, one window; one sample = 40 back-to-back calls event to event after 20 warm-up ones, 7 samples per variant,
             alternating
  fit        MacenkoEstimator.fit over 500 tiles of 256 px: host clock around the call (it ends in device-to-host copies), 7 samples,
             and the three passes alone, event to event
  extract    ViT-S FeatureExtractor.run over 2048 tiles of 256 px in batches of 256, with and without a record set: host clock around
             run + synchronise, 5 samples per variant, alternating

    python tools/stainnorm_bench.py        one JSON line
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import models as M, ops, stainnorm as SN          # noqa: E402
from gipvit.engine import FeatureExtractor                    # noqa: E402

B, REPS, SAMPLES = 256, 40, 7
MEAN, STD = (0.8998, 0.8253, 0.9357), (0.1125, 0.1751, 0.0787)


def he_tiles(n, px, seed):
    """n synthetic H&E tiles on the device (two stain vectors, gamma concentrations, 15 % near-white pixels, od noise 0.01): 32
    distinct ones, repeated."""
    rng = np.random.default_rng(seed)
    m = 32 * px * px
    cH, cE = rng.gamma(2.0, 0.35, m), rng.gamma(2.0, 0.25, m)
    white = rng.random(m) < 0.15
    cH[white] *= 0.02; cE[white] *= 0.02
    H, E = np.array([0.56, 0.72, 0.41]), np.array([0.22, 0.80, 0.56])
    od = np.outer(cH, H / np.linalg.norm(H)) + np.outer(cE, E / np.linalg.norm(E)) + rng.normal(0.0, 0.01, (m, 3))
    base = np.clip(np.rint(256.0 * np.exp(-np.maximum(od, 0.0)) - 1.0), 0, 255).astype(np.uint8).reshape(32, px, px, 3)
    return torch.from_numpy(base).to("cuda:0").repeat(-(-n // 32), 1, 1, 1)[:n].contiguous()


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    tiles = he_tiles(B, 256, 0)
    est = SN.MacenkoEstimator(dev)
    st = est.fit(tiles[:32])
    assert st.on, st.reason
    on = SN.pack_record(st.record).repeat(B).to(dev)
    off = SN.pack_record(SN.off_record()).repeat(B).to(dev)
    patches = torch.empty(B * 256, 768, dtype=ops.bf16, device=dev)
    variants = {"patchify": lambda: ops.patchify(tiles, [(0, 0)], 256, MEAN, STD, out=patches),
                "patchify_stain": lambda: ops.patchify(tiles, [(0, 0)], 256, MEAN, STD, out=patches, stain=on),
                "patchify_stain_off": lambda: ops.patchify(tiles, [(0, 0)], 256, MEAN, STD, out=patches, stain=off)}
    for _ in range(20):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(SAMPLES):
        for k, fn in variants.items():
            t[k].append(events(fn, REPS))
    out["patchify_us"] = {k: [round(x, 1) for x in v] for k, v in t.items()}
    out["patchify_median_us"] = {k: round(statistics.median(v), 1) for k, v in t.items()}
    out["patchify_bytes"] = B * 256 * 256 * 3 + B * 256 * 768 * 2

    slide = he_tiles(500, 256, 1)
    fits = []
    for i in range(SAMPLES + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = est.fit(slide)
        fits.append((time.perf_counter() - t0) * 1e3)
    assert s.on
    ref = {"V": np.linalg.qr(np.array([[0.6, 0.1], [0.7, -0.5], [0.4, 0.8]]))[0], "pinv": np.linalg.pinv(s.HE)}
    cmax = SN.LN256 * np.maximum(ref["pinv"], 0).sum(1)
    passes = {"stats": lambda: ops.stain_stats(slide, 219), "angle_hist": lambda: ops.stain_angle_hist(slide, ref["V"], 219),
              "conc_hist": lambda: ops.stain_conc_hist(slide, ref["pinv"], cmax)}
    out["fit_ms"] = [round(x, 2) for x in fits[2:]]
    out["fit_median_ms"] = round(statistics.median(fits[2:]), 2)
    out["pass_us"] = {}
    for k, fn in passes.items():
        for _ in range(3):
            fn()
        out["pass_us"][k] = round(statistics.median(events(fn, 10) for _ in range(5)), 1)
    out["pass_bytes"] = 500 * 256 * 256 * 3
    del slide

    fx = FeatureExtractor("vit_small", 256, B, 0, device=dev)
    fx.load_state(M.init_vit_state("vit_small", 256, 0, seed=0))
    many = he_tiles(2048, 256, 2)
    rate = {"plain": [], "stain": []}

    def run(rec):
        fx.set_stain(rec)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fx.run(many)
        torch.cuda.synchronize()
        return many.shape[0] / (time.perf_counter() - t0)
    run(None); run(st.record)
    for _ in range(5):
        rate["plain"].append(run(None))
        rate["stain"].append(run(st.record))
    fx.set_stain(None)
    out["extract_tiles_per_s"] = {k: [round(x) for x in v] for k, v in rate.items()}
    out["extract_median_tiles_per_s"] = {k: round(statistics.median(v)) for k, v in rate.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
