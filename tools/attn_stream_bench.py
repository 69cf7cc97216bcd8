"""Timing of gv_attention_fwd_stream on 512-px shapes (1 025 tokens, 6 heads) beside the whole-sequence gv_attention_fwd at 257
tokens, and FeatureExtractor ViT-S tiles/s at 512 and 256 px: interleaved rounds in one process, random data, median and min.
python tools/attn_stream_bench.py [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gipvit import ops as o
from gipvit.engine import FeatureExtractor
from gipvit.models import init_vit_state

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--kernels-only", action="store_true", help="skip the FeatureExtractor part")
args = ap.parse_args()
dev = torch.device("cuda:0")
bf16 = torch.bfloat16
H = 6
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def flops(n_img, N, q_rows=None):
    return 4.0 * n_img * H * (N if q_rows is None else q_rows) * N * 64


def make(n_img, N):
    g = torch.Generator().manual_seed(n_img + N)
    qkv = torch.randn(n_img * N, 3 * H * 64, generator=g).to(bf16).to(dev)
    out = torch.empty(n_img * N, H * 64, dtype=bf16, device=dev)
    lse = torch.empty(n_img, H, N, dtype=torch.float32, device=dev)
    return qkv, out, lse


cases = []
for name, fn, n_img, N, ql in (("fwd_stream", o.attention_fwd_stream, 64, 1025, 0), ("fwd_stream", o.attention_fwd_stream, 256, 1025, 0),
                               ("fwd_stream q_limit=1", o.attention_fwd_stream, 256, 1025, 1), ("fwd (whole sequence)", o.attention_fwd, 256, 257, 0),
                               ("fwd_stream", o.attention_fwd_stream, 256, 257, 0)):
    qkv, out, lse = make(n_img, N)
    cases.append(dict(name=name, n_img=n_img, N=N, ql=ql, call=(lambda fn=fn, qkv=qkv, out=out, lse=lse, n_img=n_img, N=N, ql=ql:
                                                                 fn(qkv, n_img, N, H, 0.125, o=out, lse=lse, q_limit=ql)), t=[]))
for c in cases:                       # warm-up: code objects, LDS opt-in
    for _ in range(3):
        c["call"]()
torch.cuda.synchronize()
REPS = 5
for _ in range(args.rounds):          # interleaved: every round times every case
    for c in cases:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            c["call"]()
        e1.record()
        torch.cuda.synchronize()
        c["t"].append(e0.elapsed_time(e1) * 1e3 / REPS)
say(f"attention forward, H = {H}, head_dim 64, scale 0.125, randn bf16; {args.rounds} interleaved rounds x {REPS} launches, us per launch")
for c in cases:
    t = sorted(c["t"])
    med, mn = t[len(t) // 2], t[0]
    # useful FLOPs: every query row wanted (q_limit = 1: the 128-row block the kernel computes, and the 1 row that is used)
    f = flops(c["n_img"], c["N"], 128 if c["ql"] else None)
    say(f"  {c['name']:<22} n_img {c['n_img']:>3} N {c['N']:>4}: median {med:8.1f} us  min {mn:8.1f} us  {f / med / 1e6:6.1f} TFLOP/s (median)"
        + ("  [FLOPs of the one 128-row query block per pair]" if c["ql"] else ""))

# FeatureExtractor ViT-S, tiles / s
runs = []
for img, batch in (() if args.kernels_only else ((512, 64), (256, 256))):
    fx = FeatureExtractor("vit_small", img, batch, 0, device=dev)
    fx.load_state(init_vit_state("vit_small", img, 0, seed=0))
    tiles = torch.randint(0, 256, (batch, img, img, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(img)).to(dev)
    for _ in range(2):
        fx.forward(tiles)
    torch.cuda.synchronize()
    runs.append(dict(img=img, batch=batch, fx=fx, tiles=tiles, t=[]))
for _ in range(args.rounds):
    for r in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            r["fx"].forward(r["tiles"])
        torch.cuda.synchronize()
        r["t"].append((time.perf_counter() - t0) / 3)
if runs:
    say("FeatureExtractor ViT-S forward (uint8 tiles on the device -> CLS features), host clock around 3 batches ending in a synchronise")
for r in runs:
    t = sorted(r["t"])
    say(f"  {r['img']} px, batch {r['batch']:>3}: median {t[len(t) // 2] * 1e3:7.2f} ms  min {t[0] * 1e3:7.2f} ms  = {r['batch'] / t[len(t) // 2]:8.0f} tiles/s (median)")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
