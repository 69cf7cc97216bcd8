"""gv_attention_probs timing (get_last_selfattention, vit.pyc@L255-262) at the FeatureExtractor shape -- B = 256 tiles of ViT-S at
256 px (N = 257, 6 heads) -- and the end-to-end cost of the CLS-row capture in FeatureExtractor.run (run vs run_with_attention,
alternating in one process).  Prints one JSON line.  Then the same for gv_attention_probs_stream at 512 px (N = 1 025): the CLS row at
B = 256 tiles (row form: K read once), the full map at B = 32 tiles (block form: P written once, 807 MB), and
FeatureExtractor(long_maps=True).run against run_with_attention in tiles/s -- a second JSON line (``--stream``: only that one).
Kernel times by HIP events here; run under `rocprofv3 --kernel-trace --stats` for the per-kernel table."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gipvit import ops                              # noqa: E402
from gipvit.engine import FeatureExtractor          # noqa: E402


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3          # us


def run_pair(fe, tiles, rounds):
    """median seconds of fe.run and fe.run_with_attention over one batch, alternating (host clock around work that ends in a synchronise)"""
    plain, cap = [], []
    for _ in range(2):
        fe.run(tiles); fe.run_with_attention(tiles)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for fn, acc in ((lambda: fe.run(tiles), plain), (lambda: fe.run_with_attention(tiles), cap)):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); acc.append(time.perf_counter() - t0)
    plain.sort(); cap.sort()
    return plain[len(plain) // 2], cap[len(cap) // 2]


def main():
    dev = torch.device("cuda:0")
    B, N, H = 256, 257, 6
    scale = 64 ** -0.5
    qkv = torch.randn(B * N, 3 * H * 64, device=dev).to(ops.bf16)
    _, lse = ops.attention_fwd(qkv, B, N, H, scale)
    p_all = torch.empty(B, H, N, N, device=dev)
    p_cls = torch.empty(B, H, 1, N, device=dev)
    t_all = timed(lambda: ops.attention_probs(qkv, lse, B, N, H, scale, N, p=p_all), 50)
    t_cls = timed(lambda: ops.attention_probs(qkv, lse, B, N, H, scale, 1, p=p_cls), 200)
    w_all, r_all = p_all.numel() * 4, B * N * H * 64 * 2 * 2          # P written; Q and K read once
    r_cls = B * N * H * 64 * 2 + B * H * 64 * 2                        # K read once + the CLS query
    fe = FeatureExtractor("vit_small", 256, batch=B, device=dev)
    tiles = torch.randint(0, 256, (B, 256, 256, 3), dtype=torch.uint8, device=dev)
    mp, mc = run_pair(fe, tiles, 10)
    print(json.dumps({
        "all_query_us": round(t_all, 2), "all_query_TBps": round((w_all + r_all) / t_all / 1e6, 3), "all_query_write_MB": round(w_all / 1e6, 1),
        "cls_row_us": round(t_cls, 2), "cls_row_TBps": round(r_cls / t_cls / 1e6, 3),
        "run_ms_median": round(mp * 1e3, 3), "run_with_attention_ms_median": round(mc * 1e3, 3),
        "capture_ratio": round(mc / mp, 4)}))


def stream():
    dev = torch.device("cuda:0")
    N, H = 1025, 6
    scale = 64 ** -0.5
    out = {}
    for name, B, q_rows, reps in (("cls_row", 256, 1, 2000), ("full_map", 32, N, 300)):
        qkv = torch.randn(B * N, 3 * H * 64, device=dev).to(ops.bf16)
        _, lse = ops.attention_fwd_stream(qkv, B, N, H, scale, q_limit=1 if q_rows == 1 else 0)
        p = torch.empty(B, H, q_rows, N, device=dev)
        ts = sorted(timed(lambda: ops.attention_probs_stream(qkv, lse, B, N, H, scale, q_rows, p=p), reps) for _ in range(5))
        t = ts[2]                                                       # median of 5 windows of `reps` launches
        out[f"{name}_us_min_max"] = [round(ts[0], 2), round(ts[-1], 2)]
        k_bytes, p_bytes = B * N * H * 64 * 2, p.numel() * 4
        must = k_bytes if q_rows == 1 else p_bytes                     # what the form must move: K once / P once
        out.update({f"{name}_tiles": B, f"{name}_us": round(t, 2), f"{name}_K_MB": round(k_bytes / 1e6, 1), f"{name}_P_MB": round(p_bytes / 1e6, 1),
                    f"{name}_TBps_of_must_move": round(must / t / 1e6, 3)})
        del qkv, lse, p
    B = 64
    fe = FeatureExtractor("vit_small", 512, batch=B, device=dev, long_maps=True)
    tiles = torch.randint(0, 256, (B, 512, 512, 3), dtype=torch.uint8, device=dev)
    mp, mc = run_pair(fe, tiles, 7)
    out.update({"px": 512, "batch": B, "run_tiles_per_s": round(B / mp, 1), "run_with_attention_tiles_per_s": round(B / mc, 1), "capture_ratio": round(mc / mp, 4)})
    print(json.dumps({"attention_probs_stream": out}))


if __name__ == "__main__":
    if "--stream" not in sys.argv[1:]:
        main()
    stream()
