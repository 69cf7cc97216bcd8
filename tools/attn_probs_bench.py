"""gv_attention_probs timing (get_last_selfattention, vit.pyc@L255-262) at the FeatureExtractor shape -- B = 256 tiles of ViT-S at
256 px (N = 257, 6 heads) -- and the end-to-end cost of the CLS-row capture in FeatureExtractor.run (run vs run_with_attention,
alternating in one process).  Prints one JSON line.  Kernel times by HIP events here; run under
`rocprofv3 --kernel-trace --stats` for the per-kernel table."""
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
    plain, cap = [], []
    for _ in range(2):
        fe.run(tiles); fe.run_with_attention(tiles)
    torch.cuda.synchronize()
    for _ in range(10):
        for fn, acc in ((lambda: fe.run(tiles), plain), (lambda: fe.run_with_attention(tiles), cap)):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); acc.append(time.perf_counter() - t0)
    plain.sort(); cap.sort()
    print(json.dumps({
        "all_query_us": round(t_all, 2), "all_query_TBps": round((w_all + r_all) / t_all / 1e6, 3), "all_query_write_MB": round(w_all / 1e6, 1),
        "cls_row_us": round(t_cls, 2), "cls_row_TBps": round(r_cls / t_cls / 1e6, 3),
        "run_ms_median": round(plain[len(plain) // 2] * 1e3, 3), "run_with_attention_ms_median": round(cap[len(cap) // 2] * 1e3, 3),
        "capture_ratio": round(cap[len(cap) // 2] / plain[len(plain) // 2], 4)}))


if __name__ == "__main__":
    main()
