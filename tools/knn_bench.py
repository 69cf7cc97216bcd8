"""gv_knn_vote against the same vote composed from torch calls, on one GPU in one process.

Shape: Q = 8192 query tiles against a bank of Nb = 65536 tiles, D = 384 (ViT-S), k = 20, C = 2, temp 0.07 -- one evaluation of the
k-NN monitor (gipvit/knn.py) on a mid-sized slide set.  The kernel is bound by the f32 MFMA rate (157.3 TFLOP/s) and does
2 Q Nb D FLOPs.  The baseline is what the monitor would be without the kernel: q @ bank.T in query chunks (the chunk's
similarity rows go to HBM and come back), topk, exp, scatter_add.  Both are timed with device events over repeated launches after
a warm-up, alternating, median of the windows; the two results are compared first.  With ``--monitor`` the teacher forward that
feeds the vote is timed too (ViT-S at 224 px through engine.FeatureExtractor, per batch of 256, scaled to the bank and query
counts), so the whole cost of one evaluation can be set next to the epoch it rides on.

    python tools/knn_bench.py [--monitor] [OUT]        # prints the table; OUT (profiles/knn_monitor.txt) also gets it"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import ops                                   # noqa: E402

dev = torch.device("cuda", 0)
Q, NB, D, K, C, TEMP = 8192, 65536, 384, 20, 2, 0.07
PEAK_F32_MFMA = 157.3e12
WARMUP, REPS, WINDOWS = 3, 5, 5
CHUNK = 1024                                             # baseline: query rows per matmul (a 268 MB similarity slab)


def torch_vote(q, bank, labels64):
    votes = torch.zeros(q.shape[0], C, dtype=torch.float32, device=q.device)
    for lo in range(0, q.shape[0], CHUNK):
        sim = q[lo:lo + CHUNK] @ bank.t()
        top_sim, top_idx = sim.topk(K, dim=1)
        votes[lo:lo + CHUNK].scatter_add_(1, labels64[top_idx], (top_sim / TEMP).exp())
    return votes


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps                    # ms


def main():
    argv = [a for a in sys.argv[1:] if a != "--monitor"]
    g = torch.Generator().manual_seed(0)
    q = torch.nn.functional.normalize(torch.randn(Q, D, generator=g), dim=1).to(dev)
    bank = torch.nn.functional.normalize(torch.randn(NB, D, generator=g), dim=1).to(dev)
    labels = torch.randint(0, C, (NB,), generator=g, dtype=torch.int32).to(dev)
    labels64 = labels.long()
    kern = lambda: ops.knn_vote(q, bank, labels, K, TEMP, C)
    base = lambda: torch_vote(q, bank, labels64)
    # same answer first: the two f32 products round differently, so a neighbour at the k-th boundary may swap in a few rows
    v_k, v_b = kern(), base()
    torch.cuda.synchronize()
    rel = ((v_k - v_b).abs() / v_b.abs().clamp_min(1e-30)).amax(1)
    agree = float((rel <= 1e-4).float().mean())
    for _ in range(WARMUP):
        kern(); base()
    torch.cuda.synchronize()
    tk, tb = [], []
    for _ in range(WINDOWS):                             # alternating windows: both see the same neighbours on the machine
        tk.append(window(kern, REPS))
        tb.append(window(base, REPS))
    ms_k, ms_b = statistics.median(tk), statistics.median(tb)
    flops = 2.0 * Q * NB * D
    floor_ms = flops / PEAK_F32_MFMA * 1e3
    lines = [f"# tools/knn_bench.py on {torch.cuda.get_device_name(0)}; Q = {Q}, Nb = {NB}, D = {D}, k = {K}, C = {C}; "
             f"median of {WINDOWS} alternating windows x {REPS} calls after {WARMUP} warm-up calls",
             f"gv_knn_vote (scan + merge launches)          {ms_k:9.3f} ms   windows {' '.join(f'{t:.3f}' for t in tk)}",
             f"torch: chunked q @ bank.T, topk, scatter_add  {ms_b:9.3f} ms   windows {' '.join(f'{t:.3f}' for t in tb)}",
             f"kernel / baseline                             {ms_k / ms_b:9.3f}   ({'kernel faster' if ms_k < ms_b else 'KERNEL SLOWER'})",
             f"2 Q Nb D = {flops / 1e9:.1f} GFLOP; f32 MFMA floor {floor_ms:.3f} ms; kernel at {100.0 * floor_ms / ms_k:.1f} % of 157.3 TFLOP/s "
             f"({flops / ms_k / 1e9:.1f} TFLOP/s)",
             f"rows whose votes agree with the baseline within 1e-4 relative: {100.0 * agree:.3f} % (max relative difference {float(rel.max()):.2e})"]
    if ms_k < floor_ms:
        lines.append("TIMING ERROR: the kernel time is below the f32 MFMA floor")
    if "--monitor" in sys.argv[1:]:
        from gipvit.engine import FeatureExtractor
        from gipvit.models import init_vit_state
        B = 256
        runner = FeatureExtractor("vit_small", 224, batch=B, device=dev)
        runner.load_state(init_vit_state("vit_small", 224, 0, seed=0))
        tiles = torch.randint(0, 256, (B, 224, 224, 3), generator=g, dtype=torch.uint8).to(dev)
        fwd = lambda: runner.run(tiles)
        for _ in range(WARMUP):
            fwd()
        torch.cuda.synchronize()
        ms_f = statistics.median(window(fwd, 10) for _ in range(WINDOWS))
        bank_ms, query_ms = ms_f * NB / B, ms_f * Q / B
        lines += [f"teacher forward, ViT-S 224 px, batch {B} (FeatureExtractor.run, tiles resident): {ms_f:.3f} ms = {B / ms_f * 1e3:.0f} tiles/s",
                  f"one evaluation at this shape: bank forward {bank_ms / 1e3:.2f} s ({NB} tiles, scaled from the batch time) + query forward "
                  f"{query_ms / 1e3:.2f} s ({Q} tiles) + k-NN {ms_k / 1e3:.4f} s = {(bank_ms + query_ms + ms_k) / 1e3:.2f} s (tile reading not included)"]
    text = "\n".join(lines)
    print(text)
    if argv:
        os.makedirs(os.path.dirname(os.path.abspath(argv[0])), exist_ok=True)
        with open(argv[0], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
