"""Cost of random erasing inside the patchify pass: gv_patchify against gv_patchify_erase and gv_patchify_nchw against
gv_patchify_nchw_erase at B = 256, 256 x 256, one window, with the sampler's tables at --reprob 0.25 and 1.0 (--recount 1) in the
'pixel' (noise generated in the kernel) and 'const' (a value from the table) modes -- us, algorithmic MB and GB/s.  Algorithmic
bytes: the output rows + the input of the pixels that are NOT erased (an erased pixel needs no load).  The plain kernel is timed
before and after the erase kernels of its input form: the two figures are its run-to-run spread in this session.
Device-event timing over repeated launches after a warm-up (median of 5 windows); the inputs stay resident, so the reads of a
repeat may hit the Infinity Cache.  Prints the table (profiles/random_erasing.txt); ``python tools/erase_bench.py OUT`` also writes it."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import ops                                   # noqa: E402
from gipvit.engine import MEAN_RON, STD_RON              # noqa: E402
from gipvit.erasing import EraseSampler                  # noqa: E402

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


def erased_share(rows):
    """Share of the batch's pixels inside at least one box."""
    n = 0
    for r in rows:
        m = torch.zeros(S, S, dtype=torch.bool)
        for b in range(int(r["n_box"])):
            yl, yh, xl, xh = (int(v) for v in r["box"][b])
            m[yl:yh, xl:xh] = True
        n += int(m.sum())
    return n / float(len(rows) * S * S)


def main():
    lines = [f"# tools/erase_bench.py on {torch.cuda.get_device_name(0)}; B = {B}, {S} x {S}, one window; median of {WINDOWS} windows x {REPS} launches"]
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    f = torch.randn(B, 3, S, S, generator=g).to(dev)
    out = torch.empty(B * (S // 16) ** 2, 768, dtype=ops.bf16, device=dev)
    w = [(0, 0)]
    plans = []
    for prob in (0.25, 1.0):
        for mode in ("pixel", "const"):
            p = EraseSampler(prob, mode, 1, B, S, seed=0).sample(dev)
            plans.append((f"reprob {prob:g} {mode}", (p.table, p.seed), erased_share(p.rows)))
    px = B * S * S
    out_b = out.numel() * 2
    lines.append(f"{'kernel':40s} {'erased':>7s} {'us':>8s} {'MB':>8s} {'GB/s':>8s} {'x plain':>8s}")
    for name, in_b, run in (("gv_patchify (u8)", px * 3, lambda **kw: ops.patchify(u8, w, S, MEAN_RON, STD_RON, out=out, **kw)),
                            ("gv_patchify_nchw", px * 12, lambda **kw: ops.patchify_nchw(f, w, S, out=out, **kw))):
        us0 = timed(run)
        mb0 = (in_b + out_b) / 1e6
        lines.append(f"{name:40s} {0.0:7.3f} {us0:8.1f} {mb0:8.1f} {mb0 * 1e3 / us0:8.0f} {1.0:8.2f}")
        for what, er, share in plans:
            us = timed(lambda: run(erase=er))
            mb = (in_b * (1.0 - share) + out_b) / 1e6
            lines.append(f"{'  _erase ' + what:40s} {share:7.3f} {us:8.1f} {mb:8.1f} {mb * 1e3 / us:8.0f} {us / us0:8.2f}")
        us1 = timed(run)
        lines.append(f"{name + ' (again)':40s} {0.0:7.3f} {us1:8.1f} {mb0:8.1f} {mb0 * 1e3 / us1:8.0f} {us1 / us0:8.2f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
