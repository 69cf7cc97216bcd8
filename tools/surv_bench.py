"""One epoch of the survival probe (gipvit/survival.py) beside one epoch of the MIL probe at C = 1 on the same bags, and one cohort
evaluation, on one GPU in one process.  Recorded once, no gate: nothing here is tuned.

Shape: the MIL probe's measured one (tools/mil_bench.py): 1000 bags x 500 tiles, F = 384, L = 128, batch 8: 125 Adam steps per
epoch, four launches per step (gv_surv_train) against three (gv_mil_train).  A window is fresh parameters, a warm-up epoch and one
epoch timed with device events; the rows take their windows in turn, REPEATS rounds, and report median, min and max.  gv_cox_eval
at n = 4096 (tied times and risks), median of the repeats after a warm-up call.

    python tools/surv_bench.py [OUT] [--parent-lib PATH]    # prints the table; OUT (profiles/survival.txt) also gets it
``--parent-lib``: time gv_surv_train and gv_mil_train out of another build of the library (the parent commit's) as well, window
by window in turn with this build's; a change that must not cost speed has each of its medians inside the parent's min .. max."""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gipvit import _lib as L, ops                         # noqa: E402
from gipvit.linprobe import epoch_permutations            # noqa: E402
from gipvit.mil import init_params                        # noqa: E402

dev = torch.device("cuda", 0)
BAGS, TILES, F, LH, BATCH, LR, WD = 1000, 500, 384, 128, 8, 5e-4, 1e-4
REPEATS, COHORT = 7, 4096


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def window(run, width):
    """Fresh parameters, a warm-up epoch, one timed epoch -> (ms, the state)."""
    P = init_params(LH, 1, F, 0).to(dev)
    st = (P, torch.zeros_like(P), torch.zeros_like(P), torch.zeros(2, width, device=dev))
    run(st, 0)
    torch.cuda.synchronize()
    return timed(lambda: run(st, 1)), st


def main():
    argv = [a for a in sys.argv[1:]]
    other = argv.pop(argv.index("--parent-lib") + 1) if "--parent-lib" in argv else None
    argv = [a for a in argv if a != "--parent-lib"]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(BAGS * TILES, F, generator=g).to(dev)
    y = torch.zeros(BAGS, dtype=torch.int32, device=dev)
    time = torch.randint(1, 61, (BAGS,), generator=g).to(dev, torch.float32)
    event = (torch.rand(BAGS, generator=g) < 0.6).to(dev, torch.int32)
    ptr = torch.arange(0, BAGS * TILES + 1, TILES, dtype=torch.int32, device=dev)
    order = torch.from_numpy(epoch_permutations(BAGS, 2, 0).astype(np.int32)).to(dev)
    steps = -(-BAGS // BATCH)
    entries = [("gv_surv_train (4 launches per step)",
                lambda s, e: ops.surv_train(s[0], s[1], s[2], x, ptr, time, event, order[e], s[3][e], LH, BATCH, TILES, e * steps, LR, 1.0, WD), 2),
               ("gv_mil_train at C = 1 (3 launches per step)",
                lambda s, e: ops.mil_train(s[0], s[1], s[2], x, ptr, y, order[e], s[3][e], LH, 1, BATCH, TILES, e * steps, LR, 1.0, WD), 1)]
    if other:
        lib = ctypes.CDLL(other)
        for fn, st_ in ((lib.gv_surv_train, L.gv_surv_train_args), (lib.gv_mil_train, L.gv_mil_train_args)):
            fn.argtypes, fn.restype = [ctypes.POINTER(st_), ctypes.c_void_p], ctypes.c_int
        ws = ops._scratch("surv", dev, BATCH, TILES, LH, F)               # (the MIL workspace at C = 1 and four floats more)
        tail = (ws.data_ptr(), ws.numel(), x.stride(0), x.shape[0], F, LH)
        adam = lambda e: (BAGS, BAGS, BATCH, TILES, e * steps, LR, 1.0, WD, 0.9, 0.999, 1e-8)

        def parent_surv(s, e):
            a = L.gv_surv_train_args(s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), x.data_ptr(), ptr.data_ptr(), time.data_ptr(), event.data_ptr(),
                                     order[e].data_ptr(), s[3][e].data_ptr(), *tail, *adam(e))
            assert lib.gv_surv_train(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0

        def parent_mil(s, e):
            a = L.gv_mil_train_args(s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), x.data_ptr(), ptr.data_ptr(), y.data_ptr(), order[e].data_ptr(),
                                    s[3][e].data_ptr(), *tail, 1, *adam(e))
            assert lib.gv_mil_train(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        entries = [entries[0], ("gv_surv_train, the parent build", parent_surv, 2), entries[1], ("gv_mil_train at C = 1, the parent build", parent_mil, 1)]
    wins = [[] for _ in entries]
    for _ in range(REPEATS):                                               # the rows take their windows in turn
        for k, (_, run, width) in enumerate(entries):
            ms, st = window(run, width)
            wins[k].append(ms)
            if k == 0:
                loss = float(st[3][1, 0] / st[3][1, 1])
    rows = [(name, r) for (name, _, _), r in zip(entries, wins)]
    rng = np.random.Generator(np.random.PCG64(0))
    cr = torch.from_numpy((rng.integers(-64, 65, COHORT) / 16).astype(np.float32)).to(dev)
    ct = torch.from_numpy(rng.integers(1, 121, COHORT).astype(np.float32)).to(dev)
    ce = torch.from_numpy((rng.random(COHORT) < 0.6).astype(np.int32)).to(dev)
    ops.cox_eval(cr, ct, ce)
    torch.cuda.synchronize()
    cox = [timed(lambda: ops.cox_eval(cr, ct, ce)) for _ in range(REPEATS)]
    counts = ops.cox_eval(cr, ct, ce)[1].cpu().tolist()
    lines = [f"# tools/surv_bench.py on {torch.cuda.get_device_name(0)}; {BAGS} bags x {TILES} tiles, F = {F}, L = {LH}, batch {BATCH}: {steps} steps per "
             f"epoch; device events, {REPEATS} windows per row taken in turn, each after a warm-up epoch"]
    for name, runs in rows:
        k = statistics.median(runs)
        lines.append(f"one epoch, {name:<44} median {k:8.3f} ms   min {min(runs):8.3f}   max {max(runs):8.3f}   = {1e3 * k / steps:.1f} us per step   runs "
                     + " ".join(f"{v:.3f}" for v in runs))
    for new, old in ((0, 1), (2, 3)) if other else ():
        k, lo, hi = statistics.median(wins[new]), min(wins[old]), max(wins[old])
        lines.append(f"{entries[new][0].split()[0]}: this build's median {k:.3f} ms is {'inside' if lo <= k <= hi else 'OUTSIDE'} the parent's {lo:.3f} .. {hi:.3f} ms")
    lines.append(f"second-epoch Cox loss per event (random times): {loss:.6f}")
    lines.append(f"gv_cox_eval, n = {COHORT} (3 launches, {counts[0]} events, {counts[1]} comparable pairs)   {1e3 * statistics.median(cox):9.1f} us   runs "
                 + " ".join(f"{1e3 * v:.1f}" for v in cox))
    text = "\n".join(lines)
    print(text)
    if argv:
        with open(argv[0], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
