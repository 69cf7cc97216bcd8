"""How far apart two CLEAN runs of the same configuration lie: the gate of tests/test_poison_gpu.py (profiles/poison_spread.txt).

    python tools/poison_spread.py [--pairs 5] [--only SUBSTRING] > profiles/poison_spread.txt

For every configuration of tests/poison_cases.py: PAIRS pairs of fresh engines without GIPVIT_POISON, each run over the case's
three steps (or the extractor's call sequence); per recorded quantity the largest distance between the two runs of a pair --
|a - b| for a loss, ||a - b|| / ||b|| for an arena buffer, the centre or an extractor output.  One line per configuration, in the
form of the test's table.  An exact 0 (no f32 atomics on the path) makes the test assert torch.equal; elsewhere its gate is
4 x the figure printed here."""
import argparse
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch                                                            # noqa: E402

import poison_cases as pc                                               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    assert not os.environ.get("GIPVIT_POISON"), "the spread is clean against clean"
    dev = torch.device("cuda:0")
    print(f"# tools/poison_spread.py --pairs {args.pairs}: largest clean-vs-clean distance per configuration and quantity")
    for name in pc.CASES:
        if args.only not in name:
            continue
        worst, t0, saved = {}, time.time(), dict(os.environ)
        try:
            for _ in range(args.pairs):
                a = pc.run_case(name, dev, setenv=os.environ.__setitem__)
                b = pc.run_case(name, dev, setenv=os.environ.__setitem__)
                assert a.keys() == b.keys()
                for q in a:
                    worst[q] = max(worst.get(q, 0.0), pc.spread(a[q], b[q], q))
                del a, b
                gc.collect()
        finally:
            for k in set(os.environ) - set(saved):
                del os.environ[k]
        body = ", ".join(f'"{q}": {v:.3g}' for q, v in worst.items())
        print(f'    "{name}": {{{body}}},      # {(time.time() - t0) / (2 * args.pairs):.2f} s per run', flush=True)


if __name__ == "__main__":
    main()
