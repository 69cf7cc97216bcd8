"""GPU: the draw-stream golden of the training driver.  Two short jobs, a DINO one (random crops, view augmentation, stain jitter,
iBOT masks, stochastic depth) and a supervised one (mixup, erasing, dropout, stochastic depth), leave every host draw stream at a
position that depends on the flags alone: which samplers are built, on which per-rank seed, and how often each is drawn from.
tests/golden/driver_streams.json holds the ``host_rng*`` / ``drop_path_rng`` entries of their checkpoints as the driver wrote them
before its ``main`` was cut into stages; they are host generator states and must be equal exactly.  (check_supported refuses
--drop next to --ibot-weight, so the dropout stream is drawn by the supervised job.)  The weights are not compared: float atomics
make the device arithmetic not bitwise."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = {
    "dino": ["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--out-dim", "1024", "--batches-per-epoch", "3", "--epochs", "1",
             "--random-crops", "--view-augment", "--stain-jitter", "0.05", "--ibot-weight", "1", "--drop-path", "0.1", "--seed", "7", "--no-validate"],
    "supervised": ["--model", "vit_tiny", "--dataset", "synthetic", "--num-classes", "2", "--img-size", "64", "--tile-size", "64", "-b", "2",
                   "--batches-per-epoch", "3", "--epochs", "1", "--mixup", "0.2", "--reprob", "0.25", "--drop", "0.1", "--drop-path", "0.1",
                   "--seed", "7", "--no-validate"],
}


def test_draw_streams_end_where_they_always_did(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import train
    with open(os.path.join(ROOT, "tests", "golden", "driver_streams.json")) as f:
        golden = json.load(f)
    assert {k: v["flags"] for k, v in golden.items()} == JOBS
    stream = torch.cuda.current_stream()        # train.main leaves its high-priority stream current: put the caller's back
    try:
        for name, flags in JOBS.items():
            assert train.main(flags + ["--output", str(tmp_path), "--experiment", name]) == 0
            ck = torch.load(tmp_path / name / "last.pth.tar", weights_only=True)
            got = {k: ck[k] for k in ck if k.startswith("host_rng") or k == "drop_path_rng"}
            want = golden[name]["entries"]
            assert sorted(got) == sorted(want) == ["drop_path_rng", "host_rng", "host_rng_ranks"]
            for k in want:
                assert got[k] == want[k], (name, k)
    finally:
        torch.cuda.set_stream(stream)
