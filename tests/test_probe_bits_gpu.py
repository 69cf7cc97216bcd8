"""The ABMIL probes bit for bit: tests/traces/probe_outputs.json holds, per case of tests/test_mil_host.py and
tests/test_survival_host.py, the SHA-256 of the parameters, moments and loss sums after training and of one predict's outputs
(tools/probe_outputs_record.py; cases and calls: tests/probe_bits_cases.py).  The kernels use no atomics and fix the order of
every sum, so a build that computes what the recorded one computed reproduces every digest."""
import pytest

import probe_bits_cases as pb

ROWS = pb.load()
OUTPUTS = {"mil": ["params", "m", "v", "loss_sum", "prob", "loss", "attn", "score"], "surv": ["params", "m", "v", "loss_sum", "risk", "attn", "score"]}


def test_probe_outputs_cover_the_cases():
    """Four MIL and four survival cases, the ones the fixture was recorded from, every output digested (no GPU: the JSON alone)."""
    assert len(ROWS) == 8
    assert [{k: v for k, v in r.items() if k != "sha256"} for r in ROWS] == pb.cases()
    assert all(list(r["sha256"]) == OUTPUTS[r["probe"]] and all(len(h) == 64 for h in r["sha256"].values()) for r in ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=pb.row_id)
def test_probe_output_bits(dev, row):
    """The case's epochs and one predict, once: every buffer's recorded digest."""
    got = pb.digests(pb.run(row, dev))
    print(row["id"], got)
    assert got == row["sha256"]
