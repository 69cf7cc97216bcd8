"""The full-row kernels bit for bit: tests/traces/panel_outputs.json holds, for one call per panel_kernel instantiation, the kernel's
timing-row name and the SHA-256 of every output buffer (tools/panel_outputs_record.py; cases and operands: tests/panel_bits_cases.py).
The kernels use no atomics, so a build that computes what the recorded one computed reproduces every digest."""
import pytest

import panel_bits_cases as pb

ROWS = pb.load()


def test_panel_outputs_cover_every_instantiation():
    """52 rows, 52 distinct panel_kernel instantiations, the cases the fixture was recorded from (no GPU: the JSON alone)."""
    assert len(ROWS) == 52
    kernels = {r["kernel"] for r in ROWS}
    assert len(kernels) == 52 and all(k.startswith("panel_kernel<") and k.endswith(">") for k in kernels)
    assert [{k: v for k, v in r.items() if k not in ("kernel", "sha256")} for r in ROWS] == pb.cases()
    assert all(r["sha256"] and all(len(h) == 64 for h in r["sha256"].values()) for r in ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=pb.row_id)
def test_panel_kernel_and_output_bits(dev, row):
    """The call, once, under linear_timing: the kernel the fixture names, and every output buffer's recorded digest."""
    from gipvit import _lib as L, ops as o
    trows, out = pb.run(o, L, row, dev)
    print(row["id"], [(t["kernel"], t["launches"]) for t in trows])
    assert [(t["kernel"], t["launches"]) for t in trows] == [(row["kernel"], 1)]
    got = pb.digests(out)
    print(got)
    assert got == row["sha256"]
