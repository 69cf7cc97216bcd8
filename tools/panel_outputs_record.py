"""Generator of tests/traces/panel_outputs.json: the kernel and the output bits of one call per panel_kernel instantiation
(tests/panel_bits_cases.py) from the library AS LOADED.  Needs the GPU.  Every row runs twice; nothing is written unless the two
runs agree digest for digest and the rows name as many distinct kernels as there are rows.

    [GIPVIT_LIB=path/to/libgipvit_hip.so] python tools/panel_outputs_record.py [--out PATH]

The fixture states what the kernels COMPUTE; it is regenerated only by a change that means to alter their arithmetic, from that
change's own build.  A change that must leave the arithmetic alone records it from the parent's library (GIPVIT_LIB) or not at all."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import panel_bits_cases as pb                                           # noqa: E402


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else pb.FIXTURE
    import torch
    from gipvit import _lib as L, ops as o
    assert "GIPVIT_CU_BUDGET" not in os.environ, "rows per workgroup are recorded with the default CU budget"
    dev = torch.device("cuda:0")
    rows, bad = pb.cases(), []
    for r in rows:
        runs = []
        for _ in range(2):
            trows, out = pb.run(o, L, r, dev)
            assert len(trows) == 1 and trows[0]["launches"] == 1, (r["id"], trows)
            runs.append((trows[0]["kernel"], pb.digests(out)))
        if runs[0] != runs[1]:
            bad.append(r["id"])
        r["kernel"], r["sha256"] = runs[0]
        print(r["id"], r["kernel"], " ".join("%s=%s" % (k, v[:12]) for k, v in r["sha256"].items()), flush=True)
    assert not bad, "rows whose two runs differ: %s" % bad
    names = {r["kernel"] for r in rows}
    assert len(names) == len(rows) and all(n.startswith("panel_kernel<") for n in names), "%d rows name %d kernels" % (len(rows), len(names))
    with open(out_path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("wrote", out_path, "from", L.LIB_PATH)


if __name__ == "__main__":
    main()
