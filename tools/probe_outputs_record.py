"""Generator of tests/traces/probe_outputs.json: the output bits of the ABMIL probes' cases (tests/probe_bits_cases.py: training,
then one predict, per case of tests/test_mil_host.py and tests/test_survival_host.py) from the library AS LOADED.  Needs the GPU.
Every case runs twice; nothing is written unless the two runs agree digest for digest.

    [GIPVIT_LIB=path/to/libgipvit_hip.so] python tools/probe_outputs_record.py [--out PATH]

The fixture states what gv_mil_* / gv_surv_* COMPUTE; it is regenerated only by a change that means to alter their arithmetic,
from that change's own build.  A change that must leave the arithmetic alone records it from the parent's library (GIPVIT_LIB)
or not at all."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import probe_bits_cases as pb                                           # noqa: E402


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else pb.FIXTURE
    import torch
    from gipvit import _lib as L
    dev = torch.device("cuda:0")
    rows, bad = pb.cases(), []
    for r in rows:
        runs = [pb.digests(pb.run(r, dev)) for _ in range(2)]
        if runs[0] != runs[1]:
            bad.append(r["id"])
        r["sha256"] = runs[0]
        print(r["id"], " ".join("%s=%s" % (k, v[:12]) for k, v in r["sha256"].items()), flush=True)
    assert not bad, "cases whose two runs differ: %s" % bad
    with open(out_path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("wrote", out_path, "from", L.LIB_PATH)


if __name__ == "__main__":
    main()
