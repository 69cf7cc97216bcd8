"""CPU: the kernel selection of csrc/linear_plan.h against tests/traces/linear_plans.json -- which kernel every pinned gv_linear /
gv_linear_dw_group / full-row call gets and how much scratch, as recorded from the library before the selection moved into the
header (tools/linear_plan_record.py).  The header is pure host C++: a stand-alone g++ program runs it, no library, no GPU."""
import json
import os
import subprocess
import sys

import pytest

import linear_plan_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data():
    return lc.load()


def test_fixture_holds_the_cases(data):
    """Every row has its kernel (GPU rows) and its bytes for both budgets; the ViT-S block's 50-MB slab is among them."""
    for r in data["linear"] + data["group"]:
        assert set(r["bytes"]) == set(lc.BUDGETS) and all(b >= 0 for b in r["bytes"].values()), r["id"]
        assert ("kernel" in r) == bool(r.get("gpu", 1)), r["id"]
    assert all("kernel" in r for r in data["fullrow"])
    by_id = {r["id"]: r for r in data["linear"] + data["group"]}
    assert by_id["block_D384_T44160"]["bytes"]["256"] == 49545216 and by_id["vit_s_fc1_dw"]["bytes"]["256"] == 49545216
    assert len({r["id"] for k in data for r in data[k]}) == sum(len(data[k]) for k in data)


def test_plan_header_reproduces_every_fixture_row(data, tmp_path):
    """tests/linear_plan_main.cc (g++ -std=c++17, linear_plan.h and the C header only) plans every case with CU budgets 256 and 248:
    the kernel name (budget 256, the one the recording ran with) and the scratch bytes (both budgets) of every row."""
    exe, cases = str(tmp_path / "linear_plan_main"), str(tmp_path / "cases.txt")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "linear_plan_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(cases, "w") as f:
        f.write("\n".join(lc.case_lines(data)) + "\n")
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = data["linear"] + data["group"] + data["fullrow"]
    out = [l.split("\t") for l in r.stdout.splitlines()]
    assert len(out) == 2 * len(rows)
    for k, budget in enumerate(lc.BUDGETS):
        for row, (b, name, nbytes) in zip(rows, out[k * len(rows):(k + 1) * len(rows)]):
            assert b == budget
            if budget == "256" and "kernel" in row:
                assert name == row["kernel"], (row["id"], name, row["kernel"])
            if "bytes" in row:
                assert int(nbytes) == row["bytes"][budget], (row["id"], budget, int(nbytes), row["bytes"][budget])


@pytest.mark.parametrize("budget", lc.BUDGETS)
def test_workspace_query_of_the_library_matches_the_fixture(data, budget):
    """gv_workspace_bytes of the built library, in a process of its own per CU budget (the budget is read once, when the library
    first needs it): the fixture's bytes."""
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import linear_plan_cases as lc; from gipvit import _lib; "
            "print(json.dumps(lc.query_bytes(_lib, lc.load())))" % (ROOT, os.path.join(ROOT, "tests")))
    env = {k: v for k, v in os.environ.items() if k != "GIPVIT_CU_BUDGET"}
    if budget != "256":
        env["GIPVIT_CU_BUDGET"] = budget
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    rows = data["linear"] + data["group"]
    assert len(got) == len(rows)
    for row, b in zip(rows, got):
        assert b == row["bytes"][budget], (row["id"], budget, b, row["bytes"][budget])
