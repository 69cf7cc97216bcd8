"""CPU: csrc/attn_plan.h -- the length classes, per-class workgroup shapes, LDS sizes and launch geometry of the attention entry
points -- against tests/traces/attention_plans.json, and the four attention limits of include/gipvit.h against their copies.

The fixture was written from the formulas of attention.hip / attention_stream.hip as they stood BEFORE the header existed (each
launcher's own expressions, evaluated on the host) and is not regenerated from the header.  The header is pure host C++: a
stand-alone g++ program (tests/attn_plan_main.cc) runs it, no library, no GPU."""
import json
import os
import re
import subprocess

from test_attention_probes_host import NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gipmed-project-self-supervised-vit_amd")
with open(os.path.join(ROOT, "tests", "traces", "attention_plans.json")) as _f:
    FIX = json.load(_f)


def test_fixture_holds_the_parents_tables_and_every_edge():
    assert [(r["nkt"], r["nw"], r["pairs"], r["lds"], r["occ"]) for r in FIX["fwd_cfg"]] == [
        (2, 4, 4, 32768, 1), (4, 4, 2, 32768, 1), (8, 4, 1, 32768, 1), (14, 8, 1, 57344, 4), (18, 8, 1, 73728, 2)]
    assert [(r["nkt"], r["kt"], r["nw"], r["pairs"], r["lds"], r["occ"]) for r in FIX["bwd_cfg"]] == [
        (2, 2, 4, 4, 58368, 2), (4, 1, 4, 1, 29184, 2), (8, 2, 4, 1, 66560, 2), (14, 2, 7, 1, 145152, 1), (18, 2, 9, 1, 149760, 1)]
    for kind in ("fwd", "bwd"):
        assert tuple(r["N"] for r in FIX[kind]) == NS and all(r["pairs"] == 9 for r in FIX[kind])
    assert {(r["N"], r["q_rows"]) for r in FIX["probs"]} == {(N, q) for N in NS for q in (1, 16, 17, N) if q <= N}
    for r in FIX["probs"]:
        want = (3, 256, 0) if r["q_rows"] <= 16 else (9, min((r["q_rows"] + 15) // 16, 4) * 64, r["nkt"] * 2048)
        assert (r["kernel"] == "row") == (r["q_rows"] <= 16) and (r["grid"], r["block"], r["lds"]) == want, r
    fused = {tuple(r["N"]): r for r in FIX["varlen"] if r["long"] >= 0}
    assert {k: r["long"] for k, r in fused.items()} == {(129, 33): 0, (224, 64): 0, (64, 224): 1, (33, 129): 1}
    assert all((r["grid"], r["block"], r["lds"]) == (9 + 3, 512, 65536) for r in fused.values())
    alone = {tuple(r["N"]) for r in FIX["varlen"] if r["long"] < 0}
    assert {(128, 64), (225, 64), (224, 32), (224, 65)} <= alone and any(len(k) == 3 for k in alone)
    assert {(r["N"], r["q_limit"]) for r in FIX["stream"]} == {(N, q) for N in (289, 1025, 1040) for q in (0, 1, 129)}
    for r in FIX["stream"]:
        rows = min(r["q_limit"] or r["N"], r["N"])
        assert (r["grid"], r["block"], r["lds"]) == (9 * ((rows + 127) // 128), 256, 32768), r


def _case_lines():
    """(case line of tests/attn_plan_main.cc, the integers it must print) per fixture row"""
    out = []
    for r in FIX["fwd"]:
        out.append((f"F {r['N']} {r['pairs']}", [r["nkt"], r["grid"], r["block"], r["lds"]]))
    for r in FIX["bwd"]:
        out.append((f"B {r['N']} {r['pairs']}", [r["nkt"], r["kt"], r["grid"], r["block"], r["lds"]]))
    for r in FIX["probs"]:
        out.append((f"P {r['N']} {r['pairs']} {r['q_rows']}", [int(r["kernel"] == "row"), r["nkt"], r["grid"], r["block"], r["lds"]]))
    for r in FIX["stream"]:
        out.append((f"S {r['N']} {r['pairs']} {r['q_limit']}", [r["query_blocks"], r["grid"], r["block"], r["lds"]]))
    for r in FIX["varlen"]:
        want = [r["long"]] + ([r["grid"], r["long_blocks"], r["block"], r["lds"]] if r["long"] >= 0 else [])
        out.append((f"V {r['pairs']} {len(r['N'])} " + " ".join(map(str, r["N"])), want))
    return out


def test_plan_header_reproduces_every_fixture_row(tmp_path):
    """tests/attn_plan_main.cc (g++ -std=c++17 -Wall -Werror, attn_plan.h and the C header only): the per-class tables, then the
    class and the launch of every forward / backward / probs / varlen / streaming row."""
    exe, cases = str(tmp_path / "attn_plan_main"), str(tmp_path / "cases.txt")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "attn_plan_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _case_lines()
    with open(cases, "w") as f:
        f.write("C\n" + "\n".join(l for l, _ in lines) + "\n")
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [l.split() for l in r.stdout.splitlines()]
    cfg = {k: [list(map(int, l[1:])) for l in out if l[0] == k] for k in ("fwd_cfg", "bwd_cfg")}
    assert cfg["fwd_cfg"] == [[r[k] for k in ("nkt", "nw", "pairs", "lds", "occ")] for r in FIX["fwd_cfg"]]
    assert cfg["bwd_cfg"] == [[r[k] for k in ("nkt", "kt", "nw", "pairs", "lds", "occ")] for r in FIX["bwd_cfg"]]
    rows = out[len(cfg["fwd_cfg"]) + len(cfg["bwd_cfg"]):]
    assert len(rows) == len(lines)
    for (line, want), got in zip(lines, rows):
        assert list(map(int, got)) == want, (line, got, want)


def _macros():
    hdr = open(os.path.join(ROOT, "include", "gipvit.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (GV_ATTN_(?:F32_MAX_N|MAX_N|STREAM_MAX_N|STREAM_QBLOCK))\s+(\d+)\b", hdr, re.M)}


def test_the_limits_have_one_source():
    """include/gipvit.h defines the four limits; _lib mirrors them and train.py keeps three of its own (it checks sizes before the
    library format is chosen and _lib imported).  Nothing else under the package or csrc/ spells one as a number."""
    from gipvit import _lib
    import train
    m = _macros()
    assert m == dict(GV_ATTN_MAX_N=288, GV_ATTN_F32_MAX_N=260, GV_ATTN_STREAM_MAX_N=1040, GV_ATTN_STREAM_QBLOCK=128)
    assert {k: getattr(_lib, k) for k in m} == m
    assert (train.ATTN_TRAIN_MAX_TOKENS, train.ATTN_F32_MAX_TOKENS, train.ATTN_STREAM_MAX_TOKENS) == (
        m["GV_ATTN_MAX_N"], m["GV_ATTN_F32_MAX_N"], m["GV_ATTN_STREAM_MAX_N"])
    files = [os.path.join(PKG, f) for f in os.listdir(PKG) if f.endswith(".py")]
    files += [os.path.join(PKG, "csrc", f) for f in os.listdir(os.path.join(PKG, "csrc")) if f.endswith((".hip", ".h"))]
    # a bare 288 / 260 / 1040: not part of a longer number or name, of a line range ("1037-1040") or of "288-GB"
    number = re.compile(r"(?<![\w.-])(288|260|1040)(?![\w.]|-GB)")
    spelled = re.compile(r"<= (288|260)\b|AMAXN = |(?<![A-Z_])F32_ATTN_MAX_N")
    hits = []
    for path in files:
        for n, line in enumerate(open(path), 1):
            if os.path.basename(path) == "_lib.py" and line.startswith("GV_ATTN_MAX_N, "):      # the mirror itself
                continue
            if number.search(line) or spelled.search(line):
                hits.append(f"{os.path.relpath(path, ROOT)}:{n}: {line.strip()[:120]}")
    assert not hits, "\n".join(hits)
    hdr = open(os.path.join(ROOT, "include", "gipvit.h")).read()
    assert not re.search(r"<= (288|260)\b", hdr)
