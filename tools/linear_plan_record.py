"""Generator of tests/traces/linear_plans.json: which kernel and how much scratch every pinned gv_linear / gv_linear_dw_group /
full-row call gets from the library AS BUILT.  Needs the GPU for `kernel` (the single timing-row name of the call between
linear_timing(True) and linear_timing(False)); `bytes` is gv_workspace_bytes, taken in a fresh process per CU budget
(GIPVIT_CU_BUDGET unset and 248) before the library loads.

    python tools/linear_plan_record.py [--out PATH]           # writes the fixture (default: tests/traces/linear_plans.json)

The fixture states what the kernel selection IS; it is regenerated only by a change that means to alter the selection."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linear_plan_cases as lc                                          # noqa: E402

B, G, R, DG, ACC, SP = lc.BIAS, lc.GELU, lc.RESID, lc.DGELU, lc.ACCUM, lc.SAVE_PRE


def lin(id_, M, N, K, ta, tb, c_f32, epi, colsum_a=0, in_place=0, ws=1):
    return dict(id=id_, M=M, N=N, K=K, ta=ta, tb=tb, c_f32=c_f32, epi=epi, colsum_a=colsum_a, in_place=in_place, ws=ws)


def cases():
    linear = [
        lin("dw8_k_floor", 1536, 384, 2048, 1, 1, 1, ACC),
        lin("under_k_floor_tile_slab", 1536, 384, 2016, 1, 1, 1, ACC),
        # 384 x 1536 and 384 x 1152 tile into 128 x 384 pieces as they stand: the normal orientation, whatever N / 128 is
        lin("dw8_384x1536", 384, 1536, 4096, 1, 1, 1, ACC),
        lin("dw8_384x1152_colsum", 384, 1152, 4096, 1, 1, 1, ACC, colsum_a=1),
        lin("dw8_384x1536_colsum", 384, 1536, 4096, 1, 1, 1, ACC, colsum_a=1),
        # N % 384 != 0, M % 384 == 0: the swapped orientation; with colsum_a it needs N / 128 >= 12
        lin("dw8_swapped", 384, 1664, 4096, 1, 1, 1, ACC),
        lin("dw8_swapped_colsum_13", 384, 1664, 4096, 1, 1, 1, ACC, colsum_a=1),
        lin("dw8_swapped_colsum_11_refused", 384, 1408, 4096, 1, 1, 1, ACC, colsum_a=1),
        lin("dw8_256_tiles", 2048, 6144, 2048, 1, 1, 1, ACC),
        lin("tiles_272_no_split", 2176, 6144, 2048, 1, 1, 1, ACC),
        lin("vit_s_fc1_dw", 1536, 384, 44160, 1, 1, 1, ACC),
        lin("small_dw_deep_192", 192, 192, 8192, 1, 1, 1, ACC),
        lin("small_dw_deep_256", 256, 256, 8192, 1, 1, 1, ACC),
        lin("tn_e0", 384, 128, 256, 1, 1, 1, 0),
        lin("wide_m_floor", 2048, 384, 128, 0, 0, 0, B),
        lin("under_m_floor_tile", 2040, 384, 128, 0, 0, 0, B),
        lin("k_not_128_tile", 2048, 384, 192, 0, 0, 0, B),
        lin("wide_bias_gelu_save", 4099, 1536, 384, 0, 0, 0, B | G | SP),
        lin("wide_dgelu", 3000, 1536, 384, 0, 1, 0, DG),
        lin("wide_f32_bias_resid", 47000, 768, 128, 0, 0, 1, B | R),
        lin("wide_f32_in_place_refused", 47000, 768, 128, 0, 0, 1, B | R, in_place=1),
        lin("few_row_split_640", 640, 2048, 2048, 0, 0, 0, B | G),
        lin("few_row_split_128", 128, 256, 2048, 0, 0, 0, B),
        lin("k_steps_15_no_split", 128, 256, 960, 0, 0, 0, B),
        lin("tiles_96", 1024, 1536, 1024, 0, 0, 0, B),
        lin("tiles_104_no_split", 1024, 1664, 1024, 0, 0, 0, B),
        lin("few_row_f32_out", 640, 384, 1536, 0, 0, 1, B | R),
        lin("head_dx", 640, 256, 65536, 0, 1, 1, ACC),
        lin("nn_accum", 640, 256, 4096, 0, 0, 1, ACC),
        lin("generic_n_not_8", 100, 72, 192, 0, 0, 0, B),
    ]
    # the ACCUM rows once more without a workspace: the atomic path (bytes stays the query's "as if offered")
    linear += [dict(r, id=r["id"] + "_no_ws", ws=0) for r in linear if r["epi"] == ACC]
    group = []
    for D in (192, 384, 768):
        for T in (1500, 2048, 3000, 8192, 44160):
            group.append(dict(id="block_D%d_T%d" % (D, T), D=D, T=T, probs=[[D, 4 * D], [4 * D, D], [D, D], [3 * D, D]], gpu=int(T <= 8192)))
            group.append(dict(id="cls_tail_D%d_T%d" % (D, T), D=D, T=T, probs=[[3 * D, D]], gpu=int(T <= 8192)))
    fullrow = [dict(id="%s_M%d_K%d" % (op, M, K), op=op, M=M, K=K)
               for op in ("ln_fwd", "ln_bwd", "mlp_ln_fwd") for M in (64, 1380, 4096, 4097, 44160) for K in (384, 192)]
    return dict(linear=linear, group=group, fullrow=fullrow)


def bytes_worker():
    """Fresh process, the budget already in the environment: the scratch query of every row."""
    from gipvit import _lib as L
    print(json.dumps(lc.query_bytes(L, json.loads(sys.stdin.read()))))


def main():
    data = cases()
    rows = data["linear"] + data["group"]
    for r in rows:
        r["bytes"] = {}
    for budget in lc.BUDGETS:
        env = {k: v for k, v in os.environ.items() if k != "GIPVIT_CU_BUDGET"}
        if budget != "256":
            env["GIPVIT_CU_BUDGET"] = budget
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--bytes"], input=json.dumps(data), env=env, capture_output=True, text=True, check=True)
        for r, b in zip(rows, json.loads(out.stdout.strip().splitlines()[-1])):
            r["bytes"][budget] = b
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else lc.FIXTURE
    import torch
    from gipvit import _lib as L, ops as o
    assert "GIPVIT_CU_BUDGET" not in os.environ, "kernel names are recorded with the default CU budget"
    dev = torch.device("cuda:0")
    ws = torch.empty(L.lib.gv_linear_workspace_bytes() // 4, dtype=torch.float32, device=dev)
    bad = []
    for kind in ("linear", "group", "fullrow"):
        for r in data[kind]:
            if not r.get("gpu", 1):
                continue
            trows, checks = lc.run_row(o, L, kind, r, dev, ws)
            assert len(trows) == 1 and trows[0]["launches"] == 1, (r["id"], trows)
            bad += [(r["id"], what) for what, got, want in checks if not torch.equal(got, want)]
            r["kernel"] = trows[0]["kernel"]
            print(r["id"], r["kernel"], r.get("bytes", ""), flush=True)
    with open(out_path, "w") as f:
        f.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in data[k])) for k in ("linear", "group", "fullrow")) + "\n}\n")
    print("wrote", out_path)
    assert not bad, "results that are not exact: %s" % bad


if __name__ == "__main__":
    bytes_worker() if "--bytes" in sys.argv else main()
