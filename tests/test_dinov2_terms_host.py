"""CPU: Sinkhorn-Knopp centring and KoLeo -- the specification (tests/dinov2_terms_cases.py) against DINOv2's literal iteration and
torch.autograd, the conditions on the GPU cases' fixed inputs, the ABI's refusals without a GPU, the driver's flags, and where the
new launches sit in the engine's launch sequence (tests/launch_trace.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dinov2_terms_cases as C
import launch_trace as LT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sinkhorn_shift", "sinkhorn_cols", "sinkhorn_rows", "sinkhorn_finish", "koleo_fwd", "koleo_bwd")


# ---- the specification
@pytest.mark.parametrize("R,K,tau", [(8, 256, 0.04), (128, 4096, 0.04), (128, 4096, 0.07)])
def test_log_domain_sinkhorn_is_dinov2s_iteration(R, K, tau):
    T = C.sinkhorn_logits(R, K)
    for n in (1, 3):
        a, _ = C.sinkhorn_log(T, tau, n)
        Q, P = C.sinkhorn_literal(T, tau, n), C.sinkhorn_probs(T, tau, a)
        rel = float((np.abs(P - Q) / Q).max())
        print(f"R={R} K={K} tau={tau} n={n}: max relative difference of Q {rel:.2e}")
        assert rel < 1e-12
        assert np.allclose(Q.sum(1), 1.0, rtol=1e-12)


def test_two_ranks_adding_column_sums_give_one_process_result():
    T = C.sinkhorn_logits(128, 4096)
    one, _ = C.sinkhorn_log(T, 0.04, 3)
    two, _ = C.sinkhorn_log(T, 0.04, 3, ranks=2)
    assert float(np.abs(one - two).max()) < 1e-12
    # the literal iteration with world = 2 on half the rows is NOT what a rank computes alone: the sums must span the ranks
    alone, _ = C.sinkhorn_log(T[:64], 0.04, 3)
    assert float(np.abs(C.gauge(alone) - C.gauge(one)).max()) > 1e-3


@pytest.mark.parametrize("G,B,D", C.KOLEO_CASES[:4])
def test_koleo_gradient_formula_against_autograd(G, B, D):
    x = C.koleo_inputs(G, B, D)[:G * B]
    f = C.koleo(x, G, B)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    total = 0.0
    for g in range(G):
        xc = xt[g * B:(g + 1) * B]
        y = xc / xc.norm(dim=1, keepdim=True).clamp_min(C.EPS)
        I = torch.from_numpy(f["nn"][g * B:(g + 1) * B])
        d = (y - y[I] + C.EPS).norm(dim=1)
        total = total + (-torch.log(d + C.EPS)).mean()
    total.backward()
    assert abs(float(total.detach()) - float(f["koleo"])) <= 1e-12 * abs(float(total.detach()))
    gx = C.koleo_grad(x, G, B, f["nn"])
    rel = float(np.abs(gx - xt.grad.numpy()).max() / np.abs(xt.grad.numpy()).max())
    print(f"{(G, B, D)}: gradient formula vs autograd, relative {rel:.2e}")
    assert rel < 1e-10
    if B > 2:
        assert len(set(f["nn"][:B].tolist())) < B        # several rows share a neighbour: the gather has something to add up


def test_koleo_lowest_index_wins_a_tie():
    x = np.zeros((3, 64), np.float32)
    x[0, 0] = x[1, 1] = x[2, 1] = 1.0                    # rows 1 and 2 are equal: row 0 sees two dots of 0
    assert C.koleo(x, 1, 3)["nn"].tolist() == [1, 2, 1]


# ---- conditions on the fixed inputs of the GPU cases
@pytest.mark.parametrize("G,B,D", C.KOLEO_CASES)
def test_koleo_cases_have_a_clear_neighbour(G, B, D):
    r = C.koleo_reference(G, B, D)
    gap, dmin = float(r["fwd"]["gap"].min()), float(r["fwd"]["d"].min())
    print(f"{(G, B, D)}: least best-minus-runner-up gap {gap:.3e}, least distance {dmin:.3f}, koleo {float(r['fwd']['koleo']):.4f}, "
          f"bounds koleo {r['koleo_bound']:.2e} gx {r['gx_bound']:.2e}")
    assert gap >= C.KOLEO_GAP > 10 * 768 * 2.0 ** -24 and dmin > 0.05
    assert np.array_equal(C.bf16_round(r["x"]), r["x"])


@pytest.mark.parametrize("R,K", C.SINKHORN_CASES)
def test_sinkhorn_cases_never_reach_the_clamp(R, K):
    for tau in C.TAUS:
        c64, bnd, s_min = C.sinkhorn_reference(R, K, tau, 3)
        print(f"{(R, K)} tau={tau}: min s_k {s_min:.3e}, bound on the gauged centre {bnd:.2e}")
        assert s_min >= 1e-30 and np.isfinite(c64).all() and 1e-6 <= bnd < 1e-4


# ---- the ABI without a GPU
def _lib():
    from gipvit import _lib as L
    return L


def test_both_builds_export_the_entry_points():
    L = _lib()
    entries = ["gv_sinkhorn_shift", "gv_sinkhorn_cols", "gv_sinkhorn_rows", "gv_sinkhorn_finish", "gv_koleo_fwd", "gv_koleo_bwd", "gv_koleo_fwd_f32",
               "gv_koleo_bwd_f32"]
    plain = ["gv_koleo_workspace_bytes", "gv_sinkhorn_workspace_bytes"]
    assert all(hasattr(L.lib, n) for n in entries + plain) and L.lib.gv_version() == 9
    assert all(L.ENTRY_POINTS[n] is (L.gv_sinkhorn_args if "sinkhorn" in n else L.gv_koleo_args) for n in entries)
    assert all(n in L.PLAIN_SYMBOLS for n in plain)
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); missing = [n for n in sys.argv[2:] if not hasattr(l, n)]; assert not missing, missing; "
            "l.gv_koleo_workspace_bytes.restype = ctypes.c_int64; assert l.gv_koleo_workspace_bytes(2, 64, 384) > 0 and l.gv_version() == 9")
    for lib in ("libgipvit_hip.so", "libgipvit_hip_f16.so"):
        r = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(L.LIB_PATH), lib)] + entries + plain, capture_output=True, text=True)
        assert r.returncode == 0, (lib, r.stderr[-600:])


def test_struct_layouts_match_gcc(tmp_path):
    L = _lib()
    structs = [L.gv_sinkhorn_args, L.gv_koleo_args]
    lines = []
    for st in structs:
        lines.append(f'printf("{st.__name__} %zu\\n", sizeof({st.__name__}));')
        lines += [f'printf("{st.__name__}.{f} %zu\\n", offsetof({st.__name__}, {f}));' for f, _ in st._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gipvit.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for st in structs:
        assert int(out[st.__name__]) == ctypes.sizeof(st), st.__name__
        for f, _ in st._fields_:
            assert int(out[f"{st.__name__}.{f}"]) == getattr(st, f).offset, (st.__name__, f)


def test_koleo_abi_errors():
    L = _lib()
    ok = dict(feats=4096, dfeats=8192, workspace=16384, workspace_bytes=1 << 40, nn=20480, koleo=24576, loss_scale=None, ld=384, G=2, B=64, D=384,
              weight=0.1)      # never dereferenced

    def err():
        return L.lib.gv_last_error().decode()
    for name in ("gv_koleo_fwd", "gv_koleo_bwd", "gv_koleo_fwd_f32", "gv_koleo_bwd_f32"):
        fn = getattr(L.lib, name)
        rc = lambda **kw: fn(ctypes.byref(L.gv_koleo_args(**dict(ok, **kw))), None)
        assert fn(None, None) == -3
        assert rc(workspace=None) == -3 and rc(nn=None) == -3 and "null" in err()
        assert rc(**{"dfeats" if "bwd" in name else "feats": None}) == -3
        for B in (1, 0, 1025):
            assert rc(B=B) == -1 and "2 <= B <= 1024" in err(), B
        for D in (100, 0, 832, 32):
            assert rc(D=D, ld=1024) == -1 and "multiple of 64" in err(), D
        for G in (5, 0):
            assert rc(G=G) == -1 and "1 <= G <= 4" in err(), G
        assert rc(ld=380) == -1 and "ld >= D" in err()
        need = L.lib.gv_koleo_workspace_bytes(2, 64, 384)
        assert need >= 2 * 64 * (384 + 3) * 4
        assert rc(workspace_bytes=need - 1) == -1 and str(need) in err() and "workspace" in err()
        assert rc(workspace=16384 + 4) == -2
        if "bwd" in name:
            for w in (-0.1, float("nan"), float("inf")):
                assert rc(weight=w) == -1 and "weight" in err(), w
    for bad in ((5, 64, 384), (2, 1, 384), (2, 64, 100), (0, 64, 384), (2, 1025, 384), (2, 64, 832)):
        assert L.lib.gv_koleo_workspace_bytes(*bad) == -1 and err().startswith("gv_koleo_workspace_bytes"), bad


def test_sinkhorn_abi_errors():
    L = _lib()
    ok = dict(teacher=4096, shift=8192, a=12288, b=16384, colsum=20480, sk_center=24576, workspace=28672, workspace_bytes=1 << 40, hyper=None,
              R=128, K=4096, first=1, teacher_temp=0.04)

    def err():
        return L.lib.gv_last_error().decode()
    for name in ("gv_sinkhorn_shift", "gv_sinkhorn_cols", "gv_sinkhorn_rows", "gv_sinkhorn_finish"):
        fn = getattr(L.lib, name)
        rc = lambda **kw: fn(ctypes.byref(L.gv_sinkhorn_args(**dict(ok, **kw))), None)
        assert fn(None, None) == -3
        for p in ("teacher", "shift", "a", "b", "colsum", "workspace"):
            assert rc(**{p: None}) == -3 and "null" in err(), p
        if name != "gv_sinkhorn_finish":                   # (sk_center may be NULL there: such a call would pass its checks and launch)
            continue
        assert rc(sk_center=None) == -3 and "sk_center" in err()
        for K in (4098, 0, 2, -4):
            assert rc(K=K) == -1 and "multiple of 4" in err(), K
        for R in (0, 65536):
            assert rc(R=R) == -1, R
        assert rc(teacher_temp=0.0) == -1 and "temperature" in err()
        assert rc(a=12288 + 4) == -2 and rc(teacher=4096 + 8) == -2 and "16-byte" in err()
        need = L.lib.gv_sinkhorn_workspace_bytes(128, 4096)
        assert need >= 128 * 4096 * 4 and rc(workspace_bytes=need - 1) == -1 and str(need) in err()
    for name in ("gv_sinkhorn_shift", "gv_sinkhorn_cols", "gv_sinkhorn_rows"):
        fn = getattr(L.lib, name)
        assert fn(ctypes.byref(L.gv_sinkhorn_args(**dict(ok, K=4098))), None) == -1
        assert fn(ctypes.byref(L.gv_sinkhorn_args(**dict(ok, workspace_bytes=16))), None) == -1
    assert L.lib.gv_sinkhorn_workspace_bytes(128, 65536) == 16 * 65536 * 4          # 64 column tiles x 16 row slices of 8 rows
    assert L.lib.gv_sinkhorn_workspace_bytes(128, 4098) == -1 and err().startswith("gv_sinkhorn_workspace_bytes")


# ---- the driver
def _train():
    sys.path.insert(0, ROOT)
    import train
    return train


def test_flags_reach_the_engine():
    train = _train()
    base, _ = train.parse_args(["--model", "vit_tiny", "--dino"])
    assert train.dino_loss_options(base) == dict(centering="center", sinkhorn_iters=3, koleo_weight=0.0)
    assert train.check_supported(base, lambda m: None) is None
    on, _ = train.parse_args(["--model", "vit_tiny", "--dino", "--centering", "sinkhorn_knopp", "--sinkhorn-iters", "5", "--koleo-weight", "0.1",
                              "--batch-size", "2"])
    assert train.check_supported(on, lambda m: None) is None
    kw = train.dino_loss_options(on)
    assert kw == dict(centering="sinkhorn_knopp", sinkhorn_iters=5, koleo_weight=0.1)
    from gipvit.engine import DinoEngine
    eng = DinoEngine(arch="vit_tiny", img_size=224, out_dim=256, batch=2, device="cpu", **kw)
    assert (eng.centering, eng.sinkhorn_iters, eng.koleo_weight) == ("sinkhorn_knopp", 5, 0.1)
    assert eng.sk_center.shape == (256,) and eng.koleo.shape == (1,) and eng.koleo_nn.shape == (4,) and eng.koleo_nn.dtype == torch.int32
    off = DinoEngine(arch="vit_tiny", img_size=224, out_dim=256, batch=1, device="cpu")
    assert off.sk_center is None and off.koleo is None and off.koleo_nn is None
    # (that train.main builds its engine with these, and the log line: tests/test_dinov2_terms_gpu.py::test_driver_hands_the_options_to_the_engine)


@pytest.mark.parametrize("flags,word", [
    (["--centering", "sinkhorn_knopp"], "--dino"),
    (["--koleo-weight", "0.1"], "--dino"),
    (["--dino", "--koleo-weight", "-0.1"], "--koleo-weight"),
    (["--dino", "--koleo-weight", "nan"], "--koleo-weight"),
    (["--dino", "--koleo-weight", "inf"], "--koleo-weight"),
    (["--dino", "--centering", "sinkhorn_knopp", "--sinkhorn-iters", "0"], "--sinkhorn-iters"),
    (["--dino", "--centering", "sinkhorn_knopp", "--sinkhorn-iters", "9"], "--sinkhorn-iters"),
    (["--dino", "--koleo-weight", "0.1", "--batch-size", "1"], "--koleo-weight"),
    (["--sinkhorn-iters", "0"], "--sinkhorn-iters"),                                           # refused with or without --dino
    (["--sinkhorn-iters", "9"], "--sinkhorn-iters"),
])
def test_driver_refuses_before_any_gpu_work(flags, word):
    train = _train()
    args, _ = train.parse_args(["--model", "vit_tiny"] + flags)
    with pytest.raises(SystemExit) as e:
        train.check_supported(args, lambda m: None)
    assert word in str(e.value)


def test_unknown_centering_does_not_parse():
    with pytest.raises(SystemExit):
        _train().parse_args(["--model", "vit_tiny", "--dino", "--centering", "swav"])


def test_engine_refuses_bad_options():
    from gipvit.engine import DinoEngine
    for kw in (dict(centering="swav"), dict(sinkhorn_iters=0), dict(sinkhorn_iters=9), dict(koleo_weight=-1.0), dict(koleo_weight=float("nan")),
               dict(koleo_weight=0.1, batch=1)):
        with pytest.raises(ValueError):
            DinoEngine(**dict(dict(arch="vit_tiny", img_size=224, out_dim=256, batch=2, device="cpu"), **kw))


# ---- the launch sequence
def _traced(micro=False, **kw):
    from gipvit.engine import DinoEngine
    with LT.recording() as rec:
        eng = DinoEngine(arch="vit_tiny", img_size=224, out_dim=256, batch=2, device="cpu", **kw)
        eng.load_state(eng.backbone_state_dict(), eng.head_state_dict())
        eng.load_teacher_state(eng.backbone_state_dict(), eng.head_state_dict(), center=eng.center)
        tiles = torch.zeros(2, 256, 256, 3, dtype=torch.uint8)
        if micro:
            eng.step_micro([tiles, tiles])
        else:
            eng.step(tiles)
    return eng, rec


def _storage(rec, t):
    return rec.storages[t.untyped_storage().data_ptr()]


def _mentions(ev, n):
    def walk(v):
        if isinstance(v, dict):
            return ("tensor" in v and v["tensor"][0] == n) or any(walk(x) for k, x in v.items() if k != "tensor")
        return isinstance(v, list) and any(walk(x) for x in v)
    return len(ev) == 3 and (walk(ev[1]) or walk(ev[2]))


BOTH = dict(centering="sinkhorn_knopp", sinkhorn_iters=3, koleo_weight=0.1)


def test_options_off_leave_the_recorded_sequence():
    """The dino_t procedure of tests/launch_trace.py at batch 2 (KoLeo needs two tiles): the name sequence is the fixture's."""
    fix = LT.load_fixture()["dino_t"]["names"]
    _, rec = _traced()
    assert [e[0] for e in rec.events] == fix
    _, rec = _traced(**BOTH)
    names = [e[0] for e in rec.events]
    assert [n for n in names if n not in NEW] == fix
    assert [n for n in names if n in NEW] == ["koleo_fwd", "sinkhorn_shift", "sinkhorn_cols", "sinkhorn_rows", "sinkhorn_cols", "sinkhorn_rows",
                                              "sinkhorn_cols", "sinkhorn_finish", "koleo_bwd"]


def test_options_off_leave_the_full_trace():
    """Spelled out as off, the options change no launch, no argument, no fill and no wait: the full trace (tests/launch_trace.py's
    SHA-256 form) is that of an engine built without them, for one step and for two micro-batches."""
    for micro in (False, True):
        _, plain = _traced(micro=micro)
        _, off = _traced(micro=micro, centering="center", sinkhorn_iters=5, koleo_weight=0.0)
        assert LT.summary(off.events) == LT.summary(plain.events)
        _, on = _traced(micro=micro, **BOTH)
        assert LT.summary(on.events)["sha256"] != LT.summary(plain.events)["sha256"]


def test_new_launches_sit_where_their_operands_are_ready():
    eng, rec = _traced(**BOTH)
    ev = rec.events
    names = [e[0] for e in ev]
    # Sinkhorn directly precedes the loss, on the main stream behind the teacher's join, and the loss's centre is sk_center
    iloss = names.index("dino_loss")
    assert names[iloss - 7:iloss] == ["sinkhorn_shift", "sinkhorn_cols", "sinkhorn_rows", "sinkhorn_cols", "sinkhorn_rows", "sinkhorn_cols", "sinkhorn_finish"]
    assert names[iloss - 8] == "side.join"
    sk = _storage(rec, eng.sk_center)
    assert ev[iloss][1][2]["tensor"][0] == sk and ev[iloss - 1][1][6]["tensor"][0] == sk and sk != _storage(rec, eng.hb_t.logits)
    assert all(e[1][0]["tensor"][0] == _storage(rec, eng.hb_t.logits) for e in ev[iloss - 7:iloss])
    assert [e[2]["first"] for e in ev[iloss - 6:iloss]] == [True, True, False, False, False, False]
    # KoLeo forward: after the student's backbone wrote the features, before anything reads the workspace
    feats, ikf = _storage(rec, eng.hb_s.feats), names.index("koleo_fwd")
    assert ev[ikf][1][0]["tensor"][0] == feats and any(_mentions(e, feats) for e in ev[:ikf]) and ikf < iloss
    # KoLeo backward: behind the last launch that writes dfeats (the head's last input-gradient product), before its first reader
    df, ikb = _storage(rec, eng.hb_s.dfeats), names.index("koleo_bwd")
    refs = [i for i, e in enumerate(ev) if _mentions(e, df)]
    p = refs.index(ikb)
    assert p == 1 and len(refs) >= 3, refs
    writer = ev[refs[0]]
    assert writer[0] == "linear" and writer[1][2]["tensor"][0] == df and refs[0] > iloss
    assert all(ev[i][0] != "linear" or ev[i][1][2]["tensor"][0] != df for i in refs[2:])      # later mentions read it
    assert ev[ikb][2]["loss_scale"] is None and ev[ikb][1][6] == "0.1"


def test_every_micro_batch_has_its_own_set():
    eng, rec = _traced(micro=True, **BOTH)
    names = [e[0] for e in rec.events]
    assert names.count("sinkhorn_shift") == names.count("sinkhorn_finish") == names.count("koleo_fwd") == names.count("koleo_bwd") == 2
    assert names.count("sinkhorn_cols") == 6 and names.count("sinkhorn_rows") == 4 and names.count("dino_loss") == 2
    order = [n for n in names if n in ("koleo_fwd", "sinkhorn_finish", "dino_loss", "koleo_bwd")]
    assert order == ["koleo_fwd", "sinkhorn_finish", "dino_loss", "koleo_bwd"] * 2
    _, plain = _traced(micro=True)
    assert [n for n in names if n not in NEW] == [e[0] for e in plain.events]
