"""CPU: gv_attention_bwd_stream (csrc/attention_stream_bwd.hip), the streaming attention backward for N <= 1040 tokens, and the
opt-in that carries it up to the driver (engine ``long_seq=True``, train.py --train-long-seq).

What this file holds for the GPU file (tests/test_attention_stream_bwd_gpu.py):
  * `bwd_check(probe)`: the assertion a probe's dq / dk / dv are held to -- the existing check functions on their backward parts,
    no new tolerance,
  * `stream_bwd_model`, fp64 arithmetic with the two launches' rounding points, a key-block and a query-block size, that stands in
    for the kernel here: it meets every check, and each of four streaming-specific faults put into it is rejected by the checks the
    GPU file applies.
Then, without a device: the C ABI's refusals, the launch traces of the engines with and without the keyword, the engines' and the
driver's refusals."""
import ctypes as C
import os

import pytest
import torch

import launch_trace as lt
from test_attention_probes_host import CHECKS, H, N_IMG, SCALE, build, model, rb
from test_attention_stream_host import B_NS, KEY_BLOCK, STREAM_MAX_N, STREAM_NS, STREAM_QBLOCK, r32

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BWD_PARTS = {"A": ("dq", "dk", "dv"), "B": ("dq", "dk", "dv"), "C": ("dk",), "D": ("dq", "dk", "dv")}
KEYS_PER_WG = 128              # keys of a dK / dV workgroup (csrc/attn_plan.h StreamBwdCfg::KEYS); its query stage is KEY_BLOCK rows


def bwd_check(probe):
    """the assertion the GPU file applies to a probe's dq / dk / dv"""
    return lambda got, case: CHECKS[probe](got, case, parts=BWD_PARTS[probe])


def _rejects(check, got, case):
    try:
        check(got, case)
    except AssertionError:
        return True
    return False


# --------------------------------------------------------------------------------------------------- rounding-point model
MUTANTS = ("dq_drops_block_first_key", "dkv_drops_block_first_row", "delta_wrong_row", "block_twice")


def stream_bwd_model(case, kblock=KEY_BLOCK, qblock=STREAM_QBLOCK, scale=SCALE, mutant=None, fwd=None):
    """attn_bwd_stream_dq_kernel + attn_bwd_stream_dkv_kernel in fp64 with their roundings, from the o / lse of ``fwd`` (default: the
    whole-sequence model's): delta = rowsum(dO o) in f32; P = exp(scale S - lse) from the f32 lse; dS = P (dP scale - delta scale);
    P and dS rounded to bf16 before their products; dQ accumulated in f32 over key blocks of `kblock`, dK / dV in f32 over query
    blocks of `qblock`; one bf16 rounding at the store.  `mutant` puts one fault in:
      "dq_drops_block_first_key"    dQ loses the first key of every key block after the first
      "dkv_drops_block_first_row"   dK / dV lose the first query row of every query block after the first
      "delta_wrong_row"             delta[q] is taken from row q + 1 of o / dO (the last row from row 0)
      "block_twice"                 the last key block is added to dQ twice, the last query block to dK / dV twice"""
    q, k, v, d_o, N = case["q"], case["k"], case["v"], case["d_o"], case["N"]
    fwd = model(case, scale) if fwd is None else fwd
    o, lse = fwd["o"], fwd["lse"][..., None]
    delta = (o * d_o).sum(-1, keepdim=True).to(f32).to(f64)
    if mutant == "delta_wrong_row":
        delta = delta.roll(-1, 1)
    s = r32(q @ k.transpose(-1, -2))
    p = (s * scale - lse).exp()
    ds = p * (r32(d_o @ v.transpose(-1, -2)) * scale - delta * scale)
    pb, dsb = rb(p), rb(ds)
    dq = torch.zeros_like(q)
    kstarts = list(range(0, N, kblock))
    for k0 in kstarts + (kstarts[-1:] if mutant == "block_twice" else []):
        blk = dsb[..., k0:k0 + kblock]
        if mutant == "dq_drops_block_first_key" and k0 > 0:
            blk = blk.clone()
            blk[..., 0] = 0.0
        dq = r32(dq + blk @ k[:, k0:k0 + kblock])
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    qstarts = list(range(0, N, qblock))
    for q0 in qstarts + (qstarts[-1:] if mutant == "block_twice" else []):
        pq, dsq = pb[:, q0:q0 + qblock], dsb[:, q0:q0 + qblock]
        if mutant == "dkv_drops_block_first_row" and q0 > 0:
            pq, dsq = pq.clone(), dsq.clone()
            pq[:, 0], dsq[:, 0] = 0.0, 0.0
        dk = r32(dk + dsq.transpose(-1, -2) @ q[:, q0:q0 + qblock])
        dv = r32(dv + pq.transpose(-1, -2) @ d_o[:, q0:q0 + qblock])
    return dict(dq=rb(dq), dk=rb(dk), dv=rb(dv))


# ------------------------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("N", STREAM_NS)
def test_probe_conditions_hold_on_the_backward_parts_at_the_streaming_lengths(N):
    """The whole-sequence rounding model meets every probe's check on dq / dk / dv at every streaming length (B on B_NS), and the
    three faults of the host probe file are rejected there by A, B and D."""
    for probe in "ABCD":
        if probe == "B" and N not in B_NS:
            continue
        case = build(probe, N)
        bwd_check(probe)(model(case), case)
        if probe == "C":
            continue
        for mutant in ("drop_last_key", "drop_last_query", "swap_pairs"):
            assert _rejects(bwd_check(probe), model(case, mutant=mutant), case), (probe, N, mutant)


@pytest.mark.parametrize("N", [289, 320, 1025, 1040])
def test_block_model_meets_every_probe(N):
    """Key blocks of 64 and query blocks of 128 / 64 with f32 accumulators across them give probe A's dv bit for bit and meet
    every check; the block sizes change nothing the checks see."""
    for probe in "ABCD":
        if probe == "B" and N not in B_NS:
            continue
        case = build(probe, N)
        for kblock, qblock in ((KEY_BLOCK, STREAM_QBLOCK), (KEY_BLOCK, KEY_BLOCK), (KEYS_PER_WG, STREAM_QBLOCK)):
            got = stream_bwd_model(case, kblock, qblock)
            bwd_check(probe)(got, case)
            if probe == "A":
                assert torch.equal(got["dv"], case["dv"])


@pytest.mark.parametrize("N", [320, 1024])
def test_exact_probes_reject_the_streaming_faults(N):
    """A key lost from dQ at a block seam: probe B (its dQ is exact and nonzero).  A query row lost from dK / dV at a block seam: probe
    A's bit-exact dv.  delta from a wrong row: probe A (dS = 0 needs delta[q] = dO[q] . o[q]) and B.  A block added twice: both."""
    a, b = build("A", N), build("B", N)
    assert N in B_NS
    assert _rejects(bwd_check("B"), stream_bwd_model(b, mutant="dq_drops_block_first_key"), b)
    got = stream_bwd_model(a, mutant="dkv_drops_block_first_row")
    assert _rejects(lambda g, c: CHECKS["A"](g, c, parts=("dv",)), got, a)
    for case, probe in ((a, "A"), (b, "B")):
        assert _rejects(bwd_check(probe), stream_bwd_model(case, mutant="delta_wrong_row"), case), probe
        assert _rejects(bwd_check(probe), stream_bwd_model(case, mutant="block_twice"), case), probe


def test_probe_d_rejects_the_streaming_faults_at_1025():
    d = build("D", 1025)
    bwd_check("D")(stream_bwd_model(d), d)
    for mutant in MUTANTS:
        assert _rejects(bwd_check("D"), stream_bwd_model(d, mutant=mutant), d), mutant


# ---- the C ABI without a device
def _abi():
    from gipvit import _lib
    buf = (C.c_char * 4096)()
    ptr = (C.addressof(buf) + 255) & ~255
    call = lambda *a: _lib.lib.gv_attention_bwd_stream(C.byref(_lib.gv_attention_bwd_stream_args(*a)), None)
    return _lib, buf, ptr, call


def test_entry_point_is_declared_bound_and_exported_by_both_libraries():
    import re
    import subprocess
    import sys
    _lib = _abi()[0]
    hdr = open(os.path.join(ROOT, "include", "gipvit.h")).read()
    assert "gv_attention_bwd_stream" in set(re.findall(r"^int\s+(gv_\w+)\(", hdr, re.M))
    assert _lib.ENTRY_POINTS["gv_attention_bwd_stream"] is _lib.gv_attention_bwd_stream_args
    assert [f[0] for f in _lib.gv_attention_bwd_stream_args._fields_] == ["qkv", "o", "d_o", "lse", "dqkv", "delta", "n_img", "N", "H", "scale", "q_limit"]
    assert hasattr(_lib.lib, "gv_attention_bwd_stream")
    code = "import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); assert hasattr(l, 'gv_attention_bwd_stream') and l.gv_act_format() == 1"
    r = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(_lib.LIB_PATH), "libgipvit_hip_f16.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_arguments_are_validated_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail with a HIP error code (> 0), not with GV_E_*."""
    _lib, buf, ptr, call = _abi()
    ok = (ptr,) * 6
    for N in (0, STREAM_MAX_N + 1, -5):
        assert call(*ok, 1, N, 1, SCALE, 0) == -1                                  # GV_E_SHAPE
        msg = _lib.lib.gv_last_error().decode()
        assert str(STREAM_MAX_N) in msg and "gv_attention_bwd_stream" in msg, msg
    assert call(*ok, 0, 300, 1, SCALE, 0) == -1 and call(*ok, 1, 300, 0, SCALE, 0) == -1
    for i in range(6):                                                             # qkv, o, d_o, lse, dqkv, delta
        args = list(ok)
        args[i] = None
        assert call(*args, 1, 300, 1, SCALE, 0) == -3, i                           # GV_E_NULL
    assert _lib.lib.gv_attention_bwd_stream(None, None) == -3
    for i in (0, 1, 2, 4):                                                         # qkv, o, d_o, dqkv
        args = list(ok)
        args[i] = ptr + 2
        assert call(*args, 1, 300, 1, SCALE, 0) == -2, i                           # GV_E_ALIGN
    for bad_scale in (0.0, -0.125):
        assert call(*ok, 1, 300, 1, bad_scale, 0) == -1 and "scale" in _lib.lib.gv_last_error().decode()
    # the order of the streaming forward: pointers, shape, scale, alignment
    assert call(None, ptr, ptr, ptr, ptr, ptr, 1, 0, 1, 0.0, 0) == -3
    assert call(ptr + 2, ptr, ptr, ptr, ptr, ptr, 1, 0, 1, 0.0, 0) == -1 and str(STREAM_MAX_N) in _lib.lib.gv_last_error().decode()
    assert call(ptr + 2, ptr, ptr, ptr, ptr, ptr, 1, 300, 1, 0.0, 0) == -1 and "scale" in _lib.lib.gv_last_error().decode()
    # the whole-sequence backward keeps its limit
    assert _lib.lib.gv_attention_bwd(C.byref(_lib.gv_attention_bwd_args(ptr, ptr, ptr, ptr, ptr, 1, 289, 1, SCALE, 0)), None) == -1


def test_ops_wrapper_refuses_other_dtypes():
    from gipvit import ops
    qkv, o = torch.zeros(300, 3 * 64, dtype=bf16), torch.zeros(300, 64, dtype=bf16)
    lse = torch.zeros(1, 1, 300)
    with pytest.raises(TypeError, match="no fp32 operand form"):
        ops.attention_bwd_stream(qkv.float(), o.float(), o.float(), lse, 1, 300, 1, SCALE)
    with pytest.raises(TypeError, match="share one dtype"):
        ops.attention_bwd_stream(qkv, o, o.float(), lse, 1, 300, 1, SCALE)
    with pytest.raises(TypeError, match="share one dtype"):
        ops.attention_bwd_stream(qkv, o, o, lse, 1, 300, 1, SCALE, dqkv=torch.zeros(300, 3 * 64))
    with pytest.raises(TypeError, match="delta"):
        ops.attention_bwd_stream(qkv, o, o, lse, 1, 300, 1, SCALE, delta=torch.zeros(299))


# ---- launch traces
def _tiles(n, px):
    return torch.zeros(n, px, px, 3, dtype=torch.uint8)


def _sup_trace(px, **kw):
    from gipvit.engine import SupervisedEngine
    with lt.recording() as rec:
        eng = SupervisedEngine(arch="vit_tiny", img_size=px, num_classes=2, batch=2, device="cpu", **kw)
        eng.step(_tiles(2, px), torch.zeros(2, 1, dtype=torch.int64))
    return eng, rec.events


def _dino_trace(**kw):
    from gipvit.engine import DinoEngine
    with lt.recording() as rec:
        eng = DinoEngine(arch="vit_tiny", out_dim=256, batch=1, device="cpu", **kw)
        eng.step(_tiles(1, kw.get("tile", 256)))
    return eng, rec.events


def _calls(events, name):
    return [e for e in events if e[0] == name]


def test_the_keyword_changes_no_launch_below_the_limit():
    (e0, off), (e1, on) = _sup_trace(64), _sup_trace(64, long_seq=True)
    assert e1.grp.stream_bwd and not e0.grp.stream_bwd and not hasattr(e1.grp, "delta")
    assert on == off and lt.summary(on)["sha256"] == lt.summary(off)["sha256"]
    (d0, off), (d1, on) = _dino_trace(img_size=224), _dino_trace(img_size=224, long_seq=True)
    assert d1.g_stu.stream_bwd and not hasattr(d1.g_stu, "delta") and not getattr(d1.g_teach, "stream_bwd")
    assert on == off and lt.summary(on)["sha256"] == lt.summary(off)["sha256"]
    assert len(_calls(on, "attention_bwd_varlen")) == 12 and not _calls(on, "attention_bwd_stream")


def test_supervised_step_above_the_limit_streams_every_block():
    eng, ev = _sup_trace(272, long_seq=True)
    fwd, bwd = _calls(ev, "attention_fwd_stream"), _calls(ev, "attention_bwd_stream")
    assert len(fwd) == 12 and len(bwd) == 12
    assert not _calls(ev, "attention_bwd") and not _calls(ev, "attention_bwd_varlen") and not _calls(ev, "attention_fwd") and not _calls(ev, "attention_fwd_varlen")
    # the CLS-only last block: its forward (the last one recorded) and its backward (the first) carry q_limit = 1, the others 0 / none
    assert [c[2].get("q_limit", 0) for c in fwd] == [0] * 11 + [1]
    assert [c[2].get("q_limit", 0) for c in bwd] == [1] + [0] * 11
    for c in bwd:
        assert c[1][4:] == [2, 290, 3, repr(64 ** -0.5)] and c[2]["delta"]["tensor"][2] == [2 * 3 * 290] and c[2]["delta"]["tensor"][4] == "torch.float32"
    assert eng.grp.delta.numel() == 2 * 3 * 290


def test_dino_step_streams_the_global_segment_only():
    eng, ev = _dino_trace(img_size=272, tile=288, gsize=272, lsize=96, n_local=2, long_seq=True)
    G = eng.g_stu
    assert [sg.N for sg in G.segs] == [290, 37] and G.delta.numel() == 2 * 3 * 290 and not hasattr(eng.g_teach, "delta")
    bwd_s, bwd = _calls(ev, "attention_bwd_stream"), _calls(ev, "attention_bwd")
    assert len(bwd_s) == 12 and len(bwd) == 12 and not _calls(ev, "attention_bwd_varlen") and not _calls(ev, "attention_fwd_varlen")
    assert all(c[1][4:6] == [2, 290] for c in bwd_s) and all(c[1][4:6] == [2, 37] for c in bwd)
    # the same q_limit reaches both segments of a block
    assert [c[2].get("q_limit", 0) for c in bwd_s] == [c[2].get("q_limit", 0) for c in bwd] == [1] + [0] * 11
    # student (12 blocks) and teacher (12 blocks) stream the 290-token segment forward, the student's local crops do not
    assert len(_calls(ev, "attention_fwd_stream")) == 24
    assert len(_calls(ev, "attention_fwd")) == 12 and all(c[1][1:3] == [2, 37] for c in _calls(ev, "attention_fwd"))


# ---- the inputs of the GPU file's whole-step comparison
def step_targets(B):
    """One label for every image of the supervised step the GPU file compares with the oracle (the first draw of the seed that
    tests/test_engine_gpu.py uses): see test_one_label_keeps_the_batch_gradient_from_cancelling."""
    return torch.randint(0, 2, (1, 1), generator=torch.Generator().manual_seed(5)).expand(B, 1).contiguous()


def test_one_label_keeps_the_batch_gradient_from_cancelling():
    """Why the two images of the 272- / 512-px step carry ONE label -- shown on the fp32 oracle alone, no kernel involved.  The
    synthetic tiles are noise around one mean, so at initialisation (p ~ 1/2) the two per-image gradients are nearly equal in size
    and, with opposite labels, opposite in sign: the batch gradient is what their cancellation leaves.  With labels (1, 0) the
    median parameter keeps 9 % of the per-image gradient norm and norm.bias 2.3 % (a 43-fold cancellation): one bf16 rounding
    (2^-9 relative) of a per-image term is then already 8 % of the quantity a 5e-2 relative gate is put on.  With one label the terms
    add and every parameter keeps more than 90 %, so the gate measures the engine, not the cancellation."""
    from oracle import step_oracle as so, vit_oracle as vo
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    orc = so.SupervisedOracle(arch="vit_tiny", img_size=272, num_classes=2, seed=0, lr=1e-3, wd=0.05)
    tiles = vo.synth_tiles(2, 272, seed=1234)
    grads = lambda t, labels: orc.forward_backward(t, torch.tensor(labels).view(-1, 1))[1]
    first = int(step_targets(2)[0])
    img0, img1 = grads(tiles[:1], [first]), {lab: grads(tiles[1:], [lab]) for lab in (0, 1)}

    def kept(labels):
        g, g1 = grads(tiles, labels), img1[labels[1]]
        r = sorted(float(g[k].norm() / ((img0[k].norm() + g1[k].norm()) / 2)) for k in g if float(g[k].abs().max()) >= 1e-12)
        return r[0], r[len(r) // 2]
    worst, median = kept([first, 1 - first])
    assert worst < 0.03 and median < 0.12, (worst, median)
    worst, median = kept(step_targets(2).view(-1).tolist())
    assert worst > 0.9 and median > 0.98, (worst, median)


# ---- refusals
def test_engine_refusals():
    from types import SimpleNamespace as NS
    from gipvit.engine import DinoEngine, SupervisedEngine, VitRunner
    tiles, tgt = _tiles(2, 272), torch.zeros(2, 1, dtype=torch.int64)
    with lt.recording():
        eng = SupervisedEngine(arch="vit_tiny", img_size=272, num_classes=2, batch=2, device="cpu")
        with pytest.raises(ValueError, match="288-token limit"):
            eng.step(tiles, tgt)
        d = DinoEngine(arch="vit_tiny", img_size=272, out_dim=256, batch=1, tile=288, gsize=272, n_local=0, device="cpu")
        with pytest.raises(ValueError, match="288-token limit"):
            d.step(_tiles(1, 288))
    for Engine, kw in ((SupervisedEngine, dict(img_size=272)), (DinoEngine, dict(img_size=272, gsize=272, tile=288, out_dim=256))):
        with pytest.raises(ValueError, match="fp32"):
            Engine(arch="vit_tiny", batch=2, device="cpu", long_seq=True, precision="fp32", **kw)
    with pytest.raises(ValueError, match="1040"):
        SupervisedEngine(arch="vit_tiny", img_size=528, batch=2, device="cpu", long_seq=True)
    with pytest.raises(ValueError, match="1040"):
        DinoEngine(arch="vit_tiny", img_size=224, gsize=528, tile=544, out_dim=256, batch=1, device="cpu", long_seq=True)
    with pytest.raises(ValueError, match="1040"):
        DinoEngine(arch="vit_tiny", img_size=224, lsize=528, tile=544, out_dim=256, batch=1, device="cpu", long_seq=True)
    long_grp = NS(segs=[NS(N=290, crop=272)], stream_bwd=True)
    VitRunner.require_trainable(long_grp)
    with pytest.raises(ValueError, match="288-token limit"):
        VitRunner.require_trainable(NS(segs=[NS(N=290, crop=272)], stream_bwd=False))
    with pytest.raises(ValueError, match="1040"):
        VitRunner.require_trainable(NS(segs=[NS(N=1090, crop=528)], stream_bwd=True))
    with pytest.raises(ValueError, match="288-token limit"):
        VitRunner.require_attention_maps(long_grp)


_BASE = ["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "-b", "2", "--epochs", "1"]


def test_train_py_token_limits_with_the_flag():
    import train
    check = lambda extra: train.check_token_limits(train.parse_args(_BASE + extra)[0])
    assert train.parse_args(_BASE)[0].train_long_seq is False
    for px in ("272", "512"):
        check(["--img-size", px, "--tile-size", px, "--train-long-seq"])
    check(["--dino", "--global-crop-size", "448", "--tile-size", "512", "--train-long-seq"])
    check(["--dino", "--global-crop-size", "272", "--local-crop-size", "304", "--tile-size", "512", "--train-long-seq"])
    check(["--img-size", "256", "--tile-size", "256", "--train-long-seq", "--precision", "fp32"])
    refused = ((["--img-size", "528", "--tile-size", "528"], "1040"),
               (["--dino", "--global-crop-size", "528", "--tile-size", "544"], "1040"),
               (["--dino", "--local-crop-size", "528", "--tile-size", "544"], "1040"),
               (["--img-size", "272", "--tile-size", "272", "--precision", "fp32"], "260"),
               (["--img-size", "272", "--tile-size", "272", "--extract_features", "--extract-attention"], "288 tokens"),
               (["--dino", "--global-crop-size", "272", "--tile-size", "272", "--extract_features"], "288 tokens"))
    for extra, word in refused:
        with pytest.raises(SystemExit, match=word):
            check(extra + ["--train-long-seq"])
    # without the flag every message is today's
    with pytest.raises(SystemExit, match="training stops at 288 tokens"):
        check(["--img-size", "272", "--tile-size", "272"])
    assert "--train-long-seq" not in {f for e in train.REFERENCE_FLAGS for f in e["flags"]}
