"""CPU: gv_attention_probs_stream (csrc/attention_probs_stream.hip), the attention probabilities for sequences past 288 tokens, and
the opt-in that carries it up to the driver (VitGroup stream_maps, FeatureExtractor / create_model long_maps,
train.py --long-attention-maps).

What this file holds for the GPU file (tests/test_attention_probs_stream_gpu.py), on top of build("A" | "C" | "D", N) of
tests/test_attention_probes_host.py and STREAM_NS / SHORT_NS of tests/test_attention_stream_host.py:
  * `build_probs_spike`, the spike input of tests/test_attention_maps_gpu.py::check_probs (q = 1, one key = 3: score 24 against
    O(1)) with the key at a chosen place, pair-major like the probes' cases,
  * `softmax_ref`, torch's f32 softmax of a case's 16-bit inputs, and `probs_model`, the kernel in torch -- f32
    exp(s scale - lse) on the same inputs -- which stands in for the kernel here and takes six faults,
  * the assertion functions the GPU file applies (`check_probs_selector`, `check_probs_uniform`, `check_probs_random`); a
    failure names probe, N, q_rows, pair and row.
The CPU tests show that the model meets every assertion and that each fault put into it is rejected; then the entry point, its
refusals, the host plan, the launch traces of the opt-in and the refusals that need no device."""
import math
import os
import subprocess
import sys

import pytest
import torch

from launch_trace import recording
from test_attention_probes_host import H, N_IMG, SCALE, build
from test_attention_stream_host import SHORT_NS, STREAM_MAX_N, STREAM_NS, STREAM_QBLOCK, KEY_BLOCK

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = N_IMG * H
MAX_N = 288                                   # GV_ATTN_MAX_N: gv_attention_probs' limit

# the issue's gates
OFF_SELECTED = 2e-14                          # probe A: score gap >= 32, exp(-32) = 1.27e-14
DP_GATE, ROWSUM_GATE, PV_GATE = 1e-4, 1e-4, 2e-2      # those of tests/test_attention_maps_gpu.py::check_probs
RANDOM_NS = (289, 513, 1025, 1039, 1040)
Q_ROWS = lambda N: (1, 5, 16, 17, 128, 129, N)


# ------------------------------------------------------------------------------------------------------------ builders
_spikes = {}


def build_probs_spike(N, key):
    """check_probs' spike: randn q, k, v rounded to bf16, then every q = 1 and k[key] = 3 (score 64 * 3 * 0.125 = 24)"""
    if (N, key) not in _spikes:
        g = torch.Generator().manual_seed(N * 131 + H + 7919 * key)
        q, k, v = (torch.randn(P, N, 64, generator=g).to(bf16).to(f64) for _ in range(3))
        q[:] = 1.0
        k[:, key] = 3.0
        _spikes[(N, key)] = dict(q=q, k=k, v=v, N=N, probe=f"spike-key{key}")
    return _spikes[(N, key)]


def spike_keys(N):
    """key 7, and the last key: in the last KEY_BLOCK-key block and in its last, partial 16-key tile"""
    return (7, N - 1)


def scores_f32(case):
    """q k^T in f32 on the case's 16-bit inputs [P, N, N] (unscaled: what the MFMAs accumulate)"""
    return case["q"].to(f32) @ case["k"].to(f32).transpose(-1, -2)


def softmax_ref(case, scale=SCALE):
    """torch's f32 softmax of the same 16-bit inputs, [P, N, N]"""
    return (scores_f32(case) * scale).softmax(-1)


def lse_ref(case, scale=SCALE):
    """what the forward leaves: the f32 rounding of the log-sum-exp of the scaled scores (taken in fp64)"""
    return torch.logsumexp(case["q"] @ case["k"].transpose(-1, -2) * scale, -1).to(f32)


MUTANTS = ("shift_last_tile", "drop_seam", "lse_next_row", "swap_pairs", "row_stride_16", "shift_last_qblock")


def probs_model(case, q_rows, lse=None, scale=SCALE, mutant=None):
    """The kernel in torch: p = exp(s scale - lse) in f32 for rows < q_rows -> f32 [P, q_rows, N].  `mutant` puts one fault in:
      "shift_last_tile"    the key index is shifted by one inside the last partial 16-key tile (the tile's last key reads a zero pad key)
      "drop_seam"          the first key of every key block after the first is never written (p holds what was there: 0)
      "lse_next_row"       row q uses the lse of row q + 1
      "swap_pairs"         the outputs of pairs 1 and 2 change places
      "row_stride_16"      rows are stored with a stride of N rounded up to 16 into the compact buffer
      "shift_last_qblock"  the rows of the last block of STREAM_QBLOCK query rows are shifted by one"""
    N = case["N"]
    lse = lse_ref(case, scale) if lse is None else lse
    s = scores_f32(case)
    if mutant == "shift_last_tile":
        idx = torch.arange(N)
        idx[(N - 1) // 16 * 16:] += 1
        s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)[..., idx]
    rows = torch.arange(q_rows)
    lrows = (rows + 1).clamp_max(N - 1) if mutant == "lse_next_row" else rows
    if mutant == "shift_last_qblock":
        q0 = (q_rows - 1) // STREAM_QBLOCK * STREAM_QBLOCK
        rows = lrows = torch.where(rows >= q0, (rows + 1).clamp_max(N - 1), rows)
    p = (s[:, rows] * scale - lse[:, lrows][..., None]).exp()
    if mutant == "drop_seam":
        p[..., KEY_BLOCK::KEY_BLOCK] = 0.0
    if mutant == "swap_pairs":
        p = p[[0, 2, 1] + list(range(3, p.shape[0]))]
    if mutant == "row_stride_16":
        Np = (N + 15) // 16 * 16
        flat = torch.zeros(P * q_rows * Np, dtype=f32)
        flat.view(P, q_rows, Np)[..., :N] = p
        p = flat[:P * q_rows * N].view(P, q_rows, N).clone()
    return p


# --------------------------------------------------------------------------------------------------- assertion functions
def _fail(case, q_rows, what, ok_rows, extra=""):
    """`ok_rows`: boolean [P, q_rows]; names probe, N, q_rows and the first failing (pair, row)"""
    if bool(ok_rows.all()):
        return
    bad = (~ok_rows).nonzero()
    pair, row = (int(i) for i in bad[0])
    raise AssertionError(f"probe {case['probe']} N={case['N']} q_rows={q_rows}: {what}: {bad.shape[0]} of {ok_rows.numel()} (pair, row) wrong, "
                         f"first pair {pair} row {row} (pairs {sorted(set(bad[:, 0].tolist()))}){extra}")


def check_probs_selector(p, case, q_rows):
    """probe A: p[q, perm[q]] == 1.0 bit for bit (the selected score times scale log2e and lse log2e cancel exactly at lse = 128),
    every other entry <= 2e-14; a NaN fails."""
    assert p.shape == (case["q"].shape[0], q_rows, case["N"]) and p.dtype == f32
    perm = case["perm"][:, :q_rows]
    sel = torch.gather(p, 2, perm[..., None])[..., 0]
    _fail(case, q_rows, "the selected key's p is not 1.0", sel == 1.0)
    rest = p.clone()
    rest.scatter_(2, perm[..., None], 0.0)
    _fail(case, q_rows, f"an unselected key's p is above {OFF_SELECTED}", (rest <= OFF_SELECTED).all(-1) & (rest >= 0).all(-1))


def check_probs_uniform(p, case, q_rows):
    """probe C (Q = 0): the N entries of a row are bitwise equal and |row sum - 1| <= 1e-4"""
    assert p.shape == (case["q"].shape[0], q_rows, case["N"]) and p.dtype == f32
    bits = p.contiguous().view(torch.int32)
    _fail(case, q_rows, "the entries of a row differ", (bits == bits[..., :1]).all(-1))
    _fail(case, q_rows, f"|row sum - 1| > {ROWSUM_GATE}", (p.double().sum(-1) - 1).abs() <= ROWSUM_GATE)


def check_probs_random(p, case, q_rows, ref=None):
    """randn / spike: |dP| <= 1e-4 against torch's f32 softmax of the same 16-bit inputs (`ref`: softmax_ref(case), computed once by
    the caller), |row sum - 1| <= 1e-4; a NaN fails"""
    assert p.shape == (case["q"].shape[0], q_rows, case["N"]) and p.dtype == f32
    ref = softmax_ref(case) if ref is None else ref
    d = (p - ref[:, :q_rows]).abs()
    _fail(case, q_rows, f"|dP| > {DP_GATE}", (d <= DP_GATE).all(-1), f", max |dP| {float(torch.nan_to_num(d, nan=math.inf).max()):.3e}")
    rs = (p.double().sum(-1) - 1).abs()
    _fail(case, q_rows, f"|row sum - 1| > {ROWSUM_GATE}", rs <= ROWSUM_GATE, f", max {float(torch.nan_to_num(rs, nan=math.inf).max()):.3e}")


def check_bitwise(p, want, case, q_rows, what):
    """two results that must agree bit for bit, [P, q_rows, N]"""
    same = (p.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)).all(-1)
    _fail(case, q_rows, what, same)


def _rejects(check, *args):
    try:
        check(*args)
    except AssertionError as e:
        msg = str(e)
        assert all(w in msg for w in ("probe", "N=", "q_rows=", "pair", "row")), msg
        return True
    return False


# ---------------------------------------------------------------------------------------- the model and its mutants (CPU)
@pytest.mark.parametrize("N", [289, 321, 1025])
def test_the_model_meets_every_assertion(N):
    a, c, d = build("A", N), build("C", N), build("D", N)
    for q_rows in (1, 17, N):
        check_probs_selector(probs_model(a, q_rows), a, q_rows)
        check_probs_uniform(probs_model(c, q_rows), c, q_rows)
        check_probs_random(probs_model(d, q_rows), d, q_rows)
    for key in spike_keys(N):
        sp = build_probs_spike(N, key)
        check_probs_random(probs_model(sp, N), sp, N)
    assert spike_keys(N)[1] >= (N - 1) // KEY_BLOCK * KEY_BLOCK and spike_keys(N)[1] < N
    # probe A's premise for the exact 1.0: lse = 128 exactly, the selected score 128 exactly
    assert bool((lse_ref(a) == 128.0).all()) and float((scores_f32(a) * SCALE).max()) == 128.0


@pytest.mark.parametrize("N", [289, 1025])
def test_the_assertions_reject_every_mutant(N):
    """Each fault is rejected by the assertion the GPU file applies to that input, with a message that names probe, N, q_rows, pair
    and row.  (lse_next_row is invisible to probes A and C, whose lse is one number: the randn and spike inputs catch it.)"""
    a, d = build("A", N), build("D", N)
    ref_d = softmax_ref(d)
    for mutant in ("shift_last_tile", "drop_seam", "swap_pairs", "row_stride_16"):
        assert _rejects(check_probs_selector, probs_model(a, N, mutant=mutant), a, N), (N, mutant)
    for mutant in ("shift_last_tile", "drop_seam", "lse_next_row", "swap_pairs", "row_stride_16"):
        assert _rejects(check_probs_random, probs_model(d, N, mutant=mutant), d, N, ref_d), (N, mutant)
    # (at q_rows = N = 1 025 the last query block is one row: the shift is shown where the block holds more, rows 128 .. 199)
    assert _rejects(check_probs_selector, probs_model(a, 200, mutant="shift_last_qblock"), a, 200)
    assert _rejects(check_probs_random, probs_model(d, 200, mutant="shift_last_qblock"), d, 200, ref_d)
    assert _rejects(check_probs_random, probs_model(d, 17, mutant="lse_next_row"), d, 17, ref_d)
    sp = build_probs_spike(N, spike_keys(N)[1])
    assert _rejects(check_probs_random, probs_model(sp, N, mutant="shift_last_tile"), sp, N)
    c = build("C", N)
    assert _rejects(check_probs_uniform, probs_model(c, N, mutant="drop_seam"), c, N)
    # the bitwise comparisons see a one-row shift of the last query block at any q_rows past one block
    good = probs_model(d, N)
    for q_rows in (129, 200):
        assert _rejects(check_bitwise, probs_model(d, q_rows, mutant="shift_last_qblock"), good[:, :q_rows], d, q_rows, "rows differ")


# --------------------------------------------------------------------------------------------------- entry point and ABI
def _declared():
    import re
    return set(re.findall(r"^int\s+(gv_\w+)\(", open(os.path.join(ROOT, "include", "gipvit.h")).read(), re.M))


def test_both_libraries_export_the_entry_point_and_the_binding_uses_the_probs_struct():
    from gipvit import _lib, build as B
    assert "gv_attention_probs_stream" in _declared() and "gv_attention_probs_stream_f32" not in _declared()
    assert _lib.ENTRY_POINTS["gv_attention_probs_stream"] is _lib.gv_attention_probs_args
    assert hasattr(_lib.lib, "gv_attention_probs_stream")
    assert "attention_probs_stream" in B.SOURCES and os.path.exists(os.path.join(os.path.dirname(B.__file__), "csrc", "attention_probs_stream.hip"))
    code = "import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); assert hasattr(l, 'gv_attention_probs_stream') and l.gv_act_format() == 1"
    r = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(_lib.LIB_PATH), "libgipvit_hip_f16.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_arguments_are_validated_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail with a HIP error code (> 0), not with GV_E_*."""
    from gipvit import _lib
    import ctypes as C
    buf = (C.c_char * 4096)()
    ptr = (C.addressof(buf) + 255) & ~255
    call = lambda *a: _lib.lib.gv_attention_probs_stream(C.byref(_lib.gv_attention_probs_args(*a)), None)
    err = lambda: _lib.lib.gv_last_error().decode()
    for N in (0, STREAM_MAX_N + 1):
        assert call(ptr, ptr, ptr, 1, N, 1, SCALE, 1) == -1                     # GV_E_SHAPE
        assert str(STREAM_MAX_N) in err() and "gv_attention_probs_stream" in err(), err()
    for q_rows in (0, 301):
        assert call(ptr, ptr, ptr, 1, 300, 1, SCALE, q_rows) == -1 and "q_rows" in err(), err()
    assert call(ptr, ptr, ptr, 1, 300, 1, 0.0, 1) == -1 and "scale" in err(), err()
    for args in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None)):
        assert call(*args, 1, 300, 1, SCALE, 1) == -3                           # GV_E_NULL
    assert _lib.lib.gv_attention_probs_stream(None, None) == -3
    assert call(ptr + 2, ptr, ptr, 1, 300, 1, SCALE, 1) == -2 and "16-byte" in err()        # GV_E_ALIGN
    # the order of the streaming forward: pointers, N, (q_rows,) scale, alignment
    assert call(None, ptr, ptr, 1, 0, 1, 0.0, 0) == -3
    assert call(ptr + 2, ptr, ptr, 1, 0, 1, 0.0, 0) == -1 and str(STREAM_MAX_N) in err()
    assert call(ptr + 2, ptr, ptr, 1, 300, 1, 0.0, 0) == -1 and "q_rows" in err()
    assert call(ptr + 2, ptr, ptr, 1, 300, 1, 0.0, 1) == -1 and "scale" in err()
    # the whole-sequence entry point keeps its limit
    assert _lib.lib.gv_attention_probs(C.byref(_lib.gv_attention_probs_args(ptr, ptr, ptr, 1, MAX_N + 1, 1, SCALE, 1)), None) == -1


def test_ops_wrapper_refuses_f32_operands_and_mismatched_dtypes():
    from gipvit import ops
    qkv, lse = torch.zeros(300, 3 * 64, dtype=ops.bf16), torch.zeros(1, 1, 300)
    with pytest.raises(ValueError, match="_f32"):
        ops.attention_probs_stream(qkv.float(), lse, 1, 300, 1, SCALE, 1)
    with pytest.raises(TypeError, match="attention_probs_stream"):
        ops.attention_probs_stream(qkv.double(), lse, 1, 300, 1, SCALE, 1)
    with pytest.raises(TypeError, match="attention_probs_stream"):
        ops.attention_probs_stream(qkv, lse.to(ops.bf16), 1, 300, 1, SCALE, 1)
    with pytest.raises(TypeError, match="attention_probs_stream"):
        ops.attention_probs_stream(qkv, lse, 1, 300, 1, SCALE, 1, p=torch.zeros(1, 1, 1, 300, dtype=ops.bf16))
    with pytest.raises(ValueError, match="contiguous buffer"):
        ops.attention_probs_stream(qkv, lse, 1, 300, 1, SCALE, 1, p=torch.zeros(1, 1, 2, 300))
    with pytest.raises(ValueError, match="smaller"):
        ops.attention_probs_stream(qkv[:100], lse, 1, 300, 1, SCALE, 1)


# ------------------------------------------------------------------------------------------------------------ host plan
def test_plan_of_both_forms(tmp_path):
    """ProbsStreamCfg through a plain g++ program (tests/attn_probs_stream_plan_main.cc): row form = one workgroup per pair and no
    LDS, block form = pairs x ceil(q_rows / 128) workgroups of the Cfg's threads within 160 KB of LDS."""
    exe = str(tmp_path / "plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "attn_probs_stream_plan_main.cc"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n_img, Hh = 5, 3
    cases = [(N, q) for N in (289, 1025, STREAM_MAX_N) for q in (1, 16, 17, 128, 129, N)]
    r = subprocess.run([exe] + [str(x) for _, q in cases for x in (n_img, Hh, q)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    assert lines[0][0] == "cfg" and len(lines) == 1 + len(cases)
    row_threads, row_nw, row_ch, threads, qb, kb, lds, occ = map(int, lines[0][1:])
    assert qb == STREAM_QBLOCK and kb == KEY_BLOCK and lds == 2 * kb * 128 and occ * lds <= 160 * 1024
    assert row_threads == 64 * row_nw <= 1024 and threads % 64 == 0 and threads // 64 * 32 == qb and row_ch * 8 <= 128
    for (N, q), got in zip(cases, lines[1:]):
        by_row, grid, block, l, nqb = map(int, got)
        pairs = n_img * Hh
        if q <= 16:
            assert (by_row, grid, block, l) == (1, pairs, row_threads, 0), (N, q, got)
        else:
            assert nqb == (q + STREAM_QBLOCK - 1) // STREAM_QBLOCK
            assert (by_row, grid, block, l) == (0, pairs * nqb, threads, lds) and l <= 160 * 1024, (N, q, got)


# -------------------------------------------------------------------------------------------------------- launch traces
def _trace(img, long_maps, what, n_tiles=3, batch=2):
    from gipvit.engine import FeatureExtractor
    kw = dict(long_maps=True) if long_maps else {}
    with recording() as rec:
        fx = FeatureExtractor(arch="vit_tiny", img_size=img, batch=batch, num_classes=2, device="cpu", **kw)
        tiles = torch.zeros(n_tiles, img, img, 3, dtype=torch.uint8)
        try:
            if what == "run_with_attention":
                fx.run_with_attention(tiles)
            else:
                fx.last_selfattention(tiles, cls_only=(what == "cls_only"))
        except ValueError as e:
            return rec.events, e
    return rec.events, None


@pytest.mark.parametrize("img", [64, 256])
@pytest.mark.parametrize("what", ["run_with_attention", "last_selfattention"])
def test_the_keyword_changes_no_launch_at_or_below_256_px(img, what):
    n_tiles, batch = (3, 2) if img == 64 else (2, 1)
    with_kw, e1 = _trace(img, True, what, n_tiles, batch)
    without, e2 = _trace(img, False, what, n_tiles, batch)
    assert e1 is None and e2 is None and with_kw == without and len(without) > 50
    names = [e[0] for e in with_kw]
    assert names.count("attention_probs") == (n_tiles + batch - 1) // batch and "attention_probs_stream" not in names


@pytest.mark.parametrize("what", ["run_with_attention", "last_selfattention", "cls_only"])
def test_at_272_px_the_keyword_streams_the_map_and_its_absence_raises_before_the_first_event(what):
    events, err = _trace(272, True, what)                   # 3 tiles in batches of 2: a full batch and a padded one
    assert err is None
    names = [e[0] for e in events]
    assert names.count("attention_probs_stream") == 2 and "attention_probs" not in names
    assert names.count("attention_fwd_stream") == 2 * 12 and "attention_fwd" not in names
    call = [e for e in events if e[0] == "attention_probs_stream"][0]
    assert call[1][2:5] == [2, 290, 3] and call[1][6] == (290 if what == "last_selfattention" else 1) and set(call[2]) == {"p"}
    events, err = _trace(272, False, what)
    assert events == [] and err is not None and "288-token limit" in str(err)


# ------------------------------------------------------------------------------------------ refusals that need no device
def test_engine_refusals_need_no_device():
    from types import SimpleNamespace as NS
    from gipvit.engine import FeatureExtractor, VitRunner
    VitRunner.require_attention_maps(NS(segs=[NS(N=290, crop=272)], stream_maps=True))
    VitRunner.require_attention_maps(NS(segs=[NS(N=1025, crop=512)], stream_maps=True))
    with pytest.raises(ValueError, match="1040"):
        VitRunner.require_attention_maps(NS(segs=[NS(N=1090, crop=528)], stream_maps=True))
    today = None
    for grp in (NS(segs=[NS(N=290, crop=272)], stream_maps=False), NS(segs=[NS(N=290, crop=272)]), NS(segs=[NS(N=290, crop=272)], stream_bwd=True)):
        with pytest.raises(ValueError, match="288-token limit") as ei:
            VitRunner.require_attention_maps(grp)
        today = today or str(ei.value)
        assert str(ei.value) == today
    assert today == ("attention maps: 290 tokens per image is past the 288-token limit of gv_attention_probs (images up to 256 px at patch 16); "
                     "features and intermediate layers work up to 1040 tokens")
    # stream_maps is not stream_bwd: the backward of such a group is still refused
    with pytest.raises(ValueError, match="288-token limit"):
        VitRunner.require_trainable(NS(segs=[NS(N=290, crop=272)], stream_maps=True))
    # the fp32 mode keeps its construction-time refusal, the size check its own
    with pytest.raises(ValueError, match="260"):
        FeatureExtractor("vit_tiny", 272, 2, precision="fp32", device="cpu", long_maps=True)
    with pytest.raises(ValueError, match="up to 512"):
        FeatureExtractor("vit_tiny", 528, 2, device="cpu", long_maps=True)
    fx = FeatureExtractor("vit_tiny", 272, 2, device="cpu", long_maps=True)
    assert fx.long_maps is True and fx.grp.stream_maps is True
    assert FeatureExtractor("vit_tiny", 272, 2, device="cpu").grp.stream_maps is False


def test_create_model_keeps_the_keyword_off_the_engine():
    import inspect
    from gipvit import models as M
    sig = inspect.signature(M.create_model)
    assert sig.parameters["long_maps"].default is False
    src = inspect.getsource(M.VitModel._extractor)
    assert "long_maps=self.long_maps" in src


_TRAIN = ["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "-b", "2", "--epochs", "1"]


def test_train_py_token_check_with_the_flag():
    import train
    from gipvit import cli_spec
    ok = lambda extra: train.check_token_limits(train.parse_args(_TRAIN + extra)[0])
    maps = ["--extract_features", "--extract-attention", "--long-attention-maps"]
    ok(["--img-size", "272", "--tile-size", "272"] + maps)
    ok(["--img-size", "512", "--tile-size", "512"] + maps)
    ok(["--img-size", "256", "--tile-size", "256"] + maps)
    for extra, word in ((["--img-size", "272", "--tile-size", "272", "--extract_features", "--long-attention-maps"], "--long-attention-maps"),
                        (["--img-size", "272", "--tile-size", "272", "--long-attention-maps"], "--long-attention-maps"),
                        (["--img-size", "528", "--tile-size", "528"] + maps, "1040"),
                        (["--dino", "--global-crop-size", "272", "--tile-size", "272"] + maps, "288 tokens"),
                        (["--img-size", "272", "--tile-size", "272", "--precision", "fp32"] + maps, "260"),
                        (["--img-size", "272", "--tile-size", "272", "--extract_features", "--extract-attention"], "288 tokens")):
        with pytest.raises(SystemExit, match=word):
            ok(extra)
    # the fp32 refusal and the refusal without the flag are today's messages
    with pytest.raises(SystemExit) as ei:
        ok(["--img-size", "272", "--tile-size", "272", "--precision", "fp32"] + maps)
    with pytest.raises(SystemExit) as ej:
        ok(["--img-size", "272", "--tile-size", "272", "--precision", "fp32", "--extract_features"])
    assert str(ei.value) == str(ej.value)
    assert "--long-attention-maps" not in cli_spec.REFERENCE_FLAGS and "long-attention-maps" not in cli_spec.REFERENCE_FLAGS


def test_train_py_refuses_the_flag_alone_before_any_device_work(tmp_path):
    """SystemExit before any device work (there is no device here: a run that got that far would name the GPU)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + _TRAIN + ["--output", str(tmp_path), "--img-size", "272", "--tile-size", "272",
                       "--extract_features", "--long-attention-maps"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode not in (0, None) and "--long-attention-maps" in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
