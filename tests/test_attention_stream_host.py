"""CPU: gv_attention_fwd_stream (csrc/attention_stream.hip), the streaming attention forward for 288 < N <= 1040 tokens.

What this file holds for the GPU file (tests/test_attention_stream_gpu.py), next to what it imports from
tests/test_attention_probes_host.py (builders, fp64 references and assertion functions of probes A - D):
  * STREAM_NS and the subset probe B runs on (its code-distance condition fails at four lengths),
  * two builders that force the online softmax to rescale at a chosen place -- random data never does:
      "spike"      one key, in the first / a middle / the last key block, is 3.75 x a chosen query: the running max of that row
                   jumps by ~30 there,
      "staircase"  queries get +8, keys +40 j / (N - 1) along a unit vector, ascending or descending in the key index j:
                   ascending, every key block raises every row's max; descending, none does after the first,
    with fp64 softmax / logsumexp as the reference, and `check_stream`, their assertion function (also probe D's here),
  * probe D's lse bound for this kernel (STREAM_LSE_*), measured on an MI355X,
  * `stream_model`, fp64 arithmetic with the kernel's rounding points and a key-block size, that stands in for the kernel here:
    it meets every check, and each of four faults put into it is rejected by the checks the GPU file applies."""
import math
import os
import subprocess
import sys

import pytest
import torch

from test_attention_probes_host import (CHECKS, H, MIN_DIST, N_IMG, SCALE, _raise, _require, _stack, _ulp, _within, build, check_selector,
                                        check_tie, check_uniform, min_code_distance, pad_key_shift, rb)

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the first length over the old limit, ragged 16- / 64- / 128-key edges, 384 px (577), 512 px (1 025), the cap
STREAM_NS = (289, 319, 320, 321, 383, 384, 385, 511, 512, 513, 577, 785, 1023, 1024, 1025, 1039, 1040)
SHORT_NS = (1, 17, 197, 257, 288)                          # the streaming kernel below the old limit
B_FAILS = (319, 577, 1025, 1039)                           # probe B's code distance is 7, 7, 6, 6 there (< MIN_DIST)
B_NS = tuple(N for N in STREAM_NS if N not in B_FAILS)
STREAM_MAX_N, STREAM_QBLOCK, KEY_BLOCK = 1040, 128, 64     # include/gipvit.h; keys per block of the kernel
P = N_IMG * H

# Probe D: max |lse - fp64 logsumexp| of gv_attention_fwd_stream measured on an MI355X over STREAM_NS and SHORT_NS (9 pairs each,
# the host file's seeds): 9.96e-7 (9.951e-7 rounded up), at N = 1040 (1.3e-7 at N = 1, 9.3e-7 at N = 257, 9.2e-7 at N = 1025 -- the level of the
# whole-sequence kernel, 9.8e-7; the rounding model below gives 4.5e-7 at N = 1025, the rest is the exp2 / __logf error).
# Bound = 4 x measured, as the host file's rule; test_stream_lse_bound_... holds it to a quarter of the smallest shift one
# counted pad key causes (3.35e-4, at N = 1039).
STREAM_LSE_MEASURED = 9.96e-7
STREAM_LSE_MEASURED_AT = 1040
STREAM_LSE_BOUND = 4 * STREAM_LSE_MEASURED


# ------------------------------------------------------------------------------------------------------------ builders
def key_block_of(N, where):
    """first key of the first / a middle / the last KEY_BLOCK-key block"""
    nb = (N + KEY_BLOCK - 1) // KEY_BLOCK
    return {"first": 0, "middle": nb // 2, "last": nb - 1}[where] * KEY_BLOCK


def _randn_case(seed, N):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(N, 64, generator=g).to(bf16).to(f64) for _ in range(3))
    return g, q, k, v


def _finish(q, k, v):
    s = q @ k.t() * SCALE
    return dict(q=q, k=k, v=v, o=s.softmax(-1) @ v, lse=torch.logsumexp(s, -1))


def _spike_pair(N, where, pair):
    g, q, k, v = _randn_case((7000 + ("first", "middle", "last").index(where)) * 100000 + N * 10 + pair, N)
    qi = (pair * 37 + 5) % N                                 # another row (wave, lane) in every pair
    k0 = key_block_of(N, where)
    j = min(N - 1, k0 + (pair * 7) % KEY_BLOCK)
    k[j] = rb(3.75 * q[qi])
    return dict(_finish(q, k, v), spike=torch.tensor([qi, j]))


def _staircase_pair(N, up, pair):
    g, q, k, v = _randn_case((7100 + int(up)) * 100000 + N * 10 + pair, N)
    u = torch.randn(64, generator=g).to(f64)
    u = u / u.norm()
    t = torch.arange(N, dtype=f64) / max(N - 1, 1)
    q = rb(q + 8 * u)
    k = rb(k + 40 * (t if up else 1 - t)[:, None] * u)
    return _finish(q, k, v)


_cache = {}


def build_spike(N, where):
    key = ("spike", N, where)
    if key not in _cache:
        _cache[key] = dict(_stack([_spike_pair(N, where, p) for p in range(P)]), probe=f"spike-{where}", N=N)
    return _cache[key]


def build_staircase(N, up):
    key = ("stair", N, up)
    if key not in _cache:
        _cache[key] = dict(_stack([_staircase_pair(N, up, p) for p in range(P)]), probe="staircase-" + ("up" if up else "down"), N=N)
    return _cache[key]


def check_stream(got, case, parts=("o", "lse")):
    """probe D, spike and staircase through the streaming kernel: o as check_random (2e-2 + 2e-2 |ref|: bf16 P and bf16 output), lse
    within the larger of STREAM_LSE_BOUND and 4 f32 ulp of the reference (|lse| reaches 63 on the staircase: f32 ulp 3.8e-6)."""
    bad = []
    for name in parts:
        g, r = got[name], case[name]
        tol = torch.maximum(torch.full_like(r, STREAM_LSE_BOUND), 4 * _ulp(r, 23)) if name == "lse" else 2e-2 + 2e-2 * r.abs()
        bad.append(_require(_within(g, r, tol), name, case, g, r))
    _raise(bad)


STREAM_CHECKS = dict(CHECKS, D=check_stream)


def fwd_check(probe):
    """the assertion the GPU file applies to a probe's o / lse"""
    return lambda got, case: STREAM_CHECKS[probe](got, case, parts=("o", "lse"))


# --------------------------------------------------------------------------------------------------- rounding-point model
def r32(x):
    return x.to(f32).to(f64)


MUTANTS = ("no_o_rescale", "no_sum_rescale", "pad_keys", "drop_seam_key")


def stream_model(case, block=KEY_BLOCK, scale=SCALE, mutant=None):
    """attn_fwd_stream_kernel in fp64 with its roundings: per `block` keys, f32 scores, m' = max(m, block max), alpha = exp2((m - m') c),
    p = exp2(fma(s, c, -m' c)) in f32, l = l alpha + sum p (f32), O = O alpha + V^T bf16(p) (f32), at the end O / l rounded to bf16 and
    lse = m scale + log l in f32.  `mutant` puts one fault in:
      "no_o_rescale"    O is not multiplied by alpha            "no_sum_rescale"  l is not multiplied by alpha
      "pad_keys"        the zero pad keys of the last block (score 0, V = 0) are counted
      "drop_seam_key"   the first key of every block after the first is masked out"""
    q, k, v, N = case["q"], case["k"], case["v"], case["N"]
    c = float(torch.tensor(scale * 1.4426950408889634, dtype=f32))
    s_all = r32(q @ k.transpose(-1, -2))                                  # the MFMA accumulates in f32
    m = torch.full(s_all.shape[:-1] + (1,), -math.inf, dtype=f64)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for k0 in range(0, N, block):
        s, vb = s_all[..., k0:k0 + block], v[:, k0:k0 + block]
        if mutant == "drop_seam_key" and k0 > 0:
            s = s.clone()
            s[..., 0] = -math.inf
        if mutant == "pad_keys" and k0 + block > N:
            pad = k0 + block - N
            s = torch.cat([s, torch.zeros(s.shape[:-1] + (pad,), dtype=f64)], -1)
            vb = torch.cat([vb, torch.zeros(vb.shape[0], pad, 64, dtype=f64)], 1)
        mn = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha = r32(torch.exp2(r32((m - mn) * c)))
        p = r32(torch.exp2(r32(s * c - r32(mn * c))))                     # fma: one rounding of s c - round(m' c)
        bs = p.to(f32).sum(-1, keepdim=True).to(f64)
        l = r32(l * (1.0 if mutant == "no_sum_rescale" else alpha) + bs)
        o = r32(r32(o * (1.0 if mutant == "no_o_rescale" else alpha)) + rb(p) @ vb)
        m = mn
    return dict(o=rb(r32(o * r32(1.0 / l))), lse=r32(r32(m * scale) + r32(l.log()))[..., 0])


def _rejects(check, got, case):
    try:
        check(got, case)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------- CPU tests
def _declared():
    import re
    return set(re.findall(r"^int\s+(gv_\w+)\(", open(os.path.join(ROOT, "include", "gipvit.h")).read(), re.M))


def test_both_libraries_export_the_entry_point_and_the_binding_uses_the_forward_struct():
    from gipvit import _lib
    assert "gv_attention_fwd_stream" in _declared()
    assert _lib.ENTRY_POINTS["gv_attention_fwd_stream"] is _lib.gv_attention_fwd_args
    assert hasattr(_lib.lib, "gv_attention_fwd_stream") and _lib.lib.gv_version() == 9
    assert (_lib.GV_ATTN_MAX_N, _lib.GV_ATTN_STREAM_MAX_N, _lib.GV_ATTN_STREAM_QBLOCK) == (288, STREAM_MAX_N, STREAM_QBLOCK)
    hdr = open(os.path.join(ROOT, "include", "gipvit.h")).read()
    assert f"#define GV_ATTN_STREAM_MAX_N {STREAM_MAX_N}" in hdr and f"#define GV_ATTN_STREAM_QBLOCK {STREAM_QBLOCK}" in hdr and STREAM_QBLOCK % 32 == 0
    code = "import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); assert hasattr(l, 'gv_attention_fwd_stream'); assert l.gv_version() == 9 and l.gv_act_format() == 1"
    r = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(_lib.LIB_PATH), "libgipvit_hip_f16.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_arguments_are_validated_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail with a HIP error code (> 0), not with GV_E_*."""
    from gipvit import _lib
    import ctypes as C
    buf = (C.c_char * 4096)()
    ptr = (C.addressof(buf) + 255) & ~255
    call = lambda *a: _lib.lib.gv_attention_fwd_stream(C.byref(_lib.gv_attention_fwd_args(*a)), None)
    for N in (0, STREAM_MAX_N + 1, -5):
        assert call(ptr, ptr, ptr, 1, N, 1, SCALE, 0) == -1                    # GV_E_SHAPE
        msg = _lib.lib.gv_last_error().decode()
        assert str(STREAM_MAX_N) in msg and "gv_attention_fwd_stream" in msg, msg
    assert call(ptr, ptr, ptr, 0, 300, 1, SCALE, 0) == -1 and call(ptr, ptr, ptr, 1, 300, 0, SCALE, 0) == -1
    for args in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None)):
        assert call(*args, 1, 300, 1, SCALE, 0) == -3                          # GV_E_NULL
    assert _lib.lib.gv_attention_fwd_stream(None, None) == -3
    assert call(ptr + 2, ptr, ptr, 1, 300, 1, SCALE, 0) == -2                  # GV_E_ALIGN
    for bad_scale in (0.0, -0.125):
        assert call(ptr, ptr, ptr, 1, 300, 1, bad_scale, 0) == -1 and "scale" in _lib.lib.gv_last_error().decode()
    # the old entry point keeps its limit
    assert _lib.lib.gv_attention_fwd(C.byref(_lib.gv_attention_fwd_args(ptr, ptr, ptr, 1, 289, 1, SCALE, 0)), None) == -1


def test_ops_wrapper_refuses_mismatched_dtypes():
    from gipvit import ops
    qkv = torch.zeros(300, 3 * 64, dtype=bf16)
    with pytest.raises(TypeError, match="attention_fwd_stream"):
        ops.attention_fwd_stream(qkv, 1, 300, 1, SCALE, o=torch.zeros(300, 64, dtype=f32))
    with pytest.raises(TypeError, match="no fp32 operand form"):
        ops.attention_fwd_stream(qkv.float(), 1, 300, 1, SCALE)


@pytest.mark.parametrize("N", STREAM_NS)
def test_probe_conditions_for_the_stream_lengths(N):
    """Probe A's code distance holds at every N of STREAM_NS; probe B's holds exactly on B_NS, the set the GPU file runs it on."""
    a, b = build("A", N), build("B", N)
    assert all(min_code_distance(a["codes"][p]) >= MIN_DIST for p in range(P))
    dist_b = min(min_code_distance(b["codes"][p]) for p in range(P))
    assert (dist_b >= MIN_DIST) == (N in B_NS), (N, dist_b)
    if N in B_FAILS:
        assert dist_b == {319: 7, 577: 7, 1025: 6, 1039: 6}[N]
    s = a["q"] @ a["k"].transpose(-1, -2) * SCALE
    assert float(s.max(-1).values.min()) == 128.0 and bool(((s == 128.0).sum(-1) == 1).all())
    assert float((128.0 - torch.where(s == 128.0, torch.full_like(s, -math.inf), s)).min()) >= 4 * MIN_DIST
    if N in B_NS:
        s = b["q"] @ b["k"].transpose(-1, -2) * SCALE
        assert float(s.max(-1).values.min()) == 96.0 and bool(((s == 96.0).sum(-1) <= 2).all())


def test_stream_lse_bound_is_a_quarter_of_the_pad_key_shift():
    shifts = {N: float(pad_key_shift(build("D", N)).min()) for N in STREAM_NS}
    at = min(shifts, key=shifts.get)
    assert at == 1039 and 3.3e-4 < shifts[at] < 3.4e-4, (at, shifts[at])
    assert STREAM_LSE_BOUND == 4 * STREAM_LSE_MEASURED and STREAM_LSE_BOUND <= 8.4e-5 and STREAM_LSE_BOUND <= shifts[at] / 4
    assert 2.5e-7 < STREAM_LSE_MEASURED < 4e-6                  # near 1e-6: f32 ulp at |lse| <= 8 is 4.8e-7
    assert STREAM_LSE_MEASURED_AT in STREAM_NS + SHORT_NS


@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("N", [289, 320, 1024, 1025, 1040])
def test_online_softmax_reproduces_the_exact_probes(N, block):
    """An online softmax in f32 with bf16 P gives probe A bit for bit, probe B to 1e-6 and probe C inside check_uniform."""
    a = build("A", N)
    got = stream_model(a, block)
    assert torch.equal(got["o"], a["o"])
    fwd_check("A")(got, a)
    if N in B_NS:
        b = build("B", N)
        got = stream_model(b, block)
        assert float((got["o"] - b["o"]).abs().max()) <= 1e-6
        fwd_check("B")(got, b)
    fwd_check("C")(stream_model(build("C", N), block), build("C", N))
    fwd_check("D")(stream_model(build("D", N), block), build("D", N))


@pytest.mark.parametrize("N", [321, 1025, 1040])
def test_probe_d_rejects_every_mutant(N):
    d = build("D", N)
    fwd_check("D")(stream_model(d), d)
    for mutant in MUTANTS:
        assert _rejects(fwd_check("D"), stream_model(d, mutant=mutant), d), (N, mutant)
    if N == 1025:
        err = (stream_model(d)["lse"] - d["lse"]).abs().max()
        assert float(err) < 1e-6                                    # the rounding model alone: 4.5e-7


@pytest.mark.parametrize("N", [289, 321, 1025, 1040])
def test_spike_and_staircase_hold_in_the_model_and_reject_the_rescale_mutants(N):
    """The model meets check_stream on all five; the descending staircase and the first-block spike never rescale after the first
    block (they hold the no-rescale path to the same bounds), the others reject a missing rescale of O and of the row sum."""
    cases = [build_spike(N, w) for w in ("first", "middle", "last")] + [build_staircase(N, up) for up in (True, False)]
    for case in cases:
        got = stream_model(case)
        check_stream(got, case)
        # (the model's lse error reaches 1.3 f32 ulp of the staircase's lse ~ 57: m' c is rounded before it enters the fma, so a block's
        #  p carry a common factor 2^-err(m' c) that alpha, taken from m - m', does not know -- inherent to exp2(fma(s, c, -m' c)))
    spike_rows = cases[2]["spike"]
    row_lse = cases[2]["lse"][torch.arange(P), spike_rows[:, 0]]
    assert float(row_lse.min()) > 15 and float(cases[3]["lse"].max()) > 45          # the max really jumps / climbs
    rescaling = [c for c in cases if c["probe"] in ("spike-last", "staircase-up")] + ([cases[1]] if key_block_of(N, "middle") > 0 else [])
    for case in rescaling:
        for mutant in ("no_o_rescale", "no_sum_rescale"):
            assert _rejects(check_stream, stream_model(case, mutant=mutant), case), (case["probe"], N, mutant)


def test_the_exact_probes_reject_pad_keys_and_a_dropped_seam_key():
    for N in (321, 1025):
        c = build("C", N)
        assert _rejects(fwd_check("C"), stream_model(c, mutant="pad_keys"), c)
        a = build("A", N)
        assert _rejects(fwd_check("A"), stream_model(a, mutant="drop_seam_key"), a)


_TRAIN = [sys.executable, os.path.join(ROOT, "train.py"), "--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "-b", "2", "--epochs", "1"]
_REFUSED = {
    "supervised-train": ["--img-size", "272", "--tile-size", "272"],
    "supervised-tile": ["--tile-size", "512"],
    "dino-global": ["--dino", "--global-crop-size", "272", "--tile-size", "272"],
    "dino-local": ["--dino", "--local-crop-size", "272", "--tile-size", "288"],
    "attention-maps": ["--img-size", "272", "--tile-size", "272", "--extract_features", "--extract-attention"],
    "dino-extract": ["--dino", "--global-crop-size", "272", "--tile-size", "272", "--extract_features"],
}


def test_train_py_refuses_training_and_attention_maps_past_288_tokens(tmp_path):
    """SystemExit naming the limit, before any device work (there is no device here: a run that got that far would name the GPU)."""
    procs = {name: subprocess.Popen(_TRAIN + ["--output", str(tmp_path)] + extra, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for name, extra in _REFUSED.items()}
    for name, p in procs.items():
        out, err = p.communicate(timeout=300)
        assert p.returncode not in (0, None) and "288 tokens" in err and "Traceback" not in err, (name, p.returncode, err[-2000:])


def test_train_py_token_check_lets_inference_up_to_512_through():
    import train
    ok = lambda extra: train.check_token_limits(train.parse_args(_TRAIN[2:] + extra)[0])
    ok(["--img-size", "512", "--tile-size", "512", "--extract_features"])
    ok(["--img-size", "256", "--tile-size", "256"])
    ok(["--img-size", "256", "--tile-size", "256", "--extract_features", "--extract-attention"])
    ok(["--dino"])
    for extra, word in ((["--img-size", "528", "--tile-size", "528", "--extract_features"], "1040"),
                        (["--img-size", "272", "--tile-size", "272", "--extract_features", "--precision", "fp32"], "260")):
        with pytest.raises(SystemExit, match=word):
            ok(extra)


def test_engine_refusals_need_no_device():
    """VitRunner's 288-token refusals are raised from the group's shape alone, and FeatureExtractor checks its size at construction."""
    from types import SimpleNamespace as NS
    from gipvit.engine import FeatureExtractor, VitRunner
    long_grp, short_grp = NS(segs=[NS(N=290, crop=272)]), NS(segs=[NS(N=257, crop=256)])
    VitRunner.require_trainable(short_grp)
    VitRunner.require_attention_maps(short_grp)
    with pytest.raises(ValueError, match="288-token limit"):
        VitRunner.require_trainable(long_grp)
    with pytest.raises(ValueError, match="288-token limit"):
        VitRunner.require_attention_maps(long_grp)
    with pytest.raises(ValueError, match="260"):
        FeatureExtractor("vit_tiny", 272, 2, precision="fp32", device="cpu")
    for bad in (528, 260):
        with pytest.raises(ValueError, match="up to 512"):
            FeatureExtractor("vit_tiny", bad, 2, device="cpu")
