"""GPU: gv_attention_fwd_stream (the streaming attention forward, 288 < N <= 1040 tokens) on the exact probes of
tests/test_attention_probes_host.py and the rescale-forcing cases of tests/test_attention_stream_host.py, then end to end:
FeatureExtractor / create_model / train.py --extract_features on tiles above 256 px against the CPU oracle, and the refusals of
everything that would need a backward or an attention map past 288 tokens.  The host file shows on the CPU that the assertion
functions used here reject a kernel that forgets a rescale, counts pad keys or drops a key at a block seam.  Every output buffer
has a sentinel-filled guard region behind it that must stay untouched."""
import os
import subprocess
import sys

import pytest
import torch

from test_attention_probes_host import H, N_IMG, SCALE, build, check_selector, pack_qkv, unpack_lse, unpack_rows
from test_attention_probes_gpu import _all_pairs_equal_pair0, _bits, _guarded, _guards_untouched, _nan_like, _replicated, _rows
from test_attention_stream_host import (B_NS, SHORT_NS, STREAM_CHECKS, STREAM_LSE_BOUND, STREAM_NS, STREAM_QBLOCK, build_spike, build_staircase,
                                        check_stream)

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_stream(dev, case, n_img=N_IMG, H=H, dtype=bf16, q_limit=0):
    """one case through gv_attention_fwd_stream into guarded, sentinel-filled buffers -> o [P, N, 64], lse [P, N] (fp64, CPU)"""
    from gipvit import ops
    N = case["N"]
    qkv = pack_qkv(case, n_img, H, dtype).to(dev)
    obuf, out = _guarded(n_img * N, H * 64, dtype, dev)
    lbuf, lse = _guarded(n_img * H, N, f32, dev)
    lse = lse.view(n_img, H, N)
    if q_limit:      # what the limited forward must leave as it is: NaN, compared on the bit pattern
        out.fill_(float("nan")); lse.fill_(float("nan"))
        qe = min(N, (q_limit + STREAM_QBLOCK - 1) // STREAM_QBLOCK * STREAM_QBLOCK)
    ops.attention_fwd_stream(qkv, n_img, N, H, SCALE, o=out, lse=lse, q_limit=q_limit)
    _guards_untouched((obuf, out), (lbuf, lse))
    if q_limit and qe < N:
        ov, lv = out.view(n_img, N, H * 64)[:, qe:], lse[:, :, qe:]
        assert torch.equal(_bits(ov), _bits(_nan_like(ov))) and torch.equal(_bits(lv), _bits(_nan_like(lv))), "the forward wrote behind q_limit's last block"
    return dict(o=unpack_rows(out, n_img, H), lse=unpack_lse(lse, n_img, H))


def _probe(dev, probe, N):
    case = build(probe, N)
    got = run_stream(dev, case)
    if probe == "D":
        print(f"stream probe D N={N}: max |lse - fp64 logsumexp| = {float((got['lse'] - case['lse']).abs().max()):.3e} (bound {STREAM_LSE_BOUND:.3e})")
    STREAM_CHECKS[probe](got, case, parts=("o", "lse"))


@pytest.mark.parametrize("probe,N", [(p, N) for p in "ACD" for N in STREAM_NS] + [("B", N) for N in B_NS])
def test_probe(dev, probe, N):
    """Probes A (selector: O bit exact), B (two-key tie), C (uniform: a counted pad key moves lse) and D (randn: lse within
    STREAM_LSE_BOUND of fp64 logsumexp) at every length of STREAM_NS; B on B_NS, the lengths where its code-distance condition holds
    (the host file asserts it for exactly that set).
    D, measured on an MI355X over all N: max |lse - ref| = 9.96e-7 (N = 1040); STREAM_LSE_BOUND = 4 x that = 3.98e-6."""
    _probe(dev, probe, N)


@pytest.mark.parametrize("N", SHORT_NS)
@pytest.mark.parametrize("probe", "ABCD")
def test_probe_below_the_old_limit(dev, probe, N):
    """The streaming kernel is correct for the lengths gv_attention_fwd serves too (one key block, one partial query block, ...)."""
    _probe(dev, probe, N)


@pytest.mark.parametrize("N", [289, 321, 1025, 1040])
@pytest.mark.parametrize("kind", ["spike-first", "spike-middle", "spike-last", "staircase-up", "staircase-down"])
def test_forced_rescale(dev, kind, N):
    """The running max jumps by ~30 at a chosen key block (spike), rises in every block or in none after the first (staircase):
    o within check_random's bounds, lse within max(STREAM_LSE_BOUND, 4 f32 ulp) of fp64."""
    name, arg = kind.split("-")
    case = build_spike(N, arg) if name == "spike" else build_staircase(N, arg == "up")
    got = run_stream(dev, case)
    print(f"{kind} N={N}: max |o err| {float((got['o'] - case['o']).abs().max()):.3e}, max |lse err| {float((got['lse'] - case['lse']).abs().max()):.3e}")
    check_stream(got, case)


@pytest.mark.parametrize("ql,N", [(1, 289), (33, 289), (1, 1025), (33, 1025), (129, 1025)])
def test_q_limit(dev, ql, N):
    """Probe A under q_limit: whole GV_ATTN_STREAM_QBLOCK-row blocks that hold a row < q_limit are exact (1 and 33: one block;
    129: two), every row behind them still holds the NaN it was filled with (run_stream compares the bit pattern)."""
    case = build("A", N)
    got = run_stream(dev, case, q_limit=ql)
    qe = min(N, (ql + STREAM_QBLOCK - 1) // STREAM_QBLOCK * STREAM_QBLOCK)
    assert qe == (2 if ql == 129 else 1) * STREAM_QBLOCK < N
    check_selector(_rows(got, slice(0, qe)), _rows(case, slice(0, qe)), parts=("o", "lse"))
    assert bool(torch.isnan(got["o"][:, qe:]).all()) and bool(torch.isnan(got["lse"][:, qe:]).all()), "the forward wrote behind q_limit's last block"


@pytest.mark.parametrize("N", [289, 1025])
def test_replicated_pairs_are_bit_equal(dev, N):
    """One pair's randn data in every pair of a launch of 1 539 workgroups (513 / 171 pairs, both odd; a CU holds three): o and lse
    of every pair equal pair 0 bit for bit -- a wave reading a stale K / V buffer or a missing barrier shows as a difference.
    Pair 0 itself is held to probe D's bounds."""
    from gipvit import ops
    n_img, Hh = (171, 3) if N == 289 else (57, 3)
    case1 = build("D", N, 1)
    qkv, _ = _replicated(dev, case1, n_img, Hh)
    obuf, out = _guarded(n_img * N, Hh * 64, bf16, dev)
    lbuf, lse = _guarded(n_img * Hh, N, f32, dev)
    lse = lse.view(n_img, Hh, N)
    ops.attention_fwd_stream(qkv, n_img, N, Hh, SCALE, o=out, lse=lse)
    _guards_untouched((obuf, out), (lbuf, lse))
    _all_pairs_equal_pair0(f"N={N} o", out, n_img, Hh)
    _all_pairs_equal_pair0(f"N={N} lse", lse, n_img, Hh, lse=True)
    check_stream(dict(o=unpack_rows(out[:N, :64], 1, 1), lse=lse[0, :1].cpu().to(f64)), case1)


# ------------------------------------------------------------------------------------------------------------ end to end
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("arch,img,batch", [("vit_tiny", 272, 3), ("vit_small", 272, 2), ("vit_tiny", 512, 2)])
def test_feature_extractor_matches_oracle_above_256_px(dev, arch, img, batch):
    """CLS features and logits against the CPU oracle at the gates of test_feature_extractor_matches_oracle (2e-2 / 3e-2): 272 px =
    290 tokens, the smallest size over the edge (ViT-S: the fused full-row path), and 512 px = 1 025 tokens.  At 272 the CLS row of
    intermediate_layers (every query of the last block) agrees with run() (q_limit = 1) within the same gate."""
    from gipvit.engine import FeatureExtractor
    from oracle import vit_oracle as vo
    p = vo.init_vit(arch, img, 2, seed=4)
    fx = FeatureExtractor(arch=arch, img_size=img, batch=batch, num_classes=2, device=dev)
    fx.load_state(p)
    tiles = vo.synth_tiles(batch, img, seed=21)
    feats, logits = fx.run(tiles.to(dev))
    torch.cuda.synchronize()
    x = vo.normalize_window(tiles, (0, 0, img))
    ref_f, ref_l = vo.vit_features(p, x, arch), vo.vit_logits(p, x, arch)
    rf, rl = _rel(feats, ref_f), _rel(logits, ref_l)
    print(f"{arch} {img} px: features {rf:.3e} (gate 2e-2), logits {rl:.3e} (gate 3e-2)")
    assert rf < 2e-2 and rl < 3e-2, (rf, rl)
    if img == 272:
        cls_all_q = fx.intermediate_layers(tiles.to(dev), 1)[0][:, 0]
        r = _rel(cls_all_q, feats)
        print(f"{arch} {img} px: CLS of intermediate_layers vs run: {r:.3e}")
        assert r < 2e-2, r
        with pytest.raises(ValueError, match="288-token limit"):
            fx.last_selfattention(tiles.to(dev))
        with pytest.raises(ValueError, match="288-token limit"):
            fx.run_with_attention(tiles.to(dev))


def test_model_seam_at_272_px(dev):
    """create_model(img_size=272): model(x) runs engine.forward (streaming attention) and equals the extractor's logits over the same
    weights; everything that needs the backward or an attention map raises before it launches."""
    from gipvit.engine import FeatureExtractor
    from gipvit.models import create_model
    from oracle import vit_oracle as vo
    model = create_model("vit_tiny_patch16_224", img_size=272, batch=2, device=dev, seed=3)
    eng = model.engine
    x = vo.synth_tiles(2, 272, seed=5).to(dev)
    logits = model(x).clone()
    feats = model.forward_features(x).float().clone()
    fx = FeatureExtractor("vit_tiny", 272, 2, 2, eng.mean, eng.std, dev, weights=eng.W)
    f2, l2 = fx.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(logits, l2) and torch.equal(feats, f2.float()), (float((logits - l2).abs().max()), float((feats - f2.float()).abs().max()))
    assert bool(torch.isfinite(logits).all())
    tgt = torch.zeros(2, 1, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="288-token limit"):
        eng.forward_backward(x, tgt)
    with pytest.raises(ValueError, match="288-token limit"):
        eng.step(x, tgt)
    with pytest.raises(ValueError, match="288-token limit"):
        model.get_last_selfattention(x)
    assert model.get_intermediate_layers(x, 1)[0].shape == (2, 290, 192)


def test_train_py_extracts_features_at_272_px_and_refuses_to_train(dev, tmp_path):
    import train
    fd = tmp_path / "feats"
    args = ["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "--img-size", "272", "--tile-size", "272", "-b", "4", "--epochs", "1",
            "--output", str(tmp_path), "--experiment", "fx", "--synthetic-slides", "2", "--num_tiles", "5", "--tiles_per_iter", "3",
            "--features-dir", str(fd)]
    assert train.main(args + ["--extract_features"]) == 0
    files = sorted(os.listdir(fd))
    assert files == [f"synthetic_{k}_features.pt" for k in range(2)]
    f0 = torch.load(fd / files[0], weights_only=True)
    assert f0.shape == (5, 192) and bool(torch.isfinite(f0).all()) and float(f0.std()) > 0.05
    with pytest.raises(SystemExit, match="288 tokens"):
        train.main(args)


def test_float16_build(dev):
    """tests/attention_stream_f16_worker.py in a process of its own (GIPVIT_ACT_FORMAT=f16): probes A, C, D at N = 289 and 1 025."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attention_stream_f16_worker.py")], cwd=ROOT,
                       env=dict(os.environ, GIPVIT_ACT_FORMAT="f16"), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("STREAM F16 OK"), (r.stdout[-2000:], r.stderr[-3000:])
