"""GPU: gv_attention_probs_stream (attention probabilities for 288 < N <= 1040 tokens) on the exact probes and the randn / spike
inputs of tests/test_attention_probs_stream_host.py, bit for bit against gv_attention_probs and against itself across q_rows,
forms and launch sizes, then end to end: FeatureExtractor(long_maps=True) / create_model(long_maps=True) /
train.py --long-attention-maps on tiles above 256 px against the CPU oracle.  `lse` always comes from ops.attention_fwd_stream.
The host file shows on the CPU that the assertion functions used here reject a shifted key index in the last partial tile, a
dropped key-block seam, the lse of the next row, swapped pairs, a padded row stride and shifted rows of the last query block.
p is always carved out of a sentinel-filled buffer with guards before and behind it, which must stay untouched."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import vit_oracle as vo
from test_attention_maps_host import reference_attention_and_layers
from test_attention_probes_gpu import _replicated
from test_attention_probes_host import H, N_IMG, SCALE, build, pack_qkv
from test_attention_probs_stream_host import (DP_GATE, PV_GATE, Q_ROWS, RANDOM_NS, ROWSUM_GATE, build_probs_spike, check_bitwise, check_probs_random,
                                              check_probs_selector, check_probs_uniform, softmax_ref, spike_keys)
from test_attention_stream_host import SHORT_NS, STREAM_NS, STREAM_QBLOCK

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENT = 37, -12345.0           # an odd guard: p starts on no more than a 4-byte boundary
PAIRS = N_IMG * H


def forward(dev, case, n_img=N_IMG, Hh=H, q_limit=0):
    """the case through ops.attention_fwd_stream -> (qkv, o, lse) on the device; under q_limit lse is NaN behind what the call writes"""
    from gipvit import ops
    N = case["N"]
    qkv = pack_qkv(case, n_img, Hh, ops.bf16).to(dev)
    lse = torch.full((n_img, Hh, N), float("nan"), dtype=f32, device=dev)
    o, lse = ops.attention_fwd_stream(qkv, n_img, N, Hh, SCALE, lse=lse, q_limit=q_limit)
    return qkv, o, lse


def probs(dev, qkv, lse, N, q_rows, n_img=N_IMG, Hh=H, entry="attention_probs_stream", cpu=True):
    """one call into a guarded, sentinel-filled buffer -> p f32 [n_img * Hh, q_rows, N]"""
    from gipvit import ops
    n = n_img * Hh * q_rows * N
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=f32, device=dev)
    p = buf[GUARD:GUARD + n].view(n_img, Hh, q_rows, N)
    getattr(ops, entry)(qkv, lse, n_img, N, Hh, SCALE, q_rows, p=p)
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all()), f"N={N} q_rows={q_rows}: {entry} wrote outside p"
    p = p.reshape(n_img * Hh, q_rows, N)
    return p.cpu() if cpu else p


ALL_NS = STREAM_NS + SHORT_NS


@pytest.mark.parametrize("N", ALL_NS)
def test_selector_probe(dev, N):
    """Probe A, 9 pairs, q_rows = N (block form above 16 rows) and 1 (row form): the selected key's p is 1.0 bit for bit, every other
    entry <= 2e-14."""
    case = build("A", N)
    qkv, _, lse = forward(dev, case)
    for q_rows in sorted({N, 1}):
        check_probs_selector(probs(dev, qkv, lse, N, q_rows), case, q_rows)


@pytest.mark.parametrize("N", ALL_NS)
def test_uniform_probe(dev, N):
    """Probe C (Q = 0): the N entries of a row are bitwise equal, |row sum - 1| <= 1e-4 -- a pad key counted by the forward or a key
    column left unwritten shows here."""
    case = build("C", N)
    qkv, _, lse = forward(dev, case)
    for q_rows in sorted({N, 1}):
        check_probs_uniform(probs(dev, qkv, lse, N, q_rows), case, q_rows)


def _case(kind, N):
    return build("D", N) if kind == "randn" else build_probs_spike(N, spike_keys(N)[kind == "spike-last"])


@pytest.mark.parametrize("N", RANDOM_NS)
@pytest.mark.parametrize("kind", ["randn", "spike-7", "spike-last"])
def test_random_and_spike(dev, kind, N):
    """Probe D's randn inputs and check_probs' spike (at key 7, and at the last key) for q_rows in {1, 5, 16, 17, 128, 129, N}, at the
    gates of tests/test_attention_maps_gpu.py: |dP| <= 1e-4 against torch's f32 softmax of the same 16-bit inputs,
    |row sum - 1| <= 1e-4, at q_rows = N p @ v within 2e-2 of the forward's o.  On the way, bit for bit: rows [0, q_rows) of every
    smaller q_rows (row form included) equal the q_rows = N result; lse rows >= q_rows overwritten with NaN change nothing; a second
    call on the same buffers changes nothing."""
    case = _case(kind, N)
    ref = softmax_ref(case)
    qkv, o, lse = forward(dev, case)
    full = probs(dev, qkv, lse, N, N)
    worst = [0.0, 0.0]
    for q_rows in Q_ROWS(N):
        p = full if q_rows == N else probs(dev, qkv, lse, N, q_rows)
        worst = [max(worst[0], float((p - ref[:, :q_rows]).abs().max())), max(worst[1], float((p.double().sum(-1) - 1).abs().max()))]
        check_probs_random(p, case, q_rows, ref)
        check_bitwise(p, full[:, :q_rows], case, q_rows, "rows differ from those of q_rows = N")
        if q_rows < N:
            nan_tail = lse.clone()
            nan_tail[:, :, q_rows:] = float("nan")
            check_bitwise(probs(dev, qkv, nan_tail, N, q_rows), p, case, q_rows, "p depends on lse rows >= q_rows")
        if q_rows in (1, N):
            check_bitwise(probs(dev, qkv, lse, N, q_rows), p, case, q_rows, "a second call gives other bits")
    pv = full @ case["v"].to(f32)                                                        # [P, N, 64]
    got_o = o.float().cpu().view(N_IMG, N, H, 64).permute(0, 2, 1, 3).reshape(PAIRS, N, 64)
    e = float((pv - got_o).abs().max())
    print(f"{kind} N={N}: max |dP| {worst[0]:.3e} (gate {DP_GATE}), max |row sum - 1| {worst[1]:.3e} (gate {ROWSUM_GATE}), |p v - o| {e:.3e} (gate {PV_GATE})")
    assert e <= PV_GATE, (kind, N, e)


@pytest.mark.parametrize("q_rows", [1, 128])
def test_on_the_lse_of_a_cls_only_forward(dev, q_rows):
    """N = 1 025 on the lse a q_limit = 1 forward leaves: rows 0 .. 127 are valid, everything behind them still holds the NaN it was
    filled with -- the map of those rows meets the gates and equals, bit for bit, the one taken on a full forward's lse."""
    N = 1025
    case = build("D", N)
    qkv, _, lse1 = forward(dev, case, q_limit=1)
    assert bool(torch.isnan(lse1[:, :, STREAM_QBLOCK:]).all()) and bool(torch.isfinite(lse1[:, :, :STREAM_QBLOCK]).all())
    p = probs(dev, qkv, lse1, N, q_rows)
    check_probs_random(p, case, q_rows)
    _, _, lse = forward(dev, case)
    check_bitwise(p, probs(dev, qkv, lse, N, q_rows), case, q_rows, "differs from the map on a full forward's lse")


@pytest.mark.parametrize("N", SHORT_NS)
def test_bitwise_against_attention_probs(dev, N):
    """Below the old limit, on the same lse buffer: gv_attention_probs_stream writes the bits gv_attention_probs writes, for
    q_rows in {1, 17, N} (row form and block form against the register and LDS forms of the whole-sequence call)."""
    for probe in "AD":
        case = build(probe, N)
        qkv, _, lse = forward(dev, case)
        for q_rows in sorted({min(q, N) for q in (1, 17, N)}):
            got = probs(dev, qkv, lse, N, q_rows)
            want = probs(dev, qkv, lse, N, q_rows, entry="attention_probs")
            check_bitwise(got, want, case, q_rows, "differs from gv_attention_probs")


@pytest.mark.parametrize("form,n_img,q_rows", [("row", 855, 1), ("row", 855, 16), ("block", 171, 289)])
def test_replicated_pairs_are_bit_equal(dev, form, n_img, q_rows):
    """One pair's randn data in every pair of a launch of more workgroups than the chip holds at once, N = 289 -- row form: 2 565
    workgroups of 4 waves (a CU holds at most 8); block form: 513 pairs x 3 query blocks = 1 539 workgroups (a CU holds 4) -- every
    pair's p equals pair 0 bit for bit, and pair 0 meets the randn gates."""
    from gipvit import ops
    N, Hh = 289, 3
    case1 = build("D", N, 1)
    qkv, _ = _replicated(dev, case1, n_img, Hh)
    _, lse = ops.attention_fwd_stream(qkv, n_img, N, Hh, SCALE)
    p = probs(dev, qkv, lse, N, q_rows, n_img, Hh, cpu=False)
    bits = p.view(torch.int32).view(n_img * Hh, -1)
    bad = (bits != bits[:1]).any(-1).nonzero()[:, 0].tolist()
    assert not bad, f"{form} form N={N} q_rows={q_rows}: {len(bad)} of {n_img * Hh} pairs differ from pair 0, first (image, head) {[divmod(b, Hh) for b in bad[:8]]}"
    check_probs_random(p[:1].cpu(), case1, q_rows)


# ------------------------------------------------------------------------------------------------------------ end to end
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("arch,img,batch,n_tiles", [("vit_tiny", 272, 3, 3), ("vit_small", 272, 2, 3), ("vit_tiny", 512, 2, 2)])
def test_feature_extractor_maps_match_the_oracle_above_256_px(dev, arch, img, batch, n_tiles):
    """FeatureExtractor(long_maps=True) against the oracle's last-block softmax: full map max |d| <= 1e-2 (the 16-bit gate of
    test_model_seam_against_reference and test_feature_extractor_vit_s_256); cls_only and run_with_attention are row 0 of the full map
    bit for bit; features and logits of run_with_attention are those of run bit for bit.  ViT-S runs a padded last batch (3 tiles in
    batches of 2).  Measured on an MI355X (max |d|, relative Frobenius error): see DESIGN.md section 8."""
    from gipvit.engine import FeatureExtractor
    p = vo.init_vit(arch, img, 2, seed=4)
    fx = FeatureExtractor(arch=arch, img_size=img, batch=batch, num_classes=2, device=dev, long_maps=True)
    fx.load_state(p)
    tiles = vo.synth_tiles(n_tiles, img, seed=21)
    x = tiles.to(dev)
    full = fx.last_selfattention(x).cpu()
    cls = fx.last_selfattention(x, cls_only=True).cpu()
    feats, logits, attn = fx.run_with_attention(x)
    f0, l0 = fx.run(x)
    torch.cuda.synchronize()
    N, Hh = (img // 16) ** 2 + 1, vo.ARCHS[arch]["num_heads"]
    assert full.shape == (n_tiles, Hh, N, N) and cls.shape == (n_tiles, Hh, 1, N) and attn.shape == (n_tiles, Hh, N)
    with torch.no_grad():
        ref_attn, _ = reference_attention_and_layers(p, vo.normalize_window(tiles, (0, 0, img)), arch)
    da, rf = float((full - ref_attn).abs().max()), _rel(full, ref_attn)
    print(f"{arch} {img} px, {n_tiles} tiles in batches of {batch}: attention max |d| {da:.3e} (gate 1e-2), relative Frobenius error {rf:.3e}")
    assert da <= 1e-2, da
    assert torch.equal(cls, full[:, :, :1]) and torch.equal(attn.cpu(), full[:, :, 0])
    assert torch.equal(feats, f0) and torch.equal(logits, l0)
    assert float((full.double().sum(-1) - 1).abs().max()) <= ROWSUM_GATE
    # float32 NCHW input, already normalised: the same map within the input's own rounding
    cls_f = fx.last_selfattention(vo.normalize_window(tiles, (0, 0, img)).to(dev), cls_only=True).cpu()
    assert float((cls_f - cls).abs().max()) <= 1e-2


def test_set_stain_composes_with_long_maps(dev):
    """set_stain at 272 px: the record reaches the pass (the map moves), rows still sum to 1, and switching it off gives the first
    map back bit for bit."""
    from gipvit.engine import FeatureExtractor
    from gipvit.stainnorm import normaliser_record
    fx = FeatureExtractor("vit_tiny", 272, 2, device=dev, long_maps=True)
    fx.load_state(vo.init_vit("vit_tiny", 272, 0, seed=4))
    x = vo.synth_tiles(2, 272, seed=22).to(dev)
    plain = fx.last_selfattention(x, cls_only=True).clone()
    fx.set_stain(normaliser_record(((0.65, 0.07), (0.70, 0.99), (0.29, 0.11)), (1.2, 0.8)))
    stained = fx.last_selfattention(x, cls_only=True).clone()
    assert bool(torch.isfinite(stained).all()) and float((stained.double().sum(-1) - 1).abs().max()) <= ROWSUM_GATE
    assert not torch.equal(stained, plain)
    fx.set_stain(None)
    assert torch.equal(fx.last_selfattention(x, cls_only=True), plain)


def test_model_seam_at_272_px(dev):
    """create_model(img_size=272, long_maps=True).get_last_selfattention equals the extractor's result over the same weights; the same
    model built without the keyword still raises."""
    from gipvit.engine import FeatureExtractor
    from gipvit.models import create_model
    x = vo.synth_tiles(2, 272, seed=5).to(dev)
    model = create_model("vit_tiny_patch16_224", img_size=272, batch=2, device=dev, seed=3, long_maps=True)
    a = model.get_last_selfattention(x)
    assert a.shape == (2, 3, 290, 290) and a.dtype == f32
    eng = model.engine
    fx = FeatureExtractor("vit_tiny", 272, 2, 2, eng.mean, eng.std, dev, weights=eng.W, long_maps=True)
    assert torch.equal(a, fx.last_selfattention(x))
    assert float((a.double().sum(-1) - 1).abs().max()) <= ROWSUM_GATE
    plain = create_model("vit_tiny_patch16_224", img_size=272, batch=2, device=dev, seed=3)
    with pytest.raises(ValueError, match="288-token limit"):
        plain.get_last_selfattention(x)


def test_driver_long_attention_maps(dev, tmp_path):
    """train.py --extract_features --extract-attention --long-attention-maps at 272 px writes <slide>_attention.pt (tiles, 3, 290): rows sum
    to 1 within 1e-4 and equal last_selfattention(cls_only=True) of an extractor over the same checkpoint within 1e-6 (the gates of
    test_driver_extract_attention)."""
    import train
    from gipvit import data as D, models as M
    from gipvit.engine import FeatureExtractor
    fd = tmp_path / "feats"
    args = ["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "--img-size", "272", "--tile-size", "272", "-b", "4", "--epochs", "1",
            "--output", str(tmp_path), "--experiment", "fx", "--synthetic-slides", "2", "--num_tiles", "5", "--tiles_per_iter", "3",
            "--features-dir", str(fd), "--seed", "0", "--extract_features", "--extract-attention"]
    assert train.main(args + ["--long-attention-maps"]) == 0
    files = sorted(os.listdir(fd))
    assert files == sorted([f"synthetic_{k}_features.pt" for k in range(2)] + [f"synthetic_{k}_attention.pt" for k in range(2)])
    fe = FeatureExtractor("vit_tiny", 272, 32, 2, device=dev, long_maps=True)
    fe.load_state(M.init_vit_state("vit_tiny", 272, 2, seed=0))
    slides = {}
    for mb in D.SyntheticSlides(2, 5, 272, 3, seed=0 + 99):
        slides.setdefault(mb["Slide Filename"], []).append(mb["Data"])
    for k in range(2):
        a = torch.load(fd / f"synthetic_{k}_attention.pt", weights_only=True)
        assert a.shape == (5, 3, 290) and a.dtype == f32
        assert float((a.double().sum(-1) - 1).abs().max()) <= 1e-4
        ref = fe.last_selfattention(torch.cat(slides[f"synthetic_{k}"]).to(dev), cls_only=True)[:, :, 0].cpu()
        assert float((a - ref).abs().max()) <= 1e-6
    with pytest.raises(SystemExit, match="288 tokens"):
        train.main(args)


def test_float16_build(dev):
    """tests/attention_probs_stream_f16_worker.py in a process of its own (GIPVIT_ACT_FORMAT=f16): probes A and C at N = 289 and 1 025."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attention_probs_stream_f16_worker.py")], cwd=ROOT,
                       env=dict(os.environ, GIPVIT_ACT_FORMAT="f16"), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PROBS STREAM F16 OK"), (r.stdout[-2000:], r.stderr[-3000:])
