"""Random erasing on the device: gv_patchify_erase / gv_patchify_nchw_erase (and their _f32 forms) against the kernels without the
table and against gipvit.erasing's restatements (apply_reference, noise_reference), the supervised step with a plan, the driver.

Value boxes are held bit for bit.  Noise pixels of the f32 entries are held to 1e-5 absolute against noise_reference: |z| <= 5.77
(u1 >= 2^-24), the f32 formula's own error against the double evaluation is bounded by about 6e-6 (the rounding of the cosine's
argument, half an ulp of a value below 2 pi, times 5.77, is 1.4e-6 of it; the logarithm's and the square root's roundings are
relative and smaller), the rest allows for 1-2 ulp device logf / cosf.  The measured maximum is printed."""
import csv
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixup_worker as mw      # noqa: E402

pytestmark = pytest.mark.gpu
NOISE_TOL = 1e-5
WIN = (5, 7)                   # the uint8 tests' window inside a 96-px tile: an odd origin


def _rows32(n, crop, dev):
    return torch.empty(n * (crop // 16) ** 2, 768, dtype=torch.float32, device=dev)


def _u8(ops, td, crop, dev, f32=True, **kw):
    from oracle import vit_oracle as vo
    out = _rows32(td.shape[0], crop, dev) if f32 else None
    return ops.patchify(td, [WIN], crop, vo.MEAN_RON, vo.STD_RON, out=out, **kw).cpu()


def _nchw(ops, src, win, crop, dev, f32=True, **kw):
    out = _rows32(src.shape[0], crop, dev) if f32 else None
    return ops.patchify_nchw(src, [win], crop, out=out, **kw).cpu()


def _er(plan):
    return {"erase": (plan.table, plan.seed)}


def _box_mask(rows, S):
    """bool [B, 1, S, S]: the pixels the rows erase."""
    from gipvit.erasing import ErasePlan, apply_reference
    r = rows.copy()
    r["mode"][(r["mode"] == 1) | (r["mode"] == 2)] = 1
    r["value"][:] = 1.0
    return apply_reference(torch.zeros(len(rows), 3, S, S), ErasePlan(r)).bool()[:, :1]


def _edge_tables(B, S):
    """Two tables of value rows for one batch of B >= 4 images: A the awkward boxes, B the full row, the refused rows and boxes that
    leave the window."""
    from gipvit.erasing import ErasePlan
    a = ErasePlan.make_rows(B)
    add = ErasePlan.add_box
    add(a, 0, (0, 5, 0, 7), (0.5, -1.5, 2.25))                     # touches the window's top-left, corners off the 4 / 16 grid
    add(a, 0, (S - 3, S, S - 21, S), (-0.75, 0.125, 3.0))          # touches its bottom-right
    add(a, 0, (33, 34, 17, 18), (9.0, 8.0, 7.0))                   # 1 x 1
    add(a, 0, (13, 35, 11, 38), (1.0, 2.0, 3.0))                   # crosses patch boundaries in both directions
    add(a, 1, (1, S, 0, S - 1), (0.0, 0.0, 0.0))                   # all but one row and one column ('const')
    add(a, 2, (10, 30, 10, 30), (1.5, 1.5, 1.5))                   # two overlapping boxes, different values: the later one wins
    add(a, 2, (20, 41, 25, 50), (-2.5, 0.25, 4.0))
    add(a, 3, (16, 32, 16, 48), (0.1, 0.2, 0.3))                   # exactly on the patch grid: whole runs / items
    if S > 256:                                                   # the boundary between two strips of 16 patches
        add(a, 3, (100, 130, 250, 262), (6.0, 5.0, 4.0))
        add(a, 2, (S - 40, S - 2, 255, 257), (-6.0, -5.0, -4.0))
    b = ErasePlan.make_rows(B)
    g = np.random.default_rng(S)
    for k in range(8):                                            # an image with 8 boxes
        y, x = int(g.integers(0, S - 20)), int(g.integers(0, S - 20))
        add(b, 0, (y, y + int(g.integers(1, 20)), x, x + int(g.integers(1, 20))), g.standard_normal(3))
    add(b, 1, (-7, 9, S - 9, S + 100), (1.0, 1.0, 1.0))           # clamped to the window
    add(b, 1, (40, 30, 5, 50), (2.0, 2.0, 2.0))                   # empty
    add(b, 2, (3, 50, 3, 50), (5.0, 5.0, 5.0)); b["n_box"][2] = 9   # n_box = 9: the row is off
    add(b, 3, (3, 50, 3, 50), (5.0, 5.0, 5.0)); b["mode"][3] = 7    # mode 7: the row is off
    return a, b


def _fold(rows, B):
    """The tables are written for 4 images; a batch of 2 takes images 0 and 3's boxes onto 0, 1 and 2's onto 1."""
    if B >= 4:
        return rows
    from gipvit.erasing import ErasePlan
    out = ErasePlan.make_rows(B)
    for i, r in enumerate(rows):
        if int(r["mode"]) != 1 or not 0 <= int(r["n_box"]) <= 8:
            continue
        for k in range(int(r["n_box"])):
            ErasePlan.add_box(out, (0, 1, 1, 0)[i], r["box"][k], r["value"][k])
    return out


def _fill(B, dev):
    fill = torch.zeros(B, 8)
    fill[1] = torch.tensor([10., 50., 20., 70., 0.5, -0.25, 1.5, 1.])
    return fill.to(dev)


# ------------------------------------------------------------------ kernels
def test_off_table_equals_the_kernels_without_it(dev):
    """An all-off table: with mix = NULL all four entries are bit-identical to the plain kernels, with a mix table to the mix kernels."""
    from gipvit import ops
    from gipvit.erasing import ErasePlan
    from gipvit.mixup import MixPlan
    from oracle import vit_oracle as vo
    B, S = 8, 64
    off = _er(ErasePlan(ErasePlan.make_rows(B), seed=123, device=dev))
    mix = MixPlan(mw.hand_plan(B, S), dev).table
    td = vo.synth_tiles(B, 96, seed=3).to(dev)
    x = torch.randn(B, 3, 80, 88, generator=torch.Generator().manual_seed(1)).to(dev)
    for f32 in (True, False):
        for kw in ({}, {"mix": mix}, {"fill": _fill(B, dev)}, {"mix": mix, "fill": _fill(B, dev)}):
            mw.assert_bits_equal(_u8(ops, td, S, dev, f32, **kw, **off), _u8(ops, td, S, dev, f32, **kw), f"u8 f32={f32} {sorted(kw)}")
        for kw in ({}, {"mix": mix}):
            for win in ((0, 0), (3, 5)):
                mw.assert_bits_equal(_nchw(ops, x, win, S, dev, f32, **kw, **off), _nchw(ops, x, win, S, dev, f32, **kw), f"nchw f32={f32} {sorted(kw)} {win}")
    with pytest.raises(ValueError, match="one crop window"):
        ops.patchify_nchw(x, [(0, 0), (0, 0)], 32, **off)
    with pytest.raises(ValueError, match="gv_erase_row"):
        ops.patchify_nchw(x, [(0, 0)], S, erase=(off["erase"][0][:-8], 0))


def test_value_boxes_u8_exact(dev):
    """B = 4, S = 64, uint8: the f32 entry equals apply_reference of the plain kernel's own f32 rows, the 16-bit entry its .to()."""
    from gipvit import ops
    from gipvit.erasing import ErasePlan, apply_reference
    from oracle import vit_oracle as vo
    B, S = 4, 64
    td = vo.synth_tiles(B, 96, seed=7).to(dev)
    for kw in ({}, {"fill": _fill(B, dev)}):
        R = mw.images_of(_u8(ops, td, S, dev, **kw), B, S)
        for name, rows in zip("AB", _edge_tables(B, S)):
            plan = ErasePlan(rows, seed=1, device=dev)
            ref = mw.rows_of(apply_reference(R, plan), S)
            assert not torch.equal(ref, mw.rows_of(R, S))
            mw.assert_bits_equal(_u8(ops, td, S, dev, **kw, **_er(plan)), ref, f"u8 f32 table {name} {sorted(kw)}")
            mw.assert_bits_equal(_u8(ops, td, S, dev, False, **kw, **_er(plan)), ref.to(ops.bf16), f"u8 16-bit table {name} {sorted(kw)}")


@pytest.mark.parametrize("B,S", [(4, 64), (2, 272)])
def test_value_boxes_nchw_exact(dev, B, S):
    """float32 NCHW: contiguous, a sliced (strided) batch, and windows at an odd column (the 4-byte-load path); S = 272 makes a
    patch row span two strips of 16 patches."""
    from gipvit import ops
    from gipvit.erasing import ErasePlan, apply_reference
    g = torch.Generator().manual_seed(17 + S)
    x = 3.0 * torch.randn(B, 3, S + 16, S + 24, generator=g)
    x[0, 0, 5, 7] = float("inf"); x[1, 1, 30, 40] = float("nan"); x[0, 1, 20, 21] = -0.0
    big = torch.randn(B + 3, 3, S + 26, S + 35, generator=g)
    sl = big[2:2 + B, :, 3:S + 19, 7:S + 31]                       # N / C / H strides of the big batch, odd offset
    for src_cpu, src in ((x, x.to(dev)), (sl, big.to(dev)[2:2 + B, :, 3:S + 19, 7:S + 31])):
        for win in ((0, 0), (3, 5), (16, 24)):
            w = src_cpu[:, :, win[0]:win[0] + S, win[1]:win[1] + S]
            for name, rows in zip("AB", _edge_tables(4, S)):
                plan = ErasePlan(_fold(rows, B), seed=1, device=dev)
                ref = mw.rows_of(apply_reference(w.contiguous(), plan), S)
                mw.assert_bits_equal(_nchw(ops, src, win, S, dev, **_er(plan)), ref, f"nchw f32 table {name} {win} {src.stride()}")
                mw.assert_bits_equal(_nchw(ops, src, win, S, dev, False, **_er(plan)), ref.to(ops.bf16), f"nchw 16-bit table {name} {win} {src.stride()}")


def _noise_rows(B, S):
    """Hand boxes (the edges of _edge_tables, as noise rows) for images 0 .. 2, the sampler's ('pixel', count 3) for the rest."""
    from gipvit.erasing import ERASE_NOISE, ErasePlan, EraseSampler
    rows, _ = EraseSampler(1.0, "pixel", 3, B, S, seed=9).sample_host()
    a, _b = _edge_tables(4, S)
    for i in range(3):
        rows[i] = a[i]
        rows["mode"][i] = ERASE_NOISE
    return rows


def test_noise_boxes(dev):
    from gipvit import ops
    from gipvit.erasing import ErasePlan, noise_reference
    from oracle import vit_oracle as vo
    B, S, seed = 6, 64, 0xC0FFEE11
    rows = _noise_rows(B, S)
    plan, plan2 = ErasePlan(rows, seed, dev), ErasePlan(rows, seed + 1, dev)
    inside = _box_mask(rows, S).expand(B, 3, S, S)
    assert 0.1 < float(inside.float().mean()) < 0.9
    z = torch.from_numpy(noise_reference(seed, B, S))
    td = vo.synth_tiles(B, 96, seed=7).to(dev)
    x = torch.randn(B, 3, 80, 88, generator=torch.Generator().manual_seed(2)).to(dev)
    got = {}
    for form, run in (("u8", lambda f32, **kw: _u8(ops, td, S, dev, f32, **kw)), ("nchw", lambda f32, **kw: _nchw(ops, x, (3, 5), S, dev, f32, **kw))):
        plain = mw.images_of(run(True), B, S)
        rows32 = run(True, **_er(plan))
        e32 = mw.images_of(rows32, B, S)
        mw.assert_bits_equal(e32[~inside], plain[~inside], f"{form}: outside the boxes")
        err = float((e32.double() - z)[inside].abs().max())
        print(f"[erase noise {form}] max |device - noise_reference| inside the boxes: {err:.3e} over {int(inside.sum())} values")
        assert err <= NOISE_TOL, err
        mw.assert_bits_equal(run(False, **_er(plan)), rows32.to(ops.bf16), f"{form}: 16-bit entry = .to() of the f32 entry")
        other = mw.images_of(run(True, **_er(plan2)), B, S)
        assert not torch.equal(other[inside], e32[inside]) and float((other[inside] == e32[inside]).float().mean()) < 1e-3
        mw.assert_bits_equal(other[~inside], plain[~inside], f"{form}: outside the boxes, second seed")
        got[form] = e32
    mw.assert_bits_equal(got["u8"][inside], got["nchw"][inside], "same seed: the u8 and the NCHW kernel agree bit for bit inside the boxes")


def test_erase_after_mix(dev):
    """Blend, paste and copy rows + erase boxes that overlap the paste boxes: apply_reference of the mix kernel's own f32 output,
    bit for bit outside noise pixels (those: 1e-5 against noise_reference)."""
    from gipvit import ops
    from gipvit.erasing import ERASE_NOISE, ErasePlan, apply_reference, noise_reference
    from gipvit.mixup import MixPlan
    from oracle import vit_oracle as vo
    B, S, seed = 8, 64, 77
    mrows = mw.hand_plan(B, S)                                     # paste boxes: (0,64,0,10) (5,5,3,9) (1,33,3,29) (7,25,9,23) (0,64,0,64)
    mix = MixPlan(mrows, dev).table
    assert set(mrows["mode"].tolist()) == {0, 1, 2}
    rows = ErasePlan.make_rows(B)
    add = ErasePlan.add_box
    add(rows, 0, (3, 40, 5, 37), (1.0, -1.0, 0.5))                # a blend row
    add(rows, 1, (10, 30, 4, 20), (0.25, 0.5, 0.75))              # cut by the paste box's edge x = 10
    add(rows, 3, (0, 16, 0, 32), mode=ERASE_NOISE)                # inside and around the paste box (1,33,3,29)
    add(rows, 3, (20, 50, 20, 40), mode=ERASE_NOISE)
    add(rows, 4, (16, 32, 0, 64), (2.0, 2.0, 2.0))                # whole runs of a paste row
    add(rows, 5, (1, 63, 1, 63), mode=ERASE_NOISE)                # the partner replaces the whole window, then nearly all of it is erased
    add(rows, 6, (30, 35, 30, 35), (3.0, 3.0, 3.0))               # a copy row
    plan = ErasePlan(rows, seed, dev)
    noisy = _box_mask(rows[[3, 5]], S).expand(2, 3, S, S)
    z = torch.from_numpy(noise_reference(seed, B, S))[[3, 5]]
    td = vo.synth_tiles(B, 96, seed=11).to(dev)
    x = torch.randn(B, 3, 80, 88, generator=torch.Generator().manual_seed(3)).to(dev)
    runs = [("u8", lambda f32, **kw: _u8(ops, td, S, dev, f32, mix=mix, **kw)),
            ("u8 fill", lambda f32, **kw: _u8(ops, td, S, dev, f32, mix=mix, fill=_fill(B, dev), **kw)),
            ("nchw", lambda f32, **kw: _nchw(ops, x, (3, 5), S, dev, f32, mix=mix, **kw))]
    for form, run in runs:
        mixed = mw.images_of(run(True), B, S)
        ref = apply_reference(mixed, plan)
        rows32 = run(True, **_er(plan))
        e32 = mw.images_of(rows32, B, S)
        keep = torch.ones(B, 3, S, S, dtype=torch.bool)
        keep[[3, 5]] = ~noisy
        mw.assert_bits_equal(e32[keep], ref[keep], f"{form}: every pixel that is not noise")
        err = float((e32[[3, 5]].double() - z)[noisy].abs().max())
        print(f"[erase after mix {form}] noise pixels: max err {err:.3e}")
        assert err <= NOISE_TOL
        mw.assert_bits_equal(run(False, **_er(plan)), rows32.to(ops.bf16), f"{form}: 16-bit entry")


# ------------------------------------------------------------------ the step
def test_supervised_step_with_erase_plan(dev):
    """ViT-T, 64 px, B = 8, 'rand' boxes: the patch rows the engine fills are bit-identical to those a plain forward_backward fills
    from apply_reference's batch, the losses agree within 1e-3 (the bf16 loss gate) -- float32 NCHW input, and uint8
    input with fill= present; erase= with mix= runs; the DINO engine has no such argument."""
    from gipvit import ops
    from gipvit.engine import DinoEngine, SupervisedEngine
    from gipvit.erasing import EraseSampler, apply_reference
    from gipvit.mixup import MixPlan
    from gipvit.models import init_vit_state
    from oracle import vit_oracle as vo
    B, S = 8, 64
    plan = EraseSampler(0.75, "rand", 3, B, S, seed=4).sample(dev)
    assert 0 < int((plan.rows["n_box"] > 0).sum()) and set(plan.rows["mode"].tolist()) <= {0, 1}
    tgt = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1]).view(B, 1).to(dev)
    st = init_vit_state("vit_tiny", S, 2, seed=0)
    eng = SupervisedEngine(arch="vit_tiny", img_size=S, num_classes=2, batch=B, device=dev)          # lsce stays legal: labels are unchanged
    eng.load_state(st)
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(8))
    tiles = vo.synth_tiles(B, S, seed=21).to(dev)
    fill = _fill(B, dev)
    fill[1, :4] = torch.tensor([10., 50., 20., 60.])
    norm = mw.images_of(ops.patchify(tiles, [(0, 0)], S, vo.MEAN_RON, vo.STD_RON, out=_rows32(B, S, dev), fill=fill).cpu(), B, S)
    for form, src, kw, base in (("f32", x.to(dev), {}, x), ("u8 + fill", tiles, {"fill": fill}, norm)):
        eng.forward_backward(src, tgt, erase=plan, **kw)
        torch.cuda.synchronize()
        rows_e, loss_e, g_e = eng.grp.segs[0].patches.clone(), float(eng.loss), eng.grads()["patch_embed.proj.weight"].clone()
        eng.forward_backward(apply_reference(base, plan).to(dev), tgt)
        torch.cuda.synchronize()
        mw.assert_bits_equal(rows_e, eng.grp.segs[0].patches, f"{form}: patch rows")
        print(f"[erase step {form}] loss {loss_e:.6f}, from the restated batch {float(eng.loss):.6f}")
        assert math.isfinite(loss_e) and abs(loss_e - float(eng.loss)) <= 1e-3
        assert float((g_e - eng.grads()["patch_embed.proj.weight"]).norm()) <= 1e-2 * float(g_e.norm())
        eng.forward_backward(src, tgt, **kw)
        torch.cuda.synchronize()
        assert not torch.equal(rows_e, eng.grp.segs[0].patches)
    soft = SupervisedEngine(arch="vit_tiny", img_size=S, num_classes=2, batch=B, device=dev, loss="soft_ce")
    soft.load_state(st)
    mrows = MixPlan.make_rows(B)
    MixPlan.set_row(mrows, 0, 0.3, None); MixPlan.set_row(mrows, B - 1, 0.3, None); MixPlan.set_row(mrows, 2, 0.8, (7, 37, 9, 31))
    assert math.isfinite(float(soft.step(tiles, tgt, fill=fill, mix=MixPlan(mrows, dev), erase=plan)))
    assert math.isfinite(float(soft.step(x.to(dev), tgt, mix=MixPlan(mrows, dev), erase=EraseSampler(1.0, "pixel", 2, B, S, seed=1).sample(dev))))
    e32 = SupervisedEngine(arch="vit_tiny", img_size=S, num_classes=2, batch=B, device=dev, precision="fp32")
    e32.load_state(st)
    e32.forward_backward(x.to(dev), tgt, erase=plan)
    torch.cuda.synchronize()
    mw.assert_bits_equal(e32.grp.segs[0].patches.cpu(), mw.rows_of(apply_reference(x, plan), S), "fp32 engine: f32 patch rows")
    assert "erase" not in inspect.signature(DinoEngine.step).parameters and "erase" not in inspect.signature(DinoEngine.forward_backward).parameters


# ------------------------------------------------------------------ the driver
def test_train_random_erasing_through_the_driver(dev, tmp_path, caplog, monkeypatch):
    sys.path.insert(0, ROOT)
    import train
    from gipvit.engine import SupervisedEngine
    from gipvit.erasing import ERASE_NOISE, ErasePlan

    def common(exp):          # the argument list of test_train_supervised_and_resume
        return ["--supervised", "--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "--num-classes", "2", "--img-size", "64", "--tile-size", "64",
                "-b", "8", "--batches-per-epoch", "6", "--opt", "adam", "--lr-base", "0.001", "--sched", "cosine", "--warmup-epochs", "1",
                "--log-interval", "2", "--output", str(tmp_path), "--experiment", exp, "--subexperiment", "sub", "--seed", "1",
                "--synthetic-slides", "4", "--num_tiles", "12", "--tiles_per_iter", "5"]
    ef = ["--reprob", "0.5", "--remode", "pixel"]
    seen, fwd = [], []
    orig, orig_fwd = SupervisedEngine.step, SupervisedEngine.forward
    monkeypatch.setattr(SupervisedEngine, "step", lambda self, *a, **k: (seen.append(k.get("erase")), orig(self, *a, **k))[1])
    monkeypatch.setattr(SupervisedEngine, "forward", lambda self, *a, **k: (fwd.append(sorted(k)), orig_fwd(self, *a, **k))[1])
    with caplog.at_level("INFO"):
        assert train.main(common("erase") + ef + ["--epochs", "1"]) == 0
    assert len(seen) == 6 and all(isinstance(p, ErasePlan) for p in seen)
    assert all("erase" not in k for k in fwd)                               # validation never erases
    modes = np.concatenate([p.rows["mode"] for p in seen])
    assert set(modes.tolist()) == {0, ERASE_NOISE} and len({p.seed for p in seen}) == 6
    assert any("random erasing on the device: reprob 0.5 remode pixel recount 1" in m for m in caplog.messages)
    for m in caplog.messages:
        if "accepted for CLI compatibility" in m:
            assert not any(f in m.split() for f in ("--reprob", "--remode", "--recount")), m
    rows = list(csv.DictReader(open(tmp_path / "erase" / "sub" / "summary.csv")))
    assert len(rows) == 1 and np.isfinite(float(rows[0]["train_loss"])) and np.isfinite(float(rows[0]["eval_loss"]))
    # the erase stream rides in the checkpoint: the resumed run goes on from it
    ck = torch.load(tmp_path / "erase" / "sub" / "last.pth.tar", weights_only=True)
    assert "erase" in ck["host_rng"]
    args, _ = train.parse_args(common("erase") + ef)
    whole = train.build_erase_sampler(args, 64, 0)
    for _ in range(6):
        whole.sample_host()
    assert ck["host_rng"]["erase"] == whole.state_dict()["rng"]
    del seen[:]
    assert train.main(common("erase") + ef + ["--epochs", "2", "--resume", str(tmp_path / "erase" / "sub" / "last.pth.tar")]) == 0
    assert len(seen) == 6
    nxt, nseed = whole.sample_host()
    assert np.array_equal(seen[0].rows, nxt) and seen[0].seed == nseed
    assert [int(r["epoch"]) for r in csv.DictReader(open(tmp_path / "erase" / "sub" / "summary.csv"))] == [0, 1]
    # --reprob 0 (the default): no sampler, no keyword
    del seen[:]
    assert train.main(common("plain") + ["--remode", "const", "--epochs", "1"]) == 0
    assert seen == [None] * 6
    assert "erase" not in torch.load(tmp_path / "plain" / "sub" / "last.pth.tar", weights_only=True)["host_rng"]
