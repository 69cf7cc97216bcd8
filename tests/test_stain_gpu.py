"""GPU: the H&E stain jitter inside the crop pass (gv_crop_augment_stain) against gipvit.stain.stain_reference (fp64) and the
PIL-pinned view oracle, its argument checks, the DINO step and the driver with --stain-jitter.

The tie rule of test 1.  The device evaluates od' and 256 exp(-od') - 1 in f32, the reference in fp64; a numpy f32 restatement
of the kernel's arithmetic was off the fp64 value by at most 2e-4 of a grey level, so a channel value whose fp64 result lies
within DELTA = 0.01 (50 x that) of a rounding tie x.5 inside (-0.5, 255.5) may come out as either neighbouring byte; every
other value must be the reference's byte.  For uniformly spread fractional parts 2 DELTA = 2 % of the values are ambiguous;
the test holds its own inputs to <= 5 %."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 0.01
TH, TW = 48, 40                     # tile_h != tile_w
SIZES = (36, 96)                    # 36: one full 32-region + a ragged 4-wide one per axis; 96: the local crops' size
SIGMAS = (0.05, 0.2, 0.5, None, 0.5, None, 0.2)        # per crop; None: on = 0
GV_E_SHAPE, GV_E_ALIGN, GV_E_NULL = -1, -2, -3


def _tiles():
    rng = np.random.default_rng(0)
    t = rng.integers(0, 256, (3, TH, TW, 3), dtype=np.uint8)
    t[1] = np.clip(np.rint(rng.normal((200, 140, 180), 40, (TH, TW, 3))), 0, 255).astype(np.uint8)       # pinkish, H&E-like
    t[2, 4:20, 3:30] = 0
    t[2, 24:44, 10:38] = 255
    return t


def _boxes(seed):
    from oracle import augment_oracle as ao
    rng = np.random.default_rng(seed)
    rows = [(n % 3, *ao.sample_box(rng, TH, TW, (0.3, 1.0)), n % 2) for n in range(7)]
    rows[2] = (2, 0, 0, TH, TW, 0)                                  # sigma = 0.5 on the whole tile of 0 / 255 blocks, both flips
    rows[4] = (2, 0, 0, TH, TW, 1)
    return np.array(rows, np.int32)


def _stains(seed):
    """Records at SIGMAS; crop 2 sits at the corner of its range that clamps at both ends (alpha up: dark pixels to 0; beta down:
    bright pixels past 255), crop 3's on = 0 record carries an A and b that must not be looked at."""
    from gipvit.stain import DT, stain_record
    rng = np.random.default_rng(seed)
    rec = np.zeros(7, DT)
    for n, s in enumerate(SIGMAS):
        if s is None:
            rec[n]["A"] = np.eye(3)
            continue
        alpha, beta = rng.uniform(1 - s, 1 + s, 3), rng.uniform(-s, s, 3)
        if n == 2:
            alpha, beta = np.array([1.45, 1.4, 1.35]), np.array([-0.45, -0.4, -0.3])
        rec[n] = stain_record(alpha, beta)
    rec[3]["A"], rec[3]["b"] = 7.0, -3.0
    return rec


def _plain_views(n):
    """n gv_view_params records with every operation off."""
    from gipvit.multicrop import ViewAugmentSampler
    a = np.zeros(n, ViewAugmentSampler.DT)
    a["bf"] = a["cf"] = a["sf"] = 1.0
    a["solar"] = -1
    return a


def _view_draws(seed):
    """ViewAugmentSampler draws for the 7 crops, with the four cases test 3 needs put on stained crops."""
    from gipvit.multicrop import ViewAugmentSampler
    rec = ViewAugmentSampler(7, 1, 1, jitter_p=0.9, gray_p=0.3, blur_p=(0.5, 0.5, 0.5), solar_p=(0.3, 0.3, 0.3), seed=seed).sample_host()[0]
    rec["n_color"][0] = 4; rec["n_color"][2] = 4           # all four colour operations: contrast is in the order
    rec["gray"][1] = 1
    rec["blur"][2] = 1; rec["blur"][4] = 1
    rec["solar"][6] = 128
    rec["n_color"][5] = 0                                  # and one crop whose RandomApply missed
    return rec


class Case:
    """Everything tests 1-4 share, computed once: tiles, boxes, records, the oracle's crops, the fp64 reference, the device's
    stain-only output D."""

    def __init__(self, dev):
        from gipvit import ops
        from gipvit.multicrop import ViewAugmentSampler
        from gipvit.stain import StainJitterSampler, stain_reference
        from oracle import augment_oracle as ao
        self.dev, self.ops = dev, ops
        self.tiles = _tiles()
        self.t_dev = torch.from_numpy(self.tiles).to(dev)
        self.stats = torch.zeros(7, dtype=torch.int64, device=dev)
        self.pack_v, self.pack_s = ViewAugmentSampler.pack, StainJitterSampler.pack
        self.size = {}
        for k, out in enumerate(SIZES):
            boxes, stains, views = _boxes(10 + k), _stains(20 + k), _view_draws(30 + k)
            crops = ao.crop_resize(self.tiles, boxes, out)
            x = np.empty(crops.shape, np.float64)
            ref = np.empty_like(crops)
            for n in range(7):
                if stains[n]["on"]:
                    x[n], ref[n] = stain_reference(crops[n], stains[n]["A"], stains[n]["b"])
                else:
                    x[n], ref[n] = crops[n], crops[n]
            b_dev = torch.from_numpy(boxes).to(dev)
            D = self.run(out, b_dev, _plain_views(7), stains)
            self.size[out] = dict(boxes=boxes, b_dev=b_dev, stains=stains, views=views, crops=crops, x=x, ref=ref, D=D)

    def run(self, out, b_dev, views, stains):
        return self.ops.crop_augment_stain(self.t_dev, b_dev, self.pack_v(views).to(self.dev), self.pack_s(stains).to(self.dev), self.stats,
                                           out).cpu().numpy()


@pytest.fixture(scope="module")
def case(dev):
    return Case(dev)


# ---- 1. the stain alone against fp64
@pytest.mark.parametrize("out", SIZES)
def test_stain_alone_against_fp64_with_the_tie_rule(case, out):
    c = case.size[out]
    x, ref, D, on = c["x"], c["ref"], c["D"], c["stains"]["on"] != 0
    assert on.sum() == 5 and (~on).sum() == 2
    frac = x - np.floor(x)
    amb = (np.abs(frac - 0.5) <= DELTA) & (x > -0.5) & (x < 255.5)
    amb[~on] = False                                                 # pass-through crops are exact
    share = amb[on].mean()
    print(f"out {out}: ambiguous share {share:.4f}, clamped low {(x[on] < -0.5).mean():.4f} high {(x[on] > 255.5).mean():.4f}, "
          f"bytes off the reference {(D != ref).sum()} of {D.size} (all on ambiguous values: {bool(np.all((D == ref) | amb))})")
    assert share <= 0.05, share
    assert (x[2] < -0.5).any() and (x[2] > 255.5).any()              # sigma = 0.5 clamps at both ends
    lo, hi = np.clip(np.floor(x), 0, 255).astype(np.uint8), np.clip(np.ceil(x), 0, 255).astype(np.uint8)
    good = (D == ref) | (amb & ((D == lo) | (D == hi)))
    if not good.all():
        n, y, xx, ch = (int(v) for v in np.argwhere(~good)[0])
        pytest.fail(f"out {out}: {int((~good).sum())} wrong bytes; first: crop {n} pixel ({y}, {xx}) channel {ch}: fp64 {x[n, y, xx, ch]!r}, "
                    f"reference byte {ref[n, y, xx, ch]}, device {D[n, y, xx, ch]}, input {c['crops'][n, y, xx].tolist()}, "
                    f"record {c['stains'][n]}")
    assert (D[on] != c["crops"][on]).mean() > 0.3                    # and the transform did something


# ---- 2. identity and pass-through
@pytest.mark.parametrize("out", SIZES)
def test_identity_and_pass_through_are_exact(case, out):
    from gipvit.stain import DT
    c = case.size[out]
    plain = case.ops.crop_resize(case.t_dev, c["b_dev"], out).cpu().numpy()
    assert np.array_equal(plain, c["crops"])
    rec = np.zeros(7, DT)
    rec["A"] = np.eye(3)
    rec["on"] = [1, 0, 1, 0, 1, 0, 1]
    rec[1]["A"], rec[1]["b"] = 7.0, -3.0                             # on = 0: A and b are not looked at
    got = case.run(out, c["b_dev"], _plain_views(7), rec)
    bad = [n for n in range(7) if not np.array_equal(got[n], plain[n])]
    assert not bad, (bad, [int(rec[n]["on"]) for n in bad])
    # every record off: gv_crop_augment itself, bit for bit, with the full view chain
    rec["on"] = 0
    want = case.ops.crop_augment(case.t_dev, c["b_dev"], case.pack_v(c["views"]).to(case.dev), case.stats, out).cpu().numpy()
    assert np.array_equal(case.run(out, c["b_dev"], c["views"], rec), want)


# ---- 3. the chain
@pytest.mark.parametrize("out", SIZES)
def test_chain_behind_the_stain_is_byte_exact(case, out):
    """crop + flip -> stain -> view chain: the full call equals the oracle's view chain applied to the device's own stain-only
    output D, byte for byte -- the stain sits directly behind the crop, in the stats pass too (contrast blends with the mean of
    the stained view), and the LDS window holds stained pixels."""
    from gipvit.multicrop import ViewAugmentSampler
    from oracle import augment_oracle as ao
    c = case.size[out]
    views, on = c["views"], c["stains"]["on"] != 0
    has = lambda f: any(f(r) and on[n] for n, r in enumerate(views))        # each case on a crop that is stained
    assert has(lambda r: 1 in list(r["order"][: r["n_color"]])), "no contrast"
    assert has(lambda r: r["gray"]) and has(lambda r: r["blur"]) and has(lambda r: r["solar"] >= 0)
    assert any(r["blur"] and 1 in list(r["order"][: r["n_color"]]) for r in views[on])
    got = case.run(out, c["b_dev"], views, c["stains"])
    dicts = ViewAugmentSampler.to_dicts(views)
    bad = []
    for n in range(7):
        ref = ao.view_augment(c["D"][n], dicts[n])
        if not np.array_equal(got[n], ref):
            bad.append((n, int((got[n] != ref).sum()), int(np.abs(got[n].astype(int) - ref.astype(int)).max())))
    assert not bad, (bad, dicts[bad[0][0]])
    # a stained crop whose first operation is contrast, and whose mean grey moved with the stain: byte-exact above only if the
    # stats pass summed the stained pixels
    mean = lambda img: int(ao.to_gray(img)[..., 0].astype(np.float64).mean() + 0.5)
    assert any(on[n] and r["n_color"] and r["order"][0] == 1 and mean(c["D"][n]) != mean(c["crops"][n]) for n, r in enumerate(views))


# ---- 4. argument checks
def test_argument_checks_come_before_any_launch(case):
    from gipvit import _lib as L
    c = case.size[36]
    dev = case.dev
    views, stains = case.pack_v(c["views"]).to(dev), case.pack_s(c["stains"]).to(dev)
    shifted = torch.zeros(stains.numel() + 4, dtype=torch.uint8, device=dev)
    out = torch.full((7, 36, 36, 3), 77, dtype=torch.uint8, device=dev)
    stats = torch.full((7,), 5, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def rc(size=36, stain=stains.data_ptr(), params=views.data_ptr()):
        v = L.gv_crop_augment_args(case.t_dev.data_ptr(), out.data_ptr(), c["b_dev"].data_ptr(), params, stats.data_ptr(), 7, 3, TH, TW, size)
        return L.lib.gv_crop_augment_stain(ctypes.byref(L.gv_crop_augment_stain_args(v, stain)), ctypes.c_void_p(stream))
    assert rc(stain=None) == GV_E_NULL and b"null" in L.lib.gv_last_error()
    assert rc(stain=shifted.data_ptr() + 1) == GV_E_ALIGN and b"stain" in L.lib.gv_last_error()
    assert rc(stain=shifted.data_ptr() + 2) == GV_E_ALIGN
    assert rc(size=34) == GV_E_SHAPE and b"multiple of 4" in L.lib.gv_last_error()
    assert rc(params=None) == GV_E_NULL                              # gv_crop_augment's own checks hold too
    assert L.lib.gv_crop_augment_stain(None, ctypes.c_void_p(stream)) == GV_E_NULL
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((stats == 5).all())      # nothing was launched: not even the zeroing of stats
    with pytest.raises(L.GipvitError, match="multiple of 4"):
        case.ops.crop_augment_stain(case.t_dev, c["b_dev"], views, stains, case.stats, 34)
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((out == 77).all())


# ---- 5. the engine
def test_engine_step_with_stains(dev):
    import math
    from gipvit import ops
    from gipvit.engine import DinoEngine
    from gipvit.multicrop import MultiCropSampler, ViewAugmentSampler
    from gipvit.stain import StainJitterSampler
    from oracle import step_oracle as so, vit_oracle as vo
    tiles = vo.synth_tiles(2, 256, seed=11).to(dev)
    orc = so.DinoOracle(arch="vit_tiny", img_size=224, out_dim=1024, seed=0, n_local=2)        # the weights every engine below starts from

    def run(with_stains, sigma=0.2):
        eng = DinoEngine(arch="vit_tiny", img_size=224, out_dim=1024, batch=2, n_local=2, device=dev)
        eng.load_state(orc.p, orc.hp)
        boxes = MultiCropSampler(batch=2, tile=256, n_local=2, seed=11).sample(dev)
        views = ViewAugmentSampler(2, 2, 2, seed=12).sample(dev)
        stains = StainJitterSampler(2, 2, 2, sigma, seed=13).sample(dev) if with_stains else None
        loss = float(eng.step(tiles, boxes=boxes, views=views, stains=stains))
        torch.cuda.synchronize()
        return eng, boxes, views, stains, loss
    eng, boxes, views, stains, loss = run(True)
    assert math.isfinite(loss) and loss > 0
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    assert torch.equal(eng._gcrops, ops.crop_augment_stain(tiles, boxes[0], views[0], stains[0], stats, 224))
    assert torch.equal(eng._lcrops, ops.crop_augment_stain(tiles, boxes[1], views[1], stains[1], stats, 96))
    twin = run(True)[0]
    assert torch.equal(twin._gcrops, eng._gcrops) and torch.equal(twin._lcrops, eng._lcrops)
    off, _, _, _, loss_off = run(False)
    assert math.isfinite(loss_off)
    assert not torch.equal(off._gcrops, eng._gcrops) and not torch.equal(off._lcrops, eng._lcrops)
    assert torch.equal(off._gcrops, ops.crop_augment(tiles, boxes[0], views[0], stats, 224))
    with pytest.raises(ValueError, match="stains"):
        eng.step(tiles, boxes=boxes, stains=stains)


# ---- 6. the driver
def test_train_dino_stain_jitter(dev, tmp_path, caplog):
    """--stain-jitter through the driver: the run trains, says at start-up that the jitter is on, and its checkpoint carries the
    sampler's stream; the same command without the flag writes no such stream."""
    sys.path.insert(0, ROOT)
    import train
    base = ["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--out-dim", "1024", "--batches-per-epoch", "2", "--lr", "1e-4",
            "--epochs", "1", "--log-interval", "1", "--output", str(tmp_path), "--seed", "7", "--no-validate", "--random-crops", "--view-augment"]
    with caplog.at_level("INFO"):
        assert train.main(base + ["--experiment", "stain", "--stain-jitter", "0.05"]) == 0
    line = [m for m in caplog.messages if "stain jitter" in m]
    assert len(line) == 1 and "sigma 0.05" in line[0] and "prob 1" in line[0]
    caplog.clear()
    with caplog.at_level("INFO"):
        assert train.main(base + ["--experiment", "plain"]) == 0
    assert not [m for m in caplog.messages if "stain jitter" in m]
    ck = {n: torch.load(tmp_path / n / "last.pth.tar", weights_only=True) for n in ("stain", "plain")}
    assert {"crops", "views", "stain"} <= set(ck["stain"]["host_rng"]) and "stain" in ck["stain"]["host_rng_ranks"]["states"][0]
    assert "stain" not in ck["plain"]["host_rng"] and "stain" not in ck["plain"]["host_rng_ranks"]["states"][0]
    assert {"crops", "views"} <= set(ck["plain"]["host_rng"])
    w = {n: ck[n]["state_dict"]["backbone.blocks.0.attn.qkv.weight"] for n in ck}
    assert torch.isfinite(w["stain"]).all() and not torch.equal(w["stain"], w["plain"])
