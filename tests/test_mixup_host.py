"""CPU: the host side of supervised mixup / cutmix -- gipvit.mixup's draws (timm Mixup restated), the dense target of the
restatement the GPU tests check against, the new C-ABI entry points' argument validation, and the driver's flag handling."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixup_worker as mw      # noqa: E402

NINE = ("--mixup", "--cutmix", "--cutmix-minmax", "--mixup-prob", "--mixup-switch-prob", "--mixup-mode", "--mixup-off-epoch",
        "--bce-loss", "--bce-target-thresh")


def _sampler(**kw):
    from gipvit.mixup import MixSampler
    d = dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch", batch=8, img_size=64, seed=3)
    d.update(kw)
    return MixSampler(**d)


def test_sampler_streams_and_state():
    a, b = _sampler(mode="elem"), _sampler(mode="elem")
    for _ in range(5):
        assert np.array_equal(a.sample_host(), b.sample_host())
    assert not np.array_equal(_sampler(mode="elem", seed=4).sample_host(), _sampler(mode="elem", seed=5).sample_host())
    sd = a.state_dict()
    assert isinstance(sd["rng"], str)                       # plain types: the checkpoint loads with weights_only=True
    nxt = [a.sample_host() for _ in range(3)]
    c = _sampler(mode="elem", seed=99)
    c.load_state_dict(sd)
    for r in nxt:
        assert np.array_equal(c.sample_host(), r)
    # --mixup-off-epoch: disabled -> no plan, and no draw is consumed
    st = a.rng.bit_generator.state
    a.enabled = False
    assert a.sample() is None and a.sample_host() is None and a.rng.bit_generator.state == st


def test_sampler_rows():
    from gipvit import _lib
    from gipvit.mixup import MixPlan, ROW_DT
    assert ROW_DT.itemsize == ctypes.sizeof(_lib.gv_mix_row) == 32
    assert [ROW_DT.fields[n][1] for n in ROW_DT.names] == [getattr(_lib.gv_mix_row, n).offset for n, _ in _lib.gv_mix_row._fields_]
    B, S = 8, 64
    for mode in ("batch", "pair", "elem"):
        s = _sampler(mode=mode)
        for _ in range(40):
            rows = s.sample_host()
            assert rows["partner"].tolist() == [B - 1 - i for i in range(B)]
            for r in rows:
                lam = float(r["lam"])
                if r["mode"] == 0:
                    assert lam == 1.0 and r["one_minus_lam"] == 0.0
                elif r["mode"] == 1:
                    assert 0.0 <= lam < 1.0 and abs(lam + float(r["one_minus_lam"]) - 1.0) < 1e-6
                else:      # box inside the image, lam == 1 - area / HW exactly (correct_lam), never an empty box
                    assert 0 <= r["yl"] < r["yh"] <= S and 0 <= r["xl"] < r["xh"] <= S
                    area = int(r["yh"] - r["yl"]) * int(r["xh"] - r["xl"])
                    assert r["lam"] == np.float32(1.0 - area / float(S * S)) and r["one_minus_lam"] == np.float32(area / float(S * S))
            if mode == "batch":
                assert all(rows[i].tolist()[1:] == rows[0].tolist()[1:] for i in range(B))
            if mode == "pair":
                for i in range(B // 2):
                    assert rows[i].tolist()[1:] == rows[B - 1 - i].tolist()[1:]
    assert set(_sampler(prob=0.0, mode="elem").sample_host()["mode"].tolist()) == {0}
    cut_only = _sampler(mixup_alpha=0.0, cutmix_alpha=1.0, mode="elem")
    assert all(1 not in cut_only.sample_host()["mode"] for _ in range(50))
    mm = _sampler(mixup_alpha=0.0, cutmix_alpha=0.0, cutmix_minmax=(0.25, 0.75), mode="elem")
    assert mm.cutmix_alpha == 1.0
    for _ in range(50):
        for r in mm.sample_host():
            assert r["mode"] == 2 and 16 <= r["yh"] - r["yl"] < 48 and 16 <= r["xh"] - r["xl"] < 48 and r["yh"] <= 64 and r["xh"] <= 64
    # the device form
    p = MixPlan(_sampler(mode="elem").sample_host())
    assert p.table.dtype == torch.uint8 and p.table.numel() == 8 * 32 and p.partner.dtype == torch.int32 and p.lam.dtype == torch.float32
    assert np.array_equal(p.table.numpy().view(ROW_DT), p.rows)
    for bad in (dict(batch=7), dict(mode="half"), dict(cutmix_minmax=(0.2,)), dict(cutmix_minmax=(0.2, 0.5, 0.7)), dict(cutmix_minmax=(0.6, 0.3)),
                dict(mixup_alpha=-1.0), dict(mixup_alpha=0.0, cutmix_alpha=0.0)):
        with pytest.raises(ValueError):
            _sampler(**bad)


def test_sampler_statistics():
    """Fixed seeds, so deterministic.  Bounds: 4 sigma at n = 2000, rounded up -- Bernoulli(0.5): 4 * sqrt(0.25 / 2000) = 0.045 -> 0.05;
    the mean of U(0, 1) = Beta(1, 1): 4 * sqrt(1 / 12 / 2000) = 0.026 -> 0.03."""
    s = _sampler(mixup_alpha=1.0, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", seed=2024)
    # (a cutmix decision whose box comes out empty is a copy row: counted by its lam == 1 together with the paste rows)
    modes = [int(s.sample_host()["mode"][0]) for _ in range(2000)]
    share = sum(m != 1 for m in modes) / 2000.0
    assert abs(share - 0.5) <= 0.05, share
    s = _sampler(mixup_alpha=1.0, cutmix_alpha=0.0, prob=1.0, mode="batch", seed=2025)
    lam = [float(s.sample_host()["lam"][0]) for _ in range(2000)]
    assert abs(sum(lam) / 2000.0 - 0.5) <= 0.03, sum(lam) / 2000.0


def test_dense_target_of_the_restatement():
    B, C = 8, 5
    g = torch.Generator().manual_seed(0)
    tgt = torch.randint(0, C, (B, 1), generator=g)
    partner = B - 1 - torch.arange(B)
    lam = torch.rand(B, generator=g)
    t = mw.mixup_target(tgt, C, lam, partner, 0.1)
    assert torch.allclose(t.sum(1), torch.ones(B), atol=1e-6)
    one = mw.mixup_target(tgt, C, torch.ones(B), partner, 0.1)
    ref = torch.full((B, C), 0.1 / C).scatter_(1, tgt, 1.0 - 0.1 + 0.1 / C)
    assert torch.equal(one, ref)
    # with lam = 1 SoftTargetCrossEntropy on that target is the label-smoothing loss of the default path
    from oracle import vit_oracle as vo
    z = torch.randn(B, C, generator=g)
    assert abs(float(mw.mix_loss(z, one, "soft_ce")) - float(vo.softmax_lsce(z, tgt, 0.1))) < 1e-6
    # BinaryCrossEntropy's threshold makes the target binary
    thr = mw.mixup_target(tgt, C, lam, partner, 0.1).gt(0.2)
    assert set(thr.unique().tolist()) <= {False, True} and float(mw.mix_loss(z, t, "bce", 0.2)) > 0


def test_new_entry_points_validate_arguments():
    """Errors come back through the ABI before any launch (no GPU touched); both library builds export the symbols."""
    import subprocess
    from gipvit import _lib
    P = 1 << 20
    for name in ("gv_patchify_mix", "gv_patchify_mix_f32"):
        a = _lib.gv_patchify_mix_args()
        fn = getattr(_lib.lib, name)
        assert fn(ctypes.byref(a), None) == -3
        a.p.tiles = a.p.patches = P
        a.p.n_img, a.p.n_tiles, a.p.n_win, a.p.tile_h, a.p.tile_w, a.p.crop, a.p.img_stride = 8, 8, 1, 64, 64, 64, 64 * 64 * 3
        for c in range(3):
            a.p.std[c] = 1.0
        assert fn(ctypes.byref(a), None) == -3 and b"mix table" in _lib.lib.gv_last_error()
        a.mix = P
        a.p.n_win, a.p.n_img = 2, 16
        assert fn(ctypes.byref(a), None) == -1 and b"one window" in _lib.lib.gv_last_error()
    for name in ("gv_patchify_nchw_mix", "gv_patchify_nchw_mix_f32"):
        a = _lib.gv_patchify_nchw_mix_args()
        fn = getattr(_lib.lib, name)
        assert fn(ctypes.byref(a), None) == -3
        a.p.images = a.p.patches = P
        a.p.n_img, a.p.n_tiles, a.p.n_win, a.p.img_h, a.p.img_w, a.p.crop = 8, 8, 1, 64, 64, 64
        a.p.stride_n, a.p.stride_c, a.p.stride_h = 3 * 64 * 64, 64 * 64, 64
        assert fn(ctypes.byref(a), None) == -3 and b"mix table" in _lib.lib.gv_last_error()
        a.mix = P
        a.p.n_win, a.p.n_img = 2, 16
        assert fn(ctypes.byref(a), None) == -1 and b"one window" in _lib.lib.gv_last_error()
    b = _lib.gv_softmax_mix_loss_args()
    assert _lib.lib.gv_softmax_mix_loss(ctypes.byref(b), None) == -3
    b.logits = b.target = b.loss = b.dlogits = P
    b.B, b.C = 8, 65
    assert _lib.lib.gv_softmax_mix_loss(ctypes.byref(b), None) == -1
    b.C, b.kind = 5, 2
    assert _lib.lib.gv_softmax_mix_loss(ctypes.byref(b), None) == -4
    b.kind, b.has_threshold = 0, 1
    assert _lib.lib.gv_softmax_mix_loss(ctypes.byref(b), None) == -4 and b"BCE only" in _lib.lib.gv_last_error()
    pkg = os.path.dirname(_lib.LIB_PATH)
    names = ["gv_patchify_mix", "gv_patchify_mix_f32", "gv_patchify_nchw_mix", "gv_patchify_nchw_mix_f32", "gv_softmax_mix_loss"]
    for lib in ("libgipvit_hip.so", "libgipvit_hip_f16.so"):
        code = f"import ctypes; l = ctypes.CDLL({os.path.join(pkg, lib)!r}); [getattr(l, n) for n in {names!r}]; assert l.gv_version() == 9"
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-500:]
    assert all(n in _lib.ENTRY_POINTS for n in names)


def test_engine_refuses_bad_loss_arguments():
    from gipvit.engine import SupervisedEngine
    with pytest.raises(ValueError, match="loss"):
        SupervisedEngine(loss="jsd", device="cpu")
    with pytest.raises(ValueError, match="bce_target_thresh"):
        SupervisedEngine(loss="soft_ce", bce_target_thresh=0.2, device="cpu")


def test_cli_flags_reach_the_sampler_and_refusals():
    sys.path.insert(0, ROOT)
    import train
    from gipvit.cli_spec import REFERENCE_FLAGS
    assert len(REFERENCE_FLAGS) == 148
    used = {e["flags"][-1]: e["used"] for e in REFERENCE_FLAGS}
    assert all(used[f] for f in NINE) and not used["--jsd-loss"] and not used["--aug-splits"]
    base = ["--model", "vit_tiny", "-b", "8"]
    a, _ = train.parse_args(base)
    train.check_supported(a, lambda m: None)
    assert not train.mix_active(a) and train.build_mix_sampler(a, 64) is None and train.loss_kind(a) == "lsce"
    a, _ = train.parse_args(base + ["--mixup", "0.8", "--cutmix", "1.0", "--mixup-prob", "0.7", "--mixup-switch-prob", "0.3", "--mixup-mode", "pair",
                                    "--mixup-off-epoch", "3", "--seed", "5"])
    train.check_supported(a, lambda m: None)
    s = train.build_mix_sampler(a, 64, rank=1)
    assert (s.mixup_alpha, s.cutmix_alpha, s.minmax, s.prob, s.switch_prob, s.mode, s.B, s.img) == (0.8, 1.0, None, 0.7, 0.3, "pair", 8, 64)
    assert train.loss_kind(a) == "soft_ce" and a.mixup_off_epoch == 3
    assert not np.array_equal(s.sample_host(), train.build_mix_sampler(a, 64, rank=0).sample_host())       # a stream per rank
    a, _ = train.parse_args(base + ["--cutmix-minmax", "0.2", "0.8", "--bce-loss", "--bce-target-thresh", "0.2"])
    train.check_supported(a, lambda m: None)
    s = train.build_mix_sampler(a, 64)
    assert s.minmax == (0.2, 0.8) and s.cutmix_alpha == 1.0 and train.loss_kind(a) == "bce" and a.bce_target_thresh == 0.2
    a, _ = train.parse_args(base + ["--bce-loss"])
    assert train.loss_kind(a) == "bce" and train.build_mix_sampler(a, 64) is None
    a, _ = train.parse_args(base + ["--bce-loss", "--smoothing", "0"])          # train.py:838-844: plain cross-entropy
    assert train.loss_kind(a) == "lsce"
    bad = [["--dino", "--opt", "adamw"] + [f] + v for f, v in (("--mixup", ["0.8"]), ("--cutmix", ["1.0"]), ("--cutmix-minmax", ["0.2", "0.8"]),
                                                             ("--mixup-prob", ["0.5"]), ("--mixup-switch-prob", ["0.2"]), ("--mixup-mode", ["elem"]),
                                                             ("--mixup-off-epoch", ["2"]), ("--bce-loss", []), ("--bce-target-thresh", ["0.2"]))]
    bad += [["--mixup", "0.8", "--mixup-mode", "half"], ["--mixup", "0.8", "-b", "7"], ["--cutmix", "1.0", "-b", "9"], ["--mixup", "-0.1"],
            ["--cutmix", "-1"], ["--cutmix-minmax", "0.2"], ["--cutmix-minmax", "0.2", "0.5", "0.8"], ["--cutmix-minmax", "0.5", "0.2"],
            ["--cutmix-minmax", "0.5", "0.5"], ["--cutmix-minmax", "0.0", "0.5"], ["--cutmix-minmax", "0.5", "1.5"]]
    for b in bad:
        a, _ = train.parse_args(base + b)
        with pytest.raises(SystemExit):
            train.check_supported(a, lambda m: None)
    a, _ = train.parse_args(base + ["-b", "7"])                                  # an odd batch is fine without mixing
    train.check_supported(a, lambda m: None)
