"""CPU: the host logic of train.py's stages -- the one table of per-rank draw-stream seeds (checkpoint.HOST_STREAMS) and the
samplers built from it, the monitor list (which is due when, which metric chooses the checkpoint and in which direction) and the
fold selection.  The literal numbers and tables below are restated here on purpose: they pin what the driver did before its
``main`` was cut into stages."""
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DINO = ["--model", "vit_tiny", "--dino", "-b", "2", "--random-crops", "--view-augment", "--stain-jitter", "0.05", "--ibot-weight", "1", "--drop-path", "0.1"]
SUPERVISED = ["--model", "vit_tiny", "-b", "2", "--mixup", "0.2", "--reprob", "0.25", "--drop", "0.1", "--drop-path", "0.1"]
# seed 42, ranks 0 / 1 / 3
SEEDS = {"crops": (42, 43, 45), "drop": (53, 7972, 23810), "views": (47, 100, 206), "stain": (83, 396, 1022), "mix": (65, 166, 368),
         "erase": (79, 290, 712), "ibot": (45, 146, 348), "drop_path": (42, 59, 93)}


def test_stream_seed_is_the_table_of_the_driver():
    from gipvit.checkpoint import HOST_STREAMS, stream_seed
    assert set(HOST_STREAMS) == set(SEEDS)
    for name, want in SEEDS.items():
        assert tuple(stream_seed(name, 42, r) for r in (0, 1, 3)) == want, name
    src = open(os.path.join(ROOT, "train.py")).read()          # and train.py states none of them a second time
    assert not re.search(r"7919|313 \*|211 \*|101 \*", src)


def _first_draw(s):
    x = s.integers(0, 1 << 32) if isinstance(s, np.random.Generator) else s.sample_host() if hasattr(s, "sample_host") else s.sample()
    flat = lambda v: (tuple(flat(u) for u in v) if isinstance(v, (tuple, list)) else v.numpy().tobytes() if torch.is_tensor(v)
                      else v.tobytes() if isinstance(v, np.ndarray) else v)
    return flat(x)


@pytest.mark.parametrize("rank", [0, 1, 3])
def test_every_sampler_is_built_on_its_literal_seed(rank):
    import train
    from gipvit.droppath import DropPathSampler
    from gipvit.erasing import EraseSampler
    from gipvit.masking import MaskSampler
    from gipvit.mixup import MixSampler
    from gipvit.multicrop import MultiCropSampler, ViewAugmentSampler
    from gipvit.stain import StainJitterSampler
    seed = {k: v[(0, 1, 3).index(rank)] for k, v in SEEDS.items()}
    a, _ = train.parse_args(DINO + ["--seed", "42"])
    train.check_supported(a, lambda m: None)
    s = train.build_samplers(a, rank, False, "cpu", 224, 12, 20)
    want = {"crops": MultiCropSampler(2, 256, 2, 8, (0.4, 1.0), (0.05, 0.4), seed=seed["crops"]), "ibot": MaskSampler(14, 4, (0.1, 0.5), 0.5, seed=seed["ibot"]),
            "views": ViewAugmentSampler(2, 2, 8, jitter_p=0.8, gray_p=0.2, blur_p=(1.0, 0.1, 0.5), solar_p=(0.0, 0.2, 0.0), seed=seed["views"]),
            "stain": StainJitterSampler(2, 2, 8, 0.05, prob=1.0, seed=seed["stain"]), "drop_path": DropPathSampler(12, 20, 0.1, seed["drop_path"], "cpu")}
    assert (s.mix, s.erase, s.drop) == (None, None, None)
    for k, w in want.items():
        assert _first_draw(getattr(s, k)) == _first_draw(w), k
    a, _ = train.parse_args(SUPERVISED + ["--seed", "42"])
    train.check_supported(a, lambda m: None)
    s = train.build_samplers(a, rank, False, "cpu", 64, 12, 2)
    want = {"mix": MixSampler(mixup_alpha=0.2, cutmix_alpha=0.0, batch=2, img_size=64, seed=seed["mix"]),
            "erase": EraseSampler(prob=0.25, batch=2, img_size=64, seed=seed["erase"]), "drop": np.random.default_rng(seed["drop"]),
            "drop_path": DropPathSampler(12, 2, 0.1, seed["drop_path"], "cpu")}
    assert (s.crops, s.ibot, s.views, s.stain) == (None, None, None, None)
    for k, w in want.items():
        assert _first_draw(getattr(s, k)) == _first_draw(w), k
    assert _first_draw(train.build_mix_sampler(a, 64, rank)) == _first_draw(MixSampler(mixup_alpha=0.2, cutmix_alpha=0.0, batch=2, img_size=64, seed=seed["mix"]))
    assert _first_draw(train.build_erase_sampler(a, 64, rank)) == _first_draw(EraseSampler(prob=0.25, batch=2, img_size=64, seed=seed["erase"]))


def test_restore_gets_a_seed_for_every_stream_that_is_packed():
    """What main hands to pack_host_rng / restore_host_rng: ``streams`` under the checkpoint's names, the run's generators in it,
    and ``seeds`` with exactly those names plus the DropPathSampler's."""
    import train
    for flags in (DINO, SUPERVISED, ["--model", "vit_tiny"]):
        a, _ = train.parse_args(flags + ["--seed", "42"])
        s = train.build_samplers(a, 3, False, "cpu", 64, 12, 2)
        assert set(s.seeds) == set(s.streams) | {"drop_path"} == set(SEEDS)
        assert s.seeds == {k: v[2] for k, v in SEEDS.items()}
        assert list(s.streams) == ["drop", "crops", "views", "stain", "mix", "erase", "ibot"]
        for k, g in s.streams.items():
            owner = s.drop if k == "drop" else getattr(getattr(s, k), "rng", None)
            assert g is owner and (g is None or isinstance(g, np.random.Generator)), k
    a, _ = train.parse_args(DINO)
    s = train.build_samplers(a, 0, False, "cpu", 224, 12, 20)
    assert sorted(k for k, g in s.streams.items() if g is not None) == ["crops", "ibot", "stain", "views"] and s.drop_path is not None


def test_monitor_due_is_the_three_rules():
    import train
    for rate in (0, 1, 3, 5):
        a, _ = train.parse_args(["--model", "vit_tiny", "--epochs", "12", "--knn-rate", str(rate), "--linprobe-rate", str(rate), "--mil-rate", str(rate)])
        for epoch in range(12):
            if rate == 0:               # (refused by check_supported; the rule itself is a plain modulo, as it was)
                with pytest.raises(ZeroDivisionError):
                    train.monitor_due(a, "knn_", epoch)
            else:
                assert train.monitor_due(a, "knn_", epoch) == ((epoch + 1) % rate == 0)
            probe = epoch == 11 or (rate >= 1 and (epoch + 1) % rate == 0)
            assert train.monitor_due(a, "linear_", epoch) == probe and train.monitor_due(a, "mil_", epoch) == probe
    a, _ = train.parse_args(["--model", "vit_tiny", "--epochs", "12", "--knn-rate", "5", "--linprobe-rate", "3", "--mil-rate", "0"])       # each its own flag
    assert [e for e in range(12) if train.monitor_due(a, "knn_", e)] == [4, 9]
    assert [e for e in range(12) if train.monitor_due(a, "linear_", e)] == [2, 5, 8, 11] and [e for e in range(12) if train.monitor_due(a, "mil_", e)] == [11]


NAMES = ("top1", "loss", "knn_top1", "linear_loss", "mil_auc_per_slide")
RESOLVED = {      # (knn, probe, mil) -> resolve_eval_metric of NAMES, as the function stood before the driver was cut into stages
    (False, False, False): ("top1", "loss", "knn_top1", "linear_loss", "mil_auc_per_slide"),
    (False, False, True): ("mil_top1", "mil_loss", "knn_top1", "linear_loss", "mil_auc_per_slide"),
    (False, True, False): ("linear_top1", "linear_loss", "knn_top1", "linear_loss", "mil_auc_per_slide"),
    (False, True, True): ("linear_top1", "linear_loss", "knn_top1", "linear_loss", "mil_auc_per_slide"),
    (True, False, False): ("knn_top1", "knn_loss", "knn_top1", "linear_loss", "mil_auc_per_slide"),
    (True, False, True): ("knn_top1", "knn_loss", "knn_top1", "linear_loss", "mil_auc_per_slide"),
    (True, True, False): ("knn_top1", "knn_loss", "knn_top1", "linear_loss", "mil_auc_per_slide"),
    (True, True, True): ("knn_top1", "knn_loss", "knn_top1", "linear_loss", "mil_auc_per_slide")}


class _Runner:
    D, img, dev = 192, 64, "cpu"

    class vit:
        depth = 12


def _monitors(train, knn, probe, mil, more=()):
    flags = ["--model", "vit_tiny", "--dino"] + ["--knn-monitor"] * knn + ["--linear-probe"] * probe + ["--mil-probe"] * mil + list(more)
    a, _ = train.parse_args(flags)
    return a, train.build_monitors(a, _Runner(), primary=False)


def test_eval_metric_and_its_direction_over_the_monitor_grid():
    import train
    assert set(RESOLVED) == set(itertools.product((False, True), repeat=3))
    for (knn, probe, mil), want in RESOLVED.items():
        a, monitors = _monitors(train, knn, probe, mil)
        assert [m.prefix for m in monitors] == [p for p, on in (("knn_", knn), ("linear_", probe), ("mil_", mil)) if on]
        assert [n for m in monitors for n in m.metric_names()] == train.monitor_metric_names(a)
        for name, resolved in zip(NAMES, want):
            assert train.resolve_eval_metric(name, knn, probe, mil) == resolved
            assert train.resolve_eval_metric(name, *(any(m.prefix == p for m in monitors) for p in ("knn_", "linear_", "mil_"))) == resolved
            assert (resolved in train.LOWER_IS_BETTER) == (resolved in ("loss", "linear_loss", "mil_loss")), (knn, probe, mil, name)
        # the saver's direction is the literal the driver always had; what the monitors of the list declare has to agree with it
        # (build_monitors asserts that too), for every metric the run reports
        lower = [m.prefix + x for m in monitors for x in m.lower_is_better]
        assert lower == [n for n in train.monitor_metric_names(a) if n in ("linear_loss", "mil_loss")]
        assert all((n in train.LOWER_IS_BETTER) == (n in lower) for n in train.monitor_metric_names(a))
        if knn and probe and mil:
            assert ("loss",) + tuple(lower) == train.LOWER_IS_BETTER


def test_monitor_list_follows_the_flags():
    import train
    a, monitors = _monitors(train, True, True, True, ["--num-classes", "1", "--knn-k", "5", "--mil-hidden", "32", "--linprobe-lrs", "0.1", "0.2"])
    assert [n for m in monitors for n in m.metric_names()] == ["knn_top1", "linear_top1", "linear_loss", "mil_top1", "mil_loss"]
    assert (monitors[0].k, monitors[1].lrs, monitors[2].L) == (5, (0.1, 0.2), 32) and all(m.normaliser is None and m.C == 1 for m in monitors)
    norm = object()
    assert all(m.normaliser is norm for m in train.build_monitors(a, _Runner(), False, norm))
    b, _ = train.parse_args(["--model", "vit_tiny", "--dino", "--knn-monitor", "--extract_features"])      # --extract_features runs alone: no runner is built
    assert train.build_monitors(b, None) == [] and _monitors(train, False, False, False)[1] == []
    assert all(callable(m.fit) and callable(m.evaluate) for m in monitors)
    from gipvit.knn import KnnMonitor
    assert KnnMonitor.fit is KnnMonitor.build_bank


# ---- select_slides on a dozen slides: folds 1 (4 slides), 2 (4), 3 (3), 4 (1)
@pytest.fixture(scope="module")
def slides(tmp_path_factory):
    from gipvit import data as D
    root = tmp_path_factory.mktemp("tiles")
    folds = [1] * 4 + [2] * 4 + [3] * 3 + [4]
    for s, _ in enumerate(folds):
        os.makedirs(root / f"slide{s:02d}")
        D.write_tile_file(str(root / f"slide{s:02d}" / "tile_0.data"), np.full((16, 16, 3), s, dtype=np.uint8))
    (root / "labels.csv").write_text("slide,label,fold\n" + "".join(f"slide{s:02d},{s % 2},{f}\n" for s, f in enumerate(folds)))
    return D.scan_slides(str(root))


def _select(train, slides, flags, primary=True):
    a, _ = train.parse_args(["--model", "vit_tiny", "--seed", "5"] + flags)
    tr, ev, want = train.select_slides(a, slides, primary)
    return [s[0] for s in tr], [s[0] for s in ev], want


def test_select_slides(slides, caplog):
    import train
    name = lambda i: f"slide{i:02d}"
    assert len(slides) == 12
    # a normal fold: train on the others, evaluate on it
    assert _select(train, slides, ["--test_fold", "2"]) == ([name(i) for i in (0, 1, 2, 3, 8, 9, 10, 11)], [name(i) for i in (4, 5, 6, 7)], True)
    # nothing evaluates: no selection is made at all (--no-validate; a --dino run without a monitor)
    for flags in (["--no-validate"], ["--dino"]):
        tr, ev, want = _select(train, slides, ["--test_fold", "2"] + flags)
        assert len(tr) == 8 and ev == [] and want is False
    # --dino --extract_features and the monitors do evaluate
    assert _select(train, slides, ["--test_fold", "2", "--dino", "--extract_features"])[1:] == ([name(i) for i in (4, 5, 6, 7)], True)
    assert _select(train, slides, ["--test_fold", "2", "--dino", "--mil-probe"])[1:] == ([name(i) for i in (4, 5, 6, 7)], False)
    # --supervised: the test fold re-split 80 / 20 by default_rng(seed)
    perm = np.random.default_rng(5).permutation(4)
    assert _select(train, slides, ["--test_fold", "2", "--supervised"]) == ([name(4 + i) for i in perm[:3]], [name(4 + perm[3])], True)
    perm = np.random.default_rng(5).permutation(3)
    assert _select(train, slides, ["--test_fold", "3", "--supervised"])[:2] == ([name(8 + i) for i in perm[:2]], [name(8 + perm[2])])
    assert _select(train, slides, ["--test_fold", "4", "--supervised", "--no-validate"]) == ([name(11)], [name(11)], False)      # the 20 % side is empty: "or eval_slides"
    # --test_fold -1: every fold trains, validate() is skipped and the primary says so once
    with caplog.at_level("INFO", logger="train"):
        assert _select(train, slides, ["--test_fold", "-1"]) == ([name(i) for i in range(12)], [], False)
        assert _select(train, slides, ["--test_fold", "-1"], primary=False)[2] is False
        assert _select(train, slides, ["--test_fold", "-1", "--no-validate"])[2] is False
    assert len([m for m in caplog.messages if m.startswith("--test_fold -1: no validation fold")]) == 1
    with pytest.raises(ValueError, match="no evaluation slides"):      # ... but a monitor needs an evaluation fold
        _select(train, slides, ["--test_fold", "-1", "--dino", "--knn-monitor"])
    with pytest.raises(ValueError, match="no evaluation slides"):      # a fold without a slide
        _select(train, slides, ["--test_fold", "7"])
