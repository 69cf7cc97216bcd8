"""CPU: the host side of the H&E stain jitter (gipvit.stain, --stain-jitter): the fp64 restatement of the transform, the folded
record, the sampler, the driver's refusals, where the call sits in the engine's launch sequence (tests/launch_trace.py) and the
sampler's stream across a resume."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import launch_trace as LT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


def _colours():
    g = np.arange(256, dtype=np.uint8)
    return np.concatenate([np.stack([g, g, g], 1), np.random.default_rng(0).integers(0, 256, (4096, 3), dtype=np.uint8)])


# ---- stain_reference / stain_record
def test_matrix_is_ruifrok_johnston_unit_rows():
    from gipvit.stain import STAIN_MATRIX as M
    assert M.shape == (3, 3) and M.dtype == np.float64 and np.allclose(np.linalg.norm(M, axis=1), 1.0, atol=1e-15)
    assert np.allclose(M[0] / M[0, 0], np.array([0.65, 0.70, 0.29]) / 0.65, atol=1e-15)
    assert np.allclose(M[1] / M[1, 1], np.array([0.07, 0.99, 0.11]) / 0.99, atol=1e-15)
    assert np.allclose(M[2] / M[2, 2], np.array([0.27, 0.57, 0.78]) / 0.78, atol=1e-15)
    assert 3.7 < np.linalg.cond(M) < 3.9


def test_reference_identity_on_every_byte():
    from gipvit.stain import stain_record, stain_reference
    px = _colours()
    for A, b in ((I3, Z3), (stain_record([1, 1, 1], [0, 0, 0])["A"], stain_record([1, 1, 1], [0, 0, 0])["b"])):
        x, v = stain_reference(px, A, b)
        assert np.array_equal(v, px)
        assert float(np.abs(x - px).max()) < 1e-3          # the folded identity: M^-1 M in f32, far from any tie


def test_reference_moves_a_single_stain_along_its_vector():
    """alpha = (a, 1, 1), beta = 0: a pixel of pure haematoxylin, od = t M[0], keeps its direction and scales by a; the other two
    stains' pixels do not move."""
    from gipvit.stain import STAIN_MATRIX as M, stain_affine, stain_od
    for a in (0.5, 0.8, 1.3):
        A, b = stain_affine([a, 1.0, 1.0], [0.0, 0.0, 0.0])
        assert np.array_equal(b, np.zeros(3))
        for t in (0.1, 1.0, 2.5):
            assert float(np.abs(stain_od(t * M[0], A, b) - a * t * M[0]).max()) < 1e-12
            assert float(np.abs(stain_od(t * M[1], A, b) - t * M[1]).max()) < 1e-12
            assert float(np.abs(stain_od(t * M[2], A, b) - t * M[2]).max()) < 1e-12


def test_record_then_reference_is_the_unfolded_formula():
    """stain_record + stain_reference against section 1's formula step by step in fp64 (M^-1 applied, then alpha / beta, then M): apart
    only by the rounding of A and b to f32, |dv'| < 1e-3 on every pixel whose result is in range."""
    from gipvit.stain import STAIN_MATRIX as M, stain_record, stain_reference
    px = _colours()
    rng = np.random.default_rng(3)
    seen = 0
    for sigma in (0.05, 0.2, 0.5):
        for _ in range(4):
            alpha, beta = rng.uniform(1 - sigma, 1 + sigma, 3), rng.uniform(-sigma, sigma, 3)
            r = stain_record(alpha, beta)
            assert r.shape == () and int(r["on"]) == 1 and r["A"].dtype == np.float32 and r["b"].dtype == np.float32
            x, v = stain_reference(px, r["A"], r["b"])
            od = -np.log((px.astype(np.float64) + 1.0) / 256.0)
            s = od @ np.linalg.inv(M)
            want = 256.0 * np.exp(-((alpha * s + beta) @ M)) - 1.0
            ok = (want > -0.5) & (want < 255.5)
            seen += int(ok.sum())
            assert float(np.abs(x - want)[ok].max()) < 1e-3
            assert np.array_equal(v, np.clip(np.rint(x), 0, 255).astype(np.uint8))
    assert seen > 100000


def test_record_batches_and_custom_matrix():
    from gipvit.stain import stain_record, stain_affine
    al, be = np.array([[1.1, 0.9, 1.0], [0.7, 1.2, 1.05]]), np.array([[0.01, -0.02, 0.0], [0.1, 0.0, -0.1]])
    r = stain_record(al, be)
    assert r.shape == (2,)
    for i in range(2):
        assert np.array_equal(r[i]["A"], stain_record(al[i], be[i])["A"]) and np.array_equal(r[i]["b"], stain_record(al[i], be[i])["b"])
    A, b = stain_affine(al[0], be[0], matrix=np.eye(3))            # with M = I the stains are the channels
    assert np.allclose(A, np.diag(al[0]), atol=1e-15) and np.allclose(b, be[0], atol=1e-15)


# ---- the sampler
def test_sampler_is_seeded_and_packs_gv_stain_params():
    from gipvit import _lib
    from gipvit.stain import DT, StainJitterSampler
    assert DT.itemsize == ctypes.sizeof(_lib.gv_stain_params) == 52 and StainJitterSampler.DT is DT
    assert [DT.fields[k][1] for k in ("on", "A", "b")] == [getattr(_lib.gv_stain_params, k).offset for k in ("on", "A", "b")] == [0, 4, 40]
    assert _lib.ENTRY_POINTS["gv_crop_augment_stain"] is _lib.gv_crop_augment_stain_args
    assert _lib.gv_crop_augment_stain_args.stain.offset == ctypes.sizeof(_lib.gv_crop_augment_args)
    a, b, c = (StainJitterSampler(3, 2, 4, 0.2, prob=0.6, seed=s) for s in (5, 5, 6))
    for _ in range(3):
        ra, rb, rc = a.sample_host(), b.sample_host(), c.sample_host()
        assert [len(x) for x in ra] == [6, 12]                     # global crops first
        assert all(np.array_equal(x, y) for x, y in zip(ra, rb)) and not all(np.array_equal(x, y) for x, y in zip(ra, rc))
    pg, pl = a.sample()
    hg, hl = b.sample_host()
    assert pg.dtype == torch.uint8 and pg.numel() == 6 * 52 and pl.numel() == 12 * 52
    assert np.array_equal(pg.numpy().view(DT), hg) and np.array_equal(pl.numpy().view(DT), hl)
    d = StainJitterSampler.to_dicts(hg)
    assert len(d) == 6 and d[0]["on"] == bool(hg[0]["on"]) and np.array_equal(d[0]["A"], hg[0]["A"]) and np.array_equal(d[0]["b"], hg[0]["b"])
    for bad in (dict(sigma=-0.1), dict(sigma=1.0), dict(sigma=float("nan")), dict(sigma=0.1, prob=0.0), dict(sigma=0.1, prob=1.5)):
        with pytest.raises(ValueError):
            StainJitterSampler(2, **bad)


@pytest.mark.parametrize("sigma,prob", [(0.05, 1.0), (0.2, 0.7), (0.5, 0.25)])
def test_sampler_statistics(sigma, prob):
    """4 000 crops: alpha in (1 - s, 1 + s) with mean 1, beta in (-s, s) with mean 0 (each within 5 standard errors of a uniform's
    mean, s / sqrt(3 n)), the share of jittered crops within 3 binomial sigma of prob; records of the draws; on = 0 records are I, 0."""
    from gipvit.stain import StainJitterSampler, stain_record
    twin = StainJitterSampler(2000, 1, 1, sigma, prob=prob, seed=9)
    sp = StainJitterSampler(2000, 1, 1, sigma, prob=prob, seed=9)
    draws, recs = twin.sample_draws(), sp.sample_host()
    on = np.concatenate([d[0] for d in draws]); alpha = np.concatenate([d[1] for d in draws]); beta = np.concatenate([d[2] for d in draws])
    rec = np.concatenate(recs)
    n = len(on)
    assert n == 4000 and alpha.shape == beta.shape == (n, 3)
    assert alpha.min() >= 1 - sigma and alpha.max() <= 1 + sigma and beta.min() >= -sigma and beta.max() <= sigma
    se = sigma / math.sqrt(3 * n)
    assert np.all(np.abs(alpha.mean(0) - 1.0) < 5 * se) and np.all(np.abs(beta.mean(0)) < 5 * se)
    assert alpha.std() > 0.5 * sigma and beta.std() > 0.5 * sigma
    assert abs(on.mean() - prob) <= 3 * math.sqrt(prob * (1 - prob) / n) + 1e-12
    assert np.array_equal(rec["on"] != 0, on)
    off = rec[rec["on"] == 0]
    assert (len(off) > 0) == (prob < 1) and np.all(off["A"] == I3) and np.all(off["b"] == 0)
    k = np.flatnonzero(on)[:50]
    want = stain_record(alpha[k], beta[k])
    assert np.array_equal(rec[k]["A"], want["A"]) and np.array_equal(rec[k]["b"], want["b"])


# ---- the driver's flags
def _args(*extra):
    sys.path.insert(0, ROOT)
    import train
    args, _ = train.parse_args(["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--no-validate"] + list(extra))
    train.check_supported(args, log=lambda *a, **k: None)
    return args


def test_flags_defaults_and_accepted_case():
    a = _args()
    assert a.stain_jitter == 0.0 and a.stain_prob == 1.0
    a = _args("--random-crops", "--view-augment", "--stain-jitter", "0.05")
    assert a.stain_jitter == 0.05 and a.stain_prob == 1.0
    a = _args("--random-crops", "--view-augment", "--stain-jitter", "0.2", "--stain-prob", "0.5")
    assert a.stain_jitter == 0.2 and a.stain_prob == 0.5
    from gipvit.cli_spec import REFERENCE_FLAGS
    assert not any("stain" in f for e in REFERENCE_FLAGS for f in e["flags"])


@pytest.mark.parametrize("extra,flag", [
    (["--stain-jitter", "0.05"], "--stain-jitter"),                                                  # no --random-crops --view-augment
    (["--random-crops", "--stain-jitter", "0.05"], "--stain-jitter"),                                # no --view-augment
    (["--random-crops", "--view-augment", "--stain-jitter", "-0.1"], "--stain-jitter"),
    (["--random-crops", "--view-augment", "--stain-jitter", "1.0"], "--stain-jitter"),
    (["--random-crops", "--view-augment", "--stain-jitter", "nan"], "--stain-jitter"),
    (["--random-crops", "--view-augment", "--stain-jitter", "inf"], "--stain-jitter"),
    (["--random-crops", "--view-augment", "--stain-jitter", "0.05", "--stain-prob", "0"], "--stain-prob"),
    (["--random-crops", "--view-augment", "--stain-jitter", "0.05", "--stain-prob", "1.01"], "--stain-prob"),
    (["--random-crops", "--view-augment", "--stain-jitter", "0.05", "--stain-prob", "nan"], "--stain-prob"),
])
def test_flags_refused(extra, flag):
    with pytest.raises(SystemExit) as e:
        _args(*extra)
    assert flag in str(e.value)


def test_supervised_run_refuses_the_flag():
    sys.path.insert(0, ROOT)
    import train
    args, _ = train.parse_args(["--model", "vit_tiny_patch16_224", "--dataset", "synthetic", "--stain-jitter", "0.05"])
    with pytest.raises(SystemExit) as e:
        train.check_supported(args, log=lambda *a, **k: None)
    assert "--stain-jitter" in str(e.value)


# ---- the engine's launch sequence
def _traced(stains=False, views=True, boxes=True, tiles=None):
    from gipvit.engine import DinoEngine
    from gipvit.multicrop import MultiCropSampler, ViewAugmentSampler
    from gipvit.stain import StainJitterSampler
    with LT.recording() as rec:
        eng = DinoEngine(arch="vit_tiny", img_size=224, out_dim=256, batch=2, n_local=2, device="cpu")
        kw = {}
        if boxes:
            kw["boxes"] = MultiCropSampler(2, 256, 2, 2, seed=1).sample()
        if views:
            kw["views"] = ViewAugmentSampler(2, 2, 2, seed=2).sample()
        if stains:
            kw["stains"] = StainJitterSampler(2, 2, 2, 0.2, seed=3).sample()
        eng.step(torch.zeros(2, 256, 256, 3, dtype=torch.uint8) if tiles is None else tiles, **kw)
    return rec.events


def _renumbered(events):
    """The trace with its storages numbered again by first appearance (the recorder numbers them as it meets them, so two more
    tensors early in a step shift every later number)."""
    seen = {}

    def walk(v):
        if isinstance(v, dict) and "tensor" in v:
            t = v["tensor"]
            return {"tensor": [seen.setdefault(t[0], len(seen))] + t[1:]}
        if isinstance(v, dict):
            return {k: walk(x) for k, x in v.items()}
        return [walk(x) for x in v] if isinstance(v, list) else v
    return [walk(e) for e in events]


def test_trace_differs_in_the_two_crop_calls_only():
    off, on = _traced(False), _traced(True)
    assert len(off) == len(on) and [e[0] for e in off].count("crop_augment") == 2
    calls = [i for i, e in enumerate(on) if e[0] == "crop_augment_stain"]
    assert calls == [i for i, e in enumerate(off) if e[0] == "crop_augment"] and not any(e[0] == "crop_augment" for e in on)
    # (tiles, boxes, params, stains, stats, out_size): the packed records of the 4 crops of each size go in between ...
    for i, size in zip(calls, (224, 96)):
        st = on[i][1][3]["tensor"]
        assert st[2] == [4 * 52] and st[4] == "torch.uint8" and on[i][1][5] == size
    # ... and taken out again, with the name put back, the step is the step without them, event for event
    same = [[("crop_augment" if i in calls else e[0])] + ([e[1][:3] + e[1][4:]] if i in calls else [e[1]]) + e[2:] if len(e) > 2 else e
            for i, e in enumerate(on)]
    assert _renumbered(same) == _renumbered(off)


def test_no_stains_is_todays_trace():
    """stains=None: the step's calls are the ones it made before the keyword existed -- the recorded dino_t / dino_s fixtures, hash
    and all -- and no call of the new entry appears anywhere in a step without the records."""
    fix = LT.load_fixture()
    for cfg in ("dino_t", "dino_s", "dino_s_g"):
        got = LT.summary(LT.trace(cfg)[0])
        assert got["names"] == fix[cfg]["names"] and got["sha256"] == fix[cfg]["sha256"], cfg
    assert "crop_augment_stain" in LT.launching_ops(__import__("gipvit.ops", fromlist=["ops"]))
    assert not any(e[0] == "crop_augment_stain" for e in _traced(False))
    names = [e[0] for e in _traced(False, views=False)]
    assert "crop_resize" in names and "crop_augment" not in names


def test_stains_need_views_and_uint8_tiles():
    with pytest.raises(ValueError) as e:
        _traced(True, views=False)
    assert "stains" in str(e.value) and "views" in str(e.value)
    with pytest.raises(ValueError) as e:
        _traced(True, views=False, boxes=False)
    assert "stains" in str(e.value)
    from gipvit.engine import input_form
    with pytest.raises(ValueError) as e:
        input_form(torch.zeros(2, 3, 256, 256), 2, (256, 256), (("fill", None), ("boxes", None), ("views", None), ("stains", object())))
    assert "stains=" in str(e.value)
    with pytest.raises(ValueError) as e:                              # float input: refused by name before anything is queued
        _traced(True, views=False, boxes=False, tiles=torch.zeros(2, 3, 256, 256))
    assert "stains=" in str(e.value)


# ---- the sampler's stream across a resume
def _streams(sp, crops):
    return {"drop": None, "crops": crops.rng, "views": None, "stain": None if sp is None else sp.rng, "mix": None, "erase": None, "ibot": None}


def test_stain_stream_rides_in_the_checkpoint(tmp_path):
    from gipvit.checkpoint import load_checkpoint_file, pack_host_rng, restore_host_rng, stream_seed
    from gipvit.multicrop import MultiCropSampler
    from gipvit.stain import StainJitterSampler
    mk = lambda seed=stream_seed("stain", 42, 0): (StainJitterSampler(2, 2, 3, 0.2, prob=0.7, seed=seed),
                                                   MultiCropSampler(2, 256, 2, 3, seed=stream_seed("crops", 42, 0)))
    sp, crops = mk()
    for _ in range(3):
        sp.sample_host(); crops.sample()
    ex = pack_host_rng(_streams(sp, crops), None, lambda o: [o])
    assert set(ex["host_rng"]) == {"crops", "stain"} and set(ex["host_rng_ranks"]["states"][0]) == {"crops", "stain"}
    torch.save(ex, tmp_path / "ck.pth")
    ck = load_checkpoint_file(str(tmp_path / "ck.pth"))                   # plain containers: weights_only loads them
    cont = [sp.sample_host() for _ in range(2)]
    sp2, crops2 = mk()
    assert restore_host_rng(ck, _streams(sp2, crops2), None, 0, 1, 1) == "ranks"
    for want in cont:
        got = sp2.sample_host()
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # the flat single-process form
    sp3, crops3 = mk()
    assert restore_host_rng({"host_rng": ck["host_rng"]}, _streams(sp3, crops3), None, 0, 1, 1) == "flat"
    assert all(np.array_equal(g, w) for g, w in zip(sp3.sample_host(), cont[0]))
    # a run without the flag: no such key, and a run with it resumes from such a file with its stream as seeded
    ex_off = pack_host_rng(_streams(None, crops), None, lambda o: [o])
    assert "stain" not in ex_off["host_rng"] and "stain" not in ex_off["host_rng_ranks"]["states"][0]
    sp4, crops4 = mk()
    fresh = mk()[0].sample_host()
    assert restore_host_rng(ex_off, _streams(sp4, crops4), None, 0, 1, 1) == "ranks"
    assert all(np.array_equal(g, w) for g, w in zip(sp4.sample_host(), fresh))


def test_stain_stream_is_reseeded_per_rank_when_the_world_changes():
    from gipvit.checkpoint import pack_host_rng, restore_host_rng, stream_seed
    from gipvit.multicrop import MultiCropSampler
    from gipvit.stain import StainJitterSampler
    sp, crops = StainJitterSampler(2, 2, 3, 0.2, seed=stream_seed("stain", 42, 0)), MultiCropSampler(2, 256, 2, 3, seed=stream_seed("crops", 42, 0))
    ex = pack_host_rng(_streams(sp, crops), None, lambda o: [o])          # saved by one rank, resumed by two
    got = []
    for rank in (0, 1):
        s, c = StainJitterSampler(2, 2, 3, 0.2, seed=0), MultiCropSampler(2, 256, 2, 3, seed=0)
        seeds = {k: stream_seed(k, 42, rank) for k in ("crops", "stain")}
        assert restore_host_rng(ex, _streams(s, c), None, rank, 2, 4, seeds=seeds) == "reseeded"
        want = np.random.default_rng([4, seeds["stain"]]).bit_generator.state
        assert s.rng.bit_generator.state == want
        got.append(s.sample_host())
    assert not np.array_equal(got[0][0]["A"], got[1][0]["A"])
    with pytest.raises(KeyError):                                         # a stream without a per-rank seed is an error, not a shared draw
        restore_host_rng(ex, _streams(sp, crops), None, 0, 2, 4, seeds={"crops": 1})
