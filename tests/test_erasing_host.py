"""CPU: the host side of random erasing (--reprob / --remode / --recount) -- the erase table's layout against the header, the new
C-ABI entry points' exports and argument validation, gipvit.erasing's draws (timm RandomErasing restated), the numpy restatement
of the kernels' noise generator, the torch restatement of the whole operation, what the engine hands to gipvit.ops, and the
driver's flag handling."""
import ctypes
import inspect
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_trace as lt      # noqa: E402
import mixup_worker as mw      # noqa: E402

NAMES = ("gv_patchify_erase", "gv_patchify_erase_f32", "gv_patchify_nchw_erase", "gv_patchify_nchw_erase_f32")
FLAGS = ("--reprob", "--remode", "--recount")


def _sampler(**kw):
    from gipvit.erasing import EraseSampler
    d = dict(prob=0.5, mode="pixel", count=3, batch=8, img_size=64, seed=3)
    d.update(kw)
    return EraseSampler(**d)


# ------------------------------------------------------------------ the ABI
def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of gv_erase_row and the two argument structs as the C compiler sees them == ctypes' and numpy's view."""
    from gipvit import _lib
    from gipvit.erasing import MAX_BOXES, ROW_DT
    fields = {"gv_erase_row": ("mode", "n_box", "box", "value"), "gv_patchify_erase_args": ("p", "mix", "erase", "seed"),
              "gv_patchify_nchw_erase_args": ("p", "mix", "erase", "seed")}
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));' + "".join(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs)
                   for s, fs in fields.items())
    src = f'#include <stdio.h>\n#include <stddef.h>\n#include "gipvit.h"\nint main(){{{body}printf("max %d\\n", GV_ERASE_MAX_BOXES);return 0;}}'
    exe = str(tmp_path / "erase_layout")
    r = subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    seen = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(seen.pop("max")) == MAX_BOXES == _lib.GV_ERASE_MAX_BOXES == 8
    for s, fs in fields.items():
        st = getattr(_lib, s)
        assert [n for n, _ in st._fields_] == list(fs)
        assert int(seen[s]) == ctypes.sizeof(st), s
        for f in fs:
            assert int(seen[f"{s}.{f}"]) == getattr(st, f).offset, (s, f)
    assert ROW_DT.itemsize == ctypes.sizeof(_lib.gv_erase_row) == 232
    assert [ROW_DT.fields[n][1] for n in ROW_DT.names] == [getattr(_lib.gv_erase_row, n).offset for n in ROW_DT.names]
    assert ROW_DT["box"].shape == (8, 4) and ROW_DT["value"].shape == (8, 3)
    assert all(_lib.ENTRY_POINTS[n] is (_lib.gv_patchify_nchw_erase_args if "nchw" in n else _lib.gv_patchify_erase_args) for n in NAMES)


def test_both_builds_export_the_entries_at_abi_9():
    from gipvit import _lib
    pkg = os.path.dirname(_lib.LIB_PATH)
    for lib in ("libgipvit_hip.so", "libgipvit_hip_f16.so"):
        code = f"import ctypes; l = ctypes.CDLL({os.path.join(pkg, lib)!r}); [getattr(l, n) for n in {NAMES!r}]; assert l.gv_version() == 9"
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-500:]


def test_entry_points_validate_arguments():
    """Errors come back through the ABI before any launch (no GPU touched)."""
    from gipvit import _lib
    P = 1 << 20
    err = _lib.lib.gv_last_error
    for name in NAMES:
        nchw = "nchw" in name
        a = _lib.ENTRY_POINTS[name]()
        fn = getattr(_lib.lib, name)
        assert fn(None, None) == -3
        assert fn(ctypes.byref(a), None) == -3
        a.p.patches = P
        a.p.n_img, a.p.n_tiles, a.p.n_win, a.p.crop = 8, 8, 1, 64
        if nchw:
            a.p.images, a.p.img_h, a.p.img_w = P, 64, 64
            a.p.stride_n, a.p.stride_c, a.p.stride_h = 3 * 64 * 64, 64 * 64, 64
        else:
            a.p.tiles, a.p.tile_h, a.p.tile_w, a.p.img_stride = P, 64, 64, 64 * 64 * 3
            for c in range(3):
                a.p.std[c] = 1.0
        assert fn(ctypes.byref(a), None) == -3 and b"null erase table" in err(), err()        # mix may be NULL, erase may not
        a.erase = P + 2
        assert fn(ctypes.byref(a), None) == -2 and b"erase table must be 4-byte aligned" in err(), err()
        a.erase, a.mix = P, P + 1
        assert fn(ctypes.byref(a), None) == -2 and b"mix table must be 4-byte aligned" in err(), err()
        a.mix = None
        a.p.n_win, a.p.n_img = 2, 16
        assert fn(ctypes.byref(a), None) == -1 and b"one window" in err(), err()
        # the noise generator's 32-bit pixel index: n_img * 3 * crop^2 < 2^32 (21846 * 3 * 256^2 = 2^32 + 2 * 2^16)
        a.p.n_win, a.p.n_img, a.p.n_tiles, a.p.crop = 1, 21846, 21846, 256
        if nchw:
            a.p.img_h = a.p.img_w = 256
        else:
            a.p.tile_h = a.p.tile_w = 256
        assert fn(ctypes.byref(a), None) == -1 and b"2^32" in err(), err()


# ------------------------------------------------------------------ the sampler
def test_sampler_boxes_and_counts():
    """4 000 images at S = 64, prob 0.5, count 3.  The share of erased images: 4 binomial standard deviations at n = 4000, p = 0.5
    are 4 * sqrt(0.25 / 4000) = 0.0316 (an erased image always gets a box here: h, w < 64 needs one of ten attempts at an area
    <= 1/3 * 64^2 / count, which never fails)."""
    from gipvit.erasing import ERASE_NOISE, ERASE_VALUE
    S, n = 64, 4000
    s = _sampler(batch=n, img_size=S)
    rows, seed = s.sample_host()
    assert 0 <= seed < 1 << 32 and rows.shape == (n,)
    assert int(rows["n_box"].max()) == 3 and int(rows["n_box"].min()) == 0 and set(rows["n_box"].tolist()) == {0, 1, 2, 3}
    for r in rows:
        for b in range(int(r["n_box"])):
            yl, yh, xl, xh = (int(v) for v in r["box"][b])
            assert 0 <= yl < yh <= S and 0 <= xl < xh <= S and 0 < yh - yl < S and 0 < xh - xl < S
        assert not r["box"][int(r["n_box"]):].any() and not r["value"][int(r["n_box"]):].any()
    share = float((rows["n_box"] > 0).mean())
    print(f"[erase sampler] share of erased images {share:.4f}")
    assert abs(share - 0.5) <= 4.0 * math.sqrt(0.25 / n), share
    assert set(rows["mode"][rows["n_box"] > 0].tolist()) == {ERASE_NOISE} and set(rows["mode"][rows["n_box"] == 0].tolist()) == {0}
    # box area: U(0.02, 1/3) * S^2 / count before the two roundings -- never above a third of the window (+ rounding)
    areas = np.array([(r["box"][b][1] - r["box"][b][0]) * (r["box"][b][3] - r["box"][b][2]) for r in rows for b in range(int(r["n_box"]))])
    assert areas.max() <= S * S / 3.0 * 1.1 and areas.min() >= 1
    rc, _ = _sampler(mode="const", batch=400).sample_host()
    assert set(rc["mode"].tolist()) == {0, ERASE_VALUE} and not rc["value"].any()
    rr, _ = _sampler(mode="rand", batch=400).sample_host()
    vals = np.concatenate([r["value"][:int(r["n_box"])].reshape(-1) for r in rr])
    assert set(rr["mode"].tolist()) == {0, ERASE_VALUE} and len(np.unique(vals)) == len(vals) and abs(float(vals.mean())) < 0.2 and 0.8 < float(vals.std()) < 1.2
    one, _ = _sampler(count=1, prob=1.0, batch=200).sample_host()
    assert set(one["n_box"].tolist()) == {1}
    assert not _sampler(prob=0.0, batch=200).sample_host()[0]["n_box"].any()
    for bad in (dict(prob=-0.1), dict(prob=1.5), dict(mode="noise"), dict(count=0), dict(count=9)):
        with pytest.raises(ValueError):
            _sampler(**bad)


def test_sampler_streams_and_state():
    from gipvit.erasing import ROW_DT, ErasePlan
    a, b = _sampler(), _sampler()
    for _ in range(5):
        (ra, sa), (rb, sb) = a.sample_host(), b.sample_host()
        assert np.array_equal(ra, rb) and sa == sb
    (r4, s4), (r5, s5) = _sampler(seed=4).sample_host(), _sampler(seed=5).sample_host()
    assert not np.array_equal(r4, r5) and s4 != s5
    sd = json.loads(json.dumps(a.state_dict()))             # plain types: the checkpoint loads with weights_only=True
    assert isinstance(sd["rng"], str)
    nxt = [a.sample_host() for _ in range(3)]
    c = _sampler(seed=99)
    c.load_state_dict(sd)
    for rows, seed in nxt:
        rc, sc = c.sample_host()
        assert np.array_equal(rc, rows) and sc == seed
    p = _sampler(mode="rand").sample()                      # the device form
    assert isinstance(p, ErasePlan) and p.table.dtype == torch.uint8 and p.table.numel() == 8 * 232 and 0 <= p.seed < 1 << 32
    assert np.array_equal(p.table.numpy().view(ROW_DT), p.rows)


# ------------------------------------------------------------------ the noise generator, restated
def _corr(a, b):
    a, b = a.reshape(-1) - a.mean(), b.reshape(-1) - b.mean()
    return float((a * b).mean() / math.sqrt(float((a * a).mean()) * float((b * b).mean())))


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_noise_reference_statistics(seed):
    from gipvit.erasing import noise_reference
    z = noise_reference(seed, 8, 96)
    assert z.shape == (8, 3, 96, 96) and z.dtype == np.float64 and np.isfinite(z).all()
    assert float(np.abs(z).max()) <= 5.77                   # u1 >= 2^-24
    c = {"x": _corr(z[..., :-1], z[..., 1:]), "y": _corr(z[:, :, :-1], z[:, :, 1:]), "channel": _corr(z[:, :-1], z[:, 1:]), "image": _corr(z[:-1], z[1:])}
    print(f"[noise seed {seed}] mean {z.mean():+.5f} var {z.var():.5f} m4 {np.mean(z ** 4):.4f} corr {c}")
    assert abs(float(z.mean())) < 0.01 and abs(float(z.var()) - 1.0) < 0.01
    assert all(abs(v) < 0.01 for v in c.values()), c


def test_noise_reference_is_the_stated_formula():
    """Three pixels by hand (python ints and math), and the value is keyed by the pixel alone: a larger batch extends the smaller."""
    from gipvit.erasing import noise_reference
    def fmix(h):
        h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    seed, S = 0xFFFFFFFF, 16
    z = noise_reference(seed, 2, S)
    for img, c, y, x in ((0, 0, 0, 0), (1, 2, 15, 15), (1, 0, 3, 7)):
        idx = ((img * 3 + c) * S + y) * S + x
        h1 = fmix((seed + 0x9E3779B9 * (idx + 1)) & 0xFFFFFFFF)
        h2 = fmix((h1 + 0x6D2B79F5) & 0xFFFFFFFF)
        u1, u2 = ((h1 >> 8) + 1) * 2.0 ** -24, (h2 >> 8) * 2.0 ** -24
        ref = math.sqrt(-2.0 * math.log(u1)) * math.cos(float(np.float32(6.2831853)) * u2)
        assert abs(z[img, c, y, x] - ref) < 1e-12
    assert np.array_equal(noise_reference(seed, 1, S), z[:1]) and not np.array_equal(noise_reference(1, 2, S), z)
    with pytest.raises(ValueError):
        noise_reference(0, 21846, 256)


# ------------------------------------------------------------------ the whole operation, restated
def test_apply_reference():
    from gipvit.erasing import ERASE_NOISE, ErasePlan, apply_reference, noise_reference
    from gipvit.mixup import MixPlan
    B, S = 4, 32
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(0))
    rows = ErasePlan.make_rows(B)
    ErasePlan.add_box(rows, 0, (2, 20, 3, 17), (1.0, 2.0, 3.0))
    ErasePlan.add_box(rows, 0, (10, 30, 9, 12), (-1.0, -2.0, -3.0))      # overlaps the first: the later box wins
    ErasePlan.add_box(rows, 1, (5, 9, 5, 9), (7.0, 7.0, 7.0))
    rows["mode"][1] = 0                                                 # switched off
    ErasePlan.add_box(rows, 3, (-5, 7, 28, 99), mode=ERASE_NOISE)        # clamped to the window
    y = ErasePlan(rows, seed=5)
    out = apply_reference(x, y)
    assert torch.equal(out[1], x[1]) and torch.equal(out[2], x[2])      # mode 0, n_box 0: the input
    exp = x[0].clone()
    exp[:, 2:20, 3:17] = torch.tensor([1.0, 2.0, 3.0]).view(3, 1, 1)
    exp[:, 10:30, 9:12] = torch.tensor([-1.0, -2.0, -3.0]).view(3, 1, 1)
    assert torch.equal(out[0], exp) and float(out[0, 1, 12, 10]) == -2.0 and float(out[0, 1, 12, 13]) == 2.0
    z = torch.from_numpy(noise_reference(5, B, S).astype(np.float32))
    exp = x[3].clone()
    exp[:, 0:7, 28:32] = z[3, :, 0:7, 28:32]
    assert torch.equal(out[3], exp)
    for bad_mode, bad_n in ((7, 1), (1, 9), (1, -1)):
        r2 = rows.copy()
        r2["mode"][0], r2["n_box"][0] = bad_mode, bad_n
        assert torch.equal(apply_reference(x, ErasePlan(r2))[0], x[0])
    # erasing comes after mixing: the erased pixels of a mixed batch do not depend on either source
    mrows = MixPlan.make_rows(B)
    MixPlan.set_row(mrows, 0, 0.4, None); MixPlan.set_row(mrows, 3, 0.4, None)
    mixed = mw.mix_images(x, mrows)
    out = apply_reference(mixed, y)
    assert float(out[0, 0, 3, 4]) == 1.0 and torch.equal(out[0, :, 0, :], mixed[0, :, 0, :]) and not torch.equal(mixed[0], x[0])
    with pytest.raises(ValueError):
        for _ in range(9):
            ErasePlan.add_box(rows, 2, (0, 1, 0, 1))


# ------------------------------------------------------------------ the engine's launches
def test_engine_passes_erase_only_with_a_plan():
    """Recorded on the CPU (tests/launch_trace.py): with a plan the patchify call carries erase=(table, seed) next to mix / fill,
    without one the call has exactly the keywords it had; forward(), FeatureExtractor and DinoEngine have no such argument."""
    from gipvit.engine import DinoEngine, FeatureExtractor, SupervisedEngine
    from gipvit.erasing import ErasePlan
    from gipvit.mixup import MixPlan
    rows = ErasePlan.make_rows(2)
    ErasePlan.add_box(rows, 1, (1, 9, 2, 30), (0.5, 0.5, 0.5))
    plan = ErasePlan(rows, seed=77)
    tgt = torch.zeros(2, 1, dtype=torch.int64)
    with lt.recording() as rec:
        eng = SupervisedEngine(arch="vit_tiny", img_size=64, num_classes=2, batch=2, device="cpu", loss="soft_ce")
        eng.step(torch.zeros(2, 64, 64, 3, dtype=torch.uint8), tgt, fill=torch.zeros(2, 8), erase=plan)
        eng.step(torch.zeros(2, 3, 64, 64), tgt, mix=MixPlan(MixPlan.make_rows(2)), erase=plan)
        eng.step(torch.zeros(2, 3, 64, 64), tgt)
        eng.forward(torch.zeros(2, 3, 64, 64))
    calls = [e for e in rec.events if e[0] in ("patchify", "patchify_nchw")]
    assert [c[0] for c in calls] == ["patchify", "patchify_nchw", "patchify_nchw", "patchify_nchw"]
    assert calls[0][2]["erase"][1] == 77 and calls[0][2]["erase"][0]["tensor"][2] == [2 * 232] and calls[0][2]["fill"] is not None and calls[0][2]["mix"] is None
    assert calls[1][2]["erase"][1] == 77 and calls[1][2]["mix"] is not None
    assert sorted(calls[2][2]) == sorted(calls[3][2]) == ["mix", "out"]
    for fn in (SupervisedEngine.forward, DinoEngine.step, DinoEngine.forward_backward, FeatureExtractor.__init__):
        assert "erase" not in inspect.signature(fn).parameters
    assert not any("erase" in inspect.signature(f).parameters for _, f in inspect.getmembers(FeatureExtractor, inspect.isfunction))
    assert "erase" in inspect.signature(SupervisedEngine.step).parameters and "erase" in inspect.signature(SupervisedEngine.forward_backward).parameters


# ------------------------------------------------------------------ the driver
def test_cli_flags_reach_the_sampler_and_refusals():
    sys.path.insert(0, ROOT)
    import train
    from gipvit.cli_spec import REFERENCE_FLAGS
    used = {e["flags"][-1]: e["used"] for e in REFERENCE_FLAGS}
    assert all(used[f] for f in FLAGS) and not used["--resplit"]
    base = ["--model", "vit_tiny", "-b", "8"]
    a, _ = train.parse_args(base)
    train.check_supported(a, lambda m: None)
    assert train.build_erase_sampler(a, 64) is None                              # --reprob 0 (the default): nothing is built
    a, _ = train.parse_args(base + ["--reprob", "0.25"])
    train.check_supported(a, lambda m: None)
    s = train.build_erase_sampler(a, 64)
    assert (s.prob, s.mode, s.count, s.B, s.img) == (0.25, "pixel", 1, 8, 64)
    a, _ = train.parse_args(base + ["--reprob", "1.0", "--remode", "rand", "--recount", "8", "--seed", "5", "--mixup", "0.8"])
    train.check_supported(a, lambda m: None)
    s = train.build_erase_sampler(a, 96, rank=1)
    assert (s.prob, s.mode, s.count, s.B, s.img) == (1.0, "rand", 8, 8, 96)
    assert not np.array_equal(s.sample_host()[0], train.build_erase_sampler(a, 96, rank=0).sample_host()[0])        # a stream per rank
    a, _ = train.parse_args(base + ["--remode", "const", "--recount", "2"])      # without --reprob: legal, and nothing is built
    train.check_supported(a, lambda m: None)
    assert train.build_erase_sampler(a, 64) is None
    bad = [["--dino", "--opt", "adamw", "--reprob", "0.25"], ["--dino", "--opt", "adamw", "--remode", "const"], ["--dino", "--opt", "adamw", "--recount", "2"],
           ["--reprob", "-0.1"], ["--reprob", "1.5"], ["--reprob", "0.25", "--remode", "noise"], ["--remode", "zeros"],
           ["--reprob", "0.25", "--recount", "0"], ["--reprob", "0.25", "--recount", "9"], ["--recount", "-1"]]
    for b in bad:
        a, _ = train.parse_args(base + b)
        with pytest.raises(SystemExit):
            train.check_supported(a, lambda m: None)
    a, _ = train.parse_args(base + ["--dino", "--opt", "adamw"])                 # the defaults do not trip the --dino refusal
    train.check_supported(a, lambda m: None)
    src = open(os.path.join(ROOT, "train.py")).read()
    assert "args.resplit" not in src
