"""CPU: Macenko stain normalisation (gipvit/stainnorm.py, ``--stain-normalize``).  The fp64 restatement against a textbook
Macenko with exact percentiles, the histogram percentile, the normalisation's effect on two synthetic slides, the fallbacks, the
CLI, the launch traces with the flag off, and the ctypes layout of the new argument records."""
import ctypes
import math
from fractions import Fraction
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gipvit import stainnorm as SN
from gipvit.stain import stain_reference

BINS = 4096
# Two slides' stain vectors.  Every component is >= 0.2 on purpose: the tissue mask asks for od >= beta in EVERY channel, so a
# stain with a near-zero channel (Ruifrok & Johnston's eosin, 0.07 in red) loses its pure pixels to the mask on one slide and not
# on the other, and Macenko's extreme-angle estimate -- textbook or histogram alike -- then differs by that, about one grey level.
H_VEC, E_VEC = (0.56, 0.72, 0.41), (0.22, 0.80, 0.56)
H_VEC2, E_VEC2 = (0.65, 0.65, 0.40), (0.30, 0.75, 0.59)                # another scanner / batch of stain


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def concentrations(shape, seed, k=2.0, scale=(0.35, 0.25)):
    """The concentration field of a synthetic slide: gamma-distributed (shape ``k``) H and E per pixel, 15 % of the pixels near
    white, and the od noise of every pixel."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    cH, cE = rng.gamma(k, scale[0], n), rng.gamma(k, scale[1], n)
    white = rng.random(n) < 0.15
    cH[white], cE[white] = rng.uniform(0, 0.02, white.sum()), rng.uniform(0, 0.02, white.sum())
    return cH, cE, rng.normal(0.0, 0.01, (n, 3))


def he_tiles(shape, seed, h_vec=H_VEC, e_vec=E_VEC, strength=(1.0, 1.0), field=None):
    """Seeded synthetic H&E tiles uint8 [n, h, w, 3]: two stain vectors, gamma-distributed concentrations, 15 % near-white
    pixels, od noise 0.01, in the project's od convention."""
    cH, cE, noise = field if field is not None else concentrations(shape, seed)
    od = np.outer(cH * strength[0], _unit(h_vec)) + np.outer(cE * strength[1], _unit(e_vec)) + noise
    v = np.clip(np.rint(256.0 * np.exp(-np.maximum(od, 0.0)) - 1.0), 0, 255).astype(np.uint8)
    return v.reshape(*shape, 3)


def textbook_macenko(tiles, beta=0.15, alpha=1.0):
    """Macenko's method as the usual scripts write it (np.cov, np.percentile on the exact angles and concentrations, no
    histogram), in the project's od convention and with the definition's orientation rule."""
    od = -np.log((tiles.reshape(-1, 3).astype(np.float64) + 1.0) / 256.0)
    odhat = od[~np.any(od < beta, axis=1)]
    _, vec = np.linalg.eigh(np.cov(odhat.T))
    V = vec[:, [2, 1]]
    V = V * np.where(V.sum(axis=0) < 0, -1.0, 1.0)
    t = odhat @ V
    phi = np.arctan2(t[:, 1], t[:, 0])
    lo, hi = np.percentile(phi, alpha), np.percentile(phi, 100.0 - alpha)
    v1, v2 = V @ np.array([math.cos(lo), math.sin(lo)]), V @ np.array([math.cos(hi), math.sin(hi)])
    HE = np.stack([v1, v2] if v1[0] > v2[0] else [v2, v1], axis=1)
    C = np.linalg.lstsq(HE, od.T, rcond=None)[0]
    return dict(phi_lo=lo, phi_hi=hi, HE=HE, maxC=np.percentile(C, 99, axis=1), n=len(odhat))


def _angle_deg(a, b):
    return math.degrees(math.acos(min(1.0, abs(float(a @ b)) / (np.linalg.norm(a) * np.linalg.norm(b)))))


# ---- 1. the restatement against the textbook ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", [((6, 48, 40), 1), ((4, 64, 64), 2)])
def test_reference_against_textbook(shape, seed):
    tiles = he_tiles(shape, seed)
    ref, tb = SN.macenko_reference(tiles, 0.15, 1.0, BINS), textbook_macenko(tiles)
    assert ref["on"] and ref["n"] == tb["n"] and ref["v_max"] == 219
    wa = 2.0 * math.pi / BINS
    d_lo, d_hi = abs(ref["phi_lo"] - tb["phi_lo"]) / wa, abs(ref["phi_hi"] - tb["phi_hi"]) / wa
    d_c = np.abs(ref["maxC"] - tb["maxC"]) / (ref["cmax"] / BINS)
    deg = [_angle_deg(ref["HE"][:, k], tb["HE"][:, k]) for k in range(2)]
    print(f"{shape}: phi_lo {d_lo:.3f} phi_hi {d_hi:.3f} bin widths, maxC {d_c.round(3)} bin widths, vectors {np.round(deg, 4)} deg")
    assert d_lo <= 1.0 and d_hi <= 1.0
    assert (d_c <= 1.0).all()
    assert max(deg) <= 0.1
    # the intermediates are the definition's: the histograms count every pixel they should
    assert ref["angle_hist"].sum() == ref["n"] and (ref["conc_hist"].sum(axis=1) == ref["n_pixels"]).all()
    assert np.allclose(np.linalg.norm(ref["HE"], axis=0), 1.0, atol=1e-12) and ref["HE"][0, 0] > ref["HE"][0, 1]
    assert ref["record"]["on"][0] == 1 and not ref["record"]["b"].any()


# ---- 2. the percentile of a histogram ----------------------------------------------------------------------------------------
def test_hist_percentile_exact_cases():
    hp = SN.hist_percentile
    # a single bin of 5 values over [2, 4): the value of rank i sits at the centre of cell i of 5, 2 + (i + 1/2) / 5 * 2
    assert hp([5], 0, 2.0, 4.0, 0.0) == 2.2
    assert hp([5], 0, 2.0, 4.0, 50.0) == 3.0
    assert hp([5], 0, 2.0, 4.0, 100.0) == 3.8
    assert hp([5], 0, 2.0, 4.0, 62.5) == 3.2                                # r = 2.5: half way from rank 2 (3.0) to rank 3 (3.4)
    assert hp([1], 0, 2.0, 4.0, 37.0) == 3.0                                # one value: the centre of its bin, whatever p
    # rank on a bin boundary: 4 + 4 + 3 values in three bins over [0, 3); n - 1 = 10
    assert hp([4, 4, 3], 0, 0.0, 3.0, 40.0) == 1.125                        # r = 4: the first value of bin 1, centre of cell 0 of 4
    assert hp([4, 4, 3], 0, 0.0, 3.0, 30.0) == 0.875                        # r = 3: the last value of bin 0
    assert hp([4, 4, 3], 0, 0.0, 3.0, 35.0) == 1.0                          # r = 3.5: between them, on the edge itself
    assert hp([4, 4, 3], 0, 0.0, 3.0, 100.0) == float(Fraction(17, 6))
    # empty bins between two ranks are crossed by the interpolation, as np.percentile crosses the gap between two values
    assert hp([1, 0, 0, 1], 0, 0.0, 4.0, 50.0) == 2.0                       # 0.5 and 3.5, half way
    assert hp([1, 0, 0, 1], 0, 0.0, 4.0, 25.0) == 1.25
    # everything in the underflow count
    assert hp([0, 0, 0, 0], 9, 0.5, 2.5, 99.0) == 0.5
    assert hp([0, 3], 7, 0.0, 2.0, 50.0) == 0.0                             # r = 4.5 < 7
    assert hp([0, 3], 7, 0.0, 2.0, 100.0) == float(Fraction(11, 6))               # r = 9: the last of the 3 in bin 1
    assert hp([0, 4], 4, 0.0, 2.0, 50.0) == 0.5 * 1.125                     # r = 3.5: from the underflow (lo) to the first of bin 1
    # counts past 2^53 stay exact (integer arithmetic): n - 1 = 2^61 + 3 is no fp64 number, r = 2^60 + 1.5 lies half way between
    # the two values of bin 1 (1.25 and 1.75); in floating point r would round to 2^60 + 2, the second of them
    big = 1 << 60
    assert hp([big + 1, 2, big + 1], 0, 0.0, 3.0, 50.0) == 1.5
    assert hp([big, 1, big], 0, 0.0, 3.0, 50.0) == 1.5                      # r = 2^60 exactly: the one value of bin 1
    with pytest.raises(ValueError):
        hp([0, 0], 0, 0.0, 1.0, 50.0)
    with pytest.raises(ValueError):
        hp([1], 0, 0.0, 1.0, 101.0)


# ---- 3. what it is for -------------------------------------------------------------------------------------------------------
def test_two_slides_meet_after_normalisation():
    shape = (4, 64, 64)
    field = concentrations(shape, 5)
    a = he_tiles(shape, 0, H_VEC, E_VEC, (1.0, 1.0), field)
    b = he_tiles(shape, 0, H_VEC2, E_VEC2, (1.5, 0.7), field)
    raw = np.abs(a.reshape(-1, 3).mean(0) - b.reshape(-1, 3).mean(0))
    out = []
    for t in (a, b):
        rec = SN.macenko_reference(t)["record"]
        assert rec["on"][0] == 1
        out.append(stain_reference(t, rec["A"][0], rec["b"][0])[1].reshape(-1, 3).astype(np.float64).mean(0))
    norm = np.abs(out[0] - out[1])
    print(f"mean colour difference raw {raw.round(2)} normalised {norm.round(3)}")
    assert raw.max() > 10.0
    assert norm.max() < 1.0


# ---- 4. fallbacks and the identity -------------------------------------------------------------------------------------------
def test_fallbacks():
    white = np.full((2, 16, 16, 3), 255, np.uint8)
    r = SN.macenko_reference(white)
    assert not r["on"] and r["reason"] == SN.FEW_TISSUE and r["n"] == 0 and r["record"]["on"][0] == 0
    assert np.array_equal(r["record"]["A"][0], np.eye(3, dtype=np.float32)) and not r["record"]["b"].any()
    one = np.empty((2, 16, 16, 3), np.uint8)
    one[...] = (120, 80, 150)
    r = SN.macenko_reference(one)
    assert not r["on"] and r["reason"] == SN.COLLINEAR and r["n"] == one.size // 3 and r["record"]["on"][0] == 0
    single = white.copy()
    single[1, 3, 4] = (100, 60, 140)
    r = SN.macenko_reference(single)
    assert not r["on"] and r["reason"] == SN.FEW_TISSUE and r["n"] == 1
    st = r["stain"]
    assert isinstance(st, SN.SlideStain) and not st.on and st.n_tissue == 1 and st.n_pixels == 512 and np.isnan(st.HE).all()


def test_target_maps_onto_itself():
    """Tiles synthesised from the target's own vectors, with the target's 99th-percentile concentrations: A is the identity on the
    tissue plane (the span of H and E) to 5 %.  Macenko's premise is that the extreme angles ARE the stains, i.e. that more than
    alpha % of the tissue is dominated by one stain: the field here is gamma with shape 0.7 (mass near zero), which has such
    pixels -- seeds 9 .. 16 give 3.3 .. 5.0 %, the rest being the outward pull of the od noise on the 1st / 99th angle percentile
    (about 1 degree; without noise: 1.5 .. 1.9 %).  With shape 2, where nearly every pixel is a mixture, the estimate sits inside the
    true vectors and the same figure is 10 .. 12 %, for the textbook method as for this one."""
    tg = SN.MacenkoTarget()
    shape = (4, 64, 64)
    cH, cE, noise = concentrations(shape, 9, k=0.7, scale=(1.0, 0.7))
    field = (cH * tg.maxC[0] / np.percentile(cH, 99), cE * tg.maxC[1] / np.percentile(cE, 99), noise)
    r = SN.macenko_reference(he_tiles(shape, 0, tg.HE[:, 0], tg.HE[:, 1], field=field))
    assert r["on"]
    plane = tg.HE.T                                                        # rows: od of pure H and pure E
    err = np.linalg.norm(plane @ r["A"] - plane) / np.linalg.norm(plane)
    print(f"identity on the tissue plane: relative error {err:.4f}")
    assert err <= 0.05
    # and exactly: a slide whose estimate IS the target gets HE_t pinv(HE_t), which fixes every od on the plane
    rec = SN.normaliser_record(tg.HE, tg.maxC, tg)
    assert np.allclose(plane @ rec["A"][0].astype(np.float64), plane, atol=1e-6)


def test_parameter_checks():
    for kw in (dict(beta=0.0), dict(beta=math.log(256.0)), dict(alpha=0.0), dict(alpha=50.0), dict(bins=255), dict(bins=4097), dict(max_tiles=-1)):
        with pytest.raises(ValueError):
            SN.MacenkoEstimator("cpu", **kw)
    assert SN.tissue_v_max(0.15) == 219
    with pytest.raises(ValueError):
        SN.MacenkoTarget(maxC=(1.0, 0.0))


# ---- 5. CLI, and nothing changes with the flag off ---------------------------------------------------------------------------
BASE = ["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2"]


@pytest.mark.parametrize("extra,flag", [
    (["--stain-normalize", "vahadane"], "--stain-normalize"),
    (["--stain-normalize", "macenko", "--stain-norm-beta", "0"], "--stain-norm-beta"),
    (["--stain-normalize", "macenko", "--stain-norm-beta", "5.6"], "--stain-norm-beta"),
    (["--stain-normalize", "macenko", "--stain-norm-alpha", "50"], "--stain-norm-alpha"),
    (["--stain-normalize", "macenko", "--stain-norm-alpha", "nan"], "--stain-norm-alpha"),
    (["--stain-normalize", "macenko", "--stain-norm-tiles", "-1"], "--stain-norm-tiles"),
])
def test_flags_refused_before_any_gpu_work(extra, flag, monkeypatch):
    sys.path.insert(0, ROOT)
    import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flag must be refused before the device is looked at"))
    args, _ = train.parse_args(BASE + extra)                       # parsing alone accepts the text
    with pytest.raises(SystemExit) as e:
        train.check_stain_normalize(args)
    assert flag in str(e.value)
    with pytest.raises(SystemExit) as e:
        train.main(BASE + extra)
    assert flag in str(e.value)


def test_flag_defaults_and_float_hook_refused(monkeypatch):
    sys.path.insert(0, ROOT)
    import train
    args, _ = train.parse_args(BASE)
    assert (args.stain_normalize, args.stain_norm_tiles, args.stain_norm_beta, args.stain_norm_alpha) == ("none", 0, 0.15, 1.0)
    train.check_stain_normalize(args)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("refused before the device is looked at"))
    monkeypatch.setattr(train, "hook_batch_format", lambda *a, **k: "f32_nchw")
    with pytest.raises(SystemExit) as e:
        train.main(BASE + ["--stain-normalize", "macenko"], transform=lambda t: t)
    assert "--stain-normalize" in str(e.value) and "uint8" in str(e.value)


def test_traces_without_the_flag_name_no_stain_entry_point():
    import launch_trace as lt
    fix = lt.load_fixture()
    for cid in ("fx", "dino_t"):
        events, _ = lt.trace(cid)
        got = lt.summary(events)
        assert not [n for n in got["names"] if "stain" in n], cid
        assert '"stain"' not in "\n".join(lt._lines(events))
        assert got["sha256"] == fix[cid]["sha256"], f"{cid}: the launch trace moved"


def test_trace_with_a_record_patchifies_through_the_stain_kernel():
    """On the CPU recorder: with a record set every patchify call of the extractor carries the B-record table; taking it off
    restores the plain calls."""
    import launch_trace as lt
    from gipvit.engine import FeatureExtractor
    with lt.recording() as rec:
        fx = FeatureExtractor(arch="vit_tiny", img_size=64, batch=2, num_classes=0, device="cpu")
        fx.set_stain(SN.normaliser_record(SN.MacenkoTarget().HE, (1.5, 0.9)))
        tiles = torch.zeros(3, 64, 64, 3, dtype=torch.uint8)
        fx.run(tiles)
        fx.intermediate_layers(tiles)
        n_on = len(rec.events)
        with pytest.raises(ValueError, match="float32"):
            fx.run(torch.zeros(3, 3, 64, 64))
        fx.set_stain(None)
        fx.run(tiles)
    calls = [e for e in rec.events if e[0] == "patchify"]
    on = [e for e in rec.events[:n_on] if e[0] == "patchify"]
    assert len(on) == 4 and len(calls) == 6
    for e in on:
        assert e[2]["stain"]["tensor"][2] == [2 * 52] and e[2]["stain"]["tensor"][4] == "torch.uint8"
    assert all("stain" not in e[2] for e in calls[4:])
    assert not [e for e in rec.events if e[0] == "patchify_nchw"]


# ---- 6. the binding --------------------------------------------------------------------------------------------------------
def test_new_structs_have_the_headers_layout(tmp_path):
    from gipvit import _lib
    names = ["gv_stain_params", "gv_stain_stats_args", "gv_stain_angle_hist_args", "gv_stain_conc_hist_args", "gv_stain_apply_args",
             "gv_patchify_stain_args"]
    fields = [("gv_stain_angle_hist_args", "V"), ("gv_stain_angle_hist_args", "out"), ("gv_stain_conc_hist_args", "pinv"),
              ("gv_stain_conc_hist_args", "cmax"), ("gv_stain_conc_hist_args", "out"), ("gv_stain_stats_args", "out"),
              ("gv_stain_apply_args", "img_stride"), ("gv_patchify_stain_args", "stain")]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "gipvit.h"\nint main(){'
           + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
           + "".join(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for s, f in fields) + "return 0;}")
    exe = str(tmp_path / "sizeof_stainnorm")
    r = subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    out = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True).stdout.splitlines())
    for n in names:
        assert int(out[n]) == ctypes.sizeof(getattr(_lib, n)), n
    for s, f in fields:
        assert int(out[f"{s}.{f}"]) == getattr(getattr(_lib, s), f).offset, (s, f)
    for sym in ("gv_stain_stats", "gv_stain_angle_hist", "gv_stain_conc_hist", "gv_stain_apply", "gv_patchify_stain", "gv_patchify_stain_f32"):
        assert sym in _lib.ENTRY_POINTS and hasattr(_lib.lib, sym)


def test_argument_checks_come_back_through_the_abi_without_a_gpu():
    """Refused before any launch: nothing here touches a device."""
    from gipvit import _lib
    P = 1 << 20
    a = _lib.gv_stain_stats_args()
    assert _lib.lib.gv_stain_stats(ctypes.byref(a), None) == -3
    a = _lib.gv_stain_stats_args(P, 3 * 16 * 16, 1, 16, 16, 219, P + 4, P)
    assert _lib.lib.gv_stain_stats(ctypes.byref(a), None) == -2 and b"aligned" in _lib.lib.gv_last_error()
    a = _lib.gv_stain_stats_args(P, 3 * 65536 * 65536, 1, 65536, 65536, 219, P, P)
    assert _lib.lib.gv_stain_stats(ctypes.byref(a), None) == -1 and b"2^32" in _lib.lib.gv_last_error()
    for nb in (255, 4097, 0):
        h = _lib.gv_stain_angle_hist_args(); h.tiles = h.workspace = h.out = P; h.img_stride, h.n, h.h, h.w, h.v_max, h.n_bins = 768, 1, 16, 16, 219, nb
        assert _lib.lib.gv_stain_angle_hist(ctypes.byref(h), None) == -1 and b"n_bins" in _lib.lib.gv_last_error()
        c = _lib.gv_stain_conc_hist_args(); c.tiles = c.workspace = c.out = P; c.img_stride, c.n, c.h, c.w, c.n_bins = 768, 1, 16, 16, nb
        c.cmax[0] = c.cmax[1] = 1.0
        assert _lib.lib.gv_stain_conc_hist(ctypes.byref(c), None) == -1 and b"n_bins" in _lib.lib.gv_last_error()
    s = _lib.gv_stain_apply_args(P, P, None, 768, 1, 16, 16)
    assert _lib.lib.gv_stain_apply(ctypes.byref(s), None) == -3
    s = _lib.gv_stain_apply_args(P, P, P + 2, 768, 1, 16, 16)
    assert _lib.lib.gv_stain_apply(ctypes.byref(s), None) == -2
    p = _lib.gv_patchify_stain_args(); p.p.tiles = p.p.patches = P
    assert _lib.lib.gv_patchify_stain(ctypes.byref(p), None) == -3 and b"stain" in _lib.lib.gv_last_error()
    p.stain = P + 1
    assert _lib.lib.gv_patchify_stain_f32(ctypes.byref(p), None) == -2 and b"stain" in _lib.lib.gv_last_error()
