"""GPU: Macenko stain normalisation at inference -- the three estimation passes (gv_stain_stats / _angle_hist / _conc_hist), the
estimator end to end against gipvit.stainnorm.macenko_reference (fp64), gv_stain_apply against gipvit.stain.stain_reference,
gv_patchify_stain against gv_patchify over gv_stain_apply's bytes (bit for bit), the argument checks, FeatureExtractor.set_stain,
validate() / the k-NN monitor with a normaliser, and the driver with --stain-normalize.

Inputs are tiny on purpose: 6 tiles of 48 x 40 (tile_h != tile_w, 45 workgroups), one tile of 16 x 16 (one workgroup) and 70
tiles of 16 x 16 (70 partials: more than the 64 one round of the fixed-order sum takes).

The tie rule of test 4 is tests/test_stain_gpu.py's: the device evaluates the map in f32, the reference in fp64; a value whose fp64
result lies within DELTA = 0.01 of a rounding tie x.5 inside (-0.5, 255.5) may come out as either neighbouring byte, every other
value must be the reference's byte.

The histogram rule of test 2: the device's atan2 / products may differ from numpy's in the last place, so a pixel whose reference
position lies within EDGE = 1e-9 bins of a bin edge may fall on either side; every bin may differ from the reference's by at most
the number of such pixels at its two edges."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DELTA, EDGE, BINS = 0.01, 1e-9, 4096
GV_E_SHAPE, GV_E_ALIGN, GV_E_NULL = -1, -2, -3
SHAPES = {"t6": (6, 48, 40), "t1": (1, 16, 16), "t70": (70, 16, 16)}


class Case:
    """One input: the tiles, the fp64 reference (computed once, never changed) and the device copy."""

    def __init__(self, dev, name):
        from gipvit import stainnorm as SN
        from test_stainnorm_host import he_tiles
        self.shape = SHAPES[name]
        self.tiles = he_tiles(self.shape, {"t6": 1, "t1": 3, "t70": 4}[name])
        # a pure white pixel has od = 0 and concentration 0 exactly, ON the edge between the underflow count and bin 0: the test
        # holds its inputs to <= 0.1 % pixels at an edge, so the 0.3 % of them become (254, 254, 254)
        self.tiles[(self.tiles == 255).all(axis=-1)] = 254
        self.ref = SN.macenko_reference(self.tiles, 0.15, 1.0, BINS)
        assert self.ref["on"], (name, self.ref["reason"])
        self.t_dev = torch.from_numpy(self.tiles).to(dev)


@pytest.fixture(scope="module")
def cases(dev):
    return {n: Case(dev, n) for n in SHAPES}


def _edge_counts(pos, bins):
    """Pixels within EDGE of bin edge e, for e = 0 .. bins (pos: the reference's position in bins)."""
    e = np.rint(pos)
    near = np.abs(pos - e) <= EDGE
    return np.bincount(np.clip(e[near], 0, bins).astype(np.int64), minlength=bins + 1), int(near.sum())


# ---- 1. pass 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_stain_stats(cases, name):
    from gipvit import ops, stainnorm as SN
    c = cases[name]
    n_dev, s_dev = ops.stain_stats(c.t_dev, 219)
    n_dev, s = int(n_dev.cpu()[0]), s_dev.cpu().numpy()
    px = c.tiles.reshape(-1, 3)
    od = SN.od_table()[px][(px <= 219).all(axis=1)]
    assert n_dev == len(od) == c.ref["n"]                                              # exact
    r, g, b = od[:, 0], od[:, 1], od[:, 2]
    want = [math.fsum(v) for v in (r, g, b, r * r, r * g, r * b, g * g, g * b, b * b)]   # numpy's terms, summed exactly
    rel = max(abs(a - w) / w for a, w in zip(s, want))
    bound = (n_dev + 2) * 2.0 ** -52
    print(f"{name}: n {n_dev}, {ops._stain_groups(px.shape[0])} partials, worst relative error {rel:.3e} (bound {bound:.3e})")
    assert rel <= bound
    n2, s2 = ops.stain_stats(c.t_dev, 219)
    assert torch.equal(n2.cpu(), torch.tensor([n_dev])) and np.array_equal(s2.cpu().numpy().view(np.int64), s.view(np.int64))     # bitwise
    # the mask is the byte test: one level up lets more pixels in
    assert int(ops.stain_stats(c.t_dev, 255)[0].cpu()[0]) == px.shape[0]


# ---- 2. passes 2 and 3 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_histograms(cases, name):
    from gipvit import ops
    c, ref = cases[name], cases[name].ref
    n_px = ref["n_pixels"]
    ah = ops.stain_angle_hist(c.t_dev, ref["V"], 219, BINS).cpu().numpy()
    assert ah.shape == (BINS,) and int(ah.sum()) == ref["n"]                           # exact
    edges, n_amb = _edge_counts(ref["angle_pos"], BINS)
    assert n_amb <= 0.001 * ref["n"]
    allowed = edges[:-1] + edges[1:]
    allowed[0] += edges[0]; allowed[-1] += edges[-1]                                    # the clamp
    diff = np.abs(ah - ref["angle_hist"])
    print(f"{name}: angle bins off {int((diff > 0).sum())}, ambiguous pixels {n_amb}")
    assert (diff <= allowed).all()
    ch = ops.stain_conc_hist(c.t_dev, ref["pinv"], ref["cmax"], BINS).cpu().numpy()
    assert ch.shape == (2, BINS + 1) and (ch.sum(axis=1) == n_px).all()                # exact, underflow included
    for k in range(2):
        edges, n_amb = _edge_counts(ref["conc_pos"][k], BINS)
        assert n_amb <= 0.001 * n_px
        allowed = np.empty(BINS + 1, np.int64)
        allowed[:BINS] = edges[:-1] + edges[1:]
        allowed[BINS - 1] += edges[BINS]
        allowed[BINS] = edges[0]                                                       # c = 0: the underflow's only edge
        diff = np.abs(ch[k] - ref["conc_hist"][k])
        print(f"{name}: stain {k} bins off {int((diff > 0).sum())}, ambiguous pixels {n_amb}, underflow {int(ch[k, BINS])}")
        assert (diff <= allowed).all()
    # other bin counts take the same path
    ah = ops.stain_angle_hist(c.t_dev, ref["V"], 219, 256).cpu().numpy()
    pos = ref["angle_pos"] * 256.0 / BINS
    want = np.bincount(np.clip(np.floor(pos), 0, 255).astype(np.int64), minlength=256)
    assert int(ah.sum()) == ref["n"] and int(np.abs(ah - want).sum()) <= 2 * _edge_counts(pos, 256)[1]
    # bitwise the same twice
    assert np.array_equal(ch, ops.stain_conc_hist(c.t_dev, ref["pinv"], ref["cmax"], BINS).cpu().numpy())


# ---- 3. the estimator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_fit_against_the_reference(cases, dev, name):
    from gipvit import stainnorm as SN
    c, ref = cases[name], cases[name].ref
    st = SN.MacenkoEstimator(dev, 0.15, 1.0, BINS).fit(c.t_dev)
    assert st.on and st.reason == "" and st.n_tissue == ref["n"] and st.n_pixels == ref["n_pixels"]
    amb = _edge_counts(ref["angle_pos"], BINS)[1] + sum(_edge_counts(ref["conc_pos"][k], BINS)[1] for k in range(2))
    d_he, d_c = float(np.abs(st.HE - ref["HE"]).max()), np.abs(st.maxC - ref["maxC"])
    print(f"{name}: ambiguous pixels {amb}, |dHE| {d_he:.3e}, |dmaxC| {d_c}")
    if amb == 0:
        assert d_he <= 1e-9 and (d_c <= 1e-9).all()
        assert float(np.abs(st.record["A"] - ref["record"]["A"]).max()) <= 1e-6
    else:
        assert d_he <= 2.0 * math.pi / BINS and (d_c <= ref["cmax"] / BINS).all()
    assert st.record["on"][0] == 1 and not st.record["b"].any()
    # max_tiles: the first tiles only
    if c.shape[0] > 2:
        st2 = SN.MacenkoEstimator(dev, 0.15, 1.0, BINS, max_tiles=2).fit(c.t_dev)
        ref2 = SN.macenko_reference(c.tiles[:2], 0.15, 1.0, BINS)
        assert st2.n_pixels == ref2["n_pixels"] and st2.n_tissue == ref2["n"] and st2.on == ref2["on"]


def test_fallbacks_on_the_device(dev):
    from gipvit import stainnorm as SN
    est = SN.MacenkoEstimator(dev)
    white = torch.full((2, 16, 16, 3), 255, dtype=torch.uint8, device=dev)
    st = est.fit(white)
    assert not st.on and st.reason == SN.FEW_TISSUE and st.n_tissue == 0 and st.record["on"][0] == 0
    one = torch.empty((2, 16, 16, 3), dtype=torch.uint8, device=dev)
    one[...] = torch.tensor([120, 80, 150], dtype=torch.uint8, device=dev)
    st = est.fit(one)
    assert not st.on and st.reason == SN.COLLINEAR and st.n_tissue == 512
    single = white.clone()
    single[1, 3, 4] = torch.tensor([100, 60, 140], dtype=torch.uint8, device=dev)
    st = est.fit(single)
    assert not st.on and st.reason == SN.FEW_TISSUE and st.n_tissue == 1 and st.n_pixels == 512
    with pytest.raises(ValueError, match="uint8"):
        est.fit(torch.zeros(2, 3, 16, 16, device=dev))


# ---- 4. gv_stain_apply -------------------------------------------------------------------------------------------------------
def _records(cases, n, seed=0):
    """n records: the case's own normaliser, jitter records (b != 0), a normaliser towards another target, and every third one off
    with an A and b that must not be looked at."""
    from gipvit import stainnorm as SN
    from gipvit.stain import DT, stain_record
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, DT)
    other = SN.MacenkoTarget(HE=((0.65, 0.30), (0.65, 0.75), (0.40, 0.59)), maxC=(1.4, 1.2))
    for i in range(n):
        if i % 3 == 2:
            rec[i]["A"], rec[i]["b"] = 7.0, -3.0
        elif i % 3 == 0:
            r = cases["t6"].ref
            rec[i] = SN.normaliser_record(r["HE"], r["maxC"], None if i % 2 == 0 else other)[0]
        else:
            rec[i] = stain_record(rng.uniform(0.7, 1.3, 3), rng.uniform(-0.2, 0.2, 3))
    return rec


def _pack(rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1).copy())


@pytest.mark.parametrize("name", list(SHAPES))
def test_stain_apply_against_fp64_with_the_tie_rule(cases, dev, name):
    from gipvit import ops
    from gipvit.stain import stain_reference
    c = cases[name]
    n = c.shape[0]
    rec = _records(cases, n)
    D = ops.stain_apply(c.t_dev, _pack(rec).to(dev)).cpu().numpy()
    on = rec["on"] != 0
    x, ref = c.tiles.astype(np.float64), c.tiles.copy()
    for i in np.nonzero(on)[0]:
        x[i], ref[i] = stain_reference(c.tiles[i], rec[i]["A"], rec[i]["b"])
    assert np.array_equal(D[~on], c.tiles[~on])                                        # on = 0: copied bit for bit
    amb = (np.abs(x - np.floor(x) - 0.5) <= DELTA) & (x > -0.5) & (x < 255.5)
    amb[~on] = False
    share = amb[on].mean()
    print(f"{name}: ambiguous share {share:.4f}, bytes off the reference {(D != ref).sum()} of {D.size}")
    assert share <= 0.05
    lo, hi = np.clip(np.floor(x), 0, 255).astype(np.uint8), np.clip(np.ceil(x), 0, 255).astype(np.uint8)
    good = (D == ref) | (amb & ((D == lo) | (D == hi)))
    if not good.all():
        i, y, xx, ch = (int(v) for v in np.argwhere(~good)[0])
        pytest.fail(f"{int((~good).sum())} wrong bytes; first: tile {i} pixel ({y}, {xx}) channel {ch}: fp64 {x[i, y, xx, ch]!r}, reference "
                    f"{ref[i, y, xx, ch]}, device {D[i, y, xx, ch]}, input {c.tiles[i, y, xx].tolist()}, record {rec[i]}")
    assert (D[on] != c.tiles[on]).mean() > 0.3                                         # and the map did something
    # a strided view along the tiles and an out= buffer
    if n >= 4:
        got = ops.stain_apply(c.t_dev[::2], _pack(rec[::2]).to(dev), out=torch.empty_like(c.t_dev[::2]).contiguous())
        assert np.array_equal(got.cpu().numpy(), D[::2])


# ---- 5. patchify with the map inside -----------------------------------------------------------------------------------------
MEAN, STD = (0.8998, 0.8253, 0.9357), (0.1125, 0.1751, 0.0787)


@pytest.mark.parametrize("wide", [False, True], ids=["16bit", "f32"])
@pytest.mark.parametrize("name,crop,windows", [
    ("t6", 32, [(0, 0)]), ("t6", 32, [(0, 0), (16, 8)]), ("t6", 32, [(3, 5)]), ("t6", 16, [(31, 23), (0, 1)]),
    ("t1", 16, [(0, 0)]), ("t70", 16, [(0, 0)])])
def test_patchify_stain_is_patchify_of_the_stained_bytes(cases, dev, name, crop, windows, wide):
    from gipvit import ops
    c = cases[name]
    n = c.shape[0]
    P = (crop // 16) ** 2
    table = _pack(_records(cases, n, seed=1)).to(dev)
    stained = ops.stain_apply(c.t_dev, table)
    mk = lambda: torch.full((n * len(windows) * P, 768), float("nan"), dtype=torch.float32 if wide else ops.bf16, device=dev)
    got = ops.patchify(c.t_dev, windows, crop, MEAN, STD, out=mk(), stain=table)
    want = ops.patchify(stained, windows, crop, MEAN, STD, out=mk())
    assert torch.equal(got, want) and bool(torch.isfinite(got.float()).all())
    assert not torch.equal(got, ops.patchify(c.t_dev, windows, crop, MEAN, STD, out=mk()))
    # fill= is applied after the stain, as after Normalize
    fill = torch.zeros(n, 8, dtype=torch.float32, device=dev)
    fill[:, :4] = torch.tensor([2.0, crop - 3.0, 1.0, crop - 6.0])
    fill[:, 4:7] = torch.tensor([0.25, -1.5, 3.0])
    fill[::2, 7] = 1.0
    got = ops.patchify(c.t_dev, windows, crop, MEAN, STD, out=mk(), stain=table, fill=fill)
    assert torch.equal(got, ops.patchify(stained, windows, crop, MEAN, STD, out=mk(), fill=fill))
    # every record off: gv_patchify itself
    off = _records(cases, n, seed=1)
    off["on"] = 0
    got = ops.patchify(c.t_dev, windows, crop, MEAN, STD, out=mk(), stain=_pack(off).to(dev))
    assert torch.equal(got, ops.patchify(c.t_dev, windows, crop, MEAN, STD, out=mk()))
    with pytest.raises(ValueError, match="stain"):
        ops.patchify(c.t_dev, windows[:1], crop, MEAN, STD, stain=table, erase=(torch.zeros(1, dtype=torch.uint8, device=dev), 0))


# ---- 6. argument checks ------------------------------------------------------------------------------------------------------
def test_argument_checks_come_before_any_launch(cases, dev):
    from gipvit import _lib as L, ops
    c = cases["t6"]
    n, h, w = c.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = _pack(_records(cases, n)).to(dev)
    shifted = torch.zeros(table.numel() + 8, dtype=torch.uint8, device=dev)
    out_p = torch.full((n * 4, 768), 3.0, dtype=ops.bf16, device=dev)
    out_u8 = torch.full((n, h, w, 3), 77, dtype=torch.uint8, device=dev)
    ws = torch.full((1 << 18,), 5, dtype=torch.int64, device=dev)       # 2 MiB: past the 45 x 2 x 4097 x 4 bytes of the largest call here
    out_h = torch.full((2 * (BINS + 1),), 9, dtype=torch.int64, device=dev)

    def patchify_rc(stain, f32=False):
        a = L.gv_patchify_args()
        a.tiles, a.patches, a.n_img, a.tile_h, a.tile_w, a.img_stride, a.n_win, a.crop, a.n_tiles = c.t_dev.data_ptr(), out_p.data_ptr(), n, h, w, h * w * 3, 1, 32, n
        for k in range(3):
            a.mean[k], a.std[k] = MEAN[k], STD[k]
        fn = L.lib.gv_patchify_stain_f32 if f32 else L.lib.gv_patchify_stain
        return fn(ctypes.byref(L.gv_patchify_stain_args(a, stain)), stream)
    assert patchify_rc(None) == GV_E_NULL and b"stain" in L.lib.gv_last_error()
    assert patchify_rc(shifted.data_ptr() + 1) == GV_E_ALIGN and b"stain" in L.lib.gv_last_error()
    assert patchify_rc(shifted.data_ptr() + 2, f32=True) == GV_E_ALIGN
    assert L.lib.gv_patchify_stain(None, stream) == GV_E_NULL

    def apply_rc(stain):
        return L.lib.gv_stain_apply(ctypes.byref(L.gv_stain_apply_args(c.t_dev.data_ptr(), out_u8.data_ptr(), stain, h * w * 3, n, h, w)), stream)
    assert apply_rc(None) == GV_E_NULL and apply_rc(shifted.data_ptr() + 3) == GV_E_ALIGN

    def angle_rc(nb=BINS, wsp=ws.data_ptr(), outp=out_h.data_ptr(), tiles=c.t_dev.data_ptr()):
        a = L.gv_stain_angle_hist_args()
        a.tiles, a.img_stride, a.n, a.h, a.w, a.v_max, a.n_bins, a.workspace, a.out = tiles, h * w * 3, n, h, w, 219, nb, wsp, outp
        for i, v in enumerate(c.ref["V"].reshape(-1)):
            a.V[i] = v
        return L.lib.gv_stain_angle_hist(ctypes.byref(a), stream)

    def conc_rc(nb=BINS, wsp=ws.data_ptr()):
        a = L.gv_stain_conc_hist_args()
        a.tiles, a.img_stride, a.n, a.h, a.w, a.n_bins, a.workspace, a.out = c.t_dev.data_ptr(), h * w * 3, n, h, w, nb, wsp, out_h.data_ptr()
        a.cmax[0] = a.cmax[1] = 1.0
        return L.lib.gv_stain_conc_hist(ctypes.byref(a), stream)
    for nb in (255, 4097, 8192, -1):
        assert angle_rc(nb=nb) == GV_E_SHAPE and b"n_bins" in L.lib.gv_last_error()
        assert conc_rc(nb=nb) == GV_E_SHAPE and b"n_bins" in L.lib.gv_last_error()
    assert angle_rc(tiles=None) == GV_E_NULL and angle_rc(wsp=None) == GV_E_NULL and angle_rc(outp=None) == GV_E_NULL
    assert angle_rc(wsp=ws.data_ptr() + 4) == GV_E_ALIGN and angle_rc(outp=out_h.data_ptr() + 2) == GV_E_ALIGN
    assert conc_rc(wsp=ws.data_ptr() + 1) == GV_E_ALIGN
    s = L.gv_stain_stats_args(c.t_dev.data_ptr(), h * w * 3, n, h, w, 219, ws.data_ptr(), out_h.data_ptr() + 4)
    assert L.lib.gv_stain_stats(ctypes.byref(s), stream) == GV_E_ALIGN
    s = L.gv_stain_stats_args(c.t_dev.data_ptr(), h * w * 3, n, h, w, 256, ws.data_ptr(), out_h.data_ptr())
    assert L.lib.gv_stain_stats(ctypes.byref(s), stream) == GV_E_SHAPE and b"v_max" in L.lib.gv_last_error()
    s = L.gv_stain_stats_args(c.t_dev.data_ptr(), 3 * 65536 * 65536, 1, 65536, 65536, 219, ws.data_ptr(), out_h.data_ptr())
    assert L.lib.gv_stain_stats(ctypes.byref(s), stream) == GV_E_SHAPE and b"2^32" in L.lib.gv_last_error()
    torch.cuda.synchronize()
    assert bool((out_p == 3.0).all()) and bool((out_u8 == 77).all()) and bool((ws == 5).all()) and bool((out_h == 9).all())      # nothing ran
    with pytest.raises(L.GipvitError, match="n_bins"):
        ops.stain_angle_hist(c.t_dev, c.ref["V"], 219, 100)
    with pytest.raises(ValueError, match="stain"):
        ops.stain_apply(c.t_dev, table[:-4])
    assert patchify_rc(table.data_ptr()) == 0 and apply_rc(table.data_ptr()) == 0 and angle_rc() == 0
    torch.cuda.synchronize()
    assert not bool((out_p == 3.0).all()) and not bool((out_u8 == 77).all()) and int(out_h[:BINS].sum()) == c.ref["n"]


# ---- 7. the extractor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_feature_extractor_with_a_record(cases, dev, precision):
    from gipvit import models as M, ops, stainnorm as SN
    from gipvit.engine import FeatureExtractor
    from test_stainnorm_host import he_tiles
    fx = FeatureExtractor("vit_tiny", 64, 4, 2, device=dev, precision=precision)
    fx.load_state(M.init_vit_state("vit_tiny", 64, 2, seed=0))
    tiles = torch.from_numpy(he_tiles((6, 64, 64), 12)).to(dev)                         # 4 + 2: a padded last batch
    st = SN.MacenkoEstimator(dev).fit(tiles)
    assert st.on
    stained = ops.stain_apply(tiles, SN.pack_record(st.record).repeat(6).to(dev))
    assert not torch.equal(stained, tiles)

    def both(fn):
        fx.set_stain(st.record)
        a = fn(tiles)
        fx.set_stain(None)
        return a, fn(stained), fn(tiles)
    for fn in (fx.run, lambda t: fx.intermediate_layers(t, 2), fx.run_with_attention, lambda t: (fx.probe_features(t, 2),),
               lambda t: (fx.last_selfattention(t, cls_only=True),)):
        a, b, plain = both(fn)
        assert all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)
        assert not all(torch.equal(x, y) for x, y in zip(a, plain) if x is not None)
    # an on = 0 record is the plain pass; the packed bytes are accepted as well
    fx.set_stain(SN.off_record())
    off = fx.run(tiles)[0]
    fx.set_stain(SN.pack_record(st.record))
    packed = fx.run(tiles)[0]
    on, _, plain = both(fx.run)
    assert torch.equal(off, plain[0]) and torch.equal(packed, on[0])
    fx.set_stain(st.record)
    with pytest.raises(ValueError, match="float32"):
        fx.run(torch.zeros(6, 3, 64, 64, device=dev))
    fx.set_stain(None)
    fx.run(torch.zeros(6, 3, 64, 64, device=dev))                                       # without a record float input is served as before


# ---- 8. validate() and the monitor -------------------------------------------------------------------------------------------
class HeSlides:
    """data.SyntheticSlides' interface over synthetic H&E slides: slide k has its own stain vectors and strength; slide
    ``white`` is all white (the fallback)."""

    def __init__(self, n_slides, tiles, size, per_iter, white=None, seed=0):
        from test_stainnorm_host import H_VEC, E_VEC, H_VEC2, E_VEC2, he_tiles
        self.slides = []
        for k in range(n_slides):
            hv, ev = (H_VEC, E_VEC) if k % 2 == 0 else (H_VEC2, E_VEC2)
            t = he_tiles((tiles, size, size), seed + k, hv, ev, (1.0 + 0.2 * k, 1.0 - 0.1 * k))
            self.slides.append(np.full_like(t, 255) if k == white else t)
        self.per_iter = per_iter

    def __iter__(self):
        for k, t in enumerate(self.slides):
            chunks = [t[i:i + self.per_iter] for i in range(0, len(t), self.per_iter)]
            for ci, ch in enumerate(chunks):
                yield {"Data": torch.from_numpy(ch), "Label": torch.tensor([k % 2]), "Is Last Batch": ci == len(chunks) - 1, "Slide Filename": f"he_{k}"}


def _runner(dev, img=64, batch=4):
    from gipvit import models as M
    from gipvit.engine import FeatureExtractor
    fx = FeatureExtractor("vit_tiny", img, batch, 0, device=dev)
    fx.load_state(M.init_vit_state("vit_tiny", img, 0, seed=0))
    return fx


def test_validate_extracts_normalised_features(dev, tmp_path, caplog):
    from gipvit import ops, stainnorm as SN
    from gipvit.validate import validate
    fx = _runner(dev)
    loader = HeSlides(3, 7, 64, 3, white=1)                      # chunks of 3, 3, 1: smaller than a slide
    est = SN.MacenkoEstimator(dev, max_tiles=2)
    records = []

    class Spy(SN.SlideNormaliser):
        def begin(self, data, first, name=""):
            st = super().begin(data, first, name)
            records.append((bool(first), SN.pack_record(st.record).numpy().tobytes()))
            return st
    norm = Spy(fx, est)
    with caplog.at_level("WARNING"):
        m = validate(fx, loader, extract_features=True, out_dir=str(tmp_path), normaliser=norm)
    assert m["slides"] == 3.0 and fx._stain is None                                  # the record is taken off at the end
    assert [f for f, _ in records] == [True, False, False] * 3
    assert all(records[i][1] == records[3 * (i // 3)][1] for i in range(9))          # the record changes at slide boundaries only
    assert len({records[0][1], records[3][1], records[6][1]}) == 3
    assert norm.fallbacks == {SN.FEW_TISSUE: 1} and len([x for x in caplog.messages if "he_1" in x and SN.FEW_TISSUE in x]) == 1
    for k, t in enumerate(loader.slides):
        t_dev = torch.from_numpy(t).to(dev)
        st = est.fit(t_dev[:3])                                                      # the first chunk's first 2 tiles (max_tiles)
        assert st.on == (k != 1)
        want = fx.run(ops.stain_apply(t_dev, SN.pack_record(st.record).repeat(7).to(dev)))[0].cpu()
        assert torch.equal(torch.load(tmp_path / f"he_{k}_features.pt", weights_only=True), want)
        s = torch.load(tmp_path / f"he_{k}_stain.pt", weights_only=True)
        assert set(s) == {"HE", "maxC", "n_tissue", "on", "reason"} and s["on"] == st.on and s["n_tissue"] == st.n_tissue
        assert s["reason"] == ("" if st.on else SN.FEW_TISSUE)
        if st.on:
            assert np.array_equal(s["HE"].numpy(), st.HE) and np.array_equal(s["maxC"].numpy(), st.maxC)
    # without a normaliser: the features of the raw tiles, and no stain file
    plain = tmp_path / "plain"
    validate(fx, loader, extract_features=True, out_dir=str(plain))
    assert sorted(os.listdir(plain)) == [f"he_{k}_features.pt" for k in range(3)]
    assert torch.equal(torch.load(plain / "he_0_features.pt", weights_only=True), fx.run(torch.from_numpy(loader.slides[0]).to(dev))[0].cpu())
    assert torch.equal(torch.load(plain / "he_1_features.pt", weights_only=True), torch.load(tmp_path / "he_1_features.pt", weights_only=True))


def test_knn_monitor_builds_its_bank_through_the_normaliser(dev):
    from gipvit import ops, stainnorm as SN
    from gipvit.knn import KnnMonitor
    fx = _runner(dev, img=48)                                    # 64-px tiles: the runner sees the centred 48-px window
    est = SN.MacenkoEstimator(dev)
    loader = HeSlides(4, 5, 64, 2, white=2)
    mon = KnnMonitor(fx, k=3, num_classes=2, normaliser=SN.SlideNormaliser(fx, est))
    assert mon.build_bank(loader) == 20 and fx._stain is None
    rows = []
    for k, t in enumerate(loader.slides):
        win = torch.from_numpy(t[:, 8:56, 8:56]).contiguous().to(dev)
        st = est.fit(win[:2])                                                        # the first chunk, cut to the window
        assert st.on == (k != 2)
        f = fx.run(ops.stain_apply(win, SN.pack_record(st.record).repeat(5).to(dev)))[0]
        rows.append(torch.nn.functional.normalize(f.double(), dim=1))
    assert float((mon.bank.double() - torch.cat(rows)).abs().max()) <= 1e-6
    assert mon.normaliser.fallbacks == {SN.FEW_TISSUE: 1}
    m = mon.evaluate(loader)
    assert all(math.isfinite(v) for v in m.values()) and mon.normaliser.fallbacks == {SN.FEW_TISSUE: 2}
    plain = KnnMonitor(fx, k=3, num_classes=2)
    plain.build_bank(loader)
    assert not torch.equal(plain.bank, mon.bank)


# ---- 9. the driver -----------------------------------------------------------------------------------------------------------
def test_train_dino_knn_monitor_stain_normalize(dev, tmp_path, caplog):
    import csv
    sys.path.insert(0, ROOT)
    import train
    base = ["--dino", "--model", "vit_tiny", "--dataset", "synthetic", "-b", "2", "--out-dim", "1024", "--batches-per-epoch", "2", "--epochs", "1",
            "--lr", "1e-4", "--warmup-epochs", "0", "--log-interval", "1", "--output", str(tmp_path), "--seed", "3", "--knn-monitor", "--knn-k", "3"]
    with caplog.at_level("INFO"):
        assert train.main(base + ["--experiment", "norm", "--stain-normalize", "macenko", "--stain-norm-tiles", "2"]) == 0
    line = [m for m in caplog.messages if m.startswith("stain normalisation: macenko")]
    assert len(line) == 1 and "the first 2 tiles" in line[0] and "training batches are not normalised" in line[0]
    row = list(csv.DictReader(open(tmp_path / "norm" / "summary.csv")))[0]
    for n in ("eval_knn_top1", "eval_knn_auc_per_patch", "eval_knn_auc_per_slide"):
        assert math.isfinite(float(row[n])), (n, row[n])
    caplog.clear()
    with caplog.at_level("INFO"):
        assert train.main(base + ["--experiment", "plain"]) == 0
    assert not [m for m in caplog.messages if "stain normalisation" in m]
