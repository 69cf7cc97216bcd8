"""The small HBM-bound kernels (csrc/layernorm.hip, rowops.hip, optim.hip, dino_loss.hip) at the shapes where their loops take a
second trip, a ragged last trip, an odd slice count or another template arm -- tests/test_kernels_gpu.py holds each of them at one
shape that makes one pass or none.

Three kinds of assertion, nothing else:
  exact    integer data ({-1, 0, 1} or -2..2): every partial and total stays below 2^24, so an f32 sum is exact in any order,
           atomics included, and the 16-bit format holds every value -> torch.equal against an integer sum formed on the CPU.
  derived  a bound worked out from the number format or the summation depth, in a comment next to it.
  measured fp64 restatement of the operation on the CPU is the reference; the SAME operation in plain f32 torch on the CPU, on the
           test's own data, gives e32 = max |f32 - fp64|.  An f32 output may miss the reference by 4 * e32 (the kernels sum in
           another order than torch), a 16-bit output by 2^-8 * |ref| + 4 * e32 (twice the bf16 half-ulp of 2^-9 for the final
           rounding).  e32 is taken per comparison -- one output of one shape, on that shape's own data -- and is never less
           than half an f32 ulp of that comparison's largest reference value (2^-24 * max |ref|): over a handful of elements the
           measured figure can be 0 by luck.  Only single numbers (a loss, a one-element vector) are pooled over the cases of
           their test, named where it is done.  Each test's docstring records the e32 its data gives.

Every output lies in a buffer with sentinel guard elements behind it (and between rows where a stride leaves gaps); every shape
passes the entry point's own argument checks.  The pure-Python launch geometry below (caps read out of the sources as text) is
what tests/test_row_kernels_host.py holds the shape tables against on a machine without a GPU."""
import functools
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gipmed-project-self-supervised-vit_amd")


# ============================================================================ launch geometry, restated
_CAPS = {   # name: (file, regex with one group per number, the numbers today)
    "ln_fwd_grid": ("csrc/layernorm.hip", r"dim3 grid\(blocks < (\d+) \? blocks : (\d+)\)", (2048, 2048)),
    "ln_partial_blocks": ("../include/gipvit.h", r"#define GV_LN_PARTIAL_BLOCKS (\d+)", (1024,)),
    "ln_finalize_slices": ("csrc/layernorm.hip", r"ln_finalize_kernel, dim3\(\(a->C \+ 63\) / 64, 3, (\d+)\)", (32,)),
    "colsum_slices": ("csrc/layernorm.hip", r"nslice = a->rows >= (\d+) \* (\d+) \? (\d+) : \(a->rows \+ (\d+)\) / (\d+);", (64, 16, 64, 15, 16)),
    "colsum_cols": ("csrc/layernorm.hip", r"dim3 grid\(\(a->C \+ 127\) / (\d+), nslice\)", (128,)),
    "adam_grid": ("csrc/optim.hip", r"blocks > (\d+)\) blocks = (\d+);\s*hipLaunchKernelGGL\(adamw_ema_kernel,", (4096, 4096)),
    "cast_grid": ("csrc/rowops.hip", r"blocks > (\d+)\) blocks = (\d+); if \(blocks < 1\) blocks = 1;\s*hipLaunchKernelGGL\(cast_bf16_kernel,", (4096, 4096)),
    "sumsq_grid": ("csrc/rowops.hip", r"blocks > (\d+)\) blocks = (\d+); if \(blocks < 1\) blocks = 1;\s*hipLaunchKernelGGL\(sumsq_kernel,", (1024, 1024)),
    "dropout_grid": ("csrc/rowops.hip", r"blocks > (\d+)\) blocks = (\d+);\s*if \(a->x_is_f32\) hipLaunchKernelGGL\(dropout_kernel<float>,", (8192, 8192)),
    "dropout_add_grid": ("csrc/rowops.hip", r"blocks > (\d+)\) blocks = (\d+);\s*hipLaunchKernelGGL\(dropout_add_kernel,", (8192, 8192)),
    "tok_img_per_chunk": ("csrc/rowops.hip", r"constexpr int TOK_IMG_PER_CHUNK = (\d+);", (8,)),
    "small_matmul_cols": ("csrc/rowops.hip", r"const dim3 grid\(\(a->N \+ 127\) / (\d+), a->M\);", (128,)),
    "small_matmul_unroll": ("csrc/rowops.hip", r"for \(; k \+ (\d+) <= a\.K; k \+= (\d+)\)", (8, 8)),
    "row_loop_cols": ("csrc/rowops.hip", r"for \(int c = lane \* 4; c < a\.C; c \+= (\d+)\)", (256,)),
    "dino_kblock": ("csrc/dino_loss.hip", r"kblocks = \(a->K \+ 1023\) / (\d+);", (1024,)),
    "dino_bsplit": ("csrc/dino_loss.hip", r"int bsplit = \((\d+) \+ kblocks - 1\) / kblocks;", (1024,)),
    "dino_row_stats": ("csrc/dino_loss.hip", r"row_stats_kernel<DT, (\d+), (\d+)>", (256, 2)),
}


@functools.lru_cache(maxsize=None)
def cap(name):
    """The numbers of one launch rule, read from the source text.  A rule that is no longer spelled this way fails here: the launch
    was retuned, and the shape tables of this file (chosen against the old numbers) have to be looked at again."""
    rel, pattern, _ = _CAPS[name]
    path = os.path.normpath(os.path.join(PKG, rel))
    with open(path) as f:
        m = re.search(pattern, f.read())
    assert m, (f"{os.path.relpath(path, ROOT)}: the launch rule '{name}' (/{pattern}/) is no longer in the source -- revisit the shape "
               f"tables of tests/test_row_kernels_gpu.py (LN_*, ADAM_*, SUMSQ_NS, TOK_*, COLSUM_*, FINALIZE_*, DINO_CASES ...)")
    return tuple(int(x) for x in m.groups())


def cdiv(a, b):
    return (a + b - 1) // b


def grid_stride(units, per_block, grid_cap):
    """(trips of the busiest thread, units in the last trip) of a grid-stride loop: min(ceil(units / per_block), cap) workgroups"""
    blocks = max(1, min(cdiv(units, per_block), grid_cap))
    per_trip = blocks * per_block
    trips = cdiv(units, per_trip)
    return trips, units - (trips - 1) * per_trip


def ln_fwd_trips(rows):          # one wave per row, 4 rows per workgroup
    return grid_stride(rows, 4, cap("ln_fwd_grid")[0])


def ln_bwd_trips(rows):          # always GV_LN_PARTIAL_BLOCKS workgroups
    per_trip = 4 * cap("ln_partial_blocks")[0]
    trips = cdiv(rows, per_trip)
    return trips, rows - (trips - 1) * per_trip


def ln_bwd_idle_blocks(rows):    # workgroups that own no row: their partial block must be zero
    return max(0, cap("ln_partial_blocks")[0] - cdiv(rows, 4))


def adam_trips(n):               # f32x4 units
    return grid_stride(n // 4, 256, cap("adam_grid")[0])


def cast_trips(n):
    return grid_stride(n // 4, 256, cap("cast_grid")[0]) + (n % 4,)


def sumsq_pieces(n):
    """(threads that run the two-piece loop, most two-piece trips of one thread, threads that take the one-piece remainder, scalar
    tail elements) of sumsq_kernel"""
    n4 = n // 4
    blocks = max(1, min(cdiv(n4, 256), cap("sumsq_grid")[0]))
    stride = blocks * 256
    i = torch.arange(stride)
    trips = torch.clamp((n4 - stride - i + 2 * stride - 1) // (2 * stride), min=0)        # j with i + 2 j stride + stride < n4
    rem = (i + 2 * stride * trips) < n4
    return int((trips > 0).sum()), int(trips.max()), int(rem.sum()), n % 4


def dropout_trips(n, add=False):
    return grid_stride(n, 256, cap("dropout_add_grid" if add else "dropout_grid")[0])


def tok_chunks(n_img):
    per = cap("tok_img_per_chunk")[0]
    chunks = cdiv(n_img, per)
    return chunks, n_img - (chunks - 1) * per


def colsum_slices(rows):
    """(row slices, rows per slice, rows of the last non-empty slice)"""
    big, per16, n_big, _, _ = cap("colsum_slices")
    nslice = n_big if rows >= big * per16 else cdiv(rows, per16)
    per = cdiv(rows, nslice)
    full = (rows - 1) // per
    return nslice, per, rows - full * per


def ln_finalize_slices(n_blocks):
    """(partial blocks per slice, slices that hold any, blocks of the last such slice)"""
    nz = cap("ln_finalize_slices")[0]
    per = cdiv(n_blocks, nz)
    used = cdiv(n_blocks, per)
    return per, used, n_blocks - (used - 1) * per


def dino_split(B, K):
    """(k blocks, batch slices, batch rows per slice, rows of the last slice) of loss_grad_kernel"""
    kblocks = cdiv(K, cap("dino_kblock")[0])
    bsplit = max(1, min(cdiv(cap("dino_bsplit")[0], kblocks), B))
    b_per = cdiv(B, bsplit)
    bsplit = cdiv(B, b_per)
    return kblocks, bsplit, b_per, B - (bsplit - 1) * b_per


def row_stats_trips(K):
    """(trips of thread 0; in the last trip: threads whose second piece lies inside the row, threads whose first piece does and whose
    second does not) of row_stats_kernel"""
    nt, u = cap("dino_row_stats")
    assert u == 2
    span = nt * 4 * u
    trips = cdiv(K, span)
    base = (trips - 1) * span
    inside = sum(1 for t in range(nt) if base + t * 4 + nt * 4 < K)
    outside = sum(1 for t in range(nt) if base + t * 4 < K <= base + t * 4 + nt * 4)
    return trips, inside, outside


def row_loop_trips(C):           # l2norm / generic weightnorm: 64 lanes x 4 columns per trip
    per = cap("row_loop_cols")[0]
    trips = cdiv(C, per)
    return trips, C - (trips - 1) * per


# ============================================================================ shape tables (held by tests/test_row_kernels_host.py)
LN_DS = (192, 384, 768)
LN_FWD_ROWS = (8192, 8197, 16387)              # one trip exactly; five rows in a second; three rows in a third
LN_FWD_STRIDED_ROWS = 8197
LN_BWD_ROWS = (4096, 4109, 8197)               # one trip exactly; 13 rows in a second; five in a third
LN_BWD_IDLE_ROWS = 37                          # 10 workgroups own rows, 1014 must write zero partials
FINALIZE_BLOCKS = (1, 3, 5, 31, 33, 100, 1024)
FINALIZE_CS = (2, 64, 192, 384)
COLSUM_ROWS = (1, 15, 17, 36, 196, 1023, 1024, 2051)
COLSUM_CS = (2, 130, 192, 1152)
SUMSQ_NS = (3, 4, 1027, 1 << 20, (1 << 20) + 4, 2 * (1 << 20) + 4000 + 3)
CAST_N = (1 << 22) + 1200 + 2
DROPOUT_N = (1 << 21) + 1280 + 3
DROPOUT_ADD_SHAPE = (5462, 384)
TOK_IMGS = (8, 9, 21)
TOK_NS = (2, 37)
TOK_DS = (192, 384, 768)
SMM_KS = (1, 7, 8, 9, 196)
SMM_NS = (2, 128, 130)
SMM_MS = (1, 36)
NORM_CS = (4, 256, 260, 384, 768)
NORM_ROWS = (1, 5, 77)
WN256_ROWS = (1, 4, 5, 8, 9)                   # a wave with and without its second row (row r pairs with r + 4)
DINO_CASES = ((19, 2, 2, 65536), (3, 6, 4, 1028), (2, 3, 3, 2052), (2, 16, 2, 256), (2, 2, 1, 4))     # (B, V, G, K)
DINO_OPTIONS_CASE = (3, 6, 4, 1028)
DINO_INT_TEACHER_CASE = (2, 3, 3, 2052)
LSCE_CS = (1, 2, 64)
LSCE_BS = (1, 256, 257)
ADAM_N = 8192
ADAM_TRIP_N = (1 << 22) + 3108                 # 777 f32x4 units take a second trip
CENTER_KS = (1, 255, 257)

GUARD = 64
SENT = 12345.0                                 # guard fill (exact in f32; the 16-bit guards are compared with their own rounding)


# ============================================================================ helpers
def ops():
    from gipvit import ops as o
    return o


def L():
    from gipvit import _lib
    return _lib


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rint(shape, lo, hi, seed, dtype=f32):
    """integers lo..hi (inclusive) on the CPU"""
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).to(dtype)


def guarded(dev, n, dtype=f32, fill=SENT):
    """(flat buffer of n + GUARD sentinels, its first n elements)"""
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[:n]


def guard_ok(buf, n, what, fill=SENT):
    assert torch.equal(buf[n:], torch.full_like(buf[n:], fill)), f"{what}: guard elements behind the output were written"


def put(dev, t, dtype=None, fill=SENT):
    """a CPU tensor copied into a guarded device buffer -> (buffer, view of its shape)"""
    dtype = t.dtype if dtype is None else dtype
    buf, v = guarded(dev, t.numel(), dtype, fill)
    v.copy_(t.reshape(-1).to(dtype))
    return buf, v.view(t.shape)


class Measured:
    """The 'measured' rule of the file header.  add() collects one comparison; check() forms e32 per comparison (per `pool` where one
    is given: single numbers of several cases), prints the figures and asserts."""

    def __init__(self):
        self.items = []

    def add(self, name, got, ref64, plain32, sixteen=False, what="", pool=None):
        self.items.append((name, got.detach().double().cpu().reshape(-1), ref64.detach().double().reshape(-1),
                           plain32.detach().double().reshape(-1), sixteen, what, pool if pool is not None else (name, what, len(self.items))))

    def check(self):
        e32, top = {}, {}
        for _, _, ref, plain, _, _, key in self.items:
            e32[key] = max(e32.get(key, 0.0), float((plain - ref).abs().max()))
            top[key] = max(top.get(key, 0.0), float(ref.abs().max()))
        fails = []
        for name, got, ref, _, sixteen, what, key in self.items:
            e = max(e32[key], 2.0 ** -24 * top[key])
            bound = torch.full_like(ref, 4.0 * e) + (2.0 ** -8 * ref.abs() if sixteen else 0.0)
            err = (got - ref).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            print(f"[measured] {name} {what}: e32 {e32[key]:.3e} (floor {2.0 ** -24 * top[key]:.3e}) kernel max err {float(err.max()):.3e} "
                  f"worst err / bound {ratio:.3f}{' (16-bit rule)' if sixteen else ''}")
            if not bool((err <= bound).all()) or not bool(torch.isfinite(got).all()):
                fails.append(f"{name} {what}: {int((err > bound).sum())}/{err.numel()} off, max err {float(err.max()):.4g}, e32 {e32[key]:.4g}, worst err / bound {ratio:.3g}")
        assert not fails, "; ".join(fails)


def r32(x):
    """a Python float rounded to f32 (what an entry point receives for a by-value float)"""
    return float(torch.tensor(x, dtype=f32))


# ============================================================================ 1. LayerNorm forward
EPS = r32(1e-6)
CONST_X = 0.75        # the constant row: sum and mean are exact in f32 (0.75 D and 0.75), so variance 0, rstd = eps^-1/2, y = beta


@functools.lru_cache(maxsize=2)
def _ln_fwd_case(D, rows, stride):
    g = gen(D * 100003 + rows + stride)
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    crow = min(rows - 1, 4 * cap("ln_fwd_grid")[0] + 2)     # a row of the second trip where there is one
    x[crow] = CONST_X
    gamma = 1 + 0.1 * torch.randn(D, generator=g); beta = 0.1 * torch.randn(D, generator=g)
    F = torch.nn.functional
    x64 = x.double()
    ref = dict(y=F.layer_norm(x64, (D,), gamma.double(), beta.double(), EPS), mean=x64.mean(-1),
               rstd=1.0 / torch.sqrt(x64.var(-1, unbiased=False) + EPS))
    plain = dict(y=F.layer_norm(x, (D,), gamma, beta, EPS), mean=x.mean(-1), rstd=1.0 / torch.sqrt(x.var(-1, unbiased=False) + EPS))
    assert torch.equal(ref["y"][crow], beta.double()) and abs(float(ref["rstd"][crow]) - EPS ** -0.5) < 1e-9
    return x, gamma, beta, crow, ref, plain


def _ln_fwd(dev, D, rows, dt, stride):
    x, gamma, beta, crow, ref, plain = _ln_fwd_case(D, rows, stride)
    xs = torch.full((rows, stride), 3.0e4)                  # the gap columns of a strided input must not be read
    xs[:, :D] = x
    ybuf, y = guarded(dev, rows * D, dt); mbuf, mean = guarded(dev, rows); rbuf, rstd = guarded(dev, rows)
    ops().layernorm_fwd(xs.to(dev), gamma.to(dev), beta.to(dev), rows, D, x_stride=stride, eps=EPS, y=y.view(rows, D), mean=mean, rstd=rstd)
    torch.cuda.synchronize()
    guard_ok(ybuf, rows * D, "y"); guard_ok(mbuf, rows, "mean"); guard_ok(rbuf, rows, "rstd")
    ordinary = torch.arange(rows) != crow
    m = Measured()
    m.add("y", y.view(rows, D), ref["y"], plain["y"], sixteen=dt != f32)
    m.add("mean", mean, ref["mean"], plain["mean"])
    m.add("rstd", rstd.cpu()[ordinary], ref["rstd"][ordinary], plain["rstd"][ordinary])
    m.add("rstd(constant row)", rstd.cpu()[crow:crow + 1], ref["rstd"][crow:crow + 1], plain["rstd"][crow:crow + 1])
    m.check()


@pytest.mark.parametrize("dt", [bf16, f32], ids=["16bit", "f32"])
@pytest.mark.parametrize("rows", LN_FWD_ROWS)
@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_fwd_trips(dev, D, rows, dt):
    """ln_fwd_kernel beyond its 2048-workgroup grid: the prefetched row (nv -> v, row = nrow) at 8197 rows (second trip of five rows)
    and 16 387 rows (third trip of three), 8192 rows as the single-trip control; y, mean AND rstd against fp64, one row of the
    second trip constant (variance 0: rstd = eps^-1/2 = 1000, y = beta).
    e32 on this data (plain f32 torch on the CPU against fp64, the largest over the D and row counts): y 1.2e-6, mean 1.3e-7,
    rstd 7.2e-8; the constant row's rstd 6.2e-5 (one f32 ulp of 1000 is 6.1e-5), compared on its own so that it does not widen the
    bound of the ordinary rows."""
    _ln_fwd(dev, D, rows, dt, D)


@pytest.mark.parametrize("dt", [bf16, f32], ids=["16bit", "f32"])
@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_fwd_trips_strided(dev, D, dt):
    """The same at x_stride = 2 D and 8197 rows: the prefetch addresses the NEXT trip's row through the stride; the gap columns hold
    3e4 and must not enter any row.  e32 as test_layernorm_fwd_trips."""
    _ln_fwd(dev, D, LN_FWD_STRIDED_ROWS, dt, 2 * D)


# ============================================================================ 2. LayerNorm backward
@functools.lru_cache(maxsize=2)
def _ln_bwd_case(D, rows):
    g = gen(D * 7919 + rows)
    F = torch.nn.functional
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g).to(bf16).float()          # representable in both element types
    g0 = torch.randn(rows, D, generator=g)
    gs = 0.5 + torch.rand(rows, generator=g)
    out = {}
    for name, dt in (("ref", f64), ("plain", f32)):
        xr = x.to(dt).clone().requires_grad_(True); gr = gamma.to(dt).clone().requires_grad_(True); br = torch.zeros(D, dtype=dt, requires_grad=True)
        F.layer_norm(xr, (D,), gr, br, EPS).backward(dy.to(dt))
        out[name] = dict(dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)
    x64 = x.double()
    mean = x64.mean(-1).float(); rstd = (1.0 / torch.sqrt(x64.var(-1, unbiased=False) + EPS)).float()      # inputs of the backward
    return x, gamma, dy, g0, gs, mean, rstd, out["ref"], out["plain"]


# (rows, g_init, gb given, gb_scale given, g / gb row stride - D)
LN_BWD_VARIANTS = ((4096, True, True, False, 0), (4109, False, False, False, 0), (4109, True, True, False, 4), (8197, False, True, True, 0),
                   (8197, True, False, False, 0), (LN_BWD_IDLE_ROWS, False, True, True, 4))


@pytest.mark.parametrize("dt", [bf16, f32], ids=["16bit", "f32"])
@pytest.mark.parametrize("rows,g_init,with_gb,with_scale,gap", LN_BWD_VARIANTS)
@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_bwd_trips(dev, D, rows, g_init, with_gb, with_scale, gap, dt):
    """ln_bwd_kernel past one trip of its 1024 workgroups (4096 rows): 4109 rows (13 in a second trip) and 8197 (five in a third)
    carry s_dg / s_db / s_g in registers across the rows of one wave; 4096 is the one-trip control and 37 rows leave 1014 workgroups
    without a row (their partial blocks must be exactly zero).  g_init 0 / 1, gb given / None, gb_scale once per row count, a
    g / gb row stride of D + 4 with sentinel gaps.  The partials are reduced by colsum_finalize AND ln_finalize.
    e32 on this data (f32 autograd of F.layer_norm on the CPU against fp64, the largest over the D and variants): dx 6.2e-7, gb
    7.6e-7, dgamma 1.8e-4, dbeta 3.1e-5, column sum of g 5.7e-5 (sums of up to 8197 terms of size ~1)."""
    o = ops()
    x, gamma, dy, g0, gs, mean, rstd, ref, plain = _ln_bwd_case(D, rows)
    ld = D + gap
    gs_ = gs if with_scale else torch.ones(rows)
    g_in = torch.full((rows, ld), SENT); g_in[:, :D] = g0
    gbuf, gv = put(dev, g_in)
    gbbuf, gb = guarded(dev, rows * ld, dt)
    pbuf, part = guarded(dev, L().LN_PARTIAL_BLOCKS * 3 * D)
    part = part.view(L().LN_PARTIAL_BLOCKS, 3, D)
    o.layernorm_bwd(dy.to(dev).to(dt), x.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), gv, gb.view(rows, ld) if with_gb else None,
                    part, rows, D, g_stride=ld, gb_stride=ld, g_init=g_init, gb_scale=gs.to(dev) if with_scale else None)
    outs_buf = [guarded(dev, D) for _ in range(3)]
    for w in range(3):
        o.colsum_finalize(part, L().LN_PARTIAL_BLOCKS, 3, w, D, outs_buf[w][1], False)
    fin = [torch.ones(D, device=dev) for _ in range(3)]
    o.ln_finalize(part, L().LN_PARTIAL_BLOCKS, D, fin[0], fin[1], fin[2])
    torch.cuda.synchronize()
    guard_ok(gbuf, rows * ld, "g"); guard_ok(pbuf, part.numel(), "partials")
    for w in range(3):
        guard_ok(outs_buf[w][0], D, f"colsum_finalize {w}")
    gv_c, gb_c = gv.cpu(), gb.view(rows, ld).cpu()
    assert torch.equal(gv_c[:, D:], torch.full((rows, gap), SENT)), "g: the gap between rows was written"
    untouched = gb_c[:, D:] if with_gb else gb_c
    assert torch.equal(untouched, torch.full_like(untouched, SENT)), "gb: written outside its rows (or written at all without gb)"
    guard_ok(gbbuf, rows * ld, "gb")
    idle = ln_bwd_idle_blocks(rows)
    if idle:
        assert float(part[-idle:].abs().max()) == 0.0, "partial blocks of workgroups without a row are not zero"
    base = 0.0 if g_init else 1.0
    m = Measured()
    gnew = {k: base * g0.to(d) + r["dx"] for k, r, d in (("ref", ref, f64), ("plain", plain, f32))}
    m.add("dx", gv_c[:, :D], gnew["ref"], gnew["plain"])
    if with_gb:
        m.add("gb", gb_c[:, :D], gnew["ref"] * gs_[:, None].double(), gnew["plain"] * gs_[:, None], sixteen=dt != f32)
    cs = {k: (gnew[k] * gs_[:, None].to(gnew[k].dtype)).sum(0) for k in gnew}
    for name, w, r, p in (("dgamma", 0, ref["dgamma"], plain["dgamma"]), ("dbeta", 1, ref["dbeta"], plain["dbeta"]), ("colsum g", 2, cs["ref"], cs["plain"])):
        m.add(name, outs_buf[w][1], r, p, what="colsum_finalize")
        m.add(name, fin[w], 1.0 + r, 1.0 + p, what="ln_finalize (+1)")
    m.check()


# ============================================================================ 3. finalizers, exact
@pytest.mark.parametrize("n_blocks", FINALIZE_BLOCKS)
def test_finalizers_exact(dev, n_blocks):
    """colsum_finalize (pairs b, b + 4 with an odd tail, 4 row groups) and ln_finalize (32 slices of ceil(n_blocks / 32): empty slices
    below 32 blocks, a ragged last slice at 33 and 100) on integer partials [n_blocks, 3, C]: torch.equal against the CPU sum.
    accumulate 0 / 1 for each `which`; ln_finalize adds into prefilled outputs and leaves a None output's neighbour alone."""
    o = ops()
    for C in FINALIZE_CS:
        p = rint((n_blocks, 3, C), -1, 1, seed=n_blocks * 1000 + C)
        pbuf, pd = put(dev, p)
        want = p.sum(0)
        for which in range(3):
            for acc in (False, True):
                obuf, out = guarded(dev, C)
                out.fill_(5.0)
                o.colsum_finalize(pd, n_blocks, 3, which, C, out, acc)
                assert torch.equal(out.cpu(), want[which] + (5.0 if acc else 0.0)), (C, which, acc)
                guard_ok(obuf, C, f"colsum_finalize C={C}")
        for skip in range(3):
            bufs = [guarded(dev, C) for _ in range(3)]
            for w in range(3):
                bufs[w][1].fill_(float(w + 2))
            args = [None if w == skip else bufs[w][1] for w in range(3)]
            o.ln_finalize(pd, n_blocks, C, *args)
            for w in range(3):
                assert torch.equal(bufs[w][1].cpu(), torch.full((C,), float(w + 2)) + (0.0 if w == skip else 1.0) * want[w]), (C, skip, w)
                guard_ok(bufs[w][0], C, f"ln_finalize C={C}")


# ============================================================================ 4. colsum, exact
@pytest.mark.parametrize("dt", [bf16, f32], ids=["16bit", "f32"])
@pytest.mark.parametrize("rows", COLSUM_ROWS)
def test_colsum_exact(dev, rows, dt):
    """gv_colsum on {-1, 0, 1}: the slice rule below 1024 rows (1, 15 rows: one slice; 17: two; 36: 3 and 196: 13 slices as the
    engine calls it, both odd for the finalize's pair loop; 1023: 64 slices of 16 with a 15-row last one) and at / above it (1024,
    2051: 64 slices, 33 rows each with a 5-row last one), C = 2 / 130 / 192 (a partly filled 128-column workgroup), ld = C and
    C + 6 with 4096 in the gap columns, accumulate 0 / 1.  torch.equal against the CPU column sums."""
    o = ops()
    for C in COLSUM_CS:
        for ld in (C, C + 6):
            x = torch.full((rows, ld), 4096.0)
            x[:, :C] = rint((rows, C), -1, 1, seed=rows * 10000 + C)
            want = x[:, :C].sum(0)
            _, xd = put(dev, x, dt)
            ws = torch.full((64 * C + GUARD,), SENT, device=dev)
            for acc in (False, True):
                obuf, out = guarded(dev, C)
                out.fill_(3.0)
                o.colsum(xd, rows, C, ws, out, accumulate=acc, ld=ld)
                assert torch.equal(out.cpu(), want + (3.0 if acc else 0.0)), (C, ld, acc)
                guard_ok(obuf, C, f"colsum C={C} ld={ld}")
            assert torch.equal(ws[colsum_slices(rows)[0] * C:], torch.full_like(ws[colsum_slices(rows)[0] * C:], SENT)), "workspace written past nslice * C"


# ============================================================================ 5. sumsq
@pytest.mark.parametrize("n", SUMSQ_NS)
def test_sumsq_exact(dev, n):
    """gv_sumsq on {-1, 0, 1} (the sum is a count below 2^24: exact): n = 3 (scalar tail only), 4, 1027, 2^20 (n4 = 262 144 = one
    grid of threads: the two-piece loop still idle), 2^20 + 4 (one thread takes it) and 2 x 2^20 + 4003 (every thread one full
    two-piece trip, 1000 threads the remainder piece, three tail elements).  accumulate onto a prefilled integer."""
    o = ops()
    x = rint((n,), -1, 1, seed=n)
    want = float((x != 0).sum())
    _, xd = put(dev, x)
    ws = torch.full((1024,), float("nan"), device=dev)
    obuf, out = guarded(dev, 1)
    o.sumsq(xd, ws, out, n=n)
    assert float(out) == want, (float(out), want)
    out.fill_(41.0)
    o.sumsq(xd, ws.fill_(float("nan")), out, accumulate=True, n=n)
    assert float(out) == want + 41.0
    guard_ok(obuf, 1, "sumsq out")


def test_sumsq_randn_and_nonfinite(dev):
    """randn at the largest n against the fp64 sum: relative 1e-5.  Derived: at most 64 additions lie between a term and the result
    (a thread's 2 trips x 8 terms, 6 wave steps, 4 waves, then sumsq_final's 4 terms, 6 steps, 4 waves), the terms are >= 0, so
    |err| <= 64 * 2^-24 * sum < 4e-6 * sum.  An inf or a NaN in the LAST scalar-tail element must make the result non-finite
    (the clip and the loss scaler's finite check read this value)."""
    o = ops()
    n = SUMSQ_NS[-1]
    x = torch.randn(n, generator=gen(77))
    ref = float((x.double() ** 2).sum())
    _, xd = put(dev, x)
    ws = torch.full((1024,), float("nan"), device=dev); out = torch.empty(1, device=dev)
    o.sumsq(xd, ws, out, n=n)
    print(f"[derived] sumsq randn: rel err {abs(float(out) - ref) / ref:.3e} (bound 1e-5)")
    assert abs(float(out) - ref) <= 1e-5 * ref, (float(out), ref)
    for bad in (float("inf"), float("nan")):
        xd[n - 1] = bad
        o.sumsq(xd, ws.fill_(float("nan")), out, n=n)
        assert not math.isfinite(float(out)), bad


# ============================================================================ 6. cast
def test_cast_bf16_second_trip(dev):
    """cast_bf16_kernel past its 4096-workgroup grid: 2^22 + 1202 elements = 300 f32x4 units in a second trip and a 2-element tail."""
    n = CAST_N
    src = torch.randn(n, generator=gen(6))
    _, sd = put(dev, src)
    dbuf, dst = guarded(dev, n, bf16)
    ops().cast_bf16(sd, dst, n)
    assert torch.equal(dst.cpu(), src.to(bf16))
    guard_ok(dbuf, n, "cast dst")


# ============================================================================ 7. dropout
@pytest.mark.parametrize("dt", [bf16, f32], ids=["16bit", "f32"])
def test_dropout_second_trip(dev, dt):
    """dropout_kernel past its 8192-workgroup grid (2 097 152 elements): 1283 elements in a second trip.  Mask bit-identical to the
    oracle's counter-based restatement; integer data and p = 0.5 (scale 2) keep the kept values exact in both element types."""
    from oracle import vit_oracle as vo
    n = DROPOUT_N
    x = rint((n,), -2, 2, seed=8)
    xbuf, xd = put(dev, x, dt)
    ops().dropout(xd, 0xC0FFEE, 0.5, n=n)
    assert torch.equal(xd.float().cpu(), x * vo.dropout_mask(0xC0FFEE, 0, n, 0.5))
    guard_ok(xbuf, n, "dropout x")


@pytest.mark.parametrize("with_scale", [False, True])
def test_dropout_add_second_trip(dev, with_scale):
    """dropout_add_kernel at 5462 x 384 = 2 097 408 elements: 256 in a second trip (rows 5461 and up).  Integer t / resid, p = 0.5 and
    row scales from {0.5, 1, 2}: exact whatever the compiler contracts."""
    from oracle import vit_oracle as vo
    rows, cols = DROPOUT_ADD_SHAPE
    t = rint((rows, cols), -2, 2, seed=9); resid = rint((rows, cols), -2, 2, seed=10)
    rs = torch.tensor([0.5, 1.0, 2.0])[rint((rows,), 0, 2, seed=11, dtype=torch.long)]
    obuf, out = guarded(dev, rows * cols)
    ops().dropout_add(t.to(dev), resid.to(dev), out.view(rows, cols), rows, cols, 4242, 0.5, row_scale=rs.to(dev) if with_scale else None)
    mask = vo.dropout_mask(4242, 0, rows * cols, 0.5).view(rows, cols)
    want = resid + (rs[:, None] if with_scale else 1.0) * (t * mask)
    assert torch.equal(out.view(rows, cols).cpu(), want)
    guard_ok(obuf, rows * cols, "dropout_add out")


# ============================================================================ 8. tokens_bwd, exact
@pytest.mark.parametrize("D", TOK_DS)
@pytest.mark.parametrize("n_img", TOK_IMGS)
def test_tokens_bwd_exact(dev, n_img, D):
    """tokens_bwd_kernel on integers -2..2: 8 images (one full chunk), 9 (a one-image second chunk), 21 (three chunks, five images in
    the last) meet in dpos / dcls through atomics; D = 192 (64 idle threads), 384, 768 (three column blocks); N = 2 and 37; patch
    rows 16-bit and f32; accumulate=False into sentinel-filled dpos / dcls (the memset path), accumulate=True onto prefilled
    integers, dcls = None (what the engine passes).  Everything torch.equal."""
    o = ops()
    for N in TOK_NS:
        g = rint((n_img, N, D), -2, 2, seed=n_img * 100 + N + D)
        gd = g.to(dev)
        for dt in (bf16, f32):
            for acc, with_cls in ((False, True), (True, True), (False, False), (True, False)):
                pbuf, gp = guarded(dev, n_img * (N - 1) * D, dt)
                dbuf, dpos = guarded(dev, N * D); cbuf, dcls = guarded(dev, D)
                if acc:
                    dpos.fill_(3.0); dcls.fill_(-2.0)
                o.tokens_bwd(gd, gp, dpos, dcls if with_cls else None, n_img, N, D, accumulate=acc)
                tag = (N, dt, acc, with_cls)
                assert torch.equal(dpos.view(N, D).cpu(), g.sum(0) + (3.0 if acc else 0.0)), tag
                if with_cls:
                    assert torch.equal(dcls.cpu(), g[:, 0].sum(0) + (-2.0 if acc else 0.0)), tag
                else:
                    assert torch.equal(dcls.cpu(), torch.full((D,), -2.0 if acc else SENT)), tag
                assert torch.equal(gp.view(n_img, N - 1, D).float().cpu(), g[:, 1:]), tag
                guard_ok(pbuf, gp.numel(), "gpatch"); guard_ok(dbuf, N * D, "dpos"); guard_ok(cbuf, D, "dcls")


# ============================================================================ 9. cls_rows / gather_cls
@pytest.mark.parametrize("D", TOK_DS)
def test_cls_rows_gather_cls(dev, D):
    """The 256-thread column loops at D = 192 (idle threads), 384 and 768 (three trips).  cls + pos is one f32 addition and the
    gather one rounding: both torch.equal; every row but row 0 of each image keeps its sentinel."""
    o = ops()
    n_img, N = 3, 5
    g = gen(D)
    cls = torch.randn(D, generator=g); pos = torch.randn(N, D, generator=g)
    xbuf, x = guarded(dev, n_img * N * D)
    o.cls_rows(x, cls.to(dev), pos.to(dev), n_img, N, D)
    xv = x.view(n_img, N, D).cpu()
    assert torch.equal(xv[:, 0], (cls + pos[0]).expand(n_img, D))
    assert torch.equal(xv[:, 1:], torch.full((n_img, N - 1, D), SENT))
    guard_ok(xbuf, n_img * N * D, "cls_rows x")
    src = torch.randn(n_img, N, D, generator=g)
    ybuf, y = guarded(dev, n_img * D, bf16)
    o.gather_cls(src.to(dev), y, n_img, N, D)
    assert torch.equal(y.view(n_img, D).cpu(), src[:, 0].to(bf16))
    guard_ok(ybuf, n_img * D, "gather_cls y")


# ============================================================================ 10. small_matmul, exact
@pytest.mark.parametrize("bt", [bf16, f32], ids=["B16", "B32"])
@pytest.mark.parametrize("at", [bf16, f32], ids=["A16", "A32"])
def test_small_matmul_exact(dev, at, bt):
    """All four A / B element-type instantiations on {-1, 0, 1} with an integer bias: K = 1, 7 (tail only), 8 (one unrolled trip),
    9, 196; N = 2, 128, 130 (a second workgroup with two live threads); M = 1, 36; C in f32 and in the 16-bit format with accumulate
    (|C| <= 196 + 4: exact in 8 significant bits); ldc = N + 6 with guard columns; the transposed form (sam = 1, sak = M) and the
    engine's broadcast form (sam = sak = sbk = 0, a one-element A)."""
    o = ops()
    for K in SMM_KS:
        for N in SMM_NS:
            for M in SMM_MS:
                seed = K * 10007 + N * 101 + M
                A = rint((M, K), -1, 1, seed); B = rint((K, N), -1, 1, seed + 1); bias = rint((N,), -2, 2, seed + 2); C0 = rint((M, N), -2, 2, seed + 3)
                Ad, Bd, bd = A.to(dev).to(at), B.to(dev).to(bt), bias.to(dev)
                AdT = A.t().contiguous().to(dev).to(at)                 # stored [K, M]
                ldc = N + 6
                for ct in (f32, bf16):
                    for form in ("plain", "transposed"):
                        cbuf, c = guarded(dev, M * ldc, ct)
                        cv = c.view(M, ldc)
                        cv[:, :N] = C0.to(dev).to(ct)
                        if form == "plain":
                            o.small_matmul(Ad, Bd, cv, M, N, K, sam=K, sak=1, sbk=N, sbn=1, ldc=ldc, bias=bd, accumulate=True)
                        else:
                            o.small_matmul(AdT, Bd, cv, M, N, K, sam=1, sak=M, sbk=N, sbn=1, ldc=ldc, bias=bd, accumulate=True)
                        got = cv.float().cpu()
                        assert torch.equal(got[:, :N], C0 + A @ B + bias), (K, N, M, ct, form)
                        assert torch.equal(got[:, N:], torch.full((M, 6), float(torch.tensor(SENT, dtype=ct)))), "guard columns written"
                        guard_ok(cbuf, M * ldc, "small_matmul C", float(torch.tensor(SENT, dtype=ct)))
                # broadcast: C[m, n] = K * a0 * B[n] + bias[n], overwrite
                a0 = torch.tensor([-1.0]).to(dev).to(at)
                cbuf, c = guarded(dev, M * N)
                o.small_matmul(a0, Bd, c.view(M, N), M, N, K, sam=0, sak=0, sbk=0, sbn=1, bias=bd)
                assert torch.equal(c.view(M, N).cpu(), (-float(K) * B[0] + bias).expand(M, N)), (K, N, M, "broadcast")
                guard_ok(cbuf, M * N, "small_matmul C (broadcast)")


# ============================================================================ 11. l2norm / weightnorm
@pytest.mark.parametrize("dt", [bf16, f32], ids=["16bit", "f32"])
def test_l2norm_weightnorm_fp64(dev, dt):
    """l2norm_* and the generic weightnorm_* at C = 4 (one live lane), 256, 260 (a second column trip with one live lane), 384 and 768
    (two and three trips: what gipvit/knn.py normalises), rows 1 / 5 / 77, outputs 16-bit and f32; the two-rows-per-wave C = 256
    weightnorm kernels at 1, 4, 5, 8 and 9 rows (a wave with and without its second row), accumulate 0 / 1.  A zero row for l2norm:
    y = 0, inv_norm = 1 / 1e-12f, dx finite.  Everything against fp64; the backward kernels get the rounded fp64 forward as input.
    e32 over the whole test (plain f32 torch on the CPU): l2norm y 1.0e-7, inv_norm 2.9e-7 (floor 3.7e-7: half an ulp of the
    largest, 6.1 at C = 4), dx 4.8e-7 (floor 5.2e-7); weightnorm w 9.8e-8, dv 5.1e-7 (floor 5.8e-7), dg 7.6e-7."""
    o = ops()
    m = Measured()
    F = torch.nn.functional
    for C in NORM_CS:
        for rows in sorted(set(NORM_ROWS + (WN256_ROWS if C == 256 else ()))):
            g = gen(C * 1000 + rows)
            tag = f"{rows}x{C}"
            # ---- l2norm (the last row is zero where there is more than one)
            x = torch.randn(rows, C, generator=g)
            zero = rows > 1
            if zero:
                x[-1] = 0.0
            live = slice(0, rows - 1 if zero else rows)
            ybuf, y = guarded(dev, rows * C, dt); ibuf, inv = guarded(dev, rows)
            o.l2norm_fwd(x.to(dev), y.view(rows, C), inv, rows, C)
            ref_y = F.normalize(x.double(), dim=-1); ref_inv = 1.0 / x.double().norm(dim=-1).clamp_min(1e-12)
            m.add("l2norm y", y.view(rows, C).cpu()[live], ref_y[live], F.normalize(x, dim=-1)[live], sixteen=dt != f32, what=tag)
            m.add("l2norm inv_norm", inv.cpu()[live], ref_inv[live], (1.0 / x.norm(dim=-1))[live], what=tag)
            if zero:
                assert float(y.view(rows, C)[-1].float().abs().max()) == 0.0
                # 1e-12f and one division, each rounded once: within 2^-23 of 1e12, asserted at 2^-22
                assert abs(float(inv[-1]) - 1e12) <= 1e12 * 2.0 ** -22, float(inv[-1])
            guard_ok(ybuf, rows * C, "l2norm y"); guard_ok(ibuf, rows, "inv_norm")
            dy = torch.randn(rows, C, generator=g)
            y_in = ref_y.to(dt); inv_in = ref_inv.float()
            dxbuf, dx = guarded(dev, rows * C, dt)
            o.l2norm_bwd(dy.to(dev), y_in.to(dev), inv_in.to(dev), dx.view(rows, C), rows, C)

            def l2b(d, yy, iv):
                return (d - yy * (d * yy).sum(-1, keepdim=True)) * iv[:, None]
            m.add("l2norm dx", dx.view(rows, C).cpu()[live], l2b(dy.double(), y_in.double(), inv_in.double())[live],
                  l2b(dy, y_in.float(), inv_in)[live], sixteen=dt != f32, what=tag)
            assert bool(torch.isfinite(dx.float()).all()), "l2norm_bwd: non-finite dx (zero row)"
            guard_ok(dxbuf, rows * C, "l2norm dx")
            # ---- weightnorm
            v = torch.randn(rows, C, generator=g); gg = 1 + 0.1 * torch.randn(rows, generator=g); dw = torch.randn(rows, C, generator=g)
            wbuf, w = guarded(dev, rows * C, dt)
            o.weightnorm_fwd(v.to(dev), gg.to(dev), w.view(rows, C), rows, C)

            def wn(vv, g_):
                return g_[:, None] * vv / vv.norm(dim=1, keepdim=True)
            m.add("weightnorm w", w.view(rows, C), wn(v.double(), gg.double()), wn(v, gg), sixteen=dt != f32, what=tag)
            guard_ok(wbuf, rows * C, "weightnorm w")
            if dt == f32:           # the backward has one form (f32 throughout): run it once
                grads = {}
                for name, d in (("ref", f64), ("plain", f32)):
                    vr = v.to(d).clone().requires_grad_(True); gr = gg.to(d).clone().requires_grad_(True)
                    wn(vr, gr).backward(dw.to(d))
                    grads[name] = (vr.grad, gr.grad)
                for acc in (False, True):
                    vbuf, dv = guarded(dev, rows * C); gbuf, dg = guarded(dev, rows)
                    dv.fill_(7.0); dg.fill_(7.0)
                    o.weightnorm_bwd(dw.to(dev), v.to(dev), gg.to(dev), dv.view(rows, C), dg, rows, C, accumulate=acc)
                    b = 7.0 if acc else 0.0
                    m.add("weightnorm dv", dv.view(rows, C), b + grads["ref"][0], b + grads["plain"][0], what=f"{tag} acc={acc}")
                    m.add("weightnorm dg", dg, b + grads["ref"][1], b + grads["plain"][1], what=f"{tag} acc={acc}")
                    guard_ok(vbuf, rows * C, "dv"); guard_ok(gbuf, rows, "dg")
    m.check()


# ============================================================================ 12. DINO loss
TS, TT = r32(0.1), r32(0.04)


@functools.lru_cache(maxsize=2)
def _dino_case(B, V, G, K, int_teacher=False):
    from oracle import vit_oracle as vo
    g = gen(B * 1000003 + V * 1009 + G * 101 + K)
    s = torch.randn(V * B, K, generator=g)
    t = rint((G * B, K), -2, 2, seed=K + B) if int_teacher else torch.randn(G * B, K, generator=g)
    center = 0.1 * torch.randn(1, K, generator=g)
    out = {}
    for name, d in (("ref", f64), ("plain", f32)):
        sr = s.to(d).clone().requires_grad_(True)
        loss, csum = vo.dino_loss(sr, t.to(d), center.to(d), V, G, TS, TT)
        loss.backward()
        out[name] = dict(loss=loss.detach().reshape(1), grad=sr.grad, csum=csum[0])
    return s, t, center, out["ref"], out["plain"]


def _dino_run(dev, s, t, center, B, V, G, K, dt, **kw):
    dbuf, ds = guarded(dev, V * B * K, dt); lbuf, loss = guarded(dev, 1); cbuf, csum = guarded(dev, K)
    wbuf, ws = guarded(dev, 2 * (V + G) * B)
    ws.fill_(float("nan"))                           # the row stats are written before they are read (the guard keeps its sentinel)
    st, tt = kw.pop("student_temp", TS), kw.pop("teacher_temp", TT)
    ops().dino_loss(s.to(dev), t.to(dev), center[0].to(dev), ds.view(V * B, K), loss, csum, ws, B, V, G, K, st, tt, **kw)
    torch.cuda.synchronize()
    guard_ok(dbuf, V * B * K, "dstudent"); guard_ok(lbuf, 1, "loss"); guard_ok(cbuf, K, "center_sum"); guard_ok(wbuf, ws.numel(), "workspace")
    return ds.view(V * B, K).cpu(), loss.cpu(), csum.cpu()


# The 16-bit form evaluates exp and log with the hardware's approximate instructions.  Reference side: perturb every exp and every
# log of the fp64 restatement by a relative 2^-21 (four f32 ulps, the allowance this file grants an approximate transcendental).  A
# teacher probability is exp(.) / exp(log-sum): two perturbed factors, so every t -- and with it the loss, which is linear in t --
# moves by a relative 2^-20; the student's log-sum-exp moves logp by 2^-21 * |lse|, which |loss| bounds.  The 16-bit form's loss may
# therefore miss fp64 by FAST_REL * |loss| on top of the plain-f32 error, 4 x the sum as everywhere.  (It also still adds its
# workgroups' partial sums by f32 atomics in arrival order: ~3e-5 at a loss of 45, inside this allowance; the f32 form does not.)
FAST_REL = 2.0 ** -20


def _dino_add(m, what, ds, loss, csum, ref, plain, dt, gscale=1.0, with_loss=True):
    m.add("grad" if gscale == 1.0 else f"grad x {gscale:g}", ds, gscale * ref["grad"], gscale * plain["grad"], sixteen=dt != f32, what=what)
    lp = plain["loss"].double()
    if dt != f32:     # the loss is an f32 scalar of the fast-math kernel: 4 x (e32 + FAST_REL * |ref|)
        lp = ref["loss"] + (lp - ref["loss"]).abs() + FAST_REL * ref["loss"].abs()
    if with_loss:
        m.add("loss", loss, ref["loss"], lp, what=what)
    m.add("center_sum", csum, ref["csum"], plain["csum"], what=what)


@pytest.mark.parametrize("dt", [bf16, f32], ids=["16bit", "f32"])
@pytest.mark.parametrize("B,V,G,K", DINO_CASES)
def test_dino_loss_fp64(dev, B, V, G, K, dt):
    """loss_grad_kernel's batch loop (B = 19 at K = 65 536: b_per = 2 and a one-row last slice), the t[2] / t[3] arms (G = 3 = V, G = 4),
    V = 16, K = 1028 / 2052 (row_stats' second 16-byte piece partly outside the row, K no multiple of 1024), K = 4 (one live thread).
    Loss, gradient and centre sum against oracle.vit_oracle.dino_loss on doubles; the f32 form (expf / logf) under the f32 rule, the
    16-bit form under the 16-bit rule; its f32 loss scalar may add 4 x FAST_REL * |loss| (derived above FAST_REL).
    (The f32 form's loss scalar has a test of its own below: test_dino_loss_f32_loss_scalar.)
    At (2, 3, 3, 2052) the teacher logits are integers -2..2 and the centre sum is torch.equal.
    e32 on this data (vo.dino_loss in f32 on the CPU), cases in the order of DINO_CASES: grad 6.8e-7, 2.5e-7, 6.6e-7, 7.9e-8, 2.3e-7
    (floor 3.0e-7); loss 2.6e-6, 2.2e-6, 2.0e-6, 2.7e-6, 4.8e-7 (loss values 12 to 45); centre sum 3.7e-6, 1.1e-6, 0 (integers),
    3.6e-7, 1.2e-7.  Before loss_grad_kernel<float> rounded logit / temperature as row_stats_kernel does, its gradient missed this
    bound by up to 4.1x at the three small cases (LAB_NOTES.md)."""
    integer = (B, V, G, K) == DINO_INT_TEACHER_CASE
    s, t, center, ref, plain = _dino_case(B, V, G, K, integer)
    ds, loss, csum = _dino_run(dev, s, t, center, B, V, G, K, dt)
    if integer:
        assert torch.equal(csum, t.sum(0)), "centre sum of integer teacher logits"
    m = Measured()
    _dino_add(m, f"{(B, V, G, K)}", ds, loss, csum, ref, plain, dt, with_loss=dt != f32)
    m.check()


@pytest.mark.parametrize("B,V,G,K", DINO_CASES)
def test_dino_loss_f32_loss_scalar(dev, B, V, G, K):
    """The loss scalar of gv_dino_loss_f32 under the f32 rule: 4 x the error of vo.dino_loss in f32 on the CPU (e32, cases in the
    order of DINO_CASES: 2.6e-6, 2.2e-6, 2.0e-6, 2.7e-6, 4.8e-7), never less than 4 x half an f32 ulp of the loss; and the same bits
    from a second call.  The f32 form sums its loss in a fixed order (loss_rows_kernel: one workgroup per student row, then one
    workgroup over the rows).  While loss_grad_kernel<float> added one partial sum per workgroup with atomicAdd in arrival order --
    640 roundings at a running sum of up to 45 at (19, 2, 2, 65 536) -- three runs of one build gave |loss - fp64| = 2.6e-6, 2.4e-5
    (2.25 x the bound) and 8.9e-6 there."""
    s, t, center, ref, plain = _dino_case(B, V, G, K, (B, V, G, K) == DINO_INT_TEACHER_CASE)
    _, loss, _ = _dino_run(dev, s, t, center, B, V, G, K, f32)
    m = Measured()
    _, again, _ = _dino_run(dev, s, t, center, B, V, G, K, f32)
    assert torch.equal(loss, again), "the f32 form's loss changes from call to call"
    m.add("loss", loss, ref["loss"], plain["loss"], what=f"{(B, V, G, K)}")
    m.check()


def test_dino_loss_options(dev):
    """The 16-bit (fast-math) kernel at (3, 6, 4, 1028), each option under the 16-bit rule against fp64: (a) `hyper` carries the
    temperatures and the by-value ones differ (0.2 / 0.07): the result is that of the hyper temperatures; (b) loss_scale = 1024: the
    gradient is bit for bit 1024 x the unscaled one (a power of two), the loss is not scaled; (c) grad_scale = 0.25.
    e32 as test_dino_loss_fp64 at this case (grad 2.5e-7, times the option's scale)."""
    B, V, G, K = DINO_OPTIONS_CASE
    s, t, center, ref, plain = _dino_case(B, V, G, K, False)
    base = _dino_run(dev, s, t, center, B, V, G, K, bf16)
    m = Measured()
    hyper = torch.zeros(L().HYP_COUNT)
    hyper[L().HYP_TEACHER_TEMP], hyper[L().HYP_STUDENT_TEMP] = TT, TS
    a = _dino_run(dev, s, t, center, B, V, G, K, bf16, student_temp=r32(0.2), teacher_temp=r32(0.07), hyper=hyper.to(dev))
    _dino_add(m, "(a) hyper", *a, ref, plain, bf16)
    b = _dino_run(dev, s, t, center, B, V, G, K, bf16, loss_scale=torch.tensor([1024.0, 0.0, 0.0, 0.0], device=dev))
    assert torch.equal(b[0].float(), base[0].float() * 1024.0), "(b) the gradient is not exactly 1024 x the unscaled one"
    _dino_add(m, "(b) loss_scale", *b, ref, plain, bf16, gscale=1024.0)
    c = _dino_run(dev, s, t, center, B, V, G, K, bf16, grad_scale=0.25)
    _dino_add(m, "(c) grad_scale", *c, ref, plain, bf16, gscale=0.25)
    m.check()


# ============================================================================ 13. softmax_lsce
def test_softmax_lsce_fp64(dev):
    """softmax_lsce_kernel (one thread per sample) at C = 1, 2, 64 (its register arrays full) and B = 1, 256 (one full workgroup), 257
    (a second one with one live thread), against oracle.vit_oracle.softmax_lsce on doubles; with loss_scale = 1024 the gradient is
    bit for bit 1024 x the unscaled one and the loss is the same number.
    e32 over the test (vo.softmax_lsce in f32 on the CPU): loss 2.7e-7, dlogits 5.0e-8, prob 1.0e-7."""
    from oracle import vit_oracle as vo
    o = ops()
    m = Measured()
    S = torch.tensor([1024.0, 0.0, 0.0, 0.0], device=dev)
    for C in LSCE_CS:
        for B in LSCE_BS:
            g = gen(C * 1000 + B)
            z = torch.randn(B, C, generator=g) * 2; tgt = torch.randint(0, C, (B, 1), generator=g)
            res = {}
            for name, d in (("ref", f64), ("plain", f32)):
                zr = z.to(d).clone().requires_grad_(True)
                loss = vo.softmax_lsce(zr, tgt, r32(0.1)); loss.backward()
                res[name] = (loss.detach().reshape(1), zr.grad, torch.softmax(z.to(d), 1))
            runs = []
            for ls in (None, S):
                lbuf, loss = guarded(dev, 1); dbuf, dz = guarded(dev, B * C); pbuf, prob = guarded(dev, B * C)
                o.softmax_lsce(z.to(dev), tgt.view(-1).to(dev), loss, dz.view(B, C), prob.view(B, C), B, C, r32(0.1), loss_scale=ls)
                torch.cuda.synchronize()
                guard_ok(lbuf, 1, "loss"); guard_ok(dbuf, B * C, "dlogits"); guard_ok(pbuf, B * C, "prob")
                runs.append((loss.cpu(), dz.cpu(), prob.cpu()))
            assert torch.equal(runs[1][1], runs[0][1] * 1024.0) and torch.equal(runs[1][0], runs[0][0]), (C, B, "loss_scale")
            tag = f"C={C} B={B}"
            m.add("loss", runs[0][0], res["ref"][0], res["plain"][0], what=tag, pool="loss: one number per case, pooled")
            m.add("dlogits", runs[0][1], res["ref"][1], res["plain"][1], what=tag)
            m.add("prob", runs[0][2], res["ref"][2], res["plain"][2], what=tag)
    m.check()


# ============================================================================ 14. optimizer against an independent Adam
B1, B2, AEPS = r32(0.9), r32(0.999), r32(1e-8)


def adam_step(st, g, *, lr, wd, bc1, bc2, mom, mode):
    """One step of the three optimizer modes + the EMA copy, in the dtype of the state (fp64: the reference; f32: the plain-f32
    figure).  st = dict(p, m, v, t).  torch.optim.AdamW / Adam(+L2) / SGD(Nesterov) semantics, written out."""
    p, m, v, t = st["p"], st["m"], st["v"], st["t"]
    if mode == 0:
        p = p * (1.0 - lr * wd)
    elif mode in (1, 2):
        g = g + wd * p
    if mode == 2:
        m = m * B1 + g
        p = p - lr * (g + m * B1)
    elif mode in (0, 1):
        m = B1 * m + (1.0 - B1) * g
        v = B2 * v + (1.0 - B2) * g * g
        p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + AEPS)
    t = mom * t + (1.0 - mom) * p
    return dict(p=p, m=m, v=v, t=t)


class AdamState:
    """device buffers of one optimizer test (all guarded) + the fp64 / f32 CPU states"""

    def __init__(self, dev, n, seed):
        g = gen(seed)
        self.n, self.dev = n, dev
        init = dict(p=torch.randn(n, generator=g), m=0.1 * torch.randn(n, generator=g), v=0.01 * torch.rand(n, generator=g), t=torch.randn(n, generator=g))
        self.ref = {k: x.double() for k, x in init.items()}
        self.plain = {k: x.clone() for k, x in init.items()}
        self.buf, self.d = {}, {}
        for k, x in init.items():
            self.buf[k], self.d[k] = put(dev, x)
        self.buf["pb"], self.d["pb"] = guarded(dev, n, bf16)
        self.buf["tb"], self.d["tb"] = guarded(dev, n, bf16)
        self.g = g

    def grad(self, scale=1.0):
        return torch.randn(self.n, generator=self.g) * scale

    def launch(self, grad_d, **kw):
        d = self.d
        ops().adamw_ema(d["p"], grad_d, d["m"], d["v"], d["pb"], d["t"], d["tb"], self.n, beta1=B1, beta2=B2, eps=AEPS, **kw)

    def step_refs(self, g, gscale=1.0, **kw):
        self.ref = adam_step(self.ref, g.double() * gscale, **kw)
        self.plain = adam_step(self.plain, g * gscale, **kw)

    def check(self, what, names="pmvt"):
        torch.cuda.synchronize()
        m = Measured()
        for k in names:
            m.add({"p": "p", "m": "m", "v": "v", "t": "EMA copy"}[k], self.d[k], self.ref[k], self.plain[k], what=what)
            guard_ok(self.buf[k], self.n, k)
        assert torch.equal(self.d["pb"], self.d["p"].to(bf16)) and torch.equal(self.d["tb"], self.d["t"].to(bf16)), f"{what}: 16-bit copies"
        guard_ok(self.buf["pb"], self.n, "p_bf16"); guard_ok(self.buf["tb"], self.n, "teacher_bf16")
        m.check()


def _bc(step):
    return 1.0 - B1 ** step, 1.0 - B2 ** step


def test_adamw_second_trip(dev):
    """adamw_ema_kernel past its 4096-workgroup grid: n = 2^22 + 3108, so only the first 777 f32x4 units take the grid-stride step; one
    AdamW step (mode 0) against fp64, elements behind n guarded in all six buffers.
    e32 on this data (adam_step in f32 on the CPU): p 4.8e-7, m 5.7e-8, v 2.3e-9, EMA copy 4.7e-7."""
    st = AdamState(dev, ADAM_TRIP_N, 14)
    assert adam_trips(ADAM_TRIP_N) == (2, 777)
    g = st.grad()
    lr, wd, mom = r32(1e-3), r32(0.04), r32(0.99)
    st.launch(g.to(dev), lr=lr, weight_decay=wd, step=1, teacher_momentum=mom)
    bc1, bc2 = _bc(1)
    st.step_refs(g, lr=lr, wd=wd, bc1=bc1, bc2=bc2, mom=mom, mode=0)
    st.check("second trip")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_adamw_hyper_fp64(dev, mode):
    """The `hyper` branch of adam_resolve against fp64, three steps with a new gradient each: the device vector carries lr, wd, both
    bias corrections, the teacher momentum and the gradient scale of the step; the by-value fields are poisoned (lr = 0, step = 1,
    teacher_momentum = 0, grad_scale = 1) and by-value weight_decay is the 0 / 1 multiplier (1, 0, 1 over the steps).
    e32 on this data (n = 8192, adam_step in f32 on the CPU, the third step): mode 0: p 4.9e-7, m 5.7e-8, v 3.9e-9, EMA copy 5.3e-7;
    mode 1: p 3.3e-7, m 7.7e-8, v 6.5e-9, EMA copy 4.9e-7; mode 2 (SGD): p 3.2e-7, m 6.3e-7, v 0 (untouched), EMA copy 4.8e-7."""
    st = AdamState(dev, ADAM_N, 20 + mode)
    hyper = torch.zeros(L().HYP_COUNT, device=dev)
    for step, mult in ((1, 1.0), (2, 0.0), (3, 1.0)):
        g = st.grad()
        lr, wd, mom, gscale = r32(1e-3 * step), r32(0.05), r32(0.99 + 0.002 * step), r32(0.5 * step)
        bc1, bc2 = (r32(x) for x in _bc(step))
        hv = [0.0] * L().HYP_COUNT
        for k, x in ((L().HYP_LR, lr), (L().HYP_WD, wd), (L().HYP_BC1, bc1), (L().HYP_BC2, bc2), (L().HYP_TEACHER_MOM, mom), (L().HYP_GRAD_SCALE, gscale)):
            hv[k] = x
        hyper.copy_(torch.tensor(hv))
        st.launch(g.to(dev), lr=0.0, weight_decay=mult, step=1, teacher_momentum=0.0, grad_scale=1.0, hyper=hyper, mode=mode)
        st.step_refs(g, gscale, lr=lr, wd=wd * mult, bc1=bc1, bc2=bc2, mom=mom, mode=mode)
        st.check(f"hyper mode {mode} step {step}")


@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("applied", [0, 5])
def test_adamw_loss_scale_fp64(dev, applied, clip):
    """The loss-scaling branch against fp64: state [S = 1024, ., ., applied]; g = grad * grad_scale / S and the bias corrections are
    those of step applied + 1 whatever `step` the call passes (here 40); with clip_norm the scale is
    min(1, clip / (sqrt(gnorm_sq) * |grad_scale / S| + 1e-6)).  Three steps, the applied count advanced by hand.
    e32 on this data (n = 8192, adam_step in f32 on the CPU, the largest over the cases): p 6.2e-7, m 5.1e-8, v 2.4e-9, EMA copy
    5.2e-7."""
    st = AdamState(dev, ADAM_N, 30 + applied)
    S, gscale, lr, wd, mom = 1024.0, r32(0.5), r32(1e-3), r32(0.04), r32(0.99)
    for i in range(3):
        g = st.grad(S)                                                       # what a scaled backward leaves
        gn = torch.tensor([float((g.double() ** 2).sum())], dtype=f32)
        state = torch.tensor([S, 1.0, 0.0, float(applied + i)], device=dev)
        st.launch(g.to(dev), lr=lr, weight_decay=wd, step=40, grad_scale=gscale, clip_norm=clip, gnorm_sq=gn.to(dev), teacher_momentum=mom, loss_scale=state)
        eff = gscale / S
        if clip > 0:
            eff = eff * min(1.0, clip / (math.sqrt(float(gn)) * abs(gscale / S) + 1e-6))
        bc1, bc2 = _bc(applied + i + 1)
        st.step_refs(g, eff, lr=lr, wd=wd, bc1=bc1, bc2=bc2, mom=mom, mode=0)
        st.check(f"loss_scale applied={applied + i} clip={clip}")


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_adamw_loss_scale_skips_nonfinite(dev, bad):
    """A non-finite *gnorm_sq under loss scaling skips the step: p / m / v keep their bits, the EMA copy still moves (towards the
    unchanged p) and both 16-bit copies are refreshed.  e32: EMA copy 2.2e-7 (p / m / v: 0, they are compared bit for bit first)."""
    st = AdamState(dev, ADAM_N, 41)
    before = {k: st.d[k].clone() for k in "pmvt"}
    g = st.grad(1024.0); g[5] = bad
    mom = r32(0.9)
    st.launch(g.to(dev), lr=r32(1e-3), weight_decay=r32(0.04), step=1, clip_norm=1.0, gnorm_sq=torch.tensor([bad], device=dev), teacher_momentum=mom,
              loss_scale=torch.tensor([1024.0, 0.0, 0.0, 0.0], device=dev))
    torch.cuda.synchronize()
    for k in "pmv":
        assert torch.equal(st.d[k], before[k]), f"{k} changed in a skipped step"
    assert not torch.equal(st.d["t"], before["t"]), "the EMA copy did not move"
    for d in (st.ref, st.plain):
        d["t"] = mom * d["t"] + (1.0 - mom) * d["p"]
    st.check("skipped step", "pmvt")


def test_adamw_mode3_frozen(dev):
    """Mode 3 (frozen range): p / m / v keep their bits and the gradient buffer, all NaN, is read into nothing; the EMA and both
    16-bit copies are those of the unchanged p.  e32: EMA copy 2.3e-7."""
    st = AdamState(dev, ADAM_N, 43)
    before = {k: st.d[k].clone() for k in "pmv"}
    mom = r32(0.95)
    st.launch(torch.full((ADAM_N,), float("nan"), device=dev), lr=r32(1e-3), weight_decay=r32(0.04), step=1, teacher_momentum=mom, mode=3)
    torch.cuda.synchronize()
    for k in "pmv":
        assert torch.equal(st.d[k], before[k]), f"{k} changed in mode 3"
    for d in (st.ref, st.plain):
        d["t"] = mom * d["t"] + (1.0 - mom) * d["p"]
    st.check("mode 3", "pmvt")


def test_loss_scale_update_transitions(dev):
    """gv_loss_scale_update as a standalone sequence (growth interval 3), state = [S, tracker, skipped, applied], exact:
    finite, finite, finite (growth, tracker reset), inf (back-off, skip count up, applied unchanged), NaN (the same)."""
    sc = ops().LossScaler(dev, init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    gn = torch.zeros(1, device=dev)
    seq = ((4.0, [1024.0, 1.0, 0.0, 1.0]), (4.0, [1024.0, 2.0, 0.0, 2.0]), (4.0, [2048.0, 0.0, 0.0, 3.0]), (float("inf"), [1024.0, 0.0, 1.0, 3.0]),
           (float("nan"), [512.0, 0.0, 2.0, 3.0]), (1.0, [512.0, 1.0, 2.0, 4.0]))
    for val, want in seq:
        gn.fill_(val)
        sc.update(gn)
        assert sc.state.tolist() == want, (val, sc.state.tolist(), want)


# ============================================================================ 15. store_f32, center_update
def test_store_f32_and_center_update(dev):
    """gv_store_f32 at n = 1 and n = 16 (its maximum) with guards behind; center_update_kernel at K = 1, 255 and 257 (a partly filled
    and a second workgroup) against doubles.  e32 over the three K (the same line in f32 on the CPU): 5.2e-8 (floor 5.4e-8)."""
    o = ops()
    for n in (1, 16):
        buf, dst = guarded(dev, n)
        vals = [0.1 * (i + 1) for i in range(n)]
        o.store_f32(dst, vals)
        assert torch.equal(dst.cpu(), torch.tensor(vals, dtype=f32))
        guard_ok(buf, n, "store_f32")
    m = Measured()
    mom, inv_rows = r32(0.9), r32(1.0 / 6)
    for K in CENTER_KS:
        g = gen(K)
        c = 0.3 * torch.randn(K, generator=g); cs = 6 * torch.randn(K, generator=g)
        buf, cd = put(dev, c)
        o.center_update(cd, cs.to(dev), K, mom, inv_rows)
        m.add("center", cd, c.double() * mom + cs.double() * inv_rows * (1.0 - mom), c * mom + cs * inv_rows * (1.0 - mom), what=f"K={K}", pool="center: K = 1 is one number, pooled")
        guard_ok(buf, K, "center")
    m.check()


# ============================================================================ argument checks (nothing is launched)
def test_row_kernels_reject_bad_arguments(dev):
    """What a GV_REQUIRE refuses before any launch, as GipvitError."""
    o, l = ops(), L()
    E = l.GipvitError
    z = torch.zeros(4096, device=dev)
    with pytest.raises(E, match="even"):
        o.colsum(z, 4, 3, z, z, ld=4)                                         # odd C
    with pytest.raises(E, match="multiple of 4"):
        o.adamw_ema(z, z, z, z, None, None, None, 6, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1)
    zb = torch.zeros(4096, dtype=bf16, device=dev)
    for (B, V, G, K), pat in (((2, 2, 2, 6), "multiple of 4"), ((2, 1, 1, 8), "G <= V"), ((2, 6, 5, 8), "1 <= G")):
        with pytest.raises(E, match=pat):
            o.dino_loss(z, z, z, zb, z, z, z, B, V, G, K, 0.1, 0.04)
    with pytest.raises(E, match="C <= 64"):
        o.softmax_lsce(z, torch.zeros(4, dtype=torch.int64, device=dev), z, z, None, 4, 65, 0.1)
    a = l.gv_store_f32_args()                                                 # ops.store_f32 cannot even hold a 17th value
    a.dst, a.n = z.data_ptr(), 17
    with pytest.raises(E, match="n <= 16"):
        l.call("gv_store_f32", a, o._stream())
    blocks = o.range_block_table([(0, 4096)]).to(dev); ranges = torch.ones(1, 2, device=dev)
    with pytest.raises(E, match="frozen range is left out"):
        o.adamw_ema_ranges(z, z, z, z, None, None, None, 4096, blocks, ranges, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, mode=3)
    torch.cuda.synchronize()
    assert float(z.abs().max()) == 0.0 and float(zb.float().abs().max()) == 0.0, "a rejected call wrote something"
