"""The cases of tests/traces/panel_outputs.json: one call per panel_kernel instantiation, and how a fixture row becomes that call.

Shared by the recorder (tools/panel_outputs_record.py) and the GPU test (tests/test_panel_bits_gpu.py).  A row holds the call;
`kernel` and `sha256` are what the recorder saw at the commit the fixture was taken from: the timing-row name of the launch and the
SHA-256 of every output buffer, copied back to the host.  The panel kernels use no atomics, so the digests are reproducible.

Operands are built on the CPU (no device RNG): the 16-bit ones are linear_plan_cases.ints, everything in f32 is a closed form of its
index -- none of them all ones or all zeros.  Every output buffer carries one guard row of 9s behind its last row, inside the digest."""
import functools
import hashlib
import json
import os

import linear_plan_cases as lc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "traces", "panel_outputs.json")
PN = 384
ROW_M = (200, 16400, 28700, 36900, 45100)           # FM 4, 7, 9, 11, 12 of pick_fm at the default CU budget, a ragged last panel each
WIDE_M = (2100, 16400, 28700, 36900, 45100)         # the same of pick_fm_wide with two column blocks
B, G, R, DG, SP = lc.BIAS, lc.GELU, lc.RESID, lc.DGELU, lc.SAVE_PRE
# (label, epilogue flags, trans_b, f32 C): one gv_linear call per MODE_WIDE epilogue, as plan_wide maps the flags
WIDE_EPS = (("bias", B, 0, 0), ("bias_gelu", B | G, 0, 0), ("bias_gelu_save", B | G | SP, 0, 0), ("none_tb", 0, 1, 0), ("dgelu_tb", DG, 1, 0),
            ("bias_resid_f32", B | R, 0, 1))


def cases():
    rows = []
    for op in ("ln_fwd", "ln_bwd"):
        for K in (256, 192):            # 256: the ping-pong loop, two tile pairs; 192: the one-stage-ahead loop
            rows += [dict(id="%s_M%d_K%d" % (op, M, K), op=op, M=M, N=PN, K=K) for M in ROW_M]
    rows += [dict(id="mlp_ln_fwd_M%d" % M, op="mlp_ln_fwd", M=M, N=PN, K=128, hidden=512) for M in ROW_M[:2]]
    for label, epi, tb, c_f32 in WIDE_EPS:
        rows += [dict(id="wide_%s_M%d" % (label, M), op="wide", M=M, N=2 * PN, K=256, epi=epi, tb=tb, c_f32=c_f32) for M in WIDE_M]
    return rows


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def row_id(r):
    return r["id"]


# ---------------------------------------------------------------------------------------------- operands (CPU, cached, never written)
def _closed(n, mul, mod, off, scale):
    """f32 value ((i * mul) % mod + off) * scale of every index i < n (exact: small integers times a power of two)"""
    import torch
    return ((torch.arange(n, dtype=torch.int64) * mul) % mod + off).to(torch.float32) * scale


@functools.lru_cache(maxsize=None)
def vec(what, n, dev):
    mul, mod, off, scale = {"bias": (1, 5, -2, 0.25), "bias1": (3, 7, -3, 0.125), "gamma": (1, 3, 2, 0.25), "beta": (1, 4, -1, 0.125),
                            "row_scale": (1, 4, 1, 0.25), "gb_scale": (1, 3, 1, 0.5), "mean": (1, 5, -2, 0.125), "rstd": (1, 3, 2, 0.25)}[what]
    return _closed(n, mul, mod, off, scale).to(dev)


@functools.lru_cache(maxsize=None)
def mat(what, M, N, dev):
    mul, mod, off, scale = {"resid": (1, 7, -3, 0.5), "x": (7, 11, -5, 0.25), "g": (5, 13, -6, 0.125), "aux": (3, 9, -4, 0.25)}[what]
    return _closed(M * N, mul, mod, off, scale).view(M, N).to(dev)


@functools.lru_cache(maxsize=None)
def ints(shape, dev, lo, hi, seed):
    return lc.ints(shape, dev, lo, hi, seed)


def guarded(M, N, dtype, dev):
    import torch
    return torch.full((M + 1, N), 9.0, dtype=dtype, device=dev)


# ---------------------------------------------------------------------------------------------- the call and its output buffers
def run(o, L, r, dev):
    """One row, once, under linear_timing: (timing rows, {output name: tensor})."""
    import torch
    f32, b16 = torch.float32, torch.bfloat16
    dev = str(dev)
    M, N, K = r["M"], r["N"], r["K"]
    if r["op"] == "ln_fwd":
        A, W = ints((M, K), dev, -2, 3, 91), ints((N, K), dev, -2, 3, 92)
        out = dict(out=guarded(M, N, f32, dev), y=guarded(M, N, b16, dev), mean=guarded(M, 1, f32, dev), rstd=guarded(M, 1, f32, dev))
        rows = lc.timed(o, lambda: o.linear_ln_fwd(A, W, out["out"], M, K, bias=vec("bias", N, dev), resid=mat("resid", M, N, dev),
                                                   gamma=vec("gamma", N, dev), beta=vec("beta", N, dev), y=out["y"], mean=out["mean"],
                                                   rstd=out["rstd"], row_scale=vec("row_scale", M, dev)))
        return rows, out
    if r["op"] == "mlp_ln_fwd":
        H = r["hidden"]
        A, W1, W2 = ints((M, K), dev, -2, 3, 93), ints((H, K), dev, -1, 2, 94), ints((N, H), dev, -1, 2, 95)
        out = dict(out=guarded(M, N, f32, dev), y=guarded(M, N, b16, dev), mean=guarded(M, 1, f32, dev), rstd=guarded(M, 1, f32, dev))
        rows = lc.timed(o, lambda: o.mlp_ln_fwd(A, W1, vec("bias1", H, dev), W2, out["out"], M, K, H, bias2=vec("bias", N, dev),
                                                resid=mat("resid", M, N, dev), gamma=vec("gamma", N, dev), beta=vec("beta", N, dev),
                                                y=out["y"], mean=out["mean"], rstd=out["rstd"]))
        return rows, out
    if r["op"] == "ln_bwd":
        dY, W = ints((M, K), dev, -2, 3, 96), ints((K, N), dev, -2, 3, 97)
        g = guarded(M, N, f32, dev)
        g[:M] = mat("g", M, N, dev)
        gb = guarded(M, N, b16, dev)
        blocks = L.lib.gv_linear_ln_blocks(M)
        partials = torch.full((blocks + 1, 3, N), 9.0, dtype=f32, device=dev)      # (the guard row: one block past the launch's)
        rows = lc.timed(o, lambda: o.linear_ln_bwd(dY, W, mat("x", M, N, dev), vec("mean", M, dev), vec("rstd", M, dev), vec("gamma", N, dev),
                                                   g, gb, partials, M, K, g_init=False, gb_scale=vec("gb_scale", M, dev)))
        return rows, dict(g=g, gb=gb, partials=partials)
    e, tb = r["epi"], r["tb"]
    A, Bm = ints((M, K), dev, -2, 3, 98), ints((K, N) if tb else (N, K), dev, -2, 3, 99)
    out = dict(C=guarded(M, N, f32 if r["c_f32"] else b16, dev))
    kw = dict(trans_b=bool(tb), epilogue=e)
    if e & B:
        kw["bias"] = vec("bias", N, dev)
    if e & R:
        kw["resid"], kw["row_scale"] = mat("resid", M, N, dev), vec("row_scale", M, dev)
    if e & DG:
        kw["aux_in"] = mat("aux", M, N, dev).to(b16)
    if e & SP:
        out["aux_out"] = kw["aux_out"] = guarded(M, N, b16, dev)
    rows = lc.timed(o, lambda: o.linear(A, Bm, out["C"], M, N, K, **kw))
    return rows, out


def digests(out):
    """{name: SHA-256 of the buffer's bytes on the host}"""
    import torch
    res = {}
    for name, t in out.items():
        h = t.detach().cpu().contiguous()
        h = h.view(torch.int16) if h.dtype == torch.bfloat16 else h
        res[name] = hashlib.sha256(h.numpy().tobytes()).hexdigest()
    return res
