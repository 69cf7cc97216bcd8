"""Framed operands for the GEMM-class entry points: every matrix of a call sits inside a larger buffer, so that its leading dimension
differs from its width (include/gipvit.h: "matrices are row-major with an explicit leading dimension in ELEMENTS").

A frame is a flat buffer: a guard of at least ld + 8 elements, then `rows` rows of `ld` elements of which the first `width` are the
matrix, then a guard of ld + 8 elements; the first element of the matrix is 16-byte aligned.  Whatever is not the matrix holds NaN
where the call only reads the operand, and a fixed bit pattern where it writes it.  Contiguous outputs (y, mean, rstd, column sums,
partials) are frames with ld = width: guards only.  A case runs twice, on compact operands (ld = width, the same guards) and on framed
ones, and check():
  (a) every element outside the matrices of the written buffers is bit-unchanged (both runs);
  (b) the framed outputs are bit-identical to the compact ones (integer views, never floats);
  (c) both runs report one launch of the kernel the case names (linear_timing);
  (d) where the case carries an expectation (integer operands: the f64 product is exact), both equal it.
Two pad sets: "aligned" -- ld = width rounded up to 8, + 8 k with k = 1, 2, .. over the operands of the call (rows stay 16-byte aligned,
no two operands of a call share a pad); "minimum" -- the smallest ld > width that the entry point's own check accepts.

    python tests/leading_dims_cases.py GROUP      every case of the group on both pad sets (the test starts it with GIPVIT_CU_BUDGET=248:
                                                  the budget is read once per process)"""
import os
import sys

import linear_plan_cases as lpc
import panel_bits_cases as pb

BIAS, GELU, RESID, DGELU, ACCUM, SAVE_PRE = lpc.BIAS, lpc.GELU, lpc.RESID, lpc.DGELU, lpc.ACCUM, lpc.SAVE_PRE
PN = 384
LEFT = 8
PATTERN = {2: 0x3C5A, 4: 0x3C5A5A3C}          # what the padding of written buffers holds, per element size
PADS = ("aligned", "minimum")
_b = os.environ.get("GIPVIT_CU_BUDGET")
CU_BUDGET = int(_b) if _b and 64 <= int(_b) <= 256 else 256          # as gv_cu_budget() reads it


class Operand:
    """data: the compact matrix [rows, width] (a vector: [1, n]); mod: what the entry point's check asks of its leading dimension
    (ld % mod == 0), 0: the buffer is contiguous by contract (guards only); written: the call stores into it"""
    def __init__(self, data, mod, written=False):
        self.data, self.mod, self.written = data, mod, written


class Frame:
    def __init__(self, op, ld):
        import torch
        d = op.data
        self.rows, self.width, self.ld, self.written = d.shape[0], d.shape[1], ld, op.written
        es = d.element_size()
        unit = 16 // es
        self.off = -(-(ld + LEFT) // unit) * unit
        self.ity = torch.int16 if es == 2 else torch.int32
        self.buf = torch.empty(self.off + self.rows * ld + ld + LEFT, dtype=d.dtype, device=d.device)
        if op.written:
            self.buf.view(self.ity).fill_(PATTERN[es])
        else:
            self.buf.fill_(float("nan"))
        self.m = torch.as_strided(self.buf, (self.rows, self.width), (ld, 1), self.off)      # the matrix: what the call is handed
        self.m.copy_(d)
        assert self.m.data_ptr() % 16 == 0
        self.before = self._outside()

    def _outside(self):
        """the bits of everything that is not the matrix"""
        import torch
        t = self.buf.view(self.ity).clone()
        torch.as_strided(t, (self.rows, self.width), (self.ld, 1), self.off).zero_()
        return t

    def untouched(self):
        import torch
        return torch.equal(self._outside(), self.before)

    def bits(self):
        return self.m.contiguous().view(self.ity)


def pick_ld(width, mod, pads, k):
    if mod == 0 or pads == "compact":
        return width
    if pads == "aligned":
        return (width + 7) // 8 * 8 + 8 * k
    return (width // mod + 1) * mod


def frames(operands, pads):
    out, k = {}, 0
    for name, op in operands.items():
        k += 1 if op.mod else 0
        out[name] = Frame(op, pick_ld(op.data.shape[1], op.mod, pads, k))
    return out


# ---------------------------------------------------------------------------------------------- the cases
def _lin(id, kernel, M, N, K, ta=0, tb=0, c_f32=0, epi=0, colsum=0, ws=0, row_scale=0, f32=0):
    return dict(id=id, group="f32" if f32 else "wide" if kernel.startswith("panel") else "dw" if kernel.startswith("dw8") else "tile",
                op="linear", kernel=kernel, M=M, N=N, K=K, ta=ta, tb=tb, c_f32=c_f32, epi=epi, colsum=colsum, ws=ws, row_scale=row_scale, f32=f32)


def cases():
    tile = "gemm_kernel<%s>"
    c = [
        # the 128 x 128 tile kernel: ragged M, N and (K % 64 == 32) a ragged last K-step of the k-contiguous operands
        _lin("tile_nt_bias_bf16", tile % "false, false, bf16, false, 1", 130, 136, 96, epi=BIAS),
        _lin("tile_nt_bias_gelu_save", tile % "false, false, bf16, false, 67", 130, 136, 96, epi=BIAS | GELU | SAVE_PRE),
        _lin("tile_nt_f32_bias_resid_scaled", tile % "false, false, float, false, 5", 130, 136, 96, c_f32=1, epi=BIAS | RESID, row_scale=1),
        _lin("tile_nn_dgelu", tile % "false, true, bf16, false, 8", 130, 136, 96, tb=1, epi=DGELU),
        # the runtime-mask build: an epilogue without an instantiation of its own; N % 8 != 0 takes its scalar path
        _lin("tile_runtime_mask_f32", tile % "false, false, float, false, -1", 100, 72, 192, c_f32=1, epi=BIAS | GELU),
        _lin("tile_runtime_mask_bf16", tile % "false, false, bf16, false, -1", 100, 72, 192, epi=BIAS | RESID),
        _lin("tile_runtime_mask_ragged_n", tile % "false, false, bf16, false, -1", 100, 76, 192, epi=BIAS),
        # dW layout: K is the token count, any value
        _lin("tile_tn_f32", tile % "true, true, float, false, 0", 136, 72, 301, ta=1, tb=1, c_f32=1),
        _lin("tile_tn_accum_colsum", tile % "true, true, float, false, 16", 136, 72, 301, ta=1, tb=1, c_f32=1, epi=ACCUM, colsum=1),
        # four-stage ring
        _lin("deep_nt_bias", "gemm_deep_kernel<false, false, bf16, false, 1>", 128, 256, 960, epi=BIAS),
        # split-K ACCUM: f32 atomics into C without scratch, slab + splitk_reduce_kernel with it
        _lin("splitk_accum_atomics", "gemm_deep_kernel<true, true, float, true, 16>", 192, 192, 2053, ta=1, tb=1, c_f32=1, epi=ACCUM),
        _lin("splitk_accum_slab", "gemm_deep_kernel<true, true, float, true, 16>", 192, 192, 2053, ta=1, tb=1, c_f32=1, epi=ACCUM, ws=1),
        # few rows, a long reduction, scratch: split K, then splitk_epilogue_kernel
        _lin("fewrow_bias_gelu_save", tile % "false, false, float, true, 16", 128, 256, 2048, epi=BIAS | GELU | SAVE_PRE, ws=1),
        _lin("fewrow_f32_bias_resid_scaled", tile % "false, false, float, true, 16", 128, 256, 2048, c_f32=1, epi=BIAS | RESID, row_scale=1, ws=1),
        _lin("fewrow_nn_dgelu", tile % "false, true, float, true, 16", 128, 256, 2048, tb=1, epi=DGELU, ws=1),
        # the ping-pong dW kernel, both orientations (a ragged last K-tile in the normal one)
        _lin("dw8_normal_colsum", "dw8_kernel<false>", 128, 384, 2053, ta=1, tb=1, c_f32=1, epi=ACCUM, colsum=1, ws=1),
        _lin("dw8_swapped", "dw8_kernel<true>", 384, 1664, 4096, ta=1, tb=1, c_f32=1, epi=ACCUM, ws=1),
        _lin("dw8_swapped_colsum", "dw8_kernel<true>", 384, 1664, 4096, ta=1, tb=1, c_f32=1, epi=ACCUM, colsum=1, ws=1),
    ]
    # wide products on the full-row kernel: one and two column blocks, every MODE_WIDE epilogue, a ragged last row panel
    for N in (384, 768):
        for label, epi, tb, c_f32 in pb.WIDE_EPS:
            ep = {"none_tb": 0, "bias": 1, "bias_gelu": 2, "bias_gelu_save": 3, "dgelu_tb": 4, "bias_resid_f32": 5}[label]
            c.append(_lin("wide_%s_N%d" % (label, N), "panel_kernel<4, 8, 64, %s, 2, %d, 1>" % ("true" if tb else "false", ep), 2100, N, 128,
                          tb=tb, c_f32=c_f32, epi=epi, row_scale=int(label == "bias_resid_f32")))
    # fp32 operand mode: 4-byte alignment is all its checks ask
    for M, N, K in ((17, 5, 3), (136, 192, 96)):
        for ta, tb in ((0, 0), (0, 1), (1, 1)):      # (trans_a without trans_b is not built in either mode)
            c.append(_lin("f32_%d%d_%dx%dx%d" % (ta, tb, M, N, K), "linear_f32_kernel", M, N, K, ta=ta, tb=tb, c_f32=1, f32=1))
        c.append(_lin("f32_bias_gelu_save_%dx%dx%d" % (M, N, K), "linear_f32_kernel", M, N, K, c_f32=1, epi=BIAS | GELU | SAVE_PRE, f32=1))
        c.append(_lin("f32_bias_resid_%dx%dx%d" % (M, N, K), "linear_f32_kernel", M, N, K, c_f32=1, epi=BIAS | RESID, row_scale=1, f32=1))
        c.append(_lin("f32_accum_colsum_%dx%dx%d" % (M, N, K), "linear_f32_kernel", M, N, K, ta=1, tb=1, c_f32=1, epi=ACCUM, colsum=1, f32=1))
    # grouped dW: the tile group (ragged T) and the ping-pong group (every problem tiles into 128 x 384 pieces)
    c.append(dict(id="group_tile_D192_T1500", group="dw", op="group", kernel="gemm_dw_group_kernel", T=1500, probs=[[192, 768], [768, 192], [192, 192], [576, 192]]))
    c.append(dict(id="group_dw8_D384_T2048", group="dw", op="group", kernel="dw8_group_kernel", T=2048, probs=[[384, 1536], [1536, 384], [384, 384], [1152, 384]]))
    # full-row kernels: K = 192 the one-stage-ahead loop, K = 384 the ping-pong loop; M = 64 one workgroup, M = 1380 a ragged last one
    for M in (64, 1380):
        for K in (192, 384):
            pp = int(K % 128 == 0)
            for ln in (0, 1):
                c.append(dict(id="ln_fwd_M%d_K%d_%s" % (M, K, "ln_scaled" if ln else "plain"), group="fullrow", op="ln_fwd", kernel="panel_kernel<4, 8, 64, false, 0, 0, %d>" % pp,
                              M=M, K=K, ln=ln))
            for g_init in (0, 1):
                c.append(dict(id="ln_bwd_M%d_K%d_ginit%d" % (M, K, g_init), group="fullrow", op="ln_bwd", kernel="panel_kernel<4, 8, 64, true, 1, 0, %d>" % pp,
                              M=M, K=K, g_init=g_init))
    c.append(dict(id="mlp_fm4", group="fullrow", op="mlp", kernel="panel_kernel<4, 8, 64, false, 0, 1, 0>", M=300, K=384, hidden=1536))
    # (the smallest M past pick_fm_mlp's threshold, M > 64 x the CU budget)
    c.append(dict(id="mlp_fm7", group="fullrow", op="mlp", kernel="panel_kernel<7, 8, 64, false, 0, 1, 0>", M=64 * CU_BUDGET + 1, K=128, hidden=256))
    return c


GROUPS = ("tile", "wide", "dw", "f32", "fullrow")


# ---------------------------------------------------------------------------------------------- operands, the call, the expectation
def _ints(shape, dev, lo, hi, seed, dtype):
    return pb.ints(tuple(shape), str(dev), lo, hi, seed).to(dtype)


def _closed(rows, cols, mul, mod, off, scale, dev):
    import torch
    return (((torch.arange(rows * cols, dtype=torch.int64) * mul) % mod + off).to(torch.float32) * scale).view(rows, cols).to(dev)


def build_linear(o, r, dev):
    """operands of a gv_linear case + what the outputs must hold (exact: integer products, integer or dyadic epilogue operands)"""
    import torch
    f32 = torch.float32
    t16 = f32 if r["f32"] else o.bf16
    M, N, K, e = r["M"], r["N"], r["K"], r["epi"]
    lo, hi = (-1, 2) if K > 2048 else (-2, 3)
    A = _ints((K, M) if r["ta"] else (M, K), dev, lo, hi, 51, t16)
    B = _ints((K, N) if r["tb"] else (N, K), dev, lo, hi, 52, t16)
    amod = 1 if r["f32"] else 8
    cmod = 1 if r["f32"] else 4
    out_t = f32 if r["c_f32"] else t16
    ops = dict(A=Operand(A, amod), B=Operand(B, amod))
    v = ((A.double().t() if r["ta"] else A.double()) @ (B.double() if r["tb"] else B.double().t())).to(f32)
    kw, expect = {}, {}
    C0 = torch.full((M, N), 9.0, dtype=out_t, device=dev)
    if e & BIAS:
        kw["bias"] = pb.vec("bias", N, str(dev)) * 4.0                 # integers -2 .. 2
        v = v + kw["bias"]
    if e & SAVE_PRE:
        ops["aux_out"] = Operand(torch.full((M, N), 9.0, dtype=t16, device=dev), cmod, written=True)
        expect["aux_out"] = v.to(t16)
    if e & GELU:
        v = None if r["f32"] else lpc.gelu_ref(v.cpu()).to(dev)      # (the fp32 mode calls erff: no exact form; its pre-activation is checked)
    if e & DGELU:
        aux = _closed(M, N, 3, 41, -20, 0.25, dev).to(t16)              # -5 .. 5 in quarters
        ops["aux_in"] = Operand(aux, cmod)
        v = v * lpc.dgelu_ref(aux.float().cpu()).to(dev)
    if e & RESID:
        resid = pb.mat("resid", M, N, str(dev))
        ops["resid"] = Operand(resid, cmod)
        if r["row_scale"]:
            kw["row_scale"] = pb.vec("row_scale", M, str(dev))          # quarters: the product with an integer is exact, fused or not
            v = v * kw["row_scale"][:, None]
        v = v + resid
    if e & ACCUM:
        C0 = _closed(M, N, 1, 5, -2, 1.0, dev)
        v = v + C0
    ops["C"] = Operand(C0, cmod, written=True)
    if v is not None:
        expect["C"] = v.to(out_t)
    if r["colsum"]:
        ops["colsum_a"] = Operand(torch.full((1, M), 2.0, dtype=f32, device=dev), 0, written=True)
        expect["colsum_a"] = (2.0 + A.double().sum(0)).to(f32).view(1, M)
    return ops, kw, expect


def call_linear(o, r, fr, kw, ws):
    ld = {n: f.ld for n, f in fr.items()}
    more = dict(kw)
    for n in ("resid", "aux_in", "aux_out"):
        if n in fr:
            more[n] = fr[n].m
    if "colsum_a" in fr:
        more["colsum_a"] = fr["colsum_a"].m
    if r["ws"]:
        more["workspace"] = ws
    o.linear(fr["A"].m, fr["B"].m, fr["C"].m, r["M"], r["N"], r["K"], trans_a=bool(r["ta"]), trans_b=bool(r["tb"]), epilogue=r["epi"],
             lda=ld["A"], ldb=ld["B"], ldc=ld["C"], ldr=ld.get("resid"), ld_aux=ld.get("aux_in", ld.get("aux_out")), **more)


def build_group(o, r, dev):
    import torch
    f32 = torch.float32
    T, ops, expect = r["T"], {}, {}
    for q, (m, n) in enumerate(r["probs"]):
        dY, X = _ints((T, m), dev, -1, 2, 60 + q, o.bf16), _ints((T, n), dev, -1, 2, 70 + q, o.bf16)
        ops["dY%d" % q], ops["X%d" % q] = Operand(dY, 8), Operand(X, 8)
        ops["dW%d" % q] = Operand(torch.full((m, n), float(q), dtype=f32, device=dev), 4, written=True)
        expect["dW%d" % q] = (q + dY.double().t() @ X.double()).to(f32)
        if q % 2 == 0:
            ops["cs%d" % q] = Operand(torch.full((1, m), 2.0, dtype=f32, device=dev), 0, written=True)
            expect["cs%d" % q] = (2.0 + dY.double().sum(0)).to(f32).view(1, m)
    return ops, {}, expect


def call_group(o, r, fr, kw, ws):
    probs = [(fr["dY%d" % q].m, fr["X%d" % q].m, fr["dW%d" % q].m, fr["cs%d" % q].m if "cs%d" % q in fr else None) for q in range(len(r["probs"]))]
    o.linear_dw_group(probs, r["T"], ws)


def _fwd_outputs(o, M, dev):
    import torch
    f32 = torch.float32
    return dict(out=Operand(torch.full((M, PN), 9.0, dtype=f32, device=dev), 2, written=True),
                y=Operand(torch.full((M, PN), 9.0, dtype=o.bf16, device=dev), 0, written=True),
                mean=Operand(torch.full((1, M), 9.0, dtype=f32, device=dev), 0, written=True),
                rstd=Operand(torch.full((1, M), 9.0, dtype=f32, device=dev), 0, written=True))


def build_ln_fwd(o, r, dev):
    M, K, d = r["M"], r["K"], str(dev)
    A, W = _ints((M, K), dev, -2, 3, 91, o.bf16), _ints((PN, K), dev, -2, 3, 92, o.bf16)
    resid = pb.mat("resid", M, PN, d)
    ops = dict(A=Operand(A, 8), W=Operand(W, 8), resid=Operand(resid, 4), **_fwd_outputs(o, M, dev))
    kw = dict(bias=pb.vec("bias", PN, d))
    v = (A.double() @ W.double().t()).float() + kw["bias"]
    if r["ln"]:
        kw.update(gamma=pb.vec("gamma", PN, d), beta=pb.vec("beta", PN, d), row_scale=pb.vec("row_scale", M, d))
        v = v * kw["row_scale"][:, None]
    return ops, kw, dict(out=v + resid)                                 # (quarters and halves of small integers: exact in f32)


def call_ln_fwd(o, r, fr, kw, ws):
    more = dict(kw)
    if r["ln"]:
        more.update(y=fr["y"].m, mean=fr["mean"].m, rstd=fr["rstd"].m)
    o.linear_ln_fwd(fr["A"].m, fr["W"].m, fr["out"].m, r["M"], r["K"], resid=fr["resid"].m, lda=fr["A"].ld, ldw=fr["W"].ld, ldr=fr["resid"].ld, ldo=fr["out"].ld, **more)


def build_mlp(o, r, dev):
    M, K, H, d = r["M"], r["K"], r["hidden"], str(dev)
    ops = dict(A=Operand(_ints((M, K), dev, -2, 3, 93, o.bf16), 8), W1=Operand(_ints((H, K), dev, -1, 2, 94, o.bf16), 8),
               W2=Operand(_ints((PN, H), dev, -1, 2, 95, o.bf16), 8), resid=Operand(pb.mat("resid", M, PN, d), 4), **_fwd_outputs(o, M, dev))
    kw = dict(bias2=pb.vec("bias", PN, d), gamma=pb.vec("gamma", PN, d), beta=pb.vec("beta", PN, d), row_scale=pb.vec("row_scale", M, d))
    return ops, kw, {}


def call_mlp(o, r, fr, kw, ws):
    o.mlp_ln_fwd(fr["A"].m, fr["W1"].m, pb.vec("bias1", r["hidden"], str(fr["A"].m.device)), fr["W2"].m, fr["out"].m, r["M"], r["K"], r["hidden"],
                 resid=fr["resid"].m, y=fr["y"].m, mean=fr["mean"].m, rstd=fr["rstd"].m, lda=fr["A"].ld, ldw1=fr["W1"].ld, ldw2=fr["W2"].ld,
                 ldr=fr["resid"].ld, ldo=fr["out"].ld, **kw)


def build_ln_bwd(o, L, r, dev):
    import torch
    f32 = torch.float32
    M, K, d = r["M"], r["K"], str(dev)
    blocks = L.lib.gv_linear_ln_blocks(M)
    g0 = torch.full((M, PN), float("nan"), dtype=f32, device=dev) if r["g_init"] else pb.mat("g", M, PN, d)      # g_init: g is not read
    ops = dict(dY=Operand(_ints((M, K), dev, -2, 3, 96, o.bf16), 8), W=Operand(_ints((K, PN), dev, -2, 3, 97, o.bf16), 8),
               x=Operand(pb.mat("x", M, PN, d), 2), g=Operand(g0, 2, written=True),
               gb=Operand(torch.full((M, PN), 9.0, dtype=o.bf16, device=dev), 2, written=True),
               partials=Operand(torch.full((blocks, 3 * PN), 9.0, dtype=f32, device=dev), 0, written=True))
    return ops, dict(gb_scale=pb.vec("gb_scale", M, d)), {}


def call_ln_bwd(o, r, fr, kw, ws):
    d = str(fr["x"].m.device)
    M = r["M"]
    blocks = o.linear_ln_bwd(fr["dY"].m, fr["W"].m, fr["x"].m, pb.vec("mean", M, d), pb.vec("rstd", M, d), pb.vec("gamma", PN, d), fr["g"].m, fr["gb"].m,
                             fr["partials"].m, M, r["K"], g_init=bool(r["g_init"]), lda=fr["dY"].ld, ldw=fr["W"].ld, ldx=fr["x"].ld, ldg=fr["g"].ld,
                             ldgb=fr["gb"].ld, **kw)
    assert blocks == fr["partials"].rows, (blocks, fr["partials"].rows)


def build(o, L, r, dev):
    if r["op"] == "linear":
        return build_linear(o, r, dev)
    if r["op"] == "group":
        return build_group(o, r, dev)
    if r["op"] == "ln_fwd":
        return build_ln_fwd(o, r, dev)
    if r["op"] == "mlp":
        return build_mlp(o, r, dev)
    return build_ln_bwd(o, L, r, dev)


CALLS = dict(linear=call_linear, group=call_group, ln_fwd=call_ln_fwd, mlp=call_mlp, ln_bwd=call_ln_bwd)


def run(o, L, r, dev, ws, pads):
    """The case on `pads` ("compact", "aligned", "minimum"): (timing rows, frames, expectation)."""
    import torch
    ops, kw, expect = build(o, L, r, dev)
    fr = frames(ops, pads)
    ws.fill_(float("nan"))      # the split-K scratch as a kernel must expect it, in front of every call: a slab reduce that reads a slice nothing stored gives NaN
    rows = lpc.timed(o, lambda: CALLS[r["op"]](o, r, fr, kw, ws))
    torch.cuda.synchronize()
    return rows, fr, expect


def check(o, L, r, dev, ws, pads):
    """(a) - (d) of the module docstring for case r on pad set `pads`; raises AssertionError."""
    import torch
    rows_c, fc, expect = run(o, L, r, dev, ws, "compact")
    rows_f, ff, _ = run(o, L, r, dev, ws, pads)
    names_c, names_f = [(x["kernel"], x["launches"]) for x in rows_c], [(x["kernel"], x["launches"]) for x in rows_f]
    print(r["id"], pads, names_f, {n: f.ld for n, f in ff.items() if f.ld != f.width})
    assert names_c == [(r["kernel"], 1)], ("compact", names_c)
    assert names_f == [(r["kernel"], 1)], (pads, names_f)
    written = [n for n, f in ff.items() if f.written]
    assert written
    assert all(f.ld != f.width for n, f in ff.items() if n in ("A", "B", "C", "W", "out", "g", "gb", "x", "dY", "dW0", "X0", "W1", "W2", "resid", "aux_in", "aux_out"))
    for what, fr in (("compact", fc), (pads, ff)):
        for n in written:
            assert fr[n].untouched(), "%s: the call wrote outside %s" % (what, n)
    for n in written:
        got, ref = ff[n].bits(), fc[n].bits()
        assert torch.equal(got, ref), "%s: %d of %d elements differ from the compact call (first at %s)" % (
            n, int((got != ref).sum()), got.numel(), (got != ref).nonzero()[0].tolist())
    for n, want in expect.items():
        for what, fr in (("compact", fc), (pads, ff)):
            assert torch.equal(fr[n].m, want), "%s: %s is not the exact result (%d of %d off, NaN: %d)" % (
                what, n, int((fr[n].m != want).sum()), want.numel(), int(torch.isnan(fr[n].m.float()).sum()))
    for n in written:                                                   # no case leaves a NaN or a 9 behind (outputs are written everywhere)
        if r["op"] == "ln_fwd" and not r["ln"] and n in ("y", "mean", "rstd"):
            continue
        m = ff[n].m.float()
        assert bool(torch.isfinite(m).all()), "%s holds a non-finite value" % n
    if r["op"] == "linear" and r["f32"] and r["epi"] & GELU:            # fp32 mode: erff of the device library, no exact form
        pre = ff["aux_out"].m
        ref = torch.nn.functional.gelu(pre.double()).float()
        assert bool(((ff["C"].m - ref).abs() <= 1e-5 * ref.abs() + 1e-6).all())
    if r["op"] == "ln_bwd":
        check_finalize(o, r, ff, dev)


def check_finalize(o, r, fr, dev):
    """gv_ln_finalize over the blocks the launch reported: its f32 atomics make the order of addition free, so the column sums are compared
    with the f64 sums of the same partials within blocks x 2^-24 x sum |partial| (each of the `blocks` additions rounds once)."""
    import torch
    p = fr["partials"].m.view(-1, 3, PN)
    blocks = p.shape[0]
    outs = [Frame(Operand(torch.ones(1, PN, device=dev), 0, written=True), PN) for _ in range(3)]
    o.ln_finalize(p, blocks, PN, outs[0].m, outs[1].m, outs[2].m)
    torch.cuda.synchronize()
    for w in range(3):
        assert outs[w].untouched()
        ref = 1.0 + p[:, w].double().sum(0)
        bound = (blocks + 1) * 2.0 ** -24 * (1.0 + p[:, w].double().abs().sum(0)) + 1e-30
        assert bool(((outs[w].m[0].double() - ref).abs() <= bound).all()), ("ln_finalize", w)


def main(argv):
    import torch
    from gipvit import _lib as L, ops as o
    dev = torch.device("cuda:0")
    ws = torch.empty(L.lib.gv_linear_workspace_bytes() // 4, dtype=torch.float32, device=dev)
    n = 0
    for r in cases():
        if r["group"] in argv:
            for pads in PADS:
                check(o, L, r, dev, ws, pads)
                n += 1
    print("OK %d checks, CU budget %d" % (n, CU_BUDGET))


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    main(sys.argv[1:])
