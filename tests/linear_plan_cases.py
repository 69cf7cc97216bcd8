"""The cases of tests/traces/linear_plans.json: how a fixture row becomes a call.

Shared by the recorder (tools/linear_plan_record.py), the CPU test (argument structs for gv_workspace_bytes, the case file of
tests/linear_plan_main.cc) and the GPU test (seeded integer operands, the call, the exact expectation).  A row holds the
arguments only; `kernel` and `bytes` are what the recorder saw at the commit the fixture was taken from."""
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "traces", "linear_plans.json")
BUDGETS = ("256", "248")                 # GIPVIT_CU_BUDGET unset (= 256) and a data-parallel run's 248
P0, P1 = 1 << 20, 2 << 20               # 16-byte aligned stand-ins for the scratch query: never dereferenced
BIAS, GELU, RESID, DGELU, ACCUM, POS, SAVE_PRE = 1, 2, 4, 8, 16, 32, 64


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def row_id(r):
    return r["id"]


# ---------------------------------------------------------------------------------------------- argument structs (no GPU)
def linear_args(L, r, ptr=None):
    """gv_linear_args of a `linear` row.  ptr: {field: address} of real buffers; without it aligned stand-ins."""
    e = r["epi"]
    a = L.gv_linear_args()
    p = ptr or {}
    a.A, a.B, a.C = p.get("A", P0), p.get("B", P0), p.get("C", P0)
    a.M, a.N, a.K = r["M"], r["N"], r["K"]
    a.lda = r["M"] if r["ta"] else r["K"]
    a.ldb = r["N"] if r["tb"] else r["K"]
    a.ldc = a.ldr = a.ld_aux = r["N"]
    a.trans_a, a.trans_b, a.c_is_f32, a.epilogue, a.alpha = r["ta"], r["tb"], r["c_f32"], e, 1.0
    if e & BIAS:
        a.bias = p.get("bias", P0)
    if e & RESID:
        a.resid = a.C if r["in_place"] else p.get("resid", P1)
    if e & DGELU:
        a.aux_in = p.get("aux_in", P0)
    if e & SAVE_PRE:
        a.aux_out = p.get("aux_out", P0)
    if r["colsum_a"]:
        a.colsum_a = p.get("colsum_a", P0)
    if r["ws"] and "ws" in p:
        a.workspace, a.workspace_bytes = p["ws"]
    return a


def group_args(L, r, bufs=None, ws=None):
    a = L.gv_linear_dw_group_args()
    a.n, a.K = len(r["probs"]), r["T"]
    for q, (m, n) in enumerate(r["probs"]):
        pr = a.prob[q]
        pr.dY, pr.X, pr.dW = bufs[q] if bufs else (P0, P0, P0)
        pr.M, pr.N, pr.ldy, pr.ldx, pr.ldw = m, n, m, n, n
    if ws:
        a.workspace, a.workspace_bytes = ws
    return a


def query_bytes(L, data):
    """gv_workspace_bytes of every linear and group row, in fixture order (the CU budget is the process's)."""
    import ctypes
    out = [L.lib.gv_workspace_bytes(L.OP_LINEAR, ctypes.byref(linear_args(L, r))) for r in data["linear"]]
    out += [L.lib.gv_workspace_bytes(L.OP_LINEAR_DW_GROUP, ctypes.byref(group_args(L, r))) for r in data["group"]]
    return out


def case_lines(data):
    """The case file of linear_plan_main: one line of integers per row."""
    lines = []
    for r in data["linear"]:
        lines.append("L %d %d %d %d %d %d %d %d %d %d" % (r["M"], r["N"], r["K"], r["ta"], r["tb"], r["c_f32"], r["epi"], r["colsum_a"], r["in_place"], r["ws"]))
    for r in data["group"]:
        lines.append("G %d %d " % (r["T"], len(r["probs"])) + " ".join("%d %d" % (m, n) for m, n in r["probs"]))
    for r in data["fullrow"]:
        lines.append("F %d %d %d" % ({"ln_fwd": 0, "ln_bwd": 1, "mlp_ln_fwd": 2}[r["op"]], r["M"], r["K"]))
    return lines


# ---------------------------------------------------------------------------------------------- the calls (GPU)
def ints(shape, dev, lo=-2, hi=3, seed=0):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).to(dev).to(torch.bfloat16)


def gelu_ref(v):
    """gv_common.h's gelu_f on f32 values, fused multiply-adds emulated in f64 (the product of two f32 is exact there)."""
    import torch
    f = lambda t: t.float().double()                                  # round to f32, carry on in f64
    x = v.double()
    xc = x.clamp(-4.0, 4.0)
    s = f(xc * xc)
    c = [float(torch.tensor(t, dtype=torch.float32)) for t in (-1.9031826664e-09, 1.4105862408e-07, -4.5653132491e-06, 8.6345539916e-05,
                                                                -1.085383136e-03, 9.7898487455e-03, -6.6360631345e-02, 3.9892696491e-01)]
    q = f(c[0] * s + c[1])
    for ck in c[2:]:
        q = f(q * s + ck)
    return (x * f(xc * q + 0.5)).float()


def dgelu_ref(v):
    """gv_common.h's dgelu_f on f32 values, emulated like gelu_ref."""
    import torch
    f = lambda t: t.float().double()
    xd = v.double().clamp(-4.0, 4.0)
    s = f(xd * xd)
    c = [float(torch.tensor(t, dtype=torch.float32)) for t in (-1.154122852e-11, 1.5301791658e-09, -8.8285028494e-08, 2.9218555444e-06, -6.1681373513e-05,
                                                                8.7549978582e-04, -8.5804168959e-03, 5.8243992531e-02, -2.6485431579e-01, 7.9775551922e-01)]
    r = f(c[0] * s + c[1])
    for ck in c[2:]:
        r = f(r * s + ck)
    return f(xd * r + 0.5).float()


def timed(o, fn):
    """fn() between linear_timing(True) and (False): the timing rows."""
    o.linear_timing(True)
    try:
        fn()
    finally:
        o.linear_timing(False)
    return o.linear_timing_read()


def run_linear(o, L, r, dev, ws):
    """One `linear` row on seeded integers: (timing rows, list of (what, got, expected) that must be equal)."""
    import torch
    f32, b16 = torch.float32, torch.bfloat16
    M, N, K, e = r["M"], r["N"], r["K"], r["epi"]
    lo, hi = (-1, 2) if K > 2048 else (-2, 3)                          # long reductions: the range of test_linear_tn_exact
    A = ints((K, M) if r["ta"] else (M, K), dev, lo, hi, seed=51)
    B = ints((K, N) if r["tb"] else (N, K), dev, lo, hi, seed=52)
    opA, opB = (A.float().t() if r["ta"] else A.float()), (B.float() if r["tb"] else B.float().t())
    v = opA @ opB
    checks = []
    out_t = f32 if r["c_f32"] else b16
    C = torch.full((M + 1, N), 9.0, dtype=out_t, device=dev)          # one guard row behind the output
    kw = dict(trans_a=bool(r["ta"]), trans_b=bool(r["tb"]), epilogue=e)
    if e & BIAS:
        kw["bias"] = torch.arange(N, dtype=f32, device=dev) % 5 - 2
        v = v + kw["bias"]
    if e & SAVE_PRE:
        kw["aux_out"] = torch.full((M + 1, N), 9.0, dtype=b16, device=dev)
        checks.append(("pre", kw["aux_out"], torch.cat([v.to(b16), torch.full((1, N), 9.0, dtype=b16, device=dev)])))
    if e & GELU:
        v = gelu_ref(v)
    if e & DGELU:
        kw["aux_in"] = torch.zeros(M, N, dtype=b16, device=dev)       # gelu'(0) = 1/2 exactly
        v = v * 0.5
    if e & RESID:
        resid = (torch.arange(M * N, device=dev) % 7 - 3).to(f32).view(M, N)
        if r["in_place"]:
            C[:M] = resid
            kw["resid"] = C
        else:
            kw["resid"] = resid
        v = v + resid
    if e & ACCUM:
        C[:M] = 1.0
        v = v + 1.0
    if r["colsum_a"]:
        kw["colsum_a"] = torch.full((M,), 2.0, dtype=f32, device=dev)
        checks.append(("colsum_a", kw["colsum_a"], 2.0 + A.float().sum(0)))
    if r["ws"]:
        kw["workspace"] = ws
    rows = timed(o, lambda: o.linear(A, B, C, M, N, K, **kw))
    checks.append(("C", C, torch.cat([v.to(out_t), torch.full((1, N), 9.0, dtype=out_t, device=dev)])))
    return rows, checks


def run_group(o, L, r, dev, ws):
    import torch
    f32 = torch.float32
    T = r["T"]
    probs, checks = [], []
    for q, (m, n) in enumerate(r["probs"]):
        dY, X = ints((T, m), dev, -1, 2, seed=60 + q), ints((T, n), dev, -1, 2, seed=70 + q)
        dW = torch.full((m, n), float(q), dtype=f32, device=dev)
        cs = torch.full((m,), 2.0, dtype=f32, device=dev) if q % 2 == 0 else None
        probs.append((dY, X, dW, cs))
        checks.append(("dW%d" % q, dW, q + dY.float().t() @ X.float()))
        if cs is not None:
            checks.append(("colsum%d" % q, cs, 2.0 + dY.float().sum(0)))
    rows = timed(o, lambda: o.linear_dw_group(probs, T, ws))
    return rows, checks


def run_fullrow(o, L, r, dev):
    """The full-row entry points: the kernel is what the row pins.  gv_linear_ln_fwd without LayerNorm outputs is exact on integers;
    the other two have no exact form (tests/test_kernels_gpu.py holds their tolerances) -- finite outputs only."""
    import torch
    f32, b16 = torch.float32, torch.bfloat16
    M, K, N = r["M"], r["K"], 384
    if r["op"] == "ln_fwd":
        A, W = ints((M, K), dev, seed=81), ints((N, K), dev, seed=82)
        out = torch.full((M + 1, N), 9.0, dtype=f32, device=dev)
        rows = timed(o, lambda: o.linear_ln_fwd(A, W, out, M, K))
        return rows, [("out", out, torch.cat([A.float() @ W.float().t(), torch.full((1, N), 9.0, device=dev)]))]
    if r["op"] == "mlp_ln_fwd":
        A, W1, W2 = ints((M, K), dev, seed=83), ints((4 * K, K), dev, -1, 2, seed=84), ints((N, 4 * K), dev, -1, 2, seed=85)
        b1 = torch.zeros(4 * K, dtype=f32, device=dev)
        out = torch.empty(M, N, dtype=f32, device=dev)
        rows = timed(o, lambda: o.mlp_ln_fwd(A, W1, b1, W2, out, M, K, 4 * K))
        return rows, [("finite", torch.isfinite(out).all(), torch.tensor(True, device=dev))]
    dY, W = ints((M, K), dev, seed=86), ints((K, N), dev, seed=87)
    g = torch.Generator().manual_seed(88)
    x = torch.randn(M, N, generator=g).to(dev)
    gamma, beta = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    _, mean, rstd = o.layernorm_fwd(x, gamma, beta, M, N)
    gbuf = torch.zeros(M, N, dtype=f32, device=dev); gb = torch.empty(M, N, dtype=b16, device=dev)
    partials = torch.empty(L.LN_PARTIAL_BLOCKS, 3, N, dtype=f32, device=dev)
    rows = timed(o, lambda: o.linear_ln_bwd(dY, W, x, mean, rstd, gamma, gbuf, gb, partials, M, K))
    return rows, [("finite", torch.isfinite(gbuf).all(), torch.tensor(True, device=dev))]


def run_row(o, L, kind, r, dev, ws):
    if kind == "linear":
        return run_linear(o, L, r, dev, ws)
    if kind == "group":
        return run_group(o, L, r, dev, ws)
    return run_fullrow(o, L, r, dev)
