"""Sinkhorn-Knopp centring and KoLeo: the specification in numpy, shared by tests/test_dinov2_terms_host.py and _gpu.py.

* ``sinkhorn_log``: the log-domain iteration of include/gipvit.h in a chosen dtype (float64: the reference; float32: the same
  passes as the kernels form them, whose distance from float64 sizes the GPU bounds); ``ranks`` > 1 splits the rows and adds the
  ranks' column sums, as the data-parallel engine does.
* ``sinkhorn_literal``: DINOv2's ``sinkhorn_knopp_teacher`` on Q = exp(T / tau)^T, restated with every scalar constant it carries.
* ``koleo`` / ``koleo_grad``: forward and the hand-derived backward, numpy in a chosen dtype.
* the fixed inputs of the GPU cases and ``bound``: 8 x the float32 restatement's deviation from float64 on those inputs (the factor
  covers another summation order in the kernel), never below 1e-6 absolute."""
import functools

import numpy as np

EPS = 1e-8
FLT_MIN = float(np.finfo(np.float32).tiny)

# (R, K): the issue's four, then the edges of the kernels' splits.  The column pass tiles K by 1024 and slices the rows so that
# tiles x slices reaches 1024 workgroups (K <= 1024: one row per slice; K = 5120: at most 205 slices, so R = 409 gives 204 slices of
# two rows and one of one, R = 410 205 full ones, R = 411 137 of three); the row pass takes 256 threads below K = 8192 and 1024
# from there on; the shift pass strides 1024 workgroups of 1024 elements (R K = 2^20 + 4: the first workgroup takes a second trip).
SINKHORN_CASES = [(2, 256), (6, 1028), (130, 4096), (128, 65536),
                  (3, 1020), (3, 1024), (409, 5120), (410, 5120), (411, 5120), (5, 8188), (5, 8192), (5, 8196), (1, 1048580), (257, 4)]
SINKHORN_BIG = (128, 65536)
TAUS, ITERS = (0.04, 0.07), (1, 3)
KOLEO_CASES = [(2, 2, 192), (2, 5, 384), (2, 64, 384), (1, 130, 768), (2, 512, 192)]
KOLEO_GAP = 1e-3


def bf16_round(x):
    """float32 array rounded to the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=4)
def sinkhorn_logits(R, K, d=32):
    """T = z W^T of unit rows, float32: cosines, like the weight-normalised last layer's output."""
    rng = np.random.Generator(np.random.PCG64([R, K]))
    z = rng.standard_normal((R, d)); z /= np.linalg.norm(z, axis=1, keepdims=True)
    W = rng.standard_normal((K, d)); W /= np.linalg.norm(W, axis=1, keepdims=True)
    return (z @ W.T).astype(np.float32)


def sinkhorn_log(T, tau, n, dtype=np.float64, ranks=1):
    """-> (a [K] = log u, min over the passes of min_k s_k).  float32: logit * (1 / tau) rounded on its own, as the kernels do."""
    T = np.asarray(T).astype(dtype)
    x = T * (dtype(1) / dtype(tau)) if dtype == np.float32 else T / dtype(tau)
    shift = x.max()
    a, b = np.zeros(T.shape[1], dtype), np.zeros(T.shape[0], dtype)
    parts = np.array_split(np.arange(T.shape[0]), ranks)
    s_min = np.inf
    for it in range(n):
        s = np.zeros(T.shape[1], dtype)
        for rows in parts:
            s += np.exp(((x[rows] - shift) + a[None, :]) + b[rows, None]).sum(0, dtype=dtype)
        s_min = min(s_min, float(s.min()))
        a = a - np.log(np.maximum(s, dtype(FLT_MIN)))
        if it < n - 1:
            b = -np.log(np.exp((x - shift) + a[None, :]).sum(1, dtype=dtype))
    return a, s_min


def sinkhorn_probs(T, tau, a):
    """softmax((T - c) / tau) with c = -tau a, float64: the teacher probabilities gv_dino_loss forms from sk_center."""
    x = np.asarray(T, np.float64) / tau + np.asarray(a, np.float64)[None, :]
    x -= x.max(1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(1, keepdims=True)


def sinkhorn_literal(T, tau, n, world=1):
    """DINOv2's sinkhorn_knopp_teacher in float64, constants and all -> Q [R, K] (rows sum to 1)."""
    Q = np.exp(np.asarray(T, np.float64) / tau).T
    B, K = Q.shape[1] * world, Q.shape[0]
    Q /= Q.sum()
    for _ in range(n):
        Q /= Q.sum(1, keepdims=True)
        Q /= K
        Q /= Q.sum(0, keepdims=True)
        Q /= B
    Q *= B
    return Q.T


def gauge(c):
    """A centre is defined up to a constant (the softmax drops it): compare after subtracting the mean."""
    c = np.asarray(c, np.float64)
    return c - c.mean()


@functools.lru_cache(maxsize=64)
def sinkhorn_reference(R, K, tau, n):
    """-> (gauged float64 centre, bound on the gauged centre, min s_k) of a GPU case."""
    T = sinkhorn_logits(R, K)
    a64, s_min = sinkhorn_log(T, tau, n)
    a32, _ = sinkhorn_log(T, tau, n, np.float32)
    c64, c32 = gauge(-tau * a64), gauge(-np.float32(tau) * a32)
    return c64, bound(c32, c64), s_min


def bound(x32, x64):
    return max(8.0 * float(np.abs(np.asarray(x32, np.float64) - np.asarray(x64, np.float64)).max()), 1e-6)


# ------------------------------------------------------------------------------------------------------------------------- KoLeo
@functools.lru_cache(maxsize=8)
def koleo_inputs(G, B, D):
    """Features [G * B + 3, D] (three rows past the crops: a local crop's, which KoLeo must leave alone), bfloat16-representable
    float32.  A crop is made of clusters of three rows (the last takes the remainder) at noise 0 / 0.25 / 0.45 / 0.6 around a common
    direction: every row's nearest neighbour is clear (test_dinov2_terms_host.py holds the gap), several rows share one."""
    rng = np.random.Generator(np.random.PCG64([G, B, D]))
    x = np.empty((G * B + 3, D))
    sig = (0.0, 0.25, 0.45, 0.6, 0.75)
    for g in range(G):
        n_cl = max(B // 3, 1)
        for i in range(B):
            m = min(i // 3, n_cl - 1)
            if i - 3 * m == 0:
                c = rng.standard_normal(D)
            x[g * B + i] = (c + sig[i - 3 * m] * rng.standard_normal(D)) * (0.5 + 1.5 * rng.random())
    x[G * B:] = rng.standard_normal((3, D))
    return bf16_round(x.astype(np.float32))


def koleo(x, G, B, dtype=np.float64, nn=None):
    """x [>= G * B, D] -> dict(y, inv, nn [G * B] within the crop, gap [G * B] best-minus-runner-up dot, d, koleo)."""
    x = np.asarray(x)[:G * B].astype(dtype)
    eps = dtype(EPS)
    nrm = np.maximum(np.sqrt((x * x).sum(1, dtype=dtype)), eps)
    y = x / nrm[:, None]
    out_nn, gap, d = np.zeros(G * B, np.int64), np.full(G * B, np.inf), np.zeros(G * B, dtype)
    total = dtype(0)
    for g in range(G):
        yc = y[g * B:(g + 1) * B]
        dots = yc @ yc.T
        np.fill_diagonal(dots, -np.inf)
        I = dots.argmax(1) if nn is None else np.asarray(nn[g * B:(g + 1) * B])
        if B > 2:
            top = np.sort(dots, axis=1)
            gap[g * B:(g + 1) * B] = top[:, -1] - top[:, -2]
        delta = yc - yc[I] + eps
        dg = np.sqrt((delta * delta).sum(1, dtype=dtype))
        out_nn[g * B:(g + 1) * B], d[g * B:(g + 1) * B] = I, dg
        total = total + (-np.log(dg + eps)).sum(dtype=dtype) / dtype(B)
    return dict(y=y, inv=dtype(1) / nrm, nn=out_nn, gap=gap, d=d, koleo=total)


def koleo_grad(x, G, B, nn, dtype=np.float64):
    """d koleo / d x [G * B, D] with the neighbours ``nn`` held constant: the formulas of include/gipvit.h."""
    f = koleo(x, G, B, dtype, nn=nn)
    y, d, eps = f["y"], f["d"], dtype(EPS)
    gx = np.zeros_like(y)
    for g in range(G):
        sl = slice(g * B, (g + 1) * B)
        yc, I = y[sl], np.asarray(nn[sl])
        w = dtype(1) / (dtype(B) * d[sl] * (d[sl] + eps))
        delta = yc - yc[I] + eps
        gy = -w[:, None] * delta
        np.add.at(gy, I, w[:, None] * delta)
        gx[sl] = (gy - yc * (yc * gy).sum(1, keepdims=True)) * f["inv"][sl, None]
    return gx


@functools.lru_cache(maxsize=8)
def koleo_reference(G, B, D):
    """-> dict of a GPU case: x, the float64 forward and gradient, and the bounds on koleo and gx."""
    x = koleo_inputs(G, B, D)
    f64 = koleo(x, G, B)
    f32 = koleo(x, G, B, np.float32, nn=f64["nn"])
    g64 = koleo_grad(x, G, B, f64["nn"])
    g32 = koleo_grad(x, G, B, f64["nn"], np.float32)
    return dict(x=x, fwd=f64, gx=g64, koleo_bound=bound(f32["koleo"], f64["koleo"]), gx_bound=bound(g32, g64))
