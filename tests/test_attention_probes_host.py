"""CPU: the exact probes of the attention forward / backward (csrc/attention.hip) -- input builders, closed-form fp64
references, the assertion functions the GPU file (tests/test_attention_probes_gpu.py) applies to the kernels' output, and a
"rounding-point model" of the kernel (fp64 with the kernel's bf16 / f32 roundings) that stands in for the kernel here.

The CPU tests below show, without a GPU, that (1) the constructions are exactly representable under the kernel's roundings and
their conditions (code distance) hold for every seed the GPU file uses, and (2) each assertion function rejects the model once
a subtle fault is put into it: a zero pad key counted in the softmax, the last key dropped, the last query missing from dK / dV,
the outputs of two (image, head) pairs swapped, the key index shifted by one inside the last partial 16-key tile.

Everything is kept pair-major: a case holds q, k, v, d_o [P, N, 64] and the references o, dq, dk, dv [P, N, 64], lse [P, N] as
float64 CPU tensors, P = n_img * H, pair = img * H + h; `pack_*` / `unpack_*` convert to and from the kernels' row layouts.

  probe A "selector": keys are +-4 codes, each query is one key's code -> its score beats every other by >= 32, P is a
                      permutation matrix to f32 precision: O, dV bit exact, lse = 128, dQ = dK ~ 0.
  probe B "tie":      keys come in pairs with one code (and free parts the zero-padded queries do not see) -> p = 1/2 each;
                      every value the kernel rounds has <= 8 significant bits, so fp64 IS the expected output, dQ / dK nonzero.
  probe C "uniform":  Q = 0 -> every real key scores what a zero pad key would score; lse = ln N.
  probe D "random":   randn data, lse against fp64 logsumexp within LSE_BOUND."""
import functools
import math

import pytest
import torch

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16

# every length-class edge of launch_fwd_any / gv_attention_bwd (N <= 32 / 64 / 128 / 224 / 288) and every ragged last tile
NS = (1, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 223, 224, 225, 287, 288)
F32_NS = (1, 17, 64, 65, 259, 260)              # the fp32 operand mode (N <= 260)
H, N_IMG, SCALE = 3, 3, 0.125                   # 9 pairs: a partial last workgroup for 2 and for 4 pairs per workgroup
MIN_DIST = 8                                    # code distance: score gap >= 4 * 8 = 32, exp(-32) = 1.3e-14

# Probe D: max |lse - fp64 logsumexp| of gv_attention_fwd measured on an MI355X over every N of NS (9 pairs each, the seeds
# below): 9.8e-7 (N = 223; 1.3e-7 at N = 1, 6.8e-7 at N = 64 -- mx * scale + __logf(sum) in f32 at |lse| <= 7, f32 ulp 4.8e-7).
# Bound = 4 x measured, for the seed-to-seed variation of the exp2 / __logf error.
# test_lse_bound_is_a_quarter_of_the_pad_key_shift holds it to 1/4 of the smallest shift one counted zero key causes (1.2e-3 at
# N = 288).
LSE_MEASURED = 9.8e-7
LSE_BOUND = 4 * LSE_MEASURED


def seed_of(probe, N, pair):
    """One seed per (probe, N, pair): no two pairs of a launch share data, so a pair mix-up cannot cancel."""
    return ("ABCD".index(probe) * 1000 + N) * 100 + pair


def _gen(probe, N, pair):
    return torch.Generator().manual_seed(seed_of(probe, N, pair))


def _nonzero_ints(g, shape):
    """integers in +-[1, 8] (a zero would let the other keys' ~1e-29 leakage show instead of an exact value)"""
    return (torch.randint(1, 9, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).to(f64)


def min_code_distance(codes):
    """smallest Hamming distance between two rows of a +-1 code matrix (inf for a single row)"""
    n, d = codes.shape
    if n < 2:
        return math.inf
    dist = (d - codes @ codes.t()) / 2
    dist.fill_diagonal_(math.inf)
    return float(dist.min())


def closed_form(q, k, v, d_o, P, scale):
    """Attention forward / backward for a GIVEN softmax matrix P [.., N, N] in fp64: o, dq, dk, dv."""
    o = P @ v
    dP = d_o @ v.transpose(-1, -2)
    delta = (d_o * o).sum(-1, keepdim=True)
    dS = P * (dP - delta) * scale
    return o, dS @ k, dS.transpose(-1, -2) @ q, P.transpose(-1, -2) @ d_o


def _stack(pairs):
    return {key: torch.stack([p[key] for p in pairs]) for key in pairs[0]}


# ------------------------------------------------------------------------------------------------------------ builders
def _selector_pair(N, pair):
    g = _gen("A", N, pair)
    codes = (torch.randint(0, 2, (N, 64), generator=g) * 2 - 1).to(f64)
    perm = torch.randperm(N, generator=g)
    v, d_o = _nonzero_ints(g, (N, 64)), _nonzero_ints(g, (N, 64))
    dv = torch.empty(N, 64, dtype=f64)
    dv[perm] = d_o                                                   # dV_j = dO_{perm^-1(j)}
    z = torch.zeros(N, 64, dtype=f64)
    return dict(q=4 * codes[perm], k=4 * codes, v=v, d_o=d_o, o=v[perm], lse=torch.full((N,), 128.0, dtype=f64), dq=z, dk=z.clone(), dv=dv,
                codes=codes, perm=perm)


def _tie_pair(N, pair):
    g = _gen("B", N, pair)
    T = (N + 1) // 2
    codes = (torch.randint(0, 2, (T, 48), generator=g) * 2 - 1).to(f64)
    grp_k = torch.arange(N) // 2                                      # keys (2t, 2t + 1) share code t; an odd N leaves one single key
    grp_q = torch.randperm(N, generator=g) // 2
    k = torch.cat([4 * codes[grp_k], torch.randint(-4, 5, (N, 16), generator=g).to(f64)], 1)
    q = torch.cat([4 * codes[grp_q], torch.zeros(N, 16, dtype=f64)], 1)
    v = torch.randint(1, 9, (T, 64), generator=g).to(f64)[grp_k]
    for j in range(1, N, 2):                                          # V_{2t+1} = V_{2t} + 2 in two random dimensions
        v[j, torch.randperm(64, generator=g)[:2]] += 2
    d_o = _nonzero_ints(g, (N, 64))
    same = (grp_q[:, None] == grp_k[None, :]).to(f64)
    size = same.sum(-1, keepdim=True)                                 # 2, or 1 for the single last key
    o, dq, dk, dv = closed_form(q, k, v, d_o, same / size, SCALE)
    return dict(q=q, k=k, v=v, d_o=d_o, o=o, lse=96.0 + size[:, 0].log(), dq=dq, dk=dk, dv=dv, codes=codes)


def _uniform_pair(N, pair):
    g = _gen("C", N, pair)
    k = torch.randn(N, 64, generator=g).to(bf16).to(f64)
    v = torch.randint(1, 9, (N, 64), generator=g).to(f64)
    d_o = _nonzero_ints(g, (N, 64))
    q = torch.zeros(N, 64, dtype=f64)
    o, dq, dk, dv = closed_form(q, k, v, d_o, torch.full((N, N), 1.0 / N, dtype=f64), SCALE)
    return dict(q=q, k=k, v=v, d_o=d_o, o=o, lse=torch.full((N,), math.log(N), dtype=f64), dq=dq, dk=dk, dv=dv)


def _random_pair(N, pair):
    g = _gen("D", N, pair)
    q, k, v, d_o = (torch.randn(N, 64, generator=g).to(bf16).to(f64) for _ in range(4))
    s = q @ k.t() * SCALE
    o, dq, dk, dv = closed_form(q, k, v, d_o, s.softmax(-1), SCALE)
    return dict(q=q, k=k, v=v, d_o=d_o, o=o, lse=torch.logsumexp(s, -1), dq=dq, dk=dk, dv=dv)


_BUILDERS = dict(A=_selector_pair, B=_tie_pair, C=_uniform_pair, D=_random_pair)


@functools.lru_cache(maxsize=None)
def build(probe, N, n_pairs=N_IMG * H):
    """The case of one probe at one length: inputs and fp64 references of `n_pairs` pairs.  Built once and shared -- read only."""
    case = _stack([_BUILDERS[probe](N, pair) for pair in range(n_pairs)])
    case.update(probe=probe, N=N)
    return case


# ------------------------------------------------------------------------------------- kernel row layouts <-> pair-major
def pack_qkv(case, n_img, H, dtype):
    """q, k, v [P, N, 64] -> the kernels' qkv [n_img * N, 3 * H * 64]"""
    N = case["N"]
    x = torch.stack([case["q"], case["k"], case["v"]], 2).view(n_img, H, N, 3, 64)
    return x.permute(0, 2, 3, 1, 4).reshape(n_img * N, 3 * H * 64).to(dtype)


def pack_rows(x, n_img, H, dtype):
    """[P, N, 64] -> [n_img * N, H * 64] (o, d_o)"""
    N = x.shape[1]
    return x.view(n_img, H, N, 64).permute(0, 2, 1, 3).reshape(n_img * N, H * 64).to(dtype)


def unpack_rows(t, n_img, H):
    N = t.shape[0] // n_img
    return t.detach().cpu().to(f64).reshape(n_img, N, H, 64).permute(0, 2, 1, 3).reshape(n_img * H, N, 64)


def unpack_dqkv(t, n_img, H):
    N = t.shape[0] // n_img
    x = t.detach().cpu().to(f64).reshape(n_img, N, 3, H, 64).permute(2, 0, 3, 1, 4).reshape(3, n_img * H, N, 64)
    return x[0], x[1], x[2]


def unpack_lse(t, n_img, H):
    return t.detach().cpu().to(f64).reshape(n_img * H, -1)


# --------------------------------------------------------------------------------------------------- assertion functions
def _ulp(x, mant_bits):
    """unit in the last place of |x| in a format with `mant_bits` explicit mantissa bits (23: f32, 7: bf16)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - mant_bits)


def _require(ok, what, case, got, ref):
    """`ok`: boolean [P, N] or [P, N, 64]; names the first failing (pair, row) -- a NaN fails (ok is built from <=, ==)"""
    if bool(ok.all()):
        return None
    rows = ~(ok if ok.dim() == 2 else ok.all(-1))
    pair, row = (int(i) for i in rows.nonzero()[0])
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    return (f"probe {case['probe']} N={case['N']}: {what}: {int(rows.sum())} of {rows.numel()} (pair, row) wrong, first pair {pair} "
            f"row {row} (pairs {sorted(set(rows.nonzero()[:, 0].tolist()))}), max |err| {float(err.max()):.4g}")


def _raise(failures):
    """every failing part of a probe in one error"""
    failures = [f for f in failures if f]
    assert not failures, "\n".join(failures)


def _within(got, ref, tol):
    return (got - ref).abs() <= tol


def check_selector(got, case, tol=None, parts=("o", "lse", "dq", "dk", "dv")):
    """probe A.  bf16 kernels (tol None): o and dv bit for bit, lse within 2 f32 ulp of 128 (the forward's f32 row sum is exactly
    1.0), |dq|, |dk| <= 1e-6 (not zero: bf16(dS) of the other keys is ~1e-12, not flushed).  `tol`: absolute, on everything
    (the fp32 operand mode)."""
    bad = []
    for name in parts:
        g, r = got[name], case[name]
        if tol is not None:
            ok = _within(g, r, tol)
        elif name in ("o", "dv"):
            # an entry whose reference is zero (dv of a key whose query is behind q_limit) holds the other keys' leakage instead
            ok = torch.where(r != 0, g == r, g.abs() <= 1e-6)
        elif name == "lse":
            ok = _within(g, r, 2 * 2.0 ** -16)
        else:
            ok = g.abs() <= 1e-6
        bad.append(_require(ok, name, case, g, r))
    _raise(bad)


def check_tie(got, case, tol=None, parts=("o", "lse", "dq", "dk", "dv")):
    """probe B: |got - ref| <= 1e-6 for o, dq, dk, dv (exact where the reference is nonzero: a bf16 value near 1/16 or above cannot be
    1e-6 off without being a different bf16 value; leakage tolerant where it is zero), lse within 4 f32 ulp.
    `tol`: absolute, on everything instead (the fp32 operand mode)."""
    bad = []
    for name in parts:
        g, r = got[name], case[name]
        if tol is not None:
            ok = _within(g, r, tol)
        elif name == "lse":
            ok = _within(g, r, 4 * _ulp(r, 23))
        else:
            ok = _within(g, r, 1e-6)
        bad.append(_require(ok, name, case, g, r))
    _raise(bad)


def check_uniform(got, case, parts=("o", "lse", "dk")):
    """probe C: |lse - ln N| <= 1e-5 (a counted pad key moves it by ln((N + 1) / N) >= 3.4e-3), o within 1 bf16 ulp of the mean of
    V, dk exactly zero (Q = 0)."""
    bad = []
    for name in parts:
        g, r = got[name], case[name]
        if name == "lse":
            ok = _within(g, r, 1e-5)
        elif name == "o":
            ok = _within(g, r, _ulp(r, 7))
        else:
            ok = g == 0
        bad.append(_require(ok, name, case, g, r))
    _raise(bad)


def check_random(got, case, parts=("o", "lse", "dq", "dk", "dv")):
    """probe D: lse within LSE_BOUND of the fp64 logsumexp; o and the gradients within the bf16 tolerances of test_attention_fwd_bwd
    (2e-2 + 2e-2 |ref| for o: bf16 P and bf16 output; 3e-2 |ref| + 2e-2 max(max |grad|, 1) for the gradients)."""
    gmax = max(float(torch.cat([case["dq"], case["dk"], case["dv"]]).abs().max()), 1.0)
    bad = []
    for name in parts:
        g, r = got[name], case[name]
        if name == "lse":
            ok = _within(g, r, LSE_BOUND)
        elif name == "o":
            ok = _within(g, r, 2e-2 + 2e-2 * r.abs())
        else:
            ok = _within(g, r, 2e-2 * gmax + 3e-2 * r.abs())
        bad.append(_require(ok, name, case, g, r))
    _raise(bad)


CHECKS = dict(A=check_selector, B=check_tie, C=check_uniform, D=check_random)


# --------------------------------------------------------------------------------------------------- rounding-point model
def rb(x):
    """round to bf16 (the kernel's (bf16) casts), kept as fp64"""
    return x.to(f32).to(bf16).to(f64)


def model(case, scale=SCALE, mutant=None, p_wobble=0.0):
    """The fp64 reference of attn_fwd_kernel + attn_bwd_kernel with the kernel's roundings: P rounded to bf16 before P V, the row
    sum taken in f32, O rounded to bf16, P recomputed from the f32 lse, dS rounded to bf16, outputs rounded to bf16.
    `mutant` puts one fault in:
      "pad_key"          one zero pad key (score 0, V = 0) is counted in the softmax
      "drop_last_key"    key N - 1 is masked out of the forward and the backward
      "drop_last_query"  query N - 1 is missing from the dK / dV sums
      "swap_pairs"       the outputs of pairs 1 and 2 change places
      "shift_last_tile"  P V reads row j + 1 of the (zero-padded) V image for every key j of the last partial 16-key tile
    `p_wobble`: relative error put on the backward's recomputed P (stands for the exp2 / __logf error)."""
    q, k, v, d_o, N = case["q"], case["k"], case["v"], case["d_o"], case["N"]
    s = q @ k.transpose(-1, -2) * scale
    sf, vf = s, v
    zrow = torch.zeros_like(v[:, :1])
    if mutant == "pad_key":
        sf, vf = torch.cat([s, torch.zeros_like(s[..., :1])], -1), torch.cat([v, zrow], 1)
    if mutant == "drop_last_key":
        sf = s.clone()
        sf[..., -1] = -math.inf
    if mutant == "shift_last_tile":
        idx = torch.arange(N)
        idx[(N - 1) // 16 * 16:] += 1
        vf = torch.cat([v, zrow], 1)[:, idx]
    mx = sf.max(-1, keepdim=True).values
    p = (sf - mx).exp()
    rsum = p.to(f32).sum(-1, keepdim=True).to(f64)
    o = rb(rb(p) @ vf / rsum)
    lse = (mx + rsum.log()).to(f32).to(f64)
    # backward, from the forward's o and lse
    p2 = (s - lse).exp() * (1.0 + p_wobble)
    if mutant == "drop_last_key":
        p2[..., -1] = 0.0
    delta = (o * d_o).sum(-1, keepdim=True).to(f32).to(f64)
    dS = p2 * ((d_o @ v.transpose(-1, -2)) * scale - delta * scale)
    pb, dsb = rb(p2), rb(dS)
    dq = rb(dsb @ k)
    if mutant == "drop_last_query":
        pb, dsb = pb.clone(), dsb.clone()
        pb[:, -1], dsb[:, -1] = 0.0, 0.0
    out = dict(o=o, lse=lse[..., 0], dq=dq, dk=rb(dsb.transpose(-1, -2) @ q), dv=rb(pb.transpose(-1, -2) @ d_o))
    if mutant == "swap_pairs":
        out = {name: x[[0, 2, 1] + list(range(3, x.shape[0]))] for name, x in out.items()}
    return out


def pad_key_shift(case):
    """by how much one counted zero key (score 0) raises each lse: ln(1 + exp(-lse))"""
    return torch.log1p((-case["lse"]).exp())


def _rejects(check, got, case):
    try:
        check(got, case)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------- CPU tests
ALL_NS = tuple(sorted(set(NS + F32_NS)))


@pytest.mark.parametrize("N", ALL_NS)
def test_probe_conditions_hold_for_every_seed_used(N):
    """min code distance >= 8 (score gap >= 32) for every (N, pair) the GPU file runs; the integer ranges of the constructions."""
    for probe, bits in (("A", 64), ("B", 48)):
        case = build(probe, N)
        for pair in range(N_IMG * H):
            assert min_code_distance(case["codes"][pair]) >= MIN_DIST, (probe, N, pair, seed_of(probe, N, pair))
        assert case["codes"].shape[-1] == bits
        for name in ("v", "d_o"):
            x = case[name]
            assert bool((x == x.round()).all()) and float(x.abs().min()) >= 1 and float(x.abs().max()) <= (8 if probe == "A" or name == "d_o" else 10)
    a = build("A", N)
    s = a["q"] @ a["k"].transpose(-1, -2) * SCALE
    assert float(s.max(-1).values.min()) == 128.0 and bool(((s == 128.0).sum(-1) == 1).all())
    assert float((128.0 - torch.where(s == 128.0, torch.full_like(s, -math.inf), s)).min()) >= 4 * MIN_DIST
    b = build("B", N)
    s = b["q"] @ b["k"].transpose(-1, -2) * SCALE
    assert float(s.max(-1).values.min()) == 96.0 and bool(((s == 96.0).sum(-1) <= 2).all())
    assert bool((b["q"][..., 48:] == 0).all()) and float(b["k"][..., 48:].abs().max()) <= 4
    # the tie probe is there for its nonzero dQ / dK
    if N > 1:
        assert float((b["dq"] != 0).double().mean()) > 0.1 and float((b["dk"] != 0).double().mean()) > 0.3
    c = build("C", N)
    assert bool((c["q"] == 0).all()) and bool((c["dk"] == 0).all())


@pytest.mark.parametrize("N", ALL_NS)
def test_model_reproduces_the_closed_forms(N):
    """The constructions are exactly representable: under the kernel's roundings the model gives the fp64 references of A and B to
    1e-12 (lse: to the f32 rounding of the value), with a 2e-5 relative error on the recomputed P (exp2 / __logf) changing nothing;
    the permutation gather of probe A equals the dense closed form."""
    for probe in "AB":
        case = build(probe, N)
        got = model(case)
        for name in ("o", "dq", "dk", "dv"):
            assert float((got[name] - case[name]).abs().max()) <= 1e-12, (probe, N, name)
        assert bool(((got["lse"] - case["lse"]).abs() <= _ulp(case["lse"], 23) / 2).all())
        CHECKS[probe](got, case)
        for wobble in (-2e-5, 2e-5):
            got = model(case, p_wobble=wobble)
            for name in ("dq", "dk", "dv"):
                assert float((got[name] - case[name]).abs().max()) <= 1e-12, (probe, N, name, wobble)
    a = build("A", N)
    P = torch.zeros(a["q"].shape[0], N, N, dtype=f64)
    P[torch.arange(P.shape[0])[:, None], torch.arange(N)[None, :], a["perm"]] = 1.0
    o, dq, dk, dv = closed_form(a["q"], a["k"], a["v"], a["d_o"], P, SCALE)
    assert torch.equal(o, a["o"]) and torch.equal(dv, a["dv"]) and float(dq.abs().max()) == 0 and float(dk.abs().max()) == 0
    for probe in "CD":
        CHECKS[probe](model(build(probe, N)), build(probe, N))


@pytest.mark.parametrize("N", NS)
def test_probes_reject_a_subtly_wrong_kernel(N):
    """Each fault, put into the model, is rejected by the assertion function the GPU file applies to the kernel."""
    a, b, c, d = (build(p, N) for p in "ABCD")
    assert _rejects(check_uniform, model(c, mutant="pad_key"), c)
    assert _rejects(check_random, model(d, mutant="pad_key"), d)
    for case, check in ((a, check_selector), (b, check_tie)):
        assert _rejects(check, model(case, mutant="drop_last_key"), case)           # (N = 1: no key left, NaN -- rejected too)
        assert _rejects(check, model(case, mutant="drop_last_query"), case)
        assert _rejects(check, model(case, mutant="swap_pairs"), case)
        # ... and each of them by the forward or the backward part alone where it acts there
        fwd_only = lambda got, cs, ck=check: ck(got, cs, parts=("o", "lse"))
        assert _rejects(fwd_only, model(case, mutant="swap_pairs"), case)
        bwd_only = lambda got, cs, ck=check: ck(got, cs, parts=("dq", "dk", "dv"))
        assert _rejects(bwd_only, model(case, mutant="drop_last_query"), case)
    assert _rejects(check_selector, model(a, mutant="shift_last_tile"), a)


def test_lse_bound_is_a_quarter_of_the_pad_key_shift():
    """LSE_BOUND (4 x the measured error) is at most 1/4 of the smallest lse shift one counted zero key causes at any row of any
    tested N on probe D's inputs."""
    shift = min(float(pad_key_shift(build("D", N)).min()) for N in NS)
    assert 1.0e-3 < shift < 2.0e-3                                   # ~1.3e-3, at N = 288
    assert LSE_BOUND == 4 * LSE_MEASURED and LSE_BOUND <= shift / 4


def _close_ok(got, ref, rtol, atol):
    """test_kernels_gpu.close as a predicate"""
    return bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())


def test_existing_tolerances_miss_the_pad_key_and_the_bound_catches_it():
    """Why LSE_BOUND exists: on the seeded randn inputs of test_attention_fwd_bwd at N = 288, a kernel that counts one zero pad key
    passes every assertion that test made before (o 2e-2 / 2e-2, lse 1e-3 / 1e-3, gradients 3e-2 / 2e-2 max |grad|), although it
    shifts every lse by more than 1e-3 (f32 lse is good to ~1e-5); the new lse bound rejects it."""
    N, Hh, n_img, scale = 288, 3, 3, 64 ** -0.5
    g = torch.Generator().manual_seed(N * 7 + Hh)
    qkv = torch.randn(n_img * N, 3 * Hh * 64, generator=g).to(bf16)
    d_o = torch.randn(n_img * N, Hh * 64, generator=g).to(bf16)
    q, k, v = unpack_dqkv(qkv, n_img, Hh)
    case = dict(q=q, k=k, v=v, d_o=unpack_rows(d_o, n_img, Hh), N=N, probe="D")
    s = q @ k.transpose(-1, -2) * scale
    case["o"], case["dq"], case["dk"], case["dv"] = closed_form(q, k, v, case["d_o"], s.softmax(-1), scale)
    case["lse"] = torch.logsumexp(s, -1)
    gmax = max(float(torch.cat([case["dq"], case["dk"], case["dv"]]).abs().max()), 1.0)

    def old_assertions(got):
        return (_close_ok(got["o"], case["o"], 2e-2, 2e-2) and _close_ok(got["lse"], case["lse"], 1e-3, 1e-3)
                and all(_close_ok(got[n], case[n], 3e-2, 2e-2 * gmax) for n in ("dq", "dk", "dv")))

    good, bad = model(case, scale), model(case, scale, mutant="pad_key")
    assert old_assertions(good) and not _rejects(check_random, good, case)
    assert float((bad["lse"] - case["lse"]).abs().min()) > 1.0e-3
    assert old_assertions(bad)
    assert _rejects(lambda got, cs: check_random(got, cs, parts=("lse",)), bad, case)


def test_layout_round_trip():
    case = build("D", 17)
    qkv = pack_qkv(case, N_IMG, H, bf16)
    assert qkv.shape == (N_IMG * 17, 3 * H * 64)
    q, k, v = unpack_dqkv(qkv, N_IMG, H)
    assert torch.equal(q, case["q"]) and torch.equal(k, case["k"]) and torch.equal(v, case["v"])
    assert torch.equal(unpack_rows(pack_rows(case["d_o"], N_IMG, H, bf16), N_IMG, H), case["d_o"])
    # pair = img * H + h sits at rows img * N .., columns h * 64 ..
    assert torch.equal(qkv.view(N_IMG, 17, 3, H, 64)[2, :, 1, 1].double(), case["k"][2 * H + 1])
