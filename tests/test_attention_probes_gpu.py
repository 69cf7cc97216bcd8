"""GPU: gv_attention_fwd / gv_attention_bwd (and their varlen, q_limit and fp32-operand entry points) on the exact probes of
tests/test_attention_probes_host.py, at every length-class edge (N <= 32 / 64 / 128 / 224 / 288) and every ragged last tile.
The host file owns the builders, the fp64 references and the assertion functions -- and shows on the CPU that those functions
reject a subtly wrong kernel.  A failure names the probe, N, the (image, head) pair and the row.  Every output buffer has a
sentinel-filled guard region behind it that must stay untouched."""
import pytest
import torch

from test_attention_probes_host import (CHECKS, F32_NS, H, LSE_BOUND, N_IMG, NS, SCALE, build, check_random, check_selector, pack_qkv,
                                        pack_rows, unpack_dqkv, unpack_lse, unpack_rows)

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
GUARD, SENT = 8, -768.0                    # guard rows behind every output buffer, and what they (and untouched rows) hold
NAMES = ("o", "lse", "dq", "dk", "dv")


def ops():
    from gipvit import ops as o
    return o


def _guarded(rows, cols, dtype, dev):
    buf = torch.full(((rows + GUARD) * cols,), SENT, dtype=dtype, device=dev)
    return buf, buf[:rows * cols].view(rows, cols)


def _guards_untouched(*bufs_and_views):
    for buf, view in bufs_and_views:
        assert bool((buf[view.numel():] == SENT).all()), "a kernel wrote behind its output buffer"


class Segment:
    """one (n_img, N) block of a token-concatenated row space: inputs on the device, guarded outputs"""

    def __init__(self, dev, case, n_img, H, dtype, d_o=None):
        self.case, self.n_img, self.H, self.N = case, n_img, H, case["N"]
        self.qkv = pack_qkv(case, n_img, H, dtype).to(dev)
        self.d_o = pack_rows(case["d_o"] if d_o is None else d_o, n_img, H, dtype).to(dev)
        self.lbuf, lse = _guarded(n_img * H, self.N, f32, dev)
        self.lse = lse.view(n_img, H, self.N)

    def result(self, out, dqkv):
        dq, dk, dv = unpack_dqkv(dqkv, self.n_img, self.H)
        return dict(o=unpack_rows(out, self.n_img, self.H), lse=unpack_lse(self.lse, self.n_img, self.H), dq=dq, dk=dk, dv=dv)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def run(dev, case, n_img=N_IMG, H=H, dtype=bf16, q_limit=0, d_o=None):
    """forward + backward (from the forward's own o / lse) of one case through gv_attention_fwd / gv_attention_bwd.  Under
    q_limit everything the header says is neither written nor read is NaN: o / lse are NaN-filled before the forward, the rows
    behind ceil32(q_limit) must keep that bit pattern, the backward runs on those NaN-tailed o / lse (as the limited forward
    leaves them in the engine) and on a dO whose rows behind ceil32(q_limit) are NaN too (a finite sentinel times the zero dO
    would hide a read)."""
    o, sg = ops(), Segment(dev, case, n_img, H, dtype, d_o)
    T = n_img * sg.N
    obuf, out = _guarded(T, H * 64, dtype, dev)
    gbuf, dqkv = _guarded(T, 3 * H * 64, dtype, dev)
    qe = min(sg.N, (q_limit + 31) // 32 * 32) if q_limit else sg.N
    if q_limit:
        out.fill_(float("nan")); sg.lse.fill_(float("nan"))
        sg.d_o.view(n_img, sg.N, H * 64)[:, qe:] = float("nan")
    o.attention_fwd(sg.qkv, n_img, sg.N, H, SCALE, o=out, lse=sg.lse, q_limit=q_limit)
    if qe < sg.N:
        ov, lv = out.view(n_img, sg.N, H * 64)[:, qe:], sg.lse[:, :, qe:]
        assert torch.equal(_bits(ov), _bits(_nan_like(ov))) and torch.equal(_bits(lv), _bits(_nan_like(lv))), "forward wrote behind q_limit"
    o.attention_bwd(sg.qkv, out, sg.d_o, sg.lse, n_img, sg.N, H, SCALE, dqkv=dqkv, q_limit=q_limit)
    _guards_untouched((obuf, out), (gbuf, dqkv), (sg.lbuf, sg.lse))
    res = sg.result(out, dqkv)
    res["dqkv_raw"] = dqkv.clone()
    return res


def run_varlen(dev, cases, n_imgs, H=H):
    """the segments `cases` as one token-concatenated row space through gv_attention_fwd_varlen / gv_attention_bwd_varlen"""
    o = ops()
    segs = [Segment(dev, case, n, H, bf16) for case, n in zip(cases, n_imgs)]
    T = sum(s.n_img * s.N for s in segs)
    qkv, d_o = torch.cat([s.qkv for s in segs]), torch.cat([s.d_o for s in segs])
    obuf, out = _guarded(T, H * 64, bf16, dev)
    gbuf, dqkv = _guarded(T, 3 * H * 64, bf16, dev)
    table = [(s.n_img, s.N, s.lse) for s in segs]
    o.attention_fwd_varlen(qkv, out, table, H, SCALE)
    o.attention_bwd_varlen(qkv, out, d_o, dqkv, table, H, SCALE)
    _guards_untouched((obuf, out), (gbuf, dqkv), *[(s.lbuf, s.lse) for s in segs])
    res, row = [], 0
    for s in segs:
        r = slice(row, row + s.n_img * s.N)
        res.append(s.result(out[r], dqkv[r]))
        row = r.stop
    return res


def _rows(d, sl):
    """the rows `sl` of every per-row entry of a case or a result"""
    return {k: (v[:, sl] if k in NAMES else v) for k, v in d.items()}


# ----------------------------------------------------------------------------------- A - D at every length-class edge
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("probe", "ABCD")
def test_probe(dev, probe, N):
    """Probes A (selector: O, dV bit exact), B (two-key tie: exact nonzero dQ, dK), C (uniform: a counted pad key moves lse) and
    D (randn: lse within LSE_BOUND of fp64 logsumexp on the CPU) through the bf16 forward and backward.
    D, measured on an MI355X over all N: max |lse - ref| = 9.8e-7 (N = 223); LSE_BOUND = 4 x that = 3.9e-6."""
    case = build(probe, N)
    got = run(dev, case)
    if probe == "D":
        print(f"probe D N={N}: max |lse - fp64 logsumexp| = {float((got['lse'] - case['lse']).abs().max()):.3e} (bound {LSE_BOUND:.3e})")
    CHECKS[probe](got, case)


# ------------------------------------------------------------------------------------ E: replication invariance (bitwise)
def _replicated(dev, case1, n_img, H):
    """pair 0 of `case1` copied into every (image, head) pair: qkv [n_img N, 3 H 64], d_o [n_img N, H 64]"""
    N = case1["N"]
    x = torch.stack([case1["q"][0], case1["k"][0], case1["v"][0]], 1).to(bf16).to(dev)            # [N, 3, 64]
    qkv = x[None, :, :, None, :].expand(n_img, N, 3, H, 64).reshape(n_img * N, 3 * H * 64)
    d_o = case1["d_o"][0].to(bf16).to(dev)[None, :, None, :].expand(n_img, N, H, 64).reshape(n_img * N, H * 64)
    return qkv, d_o


def _all_pairs_equal_pair0(what, t, n_img, H, lse=False):
    """bit for bit; t: [n_img N, C H 64] rows (C = 1 or 3), or lse [n_img, H, N]"""
    if lse:
        x = t.reshape(n_img * H, -1).view(torch.int32)
    else:
        N = t.shape[0] // n_img
        x = t.view(n_img, N, -1, H, 64).permute(0, 3, 1, 2, 4).reshape(n_img * H, -1).view(torch.int16)
    bad = (x != x[:1]).any(-1).nonzero()[:, 0].tolist()
    assert not bad, f"{what}: {len(bad)} of {n_img * H} pairs differ from pair 0, first (image, head) {[divmod(p, H) for p in bad[:8]]}"


@pytest.mark.parametrize("N", [17, 33, 64, 129, 224, 288])
def test_replicated_pairs_are_bit_equal(dev, N):
    """One pair's randn data in every pair of a launch that exceeds one resident round of workgroups (an odd pair count: a partial
    last workgroup): o, lse and dqkv of every pair equal pair 0 bit for bit (no atomics in these kernels) -- a wave reading another
    pair's LDS slot, a stale dS^T image or a missing barrier shows as a difference.  Pair 0 itself is held to probe D's bounds."""
    o = ops()
    n_img, Hh = (205, 5) if N <= 64 else (171, 3)                      # 1025 / 513 pairs
    case1 = build("D", N, 1)
    qkv, d_o = _replicated(dev, case1, n_img, Hh)
    T = n_img * N
    obuf, out = _guarded(T, Hh * 64, bf16, dev)
    gbuf, dqkv = _guarded(T, 3 * Hh * 64, bf16, dev)
    lbuf, lse = _guarded(n_img * Hh, N, f32, dev)
    lse = lse.view(n_img, Hh, N)
    o.attention_fwd(qkv, n_img, N, Hh, SCALE, o=out, lse=lse)
    o.attention_bwd(qkv, out, d_o, lse, n_img, N, Hh, SCALE, dqkv=dqkv)
    _guards_untouched((obuf, out), (gbuf, dqkv), (lbuf, lse))
    _all_pairs_equal_pair0(f"N={N} o", out, n_img, Hh)
    _all_pairs_equal_pair0(f"N={N} lse", lse, n_img, Hh, lse=True)
    _all_pairs_equal_pair0(f"N={N} dqkv", dqkv, n_img, Hh)
    dq, dk, dv = unpack_dqkv(dqkv[:N, :3 * Hh * 64].reshape(N, 3, Hh, 64)[:, :, 0].reshape(N, 192), 1, 1)
    got0 = dict(o=unpack_rows(out[:N, :64], 1, 1), lse=lse[0, :1].cpu().to(f64), dq=dq, dk=dk, dv=dv)
    check_random(got0, case1)


@pytest.mark.parametrize("n_long,n_short", [(129, 33), (224, 64)])
def test_replicated_pairs_are_bit_equal_varlen(dev, n_long, n_short):
    """The same through the fused long + short varlen launch (two 4-wave short instances per workgroup; 1029 short pairs = 1 mod 4
    leave the last workgroup one pair of four): every long pair equals long pair 0, every short pair short pair 0."""
    o = ops()
    shapes = ((171, n_long), (343, n_short))
    data = [_replicated(dev, build("D", N, 1), n, H) for n, N in shapes]
    qkv, d_o = torch.cat([d[0] for d in data]), torch.cat([d[1] for d in data])
    T = qkv.shape[0]
    obuf, out = _guarded(T, H * 64, bf16, dev)
    gbuf, dqkv = _guarded(T, 3 * H * 64, bf16, dev)
    lses = [_guarded(n * H, N, f32, dev) for n, N in shapes]
    table = [(n, N, l[1].view(n, H, N)) for (n, N), l in zip(shapes, lses)]
    o.attention_fwd_varlen(qkv, out, table, H, SCALE)
    o.attention_bwd_varlen(qkv, out, d_o, dqkv, table, H, SCALE)
    _guards_untouched((obuf, out), (gbuf, dqkv), *lses)
    row = 0
    for n, N, lse in table:
        r = slice(row, row + n * N)
        _all_pairs_equal_pair0(f"varlen N={N} o", out[r], n, H)
        _all_pairs_equal_pair0(f"varlen N={N} lse", lse, n, H, lse=True)
        _all_pairs_equal_pair0(f"varlen N={N} dqkv", dqkv[r], n, H)
        ref_o, ref_lse = o.attention_fwd(qkv[r], n, N, H, SCALE)                  # ... and pair 0 is what the plain launch gives
        assert torch.equal(out[r][:N], ref_o[:N]) and torch.equal(lse[0], ref_lse[0])
        row = r.stop


# ------------------------------------------------------------------------------------ F: A - C on the other entry points
@pytest.mark.parametrize("order", ["long-short", "short-long"])
@pytest.mark.parametrize("n_long,n_short", [(129, 33), (224, 64)])
@pytest.mark.parametrize("probe", "AB")
def test_probe_varlen(dev, probe, n_long, n_short, order):
    """Probes A and B per segment through gv_attention_fwd_varlen (the fused long + short launch; 9 short pairs: the last workgroup
    holds one of four) and gv_attention_bwd_varlen, either segment order."""
    lens = (n_long, n_short) if order == "long-short" else (n_short, n_long)
    cases = [build(probe, N) for N in lens]
    for got, case in zip(run_varlen(dev, cases, (N_IMG, N_IMG)), cases):
        CHECKS[probe](got, case)


@pytest.mark.parametrize("n_a,n_b", [(128, 64), (225, 64), (224, 32), (224, 65)])
def test_varlen_just_outside_the_fused_window(dev, n_a, n_b):
    """Two segments one token class off the long + short pair that shares a launch (csrc/attn_plan.h VarlenCfg::fuses): the call
    runs one launch per segment, so o and lse of ONE gv_attention_fwd_varlen call equal the per-segment gv_attention_fwd calls bit
    for bit -- and at (225, 64) dqkv of one gv_attention_bwd_varlen call the per-segment gv_attention_bwd calls.  Probe A, 3 x 3
    pairs per segment (every N here is held to probe A's own checks by test_probe)."""
    o = ops()
    segs = [Segment(dev, build("A", N), N_IMG, H, bf16) for N in (n_a, n_b)]
    T = sum(s.n_img * s.N for s in segs)
    qkv, d_o = torch.cat([s.qkv for s in segs]), torch.cat([s.d_o for s in segs])
    obuf, out = _guarded(T, H * 64, bf16, dev)
    gbuf, dqkv = _guarded(T, 3 * H * 64, bf16, dev)
    table = [(s.n_img, s.N, s.lse) for s in segs]
    o.attention_fwd_varlen(qkv, out, table, H, SCALE)
    if (n_a, n_b) == (225, 64):
        o.attention_bwd_varlen(qkv, out, d_o, dqkv, table, H, SCALE)
    _guards_untouched((obuf, out), (gbuf, dqkv), *[(s.lbuf, s.lse) for s in segs])
    row = 0
    for s in segs:
        r = slice(row, row + s.n_img * s.N)
        ref_o, ref_lse = o.attention_fwd(qkv[r], s.n_img, s.N, H, SCALE)
        assert torch.equal(out[r], ref_o) and torch.equal(s.lse, ref_lse), f"forward, segment N={s.N}"
        if (n_a, n_b) == (225, 64):
            ref_g = o.attention_bwd(qkv[r], ref_o, d_o[r], ref_lse, s.n_img, s.N, H, SCALE)
            assert torch.equal(dqkv[r], ref_g), f"backward, segment N={s.N}"
        row = r.stop


@pytest.mark.parametrize("N", [33, 225, 288])
@pytest.mark.parametrize("ql", [1, 32, 33])
def test_probe_q_limit(dev, ql, N):
    """Probe A under q_limit: the forward's rows < min(N, ceil32(q_limit)) are exact, the rest untouched (NaN before and after, bit
    for bit); the backward with dO zero behind q_limit and NaN behind ceil32(q_limit), on the NaN-tailed o / lse: dV exact (dO of
    the matching query, ~0 for a key whose query is behind the limit), skipped dQ rows exactly 0, every gradient bit-equal to the
    full kernels' on the zero-tailed dO."""
    full = build("A", N)
    d_o = full["d_o"].clone()
    d_o[:, ql:] = 0
    dv = torch.zeros_like(d_o)
    dv.scatter_(1, full["perm"][:, :, None].expand(-1, -1, 64), d_o)            # dV_{perm(i)} = dO_i
    case = dict(full, d_o=d_o, dv=dv)
    got = run(dev, case, q_limit=ql, d_o=d_o)
    qe = min(N, (ql + 31) // 32 * 32)
    check_selector(_rows(got, slice(0, qe)), _rows(case, slice(0, qe)), parts=("o", "lse"))
    check_selector(got, case, parts=("dq", "dk", "dv"))
    # (run() has NaN behind the limit in o, lse and dO, and checks that the forward left those o / lse rows as they were)
    assert torch.equal(got["dqkv_raw"], run(dev, case, d_o=d_o)["dqkv_raw"]), "gradients differ from the full kernels' on the zero-tailed dO"
    if qe < N:
        assert bool(torch.isnan(got["o"][:, qe:]).all()) and bool(torch.isnan(got["lse"][:, qe:]).all()), "forward wrote behind q_limit"
        assert bool((got["dq"][:, qe:] == 0).all()), "skipped dQ rows are not exactly zero"


@pytest.mark.parametrize("N", F32_NS)
@pytest.mark.parametrize("probe", "AB")
def test_probe_f32(dev, probe, N):
    """Probes A and B through the fp32 operand mode (gv_attention_fwd_f32 / gv_attention_bwd_f32, N <= 260): 1e-5 absolute.
    (Probe B is what made the f32 backward renormalise its recomputed P by the row sum: lse = 96 + ln 2 is stored as the f32
    96.693146, 1.43e-6 low, and P = expf(s - lse) taken from it alone put 1.43e-6 |ref| on every gradient -- 1.144e-5 on dv and
    dq at |ref| = 8, measured on an MI355X.)"""
    case = build(probe, N)
    CHECKS[probe](run(dev, case, dtype=f32), case, tol=1e-5)
