"""Shared by tests/test_mixup_host.py and tests/test_mixup_gpu.py: timm's Mixup / mixup_target / SoftTargetCrossEntropy /
BinaryCrossEntropy restated in plain torch (timm 0.8.x; timm is not installed and the reference pins no version, so these are
pinned by nothing but themselves), and the device checks of the mixing kernels that run once per library build.

Run as a program with GIPVIT_ACT_FORMAT=f16 (tests/test_mixup_gpu.py does, as tests/test_f16_gpu.py runs tests/f16_worker.py:
one process loads one of the two libraries) it runs those checks on the float16 build and prints 'MIXUP F16 OK'."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ------------------------------------------------------------------ restatements (CPU, plain torch)
def mixup_target(target, num_classes, lam, partner, smoothing):
    """timm mixup_target: one_hot(target) * lam + one_hot(target.flip(0)) * (1 - lam), on / off values from the smoothing.
    ``lam``: float32 [B] (timm's elem / pair modes pass a tensor; batch mode a scalar = the same value in every row)."""
    off = smoothing / num_classes
    on = 1.0 - smoothing + off
    y = target.view(-1, 1).long()
    one_hot = lambda idx: torch.full((y.shape[0], num_classes), off, dtype=torch.float32).scatter_(1, idx, on)
    lam = torch.as_tensor(lam, dtype=torch.float32).view(-1, 1)
    return one_hot(y) * lam + one_hot(y[partner.long()]) * (1.0 - lam)


def mix_loss(logits, dense_target, kind, threshold=None):
    """The reference's quirk (train.py:1046): the loss sees softmax(logits).  kind 'soft_ce' = timm SoftTargetCrossEntropy,
    'bce' = timm BinaryCrossEntropy (target_threshold -> target.gt(thr); binary_cross_entropy_with_logits, mean)."""
    p = torch.softmax(logits, dim=1)
    t = dense_target
    if kind == "soft_ce":
        return torch.sum(-t * F.log_softmax(p, dim=-1), dim=-1).mean()
    if threshold is not None:
        t = t.gt(threshold).to(t.dtype)
    return F.binary_cross_entropy_with_logits(p, t, reduction="mean")


def mix_images(x, rows):
    """timm Mixup._mix_elem / _mix_pair / _mix_batch on a float NCHW batch, from the plan's rows: sources are the ORIGINAL images.
    blend: x[i] * lam + x[j] * (1 - lam), two products and a sum in float32; paste: the partner's box."""
    out = x.clone()
    for i, r in enumerate(rows):
        j = int(r["partner"])
        if r["mode"] == 1:
            out[i] = x[i] * float(r["lam"]) + x[j] * float(r["one_minus_lam"])
        elif r["mode"] == 2:
            yl, yh, xl, xh = (int(r[k]) for k in ("yl", "yh", "xl", "xh"))
            out[i][:, yl:yh, xl:xh] = x[j][:, yl:yh, xl:xh]
    return out


def rows_of(x, crop):
    """NCHW [n, 3, crop, crop] -> patch rows [n * side^2, 768], k = c*256 + py*16 + px."""
    side = crop // 16
    return x.reshape(x.shape[0], 3, side, 16, side, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1, 768)


def images_of(rows, n, crop):
    side = crop // 16
    return rows.reshape(n, side, side, 3, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(n, 3, crop, crop)


def hand_plan(B, crop):
    """Copy, blend and paste rows with the awkward boxes: touching the border, empty, starting at odd pixels, cutting through a
    16-pixel patch, the whole window."""
    from gipvit.mixup import MixPlan
    rows = MixPlan.make_rows(B)
    boxes = [(0, crop, 0, 10), (5, 5, 3, 9), (1, 33, 3, 29), (7, 25, 9, 23), (0, crop, 0, crop), (crop - 3, crop, crop - 17, crop)]
    MixPlan.set_row(rows, 0, 0.3, None)
    MixPlan.set_row(rows, B - 1, 0.3, None)
    for k, bx in enumerate(boxes[: B - 3]):
        area = (bx[1] - bx[0]) * (bx[3] - bx[2])
        i = 1 + k
        MixPlan.set_row(rows, i, 1.0 - area / float(crop * crop) if area else 0.999, bx)      # an empty box still is a paste row here
    return rows                                                                              # row B - 2 stays a copy row


def sampler_plans(B, crop):
    from gipvit.mixup import MixSampler
    out = []
    for mode in ("batch", "pair", "elem"):
        s = MixSampler(0.8, 1.0, None, 1.0, 0.5, mode, B, crop, seed=11)
        out += [(mode, s.sample_host()) for _ in range(3)]
    s = MixSampler(0.0, 0.0, (0.2, 0.8), 0.7, 0.5, "elem", B, crop, seed=5)
    out.append(("elem minmax", s.sample_host()))
    return out


def assert_bits_equal(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan), what
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(it)[~nan], ref.view(it)[~nan]), (what, int((got.view(it) != ref.view(it)).sum()))


# ------------------------------------------------------------------ device checks, once per library build
def check_patchify_mix_u8(dev):
    """gv_patchify_mix[_f32] against the unmixed kernel's own f32 rows R (exactness is the gate)."""
    from gipvit import ops
    from gipvit.mixup import MixPlan
    from oracle import vit_oracle as vo
    B, crop, tile, win = 8, 64, 96, (5, 7)
    tiles = vo.synth_tiles(B, tile, seed=7)
    td = tiles.to(dev)
    fill = torch.zeros(B, 8)
    fill[1] = torch.tensor([10., 50., 20., 70., 0.5, -0.25, 1.5, 1.]); fill[6] = torch.tensor([0., 96., 0., 96., 0.1, 0.2, 0.3, 1.])
    fill[3] = torch.tensor([10., 50., 20., 70., 9., 9., 9., 0.])                                  # switched off
    f32rows = lambda t, **kw: ops.patchify(t, [win], crop, vo.MEAN_RON, vo.STD_RON, out=torch.empty(B * 16, 768, dtype=torch.float32, device=dev), **kw)
    plans = [("hand", hand_plan(B, crop))] + sampler_plans(B, crop)
    seen = set()
    for fl in (None, fill.to(dev)):
        kw = {} if fl is None else {"fill": fl}
        R = images_of(f32rows(td, **kw).cpu(), B, crop)
        for name, rows in plans:
            seen |= set(rows["mode"].tolist())
            plan = MixPlan(rows, dev)
            ref = rows_of(mix_images(R, rows), crop)
            got32 = f32rows(td, mix=plan.table, **kw).cpu()
            assert_bits_equal(got32, ref, f"f32 {name} fill={fl is not None}")
            got16 = ops.patchify(td, [win], crop, vo.MEAN_RON, vo.STD_RON, mix=plan.table, **kw).cpu()
            assert_bits_equal(got16, ref.to(ops.bf16), f"16-bit {name} fill={fl is not None}")
            if fl is None:      # copy and paste rows: gv_patchify of the batch pasted on the host as uint8
                tp = tiles.clone()
                keep = torch.zeros(B, dtype=torch.bool)
                for i, r in enumerate(rows):
                    keep[i] = bool(r["mode"] != 1)
                    if r["mode"] == 2:
                        j, yl, yh, xl, xh = (int(r[k]) for k in ("partner", "yl", "yh", "xl", "xh"))
                        tp[i, win[0] + yl:win[0] + yh, win[1] + xl:win[1] + xh] = tiles[j, win[0] + yl:win[0] + yh, win[1] + xl:win[1] + xh]
                sel = keep.repeat_interleave(16)
                assert_bits_equal(got32[sel], f32rows(tp.to(dev)).cpu()[sel], f"f32 pasted u8 {name}")
                assert_bits_equal(got16[sel], ops.patchify(tp.to(dev), [win], crop, vo.MEAN_RON, vo.STD_RON).cpu()[sel], f"16-bit pasted u8 {name}")
    assert seen == {0, 1, 2}


def check_patchify_mix_nchw(dev):
    """gv_patchify_nchw_mix[_f32]: bit-identical to torch's expression then .to(16-bit); contiguous and strided (sliced) input."""
    from gipvit import ops
    from gipvit.mixup import MixPlan
    B, crop = 8, 64
    g = torch.Generator().manual_seed(17)
    x = 3.0 * torch.randn(B, 3, 80, 88, generator=g)
    x[0, 0, 5, 7] = float("inf"); x[2, 1, 30, 40] = float("nan"); x[1, 0, 50, 60] = 1e30; x[0, 1, 20, 21] = -0.0
    big = torch.randn(B + 3, 3, 90, 99, generator=g)
    sl = big[2:2 + B, :, 3:83, 7:95]                                    # N / C / H strides of the big batch, odd offset
    for src_cpu, src in ((x, x.to(dev)), (sl, big.to(dev)[2:2 + B, :, 3:83, 7:95])):
        assert src.stride(-1) == 1
        for win in ((0, 0), (3, 5), (16, 24)):
            w = src_cpu[:, :, win[0]:win[0] + crop, win[1]:win[1] + crop]
            for name, rows in [("hand", hand_plan(B, crop))] + sampler_plans(B, crop):
                plan = MixPlan(rows, dev)
                ref = rows_of(mix_images(w, rows), crop)
                out = torch.empty(ref.shape, dtype=torch.float32, device=dev)
                assert_bits_equal(ops.patchify_nchw(src, [win], crop, out=out, mix=plan.table).cpu(), ref, f"f32 {name} {win} {src.stride()}")
                assert_bits_equal(ops.patchify_nchw(src, [win], crop, mix=plan.table).cpu(), ref.to(ops.bf16), f"16-bit {name} {win} {src.stride()}")
        # timm's batch-mode line itself, lam a Python double: x.mul(lam).add(x.flip(0).mul(1 - lam))
        lam = 0.37219473
        rows = MixPlan.make_rows(B)
        for i in range(B):
            MixPlan.set_row(rows, i, lam, None)
        w = src_cpu[:, :, :crop, :crop].clone()
        ref = rows_of(w.mul(lam).add(w.flip(0).mul(1.0 - lam)), crop)
        assert_bits_equal(ops.patchify_nchw(src, [(0, 0)], crop, mix=MixPlan(rows, dev).table).cpu(), ref.to(ops.bf16), "timm batch line")


def check_mix_loss(dev, cases=((8, 2), (300, 5), (64, 64))):
    """gv_softmax_mix_loss against the restatement under autograd, at test_softmax_lsce's gates."""
    from gipvit import ops
    for B, C in cases:
        g = torch.Generator().manual_seed(B)
        z = torch.randn(B, C, generator=g)
        tgt = torch.randint(0, C, (B, 1), generator=g)
        partner = (B - 1 - torch.arange(B)).to(torch.int32)
        lam = torch.rand(B, generator=g)
        lam[::3] = 1.0
        for kind, thr in (("soft_ce", None), ("bce", None), ("bce", 0.2)):
            for mixed in (True, False):
                zr = z.clone().requires_grad_(True)
                lm = lam if mixed else torch.ones(B)
                ref = mix_loss(zr, mixup_target(tgt, C, lm, partner, 0.1), kind, thr)
                ref.backward()
                loss, dz, prob = torch.empty(1, device=dev), torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
                ops.softmax_mix_loss(z.to(dev), tgt.view(-1).to(dev), loss, dz, prob, B, C, 0.1, kind, partner=partner.to(dev) if mixed else None,
                                     lam=lam.to(dev) if mixed else None, threshold=thr)
                what = f"B={B} C={C} {kind} thr={thr} mixed={mixed}"
                print(f"[mix loss] {what}: loss {float(loss):.6f} ref {float(ref.detach()):.6f}")
                assert abs(float(loss) - float(ref.detach())) < 1e-5, what
                assert torch.allclose(dz.cpu(), zr.grad, rtol=1e-4, atol=1e-6), (what, float((dz.cpu() - zr.grad).abs().max()))
                assert torch.allclose(prob.cpu(), torch.softmax(z, 1), rtol=1e-5, atol=1e-6), what


if __name__ == "__main__":          # the float16 build, in a process of its own
    assert sys.argv[1:] == ["f16"] and os.environ.get("GIPVIT_ACT_FORMAT") == "f16"
    from gipvit import _lib, ops
    assert _lib.lib.gv_act_format() == 1 and ops.bf16 is torch.float16
    d = torch.device("cuda:0")
    check_patchify_mix_u8(d)
    check_patchify_mix_nchw(d)
    check_mix_loss(d, cases=((300, 5),))
    torch.cuda.synchronize()
    print("MIXUP F16 OK")
