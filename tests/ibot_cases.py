"""Shared builders of the iBOT tests (tests/test_ibot_host.py, tests/test_ibot_gpu.py): the term restated in torch from the
oracle's pieces (``oracle.vit_oracle``'s block, layer_norm, dino_head and interpolate_pos_encoding; the oracle is imported, not
edited), the fixed masks of the step tests and the fixed inputs of the kernel tests."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import step_oracle as so
from oracle import vit_oracle as vo

f64 = torch.float64


# ---- the loss, as the issue states it
def ibot_loss_ref(s, t, c, w, ts, tt):
    """-> (L_ibot, column sums of t) in the dtype of ``s``: -sum_i w_i sum_k softmax((t_i - c) / tt)_k log_softmax(s_i / ts)_k."""
    p = torch.softmax((t - c) / tt, dim=-1).detach()
    return -(w[:, None] * p * torch.log_softmax(s / ts, dim=-1)).sum(), t.sum(0)


def loss_inputs(M, K, seed=0, zero_weight=True, dominant=True):
    """Student / teacher logits f32 [M, K], centre [K], weights [M] (one exact zero when M > 1) -- and one teacher row with a single
    dominant logit (its softmax is one-hot to f32: the other classes' exponentials underflow)."""
    g = torch.Generator().manual_seed(1000 * M + K + seed)
    s, t = torch.randn(M, K, generator=g), torch.randn(M, K, generator=g)
    c = 0.1 * torch.randn(K, generator=g)
    w = torch.rand(M, generator=g) * 0.2 + 0.01
    if zero_weight and M > 1:
        w[M // 2] = 0.0
    if dominant and K > 1:
        t[M - 1, K // 3] = 60.0
    return s, t, c, w


def patch_center_ref(c, total, momentum):
    """c <- m c + (1 - m) sum / count on a [K + 1] vector (sums, count); a count of 0 leaves c."""
    n = float(total[-1])
    return c.clone() if not n > 0 else c * momentum + (total[:-1] / n) * (1.0 - momentum)


# ---- the step
def fixed_masks(J, P, variant=0):
    """One image unmasked, one with a single patch, one with the four corner patches (the first and the last patch of an image
    among them); any further image unmasked.  ``variant`` 1 moves the marks to other images and patches (a second micro-batch)."""
    side = int(round(P ** 0.5))
    m = np.zeros((J, P), np.bool_)
    corners = [0, side - 1, P - side, P - 1]
    if variant == 0:
        m[1 % J, 5 % P] = True
        m[2 % J, corners] = True
    else:
        m[0, corners] = True
        m[J - 1, [1, 2, side, P - 2]] = True
        m[1 % J, 7 % P] = True
    return m


def tokens(p, x, arch, masks=None, drop=None):
    """The encoder's final-norm output on EVERY token [n, N, D] of NCHW images ``x``: prepare_tokens with the marked patch embeddings
    replaced by mask_token before the position embedding is added (DINOv2's prepare_tokens_with_masks), the oracle's blocks and
    norm.  ``masks`` bool [n, P] tensor or None; ``drop`` [depth, 2, n] stochastic-depth factors or None."""
    a = vo.ARCHS[arch]
    n, _, w, h = x.shape
    t = F.conv2d(x, p["patch_embed.proj.weight"], p["patch_embed.proj.bias"], stride=vo.PATCH).flatten(2).transpose(1, 2)
    if masks is not None:
        t = torch.where(masks[:, :, None], p["mask_token"].to(t.dtype).view(1, 1, -1), t)
    t = torch.cat((p["cls_token"].expand(n, -1, -1), t), dim=1)
    t = t + vo.interpolate_pos_encoding(p["pos_embed"], t.shape[1] - 1, w, h)
    for i in range(a["depth"]):
        t = vo.block(t, p, i, a["num_heads"], None if drop is None else drop[i])
    return vo.layer_norm(t, p["norm.weight"], p["norm.bias"])


def reference_step(orc: "so.DinoOracle", mask_token, tiles, masks, weight, patch_center, drop=None):
    """One forward / backward of L_dino + weight * L_ibot on the oracle's networks.  ``masks`` bool [G * B, P] (numpy), crop-major
    like the feature rows.  -> dict(loss, ibot, grads (arena names, backbone.mask_token included), s_out, t_out, sp_out, tp_out,
    center_sum, patch_sum [K + 1])."""
    crops = orc.crops(tiles)
    V, G = len(crops), orc.n_global
    mk = torch.from_numpy(np.ascontiguousarray(masks))
    J, P = mk.shape
    counts = mk.sum(1)
    w = (1.0 / (counts.to(orc.dtype) * J))[mk.nonzero()[:, 0]]
    xg = torch.cat(list(crops[:G]))
    with torch.no_grad():
        tt = tokens(orc.tp, xg, orc.arch)
        t_out = vo.dino_head(orc.thp, tt[:, 0])
        tp_out = vo.dino_head(orc.thp, tt[:, 1:][mk])
    sp, shp = so._leafify(dict(orc.p, mask_token=mask_token)), so._leafify(orc.hp)
    ts_ = tokens(sp, xg, orc.arch, masks=mk, drop=None if drop is None else drop[:, :, :J])
    feats = [ts_[:, 0]]
    if V > G:
        xl = torch.cat(list(crops[G:]))
        feats.append(vo.vit_features(sp, xl, orc.arch, drop=None if drop is None else drop[:, :, J:]))
    s_out = vo.dino_head(shp, torch.cat(feats))
    sp_out = vo.dino_head(shp, ts_[:, 1:][mk])
    loss, bsum = vo.dino_loss(s_out, t_out, orc.center, V, G, orc.ts, orc.tt)
    ibot, psum = ibot_loss_ref(sp_out, tp_out, patch_center, w, orc.ts, orc.tt)
    (loss + weight * ibot).backward()
    grads = {**{"backbone." + k: v.grad for k, v in sp.items()}, **{"head." + k: v.grad for k, v in shp.items()}}
    return dict(loss=loss.detach(), ibot=ibot.detach(), grads=grads, s_out=s_out.detach(), t_out=t_out, sp_out=sp_out.detach(), tp_out=tp_out,
                center_sum=bsum, patch_sum=torch.cat([psum, torch.tensor([float(mk.sum())], dtype=psum.dtype)]), tokens=ts_, leaves=sp)


def step_case(arch, gsize, lsize, K, B=2, n_local=2, seed=0):
    """The oracle of a small DINO + iBOT step, a non-zero mask token and patch centre, and the tiles."""
    orc = so.DinoOracle(arch=arch, img_size=gsize, out_dim=K, seed=seed, n_local=n_local, gsize=gsize, lsize=lsize)
    D = vo.ARCHS[arch]["embed_dim"]
    g = torch.Generator().manual_seed(17 + seed)
    mask_token = 0.02 * torch.randn(1, D, generator=g)
    patch_center = 0.05 * torch.randn(K, generator=g)
    orc.center = 0.05 * torch.randn(1, K, generator=g)
    tiles = vo.synth_tiles(B, 256, seed=1234 + seed)
    return orc, mask_token, patch_center, tiles


def make_engine(orc, mask_token, patch_center, K, B, dev, weight=1.0, **kw):
    """The engine of ``step_case`` with the oracle's state, mask token, centres and crop windows."""
    from gipvit.engine import DinoEngine
    gsize, lsize = orc.wins[0][2], (orc.wins[-1][2] if orc.n_local else 32)
    eng = DinoEngine(arch=orc.arch, img_size=gsize, out_dim=K, batch=B, n_global=orc.n_global, n_local=orc.n_local, gsize=gsize, lsize=lsize,
                     windows=[(y, x) for y, x, _ in orc.wins], device=dev, ibot_weight=weight, **kw)
    eng.load_state(dict(orc.p, mask_token=mask_token), orc.hp)
    eng.center.copy_(orc.center[0])
    if weight > 0:
        eng.patch_center.copy_(patch_center)
    return eng
