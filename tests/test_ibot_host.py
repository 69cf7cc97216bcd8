"""CPU: the iBOT masked-patch term -- the mask sampler and its plan, the term's torch restatement (tests/ibot_cases.py) and what it says
about mask_token and the patch embedding, two gloo ranks reaching the one-process patch centre, the new entry points' refusals and
struct layouts without a GPU, the driver's flags, and where the new launches sit in the engine's sequence (tests/launch_trace.py)."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import ibot_cases as C
import launch_trace as LT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mask_tokens_fwd", "mask_tokens_bwd", "rows_gather", "rows_scatter", "ibot_loss", "patch_center_update")


# ---- the sampler and the plan
@pytest.mark.parametrize("grid,J,ratio,prob", [(4, 8, (0.1, 0.5), 0.5), (14, 16, (0.1, 0.5), 0.5), (14, 5, (0.3, 0.3), 1.0), (6, 3, (0.1, 0.9), 0.4)])
def test_sampler_counts_and_plan(grid, J, ratio, prob):
    from gipvit.masking import MaskSampler, MaskPlan, max_rows
    P = grid * grid
    a, b = MaskSampler(grid, J, ratio, prob, seed=7), MaskSampler(grid, J, ratio, prob, seed=7)
    other = MaskSampler(grid, J, ratio, prob, seed=8)
    differs = False
    for _ in range(20):
        pa, pb = a.sample(), b.sample()
        assert np.array_equal(pa.masks, pb.masks) and torch.equal(pa.rows, pb.rows) and torch.equal(pa.weight, pb.weight)      # same seed, same plans
        differs |= not np.array_equal(pa.masks, other.sample_host())
        assert pa.masks.shape == (J, P) and pa.masks.dtype == np.bool_
        n = int(J * prob)
        assert int((a.last_targets > 0).sum()) == n or int(P * ratio[0]) == 0
        # no image without a target is masked (one with a target of a patch or two may stay empty: ten tries, blocks of about 4)
        assert (pa.counts[a.last_targets == 0] == 0).all() and pa.n_masked_images <= n
        if grid >= 6:
            assert pa.n_masked_images == n
        assert (pa.counts <= a.last_targets).all() and int(pa.counts.max()) <= int(ratio[1] * P) and pa.M <= max_rows(J, P, ratio, prob)
        rows = pa.rows.numpy()
        assert rows.dtype == np.int32 and len(rows) == pa.M == int(pa.masks.sum())
        assert (np.diff(rows) > 0).all() and (rows % (P + 1) != 0).all() and rows.min() >= 1 and rows.max() < J * (P + 1)
        back = np.zeros((J, P + 1), bool); back.reshape(-1)[rows] = True
        assert np.array_equal(back[:, 1:], pa.masks)
        assert abs(float(pa.weight.double().sum()) - pa.n_masked_images / J) < 1e-6
        assert np.allclose(pa.weight.numpy(), 1.0 / (pa.counts[rows // (P + 1)] * J))
    assert differs
    assert isinstance(MaskPlan.from_masks(pa.masks), MaskPlan)


def test_sampler_exact_number_of_masked_images_and_shuffle():
    from gipvit.masking import MaskSampler
    s = MaskSampler(14, 128, (0.1, 0.5), 0.5, seed=0)
    first = []
    for _ in range(5):
        p = s.sample()
        assert p.n_masked_images == 64                     # exactly int(J * prob)
        first.append(tuple(np.nonzero(p.counts)[0][:8]))
        # the i-th masked image's target lies in the i-th of 64 sub-intervals of the ratio: the sorted targets rise through [0.1 P, 0.5 P]
        t = np.sort(s.last_targets[s.last_targets > 0])
        edges = np.linspace(0.1, 0.5, 65) * 196
        assert (t >= np.floor(edges[:-1]) - 1e-9).all() and (t <= edges[1:] + 1e-9).all()
    assert len(set(first)) > 1                             # masked and unmasked images are shuffled, anew every time
    assert 0.25 * 196 * 64 < np.mean([s.sample().M for _ in range(10)]) < 0.31 * 196 * 64       # about 0.3 P per masked image


def test_sampler_stream_survives_save_and_restore():
    from gipvit.masking import MaskSampler
    a = MaskSampler(14, 8, seed=3)
    a.sample()
    sd = a.state_dict()
    assert all(isinstance(v, str) for v in sd.values())
    want = [a.sample_host() for _ in range(3)]
    b = MaskSampler(14, 8, seed=99)
    b.load_state_dict(sd)
    assert all(np.array_equal(w, b.sample_host()) for w in want)


def test_sampler_and_plan_refuse_bad_options():
    from gipvit.masking import MaskSampler, MaskPlan
    for kw in (dict(ratio=(0.0, 0.5)), dict(ratio=(0.6, 0.5)), dict(ratio=(0.1, 1.0)), dict(prob=0.0), dict(prob=1.5), dict(prob=float("nan")),
               dict(grid=3), dict(n_images=0)):
        with pytest.raises(ValueError):
            MaskSampler(**dict(dict(grid=14, n_images=4, seed=0), **kw))
    with pytest.raises(ValueError):
        MaskPlan(np.zeros((4, 16), np.float32))
    empty = MaskPlan.from_masks(np.zeros((4, 16), bool))
    assert empty.M == 0 and empty.rows.numel() == 0 and empty.weight.numel() == 0 and empty.rows.dtype == torch.int32
    assert "not bit-compatible" in sys.modules["gipvit.masking"].__doc__


# ---- the term, restated in torch
@pytest.fixture(scope="module")
def ref():
    torch.set_num_threads(min(8, len(os.sched_getaffinity(0))))
    orc, mt, pc, tiles = C.step_case("vit_tiny", 64, 32, 64, n_local=1)
    masks = C.fixed_masks(4, 16)
    return orc, mt, pc, tiles, masks, C.reference_step(orc, mt, tiles, masks, 1.0, pc)


def test_reference_mask_token_gradient_is_the_sum_over_marked_rows(ref):
    """With the teacher's outputs held: d mask_token = the sum of the token-input gradients at the marked rows, and the patch embedding
    is blind to a marked patch -- the loss's gradient with respect to that patch's pixels is exactly zero (and is not for the others),
    so the patch-embedding weight gradient holds nothing of it."""
    import torch.nn.functional as F
    orc, mt, pc, tiles, masks, r = ref
    assert float(r["ibot"]) > 0 and float(r["grads"]["backbone.mask_token"].abs().max()) > 0
    sp = {k: v.detach() for k, v in r["leaves"].items()}
    hp = {k: v.detach() for k, v in orc.hp.items()}
    mk = torch.from_numpy(masks)
    crops = orc.crops(tiles)
    xg = torch.cat(list(crops[:2])).requires_grad_(True)
    probe = torch.zeros(4, 17, 192, requires_grad=True)         # an additive probe at the student's token input: its gradient is the tokens'
    t = F.conv2d(xg, sp["patch_embed.proj.weight"], sp["patch_embed.proj.bias"], stride=16).flatten(2).transpose(1, 2)
    t = torch.where(mk[:, :, None], sp["mask_token"].view(1, 1, -1), t)
    t = torch.cat((sp["cls_token"].expand(4, -1, -1), t), dim=1) + sp["pos_embed"] + probe
    for i in range(12):
        t = C.vo.block(t, sp, i, 3)
    t = C.vo.layer_norm(t, sp["norm.weight"], sp["norm.bias"])
    feats = torch.cat([t[:, 0], C.vo.vit_features(sp, torch.cat(list(crops[2:])), "vit_tiny")])
    loss, _ = C.vo.dino_loss(C.vo.dino_head(hp, feats), r["t_out"], orc.center, 3, 2, orc.ts, orc.tt)
    w = (1.0 / (mk.sum(1).float() * 4))[mk.nonzero()[:, 0]]
    ibot, _ = C.ibot_loss_ref(C.vo.dino_head(hp, t[:, 1:][mk]), r["tp_out"], pc, w, orc.ts, orc.tt)
    assert abs(float(loss) - float(r["loss"])) < 1e-5 and abs(float(ibot) - float(r["ibot"])) < 1e-5
    (loss + ibot).backward()
    want = probe.grad[:, 1:][mk].sum(0)
    got = r["grads"]["backbone.mask_token"][0]
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    gpix = F.unfold(xg.grad, 16, stride=16).transpose(1, 2)      # [4, 16, 768]: the pixel gradient, patch by patch
    assert float(gpix[mk].abs().max()) == 0.0 and float(gpix[~mk].abs().amax(1).min()) > 0.0


def _center_worker(rank, world, port, q, sums):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gipvit.dist import RcclReducer
    v = sums[rank].clone()
    red = RcclReducer()
    red.reduce_tensor(v)
    red.finish()
    q.put((rank, v))
    dist.destroy_process_group()


def test_two_ranks_with_different_counts_reach_the_one_process_centre():
    """Rank 0 marks 5 rows, rank 1 marks 11 (and, in a second round, none): their [K + 1] vectors (column sums, count) added by
    reducer.reduce_tensor give the centre of one process that saw all 16 rows."""
    import torch.multiprocessing as mp
    K = 64
    g = torch.Generator().manual_seed(0)
    t0, t1 = torch.randn(5, K, generator=g), torch.randn(11, K, generator=g)
    c = 0.1 * torch.randn(K, generator=g)
    sums = [torch.cat([t0.sum(0), torch.tensor([5.0])]), torch.cat([t1.sum(0), torch.tensor([11.0])])]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ps = [ctx.Process(target=_center_worker, args=(r, 2, port, q, sums)) for r in range(2)]
    [p.start() for p in ps]
    res = dict(q.get(timeout=120) for _ in ps)
    [p.join(60) for p in ps]
    one = torch.cat([torch.cat([t0, t1]).sum(0), torch.tensor([16.0])])
    for r in (0, 1):
        assert float(res[r][K]) == 16.0 and torch.allclose(res[r], one, rtol=1e-6, atol=1e-6)
        got = C.patch_center_ref(c, res[r], 0.9)
        want = 0.9 * c + 0.1 * torch.cat([t0, t1]).mean(0)
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    # a rank without a marked row adds zeros and a zero count; all ranks empty: the centre stays
    assert torch.equal(C.patch_center_ref(c, torch.zeros(K + 1), 0.9), c)
    alone = C.patch_center_ref(c, sums[0] + torch.zeros(K + 1), 0.9)
    assert torch.allclose(alone, 0.9 * c + 0.1 * t0.mean(0), rtol=1e-6, atol=1e-7)


# ---- the ABI without a GPU
def _lib():
    from gipvit import _lib as L
    return L


ENTRIES = {"gv_mask_tokens_fwd": "gv_mask_tokens_fwd_args", "gv_mask_tokens_bwd": "gv_mask_tokens_bwd_args", "gv_mask_tokens_bwd_f32": "gv_mask_tokens_bwd_args",
           "gv_rows_gather": "gv_rows_gather_args", "gv_rows_scatter": "gv_rows_scatter_args", "gv_rows_scatter_f32": "gv_rows_scatter_args",
           "gv_ibot_loss": "gv_ibot_loss_args", "gv_ibot_loss_f32": "gv_ibot_loss_args", "gv_patch_center_update": "gv_patch_center_update_args"}
PLAIN = ["gv_mask_tokens_workspace_bytes", "gv_ibot_loss_workspace_bytes"]


def test_both_builds_export_the_entry_points():
    L = _lib()
    assert all(hasattr(L.lib, n) for n in list(ENTRIES) + PLAIN) and L.lib.gv_version() == 9
    assert all(L.ENTRY_POINTS[n] is getattr(L, s) for n, s in ENTRIES.items()) and all(n in L.PLAIN_SYMBOLS for n in PLAIN)
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); missing = [n for n in sys.argv[2:] if not hasattr(l, n)]; assert not missing, missing; "
            "l.gv_ibot_loss_workspace_bytes.restype = ctypes.c_int64; assert l.gv_ibot_loss_workspace_bytes(67, 1000) > 0 and l.gv_version() == 9")
    for lib in ("libgipvit_hip.so", "libgipvit_hip_f16.so"):
        r = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(L.LIB_PATH), lib)] + list(ENTRIES) + PLAIN, capture_output=True, text=True)
        assert r.returncode == 0, (lib, r.stderr[-600:])


def test_struct_layouts_match_gcc(tmp_path):
    L = _lib()
    structs = [getattr(L, s) for s in sorted(set(ENTRIES.values()))]
    lines = []
    for st in structs:
        lines.append(f'printf("{st.__name__} %zu\\n", sizeof({st.__name__}));')
        lines += [f'printf("{st.__name__}.{f} %zu\\n", offsetof({st.__name__}, {f}));' for f, _ in st._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gipvit.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for st in structs:
        assert int(out[st.__name__]) == ctypes.sizeof(st), st.__name__
        for f, _ in st._fields_:
            assert int(out[f"{st.__name__}.{f}"]) == getattr(st, f).offset, (st.__name__, f)


def _err():
    return _lib().lib.gv_last_error().decode()


def _rc(name, ok):
    L = _lib()
    fn = getattr(L.lib, name)
    assert fn(None, None) == -3
    return lambda **kw: fn(ctypes.byref(L.ENTRY_POINTS[name](**dict(ok, **kw))), None)


def test_mask_tokens_abi_errors():
    L = _lib()
    ok = dict(x=4096, mask_token=8192, pos=12288, rows=16384, M=5, N=17, D=192, n_rows=68)          # never dereferenced
    rc = _rc("gv_mask_tokens_fwd", ok)
    for p in ("x", "mask_token", "pos", "rows"):
        assert rc(**{p: None}) == -3 and "null" in _err(), p
    for kw in (dict(M=0), dict(D=190), dict(D=0), dict(N=1), dict(n_rows=67), dict(n_rows=0)):
        assert rc(**kw) == -1, kw
    assert rc(x=4096 + 4) == -2 and rc(pos=12288 + 8) == -2 and rc(rows=16384 + 2) == -2 and "aligned" in _err()
    okb = dict(g=4096, gpatch=8192, dmask_token=12288, rows=16384, workspace=20480, workspace_bytes=1 << 30, M=65, N=17, D=192, n_rows=68, accumulate=0)
    for name in ("gv_mask_tokens_bwd", "gv_mask_tokens_bwd_f32"):
        rc = _rc(name, okb)
        for p in ("g", "gpatch", "dmask_token", "rows", "workspace"):
            assert rc(**{p: None}) == -3 and "null" in _err(), p
        for kw in (dict(M=0), dict(D=190), dict(D=1028), dict(N=1), dict(n_rows=67)):
            assert rc(**kw) == -1, kw
        need = L.lib.gv_mask_tokens_workspace_bytes(65, 192)
        assert need == 2 * 192 * 4 and rc(workspace_bytes=need - 1) == -1 and str(need) in _err() and "workspace" in _err()
        assert rc(g=4096 + 4) == -2 and rc(dmask_token=12288 + 8) == -2 and rc(workspace=20480 + 4) == -2
        assert rc(gpatch=8192 + (8 if "f32" in name else 4)) == -2
    assert L.lib.gv_mask_tokens_workspace_bytes(1, 768) == 768 * 4 and L.lib.gv_mask_tokens_workspace_bytes(64, 768) == 768 * 4
    for bad in ((0, 192), (5, 190), (5, 1028)):
        assert L.lib.gv_mask_tokens_workspace_bytes(*bad) == -1 and _err().startswith("gv_mask_tokens_workspace_bytes"), bad


def test_rows_gather_scatter_abi_errors():
    ok = dict(x=4096, x_stride=192, rows=8192, out=12288, scale=None, scale_out=None, M=5, D=192, n_rows=68)
    rc = _rc("gv_rows_gather", ok)
    for p in ("x", "rows", "out"):
        assert rc(**{p: None}) == -3 and "null" in _err(), p
    assert rc(scale=16384) == -3 and rc(scale_out=16384) == -3 and "together" in _err()
    for kw in (dict(M=0), dict(D=190), dict(n_rows=0), dict(x_stride=190), dict(x_stride=188)):
        assert rc(**kw) == -1, kw
    assert rc(x=4096 + 4) == -2 and rc(out=12288 + 8) == -2 and rc(rows=8192 + 1) == -2
    oks = dict(g_src=4096, g=8192, g_stride=192, gb_src=12288, gb=16384, gb_stride=192, rows=20480, M=5, D=192, n_rows=68)
    for name in ("gv_rows_scatter", "gv_rows_scatter_f32"):
        rc = _rc(name, oks)
        for p in ("g_src", "g", "rows"):
            assert rc(**{p: None}) == -3 and "null" in _err(), p
        assert rc(gb=None) == -3 and rc(gb_src=None) == -3 and "together" in _err()
        for kw in (dict(M=0), dict(D=190), dict(g_stride=100), dict(gb_stride=190), dict(n_rows=0)):
            assert rc(**kw) == -1, kw
        assert rc(g=8192 + 4) == -2 and rc(g_src=4096 + 8) == -2 and rc(gb=16384 + (8 if "f32" in name else 4)) == -2


def test_ibot_loss_and_patch_center_abi_errors():
    L = _lib()
    ok = dict(student=4096, teacher=8192, center=12288, weight=16384, dstudent=20480, loss=24576, center_sum=28672, workspace=32768,
              workspace_bytes=1 << 40, M=67, K=1000, student_temp=0.1, teacher_temp=0.04, ibot_weight=1.0, grad_scale=1.0, hyper=None, loss_scale=None)
    for name in ("gv_ibot_loss", "gv_ibot_loss_f32"):
        rc = _rc(name, ok)
        for p in ("student", "teacher", "center", "weight", "dstudent", "loss", "center_sum", "workspace"):
            assert rc(**{p: None}) == -3 and "null" in _err(), p
        for kw in (dict(M=0), dict(K=0), dict(M=-1), dict(K=(1 << 20) + 1), dict(M=(1 << 20) + 1)):
            assert rc(**kw) == -1 and "<=" in _err(), kw
        assert rc(student_temp=0.0) == -1 and rc(teacher_temp=-1.0) == -1 and "temperatures" in _err()
        for w in (-0.5, float("nan"), float("inf")):
            assert rc(ibot_weight=w) == -1 and "ibot_weight" in _err(), w
        need = L.lib.gv_ibot_loss_workspace_bytes(67, 1000)
        assert need >= (4 * 67 + 67 * 1000) * 4 and rc(workspace_bytes=need - 1) == -1 and str(need) in _err()
        assert rc(student=4096 + 4) == -2 and rc(center_sum=28672 + 8) == -2 and rc(workspace=32768 + 4) == -2 and "aligned" in _err()
        assert rc(K=1001, student=4096 + 4, teacher=8192 + 4, center=12288 + 4) != -2          # no multiple of 4: 4-byte alignment is enough
    assert L.lib.gv_ibot_loss_workspace_bytes(1, 1) > 0
    for bad in ((0, 8), (8, 0), ((1 << 20) + 1, 8)):
        assert L.lib.gv_ibot_loss_workspace_bytes(*bad) == -1 and _err().startswith("gv_ibot_loss_workspace_bytes"), bad
    okc = dict(center=4096, center_sum=8192, K=1000, momentum=0.9)
    rc = _rc("gv_patch_center_update", okc)
    assert rc(center=None) == -3 and rc(center_sum=None) == -3 and "null" in _err()
    assert rc(K=0) == -1 and rc(momentum=1.5) == -1 and rc(momentum=-0.1) == -1 and "momentum" in _err()


# ---- the driver
def _train():
    sys.path.insert(0, ROOT)
    import train
    return train


SMALL = ["--model", "vit_tiny", "--dino", "--global-crop-size", "64", "--local-crop-size", "32", "--tile-size", "96", "--batch-size", "2"]


def test_flags_reach_the_engine():
    train = _train()
    base, _ = train.parse_args(["--model", "vit_tiny", "--dino"])
    assert train.ibot_options(base) == dict(ibot_weight=0.0, ibot_mask_ratio=(0.1, 0.5), ibot_mask_prob=0.5, drop=0.0)
    assert train.check_supported(base, lambda m: None) is None
    on, _ = train.parse_args(SMALL + ["--ibot-weight", "1", "--ibot-mask-ratio", "0.2", "0.6", "--ibot-mask-prob", "1.0", "--out-dim", "256"])
    assert train.check_supported(on, lambda m: None) is None
    kw = train.ibot_options(on)
    assert kw == dict(ibot_weight=1.0, ibot_mask_ratio=(0.2, 0.6), ibot_mask_prob=1.0, drop=0.0)
    from gipvit.engine import DinoEngine
    eng = DinoEngine(arch="vit_tiny", img_size=64, gsize=64, lsize=32, tile=96, out_dim=256, batch=2, device="cpu", **kw)
    assert eng.ibot_weight == 1.0 and eng.ibot_rows == 4 * int(0.6 * 16) and eng.pr_s.hb.logits.shape == (eng.ibot_rows, 256)
    assert eng.patch_center.shape == (256,) and eng.patch_center_sum.shape == (257,) and eng.ibot.shape == (1,)
    assert eng.g_stu.all_tokens and eng.g_teach.all_tokens
    # mask_token: last of the no-decay part of the arena, in both state dicts, zeros at the start, every other offset unchanged
    off = DinoEngine(arch="vit_tiny", img_size=64, gsize=64, lsize=32, tile=96, out_dim=256, batch=2, device="cpu")
    assert off.ibot is None and off.patch_center is None and off.pr_s is None and not off.g_stu.all_tokens and "backbone.mask_token" not in off.arena.specs
    assert eng.arena.order[-1] == "backbone.mask_token" and eng.arena.order[:-1] == off.arena.order and eng.arena.off["backbone.mask_token"] == off.arena.n
    assert all(eng.arena.off[n] == off.arena.off[n] for n in off.arena.order) and eng.arena.n_decay == off.arena.n_decay
    from gipvit.engine import no_weight_decay
    assert no_weight_decay("backbone.mask_token", (1, 192)) and no_weight_decay("mask_token", (1, 192))
    assert "mask_token" in eng.backbone_state_dict() and "mask_token" in eng.backbone_state_dict(teacher=True)
    assert float(eng.backbone_state_dict()["mask_token"].abs().max()) == 0.0


@pytest.mark.parametrize("flags,word", [
    (["--model", "vit_tiny", "--ibot-weight", "1"], "--dino"),
    (["--model", "vit_tiny", "--ibot-mask-prob", "0.3"], "--dino"),
    (["--model", "vit_tiny", "--ibot-mask-ratio", "0.2", "0.4"], "--dino"),
    (SMALL + ["--ibot-weight", "-1"], "--ibot-weight"),
    (SMALL + ["--ibot-weight", "nan"], "--ibot-weight"),
    (SMALL + ["--ibot-weight", "inf"], "--ibot-weight"),
    (SMALL + ["--ibot-weight", "1", "--ibot-mask-ratio", "0", "0.5"], "--ibot-mask-ratio"),
    (SMALL + ["--ibot-weight", "1", "--ibot-mask-ratio", "0.6", "0.5"], "--ibot-mask-ratio"),
    (SMALL + ["--ibot-weight", "1", "--ibot-mask-ratio", "0.1", "1.0"], "--ibot-mask-ratio"),
    (SMALL + ["--ibot-weight", "1", "--ibot-mask-prob", "0"], "--ibot-mask-prob"),
    (SMALL + ["--ibot-weight", "1", "--ibot-mask-prob", "1.1"], "--ibot-mask-prob"),
    (["--model", "vit_tiny", "--dino", "--global-crop-size", "48", "--local-crop-size", "32", "--tile-size", "96", "--ibot-weight", "1"], "--global-crop-size"),
    (SMALL + ["--ibot-weight", "1", "--drop", "0.1"], "--drop"),
    (SMALL + ["--ibot-weight", "1", "--amp"], "--amp-dtype"),
    (SMALL + ["--ibot-weight", "1", "--centering", "sinkhorn_knopp"], "--centering"),
])
def test_driver_refuses_before_any_gpu_work(flags, word):
    train = _train()
    args, _ = train.parse_args(flags)
    with pytest.raises(SystemExit) as e:
        train.check_supported(args, lambda m: None)
    assert word in str(e.value), str(e.value)


def test_engine_refuses_bad_options():
    from gipvit.engine import DinoEngine
    from gipvit.masking import MaskPlan
    base = dict(arch="vit_tiny", img_size=64, gsize=64, lsize=32, tile=96, out_dim=256, batch=2, device="cpu")
    for kw, word in ((dict(ibot_weight=-1.0), "ibot_weight"), (dict(ibot_weight=float("nan")), "ibot_weight"), (dict(ibot_weight=float("inf")), "ibot_weight"),
                     (dict(ibot_weight=1.0, ibot_mask_ratio=(0.0, 0.5)), "ratio"), (dict(ibot_weight=1.0, ibot_mask_ratio=(0.5, 1.0)), "ratio"),
                     (dict(ibot_weight=1.0, ibot_mask_prob=0.0), "probability"), (dict(ibot_weight=1.0, gsize=48, img_size=48), "64 px"),
                     (dict(ibot_weight=1.0, drop=0.1), "drop"), (dict(ibot_weight=1.0, centering="sinkhorn_knopp"), "sinkhorn_knopp")):
        with pytest.raises(ValueError) as e:
            DinoEngine(**dict(base, **kw))
        assert word in str(e.value), (kw, str(e.value))
    tiles = torch.zeros(2, 96, 96, 3, dtype=torch.uint8)
    plan = MaskPlan.from_masks(C.fixed_masks(4, 16))
    with LT.recording():
        on, off = DinoEngine(**dict(base, ibot_weight=1.0)), DinoEngine(**base)
        with pytest.raises(ValueError) as e:
            on.step(tiles)
        assert "MaskPlan" in str(e.value)
        with pytest.raises(ValueError) as e:
            off.step(tiles, masks=plan)
        assert "iBOT" in str(e.value)
        with pytest.raises(ValueError):                     # a plan for another number of images, or more rows than the buffers hold
            on.step(tiles, masks=MaskPlan.from_masks(np.zeros((2, 16), bool)))
        with pytest.raises(ValueError):
            on.step(tiles, masks=MaskPlan.from_masks(np.ones((4, 16), bool)))
        with pytest.raises(ValueError):
            on.set_dropout(0.1, 1)


def test_states_without_and_with_mask_token(capsys):
    from gipvit.engine import DinoEngine, FeatureExtractor
    base = dict(arch="vit_tiny", img_size=64, gsize=64, lsize=32, tile=96, out_dim=256, batch=2, device="cpu")
    with LT.recording():
        on, off = DinoEngine(**dict(base, ibot_weight=1.0)), DinoEngine(**base)
        bb_off, bb_on = off.backbone_state_dict(), on.backbone_state_dict()
        bb_on["mask_token"] = torch.full((1, 192), 0.5)
        on.load_state(bb_off, off.head_state_dict())        # a file from a run without iBOT: zeros, and says so
        assert "mask_token" in capsys.readouterr().out and float(on.backbone_state_dict()["mask_token"].abs().max()) == 0.0
        on.load_state(bb_on, off.head_state_dict())
        assert capsys.readouterr().out == "" and float(on.backbone_state_dict()["mask_token"].min()) == 0.5
        assert float(on.backbone_state_dict(teacher=True)["mask_token"].min()) == 0.5          # the teacher starts as a copy
        off.load_state(bb_on, off.head_state_dict())        # a --dino run without the flag: dropped, and says so
        assert "dropped" in capsys.readouterr().out and "mask_token" not in off.backbone_state_dict()
        fx = FeatureExtractor(arch="vit_tiny", img_size=64, batch=2, device="cpu")
        fx.load_state(bb_on)
        assert "dropped" in capsys.readouterr().out
        fx.load_state(bb_off)
        assert capsys.readouterr().out == ""


def test_initial_checkpoint_drops_or_keeps_mask_token(tmp_path, capsys):
    from gipvit import models as M
    sd = M.init_vit_state("vit_tiny", 64, 0, seed=0)
    sd["mask_token"] = torch.full((1, 192), 0.25)
    path = str(tmp_path / "ck.pth.tar")
    torch.save({"state_dict": {"backbone." + k: v for k, v in sd.items()}}, path)
    out = M.load_encoder_checkpoint(path, "vit_tiny", 64)
    assert "mask_token" not in out and "dropped" in capsys.readouterr().out
    out = M.load_encoder_checkpoint(path, "vit_tiny", 64, mask_token=True)
    assert float(out["mask_token"].min()) == 0.25 and capsys.readouterr().out == ""


# ---- the launch sequence
def _traced(cfg="dino_t", micro=False, plans=None, **kw):
    from gipvit.engine import DinoEngine
    from gipvit.masking import MaskPlan
    arch = {"dino_t": "vit_tiny", "dino_s": "vit_small"}[cfg]
    with LT.recording() as rec:
        eng = DinoEngine(arch=arch, img_size=224, out_dim=256, batch=2, device="cpu", **kw)
        eng.load_state(eng.backbone_state_dict(), eng.head_state_dict())
        eng.load_teacher_state(eng.backbone_state_dict(), eng.head_state_dict(), center=eng.center)
        tiles = torch.zeros(2, 256, 256, 3, dtype=torch.uint8)
        if plans is not None:
            plans = [MaskPlan.from_masks(m) for m in plans]
        if micro:
            eng.step_micro([tiles, tiles], **({} if plans is None else {"masks": plans}))
        else:
            eng.step(tiles, **({} if plans is None else {"masks": plans[0]}))
    return eng, rec, plans


def _storage(rec, t):
    return rec.storages[t.untyped_storage().data_ptr()]


def _mentions(ev, n):
    def walk(v):
        if isinstance(v, dict):
            return ("tensor" in v and v["tensor"][0] == n) or any(walk(x) for k, x in v.items() if k != "tensor")
        return isinstance(v, list) and any(walk(x) for x in v)
    return len(ev) == 3 and (walk(ev[1]) or walk(ev[2]))


def test_weight_zero_is_the_recorded_trace():
    """tests/launch_trace.py's own procedures, run through its own builder with the weight spelled out as 0: the dino_t and dino_s
    traces are the fixture's, hash and all."""
    from gipvit import engine
    fix = LT.load_fixture()
    real = engine.DinoEngine

    class Spelled(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, ibot_weight=0.0, ibot_mask_ratio=(0.2, 0.4), ibot_mask_prob=0.7, **kw)
    engine.DinoEngine = Spelled
    try:
        for cfg in ("dino_t", "dino_s"):
            got = LT.summary(LT.trace(cfg)[0])
            assert got["names"] == fix[cfg]["names"] and got["sha256"] == fix[cfg]["sha256"], cfg
    finally:
        engine.DinoEngine = real
    # ... and for two micro-batches: the full trace of an engine built without the options
    _, plain, _ = _traced(micro=True)
    _, off, _ = _traced(micro=True, ibot_weight=0.0)
    assert LT.summary(off.events) == LT.summary(plain.events)


@pytest.mark.parametrize("cfg", ["dino_t", "dino_s"])
def test_new_launches_sit_behind_the_writers_of_their_operands(cfg):
    eng, rec, (plan,) = _traced(cfg, plans=[C.fixed_masks(4, 196)], ibot_weight=1.0)
    ev = rec.events
    names = [e[0] for e in ev]
    M = plan.M
    assert [n for n in names if n in NEW] == ["rows_gather", "mask_tokens_fwd", "rows_gather", "ibot_loss", "rows_scatter", "mask_tokens_bwd",
                                              "patch_center_update"]
    # the teacher: its patch rows are gathered, normed and sent through the head INSIDE the side-stream item of the teacher's forward
    b, e = [i for i, x in enumerate(ev) if x[0] == "side.run.begin"], [i for i, x in enumerate(ev) if x[0] == "side.run.end"]
    ig_t = names.index("rows_gather")
    item = next((lo, hi) for lo, hi in zip(b, e) if lo < ig_t < hi)
    tp_logits = _storage(rec, eng.pr_t.hb.logits)
    inside = [i for i in range(*item) if _mentions(ev[i], tp_logits)]
    assert len(inside) == 1 and ev[inside[0]][0] == "linear" and ev[inside[0]][1][3] == M          # the head's last product, on M rows
    xl_t = _storage(rec, eng.g_teach.xbuf(2 * 12))
    assert ev[ig_t][1][0]["tensor"][0] == xl_t and any(_mentions(x, xl_t) for x in ev[item[0]:ig_t])
    assert names[ig_t + 1] == "layernorm_fwd" and ev[ig_t + 1][1][0]["tensor"][0] == _storage(rec, eng.pr_t.x)
    join = next(i for i, x in enumerate(ev) if x[0] == "side.join" and x[1] == ev[item[0]][1])
    # the student: mask tokens behind cls_rows and the patch-embedding product of the global segment, before the first block's norm
    im = names.index("mask_tokens_fwd")
    x0 = _storage(rec, eng.g_stu.x[0])
    assert ev[im][1][0]["tensor"][0] == x0 and ev[im][1][4] == M and ev[im][1][5] == 197
    before = [x[0] for x in ev[:im] if _mentions(x, x0)]
    assert before[-2:] == ["cls_rows", "linear"]
    first_norm = next(i for i in range(im, len(ev)) if ev[i][0] == "layernorm_fwd")
    assert not any(x[0] == "layernorm_fwd" and _mentions(x, x0) for x in ev[:im]) and first_norm > im
    # the loss: behind the teacher's join, the student's patch head and the DINO loss's neighbourhood
    il = names.index("ibot_loss")
    sp_logits = _storage(rec, eng.pr_s.hb.logits)
    assert il > join and any(_mentions(x, sp_logits) and x[0] == "linear" for x in ev[:il])
    assert ev[il][1][0]["tensor"][0] == sp_logits and ev[il][1][1]["tensor"][0] == tp_logits and ev[il][1][8] == M and ev[il][1][12] == "1.0"
    assert names[il - 1] == "dino_loss"
    # backward: the patch rows' norm backward and scatter behind the head's second backward pass, before the first block's backward
    isc = names.index("rows_scatter")
    dfe = _storage(rec, eng.pr_s.hb.dfeats)
    writers = [i for i, x in enumerate(ev) if x[0] == "linear" and x[1][2].get("tensor", [None])[0] == dfe]
    assert len(writers) == 1 and writers[0] < isc
    assert names[isc - 2:isc] == ["layernorm_bwd", "ln_finalize"] and ev[isc - 2][1][0]["tensor"][0] == dfe
    assert ev[isc][1][1]["tensor"][0] == _storage(rec, eng.g_stu.g)
    # mask_tokens_bwd: directly behind the global segment's tokens_bwd, before the patch-embedding weight gradient reads gpatch
    ib = names.index("mask_tokens_bwd")
    assert names[ib - 1] == "tokens_bwd"
    gp = _storage(rec, eng.g_stu.segs[0].gpatch)
    assert ev[ib][1][1]["tensor"][0] == gp and ev[ib - 1][1][1]["tensor"][0] == gp
    later = [x[0] for x in ev[ib + 1:] if _mentions(x, gp)]
    assert later == ["linear"]
    assert names[-1] == "patch_center_update" and names[-2] == "center_update"
    # no CLS-only tail, no q_limit: the last block's attention runs for every query in both groups
    assert all(x[2].get("q_limit", 0) == 0 for x in ev if x[0].startswith("attention"))


def test_no_marked_patch_no_patch_launch():
    eng, rec, _ = _traced(plans=[np.zeros((4, 196), bool)], ibot_weight=1.0)
    names = [e[0] for e in rec.events]
    assert [n for n in names if n in NEW] == ["patch_center_update"]
    # the same launches as a DINO step on every token (GIPVIT_CLS_ONLY_LAST=0), plus the fills of ibot / the sums and the update
    with LT.recording(switches=dict(cls_only_last=False)) as ref:
        from gipvit.engine import DinoEngine
        e2 = DinoEngine(arch="vit_tiny", img_size=224, out_dim=256, batch=2, device="cpu")
        e2.load_state(e2.backbone_state_dict(), e2.head_state_dict())
        e2.load_teacher_state(e2.backbone_state_dict(), e2.head_state_dict(), center=e2.center)
        e2.step(torch.zeros(2, 256, 256, 3, dtype=torch.uint8))
    assert [n for n in names if n not in NEW and n != "Tensor.zero_"] == [e[0] for e in ref.events if e[0] != "Tensor.zero_"]


def test_every_micro_batch_uses_its_own_plan():
    m0, m1 = C.fixed_masks(4, 196, 0), C.fixed_masks(4, 196, 1)
    eng, rec, plans = _traced(micro=True, plans=[m0, m1], ibot_weight=1.0)
    ev = rec.events
    names = [e[0] for e in ev]
    assert plans[0].M != plans[1].M
    for n, per in (("mask_tokens_fwd", 1), ("mask_tokens_bwd", 1), ("ibot_loss", 1), ("rows_scatter", 1), ("rows_gather", 2)):
        calls = [e for e in ev if e[0] == n]
        assert len(calls) == 2 * per, n
    fw = [e for e in ev if e[0] == "mask_tokens_fwd"]
    assert [e[1][4] for e in fw] == [plans[0].M, plans[1].M]
    assert fw[0][1][3]["tensor"][0] != fw[1][1][3]["tensor"][0]                    # two row tables
    assert [e[1][8] for e in ev if e[0] == "ibot_loss"] == [plans[0].M, plans[1].M]
    assert names.count("patch_center_update") == 1 and names.count("dino_loss") == 2
    _, plain, _ = _traced(micro=True, ibot_weight=1.0, plans=[np.zeros((4, 196), bool)] * 2)
    assert [n for n in names if n in NEW] != [e[0] for e in plain.events if e[0] in NEW]
