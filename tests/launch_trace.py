"""The engine's launch sequence, recorded on the CPU (no GPU, no kernel runs).

Every launching function of ``gipvit.ops`` is replaced by a recorder and ``engine.SideStream`` by a stand-in that reports a side
stream and logs what it is asked to do, so an engine built on ``device="cpu"`` walks the code path of a GPU run -- teacher on the
side stream, early ``prepare_backward``, side scratch in the head -- and leaves a trace of every launch, fill and wait:

  [name, args, kwargs]      a call of ``ops.<name>`` or ``Tensor.zero_``; a tensor is [storage number by first appearance,
                            storage offset, shape, strides, dtype], a float its repr, lists / tuples are recorded recursively
  ["side.run.begin", k] ... ["side.run.end", k]      SideStream.run(fn), k its token;  ["side.join", k]: main waits for run k
  ["side.then.begin"] ... ["side.then.end"]       (join(None) waits for nothing -- the event of work that was not queued -- and
                                                   is not an event)

``tests/traces/engine_launches.json`` holds, per configuration, the SHA-256 of the full trace, the event count and the bare name
sequence (tests/test_launch_trace_host.py compares them).

    python tests/launch_trace.py --write       regenerate the fixture from the engine in the tree
    python tests/launch_trace.py --dump DIR    write the full traces (30-270 KB each), one event per line, for a diff

The REDUCED form says "the same launches on the same parameters, gradients and shapes" without fixing their order, the stream
topology or which scratch buffer a launch uses: stream markers and fills are dropped, a tensor inside one of the arena's flat
buffers keeps [buffer name, offset, shape], every other tensor [dtype, shape], a varlen attention call is written as the
per-segment calls it stands for (``ops`` itself splits it that way for f32 operands), and the events are sorted.
"""
import contextlib
import hashlib
import inspect
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "traces", "engine_launches.json")
# pure host helpers of gipvit.ops: they stay real
HOST_HELPERS = {"dropout_site_seed", "dropout_threshold", "range_block_table", "lamb_block_table", "agc_units", "LossScaler",
                "linear_timing", "linear_timing_read", "C_sizeof_augment_params"}
# configurations whose launch ORDER changed on purpose when VitRunner.backward became one loop: they are held to the parent
# commit's recording in the reduced form (their full form is pinned from the single loop on; "before_single_loop" in the
# fixture is the parent's full recording, kept so that the parent's engine.py still passes the test)
REDUCED = ("dino_s_ungrouped", "dino_t_fp32", "sup_t_fp32")
ARENA_BUFFERS = ("p", "g", "m", "v", "pb", "t", "tb")


class Recorder:
    def __init__(self):
        self.events, self.storages, self.keep, self.tokens = [], {}, [], 0

    def enc(self, v):
        if isinstance(v, torch.Tensor):
            self.keep.append(v)          # an address is never reused within a trace
            k = v.untyped_storage().data_ptr()
            n = self.storages.setdefault(k, len(self.storages))
            return {"tensor": [n, v.storage_offset(), list(v.shape), list(v.stride()), str(v.dtype)]}
        if isinstance(v, (list, tuple)):
            return [self.enc(x) for x in v]
        if isinstance(v, float):
            return repr(v)
        if v is None or isinstance(v, (bool, int, str)):
            return v
        raise TypeError(f"launch trace: cannot record a {type(v).__name__} argument")

    def call(self, name, args, kwargs):
        self.events.append([name, [self.enc(a) for a in args], {k: self.enc(v) for k, v in sorted(kwargs.items())}])

    def storage_names(self, arena):
        out = {}
        for nm in ARENA_BUFFERS:
            buf = getattr(arena, nm)
            if buf is not None:
                out[self.storages.get(buf.untyped_storage().data_ptr())] = nm
        out.pop(None, None)
        return out


def launching_ops(ops):
    return sorted(n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__
                  and not n.startswith("_") and n not in HOST_HELPERS)


@contextlib.contextmanager
def recording(switches=None):
    """Patch gipvit.ops, Tensor.zero_, engine.SideStream and EngineSwitches.from_env; yields the Recorder."""
    from gipvit import _lib, engine, ops
    rec = Recorder()
    sw = engine.EngineSwitches(**(switches or {}))

    def recorder(name):
        if name == "linear_ln_bwd":
            def fn(*a, **kw):
                rec.call(name, a, kw)
                return _lib.lib.gv_linear_ln_blocks(a[9])        # M: the engine hands the block count to ln_finalize
        else:
            def fn(*a, **kw):
                rec.call(name, a, kw)
        return fn

    class SideStream:
        def __init__(self, side, pool):
            self.side, self.pool = "side", pool

        def run(self, fn):
            rec.tokens += 1
            k = rec.tokens
            rec.events.append(["side.run.begin", k])
            fn()
            rec.events.append(["side.run.end", k])
            return k

        def then(self, fn):
            rec.events.append(["side.then.begin"])
            fn()
            rec.events.append(["side.then.end"])

        def join(self, ev):
            if ev is not None:
                rec.events.append(["side.join", ev])

    zero_ = torch.Tensor.zero_

    def rec_zero_(self):
        rec.call("Tensor.zero_", (self,), {})
        return zero_(self)

    saved = {n: getattr(ops, n) for n in launching_ops(ops)}
    saved_side, saved_env = engine.SideStream, engine.EngineSwitches.__dict__["from_env"]
    try:
        for n in saved:
            setattr(ops, n, recorder(n))
        torch.Tensor.zero_ = rec_zero_
        engine.SideStream = SideStream
        engine.EngineSwitches.from_env = classmethod(lambda cls: sw)
        yield rec
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
        torch.Tensor.zero_ = zero_
        engine.SideStream = saved_side
        engine.EngineSwitches.from_env = saved_env


# --------------------------------------------------------------------------- #
# configurations: each builds an engine on the CPU, runs it and returns it
# --------------------------------------------------------------------------- #
def _tiles(n, px):
    return torch.zeros(n, px, px, 3, dtype=torch.uint8)


def _dino(arch, batch=1, **kw):
    from gipvit.engine import DinoEngine
    return DinoEngine(arch=arch, img_size=224, out_dim=256, batch=batch, device="cpu", **kw)


def _dino_step(arch, **kw):
    eng = _dino(arch, **kw)
    eng.step(_tiles(1, 256))
    return eng


def dino_t():
    eng = _dino("vit_tiny")
    eng.load_state(eng.backbone_state_dict(), eng.head_state_dict())
    eng.load_teacher_state(eng.backbone_state_dict(), eng.head_state_dict(), center=eng.center)
    eng.step(_tiles(1, 256))
    return eng


def dino_s_g():
    eng = _dino("vit_small", n_local=0, clip_grad=3.0)
    eng.train_last_layer = False
    bg = torch.tensor([[0, y, x, 224, 224, 0] for (y, x) in eng.gwins], dtype=torch.int32)
    eng.step(_tiles(1, 256), boxes=(bg, None))
    return eng


def dino_t_drop():
    eng = _dino("vit_tiny")
    eng.set_dropout(0.1, 7)
    eng.set_drop_path(torch.ones(12, 2, eng.V * eng.B))
    eng.step_micro([_tiles(1, 256), _tiles(1, 256)])
    return eng


def _sup(arch="vit_tiny", batch=2, **kw):
    from gipvit.engine import SupervisedEngine
    return SupervisedEngine(arch=arch, img_size=64, num_classes=2, batch=batch, device="cpu", **kw)


def _sup_step(**kw):
    eng = _sup(**kw)
    eng.step(_tiles(2, 64), torch.zeros(2, 1, dtype=torch.int64))
    return eng


def sup_t():
    eng = _sup()
    eng.load_state(eng.state_dict())
    eng.step(_tiles(2, 64), torch.zeros(2, 1, dtype=torch.int64))
    return eng


def sup_s_ld():
    from gipvit.mixup import MixPlan
    eng = _sup("vit_small", loss="soft_ce", layer_decay=0.75, model_ema_decay=0.99)
    rows = MixPlan.make_rows(2)
    MixPlan.set_row(rows, 0, 0.7, None)
    eng.step(torch.zeros(2, 3, 64, 64), torch.zeros(2, 1, dtype=torch.int64), mix=MixPlan(rows))
    return eng


def fx():
    from gipvit.engine import FeatureExtractor
    eng = FeatureExtractor(arch="vit_small", img_size=64, batch=2, num_classes=2, device="cpu")
    tiles = _tiles(3, 64)                   # a full batch and a padded one
    eng.run_with_attention(tiles)
    eng.last_selfattention(tiles)
    eng.intermediate_layers(tiles, n=2)
    return eng


def _masks(eng, marked):
    """A MaskPlan over the engine's G * B global crops: ``marked`` patches in the first image, none elsewhere."""
    import numpy as np
    from gipvit.masking import MaskPlan
    m = np.zeros((eng.G * eng.B, (eng.gsize // 16) ** 2), np.bool_)
    m[0, 3:3 + marked] = True
    return MaskPlan(m, "cpu")


def dino_s_ibot():
    eng = _dino("vit_small", ibot_weight=1.0)
    eng.step(_tiles(1, 256), masks=_masks(eng, 20))
    return eng


def dino_t_ibot_micro():
    eng = _dino("vit_tiny", ibot_weight=1.0)          # the first micro-batch marks nothing: the M = 0 fills, then the sums
    eng.set_drop_path(torch.ones(12, 2, eng.V * eng.B))
    eng.step_micro([_tiles(1, 256)] * 2, masks=[_masks(eng, 0), _masks(eng, 9)])
    return eng


def dino_s_sk_koleo():
    eng = _dino("vit_small", batch=2, centering="sinkhorn_knopp", koleo_weight=0.1)
    eng.step_micro([_tiles(2, 256)] * 2)
    return eng


def dino_t_views_stains():
    from gipvit.engine import DinoEngine
    from gipvit.multicrop import MultiCropSampler, ViewAugmentSampler
    from gipvit.stain import StainJitterSampler
    eng = DinoEngine(arch="vit_tiny", img_size=224, out_dim=256, batch=2, n_local=2, device="cpu")
    boxes = MultiCropSampler(2, 256, 2, 2, seed=1).sample()
    views = ViewAugmentSampler(2, 2, 2, seed=2).sample()
    stains = StainJitterSampler(2, 2, 2, 0.2, seed=3).sample()
    eng.step(_tiles(2, 256), boxes=boxes)
    eng.step(_tiles(2, 256), boxes=boxes, views=views)
    eng.step(_tiles(2, 256), boxes=boxes, views=views, stains=stains)
    eng.step(_tiles(2, 256), fill=torch.zeros(2, 8))
    eng.step(torch.zeros(2, 3, 256, 256))
    return eng


def _erase_plan():
    from gipvit.erasing import ErasePlan
    rows = ErasePlan.make_rows(2)
    ErasePlan.add_box(rows, 1, (1, 9, 2, 30), (0.5, 0.5, 0.5))
    return ErasePlan(rows, seed=77)


def sup_t_mix_erase():
    from gipvit.mixup import MixPlan
    eng, plan, tgt = _sup(loss="soft_ce"), _erase_plan(), torch.zeros(2, 1, dtype=torch.int64)
    eng.step(_tiles(2, 64), tgt, fill=torch.zeros(2, 8), erase=plan)
    eng.step(torch.zeros(2, 3, 64, 64), tgt, mix=MixPlan(MixPlan.make_rows(2)), erase=plan)
    eng.forward(_tiles(2, 64))
    return eng


def sup_t_avg_drop():
    eng = _sup(global_pool="avg")
    eng.set_dropout(0.1, 5)
    eng.set_drop_path(torch.ones(12, 2, 2))
    eng.step(_tiles(2, 64), torch.zeros(2, 1, dtype=torch.int64))
    return eng


def fx_stain_512():
    from gipvit import ops
    from gipvit.engine import FeatureExtractor
    eng = FeatureExtractor(arch="vit_tiny", img_size=512, batch=1, device="cpu")       # 1025 tokens: the streaming attention forward
    eng.set_stain(torch.zeros(ops._STAIN_PARAMS_BYTES, dtype=torch.uint8))
    eng.run(_tiles(1, 512))
    eng.set_stain(None)
    eng.probe_features(_tiles(1, 512), n_last=2, avgpool=True)
    return eng


def fx_padded():
    """Every batched capture on a padded last batch, float input included."""
    from gipvit.engine import FeatureExtractor
    eng = FeatureExtractor(arch="vit_tiny", img_size=64, batch=2, device="cpu")
    tiles = _tiles(3, 64)
    eng.last_selfattention(tiles, cls_only=True)
    eng.probe_features(tiles, n_last=2, avgpool=True)
    eng.intermediate_layers(tiles, n=3)             # the scratch of probe_features, and one more
    eng.run(torch.zeros(3, 3, 64, 64))
    return eng


# id -> (EngineSwitches fields that differ from the defaults, run)
CONFIGS = {
    "dino_s": ({}, lambda: _dino_step("vit_small")),
    "dino_t": ({}, dino_t),
    "dino_s_g": ({}, dino_s_g),
    "dino_t_drop": ({}, dino_t_drop),
    "dino_s_every_token": (dict(cls_only_last=False), lambda: _dino_step("vit_small")),
    "dino_s_ungrouped": (dict(group_dw=False), lambda: _dino_step("vit_small")),
    "dino_t_fp32": ({}, lambda: _dino_step("vit_tiny", precision="fp32")),
    "sup_t": ({}, sup_t),
    "sup_t_fp32": ({}, lambda: _sup_step(precision="fp32")),
    "sup_s_ld": ({}, sup_s_ld),
    "sup_lamb": ({}, lambda: _sup_step(opt="lamb")),
    "sup_agc_head": ({}, lambda: _sup_step(clip_mode="agc", clip_grad=0.01, train_backbone=False)),
    "fx": ({}, fx),
    "dino_s_ibot": ({}, dino_s_ibot),
    "dino_t_ibot_micro": ({}, dino_t_ibot_micro),
    "dino_s_sk_koleo": ({}, dino_s_sk_koleo),
    "dino_t_views_stains": ({}, dino_t_views_stains),
    "sup_t_mix_erase": ({}, sup_t_mix_erase),
    "sup_t_avg_drop": ({}, sup_t_avg_drop),
    "fx_stain_512": ({}, fx_stain_512),
    "fx_padded": ({}, fx_padded),
    "dino_t_teacher_inline": (dict(teacher_side=False), lambda: _dino_step("vit_tiny")),
    "dino_s_unfused_mlp": (dict(fused_mlp=False), lambda: _dino_step("vit_small")),
    "dino_s_unfused_ln": (dict(fused_ln=False, cls_qlimit=False, varlen_attn=False), lambda: _dino_step("vit_small")),
    "sup_ld_head": ({}, lambda: _sup_step(layer_decay=0.75, train_backbone=False)),
}


def trace(cid):
    """-> (events, {storage number: arena buffer name}) of one configuration."""
    switches, run = CONFIGS[cid]
    with recording(switches) as rec:
        eng = run()
    return rec.events, rec.storage_names(eng.arena)


def _lines(events):
    return [json.dumps(e, sort_keys=True, separators=(",", ":")) for e in events]


def _digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def summary(events):
    return {"sha256": _digest(_lines(events)), "count": len(events), "names": [e[0] for e in events]}


def reduced(events, arena_names):
    """The sorted lines of the reduced form (module docstring)."""
    def red(v):
        if isinstance(v, dict) and "tensor" in v:
            n, off, shape, _, dt = v["tensor"]
            return ["arena", arena_names[n], off, shape] if n in arena_names else [dt, shape]
        if isinstance(v, dict):         # keyword arguments
            return {k: red(x) for k, x in v.items()}
        return [red(x) for x in v] if isinstance(v, list) else v

    def rows(t, r0, n):          # rows [r0, r0 + n) of a contiguous 2-D tensor record
        s, off, shape, strides, dt = t["tensor"]
        return {"tensor": [s, off + r0 * strides[0], [n] + shape[1:], strides, dt]}
    out = []
    for e in events:
        name = e[0]
        if name.startswith("side.") or name == "Tensor.zero_":
            continue
        args, kw = e[1], dict(e[2])
        if name in ("attention_fwd_varlen", "attention_bwd_varlen"):
            ql = kw.pop("q_limit", 0)
            assert not kw, kw
            per_seg, r0 = [], 0
            if name == "attention_fwd_varlen":
                qkv, o, segs, H, scale = args
                for n_img, N, lse in segs:
                    per_seg.append(["attention_fwd", [rows(qkv, r0, n_img * N), n_img, N, H, scale], {"o": rows(o, r0, n_img * N), "lse": lse}])
                    r0 += n_img * N
            else:
                qkv, o, d_o, dqkv, segs, H, scale = args
                for n_img, N, lse in segs:
                    T = n_img * N
                    per_seg.append(["attention_bwd", [rows(qkv, r0, T), rows(o, r0, T), rows(d_o, r0, T), lse, n_img, N, H, scale],
                                    {"dqkv": rows(dqkv, r0, T)}])
                    r0 += T
            for p in per_seg:
                p[2]["q_limit"] = ql
                out.append(p)
            continue
        if name in ("attention_fwd", "attention_bwd"):
            kw.setdefault("q_limit", 0)
        out.append([name, args, kw])
    return sorted(_lines([[n, red(a), red(k)] for n, a, k in out]))


def reduced_summary(events, arena_names):
    lines = reduced(events, arena_names)
    return {"sha256": _digest(lines), "count": len(lines)}


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def main(argv):
    if argv[:1] == ["--dump"] and len(argv) == 2:
        os.makedirs(argv[1], exist_ok=True)
        for cid in CONFIGS:
            events, names = trace(cid)
            with open(os.path.join(argv[1], cid + ".trace"), "w") as f:
                f.write("\n".join(_lines(events)) + "\n")
            if cid in REDUCED:
                with open(os.path.join(argv[1], cid + ".reduced"), "w") as f:
                    f.write("\n".join(reduced(events, names)) + "\n")
            print(f"{cid}: {len(events)} events")
    elif argv == ["--write"]:
        old = load_fixture() if os.path.exists(FIXTURE) else {}
        fix = {}
        for cid in CONFIGS:
            events, names = trace(cid)
            fix[cid] = summary(events)
            if cid in REDUCED:
                fix[cid]["reduced"] = reduced_summary(events, names)
                if "before_single_loop" in old.get(cid, {}):
                    fix[cid]["before_single_loop"] = old[cid]["before_single_loop"]
            print(f"{cid}: {fix[cid]['count']} events {fix[cid]['sha256'][:12]}")
        os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(c)}: {json.dumps(v, separators=(',', ':'))}" for c, v in fix.items()) + "\n}\n")
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
