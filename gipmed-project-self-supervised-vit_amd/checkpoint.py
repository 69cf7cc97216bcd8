"""Checkpoint files in the layout the reference writes through timm's CheckpointSaver
(reference train.py:867-877, 970-973): ``checkpoint-<epoch>.pth.tar``,
``last.pth.tar``, ``model_best.pth.tar``, ``recovery-<epoch>-<batch>.pth.tar`` holding
``{'epoch', 'arch', 'state_dict', 'optimizer', 'version': 2, 'args', 'metric', 'state_dict_ema'}``
(``state_dict_ema`` = timm's key for the ``--model-ema`` copy; a DINO run stores its teacher there, plus ``dino_center``).

Deviation (documented): ``'args'`` is stored as a plain dict, not a pickled Namespace, and
the optimizer state as tensors, so every file loads with ``torch.load(weights_only=True)``.
"""
from __future__ import annotations

import os
import shutil
from typing import Dict, Optional

import torch


class CheckpointSaver:
    def __init__(self, checkpoint_dir: str, arch: str, args: Optional[dict] = None, decreasing: bool = False, max_history: int = 10):
        self.dir, self.arch, self.args, self.decreasing, self.max_history = checkpoint_dir, arch, dict(args or {}), decreasing, max_history
        os.makedirs(checkpoint_dir, exist_ok=True)
        self.history = []            # (path, metric)
        self.best_metric, self.best_epoch = None, None

    def _payload(self, epoch, state_dict, optimizer, metric, extra):
        p = {"epoch": epoch, "arch": self.arch, "state_dict": {k: v.detach().cpu() for k, v in state_dict.items()}, "version": 2,
             "args": {k: v for k, v in self.args.items() if isinstance(v, (int, float, str, bool, type(None), list, tuple))}}
        if optimizer is not None:
            p["optimizer"] = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in optimizer.items()}
        if metric is not None:
            p["metric"] = float(metric)
        for k, v in (extra or {}).items():       # e.g. 'state_dict_ema' (timm key: the EMA model / DINO teacher), 'dino_center'
            cpu = lambda t: t.detach().cpu() if torch.is_tensor(t) else t          # (plain str / int entries, e.g. a sampler's stream position, pass through)
            p[k] = {n: cpu(t) for n, t in v.items()} if isinstance(v, dict) else cpu(v)
        return p

    def save_checkpoint(self, epoch: int, state_dict: Dict[str, torch.Tensor], optimizer: Optional[dict] = None,
                        metric: Optional[float] = None, extra: Optional[dict] = None):
        last = os.path.join(self.dir, "last.pth.tar")
        torch.save(self._payload(epoch, state_dict, optimizer, metric, extra), last)
        path = os.path.join(self.dir, f"checkpoint-{epoch}.pth.tar")
        shutil.copyfile(last, path)
        self.history.append((path, metric))
        better = metric is not None and (self.best_metric is None or (metric < self.best_metric if self.decreasing else metric > self.best_metric))
        if better:
            self.best_metric, self.best_epoch = metric, epoch
            shutil.copyfile(last, os.path.join(self.dir, "model_best.pth.tar"))
        while len(self.history) > self.max_history:
            old, _ = self.history.pop(0)
            if os.path.exists(old):
                os.remove(old)
        return self.best_metric, self.best_epoch

    def save_recovery(self, epoch: int, batch_idx: int, state_dict, optimizer=None, extra: Optional[dict] = None):
        path = os.path.join(self.dir, f"recovery-{epoch}-{batch_idx}.pth.tar")
        torch.save(self._payload(epoch, state_dict, optimizer, None, dict(extra or {}, batch_idx=batch_idx)), path)
        return path


# --------------------------------------------------------------------------- #
# the host-side draw streams of a run (dropout step seeds, crop boxes, view augmentation, mixup, erasing, iBOT masks,
# stochastic depth): every rank has its own, seeded from (seed, rank) by the table below -- stream -> (rank multiplier, offset), for the
# samplers and a re-seeding resume alike ("drop_path": the DropPathSampler's) --, and a checkpoint holds every rank's position
# --------------------------------------------------------------------------- #
HOST_STREAMS = {"crops": (1, 0), "drop": (7919, 11), "views": (53, 5), "stain": (313, 41), "mix": (101, 23), "erase": (211, 37),
                "ibot": (101, 3), "drop_path": (17, 0)}


def stream_seed(name: str, seed: int, rank: int) -> int:
    mul, off = HOST_STREAMS[name]
    return seed + mul * rank + off


def _stream_states(streams) -> dict:
    import json
    return {k: json.dumps(g.bit_generator.state) for k, g in streams.items() if g is not None}


def pack_host_rng(streams, drop_sampler, gather) -> dict:
    """The checkpoint entries of the host draw streams.  ``streams``: {name: numpy Generator or None} of THIS rank,
    ``drop_sampler``: its DropPathSampler or None, ``gather(obj) -> [rank 0's obj, rank 1's, ...]`` (the identity list at world
    size 1, ``all_gather_object`` otherwise: a collective, so EVERY rank calls this at every save point and only the write is
    the primary's).  ``host_rng`` / ``drop_path_rng`` are rank 0's streams in the flat form single-process checkpoints always
    had; ``host_rng_ranks`` = {"world": W, "states": [per rank: its host_rng entries, plus "drop_path_rng" with a sampler]}.
    Plain dict / list / str / int throughout: loads with ``weights_only=True``."""
    mine = _stream_states(streams)
    if drop_sampler is not None:
        mine["drop_path_rng"] = drop_sampler.state_dict()
    states = [dict(s) for s in gather(mine)]
    ex = {"host_rng": {k: v for k, v in states[0].items() if k != "drop_path_rng"}}
    if "drop_path_rng" in states[0]:
        ex["drop_path_rng"] = dict(states[0]["drop_path_rng"])
    ex["host_rng_ranks"] = {"world": len(states), "states": states}
    return ex


def _load_streams(st: dict, streams, drop_sampler):
    import json
    for k, g in streams.items():
        if g is not None and k in st:
            g.bit_generator.state = json.loads(st[k])
    if drop_sampler is not None and isinstance(st.get("drop_path_rng"), dict):
        drop_sampler.load_state_dict(st["drop_path_rng"])


def restore_host_rng(ck: dict, streams, drop_sampler, rank: int, world: int, start_epoch: int, seeds: Optional[dict] = None, warn=None) -> str:
    """Continue this rank's draw streams from checkpoint ``ck`` -> what was done:
    "ranks": ``host_rng_ranks`` of the same world size, rank r takes ``states[r]``;
    "flat": world size 1 and the flat entries only (rank 0's streams, the single-process form), as ever;
    "reseeded": anything else with a second rank involved (another world size, or a checkpoint without per-rank states at
    world > 1, whose flat entries are rank 0's: restored everywhere they would make every rank draw the same boxes, masks and
    seeds from then on).  Nothing is restored; every stream restarts from (its per-rank seed in ``seeds`` -- "drop_path" for the
    sampler --, ``start_epoch``), so the ranks neither share their draws nor replay epoch 0, and ``warn`` is told once, on rank 0."""
    import numpy as np
    per = ck.get("host_rng_ranks")
    if isinstance(per, dict) and int(per.get("world", -1)) == world and len(per.get("states", ())) == world:
        _load_streams(per["states"][rank], streams, drop_sampler)
        return "ranks"
    if world == 1 and not isinstance(per, dict):
        flat = dict(ck["host_rng"]) if isinstance(ck.get("host_rng"), dict) else {}
        if isinstance(ck.get("drop_path_rng"), dict):
            flat["drop_path_rng"] = ck["drop_path_rng"]
        _load_streams(flat, streams, drop_sampler)
        return "flat"
    seeds = seeds or {}
    for k, g in list(streams.items()) + [("drop_path", getattr(drop_sampler, "rng", None))]:
        if g is not None:
            if k not in seeds:
                raise KeyError(f"restore_host_rng: no per-rank seed for the {k!r} stream")
            g.bit_generator.state = np.random.default_rng([int(start_epoch), int(seeds[k])]).bit_generator.state
    if rank == 0 and warn is not None:
        saved = f"of {int(per.get('world', 0))} ranks" if isinstance(per, dict) else "of rank 0 only"
        warn(f"--resume: the checkpoint holds the host draw streams {saved}, this run has {world}: they are not restored; every rank's "
             f"streams restart from (its own seed, epoch {start_epoch})")
    return "reseeded"


def load_checkpoint_file(path: str) -> dict:
    """Never executes anything from the file."""
    return torch.load(path, map_location="cpu", weights_only=True)
