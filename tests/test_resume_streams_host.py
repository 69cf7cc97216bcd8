"""CPU: the host-side draw streams of a data-parallel run across a resume (checkpoint.pack_host_rng / restore_host_rng), and
the refusals of dist.reduction_plan / dist.comm_setup.

Every rank seeds its own streams (the driver's seeds: checkpoint.HOST_STREAMS through checkpoint.stream_seed).  A checkpoint
is written by rank 0 alone, so before ``host_rng_ranks`` existed it held rank 0's positions only and a resumed world > 1 run
restored them on EVERY rank: from then on all ranks drew the same boxes, masks and seeds."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 42


class Rank:
    """One rank's host draw streams, built as train.py builds them and seeded from the same table."""

    def __init__(self, rank):
        from gipvit.checkpoint import stream_seed
        from gipvit.droppath import DropPathSampler
        from gipvit.masking import MaskSampler
        from gipvit.multicrop import MultiCropSampler
        self.rank = rank
        self.seeds = {k: stream_seed(k, SEED, rank) for k in ("drop", "crops", "ibot", "drop_path")}
        self.crops = MultiCropSampler(2, 256, 2, 3, seed=self.seeds["crops"])
        self.masks = MaskSampler(14, 4, (0.1, 0.5), 0.5, seed=self.seeds["ibot"])
        self.drop = np.random.default_rng(self.seeds["drop"])
        self.dp = DropPathSampler(12, 10, 0.1, self.seeds["drop_path"], "cpu")

    def streams(self):      # the driver's names; streams a run does not use are None there
        return {"drop": self.drop, "crops": self.crops.rng, "views": None, "mix": None, "erase": None, "ibot": self.masks.rng}

    def draw(self):
        """One step's draws, as arrays: crop boxes (global, local), iBOT masks, the dropout seed, the stochastic-depth factors."""
        bg, bl = self.crops.sample()
        return [bg.numpy().copy(), bl.numpy().copy(), self.masks.sample().masks.copy(), np.array(int(self.drop.integers(0, 1 << 32))),
                self.dp.sample().numpy().copy()]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def saved_run(steps=3):
    """Two ranks draw ``steps`` steps and pack -> (the checkpoint entries as rank 0 writes them, each rank's NEXT draws)."""
    from gipvit.checkpoint import pack_host_rng
    ranks = [Rank(0), Rank(1)]
    for r in ranks:
        for _ in range(steps):
            r.draw()
    def gather_of(r):       # the fake all_gather: a rank hands in its own entry and gets the list of all of them
        def gather(obj):
            return [obj if q == r else _peer_entry(ranks[q]) for q in range(2)]
        return gather
    packed = [pack_host_rng(r.streams(), r.dp, gather_of(r.rank)) for r in ranks]
    assert packed[0]["host_rng_ranks"] == packed[1]["host_rng_ranks"]          # every rank sees the same gathered list
    cont = [r.draw() for r in ranks]
    return packed[0], cont


def _peer_entry(r):
    from gipvit.checkpoint import _stream_states
    return dict(_stream_states(r.streams()), drop_path_rng=r.dp.state_dict())


def test_each_rank_continues_its_own_streams_across_a_resume(tmp_path):
    """Rank r of the resumed run draws what rank r of the uninterrupted run draws next -- crop boxes through
    MultiCropSampler.sample, iBOT masks, the dropout step seed, the stochastic-depth factors -- the two ranks' draws differ, the
    flat entries are rank 0's in the form they always had, and the whole entry survives torch.save / load(weights_only=True)."""
    from gipvit.checkpoint import restore_host_rng
    ex, cont = saved_run()
    assert not same(cont[0], cont[1])
    assert ex["host_rng_ranks"]["world"] == 2 and len(ex["host_rng_ranks"]["states"]) == 2
    assert ex["host_rng"] == {k: v for k, v in ex["host_rng_ranks"]["states"][0].items() if k != "drop_path_rng"}
    assert sorted(ex["host_rng"]) == ["crops", "drop", "ibot"] and all(isinstance(v, str) for v in ex["host_rng"].values())
    assert ex["drop_path_rng"] == ex["host_rng_ranks"]["states"][0]["drop_path_rng"] and sorted(ex["drop_path_rng"]) == ["k", "rng"]
    torch.save(dict(ex, epoch=0), tmp_path / "ck.pth")
    ck = torch.load(tmp_path / "ck.pth", weights_only=True)
    assert ck["host_rng_ranks"] == ex["host_rng_ranks"] and ck["host_rng"] == ex["host_rng"]
    got = []
    for rank in range(2):
        r = Rank(rank)
        assert restore_host_rng(ck, r.streams(), r.dp, rank, 2, 1, seeds=r.seeds) == "ranks"
        got.append(r.draw())
        assert same(got[rank], cont[rank]), rank
    assert not same(got[0], got[1])


def test_single_rank_forms_restore_as_ever():
    """World size 1: a checkpoint with the flat entries only (every checkpoint before ``host_rng_ranks``) restores them, one
    written at world size 1 with the per-rank entry restores the same state, and one without any entry changes nothing."""
    from gipvit.checkpoint import pack_host_rng, restore_host_rng
    r = Rank(0)
    r.draw()
    ex = pack_host_rng(r.streams(), r.dp, lambda o: [o])
    cont = r.draw()
    old = {"host_rng": ex["host_rng"], "drop_path_rng": ex["drop_path_rng"]}
    for ck, how in ((old, "flat"), (ex, "ranks")):
        q = Rank(0)
        assert restore_host_rng(ck, q.streams(), q.dp, 0, 1, 1, seeds=q.seeds) == how
        assert same(q.draw(), cont)
    q = Rank(0)
    assert restore_host_rng({}, q.streams(), q.dp, 0, 1, 0) == "flat"
    assert same(q.draw(), Rank(0).draw())


def test_old_format_checkpoint_at_world_2_keeps_the_ranks_apart():
    """A checkpoint with rank 0's flat entries only, resumed by two ranks.  The driver used to restore the flat entries on every
    rank (this test FAILS on that code: both ranks then hold rank 0's streams and draw identical boxes, masks and seeds for the
    rest of the run).  Now nothing is restored: each rank restarts from (its own seed, the start epoch) -- apart from the other
    rank, and not replaying epoch 0 -- and the primary warns once."""
    from gipvit.checkpoint import restore_host_rng
    ex, _ = saved_run()
    old = {"host_rng": ex["host_rng"], "drop_path_rng": ex["drop_path_rng"]}
    was = []        # what the driver did: the flat entries into every rank's streams
    for rank in range(2):
        r = Rank(rank)
        for k, g in r.streams().items():
            if g is not None:
                g.bit_generator.state = json.loads(old["host_rng"][k])
        r.dp.load_state_dict(old["drop_path_rng"])
        was.append(r.draw())
    assert same(was[0], was[1])         # the fault: one stream for both ranks
    warned, got = [], []
    for rank in range(2):
        r = Rank(rank)
        assert restore_host_rng(old, r.streams(), r.dp, rank, 2, 5, seeds=r.seeds, warn=warned.append) == "reseeded"
        got.append(r.draw())
    assert len(warned) == 1 and "rank 0 only" in warned[0] and "not restored" in warned[0]
    for i in range(5):      # every stream, one by one: no pair of ranks shares one
        assert not np.array_equal(got[0][i], got[1][i]), i
    for rank in range(2):
        fresh = Rank(rank).draw()
        for i in range(5):
            assert not np.array_equal(got[rank][i], fresh[i]), (rank, i)           # not epoch 0's draws again
        again = Rank(rank)          # deterministic in (seed, epoch), and another epoch is another stream
        restore_host_rng(old, again.streams(), again.dp, rank, 2, 5, seeds=again.seeds)
        assert same(again.draw(), got[rank])
        other = Rank(rank)
        restore_host_rng(old, other.streams(), other.dp, rank, 2, 6, seeds=other.seeds)
        assert not same(other.draw(), got[rank])


def test_world_size_mismatch_restores_nothing_and_warns():
    """Saved by two ranks, resumed by one or by three: no rank's state is taken (rank 2 has none, and a lone rank that took
    rank 0's would silently drop rank 1's half of the data order): re-seeded, one warning on the primary."""
    from gipvit.checkpoint import restore_host_rng
    ex, cont = saved_run()
    for world in (1, 3):
        warned, got = [], []
        for rank in range(world):
            r = Rank(rank)
            assert restore_host_rng(ex, r.streams(), r.dp, rank, world, 2, seeds=r.seeds, warn=warned.append) == "reseeded"
            got.append(r.draw())
            assert not any(same(got[-1], c) for c in cont)
        assert len(warned) == 1 and "of 2 ranks" in warned[0] and f"has {world}" in warned[0]
        for i in range(world):
            for j in range(i):
                assert not same(got[i], got[j])
    r = Rank(0)
    with pytest.raises(KeyError, match="crops"):        # a stream without a seed is refused, not left where it was
        restore_host_rng(ex, r.streams(), r.dp, 0, 1, 2, seeds={"drop": 1})


def _gather_worker(rank, world, port, q):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from gipvit.checkpoint import pack_host_rng
    from test_resume_streams_host import Rank
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def gather(obj):        # the driver's gather_ranks
        out = [None] * world
        dist.all_gather_object(out, obj)
        return out
    r = Rank(rank)
    for _ in range(2 + rank):       # the ranks need not be at the same position
        r.draw()
    ex = pack_host_rng(r.streams(), r.dp, gather)
    q.put((rank, json.dumps(ex, sort_keys=True), [x.tolist() for x in r.draw()]))
    dist.destroy_process_group()


def test_pack_gathers_over_gloo_with_two_processes():
    """The real collective: two processes, all_gather_object over gloo.  Both get the same entry, and states[r] continues rank r."""
    import socket
    import torch.multiprocessing as mp
    from gipvit.checkpoint import restore_host_rng
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ps = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    try:
        res = sorted([q.get(timeout=120) for _ in ps], key=lambda t: t[0])
        [p.join(60) for p in ps]
        assert not any(p.is_alive() for p in ps)
    finally:
        [p.terminate() for p in ps if p.is_alive()]
    assert res[0][1] == res[1][1]
    ck = json.loads(res[0][1])
    assert ck["host_rng_ranks"]["world"] == 2
    for rank in range(2):
        r = Rank(rank)
        assert restore_host_rng(ck, r.streams(), r.dp, rank, 2, 1, seeds=r.seeds) == "ranks"
        assert [x.tolist() for x in r.draw()] == res[rank][2]


def _pack_sites(src):
    """-> (line numbers of the pack_host_rng calls reachable from ``main``, those of them under a gate, the functions entered).  The
    walk starts at ``main`` and follows its calls into the module's own functions, carrying the gate of the call site along.  A gate
    is an ``if`` (either branch) whose test names ``saver`` / ``primary``, bare or as an attribute (``run.saver``, ``ctx.primary``),
    and everything in a block behind such an ``if`` that can leave the block (return / break / continue / raise)."""
    import ast
    funcs = {n.name: n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}
    gated, calls, entered = set(), [], {"main"}
    is_gate = lambda test: any((isinstance(n, ast.Name) and n.id in ("saver", "primary")) or (isinstance(n, ast.Attribute) and n.attr in ("saver", "primary"))
                               for n in ast.walk(test))
    leaves = lambda st: any(isinstance(n, (ast.Return, ast.Break, ast.Continue, ast.Raise)) for n in ast.walk(st))

    def walk(node, g):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name):
            if node.func.id == "pack_host_rng":
                calls.append(node.lineno)
                if g:
                    gated.add(node.lineno)
            elif node.func.id in funcs and node.func.id not in entered:
                entered.add(node.func.id)
                walk(funcs[node.func.id], g)
        for field, value in ast.iter_fields(node):
            if isinstance(value, list) and value and isinstance(value[0], ast.stmt):
                gg = g or (isinstance(node, ast.If) and is_gate(node.test))
                for st in value:
                    walk(st, gg)
                    gg = gg or (isinstance(st, ast.If) and is_gate(st.test) and leaves(st))
            else:
                for ch in (value if isinstance(value, list) else [value]):
                    if isinstance(ch, ast.AST):
                        walk(ch, g or (isinstance(node, ast.If) and field != "test" and is_gate(node.test)))
    walk(funcs["main"], False)
    return calls, gated, entered


def test_driver_packs_on_every_rank_and_writes_on_the_primary():
    """train.py: pack_host_rng (a collective at world > 1) is called outside every ``saver is not None`` / ``primary`` gate, at both
    save points, and the old rank-0-only restore is gone.  The save points sit in the stages ``main`` calls; the walk follows it there."""
    src = open(os.path.join(ROOT, "train.py")).read()
    calls, gated, entered = _pack_sites(src)
    assert len(calls) == 2 and not gated, (calls, gated)
    assert {"train_epoch", "end_of_epoch"} <= entered
    assert "restore_host_rng(ck," in src and 'ck["host_rng"]' not in src and 'ck.get("drop_path_rng")' not in src
    # the walk sees every form of the gate: attribute tests, a gated call site of the stage, an early return ahead of the call
    stage = "def main():\n    stage(run)\n\n\ndef stage(run):\n"
    for body in ("    if run.saver is not None:\n        x = pack_host_rng(s, d, g)\n", "    if ctx.primary:\n        x = pack_host_rng(s, d, g)\n",
                 "    if saver is None:\n        pass\n    else:\n        x = pack_host_rng(s, d, g)\n",
                 "    if not run.primary:\n        return\n    x = pack_host_rng(s, d, g)\n",
                 "    for i in r:\n        if not ctx.primary:\n            continue\n        x = pack_host_rng(s, d, g)\n"):
        assert _pack_sites(stage + body)[:2] == ([6 + body.count("\n") - 1], {6 + body.count("\n") - 1}), body
    assert _pack_sites("def main():\n    if primary:\n        stage(run)\n\n\ndef stage(run):\n    x = pack_host_rng(s, d, g)\n")[:2] == ([7], {7})
    assert _pack_sites(stage + "    if args.recovery_interval:\n        x = pack_host_rng(s, d, g)\n    if not run.primary:\n        return\n")[:2] == ([7], set())
    # and on the driver itself: either save point moved under either gate is found
    lines = src.splitlines()
    for at in calls:
        pad = lines[at - 1][:len(lines[at - 1]) - len(lines[at - 1].lstrip())]
        for gate in ("if run.saver is not None:", "if run.primary:"):
            moved = "\n".join(lines[:at - 1] + [pad + gate, "    " + lines[at - 1]] + lines[at:])
            assert _pack_sites(moved)[:2] == ([c + (c >= at) for c in calls], {at + 1}), (at, gate)


def test_reduction_plan_refuses_a_layout_that_is_not_in_backward_order():
    """dist.reduction_plan: the head range is issued from offset 0, so a head that does not open the arena is refused (whatever
    lay in front of it would be reduced before it is final), and so is any block span in front of the range released before it --
    the LAST block's included, which the loop used to leave unchecked."""
    from gipvit.dist import reduction_plan
    assert reduction_plan((0, 50), {1: (50, 80), 0: (80, 100)}, 130, bucket_bytes=0) == [("head", 0, 50), (1, 50, 80), ("end", 80, 130)]
    with pytest.raises(AssertionError, match="open the arena"):
        reduction_plan((10, 50), {1: (50, 80), 0: (80, 100)}, 130)
    with pytest.raises(AssertionError, match="backward-completion order"):
        reduction_plan((0, 50), {1: (50, 80), 0: (40, 50)}, 130)            # the last block, inside the head range
    with pytest.raises(AssertionError, match="backward-completion order"):
        reduction_plan((0, 50), {2: (50, 80), 1: (80, 100), 0: (60, 70)}, 130, bucket_bytes=0)      # ... inside a released block range
    with pytest.raises(AssertionError, match="backward-completion order"):
        reduction_plan((0, 50), {1: (40, 80), 0: (80, 100)}, 130)
    with pytest.raises(AssertionError, match="backward-completion order"):
        reduction_plan(None, {0: (0, 100), 1: (100, 130)}, 130)             # ascending block order is forward order


def test_comm_setup_refuses_a_budget_the_library_would_ignore(monkeypatch):
    """dist.comm_setup: GIPVIT_COMM_CUS outside 0..192 (the library sizes for the whole chip below a budget of 64 CUs while the
    log would report the request) or not an integer is a ValueError that names the variable; the edges 0 and 192 pass."""
    from gipvit.dist import comm_setup
    for k in ("GIPVIT_COMM_CUS", "NCCL_MAX_NCHANNELS", "NCCL_MIN_NCHANNELS"):
        monkeypatch.setenv(k, "")           # (so that what comm_setup itself sets is undone with the test)
        monkeypatch.delenv(k)
    monkeypatch.setenv("GIPVIT_CU_BUDGET", "64")          # set by the caller, so the call does not depend on whether the library is loaded
    for bad in ("193", "256", "-1", "8.5", "eight", ""):
        monkeypatch.setenv("GIPVIT_COMM_CUS", bad)
        with pytest.raises(ValueError, match="GIPVIT_COMM_CUS"):
            comm_setup(2, "nccl")
        assert "NCCL_MAX_NCHANNELS" not in os.environ
        assert comm_setup(1, "nccl")["comm_cus"] == 0 and comm_setup(2, "gloo")["comm_cus"] == 0      # not read where it has no effect
    monkeypatch.setenv("GIPVIT_COMM_CUS", "192")
    assert comm_setup(2, "nccl")["comm_cus"] == 192 and os.environ["NCCL_MAX_NCHANNELS"] == "192"
    monkeypatch.setenv("GIPVIT_COMM_CUS", "0")
    assert comm_setup(2, "nccl")["comm_cus"] == 0
