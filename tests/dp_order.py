"""Stream-order checker for the data-parallel step, over the CPU launch trace (tests/launch_trace.py).

An engine built on ``device="cpu"`` inside ``launch_trace.recording()`` with a ``RecordingReducer`` (world 2) leaves a trace in
which every launch, fill, side-stream marker AND every call of the reducer appears in host order:

  ["reduce_range", lo, hi]   ["reduce_tensor", <tensor record>]   ["reduce_max", <tensor record>]   ["finish"]
  ["micro", j, n] / ["optimizer"]      markers put in by ``instrument()`` around forward_backward / optimizer_step

STREAM MODEL.  Two streams.  An event between ``side.run.begin k`` / ``side.run.end k`` or between ``side.then.begin`` /
``side.then.end`` is on the side stream, everything else on main.  ``side.run.begin``: side has seen every earlier main event
(and what main had seen).  ``side.join k``: main has seen every side event up to ``side.run.end k``.  ``side.then``: no edge.  A
collective (``reduce_*``) waits for the stream it was issued on, at that point, and is an event on a stream of its own.
``finish`` (on main): main has seen every earlier collective and what each of them had seen.

Every event carries a clock {main, side, coll}: the trace index of the last event of each stream it is ordered behind.  Event
``a`` (earlier in the trace) happens before ``b`` iff ``clock(b)[stream(a)] >= index(a)``; a later event never happens before
an earlier one (the host issues in trace order and the streams are FIFO).

An ACCESS is a recorded launch (or ``Tensor.zero_``) with a tensor argument; its range in that tensor's storage is
[offset, offset + extent).  Every access counts as a write: conservative, and right for the gradient arena, which is only
written and accumulated until the optimizer reads it.

``check(trace)`` -> list of violations, each a string that names the property and the two events:
  P1  two accesses to overlapping ranges of ``g`` on different streams are ordered
  P2  every access overlapping a collective's range that precedes it in the trace happens before the collective
  P3  no access overlaps a collective's range between its issue and the next ``finish`` (nor does a second collective)
  P4  per optimizer step the ``reduce_range`` calls are ``plan`` (dist.reduction_plan's output), in that order, tile [0, n)
      once, and none is issued before the step's last micro-batch
  P5  P2 / P3 for the tensors handed to ``reduce_tensor`` / ``reduce_max`` (the same code path: a collective is a collective),
      and their first consumer (``center_update``, ``patch_center_update``, the next Sinkhorn pass) comes after a ``finish``
      -- which P3 implies, since the consumer is an access
  P6  ``finish`` is on main, and no optimizer launch that touches ``g`` (sumsq, adamw_ema*, lamb, agc) runs while a collective is
      pending
"""
import dataclasses

MARKERS = ("side.run.begin", "side.run.end", "side.join", "side.then.begin", "side.then.end")
COLLECTIVES = ("reduce_range", "reduce_tensor", "reduce_max")
OPTIMIZER = ("sumsq", "adamw_ema", "adamw_ema_ranges", "lamb", "agc")


class RecordingReducer:
    """The reducer an engine under ``launch_trace.recording()`` is built with: world 2, every call becomes a trace event."""
    world, rank = 2, 0

    def __init__(self, rec):
        self.rec = rec

    def reduce_range(self, buf, lo, hi):
        self.rec.enc(buf)       # (the arena's storage gets its number even if no launch has named it yet)
        self.rec.events.append(["reduce_range", lo, hi])

    def reduce_tensor(self, t):
        self.rec.events.append(["reduce_tensor", self.rec.enc(t)])

    def reduce_max(self, t):
        self.rec.events.append(["reduce_max", self.rec.enc(t)])

    def finish(self):
        self.rec.events.append(["finish"])


def instrument(eng, rec):
    """Mark the micro-batches and the optimizer steps of ``eng`` in the trace (wrappers on the instance: the engine's code is as it is)."""
    fb, opt = eng.forward_backward, eng.optimizer_step

    def forward_backward(*a, **kw):
        j, n = kw.get("micro", (0, 1))
        rec.events.append(["micro", j, n])
        return fb(*a, **kw)

    def optimizer_step(*a, **kw):
        rec.events.append(["optimizer"])
        return opt(*a, **kw)
    eng.forward_backward, eng.optimizer_step = forward_backward, optimizer_step
    return eng


@dataclasses.dataclass
class Trace:
    events: list        # the recording
    g: int              # storage number of arena.g
    n: int              # arena.n
    plan: list          # [(lo, hi)] of one step, from dist.reduction_plan


def tensor_ranges(v, out):
    """Every tensor record inside a recorded argument -> (storage, lo, hi) appended to ``out``."""
    if isinstance(v, dict) and "tensor" in v:
        s, off, shape, strides, _ = v["tensor"]
        if all(n > 0 for n in shape):
            out.append((s, off, off + 1 + sum((n - 1) * abs(st) for n, st in zip(shape, strides))))
    elif isinstance(v, dict):
        for x in v.values():
            tensor_ranges(x, out)
    elif isinstance(v, list):
        for x in v:
            tensor_ranges(x, out)


@dataclasses.dataclass
class Ev:
    i: int              # trace index
    name: str
    stream: str         # "main" | "side" | "coll"
    clock: dict         # {"main": i, "side": j, "coll": k}
    ranges: list        # [(storage, lo, hi)]

    def __str__(self):
        return f"#{self.i} {self.name} [{self.stream}] " + ",".join(f"s{s}:{lo}-{hi}" for s, lo, hi in self.ranges[:3])


def before(a: Ev, b: Ev) -> bool:
    """``a`` (earlier in the trace) happens before ``b``."""
    assert a.i < b.i
    return b.clock[a.stream] >= a.i


def overlap(a: Ev, b: Ev, storage=None):
    return any(sa == sb and (storage is None or sa == storage) and la < hb and lb < ha for sa, la, ha in a.ranges for sb, lb, hb in b.ranges)


def replay(tr: Trace):
    """-> (accesses and collectives as Ev, in trace order; violations of the model itself)."""
    clock = {"main": {"main": -1, "side": -1, "coll": -1}, "side": {"main": -1, "side": -1, "coll": -1}}
    run_end, open_runs, in_then, pending, out, bad = {}, [], False, [], [], []
    for i, e in enumerate(tr.events):
        name = e[0]
        cur = "side" if (open_runs or in_then) else "main"
        if name == "side.run.begin":
            for k in clock["main"]:         # side has seen every earlier main event, and what main had seen
                clock["side"][k] = max(clock["side"][k], clock["main"][k])
            open_runs.append(e[1])
        elif name == "side.run.end":
            assert open_runs.pop() == e[1]
            run_end[e[1]] = dict(clock["side"])
        elif name == "side.join":
            for k, v in run_end[e[1]].items():
                clock["main"][k] = max(clock["main"][k], v)
        elif name == "side.then.begin":
            in_then = True
        elif name == "side.then.end":
            in_then = False
        elif name in ("micro", "optimizer"):
            continue
        elif name == "finish":
            if cur != "main":
                bad.append(f"P6: #{i} finish is issued on the side stream")
            for c in pending:
                for k, v in c.clock.items():
                    clock["main"][k] = max(clock["main"][k], v)
                clock["main"]["coll"] = max(clock["main"]["coll"], c.i)
            pending = []
        elif name in COLLECTIVES:
            ranges = []
            if name == "reduce_range":
                ranges.append((tr.g, e[1], e[2]))
            else:
                tensor_ranges(e[1], ranges)
            clock[cur][cur] = i
            c = Ev(i, name, "coll", dict(clock[cur]), ranges)
            c.issued_on = cur
            pending.append(c)
            out.append(c)
        else:
            ranges = []
            tensor_ranges(e[1], ranges)
            tensor_ranges(e[2], ranges)
            clock[cur][cur] = i
            out.append(Ev(i, name, cur, dict(clock[cur]), ranges))
    assert not open_runs and not in_then
    return out, bad


def check(tr: Trace, properties=("P1", "P2", "P3", "P4", "P5", "P6")):
    evs, bad = replay(tr)
    nfin = [0]
    for e in tr.events:         # finishes in events[:i]
        nfin.append(nfin[-1] + (e[0] == "finish"))
    bad = bad if "P6" in properties else []
    acc = [e for e in evs if e.stream != "coll"]
    g_acc = [e for e in acc if any(s == tr.g for s, _, _ in e.ranges)]
    if "P1" in properties:
        for x, a in enumerate(g_acc):
            for b in g_acc[x + 1:]:
                if a.stream != b.stream and overlap(a, b, tr.g) and not before(a, b):
                    bad.append(f"P1: {a} and {b} touch the same gradients and are not ordered")
    # P2 / P3 (P5: the same for the small tensors), P6: walk the trace with the set of collectives in flight
    pending = []
    for e in evs:
        if e.stream == "coll":
            tag = "P2" if e.name == "reduce_range" else "P5"
            if tag == "P2" and "P2" in properties or tag == "P5" and "P5" in properties:
                for a in acc:
                    if a.i > e.i:
                        break
                    if overlap(a, e) and not before(a, e):
                        bad.append(f"{tag}: {a} is not ordered before {e}, issued on {e.issued_on}")
            for c in pending:
                if overlap(c, e) and "P3" in properties:
                    bad.append(f"P3: {e} is issued while {c} is in flight on the same range")
            pending.append(e)
            continue
        # an access: which finish it follows is positional
        pending = [c for c in pending if nfin[e.i] == nfin[c.i + 1]]
        for c in pending:
            tag = "P3" if c.name == "reduce_range" else "P5"
            if tag in properties and overlap(c, e):
                bad.append(f"{tag}: {e} touches the range of {c} before the next finish")
        if "P6" in properties and e.name in OPTIMIZER and e in g_acc:
            if e.stream != "main":
                bad.append(f"P6: {e} is an optimizer launch on the side stream")
            for c in pending:
                bad.append(f"P6: {e} runs with {c} pending: no finish in between")
    if "P4" in properties:
        bad += check_plan(tr)
    return bad


def check_plan(tr: Trace):
    """P4: split the trace at the ``optimizer`` markers; per step the released ranges are the plan's, in its order."""
    bad, released, last_micro_seen, steps = [], [], True, 0
    for i, e in enumerate(tr.events):
        if e[0] == "micro":
            last_micro_seen = e[1] == e[2] - 1
        elif e[0] == "reduce_range":
            if not last_micro_seen:
                bad.append(f"P4: #{i} reduce_range {e[1]}-{e[2]} is issued before the step's last micro-batch")
            released.append((e[1], e[2]))
        elif e[0] in ("reduce_tensor", "reduce_max") and not last_micro_seen and _is_grad_sum(tr, e):
            bad.append(f"P4: #{i} {e[0]} is issued before the step's last micro-batch")
        elif e[0] == "optimizer":
            steps += 1
            if released != tr.plan:
                bad.append(f"P4: step {steps} released {released}, the plan is {tr.plan}")
            pos = 0
            for lo, hi in released:
                if lo != pos or hi <= lo:
                    bad.append(f"P4: step {steps}: range {lo}-{hi} does not continue the tiling at {pos}")
                pos = hi
            if pos != tr.n:
                bad.append(f"P4: step {steps}: the released ranges end at {pos}, the arena at {tr.n}")
            released = []
    if released or not steps:
        bad.append(f"P4: {len(released)} ranges released behind the last of {steps} optimizer steps")
    return bad


def _is_grad_sum(tr, e):
    """The centre sums (step-level sums like the gradients) as opposed to Sinkhorn's per-forward reductions: they are ``reduce_tensor``
    calls outside a Sinkhorn pass, i.e. the previous launch is a loss, not a ``sinkhorn_*`` kernel."""
    i = next(k for k, x in enumerate(tr.events) if x is e)
    for k in range(i - 1, -1, -1):
        n = tr.events[k][0]
        if n not in MARKERS and n not in COLLECTIVES and n != "finish":
            return not n.startswith("sinkhorn_")
    return True


# --------------------------------------------------------------------------- #
# doctored traces: each must be flagged
# --------------------------------------------------------------------------- #
def _then_groups(events):
    """[(begin, end)] index pairs of the ``side.then`` groups that hold a reduce_range."""
    out, b = [], None
    for i, e in enumerate(events):
        if e[0] == "side.then.begin":
            b = i
        elif e[0] == "side.then.end":
            if any(x[0] == "reduce_range" for x in events[b:i]):
                out.append((b, i))
    return out


def releases_from_main(events):
    """1. The ``side.then`` markers around every reduce_range removed: the releases are issued from main."""
    drop = {i for pair in _then_groups(events) for i in pair}
    assert drop
    return [e for i, e in enumerate(events) if i not in drop]


def release_one_block_early(tr: Trace):
    """2. One block's reduce_range moved in front of the ``side.run`` that holds the last weight-gradient launch into its range."""
    ev = tr.events
    for b, e in _then_groups(ev)[1:]:          # (the first group is the head's)
        lo, hi = next((x[1], x[2]) for x in ev[b:e] if x[0] == "reduce_range")
        probe = Ev(-1, "", "", {}, [(tr.g, lo, hi)])
        depth, start = 0, None
        for i in range(b - 1, -1, -1):          # the last side.run before the release that writes into [lo, hi)
            if ev[i][0] == "side.run.end":
                end = i
                j = next(k for k in range(i, -1, -1) if ev[k][0] == "side.run.begin" and ev[k][1] == ev[i][1])
                hit = False
                for x in ev[j + 1:end]:
                    if x[0] not in MARKERS and len(x) == 3 and isinstance(x[2], dict):
                        r = []
                        tensor_ranges(x[1], r); tensor_ranges(x[2], r)
                        hit |= overlap(probe, Ev(-1, "", "", {}, r))
                if hit:
                    start = j
                    break
        if start is not None:
            return ev[:start] + ev[b:e + 1] + ev[start:b] + ev[e + 1:]
    raise AssertionError("no block release with a side.run into its range")


def drop_last_finish(events):
    """3. The step's last ``finish`` removed."""
    i = max(k for k, e in enumerate(events) if e[0] == "finish")
    return events[:i] + events[i + 1:]


def drop_joins_from_fill(tr: Trace):
    """4. The join of the arena fill (the ``side.run`` that holds ``Tensor.zero_`` of g) removed together with every later join."""
    ev = tr.events
    z = next(i for i, e in enumerate(ev) if e[0] == "Tensor.zero_" and e[1][0]["tensor"][0] == tr.g)
    k = next(ev[i][1] for i in range(z, -1, -1) if ev[i][0] == "side.run.begin")
    j = next(i for i, e in enumerate(ev) if e[0] == "side.join" and e[1] == k)
    return ev[:j] + [e for e in ev[j:] if e[0] != "side.join"]
