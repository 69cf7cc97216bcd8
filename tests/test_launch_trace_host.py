"""CPU: the launch sequence of every engine -- which ``ops`` call with which buffers, on which stream, behind which wait -- equals
the recording in tests/traces/engine_launches.json (tests/launch_trace.py records it without a GPU; regenerate the fixture there
when a change to the sequence is intended, and say so)."""
import pytest

import launch_trace as lt

FIX = lt.load_fixture()


def _first_difference(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f"event {k}: {a} (recorded: {b}); before it: {got[max(0, k - 4):k]}"
    return f"one sequence is a prefix of the other ({len(got)} against {len(want)} recorded events)"


def test_every_configuration_is_recorded():
    assert set(FIX) == set(lt.CONFIGS)
    assert all(("reduced" in FIX[c]) == (c in lt.REDUCED) for c in FIX)


@pytest.mark.parametrize("cid", list(lt.CONFIGS))
def test_engine_launch_trace(cid):
    events, arena_names = lt.trace(cid)
    got, want = lt.summary(events), FIX[cid]
    if cid in lt.REDUCED:
        # held to the parent commit's recording as a multiset of launches ...
        assert lt.reduced_summary(events, arena_names) == want["reduced"]
        # ... and in full either to the single loop's order or to the parent's own (its engine.py still passes)
        before = want.get("before_single_loop")
        if before is not None and (got["sha256"], got["count"]) == (before["sha256"], before["count"]):
            return
    assert got["names"] == want["names"], _first_difference(got["names"], want["names"])
    assert got["count"] == want["count"]
    assert got["sha256"] == want["sha256"], "same launch names, other arguments: diff the output of `python tests/launch_trace.py --dump DIR`"


def test_trace_is_the_same_twice():
    a, b = lt.trace("sup_t")[0], lt.trace("sup_t")[0]
    assert lt.summary(a) == lt.summary(b)
