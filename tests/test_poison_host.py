"""engine._empty / _carried / repoison on the host: the registry behind GIPVIT_POISON=1 (tests/test_poison_gpu.py runs the steps).
CPU tensors need none of the library's kernels."""
import gc

import pytest
import torch


@pytest.fixture
def pool():
    """The engine module with an empty registry (restored afterwards: other tests' engines may have registered buffers)."""
    from gipvit import engine
    saved = list(engine._POISON_POOL)
    engine._POISON_POOL[:] = []
    yield engine
    engine._POISON_POOL[:] = saved


def test_poison_registers_and_refills(pool, monkeypatch):
    monkeypatch.setenv("GIPVIT_POISON", "1")
    f = pool._empty((3, 5), torch.float32, "cpu")
    h = pool._empty((4,), torch.bfloat16, "cpu")
    u = pool._empty((2, 2, 3), torch.uint8, "cpu")
    assert bool(torch.isnan(f).all()) and bool(torch.isnan(h).all()) and bool((u == 255).all())
    assert len(pool._POISON_POOL) == 3
    f.zero_(); h.fill_(1.0); u.fill_(7)
    assert pool.repoison() == 3
    assert bool(torch.isnan(f).all()) and bool(torch.isnan(h).all()) and bool((u == 255).all())


def test_carried_is_poisoned_once(pool, monkeypatch):
    monkeypatch.setenv("GIPVIT_POISON", "1")
    c = pool._carried((6,), torch.float32, "cpu")
    cu = pool._carried((6,), torch.uint8, "cpu")
    e = pool._empty((6,), torch.float32, "cpu")
    assert bool(torch.isnan(c).all()) and bool((cu == 255).all())
    assert len(pool._POISON_POOL) == 1
    c.fill_(2.0); cu.fill_(3); e.fill_(2.0)
    assert pool.repoison() == 1
    assert bool((c == 2.0).all()) and bool((cu == 3).all()) and bool(torch.isnan(e).all())


def test_dead_tensor_leaves_the_pool(pool, monkeypatch):
    monkeypatch.setenv("GIPVIT_POISON", "1")
    a = pool._empty((2,), torch.float32, "cpu")
    b = pool._empty((2,), torch.float32, "cpu")
    assert pool.repoison() == 2
    del b
    gc.collect()
    assert pool.repoison() == 1 and len(pool._POISON_POOL) == 1
    assert pool._POISON_POOL[0]() is a


@pytest.mark.parametrize("dt", [torch.int32, torch.int64, torch.int16, torch.int8, torch.bool])
@pytest.mark.parametrize("on", [True, False])
def test_wide_integers_are_refused(pool, monkeypatch, dt, on):
    """Poison must never become a wild index: refused whether or not poison is on, by both allocators."""
    if on:
        monkeypatch.setenv("GIPVIT_POISON", "1")
    else:
        monkeypatch.delenv("GIPVIT_POISON", raising=False)
    for alloc in (pool._empty, pool._carried):
        with pytest.raises(TypeError):
            alloc((4,), dt, "cpu")
    assert pool._POISON_POOL == []


def test_poison_off_changes_nothing(pool, monkeypatch):
    monkeypatch.delenv("GIPVIT_POISON", raising=False)
    calls = []
    real = torch.empty

    def spy(*a, **kw):
        t = real(*a, **kw)
        calls.append(t)
        return t
    monkeypatch.setattr(torch, "empty", spy)
    e = pool._empty((3, 4), torch.float32, "cpu")
    c = pool._carried((5,), torch.uint8, "cpu")
    assert len(calls) == 2 and calls[0] is e and calls[1] is c          # plain torch.empty memory, handed through
    assert (e.shape, e.dtype, c.shape, c.dtype) == ((3, 4), torch.float32, (5,), torch.uint8)
    e.fill_(1.5); c.fill_(9)
    assert pool._POISON_POOL == [] and pool.repoison() == 0
    assert bool((e == 1.5).all()) and bool((c == 9).all())              # ... and repoison touches nothing
