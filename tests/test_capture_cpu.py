"""CPU: capture.HostMirrors, the host-side counters a hipGraph capture measures, undoes and replays -- on plain stand-ins
that carry only the counter attributes (no device, no library call)."""
from types import SimpleNamespace as NS

import pytest

import vaegan_amd as V  # noqa: F401  (registers the package's submodules under the alias)
from vaegan_amd.capture import HostMirrors


def _world(reducer_attrs=("collectives", "bytes_reduced", "stat_collectives")):
    engines = [NS(pending_bn_ticks=3), NS(pending_bn_ticks=0)]
    opts = [NS(steps=7), NS(steps=11), NS(steps=0)]
    red = NS(**{n: 100 * (i + 1) for i, n in enumerate(reducer_attrs)})
    return engines, opts, red


def _iteration(engines, opts, red):
    """What one captured iteration does to the counters."""
    engines[0].pending_bn_ticks += 1
    engines[1].pending_bn_ticks += 5
    opts[0].steps += 1
    opts[2].steps += 2
    for n, d in (("collectives", 9), ("bytes_reduced", 4096), ("stat_collectives", 30)):
        if hasattr(red, n):
            setattr(red, n, getattr(red, n) + d)


def _state(engines, opts, red):
    return [e.pending_bn_ticks for e in engines], [o.steps for o in opts], dict(vars(red))


@pytest.mark.parametrize("replay_reducer", [False, True])
def test_host_mirrors_snapshot_deltas_restore_apply(replay_reducer):
    engines, opts, red = _world()
    m = HostMirrors(engines, opts, red, replay_reducer=replay_reducer)
    before = _state(engines, opts, red)
    snap = m.snapshot()
    _iteration(engines, opts, red)
    after = _state(engines, opts, red)
    deltas = m.deltas(snap)
    assert deltas[:5] == [1, 5, 1, 0, 2]                               # engines, then optimizers: the mutation
    assert deltas[5:] == ([9, 4096, 30] if replay_reducer else [])    # a segmented reducer counts for itself
    m.restore(snap)
    assert _state(engines, opts, red) == before                        # every attribute back, the reducer's too
    m.apply(deltas)
    want = after if replay_reducer else (after[0], after[1], before[2])
    assert _state(engines, opts, red) == want
    m.apply(deltas)                                                    # per replay: twice is two iterations
    assert [e.pending_bn_ticks for e in engines] == [5, 10] and [o.steps for o in opts] == [9, 11, 4]
    assert red.collectives == 100 + (18 if replay_reducer else 0)


def test_host_mirrors_without_a_reducer():
    engines, opts, _ = _world()
    m = HostMirrors(engines, opts)
    snap = m.snapshot()
    _iteration(engines, opts, NS())
    assert m.deltas(snap) == [1, 5, 1, 0, 2]
    m.restore(snap)
    assert [e.pending_bn_ticks for e in engines] == [3, 0] and [o.steps for o in opts] == [7, 11, 0]


@pytest.mark.parametrize("missing", ["collectives", "bytes_reduced", "stat_collectives"])
def test_host_mirrors_tolerate_a_reducer_that_lacks_a_counter(missing):
    have = tuple(n for n in ("collectives", "bytes_reduced", "stat_collectives") if n != missing)
    engines, opts, red = _world(have)
    m = HostMirrors(engines, opts, red, replay_reducer=True)
    before = _state(engines, opts, red)
    snap = m.snapshot()
    _iteration(engines, opts, red)
    after = _state(engines, opts, red)
    deltas = m.deltas(snap)
    assert len(deltas) == 5 + 2
    m.restore(snap)
    assert _state(engines, opts, red) == before and not hasattr(red, missing)
    m.apply(deltas)
    assert _state(engines, opts, red) == after and not hasattr(red, missing)
