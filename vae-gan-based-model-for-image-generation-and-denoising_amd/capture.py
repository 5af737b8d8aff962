"""Whole-iteration hipGraph capture and replay, ONE implementation for every graphed step path (trainer.VAEGANTrainer,
the sibling trainers, graphed.GraphedStep).  The callers keep their policy -- what goes into the key, how many eager
warm-up calls, how many graphs they hold, which memory pool and capture mode -- and hand the dangerous part to
``capture`` / ``replay``.
"""
import gc
from typing import Any, Callable, List, NamedTuple, Optional, Sequence

import torch

REDUCER_COUNTERS = ("collectives", "bytes_reduced", "stat_collectives")


class no_gc_while_capturing:
    """Context for a hipGraph capture: collect garbage first and keep Python's cyclic collector off until the capture has
    ended.  A collection in the middle of a capture can destroy an older trainer's CUDAGraph or tensors of its private
    pool; releasing device memory is not permitted while the thread captures, and the error surfaces inside a destructor,
    i.e. as an abort of the process (seen once in four full test runs, under "Garbage-collecting" in the fault dump).
    torch.cuda.graph() takes the same precaution (gc.collect() before capture_begin)."""

    def __enter__(self):
        gc.collect()
        self._was = gc.isenabled()
        gc.disable()
        return self

    def __exit__(self, *exc):
        if self._was:
            gc.enable()
        return False


class HostMirrors:
    """The host-side counters an iteration moves next to its device work: every engine's BatchNorm forward count
    (``pending_bn_ticks``), every optimizer's ``steps`` (the authoritative Adam step counter lives on the device) and,
    of a gradient reducer, those of its statistics counters it has.  A capture executes nothing, so what it did to them is
    measured (``deltas``), undone (``restore``) and then applied once per replay (``apply``).
    replay_reducer: the reducer's counters advance per replay too -- for collectives recorded INSIDE the graph, whose
    replay runs no Python of the reducer.  Collectives that run between graph segments count for themselves."""

    def __init__(self, engines: Sequence, optimizers: Sequence, reducer=None, replay_reducer: bool = False):
        self.engines = tuple(engines)
        self._slots = [(e, "pending_bn_ticks") for e in self.engines] + [(o, "steps") for o in optimizers]
        self._replayed = len(self._slots)
        if reducer is not None:
            self._slots += [(reducer, n) for n in REDUCER_COUNTERS if hasattr(reducer, n)]
        if replay_reducer:
            self._replayed = len(self._slots)

    def snapshot(self) -> List:
        return [getattr(o, n) for o, n in self._slots]

    def restore(self, snap: List) -> None:
        for (o, n), v in zip(self._slots, snap):
            setattr(o, n, v)

    def deltas(self, snap: List) -> List:
        return [getattr(o, n) - v for (o, n), v in zip(self._slots[:self._replayed], snap)]

    def apply(self, deltas: List) -> None:
        for (o, n), d in zip(self._slots, deltas):
            setattr(o, n, getattr(o, n) + d)


class CaptureRefused(RuntimeError):
    """Raised by a caller's pre_capture hook: no capture was begun (nothing to clean up, the call may be repeated)."""


class Captured(NamedTuple):
    key: Any                # what the caller looks the capture up by
    graphs: List            # the hipGraph segments, in replay order
    cuts: List[Callable]    # cuts[i] runs eagerly between graphs[i] and graphs[i + 1]
    sin: List               # static inputs the captured launches read
    out: Any                # static output of the step (the next replay overwrites it)
    deltas: List            # what one iteration adds to the host mirrors
    mirrors: HostMirrors
    keep: Any = None        # whatever else must live as long as the graphs


def capture(step: Callable, sin: Sequence, mirrors: HostMirrors, device, key=None, pool=None,
            error_mode: str = "thread_local", pre_capture: Optional[Callable] = None,
            install_cut: Optional[Callable] = None, keep=None) -> Captured:
    """Capture ``step(*sin)`` into hipGraphs.  Executes nothing: the host mirrors are put back and the caller replays.
    pool: memory pool handle shared by the segments (None: a private one per graph).
    error_mode: "thread_local" where other threads may legitimately touch the runtime meanwhile -- torch.distributed's
    watchdog thread polls finished collectives with hipEventQuery at its own pace, and under the global mode such a call
    from ANOTHER thread while this one captures is an error that takes the process down (seen once in four runs with
    RCCL).  "global" (torch's default) where other threads launch INTO the capture: the autograd engine runs the backward
    nodes of a reference-shaped step on its own device thread, and their work must be captured with the rest.
    pre_capture: runs after the engines' packed operands were invalidated and before the device is synchronised; it may
    raise CaptureRefused.
    install_cut: called with ``cut`` before the step and with None after it; ``cut(fn)`` inside the step closes the
    current segment, remembers fn to run between the segment replays and opens the next segment.
    If anything raises once the capture has begun, the open capture is ended, the mirrors are restored, the engines are
    invalidated and the exception propagates: the caller is where it was and can run eagerly or capture again."""
    for e in mirrors.engines:
        e.invalidate()                              # the captured sequence must contain the operand re-packs
    if pre_capture is not None:
        pre_capture()
    torch.cuda.synchronize()
    snap = mirrors.snapshot()
    graphs, cuts = [], []
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())

    def begin():
        g = torch.cuda.CUDAGraph()
        g.capture_begin(pool=pool, capture_error_mode=error_mode)
        graphs.append(g)

    def cut(between):
        graphs[-1].capture_end()
        cuts.append(between)
        begin()

    with no_gc_while_capturing(), torch.cuda.stream(side):
        if install_cut is not None:
            install_cut(cut)
        try:
            begin()
            out = step(*sin)
            graphs[-1].capture_end()
        except BaseException:
            try:                                    # leave no stream behind in capture mode
                graphs[-1].capture_end()
            except Exception:
                pass
            mirrors.restore(snap)
            for e in mirrors.engines:
                e.invalidate()
            raise
        finally:
            if install_cut is not None:
                install_cut(None)
    torch.cuda.current_stream().wait_stream(side)
    deltas = mirrors.deltas(snap)
    mirrors.restore(snap)                           # capture only records: the caller replays for real
    return Captured(key, graphs, cuts, sin, out, deltas, mirrors, keep)


def replay(cap: Captured) -> None:
    """One iteration: every segment, the cut that follows it, then the host mirrors."""
    cuts = cap.cuts
    for i, g in enumerate(cap.graphs):
        g.replay()
        if i < len(cuts):
            cuts[i]()
    cap.mirrors.apply(cap.deltas)
