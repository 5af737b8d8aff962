"""Exponential moving average of network weights on the device (not in the reference).

A GAN-trained decoder's weights jitter from step to step with the adversarial game; what is evaluated and saved is
usually a slowly moving average of them.  The parameters here live in ``optim.Adam``'s flat buffers and are rewritten by a
raw-pointer kernel inside a replayed hipGraph, so the average is kept the same way: one shadow buffer per optimizer, updated
by ONE launch for all of them (``ops.ema_update``, csrc/ema.hip) that reads the optimizers' device-resident step counters
and can be captured with the iteration.

    ema = EMA([encoder, decoder], [opt_E, opt_Dec], decay=0.999)
    trainer = VAEGANTrainer(encoder, decoder, discriminator, opt_E, opt_Dec, opt_Dis, ema=ema)
    ...training steps (eager or graphed)...
    images = ema.module(decoder)(z)                      # the averaged Generator, eval mode
    torch.save(ema.module(decoder).state_dict(), "decoder.pth")

Construct an EMA AFTER ``.to(device)``, after the optimizers (they re-home the parameters into their flat buffers) and, in
data-parallel runs, after ``ddp``'s initial broadcast: the shadow starts as a copy of the weights it finds.  Every rank then
holds identical parameters after each all-reduced step and hence identical shadows; no collective is needed.

With ``warmup`` the decay of step t (the optimizer's step count, t = 1 for the first update) is
``min(decay, (1 + t) / (10 + t))``: a young average follows the weights quickly instead of remembering their initial values
for ~1 / (1 - decay) steps.

A shadow network is a view of state that training keeps moving: re-fetch it through ``module()`` after training steps
(``module()`` drops the shadow's packed GEMM operands, so what it returns always computes with the current average), do
not hold on to it across them.
"""
import math
from typing import Dict, List

import torch

from . import ops
from ._lib import VG_EMA_MAX
from .engine import bump_weights_epoch
from .optim import Adam


def _engines(module) -> List:
    return [m._engine for m in module.modules() if getattr(m, "_engine", None) is not None]


class EMA:
    """EMA(modules, optimizers, decay=0.999, warmup=True).

    modules: the networks to average (``Encoder`` / ``Generator`` / ``Discriminator`` / ``ConvBlock``), one or a sequence;
    optimizers: the ``vaegan_amd.Adam`` instances that hold their parameters (at most 4; one optimizer may hold several
    networks, as VAETrainer's does).  Every parameter of every module must be homed in one of the optimizers' flat buffers
    and every optimizer must hold at least one of them, else ValueError.

    Per optimizer there is one shadow buffer (``flat_p.clone()``; the padding slots stay 0), per module one shadow instance
    of the same class (same constructor arguments and dtype) in eval mode with ``requires_grad`` off.  A shadow's parameters
    are views into the shadow buffer at the live parameters' offsets; its BatchNorm buffers ARE the live module's tensors
    (running statistics are copied, not averaged, as is usual: aliasing copies them for free and keeps them current)."""

    def __init__(self, modules, optimizers, decay: float = 0.999, warmup: bool = True):
        modules = [modules] if isinstance(modules, torch.nn.Module) else list(modules)
        optimizers = [optimizers] if isinstance(optimizers, Adam) else list(optimizers)
        self.decay = self._check_decay(decay)
        self.warmup = bool(warmup)
        if not modules:
            raise ValueError("EMA needs at least one module")
        if not 1 <= len(optimizers) <= VG_EMA_MAX:
            raise ValueError(f"EMA takes 1..{VG_EMA_MAX} optimizers, got {len(optimizers)}")
        for o in optimizers:
            if not isinstance(o, Adam):
                raise ValueError("EMA needs vaegan_amd.Adam optimizers (their flat parameter buffers are what is averaged)")
        home = {}                                   # id(parameter) -> (optimizer index, offset)
        for k, o in enumerate(optimizers):
            for p, off in zip(o.params, o.offsets):
                home[id(p)] = (k, off)
        used = set()
        for m in modules:
            if not hasattr(m, "_vg_ctor"):
                raise ValueError(f"EMA cannot copy a {type(m).__name__}: only the networks of vaegan_amd.nets record their "
                                 "constructor arguments")
            for name, p in m.named_parameters():
                k, off = home.get(id(p), (None, None))
                if k is None or p.data_ptr() != optimizers[k].flat_p.data_ptr() + 4 * off:
                    raise ValueError(f"parameter {name} of {type(m).__name__} is not homed in any of the given optimizers' "
                                     "flat buffers (construct the EMA after .to(device) and after the optimizers)")
                used.add(k)
        if len(used) != len(optimizers):
            raise ValueError("an optimizer holds no parameter of the given modules")
        self.modules, self.optimizers = modules, optimizers
        self.shadow_bufs = [o.flat_p.clone() for o in optimizers]
        self.shadows = [self._make_shadow(m, home) for m in modules]
        self._by_id = {id(m): s for m, s in zip(modules, self.shadows)}
        self._params = [p for s in self.shadows for p in s.parameters()]
        bump_weights_epoch(self._params)

    @staticmethod
    def _check_decay(decay) -> float:
        decay = float(decay)
        if not (math.isfinite(decay) and 0.0 <= decay <= 1.0):
            raise ValueError(f"decay must be finite and in [0, 1], got {decay}")
        return decay

    def _make_shadow(self, live, home):
        dev = next(live.parameters()).device
        with torch.random.fork_rng(devices=[]):     # the constructor draws initial weights: leave the caller's generator alone
            sh = type(live)(**live._vg_ctor)
        sh.to(dev)
        sh.eval()
        with torch.no_grad():
            for (_, pl), (_, ps) in zip(live.named_parameters(), sh.named_parameters()):
                k, off = home[id(pl)]
                ps.data = self.shadow_bufs[k][off:off + pl.numel()].view(pl.shape)
                ps.requires_grad_(False)
        for ml, ms in zip(live.modules(), sh.modules()):
            for name in ml._buffers:
                ms._buffers[name] = ml._buffers[name]
        # fused pairs (the Encoder's fc_mu | fc_logvar) sit back to back in the shadow buffer as they do in the live one:
        # the shadow's engine finds them contiguous; its operand tables are built on first use
        for e in _engines(sh):
            e.invalidate()
        return sh

    # ---- the update -------------------------------------------------------------------------------------------------
    def update(self) -> None:
        """One launch for all shadow buffers, after the optimizers' step of this iteration (their device step counters are
        already incremented).  Capturable; the shadows' packed operands become stale (weight epochs bumped)."""
        ops.ema_update(self.shadow_bufs, [o.flat_p for o in self.optimizers], [o.state_dev for o in self.optimizers],
                       [self.decay] * len(self.optimizers), [self.warmup] * len(self.optimizers))
        self.touch()

    def touch(self) -> None:
        """The shadow buffers were rewritten behind torch's back (update(), a graph replay that contains one)."""
        bump_weights_epoch(self._params)

    def reset(self) -> None:
        """Shadow := the live weights as they are now."""
        with torch.no_grad():
            for b, o in zip(self.shadow_bufs, self.optimizers):
                b.copy_(o.flat_p)
        self.touch()

    def key(self):
        """What a captured update freezes (part of the trainers' capture keys)."""
        return (self.decay, self.warmup, tuple(b.data_ptr() for b in self.shadow_bufs))

    def module(self, live):
        """The shadow of `live` (one of the modules given at construction): same class, eval mode, averaged parameters, the
        live BatchNorm buffers.  Its packed operands are dropped first, so a shadow fetched after any number of graph
        replays computes with the current average.  Re-fetch after training steps."""
        try:
            sh = self._by_id[id(live)]
        except KeyError:
            raise ValueError("module() takes one of the modules this EMA was built over") from None
        for e in _engines(live):
            e.flush_bn_ticks()                      # num_batches_tracked, shared with the shadow, is current as well
        for e in _engines(sh):
            e.invalidate()
        return sh

    # ---- checkpoint -------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict:
        """Format 1: decay, warmup and each shadow's module state_dict (the reference's keys: ema.module(decoder)
        .state_dict() is a drop-in decoder.pth), taken after the live engines' pending BatchNorm ticks are flushed."""
        for m in self.modules:
            for e in _engines(m):
                e.flush_bn_ticks()
        return {"format": 1, "decay": self.decay, "warmup": self.warmup,
                "shadows": [{k: v.clone() for k, v in s.state_dict().items()} for s in self.shadows]}

    def load_state_dict(self, sd: Dict) -> None:
        """Restores decay, warmup and the averaged PARAMETERS; the BatchNorm buffers are the live modules' and stay theirs
        (load the live networks' state for those)."""
        if sd.get("format") != 1:
            raise RuntimeError(f"unknown EMA checkpoint format {sd.get('format')!r}")
        shadows = sd["shadows"]
        if len(shadows) != len(self.shadows):
            raise RuntimeError(f"EMA checkpoint holds {len(shadows)} networks, this EMA {len(self.shadows)}")
        for s, st in zip(self.shadows, shadows):
            missing = [k for k, _ in s.named_parameters() if k not in st]
            if missing:
                raise RuntimeError(f"EMA checkpoint lacks {missing} of {type(s).__name__}")
        self.decay, self.warmup = self._check_decay(sd["decay"]), bool(sd["warmup"])
        with torch.no_grad():
            for s, st in zip(self.shadows, shadows):
                for k, p in s.named_parameters():
                    p.data.copy_(st[k])
        self.touch()
        for s in self.shadows:
            for e in _engines(s):
                e.invalidate()
