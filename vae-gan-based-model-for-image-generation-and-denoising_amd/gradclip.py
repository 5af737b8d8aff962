"""The trainers' ``max_grad_norm`` option: which networks' gradients are clipped to which global L2
norm, the device tensor the norms and coefficients of the last iteration are kept in, and the one call the trainers place
directly before an optimizer step.  The arithmetic is optim.clip_grad_norm_'s (vg_grad_norm_clip + vg_adam_apply_clip): per-
network norms only -- a joint norm over several optimizers is not offered.
"""
from typing import Dict, Optional

import torch

from .optim import Adam, check_max_norm, clip_grad_norm_


class GradClip:
    """max_grad_norm as the trainers accept it, bound to their optimizers.

    max_grad_norm: a number (every network is clipped to its own norm at that value; inf: monitor only) or a dict whose
    keys are among the trainer's network names (only the named networks are clipped).  NaN, a negative value, another type
    or an unknown name: ValueError.
    grad_norms: f32 device tensor [len(names), 2], row i = [norm, coefficient] of network names[i] as its LAST clip call left
    them (rows of networks that are not configured stay 0).  Each configured optimizer's clip_dev is a view of its row, so
    the reduction writes there and the Adam step reads the coefficient from there: nothing is copied."""

    def __init__(self, max_grad_norm, opts: Dict[str, Adam], grad_norms: Optional[torch.Tensor] = None):
        self.names = tuple(opts)
        if isinstance(max_grad_norm, dict):
            for k in max_grad_norm:
                if k not in opts:
                    raise ValueError(f"max_grad_norm: unknown network {k!r} (this trainer has {', '.join(self.names)})")
            self.max = {k: check_max_norm(max_grad_norm[k]) for k in self.names if k in max_grad_norm}
        else:
            m = check_max_norm(max_grad_norm)
            self.max = {k: m for k in self.names}
        self.opts = dict(opts)
        dev = next(iter(opts.values())).flat_g.device
        self.grad_norms = grad_norms if grad_norms is not None else \
            torch.zeros(len(self.names), 2, dtype=torch.float32, device=dev)
        for i, k in enumerate(self.names):
            if k in self.max:
                self.opts[k].clip_dev = self.grad_norms[i]

    def key(self):
        """What a captured iteration freezes of this option."""
        return tuple((k, self.max[k]) for k in self.names if k in self.max) + (self.grad_norms.data_ptr(),)

    def clip(self, *names) -> None:
        """ONE clip_grad_norm_ call (two launches) over those of `names` that are configured; none: nothing is launched.
        Arms their optimizers: place it directly before their step()."""
        sel = [k for k in names if k in self.max]
        if sel:
            clip_grad_norm_([self.opts[k] for k in sel], [self.max[k] for k in sel])

    def report(self) -> Dict[str, float]:
        """Host copy (one sync): grad_norm_<name> / clip_coef_<name> of every configured network."""
        v = self.grad_norms.tolist()
        out = {}
        for i, k in enumerate(self.names):
            if k in self.max:
                out[f"grad_norm_{k}"] = v[i][0]
                out[f"clip_coef_{k}"] = v[i][1]
        return out


class ClipOption:
    """Mixin of the trainers: the ``max_grad_norm`` attribute (assignable; a captured graph is keyed on it) and
    ``grad_norms``.  The trainer provides _clip_opts() -> {network name: optimizer}."""
    _clip: Optional[GradClip] = None
    _max_grad_norm = None

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value) -> None:
        if value is None:
            self._clip = None
        else:
            self._clip = GradClip(value, self._clip_opts(), None if self._clip is None else self._clip.grad_norms)
        self._max_grad_norm = value

    @property
    def grad_norms(self) -> Optional[torch.Tensor]:
        """[networks, 2] device tensor: [norm, coefficient] per network of the last iteration (GradClip), None when
        max_grad_norm is None."""
        return None if self._clip is None else self._clip.grad_norms

    def _clip_key(self):
        return () if self._clip is None else (("clip",) + self._clip.key(),)
