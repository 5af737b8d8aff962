"""Differentiable augmentation of the Discriminator's inputs (Zhao et al., NeurIPS 2020, "DiffAugment"; not in the reference;
DESIGN.md section 4.4j): per image a random colour change (brightness, saturation, contrast), translation and cutout, applied
on the device to everything the Discriminator sees -- real and generated alike -- with the Generator's gradient carried back
through the exact adjoint (csrc/diffaug.hip; contract in include/vaegan_hip.h, "Differentiable augmentation").

    trainer = VAEGANTrainer(..., augment="color,translation,cutout")        # or augment=DiffAugment("color")

One parameter table is drawn per iteration from the trainer's noise stream; the real image and its reconstruction share a
row, so a feature loss between the two is not measuring the shift.
"""
import torch

from . import ops

_BITS = {"brightness": ops.AUG_BRIGHTNESS, "saturation": ops.AUG_SATURATION, "contrast": ops.AUG_CONTRAST,
         "color": ops.AUG_BRIGHTNESS | ops.AUG_SATURATION | ops.AUG_CONTRAST,
         "translation": ops.AUG_TRANSLATION, "cutout": ops.AUG_CUTOUT}


def parse_policy(policy: str) -> int:
    """'color,translation,cutout' -> the AUG_* bit sum; '' is the identity (every launch still runs).  Unknown names raise
    ValueError."""
    if not isinstance(policy, str):
        raise ValueError("augmentation policy must be a string of comma-separated names")
    bits = 0
    for name in policy.split(","):
        name = name.strip()
        if not name:
            continue
        if name not in _BITS:
            raise ValueError(f"unknown augmentation {name!r}: choose among {sorted(_BITS)}")
        bits |= _BITS[name]
    return bits


class DiffAugment:
    """A policy and the launches that go with it.  `bits` is what a captured graph freezes (key())."""

    def __init__(self, policy: str = "color,translation,cutout"):
        self.bits = parse_policy(policy)
        self.policy = policy

    @staticmethod
    def of(augment):
        """None, a DiffAugment or a policy string -> None or a DiffAugment."""
        if augment is None or isinstance(augment, DiffAugment):
            return augment
        return DiffAugment(augment)

    def key(self):
        return ("augment", self.bits)

    @property
    def need_sum(self) -> bool:
        """Whether the whole-image sums are needed: only contrast uses them (their coefficient 1 - k is 0 otherwise)."""
        return bool(self.bits & ops.AUG_CONTRAST)

    def draw(self, state: torch.Tensor, B: int, H: int, W: int, out=None) -> torch.Tensor:
        """One table [B, 8] from the noise state {seed, iteration} (one launch)."""
        return ops.diffaug_params(state, B, self.bits, H, W, out)

    def forward(self, x, params, C, dtype, out=None):
        """x [N,H,W,CP] in the engine layout -> the augmented batch (image n by row n % PB)."""
        return ops.diffaug_forward(x, params, C, ops.diffaug_cut(self.bits, x.shape[1], x.shape[2]), dtype, out, self.need_sum)

    def backward(self, g, params, C, dtype, out=None):
        """The gradient w.r.t. the augmented batch -> the gradient w.r.t. the batch."""
        return ops.diffaug_backward(g, params, C, ops.diffaug_cut(self.bits, g.shape[1], g.shape[2]), dtype, out, self.need_sum)


def check_dtype(dt: int) -> None:
    if dt not in (ops.F32, ops.BF16):
        raise ValueError("augment= needs a Discriminator whose input dtype is f32 or bf16")
