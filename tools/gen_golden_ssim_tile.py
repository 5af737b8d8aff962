"""Writes tests/golden/ssim_tile_parent.npz: the raw output bits of the single-scale and the multi-scale SSIM losses
(csrc/ssimloss.hip, csrc/msssim.hip) on seeded inputs, from the build of commit 9969252 -- the last one in which the two
files each held their own statement of the tile pass.  tests/test_gpu_ssim_tile_parent.py regenerates the inputs
(tests/_pointwise_ref.ssim_inputs) and asserts bit equality, so the fixture pins the arithmetic of the tile pass now shared
in csrc/ssim_tile.hpp: a reordered sum or a contracted product shows as a moved bit.

The fixture holds results only, as uint32 words; an array of more than LIMIT elements is stored as the SHA-256 of its bytes.

Run it ONCE on a checkout whose results are to be preserved (it uses only ops.ssim_loss_forward_backward and
ops.msssim_loss_forward_backward), on the GPU:

    python tools/gen_golden_ssim_tile.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
OUT = os.path.join(ROOT, "tests", "golden", "ssim_tile_parent.npz")
DEV = "cuda"
LIMIT = 16384
GSCALE = 0.37                               # the accumulating variants: d pre-filled, loss slot holding 3.0

SINGLE_KINDS = ("noise", "blocks", "same")
SINGLE_SHAPES = [(1, 1, 11, 11),            # one interior pixel, the halo is larger than the plane
                 (2, 3, 12, 17),            # small ragged plane
                 (1, 3, 70, 45),            # 3 x 2 tiles, ragged both ways
                 (1, 1, 11, 300)]           # one interior row, ten tiles
SINGLE_ACCUMULATING = SINGLE_SHAPES[:2]

MULTI_KINDS = ("noise", "small_noise", "blocks")
MULTI_SHAPES = [((1, 1, 22, 22), 2),        # the coarse level is one interior pixel
                ((2, 3, 23, 37), 2),        # a dropped row and a dropped column
                ((1, 3, 70, 45), 3),        # ragged tiles, last level 17 x 11
                ((2, 3, 64, 64), 3),        # with `noise`, one image on the clamp and one not (_msssim_ref.CLAMPED)
                ((1, 1, 176, 176), 5)]      # all five levels of the Plan table
EXPLICIT = ((2, 3, 23, 37), (0.3, 1.2))     # this shape also runs with explicit unnormalised weights ...
PREFILLED = ((2, 3, 23, 37), "small_noise")  # ... and, for this kind, into a pre-filled d


def _ref():
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _pointwise_ref as P
    return P


def pack(t) -> np.ndarray:
    """f32 tensor -> its uint32 words, or the SHA-256 of their bytes (uint8 [32]) above LIMIT elements."""
    bits = np.ascontiguousarray(t.detach().cpu().contiguous().numpy()).view(np.uint32)
    if bits.size > LIMIT:
        return np.frombuffer(hashlib.sha256(bits.tobytes()).digest(), dtype=np.uint8)
    return bits


def prefill(P, shape):
    import torch
    return (torch.randn(shape, generator=P.gen(sum(shape))) * 1e-3).float().to(DEV)


def single_id(shape, kind):
    return "ssim/" + "x".join(map(str, shape)) + "/" + kind


def multi_id(shape, M, kind):
    return "msssim/" + "x".join(map(str, shape)) + f"_M{M}/" + kind


def run_single(ops, shape, kind):
    """-> {variant/name: packed array} of one single-scale case."""
    import torch
    P = _ref()
    a, b = (t.to(DEV) for t in P.ssim_inputs(kind, *shape))
    out = {}
    loss, d = torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV)
    ops.ssim_loss_forward_backward(a, b, 1.0, loss, False, d)
    out["zeroed/loss"], out["zeroed/d"] = pack(loss), pack(d)
    if shape in SINGLE_ACCUMULATING:
        loss, d = torch.full((1,), 3.0, device=DEV), prefill(P, shape)
        ops.ssim_loss_forward_backward(a, b, GSCALE, loss, True, d)
        out["prefilled/loss"], out["prefilled/d"] = pack(loss), pack(d)
    loss = torch.zeros(1, device=DEV)
    ops.ssim_loss_forward_backward(a, b, 1.0, loss, False, None)
    out["forward/loss"] = pack(loss)
    torch.cuda.synchronize()
    return out


def run_multi(ops, shape, M, kind):
    """-> {variant/name: packed array} of one multi-scale case."""
    import torch
    P = _ref()
    a, b = (t.to(DEV) for t in P.ssim_inputs(kind, *shape))
    out = {}
    sets = [("default", ops.msssim_weights(shape[2], shape[3], M))]
    if shape == EXPLICIT[0]:
        sets.append(("explicit", EXPLICIT[1]))
    for tag, w in sets:
        assert len(w) == M
        loss, d, per = torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV), torch.zeros(shape[0], M, device=DEV)
        ops.msssim_loss_forward_backward(a, b, w, 1.0, loss, False, d, per)
        out[f"{tag}/loss"], out[f"{tag}/per_scale"], out[f"{tag}/d"] = pack(loss), pack(per), pack(d)
        loss = torch.zeros(1, device=DEV)
        ops.msssim_loss_forward_backward(a, b, w, 1.0, loss, False, None)
        out[f"{tag}/forward_loss"] = pack(loss)
    if (shape, kind) == PREFILLED:
        loss, d = torch.full((1,), 3.0, device=DEV), prefill(P, shape)
        ops.msssim_loss_forward_backward(a, b, sets[0][1], GSCALE, loss, True, d)
        out["prefilled/loss"], out["prefilled/d"] = pack(loss), pack(d)
    torch.cuda.synchronize()
    return out


def main() -> None:
    sys.path[:0] = [ROOT]
    from importlib import import_module
    ops = import_module(PKG + ".ops")
    arrays = {}
    for shape in SINGLE_SHAPES:
        for kind in SINGLE_KINDS:
            for k, v in run_single(ops, shape, kind).items():
                arrays[f"{single_id(shape, kind)}/{k}"] = v
    for shape, M in MULTI_SHAPES:
        for kind in MULTI_KINDS:
            for k, v in run_multi(ops, shape, M, kind).items():
                arrays[f"{multi_id(shape, M, kind)}/{k}"] = v
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
