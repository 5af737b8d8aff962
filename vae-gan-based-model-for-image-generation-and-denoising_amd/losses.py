"""Drop-in mirrors of the two loss modules the reference builds at vaegan_code.py:46-47
(``nn.BCELoss()``, ``nn.MSELoss(reduction='mean')``), running the fused HIP loss kernels.
Optional: the stock torch modules also work on the engine's outputs (they are ordinary tensors).
``SSIMLoss`` (not in the reference) is the structural term: 1 - the SSIM the denoising passes report."""
import torch
import torch.nn as nn

from . import ops


class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, target):
        if target.numel() != p.numel():
            raise ValueError(f"Using a target size ({tuple(target.shape)}) that is different to the input size "
                             f"({tuple(p.shape)}) is deprecated. Please ensure they have the same size.")
        t0 = float(target.flatten()[0])          # the reference only uses constant soft labels (0.9 / 0.1)
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        dp = ops.bce_forward_backward(p.contiguous(), t0, 1.0, loss, False, True)
        ctx.save_for_backward(dp)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return dp * g, None


class BCELoss(nn.Module):
    """nn.BCELoss() for a constant target vector (vaegan_code.py:88-89 uses torch.full labels)."""

    def forward(self, input, target):
        if not bool((target == target.flatten()[0]).all()):
            raise NotImplementedError("vaegan_amd.BCELoss supports the reference's constant soft labels only")
        return _BCEFn.apply(input, target)


class _MSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        loss = torch.empty(1, dtype=torch.float32, device=a.device)
        da = ops.mse_forward_backward(a.contiguous(), b.contiguous(), 1.0, loss, True)
        ctx.save_for_backward(da)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (da,) = ctx.saved_tensors
        ga = da * g if ctx.needs_input_grad[0] else None
        gb = -da * g if ctx.needs_input_grad[1] else None
        return ga, gb


class MSELoss(nn.Module):
    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("only reduction='mean' (vaegan_code.py:47)")

    def forward(self, input, target):
        return _MSEFn.apply(input, target)


msssim_weights = ops.msssim_weights


def _check_images(who, input, target, multi_scale=False, scales=None):
    """The argument checks of ``SSIMLoss`` and ``MSSSIMLoss`` (``who``), in the order they report: device, dtype, one
    [B,C,H,W] shape, the size (single scale: the 11 x 11 window; multi_scale: ``msssim_weights``, whose weights are
    returned), a constant target."""
    for name, t in (("input", input), ("target", target)):
        if not t.is_cuda:
            raise RuntimeError(f"vaegan_amd.{who} needs {name} on the MI355X ('cuda'); there is no CPU path")
        if t.dtype != torch.float32:
            raise TypeError(f"vaegan_amd.{who} supports float32 images only, got {name} of {t.dtype}")
    if input.dim() != 4 or input.shape != target.shape:
        raise ValueError(f"vaegan_amd.{who} needs input and target of one [B,C,H,W] shape, got {tuple(input.shape)} "
                         f"and {tuple(target.shape)}")
    weights = None
    if multi_scale:
        weights = msssim_weights(input.shape[2], input.shape[3], scales)      # ValueError: too small for the scales
    elif input.shape[2] < 11 or input.shape[3] < 11:
        raise ValueError(f"vaegan_amd.{who} needs images of at least 11 x 11 pixels (the 11 x 11 window), got "
                         f"{input.shape[2]} x {input.shape[3]}")
    if target.requires_grad:
        raise NotImplementedError(f"vaegan_amd.{who} treats the target as a constant; detach it")
    return weights


class _SSIMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        loss = torch.empty(1, dtype=torch.float32, device=a.device)
        da = torch.zeros_like(a, memory_format=torch.contiguous_format)
        ops.ssim_loss_forward_backward(a.contiguous(), b.contiguous(), 1.0, loss, False, da)
        ctx.save_for_backward(da)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (da,) = ctx.saved_tensors
        return da * g, None


class SSIMLoss(nn.Module):
    """1 - mean SSIM(input, target) of two [B,C,H,W] f32 image batches in [-1, 1] on the device: the metric of the
    denoising passes (gaussian 11 x 11, sigma 1.5, data range 1 after the rescale to [0, 1], 5-pixel border cropped) as a
    loss.  One HIP launch computes the value and the gradient w.r.t. ``input``; ``target`` is a constant (no gradient)."""

    def forward(self, input, target):
        _check_images("SSIMLoss", input, target)
        return _SSIMFn.apply(input, target)


def trainer_scales(ssim_scales, H, W):
    """The trainers' ``ssim_scales`` argument (not None) -> the weight tuple for H x W images: True or "auto" = the
    default scales of the image size (``msssim_weights(H, W)``), an int or a sequence of weights as ``msssim_weights``
    takes them."""
    if ssim_scales is True or (isinstance(ssim_scales, str) and ssim_scales == "auto"):
        return msssim_weights(H, W)
    if ssim_scales is None or ssim_scales is False or isinstance(ssim_scales, str):
        raise ValueError(f"ssim_scales must be None, True / 'auto', an int or a sequence of weights, got {ssim_scales!r}")
    return msssim_weights(H, W, ssim_scales)


class _MSSSIMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, weights):
        loss = torch.empty(1, dtype=torch.float32, device=a.device)
        da = torch.zeros_like(a, memory_format=torch.contiguous_format)
        ops.msssim_loss_forward_backward(a.contiguous(), b.contiguous(), weights, 1.0, loss, False, da)
        ctx.save_for_backward(da)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (da,) = ctx.saved_tensors
        return da * g, None, None


class MSSSIMLoss(nn.Module):
    """1 - MS-SSIM(input, target) (Wang, Simoncelli & Bovik 2003) of two [B,C,H,W] f32 image batches in [-1, 1] on the
    device: the SSIM maps of ``SSIMLoss`` over a 2x average-pooling pyramid, the contrast-structure mean of every level
    but the last and the SSIM mean of the last, each raised to its scale's weight, multiplied per image and averaged over
    the batch; an image with a non-positive mean at any level counts 0 and gets no gradient.  ``scales``: None = as many
    of the five published scales as the image holds (3 at 64, 4 at 128, 5 at 256; weights renormalised), an int, or 1 - 5
    weights (``msssim_weights``).  At most five HIP launches whatever the number of scales; ``target`` is a constant.
    Parity with the torchmetrics / pytorch-msssim packages is unpinned (neither is installed where this is tested): the
    tests restate the formulas in f64."""

    def __init__(self, scales=None):
        super().__init__()
        msssim_weights(1 << 14, 1 << 14, scales)          # a bad count / weight fails here
        self.scales = scales

    def forward(self, input, target):
        weights = _check_images("MSSSIMLoss", input, target, multi_scale=True, scales=self.scales)
        return _MSSSIMFn.apply(input, target, weights)
