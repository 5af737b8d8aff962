"""Writes tests/golden/eval_passes_parent.json: what the five evaluation passes of denoise.py -- denoise_eval,
validation_epoch, paired_test_epoch, tiled_denoise_eval, tiled_test_epoch -- returned on seeded networks and inputs at commit
c894c74, the last one in which every pass spelled out its own reconstruction step, noise draw and accumulator layout.
tests/test_gpu_eval_passes_parent.py reruns the cases defined here and asserts equality, so the fixture pins every result
bit, the key order, the launches and the host reads of the passes now built from denoise.py's shared pieces.

Per case the fixture holds results only:

    keys         the result's keys in insertion order
    values       float -> float.hex() ("inf" for an infinity), int -> int, tensor -> its shape and the SHA-256 of its bytes
    launches     the ops.launch_count() delta over the call
    host_reads   Tensor.tolist + Tensor.item calls during the call
    noise        the default noise stream's [seed, iteration counter] after the call

Every case is called twice from the same seeds; the second call is the recorded one (weight packing, workspace growth and the
refiner's graph capture happen in the first).

Run it ONCE on a checkout whose results are to be preserved, on the GPU:

    python tools/gen_golden_eval_passes.py
"""
import hashlib
import json
import os
import sys
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
OUT = os.path.join(ROOT, "tests", "golden", "eval_passes_parent.json")
DEV = "cuda"
S, L = 64, 100
SEED = 5                                    # torch's seed at the start of every call (the loaders and the default draws key on it)
BATCHES = (2, 2, 1)
LARGE = (80, 101)                           # 2 x 2 tiles of 64 at stride 48, ragged both ways; 3 MS-SSIM levels (20 x 25 >= 11)


def _mods():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from importlib import import_module
    import vaegan_amd as V
    return V, import_module(PKG + ".ops"), import_module(PKG + ".data")


def images(n, H=S, W=S):
    """f32 [n,3,H,W] in [-1, 1]: tests/_nlm_ref.synthetic (a sinusoid, a disc, a ramp), shifted and dimmed per image."""
    import torch
    import _nlm_ref as NR
    base = NR.synthetic(H, W)[0]
    x = np.stack([np.roll(base, (7 * i, 5 * i), axis=(1, 2)) * (1.0 - 0.12 * i) for i in range(n)])
    return torch.from_numpy(x.astype(np.float32))


def randn(seed, *shape):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def nets(dtype="fp32", with_d=False, train=False):
    V, _, _ = _mods()
    V.configure_seed(42)
    e, g = V.Encoder([3, S, S], L, dtype=dtype), V.Generator(nz=L, img_size=S, dtype=dtype)
    d = V.Discriminator(img_size=S, dtype=dtype) if with_d else None
    for n in (g, d):
        if n is not None:
            n.apply(V.weights_init)
    for n in (e, g, d):
        if n is not None:
            n.to(DEV)
            n.train(train)
    return e, g, d


# ---- the cases: each builds its networks and inputs once and returns the call --------------------------------------------
def _denoise_eval(ms_ssim=False, given=False, inject=True, train=False):
    def make():
        V, _, _ = _mods()
        e, g, _ = nets(train=train)
        img = images(3).to(DEV)
        kw = dict(sigma=0.1, ms_ssim=ms_ssim)
        if inject:
            kw.update(eps=randn(11, 3, 3, S, S).to(DEV), eps_z=randn(12, 3, L).to(DEV))
        if given:
            kw["noisy"] = (img + 0.1 * randn(13, 3, 3, S, S).to(DEV)).clamp(-1, 1)
            kw.pop("eps", None), kw.pop("eps_z", None)           # noisy= given and nothing injected: only eps_z is drawn
        return lambda: V.denoise_eval(e, g, img, **kw)
    return make


def _validation_epoch(ms_ssim=False, inject=True, dtype="fp32"):
    def make():
        V, _, _ = _mods()
        e, g, _ = nets(dtype)
        loader = list(images(sum(BATCHES)).to(DEV).split(BATCHES))
        draws = [(randn(20 + i, b, 3, S, S).to(DEV), randn(30 + i, b, L).to(DEV)) for i, b in enumerate(BATCHES)]
        noise_fn = (lambda i, img: draws[i]) if inject else None
        return lambda: V.validation_epoch(e, g, loader, sigma=0.1, noise_fn=noise_fn, ms_ssim=ms_ssim)
    return make


def _draws_z():
    draws = [randn(60 + i, b, L).to(DEV) for i, b in enumerate(BATCHES)]
    return lambda i, noisy: draws[i]


def _paired_test_epoch(regions=False, ms_ssim=False, refine=False, baseline=None):
    def make():
        import torch
        V, _, data = _mods()
        e, g, d = nets(with_d=refine)
        u8 = ((images(sum(BATCHES)) + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        ds = data.ResidentImages(u8, device=DEV)
        loader = data.DeviceLoader(ds, torch.arange(sum(BATCHES)), 2, shuffle=False, degrade=data.Degrade(0.25))
        refiner = V.LatentRefiner(e, g, d, steps=2, lr=0.05, alpha_adv=0.1, prior_weight=0.01) if refine else None
        noise_fn = _draws_z()
        return lambda: V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, regions=regions, ms_ssim=ms_ssim, refine=refiner,
                                           baseline=baseline)
    return make


def _pairs(batches, H, W, seed):
    clean = images(sum(batches), H, W)
    noisy = (clean + 0.1 * randn(seed, *clean.shape)).clamp(-1, 1)
    return list(zip(noisy.to(DEV).split(batches), clean.to(DEV).split(batches)))


def _paired_list():
    V, _, _ = _mods()
    e, g, _ = nets()
    pairs, noise_fn = _pairs(BATCHES, S, S, 70), _draws_z()
    return lambda: V.paired_test_epoch(e, g, pairs, noise_fn=noise_fn, baseline=dict(sigma=0.1))


def _tiled_denoise_eval(ms_ssim=False):
    def make():
        V, _, _ = _mods()
        e, g, _ = nets()
        img, eps = images(2, *LARGE).to(DEV), randn(80, 2, 3, *LARGE).to(DEV)
        return lambda: V.tiled_denoise_eval(e, g, img, sigma=0.1, eps=eps, ms_ssim=ms_ssim, stride=48, sample=False)
    return make


def _tiled_test_epoch(ms_ssim=False, baseline=None):
    def make():
        V, _, _ = _mods()
        e, g, _ = nets()
        pairs = _pairs((1, 2), *LARGE, 90)
        return lambda: V.tiled_test_epoch(e, g, pairs, ms_ssim=ms_ssim, baseline=baseline, stride=48, sample=False)
    return make


CASES = {
    "denoise_eval/injected": _denoise_eval(),
    "denoise_eval/injected_ms_ssim": _denoise_eval(ms_ssim=True),
    "denoise_eval/noisy_given": _denoise_eval(given=True),
    "denoise_eval/default_draws": _denoise_eval(inject=False),
    "denoise_eval/train_mode": _denoise_eval(train=True),       # BatchNorm follows module.training: batch statistics
    "validation_epoch/injected": _validation_epoch(),
    "validation_epoch/injected_ms_ssim": _validation_epoch(ms_ssim=True),
    "validation_epoch/default_draws": _validation_epoch(inject=False),
    "validation_epoch/bf16": _validation_epoch(dtype="bf16"),
    "paired_test_epoch/plain": _paired_test_epoch(),
    "paired_test_epoch/regions": _paired_test_epoch(regions=True),
    "paired_test_epoch/ms_ssim": _paired_test_epoch(ms_ssim=True),
    "paired_test_epoch/refine": _paired_test_epoch(refine=True),
    "paired_test_epoch/nlm": _paired_test_epoch(baseline="nlm"),
    "paired_test_epoch/all": _paired_test_epoch(regions=True, ms_ssim=True, refine=True, baseline="nlm"),
    "paired_test_epoch/list_nlm_sigma": _paired_list,
    "tiled_denoise_eval/plain": _tiled_denoise_eval(),
    "tiled_denoise_eval/ms_ssim": _tiled_denoise_eval(ms_ssim=True),
    "tiled_test_epoch/plain": _tiled_test_epoch(),
    "tiled_test_epoch/ms_ssim": _tiled_test_epoch(ms_ssim=True),
    "tiled_test_epoch/nlm_sigma": _tiled_test_epoch(baseline=dict(sigma=0.1)),
    "tiled_test_epoch/ms_ssim_nlm_sigma": _tiled_test_epoch(ms_ssim=True, baseline=dict(sigma=0.1)),
}


def encode(v):
    import torch
    if isinstance(v, torch.Tensor):
        t = v.detach().cpu().contiguous()
        return {"dtype": str(t.dtype), "shape": list(t.shape), "sha256": hashlib.sha256(t.numpy().tobytes()).hexdigest()}
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"a result of type {type(v).__name__} is not recorded")
    if isinstance(v, int):
        return v
    return "inf" if v == float("inf") else float(v).hex()


def _start(ops):
    """Every call starts from the same seeds and a fresh default noise stream."""
    import torch
    ops.reset_noise()
    torch.manual_seed(SEED)


def run_case(name):
    """-> the record of one case (module docstring)."""
    import torch
    _, ops, _ = _mods()
    call = CASES[name]()
    _start(ops)
    call()                                                      # warm-up: packs, workspaces, graph captures
    _start(ops)
    reads = [0]

    def counted(fn):
        def wrapper(self, *a, **kw):
            reads[0] += 1
            return fn(self, *a, **kw)
        return wrapper
    torch.cuda.synchronize()
    with mock.patch.object(torch.Tensor, "tolist", counted(torch.Tensor.tolist)), \
            mock.patch.object(torch.Tensor, "item", counted(torch.Tensor.item)):
        before = ops.launch_count()
        out = call()
        launches = ops.launch_count() - before
    host_reads = reads[0]
    return {"keys": list(out), "values": {k: encode(v) for k, v in out.items()}, "launches": launches,
            "host_reads": host_reads, "noise": ops.default_noise(torch.zeros(1, device=DEV).device).state.tolist()}


def main() -> None:
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    records = {name: run_case(name) for name in CASES}
    with open(out, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes,", len(records), "cases")


if __name__ == "__main__":
    main()
