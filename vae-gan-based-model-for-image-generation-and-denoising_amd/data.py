"""Data path of the reference (dataset_code.py: ``CelebAHQDataset`` :137-165, ``CelebADatasetV0`` :13-65 and
``get_dataset_loaders`` :167-178), MI355X-first.

The reference preloads every decoded image into host RAM as float tensors and lets a DataLoader copy one batch per
step over PCIe.  Here the decoded images stay **u8 and resident in HBM** (CelebA-HQ 30 000 x 256 x 256 x 3 = 5.9 GB
of the 288 GB); a batch is assembled ON THE DEVICE from the sampler's indices by one HIP kernel that also applies
``ToTensor`` + ``Normalize((0.5,), (0.5,))`` (dataset_code.py:147-150) -- no per-step host work, no PCIe traffic,
4x less resident memory than f32, and the batch equals the reference's bit for bit.

What is reproduced exactly (checked against torch.utils.data in tests/test_data_cpu.py):
  * file order ``glob.iglob(folder/*.jpg)`` and ``dataset_size`` truncation (:141-145),
  * the 90/10 ``random_split`` (:175) -- ``randperm(n)`` from torch's default generator,
  * ``DataLoader(shuffle=True)`` order, batch boundaries and the ragged last batch (``drop_last=False``, the
    variable last-batch size of vaegan_code.py:67), including how much of the default RNG stream an epoch consumes
    (one int64 draw for the iterator's base seed, one for the sampler's private generator),
  * ``DataLoader(shuffle=False)`` for the validation split.
New (the reference is single-process): ``rank`` / ``world`` shard every global batch of ``world * batch_size``
samples contiguously over the ranks (same sample order as a single process with the global batch).
JPEG decoding is host work (PIL, a process pool as dataset_code.py:153-155); there is no device JPEG decoder here.

Degraded pairs (dataset_type 'LQ' / ``CelebADatasetV0`` with ``noise_max_std`` set, :35-65): a ``DeviceLoader`` built
with a ``Degrade`` yields ``(noisy, clean)``.  ONE HIP kernel (ops.gather_degrade_u8) reads the batch's u8 images once
and writes the clean batch, the degraded batch -- random rectangle of uniform noise, Gaussian noise whose standard
deviation is drawn per image, clamp to [-1, 1] -- and, on request, the degraded batch in the Encoder's NHWC input layout.
The random numbers are counter-based Philox draws keyed by (epoch seed, position of the sample in the epoch's order,
element), include/vaegan_hip.h "Degraded pairs": a sample's degradation does not depend on batch size, rank or world
size.  They cannot equal torch's CPU generator; the distribution and the arithmetic are the reference's
(tests/test_gpu_degrade.py).  The epoch seed is the int64 base seed that ``iter(DataLoader)`` draws from the default
generator -- the number a real DataLoader hands its workers as their RNG seed -- so ``utils.configure_seed`` governs
the noise, every epoch differs, and no default-RNG state is consumed beyond what the plain loader consumes.
Noise models (not in the reference): ``Degrade(noise_model="speckle" | "shot", impulse_max_p=, salt_ratio=)`` scales the same
normal by the intensity or its root and lays salt-and-pepper impulses on top, in the same kernel pass from the same keyed
draws (include/vaegan_hip.h "Degraded pairs", noise models; tests/test_gpu_noise_models.py); the defaults are the model above.
``image_size`` (``decode_folder`` / ``from_folder`` / 'LQ'): V0's ``Resize`` + ``CenterCrop`` (:26-30).  ``resize_on="host"``
(the default): at decode time with PIL, so the resident set is frozen at the size asked for.  ``resize_on="device"``: the
files are decoded ONCE at their own size and uploaded; ``ResidentImages.resized(image_size)`` then makes any member of
the size family from that raw set with one HIP kernel (ops.resize_u8) whose output equals PIL's byte for byte -- PIL's
8-bit bilinear resampler is integer arithmetic over a small coefficient table, which ``resample_coeffs`` builds on the
host in double exactly as PIL does (include/vaegan_hip.h "Resize"; tests/test_resize_cpu.py holds the restated contract
against recorded PIL output, tests/test_gpu_resize.py the kernel).  ``resize_geometry`` is the one place that turns an
``image_size`` into (Hr, Wr, top, left, ch, cw) for both routes.
"""
from functools import partial
import glob
import math
import os
from multiprocessing import Pool, cpu_count
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from . import ops


def resize_geometry(H: int, W: int, image_size) -> Tuple[int, int, int, int, int, int]:
    """transforms.Resize(image_size) + transforms.CenterCrop(image_size) (dataset_code.py:27-28) of an H x W image ->
    (Hr, Wr, top, left, ch, cw), restated from torchvision's PIL path: an int resizes the SHORTER edge to it (longer edge
    int(size * long / short)) and crops size x size, an (h, w) pair resizes to exactly that (the crop is a no-op); the crop
    window starts at int(round((Hr - ch) / 2)), python's round.  A crop larger than the resized image (torchvision would
    pad) raises.  Parity unpinned against torchvision (the package is not installed here)."""
    H, W = int(H), int(W)
    if isinstance(image_size, int):
        short, long = (W, H) if W <= H else (H, W)
        new_short, new_long = image_size, int(image_size * long / short)
        new_w, new_h = (new_short, new_long) if W <= H else (new_long, new_short)
        ch = cw = image_size
    else:
        ch, cw = (int(v) for v in image_size)
        new_h, new_w = ch, cw
    if new_h < ch or new_w < cw:
        raise RuntimeError("CenterCrop larger than the resized image (padding) is not supported")
    top, left = int(round((new_h - ch) / 2.0)), int(round((new_w - cw) / 2.0))
    return new_h, new_w, top, left, ch, cw


def _resize_center_crop(img, image_size):
    """resize_geometry on a PIL image: ``img.resize((Wr, Hr), BILINEAR)`` where the size changes, then the crop."""
    from PIL import Image
    w, h = img.size
    new_h, new_w, top, left, ch, cw = resize_geometry(h, w, image_size)
    if (new_w, new_h) != (w, h):
        img = img.resize((new_w, new_h), Image.BILINEAR)
    return img.crop((left, top, left + cw, top + ch))


RESAMPLE_PRECISION_BITS = 22                 # PIL's PRECISION_BITS = 32 - 8 - 2


def resample_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Coefficient table of one axis of PIL's 8-bit bilinear resampler, in_size -> out_size (include/vaegan_hip.h
    "Resize"; PIL's precompute_coeffs + normalize_coeffs_8bpc with the triangle filter): python floats are IEEE doubles
    and every line below is one of the contract's operations, in its order.
    -> (k int32 [out_size, ksize], bounds int32 [out_size, 2] = (xmin, n))."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resample_coeffs: sizes must be >= 1")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    one = float(1 << RESAMPLE_PRECISION_BITS)
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            p = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(-0.5 + p * one) if p < 0 else int(0.5 + p * one)
        bounds[xx] = (xmin, n)
    return k, bounds


def _decode(path: str, image_size=None) -> np.ndarray:
    from PIL import Image                      # torchvision's default_loader: Image.open(f).convert("RGB")
    with open(path, "rb") as f:
        img = Image.open(f).convert("RGB")
        if image_size is not None:
            img = _resize_center_crop(img, image_size)
        return np.asarray(img, dtype=np.uint8)


def list_images(image_folder: str, dataset_size: Optional[int] = None):
    paths = list(glob.iglob(os.path.join(image_folder, "*.jpg"), recursive=False))      # dataset_code.py:141-142
    if dataset_size is not None:
        paths = paths[:dataset_size]                                                     # :144-145
    return paths


def _check_resize_on(resize_on: str) -> bool:
    if resize_on not in ("host", "device"):
        raise ValueError("resize_on must be 'host' or 'device'")
    return resize_on == "device"


def decode_folder(image_folder: str, dataset_size: Optional[int] = None, workers: Optional[int] = None,
                  image_size=None, resize_on: str = "host") -> torch.Tensor:
    """-> uint8 tensor [N, H, W, 3] on the host (all images must share one size, as CelebA-HQ does).
    image_size (int or (h, w)): CelebADatasetV0's Resize + CenterCrop at decode time (_resize_center_crop), e.g. a folder
    of 178 x 218 CelebA files becomes a 64 x 64 set; None: the files as they are.
    resize_on="device": the files as they are whatever image_size says -- the caller resizes the uploaded set
    (ResidentImages.resized; from_folder does both)."""
    if _check_resize_on(resize_on):
        image_size = None
    paths = list_images(image_folder, dataset_size)
    if not paths:
        raise RuntimeError(f"no *.jpg files in {image_folder}")
    if workers is None:
        workers = max(1, cpu_count() - 2)                                                # :153
    if workers > 1 and len(paths) > 64:
        with Pool(workers) as pool:
            arrs = pool.map(partial(_decode, image_size=image_size), paths, chunksize=64)
    else:
        arrs = [_decode(p, image_size) for p in paths]
    shape = arrs[0].shape
    for p, a in zip(paths, arrs):
        if a.shape != shape:
            raise RuntimeError(f"{p}: image size {a.shape} differs from {shape} (the resident layout is one [N,H,W,3] array)")
    return torch.from_numpy(np.stack(arrs))


def degrade_bounds(H: int, W: int) -> Tuple[int, int, int, int, int, int]:
    """Integer ranges of add_random_rectangle (dataset_code.py:44-52) for an H x W image, with python's round() (banker's)
    as the reference: (min_size, max_size, x0, x1, y0, y1) -- rect_h, rect_w in [min_size, max_size],
    x in [x0, x1 - rect_w), y in [y0, y1 - rect_h).  64 x 64: (1, 16, 16, 49, 16, 49)."""
    m = min(H, W)
    return (round(m * 0.01), round(m * 0.25), round(W * 0.25), round(W * 0.75) + 1, round(H * 0.25), round(H * 0.75) + 1)


class Degrade:
    """Settings of the degraded-pair path (CelebADatasetV0's noise_max_std / rect, dataset_code.py:14) plus the value
    mapping: normalize=True maps bytes like the 'HQ' dataset, (u/255 - 0.5)/0.5 -- the range the clamp to [-1, 1] and the
    Tanh decoder assume; normalize=False is V0's literal u/255.  noise_max_std=None: clean batches only (no pairs), in
    that value mapping.
    noise_model (not in the reference; include/vaegan_hip.h "Degraded pairs", noise models): what the per-image level
    s * noise_max_std scales -- "gaussian" additive noise (the reference's), "speckle" noise proportional to the intensity
    (sonar), "shot" noise whose variance is proportional to the intensity (low light, ranging); the level is the standard
    deviation at white for all three.  impulse_max_p > 0 lays salt-and-pepper impulses on top (drop-outs and spurious
    returns): image b has hit probability s_b * impulse_max_p, a hit is white with probability salt_ratio, else black.
    The defaults are the reference's model, bit for bit what the loader made before it had these."""

    NOISE_MODELS = ("gaussian", "speckle", "shot")

    def __init__(self, noise_max_std: Optional[float], rect: bool = True, normalize: bool = True,
                 noise_model: str = "gaussian", impulse_max_p: float = 0.0, salt_ratio: float = 0.5):
        if noise_max_std is not None and not noise_max_std >= 0:
            raise ValueError("noise_max_std must be >= 0 or None")
        if noise_model not in self.NOISE_MODELS:
            raise ValueError(f"noise_model must be 'gaussian', 'speckle' or 'shot', got {noise_model!r}")
        for name, v in (("impulse_max_p", impulse_max_p), ("salt_ratio", salt_ratio)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:
                raise ValueError(f"{name} must be a number in [0, 1], got {v!r}")
        self.noise_max_std, self.rect, self.normalize = noise_max_std, bool(rect), bool(normalize)
        self.noise_model, self.impulse_max_p, self.salt_ratio = noise_model, float(impulse_max_p), float(salt_ratio)

    @property
    def pairs(self) -> bool:
        return self.noise_max_std is not None

    @property
    def pure_gaussian(self) -> bool:
        """Column 1 of the rectangle records (s * noise_max_std) is the standard deviation of additive Gaussian noise."""
        return self.noise_model == "gaussian" and self.impulse_max_p == 0.0

    @property
    def model_kw(self) -> dict:
        """The noise-model keywords of ops.gather_degrade_u8 / ops.degrade_params."""
        return dict(kind=self.noise_model, impulse_max_p=self.impulse_max_p, salt_ratio=self.salt_ratio)

    def __repr__(self):
        extra = ""
        if self.noise_model != "gaussian":
            extra += f", noise_model={self.noise_model!r}"
        if self.impulse_max_p != 0.0:
            extra += f", impulse_max_p={self.impulse_max_p}"
        if self.salt_ratio != 0.5:
            extra += f", salt_ratio={self.salt_ratio}"
        return f"Degrade(noise_max_std={self.noise_max_std}, rect={self.rect}, normalize={self.normalize}{extra})"


RESIZE_CHUNK = 8192          # images per resize launch / per upload of a raw set (218 x 178 x 3: 0.95 GB)


class ResidentImages:
    """The decoded image set in HBM: u8 [N, H, W, C].  ``ds[i]`` returns what ``CelebAHQDataset[i]`` returns
    (f32 [C,H,W] in [-1,1]) -- as a device tensor."""

    def __init__(self, images_u8: torch.Tensor, device="cuda"):
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
            raise RuntimeError("ResidentImages needs a uint8 [N,H,W,C] tensor")
        self.images = images_u8.to(device).contiguous()
        if not self.images.is_cuda:
            raise RuntimeError("ResidentImages lives in MI355X HBM ('cuda'); there is no CPU path")
        self.raw: Optional["ResidentImages"] = None                # from_folder(resize_on="device", keep_raw=True)

    @classmethod
    def from_folder(cls, image_folder: str, dataset_size: Optional[int] = None, device="cuda", workers=None,
                    image_size=None, resize_on: str = "host", keep_raw: bool = False, chunk: int = RESIZE_CHUNK):
        """resize_on="host": Resize + CenterCrop inside the decode pool (PIL), the set is uploaded at image_size.
        resize_on="device": the files are decoded at their own size, uploaded `chunk` images at a time and resized on the
        device (the same bytes); keep_raw=True keeps the uploaded raw set as ``.raw`` for further ``resized()`` calls,
        otherwise only one chunk of it is on the device at a time."""
        if not _check_resize_on(resize_on) or image_size is None:
            return cls(decode_folder(image_folder, dataset_size, workers, image_size), device)
        raw = decode_folder(image_folder, dataset_size, workers, None)
        N, H, W, C = raw.shape
        chunk = max(1, int(chunk))
        if keep_raw:
            up = torch.empty(raw.shape, dtype=torch.uint8, device=device)
            for lo in range(0, N, chunk):
                up[lo:lo + chunk].copy_(raw[lo:lo + chunk])
            rawset = cls(up, device)
            ds = rawset.resized(image_size, chunk)
            ds.raw = rawset
            return ds
        geom = resize_geometry(H, W, image_size)
        out = torch.empty(N, geom[4], geom[5], C, dtype=torch.uint8, device=device)
        for lo in range(0, N, chunk):
            ops.resize_u8(raw[lo:lo + chunk].to(device), geom, out=out[lo:lo + chunk])
        return cls(out, device)

    def resized(self, image_size, chunk: int = RESIZE_CHUNK) -> "ResidentImages":
        """A new resident set: every image of this one through Resize(image_size) + CenterCrop(image_size) on the device
        (ops.resize_u8; equals the host route's PIL bytes).  chunk: images per launch -- it bounds the launch size only."""
        if not self.images.is_cuda:
            raise RuntimeError("ResidentImages lives in MI355X HBM ('cuda'); there is no CPU path")
        N, H, W, C = self.images.shape
        geom = resize_geometry(H, W, image_size)
        dev = self.images.device
        out = torch.empty(N, geom[4], geom[5], C, dtype=torch.uint8, device=dev)
        chunk = max(1, int(chunk))
        if chunk >= N:
            ops.resize_u8(self.images, geom, out=out)
        else:
            order = torch.arange(N, dtype=torch.int64, device=dev)
            for lo in range(0, N, chunk):
                ops.resize_u8(self.images, geom, idx=order[lo:lo + chunk], out=out[lo:lo + chunk])
        return ResidentImages(out, dev)

    def __len__(self) -> int:
        return self.images.shape[0]

    @property
    def image_shape(self) -> Tuple[int, int, int]:
        n, h, w, c = self.images.shape
        return (c, h, w)                                           # dataset[0].numpy().shape (:178)

    def batch(self, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return ops.gather_normalize_u8(self.images, idx, out)

    def pair(self, idx: torch.Tensor, seed: int, pos0: int, degrade: Degrade, out: Optional[torch.Tensor] = None,
             nhwc=None, out_noisy: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (noisy, clean), both [B,C,H,W] f32, what a batch of ``CelebADatasetV0[i]`` with noise_max_std set collates
        to (dataset_code.py:64-65).  seed: the epoch's seed; pos0: position of idx[0] in the epoch's order (sample k of
        the batch is keyed by pos0 + k).  out: receives ``clean``.  nhwc: a [B,H,W,CP] engine tensor that also receives
        ``noisy`` in the Encoder's input layout.  out_noisy: receives ``noisy``.  degrade.noise_max_std None: sigma 0 and no
        rectangle (noisy == clean)."""
        _, H, W, _ = self.images.shape
        rect = degrade.rect and degrade.pairs
        noisy, clean, _ = ops.gather_degrade_u8(self.images, idx, seed, pos0, degrade.noise_max_std or 0.0, rect,
                                                degrade.normalize, degrade_bounds(H, W) if rect else None,
                                                out_clean=out, out_noisy=out_noisy, nhwc=nhwc, **degrade.model_kw)
        return noisy, clean

    def __getitem__(self, i: int) -> torch.Tensor:
        n = len(self)
        if not -n <= i < n:
            raise IndexError(i)
        return self.batch(torch.tensor([i % n], dtype=torch.int64, device=self.images.device))[0]


def random_split_indices(n: int, train_p: float = 0.9):
    """torch.utils.data.random_split(dataset, [train, test]) of dataset_code.py:172-175: one randperm(n) from
    torch's DEFAULT generator (so utils.configure_seed governs it), first ``round(train_p*n)`` indices train."""
    train_size = round(train_p * n)
    perm = torch.randperm(n)
    return perm[:train_size].clone(), perm[train_size:].clone()


class DeviceLoader:
    """Iterates batches of a subset of a ResidentImages set like ``DataLoader(Subset, batch_size, shuffle,
    num_workers=0, drop_last=False)`` would, yielding device tensors [b,C,H,W] f32.
    degrade: a ``Degrade`` -> the loader yields ``(noisy, clean)`` pairs like a DataLoader over ``CelebADatasetV0`` with
    noise_max_std set (clean batches in the Degrade's value mapping when its noise_max_std is None).  The epoch's seed
    is ``last_base_seed``; the pos0 of a batch is its ``lo`` of ``global_batches()``."""

    def __init__(self, dataset: ResidentImages, indices: torch.Tensor, batch_size: int = 64, shuffle: bool = False,
                 rank: int = 0, world: int = 1, degrade: Optional[Degrade] = None):
        if batch_size <= 0 or world <= 0 or not 0 <= rank < world:
            raise ValueError("bad batch_size / rank / world")
        idx = torch.as_tensor(indices, dtype=torch.int64).cpu()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(dataset)):
            raise IndexError("subset index outside the dataset")
        self.dataset, self.indices = dataset, idx
        self.batch_size, self.shuffle, self.rank, self.world = batch_size, shuffle, rank, world
        self.last_order: Optional[torch.Tensor] = None           # the epoch's sample order (host), for inspection
        self.last_base_seed: Optional[int] = None                # the epoch's base seed = seed of its degradation draws
        self.degrade = degrade
        self.last_nhwc: Optional[torch.Tensor] = None            # see want_nhwc()
        self._nhwc = None
        self.last_rects: Optional[torch.Tensor] = None           # see want_rects()
        self._rects = False
        self._out_noisy: Optional[torch.Tensor] = None           # see bind_noisy()

    def __len__(self) -> int:
        return sum(1 for _ in self.global_batches(self.indices.numel()))

    def global_batches(self, n: int):
        """(lo, hi) bounds of THIS rank's shard of every global batch of an epoch of n samples.
        world == 1: exactly DataLoader(drop_last=False): the ragged last batch is kept (vaegan_code.py:67).
        world  > 1: every rank must take the same number of steps with the SAME number of rows -- a rank without
        rows would miss the gradient all-reduce its peers wait in, and unequal shards make SUM/world differ from the
        global-batch gradient (ddp.py) and break the SyncBN element count.  The ragged last global batch is therefore
        cut down to the largest multiple of `world` (at most world-1 samples of an epoch are skipped; they come back
        in the next epoch's shuffle) and dropped when it has fewer samples than ranks."""
        B, W, r = self.batch_size, self.world, self.rank
        for start in range(0, n, B * W):
            stop = min(n, start + B * W)
            if W == 1:
                yield start, stop
                continue
            per = (stop - start) // W                                      # equal shards, remainder skipped
            if per == 0:
                return
            yield start + r * per, start + (r + 1) * per

    def epoch_order(self) -> torch.Tensor:
        """Consumes the default RNG exactly as one ``iter(DataLoader)`` + first ``next()`` does."""
        # _BaseDataLoaderIter: base seed (what a DataLoader hands its workers as their RNG seed), kept for the degradation
        self.last_base_seed = int(torch.empty((), dtype=torch.int64).random_().item())
        n = self.indices.numel()
        if self.shuffle:                                                   # RandomSampler.__iter__, generator=None
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
            g = torch.Generator()
            g.manual_seed(seed)
            perm = torch.randperm(n, generator=g)
        else:
            perm = torch.arange(n)
        return self.indices[perm]

    def bind_output(self, out: Optional[torch.Tensor]) -> None:
        """Assemble every FULL batch into `out` ([B, C, H, W] f32 on the device, e.g. VAEGANTrainer.graph_input()) and
        yield that same tensor: the consumer must be done with a batch before asking for the next (a training loop
        is).  A ragged last batch gets its own tensor.  None unbinds.  A degraded loader binds the CLEAN half (the
        training target and the trainer's input); ``noisy`` is a fresh tensor unless bind_noisy() binds it too."""
        self._out = out

    def bind_noisy(self, out: Optional[torch.Tensor]) -> None:
        """Degraded loaders only: assemble the ``noisy`` half of every FULL batch into `out` ([B, C, H, W] f32 on the device,
        e.g. VAEGANTrainer.graph_noisy_input()) and yield that same tensor, as bind_output does for the clean half.  A
        ragged last batch gets its own tensor.  None unbinds."""
        if out is not None and (self.degrade is None or not self.degrade.pairs):
            raise RuntimeError("bind_noisy: this loader does not yield degraded pairs")
        self._out_noisy = out

    def want_rects(self, on: bool) -> None:
        """Degraded loaders only: while on, ``last_rects`` holds the f32 [b, 8] device tensor of the batch just yielded --
        ops.degrade_params(last_base_seed, lo, b, ...) with this loader's Degrade and bounds: the occlusion rectangle of
        every image as the degradation kernel drew it (the region-weighted loss and the region metrics read it).  With
        rect=False the four geometry entries are 0: no hole.  Off: ``last_rects`` is None."""
        if on and (self.degrade is None or not self.degrade.pairs):
            raise RuntimeError("want_rects: this loader does not yield degraded pairs")
        self._rects = bool(on)
        if not on:
            self.last_rects = None

    def want_nhwc(self, CP: Optional[int], dtype: Optional[int] = None) -> None:
        """Degraded loaders only: also write every ``noisy`` batch in the Encoder's NHWC input layout ([b,H,W,CP] in the
        engine dtype) in the same kernel pass; ``last_nhwc`` holds it for the batch just yielded.  CP None turns it off."""
        if CP is not None and (self.degrade is None or not self.degrade.pairs):
            raise RuntimeError("want_nhwc: this loader does not yield degraded pairs")
        self._nhwc = None if CP is None else (int(CP), int(dtype))

    def __iter__(self) -> Iterator[torch.Tensor]:
        order = self.epoch_order()
        self.last_order = order
        dev_order = order.to(self.dataset.images.device)                   # one small H2D copy per epoch
        out = getattr(self, "_out", None)
        for lo, hi in self.global_batches(order.numel()):
            idx = dev_order[lo:hi]
            dst = out if out is not None and out.shape[0] == idx.numel() else None
            if self.degrade is None:
                yield self.dataset.batch(idx) if dst is None else self.dataset.batch(idx, dst)
                continue
            nhwc = None
            if self._nhwc is not None:
                nhwc = ops.empty_act((idx.numel(),) + tuple(self.dataset.images.shape[1:3]) + (self._nhwc[0],),
                                     self._nhwc[1], idx.device)
            bound = self._out_noisy
            dst_noisy = bound if bound is not None and bound.shape[0] == idx.numel() else None
            noisy, clean = self.dataset.pair(idx, self.last_base_seed, lo, self.degrade, dst, nhwc, dst_noisy)
            self.last_nhwc = nhwc
            if self._rects:
                H, W = self.dataset.images.shape[1:3]
                rect = self.degrade.rect and self.degrade.pairs
                self.last_rects = ops.degrade_params(self.last_base_seed, lo, idx.numel(), self.degrade.noise_max_std or 0.0,
                                                     rect, H, W, degrade_bounds(H, W) if rect else None, idx.device,
                                                     **self.degrade.model_kw)
            yield (noisy, clean) if self.degrade.pairs else clean


def get_dataset_loaders(path, batch_size=64, train_p=0.9, dataset_size=None, device="cuda", rank=0, world=1,
                        workers=None, dataset_type="HQ", image_size=(64, 64), noise_max_std=None, rect=True,
                        normalize=None, resize_on="host", noise_model="gaussian", impulse_max_p=0.0, salt_ratio=0.5):
    """dataset_code.py:167-178 -> (train_loader, test_loader, image_shape).
    dataset_type 'HQ' (:168-169): the files as they are, values (u/255 - 0.5)/0.5.  'LQ' (:170-171, CelebADatasetV0):
    Resize + CenterCrop to image_size, values u/255; resize_on="host": at decode time with PIL, "device": the files are
    decoded at their own size and resized on the device (same bytes).  A ResidentImages passed as `path` is used as it is,
    unless dataset_type is 'LQ' and resize_on="device": then it is taken as a raw set and ``path.resized(image_size)`` is
    what the loaders serve -- one raw resident set feeds every member of the size family.
    normalize overrides the value mapping (default: True for 'HQ', False for 'LQ').  noise_max_std set: both loaders
    yield (noisy, clean) pairs with `rect` (the call the reference's own test script asks for, main_vae.py:240);
    noise_model / impulse_max_p / salt_ratio are ``Degrade``'s (not in the reference; the defaults are its model).
    The defaults are the 'HQ' clean-batch loaders."""
    if dataset_type not in ("HQ", "LQ"):
        raise ValueError("dataset_type must be 'HQ' or 'LQ'")
    model = Degrade(noise_max_std, rect, True, noise_model, impulse_max_p, salt_ratio)      # validates before any decoding
    lq = dataset_type == "LQ"
    on_device = _check_resize_on(resize_on)
    if isinstance(path, ResidentImages):
        ds = path.resized(image_size) if (lq and on_device) else path
    else:
        ds = ResidentImages.from_folder(path, dataset_size, device, workers, image_size if lq else None, resize_on)
    normalize = (not lq) if normalize is None else bool(normalize)
    degrade = None if (noise_max_std is None and normalize) else Degrade(noise_max_std, rect, normalize, model.noise_model,
                                                                         model.impulse_max_p, model.salt_ratio)
    train_idx, test_idx = random_split_indices(len(ds), train_p)
    train = DeviceLoader(ds, train_idx, batch_size, shuffle=True, rank=rank, world=world, degrade=degrade)
    test = DeviceLoader(ds, test_idx, batch_size, shuffle=False, rank=rank, world=world, degrade=degrade)
    return train, test, ds.image_shape
