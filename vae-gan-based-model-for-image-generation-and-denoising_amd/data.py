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
``image_size`` (``decode_folder`` / ``from_folder`` / 'LQ'): V0's ``Resize`` + ``CenterCrop`` (:26-30) at decode time on
the host with PIL, so the resident set is already at the training size.
"""
from functools import partial
import glob
import os
from multiprocessing import Pool, cpu_count
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from . import ops


def _resize_center_crop(img, image_size):
    """transforms.Resize(image_size) + transforms.CenterCrop(image_size) (dataset_code.py:27-28) on a PIL image, restated
    from torchvision's PIL path: an int resizes the SHORTER edge to it (longer edge int(size * long / short)), an (h, w)
    pair resizes to exactly that; ``img.resize((w, h), BILINEAR)``; the crop window starts at int(round((H - h) / 2)).
    Parity unpinned against torchvision (the package is not installed here)."""
    from PIL import Image
    w, h = img.size
    if isinstance(image_size, int):
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = image_size, int(image_size * long / short)
        new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
        ch = cw = image_size
    else:
        ch, cw = (int(v) for v in image_size)
        new_h, new_w = ch, cw
    if (new_w, new_h) != (w, h):
        img = img.resize((new_w, new_h), Image.BILINEAR)
    if new_h < ch or new_w < cw:
        raise RuntimeError("CenterCrop larger than the resized image (padding) is not supported")
    top, left = int(round((new_h - ch) / 2.0)), int(round((new_w - cw) / 2.0))
    return img.crop((left, top, left + cw, top + ch))


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


def decode_folder(image_folder: str, dataset_size: Optional[int] = None, workers: Optional[int] = None,
                  image_size=None) -> torch.Tensor:
    """-> uint8 tensor [N, H, W, 3] on the host (all images must share one size, as CelebA-HQ does).
    image_size (int or (h, w)): CelebADatasetV0's Resize + CenterCrop at decode time (_resize_center_crop), e.g. a folder
    of 178 x 218 CelebA files becomes a 64 x 64 set; None: the files as they are."""
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
    that value mapping."""

    def __init__(self, noise_max_std: Optional[float], rect: bool = True, normalize: bool = True):
        if noise_max_std is not None and not noise_max_std >= 0:
            raise ValueError("noise_max_std must be >= 0 or None")
        self.noise_max_std, self.rect, self.normalize = noise_max_std, bool(rect), bool(normalize)

    @property
    def pairs(self) -> bool:
        return self.noise_max_std is not None

    def __repr__(self):
        return f"Degrade(noise_max_std={self.noise_max_std}, rect={self.rect}, normalize={self.normalize})"


class ResidentImages:
    """The decoded image set in HBM: u8 [N, H, W, C].  ``ds[i]`` returns what ``CelebAHQDataset[i]`` returns
    (f32 [C,H,W] in [-1,1]) -- as a device tensor."""

    def __init__(self, images_u8: torch.Tensor, device="cuda"):
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
            raise RuntimeError("ResidentImages needs a uint8 [N,H,W,C] tensor")
        self.images = images_u8.to(device).contiguous()
        if not self.images.is_cuda:
            raise RuntimeError("ResidentImages lives in MI355X HBM ('cuda'); there is no CPU path")

    @classmethod
    def from_folder(cls, image_folder: str, dataset_size: Optional[int] = None, device="cuda", workers=None,
                    image_size=None):
        return cls(decode_folder(image_folder, dataset_size, workers, image_size), device)

    def __len__(self) -> int:
        return self.images.shape[0]

    @property
    def image_shape(self) -> Tuple[int, int, int]:
        n, h, w, c = self.images.shape
        return (c, h, w)                                           # dataset[0].numpy().shape (:178)

    def batch(self, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return ops.gather_normalize_u8(self.images, idx, out)

    def pair(self, idx: torch.Tensor, seed: int, pos0: int, degrade: Degrade, out: Optional[torch.Tensor] = None,
             nhwc=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (noisy, clean), both [B,C,H,W] f32, what a batch of ``CelebADatasetV0[i]`` with noise_max_std set collates
        to (dataset_code.py:64-65).  seed: the epoch's seed; pos0: position of idx[0] in the epoch's order (sample k of
        the batch is keyed by pos0 + k).  out: receives ``clean``.  nhwc: a [B,H,W,CP] engine tensor that also receives
        ``noisy`` in the Encoder's input layout.  degrade.noise_max_std None: sigma 0 and no rectangle (noisy == clean)."""
        _, H, W, _ = self.images.shape
        rect = degrade.rect and degrade.pairs
        noisy, clean, _ = ops.gather_degrade_u8(self.images, idx, seed, pos0, degrade.noise_max_std or 0.0, rect,
                                                degrade.normalize, degrade_bounds(H, W) if rect else None,
                                                out_clean=out, nhwc=nhwc)
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
        training target and the trainer's input); ``noisy`` is always a fresh tensor."""
        self._out = out

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
            noisy, clean = self.dataset.pair(idx, self.last_base_seed, lo, self.degrade, dst, nhwc)
            self.last_nhwc = nhwc
            yield (noisy, clean) if self.degrade.pairs else clean


def get_dataset_loaders(path, batch_size=64, train_p=0.9, dataset_size=None, device="cuda", rank=0, world=1,
                        workers=None, dataset_type="HQ", image_size=(64, 64), noise_max_std=None, rect=True,
                        normalize=None):
    """dataset_code.py:167-178 -> (train_loader, test_loader, image_shape).
    dataset_type 'HQ' (:168-169): the files as they are, values (u/255 - 0.5)/0.5.  'LQ' (:170-171, CelebADatasetV0):
    Resize + CenterCrop to image_size at decode time, values u/255 (a ResidentImages passed as `path` is used as it is).
    normalize overrides the value mapping (default: True for 'HQ', False for 'LQ').  noise_max_std set: both loaders
    yield (noisy, clean) pairs with `rect` (the call the reference's own test script asks for, main_vae.py:240).
    The defaults are the 'HQ' clean-batch loaders."""
    if dataset_type not in ("HQ", "LQ"):
        raise ValueError("dataset_type must be 'HQ' or 'LQ'")
    lq = dataset_type == "LQ"
    if isinstance(path, ResidentImages):
        ds = path
    else:
        ds = ResidentImages.from_folder(path, dataset_size, device, workers, image_size if lq else None)
    normalize = (not lq) if normalize is None else bool(normalize)
    degrade = None if (noise_max_std is None and normalize) else Degrade(noise_max_std, rect, normalize)
    train_idx, test_idx = random_split_indices(len(ds), train_p)
    train = DeviceLoader(ds, train_idx, batch_size, shuffle=True, rank=rank, world=world, degrade=degrade)
    test = DeviceLoader(ds, test_idx, batch_size, shuffle=False, rank=rank, world=world, degrade=degrade)
    return train, test, ds.image_shape
