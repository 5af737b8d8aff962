"""GPU: Resize + CenterCrop on the device (vg_resize_u8, include/vaegan_hip.h "Resize").  Every comparison is torch.equal /
array_equal on u8: the kernel against Pillow's recorded output (tests/golden/resize_pil.npz; the SHA-256 cases hash the
device output copied to the host), across band heights, batch sizes, index gathers, a source set beyond 2^32 bytes, and
end to end against the host (PIL) route of data.py."""
import os

import numpy as np
import pytest
import torch

import vaegan_amd as V
from test_resize_cpu import formula_image, load_cases, resize_contract

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops, data = V.ops, V.data


def dev_resize(a: np.ndarray, image_size, **kw) -> np.ndarray:
    t = torch.from_numpy(np.ascontiguousarray(a))[None].to(DEV)
    out = ops.resize_u8(t, data.resize_geometry(a.shape[0], a.shape[1], image_size), **kw)
    return out[0].cpu().numpy()


def formula_set(n, H, W, C, salt0=100):
    return torch.from_numpy(np.stack([formula_image(H, W, C, salt0 + i) for i in range(n)])).to(DEV)


def test_kernel_equals_pillow_on_every_recorded_case(golden_dir):
    for c, a, check in load_cases(golden_dir):
        check(dev_resize(a, c["image_size"]))


SEAM_CASES = ["celeba_int64", "hq1024_256", "up_64_100", "gray_50x70_64", "cmyk_celeba_int64", "celeba_218x64",
              "identity_37x53"]


def test_result_does_not_depend_on_the_band_height(golden_dir):
    cases = {c["name"]: (c, a, check) for c, a, check in load_cases(golden_dir)}
    for name in SEAM_CASES:
        c, a, check = cases[name]
        ch = c["out_shape"][0]
        for band in (1, 2, 3, 5, 8, 13, 32, ch):
            geom = data.resize_geometry(c["H"], c["W"], c["image_size"])
            if ops.resize_u8_lds_bytes(c["H"], c["W"], c["C"], geom, 1, band) < 0:
                with pytest.raises(RuntimeError, match="VG_EINVAL"):          # a band too tall for LDS is refused, not served
                    dev_resize(a, c["image_size"], band=band)
                continue
            check(dev_resize(a, c["image_size"], band=band))


@pytest.mark.parametrize("H,W,C,size", [(218, 178, 3, 64), (256, 256, 3, (128, 128)), (50, 70, 1, (64, 64)),
                                        (37, 53, 4, (64, 16))])
def test_batch_of_one_and_of_257_give_the_same_bytes(H, W, C, size):
    src = formula_set(5, H, W, C)
    geom = data.resize_geometry(H, W, size)
    ones = torch.cat([ops.resize_u8(src[i:i + 1].clone(), geom) for i in range(5)])     # B = 1 launches
    for i in range(5):
        assert np.array_equal(ones[i].cpu().numpy(), resize_contract(src[i].cpu().numpy(), size))
    idx = (torch.arange(257, device=DEV) * 3) % 5
    many = ops.resize_u8(src, geom, idx=idx)                                            # B = 257
    assert many.shape[0] == 257 and torch.equal(many, ones[idx])


def test_idx_gather_permuted_and_repeated():
    src = formula_set(23, 218, 178, 3)
    geom = data.resize_geometry(218, 178, 64)
    every = ops.resize_u8(src, geom)
    assert tuple(every.shape) == (23, 64, 64, 3)
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(23, generator=g).to(DEV)
    assert torch.equal(ops.resize_u8(src, geom, idx=perm), every[perm])
    rep = torch.tensor([4, 4, 0, 22, 4, 22, 0, 0, 7], device=DEV)
    assert torch.equal(ops.resize_u8(src, geom, idx=rep), every[rep])
    out = torch.zeros(9, 64, 64, 3, dtype=torch.uint8, device=DEV)
    assert ops.resize_u8(src, geom, idx=rep, out=out) is out and torch.equal(out, every[rep])
    with pytest.raises(RuntimeError):
        ops.resize_u8(src, geom, idx=rep, out=torch.zeros(8, 64, 64, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.resize_u8(src, geom, idx=rep.to(torch.int32))


def test_source_set_beyond_4_gib_uses_64_bit_offsets(golden_dir):
    cases = {c["name"]: (c, a, check) for c, a, check in load_cases(golden_dir)}
    c, a, check = cases["celeba_int64"]
    base = torch.cat([torch.from_numpy(a)[None].to(DEV), formula_set(6, 218, 178, 3)])  # image 0: the fixture's own input
    geom = data.resize_geometry(218, 178, 64)
    want = ops.resize_u8(base, geom)
    check(want[0].cpu().numpy())                                                        # fixture-checked ...
    for i in range(1, 7):
        assert np.array_equal(want[i].cpu().numpy(), resize_contract(base[i].cpu().numpy(), 64))   # ... or contract-checked
    N = 40000
    which = torch.arange(N, device=DEV) % 7
    big = base[which]
    assert big.numel() > 2 ** 32 and big.is_contiguous()
    idx = torch.cat([torch.arange(0, 100), torch.arange(N // 2 - 50, N // 2 + 50), torch.arange(N - 100, N)]).to(DEV)
    got = ops.resize_u8(big, geom, idx=idx)
    assert torch.equal(got, want[which[idx]])
    del big


def test_one_raw_256_set_feeds_the_size_family():
    raw = V.ResidentImages(formula_set(6, 256, 256, 3), DEV)
    host = raw.images.cpu().numpy()
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for S in (64, 128, 256):
        ds = raw.resized(S)
        assert isinstance(ds, V.ResidentImages) and tuple(ds.images.shape) == (6, S, S, 3) and ds.image_shape == (3, S, S)
        for i in range(6):
            if Image is not None:
                want = np.asarray(data._resize_center_crop(Image.fromarray(host[i]), S))
            else:
                want = resize_contract(host[i], S)
            assert np.array_equal(ds.images[i].cpu().numpy(), want), (S, i)
        assert torch.equal(raw.resized(S, chunk=4).images, ds.images)                   # chunk bounds the launch only
        assert torch.equal(raw.resized((S, S)).images, ds.images)
    same = raw.resized(256)
    assert torch.equal(same.images, raw.images) and same.images.data_ptr() != raw.images.data_ptr()   # a copy
    b = ds.batch(torch.tensor([1, 3], device=DEV))                                      # the new set serves loaders as any other
    assert tuple(b.shape) == (2, 3, 256, 256)


def test_launch_is_capturable_in_a_graph():
    src = formula_set(9, 218, 178, 3)
    geom = data.resize_geometry(218, 178, 64)
    idx = torch.tensor([8, 1, 1, 5], device=DEV)
    eager = ops.resize_u8(src, geom, idx=idx)                           # also uploads and caches the coefficient tables
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):                             # one stream, no parallel branches
            ops.resize_u8(src, geom, idx=idx, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    idx.copy_(torch.tensor([0, 2, 3, 4], device=DEV))                   # the graph reads idx at replay time
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.resize_u8(src, geom)[idx])


@pytest.fixture(scope="module")
def celeba_like_folder(tmp_path_factory):
    Image = pytest.importorskip("PIL.Image")
    d = tmp_path_factory.mktemp("celeba_178x218")
    rng = np.random.default_rng(9)
    for i in range(40):
        yy, xx = np.mgrid[0:218, 0:178]
        base = np.stack([(yy * 3 + i * 5) % 256, (xx * 5 + i * 7) % 256, ((yy * xx >> 4) + i * 11) % 256], -1)
        img = np.clip(base + rng.integers(-25, 25, base.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img, "RGB").save(os.path.join(d, f"{i:05d}.jpg"), quality=90)
    return str(d)


@pytest.mark.parametrize("size", [64, (64, 64), 128])
def test_from_folder_device_route_equals_host_route(celeba_like_folder, size):
    host = data.ResidentImages.from_folder(celeba_like_folder, None, DEV, 1, image_size=size)
    dev = data.ResidentImages.from_folder(celeba_like_folder, None, DEV, 1, image_size=size, resize_on="device")
    assert dev.images.dtype == torch.uint8 and torch.equal(dev.images, host.images) and dev.raw is None
    kept = data.ResidentImages.from_folder(celeba_like_folder, None, DEV, 1, image_size=size, resize_on="device",
                                           keep_raw=True, chunk=16)
    assert torch.equal(kept.images, host.images) and tuple(kept.raw.images.shape) == (40, 218, 178, 3)
    assert torch.equal(kept.raw.images.cpu(), data.decode_folder(celeba_like_folder, workers=1))
    assert torch.equal(data.decode_folder(celeba_like_folder, workers=1, image_size=size, resize_on="device"),
                       kept.raw.images.cpu())
    small = data.ResidentImages.from_folder(celeba_like_folder, None, DEV, 1, image_size=size, resize_on="device", chunk=7)
    assert torch.equal(small.images, host.images)


@pytest.mark.parametrize("noise_max_std", [None, 0.25])
def test_lq_loaders_device_route_equals_host_route(celeba_like_folder, noise_max_std):
    def batches(**kw):
        V.configure_seed(42)
        tl, vl, shape = data.get_dataset_loaders(batch_size=8, device=DEV, workers=1, dataset_type="LQ", image_size=64,
                                                 noise_max_std=noise_max_std, **kw)
        assert tuple(shape) == (3, 64, 64)
        return [b for loader in (tl, vl) for b in loader]

    host = batches(path=celeba_like_folder)
    dev = batches(path=celeba_like_folder, resize_on="device")
    raw = data.ResidentImages(data.decode_folder(celeba_like_folder, workers=1), DEV)
    from_raw = batches(path=raw, resize_on="device")                    # one raw resident set, resized for the loaders
    assert len(host) == len(dev) == len(from_raw) == 6
    for h, d, r in zip(host, dev, from_raw):
        if noise_max_std is None:
            assert torch.equal(h, d) and torch.equal(h, r)
        else:                                                           # (noisy, clean): the degraded pairs are equal too
            assert torch.equal(h[0], d[0]) and torch.equal(h[1], d[1]) and torch.equal(h[0], r[0]) and torch.equal(h[1], r[1])
    V.configure_seed(42)
    tl, _, shape = data.get_dataset_loaders(raw, batch_size=8, device=DEV, dataset_type="LQ", image_size=64)
    assert tuple(shape) == (3, 218, 178)                                # without resize_on="device" a passed set is used as it is
