"""GPU: the noise models of the degraded pairs (vg_gather_degrade_u8_ex, vg_degrade_params_ex) and the median baseline
(vg_median_filter) against tests/_noise_models_ref.py.  As for the Gaussian pairs (tests/test_gpu_degrade.py) device draws cannot
equal a host generator, so the kernels are compared, bit for bit, with the restatement fed the MATERIALISED draws -- vg_randn
for the normals, vg_rand_u01 for the fill, impulse and salt uniforms -- and the impulse positions also with host Philox words.
Every expectation comes from the materialisers, the host reference and the contract text, never from the kernel under test."""
import math

import numpy as np
import pytest
import torch

import _noise_models_ref as R
import vaegan_amd as V
from test_gpu_data import jpeg_folder  # noqa: F401  (fixture: 45 generated 64 x 64 JPEGs)
from test_gpu_degrade import params_from_words, randn_at, state_at
from test_gpu_pairloss import assert_same_state, vae_state
from test_gpu_siblings import build_vae

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops, data, G, L = V.ops, V.data, V.geometry, V.ops.L
NAN = float("nan")
NMS, P_IMP, SALT = 0.3, 0.3, 0.4             # 0.3: not a power of two, so a contracted multiply-add would show
KINDS = ("gaussian", "speckle", "shot")


def nan_like(shape, offset=0):
    """A NaN-filled f32 tensor of `shape` that starts `offset` floats into its buffer -> (tensor, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + offset + 4,), NAN, dtype=torch.float32, device=DEV)
    return buf[offset:offset + n].view(shape), buf


def byte_images(N, H, W, C, seed):
    gen = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, generator=gen)
    images[0, :2] = 0
    images[0, 2:4] = 255                                                  # the extreme bytes are present
    return images


def clean_ref(images, idx, normalize):
    u = images[idx].permute(0, 3, 1, 2).numpy().astype(np.float32) / np.float32(255.0)
    return (u - np.float32(0.5)) / np.float32(0.5) if normalize else u


def restate(images, idx, seed, pos0, kind, p, rect, normalize, bounds):
    """-> (noisy, clean) f32 [B,C,H,W] numpy, every draw materialised on the device for (seed, pos0 + b)."""
    _, H, W, C = images.shape
    clean = clean_ref(images, idx, normalize)
    n_el = C * H * W
    out = []
    for b in range(len(idx)):
        pos = pos0 + b
        u = {d: ops.rand_u01(n_el, state_at(seed, pos), d).cpu().numpy().reshape(C, H, W)
             for d in (R.DRAW_FILL, R.DRAW_IMPULSE, R.DRAW_SALT)}
        n = randn_at(seed, pos, n_el, R.DRAW_NORMAL).cpu().numpy().reshape(C, H, W)
        s, rh, rw, x, y = params_from_words(seed, pos, rect, bounds)
        out.append(R.degrade_ref(clean[b], n, s, NMS, R.KINDS[kind], normalize, u[R.DRAW_FILL], (rh, rw, x, y) if rect else None,
                                 u[R.DRAW_IMPULSE], u[R.DRAW_SALT], p, SALT))
    return np.stack(out), clean


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint32)


def nhwc_ref(noisy, CP, dt):
    """The engine layout of a host f32 [B,C,H,W] batch: channels last, pad channels zero, bf16 by round-to-nearest-even."""
    B, C, H, W = noisy.shape
    y = torch.zeros(B, H, W, CP, dtype=torch.float32)
    y[..., :C] = torch.from_numpy(noisy).permute(0, 2, 3, 1)
    return y.to(torch.bfloat16).float() if dt == G.BF16 else y


# (B, C, H, W, seed): the seeds give non-empty rectangles at pos0 = 1000 (tests/_philox_ref.py words; asserted below)
SHAPES = {"quad_16x16": (3, 3, 16, 16, 20240607), "scalar_10x7": (2, 3, 10, 7, 3), "c1_12x12": (2, 1, 12, 12, 3),
          "c4_8x8": (2, 4, 8, 8, 3)}


@pytest.mark.parametrize("impulses", [False, True], ids=["plain", "impulses"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(SHAPES))
def test_pairs_equal_the_restatement_on_the_materialised_draws_bitwise(case, kind, impulses):
    B, C, H, W, seed = SHAPES[case]
    pos0, N = 1000, 5
    p = P_IMP if impulses else 0.0
    images = byte_images(N, H, W, C, H * 100 + W + C)
    idx = torch.tensor([(3 * b + 1) % N for b in range(B)])
    dimg, didx = images.to(DEV), idx.to(DEV)
    bounds = data.degrade_bounds(H, W)
    for rect in (True, False):
        for normalize in (True, False):
            want, want_clean = restate(images, idx, seed, pos0, kind, p, rect, normalize, bounds)
            if rect:
                geo = [params_from_words(seed, pos0 + b, True, bounds) for b in range(B)]
                assert any(rh > 0 and rw > 0 for _, rh, rw, _, _ in geo)
                if case == "quad_16x16":                                  # a rectangle edge inside a quad of four columns
                    assert any(rh > 0 and rw > 0 and (x % 4 or (x + rw) % 4) for _, rh, rw, x, _ in geo)
            for CP, dt in ((8, G.BF16), (4, G.F32)):
                clean, _ = nan_like((B, C, H, W))
                noisy, _ = nan_like((B, C, H, W))
                nhwc = ops.empty_act((B, H, W, CP), dt, DEV).fill_(NAN)
                ops.gather_degrade_u8(dimg, didx, seed, pos0, NMS, rect, normalize, bounds, out_clean=clean, out_noisy=noisy,
                                      nhwc=nhwc, kind=kind, impulse_max_p=p, salt_ratio=SALT)
                what = (case, kind, p, rect, normalize, CP)
                assert np.array_equal(bits(clean), bits(want_clean)), what
                assert np.array_equal(bits(noisy), bits(want)), what
                assert np.array_equal(bits(nhwc.float()), bits(nhwc_ref(want, CP, dt))), what
                assert torch.equal(nhwc, ops.nchw_to_nhwc(noisy, CP, dt)), what
            if impulses:
                lo = -1.0 if normalize else 0.0
                assert ((want == 1.0) | (want == lo)).sum() > 0


@pytest.mark.parametrize("impulses", [False, True], ids=["plain", "impulses"])
@pytest.mark.parametrize("kind", KINDS)
def test_outputs_off_the_16_byte_grid_take_the_scalar_kernel_and_write_the_quad_kernels_bits(kind, impulses):
    B, C, H, W, seed = SHAPES["quad_16x16"]
    p = P_IMP if impulses else 0.0
    images = byte_images(5, H, W, C, 77).to(DEV)
    idx = torch.tensor([4, 0, 2], device=DEV)
    bounds = data.degrade_bounds(H, W)
    kw = dict(kind=kind, impulse_max_p=p, salt_ratio=SALT)
    for normalize in (True, False):
        qn, qc, qy = ops.gather_degrade_u8(images, idx, seed, 1000, NMS, True, normalize, bounds, nhwc=(8, G.BF16), **kw)
        assert qn.data_ptr() % 16 == 0 and qc.data_ptr() % 16 == 0
        (clean, cbuf), (noisy, nbuf) = nan_like((B, C, H, W), 1), nan_like((B, C, H, W), 1)      # 4 bytes off
        assert noisy.data_ptr() % 16 == 4 and clean.data_ptr() % 16 == 4
        _, _, sy = ops.gather_degrade_u8(images, idx, seed, 1000, NMS, True, normalize, bounds, out_clean=clean, out_noisy=noisy,
                                         nhwc=(8, G.BF16), **kw)
        assert np.array_equal(bits(noisy), bits(qn)) and np.array_equal(bits(clean), bits(qc)) and torch.equal(sy, qy)
        n = B * C * H * W
        for buf in (cbuf, nbuf):
            assert bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[1 + n:]).all())


# ---- entry-point equivalences ------------------------------------------------------------------------------------------------
def gather_ex(images, idx, seed, pos0, nms, rect, normalize, bounds, kind, p, salt, CP, dt):
    """vg_gather_degrade_u8_ex called directly (ops routes the default model to the old entry point)."""
    N, H, W, C = images.shape
    B = idx.numel()
    clean, _ = nan_like((B, C, H, W))
    noisy, _ = nan_like((B, C, H, W))
    y = ops.empty_act((B, H, W, CP), dt, DEV).fill_(NAN)
    L.check(L.load().vg_gather_degrade_u8_ex(images.data_ptr(), N, idx.data_ptr(), B, C, H, W, seed, pos0, nms, int(rect),
                                             int(normalize), *(bounds if rect else (0,) * 6), clean.data_ptr(), noisy.data_ptr(),
                                             y.data_ptr(), CP, dt, kind, p, salt, L.stream_ptr()), "vg_gather_degrade_u8_ex")
    return noisy, clean, y


@pytest.mark.parametrize("shape", [(16, 16, 3), (10, 7, 3), (64, 64, 3)])
def test_new_entry_at_gaussian_without_impulses_writes_the_old_entrys_bits(shape):
    H, W, C = shape
    images = byte_images(6, H, W, C, 5).to(DEV)
    idx = torch.tensor([5, 1, 4, 2, 0, 3, 2], device=DEV)
    bounds = data.degrade_bounds(H, W)
    for rect in (True, False):
        for normalize in (True, False):
            for CP, dt in ((8, G.BF16), (4, G.F32)):
                on, oc, oy = ops.gather_degrade_u8(images, idx, 99, 40, NMS, rect, normalize, bounds, nhwc=(CP, dt))
                for salt in (0.5, 0.0):                                   # without impulses salt_ratio is inert
                    n, c, y = gather_ex(images, idx, 99, 40, NMS, rect, normalize, bounds, 0, 0.0, salt, CP, dt)
                    assert np.array_equal(bits(n), bits(on)) and np.array_equal(bits(c), bits(oc)) and torch.equal(y, oy)


def test_degrade_params_columns():
    H = W = 64
    bounds = data.degrade_bounds(H, W)
    B, seed, pos0 = 300, 424242, 17                                       # more than one workgroup of the parameter kernel
    old = ops.degrade_params(seed, pos0, B, NMS, True, H, W, bounds)
    assert bool((old[:, 6:] == 0).all())
    raw = torch.full((B, 8), NAN, device=DEV)
    L.check(L.load().vg_degrade_params_ex(seed, pos0, B, NMS, 1, H, W, *bounds, raw.data_ptr(), 0, 0.0, 0.5, L.stream_ptr()), "ex")
    assert np.array_equal(bits(raw), bits(old))                           # Gaussian, no impulses: today's row
    s = old[:, 0].cpu().numpy()
    for kind in KINDS:
        for p in (0.0, 0.3, 1.0):
            got = ops.degrade_params(seed, pos0, B, NMS, True, H, W, bounds, kind=kind, impulse_max_p=p, salt_ratio=0.25)
            assert np.array_equal(bits(got[:, :6]), bits(old[:, :6])), (kind, p)
            assert np.array_equal(bits(got[:, 6]), bits(s * np.float32(p))), (kind, p)
            assert bool((got[:, 7] == float(R.KINDS[kind])).all())
    host_s = np.array([R.severity(seed, pos0 + b) for b in range(B)], np.float32)
    assert np.array_equal(bits(s), bits(host_s))                          # ... and s is the host Philox word's
    with pytest.raises(ValueError, match="poisson"):
        ops.degrade_params(seed, pos0, B, NMS, True, H, W, bounds, kind="poisson")
    with pytest.raises(ValueError, match="impulse_max_p"):
        ops.degrade_params(seed, pos0, B, NMS, True, H, W, bounds, impulse_max_p=1.5)


# ---- impulse behaviour -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
def test_impulses_sit_where_the_host_philox_words_say_and_are_exactly_black_or_white(normalize):
    seed, C, H, W, B = 20240607, 3, 32, 32, 16
    images = byte_images(B, H, W, C, 21)
    images.clamp_(32, 224)                                                # no clean value within the noise of black or white
    dimg, idx = images.to(DEV), torch.arange(B, device=DEV)
    lo = -1.0 if normalize else 0.0
    for kind in ("gaussian", "shot"):
        plain = ops.gather_degrade_u8(dimg, idx, seed, 0, 0.01, False, normalize, kind=kind)[0].cpu().numpy()
        got = ops.gather_degrade_u8(dimg, idx, seed, 0, 0.01, False, normalize, kind=kind, impulse_max_p=0.3,
                                    salt_ratio=0.5)[0].cpu().numpy()
        assert not ((plain == 1.0) | (plain == lo)).any()                 # level 0.01: at most 0.068 from a clean value
        for b in range(B):
            hit, salt, _ = R.impulse_masks(seed, b, C * H * W, 0.3, 0.5)
            hit, salt = hit.reshape(C, H, W), salt.reshape(C, H, W)
            assert (got[b][salt] == 1.0).all() and (got[b][hit & ~salt] == lo).all()
            assert np.array_equal(bits(got[b][~hit]), bits(plain[b][~hit]))
            assert hit.sum() > 0 or R.severity(seed, b) * 0.3 * C * H * W < 5
    # salt_ratio 0 and 1
    for ratio, value in ((0.0, lo), (1.0, 1.0)):
        got = ops.gather_degrade_u8(dimg, idx, seed, 0, 0.01, False, normalize, impulse_max_p=0.3, salt_ratio=ratio)[0].cpu().numpy()
        for b in range(B):
            hit = R.impulse_masks(seed, b, C * H * W, 0.3, ratio)[0].reshape(C, H, W)
            assert (got[b][hit] == value).all()


@pytest.mark.parametrize("shape", [(16, 16), (10, 7)], ids=["quad", "scalar"])
def test_impulses_are_keyed_by_epoch_position_not_by_batch_slot(shape):
    H, W = shape
    images = byte_images(6, H, W, 3, 8).to(DEV)
    bounds = data.degrade_bounds(H, W)
    idx = torch.tensor([5, 1, 4, 2], device=DEV)
    kw = dict(kind="speckle", impulse_max_p=0.5, salt_ratio=0.5)
    whole = ops.gather_degrade_u8(images, idx, 99, 40, 0.25, True, True, bounds, **kw)[0]
    first = ops.gather_degrade_u8(images, idx[:2].contiguous(), 99, 40, 0.25, True, True, bounds, **kw)[0]
    second = ops.gather_degrade_u8(images, idx[2:].contiguous(), 99, 42, 0.25, True, True, bounds, **kw)[0]
    assert torch.equal(whole[:2], first) and torch.equal(whole[2:], second)
    other = ops.gather_degrade_u8(images, idx[2:].contiguous(), 99, 40, 0.25, True, True, bounds, **kw)[0]
    assert not torch.equal(other, second)


# ---- the median filter ---------------------------------------------------------------------------------------------------------------
def median_input(B, C, H, W, seed, ties):
    rng = np.random.default_rng(seed)
    if ties:                                                              # a few distinct values: windows full of equal elements
        return rng.integers(-3, 4, (B, C, H, W)).astype(np.float32) + np.float32(0.5)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    x[x == 0] = 1.0                                                       # no zeros of either sign
    return x


# all halo (2x2, 3x3), one 64 x 16 tile, ragged tiles in y (37x45), in x and y with and without 16-byte rows (19x131, 33x72)
MEDIAN_SHAPES = [(1, 2, 1, 2, 2), (1, 2, 3, 3, 7), (2, 2, 3, 3, 3), (2, 1, 4, 3, 7), (1, 3, 3, 16, 64), (2, 3, 3, 16, 64),
                 (1, 2, 3, 37, 45), (2, 2, 3, 37, 45), (1, 2, 1, 19, 131), (2, 2, 1, 19, 131), (1, 1, 4, 33, 72),
                 (2, 1, 4, 33, 72)]


@pytest.mark.parametrize("r,B,C,H,W", MEDIAN_SHAPES)
def test_median_filter_equals_the_restatement(r, B, C, H, W):
    for ties in (False, True):
        x = median_input(B, C, H, W, 1000 * r + H * W + C, ties)
        want = R.median_ref(x, r)
        got = ops.median_filter(torch.from_numpy(x).to(DEV), r)
        assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
        assert np.array_equal(got.cpu().numpy(), want), (r, B, C, H, W, ties)


@pytest.mark.parametrize("r,W,offset", [(1, 40, 8), (2, 40, 8), (1, 40, 5), (2, 45, 3)])
def test_median_filter_into_a_view_leaves_the_rest_of_the_buffer_alone(r, W, offset):
    B, C, H = 2, 3, 21
    x = median_input(B, C, H, W, 5, False)
    out, buf = nan_like((B, C, H, W), offset)
    assert (out.data_ptr() % 16 == 0) == (offset % 4 == 0)                # both store paths: 16-byte stores and single floats
    y = ops.median_filter(torch.from_numpy(x).to(DEV), r, out=out)
    assert y is out and np.array_equal(out.cpu().numpy(), R.median_ref(x, r))
    n = B * C * H * W
    assert bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all())


def test_median_filter_images_are_independent_and_a_graph_replay_equals_eager():
    r, B, C, H, W = 2, 5, 3, 23, 68
    x = torch.from_numpy(median_input(B, C, H, W, 9, False)).to(DEV)
    y = ops.median_filter(x, r)
    perm = torch.tensor([3, 0, 4, 1, 2], device=DEV)
    assert torch.equal(ops.median_filter(x[perm].contiguous(), r), y[perm])
    assert torch.equal(ops.median_filter(x[1:2].contiguous(), r), y[1:2])
    yg = torch.full_like(y, NAN)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):                                       # one stream, no parallel branches
            ops.median_filter(x, r, out=yg)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y)
    with pytest.raises(RuntimeError):
        ops.median_filter(x, r, out=x)
    with pytest.raises(RuntimeError):
        ops.median_filter(x, 3)
    with pytest.raises(RuntimeError):
        ops.median_filter(x[:, :, :2], 2)                                 # min(H, W) < r + 1
    assert torch.equal(V.Median(2)(x), y) and torch.equal(V.Median()(x), ops.median_filter(x, 1))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    S = 64
    V.configure_seed(42)
    e, g = V.Encoder([3, S, S], 100), V.Generator(nz=100, img_size=S)
    g.apply(V.weights_init)
    return e.to(DEV), g.to(DEV)


def test_loader_pairs_equal_pair_called_by_hand(jpeg_folder):  # noqa: F811
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    dg = data.Degrade(0.25, noise_model="shot", impulse_max_p=0.1)
    loader = data.DeviceLoader(ds, torch.arange(len(ds)), 16, shuffle=True, degrade=dg)
    loader.want_rects(True)
    torch.manual_seed(3)
    H, W = ds.images.shape[1:3]
    batches = 0
    for (lo, hi), (noisy, clean) in zip(loader.global_batches(len(ds)), loader):
        idx = loader.last_order[lo:hi].to(DEV)
        n2, c2 = ds.pair(idx, loader.last_base_seed, lo, dg)
        assert torch.equal(noisy, n2) and torch.equal(clean, c2)
        want = ops.degrade_params(loader.last_base_seed, lo, hi - lo, 0.25, True, H, W, data.degrade_bounds(H, W), kind="shot",
                                  impulse_max_p=0.1)
        assert torch.equal(loader.last_rects, want) and bool((want[:, 7] == 2).all())
        assert torch.equal(want[:, 6], want[:, 0] * 0.1)
        plain = ds.pair(idx, loader.last_base_seed, lo, data.Degrade(0.25))[0]
        assert not torch.equal(plain, noisy) and int(((noisy == 1) | (noisy == -1)).sum()) > int(((plain == 1) | (plain == -1)).sum())
        batches += 1
    assert batches == 3
    # get_dataset_loaders hands the three keywords to both loaders
    tl, vl, _ = data.get_dataset_loaders(ds, batch_size=8, noise_max_std=0.2, noise_model="speckle", impulse_max_p=0.05,
                                         salt_ratio=0.25)
    for ld in (tl, vl):
        assert (ld.degrade.noise_model, ld.degrade.impulse_max_p, ld.degrade.salt_ratio) == ("speckle", 0.05, 0.25)
    tl, vl, _ = data.get_dataset_loaders(ds, batch_size=8, noise_max_std=0.2)
    assert tl.degrade.pure_gaussian and vl.degrade.pure_gaussian


MEDIAN_KEYS = {"recon_loss_median", "ssim_median", "psnr_median"}
U = 2.0 ** -24


def test_paired_test_epoch_median_baseline_and_the_oracle_refusal(nets, jpeg_folder):  # noqa: F811
    e, g = nets
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    dg = data.Degrade(0.25, noise_model="shot", impulse_max_p=0.1)
    loader = data.DeviceLoader(ds, torch.arange(40, 45), 2, shuffle=False, degrade=dg)
    eps = [torch.randn(b, 100, generator=torch.Generator().manual_seed(60 + i)) for i, b in enumerate((2, 2, 1))]
    noise_fn = lambda i, noisy: eps[i].to(DEV)                                  # noqa: E731
    torch.manual_seed(5)
    base = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn)
    torch.manual_seed(5)
    got = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, baseline="median", ms_ssim=True)
    assert set(got) == set(base) | MEDIAN_KEYS | {"ms_ssim", "ms_ssim_noisy", "ms_ssim_median"}
    assert all(got[k] == base[k] for k in base) and not any(k.endswith("_nlm") for k in got)
    assert loader._rects is False and loader.last_rects is None              # the median reads no rectangles
    acc_ssim = acc_mse = acc_ms = 0.0
    seen = 0
    torch.manual_seed(5)
    for noisy, clean in loader:
        b = clean.shape[0]
        f = ops.median_filter(noisy.contiguous(), 1)
        slot = torch.empty(1, device=DEV)
        ops.mse_forward_backward(f, clean.contiguous(), 1.0, slot, False)
        acc_mse += b * float(slot)
        acc_ssim += b * float(ops.ssim(f, clean))
        acc_ms += b * float(ops.ms_ssim(f, clean))
        seen += b
    print("median", {k: got[k] for k in sorted(MEDIAN_KEYS)}, "noisy", got["psnr_noisy"], got["ssim_noisy"])
    # the pass accumulates b * value in f32 on the device, this loop in f64 on the host: a few f32 roundings
    assert got["recon_loss_median"] == pytest.approx(acc_mse / seen, rel=8 * U)
    assert got["ssim_median"] == pytest.approx(acc_ssim / seen, rel=8 * U)
    assert got["ms_ssim_median"] == pytest.approx(acc_ms / seen, rel=8 * U)
    assert got["psnr_median"] == pytest.approx(10 * math.log10(4.0 / (acc_mse / seen)), abs=1e-4)
    torch.manual_seed(5)
    r2 = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, baseline={"radius": 2})
    torch.manual_seed(5)
    r2b = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, baseline=V.Median(2))
    assert r2 == r2b and MEDIAN_KEYS <= set(r2) and r2["psnr_median"] != got["psnr_median"]
    # sigma="oracle" on a loader whose level is not a Gaussian sigma: refused; the blind estimate and a number run
    for bad in ("nlm", V.NLMeans(), dict(sigma="oracle")):
        with pytest.raises(ValueError, match="column 1"):
            V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, baseline=bad)
    torch.manual_seed(5)
    est = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, baseline={"sigma": "estimate"})
    assert {"recon_loss_nlm", "ssim_nlm", "psnr_nlm"} <= set(est) and math.isfinite(est["psnr_nlm"])
    assert all(est[k] == base[k] for k in base)
    # the tiled pass takes the median too
    torch.manual_seed(5)
    pairs = [(n.clone(), c.clone()) for n, c in loader]
    t = V.tiled_test_epoch(e, g, pairs, stride=48, sample=False, baseline="median")
    assert MEDIAN_KEYS <= set(t) and t["psnr_median"] == pytest.approx(got["psnr_median"], abs=1e-4)


def test_two_paired_vae_steps_on_a_speckle_loader_graphed_equal_eager(jpeg_folder):  # noqa: F811
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    dg = data.Degrade(0.25, noise_model="speckle", impulse_max_p=0.05)
    res = []
    for graphed in (False, True):
        e, g, tr = build_vae(64)
        loader = data.DeviceLoader(ds, torch.arange(8), 4, shuffle=False, degrade=dg)
        loader.want_rects(True)
        torch.manual_seed(7)
        out = []
        for step, (noisy, clean) in enumerate(loader):
            eps_z = torch.randn(4, 100, generator=torch.Generator().manual_seed(90 + step)).to(DEV)
            rects = loader.last_rects
            if graphed:
                out.append(tr.step_graphed(clean, None, eps_z, noisy=noisy, rects=rects, epoch=25).cpu().clone())
            else:
                out.append(tr.train_step(clean, None, eps_z, epoch=25, noisy=noisy, rects=rects).cpu().clone())
        assert len(out) == 2 and all(bool(torch.isfinite(v).all()) for v in out)
        res.append((out, vae_state(e, g, tr)))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert_same_state(res[0][1], res[1][1])
