"""CPU: tiled denoising before any kernel runs.  (1) tiling.tile_plan against the restatement tests/_tiling_ref.py: origins,
cover ranges, coefficient rows, refused plans; (2) the f64 blend against torch's F.fold on uniform-stride geometries; (3) the
exact-input cases of the GPU tests really are exact (every product and partial sum representable, held against Fraction
arithmetic), so a bitwise comparison there has no blind spot; (4) the C ABI declarations, the ctypes table, host-side argument
validation of the two entry points, the package exports and the "no CPU path" errors."""
import ctypes
import math
import os
import re
from fractions import Fraction
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _tiling_ref as R

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vg_tile_gather", "vg_tile_blend")
T = import_module(PKG + ".tiling")

# (H, W, S, stride, window): what the GPU tests blend bit for bit
EXACT_CASES = [(8, 8, 8, 4, "hann"), (20, 12, 8, 4, "tri"), (19, 13, 8, 8, "box")]


# ---- 1. the plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,S,stride,want", [
    (8, 8, 4, [0]),                                      # L == S: the single origin 0
    (20, 8, 4, [0, 4, 8, 12]),                           # regular: the last regular origin is the flush one
    (19, 8, 8, [0, 8, 11]),                              # ragged: one last tile flush with the edge
    (24, 8, 8, [0, 8, 16]),                              # stride = S, no overlap at all
    (12, 8, 1, [0, 1, 2, 3, 4]),                         # stride = 1
    (9, 8, 3, [0, 1]), (13, 8, 3, [0, 3, 5]), (37, 8, 3, [0, 3, 6, 9, 12, 15, 18, 21, 24, 27, 29])])
def test_origins(L, S, stride, want):
    assert R.origins(L, S, stride) == want
    assert T.axis_origins(L, S, stride).tolist() == want
    p = T.tile_plan(L, max(L, S), S, stride)
    assert p.oy.tolist() == want and p.ny == len(want)


@pytest.mark.parametrize("H,W,S,stride,window", EXACT_CASES + [
    (13, 37, 8, 3, "hann"), (37, 29, 8, 3, "hann"), (23, 9, 8, 2, "tri"), (12, 11, 8, 1, "hann"), (101, 80, 64, 48, "hann"),
    (64, 64, 64, None, "hann"), (200, 130, 64, None, "tri")])
def test_plan_equals_the_restatement(H, W, S, stride, window):
    p, q = R.plan(H, W, S, stride, window), T.tile_plan(H, W, S, stride, window)
    assert R.same_plan(p, q)
    assert q.stride == (S // 2 if stride is None else stride)
    assert (q.cover_y, q.cover_x) == (int(p.count_y.max()), int(p.count_x.max()))
    bound = math.ceil(S / q.stride) + 1
    assert q.cover_y <= bound and q.cover_x <= bound
    for first, count, coef, n, L in ((q.first_y, q.count_y, q.coef_y, q.ny, H), (q.first_x, q.count_x, q.coef_x, q.nx, W)):
        assert first.min() >= 0 and count.min() >= 1 and (first + count).max() <= n
        for pp in range(L):                                             # unused slots 0, used slots positive
            assert np.all(coef[pp, :count[pp]] > 0) and np.all(coef[pp, count[pp]:] == 0)
        s = coef.astype(np.float64).sum(axis=1)                         # every row sums to 1 within 2 ulp (of 1.0, f32)
        assert np.abs(s - 1.0).max() <= 2 * 2.0 ** -23, np.abs(s - 1.0).max()


def test_cover_bound_is_never_passed_and_is_reached():
    """ceil(S / stride) + 1 bounds the cover count.  It is reached where the flush tile can lie off the stride lattice inside
    a fully covered stretch (the common strides below); with stride 1 the flush tile is on the lattice and the most is S."""
    seen = {}
    for S in (4, 7, 8, 16):
        for stride in range(1, S + 1):
            bound = math.ceil(S / stride) + 1
            most = 0
            for L in range(S, 4 * S + 3):
                _, _, count, _ = R.axis(L, S, stride, R.window("box", S))
                assert count.max() <= bound
                most = max(most, int(count.max()))
            seen[S, stride] = most
    for S, stride in ((8, 4), (8, 2), (8, 3), (7, 4), (16, 8), (16, 2), (8, 8)):
        assert seen[S, stride] == math.ceil(S / stride) + 1
    assert seen[8, 1] == 8 and seen[16, 1] == 16
    assert T.VG_TILE_MAX_COVER == R.MAX_COVER == 8


@pytest.mark.parametrize("name", T.WINDOWS)
@pytest.mark.parametrize("S", [1, 2, 7, 8, 64, 256])
def test_windows_are_positive_and_symmetric(name, S):
    w = T.window_weights(name, S)
    assert w.dtype == np.float64 and w.shape == (S,) and np.all(w > 0) and np.allclose(w, w[::-1], rtol=0, atol=1e-15)
    assert np.array_equal(w, R.window(name, S))
    if name == "tri" and S == 8:
        assert np.array_equal(w * 8, [1, 3, 5, 7, 7, 5, 3, 1])


@pytest.mark.parametrize("args", [(7, 8, 8), (8, 7, 8), (16, 16, 8, 0), (16, 16, 8, -1), (16, 16, 8, 9), (33, 16, 16, 2), (16, 33, 16, 2),
                                  (16, 16, 8, 4, "gauss"), (16, 16, 0)])
def test_refused_plans(args):
    with pytest.raises(RuntimeError):
        T.tile_plan(*args)


def test_cover_above_the_table_width_is_refused_only_where_it_occurs():
    assert T.tile_plan(12, 12, 8, 1).cover_y == 5                            # stride 1, but the image is short: cover 5
    assert T.tile_plan(16, 15, 8, 1).cover_y == 8                            # stride 1: the flush tile is on the lattice
    assert T.tile_plan(32, 32, 16, 2).cover_y == 8                           # S / stride = 8 with the flush tile on the lattice
    with pytest.raises(RuntimeError, match="VG_TILE_MAX_COVER"):
        T.tile_plan(33, 32, 16, 2)                                           # origins 0, 2, ..., 16 and the flush tile at 17: 9 at y = 17


def test_cached_plan_returns_one_object_per_geometry():
    a, b = T.cached_plan(20, 12, 8, 4, "tri"), T.cached_plan(20, 12, 8, 4, "tri")
    assert a is b and T.cached_plan(20, 12, 8, 4, "box") is not a


# ---- 2. the f64 blend against F.fold ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,S,stride,window", [(20, 12, 8, 4, "tri"), (24, 16, 8, 8, "box"), (17, 23, 8, 3, "hann"),
                                                 (12, 11, 8, 1, "hann"), (8, 8, 8, 4, "hann")])
def test_f64_blend_equals_fold_over_fold(H, W, S, stride, window):
    p = R.plan(H, W, S, stride, window)
    assert p.oy.tolist() == list(range(0, H - S + 1, stride)) and p.ox.tolist() == list(range(0, W - S + 1, stride))   # uniform
    N, C = 2, 3
    rng = np.random.default_rng(5)
    tiles = rng.uniform(-1, 1, size=(N * p.ny * p.nx, C, S, S))
    w2 = torch.from_numpy(np.outer(p.w, p.w))
    t = torch.from_numpy(tiles).view(N, p.ny * p.nx, C, S, S)
    cols = (t * w2).permute(0, 2, 3, 4, 1).reshape(N, C * S * S, p.ny * p.nx)
    wcols = w2.reshape(1, S * S, 1).expand(1, S * S, p.ny * p.nx)
    want = F.fold(cols, (H, W), S, stride=stride) / F.fold(wcols, (H, W), S, stride=stride)
    got = R.blend_f64(p, tiles)
    assert np.abs(got - want.numpy()).max() <= 1e-12
    # and the f32 contract stays within the counted bound of it
    assert np.abs(R.blend_f32(p, tiles.astype(np.float32)).astype(np.float64)
                  - R.blend_f64(p, tiles.astype(np.float32))).max() <= R.blend_bound(p, 1.0)


# ---- 3. the exact cases are exact ------------------------------------------------------------------------------------
def _exact_blend(p, tiles):
    """The contract in Fraction arithmetic, asserting that every product and every partial sum is an f32 number."""
    def f32_exact(v):
        assert Fraction(float(np.float32(float(v)))) == v, v
        return v
    S, per = p.S, p.ny * p.nx
    N, C = tiles.shape[0] // per, tiles.shape[1]
    r = tiles.reshape(N, p.ny, p.nx, C, S, S)
    out = np.zeros((N, C, p.H, p.W), dtype=np.float32)
    for n in range(N):
        for c in range(C):
            for y in range(p.H):
                for x in range(p.W):
                    acc = Fraction(0)
                    for jy in range(p.count_y[y]):
                        ky = p.first_y[y] + jy
                        inner = Fraction(0)
                        for jx in range(p.count_x[x]):
                            kx = p.first_x[x] + jx
                            t = f32_exact(Fraction(float(p.coef_x[x, jx])) * Fraction(float(r[n, ky, kx, c, y - p.oy[ky], x - p.ox[kx]])))
                            inner = f32_exact(inner + t)
                        acc = f32_exact(acc + f32_exact(Fraction(float(p.coef_y[y, jy])) * inner))
                    out[n, c, y, x] = float(acc)
    return out


@pytest.mark.parametrize("H,W,S,stride,window", EXACT_CASES)
def test_exact_blend_cases_are_exact(H, W, S, stride, window):
    p = R.plan(H, W, S, stride, window)
    for coef in (p.coef_y, p.coef_x):                                       # dyadic: multiples of 1/8
        assert np.array_equal(coef * 8, np.round(coef * 8))
    if window == "box" and stride == 8:
        assert p.oy.tolist() == [0, 8, 11] and np.all(p.coef_y[11:16, :2] == 0.5) and np.all(p.coef_y[16:, 0] == 1.0)
    tiles = R.exact_tiles(p.ny * p.nx, 1, S, seed=H)
    want = _exact_blend(p, tiles)
    assert np.array_equal(R.blend_f32(p, tiles), want)
    if window != "hann":                                                     # the window itself is dyadic: the f64 form is exact too
        assert np.array_equal(R.blend_f64(p, tiles), want.astype(np.float64))
    if (H, W) == (S, S):
        assert np.array_equal(want, tiles.reshape(1, 1, S, S))                # one tile: the output is the tile


def test_hand_made_dyadic_tables_are_exact():
    p = R.dyadic_tables(R.plan(23, 9, 8, 2, "tri"), 5)
    assert int(p.count_y.max()) == 5 and p.coef_y.shape == (23, 5) and p.coef_x.shape == (9, 5)
    for coef, count in ((p.coef_y, p.count_y), (p.coef_x, p.count_x)):
        assert np.array_equal(coef.sum(axis=1), np.ones(coef.shape[0], dtype=np.float32))
        assert all(np.all(coef[q, count[q]:] == 0) for q in range(coef.shape[0]))
    tiles = R.exact_tiles(p.ny * p.nx, 1, 8, seed=23)
    assert np.array_equal(R.blend_f32(p, tiles), _exact_blend(p, tiles))


def test_normalisation_restated_as_torch_does_it():
    u = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(u).float().div(255).sub(0.5).div(0.5).numpy()       # ToTensor + Normalize((0.5,), (0.5,))
    assert np.array_equal(R.normalize_u8(u), want)
    x = np.array([1.0, -1.0, 0.1, 1.00390625, 1.01171875, 3.0e-40], dtype=np.float32)
    assert np.array_equal(R.bf16_round(x), torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16))


# ---- 4. the library, host side --------------------------------------------------------------------------------------
def test_header_declares_and_binding_table_binds_the_new_entry_points():
    L = import_module(PKG + "._lib")
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    m = re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src)
    assert int(m.group(1)) == L.ABI_VERSION >= 29 and lib.vg_abi_version() == L.ABI_VERSION
    cover = int(re.search(r"#define\s+VG_TILE_MAX_COVER\s+(\d+)", src).group(1))
    assert cover == L.VG_TILE_MAX_COVER == T.VG_TILE_MAX_COVER == 8
    for text in ("Tiled denoising", "Table safety", "never divide"):
        assert text in src


def test_c_abi_of_the_tile_entry_points_rejects_bad_arguments_on_host():
    L = import_module(PKG + "._lib")
    lib = L.load()
    b = ctypes.c_void_p(256)                                             # never dereferenced: validation comes first
    odd16 = ctypes.c_void_p(260)                                         # 4-byte but not 16-byte aligned
    odd4 = ctypes.c_void_p(258)

    # vg_tile_gather(src_u8, src_f32, N, C, H, W, S, ny, nx, oy, ox, t0, B, out, CP, dtype, stream)
    def g(u8=None, f=b, N=2, C=3, H=20, W=12, S=8, ny=4, nx=2, oy=b, ox=b, t0=0, B=16, out=b, CP=4, dt=0):
        return lib.vg_tile_gather(u8, f, N, C, H, W, S, ny, nx, oy, ox, t0, B, out, CP, dt, None)
    for kw in (dict(f=None), dict(u8=b), dict(oy=None), dict(ox=None), dict(out=None), dict(N=0), dict(C=0), dict(S=0),
               dict(H=7), dict(W=7), dict(ny=0), dict(nx=0), dict(ny=14), dict(nx=6), dict(B=0), dict(t0=-1), dict(B=17),
               dict(t0=1), dict(t0=16, B=1), dict(CP=0), dict(C=5, CP=4), dict(N=1 << 30)):
        assert g(**kw) == -1, kw
    assert g(dt=2) == -3 and g(dt=7) == -3
    assert g(CP=6) == -2 and g(CP=4, dt=1) == -2 and g(out=odd16) == -2 and g(f=odd4) == -2 and g(oy=odd4) == -2

    # vg_tile_blend(tiles, out, N, C, H, W, S, ny, nx, oy, ox, first_y, count_y, coef_y, wy, first_x, count_x, coef_x, wx, stream)
    o = ctypes.c_void_p(512)

    def bl(tiles=b, out=o, N=2, C=3, H=20, W=12, S=8, ny=4, nx=2, oy=b, ox=b, fy=b, cy=b, ky=b, wy=2, fx=b, cx=b, kx=b, wx=2):
        return lib.vg_tile_blend(tiles, out, N, C, H, W, S, ny, nx, oy, ox, fy, cy, ky, wy, fx, cx, kx, wx, None)
    for kw in (dict(tiles=None), dict(out=None), dict(oy=None), dict(ox=None), dict(fy=None), dict(cy=None), dict(ky=None),
               dict(fx=None), dict(cx=None), dict(kx=None), dict(out=b), dict(N=0), dict(C=0), dict(S=0), dict(H=7), dict(W=7),
               dict(ny=0), dict(nx=0), dict(ny=14), dict(nx=6), dict(wy=0), dict(wx=0), dict(wy=9), dict(wx=9), dict(N=1 << 30)):
        assert bl(**kw) == -1, kw
    assert bl(tiles=odd4) == -2 and bl(out=odd4) == -2 and bl(kx=odd4) == -2 and bl(cy=odd4) == -2


def test_package_exports_and_host_tensors_are_refused():
    import vaegan_amd as V
    for name in ("tiling", "TilePlan", "tile_plan", "denoise_tiled", "tiled_denoise_eval", "tiled_test_epoch"):
        assert name in V.__all__ and hasattr(V, name), name
    assert V.tile_plan is T.tile_plan and "denoise_tiled" in V.__doc__
    ops = import_module(PKG + ".ops")
    plan = T.tile_plan(20, 12, 8, 4, "tri")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tile_gather(torch.zeros(1, 3, 20, 12), plan, 0, 2, 4, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tile_blend(torch.zeros(8, 3, 8, 8), plan)
    e, g = V.Encoder([3, 64, 64], 16), V.Generator(nz=16, img_size=64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.denoise_tiled(e, g, torch.zeros(1, 3, 80, 80))
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.tiled_denoise_eval(e, g, torch.zeros(1, 3, 80, 80))
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.tiled_test_epoch(e, g, [(torch.zeros(1, 3, 80, 80), torch.zeros(1, 3, 80, 80))])
