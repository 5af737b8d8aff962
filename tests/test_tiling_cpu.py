"""CPU: tiled denoising before any kernel runs.  (1) tiling.tile_plan against the restatement tests/_tiling_ref.py: origins,
cover ranges, coefficient rows, refused plans; (2) the f64 blend against torch's F.fold on uniform-stride geometries; (3) the
exact-input cases of the GPU tests really are exact (every product and partial sum representable, held against Fraction
arithmetic), so a bitwise comparison there has no blind spot; (3b) the slot-vectorised restatement equals the pixel loop bit
for bit, the large cases reach the launch geometry they are there for, and the bad-table cases stay inside their guards even
for a blend without checks; (4) the C ABI declarations, the ctypes table, host-side argument
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


# ---- 3b. the restatement that scales, the case table, the bad tables ----------------------------------------------------
def _loop_table_safe(p, tiles):
    """blend_f32's pixel loop with the header's "Table safety" words written out: the form the slot-vectorised one is held to."""
    S, per = p.S, p.ny * p.nx
    N, C = tiles.shape[0] // per, tiles.shape[1]
    wy, wx = p.coef_y.shape[1], p.coef_x.shape[1]
    r = tiles.reshape(N, p.ny, p.nx, C, S, S)
    out = np.zeros((N, C, p.H, p.W), dtype=np.float32)
    for y in range(p.H):
        for x in range(p.W):
            acc = np.zeros((N, C), dtype=np.float32)
            for jy in range(min(max(int(p.count_y[y]), 0), wy)):              # count clamped to [0, width]
                ky = int(p.first_y[y]) + jy
                if not 0 <= ky < p.ny or not 0 <= y - int(p.oy[ky]) < S:        # tile index / local coordinate: term dropped
                    continue
                inner = np.zeros((N, C), dtype=np.float32)
                for jx in range(min(max(int(p.count_x[x]), 0), wx)):
                    kx = int(p.first_x[x]) + jx
                    if not 0 <= kx < p.nx or not 0 <= x - int(p.ox[kx]) < S:
                        continue
                    inner = inner + p.coef_x[x, jx] * r[:, ky, kx, :, y - p.oy[ky], x - p.ox[kx]]
                acc = acc + p.coef_y[y, jy] * inner
            out[:, :, y, x] = acc
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("H,W,S,stride,window", EXACT_CASES + [
    (13, 37, 8, 3, "hann"), (37, 13, 8, 3, "hann"), (12, 24, 8, 3, "hann"),   # the cover count differs from coordinate to coordinate
    (16, 15, 8, 1, "hann"), (37, 29, 8, 3, "tri")])
def test_slot_vectorised_blend_equals_the_pixel_loop_bit_for_bit(H, W, S, stride, window):
    p = R.plan(H, W, S, stride, window)
    if (H, W) == (13, 37):
        assert sorted(set(p.count_x.tolist())) == [1, 2, 3] and sorted(set(p.count_y.tolist())) == [1, 2, 3]
    tiles = R.uniform_tiles(p, 2, 3, seed=H * W)
    want = R.blend_f32(p, tiles)
    assert np.array_equal(_bits(R.blend_f32_fast(p, tiles)), _bits(want))
    assert np.array_equal(_bits(R.blend_f32_table_safe(p, tiles)), _bits(want))   # a sound table needs none of the clauses
    assert np.array_equal(_bits(_loop_table_safe(p, tiles)), _bits(want))


def test_slot_vectorised_blend_with_hand_made_tables_wider_than_the_cover():
    p = R.dyadic_tables(R.plan(23, 9, 8, 2, "tri"), 5)
    assert int(p.count_x.max()) == 2 and int(p.count_y.max()) == 5 and p.coef_x.shape[1] == 5
    tiles = R.uniform_tiles(p, 2, 1, seed=3)
    assert np.array_equal(_bits(R.blend_f32_fast(p, tiles)), _bits(R.blend_f32(p, tiles)))


@pytest.mark.parametrize("case", list(R.BLEND_CASES), ids=lambda c: "x".join(map(str, c)))
def test_blend_cases_reach_the_paths_they_are_there_for(case):
    H, W, S, stride = case
    p = R.plan(H, W, S, stride)
    assert R.same_plan(p, T.tile_plan(H, W, S, stride))
    got, want = R.case_properties(p), R.BLEND_CASES[case]
    assert got == want, (got, want)
    assert got["blend_grid"] == (math.ceil(H / 32), math.ceil(math.ceil(W / 4) / 64)) and got["gather_grid"][1] == math.ceil(S / 64)
    if got["groups"] is not None:
        assert sum(got["groups"]) == math.ceil(W / 4) and got["cover"][1] <= 4


def test_the_case_table_as_a_whole_reaches_every_row_of_the_gap_list():
    props = list(R.BLEND_CASES.values())
    assert max(q["blend_grid"][1] for q in props) == 3 and max(q["blend_grid"][0] for q in props) == 9
    assert {q["cover"][1] for q in props} >= {2, 3, 4, 8}
    assert any(q["cover"] == (R.MAX_COVER, R.MAX_COVER) and not q["vector_store"] for q in props)
    assert any(q["groups"] is None and q["vector_store"] for q in props)            # wide x table with the 16-byte store
    for zgrid in (1, 2, 4):                                                          # S = 64, 128, 256
        assert any(q["gather_grid"][1] == zgrid and q["groups"] and min(q["groups"]) > 0 for q in props)
    # a second workgroup along x in each store form and in each read path
    assert any(q["blend_grid"][1] > 1 and q["vector_store"] and q["groups"][1] == 0 for q in props)
    assert any(q["blend_grid"][1] > 1 and not q["vector_store"] and q["groups"][0] == 0 for q in props)
    assert any(q["blend_grid"][1] > 1 and q["cover"][1] == 4 for q in props)
    assert R.case_properties(R.plan(12, 24, 8, 1))["cover"] == (5, 8)              # a real plan with 5 to 8 covering tiles


@pytest.mark.parametrize("case", list(R.GATHER_CASES), ids=lambda c: "x".join(map(str, c)))
def test_gather_cases_have_odd_flush_origins_and_the_engines_grid(case):
    H, W, S = case
    p, want = R.plan(H, W, S), R.GATHER_CASES[case]
    assert p.oy.tolist() == want["oy"] and p.ox.tolist() == want["ox"] and p.oy[-1] % 2 == 1 and p.ox[-1] % 2 == 1
    assert R.case_properties(p)["gather_grid"] == want["gather_grid"] == (math.ceil(S / 4), math.ceil(S / 64))
    assert 2 * p.ny * p.nx <= 12 and (S < 256 or 2 * p.ny * p.nx <= 8)


@pytest.mark.parametrize("path", ["reg", "wide"])
def test_bad_table_entries_and_their_restatement(path):
    """Every edit really holds the bad entry it is named for, is off by one only, changes the result where it should, and the
    slot-vectorised table-safe restatement equals the pixel loop that spells the header's words out."""
    p = R.safety_plan(path)
    assert (p.coef_x.shape[1] <= 4) == (path == "reg")
    if path == "reg":
        assert R.group_kinds(p) == (p.W // 4, 0)
    C = 2
    tiles = R.uniform_tiles(p, 2, C, seed=17)
    sound = R.blend_f32(p, tiles)
    edits = R.blend_table_edits(p, C)
    assert tuple(edits) == R.BLEND_EDIT_NAMES
    for name, (q, reach) in edits.items():
        want = _loop_table_safe(q, tiles)
        assert np.array_equal(_bits(R.blend_f32_table_safe(q, tiles)), _bits(want)), name
        assert np.isfinite(want).all() and not np.array_equal(_bits(want), _bits(sound)), name
        assert 0 <= reach <= p.nx * C * p.S * p.S
        for k in ("oy", "ox", "first_y", "first_x"):                        # off by one: no entry further than 1 from a sound one
            assert np.abs(getattr(q, k).astype(np.int64) - getattr(p, k)).max() <= 1, (name, k)
        assert (q.first_y + q.count_y).max() <= p.ny + 1 and (q.first_x + q.count_x).max() <= p.nx + 1
        assert q.count_y.max() <= q.coef_y.shape[1] + 1 and q.count_x.max() <= q.coef_x.shape[1] + 1 and min(q.count_y.min(), q.count_x.min()) >= -1
    q = edits["count=-1"][0]
    want = R.blend_f32_table_safe(q, tiles)
    assert not want[:, :, 2, :].any() and not want[:, :, :, 4:8].any()      # clamped to 0 terms: the element is 0
    q = edits["first_x=-1"][0]
    assert np.all(q.first_x[:4] == -1) and np.all(q.coef_x[:4] > 0)


def _blend_without_any_check(q, tiles, guard):
    """What a blend that formed its addresses WITHOUT the promised checks would do with q's tables, on the host: the tile
    buffer between `guard` NaN floats, an origin read one outside its table giving the sentinel the GPU test puts there (0
    before, L - S behind), a coefficient read behind its table NaN.  -> (result, furthest offset before the buffer, behind it)."""
    S, SS, per = q.S, q.S * q.S, q.ny * q.nx
    N, C = tiles.shape[0] // per, tiles.shape[1]
    wy, wx = q.coef_y.shape[1], q.coef_x.shape[1]
    flat = np.concatenate([np.full(guard, np.nan, np.float32), tiles.ravel(), np.full(guard, np.nan, np.float32)])
    ky_flat, kx_flat = (np.concatenate([k.ravel(), np.full(16, np.nan, np.float32)]) for k in (q.coef_y, q.coef_x))
    plane = (np.arange(N)[:, None] * per * C + np.arange(C)[None, :]) * SS                # [N, C]: tile 0 of image n, channel c

    def origin(o, k, L):
        return 0 if k < 0 else L - S if k >= o.size else int(o[k])
    out = np.zeros((N, C, q.H, q.W), dtype=np.float32)
    before = behind = 0
    with np.errstate(invalid="ignore"):
        for y in range(q.H):
            for x in range(q.W):
                acc = np.zeros((N, C), dtype=np.float32)
                for jy in range(max(int(q.count_y[y]), 0)):
                    ky = int(q.first_y[y]) + jy
                    assert -1 <= ky <= q.ny and jy <= wy
                    inner = np.zeros((N, C), dtype=np.float32)
                    for jx in range(max(int(q.count_x[x]), 0)):
                        kx = int(q.first_x[x]) + jx
                        assert -1 <= kx <= q.nx and jx <= wx
                        addr = plane + (ky * q.nx + kx) * C * SS + (y - origin(q.oy, ky, q.H)) * S + (x - origin(q.ox, kx, q.W))
                        before, behind = max(before, -int(addr.min())), max(behind, int(addr.max()) - (tiles.size - 1))
                        assert before <= guard and behind <= guard, "the guards of the GPU test would not hold this entry"
                        inner = inner + kx_flat[x * wx + jx] * flat[guard + addr]
                    acc = acc + ky_flat[y * wy + jy] * inner
                out[:, :, y, x] = acc
    return out, before, behind


@pytest.mark.parametrize("path", ["reg", "wide"])
def test_a_blend_without_the_checks_stays_inside_the_guards_and_fails_the_comparison(path):
    """The design of the GPU table-safety test, computed instead of argued: for every edit, the addresses an unchecked blend
    forms leave the tile buffer by exactly the edit's stated reach, which the guards cover, and its result differs from the
    promised one (it read a NaN guard, a neighbouring tile or a coefficient of another slot), so the GPU comparison would fail
    without an out-of-range access.  count = -1 needs no check to be safe: the loop simply does not run."""
    p = R.safety_plan(path)
    N, C = 2, 2
    guard = (p.nx + 1) * C * p.S * p.S                                       # as tests/test_gpu_tiling.py
    tiles = R.uniform_tiles(p, N, C, seed=41)
    sound, before, behind = _blend_without_any_check(p, tiles, guard)
    assert (before, behind) == (0, 0) and np.array_equal(_bits(sound), _bits(R.blend_f32(p, tiles)))
    for name, (q, reach) in R.blend_table_edits(p, C).items():
        got, before, behind = _blend_without_any_check(q, tiles, guard)
        assert max(before, behind) == reach <= guard, (name, before, behind, reach)
        assert min(before, behind) == 0, name
        same = np.array_equal(_bits(got), _bits(R.blend_f32_table_safe(q, tiles)))
        assert same == (name == "count=-1"), name


def test_gather_origin_edits_and_their_restatement():
    p = R.plan(13, 11, 8, 3)
    img = np.random.default_rng(2).uniform(-1, 1, size=(2, 3, 13, 11)).astype(np.float32)
    sound = R.gather(p, 0, 12, 4, images_f32=img)
    assert np.array_equal(R.gather_table_safe(p, 0, 12, 4, images_f32=img), sound)
    edits = R.gather_origin_edits(p)
    assert tuple(edits) == R.GATHER_EDIT_NAMES
    for name, (q, reach) in edits.items():
        got = R.gather_table_safe(q, 0, 12, 4, images_f32=img)
        zero = np.array([not got[b].any() for b in range(12)])
        ky, kx = np.divmod(np.arange(12) % 6, p.nx)
        bad = {"oy=-1": ky == 0, "oy=H-S+1": ky == p.ny - 1, "ox=-1": kx == 0, "ox=W-S+1": kx == p.nx - 1}[name]
        assert np.array_equal(zero, bad), name
        assert np.array_equal(got[~bad], sound[~bad]) and reach in (1, p.W)


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
