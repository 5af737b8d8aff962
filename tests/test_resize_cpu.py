"""CPU: the Resize contract of include/vaegan_hip.h ("Resize") restated in plain numpy FROM THE HEADER TEXT (nothing is
imported from data.py for it) and held against Pillow's own output recorded in tests/golden/resize_pil.npz
(tools/gen_golden_resize.py, Pillow 12.2.0) byte for byte -- this pins the contract to PIL before any kernel runs.  Plus
the host table builder, the geometry rule, the C ABI declarations, the ctypes table, host-side validation and exports.

Where a bounds table that reaches outside the input is caught: in vg_resize_u8 itself, on the host, before the launch --
the call takes the bounds in host memory next to the device tables and checks every (xmin, n) against the input size
(test_c_abi_of_the_resize_entry_points_rejects_bad_arguments_on_host)."""
import ctypes
import hashlib
import json
import math
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vg_resize_u8", "vg_resize_u8_lds_bytes", "vg_resize_u8_band")
PB = 22


# ---- the contract, one double / integer operation per line, written from the header ---------------------------------
def coeffs_contract(in_size: int, out_size: int):
    scale = float(in_size) / float(out_size)
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)                              # int() truncates toward zero
        xmin = max(xmin, 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(n):
            wx = 1.0 - abs((x + xmin - center + 0.5) * ss)
            wx = max(0.0, wx)
            w.append(wx)
            ww = ww + wx                                                # left to right
        for x in range(n):
            p = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(-0.5 + p * 2.0 ** PB) if p < 0 else int(0.5 + p * 2.0 ** PB)
        bounds[xx] = (xmin, n)
    return k, bounds


def pass_contract(a: np.ndarray, k: np.ndarray, bounds: np.ndarray, axis: int) -> np.ndarray:
    """One pass along `axis` of u8 [H][W][C] with an int32 accumulator."""
    a = np.moveaxis(a, axis, 0)
    out = np.empty((k.shape[0],) + a.shape[1:], np.uint8)
    for o in range(k.shape[0]):
        xmin, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = np.full(a.shape[1:], 1 << (PB - 1), np.int64)
        for x in range(n):
            acc = acc + a[xmin + x].astype(np.int64) * int(k[o, x])
        assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31            # the int32 accumulator of the contract holds it
        out[o] = np.clip(acc >> PB, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def geometry_contract(H: int, W: int, image_size):
    if isinstance(image_size, int):
        short, long = (W, H) if W <= H else (H, W)
        new_long = int(image_size * long / short)
        Hr, Wr = (new_long, image_size) if W <= H else (image_size, new_long)
        ch = cw = image_size
    else:
        ch, cw = image_size
        Hr, Wr = ch, cw
    assert ch <= Hr and cw <= Wr
    top, left = int(round((Hr - ch) / 2.0)), int(round((Wr - cw) / 2.0))
    return Hr, Wr, top, left, ch, cw


def resize_contract(a: np.ndarray, image_size) -> np.ndarray:
    H, W, _ = a.shape
    Hr, Wr, top, left, ch, cw = geometry_contract(H, W, image_size)
    if Wr != W:                                                         # horizontal first; an unchanged size is skipped
        a = pass_contract(a, *coeffs_contract(W, Wr), axis=1)
    if Hr != H:                                                         # vertical on the u8 result
        a = pass_contract(a, *coeffs_contract(H, Hr), axis=0)
    return a[top:top + ch, left:left + cw].copy()


def formula_image(H, W, C, salt):
    """Full-size fixture inputs: (37 y + 101 x + 59 c + ((x y) >> 3) + 29 ((x ^ y ^ salt) & 7)) & 255."""
    y = np.arange(H, dtype=np.int64)[:, None, None]
    x = np.arange(W, dtype=np.int64)[None, :, None]
    c = np.arange(C, dtype=np.int64)[None, None, :]
    return ((37 * y + 101 * x + 59 * c + ((x * y) >> 3) + 29 * ((x ^ y ^ salt) & 7)) & 255).astype(np.uint8)


def load_cases(golden_dir):
    """-> list of (case dict, input u8 [H][W][C], check(out u8 [ch][cw][C]) -> None)."""
    fx = np.load(os.path.join(golden_dir, "resize_pil.npz"))
    cases = []
    for c in json.loads(str(fx["cases"])):
        c["image_size"] = c["image_size"] if isinstance(c["image_size"], int) else tuple(c["image_size"])
        if c["input"] == "random":
            a = fx[f"in_{c['H']}x{c['W']}x{c['C']}"]
        else:
            a = formula_image(c["H"], c["W"], c["C"], c["salt"])
        assert a.shape == (c["H"], c["W"], c["C"]) and a.dtype == np.uint8

        def check(out, c=c):
            assert out.dtype == np.uint8 and list(out.shape) == c["out_shape"], c["name"]
            if "sha256" in c:
                assert np.array_equal(out[:2], fx["head_" + c["name"]]), c["name"]
                assert hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest() == c["sha256"], c["name"]
            else:
                assert np.array_equal(out, fx["out_" + c["name"]]), c["name"]

        cases.append((c, a, check))
    return cases


ISSUE_GEOMETRIES = [((218, 178), (78, 64)), ((218, 178), (156, 128)), ((256, 256), (64, 64)), ((256, 256), (128, 128)),
                    ((256, 256), (32, 32)), ((256, 256), (16, 16)), ((64, 64), (100, 100)), ((50, 70), (64, 64)),
                    ((1024, 1024), (256, 256)), ((218, 178), (218, 64)), ((37, 53), (64, 16))]


def test_fixture_holds_the_cases_the_issue_names(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "resize_pil.npz")) <= 156 * 1024
    cases = [c for c, _, _ in load_cases(golden_dir)]
    have = {((c["H"], c["W"]), c["image_size"]) for c in cases if c["C"] == 3}
    for g in ISSUE_GEOMETRIES:
        assert g in have, g
    by = {c["name"]: c for c in cases}
    assert by["celeba_int64"]["geometry"] == [78, 64, 7, 0, 64, 64]             # crop rows 7 .. 70
    assert by["celeba_int128"]["geometry"] == [156, 128, 14, 0, 128, 128]       # crop rows 14 .. 141
    assert {c["C"] for c in cases} == {1, 3, 4}
    assert any((c["H"], c["W"]) == tuple(c["out_shape"][:2]) for c in cases)    # an identity size
    assert any("sha256" in c for c in cases) and any("sha256" not in c for c in cases)


def test_contract_reproduces_pillow_bytewise_on_every_recorded_case(golden_dir):
    for c, a, check in load_cases(golden_dir):
        assert list(geometry_contract(c["H"], c["W"], c["image_size"])) == c["geometry"], c["name"]
        check(resize_contract(a, c["image_size"]))


def test_resample_coeffs_equals_the_restated_tables():
    data = import_module(PKG + ".data")
    sizes = [(178, 64), (218, 78), (218, 156), (256, 64), (256, 16), (1024, 256), (64, 100), (64, 128), (50, 64), (53, 16),
             (37, 64), (70, 44), (7, 1), (1, 5), (300, 299), (299, 300), (5, 5)]
    for i, o in sizes:
        k, b = data.resample_coeffs(i, o)
        kc, bc = coeffs_contract(i, o)
        assert k.dtype == b.dtype == np.int32 and k.shape == kc.shape and b.shape == (o, 2)
        assert np.array_equal(k, kc) and np.array_equal(b, bc), (i, o)
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= i).all() and (b[:, 1] >= 1).all()
        assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()   # what the launcher relies on
        assert (np.abs(k.sum(1) - (1 << PB)) <= k.shape[1]).all()


def test_resize_geometry_is_the_restated_rule():
    data = import_module(PKG + ".data")
    assert data.resize_geometry(218, 178, 64) == (78, 64, 7, 0, 64, 64)
    assert data.resize_geometry(218, 178, 128) == (156, 128, 14, 0, 128, 128)
    assert data.resize_geometry(178, 218, 64) == (64, 78, 0, 7, 64, 64)
    assert data.resize_geometry(256, 256, (64, 32)) == (64, 32, 0, 0, 64, 32)
    assert data.resize_geometry(50, 55, 50) == (50, 55, 0, 2, 50, 50)           # (55 - 50) / 2 = 2.5 -> 2, ties to even
    assert data.resize_geometry(50, 57, 50) == (50, 57, 0, 4, 50, 50)           # 3.5 -> 4
    rng = np.random.default_rng(7)
    for _ in range(300):
        H, W = (int(v) for v in rng.integers(8, 400, 2))
        size = int(rng.integers(4, 300)) if rng.random() < 0.6 else tuple(int(v) for v in rng.integers(4, 300, 2))
        assert data.resize_geometry(H, W, size) == geometry_contract(H, W, size)


def test_resize_geometry_equals_resize_center_crop_on_a_pil_image():
    Image = pytest.importorskip("PIL.Image")                            # only this live comparison may skip
    data = import_module(PKG + ".data")
    rng = np.random.default_rng(11)
    draws = [(50, 55, 50), (50, 57, 50), (57, 50, 50), (218, 178, 64), (37, 53, 37)]     # round ties, odd sizes
    while len(draws) < 200:
        H, W = (int(v) for v in rng.integers(5, 90, 2))
        size = int(rng.integers(3, 100)) if rng.random() < 0.6 else tuple(int(v) for v in rng.integers(3, 100, 2))
        draws.append((H, W, size))
    for H, W, size in draws:
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        Hr, Wr, top, left, ch, cw = data.resize_geometry(H, W, size)
        got = np.asarray(data._resize_center_crop(Image.fromarray(a), size))
        assert got.shape == (ch, cw, 3), (H, W, size)
        img = Image.fromarray(a)
        if (Wr, Hr) != (W, H):
            img = img.resize((Wr, Hr), Image.BILINEAR)
        want = np.asarray(img)[top:top + ch, left:left + cw]
        assert np.array_equal(got, want), (H, W, size)
        assert np.array_equal(resize_contract(a, size), want), (H, W, size)              # and the contract, live


def test_header_declares_and_binding_table_binds_the_new_entry_points():
    L = import_module(PKG + "._lib")
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", src), name
        assert name in L.SIGNATURES, name
    m = re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src)
    assert int(m.group(1)) == L.ABI_VERSION >= 13
    for text in ("Resize", "PB = 22", "summed left to right", "horizontal pass first", "ties to even"):
        assert text in src, text
    assert L.load().vg_abi_version() == L.ABI_VERSION


def _tables(in_size, out_size, lo=0, n=None):
    k, b = coeffs_contract(in_size, out_size)
    n = out_size if n is None else n
    return np.ascontiguousarray(b[lo:lo + n]), k.shape[1]


def test_c_abi_of_the_resize_entry_points_rejects_bad_arguments_on_host():
    L = import_module(PKG + "._lib")
    lib = L.load()
    buf = ctypes.c_void_p(256)                                          # never dereferenced: validation comes first
    bh, ksh = _tables(178, 64)
    bv, ksv = _tables(218, 78, 7, 64)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)                       # noqa: E731

    def call(src=buf, N=10, Hin=218, Win=178, C=3, idx=None, B=4, kh=buf, bhd=buf, bhh=hp(bh), ksh=ksh, kv=buf, bvd=buf,
             bvh=hp(bv), ksv=ksv, top=7, left=0, dst=buf, ch=64, cw=64, band=0):
        return lib.vg_resize_u8(src, N, Hin, Win, C, idx, B, kh, bhd, bhh, ksh, kv, bvd, bvh, ksv, top, left, dst, ch, cw,
                                band, None)

    def lds(Hin=218, Win=178, C=3, bhh=hp(bh), ksh=ksh, bvh=hp(bv), ksv=ksv, top=7, left=0, ch=64, cw=64, B=4, band=0):
        return lib.vg_resize_u8_lds_bytes(Hin, Win, C, bhh, ksh, bvh, ksv, top, left, ch, cw, B, band)

    assert 0 < lds() <= 64 * 1024
    assert call(src=None) == -1 and call(dst=None) == -1
    assert call(C=5) == -1 and call(C=0) == -1 and lds(C=5) == -1
    assert call(B=0) == -1 and call(N=0) == -1 and call(B=11) == -1                 # idx NULL means images 0 .. B-1 of N
    assert call(kh=None) == -1 and call(bvh=None) == -1                             # a pass has all its tables or none
    # crop larger than the (un)resized image: a skipped pass whose window leaves the input
    assert call(kv=None, bvd=None, bvh=None, top=0, ch=219) == -1
    assert call(kh=None, bhd=None, bhh=None, left=100, cw=100) == -1
    assert lds(bvh=None, top=200, ch=64) == -1
    # bounds that reach outside the input, caught on the host before the launch
    bad = bv.copy()
    bad[-1, 1] += 40                                                    # last window ends beyond row 217
    assert call(bvh=hp(bad)) == -1 and lds(bvh=hp(bad)) == -1
    bad = bh.copy()
    bad[0, 0] = -1
    assert call(bhh=hp(bad)) == -1
    bad = bh.copy()
    bad[5, 1] = ksh + 1                                                 # more taps than the table holds
    assert call(bhh=hp(bad)) == -1
    assert call(Win=100) == -1                                          # the table of a 178-wide input on a 100-wide one
    # unsupported geometry: the LDS image of one output row does not fit
    wide, ksw = _tables(16000, 32000)
    assert lds(Hin=8, Win=16000, C=4, bhh=hp(wide), ksh=ksw, bvh=None, ksv=0, top=0, ch=8, cw=32000) == -1
    assert call(Hin=8, Win=16000, C=4, bhh=hp(wide), ksh=ksw, kv=None, bvd=None, bvh=None, ksv=0, top=0, ch=8, cw=32000) == -1
    assert lds(band=64) > 0 and lds(band=100000) > 0 and lds(band=-1) == -1
    big, ksb = _tables(1024, 256)
    assert lds(Hin=1024, Win=1024, bhh=hp(big), ksh=ksb, bvh=hp(big), ksv=ksb, top=0, ch=256, cw=256, band=256) == -1
    # misaligned table pointer
    assert call(kh=ctypes.c_void_p(260)) == -2 and call(bvd=ctypes.c_void_p(264)) == -2
    assert call(src=ctypes.c_void_p(258)) == -2


def test_every_size_family_member_is_served():
    ops = import_module(PKG + ".ops")
    data = import_module(PKG + ".data")
    for H, W in ((218, 178), (256, 256), (1024, 1024)):
        for S in (16, 32, 64, 128, 256):
            for size in (S, (S, S)):
                for C in (1, 3, 4):
                    n = ops.resize_u8_lds_bytes(H, W, C, data.resize_geometry(H, W, size))
                    assert 0 < n <= 64 * 1024, (H, W, size, C, n)
    for H, W, C in ((218, 178, 3), (256, 256, 4), (1024, 1024, 4)):                  # enlargements up to 2x
        assert ops.resize_u8_lds_bytes(H, W, C, data.resize_geometry(H, W, (2 * H, 2 * W))) > 0
    assert ops.resize_u8_lds_bytes(8, 16000, 4, (8, 32000, 0, 0, 8, 32000)) == -1
    tr = ops.resize_u8_traffic(218, 178, 3, data.resize_geometry(218, 178, (78, 64)), B=4096)
    assert tr["algorithmic"] == 218 * 178 * 3 + 78 * 64 * 3 and tr["actual"] >= tr["algorithmic"] and 1 <= tr["band"] <= 78
    crop = ops.resize_u8_traffic(218, 178, 3, data.resize_geometry(218, 178, 64), B=4096)
    assert crop["rows_read"] < 218 and crop["cols_read"] == 178                      # rows outside the crop window are not read
    one = ops.resize_u8_traffic(218, 178, 3, data.resize_geometry(218, 178, 64), band=64)
    assert one["band"] == 64 and one["actual"] == one["algorithmic"]                 # one band: nothing is read twice
    # neither form of image_size can ask for a crop beyond the resized image; a hand-made geometry can, and is refused
    with pytest.raises(RuntimeError, match="padding"):
        ops.resize_u8_lds_bytes(218, 178, 3, (78, 64, 0, 0, 80, 64))


def test_package_exports_and_host_tensors_are_refused():
    import vaegan_amd as V
    for name in ("ResidentImages", "resample_coeffs", "resize_geometry"):
        assert hasattr(V, name) and name in V.__all__, name
    assert V.ResidentImages is V.data.ResidentImages and V.resample_coeffs is V.data.resample_coeffs
    ops = import_module(PKG + ".ops")
    x = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resize_u8(x, (8, 8, 0, 0, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.ResidentImages(x, device="cpu")
    ds = V.ResidentImages.__new__(V.ResidentImages)                     # a set that somehow holds a host tensor
    ds.images = x
    with pytest.raises(RuntimeError, match="no CPU path"):
        ds.resized(8)
    with pytest.raises(ValueError, match="resize_on"):
        V.data.decode_folder("/nonexistent", resize_on="gpu")
    with pytest.raises(ValueError, match="resize_on"):
        V.data.get_dataset_loaders("/nonexistent", resize_on="gpu")
