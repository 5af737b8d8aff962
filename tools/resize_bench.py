"""Resize + CenterCrop of a resident u8 set on the device (ops.resize_u8) against the host route on the same arrays
(data._resize_center_crop with PIL over a 16-process pool) and against a second JPEG decode pass, which is what a size
change of a resident set cost before.

Device leg: N resident images, one launch over all of them, device events around `reps` back-to-back launches after a
warm-up, geometries interleaved round by round; the figure is the median over the rounds.  Beside it the algorithmic byte
count B * (rows_read * cols_read * C + ch * cw * C) over the time as a fraction of the 8 TB/s HBM peak and of the 6.3 TB/s
a device copy reaches, and the bytes the launch really reads (adjacent bands re-read about 2 * support input
rows).  Host legs: wall clock of a 16-process pool over `--host-n` of the same images (raw arrays; and the same images as
in-memory JPEGs, decoded and resized), scaled to N.  Reported, no threshold.

    python tools/resize_bench.py [--n 4096] [--reps 20] [--rounds 5] [--host-n 256] [--out profiles/resize_bench.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from multiprocessing import get_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch
from importlib import import_module

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
HBM_PEAK, COPY_RATE = 8.0e12, 6.3e12                # bytes / s
GEOMS = [("celeba 218x178 -> (64, 64)", 218, 178, (64, 64)), ("celeba 218x178 -> 64", 218, 178, 64),
         ("hq 256x256 -> 64", 256, 256, 64), ("hq 256x256 -> 128", 256, 256, 128), ("hq 1024x1024 -> 256", 1024, 1024, 256)]


def _host_resize(args):
    from PIL import Image
    data = import_module(PKG + ".data")
    a, size = args
    return np.asarray(data._resize_center_crop(Image.fromarray(a), size)).shape


def _host_decode_resize(args):
    from PIL import Image
    data = import_module(PKG + ".data")
    blob, size = args
    img = Image.open(io.BytesIO(blob)).convert("RGB")
    return np.asarray(data._resize_center_crop(img, size)).shape


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps         # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.json"))
    a = ap.parse_args()
    ops = import_module(PKG + ".ops")
    data = import_module(PKG + ".data")
    dev, C, N = "cuda", 3, a.n
    hn = min(a.host_n, N)
    try:
        import PIL
        from PIL import Image
        pil = PIL.__version__
    except ImportError:
        Image, pil = None, None
    # host legs first: the pool's processes are started before this process opens the GPU and never open it themselves
    host_arrays, host_rows = {}, {}
    rng = np.random.default_rng(4096)
    with get_context("spawn").Pool(16) as pool:
        for name, H, W, size in GEOMS:
            if (H, W) not in host_arrays:
                host_arrays[(H, W)] = rng.integers(0, 256, (hn, H, W, C), dtype=np.uint8)
            if Image is None:
                continue
            arrs = list(host_arrays[(H, W)])
            blobs = []
            for arr in arrs:
                buf = io.BytesIO()
                Image.fromarray(arr).save(buf, format="JPEG", quality=90)
                blobs.append(buf.getvalue())
            pool.map(_host_resize, [(arrs[0], size)] * 32)                       # start the workers
            t0 = time.perf_counter()
            pool.map(_host_resize, [(x, size) for x in arrs], chunksize=4)
            t1 = time.perf_counter()
            pool.map(_host_decode_resize, [(b, size) for b in blobs], chunksize=4)
            t2 = time.perf_counter()
            host_rows[name] = {"host_images": hn, "host_pool16_resize_s_per_set": round((t1 - t0) / hn * N, 3),
                               "host_pool16_decode_resize_s_per_set": round((t2 - t1) / hn * N, 3)}
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench needs the MI355X; a CPU run cannot give a time")
    legs = []
    for name, H, W, size in GEOMS:
        gen = torch.Generator(device=dev).manual_seed(H + W)
        src = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, device=dev, generator=gen)
        src[:hn] = torch.from_numpy(host_arrays[(H, W)]).to(dev)                # the images the host legs ran on
        geom = data.resize_geometry(H, W, size)
        out = torch.empty(N, geom[4], geom[5], C, dtype=torch.uint8, device=dev)
        legs.append((name, H, W, size, geom, src, out))
    fns = [lambda s=src, g=geom, o=out: ops.resize_u8(s, g, out=o) for _, _, _, _, geom, src, out in legs]
    for fn in fns:                                  # warm-up: code objects, coefficient tables
        timed(fn, 3)
    times = [[] for _ in legs]
    for _ in range(a.rounds):
        for i, fn in enumerate(fns):
            times[i].append(timed(fn, a.reps))
    rows = []
    for (name, H, W, size, geom, src, out), t in zip(legs, times):
        us = statistics.median(t)
        tr = ops.resize_u8_traffic(H, W, C, geom, B=N)
        row = {"geometry": name, "N": N, "band": tr["band"], "lds_bytes": tr["lds_bytes"],
               "set_ms": round(us / 1e3, 3), "ns_per_image": round(us * 1e3 / N, 1),
               "set_ms_min_max": [round(min(t) / 1e3, 3), round(max(t) / 1e3, 3)],
               "algorithmic_bytes_per_image": tr["algorithmic"], "actual_bytes_per_image": tr["actual"],
               "algorithmic_GBps": round(tr["algorithmic"] * N / us / 1e3, 1),
               "hbm_peak_fraction": round(tr["algorithmic"] * N / (us * 1e-6) / HBM_PEAK, 3),
               "copy_rate_fraction": round(tr["algorithmic"] * N / (us * 1e-6) / COPY_RATE, 3),
               "actual_GBps": round(tr["actual"] * N / us / 1e3, 1)}
        if name in host_rows:
            row.update(host_rows[name])
            row["device_over_host_resize"] = round(us * 1e-6 / host_rows[name]["host_pool16_resize_s_per_set"], 6)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"what": "one launch over N resident images, median of %d interleaved rounds of %d eager launches, device events; "
                   "host legs: 16-process pool, wall clock over host_images images scaled to N (random-noise images: "
                   "the JPEG leg decodes the least compressible content)" % (a.rounds, a.reps),
           "device": torch.cuda.get_device_name(0), "pillow": pil, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
