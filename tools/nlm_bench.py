"""What the non-local-means baseline (ops.nlm_denoise, csrc/nlm.hip) costs and what it gains, measured
on the MI355X with the interleaved method of tools/ssimloss_bench.py:

  kernel   the launch REPLAYED from a graph of its own at 64 x 64, B = 128, C = 3 for (P, R) = (1, 5), (2, 7), (3, 10) and at
           one 2048 x 2048 image (P, R) = (2, 7), against (a) the kernel's own operation count per pixel-offset (``op_count``
           below: LDS reads / writes and vector instructions, counted from the source) over the LDS rates (4-byte reads at
           128, writes at 64 B per clock and CU) and the vector-ALU rate of the chip, and (b) a stock-torch route on the same
           GPU (reflect pad, then per offset: shifted difference, channel sum, avg_pool2d box sum, exp, two accumulations),
           whose result is also compared with the kernel's.
           ops.noise_sigma is timed on the same inputs against its byte count.
  epoch    paired_test_epoch over the generated JPEG set (the 45 images of tests/test_gpu_data.py) with the baseline off / on,
           in interleaved windows.
  psnr     the evidence behind NLMeans' default h_factor: PSNR of NLM against the noisy input on that set at
           noise_max_std = 0.2 (no rectangles), for h_factor 0.4 ... 1.0, with the loader's own sigma ("oracle") and the blind
           estimate.

A measurement path without the GPU fails; nothing is gated.

    python tools/nlm_bench.py [--steps 20] [--rounds 5] [--commit <text>]

The JSON records the commit it is told (else git's HEAD) and the sha256 of the sources it measured."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import torch.nn.functional as F
from importlib import import_module

import vaegan_amd as V
from ssimloss_bench import window_ms

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
data = import_module(PKG + ".data")
CUS, CLOCK = 256, 2.4e9
VALU_LANE_OPS = CUS * 4 * 32 * CLOCK            # one f32 vector instruction retires 32 lanes per SIMD and clock
LDS_READ_B32_BYTES = CUS * 128 * CLOCK          # ds_read_b32: 128 B per clock and CU
LDS_WRITE_B32_BYTES = CUS * 64 * CLOCK          # ds_write_b32: 64 B per clock and CU
HBM_PEAK = 8.0e12
TILE = 16


def op_count(C, P):
    """Per pixel-offset of one output pixel, counted from csrc/nlm.hip (16 x 16 tile, the map work shared by its 256 pixels):
    4-byte LDS reads, 4-byte LDS writes, vector instructions (the exponential weighs 2: its issue cost is twice an add's)."""
    if P == 0:
        return {"lds_reads": 2 * C + C, "lds_writes": 0, "valu": 2 * C + 4 + 2 + 1 + C}
    DW = TILE + 2 * P
    a, b = DW * DW / 256.0, DW * TILE / 256.0
    reads = a * 2 * C + b * (2 * P + 1) + (2 * P + 1) + C
    writes = a + b
    valu = a * 2 * C + b * 2 * P + 2 * P + 4 + 2 + 1 + C          # sub + fma; adds; adds; mul, sub, max, mul; exp; den; fma
    return {"lds_reads": reads, "lds_writes": writes, "valu": valu}


def graphed(fn):
    fn()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def torch_nlm(x, sigma, P, R, h):
    """The same definition from stock torch ops (f32): one pass of shifted tensors per offset."""
    B, C, H, W = x.shape
    HALO = P + R
    xp = F.pad(x, (HALO,) * 4, mode="reflect")
    A = xp[:, :, R:R + H + 2 * P, R:R + W + 2 * P]
    num, den = torch.zeros_like(x), torch.zeros(B, 1, H, W, device=x.device)
    for ty in range(-R, R + 1):
        for tx in range(-R, R + 1):
            Bm = xp[:, :, R + ty:R + ty + H + 2 * P, R + tx:R + tx + W + 2 * P]
            d2 = F.avg_pool2d(((A - Bm) ** 2).mean(1, keepdim=True), 2 * P + 1, 1) if P else ((A - Bm) ** 2).mean(1, keepdim=True)
            w = torch.exp(-torch.clamp(d2 - 2 * sigma * sigma, min=0) / (h * h))
            den += w
            num += w * xp[:, :, HALO + ty:HALO + ty + H, HALO + tx:HALO + tx + W]
    return num / den


def mode_kernel(a, dev):
    out = []
    gen = torch.Generator().manual_seed(3)
    for (B, C, H, W, P, R, torch_steps) in ((128, 3, 64, 64, 1, 5, 3), (128, 3, 64, 64, 2, 7, 3), (128, 3, 64, 64, 3, 10, 2),
                                            (1, 3, 2048, 2048, 2, 7, 1)):
        yy = torch.linspace(0, 9.0, H)[:, None]
        xx = torch.linspace(0, 7.0, W)[None, :]
        x = (0.7 * torch.sin(yy) * torch.cos(xx) + 0.1 * torch.randn(B, C, H, W, generator=gen)).clamp(-1, 1).to(dev)
        y = torch.empty_like(x)
        sig = torch.full((B,), 0.1, device=dev)
        rep = graphed(lambda: ops.nlm_denoise(x, sig, patch_radius=P, search_radius=R, h_factor=0.8, out=y))
        window_ms(rep, 3)
        steps = a.steps if H <= 64 else max(2, a.steps // 4)
        t = [window_ms(rep, steps) for _ in range(a.rounds)]
        med = statistics.median(t)
        oc = op_count(C, P)
        po = B * H * W * (2 * R + 1) ** 2                                    # pixel-offsets
        lds_ms = po * 4 * (oc["lds_reads"] / LDS_READ_B32_BYTES + oc["lds_writes"] / LDS_WRITE_B32_BYTES) * 1e3
        valu_ms = po * oc["valu"] / VALU_LANE_OPS * 1e3
        tt = [window_ms(lambda: torch_nlm(x, 0.1, P, R, 0.08), torch_steps) for _ in range(2)]
        ref = torch_nlm(x, 0.1, P, R, 0.08)
        ns = graphed(lambda: ops.noise_sigma(x, out=sig.clone()))
        window_ms(ns, 3)
        tn = statistics.median([window_ms(ns, a.steps) for _ in range(a.rounds)])
        row = {"shape": [B, C, H, W], "P": P, "R": R, "ms_per_replay": t, "median_ms": med, "spread_ms": max(t) - min(t),
               "pixel_offsets": po, "ns_per_pixel_offset": med * 1e6 / po, "op_count_per_pixel_offset": oc,
               "floor_ms_lds_rate": lds_ms, "floor_ms_valu_rate": valu_ms,
               "fraction_of_lds_rate": lds_ms / med, "fraction_of_valu_rate": valu_ms / med,
               "torch_route_ms": tt, "torch_over_kernel": min(tt) / med,
               "max_abs_diff_vs_torch_route": float((y - ref).abs().max()),
               "noise_sigma_ms": tn, "noise_sigma_fraction_of_hbm_peak": x.numel() * 4 / (tn * 1e-3) / HBM_PEAK}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def jpeg_set(folder):
    """The generated set of tests/test_gpu_data.py (fixture jpeg_folder), image for image."""
    from PIL import Image
    rng = np.random.default_rng(5)
    for i in range(45):
        yy, xx = np.mgrid[0:64, 0:64]
        base = np.stack([(yy * 4 + i * 3) % 256, (xx * 4 + i * 7) % 256, ((yy + xx) * 2 + i * 11) % 256], -1)
        img = np.clip(base + rng.integers(-20, 20, base.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img, "RGB").save(os.path.join(folder, f"{i:05d}.jpg"), quality=92)


def nets(dev):
    V.configure_seed(42)
    e, g = V.Encoder([3, 64, 64], 100), V.Generator(nz=100, img_size=64)
    g.apply(V.weights_init)
    return e.to(dev), g.to(dev)


def mode_epoch(a, dev, ds):
    e, g = nets(dev)
    loader = data.DeviceLoader(ds, torch.arange(0, 45), 15, shuffle=False, degrade=data.Degrade(0.2, rect=False))
    routes = {"baseline_off": lambda: V.paired_test_epoch(e, g, loader),
              "baseline_on": lambda: V.paired_test_epoch(e, g, loader, baseline="nlm")}
    for fn in routes.values():
        fn()
    import time
    windows = {k: [] for k in routes}
    for _ in range(a.rounds):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()                                                        # ends in the pass's host sync
            windows[name].append((time.perf_counter() - t0) / 3 * 1e3)
    med = {k: statistics.median(v) for k, v in windows.items()}
    out = {"images": 45, "batch": 15, "ms_per_epoch": windows, "median_ms": med,
           "baseline_cost_ms": med["baseline_on"] - med["baseline_off"]}
    print(json.dumps(out), flush=True)
    return out


def mode_psnr(a, dev, ds):
    e, g = nets(dev)
    loader = data.DeviceLoader(ds, torch.arange(0, 45), 15, shuffle=False, degrade=data.Degrade(0.2, rect=False))
    rows = []
    for hf in (0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0):
        row = {"h_factor": hf}
        for mode in ("oracle", "estimate"):
            torch.manual_seed(11)                                           # the same degradation draws for every row
            r = V.paired_test_epoch(e, g, loader, baseline=dict(h_factor=hf, sigma=mode))
            row["psnr_noisy"] = r["psnr_noisy"]
            row["psnr_nlm_" + mode] = r["psnr_nlm"]
            row["gain_db_" + mode] = r["psnr_nlm"] - r["psnr_noisy"]
            row["ssim_nlm_" + mode] = r["ssim_nlm"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    best = {m: max(rows, key=lambda r: r["psnr_nlm_" + m])["h_factor"] for m in ("oracle", "estimate")}
    return {"noise_max_std": 0.2, "patch_radius": 2, "search_radius": 7, "rows": rows, "best_h_factor": best}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlm_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nlm_bench needs the MI355X: there is nothing to time without it")
    dev = "cuda"
    torch.cuda.set_device(0)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip()
        except Exception:
            commit = "unknown (no git metadata where this ran)"
    # the measured code, identified by content whatever the checkout says: `sha256sum` of these files must give these digests
    measured = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()
                for rel in (PKG + "/csrc/nlm.hip", PKG + "/ops.py", PKG + "/baselines.py", PKG + "/denoise.py", "tools/nlm_bench.py")}
    out = {"device": torch.cuda.get_device_name(0), "commit": commit, "sha256_of_the_measured_sources": measured,
           "what": "non-local-means baseline: the launch replayed from a graph against its operation count and a stock-torch "
                   "route; paired_test_epoch with the baseline off / on; PSNR gain by h_factor; tools/nlm_bench.py",
           "peaks": {"valu_lane_ops_per_s": VALU_LANE_OPS, "lds_read_b32_bytes_per_s": LDS_READ_B32_BYTES, "lds_write_b32_bytes_per_s": LDS_WRITE_B32_BYTES, "hbm_bytes_per_s": HBM_PEAK}}
    out["kernel"] = mode_kernel(a, dev)
    with tempfile.TemporaryDirectory() as d:
        jpeg_set(d)
        ds = data.ResidentImages.from_folder(d, device=dev, workers=1)
    out["psnr"] = mode_psnr(a, dev, ds)
    out["epoch"] = mode_epoch(a, dev, ds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
