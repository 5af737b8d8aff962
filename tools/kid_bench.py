"""Kernel Inception Distance: the device route (metrics.kernel_distance -> ops.kid_scores -> vg_kid_scores, two launches)
against what a user does today, measured in the same process on the same box:

  (a) the host route: device -> host copy of both feature matrices, then per subset the numpy f64 Gram matrices, the
      power and the sums (what tests/_kid_ref.py states);
  (b) stock torch on the same GPU, in f32 and in f64: per subset index_select, three ``mm``, the affine step, the power
      and the sums; mean and std over the stacked scores.

N = 3 000 rows per side (the reference's 10 % validation split of CelebA-HQ), D in {100, 200, 2048}, S = 100 subsets of
m = 1000 rows, degree 3, gamma = 1 / D, coef = 1; real = N(0, I), fake = 0.25 + 0.9 N(0, I); the subset tables are
metrics.kid_subsets' and are uploaded once, outside the timed region, for every route.  Device legs: one device-event pair
around each call, `--reps` (>= 20) calls after a warm-up: median, min and max.  Host leg: perf_counter around one call, the
D2H copy included, `--host-reps` calls.  Beside the times: the f64 flops the algorithm needs, S 2 D (m^2 + 2 m (m + 1) / 2)
(the xy square and the two triangles with their diagonals), over the measured time as a fraction of the f64 MFMA peak
(78.6 TF, AMD's published figure); the bytes one k-step of one tile pulls from L2 (two 64-row x 32-column f32 blocks,
one on a diagonal tile) and their total; the workspace.  Before timing, the device scores are compared with route (b)'s
f64 scores.  No threshold: the numbers are recorded, not gated; where a shape is slower than (b) the JSON says so.

    python tools/kid_bench.py [--reps 20] [--out profiles/kid_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch
from importlib import import_module

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
M = import_module(PKG + ".metrics")
LIB = import_module(PKG + "._lib")
F64_PEAK = 78.6e12


def event_times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def wall_times(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def poly(a, c, gamma, coef, degree):
    base = gamma * (a @ c.T) + coef
    k = base
    for _ in range(degree - 1):
        k = k * base
    return k


def host_route(rd, fd, ir, jf, gamma, coef, degree):
    r, f = rd.cpu().numpy().astype(np.float64), fd.cpu().numpy().astype(np.float64)
    m = ir.shape[1]
    sc = np.empty(len(ir))
    for s in range(len(ir)):
        x, y = r[ir[s]], f[jf[s]]
        kxx, kyy, kxy = poly(x, x, gamma, coef, degree), poly(y, y, gamma, coef, degree), poly(x, y, gamma, coef, degree)
        sc[s] = ((kxx.sum() - np.trace(kxx)) + (kyy.sum() - np.trace(kyy))) / (m * (m - 1.0)) - 2.0 * kxy.sum() / (m * m)
    return sc.mean(), sc.std()


def torch_route(rd, fd, ird, jfd, gamma, coef, degree, dtype):
    m = ird.shape[1]
    sc = []
    for s in range(ird.shape[0]):
        x, y = rd.index_select(0, ird[s]).to(dtype), fd.index_select(0, jfd[s]).to(dtype)
        kxx, kyy, kxy = poly(x, x, gamma, coef, degree), poly(y, y, gamma, coef, degree), poly(x, y, gamma, coef, degree)
        sc.append(((kxx.sum() - kxx.diagonal().sum()) + (kyy.sum() - kyy.diagonal().sum())) / (m * (m - 1.0))
                  - 2.0 * kxy.sum() / (m * m))
    sc = torch.stack(sc)
    return sc, torch.stack([sc.mean(), sc.std(unbiased=False)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=3000)
    ap.add_argument("--dims", type=int, nargs="+", default=[100, 200, 2048])
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kid_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kid_bench needs the MI355X: there is nothing to time without it")
    if a.reps < 20:
        raise SystemExit("kid_bench: --reps must be at least 20")
    dev, N, S, m, deg = "cuda", a.rows, a.subsets, a.subset_size, a.degree
    lib = LIB.load()
    T = (m + 63) // 64
    P = T * (T + 1) // 2
    rows = []
    for D in a.dims:
        g = torch.Generator(device=dev).manual_seed(1000 * D + N)
        real = torch.randn(N, D, generator=g, device=dev)
        fake = 0.25 + 0.9 * torch.randn(N, D, generator=g, device=dev)
        gamma, coef = 1.0 / D, 1.0
        ir, jf = M.kid_subsets(N, N, S, m, 0)
        ird, jfd = torch.from_numpy(ir).to(dev), torch.from_numpy(jf).to(dev)
        ird64, jfd64 = ird.long(), jfd.long()
        scores, stat, _ = ops.kid_scores(real, fake, ird, jfd, deg, gamma, coef)
        sc64, st64 = torch_route(real, fake, ird64, jfd64, gamma, coef, deg, torch.float64)
        sc32, st32 = torch_route(real, fake, ird64, jfd64, gamma, coef, deg, torch.float32)
        row = {"N": N, "D": D, "subsets": S, "subset_size": m, "degree": deg,
               "kid_mean": float(stat[0]), "kid_std": float(stat[1]),
               "scores_max_abs_diff_vs_torch_f64": float((scores - sc64).abs().max()),
               "torch_f32_scores_max_abs_diff_vs_torch_f64": float((sc32.double() - sc64).abs().max()),
               "torch_f32_kid_mean": float(st32[0]), "torch_f64_kid_mean": float(st64[0])}
        dev_ms = event_times(lambda: ops.kid_scores(real, fake, ird, jfd, deg, gamma, coef), a.reps, a.warmup)
        b64 = event_times(lambda: torch_route(real, fake, ird64, jfd64, gamma, coef, deg, torch.float64), a.reps, a.warmup)
        b32 = event_times(lambda: torch_route(real, fake, ird64, jfd64, gamma, coef, deg, torch.float32), a.reps, a.warmup)
        host = wall_times(lambda: host_route(real, fake, ir, jf, gamma, coef, deg), a.host_reps)
        flops = float(S) * 2.0 * D * (m * m + 2.0 * m * (m + 1) / 2.0)
        steps = (D + 31) // 32
        med = statistics.median(dev_ms)
        row.update({
            "device": summary(dev_ms), "torch_f64": summary(b64), "torch_f32": summary(b32), "host": summary(host),
            "f64_flops_needed": flops, "f64_mfma_peak_fraction": flops / (med * 1e-3) / F64_PEAK,
            "l2_bytes_per_tile_step": {"off_diagonal": 2 * 64 * 32 * 4, "diagonal": 64 * 32 * 4},
            "l2_bytes_total": S * steps * ((2 * (P - T) + T * T) * 16384 + 2 * T * 8192),
            "workgroups": S * (2 * P + T * T), "workspace_bytes": int(lib.vg_kid_scores_ws_bytes(m, S)),
            "slower_than_torch_f64": bool(med > statistics.median(b64)),
            "slower_than_torch_f32": bool(med > statistics.median(b32))})
        print(json.dumps(row), flush=True)
        rows.append(row)
        del real, fake
    out = {"what": "KID: device route vs host route (a) and stock torch on the GPU in f32 / f64 (b); tools/kid_bench.py",
           "device": torch.cuda.get_device_name(0), "peaks": {"f64_mfma_published": F64_PEAK}, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
