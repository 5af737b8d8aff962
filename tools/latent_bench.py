"""Latent prior: the device route (ops.latent_hist: fit of the [N, 2L] latents; ops.latent_sample: n draws to the
Generator's input z) against the host route the reference takes (main_vae.py:415-436, :469-487: the latents as a numpy
array, 2L x np.histogram + np.cumsum, then a Python loop of three numpy calls per sampled element).

N = 30 000, 2L = 200, 100 bins (CelebA-HQ with latent_dim 100).  Both legs in one process on the same box.  Device: eager
launches (no hipGraph), device events around `reps` back-to-back calls after a warm-up; host: perf_counter around one
call; the figure is the median over the rounds.  The D2H copy of the latents (24 MB) and the H2D copy of the host draws
are excluded on both sides.  The host sampling loop is timed for n = 64 only (it is minutes at 3 000).  Before timing, the
device fit is compared with numpy's on the same matrix (bitwise).  Beside the times: the bytes the fit has to read,
2 * N * D * 4 (one min / max pass, one binning pass), over the time of the whole fit (its four launches), as a fraction
of the MI355X's 8 TB/s HBM peak -- reported, no threshold.  Exit status 1 if the device fit is slower than the host fit.

    python tools/latent_bench.py [--reps 200] [--rounds 7] [--out profiles/latent_bench.json]"""
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
G = import_module(PKG + ".geometry")
HBM_PEAK = 8.0e12                                   # bytes / s


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps         # us per call


def host_fit(x, n_bins):
    D = x.shape[1]
    edges, cdf = np.empty((D, n_bins + 1)), np.empty((D, n_bins))
    for c in range(D):
        freqs, edges[c] = np.histogram(x[:, c], bins=n_bins)
        cdf[c] = np.cumsum(freqs / x.shape[0])
    return edges, cdf


def host_sample_z(edges, cdf, n, L):
    """Inverse-CDF draw per element through the legacy global numpy stream, then z = mu + exp(logvar / 2) * randn."""
    mulv = np.empty((n, 2 * L), np.float32)
    for row in mulv:
        for c in range(2 * L):
            b = np.searchsorted(cdf[c], np.random.rand())
            row[c] = np.random.uniform(edges[c, b], edges[c, b + 1])
    return mulv[:, :L] + np.exp(0.5 * mulv[:, L:]) * np.random.standard_normal((n, L)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latent_bench needs the MI355X; a CPU run cannot give a time")
    dev, N, L, NB = "cuda", 30000, 100, 100
    D = 2 * L
    g = np.random.default_rng(1)
    xh = (g.standard_normal((N, D)) * g.uniform(0.3, 2.0, D) + g.uniform(-3, 3, D)).astype(np.float32)
    x = torch.from_numpy(xh).to(dev)
    edges, counts, cdf, status = ops.latent_hist(x, NB)
    he, hc = host_fit(xh, NB)
    same = (int(status.item()) == 0 and np.array_equal(edges.cpu().numpy().astype(np.float64), he)
            and np.array_equal(cdf.cpu().numpy(), hc))
    if not same:
        raise SystemExit("the device fit differs from numpy's on the benchmark matrix; no time is reported")
    ns = ops.NoiseStream(dev, 7)
    zspec = (G.padc(L, G.BF16), G.BF16)

    def dev_fit():
        return ops.latent_hist(x, NB)

    def dev_sample(n):
        return lambda: ops.latent_sample(edges, cdf, L, n, None, None, None, ns.state, want_mulv=False, z=zspec)

    for fn in (dev_fit, dev_sample(64), dev_sample(3000)):          # warm-up: code objects, allocator, workspace
        timed(fn, 20)
    t = {"dev_fit": [], "host_fit": [], "dev_s64": [], "dev_s3000": [], "host_s64": []}
    np.random.seed(0)
    for _ in range(a.rounds):
        t["dev_fit"].append(timed(dev_fit, a.reps))
        t0 = time.perf_counter()
        host_fit(xh, NB)
        t["host_fit"].append((time.perf_counter() - t0) * 1e6)
        t["dev_s64"].append(timed(dev_sample(64), a.reps))
        t["dev_s3000"].append(timed(dev_sample(3000), a.reps))
        t0 = time.perf_counter()
        host_sample_z(he, hc, 64, L)
        t["host_s64"].append((time.perf_counter() - t0) * 1e6)
    med = {k: statistics.median(v) for k, v in t.items()}
    nbytes = 2 * N * D * 4
    out = {"what": "us per call, median of %d interleaved rounds; device: %d eager calls between device events; host: one call, "
                   "perf_counter; copies between host and device excluded on both sides" % (a.rounds, a.reps),
           "device": torch.cuda.get_device_name(0), "numpy": np.__version__, "N": N, "D": D, "n_bins": NB,
           "device_fit_equals_numpy_bitwise": True,
           "fit": {"device_us": round(med["dev_fit"], 2), "host_us": round(med["host_fit"], 1),
                   "device_us_min_max": [round(min(t["dev_fit"]), 2), round(max(t["dev_fit"]), 2)],
                   "host_us_min_max": [round(min(t["host_fit"]), 1), round(max(t["host_fit"]), 1)],
                   "host_over_device": round(med["host_fit"] / med["dev_fit"], 1),
                   "device_not_slower_than_host": med["dev_fit"] <= med["host_fit"],
                   "bytes_read": nbytes, "GBps_over_the_whole_fit": round(nbytes / med["dev_fit"] / 1e3, 1),
                   "hbm_fraction": round(nbytes / (med["dev_fit"] * 1e-6) / HBM_PEAK, 4)},
           "sample_to_z": {"device_us_n64": round(med["dev_s64"], 2), "device_us_n3000": round(med["dev_s3000"], 2),
                           "host_us_n64": round(med["host_s64"], 1), "host_us_n3000": "not measured",
                           "host_over_device_n64": round(med["host_s64"] / med["dev_s64"], 1)}}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    if not out["fit"]["device_not_slower_than_host"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
