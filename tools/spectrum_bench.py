"""Radial power spectra: the device route (ops.spectrum_profiles -> vg_spectrum_profiles: mean, transform and bin launches)
against a stock route on the same GPU, measured in one process with the legs interleaved:

  (a) stock torch: subtract the plane means, multiply by the 2-D Hann window, ``torch.fft.rfft2`` (in f64, what the kernel
      computes in, and in f32), |.|^2 summed over the channels, the Hermitian weight, ``index_add_`` into the radial bins.
      If torch.fft does not run on the box the row says so and the leg is left out.

Shapes: S = 64 / B = 128, S = 128 / B = 64, S = 256 / B = 32, C = 3, the default n_bins = S / 2, Hann window, centring on;
``device_2d`` is the same call with the identity table (``bins="2d"``), whose one-entry bins take the thread-per-bin sum.
Every leg: one device-event pair around each call, `--reps` (>= 20) calls after a warm-up, one call of each leg in turn:
median, min and max.  Beside the times: the f64 FLOPs of the two matrix products, 2 C H W Wh (2 + 4 H / W) per image
(SpectrumPlan.flops), over the median as a fraction of the f64 MFMA peak (78.6 TF, AMD's published figure), the workspace,
and the largest relative deviation of the device profiles from route (a) in f64.

End to end: ``evaluate_generation_spectrum`` against ``evaluate_generation`` on the same loader (S = 64, 16 batches of 64
uniform-noise images, injected z), wall clock around whole passes (each ends in its host sync), interleaved.

No threshold: the numbers are recorded, not gated; where the stock route is faster the JSON says so.

    python tools/spectrum_bench.py [--reps 20] [--out profiles/spectrum_bench.json]"""
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

import vaegan_amd as V

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
S = import_module(PKG + ".spectrum")
LIB = import_module(PKG + "._lib")
F64_PEAK = 78.6e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def interleaved(legs, reps, warmup):
    """legs: name -> callable.  One call of each leg in turn per repeat."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    out = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            out[k].append(timed(fn))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def stock_route(x, plan, w2, weight, bin_of, dtype):
    xd = x.to(dtype)
    xc = (xd - xd.mean(dim=(2, 3), keepdim=True)) * w2.to(dtype)
    F = torch.fft.rfft2(xc)
    P = (F.real ** 2 + F.imag ** 2).sum(1) * weight.to(dtype)
    prof = torch.zeros(x.shape[0], plan.n_bins, dtype=dtype, device=x.device)
    return prof.index_add_(1, bin_of, P.flatten(1))


def end_to_end(reps):
    V.configure_seed(42)
    g = V.Generator(nz=100, img_size=64, dtype="bf16")         # the flagship configuration's Generator, initial weights
    g.apply(V.weights_init)
    g.to("cuda")
    gen = torch.Generator().manual_seed(5)
    vl = [(torch.rand(64, 3, 64, 64, generator=gen) * 2 - 1).to("cuda") for _ in range(16)]
    zs = [torch.randn(64, 100, generator=gen).to("cuda") for _ in vl]
    nf = lambda i, b: zs[i]                                                            # noqa: E731
    legs = {"evaluate_generation": lambda: V.evaluate_generation(g, vl, noise_fn=nf),
            "evaluate_generation_spectrum": lambda: V.evaluate_generation_spectrum(g, vl, noise_fn=nf)}
    for fn in legs.values():
        fn()
    out = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            out[k].append((time.perf_counter() - t0) * 1e3)
    res = {k: summary(v) for k, v in out.items()}
    res["images"] = 16 * 64
    res["added_ms_median"] = res["evaluate_generation_spectrum"]["median_ms"] - res["evaluate_generation"]["median_ms"]
    res["result"] = {k: v for k, v in legs["evaluate_generation_spectrum"]().items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[64, 128, 128, 64, 256, 32], help="S B pairs")
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_bench needs the MI355X: there is nothing to time without it")
    if a.reps < 20:
        raise SystemExit("spectrum_bench: --reps must be at least 20")
    dev, C = "cuda", a.channels
    lib = LIB.load()
    rows = []
    for Sz, B in zip(a.shapes[0::2], a.shapes[1::2]):
        plan = S.spectrum_plan(Sz, Sz)
        g = torch.Generator(device=dev).manual_seed(Sz * 1000 + B)
        x = torch.rand(B, C, Sz, Sz, generator=g, device=dev) * 2 - 1
        w2 = torch.from_numpy(np.outer(S.window_table(Sz, "hann"), S.window_table(Sz, "hann"))).to(dev)
        weight = torch.from_numpy(plan.weight).to(dev)
        bin_of = torch.from_numpy(plan.bin_of.reshape(-1)).to(dev)
        plan2d = S.spectrum_plan(Sz, Sz, bins="2d")            # short bins: the thread-per-bin form of the bin sum
        legs = {"device": lambda: ops.spectrum_profiles(x, plan), "device_2d": lambda: ops.spectrum_profiles(x, plan2d)}
        row = {"S": Sz, "B": B, "C": C, "n_bins": plan.n_bins}
        try:
            ref = stock_route(x, plan, w2, weight, bin_of, torch.float64)
            got = ops.spectrum_profiles(x, plan)
            row["max_rel_diff_vs_torch_f64"] = float(((got - ref).abs() / ref.abs()).max())
            legs["torch_fft_f64"] = lambda: stock_route(x, plan, w2, weight, bin_of, torch.float64)
            legs["torch_fft_f32"] = lambda: stock_route(x, plan, w2, weight, bin_of, torch.float32)
        except RuntimeError as e:
            row["torch_fft"] = "did not run on this box: " + str(e).splitlines()[0]
        ms = interleaved(legs, a.reps, a.warmup)
        flops = plan.flops(C) * B
        med = statistics.median(ms["device"])
        need = LIB.c_int64(0)
        lib.vg_spectrum_ws_bytes(B, C, Sz, Sz, LIB.byref(need))
        row.update({k: summary(v) for k, v in ms.items()})
        row.update({"f64_flops_needed": flops, "f64_tflops": flops / (med * 1e-3) / 1e12,
                    "f64_mfma_peak_fraction": flops / (med * 1e-3) / F64_PEAK, "workspace_bytes": int(need.value),
                    "workgroups_transform": B * ((plan.Wh + 15) // 16), "lds_bytes_per_workgroup": 2 * ((Sz + 15) // 16 * 16) * 16 * 8})
        for k in ("torch_fft_f64", "torch_fft_f32"):
            if k in ms:
                row["slower_than_" + k] = bool(med > statistics.median(ms[k]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    e2e = end_to_end(a.reps)
    print(json.dumps(e2e), flush=True)
    out = {"what": "radial power spectra: vg_spectrum_profiles vs torch.fft.rfft2 + index_add_ on the same GPU, and "
                   "evaluate_generation_spectrum vs evaluate_generation; tools/spectrum_bench.py",
           "device": torch.cuda.get_device_name(0), "peaks": {"f64_mfma_published": F64_PEAK}, "rows": rows,
           "end_to_end_S64": e2e}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
