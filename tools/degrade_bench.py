"""Degraded-pair batch assembly: the fused kernel (ops.gather_degrade_u8: clean NCHW + noisy NCHW + noisy NHWC bf16 in
one pass, per-image sigma, rectangle) against the nearest thing the three older entry points give -- ResidentImages.batch
+ NoiseStream.randn + ops.noisy_clamp_to_nhwc (three launches, ONE global sigma, no rectangle, same three outputs).

Both legs run in one process, interleaved round by round, eager launches (no hipGraph), device events around `reps`
back-to-back calls after a warm-up of every shape; the figure is the median over the rounds of the time per call.
Beside it: the algorithmic byte count of the fused kernel, B*H*W*(C + 8C + 2*CP) (u8 read, two f32 writes, bf16 NHWC write),
over its time, as a fraction of the MI355X's 8 TB/s HBM peak -- reported, no threshold.

    python tools/degrade_bench.py [--reps 2000] [--rounds 7] [--out profiles/degrade_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch
from importlib import import_module

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
data = import_module(PKG + ".data")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrade_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("degrade_bench needs the MI355X; a CPU run cannot give a time")
    dev, C, CP, N = "cuda", 3, 8, 512
    ns = ops.NoiseStream(dev, 1234)
    rows = []
    for S, B in ((64, 128), (128, 64), (256, 32)):
        gen = torch.Generator().manual_seed(S)
        ds = data.ResidentImages(torch.randint(0, 256, (N, S, S, C), dtype=torch.uint8, generator=gen), dev)
        idx = torch.randperm(N, generator=gen)[:B].to(dev)
        bounds = data.degrade_bounds(S, S)

        def fused():
            return ops.gather_degrade_u8(ds.images, idx, 99, 0, 0.25, True, True, bounds, nhwc=(CP, G.BF16))

        def chain():
            clean = ds.batch(idx)
            eps = ns.randn((B, C, S, S), 0)
            return ops.noisy_clamp_to_nhwc(clean, eps, 0.125, CP, G.BF16)

        # same clean batch from both; with sigma 0 and no rectangle the fused kernel's noisy output is the clean batch
        n0, c0, _ = ops.gather_degrade_u8(ds.images, idx, 99, 0, 0.0, False, True)
        assert torch.equal(c0, ds.batch(idx)) and torch.equal(n0, c0)
        for fn in (fused, chain):                    # warm-up: code objects, allocator
            timed(fn, 50)
        t = {"fused": [], "chain": []}
        for _ in range(a.rounds):
            t["fused"].append(timed(fused, a.reps))
            t["chain"].append(timed(chain, a.reps))
        f, c = statistics.median(t["fused"]), statistics.median(t["chain"])
        nbytes = B * S * S * (C + 8 * C + 2 * CP)
        row = {"S": S, "B": B, "fused_us": round(f, 2), "chain_us": round(c, 2), "fused_over_chain": round(f / c, 3),
               "fused_us_min_max": [round(min(t["fused"]), 2), round(max(t["fused"]), 2)],
               "chain_us_min_max": [round(min(t["chain"]), 2), round(max(t["chain"]), 2)],
               "fused_bytes": nbytes, "fused_GBps": round(nbytes / f / 1e3, 1),
               "fused_hbm_fraction": round(nbytes / (f * 1e-6) / HBM_PEAK, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "us per call, median of %d interleaved rounds of %d eager calls, device events; bf16 NHWC on" % (a.rounds, a.reps),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
