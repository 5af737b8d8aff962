"""What training on degraded pairs (VAEGANTrainer.train_step(..., noisy=, rects=), hole_weight) costs,
measured on the MI355X.  Four modes (`--mode`; `all` runs kernel and step in one process), writing into one JSON (`--out`):

  kernel  ops.region_mse_forward_backward (loss + hole_mse + gradient) against ops.mse_forward_backward (loss + gradient) on
          the same tensors at (128,3,64,64) and (32,3,256,256).  Outputs are compared first (w_hole = 1: the two losses and
          gradients must agree to rounding).  Each side's `--reps` launches are captured into one hipGraph and the two graphs
          are replayed INTERLEAVED, `--rounds` rounds of (mse window, region window), one device-event pair per window: no
          launch overhead in the figure.  Reported: us per call (both launches of a call: partial sums + gradient, one-wave
          final), the 12 B / element the pass has to move over the HBM rate (peak: MI355X_MICROARCH.md) as its floor, the
          ratio region / mse with the mse side's own spread.
  step    S = 64, B = 128, bf16, train_step_graphed with device-drawn noise (the benchmarked configuration), three trainers
          built from the same seed -- unpaired; paired with hole_weight = 1 (noisy given, the pixel MSE launches); paired with
          hole_weight = 6 and rects (the region kernel) -- timed INTERLEAVED: `--rounds` rounds of one window each, `--steps`
          replayed iterations per window.  Reported: every window's ms / step, medians, the unpaired side's spread (max -
          min) as the noise of the comparison, both ratios, kernel launches per step.
  trace   `--shape B,C,H,W`: nothing but `--reps` eager calls of each side at one shape, to be run under
          `rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace_BxCxHxW -- python tools/pairloss_bench.py
          --mode trace --shape B,C,H,W` (a run of its own per shape).
  merge   `--trace-dir DIR`: no device; reads the *kernel_stats.csv of every DIR/trace_* and adds the four kernels' own
          times (streaming and final launch of each side) and the streaming kernels' share of the HBM peak.

A measurement path without the GPU fails; nothing is gated.

    python tools/pairloss_bench.py --mode all [--rounds 5] [--steps 300] [--reps 200]
    python tools/pairloss_bench.py --mode merge --trace-dir runs/pairloss"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch
from importlib import import_module

import vaegan_amd as V

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
HBM_PEAK = 8.0e12
SHAPES = [(128, 3, 64, 64), (32, 3, 256, 256)]
BYTES_PER_ELEMENT = 12                  # a and b read once, d_a written once


def build(S, dtype, dev, **kw):
    V.configure_seed(42)
    e, g, d = V.Encoder([3, S, S], 100, dtype=dtype), V.Generator(nz=100, img_size=S, dtype=dtype), \
        V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init), d.apply(V.weights_init)
    e.to(dev), g.to(dev), d.to(dev)
    tr = V.VAEGANTrainer(e, g, d, *(V.Adam(m.parameters(), lr=2e-4) for m in (e, g, d)), **kw)
    tr.train()
    return tr


def window_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def make_rects(B, H, W, dev, seed=3):
    """Rectangles in the ranges data.degrade_bounds gives: sides in [1 %, 25 %] of the image, inside its middle half."""
    g = torch.Generator().manual_seed(seed)
    r = torch.zeros(B, 8)
    r[:, 2] = torch.randint(max(1, round(H * 0.01)), round(H * 0.25) + 1, (B,), generator=g)
    r[:, 3] = torch.randint(max(1, round(W * 0.01)), round(W * 0.25) + 1, (B,), generator=g)
    r[:, 4] = round(W * 0.25) + (torch.rand(B, generator=g) * (W * 0.5 - r[:, 3])).floor()
    r[:, 5] = round(H * 0.25) + (torch.rand(B, generator=g) * (H * 0.5 - r[:, 2])).floor()
    return r.to(dev)


def degrade(clean, rects, seed=4):
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = clean.shape
    h, w = torch.arange(H).view(1, 1, H, 1), torch.arange(W).view(1, 1, 1, W)
    r = rects.cpu()
    rh, rw, x, y = (r[:, k].view(B, 1, 1, 1) for k in (2, 3, 4, 5))
    m = (h >= y) & (h < y + rh) & (w >= x) & (w < x + rw)
    fill = torch.rand(clean.shape, generator=g) * 2 - 1
    return (torch.where(m, fill, clean.cpu()) + 0.1 * torch.randn(clean.shape, generator=g)).clamp(-1, 1).to(clean.device)


def capture_reps(fn, reps):
    """`reps` calls of fn in one hipGraph (one stream, no parallel branches)."""
    fn()                                                          # sizes the workspace
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    return g


def mode_kernel(a, dev):
    rows = []
    for shape in SHAPES:
        B, C, H, W = shape
        gen = torch.Generator().manual_seed(sum(shape))
        x = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
        y = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
        rects = make_rects(B, H, W, dev)
        l_m, l_r, h_r = (torch.zeros(1, device=dev) for _ in range(3))
        d_m = ops.mse_forward_backward(x, y, 0.37, l_m, True)
        d_r = ops.region_mse_forward_backward(x, y, rects, 1.0, 0.37, loss=l_r, hole_mse=h_r, want_grad=True)
        cmp_ = {"loss_mse": float(l_m), "loss_region_w1": float(l_r),
                "grad_max_abs_diff_over_max": float((d_m - d_r).abs().max() / d_m.abs().max())}
        assert abs(cmp_["loss_mse"] - cmp_["loss_region_w1"]) <= 1e-6 * cmp_["loss_mse"] and cmp_["grad_max_abs_diff_over_max"] <= 1e-6, cmp_

        def mse_call():
            ops.mse_forward_backward(x, y, 0.37, l_m, True)

        def region_call():
            ops.region_mse_forward_backward(x, y, rects, 6.0, 0.37, loss=l_r, hole_mse=h_r, want_grad=True)

        graphs = {"mse": capture_reps(mse_call, a.reps), "region": capture_reps(region_call, a.reps)}
        for g in graphs.values():
            window_ms(g.replay, 3)
        us = {"mse": [], "region": []}
        for _ in range(a.rounds):
            for name, g in graphs.items():
                us[name].append(window_ms(g.replay, a.windows) / a.reps * 1e3)
        med = {k: statistics.median(v) for k, v in us.items()}
        n = B * C * H * W
        floor_us = n * BYTES_PER_ELEMENT / HBM_PEAK * 1e6
        rows.append({"shape": list(shape), "n": n, "outputs_compared_first": cmp_, "us_per_call": us, "median_us": med,
                     "mse_spread_us": max(us["mse"]) - min(us["mse"]), "region_over_mse": med["region"] / med["mse"],
                     "bytes_per_element": BYTES_PER_ELEMENT, "floor_us_bytes_over_hbm_peak": floor_us,
                     "floor_over_call_time": {k: floor_us / v for k, v in med.items()},
                     "achieved_bytes_per_s": {k: n * BYTES_PER_ELEMENT / (v * 1e-6) for k, v in med.items()},
                     "note": f"{a.reps} calls per captured graph, {a.windows} replays per window, device events; a call is the "
                             "streaming launch plus its one-wave final launch, so the figure is a call time, not a kernel time"})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def mode_step(a, dev):
    S, B = a.size, a.batch
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    rects = make_rects(B, S, S, dev)
    noisy = degrade(real, rects)
    trs = {"unpaired": (build(S, a.dtype, dev), {}),
           "paired_w1": (build(S, a.dtype, dev), dict(noisy=noisy)),
           "paired_w6": (build(S, a.dtype, dev, hole_weight=6.0), dict(noisy=noisy, rects=rects))}
    launches = {}
    for name, (tr, kw) in trs.items():
        n0 = ops.launch_count()
        tr.train_step_graphed(real, 60, **kw)                   # eager: sizes the workspaces, counts the launches
        launches[name] = ops.launch_count() - n0
        for _ in range(a.warmup):
            tr.train_step_graphed(real, 60, **kw)               # capture + replays
        assert tr._graph is not None and len(tr._graph[1]) == 1
    windows = {k: [] for k in trs}
    for _ in range(a.rounds):
        for name, (tr, kw) in trs.items():
            windows[name].append(window_ms(lambda: tr.train_step_graphed(real, 60, **kw), a.steps))
    med = {k: statistics.median(v) for k, v in windows.items()}
    losses = {k: tr.loss_dict(epoch=60) for k, (tr, _) in trs.items()}
    step = {"config": {"S": S, "B": B, "dtype": a.dtype, "hole_weight_on": 6.0, "mode": "train_step_graphed, device-drawn noise",
                       "steps_per_window": a.steps, "rounds": a.rounds, "warmup_steps": a.warmup},
            "ms_per_step": windows, "median_ms_per_step": med,
            "unpaired_spread_ms": max(windows["unpaired"]) - min(windows["unpaired"]),
            "paired_w1_over_unpaired": med["paired_w1"] / med["unpaired"],
            "paired_w6_over_unpaired": med["paired_w6"] / med["unpaired"],
            "paired_w6_minus_paired_w1_ms": med["paired_w6"] - med["paired_w1"],
            "kernel_launches_per_step": launches, "hole_mse_after_timing": losses["paired_w6"].get("hole_mse"),
            "finite": all(x == x and abs(x) != float("inf") for d in losses.values() for x in d.values())}
    print(json.dumps(step), flush=True)
    return step


KERNELS = ("region_mse_partial_kernel", "region_mse_final_kernel", "mse_partial_kernel", "mse_final_kernel")


def mode_trace(a, dev):
    shape = tuple(int(v) for v in a.shape.split(","))
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
    y = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
    rects = make_rects(B, H, W, dev)
    l_m, l_r, h_r = (torch.zeros(1, device=dev) for _ in range(3))
    for _ in range(a.reps):
        ops.mse_forward_backward(x, y, 0.37, l_m, True)
        ops.region_mse_forward_backward(x, y, rects, 6.0, 0.37, loss=l_r, hole_mse=h_r, want_grad=True)
    torch.cuda.synchronize()
    print("traced", shape, a.reps, "calls of each side; losses", float(l_m), float(l_r))


def mode_merge(a):
    rows = []
    for dname in sorted(glob.glob(os.path.join(a.trace_dir, "trace_*"))):
        shape = [int(v) for v in os.path.basename(dname)[len("trace_"):].split("x")]
        files = glob.glob(os.path.join(dname, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit(f"pairloss_bench --mode merge: no kernel_stats.csv under {dname}")
        stat = {}
        for r in csv.DictReader(open(max(files))):
            key = next((k for k in KERNELS if k in r["Name"]), None)      # region_* first: mse_* is a substring of it
            if key is not None and key not in stat:
                stat[key] = {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]),
                             "max_ns": float(r["MaxNs"])}
        n = shape[0] * shape[1] * shape[2] * shape[3]
        floor_us = n * BYTES_PER_ELEMENT / HBM_PEAK * 1e6
        row = {"shape": shape, "n": n, "rocprofv3_kernel_stats": stat, "floor_us_bytes_over_hbm_peak": floor_us}
        for side in ("region_mse", "mse"):
            part, fin = stat[side + "_partial_kernel"]["average_ns"] * 1e-3, stat[side + "_final_kernel"]["average_ns"] * 1e-3
            row[side] = {"streaming_kernel_us": part, "final_kernel_us": fin, "floor_over_streaming_kernel": floor_us / part,
                         "achieved_bytes_per_s": n * BYTES_PER_ELEMENT / (part * 1e-6)}
        row["region_minus_mse_us"] = {"streaming_kernel": row["region_mse"]["streaming_kernel_us"] - row["mse"]["streaming_kernel_us"],
                                      "final_kernel": row["region_mse"]["final_kernel_us"] - row["mse"]["final_kernel_us"]}
        rows.append(row)
        print(json.dumps(row))
    if not rows:
        raise SystemExit(f"pairloss_bench --mode merge: no trace_* directories in {a.trace_dir}")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "kernel", "all", "trace", "merge"), required=True)
    ap.add_argument("--shape", default="128,3,64,64")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "runs", "pairloss"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=200, help="kernel mode: calls per captured graph")
    ap.add_argument("--windows", type=int, default=10, help="kernel mode: graph replays per timed window")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairloss_bench.json"))
    a = ap.parse_args()
    if a.mode == "merge":
        out = json.load(open(a.out)) if os.path.isfile(a.out) else {}
        out["kernel_trace"] = mode_merge(a)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return print("wrote", a.out)
    if not torch.cuda.is_available():
        raise SystemExit("pairloss_bench needs the MI355X: there is nothing to time without it")
    dev = "cuda"
    torch.cuda.set_device(0)
    if a.mode == "trace":
        return mode_trace(a, dev)
    out = json.load(open(a.out)) if os.path.isfile(a.out) else {}
    out["what"] = "training on degraded pairs: the region-weighted MSE launch against the MSE launch (replayed from graphs, " \
                  "interleaved) and the graphed step unpaired / paired / paired with the weighted term; tools/pairloss_bench.py"
    out["peaks"] = {"hbm_bytes_per_s": HBM_PEAK}
    out["device"] = torch.cuda.get_device_name(0)
    if a.mode in ("kernel", "all"):
        out["kernel_vs_mse"] = mode_kernel(a, dev)
    if a.mode in ("step", "all"):
        out["step"] = mode_step(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
