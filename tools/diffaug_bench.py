"""What the differentiable augmentation of the Discriminator's inputs (VAEGANTrainer(..., augment=))
costs, measured on the MI355X in one process:

  (1) the step: S = 64, B = 128, bf16, VAEGANTrainer.train_step_graphed with device-drawn noise (the benchmarked
      configuration), two trainers of the SAME build from the same seed -- off: augment=None, on: the full policy
      "color,translation,cutout" -- timed INTERLEAVED: `--rounds` rounds of (off window, on window), each window `--steps`
      replayed iterations between one device-event pair.  Reported: every window's ms / step, the medians, the off trainer's
      spread (max - min) as the noise of the comparison, and on - off: 5 more launches (the table; reduce + apply over the
      [2B] batch forward; reduce + apply over the [B] gradient backward).
  (2) the launches alone: ops.diffaug_forward over a [2B] batch and ops.diffaug_backward over a [B] gradient of the step's
      shape, `--chain` calls captured into ONE hipGraph and the graph replayed `--reps` times between one event pair (no host
      launch cost; the gaps between graph nodes, two per call, are in the figure), against their byte counts -- read, read,
      write: 3 passes over the tensor (2 without the contrast bit's reduce) -- over the HBM peak (8 TB/s,
      MI355X_MICROARCH.md) and over the measured streaming rate (6.3 TB/s).  The step-sized tensors (16.8 MB and 8.4 MB) fit the
      256 MiB Infinity Cache when the call is repeated back to back, so those rows are NOT HBM stream measurements; a second
      pair of rows takes 512 images of 256 x 256 (537 MB per pass, bf16), which do not fit.

A measurement path without the GPU fails; both are recorded, not gated.

    python tools/diffaug_bench.py [--rounds 5] [--steps 300] [--out profiles/diffaug_bench.json]"""
import argparse
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
G = import_module(PKG + ".geometry")
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12
POLICY = "color,translation,cutout"


def build(S, dtype, dev, augment):
    V.configure_seed(42)
    e, g, d = V.Encoder([3, S, S], 100, dtype=dtype), V.Generator(nz=100, img_size=S, dtype=dtype), \
        V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init), d.apply(V.weights_init)
    e.to(dev), g.to(dev), d.to(dev)
    oe, og, od = (V.Adam(m.parameters(), lr=2e-4) for m in (e, g, d))
    tr = V.VAEGANTrainer(e, g, d, oe, og, od, augment=augment)
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


def kernel_row(name, which, N, PB, S, dt, need_sum, chain, reps, rounds, dev):
    """`chain` calls of one direction over [N, S, S, padc(3)] in one hipGraph, replayed: us per call and bytes / s."""
    aug = V.DiffAugment(POLICY if need_sum else "brightness,saturation,translation,cutout")
    CP = G.padc(3, dt)
    x = torch.randn(N, S, S, CP, generator=torch.Generator(device=dev).manual_seed(N), device=dev).to(ops.TORCH_DT[dt])
    y = torch.empty_like(x)
    table = aug.draw(torch.tensor([42, 1], dtype=torch.int64, device=dev), PB, S, S)
    call = aug.forward if which == "forward" else aug.backward
    fn = lambda: call(x, table, 3, dt, out=y)                                               # noqa: E731
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            fn()
    window_ms(graph.replay, 3)
    ms = [window_ms(graph.replay, reps) / chain for _ in range(rounds)]
    m = statistics.median(ms)
    tensor = x.numel() * x.element_size()
    nbytes = (3 if need_sum else 2) * tensor
    return {"name": name, "direction": which, "shape": [N, S, S, CP], "dtype": "bf16" if dt == G.BF16 else "fp32",
            "parameter_rows": PB, "launches_per_call": 2 if need_sum else 1, "workgroups_per_launch": N * ((S * S + 1023) // 1024),
            "tensor_bytes": tensor, "bytes_moved": nbytes, "calls_per_graph": chain, "graph_replays_per_window": reps,
            "us_per_call": [v * 1e3 for v in ms], "median_us_per_call": m * 1e3, "achieved_bytes_per_s": nbytes / (m * 1e-3),
            "least_time_us_at_hbm_peak": nbytes / HBM_PEAK * 1e6, "least_time_us_at_measured_stream_rate": nbytes / HBM_STREAM * 1e6,
            "share_of_hbm_peak": nbytes / HBM_PEAK / (m * 1e-3), "share_of_measured_stream_rate": nbytes / HBM_STREAM / (m * 1e-3),
            "fits_infinity_cache": 2 * tensor < (256 << 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffaug_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffaug_bench needs the MI355X: there is nothing to time without it")
    dev, S, B = "cuda", a.size, a.batch
    torch.cuda.set_device(0)

    # ---- (1) the step, interleaved ----
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    trs = {"off": build(S, a.dtype, dev, None), "on": build(S, a.dtype, dev, POLICY)}
    launches = {}
    for name, tr in trs.items():
        n0 = ops.launch_count()
        tr.train_step_graphed(real, 60)                         # eager: sizes the workspaces, counts the launches
        launches[name] = ops.launch_count() - n0
        for _ in range(a.warmup):
            tr.train_step_graphed(real, 60)                     # capture + replays
        assert tr._graph is not None and len(tr._graph[1]) == 1
    windows = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name, tr in trs.items():
            windows[name].append(window_ms(lambda: tr.train_step_graphed(real, 60), a.steps))
    med = {k: statistics.median(v) for k, v in windows.items()}
    on = trs["on"]
    dt = on.dt
    pixel = G.padc(3, dt) * (2 if dt == G.BF16 else 4)
    moved = 3 * (2 * B) * S * S * pixel + 3 * B * S * S * pixel
    report = on.loss_dict(epoch=60)
    step = {"config": {"S": S, "B": B, "dtype": a.dtype, "augment": POLICY, "d_iters": on.d_iters,
                       "mode": "train_step_graphed, device-drawn noise", "steps_per_window": a.steps,
                       "rounds": a.rounds, "warmup_steps": a.warmup},
            "bytes_moved_by_the_augmentation_per_step": moved,
            "least_time_us_for_those_bytes_at_measured_stream_rate": moved / HBM_STREAM * 1e6,
            "ms_per_step": windows, "median_ms_per_step": med,
            "off_spread_ms": max(windows["off"]) - min(windows["off"]),
            "on_minus_off_ms": med["on"] - med["off"], "on_over_off": med["on"] / med["off"],
            "kernel_launches_per_step": launches, "more_launches": launches["on"] - launches["off"],
            "last_table_first_rows": on.aug_params[:2].tolist(),
            "last_step_losses": report, "finite": all(x == x and abs(x) != float("inf") for x in report.values())}
    print(json.dumps(step), flush=True)
    del trs, on

    # ---- (2) the launches alone, replayed from a graph ----
    rows = []
    for which, N, PB in (("forward", 2 * B, B), ("backward", B, B)):
        rows.append(kernel_row(f"step-sized {which}: [{N}, {S}, {S}] images", which, N, PB, S, dt, True, a.chain, a.reps,
                               a.rounds, dev))
    rows.append(kernel_row("step-sized forward without the contrast bit: one launch", "forward", 2 * B, B, S, dt, False,
                           a.chain, a.reps, a.rounds, dev))
    for which in ("forward", "backward"):
        rows.append(kernel_row(f"512 images of 256 x 256, {which}: past the Infinity Cache", which, 512, 256, 256, G.BF16, True,
                               4, max(a.reps // 20, 3), a.rounds, dev))
    for r in rows:
        print(json.dumps(r), flush=True)
    out = {"what": "differentiable augmentation: interleaved A/B of the graphed step with augment off / on (same build), and the "
                   "forward / backward launches alone, replayed from a graph, against their byte counts; tools/diffaug_bench.py",
           "command": "python tools/diffaug_bench.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "peaks": {"hbm_bytes_per_s": HBM_PEAK, "measured_stream_bytes_per_s": HBM_STREAM},
           "step": step, "kernel": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
