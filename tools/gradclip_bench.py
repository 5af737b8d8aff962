"""What gradient-norm clipping (VAEGANTrainer(..., max_grad_norm=)) costs, measured on the MI355X in
one process:

  (1) the step: S = 64, B = 128, bf16, VAEGANTrainer.train_step_graphed with device-drawn noise (the benchmarked
      configuration), two trainers of the SAME build from the same seed -- off: max_grad_norm=None, on: a finite max norm on
      all three networks -- timed INTERLEAVED: `--rounds` rounds of (off window, on window), each window `--steps` replayed
      iterations between one device-event pair.  Reported: every window's ms / step, the medians, the off trainer's spread
      (max - min) as the noise of the comparison, and on - off: 2 d_iters + 2 more launches (two per clip point) that read
      the Discriminator's gradient buffer d_iters times and the Encoder's and the Generator's once.
  (2) the reduction alone: ops.grad_norm_clip over gradient buffers of the Encoder's and the Generator's sizes (one call for
      both, as the trainer issues it), `--chain` calls captured into ONE hipGraph and the graph replayed `--reps` times between
      one event pair (no host launch cost; the gaps between graph nodes, two per call, are in the figure), against its byte
      count -- 4 bytes per element, read once -- over the HBM peak (8 TB/s, MI355X_MICROARCH.md) and over the measured
      streaming rate (6.3 TB/s).  The trainer-sized buffers (~55 MB) fit the 256 MiB Infinity Cache when the call is repeated
      back to back, so that row is NOT an HBM stream measurement; a second row takes one buffer of 2^27 elements (537 MB
      per call), which does not fit.

A measurement path without the GPU fails; both are recorded, not gated.

    python tools/gradclip_bench.py [--rounds 5] [--steps 300] [--out profiles/gradclip_bench.json]"""
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
L = import_module(PKG + "._lib")
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12


def build(S, dtype, dev, max_grad_norm):
    V.configure_seed(42)
    e, g, d = V.Encoder([3, S, S], 100, dtype=dtype), V.Generator(nz=100, img_size=S, dtype=dtype), \
        V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init), d.apply(V.weights_init)
    e.to(dev), g.to(dev), d.to(dev)
    oe, og, od = (V.Adam(m.parameters(), lr=2e-4) for m in (e, g, d))
    tr = V.VAEGANTrainer(e, g, d, oe, og, od, max_grad_norm=max_grad_norm)
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


def kernel_row(name, sizes, chain, reps, rounds, dev):
    """`chain` grad_norm_clip calls over buffers of `sizes` elements in one hipGraph, replayed: us per call and bytes / s."""
    gen = torch.Generator(device=dev).manual_seed(len(sizes))
    g = [torch.randn(n, generator=gen, device=dev) for n in sizes]
    out = [torch.zeros(2, device=dev) for _ in sizes]
    ws = torch.empty(L.VG_GNORM_MAX * L.VG_GNORM_PARTS, dtype=torch.float64, device=dev)
    fn = lambda: ops.grad_norm_clip(g, [1.0] * len(sizes), [1.0] * len(sizes), out, ws)        # noqa: E731
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            fn()
    window_ms(graph.replay, 3)
    ms = [window_ms(graph.replay, reps) / chain for _ in range(rounds)]
    m = statistics.median(ms)
    nbytes = 4 * sum(sizes)
    grid = sum(min(max((n // 4 + 1023) // 1024, 1), L.VG_GNORM_PARTS) for n in sizes)
    return {"name": name, "elements": list(sizes), "buffers_per_call": len(sizes), "launches_per_call": 2,
            "workgroups_launch_a": grid, "bytes_read": nbytes, "calls_per_graph": chain, "graph_replays_per_window": reps,
            "us_per_call": [x * 1e3 for x in ms], "median_us_per_call": m * 1e3,
            "achieved_bytes_per_s": nbytes / (m * 1e-3),
            "least_time_us_at_hbm_peak": nbytes / HBM_PEAK * 1e6, "least_time_us_at_measured_stream_rate": nbytes / HBM_STREAM * 1e6,
            "share_of_hbm_peak": nbytes / HBM_PEAK / (m * 1e-3), "share_of_measured_stream_rate": nbytes / HBM_STREAM / (m * 1e-3),
            "fits_infinity_cache": nbytes < (256 << 20),
            "norm_coef_of_the_last_call": [o.tolist() for o in out]}


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
    ap.add_argument("--max-norm", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradclip_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gradclip_bench needs the MI355X: there is nothing to time without it")
    dev, S, B = "cuda", a.size, a.batch
    torch.cuda.set_device(0)

    # ---- (1) the step, interleaved ----
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    trs = {"off": build(S, a.dtype, dev, None), "on": build(S, a.dtype, dev, a.max_norm)}
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
    sizes = {k: o.numel for k, o in (("E", on.opt_E), ("G", on.opt_G), ("D", on.opt_D))}
    report = on.loss_dict(epoch=60)
    read = 4 * (sizes["E"] + sizes["G"] + on.d_iters * sizes["D"])
    step = {"config": {"S": S, "B": B, "dtype": a.dtype, "max_grad_norm": a.max_norm, "d_iters": on.d_iters,
                       "mode": "train_step_graphed, device-drawn noise", "steps_per_window": a.steps,
                       "rounds": a.rounds, "warmup_steps": a.warmup},
            "gradient_elements": sizes, "bytes_read_by_the_reductions_per_step": read,
            "least_time_us_for_those_bytes_at_measured_stream_rate": read / HBM_STREAM * 1e6,
            "ms_per_step": windows, "median_ms_per_step": med,
            "off_spread_ms": max(windows["off"]) - min(windows["off"]),
            "on_minus_off_ms": med["on"] - med["off"], "on_over_off": med["on"] / med["off"],
            "kernel_launches_per_step": launches, "more_launches": launches["on"] - launches["off"],
            "last_step_norms_and_coefficients": {k: v for k, v in report.items() if k.startswith(("grad_norm_", "clip_coef_"))},
            "finite": all(x == x and abs(x) != float("inf") for x in report.values())}
    print(json.dumps(step), flush=True)
    del trs, on

    # ---- (2) the reduction alone, replayed from a graph ----
    rows = [kernel_row("trainer-sized: the Encoder's and the Generator's gradient buffers in one call", [sizes["E"], sizes["G"]],
                       a.chain, a.reps, a.rounds, dev),
            kernel_row("one buffer of 2^27 elements: past the Infinity Cache", [1 << 27], a.chain, max(a.reps // 10, 5),
                       a.rounds, dev)]
    for r in rows:
        print(json.dumps(r), flush=True)
    out = {"what": "gradient-norm clipping: interleaved A/B of the graphed step with max_grad_norm off / on (same build), and the "
                   "reduction alone, replayed from a graph, against its byte count; tools/gradclip_bench.py",
           "command": "python tools/gradclip_bench.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "peaks": {"hbm_bytes_per_s": HBM_PEAK, "measured_stream_bytes_per_s": HBM_STREAM},
           "step": step, "kernel": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
