"""What weight averaging (ema.EMA, VAEGANTrainer(..., ema=)) costs, measured on the MI355X in one
process:

  (1) the step: S = 64, B = 128, bf16, VAEGANTrainer.train_step_graphed with device-drawn noise (the benchmarked
      configuration), two trainers of the SAME build from the same seed -- off: ema=None, on: an EMA over the Encoder and the
      Generator -- timed INTERLEAVED: `--rounds` rounds of (off window, on window), each window `--steps` replayed iterations
      between one device-event pair.  Reported: every window's ms / step, the medians, the off trainer's spread (max - min)
      as the noise of the comparison, and on - off: the one more launch at the end of the captured iteration.
  (2) the kernel alone: ops.ema_update over shadow / parameter buffers of the two optimizers' sizes (one launch for both, as
      the trainer issues it), `--chain` launches captured into ONE hipGraph and the graph replayed `--reps` times between one
      event pair (no host launch cost per kernel; the gaps between graph nodes are in the figure), against its byte count
      -- ema and p are read and ema is written: 12 bytes per element -- over the HBM peak (8 TB/s, MI355X_MICROARCH.md) and
      over the measured streaming rate (6.3 TB/s).  The trainer-sized buffers (~165 MB of traffic) fit the 256 MiB Infinity
      Cache when the launch is repeated back to back, so that row is NOT an HBM stream measurement; a second row takes one
      buffer of 2^27 elements (1.6 GB of traffic per launch), which does not fit.

A measurement path without the GPU fails; both are recorded, not gated.  The off case against the PARENT COMMIT is
tools/ab_tree.sh's job (interleaved bench.py runs of two built checkouts); `--merge-ab DIR` adds its bench lines to the JSON.

    python tools/ema_bench.py [--rounds 5] [--steps 300] [--out profiles/ema_bench.json]"""
import argparse
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
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12


def build(S, dtype, dev, with_ema, decay):
    V.configure_seed(42)
    e, g, d = V.Encoder([3, S, S], 100, dtype=dtype), V.Generator(nz=100, img_size=S, dtype=dtype), \
        V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init), d.apply(V.weights_init)
    e.to(dev), g.to(dev), d.to(dev)
    oe, og, od = (V.Adam(m.parameters(), lr=2e-4) for m in (e, g, d))
    ema = V.EMA([e, g], [oe, og], decay=decay) if with_ema else None
    tr = V.VAEGANTrainer(e, g, d, oe, og, od, ema=ema)
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


def merge_ab(ab_dir, out_path):
    """Add the interleaved parent-vs-this-tree bench lines of tools/ab_tree.sh to the JSON at out_path."""
    sides = {}
    for side in ("this_tree", "parent"):
        files = sorted(f for f in glob.glob(os.path.join(ab_dir, "ab_tree_*_*.json"))
                       if (os.path.basename(f).startswith("ab_tree_._")) == (side == "this_tree"))
        lines = [json.loads(open(f).read().strip().splitlines()[-1]) for f in files]
        if not lines:
            raise SystemExit(f"ema_bench --merge-ab: no bench lines of the {side} in {ab_dir}")
        sides[side] = {"ms_per_step": [d["ms_per_step"] for d in lines],
                       "median_ms_per_step": statistics.median(d["ms_per_step"] for d in lines)}
    spread = max(sides["parent"]["ms_per_step"]) - min(sides["parent"]["ms_per_step"])
    diff = sides["this_tree"]["median_ms_per_step"] - sides["parent"]["median_ms_per_step"]
    blk = dict(what="ema=None (the trainer bench.py builds) against the parent commit: tools/ab_tree.sh <parent checkout> "
                    f"{len(sides['parent']['ms_per_step'])} (interleaved bench.py runs, parent then this tree)",
               **sides, parent_spread_ms=spread, median_difference_ms=diff,
               criterion="this tree's median <= parent's median + parent's spread (max - min)", within_margin=bool(diff <= spread))
    out = json.load(open(out_path)) if os.path.isfile(out_path) else {}
    out["ema_off_vs_parent"] = blk
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(blk))


def kernel_row(name, sizes, decay, chain, reps, rounds, dev):
    """`chain` ema_update launches over buffers of `sizes` elements in one hipGraph, replayed: us per launch and bytes / s."""
    gen = torch.Generator(device=dev).manual_seed(len(sizes))
    ema = [torch.randn(n, generator=gen, device=dev) for n in sizes]
    p = [torch.randn(n, generator=gen, device=dev) for n in sizes]
    state = [torch.tensor([1000.0, 0.0, 0.0, 0.0], device=dev) for _ in sizes]
    fn = lambda: ops.ema_update(ema, p, state, [decay] * len(sizes), [True] * len(sizes))        # noqa: E731
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            fn()
    window_ms(graph.replay, 3)
    ms = [window_ms(graph.replay, reps) / chain for _ in range(rounds)]
    m = statistics.median(ms)
    nbytes = 12 * sum(sizes)
    grid = sum(min(max((n // 4 + 255) // 256, 1), 2048) for n in sizes)
    return {"name": name, "elements": list(sizes), "buffers_per_launch": len(sizes), "workgroups": grid,
            "bytes_read_ema_p_write_ema": nbytes, "launches_per_graph": chain, "graph_replays_per_window": reps,
            "us_per_launch": [x * 1e3 for x in ms], "median_us_per_launch": m * 1e3,
            "achieved_bytes_per_s": nbytes / (m * 1e-3),
            "least_time_us_at_hbm_peak": nbytes / HBM_PEAK * 1e6, "least_time_us_at_measured_stream_rate": nbytes / HBM_STREAM * 1e6,
            "share_of_hbm_peak": nbytes / HBM_PEAK / (m * 1e-3), "share_of_measured_stream_rate": nbytes / HBM_STREAM / (m * 1e-3),
            "fits_infinity_cache": 8 * sum(sizes) < (256 << 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-ab", metavar="DIR", help="only merge tools/ab_tree.sh's bench lines in DIR into --out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args()
    if a.merge_ab:
        return merge_ab(a.merge_ab, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench needs the MI355X: there is nothing to time without it")
    dev, S, B = "cuda", a.size, a.batch
    torch.cuda.set_device(0)

    # ---- (1) the step, interleaved ----
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    trs = {"off": build(S, a.dtype, dev, False, a.decay), "on": build(S, a.dtype, dev, True, a.decay)}
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
    sizes = [o.numel for o in on.ema.optimizers]
    losses_on = on.loss_dict(epoch=60)
    drift = [float((b - o.flat_p).abs().max()) for b, o in zip(on.ema.shadow_bufs, on.ema.optimizers)]
    step = {"config": {"S": S, "B": B, "dtype": a.dtype, "decay": a.decay, "warmup": True,
                       "mode": "train_step_graphed, device-drawn noise", "steps_per_window": a.steps,
                       "rounds": a.rounds, "warmup_steps": a.warmup},
            "averaged_elements": {"encoder": sizes[0], "generator": sizes[1], "total": sum(sizes)},
            "ema_bytes_per_step": 12 * sum(sizes),
            "ms_per_step": windows, "median_ms_per_step": med,
            "off_spread_ms": max(windows["off"]) - min(windows["off"]),
            "on_minus_off_ms": med["on"] - med["off"], "on_over_off": med["on"] / med["off"],
            "kernel_launches_per_step": launches,
            "max_abs_shadow_minus_live_after_timing": drift,
            "finite": all(x == x and abs(x) != float("inf") for x in losses_on.values())}
    print(json.dumps(step), flush=True)
    del trs, on

    # ---- (2) the kernel alone, replayed from a graph ----
    rows = [kernel_row("trainer-sized: the Encoder's and the Generator's buffers in one launch", sizes, a.decay, a.chain,
                       a.reps, a.rounds, dev),
            kernel_row("one buffer of 2^27 elements: past the Infinity Cache", [1 << 27], a.decay, a.chain,
                       max(a.reps // 10, 5), a.rounds, dev)]
    for r in rows:
        print(json.dumps(r), flush=True)
    out = {"what": "weight averaging: interleaved A/B of the graphed step with the EMA off / on (same build), and the update "
                   "kernel alone, replayed from a graph, against its byte count; tools/ema_bench.py",
           "command": "python tools/ema_bench.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "peaks": {"hbm_bytes_per_s": HBM_PEAK, "measured_stream_bytes_per_s": HBM_STREAM},
           "step": step, "kernel": rows}
    if os.path.isfile(a.out):                                   # keep a merged parent comparison
        prev = json.load(open(a.out))
        if "ema_off_vs_parent" in prev:
            out["ema_off_vs_parent"] = prev["ema_off_vs_parent"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
