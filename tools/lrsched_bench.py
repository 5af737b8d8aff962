"""What a learning-rate schedule and decoupled weight decay (vaegan_amd.LRSchedule, vaegan_amd.AdamW)
cost, measured on the MI355X in one process:

  (1) the step: S = 64, B = 128, bf16, VAEGANTrainer.train_step_graphed with device-drawn noise (the benchmarked
      configuration), three trainers of the SAME build from the same seed --
        plain:  Adam without a schedule on all three networks (what bench.py times),
        sched:  Adam with a warm-up + cosine schedule on all three,
        adamw:  AdamW (weight_decay 0.01, the same schedule) on all three --
      timed INTERLEAVED: `--rounds` rounds of (plain window, sched window, adamw window), each window `--steps` replayed
      iterations between one device-event pair.  Reported: every window's ms / step, the medians, the plain trainer's spread
      (max - min) as the noise of the comparison, and each arm minus plain.  The kernel launches per iteration
      (ops.launch_count over the eager first step) must be EQUAL in the three arms -- the schedule rides in the prologue launch,
      the decay in the update launch -- and every arm must have captured exactly once while its rate moved: both asserted.
  (2) the update alone: vg_adamw_apply (ops.adam_apply_clip over two AdamW-like optimizers) against vg_adam_apply2 over buffers
      of the Encoder's and the Generator's sizes, `--chain` calls captured into ONE hipGraph and the graph replayed `--reps`
      times between one event pair, against their byte count -- 28 bytes per element: p, g, m, v read, p, m, v written -- over
      the HBM peak (8 TB/s, MI355X_MICROARCH.md) and over the measured streaming rate (6.3 TB/s).  Both kernels run over
      the SAME buffers, their windows interleaved.  One row has the trainer's sizes (383 MB per call), a second two buffers of
      2^25 elements (1.9 GB per call); neither fits the 256 MiB Infinity Cache.

A measurement path without the GPU fails; everything is recorded, nothing is gated on a time.

    python tools/lrsched_bench.py [--rounds 5] [--steps 300] [--out profiles/lrsched_bench.json]"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch
from importlib import import_module

import vaegan_amd as V

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12
ARMS = ("plain", "sched", "adamw")


def build(S, dtype, dev, arm, steps_total):
    V.configure_seed(42)
    e, g, d = V.Encoder([3, S, S], 100, dtype=dtype), V.Generator(nz=100, img_size=S, dtype=dtype), \
        V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init), d.apply(V.weights_init)
    e.to(dev), g.to(dev), d.to(dev)

    def opt(m, hold):
        # warm-up over a tenth of the run, cosine to a hundredth of the rate over the rest: the rate moves at every step
        sched = V.LRSchedule(warmup=steps_total // 10, warmup_start=0.01, decay="cosine", decay_steps=steps_total, final=0.01,
                             hold=hold)
        if arm == "plain":
            return V.Adam(m.parameters(), lr=2e-4)
        if arm == "sched":
            return V.Adam(m.parameters(), lr=2e-4, lr_schedule=sched)
        return V.AdamW(m.parameters(), lr=2e-4, weight_decay=0.01, lr_schedule=sched)

    tr = V.VAEGANTrainer(e, g, d, opt(e, 1), opt(g, 1), opt(d, 2))
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


def fake_opts(sizes, dev):
    """What ops.adam_apply2 / ops.adam_apply_clip read of an optimizer, prepared as after three steps: -> (plain, decoupled),
    two views of the SAME buffers, so that the two kernels are timed over the same addresses."""
    gen = torch.Generator(device=dev).manual_seed(len(sizes))
    plain = [SimpleNamespace(flat_p=torch.randn(n, generator=gen, device=dev), flat_g=torch.randn(n, generator=gen, device=dev),
                             exp_avg=torch.zeros(n, device=dev), exp_avg_sq=torch.zeros(n, device=dev),
                             state_dev=torch.tensor([3.0, 2.2857143e-4, 0.05474375, 0.999998], device=dev), betas=(0.5, 0.999),
                             eps=1e-8, grad_scale=1.0, _DECOUPLED=False) for n in sizes]
    return plain, [SimpleNamespace(**{**vars(o), "_DECOUPLED": True}) for o in plain]


def kernel_rows(name, sizes, chain, reps, rounds, dev):
    """`chain` update calls over two buffers of `sizes` elements in one hipGraph, replayed; the two kernels interleaved."""
    fns = {}
    plain, decoupled = fake_opts(sizes, dev)
    for which in ("vg_adam_apply2", "vg_adamw_apply"):
        a, b = plain if which == "vg_adam_apply2" else decoupled
        fn = (lambda a=a, b=b: ops.adam_apply2(a, b)) if which == "vg_adam_apply2" else \
            (lambda a=a, b=b: ops.adam_apply_clip([a, b], [None, None]))
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(chain):
                fn()
        window_ms(graph.replay, 3)
        fns[which] = (graph, (a, b))
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (graph, _) in fns.items():
            ms[k].append(window_ms(graph.replay, reps) / chain)
    nbytes = 28 * sum(sizes)
    rows = []
    for k, v in ms.items():
        m = statistics.median(v)
        rows.append({"name": name, "entry_point": k, "elements": list(sizes), "bytes_moved": nbytes, "calls_per_graph": chain,
                     "graph_replays_per_window": reps, "us_per_call": [x * 1e3 for x in v], "median_us_per_call": m * 1e3,
                     "spread_us": (max(v) - min(v)) * 1e3, "achieved_bytes_per_s": nbytes / (m * 1e-3),
                     "least_time_us_at_hbm_peak": nbytes / HBM_PEAK * 1e6,
                     "least_time_us_at_measured_stream_rate": nbytes / HBM_STREAM * 1e6,
                     "share_of_hbm_peak": nbytes / HBM_PEAK / (m * 1e-3),
                     "share_of_measured_stream_rate": nbytes / HBM_STREAM / (m * 1e-3),
                     "fits_infinity_cache": nbytes < (256 << 20),
                     "finite": all(bool(torch.isfinite(o.flat_p).all()) for o in fns[k][1])})
    return rows


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lrsched_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lrsched_bench needs the MI355X: there is nothing to time without it")
    dev, S, B = "cuda", a.size, a.batch
    torch.cuda.set_device(0)

    # ---- (1) the step, interleaved ----
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    total = 1 + a.warmup + a.rounds * a.steps
    trs = {arm: build(S, a.dtype, dev, arm, total) for arm in ARMS}
    launches, graphs = {}, {}
    for arm, tr in trs.items():
        n0 = ops.launch_count()
        tr.train_step_graphed(real, 60)                         # eager: sizes the workspaces, counts the launches
        launches[arm] = ops.launch_count() - n0
        for _ in range(a.warmup):
            tr.train_step_graphed(real, 60)                     # capture + replays
        assert tr._graph is not None and len(tr._graph[1]) == 1
        graphs[arm] = tr._graph
    assert len(set(launches.values())) == 1, f"the arms differ in kernel launches per iteration: {launches}"
    windows = {arm: [] for arm in ARMS}
    for _ in range(a.rounds):
        for arm, tr in trs.items():
            windows[arm].append(window_ms(lambda: tr.train_step_graphed(real, 60), a.steps))
    for arm, tr in trs.items():
        assert tr._graph is graphs[arm], f"{arm}: the iteration was captured again while the rate moved"
    med = {k: statistics.median(v) for k, v in windows.items()}
    reports = {arm: tr.loss_dict(epoch=60) for arm, tr in trs.items()}
    step = {"config": {"S": S, "B": B, "dtype": a.dtype, "mode": "train_step_graphed, device-drawn noise",
                       "schedule": trs["sched"].opt_E.lr_schedule.state_dict(), "weight_decay_of_the_adamw_arm": 0.01,
                       "steps_per_window": a.steps, "rounds": a.rounds, "warmup_steps": a.warmup},
            "ms_per_step": windows, "median_ms_per_step": med,
            "plain_spread_ms": max(windows["plain"]) - min(windows["plain"]),
            "spread_ms": {k: max(v) - min(v) for k, v in windows.items()},
            "sched_minus_plain_ms": med["sched"] - med["plain"], "adamw_minus_plain_ms": med["adamw"] - med["plain"],
            "kernel_launches_per_step": launches,
            "optimizer_steps": {arm: [tr.opt_E.steps, tr.opt_G.steps, tr.opt_D.steps] for arm, tr in trs.items()},
            "rates_of_the_last_step": {arm: {k: v for k, v in r.items() if k.startswith("lr_")} for arm, r in reports.items()},
            "finite": all(x == x and abs(x) != float("inf") for r in reports.values() for x in r.values())}
    print(json.dumps(step), flush=True)
    sizes = [trs["plain"].opt_E.numel, trs["plain"].opt_G.numel]
    del trs, graphs

    # ---- (2) the update alone, replayed from a graph ----
    rows = kernel_rows("trainer-sized: the Encoder's and the Generator's buffers in one launch", sizes, a.chain, a.reps,
                       a.rounds, dev)
    rows += kernel_rows("two buffers of 2^25 elements: past the Infinity Cache", [1 << 25, 1 << 25], max(a.chain // 4, 2),
                        max(a.reps // 10, 5), a.rounds, dev)
    for r in rows:
        print(json.dumps(r), flush=True)
    out = {"what": "learning-rate schedules and AdamW: interleaved A/B/C of the graphed step (plain Adam / scheduled Adam / "
                   "scheduled AdamW, same build), and vg_adamw_apply against vg_adam_apply2, replayed from a graph, against their "
                   "byte count; tools/lrsched_bench.py",
           "command": "python tools/lrsched_bench.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "peaks": {"hbm_bytes_per_s": HBM_PEAK, "measured_stream_bytes_per_s": HBM_STREAM},
           "step": step, "kernel": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
