"""What the prior stream (trainer keyword prior_stream) costs, measured on the MI355X in one process:

  (1) the step: S = 64, B = 128, bf16, VAEGANTrainer.train_step_graphed with device-drawn noise (the benchmarked
      configuration), two trainers built from the same seed -- off: prior_stream=False, on: prior_stream=True -- timed
      INTERLEAVED: `--rounds` rounds of (off window, on window), each window `--steps` replayed iterations between one
      device-event pair.  Reported: every window's ms / step, the medians, off's spread (max - min) as the noise of the
      comparison, on / off, and the kernel launches per step of each (vg_launch_count over the eager first call).  Next to
      it the ratio the COUNTS predict: per iteration the Discriminator reads 3 d_iters + 2 batches of B rows instead of
      2 d_iters + 1 (+ the feature pass when that is on), the Generator runs 2 forwards and 2 backwards instead of 1 and 1.
  (2) the three new launches alone (vg_prior_forward, vg_head_backward_g at 3 groups, vg_nhwc_grad_tanh_to_nhwc) at the shapes
      of that step, each captured `--reps` times into ONE hipGraph and replayed (no per-launch host cost in the figure),
      against its own byte count over the HBM peak (8 TB/s, MI355X_MICROARCH.md).  At these sizes the operands fit the
      Infinity Cache, so the figure is not an HBM stream measurement; the JSON says which bound was used.

A measurement path without the GPU fails; everything is recorded, nothing is gated.

    python tools/prior_stream_bench.py [--rounds 5] [--steps 300] [--out profiles/prior_stream_bench.json]"""
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
HBM_PEAK = 8.0e12


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


def graph_of(fn, reps):
    """`reps` back-to-back launches of fn on one stream as one hipGraph."""
    fn()                                                        # eager once: loads the code object
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=500, help="launches per captured graph in part (2)")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_stream_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prior_stream_bench needs the MI355X: there is nothing to time without it")
    dev, S, B = "cuda", a.size, a.batch
    torch.cuda.set_device(0)

    # ---- (1) the step, interleaved ----
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    trs = {"off": build(S, a.dtype, dev), "on": build(S, a.dtype, dev, prior_stream=True)}
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
    tr = trs["on"]
    losses_on = tr.loss_dict(epoch=60)
    di = tr.d_iters
    step = {"config": {"S": S, "B": B, "dtype": a.dtype, "mode": "train_step_graphed, device-drawn noise", "d_iters": di,
                       "steps_per_window": a.steps, "rounds": a.rounds, "warmup_steps": a.warmup,
                       "grouped_3B": bool(tr.group_d_passes and tr.D._engine.can_group(B, 3)),
                       "grouped_2B": bool(tr.group_d_passes and tr.D._engine.can_group(B, 2))},
            "ms_per_step": windows, "median_ms_per_step": med,
            "off_spread_ms": max(windows["off"]) - min(windows["off"]),
            "on_minus_off_ms": med["on"] - med["off"], "on_over_off": med["on"] / med["off"],
            "kernel_launches_per_step": launches,
            "by_counts": {"discriminator_batches_of_B": {"off": 2 * di + 1, "on": 3 * di + 2,
                                                         "ratio": (3 * di + 2) / (2 * di + 1)},
                          "generator_forward_backward_pairs": {"off": 1, "on": 2, "ratio": 2.0},
                          "encoder_passes": {"off": 1, "on": 1, "ratio": 1.0}},
            "g_loss_adv_prior_after_timing": losses_on.get("g_loss_adv_prior"),
            "finite": all(x == x and abs(x) != float("inf") for x in losses_on.values())}
    print(json.dumps(step), flush=True)
    del trs, tr

    # ---- (2) the three new launches, replayed from graphs ----
    dt = G.BF16 if a.dtype == "bf16" else G.F32
    tdt, es = ops.TORCH_DT[dt], G.esize(dt)
    gen = torch.Generator(device=dev).manual_seed(3)
    Ld, ZP, CP, K, C, HW = 100, G.padc(100, dt), G.padc(3, dt), 4 * 4 * 512, 512, 16
    eps = torch.randn(B, Ld, generator=gen, device=dev)
    p = torch.sigmoid(torch.randn(3 * B, generator=gen, device=dev))
    x = torch.randn(3 * B, K, generator=gen, device=dev).to(tdt)
    w = (torch.randn(K, generator=gen, device=dev) * 0.05).to(tdt)
    dw, loss = torch.zeros(C * HW, device=dev), torch.zeros(1, device=dev)
    t = torch.tanh(torch.randn(B, 3, S, S, generator=gen, device=dev))
    add = torch.randn(B, S, S, CP, generator=gen, device=dev).to(tdt)
    cases = [
        ("vg_prior_forward", lambda: ops.prior_forward(eps, B, Ld, ZP, dt), B * Ld * 4 + B * ZP * es,
         "eps read (f32), z written"),
        ("vg_head_backward_g (3 groups, dx and dw)",
         lambda: ops.head_backward_g(p, x, w, B, (0.9, 0.1, 0.1), 1.0, loss, False, dw, False, K, C, HW, dt, True),
         2 * 3 * B * K * es + K * es + K * 4 + 3 * B * 4, "x read, dx written, w read, dw written, p read"),
        ("vg_nhwc_grad_tanh_to_nhwc", lambda: ops.nhwc_grad_tanh_to_nhwc(add, t, CP, dt),
         B * 3 * S * S * 4 + 2 * B * S * S * CP * es, "t read (f32, 3 channels), add read, dx written"),
    ]
    rows = []
    for name, fn, nbytes, what in cases:
        g = graph_of(fn, a.reps)
        window_ms(g.replay, 3)
        ms = [window_ms(g.replay, 4) / a.reps for _ in range(a.rounds)]
        m = statistics.median(ms)
        rows.append({"entry": name, "dtype": a.dtype, "B": B, "bytes": nbytes, "bytes_are": what,
                     "launches_per_graph": a.reps, "ms_per_launch": ms, "median_us_per_launch": m * 1e3,
                     "achieved_bytes_per_s": nbytes / (m * 1e-3), "least_time_us_at_hbm_peak": nbytes / HBM_PEAK * 1e6,
                     "share_of_hbm_peak": nbytes / HBM_PEAK / (m * 1e-3),
                     "bound": "bytes over HBM peak (8 TB/s); operands fit the Infinity Cache at this size"})
        print(json.dumps(rows[-1]), flush=True)
    out = {"what": "prior stream (decoded prior samples as the third Discriminator input): interleaved A/B of the graphed "
                   "step with the stream off / on, and the three new launches replayed from graphs against their byte "
                   "counts; tools/prior_stream_bench.py",
           "command": "python tools/prior_stream_bench.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "peaks": {"hbm_bytes_per_s": HBM_PEAK}, "step": step, "kernels": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
