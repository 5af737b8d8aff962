"""What test-time latent refinement (denoise.LatentRefiner, csrc/refine.hip) costs, measured on the
MI355X with the interleaved method of tools/ssimloss_bench.py, at S = 64, B = 128, bf16 (`--size`, `--batch`, `--dtype`):

  iteration  one refinement iteration REPLAYED from its captured graph against the same iteration launched eagerly, with and
             without the Discriminator term, and -- from the same run, the same networks -- the graphed training step of
             VAEGANTrainer: four routes in interleaved windows (`--rounds` rounds, `--steps` calls per window between one
             device-event pair).  Kernel launches per call are counted by the library (ops.launch_count).  The expectation
             stated next to the result is a COUNT, not a time: an iteration is one G forward and one G data-gradient pass
             (+ one D forward and one D data-gradient pass), no weight gradient, no statistics pass, no optimiser sweep over
             parameters; compare it against the training step of this run.
  kernels    each new kernel replayed from a graph of its own against its byte count over the HBM rate: the eval-mode
             BatchNorm backward on the Generator's largest BatchNorm tensor ([B S S, 64]), the masked per-image MSE on the
             image batch, the latent Adam launch (a few hundred bytes per row: a launch-latency figure, no rate).

A measurement path without the GPU fails; nothing is gated.

    python tools/refine_bench.py [--steps 200] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch
from importlib import import_module

import vaegan_amd as V
from ssimloss_bench import build, window_ms

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
G = import_module(PKG + ".geometry")
capture = import_module(PKG + ".capture")
HBM_PEAK = 8.0e12


def graphed(fn):
    fn()                                                    # sizes the workspace
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def rects_for(B, S, dev):
    r = torch.zeros(B, 8)
    for i in range(B):
        r[i] = torch.tensor([0.5, 0.1, S // 4 + i % 5, S // 3 + i % 7, i % (S // 2), (3 * i) % (S // 2), 0, 0], dtype=torch.float32)
    return r.to(dev)


def mode_iteration(a, dev):
    S, B = a.size, a.batch
    tr = build(S, a.dtype, dev)
    e, g, d = tr.E, tr.G, tr.D
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    rects = rects_for(B, S, dev)
    for _ in range(a.warmup):
        tr.train_step_graphed(real, 60)
    routes, launches, objective = {}, {}, {}
    for name, disc in (("context", None), ("context_adv", d)):
        r = V.LatentRefiner(e, g, disc, steps=a.refine_steps, alpha_adv=0.1 if disc is not None else 0.0)
        out = r.refine(real, rects)                          # captures the iteration; weights as the warm-up steps left them
        objective[name] = {"objective0_mean": float(out["objective0"].mean()), "objective_mean": float(out["objective"].mean())}
        assert bool((out["objective"] <= out["objective0"]).all())
        buf, cap = r._bufs[B], r._caps[B]
        routes[name + "_replay"] = lambda cap=cap: capture.replay(cap)
        routes[name + "_eager"] = lambda r=r, buf=buf: r._iterate(buf, B)
        n0 = ops.launch_count()
        r._iterate(buf, B)
        launches[name] = ops.launch_count() - n0
    n0 = ops.launch_count()
    tr.train_step(real, 60)
    launches["train_step"] = ops.launch_count() - n0
    routes["train_step_graphed"] = lambda: tr.train_step_graphed(real, 60)
    for fn in routes.values():
        window_ms(fn, 10)
    windows = {k: [] for k in routes}
    for _ in range(a.rounds):
        for name, fn in routes.items():
            windows[name].append(window_ms(fn, a.steps))
    med = {k: statistics.median(v) for k, v in windows.items()}
    out = {"config": {"S": S, "B": B, "dtype": a.dtype, "calls_per_window": a.steps, "rounds": a.rounds, "refine_steps": a.refine_steps},
           "ms_per_call": windows, "median_ms_per_call": med,
           "spread_ms": {k: max(v) - min(v) for k, v in windows.items()},
           "replay_over_eager": {n: med[n + "_replay"] / med[n + "_eager"] for n in ("context", "context_adv")},
           "iteration_over_train_step": {n: med[n + "_replay"] / med["train_step_graphed"] for n in ("context", "context_adv")},
           "discriminator_term_ms": med["context_adv_replay"] - med["context_replay"],
           "kernel_launches_per_call": launches, "refine": objective,
           "expectation": "count only: 1 G forward + 1 G data-gradient pass (+ 1 D forward + 1 D data-gradient pass); no weight "
                          "gradients, no statistics passes, no optimiser sweep over parameters -- compare with train_step_graphed "
                          "of this run"}
    print(json.dumps(out), flush=True)
    return out


def mode_kernels(a, dev):
    S, B = a.size, a.batch
    dt = G.BF16 if a.dtype == "bf16" else G.F32
    es = 2 if dt == G.BF16 else 4
    tdt = ops.TORCH_DT[dt]
    rows, C = B * S * S, 64
    gen = torch.Generator().manual_seed(2)
    x, dy = (torch.randn(rows, C, generator=gen).to(tdt).to(dev) for _ in range(2))
    co = torch.randn(1, 4, C, generator=gen).to(dev)
    dx = torch.empty_like(x)
    img_a, img_b = ((torch.rand(B, 3, S, S, generator=gen) * 2 - 1).to(dev) for _ in range(2))
    rects, loss_rows, d_a = rects_for(B, S, dev), torch.empty(B, device=dev), torch.empty(B, 3, S, S, device=dev)
    L_dim, ZP = 100, G.padc(100, dt)
    st = ops.latent_state(B, L_dim, dev)
    z_eng = torch.randn(B, ZP, generator=gen).to(tdt).to(dev)
    dz = torch.randn(B, ZP, generator=gen).to(tdt).to(dev)
    ops.latent_adam("init", st, dt, ZP, z_in=z_eng.clone(), z_out=z_eng)
    calls = {
        "bn_act_backward_eval": (lambda: ops.bn_act_backward_eval(x, dy, co, rows, C, 1, 0.0, dt, out=dx), 3 * rows * C * es),
        "masked_mse_rows": (lambda: ops.masked_mse_rows(img_a, img_b, rects, 1.0, loss_rows, True, out=d_a), 12 * img_a.numel()),
        "latent_adam": (lambda: ops.latent_adam("update", st, dt, ZP, dz=dz, loss_rows=loss_rows, z_out=z_eng, lr=0.05),
                        B * (L_dim * 4 * 7 + 2 * ZP * es)),
    }
    out = {}
    for name, (fn, nbytes) in calls.items():
        rep = graphed(fn)
        window_ms(rep, 20)
        t = [window_ms(rep, a.steps) * 1e3 for _ in range(a.rounds)]
        med = statistics.median(t)
        out[name] = {"bytes": nbytes, "us_per_replay": t, "median_us": med, "floor_us_at_hbm_peak": nbytes / HBM_PEAK * 1e6,
                     "fraction_of_hbm_peak": nbytes / (med * 1e-6) / HBM_PEAK}
    out["shapes"] = {"bn_act_backward_eval": [rows, C], "masked_mse_rows": [B, 3, S, S], "latent_adam": [B, L_dim, ZP]}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--refine-steps", type=int, default=20)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refine_bench needs the MI355X: there is nothing to time without it")
    dev = "cuda"
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0),
           "what": "test-time latent refinement: one iteration replayed from its graph against eager, with and without the "
                   "Discriminator term, against the graphed training step of the same run; each new kernel replayed against its "
                   "byte count; tools/refine_bench.py",
           "peaks": {"hbm_bytes_per_s": HBM_PEAK}}
    out["kernels"] = mode_kernels(a, dev)
    out["iteration"] = mode_iteration(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
