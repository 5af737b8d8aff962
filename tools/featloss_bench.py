"""What the Discriminator-feature reconstruction loss (trainer arguments feat_layer / alpha_feat)
costs, measured on the MI355X in one process:

  (1) the step: S = 64, B = 128, bf16, VAEGANTrainer.train_step_graphed with device-drawn noise (the benchmarked
      configuration), two trainers built from the same seed -- A: alpha_feat = 0, B: alpha_feat = 1 at feat_layer = 2 --
      timed INTERLEAVED: `--rounds` rounds of (A window, B window), each window `--steps` replayed iterations between one
      device-event pair (>= 0.5 s of work per window at the defaults).  Reported: every window's ms / step, the medians,
      A's spread (max - min) as the noise of the comparison, and B - A: the extra Discriminator forward on the real batch
      plus the two feature-loss launches.
  (2) the kernel alone: ops.feat_mse_forward_backward on the activations of that stage ([B, 8, 8, 256] bf16; also stages 1
      and 3 and f32), `--reps` launches per window between one event pair, against its own byte count -- a, b and d are
      read once and d is written once: 4 n esize bytes -- over the HBM peak (8 TB/s, MI355X_MICROARCH.md) and as achieved
      bytes / s.  At these sizes (4 ... 16 MiB of traffic) the operands fit the 256 MiB Infinity Cache, so the figure is not
      an HBM stream measurement; the JSON says which bound was used.

  (3) the requirement for alpha_feat = 0, the step against the PARENT COMMIT: `--merge-ab DIR` reads the bench lines that
      `OUT=DIR tools/ab_tree.sh <built checkout of the parent> 5` left (interleaved bench.py runs, parent then this tree)
      and writes both sets of ms / step into the same JSON with the criterion: this tree's median <= the parent's median +
      the parent's own spread (max - min) in that interleaved run.  No device needed for the merge itself.

A measurement path without the GPU fails; (1) and (2) are recorded, not gated.

    python tools/featloss_bench.py [--rounds 5] [--steps 300] [--out profiles/featloss_bench.json]
    OUT=runs/ab tools/ab_tree.sh <parent checkout> 5 && python tools/featloss_bench.py --merge-ab runs/ab"""
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


def merge_ab(ab_dir, out_path):
    """Add the interleaved parent-vs-this-tree bench lines of tools/ab_tree.sh to the JSON at out_path."""
    import glob
    sides = {}
    for side, pat in (("this_tree", "ab_tree_._*.json"), ("parent", "ab_tree_*_*.json")):
        files = sorted(f for f in glob.glob(os.path.join(ab_dir, pat))
                       if (os.path.basename(f).startswith("ab_tree_._")) == (side == "this_tree"))
        lines = [json.loads(open(f).read().strip().splitlines()[-1]) for f in files]
        if not lines:
            raise SystemExit(f"featloss_bench --merge-ab: no bench lines of the {side} in {ab_dir}")
        sides[side] = {"ms_per_step": [d["ms_per_step"] for d in lines], "images_per_s": [d["value"] for d in lines],
                       "kernel_launches_per_step": sorted({d.get("kernel_launches_per_step") for d in lines} - {None}),
                       "median_ms_per_step": statistics.median(d["ms_per_step"] for d in lines)}
    spread = max(sides["parent"]["ms_per_step"]) - min(sides["parent"]["ms_per_step"])
    diff = sides["this_tree"]["median_ms_per_step"] - sides["parent"]["median_ms_per_step"]
    blk = dict(what="alpha_feat = 0 (the default trainer bench.py builds) against the parent commit: tools/ab_tree.sh <parent "
                    "checkout> 5 (bench.py --steps 300 --warmup 30 --full --no-cpu-baseline --no-extra-paths, runs alternate "
                    "parent, this tree; one MI355X, one session)",
               **sides, parent_spread_ms=spread, median_difference_ms=diff,
               criterion="this tree's median <= parent's median + parent's spread (max - min)", within_margin=bool(diff <= spread))
    out = json.load(open(out_path)) if os.path.isfile(out_path) else {}
    out["alpha_feat_0_vs_parent"] = blk
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(blk))
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-ab", metavar="DIR", help="only merge tools/ab_tree.sh's bench lines in DIR into --out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--layer", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "featloss_bench.json"))
    a = ap.parse_args()
    if a.merge_ab:
        return merge_ab(a.merge_ab, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("featloss_bench needs the MI355X: there is nothing to time without it")
    dev, S, B = "cuda", a.size, a.batch
    torch.cuda.set_device(0)

    # ---- (1) the step, interleaved ----
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    trs = {"off": build(S, a.dtype, dev), "on": build(S, a.dtype, dev, feat_layer=a.layer, alpha_feat=1.0)}
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
    losses_on = trs["on"].loss_dict(epoch=60)
    step = {"config": {"S": S, "B": B, "dtype": a.dtype, "feat_layer": a.layer, "alpha_feat_on": 1.0,
                       "mode": "train_step_graphed, device-drawn noise", "steps_per_window": a.steps,
                       "rounds": a.rounds, "warmup_steps": a.warmup},
            "ms_per_step": windows, "median_ms_per_step": med,
            "off_spread_ms": max(windows["off"]) - min(windows["off"]),
            "on_minus_off_ms": med["on"] - med["off"], "on_over_off": med["on"] / med["off"],
            "kernel_launches_per_step": launches, "feat_loss_after_timing": losses_on.get("feat_loss"),
            "finite": all(x == x and abs(x) != float("inf") for x in losses_on.values())}
    print(json.dumps(step), flush=True)
    del trs

    # ---- (2) the kernel alone ----
    rows = []
    for dtype, l in ((G.BF16, 2), (G.BF16, 1), (G.BF16, 3), (G.F32, 2)):
        shape = (B, 32 >> l, 32 >> l, 64 << l)
        tdt = ops.TORCH_DT[dtype]
        g = torch.Generator(device=dev).manual_seed(l)
        fa, fb = (torch.randn(shape, generator=g, device=dev).to(tdt) for _ in range(2))
        d = torch.zeros(shape, device=dev, dtype=tdt)
        loss = torch.zeros(1, device=dev)
        n = fa.numel()
        fn = lambda: ops.feat_mse_forward_backward(fa, fb, d, 1e-3, loss, False, dtype)      # noqa: E731
        window_ms(fn, 50)
        ms = [window_ms(fn, a.reps) for _ in range(a.rounds)]
        nbytes = 4 * n * G.esize(dtype)
        m = statistics.median(ms)
        rows.append({"dtype": "bf16" if dtype == G.BF16 else "f32", "stage": l, "shape": list(shape), "n": n,
                     "bytes_read_a_b_d_write_d": nbytes, "launches_per_call": 2,
                     "ms_per_call": ms, "median_us_per_call": m * 1e3,
                     "note": "per call = partial-sum + gradient launch and the one-wave final-sum launch, back to back "
                             "on one stream, launch overhead included (eager launches, not a graph)",
                     "achieved_bytes_per_s": nbytes / (m * 1e-3),
                     "least_time_us_at_hbm_peak": nbytes / HBM_PEAK * 1e6,
                     "share_of_hbm_peak": nbytes / HBM_PEAK / (m * 1e-3),
                     "bound": "bytes over HBM peak (8 TB/s); operands fit the Infinity Cache at this size"})
        print(json.dumps(rows[-1]), flush=True)
    out = {"what": "Discriminator-feature reconstruction loss: interleaved A/B of the graphed step with the feature off / on, "
                   "and the feature-loss kernel alone against its byte count; tools/featloss_bench.py",
           "command": "python tools/featloss_bench.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "peaks": {"hbm_bytes_per_s": HBM_PEAK}, "step": step, "kernel": rows}
    if os.path.isfile(a.out):                                   # keep a merged parent comparison
        prev = json.load(open(a.out))
        if "alpha_feat_0_vs_parent" in prev:
            out["alpha_feat_0_vs_parent"] = prev["alpha_feat_0_vs_parent"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
