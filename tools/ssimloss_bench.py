"""What the SSIM reconstruction loss (trainer argument alpha_ssim, losses.SSIMLoss) costs, measured
on the MI355X.  Four modes, each a process of its own (`--mode`), all writing into one JSON (`--out`):

  step    S = 64, B = 128, bf16, VAEGANTrainer.train_step_graphed with device-drawn noise (the benchmarked configuration),
          two trainers built from the same seed -- A: alpha_ssim = 0, B: alpha_ssim = 1 -- timed INTERLEAVED: `--rounds`
          rounds of (A window, B window), each window `--steps` replayed iterations between one device-event pair.
          Reported: every window's ms / step, the medians, A's spread (max - min) as the noise of the comparison, B - A.
  kernel  ops.ssim_loss_forward_backward at (128,3,64,64), (64,3,128,128), (32,3,256,256) against the stock-torch route a
          user would otherwise take -- grouped F.conv2d SSIM (valid convolution = the interior pixels) plus autograd, f32,
          same device, same inputs.  Outputs are compared first (loss and gradient), then both are timed with device
          events around `--reps` eager calls (launch overhead included on both sides).
  trace   `--shape B,C,H,W`: nothing but `--reps` calls of the kernel at one shape, to be run under
          `rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace_BxCxHxW -- python tools/ssimloss_bench.py
          --mode trace --shape B,C,H,W` (a run of its own per shape: the statistics are per kernel name).
  merge   `--trace-dir DIR`: no device; reads the *kernel_stats.csv of every DIR/trace_* and adds the kernel's average
          time, its floor -- the larger of 4 n_pix 4 bytes over the HBM rate and the separable flop count over the f32
          vector peak (peaks: MI355X_MICROARCH.md) -- and which of the two bounds it.

A measurement path without the GPU fails; nothing is gated.

    python tools/ssimloss_bench.py --mode step   [--rounds 5] [--steps 300]
    python tools/ssimloss_bench.py --mode kernel [--reps 300]
    python tools/ssimloss_bench.py --mode merge --trace-dir runs/ssimloss [--ab-dir runs/ab]

`--ab-dir DIR` (merge mode) adds the requirement for alpha_ssim = 0, the step against the PARENT COMMIT: the bench lines that
`OUT=DIR tools/ab_tree.sh <built checkout of the parent> 3` left (interleaved bench.py runs, parent then this tree), with the
criterion: this tree's median <= the parent's median + the parent's own spread (max - min) in that run."""
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
import torch.nn.functional as F
from importlib import import_module

import vaegan_amd as V

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
HBM_PEAK, F32_VECTOR_PEAK = 8.0e12, 157.3e12
SHAPES = [(128, 3, 64, 64), (64, 3, 128, 128), (32, 3, 256, 256)]
# separable algorithm, per pixel of the plane, halo work not counted: the three products u u, v v, u v; five forward maps
# and three derivative maps, each a row and a column pass of 11 multiply-adds; ~40 for S, the derivative maps and the
# final combination
FLOPS_PER_PIXEL = 3 + 5 * 2 * 11 * 2 + 3 * 2 * 11 * 2 + 40
BYTES_PER_PIXEL = 4 * 4                 # a, b and d read once, d written once


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


def images(shape, dev):
    """A smooth picture and the same picture with N(0, 0.1^2) on it, in [-1, 1]."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(B + C + H + W)
    yy = torch.linspace(0, 3.0, H)[:, None] + torch.rand(B, C, 1, 1, generator=g) * 6
    xx = torch.linspace(0, 2.0, W)[None, :] + torch.rand(B, C, 1, 1, generator=g) * 6
    b = 0.8 * torch.sin(yy) * torch.cos(xx)
    a = torch.clamp(b + 0.1 * torch.randn(B, C, H, W, generator=g), -1, 1)
    return a.contiguous().to(dev), b.contiguous().to(dev)


def torch_window(C, dev):
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(k * k) / (2 * 1.5 * 1.5))
    g = g / g.sum()
    return (g[:, None] * g[None, :]).float().expand(C, 1, 11, 11).contiguous().to(dev)


def torch_ssim_loss(a, b, w):
    """The stock-torch route: grouped conv2d without padding (= the interior pixels), f32."""
    C = a.shape[1]
    u, v = (a + 1) * 0.5, (b + 1) * 0.5
    mu, mv = F.conv2d(u, w, groups=C), F.conv2d(v, w, groups=C)
    suu = F.conv2d(u * u, w, groups=C) - mu * mu
    svv = F.conv2d(v * v, w, groups=C) - mv * mv
    suv = F.conv2d(u * v, w, groups=C) - mu * mv
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = ((2 * mu * mv + c1) * (2 * suv + c2)) / ((mu * mu + mv * mv + c1) * (suu + svv + c2))
    return 1.0 - s.mean()


def load_out(path):
    return json.load(open(path)) if os.path.isfile(path) else {}


def save_out(path, out):
    out["what"] = "SSIM reconstruction loss: interleaved A/B of the graphed step with the term off / on; the kernel against " \
                  "the stock-torch conv2d + autograd route; rocprofv3 kernel time against its floor; tools/ssimloss_bench.py"
    out["peaks"] = {"hbm_bytes_per_s": HBM_PEAK, "f32_vector_flops_per_s": F32_VECTOR_PEAK}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


def mode_step(a, dev):
    S, B = a.size, a.batch
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    trs = {"off": build(S, a.dtype, dev), "on": build(S, a.dtype, dev, alpha_ssim=1.0)}
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
    step = {"config": {"S": S, "B": B, "dtype": a.dtype, "alpha_ssim_on": 1.0, "mode": "train_step_graphed, device-drawn noise",
                       "steps_per_window": a.steps, "rounds": a.rounds, "warmup_steps": a.warmup},
            "ms_per_step": windows, "median_ms_per_step": med,
            "off_spread_ms": max(windows["off"]) - min(windows["off"]),
            "on_minus_off_ms": med["on"] - med["off"], "on_over_off": med["on"] / med["off"],
            "kernel_launches_per_step": launches, "ssim_loss_after_timing": losses_on.get("ssim_loss"),
            "finite": all(x == x and abs(x) != float("inf") for x in losses_on.values())}
    print(json.dumps(step), flush=True)
    return step


def mode_kernel(a, dev):
    rows = []
    for shape in SHAPES:
        B, C, H, W = shape
        x, y = images(shape, dev)
        w = torch_window(C, dev)
        loss = torch.zeros(1, device=dev)
        d = torch.zeros(shape, device=dev)
        ops.ssim_loss_forward_backward(x, y, 1.0, loss, False, d)
        xt = x.clone().requires_grad_(True)
        lt = torch_ssim_loss(xt, y, w)
        lt.backward()
        gmax = float(xt.grad.abs().max())
        cmp_ = {"loss_hip": float(loss), "loss_torch": float(lt), "grad_max_abs": gmax,
                "grad_max_abs_diff": float((d - xt.grad).abs().max()),
                "grad_max_abs_diff_over_max": float((d - xt.grad).abs().max()) / gmax}
        assert abs(cmp_["loss_hip"] - cmp_["loss_torch"]) <= 1e-4 and cmp_["grad_max_abs_diff_over_max"] <= 1e-2, cmp_

        def hip_call():
            ops.ssim_loss_forward_backward(x, y, 1.0, loss, False, d)

        def torch_call():
            xt.grad = None
            torch_ssim_loss(xt, y, w).backward()

        window_ms(hip_call, 20), window_ms(torch_call, 5)
        hip = [window_ms(hip_call, a.reps) for _ in range(a.rounds)]
        tor = [window_ms(torch_call, max(a.reps // 10, 10)) for _ in range(a.rounds)]
        mh, mt = statistics.median(hip), statistics.median(tor)
        rows.append({"shape": list(shape), "n_pix": B * C * H * W, "outputs_compared_first": cmp_,
                     "hip_ms_per_call": hip, "torch_ms_per_call": tor, "hip_median_us": mh * 1e3, "torch_median_us": mt * 1e3,
                     "torch_over_hip": mt / mh,
                     "note": "device events around eager calls, launch overhead included on both sides; hip = the tile launch + "
                             "the one-wave final sum; torch = five grouped conv2d, the pointwise graph and its autograd backward"})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def mode_trace(a, dev):
    shape = tuple(int(v) for v in a.shape.split(","))
    x, y = images(shape, dev)
    loss, d = torch.zeros(1, device=dev), torch.zeros(shape, device=dev)
    for _ in range(a.reps):
        ops.ssim_loss_forward_backward(x, y, 1.0, loss, False, d)
    torch.cuda.synchronize()
    print("traced", shape, a.reps, "calls; loss", float(loss))


def mode_merge(a):
    rows = []
    for dname in sorted(glob.glob(os.path.join(a.trace_dir, "trace_*"))):
        shape = [int(v) for v in os.path.basename(dname)[len("trace_"):].split("x")]
        files = glob.glob(os.path.join(dname, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit(f"ssimloss_bench --mode merge: no kernel_stats.csv under {dname}")
        stat = {}
        for r in csv.DictReader(open(max(files))):
            for key in ("ssim_loss_tile_kernel", "ssim_loss_final_kernel"):
                if key in r["Name"]:
                    stat[key] = {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]),
                                 "max_ns": float(r["MaxNs"])}
        n_pix = shape[0] * shape[1] * shape[2] * shape[3]
        t_bytes, t_flops = n_pix * BYTES_PER_PIXEL / HBM_PEAK, n_pix * FLOPS_PER_PIXEL / F32_VECTOR_PEAK
        t = stat["ssim_loss_tile_kernel"]["average_ns"] * 1e-9
        rows.append({"shape": shape, "n_pix": n_pix, "rocprofv3_kernel_stats": stat,
                     "floor_us_bytes_over_hbm_peak": t_bytes * 1e6, "floor_us_flops_over_f32_vector_peak": t_flops * 1e6,
                     "flops_per_pixel_separable": FLOPS_PER_PIXEL, "bytes_per_pixel": BYTES_PER_PIXEL,
                     "bound": "flops over the f32 vector peak" if t_flops > t_bytes else "bytes over the HBM rate",
                     "floor_over_kernel_time": max(t_bytes, t_flops) / t,
                     "achieved_flops_per_s": n_pix * FLOPS_PER_PIXEL / t, "achieved_bytes_per_s": n_pix * BYTES_PER_PIXEL / t})
        print(json.dumps(rows[-1]))
    if not rows:
        raise SystemExit(f"ssimloss_bench --mode merge: no trace_* directories in {a.trace_dir}")
    return rows


def merge_ab(ab_dir):
    """The interleaved parent-vs-this-tree bench lines that `OUT=DIR tools/ab_tree.sh <built checkout of the parent> 3` left."""
    sides = {}
    for side in ("parent", "this_tree"):
        files = sorted(f for f in glob.glob(os.path.join(ab_dir, "ab_tree_*_*.json"))
                       if os.path.basename(f).startswith("ab_tree_._") == (side == "this_tree"))
        lines = [json.loads(open(f).read().strip().splitlines()[-1]) for f in files]
        if not lines:
            raise SystemExit(f"ssimloss_bench --ab-dir: no bench lines of the {side} in {ab_dir}")
        sides[side] = {"ms_per_step": [d["ms_per_step"] for d in lines], "images_per_s": [d["value"] for d in lines],
                       "kernel_launches_per_step": sorted({d.get("kernel_launches_per_step") for d in lines} - {None}),
                       "median_ms_per_step": statistics.median(d["ms_per_step"] for d in lines)}
    spread = max(sides["parent"]["ms_per_step"]) - min(sides["parent"]["ms_per_step"])
    diff = sides["this_tree"]["median_ms_per_step"] - sides["parent"]["median_ms_per_step"]
    return dict(what="alpha_ssim = 0 (the default trainer bench.py builds) against the parent commit: tools/ab_tree.sh <parent "
                     "checkout> (bench.py --steps 300 --warmup 30 --full --no-cpu-baseline --no-extra-paths, runs alternate "
                     "parent, this tree; one MI355X, one session)",
                **sides, parent_spread_ms=spread, median_difference_ms=diff,
                criterion="this tree's median <= parent's median + parent's spread (max - min)", within_margin=bool(diff <= spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "kernel", "trace", "merge"), required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--shape", default="128,3,64,64")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "runs", "ssimloss"))
    ap.add_argument("--ab-dir", help="with --mode merge: also merge tools/ab_tree.sh's bench lines in this directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssimloss_bench.json"))
    a = ap.parse_args()
    if a.mode == "merge":
        out = load_out(a.out)
        out["kernel_trace"] = mode_merge(a)
        if a.ab_dir:
            out["alpha_ssim_0_vs_parent"] = merge_ab(a.ab_dir)
            print(json.dumps(out["alpha_ssim_0_vs_parent"]))
        return save_out(a.out, out)
    if not torch.cuda.is_available():
        raise SystemExit("ssimloss_bench needs the MI355X: there is nothing to time without it")
    dev = "cuda"
    torch.cuda.set_device(0)
    if a.mode == "trace":
        return mode_trace(a, dev)
    out = load_out(a.out)
    out["device"] = torch.cuda.get_device_name(0)
    if a.mode == "step":
        out["step"] = mode_step(a, dev)
    else:
        out["kernel_vs_torch"] = mode_kernel(a, dev)
    save_out(a.out, out)


if __name__ == "__main__":
    main()
