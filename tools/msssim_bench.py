"""What the multi-scale SSIM loss (ops.msssim_loss_forward_backward, losses.MSSSIMLoss, the trainers' ssim_scales; DESIGN.md
section 4.4p) costs, measured on the MI355X with the interleaved method of tools/ssimloss_bench.py.  Two modes, each a
process of its own (`--mode`), both writing into one JSON (`--out`):

  kernel  (128,3,64,64) M = 3, (64,3,128,128) M = 4, (32,3,256,256) M = 5, forward + backward, each call REPLAYED FROM A
          GRAPH.  Three routes timed in interleaved windows (`--rounds` rounds of one window each, `--reps` replays per
          window between one device-event pair): the single-scale vg_ssim_loss_forward_backward at the same shape, the
          multi-scale entry point, and the stock-torch route a user would otherwise take (F.avg_pool2d + grouped F.conv2d +
          autograd, f32, eager -- its launch overhead is part of what it costs).  Outputs are compared first.  Reported next
          to the measured multi / single ratio: the predicted one -- the pyramid's pixel count (<= 4/3 of the base) times two
          (the maps are computed in the forward AND in the backward launch) plus the pyramid and collapse passes at their
          byte counts over the HBM rate.  Also the summed kernel time of the launches of one eager call
          (vg_timing_collect, family 5).
  step    S = 64, B = 128, bf16, VAEGANTrainer.train_step_graphed with device-drawn noise: three trainers from one seed --
          alpha_ssim off / single-scale / multi-scale (default scales) -- timed interleaved as ssimloss_bench's step mode.

A measurement path without the GPU fails; nothing is gated.  bench.py's headline against the parent commit:
tools/ab_tree.sh (the default path launches what it launched: any difference beyond the parent's own spread is a defect).

    python tools/msssim_bench.py --mode kernel [--reps 200] [--rounds 5]
    python tools/msssim_bench.py --mode step   [--steps 300] [--rounds 5]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch
import torch.nn.functional as F
from importlib import import_module

import vaegan_amd as V
from ssimloss_bench import build, images, load_out, torch_window, window_ms

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
L = import_module(PKG + "._lib")
HBM_PEAK = 8.0e12
SHAPES = [(128, 3, 64, 64), (64, 3, 128, 128), (32, 3, 256, 256)]


def torch_msssim_loss(a, b, w, weights):
    """The stock-torch route: avg_pool2d pyramid, grouped conv2d without padding per level, the clamp rule; f32."""
    C, M = a.shape[1], len(weights)
    means = []
    for j in range(M):
        u, v = (a + 1) * 0.5, (b + 1) * 0.5
        mu, mv = F.conv2d(u, w, groups=C), F.conv2d(v, w, groups=C)
        suu = F.conv2d(u * u, w, groups=C) - mu * mu
        svv = F.conv2d(v * v, w, groups=C) - mv * mv
        suv = F.conv2d(u * v, w, groups=C) - mu * mv
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        m = (2 * suv + c2) / (suu + svv + c2)
        if j == M - 1:
            m = m * (2 * mu * mv + c1) / (mu * mu + mv * mv + c1)
        means.append(m.mean(dim=(1, 2, 3)))
        if j < M - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    m = torch.stack(means, dim=1)
    ok = (m > 0).all(dim=1)
    safe = torch.where(ok[:, None], m, torch.ones_like(m))
    P = torch.where(ok, (safe ** torch.tensor(weights, device=a.device)).prod(dim=1), torch.zeros_like(safe[:, 0]))
    return 1.0 - P.mean()


def graphed(fn):
    fn()                                                    # sizes the workspace
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def mode_kernel(a, dev):
    rows = []
    lib = L.load()
    for shape in SHAPES:
        B, C, H, W = shape
        weights = V.msssim_weights(H, W)
        M = len(weights)
        x, y = images(shape, dev)
        w = torch_window(C, dev)
        loss, loss1 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        d, d1 = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
        ops.msssim_loss_forward_backward(x, y, weights, 1.0, loss, False, d)
        xt = x.clone().requires_grad_(True)
        lt = torch_msssim_loss(xt, y, w, weights)
        lt.backward()
        gmax = float(xt.grad.abs().max())
        cmp_ = {"loss_hip": float(loss), "loss_torch": float(lt), "grad_max_abs": gmax,
                "grad_max_abs_diff_over_max": float((d - xt.grad).abs().max()) / gmax}
        assert abs(cmp_["loss_hip"] - cmp_["loss_torch"]) <= 1e-4 and cmp_["grad_max_abs_diff_over_max"] <= 1e-2, cmp_

        # the summed kernel time of one eager call's launches
        ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
        lib.vg_timing_enable(1)
        for _ in range(20):
            ops.msssim_loss_forward_backward(x, y, weights, 1.0, loss, False, d)
        lib.vg_timing_collect(5, ctypes.byref(ms), ctypes.byref(n))
        lib.vg_timing_enable(0)
        kernel_sum_us, launches = ms.value * 1e3 / 20, n.value // 20

        multi = graphed(lambda: ops.msssim_loss_forward_backward(x, y, weights, 1.0, loss, False, d))
        single = graphed(lambda: ops.ssim_loss_forward_backward(x, y, 1.0, loss1, False, d1))

        def torch_call():
            xt.grad = None
            torch_msssim_loss(xt, y, w, weights).backward()

        window_ms(multi, 20), window_ms(single, 20), window_ms(torch_call, 3)
        t = {"single": [], "multi": [], "torch": []}
        for _ in range(a.rounds):
            t["single"].append(window_ms(single, a.reps))
            t["multi"].append(window_ms(multi, a.reps))
            t["torch"].append(window_ms(torch_call, max(a.reps // 20, 5)))
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        n0 = B * C * H * W
        nj = [B * C * (H >> j) * (W >> j) for j in range(M)]
        # pyramid: reads a and b, writes their levels >= 1; collapse: reads the gradient pyramid and d, writes d; the
        # backward launch WRITES the gradient pyramid where the single-scale kernel read-modify-writes d (counted there)
        extra_bytes = 4 * (2 * n0 + 2 * sum(nj[1:])) + 4 * (sum(nj) + 2 * n0)
        predicted = 2 * sum(nj) / n0 + extra_bytes / HBM_PEAK * 1e6 / med["single"]
        rows.append({"shape": list(shape), "scales": M, "launches_per_call": launches, "outputs_compared_first": cmp_,
                     "us_per_call": {k: [v * 1e3 for v in vs] for k, vs in t.items()}, "median_us": med,
                     "single_spread_us": (max(t["single"]) - min(t["single"])) * 1e3,
                     "multi_over_single": med["multi"] / med["single"], "predicted_multi_over_single": predicted,
                     "pixel_ratio": sum(nj) / n0,
                     "tile_ratio": sum(-(-(H >> j) // 32) * -(-(W >> j) // 32) for j in range(M)) / (-(-H // 32) * -(-W // 32)), "pyramid_and_collapse_bytes": extra_bytes,
                     "pyramid_and_collapse_floor_us": extra_bytes / HBM_PEAK * 1e6,
                     "torch_over_multi": med["torch"] / med["multi"], "eager_kernel_time_sum_us": kernel_sum_us,
                     "note": "single, multi: one graph replay per call; torch: eager avg_pool2d + grouped conv2d + autograd"})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def mode_step(a, dev):
    S, B = a.size, a.batch
    real = (torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    trs = {"off": build(S, a.dtype, dev), "single": build(S, a.dtype, dev, alpha_ssim=1.0),
           "multi": build(S, a.dtype, dev, alpha_ssim=1.0, ssim_scales=True)}
    launches = {}
    for name, tr in trs.items():
        n0 = ops.launch_count()
        tr.train_step_graphed(real, 60)
        launches[name] = ops.launch_count() - n0
        for _ in range(a.warmup):
            tr.train_step_graphed(real, 60)
        assert tr._graph is not None and len(tr._graph[1]) == 1
    windows = {k: [] for k in trs}
    for _ in range(a.rounds):
        for name, tr in trs.items():
            windows[name].append(window_ms(lambda: tr.train_step_graphed(real, 60), a.steps))
    med = {k: statistics.median(v) for k, v in windows.items()}
    losses = {k: tr.loss_dict(epoch=60).get("ssim_loss") for k, tr in trs.items()}
    step = {"config": {"S": S, "B": B, "dtype": a.dtype, "alpha_ssim_on": 1.0, "scales": len(V.msssim_weights(S, S)),
                       "mode": "train_step_graphed, device-drawn noise", "steps_per_window": a.steps, "rounds": a.rounds,
                       "warmup_steps": a.warmup},
            "ms_per_step": windows, "median_ms_per_step": med, "off_spread_ms": max(windows["off"]) - min(windows["off"]),
            "single_minus_off_ms": med["single"] - med["off"], "multi_minus_off_ms": med["multi"] - med["off"],
            "multi_minus_single_ms": med["multi"] - med["single"], "kernel_launches_per_step": launches,
            "ssim_loss_after_timing": losses}
    print(json.dumps(step), flush=True)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernel", "step"), required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_bench needs the MI355X: there is nothing to time without it")
    dev = "cuda"
    torch.cuda.set_device(0)
    out = load_out(a.out)
    out["device"] = torch.cuda.get_device_name(0)
    out["what"] = "multi-scale SSIM loss: the graph-replayed kernel chain against the single-scale kernel (measured and " \
                  "predicted ratio) and against the stock-torch route; interleaved A/B/C of the graphed step with the term " \
                  "off / single-scale / multi-scale; tools/msssim_bench.py"
    out["step" if a.mode == "step" else "kernel"] = (mode_step if a.mode == "step" else mode_kernel)(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
