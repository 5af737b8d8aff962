"""Tiled denoising: the two kernels against their byte counts, the blend against stock torch, and the split of one call.

  kernels   vg_tile_gather (u8 and f32 source, f32 and bf16 output) and vg_tile_blend, `--chain` launches captured into ONE
            hipGraph and the graph replayed `--reps` times between one event pair, `--rounds` windows: median us per launch.
            Bytes the algorithm needs: gather = source bytes read (every source pixel once: N H W C, 1 B or 4 B each) plus
            T S^2 CP elt written; blend = T S^2 C 4 read plus N C H W 4 written.  Over the time: bytes / s, and the share of
            the HBM peak (8.0 TB/s published) and of the measured streaming rate (6.29 TB/s, MI355X_MICROARCH.md).  The
            gather re-reads overlapping source pixels (about (S / stride)^2 times); those re-reads are cache hits the byte
            count does not include.
  torch     the same blend through stock torch on the same GPU, uniform-stride geometry only (H - S and W - S multiples of
            the stride): F.fold(tiles * w2) * (1 / F.fold(w2)), the normaliser precomputed outside the timed window -- what a
            user would write without this kernel.  Timed eagerly with device events (permute + multiply + fold + multiply).
            Its result is compared with vg_tile_blend's (max abs difference recorded).
  split     one denoise_tiled call at `--size` x `--size`, S = 64, stride 32, bf16 engines, batch 128: device events
            around the gather launches, the two networks (+ reparameterisation and the layout pass), and the blend, summed
            per part over the chunks of one call, `--calls` calls: medians; and the whole call between one event pair.

No threshold: the numbers are recorded, not gated.

    python tools/tiling_bench.py [--size 2048] [--reps 20] [--out profiles/tiling_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch
import torch.nn.functional as F

import vaegan_amd as V

ops, G, T = V.ops, V.geometry, V.tiling
HBM_PEAK, HBM_STREAM = 8.0e12, 6.29e12
S = 64


def window_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def graph_row(name, fn, nbytes, chain, reps, rounds, extra):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            fn()
    window_ms(graph.replay, 3)
    ms = [window_ms(graph.replay, reps) / chain for _ in range(rounds)]
    m = statistics.median(ms)
    row = {"name": name, "bytes_needed": nbytes, "launches_per_graph": chain, "graph_replays_per_window": reps,
           "us_per_launch": [x * 1e3 for x in ms], "median_us_per_launch": m * 1e3, "achieved_bytes_per_s": nbytes / (m * 1e-3),
           "least_time_us_at_hbm_peak": nbytes / HBM_PEAK * 1e6, "share_of_hbm_peak": nbytes / HBM_PEAK / (m * 1e-3),
           "share_of_measured_stream_rate": nbytes / HBM_STREAM / (m * 1e-3)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--stride", type=int, default=32)
    ap.add_argument("--chain", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiling_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiling_bench needs the MI355X: there is nothing to time without it")
    dev, H, W, C, N = "cuda", a.size, a.size, 3, 1
    if (H - S) % a.stride:
        raise SystemExit("tiling_bench: --size - 64 must be a multiple of --stride (the torch route needs a uniform stride)")
    plan = T.tile_plan(H, W, S, a.stride, "hann")
    Tn = N * plan.ny * plan.nx
    gen = torch.Generator(device=dev).manual_seed(1)
    img = torch.rand(N, C, H, W, generator=gen, device=dev) * 2 - 1
    u8 = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, generator=gen, device=dev)
    tiles = torch.rand(Tn, C, S, S, generator=gen, device=dev) * 2 - 1
    out = {"what": "tiled denoising: vg_tile_gather / vg_tile_blend replayed from a graph against their byte counts, the blend "
                   "against stock torch F.fold, and the split of one denoise_tiled call; tools/tiling_bench.py",
           "device": torch.cuda.get_device_name(0), "peaks": {"hbm_published": HBM_PEAK, "hbm_measured_stream": HBM_STREAM},
           "geometry": {"N": N, "C": C, "H": H, "W": W, "S": S, "stride": a.stride, "window": "hann", "tiles": Tn,
                        "cover": [plan.cover_y, plan.cover_x]}}

    # ---- the kernels, replayed from a graph ----
    rows = []
    for src_name, src, src_bytes in (("u8", u8, N * H * W * C), ("f32", img, N * H * W * C * 4)):
        for dt in (G.F32, G.BF16):
            CP = G.padc(C, dt)
            buf = ops.empty_act((Tn, S, S, CP), dt, dev)
            nbytes = src_bytes + Tn * S * S * CP * G.esize(dt)
            rows.append(graph_row(f"gather {src_name} -> {'bf16' if dt == G.BF16 else 'f32'} [T,S,S,{CP}]",
                                  lambda: ops.tile_gather(src, plan, 0, Tn, CP, dt, out=buf), nbytes, a.chain, a.reps, a.rounds,
                                  {"bytes_read_source_once": src_bytes, "bytes_written": nbytes - src_bytes}))
    blended = torch.empty(N, C, H, W, device=dev)
    nbytes = Tn * S * S * C * 4 + N * C * H * W * 4
    rows.append(graph_row("blend f32 tiles -> f32 [N,C,H,W]", lambda: ops.tile_blend(tiles, plan, out=blended), nbytes,
                          a.chain, a.reps, a.rounds, {"bytes_read_tiles": Tn * S * S * C * 4, "bytes_written": N * C * H * W * 4}))
    out["kernels"] = rows

    # ---- the blend through stock torch ----
    w = torch.from_numpy(T.window_weights("hann", S)).to(dev).float()
    w2 = torch.outer(w, w)
    inv = 1.0 / F.fold(w2.reshape(1, S * S, 1).expand(1, S * S, plan.ny * plan.nx), (H, W), S, stride=a.stride)

    def torch_blend():
        cols = (tiles.view(N, plan.ny * plan.nx, C, S, S) * w2).permute(0, 2, 3, 4, 1).reshape(N, C * S * S, plan.ny * plan.nx)
        return F.fold(cols, (H, W), S, stride=a.stride) * inv
    ref = torch_blend()
    window_ms(torch_blend, 3)
    t_ms = [window_ms(torch_blend, a.reps) for _ in range(a.rounds)]
    window_ms(lambda: ops.tile_blend(tiles, plan, out=blended), 3)
    k_ms = [window_ms(lambda: ops.tile_blend(tiles, plan, out=blended), a.reps) for _ in range(a.rounds)]
    out["blend_vs_torch"] = {"torch_route": "F.fold(tiles * w2) * (1 / F.fold(w2)), normaliser precomputed; eager, device events",
                             "torch_ms": t_ms, "torch_median_ms": statistics.median(t_ms),
                             "vg_tile_blend_eager_ms": k_ms, "vg_tile_blend_eager_median_ms": statistics.median(k_ms),
                             "torch_over_kernel": statistics.median(t_ms) / statistics.median(k_ms),
                             "max_abs_difference": float((ref - blended).abs().max())}
    print(json.dumps(out["blend_vs_torch"]), flush=True)
    del ref, inv

    # ---- the split of one denoise_tiled call ----
    V.configure_seed(42)
    e, g = V.Encoder([C, S, S], 100, dtype="bf16"), V.Generator(nz=100, img_size=S, dtype="bf16")
    g.apply(V.weights_init)
    e.to(dev), g.to(dev)
    e.eval(), g.eval()
    dt, L = G.BF16, 100
    CP, ZP = G.padc(C, dt), G.padc(100, dt)
    eps_z = torch.zeros(Tn, L, device=dev)
    for _ in range(2):
        V.denoise_tiled(e, g, img, stride=a.stride, batch=a.batch, sample=False)          # warm: code objects, workspaces
    parts = {"gather": [], "networks": [], "blend": []}
    for _ in range(a.calls):
        ev = []

        def mark():
            ev.append(torch.cuda.Event(enable_timing=True))
            ev[-1].record()
        torch.cuda.synchronize()
        for t0 in range(0, Tn, a.batch):
            b = min(a.batch, Tn - t0)
            mark()
            x = ops.tile_gather(img, plan, t0, b, CP, dt)
            mark()
            mulv, _ = e._engine.forward(x, b, False, keep=False)
            z, _ = ops.reparam_forward(mulv.view(b, -1), eps_z[t0:t0 + b], L, ZP, dt)
            pre, _ = g._engine.forward(z, b, False, keep=False)
            ops.nhwc_to_nchw(pre, C, dt, apply_tanh=True, out=tiles[t0:t0 + b])
        mark()
        ops.tile_blend(tiles, plan, out=blended)
        mark()
        torch.cuda.synchronize()
        gaps = [ev[i].elapsed_time(ev[i + 1]) for i in range(len(ev) - 1)]
        parts["gather"].append(sum(gaps[0:-1:2]))
        parts["networks"].append(sum(gaps[1:-1:2]))
        parts["blend"].append(gaps[-1])
    whole = [window_ms(lambda: V.denoise_tiled(e, g, img, stride=a.stride, batch=a.batch, sample=False), 1) for _ in range(a.calls)]
    med = {k: statistics.median(v) for k, v in parts.items()}
    total = sum(med.values())
    out["denoise_tiled_split"] = {"dtype": "bf16", "batch": a.batch, "chunks": (Tn + a.batch - 1) // a.batch, "calls": a.calls,
                                  "how": "device events between the parts of the call's own launch sequence, eager; per part "
                                         "the sum over the chunks of one call, median over the calls",
                                  "ms": parts, "median_ms": med, "share": {k: v / total for k, v in med.items()},
                                  "whole_call_ms": whole, "whole_call_median_ms": statistics.median(whole),
                                  "pixels_per_s": N * H * W / (statistics.median(whole) * 1e-3)}
    print(json.dumps(out["denoise_tiled_split"]["median_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
