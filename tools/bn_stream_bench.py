"""Per-shape timing of the three large-tensor BatchNorm passes of bn_act.hip -- normalise + activation forward
(vg_bn_act_forward), backward column reduce (vg_bn_act_backward_reduce) and backward apply (vg_bn_act_backward_apply) --
on the BatchNorm shapes of the S=64 B=128 step and of S=256 B=32, bf16, each kernel alone in a replayed graph.

The calls of one graph rotate over several tensor sets (about 600 MB in all for the large shapes), so a replay does not
find its operands in the 256 MiB Infinity Cache; every figure is the median of `trials` replays, and `scatter` is their
max - min.  GB/s counts the algorithmic streams (forward 2, reduce 2, apply 3 tensor-sized ones) against the 6.3 TB/s
achievable HBM rate.

    python tools/bn_stream_bench.py --out runs/bn_stream_this.json [--reps 20] [--trials 7] [--only G3]
    python tools/bn_stream_bench.py --compare runs/bn_stream_parent.json runs/bn_stream_this.json --out profiles/bn_stream_shapes.json
"""
import argparse
import json
import os
import sys
from ctypes import byref, c_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
HBM_GBS = 6300.0
# name, rows per group, groups, C, activation
SHAPES = [("G0", 2048, 1, 1024, 1), ("G1", 8192, 1, 512, 1), ("G2", 32768, 1, 256, 1), ("G3", 131072, 1, 128, 1),
          ("D3x2", 2048, 2, 512, 2), ("D3", 2048, 1, 512, 2), ("D2x2", 8192, 2, 256, 2), ("D2", 8192, 1, 256, 2),
          ("D1x2", 32768, 2, 128, 2), ("D1", 32768, 1, 128, 2), ("E1", 25088, 1, 64, 1), ("E2", 4608, 1, 128, 1),
          ("E3", 512, 1, 256, 1),
          # S=256 B=32: the Generator's three widest maps and the Discriminator's first three, real + fake
          ("S256.G3", 32768, 1, 128, 1), ("S256.G4", 131072, 1, 64, 1), ("S256.G5", 524288, 1, 32, 1),
          ("S256.D1x2", 131072, 2, 32, 2), ("S256.D2x2", 32768, 2, 64, 2), ("S256.D3x2", 8192, 2, 128, 2)]
PASSES = {"fwd": 2, "reduce": 2, "apply": 3}


def time_graph(torch, calls, reps, trials):
    """calls: list of closures, used round-robin reps times in one captured graph -> (median us, max - min us) per call."""
    calls[0]()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for i in range(reps):
            calls[i % len(calls)]()
    gr.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(trials):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / reps)
    us.sort()
    return us[len(us) // 2], us[-1] - us[0]


def measure(args):
    sys.path[:0] = [ROOT]
    import torch
    from importlib import import_module
    ops = import_module(PKG + ".ops")
    L = import_module(PKG + "._lib")
    G = import_module(PKG + ".geometry")
    lib = L.load()
    dev = torch.device("cuda", 0)
    rows_out = []
    for name, rpg, groups, C, act in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        rows = rpg * groups
        nbytes = rows * C * 2
        nsets = max(1, min(24, -(-600_000_000 // (3 * nbytes))))
        co = torch.rand(groups, 4, C, device=dev) + 0.5
        coef = torch.rand(groups, 3, C, device=dev)
        partial = torch.empty(2048 * 2 * C, device=dev)
        sets = [(torch.randn(rows, C, device=dev).to(torch.bfloat16), torch.randn(rows, C, device=dev).to(torch.bfloat16),
                 torch.empty(rows, C, device=dev, dtype=torch.bfloat16)) for _ in range(nsets)]
        n = c_int(0)

        def fwd(x, dy, out):
            return lambda: ops.bn_act_forward(x, co, rows, C, act, 0.2, G.BF16, out=out)

        def reduce(x, dy, out):
            return lambda: L.check(lib.vg_bn_act_backward_reduce(
                x.data_ptr(), dy.data_ptr(), co[0, 2].data_ptr(), co[0, 3].data_ptr(), co[0, 0].data_ptr(),
                co[0, 1].data_ptr(), rows, C, act, 0.2, partial.data_ptr(), 2048, byref(n), groups, 4 * C, G.BF16,
                L.stream_ptr()), "vg_bn_act_backward_reduce")

        def apply(x, dy, out):
            return lambda: L.check(lib.vg_bn_act_backward_apply(
                x.data_ptr(), dy.data_ptr(), out.data_ptr(), co[0, 2].data_ptr(), co[0, 3].data_ptr(),
                co[0, 0].data_ptr(), co[0, 1].data_ptr(), coef.data_ptr(), rows, C, act, 0.2, groups, 4 * C, 3 * C,
                G.BF16, L.stream_ptr()), "vg_bn_act_backward_apply")

        rec = dict(name=name, rows_per_group=rpg, groups=groups, C=C, tensor_bytes=nbytes, sets=nsets)
        for key, mk in (("fwd", fwd), ("reduce", reduce), ("apply", apply)):
            us, scatter = time_graph(torch, [mk(*s) for s in sets], max(args.reps, nsets), args.trials)
            rec[key] = dict(us=round(us, 2), scatter_us=round(scatter, 2), gbs=round(PASSES[key] * nbytes / us / 1e3, 1),
                            frac_of_hbm=round(PASSES[key] * nbytes / us / 1e3 / HBM_GBS, 3))
        print(json.dumps(rec), flush=True)
        rows_out.append(rec)
        del sets
        torch.cuda.empty_cache()
    res = dict(tool="tools/bn_stream_bench.py", dtype="bf16", reps=args.reps, trials=args.trials, hbm_ceiling_gbs=HBM_GBS,
               device=torch.cuda.get_device_name(0), shapes=rows_out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def compare(args):
    base, new = (json.load(open(p)) for p in args.compare)
    nb = {s["name"]: s for s in new["shapes"]}
    table, bad = [], []
    for s in base["shapes"]:
        t = nb[s["name"]]
        row = {k: s[k] for k in ("name", "rows_per_group", "groups", "C", "tensor_bytes")}
        for key in PASSES:
            b, a = s[key], t[key]
            noise = max(b["scatter_us"], a["scatter_us"])
            row[key] = dict(parent_us=b["us"], this_us=a["us"], parent_gbs=b["gbs"], this_gbs=a["gbs"],
                            scatter_us=noise, speedup=round(b["us"] / a["us"], 3))
            if a["us"] > b["us"] + noise:
                bad.append(f"{s['name']} {key}: slower than the parent by more than the scatter ({b['us']} -> {a['us']} us)")
            if s["tensor_bytes"] >= 8_000_000 and key != "reduce" and a["us"] >= b["us"]:
                bad.append(f"{s['name']} {key}: a shape of >= 8 MB that is not faster ({b['us']} -> {a['us']} us)")
        table.append(row)
        print(row["name"], *(f"{k} {row[k]['parent_us']:.1f}->{row[k]['this_us']:.1f} us ({row[k]['this_gbs']:.0f} GB/s)"
                             for k in PASSES))
    res = dict(tool="tools/bn_stream_bench.py", dtype="bf16", hbm_ceiling_gbs=HBM_GBS, device=new.get("device"),
               reps=new["reps"], trials=new["trials"], shapes=table, violations=bad)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("violations:", bad if bad else "none")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--only")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "THIS"))
    a = ap.parse_args()
    compare(a) if a.compare else measure(a)
