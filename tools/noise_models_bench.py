"""What the noise models of the degraded pairs and the median baseline cost, measured on the MI355X at
S = 64, B = 128, C = 3 with the interleaved method of tools/ssimloss_bench.py: every candidate is captured into a graph of its own
(CALLS back-to-back launches, so the replay overhead is shared), the graphs are replayed in interleaved windows, and the figure is
the median over the rounds of the time per launch.

  gather   the old entry (vg_gather_degrade_u8: rectangle, bf16 NHWC copy on) and vg_gather_degrade_u8_ex at each kind without and
           with impulses, each beside its algorithmic byte count B*H*W*(C + 8C + 2*CP) -- u8 read, two f32 writes, bf16 NHWC write;
           the models add arithmetic and Philox blocks, no bytes.
  median   vg_median_filter at r = 1 and r = 2 against its byte count (one f32 read, one f32 write per element) and against a
           stock-torch route on the same GPU (reflect pad, unfold twice, median over the window), whose result must equal the
           kernel's.
  ab       --parent-lib LIB [--parent-copy LIB2]: the OLD entry of this tree's library against the same entry of a library built
           from the parent commit, loaded side by side in this one process and replayed in interleaved windows; LIB2, a byte copy
           of LIB, is the A/A leg that sizes the noise on the same box in the same run.  Per round i: r_i = new_i / parent_i and
           a_i = copy_i / parent_i.  ratio = median(r_i); spread = max |a_i - 1|.  The templating leaked into the default path if
           ratio > 1 + 2 * spread.  (tools/ab_tree.sh runs bench.py in two checkouts; bench.py never launches this kernel, so the
           entry is timed here, with that script's interleaving, in one process.)

A measurement path without the GPU fails; nothing is gated.

    python tools/noise_models_bench.py [--steps 200] [--rounds 7] [--parent-lib LIB --parent-copy LIB2] [--commit <text>]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch
import torch.nn.functional as F
from importlib import import_module

from ssimloss_bench import window_ms

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
data = import_module(PKG + ".data")
G = import_module(PKG + ".geometry")
L = import_module(PKG + "._lib")
HBM_PEAK = 8.0e12
S, B, C, CP, N = 64, 128, 3, 8, 512
CALLS = 8                                           # launches per captured graph


def graphed(fn):
    fn()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    return g.replay


def interleaved(routes, steps, rounds):
    """{name: [us per launch, one per round]}: every round visits every route once, in order."""
    for rep in routes.values():
        window_ms(rep, 3)
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, rep in routes.items():
            t[k].append(window_ms(rep, steps) * 1e3 / CALLS)
    return t


def summary(ts, nbytes=None):
    med = statistics.median(ts)
    row = {"us_per_launch": [round(v, 3) for v in ts], "median_us": round(med, 3), "spread_us": round(max(ts) - min(ts), 3)}
    if nbytes is not None:
        row.update(bytes=nbytes, GBps=round(nbytes / med / 1e3, 1), fraction_of_hbm_peak=round(nbytes / (med * 1e-6) / HBM_PEAK, 4))
    return row


def gather_inputs(dev):
    gen = torch.Generator().manual_seed(S)
    images = torch.randint(0, 256, (N, S, S, C), dtype=torch.uint8, generator=gen).to(dev)
    idx = torch.randperm(N, generator=gen)[:B].to(dev)
    out = dict(clean=torch.empty(B, C, S, S, device=dev), noisy=torch.empty(B, C, S, S, device=dev),
               nhwc=ops.empty_act((B, S, S, CP), G.BF16, dev))
    return images, idx, out


def mode_gather(a, dev):
    images, idx, o = gather_inputs(dev)
    bounds = data.degrade_bounds(S, S)
    nbytes = B * S * S * (C + 8 * C + 2 * CP)

    def call(**kw):
        return lambda: ops.gather_degrade_u8(images, idx, 99, 0, 0.25, True, True, bounds, out_clean=o["clean"],
                                             out_noisy=o["noisy"], nhwc=o["nhwc"], **kw)
    routes = {"old_entry": graphed(call())}
    for kind in ("gaussian", "speckle", "shot"):
        for p in (0.0, 0.1):
            if kind == "gaussian" and p == 0.0:
                continue                                                 # that model IS the old entry (ops routes it there)
            routes[f"ex_{kind}_p{p}"] = graphed(call(kind=kind, impulse_max_p=p, salt_ratio=0.5))
    t = interleaved(routes, a.steps, a.rounds)
    rows = {k: summary(v, nbytes) for k, v in t.items()}
    base = rows["old_entry"]["median_us"]
    for k, r in rows.items():
        r["over_old_entry"] = round(r["median_us"] / base, 3)
        print(k, json.dumps(r), flush=True)
    return rows


def torch_median(x, r):
    k = 2 * r + 1
    xp = F.pad(x, (r,) * 4, mode="reflect")
    w = xp.unfold(2, k, 1).unfold(3, k, 1)                               # [B, C, H, W, k, k]
    return w.reshape(*x.shape, k * k).median(dim=-1).values


def mode_median(a, dev):
    gen = torch.Generator().manual_seed(7)
    x = (torch.rand(B, C, S, S, generator=gen) * 2 - 1).to(dev)
    y = torch.empty_like(x)
    nbytes = 2 * 4 * x.numel()
    rows = {}
    for r in (1, 2):
        rep = graphed(lambda: ops.median_filter(x, r, out=y))
        t = interleaved({"kernel": rep}, a.steps, a.rounds)["kernel"]
        row = summary(t, nbytes)
        ref = torch_median(x, r)
        tt = [window_ms(lambda: torch_median(x, r), 5) * 1e3 for _ in range(3)]
        row.update(torch_route_us=[round(v, 1) for v in tt], torch_over_kernel=round(min(tt) / row["median_us"], 1),
                   equals_torch_route=bool(torch.equal(y, ref)))
        rows[f"r{r}"] = row
        print("median r", r, json.dumps(row), flush=True)
    return rows


def old_entry_of(path):
    """The old gather entry of the library at `path`, bound with this tree's signature (the parent's is the same)."""
    lib = ctypes.CDLL(path)
    fn = lib.vg_gather_degrade_u8
    fn.restype, fn.argtypes = L.SIGNATURES["vg_gather_degrade_u8"]
    return fn


def mode_ab(a, dev):
    images, idx, o = gather_inputs(dev)
    bounds = data.degrade_bounds(S, S)
    libs = {"parent": a.parent_lib, "parent_copy": a.parent_copy, "new": L.LIB_PATH}
    for k, p in libs.items():
        if not os.path.isfile(p):
            raise SystemExit(f"ab: no library at {p} ({k})")
    if os.path.samefile(libs["parent"], libs["parent_copy"]):
        raise SystemExit("ab: --parent-copy must be a byte COPY of --parent-lib at another path (the loader shares one file)")
    routes, outs = {}, {}
    for k, p in libs.items():
        fn = old_entry_of(p)

        def call(fn=fn):
            rc = fn(images.data_ptr(), N, idx.data_ptr(), B, C, S, S, 99, 0, 0.25, 1, 1, *bounds, o["clean"].data_ptr(),
                    o["noisy"].data_ptr(), o["nhwc"].data_ptr(), CP, G.BF16, L.stream_ptr())
            if rc != 0:
                raise RuntimeError(f"vg_gather_degrade_u8 of {k}: {rc}")
        call()
        torch.cuda.synchronize()
        outs[k] = (o["noisy"].clone(), o["clean"].clone(), o["nhwc"].clone())
        routes[k] = graphed(call)
    same = all(torch.equal(x, y) for k in ("parent_copy", "new") for x, y in zip(outs["parent"], outs[k]))
    t = interleaved(routes, a.steps, a.rounds)
    r = [n / p for n, p in zip(t["new"], t["parent"])]
    aa = [c / p for c, p in zip(t["parent_copy"], t["parent"])]
    ratio, spread = statistics.median(r), max(abs(v - 1.0) for v in aa)
    out = {"what": "old entry vg_gather_degrade_u8, S=64 B=128 C=3, rect on, bf16 NHWC on; three libraries in one process, "
                   "interleaved windows of graph replays",
           "sha256": {k: hashlib.sha256(open(p, "rb").read()).hexdigest() for k, p in libs.items()},
           "us_per_launch": {k: summary(v) for k, v in t.items()},
           "new_over_parent_per_round": [round(v, 4) for v in r], "copy_over_parent_per_round": [round(v, 4) for v in aa],
           "ratio": round(ratio, 4), "aa_spread": round(spread, 4), "bound": round(1 + 2 * spread, 4),
           "within_bound": bool(ratio <= 1 + 2 * spread), "outputs_bit_identical_to_parent": bool(same)}
    print("ab", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-copy", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_models_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_models_bench needs the MI355X: there is nothing to time without it")
    if (a.parent_lib is None) != (a.parent_copy is None):
        raise SystemExit("ab needs both --parent-lib and --parent-copy")
    dev = "cuda"
    torch.cuda.set_device(0)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip()
        except Exception:
            commit = "unknown (no git metadata where this ran)"
    measured = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()
                for rel in (PKG + "/csrc/degrade.hip", PKG + "/csrc/median.hip", PKG + "/ops.py", "tools/noise_models_bench.py")}
    out = {"device": torch.cuda.get_device_name(0), "commit": commit, "sha256_of_the_measured_sources": measured,
           "what": "noise models of the degraded pairs and the median baseline at S=64 B=128 C=3: us per launch, median of "
                   "%d interleaved rounds of %d replays of graphs holding %d launches; tools/noise_models_bench.py"
                   % (a.rounds, a.steps, CALLS),
           "command": "python tools/noise_models_bench.py --steps %d --rounds %d%s" % (
               a.steps, a.rounds, " --parent-lib <parent build> --parent-copy <its byte copy>" if a.parent_lib else ""),
           "hbm_peak_bytes_per_s": HBM_PEAK}
    out["gather"] = mode_gather(a, dev)
    out["median"] = mode_median(a, dev)
    if a.parent_lib is not None:
        out["old_entry_ab"] = mode_ab(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
