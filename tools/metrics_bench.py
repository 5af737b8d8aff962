"""Feature-space metrics: the device route (ops.feat_stats_accum; metrics.precision_recall = 2 x ops.knn_radius2 +
2 x ops.manifold_cover) against what a user does today, measured in the same process on the same box:

  (a) the host route: device -> host copy of the features, then numpy f64 ``x.T @ x`` and a chunked numpy f32
      GEMM-form k-NN / cover (what tests/_metrics_ref.py states, made fast enough to time);
  (b) stock torch on the same GPU: ``X.double().T @ X.double()`` and a chunked ``torch.cdist`` + ``topk`` / compare.

N in {3 000, 30 000} (the reference's 10 % validation split of CelebA-HQ and the whole set), D in {64, 100, 2048}, k = 3,
real = N(0, I), fake = 0.25 + 0.9 N(0, I).  Device legs: eager launches, device events around `reps` back-to-back calls
after a warm-up, median over the rounds; precision_recall is timed with its one host sync (perf_counter around the call
after a synchronise).  Host legs: perf_counter around one call, the D2H copy included; the host k-NN leg is skipped where
it needs more than --host-max-tflop of arithmetic ("not measured").  Beside the times: the arithmetic the algorithm
needs -- n D (D + 1) f64 flops for the upper triangle of X^T X, 8 N^2 D f32 flops for the four distance passes -- over
the measured time as a fraction of the MFMA peaks (f32 157.3 TF; f64 78.6 TF, AMD's published figure), the kernel's
workspace and route (b)'s peak allocation.  Before timing, both device results are compared with route (b)'s.  No
threshold: the claim is "no host round trip, no N x N allocation, deterministic"; where a shape is slower than (b) the
JSON says so.

    python tools/metrics_bench.py [--rounds 5] [--out profiles/metrics_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch
from importlib import import_module

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
M = import_module(PKG + ".metrics")
LIB = import_module(PKG + "._lib")
F32_PEAK, F64_PEAK = 157.3e12, 78.6e12


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps                       # ms per call


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def med(fn, rounds):
    return statistics.median(fn() for _ in range(rounds))


# ---- route (a): host ---------------------------------------------------------------------------------------------------
def host_stats(xd):
    x = xd.cpu().numpy().astype(np.float64)
    return x.sum(0), x.T @ x


def host_d2_chunks(a, b, chunk=2048):
    na, nb = (a * a).sum(1), (b * b).sum(1)
    for i in range(0, len(a), chunk):
        yield i, np.maximum(na[i:i + chunk, None] + nb[None, :] - 2.0 * (a[i:i + chunk] @ b.T), 0.0)


def host_knn(x, k):
    out = np.empty(len(x), np.float32)
    for i, d in host_d2_chunks(x, x):
        d[np.arange(d.shape[0]), i + np.arange(d.shape[0])] = np.inf
        out[i:i + d.shape[0]] = np.partition(d, k - 1, axis=1)[:, k - 1]
    return out


def host_cover(q, ref, r2):
    return sum(int((d <= r2[None, :]).any(1).sum()) for _, d in host_d2_chunks(q, ref))


def host_pr(rd, fd, k):
    r, f = rd.cpu().numpy(), fd.cpu().numpy()
    return host_cover(f, r, host_knn(r, k)) / len(f), host_cover(r, f, host_knn(f, k)) / len(r)


# ---- route (b): stock torch on the GPU -------------------------------------------------------------------------------------
def torch_stats(xd):
    x = xd.double()
    return x.sum(0), x.T @ x


def torch_knn(x, k, chunk=4096):
    out = torch.empty(len(x), dtype=torch.float32, device=x.device)
    for i in range(0, len(x), chunk):
        d = torch.cdist(x[i:i + chunk], x).square_()
        n = d.shape[0]
        d[torch.arange(n, device=x.device), i + torch.arange(n, device=x.device)] = float("inf")
        out[i:i + n] = d.topk(k, dim=1, largest=False).values[:, k - 1]
    return out


def torch_cover(q, ref, r2, chunk=4096):
    tot = torch.zeros((), dtype=torch.int64, device=q.device)
    for i in range(0, len(q), chunk):
        tot += (torch.cdist(q[i:i + chunk], ref).square_() <= r2[None, :]).any(1).sum()
    return tot


def torch_pr(rd, fd, k):
    a = torch_cover(fd, rd, torch_knn(rd, k))
    b = torch_cover(rd, fd, torch_knn(fd, k))
    a, b = torch.stack([a, b]).tolist()
    return a / len(fd), b / len(rd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[3000, 30000])
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 100, 2048])
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--host-max-tflop", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs the MI355X: there is nothing to time without it")
    dev, k = "cuda", a.k
    lib = LIB.load()
    rows = []
    for N in a.sizes:
        for D in a.dims:
            g = torch.Generator(device=dev).manual_seed(1000 * D + N)
            real = torch.randn(N, D, generator=g, device=dev)
            fake = 0.25 + 0.9 * torch.randn(N, D, generator=g, device=dev)
            row = {"N": N, "D": D, "k": k}
            # ---- statistics ----
            s = torch.zeros(D, dtype=torch.float64, device=dev)
            o = torch.zeros(D, D, dtype=torch.float64, device=dev)
            ops.feat_stats_accum(real, s, o)
            ts, to = torch_stats(real)
            row["stats_max_rel_diff_vs_torch"] = float(((o - to).abs().max() / to.abs().max()).item())
            flops = float(N) * D * (D + 1)
            reps = max(2, min(200, int(2e11 / max(flops, 1))))
            ms = med(lambda: timed(lambda: ops.feat_stats_accum(real, s, o), reps), a.rounds)
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            torch_stats(real)
            peak_b = torch.cuda.max_memory_allocated() - base
            ms_b = med(lambda: timed(lambda: torch_stats(real), reps), a.rounds)
            ms_a = med(lambda: wall(lambda: host_stats(real))[0], min(a.rounds, 3))
            row["stats"] = {"device_ms": ms, "torch_ms": ms_b, "host_ms": ms_a, "f64_flops_needed": flops,
                            "f64_mfma_peak_fraction": flops / (ms * 1e-3) / F64_PEAK,
                            "workspace_bytes": int(lib.vg_feat_stats_accum_ws_bytes(N, D)),
                            "torch_peak_extra_bytes": int(peak_b), "slower_than_torch": bool(ms > ms_b)}
            # ---- precision / recall ----
            got = M.precision_recall(real, fake, k)
            pb, rb = torch_pr(real, fake, k)
            row["pr_device"] = {"precision": got["precision"], "recall": got["recall"]}
            row["pr_torch"] = {"precision": pb, "recall": rb}
            flops = 8.0 * N * N * D
            ms = med(lambda: wall(lambda: M.precision_recall(real, fake, k))[0], a.rounds)
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            torch_pr(real, fake, k)
            peak_b = torch.cuda.max_memory_allocated() - base
            ms_b = med(lambda: wall(lambda: torch_pr(real, fake, k))[0], a.rounds)
            if flops <= a.host_max_tflop * 1e12:
                ms_a, (pa, ra) = wall(lambda: host_pr(real, fake, k))
                row["pr_host"] = {"precision": pa, "recall": ra}
            else:
                ms_a = None                                   # not measured: minutes of host arithmetic
            ws = 2 * int(lib.vg_knn_radius2_ws_bytes(N, D, k)) + 2 * int(lib.vg_manifold_cover_ws_bytes(N, N, D))
            row["pr"] = {"device_ms": ms, "torch_ms": ms_b, "host_ms": ms_a, "f32_flops_needed": flops,
                         "f32_mfma_peak_fraction": flops / (ms * 1e-3) / F32_PEAK,
                         "workspace_bytes_sum_of_four_calls": ws, "torch_peak_extra_bytes": int(peak_b),
                         "slower_than_torch": bool(ms > ms_b)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del real, fake, s, o
    out = {"what": "feature-space metrics: device route vs host route (a) and stock torch on the GPU (b); tools/metrics_bench.py",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "peaks": {"f32_mfma": F32_PEAK, "f64_mfma_published": F64_PEAK}, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
