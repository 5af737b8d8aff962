"""Gaussian-mixture prior: one EM iteration on the device (ops.gmm_log_resp + ops.gmm_moments: vg_gmm_log_resp, one launch;
vg_gmm_moments, two launches) against scikit-learn on the host, and the sampler, measured in the same process on the same
box.  N = 200 000 rows, D = 100, K = 10 on synthetic latents (a seeded 10-component mixture, f32 on the device).

  kernels   one device-event pair around the E-step call, around the M-step call and around both, `--reps` (>= 20) calls
            after a warm-up, at the parameters of a fit that has run `--iters` iterations: median, min, max.  Beside the
            times: the f64 flops the algorithm needs -- E: N K D (D + 1) for the triangular product y = d U plus 2 N K D for
            the squares; M: N K D (D + 1) for the symmetric s2 plus 3 N K D for r * d and s1 -- over the measured time, as a
            fraction of the f64 matrix peak (78.6 TF, AMD's published figure), and the flops the MFMAs actually issue
            (D padded to 16, diagonal blocks computed in full).
  fit       wall clock (perf_counter around a call that ends in a host sync) of GaussianMixturePrior.fit with tol = 0 and
            max_iter = `--iters`: the three launches, the host sync and the K small D x D host steps of every iteration.
  host      the same `--iters` iterations of sklearn.mixture.GaussianMixture (covariance_type="full", tol = 0) on the f64
            host copy from the same initialisation, threads as the environment sets them (recorded); the device -> host
            copy is timed separately.  lower_bound_ of both sides is recorded as the check that they do the same work.
  sampler   vg_gmm_sample at n = 4096 into the bf16 Generator input, draws made in the kernel: device events.

No threshold: the numbers are recorded, not gated.

    python tools/gmm_bench.py [--reps 20] [--iters 3] [--out profiles/gmm_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch
from importlib import import_module

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
latent = import_module(PKG + ".latent")
G = import_module(PKG + ".geometry")
LIB = import_module(PKG + "._lib")
F64_PEAK = 78.6e12


def event_times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def synthetic_latents(N, D, K, seed):
    """f32 [N, D]: K overlapping full-covariance Gaussians."""
    r = np.random.default_rng(seed)
    cen = r.normal(size=(K, D)) * 1.2
    A = r.normal(size=(K, D, D)) / np.sqrt(D) + np.eye(D) * 0.5
    lab = r.integers(0, K, N)
    x = np.empty((N, D), np.float32)
    for k in range(K):
        rows = np.nonzero(lab == k)[0]
        x[rows] = cen[k] + r.normal(size=(len(rows), D)) @ A[k].T
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--components", type=int, default=10)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gmm_bench needs the MI355X: there is nothing to time without it")
    if a.reps < 20:
        raise SystemExit("gmm_bench: --reps must be at least 20")
    dev, N, D, K, iters, reg = "cuda", a.rows, a.dim, a.components, a.iters, 1e-6
    lib = LIB.load()
    xh = synthetic_latents(N, D, K, 7)
    x = torch.from_numpy(xh).to(dev)
    idx = np.random.default_rng(0).choice(N, K, replace=False)

    def fit():
        return latent.GaussianMixturePrior.fit(x, K, reg_covar=reg, tol=0.0, max_iter=iters, init_idx=idx)

    prior = fit()                                                        # warm: code objects, workspace
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prior = fit()
        walls.append((time.perf_counter() - t0) * 1e3)
    coef = prior._log_coef
    e_ms = event_times(lambda: ops.gmm_log_resp(x, prior.means, prior.prec_chol, coef), a.reps, a.warmup)
    _, ln, resp = ops.gmm_log_resp(x, prior.means, prior.prec_chol, coef)
    m_ms = event_times(lambda: ops.gmm_moments(x, prior.means, resp, ln), a.reps, a.warmup)

    def both():
        _, l2, r2 = ops.gmm_log_resp(x, prior.means, prior.prec_chol, coef)
        ops.gmm_moments(x, prior.means, r2, l2)
    it_ms = event_times(both, a.reps, a.warmup)
    DP = (D + 15) // 16 * 16
    NB = (DP // 16) * (DP // 16 + 1) // 2                               # 16 x 16 blocks of the upper triangle of s2
    e_need = float(N) * K * (D * (D + 1) + 2 * D)
    m_need = float(N) * K * (D * (D + 1) + 3 * D)
    e_issued = float((N + 63) // 64 * 64) * K * 2 * 16 * sum(16 * (jt + 1) for jt in range(DP // 16))
    m_issued = float((N + 15) // 16 * 16) * K * NB * 2 * 16 * 16
    rate = lambda flops, ms: flops / (statistics.median(ms) * 1e-3)      # noqa: E731
    out = {"what": "Gaussian-mixture prior: one EM iteration on the device vs scikit-learn on the host, and the sampler; "
                   "tools/gmm_bench.py",
           "device": torch.cuda.get_device_name(0), "peaks": {"f64_matrix_published": F64_PEAK},
           "N": N, "D": D, "K": K, "iterations": iters, "reg_covar": reg,
           "e_step": dict(summary(e_ms), launches=1, f64_flops_needed=e_need, f64_flops_issued_on_mfma=e_issued,
                          f64_flop_rate=rate(e_need, e_ms), f64_peak_fraction=rate(e_need, e_ms) / F64_PEAK,
                          bytes_min=N * D * 4 + N * K * 8 + N * 8),
           "m_step": dict(summary(m_ms), launches=2, f64_flops_needed=m_need, f64_flops_issued_on_mfma=m_issued,
                          f64_flop_rate=rate(m_need, m_ms), f64_peak_fraction=rate(m_need, m_ms) / F64_PEAK,
                          bytes_min=N * D * 4 + N * K * 8 + N * 8,
                          workspace_bytes=int(lib.vg_gmm_moments_ws_bytes(N, D, K))),
           "em_iteration_kernels": dict(summary(it_ms), launches=3, f64_flops_needed=e_need + m_need,
                                        f64_flop_rate=rate(e_need + m_need, it_ms),
                                        f64_peak_fraction=rate(e_need + m_need, it_ms) / F64_PEAK),
           "device_fit": {"wall_ms": summary(walls), "per_iteration_ms": statistics.median(walls) / iters,
                          "lower_bound": prior.lower_bound, "n_iter": prior.n_iter,
                          "includes": "init moments call, 3 launches + 1 host sync + K host Cholesky steps per iteration"}}
    print(json.dumps({k: out[k] for k in ("e_step", "m_step", "em_iteration_kernels", "device_fit")}), flush=True)

    if a.skip_host:
        out["host_sklearn"] = "not measured (--skip-host)"
    else:
        from sklearn.mixture import GaussianMixture
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x64 = x.cpu().numpy().astype(np.float64)
        copy_ms = (time.perf_counter() - t0) * 1e3
        var = x64.var(axis=0)
        prec = np.tile(np.diag(1.0 / (var + reg)), (K, 1, 1))
        gm = GaussianMixture(K, covariance_type="full", reg_covar=reg, tol=0.0, max_iter=iters, init_params="random",
                             weights_init=np.full(K, 1.0 / K), means_init=x64[idx], precisions_init=prec)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                              # tol = 0 never converges: that is the point
            gm.fit(x64)
        host_ms = (time.perf_counter() - t0) * 1e3
        try:
            from threadpoolctl import threadpool_info
            threads = [{"api": p.get("user_api"), "threads": p.get("num_threads")} for p in threadpool_info()]
        except ImportError:
            threads = "threadpoolctl not available"
        out["host_sklearn"] = {"wall_ms": host_ms, "per_iteration_ms": host_ms / iters, "d2h_copy_and_widen_ms": copy_ms,
                               "n_iter": int(gm.n_iter_), "lower_bound": float(gm.lower_bound_), "threads": threads,
                               "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"),
                               "includes": "the random responsibilities of init_params='random' (unused) and one extra "
                                           "E-step at the end of fit",
                               "lower_bound_diff_vs_device": abs(float(gm.lower_bound_) - prior.lower_bound),
                               "per_iteration_ratio_host_over_device_fit": (host_ms / iters) /
                                                                           (statistics.median(walls) / iters)}
        print(json.dumps(out["host_sklearn"]), flush=True)

    n = a.samples
    ns = ops.NoiseStream(dev, 11)
    ns.advance()
    zp = G.padc(D, G.BF16)
    s_ms = event_times(lambda: ops.gmm_sample(prior.cdf, prior.means, prior.cov_chol, n, None, None, ns.state,
                                              want_z32=False, z=(zp, G.BF16)), a.reps, a.warmup)
    out["sampler"] = dict(summary(s_ms), n=n, launches=1, output="bf16 [n,1,1,%d], draws made in the kernel" % zp,
                          f64_flops=float(n) * D * (D + 1))
    print(json.dumps(out["sampler"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
