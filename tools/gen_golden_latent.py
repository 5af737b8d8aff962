"""Writes tests/golden/latent_prior.npz: the reference's own vals_to_hist / sample_distribution (main_vae.py:415-436)
on a small f32 matrix, the fixture the latent-prior tests compare against bit for bit.

Runs only where the reference checkout exists (oracle/load_reference.py finds it); the two functions are taken from the
imported ``main_vae`` module.  The uniforms sample_distribution consumed are recovered without touching it: every
``np.random.rand()`` and every ``np.random.uniform()`` consumes exactly one double of the legacy global stream, so
re-seeding and drawing ``2 * n * D`` doubles gives them in order -- [..., 0] is u (picks the bin), [..., 1] is v (the
place inside it).

    python tools/gen_golden_latent.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

N, D, N_BINS, N_SAMPLES, SEED = 1500, 12, 100, 40, 20240


def make_matrix() -> np.ndarray:
    rng = np.random.default_rng(415)
    x = np.empty((N, D), dtype=np.float32)
    x[:, 0] = 0.75                                                    # constant column: range widened by +-0.5
    x[:, 1] = np.where(rng.random(N) < 0.3, -1.5, 2.25)               # two values: 98 empty bins
    q = rng.integers(0, 101, N).astype(np.float32) / 4.0              # quarter-integers in [0, 25]: values ON bin edges
    q[:2] = (0.0, 25.0)
    x[:, 2] = q
    x[:, 3] = rng.standard_normal(N)                                  # mu-like
    x[:, 4] = 3.0 * rng.standard_normal(N) + 7.0
    x[:, 5] = 1e-3 * rng.standard_normal(N) + 1000.0                  # narrow range far from zero: coarse f32 edges
    x[:, 6] = 0.3 * rng.standard_normal(N) - 5.0                      # logvar-like
    x[:, 7] = 1e-4 * rng.standard_normal(N)
    x[:, 8] = 250.0 * rng.standard_normal(N) - 40.0
    x[:, 9] = np.exp(rng.standard_normal(N))                          # skewed
    x[:, 10] = 0.05 * rng.standard_normal(N) - 9.5
    x[:, 11] = rng.standard_normal(N) ** 3
    return x


def main() -> None:
    from load_reference import load_reference
    load_reference()
    ref = sys.modules["main_vae"]
    x = make_matrix()
    bins, cdf = ref.vals_to_hist(x, N_BINS)
    np.random.seed(SEED)
    samples = ref.sample_distribution(bins, cdf, N_SAMPLES)
    np.random.seed(SEED)
    uv = np.random.random_sample(2 * N_SAMPLES * D).reshape(N_SAMPLES, D, 2)
    assert bins.dtype == np.float64 and cdf.dtype == np.float64 and samples.dtype == np.float32
    assert np.array_equal(bins, bins.astype(np.float32).astype(np.float64)), "numpy >= 2 keeps f32 edges"
    out = os.path.join(ROOT, "tests", "golden", "latent_prior.npz")
    np.savez_compressed(out, x=x, bins=bins, cdf=cdf, samples=samples, u=np.ascontiguousarray(uv[..., 0]),
                        v=np.ascontiguousarray(uv[..., 1]), n_bins=np.int64(N_BINS), seed=np.int64(SEED),
                        numpy_version=np.array(np.__version__))
    print("wrote", out, os.path.getsize(out), "bytes; numpy", np.__version__)


if __name__ == "__main__":
    main()
