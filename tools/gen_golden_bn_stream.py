"""Writes tests/golden/bn_stream_parent.npz: the raw output bits of the large-tensor BatchNorm passes (bn_act.hip:
column reduce, normalise + activation with and without the e4m3 twin, activation-only mode, backward reduce + apply)
on seeded inputs, with the fused small-tensor forms switched off.  tests/test_gpu_bn_stream.py regenerates the inputs
from the seeds and asserts bit equality, so the fixture pins the arithmetic of whichever build wrote it.

Run it ONCE on a checkout whose results are to be preserved (it only uses calls that have been there since the
grouped BatchNorm passes), on the GPU:

    python tools/gen_golden_bn_stream.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
OUT = os.path.join(ROOT, "tests", "golden", "bn_stream_parent.npz")
DEV = "cuda"

# name, rows per group, groups, C, act (0 none, 1 ReLU, 2 LeakyReLU), activation-only mode too.
# Threads per row / rows per pass are given for the 16-byte bf16 vector (8 channels); f32 and C % 8 != 0 use 4 channels.
CASES = [
    ("c4", 35, 1, 4, 1, True),            # 4-wide path, 1 thread per row
    ("c36", 35, 1, 36, 2, True),          # 4-wide path, 9 threads per row, 28 rows per pass, 4 threads idle
    ("c8_row1", 1, 1, 8, 0, True),        # a single row
    ("c8_ragged", 600, 1, 8, 2, False),   # several workgroups (256 / 128 rows per pass) and a ragged last one
    ("c200", 23, 1, 200, 2, False),       # 25 threads per row, 10 rows per pass, 6 threads idle, ragged third pass
    ("c200_g3", 7, 3, 200, 1, False),     # three groups, 7 rows each: less than one pass per group
    ("c64_g2", 45, 2, 64, 2, False),      # two groups, 45 rows each against 32 rows per pass
    ("c1024_g2", 3, 2, 1024, 1, False),   # 2 rows per pass, 3 rows per group
    ("c4096", 1, 1, 4096, 0, False),      # more than one column block
]
SLOPE = 0.2


def case_seed(name: str, dtype: int) -> int:
    return 9000 + 17 * [c[0] for c in CASES].index(name) + dtype


def make_inputs(name, rpg, groups, C, dtype):
    """x, dy [groups * rpg][C] rounded to the storage dtype (as float32), gamma, beta [C]; every group has its own
    offset and spread so that its coefficients differ from the other groups'."""
    import torch
    g = torch.Generator().manual_seed(case_seed(name, dtype))
    x = torch.randn(groups, rpg, C, generator=g)
    for k in range(groups):
        x[k] = x[k] * (1.7 - 0.5 * k) + (0.3 + 0.9 * k)
    dy = torch.randn(groups * rpg, C, generator=g)
    gamma = torch.randn(C, generator=g) * 0.1 + 1
    beta = torch.randn(C, generator=g) * 0.1
    td = torch.bfloat16 if dtype == 1 else torch.float32
    return x.view(groups * rpg, C).to(td), dy.to(td), gamma, beta


def run_case(ops, name, rpg, groups, C, act, act_only, dtype):
    """-> dict of CPU tensors: every output of the passes, as the library wrote it."""
    import torch
    x, dy, gamma, beta = make_inputs(name, rpg, groups, C, dtype)
    rows = rpg * groups
    X, DY, gm, bt = x.to(DEV), dy.to(DEV), gamma.to(DEV), beta.to(DEV)
    out = {}
    slabs = []
    for k in range(groups):                 # vg_channel_stats has no groups: one call per group, slabs concatenated
        st, n = ops.channel_stats(X[k * rpg:(k + 1) * rpg], rpg, C, dtype)
        slabs.append(st[:n * 2 * C].clone())
    stats = torch.cat(slabs)
    out["stats"] = stats
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    co = ops.bn_finalize(stats, n * groups, C, rows, gm, bt, rm, rv, 0.1, 1e-5, DEV, groups=groups)
    out["coeffs"] = co
    out["y"] = ops.bn_act_forward(X, co, rows, C, act, SLOPE, dtype)
    if dtype == 1:
        y2, y8 = ops.bn_act_forward(X, co, rows, C, act, SLOPE, dtype, want_fp8=True)
        out["y_twin"], out["y8"] = y2, y8
    if act_only:
        out["y_act_only"] = ops.bn_act_forward(X, None, rows, C, 2, SLOPE, dtype)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    out["dx"] = ops.bn_act_backward(X, DY, co, rows, C, rows, gm, act, SLOPE, dg, db, False, dtype)
    out["partial"] = ops.WS.get("bnbwd", 0, X.device)[:groups * n * 2 * C].clone()     # the reduce's slabs, by group
    out["dgamma"], out["dbeta"] = dg, db
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def to_bits(t) -> np.ndarray:
    import torch
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    if t.dtype == torch.float32:
        return t.numpy().view(np.uint32)
    return t.numpy()


def separate_passes(ops) -> None:
    """Switch the one-launch forms off so that every call goes through the large-tensor kernels."""
    os.environ["VG_BN_FUSED_FWD"] = "0"
    os.environ["VG_BN_ONEPASS"] = "0"
    ops.reload_switches()


def main() -> None:
    sys.path[:0] = [ROOT]
    from importlib import import_module
    ops = import_module(PKG + ".ops")
    separate_passes(ops)
    arrays = {}
    for dtype in (0, 1):
        for name, rpg, groups, C, act, act_only in CASES:
            arrays[f"seed/{name}/{dtype}"] = np.int64(case_seed(name, dtype))
            for k, v in run_case(ops, name, rpg, groups, C, act, act_only, dtype).items():
                if k != "y_twin":           # the twin call's y is compared with "y" itself
                    arrays[f"{name}/{dtype}/{k}"] = to_bits(v)
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
