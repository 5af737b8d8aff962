"""Writes tests/golden/ggn_parent.npz: the raw output and statistics-slab bits of the narrow-K direct convolution
(csrc/conv_narrowk.hpp) on the seeded normal bf16 operands of tests/_ggn_cases.py.  tests/test_gpu_ggn_stream.py regenerates
the operands from the seeds and asserts bit equality, so the fixture pins the arithmetic of whichever build wrote it.

Run it ONCE on a checkout whose results are to be preserved, on the GPU:

    python tools/gen_golden_ggn.py [output.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
OUT = os.path.join(ROOT, "tests", "golden", "ggn_parent.npz")


def main() -> None:
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from importlib import import_module
    ops = import_module(PKG + ".ops")
    import _ggn_cases as C
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    arrays = {}
    for name in sorted(C.CASES):
        y, st = C.run(ops, name)
        arrays[f"seed/{name}"] = np.int64(C.seed_of(name))
        arrays[f"{name}/y"] = y.numpy().view(np.uint16)
        if st is not None:
            arrays[f"{name}/stats"] = st.numpy().view(np.uint32)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
