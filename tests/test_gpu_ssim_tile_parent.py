"""GPU: the single-scale and the multi-scale SSIM losses compute, bit for bit, what they computed while csrc/ssimloss.hip
and csrc/msssim.hip each held their own statement of the tile pass: tests/golden/ssim_tile_parent.npz holds the raw output
bits (or, for the large gradients, their SHA-256) of that build on seeded inputs (tools/gen_golden_ssim_tile.py, which also
defines the cases and the calls).  The f64 comparisons of tests/test_gpu_ssimloss.py and tests/test_gpu_msssim.py bound the
error; this file pins the order of every sum and the absence of fma contraction in the shared csrc/ssim_tile.hpp."""
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("gen_golden_ssim_tile", os.path.join(ROOT, "tools", "gen_golden_ssim_tile.py"))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)

SINGLE = [(s, k) for s in GEN.SINGLE_SHAPES for k in GEN.SINGLE_KINDS]
MULTI = [(s, m, k) for s, m in GEN.MULTI_SHAPES for k in GEN.MULTI_KINDS]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ssim_tile_parent.npz"))


def assert_parents_bits(golden, case, got):
    stored = {k[len(case) + 1:] for k in golden.files if k.startswith(case + "/")}
    assert stored and stored == set(got), (case, sorted(stored), sorted(got))
    for key in sorted(stored):
        want, have = golden[f"{case}/{key}"], got[key]
        assert want.dtype == have.dtype and want.shape == have.shape, (case, key)
        what = "the digest differs" if want.dtype == np.uint8 else f"{int((want != have).sum())} of {want.size} words differ"
        assert np.array_equal(want, have), f"{case} {key}: {what}"


def test_the_fixture_holds_every_case_and_nothing_else(golden):
    cases = {GEN.single_id(*c) for c in SINGLE} | {GEN.multi_id(*c) for c in MULTI}
    assert {k.rsplit("/", 2)[0] for k in golden.files} == cases
    assert all(golden[k].dtype == (np.uint8 if golden[k].shape == (32,) and k.endswith("/d") else np.uint32) for k in golden.files)


@pytest.mark.parametrize("shape,kind", SINGLE, ids=[GEN.single_id(*c) for c in SINGLE])
def test_single_scale_outputs_are_the_parents_bits(ops, golden, shape, kind):
    got = GEN.run_single(ops, shape, kind)
    assert ("prefilled/d" in got) == (shape in GEN.SINGLE_ACCUMULATING)
    assert_parents_bits(golden, GEN.single_id(shape, kind), got)


@pytest.mark.parametrize("shape,M,kind", MULTI, ids=[GEN.multi_id(*c) for c in MULTI])
def test_multi_scale_outputs_are_the_parents_bits(ops, golden, shape, M, kind):
    got = GEN.run_multi(ops, shape, M, kind)
    assert ("explicit/d" in got) == (shape == GEN.EXPLICIT[0]) and ("prefilled/d" in got) == ((shape, kind) == GEN.PREFILLED)
    assert_parents_bits(golden, GEN.multi_id(shape, M, kind), got)
