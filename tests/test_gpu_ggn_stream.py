"""GPU: the narrow-K direct convolution (csrc/conv_narrowk.hpp) against tests/golden/ggn_parent.npz, bit for bit.

The fixture (tools/gen_golden_ggn.py) holds the output and statistics-slab bits of the one-tile-per-workgroup kernel on
seeded normal bf16 operands (tests/_ggn_cases.py: four instantiations, 1331 output pixels = 5 tiles and a last one of 51).
However many tiles a workgroup walks -- VG_NK_WGS caps the workgroups of a launch: 1 (one workgroup walks all six tiles),
2 (three each) and unset (one each at this size) -- the bits must be those."""
import importlib
import os

import numpy as np
import pytest
import torch

import _ggn_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(C.R.PKG + ".ops")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ggn_parent.npz"))


@pytest.mark.parametrize("cap", [1, 2, None], ids=["wgs1", "wgs2", "unset"])
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_bits_of_the_one_tile_kernel(ops, golden, vg_switch, monkeypatch, name, cap):
    assert int(golden[f"seed/{name}"]) == C.seed_of(name)
    monkeypatch.delenv("VG_NK_WGS", raising=False)
    if cap is not None:
        vg_switch("VG_NK_WGS", cap)
    else:
        ops.reload_switches()
    y, st = C.run(ops, name)
    want = torch.from_numpy(golden[f"{name}/y"].view(np.int16))
    bad = (y != want)
    assert not bad.any(), f"output: {int(bad.sum())} of {want.numel()} words differ; first at {tuple(int(v) for v in bad.nonzero()[0])}"
    assert (st is not None) == (f"{name}/stats" in golden.files)
    if st is not None:
        want = torch.from_numpy(golden[f"{name}/stats"].view(np.int32))
        bad = (st != want)
        assert not bad.any(), f"statistics: {int(bad.sum())} of {want.numel()} words differ; first at (slab, which, n) {tuple(int(v) for v in bad.nonzero()[0])}"
