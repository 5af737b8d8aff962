"""CPU: the numpy restatement of the operand-pack formula (tests/_pack_ref.py) against the index-level emulator the geometry
tests use (tests/_emulate.py: written separately, element by element), over the operand list the GPU pack tests share."""
import numpy as np
import pytest
import torch

import _pack_ref as PR
from _emulate import emulate_pack

G = PR.G


@pytest.mark.parametrize("dtype", [G.F32, G.BF16], ids=["f32", "bf16"])
def test_restated_pack_equals_the_index_level_emulator(dtype):
    g = torch.Generator().manual_seed(3)
    forms = set()
    for pk, wshape in PR.pack_specs(dtype):
        w = torch.randn(wshape, generator=g)
        ref, written = PR.pack_ref(pk, w.numpy())
        assert ref.shape == (pk.nphase, pk.N, pk.Kp) and ref.dtype == np.float32
        assert np.array_equal(ref.astype(np.float64), emulate_pack(pk, w).numpy()), pk
        assert (ref[~written] == 0).all()
        assert written.sum() == pk.nphase * pk.N * pk.TH * pk.TW * pk.C
        forms.add((pk.nphase, pk.tap_in_n, pk.IC > pk.C, pk.Kp > pk.TH * pk.TW * pk.IC))
    # the list holds both forms, one and four phases, channel padding and K padding
    assert {f[:2] for f in forms} == {(1, 0), (4, 0), (1, 1)}
    assert any(f[2] for f in forms) and any(f[3] for f in forms)
