"""GPU: the large-tensor BatchNorm passes of bn_act.hip (column reduce, normalise + activation, backward apply) compute,
bit for bit, what they computed before their thread mapping changed: tests/golden/bn_stream_parent.npz holds the raw
output bits of the earlier kernels on seeded inputs (tools/gen_golden_bn_stream.py, which also defines the cases).  The
step's largest shape is outside the fixture: it is checked against fp64 torch and for invariance under a row split."""
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = importlib.import_module(PKG + ".geometry")
DEV = "cuda"

_spec = importlib.util.spec_from_file_location("gen_golden_bn_stream", os.path.join(ROOT, "tools", "gen_golden_bn_stream.py"))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "bn_stream_parent.npz"))


@pytest.fixture
def separate(vg_switch):
    """The one-launch forms off: every call goes through the large-tensor kernels."""
    vg_switch("VG_BN_FUSED_FWD", 0)
    vg_switch("VG_BN_ONEPASS", 0)


# bf16 twice: as shipped (tensors this small keep 8-byte vectors per thread, VG_BN_WIDE_MIN) and with the 16-byte vectors
# of the large tensors forced on them -- the thread mapping the cases were chosen for
@pytest.mark.parametrize("dtype,wide_min", [(G.F32, None), (G.BF16, None), (G.BF16, 0)], ids=["f32", "bf16", "bf16_wide"])
@pytest.mark.parametrize("case", GEN.CASES, ids=[c[0] for c in GEN.CASES])
def test_outputs_are_the_parents_bits(ops, golden, separate, vg_switch, case, dtype, wide_min):
    if wide_min is not None:
        vg_switch("VG_BN_WIDE_MIN", wide_min)
    name = case[0]
    assert int(golden[f"seed/{name}/{dtype}"]) == GEN.case_seed(name, dtype)
    got = GEN.run_case(ops, *case, dtype)
    expected = {k.split("/")[2] for k in golden.files if k.startswith(f"{name}/{dtype}/")}
    assert expected == set(got) - {"y_twin"}
    for key in sorted(expected):
        want = torch.from_numpy(golden[f"{name}/{dtype}/{key}"].astype(np.int64))
        have = torch.from_numpy(GEN.to_bits(got[key]).astype(np.int64))
        assert want.shape == have.shape, key
        assert torch.equal(have, want), f"{name} dtype {dtype} {key}: {(have != want).sum().item()} of {want.numel()} words differ"
    if "y_twin" in got:                                         # the twin call writes the same activations
        assert torch.equal(got["y_twin"].view(torch.int16), got["y"].view(torch.int16))


# ---- the step's largest BatchNorm tensor: 131072 rows x 128 channels of bf16 (16.8 M elements) -------------------------
ROWS, C, ACT, SLOPE = 131072, 128, 2, 0.2
SPLIT = 50001                    # an odd row: both parts get another row-block plan than the whole; 50001 * 256 B is 16-byte aligned


@pytest.fixture(scope="module")
def big(ops):
    g = torch.Generator().manual_seed(131072)
    x = (torch.randn(ROWS, C, generator=g) * 1.7 + 0.3).to(torch.bfloat16).to(DEV)
    dy = torch.randn(ROWS, C, generator=g).to(torch.bfloat16).to(DEV)
    gamma = (torch.randn(C, generator=g) * 0.1 + 1).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.1).to(DEV)
    stats, nparts = ops.channel_stats(x, ROWS, C, G.BF16)
    co = ops.bn_finalize(stats, nparts, C, ROWS, gamma, beta, None, None, 0.1, 1e-5, DEV)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, co=co)


def test_largest_shape_against_fp64(ops, big, separate):
    """Tolerances of test_gpu_kernels.py::test_batchnorm_activation_forward_backward (bf16)."""
    x64 = big["x"].double().requires_grad_(True)
    g64, b64 = big["gamma"].double().requires_grad_(True), big["beta"].double().requires_grad_(True)
    z = F.batch_norm(x64.view(ROWS, C, 1, 1), None, None, g64, b64, True, 0.1, 1e-5)
    a_ref = F.leaky_relu(z, SLOPE)
    dx_ref, dg_ref, db_ref = torch.autograd.grad(a_ref, (x64, g64, b64), big["dy"].double().view(ROWS, C, 1, 1))
    a = ops.bn_act_forward(big["x"], big["co"], ROWS, C, ACT, SLOPE, G.BF16)
    torch.testing.assert_close(a.double(), a_ref.detach().view(ROWS, C), rtol=3e-2, atol=3e-2)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops.bn_act_backward(big["x"], big["dy"], big["co"], ROWS, C, ROWS, big["gamma"], ACT, SLOPE, dg, db, False, G.BF16)
    torch.testing.assert_close(dx.double(), dx_ref, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(dg.double(), dg_ref, rtol=5e-2, atol=5e-1)
    torch.testing.assert_close(db.double(), db_ref, rtol=5e-2, atol=5e-1)


def _apply(ops, x, dy, co, coef, rows):
    L = importlib.import_module(PKG + "._lib")
    dx = torch.empty_like(x)
    L.check(L.load().vg_bn_act_backward_apply(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), co[0, 2].data_ptr(),
                                              co[0, 3].data_ptr(), co[0, 0].data_ptr(), co[0, 1].data_ptr(),
                                              coef.data_ptr(), rows, C, ACT, SLOPE, 1, 4 * C, 3 * C, G.BF16, L.stream_ptr()),
            "vg_bn_act_backward_apply")
    return dx


def test_largest_shape_split_invariance(ops, big, separate):
    """Elementwise passes: all rows at once == rows [0, SPLIT) and [SPLIT, ROWS) in two calls, bit for bit."""
    x, dy, co = big["x"], big["dy"], big["co"]
    y, y8 = ops.bn_act_forward(x, co, ROWS, C, ACT, SLOPE, G.BF16, want_fp8=True)
    coef = torch.rand(1, 3, C, generator=torch.Generator().manual_seed(3)).to(DEV)
    dx = _apply(ops, x, dy, co, coef, ROWS)
    parts_y, parts_y8, parts_dx = [], [], []
    for lo, hi in ((0, SPLIT), (SPLIT, ROWS)):
        py, py8 = ops.bn_act_forward(x[lo:hi], co, hi - lo, C, ACT, SLOPE, G.BF16, want_fp8=True)
        parts_y.append(py), parts_y8.append(py8)
        parts_dx.append(_apply(ops, x[lo:hi], dy[lo:hi], co, coef, hi - lo))
    assert torch.equal(torch.cat(parts_y).view(torch.int16), y.view(torch.int16))
    assert torch.equal(torch.cat(parts_y8), y8)
    assert torch.equal(torch.cat(parts_dx).view(torch.int16), dx.view(torch.int16))
    assert torch.equal(ops.bn_act_forward(x, co, ROWS, C, ACT, SLOPE, G.BF16).view(torch.int16), y.view(torch.int16))
