"""CPU: host-side logic of the product -- module tree / state_dict / init parity with the reference
(through the golden vectors), loud failure off-GPU, and the C ABI: the shared library loads and
exports every symbol include/vaegan_hip.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import vaegan_ref as R
from _inputs import tstats

import vaegan_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Encoder.__init__ (main_vae.py:43-45) pushes zeros through the CNN on the CPU.  In exact arithmetic every
# block then sees zeros (BatchNorm of a constant map is beta = 0); the reference's ATen kernels leave ~1e-6
# rounding noise instead, so its deeper running_mean buffers are 0.1*bias + O(1e-7).  The product has no CPU
# compute path and sets the noise-free values; tolerance on exactly these buffers (decays 0.9x per train step).
_NOISY = re.compile(r"cnn\.[123]\.bn\.running_mean")
_NOISE_ATOL = 2e-7


def _build(S=256):
    V.configure_seed(42)
    e = V.Encoder([3, S, S], 100)
    g = V.Generator(nz=100, img_size=S)
    d = V.Discriminator(img_size=S)
    g.apply(V.weights_init)
    d.apply(V.weights_init)
    return e, g, d


def test_seed42_construction_matches_reference_golden(golden_dir):
    """vaegan_code.py:19-40: same RNG consumption order, same values, same state_dict keys (App. A.3)."""
    gold = np.load(os.path.join(golden_dir, "init_seed42.npz"))
    e, g, d = _build(256)
    fz = torch.randn(64, 100, 1, 1)
    np.testing.assert_array_equal(fz.flatten()[:8].numpy(), gold["fixed_noise#samp"])
    for name, m in (("E", e), ("G", g), ("D", d)):
        sd = m.state_dict()
        gold_keys = sorted(k[len(name) + 1:-6] for k in gold.files if k.startswith(name + ".") and k.endswith("#stats"))
        assert sorted(sd.keys()) == gold_keys
        for k, v in sd.items():
            s, samp = tstats(v.float())
            if _NOISY.search(k):
                np.testing.assert_allclose(samp, gold[f"{name}.{k}#samp"], rtol=0, atol=_NOISE_ATOL, err_msg=k)
                continue
            np.testing.assert_array_equal(s, gold[f"{name}.{k}#stats"], err_msg=f"{name}.{k}")
            np.testing.assert_array_equal(samp, gold[f"{name}.{k}#samp"], err_msg=f"{name}.{k}")


@pytest.mark.parametrize("S", [64, 128, 256])
def test_encoder_dummy_forward_side_effect_is_reproduced(golden_dir, S):
    """main_vae.py:43-45 / SURVEY A.2 -- reproduced analytically (no CPU compute path exists)."""
    gold = np.load(os.path.join(golden_dir, "init_seed42.npz"))
    V.configure_seed(42)
    e = V.Encoder([3, S, S], 100)
    assert e.flatten_size == int(gold[f"E{S}.flatten_size"][0])
    for i in range(4):
        np.testing.assert_array_equal(e.cnn[i].conv.bias.detach().numpy(), gold[f"E{S}.cnn.{i}.conv.bias"])
        if i == 0:
            np.testing.assert_array_equal(e.cnn[i].bn.running_mean.numpy(), gold[f"E{S}.cnn.{i}.bn.running_mean"])
        else:
            np.testing.assert_allclose(e.cnn[i].bn.running_mean.numpy(), gold[f"E{S}.cnn.{i}.bn.running_mean"],
                                       rtol=0, atol=_NOISE_ATOL)
        np.testing.assert_array_equal(e.cnn[i].bn.running_var.numpy(), gold[f"E{S}.cnn.{i}.bn.running_var"])
        assert int(e.cnn[i].bn.num_batches_tracked) == 1


@pytest.mark.parametrize("S", [64, 128, 256])
def test_state_dict_matches_oracle_family(S):
    e, g, d = _build(S)
    o = R.RefVAEGAN(img_size=S, seed=42)
    for m, st in ((e, o.E), (g, o.G), (d, o.D)):
        sd = m.state_dict()
        assert list(sd.keys()) == list(st.keys())
        for k in sd:
            if _NOISY.search(k):
                torch.testing.assert_close(sd[k], st[k].detach(), rtol=0, atol=_NOISE_ATOL)
            else:
                assert torch.equal(sd[k], st[k].detach()), k


def test_reference_style_checkpoint_files_interchange(tmp_path):
    """torch.save(decoder.state_dict()) (vaegan_code.py:193) / torch.load(weights_only=True) + load_state_dict
    (main_vae.py:246-249): files written from this package load into a torch.nn replica of the reference's module
    tree (same keys, shapes, dtypes) and files written by that replica load into this package."""
    e, g, d = _build(256)
    path = str(tmp_path / "vaegan_0000_decoder.pth")
    torch.save(g.state_dict(), path)
    sd = torch.load(path, weights_only=True)
    nn = torch.nn
    layers, c = [nn.ConvTranspose2d(100, 1024, 4, 1, 0, bias=False), nn.BatchNorm2d(1024), nn.ReLU(True)], 1024
    while c > 16:
        layers += [nn.ConvTranspose2d(c, c // 2, 4, 2, 1, bias=False), nn.BatchNorm2d(c // 2), nn.ReLU(True)]
        c //= 2
    layers += [nn.ConvTranspose2d(16, 3, 3, 1, 1, bias=False), nn.Tanh()]

    class RefShaped(nn.Module):                        # the reference Generator's module tree (gan_code.py:16-54)
        def __init__(self):
            super().__init__()
            self.main = nn.Sequential(*layers)

    ref = RefShaped()
    ref.load_state_dict(sd)                            # strict: keys and shapes must match exactly
    for k, v in ref.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k])
    with torch.no_grad():
        ref.main[0].weight.mul_(2.0)
    torch.save(ref.state_dict(), path)
    g.load_state_dict(torch.load(path, weights_only=True))
    assert torch.equal(g.main[0].weight, ref.main[0].weight)


def test_weights_init_matches_on_class_names():
    g = V.Generator(nz=100, img_size=64)
    names = {type(m).__name__ for m in g.modules()}
    assert {"ConvTranspose2d", "BatchNorm2d", "ReLU", "Tanh"} <= names
    d = V.Discriminator(img_size=64)
    assert {type(m).__name__ for m in d.main} == {"Conv2d", "BatchNorm2d", "LeakyReLU", "Sigmoid"}


def test_no_cpu_fallback():
    e, g, d = _build(64)
    with pytest.raises(RuntimeError, match="only runs on the MI355X"):
        e(torch.zeros(2, 3, 64, 64))
    with pytest.raises(RuntimeError, match="only runs on the MI355X"):
        g(torch.zeros(2, 100, 1, 1))
    with pytest.raises(RuntimeError, match="only runs on the MI355X"):
        d(torch.zeros(2, 3, 64, 64))
    with pytest.raises(RuntimeError, match="parameter container"):
        g.main[0](torch.zeros(2, 100, 1, 1))
    with pytest.raises(RuntimeError, match="MI355X"):
        V.Adam(e.parameters(), lr=2e-4)


def test_size_rule_rejects_unsupported_sizes():
    with pytest.raises(ValueError):
        V.Generator(nz=100, img_size=96)


def _header_functions():
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vg_[a-z0-9_]+)\s*\(", src)))


def test_c_abi_library_exports_every_declared_symbol():
    from importlib import import_module
    L = import_module("vae-gan-based-model-for-image-generation-and-denoising_amd._lib")
    assert os.path.isfile(L.LIB_PATH), "libvaegan_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(L.LIB_PATH)
    declared = _header_functions()
    assert declared, "no declarations parsed from include/vaegan_hip.h"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in vaegan_hip.h but not exported"
    assert sorted(L.SIGNATURES) == declared, "ctypes binding table out of sync with the header"
    lib.vg_abi_version.restype = ctypes.c_int
    assert lib.vg_abi_version() == L.ABI_VERSION


def test_c_abi_rejects_bad_arguments_on_host():
    """Shape / alignment validation happens before any launch, so it is testable without a GPU."""
    from importlib import import_module
    L = import_module("vae-gan-based-model-for-image-generation-and-denoising_amd._lib")
    lib = L.load()
    d = L.GGDesc()                                  # all zeros: NULL pointers, zero sizes
    assert lib.vg_gather_gemm(ctypes.byref(d), 0, None) == -1
    assert lib.vg_gather_gemm(ctypes.byref(d), 7, None) == -3
    plan = L.GGPlan()                               # the launcher's plan as a host-only query: validated like a launch
    assert lib.vg_gather_gemm_plan(ctypes.byref(d), 0, ctypes.byref(plan)) == -1
    assert lib.vg_gather_gemm_plan(ctypes.byref(d), 7, ctypes.byref(plan)) == -3
    # the BatchNorm launchers' plan, validated like their launches: no record, no rows, an unknown kind, rows that do not
    # divide into the groups (-1); C % 4 (-2); a dtype the passes do not have (-3); a refused one-launch form is an answer (0)
    bn = L.BNPlan()
    assert lib.vg_bn_launch_plan(1, 64, 64, 1, 1, 1, 0, None) == -1
    assert lib.vg_bn_launch_plan(1, 0, 64, 1, 1, 1, 0, ctypes.byref(bn)) == -1
    assert lib.vg_bn_launch_plan(4, 64, 64, 1, 1, 1, 0, ctypes.byref(bn)) == -1
    assert lib.vg_bn_launch_plan(-1, 64, 64, 1, 1, 1, 0, ctypes.byref(bn)) == -1
    assert lib.vg_bn_launch_plan(0, 65, 64, 2, 1, 1, 0, ctypes.byref(bn)) == -1
    assert lib.vg_bn_launch_plan(0, 64, 64, 0, 1, 1, 0, ctypes.byref(bn)) == -1
    assert lib.vg_bn_launch_plan(2, 64, 6, 1, 1, 1, 0, ctypes.byref(bn)) == -2
    assert lib.vg_bn_launch_plan(1, 64, 64, 1, 2, 1, 0, ctypes.byref(bn)) == -3
    assert lib.vg_bn_launch_plan(3, 64, 96, 1, 1, 1, 4, ctypes.byref(bn)) == 0 and bn.fused == 0 and bn.kind == 3
    assert lib.vg_bn_launch_plan(0, 64, 64, 2, 0, 1, 0, ctypes.byref(bn)) == 0 and (bn.kind, bn.vec, bn.groups) == (0, 4, 2)
    # the weight-gradient launchers' plans, validated like their launches
    w, wp = L.WGDesc(), L.WGPlan()
    assert lib.vg_wgrad_plan(ctypes.byref(w), 0, ctypes.byref(wp)) == -1
    assert lib.vg_wgrad_plan(ctypes.byref(w), 7, ctypes.byref(wp)) == -3
    assert lib.vg_wgrad_plan(ctypes.byref(w), 0, None) == -1
    e, ep = L.EWDesc(), L.EWPlan()
    assert lib.vg_edge_wgrad_plan(ctypes.byref(e), ctypes.byref(ep)) == -1
    assert lib.vg_edge_wgrad_plan(ctypes.byref(e), None) == -1
    e = L.EWDesc(B=1, WH=8, WW=8, C=48, NH=16, NW=16, N=3, K=4, S=2, P=1)
    assert lib.vg_edge_wgrad_plan(ctypes.byref(e), ctypes.byref(ep)) == -3
    # the transposed edge convolution's plan: validated like its launch, except that it looks at no pointer but rng
    t, tp = L.TNDesc(), L.TNPlan()
    assert lib.vg_tnconv_plan(ctypes.byref(t), ctypes.byref(tp)) == -1
    geo = dict(B=1, IH=16, IW=16, C=64, N=3, K=3, S=1, P=1, OH=16, OW=16, OC=8, Wpitch=64)
    t = L.TNDesc(**geo)
    assert lib.vg_tnconv_plan(ctypes.byref(t), None) == -1
    assert lib.vg_tnconv_plan(ctypes.byref(t), ctypes.byref(tp)) == 0 and (tp.nt, tp.kc, tp.grid, tp.quad_noise) == (2, 2, 1, 0)
    assert lib.vg_tnconv_supported(ctypes.byref(t)) == -1 and lib.vg_tnconv(ctypes.byref(t), None) == -1      # NULL operands
    for bad, rc in ((dict(C=48), -3), (dict(IW=24, OW=24), -3), (dict(N=5), -3), (dict(K=4), -3), (dict(Wpitch=32), -2),
                    (dict(OW=17), -1), (dict(P=9, OH=0, OW=0), -1)):      # P = 9: a padding that leaves no output
        t = L.TNDesc(**dict(geo, **bad))
        assert lib.vg_tnconv_plan(ctypes.byref(t), ctypes.byref(tp)) == rc, bad
        t.X = t.Wp = t.Y = 64                            # with operands in place the launch path gives the same code
        assert lib.vg_tnconv_supported(ctypes.byref(t)) == rc and lib.vg_tnconv(ctypes.byref(t), None) == rc, bad
    assert lib.vg_adam_step(None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, None) == -1
    # the iteration prologue: nothing to do at all, too many optimizers, a NULL state
    assert lib.vg_step_prologue(None, None, None, None, None, 0, None, 0, None) == -1
    assert lib.vg_step_prologue(None, None, None, None, None, 5, None, 0, None) == -1
    one = (ctypes.c_double * 1)(1e-3)
    assert lib.vg_step_prologue(None, (ctypes.c_void_p * 1)(None), one, one, one, 1, None, 0, None) == -1
    # round 4: loss slots to zero without a pointer, a negative learning rate (no longer an overload for "prepared"), the
    # prepared form and the two-optimizer form without buffers, the one-launch BatchNorm backward without workspace
    assert lib.vg_step_prologue(None, None, None, None, None, 0, None, 8, None) == -1
    buf = ctypes.c_void_p(64)
    assert lib.vg_adam_step(buf, buf, buf, buf, 4, -1.0, 0.9, 0.999, 1e-8, 1.0, buf, None) == -1
    assert lib.vg_adam_apply(None, None, None, None, 0, 0.9, 0.999, 1e-8, 1.0, None, None) == -1
    assert lib.vg_adam_apply2(None, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.vg_bn_backward_onepass(None, None, None, None, None, None, None, 0, None, None, 0, 64, 1, 0, 0.0, 1, None) == -1
    assert lib.vg_mse_partial(None, None, 0, 1.0, None, None, 0, None, None) == -1
    assert lib.vg_nchw_to_nhwc_pair(None, None, None, 0, 0.0, None, None, 0, 0, 0, 0, 8, 1, None) == -1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No silent fallback: without libvaegan_hip.so every entry into the product raises."""
    from importlib import import_module
    L = import_module("vae-gan-based-model-for-image-generation-and-denoising_amd._lib")
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "libvaegan_hip.so"))
    monkeypatch.setattr(L, "_lib", None)
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        L.load()


def test_torch_custom_op_library_loads_and_registers_the_schemas_without_a_gpu():
    """libvaegan_torch_ops.so (TORCH_LIBRARY(vaegan, ...), csrc_torch/): loads next to libvaegan_hip.so, agrees on the
    ABI version, exposes the schemas; the device ops have no CPU kernel (RuntimeError, never a silent fallback)."""
    import importlib
    ops = importlib.import_module("vae-gan-based-model-for-image-generation-and-denoising_amd.ops")
    t = ops.torch_ops()
    L = importlib.import_module("vae-gan-based-model-for-image-generation-and-denoising_amd._lib")
    assert t.abi_version() == L.ABI_VERSION
    schema = str(torch.ops.vaegan.adam_step.default._schema)
    assert "Tensor(a!) p" in schema and "Tensor(d!) state" in schema
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.adam_step(torch.zeros(8), torch.zeros(8), torch.zeros(8), torch.zeros(8), 1e-3, 0.9, 0.999, 1e-8, 1.0, torch.zeros(4))
    # host-only query through the custom-op face == the C ABI's answer through ctypes
    G = importlib.import_module("vae-gan-based-model-for-image-generation-and-denoising_amd.geometry")
    wg = G.conv_wgrad(8, 32, 32, 64, 128, 4, 2, 1, G.BF16)
    geom = [wg.B, wg.GH, wg.GW, wg.PC, wg.NP, wg.QH, wg.QW, wg.QC, wg.NQ, wg.SY, wg.SX, wg.DY, wg.DX, wg.TH, wg.TW, wg.y0,
            wg.x0, wg.s_np, wg.s_cq, wg.s_t, 0]
    assert t.wgrad_ws_bytes(geom, G.BF16) > 0
