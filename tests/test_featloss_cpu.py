"""No GPU: the references the Discriminator-feature reconstruction loss is tested against (tests/_featloss_ref.py) are
themselves checked -- the f64 kernel restatement against torch.autograd, ref_step against the oracle it extends -- and
the host-side argument checks of vg_feat_mse_forward_backward against the built library."""
import ctypes
import os
import re
from importlib import import_module

import pytest
import torch
import torch.nn.functional as F

import _featloss_ref as FR
import vaegan_ref as R
from _inputs import make_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"


@pytest.mark.parametrize("n,gscale", [(8, 1.0), (8 * 1001, 0.37), (2 * 16 * 16 * 128, 0.1)])
def test_f64_restatement_equals_autograd_of_mse_loss(n, gscale):
    g = torch.Generator().manual_seed(n)
    a = torch.randn(n, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(n, generator=g, dtype=torch.float64)
    d_in = torch.randn(n, generator=g, dtype=torch.float64)
    loss = F.mse_loss(a, b)
    lv = float(loss.detach())
    # the gradient-add: d(total)/da where total = <d_in, a> + gscale * mse(a, b), i.e. a non-zero gradient arriving from above
    ((d_in * a).sum() + gscale * loss).backward()
    # two f64 sums of the same n non-negative terms in different orders: at most n 2^-52 relative apart
    assert abs(float(FR.feat_mse(a.detach(), b)) - lv) <= n * 2.0 ** -52 * lv
    grad, added = FR.feat_mse_grad_add(a.detach(), b, d_in, gscale)
    assert torch.allclose(added, a.grad, rtol=1e-14, atol=1e-18)
    # (a.grad - d_in cancels: its own rounding error is an ulp of |d_in| ~ 1, i.e. up to ~1e-15 absolute)
    assert torch.allclose(grad, a.grad - d_in, rtol=1e-12, atol=2e-15)
    assert torch.equal(FR.feat_mse_grad_add(a.detach(), b, None, gscale)[1], grad)


def test_stage_map_names_the_batchnorm_stages():
    s64, s256 = R.discriminator_spec(img_size=64), R.discriminator_spec(img_size=256)
    assert FR.feature_stages(s64) == [1, 2, 3] and FR.feature_stages(s256) == [1, 2, 3, 4, 5]
    # 64 -> 128 @ 16^2, 128 -> 256 @ 8^2, 256 -> 512 @ 4^2
    for l, cout in ((1, 128), (2, 256), (3, 512)):
        k = FR.stage_prefix_len(s64, l)
        assert s64[k - 3][:3] == ("conv", cout // 2, cout) and s64[k - 2] == ("bn", cout) and s64[k - 1] == ("lrelu", 0.2)
    for bad in (0, 4, -1, 7):
        with pytest.raises(ValueError):
            FR.stage_prefix_len(s64, bad)


def _walk_eval(st, spec, x):
    """The Discriminator's Sequential entry by entry in eval mode, under its own state_dict keys -> every intermediate."""
    outs = []
    for i, ent in enumerate(spec):
        if ent[0] == "conv":
            x = F.conv2d(x, st[f"main.{i}.weight"], None, stride=ent[4], padding=ent[5])
        elif ent[0] == "bn":
            x = F.batch_norm(x, st[f"main.{i}.running_mean"], st[f"main.{i}.running_var"], st[f"main.{i}.weight"],
                             st[f"main.{i}.bias"], False, R.BN_MOMENTUM, R.BN_EPS)
        elif ent[0] == "lrelu":
            x = F.leaky_relu(x, ent[1])
        else:
            assert ent[0] == "sigmoid"
            x = torch.sigmoid(x)
        outs.append(x)
    return outs


def test_prefix_forward_equals_the_full_forwards_intermediate():
    S, B = 64, 3
    o = R.RefVAEGAN(img_size=S, seed=42)
    x = make_inputs(B, S, 11)[0]
    clone = lambda st: {k: v.detach().clone() for k, v in st.items()}      # noqa: E731
    with torch.no_grad():
        outs = _walk_eval(o.D, o.d_spec, x)
        plain = clone(o.D)
        p_train = R.discriminator_forward(plain, o.d_spec, x, True)
        for l in FR.feature_stages(o.d_spec):
            st = clone(o.D)
            p, f = FR.d_forward_tapped(st, o.d_spec, x, l, False)
            assert f.shape == (B, 64 << l, 32 >> l, 32 >> l)
            assert torch.equal(f, outs[3 * l + 1]) and torch.equal(p, outs[-1].view(-1))
            assert all(torch.equal(v, o.D[k]) for k, v in st.items()), "an eval-mode call moved a buffer"
            # train mode: the whole stack runs -- output and EVERY BatchNorm buffer as after one plain call
            p, f = FR.d_forward_tapped(st, o.d_spec, x, l, True)
            assert torch.equal(p, p_train)
            for k, v in st.items():
                assert torch.equal(v, plain[k]), k
            assert int(st["main.3.num_batches_tracked"]) == 1 and not torch.equal(st["main.9.running_mean"], o.D["main.9.running_mean"])


def test_ref_step_with_the_feature_off_is_the_oracle_step_bit_for_bit():
    S, B = 64, 2
    a, b = R.RefVAEGAN(img_size=S, seed=42), R.RefVAEGAN(img_size=S, seed=42)
    inp = make_inputs(B, S, 7000 + S)
    la = a.train_step(*inp, 60)
    lb = FR.ref_step(b, *inp, 60, feat_layer=2, alpha_feat=0.0, alpha_pix=1.0)
    assert lb.pop("feat_loss") == 0.0
    assert la == lb
    for sa, sb in ((a.E, b.E), (a.G, b.G), (a.D, b.D)):
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    for oa, ob in ((a.opt_E, b.opt_E), (a.opt_G, b.opt_G), (a.opt_D, b.opt_D)):
        assert oa.t == ob.t
        for x, y in zip(oa.exp_avg + oa.exp_avg_sq, ob.exp_avg + ob.exp_avg_sq):
            assert torch.equal(x, y)


def test_ref_step_with_the_feature_on_moves_what_it_should():
    S, B = 64, 2
    a, b = R.RefVAEGAN(img_size=S, seed=42), R.RefVAEGAN(img_size=S, seed=42)
    inp = make_inputs(B, S, 7000 + S)
    la = a.train_step(*inp, 60)
    lb = FR.ref_step(b, *inp, 60, feat_layer=2, alpha_feat=1.0)
    assert lb["feat_loss"] > 0 and abs(lb["total"] - la["total"] - lb["feat_loss"]) <= 1e-5 * abs(lb["total"])
    # up to the Generator + VAE section nothing changed; D's parameters are not updated there; its BatchNorms saw one more call
    for k in ("recon_loss", "kl_loss", "d_loss_1", "d_loss_2"):
        assert la[k] == lb[k]
    for k in a.D:
        if k.endswith("num_batches_tracked"):
            assert int(b.D[k]) == int(a.D[k]) + 1 == 6
        elif not (k.endswith("running_mean") or k.endswith("running_var")):
            assert torch.equal(a.D[k], b.D[k]), k
    assert not torch.equal(a.opt_G.exp_avg[0], b.opt_G.exp_avg[0])


def test_c_abi_rejects_bad_feature_loss_arguments_on_host():
    """Validation happens before any launch (pattern: test_host_cpu.test_c_abi_rejects_bad_arguments_on_host)."""
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION >= 16
    assert "vg_feat_mse_forward_backward" in L.SIGNATURES
    f = lib.vg_feat_mse_forward_backward
    buf, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    EINVAL, EALIGN, ENOSUP = -1, -2, -3
    assert f(None, None, None, 0, 1.0, None, 0, None, 0, 0, None) == EINVAL
    assert f(None, buf, None, 8, 1.0, buf, 0, buf, 1024, 0, None) == EINVAL        # f_fake NULL
    assert f(buf, None, None, 8, 1.0, buf, 0, buf, 1024, 1, None) == EINVAL        # f_real NULL
    assert f(buf, buf, None, 0, 1.0, buf, 0, buf, 1024, 0, None) == EINVAL         # n = 0
    assert f(buf, buf, None, -8, 1.0, buf, 0, buf, 1024, 0, None) == EINVAL        # n < 0
    assert f(buf, buf, None, 8, 1.0, None, 0, buf, 1024, 0, None) == EINVAL        # no loss slot
    assert f(buf, buf, None, 8, 1.0, buf, 0, None, 1024, 0, None) == EINVAL        # no workspace
    assert f(buf, buf, None, 8, 1.0, buf, 0, buf, 0, 0, None) == EINVAL            # workspace capacity 0
    for dt in (2, 7, -1):                                                          # fp8 storage / unknown dtypes
        assert f(buf, buf, buf, 8, 1.0, buf, 0, buf, 1024, dt, None) == ENOSUP
    assert f(odd, buf, None, 8, 1.0, buf, 0, buf, 1024, 0, None) == EALIGN
    assert f(buf, odd, None, 8, 1.0, buf, 0, buf, 1024, 1, None) == EALIGN
    assert f(buf, buf, odd, 8, 1.0, buf, 0, buf, 1024, 1, None) == EALIGN
