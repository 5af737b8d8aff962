"""The cases of tests/golden/ggn_parent.npz (tools/gen_golden_ggn.py writes it, tests/test_gpu_ggn_stream.py reads it): the
narrow-K direct convolution (csrc/conv_narrowk.hpp) on seeded NORMAL bf16 operands.  tests/_gg_ref.py's integer operands give
the same bits in any order; these do not, so the fixture pins the order of the MFMA chain, of the epilogue and of the
statistics adds (rows of a lane, lanes of a wave, waves of a workgroup) of the build that wrote it.

Every case has 11 images of 11 x 11 output pixels: 1331 pixels = 5 tiles of 256 and a last one of 51."""
import torch

import _gg_ref as R

G = R.G
CASES = {
    # Discriminator's first layer: Conv2d(3 -> 64, k4 s2 p1), bias + LeakyReLU
    "n64_k4s2p1_bias_lrelu": R.Case("ggn<4,4>", "conv", 11, 22, 3, 64, 4, 2, 1, G.BF16, "b+l"),
    # the data gradient of the Generator's last ConvTranspose2d(64 -> 3, k3 s1 p1): a 3 x 3 convolution, statistics
    "n64_k3s1p1_stats": R.Case("ggn<4,3>", "convT_dgrad", 11, 11, 64, 3, 3, 1, 1, G.BF16, "s"),
    # Encoder's first layer: Conv2d(3 -> 32, k4 s2 p0), bias + statistics
    "n32_k4s2p0_bias_stats": R.Case("ggn<2,4>", "conv", 11, 24, 3, 32, 4, 2, 0, G.BF16, "b+s"),
    "n16_k3s1p1_bias_relu": R.Case("ggn<1,3>", "conv", 11, 11, 3, 16, 3, 1, 1, G.BF16, "b+r"),
}
SLOPE = 0.2


def seed_of(name):
    return 7300 + 11 * sorted(CASES).index(name)


def operands(name):
    """-> x NCHW f32 (bf16 values), w f32 in the parameter layout, bias f32 [N] or None: seeded normal."""
    case = CASES[name]
    g, _ = case.specs()
    gen = torch.Generator().manual_seed(seed_of(name))
    x = torch.randn(case.x_shape(), generator=gen).to(torch.bfloat16).float()
    w = (torch.randn(case.w_shape(), generator=gen) * 0.2).float()
    bias = (torch.randn(g.N, generator=gen) * 0.5).float() if case.has("b") else None
    return x, w, bias


def act_of(case):
    return None if case.act is None else (case.act[0], SLOPE if case.act[0] == R.LRELU else 0.0)


def run(ops, name, dev="cuda"):
    """One launch through ops.gather_gemm under the current switches -> (Y bits int16 [B][OH][OW][OC], slab bits int32
    [nparts][2][N] or None), on the CPU.  The plan must be the kernel the case is named for."""
    case = CASES[name]
    g, pk = case.specs()
    x, w, bias = operands(name)
    plan = ops.gather_gemm_plan(g, case.dtype, bias=bias is not None, want_stats=case.has("s"), act=act_of(case))
    assert R.label(plan) == case.label and plan["bm"] == 256, plan
    X = R.x_nhwc(case, x).to(dev)
    Wp = ops.pack_weights(pk, w.flatten().to(dev), case.dtype)
    out = torch.full((g.B, g.OH, g.OW, g.OC), float("nan"), dtype=torch.bfloat16, device=dev)
    if case.has("s"):
        ops.WS.get("stats", plan["nparts"] * 2 * g.N * 4, X.device).fill_(float("nan"))
    Y, stats, nparts = ops.gather_gemm(g, X, Wp, case.dtype, bias=None if bias is None else bias.to(dev),
                                       want_stats=case.has("s"), out=out, act=act_of(case))
    torch.cuda.synchronize()
    yb = Y.view(g.B, g.OH, g.OW, g.OC).cpu().view(torch.int16)
    sb = None if stats is None else stats[: nparts * 2 * g.N].view(nparts, 2, g.N).cpu().view(torch.int32)
    return yb, sb
