"""Network-level sequencing of the HIP kernels: forward and backward of the Encoder, Generator
and Discriminator stacks (main_vae.py:34-58, gan_code.py:16-89) as explicit kernel chains.

No autograd and no ATen compute in here: every stage is
    gather-GEMM (conv / convT / linear, + bias, + BN batch statistics in the epilogue)
 -> bn_finalize (mean / invstd / scale / shift, running-stat update)
 -> fused scale-shift-activation
and the backward chain mirrors it (BN+activation backward in two passes, weight gradient,
data gradient).  Activations live in NHWC; parameters stay in the
reference's fp32 layouts inside the nn.Modules and are re-packed into K-major GEMM operands
whenever they change.

The nn.Module classes in nets.py wrap these chains in torch.autograd.Function objects (drop-in
path); trainer.py drives them directly (fast path, no autograd graph).
"""
from dataclasses import dataclass
import os
from typing import Dict, List, Optional

import torch

from . import geometry as G
from . import ops
from ._lib import VG_ACT_LRELU, VG_ACT_NONE, VG_ACT_RELU, VG_ACT_TANH, VG_FP8_WSHIFT

BN_MOMENTUM, BN_EPS = 0.1, 1e-5       # nn.BatchNorm2d defaults (main_vae.py:24, gan_code.py:22)
# VG_EDGE=0 / VG_EDGE_WGRAD=0 (read once, at import): the 3-channel image layers on the generic gather-GEMM / wgrad kernels
# instead of the edge-layer kernels (csrc/edge_conv.hip, conv_narrowk.hpp) -- A/B and test switch
_EDGE = os.environ.get("VG_EDGE", "1") != "0"
_EDGE_WGRAD = os.environ.get("VG_EDGE_WGRAD", "1") != "0"


def fused_pair(a: torch.Tensor, b: torch.Tensor):
    """[rows_a + rows_b, ...] view over two row-blocks that lie back to back in one allocation (how optim.Adam homes
    the Encoder's fc_mu / fc_logvar parameters and gradients), else None."""
    if a is None or b is None or a.shape[1:] != b.shape[1:] or a.dtype != b.dtype:
        return None
    if not (a.is_contiguous() and b.is_contiguous()):
        return None
    if b.data_ptr() != a.data_ptr() + a.numel() * a.element_size():
        return None
    if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return None
    stride = a.stride() if a.dim() > 1 else (1,)
    return torch.as_strided(a, (a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), stride)


def bump_weights_epoch(params) -> None:
    """Called by optim.Adam after it rewrote `params` behind torch's back (raw-pointer kernel): packed operand
    copies of exactly these parameters become stale (a global counter would re-pack E and G every time D steps)."""
    for p in params:
        p._vg_epoch = getattr(p, "_vg_epoch", 0) + 1


@dataclass
class Stage:
    kind: str                       # 'conv' | 'convT' | 'linear2' | 'head'
    cin: int
    cout: int
    k: int
    s: int
    p: int
    hin: int                        # input spatial size (square)
    hout: int
    conv: object = None             # module(s) owning weight / bias
    conv2: object = None            # second Linear of the fused fc_mu|fc_logvar pair
    bn: object = None
    act: int = VG_ACT_NONE
    slope: float = 0.0

    @property
    def has_bias(self) -> bool:
        return getattr(self.conv, "bias", None) is not None

    def alg(self, B: int, dtype: int):
        """ALGORITHMIC work of one pass (fprop, dgrad or wgrad -- all equal) of this layer for a batch of B:
        FLOP = 2*Cin*Cout*k^2*(Hout^2 | Hin^2 for transposed); bytes = |X| + |Y| + |W|
        at storage width."""
        es = G.esize(dtype)
        if self.kind == "linear2":
            macs = self.cin * self.hin * self.hin * self.cout
            wel = macs
        else:
            sp = self.hin if self.kind == "convT" else self.hout
            macs = self.cin * self.cout * self.k * self.k * sp * sp
            wel = self.cin * self.cout * self.k * self.k
        nbytes = B * (self.hin * self.hin * self.cin + self.hout * self.hout * self.cout) * es + wel * es
        return 2 * B * macs, nbytes


class GradSink:
    """Where parameter gradients go.  direct=True: into param.grad (allocated or accumulated in place -- trainer path);
    direct=False: fresh tensors collected for autograd to return; direct="homed" (the autograd path's default): in place
    for exactly those parameters whose .grad IS their slot of optim.Adam's flat gradient buffer and that are in `wanted`
    (ids of the parameters autograd asked gradients for; None = all) -- every other parameter gets a fresh tensor that
    is returned to autograd, so torch.autograd.grad(), AccumulateGrad hooks and foreign optimizers see real gradients."""

    def __init__(self, direct, wanted=None):
        self.direct = direct
        self.wanted = wanted
        self.out: Dict[int, torch.Tensor] = {}

    def _in_place(self, param: torch.Tensor) -> bool:
        if self.direct != "homed":
            return bool(self.direct)
        if self.wanted is not None and id(param) not in self.wanted:
            return False
        return param.grad is not None and getattr(param, "_vg_homed", None) == param.grad.data_ptr()

    def pair(self, pa: torch.Tensor, pb: torch.Tensor):
        """Gradient tensors of two parameters that one kernel writes as a fused [rows_a + rows_b, ...] block
        -> (grad_a, grad_b, accumulate).  direct: the optimizer's views (back to back when it homed the pair so);
        collected: one fresh allocation split in two."""
        if not (self._in_place(pa) and self._in_place(pb)):
            t = torch.empty((pa.shape[0] + pb.shape[0],) + tuple(pa.shape[1:]), dtype=pa.dtype, device=pa.device)
            ga, gb = t[:pa.shape[0]], t[pa.shape[0]:]
            self.out[id(pa)], self.out[id(pb)] = ga, gb
            return ga, gb, False
        ga, acc_a = self.get(pa)
        gb, acc_b = self.get(pb)
        if acc_a != acc_b:
            raise RuntimeError("fused parameter pair with different accumulation state")
        return ga, gb, acc_a

    def get(self, param: torch.Tensor):
        """-> (tensor to write, accumulate flag)"""
        if not self._in_place(param):
            t = torch.empty_like(param)
            self.out[id(param)] = t
            return t, False
        if param.grad is None:
            param.grad = torch.empty_like(param)
            param._vg_fresh = False
            return param.grad, False
        fresh = getattr(param, "_vg_fresh", False)
        param._vg_fresh = False
        return param.grad, not fresh


class StackEngine:
    """A chain of conv-like stages sharing one activation dtype."""

    def __init__(self, stages: List[Stage], dtype: int, in_ch: int, fp8_fprop: bool = False):
        self.stages = stages
        # forward GEMMs of the wide conv layers on e4m3 operands (bf16 engines only; BASELINE configs[4])
        self.fp8_fprop = bool(fp8_fprop) and dtype == G.BF16
        self.dtype = dtype
        self.in_ch = in_ch
        self._specs: Dict = {}
        self._packs: Optional[Dict] = None
        self._pack_key = None
        self._pack_ptrs = None
        self.pending_bn_ticks = 0           # num_batches_tracked increments not yet applied (flushed lazily)
        # test instrumentation: a list -> backward() appends, per stage, the tensors each kernel group read and wrote
        # (clones), so that a test can re-derive every stage's output from the engine's OWN stored inputs in exact
        # arithmetic (tests/test_gpu_layerwise.py).  None (the default): nothing is recorded.
        self.trace = None
        self.bn_sync = None                 # ddp.GradReducer -> BatchNorm statistics over all ranks (SyncBN mode)

    # ---- geometry (cached per batch size) -----------------------------------------------------
    def spec(self, i: int, B: int, what: str):
        key = (i, B, what)
        sp = self._specs.get(key)
        if sp is None:
            st, dt = self.stages[i], self.dtype
            a = (B, st.hin, st.hin, st.cin, st.cout, st.k, st.s, st.p, dt)
            if st.kind == "conv":
                sp = {"fprop": G.conv_fprop, "dgrad": G.conv_dgrad, "wgrad": G.conv_wgrad}[what](*a)
            elif st.kind == "convT":
                sp = {"fprop": G.convT_fprop, "dgrad": G.convT_dgrad, "wgrad": G.convT_wgrad}[what](*a)
            elif st.kind == "linear2":
                b = (B, st.hin, st.hin, st.cin, st.cout, dt)
                sp = {"fprop": G.linear_fprop, "dgrad": G.linear_dgrad, "wgrad": G.linear_wgrad}[what](*b)
            elif st.kind == "head":
                sp = G.conv_fprop(*a)
            self._specs[key] = sp
        return sp

    def fp8_ok(self, i: int) -> bool:
        """Stage i's forward GEMM reads fp8 operands: a conv / convT whose packed bf16 operand has whole 64-element
        K rows (then the fp8 operand is its elementwise cast) and >= 16 input channels; not the edge layers, and not the
        layers with <= 32 output channels -- HBM-bound streams that gain nothing from a faster MFMA and have a bf16 kernel
        of their own (csrc/conv_phase4.hpp: 2.8x the generic tile the fp8 launch would take)."""
        key = (i, "fp8")
        if key not in self._specs:
            st, ok = self.stages[i], False
            if self.fp8_fprop and st.kind in ("conv", "convT"):
                gg, pk = self.spec(i, 1, "fprop")
                ok = (not pk.tap_in_n and gg.IC % 16 == 0 and gg.Kp % 64 == 0 and gg.N > 32 and
                      self.tn(i, 1, "fprop") is None)
            self._specs[key] = ok
        return self._specs[key]

    def edge_wg(self, i: int, B: int):
        """EWSpec when stage i's weight gradient runs on the edge-layer kernel (3-channel side: first Conv2d of D / E,
        last ConvTranspose2d of G), else None."""
        key = (i, B, "edge_wg")
        if key not in self._specs:
            st, sp = self.stages[i], None
            if _EDGE and _EDGE_WGRAD:
                a = (B, st.hin, st.hin, st.cin, st.cout, st.k, st.s, st.p, self.dtype)
                if st.kind == "conv" and st.cin <= 3 and G.padc(st.cin, self.dtype) == 8:
                    sp = G.conv_wgrad_edge(*a)
                elif st.kind == "convT" and st.cout <= 3 and G.padc(st.cout, self.dtype) == 8:
                    sp = G.convT_wgrad_edge(*a)
            self._specs[key] = sp
        return self._specs[key]

    def tn(self, i: int, B: int, what: str):
        """(TNSpec, PackSpec) when stage i's `what` ('fprop' of a narrow ConvTranspose2d, 'dgrad' of a narrow Conv2d)
        runs on the edge-layer kernel (vg_tnconv) instead of the gather-GEMM, else None.  VG_EDGE=0 turns it off."""
        key = (i, B, "tn_" + what)
        if key not in self._specs:
            st, sp = self.stages[i], None
            if _EDGE and st.bn is None and not st.has_bias:
                a = (B, st.hin, st.hin, st.cin, st.cout, st.k, st.s, st.p, self.dtype)
                if st.kind == "convT" and what == "fprop" and st.act == VG_ACT_NONE:
                    sp = G.convT_fprop_tn(*a)
                elif st.kind == "conv" and what == "dgrad":
                    sp = G.conv_dgrad_tn(*a)
            self._specs[key] = sp
        return self._specs[key]

    # ---- parameter handling ---------------------------------------------------------------------
    def params(self) -> List[torch.Tensor]:
        ps = []
        for st in self.stages:
            for m in (st.conv, st.conv2):
                if m is not None:
                    ps.append(m.weight)
                    if getattr(m, "bias", None) is not None:
                        ps.append(m.bias)
            if st.bn is not None:
                ps += [st.bn.weight, st.bn.bias]
        return ps

    def invalidate(self) -> None:
        self._pack_key = None

    def pack_key(self):
        """What the packed operand copies are valid for: every parameter's (optimizer epoch, torch version) and where the
        first weight lives.  A caller that captures launches reading the packs keys its capture by it (denoise.LatentRefiner)."""
        return (tuple((getattr(p, "_vg_epoch", 0), p._version) for p in self.params()),
                self.stages[0].conv.weight.data_ptr())

    def _ensure_packed(self) -> Dict:
        key = self.pack_key()
        if self._packs is not None and key == self._pack_key:
            return self._packs
        ptr_key = tuple(p.data_ptr() for p in self.params())
        if self._packs is None or self._pack_ptrs != ptr_key:
            self._build_pack_table(ptr_key)
        packs = self._packs
        for i, st in enumerate(self.stages):
            ent = packs[i]
            if st.kind == "linear2":
                if not ent["fused"]:            # parameters not homed back to back (foreign optimizer): device copies
                    n1 = st.conv.weight.shape[0]
                    ent["wcat"][:n1].copy_(st.conv.weight.detach()), ent["wcat"][n1:].copy_(st.conv2.weight.detach())
                    ent["bias"][:n1].copy_(st.conv.bias.detach()), ent["bias"][n1:].copy_(st.conv2.bias.detach())
            else:
                ent["bias"] = st.conv.bias.detach() if st.has_bias else None
        ops.pack_weights_multi(self._pack_table, self._pack_n, self._pack_max, self.dtype)
        for i in range(len(self.stages)):
            if self.fp8_ok(i):                  # e4m3 twin of the forward operand, weights pre-scaled by 2^VG_FP8_WSHIFT
                ops.cast_fp8(packs[i]["fprop"], VG_FP8_WSHIFT, out=packs[i]["fprop8"])
        self._pack_key = key
        return packs

    def _build_pack_table(self, ptr_key) -> None:
        """(Re)allocate the packed operand buffers and the device-side descriptor table (pointers are stable while
        the parameters stay where they are, i.e. after the optimizer re-homed them into its flat buffer)."""
        packs, descs = {}, []
        dev = self.stages[0].conv.weight.device
        for i, st in enumerate(self.stages):
            ent = packs.setdefault(i, {})
            if st.kind == "linear2":
                wv = fused_pair(st.conv.weight.detach(), st.conv2.weight.detach())
                bv = fused_pair(st.conv.bias.detach(), st.conv2.bias.detach())
                ent["fused"] = wv is not None and bv is not None
                if ent["fused"]:                # [fc_mu | fc_logvar] is a view into the optimizer's flat buffer
                    ent["wcat"], ent["bias"] = wv, bv
                else:
                    n1, n2 = st.conv.weight.shape[0], st.conv2.weight.shape[0]
                    ent["wcat"] = torch.empty(n1 + n2, st.conv.weight.shape[1], dtype=torch.float32, device=dev)
                    ent["bias"] = torch.empty(n1 + n2, dtype=torch.float32, device=dev)
                w = ent["wcat"]
            else:
                w = st.conv.weight.detach()
            for what in (("fprop",) if st.kind == "head" else ("fprop", "dgrad")):
                _, pk = self.spec(i, 1, what)
                ent[what] = torch.empty(pk.numel(), dtype=ops.TORCH_DT[self.dtype], device=dev)
                descs.append(ops.pack_desc(pk, w, ent[what]))
                if what == "fprop" and self.fp8_ok(i):
                    ent["fprop8"] = torch.empty(pk.numel(), dtype=torch.uint8, device=dev)
                if st.kind != "head" and self.tn(i, 1, what) is not None:      # edge-layer operand [(kh,kw,n)][C]
                    _, tpk = self.tn(i, 1, what)
                    ent["tn_" + what] = torch.empty(tpk.numel(), dtype=ops.TORCH_DT[self.dtype], device=dev)
                    descs.append(ops.pack_desc(tpk, w, ent["tn_" + what]))
        self._packs, self._pack_ptrs = packs, ptr_key
        (self._pack_table, self._pack_max), self._pack_n = ops.pack_table(descs, dev), len(descs)

    def flush_bn_ticks(self) -> None:
        if self.pending_bn_ticks:
            for st in self.stages:
                if st.bn is not None:
                    st.bn.num_batches_tracked += self.pending_bn_ticks
            self.pending_bn_ticks = 0

    # ---- forward ----------------------------------------------------------------------------------
    def can_group(self, B: int, groups: int, probe_x=None) -> bool:
        """True when `groups` independent batches of B images can run as ONE pass of groups*B images with
        per-group BatchNorm statistics: every statistics slab (one per M tile of the conv kernel) must lie inside
        one group.  Only plain (single-phase) convolution stacks qualify (the Discriminator).  Host only: the tile
        rows come from the launch plan (probe_x, once the device to allocate a probe tensor on, is ignored)."""
        key = ("grp", B, groups)
        if key not in self._specs:
            ok = True
            for i, st in enumerate(self.stages):
                if st.kind == "head":
                    continue
                gg, pk = self.spec(i, B * groups, "fprop")
                if st.bn is None:
                    continue
                if gg.nphase != 1 or pk.tap_in_n:
                    ok = False
                    break
                bm = ops.gather_gemm_plan(gg, G.FP8 if self.fp8_ok(i) else self.dtype, want_stats=True)["bm"]
                if (B * st.hout * st.hout) % bm != 0:
                    ok = False
                    break
            self._specs[key] = ok
        return self._specs[key]

    def check_feat_stage(self, l) -> int:
        """Stage index `l` as a legal tap / feature-loss stage, else ValueError: a stage WITH BatchNorm (a stage without one
        has its activation backward folded into the next stage's dgrad mask, which a gradient added at its output would
        bypass), followed by another stage, whose channel rows carry no padding (the feature loss reads them flat)."""
        if isinstance(l, bool) or not isinstance(l, int) or not 0 <= l < len(self.stages) - 1:
            raise ValueError(f"feature stage must be an integer in [0, {len(self.stages) - 1}) naming a BatchNorm stage, got {l!r}")
        st = self.stages[l]
        if st.kind == "head" or st.bn is None:
            raise ValueError(f"feature stage {l} has no BatchNorm: only BatchNorm stages can be tapped")
        if st.cout != G.padc(st.cout, self.dtype):
            raise ValueError(f"feature stage {l}: {st.cout} channels are padded to {G.padc(st.cout, self.dtype)} in the "
                             f"engine layout, which the feature loss does not handle")
        return l

    def forward(self, x: torch.Tensor, B: int, train: bool, keep: bool = True, groups: int = 1, tail=None, tap=None):
        """x: NHWC activation of the first stage.  Returns (output, ctx).  For a 'head' last stage the
        output is p [B] (f32); otherwise the (activated) NHWC output of the last stage.
        groups > 1: x holds `groups` independent batches of B images (see can_group); BatchNorm statistics,
        running-stat updates and coefficients are per group, in group order.
        tap = l (see check_feat_stage): returns (output, ctx, A_l) with A_l the ACTIVATED output of stage l (after BatchNorm
        and the activation; with keep=True it is ctx[l + 1]["x"]), also when keep=False.  The launches are those of the
        untapped call."""
        if tap is not None:
            self.check_feat_stage(tap)
            if groups != 1:
                raise ValueError("tap needs groups == 1")
        tapped = None
        packs = self._ensure_packed()
        dt = self.dtype
        ctx = []
        a = x
        a8 = None                             # e4m3 twin of `a` when the producing pass already made one (fp8 engines)
        Bg, B = B, B * groups
        for i, st in enumerate(self.stages):
            if st.kind == "head":
                K = st.hin * st.hin * G.padc(st.cin, dt)
                p = ops.dot_sigmoid_forward(a, packs[i]["fprop"], B, K, dt)
                ctx.append({"x": a, "p": p})
                if self.trace is not None:
                    self.trace.append(dict(stage=i, what="head_fwd", x=a.clone(), p=p.clone(), B=B))
                a = p
                continue
            if self.tn(i, B, "fprop") is not None:
                # edge layer (the Generator's last ConvTranspose2d): GEMM + col2im kernel; `tail` = dict(noise, sigma,
                # out_noisy) fuses Tanh, the NCHW f32 image and the instance-noise add (vaegan_code.py:83,92) into it
                tnsp, _ = self.tn(i, B, "fprop")
                OC = G.padc(st.cout, dt)
                if tail is not None and i == len(self.stages) - 1:
                    Yn, img = ops.tnconv(tnsp, a, packs[i]["tn_fprop"], want_nhwc=tail.get("out_noisy") is not None,
                                         want_nchw=True, act=VG_ACT_TANH, noise=tail.get("noise"),
                                         sigma=tail.get("sigma", 0.0), out_nhwc=tail.get("out_noisy"), alg=st.alg(B, dt))
                    out = img
                    Yshape = (B, st.hout, st.hout, OC)
                else:
                    out, _ = ops.tnconv(tnsp, a, packs[i]["tn_fprop"], alg=st.alg(B, dt))
                    Yshape = tuple(out.shape)
                if keep:
                    ctx.append({"x": a, "Y": None, "Yshape": Yshape, "coeffs": None,
                                "rows": B * st.hout * st.hout, "OC": OC})
                if self.trace is not None:
                    self.trace.append(dict(stage=i, what="fwd_tn", x=a.clone(), A=out.clone(), B=B,
                                           noisy=None if (tail is None or tail.get("out_noisy") is None) else tail["out_noisy"].clone()))
                a, a8 = out, None
                continue
            gg, pk = self.spec(i, B, "fprop")
            want_stats = st.bn is not None and train
            # the "taps folded into N" GEMM has one column per (tap, channel): its epilogue sums are not
            # per-channel, so that (tiny) stage takes its BatchNorm statistics from a separate pass
            epilogue_stats = want_stats and not pk.tap_in_n
            # a layer without BatchNorm gets its (Leaky)ReLU in the conv epilogue: "Y" is then the ACTIVATED output,
            # which carries the same sign information the activation's backward needs (slope >= 0)
            fuse_act = st.bn is None and st.act != VG_ACT_NONE
            x8 = None
            if self.fp8_ok(i):
                # e4m3 copy of the input activation (elementwise, same NHWC layout), block-scaled fp8 MFMA, bf16 output
                x8 = a8 if a8 is not None else ops.cast_fp8(a)
                Y, stats, nparts = ops.gather_gemm(gg, x8, packs[i]["fprop8"], G.FP8,
                                                   bias=packs[i]["bias"],
                                                   want_stats=epilogue_stats, alg=st.alg(B, dt),
                                                   act=(st.act, st.slope) if fuse_act else None)
            else:
                Y, stats, nparts = ops.gather_gemm(gg, a, packs[i]["fprop"], dt, bias=packs[i]["bias"],
                                                   want_stats=epilogue_stats, alg=st.alg(B, dt),
                                                   act=(st.act, st.slope) if fuse_act else None)
            OC = G.padc(st.cout, dt)
            Y = Y.view(B, st.hout, st.hout, OC)
            rows = B * st.hout * st.hout
            if want_stats and not epilogue_stats:
                stats, nparts = ops.channel_stats(Y, rows, OC, dt)
            coeffs = None
            if st.bn is not None:
                bn = st.bn
                nxt8 = i + 1 < len(self.stages) and self.stages[i + 1].kind != "head" and self.fp8_ok(i + 1)
                fused = None
                if train and self.bn_sync is None and not nxt8 and st.cout == OC:
                    # small statistics slab: finalize + normalise + activation in one launch
                    fused = ops.bn_finalize_act_forward(Y, stats, nparts, OC, rows, bn.weight.detach(), bn.bias.detach(),
                                                        bn.running_mean, bn.running_var, BN_MOMENTUM, BN_EPS, st.act,
                                                        st.slope, dt, groups=groups)
                if fused is not None:
                    coeffs = fused[0]
                elif train:
                    coeffs = ops.bn_finalize(stats, nparts, st.cout, rows, bn.weight.detach(), bn.bias.detach(),
                                             bn.running_mean, bn.running_var, BN_MOMENTUM, BN_EPS, Y.device,
                                             groups=groups, sync=self.bn_sync)
                else:
                    coeffs = ops.bn_eval_coeffs(bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                                bn.running_var, BN_EPS)
                if fused is not None:
                    out, out8 = fused[1], None
                elif nxt8:                                  # the next layer's fp8 operand comes out of this same pass
                    out, out8 = ops.bn_act_forward(Y, coeffs, rows, OC, st.act, st.slope, dt, want_fp8=True)
                else:
                    out, out8 = ops.bn_act_forward(Y, coeffs, rows, OC, st.act, st.slope, dt), None
            else:
                out, out8 = Y, None                         # activation (if any) already applied by the epilogue
            if keep:
                ctx.append({"x": a, "Y": Y, "coeffs": coeffs, "rows": rows, "OC": OC})
            if self.trace is not None:
                self.trace.append(dict(stage=i, what="fwd", x=a.clone(), Y=Y.clone(), A=out.clone(), groups=groups, B=B,
                                       coeffs=None if coeffs is None else coeffs.clone(), fused_act=fuse_act,
                                       x8=None if x8 is None else x8.clone(), nparts=nparts))
            a, a8 = out, out8
            if i == tap:
                tapped = out
        if train and any(st.bn is not None for st in self.stages):
            self.pending_bn_ticks += groups
        if tap is not None:
            return a, (ctx, B, train), tapped
        return a, (ctx, B, train)

    # ---- backward ---------------------------------------------------------------------------------
    def param_stage(self) -> Dict[int, int]:
        """id(parameter) -> index of the stage whose backward produces its gradient (ddp bucket planning)."""
        out = {}
        for i, st in enumerate(self.stages):
            for m in (st.conv, st.conv2, st.bn):
                if m is not None:
                    for p in m.parameters(recurse=False):
                        out[id(p)] = i
        return out

    def backward(self, ctxpack, dout: torch.Tensor, need_dx: bool, sink: GradSink, param_grads: bool = True,
                 on_grads=None, head_loss=None, feat=None, weight_grad_groups: int = 1):
        """dout: gradient w.r.t. forward()'s output.  Returns the gradient w.r.t. the NHWC input (or None).
        param_grads=False skips every weight/bias/BN-parameter gradient (legal when the caller discards
        them, e.g. the generator-loss pass through the discriminator).
        on_grads(i): called right after every parameter gradient of stage i has been enqueued (stages run
        last-to-first) -- the data-parallel trainer launches a gradient bucket's all-reduce from it.
        head_loss = (target0, target1, groups, gscale, loss_slot, accumulate): instead of `dout`, for a stack that ends
        in the Discriminator's head -- the BCE of its output probabilities against target0 (first group of rows) / target1
        (second group), its gradient, the sigmoid backward and the head's data / weight gradients run as ONE launch
        (ops.head_backward; vaegan_code.py:99-104, :115); loss_slot[0] (+)= the loss.  groups = 3 takes a seventh entry,
        target2 (third group of rows; ops.head_backward_g: the prior stream's Discriminator update).
        feat = (l, f_real, gscale, loss_slot): the Discriminator-feature reconstruction loss at stage l (check_feat_stage):
        when the loop reaches stage l, BEFORE its BatchNorm backward, ops.feat_mse_forward_backward writes
        loss_slot[0] = mean((A_l - f_real)^2) and adds gscale * 2 (A_l - f_real) / n onto dA in place (A_l = ctx[l + 1]["x"],
        the activation this pass stored; f_real a constant of the same shape) -- dA then carries both branches.
        weight_grad_groups = g > 1, for a grouped pass (forward(groups=g)): every convolution / head WEIGHT gradient is formed
        group after group over that group's rows, the later ones accumulating -- the launches, and therefore the bits, of g
        separate passes (one launch over all rows sums in another order).  Everything else of a grouped backward already is
        what separate passes compute, bit for bit: the BatchNorm backward and its parameter gradients are per group, a data
        gradient's rows do not mix.
        A context of forward(train=False, keep=True) is accepted with param_grads=False only: every BatchNorm stage then runs
        ops.bn_act_backward_eval on the constant coefficients its forward used (no statistics pass, no parameter gradient), the
        rest of the chain is the train-mode one; sync / feat / weight_grad_groups are refused (ValueError), param_grads=True
        raises the RuntimeError it always raised.
        Everything runs on the current stream: forking weight gradients onto a second stream (three schedules, rounds 1
        and 2) measured slower every time and is gone ("Concurrency does not pay")."""
        ctx, B, train = ctxpack
        if not train:
            # a context of forward(train=False, keep=True): data gradients only (test-time latent refinement).
            # BatchNorm is then a constant per-channel scale and shift, whose backward needs no statistics pass
            if param_grads:
                raise RuntimeError("backward through an eval-mode network is not supported (the reference never does it)")
            if self.bn_sync is not None or feat is not None or weight_grad_groups != 1:
                raise ValueError("an eval-mode backward takes no SyncBN, no feat and no weight_grad_groups: its BatchNorm "
                                 "has no batch statistics and it forms no weight gradient")
        if feat is not None:
            self.check_feat_stage(feat[0])
        packs = self._ensure_packed()
        dt = self.dtype
        dA = dout
        masked = False                      # dA already carries the activation backward of the stage it belongs to
        for i in range(len(self.stages) - 1, -1, -1):
            st, c = self.stages[i], ctx[i]
            want_dx = need_dx or i > 0
            if st.kind == "head" and head_loss is not None:
                K = st.hin * st.hin * G.padc(st.cin, dt)
                t0, t1, grp, gscale, slot, acc_loss = head_loss[:6]
                gw, acc = sink.get(st.conv.weight) if param_grads else (None, False)
                if grp == 3:
                    split = gw is not None and weight_grad_groups > 1     # the launch leaves dlogit, the weight gradient follows
                    dlogit = torch.empty_like(c["p"]) if split else None
                    dA = ops.head_backward_g(c["p"], c["x"], packs[i]["fprop"], B // grp, (t0, t1, head_loss[6]), gscale, slot,
                                             acc_loss, None if split else gw, acc, K, G.padc(st.cin, dt), st.hin * st.hin, dt,
                                             want_dx, dlogit=dlogit)
                    if split:
                        self._head_wgrad(st, c["x"], dlogit, gw, acc, B, K, weight_grad_groups)
                else:
                    dA = ops.head_backward(c["p"], c["x"], packs[i]["fprop"], B // grp, grp, t0, t1, gscale, slot, acc_loss,
                                           gw, acc, K, G.padc(st.cin, dt), st.hin * st.hin, dt, want_dx)
                if self.trace is not None:
                    self.trace.append(dict(stage=i, what="head_bwd", p=c["p"].clone(), x=c["x"].clone(), dp=None,
                                           bce=(t0, t1, grp, gscale) + tuple(head_loss[6:7]),
                                           dX=None if dA is None else dA.clone(), acc=acc,
                                           gw=None if gw is None else gw.clone()))
                if param_grads and on_grads is not None:
                    on_grads(i)
                continue
            if st.kind == "head":
                K = st.hin * st.hin * G.padc(st.cin, dt)
                dx, dlogit = ops.dot_sigmoid_backward(c["p"], dA, packs[i]["fprop"], B, K, dt, want_dx, c["x"])
                gw, acc = None, False
                if param_grads:
                    gw, acc = sink.get(st.conv.weight)
                    self._head_wgrad(st, c["x"], dlogit, gw, acc, B, K, weight_grad_groups)
                    if on_grads is not None:
                        on_grads(i)
                if self.trace is not None:
                    self.trace.append(dict(stage=i, what="head_bwd", p=c["p"].clone(), x=c["x"].clone(), dp=dA.clone(),
                                           bce=None, dX=None if dx is None else dx.clone(), acc=acc,
                                           gw=None if gw is None else gw.clone()))
                dA = dx
                continue
            Y, rows, OC = c["Y"], c["rows"], c["OC"]
            yshape = c["Yshape"] if Y is None else Y.shape
            dA = dA.view(yshape) if dA.shape != yshape else dA
            if feat is not None and i == feat[0]:
                _, f_real, fscale, fslot = feat
                # f_real has the rows the loss is taken over: all of this pass's, or the leading group of a grouped pass (the
                # reconstruction's half of the prior stream's [reconstruction | decoded prior samples] pass)
                nf = f_real.shape[0]
                f_fake, dA_f = ctx[i + 1]["x"][:nf], dA[:nf]
                dA_in = dA_f.clone() if self.trace is not None else None
                ops.feat_mse_forward_backward(f_fake, f_real.view(f_fake.shape), dA_f, fscale, fslot, False, dt)
                if self.trace is not None:
                    self.trace.append(dict(stage=i, what="feat", f_fake=f_fake.clone(), f_real=f_real.clone(), dA_in=dA_in,
                                           dA=dA_f.clone(), gscale=fscale, loss=fslot.clone()))
            gg_, gb_, acc_g = None, None, False
            if st.bn is not None and not train:
                dY = ops.bn_act_backward_eval(Y, dA, c["coeffs"], rows, OC, st.act, st.slope, dt)
            elif st.bn is not None:
                if param_grads:
                    gg_, acc_g = sink.get(st.bn.weight)
                    gb_, acc_b = sink.get(st.bn.bias)
                    assert acc_g == acc_b
                dY = ops.bn_act_backward(Y, dA, c["coeffs"], rows, OC, rows, st.bn.weight.detach(), st.act, st.slope,
                                         gg_, gb_, acc_g, dt, sync=self.bn_sync)
            elif st.act != VG_ACT_NONE and not masked:
                dY = ops.act_backward(Y, dA, st.act, st.slope, dt)
            else:
                dY = dA                                     # no activation, or its backward was fused into the dgrad above
            if self.trace is not None:
                self.trace.append(dict(stage=i, what="bn_bwd", dA=dA.clone(), dY=dY.clone(), Y=None if Y is None else Y.clone(),
                                       coeffs=None if c["coeffs"] is None else c["coeffs"].clone(), masked_in=masked,
                                       dgamma=None if gg_ is None else gg_.clone(), dbeta=None if gb_ is None else gb_.clone(),
                                       acc_bn=acc_g))
            masked = False
            if param_grads:
                acc_before = st.conv.weight.grad is not None and not getattr(st.conv.weight, "_vg_fresh", False)
                self._param_grads(i, st, c, dY, B, rows, OC, sink, weight_grad_groups)
                if on_grads is not None:
                    on_grads(i)
                if self.trace is not None:
                    self.trace.append(dict(stage=i, what="wgrad", dY=dY.clone(), x=c["x"].clone(), acc=acc_before,
                                           gw=None if st.conv.weight.grad is None else st.conv.weight.grad.detach().clone(),
                                           gw2=None if (st.conv2 is None or st.conv2.weight.grad is None) else st.conv2.weight.grad.detach().clone(),
                                           gb=None if not st.has_bias or st.conv.bias.grad is None else st.conv.bias.grad.detach().clone(),
                                           gb2=None if (st.conv2 is None or st.conv2.bias.grad is None) else st.conv2.bias.grad.detach().clone()))
            if want_dx and self.tn(i, B, "dgrad") is not None:
                tnsp, _ = self.tn(i, B, "dgrad")            # image gradient below a narrow first Conv2d (edge layer)
                dX, _ = ops.tnconv(tnsp, dY, packs[i]["tn_dgrad"], alg=st.alg(B, dt))
                dA = dX.view(c["x"].shape)
                if self.trace is not None:
                    self.trace.append(dict(stage=i, what="dgrad", dY=dY.clone(), dX=dA.clone(), mask=None))
            elif want_dx:
                ggd, _ = self.spec(i, B, "dgrad")
                mask = None
                if i > 0:
                    pst, pc = self.stages[i - 1], ctx[i - 1]
                    # the stage below has an activation but no BatchNorm: its backward is a mask on this dgrad's output
                    if pst.bn is None and pst.act != VG_ACT_NONE and pst.kind != "head" and ggd.N == pst.cout and \
                            ggd.OC == pc["OC"]:
                        mask = (pc["Y"], pst.act, pst.slope)
                        masked = True
                dX, _, _ = ops.gather_gemm(ggd, dY, packs[i]["dgrad"], dt, alg=st.alg(B, dt), mask=mask)
                dA = dX.view(c["x"].shape)
                if self.trace is not None:
                    self.trace.append(dict(stage=i, what="dgrad", dY=dY.clone(), dX=dA.clone(),
                                           mask=None if mask is None else (mask[0].clone(), mask[1], mask[2])))
            else:
                dA = None
        return dA

    def _head_wgrad(self, st, x, dlogit, gw, acc, B, K, groups=1):
        """The head's weight gradient over B rows, as `groups` accumulating launches over B / groups rows each."""
        Bg, dt = B // groups, self.dtype
        for g in range(groups):
            rows = slice(g * Bg, (g + 1) * Bg)
            ops.dot_wgrad(x[rows], dlogit[rows], gw, Bg, K, G.padc(st.cin, dt), st.hin * st.hin, acc or g > 0, dt)

    def _param_grads(self, i, st, c, dY, B, rows, OC, sink, groups=1):
        dt = self.dtype
        if groups > 1:
            # a grouped pass, weight gradient group after group (backward: weight_grad_groups).  Only bias-free convolutions
            # run grouped (the Discriminator, can_group)
            if st.kind != "conv" or st.has_bias:
                raise RuntimeError("weight_grad_groups needs a stack of bias-free convolutions")
            gw, acc = sink.get(st.conv.weight)
            Bg = B // groups
            wg, ew = self.spec(i, Bg, "wgrad"), self.edge_wg(i, Bg)
            for g in range(groups):
                dYg, xg = dY[g * Bg:(g + 1) * Bg], c["x"][g * Bg:(g + 1) * Bg]
                if ew is not None and gw.is_contiguous():
                    ops.edge_wgrad(ew, dYg, xg, gw, acc or g > 0, alg=st.alg(Bg, dt))
                else:
                    ops.wgrad(wg, dYg, xg, gw, acc or g > 0, dt, alg=st.alg(Bg, dt))
            return
        wg = self.spec(i, B, "wgrad")
        if st.kind == "linear2":
            # one wgrad / one bias reduction for the fused [fc_mu | fc_logvar] head, written straight into the pair's
            # gradient storage when the two gradients lie back to back (optim.Adam's flat buffer; GradSink.pair)
            (gw1, gw2, accw), (gb1, gb2, accb) = sink.pair(st.conv.weight, st.conv2.weight), sink.pair(st.conv.bias, st.conv2.bias)
            fw, fb = fused_pair(gw1, gw2), fused_pair(gb1, gb2)
            if fw is not None and fb is not None:
                ops.wgrad(wg, dY, c["x"], fw, accw, dt, alg=st.alg(B, dt))
                ops.bias_grad(dY, rows, OC, st.cout, fb, accb, dt)
                return
            N1 = st.conv.weight.shape[0]
            tmp = torch.empty(st.cout, st.conv.weight.shape[1], dtype=torch.float32, device=dY.device)
            ops.wgrad(wg, dY, c["x"], tmp, False, dt, alg=st.alg(B, dt))
            tb = torch.empty(st.cout, dtype=torch.float32, device=dY.device)
            ops.bias_grad(dY, rows, OC, st.cout, tb, False, dt)
            for g, src, acc in ((gw1, tmp[:N1], accw), (gw2, tmp[N1:], accw), (gb1, tb[:N1], accb), (gb2, tb[N1:], accb)):
                if acc:
                    ops.axpy(g, src.contiguous(), 1.0, out=g)
                else:
                    g.copy_(src.view(g.shape))                 # contiguous device copy (hipMemcpyAsync), no ATen kernel
            return
        gw, acc = sink.get(st.conv.weight)
        ew = self.edge_wg(i, B)
        if ew is not None and gw.is_contiguous():
            # wide operand = the many-channel side, narrow = the 3-channel side (conv: dY / input image; convT: input / dY)
            wide, narrow = (dY, c["x"]) if st.kind == "conv" else (c["x"], dY)
            ops.edge_wgrad(ew, wide, narrow, gw, acc, alg=st.alg(B, dt))
        elif st.kind == "conv":
            ops.wgrad(wg, dY, c["x"], gw, acc, dt, alg=st.alg(B, dt))
        else:
            ops.wgrad(wg, c["x"], dY, gw, acc, dt, alg=st.alg(B, dt))
        if st.has_bias:
            gb, accb = sink.get(st.conv.bias)
            if st.bn is not None:
                # A conv bias directly in front of a train-mode BatchNorm (main_vae.py:23-24): the batch mean removes it,
                # so its gradient -- the column sums of the BatchNorm backward's output -- is IDENTICALLY ZERO in exact
                # arithmetic (sum_m dx = a*sum(dz) - N*a*mean(dz) - b*sum(xhat) = 0).  What the reference's autograd
                # returns there is the fp32 rounding residue of that expression (|g| ~ 1e-8, a different residue in every
                # implementation; tests/test_gpu_parity.py skips these tensors for that reason).  The engine writes the
                # exact value, 0: no column-reduce + finalize launches (8 per iteration at S=64).  The slot is zeroed once
                # and left alone while nothing else has written it.
                if not accb and getattr(st.conv.bias, "_vg_zero_slot", None) != gb.data_ptr():
                    ops.memset_zero(gb)
                    # (remembered only for a slot of optim.Adam's flat gradient buffer, which nothing else writes; any
                    # other gradient tensor may be a recycled allocation and is zeroed every time)
                    # ... and only when the memset really ran: one that was merely RECORDED into a hipGraph capture (which
                    # may still abort) proves nothing about the slot's contents
                    homed = bool(sink.direct) and getattr(st.conv.bias, "_vg_homed", None) == gb.data_ptr() and \
                        not torch.cuda.is_current_stream_capturing()
                    st.conv.bias._vg_zero_slot = gb.data_ptr() if homed else None
            else:
                ops.bias_grad(dY, rows, OC, st.cout, gb, accb, dt)
