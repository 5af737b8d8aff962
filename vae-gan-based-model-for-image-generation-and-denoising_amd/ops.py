"""Thin tensor-level wrappers over the C ABI (libvaegan_hip.so).

Each function takes torch CUDA tensors (used only as device-memory handles), fills the
descriptor struct, and launches on torch's current HIP stream.  No computation happens in
Python/ATen here.  All functions raise RuntimeError when the library rejects the arguments.
"""
import ctypes
import math
import os
from ctypes import byref, c_int

import torch

from . import _lib as L
from .geometry import BF16, F32, FP8, EWSpec, GGSpec, PackSpec, TNSpec, WGSpec, esize

TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, FP8: torch.uint8}      # e4m3 bytes travel as uint8


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("vaegan_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
        if t is not None and not t.is_contiguous():
            raise RuntimeError("vaegan_amd ops need contiguous tensors")


class _Workspace:
    """Grow-only scratch buffers, one per (device, tag); all users are ordered on one stream.
    A buffer that is outgrown is RETIRED, never freed: captured hipGraphs (trainer.train_step_graphed, the sibling
    trainers) hold raw pointers into the buffers that existed when they were captured, and a later, larger eager
    call (another trainer, a bigger validation batch) must not hand that memory back to the allocator under them.
    Growth is geometric, so the retired buffers sum to less than four times the live one."""

    def __init__(self):
        self.bufs = {}
        self.retired = []

    def get(self, tag: str, nbytes: int, device) -> torch.Tensor:
        key = (tag, str(device))
        buf = self.bufs.get(key)
        if buf is None or buf.numel() * 4 < nbytes:
            n = max(int(nbytes * 1.25) // 4 + 64, 1 << 16)
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"workspace '{tag}' would grow during graph capture; run a warm-up step first")
            if buf is not None:
                self.retired.append(buf)
            buf = torch.empty(n, dtype=torch.float32, device=device)
            self.bufs[key] = buf
        return buf


WS = _Workspace()


def reload_switches() -> None:
    """Re-read the library's optional VG_* kernel-selection switches from the environment (they are read once, when the
    library is loaded: include/vaegan_hip.h vg_reload_switches).  For tests / A-B scripts that flip one in-process."""
    L.check(L.load().vg_reload_switches(), "vg_reload_switches")


class KernelTimer:
    """Live timing of the GEMM-class launches (bench.py's roofline leg): the library brackets each kernel with a
    HIP start/stop event pair on its launch stream (vg_timing_*); this object only adds up the algorithmic
    FLOP / bytes of the same launches.  Off by default."""
    # "bn": every launch of csrc/bn_act.hip -- BatchNorm finalize / normalise + activation / backward reduce + apply,
    # plain activation backward, bias-gradient column sums: HBM-bound passes over the activation tensors
    FAMILIES = {"gather_gemm": 0, "wgrad": 1, "edge": 2, "gather_gemm_fp8": 3, "bn": 4}

    def __init__(self):
        self.acc = {k: dict(flops=0, bytes=0) for k in self.FAMILIES}
        L.load().vg_timing_enable(1)

    def add(self, family, flops, nbytes):
        self.acc[family]["flops"] += flops
        self.acc[family]["bytes"] += nbytes

    def summary(self):
        """family -> dict(launches, ms, flops, bytes); synchronises the recorded events and stops timing."""
        import ctypes
        out = {}
        lib = L.load()
        for fam, idx in self.FAMILIES.items():
            ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
            L.check(lib.vg_timing_collect(idx, ctypes.byref(ms), ctypes.byref(n)), "vg_timing_collect")
            out[fam] = dict(launches=n.value, ms=ms.value, **self.acc[fam])
        lib.vg_timing_enable(0)
        return out


TIMER = None


def _bn_bytes(passes: int, numel: int, dtype: int) -> None:
    """Algorithmic HBM bytes of a BatchNorm / activation pass for bench.py's roofline_bn: `passes` tensor-sized streams
    (forward: read the raw output, write the activated one = 2; backward: reduce reads x and dy, apply reads x and dy and
    writes dx = 5; the small statistics / coefficient vectors are not counted)."""
    if TIMER is not None:
        TIMER.add("bn", 0, passes * numel * (4 if dtype == F32 else 2))

# ---- binding ---------------------------------------------------------------------------------------------------------
# The kernels live behind the C ABI (include/vaegan_hip.h).  Two faces reach it from Python:
#   "ctypes"   (default)  _lib.py marshals pointers and descriptor structs;
#   "torchops"            the PyTorch-ROCm custom-op face: torch.ops.vaegan.* registered by libvaegan_torch_ops.so
#                         (csrc_torch/vaegan_torch_ops.cpp, TORCH_LIBRARY + TORCH_LIBRARY_IMPL(CUDA)), a thin shim over
#                         the SAME entry points.  Covers the GEMM-class and optimizer launches (gather_gemm, wgrad,
#                         adam_step, bn_act_forward, pack_weights_multi); host-only queries stay on ctypes.
# Select with VG_BINDING=torchops or ops.set_binding("torchops"); results are bit-identical (tests/test_gpu_binding.py).
BINDING = "ctypes"
_TORCH_OPS = None


def torch_ops():
    """torch.ops.vaegan, loading libvaegan_torch_ops.so on first use (RuntimeError if it was not built)."""
    global _TORCH_OPS
    if _TORCH_OPS is None:
        import os
        path = os.path.join(os.path.dirname(L.LIB_PATH), "libvaegan_torch_ops.so")
        if not os.path.isfile(path):
            raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L.load()                                   # libvaegan_hip.so first: the shim links against it
        torch.ops.load_library(path)
        if torch.ops.vaegan.abi_version() != L.ABI_VERSION:
            raise RuntimeError("libvaegan_torch_ops.so was built against another libvaegan_hip ABI; rebuild")
        _TORCH_OPS = torch.ops.vaegan
    return _TORCH_OPS


def set_binding(name: str) -> None:
    global BINDING
    if name not in ("ctypes", "torchops"):
        raise ValueError("binding must be 'ctypes' or 'torchops'")
    if name == "torchops":
        torch_ops()
    BINDING = name


def _gg_geom(d) -> list:
    return ([d.B, d.GH, d.GW, d.IH, d.IW, d.IC, d.SY, d.SX, d.DY, d.DX, d.TH, d.TW] + list(d.y0) + list(d.x0) +
            [d.N, d.Kp, d.OH, d.OW, d.OC, d.OSY, d.OSX] + list(d.ooy) + list(d.oox) +
            [d.nphase, d.stats_capacity, d.act, d.mask_act])


def _wg_geom(d) -> list:
    return [d.B, d.GH, d.GW, d.PC, d.NP, d.QH, d.QW, d.QC, d.NQ, d.SY, d.SX, d.DY, d.DX, d.TH, d.TW, d.y0, d.x0,
            d.s_np, d.s_cq, d.s_t, d.accumulate]


def set_timer(t) -> None:
    global TIMER
    TIMER = t


def empty_act(shape, dtype: int, device) -> torch.Tensor:
    return torch.empty(shape, dtype=TORCH_DT[dtype], device=device)


def zeros_f32(n: int, device) -> torch.Tensor:
    """f32 zeros through hipMemsetAsync (no ATen fill kernel)."""
    t = torch.empty(n, dtype=torch.float32, device=device)
    L.check(L.load().vg_memset_zero(t.data_ptr(), n * 4, L.stream_ptr()), "vg_memset_zero")
    return t


def memset_zero(t: torch.Tensor) -> None:
    _need_cuda(t)
    L.check(L.load().vg_memset_zero(t.data_ptr(), t.numel() * t.element_size(), L.stream_ptr()), "vg_memset_zero")


class NoiseDraw:
    """One of the N(0,1) draws of an iteration, generated inside the kernel that consumes it (vg_*_rng)."""
    __slots__ = ("state", "draw")

    def __init__(self, state: torch.Tensor, draw: int):
        self.state, self.draw = state, draw


class NoiseStream:
    """Device-resident generator for the in-kernel draws (include/vaegan_hip.h "In-kernel N(0,1) noise"):
    int64[2] = {seed, iteration counter}.  advance() is a one-thread kernel, captured with the iteration."""

    def __init__(self, device, seed: int):
        self.seed = int(seed)
        self.state = torch.tensor([self.seed & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=device)
        if not self.state.is_cuda:
            raise RuntimeError("NoiseStream lives on the MI355X ('cuda'); there is no CPU path")

    def advance(self) -> None:
        L.check(L.load().vg_rng_advance(self.state.data_ptr(), L.stream_ptr()), "vg_rng_advance")

    def draw(self, k: int) -> NoiseDraw:
        return NoiseDraw(self.state, k)

    def randn(self, shape, k: int) -> torch.Tensor:
        """Materialise draw k of the current iteration (exactly what the *_rng kernels consume)."""
        out = torch.empty(shape, dtype=torch.float32, device=self.state.device)
        L.check(L.load().vg_randn(out.data_ptr(), out.numel(), self.state.data_ptr(), k, L.stream_ptr()), "vg_randn")
        return out

    def get_state(self):
        return self.state.clone()

    def set_state(self, st: torch.Tensor) -> None:
        self.state.copy_(st.to(self.state.device))


_NOISE = {}


def reset_noise() -> None:
    """Forget the per-device default noise streams: the next draw starts a fresh stream at iteration 0, keyed by
    torch's current device seed (utils.configure_seed calls this)."""
    _NOISE.clear()


def default_noise(device) -> NoiseStream:
    """Per-device stream seeded from torch's device generator seed (utils.configure_seed / torch.cuda.manual_seed
    govern it, as they govern torch.randn_like in the reference); re-seeding torch starts a new stream."""
    key = str(device)
    seed = torch.cuda.initial_seed()
    ns = _NOISE.get(key)
    if ns is None or ns.seed != seed:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the noise stream cannot be (re)created during graph capture; run a warm-up step first")
        ns = NoiseStream(device, seed)
        _NOISE[key] = ns
    return ns


# ---------------------------------------------------------------------------------------------
def pack_weights(pk: PackSpec, w: torch.Tensor, dtype: int, out: torch.Tensor = None) -> torch.Tensor:
    _need_cuda(w, out)
    if w.dtype != torch.float32:
        raise RuntimeError("parameters must be float32 (fp32 master weights)")
    if out is None:
        out = torch.empty(pk.numel(), dtype=TORCH_DT[dtype], device=w.device)
    L.check(L.load().vg_pack_weights(byref(pack_desc(pk, w, out)), dtype, L.stream_ptr()), "vg_pack_weights")
    return out


def pack_desc(pk: PackSpec, w: torch.Tensor, out: torch.Tensor) -> L.PackDesc:
    return L.PackDesc(src=w.data_ptr(), dst=out.data_ptr(), nphase=pk.nphase, N=pk.N, C=pk.C, IC=pk.IC, TH=pk.TH,
                      TW=pk.TW, Kp=pk.Kp, s_n=pk.s_n, s_c=pk.s_c, KW=pk.KW, kh0=L.i4(pk.kh0), kw0=L.i4(pk.kw0),
                      kh_step=pk.kh_step, kw_step=pk.kw_step, tap_in_n=pk.tap_in_n, KHW=pk.KHW)


def pack_table(descs, device):
    """Descriptor table in device memory for pack_weights_multi (built once per network).
    Returns (table, total_tiles); fills every descriptor's tile_start (flat one-workgroup-per-tile launch)."""
    import ctypes
    lib = L.load()
    total = 0
    for d in descs:
        d.tile_start = total
        nt = lib.vg_pack_tile_count(byref(d))
        if nt <= 0:
            L.check(nt if nt < 0 else -1, "vg_pack_tile_count")
        total += nt
    arr = (L.PackDesc * len(descs))(*descs)
    raw = bytes(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr)))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device), total


def pack_weights_multi(table: torch.Tensor, n: int, total_tiles: int, dtype: int) -> None:
    if BINDING == "torchops":
        torch_ops().pack_weights_multi(table, n, total_tiles, dtype)
        return
    L.check(L.load().vg_pack_weights_multi(table.data_ptr(), n, total_tiles, dtype, L.stream_ptr()),
            "vg_pack_weights_multi")


_ZEROS = {}


def zero_page(device) -> torch.Tensor:
    z = _ZEROS.get(str(device))
    if z is None:
        z = zeros_f32(64, device)                                     # 256 zero bytes
        _ZEROS[str(device)] = z
    return z


_SOME = 64                # a plan query only tests pointers against NULL and for 16-byte alignment: stands in for a tensor
_WS_ENOUGH = 1 << 62      # ... and for the size of a workspace that is allocated from the plan's ws_bytes


def _addr(t) -> int:
    """Descriptor pointer: the tensor's; True -> the query placeholder (a buffer supplied after planning); None -> NULL."""
    return 0 if t is None or t is False else _SOME if t is True else t.data_ptr()


def _gg_desc(g: GGSpec, X, Wp, Y, zeros, bias=None, stats=None, act=None, mask=None, ws=None) -> L.GGDesc:
    """The one place a vg_gg_desc is filled, for the plan query and for the launch.  Every operand: a tensor, True (see
    _addr) or None.  act = (code, slope); mask = (code, slope) or (tensor, code, slope)."""
    d = L.GGDesc(zeros=_addr(zeros), X=_addr(X), W=_addr(Wp), Y=_addr(Y), bias=_addr(bias), stats=_addr(stats),
                 B=g.B, GH=g.GH, GW=g.GW, IH=g.IH, IW=g.IW, IC=g.IC, SY=g.SY, SX=g.SX, DY=g.DY, DX=g.DX,
                 TH=g.TH, TW=g.TW, y0=L.i4(g.y0), x0=L.i4(g.x0), N=g.N, Kp=g.Kp, OH=g.OH, OW=g.OW, OC=g.OC,
                 OSY=g.OSY, OSX=g.OSX, ooy=L.i4(g.ooy), oox=L.i4(g.oox), nphase=g.nphase,
                 ws=_addr(ws), ws_bytes=_WS_ENOUGH if ws is True else 0)
    if act is not None:                      # (code, slope): activation of a BatchNorm-less layer, fused in the epilogue
        d.act, d.act_slope = act
    if mask is not None:                     # (activated output of the layer below, code, slope): its activation backward, fused
        d.mask_x, d.mask_act, d.mask_slope = _addr(mask[0] if len(mask) == 3 else True), mask[-2], mask[-1]
    return d


def _gg_plan(d: L.GGDesc, dtype: int) -> L.GGPlan:
    p = L.GGPlan()
    L.check(L.load().vg_gather_gemm_plan(byref(d), dtype, byref(p)), "vg_gather_gemm_plan")
    return p


def _wg_desc(wg: WGSpec, P, Q, dW, zeros, accumulate=False) -> L.WGDesc:
    """The one place a vg_wg_desc is filled, for the plan query and for the launch (operands as in _gg_desc); the launch
    adds the workspace the plan asks for."""
    return L.WGDesc(P=_addr(P), Q=_addr(Q), dW=_addr(dW), zeros=_addr(zeros), B=wg.B, GH=wg.GH, GW=wg.GW, PC=wg.PC, NP=wg.NP,
                    QH=wg.QH, QW=wg.QW, QC=wg.QC, NQ=wg.NQ, SY=wg.SY, SX=wg.SX, DY=wg.DY, DX=wg.DX, TH=wg.TH, TW=wg.TW,
                    y0=wg.y0, x0=wg.x0, s_np=wg.s_np, s_cq=wg.s_cq, s_t=wg.s_t, accumulate=1 if accumulate else 0)


def _wg_plan(d: L.WGDesc, dtype: int) -> L.WGPlan:
    p = L.WGPlan()
    L.check(L.load().vg_wgrad_plan(byref(d), dtype, byref(p)), "vg_wgrad_plan")
    return p


def _ew_desc(ew: EWSpec, wide, narrow, dW, zeros, accumulate=False) -> L.EWDesc:
    """The same for vg_ew_desc."""
    return L.EWDesc(Wd=_addr(wide), Nr=_addr(narrow), dW=_addr(dW), zeros=_addr(zeros), B=ew.B, WH=ew.WH, WW=ew.WW, C=ew.C,
                    NH=ew.NH, NW=ew.NW, N=ew.N, K=ew.K, S=ew.S, P=ew.P, s_c=ew.s_c, s_n=ew.s_n,
                    accumulate=1 if accumulate else 0)


def _ew_plan(d: L.EWDesc) -> L.EWPlan:
    p = L.EWPlan()
    L.check(L.load().vg_edge_wgrad_plan(byref(d), byref(p)), "vg_edge_wgrad_plan")
    return p


def gather_gemm(g: GGSpec, X: torch.Tensor, Wp: torch.Tensor, dtype: int, bias: torch.Tensor = None,
                want_stats: bool = False, out: torch.Tensor = None, alg=None, act=None, mask=None):
    """Returns (Y [B,OH,OW,OC], stats slabs or None, nparts).  alg = (flops, bytes) of the layer for the timer.
    Two library calls: the plan, asked with placeholders for the statistics slabs and the split-K workspace, sizes both
    and names the timer family; the launch then runs from the same record (include/vaegan_hip.h, vg_gg_plan)."""
    _need_cuda(X, Wp, bias, out)
    if X.dtype != TORCH_DT[dtype] or Wp.dtype != TORCH_DT[dtype]:
        raise RuntimeError(f"gather_gemm: operand dtype {X.dtype}/{Wp.dtype} does not match engine dtype")
    if X.numel() != g.B * g.IH * g.IW * g.IC:
        raise RuntimeError(f"gather_gemm: input has {X.numel()} elements, geometry expects "
                           f"{(g.B, g.IH, g.IW, g.IC)}")
    if Wp.numel() != g.nphase * g.N * g.Kp:
        raise RuntimeError("gather_gemm: packed weight size mismatch")
    Y = out if out is not None else empty_act((g.B, g.OH, g.OW, g.OC), BF16 if dtype == FP8 else dtype, X.device)
    if Y.numel() != g.B * g.OH * g.OW * g.OC:
        raise RuntimeError("gather_gemm: output size mismatch")
    if mask is not None and (mask[0].numel() != Y.numel() or mask[0].dtype != Y.dtype):
        raise RuntimeError("gather_gemm: mask tensor must be shaped and typed like the output")
    d = _gg_desc(g, X, Wp, Y, zero_page(X.device), bias, stats=want_stats, act=act, mask=mask, ws=True)
    p = _gg_plan(d, dtype)
    stats = WS.get("stats", p.nparts * 2 * g.N * 4, X.device) if want_stats else None
    ws = WS.get("splitk", p.ws_bytes, X.device) if p.ws_bytes > 0 else None
    d.stats, d.stats_capacity = _addr(stats), p.nparts
    d.ws, d.ws_bytes = _addr(ws), ws.numel() * 4 if ws is not None else 0
    if TIMER is not None:
        TIMER.add({0: "gather_gemm", 2: "edge", 3: "gather_gemm_fp8"}[p.timing_family], *(alg or (g.flops(), 0)))
    if BINDING == "torchops":
        torch_ops().gather_gemm(X, Wp, Y, bias, stats, ws, zero_page(X.device), mask[0] if mask is not None else None,
                                _gg_geom(d), float(d.act_slope), float(d.mask_slope), dtype)
    else:
        L.check(L.load().vg_gather_gemm(byref(d), dtype, L.stream_ptr()), "vg_gather_gemm")
    return Y, stats, p.nparts


def edge_wgrad(ew: EWSpec, wide: torch.Tensor, narrow: torch.Tensor, dW: torch.Tensor, accumulate: bool, alg=None) -> None:
    """Weight gradient of an edge layer (vg_edge_wgrad): wide [B,WH,WW,C] bf16, narrow [B,NH,NW,8] bf16, dW f32."""
    _need_cuda(wide, narrow, dW)
    if wide.dtype != torch.bfloat16 or narrow.dtype != torch.bfloat16 or dW.dtype != torch.float32:
        raise RuntimeError("edge_wgrad: bf16 operands, float32 gradient")
    if wide.numel() != ew.B * ew.WH * ew.WW * ew.C or narrow.numel() != ew.B * ew.NH * ew.NW * 8:
        raise RuntimeError("edge_wgrad: operand size mismatch")
    d = _ew_desc(ew, wide, narrow, dW, zero_page(wide.device), accumulate)
    ws = WS.get("wgrad", _ew_plan(d).ws_bytes, wide.device)
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    if TIMER is not None:
        TIMER.add("wgrad", *(alg or (ew.flops(), 0)))
    L.check(L.load().vg_edge_wgrad(byref(d), L.stream_ptr()), "vg_edge_wgrad")


def cast_fp8(x: torch.Tensor, shift: int = 0, out: torch.Tensor = None) -> torch.Tensor:
    """bf16 -> e4m3 bytes (uint8 tensor of the same shape), y = fp8(x * 2^shift)."""
    _need_cuda(x, out)
    if x.dtype != torch.bfloat16 or x.numel() % 8:
        raise RuntimeError("cast_fp8: bf16 input with a multiple of 8 elements")
    y = out if out is not None else torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    L.check(L.load().vg_cast_fp8(x.data_ptr(), y.data_ptr(), x.numel(), shift, L.stream_ptr()), "vg_cast_fp8")
    return y


def tnconv(tn: TNSpec, X: torch.Tensor, Wp: torch.Tensor, want_nhwc: bool = True, want_nchw: bool = False,
           act: int = 0, noise=None, sigma: float = 0.0, out_nhwc: torch.Tensor = None, alg=None):
    """Narrow-N transposed convolution (vg_tnconv) -> (Y NHWC bf16 [B,OH,OW,OC] or None, Y NCHW f32 or None).
    noise: None, an NCHW f32 tensor [B,N,OH,OW] or a NoiseDraw; with noise, Y = act(.) + sigma*noise."""
    rng = isinstance(noise, NoiseDraw)
    _need_cuda(X, Wp, None if rng else noise, out_nhwc)
    if X.dtype != torch.bfloat16 or Wp.dtype != torch.bfloat16:
        raise RuntimeError("tnconv: bf16 operands only")
    if X.numel() != tn.B * tn.IH * tn.IW * tn.C or Wp.numel() != tn.K * tn.K * tn.N * tn.Wpitch:
        raise RuntimeError("tnconv: operand size mismatch")
    Y = None
    if want_nhwc:
        Y = out_nhwc if out_nhwc is not None else torch.empty(tn.B, tn.OH, tn.OW, tn.OC, dtype=torch.bfloat16, device=X.device)
        if Y.numel() != tn.B * tn.OH * tn.OW * tn.OC:
            raise RuntimeError("tnconv: output size mismatch")
    Yc = torch.empty(tn.B, tn.N, tn.OH, tn.OW, dtype=torch.float32, device=X.device) if want_nchw else None
    if noise is not None and not rng and noise.numel() != tn.B * tn.N * tn.OH * tn.OW:
        raise RuntimeError("tnconv: noise tensor must be [B,N,OH,OW]")
    d = L.TNDesc(X=X.data_ptr(), Wp=Wp.data_ptr(), Y=0 if Y is None else Y.data_ptr(),
                 Y_nchw=0 if Yc is None else Yc.data_ptr(),
                 eps=noise.data_ptr() if (noise is not None and not rng) else 0,
                 rng=noise.state.data_ptr() if rng else 0, draw=noise.draw if rng else 0, sigma=sigma,
                 B=tn.B, IH=tn.IH, IW=tn.IW, C=tn.C, N=tn.N, K=tn.K, S=tn.S, P=tn.P, OH=tn.OH, OW=tn.OW, OC=tn.OC,
                 Wpitch=tn.Wpitch, act=act)
    if TIMER is not None:
        TIMER.add("edge", *(alg or (tn.flops(), 0)))
    L.check(L.load().vg_tnconv(byref(d), L.stream_ptr()), "vg_tnconv")
    return Y, Yc


def wgrad(wg: WGSpec, P: torch.Tensor, Q: torch.Tensor, dW: torch.Tensor, accumulate: bool, dtype: int,
          alg=None) -> None:
    _need_cuda(P, Q, dW)
    if dW.dtype != torch.float32:
        raise RuntimeError("weight gradients are float32")
    if P.numel() != wg.B * wg.GH * wg.GW * wg.PC or Q.numel() != wg.B * wg.QH * wg.QW * wg.QC:
        raise RuntimeError("wgrad: operand size mismatch")
    d = _wg_desc(wg, P, Q, dW, zero_page(P.device), accumulate)
    # the slab workspace is shared by all launches of one stream; work forked onto another stream gets its own
    ws = WS.get("wgrad", _wg_plan(d, dtype).ws_bytes, P.device)
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    if TIMER is not None:
        TIMER.add("wgrad", *(alg or (0, 0)))
    if BINDING == "torchops":
        torch_ops().wgrad(P, Q, dW, ws, zero_page(P.device), _wg_geom(d), dtype)
    else:
        L.check(L.load().vg_wgrad(byref(d), dtype, L.stream_ptr()), "vg_wgrad")


# ---------------------------------------------------------------------------------------------
GG_FAMILY = {0: "generic", 1: "narrowk", 2: "phase4", 3: "patch"}
GG_REDUCE = {0: "none", 1: "flat", 2: "tile"}


def gather_gemm_plan(g: GGSpec, dtype: int, bias: bool = False, want_stats: bool = False, act=None, mask=None,
                     workspace=True, zeros: bool = True) -> dict:
    """What vg_gather_gemm launches for this geometry and epilogue under the current switches (vg_gather_gemm_plan: the
    record the launcher itself launches from, and the one gather_gemm sizes its buffers from).  Host only, no GPU and no
    tensors: the descriptor's pointers are only tested against NULL by the query, so placeholders stand in for them --
    bias / want_stats / mask say which are set, as in gather_gemm (which always passes the zero page, and the workspace
    the plan asks for).  workspace: True (as gather_gemm: a workspace of ws_bytes will be supplied), False (none), or the
    bytes of the one that is passed.
    -> dict(family, bm, bn, detail, dma, ksplit, stages_per_split, nstages, reduce, n_major, nparts, timing_family, ws_bytes);
    bm = rows covered by one BatchNorm statistics slab."""
    d = _gg_desc(g, True, True, True, zeros, bias, stats=want_stats, act=act, mask=mask, ws=bool(workspace))
    if workspace is not True and workspace:
        d.ws_bytes = int(workspace)
    p = _gg_plan(d, dtype)
    return dict(family=GG_FAMILY[p.family], bm=p.bm, bn=p.bn, detail=(p.detail[0], p.detail[1]), dma=bool(p.dma),
                ksplit=p.ksplit, stages_per_split=p.stages_per_split, nstages=p.nstages, reduce=GG_REDUCE[p.reduce],
                n_major=bool(p.n_major), nparts=p.nparts, timing_family=p.timing_family, ws_bytes=p.ws_bytes)


WG_MAIN = {0: "f32", 1: "bf16_reg", 2: "bf16_dma", 3: "ws"}
WG_REDUCE = {0: "stream", 1: "generic"}


def wgrad_plan(wg: WGSpec, dtype: int, zeros: bool = True, aligned16: bool = True) -> dict:
    """What vg_wgrad launches for this geometry under the current switches (vg_wgrad_plan: the record the launcher itself
    launches from, and the one wgrad sizes its workspace from).  Host only, no GPU and no tensors.  zeros: whether the
    zero page is passed (wgrad always does); aligned16: whether dW is 16-byte aligned.
    -> dict of the fields of vg_wg_plan, main and reduce by name (WG_MAIN, WG_REDUCE)."""
    d = _wg_desc(wg, True, True, True, zeros)
    if not aligned16:
        d.dW = _SOME + 4
    p = _wg_plan(d, dtype)
    return dict({name: getattr(p, name) for name, _ in L.WGPlan._fields_}, main=WG_MAIN[p.main], reduce=WG_REDUCE[p.reduce],
                xcd_order=bool(p.xcd_order))


def edge_wgrad_plan(ew: EWSpec) -> dict:
    """What vg_edge_wgrad launches for this geometry (vg_edge_wgrad_plan).  Host only -> dict of the fields of vg_ew_plan."""
    p = _ew_plan(_ew_desc(ew, True, True, True, True))
    return {name: getattr(p, name) for name, _ in L.EWPlan._fields_}


def tnconv_plan(tn: TNSpec, rng: bool = False) -> dict:
    """What vg_tnconv launches for this geometry (vg_tnconv_plan: the record the launcher itself launches from).  Host
    only, no GPU and no tensors.  rng: whether the noise is drawn in-kernel (tnconv with a NoiseDraw) -- the only pointer
    of the descriptor the query looks at.  -> dict of the fields of vg_tn_plan, quad_noise as a bool."""
    d = L.TNDesc(rng=_addr(bool(rng)), B=tn.B, IH=tn.IH, IW=tn.IW, C=tn.C, N=tn.N, K=tn.K, S=tn.S, P=tn.P, OH=tn.OH, OW=tn.OW,
                 OC=tn.OC, Wpitch=tn.Wpitch)
    p = L.TNPlan()
    L.check(L.load().vg_tnconv_plan(byref(d), byref(p)), "vg_tnconv_plan")
    return dict({name: getattr(p, name) for name, _ in L.TNPlan._fields_}, quad_noise=bool(p.quad_noise))


def bn_finalize(stats, nparts, C, count, gamma, beta, running_mean, running_var, momentum, eps, device, groups=1,
                sync=None):
    """-> coeffs tensor [groups][4][C]: mean, invstd, scale, shift.  With groups > 1 the slabs of group g are
    parts [g*nparts/groups, ...) and the running statistics are updated group after group (the order in which
    the reference runs its separate forward passes).  sync: None, or an object with .world and
    .all_reduce_sum(tensor) (ddp.GradReducer) -> statistics over the global batch of all ranks."""
    co = torch.empty(groups, 4, C, dtype=torch.float32, device=device)
    npg = nparts // groups
    if sync is not None:
        # synchronised BatchNorm: per-group f64 sums -> ONE all-reduce -> coefficients from the global sums
        sums = torch.empty(groups, 2, C, dtype=torch.float64, device=device)
        for g in range(groups):
            L.check(L.load().vg_slab_sums(stats.data_ptr() + g * npg * 2 * C * 4, npg, C, sums[g].data_ptr(),
                                          L.stream_ptr()), "vg_slab_sums")
        sync.all_reduce_sum(sums)
        for g in range(groups):
            L.check(L.load().vg_bn_finalize_sums(sums[g].data_ptr(), C, (count // groups) * sync.world,
                                                 L.ptr(gamma), L.ptr(beta), L.ptr(running_mean), L.ptr(running_var),
                                                 momentum, eps, co[g, 0].data_ptr(), co[g, 1].data_ptr(),
                                                 co[g, 2].data_ptr(), co[g, 3].data_ptr(), L.stream_ptr()),
                    "vg_bn_finalize_sums")
        return co
    L.check(L.load().vg_bn_finalize_grouped(stats.data_ptr(), npg, groups, C, count // groups, L.ptr(gamma), L.ptr(beta),
                                            L.ptr(running_mean), L.ptr(running_var), momentum, eps, co.data_ptr(),
                                            L.stream_ptr()), "vg_bn_finalize_grouped")
    return co


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps):
    C = running_mean.numel()
    co = torch.empty(1, 4, C, dtype=torch.float32, device=running_mean.device)
    L.check(L.load().vg_bn_eval_coeffs(L.ptr(gamma), L.ptr(beta), L.ptr(running_mean), L.ptr(running_var), eps, C,
                                       co[0, 2].data_ptr(), co[0, 3].data_ptr(), L.stream_ptr()), "vg_bn_eval_coeffs")
    return co


def bn_act_forward(x, coeffs, rows, C, act, slope, dtype, out=None, want_fp8=False):
    """coeffs: [groups][4][C] (or None for a pure activation).  want_fp8: -> (y, e4m3 copy of y as uint8)."""
    _need_cuda(x, coeffs)
    y = out if out is not None else torch.empty_like(x)
    groups = coeffs.shape[0] if coeffs is not None else 1
    _bn_bytes(2, x.numel(), dtype)
    if want_fp8:
        y8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        L.check(L.load().vg_bn_act_forward_fp8(x.data_ptr(), y.data_ptr(), y8.data_ptr(),
                                               coeffs[0, 2].data_ptr() if coeffs is not None else 0,
                                               coeffs[0, 3].data_ptr() if coeffs is not None else 0, rows, C, act, slope,
                                               groups, 4 * C, dtype, L.stream_ptr()), "vg_bn_act_forward_fp8")
        return y, y8
    if BINDING == "torchops":
        torch_ops().bn_act_forward(x, y, coeffs[0, 2] if coeffs is not None else None,
                                   coeffs[0, 3] if coeffs is not None else None, rows, C, act, float(slope), groups, 4 * C, dtype)
        return y
    sc = coeffs[0, 2].data_ptr() if coeffs is not None else 0
    sh = coeffs[0, 3].data_ptr() if coeffs is not None else 0
    L.check(L.load().vg_bn_act_forward(x.data_ptr(), y.data_ptr(), sc, sh, rows, C, act, slope, groups, 4 * C, dtype,
                                       L.stream_ptr()), "vg_bn_act_forward")
    return y


def bn_finalize_act_forward(x, stats, nparts, C, rows, gamma, beta, running_mean, running_var, momentum, eps, act, slope,
                            dtype, groups=1):
    """Train-mode finalize + normalise + activation in one launch where the statistics slab is small
    (bn_act.hip bn_fin_act_fwd_kernel).  Returns (coeffs [groups][4][C], y), or None when the shape does not qualify
    (the caller then runs bn_finalize + bn_act_forward)."""
    lib = L.load()
    if x.shape[-1] != C or not bn_launch_plan("fused", rows, C, dtype, groups, nparts=nparts // groups)["fused"]:
        return None
    _need_cuda(x, stats)
    co = torch.empty(groups, 4, C, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    _bn_bytes(2, x.numel(), dtype)
    L.check(lib.vg_bn_finalize_act_forward(x.data_ptr(), y.data_ptr(), stats.data_ptr(), nparts // groups, groups, C, rows,
                                           L.ptr(gamma), L.ptr(beta), L.ptr(running_mean), L.ptr(running_var), momentum, eps,
                                           co.data_ptr(), act, slope, dtype, L.stream_ptr()), "vg_bn_finalize_act_forward")
    return co, y


def channel_stats(x, rows, C, dtype):
    n = c_int(0)
    cap = 1024
    stats = WS.get("stats", cap * 2 * C * 4, x.device)
    _bn_bytes(1, x.numel(), dtype)
    L.check(L.load().vg_channel_stats(x.data_ptr(), rows, C, stats.data_ptr(), cap, byref(n), dtype, L.stream_ptr()),
            "vg_channel_stats")
    return stats, n.value


_GRID_SYNC = {}


def grid_sync_words(device) -> torch.Tensor:
    """The zero-initialised counter words of the kernels that synchronise their whole grid (csrc/bn_onepass.hip): int32[16],
    [0] arrivals, [1] departures (both back at zero after every launch), [2] sticky error (a bounded wait gave up)."""
    key = str(device)
    t = _GRID_SYNC.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("grid-sync words would be allocated during graph capture; run a warm-up step first")
        t = torch.zeros(16, dtype=torch.int32, device=device)
        _GRID_SYNC[key] = t
    return t


def grid_sync_error(device) -> bool:
    """True when a grid-wide wait of some earlier launch gave up (results of that launch are invalid).  Synchronises."""
    t = _GRID_SYNC.get(str(device))
    return bool(t is not None and int(t[2].item()) != 0)


def bn_act_backward(x, dy, coeffs, rows, C, count, gamma, act, slope, dgamma, dbeta, accumulate, dtype, sync=None):
    """Full BN(+act) backward: returns dx (gradient w.r.t. the raw conv output).  coeffs: [groups][4][C]."""
    _need_cuda(x, dy, coeffs)
    lib = L.load()
    groups = coeffs.shape[0]
    if sync is None and x.shape[-1] == C and lib.vg_bn_backward_onepass_supported(rows, C, groups, dtype):
        # one launch: the workgroups keep their x / dy rows in registers across a grid-wide exchange of the partial sums
        # (csrc/bn_onepass.hip): 3 tensor-sized streams instead of 5, no finalize launch
        _bn_bytes(3, x.numel(), dtype)
        slab = WS.get("bn1pass", lib.vg_bn_backward_onepass_ws_bytes(rows, C, groups, dtype), x.device)
        dx = torch.empty_like(x)
        L.check(lib.vg_bn_backward_onepass(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), coeffs.data_ptr(), L.ptr(gamma),
                                           L.ptr(dgamma), L.ptr(dbeta), 1 if accumulate else 0, slab.data_ptr(),
                                           grid_sync_words(x.device).data_ptr(), rows, C, groups, act, slope, dtype,
                                           L.stream_ptr()), "vg_bn_backward_onepass")
        return dx
    n = c_int(0)
    cap = 2048
    _bn_bytes(5, x.numel(), dtype)
    partial = WS.get("bnbwd", cap * 2 * C * 4, x.device)
    L.check(lib.vg_bn_act_backward_reduce(x.data_ptr(), dy.data_ptr(), coeffs[0, 2].data_ptr(),
                                          coeffs[0, 3].data_ptr(), coeffs[0, 0].data_ptr(), coeffs[0, 1].data_ptr(),
                                          rows, C, act, slope, partial.data_ptr(), cap, byref(n), groups, 4 * C,
                                          dtype, L.stream_ptr()), "vg_bn_act_backward_reduce")
    if sync is None and x.shape[-1] == C and bn_launch_plan("fused", rows, C, dtype, groups, nparts=n.value)["fused"]:
        # small layer: finalize + apply in one launch (bn_act.hip bn_bwd_fin_apply_kernel); n = partial rows PER GROUP
        dx = torch.empty_like(x)
        L.check(lib.vg_bn_backward_finalize_apply(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), partial.data_ptr(),
                                                  n.value, groups, C, rows, L.ptr(gamma), coeffs.data_ptr(),
                                                  L.ptr(dgamma), L.ptr(dbeta), 1 if accumulate else 0, act, slope, dtype,
                                                  L.stream_ptr()), "vg_bn_backward_finalize_apply")
        return dx
    coef = torch.empty(groups, 3, C, dtype=torch.float32, device=x.device)
    if sync is not None:
        lsums = torch.empty(groups, 2, C, dtype=torch.float64, device=x.device)
        for g in range(groups):
            L.check(lib.vg_slab_sums(partial.data_ptr() + g * n.value * 2 * C * 4, n.value, C, lsums[g].data_ptr(),
                                     L.stream_ptr()), "vg_slab_sums")
        gsums = lsums.clone()
        sync.all_reduce_sum(gsums)
        for g in range(groups):
            L.check(lib.vg_bn_backward_finalize_sums(gsums[g].data_ptr(), lsums[g].data_ptr(), C,
                                                     (count // groups) * sync.world, L.ptr(gamma),
                                                     coeffs[g, 1].data_ptr(), L.ptr(dgamma), L.ptr(dbeta),
                                                     1 if (accumulate or g > 0) else 0, coef[g].data_ptr(),
                                                     L.stream_ptr()), "vg_bn_backward_finalize_sums")
    if sync is None:
        L.check(lib.vg_bn_backward_finalize_grouped(partial.data_ptr(), n.value, groups, C, count // groups, L.ptr(gamma),
                                                    coeffs.data_ptr(), L.ptr(dgamma), L.ptr(dbeta),
                                                    1 if accumulate else 0, coef.data_ptr(), L.stream_ptr()),
                "vg_bn_backward_finalize_grouped")
    dx = torch.empty_like(x)
    L.check(lib.vg_bn_act_backward_apply(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), coeffs[0, 2].data_ptr(),
                                         coeffs[0, 3].data_ptr(), coeffs[0, 0].data_ptr(), coeffs[0, 1].data_ptr(),
                                         coef.data_ptr(), rows, C, act, slope, groups, 4 * C, 3 * C, dtype,
                                         L.stream_ptr()), "vg_bn_act_backward_apply")
    return dx


BN_PLAN_KIND = {"reduce": 0, "forward": 1, "apply": 2, "fused": 3}


def bn_launch_plan(kind: str, rows: int, C: int, dtype: int, groups: int = 1, aligned16: bool = True, nparts: int = 0) -> dict:
    """What the BatchNorm launcher of this kind ("reduce", "forward", "apply", "fused") launches for a [rows][C] tensor of
    `groups` equal row blocks under the current switches (vg_bn_launch_plan: the record the launchers themselves launch
    from).  Host only, no GPU and no tensors.  nparts: slab rows PER GROUP, read by "fused" only.
    -> dict(vec, threads_per_row, rows_per_pass, rows_per_block, blocks_per_group, col_blocks, groups, fused)."""
    p = L.BNPlan()
    L.check(L.load().vg_bn_launch_plan(BN_PLAN_KIND[kind], rows, C, groups, dtype, 1 if aligned16 else 0, nparts, byref(p)),
            "vg_bn_launch_plan")
    return dict(vec=p.vec, threads_per_row=p.threads_per_row, rows_per_pass=p.rows_per_pass,
                rows_per_block=p.rows_per_block, blocks_per_group=p.blocks_per_group, col_blocks=p.col_blocks,
                groups=p.groups, fused=bool(p.fused))


def act_backward(x, dy, act, slope, dtype):
    dx = torch.empty_like(x)
    _bn_bytes(3, x.numel(), dtype)
    L.check(L.load().vg_act_backward(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), act, slope, dtype,
                                     L.stream_ptr()), "vg_act_backward")
    return dx


def bias_grad(dy, rows, C, NC, dbias, accumulate, dtype):
    cap = 1024
    _bn_bytes(1, rows * C, dtype)
    ws = WS.get("biasgrad", cap * 2 * C * 4, dy.device)
    L.check(L.load().vg_bias_grad(dy.data_ptr(), rows, C, NC, dbias.data_ptr(), 1 if accumulate else 0,
                                  ws.data_ptr(), cap, dtype, L.stream_ptr()), "vg_bias_grad")


# ---------------------------------------------------------------------------------------------
def nchw_to_nhwc(x, CP, dtype, eps=None, sigma=0.0, out=None):
    """eps: None, an NCHW f32 noise tensor, or a NoiseDraw (generated inside the kernel)."""
    _need_cuda(x, None if isinstance(eps, NoiseDraw) else eps, out)
    B, C, H, W = x.shape
    y = out if out is not None else empty_act((B, H, W, CP), dtype, x.device)
    if isinstance(eps, NoiseDraw):
        L.check(L.load().vg_nchw_to_nhwc_rng(x.data_ptr(), eps.state.data_ptr(), eps.draw, sigma, y.data_ptr(), B, C, H,
                                             W, CP, dtype, L.stream_ptr()), "vg_nchw_to_nhwc_rng")
        return y
    L.check(L.load().vg_nchw_to_nhwc(x.data_ptr(), L.ptr(eps), sigma, y.data_ptr(), B, C, H, W, CP, dtype,
                                     L.stream_ptr()), "vg_nchw_to_nhwc")
    return y


def nchw_to_nhwc_pair(x, CP, dtype, eps, sigma, out_noisy):
    """(x as NHWC, x + sigma * eps as NHWC written into out_noisy) in ONE pass over x (vg_nchw_to_nhwc_pair), or None where
    the four-pixel kernel does not apply.  eps: NCHW f32 noise tensor or a NoiseDraw."""
    rng = isinstance(eps, NoiseDraw)
    _need_cuda(x, None if rng else eps, out_noisy)
    B, C, H, W = x.shape
    if dtype != 1 or CP != 8 or C > 4 or (H * W) % 4 != 0:
        return None
    plain = empty_act((B, H, W, CP), dtype, x.device)
    rc = L.load().vg_nchw_to_nhwc_pair(x.data_ptr(), None if rng else eps.data_ptr(), eps.state.data_ptr() if rng else None,
                                       eps.draw if rng else 0, sigma, out_noisy.data_ptr(), plain.data_ptr(), B, C, H, W, CP,
                                       dtype, L.stream_ptr())
    if rc == L.VG_ENOSUP:
        return None
    L.check(rc, "vg_nchw_to_nhwc_pair")
    return plain, out_noisy


def gather_normalize_u8(images_u8, idx, out=None):
    """images_u8 [N,H,W,C] uint8 on the device, idx [B] int64 on the device -> [B,C,H,W] f32 in [-1,1]
    (ToTensor + Normalize(0.5,0.5), dataset_code.py:147-150)."""
    _need_cuda(images_u8, idx, out)
    if images_u8.dtype != torch.uint8 or idx.dtype != torch.int64 or images_u8.dim() != 4:
        raise RuntimeError("gather_normalize_u8: images must be uint8 [N,H,W,C], idx int64 [B]")
    N, H, W, C = images_u8.shape
    B = idx.numel()
    y = out if out is not None else torch.empty(B, C, H, W, dtype=torch.float32, device=images_u8.device)
    L.check(L.load().vg_gather_normalize_u8(images_u8.data_ptr(), N, idx.data_ptr(), B, C, H, W, y.data_ptr(),
                                            L.stream_ptr()), "vg_gather_normalize_u8")
    return y


class _ResizeTables:
    """Device coefficient tables of one resize geometry, restricted to the crop window, plus the host copy of the
    bounds that vg_resize_u8 validates before every launch (kept alive here)."""

    def __init__(self, Hin, Win, geometry, device):
        from .data import resample_coeffs                               # data imports ops
        Hr, Wr, top, left, ch, cw = geometry
        if ch > Hr or cw > Wr:
            raise RuntimeError("CenterCrop larger than the resized image (padding) is not supported")
        if min(Hr, Wr, ch, cw) < 1 or top < 0 or left < 0 or top + ch > Hr or left + cw > Wr:
            raise RuntimeError(f"resize_u8: bad geometry {geometry}")
        self.top, self.left, self.ch, self.cw = top, left, ch, cw
        self.kh = self.bh = self.bh_host = self.kv = self.bv = self.bv_host = None
        self.ksh = self.ksv = 0
        if Wr != Win:
            k, b = resample_coeffs(Win, Wr)
            self.ksh = k.shape[1]
            self.bh_host = b[left:left + cw].copy()
            self.kh = torch.from_numpy(k[left:left + cw].copy()).to(device)
            self.bh = torch.from_numpy(self.bh_host).to(device)
        if Hr != Hin:
            k, b = resample_coeffs(Hin, Hr)
            self.ksv = k.shape[1]
            self.bv_host = b[top:top + ch].copy()
            self.kv = torch.from_numpy(k[top:top + ch].copy()).to(device)
            self.bv = torch.from_numpy(self.bv_host).to(device)

    def host(self, b):
        return 0 if b is None else b.ctypes.data


_RESIZE_TABLES = {}          # (Hin, Win, Hr, Wr, top, left, ch, cw, device) -> _ResizeTables; a few hundred bytes to a few KB each


def resize_tables(Hin, Win, geometry, device) -> _ResizeTables:
    key = (int(Hin), int(Win)) + tuple(int(v) for v in geometry) + (str(device),)
    t = _RESIZE_TABLES.get(key)
    if t is None:
        if len(_RESIZE_TABLES) >= 64:
            _RESIZE_TABLES.clear()
        t = _RESIZE_TABLES[key] = _ResizeTables(int(Hin), int(Win), key[2:8], device)
    return t


def resize_u8_lds_bytes(Hin, Win, C, geometry, B=1, band=0) -> int:
    """LDS bytes per workgroup of resize_u8 for this geometry, or -1 where the library does not serve it (host only)."""
    t = _ResizeTables(Hin, Win, tuple(int(v) for v in geometry), "cpu")
    return int(L.load().vg_resize_u8_lds_bytes(Hin, Win, C, t.host(t.bh_host), t.ksh, t.host(t.bv_host), t.ksv, t.top, t.left,
                                               t.ch, t.cw, B, band))


def resize_u8_traffic(Hin, Win, C, geometry, B=1, band=0) -> dict:
    """Bytes per image of a resize_u8 launch (host only): `algorithmic` = rows_read * cols_read * C + ch * cw * C, and
    `actual` with the input rows that adjacent bands read twice; plus the band height and the LDS bytes of the launch."""
    t = _ResizeTables(Hin, Win, tuple(int(v) for v in geometry), "cpu")
    args = (Hin, Win, C, t.host(t.bh_host), t.ksh, t.host(t.bv_host), t.ksv, t.top, t.left, t.ch, t.cw, B, band)
    bd = int(L.load().vg_resize_u8_band(*args))
    if bd < 0:
        L.check(bd, "vg_resize_u8_band")
    cols = t.cw if t.bh_host is None else int(t.bh_host[-1].sum() - t.bh_host[0, 0])
    lo = [t.top + y for y in range(t.ch)] if t.bv_host is None else [int(v) for v in t.bv_host[:, 0]]
    hi = [v + 1 for v in lo] if t.bv_host is None else [int(v) for v in t.bv_host.sum(1)]
    rows = hi[-1] - lo[0]
    rows_banded = sum(hi[min(y0 + bd, t.ch) - 1] - lo[y0] for y0 in range(0, t.ch, bd))
    out = t.ch * t.cw * C
    return {"band": bd, "lds_bytes": int(L.load().vg_resize_u8_lds_bytes(*args)), "rows_read": rows, "cols_read": cols,
            "algorithmic": rows * cols * C + out, "actual": rows_banded * cols * C + out}


def resize_u8(images_u8, geometry, idx=None, out=None, band=0):
    """Resize + CenterCrop on the device (vg_resize_u8, include/vaegan_hip.h "Resize"): images_u8 [N,Hin,Win,C] uint8 ->
    uint8 [B,ch,cw,C], equal to PIL's ``resize((Wr, Hr), BILINEAR)`` + crop byte for byte.  geometry = (Hr, Wr, top, left,
    ch, cw), see data.resize_geometry.  idx: int64 [B] on the device (source image of each output image) or None: all N
    images in order.  band: output rows per workgroup (0: chosen by the library; the result does not depend on it).
    The coefficient tables are built on the host once per geometry and cached on the device; a launch whose tables are
    cached does no host-to-device copy (graph capture)."""
    _need_cuda(images_u8, idx, out)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.numel() == 0:
        raise RuntimeError("resize_u8: images must be a non-empty uint8 [N,H,W,C] tensor")
    if idx is not None and (idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() == 0):
        raise RuntimeError("resize_u8: idx must be a non-empty int64 [B] tensor")
    N, Hin, Win, C = images_u8.shape
    B = N if idx is None else idx.numel()
    t = resize_tables(Hin, Win, geometry, images_u8.device)
    y = out if out is not None else torch.empty(B, t.ch, t.cw, C, dtype=torch.uint8, device=images_u8.device)
    if tuple(y.shape) != (B, t.ch, t.cw, C) or y.dtype != torch.uint8:
        raise RuntimeError("resize_u8: out must be uint8 [B,ch,cw,C]")
    L.check(L.load().vg_resize_u8(images_u8.data_ptr(), N, Hin, Win, C, L.ptr(idx), B, L.ptr(t.kh), L.ptr(t.bh),
                                  t.host(t.bh_host), t.ksh, L.ptr(t.kv), L.ptr(t.bv), t.host(t.bv_host), t.ksv, t.top, t.left,
                                  y.data_ptr(), t.ch, t.cw, int(band), L.stream_ptr()), "vg_resize_u8")
    return y


# draw ids of the degraded-pair data path (include/vaegan_hip.h "Degraded pairs"; 0..2 belong to the training iteration)
DRAW_DEGRADE_NORMAL, DRAW_DEGRADE_FILL, DRAW_DEGRADE_PARAMS = 16, 17, 18
DRAW_DEGRADE_IMPULSE, DRAW_DEGRADE_SALT = 19, 20
_NO_BOUNDS = (0, 0, 0, 0, 0, 0)
NOISE_KIND = {"gaussian": L.VG_NOISE_GAUSSIAN, "speckle": L.VG_NOISE_SPECKLE, "shot": L.VG_NOISE_SHOT}


def rand_u01(n: int, state: torch.Tensor, draw: int, out=None) -> torch.Tensor:
    """U[0,1) twin of NoiseStream.randn: element i = (word i & 3 of Philox block i >> 2) >> 8, times 2^-24.
    state: int64[2] on the device = {seed, counter}."""
    _need_cuda(state, out)
    y = out if out is not None else torch.empty(n, dtype=torch.float32, device=state.device)
    L.check(L.load().vg_rand_u01(y.data_ptr(), n, state.data_ptr(), draw, L.stream_ptr()), "vg_rand_u01")
    return y


def _degrade_key(seed, pos0) -> None:
    if not 0 <= int(seed) < 1 << 63 or not 0 <= int(pos0) < 1 << 56:
        raise RuntimeError("degrade: seed must be in [0, 2^63) (an int64 {seed, position} state addresses the same draws) "
                           "and pos0 in [0, 2^56)")


def _degrade_bounds(rect, bounds):
    if not rect:
        return _NO_BOUNDS
    if bounds is None or len(bounds) != 6:
        raise RuntimeError("rect=True needs bounds = (min_size, max_size, x0, x1, y0, y1), see data.degrade_bounds")
    return tuple(int(v) for v in bounds)


def _noise_model(what, kind, impulse_max_p, salt_ratio):
    """-> None for the reference's model (the old entry points serve it), else (kind id, impulse_max_p, salt_ratio)."""
    if kind not in NOISE_KIND:
        raise ValueError(f"{what}: kind must be 'gaussian', 'speckle' or 'shot', got {kind!r}")
    for name, v in (("impulse_max_p", impulse_max_p), ("salt_ratio", salt_ratio)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:
            raise ValueError(f"{what}: {name} must be a number in [0, 1], got {v!r}")
    if kind == "gaussian" and impulse_max_p == 0:
        return None
    return NOISE_KIND[kind], float(impulse_max_p), float(salt_ratio)


def gather_degrade_u8(images_u8, idx, seed, pos0, noise_max_std, rect, normalize, bounds=None, out_clean=None,
                      out_noisy=None, nhwc=None, kind="gaussian", impulse_max_p=0.0, salt_ratio=0.5):
    """(noisy, clean) pair batch in one pass over the resident u8 set (vg_gather_degrade_u8; dataset_code.py:35-65).
    images_u8 [N,H,W,C] uint8, idx [B] int64, both on the device; seed / pos0: python ints, pos0 = position of idx[0]
    in the epoch's order.  nhwc: None, or (CP, dtype) / a preallocated [B,H,W,CP] engine tensor that also receives
    `noisy` in the Encoder's input layout.  kind / impulse_max_p / salt_ratio: the noise model (include/vaegan_hip.h "Degraded
    pairs", noise models) -- "gaussian" | "speckle" | "shot", plus salt-and-pepper impulses with per-image probability
    s * impulse_max_p; the defaults are the reference's model and call the entry point they always called, anything else
    goes to vg_gather_degrade_u8_ex.  -> (noisy NCHW f32, clean NCHW f32, nhwc tensor or None)."""
    model = _noise_model("gather_degrade_u8", kind, impulse_max_p, salt_ratio)
    _need_cuda(images_u8, idx, out_clean, out_noisy, nhwc if isinstance(nhwc, torch.Tensor) else None)
    if images_u8.dtype != torch.uint8 or idx.dtype != torch.int64 or images_u8.dim() != 4:
        raise RuntimeError("gather_degrade_u8: images must be uint8 [N,H,W,C], idx int64 [B]")
    N, H, W, C = images_u8.shape
    B = idx.numel()
    dev = images_u8.device
    _degrade_key(seed, pos0)
    clean = out_clean if out_clean is not None else torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
    noisy = out_noisy if out_noisy is not None else torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
    CP, dtype, y = 0, F32, None
    if isinstance(nhwc, torch.Tensor):
        y = nhwc
        CP = y.shape[-1]
        dtype = {v: k for k, v in TORCH_DT.items()}[y.dtype]
        if tuple(y.shape) != (B, H, W, CP):
            raise RuntimeError("gather_degrade_u8: nhwc must be [B,H,W,CP]")
    elif nhwc is not None:
        CP, dtype = nhwc
        y = empty_act((B, H, W, CP), dtype, dev)
    for t in (clean, noisy):
        if tuple(t.shape) != (B, C, H, W) or t.dtype != torch.float32:
            raise RuntimeError("gather_degrade_u8: outputs must be f32 [B,C,H,W]")
    args = (images_u8.data_ptr(), N, idx.data_ptr(), B, C, H, W, int(seed), int(pos0), float(noise_max_std), 1 if rect else 0,
            1 if normalize else 0, *_degrade_bounds(rect, bounds), clean.data_ptr(), noisy.data_ptr(), L.ptr(y), CP, dtype)
    if model is None:
        L.check(L.load().vg_gather_degrade_u8(*args, L.stream_ptr()), "vg_gather_degrade_u8")
    else:
        L.check(L.load().vg_gather_degrade_u8_ex(*args, *model, L.stream_ptr()), "vg_gather_degrade_u8_ex")
    return noisy, clean, y


def degrade_params(seed, pos0, B, noise_max_std, rect, H, W, bounds=None, device="cuda", kind="gaussian", impulse_max_p=0.0,
                   salt_ratio=0.5) -> torch.Tensor:
    """-> f32 [B,8] on the device: s, sigma = s*noise_max_std, rect_h, rect_w, x, y, p = s*impulse_max_p, kind id of epoch
    positions pos0 .. pos0+B-1 (vg_degrade_params; vg_degrade_params_ex for another noise model than the default, whose last
    two columns are 0, 0): what gather_degrade_u8 uses for the same seed and positions."""
    model = _noise_model("degrade_params", kind, impulse_max_p, salt_ratio)
    out = torch.empty(B, 8, dtype=torch.float32, device=device)
    _need_cuda(out)
    _degrade_key(seed, pos0)
    args = (int(seed), int(pos0), B, float(noise_max_std), 1 if rect else 0, H, W, *_degrade_bounds(rect, bounds), out.data_ptr())
    if model is None:
        L.check(L.load().vg_degrade_params(*args, L.stream_ptr()), "vg_degrade_params")
    else:
        L.check(L.load().vg_degrade_params_ex(*args, *model, L.stream_ptr()), "vg_degrade_params_ex")
    return out


# draw ids of the latent prior (include/vaegan_hip.h "Latent prior"): outside 0..2 and 16..18
DRAW_LATENT_U, DRAW_LATENT_V, DRAW_LATENT_EPS = 32, 33, 34


def latent_hist(x, n_bins=100):
    """Per-column np.histogram + np.cumsum(counts / N) of x f32 [N,D] on the device (vg_latent_hist); x may be a view
    whose rows are further apart than D (stride(1) == 1).  -> (edges f32 [D,n_bins+1], counts int32 [D,n_bins],
    cdf f64 [D,n_bins], status int32 [1]: non-zero where a column's range is not finite).  No host sync."""
    if not x.is_cuda:
        raise RuntimeError("vaegan_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise RuntimeError("latent_hist: x must be a non-empty f32 [N,D] tensor")
    N, D = x.shape
    stride = x.stride(0) if N > 1 else D
    if (D > 1 and x.stride(1) != 1) or stride < D:
        raise RuntimeError("latent_hist: the columns of x must be adjacent in memory (stride(1) == 1, stride(0) >= D)")
    lib = L.load()
    nbytes = lib.vg_latent_hist_ws_bytes(N, D, int(n_bins))
    if nbytes < 0:
        L.check(int(nbytes), "vg_latent_hist_ws_bytes")
    dev = x.device
    edges = torch.empty(D, n_bins + 1, dtype=torch.float32, device=dev)
    counts = torch.empty(D, n_bins, dtype=torch.int32, device=dev)
    cdf = torch.empty(D, n_bins, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = WS.get("latent", nbytes, dev)
    L.check(lib.vg_latent_hist(x.data_ptr(), N, D, stride, int(n_bins), edges.data_ptr(), counts.data_ptr(), cdf.data_ptr(),
                               status.data_ptr(), ws.data_ptr(), ws.numel() * 4, L.stream_ptr()), "vg_latent_hist")
    return edges, counts, cdf, status


def latent_sample(edges, cdf, L_dim, n, u=None, v=None, eps=None, state=None, want_mulv=True, z=None):
    """n draws from a fitted prior (vg_latent_sample).  edges f32 [2L,n_bins+1], cdf f64 [2L,n_bins].  u, v: f64 [n,2L]
    (both or neither), eps: f32 [n,L]; whatever is None is drawn in the kernel from state = int64[2] {seed, counter}.
    z: None or (ZP, dtype) -> also the Generator's input [n,1,1,ZP].  -> (mulv f32 [n,2L] or None, z or None)."""
    _need_cuda(edges, cdf, u, v, eps, state)
    n, L_dim = int(n), int(L_dim)
    n_bins = cdf.shape[-1]
    if (edges.dtype != torch.float32 or cdf.dtype != torch.float64 or tuple(edges.shape) != (2 * L_dim, n_bins + 1)
            or tuple(cdf.shape) != (2 * L_dim, n_bins)):
        raise RuntimeError("latent_sample: edges must be f32 [2L,n_bins+1] and cdf f64 [2L,n_bins]")
    if n < 1:
        raise RuntimeError("latent_sample: n must be >= 1")
    for t, name in ((u, "u"), (v, "v")):
        if t is not None and (t.dtype != torch.float64 or t.numel() != n * 2 * L_dim):
            raise RuntimeError(f"latent_sample: {name} must be f64 [n,2L]")
    if eps is not None and (eps.dtype != torch.float32 or eps.numel() != n * L_dim):
        raise RuntimeError("latent_sample: eps must be f32 [n,L]")
    if state is not None and (state.dtype != torch.int64 or state.numel() != 2):
        raise RuntimeError("latent_sample: state must be int64[2] = {seed, counter}")
    dev = edges.device
    mulv = torch.empty(n, 2 * L_dim, dtype=torch.float32, device=dev) if want_mulv else None
    ZP, dtype, zt = 0, F32, None
    if z is not None:
        ZP, dtype = z
        zt = empty_act((n, 1, 1, ZP), dtype, dev)
    L.check(L.load().vg_latent_sample(edges.data_ptr(), cdf.data_ptr(), n_bins, L_dim, n, L.ptr(u), L.ptr(v), L.ptr(eps),
                                      L.ptr(state), L.ptr(mulv), L.ptr(zt), ZP, dtype, L.stream_ptr()), "vg_latent_sample")
    return mulv, zt


def to_u8(x, grid_cols=0):
    """[-1,1] f32 [B,C,H,W] -> uint8 ((x + 1) / 2 * 255, clamp, truncate; main_vae.py:492,498-499) on the device:
    [B,C,H,W], or with grid_cols > 0 ONE [rows*H, grid_cols*W, C] picture, image i at tile (i // grid_cols, i % grid_cols)."""
    _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 4 or x.numel() == 0 or grid_cols < 0:
        raise RuntimeError("to_u8: x must be a non-empty f32 [B,C,H,W] tensor and grid_cols >= 0")
    B, C, H, W = x.shape
    if grid_cols:
        y = torch.empty((B + grid_cols - 1) // grid_cols * H, grid_cols * W, C, dtype=torch.uint8, device=x.device)
    else:
        y = torch.empty(B, C, H, W, dtype=torch.uint8, device=x.device)
    L.check(L.load().vg_to_u8(x.data_ptr(), y.data_ptr(), B, C, H, W, int(grid_cols), L.stream_ptr()), "vg_to_u8")
    return y


def _ws_query(nbytes: int, what: str) -> int:
    if nbytes < 0:
        L.check(int(nbytes), what)
    return int(nbytes)


def _feature_rows(x, what: str, name: str = "x"):
    """f32 [N,D] device matrix whose columns are adjacent in memory -> (N, D, row stride in elements)."""
    if not x.is_cuda:
        raise RuntimeError("vaegan_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] < 1:
        raise RuntimeError(f"{what}: {name} must be an f32 [N,D] tensor with D >= 1")
    N, D = x.shape
    stride = x.stride(0) if N > 1 else D
    if (D > 1 and N > 0 and x.stride(1) != 1) or (N > 1 and stride < D):
        raise RuntimeError(f"{what}: the columns of {name} must be adjacent in memory (stride(1) == 1, stride(0) >= D)")
    return N, D, stride


# draw ids of the Gaussian-mixture prior (include/vaegan_hip.h "Gaussian-mixture prior")
DRAW_GMM_U, DRAW_GMM_EPS = 40, 41
GMM_MAX_D, GMM_MAX_K = 256, 64


def _gmm_params(what, K, D, **tensors):
    """The f64 parameter tensors of a mixture: on the device, contiguous, of the stated shape."""
    for name, (t, shape) in tensors.items():
        if not t.is_cuda:
            raise RuntimeError("vaegan_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be a contiguous f64 tensor of shape {list(shape)}")
    if not (1 <= K <= GMM_MAX_K and 1 <= D <= GMM_MAX_D):
        raise RuntimeError(f"{what}: needs 1 <= K <= {GMM_MAX_K} components and 1 <= D <= {GMM_MAX_D} dimensions")


def gmm_log_resp(x, mean, prec_chol, log_coef, want_log_prob=False, want_log_norm=True, want_resp=True):
    """E-step of a full-covariance Gaussian mixture on the device (vg_gmm_log_resp).  x f32 [N,D] (may be a view whose
    rows are further apart than D); mean f64 [K,D], prec_chol f64 [K,D,D] (upper triangular, scikit-learn's
    precisions_cholesky_), log_coef f64 [K].  -> (log_prob f64 [N,K], log_norm f64 [N], resp f64 [N,K]), None for what
    was not asked for.  One launch, no host sync."""
    N, D, stride = _feature_rows(x, "gmm_log_resp")
    if N < 1:
        raise RuntimeError("gmm_log_resp: x must hold at least one row")
    K = mean.shape[0] if mean.dim() == 2 else 0
    _gmm_params("gmm_log_resp", K, D, mean=(mean, (K, D)), prec_chol=(prec_chol, (K, D, D)), log_coef=(log_coef, (K,)))
    if not (want_log_prob or want_log_norm or want_resp):
        raise RuntimeError("gmm_log_resp: ask for at least one output")
    dev = x.device
    lp = torch.empty(N, K, dtype=torch.float64, device=dev) if want_log_prob else None
    ln = torch.empty(N, dtype=torch.float64, device=dev) if want_log_norm else None
    rs = torch.empty(N, K, dtype=torch.float64, device=dev) if want_resp else None
    L.check(L.load().vg_gmm_log_resp(x.data_ptr(), N, D, stride, K, mean.data_ptr(), prec_chol.data_ptr(),
                                     log_coef.data_ptr(), L.ptr(lp), L.ptr(ln), L.ptr(rs), L.stream_ptr()),
            "vg_gmm_log_resp")
    return lp, ln, rs


def gmm_moments(x, shift, resp, log_norm=None):
    """M-step sums of a Gaussian mixture on the device (vg_gmm_moments), d = x - shift_k: nk f64 [K] = sum r, s1 f64 [K,D]
    = sum r d, s2 f64 [K,D,D] = sum r d d^T, loglik f64 [1] = sum log_norm (None without log_norm).  x f32 [N,D] (may be
    a strided view), shift f64 [K,D], resp f64 [N,K], log_norm f64 [N].  Deterministic; two launches, no host sync.
    -> (nk, s1, s2, loglik)."""
    N, D, stride = _feature_rows(x, "gmm_moments")
    if N < 1:
        raise RuntimeError("gmm_moments: x must hold at least one row")
    K = shift.shape[0] if shift.dim() == 2 else 0
    _gmm_params("gmm_moments", K, D, shift=(shift, (K, D)), resp=(resp, (N, K)))
    if log_norm is not None:
        _gmm_params("gmm_moments", K, D, log_norm=(log_norm, (N,)))
    lib = L.load()
    nbytes = _ws_query(lib.vg_gmm_moments_ws_bytes(N, D, K), "vg_gmm_moments_ws_bytes")
    dev = x.device
    nk = torch.empty(K, dtype=torch.float64, device=dev)
    s1 = torch.empty(K, D, dtype=torch.float64, device=dev)
    s2 = torch.empty(K, D, D, dtype=torch.float64, device=dev)
    ll = torch.empty(1, dtype=torch.float64, device=dev) if log_norm is not None else None
    ws = WS.get("gmm", nbytes, dev)
    L.check(lib.vg_gmm_moments(x.data_ptr(), N, D, stride, K, shift.data_ptr(), resp.data_ptr(), L.ptr(log_norm),
                               nk.data_ptr(), s1.data_ptr(), s2.data_ptr(), L.ptr(ll), ws.data_ptr(), ws.numel() * 4,
                               L.stream_ptr()), "vg_gmm_moments")
    return nk, s1, s2, ll


def gmm_sample(cdf, mean, cov_chol, n, u=None, eps=None, state=None, want_comp=False, want_z32=True, z=None):
    """n draws from a Gaussian mixture (vg_gmm_sample).  cdf f64 [K] (cumulative weights), mean f64 [K,D], cov_chol f64
    [K,D,D] (lower factors).  u: f64 [n] picks the component, eps: f32 [n,D] is the normal draw; whatever is None is drawn
    in the kernel from state = int64[2] {seed, counter}.  z: None or (ZP, dtype) -> also the Generator's input [n,1,1,ZP].
    -> (comp int32 [n] or None, z32 f32 [n,D] or None, z or None).  One launch, no host sync."""
    _need_cuda(cdf, mean, cov_chol, u, eps, state)
    n = int(n)
    K, D = (mean.shape[0], mean.shape[1]) if mean.dim() == 2 else (0, 0)
    _gmm_params("gmm_sample", K, D, cdf=(cdf, (K,)), mean=(mean, (K, D)), cov_chol=(cov_chol, (K, D, D)))
    if n < 1:
        raise RuntimeError("gmm_sample: n must be >= 1")
    if u is not None and (u.dtype != torch.float64 or u.numel() != n):
        raise RuntimeError("gmm_sample: u must be f64 [n]")
    if eps is not None and (eps.dtype != torch.float32 or eps.numel() != n * D):
        raise RuntimeError("gmm_sample: eps must be f32 [n,D]")
    if state is not None and (state.dtype != torch.int64 or state.numel() != 2):
        raise RuntimeError("gmm_sample: state must be int64[2] = {seed, counter}")
    if state is None and (u is None or eps is None):
        raise RuntimeError("gmm_sample: whatever is not injected (u, eps) needs the generator state")
    if not (want_comp or want_z32 or z is not None):
        raise RuntimeError("gmm_sample: ask for at least one output")
    dev = mean.device
    comp = torch.empty(n, dtype=torch.int32, device=dev) if want_comp else None
    z32 = torch.empty(n, D, dtype=torch.float32, device=dev) if want_z32 else None
    ZP, dtype, zt = 0, F32, None
    if z is not None:
        ZP, dtype = z
        zt = empty_act((n, 1, 1, ZP), dtype, dev)
    L.check(L.load().vg_gmm_sample(cdf.data_ptr(), mean.data_ptr(), cov_chol.data_ptr(), K, D, n, L.ptr(u), L.ptr(eps),
                                   L.ptr(state), L.ptr(comp), L.ptr(z32), L.ptr(zt), ZP, dtype, L.stream_ptr()),
            "vg_gmm_sample")
    return comp, z32, zt


# draw id of the k-means++ seeding (include/vaegan_hip.h "K-means")
DRAW_KMEANS_U = 42
KMEANS_MAX_D, KMEANS_MAX_K = 256, 1024


def _kmeans_shape(what, N, D, K):
    if N < 1:
        raise RuntimeError(f"{what}: x must hold at least one row")
    if not (1 <= K <= KMEANS_MAX_K and 1 <= D <= KMEANS_MAX_D):
        raise RuntimeError(f"{what}: needs 1 <= K <= {KMEANS_MAX_K} clusters and 1 <= D <= {KMEANS_MAX_D} dimensions")


def _kmeans_tensor(what, name, t, dtype, shape):
    if not t.is_cuda:
        raise RuntimeError("vaegan_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape "
                           f"{list(shape)}")


def kmeans_plan(N: int, D: int, K: int) -> dict:
    """What the k-means launchers launch for N rows, D columns and K clusters (vg_kmeans_plan; host-only, needs no GPU):
    rows per workgroup / centre tile / row-split flag / LDS bytes / grid of the assign kernel, splits / rows per split /
    cluster chunk / chunks / workspace bytes of the update, block size / blocks / workspace bytes of the seed."""
    p = L.KMPlan()
    L.check(L.load().vg_kmeans_plan(int(N), int(D), int(K), L.byref(p)), "vg_kmeans_plan")
    return {n: int(getattr(p, n)) for n, _ in L.KMPlan._fields_}


def kmeans_assign(x, center, want_label=True, want_dist2=False, want_resp=False, prev_label=None):
    """Nearest centre of every row on the device (vg_kmeans_assign): label int32 [N] = the LOWEST k minimising
    0.5 |c_k|^2 - x . c_k (f64 MFMA), dist2 f64 [N] = |x - c_label|^2 in direct form, resp f64 [N, K] one-hot (what
    ``gmm_moments`` consumes), changed int32 [1] = rows whose label differs from ``prev_label`` int32 [N].  x f32 [N, D]
    (may be a strided view), center f64 [K, D].  One launch, no host sync.  -> (label, dist2, resp, changed), None for
    what was not asked for."""
    N, D, stride = _feature_rows(x, "kmeans_assign")
    K = center.shape[0] if center.dim() == 2 else 0
    _kmeans_tensor("kmeans_assign", "center", center, torch.float64, (K, D))
    _kmeans_shape("kmeans_assign", N, D, K)
    if prev_label is not None:
        _kmeans_tensor("kmeans_assign", "prev_label", prev_label, torch.int32, (N,))
    if not (want_label or want_dist2 or want_resp or prev_label is not None):
        raise RuntimeError("kmeans_assign: ask for at least one output")
    dev = x.device
    label = torch.empty(N, dtype=torch.int32, device=dev) if want_label else None
    dist2 = torch.empty(N, dtype=torch.float64, device=dev) if want_dist2 else None
    resp = torch.empty(N, K, dtype=torch.float64, device=dev) if want_resp else None
    changed = torch.empty(1, dtype=torch.int32, device=dev) if prev_label is not None else None
    L.check(L.load().vg_kmeans_assign(x.data_ptr(), N, D, stride, K, center.data_ptr(), L.ptr(label), L.ptr(dist2),
                                      L.ptr(resp), L.ptr(prev_label), L.ptr(changed), L.stream_ptr()), "vg_kmeans_assign")
    return label, dist2, resp, changed


def kmeans_update(x, label, K, old=None, dist2=None, want_sum=False, want_stats=None):
    """Cluster counts, sums and new centres from the labels on the device (vg_kmeans_update): count int64 [K]; sum f64
    [K, D] (``want_sum``); center f64 [K, D] = sum / count, an empty cluster keeping ``old`` f64 [K, D] (centres are made
    only where ``old`` is given); stats f64 [2] = (sum of squared centre shifts, sum of ``dist2`` f64 [N]) -- made where
    ``old`` or ``dist2`` is given unless ``want_stats=False``.  Rows whose label is outside [0, K) are skipped.  x f32
    [N, D] (may be a strided view), label int32 [N].  Deterministic; two or three launches, no host sync.
    -> (count, sum, center, stats), None for what was not made."""
    N, D, stride = _feature_rows(x, "kmeans_update")
    K = int(K)
    _kmeans_shape("kmeans_update", N, D, K)
    _kmeans_tensor("kmeans_update", "label", label, torch.int32, (N,))
    if old is not None:
        _kmeans_tensor("kmeans_update", "old", old, torch.float64, (K, D))
    if dist2 is not None:
        _kmeans_tensor("kmeans_update", "dist2", dist2, torch.float64, (N,))
    if want_stats is None:
        want_stats = old is not None or dist2 is not None
    if dist2 is not None and not want_stats:
        raise RuntimeError("kmeans_update: dist2 is only read for stats")
    lib = L.load()
    nbytes = _ws_query(lib.vg_kmeans_update_ws_bytes(N, D, K), "vg_kmeans_update_ws_bytes")
    dev = x.device
    count = torch.empty(K, dtype=torch.int64, device=dev)
    sm = torch.empty(K, D, dtype=torch.float64, device=dev) if want_sum else None
    center = torch.empty(K, D, dtype=torch.float64, device=dev) if old is not None else None
    stats = torch.empty(2, dtype=torch.float64, device=dev) if want_stats else None
    ws = WS.get("kmeans", nbytes, dev)
    L.check(lib.vg_kmeans_update(x.data_ptr(), N, D, stride, K, label.data_ptr(), L.ptr(dist2), L.ptr(old), count.data_ptr(),
                                 L.ptr(sm), L.ptr(center), L.ptr(stats), ws.data_ptr(), ws.numel() * 4, L.stream_ptr()),
            "vg_kmeans_update")
    return count, sm, center, stats


def kmeans_seed(x, K, u=None, state=None):
    """Plain k-means++ seeding on the device with no host sync (vg_kmeans_seed): idx int32 [K] (row numbers), center f64
    [K, D] (those rows), mind2 f64 [N] (squared distance of every row to its nearest chosen row).  u: f64 [K] in [0, 1)
    picks the rows; None: drawn in the kernel from state = int64[2] {seed, counter} with draw id DRAW_KMEANS_U.  x f32
    [N, D] (may be a strided view).  2 K - 1 launches.  With fewer than K distinct rows the centres hold duplicates.
    -> (idx, center, mind2)."""
    N, D, stride = _feature_rows(x, "kmeans_seed")
    K = int(K)
    _kmeans_shape("kmeans_seed", N, D, K)
    if u is not None:
        _kmeans_tensor("kmeans_seed", "u", u, torch.float64, (K,))
    if state is not None:
        _need_cuda(state)
        if state.dtype != torch.int64 or state.numel() != 2:
            raise RuntimeError("kmeans_seed: state must be int64[2] = {seed, counter}")
    if u is None and state is None:
        raise RuntimeError("kmeans_seed: u is not injected, so the draws need the generator state")
    lib = L.load()
    nbytes = _ws_query(lib.vg_kmeans_seed_ws_bytes(N, D, K), "vg_kmeans_seed_ws_bytes")
    dev = x.device
    idx = torch.empty(K, dtype=torch.int32, device=dev)
    center = torch.empty(K, D, dtype=torch.float64, device=dev)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    L.check(lib.vg_kmeans_seed(x.data_ptr(), N, D, stride, K, L.ptr(u), L.ptr(state), idx.data_ptr(), center.data_ptr(),
                               ws.data_ptr(), nbytes, L.stream_ptr()), "vg_kmeans_seed")
    return idx, center, ws[:N]


def feat_stats_accum(x, sum, outer):
    """FID's running statistics on the device (vg_feat_stats_accum): sum f64 [D] += column sums of x, outer f64 [D,D] +=
    x^T x, every product and addition in f64 on the exactly converted f32 rows of x f32 [n,D] (n >= 0; x may be a view
    whose rows are further apart than D).  Deterministic; in place; no host sync.  -> (sum, outer)."""
    n, D, stride = _feature_rows(x, "feat_stats_accum")
    _need_cuda(sum, outer)
    if (sum.dtype != torch.float64 or outer.dtype != torch.float64 or tuple(sum.shape) != (D,)
            or tuple(outer.shape) != (D, D)):
        raise RuntimeError(f"feat_stats_accum: sum must be f64 [{D}] and outer f64 [{D},{D}]")
    if n == 0:
        return sum, outer
    lib = L.load()
    nbytes = _ws_query(lib.vg_feat_stats_accum_ws_bytes(n, D), "vg_feat_stats_accum_ws_bytes")
    ws = WS.get("metrics", nbytes, x.device)
    L.check(lib.vg_feat_stats_accum(x.data_ptr(), n, D, stride, sum.data_ptr(), outer.data_ptr(), ws.data_ptr(),
                                    ws.numel() * 4, L.stream_ptr()), "vg_feat_stats_accum")
    return sum, outer


def knn_radius2(x, k=3):
    """r2 f32 [N]: the k-th smallest squared Euclidean distance from row i of x f32 [N,D] to the OTHER rows (row i is left
    out by index; a duplicate row counts with distance 0).  vg_knn_radius2: exact-f32 MFMA, the N x N matrix is never
    written.  1 <= k <= 8, k < N.  No host sync."""
    N, D, stride = _feature_rows(x, "knn_radius2")
    k = int(k)
    if not 1 <= k <= 8 or k >= N:
        raise RuntimeError(f"knn_radius2: k must be in [1, 8] and below the number of rows ({N}), got {k}")
    if N > 1 and stride != D:
        x = x.contiguous()
    x = _aligned16(x)
    lib = L.load()
    nbytes = _ws_query(lib.vg_knn_radius2_ws_bytes(N, D, k), "vg_knn_radius2_ws_bytes")
    ws = WS.get("metrics", nbytes, x.device)
    r2 = torch.empty(N, dtype=torch.float32, device=x.device)
    L.check(lib.vg_knn_radius2(x.data_ptr(), N, D, k, r2.data_ptr(), ws.data_ptr(), ws.numel() * 4, L.stream_ptr()),
            "vg_knn_radius2")
    return r2


def _aligned16(x):
    """The distance kernels read rows as 16-byte vectors: a view that starts off that grid is copied once."""
    return x if x.data_ptr() % 16 == 0 else x.clone()


def manifold_cover(q, ref, r2_ref, count=None):
    """inside int32 [Nq]: 1 where row i of q f32 [Nq,D] lies in the ball of radius^2 r2_ref[j] around some row j of ref
    f32 [Nr,D] (d2 <= r2_ref[j]); count int64 [1] (allocated unless given): the number of ones, on the device
    (vg_manifold_cover).  -> (inside, count).  No host sync."""
    Nq, D, sq = _feature_rows(q, "manifold_cover", "q")
    Nr, Dr, sr = _feature_rows(ref, "manifold_cover", "ref")
    _need_cuda(r2_ref)
    if Nq < 1 or Nr < 1 or D != Dr:
        raise RuntimeError("manifold_cover: q [Nq,D] and ref [Nr,D] must be non-empty and share D")
    if r2_ref.dtype != torch.float32 or tuple(r2_ref.shape) != (Nr,):
        raise RuntimeError(f"manifold_cover: r2_ref must be f32 [{Nr}]")
    if Nq > 1 and sq != D:
        q = q.contiguous()
    if Nr > 1 and sr != D:
        ref = ref.contiguous()
    q, ref = _aligned16(q), _aligned16(ref)
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=q.device)
    elif not count.is_cuda or count.dtype != torch.int64 or count.numel() != 1:
        raise RuntimeError("manifold_cover: count must be an int64 [1] device tensor")
    lib = L.load()
    nbytes = _ws_query(lib.vg_manifold_cover_ws_bytes(Nq, Nr, D), "vg_manifold_cover_ws_bytes")
    ws = WS.get("metrics", nbytes, q.device)
    inside = torch.empty(Nq, dtype=torch.int32, device=q.device)
    L.check(lib.vg_manifold_cover(q.data_ptr(), Nq, ref.data_ptr(), Nr, D, r2_ref.data_ptr(), inside.data_ptr(),
                                  count.data_ptr(), ws.data_ptr(), ws.numel() * 4, L.stream_ptr()), "vg_manifold_cover")
    return inside, count


def kid_scores(real, fake, idx_real, idx_fake, degree=3, gamma=1.0, coef=1.0):
    """Kernel Inception Distance per subset pair (vg_kid_scores): real f32 [Nr,D], fake f32 [Nf,D]; idx_real, idx_fake int32
    [S,m] device tables of row indices (subset s = real[idx_real[s]], fake[idx_fake[s]]; the kernel clamps indices, callers
    validate them).  k(a, c) = (gamma dot(a, c) + coef)^degree, everything in f64 on the f64 MFMA.  -> (scores f64 [S],
    stat f64 [2] = mean and population standard deviation of the scores, sums f64 [S,3] = the xx and yy sums over
    positions i != j and the xy sum over all pairs).  Deterministic; two launches; no host sync."""
    Nr, D, sr = _feature_rows(real, "kid_scores", "real")
    Nf, Df, sf = _feature_rows(fake, "kid_scores", "fake")
    _need_cuda(idx_real, idx_fake)
    if D != Df:
        raise RuntimeError(f"kid_scores: real [Nr,{D}] and fake [Nf,{Df}] must share D")
    if (idx_real.dtype != torch.int32 or idx_fake.dtype != torch.int32 or idx_real.dim() != 2
            or idx_real.shape != idx_fake.shape):
        raise RuntimeError("kid_scores: idx_real and idx_fake must be int32 [S, m] tensors of one shape")
    S, m = idx_real.shape
    degree, gamma, coef = int(degree), float(gamma), float(coef)
    if not (1 <= D <= 2048 and 1 <= S <= 4096 and 2 <= m <= min(Nr, Nf, 32768) and 1 <= degree <= 8
            and math.isfinite(gamma) and math.isfinite(coef)):
        raise RuntimeError(f"kid_scores: need 1 <= D <= 2048, 1 <= S <= 4096, 2 <= m <= min(Nr, Nf, 32768), 1 <= degree <= 8 "
                           f"and finite gamma, coef; got D={D} S={S} m={m} Nr={Nr} Nf={Nf} degree={degree} gamma={gamma} "
                           f"coef={coef}")
    if Nr > 1 and sr != D:
        real = real.contiguous()
    if Nf > 1 and sf != D:
        fake = fake.contiguous()
    real, fake = _aligned16(real), _aligned16(fake)
    lib = L.load()
    nbytes = _ws_query(lib.vg_kid_scores_ws_bytes(m, S), "vg_kid_scores_ws_bytes")
    ws = WS.get("metrics", nbytes, real.device)
    out = torch.empty(4 * S + 2, dtype=torch.float64, device=real.device)
    sums, scores, stat = out[:3 * S].view(S, 3), out[3 * S:4 * S], out[4 * S:]
    L.check(lib.vg_kid_scores(real.data_ptr(), Nr, fake.data_ptr(), Nf, D, idx_real.data_ptr(), idx_fake.data_ptr(), S, m,
                              degree, gamma, coef, sums.data_ptr(), scores.data_ptr(), stat.data_ptr(), ws.data_ptr(),
                              ws.numel() * 4, L.stream_ptr()), "vg_kid_scores")
    return scores, stat, sums


def noisy_clamp_to_nhwc(x, eps, sigma, CP, dtype, lo=-1.0, hi=1.0):
    """-> (noisy NHWC engine tensor, noisy NCHW f32)."""
    _need_cuda(x, eps)
    B, C, H, W = x.shape
    y = empty_act((B, H, W, CP), dtype, x.device)
    yn = torch.empty_like(x)
    L.check(L.load().vg_noisy_clamp_to_nhwc(x.data_ptr(), eps.data_ptr(), sigma, lo, hi, y.data_ptr(), yn.data_ptr(),
                                            B, C, H, W, CP, dtype, L.stream_ptr()), "vg_noisy_clamp_to_nhwc")
    return y, yn


def ssim(a, b):
    """Mean SSIM of two NCHW f32 batches in [-1,1] -> device scalar tensor [1]."""
    _need_cuda(a, b)
    B, C, H, W = a.shape
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    ws = WS.get("mse", 1024 * 4, a.device)
    L.check(L.load().vg_ssim(a.data_ptr(), b.data_ptr(), B, C, H, W, out.data_ptr(), ws.data_ptr(), 1024,
                             L.stream_ptr()), "vg_ssim")
    return out


def nhwc_to_nchw(x, C, dtype, apply_tanh=False, out=None):
    """out: an f32 [B,C,H,W] tensor to write into (a slice of a larger buffer), else a new one."""
    _need_cuda(x, out)
    B, H, W, CP = x.shape
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (B, C, H, W)):
        raise RuntimeError("nhwc_to_nchw: out must be f32 [B,C,H,W]")
    y = out if out is not None else torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    L.check(L.load().vg_nhwc_to_nchw(x.data_ptr(), y.data_ptr(), B, C, H, W, CP, 1 if apply_tanh else 0, dtype,
                                     L.stream_ptr()), "vg_nhwc_to_nchw")
    return y


def tile_gather(images, plan, t0, B, CP, dtype, out=None):
    """Tiles [t0, t0 + B) of ``plan`` (tiling.TilePlan) over ``images`` -- a resident uint8 [N,H,W,C] set (normalised as
    gather_normalize_u8 does) or an f32 [N,C,H,W] batch -- as the Encoder's NHWC input [B,S,S,CP] (vg_tile_gather)."""
    _need_cuda(images, out)
    u8 = images.dtype == torch.uint8
    if images.dim() != 4 or not (u8 or images.dtype == torch.float32):
        raise RuntimeError("tile_gather: images must be uint8 [N,H,W,C] or float32 [N,C,H,W]")
    N, H, W, C = images.shape if u8 else (images.shape[0], images.shape[2], images.shape[3], images.shape[1])
    if (H, W) != (plan.H, plan.W):
        raise RuntimeError(f"tile_gather: the plan is for {plan.H} x {plan.W} images, got {H} x {W}")
    S = plan.S
    y = out if out is not None else empty_act((B, S, S, CP), dtype, images.device)
    if y.numel() != B * S * S * CP or y.dtype != TORCH_DT[dtype]:
        raise RuntimeError("tile_gather: out must be [B,S,S,CP] in the engine dtype")
    t = plan.device_tables(images.device)
    L.check(L.load().vg_tile_gather(images.data_ptr() if u8 else None, None if u8 else images.data_ptr(), N, C, H, W, S,
                                    plan.ny, plan.nx, t["oy"].data_ptr(), t["ox"].data_ptr(), int(t0), int(B), y.data_ptr(),
                                    CP, dtype, L.stream_ptr()), "vg_tile_gather")
    return y


def tile_blend(tiles, plan, out=None):
    """f32 [N,C,H,W] from the reconstruction tiles f32 [N * ny * nx, C, S, S] of ``plan``, blended with the plan's
    coefficient tables in one launch (vg_tile_blend): no atomics, the same bits on every launch."""
    _need_cuda(tiles, out)
    S, per = plan.S, plan.ny * plan.nx
    if tiles.dtype != torch.float32 or tiles.dim() != 4 or tuple(tiles.shape[2:]) != (S, S) or tiles.shape[0] % per != 0 \
            or tiles.shape[0] == 0:
        raise RuntimeError(f"tile_blend: tiles must be f32 [N * {per}, C, {S}, {S}]")
    N, C = tiles.shape[0] // per, tiles.shape[1]
    y = out if out is not None else torch.empty(N, C, plan.H, plan.W, dtype=torch.float32, device=tiles.device)
    if y.dtype != torch.float32 or tuple(y.shape) != (N, C, plan.H, plan.W):
        raise RuntimeError("tile_blend: out must be f32 [N,C,H,W]")
    t = plan.device_tables(tiles.device)
    L.check(L.load().vg_tile_blend(tiles.data_ptr(), y.data_ptr(), N, C, plan.H, plan.W, S, plan.ny, plan.nx,
                                   t["oy"].data_ptr(), t["ox"].data_ptr(), t["first_y"].data_ptr(), t["count_y"].data_ptr(),
                                   t["coef_y"].data_ptr(), plan.cover_y, t["first_x"].data_ptr(), t["count_x"].data_ptr(),
                                   t["coef_x"].data_ptr(), plan.cover_x, L.stream_ptr()), "vg_tile_blend")
    return y


def nhwc_tanh_to_nchw_noisy(x, C, eps, sigma, out_noisy, dtype):
    """x NHWC (pre-tanh) -> (tanh(x) as NCHW f32, tanh(x) + sigma*eps written into out_noisy [B,H,W,CP])."""
    rng = isinstance(eps, NoiseDraw)
    _need_cuda(x, None if rng else eps, out_noisy)
    B, H, W, CP = x.shape
    if out_noisy.numel() != x.numel() or (not rng and eps.numel() != B * C * H * W):
        raise RuntimeError("nhwc_tanh_to_nchw_noisy: shape mismatch")
    y = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    if rng:
        L.check(L.load().vg_nhwc_tanh_to_nchw_noisy_rng(x.data_ptr(), y.data_ptr(), eps.state.data_ptr(), eps.draw, sigma,
                                                        out_noisy.data_ptr(), B, C, H, W, CP, dtype, L.stream_ptr()),
                "vg_nhwc_tanh_to_nchw_noisy_rng")
        return y
    L.check(L.load().vg_nhwc_tanh_to_nchw_noisy(x.data_ptr(), y.data_ptr(), eps.data_ptr(), sigma, out_noisy.data_ptr(),
                                                B, C, H, W, CP, dtype, L.stream_ptr()), "vg_nhwc_tanh_to_nchw_noisy")
    return y


def nchw_grad_add_to_nhwc(dy, add_nhwc, tanh_out, CP, dtype):
    """dx NHWC = (dy NCHW f32 + add_nhwc) * (1 - tanh_out^2): two gradient branches of the reconstruction in one pass."""
    _need_cuda(dy, add_nhwc, tanh_out)
    B, C, H, W = dy.shape
    if add_nhwc.numel() != B * H * W * CP:
        raise RuntimeError("nchw_grad_add_to_nhwc: add_nhwc must be [B,H,W,CP]")
    dx = empty_act((B, H, W, CP), dtype, dy.device)
    L.check(L.load().vg_nchw_grad_add_to_nhwc(dy.data_ptr(), add_nhwc.data_ptr(), L.ptr(tanh_out), dx.data_ptr(), B, C, H, W,
                                              CP, dtype, L.stream_ptr()), "vg_nchw_grad_add_to_nhwc")
    return dx


def nhwc_grad_tanh_to_nhwc(add_nhwc, tanh_out, CP, dtype):
    """dx NHWC = add_nhwc * (1 - tanh_out^2): nchw_grad_add_to_nhwc for an image without an MSE branch (dy == 0), i.e. the
    decoded prior samples; tanh_out NCHW f32, add_nhwc [B, H, W, CP] in the engine dtype."""
    _need_cuda(add_nhwc, tanh_out)
    B, C, H, W = tanh_out.shape
    if tanh_out.dtype != torch.float32 or add_nhwc.dtype != TORCH_DT[dtype] or add_nhwc.numel() != B * H * W * CP or CP < C:
        raise RuntimeError("nhwc_grad_tanh_to_nhwc: tanh_out f32 [B,C,H,W], add_nhwc [B,H,W,CP] in the engine dtype")
    dx = empty_act((B, H, W, CP), dtype, tanh_out.device)
    L.check(L.load().vg_nhwc_grad_tanh_to_nhwc(add_nhwc.data_ptr(), tanh_out.data_ptr(), dx.data_ptr(), B, C, H, W, CP, dtype,
                                               L.stream_ptr()), "vg_nhwc_grad_tanh_to_nhwc")
    return dx


def nchw_grad_to_nhwc(dy, tanh_out, CP, dtype):
    _need_cuda(dy, tanh_out)
    B, C, H, W = dy.shape
    dx = empty_act((B, H, W, CP), dtype, dy.device)
    L.check(L.load().vg_nchw_grad_to_nhwc(dy.data_ptr(), L.ptr(tanh_out), dx.data_ptr(), B, C, H, W, CP, dtype,
                                          L.stream_ptr()), "vg_nchw_grad_to_nhwc")
    return dx


def reparam_forward(mulv, eps, L_dim, ZP, dtype):
    rng = isinstance(eps, NoiseDraw)
    _need_cuda(mulv, None if rng else eps)
    B, MP = mulv.shape[0], mulv.shape[-1]
    z = empty_act((B, 1, 1, ZP), dtype, mulv.device)
    lvc = torch.empty(B, L_dim, dtype=torch.float32, device=mulv.device)
    if rng:
        L.check(L.load().vg_reparam_forward_rng(mulv.data_ptr(), eps.state.data_ptr(), eps.draw, z.data_ptr(),
                                                lvc.data_ptr(), B, L_dim, MP, ZP, dtype, L.stream_ptr()),
                "vg_reparam_forward_rng")
        return z, lvc
    L.check(L.load().vg_reparam_forward(mulv.data_ptr(), eps.data_ptr(), z.data_ptr(), lvc.data_ptr(), B, L_dim, MP,
                                        ZP, dtype, L.stream_ptr()), "vg_reparam_forward")
    return z, lvc


def prior_forward(eps, B, L_dim, ZP, dtype):
    """z_p [B, 1, 1, ZP] in the engine dtype = eps [B, L_dim] (f32 tensor, or a NoiseDraw generated in the kernel), pad columns
    zero: the Generator's input for a latent drawn from the prior N(0, I) (vg_prior_forward; reparam_forward on mu = 0,
    logvar = 0 bit for bit)."""
    rng = isinstance(eps, NoiseDraw)
    if rng:
        dev = eps.state.device
    else:
        _need_cuda(eps)
        if eps.dtype != torch.float32 or eps.numel() != B * L_dim:
            raise RuntimeError("prior_forward: eps must be f32 [B, L]")
        dev = eps.device
    if B <= 0 or L_dim <= 0 or ZP < L_dim or ZP % 4 != 0:
        raise ValueError("prior_forward: B, L > 0 and ZP >= L, a multiple of 4 (geometry.padc)")
    z = empty_act((B, 1, 1, ZP), dtype, dev)
    if rng:
        L.check(L.load().vg_prior_forward_rng(eps.state.data_ptr(), eps.draw, z.data_ptr(), B, L_dim, ZP, dtype,
                                              L.stream_ptr()), "vg_prior_forward_rng")
        return z
    L.check(L.load().vg_prior_forward(eps.data_ptr(), z.data_ptr(), B, L_dim, ZP, dtype, L.stream_ptr()), "vg_prior_forward")
    return z


def kl_forward(mulv, lvc, L_dim, divisor, dtype, out=None, mse=None):
    """mse = (workspace, nparts, n, loss slot) from mse_forward_backward(..., defer_final=True): the MSE's final sum is
    formed by this launch (vg_kl_forward_mse_final), same arithmetic as its own finalize launch."""
    B, MP = mulv.shape[0], mulv.shape[-1]
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=mulv.device)
    if mse is not None:
        ws, nparts, n, slot = mse
        L.check(L.load().vg_kl_forward_mse_final(mulv.data_ptr(), lvc.data_ptr(), B, L_dim, MP, divisor, out.data_ptr(),
                                                 ws.data_ptr(), nparts, n, slot.data_ptr(), dtype, L.stream_ptr()),
                "vg_kl_forward_mse_final")
        return out
    L.check(L.load().vg_kl_forward(mulv.data_ptr(), lvc.data_ptr(), B, L_dim, MP, divisor, out.data_ptr(), dtype,
                                   L.stream_ptr()), "vg_kl_forward")
    return out


def reparam_kl_backward(mulv, lvc, eps, dz, kl_scale, L_dim, dtype):
    B, MP = mulv.shape[0], mulv.shape[-1]
    ZP = dz.shape[-1]
    dmulv = torch.empty_like(mulv)
    if isinstance(eps, NoiseDraw):
        L.check(L.load().vg_reparam_kl_backward_rng(mulv.data_ptr(), lvc.data_ptr(), eps.state.data_ptr(), eps.draw,
                                                    dz.data_ptr(), kl_scale, dmulv.data_ptr(), B, L_dim, MP, ZP, dtype,
                                                    L.stream_ptr()), "vg_reparam_kl_backward_rng")
        return dmulv
    L.check(L.load().vg_reparam_kl_backward(mulv.data_ptr(), lvc.data_ptr(), eps.data_ptr(), dz.data_ptr(), kl_scale,
                                            dmulv.data_ptr(), B, L_dim, MP, ZP, dtype, L.stream_ptr()),
            "vg_reparam_kl_backward")
    return dmulv


def dot_sigmoid_forward(x, w, B, K, dtype):
    p = torch.empty(B, dtype=torch.float32, device=x.device)
    L.check(L.load().vg_dot_sigmoid_forward(x.data_ptr(), w.data_ptr(), p.data_ptr(), B, K, dtype, L.stream_ptr()),
            "vg_dot_sigmoid_forward")
    return p


def dot_sigmoid_backward(p, dp, w, B, K, dtype, need_dx, like):
    dlogit = torch.empty(B, dtype=torch.float32, device=p.device)
    dx = torch.empty_like(like) if need_dx else None
    L.check(L.load().vg_dot_sigmoid_backward(p.data_ptr(), dp.data_ptr(), w.data_ptr(), L.ptr(dx), dlogit.data_ptr(),
                                             B, K, dtype, L.stream_ptr()), "vg_dot_sigmoid_backward")
    return dx, dlogit


def dot_wgrad(x, dlogit, dw, B, K, C, HW, accumulate, dtype):
    L.check(L.load().vg_dot_wgrad(x.data_ptr(), dlogit.data_ptr(), dw.data_ptr(), B, K, C, HW,
                                  1 if accumulate else 0, dtype, L.stream_ptr()), "vg_dot_wgrad")


HEAD_BWD_MAXROWS = 4096


def head_backward(p, x, w, B, groups, target0, target1, gscale, loss, accumulate_loss, dw, accumulate_dw, K, C, HW, dtype,
                  need_dx):
    """BCE(sigmoid(head)) backward in one launch (vg_head_backward): p [groups*B] probabilities, x the head's input
    [groups*B, K] (NHWC-flattened), w its packed weight [K]; loss[0] (+)= the groups' BCE means; returns dx (or None);
    dw (f32, reference layout, or None) (+)= the weight gradient.  Bit-identical to bce[_pair]_forward_backward +
    dot_sigmoid_backward + dot_wgrad."""
    _need_cuda(p, x, w, loss, dw)
    dx = torch.empty_like(x) if need_dx else None
    L.check(L.load().vg_head_backward(p.data_ptr(), x.data_ptr(), w.data_ptr(), L.ptr(dx), L.ptr(dw), 0, B, groups,
                                      target0, target1, gscale, loss.data_ptr(), 1 if accumulate_loss else 0,
                                      1 if accumulate_dw else 0, K, C, HW, dtype, L.stream_ptr()), "vg_head_backward")
    return dx


def head_backward_g(p, x, w, B, targets, gscale, loss, accumulate_loss, dw, accumulate_dw, K, C, HW, dtype, need_dx,
                    dlogit=None):
    """head_backward for len(targets) in 1..3 groups of B rows with one target each (vg_head_backward_g; the prior stream's
    Discriminator update holds [real | reconstruction | decoded prior samples] against three targets in one launch).
    dlogit (f32 [groups * B], optional): receives the gradient w.r.t. the logits."""
    _need_cuda(p, x, w, loss, dw, dlogit)
    groups = len(targets)
    if not 1 <= groups <= 3:
        raise ValueError("head_backward_g: one to three groups")
    if p.dtype != torch.float32 or p.numel() != groups * B or x.numel() != groups * B * K or w.numel() < K:
        raise RuntimeError("head_backward_g: p must be f32 [groups * B], x [groups * B, K], w [K]")
    if x.dtype != TORCH_DT[dtype] or w.dtype != TORCH_DT[dtype] or loss.dtype != torch.float32 or \
            (dw is not None and (dw.dtype != torch.float32 or dw.numel() != C * HW)):
        raise RuntimeError("head_backward_g: x / w in the engine dtype, loss and dw (C * HW elements) f32")
    if dlogit is not None and (dlogit.dtype != torch.float32 or dlogit.numel() != groups * B):
        raise RuntimeError("head_backward_g: dlogit must be f32 [groups * B]")
    t = [float(v) for v in targets] + [0.0] * (3 - groups)
    dx = torch.empty_like(x) if need_dx else None
    L.check(L.load().vg_head_backward_g(p.data_ptr(), x.data_ptr(), w.data_ptr(), L.ptr(dx), L.ptr(dw), L.ptr(dlogit), B, groups, t[0],
                                        t[1], t[2], gscale, loss.data_ptr(), 1 if accumulate_loss else 0,
                                        1 if accumulate_dw else 0, K, C, HW, dtype, L.stream_ptr()), "vg_head_backward_g")
    return dx


def bce_forward_backward(p, target, gscale, loss, accumulate, want_grad, out=None):
    _need_cuda(p, loss, out)
    B = p.numel()
    dp = out if out is not None else (torch.empty_like(p) if want_grad else None)
    L.check(L.load().vg_bce_forward_backward(p.data_ptr(), target, B, gscale, loss.data_ptr(),
                                             1 if accumulate else 0, L.ptr(dp), L.stream_ptr()),
            "vg_bce_forward_backward")
    return dp


def bce_pair_forward_backward(p_both, target0, target1, gscale, loss, out):
    """loss[0] = BCE(p_both[:B], target0) + BCE(p_both[B:], target1); out [2B] <- the gradients.  One launch."""
    _need_cuda(p_both, loss, out)
    B = p_both.numel() // 2
    L.check(L.load().vg_bce_pair_forward_backward(p_both.data_ptr(), target0, target1, B, gscale, loss.data_ptr(), 0,
                                                  out.data_ptr(), L.stream_ptr()), "vg_bce_pair_forward_backward")
    return out


def mean_forward_backward(p, sign, gscale, loss, accumulate, want_grad, out=None):
    """loss (+)= sign*mean(p); returns dp = sign*gscale/B (WGAN losses, gan_code.py:306-315, :328)."""
    _need_cuda(p, loss, out)
    dp = out if out is not None else (torch.empty_like(p) if want_grad else None)
    L.check(L.load().vg_mean_forward_backward(p.data_ptr(), sign, p.numel(), gscale, loss.data_ptr(),
                                              1 if accumulate else 0, L.ptr(dp), L.stream_ptr()),
            "vg_mean_forward_backward")
    return dp


def clamp_(flat, lo, hi):
    """In-place clamp of a flat f32 buffer (WGAN weight clipping, gan_code.py:320-321)."""
    _need_cuda(flat)
    L.check(L.load().vg_clamp(flat.data_ptr(), flat.numel(), lo, hi, L.stream_ptr()), "vg_clamp")


def mse_forward_backward(a, b, gscale, loss, want_grad, defer_final=False):
    """defer_final=True: only the partial sums (+ gradient) are launched; returns (da, (ws, nparts, n, loss)) for
    kl_forward(..., mse=...) to finish."""
    _need_cuda(a, b, loss)
    n = a.numel()
    da = torch.empty_like(a) if want_grad else None
    ws = WS.get("mse", 1024 * 4, a.device)
    if defer_final:
        npo = c_int(0)
        L.check(L.load().vg_mse_partial(a.data_ptr(), b.data_ptr(), n, gscale, L.ptr(da), ws.data_ptr(), 1024, byref(npo),
                                        L.stream_ptr()), "vg_mse_partial")
        return da, (ws, npo.value, n, loss)
    L.check(L.load().vg_mse_forward_backward(a.data_ptr(), b.data_ptr(), n, gscale, loss.data_ptr(), L.ptr(da),
                                             ws.data_ptr(), 1024, L.stream_ptr()), "vg_mse_forward_backward")
    return da


def feat_mse_forward_backward(f_fake, f_real, d_inout, gscale, loss, accumulate, dtype):
    """Discriminator-feature reconstruction loss (vg_feat_mse_forward_backward): loss[0] (+)= mean((f_fake - f_real)^2) and,
    when d_inout is given, d_inout += gscale * 2 (f_fake - f_real) / n IN PLACE (the gradient w.r.t. f_fake joins the one
    already there; f_real is a constant).  Engine-layout activations of `dtype` whose channel rows carry no padding."""
    _need_cuda(f_fake, f_real, d_inout, loss)
    tdt = TORCH_DT[dtype]
    if f_fake.dtype != tdt or f_real.dtype != tdt or (d_inout is not None and d_inout.dtype != tdt):
        raise RuntimeError(f"feat_mse_forward_backward: tensors must all be {tdt}")
    if f_fake.shape != f_real.shape or (d_inout is not None and d_inout.numel() != f_fake.numel()):
        raise RuntimeError("feat_mse_forward_backward: f_fake, f_real and d_inout must have the same number of elements")
    ws = WS.get("featloss", 1024 * 4, f_fake.device)
    L.check(L.load().vg_feat_mse_forward_backward(f_fake.data_ptr(), f_real.data_ptr(), L.ptr(d_inout), f_fake.numel(), gscale,
                                                  loss.data_ptr(), 1 if accumulate else 0, ws.data_ptr(), 1024, dtype,
                                                  L.stream_ptr()), "vg_feat_mse_forward_backward")
    return d_inout


def ssim_loss_forward_backward(a, b, gscale, loss, accumulate, d=None):
    """SSIM reconstruction loss (vg_ssim_loss_forward_backward): loss[0] (+)= 1 - mean SSIM(a, b) over the interior pixels
    (NCHW f32 in [-1, 1], the metric's 11 x 11 Gaussian window) and, when d is given (same shape as a), d += gscale *
    d(1 - mean SSIM) / da IN PLACE: the gradient joins the one already there; b is a constant.  Returns d."""
    _need_cuda(a, b, loss, d)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or (d is not None and d.dtype != torch.float32):
        raise RuntimeError("ssim_loss_forward_backward: tensors must all be torch.float32")
    if a.dim() != 4 or a.shape != b.shape or (d is not None and d.shape != a.shape):
        raise RuntimeError("ssim_loss_forward_backward: a, b and d must be [B,C,H,W] tensors of one shape")
    B, C, H, W = a.shape
    lib = L.load()
    nws = _ws_query(lib.vg_ssim_loss_ws_floats(B, C, H, W), "vg_ssim_loss_ws_floats (needs B, C >= 1 and H, W >= 11)")
    ws = WS.get("ssimloss", nws * 4, a.device)
    L.check(lib.vg_ssim_loss_forward_backward(a.data_ptr(), b.data_ptr(), L.ptr(d), B, C, H, W, gscale, loss.data_ptr(),
                                              1 if accumulate else 0, ws.data_ptr(), nws, L.stream_ptr()),
            "vg_ssim_loss_forward_backward")
    return d


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli & Bovik 2003


def msssim_weights(H, W, scales=None):
    """The scale weights of the multi-scale SSIM for H x W images, as a tuple of floats (host only).
    scales None: M = the largest number <= 5 of 2x levels whose smaller side min(H, W) >> (M - 1) still holds the 11 x 11
    window (3 at 64, 4 at 128, 5 at 256), and the first M of (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) divided by their sum;
    an int: that M by the same rule (ValueError if the image is too small for it); a sequence of 1 - 5 positive finite
    weights: used as given, not renormalised (ValueError if the image is too small for that many levels)."""
    H, W = int(H), int(W)
    side = min(H, W)
    if side < 11:
        raise ValueError(f"msssim_weights: images of at least 11 x 11 pixels (the 11 x 11 window), got {H} x {W}")
    fit = max(m for m in range(1, 6) if (side >> (m - 1)) >= 11)
    if scales is None or (isinstance(scales, int) and not isinstance(scales, bool)):
        M = fit if scales is None else scales
        if not 1 <= M <= 5:
            raise ValueError(f"msssim_weights: 1 to 5 scales, got {M}")
        if M > fit:
            raise ValueError(f"msssim_weights: {M} scales need min(H, W) >> {M - 1} >= 11, got {H} x {W} (at most {fit})")
        s = math.fsum(MSSSIM_WEIGHTS[:M])
        return tuple(w / s for w in MSSSIM_WEIGHTS[:M])
    try:
        if isinstance(scales, (str, bytes)):
            raise TypeError
        w = tuple(float(x) for x in scales)
    except TypeError:
        raise ValueError(f"msssim_weights: scales must be None, an int or a sequence of weights, got {scales!r}") from None
    if not 1 <= len(w) <= 5 or not all(math.isfinite(x) and x > 0 for x in w):
        raise ValueError(f"msssim_weights: 1 to 5 positive finite weights, got {w}")
    if len(w) > fit:
        raise ValueError(f"msssim_weights: {len(w)} scales need min(H, W) >> {len(w) - 1} >= 11, got {H} x {W} (at most {fit})")
    return w


def msssim_loss_forward_backward(a, b, weights, gscale, loss, accumulate, d=None, per_scale=None):
    """Multi-scale SSIM reconstruction loss (vg_msssim_loss_forward_backward): loss[0] (+)= 1 - mean_b prod_j m_{b,j}^{w_j}
    over a 2x pyramid of len(weights) levels (NCHW f32 in [-1, 1]; contrast-structure means below the last level, the SSIM
    mean at it; an image with a non-positive mean contributes 0) and, when d is given (same shape as a), d += gscale *
    d loss / da IN PLACE: the gradient joins the one already there; b is a constant.  per_scale: f32 [B, M] receives the
    per-image, per-level means.  Returns d."""
    _need_cuda(a, b, loss, d, per_scale)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or (d is not None and d.dtype != torch.float32):
        raise RuntimeError("msssim_loss_forward_backward: tensors must all be torch.float32")
    if a.dim() != 4 or a.shape != b.shape or (d is not None and d.shape != a.shape):
        raise RuntimeError("msssim_loss_forward_backward: a, b and d must be [B,C,H,W] tensors of one shape")
    B, C, H, W = a.shape
    w = tuple(float(x) for x in weights)
    M = len(w)
    if not 1 <= M <= 5 or not all(math.isfinite(x) and x > 0 for x in w):
        raise RuntimeError(f"msssim_loss_forward_backward: 1 to 5 positive finite weights, got {w}")
    if per_scale is not None and (per_scale.dtype != torch.float32 or tuple(per_scale.shape) != (B, M)
                                  or not per_scale.is_contiguous()):
        raise RuntimeError("msssim_loss_forward_backward: per_scale must be a contiguous f32 [B, M] tensor")
    lib = L.load()
    nbytes = _ws_query(lib.vg_msssim_ws_bytes(B, C, H, W, M),
                       f"vg_msssim_ws_bytes (needs B, C >= 1 and H, W >= 11 at every one of the {M} levels)")
    ws = WS.get("msssim", nbytes, a.device)
    wh = (ctypes.c_float * M)(*w)
    L.check(lib.vg_msssim_loss_forward_backward(a.data_ptr(), b.data_ptr(), L.ptr(d), B, C, H, W, M, wh, gscale,
                                                loss.data_ptr(), 1 if accumulate else 0, L.ptr(per_scale), ws.data_ptr(),
                                                ws.numel() * 4, L.stream_ptr()), "vg_msssim_loss_forward_backward")
    return d


def ms_ssim(a, b, weights=None):
    """Multi-scale SSIM of two NCHW f32 batches in [-1, 1] -> device tensor [1]: 1 - the loss above (forward only).
    weights None: msssim_weights(H, W)."""
    _need_cuda(a, b)
    if a.dim() != 4:
        raise RuntimeError("ms_ssim: a and b must be [B,C,H,W] tensors")
    if weights is None:
        weights = msssim_weights(a.shape[2], a.shape[3])
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    msssim_loss_forward_backward(a, b, weights, 1.0, out, False)
    return torch.sub(1.0, out, out=out)


def region_mse_forward_backward(a, b, rects, w_hole, gscale, loss=None, hole_mse=None, want_grad=False, stats=None):
    """Region-weighted reconstruction MSE (vg_region_mse_forward_backward): a, b NCHW f32 of one shape (b a constant), rects
    f32 [B, 8] in ops.degrade_params' layout (None: no image has a hole).  loss[0] = (S_valid + w_hole S_hole) / n (written),
    hole_mse[0] = S_hole / n_hole (0 without a hole), stats f64 [4] += {S_hole, S_valid, n_hole, n_valid} (ALWAYS
    accumulated), and with want_grad the gradient of gscale * loss w.r.t. a, written in full.  -> d_a or None."""
    what = "region_mse_forward_backward"
    _need_cuda(a, b, rects, loss, hole_mse, stats)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 4 or a.shape != b.shape:
        raise RuntimeError(f"{what}: a and b must be f32 [B,C,H,W] tensors of one shape")
    B, C, H, W = a.shape
    if rects is not None and (rects.dtype != torch.float32 or tuple(rects.shape) != (B, 8)):
        raise RuntimeError(f"{what}: rects must be f32 [B, 8] (ops.degrade_params)")
    if stats is not None and (stats.dtype != torch.float64 or tuple(stats.shape) != (4,)):
        raise RuntimeError(f"{what}: stats must be f64 [4]")
    for t in (loss, hole_mse):
        if t is not None and (t.dtype != torch.float32 or t.numel() < 1):
            raise RuntimeError(f"{what}: loss and hole_mse must be f32 slots")
    if not (math.isfinite(w_hole) and w_hole >= 0):
        raise RuntimeError(f"{what}: w_hole must be finite and >= 0")
    if loss is None and hole_mse is None and stats is None and not want_grad:
        raise RuntimeError(f"{what}: nothing to compute (every output is None)")
    lib = L.load()
    nws = _ws_query(lib.vg_region_mse_ws_doubles(B, C, H, W), "vg_region_mse_ws_doubles (needs B, C, H, W >= 1)")
    ws = WS.get("regionloss", nws * 8, a.device)
    da = torch.empty_like(a) if want_grad else None
    L.check(lib.vg_region_mse_forward_backward(a.data_ptr(), b.data_ptr(), L.ptr(rects), B, C, H, W, float(w_hole),
                                               float(gscale), L.ptr(loss), L.ptr(hole_mse), L.ptr(da), L.ptr(stats),
                                               ws.data_ptr(), nws, L.stream_ptr()), "vg_region_mse_forward_backward")
    return da


# ---- test-time latent refinement (csrc/refine.hip; denoise.LatentRefiner) -----------------------------------------------
def bn_act_backward_eval(x, dy, coeffs, rows, C, act, slope, dtype, out=None):
    """Backward of eval-mode BatchNorm + activation (vg_bn_act_backward_eval): dx = dy * act'(scale x + shift) * scale with the
    constant coefficients bn_eval_coeffs made (coeffs [1][4][C]: rows 2 and 3).  x, dy: [rows][C] in the engine dtype."""
    _need_cuda(x, dy, coeffs, out)
    if coeffs is None or coeffs.dim() != 3 or coeffs.shape[0] != 1 or coeffs.shape[1] != 4 or coeffs.shape[2] != C or \
            coeffs.dtype != torch.float32:
        raise RuntimeError("bn_act_backward_eval: coeffs must be the f32 [1, 4, C] tensor of bn_eval_coeffs (one group)")
    if x.dtype != TORCH_DT[dtype] or dy.dtype != TORCH_DT[dtype] or x.numel() != rows * C or dy.numel() != rows * C:
        raise RuntimeError("bn_act_backward_eval: x and dy must be [rows, C] tensors in the engine dtype")
    dx = out if out is not None else torch.empty_like(x)
    if dx.dtype != x.dtype or dx.numel() != x.numel():
        raise RuntimeError("bn_act_backward_eval: out must have x's dtype and size")
    _bn_bytes(3, x.numel(), dtype)
    L.check(L.load().vg_bn_act_backward_eval(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), coeffs[0, 2].data_ptr(),
                                             coeffs[0, 3].data_ptr(), rows, C, act, slope, dtype, L.stream_ptr()),
            "vg_bn_act_backward_eval")
    return dx


def masked_mse_rows(a, b, rects, gscale=1.0, loss_rows=None, want_grad=False, out=None):
    """Per-image MSE outside each image's occlusion rectangle (vg_masked_mse_rows): a, b NCHW f32 of one shape (b a
    constant), rects f32 [B, 8] in ops.degrade_params' layout (None: no image has a hole; a NaN row: that image has none).
    loss_rows f32 [B] = S_valid_i / n_valid_i (written; None skips it), and with want_grad the gradient of gscale *
    loss_rows[i] w.r.t. a (exactly 0 inside the holes), written in full into ``out`` or a new tensor.  -> d_a or None."""
    what = "masked_mse_rows"
    _need_cuda(a, b, rects, loss_rows, out)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 4 or a.shape != b.shape:
        raise RuntimeError(f"{what}: a and b must be f32 [B,C,H,W] tensors of one shape")
    B, C, H, W = a.shape
    if rects is not None and (rects.dtype != torch.float32 or tuple(rects.shape) != (B, 8)):
        raise RuntimeError(f"{what}: rects must be f32 [B, 8] (ops.degrade_params)")
    if loss_rows is not None and (loss_rows.dtype != torch.float32 or loss_rows.numel() != B):
        raise RuntimeError(f"{what}: loss_rows must be f32 [B]")
    if out is not None and (not want_grad or out.dtype != torch.float32 or out.shape != a.shape):
        raise RuntimeError(f"{what}: out is the gradient tensor (want_grad=True), f32 of a's shape")
    if not math.isfinite(gscale):
        raise RuntimeError(f"{what}: gscale must be finite")
    if loss_rows is None and not want_grad:
        raise RuntimeError(f"{what}: nothing to compute (every output is None)")
    lib = L.load()
    nws = _ws_query(lib.vg_masked_mse_rows_ws_doubles(B, C, H, W),
                    "vg_masked_mse_rows_ws_doubles (needs B, C, H, W >= 1, B <= 65535, C H W < 2^31 - 2^19)")
    ws = WS.get("maskedmse", nws * 8, a.device)
    da = (out if out is not None else torch.empty_like(a)) if want_grad else None
    L.check(lib.vg_masked_mse_rows(a.data_ptr(), b.data_ptr(), L.ptr(rects), B, C, H, W, float(gscale), L.ptr(loss_rows),
                                   L.ptr(da), ws.data_ptr(), nws, L.stream_ptr()), "vg_masked_mse_rows")
    return da


# ---- classical-denoiser baseline (csrc/nlm.hip; baselines.NLMeans) ---------------------------------------------------------
def _sigma_column(what, sigma, B, device):
    """-> (tensor kept alive, element stride) of a per-image f32 noise level: None, a number, [B] or a strided 1-D view."""
    if sigma is None:
        return None, 1
    if isinstance(sigma, (int, float)) and not isinstance(sigma, bool):
        return torch.full((B,), float(sigma), dtype=torch.float32, device=device), 1
    if not isinstance(sigma, torch.Tensor) or not sigma.is_cuda or sigma.dtype != torch.float32 or sigma.dim() != 1 or \
            sigma.shape[0] != B or (B > 1 and sigma.stride(0) < 1):
        raise RuntimeError(f"{what}: sigma must be None, a number, or a device f32 tensor [B] (a strided 1-D view such as "
                           f"rects[:, 1] is read in place)")
    if sigma.device != device:
        raise RuntimeError(f"{what}: sigma is on {sigma.device}, x on {device}")
    return sigma, (sigma.stride(0) if B > 1 else 1)


def nlm_denoise(x, sigma=None, *, patch_radius=2, search_radius=7, h_factor=0.8, h_const=0.0, out=None):
    """Non-local means of an f32 [B,C,H,W] batch (vg_nlm_denoise; C <= 4): pixelwise, uniform (2P+1)^2 patch, (2R+1)^2 search
    window, reflect padding, weight exp(-max(d2 - 2 sigma_b^2, 0) / h_b^2) with h_b = h_factor * sigma_b + h_const.  sigma: None
    (0), a number (materialised once as a [B] tensor) or a device f32 tensor -- [B], or a strided 1-D view such as
    ``loader.last_rects[:, 1]``, read in place.  An image whose h_b is not a finite positive number is copied through.  One
    launch, no host synchronisation, no atomics.  -> out (f32 of x's shape, not x) or a new tensor."""
    what = "nlm_denoise"
    _need_cuda(x, out)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError(f"{what}: x must be an f32 [B,C,H,W] tensor")
    B, C, H, W = x.shape
    if out is not None and (out.dtype != torch.float32 or out.shape != x.shape or out.device != x.device):
        raise RuntimeError(f"{what}: out must be f32 of x's shape on x's device")
    for name, v in (("patch_radius", patch_radius), ("search_radius", search_radius)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise RuntimeError(f"{what}: {name} must be an integer")
    sig, stride = _sigma_column(what, sigma, B, x.device)
    y = out if out is not None else torch.empty_like(x)
    L.check(L.load().vg_nlm_denoise(x.data_ptr(), y.data_ptr(), B, C, H, W, patch_radius, search_radius, L.ptr(sig), stride,
                                    float(h_factor), float(h_const), L.stream_ptr()), "vg_nlm_denoise")
    return y


def noise_sigma(x, out=None):
    """Blind per-image noise level of an f32 [B,C,H,W] batch, H, W >= 3 (vg_noise_sigma; Immerkaer 1996): the mean absolute
    response of the 3 x 3 mask [[1,-2,1],[-2,4,-2],[1,-2,1]] over the interior, times sqrt(pi/2) / 6.  -> f32 [B] (``out``: a
    1-D f32 tensor or strided view of B elements, written in place).  One launch, fixed summation order, no host sync."""
    what = "noise_sigma"
    _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError(f"{what}: x must be an f32 [B,C,H,W] tensor")
    B, C, H, W = x.shape
    if out is not None and (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or
                            out.dim() != 1 or out.shape[0] != B or (B > 1 and out.stride(0) < 1) or out.device != x.device):
        raise RuntimeError(f"{what}: out must be an f32 tensor [B] on x's device (a strided 1-D view is written in place)")
    s = out if out is not None else torch.empty(B, dtype=torch.float32, device=x.device)
    L.check(L.load().vg_noise_sigma(x.data_ptr(), B, C, H, W, s.data_ptr(), s.stride(0) if B > 1 else 1, L.stream_ptr()),
            "vg_noise_sigma")
    return s


def median_filter(x, radius=1, out=None):
    """Per-channel (2r+1)^2 median of an f32 [B,C,H,W] batch, r = radius in {1, 2} (vg_median_filter): reflect padding as
    nlm_denoise, min(H, W) >= r + 1; the output is one of the window's values, exact for finite inputs.  One launch, no host
    synchronisation, no atomics.  -> out (f32 of x's shape, contiguous, not x) or a new tensor."""
    what = "median_filter"
    _need_cuda(x, out)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError(f"{what}: x must be an f32 [B,C,H,W] tensor")
    if isinstance(radius, bool) or not isinstance(radius, int):
        raise RuntimeError(f"{what}: radius must be an integer")
    x = x.contiguous()
    B, C, H, W = x.shape
    if out is not None and (out.dtype != torch.float32 or out.shape != x.shape or out.device != x.device or
                            not out.is_contiguous()):
        raise RuntimeError(f"{what}: out must be contiguous f32 of x's shape on x's device")
    y = out if out is not None else torch.empty_like(x)
    L.check(L.load().vg_median_filter(x.data_ptr(), y.data_ptr(), B, C, H, W, radius, L.stream_ptr()), "vg_median_filter")
    return y


def spectrum_profiles(x, plan, center=True, want_power=False):
    """Binned power spectra of an f32 [B,C,H,W] batch, B >= 1, C <= 4 (vg_spectrum_profiles): ``plan`` is a
    ``spectrum.SpectrumPlan`` of the batch's H x W (its tables are uploaded once per device); ``center`` subtracts every
    plane's mean first.  -> prof f64 [B, n_bins], or (prof, power f64 [B, H, W // 2 + 1]) with ``want_power``: the
    channel-summed |Z|^2 map.  f64 MFMA, fixed summation order, no atomics, no host synchronisation."""
    from .spectrum import SpectrumPlan
    what = "spectrum_profiles"
    _need_cuda(x)
    if not isinstance(plan, SpectrumPlan):
        raise RuntimeError(f"{what}: plan must be a spectrum.SpectrumPlan (spectrum.spectrum_plan(H, W))")
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError(f"{what}: x must be an f32 [B,C,H,W] tensor")
    if not isinstance(center, bool) or not isinstance(want_power, bool):
        raise RuntimeError(f"{what}: center and want_power must be bools")
    B, C, H, W = x.shape
    if (H, W) != (plan.H, plan.W):
        raise RuntimeError(f"{what}: the plan is for {plan.H} x {plan.W} images, x is {H} x {W}")
    if B < 1 or not 1 <= C <= 4:
        raise RuntimeError(f"{what}: need B >= 1 and 1 <= C <= 4, got B={B} C={C}")
    lib = L.load()
    need = ctypes.c_int64(0)
    L.check(lib.vg_spectrum_ws_bytes(B, C, H, W, byref(need)), "vg_spectrum_ws_bytes")
    ws = WS.get("spectrum", need.value, x.device)
    t = plan.device_tables(x.device)
    prof = torch.empty(B, plan.n_bins, dtype=torch.float64, device=x.device)
    power = torch.empty(B, H, plan.Wh, dtype=torch.float64, device=x.device) if want_power else None
    L.check(lib.vg_spectrum_profiles(x.data_ptr(), B, C, H, W, int(center), t["tw_re"].data_ptr(), t["tw_im"].data_ptr(),
                                     t["th_re"].data_ptr(), t["th_im"].data_ptr(), t["weight"].data_ptr(),
                                     t["order"].data_ptr(), t["bin_start"].data_ptr(), plan.n_bins, L.ptr(power),
                                     prof.data_ptr(), ws.data_ptr(), ws.numel() * 4, L.stream_ptr()), "vg_spectrum_profiles")
    return (prof, power) if want_power else prof


def spectrum_accum(prof, sum, sumsq):
    """Running profile statistics (vg_spectrum_accum): sum f64 [n_bins] += prof[b], sumsq += prof[b]^2 over the rows of prof
    f64 [b, n_bins] in ascending b (b >= 0), one thread per bin.  In place; no host sync.  -> (sum, sumsq)."""
    what = "spectrum_accum"
    _need_cuda(prof, sum, sumsq)
    if prof.dtype != torch.float64 or prof.dim() != 2:
        raise RuntimeError(f"{what}: prof must be an f64 [b, n_bins] tensor")
    b, n = prof.shape
    if (sum.dtype != torch.float64 or sumsq.dtype != torch.float64 or tuple(sum.shape) != (n,) or tuple(sumsq.shape) != (n,)
            or sum.device != prof.device or sumsq.device != prof.device):
        raise RuntimeError(f"{what}: sum and sumsq must be f64 [{n}] on prof's device")
    if b == 0:
        return sum, sumsq
    L.check(L.load().vg_spectrum_accum(prof.data_ptr(), b, n, sum.data_ptr(), sumsq.data_ptr(), L.stream_ptr()),
            "vg_spectrum_accum")
    return sum, sumsq


LATENT_MODE = {"init": L.VG_LATENT_INIT, "update": L.VG_LATENT_UPDATE, "track": L.VG_LATENT_TRACK}


def latent_state(B, L_dim, device):
    """The optimiser state of vg_latent_adam for B latent rows: dict(z, m, v, best_z f32 [B, L]; t int32 [B]; best_loss f32 [B]).
    Uninitialised: latent_adam("init", ...) fills it."""
    f = dict(dtype=torch.float32, device=device)
    return dict(z=torch.empty(B, L_dim, **f), m=torch.empty(B, L_dim, **f), v=torch.empty(B, L_dim, **f),
                best_z=torch.empty(B, L_dim, **f), best_loss=torch.empty(B, **f),
                t=torch.empty(B, dtype=torch.int32, device=device))


def latent_adam(mode, state, dtype, ZP, *, dz=None, loss_rows=None, p=None, z_in=None, z_out=None, objective=None,
                lr=0.0, betas=(0.9, 0.999), eps=1e-8, alpha_adv=0.0, prior_weight=0.0):
    """Objective, keep-best and one Adam step over latent rows (vg_latent_adam).  mode: "init" (state from z_in [B, ZP] in the
    engine dtype), "update" (objective of the z just evaluated from loss_rows [B] (+ p [B]), keep-best, Adam on dz [B, ZP],
    z_out [B, ZP] = the next Generator input) or "track" (objective and keep-best only).  objective f32 [B]: receives J."""
    what = "latent_adam"
    if mode not in LATENT_MODE:
        raise ValueError(f"{what}: mode must be 'init', 'update' or 'track', got {mode!r}")
    z = state["z"]
    B, L_dim = z.shape
    _need_cuda(*state.values(), dz, loss_rows, p, z_in, z_out, objective)
    for k in ("z", "m", "v", "best_z"):
        if state[k].dtype != torch.float32 or tuple(state[k].shape) != (B, L_dim):
            raise RuntimeError(f"{what}: state['{k}'] must be f32 [B, L]")
    if state["best_loss"].dtype != torch.float32 or state["best_loss"].numel() != B or state["t"].dtype != torch.int32 or \
            state["t"].numel() != B:
        raise RuntimeError(f"{what}: state['best_loss'] must be f32 [B] and state['t'] int32 [B]")
    for name, t in (("dz", dz), ("z_in", z_in), ("z_out", z_out)):
        if t is not None and (t.dtype != TORCH_DT[dtype] or t.numel() != B * ZP):
            raise RuntimeError(f"{what}: {name} must be [B, ZP] in the engine dtype")
    for name, t in (("loss_rows", loss_rows), ("p", p), ("objective", objective)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != B):
            raise RuntimeError(f"{what}: {name} must be f32 [B]")
    need = {"init": (("z_in", z_in),), "update": (("dz", dz), ("loss_rows", loss_rows), ("z_out", z_out)),
            "track": (("loss_rows", loss_rows),)}[mode]
    for name, t in need:
        if t is None:
            raise RuntimeError(f"{what}: mode '{mode}' needs {name}")
    L.check(L.load().vg_latent_adam(z.data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), state["t"].data_ptr(),
                                    state["best_loss"].data_ptr(), state["best_z"].data_ptr(), L.ptr(dz), L.ptr(loss_rows),
                                    L.ptr(p), L.ptr(z_in), L.ptr(z_out), L.ptr(objective), B, L_dim, ZP, float(lr),
                                    float(betas[0]), float(betas[1]), float(eps), float(alpha_adv), float(prior_weight),
                                    LATENT_MODE[mode], dtype, L.stream_ptr()), "vg_latent_adam")


# draw id of the augmentation table (include/vaegan_hip.h "Differentiable augmentation"): outside 0..2, 16..18 and 32..34
DRAW_AUGMENT = 48
AUG_BRIGHTNESS, AUG_SATURATION, AUG_CONTRAST, AUG_TRANSLATION, AUG_CUTOUT = 1, 2, 4, 8, 16


def diffaug_cut(policy: int, H: int, W: int):
    """(cut_h, cut_w) the apply launches take for a table drawn with `policy`: floor(size / 2 + 0.5), or (0, 0) when the
    cutout bit is clear."""
    return ((H + 1) // 2, (W + 1) // 2) if policy & AUG_CUTOUT else (0, 0)


def diffaug_params(state: torch.Tensor, B: int, policy: int, H: int, W: int, out=None) -> torch.Tensor:
    """-> f32 [B, 8] on the device = {beta, s, k, ty, tx, cy, cx, 0} per image (vg_diffaug_params), drawn from state
    (int64[2] = {seed, counter}, NoiseStream.state) with draw id DRAW_AUGMENT; policy: a sum of the AUG_* bits."""
    _need_cuda(state, out)
    if state.dtype != torch.int64 or state.numel() != 2:
        raise RuntimeError("diffaug_params: state must be the int64[2] {seed, counter} of a NoiseStream")
    if not 0 <= int(policy) < 32:
        raise RuntimeError("diffaug_params: policy is a sum of the AUG_* bits (0..31)")
    y = out if out is not None else torch.empty(B, 8, dtype=torch.float32, device=state.device)
    if y.dtype != torch.float32 or tuple(y.shape) != (B, 8):
        raise RuntimeError("diffaug_params: out must be f32 [B, 8]")
    L.check(L.load().vg_diffaug_params(state.data_ptr(), B, int(policy), H, W, y.data_ptr(), L.stream_ptr()),
            "vg_diffaug_params")
    return y


def _diffaug(name, fn_name, x, params, C, cut, dtype, out, need_sum):
    _need_cuda(x, params, out)
    if x.dtype != TORCH_DT[dtype] or x.dim() != 4:
        raise RuntimeError(f"{name}: the image must be an engine-layout [N,H,W,CP] tensor of {TORCH_DT[dtype]}")
    if params.dtype != torch.float32 or params.dim() != 2 or params.shape[1] != 8 or params.shape[0] < 1:
        raise RuntimeError(f"{name}: params must be f32 [PB, 8] (ops.diffaug_params)")
    N, H, W, CP = x.shape
    PB = params.shape[0]
    if N % PB != 0:
        raise RuntimeError(f"{name}: the number of images must be a multiple of the parameter rows")
    y = out if out is not None else torch.empty_like(x)
    if y.shape != x.shape or y.dtype != x.dtype:
        raise RuntimeError(f"{name}: out must match the input")
    lib = L.load()
    ws, nws = None, 0
    if need_sum:
        nws = _ws_query(lib.vg_diffaug_ws_floats(N, H, W), "vg_diffaug_ws_floats (needs N, H, W >= 1)")
        ws = WS.get("diffaug", nws * 4, x.device)
    L.check(getattr(lib, fn_name)(x.data_ptr(), y.data_ptr(), params.data_ptr(), N, PB, H, W, C, CP, int(cut[0]), int(cut[1]),
                                  L.ptr(ws), nws, dtype, L.stream_ptr()), fn_name)
    return y


def diffaug_forward(x, params, C, cut, dtype, out=None, need_sum=True):
    """y = T(x) (vg_diffaug_forward): colour, translation and cutout per image of x [N,H,W,CP] (engine layout, C real channels)
    by the rows of params [PB, 8], image n using row n % PB; cut = (cut_h, cut_w) (ops.diffaug_cut).  need_sum=False skips the
    whole-image mean's reduce launch (only for tables whose k is 1 everywhere)."""
    return _diffaug("diffaug_forward", "vg_diffaug_forward", x, params, C, cut, dtype, out, need_sum)


def diffaug_backward(g, params, C, cut, dtype, out=None, need_sum=True):
    """dx = T'(g) (vg_diffaug_backward): the exact adjoint of diffaug_forward's linear part, same arguments."""
    return _diffaug("diffaug_backward", "vg_diffaug_backward", g, params, C, cut, dtype, out, need_sum)


def axpy(a, b, alpha, out=None):
    out = out if out is not None else torch.empty_like(a)
    L.check(L.load().vg_axpy(a.data_ptr(), b.data_ptr(), alpha, out.data_ptr(), a.numel(), L.stream_ptr()), "vg_axpy")
    return out


def step_prologue(noise, optimizers, zero=None) -> None:
    """Top of an iteration, one single-thread launch: noise.advance() (noise may be None), the step counters / bias
    corrections of `optimizers` (optim.Adam, at most 4) -- their step(prepared=True) then launches the update alone --
    and, when given, the iteration's loss slots `zero` (f32, <= 64 elements) set to 0 (instead of a memset node).
    An optimizer with a learning-rate schedule or a decoupled weight decay (optim.LRSchedule, optim.AdamW) has its rate of this
    step and its decay factor worked out in the same launch from the step count on the device."""
    import ctypes
    n = len(optimizers)
    states = (ctypes.c_void_p * max(n, 1))(*[o.state_dev.data_ptr() for o in optimizers])
    lr = (ctypes.c_double * max(n, 1))(*[o.lr for o in optimizers])
    b1 = (ctypes.c_double * max(n, 1))(*[o.betas[0] for o in optimizers])
    b2 = (ctypes.c_double * max(n, 1))(*[o.betas[1] for o in optimizers])
    recs = [o.sched_record() if hasattr(o, "sched_record") else None for o in optimizers]
    if any(r is not None for r in recs):
        # some optimizer has a learning-rate schedule or a decoupled decay: the same launch evaluates them on the device
        # (vg_step_prologue_sched; entries of the others are NULL -- vg_step_prologue's bits for those)
        sched = (ctypes.c_void_p * n)(*[None if r is None else ctypes.addressof(r) for r in recs])
        L.check(L.load().vg_step_prologue_sched(noise.state.data_ptr() if noise is not None else None, states, lr, b1, b2,
                                                sched, n, L.ptr(zero), 0 if zero is None else zero.numel(), L.stream_ptr()),
                "vg_step_prologue_sched")
        return
    L.check(L.load().vg_step_prologue(noise.state.data_ptr() if noise is not None else None, states, lr, b1, b2, n,
                                      L.ptr(zero), 0 if zero is None else zero.numel(), L.stream_ptr()), "vg_step_prologue")


def adam_apply2(opt_a, opt_b) -> None:
    """The prepared update of TWO optim.Adam instances in one launch (vg_adam_apply2); bit-identical to two adam_step(...,
    prepared=True) launches."""
    import ctypes
    oo = (opt_a, opt_b)
    arr = lambda f: (ctypes.c_void_p * 2)(*[f(o) for o in oo])       # noqa: E731
    n = (ctypes.c_int64 * 2)(*[o.flat_p.numel() for o in oo])
    b1 = (ctypes.c_double * 2)(*[o.betas[0] for o in oo])
    b2 = (ctypes.c_double * 2)(*[o.betas[1] for o in oo])
    eps = (ctypes.c_double * 2)(*[o.eps for o in oo])
    gs = (ctypes.c_float * 2)(*[o.grad_scale for o in oo])
    L.check(L.load().vg_adam_apply2(arr(lambda o: o.flat_p.data_ptr()), arr(lambda o: o.flat_g.data_ptr()),
                                    arr(lambda o: o.exp_avg.data_ptr()), arr(lambda o: o.exp_avg_sq.data_ptr()), n, b1, b2,
                                    eps, gs, arr(lambda o: o.state_dev.data_ptr()), L.stream_ptr()), "vg_adam_apply2")


def ema_update(ema, p, state, decay, warmup) -> None:
    """Weight averaging, ONE launch for up to 4 flat f32 buffers (vg_ema_update, include/vaegan_hip.h "Weight averaging"):
    ema[i] += (1 - d_i) * (p[i] - ema[i]) with d_i = decay[i], capped at (1 + t) / (10 + t) where warmup[i] is set; t =
    state[i][0], the optimizer's device-resident step count (state[i] may be None where warmup[i] is off).  Lists of equal
    length; ema[i] / p[i] contiguous f32 device tensors of one size.  Capturable."""
    import ctypes
    k = len(ema)
    if not (len(p) == len(state) == len(decay) == len(warmup) == k):
        raise ValueError("ema_update: ema, p, state, decay and warmup must have one length")
    if not 1 <= k <= L.VG_EMA_MAX:
        raise ValueError(f"ema_update: 1..{L.VG_EMA_MAX} buffers per launch, got {k}")
    _need_cuda(*ema, *p, *state)
    for e, q in zip(ema, p):
        if e.dtype != torch.float32 or q.dtype != torch.float32 or e.numel() != q.numel():
            raise RuntimeError("ema_update: ema[i] and p[i] must be f32 tensors of one size")
    arr = lambda ts: (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])       # noqa: E731
    L.check(L.load().vg_ema_update(arr(ema), arr(p), (ctypes.c_int64 * k)(*[q.numel() for q in p]), arr(state),
                                   (ctypes.c_double * k)(*[float(d) for d in decay]),
                                   (ctypes.c_int * k)(*[int(bool(w)) for w in warmup]), k, L.stream_ptr()), "vg_ema_update")


def grad_norm_clip(grads, grad_scales, max_norms, out, ws) -> None:
    """Gradient-norm clipping, the reduction (vg_grad_norm_clip, include/vaegan_hip.h "Gradient-norm clipping"): for up to 4
    flat f32 gradient buffers, out[i] = [norm_i, coef_i] with norm_i = |grad_scales[i]| * ||grads[i]||_2 (f64 sum in a fixed
    order) and coef_i = min(1, max_norms[i] / (norm_i + 1e-6)) as torch.nn.utils.clip_grad_norm_ forms it -- each buffer
    against its OWN norm.  TWO launches; nothing is synchronised and grads are not rewritten (adam_apply_clip applies the
    coefficient).  Lists of equal length; out[i]: f32 device tensor of >= 2 elements; ws: f64 device tensor of at least
    VG_GNORM_MAX * VG_GNORM_PARTS elements.  Capturable."""
    import ctypes
    k = len(grads)
    if not (len(grad_scales) == len(max_norms) == len(out) == k):
        raise ValueError("grad_norm_clip: grads, grad_scales, max_norms and out must have one length")
    if not 1 <= k <= L.VG_GNORM_MAX:
        raise ValueError(f"grad_norm_clip: 1..{L.VG_GNORM_MAX} buffers per call, got {k}")
    _need_cuda(*grads, *out, ws)
    for g, o in zip(grads, out):
        if g.dtype != torch.float32 or not g.is_contiguous():
            raise RuntimeError("grad_norm_clip: grads[i] must be contiguous f32 tensors")
        if o.dtype != torch.float32 or o.numel() < 2 or not o.is_contiguous() or o.device != g.device:
            raise RuntimeError("grad_norm_clip: out[i] must be a contiguous f32 tensor of >= 2 elements on grads[i]'s device")
    if ws.dtype != torch.float64 or ws.numel() < L.VG_GNORM_MAX * L.VG_GNORM_PARTS or ws.device != grads[0].device:
        raise RuntimeError(f"grad_norm_clip: ws must hold {L.VG_GNORM_MAX * L.VG_GNORM_PARTS} f64 on the gradients' device")
    arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])       # noqa: E731
    L.check(L.load().vg_grad_norm_clip(arr(grads), (ctypes.c_int64 * k)(*[g.numel() for g in grads]),
                                       (ctypes.c_float * k)(*[float(s) for s in grad_scales]),
                                       (ctypes.c_double * k)(*[float(m) for m in max_norms]), k, arr(out), ws.data_ptr(),
                                       L.stream_ptr()), "vg_grad_norm_clip")


def adam_apply_clip(opts, coefs) -> None:
    """The prepared update of ONE or TWO optim.Adam instances in one launch with the gradient scale grad_scale * coefs[i][0],
    the coefficient read from the device (vg_adam_apply_clip); coefs[i] None: grad_scale as it is, i.e. adam_apply2's /
    adam_step(prepared=True)'s bits for that optimizer.  With an optim.AdamW among them the launch is vg_adamw_apply: each
    optimizer's parameters are first multiplied by its state_dev[3] (1 - lr_t * weight_decay from the prologue; 1 for a plain
    Adam)."""
    import ctypes
    k = len(opts)
    if len(coefs) != k:
        raise ValueError("adam_apply_clip: opts and coefs must have one length")
    if k not in (1, 2):
        raise ValueError(f"adam_apply_clip: 1 or 2 optimizers per launch, got {k}")
    for o, c in zip(opts, coefs):
        if c is not None:
            _need_cuda(c)
            if c.dtype != torch.float32 or c.numel() < 1 or c.device != o.flat_p.device:
                raise RuntimeError("adam_apply_clip: coefs[i] must be an f32 tensor on the optimizer's device (or None)")
    arr = lambda f: (ctypes.c_void_p * k)(*[f(o) for o in opts])       # noqa: E731
    # an AdamW in the launch: vg_adamw_apply, which multiplies every parameter by its optimizer's state_dev[3] first
    decay = any(getattr(o, "_DECOUPLED", False) for o in opts)
    fn, name = (L.load().vg_adamw_apply, "vg_adamw_apply") if decay else (L.load().vg_adam_apply_clip, "vg_adam_apply_clip")
    L.check(fn(
        arr(lambda o: o.flat_p.data_ptr()), arr(lambda o: o.flat_g.data_ptr()), arr(lambda o: o.exp_avg.data_ptr()),
        arr(lambda o: o.exp_avg_sq.data_ptr()), (ctypes.c_int64 * k)(*[o.flat_p.numel() for o in opts]),
        (ctypes.c_double * k)(*[o.betas[0] for o in opts]), (ctypes.c_double * k)(*[o.betas[1] for o in opts]),
        (ctypes.c_double * k)(*[o.eps for o in opts]), (ctypes.c_float * k)(*[o.grad_scale for o in opts]),
        arr(lambda o: o.state_dev.data_ptr()), (ctypes.c_void_p * k)(*[None if c is None else c.data_ptr() for c in coefs]),
        k, L.stream_ptr()), name)


def launch_count() -> int:
    """Kernel launches libvaegan_hip.so has issued so far in this process (vg_launch_count)."""
    return int(L.load().vg_launch_count())


def adam_step(p, g, m, v, lr, beta1, beta2, eps, grad_scale, state, prepared: bool = False):
    """prepared=True: `state` (step count, bias corrections) was advanced by this iteration's step_prologue; only the
    update kernel is launched (vg_adam_apply)."""
    _need_cuda(p, g, m, v, state)
    if lr < 0:
        raise ValueError(f"Invalid learning rate: {lr}")
    if BINDING == "torchops":
        torch_ops().adam_step(p, g, m, v, lr, beta1, beta2, eps, grad_scale, state, bool(prepared))
        return
    if prepared:
        L.check(L.load().vg_adam_apply(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), beta1, beta2, eps,
                                       grad_scale, state.data_ptr(), L.stream_ptr()), "vg_adam_apply")
        return
    L.check(L.load().vg_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1,
                                  beta2, eps, grad_scale, state.data_ptr(), L.stream_ptr()), "vg_adam_step")


import os as _os
if _os.environ.get("VG_BINDING"):
    set_binding(_os.environ["VG_BINDING"])
