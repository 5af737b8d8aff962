"""GPU: gradient-norm clipping (vg_grad_norm_clip in csrc/gradclip.hip, vg_adam_apply_clip in csrc/pack_adam.hip;
vaegan_amd.clip_grad_norm_, max_grad_norm= on the trainers) -- the reduction against the numpy restatement of
tests/_gradclip_ref.py bit for bit on integer gradients (any order of the f64 sum gives the same integer) and to one f32 ulp on
random ones, the clipped Adam launch against the unclipped launches fed the same scale bit for bit, and the option through the
optimizers and the four trainers: what it leaves alone, what it launches, what it reports, twins, the oracle, graph replay."""
import functools
import math
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _gradclip_ref as GR
import vaegan_amd as V
import vaegan_ref as R
from _inputs import make_inputs

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))
DEV = "cuda"
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
L = import_module(PKG + "._lib")
F32 = np.float32
INF = math.inf
GUARD = 64
CAP = L.VG_GNORM_PARTS * 256 * 16                 # elements the largest grid of one buffer covers in ONE sweep per workgroup
SIZES = [1, 3, 4, 5, 1024, 1029, CAP, CAP + 3 * 1024 + 1]
WS_N = L.VG_GNORM_MAX * L.VG_GNORM_PARTS


class Guarded:
    """A buffer between two 64-element NaN guards (the buffer itself stays 16-byte aligned); tests/test_gpu_ema.py."""

    def __init__(self, values: np.ndarray):
        n = values.size
        host = np.full(n + 2 * GUARD, np.nan, dtype=values.dtype)
        host[GUARD:GUARD + n] = values
        self.host0 = host
        self.whole = torch.from_numpy(host.copy()).to(DEV)
        self.t = self.whole[GUARD:GUARD + n]

    def guards_intact(self) -> bool:
        got = self.whole.cpu().numpy()
        iv = np.int32 if got.dtype == F32 else np.int64
        return np.array_equal(got[:GUARD].view(iv), self.host0[:GUARD].view(iv)) and \
            np.array_equal(got[-GUARD:].view(iv), self.host0[-GUARD:].view(iv))

    def values(self) -> np.ndarray:
        return self.whole.cpu().numpy()[GUARD:-GUARD].copy()


@functools.lru_cache(maxsize=None)
def dev_grads(kind, n, seed):
    """(host array, device tensor) of one input, made once and never written."""
    g = (GR.int_grads if kind == "int" else GR.float_grads)(n, seed)
    if kind == "int":
        GR.check_conditions(g)
    return g, torch.from_numpy(g).to(DEV)


def launch(bufs):
    """bufs: [(device g, grad_scale, max_norm)] -> [out_i as 2 np.float32] after ONE call; checks the launch count, the guards
    around out and ws, and that g is unchanged is left to the caller."""
    outs = [Guarded(np.full(2, np.nan, dtype=F32)) for _ in bufs]
    ws = Guarded(np.full(WS_N, np.nan, dtype=np.float64))
    before = ops.launch_count()
    ops.grad_norm_clip([b[0] for b in bufs], [b[1] for b in bufs], [b[2] for b in bufs], [o.t for o in outs], ws.t)
    assert ops.launch_count() - before == 2
    torch.cuda.synchronize()
    assert ws.guards_intact(), "guard around the workspace touched"
    for o in outs:
        assert o.guards_intact(), "guard around out touched"
    return [o.values() for o in outs]


# ---- vg_grad_norm_clip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_integer_gradients_match_the_restatement_bitwise(n):
    g, gd = dev_grads("int", n, 100 + n % 97)
    for scale in (1.0, 0.5):
        for max_norm in GR.max_norms_around(g, scale) + [INF, 0.0]:
            (out,) = launch([(gd, scale, max_norm)])
            want = GR.norm_coef(g, scale, max_norm)
            assert GR.same_bits(out, np.array(want, dtype=F32)), (n, scale, max_norm, out, want)
        above, below, equal = (GR.norm_coef(g, scale, m)[1] for m in GR.max_norms_around(g, scale))
        assert above == 1.0 and below < 1.0 and equal <= 1.0
    assert np.array_equal(gd.cpu().numpy().view(np.int32), g.view(np.int32)), "g is read only"


@pytest.mark.parametrize("n", SIZES)
def test_random_gradients_are_within_one_ulp_of_the_restatement(n):
    """The kernel's and numpy's f64 sums add the same exact products in different orders: each is within n 2^-53 relative
    of S (n <= 2.1e6: 2.4e-10), so the two f64 norms differ by at most that -- far below half an f32 ulp (6e-8 relative) -- and
    the ONE narrowing to f32 can land on neighbouring values only where the f64 norm sits that close to a rounding boundary: at
    most 1 ulp in out[0].  The coefficient is a quotient of that norm and inherits the same 1-ulp bound."""
    g, gd = dev_grads("float", n, 200 + n % 97)
    norm64, _ = GR.norm_coef_f64(g, 1.0, INF)
    for scale, max_norm in ((1.0, 0.5 * norm64), (1.0 / 3.0, 0.1 * norm64), (1.0, INF)):
        (out,) = launch([(gd, scale, max_norm)])
        want = GR.norm_coef(g, scale, max_norm)
        d = [GR.ulp_distance(out[0], want[0]), GR.ulp_distance(out[1], want[1])]
        print(f"n={n} scale={scale:.3f}: norm {out[0]!r} / {want[0]!r}, coef {out[1]!r} / {want[1]!r}, ulp distances {d}")
        assert d[0] <= 1 and d[1] <= 1
        if max_norm == INF:
            assert out[1] == 1.0
    assert np.array_equal(gd.cpu().numpy().view(np.int32), g.view(np.int32))


def test_several_buffers_in_one_call_equal_their_single_calls_and_repeat_bitwise():
    sizes = [5, 1029, CAP + 3 * 1024 + 1, 1024 * 37 + 2]
    cfg = [(1.0, 0.25), (0.5, INF), (1.0 / 3.0, 3.0), (1.0, 1e-3)]
    bufs = [(dev_grads("float", n, 300 + i)[1],) + c for i, (n, c) in enumerate(zip(sizes, cfg))]
    singles = [launch([b])[0] for b in bufs]
    for count in (1, 2, 3, 4):
        for rot in range(4):                                    # every buffer in every position of the grid
            sel = [bufs[(i + rot) % 4] for i in range(count)]
            first, second = launch(sel), launch(sel)
            for i in range(count):
                assert np.array_equal(first[i].view(np.int32), singles[(i + rot) % 4].view(np.int32)), (count, rot, i)
                assert np.array_equal(first[i].view(np.int32), second[i].view(np.int32)), (count, rot, i)
    for s, (n, c) in zip(singles, zip(sizes, cfg)):
        assert np.isfinite(s).all() and s[0] > 0


def test_non_finite_elements_give_the_restatements_bits():
    n = 1029
    for where in (0, 5, 1023, 1024, 1028):                      # a vector lane, the partial sweep, the element tail
        for bad in (np.nan, np.inf, -np.inf):
            g = GR.int_grads(n, 400).copy()
            g[where] = bad
            gd = torch.from_numpy(g).to(DEV)
            for max_norm in (1.0, INF, 0.0):
                (out,) = launch([(gd, 1.0, max_norm)])
                want = np.array(GR.norm_coef(g, 1.0, max_norm), dtype=F32)
                assert GR.same_bits(out, want), (where, bad, max_norm, out, want)
    z = torch.zeros(n, device=DEV)
    (out,) = launch([(z, 1.0, 1.0)])
    assert out.tolist() == [0.0, 1.0]                           # the all-zero gradient


def test_ops_wrapper_argument_errors():
    g, out, ws = torch.zeros(8, device=DEV), torch.zeros(2, device=DEV), torch.zeros(WS_N, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.grad_norm_clip([g], [1.0, 1.0], [1.0], [out], ws)
    with pytest.raises(ValueError):
        ops.grad_norm_clip([g] * 5, [1.0] * 5, [1.0] * 5, [out] * 5, ws)
    with pytest.raises(RuntimeError, match="f32"):
        ops.grad_norm_clip([g.double()], [1.0], [1.0], [out], ws)
    with pytest.raises(RuntimeError, match="out"):
        ops.grad_norm_clip([g], [1.0], [1.0], [out[:1]], ws)
    with pytest.raises(RuntimeError, match="ws"):
        ops.grad_norm_clip([g], [1.0], [1.0], [out], ws[:8])
    with pytest.raises(RuntimeError, match="ws"):
        ops.grad_norm_clip([g], [1.0], [1.0], [out], ws.float())
    with pytest.raises(RuntimeError):
        ops.grad_norm_clip([g.cpu()], [1.0], [1.0], [out], ws)
    with pytest.raises(RuntimeError, match="VG_EINVAL"):
        ops.grad_norm_clip([g], [1.0], [-1.0], [out], ws)
    with pytest.raises(RuntimeError, match="VG_EINVAL"):
        ops.grad_norm_clip([g], [INF], [1.0], [out], ws)
    with pytest.raises(RuntimeError, match="VG_EALIGN"):
        ops.grad_norm_clip([torch.zeros(9, device=DEV)[1:]], [1.0], [1.0], [out], ws)


# ---- vg_adam_apply_clip -----------------------------------------------------------------------------------------------
LR = 2e-4
# one element, a tail alone, whole workgroups + tail, more float4 than adam_launch's 2048-workgroup cap covers in one pass
ADAM_SIZES = [1, 5, 1023, 1024 * 256 + 3, 2048 * 256 * 4 + 4 * 256 * 5 + 2]


def optimizer(n, betas, eps, scale, seed):
    """What ops.step_prologue / ops.adam_apply2 / ops.adam_apply_clip read of an optim.Adam (tests/test_gpu_optim.py)."""
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(flat_p=torch.randn(n, generator=g).to(DEV), flat_g=torch.randn(n, generator=g).to(DEV),
                           exp_avg=torch.zeros(n, device=DEV), exp_avg_sq=torch.zeros(n, device=DEV),
                           state_dev=torch.zeros(4, device=DEV), lr=LR, betas=betas, eps=eps, grad_scale=scale)


def clone(o, **kw):
    c = SimpleNamespace(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(o).items()})
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def assert_same(a, b, what):
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: {k}"


def plain_step(o):
    ops.adam_step(o.flat_p, o.flat_g, o.exp_avg, o.exp_avg_sq, o.lr, o.betas[0], o.betas[1], o.eps, o.grad_scale, o.state_dev,
                  prepared=True)


def dev_coef(c):
    """[norm (unused), coef] as vg_grad_norm_clip leaves them; the coefficient is handed over as a view of element 1."""
    return torch.tensor([123.0, c], dtype=torch.float32, device=DEV)[1:]


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_clipped_apply_of_one_buffer_equals_the_unclipped_launch_fed_the_product(n):
    for scale, c in ((1.0, 0.3), (1.0 / 3.0, 0.7), (0.25, 1.0)):
        a = optimizer(n, (0.5, 0.999), 1e-8, scale, n % 1000 + 3)
        ref = clone(a, grad_scale=float(GR.clip_scale(scale, c)))       # the parent's kernel with the host-side product
        null = clone(a)
        g0 = a.flat_g.clone()
        for it in range(2):
            for o in (a, ref, null):
                ops.step_prologue(None, [o])
            n0 = ops.launch_count()
            ops.adam_apply_clip([a], [dev_coef(c)])
            assert ops.launch_count() - n0 == 1
            plain_step(ref)
            ops.adam_apply_clip([null], [None])
            assert_same(a, ref, f"n={n} scale={scale} c={c} step {it + 1}")
        plain = clone(optimizer(n, (0.5, 0.999), 1e-8, scale, n % 1000 + 3))
        for it in range(2):
            ops.step_prologue(None, [plain])
            plain_step(plain)
        assert_same(null, plain, f"n={n}: a NULL coefficient is the unclipped launch")
        if c == 1.0:
            assert_same(a, plain, f"n={n}: coefficient 1 is the unclipped launch")
        else:
            assert not torch.equal(a.exp_avg, plain.exp_avg)    # (p alone does not show it: Adam's first steps are +- lr)
        assert torch.equal(a.flat_g, g0), "the gradient is read only"


@pytest.mark.parametrize("na,nb", [(5, 1023), (1024 * 256 + 3, 7), (2048 * 256 * 4 + 6, 1024 * 256 + 1), (1, 1)])
def test_clipped_apply_of_two_buffers_equals_adam_apply2_fed_the_products(na, nb):
    """The boundary between the two grids, each tail, the grid-stride loop of the first; the buffers differ in betas, eps,
    grad_scale and coefficient, so taking a setting from the wrong one shows."""
    for ca, cb in ((0.3, 0.9), (None, 0.5), (0.125, None), (1.0, 1.0)):
        a = optimizer(na, (0.5, 0.999), 1e-8, 0.25, 5)
        b = optimizer(nb, (0.9, 0.99), 1e-6, 1.0 / 3.0, 6)
        a2 = clone(a, grad_scale=float(GR.clip_scale(a.grad_scale, ca)))
        b2 = clone(b, grad_scale=float(GR.clip_scale(b.grad_scale, cb)))
        for it in range(2):
            ops.step_prologue(None, [a, b])
            n0 = ops.launch_count()
            ops.adam_apply_clip([a, b], [None if c is None else dev_coef(c) for c in (ca, cb)])
            assert ops.launch_count() - n0 == 1
            ops.step_prologue(None, [a2, b2])
            ops.adam_apply2(a2, b2)
            assert_same(a, a2, f"first buffer, coefs {ca} {cb}, step {it + 1}")
            assert_same(b, b2, f"second buffer, coefs {ca} {cb}, step {it + 1}")
        assert float(a.state_dev[0]) == 2.0
    with pytest.raises(ValueError):
        ops.adam_apply_clip([a, b, a], [None] * 3)
    with pytest.raises(ValueError):
        ops.adam_apply_clip([a], [None, None])
    with pytest.raises(RuntimeError, match="f32"):
        ops.adam_apply_clip([a], [torch.ones(1, dtype=torch.float64, device=DEV)])


@pytest.mark.parametrize("n", [5, 1023, 1024 * 256 + 3])
def test_reduction_and_clipped_step_against_torch_clip_grad_norm_and_torch_adam(n):
    """vg_grad_norm_clip + vg_adam_apply_clip against torch.optim.Adam (f32, CPU) fed the gradients that
    torch.nn.utils.clip_grad_norm_ (f32, CPU) clipped: the tolerances of tests/test_gpu_optim._compare (rtol 2e-6, atol 1e-8 /
    1e-9 / 1e-12 for p / exp_avg / exp_avg_sq), taken from there.  Those bounds were set for two sides that are handed the
    SAME gradient; a coefficient that differs in its last bit (torch reduces in f32, the kernel in f64) moves every clipped
    gradient by 6e-8 relative, which the 1e-9 absolute floor of exp_avg does not admit where the moments cancel.  The gradients
    are therefore tests/_gradclip_ref.pow2_norm_grads: their norm is a power of two in both reductions and both coefficients
    are the same power of two -- asserted below, not assumed -- so that what is compared is the clipped step itself."""
    import test_gpu_optim as TO
    gen = torch.Generator().manual_seed(n + 9)
    p0 = torch.randn(n, generator=gen)
    p = torch.nn.Parameter(p0.clone())
    topt = torch.optim.Adam([p], lr=TO.LR, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    o = optimizer(n, (0.9, 0.999), 1e-8, 1.0, 1)
    o.flat_p.copy_(p0)
    o.lr = TO.LR
    out, ws = torch.zeros(2, device=DEV), torch.empty(WS_N, dtype=torch.float64, device=DEV)
    for step in range(TO.STEPS):
        g, norm = GR.pow2_norm_grads(n, 50 + 7 * step + n % 13)
        max_norm = norm / (2.0, 4.0, 2.0, 8.0)[step]
        p.grad = torch.from_numpy(g.copy())
        tn = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
        t_coef = np.unique(p.grad.numpy()[g != 0] / g[g != 0])
        topt.step()
        o.flat_g.copy_(torch.from_numpy(g))
        ops.grad_norm_clip([o.flat_g], [1.0], [max_norm], [out], ws)
        ops.step_prologue(None, [o])
        ops.adam_apply_clip([o], [out[1:]])
        got_norm, coef = out.tolist()
        print(f"n={n} step {step + 1}: norm {got_norm!r} (torch {tn!r}), coefficient {coef!r} (torch {t_coef.tolist()})")
        assert got_norm == tn == norm and t_coef.tolist() == [coef] and coef == max_norm / norm < 1.0
    st = topt.state[p]
    TO._compare((o.flat_p.cpu(), o.exp_avg.cpu(), o.exp_avg_sq.cpu(), float(o.state_dev[0])),
                (p.detach(), st["exp_avg"], st["exp_avg_sq"], float(st["step"])), f"clipped n={n}")


# ---- Adam.clip_grad_norm_ and the step that follows --------------------------------------------------------------------
def small_net(seed=1):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 3)).to(DEV)      # 37*19 + 19 + 57 + 3 parameters
    return net, V.Adam(net.parameters(), lr=1e-2)


def fill_grads(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for p in opt.params:
        p.grad.copy_(torch.randn(p.shape, generator=g))


def test_clip_arms_the_next_step_only_and_leaves_the_gradients_alone():
    (_, a), (_, b), (_, c) = small_net(), small_net(), small_net()
    assert a.clip_dev is None and a.clip_ws is None and not a._clip_armed
    for o in (a, b, c):
        fill_grads(o, 7)
    g0 = a.flat_g.clone()
    n0 = ops.launch_count()
    norm = a.clip_grad_norm_(0.5)
    assert ops.launch_count() - n0 == 2 and a._clip_armed
    assert norm.dim() == 0 and norm.is_cuda and norm.data_ptr() == a.clip_dev.data_ptr()
    want = GR.norm_coef(g0.cpu().numpy(), 1.0, 0.5)
    assert GR.ulp_distance(float(norm), want[0]) <= 1 and GR.ulp_distance(float(a.clip_dev[1]), want[1]) <= 1 and want[1] < 1
    n0 = ops.launch_count()
    a.step()                                                    # unprepared: prologue + clipped apply
    assert ops.launch_count() - n0 == 2 and not a._clip_armed and a.steps == 1
    assert torch.equal(a.flat_g, g0) and all(torch.equal(p.grad.reshape(-1), g0[o:o + p.numel()])
                                             for p, o in zip(a.params, a.offsets))
    b.grad_scale = float(a.clip_dev[1])                         # the twin: an unclipped step at that scale
    b.step()
    c.step()                                                    # ... and the plain step
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert not torch.equal(a.exp_avg, c.exp_avg)
    # a second step without re-arming is unclipped
    b.grad_scale = 1.0
    n0 = ops.launch_count()
    a.step()
    assert ops.launch_count() - n0 == 2
    b.step()
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    # prepared: the clipped apply alone; max_norm = inf: coefficient 1, the unclipped step's bits
    for o in (a, b):
        fill_grads(o, 8)
    ops.step_prologue(None, [a, b])
    a.clip_grad_norm_(INF)
    n0 = ops.launch_count()
    a.step(prepared=True)
    assert ops.launch_count() - n0 == 1 and float(a.clip_dev[1]) == 1.0
    b.step(prepared=True)
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_module_function_clips_each_optimizer_to_its_own_norm_in_one_call_and_step_pair_applies_it():
    (_, a), (_, b) = small_net(1), small_net(2)
    (_, a2), (_, b2) = small_net(1), small_net(2)
    for o, s in ((a, 11), (b, 12), (a2, 11), (b2, 12)):
        fill_grads(o, s)
    ops.step_prologue(None, [a, b, a2, b2])
    n0 = ops.launch_count()
    norms = V.clip_grad_norm_([a, b], [0.5, 2.0])
    assert ops.launch_count() - n0 == 2 and len(norms) == 2 and a._clip_armed and b._clip_armed
    for o, m, nv in ((a, 0.5, norms[0]), (b, 2.0, norms[1])):
        want = GR.norm_coef(o.flat_g.cpu().numpy(), 1.0, m)
        assert GR.ulp_distance(float(nv), want[0]) <= 1 and GR.ulp_distance(float(o.clip_dev[1]), want[1]) <= 1
    n0 = ops.launch_count()
    a.step_pair(b)
    assert ops.launch_count() - n0 == 1 and not a._clip_armed and not b._clip_armed
    a2.grad_scale, b2.grad_scale = float(a.clip_dev[1]), float(b.clip_dev[1])
    a2.step_pair(b2)
    for x, y in ((a, a2), (b, b2)):
        for k in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
            assert torch.equal(getattr(x, k), getattr(y, k)), k
    # only one of the pair armed: the other steps unclipped
    for o, s in ((a, 13), (b, 14), (a2, 13), (b2, 14)):
        fill_grads(o, s)
    ops.step_prologue(None, [a, b, a2, b2])
    b.clip_grad_norm_(0.25)
    a.step_pair(b)
    a2.grad_scale, b2.grad_scale = 1.0, float(b.clip_dev[1])
    a2.step_pair(b2)
    for x, y in ((a, a2), (b, b2)):
        for k in ("flat_p", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(x, k), getattr(y, k)), k


# ---- through the trainers ---------------------------------------------------------------------------------------------
S, B = 64, 4


def build(dtype="fp32", lr=2e-4, seed=42, **kw):
    V.configure_seed(seed)
    e = V.Encoder([3, S, S], 100, dtype=dtype)
    g = V.Generator(nz=100, img_size=S, dtype=dtype)
    d = V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init), d.apply(V.weights_init)
    e.to(DEV), g.to(DEV), d.to(DEV)
    tr = V.VAEGANTrainer(e, g, d, *(V.Adam(m.parameters(), lr=lr) for m in (e, g, d)), **kw)
    tr.train()
    return e, g, d, tr


@functools.lru_cache(maxsize=None)
def batch(step):
    return tuple(t.to(DEV) for t in make_inputs(B, S, 7000 + S + step))


def full_state(e, g, d, tr):
    torch.cuda.synchronize()
    out = {}
    for n, m in (("E", e), ("G", g), ("D", d)):
        for k, v in m.state_dict().items():
            out[f"{n}.{k}"] = v.cpu().clone()
    for n, o in (("E", tr.opt_E), ("G", tr.opt_G), ("D", tr.opt_D)):
        for a in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
            out[f"opt_{n}.{a}"] = getattr(o, a).cpu().clone()
        out[f"opt_{n}.steps"] = torch.tensor(o.steps)
    return out


def assert_same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), k


def run(tr_tuple, steps=1, graphed=False):
    """-> (losses per step, launches per step, grad_norms per step, state after the last)."""
    e, g, d, tr = tr_tuple
    losses, launches, norms = [], [], []
    for k in range(steps):
        real, ez, er, ec = batch(k)
        n0 = ops.launch_count()
        out = (tr.train_step_graphed if graphed else tr.train_step)(real, 60, ez, er, ec)
        launches.append(ops.launch_count() - n0)
        losses.append(out.cpu().clone())
        norms.append(None if tr.grad_norms is None else tr.grad_norms.cpu().clone())
    return losses, launches, norms, full_state(e, g, d, tr)


@functools.lru_cache(maxsize=None)
def plain_run(dtype="fp32", d_iters=2):
    """Two eager steps of the trainer built WITHOUT the keyword."""
    return run(build(dtype, d_iters=d_iters), 2)


def test_off_is_the_trainer_without_the_keyword():
    a = plain_run()
    t = build(max_grad_norm=None)
    b = run(t, 2)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert a[1] == b[1], "max_grad_norm=None changed the number of kernel launches"
    assert_same_state(a[3], b[3])
    tr = t[3]
    assert tr.grad_norms is None and all(o.clip_dev is None and o.clip_ws is None for o in (tr.opt_E, tr.opt_G, tr.opt_D))
    assert sorted(tr.loss_dict(epoch=60)) == sorted(list(V.LOSS_NAMES) + ["total"])


@pytest.mark.parametrize("d_iters", [2, 1])
def test_monitor_only_leaves_the_step_alone_and_reports_the_norms(d_iters):
    """max_grad_norm = inf: every coefficient is 1, the state is the plain trainer's bit for bit, at 2 d_iters + 2 more
    launches.  The norms are norm_coef of flat_g read after the step, to the 1-ulp rule of the kernel test (real gradients:
    no bitwise claim).  For the Discriminator that needs d_iters = 1 and elide_dead_grads (the generator-loss pass through D
    otherwise overwrites D's weight gradients after its update); the state comparison runs without the latter."""
    a = plain_run("fp32", d_iters)
    t = build(max_grad_norm=INF, d_iters=d_iters)
    b = run(t, 2)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert_same_state(a[3], b[3])
    assert [y - x for x, y in zip(a[1], b[1])] == [2 * d_iters + 2] * 2, (a[1], b[1])
    tr = t[3]
    gn = b[2][-1].numpy()
    assert gn.shape == (3, 2) and (gn[:, 1] == 1.0).all()
    for i, o in enumerate((tr.opt_E, tr.opt_G)):
        want = GR.norm_coef(o.flat_g.cpu().numpy(), 1.0, INF)[0]
        print(f"d_iters={d_iters} network {'EG'[i]}: reported {gn[i, 0]!r}, restated {want!r}")
        assert GR.ulp_distance(gn[i, 0], want) <= 1
    ld = tr.loss_dict(epoch=60)
    assert ld["grad_norm_E"] == float(gn[0, 0]) and ld["clip_coef_D"] == 1.0
    assert sorted(ld) == sorted(list(V.LOSS_NAMES) + ["total"] + [f"{p}_{k}" for p in ("grad_norm", "clip_coef") for k in "EGD"])
    if d_iters == 1:
        e, g, d, tr = build(max_grad_norm=INF, d_iters=1, elide_dead_grads=True)
        tr.train_step(*batch(0)[:1], 60, *batch(0)[1:])
        got = float(tr.grad_norms[2, 0])
        want = GR.norm_coef(tr.opt_D.flat_g.cpu().numpy(), 1.0, INF)[0]
        print(f"network D: reported {got!r}, restated {want!r}")
        assert GR.ulp_distance(got, want) <= 1


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_clipped_step_equals_the_twin_stepped_at_the_reported_coefficients(dtype):
    """d_iters = 1, a max norm far below every norm: a twin WITHOUT clipping whose three optimizers step with grad_scale = the
    reported coefficients ends in the bit-identical state (s = 1 * coef = coef).  The flat buffers are f32 in every engine
    dtype, so bf16 holds the same."""
    e, g, d, tr = build(dtype, max_grad_norm=1e-2, d_iters=1)
    real, ez, er, ec = batch(0)
    l1 = tr.train_step(real, 60, ez, er, ec).cpu().clone()
    gn = tr.grad_norms.cpu().numpy()
    print(f"{dtype}: norms {gn[:, 0].tolist()}, coefficients {gn[:, 1].tolist()}")
    assert (gn[:, 1] < 1.0).all() and (gn[:, 1] > 0.0).all() and np.isfinite(gn).all(), "the premise: every network is clipped"
    e2, g2, d2, tw = build(dtype, d_iters=1)
    for o, c in zip((tw.opt_E, tw.opt_G, tw.opt_D), gn[:, 1]):
        o.grad_scale = float(c)
    l2 = tw.train_step(real, 60, ez, er, ec).cpu().clone()
    assert torch.equal(l1, l2)
    assert_same_state(full_state(e, g, d, tr), full_state(e2, g2, d2, tw))
    ld = tr.loss_dict()
    assert ld["clip_coef_G"] == float(gn[1, 1]) and ld["grad_norm_D"] == float(gn[2, 0])


ORACLE_MAX = {"E": 7.0, "G": 5.0, "D": 4.0}       # about half of each network's first-step norm (14.5, 11.2, 9.0 / 9.4)


TINY_MAX = 1e-9


def oracle_first_step(max_norm, d_iters=2):
    """The first clipped iteration at S = 64, B = 4, fp32, epoch 60 on the three sides:
    -> (f32 oracle, f64 oracle, their ref_step results, the trainer's modules and its loss_dict)."""
    inp = make_inputs(B, S, 7000 + S)
    o32 = R.RefVAEGAN(img_size=S, seed=42)
    o64 = R.RefVAEGAN(img_size=S, seed=42).double_()
    r32 = GR.ref_step(o32, *inp, 60, max_norm=max_norm, d_iters=d_iters)
    r64 = GR.ref_step(o64, *inp, 60, max_norm=max_norm, d_iters=d_iters)
    e, g, d, tr = build(max_grad_norm=max_norm, d_iters=d_iters)
    got = tr.loss_dict(tr.train_step(inp[0].to(DEV), 60, *(t.to(DEV) for t in inp[1:])), 60)
    return o32, o64, r32, r64, (e, g, d, tr), got


def test_first_clipped_step_losses_and_norms_against_the_f64_oracle_with_torchs_clipping():
    """Every network clipped (the coefficients are asserted to be < 1) against ref_step in f64.
      losses: FIRST_STEP_TOL of tests/test_gpu_parity.py;
      norms: the Encoder's and the Generator's gradients are evaluated after the two Discriminator updates, like g_loss_adv,
        the Discriminator's last one after its first update, like d_loss_2 -- those entries of FIRST_STEP_TOL (5e-4)."""
    from test_gpu_parity import FIRST_STEP_TOL, rel
    _, _, r32, r64, _, got = oracle_first_step(ORACLE_MAX)
    print({k: f"{got[k]:.6g} / {r64[k]:.6g} ({rel(got[k], r64[k]):.1e})" for k in FIRST_STEP_TOL})
    for k in GR.NETS:
        print(f"grad_norm_{k}: hip {got[f'grad_norm_{k}']:.7g}, f64 ref_step {r64[f'grad_norm_{k}']:.7g}, "
              f"f32 ref_step {r32[f'grad_norm_{k}']:.7g}; coefficient {got[f'clip_coef_{k}']:.4g}")
    for k, t in FIRST_STEP_TOL.items():
        assert rel(got[k], r64[k]) <= t, f"{k}: hip {got[k]} ref_step {r64[k]}"
    for k, like in (("E", "g_loss_adv"), ("G", "g_loss_adv"), ("D", "d_loss_2")):
        assert got[f"clip_coef_{k}"] < 1.0 and r64[f"grad_norm_{k}"] > ORACLE_MAX[k], "the premise: every network is clipped"
        assert rel(got[f"grad_norm_{k}"], r64[f"grad_norm_{k}"]) <= FIRST_STEP_TOL[like], k


def test_first_clipped_step_parameters_against_the_f64_oracle_with_torchs_clipping():
    """Every parameter tensor after the step within the rule of tests/test_gpu_featloss.py: max error relative to the tensor's
    max <= max(1e-5, 4 x the CPU-f32 ref_step's own error against the f64 one); the Encoder's conv biases left out as there.

    The max norm is 1e-9 on all three networks, chosen for the conditioning of this comparison and for nothing else: every
    |g * s| is then far below Adam's eps = 1e-8, where the first update lr * gs / (|gs| + eps) is PROPORTIONAL to the clipped
    gradient.  At a max norm of the order of the norms the update is lr * sign(g): a zero-initialised tensor (the BatchNorm
    biases) then holds nothing but +- lr, its maximum is lr, and an element whose true gradient is rounding noise differs by
    2 lr -- twice the tensor's scale -- between ANY two f32 implementations, which is what tests/test_gpu_featloss.py says of
    the parameters at lr > 0 and why it compares gradients at lr = 0 (the next test does that at moderate max norms).
    Measured at max norms of half the norms: G.main.7.bias 1.99 against a CPU-f32 error of 3.3e-3, two of D's biases 2e-4 and
    6e-4, every other tensor inside the bound.
    d_iters = 1, for the same reason: a second Discriminator gradient is taken at weights that differ in their last bits
    between any two f32 implementations, and a pre-activation that sits at LeakyReLU's kink then moves single elements of a
    BatchNorm bias gradient by a whole term of their 64-term sum (measured at d_iters = 2: one element of D.main.9.bias, 1e-2
    of the tensor's max, every other tensor inside the bound; the first gradient is inside it everywhere)."""
    o32, o64, _, r64, (e, g, d, tr), got = oracle_first_step(TINY_MAX, d_iters=1)
    assert all(got[f"clip_coef_{k}"] < 1e-9 and r64[f"grad_norm_{k}"] > 1.0 for k in GR.NETS)
    worst, lines = 0.0, []
    for name, m, st32, st64 in (("E", e, o32.E, o64.E), ("G", g, o32.G, o64.G), ("D", d, o32.D, o64.D)):
        sd = m.state_dict()
        for k in R.trainable_keys(st64):
            if k.endswith("conv.bias") and m is e:
                continue                    # exactly-zero true gradient in front of BatchNorm: rounding noise everywhere
            p64, p32 = st64[k].detach().double(), st32[k].detach().double()
            hip = sd[k].double().cpu().reshape(p64.shape)
            scale = float(p64.abs().max())
            err_hip, err_cpu = float((hip - p64).abs().max()) / scale, float((p32 - p64).abs().max()) / scale
            bound = max(1e-5, 4 * err_cpu)
            worst = max(worst, err_hip / bound)
            lines.append((err_hip <= bound, f"{name}.{k}: hip err {err_hip:.2e}, cpu-fp32 err {err_cpu:.2e}"))
    print(f"{len(lines)} tensors, worst parameter error / bound {worst:.3f}")
    for ok, line in lines:
        if not ok:
            print("outside:", line)
    assert all(ok for ok, _ in lines), [line for ok, line in lines if not ok]


def test_clipped_gradients_against_the_f64_oracle_with_lr_zero():
    """The same rule where it is well conditioned, as tests/test_gpu_featloss.py applies it: lr = 0 on every side (no
    network moves, so no +- lr differences enter), d_iters = 1, and the quantity compared is the CLIPPED gradient each Adam
    step was handed: exp_avg / (1 - beta1) after the first step, on the device and in the oracle (whose p.grad of the
    Discriminator goes on accumulating in the generator-loss pass).  Per tensor: max error relative to the tensor's max <= max(1e-5, 4 x the CPU-f32 oracle's own error)."""
    inp = make_inputs(B, S, 7000 + S)
    o32 = R.RefVAEGAN(img_size=S, seed=42, lr=0.0)
    o64 = R.RefVAEGAN(img_size=S, seed=42, lr=0.0).double_()
    for o in (o32, o64):
        GR.ref_step(o, *inp, 60, max_norm=ORACLE_MAX, d_iters=1)
    e, g, d, tr = build(lr=0.0, max_grad_norm=ORACLE_MAX, d_iters=1)
    tr.train_step(inp[0].to(DEV), 60, *(t.to(DEV) for t in inp[1:]))
    assert (tr.grad_norms[:, 1] < 1.0).all(), "the premise: every network is clipped"
    worst, outside = 0.0, []
    for name, m, opt, r32o, r64o, st64 in (("E", e, tr.opt_E, o32.opt_E, o64.opt_E, o64.E), ("G", g, tr.opt_G, o32.opt_G, o64.opt_G, o64.G),
                                           ("D", d, tr.opt_D, o32.opt_D, o64.opt_D, o64.D)):
        hsd = opt.state_dict()["state"]
        keys = R.trainable_keys(st64)
        assert len(keys) == len(hsd) == len(r64o.exp_avg) and r64o.t == 1
        for i, k in enumerate(keys):
            if k.endswith("conv.bias") and m is e:
                continue                    # exactly-zero true gradient in front of BatchNorm: rounding noise everywhere
            r64, r32 = (o.exp_avg[i].double() / (1 - o.betas[0]) for o in (r64o, r32o))
            hip = hsd[i]["exp_avg"].double().cpu().reshape(r64.shape) / (1 - opt.betas[0])
            scale = float(r64.abs().max())
            assert scale > 0, k
            err_hip, err_cpu = float((hip - r64).abs().max()) / scale, float((r32 - r64).abs().max()) / scale
            worst = max(worst, err_hip / max(1e-5, 4 * err_cpu))
            if err_hip > max(1e-5, 4 * err_cpu):
                outside.append(f"{name}.{k}: hip err {err_hip:.2e}, cpu-fp32 err {err_cpu:.2e}")
    print("outside:", outside)
    assert not outside, outside
    print(f"worst clipped-gradient error / bound {worst:.3f}")


def test_graphed_equals_eager_including_the_norms_and_recaptures_on_change():
    te, tg = build(max_grad_norm=1e-2), build(max_grad_norm=1e-2)
    ea = run(te, 4)
    gr = run(tg, 4, graphed=True)                               # eager warm-up, capture + replay, two replays
    assert tg[3]._graph is not None
    for k in range(4):
        assert torch.equal(ea[0][k], gr[0][k]), k
        assert torch.equal(ea[2][k].view(torch.int32), gr[2][k].view(torch.int32)), k
    assert_same_state(ea[3], gr[3])
    assert (ea[2][3][:, 1] < 1.0).all() and not torch.equal(ea[2][2], ea[2][3])
    # another max norm: the old graph is not replayed
    key = tg[3]._graph.key
    te[3].max_grad_norm = tg[3].max_grad_norm = {"E": 1e-2, "D": 5e-3}
    real, ez, er, ec = batch(4)
    le = te[3].train_step(real, 60, ez, er, ec).cpu()
    lg = tg[3].train_step_graphed(real, 60, ez, er, ec).cpu()
    assert tg[3]._graph is None and torch.equal(le, lg)
    real, ez, er, ec = batch(5)
    le = te[3].train_step(real, 60, ez, er, ec).cpu()
    lg = tg[3].train_step_graphed(real, 60, ez, er, ec).cpu()
    assert tg[3]._graph is not None and tg[3]._graph.key != key and torch.equal(le, lg)
    assert torch.equal(te[3].grad_norms.view(torch.int32), tg[3].grad_norms.view(torch.int32))
    assert_same_state(full_state(*te), full_state(*tg))


def test_dict_form_clips_only_the_named_networks():
    base = plain_run()[1][0]
    for cfg, extra in (({"G": 1e-2}, 2), ({"D": 1e-2}, 4), ({"E": INF, "D": 1e-2}, 6)):
        e, g, d, tr = t = build(max_grad_norm=cfg)
        _, launches, norms, _ = run(t, 1)
        assert launches[0] - base == extra, (cfg, launches, base)
        ld = tr.loss_dict()
        assert sorted(k for k in ld if k.startswith(("grad_norm_", "clip_coef_"))) == \
            sorted(f"{p}_{k}" for p in ("grad_norm", "clip_coef") for k in cfg)
        gn = norms[0].numpy()
        for i, k in enumerate("EGD"):
            assert (gn[i, 0] > 0) == (k in cfg), (cfg, gn)
        for o, k in zip((tr.opt_E, tr.opt_G, tr.opt_D), "EGD"):
            assert (o.clip_dev is not None) == (k in cfg)


# ---- the sibling trainers ---------------------------------------------------------------------------------------------
def sib_inputs(step):
    g = torch.Generator().manual_seed(8100 + step)
    real = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    eps_img = torch.randn(B, 3, S, S, generator=g)
    eps_z = torch.randn(B, 100, generator=g)
    noise = torch.randn(B, 100, 1, 1, generator=g)
    return [t.to(DEV) for t in (real, eps_img, eps_z, noise)]


def build_vae(**kw):
    V.configure_seed(42)
    e, g = V.Encoder([3, S, S], 100).to(DEV), V.Generator(nz=100, img_size=S).to(DEV)
    opt = V.Adam(list(e.parameters()) + list(g.parameters()), lr=1e-3)
    tr = V.VAETrainer(e, g, opt, **kw)
    tr.train()
    return tr, [opt], lambda: tr.train_step(*sib_inputs(0)[:3], epoch=25)


def build_gan(cls, **kw):
    V.configure_seed(42)
    g, d = V.Generator(nz=100, img_size=S), V.Discriminator(img_size=S)
    g.apply(V.weights_init), d.apply(V.weights_init)
    g.to(DEV), d.to(DEV)
    oG, oD = (V.Adam(m.parameters(), lr=2e-4, betas=(0.5, 0.999)) for m in (g, d))
    tr = cls(g, d, oG, oD, **kw)
    tr.train()
    real, _, _, noise = sib_inputs(0)
    if cls is V.WGANTrainer:
        return tr, [oG, oD], lambda: tr.train_step(real, noise.unsqueeze(0).clone(), noise)
    return tr, [oG, oD], lambda: tr.train_step(real, noise)


SIBLINGS = {"vae": (build_vae, {}, 1), "dcgan": (lambda **kw: build_gan(V.DCGANTrainer, **kw), {}, 2),
            "wgan": (lambda **kw: build_gan(V.WGANTrainer, **kw), dict(critic_iters=1), 2)}


@pytest.mark.parametrize("name", list(SIBLINGS))
def test_sibling_trainer_off_means_off_and_a_clipped_step_equals_its_twin(name):
    mk, kw, clip_points = SIBLINGS[name]

    def state(opts):
        torch.cuda.synchronize()
        return [getattr(o, a).clone() for o in opts for a in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev")]

    def stepped(**extra):
        tr, opts, step = mk(**kw, **extra)
        n0 = ops.launch_count()
        losses = step().cpu().clone()
        return tr, opts, losses, ops.launch_count() - n0

    _, o0, l0, n0 = stepped()
    tr1, o1, l1, n1 = stepped(max_grad_norm=None)
    assert torch.equal(l0, l1) and n0 == n1 and tr1.grad_norms is None and all(o.clip_dev is None for o in o1)
    for a, b in zip(state(o0), state(o1)):
        assert torch.equal(a, b)
    trm, om, lm, nm = stepped(max_grad_norm=INF)                # monitor only: the same state, 2 launches per clip point
    assert nm - n0 == 2 * clip_points and torch.equal(l0, lm) and (trm.grad_norms[:, 1] == 1.0).all()
    for a, b in zip(state(o0), state(om)):
        assert torch.equal(a, b)
    trc, oc, lc, nc = stepped(max_grad_norm=1e-4)
    gn = trc.grad_norms.cpu().numpy()
    print(f"{name}: norms {gn[:, 0].tolist()}, coefficients {gn[:, 1].tolist()}")
    assert nc == nm and gn.shape == (len(oc), 2) and (gn[:, 1] < 1.0).all() and (gn[:, 1] > 0.0).all()
    trt, ot, step = mk(**kw)                                    # the twin: unclipped, stepping at the reported coefficients
    for o, c in zip(ot, gn[:, 1]):
        o.grad_scale = float(c)
    lt = step().cpu()
    assert torch.equal(lc, lt)
    for a, b in zip(state(oc), state(ot)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not all(torch.equal(a, b) for a, b in zip(state(o0), state(oc)))
