"""GPU: weight averaging (vg_ema_update, csrc/ema.hip; vaegan_amd.EMA) -- the kernel against the numpy restatement of
tests/_ema_ref.py bit for bit (int32 views, NaN positions matched), and the EMA through the trainers: what it leaves alone,
what the shadows hold, graph replay, evaluation through the shadows, checkpoints."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import _ema_ref as ER
import vaegan_amd as V
from _inputs import make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
F32 = np.float32
GUARD = 64
# (decay, warmup, hand-set state[0] or None for a NULL state): both sides of each warm-up crossing, constant decays, w = 0 / 1
CONFIGS = [(0.999, True, 1), (0.5, True, 7), (0.5, True, 8), (0.999, True, 8989), (0.999, True, 8990), (0.9, False, None),
           (0.9, False, 3), (1.0, False, None), (0.0, False, None)]
SIZES = [1, 3, 4, 5, 1024, 1029, 2097152, 2097152 + 3 * 1024 + 1]     # the last two: exactly at the grid cap, past it + tail


class Guarded:
    """An f32 buffer between two 64-float NaN guards (the buffer itself stays 16-byte aligned: 64 floats = 256 bytes)."""

    def __init__(self, values: np.ndarray):
        n = values.size
        host = np.full(n + 2 * GUARD, np.nan, dtype=F32)
        host[GUARD:GUARD + n] = values
        self.host0 = host
        self.whole = torch.from_numpy(host.copy()).to(DEV)
        self.t = self.whole[GUARD:GUARD + n]

    def check(self, want: np.ndarray):
        got = self.whole.cpu().numpy()
        g0, g1 = got[:GUARD], got[-GUARD:]
        assert np.array_equal(g0.view(np.int32), self.host0[:GUARD].view(np.int32)), "front guard touched"
        assert np.array_equal(g1.view(np.int32), self.host0[-GUARD:].view(np.int32)), "back guard touched"
        return ER.same_bits(got[GUARD:-GUARD].copy(), want)


def dev_state(t):
    return None if t is None else torch.tensor([float(t), 0.5, 0.25, 0.0], dtype=torch.float32, device=DEV)


def launch(bufs):
    """bufs: [(e0, p, decay, warmup, t)] -> ([Guarded ema], [Guarded p]) after ONE launch over all of them."""
    E, P = [Guarded(b[0]) for b in bufs], [Guarded(b[1]) for b in bufs]
    before = ops.launch_count()
    ops.ema_update([e.t for e in E], [p.t for p in P], [dev_state(b[4]) for b in bufs], [b[2] for b in bufs],
                   [b[3] for b in bufs])
    assert ops.launch_count() - before == 1
    torch.cuda.synchronize()
    return E, P


@pytest.mark.parametrize("n", SIZES)
def test_single_buffer_matches_the_restatement_bitwise(n):
    e0, p = ER.inputs(n, 100 + n % 97)
    for decay, warmup, t in CONFIGS:
        ER.check_conditions(e0, p, ER.weight_f32(decay, warmup, t or 0))
        (E,), (P,) = launch([(e0, p, decay, warmup, t)])
        want = ER.step_f32(e0, p, decay, warmup, t or 0)
        assert E.check(want), (n, decay, warmup, t)
        assert P.check(p), "p is read only"
        if decay == 1.0:
            assert np.array_equal(want.view(np.int32), e0.view(np.int32))


def test_several_buffers_in_one_launch_equal_their_single_launches():
    sizes = [5, 1029, 2097152 + 3 * 1024 + 1, 1024]
    cfg = [(0.999, True, 8989), (0.5, True, 7), (0.9, False, None), (0.999, True, 8990)]
    bufs = [ER.inputs(n, 200 + i) + c for i, (n, c) in enumerate(zip(sizes, cfg))]
    singles = [launch([b])[0][0].t.cpu().numpy() for b in bufs]
    for count in (1, 2, 3, 4):
        for rot in range(count):                                # every buffer in every position of the grid
            sel = [bufs[(i + rot) % 4] for i in range(count)]
            E, P = launch(sel)
            for i, (e, p, b) in enumerate(zip(E, P, sel)):
                want = ER.step_f32(b[0], b[1], b[2], b[3], b[4] or 0)
                assert e.check(want), (count, rot, i)
                assert np.array_equal(e.t.cpu().numpy().view(np.int32), singles[(i + rot) % 4].view(np.int32))
                assert p.check(b[1])


def test_non_finite_values_propagate_as_ieee_gives_them():
    n = 1029
    e0, p = ER.inputs(n, 300)
    p[[0, 5, 1027]] = np.nan
    p[[1, 6, 1028]] = np.inf
    p[[2, 7, 1025]] = -np.inf
    e0[[3, 6]] = np.inf                                         # inf - inf -> NaN at 6, finite - inf -> -inf at 3
    e0[[4, 1026]] = np.nan
    for decay, warmup, t in ((0.9, False, None), (1.0, False, None), (0.999, True, 1)):
        (E,), _ = launch([(e0, p, decay, warmup, t)])
        want = ER.step_f32(e0, p, decay, warmup, t or 0)
        assert np.isnan(want[[0, 5, 1027, 4, 1026, 6]]).all()
        assert E.check(want), (decay, warmup, t)


def test_ops_wrapper_argument_errors():
    a, b = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError, match="VG_EINVAL"):
        ops.ema_update([a], [a], [None], [0.9], [False])       # overlap
    with pytest.raises(RuntimeError, match="VG_EINVAL"):
        ops.ema_update([a], [b], [None], [0.9], [True])        # warm-up without a state
    with pytest.raises(RuntimeError, match="VG_EALIGN"):
        ops.ema_update([torch.zeros(9, device=DEV)[1:]], [b], [None], [0.9], [False])
    with pytest.raises(ValueError):
        ops.ema_update([a] * 5, [b] * 5, [None] * 5, [0.9] * 5, [False] * 5)
    with pytest.raises(RuntimeError, match="one size"):
        ops.ema_update([a], [b[:4]], [None], [0.9], [False])


# ---- through the trainers ----------------------------------------------------------------------------------------------
S, B = 64, 4


def build(dtype="fp32", ema=None, seed=42, **kw):
    """tests/test_gpu_parity.build; ema = dict(decay=, warmup=) attaches an EMA over the Encoder and the Generator."""
    V.configure_seed(seed)
    e = V.Encoder([3, S, S], 100, dtype=dtype)
    g = V.Generator(nz=100, img_size=S, dtype=dtype)
    d = V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init), d.apply(V.weights_init)
    e.to(DEV), g.to(DEV), d.to(DEV)
    oe, og, od = (V.Adam(m.parameters(), lr=2e-4) for m in (e, g, d))
    avg = None if ema is None else V.EMA([e, g], [oe, og], **ema)
    tr = V.VAEGANTrainer(e, g, d, oe, og, od, ema=avg, **kw)
    tr.train()
    return e, g, d, tr


@functools.lru_cache(maxsize=None)
def batch(step):
    return tuple(t.to(DEV) for t in make_inputs(B, S, 7000 + S + step))


def opt_state(o):
    return [o.flat_p.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.state_dev.clone()]


def run_steps(tr, steps, graphed=False, first=0):
    """-> per step: losses, launches, the three optimizers' state and, with an EMA, its shadow buffers (clones)."""
    out = []
    for k in range(first, first + steps):
        real, ez, er, ec = batch(k)
        n0 = ops.launch_count()
        losses = (tr.train_step_graphed if graphed else tr.train_step)(real, 60, ez, er, ec)
        rec = dict(launches=ops.launch_count() - n0, losses=losses.clone(),
                   opts=[opt_state(o) for o in (tr.opt_E, tr.opt_G, tr.opt_D)],
                   shadows=None if tr.ema is None else [b.clone() for b in tr.ema.shadow_bufs])
        out.append(rec)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def three_steps(dtype, with_ema):
    e, g, d, tr = build(dtype, ema=dict(decay=0.99, warmup=True) if with_ema else None)
    init = [o.flat_p.clone() for o in (tr.opt_E, tr.opt_G)]
    return tr, init, run_steps(tr, 3)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def restate(init, recs, which, decay, warmup):
    """The restatement applied to the recorded flat_p snapshots and device step counts of optimizer `which` (0: E, 1: G)."""
    e = init.cpu().numpy().copy()
    for r in recs:
        flat_p, _, _, state = r["opts"][which]
        e = ER.step_f32(e, flat_p.cpu().numpy(), decay, warmup, float(state[0]))
    return e


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ema_leaves_the_training_step_alone_and_costs_one_launch(dtype):
    _, _, off = three_steps(dtype, False)
    _, _, on = three_steps(dtype, True)
    for k, (a, b) in enumerate(zip(off, on)):
        assert bits_equal(a["losses"], b["losses"]), k
        for oa, ob in zip(a["opts"], b["opts"]):
            for x, y in zip(oa, ob):
                assert bits_equal(x, y), k
        assert b["launches"] - a["launches"] == 1, (k, a["launches"], b["launches"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_shadow_buffers_equal_the_restatement_over_three_steps(dtype):
    tr, init, recs = three_steps(dtype, True)
    assert [float(r["opts"][0][3][0]) for r in recs] == [1.0, 2.0, 3.0]
    for which, o in enumerate((tr.opt_E, tr.opt_G)):
        want = restate(init[which], recs, which, 0.99, True)
        got = recs[-1]["shadows"][which].cpu().numpy()
        assert ER.same_bits(got, want), which
        assert not np.array_equal(got, recs[-1]["opts"][which][0].cpu().numpy())          # an average, not a copy
        pad = np.ones(o.numel, dtype=bool)
        for p, off in zip(o.params, o.offsets):
            pad[off:off + p.numel()] = False
        assert (got[pad] == 0).all() and (o.flat_p.cpu().numpy()[pad] == 0).all()
    # shadow parameters are views into the shadow buffers at the live offsets, fused pairs back to back
    sh = tr.ema.module(tr.E)
    for (name, pl), (_, ps) in zip(tr.E.named_parameters(), sh.named_parameters()):
        assert ps.data_ptr() - tr.ema.shadow_bufs[0].data_ptr() == pl.data_ptr() - tr.opt_E.flat_p.data_ptr(), name
    assert sh.fc_logvar.weight.data_ptr() == sh.fc_mu.weight.data_ptr() + 4 * sh.fc_mu.weight.numel()


def test_padding_slots_stay_zero():
    """A latent size of 10 gives the two Linear biases 10 elements each in 12-float slots (the networks above have none)."""
    V.configure_seed(42)
    e = V.Encoder([3, S, S], 10).to(DEV)
    opt = V.Adam(e.parameters(), lr=1e-3)
    ema = V.EMA(e, opt, decay=0.9, warmup=True)
    pad = np.ones(opt.numel, dtype=bool)
    for p, off in zip(opt.params, opt.offsets):
        pad[off:off + p.numel()] = False
    assert pad.sum() == 4
    want = opt.flat_p.cpu().numpy().copy()
    g = torch.Generator().manual_seed(3)
    for t in (1, 2):
        with torch.no_grad():
            for p in opt.params:
                p.add_(torch.randn(p.shape, generator=g).to(DEV) * 0.01)
            opt.state_dev[0] = float(t)
        ema.update()
        want = ER.step_f32(want, opt.flat_p.cpu().numpy(), 0.9, True, t)
    got = ema.shadow_bufs[0].cpu().numpy()
    assert ER.same_bits(got, want) and (got[pad] == 0).all() and (opt.flat_p.cpu().numpy()[pad] == 0).all()
    assert not np.array_equal(got, opt.flat_p.cpu().numpy())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graph_replay_keeps_the_shadows_and_evaluates_through_them(dtype):
    cfg = dict(decay=0.99, warmup=True)
    _, _, _, eager = build(dtype, ema=cfg)
    e, g, d, tr = build(dtype, ema=cfg)
    z = torch.randn(B, 100, 1, 1, generator=torch.Generator().manual_seed(5)).to(DEV)
    before = tr.ema.module(g)(z).clone()                        # packs the shadow's operands: they must not survive the replays
    ref = run_steps(eager, 4)
    got = run_steps(tr, 4, graphed=True)                        # warm-up, capture + replay, two replays
    assert tr._graph is not None
    for k in range(4):
        assert bits_equal(ref[k]["losses"], got[k]["losses"]), k
        for x, y in zip(ref[k]["shadows"], got[k]["shadows"]):
            assert bits_equal(x, y), k
        for x, y in zip(ref[k]["opts"], got[k]["opts"]):
            assert bits_equal(x[0], y[0]), k
    # evaluation through the shadow after the replays: equal to a fresh Generator loaded from the shadow's state_dict
    sh = tr.ema.module(g)
    img = sh(z)
    fresh = V.Generator(nz=100, img_size=S, dtype=dtype).to(DEV).eval()
    fresh.load_state_dict(sh.state_dict())
    assert list(sh.state_dict()) == list(g.state_dict())
    assert bits_equal(img, fresh(z))
    assert not bits_equal(img, before)
    g.eval()
    assert not bits_equal(img, g(z))
    # ... and denoise_eval through both shadows
    e.eval()
    real, ez, er, _ = batch(9)
    she = tr.ema.module(e)
    fe = V.Encoder([3, S, S], 100, dtype=dtype).to(DEV).eval()
    fe.load_state_dict(she.state_dict())
    a = V.denoise_eval(she, tr.ema.module(g), real, eps=er, eps_z=ez)
    b = V.denoise_eval(fe, fresh, real, eps=er, eps_z=ez)
    c = V.denoise_eval(e, g, real, eps=er, eps_z=ez)
    assert bits_equal(a["recon"], b["recon"]) and a["ssim"] == b["ssim"] and a["recon_loss"] == b["recon_loss"]
    assert not bits_equal(a["recon"], c["recon"])
    e.train(), g.train()
    # a changed decay re-captures: the next call runs eagerly (warm-up of the new key) with the new decay
    tr.ema.decay = eager.ema.decay = 0.5
    ref5, got5 = run_steps(eager, 1, first=4), run_steps(tr, 1, graphed=True, first=4)
    assert tr._graph is None
    for x, y in zip(ref5[0]["shadows"], got5[0]["shadows"]):
        assert bits_equal(x, y)
    want = ER.step_f32(got[3]["shadows"][1].cpu().numpy(), got5[0]["opts"][1][0].cpu().numpy(), 0.5, True, 5.0)
    assert ER.same_bits(got5[0]["shadows"][1].cpu().numpy(), want)
    got6 = run_steps(tr, 1, graphed=True, first=5)              # captured again, with the new decay inside
    assert tr._graph is not None
    want = ER.step_f32(want, got6[0]["opts"][1][0].cpu().numpy(), 0.5, True, 6.0)
    assert ER.same_bits(got6[0]["shadows"][1].cpu().numpy(), want)


def test_shadow_batchnorm_buffers_are_the_live_ones():
    tr, _, _ = three_steps("fp32", True)
    for live in (tr.E, tr.G):
        sh = tr.ema.module(live)
        lsd, ssd = live.state_dict(), sh.state_dict()
        assert not sh.training and live.training
        bufs = [k for k in lsd if "running_" in k or "num_batches" in k]
        assert bufs
        for k in bufs:
            assert torch.equal(lsd[k], ssd[k]), k
        for (k, bl), (_, bs) in zip(live.named_buffers(), sh.named_buffers()):
            assert bl.data_ptr() == bs.data_ptr(), k
    assert int(tr.ema.module(tr.G).state_dict()["main.1.num_batches_tracked"]) == 3


def test_checkpoint_round_trip_resumes_bit_identically(tmp_path):
    cfg = dict(decay=0.99, warmup=True)
    path = str(tmp_path / "ckpt.pt")
    _, _, _, a = build(ema=cfg)
    ra = run_steps(a, 4)
    _, _, _, b = build(ema=cfg)
    run_steps(b, 2)
    b.save_checkpoint(path, epoch=60)
    rb = run_steps(b, 2, first=2)
    _, _, _, c = build(ema=dict(decay=0.5, warmup=False), seed=7)       # other weights, other EMA settings: all restored
    assert c.load_checkpoint(path) == {"epoch": 60}
    assert c.ema.decay == 0.99 and c.ema.warmup is True
    rc = run_steps(c, 2, first=2)
    for r in (rb, rc):
        for k in (0, 1):
            assert bits_equal(ra[2 + k]["losses"], r[k]["losses"])
            for x, y in zip(ra[2 + k]["shadows"], r[k]["shadows"]):
                assert bits_equal(x, y)
            for oa, ob in zip(ra[2 + k]["opts"], r[k]["opts"]):
                for x, y in zip(oa, ob):
                    assert bits_equal(x, y)
    sd = torch.load(path, weights_only=True)
    assert sd["ema"]["format"] == 1 and sd["ema"]["decay"] == 0.99 and sd["ema"]["warmup"] is True
    assert [list(s) for s in sd["ema"]["shadows"]] == [list(sd["encoder"]), list(sd["decoder"])]
    # a checkpoint without "ema" into a trainer with one: the shadows restart from the loaded live weights
    plain = {k: v for k, v in sd.items() if k != "ema"}
    c.load_state_dict(plain)
    for buf, o in zip(c.ema.shadow_bufs, (c.opt_E, c.opt_G)):
        assert bits_equal(buf, o.flat_p)
    # a checkpoint with "ema" into a trainer without one: ignored; and such a trainer writes none
    _, _, _, n = build()
    n.load_state_dict(sd)
    assert "ema" not in n.state_dict() and bits_equal(n.opt_G.flat_p, c.opt_G.flat_p)


def sib_inputs(step):
    g = torch.Generator().manual_seed(8100 + step)
    real = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    eps_img = torch.randn(B, 3, S, S, generator=g)
    eps_z = torch.randn(B, 100, generator=g)
    noise = torch.randn(B, 100, 1, 1, generator=g)
    return [t.to(DEV) for t in (real, eps_img, eps_z, noise)]


def test_vae_trainer_one_optimizer_holding_both_networks():
    V.configure_seed(42)
    e, g = V.Encoder([3, S, S], 100), V.Generator(nz=100, img_size=S)
    e.to(DEV), g.to(DEV)
    opt = V.Adam(list(e.parameters()) + list(g.parameters()), lr=1e-3)
    ema = V.EMA([e, g], opt, decay=0.9, warmup=False)
    assert len(ema.shadow_bufs) == 1
    tr = V.VAETrainer(e, g, opt, ema=ema)
    tr.train()
    want = opt.flat_p.cpu().numpy().copy()
    for k in range(2):
        real, eps_img, eps_z, _ = sib_inputs(k)
        tr.train_step(real, eps_img, eps_z, epoch=25)
        want = ER.step_f32(want, opt.flat_p.cpu().numpy(), 0.9, False, 0)
    assert float(opt.state_dev[0]) == 2.0
    assert ER.same_bits(ema.shadow_bufs[0].cpu().numpy(), want)
    assert not bits_equal(ema.shadow_bufs[0], opt.flat_p)
    assert ema.module(g).main[0].weight.data_ptr() - ema.shadow_bufs[0].data_ptr() == \
        g.main[0].weight.data_ptr() - opt.flat_p.data_ptr()


@pytest.mark.parametrize("graphed", [False, True])
def test_dcgan_trainer_generator_only(graphed):
    V.configure_seed(42)
    g, d = V.Generator(nz=100, img_size=S), V.Discriminator(img_size=S)
    g.apply(V.weights_init), d.apply(V.weights_init)
    g.to(DEV), d.to(DEV)
    oD = V.Adam(d.parameters(), lr=2e-4, betas=(0.5, 0.999))
    oG = V.Adam(g.parameters(), lr=2e-4, betas=(0.5, 0.999))
    ema = V.EMA(g, oG, decay=0.999, warmup=True)
    tr = V.DCGANTrainer(g, d, oG, oD, ema=ema)
    tr.train()
    want = oG.flat_p.cpu().numpy().copy()
    d0 = oD.flat_p.clone()
    for k in range(3 if graphed else 2):
        real, _, _, noise = sib_inputs(k)
        (tr.step_graphed if graphed else tr.train_step)(real, noise)
        want = ER.step_f32(want, oG.flat_p.cpu().numpy(), 0.999, True, float(oG.state_dev[0]))
    assert float(oG.state_dev[0]) == (3.0 if graphed else 2.0) and not bits_equal(d0, oD.flat_p)
    assert ER.same_bits(ema.shadow_bufs[0].cpu().numpy(), want)
    with pytest.raises(ValueError, match="built over"):
        ema.module(d)


def test_reference_shaped_eager_loop_with_update_after_the_optimizer_step():
    """loss.backward(); opt.step(); ema.update() -- the autograd path, no trainer."""
    V.configure_seed(42)
    g = V.Generator(nz=100, img_size=S)
    g.apply(V.weights_init)
    g.to(DEV)
    opt = V.Adam(g.parameters(), lr=2e-4, betas=(0.5, 0.999))
    ema = V.EMA([g], [opt], decay=0.9)
    g.train()
    want = opt.flat_p.cpu().numpy().copy()
    for k in range(2):
        z = sib_inputs(k)[3]
        opt.zero_grad()
        loss = (g(z) ** 2).mean()
        loss.backward()
        opt.step()
        ema.update()
        want = ER.step_f32(want, opt.flat_p.cpu().numpy(), 0.9, True, float(k + 1))
    assert ER.same_bits(ema.shadow_bufs[0].cpu().numpy(), want)
    sh = ema.module(g)
    fresh = V.Generator(nz=100, img_size=S).to(DEV).eval()
    fresh.load_state_dict(sh.state_dict())
    z = sib_inputs(3)[3]
    with torch.no_grad():
        assert bits_equal(sh(z), fresh(z))
