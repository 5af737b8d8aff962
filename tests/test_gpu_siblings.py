"""GPU: the reference's sibling training loops (plain VAE main_vae.py:103-127, DCGAN gan_code.py:194-219,
weight-clipped WGAN gan_code.py:296-331) on the HIP kernel chains, against
  (a) golden vectors captured from the reference's own classes at S=256 (tests/golden/sibling_*.npz, made by
      oracle/gen_golden_siblings.py, where oracle/siblings_ref.py reproduced every vector bit for bit), and
  (b) the CPU oracle run live on the same seeded inputs at S=64.
Tolerances as in test_gpu_parity.py: quantities that are pure forward passes of the initial weights are held to
1e-4; quantities evaluated after in-iteration Adam(t=1) updates (sign(g)*lr per weight) to 5e-4; second-iteration
losses are a sanity bound (the trajectory is chaotic in the reference itself)."""
import os

import numpy as np
import pytest
import torch

import siblings_ref as SR
import vaegan_amd as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
torch.set_num_threads(min(16, os.cpu_count() or 1))


def sib_inputs(B, S, step, critic_iters=5, nz=100):
    """Same recipe as oracle/gen_golden_siblings.py:sib_inputs."""
    g = torch.Generator().manual_seed(8100 + step)
    real = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    eps_img = torch.randn(B, 3, S, S, generator=g)
    eps_z = torch.randn(B, nz, generator=g)
    noises = [torch.randn(B, nz, 1, 1, generator=g) for _ in range(critic_iters + 1)]
    return real, eps_img, eps_z, noises


def build_vae(S, dtype="fp32"):
    V.configure_seed(42)
    e = V.Encoder([3, S, S], 100, dtype=dtype)
    g = V.Generator(nz=100, img_size=S, dtype=dtype)            # main_vae.py:83: default init, no weights_init
    e.to(DEV), g.to(DEV)
    opt = V.Adam(list(e.parameters()) + list(g.parameters()), lr=1e-3)
    tr = V.VAETrainer(e, g, opt)
    tr.train()
    return e, g, tr


def build_gan(S, cls, dtype="fp32", **kw):
    V.configure_seed(42)
    g = V.Generator(nz=100, img_size=S, dtype=dtype)
    d = V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init), d.apply(V.weights_init)
    g.to(DEV), d.to(DEV)
    oD = V.Adam(d.parameters(), lr=2e-4, betas=(0.5, 0.999))
    oG = V.Adam(g.parameters(), lr=2e-4, betas=(0.5, 0.999))
    tr = cls(g, d, oG, oD, **kw)
    tr.train()
    return g, d, tr


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def run_vae(tr, B, S, steps=((25, 0), (60, 1))):
    out = []
    for epoch, step in steps:
        img, eps_img, eps_z, _ = sib_inputs(B, S, step)
        out.append(tr.train_step(img.to(DEV), eps_img.to(DEV), eps_z.to(DEV), epoch=epoch)[:3].tolist())
    return np.array(out)


def run_dcgan(tr, B, S, steps=2):
    out = []
    for step in range(steps):
        real, _, _, noises = sib_inputs(B, S, step)
        out.append(tr.train_step(real.to(DEV), noises[0].to(DEV))[:3].tolist())
    return np.array(out)


def run_wgan(tr, B, S, steps=2):
    out = []
    for step in range(steps):
        real, _, _, noises = sib_inputs(B, S, step)
        out.append(tr.train_step(real.to(DEV), torch.stack(noises[:5]).to(DEV), noises[5].to(DEV))[:2].tolist())
    return np.array(out)


def check_vae(got, ref):
    for i, n in enumerate(("recon_loss", "kl_loss", "total")):
        assert rel(got[0, i], ref[0, i]) <= 1e-4, f"VAE step 1 {n}: hip {got[0, i]} ref {ref[0, i]}"
        # after one Adam(lr 1e-3, t=1) sign-update of EVERY weight; kl jumps 24 -> 1.5e5 in the reference itself
        assert rel(got[1, i], ref[1, i]) <= 5e-2, f"VAE step 2 {n}: hip {got[1, i]} ref {ref[1, i]}"


def check_dcgan(got, ref):
    for i, (n, tol) in enumerate((("errD_real", 1e-4), ("errD_fake", 1e-4), ("errG", 5e-4))):
        assert rel(got[0, i], ref[0, i]) <= tol, f"DCGAN step 1 {n}: hip {got[0, i]} ref {ref[0, i]}"
        assert rel(got[1, i], ref[1, i]) <= 0.5, f"DCGAN step 2 {n}: hip {got[1, i]} ref {ref[1, i]}"


def check_wgan(got, ref):
    # the clamp to +-0.01 pins the critic's output near 0.5: d_loss = mean(p_fake) - mean(p_real) ~ -2e-3 is a
    # difference of two means ~0.5 -> absolute bounds; both follow 4-5 Adam updates of the critic
    for s in range(2):
        assert abs(got[s, 0] - ref[s, 0]) <= 5e-5 * (1 + 9 * s), f"WGAN step {s + 1} d_loss: hip {got[s, 0]} ref {ref[s, 0]}"
        assert abs(got[s, 1] - ref[s, 1]) <= 5e-5 * (1 + 9 * s), f"WGAN step {s + 1} g_loss: hip {got[s, 1]} ref {ref[s, 1]}"


# ---- (a) reference-pinned golden vectors, S=256 ---------------------------------------------------------------
def test_vae_two_steps_vs_reference_golden_S256(golden_dir):
    gold = np.load(os.path.join(golden_dir, "sibling_vae_S256_B2.npz"))
    e, g, tr = build_vae(256)
    check_vae(run_vae(tr, 2, 256), gold["losses"])
    assert tr.opt.steps == int(gold["final.adam.EG.step"][0]) == 2
    # Adam(t<=2) moves every weight by ~lr per step whatever the gradient's size: compare the second moments'
    # checksum (sum of g^2-weighted averages), which is dominated by the large, well-conditioned gradients
    s2 = float(tr.opt.exp_avg_sq.double().sum())
    assert rel(s2, float(gold["final.adam.EG.exp_avg_sq#stats"][0])) <= 5e-2


def test_dcgan_two_steps_vs_reference_golden_S256(golden_dir):
    gold = np.load(os.path.join(golden_dir, "sibling_dcgan_S256_B2.npz"))
    g, d, tr = build_gan(256, V.DCGANTrainer)
    check_dcgan(run_dcgan(tr, 2, 256), gold["losses"])
    assert tr.opt_D.steps == int(gold["final.adam.D.step"][0]) == 2 and tr.opt_G.steps == 2
    assert int(d.state_dict()["main.3.num_batches_tracked"]) == 6          # 3 D forwards per iteration


def test_wgan_two_steps_vs_reference_golden_S256(golden_dir):
    gold = np.load(os.path.join(golden_dir, "sibling_wgan_S256_B2.npz"))
    g, d, tr = build_gan(256, V.WGANTrainer)
    check_wgan(run_wgan(tr, 2, 256), gold["losses"])
    assert tr.opt_D.steps == int(gold["final.adam.D.step"][0]) == 10 and tr.opt_G.steps == 2
    assert float(tr.opt_D.flat_p.abs().max()) <= 0.01                       # the clamp of gan_code.py:320-321
    assert int(g.state_dict()["main.1.num_batches_tracked"]) == 12         # 5 critic-side + 1 generator forward


# ---- (b) live oracle, S=64 -------------------------------------------------------------------------------------
def test_vae_vs_live_oracle_S64():
    B, S = 8, 64
    o = SR.RefVAE(img_size=S, seed=42)
    ref = []
    for epoch, step in ((25, 0), (60, 1)):
        img, eps_img, eps_z, _ = sib_inputs(B, S, step)
        lo = o.train_step(img, eps_img, eps_z, epoch)
        ref.append([lo[n] for n in ("recon_loss", "kl_loss", "total")])
    e, g, tr = build_vae(S)
    check_vae(run_vae(tr, B, S), np.array(ref))


def test_dcgan_vs_live_oracle_S64():
    B, S = 8, 64
    o = SR.RefDCGAN(img_size=S, seed=42)
    ref = []
    for step in range(2):
        real, _, _, noises = sib_inputs(B, S, step)
        lo = o.train_step(real, noises[0])
        ref.append([lo[n] for n in ("errD_real", "errD_fake", "errG")])
    g, d, tr = build_gan(S, V.DCGANTrainer)
    check_dcgan(run_dcgan(tr, B, S), np.array(ref))


def test_wgan_vs_live_oracle_S64():
    B, S = 8, 64
    o = SR.RefWGAN(img_size=S, seed=42)
    ref = []
    for step in range(2):
        real, _, _, noises = sib_inputs(B, S, step)
        lo = o.train_step(real, noises[:5], noises[5])
        ref.append([lo["d_loss"], lo["g_loss"]])
    g, d, tr = build_gan(S, V.WGANTrainer)
    check_wgan(run_wgan(tr, B, S), np.array(ref))


# ---- engine properties ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["vae", "dcgan", "wgan"])
def test_sibling_graph_replay_is_bitwise_identical_to_eager(which):
    B, S, steps = 8, 64, 4
    res = []
    for graphed in (False, True):
        if which == "vae":
            e, g, tr = build_vae(S)
            nets = (e, g)
        else:
            g, d, tr = build_gan(S, V.DCGANTrainer if which == "dcgan" else V.WGANTrainer)
            nets = (g, d)
        outs = []
        for step in range(steps):
            real, eps_img, eps_z, noises = (sib_inputs(B, S, step))
            if which == "vae":
                args, kw = (real.to(DEV), eps_img.to(DEV), eps_z.to(DEV)), {"epoch": 60}
            elif which == "dcgan":
                args, kw = (real.to(DEV), noises[0].to(DEV)), {}
            else:
                args, kw = (real.to(DEV), torch.stack(noises[:5]).to(DEV), noises[5].to(DEV)), {}
            fn = tr.step_graphed if graphed else tr.train_step
            outs.append(fn(*args, **kw).clone())
        torch.cuda.synchronize()
        res.append((torch.stack(outs).cpu(), [{k: v.cpu() for k, v in n.state_dict().items()} for n in nets]))
    assert torch.equal(res[0][0], res[1][0])
    for sa, sb in zip(res[0][1], res[1][1]):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k


def test_grouped_and_separate_critic_passes_agree():
    """One grouped 2B-row critic pass (per-group BatchNorm statistics, one wgrad over 2B rows) vs the reference's
    two calls with accumulating gradients: same values up to the fp32 summation order of the weight gradients."""
    B, S = 8, 64
    outs = []
    for grouped in (True, False):
        g, d, tr = build_gan(S, V.WGANTrainer, group_d_passes=grouped)
        assert d._engine.can_group(B, 2, torch.empty(1, device=DEV)) is True
        outs.append((run_wgan(tr, B, S, steps=1), tr.opt_D.exp_avg.cpu().clone(),
                     {k: v.cpu().clone() for k, v in d.state_dict().items() if "running" in k}))
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=2e-6)
    a, b = outs[0][1], outs[1][1]                                 # Adam first moments: a running mean of the gradients
    assert float((a - b).abs().max() / b.abs().max()) < 2e-3
    for k, v in outs[0][2].items():
        torch.testing.assert_close(v, outs[1][2][k], rtol=1e-4, atol=1e-6, msg=k)


def test_bf16_siblings_track_fp32_oracle():
    """bf16 storage / f32 accumulate: first-iteration losses within 3e-2 of the fp32 oracle (stated bf16 bound)."""
    B, S = 16, 64
    img, eps_img, eps_z, noises = sib_inputs(B, S, 0)
    lo = SR.RefVAE(img_size=S, seed=42).train_step(img, eps_img, eps_z, 25)
    e, g, tr = build_vae(S, dtype="bf16")
    got = tr.train_step(img.to(DEV), eps_img.to(DEV), eps_z.to(DEV), epoch=25).tolist()
    for i, n in enumerate(("recon_loss", "kl_loss", "total")):
        assert rel(got[i], lo[n]) <= 3e-2, (n, got[i], lo[n])
    lo = SR.RefDCGAN(img_size=S, seed=42).train_step(img, noises[0])
    g, d, tr = build_gan(S, V.DCGANTrainer, dtype="bf16")
    got = tr.train_step(img.to(DEV), noises[0].to(DEV)).tolist()
    for i, n in enumerate(("errD_real", "errD_fake", "errG")):
        assert rel(got[i], lo[n]) <= 3e-2, (n, got[i], lo[n])


def test_sibling_graph_is_recaptured_after_a_reseed():
    """round-2 ADVICE: the captured vg_rng_advance / vg_randn launches hold the raw pointer of the default noise stream's
    state; utils.configure_seed() drops that stream (ops.reset_noise).  The replay after a reseed must neither write
    into the freed buffer nor ignore the new seed: the state's address is part of the capture key and the trainer keeps
    the stream it captured alive.  Device-drawn noise, graphed == eager bit for bit across the reseed."""
    B, S = 8, 64
    res = []
    for graphed in (False, True):
        e, g, tr = build_vae(S)
        img = sib_inputs(B, S, 0)[0].to(DEV)
        fn = tr.step_graphed if graphed else tr.train_step
        seq = [fn(img, None, None, epoch=60).clone() for _ in range(3)]
        if graphed:
            assert tr._gstate is not None
            old_graph, old_ptr = tr._gstate.graphs[0], tr._gstate.key[-1]
        V.configure_seed(7)                                   # new device seed: the default stream is dropped
        seq += [fn(img, None, None, epoch=60).clone() for _ in range(3)]
        if graphed:
            assert tr._gstate.graphs[0] is not old_graph and tr._gstate.key[-1] != old_ptr, "reseed must re-capture"
        torch.cuda.synchronize()
        res.append(torch.stack(seq).cpu())
    assert torch.equal(res[0], res[1])
    assert not torch.equal(res[0][2], res[0][3])


def test_failed_sibling_capture_leaves_the_trainer_where_it_was(monkeypatch):
    """A sibling trainer's capture that dies half-way (here: the critic's third Adam step raises while the stream is
    capturing, after two steps and their BatchNorm forwards have moved the host counters) has executed nothing: no stream
    is left capturing, optimizer step counts and BatchNorm ticks are what they were, the next graphed call warms up again,
    and the remaining iterations -- eager, warm-up, capture, replay -- give bit for bit what an undisturbed run gives."""
    from importlib import import_module
    ops = import_module("vae-gan-based-model-for-image-generation-and-denoising_amd.ops")
    B, S = 8, 64
    res = []
    for disturb in (False, True):
        g, d, tr = build_gan(S, V.WGANTrainer)
        batches = []
        for step in range(5):
            real, _, _, noises = sib_inputs(B, S, step)
            batches.append((real.to(DEV), torch.stack(noises[:5]).to(DEV), noises[5].to(DEV)))
        outs = [tr.step_graphed(*batches[0]).clone()]                              # eager warm-up call
        if disturb:
            real_adam, calls = ops.adam_step, [0]

            def failing_adam(*a, **k):
                if torch.cuda.is_current_stream_capturing():
                    calls[0] += 1
                    if calls[0] == 3:
                        raise RuntimeError("injected failure during capture")
                return real_adam(*a, **k)

            monkeypatch.setattr(ops, "adam_step", failing_adam)
            steps_before = (tr.opt_G.steps, tr.opt_D.steps)
            ticks_before = [n._engine.pending_bn_ticks for n in (g, d)]
            with pytest.raises(RuntimeError, match="injected failure"):
                tr.step_graphed(*batches[1])
            monkeypatch.setattr(ops, "adam_step", real_adam)
            assert calls[0] == 3 and not torch.cuda.is_current_stream_capturing()
            assert (tr.opt_G.steps, tr.opt_D.steps) == steps_before
            assert [n._engine.pending_bn_ticks for n in (g, d)] == ticks_before
            assert tr._gstate is None and tr._gwarm is None
            torch.cuda.synchronize()                                               # the device is usable
            outs.append(tr.train_step(*batches[1]).clone())                        # the iteration that failed, eagerly
            for b in batches[2:]:
                outs.append(tr.step_graphed(*b).clone())                           # warm-up again, capture, replay
            assert tr._gstate is not None
        else:
            for b in batches[1:]:
                outs.append(tr.step_graphed(*b).clone())
        torch.cuda.synchronize()
        res.append((torch.stack(outs).cpu(), tr.opt_G.flat_p.cpu().clone(), tr.opt_D.flat_p.cpu().clone(),
                    [{k: v.cpu() for k, v in n.state_dict().items()} for n in (g, d)],
                    (tr.opt_G.steps, tr.opt_D.steps, float(tr.opt_D.state_dev[0]))))
    for a, b in zip(res[0][:3], res[1][:3]):
        assert torch.equal(a, b)
    for sa, sb in zip(res[0][3], res[1][3]):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    assert res[0][4] == res[1][4] == (5, 25, 25.0)
