"""The reference's three sibling training loops on the same HIP kernel chains as the VAE-GAN path
(SURVEY.md section 8(f), row F4):

  VAETrainer    main_vae.py:103-127   plain (denoising) VAE: ONE Adam over encoder + decoder, lr 1e-3
  DCGANTrainer  gan_code.py:194-219   DCGAN: BCE against hard labels 1 / 0, Adam betas (0.5, 0.999)
  WGANTrainer   gan_code.py:296-331   weight-clipped WGAN: 5 critic iterations per generator step

Same conventions as trainer.VAEGANTrainer: direct kernel chains (no autograd graph), gradients land in the
optimizers' flat buffers, every random draw of the reference loop can be injected (parity runs) or is drawn on the
device, losses come back as one device tensor (no host sync), ``step_graphed`` replays the whole iteration from a
captured hipGraph.  There is no CPU path.
"""
import math
from typing import List, Optional, Sequence

import torch

from . import augment as A
from . import geometry as G
from . import ops
from .capture import HostMirrors, capture, replay
from .engine import GradSink, bump_weights_epoch
from .gradclip import ClipOption
from .losses import trainer_scales
from .optim import lr_report


class _Graphed(ClipOption):
    """Whole-iteration hipGraph replay for a trainer whose ``train_step(*tensors, **scalars)`` takes device tensors
    (static shapes) and plain scalars.  First call with a new signature runs eagerly (it also sizes the
    workspaces), the second captures and replays, later calls replay; every call is exactly one iteration."""

    _nets: Sequence = ()
    _opts: Sequence = ()
    # ema.EMA over the generating networks, or None: train_step then ends with ema.update(), one
    # launch directly after the (Encoder /) Generator optimizer step; None launches exactly what it launched without it
    ema = None
    # max_grad_norm (gradclip.ClipOption): every optimizer's gradient is clipped to its own global L2
    # norm directly before its step(), two launches per step, the coefficient applied inside the Adam launch; a number, a
    # dict over the trainer's network names, inf (monitor only) or None (the default: nothing launched, nothing allocated).
    # grad_norms: [networks, 2] device tensor, [norm, coefficient] of each network's last update.

    def step_graphed(self, *tensors, **scalars):
        return self._graphed_call(self.train_step, tensors, scalars)

    def _extra_key(self):
        """Whatever else a subclass's captured iteration freezes."""
        return ()

    def lr_dict(self):
        """{"lr_<network>": the learning rate of the optimizer's last step} when any optimizer has an optim.LRSchedule, {}
        otherwise; from the host's step counts (no device read).  Network names as in max_grad_norm."""
        return lr_report(self._clip_opts())

    def _graphed_call(self, step, tensors, scalars, tag=None):
        """step(*tensors, **scalars) eagerly, then captured, then replayed; tag: whatever else the capture freezes."""
        # Draws that are not injected come from the per-device default NoiseStream, whose STATE BUFFER the captured
        # vg_rng_advance / vg_randn launches point at.  utils.configure_seed() (ops.reset_noise) drops that stream: the
        # graph must then be re-captured against the new one -- the buffer's address is part of the key, and the
        # trainer holds a reference to the stream it captured so the old buffer cannot be recycled under a replay.
        noise = None
        if any(t is None for t in tensors):
            dev = next(t for t in tensors if t is not None).device
            noise = ops.default_noise(dev)
        key = (tuple(None if t is None else tuple(t.shape) for t in tensors), tuple(sorted(scalars.items())),
               tuple(n.training for n in self._nets), tuple(o.capture_key() for o in self._opts),
               None if noise is None else noise.state.data_ptr()) \
            + (() if tag is None else (tag,)) + (() if self.ema is None else (("ema",) + self.ema.key(),)) \
            + self._clip_key() + self._extra_key()
        self._gnoise = noise
        st = getattr(self, "_gstate", None)
        if st is not None and st.key == key:
            for s, t in zip(st.sin, tensors):
                if s is not None:
                    s.copy_(t)
            replay(st)
            if self.ema is not None:
                self.ema.touch()                       # the replayed update rewrote the shadow buffers
            return st.out
        if getattr(self, "_gwarm", None) != key:
            self._gwarm, self._gstate = key, None
            return step(*tensors, **scalars)
        sin = [None if t is None else t.clone() for t in tensors]      # None: drawn on the device inside the graph
        try:
            # thread_local: see capture.capture (the c10d watchdog may poll events); keep: the captured state buffer
            st = self._gstate = capture(lambda *s: step(*s, **scalars), sin,
                                        HostMirrors([n._engine for n in self._nets], self._opts), sin[0].device,
                                        key=key, error_mode="thread_local", keep=noise)
        except BaseException:
            self._gwarm = self._gstate = None          # nothing ran: the next call warms up again
            raise
        replay(st)
        if self.ema is not None:
            self.ema.touch()
        return st.out


def _need_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what} needs the batch on the MI355X ('cuda'); there is no CPU path")


def _same_dtype(*nets) -> int:
    dts = {n._dt for n in nets}
    if len(dts) != 1:
        raise ValueError("the networks must share one engine dtype")
    return dts.pop()


# ---------------------------------------------------------------------------------------------------------------
class VAETrainer(_Graphed):
    """train_vae's loop body (main_vae.py:103-127).  ``optimizer`` is ONE Adam over
    ``list(encoder.parameters()) + list(decoder.parameters())`` (main_vae.py:84-87)."""
    LOSS_NAMES = ("recon_loss", "kl_loss", "total")

    def __init__(self, encoder, decoder, optimizer, noise_max_std: float = 0.5, kl_weight: float = 1e-5,
                 alpha_ssim: float = 0.0, hole_weight: float = 1.0, ema=None, max_grad_norm=None, ssim_scales=None):
        """max_grad_norm: the one optimizer holds both networks, so its one norm is the network "EG" (a number, or
        {"EG": number}); reported in grad_norms[0]."""
        self.E, self.G, self.opt = encoder, decoder, optimizer
        self.ema = ema
        self.max_grad_norm = max_grad_norm
        self.sigma, self.kl_weight = noise_max_std, kl_weight                       # :66, :121
        # SSIM reconstruction loss (not in the reference): total += alpha_ssim * (1 - SSIM(recon,
        # img)), the gradient added onto the MSE's.  Off (0, the default): the iteration launches what it launched before.
        self.alpha_ssim = float(alpha_ssim)
        # Its multi-scale form: ssim_scales not None makes the term 1 - MS-SSIM(recon, img) over a 2x
        # pyramid (csrc/msssim.hip), same slot; True / "auto", an int or 1 - 5 weights as VAEGANTrainer takes them.  None
        # (the default): the single-scale launch, exactly.
        if ssim_scales is not None:
            if self.alpha_ssim == 0.0:
                raise ValueError("ssim_scales needs alpha_ssim != 0 (it selects the form of the SSIM term)")
            trainer_scales(ssim_scales, 1 << 14, 1 << 14)
        self.ssim_scales = ssim_scales
        # Training on degraded pairs: train_step(img, ..., noisy=, rects=) feeds `noisy` to the
        # Encoder; with hole_weight != 1 and rects the reconstruction term is the region-weighted MSE (csrc/regionloss.hip).
        self.hole_weight = float(hole_weight)
        if not (math.isfinite(self.hole_weight) and self.hole_weight >= 0.0):
            raise ValueError("hole_weight must be finite and >= 0")
        self.dt = _same_dtype(encoder, decoder)
        self._nets, self._opts = (encoder, decoder), (optimizer,)

    def _clip_opts(self):
        return {"EG": self.opt}

    def _extra_key(self):
        s = self.ssim_scales
        return () if s is None else (("msssim", s if isinstance(s, (bool, int, str)) else tuple(float(x) for x in s)),)

    def train(self):
        self.E.train(), self.G.train()                                             # :98-99

    def train_step(self, img: torch.Tensor, eps_img: Optional[torch.Tensor] = None,
                   eps_z: Optional[torch.Tensor] = None, epoch: int = 0, noisy: Optional[torch.Tensor] = None,
                   rects: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> device tensor [recon_loss, kl_loss (sum, not /B), total, ssim_loss]: slot 3 holds 1 - SSIM(recon, img)
        (unweighted; total includes alpha_ssim times it) when alpha_ssim != 0 and reads 0 otherwise.
        noisy (device f32 of img's shape): the PAIRED step -- the Encoder reads `noisy` in place of clamp(img + sigma *
        eps_img); eps_img is neither drawn nor read (the noise stream advances as ever: eps_z stays draw 1).  rects (f32
        [B, 8], data.DeviceLoader.last_rects) with hole_weight != 1: slot 0 holds the region-weighted MSE L_w, total uses
        it, and the vector grows to 5 slots: slot 4 holds the mean squared error inside the holes."""
        if noisy is None and rects is not None:
            raise ValueError("rects belongs to the paired step: pass noisy= as well")
        _need_cuda(img, "VAETrainer.train_step")
        E, Gn, dt = self.E, self.G, self.dt
        B, dev, L = img.shape[0], img.device, E.latent_dim
        img = img.contiguous()
        if noisy is not None:
            _need_cuda(noisy, "VAETrainer.train_step")
            if noisy.dtype != torch.float32 or noisy.shape != img.shape:
                raise RuntimeError("VAETrainer.train_step: noisy must be a device f32 batch of img's shape")
            noisy = noisy.contiguous()
        weighted = noisy is not None and rects is not None and self.hole_weight != 1.0
        if (eps_img is None and noisy is None) or eps_z is None:
            # the reference's randn_like draws, generated in HIP (Philox keyed by torch's device seed; the one-thread
            # advance kernel is captured with the iteration, so graph replays draw fresh noise)
            noise = ops.default_noise(dev)
            noise.advance()
            if eps_img is None and noisy is None:
                eps_img = noise.randn(tuple(img.shape), 0)                         # :104
            if eps_z is None:
                eps_z = noise.randn((B, L), 1)                                     # :114
        losses = ops.zeros_f32(5 if weighted else 4, dev)
        sink = GradSink(direct=True)
        if noisy is not None:
            noisy_h = ops.nchw_to_nhwc(noisy, G.padc(img.shape[1], dt), dt)
        else:
            noisy_h, _ = ops.noisy_clamp_to_nhwc(img, eps_img, self.sigma, G.padc(img.shape[1], dt), dt)   # :104-105
        mulv, ctxE = E._engine.forward(noisy_h, B, E.training, True)               # :111
        mulv = mulv.view(B, -1)
        z, lvc = ops.reparam_forward(mulv, eps_z, L, G.padc(Gn.nz, dt), dt)        # :112-115
        pre, ctxG = Gn.engine_forward(z, B)                                        # :116
        recon = ops.nhwc_to_nchw(pre, Gn.nc, dt, apply_tanh=True)
        if weighted:
            d_recon = ops.region_mse_forward_backward(recon, img, rects, self.hole_weight, 1.0, losses[0:1], losses[4:5], True)
        else:
            d_recon = ops.mse_forward_backward(recon, img, 1.0, losses[0:1], True)  # :119
        ops.kl_forward(mulv, lvc, L, 1.0, dt, out=losses[1:2])                     # :120
        w = min(epoch / 50, 1.0) * self.kl_weight                                  # :121
        torch.add(losses[0:1], losses[1:2], alpha=w, out=losses[2:3])
        if self.alpha_ssim != 0.0:
            if self.ssim_scales is None:
                ops.ssim_loss_forward_backward(recon, img, self.alpha_ssim, losses[3:4], False, d_recon)
            else:
                ops.msssim_loss_forward_backward(recon, img, trainer_scales(self.ssim_scales, *img.shape[2:]),
                                                 self.alpha_ssim, losses[3:4], False, d_recon)
            torch.add(losses[2:3], losses[3:4], alpha=self.alpha_ssim, out=losses[2:3])
        self.opt.zero_grad(memset=False)                                           # :124
        d_pre = ops.nchw_grad_to_nhwc(d_recon, recon, G.padc(Gn.nc, dt), dt)
        dz = Gn._engine.backward(ctxG, d_pre, True, sink)
        dmulv = ops.reparam_kl_backward(mulv, lvc, eps_z, dz, w, L, dt)
        E._engine.backward(ctxE, dmulv.view(B, 1, 1, -1), False, sink)
        if self._clip is not None:
            self._clip.clip("EG")
        self.opt.step()                                                            # :126
        if self.ema is not None:
            self.ema.update()
        return losses

    def step_graphed(self, img, eps_img=None, eps_z=None, noisy=None, rects=None, **scalars):
        """_Graphed.step_graphed; noisy / rects (the paired step) are static inputs of their own capture."""
        if noisy is None:
            if rects is not None:
                raise ValueError("rects belongs to the paired step: pass noisy= as well")
            return self._graphed_call(self.train_step, (img, eps_img, eps_z), scalars)
        return self._graphed_call(self._paired_step, (img, eps_z, noisy, rects), scalars, tag=("paired", self.hole_weight))

    def _paired_step(self, img, eps_z, noisy, rects, **scalars):
        return self.train_step(img, None, eps_z, noisy=noisy, rects=rects, **scalars)


# ---------------------------------------------------------------------------------------------------------------
class _GANBase(_Graphed):
    def __init__(self, netG, netD, optimizerG, optimizerD, elide_dead_grads: bool = False,
                 group_d_passes: bool = True, ema=None, max_grad_norm=None, augment=None):
        """max_grad_norm: networks "G" and "D"; grad_norms rows in that order (D's row: its last update's).
        augment (augment.DiffAugment or a policy string): every Discriminator pass reads the augmented
        copy of its [2B] input, real image b and fake image b sharing row b of ONE table per train_step (aug_params, [B, 8]);
        the generator pass's input gradient goes back through the adjoint.  The table is drawn from a NoiseStream of the
        trainer's own (seeded from torch's device seed like the VAE-GAN's, advanced once per train_step; augment_state() /
        load_augment_state() save and restore it).  None: nothing launched, nothing allocated."""
        self.G, self.D, self.opt_G, self.opt_D = netG, netD, optimizerG, optimizerD
        self.ema = ema
        self.max_grad_norm = max_grad_norm
        # The generator step's backward through D also produces D weight gradients that the next netD.zero_grad()
        # clears unread (module-level zero_grad, gan_code.py:195/:302).  False = compute them anyway, as the
        # reference does.
        self.elide_dead_grads = elide_dead_grads
        self.group_d_passes = group_d_passes
        self.dt = _same_dtype(netG, netD)
        self._nets, self._opts = (netG, netD), (optimizerG, optimizerD)
        self.augment = A.DiffAugment.of(augment)
        self.aug_params, self.aug_noise = None, None
        if self.augment is not None:
            A.check_dtype(self.dt)

    def _extra_key(self):
        if self.augment is None:
            return ()
        if self.aug_noise is None:                 # on the host, before any capture: the key names the state buffer
            self.aug_noise = ops.NoiseStream(next(self.D.parameters()).device, torch.cuda.initial_seed())
        return self.augment.key() + (self.aug_noise.state.data_ptr(),)

    def _aug_begin(self, B, H, W, dev):
        """Top of an augmented train_step: advance the trainer's stream, draw the step's one table."""
        if self.aug_noise is None or self.aug_params is None or self.aug_params.shape[0] != B:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the augmentation state would be allocated during graph capture; run a warm-up step first")
            if self.aug_noise is None:
                self.aug_noise = ops.NoiseStream(dev, torch.cuda.initial_seed())
            self.aug_params = torch.empty(B, 8, dtype=torch.float32, device=dev)
            self._gstate = None                    # a captured iteration points at the old buffers
        self.aug_noise.advance()
        self.augment.draw(self.aug_noise.state, B, H, W, out=self.aug_params)

    def augment_state(self):
        """The augmentation stream's {seed, iteration} (host int64[2]) for a checkpoint, or None."""
        return None if self.aug_noise is None else self.aug_noise.get_state().cpu()

    def load_augment_state(self, st) -> None:
        if st is None or self.augment is None:
            return
        dev = next(self.D.parameters()).device
        if self.aug_noise is None:
            self.aug_noise = ops.NoiseStream(dev, int(st[0]))
            self._gstate = None
        self.aug_noise.seed = int(st[0])
        self.aug_noise.set_state(st)

    def _clip_opts(self):
        return {"G": self.opt_G, "D": self.opt_D}

    def train(self):
        self.G.train(), self.D.train()

    def _gen(self, noise, keep):
        """noise [B,nz,1,1] f32 -> (tanh image NCHW f32, the same image in D's NHWC layout, ctx)."""
        dt, Gn = self.dt, self.G
        B = noise.shape[0]
        zh = ops.nchw_to_nhwc(noise.contiguous(), G.padc(Gn.nz, dt), dt)
        pre, ctx = Gn._engine.forward(zh, B, Gn.training, keep)
        return ops.nhwc_to_nchw(pre, Gn.nc, dt, apply_tanh=True), ctx

    def _gen_backward(self, ctxG, fake, d_fake_nhwc, sink):
        dt, Gn = self.dt, self.G
        d_img = ops.nhwc_to_nchw(d_fake_nhwc, Gn.nc, dt)
        d_pre = ops.nchw_grad_to_nhwc(d_img, fake, G.padc(Gn.nc, dt), dt)
        Gn._engine.backward(ctxG, d_pre, False, sink)


class DCGANTrainer(_GANBase):
    """train_gan's loop body (gan_code.py:194-219).  optimizerD / optimizerG: Adam(lr=2e-4, betas=(0.5, 0.999))
    (gan_code.py:179-180)."""
    LOSS_NAMES = ("errD_real", "errD_fake", "errG")

    def train_step(self, real: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        _need_cuda(real, "DCGANTrainer.train_step")
        D, dt = self.D, self.dt
        B, dev = real.shape[0], real.device
        if noise is None:
            ns = ops.default_noise(dev)
            ns.advance()
            noise = ns.randn((B, self.G.nz, 1, 1), 0)                              # :203
        losses = ops.zeros_f32(4, dev)
        sink = GradSink(direct=True)
        CP = G.padc(D.nc, dt)
        # D(real) -> G(noise) -> D(fake.detach()) in the reference; G's forward does not touch D, so the two D
        # passes run as ONE grouped 2B-row pass (per-group BatchNorm statistics, running stats real-then-fake)
        fake, ctxG = self._gen(noise, True)                                        # :204
        both = ops.empty_act((2 * B, real.shape[2], real.shape[3], CP), dt, dev)
        real_h = ops.nchw_to_nhwc(real.contiguous(), CP, dt, out=both[:B])
        fake_h = ops.nchw_to_nhwc(fake, CP, dt, out=both[B:])
        aug = self.augment
        if aug is not None:
            self._aug_begin(B, both.shape[1], both.shape[2], dev)
            both = aug.forward(both, self.aug_params, D.nc, dt)
            real_h, fake_h = both[:B], both[B:]
        self.opt_D.zero_grad(memset=False)                                         # :195
        if self.group_d_passes and D._engine.can_group(B, 2):
            p_both, c_both = D.engine_forward(both, B, groups=2)
            dp = torch.empty_like(p_both)
            ops.bce_forward_backward(p_both[:B], 1.0, 1.0, losses[0:1], False, True, out=dp[:B])   # :199-200
            ops.bce_forward_backward(p_both[B:], 0.0, 1.0, losses[1:2], False, True, out=dp[B:])   # :206-207
            D._engine.backward(c_both, dp, False, sink)                            # :201, :208
        else:
            p_real, c_real = D.engine_forward(real_h, B)
            p_fake, c_fake = D.engine_forward(fake_h, B)
            dp_real = ops.bce_forward_backward(p_real, 1.0, 1.0, losses[0:1], False, True)
            dp_fake = ops.bce_forward_backward(p_fake, 0.0, 1.0, losses[1:2], False, True)
            D._engine.backward(c_real, dp_real, False, sink)
            D._engine.backward(c_fake, dp_fake, False, sink)
        if self._clip is not None:
            self._clip.clip("D")
        self.opt_D.step()                                                          # :209
        self.opt_G.zero_grad(memset=False)                                         # :212
        p_adv, c_adv = D.engine_forward(fake_h, B)                                 # :214
        dp_adv = ops.bce_forward_backward(p_adv, 1.0, 1.0, losses[2:3], False, True)   # :215
        d_fake = D._engine.backward(c_adv, dp_adv, True, sink, param_grads=not self.elide_dead_grads)   # :216
        if aug is not None:
            d_fake = aug.backward(d_fake, self.aug_params, D.nc, dt)
        self._gen_backward(ctxG, fake, d_fake, sink)
        if self._clip is not None:
            self._clip.clip("G")
        self.opt_G.step()                                                          # :217
        if self.ema is not None:
            self.ema.update()
        return losses


class WGANTrainer(_GANBase):
    """train_wgan's loop body (gan_code.py:296-331): ``critic_iters`` critic updates, each followed by the weight
    clamp, then one generator update.  The critic is the same Discriminator, sigmoid included (gan_code.py:270)."""
    LOSS_NAMES = ("d_loss", "g_loss")

    def __init__(self, netG, netD, optimizerG, optimizerD, clip_value: float = 0.01, critic_iters: int = 5, **kw):
        super().__init__(netG, netD, optimizerG, optimizerD, **kw)
        self.clip_value, self.critic_iters = clip_value, critic_iters              # :281-282

    def train_step(self, real: torch.Tensor, critic_noise: Optional[torch.Tensor] = None,
                   gen_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """critic_noise: [critic_iters, B, nz, 1, 1] (the randn of :309 per critic iteration), gen_noise
        [B, nz, 1, 1] (:325).  -> device tensor [d_loss of the last critic iteration, g_loss]."""
        _need_cuda(real, "WGANTrainer.train_step")
        D, dt = self.D, self.dt
        B, dev, nz = real.shape[0], real.device, self.G.nz
        if critic_noise is None or gen_noise is None:
            ns = ops.default_noise(dev)
            ns.advance()
            if critic_noise is None:
                critic_noise = ns.randn((self.critic_iters, B, nz, 1, 1), 0)
            if gen_noise is None:
                gen_noise = ns.randn((B, nz, 1, 1), 1)
        losses = ops.zeros_f32(4, dev)
        sink = GradSink(direct=True)
        CP = G.padc(D.nc, dt)
        both = ops.empty_act((2 * B, real.shape[2], real.shape[3], CP), dt, dev)
        real_h = ops.nchw_to_nhwc(real.contiguous(), CP, dt, out=both[:B])
        grouped = self.group_d_passes and D._engine.can_group(B, 2)
        aug, seen = self.augment, both
        if aug is not None:
            self._aug_begin(B, both.shape[1], both.shape[2], dev)
            seen = torch.empty_like(both)                                          # what the critic reads
        for it in range(self.critic_iters):                                        # :301
            self.opt_D.zero_grad(memset=False)                                     # :302
            fake, _ = self._gen(critic_noise[it], False)                           # :309-310 (.detach(): forward only)
            fake_h = ops.nchw_to_nhwc(fake, CP, dt, out=both[B:])
            if aug is not None:
                aug.forward(both, self.aug_params, D.nc, dt, out=seen)             # the refilled batch, the step's one table
                real_h, fake_h = seen[:B], seen[B:]
            if grouped:
                p_both, c_both = D.engine_forward(seen, B, groups=2)
                dp = torch.empty_like(p_both)
                ops.mean_forward_backward(p_both[:B], -1.0, 1.0, losses[0:1], False, True, out=dp[:B])   # :305-306
                ops.mean_forward_backward(p_both[B:], 1.0, 1.0, losses[0:1], True, True, out=dp[B:])     # :311-315
                D._engine.backward(c_both, dp, False, sink)
            else:
                p_real, c_real = D.engine_forward(real_h, B)
                p_fake, c_fake = D.engine_forward(fake_h, B)
                dp_real = ops.mean_forward_backward(p_real, -1.0, 1.0, losses[0:1], False, True)
                dp_fake = ops.mean_forward_backward(p_fake, 1.0, 1.0, losses[0:1], True, True)
                D._engine.backward(c_real, dp_real, False, sink)
                D._engine.backward(c_fake, dp_fake, False, sink)
            if self._clip is not None:
                self._clip.clip("D")
            self.opt_D.step()                                                      # :317
            ops.clamp_(self.opt_D.flat_p, -self.clip_value, self.clip_value)       # :320-321
            bump_weights_epoch(self.opt_D.params)
        self.opt_G.zero_grad(memset=False)                                         # :324
        fake, ctxG = self._gen(gen_noise, True)                                    # :325-326
        fake_h = ops.nchw_to_nhwc(fake, CP, dt, out=both[B:])
        if aug is not None:
            fake_h = aug.forward(fake_h, self.aug_params, D.nc, dt, out=seen[B:])
        p_adv, c_adv = D.engine_forward(fake_h, B)                                 # :327
        dp_adv = ops.mean_forward_backward(p_adv, -1.0, 1.0, losses[1:2], False, True)   # :328
        d_fake = D._engine.backward(c_adv, dp_adv, True, sink, param_grads=not self.elide_dead_grads)   # :330
        if aug is not None:
            d_fake = aug.backward(d_fake, self.aug_params, D.nc, dt)
        self._gen_backward(ctxG, fake, d_fake, sink)
        if self._clip is not None:
            self._clip.clip("G")
        self.opt_G.step()                                                          # :331
        if self.ema is not None:
            self.ema.update()
        return losses
