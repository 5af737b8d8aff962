"""The VAE-GAN training iteration of the reference (vaegan_code.py:65-135) driven directly on the
HIP kernel chains -- no autograd graph, gradients written straight into the optimizers' flat
buffers.  Same op order, loss weights, zero_grad/step order and BatchNorm modes as the reference
(SURVEY.md A13); the three ``randn_like`` draws (vaegan_code.py:77,91,92) can be injected for
parity runs or are drawn on the device.

    trainer = VAEGANTrainer(encoder, decoder, discriminator, opt_E, opt_Dec, opt_Dis)
    losses = trainer.train_step(real_images, epoch)          # device tensor, no host sync
"""
import math
import os
import time
from typing import Dict, Optional

import torch

from . import geometry as G
from . import ops
from .capture import CaptureRefused, HostMirrors, capture, replay
from . import augment as A
from .engine import GradSink
from .gradclip import ClipOption
from .losses import trainer_scales
from .optim import lr_report

LOSS_NAMES = ("recon_loss", "kl_loss", "g_loss_adv", "d_loss_1", "d_loss_2")
# draw ids of the prior stream in the iteration's noise stream (0, 1, 2: eps_z, eps_real, eps_recon): the prior latent and the
# instance noise of the decoded prior samples
DRAW_PRIOR, DRAW_XP = 3, 4
# more than two periods of c10d's NCCL watchdog (ProcessGroupNCCL::kWatchdogThreadSleepMillis = 100): see _capture
WATCHDOG_PASS_SECONDS = 0.25


class _SyncBNHandoff:
    """What the engines see as `bn_sync` in SyncBN mode: the statistics all-reduce of every BatchNorm goes through the
    trainer's graph cut, so that under hipGraph capture the collective stays OUTSIDE the captured segments (it is
    re-issued between segment replays on the same static f64 buffer) and runs immediately in eager mode."""

    def __init__(self, trainer):
        self.trainer = trainer

    @property
    def world(self):
        return self.trainer.reducer.world

    def all_reduce_sum(self, t):
        self.trainer._cut(lambda: self.trainer.reducer.all_reduce_sum(t))


class VAEGANTrainer(ClipOption):
    def __init__(self, encoder, decoder, discriminator, opt_E, opt_Dec, opt_Dis, alpha_kl: float = 0.1,
                 alpha_adv: float = 0.1, noise_sigma: float = 0.05, real_label: float = 0.9, fake_label: float = 0.1,
                 d_iters: int = 2, elide_dead_grads: bool = False, reducer=None, group_d_passes: bool = True,
                 sync_bn: bool = False, feat_layer: Optional[int] = None, alpha_feat: float = 0.0, alpha_pix: float = 1.0,
                 alpha_ssim: float = 0.0, hole_weight: float = 1.0, ema=None, max_grad_norm=None, augment=None,
                 prior_stream: bool = False, ssim_scales=None):
        self.E, self.G, self.D = encoder, decoder, discriminator
        self.opt_E, self.opt_G, self.opt_D = opt_E, opt_Dec, opt_Dis
        self.alpha_kl, self.alpha_adv, self.sigma = alpha_kl, alpha_adv, noise_sigma          # :49-50, :91-92
        self.real_label, self.fake_label, self.d_iters = real_label, fake_label, d_iters      # :88-89, :95
        # The generator-loss pass through D (vaegan_code.py:110,133) also produces D weight gradients that the
        # next opt_Dis.zero_grad() discards unread.  False = compute them anyway (what the reference executes).
        self.elide_dead_grads = elide_dead_grads
        # Discriminator-feature reconstruction loss (Larsen et al. 2016, eq. 2): total +=
        # alpha_feat * mean((D_l(recon_noisy) - D_l(real_noisy))^2), D_l = the activated output of the Discriminator's engine
        # stage feat_layer, D_l(real_noisy) a constant.  alpha_pix weighs the pixel MSE (alpha_pix = 0, alpha_feat > 0 is
        # Larsen's form).  Off (alpha_feat = 0, the default): the iteration launches exactly what it launched without it.
        self.alpha_feat, self.alpha_pix = float(alpha_feat), float(alpha_pix)
        if feat_layer is not None:
            discriminator._engine.check_feat_stage(feat_layer)
        elif self.alpha_feat != 0.0:
            raise ValueError("alpha_feat != 0 needs feat_layer (a BatchNorm stage of the Discriminator)")
        self.feat_layer = feat_layer
        # SSIM reconstruction loss: total += alpha_ssim * (1 - SSIM(recon, real)), the metric of
        # denoise.py (11 x 11 Gaussian window, interior pixels) as a training term; its gradient is added onto the pixel
        # MSE's in the buffer that launch wrote (csrc/ssimloss.hip, one launch for forward and backward).  Off (0, the
        # default): the iteration launches exactly what it launched without it.
        self.alpha_ssim = float(alpha_ssim)
        # Multi-scale form of that term: with ssim_scales not None the structural term is 1 - MS-SSIM(recon,
        # real) over a 2x pyramid (csrc/msssim.hip; at most five launches whatever the number of scales) -- same place in the
        # iteration, same loss slot, same "ssim_loss" key.  ssim_scales: True or "auto" = the default scales of the image size
        # (ops.msssim_weights), an int = that many, a sequence of 1 - 5 weights = those.  None (the default): the single-scale
        # launches above, exactly.
        if ssim_scales is not None:
            if self.alpha_ssim == 0.0:
                raise ValueError("ssim_scales needs alpha_ssim != 0 (it selects the form of the SSIM term)")
            trainer_scales(ssim_scales, 1 << 14, 1 << 14)          # a bad count / weight fails here, not in the first step
        self.ssim_scales = ssim_scales
        # Training on degraded pairs: train_step(clean, ..., noisy=, rects=) feeds `noisy` to the
        # Encoder and, with hole_weight != 1, replaces the pixel MSE by the region-weighted one (csrc/regionloss.hip): the
        # squared error inside each image's occlusion rectangle counts hole_weight times.  1 (the default) or no rects:
        # the pixel MSE launches of the unpaired step.
        self.hole_weight = float(hole_weight)
        if not (math.isfinite(self.hole_weight) and self.hole_weight >= 0.0):
            raise ValueError("hole_weight must be finite and >= 0")
        # Weight averaging (ema.EMA over the Encoder and / or the Generator and their optimizers): the
        # iteration ends with ema.update(), ONE more launch directly after the Encoder / Generator optimizer step, captured
        # with the rest.  None (the default): the iteration launches exactly what it launched without it.
        self.ema = ema
        # Gradient-norm clipping: each network's gradient is clipped to its OWN global L2 norm
        # (torch.nn.utils.clip_grad_norm_ per optimizer; a joint Encoder + Generator norm is not offered).  A number clips
        # all three networks at that value, a dict with keys among "E", "G", "D" only the named ones, float("inf") only
        # reports the norms.  The reduction runs directly before each optimizer step (after the gradient all-reduce under
        # data parallelism) and leaves the coefficient on the device, where the Adam launch reads it: 2 launches per clip
        # point, 2 d_iters + 2 per iteration, captured with the rest.  grad_norms ([3, 2] device tensor, rows E, G, D =
        # [norm, coefficient]; D's is the last Discriminator update's) and loss_dict() report them.  None (the default): the
        # iteration launches exactly what it launched without it and nothing is allocated.
        self.max_grad_norm = max_grad_norm
        # Differentiable augmentation (augment.DiffAugment or a policy string): after the [2B] buffer of
        # noisy real / reconstructed images is filled, ONE table of per-image parameters is drawn from the noise stream (at the
        # iteration the prologue just advanced to; reused across d_iters, as the reference reuses its instance noise) and every
        # Discriminator pass -- the d_iters updates, the feature tap, the adversarial pass -- reads the augmented copy; image b
        # and its reconstruction share row b.  The adversarial pass's input gradient goes back through the adjoint.  The table
        # of the last iteration stays in aug_params ([B, 8] device tensor).  The noise stream then exists and advances also
        # when all three eps are injected; the checkpoint's noise state determines the draws.  None (the default): the
        # iteration launches exactly what it launched without it and nothing is allocated.
        self.augment = A.DiffAugment.of(augment)
        self.aug_params = None
        # Decoded prior samples as the third Discriminator stream (Larsen et al. 2016, algorithm 1):
        # z_p ~ N(0, I) (draw 3), x_p = G(z_p) in a second train-mode Generator forward after the reconstruction's, xp_noisy =
        # x_p + sigma eps_xp (draw 4); every Discriminator update adds BCE(D(xp_noisy.detach()), fake_label) and the Generator
        # loss adds alpha_adv * BCE(D(xp_noisy), real_label) (slot 8 of the loss tensor, g_loss_adv_prior).  Its gradient
        # reaches the Generator only, summed with the reconstruction's in the flat gradient buffer.  False (the default): the
        # iteration launches exactly what it launched without it and returns 8 slots.
        if not isinstance(prior_stream, bool):
            raise ValueError("prior_stream must be True or False")
        if prior_stream and (decoder.nc != discriminator.nc or decoder.nz != encoder.latent_dim):
            raise ValueError("prior_stream=True needs a Generator that decodes the Encoder's latent into the Discriminator's "
                             "image channels")
        self.prior_stream = prior_stream
        self.group_d_passes = group_d_passes       # run a D iteration's real+fake passes as one 2B-row launch chain
        # BCE + its gradient + the sigmoid / head backward as ONE launch per Discriminator pass (ops.head_backward;
        # bit-identical to the three separate launches, which False selects)
        self.fuse_head_backward = True
        # noise counter + the three optimizers' step counters / bias corrections in ONE launch at the top of the iteration
        # (ops.step_prologue) instead of one per optimizer step; False: every step() prepares itself
        self.fuse_step_prologue = os.environ.get("VG_STEP_PROLOGUE", "1") != "0"
        # round 4: four pairs of small launches merged (the Encoder's input conversion + the noisy real batch; the MSE's
        # final sum + the KL term; the Encoder's + the Generator's Adam step; the loss slots' memset + the prologue) --
        # bit-identical results; False restores the separate launches (A/B and test switch)
        self.merge_small_launches = os.environ.get("VG_MERGE_SMALL", "1") != "0"
        self.reducer = reducer
        # sync_bn: BatchNorm statistics over the global batch of all ranks (ddp.py) -- an N-rank step then equals
        # the reference's single-process step on the concatenated batch.  Off: per-replica statistics.
        self.sync_bn = bool(sync_bn)
        if self.sync_bn and reducer is None:
            raise ValueError("sync_bn=True needs a ddp.GradReducer (reducer=...)")
        for net in (encoder, decoder, discriminator):
            net._engine.bn_sync = _SyncBNHandoff(self) if self.sync_bn else None
        dts = {encoder._dt, decoder._dt, discriminator._dt}
        if len(dts) != 1:
            raise ValueError("encoder / decoder / discriminator must share one engine dtype")
        self.dt = dts.pop()
        if self.augment is not None:
            A.check_dtype(self.dt)
        self.latent = encoder.latent_dim
        self.losses = None
        self.noise = None               # ops.NoiseStream for the in-kernel randn_like draws (created on first use)
        self._noise_pinned_seed = None  # torch device seed at the time a checkpoint's noise stream was restored
        self._bucket_plans = {}
        self._graph = None              # capture.Captured: key, [hipGraph segments], [collectives between them], static in, ...
        self._warm_key = None
        self._cut_hook = None           # set while capturing: splits the iteration into graph segments
        self._inline_failed = False     # capturing the collectives inside the graph failed once: use the segmented form
        self.last_step_weighted = False # the last iteration used the region-weighted term (loss_dict reports hole_mse)

    def _clip_opts(self):
        return {"E": self.opt_E, "G": self.opt_G, "D": self.opt_D}

    def train(self):
        self.E.train(), self.G.train(), self.D.train()                                         # :56-58

    def _noise_stream(self, dev):
        """The generator behind the non-injected draws: torch's device seed (utils.configure_seed /
        torch.cuda.manual_seed) keys it, as it keys torch.randn_like in the reference; re-seeding torch starts a new
        stream (and invalidates a captured graph, which holds the old state buffer)."""
        seed = torch.cuda.initial_seed()
        if self.noise is not None and self._noise_pinned_seed == seed:
            return self.noise           # restored from a checkpoint: pinned until torch is explicitly re-seeded
        self._noise_pinned_seed = None
        if self.noise is None or self.noise.seed != seed:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("noise stream (re)seeded during graph capture")
            self.noise = ops.NoiseStream(dev, seed)
            self._graph = None
        return self.noise

    def _capture_key(self, real, epoch, inject, paired=False, with_rects=False):
        """Everything a captured graph freezes: shapes, every scalar kernel argument (loss weights, labels, noise
        sigma, Adam hyper-parameters, the data-parallel gradient scale), the schedule switches and the buffers the
        launches point at.  A change in any of them re-captures instead of silently replaying stale values.  Of the learning
        rate that is the base rate, the schedule's fields and the weight decay (Adam.capture_key): the rate of the step is
        worked out on the device, so a scheduled run replays one graph while the rate moves."""
        opts = tuple((o.capture_key(), o.betas, o.eps, o.grad_scale, o.flat_p.data_ptr()) for o in (self.opt_E, self.opt_G, self.opt_D))
        return (tuple(real.shape), float(self.alpha_kl * min(1.0, epoch / 50)), inject, self.E.training, self.G.training,
                self.D.training, self.alpha_adv, self.alpha_feat, self.alpha_pix, self.alpha_ssim, self.feat_layer, self.sigma,
                self.real_label,
                self.fake_label, self.d_iters,
                self.elide_dead_grads, self.group_d_passes, self.fuse_head_backward, self.fuse_step_prologue,
                self.merge_small_launches, self.prior_stream,
                id(self.reducer), self.sync_bn, opts,
                None if self.noise is None or (inject and self.augment is None) else self.noise.state.data_ptr()) \
            + (self.augment.key() if self.augment is not None else ()) \
            + ((True, with_rects, self.hole_weight) if paired else ()) \
            + ((("msssim",) + trainer_scales(self.ssim_scales, *real.shape[2:]),) if self.ssim_scales is not None else ()) \
            + ((("ema",) + self.ema.key(),) if self.ema is not None else ()) + self._clip_key()

    # ---- data-parallel gradient hand-off (ddp.GradReducer) -------------------------------------------------------
    def _buckets_for(self, opt, net):
        """Plan `opt`'s gradient buckets once: parameter -> stage whose backward completes its gradient."""
        key = id(opt)
        if key not in self._bucket_plans:
            stage_of = net._engine.param_stage()
            ready = [stage_of.get(id(p), 0) for p in opt.params]
            plan = getattr(self.reducer, "plan", None)
            self._bucket_plans[key] = plan(opt, ready) if plan is not None else None
        return self._bucket_plans[key]

    def _grad_hook(self, opt, net):
        """on_grads callback for engine.backward: after stage i's weight gradients are enqueued, launch (behind a
        graph cut) the all-reduce of every bucket that stage completes.  Stage 0 is left to _finish_reduce, which
        launches the last bucket and waits in ONE cut (no empty graph segment between two cuts)."""
        if self.reducer is None or self._buckets_for(opt, net) is None:
            return None
        events = {ev for _, _, ev in self._bucket_plans[id(opt)] if ev > 0}

        def hook(i):
            if i in events:
                self._cut(lambda: self.reducer.launch_ready(opt, i))
        return hook

    def _finish_reduce(self, opt, net, wait=True, also_wait=()):
        """End of `net`'s backward: launch what is left of opt's buckets, optionally wait for all of them."""
        if self.reducer is None:
            return
        bucketed = self._buckets_for(opt, net) is not None

        def fn():
            if bucketed:
                self.reducer.launch_ready(opt, 0)
            elif wait:
                self.reducer.reduce(opt)
            else:
                self.reducer.reduce_async(opt)
            if wait:
                self.reducer.wait(opt)
            for o in also_wait:
                self.reducer.wait(o)
        self._cut(fn)

    def _cut(self, collective) -> None:
        """A point where the iteration hands gradients to the reducer.  Eager: run the collective now.  While
        capturing: close the current hipGraph segment, remember the collective, open the next segment -- RCCL
        calls stay OUTSIDE the captured graphs and are launched between segment replays."""
        if self._cut_hook is None:
            collective()
        else:
            self._cut_hook(collective)

    def _weighted(self, noisy, rects) -> bool:
        """Whether a step with these arguments uses the region-weighted reconstruction term."""
        return noisy is not None and rects is not None and self.hole_weight != 1.0

    def _check_pair(self, real, noisy, noisy_nhwc, rects) -> None:
        """The paired step's tensors against the clean batch: device, dtype and shape, before anything reads or copies them
        (a copy into a captured step's static buffer would convert a wrong dtype or broadcast a wrong shape silently)."""
        dt, B = self.dt, real.shape[0]
        if not noisy.is_cuda or noisy.device != real.device or noisy.dtype != torch.float32 or noisy.shape != real.shape:
            raise RuntimeError("train_step: noisy must be a device f32 batch of real's shape")
        if noisy_nhwc is not None:
            want = (B, real.shape[2], real.shape[3], G.padc(real.shape[1], dt))
            if not noisy_nhwc.is_cuda or tuple(noisy_nhwc.shape) != want or noisy_nhwc.dtype != ops.TORCH_DT[dt] \
                    or not noisy_nhwc.is_contiguous():
                raise RuntimeError(f"train_step: noisy_nhwc must be a contiguous device {ops.TORCH_DT[dt]} tensor of "
                                   f"shape {want} (data.DeviceLoader.want_nhwc)")
        if rects is not None and (not rects.is_cuda or rects.device != real.device or rects.dtype != torch.float32
                                  or tuple(rects.shape) != (B, 8) or not rects.is_contiguous()):
            raise RuntimeError("train_step: rects must be a contiguous device f32 [B, 8] tensor (ops.degrade_params)")

    def train_step(self, real: torch.Tensor, epoch: int, eps_z: Optional[torch.Tensor] = None,
                   eps_real: Optional[torch.Tensor] = None, eps_recon: Optional[torch.Tensor] = None, *,
                   noisy: Optional[torch.Tensor] = None, noisy_nhwc: Optional[torch.Tensor] = None,
                   rects: Optional[torch.Tensor] = None, eps_prior: Optional[torch.Tensor] = None,
                   eps_xp: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One iteration.  Returns a device tensor [recon_loss, kl_loss, g_loss_adv, d_loss_1, d_loss_2, feat_loss, ssim_loss,
        hole_mse]: slot 5 holds the Discriminator-feature reconstruction loss (unweighted, like recon_loss) when alpha_feat
        != 0, slot 6 the SSIM reconstruction loss 1 - SSIM(recon, real) (unweighted) when alpha_ssim != 0; each reads 0 when
        its term is off.  With prior_stream=True there is a ninth slot, g_loss_adv_prior = BCE(D(xp_noisy), real_label)
        (unweighted), the d_loss slots hold the three-term loss, and eps_prior ([B, L] f32) / eps_xp ([B, C, S, S] f32) inject
        the prior latent and the instance noise of the decoded prior samples (None: draws 3 / 4 of the noise stream).
        noisy (device f32 of real's shape): the PAIRED step on a degraded pair -- the Encoder reads `noisy` as it is (no
        clamp, no noise added); everything else (the Discriminator's real batch, the MSE / SSIM / Dis_l targets) reads
        `real`, the clean image.  noisy_nhwc: the same batch already in the Encoder's input layout ([B, H, W, padc(C)] in
        the engine dtype: data.DeviceLoader.last_nhwc), used instead of converting `noisy`.  rects (f32 [B, 8],
        DeviceLoader.last_rects) with hole_weight != 1: the reconstruction term is alpha_pix * L_w, the region-weighted
        MSE; slot 0 then holds L_w and slot 7 the mean squared error inside the holes (0 otherwise)."""
        if noisy is None and (rects is not None or noisy_nhwc is not None):
            raise ValueError("rects / noisy_nhwc belong to the paired step: pass noisy= as well")
        if not self.prior_stream and (eps_prior is not None or eps_xp is not None):
            raise ValueError("eps_prior / eps_xp belong to the prior stream: build the trainer with prior_stream=True")
        steps = [o.steps for o in (self.opt_E, self.opt_G, self.opt_D)]
        try:
            return self._train_step(real, epoch, eps_z, eps_real, eps_recon, noisy, noisy_nhwc, rects, eps_prior, eps_xp)
        except BaseException:
            # The step prologue advances the DEVICE step counters / bias corrections of all three optimizers at the top of
            # the iteration, the host mirrors (opt.steps) move with the updates at its end.  An eager iteration that dies
            # in between (OOM, a bad shape in a later pass) must not leave the two apart: a retried iteration would apply
            # t + 2 and state_dict() would save a step count that disagrees with the bias correction in use.  (A capture
            # executes nothing: train_step_graphed restores the host mirrors itself.)
            if not torch.cuda.is_current_stream_capturing():
                for o, st in zip((self.opt_E, self.opt_G, self.opt_D), steps):
                    if o.steps == st:
                        try:
                            o.state_dev[0:1].fill_(float(st))
                        except Exception:
                            pass
            raise

    def _decode(self, z, B, eps, out_noisy, CP):
        """One train-mode Generator forward of z: -> (tanh image NCHW f32, ctx), with image + sigma * eps written into
        out_noisy in the Discriminator's layout (:83 and :92; the reconstruction, and the prior stream's decoded samples)."""
        Gn, D, dt = self.G, self.D, self.dt
        if Gn.nc == D.nc and G.padc(Gn.nc, dt) == CP and Gn.fused_tail(B):
            # the last ConvTranspose2d's kernel applies Tanh and writes the NCHW image AND image + sigma*eps in D's layout
            return Gn.engine_forward(z, B, tail=dict(noise=eps, sigma=self.sigma, out_noisy=out_noisy))
        pre, ctxG = Gn.engine_forward(z, B)
        if Gn.nc == D.nc and pre.shape[-1] == CP:
            img = ops.nhwc_tanh_to_nchw_noisy(pre, Gn.nc, eps, self.sigma, out_noisy, dt)      # :83 and :92 in one pass
        else:
            img = ops.nhwc_to_nchw(pre, Gn.nc, dt, apply_tanh=True)
            ops.nchw_to_nhwc(img, CP, dt, eps=eps, sigma=self.sigma, out=out_noisy)
        if Gn._engine.trace is not None:        # test instrumentation (engine.StackEngine.trace): the unfused tail
            Gn._engine.trace.append(dict(stage=len(Gn._engine.stages) - 1, what="tail", pre=pre.clone(),
                                         img=img.clone(), noisy=out_noisy.clone()))
        return img, ctxG

    def _train_step(self, real, epoch, eps_z, eps_real, eps_recon, noisy=None, noisy_nhwc=None, rects=None, eps_prior=None,
                    eps_xp=None) -> torch.Tensor:
        if not real.is_cuda:
            raise RuntimeError("train_step needs the batch on the MI355X ('cuda'); there is no CPU path")
        E, Gn, D, dt = self.E, self.G, self.D, self.dt
        B, dev = real.shape[0], real.device
        L = self.latent
        real = real.contiguous()
        if noisy is not None:
            self._check_pair(real, noisy, noisy_nhwc, rects)
            noisy = noisy.contiguous()
        weighted = self._weighted(noisy, rects)
        self.last_step_weighted = weighted
        noise = None
        ps = self.prior_stream
        if eps_z is None or eps_real is None or eps_recon is None or (ps and (eps_prior is None or eps_xp is None)):
            # the three randn_like draws (:77, :91, :92) are generated inside the kernels that consume them
            # (Philox keyed by torch's device seed; the iteration counter is bumped on the device, also under replay);
            # the prior stream's two draws likewise
            noise = self._noise_stream(dev)
            eps_z = noise.draw(0) if eps_z is None else eps_z
            eps_real = noise.draw(1) if eps_real is None else eps_real
            eps_recon = noise.draw(2) if eps_recon is None else eps_recon
            if ps:
                eps_prior = noise.draw(DRAW_PRIOR) if eps_prior is None else eps_prior
                eps_xp = noise.draw(DRAW_XP) if eps_xp is None else eps_xp
        elif self.augment is not None:
            noise = self._noise_stream(dev)         # the augmentation table is drawn from it (and it advances) all the same
        # one single-thread launch for everything that only counts: the noise iteration and the step counters / bias
        # corrections of the three Adam steps below (the Discriminator's second update prepares itself)
        prep = self.fuse_step_prologue and self.d_iters >= 1
        # slots 0..4 are written (not accumulated) below when d_iters >= 2; with d_iters = 1 slot 4 (d_loss_2) is never
        # written and with d_iters > 2 it holds the LAST iteration's loss -- zeroed so that it reads 0, not stale memory.
        # With the prologue launch the zeroing rides on it (no memset node in the captured iteration).
        nslots = 9 if ps else 8                     # slot 8: g_loss_adv_prior
        losses = torch.empty(nslots, dtype=torch.float32, device=dev) if prep else ops.zeros_f32(nslots, dev)
        if prep:
            ops.step_prologue(noise, [self.opt_D, self.opt_G, self.opt_E], zero=losses)
        elif noise is not None:
            noise.advance()
        sink = GradSink(direct=True)

        # ---- Encode / reparameterise / decode (:74-83) ----
        # instance noise, drawn once per step (:91-92), produced directly in the layout D reads.  Both noisy batches live
        # in one [2B] buffer so that a Discriminator iteration can run real+fake as ONE grouped pass (per-group BatchNorm
        # statistics, running stats updated real-then-fake as the reference's two calls do).  The Encoder's input and the
        # Discriminator's noisy real batch are the same images: one pass over `real` writes both (round 4).
        CP = G.padc(D.nc, dt)
        ngrp = 3 if ps else 2                       # prior stream: [real_noisy | recon_noisy | xp_noisy]
        both = ops.empty_act((ngrp * B, real.shape[2], real.shape[3], CP), dt, dev)
        if noisy is None:
            pair = ops.nchw_to_nhwc_pair(real, CP, dt, eps_real, self.sigma, both[:B]) \
                if (self.merge_small_launches and G.padc(real.shape[1], dt) == CP) else None
            mulv, ctxE = E.engine_forward(real, x_nhwc=None if pair is None else pair[0])
        else:
            # paired: the Encoder's input and the Discriminator's real batch are different images, one conversion each
            pair = None
            mulv, ctxE = E.engine_forward(noisy, x_nhwc=noisy_nhwc)
        ZP = G.padc(Gn.nz, dt)
        z, lvc = ops.reparam_forward(mulv, eps_z, L, ZP, dt)
        real_noisy = both[:B] if pair is not None else \
            ops.nchw_to_nhwc(real, CP, dt, eps=eps_real, sigma=self.sigma, out=both[:B])
        recon_noisy = both[B:2 * B]
        recon, ctxG = self._decode(z, B, eps_recon, recon_noisy, CP)
        if ps:
            # the second Generator forward, on a latent from the prior: its BatchNorm buffers see recon, then prior
            z_p = ops.prior_forward(eps_prior, B, L, ZP, dt)
            x_p, ctxG_p = self._decode(z_p, B, eps_xp, both[2 * B:], CP)
        aug = self.augment
        if aug is not None:
            # one table per iteration, then everything D reads below is the augmented copy of `both`
            if self.aug_params is None or self.aug_params.shape[0] != B or self.aug_params.device != dev:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("the augmentation table would be allocated during graph capture; run a warm-up step first")
                self.aug_params = torch.empty(B, 8, dtype=torch.float32, device=dev)
            aug.draw(noise.state, B, both.shape[1], both.shape[2], out=self.aug_params)
            both = aug.forward(both, self.aug_params, D.nc, dt)
            real_noisy, recon_noisy = both[:B], both[B:2 * B]
        xp_noisy = both[2 * B:] if ps else None
        grouped = self.group_d_passes and D._engine.can_group(B, ngrp)
        fused_head = self.fuse_head_backward and 2 * B <= ops.HEAD_BWD_MAXROWS and D._engine.stages[-1].kind == "head"

        # ---- Discriminator updates (:95-105) ----
        for it in range(self.d_iters):
            slot = losses[3 + min(it, 1):4 + min(it, 1)]
            self.opt_D.zero_grad(memset=False)
            if ps:
                # three terms: BCE(D(real_noisy), real) + BCE(D(recon_noisy), fake) + BCE(D(xp_noisy), fake), three train-mode
                # calls in that order (one grouped 3B pass: per-group BatchNorm statistics, running stats updated in order,
                # weight gradients formed group after group -- the bits of the three separate passes below)
                targets = (self.real_label, self.fake_label, self.fake_label)
                if grouped:
                    p_all, c_all = D.engine_forward(both, B, groups=3)
                    if fused_head and 3 * B <= ops.HEAD_BWD_MAXROWS:
                        D._engine.backward(c_all, None, False, sink, on_grads=self._grad_hook(self.opt_D, D),
                                           head_loss=targets[:2] + (3, 1.0, slot, False, targets[2]), weight_grad_groups=3)
                    else:
                        dp = torch.empty_like(p_all)
                        for g, t in enumerate(targets):
                            rows = slice(g * B, (g + 1) * B)
                            ops.bce_forward_backward(p_all[rows], t, 1.0, slot, g > 0, True, out=dp[rows])
                        D._engine.backward(c_all, dp, False, sink, on_grads=self._grad_hook(self.opt_D, D), weight_grad_groups=3)
                else:
                    passes = [D.engine_forward(x, B) for x in (real_noisy, recon_noisy, xp_noisy)]
                    dps = [ops.bce_forward_backward(p, targets[g], 1.0, slot, g > 0, True) for g, (p, _) in enumerate(passes)]
                    for g, (_, c) in enumerate(passes):       # the later passes accumulate, the last one carries the hook
                        D._engine.backward(c, dps[g], False, sink, on_grads=self._grad_hook(self.opt_D, D) if g == 2 else None)
            elif grouped:
                p_both, c_both = D.engine_forward(both, B, groups=2)                           # .detach(): no dx below
                if fused_head:
                    # :98-104: the two BCE terms, their gradient and the head's backward in one launch
                    D._engine.backward(c_both, None, False, sink, on_grads=self._grad_hook(self.opt_D, D),
                                       head_loss=(self.real_label, self.fake_label, 2, 1.0, slot, False))
                else:
                    dp = torch.empty_like(p_both)
                    ops.bce_pair_forward_backward(p_both, self.real_label, self.fake_label, 1.0, slot, dp)   # :98-103
                    D._engine.backward(c_both, dp, False, sink, on_grads=self._grad_hook(self.opt_D, D))
            else:
                p_real, c_real = D.engine_forward(real_noisy, B)
                p_fake, c_fake = D.engine_forward(recon_noisy, B)
                dp_real = ops.bce_forward_backward(p_real, self.real_label, 1.0, slot, False, True)
                dp_fake = ops.bce_forward_backward(p_fake, self.fake_label, 1.0, slot, True, True)
                D._engine.backward(c_real, dp_real, False, sink)
                D._engine.backward(c_fake, dp_fake, False, sink, on_grads=self._grad_hook(self.opt_D, D))   # the accumulating pass
            self._finish_reduce(self.opt_D, D)            # D's buckets overlap the rest of its own backward
            if self._clip is not None:
                self._clip.clip("D")                      # norm of the reduced gradient; the step below applies the coefficient
            self.opt_D.step(prepared=prep and it == 0)

        # ---- Generator + VAE loss (:110-117) ----
        feat = None
        if self.alpha_feat != 0.0:
            # Dis_l(x): one more ordinary train-mode pass of D on the noisy real batch, after the d_iters updates and BEFORE
            # the pass on the reconstruction (BatchNorm buffers see real, then fake); nothing kept but the tapped activation
            _, _, f_real = D.engine_forward(real_noisy, B, keep=False, tap=self.feat_layer)
            feat = (self.feat_layer, f_real, self.alpha_feat, losses[5:6])
        # prior stream: D sees recon, then prior -- as ONE grouped 2B pass over [recon_noisy | xp_noisy] where that is legal.  The
        # two BCE terms go to different slots (2 and 8), so a grouped pass takes the single-target BCE launches (the fused head
        # launch sums its groups into one slot); separate passes keep one fused launch each.
        group_g = ps and self.group_d_passes and D._engine.can_group(B, 2)
        c_pr = None
        if group_g:
            p_adv, c_adv = D.engine_forward(both[B:], B, groups=2)
        else:
            p_adv, c_adv = D.engine_forward(recon_noisy, B)
            if ps:
                p_pr, c_pr = D.engine_forward(xp_noisy, B)
        if weighted:
            # alpha_pix * L_w: the region-weighted MSE writes slot 0, the holes' own MSE (slot 7) and d_recon in full
            d_recon = ops.region_mse_forward_backward(recon, real, rects, self.hole_weight, self.alpha_pix, losses[0:1],
                                                      losses[7:8], True)
            ops.kl_forward(mulv, lvc, L, float(B), dt, out=losses[1:2])                       # :114
        elif self.merge_small_launches:
            # :113-114: the MSE's final sum rides on the KL launch (same arithmetic as its own one-wave launch)
            d_recon, mse_tail = ops.mse_forward_backward(recon, real, self.alpha_pix, losses[0:1], True, defer_final=True)
            ops.kl_forward(mulv, lvc, L, float(B), dt, out=losses[1:2], mse=mse_tail)
        else:
            d_recon = ops.mse_forward_backward(recon, real, self.alpha_pix, losses[0:1], True)    # :113
            ops.kl_forward(mulv, lvc, L, float(B), dt, out=losses[1:2])                       # :114
        if self.alpha_ssim != 0.0:
            # 1 - SSIM(recon, real) and its gradient, added onto the MSE's in d_recon (which that launch wrote in full, also
            # with alpha_pix = 0)
            if self.ssim_scales is None:
                ops.ssim_loss_forward_backward(recon, real, self.alpha_ssim, losses[6:7], False, d_recon)
            else:
                ops.msssim_loss_forward_backward(recon, real, trainer_scales(self.ssim_scales, *real.shape[2:]),
                                                 self.alpha_ssim, losses[6:7], False, d_recon)
        dp_adv, dp_pr = None, None
        if group_g:
            dp_adv = torch.empty_like(p_adv)                  # [2B]: :115 on the reconstruction's half, the same on the prior's
            ops.bce_forward_backward(p_adv[:B], self.real_label, self.alpha_adv, losses[2:3], False, True, out=dp_adv[:B])
            ops.bce_forward_backward(p_adv[B:], self.real_label, self.alpha_adv, losses[8:9], False, True, out=dp_adv[B:])
        elif not fused_head:
            dp_adv = ops.bce_forward_backward(p_adv, self.real_label, self.alpha_adv, losses[2:3], False, True)  # :115
            if ps:
                dp_pr = ops.bce_forward_backward(p_pr, self.real_label, self.alpha_adv, losses[8:9], False, True)

        # ---- backward of total = a_pix*recon + a_kl*min(1,epoch/50)*kl + a_adv*adv (+ a_feat*feat) (+ a_ssim*ssim), then E and G steps
        # (:131-135) ----
        self.opt_E.zero_grad(memset=False)
        self.opt_G.zero_grad(memset=False)
        head_g = fused_head and not group_g
        d_noisy = D._engine.backward(c_adv, dp_adv, True, sink, param_grads=not self.elide_dead_grads,
                                     head_loss=(self.real_label, 0.0, 1, self.alpha_adv, losses[2:3], False) if head_g else None,
                                     feat=feat)
        if c_pr is not None:
            d_xp = D._engine.backward(c_pr, dp_pr, True, sink, param_grads=not self.elide_dead_grads,
                                      head_loss=(self.real_label, 0.0, 1, self.alpha_adv, losses[8:9], False) if head_g else None)
        if aug is not None:
            d_noisy = aug.backward(d_noisy, self.aug_params, D.nc, dt)      # back to the gradient of the un-augmented batch
            if c_pr is not None:
                d_xp = aug.backward(d_xp, self.aug_params, D.nc, dt)
        if ps:
            # the prior half first, without a hook: through the instance-noise add and Tanh into the backward of the SECOND
            # Generator context (its own saved batch statistics).  It writes the Generator's gradients; the reconstruction's
            # backward below accumulates onto them and carries the bucket hook, so a bucket leaves once, after its last
            # contribution.  Nothing of it reaches the Encoder (z_p is an input).
            if group_g:
                d_noisy, d_xp = d_noisy[:B], d_noisy[B:]
            d_pre_p = ops.nhwc_grad_tanh_to_nhwc(d_xp, x_p, G.padc(Gn.nc, dt), dt)
            Gn._engine.backward(ctxG_p, d_pre_p, False, sink)
        # d total / d recon = d MSE (+ d SSIM) + d adv through the instance-noise add (:92), then through tanh: one pass
        d_pre = ops.nchw_grad_add_to_nhwc(d_recon, d_noisy, recon, G.padc(Gn.nc, dt), dt)
        dz = Gn._engine.backward(ctxG, d_pre, True, sink, on_grads=self._grad_hook(self.opt_G, Gn))
        self._finish_reduce(self.opt_G, Gn, wait=False)       # G's last bucket overlaps the encoder's backward
        kl_w = self.alpha_kl * min(1.0, epoch / 50)                                            # :117
        dmulv = ops.reparam_kl_backward(mulv, lvc, eps_z, dz, kl_w / B, L, dt)
        E._engine.backward(ctxE, dmulv.view(B, 1, 1, -1), False, sink, on_grads=self._grad_hook(self.opt_E, E))
        self._finish_reduce(self.opt_E, E, also_wait=(self.opt_G,))
        if self._clip is not None:
            self._clip.clip("E", "G")                         # one call for both, each against its own norm
        if prep and self.merge_small_launches:
            self.opt_E.step_pair(self.opt_G)                  # :134-135 in one launch (both prepared by the prologue)
        else:
            self.opt_E.step(prepared=prep)
            self.opt_G.step(prepared=prep)
        if self.ema is not None:
            self.ema.update()                                 # the shadows follow the weights this iteration left
        self.losses = losses
        return losses

    # ---- hipGraph replay of the whole iteration -------------------------------------------------------------
    def graph_input(self):
        """The static image buffer the captured iteration reads ([B, C, H, W] f32), or None before a capture.  A loader
        that assembles its batches straight into it (data.DeviceLoader.bind_output) hands them to train_step_graphed
        without the device-to-device copy; pass the SAME tensor as `real`."""
        return None if self._graph is None else self._graph.sin[0]

    def graph_noisy_input(self):
        """The static `noisy` buffer of a captured PAIRED iteration ([B, C, H, W] f32), or None (no capture, or an unpaired
        one).  data.DeviceLoader.bind_noisy assembles batches straight into it; pass the SAME tensor as `noisy`."""
        return None if self._graph is None or len(self._graph.sin) < 6 else self._graph.sin[4]

    def graph_rects_input(self):
        """The static rectangle buffer of a captured paired iteration (f32 [B, 8]), or None; copy a batch's
        DeviceLoader.last_rects into it (or pass it as it is: it is copied) and pass the SAME tensor as `rects`."""
        return None if self._graph is None or len(self._graph.sin) < 6 else self._graph.sin[5]

    def train_step_graphed(self, real: torch.Tensor, epoch: int, eps_z: Optional[torch.Tensor] = None,
                           eps_real: Optional[torch.Tensor] = None,
                           eps_recon: Optional[torch.Tensor] = None, *, noisy: Optional[torch.Tensor] = None,
                           noisy_nhwc: Optional[torch.Tensor] = None, rects: Optional[torch.Tensor] = None,
                           eps_prior: Optional[torch.Tensor] = None, eps_xp: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Same iteration as train_step, replayed from captured hipGraphs (~220 kernel launches become one graph
        launch per segment).  The returned tensor is the graph's STATIC output buffer: the next call overwrites it
        (clone it to keep a history of losses).  Every call performs exactly one training iteration: the first call with a new
        (shape, KL weight, noise mode) runs eagerly (it also sizes the workspaces), the second captures and
        replays, later calls replay.  Inputs are copied into static buffers; noise is either injected on every
        call or drawn on the device inside the graph (torch's graph-safe Philox state).
        With a gradient reducer the iteration is captured as SEGMENTS that share one memory pool, cut at the points
        where gradients are handed to the reducer (one cut per gradient bucket, ddp.py) and, in SyncBN mode, at every
        BatchNorm's statistics all-reduce; the collectives run eagerly between the segment replays.
        noisy / rects: the paired step (train_step); both become static inputs (graph_noisy_input, graph_rects_input) and the
        captured iteration converts the static NCHW `noisy` itself: noisy_nhwc is eager-only (ValueError).
        prior_stream=True: the injected form takes eps_prior and eps_xp as well (all five tensors or none); they become two
        more static inputs."""
        if noisy_nhwc is not None:
            raise ValueError("train_step_graphed: noisy_nhwc is eager-only (the captured step converts its static noisy input)")
        if noisy is None and rects is not None:
            raise ValueError("rects belongs to the paired step: pass noisy= as well")
        if noisy is not None:
            if not real.is_cuda or real.dtype != torch.float32:
                raise RuntimeError("train_step_graphed: the paired step needs a device f32 batch")
            self._check_pair(real, noisy, None, rects)          # also on a replay, whose copies would convert silently
        inject = eps_z is not None
        if inject and (eps_real is None or eps_recon is None):
            raise ValueError("inject all three noise tensors or none")
        ps = self.prior_stream
        if not ps and (eps_prior is not None or eps_xp is not None):
            raise ValueError("eps_prior / eps_xp belong to the prior stream: build the trainer with prior_stream=True")
        if ps and ((eps_prior is not None) != inject or (eps_xp is not None) != inject):
            raise ValueError("prior_stream: inject all five noise tensors (eps_z, eps_real, eps_recon, eps_prior, eps_xp) or none")
        if not inject or self.augment is not None:
            self._noise_stream(real.device)         # exists (and is keyed on the current seed) before the key is formed
        key = self._capture_key(real, epoch, inject, noisy is not None, rects is not None)
        g = self._graph
        if g is not None and g.key == key:
            sin = g.sin
            if real.data_ptr() != sin[0].data_ptr():    # a batch assembled in graph_input() needs no copy
                sin[0].copy_(real)
            if inject:
                sin[1].copy_(eps_z), sin[2].copy_(eps_real), sin[3].copy_(eps_recon)
            if noisy is not None:
                if noisy.data_ptr() != sin[4].data_ptr():
                    sin[4].copy_(noisy)
                if rects is not None and rects.data_ptr() != sin[5].data_ptr():
                    sin[5].copy_(rects)
            if ps and inject:
                sin[6].copy_(eps_prior), sin[7].copy_(eps_xp)
            self._replay(g)
            self.last_step_weighted = self._weighted(noisy, rects)
            self.losses = g.out
            return g.out
        if self._warm_key != key:
            self._warm_key = key
            self._graph = None
            return self.train_step(real, epoch, eps_z, eps_real, eps_recon, noisy=noisy, rects=rects, eps_prior=eps_prior,
                                   eps_xp=eps_xp)
        sin = [real.clone()] + ([eps_z.clone(), eps_real.clone(), eps_recon.clone()] if inject else [None] * 3)
        if noisy is not None or (ps and inject):
            sin += [None if noisy is None else noisy.clone(), None if rects is None else rects.clone()]
        if ps and inject:                           # entries 6, 7; 4 and 5 stay the paired step's (None when unpaired)
            sin += [eps_prior.clone(), eps_xp.clone()]
        # Collectives INSIDE the graph (round 4): RCCL's all-reduces are capturable on this stack (PyTorch 2.10 / RCCL 2.26:
        # tools/rccl_capture_probe.py) -- the asynchronous bucket launches fork onto RCCL's stream and the waits join it
        # back, all as graph dependencies, so the iteration stays ONE graph and no hand-off costs a graph boundary (a cut
        # is ~29 us of idle GPU, 5 per iteration: DESIGN.md section 7).  Reducers that cannot be captured (gloo: host-side
        # work) keep the segmented form; if the inline capture fails on some stack the segmented one is tried next.
        inline = self.reducer is not None and bool(getattr(self.reducer, "capturable", False)) and not self._inline_failed
        try:
            g = self._capture(key, sin, epoch, inline)
        except Exception as ex:                     # noqa: BLE001
            if not inline:
                raise
            import sys
            print(f"[vaegan_amd] capturing the gradient collectives inside the hipGraph failed ({ex!r}); "
                  f"falling back to graph segments cut at the collectives", file=sys.stderr)
            self._inline_failed = True
            g = self._capture(key, sin, epoch, False)
        self._graph = g
        self._replay(g)
        self.last_step_weighted = self._weighted(noisy, rects)
        self.losses = g.out
        return g.out

    def _replay(self, g) -> None:
        replay(g)
        if self.ema is not None:
            self.ema.touch()                        # the replayed update rewrote the shadow buffers: their packs are stale

    def _capture(self, key, sin, epoch, inline):
        """Capture one iteration on the static inputs `sin` (capture.capture).  inline: the reducer's collectives are
        recorded into the graph (one segment, and a replay advances the reducer's counters with the other host mirrors);
        else the graph is cut at every hand-off to the reducer and the collectives run between the segment replays.
        Executes nothing; on failure the trainer is exactly where it was."""
        def quiesce():
            # Nothing of torch.distributed may be in flight while a stream is capturing: c10d's watchdog thread polls
            # unfinished collectives with hipEventQuery, which is illegal next to a capture (the abort recorded in round
            # 1).  Structural guard rather than luck: wait for every collective this trainer launched and REFUSE to
            # capture if the reducer still reports outstanding work (capture.capture then drains the device).
            if self.reducer is not None and hasattr(self.reducer, "drain"):
                self.reducer.drain()
            if self.reducer is not None and getattr(self.reducer, "outstanding", lambda: 0)() != 0:
                raise CaptureRefused("hipGraph capture refused: the gradient reducer still has collectives in flight")
            if inline:
                # Collectives recorded INSIDE the graph put RCCL's stream into the capture.  c10d's watchdog keeps every
                # eagerly launched collective (the warm-up iteration's) in its list until its next pass (one every 100 ms)
                # finds it complete, and asks with hipEventQuery; a pass that falls into the capture asks about end events
                # that sit on RCCL's stream, which HIP answers with hipErrorCapturedEvent -- the watchdog then takes the
                # process down.  So: let the device finish what was launched, then give the watchdog time for a pass over
                # work that is all complete, after which its list is empty until the capture has ended (torch enqueues
                # nothing while the current stream is capturing).  Once per capture.
                torch.cuda.synchronize()
                time.sleep(WATCHDOG_PASS_SECONDS)

        def set_cut_hook(cut):                     # inline: _cut runs the collective at once, i.e. records it
            self._cut_hook = None if inline else cut

        mirrors = HostMirrors([m._engine for m in (self.E, self.G, self.D)], (self.opt_E, self.opt_G, self.opt_D),
                              self.reducer, replay_reducer=inline)
        try:
            def step(*s):                           # s = sin: [real, 3 eps][, noisy, rects][, eps_prior, eps_xp]
                kw = dict(noisy=s[4], rects=s[5]) if len(s) > 4 else {}
                if len(s) > 6:
                    kw.update(eps_prior=s[6], eps_xp=s[7])
                return self.train_step(s[0], epoch, *s[1:4], **kw)

            return capture(step, sin, mirrors, sin[0].device, key=key,
                           pool=torch.cuda.graph_pool_handle(), error_mode="thread_local", pre_capture=quiesce,
                           install_cut=set_cut_hook)
        except CaptureRefused:
            raise
        except BaseException:
            if self.reducer is not None and hasattr(self.reducer, "forget_pending"):
                self.reducer.forget_pending()
            self._graph, self._warm_key = None, None
            raise

    # ---- checkpoint / resume ----------------------------------------------------------------------------------
    # The reference only ever writes `decoder.state_dict()` (vaegan_code.py:193; main_vae.py:204-205 also the
    # encoder) and reads such files back with torch.load(weights_only=True) + load_state_dict (main_vae.py:246-249,
    # :356-357).  Module state_dicts here have the reference's keys/shapes/dtypes, so those files
    # interchange both ways.  state_dict()/load_state_dict() below add what the reference lacks: all three networks
    # plus the three Adam states in one payload of plain tensors / dicts / numbers (weights_only-loadable), from
    # which training resumes bit-identically.  With an EMA attached the payload carries "ema" (ema.EMA.state_dict) as well,
    # and only then.  A checkpoint WITHOUT "ema" loaded into a trainer that has an EMA re-initialises the shadows from the
    # loaded live weights; a checkpoint WITH "ema" loaded into a trainer without one ignores it.
    def state_dict(self) -> Dict:
        sd = {"format": 1,
              "encoder": self.E.state_dict(), "decoder": self.G.state_dict(), "discriminator": self.D.state_dict(),
              "opt_E": self.opt_E.state_dict(), "opt_Dec": self.opt_G.state_dict(), "opt_Dis": self.opt_D.state_dict(),
              # generator state of the in-kernel randn_like draws: [seed, iteration counter] (None: never used)
              "noise": None if self.noise is None else self.noise.get_state().cpu()}
        if self.ema is not None:
            sd["ema"] = self.ema.state_dict()
        return sd

    def load_state_dict(self, sd: Dict) -> None:
        if sd.get("format") != 1:
            raise RuntimeError(f"unknown VAE-GAN checkpoint format {sd.get('format')!r}")
        self.E.load_state_dict(sd["encoder"]), self.G.load_state_dict(sd["decoder"])
        self.D.load_state_dict(sd["discriminator"])
        self.opt_E.load_state_dict(sd["opt_E"]), self.opt_G.load_state_dict(sd["opt_Dec"])
        self.opt_D.load_state_dict(sd["opt_Dis"])
        if self.ema is not None:
            if sd.get("ema") is not None:
                self.ema.load_state_dict(sd["ema"])
            else:
                self.ema.reset()
        if sd.get("noise") is not None:
            st = sd["noise"]
            dev = next(self.E.parameters()).device
            if self.noise is None:
                self.noise = ops.NoiseStream(dev, int(st[0]))
                self._graph = None
            self.noise.seed = int(st[0])
            self.noise.set_state(st)
            # The restored stream (its seed AND iteration counter) stays in use although the resuming process's torch
            # seed differs from the saved one (or the saved seed was >= 2^63 and is stored masked): only an explicit
            # re-seed of torch AFTER this point (utils.configure_seed / torch.cuda.manual_seed) starts a new stream.
            self._noise_pinned_seed = torch.cuda.initial_seed()

    def save_checkpoint(self, path: str, **extra) -> None:
        """extra: plain numbers / strings / tensors stored next to the state (e.g. epoch=...)."""
        sd = self.state_dict()
        sd["extra"] = dict(extra)
        torch.save(sd, path)

    def load_checkpoint(self, path: str) -> Dict:
        """Loads with torch.load(weights_only=True) (nothing in the file is executed).  Returns the extras."""
        sd = torch.load(path, map_location=next(self.E.parameters()).device, weights_only=True)
        self.load_state_dict(sd)
        return sd.get("extra", {})

    def loss_dict(self, losses: Optional[torch.Tensor] = None, epoch: Optional[int] = None) -> Dict[str, float]:
        """Host copy of the last step's losses (one device sync, like the reference's .item() calls :125-127)."""
        v = (losses if losses is not None else self.losses)[:9].tolist()
        v += [0.0] * (9 - len(v))                # a caller's five-slot slice; slot 8 exists with the prior stream only
        out = dict(zip(LOSS_NAMES, v))
        if self.alpha_feat != 0.0:
            out["feat_loss"] = v[5]
        if self.alpha_ssim != 0.0:
            out["ssim_loss"] = v[6]
        if self.prior_stream:
            out["g_loss_adv_prior"] = v[8]       # BCE(D(xp_noisy), real_label), unweighted like g_loss_adv
        if self.last_step_weighted:
            out["hole_mse"] = v[7]               # mean squared error inside the occlusion rectangles: only after a step that
                                                 # used the weighted term (slot 7 reads 0 after any other)
        if self._clip is not None:
            out.update(self._clip.report())      # grad_norm_E/G/D, clip_coef_E/G/D of the networks that are configured
        out.update(lr_report(self._clip_opts()))  # lr_E/G/D, the rates of the last step, when any optimizer has a schedule
        if epoch is not None:
            out["total"] = self.alpha_pix * out["recon_loss"] + self.alpha_kl * min(1.0, epoch / 50) * out["kl_loss"] \
                + self.alpha_adv * out["g_loss_adv"] + self.alpha_feat * v[5] + self.alpha_ssim * v[6] \
                + (self.alpha_adv * v[8] if self.prior_stream else 0.0)
        return out
