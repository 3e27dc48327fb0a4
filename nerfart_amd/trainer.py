"""Fine-tune step (row a19): the two-pass render / back-propagation of the reference Trainer
(models/frameworks/volsdf.py:689-783, :878-939; neus.py:455-576, :629-690).

    pass 1  (no grad)  whole image through the HIP renderer                       -> rgb [1, H*W, 3]
            style loss on the image (CLIP heads, criteria.py)                      -> d loss / d rgb
    pass 2  patches of `pass2_rays` rays (reference: 1200): HIP sampler (no grad, as volsdf.py:479), then the
            differentiable per-sample evaluation + compositing (autodiff.py),
            rgb_patch.backward(d loss / d rgb[patch]); eikonal = w * MSE(|nabla|, 1) over the patch's nablas, backward.
    caller  optimizer.step()  (train.py:247); with N ranks: dist.allreduce_gradients first.

The two passes and `perturb` (volsdf.py:724-728, :759-766, :982; neus.py:520-576, :742): the reference calls its renderer with
`render_kwargs_train` in BOTH passes, and `perturb` defaults to True there - pass 2 draws NEW uniform numbers for the 64 inverse-CDF
samples of every ray and back-propagates d loss / d rgb (evaluated on pass 1's image) through THOSE samples.  This Trainer does the
same: with perturb=True pass 1 keeps no per-point state, pass 2 gets fresh random samples (NeuS: the sampler runs again; VolSDF: see
`share_algorithm1` below) and the ray-level backward re-evaluates the per-point state there (`have_state = 0`).  With perturb=False re-sampling reproduces pass 1's samples exactly
(same weights, deterministic sampler), so pass 1 keeps its depths - and for VolSDF sdf / nablas / h7 - in HBM and pass 2 reads them:
the same numbers for one sampler and one forward evaluation less.  `Trainer(reuse_pass1_samples=True)` asks for that reuse under
perturb=True as well (a deviation: the gradient is then taken at the samples the loss was evaluated on);
`Trainer(resample_pass2=True / False)` forces either behaviour.  VolSDF: pass 2's samples come from pass 1's run of Algorithm 1
(`share_algorithm1`, render_two_draws: the rounds draw nothing and repeat exactly, only the final inverse-CDF reads uniform numbers).

Other differences from the reference, all deliberate: several reference patches share one launch group
(per-patch eikonal means kept); NeuS keeps `radiance_net` frozen exactly like neus.py:455-456.

Stated once each: the render kwargs are read by the framework's own `render_args` (the defaults of ITS volume_render signature, so both passes
sample with the same settings); VolSDF's staged pass 1 is `_volsdf_depths` + `_volsdf_point_state` under the loop of `_staged_pass1` (render_keep,
render_two_draws; `_samples` shares the depths); `_pass1` picks the pass 1 of a step.
"""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import autodiff, hip, neus, volsdf
from . import dist as nd
from .nets import NeuS, VolSDF


_WARNED_AUTOGRAD = False


class Trainer(nn.Module):
    def __init__(self, model, w_eikonal: float = 0.1, use_eikonal: bool = True, pass2_rays: int = 1200, native: bool = None,
                 patches_per_launch: int = 4, freeze_radiance: bool = None, pass1_groups: int = 14, resample_pass2: bool = None,
                 reuse_pass1_samples: bool = False, share_algorithm1: bool = True):
        super().__init__()
        if not isinstance(model, (VolSDF, NeuS)):
            raise TypeError("Trainer expects a nerfart_amd VolSDF or NeuS model")
        self.model = model
        self.is_neus = isinstance(model, NeuS)
        self.w_eikonal, self.use_eikonal, self.pass2_rays = w_eikonal, use_eikonal, pass2_rays
        # native (None = True): pass 2 on the ray-level C entry points (csrc/render_backward.hip).  They read split-bf16 blobs, so a
        # training step on another precision is REFUSED (fp32-exact is an inference precision here) - checked when the step runs,
        # because set_precision may be called after get_model.  native=False is the torch-autograd formulation over library GEMMs:
        # the cross-check the native kernels are tested against, never chosen silently (it warns when it runs).
        self._native = native
        self._style_cfg = None
        # pass 2 draws its own samples (the reference's semantics, volsdf.py:759-766): None = whenever render_kwargs['perturb'] is
        # true (at perturb=False the sampler is deterministic and pass 1's samples ARE what pass 2 would draw: reused);
        # reuse_pass1_samples=True: the explicit opt-in to reuse under perturb=True as well
        if reuse_pass1_samples and resample_pass2:
            raise ValueError("Trainer: reuse_pass1_samples=True contradicts resample_pass2=True")
        self.resample_pass2, self.reuse_pass1_samples = resample_pass2, bool(reuse_pass1_samples)
        # VolSDF, pass 2 re-sampling: ONE run of Algorithm 1 serves both passes.  The weights do not change between the passes, so the
        # reference's second fine_sample call repeats the first one's rounds exactly (volsdf.py:159-285 draw nothing); only the final
        # opacity_invert_cdf_sample (:122-136, :287-300) reads fresh uniform numbers.  The sampler kernels invert a converged ray's CDF at
        # however many numbers they are given, so pass 1 asks for 2 x N_importance per ray: the first half are its own fine samples, the
        # second half pass 2's - bit-identical to a second sampler run with those numbers (tests), 0.37 s less per 480 x 270 step.
        # False: pass 2 runs the sampler again (the cross-check).  NeuS: every up-sampling round draws (neus.py:296): nothing to share.
        self.share_algorithm1 = bool(share_algorithm1)
        self._depths2 = None
        # the uniform numbers of perturb=True: None = torch.rand on the device; a callable (pass_no, first_ray, n_rays, n, device) ->
        # [n_rays, n] lets a test feed the draws the reference made (tests/golden/make_golden_finetune.py records them per pass)
        self.uniform_source = None
        self._global_rays = None          # (this rank's frame-ray indices, rays in the frame) while a ray-sharded step runs
        # native pass 2: this many of the reference's pass2_rays-ray patches share one set of kernel launches (the per-patch
        # eikonal means are kept); bounded by the kernels' 2^21 points per launch
        self.patches_per_launch = patches_per_launch
        # render_keep (VolSDF): pass 1 SAMPLES this many of pass 2's launch groups per set of sampler launches (its rounds each cost
        # a host read; results are chunk-invariant bit for bit); the per-point state is then evaluated group by group into tensors
        # of its own, which pass 2 releases as it consumes them (1 KiB per point: ~1 GB per 4 x 1200-ray group at P = 192).  14 groups =
        # 67,200 rays per sampler batch, about half the fused renderer's 131,072-ray chunk (measured: 4 -> 14 takes 8 ms off a 480 x 270 step)
        self.pass1_groups = max(1, pass1_groups)
        self._kept = None
        # finetune_step(geometry_loss=...): pass 1 also leaves every launch's (depth [n], normals [n, 3], mask [n]) maps here, in ray order; None: not wanted
        self._maps = None
        # neus.py:455-456: NeuS fine-tuning trains only the SDF net (and ln_s); pass freeze_radiance=False for the
        # reconstruction objective (reconstruction_step), which trains everything
        if self.is_neus if freeze_radiance is None else freeze_radiance:
            for p in model.radiance_net.parameters():
                p.requires_grad_(False)

    @property
    def native(self) -> bool:
        """Pass 2 on the hand-written kernels (the default).  The backward entry points and the state render_keep hands them read
        split-bf16 blobs only, so a model at another precision cannot train natively: that is an ERROR (no silent switch to library
        GEMMs), raised every time the flag is read.  Trainer(native=False) selects the autograd cross-check explicitly."""
        if self._native is False:
            global _WARNED_AUTOGRAD
            if not _WARNED_AUTOGRAD:
                _WARNED_AUTOGRAD = True
                warnings.warn("Trainer(native=False): pass 2 runs torch autograd over library GEMMs (the cross-check formulation), "
                              "not the hand-written kernels")
            return False
        if self.model.precision != "bf16x3":
            raise RuntimeError(f"training steps run on the split-bf16 kernels: call model.set_precision('bf16x3') (the model is at "
                               f"{self.model.precision!r}; 'fp32' is an inference precision - nerfart_*_render_bwd reads bf16x3 blobs). "
                               "Trainer(native=False) is the torch-autograd cross-check.")
        return True

    # ---- the losses of the fine-tune objective (the reference loads them in Trainer.__init__, volsdf.py:638-645) -----------------
    def configure_style_loss(self, args, target_hw):
        """Remember the config the style losses are built from; they are built on first use (a render-only run with an
        `is_finetune: True` YAML never loads CLIP / VGG - the reference does)."""
        self._style_cfg = (args, tuple(target_hw))

    def _ensure_style_loss(self):
        if getattr(self, "style_loss", None) is None and self._style_cfg is not None:
            from . import criteria
            args, hw = self._style_cfg
            self.style_loss = criteria.build_style_loss(args, hw, device=next(self.model.parameters()).device)
        return getattr(self, "style_loss", None)

    def _training_sampler(self):
        """A model whose sampler was calibrated for rendering (nets.calibrate_sampler: one-term weights error-compensated against ONE set of weights,
        ~2 s on the host) goes back to `mixed`'s hi + lo sampler before a step renders anything: the weights change every step."""
        m = self.model
        if getattr(m, "sampler_precision", None) == "fp16x1c":
            import warnings
            warnings.warn("Trainer: the model's sampler was calibrated for rendering (calibrate_sampler()); training uses the `mixed` mode's hi + lo "
                          "sampler - call calibrate_sampler() again before rendering with the trained weights")
            m.set_sampler_precision("fp16x2", guard=m.sampler_guard, late_round=m.sampler_late_round)

    def _render_args(self, render_kwargs):
        """The render kwargs as the framework's own volume_render reads them (volsdf / neus.render_args: its defaults, its refusals)."""
        return (neus if self.is_neus else volsdf).render_args(render_kwargs)

    def _ab(self):
        alpha, beta = self.model.forward_ab()
        return float(alpha.detach()), float(beta.detach())

    def resamples(self, render_kwargs) -> bool:
        """Does pass 2 of a fine-tune step with these render kwargs run the sampler again (module docstring)?"""
        if self.reuse_pass1_samples:
            return False
        if self.resample_pass2 is not None:
            return bool(self.resample_pass2)
        return bool(self._render_args(render_kwargs).perturb)

    def shares_algorithm1(self, render_kwargs) -> bool:
        """Pass 2 re-samples AND takes its samples from pass 1's run of Algorithm 1 (render_two_draws): native VolSDF steps."""
        return bool(self.share_algorithm1 and self.resamples(render_kwargs) and not self.is_neus and self._native is not False)

    def _uniform(self, pass_no: int, first_ray: int, n_rays: int, n: int, device):
        if self.uniform_source is not None:
            if self._global_rays is not None:
                # ray-sharded step: this rank's rays are tiles of the frame, not a contiguous block - ask the source for the frame's rows and take
                # the ones this rank holds, so that a sharded step reads exactly the draws of the single-process step
                idx, n_frame = self._global_rays
                u = self.uniform_source(pass_no, 0, n_frame, n, device)
                if tuple(u.shape) != (n_frame, n):
                    raise ValueError(f"uniform_source returned {tuple(u.shape)}, expected {(n_frame, n)}")
                return u.to(device=device, dtype=torch.float32)[idx[first_ray:first_ray + n_rays]].contiguous()
            u = self.uniform_source(pass_no, first_ray, n_rays, n, device)
            if tuple(u.shape) != (n_rays, n):
                raise ValueError(f"uniform_source returned {tuple(u.shape)}, expected {(n_rays, n)}")
            return u.to(device=device, dtype=torch.float32).contiguous()
        return torch.rand(n_rays, n, device=device)

    # ---- pass 1 ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def render_image(self, render_fn, rays_o, rays_d, want_depths: bool = False, **render_kwargs):
        """Pass 1 on the fused renderer.  want_depths: also return the sample depths [N, P] of every ray (with perturb=False and
        unchanged weights pass 2 would re-derive exactly these - it can reuse them)."""
        self._training_sampler()
        kw = dict(render_kwargs)
        kw.pop("rayschunk", None)
        ra = self._render_args(kw)
        if ra.perturb and self.uniform_source is not None:
            n = rays_o.reshape(-1, 3).shape[0]
            kw["uniforms"] = self._uniform(1, 0, n, ra.N_importance, rays_o.device)
        rgb, depth, extras = render_fn(rays_o, rays_d, detailed_output=want_depths, require_nablas=True, calc_normal=True, **kw)
        if self._maps is not None:
            self._maps.append((depth.reshape(-1), extras["normals_volume"].reshape(-1, 3), extras["mask_volume"].reshape(-1)))
        if want_depths:
            d = extras["d_all" if self.is_neus else "d_vals"]
            return rgb, d.reshape(-1, d.shape[-1])
        return rgb

    # ---- pass 2 ---------------------------------------------------------------------------------------
    def _samples(self, o, dn, d_raw, rk, pass_no: int = 2, first_ray: int = 0):
        """Sample depths of a patch (no grad): the HIP sampler.  perturb=True draws the uniform numbers of the inverse-CDF
        samples from torch's generator (a fresh draw per call, as the reference's two passes draw separately)."""
        ra = self._render_args(rk)
        u = self._uniform(pass_no, first_ray, o.shape[0], ra.N_importance, o.device) if ra.perturb else None
        if self.is_neus:
            # the renderer's sampler on its own (its stage entry points: bit-identical depths, no frame rendered to get them)
            return hip.neus_sample(self.model.packed()[0], o, d_raw, precision=self.model.precision_id, u_new=u, **ra.sampler)
        return self._volsdf_depths(o, dn, ra, None if u is None else [u], self._ab())[0]

    def _launch_rays(self, P: int) -> int:
        k = max(1, min(self.patches_per_launch, (1 << 21) // max(self.pass2_rays * P, 1)))
        return self.pass2_rays * k

    # ---- VolSDF's pass 1 stage by stage: THE statement of what pass 2 (nerfart_volsdf_render_bwd) re-derives or is handed ---------
    def _volsdf_depths(self, o, dn, ra, draws, ab):
        """ONE run of Algorithm 1 for a batch of rays (dn: normalised) -> a list of sorted depths [n, P], one per draw: coarse + that draw's fine
        samples.  draws: None (deterministic: one entry) or a list of [n, N_importance] uniform tensors, handed to the sampler side by side (bit-identical
        to a run per draw: tests).  Algorithm 1 runs on the model's sampler blob / precision (set_sampler_precision; it carries no gradient, volsdf.py:479)."""
        sa = self.model.sampler_args()
        ns, ni, k = ra.N_samples, ra.N_importance, len(draws) if draws else 1
        d_fine, _, _ = hip.volsdf_fine_sample(sa["blob"], o, dn, ra.near, ra.far, ra.obj_bounding_radius, ab[0], ab[1], ra.epsilon, 4 * ns, 4 * ns,
                                              k * ni, ra.max_upsample_steps, ra.max_bisection_steps, precision=sa["precision"],
                                              escalate=sa["escalate"], guard=sa["guard"], late_round=sa["late_round"],
                                              u_final=torch.cat(draws, dim=1).contiguous() if draws else None)
        t = hip.lin_table(ns, o.device)
        d_coarse = (ra.near * (1.0 - t) + ra.far * t)[None, :].expand(o.shape[0], ns)
        return [torch.sort(torch.cat([d_coarse, d_fine[:, c * ni:(c + 1) * ni]], dim=-1), dim=-1)[0] for c in range(k)]

    def _volsdf_point_state(self, o, dn, depths, ra, ab):
        """One launch group at its depths [R, P] in the fused renderer's order (points, sdf + nabla, radiance, composite) -> (rgb [R, 3], sdf, nablas, h7):
        the state nerfart_volsdf_render_bwd computes for itself with have_state = 0 (dn from hip.normalize_dirs, the kernel it normalises with)."""
        m = self.model
        surf_blob, rad_blob = m.packed()
        pts, v = hip.ray_points(o, dn, depths)
        sdf, nab, h7 = hip.sdf_nabla_fwd(surf_blob, pts, m.obj_bounding_radius, precision=m.precision_id)
        rgb_pt = hip.radiance_fwd(rad_blob, m.view_tiles, pts, v, nab, h7, precision=m.precision_id)
        if self._maps is not None:                             # the geometry maps from the same composite call (its normals output)
            rgb, depth, acc, normals = hip.volsdf_composite(depths, sdf.reshape(-1, ra.P), rgb_pt.reshape(-1, ra.P, 3), ab[0], ab[1], ra.white_bkgd,
                                                            nabla=nab.reshape(-1, ra.P, 3))
            self._maps.append((depth, normals, acc))
            return rgb, sdf, nab, h7
        rgb, _, _ = hip.volsdf_composite(depths, sdf.reshape(-1, ra.P), rgb_pt.reshape(-1, ra.P, 3), ab[0], ab[1], ra.white_bkgd)
        return rgb, sdf, nab, h7

    def _staged_pass1(self, rays_o, rays_d, rk, two_draws: bool):
        """VolSDF's pass 1 on the stages above -> rgb [N, 3]: one set of sampler launches per pass1_groups of pass 2's launch groups, the per-point state
        group by group.  two_draws False: every group's (depths, sdf, nablas, h7) is left in self._kept; True: the sampler gets pass 1's and pass 2's
        draw, the image is evaluated at the first, the state is dropped and the depths of the second are left in self._depths2 [N, P]."""
        ra = self._render_args(rk)                            # refuses what volume_render refuses
        o, d_raw = (r.reshape(-1, 3).float().contiguous() for r in (rays_o, rays_d))
        ab = self._ab()
        step = self._launch_rays(ra.P)
        big = step * self.pass1_groups
        draw_passes = (1, 2) if two_draws else (1,) if ra.perturb else ()     # whose uniform numbers the sampler is handed
        kept, rgbs, deps2 = [], [], []
        for i in range(0, o.shape[0], big):
            oi, dn = o[i:i + big], hip.normalize_dirs(d_raw[i:i + big])
            draws = [self._uniform(p, i, oi.shape[0], ra.N_importance, o.device) for p in draw_passes]
            deps = self._volsdf_depths(oi, dn, ra, draws, ab)
            deps2 += deps[1:]
            for j in range(0, oi.shape[0], step):                 # pass 2's launch groups: their OWN tensors, freed group by group
                dj = deps[0][j:j + step].contiguous()
                rgb, sdf, nab, h7 = self._volsdf_point_state(oi[j:j + step], dn[j:j + step], dj, ra, ab)
                rgbs.append(rgb)
                if not two_draws:
                    kept.append((dj, sdf, nab, h7))
                del sdf, nab, h7
        if two_draws:
            self._depths2 = torch.cat(deps2, 0) if deps2 else torch.zeros(0, ra.P, device=o.device)
        else:
            self._kept = kept
        return torch.cat(rgbs, 0) if rgbs else torch.zeros(0, 3, device=o.device)

    @torch.no_grad()
    def render_keep(self, rays_o, rays_d, **rk):
        """Pass 1 of the native fine-tune step with state kept for pass 2.  VolSDF: on the per-stage C-ABI entries in the fused renderer's order (sampler,
        k_sdf_grad, radiance, composite), KEEPING every launch group's sample depths, sdf, nablas and layer-7 activations
        (1 KiB / point in HBM) for pass 2: the weights do not change between the passes and perturb=False is
        deterministic, so pass 2 would recompute exactly these.  Returns rgb [N, 3]; the state waits in self._kept."""
        self._training_sampler()
        m = self.model
        if m.precision != "bf16x3":
            raise RuntimeError("render_keep keeps split-bf16 pass-1 state for the native pass 2: set_precision('bf16x3') first")
        if not self.is_neus:
            return self._staged_pass1(rays_o, rays_d, rk, two_draws=False)
        # NeuS: the fused renderer's detailed outputs already hold what pass 2 needs at the P samples (depths, sdf,
        # nablas); the mid-point quantities are re-evaluated in pass 2
        ra = self._render_args(rk)
        o, d_raw = (r.reshape(-1, 3).float().contiguous() for r in (rays_o, rays_d))
        step = self._launch_rays(ra.P)
        s_val = float(m.forward_s().detach())
        kept, rgbs = [], []
        for i in range(0, o.shape[0], step):
            oi, di = o[i:i + step], d_raw[i:i + step]
            out = hip.neus_render(*m.packed(), m.view_tiles, oi, di, s=s_val, white_bkgd=ra.white_bkgd, calc_normal=False, detailed=True,
                                  precision=m.precision_id, **ra.sampler,
                                  u_new=self._uniform(1, i, oi.shape[0], ra.N_importance, o.device) if ra.perturb else None)
            kept.append((out["d_all"], out["implicit_surface"].reshape(-1), out["implicit_nablas"].reshape(-1, 3), None))
            rgbs.append(out["rgb"])
        self._kept = kept
        return torch.cat(rgbs, 0) if rgbs else torch.zeros(0, 3, device=o.device)

    @torch.no_grad()
    def render_two_draws(self, rays_o, rays_d, **rk):
        """Pass 1 of a VolSDF fine-tune step whose pass 2 draws its own samples (perturb=True), with Algorithm 1 run ONCE: every batch of rays
        goes through the sampler with 2 x N_importance uniform numbers per ray - columns 0.. are pass 1's draw, N_importance.. pass 2's.
        Pass 1's image is evaluated at the first set (sdf + nabla, radiance, composite: the fused renderer's stages, nothing kept); the
        depths of the second set wait in self._depths2 [N, P] for backward_patches(depths_all=...), whose nerfart_volsdf_render_bwd
        (have_state = 0) evaluates the per-point state there.  Returns rgb [N, 3]."""
        self._training_sampler()
        if self.is_neus:
            raise RuntimeError("render_two_draws: VolSDF only (NeuS draws in every up-sampling round)")
        if self.model.precision != "bf16x3":
            raise RuntimeError("render_two_draws feeds the native pass 2: set_precision('mixed') or ('bf16x3') first")
        return self._staged_pass1(rays_o, rays_d, rk, two_draws=True)

    def backward_patches(self, rays_o, rays_d, gradient, depths_all=None, kept=None, gradient_depth=None, gradient_normals=None, gradient_mask=None,
                         **render_kwargs):
        """Pass 2: accumulates parameter gradients for d loss / d rgb = `gradient` [N, 3] (+ the eikonal term).
        depths_all [N, P]: sample depths from pass 1 (skips the re-sampling); kept: render_keep's per-group state of
        exactly these rays (skips the SDF re-evaluation too).  Returns the mean eikonal loss over the reference's
        pass2_rays-ray patches (what the reference prints).
        gradient_depth [N] / gradient_normals [N, 3] / gradient_mask [N]: d loss / d depth_volume, normals_volume, mask_volume - the geometry terms of
        an objective (VolSDF only; native: k_composite_volsdf_geo_bwd inside nerfart_volsdf_render_bwd2, and g_acc).  A depth cotangent on a ray that
        hits nothing is amplified by 1 / (mask_volume + 1e-10), as autograd through the reference amplifies it: weight it with the mask."""
        self._training_sampler()
        o_all = rays_o.reshape(-1, 3).float().contiguous()
        d_all_ = rays_d.reshape(-1, 3).float().contiguous()
        g_all = gradient.reshape(-1, 3)
        N = o_all.shape[0]
        geo = [None if t is None else t.detach().reshape(N, *shp).float() for t, shp in ((gradient_depth, ()), (gradient_normals, (3,)), (gradient_mask, ()))]
        have_geo = any(t is not None for t in geo)
        if have_geo and self.is_neus:
            raise NotImplementedError("backward_patches: gradient_depth / gradient_normals / gradient_mask (the geometry-map cotangents) are "
                                      "implemented for VolSDF only")
        cut = lambda t, a, b: None if t is None else t[a:b].contiguous()
        ra = self._render_args(render_kwargs)
        eik_sum, n = 0.0, 0
        if self.native:
            accum = autodiff.GradAccumulator()                    # raw GEMM results summed over patches, flushed once
            s_val = float(self.model.forward_s().detach()) if self.is_neus else None
            ab = None if self.is_neus else self._ab()
            if kept is not None:
                bounds, i = [], 0
                for grp in kept:
                    bounds.append((i, i + grp[0].shape[0]))
                    i += grp[0].shape[0]
                if i != N:
                    raise ValueError("backward_patches: the kept pass-1 state does not cover these rays")
            else:
                step = self._launch_rays(ra.P)
                bounds = [(i, min(i + step, N)) for i in range(0, N, step)]
            fresh, fresh_lo = None, 0                              # re-sampled depths of the current batch of launch groups
            for gi, (i0, i1) in enumerate(bounds):
                o, d_raw, g = o_all[i0:i1], d_all_[i0:i1], g_all[i0:i1]
                state = None
                if kept is not None:
                    depths, state = kept[gi][0], kept[gi][1:]
                    kept[gi] = None                                # release the group's state as soon as it is consumed
                elif depths_all is not None:
                    depths = depths_all[i0:i1].contiguous()
                else:
                    # pass 2 draws its own samples (volsdf.py:759-766): ONE set of sampler launches per pass1_groups launch groups
                    # (the sampler's rounds each cost a host read; its results do not depend on how rays are chunked)
                    if fresh is None or i1 > fresh_lo + fresh.shape[0]:
                        j1 = bounds[min(gi + self.pass1_groups, len(bounds)) - 1][1]
                        with torch.no_grad():
                            fresh = self._samples(o_all[i0:j1], hip.normalize_dirs(d_all_[i0:j1]), d_all_[i0:j1], render_kwargs, 2, i0)
                        fresh_lo = i0
                    depths = fresh[i0 - fresh_lo:i1 - fresh_lo].contiguous()
                if self.is_neus:
                    eik = autodiff.neus_backward_samples_native(self.model, o, d_raw, depths, g, self.w_eikonal, self.use_eikonal, ra.white_bkgd,
                                                                s_val=s_val, accum=accum, eik_group_rays=self.pass2_rays, state=state)
                else:
                    eik = autodiff.volsdf_backward_samples_native(self.model, o, d_raw, depths, g, self.w_eikonal, self.use_eikonal, ra.white_bkgd,
                                                                  ab=ab, accum=accum, state=state, eik_group_rays=self.pass2_rays,
                                                                  g_depth=cut(geo[0], i0, i1), g_normals=cut(geo[1], i0, i1), g_acc=cut(geo[2], i0, i1))
                eik_sum = eik_sum + eik
                n += -(-(i1 - i0) // self.pass2_rays)
                del state
            accum.flush(self.model)
            return float(eik_sum) / max(n, 1)
        for i in range(0, N, self.pass2_rays):
            o, d_raw = o_all[i:i + self.pass2_rays], d_all_[i:i + self.pass2_rays]
            dn = F.normalize(d_raw, dim=-1)
            with torch.no_grad():
                depths = self._samples(o, dn, d_raw, render_kwargs, 2, i) if depths_all is None else depths_all[i:i + self.pass2_rays].contiguous()
            if have_geo:
                # the native compositor of a GPU run yields rgb only: the maps need the torch formulation of the per-ray stage
                out = autodiff.volsdf_render_samples(self.model, o, dn, depths, white_bkgd=ra.white_bkgd, native_composite=False)
            else:
                fn = autodiff.neus_render_samples if self.is_neus else autodiff.volsdf_render_samples
                out = fn(self.model, o, dn, depths, white_bkgd=ra.white_bkgd)
            tensors, grads = [out["rgb"]], [g_all[i:i + self.pass2_rays]]
            for key, t in zip(("depth_volume", "normals_volume", "mask_volume"), geo):
                if t is not None:
                    tensors.append(out[key]); grads.append(t[i:i + self.pass2_rays])
            if self.use_eikonal:
                # the reference calls rgb.backward(g, retain_graph=True) and then eikonal.backward(): the same sum of
                # gradients from ONE traversal of the (double-backward) graph of the SDF net
                nn_ = out["implicit_nablas"].reshape(-1, 3).norm(dim=-1)
                eik = self.w_eikonal * F.mse_loss(nn_, torch.ones_like(nn_), reduction="mean")
                torch.autograd.backward(tensors + [eik], grads + [torch.ones_like(eik)])
                eik_sum += float(eik.detach())
            else:
                torch.autograd.backward(tensors, grads)
            n += 1
            del out
        return float(eik_sum) / max(n, 1)

    # ---- reconstruction-training branch (volsdf.py:784-824) -------------------------------------
    def reconstruction_step(self, render_fn, rays_o, rays_d, target_rgb, eikonal_points=None, w_eikonal: float = 0.1, optimizer=None,
                            mask_ignore=None, target_mask=None, w_mask: float = 0.0, **render_kwargs):
        """One step of the reconstruction objective on a batch of rays [N, 3].  Accumulates .grad; returns the losses.

        VolSDF (volsdf.py:784-824): mean |rgb - target| + w_eikonal * MSE(|nabla|, 1) over two nablas per ray - the sample
        of largest visibility weight and `eikonal_points` [N, 3] (the reference draws them uniformly in the bounding box,
        volsdf.py:799-801; here the caller does, so that runs are reproducible).
        NeuS (neus.py:578-617): |rgb - target| (masked mean over target_mask if given: `with_mask`) + w_eikonal * MSE over
        the nablas of ALL samples + w_mask * BCE(clamp(mask_volume, 1e-3, 1 - 1e-3), target_mask); the radiance net trains
        if its parameters require grad."""
        self._training_sampler()
        if self.is_neus:
            return self._reconstruction_step_neus(render_fn, rays_o, rays_d, target_rgb, w_eikonal, optimizer, mask_ignore, target_mask,
                                                  w_mask, **render_kwargs)
        if eikonal_points is None:
            raise ValueError("reconstruction_step (VolSDF) needs eikonal_points [N, 3]")
        m = self.model
        o = rays_o.reshape(-1, 3).float().contiguous()
        d = rays_d.reshape(-1, 3).float().contiguous()
        N = o.shape[0]
        kw = {k: v for k, v in render_kwargs.items() if k != "rayschunk"}
        white = self._render_args(kw).white_bkgd
        with torch.no_grad():
            rgb, _, ex = render_fn(o[None], d[None], detailed_output=True, require_nablas=True, calc_normal=True, **kw)
            rgb = rgb.reshape(N, 3)
            depths = ex["d_vals"].reshape(N, -1)
            P = depths.shape[1]
            nab = ex["implicit_nablas"].reshape(N, P, 3)
            ind = ex["visibility_weights"].reshape(N, P - 1).argmax(dim=-1)                     # [N]
            n_sel = nab[torch.arange(N, device=o.device), ind]                                    # [N, 3]
            surf_blob, _ = m.packed()
            _, n_eik, _ = hip.sdf_nabla_fwd(surf_blob, eikonal_points.reshape(-1, 3).float().contiguous(), 0.0, want_h7=False,
                                            precision=m.precision_id)
            # losses and their cotangents
            diff = rgb - target_rgb.reshape(N, 3)
            if mask_ignore is not None:
                mk = mask_ignore.reshape(N, 1).float()
                loss_img = (diff.abs() * mk).sum() / (mk.sum() + 1e-10)
                g_rgb = torch.sign(diff) * mk / (mk.sum() + 1e-10)
            else:
                loss_img = diff.abs().mean()
                g_rgb = torch.sign(diff) / diff.numel()
            nn_all = torch.cat([n_sel.norm(dim=-1), n_eik.norm(dim=-1)])
            loss_eik = w_eikonal * ((nn_all - 1.0) ** 2).mean()
            coef = w_eikonal * 2.0 / nn_all.numel()
            g_sel = coef * ((n_sel.norm(dim=-1) - 1.0) / n_sel.norm(dim=-1))[:, None] * n_sel
            g_eik = coef * ((n_eik.norm(dim=-1) - 1.0) / n_eik.norm(dim=-1))[:, None] * n_eik
            nbar_extra = torch.zeros(N, P, 3, device=o.device)
            nbar_extra[torch.arange(N, device=o.device), ind] = g_sel
        if optimizer is not None:
            optimizer.zero_grad()
        dn = F.normalize(d, dim=-1)
        if self.native:
            ab = self._ab()
            accum = autodiff.GradAccumulator()
            for i in range(0, N, self.pass2_rays):
                sl = slice(i, i + self.pass2_rays)
                autodiff.volsdf_backward_samples_native(m, o[sl], d[sl], depths[sl].contiguous(), g_rgb[sl], use_eikonal=False,
                                                        white_bkgd=white, ab=ab, nbar_extra=nbar_extra[sl], accum=accum)
            with torch.no_grad():
                autodiff.surface_param_backward(m, eikonal_points.reshape(-1, 3).float().contiguous(), g_eik.contiguous(), accum=accum)
            accum.flush(m)
        else:
            for i in range(0, N, self.pass2_rays):
                sl = slice(i, i + self.pass2_rays)
                out = autodiff.volsdf_render_samples(m, o[sl], dn[sl], depths[sl].contiguous(), white_bkgd=white)
                torch.autograd.backward([out["rgb"], out["implicit_nablas"]], [g_rgb[sl], nbar_extra[sl]])
            _, nab_e, _ = autodiff.surface_forward_with_nablas(m.implicit_surface, eikonal_points.reshape(-1, 3).float())
            nab_e.backward(g_eik)
        return {"loss_img": float(loss_img), "loss_eikonal": float(loss_eik), "total": float(loss_img + loss_eik)}

    def _reconstruction_step_neus(self, render_fn, rays_o, rays_d, target_rgb, w_eikonal, optimizer, mask_ignore, target_mask, w_mask,
                                  **render_kwargs):
        m = self.model
        o = rays_o.reshape(-1, 3).float().contiguous()
        d = rays_d.reshape(-1, 3).float().contiguous()
        N = o.shape[0]
        kw = {k: v for k, v in render_kwargs.items() if k != "rayschunk"}
        white = self._render_args(kw).white_bkgd
        with torch.no_grad():
            rgb, _, ex = render_fn(o[None], d[None], detailed_output=True, calc_normal=False, **kw)
            rgb = rgb.reshape(N, 3)
            depths = ex["d_all"].reshape(N, -1).contiguous()
            P = depths.shape[1]
            acc = ex["mask_volume"].reshape(N)
            nn_ = ex["implicit_nablas"].reshape(N * P, 3).norm(dim=-1)
            loss_eik = w_eikonal * ((nn_ - 1.0) ** 2).mean()
            diff = rgb - target_rgb.reshape(N, 3)
            g_acc, loss_mask = None, torch.zeros((), device=o.device)
            weight = None                                             # per-ray weights of the masked image loss (neus.py:600-611)
            if target_mask is not None:
                tm = target_mask.reshape(N).float()
                mv = torch.clamp(acc, 1e-3, 1.0 - 1e-3)
                loss_mask = w_mask * F.binary_cross_entropy(mv, tm, reduction="mean")
                inside = ((acc > 1e-3) & (acc < 1.0 - 1e-3)).float()  # clamp passes no gradient outside
                g_acc = (w_mask / N) * (-(tm / mv) + (1.0 - tm) / (1.0 - mv)) * inside
                weight = tm if mask_ignore is None else tm * mask_ignore.reshape(N).float()
            elif mask_ignore is not None:
                weight = mask_ignore.reshape(N).float()
            if weight is not None:
                loss_img = (diff.abs() * weight[:, None]).sum() / (weight.sum() + 1e-10)
                g_rgb = torch.sign(diff) * weight[:, None] / (weight.sum() + 1e-10)
            else:
                loss_img = diff.abs().mean()
                g_rgb = torch.sign(diff) / diff.numel()
        if optimizer is not None:
            optimizer.zero_grad()
        dn = F.normalize(d, dim=-1)
        if self.native:
            if N * P > (1 << 21):
                raise ValueError("reconstruction_step (NeuS): at most 2^21 sample points per step (the eikonal mean spans the batch)")
            autodiff.neus_backward_samples_native(m, o, d, depths, g_rgb, w_eikonal, True, white, g_acc=g_acc)
        else:
            out = autodiff.neus_render_samples(m, o, dn, depths, white_bkgd=white, calc_normal=False)
            nn_g = out["implicit_nablas"].reshape(-1, 3).norm(dim=-1)
            eik = w_eikonal * F.mse_loss(nn_g, torch.ones_like(nn_g), reduction="mean")
            tensors, grads = [out["rgb"], eik], [g_rgb, torch.ones_like(eik)]
            if g_acc is not None:
                tensors.append(out["mask_volume"]); grads.append(g_acc)
            torch.autograd.backward(tensors, grads)
        out = {"loss_img": float(loss_img), "loss_eikonal": float(loss_eik), "total": float(loss_img + loss_eik + loss_mask)}
        if target_mask is not None:
            out["loss_mask"] = float(loss_mask)
        return out

    # ---- the reference's call shape (train.py:232) --------------------------------------------------------------
    def forward(self, args, indices, model_input, ground_truth, render_kwargs_train: dict, it: int, optimizer=None, render_fn=None,
                style_loss=None):
        """`trainer.forward(args, indices, model_input, ground_truth, render_kwargs_train, it, optimizer=optimizer)` as train.py
        calls it (volsdf.py:689-877, neus.py:458-627): rays of the batch's camera (all H x W in order when fine-tuning,
        args.data.N_rays random ones otherwise), the targets gathered at them, then

        * `args.training.is_finetune`: `finetune_step` - gradients are in `.grad` on return (the reference back-propagates
          inside forward too) and `losses` is the style loss (a tensor);
        * otherwise `reconstruction_step`.  train.py calls `optimizer.zero_grad(); losses['total'].backward()` AFTER forward, so
          the native pass 2 is deferred into that backward call (`_DeferredBackward`): `losses` holds loss_img, loss_eikonal
          (loss_mask), total as tensors, and `total.backward()` accumulates the gradients.

        Returns OrderedDict(losses=..., extras={'scalars': {...}, 'select_inds': ...}).  `render_fn` defaults to `self.render_fn`;
        `style_loss` to `self.style_loss`, which get_model configures from the YAML (built on first use: the reference builds its
        losses in __init__, volsdf.py:638-645)."""
        from collections import OrderedDict
        from . import rend_util
        render_fn = render_fn if render_fn is not None else getattr(self, "render_fn", None)
        style_loss = style_loss if style_loss is not None else (self._ensure_style_loss() if bool(args.training.is_finetune) else None)
        if render_fn is None:
            raise ValueError("Trainer.forward: set trainer.render_fn (the render_fn get_model returned) or pass render_fn=")
        dev = next(self.model.parameters()).device
        intrinsics, c2w = model_input["intrinsics"].to(dev), model_input["c2w"].to(dev)
        H, W = render_kwargs_train["H"], render_kwargs_train["W"]
        finetune = bool(args.training.is_finetune)
        rays_o, rays_d, select_inds = rend_util.get_rays(c2w, intrinsics, H, W, -1 if finetune else args.data.N_rays)
        target_rgb = torch.gather(ground_truth["rgb"].to(dev), 1, torch.stack(3 * [select_inds], -1))
        mask_ignore = torch.gather(model_input["mask_ignore"].to(dev), 1, select_inds) if "mask_ignore" in model_input else None
        rk = {k: v for k, v in render_kwargs_train.items() if k not in ("H", "W")}
        if finetune:
            if style_loss is None:
                raise ValueError("Trainer.forward (fine-tune): no style loss - get_model(args, [H, W]) configures it from the YAML when "
                                 "training.is_finetune; otherwise set trainer.style_loss (criteria.StyleLoss) or pass style_loss=")
            self.w_eikonal, self.use_eikonal = args.finetune.w_eikonal, bool(args.finetune.use_eikonal)
            out = self.finetune_step(render_fn, rays_o, rays_d, target_rgb, H, style_loss, optimizer=optimizer, **rk)
            losses = torch.tensor(out["loss"], device=dev)
        else:
            kwargs = dict(w_eikonal=args.training.w_eikonal, mask_ignore=mask_ignore)
            if self.is_neus:
                if args.training.get("with_mask", False):
                    kwargs.update(target_mask=torch.gather(model_input["object_mask"].to(dev), 1, select_inds), w_mask=args.training.w_mask)
            else:
                R = args.model.obj_bounding_radius
                kwargs["eikonal_points"] = torch.empty(rays_o.shape[-2], 3, device=dev).uniform_(-R, R)       # volsdf.py:799-801
            losses = _DeferredBackward.run(self, render_fn, rays_o, rays_d, target_rgb, kwargs, rk)
        extras = {"select_inds": select_inds}
        if self.is_neus:
            extras["scalars"] = {"1/s": 1.0 / self.model.forward_s().data}
        else:
            alpha, beta = self.model.forward_ab()
            extras["scalars"] = {"beta": beta.data, "alpha": alpha.data}
        return OrderedDict([("losses", losses), ("extras", extras)])

    def _pass1(self, render_fn, rays_o, rays_d, keep: bool, share: bool, resample: bool, **rk):
        """Pass 1 of a fine-tune step -> (rgb [N, 3], the depths [N, P] pass 2 is to use or None).  keep: state left in self._kept; share: pass 2's depths
        from pass 1's run of Algorithm 1; otherwise the fused renderer - resample: nothing kept, pass 2 samples again; else its depths."""
        if keep:
            return self.render_keep(rays_o, rays_d, **rk), None
        if share:
            return self.render_two_draws(rays_o, rays_d, **rk), self._depths2
        if resample:
            return self.render_image(render_fn, rays_o, rays_d, **rk).reshape(-1, 3), None
        rgb, depths = self.render_image(render_fn, rays_o, rays_d, want_depths=True, **rk)
        return rgb.reshape(-1, 3), depths

    # ---- one fine-tune step ---------------------------------------------------------------------------
    def finetune_step(self, render_fn, rays_o, rays_d, target_rgb, H: int, style_loss, optimizer=None, tile: int = None, geometry_loss=None,
                      **render_kwargs):
        """style_loss(rgb_pred [B,3,H,W], rgb_gt [B,3,H,W]) -> scalar.  Returns dict(loss, eikonal, rgb).

        geometry_loss (VolSDF, single process): a callable that gets pass 1's maps as leaf tensors - {"depth": [1,1,H,W], "normals": [1,3,H,W],
        "mask": [1,1,H,W]} - and returns a scalar that is added to the style loss (depth preservation, normal consistency, smoothness ...); the maps'
        .grad go to backward_patches(gradient_depth=, gradient_normals=, gradient_mask=) and the returned dict gains "geometry".  The depth of a ray
        that hits nothing is a quotient by mask + 1e-10 and its cotangent is amplified accordingly: weight depth terms with the mask.  None: the step
        is exactly the step without this argument.

        With torch.distributed initialised (one process per GPU) the step is ray-parallel: pass 1
        renders this rank's tiles and all-gathers the image; every rank evaluates the (cheap, deterministic) style
        loss on the full image and keeps its own rays' d loss / d rgb; pass 2 runs on its own rays; one flat
        all-reduce(SUM) of the gradients before the caller's optimizer.step().
        tile (rays dealt to a rank at a time) defaults to pass2_rays: every rank then owns WHOLE patches of the single-process
        step's patch grid, the per-patch eikonal means coincide and the all-reduced gradients equal the single-GPU step's up to
        summation order."""
        self._training_sampler()
        sharded = nd.world_size() > 1
        tile = self.pass2_rays if tile is None else tile
        resample = self.resamples(render_kwargs)           # pass 2 draws its own samples (the reference under perturb=True)
        keep = self.native and not resample                # pass 1 keeps its per-point state for pass 2 (render_keep)
        share = self.shares_algorithm1(render_kwargs)      # ... from the SAME run of Algorithm 1 (VolSDF: render_two_draws)
        self._kept = self._depths2 = self._maps = None
        if geometry_loss is not None:
            if self.is_neus:
                raise NotImplementedError("finetune_step: geometry_loss (losses on the depth / normals / mask maps) is implemented for VolSDF only")
            if sharded:
                raise NotImplementedError("finetune_step: geometry_loss is not implemented for the ray-sharded step (torch.distributed)")
            self._maps = []
        if sharded:
            kw = {k: v for k, v in render_kwargs.items() if k != "rayschunk"}
            n_frame = rays_o.reshape(-1, 3).shape[0]
            self._global_rays = (nd.shard_plan(n_frame, tile, rays_o.device).idx, n_frame)
            def fn(ro, rd, **kw_):
                kw_ = {k: v for k, v in kw_.items() if k not in ("detailed_output", "require_nablas", "calc_normal")}
                # a rank that neither keeps nor shares renders WITHOUT keeping depths (resample=True): its pass 2 samples again
                r = self._pass1(render_fn, ro, rd, keep, share, True, **kw_)[0]
                return r, None, {"rgb": r[None]}
            rgb = nd.render_sharded(fn, rays_o.reshape(1, -1, 3), rays_d.reshape(1, -1, 3), keys=("rgb",), tile=tile,
                                    detailed_output=False, require_nablas=True, calc_normal=True, **kw)["rgb"]
            depths_all = self._depths2
        else:
            rgb, depths_all = self._pass1(render_fn, rays_o, rays_d, keep, share, resample, **render_kwargs)
        rgb = rgb.detach().reshape(1, -1, 3).requires_grad_(True)
        W = rgb.shape[1] // H
        to_img = lambda t: t.reshape(t.shape[0], H, W, 3).permute(0, 3, 1, 2)          # "B (H W) C -> B C H W"
        loss = style_loss(to_img(rgb), to_img(target_rgb.reshape(1, -1, 3)))
        geo_grads, geo_value = {}, None
        if geometry_loss is not None:
            maps_in, self._maps = self._maps, None
            to_map = lambda parts, c: torch.cat(parts, 0).detach().reshape(1, H, W, c).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            maps = {"depth": to_map([m[0] for m in maps_in], 1), "normals": to_map([m[1] for m in maps_in], 3), "mask": to_map([m[2] for m in maps_in], 1)}
            geo = geometry_loss(maps)
            geo_value = float(geo.detach())
            loss = loss + geo
        loss.backward()
        gradient = rgb.grad.detach()
        if geometry_loss is not None:
            # a map the loss did not touch has no cotangent: it is not passed on
            flat = lambda t: None if t.grad is None else t.grad.detach().permute(0, 2, 3, 1).reshape(H * W, -1)
            gd, gn, gm = flat(maps["depth"]), flat(maps["normals"]), flat(maps["mask"])
            geo_grads = dict(gradient_depth=None if gd is None else gd.reshape(-1), gradient_normals=gn, gradient_mask=None if gm is None else gm.reshape(-1))
        if optimizer is not None:
            optimizer.zero_grad()
        if sharded:
            idx = nd.shard_plan(rgb.shape[1], tile, rgb.device).idx          # cached per (frame size, tile, world)
            eik = self.backward_patches(rays_o.reshape(-1, 3)[idx], rays_d.reshape(-1, 3)[idx], gradient[0][idx], kept=self._kept,
                                        depths_all=depths_all, **render_kwargs)
            # ranks that own fewer parameters' gradients than others (none here: every rank touches every tensor)
            for p in self.model.parameters():
                if p.requires_grad and p.grad is None:
                    p.grad = torch.zeros_like(p)
            nd.allreduce_gradients([p for p in self.model.parameters() if p.requires_grad])
        else:
            eik = self.backward_patches(rays_o, rays_d, gradient[0], depths_all=depths_all, kept=self._kept, **geo_grads, **render_kwargs)
        self._kept = self._depths2 = self._global_rays = None
        out = {"loss": float(loss.detach()), "eikonal": eik, "rgb": rgb.detach()}
        if geo_value is not None:
            out["geometry"] = geo_value
        return out


class _DeferredBackward(torch.autograd.Function):
    """Hands the gradients of a reconstruction step to whoever back-propagates its total: the reference's train loop calls
    `optimizer.zero_grad(); losses['total'].backward()` AFTER trainer.forward (train.py:240-242), so the step (render, losses,
    native pass 2) runs once in `run`, its gradients are parked, and `total.backward()` adds them to `.grad`."""

    @staticmethod
    def run(trainer, render_fn, rays_o, rays_d, target_rgb, kwargs, rk):
        from collections import OrderedDict
        params = [p for p in trainer.model.parameters()]
        before = [p.grad for p in params]
        for p in params:
            p.grad = None
        parts = trainer.reconstruction_step(render_fn, rays_o, rays_d, target_rgb, **kwargs, **rk)
        step = [p.grad for p in params]
        for p, g in zip(params, before):                           # forward leaves .grad as it found it
            p.grad = g
        dev = rays_o.device
        hook = torch.zeros((), device=dev, requires_grad=True)
        total = _DeferredBackward.apply(hook, torch.tensor(parts["total"], device=dev), params, step)
        losses = OrderedDict((k, torch.tensor(v, device=dev)) for k, v in parts.items() if k != "total")
        losses["total"] = total
        return losses

    @staticmethod
    def forward(ctx, hook, value, params, step):
        ctx.params, ctx.step = params, step
        return value.clone()

    @staticmethod
    def backward(ctx, g_total):
        for p, g in zip(ctx.params, ctx.step):
            if g is not None:
                p.grad = g * g_total if p.grad is None else p.grad + g * g_total
        return None, None, None, None
