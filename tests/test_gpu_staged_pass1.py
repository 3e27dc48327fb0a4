"""The Trainer's staged VolSDF pass 1 (render_keep, render_two_draws, _samples: one routine under all three) against a flat, loop-free
restatement from hip.* calls: whole-frame sampler runs for the depths, the four stages on each launch group's slice for the state.
108 rays in launch groups of 32 and sampler batches of 64, so both loop levels end on a ragged tail: 64 + 44, and 32, 32 | 32, 12.
(The sampler's chunk invariance and its two-draws property are held bit for bit in test_gpu_train.py / test_gpu_configs.py.)"""
import inspect

import pytest
import torch

from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
H, W, N = 12, 9, 108
GROUPS = [(0, 32), (32, 64), (64, 96), (96, 108)]


@pytest.fixture(scope="module")
def ctx():
    from types import SimpleNamespace
    from nerfart_amd import hip, rend_util, scene, volsdf
    from nerfart_amd.trainer import Trainer
    model, rk, _ = scene.build_model("VolSDF", seed=0, beta=0.01, device=DEV, precision="mixed")
    c2w, K = scene.camera(H, W)
    o, d, _ = rend_util.get_rays(c2w[None].to(DEV), K[None].to(DEV), H, W)
    o, d = o[0].contiguous(), d[0].contiguous()
    kw = {k: v for k, v in rk.items() if k != "rayschunk"}
    # the arguments as volume_render itself reads them: its signature's defaults under the scene's kwargs
    a = {k: p.default for k, p in inspect.signature(volsdf.volume_render).parameters.items() if p.default is not inspect.Parameter.empty}
    a.update(kw)
    ns, ni = a["N_samples"], a["N_importance"]
    g = torch.Generator().manual_seed(11)
    u = {1: torch.rand(N, ni, generator=g).to(DEV), 2: torch.rand(N, ni, generator=g).to(DEV)}
    tr = Trainer(model, pass2_rays=16, patches_per_launch=2, pass1_groups=2)
    tr.uniform_source = lambda p, first, count, n, dev: u[p][first:first + count, :n]
    assert tr._launch_rays(ns + ni) == 32
    dn = hip.normalize_dirs(d)
    alpha, beta = (float(x.detach()) for x in model.forward_ab())
    sa = model.sampler_args()
    surf_blob, rad_blob = model.packed()

    def depths(u_final):
        fine = hip.volsdf_fine_sample(sa["blob"], o, dn, a["near"], a["far"], a["obj_bounding_radius"], alpha, beta, a["epsilon"], 4 * ns, 4 * ns, ni,
                                      a["max_upsample_steps"], a["max_bisection_steps"], precision=sa["precision"], escalate=sa["escalate"],
                                      guard=sa["guard"], late_round=sa["late_round"], u_final=u_final)[0]
        t = hip.lin_table(ns, DEV)
        coarse = (a["near"] * (1.0 - t) + a["far"] * t)[None, :].expand(N, ns)
        return torch.sort(torch.cat([coarse, fine], dim=-1), dim=-1)[0]

    def group_state(dep, i0, i1):
        """(rgb, depths, sdf, nablas, h7) of rays [i0:i1] at the depths dep[i0:i1]: the four stages, once."""
        dj = dep[i0:i1].contiguous()
        pts, v = hip.ray_points(o[i0:i1], dn[i0:i1], dj)
        sdf, nab, h7 = hip.sdf_nabla_fwd(surf_blob, pts, model.obj_bounding_radius, precision=model.precision_id)
        rad = hip.radiance_fwd(rad_blob, model.view_tiles, pts, v, nab, h7, precision=model.precision_id)
        rgb = hip.volsdf_composite(dj, sdf.reshape(i1 - i0, ns + ni), rad.reshape(i1 - i0, ns + ni, 3), alpha, beta, a["white_bkgd"])[0]
        return rgb, dj, sdf, nab, h7

    dep0, dep1, dep2 = depths(None), depths(u[1]), depths(u[2])
    assert not torch.equal(u[1], u[2]) and not torch.equal(dep1, dep2) and not torch.equal(dep0, dep1)
    return SimpleNamespace(tr=tr, o=o, d=d, dn=dn, kw=kw, dep0=dep0, dep1=dep1, dep2=dep2, group_state=group_state)


def test_two_draws_image_at_the_first_draw_depths_of_the_second(ctx):
    rgb = ctx.tr.render_two_draws(ctx.o, ctx.d, **dict(ctx.kw, perturb=True))
    assert torch.equal(ctx.tr._depths2, ctx.dep2)                  # swapped halves of the sampler's output would fail here
    assert rgb.shape == (N, 3)
    for i0, i1 in GROUPS:
        assert torch.equal(rgb[i0:i1], ctx.group_state(ctx.dep1, i0, i1)[0]), (i0, i1)


def test_kept_state_is_the_stages_on_each_launch_group(ctx):
    rgb = ctx.tr.render_keep(ctx.o, ctx.d, **dict(ctx.kw, perturb=False))
    kept = ctx.tr._kept
    assert [k[0].shape[0] for k in kept] == [32, 32, 32, 12] and rgb.shape == (N, 3)
    for (i0, i1), got in zip(GROUPS, kept):
        ref = ctx.group_state(ctx.dep0, i0, i1)
        assert torch.equal(rgb[i0:i1], ref[0]), (i0, i1)
        for name, x, y in zip(("depths", "sdf", "nablas", "h7"), got, ref[1:]):
            assert x.shape == y.shape and torch.equal(x, y), (name, i0, i1)


def test_pass2_resampling_reads_the_second_draw_of_its_rays(ctx):
    got = ctx.tr._samples(ctx.o[32:], ctx.dn[32:], ctx.d[32:], dict(ctx.kw, perturb=True), pass_no=2, first_ray=32)
    assert torch.equal(got, ctx.dep2[32:])
