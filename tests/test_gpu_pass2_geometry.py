"""Pass 2 with cotangents of the depth, normals and mask maps (Trainer.backward_patches(gradient_depth=, gradient_normals=, gradient_mask=),
Trainer.finetune_step(geometry_loss=)): the native path - k_composite_volsdf_geo_bwd inside nerfart_volsdf_render_bwd2 - against the torch-autograd
formulation, per parameter tensor, with the project's own bounds for these comparisons: 3e-2 native against autograd
(tests/test_gpu_train.py::test_native_pass2_*), 2e-3 for the same estimator in another summation order (test_pass1_state_reuse_matches_recompute).
The sphere-initialised synthetic model, 32 + 64 = 96 points per ray; cotangents are 1e-2 rand from a seeded generator, zeroed on the rays whose
pass-1 mask_volume is below 0.5 (a depth cotangent on an empty ray is amplified by 1 / (mask + 1e-10) in both formulations: nothing to compare).

The rays end at far = 4.0: behind the object (radius 1, camera at 2.5) and inside VolSDF's bounding sphere (radius 3).  With the scene's far = 6.0
every ray leaves that sphere, where sdf = min(net, R - |x|) is negative, so every ray is opaque, none misses, and the mask has no gradient: d mask /
d sdf is T_end times a factor of order one, in float64 |g_sdf| = 6.9e-10 on the 35 rays of scene.camera(7, 5), below the fp32 rounding of either
formulation (6.8e-7), and `mask alone` would compare noise with noise (measured: 28 of 43 tensors outside 3e-2, worst 2.57).  At far = 4.0, 27 of
the 35 rays of scene.camera(7, 5) and 60 of the 64 of scene.camera(8, 8) (the G9 golden camera) hit, and two rays of the first graze the surface
(mask_volume 0.976 and 0.949): they carry the mask's gradient, and `mask alone` asserts that such a ray exists.

Measured on an MI355X, worst relative difference over the parameter tensors (bound 3e-2): all three cotangents 2.9e-3 (13-ray patches) and 4.3e-4 (64 rays),
depth alone 2.1e-4, normals alone 4.2e-4, mask alone 4.6e-4, all three + rgb + eikonal 1.6e-3, the whole finetune_step(geometry_loss) native against
autograd 8.3e-4; bound 2e-3 (the differences are ln_beta's: the compositors' atomics): kept state against depths_all 6.6e-7, finetune_step(geometry_loss)
against backward_patches by hand 4.2e-7, a geometry loss that is identically zero against no geometry loss 3.8e-7."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def volsdf():
    from nerfart_amd import scene
    model, rk, render_fn = scene.build_model("VolSDF", seed=0, beta=0.01, device=DEV, precision="bf16x3")
    kw = {k: v for k, v in rk.items() if k != "rayschunk"}
    kw["N_samples"] = 32                                        # 32 + 64 = 96 points per ray: 13 rays = 19.5 tiles of 64
    kw["far"] = 4.0                                             # behind the object, inside the bounding sphere: a ray that misses stays transparent
    return model, kw, render_fn


_SCENES = {}


def _rays(volsdf, H, W):
    """(rays_o [N, 3], rays_d [N, 3], cotangents dict) of scene.camera(H, W); the cotangents are zero where pass 1's mask_volume < 0.5."""
    from nerfart_amd import scene, rend_util
    if (H, W) not in _SCENES:
        model, kw, render_fn = volsdf
        c2w, K = scene.camera(H, W)
        o, d, _ = rend_util.get_rays(c2w[None].to(DEV), K[None].to(DEV), H, W)
        with torch.no_grad():
            _, _, ex = render_fn(o, d, detailed_output=False, require_nablas=True, calc_normal=True, **kw)
        hit = (ex["mask_volume"].reshape(-1) >= 0.5).float()
        assert float(hit.mean()) >= 0.5, f"only {int(hit.sum())} of {hit.numel()} rays hit the object: choose another camera"
        g = torch.Generator().manual_seed(11 + H * W)
        N = H * W
        cot = dict(depth=torch.rand(N, generator=g).to(DEV) * 1e-2 * hit, normals=torch.rand(N, 3, generator=g).to(DEV) * 1e-2 * hit[:, None],
                   mask=torch.rand(N, generator=g).to(DEV) * 1e-2 * hit, rgb=torch.rand(N, 3, generator=g).to(DEV) * 1e-2)
        assert all(float((cot[k].reshape(N, -1).abs().sum(-1) > 0).float().mean()) >= 0.5 for k in ("depth", "normals", "mask"))
        cot["mask_volume"] = ex["mask_volume"].reshape(-1)
        _SCENES[(H, W)] = (o[0], d[0], cot)
    return _SCENES[(H, W)]


def _grads(model):
    return {n: (torch.zeros_like(p) if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}


def _compare(got, ref, bound, what):
    rels = {name: float((got[name] - r).norm() / (r.norm() + 1e-12)) for name, r in ref.items()}
    worst = max(rels, key=rels.get)
    print(f"  {what}: worst relative difference {rels[worst]:.2e} ({worst}; bound {bound:g}; {sum(v >= bound for v in rels.values())} of {len(rels)} tensors outside)")
    assert any(float(r.norm()) > 0 for r in ref.values()), (what, "every reference gradient is zero: nothing was compared")
    bad = {n: v for n, v in rels.items() if not v < bound}
    assert not bad, (what, bad)


CONFIGS = [
    ("all three, ragged 13-ray patches", 7, 5, 13, ("depth", "normals", "mask"), False),
    ("all three, 64 rays in one patch", 8, 8, 64, ("depth", "normals", "mask"), False),
    ("depth alone", 7, 5, 13, ("depth",), False),
    ("normals alone", 7, 5, 13, ("normals",), False),
    ("mask alone", 7, 5, 13, ("mask",), False),
    ("all three + rgb + eikonal", 7, 5, 13, ("depth", "normals", "mask"), True),
]


@pytest.mark.parametrize("what,H,W,patch,which,full", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_native_geometry_gradients_match_autograd(volsdf, what, H, W, patch, which, full):
    from nerfart_amd.trainer import Trainer
    model, kw, _ = volsdf
    o, d, cot = _rays(volsdf, H, W)
    if which == ("mask",):
        # d mask / d sdf is T_end times a factor of order one: on an opaque ray both formulations return rounding noise around zero
        grazing = (cot["mask_volume"] >= 0.5) & (cot["mask_volume"] < 0.999)
        assert bool(grazing.any()), "no ray with a cotangent is partially transparent: the mask has no gradient to compare"
    g_rgb = cot["rgb"] if full else torch.zeros_like(cot["rgb"])
    geo = {f"gradient_{k}": cot[k] for k in which}
    res = {}
    for native in (False, True):
        model.zero_grad()
        Trainer(model, w_eikonal=0.1, use_eikonal=full, pass2_rays=patch, native=native).backward_patches(o, d, g_rgb, **geo, **kw)
        res[native] = _grads(model)
    _compare(res[True], res[False], 3e-2, what)


def test_kept_state_and_fresh_samples_agree(volsdf):
    from nerfart_amd.trainer import Trainer
    model, kw, _ = volsdf
    o, d, cot = _rays(volsdf, 7, 5)
    geo = dict(gradient_depth=cot["depth"], gradient_normals=cot["normals"], gradient_mask=cot["mask"])
    tr = Trainer(model, w_eikonal=0.1, use_eikonal=True, pass2_rays=13, patches_per_launch=2)
    tr.render_keep(o, d, **kw)
    kept = tr._kept
    depths = torch.cat([k[0] for k in kept], 0)
    model.zero_grad()
    tr.backward_patches(o, d, cot["rgb"], kept=kept, **geo, **kw)
    with_state = _grads(model)
    model.zero_grad()
    tr.backward_patches(o, d, cot["rgb"], depths_all=depths, **geo, **kw)
    _compare(_grads(model), with_state, 2e-3, "depths_all against kept state")


def test_finetune_step_with_a_geometry_loss(volsdf):
    from nerfart_amd import scene
    from nerfart_amd.trainer import Trainer
    model, kw, render_fn = volsdf
    H, W = 7, 5
    o, d, _ = _rays(volsdf, H, W)
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    style = lambda p, t: ((p - t) ** 2).mean()
    tr = Trainer(model, w_eikonal=0.1, use_eikonal=True, pass2_rays=13)

    def step(**extra):
        model.zero_grad()
        out = tr.finetune_step(render_fn, o, d, target, H, style, **extra, **kw)
        return _grads(model), out
    plain, out0 = step()
    assert "geometry" not in out0
    zero, out1 = step(geometry_loss=lambda m: (m["depth"] * 0).sum())
    assert out1["geometry"] == 0.0
    _compare(zero, plain, 2e-3, "a geometry loss that is identically zero")
    # a depth-preservation + normal-consistency term against the maps of a differently perturbed copy of the sphere-initialised weights
    other, _, other_fn = scene.build_model("VolSDF", seed=1, beta=0.01, device=DEV, precision="bf16x3")
    with torch.no_grad():
        _, d0, ex0 = other_fn(o[None], d[None], detailed_output=False, require_nablas=True, calc_normal=True, **kw)
    to_img = lambda t, c: t.reshape(1, H, W, c).permute(0, 3, 1, 2)
    d0, n0 = to_img(d0, 1), to_img(ex0["normals_volume"], 3)
    fn = lambda m: ((m["depth"] - d0) ** 2 * m["mask"]).mean() + (1 - (m["normals"] * n0).sum(1)).mean()
    got, out2 = step(geometry_loss=fn)
    assert np.isfinite(out2["geometry"]) and out2["geometry"] > 0
    # by hand: the same pass 1, autograd's cotangents of style + fn, backward_patches
    tr._maps = []
    rgb = tr.render_keep(o, d, **kw)
    maps_in, tr._maps = tr._maps, None
    cat = lambda i, c: to_img(torch.cat([m[i] for m in maps_in], 0), c).detach().clone().requires_grad_(True)
    maps = {"depth": cat(0, 1), "normals": cat(1, 3), "mask": cat(2, 1)}
    rgb = rgb.detach().reshape(1, -1, 3).requires_grad_(True)
    loss = style(to_img(rgb, 3), to_img(target, 3)) + fn(maps)
    loss.backward()
    flat = lambda t: t.grad.permute(0, 2, 3, 1).reshape(H * W, -1)
    assert abs(float(loss) - out2["loss"]) <= 1e-6 * abs(out2["loss"])
    model.zero_grad()
    tr.backward_patches(o, d, rgb.grad[0], kept=tr._kept, gradient_depth=flat(maps["depth"]).reshape(-1), gradient_normals=flat(maps["normals"]),
                        gradient_mask=flat(maps["mask"]).reshape(-1), **kw)
    tr._kept = None
    _compare(got, _grads(model), 2e-3, "finetune_step(geometry_loss) against backward_patches by hand")
    diff = max(float((got[n] - plain[n]).norm() / (plain[n].norm() + 1e-12)) for n in got)
    assert diff > 2e-3, "the geometry loss changed no gradient"


def test_finetune_step_geometry_loss_on_the_other_pass1_paths(volsdf):
    """The maps also come out of the fused renderer (the autograd step's pass 1) and of the two-draw staged pass 1 (perturb=True): the whole autograd
    step agrees with the whole native step within the native-against-autograd bound, and a perturb=True step runs with finite results."""
    from nerfart_amd.trainer import Trainer
    model, kw, render_fn = volsdf
    H, W = 7, 5
    o, d, _ = _rays(volsdf, H, W)
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    style = lambda p, t: ((p - t) ** 2).mean()
    fn = lambda m: ((m["depth"] - 2.0) ** 2 * m["mask"]).mean() + (m["normals"][:, 2] + 1).mean()
    res, outs = {}, {}
    for native in (False, True):
        model.zero_grad()
        outs[native] = Trainer(model, w_eikonal=0.1, use_eikonal=True, pass2_rays=13, native=native).finetune_step(render_fn, o, d, target, H, style, geometry_loss=fn, **kw)
        res[native] = _grads(model)
    assert abs(outs[True]["geometry"] - outs[False]["geometry"]) <= 1e-3 * abs(outs[False]["geometry"]), outs
    _compare(res[True], res[False], 3e-2, "finetune_step(geometry_loss): native against autograd")
    draws = {p: torch.rand(H * W, 64, generator=torch.Generator().manual_seed(20 + p)).to(DEV) for p in (1, 2)}
    tr = Trainer(model, w_eikonal=0.1, use_eikonal=True, pass2_rays=13)
    tr.uniform_source = lambda pass_no, first, n, k, dev: draws[pass_no][first:first + n, :k]
    pk = dict(kw, perturb=True)
    assert tr.shares_algorithm1(pk)
    model.zero_grad()
    out = tr.finetune_step(render_fn, o, d, target, H, style, geometry_loss=fn, **pk)
    assert np.isfinite(out["geometry"]) and abs(out["geometry"] - outs[True]["geometry"]) <= 5e-2 * abs(outs[True]["geometry"]), (out["geometry"], outs[True]["geometry"])
    assert all(bool(torch.isfinite(g).all()) for g in _grads(model).values())


def test_neus_refuses_the_geometry_cotangents():
    from nerfart_amd import scene, rend_util
    from nerfart_amd.trainer import Trainer
    model, rk, render_fn = scene.build_model("NeuS", seed=0, beta=None, device=DEV, precision="bf16x3")
    H, W = 4, 4
    c2w, K = scene.camera(H, W)
    o, d, _ = rend_util.get_rays(c2w[None].to(DEV), K[None].to(DEV), H, W)
    tr = Trainer(model, pass2_rays=16)
    z = torch.zeros(H * W, device=DEV)
    with pytest.raises(NotImplementedError, match="VolSDF only"):
        tr.backward_patches(o[0], d[0], torch.zeros(H * W, 3, device=DEV), gradient_depth=z, **rk)
    with pytest.raises(NotImplementedError, match="VolSDF only"):
        tr.finetune_step(render_fn, o[0], d[0], torch.zeros(H * W, 3, device=DEV), H, lambda p, t: ((p - t) ** 2).mean(),
                         geometry_loss=lambda m: m["depth"].sum(), **rk)
    assert all(p.grad is None for p in model.parameters())
