"""The VolSDF renderer's segment-ordered final stage (csrc/volsdf_render.hip, final_stage_skipping): with no per-sample output requested the
final samples run in depth segments of 32, front to back, and a ray whose fp32 running optical depth has reached THETA = 128 - its
transmittance is exactly 0 from there on - leaves the live list: the samples behind that point are never evaluated.

Held here, on the synthetic scene at 64 x 36: the pixels are BIT-EQUAL to the full evaluation (detailed_output=True takes the unskipped loop)
and to the per-stage restatement hip.volsdf_render_mixed; ragged shapes (a ray count and sample counts that are no multiple of anything, several
ray groups); a scene with nothing to skip evaluates exactly R P points; a NaN-filled workspace poisons nothing; and the number of points the
sdf + nabla kernel evaluated is EXACTLY R P minus what the rule - restated here from the unskipped run's d_vals and sigma alone - says is dead."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 64, 36
THETA, SEG = 128.0, 32
POSES = (0, 3)                  # of an 8-view orbit
KEYS = ("rgb", "depth_volume", "mask_volume", "normals_volume")


@functools.lru_cache(maxsize=None)
def _model(precision, beta):
    from nerfart_amd import scene
    return scene.build_model("VolSDF", seed=0, beta=beta, device=DEV, precision=precision)


@functools.lru_cache(maxsize=None)
def _rays(pose):
    from nerfart_amd import scene, rend_util
    c2w, K = scene.camera(H, W, angle=scene.spiral(8)[pose])
    o, d, _ = rend_util.get_rays(c2w[None].to(DEV), K[None].to(DEV), H, W)
    return o.contiguous(), d.contiguous()


def _render(precision, beta, o, d, detailed, count=False, **extra):
    """-> (outputs by key, points the sdf + nabla kernel evaluated or None, extras)"""
    from nerfart_amd import hip
    model, rk, fn = _model(precision, beta)
    if count:
        hip.profile_begin()
    rgb, depth, ex = fn(o, d, require_nablas=True, calc_normal=True, detailed_output=detailed, **{**rk, **extra})
    torch.cuda.synchronize()
    n = hip.profile_end()["k_sdf_nabla"][2] if count else None
    return {k: ex[k][0] for k in KEYS}, n, ex


@functools.lru_cache(maxsize=None)
def _frame(precision, beta, pose):
    """One frame both ways, rendered once: (skipping outputs, points evaluated, full outputs, full extras)."""
    o, d = _rays(pose)
    skip, n_eval, _ = _render(precision, beta, o, d, False, count=True)
    full, _, ex = _render(precision, beta, o, d, True)
    return skip, n_eval, full, ex


def _points_the_rule_evaluates(ex):
    """The rule from the unskipped outputs alone: x_k = max(sigma_k (d_{k+1} - d_k), 0); the fp32 sum over k < s in ascending k, one addition at a
    time (the kernel's chain, so the count is exact); at the segment boundaries s = 32, 64, ... a ray whose sum is >= THETA is dead from s on."""
    sigma, dv = ex["sigma"][0], ex["d_vals"][0]
    R, P = dv.shape
    x = torch.clamp_min(sigma[:, :-1] * (dv[:, 1:] - dv[:, :-1]), 0.0)
    evaluated = torch.full((R,), P, dtype=torch.long, device=dv.device)
    run = torch.zeros(R, dtype=torch.float32, device=dv.device)
    for k in range(P - 1):
        run = run + x[:, k]
        s = k + 1
        if s % SEG == 0 and s < P:
            evaluated = torch.where((run >= THETA) & (evaluated == P), torch.full_like(evaluated, s), evaluated)
    return int(evaluated.sum())


@pytest.mark.parametrize("pose", POSES)
@pytest.mark.parametrize("beta", [0.01, 0.002])
@pytest.mark.parametrize("precision", ["mixed", "bf16x3"])
def test_pixels_are_bit_equal_and_exactly_the_dead_segments_are_skipped(precision, beta, pose):
    from nerfart_amd import hip
    skip, n_eval, full, ex = _frame(precision, beta, pose)
    R, P = ex["d_vals"][0].shape
    for k in KEYS:
        assert torch.equal(skip[k], full[k]), k
    # the per-stage restatement evaluates everything too
    model, rk, _ = _model(precision, beta)
    o, d = _rays(pose)
    surf, rad = model.packed()
    samp = model.packed_sampler()
    alpha, beta_ = (float(t.detach()) for t in model.forward_ab())
    staged = hip.volsdf_render_mixed(surf, rad, *(samp if samp is not None else (surf, 1)), model.view_tiles, o[0], d[0], near=rk["near"], far=rk["far"],
                                     R_bg=rk["obj_bounding_radius"], alpha=alpha, beta=beta_, max_upsample_steps=rk["max_upsample_steps"], precision=1,
                                     guard=model.sampler_guard if samp is not None else 0.0, late_round=model.sampler_late_round if samp is not None else 0)
    for k in KEYS:
        assert torch.equal(skip[k], staged[k]), k
    # not vacuous, and exact: the kernel's count is R P minus what the rule, restated from the unskipped run, marks dead
    want = _points_the_rule_evaluates(ex)
    share = 1.0 - want / (R * P)
    print(f"  {precision}, beta {beta}, pose {pose}: the rule skips {share:.4f} of {R * P} points; evaluated {n_eval}, expected {want}")
    assert share >= 0.05, "the reference share of this frame is too small to test skipping on"
    assert n_eval < R * P
    assert n_eval == want


@pytest.mark.parametrize("precision", ["mixed", "bf16x3"])
def test_ragged_shapes_and_several_groups(precision):
    o, d = _rays(POSES[0])
    o, d = o[:, :2303].contiguous(), d[:, :2303].contiguous()
    for beta in (0.01, 0.002):
        # N_samples is a power of two (Algorithm 1's 4 N_samples new depths per round are bitonic-sorted); P = 192 in 6 groups, 37 = 32 + 5 (a short
        # last segment), 29 (one segment, shorter than 32), 91 in groups of 19 rays
        for extra in (dict(k3_rays_chunk=64), dict(k3_rays_chunk=64, N_samples=32, N_importance=5), dict(k3_rays_chunk=64, N_samples=16, N_importance=13),
                      dict(k3_rays_chunk=7, N_samples=64, N_importance=27)):
            skip, n_eval, _ = _render(precision, beta, o, d, False, count=True, **extra)
            full, _, ex = _render(precision, beta, o, d, True, **extra)
            for k in KEYS:
                assert torch.equal(skip[k], full[k]), (beta, extra, k)
            assert n_eval == _points_the_rule_evaluates(ex), (beta, extra)


def test_nothing_dead_evaluates_every_point():
    o, d = _rays(POSES[0])
    skip, n_eval, _ = _render("mixed", 0.1, o, d, False, count=True)
    full, _, ex = _render("mixed", 0.1, o, d, True)
    R, P = ex["d_vals"][0].shape
    for k in KEYS:
        assert torch.equal(skip[k], full[k]), k
    assert _points_the_rule_evaluates(ex) == R * P, "beta = 0.1: the rule marks nothing on this scene"
    assert n_eval == R * P


@pytest.mark.parametrize("beta", [0.01, 0.002])
def test_nan_prefilled_workspace(beta):
    from nerfart_amd import hip
    skip, _, full, ex = _frame("mixed", beta, POSES[0])
    o, d = _rays(POSES[0])
    model, rk, _ = _model("mixed", beta)
    R = o.shape[1]
    hip._ws_cache.clear()
    nb = int(hip.lib.nerfart_volsdf_render_workspace_bytes(R, 128, 64, int(rk["max_upsample_steps"]), 8192))
    hip._workspace(nb, DEV).view(torch.int32).fill_(-1)                        # 0xffffffff: NaN as fp32
    again, _, _ = _render("mixed", beta, o, d, False)
    assert hip._workspace(nb, DEV).numel() == nb, "the render ran in the workspace filled above"
    for k in KEYS:
        assert bool(torch.isfinite(again[k]).all()), k
        assert torch.equal(again[k], skip[k]), k
