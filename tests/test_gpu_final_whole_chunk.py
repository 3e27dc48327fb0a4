"""The segment-ordered final stage of the VolSDF renderer as ONE live list per chunk (csrc/volsdf_render.hip, final_stage_skipping): the h7 rows of
a segment launch are carved out of the sampler's dead region, so the rays are no longer cut into groups of 6 k3_rays_chunk, and one launch
(k_scatter_advance) places a segment's outputs and advances the running optical depths.

Held here on 300 rays of the synthetic scene, in a NaN-filled workspace: rgb, depth, acc and normals are bit-equal for k3_rays_chunk = 16, 32, 300
and 4,096 and bit-equal to the plain loop (detailed_output=True's).  With two up-sampling rounds or one the sampler's region is too small for the
whole chunk's h7 rows and the rays run in groups again: two groups of 150 with their h7 rows in the sampler's region (2 rounds, k3_rays_chunk = 16),
groups of 192 on the workspace's own h7 carve (1 round, k3_rays_chunk = 32), one group on it where it holds the chunk.  A scene on which every ray
dies in the first segment evaluates exactly 32 points per ray, one on which none dies exactly P."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
R, NS, NI = 300, 128, 64
P = NS + NI
KEYS = ("rgb", "depth_volume", "mask_volume", "normals_volume")
K3 = (16, 32, 300, 4096)


@functools.lru_cache(maxsize=None)
def _scene(beta):
    from nerfart_amd import scene, rend_util
    model, _, _ = scene.build_model("VolSDF", seed=0, beta=beta, device=DEV, precision="mixed")
    c2w, K = scene.camera(24, 16, angle=scene.spiral(8)[3])
    o, d, _ = rend_util.get_rays(c2w[None].to(DEV), K[None].to(DEV), 24, 16)
    a, b = (float(t.detach()) for t in model.forward_ab())
    return model, o[0, :R].contiguous(), d[0, :R].contiguous(), a, b


def _render(beta, k3, detailed, alpha=None, max_iter=5, count=False):
    """One render in a workspace filled with NaN -> (the four maps, points the sdf + nabla kernel evaluated or None)"""
    from nerfart_amd import hip
    model, o, d, a, b = _scene(beta)
    surf, rad = model.packed()
    hip._ws_cache.clear()
    nb = int(hip.lib.nerfart_volsdf_render_workspace_bytes(R, NS, NI, max_iter, k3))
    hip._workspace(nb, DEV).view(torch.int32).fill_(-1)                        # 0xffffffff: NaN as fp32
    if count:
        hip.profile_begin()
    out = hip.volsdf_render(surf, rad, model.view_tiles, o, d, near=0.0, far=6.0, R_bg=3.0, alpha=a if alpha is None else alpha, beta=b, n_samples=NS,
                            n_importance=NI, max_upsample_steps=max_iter, detailed=detailed, k3_rays_chunk=k3, precision=model.precision_id,
                            sampler=model.packed_sampler(), guard=model.sampler_guard, late_round=model.sampler_late_round)
    torch.cuda.synchronize()
    n = hip.profile_end()["k_sdf_nabla"][2] if count else None
    assert hip._workspace(nb, DEV).numel() == nb, "the render ran in the workspace filled above"
    return {k: out[k] for k in KEYS}, n


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in KEYS)


@pytest.mark.parametrize("max_iter", [5, 2, 1])
@pytest.mark.parametrize("beta", [0.01, 0.002])
def test_any_chunk_size_gives_the_plain_loops_pixels(beta, max_iter):
    full, _ = _render(beta, 4096, True, max_iter=max_iter)
    assert all(bool(torch.isfinite(full[k]).all()) for k in KEYS)
    counts = []
    for k3 in K3:
        skip, n = _render(beta, k3, False, max_iter=max_iter, count=True)
        assert _same_bits(skip, full), (k3, max_iter)
        counts.append(n)
    print(f"  beta {beta}, {max_iter} rounds: {counts[0]} of {R * P} points evaluated")
    assert len(set(counts)) == 1 and counts[0] < R * P, "the same rays leave at the same segments however they are grouped, and some do leave"


def test_every_ray_dies_in_the_first_segment():
    """alpha = 1e30 at beta = 1: sigma >= 1e30 * 0.5 exp(-|sdf|) >= 1e21 wherever |sdf| <= 20, so the first segment's optical depth passes 128 on
    every ray; the other five segments are never launched."""
    full, _ = _render(1.0, 300, True, alpha=1e30)
    for k3 in K3:
        skip, n = _render(1.0, k3, False, alpha=1e30, count=True)
        assert n == R * 32, k3
        assert _same_bits(skip, full), k3


def test_no_ray_dies():
    full, _ = _render(0.1, 300, True)
    for k3 in K3:
        skip, n = _render(0.1, k3, False, count=True)
        assert n == R * P, k3
        assert _same_bits(skip, full), k3
