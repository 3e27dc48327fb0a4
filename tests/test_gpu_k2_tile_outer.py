"""The tile-outer K2 of C-ABI precision 5 (csrc/mlp_k2_f16x1_to.hip: 32 points per wave, every weight fragment feeds two point groups) against the
k-step-outer reference kernel it replaces as the default (csrc/mlp_chain_f16x1.hip, NERFART_K2_F16X1=ref), in one process: every comparison is
BITWISE on the raw fp32 - the new order changes which lane of which wave computes a point, never what is computed."""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


VAR = "NERFART_K2_F16X1"


@contextlib.contextmanager
def _reference_kernel():
    old = os.environ.get(VAR)
    os.environ[VAR] = "ref"                         # read by the launcher at every call
    try:
        yield
    finally:
        if old is None:
            del os.environ[VAR]
        else:
            os.environ[VAR] = old


def _both(fn):
    assert VAR not in os.environ, f"{VAR} is set by the caller: the first run would not be the default kernel's"
    new = fn()
    with _reference_kernel():
        ref = fn()
    return new, ref


def _kernels_launched(fn):
    """names of the GPU kernels `fn` launches, from torch's profiler (the HIP activity records of this process)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if str(e.device_type).endswith("CUDA")}


def test_the_two_runs_are_two_kernels(models):
    """Every other test compares `default` with `NERFART_K2_F16X1=ref`: that proves something only if the two launch different kernels."""
    _, blob = models[0]
    x = _points(300, False, 1)
    assert VAR not in os.environ
    new = _kernels_launched(lambda: _sdf_points(blob, x, 300, 3.0))
    with _reference_kernel():
        ref = _kernels_launched(lambda: _sdf_points(blob, x, 300, 3.0))
    print("  default:", sorted(n for n in new if "nerfart" in n), " ref:", sorted(n for n in ref if "nerfart" in n))
    assert any("k_sdf_only_to" in n for n in new) and not any("k_sdf_only_bf16" in n for n in new)
    assert any("f16x1" in n and "k_sdf_only_bf16" in n for n in ref) and not any("k_sdf_only_to" in n for n in ref)


@pytest.fixture(scope="module")
def models():
    from nerfart_amd import scene
    out = {}
    for seed in (0, 3):
        model, rk, fn = scene.build_model("VolSDF", seed=seed, beta=0.01, device=DEV, precision="mixed")
        model.calibrate_sampler()
        blob, prec = model.packed_sampler()
        assert prec == 5
        out[seed] = (model, blob)
    return out


def _points(M, wide, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(M, 3, generator=g) * 2 - 1) * (8.0 if wide else 1.5)
    return x.to(DEV).contiguous()


def _sdf_points(blob, x, M, R_bg):
    """nerfart_sdf_fwd on the first M points into a buffer with 64 sentinels behind them"""
    from nerfart_amd import hip
    out = torch.full((M + 64,), -777.25, dtype=torch.float32, device=DEV)
    hip._check(hip.lib.nerfart_sdf_fwd(blob.data_ptr(), 5, x.data_ptr(), M, float(R_bg), out.data_ptr(), torch.cuda.current_stream().cuda_stream), "nerfart_sdf_fwd")
    return out


@pytest.mark.parametrize("seed", [0, 3])
def test_points_mode_is_the_reference_kernel_bit_for_bit(models, seed):
    _, blob = models[seed]
    for wide in (False, True):
        x = _points(513, wide, 11 + seed)
        for R_bg in (0.0, 3.0):
            for M in (1, 15, 16, 17, 31, 33, 255, 256, 257, 511, 513):      # one lane, a group boundary, a wave's two groups, a tile boundary, two tiles
                new, ref = _both(lambda: _sdf_points(blob, x, M, R_bg))
                assert bool(torch.isfinite(new[:M]).all())
                assert torch.equal(new[:M], ref[:M]), (wide, R_bg, M, float((new[:M] - ref[:M]).abs().max()))
                assert bool((new[M:] == -777.25).all()), "nothing is written behind point M - 1"


def _sdf_rays(blob, o, dn, ray_idx, depth, n_slots, n_per_ray, R_bg, out_stride):
    from nerfart_amd import hip
    out = torch.full((n_slots, out_stride), -777.25, dtype=torch.float32, device=DEV)
    hip._check(hip.lib.nerfart_sdf_fwd_rays(blob.data_ptr(), 5, o.data_ptr(), dn.data_ptr(), None if ray_idx is None else ray_idx.data_ptr(), depth.data_ptr(),
                                            n_slots, n_per_ray, depth.shape[1], float(R_bg), out.data_ptr(), out_stride, torch.cuda.current_stream().cuda_stream),
               "nerfart_sdf_fwd_rays")
    return out


@pytest.mark.parametrize("n_per_ray", [5, 32, 512])
def test_rays_mode_is_the_reference_kernel_bit_for_bit(models, n_per_ray):
    from nerfart_amd import hip
    _, blob = models[0]
    g = torch.Generator().manual_seed(n_per_ray)
    R = 300
    o = (torch.randn(R, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 2.5])).to(DEV).contiguous()
    dn = hip.normalize_dirs((torch.randn(R, 3, generator=g) * 0.3 - torch.tensor([0.0, 0.0, 1.0])).to(DEV).contiguous())
    for pad_d, pad_o in ((0, 0), (3, 0), (0, 7), (3, 7)):                       # depth_stride / out_stride larger than n_per_ray
        # (a) the sampler's compacted call: n_slots slots of a shuffled subset of the rays
        n_slots = 77
        idx = torch.randperm(R, generator=g)[:n_slots].to(torch.int32).to(DEV).contiguous()
        depth = (torch.rand(n_slots, n_per_ray + pad_d, generator=g) * 6).sort(-1)[0].to(DEV).contiguous()
        new, ref = _both(lambda: _sdf_rays(blob, o, dn, idx, depth, n_slots, n_per_ray, 3.0, n_per_ray + pad_o))
        assert torch.equal(new, ref) and bool(torch.isfinite(new[:, :n_per_ray]).all())
        assert bool((new[:, n_per_ray:] == -777.25).all())
        # (b) no index: slot = ray
        depth7 = (torch.rand(7, n_per_ray + pad_d, generator=g) * 6).sort(-1)[0].to(DEV).contiguous()
        new, ref = _both(lambda: _sdf_rays(blob, o, dn, None, depth7, 7, n_per_ray, 0.0, n_per_ray + pad_o))
        assert torch.equal(new, ref) and bool((new[:, n_per_ray:] == -777.25).all())


def test_tile_loop_wraps_the_weight_stream(models):
    """Two 256-point tiles per workgroup, a third for some, a ragged last one: the weight stream goes from layer 7's last chunk back to layer 0."""
    _, blob = models[3]
    M = 2 * 256 * torch.cuda.get_device_properties(0).multi_processor_count + 77
    x = _points(M, False, 5)
    new, ref = _both(lambda: _sdf_points(blob, x, M, 3.0))
    assert torch.equal(new, ref) and bool(torch.isfinite(new[:M]).all())


def test_guarded_sampler_is_unchanged_end_to_end(models):
    from nerfart_amd import hip, rend_util, scene
    model, _ = models[0]
    H, W = 48, 27
    c2w, K = scene.camera(H, W, angle=scene.spiral(90)[3])
    o, d, _ = rend_util.get_rays(c2w[None].to(DEV), K[None].to(DEV), H, W)
    o = o[0].contiguous()
    dn = hip.normalize_dirs(d[0].contiguous())
    alpha, beta = (float(t.detach()) for t in model.forward_ab())
    sa = model.sampler_args()
    assert sa["precision"] == 5 and sa["guard"] == 0.005 and sa["late_round"] == 3

    def run():
        st = {}
        r = hip.volsdf_fine_sample(sa["blob"], o, dn, 0.0, 6.0, 3.0, alpha, beta, 0.1, 512, 512, 64, 6, 10, precision=5, escalate=sa["escalate"], guard=0.005,
                                   late_round=3, stats=st)
        return tuple(t.clone() for t in r), st["escalated"]

    (new, n_new), (ref, n_ref) = _both(run)
    assert o.shape[0] == 1296 and n_new == n_ref
    for a, b in zip(new, ref):                       # d_fine, beta_map, iter_usage
        assert torch.equal(a, b)
