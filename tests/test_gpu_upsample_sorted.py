"""k_upsample (csrc/volsdf_render.hip) leaves out its 45-stage bitonic sort for a row of new depths that is already in order
(csrc/sample_cdf.h::lane_row_in_order); NERFART_UPSAMPLE_SORT=always sorts every row, as the kernel did before.  Sorting a row that is in order
returns the same bits, so the whole sampler must give the same bits either way: held here on 256 rays of the benchmark's frame at three betas, in one
process (the launcher reads the variable at every call)."""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
VAR = "NERFART_UPSAMPLE_SORT"


@contextlib.contextmanager
def _always_sort():
    old = os.environ.get(VAR)
    os.environ[VAR] = "always"
    try:
        yield
    finally:
        if old is None:
            del os.environ[VAR]
        else:
            os.environ[VAR] = old


@pytest.fixture(scope="module")
def rays():
    """256 rays spread over bench.py's 480x270 frame (orbit pose 0)"""
    from nerfart_amd import hip, rend_util, scene
    H, W = 480, 270
    c2w, K = scene.camera(H, W, angle=scene.spiral(90)[0])
    o, d, _ = rend_util.get_rays(c2w[None].to(DEV), K[None].to(DEV), H, W)
    pick = torch.linspace(0, H * W - 1, 256, device=DEV).round().long()
    return o[0][pick].contiguous(), hip.normalize_dirs(d[0][pick].contiguous())


@pytest.mark.parametrize("beta", [0.01, 0.002, 0.1])
def test_sampler_is_the_same_with_and_without_the_sort(rays, beta):
    from nerfart_amd import hip, scene
    model, _, _ = scene.build_model("VolSDF", seed=0, beta=beta, device=DEV, precision="mixed")
    model.calibrate_sampler()
    sa = model.sampler_args()
    alpha, b = (float(t.detach()) for t in model.forward_ab())
    o, dn = rays

    def run():
        st = {}
        r = hip.volsdf_fine_sample(sa["blob"], o, dn, 0.0, 6.0, 3.0, alpha, b, 0.1, 512, 512, 64, 6, 10, precision=sa["precision"], escalate=sa["escalate"],
                                   guard=sa["guard"], late_round=sa["late_round"], stats=st)
        torch.cuda.synchronize()
        return tuple(t.clone() for t in r), st["escalated"]

    assert VAR not in os.environ, f"{VAR} is set by the caller: the first run would not be the default"
    (new, n_new), = (run(),)
    with _always_sort():
        ref, n_ref = run()
    usage = new[2]
    print(f"  beta {beta}: rounds used min {float(usage.min()):.0f} max {float(usage.max()):.0f}, {int((usage != 0).sum())} rays up-sampled, {n_new} escalated")
    if beta < 0.1:            # at beta = 0.1 every ray of this frame converges on its 512 initial samples: no up-sampling round, the case holds the rest
        assert int((usage != 0).sum()) >= 128, "most rays must go through k_upsample at this beta"
    assert n_new == n_ref
    for name, a, r in zip(("d_fine", "beta_map", "iter_usage"), new, ref):
        assert torch.equal(a, r), name
    assert bool(torch.isfinite(new[0]).all())
