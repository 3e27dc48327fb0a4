"""The per-ray sampler kernels with one LDS row less (csrc/volsdf_render.hip): k_upsample reads the sdf row from global memory (3 n + n_up floats of
LDS instead of 4 n + n_up), k_merge_check writes the merged rows straight to global memory and takes them back as a copy in the two depth rows, which
are dead by then (2 (n + n_up) floats instead of 3 (n + n_up)).  NERFART_PERRAY_LDS=ref, read at every call, runs both with the earlier LDS layout: the
same lane owns the same intervals in the same order,
so d_fine, beta_map, iter_usage and the escalated count are EQUAL BIT FOR BIT - held here on the unguarded fp32 sampler and on the guarded entry
point, over rounds 1 to 6 (the 16-interval and 24-interval register scans and the generic scan), with a NaN-filled workspace, and on an 8 + 8
sample row on which most lanes own no interval at all."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_RAYS = 70                      # more than one 64-ray block of the MLP kernels, with a ragged tail
MAX_ITER = 6


@functools.lru_cache(maxsize=None)
def _scene(precision, beta):
    from nerfart_amd import scene, rend_util, hip
    model, _, _ = scene.build_model("VolSDF", seed=0, beta=beta, device=DEV, precision=precision)
    c2w, K = scene.camera(24, 16, angle=scene.spiral(8)[3])
    o, d, _ = rend_util.get_rays(c2w[None].to(DEV), K[None].to(DEV), 24, 16)
    o, d = o[0].contiguous(), d[0].contiguous()
    alpha, beta_ = (float(t.detach()) for t in model.forward_ab())
    return model, o, hip.normalize_dirs(d), alpha, beta_


def _run(form, blob, prec, o, dn, alpha, beta, n_init=512, n_up=512, **kw):
    """-> (d_fine, beta_map, iter_usage, escalated) of one form of the kernels: 'ref' = the earlier one"""
    from nerfart_amd import hip
    st = {}
    old = os.environ.pop("NERFART_PERRAY_LDS", None)
    try:
        if form == "ref":
            os.environ["NERFART_PERRAY_LDS"] = "ref"
        out = hip.volsdf_fine_sample(blob, o, dn, 0.0, 6.0, 3.0, alpha, beta, 0.1, n_init, n_up, 64, MAX_ITER, 10, precision=prec, stats=st, **kw)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("NERFART_PERRAY_LDS", None)
        if old is not None:
            os.environ["NERFART_PERRAY_LDS"] = old
    return (*out, st["escalated"])


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def _rays_over_all_rounds(blob, prec, o, dn, alpha, beta, **kw):
    """70 of the frame's 384 rays, spread evenly over the rays sorted by the number of rounds they take (earlier form), so that every scan path runs"""
    usage = _run("ref", blob, prec, o, dn, alpha, beta, **kw)[2]
    rounds = torch.where(usage < 0, torch.full_like(usage, MAX_ITER + 1.0), usage)
    order = torch.argsort(rounds, stable=True)
    pick = order[torch.linspace(0, order.numel() - 1, N_RAYS, device=DEV).round().long()]
    return pick, rounds[pick]


@pytest.mark.parametrize("beta", [0.01, 0.002])
@pytest.mark.parametrize("entry", ["fp32", "guarded"])
def test_both_forms_give_the_same_bits_over_rounds_1_to_6(entry, beta):
    model, o, dn, alpha, beta_ = _scene("fp32" if entry == "fp32" else "mixed", beta)
    surf, _ = model.packed()
    if entry == "fp32":
        blob, prec, kw = surf, 0, {}
    else:
        blob, prec = model.packed_sampler()
        kw = dict(escalate=(surf, 1), guard=0.005, late_round=0)
    pick, rounds = _rays_over_all_rounds(blob, prec, o, dn, alpha, beta_, **kw)
    o70, dn70 = o[pick].contiguous(), dn[pick].contiguous()
    ref = _run("ref", blob, prec, o70, dn70, alpha, beta_, **kw)
    new = _run("new", blob, prec, o70, dn70, alpha, beta_, **kw)
    hist = {int(r): int((rounds == r).sum()) for r in rounds.unique()}
    print(f"  {entry}, beta {beta}: rays per number of rounds (7 = never converged) {hist}; escalated {new[3]}")
    # not vacuous: a ray that takes three rounds has been merged to 1,024 samples (the 16-interval register scan), 1,536 (24) and 2,048 (generic)
    assert bool((rounds >= 3).any()), hist
    assert bool(torch.isfinite(new[0]).all())
    assert _bits_equal(ref, new)
    if entry == "guarded":                       # the late-round rule leaves the last round without its bisection: still the earlier form's bits
        kw3 = dict(kw, late_round=3)
        assert _bits_equal(_run("ref", blob, prec, o70, dn70, alpha, beta_, **kw3), _run("new", blob, prec, o70, dn70, alpha, beta_, **kw3))


@pytest.mark.parametrize("beta", [0.01, 0.002])
def test_nan_prefilled_workspace(beta):
    from nerfart_amd import hip
    model, o, dn, alpha, beta_ = _scene("mixed", beta)
    surf, _ = model.packed()
    blob, prec = model.packed_sampler()
    kw = dict(escalate=(surf, 1), guard=0.005, late_round=3)
    pick, _ = _rays_over_all_rounds(blob, prec, o, dn, alpha, beta_, **kw)
    pick = pick[-5:]                                                           # the five rays with the most rounds
    o5, dn5 = o[pick].contiguous(), dn[pick].contiguous()
    ref = _run("ref", blob, prec, o5, dn5, alpha, beta_, **kw)
    hip._ws_cache.clear()
    nb = int(hip.lib.nerfart_volsdf_sampler_workspace_bytes(5, 512, 512, 64, MAX_ITER))
    hip._workspace(nb, DEV).view(torch.int32).fill_(-1)                        # 0xffffffff: NaN as fp32
    new = _run("new", blob, prec, o5, dn5, alpha, beta_, **kw)
    assert hip._workspace(nb, DEV).numel() == nb, "the run used the workspace filled above"
    assert bool(torch.isfinite(new[0]).all()) and bool(torch.isfinite(new[1]).all())
    assert _bits_equal(ref, new)


def test_a_row_on_which_lanes_own_no_interval():
    """n_init = n_up = 8: 15 intervals after the first merge, one per lane, lanes 15 to 63 own none; 23, 31, ... in the later rounds."""
    model, o, dn, alpha, beta_ = _scene("fp32", 0.01)
    surf, _ = model.packed()
    for ray in (0, 200):
        o1, dn1 = o[ray:ray + 1].contiguous(), dn[ray:ray + 1].contiguous()
        ref = _run("ref", surf, 0, o1, dn1, alpha, beta_, n_init=8, n_up=8)
        new = _run("new", surf, 0, o1, dn1, alpha, beta_, n_init=8, n_up=8)
        assert _bits_equal(ref, new)
