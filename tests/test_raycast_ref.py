"""CPU self-tests of tests/raycast_ref.py: the checkers accept a float32 NumPy / torch stand-in of each entry point, written independently
of the checkers' rule (the reference's cost matrix and min for the first crossing, a matrix product for the rays, F.normalize), on every case
of the GPU matrix of tests/test_gpu_raycast_stages.py, and they refuse the stand-in with each of the bugs these kernels invite switched on,
one at a time.  The stand-ins and their mutants live here, never in product code."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import raycast_ref as RC


class Mut:
    last_crossing = False     # the last sign change in place of the first
    start_ge = False          # "starts outside" with >= 0
    f_high_ge = False         # "outside -> inside" with f_high >= 0
    zero_crossing = False     # an exact zero counted as a crossing: (a > 0) != (b > 0)
    no_tau = False            # tau ignored
    depth_row0 = False        # every ray's depths read from ray 0's row
    secant_le = False         # the secant's low side with f_mid <= 0
    secant_all = False        # the secant updates unmasked rays too
    no_inside_zero = False    # root_finish without the 0 of rays that start inside
    fill_far = False          # root_finish fills far although fill_inf is set
    step_ge = False           # the sphere step kills a ray at d >= far
    step_dead = False         # the sphere step moves dead rays
    half_pixel = False        # get_rays with a half-pixel offset
    swap_ij = False           # get_rays with column and row swapped
    no_skew = False           # get_rays without the skew
    no_clamp = False          # normalize without the 1e-12 clamp

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Mut, k), k
            setattr(self, k, v)


def _out(case):
    return {k: v.copy() for k, v in case["out"].items()}


def _secant32(d_low, f_low, d_high, f_high):
    with np.errstate(all="ignore"):
        return (-f_low * (d_high - d_low) / (f_high - f_low) + d_low).astype(np.float32)


def run_first_crossing(case, m):
    """ray_casting.py:91-126: sign(v_i v_{i+1}) (N - i) with a last column of ones, min over the row."""
    o = _out(case)
    R, N = case["n_rays"], case["n"]
    val, depth = case["val"], case["depth"]
    with np.errstate(all="ignore"):
        v = val if m.no_tau else val - case["tau"]
        if m.zero_crossing:
            sign = np.where((v[:, :-1] > 0) != (v[:, 1:] > 0), -1.0, 1.0).astype(np.float32)
        else:
            sign = np.sign(v[:, :-1] * v[:, 1:])
    weight = np.arange(1, N, dtype=np.float32) if m.last_crossing else np.arange(N, 1, -1, dtype=np.float32)
    cost = np.concatenate([sign * weight, np.ones((R, 1), np.float32)], -1)
    idx = cost.argmin(-1)
    sc = cost.min(-1) < 0
    idx2 = np.minimum(idx + 1, N - 1)
    rows = np.arange(R)
    drow = np.zeros(R, np.int64) if m.depth_row0 else rows
    f_high, f_low, d_high, d_low = v[rows, idx], v[rows, idx2], depth[drow, idx], depth[drow, idx2]
    m0 = v[:, 0] >= 0 if m.start_ge else v[:, 0] > 0
    mask = sc & (f_high >= 0 if m.f_high_ge else f_high > 0) & m0
    o["mask"][:R], o["mask_sc"][:R], o["mask0"][:R] = mask, sc, m0
    o["bracket"][:R] = np.stack([d_low, f_low, d_high, f_high], -1)
    o["d_pred"][:R] = np.where(mask, _secant32(d_low, f_low, d_high, f_high), np.float32(1.0))
    return o


def run_secant(case, m):
    """run_secant_method's loop body (ray_casting.py:17-29) on the rays of the mask."""
    o = _out(case)
    R = case["n_rays"]
    f_mid = case["f_mid"] - case["tau"]
    for r in range(R):
        if not (case["mask"][r] or m.secant_all):
            continue
        d_low, f_low, d_high, f_high = o["bracket"][r]
        if (f_mid[r] <= 0) if m.secant_le else (f_mid[r] < 0):
            d_low, f_low = o["d_pred"][r], f_mid[r]
        else:
            d_high, f_high = o["d_pred"][r], f_mid[r]
        o["bracket"][r] = d_low, f_low, d_high, f_high
        o["d_pred"][r] = _secant32(*o["bracket"][r])
    return o


def run_root_finish(case, m):
    """ray_casting.py:137-152 with torch's masked assignments."""
    o = _out(case)
    R = case["n_rays"]
    mask, m0 = torch.as_tensor(case["mask"]).bool(), torch.as_tensor(case["mask0"]).bool()
    d_pred, ro, dn = torch.as_tensor(case["d_pred"]), torch.as_tensor(case["rays_o"]), torch.as_tensor(case["rays_dn"])
    pt = torch.ones(R, 3)
    pt[mask] = ro[mask] + dn[mask] * d_pred[mask][:, None]
    d_out = torch.ones(R)
    d_out[mask] = d_pred[mask]
    far = torch.as_tensor(case["far"]) if case["far"] is not None else torch.full((R,), float(case["far_s"]))
    if case["fill_inf"] and not m.fill_far:
        d_out[~mask] = float("inf")
    else:
        d_out[~mask] = far[~mask]
    if not m.no_inside_zero:
        d_out[~m0] = 0.0
    o["d_out"][:R], o["pt"][:R] = d_out.numpy(), pt.numpy()
    return o


def run_sphere_step(case, m):
    """ray_casting.py:175-180."""
    o = _out(case)
    R = case["n_rays"]
    d, mask = torch.as_tensor(o["d"][:R].copy()), torch.as_tensor(o["mask"][:R].copy()).bool()
    sdf = torch.as_tensor(case["sdf"])
    far = torch.as_tensor(case["far"]) if case["far"] is not None else torch.full((R,), float(case["far_s"]))
    if m.step_dead:
        d = d + sdf
    else:
        d[mask] += sdf[mask]
    mask[(d >= far) if m.step_ge else (d > far)] = False
    mask[d < 0] = False
    o["d"][:R], o["mask"][:R] = d.numpy(), mask.numpy()
    return o


def run_get_rays(case, m):
    """rend_util.py:112-165: the pixel grid lifted through the intrinsics, a float32 matrix product with the pose."""
    o = _out(case)
    H, W, n = case["H"], case["W"], case["n"]
    K, P = case["K"], case["pose"]
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    i, j = ii.reshape(-1), jj.reshape(-1)
    if case["select"] is not None:
        i, j = i[case["select"]], j[case["select"]]
    if m.swap_ij:
        i, j = j, i
    if m.half_pixel:
        i, j = i + np.float32(0.5), j + np.float32(0.5)
    fx, fy, cx, cy, sk = K[0, 0], K[1, 1], K[0, 2], K[1, 2], (np.float32(0) if m.no_skew else K[0, 1])
    x = (i - cx + cy * sk / fy - sk * j / fy) / fx
    y = (j - cy) / fy
    cam = np.stack([x, y, np.ones_like(x), np.ones_like(x)], 0).astype(np.float32)
    world = (P @ cam).T[:, :3]
    o["rays_d"][:n] = world - P[:3, 3][None]
    o["rays_o"][:n] = P[:3, 3][None]
    return o


def run_normalize(case, m):
    o = _out(case)
    x = torch.as_tensor(case["x"])
    with np.errstate(all="ignore"):
        o["out"][:case["n"]] = (x / x.norm(dim=-1, keepdim=True)).numpy() if m.no_clamp else F.normalize(x, dim=-1).numpy()
    return o


RUN = {"first_crossing": run_first_crossing, "secant_update": run_secant, "root_finish": run_root_finish, "sphere_step": run_sphere_step,
       "get_rays": run_get_rays, "normalize": run_normalize}


def standin(m=None):
    """stage -> callable(case) -> outputs, as raycast_ref's chains take it."""
    m = m or Mut()
    return {stage: (lambda case, f=f: f(case, m)) for stage, f in RUN.items()}


def run_stage(stage, m):
    return [RC.CHECK[stage](c, RUN[stage](c, m)) for c in RC.CASES[stage]()]


@pytest.mark.parametrize("stage", sorted(RUN))
def test_standin_passes_every_case(stage):
    reps = run_stage(stage, Mut())
    for r in reps:
        print(r.line())
    assert not [r for r in reps if r.fail], [r.line() for r in reps if r.fail]


def test_case_matrix_holds_every_row_kind():
    """The first-crossing matrix really contains each row kind with its deciding index at 0, 62, 63, 64, 65 and N - 2."""
    seen = set()
    for c in RC.first_crossing_cases():
        for e in c["expect"]:
            seen.add((e[0], e[4] if e[4] is None else (int(e[4]), int(e[4]) == c["n"] - 2)))
    kinds = {k for k, _ in seen}
    assert kinds == set(RC.FC_KINDS), kinds
    for kind in ("a", "b", "d", "g"):
        at = {p[0] for k, p in seen if k == kind and p is not None}
        assert {0, 62, 63, 64, 65} <= at and any(p[1] for k, p in seen if k == kind and p is not None), (kind, sorted(at))


MUTANTS = {
    "last_crossing": "first_crossing", "start_ge": "first_crossing", "zero_crossing": "first_crossing", "no_tau": "first_crossing",
    "depth_row0": "first_crossing", "secant_le": "secant_update", "secant_all": "secant_update", "no_inside_zero": "root_finish",
    "fill_far": "root_finish", "step_ge": "sphere_step", "step_dead": "sphere_step", "half_pixel": "get_rays", "swap_ij": "get_rays",
    "no_skew": "get_rays", "no_clamp": "normalize",
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_is_rejected(name):
    reps = run_stage(MUTANTS[name], Mut(**{name: True}))
    failed = [r for r in reps if r.fail]
    print(f"  mutant {name}: rejected by {len(failed)} of {len(reps)} cases" + (f", e.g. {failed[0].name}: {failed[0].fail[0][:120]}" if failed else ""))
    assert failed, f"mutant {name} passed every case"


def test_f_high_ge_is_the_same_function():
    """'f_high >= 0' for 'f_high > 0' cannot be told apart by any input: mask needs a sign change, a sign change needs a product
    v_i v_{i+1} < 0, and that needs f_high = v_i != 0.  So this mutant is no bug; the test pins that down (its outputs are bit-equal to the
    stand-in's on the whole matrix) instead of asking for a rejection that no case could deliver."""
    for c in RC.first_crossing_cases():
        a, b = run_first_crossing(c, Mut()), run_first_crossing(c, Mut(f_high_ge=True))
        assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a), c["name"]


@pytest.mark.parametrize("surface", RC.SURFACES)
def test_root_finding_chain_on_an_analytic_surface(surface):
    """first_crossing -> 8 x secant_update -> root_finish of the stand-in, every step checked from its own previous state; the residual
    |sdf - tau| of the hit points is what the GPU test measures the kernels against (about 1.2e-7 on the unit sphere: half an ulp of a
    depth near 2)."""
    for N in RC.CHAIN_N:
        for tau in RC.FC_TAU:
            reps, res, hit = RC.chain_root_finding(standin(), surface, N, tau)
            bad = [r.line() for r in reps if r.fail]
            inside = int((~reps[0].start_outside).sum())
            print(f"  chain {surface} N={N} tau={tau:g}: {int(hit.sum())} of {len(hit)} rays hit, {inside} start inside, largest residual "
                  f"{res.max():.3g}, worst d_pred error {max(r.worst for r in reps[:-1]):.2f} of its bound")
            assert not bad, bad
            assert (inside > 20) == (surface == "two_spheres")
            assert hit.sum() > len(hit) // 5 and (~hit).sum() > 20 and res.max() < 1e-5


def test_sphere_tracing_chain_on_the_unit_sphere():
    reps, d, mask = RC.chain_sphere_tracing(standin())
    bad = [r.line() for r in reps if r.fail]
    print(f"  sphere tracing: {int(mask.sum())} of {len(mask)} rays alive after {len(reps)} steps")
    assert not bad, bad
    o, dn, _, _ = RC.chain_rays("sphere")
    assert mask.sum() > len(mask) // 4 and (~mask).sum() > 20
    assert np.median(np.abs(RC.sdf_at("sphere", o, dn, d)[mask])) < 1e-6       # the bulk sits on the surface; grazing rays still creep
