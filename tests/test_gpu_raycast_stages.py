"""The surface renderer's per-ray stage entry points (nerfart_first_crossing, _secant_update, _root_finish, _sphere_trace_step), nerfart_get_rays
and nerfart_normalize_dirs against the exact rule and the fp64 references of tests/raycast_ref.py, one stage at a time, on the case matrix
tests/test_raycast_ref.py runs the float32 stand-in and its mutants through on the CPU; then the stages chained on an analytic surface, with
the SDF evaluated on the host.  Called through hip.lib and ctypes; every helper is local.  One line per case."""
import numpy as np
import pytest
import torch

import raycast_ref as RC
import test_raycast_ref as T

pytestmark = pytest.mark.gpu


def _lib():
    from nerfart_amd import hip
    return hip


def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _back(bufs):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items() if v is not None}


def _bufs(c, inputs):
    b = {k: _dev(c[k]) for k in inputs}
    b.update({k: _dev(v) for k, v in c["out"].items()})
    return b


def _run_first_crossing(c, n_rays=None):
    hip = _lib()
    b = _bufs(c, ("val", "depth"))
    rc = hip.lib.nerfart_first_crossing(_ptr(b["val"]), _ptr(b["depth"]), c["n_rays"] if n_rays is None else n_rays, c["n"], float(c["tau"]),
                                        _ptr(b["mask"]), _ptr(b["mask_sc"]), _ptr(b["mask0"]), _ptr(b["bracket"]), _ptr(b["d_pred"]), _stream())
    hip._check(rc, "first_crossing")
    return _back(b)


def _run_secant(c, n_rays=None):
    hip = _lib()
    b = _bufs(c, ("f_mid", "mask"))
    rc = hip.lib.nerfart_secant_update(_ptr(b["f_mid"]), c["n_rays"] if n_rays is None else n_rays, float(c["tau"]), _ptr(b["mask"]),
                                       _ptr(b["bracket"]), _ptr(b["d_pred"]), _stream())
    hip._check(rc, "secant_update")
    return _back(b)


def _run_root_finish(c, n_rays=None):
    hip = _lib()
    b = _bufs(c, ("rays_o", "rays_dn", "mask", "mask0", "d_pred", "far"))
    rc = hip.lib.nerfart_root_finish(_ptr(b["rays_o"]), _ptr(b["rays_dn"]), c["n_rays"] if n_rays is None else n_rays, _ptr(b["mask"]),
                                     _ptr(b["mask0"]), _ptr(b["d_pred"]), _ptr(b["far"]), float(c["far_s"]), c["fill_inf"], _ptr(b["d_out"]),
                                     _ptr(b["pt"]), _stream())
    hip._check(rc, "root_finish")
    return _back(b)


def _run_sphere_step(c, n_rays=None):
    hip = _lib()
    b = _bufs(c, ("sdf", "far"))
    rc = hip.lib.nerfart_sphere_trace_step(_ptr(b["sdf"]), c["n_rays"] if n_rays is None else n_rays, _ptr(b["far"]), float(c["far_s"]), _ptr(b["d"]),
                                           _ptr(b["mask"]), _stream())
    hip._check(rc, "sphere_trace_step")
    return _back(b)


def _run_get_rays(c, n=None):
    hip = _lib()
    b = _bufs(c, ("pose", "K", "select"))
    rc = hip.lib.nerfart_get_rays(_ptr(b["pose"]), _ptr(b["K"]), c["H"], c["W"], _ptr(b["select"]), c["n"] if n is None else n, _ptr(b["rays_o"]),
                                  _ptr(b["rays_d"]), _stream())
    hip._check(rc, "get_rays")
    return _back(b)


def _run_normalize(c, n=None):
    hip = _lib()
    b = _bufs(c, ("x",))
    rc = hip.lib.nerfart_normalize_dirs(_ptr(b["x"]), _ptr(b["out"]), c["n"] if n is None else n, _stream())
    hip._check(rc, "normalize_dirs")
    return _back(b)


RUN = {"first_crossing": _run_first_crossing, "secant_update": _run_secant, "root_finish": _run_root_finish, "sphere_step": _run_sphere_step,
       "get_rays": _run_get_rays, "normalize": _run_normalize}


def _report(reps):
    for r in reps:
        print(r.line())
    bad = [r.line() for r in reps if r.fail]
    assert not bad, bad


def _run_stage(stage):
    _report([RC.CHECK[stage](c, RUN[stage](c)) for c in RC.CASES[stage]()])


def test_first_crossing_is_the_exact_rule():
    """The 64-lane strided scan and its (cost, index) reduction at N below, at and above 64, R off the 4 rays of a block, exact zeros, the
    strict 'starts outside', tau deciding a sign, per-ray depth rows: masks and brackets bit for bit, the first estimate within its bound."""
    _run_stage("first_crossing")


def test_secant_update_is_the_exact_rule():
    _run_stage("secant_update")


def test_root_finish_fill_values_and_points():
    _run_stage("root_finish")


def test_sphere_trace_step_is_bit_exact():
    _run_stage("sphere_step")


def test_get_rays_against_fp64():
    _run_stage("get_rays")


def test_normalize_dirs_against_fp64():
    _run_stage("normalize")


def test_zero_rays_return_0_and_touch_nothing():
    """n_rays == 0 (n == 0): every entry point returns 0 before any launch; inputs, outputs and in / out state keep their bytes."""
    for stage in sorted(RUN):
        c = RC.CASES[stage]()[-1]
        got = RUN[stage](c, 0)                       # _check raises on a non-zero return
        for k, v in c["out"].items():
            assert np.array_equal(got[k].view(np.uint8), v.view(np.uint8)), (stage, k)
        for k, v in got.items():
            if k not in c["out"]:
                assert np.array_equal(v.view(np.uint8), np.ascontiguousarray(c[k]).view(np.uint8)), (stage, k)
        print(f"  {stage}: 0 rays -> 0, nothing written")


@pytest.mark.parametrize("surface", RC.SURFACES)
def test_root_finding_chain_on_an_analytic_surface(surface):
    """first_crossing -> 8 x secant_update -> root_finish on a unit sphere / a union of two spheres along the ray axis (two crossings, a
    start-inside subset), 1027 rays, N_steps 64 and 257, tau 0 and 0.02; f_mid is the fp64 surface at the kernel's own d_pred, rounded to
    fp32.  Every step passes the per-stage check from the kernel's own previous state.  At the end |sdf(o + d dn) - tau| of the hit rays is
    at most 4 x the largest residual the float32 stand-in of tests/test_raycast_ref.py reaches on the same rays (the factor allows for a
    differently rounded last step; it is no measurement of the kernel).  The stand-in's residual is printed on the case line; on the CPU it is
    1.2e-7 on the unit sphere (half an ulp of a depth near 2) and between 8e-8 and 6.5e-7 on the union."""
    for N in RC.CHAIN_N:
        for tau in RC.FC_TAU:
            reps, res, hit = RC.chain_root_finding(RUN, surface, N, tau)
            _, res_ref, hit_ref = RC.chain_root_finding(T.standin(), surface, N, tau)
            print(f"  chain {surface} N={N} tau={tau:g}: {int(hit.sum())} of {len(hit)} rays hit, largest residual {res.max():.3g} "
                  f"(stand-in {res_ref.max():.3g})")
            _report(reps)
            assert np.array_equal(hit, hit_ref), "the kernels and the stand-in hit different rays"
            assert res.max() <= 4 * res_ref.max(), (float(res.max()), float(res_ref.max()))


def test_sphere_tracing_chain_on_the_unit_sphere():
    """20 x sphere_trace_step with host-evaluated values: d and the mask bit-equal to the restatement after every step."""
    reps, d, mask = RC.chain_sphere_tracing(RUN)
    print(f"  sphere tracing: {int(mask.sum())} of {len(mask)} rays alive after {len(reps)} steps")
    _report(reps)
    _, d_ref, mask_ref = RC.chain_sphere_tracing(T.standin())
    assert RC.same_bits(d, d_ref) and np.array_equal(mask, mask_ref)
