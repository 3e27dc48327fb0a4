"""nerfart_volsdf_composite_geo_bwd (k_composite_volsdf_geo_bwd: the VolSDF compositor's backward w.r.t. its depth and normals maps) against the fp64
reference and error model of tests/geo_bwd_ref.py, through hip.volsdf_composite_geo_bwd, on the case matrix tests/test_geo_bwd_ref.py runs the float32
statement and its mutants through on the CPU.  Four variants per case: depth only, normals only, both, and both with accumulate = 1 onto a preloaded
g_sdf, a g_n_in, and g_alpha_beta preloaded with composite_ref.PRELOAD (the all-empty-rays case: normals only and the accumulate variant without a depth
cotangent).  Every output buffer starts from a sentinel: what a variant must not write keeps it.  One line per run, then the worst observed / bound
ratio per output over the whole matrix (1.00 = the bound, SAFETY = 2 times the first-order model).

Worst observed / bound on an MI355X (gfx950), every run passed:  g_sdf 0.23  g_nabla 0.17  d/d alpha 0.01  d/d beta 0.01;  in the accumulate variant
(the last operation is one addition onto an O(1) preload: half an ulp against a bound of one)  g_sdf 0.49  g_nabla 0.49  d/d alpha 0.03  d/d beta 0.06."""
import numpy as np
import pytest
import torch

import composite_ref as CR
import geo_bwd_ref as G

pytestmark = pytest.mark.gpu

SENT = np.float32(-7.25)


def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _out(shape, init=None):
    """A device buffer of one more row than the output: SENT (or the preload) in the rows, SENT in the extra row, which must stay untouched."""
    t = torch.full((shape[0] + 1,) + tuple(shape[1:]), float(SENT), dtype=torch.float32, device="cuda")
    if init is not None:
        t[:-1] = _dev(init)
    return t


def run_variant(c, gi, variant):
    from nerfart_amd import hip
    gd, gn, accumulate = G.variant_cotangents(c, gi, variant)
    R, P = c["n_rays"], c["P"]
    inp = dict(d=_dev(c["d"]), sdf=_dev(c["sdf"]), nabla=_dev(gi["nabla"]), g_depth=_dev(gd), g_normals=_dev(gn),
               g_n_in=_dev(gi["g_n_in"]) if accumulate else None)
    g_sdf = _out((R, P), gi["g_sdf0"] if accumulate else None)
    g_nabla = _out((R, P, 3))
    g_ab = _dev((CR.PRELOAD if accumulate else np.zeros(2, np.float32)).copy())
    ret = hip.volsdf_composite_geo_bwd(inp["d"], inp["sdf"], float(c["alpha"]), float(c["beta"]), g_depth=inp["g_depth"], g_normals=inp["g_normals"],
                                       nabla=inp["nabla"], g_n_in=inp["g_n_in"], g_sdf=g_sdf[:-1], g_nabla=g_nabla[:-1], g_alpha_beta=g_ab,
                                       accumulate=accumulate)
    torch.cuda.synchronize()
    side = []
    if not (bool((g_sdf[-1] == float(SENT)).all()) and bool((g_nabla[-1] == float(SENT)).all())):
        side.append("a row past the last ray was written")
    if gn is None:
        if not bool((g_nabla == float(SENT)).all()):
            side.append("depth only: g_nabla was written")
        if ret[1] is not None:
            side.append("depth only: the wrapper returned a g_nabla")
    src = dict(d=c["d"], sdf=c["sdf"], nabla=gi["nabla"], g_depth=gd, g_normals=gn, g_n_in=gi["g_n_in"] if accumulate else None)
    for k, t in inp.items():
        if t is not None and not CR.same_bits(t.cpu().numpy(), src[k]):
            side.append(f"input {k} changed")
    o = dict(g_sdf=g_sdf[:-1].cpu().numpy(), g_nabla=None if gn is None else g_nabla[:-1].cpu().numpy(), g_ab=g_ab.cpu().numpy())
    return o, side


def test_geo_backward_against_fp64_on_every_case_and_variant():
    reps, worst = [], {}
    for c, gi, refs in G.references():
        for v in G.variants_of(c):
            o, side = run_variant(c, gi, v)
            rep = G.check(c, gi, v, o, refs[v])
            for msg in side:
                rep.check(False, msg)
            print(rep.line())
            for k, r in rep.ratio.items():
                worst[k] = max(worst.get(k, 0.0), r)
            reps.append(rep)
    print("  WORST k_composite_volsdf_geo_bwd: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    bad = [r.line() for r in reps if r.fail]
    assert not bad, bad


def test_refused_and_empty_calls_write_nothing():
    from nerfart_amd import hip
    c = G.cases()[8]
    gi = G.geo_inputs(c)
    R, P = c["n_rays"], c["P"]
    d, sdf, nab, gd, gn = (_dev(x) for x in (c["d"], c["sdf"], gi["nabla"], gi["g_depth"], gi["g_normals"]))
    g_sdf, g_nabla, g_ab = _out((R, P)), _out((R, P, 3)), _dev(CR.PRELOAD.copy())
    with pytest.raises(hip.NerfartHipError, match="both are NULL"):
        hip.volsdf_composite_geo_bwd(d, sdf, 10.0, 0.1, g_sdf=g_sdf[:-1], g_alpha_beta=g_ab)
    with pytest.raises(hip.NerfartHipError, match="needs nabla and g_nabla"):
        hip.volsdf_composite_geo_bwd(d, sdf, 10.0, 0.1, g_normals=gn, g_sdf=g_sdf[:-1], g_nabla=g_nabla[:-1], g_alpha_beta=g_ab)
    z = torch.zeros(0, P, device="cuda")
    hip.volsdf_composite_geo_bwd(z, z, 10.0, 0.1, g_depth=torch.zeros(0, device="cuda"), g_sdf=g_sdf[:0], g_alpha_beta=g_ab)      # no rays: a no-op
    torch.cuda.synchronize()
    assert bool((g_sdf == float(SENT)).all()) and bool((g_nabla == float(SENT)).all()), "a refused or empty call wrote to an output"
    assert CR.same_bits(g_ab.cpu().numpy(), CR.PRELOAD), "a refused or empty call touched the accumulator"
    assert gd is not None and nab is not None
