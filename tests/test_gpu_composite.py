"""The four compositing entry points - nerfart_volsdf_composite, nerfart_neus_composite and their backwards - against the fp64 references and the error
model of tests/composite_ref.py, on the case matrix tests/test_composite_ref.py runs the float32 oracle, the fp32 stand-in and its mutants through on the
CPU.  Called through hip.lib and ctypes with local helpers (the hip.volsdf_composite wrapper hides normals and the detail outputs).  One line per case:
rays, gradient elements, non-strict elements, rays of unknown depth, and the worst observed / bound ratio per output (1.00 = the bound).

Worst observed / bound ratio per kernel and output over the whole matrix on an MI355X (gfx950; 1.00 = the bound, which is SAFETY = 2 times the
first-order model; every case passed, every exact check held bit for bit):
  k_composite_volsdf      rgb 0.15  acc 0.05  depth 0.04  normals 0.07  sigma_out 0.47  p_out 0.23  tau_out 0.17
  k_composite_volsdf_bwd  g_sdf 0.20  g_rad 0.17  d/d alpha 0.04  d/d beta 0.01
  k_composite_neus        rgb 0.07  acc 0.08  depth 0.03  normals 0.09  cdf_out 0.38  alpha_out 0.33  w_out 0.31  d_mid_out 0.50 (of 1 ulp)
  k_composite_neus_bwd    g_sdf 0.50  g_rad 0.50  d/d s 0.07
(0.50 on a single product or rounding is half an ulp against a bound of one.)
"""
import numpy as np
import pytest
import torch

import composite_ref as CR
from composite_ref import F

pytestmark = pytest.mark.gpu

SENT = np.float32(-7.25)          # output buffers start with it; whatever a call must not touch keeps it


def _lib():
    from nerfart_amd import hip
    return hip


def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(shape, want=True):
    """A device buffer of one more row than the output, all SENT: the extra row must stay untouched."""
    if not want:
        return None
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), float(SENT), dtype=torch.float32, device="cuda")


def _host(t):
    return None if t is None else t[:-1].cpu().numpy()


def _guard_ok(bufs):
    return all(b is None or bool((b[-1] == float(SENT)).all()) for b in bufs.values())


def run_case(c):
    """-> (outputs as composite_ref.check takes them, list of failed side conditions)."""
    hip = _lib()
    lib, side = hip.lib, []
    R, P, fw, white = c["n_rays"], c["P"], c["fw"], int(c["white"])
    names = ("d", "sdf", "rad", "nabla", "g_rgb", "g_acc")
    inp = {k: _dev(c[k]) for k in names}
    want = c["want"]
    normals = c["nabla"] is not None
    if fw == "volsdf":
        o = dict(rgb=_out((R, 3)), depth=_out((R,)), acc=_out((R,)), normals=_out((R, 3), normals), sigma=_out((R, P), want["sigma"]),
                 p=_out((R, P - 1), want["p"]), tau=_out((R, P - 1), want["tau"]))
        rc = lib.nerfart_volsdf_composite(R, P, _ptr(inp["d"]), _ptr(inp["sdf"]), _ptr(inp["rad"]), _ptr(inp["nabla"]), float(c["alpha"]), float(c["beta"]),
                                          white, _ptr(o["rgb"]), _ptr(o["depth"]), _ptr(o["acc"]), _ptr(o["normals"]), _ptr(o["sigma"]), _ptr(o["p"]),
                                          _ptr(o["tau"]), _stream())
        hip._check(rc, "nerfart_volsdf_composite")
    else:
        o = dict(rgb=_out((R, 3)), depth=_out((R,)), acc=_out((R,)), normals=_out((R, 3), normals), cdf=_out((R, P), want["cdf"]),
                 alpha=_out((R, P - 1), want["alpha"]), w=_out((R, P - 1), want["w"]), d_mid=_out((R, P - 1), want["d_mid"]))
        rc = lib.nerfart_neus_composite(R, P, _ptr(inp["d"]), _ptr(inp["sdf"]), _ptr(inp["rad"]), _ptr(inp["nabla"]), float(c["s"]), white, _ptr(o["rgb"]),
                                        _ptr(o["depth"]), _ptr(o["acc"]), _ptr(o["normals"]), _ptr(o["cdf"]), _ptr(o["alpha"]), _ptr(o["w"]), _ptr(o["d_mid"]),
                                        _stream())
        hip._check(rc, "nerfart_neus_composite")
    torch.cuda.synchronize()
    key = "g_ab" if fw == "volsdf" else "g_s"
    b = dict(g_sdf=_out((R, P)), g_rad=_out((R, P if fw == "volsdf" else P - 1, 3)))
    acc_buf = _dev(c["preload"].copy()) if want[key] else None

    def bwd():
        if fw == "volsdf":
            return lib.nerfart_volsdf_composite_bwd(R, P, _ptr(inp["d"]), _ptr(inp["sdf"]), _ptr(inp["rad"]), float(c["alpha"]), float(c["beta"]), white,
                                                    _ptr(inp["g_rgb"]), _ptr(inp["g_acc"]), _ptr(b["g_sdf"]), _ptr(b["g_rad"]), _ptr(acc_buf), _stream())
        return lib.nerfart_neus_composite_bwd(R, P, _ptr(inp["sdf"]), _ptr(inp["rad"]), float(c["s"]), white, _ptr(inp["g_rgb"]), _ptr(inp["g_acc"]),
                                              _ptr(b["g_sdf"]), _ptr(b["g_rad"]), _ptr(acc_buf), _stream())
    rc = bwd()
    torch.cuda.synchronize()
    if P <= 513:
        hip._check(rc, "composite_bwd")
    else:
        # only the backward refuses these rows (its per-lane arrays hold 8 intervals): 2, the documented message, nothing written
        if not (rc == 2 and b"2 <= P <= 513" in lib.nerfart_last_error()):
            side.append(f"the backward did not refuse P = {P}: rc {rc}, {lib.nerfart_last_error()!r}")
        if not (bool((b["g_sdf"] == float(SENT)).all()) and bool((b["g_rad"] == float(SENT)).all())):
            side.append("a refused backward wrote to its outputs")
    if not _guard_ok(o) or not _guard_ok(b):
        side.append("a row past the last ray was written")
    for k in names:
        if c[k] is not None and not CR.same_bits(inp[k].cpu().numpy(), c[k]):
            side.append(f"input {k} changed")
    out = {k: _host(v) for k, v in o.items()}
    if P <= 513:
        out.update(g_sdf=_host(b["g_sdf"]), g_rad=_host(b["g_rad"]))
        out[key] = None if acc_buf is None else acc_buf.cpu().numpy()
    return out, side


def exact_contract(c, o):
    """What is exact by construction: the forward's weights re-derived from its own p_out / alpha_out in the kernels' order (lane segments, shuffle scan,
    second pass - products only, nothing a compiler may contract), and the backward's implied forward: g_rad = tau g_rgb of the SAME tau, to 1 ulp."""
    bad = []
    fac_key, w_key = ("p", "tau") if c["fw"] == "volsdf" else ("alpha", "w")
    if o.get(fac_key) is not None and o.get(w_key) is not None:
        if c["fw"] == "volsdf":
            p = o["p"]
            mine = (((F(1) - p) + F(1e-10)).astype(F) * CR.scan_T(p)).astype(F)
        else:
            a = o["alpha"]
            mine = (a * CR.scan_T(((F(1) - a) + F(1e-10)).astype(F))).astype(F)
        if not CR.same_bits(mine, o[w_key]):
            bad.append(f"{w_key}_out is not {fac_key}_out's own scan: {int((CR.bits(mine) != CR.bits(o[w_key])).sum())} elements differ")
    if c["P"] <= 513 and o.get(w_key) is not None:
        n = c["P"] - 1
        want = (o[w_key][..., None] * c["g_rgb"][:, None, :]).astype(F)
        if not np.all(np.abs(o["g_rad"][:, :n].astype(np.float64) - want) <= CR.ulp32(want)):
            bad.append("g_rad is not the forward's own tau_out x g_rgb within 1 ulp")
    return bad


def _run_matrix(cases, kernel):
    reps, worst = [], {}
    for c in cases:
        o, side = run_case(c)
        rep = CR.check(c, o)
        for msg in side + exact_contract(c, o):
            rep.check(False, msg)
        print(rep.line())
        for k, v in rep.ratio.items():
            worst[k] = max(worst.get(k, 0.0), v)
        reps.append(rep)
    print(f"  WORST {kernel}: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    bad = [r.line() for r in reps if r.fail]
    assert not bad, bad


def test_volsdf_composite_and_backward_against_fp64():
    _run_matrix(CR.volsdf_cases(), "volsdf")


def test_neus_composite_and_backward_against_fp64():
    _run_matrix(CR.neus_cases(), "neus")


def test_normals_without_nablas_are_refused_and_an_empty_launch_is_a_no_op():
    hip = _lib()
    lib = hip.lib
    R, P = 4, 66
    c = CR.volsdf_case("refusals", P, 0.013, 1, R=R)
    inp = {k: _dev(c[k]) for k in ("d", "sdf", "rad", "g_rgb")}
    o = {k: _out(s) for k, s in dict(rgb=(R, 3), depth=(R,), acc=(R,), normals=(R, 3), a=(R, P), b=(R, P - 1), c=(R, P - 1), d=(R, P - 1), g_sdf=(R, P),
                                     g_rad=(R, P, 3)).items()}
    ab = _dev(CR.PRELOAD.copy())

    def volsdf(n_rays, nabla):
        return lib.nerfart_volsdf_composite(n_rays, P, _ptr(inp["d"]), _ptr(inp["sdf"]), _ptr(inp["rad"]), nabla, 76.0, 0.013, 0, _ptr(o["rgb"]), _ptr(o["depth"]),
                                            _ptr(o["acc"]), _ptr(o["normals"]), _ptr(o["a"]), _ptr(o["b"]), _ptr(o["c"]), _stream())

    def neus(n_rays, nabla):
        return lib.nerfart_neus_composite(n_rays, P, _ptr(inp["d"]), _ptr(inp["sdf"]), _ptr(inp["rad"]), nabla, 64.0, 0, _ptr(o["rgb"]), _ptr(o["depth"]),
                                          _ptr(o["acc"]), _ptr(o["normals"]), _ptr(o["a"]), _ptr(o["b"]), _ptr(o["c"]), _ptr(o["d"]), _stream())
    for call in (volsdf, neus):
        assert call(R, None) == 2 and b"normals requested without nablas" in lib.nerfart_last_error()
        assert call(0, None) == 0
    assert lib.nerfart_volsdf_composite_bwd(0, P, _ptr(inp["d"]), _ptr(inp["sdf"]), _ptr(inp["rad"]), 76.0, 0.013, 0, _ptr(inp["g_rgb"]), None, _ptr(o["g_sdf"]),
                                            _ptr(o["g_rad"]), _ptr(ab), _stream()) == 0
    assert lib.nerfart_neus_composite_bwd(0, P, _ptr(inp["sdf"]), _ptr(inp["rad"]), 64.0, 0, _ptr(inp["g_rgb"]), None, _ptr(o["g_sdf"]), _ptr(o["g_rad"]), _ptr(ab),
                                          _stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((v == float(SENT)).all()) for v in o.values()), "a refused or empty call wrote to an output"
    assert CR.same_bits(ab.cpu().numpy(), CR.PRELOAD), "an empty backward touched the accumulator"
