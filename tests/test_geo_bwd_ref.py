"""CPU self-tests of tests/geo_bwd_ref.py (the reference and comparator tests/test_gpu_composite_geo.py holds k_composite_volsdf_geo_bwd to): on every
case and variant the comparator accepts a float32 torch statement of the formulas (cumprod / cumsum: another summation order than the kernel's) and
rejects that statement with each of the bugs this kernel invites; the caps (rays of unknown depth, non-strict gradient elements) hold for every case
from the reference alone.  And, without a GPU: the two new entry points refuse bad arguments with 2 before any HIP call.  The statement and its
mutants live here, never in product code."""
import ctypes as C

import numpy as np
import pytest
import torch

import composite_ref as CR
import geo_bwd_ref as G


class Mut:
    no_depth_centre = False     # g_tau = g_normals . n + g_depth / inv d_k: the "- depth" term dropped
    depth_sign = False          # the sign of the depth term flipped
    no_projection = False       # normalize backward without the projection: g_nabla = tau g_normals / |nabla|
    last_tau = False            # the last sample treated as if it carried weight (its g_sdf / g_nabla not zero)
    ignore_accumulate = False   # accumulate != 0 overwrites g_sdf
    no_g_n_in = False           # g_n_in not added into g_nabla
    suffix_inclusive = False    # the suffix sum includes the interval's own term

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Mut, k), k
            setattr(self, k, v)


def _t32(x):
    return torch.as_tensor(np.array(x, np.float32))


def statement32(c, gi, variant, m):
    """The formulas of the issue / the kernel's header in float32 torch, vectorised over rays and samples."""
    gd, gn, accumulate = G.variant_cotangents(c, gi, variant)
    d, s, nab = _t32(c["d"]), _t32(c["sdf"]), _t32(gi["nabla"])
    R, P = d.shape
    al, be = _t32(c["alpha"]), _t32(c["beta"])
    e = 0.5 * torch.exp(-s.abs() / be)
    psi = torch.where(s >= 0, e, 1 - e)
    delta = d[:, 1:] - d[:, :-1]
    x = torch.relu(al * psi[:, :-1] * delta)
    p = torch.exp(-x)
    T = torch.cumprod(torch.cat([torch.ones(R, 1), p], -1), -1)[:, :-1]
    tau = (1 - p + 1e-10) * T
    acc = tau.sum(-1)
    inv = acc + 1e-10
    depth = (tau / inv[:, None] * d[:, :-1]).sum(-1)
    v = nab[:, :-1]
    nrm = v.norm(dim=-1, keepdim=True)
    n = v / nrm.clamp_min(1e-12)
    gtau = torch.zeros(R, P - 1)
    if gn is not None:
        gtau = gtau + (n * _t32(gn)[:, None, :]).sum(-1)
    if gd is not None:
        gdi = (_t32(gd) / inv)[:, None]
        centre = d[:, :-1] if m.no_depth_centre else d[:, :-1] - depth[:, None]
        gtau = gtau + (-gdi if m.depth_sign else gdi) * centre
    h = tau * gtau
    incl = torch.flip(torch.cumsum(torch.flip(h, [-1]), -1), [-1])
    S = incl if m.suffix_inclusive else torch.cat([incl[:, 1:], torch.zeros(R, 1)], -1)
    gx = p * T * gtau - S
    gsig = torch.where(x > 0, gx * delta, torch.zeros(()))
    g_sdf = torch.zeros(R, P)
    g_sdf[:, :-1] = -gsig * al * e[:, :-1] / be
    if m.last_tau:
        g_sdf[:, -1] = g_sdf[:, -2]
    g_ab = torch.stack([(gsig * psi[:, :-1]).sum(), (gsig * al * e[:, :-1] * s[:, :-1] / (be * be)).sum()])
    if accumulate:
        if not m.ignore_accumulate:
            g_sdf = g_sdf + _t32(gi["g_sdf0"])
            if not m.last_tau:
                g_sdf[:, -1] = _t32(gi["g_sdf0"])[:, -1]
        g_ab = g_ab + _t32(CR.PRELOAD)
    o = dict(g_sdf=g_sdf.numpy(), g_ab=g_ab.numpy(), g_nabla=None)
    if gn is not None:
        g3 = _t32(gn)[:, None, :]
        proj = g3.expand(R, P - 1, 3) if m.no_projection else g3 - n * (n * g3).sum(-1, keepdim=True)
        inner = tau[..., None] * torch.where(nrm >= 1e-12, proj / nrm.clamp_min(1e-30), g3 / 1e-12)
        g_nabla = torch.zeros(R, P, 3)
        g_nabla[:, :-1] = inner
        if m.last_tau:
            g_nabla[:, -1] = tau[:, -1:] * _t32(gn)
        if accumulate and not m.no_g_n_in:
            g_nabla = g_nabla + _t32(gi["g_n_in"])
        o["g_nabla"] = g_nabla.numpy()
    return o


def run_all(m, kernel_contract=False):
    reps = []
    for c, gi, refs in G.references():
        for v in G.variants_of(c):
            with np.errstate(all="ignore"):
                reps.append(G.check(c, gi, v, statement32(c, gi, v, m), refs[v], kernel_contract))
    return reps


def test_case_matrix_is_the_compositors_with_the_clamp_min_branch_pinned():
    refs = G.references()
    assert len(refs) == 25 and {c["P"] for c, _, _ in refs} == set(CR.P_LIST) and all(c["n_rays"] == 24 for c, _, _ in refs)
    assert {float(c["beta"]) for c, _, _ in refs} == {float(np.float32(b)) for b in CR.BETAS} and {int(c["white"]) for c, _, _ in refs} == {0, 1}
    assert sum(bool(c.get("depth_exempt")) for c, _, _ in refs) == 1
    for c, gi, _ in refs:
        n = np.linalg.norm(gi["nabla"].astype(np.float64), axis=-1)
        assert n[0, min(1, c["P"] - 2)] == 0 and 0 < n[1, 0] < 1e-13, "the zero nabla and the one below the floor"
        assert gi["nabla"].dtype == gi["g_depth"].dtype == gi["g_normals"].dtype == np.float32
        again = G.geo_inputs(c)
        assert all(np.array_equal(gi[k], again[k]) for k in gi), "the extra inputs are a function of the case alone"


def test_caps_hold_for_every_case():
    """At most 1 % of a case's rays have unknown depth (then their depth-driven part is not compared); the depth_exempt case - 12 of 24 - runs
    without a depth cotangent; at most 1 % non-strict gradient elements.  From the reference alone."""
    exempt = 0
    for c, gi, refs in G.references():
        for v, ref in refs.items():
            rep = CR.Report(f"{c['name']} [{v}]")
            G.check_caps(c, ref, rep)
            assert not rep.fail, rep.fail
            gd, gn, _ = G.variant_cotangents(c, gi, v)
            assert gd is not None or gn is not None
            if c.get("depth_exempt"):
                exempt += 1
                assert gd is None and int(ref["unknown"].sum()) == 12
            else:
                assert int(ref["unknown"].sum()) == 0 and not ref["skip_rays"].any()
    assert exempt == 2


def test_fp32_statement_of_the_formulas_passes_every_case():
    reps = run_all(Mut())
    for r in reps:
        print(r.line())
    assert not [r for r in reps if r.fail], [r.line() for r in reps if r.fail]
    worst = {}
    for r in reps:
        for k, v in r.ratio.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("  WORST fp32 statement: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))


MUTANTS = sorted(k for k in vars(Mut) if not k.startswith("_"))

# the case and variant each mutant must be rejected by, named so that a failure says which went blind
EXPECT = {
    "depth_sign": "volsdf P=129 beta=0.1 white=1 [depth]",
    "ignore_accumulate": "volsdf P=130 beta=0.013 white=1 [both_acc]",
    "last_tau": "volsdf P=66 beta=0.1 white=0 [normals]",
    "no_depth_centre": "volsdf P=129 beta=0.1 white=1 [depth]",
    "no_g_n_in": "volsdf P=130 beta=0.013 white=1 [both_acc]",
    "no_projection": "volsdf P=130 beta=0.013 white=1 [normals]",
    "suffix_inclusive": "volsdf P=129 beta=0.1 white=1 [both]",
}


@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_is_rejected(name):
    reps = run_all(Mut(**{name: True}))
    failed = {r.name: r for r in reps if r.fail}
    first = next(iter(failed.values()), None)
    print(f"  mutant {name}: rejected by {len(failed)} of {len(reps)} runs" + (f", e.g. {first.name}: {first.fail[0][:160]}" if first else ""))
    assert failed, f"mutant {name} passed every case"
    assert EXPECT[name] in failed, f"mutant {name} is no longer rejected by '{EXPECT[name]}' (still by {len(failed)} others)"


def test_geo_entry_points_validate_their_arguments_without_a_gpu():
    """nerfart_volsdf_composite_geo_bwd and nerfart_volsdf_render_bwd2: 2 and a message before any HIP call - null or never dereferenced pointers."""
    from nerfart_amd import hip
    lib, null, one = hip.lib, None, C.c_void_p(16)

    def err():
        return lib.nerfart_last_error().decode()

    def geo(n_rays, P, nabla=one, g_depth=one, g_normals=one, g_nabla=one, d=one):
        return lib.nerfart_volsdf_composite_geo_bwd(n_rays, P, d, one, nabla, 100.0, 0.01, g_depth, g_normals, null, 0, one, g_nabla, null, null)
    for P in (1, 0, 514, 1025):
        assert geo(1, P) == 2 and "2 <= P <= 513" in err(), (P, err())
    assert geo(0, 0) == 0 and geo(-1, 192) == 0                                   # an empty launch stays a no-op
    assert geo(4, 192, g_depth=null, g_normals=null) == 2 and "both are NULL" in err()
    assert geo(4, 192, nabla=null) == 2 and "needs nabla and g_nabla" in err()
    assert geo(4, 192, g_nabla=null) == 2 and "needs nabla and g_nabla" in err()
    assert geo(4, 192, d=null) == 2 and "null argument" in err()

    def bwd2(n_rays, P, ws=null, ws_bytes=0, ptr=one, g_depth=one, g_normals=one):
        return lib.nerfart_volsdf_render_bwd2(ptr, ptr, 1, 6, ptr, ptr, n_rays, P, ptr, ptr, null, null, g_depth, g_normals, null, null, null, 3.0, 100.0,
                                              0.01, 0, 0.1, 0, 1, ptr, ws, ws_bytes, null)
    for P in (1, 514):
        assert bwd2(4, P) == 2 and "2 <= P <= 513" in err(), (P, err())
    assert bwd2(20000, 192) == 2 and "2^21" in err()
    assert bwd2(4, 192, ptr=null) == 2 and "null" in err()
    assert bwd2(0, 192) == 0
    need = lib.nerfart_volsdf_render_bwd2_workspace_bytes(4, 192, 0, 1)
    plain = lib.nerfart_volsdf_render_bwd_workspace_bytes(4, 192, 0)
    assert lib.nerfart_volsdf_render_bwd2_workspace_bytes(4, 192, 0, 0) == plain, "no normals cotangent: today's workspace"
    assert need == plain + (4 * 192 * 3 * 4 + 255) // 256 * 256, "one [R P, 3] buffer more"
    assert bwd2(4, 192) == 2 and "bwd2_workspace_bytes" in err()
    assert bwd2(4, 192, ws=one, ws_bytes=need - 1) == 2 and "bwd2_workspace_bytes" in err()
    assert bwd2(4, 192, ws=one, ws_bytes=plain, g_depth=null) == 2 and "bwd2_workspace_bytes" in err()     # sized for the entry point without normals
