"""CPU self-tests of tests/composite_ref.py: on every case of the GPU matrix of tests/test_gpu_composite.py the comparator accepts an independent fp32
implementation (oracle/render.py in float32 with float32 autograd - another summation order, another exp), it accepts the fp32 stand-in of the
kernels' data flow (lane segments, shuffle scans, second pass), and it rejects that stand-in with each of the bugs these kernels invite.  The two
1 % caps (non-strict gradient elements, rays of unknown depth) hold for every case, from the reference alone.  The stand-ins and their mutants
live here, never in product code."""
import numpy as np
import pytest
import torch

import composite_ref as CR
from composite_ref import F
from oracle import render as orender
from oracle import sampling


def _t32(x):
    return torch.as_tensor(np.array(x, np.float32))


# ---- the independent fp32 implementation: the torch oracle in float32 -------------------------------------------------------------------------
def run_oracle32(c):
    white, P = bool(c["white"]), c["P"]
    g, gacc = _t32(c["g_rgb"]), None if c["g_acc"] is None else _t32(c["g_acc"])
    nab = None if c["nabla"] is None else _t32(c["nabla"])
    o = {}
    if c["fw"] == "volsdf":
        s, rad = _t32(c["sdf"]).requires_grad_(True), _t32(c["rad"]).requires_grad_(True)
        al, be = _t32(c["alpha"]).requires_grad_(True), _t32(c["beta"]).requires_grad_(True)
        sigma = sampling.sdf_to_sigma(s, al, be)
        r = orender.volsdf_composite(_t32(c["d"]), sigma, rad, nab, white)
        o.update(rgb=r["rgb"], depth=r["depth_volume"], acc=r["mask_volume"], normals=r.get("normals_volume"), sigma=sigma, p=r["p_i"],
                 tau=r["visibility_weights"])
        acc, leaves, key = r["mask_volume"], (al, be), "g_ab"
    else:
        s, rad, sv = _t32(c["sdf"]).requires_grad_(True), _t32(c["rad"]).requires_grad_(True), _t32(c["s"]).requires_grad_(True)
        d = _t32(c["d"])
        cdf, a = orender.sdf_to_alpha(s, sv)
        w = orender.alpha_to_w(a)
        dmid = 0.5 * (d[..., 1:] + d[..., :-1])
        acc = w.sum(-1)
        rgb = (w[..., None] * rad).sum(-2)
        if white:
            rgb = rgb + (1.0 - acc[..., None])
        o.update(rgb=rgb, depth=(w / (acc[..., None] + 1e-10) * dmid).sum(-1), acc=acc, cdf=cdf, alpha=a, w=w, d_mid=dmid)
        if nab is not None:
            o["normals"] = (torch.nn.functional.normalize(nab, dim=-1)[..., :P - 1, :] * w[..., None]).sum(-2)
        leaves, key = (sv,), "g_s"
    if P <= 513:
        ((o["rgb"] * g).sum() + (0 if gacc is None else (acc * gacc).sum())).backward()
        o["g_sdf"], o["g_rad"] = s.grad, rad.grad
        o[key] = _t32(c["preload"]) + torch.stack([x.grad.reshape(()) for x in leaves])
    o = {k: (None if v is None else v.detach().numpy()) for k, v in o.items()}
    return _select(c, o)


def _select(c, o):
    """Only what the case asks for, as the entry points with NULL for the rest."""
    for k, want in c["want"].items():
        if not want:
            o[k] = None
    if c["nabla"] is None:
        o["normals"] = None
    return o


# ---- the fp32 stand-in of the kernels' data flow, with switchable injected bugs ------------------------------------------------------------------
class Mut:
    tau_no_eps = False          # VolSDF: tau = (1 - p) T, the + 1e-10 lost
    f_no_eps = False            # NeuS: the factor 1 - alpha without its + 1e-10
    no_carry = False            # transmittance not carried across a lane-segment boundary
    drop_seg_interval = False   # the interval at k = seg * lane (lane 1) dropped
    depth_next = False          # VolSDF: depth weighted with d[k + 1]
    depth_dk = False            # NeuS: depth weighted with d[k] instead of the mid-point
    no_white_fwd = False        # white background: + (1 - acc) omitted
    no_white_bwd = False        # white background: - sum g_rgb omitted in the backward
    no_gacc = False             # g_acc ignored
    suffix_inclusive = False    # the suffix sum S includes the interval's own term
    last_nonzero = False        # VolSDF: the last sample's g_sdf / g_rad are not zero
    no_lane_carry = False       # NeuS: gc[cnt] not passed to the next lane's first sample
    drop_last = False           # NeuS: sample P - 1's g_sdf dropped
    rad_stride_P = False        # NeuS backward: rad_mid read with row stride P
    psi_neg_ignored = False     # d / d alpha: psi = e on the s < 0 branch too
    beta_sign = False           # d / d beta with the wrong sign
    no_normalize = False        # normals: nabla not normalised
    no_norm_floor = False       # normals: F.normalize's 1e-12 floor missing
    no_gate = False             # the relu / clamp gate ignored in the backward

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Mut, k), k
            setattr(self, k, v)


def _normals32(m, nab, wgt):
    v = nab[:, :-1]
    nr = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]).astype(F))
    if not m.no_norm_floor:
        nr = np.maximum(nr, F(1e-12))
    n = v if m.no_normalize else (v / nr[..., None]).astype(F)
    return np.stack([CR.lane_sum((n[..., j] * wgt).astype(F)) for j in range(3)], -1)


def _gbg(m, c, g):
    gbg = np.zeros(g.shape[0], F)
    if c["white"] and not m.no_white_bwd:
        gbg = -(g[:, 0] + g[:, 1] + g[:, 2])
    if c["g_acc"] is not None and not m.no_gacc:
        gbg = (gbg + c["g_acc"]).astype(F)
    return gbg


def _ray_total(pre, per_ray):
    tot = F(pre)
    for v in per_ray:
        tot = F(tot + v)
    return tot


def standin_volsdf(c, m):
    d, s, rad = c["d"], c["sdf"], c["rad"]
    R, P = d.shape
    nint, seg = P - 1, (P - 1 + 63) >> 6
    al, be = F(c["alpha"]), F(c["beta"])
    e = (F(0.5) * np.exp(-np.abs(s) / be)).astype(F)
    psi = np.where(s >= 0, e, F(1) - e).astype(F)
    sig = (al * psi).astype(F)
    delta = (d[:, 1:] - d[:, :-1]).astype(F)
    sd = (sig[:, :-1] * delta).astype(F)
    p = np.exp(-np.maximum(sd, F(0))).astype(F)
    q = (F(1) - p) if m.tau_no_eps else ((F(1) - p) + F(1e-10)).astype(F)
    live = np.ones(nint, bool)
    if m.drop_seg_interval and nint > seg:
        live[seg] = False
        p = np.where(live, p, F(1)).astype(F)
    T = CR.scan_T(p, carry=not m.no_carry)
    tau = np.where(live, q * T, F(0)).astype(F)
    acc = CR.lane_sum(tau)
    rgb = np.stack([CR.lane_sum((tau * rad[:, :-1, j]).astype(F)) for j in range(3)], -1)
    if c["white"] and not m.no_white_fwd:
        rgb = (rgb + (F(1) - acc)[:, None]).astype(F)
    inv = (acc + F(1e-10)).astype(F)
    dk = d[:, 1:] if m.depth_next else d[:, :-1]
    o = dict(rgb=rgb, acc=acc, depth=CR.lane_sum((tau / inv[:, None] * dk).astype(F)), sigma=sig, p=p, tau=tau,
             normals=None if c["nabla"] is None else _normals32(m, c["nabla"], tau))
    if P <= 513:
        g = c["g_rgb"]
        gtau = (g[:, None, 0] * rad[:, :-1, 0] + g[:, None, 1] * rad[:, :-1, 1] + g[:, None, 2] * rad[:, :-1, 2] + _gbg(m, c, g)[:, None]).astype(F)
        S = CR.suffix_S((tau * gtau).astype(F), inclusive=m.suffix_inclusive)
        gx = (p * T * gtau - S).astype(F)
        gsig = np.where((sd > 0) | m.no_gate, gx * delta, F(0)).astype(F)
        g_sdf = np.zeros((R, P), F)
        g_sdf[:, :-1] = gsig * al * (-e[:, :-1] / be)
        g_rad = np.zeros((R, P, 3), F)
        g_rad[:, :-1] = tau[..., None] * g[:, None, :]
        if m.last_nonzero:
            g_sdf[:, -1], g_rad[:, -1] = g_sdf[:, -2], g_rad[:, -2]
        ps = e[:, :-1] if m.psi_neg_ignored else psi[:, :-1]
        ga = CR.lane_sum((gsig * ps).astype(F))
        gb = CR.lane_sum((gsig * al * (e[:, :-1] * s[:, :-1] / (be * be))).astype(F))
        if m.beta_sign:
            gb = -gb
        o.update(g_sdf=g_sdf, g_rad=g_rad, g_ab=np.array([_ray_total(c["preload"][0], ga), _ray_total(c["preload"][1], gb)], F))
    return _select(c, o)


def standin_neus(c, m):
    d, sdf, rad = c["d"], c["sdf"], c["rad"]
    R, P = sdf.shape
    nint, seg = P - 1, (P - 1 + 63) >> 6
    s = F(c["s"])
    cdf = (F(1) / (F(1) + np.exp(-(sdf * s).astype(F)))).astype(F)
    c0, c1 = cdf[:, :-1], cdf[:, 1:]
    a = np.maximum((c0 - c1) / (c0 + F(1e-10)), F(0)).astype(F)
    f = (F(1) - a) if m.f_no_eps else ((F(1) - a) + F(1e-10)).astype(F)
    live = np.ones(nint, bool)
    if m.drop_seg_interval and nint > seg:
        live[seg] = False
        f = np.where(live, f, F(1)).astype(F)
    T = CR.scan_T(f, carry=not m.no_carry)
    w = np.where(live, a * T, F(0)).astype(F)
    acc = CR.lane_sum(w)
    rgb = np.stack([CR.lane_sum((w * rad[..., j]).astype(F)) for j in range(3)], -1)
    if c["white"] and not m.no_white_fwd:
        rgb = (rgb + (F(1) - acc)[:, None]).astype(F)
    inv = (acc + F(1e-10)).astype(F)
    dmid = (F(0.5) * (d[:, 1:] + d[:, :-1])).astype(F)
    o = dict(rgb=rgb, acc=acc, depth=CR.lane_sum((w / inv[:, None] * (d[:, :-1] if m.depth_dk else dmid)).astype(F)), cdf=cdf, alpha=a, w=w, d_mid=dmid,
             normals=None if c["nabla"] is None else _normals32(m, c["nabla"], w))
    if P <= 513:
        g = c["g_rgb"]
        rb = rad
        if m.rad_stride_P:
            flat = np.concatenate([rad.reshape(-1, 3), np.zeros((R, 3), F)])
            rb = flat[(np.arange(R)[:, None] * P + np.arange(nint)[None, :])]
        gw = (g[:, None, 0] * rb[..., 0] + g[:, None, 1] * rb[..., 1] + g[:, None, 2] * rb[..., 2] + _gbg(m, c, g)[:, None]).astype(F)
        S = CR.suffix_S((gw * w).astype(F), inclusive=m.suffix_inclusive)
        with np.errstate(all="ignore"):
            ga = (T * gw - S / f).astype(F)
        gate = (a > 0) | m.no_gate
        inv0 = (F(1) / (c0 + F(1e-10))).astype(F)
        gB = np.where(gate, ga * (c1 + F(1e-10)) * inv0 * inv0, F(0)).astype(F)
        gD = np.where(gate, -ga * inv0, F(0)).astype(F)
        if m.no_lane_carry:
            k = np.arange(nint)
            gD = np.where(((k + 1) % seg == 0) & (k + 1 < nint), F(0), gD).astype(F)
        if m.drop_last:
            gD[:, -1] = 0
        gc = np.concatenate([gB, np.zeros((R, 1), F)], -1) + np.concatenate([np.zeros((R, 1), F), gD], -1)
        t = (gc * cdf * (F(1) - cdf)).astype(F)
        g_rad = ((a * T)[..., None] * g[:, None, :]).astype(F)
        gs = CR.lane_sum((t * sdf).astype(F)[:, :-1]) + (t * sdf)[:, -1]
        o.update(g_sdf=(t * s).astype(F), g_rad=g_rad, g_s=np.array([_ray_total(c["preload"][0], gs.astype(F))], F))
    return _select(c, o)


_CASES = None


def cases():
    """(case, reference) pairs: the references are the slow part and depend on the inputs alone."""
    global _CASES
    if _CASES is None:
        _CASES = [(c, CR.volsdf_reference(c) if c["fw"] == "volsdf" else CR.neus_reference(c)) for c in CR.volsdf_cases() + CR.neus_cases()]
    return _CASES


def run_all(run_v, run_n, kernel_contract=True):
    reps = []
    for c, ref in cases():
        with np.errstate(all="ignore"):
            reps.append(CR.check(c, (run_v if c["fw"] == "volsdf" else run_n)(c), ref, kernel_contract))
    return reps


def _assert_clean(reps):
    for r in reps:
        print(r.line())
    assert not [r for r in reps if r.fail], [r.line() for r in reps if r.fail]


def test_caps_hold_for_every_case():
    """At most 1 % non-strict gradient elements and at most 1 % rays of unknown depth per case, from the reference alone; the all-empty case is
    exempt from the depth cap and must in fact contain unknown depths (it is there to show them)."""
    exempt = 0
    for c, ref in cases():
        rep = CR.Report(c["name"])
        CR.check_caps(c, ref, rep)
        print(rep.line())
        assert not rep.fail, rep.fail
        if c.get("depth_exempt"):
            exempt += 1
            assert rep.unknown >= c["n_rays"] // 2 - 1
    assert exempt == 1
    assert any(ref.get("nonstrict", 0) > 0 for _, ref in cases()), "no case exercises an in-band gate"


def test_case_matrix_covers_what_it_claims():
    """The regimes the matrix exists for, pinned: an edit of the generators that curates one away fails here."""
    cs = [c for c, _ in cases()]
    for fw in ("volsdf", "neus"):
        mine = [c for c in cs if c["fw"] == fw]
        assert {c["P"] for c in mine} == set(CR.P_LIST + CR.P_FWD_ONLY)
        assert {int(c["white"]) for c in mine} == {0, 1} and {c["g_acc"] is None for c in mine} == {True, False}
        assert {c["nabla"] is None for c in mine} == {True, False}
        detail = [k for k in mine[0]["want"] if not k.startswith("g_")]
        for k in mine[0]["want"]:
            assert {bool(c["want"][k]) for c in mine} == {True, False}, k          # every optional output NULL and non-NULL
        assert any(not any(c["want"][k] for k in detail) for c in mine), "no case with every detail output NULL (the render path's call)"
        assert any(all(c["want"][k] for k in detail) for c in mine), "no case with every detail output set"
        assert {bool(np.any(c["preload"])) for c in mine} == {True, False}, "accumulators preloaded and zero"
        assert max(c["n_rays"] for c in mine) <= 256
        for c in mine:
            if c["nabla"] is not None:
                n = np.linalg.norm(c["nabla"].astype(np.float64), axis=-1)
                assert n[0, min(1, c["P"] - 2)] == 0 and abs(n[1, 0] / 1e-20 - 1) < 1e-6, "the zero nabla and the one of norm 1e-20"
    v = [(c, r) for c, r in cases() if c["fw"] == "volsdf"]
    assert {float(c["beta"]) for c, _ in v} == {float(np.float32(b)) for b in CR.BETAS}
    assert all(float(c["alpha"]) == float(np.float32(1) / c["beta"]) for c, _ in v)
    big = [c for c, _ in v if c["P"] >= 64]
    assert all((np.diff(c["d"], axis=-1) == 0).any() for c in big), "exact duplicate depths"
    assert all((np.diff(c["d"], axis=-1) < 0).sum() == 1 for c in big), "one inverted pair"
    p_zero = 0
    for c, ref in v:
        sig, p = ref["sigma"][0], ref["p"][0]
        assert ((sig[:, :-1] == 0).all(-1)).sum() >= 3, (c["name"], "all-empty rays: sigma underflows to exactly 0")
        if c["depth_exempt"]:
            continue
        assert (c["sdf"][:, 0] < 0).any(), (c["name"], "a ray that starts inside")
        if c["P"] >= 64 and float(c["beta"]) < 0.0021:
            assert (np.cumprod(p, -1)[:, -1] == 0).sum() >= 10, (c["name"], "an opaque tail: T reaches 0")
            p_zero += bool((p == 0).any())
    assert p_zero >= 8, "p underflows to exactly 0 in too few cases"
    assert sum(ref.get("nonstrict", 0) > 0 for _, ref in v) >= 4, "VolSDF in-band gates (the one denormal exp per case)"
    n = [(c, r) for c, r in cases() if c["fw"] == "neus"]
    assert {float(c["s"]) for c, _ in n} == set(CR.S_LIST)
    for c, ref in n:
        cdf, s = ref["cdf"][0], float(c["s"])
        assert (cdf == 1).all(-1).sum() >= 4, (c["name"], "rays entirely outside: cdf == 1 throughout")
        assert (c["sdf"] < 0).all(-1).sum() >= 4, (c["name"], "rays entirely inside")
        if s >= 2048:
            assert ref["alpha"][0].max() >= 1 - 1e-9, (c["name"], "an interval with alpha -> 1")
        if c["P"] >= 64 and s >= 64:
            assert (cdf[:, :-1] == cdf[:, 1:]).mean() >= (0.7 if s >= 512 else 0.25), (c["name"], "c0 == c1 exactly: saturated intervals")
    assert sum(ref.get("nonstrict", 0) > 0 for _, ref in n) >= 3, "NeuS in-band gates (ray 0 of the longer rows at s = 64)"


def test_fp32_oracle_passes_every_case():
    _assert_clean(run_all(run_oracle32, run_oracle32, kernel_contract=False))


def test_fp32_standin_of_the_kernels_data_flow_passes_every_case():
    _assert_clean(run_all(lambda c: standin_volsdf(c, Mut()), lambda c: standin_neus(c, Mut())))


MUTANTS = sorted(k for k in vars(Mut) if not k.startswith("_"))


# The case each mutant must be rejected by (one per framework whose kernels can have the bug): named here so that a failure says which case went
# blind, not only that some case still rejects.
EXPECT = {
    "beta_sign": ["volsdf P=129 beta=0.002 white=0"],
    "depth_dk": ["neus P=130 s=512 white=1"],
    "depth_next": ["volsdf P=130 beta=0.0005 white=0"],
    "drop_last": ["neus P=128 s=20 white=1"],
    "drop_seg_interval": ["volsdf P=130 beta=0.013 white=1", "neus P=130 s=20 white=0"],
    "f_no_eps": ["neus P=128 s=2048 white=0"],
    "last_nonzero": ["volsdf P=129 beta=0.002 white=0"],
    "no_carry": ["volsdf P=130 beta=0.013 white=1", "neus P=130 s=20 white=0"],
    "no_gacc": ["volsdf P=128 beta=0.013 white=0", "neus P=129 s=64 white=1"],
    "no_gate": ["volsdf P=192 beta=0.1 white=0", "neus P=129 s=4096 white=0"],
    "no_lane_carry": ["neus P=129 s=4096 white=0"],
    "no_norm_floor": ["volsdf P=130 beta=0.013 white=1", "neus P=130 s=512 white=1"],
    "no_normalize": ["volsdf P=130 beta=0.013 white=1", "neus P=130 s=512 white=1"],
    "no_white_bwd": ["volsdf P=129 beta=0.1 white=1", "neus P=129 s=64 white=1"],
    "no_white_fwd": ["volsdf P=130 beta=0.013 white=1", "neus P=130 s=512 white=1"],
    "psi_neg_ignored": ["volsdf P=130 beta=0.013 white=1"],
    "rad_stride_P": ["neus P=129 s=64 white=1"],
    "suffix_inclusive": ["volsdf P=129 beta=0.002 white=0", "neus P=129 s=64 white=1"],
    "tau_no_eps": ["volsdf P=130 beta=0.0005 white=0"],
}


@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_is_rejected(name):
    m = Mut(**{name: True})
    reps = run_all(lambda c: standin_volsdf(c, m), lambda c: standin_neus(c, m))
    failed = {r.name: r for r in reps if r.fail}
    first = next(iter(failed.values()), None)
    print(f"  mutant {name}: rejected by {len(failed)} of {len(reps)} cases" + (f", e.g. {first.name}: {first.fail[0][:160]}" if first else ""))
    assert failed, f"mutant {name} passed every case"
    assert EXPECT[name], name
    for case in EXPECT[name]:
        assert case in failed, f"mutant {name} is no longer rejected by case '{case}' (still rejected by {len(failed)} others, e.g. '{first.name}')"
