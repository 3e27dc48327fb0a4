"""fp64 reference, first-order error model and comparator of k_composite_volsdf_geo_bwd (csrc/volsdf_geo_backward.hip): the backward of the VolSDF
compositor w.r.t. its depth and normals maps.

REFERENCE.  float64 torch.autograd through oracle.render.volsdf_composite(d, oracle.sampling.sdf_to_sigma(sdf, alpha, beta), rad, nabla, white) with
the loss  sum g_depth depth_volume + sum g_normals normals_volume, on the fp32 INPUT VALUES; sdf, nabla, alpha and beta are the leaves.  Nothing is
taken from nerfart_amd/autodiff.py.  The inputs are composite_ref.volsdf_cases() with P <= 513 (imported, not edited) plus, per case, g_depth [R],
g_normals [R, 3], g_n_in [R, P, 3], a g_sdf preload [R, P] and - where the case has no nablas - nablas from composite_ref._nablas (one zero vector and
one of norm 1e-20 per case: the clamp_min branch of F.normalize), all drawn from a generator seeded by the case's name alone and stored as fp32.  They
never consult the reference.

ERROR MODEL (first order in u = 2^-24, every tolerance SAFETY times the bound plus TINY, as composite_ref.py).
  The forward:  tau_k = (1 - p_k + 1e-10) T_k,  acc = sum tau,  inv = acc + 1e-10,  depth = sum tau_k d_k / inv,  normals = sum tau_k n_k,
  n_k = nabla_k / max(|nabla_k|, 1e-12).  The cotangent of the weights from the two maps is
        g_tau_k = g_normals . n_k + (g_depth / inv) (d_k - depth)
  and the rest is k_composite_volsdf_bwd's chain, which is LINEAR in g_tau.  So g_sdf, d / d alpha and d / d beta of the two cotangents are what
  composite_ref.volsdf_reference computes for a PSEUDO CASE c': c with  rad'[..., 0] = n_k . g_normals + g_depth d_k / inv  (other channels 0),
  g_rgb' = (1, 0, 0), g_acc' = -g_depth depth / inv, white = False: its g_tau' = rad'_0 + g_acc' is the g_tau above.  pseudo_case() builds c' in float64
  and geo_reference() asserts that c''s autograd g_sdf equals the autograd g_sdf of the two-map loss (a self-check of this linearity on every case).
  The pseudo case's tol, hull and gate handling are taken exactly as composite_ref.check takes them: they model every rounding of the chain from g_tau
  on (4 u of |rad'_0| + |g_acc'| for forming g_tau itself - which covers the cancellation in d_k - depth - then tau, the suffix sum, p T, the gate,
  sigma's derivative).
  What c' cannot know is that the kernel forms g_tau from ITS OWN fp32 n_k, depth and inv.  That adds, per interval,
        delta_k = 10 u sum_j |g_normals_j n_kj|                          n_k carries 7 u (composite_ref._normals), each product 1 u, the 3-term sum 2 u
                + |g_depth| / inv (d(depth) + |d_k - depth| (d(inv) / inv + 4 u))   depth and inv carry the bounds volsdf_reference(c) returns for them;
                                                                          the quotient g_depth / inv, the difference, the product, the final add: 1 u each
                + u |g_tau_k|
  and, the chain being linear, an error  fac_k |delta_k| (p_k T_k delta_k + sum_{i>k} tau_i delta_i)  of g_sdf_k (fac = alpha e / beta; |delta_k| the
  interval's length), gated like the pseudo case's own tol; psi_k resp. alpha e |s| / beta^2 in place of fac for d / d alpha, d / d beta.
  On a ray of UNKNOWN depth (composite_ref._depth: the denominator is not pinned down) d(depth) is infinite: with a depth cotangent the ray's g_sdf is
  not compared.  At most 1 % of a case's rays may be such (none is, in the 24 non-exempt cases); the one depth_exempt case (all-empty rays, 12 of 24
  unknown) runs with g_depth = None, normals only.
  g_nabla_k = tau_k (g_normals - n_k (n_k . g_normals)) / |nabla_k|  (|nabla_k| >= 1e-12),  tau_k g_normals / 1e-12 below, 0 for the last sample:
        d(g_nabla_kj) = d(tau_k) |proj_kj| / m_k + 10 u tau_k (|g_normals_j| + |n_kj| sum_i |n_ki g_normals_i|) / m_k + u |g_nabla_kj + g_n_in_kj|
  with m_k = max(|nabla_k|, 1e-12): the weight's own error, 10 u of the TERMS of the projected vector (|nabla| 2.5 u, n 3.5 u, the dot product 6.5 u, the
  products, tau / |nabla| 3.5 u: 5.5 u on the first term and 16 u on the second, inside SAFETY x 10 u; the terms, not their difference - g_normals nearly
  parallel to n cancels), and the addition of g_n_in.  composite_ref._normals' domain holds: |nabla| = 0, < 1e-13 or > 1e-11.
ACCUMULATION.  accumulate: g_sdf = preload + gradient, one more rounding u (|preload| + |gradient|); the last sample keeps the preload (else it is +0).
g_alpha_beta = composite_ref.PRELOAD + the sums, as composite_ref.check treats the sibling's.
"""
import zlib

import numpy as np
import torch

import composite_ref as CR
from composite_ref import U, SAFETY, TINY, DEN, X_GATE, EXP_ZERO
from oracle import render as orender
from oracle import sampling
from stage_ref import seg_of, bits

VARIANTS = ("depth", "normals", "both", "both_acc")


def cases():
    """composite_ref's VolSDF matrix, the rows the backward accepts."""
    return [c for c in CR.volsdf_cases() if c["P"] <= 513]


def geo_inputs(c):
    """The extra inputs of a case, from its name alone (fp32; the reference is never consulted)."""
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()) + 77)
    R, P = c["n_rays"], c["P"]
    nab = c["nabla"] if c["nabla"] is not None else CR._nablas(R, P, rng)
    return dict(nabla=np.ascontiguousarray(nab, np.float32), g_depth=rng.standard_normal(R).astype(np.float32),
                g_normals=rng.standard_normal((R, 3)).astype(np.float32), g_n_in=rng.standard_normal((R, P, 3)).astype(np.float32),
                g_sdf0=rng.standard_normal((R, P)).astype(np.float32))


def variant_cotangents(c, gi, variant):
    """(g_depth or None, g_normals or None, accumulate) of a variant; the depth_exempt case never gets a depth cotangent."""
    gd = gi["g_depth"] if variant != "normals" and not c.get("depth_exempt") else None
    gn = gi["g_normals"] if variant != "depth" else None
    return gd, gn, variant == "both_acc"


def variants_of(c):
    return ("normals", "both_acc") if c.get("depth_exempt") else VARIANTS


_t = CR._t


def base_reference(c, gi):
    """composite_ref.volsdf_reference of the case with the nablas the geometry backward uses: tau, acc, depth with their bounds, `unknown`."""
    return CR.volsdf_reference(dict(c, nabla=gi["nabla"]))


def _nhat(nab):
    v = nab[:, :-1]
    nrm = np.sqrt((v * v).sum(-1, keepdims=True))
    if not np.all((nrm == 0) | (nrm < 1e-13) | ((nrm > 1e-11) & (np.abs(v).max(-1, keepdims=True) < 1e18))):
        raise ValueError("nabla outside the modelled domain of F.normalize")
    return v / np.maximum(nrm, 1e-12), nrm[..., 0]


def pseudo_case(c, gi, base, gd, gn):
    """The case whose rgb backward IS the depth / normals backward (module docstring); float64 values."""
    d = np.asarray(c["d"], np.float64)
    R, P = d.shape
    n, _ = _nhat(np.asarray(gi["nabla"], np.float64))
    acc, depth = base["acc"][0], base["depth"][0]
    inv = acc + 1e-10
    rad = np.zeros((R, P, 3))
    if gn is not None:
        rad[:, :-1, 0] += (n * np.asarray(gn, np.float64)[:, None, :]).sum(-1)
    gacc = None
    if gd is not None:
        gd64 = np.asarray(gd, np.float64)
        rad[:, :, 0] += (gd64 / inv)[:, None] * d
        gacc = -gd64 * depth / inv
    g = np.zeros((R, 3))
    g[:, 0] = 1.0
    return dict(c, rad=rad, g_rgb=g, g_acc=gacc, white=0, nabla=None, name=c["name"] + " (pseudo)")


def geo_reference(c, gi, base, gd, gn):
    """-> dict: g_sdf (ref, tol) + hull, g_alpha / g_beta (ref, bound), g_nabla (ref, bound) or None, skip_rays [R], nonstrict, elements."""
    d, s, nab = (np.asarray(x, np.float64) for x in (c["d"], c["sdf"], gi["nabla"]))
    R, P = d.shape
    al, be = float(c["alpha"]), float(c["beta"])
    cost = 2 * seg_of(P) + 8
    # ---- float64 autograd through the oracle
    ts, tn, ta, tb = _t(s).requires_grad_(True), _t(nab).requires_grad_(True), _t(al).requires_grad_(True), _t(be).requires_grad_(True)
    o = orender.volsdf_composite(_t(d), sampling.sdf_to_sigma(ts, ta, tb), _t(np.asarray(c["rad"], np.float64)), tn, bool(c["white"]))
    loss = 0
    if gd is not None:
        loss = loss + (o["depth_volume"] * _t(gd)).sum()
    if gn is not None:
        loss = loss + (o["normals_volume"] * _t(gn)).sum()
    loss.backward()
    ref_gs, ref_ga, ref_gb = ts.grad.numpy(), float(ta.grad), float(tb.grad)
    ref_gnab = None if tn.grad is None else tn.grad.numpy()
    # ---- the pseudo case: tol, hull, gates of the chain from g_tau on
    pc = pseudo_case(c, gi, base, gd, gn)
    pr = CR.volsdf_reference(pc)
    scale = np.abs(ref_gs).max(-1, keepdims=True) + 1e-300
    # fp64 against fp64.  (Rows of one interval: d_0 - depth cancels to 1e-10 / inv of d_0, so the two fp64 evaluations agree to ~1e-6 of a gradient
    # that is itself ~1e-10 of the terms it is made of - far inside the fp32 tol, which counts those terms.)
    assert np.all(np.abs(pr["g_sdf"][0] - ref_gs) <= 1e-7 * scale + 1e-3 * pr["g_sdf"][1]), "the pseudo case's g_sdf left the two-map autograd's (linearity)"
    for k, r in (("g_alpha", ref_ga), ("g_beta", ref_gb)):          # fp64 against fp64: far inside the fp32 bound
        assert abs(pr[k][0] - r) <= 1e-3 * pr[k][1] + 1e-9 * abs(r), f"the pseudo case's {k} left the two-map autograd's"
    # ---- delta_k: the kernel's own fp32 evaluation of g_tau
    n, nrm = _nhat(nab)
    tau, dtau = base["tau"]
    acc, dacc = base["acc"]
    depth, ddepth = base["depth"]
    unknown = base["unknown"]
    inv = acc + 1e-10
    dinv = dacc + U * inv
    gtau = pc["rad"][:, :-1, 0] + (0.0 if pc["g_acc"] is None else pc["g_acc"][:, None])
    dlt = U * np.abs(gtau)
    if gn is not None:
        dlt = dlt + 10 * U * (np.abs(n) * np.abs(np.asarray(gn, np.float64))[:, None, :]).sum(-1)
    skip = np.zeros(R, bool)
    if gd is not None:
        agd = np.abs(np.asarray(gd, np.float64))
        skip = unknown & (agd > 0)
        with np.errstate(invalid="ignore"):
            t = (agd / inv)[:, None] * (np.where(skip, 0.0, ddepth)[:, None] + np.abs(d[:, :-1] - depth[:, None]) * (dinv / inv + 4 * U)[:, None])
        dlt = dlt + t
    p = base["p"][0]
    T = np.concatenate([np.ones((R, 1)), np.cumprod(p, -1)[:, :-1]], -1)
    prop = p * T * dlt + CR._excl_suffix(tau * dlt) + cost * U * CR._excl_suffix(tau * dlt)
    delta = d[:, 1:] - d[:, :-1]
    xs = np.abs(s) / be
    e = 0.5 * np.exp(-xs)
    psi = np.where(s >= 0, e, 1 - e)
    sig_zero = (s >= 0) & (xs > EXP_ZERO)
    x = np.maximum(np.where(sig_zero, 0.0, al * psi)[:, :-1] * delta, 0.0)
    gated = ~(sig_zero[:, :-1] | (delta <= 0))                 # certain_on | inband of composite_ref: wherever the gate can be on
    gs_prop = np.where(gated, prop * np.abs(delta), 0.0)
    z1 = np.zeros((R, 1))
    extra = np.concatenate([gs_prop * (al * e[:, :-1] / be), z1], -1)
    out = dict(g_sdf=(ref_gs, pr["g_sdf"][1] + extra), g_sdf_hull=pr["g_sdf_hull"], skip_rays=skip, nonstrict=pr["nonstrict"], elements=pr["elements"],
               unknown=unknown)
    out["g_alpha"] = (np.float64(ref_ga), pr["g_alpha"][1] + (gs_prop * psi[:, :-1]).sum())
    out["g_beta"] = (np.float64(ref_gb), pr["g_beta"][1] + (gs_prop * al * e[:, :-1] * np.abs(s[:, :-1]) / (be * be)).sum())
    out["scalars_skip"] = bool(skip.any())
    # ---- g_nabla
    out["g_nabla"] = None
    if gn is not None:
        g64 = np.asarray(gn, np.float64)[:, None, :]
        m = np.maximum(nrm, 1e-12)[..., None]
        floor = (nrm < 1e-12)[..., None]
        dotn = (n * g64).sum(-1, keepdims=True)
        proj = np.where(floor, np.broadcast_to(g64, n.shape), g64 - n * dotn)
        terms = np.abs(g64) + np.where(floor, 0.0, np.abs(n) * (np.abs(n) * np.abs(g64)).sum(-1, keepdims=True))
        val = np.concatenate([tau[..., None] * proj / m, np.zeros((R, 1, 3))], 1)
        # tau is fp32's certain value where fp32's range ends (p == 0 exactly behind x > 104.5): its distance to the true weight joins the bound
        snap = np.abs(o["visibility_weights"].detach().numpy() - tau)
        bnd = np.concatenate([(dtau + snap)[..., None] * np.abs(proj) / m + 10 * U * tau[..., None] * terms / m, np.zeros((R, 1, 3))], 1)
        gap = np.concatenate([1.001 * snap[..., None] * np.abs(proj) / m, np.zeros((R, 1, 3))], 1)
        assert np.all(np.abs(val - ref_gnab) <= 1e-9 * np.abs(val).max(-1, keepdims=True) + gap + 1e-300), "analytic g_nabla left autograd's"
        out["g_nabla"] = (ref_gnab, bnd)
    return out


def check(c, gi, variant, o, ref, kernel_contract=True):
    """o: dict g_sdf [R,P], g_nabla [R,P,3] or None, g_ab [2] of one run of `variant` -> composite_ref.Report.  The accumulate variant preloads g_sdf with
    gi['g_sdf0'], passes gi['g_n_in'] and starts g_alpha_beta from composite_ref.PRELOAD; the others start g_alpha_beta from 0 and pass no g_n_in."""
    gd, gn, accumulate = variant_cotangents(c, gi, variant)
    rep = CR.Report(f"{c['name']} [{variant}]")
    R, P = c["n_rays"], c["P"]
    rep.rays, rep.unknown, rep.nonstrict, rep.elements = R, int(ref["unknown"].sum()), ref["nonstrict"], ref["elements"]
    v, tol = ref["g_sdf"]
    lo, hi = ref["g_sdf_hull"]
    pre = np.asarray(gi["g_sdf0"], np.float64) if accumulate else np.zeros((R, P))
    skip = np.broadcast_to(ref["skip_rays"][:, None], (R, P))
    rep.within("g_sdf", o["g_sdf"], v + pre, tol + U * (np.abs(pre) + np.maximum(np.abs(lo), np.abs(hi))) * (1 if accumulate else 0), lo + pre, hi + pre, skip=skip)
    if accumulate:
        rep.check(np.array_equal(bits(o["g_sdf"][:, -1]), bits(gi["g_sdf0"][:, -1])), "accumulate: the last sample's g_sdf is not the preload")
    elif kernel_contract:
        rep.check(np.all(bits(o["g_sdf"][:, -1]) == 0), "the last sample's g_sdf is not +0")
    rep.check((o.get("g_nabla") is not None) == (gn is not None), "g_nabla present / absent against the variant")
    if gn is not None and o.get("g_nabla") is not None:
        gv, gb = ref["g_nabla"]
        gin = np.asarray(gi["g_n_in"], np.float64) if accumulate else 0.0
        rep.within("g_nabla", o["g_nabla"], gv + gin, gb + U * np.abs(gv + gin))
    got = np.asarray(o["g_ab"], np.float64)
    preload = CR.PRELOAD if accumulate else np.zeros(2, np.float32)
    if not ref["scalars_skip"]:
        for i, k in enumerate(("g_alpha", "g_beta")):
            pv, (val, b) = float(preload[i]), ref[k]
            rep.within(k, got[i] - pv, val, b + (R + 1) * U * (abs(pv) + abs(val)))
    return rep


def check_caps(c, ref, rep):
    """At most 1 % of a case's rays of unknown depth (the exempt case runs without a depth cotangent) and at most 1 % non-strict gradient elements."""
    n_unknown = int(ref["unknown"].sum())
    if not c.get("depth_exempt"):
        rep.check(n_unknown <= CR.CAP * c["n_rays"], f"{n_unknown} of {c['n_rays']} rays have unknown depth (> {CR.CAP:.0%}): fix the inputs")
    rep.check(not ref["skip_rays"].any() or not c.get("depth_exempt"), "the depth_exempt case was given a depth cotangent")
    rep.check(ref["nonstrict"] <= CR.CAP * max(ref["elements"], 1), f"{ref['nonstrict']} of {ref['elements']} gradient elements are non-strict (> {CR.CAP:.0%})")


_REFS = None


def references():
    """[(case, inputs, {variant: reference})], computed once per process (the references are the slow part; 'both_acc' shares 'both''s)."""
    global _REFS
    if _REFS is None:
        _REFS = []
        for c in cases():
            gi = geo_inputs(c)
            base = base_reference(c, gi)
            refs = {}
            for v in variants_of(c):
                gd, gn, _ = variant_cotangents(c, gi, v)
                key = (gd is not None, gn is not None)
                same = next((refs[w] for w in refs if refs[w]["_key"] == key), None)
                if same is None:
                    same = geo_reference(c, gi, base, gd, gn)
                    same["_key"] = key
                refs[v] = same
            _REFS.append((c, gi, refs))
    return _REFS
