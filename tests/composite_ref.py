"""fp64 references of the compositing stage and its backward, with a first-order error model and a comparator.

The kernels are the one-wave-per-ray k_composite_volsdf (csrc/volsdf_render.hip), k_composite_neus (csrc/neus_render.hip) and
k_composite_volsdf_bwd / k_composite_neus_bwd (csrc/volsdf_backward.hip).  Every reference value is oracle/render.py (volsdf_composite,
sdf_to_alpha, alpha_to_w) and oracle.sampling.sdf_to_sigma run on float64 tensors of the kernels' fp32 INPUT VALUES; the backward is float64
torch.autograd through those same functions, with alpha, beta and s (the fp32 values the C ABI receives) as float64 leaves.  Nothing here is
built from nerfart_amd/autodiff.py.  tests/test_composite_ref.py shows on the CPU that the comparator accepts the float32 torch oracle and
rejects fp32 stand-ins of the kernels' data flow with injected bugs; tests/test_gpu_composite.py holds the HIP kernels to it.

ERROR MODEL (first order in u = 2^-24; every tolerance is SAFETY times the bound below plus TINY = 2^-126, the end of fp32's normal range).
A row of P samples has P - 1 intervals cut into 64 lane segments of seg = ceil((P - 1) / 64) (stage_ref.seg_of): a running sum or product is a
sequential segment, a 6-level shuffle scan and a second sequential pass, so a partial sum S of terms t carries cost u sum|t|, cost = 2 seg + 8.
The bounds are ABSOLUTE where the math is:
  VolSDF   psi_k = e or 1 - e, e = 0.5 exp(-|s_k| / beta):  relative (xs' + 3) u, xs' = |s_k| / beta (s >= 0) or |s_k| / beta e / (1 - e)  (the
           rounding of the exp argument, exp itself 2 u, the subtraction); sigma = alpha psi one more; x_k = relu(sigma_k delta_k) two more.
           p_k = exp(-x_k):  dp = p (dx + 2 u);   q_k = 1 - p_k + 1e-10:  dq = dp + 2 u q  - the rounding of p next to 1 is u, it does NOT
           shrink with x_k;   T_k = prod_{j<k} p_j:  relative sum_{j<k} (dx_j + 2 u) + cost u;   tau_k = q_k T_k:  dq T + q dT + u tau.
           acc / rgb / normals are sums of tau (times |c|, |n|; n = nabla / max(|nabla|, 1e-12) carries 6 u) plus cost u sum|terms|; the white
           background adds d(acc).  depth = sum tau_k / inv d_k with inv = acc + 1e-10:  (sum d_k dtau_k + depth d(inv)) / (inv - d(inv)) +
           (cost + 3) u depth - on a nearly empty ray d(inv) / inv is of order one and the ray's depth is UNKNOWN (below).
  NeuS     c_k = 1 / (1 + exp(-z)), z = s sdf_k:  dc = c (1 - c) (|z| + 2) u + 2 u c - absolute ~2 u next to 1, relative next to 0.
           alpha_k = max(raw, 0), raw = (c_k - c_k+1) / (c_k + 1e-10):  d(raw) = (dc_k + dc_k+1 + u |num| + |raw| (dc_k + u den)) / den + u |raw|,
           i.e. the absolute ~3 u of the cancellation over c_k + 1e-10.  f_k = 1 - alpha_k + 1e-10: d(alpha) + 2 u f.  T_k = prod f_j: the
           products of the factors' lower and upper ends (a factor next to 1e-10 may be off by a large RATIO; T stays tiny there), as
           stage_ref.neus_weights.  w_k = alpha_k T_k.  acc / rgb / normals / depth as above, depth weighted with d_mid = 0.5 (d_k + d_k+1)
           (one rounding; d_mid_out is held to 1 ulp).
  backward (the formulas of the header comment of csrc/volsdf_backward.hip, each product and sum counted):
           g_tau_k = g_rgb . c_k + g_bg:  4 u (sum |g_rgb c| + |g_bg terms|);  S_k = sum_{i>k} tau_i g_tau_i (EXCLUSIVE suffix):  sum of the
           terms' errors + cost u sum|terms|.   VolSDF:  g_x = p T g_tau - S,  g_sigma = [x > 0] delta g_x,  g_sdf = -g_sigma alpha e / beta.
           NeuS:  g_alpha_k = T_k (g_w_k - V_k) with V_k = S_k / (f_k T_k) = sum_{i>k} g_w_i alpha_i prod_{k<j<i} f_j - the kernel divides its
           S_k by ITS f_k, so f_k's large relative error cancels; V's error is propagated through V_k = g_w_k+1 alpha_k+1 + f_k+1 V_k+1.
           g_cdf_k = g_alpha_k (c_k+1 + 1e-10) / (c_k + 1e-10)^2 - g_alpha_k-1 / (c_k-1 + 1e-10)  (the first factor also as (1 - raw) / (c_k + 1e-10),
           autograd's way: + |g_alpha_k| d(raw) / (c_k + 1e-10)),  g_sdf_k = g_cdf_k c_k (1 - c_k) s; the bound
           on c (1 - c) is ABSOLUTE (dc), which covers fp32's exact 0 where 1 - c rounds to 0.
           g_alpha_beta / g_s are sums over all rays accumulated with float atomics in no fixed order: (R + cost) u sum|terms|.
fp32's RANGE is kept where it is certain (constants of stage_ref): exp(-x) == 0 for x > 104.5 (sigma, p), sigmoid == 1 for z > 17.5 and
== 0 for z < -88.8; the reference takes the fp32 value there (for the backward, the distance to the true fp64 value is added to the bound
instead).  x_k == 0 exactly (sigma == 0 or delta <= 0) gives p == 1 with no error.

GATES.  relu(sigma delta) and clamp(alpha, 0) are discontinuous in the gradient.  A gate whose argument lies inside its forward error band
(VolSDF: x below 2^-120 without being certainly 0 - a denormal exp; NeuS: |raw| <= SAFETY d(raw)) may go either way: per sample, the hull over the
in-band gates of the contributions they add to g_sigma_k / g_cdf_k / g_cdf_k+1 is accepted, [lo - tol, hi + tol].  A sample no in-band gate
touches is strict.  CAPS (conditions on the inputs, decided by the reference alone; a case that breaks one changes its inputs): at most 1 % of a
case's compared gradient elements may be non-strict with a hull wider than their own tol, and at most 1 % of its rays may have UNKNOWN depth -
SAFETY d(inv) > inv / 2 (the denominator is not pinned down) or a bound above a quarter of the ray's depth span (depth is a mean of the d_k: a
wider bound tells nothing).  The one all-empty-rays case (`depth_exempt`) is exempt from the depth cap: it asserts acc, rgb, tau and reports its
unknown depths.  The case matrix below is fixed by its generators alone (kinds, seeds, the two constant windows samples are moved out of): it never
consults the reference, so a change of the model cannot change what the GPU runs - it can only make test_caps_hold_for_every_case fail.
"""
import numpy as np
import torch

from oracle import render as orender
from oracle import sampling
from stage_ref import U, SAFETY, EXP_ZERO, EXP_INF_HI, ONE_R, seg_of, ulp32, bits, same_bits, depth_rows   # noqa: F401

TINY = 2.0 ** -126
DEN = 2.0 ** -148                   # one denormal step and a bit: where exp or a division ends below the normal range
ONE_R_LO = 16.6                     # below it fp32 sigmoid is certainly < 1
X_GATE = 2.0 ** -120                # relu(sigma delta) above it: certainly > 0 in fp32
CAP = 0.01
P_LIST = [2, 3, 64, 65, 66, 128, 129, 130, 192, 257, 512, 513]
P_FWD_ONLY = [514, 1025]            # seg 9 and 16: the forward runs, the backward refuses (P > 513)
BETAS = [0.1, 0.013, 0.002, 0.0005]
S_LIST = [20.0, 64.0, 512.0, 2048.0, 4096.0]
PRELOAD = np.array([0.375, -2.5], np.float32)     # g_alpha_beta / g_s start from it: the result is preload + gradient


def _t(x):
    return torch.as_tensor(np.array(x, dtype=np.float64))


def _excl_cumsum(x):
    return np.concatenate([np.zeros_like(x[:, :1]), np.cumsum(x, -1)[:, :-1]], -1)


def _excl_suffix(x):
    return np.concatenate([np.cumsum(x[:, ::-1], -1)[:, ::-1][:, 1:], np.zeros_like(x[:, :1])], -1)


def _gbg_abs(g, gacc, white, R):
    """|terms| of the opacity cotangent g_bg = -sum g_rgb (white background) + g_acc, per ray."""
    return np.broadcast_to((np.abs(g).sum(-1) if white else 0.0) + (0.0 if gacc is None else np.abs(gacc)), (R,))


def _normals(nab, wgt, dwgt, cost):
    """sum_k n_k w_k over the first P - 1 samples, n = nabla / max(|nabla|, 1e-12) -> (value [R, 3], bound [R, 3])."""
    v = nab[:, :-1]
    nrm = np.sqrt((v * v).sum(-1, keepdims=True))
    big = np.abs(v).max(-1, keepdims=True)
    # the modelled domain: the zero vector, a norm far below the 1e-12 floor, or squares inside fp32's normal range
    if not np.all((nrm == 0) | (nrm < 1e-13) | ((nrm > 1e-11) & (big < 1e18))):
        raise ValueError("nabla outside the modelled domain of F.normalize")
    n = v / np.maximum(nrm, 1e-12)
    val = (n * wgt[..., None]).sum(-2)
    bound = (np.abs(n) * dwgt[..., None] + 7 * U * np.abs(n) * wgt[..., None]).sum(-2) + cost * U * (np.abs(n) * wgt[..., None]).sum(-2)
    return val, bound


def _depth(wgt, dwgt, dk, ddk, cost):
    """sum w_k / (sum w + 1e-10) d_k -> (value, bound, unknown) per ray."""
    acc = wgt.sum(-1)
    dacc = dwgt.sum(-1) + cost * U * acc
    inv = acc + 1e-10
    dinv = dacc + U * inv
    depth = (wgt / inv[:, None] * dk).sum(-1)
    unknown = SAFETY * dinv > 0.5 * inv
    with np.errstate(divide="ignore", invalid="ignore"):
        dd = ((dwgt * np.abs(dk) + wgt * ddk).sum(-1) + np.abs(depth) * dinv) / np.where(unknown, np.nan, inv - SAFETY * dinv) \
            + (cost + 3) * U * np.abs(depth)
    span = dk.max(-1) - dk.min(-1)
    unknown |= ~(SAFETY * dd <= 0.25 * span + TINY) & (span > 0)
    if dk.shape[1] == 1:                                   # P = 2: one interval, depth = w / inv d_0 - known unless the denominator is not
        unknown = SAFETY * dinv > 0.5 * inv
    return depth, np.where(unknown, np.inf, dd), unknown, acc, dacc


# ==== VolSDF ================================================================================================================================
def volsdf_reference(c):
    """c: a case (fp32 inputs) -> dict name -> (ref, bound) of float64 arrays, plus 'lo' / 'hi' hulls for the gradients, 'unknown' [R] and
    'nonstrict' (count of gradient elements whose hull is wider than their tol)."""
    d, s, rad = (np.asarray(c[k], np.float64) for k in ("d", "sdf", "rad"))
    nab = None if c["nabla"] is None else np.asarray(c["nabla"], np.float64)
    R, P = d.shape
    al, be, white = float(c["alpha"]), float(c["beta"]), bool(c["white"])
    cost = 2 * seg_of(P) + 8
    o = orender.volsdf_composite(_t(d), sampling.sdf_to_sigma(_t(s), _t(al), _t(be)), _t(rad), None, white)
    # ---- forward values and bounds
    xs = np.abs(s) / be
    e = 0.5 * np.exp(-xs)
    psi = np.where(s >= 0, e, 1 - e)
    rel_psi = (np.where(s >= 0, xs, xs * e / (1 - e)) + 3) * U
    sig = al * psi
    sig_zero = (s >= 0) & (xs > EXP_ZERO)
    sig = np.where(sig_zero, 0.0, sig)
    dsig = np.where(sig_zero, 0.0, sig * (rel_psi + U) + al * DEN)
    delta = d[:, 1:] - d[:, :-1]
    x = np.maximum(sig[:, :-1] * delta, 0.0)
    x_zero = sig_zero[:, :-1] | (delta <= 0)
    dx = np.where(x_zero, 0.0, x * (rel_psi[:, :-1] + 3 * U) + al * DEN * np.abs(delta))
    p_zero = x > EXP_ZERO
    p = np.where(p_zero, 0.0, np.exp(-x))
    dp = np.where(x_zero | p_zero, 0.0, p * (dx + 2 * U) + DEN)
    q = 1 - p + 1e-10
    dq = dp + 2 * U * q
    T = np.concatenate([np.ones((R, 1)), np.cumprod(p, -1)[:, :-1]], -1)
    relT = _excl_cumsum(np.where(x_zero, 0.0, dx + 2 * U)) + cost * U
    dT = T * np.expm1(SAFETY * relT) / SAFETY + 2.0 ** -140
    tau = q * T
    dtau = dq * T + q * dT + U * tau
    # (1 - p next to 0 is only as good as the host's fp64 exp: an ulp of p, whatever the size of q)
    assert np.all(np.abs(tau - o["visibility_weights"].numpy()) <= 1e-9 * tau + 1e-15 * T + 1e-40), "the bound's own forward left the oracle's"
    depth, ddepth, unknown, acc, dacc = _depth(tau, dtau, d[:, :-1], np.zeros_like(tau), cost)
    cabs = np.abs(rad[:, :-1])
    rgb = (tau[..., None] * rad[:, :-1]).sum(-2)
    drgb = (dtau[..., None] * cabs).sum(-2) + (cost + 1) * U * (tau[..., None] * cabs).sum(-2)
    if white:
        rgb = rgb + (1 - acc)[:, None]
        drgb = drgb + (dacc + U * np.abs(1 - acc))[:, None] + U * np.abs(rgb)
    out = dict(rgb=(rgb, drgb), acc=(acc, dacc), depth=(depth, ddepth), sigma=(sig, dsig), p=(p, dp), tau=(tau, dtau), unknown=unknown)
    if nab is not None:
        out["normals"] = _normals(nab, tau, dtau, cost)
    assert np.allclose(rgb, o["rgb"].numpy(), rtol=1e-9, atol=1e-12) and np.allclose(acc, o["mask_volume"].numpy(), rtol=1e-9, atol=1e-15 * P)
    if P > 513:
        return out
    # ---- backward: float64 autograd through the oracle's functions is the reference ...
    if np.any(s == 0):
        raise ValueError("sdf == 0 exactly: |s| has no derivative there")
    g = np.asarray(c["g_rgb"], np.float64)
    gacc = None if c["g_acc"] is None else np.asarray(c["g_acc"], np.float64)
    ts, tr, ta, tb = _t(s).requires_grad_(True), _t(rad).requires_grad_(True), _t(al).requires_grad_(True), _t(be).requires_grad_(True)
    oo = orender.volsdf_composite(_t(d), sampling.sdf_to_sigma(ts, ta, tb), tr, None, white)
    loss = (oo["rgb"] * _t(g)).sum() + (0 if gacc is None else (oo["mask_volume"] * _t(gacc)).sum())
    loss.backward()
    ref_gs, ref_gr, ref_ga, ref_gb = ts.grad.numpy(), tr.grad.numpy(), float(ta.grad), float(tb.grad)
    # ... and the same formulas in numpy carry the bounds and the gates
    gbg = (-g.sum(-1) if white else 0.0) + (0.0 if gacc is None else gacc)
    gbg = np.broadcast_to(gbg, (R,))
    gtau = (rad[:, :-1] * g[:, None, :]).sum(-1) + gbg[:, None]
    dgtau = 4 * U * ((cabs * np.abs(g)[:, None, :]).sum(-1) + _gbg_abs(g, gacc, white, R)[:, None])
    g_rad = np.concatenate([tau[..., None] * g[:, None, :], np.zeros((R, 1, 3))], 1)
    dg_rad = np.concatenate([dtau[..., None] * np.abs(g)[:, None, :] + U * np.abs(g_rad[:, :-1]), np.zeros((R, 1, 3))], 1)
    h = tau * gtau
    dh = dtau * np.abs(gtau) + tau * dgtau + 2 * U * np.abs(h)
    S = _excl_suffix(h)
    dS = _excl_suffix(dh) + cost * U * _excl_suffix(np.abs(h))
    pT = p * T
    dpT = dp * T + p * dT + U * pT
    gx = pT * gtau - S
    dgx = dpT * np.abs(gtau) + pT * dgtau + U * np.abs(pT * gtau) + dS + U * np.abs(gx)
    gsig = gx * delta
    dgsig = dgx * np.abs(delta) + 2 * U * np.abs(gsig)
    on_ref = (al * psi[:, :-1] * delta) > 0                                 # fp64's own gate (its sigma underflows far later than fp32's)
    certain_on = x > X_GATE
    inband = ~certain_on & ~x_zero                                          # x_zero: delta <= 0 or sigma certainly 0 - the gate is certainly off
    es, sk, psik = e[:, :-1], s[:, :-1], psi[:, :-1]
    fac = al * es / be
    v = -gsig * fac
    dv = dgsig * fac + np.abs(gsig) * (fac * (xs[:, :-1] + 6) * U + al / be * DEN)
    # fp64's gate is on where fp32's sigma is certainly 0 (e < 2^-150): those contributions are below DEN and sit in the tolerance
    analytic = np.where(on_ref, v, 0.0)
    assert np.allclose(analytic, ref_gs[:, :-1], rtol=1e-7, atol=1e-9 * (np.abs(ref_gs).max() + 1e-300)), "analytic g_sdf left autograd's"
    strict = np.where(certain_on, v, 0.0)
    vin = np.where(inband, v, 0.0)
    z1 = np.zeros((R, 1))
    lo = np.concatenate([strict + np.minimum(vin, 0), z1], -1)
    hi = np.concatenate([strict + np.maximum(vin, 0), z1], -1)
    tol = np.concatenate([np.where(certain_on | inband, dv, np.abs(np.where(on_ref, v, 0.0))), z1], -1)
    out["g_sdf"] = (ref_gs, tol)
    out["g_sdf_hull"] = (lo, hi)
    out["g_rad"] = (g_rad, dg_rad)
    assert np.all(np.abs(g_rad - ref_gr) <= 1e-9 * np.abs(g_rad) + 1e-15 * np.abs(g)[:, None, :] + 1e-40)
    nonstrict = int(((hi - lo) > SAFETY * tol + TINY).sum())
    # d / d alpha and d / d beta: sums over every interval of every ray, accumulated with atomics
    tA = gsig * psik
    dtA = dgsig * psik + np.abs(tA) * (rel_psi[:, :-1] + U)
    tB = gsig * al * es * sk / (be * be)
    dtB = dgsig * np.abs(al * es * sk / (be * be)) + np.abs(tB) * (xs[:, :-1] + 8) * U
    for name, t, dt, ref in (("g_alpha", tA, dtA, ref_ga), ("g_beta", tB, dtB, ref_gb)):
        tot = np.where(certain_on, t, 0.0).sum()
        assert np.isclose(np.where(on_ref, t, 0.0).sum(), ref, rtol=1e-7, atol=1e-9 * np.abs(t).sum() + 1e-300), f"analytic {name} left autograd's"
        band = np.abs(np.where(inband, t, 0.0)).sum()
        out[name] = (np.float64(ref), np.float64(np.where(certain_on | inband, dt, 0.0).sum() + (R + cost) * U * np.abs(t).sum() + band + abs(ref - tot)))
    out["nonstrict"], out["elements"] = nonstrict, R * P
    return out


# ==== NeuS ==================================================================================================================================
def _cdf(z):
    with np.errstate(over="ignore"):
        ct = 1.0 / (1.0 + np.exp(-z))
    one, zero = z > ONE_R, z < -EXP_INF_HI
    c = np.where(one, 1.0, np.where(zero, 0.0, ct))
    dc = np.where(one | zero, 0.0, c * (1 - c) * (np.abs(z) + 2) * U + 2 * U * c + DEN)
    dc = np.where(~zero & (c < TINY), c + DEN, dc)          # a denormal quotient: it may as well be flushed to 0
    return ct, c, dc


def _alpha_T(c, dc, R):
    c0, c1, d0, d1 = c[:, :-1], c[:, 1:], dc[:, :-1], dc[:, 1:]
    num, den = c0 - c1, c0 + 1e-10
    raw = num / den
    draw = (d0 + d1 + U * np.abs(num) + np.abs(raw) * (d0 + U * den)) / den + U * np.abs(raw)
    off = raw + SAFETY * draw <= 0
    a = np.maximum(raw, 0.0)
    da = np.where(off, 0.0, draw)
    f = 1 - a + 1e-10
    df = da + 2 * U * f
    one = np.ones((R, 1))
    T = np.cumprod(np.concatenate([one, f], -1), -1)[:, :-1]
    T_hi = np.cumprod(np.concatenate([one, np.minimum(f + SAFETY * df, 1.0 + 1e-10)], -1), -1)[:, :-1]
    T_lo = np.cumprod(np.concatenate([one, np.maximum(f - SAFETY * df, 0.0)], -1), -1)[:, :-1]
    chain = SAFETY * (2 * seg_of(c.shape[1]) + 8) * U
    dT = np.maximum(T_hi * (1 + chain) - T, T - T_lo * (1 - chain)) / SAFETY + 2.0 ** -140
    return raw, draw, a, da, f, df, T, dT


def neus_reference(c):
    d, sdf, rad = (np.asarray(c[k], np.float64) for k in ("d", "sdf", "rad"))
    nab = None if c["nabla"] is None else np.asarray(c["nabla"], np.float64)
    R, P = sdf.shape
    s, white = float(c["s"]), bool(c["white"])
    cost = 2 * seg_of(P) + 8
    ct, cs, dc = _cdf(sdf * s)
    raw, draw, a, da, f, df, T, dT = _alpha_T(cs, dc, R)
    w = a * T
    dw = da * T + a * dT + U * w
    o_cdf, o_a = orender.sdf_to_alpha(_t(sdf), s)
    o_w = orender.alpha_to_w(o_a).numpy()
    assert np.allclose(ct, o_cdf.numpy(), rtol=1e-12, atol=0) and np.all(np.abs(a - o_a.numpy()) <= 2.0 ** -24)
    snapped = (cs != ct)
    clean = ~(snapped[:, :-1] | snapped[:, 1:]).any(-1)
    assert np.allclose(w[clean], o_w[clean], rtol=1e-9, atol=1e-14), "the bound's own forward left the oracle's"   # c0 - c1 cancels: the host's fp64 exp
    dmid = 0.5 * (d[:, 1:] + d[:, :-1])
    depth, ddepth, unknown, acc, dacc = _depth(w, dw, dmid, U * np.abs(dmid), cost)
    cabs = np.abs(rad)
    rgb = (w[..., None] * rad).sum(-2)
    drgb = (dw[..., None] * cabs).sum(-2) + (cost + 1) * U * (w[..., None] * cabs).sum(-2)
    if white:
        rgb = rgb + (1 - acc)[:, None]
        drgb = drgb + (dacc + U * np.abs(1 - acc))[:, None] + U * np.abs(rgb)
    out = dict(rgb=(rgb, drgb), acc=(acc, dacc), depth=(depth, ddepth), cdf=(cs, dc), alpha=(a, da), w=(w, dw), d_mid=(dmid, None), unknown=unknown)
    if nab is not None:
        out["normals"] = _normals(nab, w, dw, cost)
    if P > 513:
        return out
    # ---- backward: float64 autograd through sdf_to_alpha / alpha_to_w
    g = np.asarray(c["g_rgb"], np.float64)
    gacc = None if c["g_acc"] is None else np.asarray(c["g_acc"], np.float64)
    ts, tr, tS = _t(sdf).requires_grad_(True), _t(rad).requires_grad_(True), _t(s).requires_grad_(True)
    _, ta = orender.sdf_to_alpha(ts, tS)
    tw = orender.alpha_to_w(ta)
    trgb = (tw[..., None] * tr).sum(-2)
    tacc = tw.sum(-1)
    if white:
        trgb = trgb + (1.0 - tacc[..., None])
    ((trgb * _t(g)).sum() + (0 if gacc is None else (tacc * _t(gacc)).sum())).backward()
    ref_gs, ref_gr, ref_gS = ts.grad.numpy(), tr.grad.numpy(), float(tS.grad)
    # the same in numpy on the TRUE fp64 values (for the self-check and the gates' contributions); the bounds add the distance of the values
    # fp32 is certain of (cdf snapped to 0 / 1) to the true ones
    _, _, at, _, ft, _, Tt, _ = _alpha_T(ct, np.zeros_like(ct), R)
    rawt = (ct[:, :-1] - ct[:, 1:]) / (ct[:, :-1] + 1e-10)
    dcb = dc + np.abs(ct - cs)
    dab = da + np.abs(at - a)
    dfb = dab + 2 * U * ft
    dTb = dT + np.abs(Tt - T)
    wt = at * Tt
    dwb = dab * Tt + at * dTb + U * wt
    gbg = np.broadcast_to((-g.sum(-1) if white else 0.0) + (0.0 if gacc is None else gacc), (R,))
    gw = (rad * g[:, None, :]).sum(-1) + gbg[:, None]
    dgw = 4 * U * ((cabs * np.abs(g)[:, None, :]).sum(-1) + _gbg_abs(g, gacc, white, R)[:, None])
    g_rad = wt[..., None] * g[:, None, :]
    dg_rad = dwb[..., None] * np.abs(g)[:, None, :] + U * np.abs(g_rad)
    assert np.all(np.abs(g_rad - ref_gr) <= 1e-9 * np.abs(g_rad) + 1e-14 * np.abs(g)[:, None, :])
    n = P - 1
    V, dV, Va = np.zeros((R, n)), np.zeros((R, n)), np.zeros((R, n))
    fhi = np.minimum(ft + SAFETY * dfb, 1.0 + 1e-10)
    for k in range(n - 2, -1, -1):
        t = gw[:, k + 1] * at[:, k + 1]
        V[:, k] = t + ft[:, k + 1] * V[:, k + 1]
        Va[:, k] = np.abs(t) + ft[:, k + 1] * Va[:, k + 1]
        dV[:, k] = at[:, k + 1] * dgw[:, k + 1] + np.abs(gw[:, k + 1]) * dab[:, k + 1] + dfb[:, k + 1] * np.abs(V[:, k + 1]) + fhi[:, k + 1] * dV[:, k + 1]
    dV = dV + (cost + 4) * U * Va + 2.0 ** -110
    ga = Tt * (gw - V)
    dga = dTb * np.abs(gw - V) + Tt * (dgw + dV) + 3 * U * Tt * (np.abs(gw) + Va) + 2.0 ** -140
    c0, c1, d0, d1 = ct[:, :-1], ct[:, 1:], dcb[:, :-1], dcb[:, 1:]
    B = (c1 + 1e-10) / (c0 + 1e-10) ** 2
    D = 1.0 / (c0 + 1e-10)
    vB, vD = ga * B, -ga * D
    # B = (1 - raw) / den is how autograd through the quotient evaluates it: next to alpha = 1 that carries d(raw) / den ABSOLUTELY.  The kernels'
    # closed form does not need the term; an independent fp32 implementation (the float32 torch oracle) does, and the comparator must accept both
    dvB = dga * B + np.abs(vB) * (d1 / (c1 + 1e-10) + 2 * d0 / (c0 + 1e-10) + 5 * U) + np.abs(ga) * (draw + np.abs(rawt - raw)) * D
    dvD = dga * D + np.abs(vD) * (d0 / (c0 + 1e-10) + 2 * U)
    on_ref = rawt >= 0          # torch's clamp_min passes the gradient AT the bound (the kernel's `a > 0` does not): an exact tie is an in-band gate
    band = SAFETY * (draw + np.abs(rawt - raw)) + TINY
    certain_on = (rawt > band) & (raw > 0)
    inband = ~certain_on & (rawt > -band)
    z1 = np.zeros((R, 1))

    def scatter(xB, xD):
        return np.concatenate([xB, z1], -1) + np.concatenate([z1, xD], -1)
    gcdf_ref = scatter(np.where(on_ref, vB, 0), np.where(on_ref, vD, 0))
    m = ct * (1 - ct) * s
    assert np.allclose(gcdf_ref * m, ref_gs, rtol=1e-6, atol=1e-9 * (np.abs(ref_gs).max() + 1e-300)), "analytic g_sdf left autograd's"
    strict = scatter(np.where(certain_on, vB, 0), np.where(certain_on, vD, 0))
    vBi, vDi = np.where(inband, vB, 0), np.where(inband, vD, 0)
    L = strict + scatter(np.minimum(vBi, 0), np.minimum(vDi, 0))
    H = strict + scatter(np.maximum(vBi, 0), np.maximum(vDi, 0))
    E = scatter(np.where(certain_on | inband, dvB, 0), np.where(certain_on | inband, dvD, 0))
    Eabs = scatter(np.where(certain_on | inband, np.abs(vB), 0), np.where(certain_on | inband, np.abs(vD), 0))
    dm = (dcb + 2 * U * ct * (1 - ct)) * s + 2 * U * m
    tol = E * m + np.maximum(np.abs(L), np.abs(H)) * dm + 2 * U * Eabs * m
    out["g_sdf"] = (ref_gs, tol)
    out["g_sdf_hull"] = (L * m, H * m)
    out["g_rad"] = (g_rad, dg_rad)
    out["nonstrict"], out["elements"] = int((((H - L) * m) > SAFETY * tol + TINY).sum()), R * P
    # d / d s = sum g_cdf_k c_k (1 - c_k) sdf_k over every sample of every ray (atomics)
    ms = np.abs(sdf) / s
    lo_s = (np.minimum(L * m * sdf / s, H * m * sdf / s)).sum()
    hi_s = (np.maximum(L * m * sdf / s, H * m * sdf / s)).sum()
    assert lo_s - 1e-9 * (Eabs * m * ms).sum() - 1e-300 <= ref_gS <= hi_s + 1e-9 * (Eabs * m * ms).sum() + 1e-300, "analytic g_s left autograd's"
    out["g_s"] = (np.float64(ref_gS), np.float64((tol * ms).sum() + (R + cost + 2) * U * (Eabs * m * ms).sum()))
    out["g_s_hull"] = (lo_s, hi_s)
    return out


# ==== the comparator ========================================================================================================================
class Report:
    """Failures, counters and the worst observed / bound ratio per output of one case."""

    def __init__(self, name):
        self.name, self.fail, self.rays, self.elements, self.nonstrict, self.unknown, self.ratio = name, [], 0, 0, 0, 0, {}

    def check(self, ok, msg):
        if not ok:
            self.fail.append(msg)

    def within(self, what, got, ref, bound, lo=None, hi=None, skip=None):
        """|got - ref| <= SAFETY bound + TINY, or with a hull lo - tol <= got <= hi + tol; skip: elements not compared (unknown depth)."""
        got = np.asarray(got, np.float64)
        tol = SAFETY * np.asarray(bound, np.float64) + TINY
        lo = ref if lo is None else lo
        hi = ref if hi is None else hi
        with np.errstate(invalid="ignore", divide="ignore"):
            excess = np.maximum(np.maximum(lo - got, got - hi), 0.0)
            ratio = np.where(excess == 0, 0.0, excess / tol)
        ratio = np.where(np.isfinite(got), ratio, np.inf)
        if skip is not None:
            ratio = np.where(skip, 0.0, ratio)
        worst = float(np.max(ratio)) if ratio.size else 0.0
        self.ratio[what] = max(self.ratio.get(what, 0.0), worst)
        if not worst <= 1.0:
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
            self.fail.append(f"{what}: {int(np.sum(ratio > 1))} of {ratio.size} outside their bound, worst {worst:.3g} x at {tuple(int(j) for j in i)}: "
                             f"got {got[i]!r}, reference [{np.asarray(lo)[i]!r}, {np.asarray(hi)[i]!r}], tol {tol[i]!r}")

    def line(self):
        r = "  ".join(f"{k} {v:.2f}" for k, v in self.ratio.items())
        return (f"  {self.name:<46s} rays {self.rays:4d}  elements {self.elements:7d}  non-strict {self.nonstrict:4d}  unknown depth {self.unknown:3d}  | {r}"
                + ("" if not self.fail else f"  FAIL: {self.fail[0]}"))


def check_caps(c, ref, rep):
    """The two 1 % caps, from the reference alone."""
    rep.rays, rep.unknown = c["n_rays"], int(ref["unknown"].sum())
    rep.nonstrict, rep.elements = ref.get("nonstrict", 0), ref.get("elements", 0)
    if not c.get("depth_exempt"):
        rep.check(rep.unknown <= CAP * rep.rays, f"{rep.unknown} of {rep.rays} rays have unknown depth (> {CAP:.0%}): fix the inputs")
    rep.check(rep.nonstrict <= CAP * max(rep.elements, 1), f"{rep.nonstrict} of {rep.elements} gradient elements are non-strict (> {CAP:.0%}): fix the inputs")


def check(c, o, ref=None, kernel_contract=True):
    """o: the outputs of one run of case c (None for an output the case passes NULL for) -> Report.  kernel_contract: also what the kernels
    promise bit for bit (the last sample's cotangents are +0); an independent implementation owes only the value 0."""
    fw = c["fw"]
    ref = ref or (volsdf_reference(c) if fw == "volsdf" else neus_reference(c))
    rep = Report(c["name"])
    check_caps(c, ref, rep)
    R, P = c["n_rays"], c["P"]
    for k in ("rgb", "acc"):
        rep.within(k, o[k], *ref[k])
    rep.within("depth", o["depth"], *ref["depth"], skip=ref["unknown"])
    detail = ("sigma", "p", "tau") if fw == "volsdf" else ("cdf", "alpha", "w")
    for k in detail + ("normals",):
        want = c["want"].get(k, True) and (k != "normals" or c["nabla"] is not None)
        rep.check((o.get(k) is not None) == want, f"{k}: output present / absent against the case")
        if o.get(k) is not None:
            rep.within(k, o[k], *ref[k])
    if fw == "neus" and o.get("d_mid") is not None:
        dm = ref["d_mid"][0]
        rep.within("d_mid", o["d_mid"], dm, ulp32(dm) / SAFETY)
    if P <= 513:
        rep.within("g_sdf", o["g_sdf"], ref["g_sdf"][0], ref["g_sdf"][1], *ref["g_sdf_hull"])
        rep.within("g_rad", o["g_rad"], *ref["g_rad"])
        if fw == "volsdf" and kernel_contract:
            rep.check(np.all(bits(o["g_sdf"][:, -1]) == 0) and np.all(bits(o["g_rad"][:, -1]) == 0), "the last sample's g_sdf / g_rad are not +0")
        names = ("g_alpha", "g_beta") if fw == "volsdf" else ("g_s",)
        acc_key = "g_ab" if fw == "volsdf" else "g_s"
        if c["want"].get(acc_key, True):
            got = np.asarray(o[acc_key], np.float64)
            for i, k in enumerate(names):
                pre = float(c["preload"][i])
                v, b = ref[k]
                lo, hi = ref.get(k + "_hull", (v, v))
                rep.within(k, got[i] - pre, v, b + (R + 1) * U * (abs(pre) + abs(v)), min(lo, v), max(hi, v))
        else:
            rep.check(o.get(acc_key) is None, f"{acc_key} returned although the case passes NULL")
    return rep


# ==== the case matrix (shared by the CPU self-tests and the GPU tests) ======================================================================
def _nablas(R, P, rng):
    nab = rng.standard_normal((R, P, 3)).astype(np.float32)
    nab[0, min(1, P - 2)] = 0.0                                             # one exactly zero vector: F.normalize's floor gives 0, not NaN
    if R > 1:
        nab[1, 0] = np.array([1e-20, 0.0, 0.0], np.float32) * np.float32(rng.choice([-1.0, 1.0]))   # norm 1e-20: below the floor
    return nab


def _volsdf_sdf(kind, d, beta, rng):
    x = d.astype(np.float64)
    P = x.size
    d0 = rng.uniform(1.5, 4.5)
    if kind == "cross":
        return (d0 - x) * rng.uniform(0.05, 0.3) + 0.004 * np.sin(7 * x + rng.uniform(0, 6))
    if kind == "graze":                                                     # random values as tests/test_gpu_train.py draws them, an opaque tail
        s = (rng.uniform(0, 1, P) - 0.4) * 0.3
        s[(3 * P) // 4:] = -0.2
        return s
    if kind == "inside":
        return -0.3 - 0.1 * np.sin(2 * x + rng.uniform(0, 6))
    if kind == "thin":                                                      # |sdf| of the order of beta: partial opacity, T never reaches 0
        return beta * (2.0 + 1.5 * np.sin(5 * x + rng.uniform(0, 6)))
    if kind == "empty":                                                     # sdf >> beta: sigma underflows to exactly 0 in fp32
        return 12.0 + 0.5 * np.sin(3 * x)
    if kind == "faint":                                                     # sigma tiny but not 0: 1 - p rounds to 0 in fp32 - depth is unknown
        return beta * rng.uniform(18.0, 30.0, P)
    raise ValueError(kind)


def _out_of_window(s, beta):
    """Move an sdf whose exp(-s / beta) would be a denormal (gate in band, sigma not a relative quantity) to where it underflows for certain."""
    xs = s / float(beta)
    return np.where((xs > 80.0) & (xs <= EXP_ZERO + 1), np.float32(1.25 * (EXP_ZERO + 1) * float(beta)), s).astype(np.float32)


VOLSDF_KINDS = ["cross", "graze", "inside", "thin", "empty", "cross", "graze", "thin"]
# rows of 2 or 3 samples: a crossing or a random row that short is mostly one faint interval (sigma tiny but not 0), whose depth no fp32 code
# can pin down - the short rows are opaque, partially opaque or exactly empty.  The kinds are fixed here; the matrix does not consult the reference.
VOLSDF_KINDS_SHORT = ["inside", "thin", "empty", "thin", "inside", "thin"]


def volsdf_case(name, P, beta, idx, R=24, kinds=None, depth_exempt=False):
    rng = np.random.default_rng(7000 + 31 * idx + P)
    beta = np.float32(beta)
    alpha = np.float32(np.float32(1.0) / beta)
    d = depth_rows(P, R, rng, dup=True)
    if P > 3:
        k = int(rng.integers(1, P - 2))
        r = 5 % R
        if d[r, k] == d[r, k + 1]:
            d[r, k + 1] = np.nextafter(d[r, k + 1], np.float32(7))
        d[r, k], d[r, k + 1] = d[r, k + 1], d[r, k]                         # one inverted pair (delta < 0): the relu must zero it
    pool = VOLSDF_KINDS if P >= 64 else VOLSDF_KINDS_SHORT
    kinds = kinds or [pool[r % len(pool)] for r in range(R)]
    sdf = np.stack([_volsdf_sdf(k, d[r], float(beta), rng) for r, k in enumerate(kinds)]).astype(np.float32)
    sdf = np.where(sdf == 0, np.float32(1e-3), sdf)
    keep = sdf[3 % R, 0]
    sdf = _out_of_window(sdf, beta)
    if P >= 64 and kinds[3 % R] == "thin":
        sdf[3 % R, 0] = np.float32(95.0 * float(beta))                      # ONE sample whose exp is a denormal: its gate is in the band
    else:
        sdf[3 % R, 0] = _out_of_window(np.array([keep], np.float32), beta)[0]
    bare = idx % 7 == 5                                                    # every detail output NULL: how the render path and hip.volsdf_composite call it
    c = dict(fw="volsdf", name=name, n_rays=R, P=P, d=d, sdf=sdf, rad=rng.uniform(0, 1, (R, P, 3)).astype(np.float32),
             nabla=_nablas(R, P, rng) if idx % 3 != 2 else None, alpha=alpha, beta=beta, white=idx % 2,
             g_rgb=rng.standard_normal((R, 3)).astype(np.float32), g_acc=rng.standard_normal(R).astype(np.float32) if idx % 4 >= 2 else None,
             want=dict(sigma=idx % 2 == 0 and not bare, p=idx % 3 != 1 and not bare, tau=idx % 7 != 3 and not bare, g_ab=idx % 5 != 4), preload=PRELOAD if idx % 2 else np.zeros(2, np.float32),
             depth_exempt=depth_exempt)
    return c


def volsdf_cases():
    cases = []
    for i, P in enumerate(P_LIST + P_FWD_ONLY):
        for j in range(2):
            beta = BETAS[(i + 2 * j) % 4]
            idx = 2 * i + j
            cases.append(volsdf_case(f"volsdf P={P} beta={beta:g} white={idx % 2}", P, beta, idx))
    cases.append(volsdf_case("volsdf P=192 beta=0.013 all-empty rays", 192, 0.013, 100, kinds=["empty", "faint"] * 12, depth_exempt=True))
    return cases


def _neus_sdf(kind, P, s, rng):
    t = np.linspace(0, 1, P)
    if kind == "noisy":                                                     # monotone decreasing plus noise, as tests/test_gpu_train.py
        return np.sort(rng.uniform(-0.3, 0.3, P))[::-1] + (rng.uniform(0, 1, P) - 0.5) * 0.02
    if kind == "clean":                                                     # a clean monotone crossing: one interval has alpha -> 1 at large s
        return 0.3 - 0.6 * t + rng.uniform(-1e-4, 1e-4)
    if kind == "outside":                                                   # cdf == 1 throughout (z > 17.5 at every s of the matrix)
        return 1.2 + 0.1 * np.sin(9 * t + rng.uniform(0, 6))
    if kind == "inside":
        return -0.5 - 0.1 * np.sin(9 * t + rng.uniform(0, 6))
    raise ValueError(kind)


NEUS_KINDS = ["noisy", "clean", "outside", "inside", "noisy", "clean"]


def neus_case(name, P, s, idx, R=24):
    rng = np.random.default_rng(9000 + 31 * idx + P)
    d = depth_rows(P, R, rng, dup=True)
    kinds = [NEUS_KINDS[r % len(NEUS_KINDS)] for r in range(R)]
    sdf = np.stack([_neus_sdf(k, P, s, rng) for k in kinds]).astype(np.float32)
    # where the cdf is within a few u of 1 without being 1 for certain (z in 11 .. 17.6), neighbouring cdfs differ by less than their own rounding
    # and the clamp's gate is in the band: such samples are moved to where fp32 saturates for certain - except on ray 0 of the longer rows, which keeps
    # its in-band gates (under the 1 % cap)
    zone = (sdf * np.float32(s) > 11.0) & (sdf * np.float32(s) < 17.6)
    zone[0] &= P < 64
    sdf = np.where(zone, np.float32(18.5 / s), sdf).astype(np.float32)
    bare = idx % 7 == 5                                                    # every detail output NULL
    c = dict(fw="neus", name=name, n_rays=R, P=P, d=d, sdf=sdf, rad=rng.uniform(0, 1, (R, P - 1, 3)).astype(np.float32),
             nabla=_nablas(R, P, rng) if idx % 3 != 1 else None, s=np.float32(s), white=(idx + 1) % 2,
             g_rgb=rng.standard_normal((R, 3)).astype(np.float32), g_acc=rng.standard_normal(R).astype(np.float32) if idx % 4 < 2 else None,
             want=dict(cdf=idx % 2 == 0 and not bare, alpha=idx % 3 != 0 and not bare, w=idx % 7 != 3 and not bare, d_mid=idx % 4 != 0 and not bare,
                       g_s=idx % 5 != 3),
             preload=PRELOAD[1:] if idx % 2 == 0 else np.zeros(1, np.float32), depth_exempt=False)
    return c


def neus_cases():
    cases = []
    for i, P in enumerate(P_LIST + P_FWD_ONLY):
        for j in range(2):
            s = S_LIST[(i + 2 * j + j) % 5]
            idx = 2 * i + j
            cases.append(neus_case(f"neus P={P} s={s:g} white={(idx + 1) % 2}", P, s, idx))
    return cases


# ==== the kernels' data flow in fp32 numpy: lane segments, shuffle scans, second pass (used by the CPU stand-ins and the exact checks) ========
F = np.float32


def lanes_of(x, nint, fill):
    """[R, nint, ...] -> [R, 64, seg, ...] padded with `fill`, and the mask of real intervals."""
    seg = (nint + 63) >> 6
    pad = 64 * seg - nint
    shape = x.shape[:1] + (pad,) + x.shape[2:]
    xp = np.concatenate([x, np.full(shape, fill, x.dtype)], 1)
    m = np.concatenate([np.ones(nint, bool), np.zeros(pad, bool)])
    return xp.reshape(x.shape[:1] + (64, seg) + x.shape[2:]), m.reshape(64, seg), seg


def wave_excl_prod(v):
    v = v.copy()
    o = 1
    while o < 64:
        t = v.copy()
        v[:, o:] = (t[:, o:] * t[:, :-o]).astype(F)
        o <<= 1
    return np.concatenate([np.ones_like(v[:, :1]), v[:, :-1]], 1)


def wave_sum(v):
    idx = np.arange(64)
    o = 32
    while o > 0:
        v = (v + v[:, idx ^ o]).astype(F)
        o >>= 1
    return v[:, 0]


def wave_excl_suffix_sum(v):
    v = v.copy()
    o = 1
    while o < 64:
        t = v.copy()
        v[:, :-o] = (t[:, :-o] + t[:, o:]).astype(F)
        o <<= 1
    return np.concatenate([v[:, 1:], np.zeros_like(v[:, :1])], 1)


def scan_T(fac, carry=True):
    """Transmittance before each interval from the per-interval factors [R, nint] (fp32), in the kernels' order: in-lane product, exclusive
    shuffle scan, in-lane sequential pass.  carry = False: the scan's result is dropped (every lane starts from 1)."""
    R, nint = fac.shape
    fl, m, seg = lanes_of(fac.astype(F), nint, F(1))
    lp = np.ones((R, 64), F)
    for i in range(seg):
        lp = (lp * fl[:, :, i]).astype(F)
    T0 = wave_excl_prod(lp) if carry else np.ones((R, 64), F)
    T = np.empty((R, 64, seg), F)
    cur = T0
    for i in range(seg):
        T[:, :, i] = cur
        cur = (cur * fl[:, :, i]).astype(F)
    return T.reshape(R, 64 * seg)[:, :nint]


def lane_sum(terms):
    """sum over the intervals in the kernels' order: in-lane sequential, then the butterfly."""
    R, nint = terms.shape
    tl, m, seg = lanes_of(terms.astype(F), nint, F(0))
    acc = np.zeros((R, 64), F)
    for i in range(seg):
        acc = (acc + tl[:, :, i]).astype(F)
    return wave_sum(acc)


def suffix_S(hterms, inclusive=False):
    """S before each interval's own term is added, walking each lane's segment backwards from the sum over the later lanes."""
    R, nint = hterms.shape
    hl, m, seg = lanes_of(hterms.astype(F), nint, F(0))
    hs = np.zeros((R, 64), F)
    for i in range(seg):
        hs = (hs + hl[:, :, i]).astype(F)
    S = wave_excl_suffix_sum(hs)
    out = np.empty((R, 64, seg), F)
    for i in range(seg - 1, -1, -1):
        if inclusive:
            S = (S + hl[:, :, i]).astype(F)
        out[:, :, i] = S
        if not inclusive:
            S = (S + hl[:, :, i]).astype(F)
    return out.reshape(R, 64 * seg)[:, :nint]
