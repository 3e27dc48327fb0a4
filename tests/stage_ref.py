"""fp64 references of the per-ray sampler stages and a comparator that is strict where the math is well conditioned.

The stages are the one-wave-per-ray kernels of csrc/volsdf_render.hip (k_first_check, k_upsample, k_merge_check, k_finalize_unconverged,
k_sort_concat, k_linspace_depths) and csrc/neus_render.hip (k_merge_pairs), built on the scans of
csrc/ray_common.h.  Every reference runs oracle/sampling.py on float64 tensors of the kernels' fp32 inputs and adds only
what one stage needs.  tests/test_stage_ref.py shows on the CPU that the comparator accepts an independent fp32 implementation and rejects
fp32 stand-ins with injected bugs; tests/test_gpu_ray_stages.py holds the HIP kernels to it.

ERROR MODEL (first order in the fp32 unit round-off u = 2^-24; the summation terms times SAFETY).  For a row of n samples the kernels cut the n - 1 intervals
into 64 lane segments of seg = ceil((n - 1) / 64): a running sum is a sequential segment sum, a 6-level shuffle scan and a second
sequential pass, so a partial sum S of non-negative terms carries at most (2 seg + 8) u S of summation error.  Per term:
  sigma_k delta_k   relative (|s_k| / beta + 7) u       (the rounding of the exp argument is |x| u; exp, divide, products, delta: 6 u)
  E term_k          relative (d*_k / beta + (|s_k| + |s_k+1| + delta_k) / beta + 9) u   (d* = max(.5 (|s_k| + |s_k+1| - delta), 0) cancels)
  B_k = exp(-R) (exp(E) - 1):   |dB| <= exp(-R) exp(E) (dE + 2 u) + B (dR + 4 u) + exp(E) 2^-148
The exp(E) term is the ABSOLUTE error of exp(E) - 1: it does not shrink with E, and against the +1e-5 floor of sample_pdf it is what
dominates the CDF error of a near-empty row.  The fp32 RANGE is kept exactly: exp(-x) is 0 for x > 104.5 (so a term or sigma beyond it is
exactly 0 and E = 0 gives B = 0 with no error), exp(E) overflows for E > 88.8 and is finite below 88.6 (NaN -> inf follows,
volsdf.py:56-94), and B is 'unknown' (dB = inf) in between; E < 2^-26 gives exp(E) == 1, i.e. B = 0 exactly.
CDF knots: the pdf CDF (k_upsample) moves by at most 2 sum(dw) / sum(w) + (2 seg + 10) u; the opacity CDF 1 - exp(-R) by
exp(-R) dR + 3 u.  Its knots are EXACT where fp32 decides them: 0 for R < 2^-30, 1 for R > 17.5 (exp(-R) < 2^-25).

COMPARATOR (icdf_bounds): the inverse CDF is monotone in u, so with the kernel's knots within du of the fp64 ones its sample lies in
[F^-1(u - du), F^-1(u + du)].  A sample whose u has no knot within du, and whose bracket denominator is not within 2 du of the 1e-5
threshold, must match F^-1(u) within slope * du + 4 ulp of depth (the STRICT path); the others get the hull of F^-1 at u -/+ du under both
readings of the threshold (the WIDENED path, counted).  Ties fp32 computes exactly are decided by searchsorted(right=False) itself: u = 0
gives bins[0], and u = 1 with every knot's side of 1 certain picks the bracket of the first knot that is exactly 1 (or bins[n-1]).
"""
import numpy as np
import torch

from oracle import sampling

U = 2.0 ** -24
SAFETY = 2.0
EXP_ZERO = 104.5                    # fp32 exp(-x) == 0 beyond (x > 103.97 rounds below half the least denormal)
EXP_INF_LO, EXP_INF_HI = 88.6, 88.8  # fp32 exp(x) overflows at x = 88.72
THR = float(np.float32(1e-5))        # invert_cdf_at: a denominator below 1e-5f becomes 1
ONE_R = 17.5                         # 1 - exp(-R) == 1 in fp32
ZERO_R = 2.0 ** -30                  # 1 - exp(-R) == 0 in fp32
WIDEN_MAX = 0.01                     # a case fails if more than 1 % of its samples take the widened path


def f32(x):
    return np.float32(x)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _t(x):
    return torch.as_tensor(np.array(x, dtype=np.float64))


def _col(x, R):
    x = np.asarray(x, dtype=np.float64)
    return np.broadcast_to(x.reshape(-1, 1) if x.ndim else x, (R, 1))


def seg_of(n):
    return (n - 1 + 63) // 64


# ---- error bound (volsdf.py:56-94) at fp32 range ---------------------------------------------------------------------------------------
def bounds(d, s, alpha, beta, clamp=False):
    """d, s [R, n] (fp32 values), alpha, beta scalars or [R] (fp32 values) -> dict of float64 [R, n-1]: b, db (the bound and its error),
    R, dR (the opacity sum before each interval and its error).  b = inf where fp32 overflow makes it inf for certain; db = inf where
    it is uncertain whether it does.  clamp: [0, 1e5] as volsdf.py:282 / the kernel's clamp_bounds."""
    d = np.asarray(d, np.float64); s = np.asarray(s, np.float64)
    Rn, n = d.shape
    al, be = _col(alpha, Rn), _col(beta, Rn)
    depth = 2 * seg_of(n) + 8
    delta = d[:, 1:] - d[:, :-1]
    a = np.abs(s)
    # sigma (oracle a11) with fp32's underflow of 0.5 exp(-|s| / beta) for s >= 0
    x_sig = a[:, :-1] / be
    sig = sampling.sdf_to_sigma(_t(s[:, :-1]), _t(al), _t(be)).numpy()
    sig = np.where((s[:, :-1] >= 0) & (x_sig > EXP_ZERO), 0.0, sig)
    sd = sig * delta
    Rs = np.concatenate([np.zeros((Rn, 1)), np.cumsum(sd, -1)[:, :-1]], -1)
    dR = (depth * Rs + np.concatenate([np.zeros((Rn, 1)), np.cumsum((x_sig + 8) * sd, -1)[:, :-1]], -1)) * U
    dstar = np.maximum(0.5 * (a[:, :-1] + a[:, 1:] - delta), 0.0)
    x_e = dstar / be
    term = al / (4 * be) * delta ** 2 * np.exp(-x_e)
    term = np.where(x_e > EXP_ZERO, 0.0, term)
    q = x_e + (a[:, :-1] + a[:, 1:] + delta) / be + 10
    E = np.cumsum(term, -1)
    dE = (depth * E + np.cumsum(q * term, -1)) * U
    with np.errstate(over="ignore", invalid="ignore"):
        eR = np.exp(-Rs)
        eR = np.where(Rs > EXP_ZERO, 0.0, eR)
        eE = np.exp(np.minimum(E, EXP_INF_LO))
        b = eR * (eE - 1.0)
        db = eR * eE * (SAFETY * dE + 2 * U) + b * (SAFETY * dR + 4 * U)
        db = db + eE * 2.0 ** -148                      # a denormal exp(-R): absolute, not relative
    zero = E < 2.0 ** -26                                # every term 0, or fp32 exp(E) == 1: B = 0 exactly
    db = np.where(zero, 0.0, db)
    b = np.where(zero, 0.0, b)
    over = E > EXP_INF_HI
    unsure = (E >= EXP_INF_LO) & ~over
    b = np.where(over, np.inf, b)
    db = np.where(over, 0.0, np.where(unsure, np.inf, db))
    if clamp:
        cb = np.clip(b, 0.0, 1e5)
        hi_sure = np.isinf(b) | (b - db > 1e5)
        db = np.where(hi_sure, 0.0, np.where(unsure, 1e5, db))
        b = cb
    return dict(b=b, db=db, R=Rs, dR=dR * SAFETY)


def max_bound_range(d, s, alpha, beta):
    """[R] lower / upper ends of the max bound the kernel can compute (the wave_max of the scan)."""
    B = bounds(d, s, alpha, beta)
    with np.errstate(invalid="ignore"):
        lo = np.where(np.isinf(B["db"]), 0.0, B["b"] - B["db"]).max(-1)
        hi = (B["b"] + B["db"]).max(-1)
    return lo, hi, B["b"].max(-1)


def decide(lo, hi, eps):
    """'mx > eps' (k_first_check / merge_check_tail): +1 surely greater, -1 surely not, 0 in the band (both allowed)."""
    return np.where(lo > eps, 1, np.where(hi <= eps, -1, 0))


# ---- CDFs --------------------------------------------------------------------------------------------------------------------------------
def pdf_cdf(b, db):
    """k_upsample / sample_pdf (rend_util.py:256-265): w = b + 1e-5, cdf = [0, cumsum(w / sum w)] -> (cdf [R, n], du [R])."""
    if not np.all(np.isfinite(b)):
        raise ValueError("a pdf row with an infinite weight (out of scope: the fp32 reference itself returns NaN there)")
    w = b + THR
    dw = db + U * w
    tot = w.sum(-1, keepdims=True)
    cdf = np.concatenate([np.zeros((b.shape[0], 1)), np.cumsum(w / tot, -1)], -1)
    du = 2 * dw.sum(-1) / tot[:, 0] + SAFETY * (2 * seg_of(b.shape[1] + 1) + 10) * U
    return cdf, du


def opacity_cdf(d, s, alpha, beta):
    """opacity_invert_cdf_sample's CDF (volsdf.py:122-136 + the leading 0 of sample_cdf) -> (cdf [R, n], du [R], exact [R, n] bool)."""
    d = np.asarray(d, np.float64); s = np.asarray(s, np.float64)
    B = bounds(d, s, alpha, beta)
    Rs, dR = B["R"], B["dR"]
    ref = 1 - torch.exp(-sampling._opacity_R(_t(d), _t(s), _t(_col(alpha, d.shape[0])), _t(_col(beta, d.shape[0])))).numpy()
    # the oracle's R is the reference's; ours keeps fp32's sigma underflow - they agree wherever that underflow does not matter
    c = 1 - np.exp(-Rs)
    assert np.allclose(c, ref, rtol=0, atol=1e-12 + 1e-9 * np.abs(ref).max())
    zero, one = Rs < ZERO_R, Rs > ONE_R
    c = np.where(zero, 0.0, np.where(one, 1.0, c))
    dk = np.where(zero | one, 0.0, np.exp(-Rs) * dR + 3 * U * SAFETY)
    cdf = np.concatenate([np.zeros((d.shape[0], 1)), c], -1)
    exact = np.concatenate([np.ones((d.shape[0], 1), bool), zero | one], -1)
    return cdf, dk.max(-1), exact


# ---- the comparator ----------------------------------------------------------------------------------------------------------------------
def _invert(bins, cdf, u, thr):
    """oracle._invert_cdf (lower-bound bracket, clamp, small denominators -> 1) on float64 with an explicit threshold."""
    return sampling._invert_cdf(_t(bins), _t(cdf), u.shape[-1], u=_t(u), eps=thr).numpy()


def icdf_bounds(bins, cdf, u, du, exact=None):
    """Interval [lo, hi] each kernel sample invert_cdf_at(bins, cdf_kernel, n, u) must lie in, and the widened-path mask.
    bins, cdf [R, n]; u [R, m] (fp32 values); du [R]: the knots' error; exact [R, n]: knots whose fp32 value is cdf itself."""
    bins = np.asarray(bins, np.float64); cdf = np.asarray(cdf, np.float64); u = np.asarray(u, np.float64)
    Rn, n = bins.shape
    du = np.asarray(du, np.float64).reshape(-1, 1) + 2 * U          # + the rounding of u - c0
    if exact is None:
        exact = np.zeros_like(bins, bool); exact[:, 0] = True
    idx = np.stack([np.searchsorted(cdf[r], u[r], side="left") for r in range(Rn)])
    below, above = np.clip(idx - 1, 0, n - 1), np.clip(idx, 0, n - 1)
    c0, c1 = np.take_along_axis(cdf, below, -1), np.take_along_axis(cdf, above, -1)
    b0, b1 = np.take_along_axis(bins, below, -1), np.take_along_axis(bins, above, -1)
    denom = c1 - c0
    ulps = 4 * np.maximum(ulp32(b0), ulp32(b1))
    near_knot = (np.abs(u - c0) <= du) | (np.abs(c1 - u) <= du)
    near_thr = np.abs(denom - THR) <= 2 * du
    val = _invert(bins, cdf, u, THR)
    slope = np.abs(b1 - b0) / np.where(denom < THR, 1.0, denom)
    lo, hi = val - slope * du - ulps, val + slope * du + ulps
    widened = near_knot | near_thr
    # the widened path: the hull of F^-1 at u -/+ du under both readings of the threshold (each row's own du)
    cand = [val]
    for r in np.nonzero(widened.any(-1))[0]:
        for sgn in (-1, 1):
            for sgn2 in (-1, 1):
                c = np.full_like(u, np.nan)
                c[r] = _invert(bins[r:r + 1], cdf[r:r + 1], np.clip(u[r:r + 1] + sgn * du[r], -1.0, 2.0), max(THR + sgn2 * 2 * du[r, 0], 0.0))[0]
                cand.append(c)
    cmin = np.nanmin(np.stack(cand), 0) - ulps
    cmax = np.nanmax(np.stack(cand), 0) + ulps
    lo, hi = np.where(widened, cmin, lo), np.where(widened, cmax, hi)
    # a hull no wider than the strict interval of the nearest real bracket (u = 1 past the last knot, say) is not counted as widened
    i2 = np.clip(idx, 1, n - 1)
    s2 = np.abs(np.take_along_axis(bins, i2, -1) - np.take_along_axis(bins, i2 - 1, -1)) / np.maximum(
        np.take_along_axis(cdf, i2, -1) - np.take_along_axis(cdf, i2 - 1, -1), THR)
    widened &= (cmax - cmin) > 2 * (np.maximum(s2, slope) * du + ulps)
    # exact ties: u = 0 -> bins[0]
    z = u == 0.0
    lo, hi = np.where(z, bins[:, :1], lo), np.where(z, bins[:, :1], hi)
    widened &= ~z
    # u = 1: lower_bound picks the first knot that is 1 in fp32 - at or after the first knot that may be 1, at or before the first that
    # surely is (none: n, i.e. bins[n-1]); the sample lies in the union of those brackets
    one = u == 1.0
    if one.any():
        for r in np.nonzero(one.any(-1))[0]:
            ex1 = exact[r] & (cdf[r] == 1.0)
            may1 = ex1 | (cdf[r] + du[r, 0] >= 1.0)
            k_hi = int(np.argmax(ex1)) if ex1.any() else n
            k_lo = int(np.argmax(may1)) if may1.any() else n
            if k_hi == n and k_lo < n:
                continue                                   # may or may not reach 1: the widened hull
            seg_b = bins[r, max(k_lo - 1, 0):min(k_hi, n - 1) + 1]
            l, h = seg_b.min(), seg_b.max()
            m = one[r]
            lo[r, m] = l - 4 * ulp32(l); hi[r, m] = h + 4 * ulp32(h)
            widened[r, m] = False
    return lo, hi, widened


class Report:
    """Failures and counters of one case: rays, samples, widened-path samples, rays in the decision band."""

    def __init__(self, name):
        self.name, self.fail, self.rays, self.samples, self.widened, self.band = name, [], 0, 0, 0, 0

    def check(self, ok, msg):
        if not ok:
            self.fail.append(msg)

    def samples_in(self, got, lo, hi, widened, what, sorted_rows=False):
        got = np.asarray(got, np.float64)
        if sorted_rows:
            lo, hi = np.sort(lo, -1), np.sort(hi, -1)
        bad = ~((got >= lo) & (got <= hi))
        self.samples += got.size
        self.widened += int(widened.sum())
        if bad.any():
            r, j = np.argwhere(bad)[0]
            self.fail.append(f"{what}: {int(bad.sum())} samples outside their interval, first row {r} col {j}: {got[r, j]!r} not in "
                             f"[{lo[r, j]!r}, {hi[r, j]!r}]")

    def finish(self):
        if self.samples and self.widened > WIDEN_MAX * self.samples:
            self.fail.append(f"{self.widened} of {self.samples} samples took the widened path (> {WIDEN_MAX:.0%}): fix the inputs")
        return self

    def line(self):
        return (f"  {self.name:<44s} rays {self.rays:5d}  samples {self.samples:7d}  widened {self.widened:5d}  band rays {self.band:3d}"
                + ("" if not self.fail else f"  FAIL: {self.fail[0]}"))


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- bisection for beta+ (volsdf.py:260-275, merge_check_tail) -----------------------------------------------------------------------
def bisect_outcomes(d, s, beta_net, beta_hi, eps, max_bisect, limit=256):
    """Every fp32 beta+ the kernel's bisection can end on for one row: mid = 0.5f (lo + hi) is emulated bit for bit, each step's decision
    m <= eps is taken from the fp64 bound and both branches are followed where it lies in the band.  -> (set of float32, band steps)."""
    out, band = set(), [0]
    d = np.asarray(d, np.float64)[None]; s = np.asarray(s, np.float64)[None]

    def rec(lo, hi, step):
        if step == max_bisect:
            out.add(np.float32(hi).item())
            return
        mid = f32(f32(lo + hi) * f32(0.5))
        alpha = f32(f32(1.0) / mid)
        mlo, mhi, _ = max_bound_range(d, s, float(alpha), float(mid))
        dec = decide(mlo, mhi, eps)[0]
        if dec == 0:
            band[0] += 1
        if len(out) > limit:
            raise RuntimeError("too many bisection outcomes: fix the inputs")
        if dec <= 0:
            rec(lo, mid, step + 1)
        if dec >= 0:
            rec(mid, hi, step + 1)
    rec(f32(beta_net), f32(beta_hi), 0)
    return out, band[0]


def beta_plus0(far, denom):
    """k_first_check: sqrtf((far * far) / denom) in fp32 (volsdf.py:149)."""
    far = np.asarray(far, np.float32)
    return np.sqrt((far * far) / np.float32(denom)).astype(np.float32)


def beta_plus0_denom(n0, eps):
    """fine_sample_run's fp32 denominator 4 (N0 - 1) log(1 + eps)."""
    return f32(4.0 * (n0 - 1) * np.log(1.0 + eps))


# ---- other exact stages ------------------------------------------------------------------------------------------------------------------
def linspace_depths(t, near, far, n_rays):
    """near (1 - t) + far t with the reference's three roundings (volsdf.py:474, :484): no FMA."""
    t = np.asarray(t, np.float32)[None, :]
    nr = np.broadcast_to(np.asarray(near, np.float32).reshape(-1, 1), (n_rays, 1))
    fr = np.broadcast_to(np.asarray(far, np.float32).reshape(-1, 1), (n_rays, 1))
    return ((nr * (np.float32(1) - t)).astype(np.float32) + (fr * t).astype(np.float32)).astype(np.float32)


def stable_merge(d_old, s_old, d_new, s_new):
    """cat + stable sort + gather (volsdf.py:217-228, neus.py:297-302): an old sample precedes a new one of equal depth."""
    d, s = sampling._merge_sorted(_t(d_old), _t(s_old), _t(d_new), _t(s_new))
    return d.numpy().astype(np.float32), s.numpy().astype(np.float32)


# ==== the case matrix (shared by the CPU self-tests and the GPU tests) ======================================================================
N_LIST = [2, 3, 40, 64, 65, 66, 512, 513, 514, 1025, 1026, 1537, 1538, 2048, 3584]   # seg = 8/9, 16/17, 24/25, generic; n < 64
N_FINAL = [1, 63, 64, 65]
SENT = np.float32(-7.25)        # output buffers start with it; whatever a stage must not touch keeps it
ISENT = -3                      # int sentinel of act_out
NEAR, FAR = 0.0, 6.0
ALPHA_NET, BETA_NET, EPS = 100.0, 0.01, 0.1
G6_ALPHA, G6_BETA, G6_NAN_ALPHA, G6_NAN_BETA = 100.0, 0.01, 1e4, 1e-4


def torch_lin(n):
    return torch.linspace(0, 1, n).numpy().astype(np.float32)


def sdf_rows(d, kinds, rng):
    """sdf rows of the given kinds on depth rows d [R, n] (fp32):
    cross   a smooth surface crossing (the realistic case; most of the mass in a few bins, opaque behind: opacity knots exactly 1)
    far     |s| / beta > 104 at beta 0.01 everywhere: fp32 sigma and every E term exactly 0 - flat CDFs, zero-bound runs (G7's case)
    gap     empty space (as far) in front of a crossing: a leading run of exactly-0 opacity knots, then the surface
    zero    s = 0 exactly
    inside  the origin inside the object: opaque from the first sample"""
    R, n = d.shape
    s = np.zeros((R, n), np.float64)
    for r, k in enumerate(kinds):
        x = d[r].astype(np.float64)
        d0 = rng.uniform(1.5, 4.5)
        if k == "cross":
            s[r] = (d0 - x) * rng.uniform(0.5, 1.0) + 0.02 * np.sin(7 * x)
        elif k == "far":
            s[r] = 2.0 + 0.1 * np.sin(3 * x)
        elif k == "gap":
            s[r] = np.where(x < d0 - 1.5, 2.0 + 0.1 * np.sin(3 * x), d0 - x)
        elif k == "zero":
            s[r] = 0.0
        elif k == "inside":
            s[r] = -0.5 - 0.1 * np.sin(2 * x)
        else:
            raise ValueError(k)
    return s.astype(np.float32)


def depth_rows(n, R, rng, dup=False):
    """Depth rows on [NEAR, FAR]: even rows the reference's linspace, odd rows sorted uniform draws; dup: repeated depths (delta = 0)."""
    d = np.empty((R, n), np.float32)
    lin = linspace_depths(torch_lin(n), NEAR, FAR, 1)[0]
    for r in range(R):
        d[r] = lin if r % 2 == 0 else np.sort(rng.uniform(NEAR, FAR, n).astype(np.float32))
        if dup and n > 3:
            k = rng.choice(np.arange(1, n), size=max(1, n // 16), replace=False)
            d[r, k] = d[r, k - 1]
            d[r] = np.sort(d[r])
    return d


def padded(x, cap, fill=np.nan):
    out = np.full((x.shape[0], cap), fill, np.float32)
    out[:, :x.shape[1]] = x
    return out


def kinds_for(R, pool):
    return [pool[r % len(pool)] for r in range(R)]


def u_rows(R, m, rng, knot_rows=None):
    """Per-ray uniform numbers (perturb): unsorted, with exactly 0, 1 - 2^-24 and (knot_rows [R, k] given) a value equal to an fp32 knot."""
    u = rng.uniform(0, 1, (R, m)).astype(np.float32)
    for r in range(0, R, 5):                   # every fifth ray: a value on a knot is a widened sample by construction
        slots = rng.permutation(m)
        u[r, slots[0]] = 0.0
        if m > 1:
            u[r, slots[1]] = np.float32(1 - 2.0 ** -24)
        if m > 2 and knot_rows is not None:
            inner = knot_rows[r][(knot_rows[r] > 0) & (knot_rows[r] < 1)]
            if inner.size:
                u[r, slots[2]] = inner[rng.integers(inner.size)]
    return u


def fp32_opacity_knots(d, s, alpha, beta):
    """fp32 knots of the opacity CDF (torch fp32 oracle) - only to place u values on them."""
    R = d.shape[0]
    al = torch.as_tensor(np.asarray(alpha, np.float32)).reshape(-1, 1).expand(R, 1)
    be = torch.as_tensor(np.asarray(beta, np.float32)).reshape(-1, 1).expand(R, 1)
    c = 1 - torch.exp(-sampling._opacity_R(torch.as_tensor(d), torch.as_tensor(s), al, be))
    return torch.cat([torch.zeros(R, 1), c], -1).numpy()


def act_subset(R, rng):
    """A permuted strict subset of the rays (never the identity); the rays left out must keep their sentinels."""
    k = max(1, (3 * R) // 4)
    act = rng.permutation(R)[:k].astype(np.int32)
    if k > 1 and np.array_equal(act, np.arange(k)):
        act = act[::-1].copy()
    return act


# ---- VolSDF stage cases ----------------------------------------------------------------------------------------------------------------------
def g6():
    """The G6 rows of the real reference's goldens (tests/golden/make_golden.py): 8 rays of n = 40, scalar (alpha, beta) = (100, 0.01), a
    per-ray beta, and the NaN -> inf rows (alpha, beta) = (1e4, 1e-4) whose row 0 has every bound inf."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "renderer_golden.npz"))
    return {k: z[k] for k in z.files if k.startswith("G6_")}


def first_check_cases(R=48):
    G = g6()
    cases = [_first_check_case("first_check G6 scalar", G["G6_d"], G["G6_s"], 43, 64, EPS, G6_ALPHA, G6_BETA, torch_lin(64), None,
                               np.random.default_rng(90)),
             _first_check_case("first_check G6 NaN->inf", G["G6_nan_d"], G["G6_nan_s"], 41, 63, EPS, G6_NAN_ALPHA, G6_NAN_BETA, torch_lin(63),
                               np.full(8, 6000.0, np.float32), np.random.default_rng(91))]
    for i, n in enumerate(N_LIST):
        rng = np.random.default_rng(100 + i)
        n_final = N_FINAL[i % 4]
        d = depth_rows(n, R, rng, dup=(i % 3 == 1))
        s = sdf_rows(d, kinds_for(R, ["cross", "far", "gap", "zero", "inside", "cross"]), rng)
        per_ray = i % 2 == 1
        if per_ray:
            u = u_rows(R, n_final, rng, fp32_opacity_knots(d, s, ALPHA_NET, BETA_NET))
        else:
            u = torch_lin(n_final)
        far = rng.uniform(4.0, 6.0, R).astype(np.float32) if i % 3 == 0 else None
        cases.append(_first_check_case(f"first_check n={n} nf={n_final}{' perturb' if per_ray else ''}", d, s, n + 3 + i % 5, n_final, EPS,
                                       ALPHA_NET, BETA_NET, u, far, rng))
    return cases


def _first_check_case(name, d, s, cap, n_final, eps, alpha, beta, u, far, rng):
    R, n = d.shape
    return dict(stage="first_check", name=name, n_rays=R, n=n, cap=cap, n_final=n_final, eps=np.float32(eps), alpha_net=np.float32(alpha),
                beta_net=np.float32(beta), dA=padded(d, cap), sA=padded(s, cap), u_final=np.ascontiguousarray(u, np.float32),
                u_stride=n_final if u.ndim == 2 else 0, denom=beta_plus0_denom(n, eps), far=far, far_s=np.float32(FAR),
                out=dict(d_fine=np.full((R, n_final), SENT, np.float32), beta_plus=np.full(R, SENT, np.float32),
                         beta_map=np.full(R, SENT, np.float32), iter_usage=np.full(R, SENT, np.float32),
                         act_out=np.full(R, ISENT, np.int32), act_count=np.zeros(1, np.int32)))


def _opacity_check(rep, what, d, s, alpha, beta, u, got, sorted_rows=False):
    cdf, du, exact = opacity_cdf(d, s, alpha, beta)
    lo, hi, wid = icdf_bounds(d, cdf, u, du, exact)
    rep.samples_in(got, lo, hi, wid, what, sorted_rows)


def _u_of(case, rays):
    u = case["u_final"]
    return u[rays] if u.ndim == 2 else np.broadcast_to(u, (len(rays), u.shape[0]))


def check_first_check(case, o):
    rep = Report(case["name"])
    R, n = case["n_rays"], case["n"]
    d, s = case["dA"][:, :n], case["sA"][:, :n]
    lo, hi, _ = max_bound_range(d, s, case["alpha_net"], case["beta_net"])
    dec = decide(lo, hi, case["eps"])
    rep.rays, rep.band = R, int((dec == 0).sum())
    conv = o["iter_usage"] == 0.0
    act = np.zeros(R, bool)
    cnt = int(o["act_count"][0])
    rep.check(0 <= cnt <= R, f"act_count {cnt}")
    listed = o["act_out"][:max(0, min(cnt, R))]
    rep.check(len(set(listed.tolist())) == len(listed) and np.all((listed >= 0) & (listed < R)), "act_out is not a set of rays")
    act[listed[(listed >= 0) & (listed < R)]] = True
    rep.check(np.all(o["act_out"][cnt:] == ISENT), "act_out written past act_count")
    rep.check(np.all(conv ^ act), "a ray neither converged nor active, or both")
    rep.check(np.all(np.where(dec > 0, act, True)) and np.all(np.where(dec < 0, conv, True)), "convergence decision outside the band")
    # converged: samples of the opacity CDF at the net's (alpha, beta), beta_map = beta_net; beta_plus untouched
    c = np.nonzero(conv)[0]
    if c.size:
        _opacity_check(rep, "d_fine", d[c], s[c], case["alpha_net"], case["beta_net"], _u_of(case, c), o["d_fine"][c])
    rep.check(same_bits(o["beta_map"][c], np.full(c.size, case["beta_net"])), "beta_map of converged rays")
    rep.check(same_bits(o["beta_plus"][c], np.full(c.size, SENT)), "beta_plus written for a converged ray")
    # active: beta+_0 = sqrtf(far^2 / denom) exactly; no samples, no beta_map, no iter_usage
    a = np.nonzero(act)[0]
    far = case["far"][a] if case["far"] is not None else np.full(a.size, case["far_s"], np.float32)
    rep.check(same_bits(o["beta_plus"][a], beta_plus0(far, case["denom"])), "initial beta+")
    rep.check(same_bits(o["d_fine"][a], np.full((a.size, case["n_final"]), SENT)), "d_fine written for an active ray")
    rep.check(same_bits(o["beta_map"][a], np.full(a.size, SENT)) and same_bits(o["iter_usage"][a], np.full(a.size, SENT)),
              "beta_map / iter_usage written for an active ray")
    return rep.finish()


def upsample_cases(R=32, n_up=512):
    G = g6()
    rng = np.random.default_rng(190)
    # the G6 rows through beta+ with clamp_bounds = 1: the per-ray beta, and the NaN -> inf rows whose inf bounds clamp to 1e5
    cases = [_upsample_case("upsample G6 per-ray beta+ clamp=1", G["G6_d"], G["G6_s"], 42, n_up, G["G6_beta_ray"][:, 0], 1, act_subset(8, rng)),
             _upsample_case("upsample G6 NaN->inf clamp=1", G["G6_nan_d"], G["G6_nan_s"], 40, n_up, np.full(8, G6_NAN_BETA, np.float32), 1,
                            act_subset(8, rng))]
    for i, n in enumerate(N_LIST):
        for clamp in (0, 1):
            rng = np.random.default_rng(200 + 2 * i + clamp)
            d = depth_rows(n, R, rng, dup=(i % 3 == 2 and n <= 66))
            # uniform-like pdf rows (far: all bounds exactly 0; zero; inside) only where the summation model's knot error is small
            # against the knot spacing 1 / n: beyond, the shared u table lands near a knot of them too often (fix the inputs, not the bound)
            pool = ["cross", "far", "cross", "gap", "zero", "inside"] if n <= 513 else ["cross", "gap"]   # n = 514: knots k / 513 = u_up
            s = sdf_rows(d, kinds_for(R, pool), rng)
            bp = pick_beta_plus(d, s, clamp, rng, n_up)
            cases.append(_upsample_case(f"upsample n={n} clamp={clamp}", d, s, n + 1 + i % 7, n_up, bp, clamp, act_subset(R, rng)))
    return cases


def _row_widened(d, s, bp, clamp, n_up):
    """The widened-path fraction the reference gives one row of k_upsample (it depends on the inputs alone)."""
    bp = np.float32(bp)
    B = bounds(d[None], s[None], np.float32(1) / bp, bp, clamp=bool(clamp))
    if not (np.isfinite(B["b"]).all() and np.isfinite(B["db"]).all()):
        return 2.0
    cdf, du = pdf_cdf(B["b"], B["db"])
    return icdf_bounds(d[None], cdf, torch_lin(n_up + 2)[None, 1:n_up + 1], du)[2].mean()


def pick_beta_plus(d, s, clamp, rng, n_up, limit=0.004):
    """beta+ per row, log-uniform in [0.0012, 0.45], moved until the row's widened-path fraction is at most `limit` (fixing the inputs, not
    the bound: a row whose bounds are all far below the 1e-5 floor, or tiny but not exactly 0, has an fp32 pdf the model cannot pin down).
    Round 1 (clamp_bounds = 0) of a row whose unclamped bounds contain inf is out of scope - the fp32 reference itself returns NaN there
    (inf / inf in the pdf) and real inputs cannot reach it (beta+_0 ~ 0.43) - so such a row counts as unusable too."""
    bp = np.empty(d.shape[0], np.float32)
    for r in range(d.shape[0]):
        b0 = np.exp(rng.uniform(np.log(0.0012), np.log(0.45)))
        grid = np.exp(np.linspace(np.log(0.0004), np.log(0.45), 28))
        best = (3.0, b0)
        for b in [b0] + sorted(grid, key=lambda g: abs(np.log(g / b0))):
            best = min(best, (_row_widened(d[r], s[r], b, clamp, n_up), b))
            if best[0] <= limit:
                break
        if best[0] > 1.0:
            raise RuntimeError(f"no usable beta+ for row {r}")
        bp[r] = best[1]
    return bp


def _upsample_case(name, d, s, cap, n_up, bp, clamp, act):
    R, n = d.shape
    return dict(stage="upsample", name=name, n_rays=R, n=n, cap=cap, n_up=n_up, dA=padded(d, cap), sA=padded(s, cap), act=act,
                beta_plus=bp.astype(np.float32), u_up=torch_lin(n_up + 2), clamp=clamp,
                out=dict(d_new=np.full((R, n_up), SENT, np.float32)))


def check_upsample(case, o):
    rep = Report(case["name"])
    n, act, k = case["n"], case["act"], len(case["act"])
    d, s = case["dA"][act, :n], case["sA"][act, :n]
    bp = case["beta_plus"][act]
    alpha = (np.float32(1) / bp).astype(np.float32)
    B = bounds(d, s, alpha, bp, clamp=bool(case["clamp"]))
    cdf, du = pdf_cdf(B["b"], B["db"])
    u = np.broadcast_to(case["u_up"][1:case["n_up"] + 1], (k, case["n_up"]))
    lo, hi, wid = icdf_bounds(d, cdf, u, du)
    rep.rays = k
    rep.samples_in(o["d_new"][:k], lo, hi, wid, "d_new", sorted_rows=True)
    rep.check(np.all(np.diff(o["d_new"][:k], axis=-1) >= 0), "d_new rows not sorted")
    rep.check(same_bits(o["d_new"][k:], np.full_like(o["d_new"][k:], SENT)), "d_new written past n_active")
    return rep.finish()


def finalize_cases(R=40):
    cases = []
    for i, n in enumerate(N_LIST):
        rng = np.random.default_rng(300 + i)
        n_final = N_FINAL[(i + 1) % 4]
        d = depth_rows(n, R, rng)
        s = sdf_rows(d, kinds_for(R, ["cross", "gap", "far", "inside", "zero"]), rng)
        bp = np.exp(rng.uniform(np.log(0.005), np.log(0.45), R)).astype(np.float32)
        per_ray = i % 2 == 0 and n < 2048
        u = u_rows(R, n_final, rng, fp32_opacity_knots(d, s, np.float32(1) / bp, bp)) if per_ray else torch_lin(n_final)
        cap = n + 2 + i % 3
        cases.append(dict(stage="finalize", name=f"finalize n={n} nf={n_final}{' perturb' if per_ray else ''}", n_rays=R, n=n, cap=cap,
                          n_final=n_final, dA=padded(d, cap), sA=padded(s, cap), act=act_subset(R, rng), u_final=np.ascontiguousarray(u, np.float32),
                          u_stride=n_final if per_ray else 0, beta_plus=bp,
                          out=dict(d_fine=np.full((R, n_final), SENT, np.float32), beta_map=np.full(R, SENT, np.float32),
                                   iter_usage=np.full(R, SENT, np.float32))))
    return cases


def check_finalize(case, o):
    rep = Report(case["name"])
    n, act = case["n"], case["act"]
    bp = case["beta_plus"][act]
    _opacity_check(rep, "d_fine", case["dA"][act, :n], case["sA"][act, :n], (np.float32(1) / bp).astype(np.float32), bp, _u_of(case, act),
                   o["d_fine"][act])
    rep.rays = len(act)
    rep.check(np.all(o["iter_usage"][act] == -1.0), "iter_usage of a finalized ray is not -1")
    rep.check(same_bits(o["beta_map"][act], bp), "beta_map is not the ray's beta+")
    rest = np.setdiff1d(np.arange(case["n_rays"]), act)
    rep.check(same_bits(o["d_fine"][rest], np.full((rest.size, case["n_final"]), SENT)) and same_bits(o["beta_map"][rest], np.full(rest.size, SENT))
              and same_bits(o["iter_usage"][rest], np.full(rest.size, SENT)), "a ray not in act was written")
    return rep.finish()


def merge_check_cases(R=32, n_up=512):
    G = g6()
    bp = G["G6_beta_ray"][:, 0]
    cases = [_merge_check_case("merge_check G6 scalar, per-ray beta+", 40, 24, 8, np.random.default_rng(390), 64, EPS, None, False, 2,
                               old=(G["G6_d"], G["G6_s"], bp), alpha=G6_ALPHA, beta=G6_BETA),
             _merge_check_case("merge_check G6 NaN->inf", 40, 24, 8, np.random.default_rng(391), 65, EPS, None, False, 4,
                               old=(G["G6_nan_d"], G["G6_nan_s"], np.maximum(bp, np.float32(2e-4))), alpha=G6_NAN_ALPHA, beta=G6_NAN_BETA)]
    for i, n in enumerate(N_LIST):
        rng = np.random.default_rng(400 + i)
        cases.append(_merge_check_case(f"merge_check n={n}+{n_up} nf={N_FINAL[(i + 2) % 4]}", n, n_up, R, rng, N_FINAL[(i + 2) % 4], EPS,
                                       ["cross", "gap", "far", "cross", "zero", "inside"], per_ray=i % 2 == 0, it=1 + i % 5))
    # eps = 0 with beta+ below beta_net: bisection steps whose max bound is EXACTLY 0 in fp32 (every E term underflows), where m <= eps
    # and m < eps part ways
    rng = np.random.default_rng(499)
    cases.append(_merge_check_case("merge_check eps=0 exact-zero bisection", 512, n_up, R, rng, 64, 0.0, ["const"], per_ray=False, it=3,
                                   beta_hi=1e-4))
    return cases


def _merge_check_case(name, n, n_up, R, rng, n_final, eps, pool, per_ray, it, beta_hi=None, old=None, alpha=ALPHA_NET, beta=BETA_NET):
    """old = (d_old, s_old, bp): given rows and beta+ (the G6 rows) instead of generated ones; their new samples get random sdf values."""
    cap = n + n_up + 3
    d_old = depth_rows(n, R, rng) if old is None else old[0]
    lo, hi = (NEAR, FAR) if old is None else (d_old[:, :1], d_old[:, -1:])
    d_new = np.sort(rng.uniform(lo, hi, (R, n_up)).astype(np.float32), -1)
    k = max(1, min(n, n_up) // 8)
    d_new[:, :k] = d_old[:, rng.choice(n, k)]                   # tied depths: old and new samples at the same depth
    d_new = np.sort(d_new, -1)
    d_cat = np.concatenate([d_old, d_new], -1)
    if old is not None:
        s_cat = np.concatenate([old[1], (rng.standard_normal((R, n_up)) * 0.5).astype(np.float32)], -1)
    elif pool == ["const"]:
        s_cat = np.broadcast_to(rng.uniform(0.12, 0.14, (R, 1)), d_cat.shape).astype(np.float32).copy()
    else:
        s_cat = sdf_rows(d_cat, kinds_for(R, pool), rng)
    s_old, s_new = s_cat[:, :n], s_cat[:, n:].copy()
    tied = np.isin(d_new, d_old)
    s_new[tied] += np.float32(0.01)                            # ... with different sdf values, so the merge order shows
    act = act_subset(R, rng)
    if old is not None:
        bp = np.asarray(old[2], np.float32).copy()
    else:
        bp = np.exp(rng.uniform(np.log(0.02), np.log(0.45), R)).astype(np.float32) if beta_hi is None else np.full(R, beta_hi, np.float32)
    slot_rows = lambda x: np.ascontiguousarray(x[act])
    if per_ray:
        d_m, s_m = stable_merge(d_old, s_old, d_new, s_new)
        u = u_rows(R, n_final, rng, fp32_opacity_knots(d_m, s_m, alpha, beta))
    else:
        u = torch_lin(n_final)
    return dict(stage="merge_check", name=name, n_rays=R, n=n, cap=cap, n_up=n_up, n_final=n_final, max_bisect=10, it=it, eps=np.float32(eps),
                alpha_net=np.float32(alpha), beta_net=np.float32(beta), dA=padded(d_old, cap), sA=padded(s_old, cap), act=act,
                d_new=slot_rows(d_new), s_new=slot_rows(s_new), u_final=np.ascontiguousarray(u, np.float32), u_stride=n_final if per_ray else 0,
                out=dict(dB=np.full((R, cap), np.nan, np.float32), sB=np.full((R, cap), np.nan, np.float32),
                         d_fine=np.full((R, n_final), SENT, np.float32), beta_plus=bp, beta_map=np.full(R, SENT, np.float32),
                         iter_usage=np.full(R, SENT, np.float32), act_out=np.full(R, ISENT, np.int32), act_count=np.zeros(1, np.int32)))


def check_merge_check(case, o):
    rep = Report(case["name"])
    R, n, nu, act = case["n_rays"], case["n"], case["n_up"], case["act"]
    nm = n + nu
    d_m, s_m = stable_merge(case["dA"][act, :n], case["sA"][act, :n], case["d_new"], case["s_new"])
    rep.check(same_bits(o["dB"][act, :nm], d_m), "merged depth rows (dB) differ")
    rep.check(same_bits(o["sB"][act, :nm], s_m), "merged sdf rows (sB) differ: not a stable merge")
    rest = np.setdiff1d(np.arange(R), act)
    rep.check(same_bits(o["dB"][:, nm:], np.full((R, case["cap"] - nm), np.nan)) and same_bits(o["dB"][rest], np.full((rest.size, case["cap"]), np.nan))
              and same_bits(o["sB"][rest], np.full((rest.size, case["cap"]), np.nan)), "dB / sB written past a row or for a ray not in act")
    lo, hi, _ = max_bound_range(d_m, s_m, case["alpha_net"], case["beta_net"])
    dec = decide(lo, hi, case["eps"])
    conv = o["iter_usage"][act] == float(case["it"])
    cnt = int(o["act_count"][0])
    listed = o["act_out"][:max(0, min(cnt, R))]
    rep.check(0 <= cnt <= len(act) and np.all(o["act_out"][cnt:] == ISENT), f"act_count {cnt} / act_out past it")
    rep.check(len(set(listed.tolist())) == len(listed) and set(listed.tolist()) <= set(act.tolist()), "act_out is not a subset of act")
    active = np.isin(act, listed)
    rep.check(np.all(conv ^ active), "a ray neither converged nor re-queued, or both")
    rep.check(np.all(np.where(dec > 0, active, True)) and np.all(np.where(dec < 0, conv, True)), "convergence decision outside the band")
    c = np.nonzero(conv)[0]
    if c.size:
        _opacity_check(rep, "d_fine", d_m[c], s_m[c], case["alpha_net"], case["beta_net"], _u_of(case, act[c]), o["d_fine"][act[c]])
    rep.check(same_bits(o["beta_map"][act[c]], np.full(c.size, case["beta_net"])), "beta_map of converged rays")
    bp_in = case["out"]["beta_plus"]
    rep.check(same_bits(o["beta_plus"][act[c]], bp_in[act[c]]), "beta_plus written for a converged ray")
    band = set(np.nonzero(dec == 0)[0].tolist())
    for j in np.nonzero(active)[0]:
        outs, nb = bisect_outcomes(d_m[j], s_m[j], case["beta_net"], bp_in[act[j]], float(case["eps"]), case["max_bisect"])
        if nb:
            band.add(j)
        got = np.float32(o["beta_plus"][act[j]]).item()
        rep.check(got in outs, f"bisected beta+ of ray {act[j]}: {got!r} not among the {len(outs)} outcome(s) {sorted(outs)[:4]}")
    a = act[active]
    rep.check(same_bits(o["d_fine"][a], np.full((a.size, case["n_final"]), SENT)) and same_bits(o["beta_map"][a], np.full(a.size, SENT))
              and same_bits(o["iter_usage"][a], np.full(a.size, SENT)), "d_fine / beta_map / iter_usage written for a re-queued ray")
    rep.check(same_bits(o["d_fine"][rest], np.full((rest.size, case["n_final"]), SENT)) and same_bits(o["beta_plus"][rest], bp_in[rest]),
              "a ray not in act was written")
    rep.rays, rep.band = len(act), len(band)
    return rep.finish()



# ==== NeuS: the weight rows of k_neus_upsample<false / true> (neus.py:36-63, :279-296) and near_far_from_sphere ==============================
# Model: sigmoid(z) = 1 / (1 + expf(-z)) carries 4 u relative plus p (1 - p) |dz|, where z = x inv_s and x itself was rounded (the slope
# estimate's pe / ne: mid, the clamped slope - 4 u relative - times the distance, the sum); alpha's numerator cancels, so pc and nc enter
# with their absolute errors over the +1e-5 (or +1e-10) of the denominator; T = cumprod(1 - alpha + 1e-10) carries the relative errors of its
# factors multiplicatively (1 - alpha loses the 1e-10 only where it is below u of it); w = alpha T.
from oracle import render as orender   # noqa: E402


def _sigmoid_err(x, dx, inv_s):
    z = x * inv_s
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-np.clip(z, -700, 700)))
    p = np.where(z < -EXP_INF_HI, 0.0, p)           # fp32 expf(-z) = inf: p = 0 exactly
    dp = p * (1 - p) * (np.abs(z) * U + inv_s * dx) + 4 * U * p + 2.0 ** -148
    return p, dp


def neus_weights(d, s, inv_s, direct):
    """The weight row k_neus_upsample<direct> inverts (before the + 1e-5 of sample_pdf) and its error -> (w, dw) [R, n-1]."""
    d = np.asarray(d, np.float64); s = np.asarray(s, np.float64)
    if direct:
        pc, dpc = _sigmoid_err(s[:, :-1], 0.0, inv_s)
        nc, dnc = _sigmoid_err(s[:, 1:], 0.0, inv_s)
        raw = (pc - nc) / (pc + 1e-10)
        a = np.maximum(raw, 0.0)
        assert np.allclose(a, orender.sdf_to_alpha(_t(s), inv_s)[1].numpy(), rtol=1e-9, atol=1e-12)
        da = (dpc + dnc + U * np.abs(pc - nc)) / (pc + 1e-10) + np.abs(raw) * (dpc + U * pc) / (pc + 1e-10) + 2 * U * np.abs(raw)
    else:
        ps, ns, pz, nz = s[:, :-1], s[:, 1:], d[:, :-1], d[:, 1:]
        mid = (ps + ns) * 0.5
        dot = (ns - ps) / (nz - pz + THR)
        prev = np.concatenate([np.zeros((s.shape[0], 1)), dot[:, :-1]], -1)
        dv = np.clip(np.minimum(prev, dot), -10.0, 0.0)
        dist = nz - pz
        pe, ne = mid - dv * dist * 0.5, mid + dv * dist * 0.5
        dx = SAFETY * U * (np.abs(mid) + 4 * np.abs(dv) * dist + np.maximum(np.abs(pe), np.abs(ne)))
        pc, dpc = _sigmoid_err(pe, dx, inv_s)
        nc, dnc = _sigmoid_err(ne, dx, inv_s)
        a = (pc - nc + THR) / (pc + THR)
        da = (dpc + dnc + U * (np.abs(pc - nc) + THR)) / (pc + THR) + a * (dpc + U * pc) / (pc + THR) + 2 * U * a
    f = 1.0 - a + 1e-10
    df = da + 2 * U * f
    T = torch.cumprod(torch.cat([torch.ones(a.shape[0], 1, dtype=torch.float64), _t(f)], -1), -1).numpy()[:, :-1]
    w = a * T
    assert np.allclose(w, orender.alpha_to_w(_t(a)).numpy(), rtol=1e-12, atol=0)
    # T's error from the products of the factors' lower and upper ends (a factor near 1e-10 may be off by a large ratio - T stays tiny there)
    # and the product chain's own roundings
    one = np.ones((a.shape[0], 1))
    T_hi = np.cumprod(np.concatenate([one, np.minimum(f + SAFETY * df, 1.0 + 1e-10)], -1), -1)[:, :-1]
    T_lo = np.cumprod(np.concatenate([one, np.maximum(f - SAFETY * df, 0.0)], -1), -1)[:, :-1]
    chain = SAFETY * (2 * seg_of(a.shape[1] + 1) + 8) * U
    dT = np.maximum(T_hi * (1 + chain) - T, T - T_lo * (1 - chain))
    dw = da * T + a * dT + 2 * U * w
    return w, dw


NEUS_N_NEW = [1, 5, 16, 63, 64, 128]
NEUS_INV_S = [64.0, 128.0, 256.0, 512.0, 4096.0]


def neus_upsample_cases(R=32):
    cases = []
    for direct in (False, True):
        for i, n in enumerate([2, 3, 40, 64, 65, 66, 128, 512, 513, 1025, 1538, 2048]):
            rng = np.random.default_rng(500 + 50 * direct + i)
            n_new = NEUS_N_NEW[i % len(NEUS_N_NEW)]
            # past ~1,000 bins a smooth (small inv_s) weight row spreads its mass over hundreds of intervals whose worst-case rounding the
            # model adds with one sign: there the sharp end of the range
            inv_s = NEUS_INV_S[i % len(NEUS_INV_S)] if n < 1500 else (4096.0 if i % 2 else 512.0)
            per_ray = i % 2 == 1
            d, s, u = neus_rows(n, R, rng, n_new, float(inv_s), direct, per_ray)
            cap = n + 1 + i % 4
            cases.append(dict(stage="neus_upsample", name=f"neus_{'direct_' if direct else ''}upsample n={n} n_new={n_new} inv_s={inv_s:g}"
                              + (" perturb" if per_ray else ""), direct=direct, n_rays=R, n=n, cap=cap, n_new=n_new, inv_s=np.float32(inv_s),
                              dA=padded(d, cap), sA=padded(s, cap), u_new=np.ascontiguousarray(u, np.float32), u_stride=n_new if per_ray else 0,
                              out=dict(d_new=np.full((R + 1, n_new), SENT, np.float32))))
    return cases


def neus_rows(n, R, rng, n_new, inv_s, direct, per_ray, limit=0.004):
    """R rays of sdf rows (crossings of random steepness, empty space in front of one, the origin inside) and their u rows, each row kept
    only if the reference puts at most `limit` of its samples (plus the one 1 - 2^-24 of a perturbed row) on the widened path.  The
    first-order model adds every fp32 rounding of a smooth, many-interval weight row with the same sign; rows it cannot pin down are redrawn
    (fixing the inputs, not the bound).  The per-ray u rows hold exactly 0 everywhere and, from 63 samples up, 1 - 2^-24 on every fifth ray."""
    d_out, s_out, u_out = [], [], []
    kinds = ["cross", "gap", "inside", "cross"]
    for tries in range(60 * R):
        r = len(d_out)
        if r == R:
            break
        if tries >= 30 * R:
            limit = 0.03                                  # rows this hard to pin down: admit a few more widened samples
        d = depth_rows(n, 1 + (r % 2), rng)[-1:]
        s = sdf_rows(d, [kinds[tries % 4]], rng) * np.float32(rng.uniform(0.1, 1.0))
        s = np.clip(s, -1, 1).astype(np.float32)
        if per_ray:
            u = rng.uniform(0, 1, (1, n_new)).astype(np.float32)
            u[0, rng.integers(n_new)] = 0.0
            if n_new >= 63 and r % 5 == 0:
                u[0, rng.integers(n_new)] = np.float32(1 - 2.0 ** -24)
        else:
            u = torch_lin(n_new)[None]
        w, dw = neus_weights(d, s, inv_s, direct)
        cdf, du = pdf_cdf(w, dw)
        if icdf_bounds(d, cdf, u, du)[2].sum() <= limit * n_new + (1 if per_ray and n_new >= 63 else 0):
            d_out.append(d[0]); s_out.append(s[0]); u_out.append(u[0])
    else:
        raise RuntimeError("not enough usable NeuS rows")
    return np.stack(d_out), np.stack(s_out), (np.stack(u_out) if per_ray else torch_lin(n_new))


def check_neus_upsample(case, o):
    rep = Report(case["name"])
    R, n = case["n_rays"], case["n"]
    d, s = case["dA"][:, :n], case["sA"][:, :n]
    w, dw = neus_weights(d, s, float(case["inv_s"]), case["direct"])
    cdf, du = pdf_cdf(w, dw)
    u = case["u_new"] if case["u_stride"] else np.broadcast_to(case["u_new"], (R, case["n_new"]))
    lo, hi, wid = icdf_bounds(d, cdf, u, du)
    rep.rays = R
    rep.samples_in(o["d_new"][:R], lo, hi, wid, "d_new", sorted_rows=True)
    rep.check(np.all(np.diff(o["d_new"][:R], axis=-1) >= 0), "d_new rows not sorted")
    rep.check(same_bits(o["d_new"][R:], np.full((1, case["n_new"]), SENT)), "d_new written past the rays")
    return rep.finish()


def near_far(o, dn, r):
    """near_far_from_sphere (rend_util.py:168-186) in fp64 -> (near, far, tolerance, near surely clamped to 0, far surely clamped to r)."""
    o = np.asarray(o, np.float64); dn = np.asarray(dn, np.float64)
    near, far = orender.near_far_from_sphere(_t(o), _t(dn), r)
    mid = -(o * dn).sum(-1)
    tol = SAFETY * (3 * U * np.abs(o * dn).sum(-1) + U * (np.abs(mid) + r)) + ulp32(np.abs(mid) + r)
    return near.numpy()[:, 0], far.numpy()[:, 0], tol, mid - r < -tol, mid < -tol
