"""References, case builders and checkers of the surface renderer's per-ray stages and of ray generation.

The stages are k_first_crossing, k_secant_update, k_root_finish and k_sphere_step of csrc/ray_casting.hip (reference models/ray_casting.py),
k_get_rays of csrc/raygen.hip (utils/rend_util.py: lift :95-109, get_rays :112-165) and k_normalize_dirs of csrc/volsdf_render.hip
(F.normalize).  They take the SDF values as an input, so no network is needed.  tests/test_raycast_ref.py shows on the CPU that the checkers
accept an independently written float32 stand-in and refuse stand-ins with the bugs these kernels invite; tests/test_gpu_raycast_stages.py
holds the HIP kernels to them.

THE EXACT RULE.  Every decision of these stages is one correctly rounded fp32 operation on the inputs: a = val - tau, one product
a_i a_{i+1}, one compare.  The NumPy float32 restatement below therefore predicts masks, indices and brackets BIT FOR BIT, with no decision
band, as long as the products stay normal fp32 numbers: the case builders keep |val - tau| in [2^-60, 2^10] or exactly 0 and assert it.
  first crossing   the first i with a_i a_{i+1} < 0 (a product with an exact 0 is no sign change: ray_casting.py:93-100, sign(0) = 0);
                   bracket = (d_low, f_low, d_high, f_high) = (depth_{i+1}, a_{i+1}, depth_i, a_i); mask_sign_change = there is one;
                   mask_start_outside = a_0 > 0 (strictly); mask = both and f_high > 0 (the crossing goes outside -> inside).
  secant update    f_mid = raw - tau; f_mid < 0 replaces the low side, anything else (+0, -0 included) the high side (ray_casting.py:11-30).
  root finish      d_out = d_pred (hit) / inf (fill_inf) / far; 0 where the ray starts inside; pt = 1 where nothing is hit (:137-152).
  sphere step      d[mask] += sdf[mask]; mask[d > far] = False; mask[d < 0] = False (:175-180): a single fp32 add, bit-exact.
Only the secant estimate, the hit point, the ray directions and the normalised directions carry rounding bounds; each is derived from the
operation count of the kernel's own expression next to the check that uses it (first order in u = 2^-24, times SAFETY).

Every output buffer is one ray longer than the case; the extra row must keep its sentinel (SENT for floats, 0x5a for bytes).
"""
import numpy as np

import stage_ref as S
from stage_ref import Report, SAFETY, SENT, U, bits, same_bits

USENT = np.uint8(0x5a)
NAN_BITS = np.uint32(0x7fc00123)            # the state of rays a stage must not touch is filled with this NaN and compared by bits
MAG_LO, MAG_HI = 2.0 ** -60, 2.0 ** 10


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def nan_fill(shape):
    return np.full(shape, NAN_BITS, np.uint32).view(np.float32)


def fsent(shape):
    return np.full(shape, SENT, np.float32)


def usent(shape):
    return np.full(shape, USENT, np.uint8)


def _same_bytes(a, b):
    return np.array_equal(np.asarray(a, np.uint8), np.asarray(b, np.uint8))


def _inputs_unchanged(rep, case, o, keys):
    for k in keys:
        if k in o and case.get(k) is not None:
            rep.check(np.array_equal(np.ascontiguousarray(o[k]).view(np.uint8), np.ascontiguousarray(case[k]).view(np.uint8)), f"input {k} changed")


# ==== the exact rule ==========================================================================================================================
def rule_first_crossing(val, depth, tau):
    """-> mask, sign_change, start_outside (bool [R]), bracket [R, 4] fp32 (meaningful where sign_change), first index [R]."""
    val, depth = f32(val), f32(depth)
    R = val.shape[0]
    with np.errstate(all="ignore"):
        a = val - np.float32(tau)
        neg = (a[:, :-1] * a[:, 1:]) < 0
    sc = neg.any(-1)
    i = np.where(sc, neg.argmax(-1), 0)
    rows = np.arange(R)
    brk = np.stack([depth[rows, i + 1], a[rows, i + 1], depth[rows, i], a[rows, i]], -1).astype(np.float32)
    m0 = a[:, 0] > 0
    return sc & (brk[:, 3] > 0) & m0, sc, m0, brk, i


def rule_secant(f_mid_raw, tau, brk, d_pred):
    """One bracket update of every ray (the caller applies it to the masked ones)."""
    f_mid = f32(f_mid_raw) - np.float32(tau)
    low = f_mid < 0
    out = f32(brk).copy()
    out[:, 0] = np.where(low, d_pred, brk[:, 0]); out[:, 1] = np.where(low, f_mid, brk[:, 1])
    out[:, 2] = np.where(low, brk[:, 2], d_pred); out[:, 3] = np.where(low, brk[:, 3], f_mid)
    return out


def secant64(brk):
    """fp64 value of -f_low (d_high - d_low) / (f_high - f_low) + d_low on the fp32 bracket, and the bound of the kernel's fp32 estimate.
    The kernel rounds four times inside term = -f_low (d_high - d_low) / (f_high - f_low) - the difference of the depths, the product, the
    difference f_high - f_low (the sum of two same-signed magnitudes, as f_low < 0 <= f_high: no cancellation) and the quotient, each
    relative to its own result - so term carries at most 4 |term| u; the final sum rounds once more, at most |d_pred| u.  The |d_low| u on
    top is slack the count does not need (the negation is exact); it is kept as the stated bound.  A quotient followed by an add cannot be
    contracted, so the count holds for any compiler.  All of it times SAFETY for the second-order terms."""
    b = np.asarray(brk, np.float64)
    with np.errstate(all="ignore"):
        term = -b[:, 1] * (b[:, 2] - b[:, 0]) / (b[:, 3] - b[:, 1])
        dp = term + b[:, 0]
    return dp, SAFETY * (4 * np.abs(term) + np.abs(b[:, 0]) + np.abs(dp)) * U


def rule_sphere_step(sdf, far, d, mask):
    d, m = f32(d).copy(), np.asarray(mask).astype(bool)
    with np.errstate(all="ignore"):
        d[m] = d[m] + f32(sdf)[m]
        m = m & ~(d > far) & ~(d < 0)
    return d, m


# ==== first_crossing ==========================================================================================================================
FC_R = [1, 3, 4, 5, 259]
FC_N = [2, 3, 63, 64, 65, 128, 129, 256, 300]
FC_TAU = [0.0, 0.02]
FC_KINDS = ["a", "b", "c+", "c-", "d", "d2", "e", "e2", "f", "g", "h"]


def _pattern(kind, N, p, tau):
    """Signs (+1 / 0 / -1) of val - tau along one row of kind `kind` with its deciding index at p (clipped to what N allows), and the
    expected (mask, sign_change, start_outside, first index or None)."""
    p = int(min(max(p, 0), N - 2))
    s = np.ones(N, np.int8)
    if kind == "g" and tau == 0.0:
        kind = "a"                                   # no value lies strictly between 0 and tau = 0
    if kind in ("a", "g", "h"):                      # one outside -> inside crossing (h: the only one, at (N - 2, N - 1))
        p = N - 2 if kind == "h" else p
        s[p + 1:] = -1
        return s, (1, 1, 1, p), kind
    if kind == "b":                                  # starts inside: inside -> outside at p, outside -> inside two steps later
        s[:p + 1] = -1
        s[p + 3:] = -1
        return s, (0, 1, 0, p), kind
    if kind in ("c+", "c-"):
        return (s if kind == "c+" else -s), (0, 0, int(kind == "c+"), None), kind
    if kind in ("d", "d2"):                          # several crossings in different lanes and 64-strides: the first must win
        flips = [p, p + 2, p + 65] if kind == "d" else [p, p + 63, p + 64, p + 129]
        for f in flips:
            if f <= N - 2:
                s[f + 1:] *= -1
        return s, (1, 1, 1, p), kind
    if kind == "e":                                  # +, 0, - only: no sign change
        if N < 3:
            return s, (0, 0, 1, None), "c+"
        p = min(p, N - 3)
        s[p + 1] = 0
        s[p + 2:] = -1
        return s, (0, 0, 1, None), kind
    if kind == "e2":                                 # +, 0, -, -, +, -: the first sign change is the inside -> outside one
        if N < 7:
            return _pattern("e", N, p, tau)
        p = min(p, N - 7)
        s[p + 1] = 0
        s[p + 2:] = -1
        s[p + 4] = 1
        return s, (0, 1, 1, p + 3), kind
    if kind == "f":                                  # val[0] - tau == 0 exactly: the ray does not start outside
        if N < 3:
            s[0], s[1] = 0, -1
            return s, (0, 0, 0, None), kind
        p = max(p, 1)
        s[0] = 0
        s[p + 1:] = -1
        return s, (0, 1, 0, p), kind
    raise ValueError(kind)


def first_crossing_rows(R, N, tau, rng, offset=0):
    """val, depth [R, N] and the per-row expectation of the construction (kind, mask, sign_change, start_outside, index)."""
    tau32 = np.float32(tau)
    pos = sorted({q for q in (0, 62, 63, 64, 65, N - 2) if 0 <= q <= N - 2})
    val, signs = np.empty((R, N), np.float32), np.empty((R, N), np.int8)
    expect = []
    for r in range(R):
        k = r + offset
        kind = FC_KINDS[k % len(FC_KINDS)]
        s, exp, kind = _pattern(kind, N, pos[(k // len(FC_KINDS)) % len(pos)], tau)
        # magnitudes: the whole admitted range at tau = 0; at tau != 0 far enough above the spacing of fp32 around tau that the sign survives
        wide = tau == 0.0 and r % 3 == 0
        mag = 2.0 ** (rng.uniform(-60, 10, N) if wide else rng.uniform(-20, 3, N))
        v = float(tau32) + s * mag
        if kind == "g":                              # 0 < val < tau behind the crossing: only the subtraction of tau makes it negative
            behind = s < 0
            v[behind] = float(tau32) * rng.uniform(0.1, 0.9, int(behind.sum()))
        val[r] = v.astype(np.float32)
        val[r, s == 0] = tau32
        signs[r] = s
        expect.append((kind,) + exp)
    # per-ray depth rows: distinct near / far, increasing, not uniform
    near = (0.05 + 0.013 * np.arange(R) % 1.7)[:, None]
    far = (4.0 + 0.021 * np.arange(R) % 2.3)[:, None]
    t = np.cumsum(rng.uniform(0.5, 1.5, (R, N)), -1)
    t = (t - t[:, :1]) / (t[:, -1:] - t[:, :1])
    depth = (near + (far - near) * t).astype(np.float32)
    assert np.all(np.diff(depth, axis=-1) > 0)
    a = val - tau32
    assert np.array_equal(np.sign(a).astype(np.int8), signs), "a sign of val - tau did not survive the rounding"
    mags = np.abs(a[a != 0])
    assert mags.size == 0 or (mags.min() >= MAG_LO and mags.max() <= MAG_HI), "val - tau outside [2^-60, 2^10]"
    return val, depth, expect


def first_crossing_case(name, val, depth, tau, expect=None):
    R, N = val.shape
    return dict(stage="first_crossing", name=name, n_rays=R, n=N, tau=np.float32(tau), val=f32(val), depth=f32(depth), expect=expect,
                out=dict(mask=usent(R + 1), mask_sc=usent(R + 1), mask0=usent(R + 1), bracket=fsent((R + 1, 4)), d_pred=fsent(R + 1)))


_FC_CASES = None


def first_crossing_cases():
    global _FC_CASES
    if _FC_CASES is None:
        _FC_CASES, k = [], 0
        for R in FC_R:
            for N in FC_N:
                for tau in FC_TAU:
                    rng = np.random.default_rng(1000 + k)
                    val, depth, expect = first_crossing_rows(R, N, tau, rng, offset=5 * k)
                    _FC_CASES.append(first_crossing_case(f"first_crossing R={R} N={N} tau={tau:g}", val, depth, tau, expect))
                    k += 1
    return _FC_CASES


def check_first_crossing(case, o):
    rep = Report(case["name"])
    R = case["n_rays"]
    rep.rays = R
    mask, sc, m0, brk, idx = rule_first_crossing(case["val"], case["depth"], case["tau"])
    if case.get("expect") is not None:               # the rule itself against what the rows were built to give
        for r, (kind, e_m, e_sc, e_m0, e_i) in enumerate(case["expect"]):
            assert (int(mask[r]), int(sc[r]), int(m0[r])) == (e_m, e_sc, e_m0) and (e_i is None or idx[r] == e_i), (case["name"], r, kind)
    rep.start_outside = m0
    for k, want in (("mask", mask), ("mask_sc", sc), ("mask0", m0)):
        rep.check(_same_bytes(o[k][:R], want.astype(np.uint8)), f"{k}: {int((np.asarray(o[k][:R]) != want.astype(np.uint8)).sum())} rays differ "
                  f"(first {np.flatnonzero(np.asarray(o[k][:R]) != want.astype(np.uint8))[:1]})")
        rep.check(o[k][R] == USENT, f"{k} written past the rays")
    rep.check(same_bits(o["bracket"][:R][sc], brk[sc]), "bracket differs where there is a sign change")
    rep.check(same_bits(o["bracket"][R], fsent(4)) and same_bits(o["d_pred"][R], SENT), "bracket / d_pred written past the rays")
    rep.check(same_bits(o["d_pred"][:R][~mask], np.ones(int((~mask).sum()), np.float32)), "d_pred is not 1.0f where mask is 0")
    ref, bound = secant64(brk[mask])
    err = np.abs(np.asarray(o["d_pred"][:R][mask], np.float64) - ref)
    rep.samples += int(mask.sum())
    rep.worst = float(np.max(err / bound, initial=0))
    rep.check(np.all(err <= bound), f"d_pred: worst error / bound {rep.worst:.3g}")
    _inputs_unchanged(rep, case, o, ("val", "depth"))
    return rep.finish()


# ==== secant_update ===========================================================================================================================
SEC_R = [1, 255, 256, 257, 1000]
F_MID_KINDS = ["neg", "pos", "zero", "negzero", "below_tau"]


def secant_case(name, f_mid, tau, mask, brk, d_pred):
    """brk [R, 4], d_pred [R]: the state the update starts from (rows of unmasked rays may hold anything; they must keep their bits)."""
    R = len(f_mid)
    b, d = fsent((R + 1, 4)), fsent(R + 1)
    b[:R], d[:R] = brk, d_pred
    return dict(stage="secant_update", name=name, n_rays=R, tau=np.float32(tau), f_mid=f32(f_mid), mask=np.ascontiguousarray(mask, np.uint8),
                out=dict(bracket=b, d_pred=d))


def _f_mid_rows(R, tau, rng):
    """raw f_mid with (raw - tau) negative, positive, exactly +0, -0.0 (tau = 0 only: -0.0 - 0 = -0.0) and 0 < raw < tau (tau != 0)."""
    tau32 = np.float32(tau)
    raw = np.empty(R, np.float32)
    for r in range(R):
        kind = F_MID_KINDS[r % len(F_MID_KINDS)]
        mag = 2.0 ** rng.uniform(-20, 0)
        if kind == "neg":
            raw[r] = tau32 - np.float32(mag)
        elif kind == "pos":
            raw[r] = tau32 + np.float32(mag)
        elif kind == "zero" or (kind == "negzero" and tau != 0.0):
            raw[r] = tau32
        elif kind == "negzero":
            raw[r] = np.float32(-0.0)
        else:
            raw[r] = tau32 * np.float32(rng.uniform(0.1, 0.9)) if tau != 0.0 else np.float32(-mag)
    return raw


def secant_cases():
    cases = []
    for k, R in enumerate(SEC_R):
        for tau in FC_TAU:
            rng = np.random.default_rng(2000 + 2 * k + int(tau != 0))
            if k % 2 == 0:                           # state out of the first-crossing rule
                val, depth, _ = first_crossing_rows(R, 65, tau, rng, offset=k)
                mask, _, _, brk, _ = rule_first_crossing(val, depth, tau)
                src = "first_crossing state"
            else:                                    # synthetic brackets: d_low > d_high (low = the inside end), f_low < 0 <= f_high
                mask = rng.uniform(size=R) < 0.7
                d_high = rng.uniform(0.1, 3.0, R)
                brk = np.stack([d_high + 2.0 ** rng.uniform(-12, 0, R), -2.0 ** rng.uniform(-20, 0, R), d_high, 2.0 ** rng.uniform(-20, 0, R)],
                               -1).astype(np.float32)
                brk[::7, 3] = 0.0                    # f_high exactly 0: the state an earlier f_mid == 0 leaves behind
                src = "synthetic state"
            if R > 1:
                mask[R - 1] = False                  # the last ray unmasked: its state must survive next to the sentinel row
            with np.errstate(all="ignore"):
                d_pred = (-brk[:, 1] * (brk[:, 2] - brk[:, 0]) / (brk[:, 3] - brk[:, 1]) + brk[:, 0]).astype(np.float32)
            brk, d_pred = brk.copy(), d_pred.copy()
            brk[~mask], d_pred[~mask] = nan_fill((int((~mask).sum()), 4)), nan_fill(int((~mask).sum()))
            cases.append(secant_case(f"secant_update R={R} tau={tau:g} {src}", _f_mid_rows(R, tau, rng), tau, mask, brk, d_pred))
    return cases


def check_secant(case, o):
    rep = Report(case["name"])
    R = case["n_rays"]
    m = case["mask"].astype(bool)
    rep.rays = int(m.sum())
    b0, d0 = case["out"]["bracket"], case["out"]["d_pred"]
    want = rule_secant(case["f_mid"], case["tau"], b0[:R], d0[:R])
    rep.check(same_bits(o["bracket"][:R][m], want[m]), "bracket of a masked ray differs from the rule")
    ref, bound = secant64(want[m])
    err = np.abs(np.asarray(o["d_pred"][:R][m], np.float64) - ref)
    rep.samples += int(m.sum())
    rep.worst = float(np.max(err / bound, initial=0))
    rep.check(np.all(err <= bound), f"d_pred: worst error / bound {rep.worst:.3g}")
    rep.check(same_bits(o["bracket"][:R][~m], b0[:R][~m]) and same_bits(o["d_pred"][:R][~m], d0[:R][~m]), "an unmasked ray was written")
    rep.check(same_bits(o["bracket"][R], b0[R]) and same_bits(o["d_pred"][R], d0[R]), "bracket / d_pred written past the rays")
    _inputs_unchanged(rep, case, o, ("f_mid", "mask"))
    return rep.finish()


# ==== root_finish =============================================================================================================================
RF_R = [1, 255, 256, 257]
RF_STATES = [(1, 1), (0, 1), (0, 0)]              # (mask, start_outside); (1, 0) cannot come out of first_crossing


def root_finish_case(name, rays_o, rays_dn, mask, mask0, d_pred, far, far_s, fill_inf):
    R = len(d_pred)
    return dict(stage="root_finish", name=name, n_rays=R, rays_o=f32(rays_o), rays_dn=f32(rays_dn), mask=np.ascontiguousarray(mask, np.uint8),
                mask0=np.ascontiguousarray(mask0, np.uint8), d_pred=f32(d_pred), far=None if far is None else f32(far), far_s=np.float32(far_s),
                fill_inf=int(fill_inf), out=dict(d_out=fsent(R + 1), pt=fsent((R + 1, 3))))


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def root_finish_cases():
    cases = []
    for k, R in enumerate(RF_R):
        for fill_inf in (0, 1):
            for per_ray in (True, False):
                rng = np.random.default_rng(3000 + 4 * k + 2 * fill_inf + per_ray)
                st = np.array([RF_STATES[(r + k) % 3] for r in range(R)], np.uint8)
                far = rng.uniform(4.0, 6.0, R).astype(np.float32) if per_ray else None
                cases.append(root_finish_case(f"root_finish R={R} fill_inf={fill_inf} far={'per-ray' if per_ray else 'scalar'}",
                                              rng.uniform(-3, 3, (R, 3)), _unit(rng.standard_normal((R, 3))), st[:, 0], st[:, 1],
                                              rng.uniform(0.3, 5.0, R), far, 5.25, fill_inf))
    return cases


def check_root_finish(case, o):
    rep = Report(case["name"])
    R = case["n_rays"]
    rep.rays = R
    m, m0 = case["mask"].astype(bool), case["mask0"].astype(bool)
    far = case["far"] if case["far"] is not None else np.full(R, case["far_s"], np.float32)
    want = np.where(m, case["d_pred"], np.float32(np.inf) if case["fill_inf"] else far).astype(np.float32)
    want[~m0] = 0.0
    rep.check(same_bits(o["d_out"][:R], want), "d_out differs from d_pred / inf / far / 0")
    rep.check(same_bits(o["pt"][:R][~m], np.ones((int((~m).sum()), 3), np.float32)), "pt is not 1.0f where mask is 0")
    # o + dn d: the product rounds once (|dn d| u), the sum once (at most (|o| + |dn d|) u); fused into one multiply-add it rounds once
    # only, which the same bound covers: (|o| + 2 |dn d|) u
    od, dn, d = case["rays_o"][m].astype(np.float64), case["rays_dn"][m].astype(np.float64), case["d_pred"][m].astype(np.float64)[:, None]
    err = np.abs(np.asarray(o["pt"][:R][m], np.float64) - (od + dn * d))
    bound = SAFETY * (np.abs(od) + 2 * np.abs(dn * d)) * U
    rep.samples += err.size
    rep.check(np.all(err <= bound), f"pt: worst error / bound {float(np.max(err / bound, initial=0)):.3g}")
    rep.check(same_bits(o["d_out"][R], SENT) and same_bits(o["pt"][R], fsent(3)), "d_out / pt written past the rays")
    _inputs_unchanged(rep, case, o, ("rays_o", "rays_dn", "mask", "mask0", "d_pred", "far"))
    return rep.finish()


# ==== sphere_trace_step =======================================================================================================================
ST_R = [1, 255, 256, 257]
ST_KINDS = ["to_far", "to_zero", "to_negzero", "ulp_over_far", "below_zero", "dead_over_far", "dead_below_zero_nan", "live_nan", "live",
            "dead_in_range"]


def sphere_step_case(name, sdf, far, far_s, d, mask):
    R = len(sdf)
    dd, mm = fsent(R + 1), usent(R + 1)
    dd[:R], mm[:R] = d, mask
    return dict(stage="sphere_step", name=name, n_rays=R, sdf=f32(sdf), far=None if far is None else f32(far), far_s=np.float32(far_s),
                out=dict(d=dd, mask=mm))


def sphere_step_cases():
    cases = []
    for k, R in enumerate(ST_R):
        for per_ray in (True, False):
            rng = np.random.default_rng(4000 + 2 * k + per_ray)
            far_s = np.float32(5.3)
            far = rng.uniform(3.0, 6.0, R).astype(np.float32) if per_ray else np.full(R, far_s, np.float32)
            d, sdf, mask = np.empty(R, np.float32), np.empty(R, np.float32), np.ones(R, np.uint8)
            for r in range(R):
                kind = ST_KINDS[(r + 3 * k + per_ray) % len(ST_KINDS)]
                half = far[r] * np.float32(0.5)                     # exact; far - half and nextafter(far) - half are exact too
                if kind == "to_far":
                    d[r], sdf[r] = half, far[r] - half
                elif kind == "to_zero":
                    d[r] = rng.uniform(0.1, 3.0); sdf[r] = -d[r]
                elif kind == "to_negzero":
                    d[r], sdf[r] = -0.0, -0.0
                elif kind == "ulp_over_far":
                    d[r], sdf[r] = half, np.nextafter(far[r], np.float32(np.inf)) - half
                elif kind == "below_zero":
                    d[r] = rng.uniform(0.1, 3.0); sdf[r] = -d[r] - np.float32(2.0 ** rng.uniform(-20, 0))
                elif kind == "dead_over_far":
                    d[r], sdf[r], mask[r] = far[r] + np.float32(rng.uniform(0.01, 1.0)), rng.uniform(-1, 1), 0
                elif kind == "dead_below_zero_nan":
                    d[r], sdf[r], mask[r] = -rng.uniform(0.01, 1.0), np.nan, 0
                elif kind == "live_nan":
                    d[r], sdf[r] = rng.uniform(0.1, 3.0), np.nan
                elif kind == "live":
                    d[r], sdf[r] = rng.uniform(0.1, 2.0), rng.uniform(-0.05, 0.9)
                else:
                    d[r], sdf[r], mask[r] = rng.uniform(0.1, 2.0), rng.uniform(0.1, 0.9), 0
            cases.append(sphere_step_case(f"sphere_trace_step R={R} far={'per-ray' if per_ray else 'scalar'}", sdf, far if per_ray else None, far_s,
                                          d, mask))
    return cases


def check_sphere_step(case, o):
    rep = Report(case["name"])
    R = case["n_rays"]
    rep.rays = R
    far = case["far"] if case["far"] is not None else np.full(R, case["far_s"], np.float32)
    d0, m0 = case["out"]["d"], case["out"]["mask"]
    d, m = rule_sphere_step(case["sdf"], far, d0[:R], m0[:R])
    nan = np.isnan(d)                                # a live ray's NaN sdf: d is NaN (its payload is the hardware's), the mask stays 1
    rep.check(np.all(np.isnan(np.asarray(o["d"][:R])[nan])), "d of a live ray with a NaN sdf is not NaN")
    rep.check(same_bits(np.asarray(o["d"][:R])[~nan], d[~nan]), f"d differs on {int((bits(np.asarray(o['d'][:R])[~nan]) != bits(d[~nan])).sum())} rays")
    rep.check(_same_bytes(o["mask"][:R], m.astype(np.uint8)), f"mask differs on rays {np.flatnonzero(np.asarray(o['mask'][:R]) != m.astype(np.uint8))[:4]}")
    rep.check(same_bits(o["d"][R], SENT) and o["mask"][R] == USENT, "d / mask written past the rays")
    _inputs_unchanged(rep, case, o, ("sdf", "far"))
    return rep.finish()


# ==== get_rays ================================================================================================================================
GR_SIZES = [(1, 1), (7, 5), (5, 7), (33, 65), (270, 480)]
GR_SELECT = ["all", "one", "257", "ends"]


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def get_rays_cases():
    cases = []
    for k, (H, W) in enumerate(GR_SIZES):
        for sel in GR_SELECT:
            for tmag in (1.0, 100.0):
                rng = np.random.default_rng(5000 + 8 * k + 2 * GR_SELECT.index(sel) + int(tmag > 1))
                m = float(max(H, W))
                K = np.eye(4, dtype=np.float32)
                K[0, 0], K[1, 1], K[0, 1], K[0, 2], K[1, 2] = 0.9 * m + 0.37, 1.1 * m + 0.21, 0.05 * m + 0.013, 0.5 * W + 0.3, 0.5 * H - 0.2
                pose = np.eye(4, dtype=np.float32)
                pose[:3, :3] = _rotation(rng)
                t = rng.standard_normal(3)
                pose[:3, 3] = tmag * t / np.linalg.norm(t)
                if sel == "all":
                    select = None
                elif sel == "one":
                    select = np.array([rng.integers(H * W)], np.int64)
                elif sel == "257":                   # unordered, with duplicates
                    select = rng.integers(0, H * W, 257).astype(np.int64)
                    select[5] = select[200]
                else:
                    select = np.array([H * W - 1, 0], np.int64)
                n = H * W if select is None else len(select)
                cases.append(dict(stage="get_rays", name=f"get_rays {H}x{W} select={sel} |t|={tmag:g}", H=H, W=W, K=K, pose=pose, select=select,
                                  n=n, out=dict(rays_o=fsent((n + 1, 3)), rays_d=fsent((n + 1, 3)))))
    return cases


def check_get_rays(case, o):
    rep = Report(case["name"])
    H, W, n = case["H"], case["W"], case["n"]
    rep.rays = n
    K, P = case["K"].astype(np.float64), case["pose"].astype(np.float64)
    pix = np.arange(n) if case["select"] is None else case["select"]
    i, j = (pix % W).astype(np.float64), (pix // W).astype(np.float64)
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    # x = (i - cx + cy sk / fy - sk j / fy) / fx, y = (j - cy) / fy, z = 1; d = (c2w [x, y, 1, 1])[:3] - t        (rend_util.py:105-106, :160)
    a, b, e = i - cx, cy * sk / fy, sk * j / fy
    c = a + b
    f = c - e
    x, y = f / fx, (j - cy) / fy
    px, py, p2, t = np.abs(P[:3, 0] * x[:, None]), np.abs(P[:3, 1] * y[:, None]), np.abs(P[:3, 2])[None], np.abs(P[:3, 3])[None]
    ref = P[:3, 0] * x[:, None] + P[:3, 1] * y[:, None] + P[:3, 2]
    # Operation count of ((p0 x + p1 y) + p2 + t) - t, each rounding relative to its own result (fused multiply-adds only round less):
    #   p0 x   the product and the four sums s1 = p0 x + p1 y, s2 = s1 + p2, s3 = s2 + t, d = s3 - t, each at most its magnitude's share: 5
    #   p1 y   the same 5 and y's own two roundings (j - cy, / fy): 7
    #   p2     s2, s3, d: 3          t   s3 alone (d = s3 - t is bounded by the exact direction): 1, the cancellation of world - cam_loc
    # and x, whose sums do cancel near the principal point, enters through its absolute error |p0| dx with
    #   fx dx <= (|a| + 2 |b| + |c| + 2 |e| + 2 |f|) u   (a = i - cx: 1; b = cy sk / fy: 2; c = a + b: 1; e = sk j / fy: 2; f = c - e: 1; / fx: 1)
    # Every constant is below the 8 (|p0 x| + |p1 y| + |p2| + 2 |t|) first proposed for this check; that this bound is the smaller one on
    # every ray of the matrix is asserted below.
    dx = (np.abs(a) + 2 * np.abs(b) + np.abs(c) + 2 * np.abs(e) + 2 * np.abs(f)) / abs(fx)
    bound = SAFETY * U * (5 * px + 7 * py + 3 * p2 + t + np.abs(P[:3, 0])[None] * dx[:, None])
    assert np.all(bound <= SAFETY * 8 * U * (px + py + p2 + 2 * t)), case["name"]
    err = np.abs(np.asarray(o["rays_d"][:n], np.float64) - ref)
    rep.samples += err.size
    rep.check(np.all(err <= bound), f"rays_d: worst error / bound {float(np.max(err / bound, initial=0)):.3g}")
    rep.check(same_bits(o["rays_o"][:n], np.broadcast_to(case["pose"][:3, 3], (n, 3))), "rays_o is not the translation")
    rep.check(same_bits(o["rays_o"][n], fsent(3)) and same_bits(o["rays_d"][n], fsent(3)), "row n written")
    _inputs_unchanged(rep, case, o, ("pose", "K", "select"))
    return rep.finish()


# ==== normalize_dirs ==========================================================================================================================
ND_N = [1, 255, 256, 257]


def normalize_cases():
    cases = []
    for k, n in enumerate(ND_N + [1]):
        rng = np.random.default_rng(6000 + k)
        x = (rng.choice([-1.0, 1.0], (n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 3))).astype(np.float32)
        zero = k == len(ND_N) or n > 1
        if zero:
            x[n - 1] = 0.0                           # the zero vector: exactly (0, 0, 0) through the 1e-12 clamp, not NaN
        if n > 2:
            x[1] = [0.0, -0.0, 3.0e-3]               # a vector along one axis
        cases.append(dict(stage="normalize", name=f"normalize_dirs n={n}{' zero vector' if zero else ''}", n=n, x=x, out=dict(out=fsent((n + 1, 3)))))
    return cases


def check_normalize(case, o):
    rep = Report(case["name"])
    n = case["n"]
    rep.rays = n
    x = case["x"].astype(np.float64)
    nrm = np.linalg.norm(x, axis=-1, keepdims=True)
    nz = nrm[:, 0] > 0
    got = np.asarray(o["out"][:n], np.float64)
    # x / max(sqrt(x x + y y + z z), 1e-12): the sum of squares carries at most 3 u (three products, two sums of non-negative terms; fewer
    # when fused), the square root halves it and rounds once (2.5 u), the quotient rounds once more: 3.5 u, rounded up to 4 u, of a component
    # of at most 1.  The norm of the result inherits the same relative error.
    tol = SAFETY * 4 * U
    rep.samples += got.size
    rep.check(np.all(np.abs(got[nz] - x[nz] / nrm[nz]) <= tol), f"worst component error {float(np.max(np.abs(got[nz] - x[nz] / nrm[nz]), initial=0)):.3g}")
    rep.check(np.all(np.abs(np.linalg.norm(got[nz], axis=-1) - 1) <= tol), "the result is not of unit length")
    rep.check(same_bits(np.abs(np.asarray(o["out"][:n])[~nz]), np.zeros((int((~nz).sum()), 3), np.float32)), "the zero vector does not give (0, 0, 0)")
    rep.check(same_bits(o["out"][n], fsent(3)), "row n written")
    _inputs_unchanged(rep, case, o, ("x",))
    return rep.finish()


# ==== chains on an analytic surface ===========================================================================================================
CHAIN_R, CHAIN_FAR = 1027, 5.5
CHAIN_N, SURFACES = [64, 257], ["sphere", "two_spheres"]
_C1, _R1, _C2, _R2 = np.array([0.0, 0.0, -0.6]), 0.5, np.array([0.0, 0.0, 0.8]), 0.6


def sdf64(surface, p):
    if surface == "sphere":
        return np.linalg.norm(p, axis=-1) - 1.0
    return np.minimum(np.linalg.norm(p - _C1, axis=-1) - _R1, np.linalg.norm(p - _C2, axis=-1) - _R2)


def chain_rays(surface, R=CHAIN_R):
    """Rays from z = -3 with jittered origins and directions; on the union of two spheres along the axis every eighth ray starts at a depth
    that lies inside the first sphere (for the rays near the axis)."""
    rng = np.random.default_rng(7000 + SURFACES.index(surface))
    o = np.concatenate([rng.normal(0, 0.03, (R, 2)), np.full((R, 1), -3.0)], -1).astype(np.float32)
    dn = _unit(np.concatenate([rng.normal(0, 0.2, (R, 2)), np.ones((R, 1))], -1))
    near = (0.5 + 0.001 * (np.arange(R) % 7)).astype(np.float32)
    if surface == "two_spheres":
        near[::8] = 2.3
    far = (CHAIN_FAR - 0.002 * (np.arange(R) % 5)).astype(np.float32)
    return o, dn, near, far


def sdf_at(surface, o, dn, d):
    """The surface on the host: fp64 at the fp32 depths d [R] or [R, N], rounded to fp32."""
    d = np.asarray(d, np.float64)
    if d.ndim == 1:
        return sdf64(surface, o.astype(np.float64) + dn.astype(np.float64) * d[:, None]).astype(np.float32)
    return sdf64(surface, o.astype(np.float64)[:, None] + dn.astype(np.float64)[:, None] * d[..., None]).astype(np.float32)


def chain_root_finding(run, surface, N, tau, n_secant=8):
    """first_crossing -> n_secant x secant_update -> root_finish through run[stage](case) -> outputs, f_mid evaluated on the host at the
    implementation's own d_pred.  Every step is checked from the implementation's own previous state (no accumulated error, no decision
    flips).  -> (reports, residual |sdf(o + d dn) - tau| [R], hit mask [R])."""
    o, dn, near, far = chain_rays(surface)
    R = len(near)
    tau32 = np.float32(tau)
    depth = S.linspace_depths(S.torch_lin(N), near, far, R)
    tag = f"chain {surface} N={N} tau={tau:g}"
    c = first_crossing_case(f"{tag}: first_crossing", sdf_at(surface, o, dn, depth), depth, tau)
    st = run["first_crossing"](c)
    reps = [check_first_crossing(c, st)]
    mask, m0 = np.asarray(st["mask"][:R]).copy(), np.asarray(st["mask0"][:R]).copy()
    brk, d_pred = np.asarray(st["bracket"][:R]).copy(), np.asarray(st["d_pred"][:R]).copy()
    for it in range(n_secant):
        c = secant_case(f"{tag}: secant {it + 1}", sdf_at(surface, o, dn, d_pred), tau, mask, brk, d_pred)
        st = run["secant_update"](c)
        reps.append(check_secant(c, st))
        brk, d_pred = np.asarray(st["bracket"][:R]).copy(), np.asarray(st["d_pred"][:R]).copy()
    c = root_finish_case(f"{tag}: root_finish", o, dn, mask, m0, d_pred, far, CHAIN_FAR, 1)
    st = run["root_finish"](c)
    reps.append(check_root_finish(c, st))
    hit = mask.astype(bool)
    with np.errstate(all="ignore"):
        d = np.where(hit, np.asarray(st["d_out"][:R], np.float64), 0.0)
    res = np.abs(sdf64(surface, o.astype(np.float64) + dn.astype(np.float64) * d[:, None]) - float(tau32))
    return reps, np.where(hit, res, 0.0), hit


def chain_sphere_tracing(run, n_iters=20):
    """n_iters x sphere_trace_step on the unit sphere with host-evaluated values: d and the mask bit-equal to the restatement after every step."""
    o, dn, near, far = chain_rays("sphere")
    R = len(near)
    d, mask = near.copy(), np.ones(R, np.uint8)
    reps = []
    for it in range(n_iters):
        c = sphere_step_case(f"chain sphere tracing: step {it + 1}", sdf_at("sphere", o, dn, d), far, CHAIN_FAR, d, mask)
        st = run["sphere_step"](c)
        reps.append(check_sphere_step(c, st))
        d, mask = np.asarray(st["d"][:R]).copy(), np.asarray(st["mask"][:R]).copy()
    return reps, d, mask.astype(bool)


CASES = {"first_crossing": first_crossing_cases, "secant_update": secant_cases, "root_finish": root_finish_cases,
         "sphere_step": sphere_step_cases, "get_rays": get_rays_cases, "normalize": normalize_cases}
CHECK = {"first_crossing": check_first_crossing, "secant_update": check_secant, "root_finish": check_root_finish,
         "sphere_step": check_sphere_step, "get_rays": check_get_rays, "normalize": check_normalize}
