"""CPU self-tests of tests/stage_ref.py: the fp64 reference reproduces the G6 / G7 goldens, the comparator accepts an independent fp32
implementation (the float32 torch oracle, a different summation order) on every case of the GPU matrix of tests/test_gpu_ray_stages.py,
and it rejects fp32 stand-ins with the bugs these kernels invite.  The stand-ins and their mutants live here, never in product code."""
import numpy as np
import pytest
import torch

import stage_ref as S
from oracle import render as orender
from oracle import sampling


# ---- the reference against the goldens of the real reference (tests/golden/make_golden.py: G6 error bound, G7 samplers) ---------------------
def test_reference_reproduces_G6(golden):
    d, s = golden["G6_d"], golden["G6_s"]
    sig = sampling.sdf_to_sigma(S._t(s), S._t(100.0), S._t(0.01)).numpy()
    x = np.abs(s) / 0.01
    sig = np.where((s >= 0) & (x > S.EXP_ZERO), 0.0, sig)                      # fp32 underflow; below it a denormal exp(-x): absolute error
    assert np.all(np.abs(sig - golden["G6_sigma"]) <= S.SAFETY * (x + 8) * S.U * sig + 100.0 * 2.0 ** -148), "sigma (the per-term model of the bounds)"
    for what, alpha, beta, g in (("scalar", S.G6_ALPHA, S.G6_BETA, golden["G6_bound_scalar"]),
                                 ("per-ray beta", (np.float32(1) / golden["G6_beta_ray"][:, 0]), golden["G6_beta_ray"][:, 0], golden["G6_bound_ray"]),
                                 ("NaN row", S.G6_NAN_ALPHA, S.G6_NAN_BETA, golden["G6_nan_bound"])):
        dd, ss = (golden["G6_nan_d"], golden["G6_nan_s"]) if what == "NaN row" else (d, s)
        B = S.bounds(dd, ss, alpha, beta)
        assert np.array_equal(np.isinf(B["b"]), np.isinf(g)), f"G6 {what}: which bounds are inf"
        fin = np.isfinite(g)
        assert np.all(np.abs(B["b"][fin] - g[fin]) <= B["db"][fin]), f"G6 {what}: outside the error model"
        print(f"  G6 {what}: {int((~fin).sum())} inf entries reproduced, {int(fin.sum())} finite within the model")
    assert np.isinf(golden["G6_nan_bound"][0]).all()


def test_reference_reproduces_G7(golden):
    bins, w = golden["G7_bins"], golden["G7_w"]
    cdf, du = S.pdf_cdf(w.astype(np.float64), np.zeros(w.shape))
    for m in (16, 66):
        u = np.broadcast_to(S.torch_lin(m), (bins.shape[0], m))
        lo, hi, wid = S.icdf_bounds(bins, cdf, u, du)
        g = golden[f"G7_pdf{m}"]
        assert np.all((g >= lo) & (g <= hi)), f"G7_pdf{m}"
        print(f"  G7 pdf{m}: within the model, {int(wid.sum())} of {g.size} widened")
    knots = np.concatenate([np.zeros((bins.shape[0], 1)), golden["G7_cdf"].astype(np.float64)], -1)
    u = np.broadcast_to(S.torch_lin(16), (bins.shape[0], 16))
    lo, hi, wid = S.icdf_bounds(bins, knots, u, np.zeros(bins.shape[0]), np.ones(knots.shape, bool))
    g = golden["G7_cdf16"]
    assert np.all((g >= lo) & (g <= hi)), "G7_cdf16"
    assert (g[2] == bins[2, -1]).sum() == 15 and g[2, 0] == bins[2, 0], "zero-weight row: u = 0 -> bins[0], every other u -> bins[n-1]"
    print(f"  G7 cdf16 (exact knots): within 4 ulp, {int(wid.sum())} widened")


# ---- the fp32 stand-in of each stage entry point (the torch oracle in float32), with switchable injected bugs --------------------------------
class Mut:
    upper_bound = False       # searchsorted(right=True) in place of lower_bound in the inverse CDF
    no_floor = False          # sample_pdf without its + 1e-5
    clamp_round1 = False      # the [0, 1e5] clamp in round 1 too
    no_clamp = False          # no clamp in rounds >= 2
    cdf_shift = False         # opacity CDF shifted by one interval
    bisect_lt = False         # the bisection with m < eps for m <= eps
    merge_new_first = False   # a new sample before an old one of equal depth
    neus_no_prev = False      # NeuS slope estimate without the min with the previous interval's slope
    neus_stride = False       # NeuS per-ray u rows read as the shared table (u_new_stride ignored)
    slot_as_ray = False       # an act slot read as a ray index

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Mut, k), k
            setattr(self, k, v)


def _invert32(m, bins, cdf, u):
    idx = torch.searchsorted(cdf.contiguous(), u.contiguous(), right=m.upper_bound)
    lo = torch.clamp_min(idx - 1, 0)
    hi = torch.clamp_max(idx, cdf.shape[-1] - 1)
    c_lo, c_hi = torch.gather(cdf, -1, lo), torch.gather(cdf, -1, hi)
    b_lo, b_hi = torch.gather(bins, -1, lo), torch.gather(bins, -1, hi)
    denom = c_hi - c_lo
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    return b_lo + (u - c_lo) / denom * (b_hi - b_lo)


def _opacity32(m, d, s, alpha, beta, u):
    R = sampling._opacity_R(d, s, alpha, beta)
    if m.cdf_shift:
        R = torch.cat([R[:, 1:], R[:, -1:] + 1e-3], -1)
    cdf = torch.cat([torch.zeros(d.shape[0], 1), 1 - torch.exp(-R)], -1)
    return _invert32(m, d, cdf, u)


def _pdf32(m, d, w, u):
    w = w if m.no_floor else w + 1e-5
    pdf = w / torch.sum(w, -1, keepdim=True)
    cdf = torch.cat([torch.zeros(d.shape[0], 1), torch.cumsum(pdf, -1)], -1)
    return _invert32(m, d, cdf, u)


def _t32(x):
    return torch.as_tensor(np.array(x, np.float32))


def _col32(x, R):
    return _t32(x).reshape(-1, 1).expand(R, 1)


def run_first_check(case, m):
    o = {k: v.copy() for k, v in case["out"].items()}
    R, n = case["n_rays"], case["n"]
    d, s = _t32(case["dA"][:, :n]), _t32(case["sA"][:, :n])
    a, b = _col32(case["alpha_net"], R), _col32(case["beta_net"], R)
    mx = sampling.error_bound(d, s, a, b).max(-1).values
    cnt = 0
    for r in range(R):
        if not (mx[r] > float(case["eps"])):
            u = _t32(case["u_final"][r] if case["u_stride"] else case["u_final"])[None]
            o["d_fine"][r] = _opacity32(m, d[r:r + 1], s[r:r + 1], a[:1], b[:1], u)[0].numpy()
            o["iter_usage"][r], o["beta_map"][r] = 0.0, case["beta_net"]
        else:
            far = case["far"][r] if case["far"] is not None else case["far_s"]
            o["beta_plus"][r] = S.beta_plus0(far, case["denom"])
            o["act_out"][cnt] = r
            cnt += 1
    o["act_count"][0] = cnt
    return o


def run_upsample(case, m):
    o = {k: v.copy() for k, v in case["out"].items()}
    n, n_up = case["n"], case["n_up"]
    for slot, ray in enumerate(case["act"]):
        src = slot if m.slot_as_ray else ray
        d, s = _t32(case["dA"][ray:ray + 1, :n]), _t32(case["sA"][ray:ray + 1, :n])
        bp = _t32(case["beta_plus"][src:src + 1]).reshape(1, 1)
        w = sampling.error_bound(d, s, 1.0 / bp, bp)
        if case["clamp"] and not m.no_clamp or m.clamp_round1:
            w = torch.clamp(w, 0, 1e5)
        u = _t32(case["u_up"][1:n_up + 1])[None]
        o["d_new"][slot] = torch.sort(_pdf32(m, d, w, u), -1)[0][0].numpy()
    return o


def run_finalize(case, m):
    o = {k: v.copy() for k, v in case["out"].items()}
    n = case["n"]
    for slot, ray in enumerate(case["act"]):
        src = slot if m.slot_as_ray else ray
        bp = _t32(case["beta_plus"][src:src + 1]).reshape(1, 1)
        u = _t32(case["u_final"][ray] if case["u_stride"] else case["u_final"])[None]
        o["d_fine"][ray] = _opacity32(m, _t32(case["dA"][ray:ray + 1, :n]), _t32(case["sA"][ray:ray + 1, :n]), 1.0 / bp, bp, u)[0].numpy()
        o["iter_usage"][ray], o["beta_map"][ray] = -1.0, case["beta_plus"][src]
    return o


def run_merge_check(case, m):
    o = {k: v.copy() for k, v in case["out"].items()}
    n, nu, eps = case["n"], case["n_up"], float(case["eps"])
    cnt = 0
    for slot, ray in enumerate(case["act"]):
        old = (_t32(case["dA"][ray:ray + 1, :n]), _t32(case["sA"][ray:ray + 1, :n]))
        new = (_t32(case["d_new"][slot:slot + 1]), _t32(case["s_new"][slot:slot + 1]))
        first, second = (new, old) if m.merge_new_first else (old, new)
        d, s = sampling._merge_sorted(first[0], first[1], second[0], second[1])
        o["dB"][ray, :n + nu], o["sB"][ray, :n + nu] = d[0].numpy(), s[0].numpy()
        a, b = _col32(case["alpha_net"], 1), _col32(case["beta_net"], 1)
        if not (sampling.error_bound(d, s, a, b).max() > eps):
            u = _t32(case["u_final"][ray] if case["u_stride"] else case["u_final"])[None]
            o["d_fine"][ray] = _opacity32(m, d, s, a, b, u)[0].numpy()
            o["iter_usage"][ray], o["beta_map"][ray] = float(case["it"]), case["beta_net"]
            continue
        hi, lo = _t32(case["out"]["beta_plus"][ray]).reshape(1, 1), b.clone()
        for _ in range(case["max_bisect"]):
            mid = 0.5 * (lo + hi)
            mm = sampling.error_bound(d, s, 1.0 / mid, mid).max()
            le = bool(mm < eps) if m.bisect_lt else bool(mm <= eps)
            hi, lo = (mid, lo) if le else (hi, mid)
        o["beta_plus"][ray] = hi.item()
        o["act_out"][cnt] = ray
        cnt += 1
    o["act_count"][0] = cnt
    return o


def run_neus_upsample(case, m):
    o = {k: v.copy() for k, v in case["out"].items()}
    R, n, inv_s = case["n_rays"], case["n"], float(case["inv_s"])
    d, s = _t32(case["dA"][:, :n]), _t32(case["sA"][:, :n])
    if case["direct"]:
        w = orender.sdf_to_w(s, inv_s)
    else:
        ps, ns, pz, nz = s[:, :-1], s[:, 1:], d[:, :-1], d[:, 1:]
        mid = (ps + ns) * 0.5
        slope = (ns - ps) / (nz - pz + 1e-5)
        prev = torch.cat([torch.zeros_like(slope[:, :1]), slope[:, :-1]], -1)
        slope = (slope if m.neus_no_prev else torch.minimum(prev, slope)).clamp(-10.0, 0.0)
        dist = nz - pz
        pc, nc = orender.cdf_Phi_s(mid - slope * dist * 0.5, inv_s), orender.cdf_Phi_s(mid + slope * dist * 0.5, inv_s)
        w = orender.alpha_to_w((pc - nc + 1e-5) / (pc + 1e-5))
    u = case["u_new"][:1] if m.neus_stride and case["u_stride"] else case["u_new"]
    u = _t32(np.broadcast_to(u, (R, case["n_new"])))
    o["d_new"][:R] = torch.sort(_pdf32(m, d, w, u), -1)[0].numpy()
    return o


RUN = {"neus_upsample": run_neus_upsample, "first_check": run_first_check, "upsample": run_upsample, "finalize": run_finalize, "merge_check": run_merge_check}
CHECK = {"neus_upsample": S.check_neus_upsample, "first_check": S.check_first_check, "upsample": S.check_upsample, "finalize": S.check_finalize, "merge_check": S.check_merge_check}


def all_cases():
    return S.first_check_cases() + S.upsample_cases() + S.finalize_cases() + S.merge_check_cases() + S.neus_upsample_cases()


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = all_cases()
    return _CASES


def run_all(m):
    reps = []
    for c in cases():
        with np.errstate(all="ignore"):
            reps.append(CHECK[c["stage"]](c, RUN[c["stage"]](c, m)))
    return reps


def test_fp32_oracle_passes_every_case():
    reps = run_all(Mut())
    for r in reps:
        print(r.line())
    assert not [r for r in reps if r.fail], [r.line() for r in reps if r.fail]


MUTANTS = {
    "upper_bound": dict(upper_bound=True),
    "no_floor": dict(no_floor=True),
    "clamp_round1": dict(clamp_round1=True),
    "no_clamp": dict(no_clamp=True),
    "cdf_shift": dict(cdf_shift=True),
    "slot_as_ray": dict(slot_as_ray=True),
    "bisect_lt": dict(bisect_lt=True),
    "merge_new_first": dict(merge_new_first=True),
    "neus_no_prev": dict(neus_no_prev=True),
    "neus_stride": dict(neus_stride=True),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_is_rejected(name):
    reps = run_all(Mut(**MUTANTS[name]))
    failed = [r for r in reps if r.fail]
    print(f"  mutant {name}: rejected by {len(failed)} of {len(reps)} cases" + (f", e.g. {failed[0].name}: {failed[0].fail[0][:120]}" if failed else ""))
    assert failed, f"mutant {name} passed every case"
