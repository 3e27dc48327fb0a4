"""tests/style_ref.py on the CPU: the resample reference is torch's float64 F.pad -> F.interpolate(align_corners=False) -> slicing -> affine chain
and its autograd, the heads reference is float64 autograd of the nerfart_amd.criteria formulas, an fp32 numpy stand-in of the data flow of
csrc/style_heads.hip (fp32 scale, real, cubic weights, row-then-column accumulation, atomics in a shuffled order, block sums as 64-lane trees + 8
partials) passes the comparator on the whole case matrix, each injected bug is rejected by a named case, and the mixed margin gives the shares of
active hinges it is documented with."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import style_ref as SR

F = np.float32


# ---- the fp32 stand-in: resample ---------------------------------------------------------------------------------------------------------------
def _c1(x, A):
    return F(F(F(F(F(A + F(2)) * x) - F(A + F(3))) * x) * x) + F(1)


def _c2(x, A):
    return F(F(F(F(F(F(A * x) - F(F(5) * A)) * x) + F(F(8) * A)) * x)) - F(F(4) * A)


def _taps32(d, in_, out_, bicubic, bug, lo=None, hi=None):
    """taps_of of csrc/style_heads.hip in fp32 -> (idx [4], w [4] fp32, n).  lo / hi: the index clamp (the kernel's 0 and in - 1)."""
    lo = 0 if lo is None else lo
    hi = (in_ if bug == "clamp_in" else in_ - 1) if hi is None else hi
    scale = F(in_) / F(out_)
    real = F(scale * (F(d) + F(0.0 if bug == "no_half" else 0.5))) - F(0.5)
    if bicubic:
        fl = np.floor(real)
        i, x, A = int(fl), F(real - fl), F(-0.5 if bug == "A_half" else -0.75)
        w = [_c2(F(x + F(1)), A), _c1(x, A), _c1(F(F(1) - x), A), _c2(F(F(2) - x), A)]
        return [min(max(i - 1 + k, lo), hi) for k in range(4)], w, 4
    if bug != "bilinear_noclamp":
        real = max(real, F(0))
    i0 = min(int(real), hi)
    i1 = i0 + (1 if i0 < hi else 0)
    l1 = F(real - F(i0))
    if bug != "bilinear_noclamp":
        l1 = min(max(l1, F(0)), F(1))
    return [max(i0, lo), max(i1, lo), i0, i0], [F(F(1) - l1), l1, F(0), F(0)], 2


def _plan(case, bug=None):
    """Per output element: the flat source indices [n_out, 16], validity, fp32 weights wy [n_out, 4], wx [n_out, 4] (taps beyond n hold weight 0 and
    are invalid), the channel and the image; plus the flat source buffer's length."""
    g, bic = case["geo"], case["mode"] == "bicubic"
    pad_t, pad_l = (g["pad_l"], g["pad_t"]) if bug == "pad_swap" else (g["pad_t"], g["pad_l"])
    idx, ok, WY, WX, CH, NN = [], [], [], [], [], []
    for n in range(g["N"]):
        y0, x0 = (int(case["crop"][n][0]), int(case["crop"][n][1])) if case["crop"] is not None else (0, 0)
        if bug == "crop_swap":
            y0, x0 = x0, y0
        sn = n if (g["n_src"] != 1 or bug == "src_n") else 0
        if case["win"] is not None:
            wy_, wx_, vHs, vWs = (int(v) for v in case["win"][n])
            vHp, vWp, pt, pl, stride = vHs, vWs, 0, 0, (vWs if bug == "win_stride" else g["Ws"])
            off = wy_ * g["Ws"] + wx_
            ylim = (-wy_, g["Hs"] - 1 - wy_) if bug == "win_clamp_src" else (None, None)
            xlim = (-wx_, g["Ws"] - 1 - wx_) if bug == "win_clamp_src" else (None, None)
            yr, xr = ((-wy_, g["Hs"] - wy_), (-wx_, g["Ws"] - wx_)) if bug == "win_clamp_src" else ((0, vHs), (0, vWs))
        else:
            vHs, vWs, vHp, vWp, pt, pl, stride, off = g["Hs"], g["Ws"], g["Hp"], g["Wp"], pad_t, pad_l, g["Ws"], 0
            ylim = (pt, pt + vHs - 1) if bug == "clamp_src_pad" else (None, None)
            xlim = (pl, pl + vWs - 1) if bug == "clamp_src_pad" else (None, None)
            yr, xr = (0, vHs), (0, vWs)
        ty = [_taps32(oy + y0, vHp, g["Hr"], bic, bug, *ylim) for oy in range(g["Ho"])]
        tx = [_taps32(ox + x0, vWp, g["Wr"], bic, bug, *xlim) for ox in range(g["Wo"])]
        for c in range(g["C"]):
            plane = (sn * g["C"] + c) * g["Hs"] * g["Ws"] + off
            for oy in range(g["Ho"]):
                for ox in range(g["Wo"]):
                    ii, kk = np.zeros(16, np.int64), np.zeros(16, bool)
                    for a in range(ty[oy][2]):
                        sy = ty[oy][0][a] - pt
                        for b in range(tx[ox][2]):
                            sx = tx[ox][0][b] - pl
                            if yr[0] <= sy < yr[1] and xr[0] <= sx < xr[1]:
                                ii[4 * a + b], kk[4 * a + b] = plane + sy * stride + sx, True
                    idx.append(ii), ok.append(kk), WY.append(ty[oy][1]), WX.append(tx[ox][1]), CH.append(c), NN.append(n)
    return dict(idx=np.array(idx), ok=np.array(ok), wy=np.array(WY, F), wx=np.array(WX, F), c=np.array(CH), n=np.array(NN))


_plans = {}


def _get_plan(case, bug):
    key = (case["name"], bug if bug in PLAN_BUGS else None)
    if key not in _plans:
        _plans[key] = _plan(case, key[1])
    return _plans[key]


PLAN_BUGS = {"A_half", "no_half", "bilinear_noclamp", "clamp_in", "clamp_src_pad", "pad_swap", "crop_swap", "win_stride", "win_clamp_src", "src_n"}


def _buffer(case, arr):
    """The flat source with seeded finite garbage behind it, so that a wrong plane or stride reads something."""
    junk = np.random.default_rng(5).standard_normal(8 * arr.size + 4096).astype(F)
    return np.concatenate([np.asarray(arr, F).reshape(-1), junk])


def stand_in_fwd(case, bug=None):
    g, p = case["geo"], _get_plan(case, bug)
    buf = _buffer(case, case["src"])
    s = np.where(p["ok"], buf[np.minimum(np.maximum(p["idx"], 0), buf.size - 1)], F(0))
    v = np.zeros(len(s), F)
    for a in range(4):
        row = np.zeros(len(s), F)
        for b in range(4):
            k = 4 * a + b
            row = np.where(p["ok"][:, k], (row + (p["wx"][:, b] * s[:, k]).astype(F)).astype(F), row)
        # a valid row without a valid column adds wy * 0: the same value either way
        v = np.where(p["ok"][:, 4 * a:4 * a + 4].any(1), (v + (p["wy"][:, a] * row).astype(F)).astype(F), v)
    if case["affine"] is not None:
        ci = np.minimum(p["n"], g["C"] - 1) if bug == "affine_n" else p["c"]
        v = ((v * case["affine"][0][ci]).astype(F) + case["affine"][1][ci]).astype(F)
    return v.reshape(g["N"], g["C"], g["Ho"], g["Wo"])


def stand_in_bwd(case, g_dst, pre, bug=None, seed=0):
    g, p = case["geo"], _get_plan(case, bug)
    gd = np.asarray(g_dst, F).reshape(-1)
    if case["affine"] is not None:
        ci = np.minimum(p["n"], g["C"] - 1) if bug == "affine_n" else p["c"]
        gd = (gd * case["affine"][0][ci]).astype(F)
        if bug == "affine_b_bwd":
            gd = (gd + case["affine"][1][ci]).astype(F)
    buf = _buffer(case, pre)
    contrib = ((gd[:, None] * np.repeat(p["wy"], 4, 1)).astype(F) * np.tile(p["wx"], (1, 4))).astype(F)
    live = p["ok"] & (gd != 0)[:, None]
    ii, cc = p["idx"][live], contrib[live]
    order = np.random.default_rng([6, seed]).permutation(len(ii))
    ii, cc = np.minimum(np.maximum(ii[order], 0), buf.size - 1), cc[order]
    if bug == "bwd_overwrite":
        buf[ii] = cc
    else:
        np.add.at(buf, ii, cc)                       # unbuffered: one fp32 rounding per add, in this (shuffled) order
    return buf[:np.asarray(pre).size].reshape(np.asarray(pre).shape)


# ---- the fp32 stand-in: heads ------------------------------------------------------------------------------------------------------------------
def _bsum32(v):
    """block_sum of csrc/style_heads.hip: 8 waves of 64 lanes, xor butterflies 32 .. 1, then the 8 partials in order."""
    x = np.asarray(v, F).reshape(v.shape[:-1] + (8, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = (x + x[..., lane ^ o]).astype(F)
    s = np.zeros(v.shape[:-1], F)
    for i in range(8):
        s = (s + x[..., i, 0]).astype(F)
    return s


def stand_in_heads(case, bug=None):
    P, S, T = case["P"], case["S"], case["T"]
    feats, tdir, t_tgt, t_con, t_neg = case["feats"], case["text_dir"], case["t_tgt"], case["t_con"], case["t_neg"]
    w_dir, w_con, w_nce = (F(w) for w in case["weights"])
    if bug == "w_swap":
        w_con, w_nce = w_nce, w_con
    margin, tau, eps_cos, eps_pd = F(case["margin"]), F(case["tau"]), F(1e-8), F(0.0 if bug == "no_eps_pd" else 1e-6)
    out, g = np.zeros(4, F), np.full((4 + P, 512), np.nan, F)

    def unit(row):
        f = feats[row]
        nrm = np.sqrt(_bsum32(f * f))
        return (f / nrm).astype(F), nrm

    def unit_bwd(gg, fh, nrm):
        if bug == "no_projection":
            return (gg / nrm).astype(F)
        return ((gg - fh * _bsum32(gg * fh)) / nrm).astype(F)

    f0, n0 = unit(0)
    f1, _ = unit(1)
    e = f0 - f1
    en = np.sqrt(_bsum32(e * e))
    eh = (e / en).astype(F)
    dn, ehn, dot = np.sqrt(_bsum32(tdir * tdir)), np.sqrt(_bsum32(eh * eh)), _bsum32(eh * tdir)
    den = F(max(ehn, eps_cos) * max(dn, eps_cos))
    cosv = F(dot / den)
    g_eh = -(tdir / den - cosv * eh / max(F(ehn * ehn), F(eps_cos * eps_cos))).astype(F)
    g_e = ((g_eh - eh * _bsum32(g_eh * eh)) / en).astype(F)
    g[0] = w_dir * unit_bwd(g_e, f0, n0)
    g[1] = g[0] if bug == "row13" else F(0)
    l_dir = F(F(1) - cosv)
    # contrastive
    f2, n2 = unit(2)
    f3, _ = unit(3)
    di = (f2 - f3 + eps_pd).astype(F)
    far_img = np.sqrt(_bsum32(di * di))
    hi = max(F(margin - far_img), F(0))
    L = F(hi * hi)
    g2 = np.zeros(512, F)
    if hi > 0:
        g2 = (F(-2) * hi * di / far_img).astype(F)
        if bug == "img_T_twice":
            g2 = (g2 / F(T)).astype(F)
    acc = F(0)
    tc, tt = (t_con / np.linalg.norm(t_con, axis=-1, keepdims=True), t_tgt / np.linalg.norm(t_tgt, axis=-1, keepdims=True)) if bug == "con_text_unit" else (t_con, t_tgt)
    for t in range(T):
        a, b = (f2 - tt[t].astype(F) + eps_pd).astype(F), (f2 - tc[t].astype(F) + eps_pd).astype(F)
        v0, v1 = _bsum32(a * a), _bsum32(b * b)
        far_t = np.sqrt(v1)
        raw = F(margin - far_t)
        ht = max(raw, F(0))
        acc = F(acc + F(v0 + F(ht * ht)))
        hg = raw if bug == "no_gate" else ht
        g2 = (g2 + ((F(2) * a + (F(-2) * hg * b / far_t if (hg > 0 or bug == "no_gate") else F(0))) / F(T)).astype(F)).astype(F)
    L = F(L + F(acc / F(T)))
    g[2] = w_con * unit_bwd(g2, f2, n2)
    g[3] = g[2] if bug == "row13" else F(0)
    terms0, terms3 = [F(w_dir * l_dir), F(w_con * L)], []
    # PatchNCE
    for p in range(P):
        fp, npn = unit(4 + p)
        fn = max(np.sqrt(_bsum32(fp * fp)), eps_cos)
        gp, Lp = np.zeros(512, F), F(0)
        for t in range(T):
            if bug == "neg_ts":
                tv = np.stack([t_tgt[t]] + [t_neg.reshape(-1, 512)[t * S + s] for s in range(S)])
            else:
                tv = np.stack([t_tgt[t]] + [t_neg[s, t] for s in range(S)])
            tn = np.maximum(np.sqrt(_bsum32(tv * tv)), eps_cos)
            c = (_bsum32(fp * tv) / (fn * tn).astype(F)).astype(F)
            ct = (c / tau).astype(F)
            mx = ct.max()
            z = F(0)
            for k in range(1 + S):
                z = F(z + np.exp(F(ct[k] - mx)))
            lse = F(mx + np.log(z))
            term = F(lse - ct[0])
            Lp = F(Lp + (term if bug == "nce_no_T" else F(term / F(T))))
            gt = np.zeros(512, F)
            for k in range(1 + S):
                pos = 1 if (bug == "softmax_k1" and S >= 1) else 0
                sk = F(np.exp(F(ct[k] - lse)) - F(1.0 if k == pos else 0.0))
                gt = (gt + sk * ((tv[k] / F(fn * tn[k])).astype(F) - (c[k] * fp / F(fn * fn)).astype(F)).astype(F)).astype(F)
            gp = (gp + (gt / (tau if bug == "nce_no_T" else F(tau * F(T)))).astype(F)).astype(F)
        g[4 + p] = w_nce * unit_bwd(gp, fp, npn)
        terms0.append(F(w_nce * Lp))
        terms3.append(Lp)
    order = np.random.default_rng(9).permutation(len(terms0))
    for i in order:
        out[0] = F(out[0] + terms0[i])
    out[1], out[2] = l_dir, L
    for v in terms3[::-1]:
        out[3] = F(out[3] + v)
    return out, g


# ---- references against torch float64 ----------------------------------------------------------------------------------------------------------
def _torch_chain(case, src):
    g, mode = case["geo"], case["mode"]
    outs = []
    for n in range(g["N"]):
        x = src[0 if g["n_src"] == 1 else n][None]
        if case["win"] is not None:
            y, xx, h, w = (int(v) for v in case["win"][n])
            x = x[:, :, y:y + h, xx:xx + w]
        else:
            x = TF.pad(x, (g["pad_l"], g["Wp"] - g["pad_l"] - g["Ws"], g["pad_t"], g["Hp"] - g["pad_t"] - g["Hs"]))
        x = TF.interpolate(x, size=(g["Hr"], g["Wr"]), mode=mode, align_corners=False)
        y0, x0 = (int(case["crop"][n][0]), int(case["crop"][n][1])) if case["crop"] is not None else (0, 0)
        x = x[:, :, y0:y0 + g["Ho"], x0:x0 + g["Wo"]]
        if case["affine"] is not None:
            a = torch.from_numpy(case["affine"].astype(np.float64))
            x = x * a[0][None, :, None, None] + a[1][None, :, None, None]
        outs.append(x)
    return torch.cat(outs)


@pytest.mark.parametrize("name", SR.rcase_names())
def test_resample_reference_equals_torch_float64(name):
    case = SR.rcase(name)
    src = torch.from_numpy(case["src"].astype(np.float64)).requires_grad_(True)
    out = _torch_chain(case, src)
    ref = SR.resample_fwd(case)
    assert out.shape == ref["val"].shape
    scale = max(1.0, float(out.detach().abs().max()))
    assert np.abs(ref["val"] - out.detach().numpy()).max() <= 1e-13 * scale
    assert (ref["bound"] >= 0).all() and np.isfinite(ref["bound"]).all()
    for kind in ("randn", "onehot_corner"):
        cot, pre = SR.cotangent(case, kind), SR.prefill(case, "randn")
        (gs,) = torch.autograd.grad((out * torch.from_numpy(cot.astype(np.float64))).sum(), src, retain_graph=True)
        b = SR.resample_bwd(case, cot, pre)
        want = pre.astype(np.float64) + gs.numpy()
        assert np.abs(b["val"] - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
        assert (gs.numpy()[b["untouched"]] == 0).all()
    # <J x, g> == <x, J^T g> with the affine's offset taken out
    x, cot = case["src"].astype(np.float64), SR.cotangent(case, "randn").astype(np.float64)
    off = 0.0 if case["affine"] is None else case["affine"][1].astype(np.float64)[None, :, None, None]
    lhs = ((ref["val"] - off) * cot).sum()
    rhs = (x * SR.resample_bwd(case, cot, np.zeros_like(x))["val"]).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def _torch_heads(case):
    P, S, T = case["P"], case["S"], case["T"]
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    f = t64(case["feats"]).requires_grad_(True)
    tdir, t_tgt, t_con = t64(case["text_dir"])[None], t64(case["t_tgt"]), t64(case["t_con"])
    m, tau = float(F(case["margin"])), float(F(case["tau"]))
    w = [float(F(x)) for x in case["weights"]]
    fh = f / f.norm(dim=-1, keepdim=True)
    edit = fh[0:1] - fh[1:2].detach()
    edit = edit / edit.norm(dim=-1, keepdim=True)
    l_dir = (1.0 - TF.cosine_similarity(edit, tdir)).mean()
    tg, sr = fh[2:3], fh[3:4].detach()
    l_con = torch.mean(TF.pairwise_distance(tg, t_tgt, keepdim=True) ** 2 + torch.clamp(m - TF.pairwise_distance(tg, t_con, keepdim=True), min=0.0) ** 2
                       + torch.clamp(m - TF.pairwise_distance(tg, sr, keepdim=True), min=0.0) ** 2)
    l_nce = torch.zeros((), dtype=torch.float64)
    if P:
        fp = fh[4:, None, :]
        pos = torch.exp(TF.cosine_similarity(fp, t_tgt[None], dim=-1) / tau)
        neg = sum(torch.exp(TF.cosine_similarity(fp, t64(case["t_neg"])[s][None], dim=-1) / tau) for s in range(S)) if S else torch.zeros_like(pos)
        l_nce = (-torch.log(pos / (pos + neg))).mean(dim=1).sum()
    total = w[0] * l_dir + w[1] * l_con + w[2] * l_nce
    total.backward()
    grad = f.grad.numpy().copy()
    grad[[1, 3]] = 0.0
    return np.array([float(v.detach()) for v in (total, l_dir, l_con, l_nce)]), grad


@pytest.mark.parametrize("name", SR.hcase_names())
def test_heads_reference_equals_torch_float64_autograd(name):
    case = SR.hcase(name)
    r = SR.heads(case)
    out, grad = _torch_heads(case)
    assert np.abs(r["out4"][0] - out).max() <= 1e-11 * max(1.0, np.abs(out).max()), (r["out4"][0], out)
    assert np.abs(r["g"][0] - grad).max() <= 1e-10 * max(np.abs(grad).max(), 1e-300), np.abs(r["g"][0] - grad).max()
    assert np.isfinite(r["g"][1]).all() and (r["g"][1] >= 0).all() and np.isfinite(r["out4"][1]).all()
    if case["S"] == 0:
        assert r["out4"][0][3] == 0.0 and not r["g"][0][4:].any()
    if case["P"] and case["S"] and any(case["weights"]):
        assert np.abs(grad[4:]).max() > 0 or case["weights"][2] == 0


# ---- the stand-in on the whole matrix, and the injected bugs -----------------------------------------------------------------------------------
_runs = {}


def run_resample(name, bug=None):
    if (name, bug) not in _runs:
        case = SR.rcase(name)
        rep = SR.check_resample_fwd(case, stand_in_fwd(case, bug))
        for kind in SR.COT_KINDS:
            for pk in SR.PREFILLS:
                cot, pre = SR.cotangent(case, kind), SR.prefill(case, pk)
                for run in (0, 1):                   # two atomic orders
                    SR.check_resample_bwd(case, cot, pre, stand_in_bwd(case, cot, pre, bug, seed=run), rep, key=f"bwd {kind}/{pk}")
        _runs[(name, bug)] = rep
    return _runs[(name, bug)]


def run_heads(name, bug=None):
    if (name, bug) not in _runs:
        case = SR.hcase(name)
        out4, g = stand_in_heads(case, bug)
        _runs[(name, bug)] = SR.check_heads(case, out4, g)
    return _runs[(name, bug)]


@pytest.mark.parametrize("name", SR.rcase_names())
def test_fp32_stand_in_passes_resample(name):
    rep = run_resample(name)
    print(rep.line())
    assert not rep.fail, rep.line()
    case = SR.rcase(name)
    if SR.resample_fwd(case)["exact"].any():
        assert rep.ratio["fwd_exact"] == 0.0
    elif case["geo"]["Hp"] != case["geo"]["Hr"] and case["geo"]["Hs"] * case["geo"]["Ws"] > 1:      # (a 1 x 1 source is copied: no rounding to see)
        assert 0 < rep.ratio["fwd"] <= 1, rep.line()
    assert 0 < rep.ratio["bwd randn/randn"] <= 1, rep.line()


@pytest.mark.parametrize("name", SR.hcase_names())
def test_fp32_stand_in_passes_heads(name):
    rep = run_heads(name)
    print(rep.line())
    assert not rep.fail, rep.line()
    assert 0 < rep.ratio["out4"] <= 1 and (0 < rep.ratio["g"] <= 1), rep.line()


# bug -> (stage, the case that rejects it, the comparison that must fail)
BUGS = {
    "A_half": ("r", "up 7x5->17x11 bicubic", "fwd"),
    "no_half": ("r", "up 4x4->8x8 bicubic", "fwd"),
    "bilinear_noclamp": ("r", "up 4x4->8x8 bilinear", "fwd"),
    "clamp_in": ("r", "up 7x5->17x11 bicubic", "fwd"),
    "clamp_src_pad": ("r", "pad->10x9 bicubic", "fwd"),
    "pad_swap": ("r", "pad->6x5 bicubic", "fwd"),
    "crop_swap": ("r", "crops bicubic", "fwd"),
    "win_stride": ("r", "windows bicubic", "fwd"),
    "win_clamp_src": ("r", "windows bicubic", "fwd"),
    "src_n": ("r", "crops bilinear", "fwd"),
    "affine_n": ("r", "batch c4 bicubic", "fwd"),
    "affine_b_bwd": ("r", "batch c4 bilinear", "bwd randn/zeros"),
    "bwd_overwrite": ("r", "windows bilinear", "bwd positive/randn"),
    "no_eps_pd": ("h", "shape 16,16,5", "g"),
    "no_gate": ("h", "margin 0", "g"),
    "img_T_twice": ("h", "base 12,8,79", "g"),
    "nce_no_T": ("h", "shape 1,1,2", "out4"),
    "softmax_k1": ("h", "shape 1,1,2", "g"),
    "row13": ("h", "base 12,8,79", None),
    "no_projection": ("h", "base 12,8,79", "g"),
    "w_swap": ("h", "weights 0.3,0,2", "g"),
    "neg_ts": ("h", "shape 3,16,79", "g"),
    "con_text_unit": ("h", "text norms", "out4"),
}


@pytest.mark.parametrize("bug", sorted(BUGS))
def test_injected_bug_is_rejected(bug):
    stage, name, key = BUGS[bug]
    run = run_resample if stage == "r" else run_heads
    rep = run(name, bug)
    assert rep.fail, (bug, rep.line())
    if key is not None:
        assert not rep.ratio.get(key, 0.0) <= 1.0, (bug, key, rep.line())
    else:
        assert "not +0" in " ".join(rep.fail)
    assert not run(name).fail


def test_bilinear_bugs_are_rejected_in_the_backward_too():
    """The bilinear path's own bugs against pad, crop and window geometry (bilinear together with each of them)."""
    for bug, name in (("pad_swap", "pad->10x9 bilinear"), ("crop_swap", "crops bilinear"), ("win_stride", "windows bilinear"), ("win_clamp_src", "windows n_src=N bilinear")):
        rep = run_resample(name, bug)
        assert not rep.ratio["fwd"] <= 1.0 and not rep.ratio["bwd randn/zeros"] <= 1.0, (bug, rep.line())


def test_mixed_margin_gives_the_documented_shares():
    shares, img = {}, {}
    for name in ("margin mixed a", "margin mixed b"):
        r = SR.heads(SR.hcase(name))
        shares[name] = float((r["far_t"] < float(F(SR.MIXED_MARGIN))).mean())
        img[name] = r["far_img"] < float(F(SR.MIXED_MARGIN))
        assert 0.25 <= shares[name] <= 0.75, shares
    print(shares, img)
    assert not img["margin mixed a"] and img["margin mixed b"], img
    r = SR.heads(SR.hcase("margin 0"))
    assert (r["far_t"] > 0).all() and r["far_img"] > 0                      # margin 0: every hinge inactive
    r = SR.heads(SR.hcase("base 12,8,79"))
    assert (r["far_t"] < 2.0).all() and r["far_img"] < 2.0                  # margin 2 on unit rows: every hinge active
    r = SR.heads(SR.hcase("close 2,3"))
    assert r["far_img"] < 0.02                                              # the image hinge deep inside the margin


def test_close_rows_make_the_bound_grow():
    base, close = SR.heads(SR.hcase("base 12,8,79")), SR.heads(SR.hcase("close 0,1"))
    rel = lambda r: float(np.median(r["g"][1][0] / np.abs(r["g"][0][0]).max()))  # noqa: E731
    assert rel(close) > 20 * rel(base), (rel(close), rel(base))


def test_the_matrix_holds_the_geometry_it_is_named_for():
    pad = SR.rcase("pad->10x9 bicubic")["geo"]
    assert pad["pad_t"] != pad["pad_l"] and pad["Hp"] != pad["Wp"] and pad["Hp"] - pad["pad_t"] - pad["Hs"] != pad["pad_t"]
    g = SR.rcase("crops bicubic")["geo"]
    assert max(c[0] for c in SR.CROPS_13x21) + g["Ho"] == g["Hr"] and max(c[1] for c in SR.CROPS_13x21) + g["Wo"] == g["Wr"]
    y, x, h, w = SR.WINDOWS_11x14[2]
    assert (y + h, x + w) == (11, 14) and SR.WINDOWS_11x14[1][2:] == (1, 1)
    for mode in SR.MODES:                            # the exact cases are exact, and the identity with a window too
        for name in ("ident c3", "ident c1", "windows ident"):
            assert SR.resample_fwd(SR.rcase(f"{name} {mode}"))["exact"].all()
    # n_src = 1 with N > 1: several outputs accumulate into one source pixel
    case = SR.rcase("windows bicubic")
    b = SR.resample_bwd(case, SR.cotangent(case, "randn"), SR.prefill(case, "zeros"))
    assert b["untouched"].any() and not b["untouched"].all()
