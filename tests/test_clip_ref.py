"""CPU checks of tests/clip_ref.py, the yardstick of tests/test_gpu_clip_stages.py: the chained fp64 references are torch's float64 autograd of
clip_vit.CLIP.encode_image; the weight cases meet their stated conditions; an fp32 / fp16 numpy stand-in of the kernels' arithmetic (the same
rounding points as csrc/clip_vit.hip) is accepted on every case; the stand-in with one injected bug is rejected, each bug by a named case."""
import numpy as np
import pytest
import torch

import clip_ref as R

F = np.float32
D, L, NH, HD, NP = R.D, R.L, R.NH, R.HD, R.NP


def h16(x):
    return np.asarray(x, F).astype(np.float16)


def f(x):
    return np.asarray(x).astype(F)


class StandIn:
    """The kernels' data flow in numpy: fp32 arithmetic, fp16 where the kernels store fp16; `bug` switches one defect on."""

    def __init__(self, W, bug=None, nl=R.NL):
        self.W = {k: f(v) for k, v in W.items()}
        self.bug, self.nl = bug, nl

    def w(self, l, n):
        return self.W[R._blk(l, n)]

    # -- LayerNorm --
    def stats(self, x):
        mean = x.mean(-1, keepdims=True, dtype=F)
        if self.bug == "ln_onepass":
            var = (x * x).mean(-1, keepdims=True, dtype=F) - mean * mean
        else:
            d = x - mean
            var = (d * d).mean(-1, keepdims=True, dtype=F)
        rstd = F(1) / np.sqrt(var + F(0.0 if self.bug == "ln_noeps" else R.EPS))
        return (x - mean) * rstd, rstd

    def ln(self, x, g, b):
        xh, _ = self.stats(x)
        return (xh if self.bug == "ln_nogain" else xh * g) + b

    def ln_bwd(self, dy, x, g):
        xh, rstd = self.stats(x)
        gy = dy if self.bug == "lnbwd_nogain" else dy * g
        m1 = F(0) if self.bug == "lnbwd_nomean" else gy.mean(-1, keepdims=True, dtype=F)
        m2 = F(0) if self.bug == "lnbwd_noxhat" else (gy * xh).mean(-1, keepdims=True, dtype=F)
        return rstd * (gy - m1 - xh * m2)

    # -- attention --
    def split(self, qkv):
        q, k, v = [f(a) for a in R.heads(f(qkv), 3)]
        if self.bug == "qkv_permuted":
            q, k, v = k, v, q
        if self.bug == "attn_image0":
            q, k, v = [np.broadcast_to(a[:1], a.shape) for a in (q, k, v)]
        return q, k, v

    def probs(self, q, k):
        S = q @ R.T(k)
        if self.bug == "softmax_64keys":
            S = np.concatenate([S, np.zeros(S.shape[:-1] + (14,), F)], -1)
        z = (S - S.max(-1, keepdims=True)) * F(1.0 if self.bug == "softmax_no_eighth" else 0.125)
        e = np.exp(z)
        return (e / e.sum(-1, keepdims=True, dtype=F))[..., :L]

    def attn(self, qkv):
        q, k, v = self.split(qkv)
        o = f(h16(self.probs(q, k))) @ v
        if self.bug == "heads_swapped":
            o = o[:, [1, 0] + list(range(2, NH))]
        return h16(R.unheads(o))

    def attn_bwd(self, qkv, datt):
        q, k, v = self.split(qkv)
        dO = f(R.heads(f(datt), 1)[0])
        p = self.probs(q, k)
        dP = dO @ R.T(v)
        rs = (p * dP).sum(-1, keepdims=True, dtype=F)
        dS = f(h16(p * (dP - rs) * F(1.0 if self.bug == "ds_no_eighth" else 0.125)))
        p16 = f(h16(p))
        dq = dS @ k
        dk = (dS if self.bug == "dk_from_ds" else R.T(dS)) @ q
        dv = (p16 if self.bug == "dv_from_p" else R.T(p16)) @ dO
        return h16(np.concatenate([R.unheads(dq), R.unheads(dk), R.unheads(dv)], 1))

    def gelu(self, x):
        return x / (F(1) + np.exp(F(-1.72 if self.bug == "gelu_constant" else -1.702) * x))

    def gelu_grad(self, x):
        s = F(1) / (F(1) + np.exp(F(-1.702) * x))
        return s if self.bug == "gelugrad_no_x_term" else s * (F(1) + F(1.702) * x * (F(1) - s))

    # -- the encoder --
    def forward(self, img):
        W, bug = self.W, self.bug
        img = np.asarray(img, F)
        B = img.shape[0]
        o = {}
        pt = img.reshape(B, 3, 7, 32, 7, 32)
        pt = pt.transpose(0, 2, 4, 1, 5, 3) if bug == "patchify_khkw" else pt.transpose(0, 2, 4, 1, 3, 5)
        o["patches"] = h16(pt.reshape(B * NP, R.PK))
        o["pe"] = f(o["patches"]) @ W["conv"].T
        pe3 = o["pe"].reshape(B, NP, D)
        cls = pe3[:, :1] if bug == "class_is_patch" else np.broadcast_to(W["class_embedding"], (B, 1, D))
        pos = W["positional_embedding"]
        if bug == "pos_off_by_one":
            pos = np.roll(pos, -1, 0)
        o["xemb"] = (np.concatenate([cls, pe3], 1) + pos[None]).reshape(B * L, D)
        x = self.ln(o["xemb"], W["ln_pre.weight"], W["ln_pre.bias"])
        o["xin"], o["xmid"], o["qkv"], o["pre"] = [], [], [], []
        for l in range(self.nl):
            w = lambda n: self.w(l, n)
            a, b = ("ln_2", "ln_2") if bug == "ln1_reads_ln2" else ("ln_1", "ln_1")
            y = f(h16(self.ln(x, w(a + ".weight"), w(b + ".bias"))))
            qkv = h16(y @ w("attn.in_proj_weight").T + (F(0) if bug == "inproj_bias_dropped" else w("attn.in_proj_bias")))
            att = f(self.attn(qkv))
            xmid = (F(0) if bug == "residual_dropped" else x) + (att @ w("attn.out_proj.weight").T + w("attn.out_proj.bias"))
            y = f(h16(self.ln(xmid, w("ln_2.weight"), w("ln_2.bias"))))
            v = y @ w("mlp.c_fc.weight").T + w("mlp.c_fc.bias")
            xn = xmid + (f(h16(self.gelu(v))) @ w("mlp.c_proj.weight").T + w("mlp.c_proj.bias"))
            o["xin"].append(x), o["xmid"].append(xmid), o["qkv"].append(qkv), o["pre"].append(h16(v))
            o["att_last"], o["act_last"] = h16(att), h16(self.gelu(v))
            x = xn
        o["xfin"] = x
        rows = x[[b * NP for b in range(B)]] if bug == "lnpost_row_b49" else x[::L]
        o["x0"] = h16(self.ln(rows, W["ln_post.weight"], W["ln_post.bias"]))
        o["feat"] = f(o["x0"]) @ W["proj"]
        return o

    def backward(self, o, g_feat):
        W, bug = self.W, self.bug
        g = np.asarray(g_feat, F)
        B = g.shape[0]
        s, inv = R.loss_scale(g)
        o["scale"] = np.array([s, inv], F)
        o["g16"] = h16(g * F(s))
        o["t0"] = f(o["g16"]) @ W["proj"].T
        dx = np.zeros((B * L, D), F)
        dx[::L] = self.ln_bwd(o["t0"], o["xfin"][::L], W["ln_post.weight"])
        o["dx_in"], o["act"], o["att"], o["dqkv"], o["t"] = [None] * self.nl, [None] * self.nl, [None] * self.nl, [None] * self.nl, [None] * self.nl
        for l in range(self.nl - 1, -1, -1):
            w = lambda n: self.w(l, n)
            o["dx_in"][l] = dx
            o["act"][l] = h16((f(h16(dx)) @ w("mlp.c_proj.weight")) * self.gelu_grad(f(o["pre"][l])))
            dx = dx + self.ln_bwd(f(o["act"][l]) @ w("mlp.c_fc.weight"), o["xmid"][l], w("ln_2.weight"))
            o["att"][l] = h16(f(h16(dx)) @ w("attn.out_proj.weight"))
            o["dqkv"][l] = self.attn_bwd(o["qkv"][l], o["att"][l])
            o["t"][l] = f(o["dqkv"][l]) @ w("attn.in_proj_weight")
            dx = dx + self.ln_bwd(o["t"][l], o["xin"][l], w("ln_1.weight"))
        o["dx0"] = dx
        dxe = self.ln_bwd(dx, o["xemb"], W["ln_pre.weight"])
        o["y"] = h16(dxe[:B * NP] if bug == "lnpre_bwd_class_row" else dxe[np.arange(B * L) % L != 0])
        o["dpatch"] = f(o["y"]) @ W["conv"]
        o["g_img"] = R.unpatchify(o["dpatch"] * (F(s) if bug == "unpatchify_times_s" else F(inv)))
        return o


_stored = {}


def _W(case):
    if case not in _stored:
        _stored[case] = R.stored(R.make_state(case))
    return _stored[case]


def _cot_kind(kind, B):
    return "image1" if (kind == "constpatch" and B == 3) else "randn"


def test_chained_reference_is_float64_autograd_of_encode_image(monkeypatch):
    from nerfart_amd import clip_vit
    # clip_vit.LayerNorm computes in fp32 whatever the module's dtype (x.float(): CLIP's fp16 convention); for a float64 yardstick it is nn.LayerNorm
    monkeypatch.setattr(clip_vit.LayerNorm, "forward", torch.nn.LayerNorm.forward)
    W = _W("distinct")
    model = clip_vit.CLIP().double()
    sd = {"visual." + k: torch.from_numpy(np.ascontiguousarray(v)).reshape(model.state_dict()["visual." + k].shape) for k, v in W.items() if k != "conv"}
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and not [k for k in missing.missing_keys if k.startswith("visual.")]
    img, g = R.make_image("randn", 1), R.make_cotangent("randn", 1)
    x = torch.from_numpy(img).double().requires_grad_(True)
    feat = model.encode_image(x)
    (feat * torch.from_numpy(g).double()).sum().backward()
    rf, rg, _ = R.chain(W, img, g)
    ef = np.abs(rf - feat.detach().numpy()).max() / np.abs(rf).max()
    eg = np.abs(rg - x.grad.numpy()).max() / np.abs(rg).max()
    print(f"  features {ef:.2e}, pixel gradient {eg:.2e} of their largest entry")
    assert ef < 1e-12 and eg < 1e-11


def test_weight_cases_are_what_they_claim():
    sd = R.make_state("distinct")
    vecs = R.packed_vectors(sd)
    assert len(vecs) == 2 + 4 + 8 * 12
    keys = {v.tobytes() for _, v in vecs}
    assert len(keys) == len(vecs), "two packed vectors are equal"
    for k, v in vecs:
        assert np.count_nonzero(v) == v.size, k
        if k.endswith(("ln_1.weight", "ln_2.weight", "ln_pre.weight", "ln_post.weight")):
            a = np.abs(v)
            assert (v < 0).sum() >= 8 and (a < 1e-3).sum() == 8 and ((a >= 0.5) & (a <= 1.5)).sum() == D - 8 and len(set(v.tolist())) == D
    gains = np.stack([v for k, v in vecs if k.endswith(".weight")])
    assert len(np.unique(gains)) == gains.size, "every LN gain differs from every other"
    b = sd[R._blk(3, "attn.in_proj_bias")]
    sq, sk, sv = b[:D].std(), b[D:2 * D].std(), b[2 * D:].std()
    assert sq > 1.5 * sv > 2.5 * sk
    seeded = R.make_state("seeded")
    assert not seeded[R._blk(0, "attn.in_proj_bias")].any() and (seeded[R._blk(0, "ln_1.weight")] == 1).all()       # what the old test could not see
    # sup |gelu'| used by the forward bound
    x = np.linspace(-20, 20, 400001)
    assert np.abs(R.quick_gelu_grad(x)[0]).max() < R.GELU_LIP


@pytest.mark.parametrize("B", R.BATCHES)
@pytest.mark.parametrize("kind", R.IMAGE_KINDS)
def test_peaked_and_outlier_conditions(kind, B):
    img = R.make_image(kind, B)
    fails, figs = R.case_conditions("peaked", _W("peaked"), img)
    print("  peaked (median row maximum, share one-hot in fp16):", figs)
    assert not fails, fails
    fails, figs = R.case_conditions("outliers", _W("outliers"), img)
    print("  outliers:", figs)
    assert not fails and figs["xin_max"] > 10, (fails, figs)
    # the seeded baseline is NOT peaked: its rows are nearly uniform (why the case exists)
    _, f0 = R.case_conditions("peaked", _W("seeded"), img) if (kind, B) == ("randn", 1) else (None, None)
    assert f0 is None or max(v[0] for v in f0.values()) < 0.2


@pytest.mark.parametrize("B", R.BATCHES)
@pytest.mark.parametrize("kind", R.IMAGE_KINDS)
@pytest.mark.parametrize("case", R.WEIGHT_CASES)
def test_standin_is_accepted(case, kind, B):
    W = _W(case)
    img, g = R.make_image(kind, B), R.make_cotangent(_cot_kind(kind, B), B)
    o = StandIn(W).backward(StandIn(W).forward(img), g)
    rep = R.Report(f"{case} {kind} B={B}")
    R.check_forward(W, img, o, rep=rep)
    R.check_backward(W, g, o, rep=rep)
    print(rep.line())
    assert not rep.fail, rep.line()
    assert max(rep.ratio.values()) > 0.001, "the stand-in is nowhere near any bound: the model pins nothing"


# bug -> (weight case, image kind, B, the buffer whose check must fail).  One block is run (block 0: a peaked block) except where noted.
BUGS = {
    "ln_nogain": ("distinct", "randn", 1, "qkv"),
    "ln1_reads_ln2": ("distinct", "randn", 1, "qkv"),
    "ln_noeps": ("distinct", "randn", 1, "xin0"),
    "inproj_bias_dropped": ("distinct", "randn", 1, "qkv"),
    "qkv_permuted": ("distinct", "randn", 1, "xmid"),
    "heads_swapped": ("distinct", "randn", 1, "xmid"),
    "softmax_no_eighth": ("peaked", "randn", 1, "att"),
    "softmax_64keys": ("distinct", "randn", 1, "att"),            # flat rows: the 14 padded keys (logit 0) take a fifth of the mass
    "attn_image0": ("distinct", "randn", 3, "xmid"),
    "gelu_constant": ("distinct", "randn", 1, "act"),
    "residual_dropped": ("distinct", "randn", 1, "xmid"),
    "class_is_patch": ("distinct", "randn", 1, "xemb"),
    "pos_off_by_one": ("distinct", "randn", 1, "xemb"),
    "patchify_khkw": ("distinct", "randn", 1, "patches"),
    "lnpost_row_b49": ("distinct", "randn", 3, "x0"),
    "lnbwd_nogain": ("distinct", "randn", 1, "b_dx"),
    "lnbwd_nomean": ("distinct", "randn", 1, "b_dx"),
    "lnbwd_noxhat": ("distinct", "randn", 1, "b_dx"),
    "ds_no_eighth": ("peaked", "randn", 1, "b_dqkv"),
    "dk_from_ds": ("peaked", "randn", 1, "b_dqkv"),
    "dv_from_p": ("peaked", "randn", 1, "b_dqkv"),
    "gelugrad_no_x_term": ("distinct", "randn", 1, "b_act"),
    "unpatchify_times_s": ("distinct", "randn", 1, "g_img"),
    "lnpre_bwd_class_row": ("distinct", "constpatch", 3, "y"),
}


@pytest.mark.parametrize("bug", sorted(BUGS))
def test_injected_bug_is_rejected(bug):
    case, kind, B, where = BUGS[bug]
    W = _W(case)
    img, g = R.make_image(kind, B), R.make_cotangent(_cot_kind(kind, B), B)
    reps = {}
    for b in (None, bug):
        o = StandIn(W, b, nl=1).backward(StandIn(W, b, nl=1).forward(img), g)
        rep = R.Report(f"{b}")
        R.check_forward(W, img, o, blocks=[0], rep=rep, nl=1)
        R.check_backward(W, g, o, blocks=[0], rep=rep, nl=1)
        reps[b] = rep
    assert not reps[None].fail, reps[None].line()
    r = reps[bug]
    print(f"  {bug}: {where} at {r.ratio[where]:.3g} x its bound ({case}, {kind}, B = {B})")
    assert r.ratio[where] > 1.0 and r.fail, r.line()


def test_one_pass_variance_is_rejected_on_rows_with_a_large_mean():
    """mean(x^2) - mean^2 in fp32 is as accurate as the two-pass form while |mean| << std, which holds for every token row of every encoder case
    (the bound cannot and should not tell them apart there).  The named case is rows of mean 1000 and deviation 1, where it cancels."""
    rng = np.random.default_rng(3)
    x = (1000.0 + rng.standard_normal((64, D))).astype(F)
    g, b = R._gains(rng, 1)[0], rng.uniform(-0.3, 0.3, D).astype(F)
    ref, bound = R.ln_fwd(x, g.astype(np.float64), b.astype(np.float64))
    W = {}
    good = np.abs(StandIn(W).ln(x, g, b) - ref) / bound
    bad = np.abs(StandIn(W, "ln_onepass").ln(x, g, b) - ref) / bound
    print(f"  two-pass {good.max():.3f}, one-pass {bad.max():.3g} x the bound")
    assert good.max() <= 1.0 < bad.max()


def test_loss_scale_reference():
    for m, k in ((1.0, 4), (16.0, 0), (17.0, -1), (1e-6, 23), (1e4, -10), (6e4, -12), (2.0 ** -100, 104), (2.0 ** -125, 126), (1e-45, 126), (15.999, 0)):
        s, inv = R.loss_scale(np.array([0.0, -m], F))
        assert s == 2.0 ** k and inv == 2.0 ** -k, (m, s)
    assert R.loss_scale(np.zeros(4, F)) == (1.0, 1.0) and R.loss_scale(np.array([np.inf], F)) == (1.0, 1.0)
