"""tests/vgg_ref.py on the CPU: the fp64 references equal torch's float64 autograd, the tie rules are torch's, an fp32 stand-in of the kernels' data
flow (im2col + GEMM on the PACKED weight layouts of csrc/vgg_conv.hip, fp32 activations stored layer by layer) passes every check on the whole
case matrix, each injected bug is rejected by a named case, and the matrix's regimes are what they are named for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import vgg_ref as VR

F = np.float32
UP = 3.0


# ---- the fp32 stand-in -------------------------------------------------------------------------------------------------------------------------
def _taps(x, bug=None):
    """x [B, H, W, C] -> [B, H, W, 9, C]: tap ky 3 + kx = the neighbour (y + ky - 1, x + kx - 1), zero outside."""
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    t = np.stack([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 3)
    # a border test off by one on one side: the tap that reads the image's outermost row / column is dropped
    if bug == "tap_top":
        t[:, 1, :, 0:3] = 0
    if bug == "tap_bottom":
        t[:, H - 2, :, 6:9] = 0
    if bug == "tap_left":
        t[:, :, 1, 0::3] = 0
    if bug == "tap_right":
        t[:, :, W - 2, 2::3] = 0
    return t


def _conv(x, W, b, bug=None, relu=True):
    B, H, Wd, C = x.shape
    Wf = (W.transpose(0, 3, 2, 1) if bug == "kykx" else W.transpose(0, 2, 3, 1)).reshape(W.shape[0], 9 * C)      # column (ky 3 + kx) Cin + c
    bb = np.roll(b, -1) if bug == "bias_c1" else b
    out = (_taps(x, bug).reshape(-1, 9 * C) @ Wf.T + bb).astype(F).reshape(B, H, Wd, -1)
    return np.maximum(out, F(0)) if relu else out


def _convT(g, W, bug=None):
    """cotangent [1, h, w, Cout] -> [1, h, w, Cin] on the backward layout [Cin, 9 Cout]: column (ky' 3 + kx') Cout + o = W[o, c, 2 - ky', 2 - kx']."""
    O, C = W.shape[:2]
    Wx = W if bug == "bwd_noflip" else W[:, :, ::-1, ::-1]
    if bug == "bwd_notrans" and O == C:
        Wx = Wx.transpose(1, 0, 2, 3)
    Wb = np.ascontiguousarray(Wx.transpose(1, 2, 3, 0)).reshape(C, 9 * O)
    return (_taps(g).reshape(-1, 9 * O) @ Wb.T).astype(F).reshape(g.shape[:3] + (C,))


def _unpool(g, yact, bug=None):
    v = [yact[:, 0::2, 0::2], yact[:, 0::2, 1::2], yact[:, 1::2, 0::2], yact[:, 1::2, 1::2]]
    m, best = v[0], np.zeros(v[0].shape, int)
    for q in (1, 2, 3):
        upd = (v[q] >= m) if bug == "unpool_last" else (v[q] > m)
        m, best = np.where(upd, v[q], m), np.where(upd, q, best)
    out = np.zeros(yact.shape, F)
    for q, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, dy::2, dx::2] = np.where((best == q) & ((m > 0) | (bug == "unpool_nogate")), g, F(0))
    return out


def stand_in(case, Ws, bs, bug=None):
    H, W = case["H"], case["W"]
    o = {}
    o["cols"] = VR.im2col_c3(case["img2"])
    y = [np.maximum((o["cols"][:, :27] @ Ws[0].reshape(64, 27).T + (np.roll(bs[0], -1) if bug == "bias_c1" else bs[0])).astype(F), F(0)).reshape(2, H, W, 64)]
    x = y[0]
    for l in range(1, 7):
        if l in VR.POOLED_INPUT:
            x = VR.maxpool2(x)
            if bug == "pool3":
                x = np.maximum(np.maximum(y[l - 1][:, 0::2, 0::2], y[l - 1][:, 0::2, 1::2]), y[l - 1][:, 1::2, 0::2])
            o["p0" if l == 2 else "p1"] = x
        x = _conv(x, Ws[l], bs[l], bug, relu=not (bug == "norelu" and l == 3))
        if bug == "swap_rows" and l == 4:
            x = x[::-1].copy()
        y.append(x)
    for l in range(7):
        o[f"y{l}"] = y[l]
    a, b = y[6][0], y[6][1]
    d = a - b
    n = a.size
    o["loss"] = F(np.abs(d).astype(F).sum(dtype=F) / F(n))
    o["loss_nokeep"] = o["loss"]
    s = np.sign(d).astype(F)
    if bug == "sign0":
        s = np.where(d >= 0, F(1), F(-1))
    o["ga"] = np.where((b if bug == "mask_target" else a) > 0, s, F(0)).astype(F)

    def bwd(up):
        g = o["ga"][None]
        for l in range(6, 0, -1):
            gin = _convT(g, Ws[l], bug)
            ylow = y[l - 1][0:1]
            if l in VR.POOLED_INPUT:
                g = _unpool(gin, ylow, bug)
            else:
                g = np.where((ylow >= 0) if bug == "mask_ge" else (ylow > 0), gin, F(0))
            if l == 2:
                gb_end = g[0]
        ga_end = g.reshape(H * W, 64)
        dcols = np.zeros((H * W, 64), F)
        dcols[:, :27] = (g.reshape(H * W, 64) @ Ws[0].reshape(64, 27)).astype(F)
        dd = dcols.reshape(H, W, 64).copy()
        if bug == "col2im_last":
            dd[H - 1] = 0
        scale = F(F(1.0 if bug == "no_upstream" else up) * F(1.0 / ((2 * n) if bug == "n_both" else n)))
        return dcols, (VR.col2im_c3(dd).astype(F) * scale).astype(F), ga_end, gb_end
    o["dcols"], o["g_img"], o["ga_end"], o["gb_end"] = bwd(1.0)
    o["dcols_up"], o["g_img_up"] = bwd(UP)[:2]
    o["upstream"] = UP
    return o


GEO_M = [1, 63, 64, 65, 200]
SENT = F(-7.25)


def geo_inputs(M):
    rng = np.random.default_rng(40 + M)
    return (rng.uniform(0.5, 1.5, 257).astype(F), rng.standard_normal((257, 256)).astype(F), rng.uniform(-0.5, 0.5, 257).astype(F),
            rng.standard_normal((M, 256)).astype(F))


def geo_stand_in(g, v, bias, h7, bug=None):
    M = h7.shape[0]
    w = ((g[1:, None] * v[1:]).astype(F) * (F(1) / np.sqrt((v[1:] * v[1:]).sum(-1, dtype=F, keepdims=True)))).astype(F)
    out = np.full((M + 64, 256), SENT, F)
    rows = M + 1 if bug == "geo_row_M" else M
    hp = np.concatenate([h7, h7[-1:]])                     # the padding row re-reads the last valid one
    out[:rows] = (hp[:rows] @ w.T + (bias[:256] if bug == "geo_bias0" else bias[1:])).astype(F)
    return out


def geo_check(inp, out):
    M = inp[3].shape[0]
    rep = VR.Report(f"geometry M={M}")
    val, bound = VR.geometry_feature(*inp)
    rep.within("feat", out[:M], val, bound)
    rep.check(VR.same_bits(out[M:], np.full((64, 256), SENT, F)), "a guard row past M was written")
    return rep


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    return VR.make_weights()


def _forward64(img2, Ws, bs):
    """The stored activations of an exact (float64) forward, in the kernels' layouts."""
    y, x = [], None
    for l in range(7):
        if l == 0:
            val = VR.conv1_1_from_cols(VR.im2col_c3(img2.astype(np.float64)), Ws[0], bs[0])[0].reshape(2, img2.shape[2], img2.shape[3], 64)
        else:
            val = VR.conv3x3_nhwc(VR.maxpool2(x) if l in VR.POOLED_INPUT else x, Ws[l], bs[l])[0]
        x = np.maximum(val, 0)
        y.append(x)
    return y


def test_reference_equals_torch_float64_autograd(weights):
    Ws, bs = weights
    case = VR.make_case((32, 32), "random", seed=3)
    img = torch.from_numpy(case["img2"].astype(np.float64))
    pred = img[0:1].clone().requires_grad_(True)
    x = torch.cat([pred, img[1:2]])
    acts = []
    for l in range(7):
        if l in VR.POOLED_INPUT:
            x = TF.max_pool2d(x, 2, 2)
        x = TF.relu(TF.conv2d(x, torch.from_numpy(Ws[l].astype(np.float64)), torch.from_numpy(bs[l].astype(np.float64)), padding=1))
        acts.append(x)
    loss = TF.l1_loss(x[0:1], x[1:2])
    (UP * loss).backward()
    y = _forward64(case["img2"], Ws, bs)
    # no decision ties: no exact 0 difference where the prediction is active, and no tied maximum in any pooled window with a positive maximum
    a, b = y[6][0], y[6][1]
    assert not ((a == b) & (a > 0)).any()
    for l in (1, 3):
        v = np.stack([y[l][0, 0::2, 0::2], y[l][0, 0::2, 1::2], y[l][0, 1::2, 0::2], y[l][0, 1::2, 1::2]])
        m = v.max(0)
        assert not (((v == m).sum(0) > 1) & (m > 0)).any()
    for l in range(7):
        np.testing.assert_allclose(y[l], acts[l].detach().permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-13)
    _, l64, _ = VR.l1_sign(y[6])
    assert abs(l64 - float(loss.detach())) <= 1e-13 * abs(l64)
    g = VR.backward(y, Ws, UP)["g_img"]
    ref = pred.grad[0].numpy()
    assert np.abs(g - ref).max() <= 1e-11 * np.abs(ref).max()
    assert np.abs(ref).max() > 0


def test_tie_rules_are_torchs():
    rng = np.random.default_rng(0)
    yact = rng.integers(-1, 3, (1, 8, 12, 5)).astype(np.float64)              # few distinct values: ties in nearly every window
    yact[0, :2, :2] = 0.0                                                      # an all-zero window
    g = rng.standard_normal((1, 4, 6, 5))
    # torch: relu then max-pool; the cotangent goes to max_pool2d's argmax and then through relu's mask
    t = torch.from_numpy(yact).permute(0, 3, 1, 2).clone().requires_grad_(True)
    TF.max_pool2d(TF.relu(t), 2, 2).backward(torch.from_numpy(g).permute(0, 3, 1, 2))
    want = t.grad.permute(0, 2, 3, 1).numpy()
    v = np.stack([yact[:, 0::2, 0::2], yact[:, 0::2, 1::2], yact[:, 1::2, 0::2], yact[:, 1::2, 1::2]])
    assert (((v == v.max(0)).sum(0) > 1) & (v.max(0) > 0)).sum() > 20
    relu_y = np.maximum(yact, 0)                                               # the kernel's stored activation is post-ReLU
    assert np.array_equal(VR.unpool2_relu(g, relu_y), want)
    # sign(0) = 0, as l1_loss's autograd
    a = rng.integers(0, 3, (1, 4, 4, 16)).astype(np.float64)
    b = rng.integers(0, 3, (1, 4, 4, 16)).astype(np.float64)
    ta = torch.from_numpy(a).requires_grad_(True)
    TF.l1_loss(TF.relu(ta), torch.from_numpy(b)).backward()
    gs, loss, _ = VR.l1_sign(np.concatenate([a, b]))
    assert ((a == b) & (a > 0)).sum() > 10
    assert np.array_equal(gs / a.size, ta.grad[0].numpy()) and loss == float(np.abs(a - b).mean())


_runs = {}


def _run(shape, kind, weights, bug=None):
    key = (shape, kind, bug)
    if key not in _runs:
        Ws, bs = weights
        case = VR.make_case(shape, kind)
        _runs[key] = VR.check(case, Ws, bs, stand_in(case, Ws, bs, bug))
    return _runs[key]


@pytest.mark.parametrize("shape", VR.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fp32_stand_in_passes_every_check(shape, weights):
    worst = {}
    for kind in VR.KINDS:
        rep = _run(shape, kind, weights)
        print(rep.line())
        assert not rep.fail, rep.line()
        for k, v in rep.ratio.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert all(0 < worst[k] <= 1 for k in ("y0", "y3", "y6", "loss", "dcols", "g_img", "g_img_up", "ga_end_stage", "dcols_stage", "g_img_stage")), worst


# bug -> (shape, case kind, a buffer whose check must fail)
BUGS = {
    "tap_top": ((8, 128), "random", "y1"), "tap_bottom": ((8, 128), "random", "y1"), "tap_left": ((128, 8), "random", "y1"),
    "tap_right": ((128, 8), "random", "y1"), "kykx": ((32, 32), "random", "y1"), "bwd_noflip": ((32, 32), "random", "ga_end_stage"),
    "bwd_notrans": ((32, 32), "random", "ga_end_stage"), "bias_c1": ((32, 32), "random", "y0"), "norelu": ((32, 32), "random", "y3"),
    "pool3": ((32, 32), "random", "p0"), "unpool_last": ((32, 32), "blocks", "gb_end"), "unpool_nogate": ((32, 32), "random", "gb_end"),
    "mask_ge": ((32, 32), "random", "ga_end_stage"), "sign0": ((32, 32), "equal", "ga"), "mask_target": ((32, 32), "random", "ga"),
    "col2im_last": ((8, 128), "random", "g_img_stage"), "no_upstream": ((32, 32), "random", "g_img_up_stage"),
    "n_both": ((32, 32), "scaled", "g_img_stage"), "swap_rows": ((128, 24), "random", "y4"),
}


@pytest.mark.parametrize("bug", sorted(BUGS))
def test_injected_bug_is_rejected(bug, weights):
    shape, kind, key = BUGS[bug]
    rep = _run(shape, kind, weights, bug)
    assert rep.fail and not rep.ratio.get(key, 0.0) <= 1.0, (bug, rep.line())
    assert not _run(shape, kind, weights).fail


@pytest.mark.parametrize("M", GEO_M)
def test_geometry_feature_stand_in_and_its_bugs(M):
    inp = geo_inputs(M)
    rep = geo_check(inp, geo_stand_in(*inp))
    print(rep.line())
    assert not rep.fail and 0 < rep.ratio["feat"] <= 1, rep.line()
    assert "guard row" in " ".join(geo_check(inp, geo_stand_in(*inp, bug="geo_row_M")).fail)
    assert geo_check(inp, geo_stand_in(*inp, bug="geo_bias0")).ratio["feat"] > 1


def test_the_matrix_holds_the_regimes_it_is_named_for(weights):
    Ws, bs = weights

    def tied_positive_windows(y):
        v = np.stack([y[0, 0::2, 0::2], y[0, 0::2, 1::2], y[0, 1::2, 0::2], y[0, 1::2, 1::2]])
        return int((((v == v.max(0)).sum(0) > 1) & (v.max(0) > 0)).sum())
    for shape in VR.SHAPES:
        for kind in VR.KINDS:
            y = _forward64(VR.make_case(shape, kind)["img2"], Ws, bs)
            a, b = y[6][0], y[6][1]
            if kind == "blocks":
                assert tied_positive_windows(y[1]) > 100, (shape, kind)      # the first pool's; two more convolutions leave no constant interior for the second
            if kind == "equal":
                assert np.array_equal(a, b) and (a > 0).any(), (shape, kind)
            else:
                assert (a != b).any(), (shape, kind)
            if kind == "left_equal" and shape[1] >= 64:                   # wide enough for features that see the left half only
                assert ((a == b) & (a > 0)).any() and ((a != b) & (a > 0)).any(), (shape, kind)
            if kind in ("random", "scaled"):
                for l in range(7):
                    assert (y[l][0] > 0).any() and (y[l][0] == 0).any(), (shape, kind, l)
                v = np.stack([y[1][0, 0::2, 0::2], y[1][0, 0::2, 1::2], y[1][0, 1::2, 0::2], y[1][0, 1::2, 1::2]])
                assert (v.max(0) == 0).any(), "no all-zero window for the un-pool's m > 0 gate"


def test_loss_bound_follows_the_launched_grid():
    """The bound's chain length and block count for the shapes tested and for sizes beyond the grid cap."""
    for n, want in ((16 * 32 * 32, 1 + 64 + 10), (16 * 224 * 224, 1 + 3136 + 10), (256 * VR.MAX_GRID * 3 + 1, 4 + VR.MAX_GRID + 10)):
        f = np.zeros((2, 1, 1, 1), F)
        k = -(-n // (256 * min((n + 255) // 256, VR.MAX_GRID))) + min((n + 255) // 256, VR.MAX_GRID) + 10
        assert k == want
    f = np.ones((2, 4, 4, 256), F)
    f[1] = 0
    _, loss, bound = VR.l1_sign(f)
    assert loss == 1.0 and abs(bound - VR.gamma(1 + 16 + 10)) < 1e-12
