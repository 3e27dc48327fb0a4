"""fp64 references of the VGG16 perceptual term's stages (csrc/vgg_conv.hip, csrc/gemm_f32.h) and of nerfart_geometry_feature
(csrc/geo_feature.hip), with a worst-case error model and a comparator.

Every function takes the kernels' own stored fp32 arrays, in the kernels' layouts (nerfart_vgg16_workspace_layout in include/nerfart_hip.h: NHWC,
both images, the prediction's rows first), as float64 VALUES.  A stage is compared with the fp64 evaluation of THAT stage on the kernel's stored
input, so no decision (ReLU, max-pool, sign) is ever taken twice: forward stages are continuous, and every backward decision is a comparison of
stored fp32 values that the reference repeats exactly.  Given the decisions, the backward is linear in the cotangent; the fp64 backward with the
kernel's decisions is the exact reference and its bound is the same linear map run over absolute values.  No case, and no share of a buffer's
elements, is left out.  tests/test_vgg_ref.py shows on the CPU that the comparator accepts an fp32 stand-in of the kernels' data flow and rejects
it with injected bugs; tests/test_gpu_vgg_stages.py holds the HIP kernels to it.

DECISION RULES (the kernels', pinned against torch's autograd in tests/test_vgg_ref.py): sign(0) = 0; the ReLU mask is y > 0, strictly; un-pool
sends a window's cotangent to the FIRST maximum of the 2 x 2 window in row-major scan (strict >), and only if that maximum is > 0 (the ReLU below
the pool); the L1's mask is the PREDICTION's feature > 0.

ERROR MODEL (u = 2^-24; no fitted factor anywhere; TINY = 2^-126 per operation stands for a flushed or denormal result).
  exact      im2col (cols), max-pool, g = sign * mask, and the zero columns 27..63 of dcols: compared bit for bit.
  conv       out = sum_k a_k w_k + b over K = 9 Cin terms (32 for conv1_1: 27 real columns and 5 zeros) in fp32, any order, then max(., 0).
             With S = sum |a_k| |w_k| + |b| no term passes more than K + 1 roundings, so |out - exact| <= gamma_{K+1} S <= (K + 2) u S
             (gamma_n = n u / (1 - n u); the second inequality holds for K <= 4000, K <= 2304 here: the bound is rigorous, not first order);
             one output rounding u |out| is added as stated by the model; ReLU is 1-Lipschitz and comes after.
  loss       k_l1_sign: grid = min(ceil(n / 256), 262144) blocks of 256 threads; a thread adds c = ceil(n / (256 grid)) terms |a - b| (1 rounding
             for the difference, c - 1 for the chain: the first add to 0 is exact), 6 shuffle adds, 3 adds of the 4 wave partials, the
             conversion of n and the division (2), and one atomic add per block.  The terms are >= 0, so every running sum is <= the loss
             and the atomics cost at most (grid - 1) u loss in any order.  |loss - exact| <= gamma_{c + grid + 10} loss + TINY.  Atomic order is
             not deterministic: the loss is never compared bit for bit (except the exact 0 of equal images).
  backward   at each transposed convolution (K = 9 Cout terms)   bound_in = |W|^T (*) bound_out + (K + 2) u (|W|^T (*) |g_out|) + (K + 2) TINY,
             through the same masks and un-pool routing as the values (a masked element is an exact 0).  dcols = ga . W0 is the same with
             K = 64.  g_img = scale * (sum of the <= 9 dcols entries of the windows that contain the pixel): the gather's 8 adds cost
             9 u sum |dcols|, scale = upstream * (1 / n) carries 2 roundings (the reciprocal on the host, the product), the final multiply one:
             bound = |scale| (sum bound_dcols + 9 u sum |dcols|) + 3 u |g_img| + TINY.
             The recursion multiplies the bound by the norm of |W| at every layer (about 50 with He-initialised weights) while the values, whose
             signs cancel, keep their size: after six layers it is orders of magnitude above the values and holds the deep chain only to
             "finite, and exactly 0 where a mask or the un-pool routing says 0".  The teeth of the backward are the stages that can be
             checked from STORED inputs, one stage's bound each (backward_tail): after the backward the ping-pong buffers hold gb = the
             un-pooled, masked cotangent of y[1] and ga = the masked cotangent of y[0], so ga is held to conv1_2^T(gb) (K = 576), dcols to
             ga . W0 (K = 64) and g_img to scale * gather(dcols) (9 u sum |dcols| + 3 u |g_img|); gb's exact zeros pin the un-pool routing.
  geometry   W[o, :] = (g[o + 1] v[o + 1, :]) * (1 / sqrt(sum v^2)) (k_fold_feature_rows): the squares (1 rounding) and the 8-level pairwise
             tree (8) give the sum to 9 u, the square root halves that (4.5 u) and adds its own <= 1 ulp = 2 u, the reciprocal <= 1 ulp = 2 u,
             the two multiplies 2 u:  e_fold = 10.5 u relative on every folded weight.  Then the GEMM with K = 256 on the folded weights:
             |out - exact| <= e_fold sum |h| |W| + (K + 2) u (1 + e_fold) S + u |out| + (K + 2) TINY,  S = sum |h| |W| + |b|.
"""
import numpy as np
import torch
import torch.nn.functional as TF

U = 2.0 ** -24
TINY = 2.0 ** -126
NCONV = 7
CIN = [3, 64, 64, 128, 128, 256, 256]
COUT = [64, 64, 128, 128, 256, 256, 256]
LEVEL = [0, 0, 1, 1, 2, 2, 2]
POOLED_INPUT = (2, 4)                       # a 2 x 2 max-pool precedes these convolutions
MAX_GRID = 4096 * 64                        # grid_for() of csrc/vgg_conv.hip
E_FOLD = 10.5 * U
# nerfart_vgg16_workspace_layout's order
WS_NAMES = ["loss", "cols"] + [f"y{l}" for l in range(NCONV)] + ["p0", "p1", "ga", "gb", "dcols", "total"]

# the smallest geometries check_geo admits and a few next to them: level-2 images 2 high / 2 wide (every pixel a border), a level-2 extent of 6,
# a non-square 10 x 32, squares
SHAPES = [(32, 32), (8, 128), (128, 8), (16, 64), (64, 16), (24, 128), (128, 24), (40, 128), (64, 64)]
KINDS = ["random", "blocks", "equal", "left_equal", "scaled"]
WEIGHT_SEED = 5


def gamma(n):
    return n * U / (1.0 - n * U)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(_f64(x))).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


# ---- weights and cases (fixed by seeds alone; nothing here consults the reference) -------------------------------------------------------------
_weights = {}


def make_weights(seed=WEIGHT_SEED):
    """vgg.VGG16Features(seed)'s convolutions with seeded NON-ZERO biases (the default initialiser's 0 would hide a bias bug) -> ([W], [b]) fp32."""
    if seed not in _weights:
        from nerfart_amd import vgg
        net = vgg.VGG16Features(seed=seed)
        rng = np.random.default_rng(1000 + seed)
        Ws, bs = [], []
        for idx, _, cout, _ in vgg._CONVS:
            Ws.append(net.features[str(idx)].weight.detach().numpy().astype(np.float32).copy())
            bs.append(rng.uniform(-0.25, 0.25, cout).astype(np.float32))
        _weights[seed] = (Ws, bs)
    return _weights[seed]


def make_case(shape, kind, seed=0):
    """img2 [2, 3, H, W] fp32: prediction, then target."""
    H, W = shape
    rng = np.random.default_rng([seed, H, W, KINDS.index(kind)])
    pred = rng.standard_normal((3, H, W))
    targ = rng.standard_normal((3, H, W))
    if kind == "blocks":            # constant 8 x 8 blocks: tied positive 2 x 2 windows at the first pool
        pred = np.repeat(np.repeat(rng.standard_normal((3, H // 8, W // 8)), 8, 1), 8, 2)
    elif kind == "equal":
        targ = pred.copy()
    elif kind == "left_equal":
        targ[:, :, :W // 2] = pred[:, :, :W // 2]
    elif kind == "scaled":
        pred = pred * 1e3
    return dict(name=f"{kind} {H}x{W}", kind=kind, H=H, W=W, img2=np.stack([pred, targ]).astype(np.float32))


def matrix(shape):
    return [make_case(shape, k) for k in KINDS]


# ---- forward stages ----------------------------------------------------------------------------------------------------------------------------
def im2col_c3(img2):
    """[B, 3, H, W] -> cols [B H W, 32] (column c 9 + ky 3 + kx < 27, zero outside the image and in columns 27..31): exact."""
    img2 = np.asarray(img2)
    B, _, H, W = img2.shape
    xp = np.zeros((B, 3, H + 2, W + 2), img2.dtype)
    xp[:, :, 1:-1, 1:-1] = img2
    cols = np.zeros((B, H, W, 32), img2.dtype)
    for c in range(3):
        for ky in range(3):
            for kx in range(3):
                cols[..., c * 9 + ky * 3 + kx] = xp[:, c, ky:ky + H, kx:kx + W]
    return cols.reshape(B * H * W, 32)


def conv1_1_from_cols(cols, W, b):
    """The first convolution as the kernel runs it: cols [M, 32] . W[64, 27]^T + b -> (value [M, 64] BEFORE the ReLU, S)."""
    c, w, b = _f64(cols)[:, :27], _f64(W).reshape(W.shape[0], 27), _f64(b)
    return c @ w.T + b, np.abs(c) @ np.abs(w).T + np.abs(b)


def conv3x3_nhwc(x, W, b):
    """3 x 3, padding 1 convolution of x [B, H, W, Cin] with the REAL weights W [Cout, Cin, 3, 3] (not the packed blob) and bias b ->
    (value [B, H, W, Cout] BEFORE the ReLU, S = sum |a| |w| + |b| per element)."""
    w, bb = torch.from_numpy(_f64(W)), torch.from_numpy(_f64(b))
    xt = _nchw(x)
    return _nhwc(TF.conv2d(xt, w, bb, padding=1)), _nhwc(TF.conv2d(xt.abs(), w.abs(), bb.abs(), padding=1))


def conv_bound(val, S, K):
    return (K + 2) * U * S + U * np.maximum(val, 0.0) + (K + 2) * TINY


def maxpool2(x):
    """[B, H, W, C] -> [B, H / 2, W / 2, C]: exact."""
    x = np.asarray(x)
    return np.maximum(np.maximum(x[:, 0::2, 0::2], x[:, 0::2, 1::2]), np.maximum(x[:, 1::2, 0::2], x[:, 1::2, 1::2]))


def l1_sign(f):
    """f [2, h, w, C] (prediction's features, then the target's) -> (g [h, w, C] = sign(fp - ft) [fp > 0] in f's dtype, exact; the loss in fp64;
    the loss's bound)."""
    f = np.asarray(f)
    a, b = _f64(f[0]), _f64(f[1])
    d = a - b
    g = np.where(a > 0, np.where(d > 0, 1.0, np.where(d < 0, -1.0, 0.0)), 0.0).astype(f.dtype)
    n = a.size
    loss = float(np.abs(d).sum() / n)
    grid = min((n + 255) // 256, MAX_GRID)
    chain = -(-n // (256 * grid))
    return g, loss, gamma(chain + grid + 10) * loss + TINY


# ---- backward ----------------------------------------------------------------------------------------------------------------------------------
def unpool2_relu(g, yact):
    """g [1, h, w, C] -> [1, 2 h, 2 w, C]: each window's value to the FIRST maximum of yact's 2 x 2 window in row-major scan (strict >), if that
    maximum is > 0; everything else 0.  g may be a value or a bound: the routing is the same."""
    g, yact = _f64(g), np.asarray(yact)
    v = [yact[:, 0::2, 0::2], yact[:, 0::2, 1::2], yact[:, 1::2, 0::2], yact[:, 1::2, 1::2]]
    m, best = v[0], np.zeros(v[0].shape, np.int64)
    for q in (1, 2, 3):
        upd = v[q] > m
        m = np.where(upd, v[q], m)
        best = np.where(upd, q, best)
    out = np.zeros(yact.shape, np.float64)
    for q, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, dy::2, dx::2] = np.where((best == q) & (m > 0), g, 0.0)
    return out


def col2im_c3(dcols):
    """dcols [H, W, >= 27] -> [3, H, W]: the sum over the nine windows that contain a pixel (window (oy, ox) = (y - ky + 1, x - kx + 1) reads the
    pixel with its tap (ky, kx))."""
    d = _f64(dcols)
    H, W = d.shape[:2]
    P = np.zeros((H + 2, W + 2, d.shape[2]))
    P[1:-1, 1:-1] = d
    g = np.zeros((3, H, W))
    for c in range(3):
        for ky in range(3):
            for kx in range(3):
                g[c] += P[2 - ky:2 - ky + H, 2 - kx:2 - kx + W, c * 9 + ky * 3 + kx]
    return g


def backward_dcols(y, Ws):
    """The part of the backward that does not depend on the upstream factor: from the stored activations y[0..6] ([2, h, w, C] each; the
    prediction's rows are used) and the real weights -> dict(ga = sign * mask, dcols [H W, 64], dcols_bound, n, H, W)."""
    g0 = l1_sign(y[6])[0]
    n = g0.size
    ga = _nchw(g0[None])
    bd = torch.zeros_like(ga)
    for l in range(NCONV - 1, 0, -1):
        w = torch.from_numpy(_f64(Ws[l]))                          # [Cout, Cin, 3, 3]: conv_transpose2d's [in, out, kH, kW]
        K = 9 * COUT[l]
        gin = TF.conv_transpose2d(ga, w, padding=1)
        bin_ = TF.conv_transpose2d(bd, w.abs(), padding=1) + (K + 2) * U * TF.conv_transpose2d(ga.abs(), w.abs(), padding=1) + (K + 2) * TINY
        ylow = np.asarray(y[l - 1])[0:1]                           # the prediction's activation below
        if l in POOLED_INPUT:
            ga = _nchw(unpool2_relu(_nhwc(gin), ylow))
            bd = _nchw(unpool2_relu(_nhwc(bin_), ylow))
        else:
            mask = _nchw(ylow > 0)
            ga, bd = gin * mask, bin_ * mask
        if l == 2:
            gb_end, gb_end_bound = _nhwc(ga)[0], _nhwc(bd)[0]
    H, W = ga.shape[2:]
    gam, bdm = _nhwc(ga).reshape(H * W, 64), _nhwc(bd).reshape(H * W, 64)
    w0 = _f64(Ws[0]).reshape(64, 27)
    dcols, dcols_bound = np.zeros((H * W, 64)), np.zeros((H * W, 64))
    dcols[:, :27] = gam @ w0
    dcols_bound[:, :27] = bdm @ np.abs(w0) + (64 + 2) * U * (np.abs(gam) @ np.abs(w0)) + (64 + 2) * TINY
    return dict(ga=g0, dcols=dcols, dcols_bound=dcols_bound, n=n, H=H, W=W, gb_end=gb_end, gb_end_bound=gb_end_bound, ga_end=gam, ga_end_bound=bdm)


def backward_tail(gb_end, ga_end, dcols, y0, W1, W0, upstream, n):
    """The last three stages of the backward, each from the kernel's own STORED input (what the ping-pong buffers and dcols hold after
    nerfart_vgg16_l1_bwd), so each bound is one stage's: ga_end [H W, 64] = [y0 > 0] conv1_2^T(gb_end [H, W, 64]) (K = 576);
    dcols = ga_end . W0 (K = 64); g_img = scale * gather(dcols) -> dict of (value, bound) pairs."""
    gb = _nchw(_f64(gb_end)[None])
    H, W = gb.shape[2:]
    w = torch.from_numpy(_f64(W1))
    K = 9 * COUT[1]
    mask = _nchw(np.asarray(y0)[0:1] > 0)
    v = _nhwc(TF.conv_transpose2d(gb, w, padding=1) * mask).reshape(H * W, 64)
    b = _nhwc(((K + 2) * U * TF.conv_transpose2d(gb.abs(), w.abs(), padding=1) + (K + 2) * TINY) * mask).reshape(H * W, 64)
    w0, ga = _f64(W0).reshape(64, 27), _f64(ga_end)
    dv, db = np.zeros((H * W, 64)), np.zeros((H * W, 64))
    dv[:, :27] = ga @ w0
    db[:, :27] = (64 + 2) * U * (np.abs(ga) @ np.abs(w0)) + (64 + 2) * TINY
    scale = float(upstream) / n
    g = scale * col2im_c3(_f64(dcols).reshape(H, W, 64))
    gbnd = abs(scale) * 9 * U * col2im_c3(np.abs(_f64(dcols)).reshape(H, W, 64)) + 3 * U * np.abs(g) + TINY
    return dict(ga_end=(v, b), dcols=(dv, db), g_img=(g, gbnd))


def backward(y, Ws, upstream=1.0, core=None):
    """nerfart_vgg16_l1_bwd -> backward_dcols' dict (`core`, if it is at hand) + g_img [3, H, W], g_img_bound, scale = upstream / n."""
    b = dict(core if core is not None else backward_dcols(y, Ws))
    H, W = b["H"], b["W"]
    scale = float(upstream) / b["n"]
    g_img = scale * col2im_c3(b["dcols"].reshape(H, W, 64))
    gather_bound = col2im_c3(b["dcols_bound"].reshape(H, W, 64)) + 9 * U * col2im_c3(np.abs(b["dcols"]).reshape(H, W, 64))
    b.update(g_img=g_img, g_img_bound=abs(scale) * gather_bound + 3 * U * np.abs(g_img) + TINY, scale=scale)
    return b


# ---- geometry feature --------------------------------------------------------------------------------------------------------------------------
def geometry_feature(g, v, bias, h7):
    """feat [M, 256] = W h7 + bias[1:], W = g[1:] v[1:] / ||v[1:]|| (rows 1..256 of the weight-normed last layer) -> (value, bound)."""
    g, v, bias, h = _f64(g).reshape(-1), _f64(v), _f64(bias).reshape(-1), _f64(h7)
    w = g[1:, None] * v[1:] / np.sqrt((v[1:] ** 2).sum(-1, keepdims=True))
    b = bias[1:]
    val = h @ w.T + b
    Sw = np.abs(h) @ np.abs(w).T
    K = 256
    return val, E_FOLD * Sw + (K + 2) * U * (1 + E_FOLD) * (Sw + np.abs(b)) + U * np.abs(val) + (K + 2) * TINY


# ---- comparator --------------------------------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self, name):
        self.name, self.ratio, self.fail = name, {}, []

    def check(self, ok, msg):
        if not ok:
            self.fail.append(msg)

    def within(self, key, got, ref, bound):
        """max |got - ref| / bound (an exact 0 bound admits only the exact value) -> recorded under key, a failure above 1."""
        got, ref, bound = _f64(got), _f64(ref), np.broadcast_to(_f64(bound), np.shape(ref))
        if got.shape != ref.shape or not np.isfinite(got).all():
            self.ratio[key] = float("inf")
            self.fail.append(f"{key}: shape {got.shape} vs {ref.shape} or a non-finite value")
            return
        err = np.abs(got - ref)
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst = float(r.max()) if r.size else 0.0
        self.ratio[key] = max(self.ratio.get(key, 0.0), worst)
        if not worst <= 1.0:
            i = np.unravel_index(int(np.argmax(r)), r.shape) if r.ndim else ()
            self.fail.append(f"{key}: {worst:.3g} x the bound at {tuple(int(j) for j in i)} (got {got[i]!r}, reference {ref[i]!r}, bound {bound[i]:.3g}; "
                             f"{int((r > 1).sum())} of {r.size} outside)")

    def exact(self, key, got, ref):
        ok = same_bits(got, ref)
        self.ratio[key] = 0.0 if ok else float("inf")
        if not ok:
            got, ref = np.asarray(got), np.asarray(ref)
            n = int((bits(got) != bits(ref)).sum()) if got.shape == ref.shape else -1
            self.fail.append(f"{key}: not bit-exact ({n} elements differ)" if n >= 0 else f"{key}: shape {got.shape} vs {ref.shape}")

    def line(self):
        return f"{self.name:<22}" + "  ".join(f"{k} {v:.3f}" for k, v in self.ratio.items()) + ("" if not self.fail else "  FAIL: " + "; ".join(self.fail))


def check(case, Ws, bs, out):
    """out: the kernels' buffers in their layouts - cols [2 H W, 32], y0..y6 / p0 / p1 [2, h, w, C], ga [H/4, W/4, 256], loss (float), dcols
    [H W, 64], g_img [3, H, W]; optional loss_nokeep (the keep_for_bwd = 0 forward's), g_img_up / dcols_up with `upstream` (a second backward
    with that device scalar), ga_end [H W, 64] / gb_end [H, W, 64] (what the ga / gb buffers hold after the backward)."""
    H, W = case["H"], case["W"]
    rep = Report(case["name"])
    for k in ["cols", "p0", "p1", "ga", "dcols", "g_img"] + [f"y{l}" for l in range(NCONV)]:
        rep.check(bool(np.isfinite(np.asarray(out[k])).all()), f"{k} holds a NaN or an infinity (a row the kernels never wrote?)")
    if rep.fail:
        return rep
    y = [np.asarray(out[f"y{l}"]) for l in range(NCONV)]
    rep.exact("cols", out["cols"], im2col_c3(case["img2"]))
    val, S = conv1_1_from_cols(out["cols"], Ws[0], bs[0])
    rep.within("y0", y[0].reshape(-1, 64), np.maximum(val, 0), conv_bound(val, S, 32))
    x = y[0]
    for l in range(1, NCONV):
        if l in POOLED_INPUT:
            key = "p0" if l == 2 else "p1"
            rep.exact(key, out[key], maxpool2(x))
            x = np.asarray(out[key])
        val, S = conv3x3_nhwc(x, Ws[l], bs[l])
        rep.within(f"y{l}", y[l], np.maximum(val, 0), conv_bound(val, S, 9 * CIN[l]))
        x = y[l]
    g, loss, loss_bound = l1_sign(y[6])
    rep.exact("ga", out["ga"], g)
    rep.within("loss", out["loss"], loss, loss_bound)
    if out.get("loss_nokeep") is not None:
        rep.within("loss_nokeep", out["loss_nokeep"], loss, loss_bound)
    b = backward(y, Ws, 1.0)
    rep.within("dcols", out["dcols"], b["dcols"], b["dcols_bound"])
    rep.within("g_img", out["g_img"], b["g_img"], b["g_img_bound"])
    if out.get("ga_end") is not None:                  # the ping-pong buffers after the backward: the last stages one by one
        rep.within("gb_end", out["gb_end"], b["gb_end"], b["gb_end_bound"])
        rep.within("ga_end", out["ga_end"], b["ga_end"], b["ga_end_bound"])
        t = backward_tail(out["gb_end"], out["ga_end"], out["dcols"], y[0], Ws[1], Ws[0], 1.0, b["n"])
        rep.within("ga_end_stage", out["ga_end"], *t["ga_end"])
        rep.within("dcols_stage", out["dcols"], *t["dcols"])
        rep.within("g_img_stage", out["g_img"], *t["g_img"])
    if out.get("g_img_up") is not None:
        up = float(out["upstream"])
        bu = backward(y, Ws, up, core=b)
        if out.get("ga_end") is not None:
            t = backward_tail(out["gb_end"], out["ga_end"], out["dcols_up"], y[0], Ws[1], Ws[0], up, b["n"])
            rep.within("g_img_up_stage", out["g_img_up"], *t["g_img"])
        rep.within("dcols_up", out["dcols_up"], bu["dcols"], bu["dcols_bound"])
        rep.within("g_img_up", out["g_img_up"], bu["g_img"], bu["g_img_bound"])
        rep.within("g_img_up_lin", out["g_img_up"], up * b["g_img"], abs(up) * b["g_img_bound"])
    if case["kind"] == "equal":
        rep.check(float(out["loss"]) == 0.0, f"equal images: loss {float(out['loss'])!r}, not exactly 0")
        rep.check(not np.asarray(out["g_img"]).any(), "equal images: g_img is not exactly 0")
    return rep
