"""fp64 references of the CLIP ViT-B/32 image encoder's stages (csrc/clip_vit.hip, k_gemm of csrc/gemm_f16.h), forward and backward, with an
error model, the weight / image / cotangent cases and a comparator.

Every function takes the kernels' own STORED buffers (nerfart_clip_vitb32_workspace_layout in include/nerfart_hip.h) as float64 VALUES and evaluates
ONE stage in float64 without any intermediate rounding; the roundings the kernels make inside the stage are part of the bound, not of the value.  So
no rounding decision is ever taken twice and a stage's bound spans that stage only (at most three kernels).  The backward works in the kernels' own
units: every backward buffer holds s x the derivative, s = scale[0].  tests/test_clip_ref.py shows on the CPU that the chained references are torch's
float64 autograd of clip_vit.CLIP.encode_image, that an fp32 / fp16 stand-in of the kernels' arithmetic is accepted and that injected bugs are
rejected; tests/test_gpu_clip_stages.py holds the HIP kernels to it.

ERROR MODEL (u = 2^-24 fp32, h = 2^-11 fp16; first order in u and h; no fitted factor).
  store16    a value v stored as fp16 lands within h |v| + 2^-25 of v (round to nearest; 2^-25 = half the smallest subnormal, which also covers
             every backward entry that rounds to zero).  The fp32 -> fp16 conversion of an A_F32 GEMM operand is the same.
  gemm       out = sum_k a_k w_k (+ bias): products of two stored fp16 numbers are exact in fp32; the K additions are fp32 inside
             v_mfma_f32_32x32x16_f16, whose internal order and rounding mode are not documented.  ASSUMPTION: every one of the K additions errs by
             at most one ulp (2 u) of the running sum, which covers truncation:  |out - exact| <= 2 (K + 2) u S,  S = sum |a_k| |w_k| + |bias|,
             with the bias add and the output rounding (or the residual add, K + 3) inside the K + 2.  An input known only to da contributes
             da . |W|.
  layernorm  mean: 12 adds per lane, 6 shuffle adds, one multiply -> 20 u mean|x|.  d = x - mean: dd = 20 u mean|x| + u |d|.  var = mean d^2:
             2 mean(|d| dd) + 23 u var.  rstd = rsqrtf(var + eps): rho = dvar / (2 (var + eps)) + u + 2 u relative; ASSUMPTION: rsqrtf (v_rsq_f32)
             is good to one ulp = 2 u.  xhat = d rstd: dxh = dd rstd + |xhat| (rho + u).  y = xhat g + b: |g| dxh + u |xhat g| + u |y|.
  ln bwd     dx = rstd (gy - m1 - xhat m2), gy = dy g, m1 = mean gy, m2 = mean(gy xhat): d m1 = 21 u mean|gy|, d m2 = mean(|gy| dxh) + 23 u
             mean|gy xhat|, inner: u |gy| + d m1 + |xhat| d m2 + dxh |m2| + 3 u (|gy| + |m1| + |xhat m2|), dx: rstd d inner + |dx| (rho + u); the
             accumulating store adds u |dx_new|.  An input cotangent known to d propagates through the same linear map over absolute values:
             rstd (|g| d + mean(|g| d) + |xhat| mean(|g| d |xhat|)).
  softmax    S = q . k (gemm, K = 64), z = (S - max S) / 8: dz = (dS + max dS + u |S - m|) / 8 + u |z|.  e = __expf(z) = exp2(z log2 e):
             the rounded product z log2 e moves e by u |z| RELATIVE (the argument-dependent term: |z| reaches 100 on peaked rows); ASSUMPTION:
             v_exp_f32 is good to one ulp, 2 u; a flushed result costs 2^-126.  p = e / sum e over 50 sequential adds:
             dp = p (rel_e + sum_c p_c rel_e_c + 54 u) + 2^-126.  P is stored to LDS as fp16 (store16), O = P V is a gemm with K = 64, stored fp16.
  quickgelu  s = 1 / (1 + __expf(-1.702 x)): rs = (1 - s) (|1.702 x| + 2) u + 3 u relative.  gelu = x s: |gelu| (rs + u).
             gelu' = s (1 + 1.702 x (1 - s)): rs (|gelu'| + 1.702 |x| s^2) + 4 u (s + 1.702 |x| s (1 - s)).  The forward applies gelu to the
             fp32 value whose fp16 rounding is the stored `pre`: |gelu'| <= 1.1 (its supremum is 1.0998) times store16(pre).
  exact      patches = fp16(img); xemb = fp32(cls or pe) + pos, one fp32 add; scale[0] the documented power of two and scale[1] its reciprocal;
             g16 = fp16(g s) (g s is exact); g_img = d patches x scale[1] (a power of two); the class rows' absence from y; rows the kernels
             must not write; zeros.  Compared bit for bit.
The bounds are worst case (every rounding at its limit with the same sign) while real errors grow like sqrt K: observed / bound ratios of a few
per cent are expected (tests/test_gpu_clip_stages.py lists the measured ones).  A wrong index, a dropped term or a wrong constant is an O(1) error.
"""
import math

import numpy as np

from vgg_ref import Report, same_bits

U = 2.0 ** -24
H16 = 2.0 ** -11
SUB16 = 2.0 ** -25
TINY = 2.0 ** -126
EPS = 1e-5
D, L, NH, HD, DM, NL, DOUT, NP, PK, IMG, PS = 768, 50, 12, 64, 3072, 12, 512, 49, 3072, 224, 32
GELU_LIP = 1.1
# nerfart_clip_vitb32_workspace_layout's order
WS_NAMES = ["scale", "patches", "pe", "xemb", "xfin", "y", "att", "act", "t", "dx", "dqkv", "x0", "g16", "t0", "saved", "layer_bytes", "xin", "xmid",
            "qkv", "pre", "total"]

WEIGHT_CASES = ["seeded", "distinct", "peaked", "outliers"]
IMAGE_KINDS = ["randn", "constpatch"]
BATCHES = [1, 3]
PEAKED_BLOCKS = (0, 5, 11)
# q and k rows of in_proj_weight times this in PEAKED_BLOCKS.  Found on the CPU with the fp64 reference, over both image kinds and both batch sizes
# (worst block of the twelve block x case figures: median row maximum, share of rows with a maximum above 1 - 2^-11):
#   2.5: 0.73, 0.04   3: 0.87, 0.14   3.5: 0.94, 0.24   4: 0.98, 0.34   4.5: 0.99, 0.44   5: 1.00, 0.51   6.5: 1.00, 0.68
# 3.5 .. 4.5 meet both conditions (median above 0.9, fewer than half of the rows one-hot in fp16); 4 is the middle.  tests/test_clip_ref.py asserts
# both on every case.
PEAKED_SCALE = 4.0
OUTLIER_CHANNELS = (5, 300, 511, 767)
OUTLIER = 40.0


def f64(x):
    return np.asarray(x, dtype=np.float64)


def r16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def store16(v):
    return H16 * np.abs(v) + SUB16


# ---- weights, images, cotangents (fixed by seeds alone) ------------------------------------------------------------------------------------------
_weights = {}


def _blk(l, name):
    return f"transformer.resblocks.{l}.{name}"


def _gains(rng, n):
    """n LayerNorm gain vectors: magnitudes 0.5 .. 1.5 on a shuffled grid (so every one of the n 768 values differs from every other, in fp32
    too), 16 negative and 8 within 1e-3 of zero in each."""
    big = 0.5 + (rng.permutation(n * (D - 8)) + 0.5) / (n * (D - 8))
    small = ((rng.permutation(n * 8) + 0.5) / (n * 8) * 2.0 - 1.0) * 1e-3
    out = []
    for i in range(n):
        g = np.empty(D)
        idx = rng.permutation(D)
        g[idx[8:]] = big[i * (D - 8):(i + 1) * (D - 8)]
        g[idx[8:24]] *= -1.0
        g[idx[:8]] = small[i * 8:(i + 1) * 8]
        out.append(g.astype(np.float32))
    return out


def make_state(case):
    """`visual.`-relative state dict of fp32 numpy arrays (as the packer takes them: matrices NOT yet rounded)."""
    if case in _weights:
        return _weights[case]
    if case == "seeded":
        from nerfart_amd import clip_vit
        sd = {k[7:]: v.detach().float().numpy().copy() for k, v in clip_vit.build_clip("cpu", seed=0).state_dict().items() if k.startswith("visual.")}
    else:
        sd = {k: v.copy() for k, v in make_state("seeded").items()}
        rng = np.random.default_rng(20260)
        names = ["ln_pre", "ln_post"] + [_blk(l, n) for l in range(NL) for n in ("ln_1", "ln_2")]
        for name, g in zip(names, _gains(rng, len(names))):
            sd[name + ".weight"] = g
            sd[name + ".bias"] = rng.uniform(0.05, 0.3, D).astype(np.float32) * rng.choice([-1.0, 1.0], D).astype(np.float32)
        for l in range(NL):
            b = rng.standard_normal(3 * D)
            b[:D] *= 0.5
            b[D:2 * D] *= 0.125
            b[2 * D:] *= 0.25
            sd[_blk(l, "attn.in_proj_bias")] = b.astype(np.float32)
            sd[_blk(l, "attn.out_proj.bias")] = (0.1 * rng.standard_normal(D)).astype(np.float32)
            sd[_blk(l, "mlp.c_fc.bias")] = (0.3 * rng.standard_normal(DM)).astype(np.float32)
            sd[_blk(l, "mlp.c_proj.bias")] = (0.1 * rng.standard_normal(D)).astype(np.float32)
        if case == "peaked":
            for l in PEAKED_BLOCKS:
                sd[_blk(l, "attn.in_proj_weight")][:2 * D] *= np.float32(PEAKED_SCALE)
        elif case == "outliers":
            for i, c in enumerate(OUTLIER_CHANNELS):
                sgn = np.float32(1.0 if i % 2 == 0 else -1.0)
                sd["class_embedding"][c] = sgn * np.float32(OUTLIER)
                sd["positional_embedding"][:, c] = sgn * np.float32(OUTLIER)
        elif case != "distinct":
            raise KeyError(case)
    _weights[case] = sd
    return sd


def stored(sd):
    """The values the blob holds, as float64: matrices through fp16, vectors fp32."""
    W = {}
    for k, v in sd.items():
        W[k] = f64(r16(v)) if (v.ndim >= 2 and k != "positional_embedding") else f64(v)
    W["conv"] = W["conv1.weight"].reshape(D, PK)
    return W


def packed_vectors(sd):
    return [(k, v) for k, v in sd.items() if v.ndim == 1 or k == "positional_embedding"]


def make_image(kind, B, seed=0):
    rng = np.random.default_rng([seed, B, IMAGE_KINDS.index(kind)])
    img = rng.standard_normal((B, 3, IMG, IMG))
    if kind == "constpatch":
        # a CLIP-normalised image ((rgb - mean) / std of rgb in 0 .. 1) whose patch (2, 3) is one colour
        mean, std = np.array([0.48145466, 0.4578275, 0.40821073]), np.array([0.26862954, 0.26130258, 0.27577711])
        rgb = rng.uniform(0.0, 1.0, (B, 3, IMG, IMG))
        rgb[:, :, 2 * PS:3 * PS, 3 * PS:4 * PS] = rng.uniform(0.0, 1.0, (B, 3, 1, 1))
        img = (rgb - mean[None, :, None, None]) / std[None, :, None, None]
    return img.astype(np.float32)


def make_cotangent(kind, B, seed=0):
    rng = np.random.default_rng([seed, B, 77])
    g = (rng.standard_normal((B, DOUT)) * 1e-3).astype(np.float32)
    if kind == "image1":
        g[[b for b in range(B) if b != 1]] = 0.0
    return g


# ---- building blocks: (value, bound) ---------------------------------------------------------------------------------------------------------------
def gemm(a, w, bias=None, da=None, extra=2):
    """a [M, K] . w [N, K]^T (+ bias) -> (value, bound); da: what is known about a's error."""
    a, w = f64(a), f64(w)
    K = a.shape[1]
    val, S = a @ w.T, np.abs(a) @ np.abs(w).T
    if bias is not None:
        val, S = val + bias, S + np.abs(bias)
    bound = 2 * (K + extra) * U * S + (K + extra) * TINY
    if da is not None:
        bound = bound + da @ np.abs(w).T
    return val, bound


def ln_stats(x):
    x = f64(x)
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + EPS)
    xh = d * rstd
    dd = 20 * U * np.abs(x).mean(-1, keepdims=True) + U * np.abs(d)
    dvar = 2 * (np.abs(d) * dd).mean(-1, keepdims=True) + 23 * U * var
    rho = 0.5 * dvar / (var + EPS) + 3 * U
    dxh = dd * rstd + np.abs(xh) * (rho + U)
    return xh, rstd, dxh, rho


def ln_fwd(x, g, b):
    xh, _, dxh, _ = ln_stats(x)
    y = xh * g + b
    return y, np.abs(g) * dxh + U * np.abs(xh * g) + U * np.abs(y) + TINY


def ln_bwd_abs(d, x, g):
    """The LayerNorm backward's linear map run over absolute values: how a cotangent known to d moves the result."""
    xh, rstd, _, _ = ln_stats(x)
    gd = np.abs(g) * d
    return rstd * (gd + gd.mean(-1, keepdims=True) + np.abs(xh) * (gd * np.abs(xh)).mean(-1, keepdims=True))


def ln_bwd(dy, x, g):
    xh, rstd, dxh, rho = ln_stats(x)
    gy = f64(dy) * g
    m1, m2 = gy.mean(-1, keepdims=True), (gy * xh).mean(-1, keepdims=True)
    dx = rstd * (gy - m1 - xh * m2)
    dm1 = 21 * U * np.abs(gy).mean(-1, keepdims=True)
    dm2 = (np.abs(gy) * dxh).mean(-1, keepdims=True) + 23 * U * np.abs(gy * xh).mean(-1, keepdims=True)
    dinner = U * np.abs(gy) + dm1 + np.abs(xh) * dm2 + dxh * np.abs(m2) + 3 * U * (np.abs(gy) + np.abs(m1) + np.abs(xh * m2))
    return dx, rstd * dinner + np.abs(dx) * (rho + U) + TINY


def heads(x, n):
    """[M, n 768] -> n arrays [B, NH, L, HD]."""
    x = f64(x)
    B = x.shape[0] // L
    x = x.reshape(B, L, n, NH, HD).transpose(2, 0, 3, 1, 4)
    return [x[i] for i in range(n)]


def unheads(x):
    B = x.shape[0]
    return x.transpose(0, 2, 1, 3).reshape(B * L, D)


def T(x):
    return np.swapaxes(x, -1, -2)


def softmax_probs(q, k):
    """-> (p, dp) [B, NH, L, L]: the fp32 probabilities the kernels hold before they round them to fp16."""
    S, Sabs = q @ T(k), np.abs(q) @ np.abs(T(k))
    dS = 2 * (HD + 2) * U * Sabs
    m = S.max(-1, keepdims=True)
    z = (S - m) * 0.125
    dz = 0.125 * (dS + dS.max(-1, keepdims=True) + U * np.abs(S - m)) + U * np.abs(z)
    rel = dz + U * np.abs(z) + 2 * U
    e = np.exp(z)
    p = e / e.sum(-1, keepdims=True)
    return p, p * (rel + (p * rel).sum(-1, keepdims=True) + 54 * U) + TINY


def quick_gelu(x):
    x = f64(x)
    s = 1.0 / (1.0 + np.exp(-1.702 * x))
    rs = (1 - s) * (np.abs(1.702 * x) + 2) * U + 3 * U
    return x * s, np.abs(x * s) * (rs + U) + TINY


def quick_gelu_grad(x):
    x = f64(x)
    s = 1.0 / (1.0 + np.exp(-1.702 * x))
    rs = (1 - s) * (np.abs(1.702 * x) + 2) * U + 3 * U
    g = s * (1.0 + 1.702 * x * (1.0 - s))
    return g, rs * (np.abs(g) + 1.702 * np.abs(x) * s * s) + 4 * U * (s + 1.702 * np.abs(x) * s * (1 - s))


# ---- forward stages --------------------------------------------------------------------------------------------------------------------------------
def patchify(img):
    """[B, 3, 224, 224] fp32 -> fp16 [B 49, 3072], row b 49 + py 7 + px, column c 1024 + kh 32 + kw: exact."""
    img = np.asarray(img, np.float32)
    B = img.shape[0]
    return r16(img.reshape(B, 3, 7, PS, 7, PS).transpose(0, 2, 4, 1, 3, 5).reshape(B * NP, PK))


def unpatchify(dp):
    dp = np.asarray(dp)
    B = dp.shape[0] // NP
    return dp.reshape(B, 7, 7, 3, PS, PS).transpose(0, 3, 1, 4, 2, 5).reshape(B, 3, IMG, IMG)


def embed(pe, W):
    """xemb = fp32(cls or pe row) + pos: one fp32 add -> fp32 array, exact."""
    pe = np.asarray(pe, np.float32)
    B = pe.shape[0] // NP
    x = np.concatenate([np.broadcast_to(W["class_embedding"].astype(np.float32), (B, 1, D)), pe.reshape(B, NP, D)], 1)
    return (x + W["positional_embedding"].astype(np.float32)[None]).reshape(B * L, D)


def attention_fwd(qkv):
    """Stored qkv -> (the attention output [M, 768], the bound of its fp16 store `att`, the probabilities)."""
    q, k, v = heads(qkv, 3)
    p, dp = softmax_probs(q, k)
    o = p @ v
    do = (dp + store16(p)) @ np.abs(v) + 2 * (HD + 2) * U * (p @ np.abs(v))
    o, do = unheads(o), unheads(do)
    return o, do + store16(o), p


def block_fwd(W, l, xin, xmid, qkv, pre):
    """The four checked stages of block l, each from the kernels' stored input -> {name: (value, bound)}; `next` is xin of block l + 1 / xfin."""
    w = lambda n: W[_blk(l, n)]
    out = {}
    y, dy = ln_fwd(xin, w("ln_1.weight"), w("ln_1.bias"))
    v, b = gemm(y, w("attn.in_proj_weight"), w("attn.in_proj_bias"), da=dy + store16(y))
    out["qkv"] = (v, b + store16(v))
    o, do, _ = attention_fwd(qkv)
    v, b = gemm(o, w("attn.out_proj.weight"), w("attn.out_proj.bias"), da=do, extra=3)
    out["xmid"] = (f64(xin) + v, b + 2 * U * np.abs(f64(xin)))
    y, dy = ln_fwd(xmid, w("ln_2.weight"), w("ln_2.bias"))
    v, b = gemm(y, w("mlp.c_fc.weight"), w("mlp.c_fc.bias"), da=dy + store16(y))
    out["pre"] = (v, b + store16(v))
    a, da = quick_gelu(pre)
    v, b = gemm(a, w("mlp.c_proj.weight"), w("mlp.c_proj.bias"), da=da + GELU_LIP * store16(pre) + store16(a), extra=3)
    out["next"] = (f64(xmid) + v, b + 2 * U * np.abs(f64(xmid)))
    return out


def class_rows(x):
    return f64(x)[::L]


def tail_fwd(W, xfin, x0):
    y, dy = ln_fwd(class_rows(xfin), W["ln_post.weight"], W["ln_post.bias"])
    return {"x0": (y, dy + store16(y)), "feat": gemm(x0, W["proj"].T)}


# ---- backward stages -------------------------------------------------------------------------------------------------------------------------------
def loss_scale(g_feat):
    """-> (s, 1 / s) as documented: s = min(2^floor(log2(16 / m)), 2^126), m = max|g|; 1 for m = 0 or a non-finite m."""
    m = float(np.abs(np.asarray(g_feat, np.float32)).max())
    if not (m > 0 and math.isfinite(m)):
        return 1.0, 1.0
    f, e = math.frexp(m)                      # m = f 2^e, 0.5 <= f < 1: floor(log2(16 / m)) = 4 - e, + 1 if f == 0.5
    k = min(4 - e + (1 if f == 0.5 else 0), 126)
    return 2.0 ** k, 2.0 ** -k


def head_bwd(W, g16, t0, xfin):
    B = np.shape(g16)[0]
    dxc, b = ln_bwd(t0, class_rows(xfin), W["ln_post.weight"])
    dx, db = np.zeros((B * L, D)), np.zeros((B * L, D))
    dx[::L], db[::L] = dxc, b
    return {"t0": gemm(g16, W["proj"]), "dx12": (dx, db)}


def attention_bwd(qkv, datt):
    """Stored qkv and stored d attention output -> (dqkv [M, 2304], bound)."""
    q, k, v = heads(qkv, 3)
    dO = heads(datt, 1)[0]
    p, dp = softmax_probs(q, k)
    dP = dO @ T(v)
    ddP = 2 * (HD + 2) * U * (np.abs(dO) @ np.abs(T(v)))
    rs = (p * dP).sum(-1, keepdims=True)
    drs = (dp * np.abs(dP) + p * ddP).sum(-1, keepdims=True) + 52 * U * np.abs(p * dP).sum(-1, keepdims=True)
    dS = p * (dP - rs) * 0.125
    ddS = 0.125 * (dp * np.abs(dP - rs) + p * (ddP + drs + U * np.abs(dP - rs))) + 3 * U * np.abs(dS)
    ddS = ddS + store16(dS)
    dp16 = dp + store16(p)
    g = 2 * (HD + 2) * U
    dq, bq = dS @ k, ddS @ np.abs(k) + g * (np.abs(dS) @ np.abs(k))
    dk, bk = T(dS) @ q, T(ddS) @ np.abs(q) + g * (np.abs(T(dS)) @ np.abs(q))
    dv, bv = T(p) @ dO, T(dp16) @ np.abs(dO) + g * (T(p) @ np.abs(dO))
    val = np.concatenate([unheads(dq), unheads(dk), unheads(dv)], 1)
    bound = np.concatenate([unheads(bq), unheads(bk), unheads(bv)], 1)
    return val, bound + store16(val)


def block_bwd(W, l, dx_in, xin, xmid, qkv, pre, act, att, dqkv, t):
    """The five checked stages of block l's backward from the stored dx that entered it and the buffers it left -> {name: (value, bound)}."""
    w = lambda n: W[_blk(l, n)]
    out = {}
    dx_in = f64(dx_in)
    v, b = gemm(dx_in, w("mlp.c_proj.weight").T, da=store16(dx_in))
    gp, dgp = quick_gelu_grad(pre)
    out["act"] = (v * gp, b * np.abs(gp) + np.abs(v) * dgp + store16(v * gp))
    tm, dtm = gemm(act, w("mlp.c_fc.weight").T)
    lb, dlb = ln_bwd(tm, xmid, w("ln_2.weight"))
    dxm = dx_in + lb
    ddxm = dlb + ln_bwd_abs(dtm, xmid, w("ln_2.weight")) + U * np.abs(dxm)
    v, b = gemm(dxm, w("attn.out_proj.weight").T, da=ddxm + store16(dxm))
    out["att"] = (v, b + store16(v))
    out["dqkv"] = attention_bwd(qkv, att)
    out["t"] = gemm(dqkv, w("attn.in_proj_weight").T)
    lb, dlb = ln_bwd(t, xin, w("ln_1.weight"))
    out["dx"] = (dxm + lb, ddxm + dlb + U * np.abs(dxm + lb))
    return out


def tail_bwd(W, dx0, xemb, y, dpatch, scale):
    """y (d patch embedding, fp16, class rows skipped) from the stored dx and xemb; d patches from the stored y; g_img exactly."""
    B = np.shape(dx0)[0] // L
    v, b = ln_bwd(dx0, xemb, W["ln_pre.weight"])
    keep = np.arange(B * L) % L != 0
    v, b = v[keep], b[keep]
    g = unpatchify(np.asarray(dpatch, np.float32) * np.float32(scale[1]))
    return {"y": (v, b + store16(v)), "dpatch": gemm(y, W["conv"].T)}, g


# ---- the chained reference (no roundings at all) -----------------------------------------------------------------------------------------------------
def chain(W, img, g_feat=None, keep=False):
    """encode_image in float64 (no fp16 anywhere) and, with g_feat, d(feat . g_feat) / d img -> (feat, g_img or None, per-block dict if keep)."""
    B = img.shape[0]
    pt = f64(img).reshape(B, 3, 7, PS, 7, PS).transpose(0, 2, 4, 1, 3, 5).reshape(B * NP, PK)
    pe = pt @ W["conv"].T
    xemb = (np.concatenate([np.broadcast_to(W["class_embedding"], (B, 1, D)), pe.reshape(B, NP, D)], 1) + W["positional_embedding"][None]).reshape(B * L, D)
    x = ln_fwd(xemb, W["ln_pre.weight"], W["ln_pre.bias"])[0]
    sv = []
    for l in range(NL):
        w = lambda n: W[_blk(l, n)]
        qkv = ln_fwd(x, w("ln_1.weight"), w("ln_1.bias"))[0] @ w("attn.in_proj_weight").T + w("attn.in_proj_bias")
        o, _, p = attention_fwd(qkv)
        xmid = x + o @ w("attn.out_proj.weight").T + w("attn.out_proj.bias")
        pre = ln_fwd(xmid, w("ln_2.weight"), w("ln_2.bias"))[0] @ w("mlp.c_fc.weight").T + w("mlp.c_fc.bias")
        xn = xmid + quick_gelu(pre)[0] @ w("mlp.c_proj.weight").T + w("mlp.c_proj.bias")
        sv.append(dict(xin=x, xmid=xmid, qkv=qkv, pre=pre, p=p))
        x = xn
    feat = ln_fwd(class_rows(x), W["ln_post.weight"], W["ln_post.bias"])[0] @ W["proj"]
    if g_feat is None:
        return feat, None, (sv if keep else None)
    dx = np.zeros((B * L, D))
    dx[::L] = ln_bwd(f64(g_feat) @ W["proj"].T, class_rows(x), W["ln_post.weight"])[0]
    for l in range(NL - 1, -1, -1):
        w = lambda n: W[_blk(l, n)]
        s = sv[l]
        dact = (dx @ w("mlp.c_proj.weight")) * quick_gelu_grad(s["pre"])[0]
        dx = dx + ln_bwd(dact @ w("mlp.c_fc.weight"), s["xmid"], w("ln_2.weight"))[0]
        dqkv = attention_bwd(s["qkv"], dx @ w("attn.out_proj.weight"))[0]
        dx = dx + ln_bwd(dqkv @ w("attn.in_proj_weight"), s["xin"], w("ln_1.weight"))[0]
    dxe = ln_bwd(dx, xemb, W["ln_pre.weight"])[0]
    dpe = dxe[np.arange(B * L) % L != 0]
    return feat, unpatchify(dpe @ W["conv"]), (sv if keep else None)


def case_conditions(case, W, img):
    """The conditions a weight case must meet ON THE fp64 REFERENCE -> list of failures (empty = met); also returns the figures."""
    _, _, sv = chain(W, img, keep=True)
    fails, figs = [], {}
    if case == "peaked":
        for l in PEAKED_BLOCKS:
            rm = sv[l]["p"].max(-1).reshape(-1)
            med, share = float(np.median(rm)), float((rm > 1 - H16).mean())
            figs[f"block{l}"] = (med, share)
            if not med > 0.9:
                fails.append(f"block {l}: median row maximum {med:.3f} <= 0.9")
            if not share < 0.5:
                fails.append(f"block {l}: {share:.2f} of the rows are one-hot in fp16")
    if case == "outliers":
        mx = max(max(float(np.abs(s["pre"]).max()), float(np.abs(s["qkv"]).max())) for s in sv)
        figs["max"] = mx
        figs["xin_max"] = max(float(np.abs(s["xin"]).max()) for s in sv)
        if not mx < 6e4:
            fails.append(f"|pre| / |qkv| reaches {mx:.3g}: fp16 overflow")
    return fails, figs


# ---- comparator ------------------------------------------------------------------------------------------------------------------------------------
def check_forward(W, img, out, blocks=range(NL), rep=None, ends=True, nl=NL):
    """out: patches, pe, xemb, xin[12], xmid[12], qkv[12], pre[12], xfin, x0, feat, att_last, act_last - the kernels' buffers, logical rows only (nl: the number of
    blocks the buffers come from - the stand-in of tests/test_clip_ref.py can stop early; the kernels always run 12)."""
    rep = rep or Report("forward")
    if ends:
        rep.exact("patches", np.asarray(out["patches"], np.float32), patchify(img).astype(np.float32))
        rep.within("pe", out["pe"], *gemm(out["patches"], W["conv"]))
        rep.exact("xemb", out["xemb"], embed(out["pe"], W))
        rep.within("xin0", out["xin"][0], *ln_fwd(out["xemb"], W["ln_pre.weight"], W["ln_pre.bias"]))
        for k, (v, b) in tail_fwd(W, out["xfin"], out["x0"]).items():
            rep.within(k, out[k], v, b)
        # what the forward leaves in the att / act scratch: the last block's attention output and QuickGELU output, each one kernel from a stored input
        o, do, _ = attention_fwd(out["qkv"][nl - 1])
        rep.within("att", out["att_last"], o, do)
        a, da = quick_gelu(out["pre"][nl - 1])
        rep.within("act", out["act_last"], a, da + GELU_LIP * store16(out["pre"][nl - 1]) + store16(a))
    for l in blocks:
        st = block_fwd(W, l, out["xin"][l], out["xmid"][l], out["qkv"][l], out["pre"][l])
        nxt = out["xfin"] if l + 1 == nl else out["xin"][l + 1]
        for k, got in (("qkv", out["qkv"][l]), ("xmid", out["xmid"][l]), ("pre", out["pre"][l]), ("next", nxt)):
            rep.within("xin" if k == "next" else k, got, *st[k])
    return rep


def check_backward(W, g_feat, out, blocks=range(NL), rep=None, ends=True, nl=NL):
    """out: the forward's buffers and scale [2], g16, t0, dx_in[12] (dx_in[l]: the dx that entered block l; dx_in[11] is the head's), act[12],
    att[12], dqkv[12], t[12], dx0 (what block 0 left), y, dpatch, g_img."""
    rep = rep or Report("backward")
    B = np.shape(g_feat)[0]
    if ends:
        s, inv = loss_scale(g_feat)
        rep.exact("scale", out["scale"], np.array([s, inv], np.float32))
        rep.exact("g16", np.asarray(out["g16"], np.float32), r16(np.asarray(g_feat, np.float32) * np.float32(s)).astype(np.float32))
        hb = head_bwd(W, out["g16"], out["t0"], out["xfin"])
        rep.within("t0", out["t0"], *hb["t0"])
        rep.within("dx12", out["dx_in"][nl - 1], *hb["dx12"])
        tb, g = tail_bwd(W, out["dx0"], out["xemb"], out["y"], out["dpatch"], out["scale"])
        rep.within("y", out["y"], *tb["y"])
        rep.within("dpatch", out["dpatch"], *tb["dpatch"])
        rep.exact("g_img", out["g_img"], g)
    for l in blocks:
        st = block_bwd(W, l, out["dx_in"][l], out["xin"][l], out["xmid"][l], out["qkv"][l], out["pre"][l], out["act"][l], out["att"][l], out["dqkv"][l],
                       out["t"][l])
        dx_out = out["dx0"] if l == 0 else out["dx_in"][l - 1]
        for k, got in (("act", out["act"][l]), ("att", out["att"][l]), ("dqkv", out["dqkv"][l]), ("t", out["t"][l]), ("dx", dx_out)):
            rep.within("b_" + k, got, *st[k])
    if ends:
        zero = [b for b in range(B) if not np.asarray(g_feat)[b].any()]
        for b in zero:
            rep.check(not np.asarray(out["g_img"])[b].any(), f"g_img of image {b} is not exactly 0 although its cotangent is")
    return rep


def zero_share(out):
    """Share of the NON-ZERO entries of each block's incoming dx that round to zero as an fp16 GEMM operand (|v| <= 2^-25): what store16's absolute
    term is there for."""
    res = []
    for d in out["dx_in"]:
        a = np.abs(f64(d))
        res.append(float(((a > 0) & (a <= SUB16)).sum() / max(1, int((a > 0).sum()))))
    return res
