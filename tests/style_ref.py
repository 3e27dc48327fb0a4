"""fp64 references of the three kernels of csrc/style_heads.hip - k_resample_fwd, k_resample_bwd, k_clip_style_heads - with an error model, the case
matrix and a comparator.

Every function takes the kernel's own arguments (the Resample geometry, crop, win, affine, the stored fp32 arrays as float64 VALUES) and evaluates
ONE launch in float64 without any intermediate rounding; the roundings the kernel makes are part of the bound, not of the value.  No case and no
element is left out of any comparison.  tests/test_style_ref.py shows on the CPU that the references are torch's float64 F.pad / F.interpolate /
slicing chains and float64 autograd of the nerfart_amd.criteria formulas, that an fp32 stand-in of the kernels' data flow is accepted on the whole
matrix and that injected bugs are rejected; tests/test_gpu_style_stages.py holds the HIP kernels to it.

ERROR MODEL (u = 2^-24; first order in u; no fitted factor anywhere).  The project builds without -ffast-math (nerfart_amd/build.py), so +, -, *,
/ and sqrtf are correctly rounded (u relative each); hipcc may contract a * b + c to an FMA, which removes a rounding and never adds one.

  resample   Per axis the tap position is real = (in / out) (d + 0.5) - 0.5, here the exact rational.  Bicubic: A = -0.75, taps floor(real) - 1 .. + 2
  forward    with cubic2(x + 1), cubic1(x), cubic1(1 - x), cubic2(2 - x), no clamp of real; bilinear: real clamped at 0.  Indices clamp to the canvas
             (to the window with `win`); the canvas reads zeros outside the source; then the per-channel affine.  An axis is a matrix R [out, source],
             the value R_y S R_x^T.  The kernel computes real in fp32: fl(in / out) (u relative, 0 if the quotient is an fp32 number), the product
             (u, none under FMA), the subtraction (u |real|), x = real - floor(real) (u |x|):
                 dpos = (rs + u) (in / out) (d + 0.5) + u |real| + u x,   0 where in == out (every step is then exact).
             The interpolant is continuous in real across every integer, clamped borders and the zero padding included, so the position error moves
             the value by at most (Lipschitz constant) x dpos; the constant is sum_k D_k |s_k| over the taps of the cell, D = sup |w_k'| = 0.75, 1.35,
             1.35, 0.75 (bicubic) or 1, 1 (bilinear), and where real lies within dpos of an integer, the element-wise larger of the two cells'.
             The fp32 position is never reproduced.  Weights: the roundings of x + 1, 1 - x, 2 - x (u each, times D_k) and the running error of the
             Horner forms as the kernel writes them, sum_i u |t_i| (product of the later factors): cubic1's five and cubic2's six intermediates.
             Accumulation: a term w_y w_x s passes one product and <= 3 adds in its row, one product and <= 3 adds in the column: gamma_8 over
             sum |w_y| |w_x| |s|.  Affine: |a| bound + u |a v| + u |out|.
             Where in == out on both axes the fp32 weights are exactly 0 / 1 (cubic1(0) = 1, cubic2(1) = cubic2(2) = cubic1(1) = 0 in fp32); without
             an affine the output is compared bit for bit with the source.
  resample   Linear in the cotangent: prefill + J^T (a_c g), J from the forward's taps.  A contribution fl(fl(fl(a g) w_y) w_x) costs three products,
  backward   every atomic add one rounding of a running sum, in any order: gamma_{n + 3} over sum |contribution| with n the number of atomic adds the
             source pixel receives (taps of outputs with a g != 0), plus the weight and position terms above over |a g|, plus u |prefill|.  The
             prefill is charged ONE rounding: the worst case for a pixel with one non-zero add.  With n adds the worst case is n u |prefill|, which
             this model does not grant; gamma_{n + 3} charges the FULL sum |contribution| at every add where a running sum holds only part of it,
             and that slack covers the difference unless |prefill| is far above its contributions.  A pixel no tap reaches keeps the prefill's bits.
  heads      The kernel's own sequence of operations, run on (value, bound) pairs: r = a op b in float64 and
                 e_r = (first-order propagation of e_a, e_b through op) + u |r|.
             block sum  512 terms: 6 shuffle adds and the 8 wave partials, <= 14 roundings on any term (the product's own u is the product's):
                        e = sum e_j + 14 u sum |term_j|.
             unit       |f| = sqrt(block sum f^2) (the square root halves the relative error and adds u), fh = f / |f|.
             unit_bwd   (g - fh (fh . g)) / |f|: a block sum, a product, a difference, a quotient, each propagated as above; the cancellation of the
                        projection is paid in full because errors propagate over absolute values.
             loops      acc += term over t (or over the 1 + S text rows): a running sum in program order, e = sum e_t + u sum_{k >= 1} sum_{i <= k} |term_i|.
             hinge      relu(m - d) is 1-Lipschitz and the squared hinge is C^1: -2 h b / d is continuous through h = 0, so it is propagated without its
                        gate and the kernel and the reference may decide `ht > 0` differently at no cost.
             directional  unit(f0), unit(f1), e = fh0 - fh1, eh = e / |e| (a small |e| makes every bound downstream grow like 1 / |e|), cos = eh . d /
                        (max(|eh|, eps) max(|d|, eps)), d cos / d eh, two projections back to f0.
             contrastive  pd(x, y) = |x - y + 1e-6| with the TEXT ROWS RAW (not normalised); image hinge once, the T text terms in a running sum, / T.
             patchnce   text rows normalised inside the cosine.  c_k / tau, mx = max_k: lse = mx + log sum exp(c_k / tau - mx) does not depend on mx, so
                        mx is taken as an exact constant.  ASSUMPTION (the one tests/clip_ref.py states): v_exp_f32 and v_log_f32 are good to one ulp
                        (2 u).  __expf(z) = exp2(z log2 e): the rounded product moves the result by u |z| RELATIVE, the argument-dependent term (|z|
                        reaches 2 / tau); e = exp(z) (e_z + u |z| + 2 u) + 2^-126.  __logf(z) = log2(z) ln 2: e_z / z + 3 u |log z| + 2^-126.
             out4       out[1], out[2]: one atomic add to the zeroed word, exact.  out[3]: P adds, out[0]: 2 + P adds of w L (u each), any order:
                        sum e + (n - 1) u sum |term|.
             exact      rows 1 and 3 of g_feats are +0; out4 is overwritten (the entry point zeroes it); with S = 0 the PatchNCE value and gradient are
                        exactly 0 (lse == c0 / tau: exp(0) = 1, log(1) = 0).  Compared bit for bit.
The bounds are worst case (every rounding at its limit with the same sign) while real errors grow like the square root of the count: observed / bound
ratios of a few per cent are expected (tests/test_gpu_style_stages.py lists the measured ones).  A wrong index, a dropped term or constant is O(1).
"""
import numpy as np

from vgg_ref import Report, same_bits  # noqa: F401  (same_bits is re-exported for the tests)

U = 2.0 ** -24
TINY = 2.0 ** -126
FD = 512
A_CUBIC = -0.75
EPS_COS = float(np.float32(1e-8))
EPS_PD = float(np.float32(1e-6))
BSUM = 14                                   # roundings a term of a 512-term block sum passes: 6 shuffle adds + the 8 wave partials
D_CUBIC = (0.75, 1.35, 1.35, 0.75)          # sup |cubic2'| on [1, 2] = 0.75 (at 1), sup |cubic1'| on [0, 1] = 1.35 (at 0.6)
MODES = ("bicubic", "bilinear")
COT_KINDS = ("randn", "onehot_corner", "onehot_edge", "onehot_interior", "positive", "half_zero")
PREFILLS = ("zeros", "randn")
# The contrastive head's mixed margin.  Unit rows put every distance near sqrt 2 (far_text = sqrt(2 - 2 cos), cos ~ N(0, 1 / 512)).  Found on the CPU
# with the fp64 reference (active text hinges of 79; far_img):
#   "margin mixed a" (seed 7):   1.40: 27 (0.34)   1.41: 40 (0.51)   1.42: 52 (0.66);  far_img = 1.4206, the image hinge INACTIVE at all three
#   "margin mixed b" (seed 32):  1.40: 30 (0.38)   1.41: 35 (0.44)   1.42: 44 (0.56);  far_img = 1.3890, the image hinge ACTIVE at all three
# 1.41 is the middle of the range that meets both conditions.  tests/test_style_ref.py asserts the shares and both states of the image hinge.
MIXED_MARGIN = 1.41


def f64(x):
    return np.asarray(x, dtype=np.float64)


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- resample: one axis as matrices ------------------------------------------------------------------------------------------------------------
def cubic1(x, A=A_CUBIC):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def cubic2(x, A=A_CUBIC):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def cubic1_err(x, A=A_CUBIC):
    t1 = (A + 2.0) * x
    t2 = t1 - (A + 3.0)
    t3 = t2 * x
    t4 = t3 * x
    return U * (abs(t1) * x * x + abs(t2) * x * x + abs(t3) * x + abs(t4) + abs(t4 + 1.0))


def cubic2_err(x, A=A_CUBIC):
    t1 = A * x
    t2 = t1 - 5.0 * A
    t3 = t2 * x
    t4 = t3 + 8.0 * A
    t5 = t4 * x
    return U * (abs(t1) * x * x + abs(t2) * x * x + abs(t3) * x + abs(t4) * x + abs(t5) + abs(t5 - 4.0 * A))


def axis_ops(d0, nout, in_, out_, bicubic, pad, valid, off, full):
    """Outputs d0 .. d0 + nout - 1 of a size-`out_` axis resampled from a size-`in_` canvas whose entries pad .. pad + valid - 1 are the source
    entries off .. off + valid - 1 of a length-`full` axis (zeros elsewhere) -> [nout, full] matrices: R the weights, Ra their absolute values tap
    by tap, Re the bound of the weights' errors (roundings + Lipschitz x dpos), Cn the number of taps."""
    R, Ra, Re, Cn = (np.zeros((nout, full)) for _ in range(4))
    ratio = in_ / out_
    rs = 0.0 if float(np.float32(ratio)) == ratio else U

    def put(M, j, idx, val, accumulate=True):
        col = min(max(idx, 0), in_ - 1) - pad
        if 0 <= col < valid:
            M[j, off + col] = M[j, off + col] + val if accumulate else max(M[j, off + col], val)

    for j in range(nout):
        d = d0 + j
        num, den = in_ * (2 * d + 1) - out_, 2 * out_                     # real = num / den, exactly
        real = num / den
        fl = num // den
        x = (num - fl * den) / den
        if bicubic:
            dpos = 0.0 if in_ == out_ else (rs + U) * ratio * (d + 0.5) + U * abs(real) + U * x
            darg = 0.0 if x == 0.0 else U
            w = (cubic2(x + 1.0), cubic1(x), cubic1(1.0 - x), cubic2(2.0 - x))
            ew = (cubic2_err(x + 1.0) + D_CUBIC[0] * darg, cubic1_err(x), cubic1_err(1.0 - x) + D_CUBIC[2] * darg, cubic2_err(2.0 - x) + D_CUBIC[3] * darg)
            base, Dk = fl - 1, D_CUBIC
        else:
            if real < 0:
                fl, x = 0, 0.0
            if fl > in_ - 1:
                fl, x = in_ - 1, 1.0                                       # i1 == i0: the weight's split does not matter
            dpos = 0.0 if in_ == out_ else (rs + U) * ratio * (d + 0.5) + U * abs(real) + U * x
            w = (1.0 - x, x)
            ew = (0.0 if x in (0.0, 1.0) else U, 0.0)
            base, Dk = fl, (1.0, 1.0)
        for k in range(len(w)):
            put(R, j, base + k, w[k])
            put(Ra, j, base + k, abs(w[k]))
            put(Re, j, base + k, ew[k])
            put(Cn, j, base + k, 1.0)
        if dpos > 0.0:
            cells = [base] + ([base - 1] if x <= dpos else []) + ([base + 1] if 1.0 - x <= dpos else [])
            L = np.zeros((1, full))
            for b in cells:
                Lc = np.zeros((1, full))
                for k in range(len(Dk)):
                    put(Lc, 0, b + k, Dk[k] * dpos)
                L = np.maximum(L, Lc)
            Re[j] += L[0]
    return dict(R=R, Ra=Ra, Re=Re, Cn=Cn)


def resample_ops(case):
    """Per output image n: (source image, the y-axis matrices, the x-axis matrices, exact: in == out on both axes)."""
    if "_ops" in case:
        return case["_ops"]
    g, bic = case["geo"], case["mode"] == "bicubic"
    ops = []
    for n in range(g["N"]):
        y0, x0 = (int(case["crop"][n][0]), int(case["crop"][n][1])) if case["crop"] is not None else (0, 0)
        if case["win"] is not None:
            wy, wx, wh, ww = (int(v) for v in case["win"][n])
            ay = axis_ops(y0, g["Ho"], wh, g["Hr"], bic, 0, wh, wy, g["Hs"])
            ax = axis_ops(x0, g["Wo"], ww, g["Wr"], bic, 0, ww, wx, g["Ws"])
            same = wh == g["Hr"] and ww == g["Wr"]
        else:
            ay = axis_ops(y0, g["Ho"], g["Hp"], g["Hr"], bic, g["pad_t"], g["Hs"], 0, g["Hs"])
            ax = axis_ops(x0, g["Wo"], g["Wp"], g["Wr"], bic, g["pad_l"], g["Ws"], 0, g["Ws"])
            same = g["Hp"] == g["Hr"] and g["Wp"] == g["Wr"]
        ops.append((0 if g["n_src"] == 1 else n, ay, ax, same))
    case["_ops"] = ops
    return ops


def _sandwich(Ay, S, Ax):
    return np.einsum("yh,chw,xw->cyx", Ay, S, Ax)


def _sandwich_t(Ay, G, Ax):
    return np.einsum("yh,cyx,xw->chw", Ay, G, Ax)


def resample_fwd(case):
    """-> dict(val [N, C, Ho, Wo], bound, exact [N]: outputs that must equal the source's window bit for bit (val is then that copy))."""
    if "_fwd" in case:
        return case["_fwd"]
    g = case["geo"]
    src = f64(case["src"])
    val, bnd = np.zeros((g["N"], g["C"], g["Ho"], g["Wo"])), np.zeros((g["N"], g["C"], g["Ho"], g["Wo"]))
    exact = np.zeros(g["N"], bool)
    for n, (sn, ay, ax, same) in enumerate(resample_ops(case)):
        S = src[sn]
        v = _sandwich(ay["R"], S, ax["R"])
        b = gamma(8) * _sandwich(ay["Ra"], np.abs(S), ax["Ra"]) + _sandwich(ay["Re"], np.abs(S), ax["Ra"]) + _sandwich(ay["Ra"], np.abs(S), ax["Re"])
        if case["affine"] is not None:
            a, c = f64(case["affine"][0])[:, None, None], f64(case["affine"][1])[:, None, None]
            b = np.abs(a) * b + U * np.abs(a * v) + U * np.abs(a * v + c)
            v = a * v + c
        else:
            exact[n] = same
        val[n], bnd[n] = v, b
    case["_fwd"] = dict(val=val, bound=bnd, exact=exact)
    return case["_fwd"]


def resample_bwd(case, g_dst, prefill):
    """-> dict(val [n_src, C, Hs, Ws] = prefill + J^T (a g), bound, untouched: source pixels no atomic add reaches)."""
    g = case["geo"]
    gd, pre = f64(g_dst), f64(prefill)
    nz = (gd != 0)
    if case["affine"] is not None:
        a = f64(case["affine"][0])[:, None, None]
        gd = gd * a
        nz = nz & (a != 0)
    val, sab, werr, cnt = pre.copy(), np.zeros(pre.shape), np.zeros(pre.shape), np.zeros(pre.shape)
    for n, (sn, ay, ax, _) in enumerate(resample_ops(case)):
        G = np.abs(gd[n])
        val[sn] += _sandwich_t(ay["R"], gd[n], ax["R"])
        sab[sn] += _sandwich_t(ay["Ra"], G, ax["Ra"])
        werr[sn] += _sandwich_t(ay["Re"], G, ax["Ra"]) + _sandwich_t(ay["Ra"], G, ax["Re"])
        cnt[sn] += _sandwich_t(ay["Cn"], nz[n].astype(np.float64), ax["Cn"])
    bound = np.where(cnt > 0, gamma(cnt + 3.0) * sab + werr + U * np.abs(pre), 0.0)
    return dict(val=val, bound=bound, untouched=cnt == 0)


# ---- resample: cases (fixed by seeds alone) ----------------------------------------------------------------------------------------------------
def _rcase(name, mode, seed, n_src, C, Hs, Ws, Hr, Wr, N=None, Ho=None, Wo=None, pad=None, crop=None, win=None, affine=False):
    rng = np.random.default_rng([77, seed])
    pad_t, pad_l, Hp, Wp = pad if pad is not None else (0, 0, Hs, Ws)
    N = n_src if N is None else N
    geo = dict(n_src=n_src, C=C, Hs=Hs, Ws=Ws, pad_t=pad_t, pad_l=pad_l, Hp=Hp, Wp=Wp, Hr=Hr, Wr=Wr, N=N, Ho=Hr if Ho is None else Ho, Wo=Wr if Wo is None else Wo)
    src = rng.standard_normal((n_src, C, Hs, Ws)).astype(np.float32)
    aff = None
    if affine:                                       # distinct a_c, b_c per channel, one a_c negative
        aff = np.stack([rng.uniform(0.5, 4.0, C) * np.where(np.arange(C) == 1, -1.0, 1.0), rng.uniform(-2.0, 2.0, C)]).astype(np.float32)
    return dict(name=f"{name} {mode}", base=name, mode=mode, seed=seed, geo=geo, src=src, affine=aff,
                crop=None if crop is None else np.asarray(crop, np.int32).reshape(N, 2), win=None if win is None else np.asarray(win, np.int32).reshape(N, 4))


WINDOWS_11x14 = [(3, 4, 4, 6), (5, 7, 1, 1), (7, 9, 4, 5), (2, 3, 3, 9), (1, 10, 9, 3)]      # interior, 1 x 1, ending on the last row and column, 3 x 9, 9 x 3
CROPS_13x21 = [(0, 0), (8, 13), (8, 0), (3, 7)]                                              # (8, 13) is the far corner of 13 x 21 for 5 x 8 outputs


def resample_cases():
    out = []
    for mode in MODES:
        c = lambda name, *a, **k: out.append(_rcase(name, mode, len(out), *a, **k))  # noqa: E731
        c("ident c3", 1, 3, 6, 9, 6, 9)
        c("ident c3 affine", 1, 3, 6, 9, 6, 9, affine=True)
        c("ident c1", 1, 1, 6, 9, 6, 9)
        c("ident c1 affine", 1, 1, 6, 9, 6, 9, affine=True)
        c("up 7x5->17x11", 1, 3, 7, 5, 17, 11, affine=True)
        c("up 4x4->8x8", 1, 3, 4, 4, 8, 8)
        c("up 1x1->5x3", 1, 3, 1, 1, 5, 3)
        c("up 2x1->6x7", 1, 2, 2, 1, 6, 7, affine=True)
        c("down 23x17->9x5", 1, 3, 23, 17, 9, 5)
        c("pad->6x5", 1, 3, 6, 5, 6, 5, pad=(7, 2, 19, 12))
        c("pad->10x9", 1, 3, 6, 5, 10, 9, pad=(7, 2, 19, 12), affine=True)
        c("crops", 1, 3, 9, 10, 13, 21, N=4, Ho=5, Wo=8, crop=CROPS_13x21, affine=True)
        c("windows", 1, 3, 11, 14, 7, 8, N=5, win=WINDOWS_11x14, affine=True)
        c("windows ident", 1, 3, 11, 14, 4, 6, N=2, win=[(3, 4, 4, 6), (7, 8, 4, 6)])              # the full-resolution PatchNCE branch in small
        c("windows n_src=N", 2, 3, 11, 14, 7, 8, N=2, win=[(7, 9, 4, 5), (2, 3, 3, 9)])
        c("batch c4", 3, 4, 5, 6, 8, 7, affine=True)
    return out


_rcases = {}


def rcase(name):
    if not _rcases:
        _rcases.update({c["name"]: c for c in resample_cases()})
    return _rcases[name]


def rcase_names():
    rcase("ident c3 bicubic")
    return list(_rcases)


def cotangent(case, kind):
    g = case["geo"]
    shape = (g["N"], g["C"], g["Ho"], g["Wo"])
    rng = np.random.default_rng([78, case["seed"], COT_KINDS.index(kind)])
    if kind == "randn":
        c = rng.standard_normal(shape)
    elif kind == "positive":
        c = rng.uniform(0.25, 2.0, shape)
    elif kind == "half_zero":
        c = rng.standard_normal(shape)
        c.reshape(-1)[: c.size // 2] = 0.0
        c[..., ::2] *= (np.arange(shape[-2]) % 3 != 0)[:, None]          # and scattered zero runs in the other half
    else:                                            # one output pixel of the last image's last channel
        c = np.zeros(shape)
        y, x = {"onehot_corner": (g["Ho"] - 1, g["Wo"] - 1), "onehot_edge": (0, g["Wo"] // 2), "onehot_interior": (g["Ho"] // 2, g["Wo"] // 2)}[kind]
        c[g["N"] - 1, g["C"] - 1, y, x] = 1.0
    return c.astype(np.float32)


def prefill(case, kind):
    g = case["geo"]
    shape = (g["n_src"], g["C"], g["Hs"], g["Ws"])
    return np.zeros(shape, np.float32) if kind == "zeros" else np.random.default_rng([79, case["seed"]]).standard_normal(shape).astype(np.float32)


def check_resample_fwd(case, dst, rep=None, key="fwd"):
    rep = rep or Report(case["name"])
    r = resample_fwd(case)
    rep.within(key, dst, r["val"], r["bound"])
    for n in np.nonzero(r["exact"])[0]:
        rep.check(bool((r["val"][n] == r["val"][n].astype(np.float32)).all()), "the exact reference is not a copy of fp32 source values")
        rep.exact(f"{key}_exact", np.asarray(dst)[n], r["val"][n].astype(np.float32))
    return rep


def check_resample_bwd(case, g_dst, pre, got, rep=None, key="bwd"):
    rep = rep or Report(case["name"])
    r = resample_bwd(case, g_dst, pre)
    rep.within(key, got, r["val"], r["bound"])
    if r["untouched"].any():
        rep.check(same_bits(np.asarray(got)[r["untouched"]], np.asarray(pre)[r["untouched"]]), f"{key}: a source pixel no tap reaches lost the prefill's bits")
    return rep


# ---- heads: (value, bound) arithmetic ----------------------------------------------------------------------------------------------------------
class E:
    """A float64 value with a first-order bound of the kernel's error on it."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = f64(v), f64(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def _lin(self, o, sign):
        o = E.of(o)
        r = self.v + sign * o.v
        return E(r, self.e + o.e + U * np.abs(r))

    def __add__(self, o):
        return self._lin(o, 1.0)

    def __sub__(self, o):
        return self._lin(o, -1.0)

    def __mul__(self, o):
        o = E.of(o)
        r = self.v * o.v
        return E(r, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U * np.abs(r))

    def __truediv__(self, o):
        o = E.of(o)
        r = self.v / o.v
        return E(r, (self.e + np.abs(r) * o.e) / np.abs(o.v) + U * np.abs(r))

    def times_exact(self, c):                        # a power of two or a sign: no rounding
        return E(self.v * c, self.e * abs(c))

    def sqrt(self):
        r = np.sqrt(self.v)
        return E(r, self.e / (2.0 * r) + U * r)

    def at_least(self, c):                           # fmaxf(., c): 1-Lipschitz, no rounding
        return E(np.maximum(self.v, c), self.e)

    def expf(self):
        r = np.exp(self.v)
        return E(r, r * (self.e + U * np.abs(self.v) + 2.0 * U) + TINY)

    def logf(self):
        r = np.log(self.v)
        return E(r, self.e / np.abs(self.v) + 3.0 * U * np.abs(r) + TINY)

    def bsum(self):
        full = np.broadcast_to(self.e, self.v.shape)
        return E(self.v.sum(-1), full.sum(-1) + BSUM * U * np.abs(self.v).sum(-1))

    def seqsum(self, axis=0):
        """acc = 0; acc += term_k in program order (the first add is exact)."""
        a = np.moveaxis(np.abs(self.v), axis, 0)
        full = np.moveaxis(np.broadcast_to(self.e, self.v.shape), axis, 0)
        return E(self.v.sum(axis), full.sum(0) + U * np.cumsum(a, 0)[1:].sum(0))

    def __getitem__(self, i):
        return E(self.v[i], np.broadcast_to(self.e, self.v.shape)[i])


def _unit(f):
    f = E(f)
    nrm = (f * f).bsum().sqrt()
    return f / nrm[..., None], nrm


def _unit_bwd(g, fh, nrm):
    return (g - fh * (g * fh).bsum()[..., None]) / nrm[..., None]


def _atomic_sum(terms):
    v = sum(float(t.v) for t in terms)
    return E(v, sum(float(t.e) for t in terms) + max(len(terms) - 1, 0) * U * sum(abs(float(t.v)) for t in terms))


def heads(case):
    """-> dict(out4 = (value [4], bound [4]), g = (value [4 + P, 512], bound), exact0: rows of g_feats that are +0 bit for bit, nce_exact0: S == 0;
    and the reference's own intermediates: far_t [T], far_img, per-crop L)."""
    if "_ref" in case:
        return case["_ref"]
    P, S, T = case["P"], case["S"], case["T"]
    feats, tdir, t_tgt, t_con, t_neg = case["feats"], f64(case["text_dir"]), f64(case["t_tgt"]), f64(case["t_con"]), case["t_neg"]
    w_dir, w_con, w_nce = (float(np.float32(w)) for w in case["weights"])
    margin, tau = float(np.float32(case["margin"])), float(np.float32(case["tau"]))
    gv, ge = np.zeros((4 + P, FD)), np.zeros((4 + P, FD))
    # ---- directional
    f0, n0 = _unit(feats[0])
    f1, _ = _unit(feats[1])
    e = f0 - f1
    en = (e * e).bsum().sqrt()
    eh = e / en
    d = E(tdir)
    dn = (d * d).bsum().sqrt()
    ehn = (eh * eh).bsum().sqrt()
    dot = (eh * d).bsum()
    den = ehn.at_least(EPS_COS) * dn.at_least(EPS_COS)
    cosv = dot / den
    g_eh = (d / den - cosv * eh / (ehn * ehn).at_least(EPS_COS * EPS_COS)).times_exact(-1.0)
    g_e = (g_eh - eh * (g_eh * eh).bsum()) / en
    g0 = E(w_dir) * _unit_bwd(g_e, f0, n0)
    gv[0], ge[0] = g0.v, g0.e
    l_dir = E(1.0) - cosv
    # ---- contrastive
    f2, n2 = _unit(feats[2])
    f3, _ = _unit(feats[3])
    di = f2 - f3 + EPS_PD
    far_img = (di * di).bsum().sqrt()
    hi = (E(margin) - far_img).at_least(0.0)
    g_img = hi.times_exact(-2.0) * di / far_img                                     # exactly 0 where the hinge is off; C^1 through hi = 0
    a = E(f2.v[None, :], np.broadcast_to(f2.e, (FD,))[None, :]) - t_tgt + EPS_PD
    b = E(f2.v[None, :], np.broadcast_to(f2.e, (FD,))[None, :]) - t_con + EPS_PD
    near2, far_t = (a * a).bsum(), (b * b).bsum().sqrt()
    ht = (E(margin) - far_t).at_least(0.0)
    acc_l = (near2 + ht * ht).seqsum(0)
    per_t = (a.times_exact(2.0) + ht.times_exact(-2.0)[:, None] * b / far_t[:, None]) / float(T)
    g2 = E(np.concatenate([g_img.v[None], per_t.v]), np.concatenate([np.broadcast_to(g_img.e, (FD,))[None], np.broadcast_to(per_t.e, per_t.v.shape)])).seqsum(0)
    l_con = hi * hi + acc_l / float(T)
    g2 = E(w_con) * _unit_bwd(g2, f2, n2)
    gv[2], ge[2] = g2.v, g2.e
    # ---- PatchNCE
    l_nce, nce_terms = [], []
    for p in range(P):
        fp, npn = _unit(feats[4 + p])
        fn = (fp * fp).bsum().sqrt().at_least(EPS_COS)
        tv = E(np.concatenate([t_tgt[None], f64(t_neg).reshape(S, T, FD)]) if S else t_tgt[None])            # [1 + S, T, 512]
        fpb = E(fp.v[None, None, :], np.broadcast_to(fp.e, (FD,))[None, None, :])
        tn = (tv * tv).bsum().sqrt().at_least(EPS_COS)
        c = (fpb * tv).bsum() / (fn * tn)                                                                    # [1 + S, T]
        ct = c / tau
        mx = E(ct.v.max(0))                                                                                  # exact: lse does not depend on it
        lse = mx + (ct - mx).expf().seqsum(0).logf()
        L = ((lse - ct[0]) / float(T)).seqsum(0)
        k0 = np.zeros((1 + S, 1))
        k0[0] = 1.0
        sk = (ct - lse).expf() - k0
        dcos = tv / (fn * tn)[..., None] - c[..., None] * fpb / (fn * fn)
        gt = (sk[..., None] * dcos).seqsum(0)                                                                # [T, 512]
        gp = (gt / (E(tau) * float(T))).seqsum(0)
        g = E(w_nce) * _unit_bwd(gp, fp, npn)
        gv[4 + p], ge[4 + p] = g.v, g.e
        l_nce.append(L)
        nce_terms.append(E(w_nce) * L)
    total = _atomic_sum([E(w_dir) * l_dir, E(w_con) * l_con] + nce_terms)
    nce = _atomic_sum(l_nce)
    out_v = np.array([total.v, l_dir.v, l_con.v, nce.v], np.float64)
    out_e = np.array([total.e, l_dir.e, l_con.e, nce.e], np.float64)
    case["_ref"] = dict(out4=(out_v, out_e), g=(gv, ge), exact0=[1, 3] + (list(range(4, 4 + P)) if S == 0 else []), nce_exact0=S == 0,
                        far_t=far_t.v, far_img=float(far_img.v), l_crop=[float(L.v) for L in l_nce])
    return case["_ref"]


# ---- heads: cases ------------------------------------------------------------------------------------------------------------------------------
def _unit_rows(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _hcase(name, seed, P=12, S=8, T=79, margin=2.0, tau=0.07, weights=(1.0, 0.2, 0.1), scale=1.0, close=None, text_norms=False):
    rng = np.random.default_rng([91, seed])
    feats = rng.standard_normal((4 + P, FD)) * 3.0
    if close is not None:                            # row `close` at an angle of 1e-2 from row close + 1
        a, b = close, close + 1
        perp = rng.standard_normal(FD)
        u = _unit_rows(feats[b])
        perp = _unit_rows(perp - u * (perp @ u))
        feats[a] = np.linalg.norm(feats[a]) * (np.cos(1e-2) * u + np.sin(1e-2) * perp)
    feats = (feats * scale).astype(np.float32)
    tdir, t_tgt, t_con = _unit_rows(rng.standard_normal(FD)), _unit_rows(rng.standard_normal((T, FD))), _unit_rows(rng.standard_normal((T, FD)))
    t_neg = _unit_rows(rng.standard_normal((S, T, FD)))
    if text_norms:                                   # rows of norm 0.5 .. 2: the contrastive head uses them raw, PatchNCE normalises them
        t_tgt, t_con = t_tgt * rng.uniform(0.5, 2.0, (T, 1)), t_con * rng.uniform(0.5, 2.0, (T, 1))
        t_neg = t_neg * rng.uniform(0.5, 2.0, (S, T, 1))
    return dict(name=name, P=P, S=S, T=T, margin=margin, tau=tau, weights=weights, feats=feats, text_dir=tdir.astype(np.float32), t_tgt=t_tgt.astype(np.float32),
                t_con=t_con.astype(np.float32), t_neg=t_neg.astype(np.float32) if S else None)


def heads_cases():
    return [
        _hcase("base 12,8,79", 0),
        _hcase("shape 0,0,1", 1, P=0, S=0, T=1),
        _hcase("shape 1,1,2", 2, P=1, S=1, T=2),
        _hcase("shape 16,16,5", 3, P=16, S=16, T=5),
        _hcase("shape 16,0,3", 4, P=16, S=0, T=3),
        _hcase("shape 3,16,79", 5, P=3, S=16, T=79),
        _hcase("margin 0", 6, margin=0.0),
        _hcase("margin mixed a", 7, margin=MIXED_MARGIN),
        _hcase("margin mixed b", 32, margin=MIXED_MARGIN),
        _hcase("tau 0.01", 9, tau=0.01),
        _hcase("weights 0.3,0,2", 10, P=3, weights=(0.3, 0.0, 2.0)),
        _hcase("weights 0,1,0", 11, P=3, weights=(0.0, 1.0, 0.0)),
        _hcase("scale 1e-3", 12, P=3, scale=1e-3),
        _hcase("scale 1e3", 13, P=3, scale=1e3),
        _hcase("close 0,1", 14, P=2, close=0),
        _hcase("close 2,3", 15, P=2, close=2, margin=MIXED_MARGIN),
        _hcase("text norms", 16, P=3, text_norms=True),
        _hcase("text norms small", 17, P=2, S=3, T=5, text_norms=True, tau=0.01, margin=MIXED_MARGIN),
    ]


_hcases = {}


def hcase(name):
    if not _hcases:
        _hcases.update({c["name"]: c for c in heads_cases()})
    return _hcases[name]


def hcase_names():
    hcase("base 12,8,79")
    return list(_hcases)


def check_heads(case, out4, g_feats, rep=None, key=""):
    """out4 [4] and g_feats [4 + P, 512] as the kernel left them (out4 prefilled with NaN by the caller: it must have been overwritten)."""
    rep = rep or Report(case["name"])
    r = heads(case)
    out4, g_feats = np.asarray(out4), np.asarray(g_feats)
    rep.within("out4" + key, out4, *r["out4"])
    rep.within("g" + key, g_feats, *r["g"])
    rows = r["exact0"]
    rep.check(same_bits(g_feats[rows], np.zeros((len(rows), FD), np.float32)), f"g_feats rows {rows} are not +0 bit for bit")
    if r["nce_exact0"]:
        rep.check(same_bits(out4[3:4], np.zeros(1, np.float32)), f"S = 0: the PatchNCE value is {out4[3]!r}, not exactly 0")
    return rep
