"""fp64 references, fp32 stand-ins and comparators of the six kernels of csrc/pass2_operands.hip: k_ray_points, k_volsdf_cotangents and the four
k_operand_* (nerfart_ray_points, nerfart_volsdf_pass2_cotangents, nerfart_wgrad_operand_embed_pair / _inputs / _rgb_delta / _sbar_ones).

tests/test_pass2_operand_ref.py shows on the CPU that the comparators accept the clean stand-ins and reject each stand-in with one injected fault;
tests/test_gpu_pass2_operands_fp64.py holds the HIP kernels to the same comparators on the same cases.  numpy, fp64 (torch only for the autograd
reference of the eikonal term).  Every comparator appends its lines to REPORT and returns (violations, {output: worst observed / allowed}).

BF16 OPERANDS: INTERVALS, NOT TOLERANCES.  Round to nearest even is monotone, so for a column whose fp32 value the kernel computes within E of the
fp64 value r
    bf16(fl32(r - E)) <= hi <= bf16(fl32(r + E))      and, with the kernel's OWN hi,      bf16(fl32(r - E) - hi) <= lo <= bf16(fl32(r + E) - hi)
(x - hi is exact in fp32; the order is the one of the bit patterns as sign-magnitude numbers, so -0 < +0 and E = 0 is bit equality).  No share of
the entries is left out.  The figure reported for such an output is the smallest fraction t of E with which every interval still holds (0: every hi
and lo is the rounding of the fp64 value itself).
    E = 0            the identity columns k < 3 of every embedding (value and tangent), every column when multires < 0, the normals, sbar, the
                     rgb_delta operand against the fp32 d4 the same call returned; the ones rows are bits 0x3f80 in column 0 and 0x0000 elsewhere
    sin / cos        r = sin or cos in fp64 of the exact product 2^k x;  E = 4 ulp32(r) + 2^-31: the 4-ulp limit the device math library is built
                     to, and an absolute floor for the range reduction at |2^k x| <= 2^11, which matters only where |r| < 2^-15
    tangent          cos(2^k x) (2^k d), -sin(2^k x) (2^k d):  E = (4 ulp32(trig) + 2^-31) |2^k d| + 2^-24 |r| (the one multiplication; 2^k d is exact)
Every column the layout leaves empty, and every row at or above M, is 0x0000.

FP32 OUTPUTS.
    d4          |d4 - g c (1 - c)| <= 3 2^-24 |ref|: the three roundings of (g * c) * (1 - c), no fma form
    block_sums  against the fp64 sum of the RETURNED d4 over rows 32 b .. 32 b + 31 below M: 32 2^-24 sum |d4|; a block wholly at or above M is +0
    pts         the bits of numpy float32 o + (d * t) (two roundings);  view: the bits of d
    sbar        exactly 0.0 or exactly the bits of g_sdf.  Decided by the fp64 margin m = s - (R_bg - |x|) + 1e-6:  m > eps: 0,  m < -eps: g_sdf,
                either inside;  eps = 2^-23 (1.75 |x| + |R_bg - |x|| + 1e-6) (three roundings in the sum of squares halved by the root, up to 2 ulp
                of sqrtf, one rounding per subtraction).  R_bg <= 0: always g_sdf
    nbar        against torch's fp64 autograd of w sum_patches mean_patch((|n| - 1)^2), plus g_n and g_n_extra.  Per element, with u = 2^-24, e the
                eikonal term and coef = 1 / (rays of the patch * P):
                    B = u (2 |g_n| + |g_n_extra| + 7 |e|) + 7 u w coef |n_c| / |n|,      A = FACTOR B.
                B counts every rounding of the fp32 route at its worst: the fmaf's on |e| + |g_n| and the last add's on the whole sum; 1 / (n P),
                (2 w) coef, times err, over |n| and the subtraction |n| - 1 (5 u |e|); and |n| itself - 3 u in the sum of squares halved by the
                root, one ulp = 2 u for sqrtf: 3.5 u |n| - through d e_c / d |n| = 2 w coef n_c / |n|^2.  At n = 0 the autograd gives 0 and the
                last summand is 0.
                DERIVED AGAIN.  The first allowance was A1 = 2^-23 (|g_n| + |g_n_extra| + 4 |e|) + 2 w coef 4 2^-24 |n_c|: about B itself (and
                without the 1 / |n| of the last summand).  The last rounding alone can take half of its first term, and the stand-in reached 0.33
                to 0.74 of A1 on the cases of this module (0.40 with both optional cotangents NULL) where 1 / FACTOR was required: A1 was a count
                of the roundings, not FACTOR times it.  A = FACTOR B is the same count, completed, times the factor every sibling module leaves
                between the fp32 route and the kernel; it comes from the list above alone.  Nothing is given up by it: check_cotangents holds
                every element to A1 as well (reported as nbar_first_A), so a kernel passes only inside min(A, A1); A is what the 1 / FACTOR
                assertion on the stand-in is made against.
    eik_ray     per ray:  A = w coef sum_p (2^-22 |n_p| ||n_p| - 1| + (P / 64 + 8) 2^-24 (|n_p| - 1)^2)
w is the fp32 value the C ABI passes.  standin_cotangents is k_volsdf_cotangents operation by operation in numpy float32 (its fmaf through one fp64
product and sum); tests/test_pass2_operand_ref.py asserts that it sits at or below 1 / FACTOR of A on every element and ray of every case.

INPUTS (the case makers).  Points in the ball |x| <= 2.2.  The first rows of every input that feeds an exact column carry the CRAFT values: a lo
half that truncation and rounding split differently, the two ties (low half 0x8000 under an even and an odd upper half), 0x3F7FFFFF (the rounding
carries into the exponent), -0.0, an fp32 denormal and +-3e38 - the last two only where no 2^k and no sin / cos touches them (multires < 0, normals,
sbar, g_sdf), +-1.25 elsewhere: the inputs times 2^k must stay finite.  No inf, no NaN.  For the clamp: class 0 the net clearly below the sphere,
class 1 the sphere branch as pass 1 produces it (s = min(net, R_bg - |x|) in numpy float32, net 0.01 .. 0.3 above), class 2 points placed inside the
band (at most 2 % of a case).  Nablas whose squares underflow fp32 are out of scope.
"""
import functools

import numpy as np
import torch

from mlp_bwd_ref import FACTOR, FILL

F32, F64 = np.float32, np.float64
REPORT = []
FILL16 = FILL * 0x0101

M_SIZES = (1, 31, 32, 33, 255, 257)
EMBED_MULTIRES = (-1, 0, 1, 4, 5, 6, 10)
INPUT_MULTIRES = ((-1, -1), (-1, 3), (-1, 4), (2, 1), (4, 4), (-1, 9))       # 9, 27, 33, 27, 57, 63 columns
RAY_SIZES = ((1, 1), (5, 13), (7, 64), (7, 65), (3, 192))
W_EIK = (0.1, 0.0)
R_BGS = (3.0, 0.0)
BALL = 2.2


def up(n, m):
    return (n + m - 1) // m * m


def rows_pads(M):
    return sorted({M, M + 1, up(M, 64), up(M, 128)})


def groups(R):
    return sorted({0, 1, 2, 3, R, R + 1})


def width(multires):
    return 3 if multires < 0 else 3 + 6 * multires


# ---- bf16 -----------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x, mode="rne"):
    """fp32 -> bf16 bit patterns (uint16).  mode 'rne' (the kernel), 'away' (ties away from zero), 'trunc': the last two for the mutants."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    if mode == "rne":
        u = u + 0x7FFF + ((u >> 16) & 1)
    elif mode == "away":
        u = u + 0x8000
    return ((u >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(b):
    return (np.asarray(b).astype(np.uint32) << 16).view(F32)


def _key(b):
    """bf16 bits as sign-magnitude integers: monotone in the value, -0 below +0."""
    b = np.asarray(b).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF) - 1, b)


def ulp32(r):
    return np.spacing(np.abs(np.asarray(r, dtype=F64)).astype(F32)).astype(F64)


def _inside(hi, lo, r, E, t):
    """-> (ok_hi, ok_lo) boolean arrays of the interval conditions with t E."""
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = (r - t * E).astype(F32), (r + t * E).astype(F32)
        kh = _key(hi)
        ok_hi = (_key(bf16_bits(a)) <= kh) & (kh <= _key(bf16_bits(b)))
        if lo is None:
            return ok_hi, None
        hv = bf16_value(hi).astype(F64)
        la, lb = (a.astype(F64) - hv).astype(F32), (b.astype(F64) - hv).astype(F32)
        kl = _key(lo)
        return ok_hi, (_key(bf16_bits(la)) <= kl) & (kl <= _key(bf16_bits(lb)))


def check_block(who, name, got, r, E, split, viol, args=None):
    """got uint16 [rows, 64] against fp64 columns r, E [M, c]: rows < M by intervals, every other entry 0x0000.  Appends to viol with the output's
    name (name, or 'pad' for what must be zero) -> the smallest fraction of E that explains the block."""
    M, c = r.shape
    rows = got.shape[0]
    hi = got[:M, :c]
    lo = got[:M, 32:32 + c] if split else None
    zero = np.ones((rows, 64), dtype=bool)
    zero[:M, :c] = False
    if split:
        zero[:M, 32:32 + c] = False
    bad = zero & (got != 0)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        viol.append(f"{who} pad: {int(bad.sum())} entries that must be 0x0000 are not, first at row {i} column {j}: 0x{int(got[i, j]):04x}")
    if M == 0:
        return 0.0

    def ok(t):
        h, l = _inside(hi, lo, r, E, t)
        return h, l, bool(h.all()) and (l is None or bool(l.all()))

    h, l, fine = ok(1.0)
    if not fine:
        for part, o, g in (("hi", h, hi), ("lo", l, lo)):
            if o is not None and not o.all():
                i, j = np.argwhere(~o)[0]
                arg = "" if args is None else f", argument {args(i, j)}"
                viol.append(f"{who} {name}: {int((~o).sum())} {part} entries outside their interval, first at row {i} column {j}: 0x{int(g[i, j]):04x}, "
                            f"fp64 value {r[i, j]!r}, E {E[i, j]:.3e}{arg}")
        t = 1.0
        while t < 64.0 and not ok(t)[2]:
            t *= 2.0
        return t
    if ok(0.0)[2]:
        return 0.0
    a, b = 0.0, 1.0
    for _ in range(8):
        m = 0.5 * (a + b)
        a, b = (a, m) if ok(m)[2] else (m, b)
    return b


# ---- the encoding ---------------------------------------------------------------------------------------------------------------------------
def embed_ref(x, d, multires, tangent):
    """fp64 columns and their E: x, d fp32 [M, 3] -> (r [M, c], E [M, c])."""
    x64, d64 = x.astype(F64), d.astype(F64)
    M, c = x.shape[0], width(multires)
    r, E = np.zeros((M, c)), np.zeros((M, c))
    r[:, :3] = d64 if tangent else x64
    for k in range(max(multires, 0)):
        f = 2.0 ** k
        s, co = np.sin(x64 * f), np.cos(x64 * f)
        es, ec = 4 * ulp32(s) + 2.0 ** -31, 4 * ulp32(co) + 2.0 ** -31
        j = 3 + 6 * k
        if not tangent:
            r[:, j:j + 3], r[:, j + 3:j + 6] = s, co
            E[:, j:j + 3], E[:, j + 3:j + 6] = es, ec
        else:
            df = d64 * f
            r[:, j:j + 3], r[:, j + 3:j + 6] = co * df, -s * df
            E[:, j:j + 3] = ec * np.abs(df) + 2.0 ** -24 * np.abs(co * df)
            E[:, j + 3:j + 6] = es * np.abs(df) + 2.0 ** -24 * np.abs(s * df)
    return r, E


def _trig32(fn, a32):
    return fn(a32.astype(F64)).astype(F32)              # the fp32 argument is exact; one rounding of the fp64 result


def embed_sim(x, d, multires, tangent, bug=None):
    """embed_col of the kernel in fp32 -> [M, c] fp32."""
    out = [d if tangent else x]
    perm = [1, 2, 0] if bug == "axes_perm" else [0, 1, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(max(multires, 0)):
            f = F32(2.0 ** (k + 1 if bug == "octave_x2" else k))
            xf = x[:, perm] * f
            s, co = _trig32(np.sin, xf), _trig32(np.cos, xf)
            if bug == "sincos_swap":
                s, co = co, s
            if not tangent:
                out += [s, co]
            else:
                df = d[:, perm] * (F32(1.0) if bug == "tan_no_factor" else f)
                out += [co * df, (s if bug == "tan_minus_dropped" else -s) * df]
    return np.concatenate(out, axis=1).astype(F32)


def pack(cols, rows, row0, out, bug=None):
    """pack8 over the rows [row0, row0 + M) of out (uint16 [*, 64]): hi in columns 0..c-1, lo at +32 when c <= 32, the rest 0x0000."""
    M, c = cols.shape
    split = c <= 32
    if bug == "split33":
        split = c <= 33
    if bug == "nosplit27":
        split = c < 27
    blk = np.zeros((M, 64), dtype=np.uint16)
    if bug == "negzero_pad":
        blk[:] = 0x8000
    hi = bf16_bits(cols, "away" if bug == "hi_away" else "rne")
    blk[:, :c] = hi
    if split:
        with np.errstate(over="ignore", invalid="ignore"):
            lo = bf16_bits(cols - bf16_value(hi), "trunc" if bug == "lo_trunc" else "rne")
        at = c if bug == "lo_at_c" else 32
        blk[:, at:at + c] = lo[:, :min(c, 64 - at)]
    out[row0:row0 + M] = blk


def _blank(rows, M_rows, bug):
    """The output buffer as the kernel leaves it before the data rows: 0x0000 everywhere (bug 'rows_left': the rows the kernel owes a zero keep the fill)."""
    out = np.zeros((rows, 64), dtype=np.uint16)
    if bug == "rows_left":
        out[:] = FILL16
    return out


def standin_embed_pair(c, rows_pad, bug=None):
    M, mr = c["M"], c["multires"]
    out = _blank(2 * rows_pad, M, bug)
    pack(embed_sim(c["pts"], c["dir"], mr, False, bug), 2 * rows_pad, 0, out, bug)
    t0 = M if bug == "tangent_at_M" else rows_pad
    pack(embed_sim(c["pts"], c["dir"], mr, True, bug), 2 * rows_pad, t0, out, bug)
    return out


def check_embed_pair(c, rows_pad, got):
    M, mr, who = c["M"], c["multires"], f"embed_pair M={c['M']} rows_pad={rows_pad} multires={c['multires']}"
    viol, ratio = [], {}
    if got.shape != (2 * rows_pad, 64):
        return [f"{who} value: shape {got.shape}"], ratio
    split = width(mr) <= 32
    for name, tangent, row0 in (("value", False, 0), ("tangent", True, rows_pad)):
        r, E = embed_ref(c["pts"], c["dir"], mr, tangent)
        arg = lambda i, j: f"2^{(j - 3) // 6} * {float(c['pts'][i, (j - 3) % 3])!r}" if j >= 3 else "-"
        ratio[name] = check_block(who, name, got[row0:row0 + rows_pad], r, E, split, viol, arg)
    return _done(who, viol, ratio)


def _done(who, viol, ratio):
    REPORT.append(f"{who}: " + "  ".join(f"{k} {v:.3g}" for k, v in ratio.items()) + (f"  VIOLATIONS {len(viol)}" if viol else ""))
    return viol, ratio


def inputs_ref(c):
    rx, Ex = embed_ref(c["x"], c["x"], c["mx"], False)
    rv, Ev = embed_ref(c["view"], c["view"], c["mv"], False)
    return np.concatenate([rx, rv, c["normals"].astype(F64)], 1), np.concatenate([Ex, Ev, np.zeros((c["M"], 3))], 1)


def standin_inputs(c, rows_pad, bug=None):
    M = c["M"]
    ex = embed_sim(c["x"], c["x"], c["mx"], False, bug)
    v = c["x"] if bug == "view_from_x" else c["view"]
    ev = embed_sim(v, v, c["mv"], False, bug)
    n = c["normals"]
    if bug == "normals_off":
        n = np.concatenate([np.zeros((M, 1), F32), n], 1)
    cols = np.concatenate([ex, ev, n], 1)
    out = _blank(rows_pad, M, bug)
    if bug == "normals_off":                     # columns 0 .. c-1 = [ex | ev | 0, n0, n1], n2 spills into column c; the split stays the true width's
        cw = cols.shape[1] - 1
        blk = np.zeros((M, 64), dtype=np.uint16)
        pack(cols[:, :cw], M, 0, blk)
        hi = bf16_bits(cols[:, cw])
        blk[:, cw] = hi
        if cw <= 32:
            blk[:, 32 + cw] = bf16_bits(cols[:, cw] - bf16_value(hi))
        out[:M] = blk
    else:
        pack(cols, rows_pad, 0, out, bug)
    return out


def check_inputs(c, rows_pad, got):
    who = f"inputs M={c['M']} rows_pad={rows_pad} multires=({c['mx']}, {c['mv']})"
    viol, ratio = [], {}
    if got.shape != (rows_pad, 64):
        return [f"{who} inputs: shape {got.shape}"], ratio
    r, E = inputs_ref(c)
    ratio["inputs"] = check_block(who, "inputs", got, r, E, r.shape[1] <= 32, viol)
    return _done(who, viol, ratio)


# ---- rgb delta, [sbar; 1] ---------------------------------------------------------------------------------------------------------------------
def standin_rgb_delta(c, rows_pad, bug=None):
    """-> (out uint16 [rows_pad, 64], d4 fp32 [M, 3], block_sums fp32 [ceil(rows_pad / 32), 3]).  The sums in the kernel's order: 8 rows per wave
    through the xor butterfly, then (w0 + w1) + (w2 + w3)."""
    M = c["M"]
    rgb, g = c["rgb"], c["g_rgb"]                              # rows beyond M exist for the 'sums_rows_ge_M' mutant only
    with np.errstate(over="ignore", invalid="ignore"):
        d_all = ((g * rgb) * (F32(1.0) - rgb)).astype(F32)
    d4 = d_all[:M].copy()
    out = _blank(rows_pad, M, bug)
    pack(d4, rows_pad, 0, out, bug)
    nb = (rows_pad + 31) // 32
    src = np.zeros((nb * 32, 3), F32)
    lim = min(rows_pad, d_all.shape[0]) if bug == "sums_rows_ge_M" else M
    src[:lim] = d_all[:lim]
    w = src.reshape(nb, 4, 8, 3)
    for o in (4, 2, 1):                                       # lanes 8 rows apart: xor 32, 16, 8 of the lane index = 4, 2, 1 of the row in the wave
        w = w + w[:, :, np.arange(8) ^ o, :]
    part = w[:, :, 0, :]
    sums = ((part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])).astype(F32)
    if bug == "sums_grand_total":
        tot = sums.sum(0, dtype=F32)
        sums = np.zeros_like(sums)
        sums[0] = tot
    return out, d4, sums


def check_rgb_delta(c, rows_pad, out, d4, sums):
    """d4 None: the call was made with d4 = NULL; the operand is then held to the reference's own fp32 d4 interval and the sums to the fp64 d4."""
    M, who = c["M"], f"rgb_delta M={c['M']} rows_pad={rows_pad}"
    viol, ratio = [], {}
    nb = (rows_pad + 31) // 32
    if out.shape != (rows_pad, 64) or sums.shape != (nb, 3) or (d4 is not None and d4.shape != (M, 3)):
        return [f"{who} operand: shapes {out.shape} {sums.shape}"], ratio
    ref = (c["g_rgb"][:M].astype(F64) * c["rgb"][:M].astype(F64)) * (1.0 - c["rgb"][:M].astype(F64))
    A = 3 * 2.0 ** -24 * np.abs(ref)
    if d4 is not None:
        if not np.isfinite(d4).all():
            viol.append(f"{who} d4: non-finite")
        err = np.abs(d4.astype(F64) - ref)
        ratio["d4"] = _ratio(err, A)
        if (err > A).any():
            i = int(np.argmax(err - A))
            viol.append(f"{who} d4: |d4 - ref| = {err.flat[i]:.3e} > {A.flat[i]:.3e} at flat index {i}")
        ratio["operand"] = check_block(who, "operand", out, d4.astype(F64), np.zeros((M, 3)), True, viol)
        base = d4.astype(F64)
    else:
        ratio["operand"] = check_block(who, "operand", out, ref, A, True, viol)
        base = ref
    pad = np.zeros((nb * 32, 3))
    pad[:M] = base
    want = pad.reshape(nb, 32, 3).sum(1)
    allow = 32 * 2.0 ** -24 * np.abs(pad).reshape(nb, 32, 3).sum(1) + (0 if d4 is not None else np.abs(np.pad(A, ((0, nb * 32 - M), (0, 0)))).reshape(nb, 32, 3).sum(1))
    if not np.isfinite(sums).all():
        viol.append(f"{who} block_sums: non-finite")
    err = np.abs(sums.astype(F64) - want)
    ratio["block_sums"] = _ratio(err, allow)
    if (err > allow).any():
        i = int(np.argmax(err - allow))
        viol.append(f"{who} block_sums: |sum - ref| = {err.flat[i]:.3e} > {allow.flat[i]:.3e} at block {i // 3} column {i % 3}")
    empty = np.arange(nb) * 32 >= M
    if (sums[empty].view(np.uint32) != 0).any():
        viol.append(f"{who} block_sums: a block wholly at or above M is not +0")
    return _done(who, viol, ratio)


def _ratio(err, A):
    """max err / A with 0 / 0 = 0 and x / 0 = inf."""
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / A)
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max())


def standin_sbar_ones(c, rows_pad, bug=None):
    M = c["M"]
    out = _blank(2 * rows_pad, M, bug)
    pack(c["sbar"][:, None], 2 * rows_pad, 0, out, bug)
    out[rows_pad:] = 0x8000 if bug == "negzero_pad" else 0
    out[rows_pad:, 1 if bug == "ones_col1" else 0] = 0x3F80
    return out


def check_sbar_ones(c, rows_pad, got):
    M, who = c["M"], f"sbar_ones M={c['M']} rows_pad={rows_pad}"
    viol, ratio = [], {}
    if got.shape != (2 * rows_pad, 64):
        return [f"{who} sbar: shape {got.shape}"], ratio
    ratio["sbar"] = check_block(who, "sbar", got[:rows_pad], c["sbar"][:, None].astype(F64), np.zeros((M, 1)), True, viol)
    ones = np.zeros((rows_pad, 64), dtype=np.uint16)
    ones[:, 0] = 0x3F80
    bad = got[rows_pad:] != ones
    ratio["ones"] = float("inf") if bad.any() else 0.0
    if bad.any():
        i, j = np.argwhere(bad)[0]
        viol.append(f"{who} ones: {int(bad.sum())} entries differ from [0x3f80, 0, ...], first at row {i} column {j}: 0x{int(got[rows_pad + i, j]):04x}")
    return _done(who, viol, ratio)


# ---- ray points -----------------------------------------------------------------------------------------------------------------------------
def standin_ray_points(c, bug=None):
    o, d, t = c["o"][:, None, :], c["dn"][:, None, :], c["depth"][:, :, None]
    if bug == "fused":
        pts = (o.astype(F64) + d.astype(F64) * t.astype(F64)).astype(F32)        # the product is exact in fp64: one rounding (up to a double rounding)
    else:
        pts = o + (d * t).astype(F32)
    return pts.reshape(-1, 3).astype(F32), np.broadcast_to(d, pts.shape).reshape(-1, 3).copy()


def check_ray_points(c, pts, view):
    who = f"ray_points R={c['R']} P={c['P']}"
    want, wview = standin_ray_points(c)
    viol, ratio = [], {}
    for name, got, w in (("pts", pts, want), ("view", view, wview)):
        if got is None:
            continue
        if got.shape != w.shape:
            viol.append(f"{who} {name}: shape {got.shape}")
            continue
        bad = got.view(np.uint32) != w.view(np.uint32)
        ratio[name] = float("inf") if bad.any() else 0.0
        if bad.any():
            viol.append(f"{who} {name}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at flat index {int(np.argmax(bad))}")
    return _done(who, viol, ratio)


def fused_share(c):
    a, b = standin_ray_points(c)[0], standin_ray_points(c, "fused")[0]
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


# ---- cotangents -----------------------------------------------------------------------------------------------------------------------------
def patch_sizes(R, group):
    """rays in the reference patch of each ray -> int64 [R]."""
    g = R if (group <= 0 or group > R) else group
    n = np.full(R, g, dtype=np.int64)
    tail = R % g
    if tail:
        n[R - tail:] = tail
    return n


def clamp_margin(c, R_bg):
    x = np.linalg.norm(c["pts"].astype(F64), axis=1)
    m = c["sdf"].astype(F64) - (R_bg - x) + 1e-6
    eps = 2.0 ** -23 * (1.75 * x + np.abs(R_bg - x) + 1e-6)
    return m, eps


def cot_ref(c, group, w, use_gn, use_extra, R_bg):
    """-> dict of the fp64 references and allowances of one call."""
    R, P = c["R"], c["P"]
    w = float(F32(w))
    coef = np.repeat(1.0 / (patch_sizes(R, group) * float(P)), P) if w else np.zeros(R * P)
    n = torch.from_numpy(c["nabla"].astype(F64)).requires_grad_(True)
    loss = (torch.from_numpy(coef) * (n.norm(dim=-1) - 1.0) ** 2).sum() * w         # each patch's mean, summed over the patches
    e = torch.autograd.grad(loss, n)[0].numpy() if w else np.zeros((R * P, 3))
    gn = c["g_n"].astype(F64) if use_gn else np.zeros((R * P, 3))
    ge = c["g_n_extra"].astype(F64) if use_extra else np.zeros((R * P, 3))
    nn = np.linalg.norm(c["nabla"].astype(F64), axis=1)
    u, n64 = 2.0 ** -24, c["nabla"].astype(F64)
    A_first = 2 * u * (np.abs(gn) + np.abs(ge) + 4 * np.abs(e)) + (2 * w * coef * 4 * u)[:, None] * np.abs(n64)
    unit = np.divide(np.abs(n64), nn[:, None], out=np.zeros_like(n64), where=nn[:, None] > 0)
    A_n = FACTOR * (u * (2 * np.abs(gn) + np.abs(ge) + 7 * np.abs(e)) + (7 * u * w * coef)[:, None] * unit)
    err2 = (nn - 1.0) ** 2
    eik = w * coef.reshape(R, P)[:, 0] * err2.reshape(R, P).sum(1)
    A_e = w * coef.reshape(R, P)[:, 0] * (2.0 ** -22 * nn * np.abs(nn - 1.0) + (P / 64.0 + 8) * 2.0 ** -24 * err2).reshape(R, P).sum(1)
    out = dict(nbar=gn + ge + e, A_nbar=A_n, A_nbar_first=A_first, eik_ray=eik, A_eik=A_e, e=e)
    if R_bg > 0:
        m, eps = clamp_margin(c, R_bg)
        out["zero_ok"], out["keep_ok"] = m >= -eps, m <= eps
    else:
        out["zero_ok"], out["keep_ok"] = np.zeros(R * P, bool), np.ones(R * P, bool)
    return out


def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def standin_cotangents(c, group, w, use_gn, use_extra, R_bg, bug=None):
    """k_volsdf_cotangents in numpy float32 -> (sbar [M], nbar [M, 3], eik_ray [R])."""
    R, P = c["R"], c["P"]
    w, R_bg = F32(w), F32(R_bg)
    x, s, n = c["pts"], c["sdf"], c["nabla"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        coef = np.zeros(R, F32)
        if w != 0:
            npatch = patch_sizes(R, group)
            if bug == "ragged_group":
                npatch = np.full(R, R if (group <= 0 or group > R) else group)
            if bug == "coef_from_R":
                npatch = np.full(R, R)
            coef = (F32(1.0) / (npatch.astype(F32) * F32(P))).astype(F32)
        coef_m = np.repeat(coef, P)
        nrm = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
        sphere = (R_bg - nrm) - (F32(0.0) if bug == "clamp_no_1e6" else F32(1e-6))
        clamped = (s >= sphere) & ((R_bg > 0) | (bug == "clamp_at_Rbg0"))
        sbar = np.where(clamped, F32(0.0), c["g_sdf"]).astype(F32)
        b = c["g_n"].copy() if use_gn else np.zeros((R * P, 3), F32)
        acc = np.zeros(R, F32)
        if w != 0:
            nn = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
            err = nn - F32(1.0)
            k = (F32(2.0) * w) * coef_m * err / nn
            if bug != "nan_at_zero":
                k = np.where(nn != 0, k, F32(0.0)).astype(F32)
            b = _fma(k[:, None], n, b)
            lanes = np.zeros((R, 64), F32)
            e2 = err.reshape(R, P)
            for p0 in range(0, P, 64):                           # each lane's own fmaf chain over p = lane, lane + 64, ...
                if bug == "lane_dropped" and p0 > 0:
                    break
                m = min(64, P - p0)
                lanes[:, :m] = _fma(e2[:, p0:p0 + m], e2[:, p0:p0 + m], lanes[:, :m])
            for o in (32, 16, 8, 4, 2, 1):
                lanes = lanes + lanes[:, np.arange(64) ^ o]
            acc = lanes[:, 0]
        if use_extra and bug != "no_extra":
            b = b + c["g_n_extra"]
        eik = (coef * acc) if bug == "eik_no_w" else (w * coef * acc)
    return sbar, b.astype(F32), eik.astype(F32)


def check_cotangents(c, group, w, use_gn, use_extra, R_bg, sbar, nbar, eik, ref=None):
    R, P, M = c["R"], c["P"], c["R"] * c["P"]
    who = f"cotangents R={R} P={P} group={group} w={w:g} g_n={int(use_gn)} extra={int(use_extra)} R_bg={R_bg:g}"
    ref = cot_ref(c, group, w, use_gn, use_extra, R_bg) if ref is None else ref
    viol, ratio = [], {}
    if sbar.shape != (M,) or nbar.shape != (M, 3) or eik.shape != (R,):
        return [f"{who} sbar: shapes {sbar.shape} {nbar.shape} {eik.shape}"], ratio
    sb, gb = sbar.view(np.uint32), c["g_sdf"].view(np.uint32)
    ok = ((sb == 0) & ref["zero_ok"]) | ((sb == gb) & ref["keep_ok"])
    ratio["sbar"] = 0.0 if ok.all() else float("inf")
    if not ok.all():
        i = int(np.argmax(~ok))
        viol.append(f"{who} sbar: {int((~ok).sum())} of {M} elements are neither the allowed 0.0 nor the allowed bits of g_sdf, first at {i}: 0x{int(sb[i]):08x}")
    for name, got, want, A in (("nbar", nbar, ref["nbar"], ref["A_nbar"]), ("eik_ray", eik, ref["eik_ray"], ref["A_eik"])):
        if not np.isfinite(got).all():
            ratio[name] = float("inf")
            viol.append(f"{who} {name}: {int((~np.isfinite(got)).sum())} non-finite elements")
            continue
        err = np.abs(got.astype(F64) - want)
        ratio[name] = _ratio(err, A)
        if name == "nbar":                                       # held to the first allowance as well: see the docstring
            A1 = ref["A_nbar_first"]
            ratio["nbar_first_A"] = _ratio(err, A1)
            if (err > A1).any():
                i = int(np.argmax(err - A1))
                viol.append(f"{who} nbar: |got - ref| = {err.flat[i]:.3e} > the first allowance A1 = {A1.flat[i]:.3e} at flat index {i} of {err.size}")
        if (err > A).any():
            i = int(np.argmax(err - A))
            viol.append(f"{who} {name}: |got - ref| = {err.flat[i]:.3e} > A = {A.flat[i]:.3e} at flat index {i} of {err.size}")
    return _done(who, viol, ratio)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
def _u32(*bits):
    return np.array(bits, dtype=np.uint32).view(F32)


# a lo half with 9 significant bits (rounds up, truncates down); ties under an even and an odd upper half; the carry into the exponent; -0.0; a
# denormal (a multiple of 4 units: a quarter of it is exact); two large values
CRAFT_BIG = _u32(0x3F8001FF, 0x3F808000, 0x3F818000, 0x3F7FFFFF, 0x80000000, 0x00012344, 0x7F61B1E6, 0xFF61B1E6)        # +-3e38
CRAFT_TRIG = np.concatenate([CRAFT_BIG[:6], np.array([1.25, -1.25], F32)])


def _craft(a, big):
    """The first entries of a (row-major) replaced by the crafted values."""
    flat = a.reshape(-1)
    pool = CRAFT_BIG if big else CRAFT_TRIG
    n = min(flat.size, 9)
    flat[:n] = np.resize(pool, 9)[:n]
    return a


def _ball(rng, n, radius=BALL * 0.995):
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (radius * rng.random((n, 1)) ** (1 / 3))).astype(F32)


def _rng(*key):
    return np.random.default_rng([abs(int(k)) + 1000 * (int(k) < 0) for k in key])


@functools.lru_cache(maxsize=None)
def embed_case(M, multires):
    rng = _rng(1, M, multires)
    big = multires < 0
    return dict(M=M, multires=multires, pts=_craft(_ball(rng, M), big), dir=_craft((rng.standard_normal((M, 3)) * 1e-2).astype(F32), big))


@functools.lru_cache(maxsize=None)
def inputs_case(M, mx, mv):
    rng = _rng(2, M, mx, mv)
    v = rng.standard_normal((M, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    return dict(M=M, mx=mx, mv=mv, x=_craft(_ball(rng, M), mx < 0), view=_craft(v, mv < 0), normals=_craft(rng.standard_normal((M, 3)).astype(F32), True))


@functools.lru_cache(maxsize=None)
def rgb_case(M):
    """rows beyond M (to the largest rows_pad) feed the 'sums_rows_ge_M' mutant only.  The crafted g_rgb sit on rgb = 0.5: d4 = g / 4 exactly."""
    rng = _rng(3, M)
    n = up(M, 128)
    rgb, g = rng.random((n, 3)).astype(F32), rng.standard_normal((n, 3)).astype(F32)
    k = min(3 * M, 9)
    rgb.reshape(-1)[:k] = 0.5
    g.reshape(-1)[:k] = np.resize(_u32(0x408001FF, 0x40808000, 0x40818000, 0x407FFFFF, 0x80000000, 0x00012344, 0x7F61B1E6, 0xFF61B1E6), 9)[:k]
    return dict(M=M, rgb=rgb, g_rgb=g)


@functools.lru_cache(maxsize=None)
def sbar_case(M):
    rng = _rng(4, M)
    return dict(M=M, sbar=_craft(rng.standard_normal(M).astype(F32), True))


@functools.lru_cache(maxsize=None)
def ray_case(R, P):
    rng = _rng(5, R, P)
    dn = rng.standard_normal((R, 3))
    dn = (dn / np.linalg.norm(dn, axis=1, keepdims=True)).astype(F32)
    return dict(R=R, P=P, o=(rng.random((R, 3)) * 2 - 1).astype(F32), dn=dn, depth=np.sort(rng.random((R, P)) * 6, axis=1).astype(F32))


@functools.lru_cache(maxsize=None)
def cot_case(R, P, R_bg=3.0):
    """One set of inputs per (R, P): the calls differ in group, w, the two optional cotangents and R_bg (the sdf is built for R_bg = 3)."""
    rng = _rng(6, R, P)
    M = R * P
    pts = _ball(rng, M)
    x32 = np.linalg.norm(pts.astype(F64), axis=1).astype(F32)   # pass 1's |x|: the rounded norm, NOT the kernel's own three-rounding sum of squares
    sphere32 = (F32(R_bg) - x32).astype(F32)
    cls = rng.integers(0, 3, M) // 2                            # a third of the points in class 1
    net = np.where(cls == 1, sphere32 + rng.uniform(0.01, 0.3, M).astype(F32), sphere32 - rng.uniform(0.01, 1.0, M).astype(F32)).astype(F32)
    sdf = np.minimum(net, sphere32).astype(F32)
    nb = M // 50                                                # class 2: at most 2 % of the case, inside the band
    if nb:
        idx = rng.choice(M, nb, replace=False)
        x64 = np.linalg.norm(pts[idx].astype(F64), axis=1)
        eps = 2.0 ** -23 * (1.75 * x64 + np.abs(R_bg - x64) + 1e-6)
        sdf[idx] = ((R_bg - x64) - 1e-6 + rng.uniform(-0.5, 0.5, nb) * eps).astype(F32)
        cls[idx] = 2
    nab = (rng.standard_normal((M, 3)) * 0.7).astype(F32)
    return dict(R=R, P=P, pts=pts, sdf=sdf, cls=cls, g_sdf=_craft(rng.standard_normal(M).astype(F32), True), nabla=nab,
                g_n=(rng.standard_normal((M, 3)) * 1e-3).astype(F32), g_n_extra=(rng.standard_normal((M, 3)) * 1e-3).astype(F32))


def zero_nabla_case(R=5, P=13):
    """cot_case with three exact-zero nablas and three with |n| = 1e-15 among the ordinary ones (squares of 1e-30: no underflow)."""
    c = dict(cot_case(R, P))
    n = c["nabla"].copy()
    n[[0, 17, 64]] = 0.0
    n[3] = (1e-15, 0, 0)
    n[30] = (0, -1e-15, 0)
    n[63] = np.array([1.0, -1.0, 1.0]) * (1e-15 / np.sqrt(3.0))
    c["nabla"] = n.astype(F32)
    c["zero_rows"], c["tiny_rows"] = [0, 17, 64], [3, 30, 63]
    return c


def cot_calls(R):
    return [(g, w, gn, ge, rb) for g in groups(R) for w in W_EIK for gn in (True, False) for ge in (True, False) for rb in R_BGS]
