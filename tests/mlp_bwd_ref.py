"""fp64 references of the per-sample backward kernels and of their dumps, a stand-in at the kernels' precision, and a comparator.

The kernels are k_sdf_fwd2_bf16 / k_sdf_bwd2_bf16 / k_radiance_bwd_bf16 (csrc/mlp_backward_bf16.hip) and the dumping forward
k_radiance_bf16<VE, true> (csrc/mlp_chain_bf16.hip), behind nerfart_sdf_fwd2, nerfart_sdf_bwd2, nerfart_radiance_fwd_dump and
nerfart_radiance_bwd.  tests/test_mlp_bwd_ref.py holds the references to torch's fp64 autograd on the CPU and shows that the
comparator accepts the stand-in and rejects it with injected bugs; tests/test_gpu_mlp_bwd.py holds the HIP kernels to it.

WEIGHTS.  oracle.nets.folded_weight in fp32 (what the packers split into bf16 hi + lo), cast to fp64.

DUMPS (include/nerfart_hip.h; header of csrc/mlp_backward_bf16.hip).  Every dump is [slot][rows][256], 512 B per row, column
k = 32 u + 8 g + e holds feature packing.unit_feature_hidden(u, g, e):
    f2_dump        rows 2 Mp, Mp = up(M, 64): value rows then tangent rows.  slot l = 0..7: [a_l; adot_l] bf16; slot 8 + l:
                   softplus'(z_l) as unorm16 in the value rows, the tangent rows are never written
    r2_dump        rows 2 Mp: slot l = 0..7: 65535 [zbar_l; t_l d_l] bf16
    radiance fwd   rows Mp = up(M, 128): slots f, r0, r1, r2, r3 bf16
    radiance bwd   rows Mp: slots delta0, delta1, delta2, delta3, g_f bf16 (rad_delta_slot: each delta in the slot of the activation it
                   multiplies)
SDF layer 3 has 217 outputs: only features 0..216 of its slots are compared, the others must be finite, and unit 7 (features
224..255) of f2 slots 3 and 11 is zero bit for bit.

PADDED ROWS (M .. Mp - 1; the weight-gradient reductions run over them unmasked).  The kernels give a padded point the inputs 0 and
the cotangents 0, so: adot_l and zbar_l rows are exactly 0 (their partners a_l and t_l d_l are finite), the radiance deltas and g_f
are exactly 0 (the radiance activations are finite) - every product row of a padded point is exactly 0.  The same holds for real rows
with zero cotangents: dir == 0 gives adot == 0; dir == 0 and gbar == 0 give zbar == 0; g_rgb == 0 gives deltas, g_f, g_h7, g_n == 0.

ALLOWANCES (check()).  With ref the fp64 reference and sim the stand-in BEFORE its output rounding,
    A = FACTOR max |sim - ref| over the slot half (or output) of the case,  FACTOR = 4:
the kernels sum in another order (MFMA tiles, k-steps) and use the hardware's exp / log / rcp approximations, which moves an error of
this kind by a small factor, not by an order of magnitude.  A is computed per case from reference and stand-in, never from the code
under test.
    bf16 element         |got - ref| <= half_ulp_bf16(ref) + A   (pack_bf16 is v_cvt_pk_bf16_f32: round to nearest even.  bf16 keeps 8
                         significant bits, so half an ulp of 2^e <= |x| < 2^(e+1) is 2^(e-8): between 2^-9 |x| and 2^-8 |x|.  A flat
                         2^-9 |ref| is half an ulp only at the top of a binade - the exact value, correctly rounded, misses it by up to
                         a factor 2 - so the term is the half ulp itself.)
    softplus' (unorm16)  |got / 65535 - d_ref| <= 2^-17 + A (v_cvt_pknorm_u16 rounds to nearest: half a step)
    fp32 outputs         |got - ref| <= A
    ReLU masks           dump r_l > 0 iff z_l^ref > 0 except where |z_l^ref| <= A; at most max(3, 1 %) excepted elements per layer
    mean of softplus'    |mean(got / 65535 - d_ref)| <= A_mean + 6 sigma, sigma = 2^-16 / sqrt(12 N): a rounding that is not to
                         nearest moves the mean of N elements by half a step, far below the per-element allowance; A_mean =
                         FACTOR max(|mean(sim - ref)|, the same after rounding)
    aggregate            every weight-gradient product surf_param_bwd / rad_param_bwd (csrc/render_backward.hip) forms from the dumps,
                         Z^T A in fp64 from the decoded dumps over ALL rows, against the reference's own; allowance FACTOR times the
                         largest error of the same product formed from the stand-in's dumps
The reverse sweeps are references of the operation the kernel performs: ref_sdf_bwd2 takes (adot, d) as decoded from the forward
dump it is given and ref_radiance_bwd the rgb and the ReLU signs of the forward dump it is given - that is what the kernels read.

The stand-in is a vectorised torch model (not bit exact; tests/emul_chain.py stays the bit-level model): operands split
hi = bf16_rne(x), lo = bf16_rne(x - hi), a product = hi hi + hi lo + lo hi accumulated in fp32, activation functions in fp32, outputs
rounded and laid out like the kernels' own.  It carries the mutants (MUTANTS) that check() must reject.
"""
import math

import torch

from nerfart_amd import packing
from oracle import nets as onets

F64, F32 = torch.float64, torch.float32
FACTOR = 4.0
RS2 = 1.0 / math.sqrt(2.0)
PERM = torch.tensor([packing.unit_feature_hidden(u, g, e) for u in range(8) for g in range(4) for e in range(8)])   # column -> feature
POS = torch.empty(256, dtype=torch.long)
POS[PERM] = torch.arange(256)                                                                                      # feature -> column
W3 = 217                                   # outputs of SDF layer 3
FILL = 0xFF                                # the tests pre-fill every buffer with it: NaN as bf16 and as fp32


def up(m, k):
    return (m + k - 1) // k * k


# ---------------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------------
class Nets:
    """Folded weights of a reference-format state dict: W[l], b[l] (SDF net, l = 0..8) and R[l], rb[l] (radiance net, l = 0..4) in fp64."""

    def __init__(self, sd, device="cpu"):
        sd = {k: v.detach().float().cpu() for k, v in sd.items()}
        s, r = "implicit_surface.surface_fc_layers", "radiance_net.layers"
        assert onets.n_layers(sd, s) == 9 and onets.n_layers(sd, r) == 5
        self.W = [onets.folded_weight(sd, f"{s}.{l}").to(device).double() for l in range(9)]
        self.b = [sd[f"{s}.{l}.bias"].to(device).double() for l in range(9)]
        self.R = [onets.folded_weight(sd, f"{r}.{l}").to(device).double() for l in range(5)]
        self.rb = [sd[f"{r}.{l}.bias"].to(device).double() for l in range(5)]
        assert self.W[3].shape == (W3, 256) and self.W[4].shape == (256, 256) and self.W[8].shape == (257, 256)
        self.nex = self.R[0].shape[1] - 256                 # [x | view | n] columns of radiance layer 0
        assert self.nex in (9, 33)
        self.multires_view = -1 if self.nex == 9 else 4
        self.view_tiles = 1 if self.nex == 9 else 3
        self.device = device

    def to(self, device):
        n = Nets.__new__(Nets)
        n.__dict__.update(self.__dict__)
        for k in ("W", "b", "R", "rb"):
            setattr(n, k, [t.to(device) for t in getattr(self, k)])
        n.device = device
        return n


# ---------------------------------------------------------------------------------------------------------------------------
# dump codecs
# ---------------------------------------------------------------------------------------------------------------------------
def _i16_to_u(v):
    return v.to(torch.int32) & 0xFFFF


def decode_bf16(raw, slots, rows):
    """uint8 [slots * rows * 512] -> fp32 [slots, rows, 256] in FEATURE order."""
    return raw.view(torch.bfloat16).view(slots, rows, 256).float()[..., POS.to(raw.device)]


def decode_unorm16(raw, slots, rows):
    """uint8 -> int32 [slots, rows, 256] (0..65535) in feature order."""
    return _i16_to_u(raw.view(torch.int16).view(slots, rows, 256))[..., POS.to(raw.device)]


def encode_bf16(x):
    """fp32 [..., 256] in feature order -> uint8 bytes in unit order, rounded to nearest even."""
    return x[..., PERM.to(x.device)].contiguous().to(torch.bfloat16).view(torch.uint8).reshape(-1)


def encode_unorm16(d, truncate=False):
    """d in [0, 1], feature order -> uint8 bytes of rint(65535 d) in unit order."""
    q = d.double().clamp(0.0, 1.0) * 65535.0
    q = (torch.floor(q) if truncate else torch.round(q)).to(torch.int32)           # torch.round: half to even, as the hardware
    q = q[..., PERM.to(d.device)].contiguous()
    return torch.where(q >= 32768, q - 65536, q).to(torch.int16).view(torch.uint8).reshape(-1)


def f2_bytes(M):
    return 16 * 2 * up(M, 64) * 512


def r2_bytes(M):
    return 8 * 2 * up(M, 64) * 512


def rad_bytes(M):
    return 5 * up(M, 128) * 512


def decode_f2(raw, M):
    """-> a [8, Mp, 256], adot [8, Mp, 256] (fp32), D [8, Mp, 256] (int 0..65535), the never-written tangent rows of slots 8..15 (uint8)."""
    Mp = up(M, 64)
    av = decode_bf16(raw[: 8 * 2 * Mp * 512], 8, 2 * Mp)
    rest = raw[8 * 2 * Mp * 512:]
    D = decode_unorm16(rest, 8, 2 * Mp)[:, :Mp]
    untouched = rest.view(8, 2 * Mp, 512)[:, Mp:]
    return av[:, :Mp], av[:, Mp:], D, untouched


def decode_r2(raw, M):
    """-> zbar [8, Mp, 256], td [8, Mp, 256]: the dump divided by 65535, fp64."""
    Mp = up(M, 64)
    v = decode_bf16(raw, 8, 2 * Mp).double() / 65535.0
    return v[:, :Mp], v[:, Mp:]


def decode_rad(raw, M):
    return decode_bf16(raw, 5, up(M, 128))


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------------
def embed_pair(x, v, multires=6):
    """Embedder (models/base.py:38-64) and its tangent along v: [x, sin(2^k x), cos(2^k x) ...]."""
    e, t = [x], [v]
    for k in range(multires):
        f = float(2 ** k)
        s, c = torch.sin(x * f), torch.cos(x * f)
        e += [s, c]
        t += [f * c * v, -f * s * v]
    return torch.cat(e, -1), torch.cat(t, -1)


def softplus100(z):
    return torch.logaddexp(torch.zeros_like(z), 100.0 * z) / 100.0


def ref_sdf_fwd2(nets, pts, dirv):
    """-> dict z, a, d, adot: lists over l = 0..7 of [M, n_l] (n_3 = 217), e, edot [M, 39].  adot_l = d_l (W_l adot_{l-1})."""
    x, v = pts.to(nets.device).double(), dirv.to(nets.device).double()
    e, edot = embed_pair(x, v)
    h, hd = e, edot
    out = dict(z=[], a=[], d=[], adot=[], e=e, edot=edot)
    for l in range(8):
        if l == 4:
            h, hd = torch.cat([h, e], -1) * RS2, torch.cat([hd, edot], -1) * RS2
        z = h @ nets.W[l].T + nets.b[l]
        d = torch.sigmoid(100.0 * z)
        h, hd = softplus100(z), d * (hd @ nets.W[l].T)
        out["z"].append(z); out["a"].append(h); out["d"].append(d); out["adot"].append(hd)
    return out


def sdf_h7_nabla(nets, pts):
    """h7 = a_7 [M, 256] and nabla = grad_x sdf [M, 3] of the fp64 SDF reference."""
    eye = torch.eye(3, dtype=F64, device=nets.device)
    nab = []
    for c in range(3):
        o = ref_sdf_fwd2(nets, pts, eye[c].expand(pts.shape[0], 3))
        nab.append(o["adot"][7] @ nets.W[8][0])
    return o["a"][7], torch.stack(nab, -1)


def ref_sdf_bwd2(nets, gbar_h7, gbar_sdf, adot, d):
    """adot, d: lists over l of [M, n_l] fp64.  -> zbar, td: lists over l."""
    w8 = nets.W[8][0]
    t = w8.expand(gbar_sdf.shape[0], 256)
    abar = gbar_h7.double() + gbar_sdf.double()[:, None] * w8
    zbar, td = [None] * 8, [None] * 8
    for l in range(7, -1, -1):
        td[l] = t * d[l]
        zbar[l] = abar * d[l] + 100.0 * t * adot[l] * (1.0 - d[l])
        if l > 0:
            t, abar = td[l] @ nets.W[l], zbar[l] @ nets.W[l]
            if l == 4:
                t, abar = t[:, :W3] * RS2, abar[:, :W3] * RS2
    return zbar, td


def rad_inputs(nets, pts, view, nabla):
    ev = onets.embed(view, nets.multires_view)
    return torch.cat([pts, ev, nabla], -1)


def ref_radiance_fwd(nets, pts, view, nabla, h7):
    """-> dict f, z (list of 4 pre-activations), r (list of 4), rgb, ex (the [x | view | n] columns)."""
    dev = nets.device
    pts, view, nabla, h7 = (t.to(dev).double() for t in (pts, view, nabla, h7))
    f = h7 @ nets.W[8][1:].T + nets.b[8][1:]
    ex = rad_inputs(nets, pts, view, nabla)
    h = torch.cat([ex, f], -1)
    z, r = [], []
    for l in range(4):
        z.append(h @ nets.R[l].T + nets.rb[l])
        h = torch.relu(z[-1])
        r.append(h)
    rgb = torch.sigmoid(h @ nets.R[4].T + nets.rb[4])
    return dict(f=f, z=z, r=r, rgb=rgb, ex=ex)


def ref_radiance_bwd(nets, rgb, g_rgb, masks):
    """masks: list of 4 boolean [M, 256].  -> dict delta (list of 4), d4, g_f, g_n, g_h7."""
    rgb, g_rgb = rgb.to(nets.device).double(), g_rgb.to(nets.device).double()
    d4 = g_rgb * rgb * (1.0 - rgb)
    g = d4 @ nets.R[4]
    delta = [None] * 4
    for l in range(3, -1, -1):
        delta[l] = g * masks[l].to(g.dtype)
        g = delta[l] @ nets.R[l]
    nex = nets.nex
    g_f = g[:, nex:]
    return dict(delta=delta, d4=d4, g_f=g_f, g_n=g[:, nex - 3: nex], g_h7=g_f @ nets.W[8][1:])


# ---------------------------------------------------------------------------------------------------------------------------
# the stand-in at the kernels' precision
# ---------------------------------------------------------------------------------------------------------------------------
MUTANTS = (
    "drop_lo_hi",            # SDF layer 2: the (activation lo) x (weight hi) term dropped
    "no_curvature",          # 100 t adot (1 - d) omitted from zbar
    "curvature_d",           # ... with d in place of 1 - d
    "no_sbar_w8",            # gbar_sdf w8 missing from abar_7
    "r2_halves_swapped",     # the zbar rows and the t d rows of one r2 slot exchanged
    "delta_slot_l",          # radiance deltas written to slot l instead of l - 1
    "mask_from_next",        # ReLU masks taken from r_{l+1}
    "perm_halves",           # the two 4-element halves of the unit permutation exchanged
    "no_rsqrt2_reverse",     # 1 / sqrt 2 of the skip missing in the reverse sweep (see standin_sdf_bwd2)
    "no_rsqrt2_enc",         # ... missing on the skip's encoding columns (forward sweep: the only sweep that has them)
    "d_truncated",           # softplus' truncated to unorm16 instead of rounded
    "ragged_shift",          # the rows of the last ragged tile shifted by one point
    "pad_delta",             # a non-zero delta in a padded row
    "pad_nan",               # a NaN left in a padded activation row
)


def _hi(x):
    return x.to(torch.bfloat16).float()


def _split(x):
    h = _hi(x)
    return h, _hi(x - h)


def _prod(x, w, drop_lo_hi=False):
    """x [M, K] @ w [N, K]^T with both operands split: hi hi + hi lo + lo hi, fp32."""
    xh, xl = _split(x)
    wh, wl = _split(w)
    y = xh @ wh.T + xh @ wl.T
    return y if drop_lo_hi else y + xl @ wh.T


def _sig_soft(z):
    """softplus'(z) and softplus(z), beta = 100, the way epi_phase forms them in fp32."""
    e = torch.exp(-(100.0 * z).abs())
    r = 1.0 / (1.0 + e)
    return torch.where(z >= 0, r, e * r), torch.relu(z) + torch.log(1.0 + e) * 0.01


def _pad_rows(x, rows):
    out = torch.zeros((rows,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    out[: x.shape[0]] = x
    return out


def _pad_cols(x):
    if x.shape[-1] == 256:
        return x
    out = torch.zeros(tuple(x.shape[:-1]) + (256,), dtype=x.dtype, device=x.device)
    out[..., : x.shape[-1]] = x
    return out


def standin_sdf_fwd2(nets, pts, dirv, mut=None):
    """-> (a, adot, d): lists over l of fp32 [Mp, n_l] before the output rounding, padded points evaluated at 0 like the kernel's."""
    dev = nets.device
    Mp = up(pts.shape[0], 64)
    x, v = _pad_rows(pts.to(dev).float(), Mp), _pad_rows(dirv.to(dev).float(), Mp)
    e, edot = embed_pair(x, v)
    h, hd = e, edot
    A, AD, D = [], [], []
    for l in range(8):
        w = nets.W[l]
        if l == 4:
            w = w * RS2                                            # the packer scales the skip layer's weights (packing.surface_plan_bf16)
            if mut == "no_rsqrt2_enc":
                w = torch.cat([w[:, :W3], nets.W[l][:, W3:]], -1)
            h, hd = torch.cat([h, e], -1), torch.cat([hd, edot], -1)
        w = w.float()
        drop = mut == "drop_lo_hi" and l == 2
        z = _prod(h, w, drop) + nets.b[l].float()
        d, a = _sig_soft(z)
        ad = d * _prod(hd, w, drop)
        A.append(a); AD.append(ad); D.append(d)
        h, hd = a, ad                                              # the next layer splits the fp32 activation again: hi + lo
    return A, AD, D


def standin_sdf_bwd2(nets, gbar_h7, gbar_sdf, adot, D, mut=None):
    """adot: list of fp32 [Mp, n_l] (bf16 values), D: list of int [Mp, n_l] (0..65535), both as decoded from a forward dump.
    -> (zbar, td): lists of fp32 [Mp, n_l], the kernel's accumulators times 65535 BEFORE the bf16 rounding.
    The kernels' reverse sweep has no encoding columns (it produces parameter gradients only: the cotangent of the encoding is never
    needed), so the skip's 1 / sqrt 2 appears there once, on the 217 hidden columns of W_4^T: 'no_rsqrt2_reverse' drops that one."""
    dev = nets.device
    Mp = adot[0].shape[0]
    w8 = nets.W[8][0].float()
    sb = _pad_rows(gbar_sdf.to(dev).float(), Mp)
    hb = _pad_rows(gbar_h7.to(dev).float(), Mp)
    t = w8.expand(Mp, 256)
    abar = hb if mut == "no_sbar_w8" else torch.addcmul(hb, sb[:, None], w8)
    zbar, td = [None] * 8, [None] * 8
    for l in range(7, -1, -1):
        Dl = D[l].to(dev).float()
        td[l] = t * Dl
        curv = (100.0 * t * adot[l].to(dev)) * (Dl if mut == "curvature_d" else 65535.0 - Dl)
        zbar[l] = abar * Dl + (0.0 if mut == "no_curvature" else curv)
        if l > 0:
            scale = (RS2 if l == 4 and mut != "no_rsqrt2_reverse" else 1.0) / 65535.0
            wt = (nets.W[l] * scale).float().T[: (W3 if l == 4 else None)]       # [in, out]: the transposed chunk, 1 / 65535 absorbed
            t, abar = _prod(td[l], wt), _prod(zbar[l], wt)
    return zbar, td


def standin_radiance_fwd(nets, pts, view, nabla, h7):
    """-> dict f, r (list of 4), rgb: fp32 [Mp, .] before the output rounding (rgb: [M, 3])."""
    dev, M = nets.device, pts.shape[0]
    Mp = up(M, 128)
    pts, view, nabla, h7 = (_pad_rows(t.to(dev).float(), Mp) for t in (pts, view, nabla, h7))
    f = _prod(h7, nets.W[8][1:].float()) + nets.b[8][1:].float()
    ex = rad_inputs(nets, pts, view, nabla)
    nex, r = nets.nex, []
    R0 = nets.R[0].float()
    h = torch.relu(_prod(f, R0[:, nex:]) + _prod(ex, R0[:, :nex]) + nets.rb[0].float())
    r.append(h)
    for l in range(1, 4):
        h = torch.relu(_prod(h, nets.R[l].float()) + nets.rb[l].float())
        r.append(h)
    rgb = torch.sigmoid(h @ nets.R[4].float().T + nets.rb[4].float())
    return dict(f=f, r=r, rgb=rgb[:M])


def standin_radiance_bwd(nets, rgb, g_rgb, masks, mut=None):
    """masks: list of 4 boolean [Mp, 256].  -> dict delta (list of 4), g_f: fp32 [Mp, 256] before rounding; g_h7 [M, 256], g_n [M, 3]."""
    dev, M = nets.device, rgb.shape[0]
    Mp = masks[0].shape[0]
    o, g_rgb = _pad_rows(rgb.to(dev).float(), Mp), _pad_rows(g_rgb.to(dev).float(), Mp)
    d4 = g_rgb * o * (1.0 - o)
    g = d4 @ nets.R[4].float()
    delta = [None] * 4
    for l in range(3, -1, -1):
        mk = masks[min(l + 1, 3)] if mut == "mask_from_next" else masks[l]
        delta[l] = g * mk.to(dev).float()
        g = _prod(delta[l], nets.R[l].float().T)
    nex = nets.nex
    g_f = g[:, nex:]
    return dict(delta=delta, g_f=g_f, g_n=g[:M, nex - 3: nex], g_h7=_prod(g_f, nets.W[8][1:].float().T)[:M])


# ---- the stand-in's output buffers, laid out like the kernels' own --------------------------------------------------------------
def _swap_halves(raw):
    """Exchange the two 4-element halves of every group of 8 columns (bf16 / unorm16 elements of 2 B)."""
    v = raw.view(-1, 2, 8)                                        # [groups of 8 elements][half][4 elements x 2 B]
    return torch.stack([v[:, 1], v[:, 0]], 1).reshape(-1)


def _shift_last_tile(raw, slots, rows_per_half, halves, M, tile):
    """Rows of the last ragged tile moved down by one point, in every slot and half."""
    v = raw.view(slots, halves, rows_per_half, 512).clone()
    t0 = (M - 1) // tile * tile
    v[:, :, t0 + 1: t0 + tile] = raw.view(slots, halves, rows_per_half, 512)[:, :, t0: t0 + tile - 1]
    return v.reshape(-1)


def encode_f2(A, AD, D, M, mut=None):
    Mp = up(M, 64)
    dev = A[0].device
    lo = torch.stack([torch.cat([_pad_cols(A[l]), _pad_cols(AD[l])], 0) for l in range(8)])              # [8, 2 Mp, 256]
    if mut == "pad_nan" and Mp > M:
        lo[5, Mp - 1, 17] = float("nan")
    raw_lo = encode_bf16(lo)
    hi = torch.full((8, 2 * Mp, 512), FILL, dtype=torch.uint8, device=dev)
    for l in range(8):
        hi[l, :Mp] = encode_unorm16(_pad_cols(D[l]), truncate=mut == "d_truncated").view(Mp, 512)
    raw = torch.cat([raw_lo, hi.reshape(-1)])
    if mut == "perm_halves":
        raw = torch.cat([_swap_halves(raw_lo), hi.reshape(-1)])
    if mut == "ragged_shift" and M % 64 > 1:
        raw = _shift_last_tile(raw, 16, Mp, 2, M, 64)
    return raw


def encode_r2(zbar, td, M, mut=None):
    Mp = up(M, 64)
    v = torch.stack([torch.cat([_pad_cols(zbar[l]), _pad_cols(td[l])], 0) for l in range(8)])
    if mut == "r2_halves_swapped":
        v[5] = torch.cat([v[5, Mp:], v[5, :Mp]], 0)
    return encode_bf16(v)


def encode_rad(slots, mut=None, M=None):
    v = torch.stack(list(slots))
    if mut == "delta_slot_l":
        v = torch.roll(v, 1, 0)
    if mut == "pad_delta" and v.shape[1] > M:
        v[2, v.shape[1] - 1, 100] = 1e-3
    return encode_bf16(v)


def run_standin(case, mut=None):
    """The stand-in through one case -> the same dict of buffers the GPU test collects from the library."""
    nets, M = case["nets"], case["M"]
    if case["kind"] == "sdf":
        A, AD, D = standin_sdf_fwd2(nets, case["pts"], case["dir"], mut)
        f2 = encode_f2(A, AD, D, M, mut)
        _, adot, Dq, _ = decode_f2(f2, M)
        n = [256, 256, 256, W3, 256, 256, 256, 256]
        zbar, td = standin_sdf_bwd2(nets, case["gbar_h7"], case["gbar_sdf"], [adot[l][:, : n[l]] for l in range(8)],
                                    [Dq[l][:, : n[l]] for l in range(8)], mut)
        return dict(f2=f2, r2=encode_r2(zbar, td, M, mut))
    fw = standin_radiance_fwd(nets, case["pts"], case["view"], case["nabla"], case["h7"])
    fdump = encode_rad([fw["f"]] + fw["r"])
    masks = [decode_rad(fdump, M)[1 + l] != 0 for l in range(4)]
    bw = standin_radiance_bwd(nets, fw["rgb"], case["g_rgb"], masks, mut)
    bdump = encode_rad(bw["delta"] + [bw["g_f"]], mut, M)
    if mut == "ragged_shift" and M % 128 > 1:
        bdump = _shift_last_tile(bdump, 5, up(M, 128), 1, M, 128)
    return dict(rgb=fw["rgb"], fdump=fdump, bdump=bdump, g_h7=bw["g_h7"], g_n=bw["g_n"])


# ---------------------------------------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------------------------------------
SDF_SIZES = (1, 63, 64, 65, 200)
SDF_WRAP = 256 * 64 + 65               # 258 tiles on the 256 workgroups launch_chain starts: two run a second tile, the last is ragged
RAD_SIZES = (1, 127, 128, 129, 300)
RAD_WRAP = 256 * 128 + 129


def specs(wrap=True):
    """(kind, framework, M): the SDF pair at every size on the VolSDF scene and two sizes on the NeuS scene; the radiance pair at
    every size for view_tiles 1 (VolSDF) and 3 (NeuS); one grid-wrapping size each."""
    s = [("sdf", "VolSDF", M) for M in SDF_SIZES] + [("sdf", "NeuS", M) for M in (65, 200)]
    s += [("rad", fw, M) for fw in ("VolSDF", "NeuS") for M in RAD_SIZES]
    if wrap:
        s += [("sdf", "VolSDF", SDF_WRAP), ("rad", "VolSDF", RAD_WRAP)]
    return s


def spec_id(s):
    return f"{s[0]}-{s[1]}-{s[2]}"


def make_case(spec, nets):
    """Seeded inputs (fp32 CPU tensors) of one case.  Points in [-1, 1]^3 with some out to |x| = 2 (fwd2 has no sphere clamp);
    cotangents ~ 1e-2 with some rows exactly 0."""
    kind, fw, M = spec
    g = torch.Generator().manual_seed(1000 * (1 + ("sdf", "rad").index(kind)) + 7 * M + (fw == "NeuS"))
    idx = torch.arange(M)
    pts = torch.rand(M, 3, generator=g) * 2 - 1
    pts[idx % 11 == 3] *= 2.0
    c = dict(kind=kind, fw=fw, M=M, nets=nets, pts=pts, id=spec_id(spec))
    if kind == "sdf":
        c["dir"] = torch.randn(M, 3, generator=g) * 1e-2
        c["gbar_sdf"] = torch.randn(M, generator=g) * 1e-2
        c["gbar_h7"] = torch.randn(M, 256, generator=g) * 1e-2
        zd, zg = (idx % 5 == 1) | (idx == 2), (idx % 7 == 2)
        c["dir"][zd] = 0.0
        c["gbar_sdf"][zg] = 0.0
        c["gbar_h7"][zg] = 0.0
    else:
        v = torch.randn(M, 3, generator=g)
        c["view"] = v / v.norm(dim=-1, keepdim=True)
        h7, nab = sdf_h7_nabla(nets, pts)
        c["h7"], c["nabla"] = h7.float().cpu(), nab.float().cpu()
        c["g_rgb"] = torch.randn(M, 3, generator=g) * 1e-2
        c["g_rgb"][idx % 4 == 1] = 0.0
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------------------
class _Report:
    def __init__(self, cid):
        self.cid, self.viol, self.ratio = cid, [], {}

    def fail(self, name, msg):
        self.viol.append(f"{self.cid} {name}: {msg}")

    def note(self, name, ratio):
        self.ratio[name] = max(self.ratio.get(name, 0.0), float(ratio))

    def finite(self, name, x):
        if not bool(torch.isfinite(x).all()):
            self.fail(name, f"{int((~torch.isfinite(x)).sum())} non-finite elements")
            return False
        return True

    def zero(self, name, x):
        if x.numel() and bool((x != 0).any()):                    # NaN != 0 too
            self.fail(name, f"{int((x != 0).sum())} elements that must be exactly 0 are not")

    def close(self, name, got, ref, sim, bf16):
        """|got - ref| <= half a bf16 ulp of ref (bf16 outputs) + FACTOR max |sim - ref|; returns the allowance A."""
        ref = ref.double()
        A = FACTOR * float((sim.double() - ref).abs().max()) if ref.numel() else 0.0
        if not self.finite(name, got):
            return A
        err, allow = (got.double() - ref).abs(), (half_ulp_bf16(ref) if bf16 else torch.zeros_like(ref)) + A
        ratio = float((err / allow.clamp_min(1e-300)).max()) if ref.numel() else 0.0
        self.note(name, ratio)
        if ratio > 1.0:
            i = int(torch.argmax(err / allow.clamp_min(1e-300)))
            self.fail(name, f"observed / allowed = {ratio:.2f} (|got - ref| = {float(err.flatten()[i]):.3e}, allowed {float(allow.flatten()[i]):.3e}, "
                            f"A = {A:.3e}) at flat index {i}")
        return A


UNORM_HALF = 2.0 ** -17


def half_ulp_bf16(x):
    """Half a unit in the last place of bf16 (8 significant bits) at |x|: 2^(e - 8) for 2^e <= |x| < 2^(e + 1); 0 at 0."""
    m, e = torch.frexp(x.double().abs())                          # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), e - 9))
_N = [256, 256, 256, W3, 256, 256, 256, 256]


def _group(name):
    """f2.a0 .. f2.a7 -> f2.a: one line of the report per kind of output."""
    return name if name == "g_h7" else name.rstrip("0123456789")


def check(case, out):
    """-> (violations: list of str, worst observed / allowed ratio per output group: dict)."""
    rep = _Report(case["id"])
    (_check_sdf if case["kind"] == "sdf" else _check_rad)(case, out, rep)
    worst = {}
    for k, v in rep.ratio.items():
        worst[_group(k)] = max(worst.get(_group(k), 0.0), v)
    return rep.viol, worst


def _check_sdf(case, out, rep):
    nets, M = case["nets"], case["M"]
    dev, Mp = nets.device, up(M, 64)
    f2, r2 = out["f2"].to(dev), out["r2"].to(dev)
    if f2.numel() != f2_bytes(M) or r2.numel() != r2_bytes(M):
        rep.fail("dumps", "wrong size")
        return
    a, adot, D, untouched = decode_f2(f2, M)
    ref = ref_sdf_fwd2(nets, case["pts"], case["dir"])
    sA, sAD, sD = standin_sdf_fwd2(nets, case["pts"], case["dir"])
    zd = (case["dir"] == 0).all(-1).to(dev)
    zg = zd & (case["gbar_sdf"] == 0).to(dev) & (case["gbar_h7"] == 0).all(-1).to(dev)
    # ---- forward dump -----------------------------------------------------------------------------------------------------------
    if bool((untouched != FILL).any()):
        rep.fail("f2.tangent rows of slots 8..15", "written (the contract: never written or read)")
    for l in range(8):
        n = _N[l]
        rep.close(f"f2.a{l}", a[l, :M, :n], ref["a"][l], sA[l][:M], True)
        rep.close(f"f2.adot{l}", adot[l, :M, :n], ref["adot"][l], sAD[l][:M], True)
        # softplus': half a unorm16 step + A, and the mean
        dref = ref["d"][l]
        A = FACTOR * float((sD[l][:M].double() - dref).abs().max())
        dgot = D[l, :M, :n].double() / 65535.0
        err = (dgot - dref).abs()
        rep.note(f"f2.d{l}", float(err.max()) / (UNORM_HALF + A))
        if float(err.max()) > UNORM_HALF + A:
            rep.fail(f"f2.d{l}", f"observed / allowed = {float(err.max()) / (UNORM_HALF + A):.2f}")
        N = dref.numel()
        simq = torch.round(sD[l][:M].double().clamp(0, 1) * 65535.0) / 65535.0
        Am = FACTOR * max(abs(float((sD[l][:M].double() - dref).mean())), abs(float((simq - dref).mean()))) + 6.0 * 2.0 ** -16 / math.sqrt(12.0 * N)
        mean = abs(float((dgot - dref).mean()))
        rep.note(f"f2.dmean{l}", mean / Am)
        if mean > Am:
            rep.fail(f"f2.dmean{l}", f"|mean(got / 65535 - d_ref)| = {mean:.3e}, allowed {Am:.3e}")
        rep.finite(f"f2.a{l} (columns past the layer, padded rows)", a[l])
        rep.zero(f"f2.adot{l} padded rows", adot[l, M:])
        rep.zero(f"f2.adot{l} rows with dir == 0", adot[l, :M][zd])
    lo16 = f2.view(16, 2 * Mp, 8, 64)
    if bool((lo16[3, :, 7] != 0).any()) or bool((lo16[11, :Mp, 7] != 0).any()):
        rep.fail("f2 slot 3 / 11 unit 7", "not zero bit for bit")
    # ---- reverse dump: a reference of the operation on the forward dump the kernel was given ------------------------------------------
    adl = [adot[l, :, : _N[l]] for l in range(8)]
    Dl = [D[l, :, : _N[l]] for l in range(8)]
    if not all(bool(torch.isfinite(t).all()) for t in adl):
        rep.fail("r2", "the forward dump's tangent rows are not finite: no reference for the reverse sweep")
        return
    rz, rtd = ref_sdf_bwd2(nets, case["gbar_h7"].to(dev), case["gbar_sdf"].to(dev), [t[:M].double() for t in adl],
                           [t[:M].double() / 65535.0 for t in Dl])
    sz, std_ = standin_sdf_bwd2(nets, case["gbar_h7"], case["gbar_sdf"], adl, Dl)
    zbar, td = decode_r2(r2, M)
    for l in range(8):
        n = _N[l]
        rep.close(f"r2.zbar{l}", zbar[l, :M, :n], rz[l], sz[l][:M].double() / 65535.0, True)
        rep.close(f"r2.td{l}", td[l, :M, :n], rtd[l], std_[l][:M].double() / 65535.0, True)
        rep.finite(f"r2.td{l} (columns past the layer, padded rows)", td[l])
        rep.finite(f"r2.zbar{l} (columns past the layer)", zbar[l])
        rep.zero(f"r2.zbar{l} padded rows", zbar[l, M:])
        rep.zero(f"r2.zbar{l} rows with dir == 0 and gbar == 0", zbar[l, :M][zg])
    # ---- aggregate: the products of surf_param_bwd ---------------------------------------------------------------------------------
    sim_f2 = encode_f2(sA, sAD, sD, M)
    sa, sad, _, _ = decode_f2(sim_f2, M)
    szq, stq = decode_r2(encode_r2(sz, std_, M), M)
    E = torch.cat([_pad_rows(ref["e"], Mp), _pad_rows(ref["edot"], Mp)], 0)                               # the operand kernel's job: fp64 here
    SO = torch.cat([_pad_rows(case["gbar_sdf"].to(dev).double(), Mp), torch.ones(Mp, dtype=F64, device=dev)], 0)

    def products(zb, tdd, aa, aad, rows):
        """zb / tdd / aa / aad: indexable by layer -> [rows, n] fp64."""
        P = {}
        for l in range(1, 8):
            Z = torch.cat([zb[l], tdd[l]], 0).double()
            Aop = torch.cat([aa[l - 1], aad[l - 1]], 0).double()
            P[f"agg.sdf_W{l}"] = (Z.T @ Aop)[: _N[l], : _N[l - 1]]
            P[f"agg.sdf_b{l}"] = zb[l].double().sum(0)[: _N[l]]
        for l in (0, 4):
            Z = torch.cat([zb[l], tdd[l]], 0).double()
            Erows = torch.cat([E[:rows], E[Mp: Mp + rows]], 0)
            P[f"agg.sdf_We{l}"] = Z.T @ Erows
        P["agg.sdf_b0"] = zb[0].double().sum(0)
        S = torch.cat([SO[:rows], SO[Mp: Mp + rows]], 0)
        P["agg.sdf_w8"] = torch.cat([aa[7], aad[7]], 0).double().T @ S
        return P

    want = products(rz, rtd, ref["a"], ref["adot"], M)
    sim = products(szq, stq, sa, sad, Mp)
    got = products(zbar, td, a.double(), adot.double(), Mp)
    _compare_products(rep, got, want, sim)


def _compare_products(rep, got, want, sim):
    for k in want:
        A = FACTOR * float((sim[k] - want[k]).abs().max())
        if not rep.finite(k, got[k]):
            continue
        err = float((got[k] - want[k]).abs().max())
        rep.note(k, err / max(A, 1e-300))
        if err > A:
            rep.fail(k, f"observed / allowed = {err / max(A, 1e-300):.2f} (max |got - ref| = {err:.3e}, allowed {A:.3e})")


def mask_exceptions(z_ref, A):
    """Elements whose ReLU sign the arithmetic allowance leaves open, and how many a layer of this size may have."""
    return z_ref.abs() <= A, max(3, z_ref.numel() // 100)


def _check_rad(case, out, rep):
    nets, M = case["nets"], case["M"]
    dev, Mp = nets.device, up(M, 128)
    fd, bd = out["fdump"].to(dev), out["bdump"].to(dev)
    if fd.numel() != rad_bytes(M) or bd.numel() != rad_bytes(M):
        rep.fail("dumps", "wrong size")
        return
    rgb, g_h7, g_n = (out[k].to(dev) for k in ("rgb", "g_h7", "g_n"))
    ref = ref_radiance_fwd(nets, case["pts"], case["view"], case["nabla"], case["h7"])
    sim = standin_radiance_fwd(nets, case["pts"], case["view"], case["nabla"], case["h7"])
    acts = decode_rad(fd, M)
    rep.finite("fwd dump", acts)
    rep.close("fwd.f", acts[0, :M], ref["f"], sim["f"][:M], True)
    for l in range(4):
        A = rep.close(f"fwd.r{l}", acts[1 + l, :M], ref["r"][l], sim["r"][l][:M], True)
        open_, cap = mask_exceptions(ref["z"][l], A)
        if int(open_.sum()) > cap:
            rep.fail(f"mask.r{l}", f"{int(open_.sum())} pre-activations within A = {A:.2e} of 0, more than the {cap} a layer of this case may have")
        bad = ((acts[1 + l, :M] > 0) != (ref["z"][l] > 0)) & ~open_
        rep.note(f"mask.r{l}", float(bad.sum()))
        if bool(bad.any()):
            rep.fail(f"mask.r{l}", f"{int(bad.sum())} ReLU signs differ from the reference outside the allowance")
    rep.close("rgb", rgb, ref["rgb"], sim["rgb"], False)
    if "rgb_plain" in out:                                           # nerfart_radiance_fwd on the same inputs: the same allowance
        rep.close("rgb_plain", out["rgb_plain"].to(dev), ref["rgb"], sim["rgb"], False)
    # ---- backward: a reference of the operation on the rgb and the forward dump the kernel was given --------------------------------
    masks = [acts[1 + l] != 0 for l in range(4)]                     # what k_radiance_bwd_bf16 reads: any non-zero bit pattern
    rb = ref_radiance_bwd(nets, rgb, case["g_rgb"], [m[:M] for m in masks])
    sb = standin_radiance_bwd(nets, rgb, case["g_rgb"], masks)
    dl = decode_rad(bd, M)
    zr = (case["g_rgb"] == 0).all(-1).to(dev)
    for l in range(4):
        rep.close(f"bwd.delta{l}", dl[l, :M], rb["delta"][l], sb["delta"][l][:M], True)
    rep.close("bwd.g_f", dl[4, :M], rb["g_f"], sb["g_f"][:M], True)
    rep.close("g_h7", g_h7, rb["g_h7"], sb["g_h7"], False)
    rep.close("g_n", g_n, rb["g_n"], sb["g_n"], False)
    rep.zero("bwd dump padded rows", dl[:, M:])
    rep.zero("bwd dump rows with g_rgb == 0", dl[:, :M][:, zr])
    rep.zero("g_h7 rows with g_rgb == 0", g_h7[zr])
    rep.zero("g_n rows with g_rgb == 0", g_n[zr])
    # ---- aggregate: the products of rad_param_bwd -----------------------------------------------------------------------------------
    h7p = _pad_rows(case["h7"].to(dev).double(), Mp)
    exp_ = _pad_rows(ref["ex"], Mp)
    d4p = _pad_rows(rb["d4"], Mp)                                    # the operand kernel's job (from the rgb given): fp64 here

    def products(deltas, g_f, act, rows):
        P = {"agg.rad_Wh7": g_f.double().T @ h7p[:rows], "agg.rad_bh7": g_f.double().sum(0)}
        for l in range(4):
            P[f"agg.rad_W{l}"] = deltas[l].double().T @ act[l].double()
            P[f"agg.rad_b{l}"] = deltas[l].double().sum(0)
        P["agg.rad_W4"] = act[4].double().T @ d4p[:rows]
        P["agg.rad_Wex"] = deltas[0].double().T @ exp_[:rows]
        return P

    want = products(rb["delta"], rb["g_f"], [ref["f"]] + ref["r"], M)
    sact = decode_rad(encode_rad([sim["f"]] + sim["r"]), M)
    sdl = decode_rad(encode_rad(sb["delta"] + [sb["g_f"]]), M)
    simp = products(sdl[:4], sdl[4], sact, Mp)
    got = products(dl[:4], dl[4], acts, Mp)
    _compare_products(rep, got, want, simp)
