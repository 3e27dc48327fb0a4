"""fp64 references of the three forward point-query families, a trained-like weight state, one stand-in per arithmetic tier, and a comparator.

The families are nerfart_sdf_fwd[_rays], nerfart_sdf_nabla_fwd[_rays] and nerfart_radiance_fwd[_rays] (csrc/mlp_chain.hip and the split kernels it
dispatches to).  tests/test_point_query_ref.py holds the references to torch's fp64 autograd of a plain nn.functional model on the CPU and shows
that the comparator accepts every stand-in and rejects it with injected bugs; tests/test_gpu_point_queries.py holds the HIP kernels to it.

STATE (trained_like_state).  scene_state() is the geometric init plus 2 % noise on weight_v: every hidden SDF bias is exactly 0, the encoding columns
carry noise only and weight_g stays within 0.4 % of |weight_v|, so a kernel, packer or plan that mishandles a bias, an encoding column or weight_g
computes the same numbers on it.  A copy is changed with a seeded generator (the values used; all of the conditions of check_state hold with them):
    encoding columns of SDF layer 0 ([:, 3:]) and of the skip layer (its last 36 input columns)   ENC_AMP = 0.25 times the rms of the xyz columns
                                                                                               (layer 0) / of the hidden columns (skip) times
                                                                                               2^-band times N(0, 1)
    hidden SDF biases (layers 0..7)                                                              BIAS_AMP = 0.02 N(0, 1)
    geometry-feature biases (layer 8, rows 1..)                                                  FEAT_BIAS_AMP = 0.05 N(0, 1)
    every weight_g (SDF layers 0..8, radiance layers)                                            times exp(G_AMP N(0, 1)), G_AMP = 0.1
    layer 8 bias[0]                                                                              shifted so that the median reference sdf over the
                                                                                               state's query points (query_points) with |x| < 1 is 0
    weight_g of the rgb layer (radiance layer 4)                                                 scaled so that the rms of its products over the query
                                                                                               points is RGB_LOGIT_RMS = 1.5 (one more condition than
                                                                                               the SDF ones: with the scene's gain of 4 on every
                                                                                               radiance weight_g the rgb of this state sits within
                                                                                               1e-3 of 0 or 1 and the sigmoid hides every error of the
                                                                                               radiance net; at least half of the rgb elements must lie
                                                                                               in [0.05, 0.95])
big_bias_layer = l gives the second state: layer l's biases are BIG_BIAS_AMP = 0.2 N(0, 1).  At 0.02 the swap of two biases of layer 1 moves the stand-in's sdf
by only 2.9 (fp16x1) and 5.4 (fp16x2) times the fp16 tiers' allowance on VolSDF: the fp16 tiers are held on the second state with l = BIG_BIAS_LAYER = 1
(27 and 39 times on the hardware), the one layer of 0..7 with which every condition holds again on both scenes (layers 2..7 flatten the inside of the
surface, |nabla| falls below 0.1; layer 0 does so on NeuS).
The conditions are evaluated on query_points(): the parity test's 1000 points; for NeuS divided by 3 and the inner ones pushed out by NEUS_PUSH = 0.2.

WEIGHTS.  The references fold weight_norm in fp64 (Nets.W, Nets.R): they are the network the state dict defines.  The stand-ins read the fold in fp32
(Nets.Wf, Nets.Rf; mlp_bwd_ref.Nets), which is what the packers fold and split: the rounding of the fold is part of every tier's error, and of A.

TIERS.  A stand-in is vectorised torch (not bit exact; tests/emul_chain.py stays the bit-level model) and returns its outputs before output rounding.
    fp32     products and sums in fp32 (C-ABI precision 0: reverse-mode nabla, softplus' kept in fp32; 3: forward-mode tangents)
    bf16x3   operands split hi = bf16(x), lo = bf16(x - hi), a product = hi hi + hi lo + lo hi in fp32 (1: reverse mode, softplus' of layers 0..6 parked
             as unorm16 and the 1 / 65535 folded into the transposed weights; 2: forward mode)
    fp16x2   ONE fp16 activation term x fp16 hi + lo weights on the units built from accumulators; the ready-made input units (the encodings of layers
             0 and 4, the radiance net's [x | view | n] and its h7 rows) keep hi + lo on both sides and the three-term form (mlp_bf16_core.h,
             NERFART_F16X2).  Precision 4: reverse mode, softplus' as unorm16, cotangent units times 1 / 65535 in fp16
    fp16x1   sdf only (precision 5): one fp16 term each on the units built from accumulators, three terms on the encodings, in the SCALED softplus
             recursion z' = c z, a' = c softplus(z) = max(z', 0) + log2(1 + 2^-|z'|), c = 100 log2 e - layer 0's weights, the skip layer's encoding
             columns and the hidden biases carry c, the sdf row 1 / c (nerfart_amd/calibrate.py with compensate=False: weights rounded to nearest)
The last layer's row (sdf) and the radiance net's rgb layer are fp32 fmaf chains over the fp32 activations in every tier.

ALLOWANCE (check()).  Per case and per output (sdf, nabla, h7, rgb), with ref the fp64 reference and sim the stand-in of the case's tier and mode,
    A = FACTOR max |sim - ref|,  FACTOR = 4,     |got - ref| <= A for EVERY element:
the kernels sum in another order (MFMA tiles, k-steps) and use the hardware's exp / log approximations, which moves an error of this kind by a small
factor, not by an order of magnitude.  A never comes from the code under test.  A case is (state, entry point, precision, R_bg, point set); the sizes M
of the GPU test are the first M rows of the case's point set and share its A: the error at one point is one sample of the tier's error on this state,
and the maximum over the first M <= 16 rows is only a noisier estimate of the quantity the whole set measures.
The sphere clamp min(sdf, R_bg - |x|) is compared against the min: min is 1-Lipschitz in both arguments, so a kernel whose sdf is within A takes
either branch within A where the two differ by less than A.

MUTANTS.  Each is the stand-in with one injected fault; check() must reject every one at every tier that has the output it touches (fp16x1 has sdf only).
"""
import math

import torch

import mlp_bwd_ref as B
from mlp_bwd_ref import F32, F64, FACTOR, PERM, RS2, W3, _sig_soft, _split  # noqa: F401  (re-exported)
from oracle import nets as onets

ENC_AMP, BIAS_AMP, FEAT_BIAS_AMP, G_AMP, BIG_BIAS_AMP, RGB_LOGIT_RMS = 0.25, 0.02, 0.05, 0.1, 0.2, 1.5
C_SCALE = 100.0 * math.log2(math.e)
FILL = 0xFF
S, R = "implicit_surface.surface_fc_layers", "radiance_net.layers"
R_BG = {"VolSDF": 3.0, "NeuS": 0.0}                    # NeuS queries without the sphere clamp (neus.py:277)
# C-ABI precision -> (tier, how nabla is formed); taken from the dispatchers of csrc/mlp_chain.hip (check_precision, sdf_query, sdf_nabla_query, radiance_query)
PRECISION = {0: ("fp32", "rev"), 3: ("fp32", "fwd"), 1: ("bf16x3", "rev"), 2: ("bf16x3", "fwd"), 4: ("fp16x2", "rev"), 5: ("fp16x1", None)}
SDF_PRECISIONS, NABLA_PRECISIONS, RAD_PRECISIONS = (0, 1, 4, 5), (0, 1, 2, 3, 4), (0, 1, 4)
TIERS = ("fp32", "bf16x3", "fp16x2", "fp16x1")
SIZES = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000)
WRAP = 100003                                          # more tiles than workgroups: every workgroup loops, the chunk stream wraps
FAR = (5.3, 0.4, -2.0)                                 # the largest |x| the product queries (camera at 2.5, far = 6): 32 x reaches 170 rad
N_TIES = 4
NEUS_PUSH = 0.2


class Nets(B.Nets):
    """mlp_bwd_ref.Nets with the weight_norm fold g v / |v| in fp64 for the references (W, R): a point query is held to the network the state dict
    defines.  Wf, Rf keep the fold in fp32 - what the packers fold and split, one fp32 rounding per weight away - for the stand-ins (kernel_view)."""

    def __init__(self, sd, device="cpu"):
        super().__init__(sd, device)
        self.Wf, self.Rf = self.W, self.R
        fold = lambda k: (sd[k + ".weight_g"].detach().cpu().double().reshape(-1, 1) * sd[k + ".weight_v"].detach().cpu().double()
                          / sd[k + ".weight_v"].detach().cpu().double().norm(dim=1, keepdim=True)).to(device)
        self.W = [fold(f"{S}.{l}") for l in range(9)]
        self.R = [fold(f"{R}.{l}") for l in range(5)]

    def to(self, device):
        n = Nets.__new__(Nets)
        n.__dict__.update(self.__dict__)
        for k in ("W", "b", "R", "rb", "Wf", "Rf"):
            setattr(n, k, [t.to(device) for t in getattr(self, k)])
        n.device = device
        return n

    def kernel_view(self):
        n = Nets.__new__(Nets)
        n.__dict__.update(self.__dict__)
        n.W, n.R = self.Wf, self.Rf
        return n


# ---------------------------------------------------------------------------------------------------------------------------
# the state
# ---------------------------------------------------------------------------------------------------------------------------
def query_points(framework, n=1000, seed=11):
    """The parity test's points: uniform in [-3, 3]^3, the first 30 % scaled to the inner region; NeuS queries inside its unit sphere (/ 3)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, 3, generator=g) * 6 - 3
    p[: (3 * n) // 10] *= 0.35
    v = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    if framework != "VolSDF":
        # an sdf has a critical point inside every closed surface, where |nabla| -> 0 in the reference itself; NeuS' surface (radius 0.5) puts 10 % of the
        # inner points within 0.2 of it, VolSDF's (radius 1) none: NeuS' inner points are pushed out radially by NEUS_PUSH
        p = p / 3.0
        r = p[: (3 * n) // 10].norm(dim=-1, keepdim=True)
        p[: (3 * n) // 10] *= (r + NEUS_PUSH) / r
    return p, v


def _base_state(framework):
    from conftest import scene_state
    return scene_state(framework, 0.01 if framework == "VolSDF" else None)[0]


def trained_like_state(framework="VolSDF", seed=0, big_bias_layer=None):
    sd = {k: v.detach().clone() for k, v in _base_state(framework).items()}
    g = torch.Generator().manual_seed(7919 * (seed + 1) + (framework == "NeuS"))
    n = lambda *shape: torch.randn(*shape, generator=g)
    band = 2.0 ** -(torch.arange(36) // 6).float()
    for l, ref_cols in ((0, slice(0, 3)), (4, slice(0, W3))):
        v = sd[f"{S}.{l}.weight_v"]
        rms = float(v[:, ref_cols].pow(2).mean().sqrt())
        v[:, -36:] = ENC_AMP * rms * band * n(v.shape[0], 36)
    for l in range(8):
        b = sd[f"{S}.{l}.bias"]
        sd[f"{S}.{l}.bias"] = (BIG_BIAS_AMP if l == big_bias_layer else BIAS_AMP) * n(*b.shape)
    sd[f"{S}.8.bias"][1:] = FEAT_BIAS_AMP * n(256)
    for k in sorted(sd):
        if k.endswith("weight_g"):
            sd[k] = sd[k] * torch.exp(G_AMP * n(*sd[k].shape))
    pts = query_points(framework)[0]
    inner = pts[pts.norm(dim=-1) < 1.0]
    sd[f"{S}.8.bias"][0] -= float(ref_surface(Nets(sd), inner)["sdf"].median())
    sd[f"{R}.4.weight_g"] = sd[f"{R}.4.weight_g"] * (RGB_LOGIT_RMS / float(_rgb_logits(sd, framework).pow(2).mean().sqrt()))
    return sd


def _rgb_logits(sd, framework):
    """The rgb layer's products (without its bias) over the state's query points, fp64."""
    nets = Nets(sd)
    pts, view = query_points(framework)
    s = ref_surface(nets, pts)
    o = B.ref_radiance_fwd(nets, pts, view, s["nabla"], s["h7"])
    return o["r"][3] @ nets.R[4].T


def check_state(sd, framework):
    """The conditions a state must meet, from the fp64 reference alone -> (list of failures, dict of measured figures)."""
    nets = Nets(sd)
    pts = query_points(framework)[0]
    o = B.ref_sdf_fwd2(nets, pts, torch.zeros_like(pts))
    ref = ref_surface(nets, pts)
    sdf, nab = ref["sdf"], ref["nabla"].norm(dim=-1)
    feat = ref["h7"] @ nets.W[8][1:].T + nets.b[8][1:]
    amax = max(float(a.abs().max()) for a in o["a"])
    view = query_points(framework)[1]
    rgb = ref_radiance(nets, pts, view, ref["nabla"], ref["h7"])
    gv = []
    for stem, nl in ((S, 9), (R, 5)):
        for l in range(nl):
            gv.append(float((sd[f"{stem}.{l}.weight_g"].reshape(-1) / sd[f"{stem}.{l}.weight_v"].norm(dim=1) - 1).abs().max()))
    fig = dict(sdf_min=float(sdf.min()), sdf_max=float(sdf.max()), neg=float((sdf < 0).double().mean()), pos=float((sdf > 0).double().mean()),
               near=int((sdf.abs() < 0.05).sum()), nabla_min=float(nab.min()), nabla_max=float(nab.max()), act_max=amax, feat_max=float(feat.abs().max()),
               g_over_v_min=min(gv), rgb_open=float(((rgb > 0.05) & (rgb < 0.95)).double().mean()))
    bad = []
    if fig["neg"] < 0.05 or fig["pos"] < 0.05:
        bad.append("sdf does not take both signs on 5 % of the points each")
    if fig["near"] < 20:
        bad.append("fewer than 20 points with |sdf| < 0.05")
    if fig["nabla_min"] < 0.1 or fig["nabla_max"] > 5:
        bad.append("|nabla| outside [0.1, 5]")
    if amax >= 4 or fig["feat_max"] >= 16:
        bad.append("a hidden activation >= 4 or a geometry feature >= 16: the fp16 tiers would be tested towards overflow")
    if any(not bool(sd[f"{S}.{l}.bias"].abs().max() > 0) for l in range(8)):
        bad.append("a zero hidden bias vector")
    if any(not bool(sd[f"{S}.{l}.weight_v"][:, -36 + 6 * k: -30 + 6 * k if k < 5 else None].abs().max() > 0) for l in (0, 4) for k in range(6)):
        bad.append("a zero encoding column block")
    if fig["g_over_v_min"] < 0.05:
        bad.append("max |g / |v| - 1| < 0.05 in a layer")
    if fig["rgb_open"] < 0.5:
        bad.append("more than half of the rgb elements within 0.05 of 0 or 1: the sigmoid would hide the radiance net's errors")
    return bad, fig


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------------
def ray_points(o, d, idx, depth, n_per_ray, dtype=F64):
    """x = o[idx] + d[idx] * depth[:, :n_per_ray], view = d[idx] per sample -> ([slots * n_per_ray, 3], the same).  In fp32: two roundings, as the kernels."""
    i = idx.long()
    oo, dd, t = o.to(dtype)[i][:, None, :], d.to(dtype)[i][:, None, :], depth.to(dtype)[:, :n_per_ray, None]
    x = oo + dd * t
    return x.reshape(-1, 3), dd.expand_as(x).reshape(-1, 3)


def clamp_sdf(sdf, x, R_bg):
    """VolSDF's sphere background min(sdf, R_bg - |x|); R_bg <= 0: no clamp.  nabla is never replaced."""
    return sdf if R_bg <= 0 else torch.minimum(sdf, R_bg - x.norm(dim=-1))


def ref_surface(nets, x, R_bg=0.0):
    """-> dict sdf (clamped), raw (unclamped), nabla [M, 3], h7 [M, 256] (feature order), fp64."""
    x = x.to(nets.device).double()
    h7, nab = B.sdf_h7_nabla(nets, x)
    raw = h7 @ nets.W[8][0] + nets.b[8][0]
    return dict(sdf=clamp_sdf(raw, x, R_bg), raw=raw, nabla=nab, h7=h7)


def ref_radiance(nets, x, view, nabla, h7):
    """rgb [M, 3] in fp64: geometry feature from h7, [x | view or its embedding (NeuS: multires 4) | nabla | feature] through the radiance net."""
    return B.ref_radiance_fwd(nets, x, view, nabla, h7)["rgb"]


# ---------------------------------------------------------------------------------------------------------------------------
# the stand-ins
# ---------------------------------------------------------------------------------------------------------------------------
MUTANTS = (
    "bias_roll",             # every hidden bias vector rolled by one element
    "bias_swap",             # two biases of one hidden layer exchanged: elements 4 g + r = 6 and 9 of tile 0 (g and r transposed), layer BIAS_SWAP_LAYER
    "tangent_bias",          # the bias added to the tangent lanes as well as to the value lane (forward mode)
    "ignore_g",              # weight_g ignored in the fold of one layer (W = v)
    "sincos_swap",           # sin and cos of band 5 exchanged
    "band_order",            # bands 3..5 evaluated at the frequencies of bands 0..2
    "skip_enc_dropped",      # the skip layer's encoding columns dropped
    "no_rsqrt2",             # the 1 / sqrt 2 of the skip missing
    "clamp_nabla",           # the sphere clamp replacing nabla as well (- x / |x| where it is active)
    "clamp_no_radius",       # the clamp applied with R_bg <= 0
    "tile_shift",            # the rows of the last ragged 16-point group shifted by one
    "h7_unit_order",         # h7 written in unit order instead of feature order
    "view_band_order",       # NeuS view embedding: [v, all sines, all cosines] instead of [v, sin, cos per band]
    "feat_bias_row",         # geometry-feature bias b8[0..255] instead of b8[1..256]
)
BIG_BIAS_LAYER = 1         # the layer whose biases the second state enlarges: the one of 0..7 with which check_state's conditions hold on both scenes
BIAS_SWAP_LAYER = BIG_BIAS_LAYER
IGNORE_G_LAYER = 6
TOUCHES = {"tangent_bias": ("nabla",), "clamp_nabla": ("nabla",), "clamp_no_radius": ("sdf",), "h7_unit_order": ("h7",), "view_band_order": ("rgb",), "feat_bias_row": ("rgb",),
           "tile_shift": ("sdf", "nabla", "h7", "rgb")}       # every other mutant: sdf, nabla and h7


def mutate_nets(nets, sd, mut):
    """The mutants that are a change of the weights the stand-in reads."""
    if mut not in WEIGHT_MUTANTS:
        return nets
    m = Nets.__new__(Nets)
    m.__dict__.update(nets.__dict__)
    m.W, m.b = [w.clone() for w in nets.W], [b.clone() for b in nets.b]
    if mut == "bias_roll":
        m.b[:8] = [torch.roll(b, 1) for b in m.b[:8]]
    elif mut == "bias_swap":
        m.b[BIAS_SWAP_LAYER][[6, 9]] = nets.b[BIAS_SWAP_LAYER][[9, 6]]
    elif mut == "ignore_g":
        m.W[IGNORE_G_LAYER] = sd[f"{S}.{IGNORE_G_LAYER}.weight_v"].to(nets.device).double()
    elif mut == "skip_enc_dropped":
        m.W[4][:, W3:] = 0.0
    elif mut == "no_rsqrt2":
        m.W[4] = m.W[4] * math.sqrt(2.0)
    elif mut == "feat_bias_row":
        m.b[8] = torch.cat([nets.b[8][:1], nets.b[8][:256]])
    return m


WEIGHT_MUTANTS = ("bias_roll", "bias_swap", "ignore_g", "skip_enc_dropped", "no_rsqrt2", "feat_bias_row")


def mutate_state(sd, mut):
    """The same faults as mutate_nets, as a state dict: what a kernel computes when its blob is packed from it is what a kernel with the fault computes
    on the true state.  (The fold g v / |v| stays the true one where a mutant changes v: g follows |v|.)"""
    assert mut in WEIGHT_MUTANTS
    out = {k: v.detach().clone() for k, v in sd.items()}
    if mut == "bias_roll":
        for l in range(8):
            out[f"{S}.{l}.bias"] = torch.roll(sd[f"{S}.{l}.bias"], 1)
    elif mut == "bias_swap":
        out[f"{S}.{BIAS_SWAP_LAYER}.bias"][[6, 9]] = sd[f"{S}.{BIAS_SWAP_LAYER}.bias"][[9, 6]]
    elif mut == "ignore_g":
        out[f"{S}.{IGNORE_G_LAYER}.weight_g"] = sd[f"{S}.{IGNORE_G_LAYER}.weight_v"].norm(dim=1, keepdim=True)
    elif mut == "skip_enc_dropped":
        v = out[f"{S}.4.weight_v"]
        v[:, W3:] = 0.0
        out[f"{S}.4.weight_g"] = sd[f"{S}.4.weight_g"] * (v.norm(dim=1, keepdim=True) / sd[f"{S}.4.weight_v"].norm(dim=1, keepdim=True))
    elif mut == "no_rsqrt2":
        out[f"{S}.4.weight_g"] = sd[f"{S}.4.weight_g"] * math.sqrt(2.0)
    elif mut == "feat_bias_row":
        out[f"{S}.8.bias"][1:] = sd[f"{S}.8.bias"][:256]
    return out


def _embed_pair(x, v, mut=None):
    """[x, sin f_k x, cos f_k x ...] and its tangent along v, in x's dtype."""
    e, t = [x], [v]
    for k in range(6):
        f = float(2 ** (k % 3 if mut == "band_order" else k))
        s, c, ds, dc = torch.sin(x * f), torch.cos(x * f), f * torch.cos(x * f) * v, -f * torch.sin(x * f) * v
        if mut == "sincos_swap" and k == 5:
            s, c, ds, dc = c, s, dc, ds
        e += [s, c]
        t += [ds, dc]
    return torch.cat(e, -1), torch.cat(t, -1)


def _f16(x):
    return x.half().float()


def _mm(x, w, tier, ready=False, kperm=None):
    """x [M, K] @ w [N, K]^T in the tier's arithmetic.  ready: x is a ready-made input unit (hi + lo kept in the fp16 tiers).  kperm: a permutation of k
    (another summation order, for the stand-in's own self-test)."""
    if kperm is not None:                                         # kperm: the seed of the permutation
        p = torch.randperm(x.shape[1], generator=torch.Generator().manual_seed(int(kperm) + x.shape[1])).to(x.device)
        x, w = x[:, p].contiguous(), w[:, p].contiguous()
    if tier == "fp32":
        return x @ w.T
    if tier == "bf16x3":
        xh, xl = _split(x)
        wh, wl = _split(w)
        return xh @ wh.T + xh @ wl.T + xl @ wh.T
    xh, wh = _f16(x), _f16(w)
    if ready:
        return xh @ wh.T + xh @ _f16(w - wh).T + _f16(x - xh) @ wh.T
    if tier == "fp16x2":
        return xh @ wh.T + xh @ _f16(w - wh).T
    return xh @ wh.T                                              # fp16x1


def _act(z, tier):
    """(softplus', activation) of a pre-activation in the tier's recursion."""
    if tier != "fp16x1":
        return _sig_soft(z)
    e = torch.exp2(-z.abs())                                       # z = c z_true: 2^-|z| = exp(-100 |z_true|)
    r = 1.0 / (1.0 + e)
    return torch.where(z >= 0, r, e * r), torch.relu(z) + torch.log2(1.0 + e)


def _layer_weights(nets, l, tier):
    """fp32 (w_hidden or None, w_enc or None, bias) of SDF layer l as the tier's blob holds them."""
    c = C_SCALE if tier == "fp16x1" else 1.0
    W, b = nets.W[l], nets.b[l] * c
    if l == 0:
        return None, (W * c).float(), b.float()
    if l == 4:
        return (W[:, :W3] * RS2).float(), (W[:, W3:] * (RS2 * c)).float(), b.float()
    return W.float(), None, b.float()


def standin_surface(nets, x, tier, mode="fwd", mut=None, kperm=None, want_nabla=True):
    """x [M, 3] fp32 -> dict raw (unclamped sdf), nabla, h7: fp32, before output rounding.  mode 'fwd': three tangent columns per point through the same
    products; 'rev': transposed-weight sweep over softplus' kept from the forward sweep."""
    dev = nets.device
    x = x.to(dev).float()
    M = x.shape[0]
    fwd = want_nabla and (mode == "fwd" or mut == "tangent_bias")
    rev = want_nabla and not fwd
    eye = torch.eye(3, device=dev)
    e, _ = _embed_pair(x, torch.zeros_like(x), mut)
    edots = [_embed_pair(x, eye[c].expand(M, 3), mut)[1] for c in range(3)] if want_nabla else []
    h, hd, D = None, None, []
    for l in range(8):
        wh, we, b = _layer_weights(nets, l, tier)
        z = b.expand(M, -1)
        if wh is not None:
            z = z + _mm(h, wh, tier, False, kperm)
        if we is not None:
            z = z + _mm(e, we, tier, True, kperm)
        d, a = _act(z, tier)
        if fwd:
            nd = []
            for c in range(3):
                t = 0.0
                if wh is not None:
                    t = t + _mm(hd[c], wh, tier, False, kperm)
                if we is not None:
                    t = t + _mm(edots[c], we, tier, True, kperm)
                if mut == "tangent_bias":
                    t = t + b
                nd.append(d * t)
            hd = nd
        D.append(d)
        h = a
    w8 = nets.W[8][0].float() / (C_SCALE if tier == "fp16x1" else 1.0)
    out = dict(raw=h @ w8 + nets.b[8][0].float(), h7=h / (C_SCALE if tier == "fp16x1" else 1.0), nabla=None)
    if fwd:
        out["nabla"] = torch.stack([hd[c] @ w8 for c in range(3)], -1)
    if rev:
        t, ge = w8.expand(M, 256), torch.zeros(M, 39, device=dev)
        for l in range(7, -1, -1):
            wh, we, _ = _layer_weights(nets, l, tier)
            q = tier != "fp32" and l < 7                              # softplus' of layers 0..6 parked as unorm16 (fp32 tier: fp32)
            Dl = torch.round(D[l].double().clamp(0, 1) * 65535.0).float() if q else D[l]
            if tier == "bf16x3" and q:
                td, s = t * Dl, 1.0 / 65535.0                         # the 1 / 65535 is folded into the transposed chunks
            else:
                td, s = (t * Dl) * (1.0 / 65535.0) if q else t * Dl, 1.0
            if we is not None:
                ge = ge + _mm(td, (we * s).T.contiguous(), tier, False, kperm)
            if wh is not None:
                t = _mm(td, (wh * s).T.contiguous(), tier, False, kperm)
        out["nabla"] = torch.stack([(ge * edots[c]).sum(-1) for c in range(3)], -1)
    return out


def _view_embed(view, nets, mut=None):
    if nets.multires_view < 0:
        return view
    ev = onets.embed(view, nets.multires_view)
    if mut == "view_band_order":
        s = [ev[:, 3 + 6 * k: 6 + 6 * k] for k in range(4)]
        c = [ev[:, 6 + 6 * k: 9 + 6 * k] for k in range(4)]
        ev = torch.cat([ev[:, :3]] + s + c, -1)
    return ev


def standin_radiance(nets, x, view, nabla, h7, tier, mut=None, kperm=None):
    """-> rgb [M, 3] fp32 before output rounding.  h7 and [x | view | n] are ready-made input units; the ReLU activations are built from accumulators."""
    dev = nets.device
    x, view, nabla, h7 = (t.to(dev).float() for t in (x, view, nabla, h7))
    f = _mm(h7, nets.W[8][1:].float(), tier, True, kperm) + nets.b[8][1:].float()
    ex = torch.cat([x, _view_embed(view, nets, mut), nabla], -1)
    nex, R0 = nets.nex, nets.R[0].float()
    h = torch.relu(_mm(f, R0[:, nex:].contiguous(), tier, False, kperm) + _mm(ex, R0[:, :nex].contiguous(), tier, True, kperm) + nets.rb[0].float())
    for l in range(1, 4):
        h = torch.relu(_mm(h, nets.R[l].float(), tier, False, kperm) + nets.rb[l].float())
    return torch.sigmoid(h @ nets.R[4].float().T + nets.rb[4].float())


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def tie_points(nets, R_bg, n=N_TIES, seed=5):
    """Points where R_bg - |x| and the reference sdf agree: bisection along n rays from the origin, in fp64, rounded to fp32."""
    g = torch.Generator().manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).double().to(nets.device)
    lo, hi = torch.zeros(n, dtype=F64, device=nets.device), torch.full((n,), float(R_bg), dtype=F64, device=nets.device)
    gap = lambda r: (R_bg - r) - ref_surface(nets, u * r[:, None])["raw"]
    assert bool((gap(lo) > 0).all()) and bool((gap(hi) < 0).all()), "no sign change of (R_bg - r) - sdf between the origin and the sphere"
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        pos = gap(mid) > 0
        lo, hi = torch.where(pos, mid, lo), torch.where(pos, hi, mid)
    return (u * lo[:, None]).float().cpu()


def case_points(nets, framework, n=1000, seed=11):
    """The point set of a case: query_points with row 0 the origin, rows 1..N_TIES on the tie of the sphere clamp (VolSDF) and the next row the largest |x|
    the product queries - the edge rows come first so that every size M > 5 has them."""
    p, v = query_points(framework, max(n, 16), seed)
    p, v = p[:n].clone(), v[:n].clone()
    p[0] = 0.0
    if n > N_TIES + 1:
        if R_BG[framework] > 0:
            p[1: 1 + N_TIES] = tie_points(nets, R_BG[framework])
        p[1 + N_TIES] = torch.tensor(FAR) / (1.0 if framework == "VolSDF" else 3.0)
    return p, v


def make_case(kind, framework, precision, nets, pts, view=None, R_bg=None, rays=None, sd=None, share=None):
    """kind 'sdf' | 'nabla' | 'rad'.  pts [M, 3] fp32 (or rays = dict(o, d, idx, depth, n_per_ray)).  A 'rad' case reads the reference's own h7 and
    nabla (rounded to fp32): the radiance kernels are held on their own.  share: a dict the cases of one point set and state pass around, so that the
    fp64 SDF reference is evaluated once for them."""
    tier, mode = PRECISION[precision]
    R_bg = R_BG[framework] if R_bg is None else R_bg
    c = dict(kind=kind, fw=framework, precision=precision, tier=tier, mode=mode, R_bg=float(R_bg), nets=nets, rays=rays, sd=sd, share=share)
    if rays is not None:
        c["x64"], c["view64"] = ray_points(rays["o"], rays["d"], rays["idx"], rays["depth"], rays["n_per_ray"], F64)
        c["x32"], c["view32"] = ray_points(rays["o"], rays["d"], rays["idx"], rays["depth"], rays["n_per_ray"], F32)
    else:
        c["x32"], c["x64"] = pts.float(), pts.double()
        c["view32"] = c["view64"] = None
        if view is not None:
            c["view32"], c["view64"] = view.float(), view.double()
    c["M"] = c["x32"].shape[0]
    c["id"] = f"{kind}-{framework}-p{precision}-R{R_bg:g}-{'rays' if rays is not None else 'pts'}-{c['M']}"
    return c


def reference(c):
    """The fp64 reference of a case (and, for 'rad', the fp32 h7 / nabla inputs it feeds every implementation)."""
    if "ref" not in c:
        share = c["share"] if c["share"] is not None else {}
        if "surface" not in share:
            share["surface"] = ref_surface(c["nets"], c["x64"])
        s = dict(share["surface"])
        s["sdf"] = clamp_sdf(s["raw"], c["x64"].to(c["nets"].device), c["R_bg"])
        if c["kind"] == "rad":
            c["h7_in"], c["nabla_in"] = s["h7"].float(), s["nabla"].float()
            c["ref"] = dict(rgb=ref_radiance(c["nets"], c["x64"], c["view64"], c["nabla_in"], c["h7_in"]))
        else:
            c["ref"] = dict(sdf=s["sdf"], raw=s["raw"]) if c["kind"] == "sdf" else dict(sdf=s["sdf"], raw=s["raw"], nabla=s["nabla"], h7=s["h7"])
    return c["ref"]


def standin(c, mut=None, kperm=None):
    """The stand-in through a case -> the dict of outputs the GPU test collects from the library (fp32, before output rounding)."""
    reference(c)
    nets = mutate_nets(c["nets"].kernel_view(), c["sd"], mut)
    x = c["x32"].to(nets.device)
    if c["kind"] == "rad":
        out = dict(rgb=standin_radiance(nets, x, c["view32"], c["nabla_in"], c["h7_in"], c["tier"], mut, kperm))
    else:
        s = standin_surface(nets, x, c["tier"], c["mode"] or "fwd", mut, kperm, want_nabla=c["kind"] == "nabla")
        R_bg = c["R_bg"]
        if mut == "clamp_no_radius" and R_bg <= 0:
            out = dict(sdf=torch.minimum(s["raw"], R_bg - x.norm(dim=-1)))
        else:
            out = dict(sdf=clamp_sdf(s["raw"], x, R_bg))
        if c["kind"] == "nabla":
            out["nabla"], out["h7"] = s["nabla"], s["h7"]
            if mut == "clamp_nabla" and R_bg > 0:
                on = (R_bg - x.norm(dim=-1)) < s["raw"]
                out["nabla"] = torch.where(on[:, None], -x / x.norm(dim=-1, keepdim=True).clamp_min(1e-30), out["nabla"])
            if mut == "h7_unit_order":
                out["h7"] = out["h7"][:, PERM.to(x.device)]
    if mut == "tile_shift":
        t0 = (c["M"] - 1) // 16 * 16
        for k, v in out.items():
            v = v.clone()
            v[t0 + 1:] = out[k][t0: c["M"] - 1]
            out[k] = v
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------------------
def allowances(c):
    """{output: A} of a case, from the reference and the clean stand-in."""
    if "A" not in c:
        ref, sim = reference(c), standin(c)
        c["A"] = {k: FACTOR * float((sim[k].double() - ref[k]).abs().max()) for k in sim}
    return c["A"]


def check(c, out, rows=None):
    """out: dict of the case's outputs (any float dtype).  rows: compare the first `rows` rows only (the sizes M of one case).
    -> (violations: list of str, max err / A per output: dict)."""
    ref, A = reference(c), allowances(c)
    viol, ratio = [], {}
    for k, a in A.items():
        if k not in out or out[k] is None:
            continue
        r = ref[k] if rows is None else ref[k][:rows]
        got = out[k].to(r.device).double()
        if got.shape != r.shape:
            viol.append(f"{c['id']} {k}: shape {tuple(got.shape)} instead of {tuple(r.shape)}")
            continue
        if not bool(torch.isfinite(got).all()):
            viol.append(f"{c['id']} {k}: {int((~torch.isfinite(got)).sum())} non-finite elements")
            continue
        err = (got - r).abs()
        ratio[k] = float(err.max()) / max(a, 1e-300) if err.numel() else 0.0
        if ratio[k] > 1.0:
            i = int(torch.argmax(err))
            viol.append(f"{c['id']} {k}: max err / A = {ratio[k]:.2f} (|got - ref| = {float(err.flatten()[i]):.3e}, A = {a:.3e}) at flat index {i} of {err.numel()}")
    return viol, ratio


def fmt(ratio):
    return "  ".join(f"{k} {v:.2f}" for k, v in ratio.items())
