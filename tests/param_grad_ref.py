"""References, models and comparator of the weight-gradient tail of pass 2: what turns the dumps of the per-sample backward kernels into .grad.

The code under test is the host sequences surf_param_bwd / rad_param_bwd of csrc/render_backward.hip (nerfart_wgrad_bf16 in place over the dumps,
k_h7_units, the add_sums kernels), k_fold and k_weight_norm_bwd, behind nerfart_sdf_param_bwd, nerfart_radiance_param_bwd, nerfart_fold_weight_grads,
nerfart_weight_norm_bwd and the two nerfart_*_render_bwd calls.  tests/test_param_grad_ref.py holds the references below to fp64 autograd on the CPU
and shows that the comparator rejects mutants; tests/test_gpu_param_grads.py holds the library to them.  Everything about the dumps themselves
(codecs, fp64 sweeps, the stand-in at the kernels' precision, the case matrix) is tests/mlp_bwd_ref.py's and is used from there.

1. THE RAW BUFFER (nerfart_pass2_raw_layout; kSectionFloats in csrc/render_backward.hip).  Sections, in floats, everything in the kernels' UNIT order
   (row / column k = 32 u + 8 g + e holds feature packing.unit_feature_hidden(u, g, e)); Mp = up(M, 64) for the SDF net, up(M, 128) for the radiance
   net; RZ[l] = the reverse dump's slot l = 65535 [zbar_l; t_l d_l], FA[l] = the forward dump's slot l = [a_l; adot_l], 2 Mp rows each:
       SURF_WW   [7][256][256]  RZ[l]^T FA[l - 1], l = 1..7, over all 2 Mp rows
       SURF_WE   [2][256][64]   RZ[0]^T E2 and RZ[4]^T E2, E2 = nerfart_wgrad_operand_embed_pair's [e; edot] (39 columns, no lo half: 39 > 32)
       SURF_CS0  [2][256]       column sums of the first Mp rows of RZ[0] (row 0) and of RZ[4] (row 1: WRITTEN - the two-matrix reduction of
                                SURF_WE produces it - and never read: the bias of layer 4 comes from SURF_CS17.  Held to the same bound as row 0.)
       SURF_CS17 [7][256]       column sums of the first Mp rows of RZ[1..7]
       SURF_W8   [256][64]      FA[7]^T SO, SO = nerfart_wgrad_operand_sbar_ones' [sbar; 1]: column 0 = a7^T hi(sbar) + column sums of adot7,
                                column 32 = a7^T lo(sbar); the other 62 columns of SO are zero: only zero is added to theirs (old + 0, the value kept)
       SURF_B8   [4]            sum of sbar; [1..3] never written
       RAD_WW    [4][256][256]  DEL[l]^T ACT[l] over Mp rows: (delta0, f), (delta1, r0), (delta2, r1), (delta3, r2)
       RAD_CS    [5][256]       column sums of DEL[0..3] over Mp rows; row 4: of DEL[4] = g_f over up(M, 64) rows
       RAD_W4    [256][64]      ACT[4]^T D4 (r3 against the output delta: hi columns 0..2, lo 32..34)
       RAD_B4    [4]            column sums of the fp32 output delta; [3] never written
       RAD_WEX   [256][64]      DEL[0]^T EX, EX = nerfart_wgrad_operand_inputs' [x | view | n] (nex = 9: hi 0..8, lo 32..40; nex = 33: hi 0..32 only)
       RAD_WH7   [256][256]     DEL[4]^T A7 over up(M, 64) rows, A7 = the layer-7 activation as bf16 in unit order
       SCALARS   [4]
   Features 217..255 of SDF layer 3 need no exception here: the reductions run over all 256 columns of whatever the dumps hold there (finite by the
   dumps' contract), so those rows / columns of SURF_WW[2], SURF_WW[3] and SURF_CS17[2] are held to the products like every other element.
   EVERY CALL ADDS to the sections it reduces into and touches no other.  The columns of the 64-wide sections that no operand column fills are
   rewritten as old + 0 (the reduction runs over all 64 columns): value kept for finite dumps.  Only SURF_B8[1..3] and RAD_B4[3] are never written.
   n of RAD_CS is per row: rows 0..3 are reduced with RAD_WW over Mp rows, row 4 with RAD_WH7 over up(M, 64) rows.

   ALLOWANCE (check_raw), per element:  |raw - P64| <= n 2^-23 S,  P64 the fp64 product of the decoded operands, S the same sum over absolute
   values, n = rows summed + split-K partials (nerfart_wgrad_workspace_bytes / the bytes of one partial result).  bf16 x bf16 is exact in fp32 and
   any summation order errs by at most one rounding per addition; 2^-23 instead of 2^-24 because nobody has established that the matrix unit's
   internal accumulation rounds to nearest.  S == 0: the element must be exactly 0 (a zeroed raw is what the comparison starts from).

2. THE FOLD (fold_model): raw -> the 28 pieces of nerfart_folded_grads_layout, written from the layout documented in include/nerfart_hip.h and
   above - one add of the hi and lo halves where the operand fits 32 columns, one multiply by 1 / 65535 (SDF layers 0..7: their reverse dump
   carries the factor) or by 1 / 65535 * 1 / sqrt 2 (the skip layer 4), un-permutation unit order -> feature order on both axes.  The same fp32
   operations, so the expected values are exact; check_fold allows one fp32 ulp.

3. THE weight_norm CHAIN RULE (wn_bwd64):  g_g = (dW . v) / |v|,  g_v = g / |v| (dW - v (dW . v) / |v|^2)  per output row.

4. END TO END (ref_param_grads): an fp64 torch model on leaf weight_g / weight_v / bias: W = g v / |v|, the 9 SDF layers with softplus beta 100, the
   skip and the embedding through mlp_bwd_ref.ref_sdf_fwd2's value + tangent sweep, loss  sbar . sdf + hbar7 . h7 + nbar . grad_x sdf;  the 5
   radiance layers with the ReLU signs GIVEN (from the forward dump of the route under test, as mlp_bwd_ref.ref_radiance_bwd takes them), loss
   g_rgb . rgb.  Allowance per parameter tensor and element:  FACTOR max |sim - ref| over the tensor + the allowance of 1 carried through fold and
   chain rule in absolute values; sim = the stand-in's dumps -> fp64 products -> fold_model in fp64 -> wn_bwd64.
"""
import numpy as np
import torch

import mlp_bwd_ref as R
from mlp_bwd_ref import F32, F64, FACTOR, POS, up

EPS = 2.0 ** -23
SECTIONS = ("SURF_WW", "SURF_WE", "SURF_CS0", "SURF_CS17", "SURF_W8", "SURF_B8", "RAD_WW", "RAD_CS", "RAD_W4", "RAD_B4", "RAD_WEX", "RAD_WH7", "SCALARS")
SHAPES = dict(SURF_WW=(7, 256, 256), SURF_WE=(2, 256, 64), SURF_CS0=(2, 256), SURF_CS17=(7, 256), SURF_W8=(256, 64), SURF_B8=(4,),
              RAD_WW=(4, 256, 256), RAD_CS=(5, 256), RAD_W4=(256, 64), RAD_B4=(4,), RAD_WEX=(256, 64), RAD_WH7=(256, 256), SCALARS=(4,))
SDF_SECTIONS, RAD_SECTIONS = SECTIONS[:6], SECTIONS[6:12]
NENC = 39                                   # columns of the SDF net's encoding (multires 6)
S_STEM, R_STEM = "implicit_surface.surface_fc_layers", "radiance_net.layers"

# the sizes of parts 1 and 4 (the smallest at which this path can go wrong): (kind, framework, M)
SDF_M = (1, 63, 65, 200, 300)               # 300: 2 Mp = 640 rows, the first size at which pick_split gives two workgroups per matrix
RAD_M = (1, 127, 129, 300, 520)             # 520: up(M, 128) = 640 and up(M, 64) = 576 both split, and the two paddings differ


def specs():
    s = [("sdf", "VolSDF", M) for M in SDF_M] + [("sdf", "NeuS", 65)]
    return s + [("rad", fw, M) for fw in ("VolSDF", "NeuS") for M in RAD_M]


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def raw_offsets():
    """({section: float offset}, total) as kSectionFloats documents it."""
    o, offs = 0, {}
    for s in SECTIONS:
        offs[s] = o
        o += numel(SHAPES[s])
    return offs, o


def section(raw, name):
    """A view of one section of a flat raw buffer (torch or numpy)."""
    o = raw_offsets()[0][name]
    return raw[o: o + numel(SHAPES[name])].reshape(SHAPES[name])


def assemble(sections, dtype=F64):
    """{section: tensor} -> flat raw buffer, the sections not given zero."""
    raw = torch.zeros(raw_offsets()[1], dtype=dtype)
    for k, v in sections.items():
        section(raw, k).copy_(v)
    return raw


# ---------------------------------------------------------------------------------------------------------------------------
# 1. operands and reductions
# ---------------------------------------------------------------------------------------------------------------------------
def units(raw_u8, *shape):
    """uint8 bytes of bf16 -> fp64 [*shape] in UNIT order (no un-permutation)."""
    return raw_u8.cpu().contiguous().view(torch.bfloat16).view(*shape).double()


def narrow_bytes(x, rows_pad):
    """Model of the nerfart_wgrad_operand_* layout: x [M, c] fp32 -> bytes of [rows_pad, 64] bf16: hi = bf16(x) in columns 0..c-1 and, when c <= 32,
    lo = bf16(x - hi) in columns 32..32+c-1; rows M.. zero."""
    M, c = x.shape
    out = torch.zeros(rows_pad, 64, dtype=F32)
    hi = R._hi(x.float())
    out[:M, :c] = hi
    if c <= 32:
        out[:M, 32: 32 + c] = R._hi(x.float() - hi)
    return out.to(torch.bfloat16).view(torch.uint8).reshape(-1)


def a7_bytes(h7, M):
    """The bf16 round-to-nearest-even of h7 [M, 256] in unit order, up(M, 64) rows, rows M.. zero: what k_h7_units builds."""
    return R.encode_bf16(R._pad_rows(h7.float().cpu(), up(M, 64)))


def sdf_operands(M, f2, r2, E2, SO, sbar):
    """Bytes of the two dumps and the two narrow operands, sbar [M] fp32 -> decoded fp64 operands."""
    Mp = up(M, 64)
    return dict(kind="sdf", M=M, Mp=Mp, FA=units(f2[: 8 * 2 * Mp * 512], 8, 2 * Mp, 256), RZ=units(r2, 8, 2 * Mp, 256),
                E2=units(E2, 2 * Mp, 64), SO=units(SO, 2 * Mp, 64), sbar=sbar.detach().cpu().double())


def rad_operands(M, fdump, bdump, D4, EX, A7, d4):
    """Bytes of the two dumps, the two narrow operands and a7; d4 [M, 3] fp32: the output delta."""
    Mp, Mp64 = up(M, 128), up(M, 64)
    return dict(kind="rad", M=M, Mp=Mp, Mp64=Mp64, ACT=units(fdump, 5, Mp, 256), DEL=units(bdump, 5, Mp, 256), D4=units(D4, Mp, 64),
                EX=units(EX, Mp, 64), A7=units(A7, Mp64, 256), d4=d4.detach().cpu().double())


REDUCE_MUTANTS = ("transposed", "act_same_layer", "no_tangent_rows", "cs_all_rows", "ragged_row_dropped", "narrow_lo_dropped", "w8_no_adot_sums")


def reduce_sections(op, dtype=F64, absolute=False, mut=None, train_radiance=True):
    """The sections one entry-point call adds to raw, from the decoded operands.  dtype fp64: the reference product P64 (absolute: S, the same sums
    over absolute values); fp32: a model of the library's reductions in another summation order.  mut: REDUCE_MUTANTS."""
    f = (lambda t: t.abs().to(dtype)) if absolute else (lambda t: t.to(dtype))
    M, Mp = op["M"], op["Mp"]
    out = {}
    if op["kind"] == "sdf":
        FA, RZ, E2, SO, sbar = (f(op[k]) for k in ("FA", "RZ", "E2", "SO", "sbar"))
        rows = slice(0, Mp if mut == "no_tangent_rows" else 2 * Mp)
        cs = slice(0, 2 * Mp if mut == "cs_all_rows" else Mp)
        if mut == "ragged_row_dropped" and M % 64:
            RZ = RZ.clone()
            RZ[:, M - 1] = 0
            RZ[:, Mp + M - 1] = 0
        if mut == "narrow_lo_dropped":
            SO = SO.clone()
            SO[:, 32:] = 0
        if mut == "w8_no_adot_sums":
            SO = SO.clone()
            SO[Mp:] = 0
        ww = [RZ[l, rows].T @ FA[l if mut == "act_same_layer" else l - 1, rows] for l in range(1, 8)]
        if mut == "transposed":
            ww[1] = ww[1].T
        out["SURF_WW"] = torch.stack(ww)
        out["SURF_WE"] = torch.stack([RZ[0, rows].T @ E2[rows], RZ[4, rows].T @ E2[rows]])
        out["SURF_CS0"] = torch.stack([RZ[0, cs].sum(0), RZ[4, cs].sum(0)])
        out["SURF_CS17"] = RZ[1:, cs].sum(1)
        out["SURF_W8"] = FA[7, rows].T @ SO[rows]
        b8 = torch.zeros(4, dtype=dtype)
        b8[0] = sbar.sum()
        out["SURF_B8"] = b8
        return out
    ACT, DEL, D4, EX, A7, d4 = (f(op[k]) for k in ("ACT", "DEL", "D4", "EX", "A7", "d4"))
    Mp64 = op["Mp64"]
    if mut == "ragged_row_dropped" and M % 128:
        DEL = DEL.clone()
        DEL[:, M - 1] = 0
    out["RAD_WH7"] = DEL[4, :Mp64].T @ A7
    rcs = torch.zeros(5, 256, dtype=dtype)
    rcs[4] = DEL[4, :Mp64].sum(0)
    if train_radiance:
        out["RAD_WW"] = torch.stack([DEL[l].T @ ACT[l] for l in range(4)])
        rcs[:4] = DEL[:4].sum(1)
        out["RAD_W4"] = ACT[4].T @ D4
        b4 = torch.zeros(4, dtype=dtype)
        b4[:3] = d4.sum(0)
        out["RAD_B4"] = b4
        out["RAD_WEX"] = DEL[0].T @ EX
    out["RAD_CS"] = rcs
    return out


def pick_split_model(n_mats, rows, cus=256):
    """pick_split of csrc/wgrad.hip on a 256-CU device: workgroups per matrix."""
    return max(1, min((2 * cus) // n_mats, ((rows + 31) // 32) // 8, 512))


def lib_split(lib):
    """Split-K partials of one nerfart_wgrad_bf16 call, from the library's own workspace size."""
    return lambda n_mats, rows, a_cols: int(lib.nerfart_wgrad_workspace_bytes(n_mats, rows, a_cols)) // (n_mats * (256 * a_cols + 256) * 4)


def additions(kind, M, split=None):
    """n of the allowance per section: rows summed + partial results added up.  split(n_mats, rows, a_cols) -> split-K partials."""
    split = split or (lambda n_mats, rows, a_cols: pick_split_model(n_mats, rows))
    if kind == "sdf":
        Mp = up(M, 64)
        return dict(SURF_WW=2 * Mp + split(7, 2 * Mp, 256), SURF_CS17=Mp + split(7, 2 * Mp, 256), SURF_WE=2 * Mp + split(2, 2 * Mp, 64),
                    SURF_CS0=Mp + split(2, 2 * Mp, 64), SURF_W8=2 * Mp + split(1, 2 * Mp, 64), SURF_B8=M + (M + 1023) // 1024)
    Mp, Mp64 = up(M, 128), up(M, 64)
    nb = (Mp + 31) // 32                                         # block sums of the output delta, then add_sums over them
    # RAD_CS per row ([5, 1], broadcasts over the columns): rows 0..3 ride with RAD_WW over Mp rows, row 4 with RAD_WH7 over up(M, 64) rows
    n_cs = torch.tensor([[Mp + split(4, Mp, 256)]] * 4 + [[Mp64 + split(1, Mp64, 256)]], dtype=F64)
    return dict(RAD_WW=Mp + split(4, Mp, 256), RAD_CS=n_cs, RAD_W4=Mp + split(1, Mp, 64),
                RAD_WEX=Mp + split(1, Mp, 64), RAD_WH7=Mp64 + split(1, Mp64, 256), RAD_B4=Mp + nb + (nb + 1023) // 1024)


def check_raw(rep, raw, P, S, n, extra=0):
    """Every section of P against the flat raw buffer (which started from zero): |raw - P| <= (n + extra) 2^-23 S per element; S == 0: exactly 0.
    -> {section: worst observed / allowed}."""
    worst = {}
    for name in P:
        got = section(raw, name).detach().cpu().double()
        if not rep.finite(f"raw.{name}", got):
            continue
        allow = (n[name] + extra) * EPS * S[name]
        err = (got - P[name]).abs()
        dead = S[name] == 0
        if bool((got[dead] != 0).any()):
            rep.fail(f"raw.{name}", f"{int((got[dead] != 0).sum())} elements no operand reaches are not what the call started from")
        ratio = float((err[~dead] / allow[~dead]).max()) if bool((~dead).any()) else 0.0
        worst[name] = ratio
        rep.note(f"raw.{name}", ratio)
        if ratio > 1.0:
            i = int(torch.argmax(torch.where(dead, torch.zeros_like(err), err / allow.clamp_min(1e-300))))
            rep.fail(f"raw.{name}", f"observed / allowed = {ratio:.3g} (|raw - P64| = {float(err.flatten()[i]):.3e}, allowed "
                                    f"{float(allow.flatten()[i]):.3e}) at flat index {i} of the section")
    return worst


def allowance_raw(S, n, extra=0):
    """The allowance of part 1 as a flat raw buffer (fp64)."""
    return assemble({k: (n[k] + extra) * EPS * S[k] for k in S})


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fold
# ---------------------------------------------------------------------------------------------------------------------------
def folded_layout(multires=6, multires_view=-1):
    """[(name, shape)] of the 28 pieces: (dW_l [out, in], db_l [out]) for the SDF net's layers 0..8, then the radiance net's 0..4."""
    nenc = 3 + 6 * multires
    nex = 3 + (3 if multires_view < 0 else 3 + 6 * multires_view) + 3
    out = []
    for l in range(9):
        o, i = (257 if l == 8 else 256 - nenc if l == 3 else 256), (nenc if l == 0 else 256)
        out += [(f"sdf.{l}.dW", (o, i)), (f"sdf.{l}.db", (o,))]
    for l in range(5):
        o, i = (3 if l == 4 else 256), (nex + 256 if l == 0 else 256)
        out += [(f"rad.{l}.dW", (o, i)), (f"rad.{l}.db", (o,))]
    return out


def folded_offsets(multires=6, multires_view=-1):
    offs = [0]
    for _, shp in folded_layout(multires, multires_view):
        offs.append(offs[-1] + numel(shp))
    return offs


FOLD_MUTANTS = ("no_65535", "no_rsqrt2_skip", "skip_enc_from_we0", "bias_neighbour_row", "unperm_one_axis", "fold_lo_dropped")


def fold_model(raw, multires=6, multires_view=-1, mut=None):
    """raw: flat numpy array (float32: the library's arithmetic; float64: the reference route) -> {piece name: array} in feature order."""
    dt = raw.dtype.type
    pos = POS.numpy()
    nenc = 3 + 6 * multires
    nex = 3 + (3 if multires_view < 0 else 3 + 6 * multires_view) + 3
    hw = 256 - nenc
    sc = dt(1.0) if mut == "no_65535" else dt(1.0) / dt(65535.0)
    sc4 = sc * (dt(1.0) if mut == "no_rsqrt2_skip" else dt(0.70710678118654752440))
    S = {k: section(raw, k) for k in SECTIONS}

    def both(m):                                                  # [256 units, 256 units] -> [feature, feature]
        return m[pos] if mut == "unperm_one_axis" else m[pos][:, pos]

    def halves(m, c):                                             # [256, 64] -> [256, c]: hi + lo where the operand fits 32 columns
        return m[:, :c] + m[:, 32: 32 + c] if c <= 32 and mut != "fold_lo_dropped" else m[:, :c]

    out = {}
    for l in range(9):
        if l == 0:
            w = halves(S["SURF_WE"][0], nenc)[pos] * sc
        elif l == 4:
            enc = halves(S["SURF_WE"][0 if mut == "skip_enc_from_we0" else 1], nenc)[pos]
            w = np.concatenate([both(S["SURF_WW"][3])[:, :hw], enc], 1) * sc4
        elif l == 8:
            w = np.concatenate([halves(S["SURF_W8"], 1)[pos].T, both(S["RAD_WH7"])], 0)
        else:
            w = both(S["SURF_WW"][l - 1])[: (hw if l == 3 else 256)] * sc
        if l == 0:
            b = S["SURF_CS0"][0][pos] * sc
        elif l == 8:
            b = np.concatenate([S["SURF_B8"][:1], S["RAD_CS"][4][pos]])
        else:
            row = l - 1 + (1 if mut == "bias_neighbour_row" and l == 5 else 0)
            b = (S["SURF_CS17"][row][pos] * sc)[: (hw if l == 3 else 256)]
        out[f"sdf.{l}.dW"], out[f"sdf.{l}.db"] = w, b
    for l in range(5):
        if l == 0:
            w = np.concatenate([halves(S["RAD_WEX"], nex)[pos], both(S["RAD_WW"][0])], 1)
        elif l == 4:
            w = halves(S["RAD_W4"], 3)[pos].T
        else:
            w = both(S["RAD_WW"][l])
        out[f"rad.{l}.dW"] = w
        out[f"rad.{l}.db"] = S["RAD_B4"][:3] if l == 4 else S["RAD_CS"][l][pos]
    for (name, shp) in folded_layout(multires, multires_view):
        assert out[name].shape == shp, (name, out[name].shape, shp)
        out[name] = np.ascontiguousarray(out[name])
    return out


def fold_unread(multires=6, multires_view=-1):
    """Boolean mask over the flat raw buffer: the slots nerfart_fold_weight_grads must not read."""
    nenc = 3 + 6 * multires
    nex = 3 + (3 if multires_view < 0 else 3 + 6 * multires_view) + 3
    m = np.zeros(raw_offsets()[1], dtype=bool)
    dead = POS.numpy()[256 - nenc:]                               # unit positions of features 217..255

    def narrow(name, c, lead=()):
        v = section(m, name)[lead]
        if c <= 32:
            v[:, c:32] = True
            v[:, 32 + c:] = True
        else:
            v[:, c:] = True                                       # single half: the lo half does not exist

    section(m, "SURF_CS0")[1] = True
    section(m, "SURF_WW")[2][dead, :] = True                      # layer 3 has 217 outputs
    section(m, "SURF_CS17")[2][dead] = True
    section(m, "SURF_WW")[3][:, dead] = True                      # ... so the skip layer has 217 hidden inputs
    narrow("SURF_WE", nenc, 0)
    narrow("SURF_WE", nenc, 1)
    narrow("SURF_W8", 1)
    narrow("RAD_W4", 3)
    narrow("RAD_WEX", nex)
    section(m, "SURF_B8")[1:] = True
    section(m, "RAD_B4")[3:] = True
    section(m, "SCALARS")[:] = True
    return m


def ulps32(got, want):
    """Distance in fp32 units in the last place between two float32 arrays (same sign or zero assumed where close)."""
    a = np.ascontiguousarray(got, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(want, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def check_fold(rep, got, want):
    """{piece: float32 array} twice -> worst ulp distance; more than one fp32 ulp anywhere is a violation naming the piece."""
    worst = 0
    for name, w in want.items():
        g = np.asarray(got[name], dtype=np.float32).reshape(w.shape)
        if not np.isfinite(g).all():
            rep.fail(f"fold.{name}", f"{int((~np.isfinite(g)).sum())} non-finite elements")
            continue
        d = ulps32(g, w)
        worst = max(worst, int(d.max()))
        if d.max() > 1:
            i = int(d.argmax())
            rep.fail(f"fold.{name}", f"{int((d > 1).sum())} elements off by more than 1 ulp (worst {int(d.max())} ulps at flat index {i}: "
                                     f"got {g.flatten()[i]!r}, want {w.flatten()[i]!r})")
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the weight_norm chain rule
# ---------------------------------------------------------------------------------------------------------------------------
def wn_bwd64(dW, v, g, no_projection=False):
    """fp64 tensors dW [out, in], v [out, in], g [out] or [out, 1] -> (g_g [out], g_v [out, in])."""
    dW, v, g = dW.double(), v.double(), g.double().reshape(-1)
    n2 = (v * v).sum(1)
    dot = (dW * v).sum(1)
    nrm = n2.sqrt()
    proj = torch.zeros_like(v) if no_projection else v * (dot / n2)[:, None]
    return dot / nrm, (g / nrm)[:, None] * (dW - proj)


def wn_bwd32_pairwise(dW, v, g):
    """The same formula in float32 numpy, the dots summed pairwise (numpy's reduction): the yardstick of part 3's allowance."""
    dW, v, g = (np.ascontiguousarray(t, dtype=np.float32) for t in (dW, v, np.reshape(g, -1)))
    n2 = (v * v).sum(1, dtype=np.float32)
    dot = (dW * v).sum(1, dtype=np.float32)
    nrm = np.sqrt(n2)
    inv = np.float32(1.0) / nrm
    return dot * inv, (g * inv)[:, None] * (dW - v * (dot / n2)[:, None])


def wn_abs(EdW, v, g):
    """A per-element bound on dW's error carried through the chain rule in absolute values -> (E_g_g, E_g_v)."""
    v, g = v.double().abs(), g.double().reshape(-1).abs()
    nrm = (v * v).sum(1).sqrt()
    edot = (EdW * v).sum(1)
    return edot / nrm, (g / nrm)[:, None] * (EdW + v * (edot / nrm ** 2)[:, None])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------------------------------------------------------
def param_names(kind):
    """The parameter tensors an entry point produces gradients of: (short name, state-dict stem, layer)."""
    if kind == "sdf":
        return [(f"sdf.{l}", S_STEM, l) for l in range(9)]
    return [(f"rad.{l}", R_STEM, l) for l in range(5)] + [("sdf.8", S_STEM, 8)]


def leaf_nets(sd):
    """A mlp_bwd_ref.Nets whose folded weights W = g v / |v| and biases hang on fp64 LEAVES -> (nets, {state-dict key: leaf})."""
    leaves = {}
    n = R.Nets.__new__(R.Nets)
    for attr, battr, stem, cnt in (("W", "b", S_STEM, 9), ("R", "rb", R_STEM, 5)):
        Ws, bs = [], []
        for l in range(cnt):
            for k in ("weight_g", "weight_v", "bias"):
                leaves[f"{stem}.{l}.{k}"] = sd[f"{stem}.{l}.{k}"].detach().cpu().double().clone().requires_grad_(True)
            g, v = leaves[f"{stem}.{l}.weight_g"], leaves[f"{stem}.{l}.weight_v"]
            Ws.append(g.reshape(-1, 1) * v / (v * v).sum(1, keepdim=True).sqrt())
            bs.append(leaves[f"{stem}.{l}.bias"])
        setattr(n, attr, Ws)
        setattr(n, battr, bs)
    n.nex = n.R[0].shape[1] - 256
    n.multires_view = -1 if n.nex == 9 else 4
    n.view_tiles = 1 if n.nex == 9 else 3
    n.device = "cpu"
    return n, leaves


def _grads(loss, leaves, kind):
    keys = [(f"{name}.{k}", f"{stem}.{l}.{k}") for name, stem, l in param_names(kind) for k in ("weight_g", "weight_v", "bias")]
    gs = torch.autograd.grad(loss, [leaves[k] for _, k in keys], allow_unused=True)
    return {short: (torch.zeros_like(leaves[k]) if g is None else g) for (short, k), g in zip(keys, gs)}


def ref_param_grads(sd, case, masks=None):
    """fp64 gradients of every parameter tensor of the case's entry point -> {'sdf.3.weight_v': tensor, ...}.
    sdf: loss = gbar_sdf . sdf + gbar_h7 . h7 + dir . grad_x sdf (the tangent sweep along dir).  rad: loss = g_rgb . rgb with the ReLU signs
    `masks` (list of 4 boolean [M, 256]) given."""
    n, leaves = leaf_nets(sd)
    if case["kind"] == "sdf":
        o = R.ref_sdf_fwd2(n, case["pts"], case["dir"])
        h7 = o["a"][7]
        sdf = h7 @ n.W[8][0] + n.b[8][0]
        loss = (case["gbar_sdf"].double() * sdf).sum() + (case["gbar_h7"].double() * h7).sum() + (o["adot"][7] @ n.W[8][0]).sum()
        return _grads(loss, leaves, "sdf")
    pts, view, nabla, h7 = (case[k].double() for k in ("pts", "view", "nabla", "h7"))
    f = h7 @ n.W[8][1:].T + n.b[8][1:]
    h = torch.cat([R.rad_inputs(n, pts, view, nabla), f], -1)
    for l in range(4):
        h = (h @ n.R[l].T + n.rb[l]) * masks[l].double()
    rgb = torch.sigmoid(h @ n.R[4].T + n.rb[4])
    return _grads((case["g_rgb"].double() * rgb).sum(), leaves, "rad")


def standin_operands(case, dumps):
    """The stand-in's dumps (mlp_bwd_ref.run_standin) + models of the narrow operands -> decoded operands."""
    M = case["M"]
    if case["kind"] == "sdf":
        Mp = up(M, 64)
        e, edot = R.embed_pair(case["pts"].float(), case["dir"].float())
        E2 = torch.cat([narrow_bytes(e, Mp), narrow_bytes(edot, Mp)])
        ones = torch.zeros(Mp, 64, dtype=F32)
        ones[:, 0] = 1.0
        SO = torch.cat([narrow_bytes(case["gbar_sdf"].float()[:, None], Mp), ones.to(torch.bfloat16).view(torch.uint8).reshape(-1)])
        return sdf_operands(M, dumps["f2"], dumps["r2"], E2, SO, case["gbar_sdf"])
    Mp = up(M, 128)
    rgb = dumps["rgb"].float().cpu()
    d4 = case["g_rgb"].float() * rgb * (1.0 - rgb)
    ex = R.rad_inputs(case["nets"], case["pts"].float(), case["view"].float(), case["nabla"].float()).float()
    return rad_operands(M, dumps["fdump"], dumps["bdump"], narrow_bytes(d4, Mp), narrow_bytes(ex, Mp), a7_bytes(case["h7"], M), d4)


def dump_masks(fdump, M):
    """The ReLU signs of a radiance forward dump, feature order: list of 4 boolean [M, 256]."""
    acts = R.decode_rad(fdump.cpu(), M)
    return [acts[1 + l, :M] != 0 for l in range(4)]


def grads_from_raw(raw, sd, kind, multires_view, fold=None, wn=None):
    """The route raw -> fold_model (in raw's own precision) -> wn_bwd64 -> {name: fp64 tensor}.  fold(raw as numpy) -> {piece: array} and
    wn(dW, v, g) -> (g_g, g_v) replace a stage."""
    raw = raw.detach().cpu().numpy() if isinstance(raw, torch.Tensor) else raw
    pieces = (fold or (lambda r: fold_model(r, 6, multires_view)))(raw)
    out = {}
    for name, stem, l in param_names(kind):
        dW = torch.as_tensor(np.array(pieces[f"{name}.dW"], dtype=np.float64))
        v, g = sd[f"{stem}.{l}.weight_v"].detach().cpu(), sd[f"{stem}.{l}.weight_g"].detach().cpu()
        g_g, g_v = (wn or wn_bwd64)(dW, v, g)
        out[f"{name}.weight_g"] = g_g.reshape(g.shape)
        out[f"{name}.weight_v"] = g_v
        out[f"{name}.bias"] = torch.as_tensor(np.array(pieces[f"{name}.db"], dtype=np.float64))
    return out


def allowance_grads(E_raw, sd, kind, multires_view):
    """The part-1 allowance (flat fp64 raw buffer) carried through the fold (a non-negative linear map) and the chain rule in absolute values."""
    pieces = fold_model(E_raw.double().numpy(), 6, multires_view)
    out = {}
    for name, stem, l in param_names(kind):
        E = torch.as_tensor(pieces[f"{name}.dW"])
        v, g = sd[f"{stem}.{l}.weight_v"].detach().cpu(), sd[f"{stem}.{l}.weight_g"].detach().cpu()
        e_g, e_v = wn_abs(E, v, g)
        out[f"{name}.weight_g"], out[f"{name}.weight_v"], out[f"{name}.bias"] = e_g.reshape(g.shape), e_v, torch.as_tensor(pieces[f"{name}.db"])
    return out


def sim_param_grads(sd, case, split=None):
    """(sim, acc): the stand-in route's gradients (run_standin's dumps -> fp64 products -> fold_model -> wn_bwd64) and the part-1 allowance of
    the same operands carried through."""
    op = standin_operands(case, R.run_standin(case))
    mv = case["nets"].multires_view
    P, S = reduce_sections(op), reduce_sections(op, absolute=True)
    n = additions(case["kind"], case["M"], split)
    return grads_from_raw(assemble(P), sd, case["kind"], mv), allowance_grads(allowance_raw(S, n), sd, case["kind"], mv)


def check_param_grads(rep, got, ref, sim, acc):
    """Per parameter tensor and element: |got - ref| <= FACTOR max |sim - ref| + acc.  -> {group: worst observed / allowed}."""
    worst = {}
    for name, r in ref.items():
        g = got[name].detach().cpu().double().reshape(r.shape)
        if not rep.finite(f"grad.{name}", g):
            continue
        A = FACTOR * float((sim[name].reshape(r.shape) - r).abs().max())
        allow = A + acc[name].reshape(r.shape)
        err = (g - r).abs()
        if float(allow.max()) == 0.0:                            # nothing reaches this tensor (row 0 of W8 on the radiance route is checked apart)
            ratio = 0.0 if float(err.max()) == 0.0 else float("inf")
        else:
            ratio = float((err / allow.clamp_min(1e-300)).max())
        grp = name.split(".")[0] + "." + name.split(".")[2]
        worst[grp] = max(worst.get(grp, 0.0), ratio)
        rep.note(f"grad.{name}", ratio)
        if ratio > 1.0:
            i = int(torch.argmax(err / allow.clamp_min(1e-300)))
            rep.fail(f"grad.{name}", f"observed / allowed = {ratio:.3g} (|got - ref| = {float(err.flatten()[i]):.3e}, allowed "
                                     f"{float(allow.flatten()[i]):.3e}, A = {A:.3e}) at flat index {i}")
    return worst


def new_report(cid):
    return R._Report(cid)
