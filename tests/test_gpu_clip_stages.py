"""The CLIP ViT-B/32 image encoder (csrc/clip_vit.hip, k_gemm of csrc/gemm_f16.h) stage by stage, forward and backward, against the fp64 references
and the error model of tests/clip_ref.py, through hip.lib and ctypes.  The workspace is filled with 0xffffffff (NaN) before every forward and read
back through nerfart_clip_vitb32_workspace_layout; every buffer is compared with the fp64 evaluation of its stage on the kernels' own stored input.
The backward keeps only the last block's scratch, so it is run 13 times through nerfart_clip_vitb32_image_bwd_partial (stop_layer 12, 11, .. 0): the
run to l + 1 leaves the dx that enters block l, the run to l everything block l writes.  One line per case: the worst observed / bound ratio per
buffer (1.00 = the bound; 0.000 on an exact buffer = bit for bit).

Worst observed / bound ratio per buffer over the 16 cases (4 weight cases x 2 images x B = 1, 3) on an MI355X (gfx950; every case passed):
  bit for bit         patches, xemb, scale, g16, g_img (= d patches x scale[1]), the non-class rows of dx after the head, the g_img of images whose
                      cotangent is zero, the zero padding rows of patches / x0 / att / act / y, nothing written past feat or g_img
  forward             xin0 (ln_pre) 0.987   qkv 0.367   xmid 0.049   pre 0.293   xin / xfin 0.031   att 0.513   x0 0.987   act 1.000 (0.9995: an
                      entry whose exact value 2^-25 is the tie between 0 and the smallest fp16 subnormal - the absolute term met exactly)
  backward            dx after the head 0.103   per block: act 0.981   att 0.240   dqkv 0.990   t 0.063   dx 0.114   tail: y 0.993
  fp32-output GEMMs   pe 0.000   feat 0.001   t0 0.001   d patches 0.001 (the block's t, K = 2304, is the 0.063 above): the assumed one ulp per MFMA addition times K, all with one sign, is three
                      orders of magnitude above what 768 .. 3072 rounded additions do.  The bound is still about 2 % of a typical entry (3.7e-4 S
                      at K = 3072, S about 55 typical entries), so these checks pin every index, a dropped k-tile, a missing bias - not the rounding.
  The ratios near 1 are buffers whose bound IS one fp16 rounding of the output (x0, y, act, dqkv; xin0: one fp32 rounding on entries with a
  near-zero gain): the half-ulp is reached by some entry among 10^5.  The numpy stand-in of tests/test_clip_ref.py gives the same figures to two
  digits (xin0 0.987, x0 0.984, y 0.992, dqkv 0.991).
  Share of a block's non-zero incoming dx entries that round to zero as fp16 GEMM operands (|v| <= 2^-25, cotangent randn x 1e-3 scaled to max-abs
  in [8, 16)): 0 in every block of every case except block 10 of the peaked cases, 0.012 .. 0.105 (behind the peaked block 11) - covered by
  store16's absolute term, b_act stays at 0.98.
  Loss scale: max-abs 0 -> 1; 2^-100 -> 2^104; 1e-6 -> 2^23; 1 -> 16; 1e4 -> 2^-10; 6e4 -> 2^-12; 2^-125 and 1.4e-45 (16 / m overflows) -> 2^126 with the
  clamp of k_gscale (before it: inf, and NaN in g16); inf -> 1.  g_img(2^k c) == 2^k g_img(c) bit for bit for k = +-10.
  NaN- and zero-prefilled workspaces give the same bits in every buffer above; keep_for_bwd = 0 gives the kept forward's features bit for bit.
  Not reached by any case: quick_gelu_grad of an infinite pre-activation (0 x inf) needs |pre| > 65504, where the forward's fp16 store has overflowed
  already; the outliers case keeps |pre| and |qkv| below 6 with a residual stream up to 20.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import clip_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
SENT = F(-7.25)
D, L, NP, PK, DM, DOUT, NL = R.D, R.L, R.NP, R.PK, R.DM, R.DOUT, R.NL
NIMG = 3 * R.IMG * R.IMG


def _lib():
    from nerfart_amd import hip
    return hip


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


_packed, _stored = {}, {}


def _blob(case):
    """The weight case packed by nerfart_clip_vitb32_pack, once per module -> (device blob, bytes)."""
    if case not in _packed:
        from nerfart_amd import clip_native
        sd = {"visual." + k: torch.from_numpy(v) for k, v in R.make_state(case).items()}
        blob = clip_native.pack_visual(sd, torch.device("cuda"))
        torch.cuda.synchronize()
        _packed[case] = (blob, blob.numel())
    return _packed[case]


def _W(case):
    if case not in _stored:
        _stored[case] = R.stored(R.make_state(case))
    return _stored[case]


def _layout(B, keep):
    offs = (C.c_longlong * 21)()
    total = int(_lib().lib.nerfart_clip_vitb32_workspace_layout(B, keep, C.cast(offs, C.c_void_p)))
    return total, dict(zip(R.WS_NAMES, [int(o) for o in offs]))


def _up64(n):
    return (n + 63) // 64 * 64


class Run:
    """One forward (keep_for_bwd = 1) on a prefilled workspace and the partial backwards on it; reads only what a check needs."""

    def __init__(self, case, img, fill=-1):
        self.hip = _lib()
        self.lib = self.hip.lib
        self.B = B = img.shape[0]
        self.M, self.P = B * L, B * NP
        self.blob, self.nblob = _blob(case)
        self.img = _dev(img)
        self.total, self.off = _layout(B, 1)
        assert self.total == int(self.lib.nerfart_clip_vitb32_workspace_bytes(B, 1))
        self.ws = torch.full((self.total // 4,), fill, dtype=torch.int32, device="cuda").view(torch.uint8)
        self.feat = torch.full((B * DOUT + 64,), float(SENT), dtype=torch.float32, device="cuda")
        self.hip._check(self.lib.nerfart_clip_vitb32_image_fwd(self.blob.data_ptr(), self.nblob, self.img.data_ptr(), B, self.feat.data_ptr(), 1, self.ws.data_ptr(),
                                                               self.total, _stream()), "clip_vitb32_image_fwd")
        torch.cuda.synchronize()

    def buf(self, name, rows, cols, dtype, layer=None, first_row=0):
        o = self.off[name] + (0 if layer is None else self.off["saved"] + layer * self.off["layer_bytes"])
        item = np.dtype(dtype).itemsize
        o += first_row * cols * item
        return self.ws[o:o + rows * cols * item].cpu().numpy().view(dtype).reshape(rows, cols).copy()

    def forward_buffers(self):
        B, M, P = self.B, self.M, self.P
        f = self.feat.cpu().numpy()
        assert (f[B * DOUT:] == SENT).all(), "the forward wrote past feat"
        o = dict(feat=f[:B * DOUT].reshape(B, DOUT).copy(), patches=self.buf("patches", P, PK, np.float16), pe=self.buf("pe", P, D, F),
                 xemb=self.buf("xemb", M, D, F), xfin=self.buf("xfin", M, D, F), x0=self.buf("x0", B, D, np.float16),
                 att_last=self.buf("att", M, D, np.float16), act_last=self.buf("act", M, DM, np.float16))
        o["xin"] = [self.buf("xin", M, D, F, l) for l in range(NL)]
        o["xmid"] = [self.buf("xmid", M, D, F, l) for l in range(NL)]
        o["qkv"] = [self.buf("qkv", M, 3 * D, np.float16, l) for l in range(NL)]
        o["pre"] = [self.buf("pre", M, DM, np.float16, l) for l in range(NL)]
        # the padding rows of the zeroed region are GEMM operands: they must be exact zeros, not the prefill
        pads = [("patches", P, PK, np.float16, _up64(P)), ("x0", B, D, np.float16, _up64(B)), ("att", M, D, np.float16, _up64(M)), ("act", M, DM, np.float16, _up64(M))]
        o["pad_nonzero"] = [n for n, r0, c, dt, rp in pads if rp > r0 and self.buf(n, rp - r0, c, dt, first_row=r0).view(np.uint16).any()]
        return o

    def bwd(self, g_feat, stop, g_img=None, full=False):
        a = (self.blob.data_ptr(), self.nblob, self.B, g_feat.data_ptr(), None if g_img is None else g_img.data_ptr(), self.ws.data_ptr(), self.total)
        if full:
            self.hip._check(self.lib.nerfart_clip_vitb32_image_bwd(*a, _stream()), "clip_vitb32_image_bwd")
        else:
            self.hip._check(self.lib.nerfart_clip_vitb32_image_bwd_partial(*a, stop, _stream()), "clip_vitb32_image_bwd_partial")
        torch.cuda.synchronize()

    def backward_buffers(self, g_feat, o):
        B, M, P = self.B, self.M, self.P
        g = _dev(np.asarray(g_feat, F))
        g_img = torch.full((B * NIMG + 64,), float(SENT), dtype=torch.float32, device="cuda")
        self.bwd(g, NL, g_img)
        assert (g_img == float(SENT)).all(), "a partial backward with stop_layer > 0 touched g_img"
        o.update(scale=self.buf("scale", 1, 2, F)[0], g16=self.buf("g16", B, DOUT, np.float16), t0=self.buf("t0", B, D, F))
        for k in ("dx_in", "act", "att", "dqkv", "t"):
            o[k] = [None] * NL
        o["dx_in"][NL - 1] = self.buf("dx", M, D, F)
        for l in range(NL - 1, -1, -1):
            self.bwd(g, l, g_img if l == 0 else None)
            o["act"][l], o["att"][l] = self.buf("act", M, DM, np.float16), self.buf("att", M, D, np.float16)
            o["dqkv"][l], o["t"][l] = self.buf("dqkv", M, 3 * D, np.float16), self.buf("t", M, D, F)
            dx = self.buf("dx", M, D, F)
            if l:
                o["dx_in"][l - 1] = dx
            else:
                o["dx0"] = dx
        gi = g_img.cpu().numpy()
        assert (gi[B * NIMG:] == SENT).all(), "the backward wrote past g_img"
        o["g_img"] = gi[:B * NIMG].reshape(B, 3, R.IMG, R.IMG).copy()
        o["y"], o["dpatch"] = self.buf("y", P, D, np.float16), self.buf("pe", P, PK, F)
        o["y_pad_nonzero"] = bool(_up64(P) > P and self.buf("y", _up64(P) - P, D, np.float16, first_row=P).view(np.uint16).any())
        # nerfart_clip_vitb32_image_bwd is the partial run to 0, bit for bit
        g2 = torch.full((B * NIMG + 64,), float(SENT), dtype=torch.float32, device="cuda")
        self.bwd(g, 0, g2, full=True)
        o["g_img_full_same"] = bool(torch.equal(g2, g_img))
        return o


def _cot_kind(kind, B):
    return "image1" if (kind == "constpatch" and B == 3) else "randn"


@pytest.mark.parametrize("B", R.BATCHES)
@pytest.mark.parametrize("kind", R.IMAGE_KINDS)
@pytest.mark.parametrize("case", R.WEIGHT_CASES)
def test_clip_stages_against_fp64(case, kind, B):
    W = _W(case)
    img, g = R.make_image(kind, B), R.make_cotangent(_cot_kind(kind, B), B)
    run = Run(case, img)
    o = run.backward_buffers(g, run.forward_buffers())
    rep = R.Report(f"{case} {kind} B={B}")
    R.check_forward(W, img, o, rep=rep)
    R.check_backward(W, g, o, rep=rep)
    rep.check(not o["pad_nonzero"], f"padding rows of {o['pad_nonzero']} are not zero after the forward")
    rep.check(not o["y_pad_nonzero"], "padding rows of y are not zero after the backward")
    rep.check(o["g_img_full_same"], "nerfart_clip_vitb32_image_bwd differs from the partial run to 0")
    print(rep.line())
    print("  share of each block's non-zero incoming dx entries that round to zero in fp16 (blocks 0 .. 11): " + " ".join(f"{s:.3f}" for s in R.zero_share(o)))
    assert not rep.fail, rep.line()


def test_workspace_contents_do_not_matter():
    """The forward zeroes the workspace only below the saved blocks; their padding rows keep the caller's bytes.  NaN there and zero there must give
    the same bits everywhere a result or a checked buffer lives; and the keep_for_bwd = 0 forward gives the kept forward's features."""
    case, B = "peaked", 3
    img, g = R.make_image("randn", B), R.make_cotangent("randn", B)
    outs = []
    for fill in (-1, 0):
        run = Run(case, img, fill)
        outs.append(run.backward_buffers(g, run.forward_buffers()))
    a, b = outs
    diff = []
    for k in a:
        va, vb = a[k], b[k]
        if isinstance(va, list) and va and isinstance(va[0], np.ndarray):
            diff += [f"{k}[{l}]" for l in range(len(va)) if va[l].tobytes() != vb[l].tobytes()]
        elif isinstance(va, np.ndarray):
            diff += [k] if va.tobytes() != vb.tobytes() else []
    assert not diff, f"buffers that depend on the workspace's earlier contents: {diff}"
    assert np.isfinite(a["feat"]).all() and np.isfinite(a["g_img"]).all()
    hip = _lib()
    n0, _ = _layout(B, 0)
    ws0 = torch.full((n0 // 4,), -1, dtype=torch.int32, device="cuda")
    feat = torch.full((B * DOUT + 64,), float(SENT), dtype=torch.float32, device="cuda")
    blob, nblob = _blob(case)
    hip._check(hip.lib.nerfart_clip_vitb32_image_fwd(blob.data_ptr(), nblob, _dev(img).data_ptr(), B, feat.data_ptr(), 0, ws0.data_ptr(), n0, _stream()), "fwd keep 0")
    torch.cuda.synchronize()
    f0 = feat.cpu().numpy()
    assert (f0[B * DOUT:] == SENT).all() and f0[:B * DOUT].tobytes() == a["feat"].tobytes()


def test_loss_scale():
    """scale[0] is the documented power of two and scale[1] its exact reciprocal over 330 binades of max-abs; g_img is exactly linear in a power-of-two
    factor; a max-abs below 2^-124 (16 / m overflows: every subnormal m) is clamped to 2^126 instead of giving inf / NaN; a non-finite max-abs gives 1."""
    B = 1
    img = R.make_image("randn", B)
    run = Run("seeded", img)
    rng = np.random.default_rng(11)
    c = rng.standard_normal((B, DOUT))
    c = (c / np.abs(c).max()).astype(F)                     # max-abs exactly 1
    for m in (0.0, 2.0 ** -100, 1e-6, 1.0, 1e4, 6e4, 2.0 ** -125, 1e-45, float("inf")):
        # + 0: no - 0 in the input (a product that is - 0 keeps its sign on one code path of k_gscale and loses it in the fma of the other; no result
        # depends on the sign of a zero operand)
        g = (c * F(m) + F(0)).astype(F) if np.isfinite(m) else np.where(np.abs(c) == 1, F(np.inf), c).astype(F)
        run.bwd(_dev(g), NL)
        s, inv = R.loss_scale(g)
        got = run.buf("scale", 1, 2, F)[0]
        print(f"  max-abs {float(np.abs(g).max()):.3g}: scale {got[0]:.6g}, 1 / scale {got[1]:.6g}")
        assert R.same_bits(got, np.array([s, inv], F)), (m, got, s)
        if np.isfinite(m):
            g16 = run.buf("g16", B, DOUT, np.float16)
            assert np.isfinite(g16).all() and R.same_bits(g16.astype(F), R.r16(g * F(s)).astype(F)), m
    # the fix: a subnormal max-abs runs the whole backward to finite numbers
    gi = torch.full((B * NIMG,), float(SENT), dtype=torch.float32, device="cuda")
    run.bwd(_dev((c * F(1e-45) + F(0)).astype(F)), 0, gi)
    assert torch.isfinite(gi).all()
    # exact linearity in 2^k
    base = (c * F(1e-3)).astype(F)
    outs = {}
    for k in (0, 10, -10):
        run.bwd(_dev(base * F(2.0 ** k)), 0, gi)
        outs[k] = gi.cpu().numpy().copy()
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    small = np.abs(outs[0])[outs[0] != 0].min()
    assert small * 2.0 ** -10 > 2.0 ** -126, "an entry would underflow: the comparison below would not be exact"
    for k in (10, -10):
        assert R.same_bits(outs[k], outs[0] * F(2.0 ** k)), k


def test_workspace_layout():
    lib = _lib().lib
    null = C.c_void_p(0)
    for B in (1, 3, 16):
        Mp, Pp, Bp = _up64(B * L), _up64(B * NP), _up64(B)
        for keep in (0, 1):
            total, off = _layout(B, keep)
            assert total == lib.nerfart_clip_vitb32_workspace_bytes(B, keep) == off["total"] == lib.nerfart_clip_vitb32_workspace_layout(B, keep, null) > 0
            o = [off[k] for k in R.WS_NAMES[:15]]
            assert o == sorted(o) and len(set(o)) == 15 and all(off[k] % 256 == 0 for k in R.WS_NAMES)
            assert off["patches"] - off["scale"] == 256 and off["pe"] - off["patches"] == 2 * Pp * PK and off["xemb"] - off["pe"] == 4 * Pp * PK
            assert off["act"] - off["att"] == 2 * Mp * D and off["t"] - off["act"] == 2 * Mp * DM and off["dqkv"] - off["dx"] == 4 * Mp * D
            assert off["g16"] - off["x0"] == 2 * Bp * D and off["t0"] - off["g16"] == 2 * Bp * DOUT and off["saved"] - off["t0"] == 4 * Bp * D
            assert (off["xin"], off["xmid"], off["qkv"], off["pre"]) == (0, 4 * Mp * D, 8 * Mp * D, 8 * Mp * D + 2 * Mp * 3 * D)
            assert off["layer_bytes"] == off["pre"] + 2 * Mp * DM
            # keep: 12 blocks; no keep: one block and the residual stream's ping-pong buffer
            assert total - off["saved"] == (NL * off["layer_bytes"] if keep else off["layer_bytes"] + 4 * Mp * D)
    assert lib.nerfart_clip_vitb32_workspace_layout(0, 1, null) == 0 == lib.nerfart_clip_vitb32_workspace_bytes(0, 1)
