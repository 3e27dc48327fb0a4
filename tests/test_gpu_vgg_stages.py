"""The VGG16 perceptual kernels (csrc/vgg_conv.hip, csrc/gemm_f32.h) stage by stage, and nerfart_geometry_feature (the same k_gemm with an arbitrary
M), against the fp64 references and the error model of tests/vgg_ref.py, through hip.lib and ctypes.  The workspace is filled with 0xffffffff (NaN)
before every forward and read back through nerfart_vgg16_workspace_layout: every buffer is compared with the fp64 evaluation of its stage on the
kernel's own stored input.  One line per case: the worst observed / bound ratio per buffer (1.00 = the bound; 0.000 on an exact buffer = bit for bit).

Worst observed / bound ratio per buffer over the nine shapes x five image cases on an MI355X (gfx950; every case passed; cols, p0, p1, ga and the zero
columns of dcols bit for bit; equal images gave loss == 0 and g_img == 0 exactly):
  forward             y0 0.155  y1 0.010  y2 0.010  y3 0.006  y4 0.004  y5 0.002  y6 0.003   (the worst-case (K + 2) u S against errors that grow like sqrt K)
  loss                keep_for_bwd = 1: 0.043   keep_for_bwd = 0: 0.066
  backward, by stage  ga_end (conv1_2^T of the stored gb) 0.010   dcols (stored ga . W0) 0.082   g_img (gather of the stored dcols) 0.320, with the
                      device scalar 3.0: 0.361
  backward, chained   dcols, g_img, gb_end, ga_end against the six-layer recursion: below 0.0005 - that bound is orders of magnitude above the values
                      (vgg_ref's docstring); what it pins are the exact zeros of the masks and of the un-pool routing
  geometry feature    M = 1: 0.007   63, 64, 65: 0.012   200: 0.017; no guard row touched, h7 of exactly M rows
"""
import ctypes as C

import numpy as np
import pytest
import torch

import vgg_ref as VR

pytestmark = pytest.mark.gpu

F = np.float32
SENT = F(-7.25)
UP = 3.0
GEO_M = [1, 63, 64, 65, 200]


def _lib():
    from nerfart_amd import hip
    return hip


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


_packed = {}


def _blob():
    """The seeded weights of vgg_ref.make_weights packed by nerfart_vgg16_pack -> (device blob, bytes)."""
    if "blob" not in _packed:
        hip = _lib()
        Ws, bs = VR.make_weights()
        total = int(hip.lib.nerfart_vgg16_blob_layout(None))
        blob = torch.zeros(total, dtype=torch.uint8, device="cuda")
        wd, bd = [_dev(w) for w in Ws], [_dev(b) for b in bs]
        wt = (C.c_void_p * 7)(*[t.data_ptr() for t in wd])
        bt = (C.c_void_p * 7)(*[t.data_ptr() for t in bd])
        hip._check(hip.lib.nerfart_vgg16_pack(wt, bt, blob.data_ptr(), total, _stream()), "nerfart_vgg16_pack")
        torch.cuda.synchronize()
        _packed["blob"] = (blob, total)
    return _packed["blob"]


def _layout(H, W, keep):
    offs = (C.c_longlong * 15)()
    total = int(_lib().lib.nerfart_vgg16_workspace_layout(H, W, keep, C.cast(offs, C.c_void_p)))
    return total, dict(zip(VR.WS_NAMES, [int(o) for o in offs]))


def run_case(case):
    hip = _lib()
    lib = hip.lib
    H, W = case["H"], case["W"]
    blob, nblob = _blob()
    img2 = _dev(case["img2"])
    out = {}
    # keep_for_bwd = 0: its own, smaller workspace
    n0 = int(lib.nerfart_vgg16_workspace_bytes(H, W, 0))
    total0, _ = _layout(H, W, 0)
    total1, off = _layout(H, W, 1)
    n1 = int(lib.nerfart_vgg16_workspace_bytes(H, W, 1))
    assert total0 == n0 and total1 == n1 and off["total"] == n1 and 0 < n0 < n1
    loss = torch.full((2,), float(SENT), dtype=torch.float32, device="cuda")
    ws0 = torch.full((n0 // 4,), -1, dtype=torch.int32, device="cuda")
    hip._check(lib.nerfart_vgg16_l1_fwd(blob.data_ptr(), nblob, img2.data_ptr(), H, W, loss.data_ptr(), 0, ws0.data_ptr(), n0, _stream()), "vgg16_l1_fwd keep 0")
    torch.cuda.synchronize()
    out["loss_nokeep"] = loss.cpu().numpy()[0]
    # the backward refuses the keep = 0 byte count on the host, before any launch
    g_img = torch.full((3 * H * W + 64,), float(SENT), dtype=torch.float32, device="cuda")
    rc = lib.nerfart_vgg16_l1_bwd(blob.data_ptr(), nblob, H, W, None, g_img.data_ptr(), ws0.data_ptr(), n0, _stream())
    assert rc != 0 and b"workspace too small" in lib.nerfart_last_error()
    # keep_for_bwd = 1
    ws = torch.full((n1 // 4,), -1, dtype=torch.int32, device="cuda")
    hip._check(lib.nerfart_vgg16_l1_fwd(blob.data_ptr(), nblob, img2.data_ptr(), H, W, loss.data_ptr(), 1, ws.data_ptr(), n1, _stream()), "vgg16_l1_fwd keep 1")
    torch.cuda.synchronize()
    host = ws.cpu().numpy().view(F)

    def buf(name, shape):
        o = off[name] // 4
        return host[o:o + int(np.prod(shape))].reshape(shape).copy()
    l = loss.cpu().numpy()
    assert l[1] == SENT
    out["loss"] = l[0]
    out["cols"] = buf("cols", (2 * H * W, 32))
    for i in range(7):
        s = 1 << VR.LEVEL[i]
        out[f"y{i}"] = buf(f"y{i}", (2, H // s, W // s, VR.COUT[i]))
    out["p0"] = buf("p0", (2, H // 2, W // 2, 64))
    out["p1"] = buf("p1", (2, H // 4, W // 4, 128))
    out["ga"] = buf("ga", (H // 4, W // 4, 256))
    assert float(buf("loss", (1,))[0]) == float(l[0])
    # backward: upstream NULL, then a device scalar
    for key, up in (("", None), ("_up", _dev(np.array([UP], F)))):
        hip._check(lib.nerfart_vgg16_l1_bwd(blob.data_ptr(), nblob, H, W, None if up is None else up.data_ptr(), g_img.data_ptr(), ws.data_ptr(), n1, _stream()),
                   "vgg16_l1_bwd")
        torch.cuda.synchronize()
        g = g_img.cpu().numpy()
        assert (g[3 * H * W:] == SENT).all(), "the backward wrote past g_img"
        out["g_img" + key] = g[:3 * H * W].reshape(3, H, W).copy()
        host = ws.cpu().numpy().view(F)
        out["dcols" + key] = buf("dcols", (H * W, 64))
        if up is None:
            out["ga_end"], out["gb_end"] = buf("ga", (H * W, 64)), buf("gb", (H, W, 64))
            # the second backward starts from sign * mask again: the ga buffer is the cotangent ping-pong, so re-run the forward
            hip._check(lib.nerfart_vgg16_l1_fwd(blob.data_ptr(), nblob, img2.data_ptr(), H, W, loss.data_ptr(), 1, ws.data_ptr(), n1, _stream()), "vgg16_l1_fwd")
    out["upstream"] = UP
    # the re-run forward wrote the same activations (the checks below read the first run's copies)
    host = ws.cpu().numpy().view(F)
    assert VR.same_bits(buf("y6", out["y6"].shape), out["y6"]) and VR.same_bits(img2.cpu().numpy(), case["img2"])
    return out


@pytest.mark.parametrize("shape", VR.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_vgg_stages_against_fp64(shape):
    Ws, bs = VR.make_weights()
    reps, worst = [], {}
    for case in VR.matrix(shape):
        rep = VR.check(case, Ws, bs, run_case(case))
        print(rep.line())
        for k, v in rep.ratio.items():
            worst[k] = max(worst.get(k, 0.0), v)
        reps.append(rep)
    print(f"  WORST {shape[0]}x{shape[1]}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = [r.line() for r in reps if r.fail]
    assert not bad, bad


def test_workspace_layout_matches_workspace_bytes():
    lib = _lib().lib
    for H, W in VR.SHAPES + [(224, 224)]:
        for keep in (0, 1):
            total, off = _layout(H, W, keep)
            assert total == lib.nerfart_vgg16_workspace_bytes(H, W, keep) == off["total"] > 0
            o = [off[k] for k in VR.WS_NAMES]
            assert o == sorted(o) and all(v % 256 == 0 for v in o) and off["cols"] - off["loss"] == 256
            assert off["y0"] - off["cols"] == 4 * 2 * H * W * 32
            assert (off["gb"] - off["ga"] == 4 * H * W * 64) if keep else (off["ga"] == off["gb"] == off["dcols"] == total)
    assert lib.nerfart_vgg16_workspace_layout(4, 64, 1, None) == 0 == lib.nerfart_vgg16_workspace_bytes(4, 64, 1)


@pytest.mark.parametrize("M", GEO_M)
def test_geometry_feature_rows_and_guard(M):
    """h7 has exactly M rows (the padding rows of the last 64-row tile re-read row M - 1), the output 64 guard rows of a sentinel."""
    hip = _lib()
    lib = hip.lib
    rng = np.random.default_rng(40 + M)
    g, v, bias = rng.uniform(0.5, 1.5, 257).astype(F), rng.standard_normal((257, 256)).astype(F), rng.uniform(-0.5, 0.5, 257).astype(F)
    h7 = rng.standard_normal((M, 256)).astype(F)
    gd, vd, bd, hd = _dev(g), _dev(v), _dev(bias), _dev(h7)
    out = torch.full((M + 64, 256), float(SENT), dtype=torch.float32, device="cuda")
    nws = int(lib.nerfart_geometry_feature_workspace_bytes())
    ws = torch.full((nws // 4,), -1, dtype=torch.int32, device="cuda")
    hip._check(lib.nerfart_geometry_feature(gd.data_ptr(), vd.data_ptr(), bd.data_ptr(), hd.data_ptr(), M, out.data_ptr(), ws.data_ptr(), nws, _stream()),
               "nerfart_geometry_feature")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    rep = VR.Report(f"geometry M={M}")
    val, bound = VR.geometry_feature(g, v, bias, h7)
    rep.within("feat", o[:M], val, bound)
    rep.check(VR.same_bits(o[M:], np.full((64, 256), SENT, F)), "a guard row past M was written")
    rep.check(VR.same_bits(hd.cpu().numpy(), h7), "h7 changed")
    print(rep.line())
    assert not rep.fail, rep.line()
