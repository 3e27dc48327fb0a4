"""The weight-gradient tail of pass 2 on the GPU - nerfart_sdf_param_bwd, nerfart_radiance_param_bwd, nerfart_fold_weight_grads,
nerfart_weight_norm_bwd and the two nerfart_*_render_bwd calls - against the references, models and allowances of tests/param_grad_ref.py, on the
sizes tests/test_param_grad_ref.py runs a model of the route and its mutants through on the CPU.  Called through hip.lib and ctypes on buffers of
the test's own: pre-filled with 0xFF bytes (NaN as bf16 and as fp32; raw buffers zeroed where the comparison starts from zero) and followed by a
guard tail that must come back untouched; workspaces sized by the *_workspace_bytes calls and filled the same way.  Every entry-point call runs
twice on the same inputs and must give the same bits.

1. raw against fp64 products of the library's own operands (the public stage entry points on the same inputs), per element n 2^-23 S.
   Decisions on the slots nothing downstream reads (from csrc/render_backward.hip): row 1 of SURF_CS0 is written - the column sums of zbar_4, held
   to the bound like row 0; features 217..255 of layer 3 are reduced like every other row / column, from whatever finite values the dumps hold;
   the columns of the 64-wide sections that no operand column fills get only zero added (old + 0: checked from a zeroed start, and from a
   sentinel in the train_radiance test); SURF_B8[1..3], RAD_B4[3] and every section of the other net are never written: exactly what the call
   started from.
2. the fold against the numpy model, every element of every piece, at most one fp32 ulp.
3. the weight_norm chain rule against fp64.
4. .grad of every parameter against fp64 autograd.
5. the ray-level calls against the chain of their public stages, bit for bit; RAD_WH7 (the entry points take a7 from the second-order forward
   dump, the public radiance route rounds the fp32 h7) is held to the bound of 1 against the product of the radiance backward dump with that
   forward dump - obtained by calling nerfart_sdf_fwd2 on the same inputs - which is tighter than the end-to-end allowance; the eikonal scalar to
   R 2^-23 sum |eik_ray|.  One more section differs by construction: the scalars d loss / d alpha, d beta, d s are summed over the rays with
   atomicAdd (k_composite_volsdf_bwd / k_composite_neus_bwd, one value per ray), so two runs of the SAME call differed in the last bit of
   d loss / d beta; they are held to R 2^-23 sum |per-ray value| against the fp64 sum of the values of one-ray launches.

OBSERVED on an MI355X (gfx950), worst observed / allowed over all sizes; every case passed and every exact check - guard tails, the 0xFF / NaN
fills, two runs, NULL cotangents, the doubling second call, train_radiance = 0, the rgb / g_h7 / g_n copies, the 11 sections of part 5 - held bit
for bit.  No bug was found in the library.
  1. SURF_WW 0.020  SURF_WE 0.010  SURF_CS0 0.007  SURF_CS17 0.026  SURF_W8 0.007  SURF_B8 0.002
     RAD_WW 0.009  RAD_CS 0.002  RAD_W4 0.007  RAD_B4 0.001  RAD_WEX 0.008  RAD_WH7 0.016;  two calls over halves: 0.004 and below
     (the bound counts one rounding per row; errors of random sign grow like its square root)
  2. bit-exact (0 ulp) on every element of the 28 pieces, (multires, multires_view) = (6, -1) and (6, 4)
  3. g_weight_g 0.60 (2 x 65)  g_weight_v 0.45 (2 x 63);  the row with dW parallel to v: 0.45 at worst (2 x 63), 0.02 at (1, 1)
  4. nerfart_sdf_param_bwd:       weight_g 0.31  weight_v 0.27  bias 0.34
     nerfart_radiance_param_bwd:  radiance weight_g 0.33  weight_v 0.32  bias 0.26;  SDF layer 8: weight_g 0.28  weight_v 0.27  bias 0.28
     (0.25 = the stand-in's own error: FACTOR = 4)
  5. RAD_WH7 0.028  alpha / beta / s scalars 0.07  eikonal scalar 0.09
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_bwd_ref as R
import param_grad_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
F32 = torch.float32


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(fw):
    from nerfart_amd import scene
    model, _, _ = scene.build_model(fw, seed=0, beta=0.01 if fw == "VolSDF" else None, device=DEV, precision="bf16x3")
    surf_blob, rad_blob = model.packed()
    sd = {k: v.detach().float().contiguous() for k, v in model.state_dict().items()}
    sd_cpu = {k: v.cpu() for k, v in sd.items()}
    nets = R.Nets(sd_cpu)
    assert nets.view_tiles == model.view_tiles
    return dict(model=model, surf=surf_blob, rad=rad_blob, vt=model.view_tiles, mv=nets.multires_view, nets=nets, sd=sd, sd_cpu=sd_cpu)


def _lib():
    from nerfart_amd import hip
    return hip.lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rc(rc, who):
    assert rc == 0, (who, rc, _lib().nerfart_last_error().decode())


class Buf:
    """nbytes of the test's own + a guard tail, all 0xFF."""

    def __init__(self, nbytes, zero=False):
        self.n = int(nbytes)
        self.t = torch.full((self.n + GUARD,), R.FILL, dtype=torch.uint8, device=DEV)
        if zero:
            self.t[: self.n] = 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def bytes(self):
        return self.t[: self.n]

    def f32(self, *shape):
        return self.t[: self.n].view(F32).view(*shape)

    def guard_ok(self):
        return bool((self.t[self.n:] == R.FILL).all())


def _p(t):
    return None if t is None else t.data_ptr()


def _raw_total():
    offs = (C.c_longlong * 14)()
    total = int(_lib().nerfart_pass2_raw_layout(offs))
    want, wtotal = G.raw_offsets()
    assert total == wtotal and [int(o) for o in offs] == [want[s] for s in G.SECTIONS] + [wtotal]
    return total


def _new_raw(sentinel=None):
    b = Buf(_raw_total() * 4, zero=sentinel is None)
    if sentinel is not None:
        b.f32(-1).fill_(sentinel)
    return b


def _dev_inputs(c, keys):
    return {k: c[k].to(DEV).float().contiguous() for k in keys}


def _sdf_entry(sc, inp, M, raw, sbar=True, hbar7=True):
    """nerfart_sdf_param_bwd into raw (a Buf).  sbar / hbar7: True = the case's, None = NULL, or a tensor."""
    lib = _lib()
    nb = int(lib.nerfart_sdf_param_bwd_workspace_bytes(M))
    ws = Buf(nb)
    s = inp["gbar_sdf"] if sbar is True else sbar
    h = inp["gbar_h7"] if hbar7 is True else hbar7
    _rc(lib.nerfart_sdf_param_bwd(sc["surf"].data_ptr(), 6, inp["pts"].data_ptr(), M, _p(s), _p(h), inp["dir"].data_ptr(), raw.ptr, ws.ptr, nb, _st()),
        "sdf_param_bwd")
    torch.cuda.synchronize()
    assert ws.guard_ok() and raw.guard_ok(), "sdf_param_bwd wrote past the end of its workspace or of raw"


def _sdf_stages(sc, inp, M, sbar=None, hbar7=None):
    """The bytes nerfart_sdf_param_bwd reduces, from the public stage entry points on the same inputs -> decoded operands."""
    lib, Mp = _lib(), R.up(M, 64)
    s = inp["gbar_sdf"] if sbar is None else sbar
    h = inp["gbar_h7"] if hbar7 is None else hbar7
    b = dict(f2=Buf(lib.nerfart_sdf_fwd2_dump_bytes(M)), r2=Buf(lib.nerfart_sdf_bwd2_dump_bytes(M)), E2=Buf(2 * Mp * 128), SO=Buf(2 * Mp * 128))
    _rc(lib.nerfart_sdf_fwd2(sc["surf"].data_ptr(), inp["pts"].data_ptr(), inp["dir"].data_ptr(), M, b["f2"].ptr, _st()), "sdf_fwd2")
    _rc(lib.nerfart_sdf_bwd2(sc["surf"].data_ptr(), M, h.data_ptr(), s.data_ptr(), b["f2"].ptr, b["r2"].ptr, _st()), "sdf_bwd2")
    _rc(lib.nerfart_wgrad_operand_embed_pair(inp["pts"].data_ptr(), inp["dir"].data_ptr(), M, Mp, 6, b["E2"].ptr, _st()), "operand_embed_pair")
    _rc(lib.nerfart_wgrad_operand_sbar_ones(s.data_ptr(), M, Mp, b["SO"].ptr, _st()), "operand_sbar_ones")
    torch.cuda.synchronize()
    assert all(v.guard_ok() for v in b.values())
    return G.sdf_operands(M, b["f2"].bytes().cpu(), b["r2"].bytes().cpu(), b["E2"].bytes().cpu(), b["SO"].bytes().cpu(), s), b


def _rad_entry(sc, inp, M, raw, train=1, outs=True):
    lib = _lib()
    nb = int(lib.nerfart_radiance_param_bwd_workspace_bytes(M))
    ws = Buf(nb)
    o = dict(rgb=Buf(M * 12), g_h7=Buf(M * 1024), g_n=Buf(M * 12)) if outs else {}
    _rc(lib.nerfart_radiance_param_bwd(sc["rad"].data_ptr(), sc["vt"], inp["pts"].data_ptr(), inp["view"].data_ptr(), inp["nabla"].data_ptr(),
                                       inp["h7"].data_ptr(), M, inp["g_rgb"].data_ptr(), o["rgb"].ptr if outs else None, o["g_h7"].ptr if outs else None,
                                       o["g_n"].ptr if outs else None, train, raw.ptr, ws.ptr, nb, _st()), "radiance_param_bwd")
    torch.cuda.synchronize()
    assert ws.guard_ok() and raw.guard_ok() and all(v.guard_ok() for v in o.values()), "radiance_param_bwd wrote past the end of a buffer"
    return o


def _rad_stages(sc, inp, M):
    lib, Mp = _lib(), R.up(M, 128)
    nd = int(lib.nerfart_radiance_dump_bytes(M))
    b = dict(rgb=Buf(M * 12), fdump=Buf(nd), bdump=Buf(nd), g_h7=Buf(M * 1024), g_n=Buf(M * 12), D4=Buf(Mp * 128), d4=Buf(M * 12),
             sums=Buf((Mp + 31) // 32 * 12), EX=Buf(Mp * 128))
    _rc(lib.nerfart_radiance_fwd_dump(sc["rad"].data_ptr(), sc["vt"], inp["pts"].data_ptr(), inp["view"].data_ptr(), M, inp["nabla"].data_ptr(),
                                      inp["h7"].data_ptr(), b["rgb"].ptr, b["fdump"].ptr, _st()), "radiance_fwd_dump")
    _rc(lib.nerfart_radiance_bwd(sc["rad"].data_ptr(), M, b["rgb"].ptr, inp["g_rgb"].data_ptr(), b["fdump"].ptr, b["bdump"].ptr, b["g_h7"].ptr,
                                 b["g_n"].ptr, _st()), "radiance_bwd")
    _rc(lib.nerfart_wgrad_operand_rgb_delta(b["rgb"].ptr, inp["g_rgb"].data_ptr(), M, Mp, b["D4"].ptr, b["d4"].ptr, b["sums"].ptr, _st()), "operand_rgb_delta")
    _rc(lib.nerfart_wgrad_operand_inputs(inp["pts"].data_ptr(), -1, inp["view"].data_ptr(), sc["mv"], inp["nabla"].data_ptr(), M, Mp, b["EX"].ptr, _st()),
        "operand_inputs")
    torch.cuda.synchronize()
    assert all(v.guard_ok() for v in b.values())
    op = G.rad_operands(M, b["fdump"].bytes().cpu(), b["bdump"].bytes().cpu(), b["D4"].bytes().cpu(), b["EX"].bytes().cpu(),
                        G.a7_bytes(inp["h7"].cpu(), M), b["d4"].f32(M, 3).cpu())
    return op, b


SDF_KEYS, RAD_KEYS = ("pts", "dir", "gbar_sdf", "gbar_h7"), ("pts", "view", "nabla", "h7", "g_rgb")


@functools.lru_cache(maxsize=None)
def _route(spec):
    """One case through the entry point (twice) and through the stages -> everything parts 1 and 4 look at."""
    kind, fw, M = spec
    sc = _scene(fw)
    c = R.make_case(spec, sc["nets"])
    inp = _dev_inputs(c, SDF_KEYS if kind == "sdf" else RAD_KEYS)
    raws, outs = [], []
    for _ in range(2):
        raw = _new_raw()
        outs.append(_sdf_entry(sc, inp, M, raw) if kind == "sdf" else _rad_entry(sc, inp, M, raw))
        raws.append(raw.f32(-1).cpu())
    op, bufs = (_sdf_stages if kind == "sdf" else _rad_stages)(sc, inp, M)
    return dict(sc=sc, c=c, inp=inp, raws=raws, outs=outs, op=op, bufs=bufs, raw_dev=raw)


def _other_sections_untouched(raw, mine, start=0.0):
    return [s for s in G.SECTIONS if s not in mine and not bool((G.section(raw, s) == start).all())]


# ---- 1. the reductions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", G.specs(), ids=R.spec_id)
def test_raw_matches_fp64_products_of_the_library_operands(spec):
    kind, fw, M = spec
    r = _route(spec)
    a, b = r["raws"]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{R.spec_id(spec)}: raw differs between two runs on the same inputs"
    P, S = G.reduce_sections(r["op"]), G.reduce_sections(r["op"], absolute=True)
    n = G.additions(kind, M, G.lib_split(_lib()))
    rep = G.new_report(R.spec_id(spec))
    worst = G.check_raw(rep, a, P, S, n)
    print(f"\n{R.spec_id(spec)}: " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert not rep.viol, "\n".join(rep.viol[:20])
    assert not _other_sections_untouched(a, P), "sections of the other net / the scalars were written"
    if kind == "rad":                                      # the copies handed out are the stage calls' own bits
        for o in r["outs"]:
            for k, shp in (("rgb", (M, 3)), ("g_h7", (M, 256)), ("g_n", (M, 3))):
                assert torch.equal(o[k].f32(*shp).view(torch.int32), r["bufs"][k].f32(*shp).view(torch.int32)), k


def test_null_cotangents_are_zero_tensors():
    spec = ("sdf", "VolSDF", 65)
    sc = _scene("VolSDF")
    c = R.make_case(spec, sc["nets"])
    inp = _dev_inputs(c, SDF_KEYS)
    zs, zh = torch.zeros(65, device=DEV), torch.zeros(65, 256, device=DEV)
    for sbar, hbar7 in ((None, True), (True, None), (None, None)):
        null, zero = _new_raw(), _new_raw()
        _sdf_entry(sc, inp, 65, null, sbar=sbar, hbar7=hbar7)
        _sdf_entry(sc, inp, 65, zero, sbar=zs if sbar is None else True, hbar7=zh if hbar7 is None else True)
        assert torch.equal(null.f32(-1).view(torch.int32), zero.f32(-1).view(torch.int32)), (sbar, hbar7)
        assert bool((null.f32(-1) != 0).any())


def _half_inputs(inp, sl):
    return {k: v[sl].contiguous() for k, v in inp.items()}


@pytest.mark.parametrize("spec", [("sdf", "VolSDF", 200), ("rad", "NeuS", 300)], ids=R.spec_id)
def test_two_calls_over_disjoint_halves_accumulate(spec):
    """Two calls over disjoint halves of the points into one raw against the fp64 product over all points (the padding differs between the two
    routes: no bit equality); then a second identical call doubles every element exactly - accumulate adds once."""
    kind, fw, M = spec
    r = _route(spec)
    sc, inp, h = r["sc"], r["inp"], M // 2
    entry = _sdf_entry if kind == "sdf" else (lambda *a: _rad_entry(*a, outs=False))
    raw = _new_raw()
    entry(sc, _half_inputs(inp, slice(0, h)), h, raw)
    entry(sc, _half_inputs(inp, slice(h, M)), M - h, raw)
    split = G.lib_split(_lib())
    na, nb = G.additions(kind, h, split), G.additions(kind, M - h, split)
    n = {k: na[k] + nb[k] for k in na}
    rep = G.new_report(R.spec_id(spec) + " halves")
    worst = G.check_raw(rep, raw.f32(-1).cpu(), G.reduce_sections(r["op"]), G.reduce_sections(r["op"], absolute=True), n, extra=1)
    print(f"\n{R.spec_id(spec)} two halves: " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert not rep.viol, "\n".join(rep.viol[:20])
    twice = _new_raw()
    entry(sc, inp, M, twice)
    once = twice.f32(-1).clone()
    assert torch.equal(once.cpu().view(torch.int32), r["raws"][0].view(torch.int32))
    entry(sc, inp, M, twice)
    assert torch.equal(twice.f32(-1), once + once), "a second identical call did not add exactly once"


def test_train_radiance_0_leaves_the_radiance_sections_alone():
    spec = ("rad", "VolSDF", 129)
    r = _route(spec)
    sentinel = 1.25
    on, off = _new_raw(sentinel), _new_raw(sentinel)
    _rad_entry(r["sc"], r["inp"], 129, on, train=1, outs=False)
    _rad_entry(r["sc"], r["inp"], 129, off, train=0, outs=False)
    a, b = on.f32(-1).cpu(), off.f32(-1).cpu()
    assert torch.equal(G.section(a, "RAD_WH7").view(torch.int32), G.section(b, "RAD_WH7").view(torch.int32))
    assert torch.equal(G.section(a, "RAD_CS")[4].view(torch.int32), G.section(b, "RAD_CS")[4].view(torch.int32))
    assert bool((G.section(b, "RAD_WH7") != sentinel).any()) and bool((G.section(a, "RAD_WW") != sentinel).any())
    for s in G.SECTIONS:
        if s == "RAD_WH7":
            continue
        v = G.section(b, s)[:4] if s == "RAD_CS" else G.section(b, s)
        assert bool((v == sentinel).all()), f"train_radiance = 0 touched {s}"
    # train_radiance = 1 from the sentinel: the columns no operand column fills get old + 0, RAD_B4[3] is never written (nex = 9 on this scene)
    assert r["sc"]["nets"].nex == 9
    w4, wex = G.section(a, "RAD_W4"), G.section(a, "RAD_WEX")
    for v, who in ((w4[:, 3:32], "RAD_W4 3..31"), (w4[:, 35:], "RAD_W4 35..63"), (wex[:, 9:32], "RAD_WEX 9..31"), (wex[:, 41:], "RAD_WEX 41..63"),
                   (G.section(a, "RAD_B4")[3:], "RAD_B4[3]")):
        assert bool((v == sentinel).all()), f"{who} did not keep the sentinel"
    assert bool((w4[:, :3] != sentinel).any()) and bool((wex[:, :9] != sentinel).any())


def test_unfilled_columns_of_the_sdf_sections_keep_a_sentinel():
    """nerfart_sdf_param_bwd into a raw pre-set to a sentinel: the columns of SURF_WE / SURF_W8 that no operand column fills get old + 0, SURF_B8[1..3]
    and every section of the radiance net are never written - the sentinel comes back bit for bit."""
    spec = ("sdf", "VolSDF", 65)
    r = _route(spec)
    sentinel = 1.25
    raw = _new_raw(sentinel)
    _sdf_entry(r["sc"], r["inp"], 65, raw)
    a = raw.f32(-1).cpu()
    we, w8 = G.section(a, "SURF_WE"), G.section(a, "SURF_W8")
    for v, who in ((we[:, :, G.NENC:], "SURF_WE 39..63"), (w8[:, 1:32], "SURF_W8 1..31"), (w8[:, 33:], "SURF_W8 33..63"), (G.section(a, "SURF_B8")[1:], "SURF_B8[1..3]")):
        assert bool((v == sentinel).all()), f"{who} did not keep the sentinel"
    assert bool((we[:, :, :G.NENC] != sentinel).any()) and bool((w8[:, 0] != sentinel).any())
    assert not _other_sections_untouched(a, G.SDF_SECTIONS, start=sentinel)


# ---- 2. the fold -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", [-1, 4])
def test_fold_every_element(mv):
    """Every element of every folded piece against the numpy model, at most one fp32 ulp apart (it came out bit-exact on an MI355X); the folded
    buffer fully overwritten and nothing written behind it; NaN in the raw slots the fold must not read changes nothing."""
    lib = _lib()
    total = _raw_total()
    offs = (C.c_longlong * 29)()
    ftotal = int(lib.nerfart_folded_grads_layout(6, mv, offs))
    assert [int(o) for o in offs] == G.folded_offsets(6, mv) and ftotal == offs[28]
    raw_np = np.arange(total, dtype=np.float32) * np.float32(1e-3) + np.float32(1.0)
    want = G.fold_model(raw_np, 6, mv)
    results = []
    for poison in (False, True):
        src = raw_np.copy()
        if poison:
            src[G.fold_unread(6, mv)] = np.nan
        raw = torch.from_numpy(src).to(DEV)
        folded = Buf(ftotal * 4)
        _rc(lib.nerfart_fold_weight_grads(raw.data_ptr(), 6, mv, folded.ptr, _st()), "fold_weight_grads")
        torch.cuda.synchronize()
        assert folded.guard_ok(), "the fold wrote past offsets[28]"
        f = folded.f32(-1).cpu().numpy()
        assert np.isfinite(f).all(), f"{int((~np.isfinite(f)).sum())} elements not overwritten, or read from a slot the fold must not read"
        results.append(f)
    assert np.array_equal(results[0], results[1]), "the fold read a raw slot it must not read"
    got = {name: results[0][offs[i]: offs[i + 1]].reshape(shp) for i, (name, shp) in enumerate(G.folded_layout(6, mv))}
    rep = G.new_report(f"fold(6, {mv})")
    worst = G.check_fold(rep, got, want)
    print(f"\nfold (6, {mv}): worst distance {worst} ulp")
    assert not rep.viol, "\n".join(rep.viol[:20])


# ---- 3. the weight_norm chain rule ---------------------------------------------------------------------------------------------------------
WN_SHAPES = ((256, 39), (256, 256), (217, 256), (257, 256), (256, 265), (256, 289), (3, 256), (1, 1), (2, 63), (2, 64), (2, 65))


def _wn(dW, v, g, g_v=True, g_g=True, accumulate=0, old=None):
    """-> (g_v Buf or None, g_g Buf or None); outputs NaN-filled unless `old` = (old_v, old_g) presets them."""
    out_f, in_f = v.shape
    bv, bg = (Buf(out_f * in_f * 4) if g_v else None), (Buf(out_f * 4) if g_g else None)
    if old is not None:
        bv.f32(out_f, in_f).copy_(old[0])
        bg.f32(out_f).copy_(old[1])
    _rc(_lib().nerfart_weight_norm_bwd(dW.data_ptr(), v.data_ptr(), g.data_ptr(), out_f, in_f, bv.ptr if bv else None, bg.ptr if bg else None, accumulate,
                                       _st()), "weight_norm_bwd")
    torch.cuda.synchronize()
    assert all(b.guard_ok() for b in (bv, bg) if b is not None)
    return bv, bg


def _wn_allow(ref, yard, scale=0.0):
    """FACTOR x the largest error of the fp32 pairwise evaluation; where that is 0, 4 fp32 ulps of the reference.  g_v of (1, 1) is pure
    cancellation: the reference is exactly 0 and so is numpy's fp32 result, while an evaluation with a fused multiply-add keeps the residual of
    dW - v (dW . v) / |v|^2, a fraction of an ulp of dW - there the ulp is taken at `scale`, the uncancelled term g / |v| |dW|."""
    E = float((torch.as_tensor(np.asarray(yard, dtype=np.float64)).reshape(ref.shape) - ref).abs().max())
    return G.FACTOR * E if E > 0 else 4.0 * float(np.spacing(np.float32(max(float(ref.abs().max()), scale))))


@pytest.mark.parametrize("shape", WN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_weight_norm_bwd_matches_the_fp64_chain_rule(shape):
    out_f, in_f = shape
    gen = torch.Generator().manual_seed(100 * out_f + in_f)
    v = torch.randn(out_f, in_f, generator=gen)
    g = torch.rand(out_f, generator=gen) + 0.5
    dW = torch.randn(out_f, in_f, generator=gen)
    par = min(3, out_f - 1)
    dW[par] = 0.7 * v[par]                                   # one row with dW parallel to v: g_v is pure cancellation there
    r_g, r_v = G.wn_bwd64(dW, v, g)
    y_g, y_v = G.wn_bwd32_pairwise(dW.numpy(), v.numpy(), g.numpy())
    A_g, A_v = _wn_allow(r_g, y_g), _wn_allow(r_v, y_v, float(((g / v.norm(dim=1))[:, None] * dW.abs()).max()))
    d = [t.to(DEV).contiguous() for t in (dW, v, g)]
    bv, bg = _wn(*d)
    bv2, bg2 = _wn(*d)
    assert torch.equal(bv.t, bv2.t) and torch.equal(bg.t, bg2.t), "two runs differ"
    k_v, k_g = bv.f32(out_f, in_f).cpu(), bg.f32(out_f).cpu()
    assert bool(torch.isfinite(k_v).all()) and bool(torch.isfinite(k_g).all()), "accumulate = 0 left NaN of the fill behind"
    e_g, e_v = float((k_g.double() - r_g).abs().max()), float((k_v.double() - r_v).abs().max())
    e_par = float((k_v[par].double() - r_v[par]).abs().max())
    print(f"\nweight_norm_bwd {out_f} x {in_f}: g_g {e_g / A_g:.3f}  g_v {e_v / A_v:.3f}  the parallel row {e_par / A_v:.3f}")
    assert e_g <= A_g and e_v <= A_v, (e_g, A_g, e_v, A_v)
    # accumulate = 1 on a known output: old + new, one more rounding
    old_v, old_g = torch.randn(out_f, in_f, generator=gen), torch.randn(out_f, generator=gen)
    av, ag = _wn(*d, accumulate=1, old=(old_v.to(DEV), old_g.to(DEV)))
    for got, old, ref, A, who in ((av.f32(out_f, in_f).cpu(), old_v, r_v, A_v, "g_v"), (ag.f32(out_f).cpu(), old_g, r_g, A_g, "g_g")):
        want = old.double() + ref
        half_ulp = torch.as_tensor(np.spacing(want.abs().float().numpy()).astype(np.float64)) * 0.5
        assert bool(((got.double() - want).abs() <= A + half_ulp).all()), f"accumulate = 1: {who} is not old + new"
    # either output may be NULL: the other one has the same bits, nothing else is written
    only_g = _wn(*d, g_v=False)[1]
    only_v = _wn(*d, g_g=False)[0]
    assert torch.equal(only_g.t, bg.t) and torch.equal(only_v.t, bv.t)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------
def _lib_grads(raw_dev, sc, kind):
    """Entry point's raw -> nerfart_fold_weight_grads -> nerfart_weight_norm_bwd per layer -> {name: tensor}."""
    lib, mv = _lib(), sc["mv"]
    offs = G.folded_offsets(6, mv)
    folded = Buf(offs[-1] * 4)
    _rc(lib.nerfart_fold_weight_grads(raw_dev.ptr, 6, mv, folded.ptr, _st()), "fold_weight_grads")
    torch.cuda.synchronize()
    assert folded.guard_ok()
    f = folded.f32(-1)
    out = {}
    for name, stem, l in G.param_names(kind):
        i = 2 * (l if stem == G.S_STEM else 9 + l)
        v, g = sc["sd"][f"{stem}.{l}.weight_v"], sc["sd"][f"{stem}.{l}.weight_g"]
        dW = f[offs[i]: offs[i + 1]].view(v.shape).contiguous()
        bv, bg = _wn(dW, v, g.reshape(-1).contiguous())
        out[f"{name}.weight_v"], out[f"{name}.weight_g"] = bv.f32(*v.shape).cpu(), bg.f32(*g.shape).cpu()
        out[f"{name}.bias"] = f[offs[i + 1]: offs[i + 2]].cpu()
    return out


@pytest.mark.parametrize("spec", G.specs(), ids=R.spec_id)
def test_param_grads_match_fp64_autograd(spec):
    kind, fw, M = spec
    r = _route(spec)
    sc, c = r["sc"], r["c"]
    got = _lib_grads(r["raw_dev"], sc, kind)
    masks = G.dump_masks(r["bufs"]["fdump"].bytes(), M) if kind == "rad" else None
    ref = G.ref_param_grads(sc["sd_cpu"], c, masks)
    split = G.lib_split(_lib())
    sim, _ = G.sim_param_grads(sc["sd_cpu"], c, split)
    acc = G.allowance_grads(G.allowance_raw(G.reduce_sections(r["op"], absolute=True), G.additions(kind, M, split)), sc["sd_cpu"], kind, sc["mv"])
    rep = G.new_report(R.spec_id(spec))
    worst = G.check_param_grads(rep, got, ref, sim, acc)
    print(f"\n{R.spec_id(spec)}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not rep.viol, "\n".join(rep.viol[:20])
    if kind == "rad":                                       # the radiance-only route leaves the sdf row of the last SDF layer exactly 0
        assert bool((got["sdf.8.weight_v"][0] == 0).all()) and float(got["sdf.8.weight_g"][0]) == 0.0 and float(got["sdf.8.bias"][0]) == 0.0


# ---- 5. the ray-level calls are the chain of their stages ---------------------------------------------------------------------------------------
def _rays(Rn, P, seed):
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.0, 0.0, -2.5]) + 0.1 * torch.randn(Rn, 3, generator=gen)
    d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(Rn, 3, generator=gen), dim=-1) * (1.0 + torch.rand(Rn, 1, generator=gen))
    depth = torch.sort(1.0 + 3.0 * torch.rand(Rn, P, generator=gen), dim=-1).values
    g = torch.rand(Rn, 3, generator=gen) * 1e-2
    g_acc = torch.rand(Rn, generator=gen) * 1e-2
    return [t.to(DEV).contiguous() for t in (o, d, depth, g, g_acc)]


def _wh7_check(sc, pts, nbar, M, bdump, raw, who):
    """RAD_WH7 of a ray-level call: the radiance backward dump's g_f against a7 of the second-order forward dump on (pts, nbar)."""
    lib, Mp = _lib(), R.up(M, 64)
    f2 = Buf(lib.nerfart_sdf_fwd2_dump_bytes(M))
    _rc(lib.nerfart_sdf_fwd2(sc["surf"].data_ptr(), pts.data_ptr(), nbar.data_ptr(), M, f2.ptr, _st()), "sdf_fwd2")
    torch.cuda.synchronize()
    a7 = G.units(f2.bytes()[7 * 2 * Mp * 512: 7 * 2 * Mp * 512 + Mp * 512], Mp, 256)
    gf = G.units(bdump.bytes(), 5, R.up(M, 128), 256)[4, :Mp]
    P, S = {"RAD_WH7": gf.T @ a7}, {"RAD_WH7": gf.abs().T @ a7.abs()}
    rep = G.new_report(who)
    worst = G.check_raw(rep, raw, P, S, {"RAD_WH7": Mp + G.lib_split(lib)(1, Mp, 256)})
    assert not rep.viol, "\n".join(rep.viol[:10])
    return worst["RAD_WH7"]


@pytest.mark.parametrize("with_state", [False, True], ids=["recomputed", "kept-state"])
@pytest.mark.parametrize("Rn,P", [(5, 13), (7, 46)])
@pytest.mark.parametrize("fw", ["VolSDF", "NeuS"])
def test_render_bwd_is_the_chain_of_its_stages(fw, Rn, P, with_state):
    from nerfart_amd import hip
    lib, sc = _lib(), _scene(fw)
    model, surf, rad, vt = sc["model"], sc["surf"], sc["rad"], sc["vt"]
    o, d, d_all, g, g_acc = _rays(Rn, P, 17 * Rn + P)
    M, w_eik, group = Rn * P, 0.1, 4
    scal = G.raw_offsets()[0]["SCALARS"]
    dn = hip.normalize_dirs(d)
    pts, view = hip.ray_points(o, dn, d_all)
    chain = _new_raw()
    entry_raws = []
    if fw == "VolSDF":
        R_bg = float(model.obj_bounding_radius)
        alpha, beta = (float(t.detach()) for t in model.forward_ab())
        sdf, nab, h7 = hip.sdf_nabla_fwd(surf, pts, R_bg, precision=1)
        for _ in range(2):
            raw = _new_raw()
            nb = int(lib.nerfart_volsdf_render_bwd_workspace_bytes(Rn, P, int(with_state)))
            ws = Buf(nb)
            st = (sdf, nab, h7) if with_state else (None, None, None)
            _rc(lib.nerfart_volsdf_render_bwd(surf.data_ptr(), rad.data_ptr(), vt, 6, o.data_ptr(), d.data_ptr(), Rn, P, d_all.data_ptr(), g.data_ptr(),
                                              g_acc.data_ptr(), None, _p(st[0]), _p(st[1]), _p(st[2]), R_bg, alpha, beta, 0, w_eik, group, 1, raw.ptr, ws.ptr,
                                              nb, _st()), "volsdf_render_bwd")
            torch.cuda.synchronize()
            assert ws.guard_ok() and raw.guard_ok()
            entry_raws.append(raw.f32(-1).cpu())
        # the chain, by hand (the list in nerfart_volsdf_render_bwd2)
        inp = dict(pts=pts, view=view, nabla=nab, h7=h7)
        nd = int(lib.nerfart_radiance_dump_bytes(M))
        b = dict(rgb=Buf(M * 12), fdump=Buf(nd), bdump=Buf(nd), g_h7=Buf(M * 1024), g_n=Buf(M * 12), g_sdf=Buf(M * 4), g_rad=Buf(M * 12), sbar=Buf(M * 4),
                 nbar=Buf(M * 12), eik=Buf(Rn * 4))
        _rc(lib.nerfart_radiance_fwd_dump(rad.data_ptr(), vt, pts.data_ptr(), view.data_ptr(), M, nab.data_ptr(), h7.data_ptr(), b["rgb"].ptr, b["fdump"].ptr,
                                          _st()), "radiance_fwd_dump")
        _rc(lib.nerfart_volsdf_composite_bwd(Rn, P, d_all.data_ptr(), sdf.data_ptr(), b["rgb"].ptr, alpha, beta, 0, g.data_ptr(), g_acc.data_ptr(),
                                             b["g_sdf"].ptr, b["g_rad"].ptr, chain.ptr + 4 * scal, _st()), "volsdf_composite_bwd")
        _rc(lib.nerfart_radiance_bwd(rad.data_ptr(), M, b["rgb"].ptr, b["g_rad"].ptr, b["fdump"].ptr, b["bdump"].ptr, b["g_h7"].ptr, b["g_n"].ptr, _st()),
            "radiance_bwd")
        _rc(lib.nerfart_volsdf_pass2_cotangents(pts.data_ptr(), sdf.data_ptr(), b["g_sdf"].ptr, nab.data_ptr(), b["g_n"].ptr, None, Rn, P, R_bg, w_eik, group,
                                                b["sbar"].ptr, b["nbar"].ptr, b["eik"].ptr, _st()), "pass2_cotangents")
        torch.cuda.synchronize()
        assert all(v.guard_ok() for v in b.values())
        sinp = dict(pts=pts, dir=b["nbar"].f32(M, 3), gbar_sdf=b["sbar"].f32(M), gbar_h7=b["g_h7"].f32(M, 256))
        _sdf_entry(sc, sinp, M, chain)
        rinp = dict(inp, g_rgb=b["g_rad"].f32(M, 3))
        _rad_entry(sc, rinp, M, chain, train=1, outs=False)
        wh7 = _wh7_check(sc, pts, b["nbar"].f32(M, 3), M, b["bdump"], entry_raws[0], f"{fw} {Rn}x{P}")
    else:
        s = float(model.forward_s().detach())
        Mm = Rn * (P - 1)
        d_mid = (0.5 * (d_all[:, 1:] + d_all[:, :-1])).contiguous()
        pts_m, view_m = hip.ray_points(o, dn, d_mid)
        sdf, nab, _ = hip.sdf_nabla_fwd(surf, pts, 0.0, want_h7=False, precision=1)
        _, nab_m, h7_m = hip.sdf_nabla_fwd(surf, pts_m, 0.0, precision=1)
        for _ in range(2):
            raw = _new_raw()
            nb = int(lib.nerfart_neus_render_bwd_workspace_bytes(Rn, P, int(with_state)))
            ws = Buf(nb)
            st = (sdf, nab) if with_state else (None, None)
            _rc(lib.nerfart_neus_render_bwd(surf.data_ptr(), rad.data_ptr(), vt, 6, o.data_ptr(), d.data_ptr(), Rn, P, d_all.data_ptr(), g.data_ptr(),
                                            g_acc.data_ptr(), _p(st[0]), _p(st[1]), s, 0, w_eik, group, 1, raw.ptr, ws.ptr, nb, _st()), "neus_render_bwd")
            torch.cuda.synchronize()
            assert ws.guard_ok() and raw.guard_ok()
            entry_raws.append(raw.f32(-1).cpu())
        nd = int(lib.nerfart_radiance_dump_bytes(Mm))
        b = dict(rgb=Buf(Mm * 12), fdump=Buf(nd), bdump=Buf(nd), g_h7=Buf(Mm * 1024), g_n=Buf(Mm * 12), g_sdf=Buf(M * 4), g_rad=Buf(Mm * 12), sbar=Buf(M * 4),
                 nbar=Buf(M * 12), eik=Buf(Rn * 4))
        _rc(lib.nerfart_radiance_fwd_dump(rad.data_ptr(), vt, pts_m.data_ptr(), view_m.data_ptr(), Mm, nab_m.data_ptr(), h7_m.data_ptr(), b["rgb"].ptr,
                                          b["fdump"].ptr, _st()), "radiance_fwd_dump")
        _rc(lib.nerfart_neus_composite_bwd(Rn, P, sdf.data_ptr(), b["rgb"].ptr, s, 0, g.data_ptr(), g_acc.data_ptr(), b["g_sdf"].ptr, b["g_rad"].ptr,
                                           chain.ptr + 4 * (scal + 2), _st()), "neus_composite_bwd")
        _rc(lib.nerfart_radiance_bwd(rad.data_ptr(), Mm, b["rgb"].ptr, b["g_rad"].ptr, b["fdump"].ptr, b["bdump"].ptr, b["g_h7"].ptr, b["g_n"].ptr, _st()),
            "radiance_bwd")
        _rc(lib.nerfart_volsdf_pass2_cotangents(pts.data_ptr(), sdf.data_ptr(), b["g_sdf"].ptr, nab.data_ptr(), None, None, Rn, P, 0.0, w_eik, group,
                                                b["sbar"].ptr, b["nbar"].ptr, b["eik"].ptr, _st()), "pass2_cotangents")
        torch.cuda.synchronize()
        assert all(v.guard_ok() for v in b.values())
        _sdf_entry(sc, dict(pts=pts, dir=b["nbar"].f32(M, 3), gbar_sdf=b["sbar"].f32(M)), M, chain, hbar7=None)            # the samples
        _sdf_entry(sc, dict(pts=pts_m, dir=b["g_n"].f32(Mm, 3), gbar_h7=b["g_h7"].f32(Mm, 256)), Mm, chain, sbar=None)     # the mid-points
        _rad_entry(sc, dict(pts=pts_m, view=view_m, nabla=nab_m, h7=h7_m, g_rgb=b["g_rad"].f32(Mm, 3)), Mm, chain, train=1, outs=False)
        wh7 = _wh7_check(sc, pts_m, b["g_n"].f32(Mm, 3), Mm, b["bdump"], entry_raws[0], f"{fw} {Rn}x{P}")
    a, a2, ch = entry_raws[0], entry_raws[1], chain.f32(-1).cpu()
    assert torch.equal(a[:scal].view(torch.int32), a2[:scal].view(torch.int32)), "two runs of the ray-level call differ"
    assert bool(torch.isfinite(a).all()), "NaN of the workspace fill leaked into raw"
    diff = [s_ for s_ in G.SECTIONS[:12] if s_ != "RAD_WH7" and not torch.equal(G.section(a, s_).view(torch.int32), G.section(ch, s_).view(torch.int32))]
    assert not diff, f"sections that differ from the chain of public stages: {diff}"
    # d loss / d alpha, d beta (VolSDF), d s (NeuS): k_composite_volsdf_bwd / k_composite_neus_bwd add one value per ray with atomicAdd, in
    # whatever order the workgroups retire - the same launch in the entry point and in the chain, but no fixed summation order, so two runs may
    # differ in the last bit BY CONSTRUCTION.  Held to the part-1 bound: each ray's value from a one-ray launch (one add onto 0: exact), their
    # fp64 sum, n = the number of rays.
    per_ray = torch.zeros(Rn, 3, dtype=torch.float64)
    tmp_s, tmp_r = Buf(P * 4), Buf(P * 12)
    for r_ in range(Rn):
        one = Buf(16, zero=True)
        if fw == "VolSDF":
            _rc(lib.nerfart_volsdf_composite_bwd(1, P, d_all.data_ptr() + 4 * r_ * P, sdf.data_ptr() + 4 * r_ * P, b["rgb"].ptr + 12 * r_ * P, alpha, beta, 0,
                                                 g.data_ptr() + 12 * r_, g_acc.data_ptr() + 4 * r_, tmp_s.ptr, tmp_r.ptr, one.ptr, _st()), "volsdf_composite_bwd")
        else:
            _rc(lib.nerfart_neus_composite_bwd(1, P, sdf.data_ptr() + 4 * r_ * P, b["rgb"].ptr + 12 * r_ * (P - 1), s, 0, g.data_ptr() + 12 * r_,
                                               g_acc.data_ptr() + 4 * r_, tmp_s.ptr, tmp_r.ptr, one.ptr + 8, _st()), "neus_composite_bwd")
        torch.cuda.synchronize()
        assert one.guard_ok() and tmp_s.guard_ok() and tmp_r.guard_ok()
        per_ray[r_] = one.f32(4)[:3].cpu().double()
    s_ratio = 0.0
    for raw_, who in ((a, "entry point"), (a2, "entry point, second run"), (ch, "chain")):
        for k in range(3):
            got, allow = float(G.section(raw_, "SCALARS")[k]), Rn * G.EPS * float(per_ray[:, k].abs().sum())
            err = abs(got - float(per_ray[:, k].sum()))
            assert err <= allow, f"{who}: scalar {k}: |got - sum of the rays' values| = {err:.3e}, allowed {allow:.3e}"
            s_ratio = max(s_ratio, err / allow) if allow > 0 else s_ratio
    assert float(per_ray.abs().sum()) > 0
    # the eikonal scalar is a deterministic two-stage sum inside the entry point: the same bits in both runs, each held to the bound.  (The chain has
    # no public stage for that sum: its SCALARS[3] stays 0 and is not looked at.)
    assert torch.equal(G.section(a, "SCALARS")[3:].view(torch.int32), G.section(a2, "SCALARS")[3:].view(torch.int32)), "the eikonal scalar differs between two runs"
    eik = b["eik"].f32(Rn).cpu().double()
    e_allow = Rn * G.EPS * float(eik.abs().sum())
    assert float(eik.abs().sum()) > 0
    for raw_ in (a, a2):
        e_err = abs(float(G.section(raw_, "SCALARS")[3]) - float(eik.sum()))
        assert e_err <= e_allow, (e_err, e_allow)
    wh7_chain = float((G.section(a, "RAD_WH7") - G.section(ch, "RAD_WH7")).abs().max() / G.section(ch, "RAD_WH7").abs().max())
    print(f"\n{fw} {Rn} x {P} {'kept state' if with_state else 'recomputed'}: 11 sections bit-identical to the chain;  RAD_WH7 observed / allowed "
          f"{wh7:.4f} (vs the chain through the rounded h7: {wh7_chain:.2e} of the largest element);  alpha / beta / s scalars {s_ratio:.3f};  "
          f"eikonal scalar {e_err / max(e_allow, 1e-300):.3f}")
