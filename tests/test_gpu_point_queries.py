"""The forward point queries - nerfart_sdf_fwd[_rays], nerfart_sdf_nabla_fwd[_rays], nerfart_radiance_fwd[_rays] - at every precision their dispatchers
accept, against the fp64 references and the allowances of tests/point_query_ref.py, on the trained-like weight state (dense encoding columns, non-zero
biases, weight_g far from |weight_v|) that tests/test_point_query_ref.py shows the comparator to reject every mutant on.  Called through hip.lib and
ctypes: every output buffer is the test's own, pre-filled with 0xFF bytes and followed by a guard tail that must come back untouched, as must the
padding columns of a strided output.  One line per case: max err / A per output (1.00 = the allowance; 0.25 = the stand-in's own error).

States: 'A' for the fp32 and split-bf16 precisions, 'B' (one hidden layer's biases at 0.2) for the fp16 precisions 4 and 5 on VolSDF; NeuS runs on its
state 'A' at every precision (it adds the view embedding and the call without clamp; the mutant matrix is VolSDF's).

Worst max err / A per entry point, precision and output on an MI355X (gfx950), over VolSDF with R_bg 3 and 0 and NeuS: the 14 sizes M = 1 .. 1000 /
ray mode (273 points) / 100,003 points.  Every case passed; every fill check (guard tails, padding columns of the strided sdf_out) held bit for bit.
    nerfart_sdf_fwd[_rays]         0 fp32     sdf 0.31 / 0.47 / 0.32
                                   1 bf16x3   sdf 0.26 / 0.29 / 0.23
                                   4 fp16x2   sdf 0.29 / 0.25 / 0.26
                                   5 fp16x1   sdf 0.28 / 0.32 / 0.27
    nerfart_sdf_nabla_fwd[_rays]   0 fp32, reverse mode     sdf 0.31 / 0.47 / 0.32   nabla 0.40 / 0.26 / 0.23   h7 0.32 / 0.37 / 0.27
                                   3 fp32, forward mode     sdf 0.31 / 0.47 / 0.32   nabla 0.29 / 0.39 / 0.22   h7 0.32 / 0.37 / 0.27
                                   1 bf16x3, reverse mode   sdf 0.26 / 0.29 / 0.23   nabla 0.25 / 0.25 / 0.28   h7 0.28 / 0.26 / 0.27
                                   2 bf16x3, forward mode   sdf 0.26 / 0.29 / 0.23   nabla 0.25 / 0.32 / 0.25   h7 0.29 / 0.26 / 0.27
                                   4 fp16x2, reverse mode   sdf 0.29 / 0.25 / 0.26   nabla 0.27 / 0.33 / 0.23   h7 0.26 / 0.25 / 0.25
    nerfart_radiance_fwd[_rays]    0 fp32     rgb 0.33 / 0.31 / 0.26
                                   1 bf16x3   rgb 0.28 / 0.31 / 0.26
                                   4 fp16x2   rgb 0.25 / 0.26 / 0.25
0.25 is the stand-in's own error: most of every tier's error is the rounding of its operands (the fp32 fold of weight_norm, the bf16 / fp16 terms of the
weights and of the inputs), which the kernels and the stand-in share; the summation order and the hardware's exp / log move it by the rest.
The same kernels on a blob packed from the state with one fault injected (test_kernels_on_a_mutated_blob_are_rejected) land at 14.7 (the feature bias
one row off, fp16x2 rgb) to 4.8e5 times A; the smallest SDF fault, two biases of one hidden layer exchanged, at 27 (fp16x1) to 1.0e4 (fp32).
"""
import functools

import pytest
import torch

import point_query_ref as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096                     # bytes behind every output
NAME = {0: "fp32", 3: "fp32", 1: "bf16x3", 2: "bf16x3", 4: "fp16x2"}
SCENES = [("VolSDF", 3.0), ("VolSDF", 0.0), ("NeuS", 0.0)]


def _state_name(fw, precision):
    return "B" if fw == "VolSDF" and Q.PRECISION[precision][0].startswith("fp16") else "A"


@functools.lru_cache(maxsize=None)
def _scene(fw, name):
    from nerfart_amd import scene
    sd = Q.trained_like_state(fw, 0, Q.BIG_BIAS_LAYER if name == "B" else None)
    bad, _ = Q.check_state(sd, fw)
    assert not bad, bad
    model, _, _ = scene.build_model(fw, seed=0, beta=0.01 if fw == "VolSDF" else None, device=DEV, precision="fp32")
    model.load_state_dict(sd)
    nets = Q.Nets(sd)
    assert nets.view_tiles == model.view_tiles
    return dict(sd=sd, model=model, nets=nets, nets_dev=nets.to(DEV), share={})


@functools.lru_cache(maxsize=None)
def _blobs(fw, name, precision):
    return _pack(_scene(fw, name)["model"], precision)


def _pack(model, precision):
    """(surface blob, radiance blob or None) through the model's own packing path (nerfart_pack_surface_blob / nerfart_pack_radiance_blob)."""
    if precision == 5:
        model.set_precision("bf16x3").set_sampler_precision("fp16x1", guard=0.05)       # one-term weights rounded to nearest, the kernel's scaled recursion
        blob, p = model.packed_sampler()
        assert p == 5
        return blob, None
    model.set_precision(NAME[precision])
    return model.packed()


@functools.lru_cache(maxsize=None)
def _points(fw, name, which):
    """The point sets: 'pts' (1000 rows; every size M takes the first M), 'rays' (ray mode), 'wrap' (100,003 rows, on the device)."""
    s = _scene(fw, name)
    if which == "pts":
        p, v = Q.case_points(s["nets"], fw)
        return dict(pts=p, view=v, rays=None, nets=s["nets"], share={})
    if which == "wrap":
        p, v = Q.case_points(s["nets"], fw, Q.WRAP, seed=5)
        return dict(pts=p.to(DEV), view=v.to(DEV), rays=None, nets=s["nets_dev"], share={})
    g = torch.Generator().manual_seed(3)
    n_rays, n_slots, n_per_ray, stride = 37, 21, 13, 16
    scale = 1.0 if fw == "VolSDF" else 1.0 / 3.0
    o = (torch.randn(n_rays, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, -2.5])) * scale
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 1.0]), dim=-1)
    idx = torch.randperm(n_rays, generator=g)[:n_slots].to(torch.int32)
    depth = torch.rand(n_slots, stride, generator=g) * 6 * scale
    depth[:, n_per_ray:] = 1e30                                       # never read
    return dict(pts=None, view=None, rays=dict(o=o, d=d, idx=idx, depth=depth, n_per_ray=n_per_ray), nets=s["nets"], share={})


@functools.lru_cache(maxsize=None)
def _case(kind, fw, precision, R_bg, which):
    name = _state_name(fw, precision)
    P = _points(fw, name, which)
    c = Q.make_case(kind, fw, precision, P["nets"], P["pts"], P["view"], R_bg=R_bg, rays=P["rays"], sd=_scene(fw, name)["sd"], share=P["share"])
    Q.allowances(c)
    return c


# ---- calling the library ------------------------------------------------------------------------------------------------------------------------
def _buf(nbytes):
    return torch.full((nbytes + GUARD,), Q.FILL, dtype=torch.uint8, device=DEV)


def _f32(buf, *shape):
    n = 4
    for s in shape:
        n *= s
    return buf[:n].view(torch.float32).view(*shape)


def _untouched(buf, nbytes):
    return bool((buf[nbytes:] == Q.FILL).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rc(rc, who):
    from nerfart_amd import hip
    assert rc == 0, (who, rc, hip.lib.nerfart_last_error().decode())


def _ray_args(c):
    r = c["rays"]
    t = {k: r[k].to(DEV).contiguous() for k in ("o", "d", "idx", "depth")}
    return t, (t["o"].data_ptr(), t["d"].data_ptr(), t["idx"].data_ptr(), t["depth"].data_ptr(), r["idx"].numel(), r["n_per_ray"], r["depth"].shape[1])


def _run(c, M, want_h7=True, blobs=None):
    """One call of the case's entry point on its first M rows (ray mode: all of them) -> (outputs, list of buffers written out of place)."""
    from nerfart_amd import hip
    lib, p, kind = hip.lib, c["precision"], c["kind"]
    name = _state_name(c["fw"], p)
    surf, rad = blobs if blobs is not None else _blobs(c["fw"], name, p)
    rays = c["rays"] is not None
    bad = []
    if rays:
        keep, ra = _ray_args(c)
        n_slots, npr = ra[4], ra[5]
    else:
        x = c["x32"][:M].to(DEV).contiguous()
    if kind == "sdf":
        if rays:
            stride = npr + 3                                          # out_stride > n_per_ray
            out = _buf(n_slots * stride * 4)
            _rc(lib.nerfart_sdf_fwd_rays(surf.data_ptr(), p, *ra, c["R_bg"], out.data_ptr(), stride, _stream()), "sdf_fwd_rays")
            full = out[: n_slots * stride * 4].view(n_slots, stride * 4)
            if not bool((full[:, npr * 4:] == Q.FILL).all()):
                bad.append("padding columns of sdf_out")
            res = dict(sdf=_f32(out, n_slots, stride)[:, :npr].reshape(-1))
            nbytes = dict(sdf=n_slots * stride * 4)
        else:
            out = _buf(M * 4)
            _rc(lib.nerfart_sdf_fwd(surf.data_ptr(), p, x.data_ptr(), M, c["R_bg"], out.data_ptr(), _stream()), "sdf_fwd")
            res, nbytes = dict(sdf=_f32(out, M)), dict(sdf=M * 4)
        bufs = dict(sdf=out)
    elif kind == "nabla":
        nb = int(lib.nerfart_sdf_nabla_workspace_bytes(p))
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=DEV)
        bufs = dict(sdf=_buf(M * 4), nabla=_buf(M * 12), h7=_buf(M * 1024 if want_h7 else 0))
        nbytes = dict(sdf=M * 4, nabla=M * 12, h7=M * 1024 if want_h7 else 0)
        tail = (bufs["sdf"].data_ptr(), bufs["nabla"].data_ptr(), bufs["h7"].data_ptr() if want_h7 else None, ws.data_ptr() if nb else None, nb, _stream())
        if rays:
            _rc(lib.nerfart_sdf_nabla_fwd_rays(surf.data_ptr(), p, *ra, c["R_bg"], *tail), "sdf_nabla_fwd_rays")
        else:
            _rc(lib.nerfart_sdf_nabla_fwd(surf.data_ptr(), p, x.data_ptr(), M, c["R_bg"], *tail), "sdf_nabla_fwd")
        res = dict(sdf=_f32(bufs["sdf"], M), nabla=_f32(bufs["nabla"], M, 3), h7=_f32(bufs["h7"], M, 256) if want_h7 else None)
    else:
        Q.reference(c)
        nab, h7 = c["nabla_in"][:M].to(DEV).contiguous(), c["h7_in"][:M].to(DEV).contiguous()
        vt = c["nets"].view_tiles
        out = _buf(M * 12)
        if rays:
            _rc(lib.nerfart_radiance_fwd_rays(rad.data_ptr(), p, vt, *ra, nab.data_ptr(), h7.data_ptr(), out.data_ptr(), _stream()), "radiance_fwd_rays")
        else:
            v = c["view32"][:M].to(DEV).contiguous()
            _rc(lib.nerfart_radiance_fwd(rad.data_ptr(), p, vt, x.data_ptr(), v.data_ptr(), M, nab.data_ptr(), h7.data_ptr(), out.data_ptr(), _stream()), "radiance_fwd")
        res, bufs, nbytes = dict(rgb=_f32(out, M, 3)), dict(rgb=out), dict(rgb=M * 12)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                         # a GPU fault: nothing more is started on the device in this session
        pytest.exit(f"{c['id']} M = {M}: {e}", returncode=3)
    bad += [k for k in bufs if not _untouched(bufs[k], nbytes[k])]
    return res, bad


def _hold(c, sizes, **kw):
    worst, lines = {}, []
    for M in sizes:
        out, bad = _run(c, M, **kw)
        assert not bad, f"{c['id']} M = {M}: written past the end of / into the padding of {bad}"
        viol, ratio = Q.check(c, out, rows=M)
        lines.append(f"    M = {M}: {Q.fmt(ratio)}")
        for k, v in ratio.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert not viol, "\n".join(viol[:10] + lines)
    extra = "".join(f" {k}={v}" for k, v in kw.items())
    print(f"\n{c['id']}{extra}: max err / A over M in {list(sizes)}: {Q.fmt(worst)}   (A: " + "  ".join(f"{k} {a:.2e}" for k, a in c["A"].items()) + ")")
    return worst


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------------
def test_precisions_are_the_dispatchers():
    """The precisions of this module are what csrc/mlp_chain.hip accepts: every other one is refused by name."""
    from nerfart_amd import hip
    surf, rad = _blobs("VolSDF", "A", 0)
    x = torch.zeros(4, 3, device=DEV)
    for p in range(-1, 8):
        if p not in Q.SDF_PRECISIONS:
            with pytest.raises(hip.NerfartHipError, match="precision"):
                hip.sdf_fwd(surf, x, 3.0, precision=p)
        if p not in Q.NABLA_PRECISIONS:
            with pytest.raises(hip.NerfartHipError, match="precision"):
                hip.sdf_nabla_fwd(surf, x, 3.0, precision=p)
        if p not in Q.RAD_PRECISIONS:
            with pytest.raises(hip.NerfartHipError, match="precision"):
                hip.radiance_fwd(rad, 1, x, x, x, torch.zeros(4, 256, device=DEV), precision=p)


@pytest.mark.parametrize("precision", Q.SDF_PRECISIONS)
@pytest.mark.parametrize("fw,R_bg", SCENES)
def test_sdf_fwd(fw, R_bg, precision):
    _hold(_case("sdf", fw, precision, R_bg, "pts"), Q.SIZES)


@pytest.mark.parametrize("want_h7", [True, False])
@pytest.mark.parametrize("precision", Q.NABLA_PRECISIONS)
@pytest.mark.parametrize("fw,R_bg", SCENES)
def test_sdf_nabla_fwd(fw, R_bg, precision, want_h7):
    _hold(_case("nabla", fw, precision, R_bg, "pts"), Q.SIZES, want_h7=want_h7)


@pytest.mark.parametrize("precision", Q.RAD_PRECISIONS)
@pytest.mark.parametrize("fw", ["VolSDF", "NeuS"])
def test_radiance_fwd(fw, precision):
    _hold(_case("rad", fw, precision, Q.R_BG[fw], "pts"), Q.SIZES)


RAY_CASES = [("sdf", p) for p in Q.SDF_PRECISIONS] + [("nabla", p) for p in Q.NABLA_PRECISIONS] + [("rad", p) for p in Q.RAD_PRECISIONS]


@pytest.mark.parametrize("kind,precision", RAY_CASES)
@pytest.mark.parametrize("fw", ["VolSDF", "NeuS"])
def test_ray_mode(fw, kind, precision):
    """A permuted ray_idx subset, depth_stride > n_per_ray, out_stride > n_per_ray (nerfart_sdf_fwd_rays: the one entry point with an output stride):
    the points are o[idx] + d[idx] depth in two fp32 roundings, the padding columns and everything past row M keep the fill bit for bit."""
    c = _case(kind, fw, precision, Q.R_BG[fw], "rays")
    _hold(c, (c["M"],))


@pytest.mark.parametrize("kind,precision", RAY_CASES)
def test_grid_wrapping_size(kind, precision):
    """100,003 points: more tiles than workgroups, so every workgroup loops and the chunk stream wraps.  Reference and stand-in in torch on the device."""
    _hold(_case(kind, "VolSDF", precision, 3.0, "wrap"), (Q.WRAP,))


@pytest.mark.parametrize("mut", Q.WEIGHT_MUTANTS)
def test_kernels_on_a_mutated_blob_are_rejected(mut):
    """The comparator's teeth on the hardware's own numbers: the blob is packed from the state with one fault injected (rolled biases, two biases
    exchanged, weight_g ignored, the skip's encoding columns or its 1 / sqrt 2 dropped, the feature bias one row off) and every entry point the fault
    reaches, at every precision, must land outside the allowance of the true state."""
    import copy
    for name, precisions in (("A", (0, 1, 2, 3)), ("B", (4, 5))):
        s = _scene("VolSDF", name)
        model = copy.deepcopy(s["model"])
        model.load_state_dict(Q.mutate_state(s["sd"], mut))
        for p in precisions:
            blobs = _pack(model, p)
            for kind in ("sdf", "nabla", "rad"):
                if p not in {"sdf": Q.SDF_PRECISIONS, "nabla": Q.NABLA_PRECISIONS, "rad": Q.RAD_PRECISIONS}[kind] or (kind == "rad") != (mut == "feat_bias_row"):
                    continue
                c = _case(kind, "VolSDF", p, 3.0, "pts")
                out, bad = _run(c, 1000, blobs=blobs)
                viol, ratio = Q.check(c, out)
                print(f"\n{c['id']} on a blob with {mut}: {Q.fmt(ratio)}")
                assert not bad and viol and all(v > 1.0 for v in ratio.values()), (c["id"], mut, ratio)


def test_direct_against_staged():
    """The relations the existing tests state between entry points, on the trained-like state: precision 4's nerfart_sdf_fwd and the sdf of
    nerfart_sdf_nabla_fwd are the same bits (test_gpu_fp16x2.py); the reverse-mode and the forward-mode kernels agree to 1e-6 (sdf, h7) and 2e-5 (nabla)
    at precisions 0 / 3 (test_gpu_parity.py) and to 5e-4 (nabla) and 1e-4 (h7) at 1 / 2 (test_gpu_bf16x3.py)."""
    def close(name, a, b, atol, rtol):
        err = (a.double() - b.double()).abs()
        print(f"  [{name}] max abs err {float(err.max()):.3e}")
        assert bool(((err <= atol + rtol * b.double().abs()) | (a == b)).all()), (name, float(err.max()))
    for M in (1000, 129):
        direct, _ = _run(_case("sdf", "VolSDF", 4, 3.0, "pts"), M)
        staged, _ = _run(_case("nabla", "VolSDF", 4, 3.0, "pts"), M)
        assert torch.equal(direct["sdf"], staged["sdf"]), f"precision 4, M = {M}: nerfart_sdf_fwd and nerfart_sdf_nabla_fwd give different sdf bits"
        rev, _ = _run(_case("nabla", "VolSDF", 0, 3.0, "pts"), M)
        fwd, _ = _run(_case("nabla", "VolSDF", 3, 3.0, "pts"), M)
        close("0 vs 3 sdf", rev["sdf"], fwd["sdf"], 1e-6, 1e-6)
        close("0 vs 3 nabla", rev["nabla"], fwd["nabla"], 2e-5, 2e-5)
        close("0 vs 3 h7", rev["h7"], fwd["h7"], 1e-6, 1e-6)
        rev, _ = _run(_case("nabla", "VolSDF", 1, 3.0, "pts"), M)
        fwd, _ = _run(_case("nabla", "VolSDF", 2, 3.0, "pts"), M)
        close("1 vs 2 nabla", rev["nabla"], fwd["nabla"], 5e-4, 5e-4)
        close("1 vs 2 h7", rev["h7"], fwd["h7"], 1e-4, 1e-4)
