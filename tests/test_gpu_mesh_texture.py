"""csrc/mesh_texture.hip (mesh_util.texel_points / bake_texture / extract_mesh(texture_model=)) against the numpy statement
tests/mesh_texture_ref.py, which tests/test_mesh_texture_ref.py holds to the two properties the atlas is built on.  The owner of every texel is
compared by equality, every point must lie within the reference's derived rounding bound, invalid texels must be exactly 0, a guard row past
the end must survive and a second run must give the same bits.  The projection step is held to its float64 formula within its derived bound;
the bake to an affine colour; extract_mesh end to end to the same colour rule evaluated by hand.

Observed on an MI355X (first run; every assertion is observed <= allowed): points, worst error / bound 0.64 (noise_24, P = 7; 0.61 on the
non-cubic mesh, 0.50 by hand); projection step 0.88 of its bound; the analytic sphere 2.33 u r of the 10 allowed; bilinear samples of the baked
affine colour at most 0.5000 levels off (allowed 0.5 + 0.00255).  Mean |sdf| over the valid texels of the decimated N = 48 meshes: VolSDF
5.941e-3 without projection, 2.363e-6 after two steps; NeuS 8.958e-3 and 1.331e-6 (only the ordering is asserted)."""
import os

import numpy as np
import pytest
import torch

import mesh_texture_ref as ref
from mesh_pipeline_ref import decimated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
PATCHES = [1, 2, 4, 7]
GUARD_F, GUARD_I = 1.0e30, 0x5A5A5A5A


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def _seven():
    """Seven faces by hand over nine vertices: a fan, a far-away sliver, a face used twice with the other winding - and large coordinates."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.5, 1.0, -0.5], [-0.75, 0.5, 0.125], [-0.5, -1.0, 0.75], [0.625, -0.875, 1.5],
                  [100.0, 200.0, -300.0], [100.001, 200.0, -300.0], [100.0, 200.002, -299.999]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 1], [6, 7, 8], [2, 1, 0]], dtype=np.int32)
    return v, f


def _marching_cubes(name):
    from nerfart_amd import mesh_util
    from test_gpu_marching_cubes import CASES
    build, level, spacing, origin = CASES[name]
    verts, faces = mesh_util.marching_cubes(build(), level=level, spacing=spacing, origin=origin)
    return verts.cpu().numpy(), faces.cpu().numpy()


MESHES = {
    "one_face": lambda: (np.array([[0.1, 0.2, 0.3], [1.3, -0.4, 0.6], [-0.2, 0.9, 1.1]], np.float32), np.array([[0, 1, 2]], np.int32)),
    "two_faces": lambda: (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.5], [0.0, 1.0, 0.0]], np.float32),
                          np.array([[0, 1, 2], [0, 2, 3]], np.int32)),
    "seven_faces": _seven,
    "noise_24": lambda: _marching_cubes("noise_24"),
    "noncubic_5x7x70": lambda: _marching_cubes("noncubic_5x7x70"),
}
_MESH, _REF = {}, {}


def mesh(name):
    """(verts, faces) as numpy and as tensors on the GPU: built once, shared, never modified."""
    if name not in _MESH:
        v, f = MESHES[name]()
        _MESH[name] = (v, f, dev(v), dev(f))
    return _MESH[name]


def reference(name, P):
    if (name, P) not in _REF:
        v, f, _, _ = mesh(name)
        _REF[(name, P)] = ref.points(v, f, P)
    return _REF[(name, P)]


def raw_atlas_points(gv, gf, P):
    """nerfart_mesh_atlas_points into guarded buffers - one row more than the atlas has, filled beforehand: (points [W H, 3], face_of [H, W],
    info); asserts that the guard row survived and that no element before it kept the fill."""
    from nerfart_amd import hip
    S, Cw, Ch, W, H = hip.mesh_atlas_layout(gf.shape[0], P)
    points = torch.full((W * H + 1, 3), GUARD_F, dtype=torch.float32, device=DEV)
    face_of = torch.full((W * H + 1,), GUARD_I, dtype=torch.int32, device=DEV)
    info = torch.full((1,), GUARD_I, dtype=torch.int32, device=DEV)
    rc = hip.lib.nerfart_mesh_atlas_points(gv.data_ptr(), gf.data_ptr(), gv.shape[0], gf.shape[0], P, points.data_ptr(), face_of.data_ptr(),
                                           info.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.nerfart_last_error()
    assert bool((points[-1] == GUARD_F).all()) and int(face_of[-1]) == GUARD_I, "the row past the end was written"
    assert not bool((points[:-1] == GUARD_F).any()) and not bool((face_of[:-1] == GUARD_I).any()), "an element of the atlas was not written"
    return points[:-1], face_of[:-1].reshape(H, W), info


@pytest.mark.parametrize("P", PATCHES)
@pytest.mark.parametrize("name", list(MESHES))
def test_points_and_owners_are_the_reference(name, P):
    from nerfart_amd import hip, mesh_util
    v, f, gv, gf = mesh(name)
    r_pts, r_face, r_bound = reference(name, P)
    assert hip.mesh_atlas_layout(len(f), P) == ref.layout(len(f), P) == mesh_util.atlas_layout(len(f), P)
    points, face_of, info = raw_atlas_points(gv, gf, P)
    assert int(info) == 0
    assert np.array_equal(face_of.cpu().numpy(), r_face), "face_of"
    got = points.cpu().numpy().astype(np.float64)
    ok = r_face.reshape(-1) >= 0
    assert ok.sum() > 0 and np.all(got[~ok] == 0.0) and not np.signbit(got[~ok]).any(), "an invalid texel's point is not +0"
    err = np.abs(got - r_pts)[ok]
    ratio = float(np.max(err / np.maximum(r_bound[ok], 1e-300)))
    print(f"[texture] {name}, P = {P}: F = {len(f)}, {r_face.shape[1]} x {r_face.shape[0]} texels, {int(ok.sum())} valid; worst error / bound = "
          f"{ratio:.3f} (largest error {err.max():.3e})")
    assert np.all(err <= r_bound[ok])
    if name == "noise_24":
        assert r_face.shape[1] > 64 and r_face.shape[0] > 4 and r_face.shape[1] % 64 != 0, "more than one block each way, the last one ragged"
    # a second run gives the same bits, and so does the wrapper that allocates for itself
    again, face_again, _ = raw_atlas_points(gv, gf, P)
    assert torch.equal(points.view(torch.int32), again.view(torch.int32)) and torch.equal(face_of, face_again)
    w_points, w_face, w_info = hip.mesh_atlas_points(gv, gf, P)
    assert torch.equal(points.view(torch.int32), w_points.view(torch.int32)) and torch.equal(face_of, w_face) and int(w_info) == 0
    t_points, t_face = mesh_util.texel_points(gv, gf, P)
    assert torch.equal(w_points.view(torch.int32), t_points.view(torch.int32)) and torch.equal(w_face, t_face)
    assert tuple(t_points.shape) == (r_face.size, 3) and tuple(t_face.shape) == r_face.shape


def test_refusals_raise_and_nothing_is_read_out_of_bounds():
    from nerfart_amd import hip, mesh_util
    v, f, gv, gf = mesh("seven_faces")
    for where, value in ((3, len(v)), (6, -1), (0, 2 ** 31 - 1)):
        bad = gf.clone()
        bad[where, 1] = value
        with pytest.raises(ValueError, match="face holds a vertex index outside"):
            mesh_util.texel_points(gv, bad, 2)
        points, face_of, info = raw_atlas_points(gv, bad, 2)            # the flagged face is written as invalid, every other texel as always
        r_pts, r_face, r_bound = reference("seven_faces", 2)
        want = np.where(r_face == where, -1, r_face)
        assert int(info) == 1 and np.array_equal(face_of.cpu().numpy(), want)
        got = points.cpu().numpy().astype(np.float64)
        assert np.all(got[want.reshape(-1) < 0] == 0.0) and np.all(np.abs(got - r_pts)[want.reshape(-1) >= 0] <= r_bound[want.reshape(-1) >= 0])
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        mesh_util.texel_points(gv.cpu(), gf.cpu(), 2)
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        hip.mesh_atlas_points(gv, gf.cpu(), 2)
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        hip.mesh_project_step(gv.cpu(), gv[:, 0].cpu(), gv.cpu(), 0.0, 1.0)
    with pytest.raises(hip.NerfartHipError, match="int32"):
        mesh_util.texel_points(gv, gf.long(), 2)
    for patch in (0, -3):
        with pytest.raises(ValueError, match="patch"):
            mesh_util.texel_points(gv, gf, patch)
        with pytest.raises(ValueError, match="patch"):
            mesh_util.bake_texture(gv, gf, lambda p: p, patch=patch)
    with pytest.raises(ValueError, match="project"):
        mesh_util.texel_points(gv, gf, 2, project=-1)
    with pytest.raises(ValueError, match="query_fn"):
        mesh_util.texel_points(gv, gf, 2, project=1, max_step=0.1)
    with pytest.raises(ValueError, match="max_step"):
        mesh_util.texel_points(gv, gf, 2, project=1, query_fn=lambda p: (p[:, 0], p))
    with pytest.raises(ValueError, match="no faces"):
        mesh_util.texel_points(gv, gf[:0], 2)
    # past the size limit: refused by F and P alone, before anything is allocated
    many = torch.zeros(600_000, 3, dtype=torch.int32, device=DEV)        # 300,000 cells, 548 a side, of 33 texels: 18,084 > 16,384
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for faces, patch in ((many, 30), (gf, 16382)):
        with pytest.raises(ValueError, match=f"F = {faces.shape[0]}.*P = {patch}.*simplify_factor"):
            mesh_util.texel_points(gv, faces, patch)
        with pytest.raises(hip.NerfartHipError, match="mesh_atlas_layout"):
            hip.mesh_atlas_points(gv, faces, patch)
        with pytest.raises(hip.NerfartHipError, match="mesh_atlas_layout"):
            hip.mesh_atlas_layout(faces.shape[0], patch)
    assert torch.cuda.memory_allocated() == before
    # the refused and flagged runs left nothing behind: the same mesh still gives the reference
    points, face_of = mesh_util.texel_points(gv, gf, 2)
    r_pts, r_face, r_bound = reference("seven_faces", 2)
    assert np.array_equal(face_of.cpu().numpy(), r_face) and np.all(np.abs(points.cpu().numpy() - r_pts) <= r_bound)


# ---- the projection step ---------------------------------------------------------------------------------------------------------------------

def test_project_step_is_the_float64_formula_within_its_bound():
    from nerfart_amd import hip
    rng = np.random.default_rng(11)
    n = 1000 + 37                                                     # five blocks of 256, the last ragged
    p = rng.normal(size=(n, 3)).astype(np.float32)
    g = (rng.normal(size=(n, 3)) * rng.uniform(0.05, 3.0, size=(n, 1))).astype(np.float32)
    s = rng.normal(scale=0.2, size=n).astype(np.float32)
    level, max_step = 0.1, 0.2
    g[5], g[6, 2], g[7, 0], g[8] = 0.0, np.nan, np.inf, 1e-7            # zero, NaN and infinite gradients; |g|^2 = 3e-14 < 1e-12
    s[9], s[10] = np.nan, -np.inf
    want, moved, bound = ref.project_step(p, s, g, np.float32(level), np.float32(max_step))
    assert not moved[5:11].any() and moved[:5].all() and moved[11:].all()
    gp = dev(p)
    gp_guard = torch.cat([gp, torch.full((1, 3), GUARD_F, device=DEV)])
    part = gp_guard[:n]
    hip.mesh_project_step(part, dev(s), dev(g), level, max_step)
    got32 = gp_guard.cpu().numpy()
    assert np.all(got32[n] == np.float32(GUARD_F)), "the row past the end was written"
    got32 = got32[:n]
    assert np.array_equal(got32[~moved].view(np.int32), p[~moved].view(np.int32)), "a row that must stay was moved"
    got = got32.astype(np.float64)
    err = np.abs(got - want)
    print(f"[texture] project_step: worst error / bound = {np.max(err[moved] / bound[moved]):.3f}; {int((np.linalg.norm(want - p, axis=1) > 0.1999).sum())} "
          f"of {n} rows clamped")
    assert np.all(err <= bound)
    # the clamp: m <= max_step exactly; c = fl(m / gn), d_k = fl(c g_k), |g| / gn <= 1 + 5 u / 2, and the stored p'_k differs from p_k + d_k by at
    # most u |p'_k|: |p' - p| <= max_step (1 + 5 u) (1 + u) + u |p'|
    step = np.linalg.norm(got - p.astype(np.float64), axis=1)
    with np.errstate(all="ignore"):                                # the rows that stay have no step length
        full = np.abs(s.astype(np.float64) - np.float32(level)) / np.linalg.norm(g.astype(np.float64), axis=1)
    assert (full[moved] > 2 * max_step).sum() > 20 and (full[moved] < 0.5 * max_step).sum() > 20          # both sides of the clamp are there
    assert np.all(step <= np.float32(max_step) * (1 + 5 * U) * (1 + U) + U * np.linalg.norm(got, axis=1))
    # a second run from the same input gives the same bits
    again = dev(p)
    hip.mesh_project_step(again, dev(s), dev(g), level, max_step)
    assert np.array_equal(again.cpu().numpy().view(np.int32), got32.view(np.int32))
    hip.mesh_project_step(again[:0], dev(s)[:0], dev(g)[:0], level, max_step)              # n = 0: nothing to do
    with pytest.raises(hip.NerfartHipError, match="max_step"):
        hip.mesh_project_step(again, dev(s), dev(g), level, 0.0)
    with pytest.raises(hip.NerfartHipError, match="expected"):
        hip.mesh_project_step(again, dev(s)[:-1], dev(g), level, max_step)


def test_one_step_lands_on_an_analytic_sphere():
    """Field |x| - r with its gradient x / |x|, points at |x| in [0.5 r, 1.5 r], max_step = r (never reached: |e| <= r / 2): the exact step ends at
    |x'| = r.  What the fp32 run may differ by, as Euclidean distances in units of u r (u = 2^-24): the kernel's own bound u (11 |d| + |p|) <=
    u (11 r / 2 + 3 r / 2) = 7; the test's sdf is rounded to fp32, |e| u <= 1 / 2; its gradient is rounded per component, |dg| <= u, which moves
    d = -e g / |g|^2 by at most 3 |e| u <= 3 / 2.  Together 9, and 10 covers the second-order terms."""
    from nerfart_amd import hip
    rng = np.random.default_rng(3)
    r, n = 0.7, 4096 + 3
    x = rng.normal(size=(n, 3))
    x *= (rng.uniform(0.5 * r, 1.5 * r, size=n) / np.linalg.norm(x, axis=1))[:, None]
    x32 = x.astype(np.float32)
    norm = np.linalg.norm(x32.astype(np.float64), axis=1)
    sdf = (norm - r).astype(np.float32)
    grad = (x32.astype(np.float64) / norm[:, None]).astype(np.float32)
    pts = dev(x32)
    hip.mesh_project_step(pts, dev(sdf), dev(grad), 0.0, r)
    off = np.abs(np.linalg.norm(pts.cpu().numpy().astype(np.float64), axis=1) - r)
    print(f"[texture] sphere: before max ||x| - r| = {np.abs(norm - r).max():.3f}, after {off.max():.3e} = {off.max() / (U * r):.2f} u r (allowed 10)")
    assert np.abs(norm - r).max() > 0.45 * r and np.all(off <= 10 * U * r)


# ---- the bake --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,P", [("seven_faces", 1), ("seven_faces", 2), ("seven_faces", 4), ("seven_faces", 7), ("two_faces", 4), ("noise_24", 2)])
def test_bake_of_an_affine_colour_samples_back_to_it(name, P):
    """Texels carry quantize_colors of an affine function of their points, with values in [0.1, 0.9] at every texel, the gutter included, so
    nothing is clamped.  Quantisation moves a texel by at most half a level, a bilinear sample is a convex combination of texels of the one
    face, and by the atlas's second property the unquantised sample is the function itself: |sample - function| <= 0.5 / 255 (+ 1e-5 for the fp32
    evaluation of the function and of the points)."""
    from nerfart_amd import mesh_util
    v, f, gv, gf = mesh(name)
    r_pts, r_face, _ = reference(name, P)
    ok = r_face.reshape(-1) >= 0
    rng = np.random.default_rng(P)
    centre = r_pts[ok].mean(axis=0)
    A = rng.normal(size=(3, 3))
    A *= 0.4 / np.abs((r_pts[ok] - centre) @ A).max()                        # the scale comes from the reference's points
    tA, tc = dev(A, np.float64), dev(centre, np.float64)
    color_fn = lambda p: (0.5 + (p.double() - tc) @ tA).float()
    image, uv = mesh_util.bake_texture(gv, gf, color_fn, patch=P)
    assert image.dtype == torch.uint8 and tuple(image.shape) == r_face.shape + (3,) and np.array_equal(uv, ref.uvs(len(f), P))
    img = image.cpu().numpy()
    assert np.all(img[r_face < 0] == 0) and img[r_face >= 0].min() >= 25 and img[r_face >= 0].max() <= 230
    tex = img.astype(np.float64) / 255.0
    faces = range(len(f)) if len(f) <= 64 else rng.choice(len(f), size=64, replace=False)
    worst = 0.0
    for k in faces:
        for lam in ref.surface_samples(rng):
            X, Y = lam @ uv[k]
            value, read = ref.bilinear(tex, X, Y)
            assert all(r_face[y, x] == k for x, y, _ in read)
            want = 0.5 + ((lam @ v[f[k]].astype(np.float64)) - centre) @ A
            worst = max(worst, float(np.abs(value - want).max()))
    print(f"[texture] bake {name}, P = {P}: worst |sample - function| = {worst * 255:.4f} levels (allowed 0.5 + 0.00255)")
    assert worst <= 0.5 / 255 + 1e-5


# ---- extract_mesh end to end -----------------------------------------------------------------------------------------------------------------

N, VOLUME_SIZE, FACTOR, PATCH, PROJECT = 48, 3.0, 2, 2, 2


@pytest.fixture(scope="module", params=["VolSDF", "NeuS"])
def model(request):
    from nerfart_amd import scene
    return scene.build_model(request.param, seed=0, beta=0.01 if request.param == "VolSDF" else None, device=DEV, precision="mixed")[0]


def test_extract_mesh_writes_the_textured_mesh(model, tmp_path):
    from nerfart_amd import hip, mesh_util
    surface = model.implicit_surface
    kw = dict(volume_size=VOLUME_SIZE, N=N, simplify_factor=FACTOR, vertex_normals=True)
    path = mesh_util.extract_mesh(surface, filepath=str(tmp_path / "mesh.obj"), texture_model=model, texture_patch=PATCH, texture_project=PROJECT, **kw)
    assert path == str(tmp_path / "mesh.obj") and all(os.path.exists(str(tmp_path / ("mesh" + e))) for e in (".obj", ".mtl", ".png"))
    obj, mtl, png = ref.read_obj(path), ref.read_mtl(str(tmp_path / "mesh.mtl")), ref.read_png(str(tmp_path / "mesh.png"))
    pts, placed, faces = decimated(surface, N, VOLUME_SIZE, FACTOR)              # extract_mesh(simplify_factor=FACTOR) by hand
    V, F = pts.shape[0], faces.shape[0]
    S, Cw, Ch, W, H = ref.layout(F, PATCH)
    assert F > 100 and png.shape == (H, W, 3) and mtl["map_Kd"] == "mesh.png" and obj["mtllib"] == "mesh.mtl"
    assert obj["v"].shape == (V, 3) and obj["vn"].shape == (V, 3) and obj["vt"].shape == (3 * F, 2) and obj["f"].shape == (F, 3, 3)
    assert obj["vt"].min() >= 0.0 and obj["vt"].max() <= 1.0
    assert np.array_equal(obj["v"].astype(np.float32), placed.cpu().numpy()) and np.array_equal(obj["f"][..., 0], faces.cpu().numpy() + 1)
    assert np.array_equal(obj["f"][..., 2], obj["f"][..., 0]) and np.array_equal(obj["f"][..., 1], np.arange(3 * F).reshape(F, 3) + 1)
    assert np.all(np.abs(np.linalg.norm(obj["vn"], axis=1) - 1) < 1e-5)
    ref.check_obj_corners(obj, png, PATCH)
    # the texels: the per-vertex colour rule at texel_points(...) with the same arguments
    max_step = FACTOR * VOLUME_SIZE / N
    points, face_of = mesh_util.texel_points(pts, faces, PATCH, query_fn=surface.forward_with_nablas, project=PROJECT, level=0.0, max_step=max_step)
    assert np.array_equal(face_of.cpu().numpy(), ref.texel_table(F, PATCH)[0])
    valid = (face_of.reshape(-1) >= 0).cpu().numpy()
    assert valid.sum() <= mesh_util.TEXEL_CHUNK
    at = points[torch.from_numpy(valid).to(DEV)]
    colours = mesh_util.vertex_attributes(model, at)[1].cpu().numpy()
    flat = png.reshape(-1, 3)
    assert np.array_equal(flat[valid], colours) and np.all(flat[~valid] == 0)
    assert len(np.unique(flat[valid], axis=0)) > 16, "the texture is meant to vary"
    # projection: the texels of the decimated faces end closer to the level set
    flat_points, _ = mesh_util.texel_points(pts, faces, PATCH)
    before = float(surface.forward(flat_points[torch.from_numpy(valid).to(DEV)]).abs().double().mean())
    after = float(surface.forward(at).abs().double().mean())
    moved = (at - flat_points[torch.from_numpy(valid).to(DEV)]).norm(dim=1)
    print(f"[texture] {type(model).__name__}: V = {V}, F = {F}, {W} x {H} texels, {int(valid.sum())} valid; mean |sdf| over valid texels {before:.4e} "
          f"without projection, {after:.4e} after {PROJECT} steps; largest move {float(moved.max()):.4f} (max_step {max_step:.4f} a step)")
    assert after < before
    assert float(moved.max()) <= PROJECT * max_step * (1 + 1e-5)


def test_extract_mesh_without_a_texture_writes_what_it_wrote(model, tmp_path):
    from nerfart_amd import mesh_util
    surface = model.implicit_surface
    for n, kw in enumerate((dict(), dict(simplify_factor=FACTOR, vertex_normals=True, color_model=model))):
        a = mesh_util.extract_mesh(surface, volume_size=VOLUME_SIZE, N=N, filepath=str(tmp_path / f"a{n}.ply"), **kw)
        b = mesh_util.extract_mesh(surface, volume_size=VOLUME_SIZE, N=N, filepath=str(tmp_path / f"b{n}.ply"), texture_model=None, texture_patch=PATCH,
                                   texture_project=PROJECT, **kw)
        assert open(a, "rb").read() == open(b, "rb").read()
        assert sorted(os.listdir(tmp_path)) == sorted(f"{c}{m}.ply" for c in "ab" for m in range(n + 1))


def test_extract_mesh_refusals(model, tmp_path):
    from nerfart_amd import mesh_util
    kw = dict(volume_size=VOLUME_SIZE, N=N, texture_model=model)
    with pytest.raises(ValueError, match=".obj"):
        mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "a.ply"), **kw)
    with pytest.raises(ValueError, match="color_model"):
        mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "a.obj"), color_model=model, **kw)
    with pytest.raises(ValueError, match="texture_model needs the regular grid"):
        mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "a.obj"), reference_shear=True, **kw)
    with pytest.raises(ValueError, match="texture_model needs backend='native'"):
        mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "a.obj"), backend="skimage", **kw)
    assert os.listdir(tmp_path) == []


def test_extract_mesh_textures_the_undecimated_mesh_too(model, tmp_path):
    """No simplify_factor, floaters filtered, refined vertices: the other branch of extract_mesh reaches the bake with the vertices it wrote."""
    from nerfart_amd import mesh_util
    path = mesh_util.extract_mesh(model.implicit_surface, volume_size=VOLUME_SIZE, N=24, filepath=str(tmp_path / "m.obj"), texture_model=model,
                                  texture_patch=1, keep_largest=1, refine_evals=2)
    obj, png = ref.read_obj(path), ref.read_png(str(tmp_path / "m.png"))
    F = len(obj["f"])
    assert F > 50 and obj["vn"] is None and obj["f"].shape == (F, 3, 2) and png.shape[:2] == ref.layout(F, 1)[:2:-1]
    ref.check_obj_corners(obj, png, 1)
    # the texels of face k's corners are the colour rule at its vertices (a = b = 0, (P, 0), (0, P): weights 1 0 0, 0 1 0, 0 0 1 - exact), in the
    # model's frame: placement and model frame share the origin, p_model = o + (p - o) N / (N - 1)
    o = -VOLUME_SIZE / 2.0
    pts = torch.from_numpy((o + (obj["v"] - o) * (24 / 23.0)).astype(np.float32)).to(DEV)
    colours = mesh_util.vertex_attributes(model, pts)[1].cpu().numpy().astype(np.int64)
    face_of, a, b = ref.texel_table(F, 1)
    ys, xs = np.nonzero((face_of >= 0) & (a == 0) & (b == 0))
    corner = colours[obj["f"][face_of[ys, xs], 0, 0] - 1]
    # the frame conversion above errs by a few fp32 ulp, which moves a colour by far less than a level: at most one quantisation flip
    assert np.abs(png[ys, xs].astype(np.int64) - corner).max() <= 1, "a corner texel is not its vertex's colour"
