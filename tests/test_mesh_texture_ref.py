"""tests/mesh_texture_ref.py - the float64 statement of the per-face texture atlas - held to the two properties the atlas is built on, to the
counts of its texel table, and shown to catch four injected bugs; mesh_util's closed forms (atlas_layout, atlas_uvs) and write_obj are held to it.
Nothing here needs a GPU."""
import importlib.util
import os

import numpy as np
import pytest
import yaml

import mesh_texture_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCHES = list(range(1, 9))
FACE_COUNTS = [1, 2, 3, 7, 50, 51]


def random_mesh(F, seed):
    """F triangles over F + 2 random fp32 vertices (a strip: consecutive faces share an edge)."""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-1.0, 1.0, size=(F + 2, 3)).astype(np.float32)
    faces = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(F)], dtype=np.int32)
    return verts, faces


@pytest.mark.parametrize("P", PATCHES)
def test_bilinear_reads_only_the_face_and_reproduces_affine_functions(P):
    for F in FACE_COUNTS:
        verts, faces = random_mesh(F, seed=100 * P + F)
        n = ref.check_atlas(verts, faces, P, np.random.default_rng(P * 1000 + F), tol=1e-9)
        assert n == F * 18


@pytest.mark.parametrize("P", PATCHES)
def test_every_face_owns_exactly_its_texels(P):
    S = P + 3
    for F in FACE_COUNTS:
        S_, Cw, Ch, W, H = ref.layout(F, P)
        cells = (F + 1) // 2
        assert S_ == S and Cw * Cw >= cells and (Cw - 1) ** 2 < cells and Ch == -(-cells // Cw) and (W, H) == (Cw * S, Ch * S)
        face_of, a, b = ref.texel_table(F, P)
        assert face_of.shape == (H, W)
        count = np.bincount(face_of[face_of >= 0], minlength=F)
        assert np.all(count[0::2] == S * (S + 1) // 2) and np.all(count[1::2] == S * (S - 1) // 2)
        assert int((face_of < 0).sum()) == W * H - count.sum()
        if F % 2:                                                  # the upper half of the last cell is nobody's
            q = cells - 1
            cell = face_of[(q // Cw) * S:(q // Cw + 1) * S, (q % Cw) * S:(q % Cw + 1) * S]
            assert int((cell == F - 1).sum()) == S * (S + 1) // 2 and int((cell == -1).sum()) == S * (S - 1) // 2
        for f in range(F):                                         # every face holds each (a, b) of its range exactly once
            mine = face_of == f
            top = P + 2 if f % 2 == 0 else P + 1
            got = sorted(zip(a[mine].tolist(), b[mine].tolist()))
            assert got == sorted((i, j) for i in range(S) for j in range(S) if i + j <= top)
            ys, xs = np.nonzero(mine)
            assert xs.min() // S == xs.max() // S == (f // 2) % Cw and ys.min() // S == ys.max() // S == (f // 2) // Cw


def test_weights_span_the_documented_gutter():
    verts, faces = random_mesh(2, seed=3)
    for P in (1, 4):
        face_of, a, b = ref.texel_table(2, P)
        w1, w2 = a / P, b / P
        w0 = 1 - w1 - w2
        assert min(w0.min(), w1.min(), w2.min()) == -2.0 / P and max(w0.max(), w1.max(), w2.max()) == (P + 2.0) / P


@pytest.mark.parametrize("bug", ref.BUGS)
def test_the_checks_catch_an_injected_bug(bug):
    caught = 0
    for P in (1, 2, 4, 7):
        for F in (2, 7):
            verts, faces = random_mesh(F, seed=7 * P + F)
            ref.check_atlas(verts, faces, P, np.random.default_rng(5), tol=1e-9)              # the rules as stated pass
            with pytest.raises(AssertionError):
                ref.check_atlas(verts, faces, P, np.random.default_rng(5), bug=bug, tol=1e-9)
            caught += 1
    assert caught == 8


def test_mesh_util_closed_forms_are_the_reference():
    from nerfart_amd import mesh_util
    for P in PATCHES:
        for F in FACE_COUNTS + [79980, 296222]:
            assert mesh_util.atlas_layout(F, P) == ref.layout(F, P)
            if F <= 51:
                uv = mesh_util.atlas_uvs(F, P)
                assert uv.dtype == np.float64 and uv.shape == (F, 3, 2) and np.array_equal(uv, ref.uvs(F, P))
    for F, P in ((1, 0), (1, -1), (0, 1)):
        with pytest.raises(ValueError):
            mesh_util.atlas_layout(F, P)
    with pytest.raises(ValueError, match="F = 10000000.*P = 8.*simplify_factor"):
        mesh_util.atlas_layout(10_000_000, 8)
    assert mesh_util.atlas_layout(2 * 2340 * 2340, 4)[3:] == (16380, 16380)                 # the largest square of cells of side 7 that fits


def test_project_step_reference_is_the_clamped_newton_step():
    rng = np.random.default_rng(0)
    p, g = rng.normal(size=(64, 3)).astype(np.float32), rng.normal(size=(64, 3)).astype(np.float32)
    s = rng.normal(size=64).astype(np.float32)
    out, moved, bound = ref.project_step(p, s, g, 0.25, 0.3)
    assert moved.all()
    d = out - p
    gn = np.linalg.norm(g.astype(np.float64), axis=1)
    full = np.abs(s.astype(np.float64) - 0.25) / gn
    assert np.allclose(np.linalg.norm(d, axis=1), np.minimum(full, 0.3), rtol=1e-12)
    assert (full > 0.3).any() and (full < 0.3).any()
    unit = g / gn[:, None]
    assert np.allclose(d, -np.sign(s - 0.25)[:, None] * np.minimum(full, 0.3)[:, None] * unit, rtol=1e-12, atol=1e-15)
    s[0], g[1], g[2, 1] = np.nan, 0.0, np.inf
    out, moved, _ = ref.project_step(p, s, g, 0.25, 0.3)
    assert not moved[:3].any() and moved[3:].all() and np.array_equal(out[:3], p[:3].astype(np.float64))


# ---- write_obj -------------------------------------------------------------------------------------------------------------------------------

def written(tmp_path, F, P, normals, name="mesh"):
    from nerfart_amd import mesh_util
    verts, faces = random_mesh(F, seed=F + P)
    _, _, _, W, H = ref.layout(F, P)
    image = np.random.default_rng(F * 10 + P).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    n = np.random.default_rng(1).normal(size=verts.shape).astype(np.float32) if normals else None
    path = mesh_util.write_obj(str(tmp_path / f"{name}.obj"), verts, faces, mesh_util.atlas_uvs(F, P), image, normals=n)
    return path, verts, faces, image, n


@pytest.mark.parametrize("F,P,normals", [(1, 1, False), (7, 2, True), (51, 4, False), (50, 7, True)])
def test_write_obj_round_trip(tmp_path, F, P, normals):
    path, verts, faces, image, n = written(tmp_path, F, P, normals)
    stem = path[:-4]
    assert path.endswith("mesh.obj") and all(os.path.exists(stem + e) for e in (".obj", ".mtl", ".png"))
    obj, mtl, png = ref.read_obj(path), ref.read_mtl(stem + ".mtl"), ref.read_png(stem + ".png")
    assert obj["mtllib"] == "mesh.mtl" and obj["usemtl"] == mtl["newmtl"] == "mesh" and mtl["map_Kd"] == "mesh.png"
    assert png.dtype == np.uint8 and np.array_equal(png, image)
    assert np.array_equal(obj["v"].astype(np.float32), verts), "%.9g gives every fp32 back"
    assert obj["vt"].shape == (3 * F, 2) and obj["f"].shape == (F, 3, 3 if normals else 2)
    assert np.array_equal(obj["f"][..., 0], faces + 1) and np.array_equal(obj["f"][..., 1], np.arange(3 * F).reshape(F, 3) + 1)
    if normals:
        assert np.array_equal(obj["vn"].astype(np.float32), n) and np.array_equal(obj["f"][..., 2], faces + 1)
    else:
        assert obj["vn"] is None
    H, W = image.shape[:2]
    assert np.allclose(ref.vt_to_pixels(obj["vt"], W, H).reshape(F, 3, 2), ref.uvs(F, P), rtol=0, atol=1e-6)
    ref.check_obj_corners(obj, png, P)


def test_an_unflipped_v_is_caught(tmp_path):
    path, verts, faces, image, _ = written(tmp_path, 7, 2, False)
    obj, png = ref.read_obj(path), ref.read_png(path[:-4] + ".png")
    ref.check_obj_corners(obj, png, 2)
    wrong = dict(obj, vt=np.stack([obj["vt"][:, 0], 1.0 - obj["vt"][:, 1]], axis=-1))       # v = Y / H: what a writer without the flip leaves
    with pytest.raises(AssertionError):
        ref.check_obj_corners(wrong, png, 2)


def test_write_obj_refusals(tmp_path):
    from nerfart_amd import mesh_util
    verts, faces = random_mesh(3, seed=0)
    uv, image = mesh_util.atlas_uvs(3, 2), np.zeros((5, 10, 3), np.uint8)
    with pytest.raises(ValueError, match=".obj"):
        mesh_util.write_obj(str(tmp_path / "a.ply"), verts, faces, uv, image)
    with pytest.raises(ValueError, match="uint8"):
        mesh_util.write_obj(str(tmp_path / "a.obj"), verts, faces, uv, image.astype(np.float32))
    with pytest.raises(ValueError, match="uv"):
        mesh_util.write_obj(str(tmp_path / "a.obj"), verts, faces, uv[:2], image)
    with pytest.raises(ValueError, match="normals"):
        mesh_util.write_obj(str(tmp_path / "a.obj"), verts, faces, uv, image, normals=verts[:2])


def test_extract_mesh_refuses_before_it_touches_the_model():
    from nerfart_amd import mesh_util
    model = object()
    with pytest.raises(ValueError, match=".obj"):
        mesh_util.extract_mesh(None, filepath="a.ply", texture_model=model)
    with pytest.raises(ValueError, match="color_model"):
        mesh_util.extract_mesh(None, filepath="a.obj", texture_model=model, color_model=model)
    with pytest.raises(ValueError, match="texture_model needs the regular grid"):
        mesh_util.extract_mesh(None, filepath="a.obj", texture_model=model, reference_shear=True)
    with pytest.raises(ValueError, match="texture_model needs backend='native'"):
        mesh_util.extract_mesh(None, filepath="a.obj", texture_model=model, backend="skimage")
    with pytest.raises(ValueError, match="texture_patch"):
        mesh_util.extract_mesh(None, filepath="a.obj", texture_model=model, texture_patch=0)
    with pytest.raises(ValueError, match="texture_project"):
        mesh_util.extract_mesh(None, filepath="a.obj", texture_model=model, texture_project=-1)


def test_the_tool_takes_the_three_flags(tmp_path):
    from nerfart_amd import scene
    spec = importlib.util.spec_from_file_location("extract_surface", os.path.join(REPO, "tools", "extract_surface.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    d = scene.synthetic_config("NeuS").to_dict()
    d["expname"] = "mesh"
    d.setdefault("training", {})["log_root_dir"] = str(tmp_path)
    path = tmp_path / "neus.yaml"
    path.write_text(yaml.dump(d))
    args, _ = tool.parse(["--config", str(path), "--texture", "--texture_patch", "6", "--texture_project", "2", "--out", "a.obj"])
    assert (args.texture, args.texture_patch, args.texture_project) == (True, 6, 2)
    args, _ = tool.parse(["--config", str(path)])
    assert (args.texture, args.texture_patch, args.texture_project) == (False, 4, 0)
