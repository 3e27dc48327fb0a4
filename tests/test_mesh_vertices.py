"""The mesh-vertex additions up to the GPU: the entry points' argument checks (nothing is launched), the refinement rule of
tests/mesh_vertices_ref.py on analytic fields, write_ply's optional vertex properties, the tool's new flags and extract_mesh's refusals."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import yaml

import mesh_vertices_ref as mv
from conftest import REPO


def test_bad_arguments_are_refused_before_any_launch():
    from nerfart_amd import hip
    lib, null, one = hip.lib, C.c_void_p(0), C.c_void_p(256)       # `one`: non-null, aligned, never dereferenced - the checks come first

    def err():
        return lib.nerfart_last_error().decode()

    need = lib.nerfart_mc_workspace_bytes(8, 8, 8)
    names = ("vol", "nx", "ny", "nz", "level", "ws", "ws_bytes", "edge", "bracket", "t", "best", "side", "V", "stream")
    default = dict(zip(names, (one, 8, 8, 8, 0.0, one, need, one, one, one, one, one, 3, null)))
    edges = lambda **kw: lib.nerfart_mc_emit_edges(*[kw.get(k, default[k]) for k in names])
    for k in ("vol", "ws", "edge", "bracket", "t", "best", "side"):
        assert edges(**{k: null}) == 2 and "null" in err(), k
    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (-4, 8, 8)):
        assert edges(nx=dims[0], ny=dims[1], nz=dims[2], ws_bytes=1 << 30) == 2 and ">= 2" in err()
    assert edges(nx=1024, ny=1024, nz=1024, ws_bytes=1 << 40) == 2 and "2^31" in err()
    assert edges(nx=178956970, ny=2, nz=2, ws_bytes=1 << 40) == 2 and "2^24" in err()
    assert edges(ws_bytes=need - 1) == 2 and "workspace" in err()
    assert edges(ws=C.c_void_p(260)) == 2 and "aligned" in err()
    # an empty mesh launches nothing and succeeds, whatever the buffers
    assert edges(V=0, vol=null, ws=null, edge=null, bracket=null, t=null, best=null, side=null) == 0
    assert lib.nerfart_mesh_edge_points(null, null, 0, 8, 8, 8, null, null, null, null) == 0
    assert lib.nerfart_mesh_edge_refine_step(null, 0.0, 0, null, null, null, null, null) == 0
    for k in range(5):
        args = [one] * 5
        args[k] = null
        assert lib.nerfart_mesh_edge_points(args[0], args[1], 3, 8, 8, 8, args[2], args[3], args[4], null) == 2 and "null" in err()
        assert lib.nerfart_mesh_edge_refine_step(args[0], 0.0, 3, args[1], args[2], args[3], args[4], null) == 2 and "null" in err()
    assert lib.nerfart_mesh_edge_points(one, one, 3, 1, 8, 8, one, one, one, null) == 2 and ">= 2" in err()
    assert lib.nerfart_mesh_edge_points(one, one, 3, 1024, 1024, 1024, one, one, one, null) == 2 and "2^31" in err()


def test_python_front_refuses_cpu_tensors():
    import torch
    from nerfart_amd import hip
    V = 4
    edge, t, f = torch.zeros(V, dtype=torch.int32), torch.zeros(V), torch.zeros(V)
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        hip.mc_emit_edges(torch.ones(4, 4, 4), 0.0, torch.zeros(1 << 16, dtype=torch.uint8), V)
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        hip.mesh_edge_points(edge, t, (4, 4, 4), [0.0] * 3, [1.0] * 3)
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        hip.mesh_edge_refine_step(f, 0.0, torch.zeros(V, 4), t, torch.zeros(V, 2), torch.zeros(V, dtype=torch.uint8))


def test_edge_records_and_points_restate_marching_cubes_vertices():
    """The numpy statement against tests/mc_ref.py: same vertex count and order, and the initial t on the recorded edges gives mc_ref's
    vertices (float64 there) to the fp32 bound tests/test_gpu_marching_cubes.py uses."""
    import mc_ref
    vol = mc_ref.noise_volume((5, 7, 9), seed=1, pad=False)
    spacing, origin = [0.5, 0.25, 0.1], [3.0, -2.0, 0.7]
    edge, bracket, t, best, side = mv.edge_records(vol, 0.0)
    rv, _ = mc_ref.marching_cubes(vol, 0.0, spacing, origin)
    assert len(edge) == len(rv) > 50 and (np.diff(edge.astype(np.int64)) > 0).all()
    assert ((t >= 0) & (t <= 1)).all() and np.array_equal(best[:, 0], t) and np.isinf(best[:, 1]).all() and not side.any()
    assert ((bracket[:, 1] < 0) != (bracket[:, 3] < 0)).all()
    pts = mv.edge_points(edge, t, vol.shape, origin, spacing)
    sp = np.asarray(spacing, np.float32).astype(np.float64)
    assert (np.abs(pts.astype(np.float64) - rv) <= 2.0 ** -22 * (np.abs(rv) + sp)).all()


@pytest.mark.parametrize("name", list(mv.FIELDS))
def test_refinement_rule_on_analytic_fields(name):
    """t_best stays on the edge, |g_best| never grows, and 5 evaluations take max |g_best| to at most 1 / 100 of the interpolated vertices'
    (measured with this mirror: sphere 7.6e-4 -> 1.8e-9, torus 9.9e-4 -> 2.1e-6, bumpy sphere 2.5e-3 -> 1.3e-7)."""
    vol, origin, spacing = mv.field_volume(name)
    t_best, hist = mv.refine_loop(vol, 0.0, origin, spacing, mv.FIELDS[name][0], 5)
    mv.check_refinement(name, t_best, hist)


def test_refine_step_special_values():
    """The rule's branches on hand-made states: NaN changes nothing but can never win, g == 0 collapses the bracket, the Illinois halving needs
    the same end to move twice, g1 == g0 and infinities fall back to the midpoint, and t stays inside the bracket."""
    f32 = np.float32
    bracket = np.array([[0, -1, 1, 1]] * 6 + [[0.25, 2, 0.75, 2]], f32)
    t = np.array([0.5] * 6 + [0.5], f32)
    best = np.array([[0.5, 0.25]] * 7, f32)
    side = np.array([0, 1, 2, 0, 0, 0, 0], np.uint8)
    f = np.array([-0.5, -0.5, -0.5, np.nan, 0.0, np.inf, 2.0], f32)
    br, tn, bs, sd = mv.refine_step(f, 0.0, bracket, t, best, side)
    assert br[0].tolist() == [0.5, -0.5, 1, 1] and sd[0] == 1 and tn[0] == f32(0.5) - f32(-0.5) * f32(0.5) / f32(1.5)
    assert br[1].tolist() == [0.5, -0.5, 1, 0.5] and sd[1] == 1                   # the same end again: the other end's value is halved
    assert br[2].tolist() == [0.5, -0.5, 1, 1] and sd[2] == 1                     # the other end moved last: no halving
    assert np.array_equal(br[3], bracket[3]) and tn[3] == t[3] and sd[3] == 0 and bs[3].tolist() == [0.5, 0.25]
    assert br[4].tolist() == [0.5, 0, 0.5, 0] and tn[4] == 0.5 and bs[4].tolist() == [0.5, 0.0]
    assert br[5].tolist() == [0, -1, 0.5, np.inf] and sd[5] == 2 and tn[5] == 0 and bs[5].tolist() == [0.5, 0.25]       # inf never wins; q = 0.5 / inf
    assert br[6].tolist() == [0.5, 2, 0.75, 2] and tn[6] == 0.625                # g1 == g0: the midpoint
    assert bs[0].tolist() == [0.5, 0.25] and bs[6].tolist() == [0.5, 0.25]       # |g| >= |g_best|: best stays


def test_write_ply_optional_properties_round_trip(tmp_path):
    from nerfart_amd import mesh_util
    rng = np.random.default_rng(0)
    verts = rng.normal(size=(7, 3)).astype(np.float32)
    faces = rng.integers(0, 7, size=(5, 3)).astype(np.int32)
    normals = rng.normal(size=(7, 3)).astype(np.float32)
    colors = rng.integers(0, 256, size=(7, 3)).astype(np.uint8)
    for n, c in ((normals, colors), (normals, None), (None, colors)):
        path = mesh_util.write_ply(str(tmp_path / "m.ply"), verts, faces, normals=n, colors=c)
        got = mv.read_ply(path)
        assert np.array_equal(got["verts"], verts) and np.array_equal(got["faces"], faces)
        assert (got["normals"] is None) if n is None else np.array_equal(got["normals"], n)
        assert (got["colors"] is None) if c is None else np.array_equal(got["colors"], c)
        want = ["property float x", "property float y", "property float z"]
        want += ["property float nx", "property float ny", "property float nz"] if n is not None else []
        want += ["property uchar red", "property uchar green", "property uchar blue"] if c is not None else []
        assert [l for l in got["header"].split("\n") if l.startswith("property ") and "list" not in l] == want
    import torch
    a = mesh_util.write_ply(str(tmp_path / "a.ply"), verts, faces, normals, colors)
    b = mesh_util.write_ply(str(tmp_path / "b.ply"), torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(normals), torch.from_numpy(colors))
    assert open(a, "rb").read() == open(b, "rb").read()                           # tensors or arrays: the same file
    assert os.path.getsize(a) == len(mv.read_ply(a)["header"]) + 7 * (12 + 12 + 3) + 5 * 13      # packed records, no padding
    with pytest.raises(ValueError):
        mesh_util.write_ply(str(tmp_path / "bad.ply"), verts, faces, colors=colors.astype(np.float32))
    with pytest.raises(ValueError):
        mesh_util.write_ply(str(tmp_path / "bad.ply"), verts, faces, normals=normals[:3])


def test_write_ply_without_the_options_is_the_two_element_file(tmp_path):
    """Bytes assembled here from the documented layout: the header of the reference's two elements, V x 3 little-endian floats, F records of
    one count byte 3 and three little-endian int32."""
    from nerfart_amd import mesh_util
    import mc_ref
    rng = np.random.default_rng(1)
    verts = rng.normal(size=(9, 3)).astype(np.float32)
    faces = rng.integers(0, 9, size=(4, 3)).astype(np.int32)
    want = (b"ply\nformat binary_little_endian 1.0\nelement vertex 9\nproperty float x\nproperty float y\nproperty float z\n"
            b"element face 4\nproperty list uchar int vertex_indices\nend_header\n")
    want += verts.astype("<f4").tobytes()
    for tri in faces:
        want += b"\x03" + tri.astype("<i4").tobytes()
    for kw in ({}, dict(normals=None, colors=None)):
        path = mesh_util.write_ply(str(tmp_path / "m.ply"), verts, faces, **kw)
        assert open(path, "rb").read() == want
    _, v, f, n = mc_ref.read_ply(path)
    assert np.array_equal(v, verts) and np.array_equal(f, faces) and n == 9 * 12 + 4 * 13


def test_quantize_colors():
    import torch
    from nerfart_amd import mesh_util
    rgb = torch.tensor([[0.0, 1.0, 0.5], [-0.3, 1.7, float("nan")], [0.5 / 255, 0.49 / 255, 254.5 / 255], [float("inf"), -float("inf"), 0.25]])
    want = torch.tensor([[0, 255, 128], [0, 255, 0], [1, 0, 255], [255, 0, 64]], dtype=torch.uint8)
    assert torch.equal(mesh_util.quantize_colors(rgb), want)


def test_tool_flags_parse(tmp_path):
    from nerfart_amd import scene
    spec = importlib.util.spec_from_file_location("extract_surface", os.path.join(REPO, "tools", "extract_surface.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    d = scene.synthetic_config("VolSDF").to_dict()
    d["expname"] = "mesh"
    d.setdefault("training", {})["log_root_dir"] = str(tmp_path)
    path = tmp_path / "volsdf.yaml"
    path.write_text(yaml.dump(d))
    args, _ = tool.parse(["--config", str(path)])
    assert (args.refine, args.normals, args.colors) == (0, False, False)
    args, conf = tool.parse(["--config", str(path), "--N", "64", "--refine", "5", "--normals", "--colors"])
    assert (args.N, args.refine, args.normals, args.colors) == (64, 5, True, True) and conf.model.framework == "VolSDF"


def test_extract_mesh_refuses_the_new_options_without_a_regular_native_grid():
    from nerfart_amd import mesh_util
    for new in (dict(refine_evals=5), dict(vertex_normals=True), dict(color_model=object())):
        with pytest.raises(ValueError, match="regular grid"):
            mesh_util.extract_mesh(None, N=8, reference_shear=True, **new)
        with pytest.raises(ValueError, match="regular grid"):
            mesh_util.extract_mesh(None, N=8, backend="skimage", **new)
