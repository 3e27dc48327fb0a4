"""csrc/mesh_repair.hip (mesh_util.repair_manifold, extract_mesh(repair=)) against the numpy statement tests/mesh_repair_ref.py, which
tests/test_mesh_repair_ref.py holds to its own properties.  Every output - verts' as bits, faces', src_vertex, mid_ends, info - is compared by
np.array_equal, for both wedges, on every mesh of that file (hand meshes, the two clustered fixtures, the tetrahedron soups on float and on
lattice positions), on the faces the GPU's own marching cubes + simplify_clusters produce for the fixtures and on a strip of 20,000 triangles;
the same bits for the default edge table and the smallest legal one; sentinel words around every output; two runs; the guarantee through the
GPU's mesh_topology; extract_mesh(repair=) end to end."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mc_ref
import mesh_components_ref as cref
import mesh_repair_ref as ref
import mesh_simplify_ref as sref
import mesh_vertices_ref as mv
from conftest import REPO
from test_mesh_repair_ref import GENERATED, all_meshes, hand_meshes, repaired

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
PAD = 32                   # sentinel words on either side of every output array
KEYS = ("verts", "faces", "src_vertex", "mid_ends")


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)               # a copy: the shared reference arrays are read-only


def gpu_repair(verts, faces, wedge, table_log2=0):
    """mesh_util.repair_manifold as numpy: dict like ref.repair's"""
    from nerfart_amd import mesh_util
    v, f, src, ends, report = mesh_util.repair_manifold(dev(verts, np.float32).reshape(-1, 3), dev(faces, np.int32).reshape(-1, 3), wedge, table_log2)
    assert v.dtype == torch.float32 and f.dtype == src.dtype == ends.dtype == torch.int32
    assert v.shape[0] == src.shape[0] and v.shape[1:] == (3,) and f.shape[1:] == (3,) and ends.shape[1:] == (2,)
    info = np.zeros(16, dtype=np.uint32)
    info[:11] = [report[k] for k in ref.INFO]
    return {"verts": v.cpu().numpy(), "faces": f.cpu().numpy(), "src_vertex": src.cpu().numpy(), "mid_ends": ends.cpu().numpy(), "info": info}


def assert_same(got, want, what=""):
    assert np.array_equal(got["info"], want["info"]), (what, ref.info_dict(got["info"]), ref.info_dict(want["info"]))
    assert got["info"][10] == 0                                             # the overflow flag
    for k in KEYS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)


def least_log2(F):
    return max(1, int(np.ceil(np.log2(3 * F + 1))))


@pytest.mark.parametrize("wedge", ref.WEDGES)
@pytest.mark.parametrize("name", list(all_meshes()))
def test_outputs_are_the_reference_for_every_table(name, wedge):
    verts, faces = all_meshes()[name]()
    want = repaired(name, wedge)
    assert_same(gpu_repair(verts, faces, wedge), want, "default table")
    assert_same(gpu_repair(verts, faces, wedge, least_log2(len(faces))), want, "smallest table")


@pytest.mark.parametrize("name", GENERATED)
def test_the_gpu_topology_of_the_output_shows_the_guarantee(name):
    from nerfart_amd import mesh_util
    verts, faces = all_meshes()[name]()
    for wedge in ref.WEDGES:
        v, f, src, ends, report = mesh_util.repair_manifold(dev(verts), dev(faces), wedge)
        t = mesh_util.mesh_topology(v, f, components=False)
        assert report["wide_edges"] == 0 and report["overflow"] == 0
        assert t["nonmanifold_edges"] == 0 and t["bowtie_vertices"] == 0 and t["degenerate_faces"] == 0 and t["bad_faces"] == 0 and t["manifold"]
        assert t["referenced_vertices"] == v.shape[0]
        if name == "shells24c4" or name.startswith("soup"):                 # balanced, closed, oriented inputs
            assert report["unpaired_half_edges"] == 0 and t["watertight"]
        again = mesh_util.repair_manifold(v, f, wedge)                      # idempotence on the GPU
        assert torch.equal(again[0].view(torch.int32), v.view(torch.int32)) and torch.equal(again[1], f) and not any(again[4].values())
        assert torch.equal(again[2], torch.arange(v.shape[0], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("fixture", ["shells24c4", "noise12c2"])
def test_the_faces_the_gpu_pipeline_produces_for_the_fixtures(fixture):
    """mesh_util.marching_cubes + simplify_clusters instead of their numpy statements: the positions may differ in the last bits, so the reference
    runs on what the GPU produced."""
    from nerfart_amd import mesh_util
    vol, c = ((sref.shells_volume((24, 24, 24), (11.4, 11.6, 11.3), 3.3, 6.4, 9.6), 4) if fixture == "shells24c4"
              else (mc_ref.noise_volume((12, 12, 12)), 2))
    gv, gf = mesh_util.marching_cubes(dev(vol), 0.0)
    sv, sf, _ = mesh_util.simplify_clusters(gv, gf, vol.shape, c)
    verts, faces = sv.cpu().numpy(), sf.cpu().numpy()
    assert np.array_equal(faces, all_meshes()[fixture]()[1])                # the integers are the statement's
    for wedge in ref.WEDGES:
        want = ref.repair(verts, faces, wedge)
        assert want["info"][3] > 0
        assert_same(gpu_repair(verts, faces, wedge), want, wedge)


@pytest.mark.parametrize("order", ["permuted", "smallest_index_at_the_far_end"])
def test_long_chains_in_the_corner_union_find(order):
    """A strip of 20,000 triangles: every interior edge joins two corners, parent chains as long as the strip; nothing to repair, and the output
    must be the input with its vertices in ascending order (all referenced: the identity)."""
    n = 20000
    strip, V = cref.triangle_strip(n), n + 2
    strip[1::2] = strip[1::2][:, [0, 2, 1]]                                 # alternate, so that the strip is oriented
    if order == "permuted":
        rng = np.random.default_rng(7)
        faces = rng.permutation(V)[strip][rng.permutation(n)].astype(np.int32)
    else:
        faces = (V - 1 - strip).astype(np.int32)
    verts = np.random.default_rng(2).normal(size=(V, 3)).astype(np.float32)
    got = gpu_repair(verts, faces, "void")
    assert not got["info"].any() and np.array_equal(got["faces"], faces) and np.array_equal(got["src_vertex"], np.arange(V))
    assert np.array_equal(got["verts"].view(np.uint32), verts.view(np.uint32)) and got["mid_ends"].shape == (0, 2)
    assert_same(got, ref.repair(verts, faces, "void"))


def test_sizes_around_wave_and_block_boundaries():
    """random faces over few vertices: duplicate, flipped, non-manifold, degenerate, bad and cancelling faces at once, edges of dozens"""
    seen = np.zeros(16, dtype=np.int64)
    for V in (1, 2, 9, 65):
        for F in (1, 85, 256, 257, 600):
            rng = np.random.default_rng(7 * V + F)
            faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)
            faces[rng.random(F) < 0.05, 1] = V + 3
            faces[rng.random(F) < 0.05, 2] = -1
            verts = rng.normal(size=(V, 3)).astype(np.float32)
            for wedge in ref.WEDGES:
                want = ref.repair(verts, faces, wedge)
                assert_same(gpu_repair(verts, faces, wedge), want, (V, F, wedge))
                seen += want["info"]
    assert (np.delete(seen[:10], 6) > 0).all()                              # every count has been met but the wide edges (the hand mesh wide_book)


def test_two_runs_give_the_same_bits():
    verts, faces = all_meshes()["soup_40_6"]()
    a, b = gpu_repair(verts, faces, "void"), gpu_repair(verts, faces, "void")
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in KEYS + ("info",))


def test_sentinels_around_every_output_and_an_untouched_workspace_in_emit():
    from nerfart_amd import hip
    verts, faces = all_meshes()["noise12c2"]()
    faces = faces.copy()
    faces[100, 1], faces[300, 2], faces[7] = -1, len(verts), (5, 5, 9)
    want = ref.repair(verts, faces, "void")
    assert want["info"][:2].tolist() == [2, 1] and len(want["mid_ends"]) > 0
    V, F = len(verts), len(faces)
    Vo, Fo, M = len(want["verts"]), len(want["faces"]), len(want["mid_ends"])
    st = torch.cuda.current_stream().cuda_stream
    full = lambda n: torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    counts, info, out_v, out_f, src, ends = full(4), full(16), full(3 * Vo), full(3 * Fo), full(Vo), full(2 * M)
    ws = torch.zeros(hip.mesh_repair_workspace_bytes(V, F), dtype=torch.uint8, device=DEV)
    v, f = dev(verts), dev(faces)
    assert hip.lib.nerfart_mesh_repair_count(v.data_ptr(), f.data_ptr(), V, F, 0, 0, ws.data_ptr(), ws.numel(), counts[PAD:].data_ptr(),
                                             info[PAD:].data_ptr(), st) == 0
    assert counts[PAD:PAD + 4].tolist() == [Vo - M, M, int(want["alive"].sum()), Fo - int(want["alive"].sum())]
    before = ws.clone()
    assert hip.lib.nerfart_mesh_repair_emit(v.data_ptr(), f.data_ptr(), V, F, 0, ws.data_ptr(), ws.numel(), out_v[PAD:].data_ptr(), out_f[PAD:].data_ptr(),
                                            src[PAD:].data_ptr(), ends[PAD:].data_ptr(), Vo, M, Fo, st) == 0
    assert torch.equal(ws, before)                                          # emit runs from the untouched workspace
    for buf, w in ((info, want["info"]), (out_v, want["verts"]), (out_f, want["faces"]), (src, want["src_vertex"]), (ends, want["mid_ends"])):
        b, n = buf.cpu().numpy().view(np.uint32), w.size
        assert (b[:PAD] == SENTINEL).all() and (b[PAD + n:] == SENTINEL).all()
        assert np.array_equal(b[PAD:PAD + n], w.reshape(-1).view(np.uint32))
    # arrays one row short: every write is checked against the caller's sizes
    out_v, out_f, src, ends = full(3 * (Vo - 1)), full(3 * (Fo - 1)), full(Vo - 1), full(2 * (M - 1))
    assert hip.lib.nerfart_mesh_repair_emit(v.data_ptr(), f.data_ptr(), V, F, 0, ws.data_ptr(), ws.numel(), out_v[PAD:].data_ptr(), out_f[PAD:].data_ptr(),
                                            src[PAD:].data_ptr(), ends[PAD:].data_ptr(), Vo - 1, M - 1, Fo - 1, st) == 0
    for buf, n in ((out_v, 3 * (Vo - 1)), (out_f, 3 * (Fo - 1)), (src, Vo - 1), (ends, 2 * (M - 1))):
        b = buf.cpu().numpy().view(np.uint32)
        assert (b[:PAD] == SENTINEL).all() and (b[PAD + n:] == SENTINEL).all()


def test_refusals_leave_the_outputs_alone():
    from nerfart_amd import hip, mesh_util
    verts, faces = (dev(a) for a in hand_meshes()["tetrahedron"])
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((64,), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.zeros(hip.mesh_repair_workspace_bytes(4, 4), dtype=torch.uint8, device=DEV)
    o = out.data_ptr()
    err = lambda: hip.lib.nerfart_last_error().decode()
    count = lambda **kw: hip.lib.nerfart_mesh_repair_count(*[kw.get(k, d) for k, d in (("verts", verts.data_ptr()), ("faces", faces.data_ptr()), ("V", 4),
                                                                                       ("F", 4), ("wedge", 0), ("table_log2", 0), ("ws", ws.data_ptr()),
                                                                                       ("ws_bytes", ws.numel()), ("counts", o), ("info", o), ("stream", st))])
    assert count(table_log2=3) == 2 and "3 F + 1" in err() and count(wedge=2) == 2 and "wedge" in err()
    assert count(ws_bytes=ws.numel() - 1) == 2 and "workspace" in err() and count(ws=ws.data_ptr() + 4) == 2 and "aligned" in err()
    assert count(counts=o + 4) == 2 and "aligned" in err() and count(V=1 << 31) == 2 and "2^31" in err()
    for k in ("verts", "faces", "ws", "counts", "info"):
        assert count(**{k: None}) == 2 and "null" in err(), k
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all() and not ws.any()
    with pytest.raises(ValueError, match="float32"):
        mesh_util.repair_manifold(verts.double(), faces)
    with pytest.raises(ValueError, match="int32"):
        mesh_util.repair_manifold(verts, faces.long())
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        mesh_util.repair_manifold(verts, faces.reshape(-1))
    with pytest.raises(ValueError, match="wedge"):
        mesh_util.repair_manifold(verts, faces, wedge="inside")
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.repair_manifold(verts.cpu(), faces)


def test_the_tool_writes_the_repaired_mesh_and_prints_both_reports(tmp_path, capsys):
    from nerfart_amd import mesh_util
    spec = importlib.util.spec_from_file_location("check_mesh", os.path.join(REPO, "tools", "check_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    verts, faces = all_meshes()["shells24c4"]()
    ply, out = mesh_util.write_ply(str(tmp_path / "m.ply"), verts, faces), str(tmp_path / "fixed.ply")
    for wedge in ref.WEDGES:
        tool.main(["--mesh", ply, "--repair", out, "--repair_wedge", wedge, "--components", "3"])
        first, second = (json.loads(line) for line in capsys.readouterr().out.strip().split("\n"))
        want = repaired("shells24c4", wedge)
        assert not first["watertight"] and first["nonmanifold_edges"] == 25
        assert second["repair"] == dict(ref.info_dict(want["info"]), wedge=wedge)
        assert second["repaired"]["watertight"] and second["repaired"]["mesh"] == {"path": out, "vertices": len(want["verts"]), "faces": len(want["faces"])}
        back = mv.read_ply(out)
        assert np.array_equal(back["faces"], want["faces"]) and np.array_equal(back["verts"].view(np.uint32), want["verts"].view(np.uint32))
    with pytest.raises(ValueError, match=".ply"):
        tool.main(["--mesh", ply, "--repair", str(tmp_path / "fixed.obj")])


# ---- extract_mesh(repair=) -------------------------------------------------------------------------------------------------------------------------

N, VOLUME_SIZE = 32, 3.0


@pytest.fixture(scope="module")
def model():
    from nerfart_amd import scene
    return scene.build_model("VolSDF", seed=0, beta=0.01, device=DEV, precision="mixed")[0]


def test_extract_mesh_repairs_the_decimated_sphere_and_leaves_the_default_alone(model, tmp_path):
    from nerfart_amd import mesh_util
    kw = dict(volume_size=VOLUME_SIZE, N=N)
    for extra in (dict(), dict(simplify_factor=2), dict(simplify_factor=2, vertex_normals=True, color_model=model)):
        a = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "a.ply"), **kw, **extra)
        b = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "b.ply"), repair=False, repair_wedge="solid", **kw, **extra)
        assert open(a, "rb").read() == open(b, "rb").read()                 # off: the same bytes
    report = {}
    r = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "r.ply"), simplify_factor=2, repair=True, repair_info=report,
                               vertex_normals=True, color_model=model, **kw)
    got = mv.read_ply(r)
    t = mesh_util.mesh_topology(dev(got["verts"]), dev(got["faces"]))
    print(f"[repair] VolSDF N = {N}, factor 2, repaired: V = {len(got['verts'])}, F = {len(got['faces'])}, {report}")
    assert report["wide_edges"] == 0 and report["overflow"] == 0 and set(report) == set(mesh_util.REPAIR_INFO)
    assert t["watertight"] and t["components"][0]["genus"] == 0
    assert got["normals"].shape == got["verts"].shape and got["colors"].shape == got["verts"].shape      # queried at the repaired vertices
    # by hand: the same stages
    plain = mv.read_ply(mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "s.ply"), simplify_factor=2, **kw))
    before = mesh_util.mesh_topology(dev(plain["verts"]), dev(plain["faces"]), components=False)
    assert report["nonmanifold_edges"] == before["nonmanifold_edges"]
    # without simplification the extracted mesh is manifold already: repair is the identity on the file
    a = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "a.ply"), **kw)
    c = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "c.ply"), repair=True, **kw)
    assert open(a, "rb").read() == open(c, "rb").read()
    for bad, words in ((dict(repair=True, backend="skimage"), "repair"), (dict(repair=True, repair_wedge="both"), "repair_wedge"),
                       (dict(repair_wedge="both"), "repair_wedge")):
        with pytest.raises(ValueError, match=words):
            mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "no.ply"), **kw, **bad)
