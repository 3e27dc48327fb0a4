"""tests/mesh_topology_ref.py (the numpy statement csrc/mesh_topology.hip is held to) against answers known by hand - closed, open, twisted and
broken meshes -, against mc_ref's predicates on the marching-cubes meshes, under relabelling, and with three injected bugs that named assertions
must catch; and, without a GPU, the refusals of the new entry points and of their Python front.  All integer comparisons are equalities."""
import ctypes as C
import math

import numpy as np
import pytest

import mc_ref
import mesh_components_ref as cref
import mesh_simplify_ref as sref
import mesh_topology_ref as ref
from test_mesh_components_ref import MESHES, mesh

TET_VERTS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
_TOPO = {}


def topo(name):
    """ref.topology of the named MESHES mesh: computed once, shared, read-only"""
    if name not in _TOPO:
        V, faces = mesh(name)[:2]
        _TOPO[name] = ref.topology(faces, V)
    return _TOPO[name]


def info(t):
    return dict(zip(ref.INFO, (int(x) for x in t["info"])))


def shells_simplified():
    """shells_volume 24^3 clustered with factor 4: a mesh with real defects.  (verts [V, 3] float32, faces [F, 3] int32)"""
    if "shells" not in _TOPO:
        v, f = mc_ref.marching_cubes(sref.shells_volume((24, 24, 24), (11.4, 11.6, 11.3), 3.3, 6.4, 9.6), 0.0)
        s = sref.simplify(v, f, (24, 24, 24), 4)
        _TOPO["shells"] = (s["verts"].astype(np.float32), s["faces"].astype(np.int32))
    return _TOPO["shells"]


# ---- answers known by hand -----------------------------------------------------------------------------------------------------------------------

def check_tetrahedron(bug=None):
    """the named assertions the injected bugs are held to"""
    t = ref.topology(ref.TETRAHEDRON, 4, _bug=bug)
    i = info(t)
    assert i["edges"] == 6, "edges are counted once per undirected edge"
    assert i["boundary_edges"] == 0 and i["flipped_edges"] == 0, "opposite half-edges meet in one key"
    assert ref.summary(t["info"])["euler"] == 2, "euler"
    return t


def check_three_on_an_edge(bug=None):
    faces = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32)
    t = ref.topology(faces, 5, _bug=bug)
    i = info(t)
    assert i["nonmanifold_edges"] == 1 and i["edges"] == 7 and i["boundary_edges"] == 6, "one edge in three faces, counted once"
    assert t["vertex_fans"].tolist() == [3, 3, 1, 1, 1], "a non-manifold edge joins no fans"
    return t


def test_tetrahedron():
    t = check_tetrahedron()
    s = ref.summary(t["info"])
    assert (s["referenced_vertices"], s["edges"], s["proper_faces"], s["euler"]) == (4, 6, 4, 2) and s["watertight"] and s["boundary_loops"] == 0
    assert t["edge_uses"].tolist() == [2] * 12 and t["vertex_fans"].tolist() == [1] * 4
    tw = t["twin"]
    assert (tw >= 0).all() and np.array_equal(tw[tw], np.arange(12)) and (tw // 3 != np.arange(12) // 3).all()
    flat = ref.TETRAHEDRON.reshape(-1)
    nxt = np.arange(12) // 3 * 3 + (np.arange(12) + 1) % 3
    assert np.array_equal(flat[tw], flat[nxt]) and np.array_equal(flat[nxt[tw]], flat)          # the twin runs the other way
    c = ref.component_stats(TET_VERTS, ref.TETRAHEDRON, 4, np.zeros(4, dtype=np.int32))
    assert c["counts"].tolist() == [[4, 6, 4, 0, 0, 0]] + [[0] * 6] * 3
    assert c["measure"][0, 1] == pytest.approx(1 / 6, rel=1e-15) and c["measure"][0, 0] == pytest.approx(1.5 + math.sqrt(3) / 2, rel=1e-15)
    r = ref.report(TET_VERTS, ref.TETRAHEDRON)
    assert len(r["components"]) == 1 and r["components"][0]["genus"] == 0 and r["components"][0]["closed"]


@pytest.mark.parametrize("n,m", [(3, 3), (4, 7)])
def test_torus_sheet_and_annulus(n, m):
    V, faces = ref.grid_faces(n, m, True, True)
    s = ref.summary(ref.topology(faces, V)["info"])
    assert s["euler"] == 0 and s["watertight"] and (s["referenced_vertices"], s["edges"], s["proper_faces"]) == (n * m, 3 * n * m, 2 * n * m)
    assert ref.report(np.zeros((V, 3), np.float32), faces)["components"][0]["genus"] == 1
    V, faces = ref.grid_faces(n, m)
    t = ref.topology(faces, V)
    s = ref.summary(t["info"])
    assert s["euler"] == 1 and s["boundary_loops"] == 1 and s["longest_loop"] == s["boundary_edges"] == 2 * (n + m) and not s["closed"]
    assert s["oriented"] and s["manifold"] and not s["watertight"] and (t["vertex_fans"] == 1).all()
    assert ref.report(np.zeros((V, 3), np.float32), faces)["components"][0]["genus"] is None
    V, faces = ref.grid_faces(n, m, wrap_u=True)
    t = ref.topology(faces, V)
    s = ref.summary(t["info"])
    assert s["euler"] == 0 and s["boundary_loops"] == 2 and t["loop_sizes"].tolist() == [n, n] and s["oriented"] and s["manifold"]


def test_two_tetrahedra_sharing_one_vertex():
    other = np.array([[0, 4, 5], [0, 5, 6], [0, 6, 4], [4, 6, 5]], dtype=np.int32)
    faces = np.concatenate([ref.TETRAHEDRON, other])
    t = ref.topology(faces, 7)
    s = ref.summary(t["info"])
    assert t["vertex_fans"].tolist() == [2, 1, 1, 1, 1, 1, 1] and s["bowtie_vertices"] == 1 and s["euler"] == 3
    assert s["closed"] and s["oriented"] and not s["manifold"] and not s["watertight"]
    r = ref.report(np.zeros((7, 3), np.float32), faces)
    assert len(r["components"]) == 1 and r["components"][0]["genus"] is None and r["components"][0]["euler"] == 3


def test_three_triangles_on_one_edge():
    t = check_three_on_an_edge()
    assert t["twin"].tolist() == [-3, -1, -1, -3, -1, -1, -3, -1, -1] and t["edge_uses"].tolist() == [3, 1, 1] * 3
    assert info(t)["boundary_loops"] == 1 and info(t)["longest_loop"] == 6


def test_two_triangles_crossing_their_edge_the_same_way():
    t = ref.topology(np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int32), 4)
    i = info(t)
    assert i["flipped_edges"] == 1 and i["edges"] == 5 and i["boundary_edges"] == 4 and i["nonmanifold_edges"] == 0
    assert t["twin"].tolist() == [-2, -1, -1, -2, -1, -1] and t["edge_uses"].tolist() == [2, 1, 1, 2, 1, 1]
    assert t["vertex_fans"].tolist() == [1, 1, 1, 1]                        # a flipped edge still joins the two faces' corners
    assert not ref.summary(t["info"])["oriented"]


def test_moebius_band_has_a_flipped_edge_for_every_orientation():
    V, faces = ref.moebius_faces(3)
    t = ref.topology(faces, V)
    assert info(t)["nonmanifold_edges"] == 0 and info(t)["boundary_loops"] == 1 and ref.summary(t["info"])["euler"] == 0
    for bits in range(1 << len(faces)):
        f = faces.copy()
        flip = [(bits >> k) & 1 == 1 for k in range(len(faces))]
        f[flip] = f[flip][:, [0, 2, 1]]
        assert info(ref.topology(f, V))["flipped_edges"] >= 1
    V, faces = ref.grid_faces(3, 1, wrap_u=True)                            # the untwisted band of the same size can be oriented
    assert info(ref.topology(faces, V))["flipped_edges"] == 0


def test_degenerate_bad_duplicated_unreferenced_and_empty():
    faces = np.array([[0, 1, 2], [3, 3, 1], [0, 1, 7], [-1, 0, 1], [0, 1, 2]], dtype=np.int32)
    t = ref.topology(faces, 6)                                              # vertices 4, 5 unreferenced; 3 only in the degenerate face
    i = info(t)
    assert (i["proper_faces"], i["degenerate_faces"], i["bad_faces"], i["referenced_vertices"]) == (2, 1, 2, 3)
    assert i["edges"] == 3 and i["flipped_edges"] == 3 and i["boundary_edges"] == 0           # the duplicate runs through every edge the same way
    assert t["twin"].tolist() == [-2] * 3 + [-4] * 9 + [-2] * 3 and t["edge_uses"].tolist() == [2] * 3 + [0] * 9 + [2] * 3
    assert t["vertex_fans"].tolist() == [1, 1, 1, 0, 0, 0] and not ref.summary(t["info"])["watertight"]
    label = cref.components(faces, 6)[0]
    c = ref.component_stats(np.zeros((6, 3), np.float32), faces, 6, label)
    assert c["counts"][0].tolist() == [3, 3, 2, 0, 3, 0] and not c["counts"][1:].any()
    for V in (0, 5):
        t = ref.topology(np.zeros((0, 3), dtype=np.int32), V)
        assert not t["info"].any() and t["twin"].shape == (0,) and t["vertex_fans"].tolist() == [0] * V
        assert ref.summary(t["info"])["watertight"] and ref.summary(t["info"])["euler"] == 0


# ---- the marching-cubes meshes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MESHES))
def test_marching_cubes_meshes_agree_with_mc_ref(name):
    V, faces, label, n_faces, cinfo = mesh(name)
    t = topo(name)
    s = ref.summary(t["info"])
    assert (s["closed"] and s["nonmanifold_edges"] == 0) == mc_ref.is_closed(faces)                       # every edge in exactly two faces
    assert (s["closed"] and s["oriented"] and s["nonmanifold_edges"] == 0) == mc_ref.is_consistently_oriented(faces)      # every edge manifold
    assert s["euler"] == mc_ref.euler_characteristic(V, faces) and s["referenced_vertices"] == V and s["proper_faces"] == len(faces)
    assert s["edges"] == len(mc_ref.undirected_edge_counts(faces)[0])
    if MESHES[name][5]:                                                     # the padded noise volumes: mc_table.py's promise
        assert s["watertight"] and (t["twin"] >= 0).all() and (t["vertex_fans"] == 1).all()
    if name == "noise_9x10x11_open":
        assert s["boundary_edges"] > 0 and s["flipped_edges"] == 0 and s["nonmanifold_edges"] == 0 and s["bowtie_vertices"] == 0
        assert int(t["loop_sizes"].sum()) == s["boundary_edges"] and s["longest_loop"] == t["loop_sizes"][0]
    verts = mc_ref.marching_cubes(MESHES[name][0](), 0.0)[0]
    c = ref.component_stats(verts, faces, V, label)
    assert np.array_equal(c["counts"][:, 2], n_faces) and int(c["counts"][:, 1].sum()) == s["edges"]
    assert (c["counts"][label != np.arange(V)] == 0).all()
    vol = mc_ref.signed_volume(verts.astype(np.float32), faces)
    assert float(c["measure"][:, 1].sum()) == pytest.approx(vol, rel=1e-12, abs=1e-12)
    r = ref.report(verts, faces)
    assert sum(k["euler"] for k in r["components"]) == s["euler"] and [k["faces"] for k in r["components"]][:3] == MESHES[name][4][:3]
    if MESHES[name][5]:
        assert all(k["genus"] is not None and k["genus"] >= 0 and k["volume"] > 0 for k in r["components"])


def test_simplified_shells_are_broken():
    """Three nested spheres (chi = 6) stay closed under vertex clustering but do not stay manifold; the counts are this statement's own, pinned."""
    v, f = mc_ref.marching_cubes(sref.shells_volume((24, 24, 24), (11.4, 11.6, 11.3), 3.3, 6.4, 9.6), 0.0)
    s = ref.summary(ref.topology(f, len(v))["info"])
    assert s["watertight"] and s["euler"] == 6
    verts, faces = shells_simplified()
    s = ref.summary(ref.topology(faces, len(verts))["info"])
    assert (s["boundary_edges"], s["flipped_edges"], s["nonmanifold_edges"], s["bowtie_vertices"], s["euler"]) == (0, 0, 25, 39, -8)
    assert not s["manifold"] and not s["watertight"]


def test_relabelled_vertices_and_permuted_faces_give_the_same_counts_and_twins():
    V, faces = mesh("noise_9x10x11_open")[:2]
    t = topo("noise_9x10x11_open")
    rng = np.random.default_rng(5)
    new_of_old, order = rng.permutation(V), rng.permutation(len(faces))
    faces2 = new_of_old[faces][order].astype(np.int32)
    t2 = ref.topology(faces2, V)
    assert np.array_equal(t2["info"], t["info"]) and np.array_equal(t2["loop_sizes"], t["loop_sizes"])
    assert np.array_equal(t2["vertex_fans"][new_of_old], t["vertex_fans"])
    he2_of_he = np.empty(3 * len(faces), dtype=np.int64)                    # old half-edge 3 f + i is new half-edge 3 position(f) + i
    he2_of_he[(3 * order[:, None] + np.arange(3)).reshape(-1)] = np.arange(3 * len(faces))
    tw, tw2 = t["twin"].astype(np.int64), t2["twin"].astype(np.int64)
    mapped = np.where(tw >= 0, he2_of_he[np.maximum(tw, 0)], tw)
    assert np.array_equal(tw2[he2_of_he], mapped) and np.array_equal(t2["edge_uses"][he2_of_he], t["edge_uses"])


@pytest.mark.parametrize("bug,check", [("reversed_key", check_tetrahedron), ("per_half_edge", check_tetrahedron),
                                       ("per_half_edge", check_three_on_an_edge), ("fans_across_nonmanifold", check_three_on_an_edge)])
def test_injected_bugs_are_caught(bug, check):
    check()
    with pytest.raises(AssertionError):
        check(bug)


def test_injected_bugs_are_caught_by_the_named_assertion():
    for bug, check, words in (("reversed_key", check_tetrahedron, "once per undirected edge"), ("per_half_edge", check_three_on_an_edge, "counted once"),
                              ("fans_across_nonmanifold", check_three_on_an_edge, "joins no fans")):
        with pytest.raises(AssertionError, match=words):
            check(bug)


# ---- without a GPU: refusals -----------------------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_before_any_launch():
    from nerfart_amd import hip
    lib, null, one = hip.lib, C.c_void_p(0), C.c_void_p(256)       # `one`: non-null, aligned, never dereferenced - the checks come first
    big = 1 << 31

    def err():
        return lib.nerfart_last_error().decode()

    wsb = lib.nerfart_mesh_topology_workspace_bytes
    for V, F, what in ((big, 4, "2^31"), (8, big, "2^31"), (8, 1431655766, "2^32")):
        assert wsb(V, F, 0) == 0 and what in err()
    assert wsb(8, 85, 7) == 0 and "3 F + 1" in err()                # 128 < 256 = 3 F + 1
    assert wsb(8, 85, 8) > 0 and wsb(8, 86, 8) == 0 and "3 F + 1" in err()
    assert wsb(8, 4, 32) == 0 and "table_log2" in err() and wsb(8, 4, -1) == 0 and "table_log2" in err()
    assert wsb(8, 715827883, 0) == 0 and "3 F + 1" in err()         # 3 F + 1 = 2^31 + 2: no table is large enough
    assert wsb(8, 715827882, 0) > 0                                 # 3 F + 1 = 2^31 - 1
    up = lambda b: (b + 255) // 256 * 256
    assert wsb(0, 0, 0) == 5 * 256 + up(24 * 8)
    assert wsb(100, 85, 0) == 2 * up(4 * 255) + 3 * up(400) + up(24 * 1024) and wsb(100, 85, 8) == 2 * up(4 * 255) + 3 * up(400) + up(24 * 256)
    need = wsb(100, 200, 0)
    half = lambda **kw: lib.nerfart_mesh_half_edges(*[kw.get(k, d) for k, d in (("faces", one), ("F", 200), ("V", 100), ("table_log2", 0), ("ws", one),
                                                                                ("ws_bytes", need), ("twin", one), ("edge_uses", one),
                                                                                ("vertex_fans", one), ("info", one), ("stream", null))])
    stats = lambda **kw: lib.nerfart_mesh_component_stats(*[kw.get(k, d) for k, d in (("verts", one), ("faces", one), ("F", 200), ("V", 100),
                                                                                      ("label", one), ("ws", one), ("ws_bytes", need), ("counts", one),
                                                                                      ("measure", one), ("stream", null))])
    for k in ("faces", "ws", "twin", "edge_uses", "vertex_fans", "info"):
        assert half(**{k: null}) == 2 and "null" in err(), k
    for k in ("verts", "faces", "label", "ws", "counts", "measure"):
        assert stats(**{k: null}) == 2 and "null" in err(), k
    for fn in (half, stats):
        assert fn(V=big) == 2 and "2^31" in err() and fn(F=big) == 2 and "2^31" in err() and fn(F=1431655766) == 2 and "2^32" in err()
        assert fn(ws=C.c_void_p(260)) == 2 and "aligned" in err()
    assert half(ws_bytes=need - 1) == 2 and "workspace" in err()
    assert half(table_log2=9) == 2 and "3 F + 1" in err()           # 512 < 601, refused before any launch
    assert half(table_log2=13, ws_bytes=need) == 2 and "workspace" in err()          # a larger table needs a larger workspace
    assert stats(ws_bytes=wsb(100, 200, 10) - 1) == 2 and "workspace" in err()       # the smallest legal table's workspace is the least
    assert stats(measure=C.c_void_p(260)) == 2 and "aligned" in err()


def test_python_front_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from nerfart_amd import hip, mesh_util
    faces, verts = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.half_edges(faces, 4)
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.mesh_topology(verts, faces)
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.half_edges(np.zeros((2, 3), np.int32), 4)
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        hip.mesh_half_edges(faces, 4)
    with pytest.raises(hip.NerfartHipError, match=r"\[F, 3\]"):
        hip.mesh_half_edges(torch.zeros(6, dtype=torch.int32), 4)
    with pytest.raises(hip.NerfartHipError, match="3 F"):
        hip.mesh_topology_workspace_bytes(4, 100, 4)
    assert mesh_util.TOPOLOGY_INFO == ref.INFO
