"""tests/mesh_repair_ref.py (the numpy statement csrc/mesh_repair.hip is held to) against its own properties: hand meshes with answers known by
hand, the two clustered fixtures with real defects, tetrahedron soups (float positions, and lattice positions whose exact coplanarity leaves the
order to the tie rule), the guarantee through mesh_topology_ref, conservation of area and volume within a derived bound, idempotence, invariance
of the counts under relabelling, and three injected bugs that named assertions must catch; and, without a GPU, the refusals of the new entry
points and of mesh_util.repair_manifold."""
import ctypes as C
import math

import numpy as np
import pytest

import mc_ref
import mesh_components_ref as cref
import mesh_repair_ref as ref
import mesh_simplify_ref as sref
import mesh_topology_ref as topo
from test_mesh_topology_ref import TET_VERTS, shells_simplified

U64, U32 = 2.0 ** -53, 2.0 ** -24
_CACHE = {}


def noise_simplified():
    """noise_volume 12^3 clustered with factor 2: fins, unbalanced edges, edges of six.  (verts [V, 3] float32, faces [F, 3] int32)"""
    if "noise" not in _CACHE:
        v, f = mc_ref.marching_cubes(mc_ref.noise_volume((12, 12, 12)), 0.0)
        s = sref.simplify(v, f, (12, 12, 12), 2)
        _CACHE["noise"] = (s["verts"].astype(np.float32), s["faces"].astype(np.int32))
    return _CACHE["noise"]


def _tets(verts, quads):
    verts = np.array(verts, dtype=np.float32)
    return verts, np.array(sum((ref.outward_tetrahedron(verts, q) for q in quads), []), dtype=np.int32)


def hand_meshes():
    """name -> (verts, faces)"""
    rng = np.random.default_rng(3)
    v7 = np.concatenate([TET_VERTS, -TET_VERTS[1:]]).astype(np.float32)
    book = np.array([[0, 1, i] if i % 2 else [1, 0, i] for i in range(2, 72)], dtype=np.int32)         # 70 pages on one edge: wide
    return {
        "tetrahedron": (TET_VERTS, topo.TETRAHEDRON),
        "two_tetrahedra_one_vertex": (v7, np.concatenate([topo.TETRAHEDRON, np.array([[0, 4, 5], [0, 5, 6], [0, 6, 4], [4, 6, 5]], dtype=np.int32)])),
        # the shared edge 0 - 1 along z, one tetrahedron on either side of the plane x = 0
        "two_tetrahedra_one_edge": _tets([[0, 0, 0], [0, 0, 1], [1, -.3, .5], [1, .3, .5], [-1, .3, .5], [-1, -.3, .5]], [[0, 1, 2, 3], [0, 1, 4, 5]]),
        "three_on_one_edge": (rng.normal(size=(5, 3)).astype(np.float32), np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32)),
        "fin_pair": (TET_VERTS, np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int32)),
        "three_and_a_reverse": (TET_VERTS, np.array([[0, 1, 2], [2, 0, 1], [1, 0, 2], [1, 2, 0]], dtype=np.int32)),
        "degenerate_bad_duplicate": (rng.normal(size=(6, 3)).astype(np.float32),
                                     np.array([[0, 1, 2], [3, 3, 1], [0, 1, 7], [-1, 0, 1], [0, 1, 2]], dtype=np.int32)),
        "no_faces": (rng.normal(size=(5, 3)).astype(np.float32), np.zeros((0, 3), dtype=np.int32)),
        "nothing": (np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)),
        "no_vertices": (np.zeros((0, 3), dtype=np.float32), np.array([[0, 1, 2], [0, 0, 0]], dtype=np.int32)),
        "wide_book": (rng.normal(size=(72, 3)).astype(np.float32), book),
        "two_subdivided_in_one_face": ref.tetrahedron_soup(2, 5, 13),          # the smallest soup found in which a face is split twice
    }


SOUPS = {f"soup_{K}_{n}" + (f"_lattice{L}" if L else ""): (K, n, L)
         for K, n, L in ((2, 6, None), (3, 6, None), (3, 8, None), (4, 9, None), (5, 7, None), (8, 16, None), (10, 8, None), (20, 12, None), (40, 20, None), (40, 6, None),
                         (10, 8, 3), (40, 12, 3), (40, 20, 4))}
GENERATED = ["shells24c4", "noise12c2"] + list(SOUPS)


def generated(name):
    if name == "shells24c4":
        return shells_simplified()
    if name == "noise12c2":
        return noise_simplified()
    if name not in _CACHE:
        K, n, L = SOUPS[name]
        _CACHE[name] = ref.tetrahedron_soup(K, n, 100 + K + n, L)
    return _CACHE[name]


def all_meshes():
    """name -> a function returning (verts, faces): every mesh tests/test_gpu_mesh_repair.py compares on"""
    out = {k: (lambda k=k: hand_meshes()[k]) for k in hand_meshes()}
    out.update({k: (lambda k=k: generated(k)) for k in GENERATED})
    return out


def repaired(name, wedge):
    """ref.repair of a named mesh: computed once, shared, read-only"""
    if (name, wedge) not in _CACHE:
        r = ref.repair(*all_meshes()[name](), wedge)
        for a in r.values():
            a.setflags(write=False)
        _CACHE[(name, wedge)] = r
    return _CACHE[(name, wedge)]


def summary(r):
    return topo.summary(topo.topology(r["faces"], len(r["verts"]))["info"])


def n_components(r):
    return int(cref.components(r["faces"], len(r["verts"]))[2][1])


def info(r):
    return ref.info_dict(r["info"])


# ---- answers known by hand -----------------------------------------------------------------------------------------------------------------------

def test_a_tetrahedron_comes_back_as_it_is():
    r = repaired("tetrahedron", "void")
    assert np.array_equal(r["faces"], topo.TETRAHEDRON) and np.array_equal(r["verts"], TET_VERTS) and r["src_vertex"].tolist() == [0, 1, 2, 3]
    assert not r["info"].any() and r["mid_ends"].shape == (0, 2) and r["faces"].dtype == np.int32 and r["verts"].dtype == np.float32


def test_two_tetrahedra_sharing_one_vertex_are_separated():
    r = repaired("two_tetrahedra_one_vertex", "void")
    s = summary(r)
    assert info(r)["vertices_split"] == 1 and len(r["verts"]) == 8 and r["src_vertex"].tolist() == [0, 0, 1, 2, 3, 4, 5, 6]
    assert s["watertight"] and n_components(r) == 2 and s["euler"] == 4
    assert np.array_equal(r["verts"], hand_meshes()["two_tetrahedra_one_vertex"][0][r["src_vertex"]])


def check_two_on_an_edge(bug=None, wedge="solid", order=None):
    verts, faces = hand_meshes()["two_tetrahedra_one_edge"]
    if order is not None:
        faces = faces[order]
    r = ref.repair(verts, faces, wedge, _bug=bug)
    s = summary(r)
    i = info(r)
    assert i["nonmanifold_edges"] == 1 and i["edges_paired"] == 1 and i["unpaired_half_edges"] == 0
    assert s["nonmanifold_edges"] == 0, "a second pair on the same two classes is subdivided"
    if wedge == "solid":
        assert n_components(r) == 2 and s["euler"] == 4, "the pairs follow the angular order"
    else:
        assert n_components(r) == 1, "the pairs follow the angular order"
    assert s["watertight"]
    return r


def test_two_tetrahedra_sharing_one_edge():
    """n = 4 on the shared edge.  solid: the two come apart, two spheres, nothing subdivided.  void: one component; both pairs run between the
    same two umbrellas, so one of them is split at the midpoint."""
    r = check_two_on_an_edge(wedge="solid")
    assert info(r)["pairs_subdivided"] == 0 and info(r)["vertices_split"] == 2 and len(r["faces"]) == 8
    r = check_two_on_an_edge(wedge="void")
    assert info(r)["pairs_subdivided"] == 1 and len(r["faces"]) == 10 and r["src_vertex"][-1] == -1 and info(r)["vertices_split"] == 0
    assert np.array_equal(r["verts"][-1], np.array([0, 0, 0.5], dtype=np.float32)) and sorted(r["mid_ends"][0].tolist()) == [0, 1]
    rng = np.random.default_rng(0)
    for _ in range(6):                                                         # the pairing is geometry: the order of the faces does not matter
        order = rng.permutation(8)
        check_two_on_an_edge(wedge="solid", order=order)
        check_two_on_an_edge(wedge="void", order=order)


def check_three_on_an_edge(bug=None):
    r = ref.repair(*hand_meshes()["three_on_one_edge"], "void", _bug=bug)
    s = summary(r)
    assert s["nonmanifold_edges"] == 0 and s["bowtie_vertices"] == 0, "an unpaired half-edge joins no class"
    return r


def test_three_triangles_on_one_edge_leave_one_unpaired():
    r = check_three_on_an_edge()
    i, s = info(r), summary(r)
    assert (i["nonmanifold_edges"], i["edges_paired"], i["unpaired_half_edges"], i["vertices_split"], i["pairs_subdivided"]) == (1, 1, 1, 2, 0)
    assert len(r["verts"]) == 7 and len(r["faces"]) == 3 and s["boundary_edges"] == 7 and not s["watertight"] and n_components(r) == 2


def test_fins_and_duplicates_cancel_in_pairs():
    r = repaired("fin_pair", "void")
    assert len(r["faces"]) == 0 and len(r["verts"]) == 0 and info(r)["dropped_cancelled"] == 2 and not r["alive"].any()
    r = repaired("three_and_a_reverse", "void")                                # three of one orientation, one of the other: the first two survive
    assert r["alive"].tolist() == [True, True, False, False] and info(r)["dropped_cancelled"] == 2
    assert r["faces"].tolist() == [[0, 1, 2], [2, 0, 1]] and summary(r)["flipped_edges"] == 3


def test_degenerate_bad_and_empty():
    r = repaired("degenerate_bad_duplicate", "void")
    i = info(r)
    assert (i["dropped_bad"], i["dropped_degenerate"], i["dropped_cancelled"]) == (2, 1, 0) and r["faces"].tolist() == [[0, 1, 2], [0, 1, 2]]
    assert r["src_vertex"].tolist() == [0, 1, 2]
    for name in ("no_faces", "nothing"):
        r = repaired(name, "solid")
        assert r["verts"].shape == (0, 3) and r["faces"].shape == (0, 3) and r["src_vertex"].shape == (0,) and not r["info"].any()
    r = repaired("no_vertices", "void")
    assert info(r)["dropped_bad"] == 2 and r["faces"].shape == (0, 3)


def test_a_wide_edge_is_left_unpaired():
    r = repaired("wide_book", "void")
    i = info(r)
    assert (i["nonmanifold_edges"], i["wide_edges"], i["unpaired_half_edges"], i["edges_paired"]) == (1, 1, 70, 0)
    assert len(r["verts"]) == 70 + 2 * 70 and summary(r)["nonmanifold_edges"] == 0         # nothing joins the pages: 70 separate triangles


def test_a_face_with_two_subdivided_half_edges():
    r = repaired("two_subdivided_in_one_face", "void")
    assert len(hand_meshes()["two_subdivided_in_one_face"][1]) == 8 and r["splits"].max() >= 2
    s = summary(r)
    assert s["watertight"] and len(r["faces"]) == int(r["alive"].sum() + r["splits"].sum())
    k = int(np.argmax(r["splits"] >= 2))                                        # its first triangle sits in the face's place and starts at a midpoint
    place = int(r["alive"][:k].sum())
    assert r["src_vertex"][r["faces"][place, 0]] == -1


# ---- the generated meshes ------------------------------------------------------------------------------------------------------------------------

EXPECTED = {("shells24c4", "void"): dict(V=165, F=318, M=0, watertight=True, euler=6, boundary=0),
            ("shells24c4", "solid"): dict(V=160, F=324, M=3, watertight=True, euler=-2, boundary=0),
            ("noise12c2", "void"): dict(V=264, F=542, M=11, watertight=False, euler=None, boundary=6),
            ("noise12c2", "solid"): dict(V=316, F=522, M=1, watertight=False, euler=None, boundary=6)}


@pytest.mark.parametrize("wedge", ref.WEDGES)
@pytest.mark.parametrize("name", ["shells24c4", "noise12c2"])
def test_the_fixtures_reproduce_the_prototype(name, wedge):
    verts, faces = generated(name)
    r, want = repaired(name, wedge), EXPECTED[(name, wedge)]
    i, s = info(r), summary(r)
    assert (len(r["verts"]), len(r["faces"]), i["pairs_subdivided"], s["watertight"], s["boundary_edges"]) == \
        (want["V"], want["F"], want["M"], want["watertight"], want["boundary"])
    assert want["euler"] is None or s["euler"] == want["euler"]
    assert i["sort_ties"] == 0 and i["wide_edges"] == 0
    if name == "shells24c4":
        assert (len(faces), len(verts), i["nonmanifold_edges"], i["dropped_cancelled"], i["unpaired_half_edges"]) == (318, 126, 25, 0, 0)
        if wedge == "void":
            assert cref.ranked(*cref.components(r["faces"], len(r["verts"]))[:2])[1].tolist() == [210, 96, 12]
    else:
        assert (len(faces), i["dropped_cancelled"], int(r["alive"].sum()), i["nonmanifold_edges"], i["unpaired_half_edges"]) == (690, 170, 520, 84, 2)


def _len(x):
    return np.sqrt((x * x).sum(axis=-1))


def measure_bound(verts, faces, delta):
    """(sum of the area terms, of the volume terms, bound on |computed - exact| of each): math.fsum of mesh_topology_ref.face_terms with, per
    sum, the summation bound m 2^-53 sum|term| that `measure` is held to, the forward error of a term evaluated in fp64 (16 rounding errors at
    most on products of the lengths involved), and what a displacement of vertex v by at most delta[v] can change: a determinant is multilinear,
    so |det(p + dp, ...) - det(p, ...)| <= prod(|p| + |dp|) - prod |p|."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    area, volume = topo.face_terms(verts, f)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    da, db, dc = delta[f[:, 0]], delta[f[:, 1]], delta[f[:, 2]]
    u, w = _len(b - a), _len(c - a)
    la, lb, lc = _len(a), _len(b), _len(c)
    m = len(f)
    e_area = m * U64 * math.fsum(np.abs(area)) + math.fsum(8 * U64 * u * w) + math.fsum(0.5 * ((u + da + db) * (w + da + dc) - u * w))
    e_vol = m * U64 * math.fsum(np.abs(volume)) + math.fsum(16 * U64 * la * lb * lc / 6) + math.fsum(((la + da) * (lb + db) * (lc + dc) - la * lb * lc) / 6)
    return math.fsum(area), math.fsum(volume), e_area, e_vol


def check_generated(name, wedge, bug=None):
    verts, faces = generated(name)
    r = repaired(name, wedge) if bug is None else ref.repair(verts, faces, wedge, _bug=bug)
    i, s = info(r), summary(r)
    assert i["wide_edges"] == 0 and i["overflow"] == 0
    # the guarantee
    assert s["nonmanifold_edges"] == 0 and s["bowtie_vertices"] == 0 and s["degenerate_faces"] == 0 and s["bad_faces"] == 0, "the guarantee"
    before = topo.summary(topo.topology(np.where(r["alive"][:, None], faces, -1), len(verts))["info"])
    if i["unpaired_half_edges"] == 0 and before["boundary_edges"] == 0 and before["flipped_edges"] == 0:
        assert s["watertight"], "watertight"
    # structure
    M = len(r["mid_ends"])
    V1 = len(r["verts"]) - M
    assert (r["src_vertex"][:V1] >= 0).all() and (r["src_vertex"][V1:] == -1).all() and (np.diff(r["src_vertex"][:V1]) >= 0).all()
    assert np.array_equal(r["verts"][:V1], verts[r["src_vertex"][:V1]]) and s["referenced_vertices"] == len(r["verts"])
    assert len(r["faces"]) == int(r["alive"].sum() + r["splits"].sum()) and M == i["pairs_subdivided"]
    assert np.array_equal(r["src_vertex"][r["faces"][:int(r["alive"].sum())][r["splits"][r["alive"]] == 0]], faces[r["alive"] & (r["splits"] == 0)])
    # area and volume: subdivision is exact in exact arithmetic; a midpoint is one fp32 ulp of itself away from the edge at the most
    delta = np.zeros(len(r["verts"]))
    delta[V1:] = math.sqrt(3.0) * 2 * U32 * np.abs(r["verts"][V1:]).max(axis=1, initial=0.0)
    a0, v0, ea0, ev0 = measure_bound(verts, faces[r["alive"]], np.zeros(len(verts)))
    a1, v1, ea1, ev1 = measure_bound(r["verts"], r["faces"], delta)
    print(f"[repair] {name} {wedge}: area {a0:.6g} -> off by {abs(a1 - a0):.3g} of {ea0 + ea1:.3g} allowed; volume {v0:.6g} -> off by "
          f"{abs(v1 - v0):.3g} of {ev0 + ev1:.3g} allowed; M = {M}")
    assert abs(a1 - a0) <= ea0 + ea1, "area"
    assert abs(v1 - v0) <= ev0 + ev1, "volume"
    return r


@pytest.mark.parametrize("wedge", ref.WEDGES)
@pytest.mark.parametrize("name", GENERATED)
def test_generated_meshes_keep_the_guarantee_and_their_measure(name, wedge):
    r = check_generated(name, wedge)
    again = ref.repair(r["verts"], r["faces"], wedge)                           # idempotence
    assert np.array_equal(again["faces"], r["faces"]) and np.array_equal(again["verts"].view(np.uint32), r["verts"].view(np.uint32))
    assert np.array_equal(again["src_vertex"], np.arange(len(r["verts"]))) and not again["info"].any()


def test_the_soups_are_what_they_are_meant_to_be():
    widest, multi, ties = 0, 0, {}
    for name in SOUPS:
        verts, faces = generated(name)
        e = topo.edges(faces, len(verts))
        assert np.array_equal(e["n_fwd"], e["n_bwd"])                           # balanced by construction
        widest = max(widest, int((e["n_fwd"] + e["n_bwd"]).max()))
        multi += info(repaired(name, "void"))["pairs_subdivided"]
        ties[name] = info(repaired(name, "void"))["sort_ties"]
    assert 24 <= widest <= 64 and multi > 100
    assert all(ties[k] > 0 for k in SOUPS if "lattice" in k)                    # exact coplanarity: the tie rule carries the answer


ORDER_FREE = ("dropped_bad", "dropped_degenerate", "dropped_cancelled", "nonmanifold_edges", "edges_paired", "unpaired_half_edges", "wide_edges",
              "overflow")


def is_generic(name):
    """Float positions and no two surviving faces over one vertex set: no two apexes of an edge lie in one half-plane through it."""
    verts, faces = generated(name)
    t = np.sort(faces[ref.cancel(faces, len(verts))[0]], axis=1)
    return "lattice" not in name and len(np.unique(t, axis=0)) == len(t)


@pytest.mark.parametrize("name", GENERATED)
def test_relabelled_vertices_and_permuted_faces_give_the_same_counts(name):
    """Every count, where the geometry is generic.  Where two half-edges of an edge have the same direction - coincident faces in a soup over
    few vertices, coplanar ones on the lattice - the rules hand their order to the half-edge ids (and, against the reference half-edge, whose
    (1, 0) is exact while the other's y is a rounded zero, to rounding): then the pairs, and with them vertices_split, pairs_subdivided and
    sort_ties, follow the labelling by the rules' own design; the counts that no order can change must still agree."""
    verts, faces = generated(name)
    rng = np.random.default_rng(11)
    new_of_old, order = rng.permutation(len(verts)), rng.permutation(len(faces))
    verts2 = np.empty_like(verts)
    verts2[new_of_old] = verts
    faces2 = new_of_old[faces][order].astype(np.int32)
    for wedge in ref.WEDGES:
        r, r2 = repaired(name, wedge), ref.repair(verts2, faces2, wedge)
        assert {k: info(r2)[k] for k in ORDER_FREE} == {k: info(r)[k] for k in ORDER_FREE}, wedge
        assert int(r2["alive"].sum()) == int(r["alive"].sum())
        if is_generic(name):
            assert info(r2) == info(r) and info(r)["sort_ties"] == 0, wedge
            assert len(r2["faces"]) == len(r["faces"]) and len(r2["verts"]) == len(r["verts"])


def test_enough_generated_meshes_are_generic():
    generic = [k for k in GENERATED if is_generic(k)]
    assert {"shells24c4", "noise12c2", "soup_3_8", "soup_4_9", "soup_8_16"} <= set(generic)
    assert sum(info(repaired(k, "void"))["pairs_subdivided"] for k in generic) >= 10


@pytest.mark.parametrize("bug,check,words", [
    ("pair_by_id", lambda bug=None: [check_two_on_an_edge(bug, w, o) for w in ref.WEDGES for o in (None, [4, 0, 5, 1, 6, 2, 7, 3])],
     "follow the angular order"),
    ("skip_multi_edge", lambda bug=None: check_two_on_an_edge(bug, "void"), "is subdivided"),
    ("skip_multi_edge", lambda bug=None: check_generated("soup_10_8", "void", bug), "the guarantee"),
    ("unite_unpaired", check_three_on_an_edge, "joins no class"),
    ("unite_unpaired", lambda bug=None: check_generated("noise12c2", "void", bug), "the guarantee")])
def test_injected_bugs_are_caught_by_the_named_assertion(bug, check, words):
    check()
    with pytest.raises(AssertionError, match=words):
        check(bug)


# ---- without a GPU: refusals -----------------------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_before_any_launch():
    from nerfart_amd import hip
    lib, null, one = hip.lib, C.c_void_p(0), C.c_void_p(256)       # `one`: non-null, aligned, never dereferenced - the checks come first
    big = 1 << 31

    def err():
        return lib.nerfart_last_error().decode()

    wsb = lib.nerfart_mesh_repair_workspace_bytes
    for V, F, what in ((big, 4, "2^31"), (8, big, "2^31"), (8, 1431655766, "2^32")):
        assert wsb(V, F, 0) == 0 and what in err()
    assert wsb(8, 85, 7) == 0 and "3 F + 1" in err() and wsb(8, 85, 8) > 0
    assert wsb(8, 4, 32) == 0 and "table_log2" in err() and wsb(8, 4, -1) == 0 and "table_log2" in err()
    assert wsb(100, 200, 10) < wsb(100, 200, 0) == wsb(100, 200, 12) and wsb(0, 0, 0) > 0
    need = wsb(100, 200, 0)
    count = lambda **kw: lib.nerfart_mesh_repair_count(*[kw.get(k, d) for k, d in (("verts", one), ("faces", one), ("V", 100), ("F", 200), ("wedge", 0),
                                                                                   ("table_log2", 0), ("ws", one), ("ws_bytes", need), ("counts", one),
                                                                                   ("info", one), ("stream", null))])
    emit = lambda **kw: lib.nerfart_mesh_repair_emit(*[kw.get(k, d) for k, d in (("verts", one), ("faces", one), ("V", 100), ("F", 200), ("table_log2", 0),
                                                                                 ("ws", one), ("ws_bytes", need), ("verts_out", one), ("faces_out", one),
                                                                                 ("src_vertex", one), ("mid_ends", one), ("V_out", 100), ("M_out", 2),
                                                                                 ("F_out", 200), ("stream", null))])
    for k in ("verts", "faces", "ws", "counts", "info"):
        assert count(**{k: null}) == 2 and "null" in err(), k
    for k in ("verts", "faces", "ws", "verts_out", "faces_out", "src_vertex", "mid_ends"):
        assert emit(**{k: null}) == 2 and "null" in err(), k
    for fn in (count, emit):
        assert fn(V=big) == 2 and "2^31" in err() and fn(F=big) == 2 and "2^31" in err() and fn(F=1431655766) == 2 and "2^32" in err()
        assert fn(ws=C.c_void_p(260)) == 2 and "aligned" in err() and fn(ws_bytes=need - 1) == 2 and "workspace" in err()
        assert fn(table_log2=9) == 2 and "3 F + 1" in err() and fn(table_log2=13) == 2 and "workspace" in err()
    assert count(wedge=2) == 2 and "wedge" in err() and count(wedge=-1) == 2 and "wedge" in err()
    assert count(counts=C.c_void_p(260)) == 2 and "aligned" in err()
    assert emit(M_out=101) == 2 and "larger" in err() and emit(V_out=1201) == 2 and "larger" in err() and emit(F_out=801) == 2 and "larger" in err()


def test_python_front_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from nerfart_amd import hip, mesh_util
    faces, verts = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.repair_manifold(verts, faces)
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.repair_manifold(np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32))
    with pytest.raises(ValueError, match="wedge"):
        mesh_util.repair_manifold(verts, faces, wedge="both")
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        hip.mesh_repair_count(verts, faces)
    with pytest.raises(hip.NerfartHipError, match="wedge"):
        hip.mesh_repair_count(verts, faces, "both")
    with pytest.raises(hip.NerfartHipError, match="3 F"):
        hip.mesh_repair_workspace_bytes(4, 100, 4)
    for bad, words in ((dict(repair_wedge="both"), "repair_wedge"), (dict(repair=True, backend="skimage"), "repair needs")):
        with pytest.raises(ValueError, match=words):                            # refused before anything is imported, queried or written
            mesh_util.extract_mesh(None, filepath="/nonexistent/no.ply", **bad)
    assert mesh_util.REPAIR_INFO == ref.INFO and mesh_util.REPAIR_WEDGES == ref.WEDGES == hip.MESH_REPAIR_WEDGES
