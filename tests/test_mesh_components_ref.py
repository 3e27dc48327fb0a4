"""tests/mesh_components_ref.py (the numpy statement csrc/mesh_components.hip is held to) against hand-made meshes, the known component tables of
five marching-cubes meshes and the properties a filtered mesh must keep; and, without a GPU, the refusals of the new entry points, the argument
errors of mesh_util.filter_components / extract_mesh and the tool's two flags.  All comparisons are integer equality."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import yaml

import mc_ref
import mesh_components_ref as ref
from conftest import REPO

# name -> (volume, V, F, components, leading face counts in rank order, closed surface)
MESHES = {
    "noise_12": (lambda: mc_ref.noise_volume((12, 12, 12), seed=0, pad=True), 1652, 3340, 28, [2972, 80, 32, 24, 24, 16, 16, 16, 8, 8], True),
    "noise_16x12x10": (lambda: mc_ref.noise_volume((16, 12, 10), seed=1, pad=True), 1876, 3756, 29, [3308, 100, 60, 32, 24, 24, 16, 16, 16, 8], True),
    "noise_24": (lambda: mc_ref.noise_volume((24, 24, 24), seed=0, pad=True), 16818, 35112, 133, [33624, 88, 72, 40, 40, 32, 24], True),
    "noise_9x10x11_open": (lambda: mc_ref.noise_volume((9, 10, 11), seed=3, pad=False), 1340, 2351, 14, [2262, 33, 14, 8, 6, 4], False),
    "three_spheres": (ref.three_spheres, 384, 756, 3, [524, 200, 32], None),
}
_CACHE = {}


def mesh(name):
    """(V, faces [F, 3] int32, label, n_faces, info) of the named mesh at level 0: computed once, shared, never modified."""
    if name not in _CACHE:
        verts, faces = mc_ref.marching_cubes(MESHES[name][0](), 0.0)
        _CACHE[name] = (len(verts), faces) + ref.components(faces, len(verts))
        for a in _CACHE[name][1:]:
            a.setflags(write=False)
    return _CACHE[name]


def test_two_tetrahedra_and_an_isolated_vertex():
    tet = [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]
    faces = np.array(tet + [[a + 5, b + 5, c + 5] for a, b, c in tet], dtype=np.int32)           # vertex 4 is in no face
    label, n_faces, info = ref.components(faces, 9)
    assert label.tolist() == [0, 0, 0, 0, 4, 5, 5, 5, 5]
    assert n_faces.tolist() == [4, 0, 0, 0, 0, 4, 0, 0, 0] and info.tolist() == [3, 2, 0]
    roots, count = ref.ranked(label, n_faces)
    assert roots.tolist() == [0, 5, 4] and count.tolist() == [4, 4, 0]                            # the tie of 4s: the smaller label first
    src, out = ref.filter_components(9, faces, keep_largest=1)
    assert src.tolist() == [0, 1, 2, 3] and np.array_equal(out, faces[:4])
    src, out = ref.filter_components(9, faces, min_faces=1)
    assert src.tolist() == [0, 1, 2, 3, 5, 6, 7, 8] and np.array_equal(out[4:], faces[4:] - 1) and np.array_equal(out[:4], faces[:4])


def test_triangles_sharing_one_vertex_are_one_component():
    label, n_faces, info = ref.components(np.array([[4, 3, 2], [2, 1, 0]], dtype=np.int32), 5)
    assert label.tolist() == [0] * 5 and n_faces.tolist() == [2, 0, 0, 0, 0] and info.tolist() == [1, 1, 0]


def test_no_faces_and_bad_faces():
    label, n_faces, info = ref.components(np.zeros((0, 3), dtype=np.int32), 5)
    assert label.tolist() == [0, 1, 2, 3, 4] and not n_faces.any() and info.tolist() == [5, 0, 0]
    label, n_faces, info = ref.components(np.zeros((0, 3), dtype=np.int32), 0)
    assert label.shape == (0,) and info.tolist() == [0, 0, 0]
    faces = np.array([[0, 1, 2], [2, 3, -1], [3, 4, 5], [5, 6, 7]], dtype=np.int32)                # V = 7: faces 1 and 3 are bad
    label, n_faces, info = ref.components(faces, 7)
    assert label.tolist() == [0, 0, 0, 3, 3, 3, 6] and n_faces.tolist() == [1, 0, 0, 1, 0, 0, 0] and info.tolist() == [3, 2, 1]
    src, out = ref.compact(label, np.ones(7, dtype=np.uint8), faces, 7)
    assert src.tolist() == list(range(7)) and out.tolist() == [[0, 1, 2], [3, 4, 5]]


@pytest.mark.parametrize("name", list(MESHES))
def test_component_tables(name):
    _, V, F, comps, leading, closed = MESHES[name]
    n_verts, faces, label, n_faces, info = mesh(name)
    assert (n_verts, len(faces)) == (V, F)
    assert info.tolist() == [comps, comps, 0]                       # a marching-cubes vertex always has a face
    roots, count = ref.ranked(label, n_faces)
    assert count[:len(leading)].tolist() == leading and int(count.sum()) == F
    assert (np.diff(count) <= 0).all() and all(a < b for a, b, same in zip(roots, roots[1:], np.diff(count) == 0) if same)
    assert (label <= np.arange(V)).all() and (label[label] == label).all()
    assert (label[faces[:, 0]] == label[faces[:, 1]]).all() and (label[faces[:, 0]] == label[faces[:, 2]]).all()
    if closed is not None:
        assert mc_ref.is_closed(faces) == closed
    if name == "three_spheres":
        assert roots.tolist() == [0, 264, 291]


@pytest.mark.parametrize("name,kw", [("noise_12", dict(keep_largest=1)), ("noise_12", dict(keep_largest=4)), ("noise_12", dict(keep_largest=5)),
                                     ("noise_12", dict(min_faces=17)), ("noise_16x12x10", dict(keep_largest=2, min_faces=9)),
                                     ("noise_24", dict(min_faces=9)), ("noise_24", dict(keep_largest=5))])
def test_a_filtered_closed_mesh_stays_closed_and_euler_characteristics_add_up(name, kw):
    V, faces, label, n_faces, _ = mesh(name)
    keep = ref.keep_mask(label, n_faces, **kw)
    src, out = ref.compact(label, keep, faces, V)
    dsrc, dout = ref.compact(label, 1 - keep, faces, V)              # the dropped part
    assert len(src) + len(dsrc) == V and len(out) + len(dout) == len(faces) and 0 < len(out) < len(faces)
    assert (np.diff(src) > 0).all() and np.array_equal(src[out], faces[keep[label[faces[:, 0]]] == 1])
    assert mc_ref.is_closed(out) and mc_ref.is_consistently_oriented(out)
    assert mc_ref.euler_characteristic(len(src), out) + mc_ref.euler_characteristic(len(dsrc), dout) == mc_ref.euler_characteristic(V, faces)
    roots, count = ref.ranked(label, n_faces)
    want = [int(c) for r, c in enumerate(count)
            if (kw.get("keep_largest") is None or r < kw["keep_largest"]) and (kw.get("min_faces") is None or c >= kw["min_faces"])]
    assert len(out) == sum(want)


def test_the_tie_rule_decides_between_equal_components():
    """keep_largest = 4 and 5 on noise_12 cut inside the tie of 24s: the one with the smaller label goes first."""
    V, faces, label, n_faces, _ = mesh("noise_12")
    roots, count = ref.ranked(label, n_faces)
    assert count[3] == count[4] == 24 and roots[3] < roots[4]
    src4, _ = ref.filter_components(V, faces, keep_largest=4)
    src5, _ = ref.filter_components(V, faces, keep_largest=5)
    extra = np.setdiff1d(src5, src4)
    assert len(extra) > 0 and (label[extra] == roots[4]).all() and (label[src4] != roots[4]).all()


def test_keeping_everything_is_the_identity():
    for name in ("noise_12", "noise_9x10x11_open"):
        V, faces, label, n_faces, info = mesh(name)
        src, out = ref.filter_components(V, faces, keep_largest=int(info[0]))
        assert np.array_equal(src, np.arange(V)) and np.array_equal(out, faces)
        src, out = ref.filter_components(V, faces, min_faces=1)
        assert np.array_equal(src, np.arange(V)) and np.array_equal(out, faces)
    src, out = ref.filter_components(V, faces, min_faces=10 ** 6)   # and nothing surviving is empty
    assert src.shape == (0,) and out.shape == (0, 3)


def test_relabelled_vertices_and_permuted_faces_give_the_same_partition():
    V, faces, label, n_faces, info = mesh("noise_16x12x10")
    rng = np.random.default_rng(11)
    new_of_old = rng.permutation(V)
    faces2 = new_of_old[faces][rng.permutation(len(faces))].astype(np.int32)
    label2, n_faces2, info2 = ref.components(faces2, V)
    assert info2.tolist() == info.tolist()
    # the same partition: old vertices u, v share a label iff their images do - the map label -> label2 is well defined and injective
    pairs = np.unique(np.stack([label, label2[new_of_old]], axis=1), axis=0)
    assert len(pairs) == int(info[0]) and len(np.unique(pairs[:, 0])) == len(pairs) and len(np.unique(pairs[:, 1])) == len(pairs)
    assert sorted(n_faces2[n_faces2 > 0].tolist()) == sorted(n_faces[n_faces > 0].tolist())


# ---- without a GPU: refusals, argument errors, the tool's flags ---------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_before_any_launch():
    from nerfart_amd import hip
    lib, null, one = hip.lib, C.c_void_p(0), C.c_void_p(256)       # `one`: non-null, aligned, never dereferenced - the checks come first
    big = 1 << 31

    def err():
        return lib.nerfart_last_error().decode()

    assert lib.nerfart_mesh_components(null, 4, 8, one, one, one, null) == 2 and "null" in err()
    assert lib.nerfart_mesh_components(one, 4, 8, null, one, one, null) == 2 and "null" in err()
    assert lib.nerfart_mesh_components(one, 4, 8, one, null, one, null) == 2 and "null" in err()
    assert lib.nerfart_mesh_components(one, 4, 8, one, one, null, null) == 2 and "null" in err()
    assert lib.nerfart_mesh_components(one, 4, big, one, one, one, null) == 2 and "2^31" in err()
    assert lib.nerfart_mesh_components(one, big, 8, one, one, one, null) == 2 and "2^31" in err()
    assert lib.nerfart_mesh_components(one, 1431655766, 8, one, one, one, null) == 2 and "2^32" in err()          # 3 F = 2^32 + 2
    for V, F, what in ((big, 4, "2^31"), (8, big, "2^31"), (8, 1431655766, "2^32")):
        assert lib.nerfart_mesh_compact_workspace_bytes(V, F) == 0 and what in err()
        assert lib.nerfart_mesh_compact_count(one, one, one, V, F, one, 1 << 40, one, null) == 2 and what in err()
        assert lib.nerfart_mesh_compact_emit(one, one, one, V, F, one, 1 << 40, one, one, 1, 1, null) == 2 and what in err()
    # the workspace: (vertex, face) offsets of max(V, F, 1) items and the block sums per level, each buffer rounded up to 256 bytes
    total = lambda sizes: sum((b + 255) // 256 * 256 for b in sizes)
    assert lib.nerfart_mesh_compact_workspace_bytes(0, 0) == 256
    assert lib.nerfart_mesh_compact_workspace_bytes(500, 512) == total([8 * 512])
    assert lib.nerfart_mesh_compact_workspace_bytes(513, 100) == total([8 * 513, 8 * 2])
    assert lib.nerfart_mesh_compact_workspace_bytes(1000, 300000) == total([8 * 300000, 8 * 586, 8 * 2])
    assert lib.nerfart_mesh_compact_workspace_bytes(1431655765, 1431655765) > 0                                   # 3 F = 2^32 - 1
    need = lib.nerfart_mesh_compact_workspace_bytes(100, 200)
    count = lambda **kw: lib.nerfart_mesh_compact_count(*[kw.get(k, d) for k, d in (("label", one), ("keep", one), ("faces", one), ("V", 100), ("F", 200),
                                                                                    ("ws", one), ("ws_bytes", need), ("counts", one), ("stream", null))])
    emit = lambda **kw: lib.nerfart_mesh_compact_emit(*[kw.get(k, d) for k, d in (("label", one), ("keep", one), ("faces", one), ("V", 100), ("F", 200),
                                                                                  ("ws", one), ("ws_bytes", need), ("src_vertex", one), ("faces_out", one),
                                                                                  ("V_out", 10), ("F_out", 20), ("stream", null))])
    for k in ("label", "keep", "faces", "ws", "counts"):
        assert count(**{k: null}) == 2 and "null" in err(), k
    for k in ("label", "keep", "faces", "ws", "src_vertex", "faces_out"):
        assert emit(**{k: null}) == 2 and "null" in err(), k
    for fn in (count, emit):
        assert fn(ws_bytes=need - 1) == 2 and "workspace" in err()
        assert fn(ws=C.c_void_p(260)) == 2 and "aligned" in err()
    assert count(counts=C.c_void_p(260)) == 2 and "aligned" in err()
    assert emit(V_out=0, F_out=0, src_vertex=null, faces_out=null) == 0          # an empty result launches nothing and succeeds


def test_python_front_refuses_cpu_tensors_and_bad_options():
    import torch
    from nerfart_amd import hip, mesh_util
    faces, verts = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        mesh_util.mesh_components(faces, 4)
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        mesh_util.filter_components(verts, faces, keep_largest=1)
    with pytest.raises(ValueError, match="keep_largest"):
        mesh_util.filter_components(verts, faces)
    with pytest.raises(ValueError, match="keep_largest"):
        mesh_util.filter_components(verts, faces, keep_largest=0)
    with pytest.raises(ValueError, match="min_faces"):
        mesh_util.filter_components(verts, faces, min_faces=0)
    for kw in (dict(keep_largest=1), dict(min_component_faces=10)):
        with pytest.raises(ValueError, match="native"):
            mesh_util.extract_mesh(None, backend="skimage", **kw)


def test_the_tool_takes_the_two_flags(tmp_path):
    from nerfart_amd import scene
    spec = importlib.util.spec_from_file_location("extract_surface", os.path.join(REPO, "tools", "extract_surface.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    d = scene.synthetic_config("NeuS").to_dict()
    d["expname"] = "mesh"
    d.setdefault("training", {})["log_root_dir"] = str(tmp_path)
    path = tmp_path / "neus.yaml"
    path.write_text(yaml.dump(d))
    args, _ = tool.parse(["--config", str(path), "--keep_largest", "2", "--min_faces", "100"])
    assert (args.keep_largest, args.min_faces) == (2, 100)
    args, _ = tool.parse(["--config", str(path)])
    assert (args.keep_largest, args.min_faces) == (None, None)
