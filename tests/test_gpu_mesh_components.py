"""csrc/mesh_components.hip (mesh_util.mesh_components / filter_components / extract_mesh(keep_largest=, min_component_faces=)) against the numpy
statement tests/mesh_components_ref.py, which tests/test_mesh_components_ref.py holds to known component tables.  Everything is integers: every
comparison is equality.  Labelling on the marching-cubes meshes, degenerate and ragged sizes, long parent chains, bad faces; the compaction for
every selection rule, its write discipline and determinism, all three depths of its scan; and extract_mesh end to end."""
import numpy as np
import pytest
import torch

import mc_ref
import mesh_components_ref as ref
import mesh_vertices_ref as mv
from mesh_pipeline_ref import WithFloaters
from test_mesh_components_ref import MESHES, mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
PAD = 32                   # sentinel words on either side of every output array


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)               # a copy: the shared reference arrays are read-only


def gpu_components(faces, V):
    from nerfart_amd import hip
    label, n_faces, info = hip.mesh_components(dev(faces, np.int32).reshape(-1, 3), V)
    assert label.dtype == n_faces.dtype == info.dtype == torch.int32 and label.shape == n_faces.shape == (V,) and info.shape == (3,)
    return label.cpu().numpy(), n_faces.cpu().numpy().view(np.uint32), info.cpu().numpy().view(np.uint32)


def check_components(faces, V):
    want = ref.components(faces, V)
    got = gpu_components(faces, V)
    for g, w, what in zip(got, want, ("label", "n_faces", "info")):
        assert np.array_equal(g, w), what
    return want


def gpu_compact(label, keep, faces, V):
    from nerfart_amd import hip
    src, out = hip.mesh_compact(dev(label, np.int32), dev(keep, np.uint8), dev(faces, np.int32).reshape(-1, 3), V)
    assert src.dtype == out.dtype == torch.int32 and out.dim() == 2 and out.shape[1] == 3
    return src.cpu().numpy(), out.cpu().numpy()


def check_compact(label, keep, faces, V):
    want = ref.compact(label, keep, faces, V)
    got = gpu_compact(label, keep, faces, V)
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return want


# ---- labelling -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["reference_faces", "gpu_marching_cubes"])
@pytest.mark.parametrize("name", list(MESHES))
def test_labels_counts_and_info_are_the_reference(name, source):
    from nerfart_amd import mesh_util
    V, faces, label, n_faces, info = mesh(name)
    if source == "gpu_marching_cubes":
        verts, gfaces = mesh_util.marching_cubes(dev(MESHES[name][0]()), 0.0)
        assert verts.shape[0] == V and np.array_equal(gfaces.cpu().numpy(), faces)
        glabel, roots, count = mesh_util.mesh_components(gfaces, V)
        assert glabel.device == roots.device == count.device == gfaces.device and roots.dtype == count.dtype == torch.int32
        rroots, rcount = ref.ranked(label, n_faces)
        assert np.array_equal(glabel.cpu().numpy(), label) and np.array_equal(roots.cpu().numpy(), rroots) and np.array_equal(count.cpu().numpy(), rcount)
        assert count[:len(MESHES[name][4])].tolist() == MESHES[name][4]
        return
    got = gpu_components(faces, V)
    assert np.array_equal(got[0], label) and np.array_equal(got[1], n_faces) and np.array_equal(got[2], info)
    assert got[2].tolist() == [MESHES[name][3], MESHES[name][3], 0]


def test_degenerate_sizes():
    none = np.zeros((0, 3), dtype=np.int32)
    label, n_faces, info = check_components(none, 0)
    assert label.shape == (0,) and info.tolist() == [0, 0, 0]
    label, n_faces, info = check_components(none, 5)
    assert label.tolist() == [0, 1, 2, 3, 4] and not n_faces.any() and info.tolist() == [5, 0, 0]
    label, n_faces, info = check_components(np.array([[2, 0, 1]], dtype=np.int32), 3)
    assert label.tolist() == [0, 0, 0] and n_faces.tolist() == [1, 0, 0] and info.tolist() == [1, 1, 0]
    # isolated vertices between used ones, and two triangles sharing ONE vertex: one component
    label, n_faces, info = check_components(np.array([[9, 7, 5], [5, 3, 1], [2, 4, 6]], dtype=np.int32), 11)
    assert label.tolist() == [0, 1, 2, 1, 2, 1, 2, 1, 8, 1, 10] and n_faces.tolist() == [0, 2, 1] + [0] * 8 and info.tolist() == [5, 2, 0]


def test_sizes_around_wave_and_block_boundaries():
    """Ragged tails of every kernel: V around one wave (64) and two scan blocks (512), F around one block of threads (256) and two scan blocks."""
    rng = np.random.default_rng(3)
    for V in (1, 63, 64, 65, 513):
        for F in (1, 255, 256, 257, 1025):
            # a face joins a random vertex to its neighbours; most faces repeat the first one, so that several components are left
            base = rng.integers(0, V, size=F)
            faces = np.stack([base, np.minimum(base + rng.integers(0, 2, size=F), V - 1), np.maximum(base - rng.integers(0, 2, size=F), 0)], 1).astype(np.int32)
            faces[rng.random(F) < 0.6] = faces[0]
            label, n_faces, info = check_components(faces, V)
            keep = (rng.random(V) < 0.5).astype(np.uint8)
            check_compact(label, keep, faces, V)
            if V == 513 and F == 255:
                assert 1 < info[1] < info[0] < V          # components with and without faces


@pytest.mark.parametrize("order", ["permuted", "smallest_index_at_the_far_end"])
def test_long_chains(order):
    """A triangle strip of 3,000 faces is one component whose parent chains can grow as long as the strip: the find / flatten loops."""
    strip = ref.triangle_strip(3000)
    V = 3002
    if order == "permuted":
        rng = np.random.default_rng(7)
        faces = rng.permutation(V)[strip][rng.permutation(len(strip))].astype(np.int32)
    else:
        faces = (V - 1 - strip).astype(np.int32)            # face k = (V - 1 - k, V - 2 - k, V - 3 - k): vertex 0 is met by the last face only
    label, n_faces, info = check_components(faces, V)
    assert not label.any() and n_faces[0] == 3000 and info.tolist() == [1, 1, 0]


def _bad_mesh():
    V, faces, *_ = mesh("noise_12")
    faces = faces.copy()
    faces[100, 1] = -1
    faces[2000, 2] = V
    return V, faces


def test_bad_faces_join_nothing_and_touch_nothing():
    from nerfart_amd import hip, mesh_util
    V, faces = _bad_mesh()
    want = ref.components(faces, V)
    good = ref.components(faces[ref.good_faces(faces, V)], V)
    assert want[2].tolist()[2] == 1 and np.array_equal(want[0], good[0]) and np.array_equal(want[1], good[1])
    # outputs inside sentinel-filled buffers
    label = torch.full((V + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    n_faces = torch.full((V + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    info = torch.full((3 + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    f = dev(faces)
    rc = hip.lib.nerfart_mesh_components(f.data_ptr(), len(faces), V, label[PAD:].data_ptr(), n_faces[PAD:].data_ptr(), info[PAD:].data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    for buf, w, n in ((label, want[0], V), (n_faces, want[1], V), (info, want[2], 3)):
        b = buf.cpu().numpy().view(np.uint32)
        assert (b[:PAD] == SENTINEL).all() and (b[PAD + n:] == SENTINEL).all()
        assert np.array_equal(b[PAD:PAD + n], w.view(np.uint32) if w.dtype != np.uint32 else w)
    with pytest.raises(ValueError, match="outside"):
        mesh_util.mesh_components(f, V)
    with pytest.raises(ValueError, match="outside"):
        mesh_util.filter_components(torch.zeros(V, 3, device=DEV), f, keep_largest=1)
    # the compaction never lets a bad face survive, whatever keep says
    src, out = check_compact(want[0], np.ones(V, dtype=np.uint8), faces, V)
    assert len(src) == V and len(out) == len(faces) - 2


# ---- compaction ----------------------------------------------------------------------------------------------------------------------------------

SELECTIONS = [dict(keep_largest=1), dict(keep_largest=2), dict(keep_largest=4), dict(keep_largest=5), dict(min_faces=9), dict(min_faces=17),
              dict(keep_largest=4, min_faces=17), dict(keep_largest=2, min_faces=9), dict(min_faces=10 ** 6), dict(keep_largest=10 ** 6), dict(min_faces=1)]


@pytest.mark.parametrize("name", ["noise_12", "noise_16x12x10", "noise_24", "noise_9x10x11_open", "three_spheres"])
def test_filtered_mesh_is_the_reference(name):
    from nerfart_amd import mesh_util
    V, faces, label, n_faces, info = mesh(name)
    verts = torch.arange(3 * V, dtype=torch.float32, device=DEV).reshape(V, 3)
    gfaces = dev(faces)
    closed = MESHES[name][5]
    for kw in SELECTIONS:
        src, out = ref.filter_components(V, faces, **kw)
        v2, f2, s2 = mesh_util.filter_components(verts, gfaces, **kw)
        assert s2.dtype == f2.dtype == torch.int32 and tuple(f2.shape) == out.shape and tuple(s2.shape) == src.shape and tuple(v2.shape) == (len(src), 3)
        assert np.array_equal(s2.cpu().numpy(), src) and np.array_equal(f2.cpu().numpy(), out), kw
        assert torch.equal(v2, verts[s2.long()])
        if kw in (dict(min_faces=10 ** 6),):
            assert tuple(f2.shape) == (0, 3) and tuple(v2.shape) == (0, 3) and tuple(s2.shape) == (0,)
        if kw in (dict(keep_largest=10 ** 6), dict(min_faces=1)):
            assert np.array_equal(src, np.arange(V)) and np.array_equal(f2.cpu().numpy(), faces)          # everything survives: the identity
        if closed and len(out):
            f2 = f2.cpu().numpy()
            assert mc_ref.is_closed(f2) and mc_ref.is_consistently_oriented(f2)
            dsrc, dout = ref.compact(label, 1 - ref.keep_mask(label, n_faces, **kw), faces, V)
            assert mc_ref.euler_characteristic(len(src), f2) + mc_ref.euler_characteristic(len(dsrc), dout) == mc_ref.euler_characteristic(V, faces)


def test_every_row_is_written_once_none_beyond_the_sizes_and_two_runs_agree():
    from nerfart_amd import hip
    V, faces, label, n_faces, _ = mesh("noise_24")
    keep = ref.keep_mask(label, n_faces, keep_largest=5, min_faces=9)
    src, out = ref.compact(label, keep, faces, V)
    Vo, Fo = len(src), len(out)
    assert 0 < Vo < V and 0 < Fo < len(faces)
    l, k, f = dev(label), dev(keep), dev(faces)
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(2):
        ws = torch.zeros(hip.mesh_compact_workspace_bytes(V, len(faces)), dtype=torch.uint8, device=DEV)      # zeroed: the padding between its buffers too
        ws, counts = hip.mesh_compact_count(l, k, f, V, ws=ws)
        assert counts.tolist() == [Vo, Fo]
        before = ws.clone()
        gs = torch.full((Vo + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
        gf = torch.full((3 * Fo + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
        assert hip.lib.nerfart_mesh_compact_emit(l.data_ptr(), k.data_ptr(), f.data_ptr(), V, len(faces), ws.data_ptr(), ws.numel(),
                                                 gs[PAD:].data_ptr(), gf[PAD:].data_ptr(), Vo, Fo, st) == 0
        assert torch.equal(ws, before)                      # emit runs from the untouched workspace
        gs, gf = gs.cpu().numpy(), gf.cpu().numpy()
        for b, w in ((gs, src), (gf, out.reshape(-1))):
            assert (b[:PAD].view(np.uint32) == SENTINEL).all() and (b[PAD + len(w):].view(np.uint32) == SENTINEL).all()
            assert np.array_equal(b[PAD:PAD + len(w)], w)   # every row written (no sentinel left: indices are < 2^31), with the reference's value
        runs.append((ws.cpu(), gs, gf))
        # arrays SHORTER than the counts: the rows that fit are written, nothing beyond them
        gs = torch.full((Vo + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
        gf = torch.full((3 * Fo + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
        assert hip.lib.nerfart_mesh_compact_emit(l.data_ptr(), k.data_ptr(), f.data_ptr(), V, len(faces), ws.data_ptr(), ws.numel(),
                                                 gs.data_ptr(), gf.data_ptr(), Vo - 7, Fo - 5, st) == 0
        gs, gf = gs.cpu().numpy(), gf.cpu().numpy()
        assert np.array_equal(gs[:Vo - 7], src[:-7]) and (gs[Vo - 7:].view(np.uint32) == SENTINEL).all()
        assert np.array_equal(gf[:3 * (Fo - 5)], out[:-5].reshape(-1)) and (gf[3 * (Fo - 5):].view(np.uint32) == SENTINEL).all()
    assert torch.equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


def test_every_depth_of_the_scan():
    """The compaction scans max(V, F) items in blocks of 512: one block, a level of block sums (noise_24 above), and - past 512 * 512 items - a
    second level.  270,000 vertices in strips of 1,000: 270 components of 998 faces, every third one kept."""
    from nerfart_amd import hip
    n = 270000
    i = np.arange(n - 2, dtype=np.int32)
    faces = np.stack([i, i + 1, i + 2], 1)[(i % 1000) < 998]
    assert n > 512 * 512 and len(faces) > 512 * 512
    got = gpu_components(faces, n)
    label = (np.arange(n, dtype=np.int32) // 1000) * 1000
    n_faces = np.zeros(n, dtype=np.uint32)
    n_faces[::1000] = 998
    assert np.array_equal(got[0], label) and np.array_equal(got[1], n_faces) and got[2].tolist() == [270, 270, 0]
    # the closed form is the reference's: checked on the first strips
    head = ref.components(faces[:4990], 5000)
    assert np.array_equal(head[0], label[:5000]) and np.array_equal(head[1], n_faces[:5000])
    keep = np.zeros(n, dtype=np.uint8)
    keep[::3000] = 1
    src, out = check_compact(label, keep, faces, n)
    assert len(src) == 90 * 1000 and len(out) == 90 * 998
    assert hip.mesh_compact_workspace_bytes(n, len(faces)) == sum((b + 255) // 256 * 256 for b in (8 * n, 8 * 528, 8 * 2))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------

def test_three_spheres_through_marching_cubes():
    from nerfart_amd import mesh_util
    verts, faces = mesh_util.marching_cubes(dev(ref.three_spheres()), 0.0)
    assert tuple(faces.shape) == (756, 3)
    for kw, want, spheres in ((dict(keep_largest=1), 524, 1), (dict(keep_largest=2), 724, 2), (dict(min_faces=33), 724, 2), (dict(keep_largest=3), 756, 3)):
        v2, f2, src = mesh_util.filter_components(verts, faces, **kw)
        assert f2.shape[0] == want and torch.equal(v2, verts[src.long()])
        f2 = f2.cpu().numpy()
        assert mc_ref.is_closed(f2) and mc_ref.is_consistently_oriented(f2) and mc_ref.euler_characteristic(len(src), f2) == 2 * spheres


@pytest.mark.parametrize("reference_shear", [False, True])
def test_extract_mesh_drops_the_floaters(reference_shear, tmp_path):
    """The plain native path, sheared grid included: the filtered file is the reference's filter of the unfiltered file, byte for byte."""
    from nerfart_amd import scene, mesh_util
    N, volume_size = 48, 3.0
    model, _, _ = scene.build_model("NeuS", seed=0, beta=None, device=DEV)
    surface = WithFloaters(model.implicit_surface)
    kw = dict(volume_size=volume_size, N=N, reference_shear=reference_shear)
    _, verts, faces, _ = mc_ref.read_ply(mesh_util.extract_mesh(surface, filepath=str(tmp_path / "all.ply"), **kw))
    label, n_faces, info = ref.components(faces, len(verts))
    roots, count = ref.ranked(label, n_faces)
    print(f"[components] shear = {reference_shear}: V = {len(verts)}, F = {len(faces)}, face counts {count.tolist()}")
    if not reference_shear:
        assert info.tolist() == [3, 3, 0] and count[0] > 500 and count[0] > count[1] >= count[2] > 0
    assert info[1] >= 2
    for name, opts in (("largest", dict(keep_largest=1)), ("two", dict(keep_largest=2)), ("min", dict(min_component_faces=int(count[1]))),
                       ("both", dict(keep_largest=2, min_component_faces=int(count[0])))):
        path = mesh_util.extract_mesh(surface, filepath=str(tmp_path / f"{name}.ply"), **kw, **opts)
        src, out = ref.filter_components(len(verts), faces, keep_largest=opts.get("keep_largest"), min_faces=opts.get("min_component_faces"))
        want = mesh_util.write_ply(str(tmp_path / f"{name}_ref.ply"), verts[src], out)
        assert open(path, "rb").read() == open(want, "rb").read(), name
        assert 0 < len(out) < len(faces)
        if not reference_shear:
            assert mc_ref.is_closed(out) and mc_ref.is_consistently_oriented(out)
    _, v1, f1, _ = mc_ref.read_ply(str(tmp_path / "largest.ply"))
    if not reference_shear:
        assert mc_ref.euler_characteristic(len(v1), f1) == 2 and mc_ref.signed_volume(v1, f1) > 0


def test_extract_mesh_with_vertex_data_filters_every_array_together(tmp_path):
    """The sphere-initialised NeuS model at N = 48 with refined vertices, normals and colours: every vertex row of the filtered file is the row
    src_vertex points to in the unfiltered file; a mesh of one component is written unchanged, byte for byte."""
    from nerfart_amd import scene, mesh_util
    N, volume_size = 48, 2.0
    model, _, _ = scene.build_model("NeuS", seed=0, beta=None, device=DEV)
    kw = dict(volume_size=volume_size, N=N, refine_evals=2, vertex_normals=True, color_model=model)
    a = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "all.ply"), **kw)
    b = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "largest.ply"), keep_largest=1, **kw)
    full, kept = mv.read_ply(a), mv.read_ply(b)
    assert kept["normals"] is not None and kept["colors"] is not None
    label, n_faces, info = ref.components(full["faces"], len(full["verts"]))
    src, out = ref.filter_components(len(full["verts"]), full["faces"], keep_largest=1)
    assert np.array_equal(kept["faces"], out) and len(out) > 1000
    for key in ("verts", "normals", "colors"):
        assert np.array_equal(mv.bits(kept[key]), mv.bits(full[key][src])), key
    assert mc_ref.is_closed(kept["faces"]) and mc_ref.is_consistently_oriented(kept["faces"])
    assert mc_ref.euler_characteristic(len(kept["verts"]), kept["faces"]) == 2
    print(f"[components] NeuS N = {N}: {int(info[0])} component(s), F = {len(full['faces'])} -> {len(out)}")
    if info[0] == 1:
        assert open(a, "rb").read() == open(b, "rb").read()
    # the plain path: a readable two-element file whose faces pass the predicates; one component: today's file
    p = mesh_util.extract_mesh(model.implicit_surface, volume_size=volume_size, N=N, filepath=str(tmp_path / "p.ply"), keep_largest=1)
    q = mesh_util.extract_mesh(model.implicit_surface, volume_size=volume_size, N=N, filepath=str(tmp_path / "q.ply"))
    _, pv, pf, _ = mc_ref.read_ply(p)
    _, qv, qf, _ = mc_ref.read_ply(q)
    assert mc_ref.is_closed(pf) and mc_ref.is_consistently_oriented(pf) and mc_ref.euler_characteristic(len(pv), pf) == 2
    psrc, pout = ref.filter_components(len(qv), qf, keep_largest=1)
    assert np.array_equal(pf, pout) and np.array_equal(mv.bits(pv), mv.bits(qv[psrc]))
    if ref.components(qf, len(qv))[2][0] == 1:
        assert open(p, "rb").read() == open(q, "rb").read()
    with pytest.raises(ValueError, match="native"):
        mesh_util.extract_mesh(model.implicit_surface, backend="skimage", keep_largest=1)
