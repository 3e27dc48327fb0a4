"""csrc/mesh_simplify.hip (mesh_util.simplify_clusters / extract_mesh(simplify_factor=)) against the numpy statement tests/mesh_simplify_ref.py,
which tests/test_mesh_simplify_ref.py holds to a second formulation and whose error bound it shows not to be vacuous.  The meshes are
mesh_util.marching_cubes of analytic volumes.  Integers - cluster, V', F', faces' - are compared by equality; every position must lie within
the reference's per-cluster bound of the float64 position, inside its cluster's cell, and come out bit-identical from a second call.

Worst observed distance / bound (first GPU run, MI355X; the assertion is <= 1): 0.022 over the marching-cubes meshes (two_spheres_24_c4, a
distance of 3.8e-6 grid cells), 0.11 over everything (three by-hand vertices without a face: the bound is then the fp32 output rounding alone,
2.5e-7 grid cells).  The largest distance anywhere was 1.1e-5 grid cells.  The normals and colours extract_mesh writes for the new vertices
were vertex_attributes' bit for bit, not merely within 1 ulp."""
import numpy as np
import pytest
import torch

import mc_ref
import mesh_simplify_ref as ref
import mesh_vertices_ref as mv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)               # a copy: the shared reference arrays are read-only


# name -> (volume, level, factor); 25^3 for factor 3 and 16^3 for factor 3 leave the last lattice layer ragged
CASES = {
    "sphere_24_c2": (lambda: ref.sphere_volume((24, 24, 24), (11.3, 11.6, 11.1), 8.7), 0.0, 2),
    "sphere_24_c3": (lambda: ref.sphere_volume((24, 24, 24), (11.3, 11.6, 11.1), 8.7), 0.0, 3),
    "sphere_25_c3": (lambda: ref.sphere_volume((25, 25, 25), (12.2, 11.9, 12.4), 9.4), 0.0, 3),
    "two_spheres_24_c4": (lambda: ref.two_spheres_volume((24, 24, 24), (7.6, 12.0, 12.0), (16.9, 12.0, 12.0), 4.1), 0.0, 4),      # 1.1 cells apart
    "nested_shells_24_c4": (lambda: ref.shells_volume((24, 24, 24), (11.4, 11.6, 11.3), 5.3, 6.4, 7.6), 0.0, 4),                   # equal triples
    "axis_plane_16_c2": (lambda: ref.plane_volume((16, 16, 16), (1.0, 0.0, 0.0), 0.0), 8.0, 2),        # level 8: every vertex at (8, j, k)
    "axis_plane_16_c4": (lambda: ref.plane_volume((16, 16, 16), (0.0, 0.0, 1.0), 0.0), 8.0, 4),
    "tilted_plane_16_c3": (lambda: ref.plane_volume((16, 16, 16), (0.31, 0.52, 1.0), 12.83), 0.0, 3),
    "sphere_40_c2": (lambda: ref.sphere_volume((40, 40, 40), (19.3, 19.6, 19.1), 15.7), 0.0, 2),
}
_CACHE = {}


def case(name):
    """(verts [V, 3] float32 on the GPU, faces [F, 3] int32 on the GPU, shape, factor, the reference's dict, the GPU's three tensors): the mesh
    is mesh_util.marching_cubes' own; everything is computed once, shared, never modified."""
    if name not in _CACHE:
        from nerfart_amd import mesh_util
        make, level, c = CASES[name]
        vol = make()
        verts, faces = mesh_util.marching_cubes(dev(vol), level)
        r = ref.simplify(verts.cpu().numpy(), faces.cpu().numpy(), vol.shape, c)
        got = mesh_util.simplify_clusters(verts, faces, vol.shape, c)
        _CACHE[name] = (verts, faces, vol.shape, c, r, got)
    return _CACHE[name]


def check(verts, faces, shape, c, r, got, what):
    """Every assertion the issue lists per mesh; returns the worst distance / bound."""
    out_v, out_f, cluster = got
    assert out_v.dtype == torch.float32 and out_f.dtype == cluster.dtype == torch.int32
    assert out_v.device == out_f.device == cluster.device == verts.device
    assert not r["bad"]
    V2, F2 = r["verts"].shape[0], r["faces"].shape[0]
    assert tuple(out_v.shape) == (V2, 3) and tuple(out_f.shape) == (F2, 3) and tuple(cluster.shape) == (verts.shape[0],)
    assert np.array_equal(cluster.cpu().numpy(), r["cluster"]), "cluster"
    gf = out_f.cpu().numpy()
    assert np.array_equal(gf, r["faces"]), "faces"
    gv = out_v.cpu().numpy().astype(np.float64)
    ratio = 0.0
    if V2:
        dist = np.linalg.norm(gv - r["verts"], axis=1)
        ratio = float(np.max(dist / r["bound"]))
        print(f"[simplify] {what}: V = {verts.shape[0]}, F = {faces.shape[0]} -> V' = {V2}, F' = {F2}; worst distance / bound = {ratio:.4f} "
              f"(largest bound {r['bound'].max():.3e}, largest distance {dist.max():.3e} grid cells)")
        assert ratio <= 1.0
        lo = r["centre"] - 0.5 * c
        assert np.all(gv >= lo) and np.all(gv <= lo + c), "a vertex outside its cluster's cell"
    if F2:
        assert np.all(gf[:, 0] < gf[:, 1]) and np.all(gf[:, 0] < gf[:, 2]) and np.all(gf[:, 1] != gf[:, 2]), "a repeated index, or not rotated"
        assert len(np.unique(gf, axis=0)) == F2, "two faces equal as rotated triples"
        assert gf.min() >= 0 and gf.max() < V2
    return ratio


@pytest.mark.parametrize("name", list(CASES))
def test_clusters_faces_and_positions_are_the_reference(name):
    verts, faces, shape, c, r, got = case(name)
    check(verts, faces, shape, c, r, got, name)
    assert 0 < r["faces"].shape[0] < faces.shape[0] and r["verts"].shape[0] < verts.shape[0]
    assert r["bound"].max() < 0.05, "a cluster of a marching-cubes mesh fell back to the cell diagonal: the bound would say nothing there"
    if name.startswith("axis_plane"):
        v = verts.cpu().numpy()
        assert np.array_equal(v, np.round(v)), "the axis plane's vertices are meant to sit on grid points"
    if name == "nested_shells_24_c4":
        t = ref.rotate(r["cluster"][faces.cpu().numpy()])
        proper = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
        assert proper.sum() > r["faces"].shape[0] and not proper.all(), "this case is meant to hold duplicate and degenerate faces"
    if name == "sphere_40_c2":                   # both lanes of the pair scan go through its block-sum level: more than two blocks of 512 each
        assert np.prod(ref.lattice(shape, c)) >= 1024 and faces.shape[0] >= 1024 and r["verts"].shape[0] >= 512


@pytest.mark.parametrize("name", list(CASES))
def test_a_second_call_gives_the_same_bits(name):
    from nerfart_amd import mesh_util
    verts, faces, shape, c, r, got = case(name)
    again = mesh_util.simplify_clusters(verts, faces, shape, c)
    assert torch.equal(got[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(got[1], again[1]) and torch.equal(got[2], again[2])


@pytest.mark.parametrize("name", ["sphere_24_c2", "sphere_25_c3", "sphere_40_c2", "two_spheres_24_c4"])
def test_orientation_survives_signed_volumes_agree(name):
    verts, faces, shape, c, r, got = case(name)
    vin = ref.signed_volume(verts.cpu().numpy(), faces.cpu().numpy())
    vref = ref.signed_volume(r["verts"], r["faces"])
    vgpu = ref.signed_volume(got[0].cpu().numpy(), got[1].cpu().numpy())
    tol = ref.volume_bound(r["verts"], r["faces"], r["bound"])
    print(f"[simplify] {name}: signed volume in {vin:.3f}, reference {vref:.6f}, GPU {vgpu:.6f}, |difference| {abs(vgpu - vref):.3e} <= {tol:.3e}")
    assert abs(vgpu - vref) <= tol
    assert vin > 0 and vref > 0 and vgpu > 0


def test_regularisation_weight_is_a_parameter():
    from nerfart_amd import mesh_util
    verts, faces, shape, c, r, got = case("tilted_plane_16_c3")
    r2 = ref.simplify(verts.cpu().numpy(), faces.cpu().numpy(), shape, c, reg=0.3)
    got2 = mesh_util.simplify_clusters(verts, faces, shape, c, reg=0.3)
    check(verts, faces, shape, c, r2, got2, "tilted_plane_16_c3, reg = 0.3")
    assert not torch.equal(got[0], got2[0]) and torch.equal(got[1], got2[1])


def test_hand_made_meshes():
    from nerfart_amd import mesh_util
    shape = (8, 8, 8)
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    tri = np.array([[0.25, 0.25, 0.5], [1.5, 0.25, 0.5], [0.25, 1.5, 0.5]], np.float32)
    fan = np.array([[2.1, 2.2, 2.3], [3.9, 2.1, 2.5], [3.8, 3.9, 3.1], [2.2, 3.7, 3.9], [3.0, 3.0, 2.0]], np.float32)
    spread = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 2.5], [7.0, 7.0, 7.0]], np.float32)      # vertex 4 in no face
    meshes = {
        "empty": (none_v, none_f, (0, 0)),
        "vertices_without_faces": (tri, none_f, (1, 0)),
        "one_triangle_in_one_cluster": (tri, np.array([[0, 1, 2]], np.int32), (1, 0)),
        "all_faces_in_one_cluster": (fan, np.array([[4, 0, 1], [4, 1, 2], [4, 2, 3], [4, 3, 0]], np.int32), (1, 0)),
        # a tetrahedron over four clusters, every face twice (one copy rotated), one face reversed, one degenerate: 5 survivors, input order
        "duplicates_rotations_and_a_reversed_face": (spread, np.array([[0, 1, 2], [1, 2, 0], [0, 3, 1], [3, 1, 0], [0, 2, 3], [2, 1, 3], [1, 3, 2],
                                                                        [0, 2, 1], [0, 0, 1], [2, 3, 0]], np.int32), (5, 5)),
    }
    for name, (v, f, sizes) in meshes.items():
        r = ref.simplify(v, f, shape, 2)
        assert (r["verts"].shape[0], r["faces"].shape[0]) == sizes, name
        got = mesh_util.simplify_clusters(dev(v).reshape(-1, 3), dev(f).reshape(-1, 3), shape, 2)
        check(dev(v).reshape(-1, 3), dev(f).reshape(-1, 3), shape, 2, r, got, name)
    assert r["faces"].tolist() == [[0, 3, 2], [0, 1, 3], [0, 2, 1], [1, 2, 3], [0, 2, 3]]        # in the new numbering: cells ascending


def test_refusals_raise_and_nothing_faults():
    from nerfart_amd import hip, mesh_util
    verts, faces, shape, c, r, got = case("sphere_24_c2")
    bad_face = faces.clone()
    bad_face[faces.shape[0] // 2, 1] = verts.shape[0]                      # one past the end
    with pytest.raises(ValueError, match="face index"):
        mesh_util.simplify_clusters(verts, bad_face, shape, c)
    bad_face[faces.shape[0] // 2, 1] = -1
    with pytest.raises(ValueError, match="face index"):
        mesh_util.simplify_clusters(verts, bad_face, shape, c)
    for value in (float("nan"), float("inf"), -0.5, 23.001):              # not finite; outside [0, n - 1]
        bad_vert = verts.clone()
        bad_vert[verts.shape[0] // 3, 2] = value
        with pytest.raises(ValueError, match="not\\s+finite or not inside the grid"):
            mesh_util.simplify_clusters(bad_vert, faces, shape, c)
    long_edge = dev(np.array([[0.5, 0.5, 0.5], [23.0, 0.5, 0.5], [0.5, 23.0, 0.5]], np.float32))       # terms far above 2^6: the guard, not a wrap
    with pytest.raises(ValueError, match="guards"):
        mesh_util.simplify_clusters(long_edge, dev(np.array([[0, 1, 2]], np.int32)), shape, c)
    with pytest.raises(ValueError, match="factor"):
        mesh_util.simplify_clusters(verts, faces, shape, 1)
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.simplify_clusters(verts.cpu(), faces.cpu(), shape, c)
    with pytest.raises(hip.NerfartHipError, match="int32"):
        mesh_util.simplify_clusters(verts, faces.long(), shape, c)
    # the flagged runs wrote nothing they should not have: the same mesh still gives the same result
    again = mesh_util.simplify_clusters(verts, faces, shape, c)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]) and torch.equal(got[2], again[2])


# ---- extract_mesh end to end -----------------------------------------------------------------------------------------------------------------

N, VOLUME_SIZE = 48, 3.0


class _WithFloaters(torch.nn.Module):
    """The model's SDF with two small spheres far from the object united to it: the floaters of a fine-tuned field, made on purpose."""
    SPHERES = (((1.2, 1.2, 1.2), 0.15), ((-1.2, 1.1, -1.2), 0.1))

    def __init__(self, surface):
        super().__init__()
        self.surface = surface

    def forward(self, x):
        d = self.surface.forward(x)
        for c, r in self.SPHERES:
            d = torch.minimum(d, (x - torch.tensor(c, device=x.device)).norm(dim=-1) - r)
        return d


@pytest.fixture(scope="module")
def model():
    from nerfart_amd import scene
    return scene.build_model("VolSDF", seed=0, beta=0.01, device=DEV, precision="mixed")[0]


def by_hand(surface, factor, keep_largest=None):
    """(grid-coordinate representatives, faces', the unsimplified (V, F)): sdf_volume -> marching_cubes in grid coordinates -> filter -> simplify."""
    from nerfart_amd import mesh_util
    vol = mesh_util.sdf_volume(surface, VOLUME_SIZE, N)
    verts, faces = mesh_util.marching_cubes(vol, 0.0)
    sizes = (verts.shape[0], faces.shape[0])
    if keep_largest is not None:
        verts, faces, _ = mesh_util.filter_components(verts, faces, keep_largest)
    g, f, _ = mesh_util.simplify_clusters(verts, faces, vol.shape, factor)
    return g, f, sizes


def test_extract_mesh_default_is_untouched_and_simplify_matches_by_hand(model, tmp_path):
    from nerfart_amd import mesh_util
    kw = dict(volume_size=VOLUME_SIZE, N=N)
    a = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "a.ply"), **kw)
    b = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "b.ply"), simplify_factor=None, **kw)
    assert open(a, "rb").read() == open(b, "rb").read()
    s = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "s.ply"), simplify_factor=2, **kw)
    g, f, (V, F) = by_hand(model.implicit_surface, 2)
    got = mv.read_ply(s)
    print(f"[simplify] VolSDF N = {N}, factor 2: V = {V}, F = {F} -> V' = {g.shape[0]}, F' = {f.shape[0]}")
    assert f"element vertex {g.shape[0]}\n" in got["header"] and f"element face {f.shape[0]}\n" in got["header"]
    assert 0 < f.shape[0] < F and 0 < g.shape[0] < V and got["normals"] is None and got["colors"] is None
    want = mesh_util.write_ply(str(tmp_path / "s_ref.ply"), mesh_util.grid_to_frame(g, *mesh_util.placement_frame(N, VOLUME_SIZE)), f)
    assert open(s, "rb").read() == open(want, "rb").read()
    assert mc_ref.signed_volume(got["verts"], got["faces"]) > 0
    for bad in (dict(reference_shear=True), dict(backend="skimage")):
        with pytest.raises(ValueError, match="simplify_factor"):
            mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "no.ply"), simplify_factor=2, **kw, **bad)


def test_extract_mesh_queries_normals_and_colours_at_the_new_vertices(model, tmp_path):
    """Same kernels on the same points - the representatives in the model's frame, mesh_util.grid_to_frame of simplify_clusters' grid coordinates
    - in a batch of the same size: the file's normals and colours are vertex_attributes' EXACTLY (observed: bit for bit, not 1 ulp)."""
    from nerfart_amd import mesh_util
    s = mesh_util.extract_mesh(model.implicit_surface, volume_size=VOLUME_SIZE, N=N, filepath=str(tmp_path / "s.ply"), simplify_factor=2,
                               vertex_normals=True, color_model=model)
    g, f, _ = by_hand(model.implicit_surface, 2)
    got = mv.read_ply(s)
    normals, colors = mesh_util.vertex_attributes(model, mesh_util.grid_to_frame(g, *mesh_util.model_frame(N, VOLUME_SIZE)))
    placed = mesh_util.grid_to_frame(g, *mesh_util.placement_frame(N, VOLUME_SIZE))
    assert np.array_equal(got["faces"], f.cpu().numpy()) and np.array_equal(mv.bits(got["verts"]), mv.bits(placed.cpu().numpy()))
    assert np.array_equal(mv.bits(got["normals"]), mv.bits(normals.cpu().numpy())) and np.array_equal(got["colors"], colors.cpu().numpy())
    # the written positions carry the model-frame points: placement and model frame share the origin, so p_model = origin + (p - origin) (N / (N - 1))
    o = -VOLUME_SIZE / 2.0
    back = o + (got["verts"].astype(np.float64) - o) * (N / (N - 1.0))
    pts = mesh_util.grid_to_frame(g, *mesh_util.model_frame(N, VOLUME_SIZE)).cpu().numpy().astype(np.float64)
    assert np.abs(back - pts).max() <= 8 * 2.0 ** -24 * VOLUME_SIZE           # at most three fp32 roundings of numbers <= 3 on either route, and 2 %
    nn = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
    assert np.all(np.abs(nn - 1) < 1e-5)


def test_extract_mesh_drops_floaters_before_it_clusters(model, tmp_path):
    from nerfart_amd import mesh_util
    surface = _WithFloaters(model.implicit_surface)
    kw = dict(volume_size=VOLUME_SIZE, N=N, simplify_factor=2)
    s = mesh_util.extract_mesh(surface, filepath=str(tmp_path / "s.ply"), keep_largest=1, **kw)
    everything = mv.read_ply(mesh_util.extract_mesh(surface, filepath=str(tmp_path / "all.ply"), **kw))
    g, f, _ = by_hand(surface, 2, keep_largest=1)
    want = mesh_util.write_ply(str(tmp_path / "s_ref.ply"), mesh_util.grid_to_frame(g, *mesh_util.placement_frame(N, VOLUME_SIZE)), f)
    assert open(s, "rb").read() == open(want, "rb").read()
    assert 0 < f.shape[0] < len(everything["faces"]) and g.shape[0] < len(everything["verts"])          # the floaters were there, and went
