"""csrc/mesh_distance.hip (mesh_util.sample_surface / closest_on_mesh / mesh_distance, tools/compare_mesh.py) against the numpy statement
tests/mesh_distance_ref.py, which tests/test_mesh_distance_ref.py holds to second formulations.  Integers - counts, offsets, face ids - and the
sample points are compared for equality; a distance must lie within the statement's allowance (half an fp32 ulp plus the fp64 term derived in
mesh_distance_ref.py) of the brute-force float64 minimum over ALL faces, and the reported face must attain it.  Every result must come out
bit-identical from a second call, from every grid, and leave the words around its arrays alone.

mesh_distance of a mesh with itself: the samples are float32 roundings of points of the surface, so "zero" is exact where the rounding stays on
the surface (the axis-aligned plane mesh: asserted == 0, F-score 1 at threshold 0) and the float32 rounding of the coordinates elsewhere
(the sphere: asserted <= sqrt(3) 2^-24 max|coordinate|).

Worst observed |dist - d_ref| / allowance (first GPU run, MI355X; the assertion is <= 1): 0.998 sphere_24, 0.999 shells_24, 0.959 plane_16, 0.973
sliver, 0.993 degenerate, 0.936 by_hand.  The allowance is almost all the half fp32 ulp (3.8e-6 .. 7.6e-6 against fp64 terms of 2e-12 .. 2e-8), so
a ratio just below 1 is a correctly rounded float32; the reported face was the statement's at every point, and `visited` on the 32^3 grid was
the statement's at every point."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_distance_ref as ref
import mesh_simplify_ref as sr
from conftest import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL_I, SENTINEL_F = 0x5a5a5a5a, -1.25e30
PAD = 4                      # words around every output (8-byte alignment of info is kept)
GRIDS = ((1, 1, 1), (2, 3, 5), (7, 7, 7), (32, 32, 32))


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)               # a copy: the shared reference arrays are read-only


def strip_mesh(F, seed):
    """F faces (i, i + 1, i + 2) over F + 2 random vertices: any F, areas of every size"""
    rng = np.random.default_rng(seed)
    verts = (rng.normal(size=(F + 2, 3)) * rng.choice([0.05, 1.0, 7.0], size=(F + 2, 1))).astype(np.float32)
    i = np.arange(F, dtype=np.int32)
    return verts, np.stack([i, i + 1, i + 2], axis=1)


def by_hand():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [4, 0, 0], [np.nan, 0, 0], [1, 1, 3]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 9], [0, 1, 4], [2, 1, 5], [-1, 0, 1]], dtype=np.int32)      # proper, zero area, bad index, NaN, proper, bad
    return v, f


MESHES = {
    "sphere_24": lambda: _mc(sr.sphere_volume((24, 24, 24), (11.3, 11.6, 11.1), 8.7)),
    "shells_24": lambda: _mc(sr.shells_volume((24, 24, 24), (11.4, 11.6, 11.3), 3.3, 6.4, 9.6)),
    "plane_16": lambda: _mc(sr.plane_volume((16, 16, 16), (0.0, 0.0, 1.0), 0.0), 8.0),
    "sliver": ref.sliver_mesh,
    "degenerate": ref.degenerate_mesh,
    "by_hand": by_hand,
    "F0": lambda: (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32)),
    "F1": lambda: (np.array([[0, 0, 0], [3, 0, 0], [0, 4, 1]], np.float32), np.array([[0, 1, 2]], np.int32)),
    "F511": lambda: strip_mesh(511, 1), "F512": lambda: strip_mesh(512, 2), "F513": lambda: strip_mesh(513, 3),
    "F262145": lambda: strip_mesh(512 * 512 + 1, 4),
}
# density and seed per sampling case: chosen so that the statement has no face within 2^-40 (relative) of an integer (asserted below)
SAMPLING = {"sphere_24": (3.0, 1), "shells_24": (1.5, 0xdeadbeef), "by_hand": (10.25, 5), "F0": (2.0, 0), "F1": (7.3, 9), "F511": (4.0, 2), "F512": (4.0, 3),
            "F513": (4.0, 4), "F262145": (0.02, 5), "sliver": (2.0e5, 6), "degenerate": (3.0, 7)}
_CACHE = {}


def _mc(vol, level=0.0):
    """mesh_util.marching_cubes' own mesh of the volume (grid coordinates), as numpy"""
    from nerfart_amd import mesh_util
    v, f = mesh_util.marching_cubes(dev(vol), level)
    return v.cpu().numpy(), f.cpu().numpy()


def mesh(name):
    """(verts, faces) as numpy and as GPU tensors; computed once, shared, never modified"""
    if name not in _CACHE:
        v, f = MESHES[name]()
        _CACHE[name] = (v, f, dev(v), dev(f))
    return _CACHE[name]


def guarded(n, dtype, cols=None):
    """(buffer, view): a sentinel-filled buffer with PAD words before and after the [n] or [n, cols] view handed to the library"""
    words = n * (cols or 1)
    buf = torch.full((words + 2 * PAD,), SENTINEL_F if dtype == torch.float32 else SENTINEL_I, dtype=dtype, device=DEV)
    view = buf[PAD:PAD + words]
    return buf, (view.view(n, cols) if cols else view)


def untouched(buf):
    fill = SENTINEL_F if buf.dtype == torch.float32 else SENTINEL_I
    return bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all())


# ---- sampling ------------------------------------------------------------------------------------------------------------------------------------

def sampled(name):
    """The statement's counts and the GPU's (offsets, info, points, face) for the case; computed once"""
    key = ("sampled", name)
    if key not in _CACHE:
        from nerfart_amd import hip
        v, f, gv, gf = mesh(name)
        rho, seed = SAMPLING[name]
        cnt = ref.sample_counts(v, f, rho, seed)
        ibuf, info = guarded(4, torch.int32)
        ws, _ = hip.mesh_sample_count(gv, gf, rho, seed, info=info)
        off = hip.mesh_sample_offsets(ws, len(f))
        n = int(info[0])
        pbuf, points = guarded(n, torch.float32, 3)
        fbuf, face = guarded(n, torch.int32)
        hip.mesh_sample_emit(gv, gf, seed, ws, n, points=points, face=face)
        _CACHE[key] = dict(cnt=cnt, ws=ws, info=info, off=off, n=n, points=points, face=face, bufs=(ibuf, pbuf, fbuf))
    return _CACHE[key]


@pytest.mark.parametrize("name", list(SAMPLING))
def test_sample_counts_and_offsets_are_the_statements(name):
    from nerfart_amd import hip
    v, f, gv, gf = mesh(name)
    rho, seed = SAMPLING[name]
    s = sampled(name)
    cnt = s["cnt"]
    assert np.all(cnt["margin"] > 2.0 ** -40), "the statement itself has a face inside the margin: choose another density or seed"
    info = s["info"].cpu().numpy()
    assert info.tolist() == [cnt["total"], cnt["bad"], 0, 0]
    assert np.array_equal(s["off"].cpu().numpy(), cnt["off"])
    got_n = np.diff(np.concatenate([s["off"].cpu().numpy().astype(np.int64), [s["n"]]])) if len(f) else np.zeros(0, dtype=np.int64)
    assert np.array_equal(got_n, cnt["n"])
    assert all(untouched(b) for b in s["bufs"])
    ws2, info2 = hip.mesh_sample_count(gv, gf, rho, seed)                    # a second call: the same bits
    assert torch.equal(info2, s["info"]) and torch.equal(hip.mesh_sample_offsets(ws2, len(f)), s["off"])
    if name == "by_hand":
        assert cnt["n"][1] == 0 and cnt["n"][2] == 0 and cnt["n"][3] == 0 and cnt["n"][5] == 0 and cnt["bad"] == 3
    if name.startswith("F") and len(f) > 1:
        assert cnt["total"] > len(f) / 4 and (cnt["n"] == 0).any() and (cnt["n"] > 1).any()


@pytest.mark.parametrize("name", list(SAMPLING))
def test_sample_points_are_the_statements_bit_for_bit(name):
    from nerfart_amd import hip
    v, f, gv, gf = mesh(name)
    _, seed = SAMPLING[name]
    s = sampled(name)
    p, face = ref.sample_points(v, f, seed, s["cnt"]["n"])
    assert s["points"].dtype == torch.float32 and s["face"].dtype == torch.int32
    assert np.array_equal(s["face"].cpu().numpy(), face)
    assert np.array_equal(s["points"].cpu().numpy().view(np.uint32), p.view(np.uint32))
    p2, f2 = hip.mesh_sample_emit(gv, gf, seed, s["ws"], s["n"])             # a second call: the same bits
    assert torch.equal(p2.view(torch.int32), s["points"].view(torch.int32)) and torch.equal(f2, s["face"])


def test_an_element_beyond_the_total_is_written_as_nothing():
    from nerfart_amd import hip
    v, f, gv, gf = mesh("F1")
    s = sampled("F1")
    p, face = hip.mesh_sample_emit(gv, gf, SAMPLING["F1"][1], s["ws"], s["n"] + 3)
    assert torch.equal(p[:s["n"]].view(torch.int32), s["points"].view(torch.int32)) and bool((p[s["n"]:] == 0).all()) and face[s["n"]:].tolist() == [-1] * 3


def test_too_many_samples_are_refused():
    """One face asking for 2^31 samples or more, and many faces whose 32-bit running sum wraps (every count below 2^31): both set the flag."""
    from nerfart_amd import hip, mesh_util
    v, f, gv, gf = mesh("F1")
    with pytest.raises(ValueError, match="2\\^31"):
        mesh_util.sample_surface(gv, gf, density=1e12)
    _, info = hip.mesh_sample_count(gv, gf, 1e12, 0)
    assert info.tolist()[2] == 1
    v, f, gv, gf = mesh("F513")
    area = ref.face_areas(v, f)
    rho = 0.9 * 2.0 ** 31 / area.max()
    assert (rho * area + 1).max() < 2.0 ** 31 and (rho * area).sum() > 2.0 ** 33
    _, info = hip.mesh_sample_count(gv, gf, rho, 0)
    assert info.tolist()[2] == 1
    with pytest.raises(ValueError, match="2\\^31"):
        mesh_util.sample_surface(gv, gf, density=rho)


# ---- closest point -------------------------------------------------------------------------------------------------------------------------------

CLOSEST = ("sphere_24", "shells_24", "plane_16", "sliver", "degenerate", "by_hand")


def queried(name):
    """The case's query points, the statement's distance matrix, brute-force answer and allowance, and the GPU's answer on the default grid"""
    key = ("queried", name)
    if key not in _CACHE:
        from nerfart_amd import mesh_util
        v, f, gv, gf = mesh(name)
        q = ref.query_points(v, f, seed=3)
        D = ref.distance_matrix(q, v, f)
        d, face = ref.closest_brute(q, v, f, D=D)
        gq = dev(q)
        gd, gface = mesh_util.closest_on_mesh(gq, gv, gf)
        _CACHE[key] = dict(q=q, gq=gq, D=D, d=d, face=face, allow=ref.allowance(q, v, f, D=D), gd=gd, gface=gface)
    return _CACHE[key]


@pytest.mark.parametrize("name", CLOSEST)
def test_distances_are_the_brute_force_minimum_within_the_allowance(name):
    c = queried(name)
    gd, gface = c["gd"].cpu().numpy().astype(np.float64), c["gface"].cpu().numpy()
    assert c["gd"].dtype == torch.float32 and c["gface"].dtype == torch.int32 and gd.shape == c["d"].shape
    allow = c["allow"]["allow"]
    err = np.abs(gd - c["d"])
    ratio = float(np.max(err / allow))
    print(f"[mesh_distance] {name}: {len(gd)} points; worst |dist - d_ref| / allowance = {ratio:.4f}; largest fp64 term {c['allow']['fp64'].max():.3e}, "
          f"largest half ulp {(allow - c['allow']['fp64']).max():.3e}; faces equal to the statement's: {(gface == c['face']).mean():.4f}")
    assert np.all(err <= allow)
    assert np.all(gface >= 0) and np.all(ref.good_faces(*mesh(name)[:2])[gface])
    attained = np.sqrt(c["D"][np.arange(len(gd)), gface])
    assert np.all(np.abs(attained - gd) <= allow), "the reported face does not attain the reported distance"
    if name == "plane_16":
        assert (gd == 0.0).sum() >= 48                                       # centroids, vertices and edge midpoints lie exactly on the mesh


@pytest.mark.parametrize("name", CLOSEST)
def test_every_grid_gives_the_same_bits(name):
    from nerfart_amd import mesh_util
    v, f, gv, gf = mesh(name)
    c = queried(name)
    for grid in GRIDS:
        d, face = mesh_util.closest_on_mesh(c["gq"], gv, gf, grid=grid)
        assert torch.equal(d.view(torch.int32), c["gd"].view(torch.int32)) and torch.equal(face, c["gface"]), grid
    d, face = mesh_util.closest_on_mesh(c["gq"], gv, gf)                      # a second call on the default grid
    assert torch.equal(d.view(torch.int32), c["gd"].view(torch.int32)) and torch.equal(face, c["gface"])


@pytest.mark.parametrize("name", ["sphere_24", "degenerate"])
def test_shuffled_faces_give_the_same_distances(name):
    from nerfart_amd import mesh_util
    v, f, gv, gf = mesh(name)
    c = queried(name)
    perm = np.random.default_rng(8).permutation(len(f))                      # new face i = old face perm[i]
    d, face = mesh_util.closest_on_mesh(c["gq"], gv, dev(f[perm]), grid=(7, 7, 7))
    assert torch.equal(d.view(torch.int32), c["gd"].view(torch.int32))
    old = perm[face.cpu().numpy()]
    same = old == c["gface"].cpu().numpy()
    # a tie between two faces (a point on a shared edge) goes to the lowest index, which the shuffle changes: the old face must then tie
    D = c["D"]
    assert np.all(D[np.arange(len(old)), old][~same] == D[np.arange(len(old)), c["gface"].cpu().numpy()][~same]) and same.mean() > 0.5


@pytest.mark.parametrize("name", ["sphere_24", "sliver"])
def test_max_distance_clamps_exactly_where_the_reference_exceeds_it(name):
    from nerfart_amd import hip, mesh_util
    v, f, gv, gf = mesh(name)
    c = queried(name)
    md = float(np.float32(np.median(c["d"]) * 1.01))
    assert np.all(np.abs(c["d"] - md) > c["allow"]["allow"]), "a point within the allowance of the clamp: choose another max_distance"
    beyond = c["d"] > md
    assert 0 < beyond.sum() < len(beyond)
    for grid in ((1, 1, 1), (7, 7, 7), (32, 32, 32)):
        d, face = mesh_util.closest_on_mesh(c["gq"], gv, gf, max_distance=md, grid=grid)
        d, face = d.cpu().numpy(), face.cpu().numpy()
        assert np.array_equal(face < 0, beyond) and np.all(d[beyond] == np.float32(md))
        assert np.array_equal(d[~beyond], c["gd"].cpu().numpy()[~beyond]) and np.array_equal(face[~beyond], c["gface"].cpu().numpy()[~beyond])
    g = hip.mesh_grid_build(gv, gf, (32, 32, 32))
    _, _, vis_inf = hip.mesh_closest(c["gq"], gv, gf, g, want_visited=True)
    _, _, vis_md = hip.mesh_closest(c["gq"], gv, gf, g, max_distance=md, want_visited=True)
    assert bool((vis_md <= vis_inf).all()) and int(vis_md.sum()) < int(vis_inf.sum())        # the bound ends far searches early


def test_an_empty_mesh_reports_the_clamp_and_no_face():
    from nerfart_amd import mesh_util
    q = dev(np.random.default_rng(0).normal(size=(70, 3)).astype(np.float32))
    for name in ("F0",):
        _, _, gv, gf = mesh(name)
        d, face = mesh_util.closest_on_mesh(q, gv, gf, max_distance=2.5)
        assert bool((d == 2.5).all()) and bool((face == -1).all())
        d, face = mesh_util.closest_on_mesh(q, gv, gf)
        assert bool(torch.isinf(d).all()) and bool((face == -1).all())
    bad = dev(np.array([[0, 1, 7], [0, 0, -1]], dtype=np.int32))             # faces, but no good one
    d, face = mesh_util.closest_on_mesh(q, mesh("F1")[2], bad, max_distance=0.5, grid=(7, 7, 7))
    assert bool((d == 0.5).all()) and bool((face == -1).all())
    d, face = mesh_util.closest_on_mesh(q[:0], *mesh("F1")[2:])              # and no points
    assert d.shape == (0,) and face.shape == (0,)


def test_a_non_finite_point_reports_nan_and_sentinels_stay():
    from nerfart_amd import hip
    v, f, gv, gf = mesh("sphere_24")
    q = queried("sphere_24")["gq"][:67].clone()
    q[5, 1] = float("nan")
    q[9, 0] = float("inf")
    g = hip.mesh_grid_build(gv, gf, (7, 7, 7))
    dbuf, d = guarded(67, torch.float32)
    fbuf, face = guarded(67, torch.int32)
    vbuf, vis = guarded(67, torch.int32)
    hip.mesh_closest(q, gv, gf, g, dist=d, face=face, visited=vis)
    assert untouched(dbuf) and untouched(fbuf) and untouched(vbuf)
    assert bool(torch.isnan(d[[5, 9]]).all()) and face[[5, 9]].tolist() == [-1, -1] and vis[[5, 9]].tolist() == [0, 0]
    keep = [i for i in range(67) if i not in (5, 9)]
    ref_d = queried("sphere_24")["gd"][:67]
    assert torch.equal(d[keep].view(torch.int32), ref_d[keep].view(torch.int32)) and bool((vis[keep] > 0).all())


@pytest.mark.parametrize("name", ["sphere_24", "shells_24"])
def test_pruning_visits_no_more_than_one_ring_beyond_the_statements_stop(name):
    from nerfart_amd import hip
    v, f, gv, gf = mesh(name)
    c = queried(name)
    s = ref.search(c["q"], v, f, (32, 32, 32), D=c["D"])
    g = hip.mesh_grid_build(gv, gf, (32, 32, 32))
    assert g.entries == ref.entries(s["par"], v, f) and g.good == s["par"]["good"]
    _, _, visited = hip.mesh_closest(c["gq"], gv, gf, g, want_visited=True)
    visited = visited.cpu().numpy()
    print(f"[mesh_distance] {name}: entries {g.entries}; visited mean {visited.mean():.1f} (statement {s['visited'].mean():.1f}, bound {s['within'].mean():.1f}); "
          f"equal to the statement's on {(visited == s['visited']).mean():.4f} of the points")
    assert np.all(visited <= s["within"])
    near = c["d"] < 1.0
    assert near.sum() > 100 and visited[near].max() < 0.05 * g.entries      # and that is far from everything


# ---- the host layer ------------------------------------------------------------------------------------------------------------------------------

def test_a_mesh_is_at_distance_zero_from_itself():
    from nerfart_amd import mesh_util
    _, _, gv, gf = mesh("plane_16")
    d = mesh_util.mesh_distance(gv, gf, gv, gf, samples=4000, threshold=0.0, seed=2)
    for side in ("a_to_b", "b_to_a"):
        assert d[side]["n"] > 3000 and d[side]["mean"] == 0.0 and d[side]["rms"] == 0.0 and d[side]["max"] == 0.0 and d[side]["within"] == 1.0
    assert d["chamfer"] == 0.0 and d["hausdorff"] == 0.0 and d["precision"] == 1.0 and d["recall"] == 1.0 and d["fscore"] == 1.0
    v, _, gv, gf = mesh("sphere_24")
    eps = float(np.sqrt(3) * 2.0 ** -24 * np.abs(v).max())                   # the float32 rounding of a sample's coordinates
    d = mesh_util.mesh_distance(gv, gf, gv, gf, samples=4000, threshold=eps, seed=2)
    assert d["hausdorff"] <= eps and d["fscore"] == 1.0 and d["a_to_b"] == d["b_to_a"]


def test_two_spheres_are_their_radius_difference_apart():
    from nerfart_amd import mesh_util
    r, delta, n_lat = 2.0, 0.25, 24
    va, fa = ref.uv_sphere(r, n_lat)
    vb, fb = ref.uv_sphere(r + delta, n_lat)
    sag_a, sag_b = (x * (1.0 - np.sqrt(1.0 - (np.pi / n_lat) ** 2)) for x in (r, r + delta))
    d = mesh_util.mesh_distance(dev(va), dev(fa), dev(vb), dev(fb), samples=5000, threshold=delta + sag_a, seed=1)
    for side in ("a_to_b", "b_to_a"):                                        # both meshes lie in their shells [R - sag, R]
        for k in ("mean", "rms", "max"):
            assert delta - sag_b - 1e-6 <= d[side][k] <= delta + sag_a + 1e-6, (side, k, d[side][k])
    assert d["fscore"] == 1.0 and abs(d["chamfer"] - delta) <= sag_b and abs(d["hausdorff"] - delta) <= sag_b


def test_the_dict_is_the_statements_on_the_same_per_sample_values():
    from nerfart_amd import mesh_util
    _, _, va, fa = mesh("sphere_24")
    _, _, vb, fb = mesh("shells_24")
    kw = dict(samples=3000, threshold=0.9, max_distance=2.0, seed=4)
    got = mesh_util.mesh_distance(va, fa, vb, fb, **kw)
    pa, _ = mesh_util.sample_surface(va, fa, n=3000, seed=4)
    pb, _ = mesh_util.sample_surface(vb, fb, n=3000, seed=4)
    d_ab, _ = mesh_util.closest_on_mesh(pa, vb, fb, 2.0)
    d_ba, f_ba = mesh_util.closest_on_mesh(pb, va, fa, 2.0)
    want = ref.distance_dict(d_ab.cpu().numpy(), d_ba.cpu().numpy(), threshold=0.9)
    assert bool((f_ba < 0).any()) and bool((d_ba[f_ba < 0] == 2.0).all())    # the inner shells are farther than max_distance from the sphere
    for side in ("a_to_b", "b_to_a"):
        assert got[side]["n"] == want[side]["n"]
        for k in ("mean", "rms", "max", "within"):
            assert abs(got[side][k] - want[side][k]) <= 1e-12 * abs(want[side][k]), (side, k)
    for k in ("chamfer", "hausdorff", "precision", "recall", "fscore"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    assert 0.0 < got["fscore"] < 1.0 and got["threshold"] == 0.9
    # n is the expectation of the count, and the samples are the statement's for the density the host computed
    v, f = mesh("sphere_24")[:2]
    cnt = ref.sample_counts(v, f, 3000 / float(ref.face_areas(v, f).sum()), 4)
    assert abs(int(pa.shape[0]) - 3000) <= 5 * np.sqrt(len(f)) / 2 and abs(int(pa.shape[0]) - cnt["total"]) <= 2


def test_wrong_device_or_dtype_is_refused_by_name():
    from nerfart_amd import mesh_util
    _, _, gv, gf = mesh("F1")
    q = dev(np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="verts must be torch.float32"):
        mesh_util.sample_surface(gv.double(), gf, n=10)
    with pytest.raises(ValueError, match="faces must be torch.int32"):
        mesh_util.closest_on_mesh(q, gv, gf.long())
    with pytest.raises(ValueError, match="points must be torch.float32"):
        mesh_util.closest_on_mesh(q.double(), gv, gf)
    with pytest.raises(ValueError, match="points must be a tensor on the GPU"):
        mesh_util.closest_on_mesh(q.cpu(), gv, gf)
    with pytest.raises(ValueError, match="faces_b must be a tensor on the GPU"):
        mesh_util.mesh_distance(gv, gf, gv, gf.cpu())
    with pytest.raises(ValueError, match="verts_a must be torch.float32"):
        mesh_util.mesh_distance(gv.half(), gf, gv, gf)
    with pytest.raises(ValueError, match=r"points must be \[n, 3\]"):
        mesh_util.closest_on_mesh(q[:, :2].contiguous(), gv, gf)
    with pytest.raises(ValueError, match="n or density"):
        mesh_util.sample_surface(gv, gf)
    with pytest.raises(ValueError, match="max_distance"):
        mesh_util.closest_on_mesh(q, gv, gf, max_distance=-1.0)


# ---- the tool ------------------------------------------------------------------------------------------------------------------------------------

def test_compare_mesh_end_to_end(tmp_path):
    from nerfart_amd import mesh_util
    va, fa = ref.uv_sphere(1.0, 8, 12)
    vb, fb = ref.uv_sphere(1.1, 8, 12, centre=(0.05, 0.0, 0.0))
    a, b, heat = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "heat.ply")
    mesh_util.write_ply(a, va, fa)
    mesh_util.write_ply(b, vb, fb)
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "compare_mesh.py"), "--a", a, "--b", b, "--samples", "2000", "--threshold", "0.12",
                          "--seed", "3", "--heatmap", heat], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["a"]["faces"] == len(fa) and out["b"]["vertices"] == len(vb) and out["max_distance"] is None and out["threshold"] == 0.12
    assert 0.0 < out["a_to_b"]["mean"] < 0.2 and out["a_to_b"]["mean"] <= out["a_to_b"]["rms"] <= out["a_to_b"]["max"] <= out["hausdorff"] < 0.3
    assert 0.0 < out["fscore"] <= 1.0 and out["a_to_b"]["n"] > 1500 and out["b_to_a"]["n"] > 1500
    m = mesh_util.read_ply(heat)
    assert m["verts"].shape == va.shape and m["faces"].shape == fa.shape and np.array_equal(m["faces"], fa) and m["colors"].shape == va.shape
    assert m["colors"].max() == 255 and out["heatmap_max"] > 0.1
