"""tests/mesh_distance_ref.py - the numpy statement of csrc/mesh_distance.hip - held to second formulations on the CPU: the hashes in Python
integers, the point-face distance by Ericson's region classification and by dense barycentric sampling plus a bound, the vectorised ring search
by a literal walk over per-cell lists, and the properties a distance and a sampler must have.  Each injected bug breaks a check on some input.
Also what needs no GPU: the entry points' refusals, the Python front's, the tool's flags."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import mesh_distance_ref as ref
import mesh_simplify_ref as sr
from conftest import REPO

GRIDS = ((1, 1, 1), (2, 3, 5), (7, 7, 7), (32, 32, 32))
_CACHE = {}


def mesh(name):
    if name not in _CACHE:
        _CACHE[name] = {
            "sphere_24": lambda: ref.mc_mesh(sr.sphere_volume((24, 24, 24), (11.3, 11.6, 11.1), 8.7)),
            "shells_24": lambda: ref.mc_mesh(sr.shells_volume((24, 24, 24), (11.4, 11.6, 11.3), 3.3, 6.4, 9.6)),
            "plane_16": lambda: ref.mc_mesh(sr.plane_volume((16, 16, 16), (0.0, 0.0, 1.0), 0.0), 8.0),
            "sliver": ref.sliver_mesh,
            "degenerate": ref.degenerate_mesh,
        }[name]()
    return _CACHE[name]


def case(name):
    """(verts, faces, query points, the distance matrix), computed once and shared"""
    key = ("case", name)
    if key not in _CACHE:
        v, f = mesh(name)
        q = ref.query_points(v, f, seed=3)
        _CACHE[key] = (v, f, q, ref.distance_matrix(q, v, f))
    return _CACHE[key]


# ---- the hashes ----------------------------------------------------------------------------------------------------------------------------------

def _mix_int(x):
    x ^= x >> 16; x = x * 0x7feb352d & 0xffffffff; x ^= x >> 15; x = x * 0x846ca68b & 0xffffffff; x ^= x >> 16
    return x


def test_hashes_in_python_integers():
    for seed in (0, 1, 0xdeadbeef, 0xffffffff):
        for f in (0, 1, 511, 512, 0x7fffffff):
            key = _mix_int(_mix_int(seed) ^ _mix_int((f + 0x9e3779b9) & 0xffffffff))
            assert int(ref.face_key(seed, f)) == key
            assert float(ref.count_h(seed, f)) == _mix_int(key ^ 0x68e31da4) / 2.0 ** 32
            for j in (0, 1, 70000):
                s = _mix_int((key + 0x85ebca6b * (j + 1)) & 0xffffffff)
                u, v = ref.sample_uv(seed, f, j, reflect=False)
                assert (float(u), float(v)) == (_mix_int(s ^ 0xb5297a4d) / 2.0 ** 32, _mix_int(s ^ 0x1b56c4e9) / 2.0 ** 32)
    h = ref.count_h(7, np.arange(100000))
    assert 0.0 <= h.min() and h.max() < 1.0 and abs(h.mean() - 0.5) < 5 * np.sqrt(1 / 12 / 100000)


# ---- the distance: second formulations -----------------------------------------------------------------------------------------------------------

def ericson_d2(p, a, b, c):
    """Closest point on a proper triangle by the Voronoi regions of its features (Ericson, Real-Time Collision Detection, 5.1.5), scalar."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return ap @ ap
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return bp @ bp
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        q = a + d1 / (d1 - d3) * ab
        return (p - q) @ (p - q)
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return cp @ cp
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        q = a + d2 / (d2 - d6) * ac
        return (p - q) @ (p - q)
    va = d3 * d6 - d5 * d4
    if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        q = b + (d4 - d3) / ((d4 - d3) + (d5 - d6)) * (c - b)
        return (p - q) @ (p - q)
    den = 1.0 / (va + vb + vc)
    q = a + ab * (vb * den) + ac * (vc * den)
    return (p - q) @ (p - q)


def _second_formulations(name, D, n_points=40, n_faces=60):
    """The worst of |d_ref - d_ericson| / allowance over proper faces, and the lattice check on every face (degenerate ones included)."""
    v, f, q, _ = case(name)
    good = ref.good_faces(v, f)
    a, b, c = ref.corners(v, f, good)
    A = ref.allowance(q, v, f)["A"]
    rng = np.random.default_rng(5)
    pi, fi = rng.permutation(len(q))[:n_points], rng.permutation(len(f))[:n_faces]
    nn = ref.dot(ref.cross(b - a, c - a), ref.cross(b - a, c - a))
    worst = 0.0
    K = 48
    i, j = np.meshgrid(np.arange(K + 1), np.arange(K + 1), indexing="ij")
    keep = i + j <= K
    wu, wv = i[keep] / K, j[keep] / K
    for k in fi:
        if not good[k]:
            continue
        lattice = a[k] + wu[:, None] * (b[k] - a[k]) + wv[:, None] * (c[k] - a[k])
        L = np.sqrt(max(ref.dot(b[k] - a[k], b[k] - a[k]), ref.dot(c[k] - b[k], c[k] - b[k]), ref.dot(a[k] - c[k], a[k] - c[k])))
        for p_ in pi:
            p = q[p_].astype(np.float64)
            d = np.sqrt(D[p_, k])
            dl = np.sqrt(((lattice - p) ** 2).sum(1).min())
            assert dl - L / K - 1e-9 <= d <= dl + 1e-9 * max(dl, 1.0), (name, k, p_, d, dl)        # the lattice's minimum brackets the distance
            if nn[k] > 0.0 and ref.conditioning(v, f)[k] < 1e6:
                worst = max(worst, abs(d - np.sqrt(ericson_d2(p, a[k], b[k], c[k]))) / A[p_, k])
    return worst


@pytest.mark.parametrize("name", ["sphere_24", "plane_16", "sliver", "degenerate"])
def test_distance_is_ericsons_and_the_lattices(name):
    worst = _second_formulations(name, case(name)[3])
    print(f"[mesh_distance_ref] {name}: worst |d_ref - d_ericson| / (2 x 64 u kappa S) = {worst:.4f}")
    assert worst <= 1.0


def test_degenerate_faces_are_their_edges():
    v, f = ref.degenerate_mesh()
    D = ref.distance_matrix(np.array([[0.5, 0.5, 0.25], [5, 5, 5], [-1, 0.5, 1], [2.5, 2.5, 2.5]], dtype=np.float32), v, f)
    assert D[1, 3] == 3.0 and D[3, 3] == 0.0                          # the collinear face (4, 5, 6) is the segment (2,2,2) - (4,4,4)
    assert D[2, 4] == 0.0 and D[0, 4] == 1.5 ** 2 + 0.75 ** 2          # the single-point face
    assert D[0, 2] == 0.0                                             # (0, 0, 3): the segment (0,0,0) - (1,1,.5) passes through the point


def test_a_bad_face_is_no_candidate():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 5]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 7], [-1, 0, 1]], dtype=np.int32)
    assert ref.good_faces(v, f).tolist() == [True, False, False, False]
    d, face = ref.closest_brute(np.array([[0.2, 0.2, 2.0]], dtype=np.float32), v, f)
    assert d[0] == 2.0 and face[0] == 0
    d, face = ref.closest_brute(np.array([[0.2, 0.2, 2.0]], dtype=np.float32), v, f[1:], max_distance=7.0)
    assert d[0] == 7.0 and face[0] == -1                              # no good face: the clamp and -1
    d, face = ref.closest_brute(np.array([[0.2, 0.2, 2.0]], dtype=np.float32), v, f, max_distance=1.5)
    assert d[0] == 1.5 and face[0] == -1


# ---- the distance: properties --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["sphere_24", "shells_24", "sliver"])
def test_samples_of_a_mesh_are_at_distance_zero_and_inside_their_faces(name):
    v, f = mesh(name)
    area = ref.face_areas(v, f).sum()
    cnt = ref.sample_counts(v, f, 400.0 / area, seed=11)
    p, face = ref.sample_points(v, f, 11, cnt["n"])
    assert len(p) == cnt["total"] and abs(cnt["total"] - 400) < 5 * np.sqrt(len(f)) / 2
    D = ref.distance_matrix(p, v, f)
    scale = np.abs(v).max()
    assert np.sqrt(D.min(1)).max() <= np.sqrt(3) * 2.0 ** -24 * scale          # the float32 rounding of the point, nothing more
    assert np.sqrt(D[np.arange(len(p)), face]).max() <= np.sqrt(3) * 2.0 ** -24 * scale
    assert _outside_share(v, f, p, face) == 0.0


def _outside_share(v, f, p, face):
    """the share of samples whose barycentrics - solved back from the point - leave the triangle by more than the float32 rounding allows"""
    good = ref.good_faces(v, f)
    a, b, c = (x[face] for x in ref.corners(v, f, good))
    e1, e2, w = b - a, c - a, p.astype(np.float64) - a
    g11, g12, g22 = ref.dot(e1, e1), ref.dot(e1, e2), ref.dot(e2, e2)
    det = g11 * g22 - g12 * g12
    ok = det > 0
    u = (g22 * ref.dot(w, e1) - g12 * ref.dot(w, e2))[ok] / det[ok]
    vv = (g11 * ref.dot(w, e2) - g12 * ref.dot(w, e1))[ok] / det[ok]
    tol = 1e-3                                                        # slivers: a float32 ulp of the point is a visible step in (u, v)
    return float(np.mean((u < -tol) | (vv < -tol) | (u + vv > 1 + tol)))


def test_distance_to_a_plane_is_the_height():
    v, f = mesh("plane_16")                                           # the plane z = 8 over [0, 15]^2, vertices on grid points
    rng = np.random.default_rng(0)
    q = np.concatenate([rng.uniform(1, 14, size=(64, 2)), rng.uniform(-6, 22, size=(64, 1))], axis=1).astype(np.float32)
    d, _ = ref.closest_brute(q, v, f)
    assert np.array_equal(d, np.abs(q[:, 2].astype(np.float64) - 8.0))


def test_distance_to_a_sphere_is_within_the_chord_error():
    r, n_lat = 2.0, 24
    v, f = ref.uv_sphere(r, n_lat)
    sag = r * (1.0 - np.sqrt(1.0 - (np.pi / n_lat) ** 2))
    rng = np.random.default_rng(1)
    dirs = rng.normal(size=(96, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    for R in (0.5, 1.9, 2.5, 9.0):
        q = (dirs * R).astype(np.float32)
        Rq = np.linalg.norm(q.astype(np.float64), axis=1)
        d, _ = ref.closest_brute(q, v, f)
        if R > r:
            assert np.all(d >= Rq - r - 1e-6) and np.all(d <= Rq - r + sag + 1e-6)
        else:
            assert np.all(d >= r - sag - Rq - 1e-6) and np.all(d <= r - Rq + 1e-6)


# ---- sampling ------------------------------------------------------------------------------------------------------------------------------------

def test_counts_are_unbiased_over_seeds():
    """n_f = floor(rho a_f) + Bernoulli(frac(rho a_f)): over S seeds the sum of a face's counts deviates from S rho a_f by a sum of S centred
    Bernoulli draws, standard deviation <= sqrt(S) / 2.  Bound: 6 standard deviations per face (2836 faces: chance 6e-6 for a fair hash), and
    5 of the sqrt(S F) / 2 of the grand total."""
    v, f = mesh("sphere_24")
    S, rho = 256, 1.7
    area = ref.face_areas(v, f)
    tot = np.zeros(len(f))
    for seed in range(S):
        tot += ref.sample_counts(v, f, rho, seed)["n"]
    dev = tot - S * rho * area
    assert np.abs(dev).max() <= 6 * np.sqrt(S) / 2
    assert abs(dev.sum()) <= 5 * np.sqrt(S * len(f)) / 2
    frac = rho * area - np.floor(rho * area)
    assert abs((dev ** 2).mean() / (S * (frac * (1 - frac)).mean()) - 1.0) < 0.1        # and the variance is the binomial's: the draws are independent


def test_counts_by_hand():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [4, 0, 0], [np.inf, 0, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 9], [0, 1, 4], [2, 1, 0]], dtype=np.int32)
    assert ref.face_areas(v, f).tolist() == [2.0, 0.0, 0.0, 0.0, 2.0]
    c = ref.sample_counts(v, f, 10.25, seed=5)
    h = ref.count_h(5, np.arange(5))
    assert c["n"].tolist() == [20 + (h[0] >= 0.5), 0, 0, 0, 20 + (h[4] >= 0.5)] and c["bad"] == 2          # zero area: none by the rule
    assert c["off"].tolist() == [0, c["n"][0], c["n"][0], c["n"][0], c["n"][0]] and c["total"] == c["n"].sum()
    e = ref.sample_counts(v, f[:0], 10.0, seed=5)
    assert e["total"] == 0 and e["bad"] == 0 and len(e["off"]) == 0


# ---- the search ----------------------------------------------------------------------------------------------------------------------------------

def literal_search(points, verts, faces, grid, max_distance=np.inf):
    """The header's search as it reads: per-cell lists, rings of cells, the stop rule.  (dist, face, visited)"""
    par = ref.grid_params(verts, faces, grid)
    c0, c1, good = ref.face_cell_ranges(par, verts, faces)
    g = par["g"]
    cells = {}
    for k in np.nonzero(good)[0]:
        for x in range(c0[k, 0], c1[k, 0] + 1):
            for y in range(c0[k, 1], c1[k, 1] + 1):
                for z in range(c0[k, 2], c1[k, 2] + 1):
                    cells.setdefault((x, y, z), []).append(k)
    a, b, c = ref.corners(verts, faces, good)
    out = []
    for p in np.asarray(points, dtype=np.float32).astype(np.float64):
        cp = ref.axis_cells(par, p[None])[0]
        best, best_f, visited, r = np.inf, -1, 0, 0
        while True:
            for x in range(max(cp[0] - r, 0), min(cp[0] + r, g[0] - 1) + 1):
                for y in range(max(cp[1] - r, 0), min(cp[1] + r, g[1] - 1) + 1):
                    for z in range(max(cp[2] - r, 0), min(cp[2] + r, g[2] - 1) + 1):
                        if max(abs(x - cp[0]), abs(y - cp[1]), abs(z - cp[2])) != r:
                            continue
                        for k in cells.get((x, y, z), []):
                            visited += 1
                            d2 = ref.face_d2(p[None], a[k:k + 1], b[k:k + 1], c[k:k + 1])[0, 0]
                            if d2 < best or (d2 == best and k < best_f):
                                best, best_f = d2, k
            bound = ref.stop_bound(par, p[None], cp[None], r)[0]
            if min(np.sqrt(best), max_distance) < bound or not np.isfinite(bound):
                break
            r += 1
        d, face = ref.clamp_result(np.array([best]), np.array([best_f]), max_distance)
        out.append((d[0], face[0], visited))
    return tuple(np.array(x) for x in zip(*out))


def test_the_vectorised_search_is_the_literal_one():
    v, f = ref.uv_sphere(1.0, 6, 8, centre=(0.3, -0.2, 0.1))
    q = ref.query_points(v, f, seed=2, n_each=6)
    for grid, maxd in (((4, 5, 3), np.inf), ((4, 5, 3), 0.4), ((1, 1, 1), np.inf), ((9, 9, 9), np.inf)):
        s = ref.search(q, v, f, grid, max_distance=maxd)
        d, face, visited = literal_search(q, v, f, grid, max_distance=maxd)
        assert np.array_equal(s["dist"], d) and np.array_equal(s["face"], face) and np.array_equal(s["visited"], visited), (grid, maxd)


@pytest.mark.parametrize("name", ["sphere_24", "shells_24", "plane_16", "sliver", "degenerate"])
def test_the_search_finds_the_brute_force_minimum_on_every_grid(name):
    v, f, q, D = case(name)
    d, face = ref.closest_brute(q, v, f, D=D)
    for grid in GRIDS:
        s = ref.search(q, v, f, grid, D=D)
        assert np.array_equal(s["dist"], d) and np.array_equal(s["face"], face), grid
    s = ref.search(q, v, f, (32, 32, 32), D=D)
    if name in ("sphere_24", "shells_24"):
        near = d < 1.0
        total = ref.entries(s["par"], v, f)                           # what a search that visits everything tests
        assert near.sum() > 100 and s["within"][near].max() < 0.05 * total, "the stop rule prunes nothing: the GPU test's bound would be empty"
    md = float(np.median(d))
    dc, fc = ref.closest_brute(q, v, f, max_distance=md, D=D)
    s = ref.search(q, v, f, (7, 7, 7), max_distance=md, D=D)
    assert np.array_equal(s["dist"], dc) and np.array_equal(s["face"], fc) and (fc < 0).sum() > 0


def test_an_empty_mesh():
    q = np.zeros((3, 3), dtype=np.float32)
    for v, f in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), (np.zeros((2, 3), np.float32), np.array([[0, 1, 5]], np.int32))):
        s = ref.search(q, v, f, (7, 7, 7), max_distance=2.5)
        assert np.all(s["dist"] == 2.5) and np.all(s["face"] == -1) and np.all(s["visited"] == 0)
        assert np.all(np.isinf(ref.search(q, v, f, (7, 7, 7))["dist"]))


# ---- injected bugs -------------------------------------------------------------------------------------------------------------------------------

def test_a_missing_reflection_is_caught():
    v, f = mesh("sphere_24")
    cnt = ref.sample_counts(v, f, 400.0 / ref.face_areas(v, f).sum(), seed=11)
    p, face = ref.sample_points(v, f, 11, cnt["n"], reflect=False)
    assert _outside_share(v, f, p, face) > 0.3                         # half the unit square lies outside the triangle


@pytest.mark.parametrize("bug", [dict(drop_edge=0), dict(drop_edge=1), dict(drop_edge=2), dict(no_plane=True)])
def test_a_missing_term_is_caught(bug):
    caught = False
    for name in ("sphere_24", "degenerate"):
        v, f, q, _ = case(name)
        try:
            caught = caught or _second_formulations(name, ref.distance_matrix(q, v, f, **bug)) > 1.0
        except AssertionError:
            caught = True
    assert caught


def test_a_stop_rule_one_ring_early_is_caught():
    caught = 0
    for name in ("sphere_24", "shells_24"):
        v, f, q, D = case(name)
        d, _ = ref.closest_brute(q, v, f, D=D)
        for grid in GRIDS[1:]:
            caught += int(np.any(ref.search(q, v, f, grid, D=D, stop_early=1)["dist"] != d))
    assert caught >= 2


# ---- the host layer's reductions -----------------------------------------------------------------------------------------------------------------

def test_distance_dict_by_hand():
    d = ref.distance_dict([0.0, 3.0, 4.0, 1.0], [2.0, 2.0], threshold=2.0)
    assert d["a_to_b"] == {"n": 4, "mean": 2.0, "rms": np.sqrt(26 / 4), "max": 4.0, "within": 0.5} and d["b_to_a"]["within"] == 1.0
    assert d["chamfer"] == 2.0 and d["hausdorff"] == 4.0 and d["precision"] == 0.5 and d["recall"] == 1.0 and d["fscore"] == 2 * 0.5 / 1.5
    assert ref.distance_dict([1.0], [1.0])["fscore"] is None and ref.distance_dict([3.0], [3.0], threshold=1.0)["fscore"] == 0.0


# ---- without a GPU: refusals, argument errors, the tool's flags ---------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_before_any_launch():
    from nerfart_amd import hip
    lib, null, one = hip.lib, C.c_void_p(0), C.c_void_p(256)       # `one`: non-null, aligned, never dereferenced - the checks come first
    inf = float("inf")

    def err():
        return lib.nerfart_last_error().decode()

    assert lib.nerfart_mesh_sample_workspace_bytes(1 << 31) == 0 and "2^31" in err()
    # off [F][2], the block sums of 513 and of 512^2 + 1 faces, the totals [2]: each rounded up to 256 bytes
    r256 = lambda b: (b + 255) // 256 * 256
    assert lib.nerfart_mesh_sample_workspace_bytes(0) == r256(8) + 256 and lib.nerfart_mesh_sample_workspace_bytes(512) == 8 * 512 + 256
    assert lib.nerfart_mesh_sample_workspace_bytes(513) == r256(8 * 513) + r256(8 * 2) + 256
    assert lib.nerfart_mesh_sample_workspace_bytes(512 * 512 + 1) == r256(8 * (512 * 512 + 1)) + r256(8 * 513) + r256(8 * 2) + 256
    need = lib.nerfart_mesh_sample_workspace_bytes(200)
    count = lambda **kw: lib.nerfart_mesh_sample_count(*[kw.get(k, d) for k, d in (("verts", one), ("faces", one), ("V", 100), ("F", 200), ("density", 1.0),
                                                                                   ("seed", 0), ("ws", one), ("ws_bytes", need), ("info", one),
                                                                                   ("stream", null))])
    emit = lambda **kw: lib.nerfart_mesh_sample_emit(*[kw.get(k, d) for k, d in (("verts", one), ("faces", one), ("V", 100), ("F", 200), ("seed", 0),
                                                                                 ("ws", one), ("ws_bytes", need), ("points", one), ("face", one),
                                                                                 ("n", 10), ("stream", null))])
    for k in ("verts", "faces", "ws", "info"):
        assert count(**{k: null}) == 2 and "null" in err(), k
    for k in ("verts", "faces", "ws", "points", "face"):
        assert emit(**{k: null}) == 2 and "null" in err(), k
    for fn in (count, emit):
        assert fn(ws_bytes=need - 1) == 2 and "workspace" in err()
        assert fn(ws=C.c_void_p(264)) == 2 and "aligned" in err()
        assert fn(F=1 << 31) == 2 and "2^31" in err()
    assert count(info=C.c_void_p(260)) == 2 and "aligned" in err()
    for rho in (-1.0, inf, float("nan")):
        assert count(density=rho) == 2 and "density" in err()
    assert emit(n=1 << 31) == 2 and "2^31" in err()
    assert emit(F=0, faces=null, ws_bytes=lib.nerfart_mesh_sample_workspace_bytes(0)) == 2 and "without faces" in err()
    assert emit(n=0, points=null, face=null) == 0                  # no samples: nothing is launched

    assert lib.nerfart_mesh_grid_workspace_bytes(0, 4, 4) == 0 and "dimension" in err()
    assert lib.nerfart_mesh_grid_workspace_bytes(4, 4, 1025) == 0 and "dimension" in err()
    assert lib.nerfart_mesh_grid_workspace_bytes(512, 512, 128) == 0 and "2^24" in err()
    assert lib.nerfart_mesh_grid_workspace_bytes(256, 256, 256) > 16 * (1 << 24)
    # params, box [8], totals [2], entries, off [L][2], (no block sums for 105 cells), cnt [L], cur [L]
    gneed = lib.nerfart_mesh_grid_workspace_bytes(3, 5, 7)
    assert gneed == 4 * 256 + r256(8 * 105) + 2 * r256(4 * 105)
    gcount = lambda **kw: lib.nerfart_mesh_grid_count(*[kw.get(k, d) for k, d in (("verts", one), ("faces", one), ("V", 100), ("F", 200), ("gx", 3),
                                                                                  ("gy", 5), ("gz", 7), ("ws", one), ("ws_bytes", gneed), ("info", one),
                                                                                  ("stream", null))])
    gfill = lambda **kw: lib.nerfart_mesh_grid_fill(*[kw.get(k, d) for k, d in (("verts", one), ("faces", one), ("V", 100), ("F", 200), ("gx", 3),
                                                                                ("gy", 5), ("gz", 7), ("ws", one), ("ws_bytes", gneed), ("list", one),
                                                                                ("entries", 300), ("stream", null))])
    closest = lambda **kw: lib.nerfart_mesh_closest(*[kw.get(k, d) for k, d in (("points", one), ("n", 10), ("verts", one), ("faces", one), ("V", 100),
                                                                                ("F", 200), ("gx", 3), ("gy", 5), ("gz", 7), ("ws", one),
                                                                                ("ws_bytes", gneed), ("list", one), ("entries", 300),
                                                                                ("max_distance", inf), ("dist", one), ("face", one), ("visited", null),
                                                                                ("stream", null))])
    for k in ("verts", "faces", "ws", "info"):
        assert gcount(**{k: null}) == 2 and "null" in err(), k
    for k in ("verts", "faces", "ws", "list"):
        assert gfill(**{k: null}) == 2 and "null" in err(), k
    for k in ("points", "verts", "faces", "ws", "list", "dist", "face"):
        assert closest(**{k: null}) == 2 and "null" in err(), k
    for fn in (gcount, gfill, closest):
        assert fn(gx=0) == 2 and "dimension" in err()
        assert fn(gx=1024, gy=1024, gz=17) == 2 and "2^24" in err()
        assert fn(ws_bytes=gneed - 1) == 2 and "workspace" in err()
        assert fn(ws=C.c_void_p(264)) == 2 and "aligned" in err()
        assert fn(V=1 << 31) == 2 and "2^31" in err()
    assert gcount(info=C.c_void_p(260)) == 2 and "aligned" in err()
    for fn in (gfill, closest):
        assert fn(entries=1 << 31) == 2 and "2^31 entries" in err()
    for md in (-1.0, float("nan")):
        assert closest(max_distance=md) == 2 and "max_distance" in err()
    assert closest(n=1 << 31) == 2 and "2^31" in err()
    assert closest(n=0, points=null, dist=null, face=null) == 0 and gfill(entries=0, list=null) == 0        # nothing to do: nothing is launched


def test_python_front_refuses_by_name():
    import torch
    from nerfart_amd import mesh_util
    verts, faces, points = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(5, 3)
    with pytest.raises(ValueError, match="sample_surface: verts must be a tensor on the GPU"):
        mesh_util.sample_surface(verts, faces, n=10)
    with pytest.raises(ValueError, match="closest_on_mesh: verts must be a tensor on the GPU"):
        mesh_util.closest_on_mesh(points, verts, faces)
    with pytest.raises(ValueError, match="mesh_distance: verts_a must be a tensor on the GPU"):
        mesh_util.mesh_distance(verts, faces, verts, faces)
    with pytest.raises(ValueError, match="verts must be a tensor"):
        mesh_util.sample_surface(verts.numpy(), faces, n=10)
    assert mesh_util.default_distance_grid(0) == (1, 1, 1) and mesh_util.default_distance_grid(800) == (10, 10, 10)
    assert mesh_util.default_distance_grid(10 ** 7) == (256, 256, 256)


def test_the_tool_takes_its_flags():
    spec = importlib.util.spec_from_file_location("compare_mesh", os.path.join(REPO, "tools", "compare_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse(["--a", "x.ply", "--b", "y.obj"])
    assert (a.samples, a.threshold, a.max_distance, a.seed, a.heatmap) == (1 << 20, None, float("inf"), 0, None)
    a = tool.parse(["--a", "x.ply", "--b", "y.obj", "--samples", "1000", "--threshold", "0.01", "--max_distance", "0.5", "--seed", "3", "--heatmap", "h.ply"])
    assert (a.samples, a.threshold, a.max_distance, a.seed, a.heatmap) == (1000, 0.01, 0.5, 3, "h.ply")
    with pytest.raises(SystemExit):
        tool.parse(["--a", "x.ply"])
    import torch
    col = tool.heat_colors(torch.tensor([0.0, 1.0, 2.0, 3.0, 9.0]), 3.0)
    assert col.tolist() == [[0, 0, 0], [255, 0, 0], [255, 255, 0], [255, 255, 255], [255, 255, 255]]
    assert tool.finite({"a": float("inf"), "b": {"c": float("nan"), "d": 1.5}}) == {"a": None, "b": {"c": None, "d": 1.5}}
