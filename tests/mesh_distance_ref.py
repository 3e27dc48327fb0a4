"""csrc/mesh_distance.hip in plain numpy - the statement tests/test_gpu_mesh_distance.py holds the kernels to, and tests/test_mesh_distance_ref.py
holds to a second formulation.  The rules are those of include/nerfart_hip.h ("distance between two meshes"):

  * the hashes in wrapping uint32 arithmetic;
  * areas, counts and sample points in float64 from the float32 vertices, every operation rounded once, in the header's order (numpy never
    fuses a multiply with an add);
  * the distance of a point to a face as the minimum of three clamped point-segment terms and, inside the prism of a non-degenerate face, the
    plane term; the result for a point is the lexicographic minimum of (d^2, face) over ALL good faces - brute force, no grid;
  * the grid, its conservative face lists and the ring search with its stop rule, formulated through "the ring at which a face is first
    visited" (the Chebyshev distance from the point's cell to the face's range of cells), so that it vectorises over points x faces.

THE ALLOWANCE for an fp64 implementation of the same formulas whose result is rounded to fp32 (`allowance`).  u = 2^-53.  For a point p and a
face f let S = 2 max(|p - a|, |p - b|, |p - c|) (it bounds every vector of the computation, edges included) and kappa = Lmax^2 / (2 area) =
longest edge over smallest altitude (kappa = 1 where the computed n . n is 0: the plane term is then not used).
  - A segment term: w and e carry one rounding per component (<= u S each); t = (w . e) / (e . e) has an absolute error of <= 8 u |w| / |e|;
    q = w - t e therefore errs by <= (2 + 8 + 2) u S per component and d = |q| by <= 12 sqrt(3) u S < 22 u S.  No cancellation: d^2 is the square of
    a small vector, not the difference of two large numbers.
  - The plane term: every component of n = e1 x e2 is two products and one difference of numbers of size |e1| |e2|, from inputs with one
    rounding each: |dn| <= 5 u |e1| |e2| = 5 u kappa' |n| with kappa' = |e1| |e2| / |n| <= kappa.  n . w adds 5 u |n| |w| of its own and |n| u S
    from w: d = |n . w| / |n| errs by <= u S (6 + 5 kappa') + d (5 kappa' + 6) u <= 22 u kappa S.
  - A sign of an edge function decided wrongly moves the point across an edge by at most the error of that function over |n| |e|, again
    <= 22 u kappa S; there the plane term and the edge's segment term differ by no more than that offset.
  So |computed d - exact d| <= 64 u kappa S =: A(p, f) with room to spare, for the statement and for the implementation alike: they differ by
  at most 2 A(p, f) on one face.  For the minimum over faces only the faces that can win count: those with d_ref(p, f) - 2 A(p, f) <=
  d_ref(p) + 2 A(p, f_ref).  The allowance is the largest 2 A over them, plus half an fp32 ulp of (d_ref + that).
"""
import numpy as np

U64 = 2.0 ** -53
C_OPS = 64.0
REL_SLACK = 1.0 - 2.0 ** -20
ABS_SLACK = 2.0 ** -30


# ---- the hashes ----------------------------------------------------------------------------------------------------------------------------------

def _u32(x):
    return np.atleast_1d(np.asarray(x).astype(np.uint32))           # arrays wrap silently; numpy warns about scalars


def mix(x):
    shape = np.shape(x)
    x = _u32(x).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x.reshape(shape)


def face_key(seed, f):
    return mix(mix(int(seed) & 0xffffffff) ^ mix((_u32(f) + np.uint32(0x9e3779b9)).reshape(np.shape(f))))


def count_h(seed, f):
    """h(seed, f) in [0, 1), float64, exact"""
    return mix(face_key(seed, f) ^ np.uint32(0x68e31da4)).astype(np.float64) * 2.0 ** -32


def sample_uv(seed, f, j, reflect=True):
    shape = np.broadcast(np.asarray(f), np.asarray(j)).shape
    s = mix((_u32(face_key(seed, f)) + np.uint32(0x85ebca6b) * (_u32(j) + np.uint32(1))).reshape(shape))
    u = mix(s ^ np.uint32(0xb5297a4d)).astype(np.float64) * 2.0 ** -32
    v = mix(s ^ np.uint32(0x1b56c4e9)).astype(np.float64) * 2.0 ** -32
    if reflect:
        out = u + v > 1.0
        u, v = np.where(out, 1.0 - u, u), np.where(out, 1.0 - v, v)
    return u, v


# ---- the mesh ------------------------------------------------------------------------------------------------------------------------------------

def good_faces(verts, faces):
    """[F] bool: every index in [0, V) and every coordinate finite"""
    verts, faces = np.asarray(verts), np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V = len(verts)
    ok = np.all((faces >= 0) & (faces < V), axis=1)
    fin = np.ones(len(faces), dtype=bool)
    if V:
        fin[ok] = np.all(np.isfinite(verts[faces[ok]].reshape(-1, 9)), axis=1)
    return ok & fin


def corners(verts, faces, good):
    """a, b, c [F, 3] float64 from the float32 vertices (zeros for a bad face)"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.where(good[:, None], np.asarray(faces).reshape(-1, 3), 0).astype(np.int64)
    if len(v) == 0:
        z = np.zeros((len(f), 3))
        return z, z.copy(), z.copy()
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def face_areas(verts, faces):
    """[F] float64 in the header's order; 0 for a bad face"""
    good = good_faces(verts, faces)
    a, b, c = corners(verts, faces, good)
    n = cross(b - a, c - a)
    return np.where(good, 0.5 * np.sqrt(dot(n, n)), 0.0)


# ---- sampling ------------------------------------------------------------------------------------------------------------------------------------

def sample_counts(verts, faces, density, seed):
    """dict: x [F] = density a_f + h, n [F] int64, off [F] int64 (exclusive scan), total, bad (number of bad faces), margin [F] = the relative
    distance of x from the nearest integer (inf for a bad face): a face with margin <= 2^-40 may legitimately get a different count from an
    implementation whose square root differs in the last bit."""
    faces = np.asarray(faces).reshape(-1, 3)
    F = len(faces)
    good = good_faces(verts, faces)
    x = float(density) * face_areas(verts, faces) + count_h(seed, np.arange(F))
    n = np.where(good, np.floor(x), 0).astype(np.int64)
    assert np.all(x < 2.0 ** 31)
    margin = np.where(good, np.abs(x - np.round(x)) / np.maximum(np.abs(x), 1.0), np.inf)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) if F else np.zeros(0, dtype=np.int64)
    return {"x": x, "n": n, "off": off, "total": int(n.sum()), "bad": int((~good).sum()), "margin": margin}


def sample_points(verts, faces, seed, n, reflect=True):
    """(points [N, 3] float32, face [N] int32) for the per-face counts n [F]"""
    faces = np.asarray(faces).reshape(-1, 3)
    n = np.asarray(n, dtype=np.int64)
    face = np.repeat(np.arange(len(faces)), n)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]) if len(n) else np.zeros(0, dtype=np.int64)
    j = np.arange(len(face)) - off[face] if len(face) else np.zeros(0, dtype=np.int64)
    good = good_faces(verts, faces)
    a, b, c = corners(verts, faces, good)
    a, b, c = a[face], b[face], c[face]
    u, v = sample_uv(seed, face, j, reflect)
    p = (a + u[:, None] * (b - a)) + v[:, None] * (c - a)
    return p.astype(np.float32), face.astype(np.int32)


# ---- the narrow phase ----------------------------------------------------------------------------------------------------------------------------

def segment_d2(w, e):
    ee = dot(e, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0.0, np.clip(dot(w, e) / np.where(ee > 0.0, ee, 1.0), 0.0, 1.0), 0.0)
    q = w - t[..., None] * e
    return dot(q, q)


def face_d2(p, a, b, c, drop_edge=None, no_plane=False):
    """[P, F] float64: squared distance of every point to every face (broadcast p [P, 1, 3] against a, b, c [F, 3]).  drop_edge / no_plane
    inject bugs for the tests."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 1, 3)
    a, b, c = a[None], b[None], c[None]
    terms = [segment_d2(p - a, b - a), segment_d2(p - b, c - b), segment_d2(p - c, a - c)]
    if drop_edge is not None:
        terms.pop(drop_edge)
    d2 = np.minimum.reduce(terms)
    if no_plane:
        return d2
    n = cross(b - a, c - a)
    nn = dot(n, n)
    e0 = dot(n, cross(b - a, p - a))
    e1 = dot(n, cross(c - b, p - b))
    e2 = dot(n, cross(a - c, p - c))
    inside = (nn > 0.0) & (e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)
    h = dot(n, p - a)
    plane = h * h / np.where(nn > 0.0, nn, 1.0)
    return np.where(inside, np.minimum(d2, plane), d2)


def distance_matrix(points, verts, faces, **bugs):
    """[P, F] float64 d^2, +inf in the columns of bad faces"""
    good = good_faces(verts, faces)
    a, b, c = corners(verts, faces, good)
    points = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    D = np.empty((len(points), len(good)))
    for s in range(0, len(points), 256):                                        # chunks keep the [P, F, 3] temporaries small
        D[s:s + 256] = face_d2(points[s:s + 256], a, b, c, **bugs)
    D[:, ~good] = np.inf
    return D


def lexmin(D):
    """(d2 [P], face [P]): the minimum and its lowest index; (inf, -1) without a finite entry"""
    if D.shape[1] == 0:
        return np.full(D.shape[0], np.inf), np.full(D.shape[0], -1, dtype=np.int64)
    f = np.argmin(D, axis=1)                                                    # the first occurrence of the minimum
    d2 = D[np.arange(D.shape[0]), f]
    return d2, np.where(np.isfinite(d2), f, -1)


def clamp_result(d2, face, max_distance):
    """(dist float64 [P], face): the header's max_distance rule"""
    d = np.sqrt(d2)
    found = (face >= 0) & (d <= max_distance)
    return np.where(found, d, max_distance), np.where(found, face, -1)


def closest_brute(points, verts, faces, max_distance=np.inf, D=None):
    D = distance_matrix(points, verts, faces) if D is None else D
    return clamp_result(*lexmin(D), max_distance)


def conditioning(verts, faces):
    """kappa [F]: longest edge^2 / (2 area) where n . n > 0 as computed, 1 elsewhere (and for bad faces)"""
    good = good_faces(verts, faces)
    a, b, c = corners(verts, faces, good)
    n = cross(b - a, c - a)
    nn = dot(n, n)
    L2 = np.maximum(np.maximum(dot(b - a, b - a), dot(c - b, c - b)), dot(a - c, a - c))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(nn > 0.0, L2 / np.sqrt(np.where(nn > 0.0, nn, 1.0)), 1.0)
    return np.maximum(k, 1.0)


def allowance(points, verts, faces, D=None):
    """dict: allow [P] (float64: what |float32 dist - d_ref| may be), fp64 [P] (its fp64 part), A [P, F] (2 x 64 u kappa S per point and face)."""
    D = distance_matrix(points, verts, faces) if D is None else D
    good = good_faces(verts, faces)
    a, b, c = corners(verts, faces, good)
    p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 1, 3)
    S = 2.0 * np.sqrt(np.maximum(np.maximum(dot(p - a[None], p - a[None]), dot(p - b[None], p - b[None])), dot(p - c[None], p - c[None])))
    A = 2.0 * C_OPS * U64 * conditioning(verts, faces)[None, :] * S
    d2, f = lexmin(D)
    d = np.sqrt(d2)
    P = len(d)
    fp = np.zeros(P)
    has = f >= 0
    if has.any():
        Af = A[np.arange(P), np.maximum(f, 0)]
        can_win = (np.sqrt(D) - A <= (d + Af)[:, None]) & good[None, :]
        fp = np.where(has, np.max(np.where(can_win, A, 0.0), axis=1), 0.0)
    with np.errstate(invalid="ignore"):
        ulp = np.spacing((np.where(has, d, 0.0) + fp).astype(np.float32)).astype(np.float64)
    return {"allow": 0.5 * ulp + fp, "fp64": fp, "A": A}


# ---- the grid and the search ---------------------------------------------------------------------------------------------------------------------

def grid_params(verts, faces, grid):
    """dict lo, s, inv [3] float64, g [3] int (the cells in use), m (the largest |coordinate| of the box), good (count)"""
    good = good_faces(verts, faces)
    a, b, c = corners(verts, faces, good)
    g = np.array(grid, dtype=np.int64)
    if not good.any():
        return {"lo": np.zeros(3), "s": np.zeros(3), "inv": np.zeros(3), "g": np.ones(3, dtype=np.int64), "m": 0.0, "good": 0}
    pts = np.concatenate([a[good], b[good], c[good]])
    lo, hi = pts.min(0), pts.max(0)
    ext = hi - lo
    flat = ~(ext > 0.0)
    safe = np.where(flat, 1.0, ext)
    return {"lo": lo, "s": np.where(flat, 0.0, safe / g), "inv": np.where(flat, 0.0, g / safe), "g": np.where(flat, 1, g),
            "m": float(max(np.abs(lo).max(), np.abs(hi).max())), "good": int(good.sum())}


def axis_cells(par, x):
    """x [..., 3] float64 -> cells [..., 3] int64"""
    t = np.floor((x - par["lo"]) * par["inv"])
    return np.clip(np.nan_to_num(t, nan=0.0), 0, par["g"] - 1).astype(np.int64)


def face_cell_ranges(par, verts, faces):
    """(c0, c1 [F, 3], good [F]): the cells each good face's box overlaps"""
    good = good_faces(verts, faces)
    a, b, c = corners(verts, faces, good)
    return axis_cells(par, np.minimum(np.minimum(a, b), c)), axis_cells(par, np.maximum(np.maximum(a, b), c)), good


def entries(par, verts, faces):
    c0, c1, good = face_cell_ranges(par, verts, faces)
    return int(np.prod(c1 - c0 + 1, axis=1)[good].sum())


def stop_bound(par, p, c, r):
    """B' [P] after ring r [P] (or a scalar) around the cells c [P, 3] of the points p [P, 3]"""
    r = np.broadcast_to(np.asarray(r, dtype=np.int64), c.shape[:1])[:, None]
    lower = p - (par["lo"] + (c - r) * par["s"])
    upper = (par["lo"] + (c + r + 1) * par["s"]) - p
    b = np.minimum(np.where(c - r > 0, lower, np.inf).min(1), np.where(c + r < par["g"] - 1, upper, np.inf).min(1))
    slack = ABS_SLACK * par["m"] + ABS_SLACK * np.abs(p).max(1)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(b), np.maximum(b * REL_SLACK - slack, 0.0), np.inf)


def search(points, verts, faces, grid, max_distance=np.inf, D=None, stop_early=0):
    """The ring search, vectorised: dict of dist, face (the header's outputs, float64 dist), ring [P] (the ring after which the search stops),
    visited [P] (faces tested, with repetition), within [P] (entries of the cells within ring + 1: the bound the pruning test holds the
    kernel's `visited` to).  stop_early = 1 injects the bug of judging ring r by the bound of ring r + 1."""
    D = distance_matrix(points, verts, faces) if D is None else D
    par = grid_params(verts, faces, grid)
    p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    P = len(p)
    c0, c1, good = face_cell_ranges(par, verts, faces)
    c = axis_cells(par, p)
    first = np.maximum(np.maximum(c0[None] - c[:, None], c[:, None] - c1[None]), 0).max(2)         # [P, F]: the ring that first visits the face
    first = np.where(good[None], first, np.iinfo(np.int64).max)
    R = np.maximum(c, par["g"] - 1 - c).max(1)

    def box_entries(r):                                                          # (face, cell) pairs inside [c - r, c + r]
        lo = np.maximum(c0[None], (c - r[:, None])[:, None])
        hi = np.minimum(c1[None], (c + r[:, None])[:, None])
        return (np.prod(np.maximum(hi - lo + 1, 0), axis=2) * good[None]).sum(1)

    ring = R.copy()
    best = np.full(P, np.inf)
    best_f = np.full(P, -1, dtype=np.int64)
    done = np.zeros(P, dtype=bool)
    for r in range(int(R.max()) + 1 if P else 0):
        d2, f = lexmin(np.where(first <= r, D, np.inf))
        b = stop_bound(par, p, c, r + stop_early)
        stop = ~done & ((np.minimum(np.sqrt(d2), max_distance) < b) | (r >= R))
        best[stop], best_f[stop], ring[stop] = d2[stop], f[stop], r
        done |= stop
    dist, face = clamp_result(best, best_f, max_distance)
    return {"dist": dist, "face": face, "ring": ring, "visited": box_entries(ring), "within": box_entries(ring + 1), "par": par}


# ---- the host layer's reductions -----------------------------------------------------------------------------------------------------------------

def direction_stats(d, threshold=None):
    d = np.asarray(d, dtype=np.float64)
    if len(d) == 0:
        return {"n": 0, "mean": 0.0, "rms": 0.0, "max": 0.0, "within": None if threshold is None else 0.0}
    return {"n": int(len(d)), "mean": float(d.mean()), "rms": float(np.sqrt((d * d).mean())), "max": float(d.max()),
            "within": None if threshold is None else float((d <= threshold).mean())}


def distance_dict(d_ab, d_ba, threshold=None):
    ab, ba = direction_stats(d_ab, threshold), direction_stats(d_ba, threshold)
    out = {"a_to_b": ab, "b_to_a": ba, "chamfer": 0.5 * (ab["mean"] + ba["mean"]), "hausdorff": max(ab["max"], ba["max"]), "threshold": threshold,
           "precision": ab["within"], "recall": ba["within"], "fscore": None}
    if threshold is not None:
        s = ab["within"] + ba["within"]
        out["fscore"] = 2.0 * ab["within"] * ba["within"] / s if s > 0.0 else 0.0
    return out


# ---- meshes the tests share ----------------------------------------------------------------------------------------------------------------------

def sliver_mesh(aspect=1e4, n=24):
    """A strip of n triangles of base 1 and height 1 / aspect, zig-zagging along x, slightly tilted out of the plane z = 0."""
    h = 1.0 / aspect
    x = np.arange(n + 2, dtype=np.float64) * 0.5
    y = np.where(np.arange(n + 2) % 2 == 0, 0.0, h)
    verts = np.stack([x, y, 0.05 * x], axis=1).astype(np.float32)
    faces = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], axis=1).astype(np.int32)
    return verts, faces


def degenerate_mesh():
    """Two proper faces, a face with a repeated vertex, three collinear vertices, and a face that is a single point."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 2, 2], [3, 3, 3], [4, 4, 4], [-1, 0.5, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [1, 3, 2], [0, 0, 3], [4, 5, 6], [7, 7, 7]], dtype=np.int32)
    return verts, faces


def uv_sphere(radius, n_lat=24, n_lon=48, centre=(0.0, 0.0, 0.0)):
    """A latitude / longitude sphere mesh, vertices exactly (to float32) on the sphere; the chord error of a face is at most
    radius (1 - cos(pi / n_lat)) (the faces' circumradius is below radius pi / n_lat)."""
    th = np.linspace(0.0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0.0, 2.0 * np.pi, n_lon, endpoint=False)
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    body = np.stack([np.sin(T) * np.cos(Ph), np.sin(T) * np.sin(Ph), np.cos(T)], axis=-1).reshape(-1, 3)
    verts = np.concatenate([[[0, 0, 1.0]], body, [[0, 0, -1.0]]]) * radius + np.asarray(centre)
    idx = lambda i, j: 1 + i * n_lon + (j % n_lon)
    faces = []
    south = 1 + (n_lat - 1) * n_lon
    for j in range(n_lon):
        faces.append([0, idx(0, j), idx(0, j + 1)])
        faces.append([south, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)])
        for i in range(n_lat - 2):
            faces.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            faces.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
    return verts.astype(np.float32), np.array(faces, dtype=np.int32)


def mc_mesh(vol, level=0.0):
    """(verts float32, faces int32) of tests/mc_ref.py's marching cubes, in grid coordinates"""
    import mc_ref
    v, f = mc_ref.marching_cubes(vol, level)
    return v.astype(np.float32), f.astype(np.int32)


def query_points(verts, faces, seed=0, n_each=48):
    """float32 [P, 3]: points ON the mesh (centroids, rounded to float32), NEAR it (centroids moved along the normal by 1e-3 and 3e-2 of the
    box's diagonal, both ways), FAR from it (several diagonals away), OUTSIDE the box beyond each of its six sides, and exactly on vertices
    and on midpoints of edges (exactly on the edge where the midpoint is a float32, as on integer grids)."""
    rng = np.random.default_rng(seed)
    good = good_faces(verts, faces)
    a, b, c = corners(verts, faces, good)
    a, b, c = a[good], b[good], c[good]
    if len(a) == 0:
        return rng.normal(size=(n_each, 3)).astype(np.float32)
    pts = np.concatenate([a, b, c])
    lo, hi = pts.min(0), pts.max(0)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-3)
    pick = rng.permutation(len(a))[:n_each]
    cen = (a[pick] + b[pick] + c[pick]) / 3.0
    n = cross(b[pick] - a[pick], c[pick] - a[pick])
    n = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    near = np.concatenate([cen + s * diag * n for s in (1e-3, -1e-3, 3e-2, -3e-2)])
    far = 0.5 * (lo + hi) + diag * rng.uniform(2.0, 6.0, size=(n_each // 2, 1)) * _unit(rng.normal(size=(n_each // 2, 3)))
    outside = []
    for k in range(3):
        for side, s in ((lo, -1.0), (hi, 1.0)):
            q = rng.uniform(lo, hi, size=(4, 3))
            q[:, k] = side[k] + s * diag * np.array([1e-4, 0.05, 0.5, 1.5])
            outside.append(q)
    on_vertices = a[pick[:n_each // 2]]
    on_edges = np.concatenate([0.5 * (a[pick] + b[pick]), 0.5 * (b[pick] + c[pick])])[:n_each]
    return np.concatenate([cen, near, far] + outside + [on_vertices, on_edges]).astype(np.float32)


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)
