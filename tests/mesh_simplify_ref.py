"""The numpy statement of csrc/mesh_simplify.hip (mesh_util.simplify_clusters; the rules are in include/nerfart_hip.h), which
tests/test_gpu_mesh_simplify.py holds the kernels to and tests/test_mesh_simplify_ref.py holds to a second formulation.

Integers are exact: the cell of every vertex, the numbering of the occupied cells, the rotated triples, the surviving faces and their order.
Quadrics and the solve are float64, straight from the formulas - no fixed point.  `simplify` also returns, per cluster, a BOUND on the distance
between its float64 representative and the one an implementation gives that computes every term in fp32 and sums the terms in fixed point
(quantum Q, rounding to nearest or truncating), and solves in fp64.

THE ERROR MODEL.  u = 2^-24 (fp32 rounding to nearest: every operation gives its exact result times (1 + d), |d| <= u; an fma only removes a
rounding).  Inputs are fp32 grid coordinates, exact.  A face (a, b, c) in cluster frame k, cf = the factor:
    e1 = (b - a) / cf, e2 = (c - a) / cf        2 roundings per component (the subtraction, the division)
    n_i = e1_j e2_k - e1_k e2_j                 each product 2 + 2 + 1 = 5, the subtraction 1 more, relative to the MAJORANT
                                                N_i = |e1_j e2_k| + |e1_k e2_j| >= |n_i| (the two products may cancel): |dn_i| <= 6 u N_i
    A_ij term = n_i n_j                         6 + 6 + 1 = 13 roundings:                     |d| <= 13 u N_i N_j
    l_i = (a_i - centre_i) / cf                 2 roundings (the centre c (k + 1/2) is exact)
    d = (n_0 l_0 + n_1 l_1) + n_2 l_2           each product 6 + 2 + 1 = 9, two sums 2 more:  |d d| <= 11 u D, D = sum_j N_j |l_j|
    b_i term = n_i d                            6 + 11 + 1 = 18 roundings:                    |d| <= 18 u N_i D
    position term = l_i                         2 roundings:                                  |d| <= 2 u |l_i|
These are first-order counts; K_A, K_B, K_M below are one larger each, which pays for the higher-order terms ((1 + u)^18 - 1 < 18 u (1 + 2e-6))
and for what the formula of the bound leaves out: lambda is computed from the perturbed trace, d lambda <= reg dA, which enters like 1 % of dA.
Every term then loses at most one quantum on its way into the sum.  So, with S|.| the sums of the majorants, accumulated HERE and for every face
with indices in range (an implementation's fp32 normal can be non-zero where the float64 one is zero), and with nf / nv the contribution counts:
    dA_ij = K_A u S|A|_ij + Q nf        db_i = K_B u S|b|_i + Q nf        dm_i = (K_M u S|l|_i + Q nv) / nv
    bound_local = ||(A + lambda I)^-1||_2 (||db||_2 + ||dA||_F |x*| + lambda ||dm||_2)         x* the UNCLAMPED float64 minimiser
That is the first order.  With eps = ||(A + lambda I)^-1||_2 ||dA||_F < 1 the perturbed matrix is still invertible and the exact statement is
bound_local / (1 - eps) (a Neumann series), which is what is returned while eps < 1/2 (eps is 1e-3 or less on a marching-cubes mesh).
Clamping to the cell is non-expansive, so the bound survives it; both points are inside the cell, so sqrt(3) always holds, and it is what is
left when eps >= 1/2 or when tr(A) == 0 in float64 while majorants are not (an fp32 normal of rounding noise can then move the point anywhere
in the cell).  tr(A) == 0 and no majorant: x* = m, bound_local = ||dm||_2.
In grid units: bound = cf bound_local + 2^-24 ||g'||_2 + 1e-12 cf.  The second term is the rounding of the fp32 output coordinate itself (half an
ulp per component, no implementation that returns fp32 can be closer); the third is the fp64 solve, cond <= 1 + 3 / reg, times 2^-53, generously.
"""
import numpy as np

U = 2.0 ** -24
QUANTUM = 2.0 ** -40          # of csrc/mesh_simplify.hip
K_A, K_B, K_M = 14, 19, 3
SQRT3 = float(np.sqrt(3.0))


def lattice(shape, c):
    return tuple(-(-int(n) // int(c)) for n in shape)


def vertex_cells(verts, shape, c):
    """cell [V] int64: the linear lattice cell of every vertex ((kx ly + ky) lz + kz with k = min(floor(x), n - 1) // c), -1 for a vertex that is
    not finite or not inside [0, n - 1]^3."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    n = np.array(shape, dtype=np.int64)
    lx, ly, lz = lattice(shape, c)
    with np.errstate(invalid="ignore"):
        ok = np.all(np.isfinite(v) & (v >= 0) & (v <= (n - 1).astype(np.float32)), axis=1)
    i = np.floor(np.where(ok[:, None], v, 0)).astype(np.int64)
    k = np.minimum(i, n - 1) // int(c)
    cell = (k[:, 0] * ly + k[:, 1]) * lz + k[:, 2]
    return np.where(ok, cell, -1)


def rotate(tri):
    """[F, 3] -> each triple rotated so that its smallest entry comes first, the cyclic order kept."""
    tri = np.asarray(tri)
    j = np.argmin(tri, axis=1)
    idx = (j[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(tri, idx, axis=1)


def cluster_faces(faces, cluster):
    """(faces' [F', 3] int32, survivors [F'] - the input indices, ascending): remap, rotate, drop fewer than three distinct, keep the first of
    equal rotated triples.  Faces with an index outside the vertex array must have been refused before."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(faces) == 0:
        return np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    r = rotate(cluster[faces])
    proper = (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2])
    idx = np.nonzero(proper)[0]
    if len(idx) == 0:
        return np.zeros((0, 3), np.int32), idx
    _, first = np.unique(r[idx], axis=0, return_index=True)          # the first occurrence of every distinct row
    keep = idx[np.sort(first)]
    return r[keep].astype(np.int32), keep


def simplify(verts, faces, shape, c, reg=0.01):
    """dict: bad (True: refused, nothing else), cluster [V] int32, cell_of [V'] (linear cell of every cluster), verts [V', 3] float64 grid
    coordinates, faces [F', 3] int32, survivors [F'], bound [V'] float64 (grid units, see the module docstring), x_local [V', 3] (clamped)."""
    v32 = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, cf = len(v32), float(c)
    cell = vertex_cells(v32, shape, c)
    if (cell < 0).any() or (len(faces) and ((faces < 0) | (faces >= V)).any()):
        return {"bad": True}
    cell_of, cluster = np.unique(cell, return_inverse=True)            # ascending cells: the numbering
    cluster = cluster.reshape(-1)
    K = len(cell_of)
    lx, ly, lz = lattice(shape, c)
    kxyz = np.stack([cell_of // (ly * lz), (cell_of // lz) % ly, cell_of % lz], axis=1).astype(np.float64)
    centre = cf * (kxyz + 0.5)                                         # [K, 3] grid coordinates
    g = v32.astype(np.float64)
    A, SA = np.zeros((K, 3, 3)), np.zeros((K, 3, 3))
    b, Sb = np.zeros((K, 3)), np.zeros((K, 3))
    s, Ss = np.zeros((K, 3)), np.zeros((K, 3))
    nf, nv = np.zeros(K), np.zeros(K)
    loc = (g - centre[cluster]) / cf
    np.add.at(s, cluster, loc)
    np.add.at(Ss, cluster, np.abs(loc))
    np.add.at(nv, cluster, 1.0)
    if len(faces):
        ga, gb, gc = g[faces[:, 0]], g[faces[:, 1]], g[faces[:, 2]]
        e1, e2 = (gb - ga) / cf, (gc - ga) / cf
        n = np.cross(e1, e2)
        N = np.abs(e1[:, [1, 2, 0]] * e2[:, [2, 0, 1]]) + np.abs(e1[:, [2, 0, 1]] * e2[:, [1, 2, 0]])
        ks = cluster[faces]
        for j in range(3):
            distinct = np.ones(len(faces), bool)
            for i in range(j):
                distinct &= ks[:, j] != ks[:, i]
            k = ks[distinct, j]
            l = (ga[distinct] - centre[k]) / cf
            nn, NN = n[distinct], N[distinct]
            np.add.at(A, k, nn[:, :, None] * nn[:, None, :])
            np.add.at(SA, k, NN[:, :, None] * NN[:, None, :])
            np.add.at(b, k, nn * np.sum(nn * l, axis=1, keepdims=True))
            np.add.at(Sb, k, NN * np.sum(NN * np.abs(l), axis=1, keepdims=True))
            np.add.at(nf, k, 1.0)
    m = s / nv[:, None]
    tr = np.trace(A, axis1=1, axis2=2)
    lam = reg * tr / 3.0
    x = m.copy()
    bound = np.full(K, SQRT3)
    dA = np.sqrt(np.sum((K_A * U * SA + QUANTUM * nf[:, None, None]) ** 2, axis=(1, 2)))
    db = np.sqrt(np.sum((K_B * U * Sb + QUANTUM * nf[:, None]) ** 2, axis=1))
    dm = np.sqrt(np.sum(((K_M * U * Ss + QUANTUM * nv[:, None]) / nv[:, None]) ** 2, axis=1))
    pos = tr > 0
    if pos.any():
        M = A[pos] + lam[pos, None, None] * np.eye(3)
        x[pos] = np.linalg.solve(M, (b[pos] + lam[pos, None] * m[pos])[:, :, None])[:, :, 0]
        inv = 1.0 / np.linalg.eigvalsh(M)[:, 0]
        lin = inv * (db[pos] + dA[pos] * np.linalg.norm(x[pos], axis=1) + lam[pos] * dm[pos])
        eps = inv * dA[pos]
        bound[pos] = np.where(eps < 0.5, lin / (1.0 - np.minimum(eps, 0.5)), SQRT3)
    flat = ~pos & (SA.sum(axis=(1, 2)) == 0)
    bound[flat] = dm[flat]
    xc = np.clip(x, -0.5, 0.5)
    out = centre + cf * xc
    bound = cf * np.minimum(bound, SQRT3) + U * np.linalg.norm(out, axis=1) + 1e-12 * cf
    f_out, survivors = cluster_faces(faces, cluster)
    return {"bad": False, "cluster": cluster.astype(np.int32), "cell_of": cell_of, "verts": out, "faces": f_out, "survivors": survivors,
            "bound": bound, "x_local": xc, "x_unclamped": x, "centre": centre}


def signed_volume(verts, faces):
    """sum v0 . (v1 x v2) / 6 in float64 (what bounds the effect of moved vertices on it is volume_bound)."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return float(np.sum(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]]))) / 6.0)


def volume_bound(verts, faces, bound):
    """The position bound propagated through signed_volume to first order plus the higher orders: moving vertex p by at most bound[p] changes
    each of its faces' triple products by at most bound[p] |v_q x v_r| (+ the products of two and three displacements)."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    total = 0.0
    for j in range(3):
        p, q, r = f[:, j], f[:, (j + 1) % 3], f[:, (j + 2) % 3]
        total += np.sum(bound[p] * np.linalg.norm(np.cross(v[q], v[r]), axis=1))                 # first order
        total += np.sum(bound[p] * bound[q] * (np.linalg.norm(v[r], axis=1) + bound[r] / 3.0))   # second and third order
    return float(total / 6.0)


# ---- the analytic volumes the tests mesh (float32 [nx, ny, nz], level 0, inside iff value < 0) ---------------------------------------------

def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def sphere_volume(shape, centre, radius):
    x, y, z = _grid(shape)
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(np.float32)


def two_spheres_volume(shape, c1, c2, radius):
    return np.minimum(sphere_volume(shape, c1, radius), sphere_volume(shape, c2, radius))


def shells_volume(shape, centre, r1, r2, r3):
    """A ball of radius r1 inside a shell r2 .. r3: three concentric sheets, the first and the third with the same orientation - clustered with a
    cell wider than r3 - r1 they give faces with EQUAL rotated triples."""
    x, y, z = _grid(shape)
    r = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return np.minimum(r - r1, np.maximum(r2 - r, r - r3)).astype(np.float32)


def slab_volume(shape, x0, x1):
    """The slab x0 < x < x1: two sheets, at x0 and x1; a sheet at an integer x has every vertex exactly on a grid point."""
    x, _, _ = _grid(shape)
    return (np.abs(x - 0.5 * (x0 + x1)) - 0.5 * (x1 - x0)).astype(np.float32)


def plane_volume(shape, normal, offset):
    """normal . p - offset; an axis normal with an integer offset puts every vertex exactly on a grid point."""
    x, y, z = _grid(shape)
    return (normal[0] * x + normal[1] * y + normal[2] * z - offset).astype(np.float32)
