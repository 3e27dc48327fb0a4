"""Float64 numpy statement of the per-face texture atlas (include/nerfart_hip.h, "per-face texture atlas"; csrc/mesh_texture.hip;
mesh_util.texel_points / bake_texture / write_obj): the layout, the table that says which face owns which texel, the corner UVs, the texels' points,
the Newton step onto the level set, a bilinear sampler that reports what it read, and parsers for the three files write_obj writes.  Written
from the rules, not from the kernel; tests/test_mesh_texture_ref.py holds it to the two properties the atlas is built on and shows that its checks
catch four injected bugs; tests/test_gpu_mesh_texture.py holds the kernels to it.

THE LAYOUT.  F faces, patch size P >= 1.  S = P + 3, n_cells = ceil(F / 2), Cw = the smallest integer with Cw^2 >= n_cells, Ch = ceil(n_cells / Cw),
W = Cw S, H = Ch S, row 0 on top.  Cell q sits at column q % Cw, row q // Cw and holds the faces 2 q and 2 q + 1.  Texel (x, y): cell
(x // S, y // S), local (i, j) = (x % S, y % S); i + j <= P + 2: the lower face 2 q with (a, b) = (i, j), else the upper face 2 q + 1 with
(a, b) = (S - 1 - i, S - 1 - j); valid iff the face index is < F.  Point: w1 = a / P, w2 = b / P, w0 = 1 - w1 - w2, p = w0 v0 + w1 v1 + w2 v2.
UVs in pixel units, relative to the cell's origin: lower (0.5, 0.5), (0.5 + P, 0.5), (0.5, 0.5 + P), upper S minus those.

THE BOUND of the fp32 points.  The kernel computes, per coordinate, w_k = fl(n_k / P) with n_k the integers P - a - b, a, b (exact in fp32: below
2^15), then r = fma(w2, v2, fma(w1, v1, fl(w0 v0))).  Every fl and every fma rounds once with relative error at most u = 2^-24.  The term w0 v0
passes four roundings (the division, the product, two fmas), w1 v1 three, w2 v2 two, so
    |r - (w0 v0 + w1 v1 + w2 v2)| <= ((1 + u)^4 - 1) sum_k |w_k| |v_k| <= 4 u / (1 - 4 u) sum_k |w_k| |v_k|
with the exact weights w_k and the fp32 vertices v_k as given.  The constant is 4 (times 1 / (1 - 4 u)), derived, not tuned.  The float64 evaluation
here (weights as quotients of integers, rounded once; three products, two sums) errs by at most 8 * 2^-53 of the same sum, which is added.

THE PROJECTION STEP.  Given sdf and g = nabla at p: d = -(sdf - level) g / |g|^2, scaled down to length max_step when longer; p stays when sdf or
g is not finite or |g|^2 < 1e-12.  The kernel computes (fp32) e = sdf - level, g2 = fma(gz, gz, fma(gy, gy, gx gx)), gn = sqrt(g2),
m = min(|e| / gn, max_step), c = copysign(m, -e) / gn, p_k + c g_k.  First-order relative errors, in units of u: e 1; g2 at most 3 (every term
passes at most three roundings); gn 3 / 2 + 1; |e| / gn 1 + 5 / 2 + 1 = 9 / 2, and min is 1-Lipschitz, so m 9 / 2; c 9 / 2 + 5 / 2 + 1 = 8;
c g_k 9.  Taking 10 u |d_k| covers these nine and every higher-order term (9 u + 45 u^2 < 10 u), and the final sum adds u |p_k + d_k| <=
u (|p_k| + |d_k|) (1 + 10 u).  Hence
    |p'_k(fp32) - p'_k(exact)| <= u (11 |d_k| + |p_k|) (1 + 2^-20)
with d the exact step - the constant 11 is derived, not tuned."""
import math

import numpy as np

U = 2.0 ** -24
MAX_SIDE = 16384
BUGS = ("S_is_P_plus_2", "corners_at_texel_edges", "upper_not_mirrored")          # variants of the rules that the checks must catch


def layout(F, P, bug=None):
    """(S, Cw, Ch, W, H); ValueError for P < 1, F < 1 or an image side above MAX_SIDE."""
    F, P = int(F), int(P)
    if P < 1 or F < 1:
        raise ValueError(f"F and P must be >= 1 (got {F}, {P})")
    S = P + (2 if bug == "S_is_P_plus_2" else 3)
    cells = -(-F // 2)
    Cw = 1
    while Cw * Cw < cells:
        Cw += 1
    Ch = -(-cells // Cw)
    if Cw * S > MAX_SIDE or Ch * S > MAX_SIDE:
        raise ValueError(f"F = {F}, P = {P}: the image would be {Cw * S} x {Ch * S}")
    return S, Cw, Ch, Cw * S, Ch * S


def texel_table(F, P, bug=None):
    """(face_of [H, W] int64 with -1 for invalid texels, a [H, W], b [H, W]): the owner of every texel and its integer coordinates in the owner."""
    S, Cw, Ch, W, H = layout(F, P, bug)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    q = (y // S) * Cw + x // S
    i, j = x % S, y % S
    lower = i + j <= P + 2
    face = 2 * q + np.where(lower, 0, 1)
    if bug == "upper_not_mirrored":
        a, b = i, j
    else:
        a, b = np.where(lower, i, S - 1 - i), np.where(lower, j, S - 1 - j)
    return np.where(face < F, face, -1), a, b


def uvs(F, P, bug=None):
    """[F, 3, 2] float64: the corner UVs in pixel units (x right, y down, texel centres at + 0.5)."""
    S, Cw, _, _, _ = layout(F, P, bug)
    h = 0.0 if bug == "corners_at_texel_edges" else 0.5
    lower = np.array([[h, h], [h + P, h], [h, h + P]])
    out = np.empty((F, 3, 2))
    for f in range(F):
        q = f // 2
        out[f] = np.array([(q % Cw) * S, (q // Cw) * S], dtype=np.float64) + (lower if f % 2 == 0 else S - lower)
    return out


def points(verts, faces, P, bug=None):
    """(points [H W, 3] float64 with 0 for invalid texels, face_of [H, W], bound [H W, 3]): the texels' points from the fp32 vertices, and the
    bound of the module's docstring on what an fp32 evaluation by the kernel's formula may differ by."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face_of, a, b = texel_table(len(f), P, bug)
    owner = face_of.reshape(-1)
    ok = owner >= 0
    ia, ib = a.reshape(-1)[ok], b.reshape(-1)[ok]
    # w0 = 1 - w1 - w2 = (P - a - b) / P from the integers: one rounding (1 - a / P - b / P leaves 6e-17 where w0 is 0, which no bound
    # relative to |w0| |v0| covers)
    w = np.stack([(P - ia - ib) / float(P), ia / float(P), ib / float(P)], axis=-1)  # [T, 3]
    tri = v[f[owner[ok]]]                                                           # [T, 3 corners, 3 coordinates]
    pts, bound = np.zeros((owner.size, 3)), np.zeros((owner.size, 3))
    pts[ok] = np.einsum("tk,tkc->tc", w, tri)
    bound[ok] = (4.0 * U / (1.0 - 4.0 * U) + 8.0 * 2.0 ** -53) * np.einsum("tk,tkc->tc", np.abs(w), np.abs(tri))
    return pts, face_of, bound


def project_step(pts, sdf, nabla, level, max_step):
    """(points' [n, 3] float64, moved [n] bool, bound [n, 3]): one Newton step of the fp32 inputs in float64, which rows moved, and the bound of
    the module's docstring."""
    p, s, g = (np.asarray(a, dtype=np.float64) for a in (pts, sdf, nabla))
    with np.errstate(all="ignore"):
        g2 = np.sum(g * g, axis=1)
        moved = np.isfinite(s) & np.all(np.isfinite(g), axis=1) & (g2 >= 1e-12)
        e = s - float(level)
        d = -(e / g2)[:, None] * g
        length = np.linalg.norm(d, axis=1)
        scale = np.where(length > max_step, max_step / length, 1.0)
        d = np.where(moved[:, None], d * scale[:, None], 0.0)
    return p + d, moved, U * (11.0 * np.abs(d) + np.abs(p)) * (1.0 + 2.0 ** -20)


def bilinear(image, X, Y, eps=1e-12):
    """Bilinear sample of image [H, W, ...] (float64) at the pixel coordinates (X, Y), texel centres at + 0.5, clamped at the border:
    (value, [(x, y, weight)]) - the texels read with a weight above eps; only they enter the value."""
    H, W = image.shape[:2]
    fx, fy = X - 0.5, Y - 0.5
    x0, y0 = math.floor(fx), math.floor(fy)
    tx, ty = fx - x0, fy - y0
    read, value = [], 0.0
    for yy, wy in ((y0, 1.0 - ty), (y0 + 1, ty)):
        for xx, wx in ((x0, 1.0 - tx), (x0 + 1, tx)):
            if wx * wy > eps:
                cx, cy = min(max(xx, 0), W - 1), min(max(yy, 0), H - 1)
                read.append((cx, cy, wx * wy))
                value = value + wx * wy * image[cy, cx]
    return value, read


def surface_samples(rng, n_interior=6, n_edge=3):
    """Barycentric triples [n, 3]: random interior points, points on each of the three edges, the three corners."""
    out = [rng.dirichlet(np.ones(3), size=n_interior)]
    for k in range(3):
        t = rng.uniform(0.0, 1.0, size=n_edge)
        e = np.zeros((n_edge, 3))
        e[:, k], e[:, (k + 1) % 3] = t, 1.0 - t
        out.append(e)
    out.append(np.eye(3))
    return np.concatenate(out)


def check_atlas(verts, faces, P, rng, bug=None, tol=1e-9):
    """The two properties the atlas is built on, for every face of the mesh: bilinear sampling at the UV of any point of a face reads, with
    non-zero weight, only texels that face owns; and texels carrying an affine function of their points give that function at the surface
    point (tol, float64).  Raises AssertionError; returns the number of samples taken."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    pts, face_of, _ = points(v, f, P, bug)
    H, W = face_of.shape
    coef, shift = rng.normal(size=(3, 2)), rng.normal(size=2)                       # two affine functions at once
    texels = np.where((face_of.reshape(-1) >= 0)[:, None], pts @ coef + shift, np.nan).reshape(H, W, 2)
    uv = uvs(len(f), P, bug)
    n = 0
    for k in range(len(f)):
        for lam in surface_samples(rng):
            X, Y = lam @ uv[k]
            value, read = bilinear(texels, X, Y)
            assert read and abs(sum(w for _, _, w in read) - 1.0) < 1e-9
            for x, y, w in read:
                assert face_of[y, x] == k, f"face {k} at barycentrics {lam} reads texel ({x}, {y}) of face {face_of[y, x]} with weight {w}"
            want = (lam @ v[f[k]]) @ coef + shift
            assert np.all(np.abs(value - want) <= tol * (1.0 + np.abs(want))), f"face {k} at {lam}: sampled {value}, the function is {want}"
            n += 1
    return n


# ---- the three files of write_obj ------------------------------------------------------------------------------------------------------------

def read_obj(path):
    """dict: mtllib, usemtl, v [V, 3], vt [T, 2], vn [N, 3] or None, f [F, 3, k] 1-based index triples as written (k = 2: v/vt, 3: v/vt/vn)."""
    out = {"mtllib": None, "usemtl": None, "v": [], "vt": [], "vn": [], "f": []}
    for line in open(path):
        tok = line.split()
        if not tok:
            continue
        if tok[0] in ("mtllib", "usemtl"):
            out[tok[0]] = tok[1]
        elif tok[0] in ("v", "vt", "vn"):
            out[tok[0]].append([float(t) for t in tok[1:]])
        elif tok[0] == "f":
            out["f"].append([[int(i) for i in t.split("/")] for t in tok[1:]])
        else:
            raise ValueError(f"unexpected OBJ line: {line!r}")
    out["v"], out["vt"] = np.array(out["v"], dtype=np.float64).reshape(-1, 3), np.array(out["vt"], dtype=np.float64).reshape(-1, 2)
    out["vn"] = np.array(out["vn"], dtype=np.float64).reshape(-1, 3) if out["vn"] else None
    out["f"] = np.array(out["f"], dtype=np.int64)
    return out


def read_mtl(path):
    """dict: newmtl, map_Kd."""
    out = {}
    for line in open(path):
        tok = line.split()
        if tok and tok[0] in ("newmtl", "map_Kd"):
            out[tok[0]] = tok[1]
    return out


def read_png(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


def vt_to_pixels(vt, W, H):
    """OBJ texture coordinates -> pixel coordinates of the image as stored (row 0 on top): X = u W, Y = (1 - v) H."""
    vt = np.asarray(vt, dtype=np.float64)
    return np.stack([vt[..., 0] * W, (1.0 - vt[..., 1]) * H], axis=-1)


def check_obj_corners(obj, image, P):
    """Sampling the stored image at every face's three vt corners returns that face's corner texels: the texels (a, b) = (0, 0), (P, 0), (0, P)
    of the face in the texel table.  Also: indices 1-based and in range, vt in [0, 1]."""
    H, W = image.shape[:2]
    f = obj["f"]
    F = len(f)
    face_of, a, b = texel_table(F, P)
    assert face_of.shape == (H, W)
    assert f[..., 0].min() >= 1 and f[..., 0].max() <= len(obj["v"]) and f[..., 1].min() >= 1 and f[..., 1].max() <= len(obj["vt"])
    if f.shape[2] == 3:
        assert obj["vn"] is not None and f[..., 2].min() >= 1 and f[..., 2].max() <= len(obj["vn"])
    assert obj["vt"].min() >= 0.0 and obj["vt"].max() <= 1.0
    img = image.astype(np.float64)
    corner_ab = ((0, 0), (P, 0), (0, P))
    for k in range(F):
        for c in range(3):
            X, Y = vt_to_pixels(obj["vt"][f[k, c, 1] - 1], W, H)
            value, read = bilinear(img, X, Y, eps=1e-4)            # vt went through %.9g: a weight of 1e-7 is print rounding
            ys, xs = np.nonzero((face_of == k) & (a == corner_ab[c][0]) & (b == corner_ab[c][1]))
            assert len(xs) == 1
            assert [(x, y) for x, y, _ in read] == [(xs[0], ys[0])], f"face {k} corner {c}: read {read}, its corner texel is ({xs[0]}, {ys[0]})"
            assert np.all(np.abs(value - img[ys[0], xs[0]]) < 1e-3)
