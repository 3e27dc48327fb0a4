"""csrc/mesh_raster.hip in plain numpy - the statement tests/test_gpu_mesh_raster.py holds the kernels to, and tests/test_mesh_raster_ref.py
holds to the properties a rasteriser is trusted for.  The rules are those of include/nerfart_hip.h:

  * project: camera space in float64 from the float32 inputs, u = fx X/Z + sk Y/Z + cx, v = fy Y/Z + cy, snapped to 1/256 pixel (half to even);
  * coverage: three integer edge functions at the sample (256 i, 256 j) - Python / int64 integers -, the top-left rule;
  * depth: the pixel's ray against the face's plane through the UNSNAPPED camera-space vertices, float64; the nearest float32(z) wins, equal
    depths go to the smaller face index;
  * resolve: barycentrics as signed areas against the face's normal, depth = z |r|, the normal turned toward the camera, in world space;
  * interp and bilinear sampling in emulated float32, operation by operation.

`bug=` injects the mistakes the CPU tests must catch."""
import numpy as np

FIX = 256
MAX_PIXEL = 32768.0
U32 = 2.0 ** -24


def camera_numbers(c2w, K):
    """(w2c [3, 4], rot [3, 3], (fx, sk, cx, fy, cy)) as float64 holding the float32 numbers the kernels are handed."""
    c = np.asarray(c2w, dtype=np.float32).reshape(4, 4)
    k = np.asarray(K, dtype=np.float32).reshape(-1).astype(np.float64)
    w2c = np.linalg.inv(c.astype(np.float64))[:3].astype(np.float32).astype(np.float64)
    return w2c, c[:3, :3].astype(np.float64), (k[0], k[1], k[2], k[5], k[6])


def project(verts, c2w, K, near=1e-3):
    """dict: u, v (float64, before the snap), xy_fix [V, 2] int64, cam [V, 3] float64 (round to float32 ONCE to get the kernel's), valid [V] bool."""
    w2c, _, (fx, sk, cx, fy, cy) = camera_numbers(c2w, K)
    p = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        cam = np.stack([((w2c[r, 0] * p[:, 0] + w2c[r, 1] * p[:, 1]) + w2c[r, 2] * p[:, 2]) + w2c[r, 3] for r in range(3)], axis=-1)
        xz, yz = cam[:, 0] / cam[:, 2], cam[:, 1] / cam[:, 2]
        u, v = (fx * xz + sk * yz) + cx, fy * yz + cy
        valid = (cam[:, 2] >= float(np.float32(near))) & (np.abs(u) <= MAX_PIXEL) & (np.abs(v) <= MAX_PIXEL)
        xy = np.where(valid[:, None], np.rint(np.stack([u, v], axis=-1) * FIX), 0.0).astype(np.int64)
    return {"u": u, "v": v, "xy_fix": xy, "cam": cam, "valid": valid}


def pixel_rays(K5, H, W, bug=None):
    """(x, y) [H, W] float64 of the camera-space rays r = (x, y, 1): k_get_rays' expressions."""
    fx, sk, cx, fy, cy = K5
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    if bug == "half_pixel":
        i, j = i + 0.5, j + 0.5
    return ((i - cx + cy * sk / fy) - sk * j / fy) / fx, (j - cy) / fy


def _edge(xa, ya, xb, yb, sx, sy, bug):
    dx, dy = xb - xa, yb - ya
    E = dx * (sy - ya) - dy * (sx - xa)
    if bug == "ge_all":
        return E >= 0
    if bug == "gt_all":
        return E > 0
    return (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def coverage(tri, H, W, bug=None):
    """bool [H, W]: the pixels the triangle tri [3, 2] (integers, 1/256 pixel) covers.  int64 throughout (|coordinate| <= 2^23)."""
    (x0, y0), (x1, y1), (x2, y2) = [(int(a), int(b)) for a, b in np.asarray(tri).reshape(3, 2)]
    A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    out = np.zeros((H, W), dtype=bool)
    if A == 0:
        return out
    if A < 0:
        x1, y1, x2, y2 = x2, y2, x1, y1
    off = FIX // 2 if bug == "half_pixel" else 0
    sy, sx = np.meshgrid(np.arange(H, dtype=np.int64) * FIX + off, np.arange(W, dtype=np.int64) * FIX + off, indexing="ij")
    return _edge(x0, y0, x1, y1, sx, sy, bug) & _edge(x1, y1, x2, y2, sx, sy, bug) & _edge(x2, y2, x0, y0, sx, sy, bug)


def face_plane(cam, tri):
    a, b, c = (cam[int(k)] for k in tri)
    u, v = b - a, c - a
    n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    return a, b, c, n, (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]


def rasterize(verts, faces, c2w, K, H, W, near=1e-3, xy_fix=None, cam32=None, valid=None, bug=None):
    """The whole pipeline.  xy_fix / cam32 / valid: take these (the kernel's own) instead of project()'s.  dict over [H W]: face_id (int64, -1),
    z, depth, bary [., 3], normals [., 3] (float64, unrounded; 0 on a miss), mask, second_z (the nearest z of ANOTHER face, inf if none);
    and bad, n_skipped, n_rejected."""
    pr = project(verts, c2w, K, near)
    xy = pr["xy_fix"] if xy_fix is None else np.asarray(xy_fix, dtype=np.int64)
    cam = (pr["cam"].astype(np.float32) if cam32 is None else np.asarray(cam32, dtype=np.float32)).astype(np.float64)
    ok = pr["valid"] if valid is None else np.asarray(valid).astype(bool)
    _, rot, K5 = camera_numbers(c2w, K)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, nr = len(cam), float(np.float32(near))
    x, y = pixel_rays(K5, H, W, bug)
    best_z = np.full((H, W), np.inf, dtype=np.float32)
    best_f = np.full((H, W), -1, dtype=np.int64)
    z1 = np.full((H, W), np.inf)                                       # nearest and second nearest z, float64, over all faces
    z2 = np.full((H, W), np.inf)
    bad, n_skipped, n_rejected = 0, 0, 0
    for k, tri in enumerate(f):
        if tri.min() < 0 or tri.max() >= V:
            bad = 1
            continue
        if not ok[tri].all():
            n_skipped += 1
            continue
        cov = coverage(xy[tri], H, W, bug)
        if not cov.any():
            continue
        a, b, c, n, na = face_plane(cam, tri)
        with np.errstate(all="ignore"):
            z = na / ((n[0] * x + n[1] * y) + n[2])
        good = cov & (z >= nr) & np.isfinite(z)
        n_rejected += int((cov & ~good).sum())
        zf = np.where(good, z, np.inf).astype(np.float32)
        wins = good & ((zf <= best_z) if bug == "tie_larger" else (zf < best_z))       # faces come in ascending order: < keeps the smaller index
        best_z[wins], best_f[wins] = zf[wins], k
        zz = np.where(good, z, np.inf)
        z2 = np.where(zz < z1, z1, np.minimum(z2, zz))
        z1 = np.minimum(z1, zz)
    out = resolve(best_f.reshape(-1), cam, f, rot, K5, H, W, bug)
    out.update(bad=bad, n_skipped=n_skipped, n_rejected=n_rejected, second_z=z2.reshape(-1), first_z=z1.reshape(-1))
    return out


def resolve(face_id, cam, faces, rot, K5, H, W, bug=None):
    """float64 z, depth, bary, normals for the given winner per pixel (face_id [H W], -1 = miss)."""
    x, y = (a.reshape(-1) for a in pixel_rays(K5, H, W, bug))
    n_pix = H * W
    z, depth, bary, normals = np.zeros(n_pix), np.zeros(n_pix), np.zeros((n_pix, 3)), np.zeros((n_pix, 3))
    for p in np.nonzero(face_id >= 0)[0]:
        a, b, c, n, na = face_plane(cam, faces[face_id[p]])
        r = np.array([x[p], y[p], 1.0])
        zp = na / ((n[0] * r[0] + n[1] * r[1]) + n[2])
        h = zp * r
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        area = lambda p1, p2: float(np.dot(n, np.cross(p1 - h, p2 - h)))
        bary[p] = [area(b, c) / nn, area(c, a) / nn, area(a, b) / nn]
        z[p] = zp
        depth[p] = zp if bug == "camera_z" else zp * np.sqrt((r[0] * r[0] + r[1] * r[1]) + 1.0)
        s = (-1.0 if (n[0] * r[0] + n[1] * r[1]) + n[2] > 0.0 else 1.0) / np.sqrt(nn)
        normals[p] = rot @ (s * n)
    return {"face_id": face_id.copy(), "z": z, "depth": depth, "bary": bary, "normals": normals, "mask": face_id >= 0}


# ---- shading -----------------------------------------------------------------------------------------------------------------------------------

def f32(a):
    return np.asarray(a, dtype=np.float32)


def fma32(a, b, c):
    """fmaf: the product of two float32 is exact in float64; the sum is rounded to float64, then to float32 (a double rounding that differs from
    the single one only when the float64 sum lands exactly on a float32 tie)."""
    return (f32(a).astype(np.float64) * f32(b).astype(np.float64) + f32(c).astype(np.float64)).astype(np.float32)


def interp(face_id, bary, attr, faces=None, fill=0.0):
    """out [n, C] float32 by the kernel's order: fma(w2, a2, fma(w1, a1, w0 * a0)).  attr [V, C] with faces, or [F, 3, C] without."""
    face_id, w, attr = np.asarray(face_id, dtype=np.int64), f32(bary), f32(attr)
    hit = face_id >= 0
    fid = np.where(hit, face_id, 0)
    corners = attr[np.asarray(faces, dtype=np.int64)[fid]] if faces is not None else attr[fid]          # [n, 3, C]
    out = fma32(w[:, 2:3], corners[:, 2], fma32(w[:, 1:2], corners[:, 1], f32(w[:, 0:1] * corners[:, 0])))
    return np.where(hit[:, None], out, np.float32(fill)).astype(np.float32)


def sample_bilinear(uv, image, mask=None, background=(0.0, 0.0, 0.0), bug=None):
    """rgb [n, 3] float32 by the kernel's order.  uv in pixel units, texel centres at + 0.5, y down; clamp to edge; level / 255."""
    uv, img = f32(uv), np.asarray(image, dtype=np.uint8)
    Ht, Wt = img.shape[:2]
    half = np.float32(0.0 if bug == "no_half_texel" else 0.5)
    u, v = uv[:, 0], uv[:, 1]
    if bug == "v_flip":
        v = f32(np.float32(Ht) - v)
    live = np.isfinite(u) & np.isfinite(v) & (np.ones(len(uv), bool) if mask is None else np.asarray(mask).astype(bool))
    u, v = np.where(live, u, 0).astype(np.float32), np.where(live, v, 0).astype(np.float32)
    X, Y = f32(u - half), f32(v - half)
    x0, y0 = np.clip(np.floor(X), -1, Wt).astype(np.float32), np.clip(np.floor(Y), -1, Ht).astype(np.float32)
    tx, ty = np.clip(f32(X - x0), 0, 1).astype(np.float32), np.clip(f32(Y - y0), 0, 1).astype(np.float32)
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb, ya, yb = np.clip(xi, 0, Wt - 1), np.clip(xi + 1, 0, Wt - 1), np.clip(yi, 0, Ht - 1), np.clip(yi + 1, 0, Ht - 1)
    t00, t10, t01, t11 = (img[r, c].astype(np.float32) for r, c in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
    top, bot = fma32(tx[:, None], f32(t10 - t00), t00), fma32(tx[:, None], f32(t11 - t01), t01)
    out = f32(fma32(ty[:, None], f32(bot - top), top) / np.float32(255.0))
    return np.where(live[:, None], out, f32(background)[None]).astype(np.float32)


# ---- ray casting, for the comparison ---------------------------------------------------------------------------------------------------------

def lift_rays(c2w, K, H, W):
    """(origin [3], dirs [H W, 3]) float64, world space, NOT normalised: rend_util's lift (z = 1) and get_rays, restated."""
    c = np.asarray(c2w, dtype=np.float32).astype(np.float64).reshape(4, 4)
    k = np.asarray(K, dtype=np.float32).astype(np.float64).reshape(4, 4)
    fx, fy, cx, cy, sk = k[0, 0], k[1, 1], k[0, 2], k[1, 2], k[0, 1]
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = np.ones_like(i)
    x_lift = (i - cx + cy * sk / fy - sk * j / fy) / fx * z
    y_lift = (j - cy) / fy * z
    pts = np.stack([x_lift, y_lift, z, np.ones_like(z)], axis=-1).reshape(-1, 4)
    world = pts @ c.T
    return c[:3, 3].copy(), world[:, :3] - c[:3, 3]


def moller_trumbore(o, d, v0, v1, v2):
    """One ray against F triangles (float64): (t [F], b1 [F], b2 [F]), t = inf where there is no hit (both sides count)."""
    e1, e2 = v1 - v0, v2 - v0
    pv = np.cross(d[None], e2)
    det = np.einsum("fk,fk->f", e1, pv)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        tv = o[None] - v0
        b1 = np.einsum("fk,fk->f", tv, pv) * inv
        qv = np.cross(tv, e1)
        b2 = np.einsum("k,fk->f", d, qv) * inv
        t = np.einsum("fk,fk->f", e2, qv) * inv
        hit = (det != 0) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1) & (t > 0)
    return np.where(hit, t, np.inf), b1, b2


def edge_distance(u, v, faces, H, W, valid):
    """[H, W] float64: the distance in pixels from every pixel centre to the nearest projected (unsnapped) edge of a face with valid vertices."""
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    best = np.full((H, W), np.inf)
    seen = set()
    for tri in np.asarray(faces, dtype=np.int64):
        if not valid[tri].all():
            continue
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            key = (min(a, b), max(a, b))
            if key in seen:
                continue
            seen.add(key)
            ax, ay, bx, by = u[a], v[a], u[b], v[b]
            dx, dy = bx - ax, by - ay
            L2 = dx * dx + dy * dy
            t = np.clip(((i - ax) * dx + (j - ay) * dy) / L2, 0.0, 1.0) if L2 > 0 else np.zeros_like(i)
            best = np.minimum(best, np.hypot(i - (ax + t * dx), j - (ay + t * dy)))
    return best


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------------

def screen_camera(fx=64.0, cx=0.0, cy=0.0):
    """Identity pose and a power-of-two focal length: a vertex ((px - cx) / fx, (py - cy) / fx, 1) projects to the pixel (px, py) EXACTLY when px, py
    are multiples of 1/256."""
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = fx
    K[0, 2], K[1, 2] = cx, cy
    return np.eye(4, dtype=np.float32), K


def screen_mesh(pixels, fx=64.0, z=1.0):
    """[V, 3] float32 whose projection by screen_camera(fx) is `pixels` [V, 2] (multiples of 1/256), all at camera depth z (a power of two)."""
    p = np.asarray(pixels, dtype=np.float64)
    return np.concatenate([p * z / fx, np.full((len(p), 1), z)], axis=1).astype(np.float32)


def grid_polygon(s=1):
    """A rectangle from (2, 1) s to (14, 10) s cut into 4 x 3 square cells of side 3 s, each split along a diagonal (alternating): every vertex
    sits on a pixel centre, every edge is horizontal, vertical or a 45-degree diagonal through pixel centres.
    (pixels [V, 2], faces [F, 3], outline [4, 2] = the rectangle's corners in order)."""
    xs, ys = [2, 5, 8, 11, 14], [1, 4, 7, 10]
    pix = np.array([[x * s, y * s] for y in ys for x in xs], dtype=np.float64)
    faces = []
    for r in range(3):
        for c in range(4):
            a, b, d, e = r * 5 + c, r * 5 + c + 1, (r + 1) * 5 + c, (r + 1) * 5 + c + 1
            faces += [[a, b, e], [a, e, d]] if (r + c) % 2 == 0 else [[a, b, d], [b, e, d]]
    return pix, np.array(faces, dtype=np.int32), np.array([[2, 1], [14, 1], [14, 10], [2, 10]], dtype=np.float64) * s


def fan_polygon(s=1):
    """A convex quadrilateral fanned from an interior point that is on no pixel centre: the rim holds the four corners and the four edge midpoints
    (exactly collinear in 1/256 pixel).  (pixels, faces, outline)."""
    corners = np.array([[2, 1], [14, 2], [13, 10], [1, 9]], dtype=np.float64) * s
    rim = []
    for k in range(4):
        rim += [corners[k], (corners[k] + corners[(k + 1) % 4]) / 2]
    pix = np.array([[7.5 * s, 5.25 * s]] + rim, dtype=np.float64)
    faces = np.array([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)], dtype=np.int32)
    return pix, faces, corners


def union_coverage(pixels, faces, H, W, bug=None):
    """(count [H, W] int: how many faces cover each pixel)."""
    xy = np.rint(np.asarray(pixels) * FIX).astype(np.int64)
    assert np.array_equal(xy, np.asarray(pixels) * FIX), "the polygon's vertices must be multiples of 1/256 pixel"
    return sum(coverage(xy[np.asarray(t)], H, W, bug).astype(np.int64) for t in faces)


def sphere_mesh(N=12, radius=0.6):
    """The marching-cubes sphere of tests/mc_ref.py on an N^3 grid over [-1, 1]^3: (verts [V, 3] float32, faces [F, 3] int32)."""
    import mc_ref
    g = np.linspace(-1.0, 1.0, N)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    vol = (np.sqrt(X * X + Y * Y + Z * Z) - radius).astype(np.float32)
    v, f = mc_ref.marching_cubes(vol, 0.0, spacing=[2.0 / (N - 1)] * 3, origin=[-1.0] * 3)
    return v.astype(np.float32), f.astype(np.int32)
