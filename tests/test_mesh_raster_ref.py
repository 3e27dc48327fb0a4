"""tests/mesh_raster_ref.py - the numpy statement of csrc/mesh_raster.hip - held to the properties a rasteriser is trusted for, on the CPU: coverage
partitions a triangulated polygon (top-left rule), the winner per pixel is what float64 ray casting finds, bilinear sampling returns an affine
texture, and each of the classic mistakes, injected, is caught.  Also the round trips of mesh_util.read_ply / read_obj."""
import numpy as np
import pytest

import mesh_raster_ref as ref

POLYGONS = {"grid": ref.grid_polygon, "fan": ref.fan_polygon}
EPS_CAM = 2.0 ** -24 * 8.0 * np.sqrt(3.0)      # how far a camera-space vertex of the sphere test can be from its exact place: see the test


def _inside_convex(outline, H, W):
    """(strictly inside, on the boundary) [H, W] of the convex polygon `outline` (clockwise on screen), exact: integers in 1/256 pixel."""
    o = np.rint(outline * ref.FIX).astype(np.int64)
    sy, sx = np.meshgrid(np.arange(H, dtype=np.int64) * ref.FIX, np.arange(W, dtype=np.int64) * ref.FIX, indexing="ij")
    E = [(o[(k + 1) % len(o), 0] - o[k, 0]) * (sy - o[k, 1]) - (o[(k + 1) % len(o), 1] - o[k, 1]) * (sx - o[k, 0]) for k in range(len(o))]
    inside = np.all([e > 0 for e in E], axis=0)
    closed = np.all([e >= 0 for e in E], axis=0)
    return inside, closed & ~inside, E, o


@pytest.mark.parametrize("s,H,W", [(1, 12, 16), (1, 17, 33), (4, 64, 64)])
@pytest.mark.parametrize("name", list(POLYGONS))
def test_coverage_partitions_a_triangulated_polygon(name, s, H, W):
    pix, faces, outline = POLYGONS[name](s)
    count = ref.union_coverage(pix, faces, H, W)
    inside, boundary, E, o = _inside_convex(outline, H, W)
    assert inside.sum() > 20 and boundary.sum() > 0
    assert np.all(count[inside] == 1), "a pixel centre strictly inside the polygon is not covered exactly once"
    assert np.all(count[~inside & ~boundary] == 0) and count.max() == 1
    # the construction: vertices on pixel centres, edges through pixel centres away from their ends, horizontal and vertical edges
    xy = np.rint(pix * ref.FIX).astype(np.int64)
    assert np.any(np.all(xy % ref.FIX == 0, axis=1))
    through, horizontal, vertical = 0, 0, 0
    for tri in faces:
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            (xa, ya), (xb, yb) = xy[a], xy[b]
            horizontal, vertical = horizontal + (ya == yb), vertical + (xa == xb)
            for j in range(H):
                for i in range(W):
                    sx, sy = i * ref.FIX, j * ref.FIX
                    if (xb - xa) * (sy - ya) - (yb - ya) * (sx - xa) == 0 and min(xa, xb) <= sx <= max(xa, xb) and min(ya, yb) <= sy <= max(ya, yb) \
                            and (sx, sy) not in ((xa, ya), (xb, yb)):
                        through += 1
    assert through > 0 and (name != "grid" or (horizontal > 0 and vertical > 0))
    # the polygon's own boundary follows the top-left rule: a pixel centre on exactly one outline edge is covered iff that edge is top or left
    on = [(e == 0) & boundary for e in E]
    n_checked = 0
    for k in range(len(o)):
        alone = on[k] & ~np.any([on[m] for m in range(len(o)) if m != k], axis=0)
        dx, dy = o[(k + 1) % len(o)] - o[k]
        top_left = dy < 0 or (dy == 0 and dx > 0)
        assert np.all(count[alone] == (1 if top_left else 0)), f"outline edge {k}"
        n_checked += int(alone.sum())
    assert n_checked > 0 or s == 1
    if name == "grid":
        j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        assert np.array_equal(count == 1, (i >= 2 * s) & (i < 14 * s) & (j >= 1 * s) & (j < 10 * s)), "top and left in, bottom and right out"
    # two big triangles cover the same pixels; so does every face wound the other way
    big = ref.union_coverage(outline, [[0, 1, 2], [0, 2, 3]], H, W)
    assert np.array_equal(big, count)
    assert np.array_equal(ref.union_coverage(pix, faces[:, ::-1], H, W), count)
    for t in faces:
        assert np.array_equal(ref.coverage(xy[t], H, W), ref.coverage(xy[t[::-1]], H, W))


def test_injected_coverage_bugs_are_caught():
    pix, faces, outline = ref.grid_polygon(1)
    H, W = 12, 16
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    want = (i >= 2) & (i < 14) & (j >= 1) & (j < 10)
    inside = (i > 2) & (i < 14) & (j > 1) & (j < 10)
    assert np.array_equal(ref.union_coverage(pix, faces, H, W) == 1, want)
    ge = ref.union_coverage(pix, faces, H, W, bug="ge_all")
    assert ge[inside].max() >= 2, ">= on every edge draws shared edges twice"
    gt = ref.union_coverage(pix, faces, H, W, bug="gt_all")
    assert gt[inside].min() == 0, "> on every edge leaves shared edges undrawn"
    # a half-pixel offset still partitions, so it is caught by a known answer: the triangle (0, 0), (3, 0), (0, 3) covers the pixels with
    # i + j < 3 (top and left edges in, the hypotenuse out); sampled at + 0.5 it would cover those with i + j < 2
    tri = np.array([[0, 0], [3, 0], [0, 3]]) * ref.FIX
    assert np.array_equal(ref.coverage(tri, H, W), i + j < 3)
    assert np.array_equal(ref.coverage(tri, H, W, bug="half_pixel"), i + j < 2)


def test_ties_go_to_the_smaller_face_and_the_order_of_faces_does_not_matter():
    pix, faces, _ = ref.fan_polygon(1)
    verts = ref.screen_mesh(pix)
    c2w, K = ref.screen_camera()
    H, W = 12, 16
    base = ref.rasterize(verts, faces, c2w, K, H, W)
    assert base["mask"].sum() > 50 and base["bad"] == 0 and base["n_skipped"] == 0
    doubled = np.concatenate([faces, faces])                          # face k + 8 is face k again: every covered pixel is an exact tie
    tie = ref.rasterize(verts, doubled, c2w, K, H, W)
    assert np.array_equal(tie["face_id"], base["face_id"])
    wrong = ref.rasterize(verts, doubled, c2w, K, H, W, bug="tie_larger")
    assert np.array_equal(wrong["face_id"][base["mask"]], base["face_id"][base["mask"]] + 8), "the injected tie rule must show"
    perm = np.random.default_rng(0).permutation(len(faces))
    shuffled = ref.rasterize(verts, faces[perm], c2w, K, H, W)
    assert np.array_equal(np.where(shuffled["mask"], perm[np.maximum(shuffled["face_id"], 0)], -1), base["face_id"])
    assert np.array_equal(shuffled["depth"], base["depth"])


@pytest.fixture(scope="module")
def sphere_case():
    from nerfart_amd import scene
    H, W = 24, 32
    c2w, K = (t.numpy() for t in scene.camera(H, W))
    verts, faces = ref.sphere_mesh(12)
    return verts, faces, c2w, K, H, W, ref.rasterize(verts, faces, c2w, K, H, W)


def _cast(verts, faces, c2w, K, H, W):
    """Float64 Moeller-Trumbore of every pixel's lifted ray against the unsnapped triangles: (face [H W], t, b1, b2, |d|)."""
    o, d = ref.lift_rays(c2w, K, H, W)
    v = verts.astype(np.float64)
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    face, t, b1, b2 = np.full(H * W, -1), np.full(H * W, np.inf), np.zeros(H * W), np.zeros(H * W)
    for p in range(H * W):
        tt, bb1, bb2 = ref.moller_trumbore(o, d[p], v0, v1, v2)
        k = int(np.argmin(tt))
        if np.isfinite(tt[k]):
            face[p], t[p], b1[p], b2[p] = k, tt[k], bb1[k], bb2[k]
    return face, t, b1, b2, np.linalg.norm(d, axis=1)


def test_the_rasterised_face_is_the_first_hit_of_the_pixels_ray(sphere_case):
    """Away from projected edges (more than 1/128 pixel: the snap moves an edge by at most sqrt(2) / 512) the rasterised face is the face float64 ray
    casting hits first, and depth and barycentrics agree.  The two differ in where the vertices are: the rasteriser takes them in camera space
    through w2c rounded to fp32 and rounds them to fp32 again, each coordinate off by at most 2^-24 (|px| + |py| + |pz| + 2.5) + 2^-24 * 3.2 <=
    2^-24 * 8 for this scene (|p| <= 0.61, camera at 2.5), so a vertex moves by eps <= 2^-24 * 8 sqrt(3).  The moved plane still passes within eps
    of the old hit point (the same barycentric mix of moved vertices), so along the unit ray the hit moves by at most eps / |cos| - allowed: 2
    eps / |cos| for the normal's own tilt -, and a barycentric by (vertex move + hit move) / altitude <= 4 eps / (|cos| h_min)."""
    verts, faces, c2w, K, H, W, ras = sphere_case
    pr = ref.project(verts, c2w, K)
    assert pr["valid"].all()
    far = (ref.edge_distance(pr["u"], pr["v"], faces, H, W, pr["valid"]) > 1.0 / 128).reshape(-1)
    face, t, b1, b2, dn = _cast(verts, faces, c2w, K, H, W)
    hit = face >= 0
    assert far.sum() > 0.9 * H * W and (hit & far).sum() > 150 and (~hit & far).sum() > 150
    assert np.array_equal(ras["face_id"][far], face[far]), "the rasterised face is not the first hit"
    sel = hit & far
    cam = pr["cam"]
    worst_d, worst_b = 0.0, 0.0
    for p in np.nonzero(sel)[0]:
        a, b, c, n, _ = ref.face_plane(cam, faces[face[p]])
        x, y = (q.reshape(-1)[p] for q in ref.pixel_rays(ref.camera_numbers(c2w, K)[2], H, W))
        r = np.array([x, y, 1.0])
        cos = abs(np.dot(n, r)) / (np.linalg.norm(n) * np.linalg.norm(r))
        h_min = np.linalg.norm(n) / max(np.linalg.norm(b - a), np.linalg.norm(c - b), np.linalg.norm(a - c))
        bound_d, bound_b = 2 * EPS_CAM / cos, 4 * EPS_CAM / (cos * h_min)
        err_d = abs(ras["depth"][p] - t[p] * dn[p])
        err_b = np.abs(ras["bary"][p] - np.array([1 - b1[p] - b2[p], b1[p], b2[p]])).max()
        worst_d, worst_b = max(worst_d, err_d / bound_d), max(worst_b, err_b / bound_b)
        assert err_d <= bound_d and err_b <= bound_b, (p, err_d, bound_d, err_b, bound_b)
    print(f"[raster ref] sphere N = 12, {int(sel.sum())} pixels: worst depth error / bound {worst_d:.3f}, worst barycentric error / bound {worst_b:.3f}")
    assert np.all(np.abs(ras["bary"][sel].sum(axis=1) - 1) < 1e-9) and ras["bary"][sel].min() > -1e-6
    # the normals: unit, toward the camera
    o, d = ref.lift_rays(c2w, K, H, W)
    assert np.all(np.abs(np.linalg.norm(ras["normals"][sel], axis=1) - 1) < 1e-12) and np.all(np.einsum("pk,pk->p", ras["normals"][sel], d[sel]) < 0)


def test_injected_depth_and_offset_bugs_are_caught(sphere_case):
    verts, faces, c2w, K, H, W, ras = sphere_case
    face, t, b1, b2, dn = _cast(verts, faces, c2w, K, H, W)
    sel = (face >= 0) & (ras["face_id"] == face)
    assert np.all(np.abs(ras["depth"][sel] - t[sel] * dn[sel]) < 1e-5)
    wrong = ref.rasterize(verts, faces, c2w, K, H, W, bug="camera_z")
    assert np.abs(wrong["depth"][sel] - t[sel] * dn[sel]).max() > 1e-2, "camera z is not the distance along the unit ray off the axis"
    half = ref.rasterize(verts, faces, c2w, K, H, W, bug="half_pixel")
    assert (half["face_id"] != face).mean() > 0.05, "a half-pixel offset sees other faces than the pixel's ray"


def test_bilinear_returns_an_affine_texture():
    Ht, Wt = 15, 20
    y, x = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    image = np.stack([3 * x + 2 * y + 10, 5 * x + 100 - 4 * y, 7 * y + x], axis=-1).astype(np.uint8)
    assert image.max() < 256 and np.array_equal(image[..., 0], 3 * x + 2 * y + 10)
    rng = np.random.default_rng(5)
    uv = np.stack([rng.uniform(0.5, Wt - 0.5, 400), rng.uniform(0.5, Ht - 0.5, 400)], axis=-1)
    uv[:4] = [[0.5, 0.5], [Wt - 0.5, Ht - 0.5], [3.5, 7.5], [3.0, 7.0]]                              # texel centres and a texel corner
    uv = uv.astype(np.float32)
    X, Y = uv[:, 0].astype(np.float64) - 0.5, uv[:, 1].astype(np.float64) - 0.5
    want = np.stack([3 * X + 2 * Y + 10, 5 * X + 100 - 4 * Y, 7 * Y + X], axis=-1) / 255.0
    got = ref.sample_bilinear(uv, image)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 8 * ref.U32, np.abs(got - want).max()
    assert np.array_equal(got[2], image[7, 3].astype(np.float32) / np.float32(255))
    for bug in ("no_half_texel", "v_flip"):
        assert np.abs(ref.sample_bilinear(uv, image, bug=bug) - want).max() > 1.0 / 255, bug
    # clamp to edge, misses and non-finite coordinates
    edge = ref.sample_bilinear(np.array([[-3.0, -2.0], [Wt + 5.0, Ht + 9.0], [np.nan, 1.0], [2.0, 2.0]], np.float32), image, mask=np.array([1, 1, 1, 0]),
                               background=(0.25, 0.5, 0.75))
    assert np.array_equal(edge[0], image[0, 0] / np.float32(255)) and np.array_equal(edge[1], image[-1, -1] / np.float32(255))
    assert np.array_equal(edge[2], np.float32([0.25, 0.5, 0.75])) and np.array_equal(edge[3], edge[2])


def test_interp_is_the_barycentric_mix():
    rng = np.random.default_rng(2)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    attr = rng.normal(size=(4, 3)).astype(np.float32)
    bary = rng.dirichlet(np.ones(3), size=6).astype(np.float32)
    fid = np.array([0, 1, -1, 1, 0, -1])
    got = ref.interp(fid, bary, attr, faces, fill=9.0)
    want = np.einsum("pk,pkc->pc", bary.astype(np.float64), attr.astype(np.float64)[faces[np.maximum(fid, 0)]])
    assert np.all(got[fid < 0] == 9.0) and np.abs(got - want)[fid >= 0].max() < 1e-6
    corner = rng.normal(size=(2, 3, 2)).astype(np.float32)
    got = ref.interp(fid, bary, corner, None, fill=-1.0)
    want = np.einsum("pk,pkc->pc", bary.astype(np.float64), corner.astype(np.float64)[np.maximum(fid, 0)])
    assert np.all(got[fid < 0] == -1.0) and np.abs(got - want)[fid >= 0].max() < 1e-6


# ---- the readers ------------------------------------------------------------------------------------------------------------------------------

def test_read_ply_gives_back_what_write_ply_wrote(tmp_path):
    from nerfart_amd import mesh_util
    rng = np.random.default_rng(1)
    v = rng.normal(size=(37, 3)).astype(np.float32)
    f = rng.integers(0, 37, size=(50, 3)).astype(np.int32)
    n = rng.normal(size=(37, 3)).astype(np.float32)
    c = rng.integers(0, 256, size=(37, 3)).astype(np.uint8)
    for k, (nn, cc) in enumerate(((None, None), (n, None), (None, c), (n, c))):
        got = mesh_util.read_ply(mesh_util.write_ply(str(tmp_path / f"m{k}.ply"), v, f, nn, cc))
        assert np.array_equal(got["verts"].view(np.int32), v.view(np.int32)) and np.array_equal(got["faces"], f) and got["faces"].dtype == np.int32
        for key, a in (("normals", nn), ("colors", cc)):
            assert (got[key] is None) if a is None else (got[key].dtype == a.dtype and np.array_equal(got[key], a))
    empty = mesh_util.read_ply(mesh_util.write_ply(str(tmp_path / "e.ply"), v[:0], f[:0]))
    assert empty["verts"].shape == (0, 3) and empty["faces"].shape == (0, 3)
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="write_ply"):
        mesh_util.read_ply(str(tmp_path / "bad.ply"))


@pytest.mark.parametrize("F,P,with_normals", [(7, 4, True), (20001, 2, False)])
def test_read_obj_gives_back_what_write_obj_wrote(tmp_path, F, P, with_normals):
    from nerfart_amd import mesh_util
    rng = np.random.default_rng(F)
    V = 3 * F // 2 + 5
    v = (rng.normal(size=(V, 3)) * 3).astype(np.float32)
    f = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    n = rng.normal(size=(V, 3)).astype(np.float32) if with_normals else None
    uv = mesh_util.atlas_uvs(F, P)
    _, _, _, W, H = mesh_util.atlas_layout(F, P)
    image = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    got = mesh_util.read_obj(mesh_util.write_obj(str(tmp_path / "m.obj"), v, f, uv, image, n))
    assert np.array_equal(got["verts"].view(np.int32), v.view(np.int32)) and np.array_equal(got["faces"], f) and got["faces"].dtype == np.int32
    assert np.array_equal(got["uv"], uv), "the pixel UVs do not come back exactly"
    assert np.array_equal(got["image"], image)
    assert (got["normals"] is None) if n is None else np.array_equal(got["normals"].view(np.int32), n.view(np.int32))
    with open(tmp_path / "m.obj", "a") as out:
        out.write("g group\n")
    with pytest.raises(ValueError, match="unexpected line"):
        mesh_util.read_obj(str(tmp_path / "m.obj"))
