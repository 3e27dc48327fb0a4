"""csrc/mesh_raster.hip (mesh_util.rasterize / render_mesh) against the numpy statement tests/mesh_raster_ref.py, which tests/test_mesh_raster_ref.py
holds to a rasteriser's properties - stage by stage.  Projection: snapped positions and validity by equality, camera-space points equal to the
float64 result rounded once.  Raster + resolve, from the kernel's own snapped positions: the face of every pixel by equality (except where the
reference's two nearest candidates are closer than 2^-20 relative in z), depth, z and barycentrics within 2 fp32 ulp of float64, guard rows
intact, a second run the same bits.  Interpolation and bilinear sampling within 2 ulp of the stated order of operations.  End to end on the two
scene models at N = 48: a baked affine colour comes back at every covered pixel, a frame from the written files is the frame from the tensors
bit for bit, and depth agrees with surface_render's sphere tracing within the bound a marching-cubes face allows.

Observed on an MI355X (first run; every assertion is observed <= allowed): no pixel of any case fell under the near-tie exception; z and depth at
most 0.500 ulp from float64, barycentrics and normals 0.25 x 2^-23 (allowed 2); interp and bilinear bit-equal to the stated order; the baked affine
colour within 0.4812 (VolSDF) and 0.4796 (NeuS) levels (allowed 0.5 + 0.00255); depth against sphere tracing, in grid steps: VolSDF median 0.013,
max 0.108 over 739 pixels, NeuS median 0.028, max 0.206 over 147 (allowed 3.464); every mesh pixel inside mask_surface."""
import numpy as np
import pytest
import torch

import mesh_pipeline_ref
import mesh_raster_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_F, GUARD_I = 1.0e30, 0x5A5A5A5A
NEAR = 1e-3
IMAGES = [(12, 16), (17, 33), (64, 64)]                               # (H, W)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=dtype))).to(DEV)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- projection -------------------------------------------------------------------------------------------------------------------------------

def _check_project(verts, c2w, K, near=NEAR):
    from nerfart_amd import hip
    want = ref.project(verts, c2w, K, near)
    ok = want["valid"]
    with np.errstate(all="ignore"):
        tie = np.abs(np.stack([want["u"], want["v"]], axis=-1)[ok] * ref.FIX % 1.0 - 0.5)
    assert tie.size == 0 or tie.min() >= 1e-6, "the reference's snapped coordinate is too close to a rounding tie: choose another seed"
    xy_fix, cam, valid = hip.mesh_project(dev(verts, np.float32), hip.mesh_camera(c2w, K), near)
    assert np.array_equal(valid.cpu().numpy().astype(bool), ok), "valid"
    assert np.array_equal(xy_fix.cpu().numpy().astype(np.int64), want["xy_fix"]), "xy_fix"
    fin = np.isfinite(want["cam"]).all(axis=1)
    with np.errstate(all="ignore"):
        assert np.array_equal(cam.cpu().numpy()[fin].view(np.int32), want["cam"][fin].astype(np.float32).view(np.int32)), "cam is not float64 rounded once"
    assert not np.isfinite(cam.cpu().numpy()[~fin]).all(axis=1).any()
    return want


def test_project_is_the_float64_projection_snapped_once():
    from nerfart_amd import scene
    rng = np.random.default_rng(7)
    V = 1000 + 37                                                     # five blocks of 256, the last ragged
    verts = rng.uniform(-1.2, 1.2, size=(V, 3)).astype(np.float32)
    c2w, K = (t.numpy().copy() for t in scene.camera(33, 17, angle=0.7))
    K[0, 1] = 0.3                                                     # skew
    loc, right, fwd = c2w[:3, 3], c2w[:3, 0], c2w[:3, 2]
    verts[3] = loc - 0.1 * fwd                                        # behind the camera
    verts[4] = [np.nan, 0.0, 0.0]
    verts[5] = loc + 0.0005 * fwd                                     # in front of the camera, closer than near = 1e-3
    verts[6] = loc + 0.01 * fwd + 900.0 * right                       # far beyond 2^15 pixels
    want = _check_project(verts, c2w, K)
    assert not want["valid"][3:7].any() and want["valid"].sum() > V - 8
    # the limits themselves, where everything is exact: identity pose, fx = 64, cx = cy = 0
    c2w, K = ref.screen_camera()
    near = float(np.float32(NEAR))
    edge = np.array([[0, 0, near], [0, 0, np.nextafter(np.float32(near), np.float32(0))], [512.0, 0, 1.0], [np.nextafter(np.float32(512), np.float32(600)), 0, 1.0],
                     [0, -512.0, 1.0], [0.2578125, 0.51171875, 1.0]], dtype=np.float32)
    want = _check_project(edge, c2w, K)
    assert want["valid"].tolist() == [True, False, True, False, True, True] and want["xy_fix"][2].tolist() == [2 ** 23, 0]
    assert want["xy_fix"][5].tolist() == [int(0.2578125 * 64 * 256), int(0.51171875 * 64 * 256)]


# ---- raster + resolve -------------------------------------------------------------------------------------------------------------------------

def _poly(fn):
    def make(H, W):
        pix, faces, _ = fn(4 if (H, W) == (64, 64) else 1)
        return (ref.screen_mesh(pix), faces) + ref.screen_camera()
    return make


def _hand(H, W):
    """Single triangles, each on vertices of its own (pixel coordinates, camera depth 1 unless said)."""
    tris = [
        [[6.25, 1.25], [6.75, 1.3125], [6.375, 1.75]],               # 0: smaller than a pixel, covers no sample
        [[2.5, 2.5], [3.75, 2.75], [2.75, 3.75]],                     # 1: covers exactly the sample (3, 3)
        [[4, 4], [8, 5], [5, 8]],                                     # 2: a vertex on a pixel centre
        [[1, 1], [5, 5], [9, 9]],                                     # 3: degenerate
        [[10, 2], [12, 2], [11, 4]],                                  # 4: one vertex behind near (below)
        [[-20, -20], [-10, -20], [-20, -10]],                         # 5: wholly off screen
    ]
    verts = ref.screen_mesh(np.array(tris, dtype=np.float64).reshape(-1, 2))
    verts[4 * 3 + 2] = [11 / 64.0, 4 / 64.0, -1.0]
    return (verts, np.arange(18, dtype=np.int32).reshape(6, 3)) + ref.screen_camera()


def _hand_bad(H, W):
    verts, faces, c2w, K = _hand(H, W)
    faces = faces.copy()
    faces[5] = [0, 18, 1]                                             # past the end
    return verts, np.concatenate([faces, [[2, -1, 3]]]).astype(np.int32), c2w, K


def _whole(H, W):
    return (ref.screen_mesh([[-10, -10], [200, -10], [-10, 200]]), np.array([[0, 1, 2]], np.int32)) + ref.screen_camera()


def _mix(H, W):
    """The whole-image triangle behind a fan and a grid: faces of the large-face launch and of the per-thread walk in one mesh."""
    s = 4 if (H, W) == (64, 64) else 1
    (p0, f0, _), (p1, f1, _) = ref.fan_polygon(s), ref.grid_polygon(1)
    parts = [(ref.screen_mesh([[-10, -10], [200, -10], [-10, 200]], z=4.0), np.array([[0, 1, 2]])), (ref.screen_mesh(p0, z=2.0), f0), (ref.screen_mesh(p1, z=1.0), f1)]
    verts, faces, base = [], [], 0
    for v, f in parts:
        verts.append(v)
        faces.append(np.asarray(f) + base)
        base += len(v)
    return (np.concatenate(verts), np.concatenate(faces).astype(np.int32)) + ref.screen_camera()


def _quads(H, W):
    """Two quads through each other: 1 / z is linear on screen, A runs 1 -> 1/2 over x = 2 .. 14, B 1/2 -> 1 over x = 2 .. 15; they cross at
    x = 8.24, on no pixel centre."""
    def quad(x0, z0, x1, z1):
        return np.array([[x0 * z0, 2 * z0, z0], [x1 * z1, 2 * z1, z1], [x1 * z1, 10 * z1, z1], [x0 * z0, 10 * z0, z0]]) * [1 / 64.0, 1 / 64.0, 1.0]
    verts = np.concatenate([quad(2, 1.0, 14, 2.0), quad(2, 2.0, 15, 1.0)]).astype(np.float32)
    return (verts, np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)) + ref.screen_camera()


def _sphere(H, W):
    from nerfart_amd import scene
    c2w, K = (t.numpy() for t in scene.camera(H, W, angle=0.4))
    return ref.sphere_mesh(12) + (c2w, K)


CASES = {"grid": _poly(ref.grid_polygon), "fan": _poly(ref.fan_polygon), "hand": _hand, "hand_bad": _hand_bad, "whole": _whole, "mix": _mix,
         "quads": _quads, "sphere": _sphere}


def raw_pipeline(gv, gf, camera, H, W, near=NEAR):
    """project, raster, resolve through the C entry points into guarded buffers (one row more than asked for, filled beforehand): dict of tensors.
    Asserts that the guard rows survived and that every element before them was written."""
    from nerfart_amd import hip
    V, F, n = gv.shape[0], gf.shape[0], H * W
    import ctypes as C
    ptr, stream = (lambda a: C.cast(a, C.c_void_p)), torch.cuda.current_stream().cuda_stream
    w2c, rot, k5 = camera
    full = lambda shape, value, dtype: torch.full(shape, value, dtype=dtype, device=DEV)
    xy_fix, cam, valid = full((V + 1, 2), GUARD_I, torch.int32), full((V + 1, 3), GUARD_F, torch.float32), full((V + 1,), 0x5A, torch.uint8)
    assert hip.lib.nerfart_mesh_project(gv.data_ptr(), V, ptr(w2c), ptr(k5), near, xy_fix.data_ptr(), cam.data_ptr(), valid.data_ptr(), stream) == 0
    zbuf, work, info = full((n + 1,), GUARD_I, torch.int64), full((F + 1,), GUARD_I, torch.int32), full((5,), GUARD_I, torch.int32)
    assert hip.lib.nerfart_mesh_raster(xy_fix.data_ptr(), cam.data_ptr(), valid.data_ptr(), gf.data_ptr(), V, F, ptr(k5), near, H, W, zbuf.data_ptr(),
                                       work.data_ptr(), info.data_ptr(), stream) == 0, hip.lib.nerfart_last_error()
    out = {"face_id": full((n + 1,), GUARD_I, torch.int32), "bary": full((n + 1, 3), GUARD_F, torch.float32), "z": full((n + 1,), GUARD_F, torch.float32),
           "depth": full((n + 1,), GUARD_F, torch.float32), "mask": full((n + 1,), 0x5A, torch.uint8), "face_normals": full((n + 1, 3), GUARD_F, torch.float32)}
    assert hip.lib.nerfart_mesh_resolve(zbuf.data_ptr(), cam.data_ptr(), gf.data_ptr(), V, F, ptr(k5), ptr(rot), H, W,
                                        *(out[k].data_ptr() for k in ("face_id", "bary", "z", "depth", "mask", "face_normals")), stream) == 0
    out.update(xy_fix=xy_fix, cam=cam, valid=valid, zbuf=zbuf, info=info)
    for k, t in out.items():
        guard = GUARD_F if t.dtype == torch.float32 else (0x5A if t.dtype == torch.uint8 else GUARD_I)
        assert bool((t[-1] == guard).all()), f"{k}: the row past the end was written"
        assert not bool((t[:-1] == guard).any()), f"{k}: an element was not written"
        out[k] = t[:-1]
    n_large = int(out["info"][3])
    assert bool((work[n_large:] == GUARD_I).all()) and not bool((work[:n_large] == GUARD_I).any()), "the large-face list"
    return out


@pytest.mark.parametrize("H,W", IMAGES)
@pytest.mark.parametrize("name", list(CASES))
def test_raster_and_resolve_are_the_reference(name, H, W):
    from nerfart_amd import hip, mesh_util
    verts, faces, c2w, K = CASES[name](H, W)
    gv, gf = dev(verts, np.float32), dev(faces, np.int32)
    camera = hip.mesh_camera(c2w, K)
    got = raw_pipeline(gv, gf, camera, H, W)
    g = {k: t.cpu().numpy() for k, t in got.items()}
    want = ref.rasterize(verts, faces, c2w, K, H, W, NEAR, xy_fix=g["xy_fix"], cam32=g["cam"], valid=g["valid"])
    bad, n_skipped, n_rejected, n_large = (int(c) for c in g["info"])
    assert (bad, n_skipped, n_rejected) == (want["bad"], want["n_skipped"], want["n_rejected"])
    covered = want["mask"]
    with np.errstate(all="ignore"):
        close = covered & (want["second_z"] - want["first_z"] < 2.0 ** -20 * want["first_z"])
    assert close.sum() <= 0.005 * covered.sum(), f"{int(close.sum())} of {int(covered.sum())} covered pixels have two candidates within 2^-20: choose other inputs"
    same = ~close
    assert np.array_equal(g["face_id"][same], want["face_id"][same]), "face_id"
    assert np.all((g["face_id"][close] >= 0)) and np.array_equal(g["mask"].astype(bool), g["face_id"] >= 0)
    hit = same & covered
    miss = g["face_id"] < 0
    for k in ("bary", "z", "depth", "face_normals"):
        assert np.all(g[k][miss] == 0.0), f"{k} of a miss is not 0"
    wz, wd = want["z"][hit], want["depth"][hit]
    ratio = {"z": np.abs(g["z"][hit] - wz) / ulp32(wz), "depth": np.abs(g["depth"][hit] - wd) / ulp32(wd),
             "bary": np.abs(g["bary"][hit] - want["bary"][hit]) / 2.0 ** -23, "normals": np.abs(g["face_normals"][hit] - want["normals"][hit]) / 2.0 ** -23}
    print(f"[raster] {name} {W} x {H}: F = {len(faces)}, {int(covered.sum())} covered, {int(close.sum())} close, {n_large} large faces, n_skipped = "
          f"{n_skipped}, n_rejected = {n_rejected}; worst error " + ", ".join(f"{k} {v.max() if v.size else 0.0:.3f}" for k, v in ratio.items())
          + " (ulp resp. 2^-23; allowed 2)")
    for k, v in ratio.items():
        assert v.size == 0 or v.max() <= 2.0, k
    # what each case is there for
    count = lambda f: int((g["face_id"] == f).sum())
    if name in ("grid", "fan"):
        s = 4 if (H, W) == (64, 64) else 1
        pix, _, _ = (ref.grid_polygon if name == "grid" else ref.fan_polygon)(s)
        assert np.array_equal(g["xy_fix"], np.rint(pix * ref.FIX).astype(np.int64)), "the polygon's vertices must project exactly"
        assert np.array_equal(g["mask"].reshape(H, W).astype(bool), ref.union_coverage(pix, faces, H, W) == 1) and covered.sum() > 50
        assert np.all(g["z"][hit] == 1.0)
    elif name == "hand":
        assert n_skipped == 1 and bad == 0 and [count(f) for f in range(6)] == [0, 1, count(2), 0, 0, 0] and count(2) > 5
        assert g["face_id"].reshape(H, W)[3, 3] == 1 and g["face_id"].reshape(H, W)[4, 4] == -1
    elif name == "hand_bad":
        assert bad == 1 and n_skipped == 1 and count(1) == 1 and count(5) == 0 and count(6) == 0
        with pytest.raises(ValueError, match="face holds a vertex index outside"):
            mesh_util.rasterize(gv, gf, c2w, K, H, W, NEAR)
    elif name == "whole":
        assert n_large == (1 if H * W > 256 else 0) and bool(g["mask"].all()) and np.all(g["face_id"] == 0)      # 16 x 12 fits the per-thread walk
    elif name == "mix":
        assert n_large >= (1 if H * W > 256 else 0) and bool(g["mask"].all()) and len(np.unique(g["face_id"])) > 10 and len(faces) % 64 != 0
    elif name == "quads":
        ids = g["face_id"].reshape(H, W)[5]
        assert set(ids[2:9]) <= {0, 1} and set(ids[9:14]) <= {2, 3} and ids[14] in (2, 3) and n_large == 0
    elif name == "sphere":
        assert covered.sum() > 40 and len(np.unique(g["face_id"])) > 20 and len(faces) % 64 != 0
    # a second run gives the same bits, and so do the wrappers that allocate for themselves
    again = raw_pipeline(gv, gf, camera, H, W)
    for k in ("xy_fix", "cam", "valid", "zbuf", "face_id", "bary", "z", "depth", "mask", "face_normals"):
        a, b = got[k], again[k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    assert torch.equal(got["info"][:3], again["info"][:3])
    if not bad:
        r = mesh_util.rasterize(gv, gf, c2w, K, H, W, NEAR)
        for k in ("face_id", "bary", "z", "depth", "mask", "face_normals"):
            assert torch.equal(r[k].view(torch.int32) if r[k].dtype == torch.float32 else r[k],
                               got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k]), k
        assert (r["n_skipped"], r["n_rejected"]) == (n_skipped, n_rejected)


def test_the_image_does_not_depend_on_the_order_of_the_faces():
    from nerfart_amd import mesh_util
    H, W = 64, 64
    verts, faces, c2w, K = _mix(H, W)
    perm = np.random.default_rng(1).permutation(len(faces))
    a = mesh_util.rasterize(dev(verts, np.float32), dev(faces, np.int32), c2w, K, H, W)
    b = mesh_util.rasterize(dev(verts, np.float32), dev(faces[perm], np.int32), c2w, K, H, W)
    assert torch.equal(dev(perm)[b["face_id"].long()].int(), a["face_id"]) and bool(a["mask"].all())
    for k in ("z", "depth", "bary", "face_normals"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_refusals():
    from nerfart_amd import hip, mesh_util
    verts, faces, c2w, K = _whole(12, 16)
    gv, gf = dev(verts, np.float32), dev(faces, np.int32)
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.rasterize(gv.cpu(), gf.cpu(), c2w, K, 12, 16)
    with pytest.raises(ValueError, match="H and W"):
        mesh_util.rasterize(gv, gf, c2w, K, 0, 16)
    with pytest.raises(ValueError, match="H and W"):
        mesh_util.rasterize(gv, gf, c2w, K, 12, 16385)
    with pytest.raises(ValueError, match="near"):
        mesh_util.rasterize(gv, gf, c2w, K, 12, 16, near=0.0)
    with pytest.raises(hip.NerfartHipError, match="int32"):
        mesh_util.rasterize(gv, gf.long(), c2w, K, 12, 16)
    flat = K.copy()
    flat[0, 0] = 0.0
    with pytest.raises(hip.NerfartHipError, match="fx and fy"):
        mesh_util.rasterize(gv, gf, c2w, flat, 12, 16)
    with pytest.raises(ValueError, match="go together"):
        mesh_util.render_mesh(gv, gf, c2w, K, 12, 16, uv=np.zeros((1, 3, 2)))
    empty = mesh_util.rasterize(gv[:0], gf[:0], c2w, K, 12, 16)                                 # no mesh: an empty frame
    assert not bool(empty["mask"].any()) and bool((empty["face_id"] == -1).all()) and empty["n_skipped"] == 0


# ---- interpolation and sampling ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 2, 3, 8])
@pytest.mark.parametrize("per_corner", [False, True])
def test_interp_is_the_stated_order_of_operations(C, per_corner):
    from nerfart_amd import hip
    rng = np.random.default_rng(10 * C + per_corner)
    n, V, F = 1000 + 37, 50, 91
    faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    face_id = rng.integers(-1, F, size=n).astype(np.int32)
    face_id[:3] = [-1, F - 1, 0]
    bary = rng.dirichlet(np.ones(3), size=n).astype(np.float32)
    bary[5] = [1.25, -0.125, -0.125]                                  # extrapolated weights
    attr = (rng.normal(size=(F, 3, C)) if per_corner else rng.normal(size=(V, C))).astype(np.float32) * 3
    want = ref.interp(face_id, bary, attr, None if per_corner else faces, fill=-7.5)
    got = hip.mesh_interp(dev(face_id), dev(bary), dev(attr), None if per_corner else dev(faces), fill=-7.5).cpu().numpy()
    assert got.shape == (n, C) and np.all(got[face_id < 0] == np.float32(-7.5)) and (face_id < 0).sum() > 3
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp32(want)
    print(f"[raster] interp C = {C}, per_corner = {per_corner}: worst error {err.max():.2f} ulp (allowed 2), {int((err > 0).sum())} of {err.size} differ")
    assert err.max() <= 2.0


def test_bilinear_is_the_stated_order_of_operations():
    from nerfart_amd import hip
    rng = np.random.default_rng(4)
    Ht, Wt, n = 37, 53, 2000 + 11
    image = rng.integers(0, 256, size=(Ht, Wt, 3)).astype(np.uint8)
    uv = np.stack([rng.uniform(-2.0, Wt + 2.0, n), rng.uniform(-2.0, Ht + 2.0, n)], axis=-1).astype(np.float32)
    uv[:6] = [[0.5, 0.5], [Wt - 0.5, Ht - 0.5], [10.0, 10.0], [np.nan, 3.0], [3.0, np.inf], [-1e9, 1e9]]
    mask = (rng.uniform(size=n) > 0.2).astype(np.uint8)
    mask[:6] = 1
    bg = (0.25, 0.5, 0.125)
    want = ref.sample_bilinear(uv, image, mask, bg)
    got = hip.mesh_sample_bilinear(dev(uv), dev(image), dev(mask), bg).cpu().numpy()
    dead = (mask == 0) | ~np.isfinite(uv).all(axis=1)
    assert np.array_equal(got[dead], np.broadcast_to(np.float32(bg), got[dead].shape)) and dead.sum() > 100
    assert np.array_equal(got[0], image[0, 0] / np.float32(255)) and np.array_equal(got[1], image[-1, -1] / np.float32(255))
    assert np.array_equal(got[5], image[-1, 0] / np.float32(255)), "clamp to edge"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp32(np.maximum(want, 2.0 ** -10))
    print(f"[raster] bilinear: worst error {err.max():.2f} ulp (allowed 2), {int((err > 0).sum())} of {err.size} differ")
    assert err.max() <= 2.0
    no_mask = hip.mesh_sample_bilinear(dev(uv), dev(image)).cpu().numpy()
    live = np.isfinite(uv).all(axis=1)
    assert np.array_equal(no_mask[live & ~dead], got[live & ~dead]) and np.abs(no_mask[live] - ref.sample_bilinear(uv, image)[live]).max() < 1e-6


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------

N, VOLUME_SIZE, FACTOR, PATCH, SIDE = 48, 3.0, 2, 2, 32


@pytest.fixture(scope="module", params=["VolSDF", "NeuS"])
def model(request):
    from nerfart_amd import scene
    return scene.build_model(request.param, seed=0, beta=0.01 if request.param == "VolSDF" else None, device=DEV, precision="mixed")[0]


@pytest.fixture(scope="module")
def decimated(model):
    """(vertices in the model's frame, in the placement frame, faces) of extract_mesh(simplify_factor=FACTOR), by hand."""
    return mesh_pipeline_ref.decimated(model.implicit_surface, N, VOLUME_SIZE, FACTOR)


def _camera():
    from nerfart_amd import scene
    return scene.camera(SIDE, SIDE)


def test_a_baked_affine_colour_comes_back_at_every_covered_pixel(model, decimated):
    """bake_texture(project=0) of an affine colour with values in [0.1, 0.9] at every texel; render_mesh(uv=, image=) must give, at every covered
    pixel, that function at the pixel's hit point within (0.5 + 0.00255) / 255: quantisation moves a texel by at most half a level, a bilinear
    sample is a convex mix of texels of the one face, and 1e-5 covers the fp32 evaluation - the bound tests/test_gpu_mesh_texture.py uses."""
    from nerfart_amd import mesh_util
    pts, _, faces = decimated
    c2w, K = _camera()
    points, face_of = mesh_util.texel_points(pts, faces, PATCH)
    ok = face_of.reshape(-1) >= 0
    tex_pts = points[ok].double().cpu().numpy()
    rng = np.random.default_rng(3)
    centre = tex_pts.mean(axis=0)
    A = rng.normal(size=(3, 3))
    A *= 0.4 / np.abs((tex_pts - centre) @ A).max()
    tA, tc = dev(A, np.float64), dev(centre, np.float64)
    image, uv = mesh_util.bake_texture(pts, faces, lambda p: (0.5 + (p.double() - tc) @ tA).float(), patch=PATCH, project=0)
    rgb, depth, extras = mesh_util.render_mesh(pts, faces, c2w, K, SIDE, SIDE, uv=uv, image=image, background=(1.0, 0.0, 1.0))
    mask = extras["mask_mesh"].cpu().numpy()
    o, d = ref.lift_rays(c2w.numpy(), K.numpy(), SIDE, SIDE)
    hit = o[None] + depth.double().cpu().numpy()[:, None] * d / np.linalg.norm(d, axis=1, keepdims=True)
    want = 0.5 + (hit - centre) @ A
    err = np.abs(rgb.double().cpu().numpy() - want)[mask]
    print(f"[raster] {type(model).__name__}: F = {faces.shape[0]}, {int(mask.sum())} of {SIDE * SIDE} pixels covered, n_skipped = {extras['n_skipped']}; "
          f"worst |rendered - affine colour| = {err.max() * 255:.4f} levels (allowed 0.5 + 0.00255)")
    assert mask.sum() > 100 and (~mask).sum() > 100
    assert err.max() <= 0.5 / 255 + 1e-5
    assert np.array_equal(rgb.cpu().numpy()[~mask], np.broadcast_to(np.float32([1.0, 0.0, 1.0]), ((~mask).sum(), 3)))
    assert bool((depth[~extras["mask_mesh"]] == 0).all())


def test_a_frame_from_the_files_is_the_frame_from_the_tensors(model, decimated, tmp_path):
    from nerfart_amd import hip, mesh_util
    pts, placed, faces = decimated
    c2w, K = _camera()
    image, uv = mesh_util.bake_texture(pts, faces, lambda p: mesh_util.normal_view_radiance(model, p)[1], patch=PATCH)
    normals = hip.normalize_dirs(model.implicit_surface.forward_with_nablas(pts)[1].contiguous())
    a = mesh_util.render_mesh(placed, faces, c2w, K, SIDE, SIDE, uv=uv, image=image, normals=normals)
    obj = mesh_util.read_obj(mesh_util.write_obj(str(tmp_path / "m.obj"), placed, faces, uv, image, normals))
    b = mesh_util.render_mesh(dev(obj["verts"]), dev(obj["faces"]), c2w, K, SIDE, SIDE, uv=obj["uv"], image=dev(obj["image"]), normals=dev(obj["normals"]))
    assert len(torch.unique(a[0], dim=0)) > 16, "the frame is meant to vary"
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    for k in ("mask_mesh", "face_id"):
        assert torch.equal(a[2][k], b[2][k]), k
    for k in ("normals_mesh", "bary"):
        assert torch.equal(a[2][k].view(torch.int32), b[2][k].view(torch.int32)), k
    norm = a[2]["normals_mesh"].norm(dim=1)
    assert bool(((norm - 1).abs() < 1e-5)[a[2]["mask_mesh"]].all()) and bool((norm[~a[2]["mask_mesh"]] == 0).all())
    # per-vertex colours, the PLY way round
    colors = mesh_util.vertex_attributes(model, pts)[1]
    ply = mesh_util.read_ply(mesh_util.write_ply(str(tmp_path / "m.ply"), placed, faces, normals, colors))
    c = mesh_util.render_mesh(placed, faces, c2w, K, SIDE, SIDE, colors=colors)
    e = mesh_util.render_mesh(dev(ply["verts"]), dev(ply["faces"]), c2w, K, SIDE, SIDE, colors=dev(ply["colors"]))
    assert torch.equal(c[0].view(torch.int32), e[0].view(torch.int32)) and torch.equal(c[1].view(torch.int32), e[1].view(torch.int32))
    assert float(c[0].min()) >= 0.0 and float(c[0][c[2]["mask_mesh"]].max()) <= 1.0 + 1e-6


def test_depth_agrees_with_surface_render(model):
    """The refined, undecimated mesh in the model's frame against surface_render (sphere tracing) of the same camera, on pixels both hit whose face
    normal has |n . dir| >= 0.5.  A marching-cubes face lies in the cells its surface crosses, so along its normal it is at most a cell diagonal,
    sqrt(3) steps, from the surface, and the obliquity bound turns that into at most 2 sqrt(3) steps along the ray: every difference is at most
    2 sqrt(3) volume_size / N.  The observed figures are printed, and quoted in the module's docstring and in DESIGN.md 4.7."""
    from nerfart_amd import hip, mesh_util, rend_util, ray_casting
    surface = model.implicit_surface
    vol = mesh_util.sdf_volume(surface, VOLUME_SIZE, N)
    ws, counts = hip.mc_count(vol, 0.0)
    V, F, bad = (int(c) for c in counts.cpu())
    assert not bad and F > 1000
    origin, spacing = mesh_util.model_frame(N, VOLUME_SIZE)
    _, faces = hip.mc_emit(vol, 0.0, origin, spacing, ws, V, F)
    edge, t, _ = mesh_util.refine_vertices(surface, vol, 0.0, ws, V, VOLUME_SIZE, 4)
    verts = hip.mesh_edge_points(edge, t, vol.shape, origin, spacing)
    c2w, K = _camera()
    rgb, depth, extras = mesh_util.render_mesh(verts, faces, c2w, K, SIDE, SIDE)
    rays_o, rays_d, _ = rend_util.get_rays(c2w[None].to(DEV), K[None].to(DEV), SIDE, SIDE)
    _, depth_s, ex = ray_casting.surface_render(rays_o, rays_d, model, calc_normal=False, ray_casting_algo="sphere_tracing",
                                                ray_casting_cfgs=dict(near=0.0, far=6.0, N_iters=20))
    mask_m, mask_s = extras["mask_mesh"], ex["mask_surface"].reshape(-1)
    dirs = torch.nn.functional.normalize(rays_d.reshape(-1, 3), dim=-1)
    facing = (extras["normals_mesh"] * dirs).sum(dim=1).abs() >= 0.5
    both = mask_m & mask_s & facing
    step = VOLUME_SIZE / N
    diff = ((depth - depth_s.reshape(-1)).abs()[both] / step).double().cpu().numpy()
    agree = int((mask_m & mask_s).sum()) / max(int(mask_m.sum()), 1)
    print(f"[raster] {type(model).__name__} depth, mesh against sphere tracing: {int(mask_m.sum())} pixels hit by the mesh, {int(mask_s.sum())} by sphere tracing, "
          f"{int((mask_m & mask_s).sum())} by both ({agree:.4f} of the mesh's), {int(both.sum())} compared; |difference| median {np.median(diff):.5f}, "
          f"p99 {np.quantile(diff, 0.99):.5f}, max {diff.max():.5f} grid steps (allowed {2 * np.sqrt(3):.3f})")
    assert both.sum() > 100
    assert diff.max() <= 2 * np.sqrt(3.0)
    assert agree >= 0.95
