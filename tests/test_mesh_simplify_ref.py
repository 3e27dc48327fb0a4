"""tests/mesh_simplify_ref.py (the numpy statement of csrc/mesh_simplify.hip) held to a second, independent formulation - a plain Python dict
over faces, clusters keyed by their integer coordinates, the representative from a stacked least-squares problem - and its error bound shown
not to be vacuous: a float32 / fixed-point emulation of the kernels stays inside it, and each of seven injected bugs leaves it, or breaks an
integer equality, on at least one input.  Also what needs no GPU: the entry points' refusals, the Python front's, the tool's flags."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import yaml

import mc_ref
import mesh_simplify_ref as ref
from conftest import REPO

F32 = np.float32


def _mc(vol):
    verts, faces = mc_ref.marching_cubes(vol, 0.0)
    return verts.astype(np.float32), faces.astype(np.int32)


def _lattice_plane_one_ulp_below():
    """The slab 15 < x < 16.5 of a 20 x 10 x 10 grid with the sheet at x = 15 moved one ulp toward 0: floor gives 14, cluster 14 // 3 = 4, while
    the sheet at 16.5 is in cluster 5 - a rule that sends the first sheet to 5 as well welds the two."""
    verts, faces = _mc(ref.slab_volume((20, 10, 10), 15.0, 16.5))
    low = verts[:, 0] == 15
    assert low.sum() == 100 and (verts[~low, 0] == 16.5).all()
    verts[low, 0] = np.nextafter(F32(15), F32(0))
    return verts, faces


# name -> (mesh, grid shape, factor); a few hundred faces each
INPUTS = {
    "sphere_12_c2": (lambda: _mc(ref.sphere_volume((12, 12, 12), (5.3, 5.6, 5.1), 3.7)), (12, 12, 12), 2),
    "sphere_13_c3": (lambda: _mc(ref.sphere_volume((13, 13, 13), (6.2, 5.9, 6.4), 4.4)), (13, 13, 13), 3),
    "two_spheres_16_c4": (lambda: _mc(ref.two_spheres_volume((16, 12, 12), (4.6, 6.0, 6.0), (10.9, 6.0, 6.0), 2.6)), (16, 12, 12), 4),
    "nested_shells_14_c4": (lambda: _mc(ref.shells_volume((14, 14, 14), (6.4, 6.6, 6.3), 2.3, 3.4, 4.6)), (14, 14, 14), 4),
    "axis_plane_10_c2": (lambda: _mc(ref.plane_volume((10, 10, 10), (1.0, 0.0, 0.0), 4.0)), (10, 10, 10), 2),
    "tilted_plane_10_c3": (lambda: _mc(ref.plane_volume((10, 10, 10), (0.31, 0.52, 1.0), 7.83)), (10, 10, 10), 3),
    "lattice_plane_one_ulp_below_c3": (_lattice_plane_one_ulp_below, (20, 10, 10), 3),
}
_CACHE = {}


def case(name):
    """(verts float32, faces int32, shape, factor, ref.simplify(...)): computed once, shared, never modified."""
    if name not in _CACHE:
        make, shape, c = INPUTS[name]
        verts, faces = make()
        verts.setflags(write=False)
        faces.setflags(write=False)
        _CACHE[name] = (verts, faces, shape, c, ref.simplify(verts, faces, shape, c))
    return _CACHE[name]


# ---- the second formulation ----------------------------------------------------------------------------------------------------------------------

def dict_simplify(verts, faces, shape, c, reg=0.01):
    """Clusters are dicts keyed by (kx, ky, kz) - numbered by sorting the keys, which is the x-major order without the linear index -, faces are
    visited one by one, and the representative solves the stacked least-squares problem  n_f . x = n_f . a_f (one row per contribution),
    sqrt(lambda) x = sqrt(lambda) m  instead of the normal equations."""
    key_of = []
    for p in verts:
        key_of.append(tuple(min(int(np.floor(float(x))), n - 1) // c for x, n in zip(p, shape)))
    number = {k: i for i, k in enumerate(sorted(set(key_of)))}
    cluster = [number[k] for k in key_of]
    rows = {i: [] for i in number.values()}
    members = {i: [] for i in number.values()}
    centre = {i: np.array([c * (kk + 0.5) for kk in k]) for k, i in number.items()}
    for v, p in enumerate(verts):
        members[cluster[v]].append((p.astype(np.float64) - centre[cluster[v]]) / c)
    seen, out_faces = set(), []
    for f in faces:
        a, b, d = (verts[i].astype(np.float64) for i in f)
        n = np.cross((b - a) / c, (d - a) / c)
        ks = [cluster[i] for i in f]
        if n.any():
            for k in dict.fromkeys(ks):                                # each distinct cluster once
                rows[k].append((n, float(n @ ((a - centre[k]) / c))))
        if len(set(ks)) == 3:
            j = ks.index(min(ks))
            t = (ks[j], ks[(j + 1) % 3], ks[(j + 2) % 3])
            if t not in seen:
                seen.add(t)
                out_faces.append(t)
    out = np.zeros((len(number), 3))
    for k in range(len(number)):
        m = np.mean(members[k], axis=0)
        tr = sum(float(n @ n) for n, _ in rows[k])
        x = m
        if tr > 0:
            lam = reg * tr / 3.0
            lhs = np.vstack([n for n, _ in rows[k]] + [np.sqrt(lam) * np.eye(3)])
            rhs = np.concatenate([[t for _, t in rows[k]], np.sqrt(lam) * m])
            x = np.linalg.lstsq(lhs, rhs, rcond=None)[0]
        out[k] = centre[k] + c * np.clip(x, -0.5, 0.5)
    return np.array(cluster, np.int32), out, np.array(out_faces, np.int32).reshape(-1, 3)


@pytest.mark.parametrize("name", list(INPUTS))
def test_reference_is_the_dict_formulation(name):
    verts, faces, shape, c, r = case(name)
    cluster, out, out_faces = dict_simplify(verts, faces, shape, c)
    assert not r["bad"] and 100 <= len(faces) <= 1500
    assert np.array_equal(cluster, r["cluster"]) and np.array_equal(out_faces, r["faces"])
    assert out.shape == r["verts"].shape and np.abs(out - r["verts"]).max() < 1e-9          # two float64 routes, cond <= 301
    assert len(r["faces"]) < len(faces) and len(r["verts"]) < len(verts)


def test_small_cases_by_hand():
    # one triangle inside one cell of a 4^3 grid, factor 2: V' = 1, F' = 0, the representative on the triangle's plane z = 0.5 (and at the mean
    # in-plane: the regulariser's job)
    verts = np.array([[0.25, 0.25, 0.5], [1.5, 0.25, 0.5], [0.25, 1.5, 0.5]], np.float32)
    r = ref.simplify(verts, [[0, 1, 2]], (4, 4, 4), 2)
    assert r["cluster"].tolist() == [0, 0, 0] and r["faces"].shape == (0, 3) and r["verts"].shape == (1, 3)
    assert np.allclose(r["verts"][0], [2 / 3, 2 / 3, 0.5], atol=1e-12)
    # a vertex exactly on a lattice plane belongs to the upper cell; the last grid point of a ragged axis to the last cell
    cells = ref.vertex_cells(np.array([[2, 0, 0], [1.9999999, 0, 0], [4, 4, 4], [3.5, 4, 0]], np.float32), (5, 5, 5), 2)
    assert cells.tolist() == [9, 0, 26, 15]
    assert ref.vertex_cells(np.array([[np.nan, 0, 0], [0, -0.001, 0], [0, 0, 4.001], [np.inf, 1, 1]], np.float32), (5, 5, 5), 2).tolist() == [-1] * 4
    # rotation keeps the orientation; the first of two equal rotated triples survives, whatever rotation it came in; a reversed one is another face
    cl = np.arange(6)
    f, keep = ref.cluster_faces([[2, 1, 0], [3, 4, 5], [5, 3, 4], [1, 0, 2], [0, 1, 2], [4, 4, 5]], cl)
    assert f.tolist() == [[0, 2, 1], [3, 4, 5], [0, 1, 2]] and keep.tolist() == [0, 1, 4]
    assert ref.simplify(verts, [[0, 1, 3]], (4, 4, 4), 2)["bad"] and ref.simplify(verts, [[0, -1, 2]], (4, 4, 4), 2)["bad"]
    empty = ref.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), (4, 4, 4), 2)
    assert not empty["bad"] and empty["verts"].shape == (0, 3) and empty["faces"].shape == (0, 3)


# ---- the bound is not vacuous ------------------------------------------------------------------------------------------------------------------

BUGS = ("quadric_to_one_cluster_only", "b_in_the_wrong_clusters_frame", "missing_clamp", "lambda_dropped", "last_duplicate_kept",
        "orientation_lost_in_the_rotation", "cluster_from_a_float_division")


def emulate(verts, faces, shape, c, reg=0.01, bug=None):
    """csrc/mesh_simplify.hip in numpy: every term in float32, operation by operation as the kernels order them (no fma), summed as
    rint(term 2^40) in int64, the solve in float64, the output rounded to float32.  bug: one of BUGS, or None."""
    v = np.asarray(verts, F32)
    faces = np.asarray(faces, np.int64)
    cf = F32(c)
    if bug == "cluster_from_a_float_division":
        # floorf(x / c) as a compiler emits it once it may use the reciprocal: x * (1 / c).  (A correctly rounded fp32 division cannot fail for a
        # vertex one ulp below the plane x = c k: x / c = k - ulp(x) / c, and rounding that up to k would need 2 ulp(x) <= c ulp(k-), i.e.
        # 2^(E + 1) <= c 2^e with 2^E <= x < c k and 2^e < k - which puts c k above itself.  The integer rule needs no such argument.)
        n = np.array(shape, np.int64)
        k = np.minimum(np.floor(v * (F32(1) / cf)).astype(np.int64), (n - 1) // c)
        lx, ly, lz = ref.lattice(shape, c)
        cell = (k[:, 0] * ly + k[:, 1]) * lz + k[:, 2]
    else:
        cell = ref.vertex_cells(v, shape, c)
    cell_of, cluster = np.unique(cell, return_inverse=True)
    cluster = cluster.reshape(-1)
    K = len(cell_of)
    lx, ly, lz = ref.lattice(shape, c)
    kxyz = np.stack([cell_of // (ly * lz), (cell_of // lz) % ly, cell_of % lz], axis=1).astype(F32)
    centre = cf * (kxyz + F32(0.5))
    fix = lambda t: np.rint(t.astype(np.float64) * 2.0 ** 40).astype(np.int64)
    acc = np.zeros((K, 12), np.int64)
    nv = np.zeros(K, np.int64)
    np.add.at(acc[:, 9:], cluster, fix((v - centre[cluster]) / cf))
    np.add.at(nv, cluster, 1)
    va, vb, vc = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    u, w = (vb - va) / cf, (vc - va) / cf
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    ks = cluster[faces]
    for j in range(1 if bug == "quadric_to_one_cluster_only" else 3):
        on = n.any(axis=1)
        for i in range(j):
            on &= ks[:, j] != ks[:, i]
        k = ks[on, j]
        frame = ks[on, 0] if bug == "b_in_the_wrong_clusters_frame" else k
        l = (va[on] - centre[frame]) / cf
        nn = n[on]
        d = (nn[:, 0] * l[:, 0] + nn[:, 1] * l[:, 1]) + nn[:, 2] * l[:, 2]
        terms = np.stack([nn[:, 0] * nn[:, 0], nn[:, 0] * nn[:, 1], nn[:, 0] * nn[:, 2], nn[:, 1] * nn[:, 1], nn[:, 1] * nn[:, 2], nn[:, 2] * nn[:, 2],
                          nn[:, 0] * d, nn[:, 1] * d, nn[:, 2] * d], axis=1)
        assert terms.dtype == F32
        np.add.at(acc[:, :9], k, fix(terms))
    s = acc.astype(np.float64) * 2.0 ** -40
    out = np.zeros((K, 3), F32)
    for k in range(K):
        A = np.array([[s[k, 0], s[k, 1], s[k, 2]], [s[k, 1], s[k, 3], s[k, 4]], [s[k, 2], s[k, 4], s[k, 5]]])
        m = s[k, 9:] / nv[k]
        x = m
        if np.trace(A) > 0:
            lam = 0.0 if bug == "lambda_dropped" else reg * np.trace(A) / 3.0
            x = np.linalg.lstsq(A + lam * np.eye(3), s[k, 6:9] + lam * m, rcond=None)[0] if lam == 0 else np.linalg.solve(A + lam * np.eye(3), s[k, 6:9] + lam * m)
        if bug != "missing_clamp":
            x = np.clip(x, -0.5, 0.5)
        out[k] = (float(c) * (kxyz[k].astype(np.float64) + 0.5) + float(c) * x).astype(F32)
    t = cluster[faces]
    r = np.sort(t, axis=1) if bug == "orientation_lost_in_the_rotation" else ref.rotate(t)
    proper = (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2])
    seen, keep = {}, []
    for f in np.nonzero(proper)[0]:
        key = tuple(r[f])
        if bug == "last_duplicate_kept":
            seen[key] = f
        elif key not in seen:
            seen[key] = f
    keep = sorted(seen.values())
    return cluster.astype(np.int32), out, r[keep].astype(np.int32)


def judge(name, bug=None):
    """(integers equal, worst distance / bound) of the emulation against the reference on one input."""
    verts, faces, shape, c, r = case(name)
    cluster, out, out_faces = emulate(verts, faces, shape, c, bug=bug)
    same = np.array_equal(cluster, r["cluster"]) and out_faces.shape == r["faces"].shape and np.array_equal(out_faces, r["faces"])
    if out.shape != r["verts"].shape:
        return False, np.inf
    return same, float(np.max(np.linalg.norm(out.astype(np.float64) - r["verts"], axis=1) / r["bound"]))


@pytest.mark.parametrize("name", list(INPUTS))
def test_a_float32_fixed_point_emulation_stays_inside_the_bound(name):
    same, ratio = judge(name)
    print(f"{name}: worst distance / bound {ratio:.3f}")
    assert same and ratio <= 1.0


@pytest.mark.parametrize("bug", BUGS)
def test_every_injected_bug_is_caught_on_some_input(bug):
    caught = []
    for name in INPUTS:
        same, ratio = judge(name, bug)
        if not same or ratio > 1.0:
            caught.append(name)
    print(f"{bug}: caught on {caught}")
    assert caught


# ---- without a GPU: refusals, argument errors, the tool's flags ---------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_before_any_launch():
    from nerfart_amd import hip
    lib, null, one = hip.lib, C.c_void_p(0), C.c_void_p(256)       # `one`: non-null, aligned, never dereferenced - the checks come first

    def err():
        return lib.nerfart_last_error().decode()

    assert lib.nerfart_mesh_simplify_workspace_bytes(10, 10, 1, 8, 8, 8) == 0 and "factor" in err()
    assert lib.nerfart_mesh_simplify_workspace_bytes(10, 10, 2, 0, 8, 8) == 0 and "dimension" in err()
    assert lib.nerfart_mesh_simplify_workspace_bytes(10, 10, 2, 8192, 4096, 512) == 0 and "2^31" in err()          # 4096 * 2048 * 256 = 2^31 cells
    assert lib.nerfart_mesh_simplify_workspace_bytes(10, 10, 2, 8192, 4096, 510) > 0                               # 255 * 2^23 cells
    assert lib.nerfart_mesh_simplify_workspace_bytes(1 << 31, 10, 2, 8, 8, 8) == 0 and "2^31" in err()
    assert lib.nerfart_mesh_simplify_workspace_bytes(10, 1 << 30, 2, 8, 8, 8) == 0 and "2^30" in err()
    need = lib.nerfart_mesh_simplify_workspace_bytes(100, 200, 2, 8, 8, 8)
    # off [200][2], cell [100], occ [64], tab [512], slot [200], acc [64][12] int64, cnt [64][2], cell_of [64]: each rounded up to 256 bytes
    assert need == sum((b + 255) // 256 * 256 for b in (8 * 200, 4 * 100, 64, 4 * 512, 4 * 200, 8 * 12 * 64, 8 * 64, 4 * 64))
    count = lambda **kw: lib.nerfart_mesh_simplify_count(*[kw.get(k, d) for k, d in (("verts", one), ("faces", one), ("V", 100), ("F", 200), ("c", 2),
                                                                                     ("nx", 8), ("ny", 8), ("nz", 8), ("ws", one), ("ws_bytes", need),
                                                                                     ("cluster", one), ("counts", one), ("stream", null))])
    emit = lambda **kw: lib.nerfart_mesh_simplify_emit(*[kw.get(k, d) for k, d in (("faces", one), ("V", 100), ("F", 200), ("c", 2), ("nx", 8), ("ny", 8),
                                                                                   ("nz", 8), ("reg", 0.01), ("ws", one), ("ws_bytes", need),
                                                                                   ("cluster", one), ("verts_out", one), ("faces_out", one),
                                                                                   ("V_out", 10), ("F_out", 20), ("stream", null))])
    for k in ("verts", "faces", "ws", "cluster", "counts"):
        assert count(**{k: null}) == 2 and "null" in err(), k
    for k in ("faces", "ws", "cluster", "verts_out", "faces_out"):
        assert emit(**{k: null}) == 2 and "null" in err(), k
    for fn in (count, emit):
        assert fn(c=1) == 2 and "factor" in err()
        assert fn(nx=1 << 25) == 2 and "dimension" in err()
        assert fn(ws_bytes=need - 1) == 2 and "workspace" in err()
        assert fn(ws=C.c_void_p(260)) == 2 and "aligned" in err()
    assert count(counts=C.c_void_p(260)) == 2 and "aligned" in err()
    for reg in (0.0, -1.0, float("nan"), 1e7):
        assert emit(reg=reg) == 2 and "reg" in err()
    assert emit(V_out=65) == 2 and "V_out" in err()                # more than min(V, cells) = 64
    assert emit(F_out=201) == 2 and "F_out" in err()
    assert emit(V_out=0, F_out=0, verts_out=null, faces_out=null) == 0          # an empty result launches nothing and succeeds


def test_python_front_refuses_cpu_tensors_and_bad_options():
    import torch
    from nerfart_amd import mesh_util
    faces, verts = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.simplify_clusters(verts, faces, (4, 4, 4), 2)
    for factor in (1, 0, -2, 2.5):
        with pytest.raises(ValueError, match="factor"):
            mesh_util.simplify_clusters(verts, faces, (4, 4, 4), factor)
    for reg in (0.0, -0.01, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="reg"):
            mesh_util.simplify_clusters(verts, faces, (4, 4, 4), 2, reg=reg)
    with pytest.raises(ValueError, match="simplify_factor needs the regular grid"):
        mesh_util.extract_mesh(None, simplify_factor=2, reference_shear=True)
    with pytest.raises(ValueError, match="simplify_factor needs backend='native'"):
        mesh_util.extract_mesh(None, simplify_factor=2, backend="skimage")


def test_the_tool_takes_the_two_flags(tmp_path):
    from nerfart_amd import scene
    spec = importlib.util.spec_from_file_location("extract_surface", os.path.join(REPO, "tools", "extract_surface.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    d = scene.synthetic_config("NeuS").to_dict()
    d["expname"] = "mesh"
    d.setdefault("training", {})["log_root_dir"] = str(tmp_path)
    path = tmp_path / "neus.yaml"
    path.write_text(yaml.dump(d))
    args, _ = tool.parse(["--config", str(path), "--simplify", "4", "--simplify_reg", "0.05"])
    assert (args.simplify, args.simplify_reg) == (4, 0.05)
    args, _ = tool.parse(["--config", str(path)])
    assert (args.simplify, args.simplify_reg) == (None, 0.01)
