"""The numpy marching cubes of tests/mc_ref.py against what is known about the surfaces it is given, so that the GPU test
(tests/test_gpu_marching_cubes.py) is not the kernels agreeing with a copy of themselves; and the PLY writer."""
import numpy as np

import mc_ref


def _grid(N):
    g = np.linspace(-1.0, 1.0, N)
    return np.meshgrid(g, g, g, indexing="ij")


def _closed_and_oriented(faces):
    _, n = mc_ref.undirected_edge_counts(faces)
    assert (n == 2).all(), np.bincount(n)
    assert mc_ref.is_consistently_oriented(faces)


def test_sphere_is_closed_oriented_and_as_accurate_as_linear_interpolation_allows():
    N, r = 33, 0.6
    h = 2.0 / (N - 1)
    X, Y, Z = _grid(N)
    vol = (np.sqrt(X * X + Y * Y + Z * Z) - r).astype(np.float32)
    verts, faces = mc_ref.marching_cubes(vol, 0.0, [h] * 3, [-1.0] * 3)
    _closed_and_oriented(faces)
    assert mc_ref.euler_characteristic(len(verts), faces) == 2
    # a vertex is the root of the linear interpolant of f = |x| - r along a grid edge of length h; |f - interpolant| <= h^2 / 8 max |f''|,
    # and the second derivative of |x| along a line is at most 1 / |x| <= 1 / (r - h) on an edge that crosses the sphere
    e_v = h * h / (8.0 * (r - h))
    assert np.abs(np.linalg.norm(verts, axis=1) - r).max() <= e_v
    # every triangle lies within one cell, so no point of it is farther than h from one of its vertices: the mesh lies between the spheres
    # of radius sqrt((r - e_v)^2 - h^2) and r + e_v
    vol_mesh = mc_ref.signed_volume(verts, faces)
    lo = 4.0 / 3.0 * np.pi * np.sqrt((r - e_v) ** 2 - h * h) ** 3
    hi = 4.0 / 3.0 * np.pi * (r + e_v) ** 3
    assert vol_mesh > 0 and lo <= vol_mesh <= hi, (lo, vol_mesh, hi)


def test_torus_has_euler_characteristic_zero():
    X, Y, Z = _grid(49)
    vol = (np.sqrt((np.sqrt(X * X + Y * Y) - 0.5) ** 2 + Z * Z) - 0.2).astype(np.float32)
    verts, faces = mc_ref.marching_cubes(vol, 0.0, [2.0 / 48] * 3, [-1.0] * 3)
    _closed_and_oriented(faces)
    assert mc_ref.euler_characteristic(len(verts), faces) == 0
    assert mc_ref.signed_volume(verts, faces) > 0


def test_two_disjoint_spheres_have_euler_characteristic_four():
    X, Y, Z = _grid(33)
    vol = np.minimum(np.sqrt((X - 0.45) ** 2 + Y * Y + Z * Z), np.sqrt((X + 0.45) ** 2 + Y * Y + Z * Z)).astype(np.float32) - np.float32(0.3)
    verts, faces = mc_ref.marching_cubes(vol, 0.0, [1.0 / 16] * 3, [-1.0] * 3)
    _closed_and_oriented(faces)
    assert mc_ref.euler_characteristic(len(verts), faces) == 4


def test_noise_volume_with_every_case_is_closed_and_oriented():
    """The test of the ambiguous faces: ~10^4 random cells hold all 256 cases (the chance of missing one is below 1e-13), and the surface still
    closes with every edge run through once in each direction."""
    vol = mc_ref.noise_volume((24, 24, 24), seed=0)
    assert len(np.unique(mc_ref.cell_cases(vol))) == 256
    verts, faces = mc_ref.marching_cubes(vol)
    assert len(faces) > 10000
    _closed_and_oriented(faces)
    assert faces.min() == 0 and faces.max() == len(verts) - 1


def test_vertex_and_face_order_are_the_documented_ones():
    """One cell, corner 0 inside: three vertices on the origin's x, y, z edges in that order, one triangle wound away from the corner."""
    vol = np.ones((2, 2, 2), dtype=np.float32)
    vol[0, 0, 0] = -1.0
    verts, faces = mc_ref.marching_cubes(vol, 0.0, [1.0, 2.0, 4.0], [10.0, 20.0, 30.0])
    assert np.array_equal(verts, [[10.5, 20.0, 30.0], [10.0, 21.0, 30.0], [10.0, 20.0, 32.0]])
    assert np.array_equal(faces, [[0, 1, 2]])
    n = np.cross(verts[1] - verts[0], verts[2] - verts[0])
    assert (n > 0).all()
    verts, faces = mc_ref.marching_cubes(vol, -2.0)              # nothing inside
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_write_ply_round_trips(tmp_path):
    from nerfart_amd import mesh_util
    vol = mc_ref.noise_volume((6, 7, 8), seed=3)
    verts, faces = mc_ref.marching_cubes(vol)
    verts = verts.astype(np.float32)
    path = str(tmp_path / "m.ply")
    assert mesh_util.write_ply(path, verts, faces) == path
    header, v, f, payload = mc_ref.read_ply(path)
    assert header == ("ply\nformat binary_little_endian 1.0\n"
                      f"element vertex {len(verts)}\nproperty float x\nproperty float y\nproperty float z\n"
                      f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
    assert payload == 12 * len(verts) + 13 * len(faces)
    assert np.array_equal(v, verts) and np.array_equal(f, faces)
    import torch
    mesh_util.write_ply(path, torch.from_numpy(verts), torch.from_numpy(faces))            # tensors are taken as well
    assert mc_ref.read_ply(path)[3] == payload
    mesh_util.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))    # an empty mesh is a valid file
    header, v, f, payload = mc_ref.read_ply(path)
    assert payload == 0 and len(v) == 0 and len(f) == 0
