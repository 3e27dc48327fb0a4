"""csrc/marching_cubes.hip (mesh_util.marching_cubes / extract_mesh) against the numpy marching cubes of tests/mc_ref.py, which
tests/test_mc_ref.py holds to what is known about its surfaces: faces identical, vertices to fp32 rounding, on volumes that take every path -
non-cubic, one cell, every level of the scan, values equal to the level, no surface at all - plus determinism, the refusals, and extract_mesh
end to end on the two sphere-initialised models."""
import sys

import numpy as np
import pytest
import torch

import mc_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCAN_BLOCK = 512          # csrc/marching_cubes.hip MC_SCAN_BLOCK: items per block at every level of the scan (256 threads x 2)


def _grid(N):
    g = torch.linspace(-1.0, 1.0, N, device=DEV, dtype=torch.float64)
    return torch.meshgrid(g, g, g, indexing="ij")


def _sphere():
    X, Y, Z = _grid(33)
    return ((X * X + Y * Y + Z * Z).sqrt() - 0.6).float()


def _torus():
    X, Y, Z = _grid(49)
    return ((((X * X + Y * Y).sqrt() - 0.5) ** 2 + Z * Z).sqrt() - 0.2).float()


def _noise(shape, seed, pad=True):
    return torch.from_numpy(mc_ref.noise_volume(shape, seed=seed, pad=pad)).to(DEV)


def _with_level_entries():
    """Integers -2..2: a fifth of the entries EQUAL the level 0 (outside by the strict rule: t = 0 or 1, degenerate triangles are kept)."""
    v = torch.from_numpy(np.random.default_rng(5).integers(-2, 3, size=(9, 10, 11)).astype(np.float32))
    assert int((v == 0).sum()) > 100
    return v.to(DEV)


# name -> (volume builder, level, spacing, origin)
CASES = {
    "sphere": (_sphere, 0.0, [1.0 / 16] * 3, [-1.0] * 3),
    "torus": (_torus, 0.0, [2.0 / 48] * 3, [-1.0] * 3),
    "noise_24": (lambda: _noise((24, 24, 24), 0), 0.0, [1.0] * 3, [0.0] * 3),
    "noncubic_5x7x70": (lambda: _noise((5, 7, 70), 1, pad=False), 0.0, [0.5, 0.25, 0.1], [3.0, -2.0, 0.7]),
    "one_cell": (lambda: torch.tensor([[[-1.0, 1.0], [1.0, 1.0]], [[1.0, 1.0], [1.0, -0.5]]], device=DEV), 0.0, [1.0, 2.0, 4.0], [10.0, 20.0, 30.0]),
    "noise_70": (lambda: _noise((70, 70, 70), 2), 0.0, [1.0 / 70] * 3, [-0.5] * 3),
    "sphere_level_0.25": (_sphere, 0.25, [1.0 / 16] * 3, [-1.0] * 3),
    "entries_equal_level": (_with_level_entries, 0.0, [1.0] * 3, [0.0] * 3),
    "all_positive": (lambda: torch.full((6, 5, 4), 0.5, device=DEV), 0.0, [1.0] * 3, [0.0] * 3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_mesh_is_the_reference_mesh(name):
    from nerfart_amd import mesh_util
    build, level, spacing, origin = CASES[name]
    vol = build()
    if name == "noise_70":
        # 343,000 points are more than one block of the block-sum level (512 sums of 512 points each), so every level of the scan runs: the
        # per-point level, two blocks of block sums, and a third level over those two
        assert vol.numel() > SCAN_BLOCK * SCAN_BLOCK
    if name == "noise_24":
        assert len(np.unique(mc_ref.cell_cases(vol.cpu().numpy()))) == 256
    verts, faces = mesh_util.marching_cubes(vol, level=level, spacing=spacing, origin=origin)
    assert verts.device == vol.device and faces.device == vol.device
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32
    rv, rf = mc_ref.marching_cubes(vol.cpu().numpy(), level, spacing, origin)
    assert tuple(verts.shape) == rv.shape and tuple(faces.shape) == rf.shape
    if name == "all_positive":
        assert tuple(verts.shape) == (0, 3) and tuple(faces.shape) == (0, 3)
        return
    assert len(rf) > 0
    assert np.array_equal(faces.cpu().numpy(), rf)
    # three fp32 roundings in t (t in [0, 1]), the rounding of pa and of the product: 2^-22 (|coordinate| + spacing) per component
    sp = np.asarray(spacing, dtype=np.float32).astype(np.float64)
    delta = np.abs(verts.cpu().numpy().astype(np.float64) - rv)
    bound = 2.0 ** -22 * (np.abs(rv) + sp)
    worst = float((delta / bound).max())
    print(f"[mc] {name}: V = {len(rv)}, F = {len(rf)}, max |delta| / bound = {worst:.3f}")
    assert (delta <= bound).all(), worst
    # and a second call gives the same bits
    verts2, faces2 = mesh_util.marching_cubes(vol, level=level, spacing=spacing, origin=origin)
    assert torch.equal(verts, verts2) and torch.equal(faces, faces2)


def test_refusals():
    from nerfart_amd import mesh_util, hip
    vol = _noise((8, 8, 8), 7)
    bad = vol.clone()
    bad[3, 4, 5] = float("nan")
    with pytest.raises(ValueError):
        mesh_util.marching_cubes(bad)
    bad[3, 4, 5] = float("inf")
    with pytest.raises(ValueError):
        mesh_util.marching_cubes(bad)
    with pytest.raises(hip.NerfartHipError, match="GPU"):
        mesh_util.marching_cubes(vol.cpu())
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1)):
        with pytest.raises(hip.NerfartHipError, match=">= 2"):
            mesh_util.marching_cubes(torch.ones(shape, device=DEV))
    need = hip.mc_workspace_bytes(8, 8, 8)
    with pytest.raises(hip.NerfartHipError, match="workspace"):
        hip.mc_count(vol, 0.0, ws=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
    ws, counts = hip.mc_count(vol, 0.0, ws=torch.empty(need, dtype=torch.uint8, device=DEV))      # the exact size is accepted
    V, F, flag = (int(c) for c in counts.cpu())
    rv, rf = mc_ref.marching_cubes(vol.cpu().numpy())
    assert (V, F, flag) == (len(rv), len(rf), 0)
    with pytest.raises(hip.NerfartHipError, match="workspace"):
        hip.mc_emit(vol, 0.0, [0.0] * 3, [1.0] * 3, ws[:need - 1], V, F)
    with pytest.raises(hip.NerfartHipError, match="2\\^31"):
        hip.mc_workspace_bytes(1024, 1024, 1024)


@pytest.mark.parametrize("framework,volume_size", [("NeuS", 2.0), ("VolSDF", 3.0)])
def test_extract_mesh_end_to_end(framework, volume_size, tmp_path):
    from nerfart_amd import scene, mesh_util
    N = 48
    model, _, _ = scene.build_model(framework, seed=0, beta=None if framework == "NeuS" else 0.01, device=DEV)
    vol = mesh_util.sdf_volume(model.implicit_surface, volume_size=volume_size, N=N)
    border = torch.ones_like(vol, dtype=torch.bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert float(vol[border].min()) > 0.0, "the sphere initialisation must lie inside the volume for `closed` to be a fair demand"
    path = str(tmp_path / "surface.ply")
    assert mesh_util.extract_mesh(model.implicit_surface, volume_size=volume_size, N=N, filepath=path) == path
    assert "skimage" not in sys.modules and "plyfile" not in sys.modules
    _, verts, faces, _ = mc_ref.read_ply(path)
    v2, f2 = mesh_util.marching_cubes(vol, spacing=[volume_size / N] * 3, origin=[-volume_size / 2.0] * 3)
    assert np.array_equal(verts, v2.cpu().numpy()) and np.array_equal(faces, f2.cpu().numpy())
    assert len(faces) > 1000
    assert mc_ref.is_closed(faces) and mc_ref.is_consistently_oriented(faces)
    assert mc_ref.euler_characteristic(len(verts), faces) == 2
    assert mc_ref.signed_volume(verts, faces) > 0
