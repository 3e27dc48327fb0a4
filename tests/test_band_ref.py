"""The numpy statement of the narrow-band sweep (tests/band_ref.py) held to the properties the method promises, on analytic distance functions and
with tests/mc_ref.py as the marching cubes; the argument refusals of the nerfart_band_* entry points (no launch); extract_mesh's two refusals.

What the bounds are: with lipschitz = 1 on 1-Lipschitz functions the band test cannot rule out a brick that touches a sign-changing edge, so no
repair round is needed and the mesh is the dense one EXACTLY.  The evaluated share at N = 96, B = 4 is capped at 0.25: the band is a shell of
thickness 2 * reach = 2 * sqrt(3) * 3 steps around a surface of area A, i.e. about A * 10.4 step bricks' worth of volume, which for the largest
surface used here (the two spheres, A = 4 pi (0.6^2 + 0.5^2) = 7.7 in a 3^3 cube, step = 3 / 95) is 0.09 of the cube before counting the bricks the
shell only clips - at most 0.25 with room.  Scaling f by 3 or 5 with lipschitz left at 1 violates the bound on purpose: the band is then too
thin by that factor, the check must find the edges it cut, and the repair must end - long before the cap of 4 - with the same mesh."""
import numpy as np
import pytest

import band_ref
import mc_ref

SIZES = {"96/4": (96, 4, 3.0), "50/8": (50, 8, 3.0), "33/4": (33, 4, 3.0)}          # N, B, volume_size; 50 = 6 * 8 + 2, 33 = 8 * 4 + 1: ragged


def coords(N, volume_size):
    a = np.arange(N, dtype=np.float64) * (volume_size / (N - 1)) + (-volume_size / 2.0)
    return np.meshgrid(a, a, a, indexing="ij")


def sphere(x, y, z):
    return np.sqrt(x * x + y * y + z * z) - 1.0


def torus(x, y, z):
    return np.sqrt((np.sqrt(x * x + y * y) - 0.9) ** 2 + z * z) - 0.35


def two_spheres(x, y, z):
    return np.minimum(np.sqrt((x + 0.55) ** 2 + y * y + z * z) - 0.6, np.sqrt((x - 0.7) ** 2 + (y - 0.2) ** 2 + (z + 0.1) ** 2) - 0.5)


SHAPES = {"sphere": sphere, "torus": torus, "two_spheres": two_spheres}
_DENSE = {}


def dense(shape, size, scale=1.0):
    """The dense float32 volume of scale * f, computed once and handed out read-only."""
    key = (shape, size, scale)
    if key not in _DENSE:
        N, _, vs = SIZES[size]
        v = (scale * SHAPES[shape](*coords(N, vs))).astype(np.float32)
        v.setflags(write=False)
        _DENSE[key] = v
    return _DENSE[key]


def same_mesh(a, b, level):
    va, fa = mc_ref.marching_cubes(a, level)
    vb, fb = mc_ref.marching_cubes(b, level)
    return len(va) > 0 and np.array_equal(va, vb) and np.array_equal(fa, fb)


def invariants(vol, masks, d, B, level):
    """What holds at every exit: true values in active bricks, probe values elsewhere, no sign-changing edge with a filled end."""
    bricks = band_ref.brick_of(d.shape[0], B)
    active = np.any(masks, axis=0)
    assert np.array_equal(vol[active[bricks]], d[active[bricks]])
    assert np.array_equal(vol[~active[bricks]], band_ref.probe_values(d, B)[bricks][~active[bricks]])
    assert not band_ref.wanted_bricks(vol, level, active, bricks).any()
    assert all(not (masks[i] & masks[j]).any() for i in range(len(masks)) for j in range(i))       # a brick is activated once


HOLDS = [(shape, size, 0.0) for shape in SHAPES for size in SIZES] + [("torus", "96/4", 0.125), ("sphere", "33/4", -0.0625)]


@pytest.mark.parametrize("shape,size,level", HOLDS)
def test_bound_that_holds_needs_no_repair_and_gives_the_dense_mesh(shape, size, level):
    N, B, vs = SIZES[size]
    d = dense(shape, size)
    vol, masks, info = band_ref.banded(d, B, level, band_ref.threshold(N, vs, B, 1.0))
    invariants(vol, masks, d, B, level)
    assert info["repair_rounds"] == 0 and not info["completed_dense"] and len(masks) == 1
    assert np.array_equal(vol < np.float32(level), d < np.float32(level))                            # every fill has the true sign
    assert same_mesh(vol, d, level)
    assert info["evaluated_points"] < N ** 3
    if size == "96/4":
        assert info["evaluated_points"] / N ** 3 <= 0.25, info


@pytest.mark.parametrize("scale", [3.0, 5.0])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_violated_bound_is_repaired_to_the_dense_mesh(shape, size, scale):
    N, B, vs = SIZES[size]
    d = dense(shape, size, scale)
    vol, masks, info = band_ref.banded(d, B, 0.0, band_ref.threshold(N, vs, B, 1.0), max_rounds=4)
    invariants(vol, masks, d, B, 0.0)
    assert info["repair_rounds"] >= 1 and not info["completed_dense"], info
    assert len(masks) == 1 + info["repair_rounds"] and info["active"] == [int(m.sum()) for m in masks]
    assert same_mesh(vol, d, 0.0)
    assert info["evaluated_points"] < N ** 3


def test_nan_probe_makes_its_brick_active():
    N, B, vs = SIZES["33/4"]
    d = dense("sphere", "33/4").copy()
    p = band_ref.probe_index(N, B)
    d[p[0], p[0], p[0]] = np.nan                                     # the corner brick's probe: far outside the sphere
    _, masks, _ = band_ref.banded(d, B, 0.0, band_ref.threshold(N, vs, B, 1.0))
    _, clean, _ = band_ref.banded(dense("sphere", "33/4"), B, 0.0, band_ref.threshold(N, vs, B, 1.0))
    assert masks[0][0] and not clean[0][0]
    assert np.array_equal(masks[0][1:], clean[0][1:])


def test_round_cap_zero_on_a_violated_bound_completes_densely():
    N, B, vs = SIZES["50/8"]
    d = dense("torus", "50/8", 5.0)
    vol, masks, info = band_ref.banded(d, B, 0.0, band_ref.threshold(N, vs, B, 1.0), max_rounds=0)
    assert info["completed_dense"] and info["repair_rounds"] == 0 and len(masks) == 2
    assert np.array_equal(vol, d) and info["evaluated_points"] == N ** 3 and sum(info["active"]) == info["bricks"]


def test_bricks_probes_and_threshold():
    assert band_ref.n_bricks_axis(50, 8) == 7 and band_ref.n_bricks_axis(33, 4) == 9 and band_ref.n_bricks_axis(96, 4) == 24
    assert list(band_ref.probe_index(50, 8)) == [4, 12, 20, 28, 36, 44, 49] and band_ref.probe_index(33, 4)[-1] == 32
    b = band_ref.brick_of(33, 4)
    assert b[0, 0, 0] == 0 and b[32, 32, 32] == 9 ** 3 - 1 and b[4, 0, 3] == 81 and np.bincount(b.reshape(-1))[-1] == 1
    assert band_ref.threshold(96, 3.0, 4, 1.0) == np.float32(np.sqrt(3.0) * 3 * 3.0 / 95)
    assert band_ref.threshold(50, 3.0, 8, 2.0) == np.float32(2.0 * np.sqrt(3.0) * 5 * 3.0 / 49)
    from nerfart_amd import mesh_util
    for N, B, vs in SIZES.values():
        assert mesh_util.band_threshold(N, vs, B, 1.5) == float(band_ref.threshold(N, vs, B, 1.5))


def test_band_entry_points_validate_their_arguments_without_a_gpu():
    """Null pointers, N < 2, B outside 2 .. 64 and N^3 >= 2^31 are refused with a message before any launch - here with pointers that are never
    dereferenced."""
    import ctypes as C
    from nerfart_amd import hip
    lib, null, one = hip.lib, C.c_void_p(0), C.c_void_p(16)

    def err():
        return lib.nerfart_last_error().decode()

    calls = {
        "band_probe_points": lambda N, B, p: lib.nerfart_band_probe_points(N, B, 0.1, -1.0, p, null),
        "band_select": lambda N, B, p: lib.nerfart_band_select(0, p, 0.0, 0.1, N, B, p, p, p, p, p, 1 << 40, p, null),
        "band_brick_points": lambda N, B, p: lib.nerfart_band_brick_points(p, p, 1, 8, 0, 8, N, B, 0.1, -1.0, p, p, null),
        "band_scatter": lambda N, B, p: lib.nerfart_band_scatter(p, p, 8, N, p, null),
        "band_fill": lambda N, B, p: lib.nerfart_band_fill(p, p, N, B, p, null),
        "band_check": lambda N, B, p: lib.nerfart_band_check(p, 0.0, p, N, B, p, p, null),
    }
    for name, call in calls.items():
        assert call(64, 8, null) == 2 and name in err() and "null" in err(), (name, err())
        for N in (1, 0, -5):
            assert call(N, 8, one) == 2 and name in err() and "N must be >= 2" in err(), (name, N, err())
        assert call(1291, 8, one) == 2 and name in err() and "2^31" in err(), (name, err())
        if name != "band_scatter":                                   # takes no brick edge
            for B in (1, 0, 65, -4):
                assert call(64, B, one) == 2 and name in err() and "2 .. 64" in err(), (name, B, err())
    assert lib.nerfart_band_workspace_bytes(1, 8) == 0 and "N must be >= 2" in err()
    assert lib.nerfart_band_workspace_bytes(64, 65) == 0 and "2 .. 64" in err()
    assert lib.nerfart_band_workspace_bytes(1291, 8) == 0 and "2^31" in err()
    n = lib.nerfart_band_workspace_bytes(1290, 2)                    # 645^3 bricks: off [n][2] + three block-sum levels, each rounded up to 256 bytes
    up = lambda b: (b + 255) // 256 * 256
    m0 = -(-645 ** 3 // 512); m1 = -(-m0 // 512); m2 = -(-m1 // 512)
    assert m2 > 1 and n == up(8 * 645 ** 3) + up(8 * m0) + up(8 * m1) + up(8 * m2)
    assert lib.nerfart_band_workspace_bytes(33, 4) == up(8 * 729) + up(8 * 2)
    ws = lib.nerfart_band_workspace_bytes(64, 8)
    assert lib.nerfart_band_select(3, one, 0.0, 0.1, 64, 8, one, one, one, one, one, ws, one, null) == 2 and "mode" in err()
    assert lib.nerfart_band_select(1, null, 0.0, 0.1, 64, 8, one, one, one, one, one, ws - 1, one, null) == 2 and "workspace" in err()
    assert lib.nerfart_band_select(1, null, 0.0, 0.1, 64, 8, one, one, one, one, C.c_void_p(8), ws, one, null) == 2 and "16-byte" in err()
    assert lib.nerfart_band_select(1, null, 0.0, 0.1, 64, 8, one, one, one, one, one, ws, C.c_void_p(12), null) == 2 and "8-byte" in err()
    for n_list, n_points, first, count in ((0, 8, 0, 8), (513, 8, 0, 8), (1, 64 ** 3 + 1, 0, 8), (1, 8, 4, 5), (1, 8, 9, 1)):
        assert lib.nerfart_band_brick_points(one, one, n_list, n_points, first, count, 64, 8, 0.1, -1.0, one, one, null) == 2, (n_list, n_points, first, count)
        assert "band_brick_points" in err() and "first + count" in err()
    assert lib.nerfart_band_brick_points(null, null, 0, 0, 0, 0, 64, 8, 0.1, -1.0, null, null, null) == 0      # an empty batch stays a no-op
    assert lib.nerfart_band_scatter(null, null, 0, 64, null, null) == 0


def test_extract_mesh_refuses_narrow_band_on_the_sheared_grid_and_with_skimage(tmp_path):
    """Both refusals come before anything touches the model or the GPU."""
    from nerfart_amd import mesh_util
    with pytest.raises(ValueError, match="regular grid"):
        mesh_util.extract_mesh(None, N=16, filepath=str(tmp_path / "a.ply"), narrow_band=True, reference_shear=True)
    with pytest.raises(ValueError, match="backend='native'"):
        mesh_util.extract_mesh(None, N=16, filepath=str(tmp_path / "b.ply"), narrow_band=True, backend="skimage")
    assert not list(tmp_path.iterdir())
