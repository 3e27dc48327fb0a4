"""csrc/mesh_band.hip and mesh_util.banded_volume on the GPU, held to tests/band_ref.py: everything is compared for EQUALITY (float32 volumes as int32
views, points by torch.equal, brick masks and counts as integers).  The premise - the SDF kernel gives a point the same bits whatever batch it is
in - is tested first; then the points against mesh_util.grid_points, the sweep against the numpy reference with analytic functions as the field, and
the two scene models end to end down to the bytes of the PLY file."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import band_ref
from conftest import REPO
from test_band_ref import SIZES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the premise --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16x3", "mixed"])
def test_sdf_kernel_gives_a_point_the_same_bits_in_any_batch(precision):
    from nerfart_amd import scene
    model, _, _ = scene.build_model("VolSDF", seed=0, beta=0.01, device=DEV, precision=precision)
    f = model.implicit_surface.forward
    g = torch.Generator().manual_seed(5)
    pts = ((torch.rand(4099, 3, generator=g) - 0.5) * 3.0).to(DEV)
    perm = torch.randperm(4099, generator=g).to(DEV)
    with torch.no_grad():
        whole = f(pts).reshape(-1)
        permuted = f(pts[perm].contiguous()).reshape(-1)
        halves = torch.cat([f(pts[:1500].contiguous()).reshape(-1), f(pts[1500:].contiguous()).reshape(-1)])
    assert whole.shape == (4099,) and torch.isfinite(whole).all()
    assert torch.equal(bits(whole[perm]), bits(permuted))
    assert torch.equal(bits(whole), bits(halves))


# ---- 2. the points ---------------------------------------------------------------------------------------------------------------------------

def evaluation_order(N, B, mask):
    """Linear grid indices of the owned points of the bricks in mask, bricks ascending, inside a brick z fastest (= ascending linear index)."""
    brick = band_ref.brick_of(N, B).reshape(-1)
    lin = np.nonzero(mask[brick])[0]
    return lin[np.lexsort((lin, brick[lin]))]


@pytest.mark.parametrize("volume_size", [2.0, 3.0])
@pytest.mark.parametrize("size", list(SIZES))
def test_probe_and_brick_points_are_grid_points_rows(size, volume_size):
    from nerfart_amd import hip, mesh_util
    N, B, _ = SIZES[size]
    step, org = volume_size / (N - 1), -volume_size / 2.0
    grid = mesh_util.grid_points(N, volume_size, DEV)
    p = band_ref.probe_index(N, B)
    lin = ((p[:, None, None] * N + p[None, :, None]) * N + p[None, None, :]).reshape(-1)
    probe = hip.band_probe_points(N, B, step, org, DEV)
    assert torch.equal(probe, grid[torch.from_numpy(lin).to(DEV)])
    # every brick (mode 2 on a fresh state): all N^3 points, in the evaluation order
    state = hip.BandState(N, B, DEV)
    assert [int(c) for c in hip.band_select(state, 2).cpu()] == [state.bricks, N ** 3]
    assert torch.equal(state.list.cpu(), torch.arange(state.bricks, dtype=torch.int32)) and bool(state.flag.all())
    pts, idx = hip.band_brick_points(state, state.bricks, N ** 3, 0, N ** 3, step, org)
    order = evaluation_order(N, B, np.ones(state.bricks, dtype=bool))
    assert np.array_equal(idx.cpu().numpy(), order)
    assert torch.equal(pts, grid[idx.long()])
    part, pidx = hip.band_brick_points(state, state.bricks, N ** 3, 1234, 777, step, org)       # a batch that starts and ends inside bricks
    assert torch.equal(part, pts[1234:2011]) and torch.equal(pidx, idx[1234:2011])
    # a sparse list (mode 0 on a hand-made probe array: every third brick and the last, ragged one)
    mask = np.zeros(state.bricks, dtype=bool)
    mask[::3] = True
    mask[-1] = True
    probe_values = torch.from_numpy(np.where(mask, 0.0, 1.0).astype(np.float32)).to(DEV)
    n_list, n_points = (int(c) for c in hip.band_select(state, 0, probe_values, 0.0, 0.5).cpu())
    order = evaluation_order(N, B, mask)
    assert (n_list, n_points) == (int(mask.sum()), len(order))
    assert np.array_equal(state.list[:n_list].cpu().numpy(), np.nonzero(mask)[0]) and np.array_equal(state.flag.cpu().numpy(), mask.astype(np.uint8))
    pts, idx = hip.band_brick_points(state, n_list, n_points, 0, n_points, step, org)
    assert np.array_equal(idx.cpu().numpy(), order) and torch.equal(pts, grid[idx.long()])


# ---- 3. the sweep against the numpy reference --------------------------------------------------------------------------------------------------

def sphere(x, y, z):
    return torch.sqrt(x * x + y * y + z * z) - 1.0


def torus(x, y, z):
    return torch.sqrt((torch.sqrt(x * x + y * y) - 0.9) ** 2 + z * z) - 0.35


def two_spheres(x, y, z):
    return torch.minimum(torch.sqrt((x + 0.55) ** 2 + y * y + z * z) - 0.6, torch.sqrt((x - 0.7) ** 2 + (y - 0.2) ** 2 + (z + 0.1) ** 2) - 0.5)


SHAPES = {"sphere": sphere, "torus": torus, "two_spheres": two_spheres}


def field(shape, scale=1.0, nan_at=None):
    """An elementwise (so batch-independent) float32 field on the GPU; nan_at: one point [3] whose value is NaN."""
    def f(pts):
        v = scale * SHAPES[shape](pts[:, 0], pts[:, 1], pts[:, 2])
        if nan_at is not None:
            v = torch.where((pts == nan_at).all(-1), torch.full_like(v, float("nan")), v)
        return v
    return f


def sweep(f, N, B, volume_size, level=0.0, lipschitz=1.0, cap=4, chunk=1 << 24):
    """mesh_util.banded_volume with every query recorded: (vol, info, masks) - masks rebuilt from the points that were asked for, after checking that
    each round asked for exactly the owned points of its bricks in the evaluation order, in batches of at most chunk."""
    from nerfart_amd import mesh_util
    step, org = volume_size / (N - 1), -volume_size / 2.0
    calls = []

    def recorded(pts):
        assert pts.dtype == torch.float32 and pts.is_cuda and pts.dim() == 2 and pts.shape[1] == 3 and 1 <= pts.shape[0] <= chunk
        calls.append(pts.clone())
        return f(pts)
    vol, info = mesh_util.banded_volume(recorded, N, volume_size, level=level, brick=B, lipschitz=lipschitz, max_repair_rounds=cap, chunk=chunk,
                                        device=DEV)
    nb3 = band_ref.n_bricks_axis(N, B) ** 3
    asked = torch.cat(calls)
    ijk = torch.round((asked.double() - org) / step).long()
    lin = ((ijk[:, 0] * N + ijk[:, 1]) * N + ijk[:, 2]).cpu().numpy()
    assert info["bricks"] == nb3 and len(lin) == nb3 + info["evaluated_points"]
    lin = lin[nb3:]                                                  # after the probe queries
    brick = band_ref.brick_of(N, B).reshape(-1)
    points_of = np.bincount(brick)
    masks, at = [], 0
    for n_active in info["active"]:
        mask = np.zeros(nb3, dtype=bool)
        seen = 0
        while seen < n_active:                                       # the round's bricks, one after the other
            b = brick[lin[at]]
            assert not mask[b]
            mask[b] = True
            seen += 1
            at += points_of[b]
        masks.append(mask)
    assert at == len(lin)
    assert np.array_equal(lin, np.concatenate([evaluation_order(N, B, m) for m in masks] + [np.zeros(0, dtype=np.int64)]))
    return vol, info, masks


def against_reference(shape, size, level=0.0, scale=1.0, cap=4, chunk=1 << 24, nan_probe=False):
    from nerfart_amd import mesh_util
    N, B, vs = SIZES[size]
    nan_at = None
    if nan_probe:
        p = int(band_ref.probe_index(N, B)[0])
        nan_at = mesh_util.grid_points(N, vs, DEV, (p * N + p) * N + p, (p * N + p) * N + p + 1)[0]
    f = field(shape, scale, nan_at)
    dense = f(mesh_util.grid_points(N, vs, DEV)).reshape(N, N, N)
    ref_vol, ref_masks, ref_info = band_ref.banded(dense.cpu().numpy(), B, level, band_ref.threshold(N, vs, B, 1.0), cap)
    vol, info, masks = sweep(f, N, B, vs, level=level, lipschitz=1.0, cap=cap, chunk=chunk)
    assert info == ref_info
    assert len(masks) == len(ref_masks) and all(np.array_equal(a, b) for a, b in zip(masks, ref_masks))
    assert np.array_equal(bits(vol).cpu().numpy(), ref_vol.view(np.int32))
    return vol, info, masks, dense


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sweep_equals_the_reference_when_the_bound_holds(shape, size):
    from nerfart_amd import mesh_util
    vol, info, _, dense = against_reference(shape, size)
    assert info["repair_rounds"] == 0 and not info["completed_dense"] and info["evaluated_points"] < SIZES[size][0] ** 3
    va, fa = mesh_util.marching_cubes(vol)
    vb, fb = mesh_util.marching_cubes(dense)
    assert va.shape[0] > 0 and torch.equal(bits(va), bits(vb)) and torch.equal(fa, fb)


@pytest.mark.parametrize("shape,size,level", [("torus", "96/4", 0.125), ("sphere", "33/4", -0.0625)])
def test_sweep_equals_the_reference_at_a_level_other_than_zero(shape, size, level):
    from nerfart_amd import mesh_util
    vol, info, _, dense = against_reference(shape, size, level=level)
    assert info["repair_rounds"] == 0 and not info["completed_dense"]
    va, fa = mesh_util.marching_cubes(vol, level)
    vb, fb = mesh_util.marching_cubes(dense, level)
    assert va.shape[0] > 0 and torch.equal(bits(va), bits(vb)) and torch.equal(fa, fb)


@pytest.mark.parametrize("scale", [3.0, 5.0])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_violated_bound_is_repaired_as_the_reference_repairs_it(shape, size, scale):
    from nerfart_amd import mesh_util
    vol, info, _, dense = against_reference(shape, size, scale=scale)
    assert info["repair_rounds"] >= 1 and not info["completed_dense"]
    va, fa = mesh_util.marching_cubes(vol)
    vb, fb = mesh_util.marching_cubes(dense)
    assert va.shape[0] > 0 and torch.equal(bits(va), bits(vb)) and torch.equal(fa, fb)


def test_round_cap_zero_completes_densely():
    vol, info, masks, dense = against_reference("torus", "50/8", scale=5.0, cap=0)
    assert info["completed_dense"] and info["repair_rounds"] == 0 and len(masks) == 2 and info["evaluated_points"] == 50 ** 3
    assert torch.equal(bits(vol), bits(dense))


def test_nan_probe_makes_its_brick_active():
    from nerfart_amd import mesh_util
    vol, info, masks, _ = against_reference("sphere", "33/4", nan_probe=True)
    assert masks[0][0] and bool(torch.isnan(vol[2, 2, 2]))
    with pytest.raises(ValueError, match="non-finite"):
        mesh_util.marching_cubes(vol)


@pytest.mark.parametrize("shape,size,scale", [("two_spheres", "50/8", 1.0), ("torus", "33/4", 3.0)])
def test_small_chunks_change_nothing(shape, size, scale):
    a, info_a, masks_a, _ = against_reference(shape, size, scale=scale)
    b, info_b, masks_b, _ = against_reference(shape, size, scale=scale, chunk=1000)
    assert info_a == info_b and all(np.array_equal(x, y) for x, y in zip(masks_a, masks_b)) and torch.equal(bits(a), bits(b))


def test_two_runs_give_the_same_bits():
    N, B, vs = SIZES["96/4"]
    from nerfart_amd import mesh_util
    f = field("two_spheres", 3.0)
    a, ia = mesh_util.banded_volume(f, N, vs, brick=B, lipschitz=1.0, device=DEV)
    b, ib = mesh_util.banded_volume(f, N, vs, brick=B, lipschitz=1.0, device=DEV)
    assert ia == ib and ia["repair_rounds"] >= 1 and torch.equal(bits(a), bits(b))


# ---- 4. the models -----------------------------------------------------------------------------------------------------------------------------

MODELS = {"VolSDF": dict(build=dict(framework="VolSDF", seed=0, beta=0.01, precision="bf16x3"), N=96, volume_size=3.0, B=4),
          "NeuS": dict(build=dict(framework="NeuS", seed=0, beta=None), N=64, volume_size=2.0, B=4)}


@pytest.fixture(scope="module", params=list(MODELS))
def swept(request):
    """(model, case, dense volume, banded volume, info, path of the default call's PLY) - the model is swept densely ONCE."""
    from nerfart_amd import scene, mesh_util
    case = MODELS[request.param]
    model, _, _ = scene.build_model(device=DEV, **case["build"])
    dense = mesh_util.sdf_volume(model.implicit_surface, case["volume_size"], case["N"])
    info = {}
    vol = mesh_util.sdf_volume(model.implicit_surface, case["volume_size"], case["N"], narrow_band=True, band_brick=case["B"], band_info=info)
    return model, case, dense, vol, info


def test_model_volume_is_the_dense_one_in_active_bricks_and_gives_its_mesh(swept):
    from nerfart_amd import mesh_util
    model, case, dense, vol, info = swept
    N, B = case["N"], case["B"]
    assert info["bricks"] == band_ref.n_bricks_axis(N, B) ** 3 and 0 < info["evaluated_points"] < N ** 3 and not info["completed_dense"]
    assert info["threshold"] == mesh_util.band_threshold(N, case["volume_size"], B, mesh_util.BAND_LIPSCHITZ)
    d = dense.cpu().numpy()
    ref_vol, ref_masks, ref_info = band_ref.banded(d, B, 0.0, info["threshold"])
    assert info == ref_info
    assert np.array_equal(bits(vol).cpu().numpy(), ref_vol.view(np.int32))           # true values in active bricks, probe values elsewhere
    active = np.any(ref_masks, axis=0)[band_ref.brick_of(N, B)]
    assert np.array_equal(bits(vol).cpu().numpy()[active], d.view(np.int32)[active])
    va, fa = mesh_util.marching_cubes(vol)
    vb, fb = mesh_util.marching_cubes(dense)
    assert va.shape[0] > 0 and torch.equal(bits(va), bits(vb)) and torch.equal(fa, fb)


@pytest.mark.parametrize("options", ["plain", "vertex_data"])
def test_extract_mesh_writes_the_same_file_with_the_narrow_band(swept, options, tmp_path):
    from nerfart_amd import mesh_util
    model, case, _, _, _ = swept
    kw = dict(volume_size=case["volume_size"], N=case["N"])
    if options == "vertex_data":
        kw.update(refine_evals=2, vertex_normals=True, color_model=model, keep_largest=1)
    info = {}
    a = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "dense.ply"), **kw)
    b = mesh_util.extract_mesh(model.implicit_surface, filepath=str(tmp_path / "band.ply"), narrow_band=True, band_brick=case["B"], band_info=info, **kw)
    data = open(a, "rb").read()
    assert len(data) > 10000 and data == open(b, "rb").read()
    assert 0 < info["evaluated_points"] < case["N"] ** 3


# ---- 5. the tool -------------------------------------------------------------------------------------------------------------------------------

def _tool():
    spec = importlib.util.spec_from_file_location("extract_surface", os.path.join(REPO, "tools", "extract_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_flags_parse_and_reach_extract_mesh(tmp_path, monkeypatch, capsys):
    from nerfart_amd import scene, mesh_util
    d = scene.synthetic_config("NeuS").to_dict()
    d["expname"] = "mesh"
    d.setdefault("training", {})["log_root_dir"] = str(tmp_path)
    cfg = tmp_path / "neus.yaml"
    cfg.write_text(yaml.dump(d))
    tool = _tool()
    args, _ = tool.parse(["--config", str(cfg)])
    assert (args.narrow_band, args.band_brick, args.band_lipschitz) == (False, 8, mesh_util.BAND_LIPSCHITZ)
    args, _ = tool.parse(["--config", str(cfg), "--narrow_band", "--band_brick", "4", "--band_lipschitz", "2.5"])
    assert (args.narrow_band, args.band_brick, args.band_lipschitz) == (True, 4, 2.5)
    seen = {}
    real = mesh_util.extract_mesh

    def spy(*a, **kw):
        seen.update(kw)
        return real(*a, **kw)
    monkeypatch.setattr(mesh_util, "extract_mesh", spy)
    out = {}
    for name, extra in (("dense", []), ("band", ["--narrow_band", "--band_brick", "4", "--band_lipschitz", "2.5"])):
        out[name] = str(tmp_path / f"{name}.ply")
        monkeypatch.setattr(sys, "argv", ["extract_surface.py", "--config", str(cfg), "--N", "48", "--out", out[name]] + extra)
        torch.manual_seed(0)                                         # no checkpoint: the tool builds the model's random initialisation anew
        tool.main()
        printed = capsys.readouterr().out
        assert out[name] in printed and (("evaluated_points" in printed) == bool(extra))
        assert (seen["narrow_band"], seen["band_brick"], seen["band_lipschitz"]) == ((True, 4, 2.5) if extra else (False, 8, mesh_util.BAND_LIPSCHITZ))
    assert open(out["dense"], "rb").read() == open(out["band"], "rb").read()
