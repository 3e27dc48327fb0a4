"""csrc/marching_cubes.hip (k_mc_emit_edges) and csrc/mesh_vertices.hip against the numpy statement of their rules in tests/mesh_vertices_ref.py -
edge records and points bit for bit, the refinement step bit for bit in its state and to a derived rounding bound in the new t - then the
refinement loop on analytic fields, and extract_mesh with refined vertices, normals and colours end to end on the two sphere-initialised models
against the mesh predicates of tests/mc_ref.py and the CPU oracle."""
import numpy as np
import pytest
import torch

import mc_ref
import mesh_vertices_ref as mv
from test_gpu_marching_cubes import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOLUMES = ["one_cell", "noncubic_5x7x70", "entries_equal_level", "noise_24", "noise_70"]
SENTINEL = 0x7FC12345          # a NaN with a payload: a row that keeps these bits was not written


def _counted(name):
    """(vol, level, spacing, origin, ws, V, F) of a volume of test_gpu_marching_cubes.CASES after mc_count."""
    from nerfart_amd import hip
    build, level, spacing, origin = CASES[name]
    vol = build()
    ws, counts = hip.mc_count(vol, level)
    V, F, bad = (int(c) for c in counts.cpu())
    assert V > 0 and not bad
    return vol, level, spacing, origin, ws, V, F


def _sentinels(*shape):
    """An int32 buffer of SENTINEL words (the fp32 outputs are written into int32 buffers: bit patterns are what is compared)."""
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)


def _np_bits(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", VOLUMES)
def test_edge_records_are_the_numpy_statement(name):
    from nerfart_amd import hip
    vol, level, _, _, ws, V, _ = _counted(name)
    r_edge, r_bracket, r_t, r_best, r_side = mv.edge_records(vol.cpu().numpy(), level)
    assert len(r_edge) == V
    if name == "entries_equal_level":                      # t exactly 0 or 1, g0 or g1 exactly 0
        assert (r_t == 0).sum() > 20 and (r_t == 1).sum() > 20 and (r_bracket[:, 1] == 0).sum() > 20 and (r_bracket[:, 3] == 0).sum() > 20
    # the buffers carry one row past V: it keeps its bits
    edge, bracket, t, best = _sentinels(V + 1), _sentinels(V + 1, 4), _sentinels(V + 1), _sentinels(V + 1, 2)
    side = torch.full((V + 1,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = hip.lib.nerfart_mc_emit_edges(vol.data_ptr(), *vol.shape, float(level), ws.data_ptr(), ws.numel(), edge.data_ptr(), bracket.data_ptr(),
                                       t.data_ptr(), best.data_ptr(), side.data_ptr(), V, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib.nerfart_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_np_bits(edge[:V]).view(np.uint32), r_edge)
    assert np.array_equal(_np_bits(bracket[:V]).view(np.uint32), mv.bits(r_bracket))
    assert np.array_equal(_np_bits(t[:V]).view(np.uint32), mv.bits(r_t))
    assert np.array_equal(_np_bits(best[:V]).view(np.uint32), mv.bits(r_best))
    assert np.array_equal(_np_bits(side[:V]), r_side)
    for buf in (edge, bracket, t, best):
        assert (buf[V:] == SENTINEL).all()
    assert int(side[V]) == 0xA5
    # the wrapper allocates exactly V rows and gives the same bits; and so does a second run
    for _ in range(2):
        w = hip.mc_emit_edges(vol, level, ws, V)
        assert torch.equal(w[0], edge[:V]) and torch.equal(w[4], side[:V])
        for got, want in zip(w[1:4], (bracket, t, best)):
            assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want[:V])


@pytest.mark.parametrize("name", VOLUMES)
def test_edge_points_are_mc_emits_vertices_and_the_one_rounding_formula(name):
    from nerfart_amd import hip
    vol, level, spacing, origin, ws, V, F = _counted(name)
    verts, _ = hip.mc_emit(vol, level, origin, spacing, ws, V, F)
    edge, _, t, _, _ = hip.mc_emit_edges(vol, level, ws, V)
    pts = hip.mesh_edge_points(edge, t, vol.shape, origin, spacing)
    assert torch.equal(pts, verts)                          # the non-cubic spacing / origin of noncubic_5x7x70 and one_cell included
    e = edge.cpu().numpy()
    want = mv.edge_points(e, t.cpu().numpy(), vol.shape, origin, spacing)
    assert np.array_equal(mv.bits(pts.cpu().numpy()), mv.bits(want))
    tr = np.random.default_rng(3).uniform(0.0, 1.0, size=V).astype(np.float32)
    tr[:: 7], tr[3:: 11] = 0.0, 1.0
    got = hip.mesh_edge_points(edge, torch.from_numpy(tr).to(DEV), vol.shape, origin, spacing)
    assert np.array_equal(mv.bits(got.cpu().numpy()), mv.bits(mv.edge_points(e, tr, vol.shape, origin, spacing)))
    # an edge that is none of the volume's writes nothing: a point index past the volume, and the last point (no neighbour toward any axis)
    n = vol.numel()
    nx, ny, nz = vol.shape
    foreign = [3 * n, 3 * n + 2, 2 ** 31 - 1, -1, -3, 3 * (n - 1), 3 * (n - 1) + 1, 3 * (n - 1) + 2,
               3 * (nz - 1) + 2, 3 * ((ny - 1) * nz) + 1, 3 * ((nx - 1) * ny * nz) + 0]
    fe = torch.tensor(foreign + [int(e[0])], dtype=torch.int64).to(torch.int32).to(DEV)
    out = torch.full((len(foreign) + 1, 3), 123.5, device=DEV)
    hip.mesh_edge_points(fe, torch.full((len(foreign) + 1,), 0.5, device=DEV), vol.shape, origin, spacing, out=out)
    assert (out[:-1] == 123.5).all() and (out[-1] != 123.5).any()


def _step_inputs(V, level, k, rng):
    """f [V] of step k: mixed signs of moderate size (no overflow or underflow in step 5), and by position the special values."""
    f = (rng.uniform(0.01, 1.0, size=V) * rng.choice([-1.0, 1.0], size=V)).astype(np.float32) + np.float32(level)
    pos = (np.arange(V) + 3 * k) % 16
    f[pos == 3] = np.float32(level)                        # g == 0
    f[pos == 5] = np.nan
    f[pos == 7] = np.inf
    f[pos == 9] = -np.inf
    return f


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("V", [1, 255, 256, 257, 1758])
def test_refine_step_is_the_numpy_rule(V, level):
    from nerfart_amd import hip
    rng = np.random.default_rng(V)
    # a sign-changing bracket per vertex as nerfart_mc_emit_edges leaves it; every 16th vertex (position 11) starts with g1 == g0 instead and is
    # handed f = g0 + level first, so step 5 divides by zero
    g0 = (rng.uniform(0.01, 1.0, size=V) * rng.choice([-1.0, 1.0], size=V)).astype(np.float32)
    g1 = (-np.sign(g0) * rng.uniform(0.01, 1.0, size=V)).astype(np.float32)
    flat = np.arange(V) % 16 == 11
    g1[flat] = g0[flat] = np.float32(2.0)
    bracket = np.stack([np.zeros(V, np.float32), g0, np.ones(V, np.float32), g1], -1)
    with np.errstate(all="ignore"):
        t = np.where(flat, np.float32(0.5), (-g0) / (g1 - g0)).astype(np.float32)
    best = np.stack([t, np.full(V, np.inf, np.float32)], -1)
    side = np.zeros(V, np.uint8)
    pad = lambda a, fill: np.concatenate([a, np.full((1,) + a.shape[1:], fill, a.dtype)])          # one sentinel row past V
    sent = np.array([SENTINEL], np.uint32).view(np.float32)[0]
    d_br, d_t, d_bs, d_sd = (torch.from_numpy(pad(a, s)).to(DEV) for a, s in ((bracket, sent), (t, sent), (best, sent), (side, 0xA5)))
    seen_sides, halvings, mismatched = set(), 0, 0
    for k in range(5):
        f = _step_inputs(V, level, k, rng)
        if k == 0:
            f[flat] = np.float32(2.0) + np.float32(level)
        d_f = torch.from_numpy(f).to(DEV)
        rc = hip.lib.nerfart_mesh_edge_refine_step(d_f.data_ptr(), float(level), V, d_br.data_ptr(), d_t.data_ptr(), d_bs.data_ptr(),
                                                   d_sd.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, hip.lib.nerfart_last_error()
        torch.cuda.synchronize()
        r_br, r_t, r_bs, r_sd = mv.refine_step(f, level, bracket, t, best, side)
        g = f - np.float32(level)
        live = ~np.isnan(g) & (g != 0)
        halvings += int((live & (side != 0) & (r_sd == side)).sum())              # the same end moves twice in a row: the other end's value is halved
        seen_sides |= set(side.tolist())
        got_br, got_t, got_bs, got_sd = (a.cpu().numpy() for a in (d_br, d_t, d_bs, d_sd))
        assert np.array_equal(mv.bits(got_br[:V]), mv.bits(r_br)), k
        assert np.array_equal(mv.bits(got_bs[:V]), mv.bits(r_bs)), k
        assert np.array_equal(got_sd[:V], r_sd), k
        for a in (got_br, got_t, got_bs):
            assert (mv.bits(a[V:]) == SENTINEL).all()
        assert got_sd[V] == 0xA5
        # the new t.  Rows the step leaves alone (NaN, g == 0) keep their bits.  Else, against float64 on the (bit-identical) updated bracket:
        # t = t0 - q, q = g0 (t1 - t0) / (g1 - g0) takes five fp32 roundings - the difference, the product, the denominator, the quotient (a
        # relative 4 u + O(u^2) on q, u = 2^-24) and the final subtraction (u on the result) - so |t - t64| <= 4.02 u |q| + 1.01 u |t0 - q|;
        # clamping into the bracket moves two numbers no further apart.  Where float64 is not finite the rule's midpoint is exact up to its own two
        # roundings, which numpy's fp32 reproduces.
        assert np.array_equal(mv.bits(got_t[:V][~live]), mv.bits(t[~live])), k
        t64, q, fin = mv.next_t64(r_br)
        lo, hi = np.minimum(r_br[:, 0], r_br[:, 2]).astype(np.float64), np.maximum(r_br[:, 0], r_br[:, 2]).astype(np.float64)
        u = 2.0 ** -24
        sel = live & fin
        bound = 4.02 * u * np.abs(q[sel]) + 1.01 * u * np.abs(t64[sel])
        delta = np.abs(got_t[:V][sel].astype(np.float64) - np.clip(t64[sel], lo[sel], hi[sel]))
        assert (delta <= bound).all(), (k, float((delta / np.maximum(bound, 1e-300)).max()))
        mid = live & ~fin
        assert np.array_equal(mv.bits(got_t[:V][mid]), mv.bits(r_t[mid])), k
        assert ((got_t[:V] >= lo) & (got_t[:V] <= hi))[live].all() and ((got_t[:V] >= 0) & (got_t[:V] <= 1)).all()
        mismatched += int((mv.bits(got_t[:V]) != mv.bits(r_t)).sum())
        bracket, t, best, side = got_br[:V].copy(), got_t[:V].copy(), got_bs[:V].copy(), got_sd[:V].copy()      # the next step starts from the kernel's own state
    print(f"[refine step] V = {V}, level = {level}: {mismatched} new t of {5 * V} differ in bits from the numpy fp32 rule; {halvings} Illinois halvings")
    if V >= 255:
        assert seen_sides == {0, 1, 2} and halvings > 0 and (best[:, 1] == 0).any()


@pytest.mark.parametrize("name", list(mv.FIELDS))
def test_refinement_loop_on_analytic_fields(name):
    """The kernels in the loop of mesh_util.refine_vertices, f computed on the host in float64: the three demands of the CPU test."""
    from nerfart_amd import hip
    vol, origin, spacing = mv.field_volume(name)
    dvol = torch.from_numpy(vol).to(DEV)
    ws, counts = hip.mc_count(dvol, 0.0)
    V = int(counts[0])

    def points(edge, t, dims, o, s):
        return hip.mesh_edge_points(edge, t, dims, o, s).cpu().numpy()

    def step(f, level, bracket, t, best, side):
        hip.mesh_edge_refine_step(torch.from_numpy(f).to(DEV), level, bracket, t, best, side)
        return bracket, t, best, side

    t_best, hist = mv.refine_loop(vol, 0.0, origin, spacing, mv.FIELDS[name][0], 5, records=lambda v, l: hip.mc_emit_edges(dvol, l, ws, V),
                                  points=points, step=step, host=lambda a: a.cpu().numpy())
    assert len(t_best) == len(mv.edge_records(vol, 0.0)[0])
    mv.check_refinement(name, t_best, hist)


def _oracle_forward(framework, sd, p, view):
    """(rgb, nabla) of the CPU oracle, as tests/test_gpu_parity.py::test_sdf_nabla_and_radiance_match_oracle takes them."""
    from oracle import nets
    if framework == "VolSDF":
        rad, _, nab = nets.volsdf_forward(sd, p, view)
        return rad.detach(), nab.detach()
    return nets.neus_forward_radiance(sd, p, view).detach(), nets.surface_forward_with_nablas(sd, p)[1].detach()


# max |g_best| after 1 -> after 5 evaluations, measured on the MI355X: NeuS 1.190e-3 -> 8.11e-6 (a factor of 147), VolSDF
# 2.944e-3 -> 5.56e-5 (53).  The asserted factor is half the measured one, rounded down to a power of ten, and at least 10: 10 for both.
REDUCTION = {"NeuS": 10.0, "VolSDF": 10.0}


@pytest.mark.parametrize("framework,volume_size", [("NeuS", 2.0), ("VolSDF", 3.0)])
def test_extract_mesh_with_refined_vertices_normals_and_colours(framework, volume_size, tmp_path):
    from nerfart_amd import scene, mesh_util, hip
    N, level = 48, 0.0
    model, _, _ = scene.build_model(framework, seed=0, beta=None if framework == "NeuS" else 0.01, device=DEV)
    surface = model.implicit_surface
    path = str(tmp_path / "surface.ply")
    assert mesh_util.extract_mesh(surface, volume_size=volume_size, N=N, filepath=path, refine_evals=5, vertex_normals=True, color_model=model) == path
    mesh = mv.read_ply(path)
    verts, faces, normals, colors = mesh["verts"], mesh["faces"], mesh["normals"], mesh["colors"]
    # faces: the unrefined mesh's, and still a closed oriented sphere
    vol = mesh_util.sdf_volume(surface, volume_size=volume_size, N=N)
    place_o, place_s = mesh_util.placement_frame(N, volume_size)
    v0, f0 = mesh_util.marching_cubes(vol, level=level, spacing=place_s, origin=place_o)
    v0 = v0.cpu().numpy()
    V = len(v0)
    assert np.array_equal(faces, f0.cpu().numpy()) and len(faces) > 1000 and verts.shape == (V, 3)
    assert mc_ref.is_closed(faces) and mc_ref.is_consistently_oriented(faces)
    assert mc_ref.euler_characteristic(V, faces) == 2 and mc_ref.signed_volume(verts, faces) > 0
    # positions: a vertex moves along its edge's axis only (one that did not move: its first evaluation stayed the best), by at most one step
    ws, _ = hip.mc_count(vol, level)
    edge5, t5, g5 = mesh_util.refine_vertices(surface, vol, level, ws, V, volume_size, 5)
    axis = edge5.cpu().numpy() % 3
    moved = mv.bits(verts) != mv.bits(v0)
    assert not (moved & (np.arange(3)[None, :] != axis[:, None])).any()              # the other two components: equal bit for bit
    assert (np.abs(verts.astype(np.float64) - v0)[np.arange(V), axis] <= place_s[0]).all()
    print(f"[mesh] {framework}: V = {V}, F = {len(faces)}, {int(moved.any(1).sum())} vertices moved")
    assert moved.any()
    assert np.array_equal(mv.bits(verts), mv.bits(hip.mesh_edge_points(edge5, t5, vol.shape, place_o, place_s).cpu().numpy()))
    # residuals: g_best is a value the SDF kernel returns at the returned points, and no worse than the interpolated vertex's
    pts = hip.mesh_edge_points(edge5, t5, vol.shape, *mesh_util.model_frame(N, volume_size))
    assert torch.equal(g5, surface.forward(pts) - level)
    edge1, t1, g1 = mesh_util.refine_vertices(surface, vol, level, ws, V, volume_size, 1)
    assert torch.equal(edge1, edge5) and (g5.abs() <= g1.abs()).all()
    assert torch.equal(hip.mesh_edge_points(edge1, t1, vol.shape, place_o, place_s).cpu(), torch.from_numpy(v0))      # one evaluation: today's vertices
    first, last = float(g1.abs().max()), float(g5.abs().max())
    print(f"[mesh] {framework}: max |g_best| after 1 evaluation {first:.3e}, after 5 {last:.3e}, ratio {first / max(last, 1e-300):.3g}")
    assert last * REDUCTION[framework] <= first
    # normals: unit, and on the side the winding calls outside
    assert np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    tri = verts.astype(np.float64)[faces]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    big = np.linalg.norm(fn, axis=1) > 1e-3 * place_s[0] ** 2                       # twice the area: above a thousandth of a grid face
    assert big.sum() > len(faces) // 2
    assert (np.einsum("ij,ij->i", fn, normals.astype(np.float64)[faces].mean(1))[big] > 0).all()
    # against the oracle at the model-frame points, view = -normal
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    rgb_ref, nab_ref = _oracle_forward(framework, sd, pts.cpu(), -torch.from_numpy(normals))
    n_err = (torch.from_numpy(normals) - torch.nn.functional.normalize(nab_ref, dim=-1)).abs().max().item()
    c_err = (torch.from_numpy(colors.astype(np.float32)) - 255.0 * rgb_ref).abs().max().item()
    print(f"[mesh] {framework}: max |normal - oracle| = {n_err:.2e}, max |u8 - 255 rgb_oracle| = {c_err:.4f} (allowed {0.5 + 255e-4:.4f})")
    assert n_err <= 1e-3
    assert c_err <= 0.5 + 255 * 1e-4
    # the attributes alone reproduce the file's
    n2, c2 = mesh_util.vertex_attributes(model, pts)
    assert np.array_equal(mv.bits(n2.cpu().numpy()), mv.bits(normals)) and np.array_equal(c2.cpu().numpy(), colors)


def test_default_options_write_todays_file(tmp_path):
    """refine_evals=0, vertex_normals=False, color_model=None: the two-element file of marching_cubes + write_ply, byte for byte; normals alone need
    no radiance net."""
    from nerfart_amd import scene, mesh_util
    N, volume_size = 24, 2.0
    model, _, _ = scene.build_model("NeuS", seed=0, beta=None, device=DEV)
    a = mesh_util.extract_mesh(model.implicit_surface, volume_size=volume_size, N=N, filepath=str(tmp_path / "a.ply"),
                               refine_evals=0, vertex_normals=False, color_model=None)
    vol = mesh_util.sdf_volume(model.implicit_surface, volume_size=volume_size, N=N)
    v, f = mesh_util.marching_cubes(vol, spacing=[volume_size / N] * 3, origin=[-volume_size / 2.0] * 3)
    b = mesh_util.write_ply(str(tmp_path / "b.ply"), v, f)
    assert open(a, "rb").read() == open(b, "rb").read()
    c = mv.read_ply(mesh_util.extract_mesh(model.implicit_surface, volume_size=volume_size, N=N, filepath=str(tmp_path / "c.ply"), vertex_normals=True))
    assert c["colors"] is None and np.array_equal(mv.bits(c["verts"]), mv.bits(v.cpu().numpy())) and np.array_equal(c["faces"], f.cpu().numpy())
    assert np.abs(np.linalg.norm(c["normals"].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
