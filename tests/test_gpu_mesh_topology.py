"""csrc/mesh_topology.hip (mesh_util.half_edges / mesh_topology, tools/check_mesh.py) against the numpy statement tests/mesh_topology_ref.py, which
tests/test_mesh_topology_ref.py holds to answers known by hand.  Every integer output - twin, edge_uses, vertex_fans, info, counts - is compared
by equality, for every table size; the fp64 sums against math.fsum of the statement's per-face terms within m 2^-53 sum|term| (m = the
component's proper faces: the bound of recursive summation in any order - the atomics' order is not fixed; the terms themselves are the
statement's bit for bit: no contraction, a correctly rounded fp64 sqrt).  Hand meshes, the marching-cubes meshes, a clustered mesh with real
defects, ragged sizes, long parent chains, the write discipline, the refusals, mesh_topology end to end and the tool."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mc_ref
import mesh_components_ref as cref
import mesh_topology_ref as ref
from conftest import REPO
from test_mesh_components_ref import MESHES, mesh
from test_mesh_topology_ref import TET_VERTS, shells_simplified, topo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
PAD = 32                   # sentinel words on either side of every output array
U = 2.0 ** -53


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)               # a copy: the shared reference arrays are read-only


def gpu_half_edges(faces, V, table_log2=0):
    """(ws, (twin, edge_uses, vertex_fans, info) as numpy)"""
    from nerfart_amd import hip
    F = len(faces)
    ws, twin, uses, fans, info = hip.mesh_half_edges(dev(faces, np.int32).reshape(-1, 3), V, table_log2)
    assert twin.dtype == uses.dtype == fans.dtype == info.dtype == torch.int32
    assert twin.shape == uses.shape == (3 * F,) and fans.shape == (V,) and info.shape == (16,)
    return ws, (twin.cpu().numpy(), uses.cpu().numpy().view(np.uint32), fans.cpu().numpy().view(np.uint32), info.cpu().numpy().view(np.uint32))


def check_half_edges(faces, V, table_log2=0, want=None):
    want = want or ref.topology(faces, V)
    ws, got = gpu_half_edges(faces, V, table_log2)
    for g, key in zip(got, ("twin", "edge_uses", "vertex_fans", "info")):
        assert np.array_equal(g, want[key]), (key, table_log2)
    assert got[3][11] == 0                                                  # the overflow flag
    return ws, want


def check_stats(verts, faces, V, ws):
    from nerfart_amd import hip
    label = cref.components(faces, V)[0]
    want = ref.component_stats(verts, faces, V, label)
    counts, measure = hip.mesh_component_stats(dev(verts, np.float32).reshape(-1, 3), dev(faces, np.int32).reshape(-1, 3), dev(label, np.int32), ws)
    assert counts.dtype == torch.int32 and measure.dtype == torch.float64 and tuple(counts.shape) == (V, 6) and tuple(measure.shape) == (V, 2)
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want["counts"])
    got = measure.cpu().numpy()
    bound = want["faces"][:, None] * U * want["abs_sum"]
    err = np.abs(got - want["measure"])
    print(f"[topology] worst share of the summation bound: {float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)):.4f} "
          f"(m up to {int(want['faces'].max(initial=0))})")
    assert (err <= bound).all(), (err.max(), bound.max())
    assert (got[want["faces"] == 0] == 0).all()                             # nothing but a label carries a sum
    return want


def hand_meshes():
    """name -> (V, faces): the meshes tests/test_mesh_topology_ref.py answers by hand"""
    out = {"tetrahedron": (4, ref.TETRAHEDRON), "torus_4x7": ref.grid_faces(4, 7, True, True), "sheet_4x7": ref.grid_faces(4, 7),
           "annulus_4x7": ref.grid_faces(4, 7, wrap_u=True), "moebius_5": ref.moebius_faces(5),
           "two_tetrahedra_one_vertex": (7, np.concatenate([ref.TETRAHEDRON, np.array([[0, 4, 5], [0, 5, 6], [0, 6, 4], [4, 6, 5]], dtype=np.int32)])),
           "three_on_one_edge": (5, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32)),
           "flipped_pair": (4, np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int32)),
           "degenerate_bad_duplicate": (6, np.array([[0, 1, 2], [3, 3, 1], [0, 1, 7], [-1, 0, 1], [0, 1, 2]], dtype=np.int32)),
           "no_faces": (5, np.zeros((0, 3), dtype=np.int32)), "nothing": (0, np.zeros((0, 3), dtype=np.int32)),
           "no_vertices": (0, np.array([[0, 1, 2], [0, 0, 0]], dtype=np.int32)),
           "one_vertex_one_face": (1, np.array([[0, 0, 0]], dtype=np.int32)), "one_face": (3, np.array([[2, 0, 1]], dtype=np.int32))}
    return out


@pytest.mark.parametrize("name", list(hand_meshes()))
def test_hand_meshes(name):
    V, faces = hand_meshes()[name]
    ws, want = check_half_edges(faces, V)
    rng = np.random.default_rng(1)
    check_stats(rng.uniform(-1, 1, size=(V, 3)).astype(np.float32), faces, V, ws)
    if name == "no_vertices":
        assert want["info"][:3].tolist() == [0, 0, 2] and want["twin"].tolist() == [-4] * 6


def test_tetrahedron_measures_in_closed_form():
    from nerfart_amd import mesh_util
    r = mesh_util.mesh_topology(dev(TET_VERTS), dev(ref.TETRAHEDRON))
    assert r["watertight"] and r["euler"] == 2 and len(r["components"]) == 1
    k = r["components"][0]
    assert k["genus"] == 0 and k["volume"] == pytest.approx(1 / 6, rel=1e-15) and k["area"] == pytest.approx(1.5 + np.sqrt(3) / 2, rel=1e-15)


@pytest.mark.parametrize("source", ["reference_faces", "gpu_marching_cubes"])
@pytest.mark.parametrize("name", list(MESHES))
def test_outputs_are_the_reference_on_marching_cubes_meshes(name, source):
    from nerfart_amd import mesh_util
    V, faces = mesh(name)[:2]
    if source == "gpu_marching_cubes":
        gverts, gfaces = mesh_util.marching_cubes(dev(MESHES[name][0]()), 0.0)
        assert gverts.shape[0] == V and np.array_equal(gfaces.cpu().numpy(), faces)
        verts = gverts.cpu().numpy()
        twin, uses, fans, info = mesh_util.half_edges(gfaces, V)
        want = topo(name)
        for g, key in zip((twin, uses, fans, info), ("twin", "edge_uses", "vertex_fans", "info")):
            assert g.device == gfaces.device and np.array_equal(g.cpu().numpy().view(want[key].dtype), want[key]), key
    else:
        verts = mc_ref.marching_cubes(MESHES[name][0](), 0.0)[0]
    ws, _ = check_half_edges(faces, V, want=topo(name))
    check_stats(verts, faces, V, ws)


def test_per_face_terms_are_the_reference_bit_for_bit():
    """3,000 separate triangles of every size and aspect: each is a component of its own, so measure[label] IS the face's area and volume term
    (0 + term is exact) - equal to the statement's bits: the operation order, no contraction, and a correctly rounded fp64 sqrt and division."""
    from nerfart_amd import hip
    n = 3000
    rng = np.random.default_rng(9)
    verts = (rng.normal(size=(3 * n, 3)) * 10.0 ** rng.uniform(-3, 3, size=(3 * n, 1))).astype(np.float32)
    faces = rng.permutation(3 * n).astype(np.int32).reshape(n, 3)
    thin = faces[::3]
    verts[thin[:, 1]] = verts[thin[:, 0]] + np.float32(1e-3) * verts[thin[:, 1]]      # slivers: heavy cancellation in the cross product
    label = faces.min(axis=1)
    full = np.arange(3 * n, dtype=np.int32)
    full[faces.reshape(-1)] = np.repeat(label, 3)
    assert np.array_equal(full, cref.components(faces, 3 * n)[0])
    area, volume = ref.face_terms(verts, faces)
    ws = gpu_half_edges(faces, 3 * n)[0]
    _, measure = hip.mesh_component_stats(dev(verts), dev(faces), dev(full), ws)
    got = measure.cpu().numpy()[label]
    assert np.array_equal(got[:, 0].view(np.uint64), area.view(np.uint64)) and np.array_equal(got[:, 1].view(np.uint64), volume.view(np.uint64))
    assert len(np.unique(np.floor(np.log10(area[area > 0])))) > 8


def test_a_clustered_mesh_with_real_defects():
    verts, faces = shells_simplified()
    ws, want = check_half_edges(faces, len(verts))
    assert want["info"][7] > 0 and want["info"][8] > 0 and (want["twin"] == -3).any() and want["vertex_fans"].max() > 1
    check_stats(verts, faces, len(verts), ws)


def test_the_same_bits_for_every_table_size():
    """85 separate triangles: 255 distinct edges.  The smallest legal table has 256 slots (load factor 255 / 256: probe chains through most of the
    table), the default 1024, 512 lies between; then a mesh with defects and an open marching-cubes mesh, whose smallest tables are not full."""
    from nerfart_amd import hip
    i = np.arange(85, dtype=np.int32)
    separate = np.stack([3 * i, 3 * i + 1, 3 * i + 2], axis=1)
    assert hip.mesh_topology_workspace_bytes(255, 85, 8) < hip.mesh_topology_workspace_bytes(255, 85, 9) < hip.mesh_topology_workspace_bytes(255, 85, 0) \
        == hip.mesh_topology_workspace_bytes(255, 85, 10)
    for V, faces, least in ((255, separate, 8), (len(shells_simplified()[0]), shells_simplified()[1], None), mesh("noise_9x10x11_open")[:2] + (None,)):
        least = least or int(np.ceil(np.log2(3 * len(faces) + 1)))
        assert 2 ** least >= 3 * len(faces) + 1 > 2 ** (least - 1)
        want = ref.topology(faces, V)
        label = dev(cref.components(faces, V)[0], np.int32)
        verts = torch.rand(V, 3, device=DEV)
        runs = []
        for log2 in (0, least, least + 1):
            ws, _ = check_half_edges(faces, V, log2, want=want)
            counts, measure = hip.mesh_component_stats(verts, dev(faces), label, ws)
            runs.append(counts.cpu().numpy())
        assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
        f = dev(faces)
        with pytest.raises(hip.NerfartHipError, match="3 F"):               # refused with 2 before any launch
            hip.mesh_half_edges(f, V, least - 1)
        with pytest.raises(hip.NerfartHipError, match="3 F"):
            hip.mesh_topology_workspace_bytes(V, len(faces), least - 1)


def test_two_runs_give_the_same_integers():
    V, faces = mesh("noise_24")[:2]
    a, b = gpu_half_edges(faces, V)[1], gpu_half_edges(faces, V)[1]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _messy(V, F, seed):
    """random faces over few vertices: duplicate, flipped, non-manifold, degenerate and (a few) bad faces at once"""
    rng = np.random.default_rng(seed)
    faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    faces[rng.random(F) < 0.05, 1] = V + 3
    faces[rng.random(F) < 0.05, 2] = -1
    return faces


def test_sizes_around_wave_and_block_boundaries():
    seen = np.zeros(16, dtype=np.int64)
    for V in (1, 2, 63, 65, 300):
        for F in (1, 85, 255, 256, 257, 600):
            faces = _messy(V, F, 7 * V + F)
            ws, want = check_half_edges(faces, V)
            check_stats(np.random.default_rng(V).normal(size=(V, 3)).astype(np.float32), faces, V, ws)
            seen += want["info"]
    assert (seen[:11] > 0).all()                                            # every kind of face, edge, fan and loop has been met


@pytest.mark.parametrize("order", ["permuted", "smallest_index_at_the_far_end"])
def test_long_chains_in_both_union_finds(order):
    """A strip of 20,000 triangles: every interior edge joins two corners into a fan, and its boundary is ONE loop of 20,002 edges - parent chains
    as long as the strip among the corners and among the vertices."""
    n = 20000
    strip, V = cref.triangle_strip(n), n + 2
    strip[1::2] = strip[1::2][:, [0, 2, 1]]                                 # alternate, so that the strip is oriented
    if order == "permuted":
        rng = np.random.default_rng(7)
        faces = rng.permutation(V)[strip][rng.permutation(n)].astype(np.int32)
    else:
        faces = (V - 1 - strip).astype(np.int32)
    ws, want = check_half_edges(faces, V)
    s = ref.summary(want["info"])
    assert s["boundary_loops"] == 1 and s["longest_loop"] == n + 2 and s["flipped_edges"] == 0 and s["euler"] == 1 and (want["vertex_fans"] == 1).all()
    check_stats(np.random.default_rng(2).normal(size=(V, 3)).astype(np.float32), faces, V, ws)


def test_sentinels_around_every_output_and_bad_faces_touch_nothing():
    from nerfart_amd import hip
    V, faces = mesh("noise_12")[:2]
    faces = faces.copy()
    faces[100, 1], faces[2000, 2], faces[7] = -1, V, (5, 5, 9)
    F = len(faces)
    want = ref.topology(faces, V)
    assert want["info"][:3].tolist() == [F - 3, 1, 2]
    label = cref.components(faces, V)[0]
    verts = np.random.default_rng(4).normal(size=(V, 3)).astype(np.float32)
    stats = ref.component_stats(verts, faces, V, label)
    st = torch.cuda.current_stream().cuda_stream
    full = lambda n, dt=torch.int32: torch.full((n + 2 * PAD,), SENTINEL, dtype=dt, device=DEV)
    twin, uses, fans, info, counts, measure = full(3 * F), full(3 * F), full(V), full(16), full(6 * V), full(2 * (2 * V))
    ws = torch.zeros(hip.mesh_topology_workspace_bytes(V, F), dtype=torch.uint8, device=DEV)
    f, v, l = dev(faces), dev(verts), dev(label, np.int32)
    assert hip.lib.nerfart_mesh_half_edges(f.data_ptr(), F, V, 0, ws.data_ptr(), ws.numel(), twin[PAD:].data_ptr(), uses[PAD:].data_ptr(),
                                           fans[PAD:].data_ptr(), info[PAD:].data_ptr(), st) == 0
    before = ws.clone()
    assert hip.lib.nerfart_mesh_component_stats(v.data_ptr(), f.data_ptr(), F, V, l.data_ptr(), ws.data_ptr(), ws.numel(), counts[PAD:].data_ptr(),
                                                measure[PAD:].data_ptr(), st) == 0
    assert torch.equal(ws, before)                                          # the stats run from the untouched workspace
    for buf, w, n in ((twin, want["twin"], 3 * F), (uses, want["edge_uses"], 3 * F), (fans, want["vertex_fans"], V), (info, want["info"], 16),
                      (counts, stats["counts"].reshape(-1), 6 * V)):
        b = buf.cpu().numpy().view(np.uint32)
        assert (b[:PAD] == SENTINEL).all() and (b[PAD + n:] == SENTINEL).all()
        assert np.array_equal(b[PAD:PAD + n], w.view(np.uint32))
    m = measure.cpu().numpy().view(np.uint32)
    assert (m[:PAD] == SENTINEL).all() and (m[PAD + 4 * V:] == SENTINEL).all()
    got = m[PAD:PAD + 4 * V].copy().view(np.float64).reshape(V, 2)
    assert (np.abs(got - stats["measure"]) <= stats["faces"][:, None] * U * stats["abs_sum"]).all()


def test_refusals_leave_the_outputs_alone():
    from nerfart_amd import hip
    V, faces = 4, dev(ref.TETRAHEDRON)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((64,), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.zeros(hip.mesh_topology_workspace_bytes(V, 4), dtype=torch.uint8, device=DEV)
    o = out.data_ptr()
    err = lambda: hip.lib.nerfart_last_error().decode()
    half = lambda **kw: hip.lib.nerfart_mesh_half_edges(*[kw.get(k, d) for k, d in (("faces", faces.data_ptr()), ("F", 4), ("V", V), ("table_log2", 0),
                                                                                    ("ws", ws.data_ptr()), ("ws_bytes", ws.numel()), ("twin", o),
                                                                                    ("edge_uses", o), ("vertex_fans", o), ("info", o), ("stream", st))])
    stats = lambda **kw: hip.lib.nerfart_mesh_component_stats(*[kw.get(k, d) for k, d in (("verts", o), ("faces", faces.data_ptr()), ("F", 4), ("V", V),
                                                                                          ("label", o), ("ws", ws.data_ptr()), ("ws_bytes", ws.numel()),
                                                                                          ("counts", o), ("measure", o), ("stream", st))])
    assert half(table_log2=3) == 2 and "3 F + 1" in err()                   # 8 < 13
    assert half(table_log2=32) == 2 and "table_log2" in err()
    assert half(ws_bytes=ws.numel() - 1) == 2 and "workspace" in err() and half(ws=ws.data_ptr() + 4) == 2 and "aligned" in err()
    assert half(V=1 << 31) == 2 and "2^31" in err() and half(F=1 << 31) == 2 and "2^31" in err() and half(F=1431655766) == 2 and "2^32" in err()
    for k in ("faces", "ws", "twin", "edge_uses", "vertex_fans", "info"):
        assert half(**{k: None}) == 2 and "null" in err(), k
    for k in ("verts", "faces", "label", "ws", "counts", "measure"):
        assert stats(**{k: None}) == 2 and "null" in err(), k
    assert stats(ws_bytes=hip.mesh_topology_workspace_bytes(V, 4, 4) - 1) == 2 and "workspace" in err()
    assert stats(ws=ws.data_ptr() + 4) == 2 and "aligned" in err() and stats(measure=o + 4) == 2 and "aligned" in err()
    assert stats(V=1 << 31) == 2 and "2^31" in err()
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all() and not ws.any()


# ---- mesh_topology end to end and the tool -----------------------------------------------------------------------------------------------------

def check_report(verts, faces):
    """mesh_util.mesh_topology against ref.report: integers and verdicts equal, area and volume within the summation bound"""
    from nerfart_amd import mesh_util
    V = len(verts)
    got = mesh_util.mesh_topology(dev(verts, np.float32), dev(faces, np.int32))
    want = ref.report(verts, faces)
    tensors = got.pop("tensors")
    label = cref.components(faces, V)[0]
    stats = ref.component_stats(verts, faces, V, label)
    assert np.array_equal(tensors["label"].cpu().numpy(), label) and np.array_equal(tensors["counts"].cpu().numpy().view(np.uint32), stats["counts"])
    assert tensors["measure"].dtype == torch.float64 and tuple(tensors["measure"].shape) == (V, 2)
    assert len(got["components"]) == len(want["components"])
    for g, w in zip(got["components"], want["components"]):
        r = w["label"]
        for key, col in (("area", 0), ("volume", 1)):
            assert abs(g[key] - w[key]) <= stats["faces"][r] * U * stats["abs_sum"][r, col]
            assert isinstance(g[key], float)
        assert {k: v for k, v in g.items() if k not in ("area", "volume")} == {k: v for k, v in w.items() if k not in ("area", "volume")}
    assert {k: v for k, v in got.items() if k != "components"} == {k: v for k, v in want.items() if k != "components"}
    plain = mesh_util.mesh_topology(dev(verts, np.float32), dev(faces, np.int32), components=False)
    assert plain == {k: v for k, v in want.items() if k != "components"}
    return got


def test_mesh_topology_of_a_watertight_marching_cubes_mesh():
    from nerfart_amd import mesh_util
    V, faces, label, n_faces, _ = mesh("noise_12")
    verts = mc_ref.marching_cubes(MESHES["noise_12"][0](), 0.0)[0]
    got = check_report(verts, faces)
    assert got["watertight"] and got["closed"] and got["oriented"] and got["manifold"] and got["euler"] == -18 and got["boundary_loops"] == 0
    assert all(type(v) in (int, bool) for k, v in got.items() if k != "components")
    _, roots, count = mesh_util.mesh_components(dev(faces), V)             # the same order as mesh_components' ranking
    assert [k["label"] for k in got["components"]] == roots.tolist() and [k["faces"] for k in got["components"]] == count.tolist()
    assert [k["faces"] for k in got["components"]][:10] == MESHES["noise_12"][4]
    assert all(k["genus"] is not None and k["closed"] and k["volume"] > 0 and k["area"] > 0 for k in got["components"])
    assert sum(k["euler"] for k in got["components"]) == -18


def test_mesh_topology_of_the_clustered_shells():
    verts, faces = shells_simplified()
    got = check_report(verts, faces)
    assert got["closed"] and got["oriented"] and not got["manifold"] and not got["watertight"]
    assert (got["nonmanifold_edges"], got["bowtie_vertices"], got["euler"]) == (25, 39, -8)
    broken = [k for k in got["components"] if k["nonmanifold_edges"] or k["bowtie_vertices"]]
    assert broken and all(k["genus"] is None for k in broken)
    assert all(k["genus"] is not None for k in got["components"] if k not in broken and k["closed"] and k["faces"])


def test_mesh_topology_refuses_what_it_cannot_read():
    from nerfart_amd import mesh_util
    v, f = dev(TET_VERTS), dev(ref.TETRAHEDRON)
    with pytest.raises(ValueError, match="float32"):
        mesh_util.mesh_topology(v.double(), f)
    with pytest.raises(ValueError, match="int32"):
        mesh_util.mesh_topology(v, f.long())
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        mesh_util.mesh_topology(v, f.reshape(-1))
    with pytest.raises(ValueError, match="int32"):
        mesh_util.half_edges(f.long(), 4)
    with pytest.raises(ValueError, match="GPU"):
        mesh_util.mesh_topology(v.cpu(), f)


def _tool():
    spec = importlib.util.spec_from_file_location("check_mesh", os.path.join(REPO, "tools", "check_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tool_prints_the_direct_call_and_colours_the_defects(tmp_path, capsys):
    from nerfart_amd import mesh_util
    tool = _tool()
    verts, faces = shells_simplified()
    direct = mesh_util.mesh_topology(dev(verts), dev(faces))
    direct.pop("tensors")
    ply = mesh_util.write_ply(str(tmp_path / "m.ply"), verts, faces)
    uv = mesh_util.atlas_uvs(len(faces), 1)
    S, Cw, Ch, W, H = mesh_util.atlas_layout(len(faces), 1)
    obj = mesh_util.write_obj(str(tmp_path / "m.obj"), verts, faces, uv, np.zeros((H, W, 3), dtype=np.uint8))
    for path in (ply, obj):
        tool.main(["--mesh", str(path), "--components", "3"])
        line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
        want = dict(direct, components=direct["components"][:3])
        for g, w in zip(line["components"], want["components"]):            # the sums' last bits are free between two runs
            for key in ("area", "volume"):
                assert g.pop(key) == pytest.approx(w[key], rel=1e-12)
        assert {k: v for k, v in line.items() if k not in ("mesh", "n_components")} == \
            dict(want, components=[{k: v for k, v in c.items() if k not in ("area", "volume")} for c in want["components"]])
        assert line["n_components"] == len(direct["components"])
    out = str(tmp_path / "defects.ply")
    tool.main(["--mesh", ply, "--defects", out])
    capsys.readouterr()
    back = mesh_util.read_ply(out)
    assert np.array_equal(back["faces"], faces) and np.array_equal(back["verts"], verts)
    t = ref.topology(faces, len(verts))
    e = ref.edges(faces, len(verts))
    n = e["n_fwd"] + e["n_bwd"]
    colour = np.tile(np.array(tool.GREY, dtype=np.uint8), (len(verts), 1))
    colour[t["vertex_fans"] > 1] = tool.YELLOW
    colour[np.unique(e["key"][(n > 2) | ((n == 2) & ~((e["n_fwd"] == 1) & (e["n_bwd"] == 1)))])] = tool.MAGENTA
    colour[np.unique(e["key"][n == 1])] = tool.RED
    assert np.array_equal(back["colors"], colour) and (colour == tool.MAGENTA).all(axis=1).any() and (colour == tool.YELLOW).all(axis=1).any()
    # an open mesh: red along its boundary
    V, ofaces = ref.grid_faces(3, 4)
    overts = np.random.default_rng(0).normal(size=(V, 3)).astype(np.float32)
    tool.main(["--mesh", mesh_util.write_ply(str(tmp_path / "open.ply"), overts, ofaces), "--defects", out])
    capsys.readouterr()
    back = mesh_util.read_ply(out)
    on_boundary = np.zeros(V, dtype=bool)
    oe = ref.edges(ofaces, V)
    on_boundary[np.unique(oe["key"][oe["n_fwd"] + oe["n_bwd"] == 1])] = True
    assert (back["colors"][on_boundary] == tool.RED).all() and (back["colors"][~on_boundary] == tool.GREY).all() and 0 < on_boundary.sum() < V
