"""SDF volume for mesh extraction (reference utils/mesh_util.py:82-112): the N^3 grid sweep of
`extract_mesh`, a pure consumer of the SDF kernel K2.

`sdf_volume` evaluates `implicit_surface.forward` (no sphere clamp, as :110) on the regular grid over
[-volume_size / 2, volume_size / 2]^3, x slowest / z fastest, returned as [N, N, N] - the array the reference hands to
`skimage.measure.marching_cubes` in convert_sigma_samples_to_ply.  Two deliberate differences:
  * the reference builds grid indices with true division (`(overall_index / N) % N`, inherited from Python-2-era code), which
    shears the y and x coordinates by up to one voxel, and calls `np.int` (removed from numpy 1.24 - the function no longer
    runs); the regular grid is evaluated here; `reference_shear=True` reproduces the sheared coordinates;
  * grid points are generated on the GPU and evaluated in chunks of millions of points (the reference: 16 K).

`extract_mesh` runs natively by default: `sdf_volume` -> `marching_cubes` (csrc/marching_cubes.hip: classify / scan / emit on the device, the
volume never leaves the GPU) -> `write_ply` (numpy only, the layout plyfile writes for the reference's two elements).  The native extractor is
table-based marching cubes on the case table nerfart_amd/mc_table.py generates - not scikit-image's Lewiner variant: the surface is the same, the
triangulation inside ambiguous cells differs ("deviations").  `backend="skimage"` keeps the reference's route through
scikit-image and plyfile, for machines that have them.

Beyond the reference, each off by default, the native route of `extract_mesh` is one sequence of public stage functions (its docstring: the order,
the options, the refusals; DESIGN.md 4.7: the kernels).  Sweep: narrow_band=True makes it `banded_volume` - the SDF is queried only in the bricks
of the grid that can hold the level set, the rest is filled with a value of the right sign, and the result checks and repairs itself
(csrc/mesh_band.hip).  Vertices: refine_evals= / vertex_normals= / color_model= / simplify_factor= / texture_model= keep every vertex as (grid edge, t),
and `refine_vertices` moves t against the SDF without leaving the edge (csrc/mesh_vertices.hip).  simplify_factor=c: `simplify_clusters` merges the
vertices of every block of c^3 grid cells into one, placed by the quadric error metric of the block's faces (csrc/mesh_simplify.hip).  Per-vertex
normals (the SDF gradient) and colours (the radiance net looking down the normal; `vertex_attributes`) become extra PLY vertex properties.
keep_largest= / min_component_faces= drop the floaters: `mesh_components` labels the connected components of the indexed mesh on the GPU
(csrc/mesh_components.hip), `filter_components` keeps the largest ones and compacts vertices and faces.  texture_model= with filepath="*.obj" writes
a textured mesh - OBJ, MTL, PNG (`write_obj`) - instead of the PLY: `bake_texture` gives every face of the final mesh a patch of a per-face atlas
and colours every texel at its own point, `texel_points` says where that is (csrc/mesh_texture.hip).
`rasterize` / `render_mesh` look at the mesh that came out, through a rend_util.get_rays camera (csrc/mesh_raster.hip): exact
integer coverage, a depth test by integer atomics, per-pixel face / barycentrics / depth / normal, then per-vertex colours or the baked texture.
`read_ply` / `read_obj` read back the files `write_ply` / `write_obj` write.  `sample_surface` / `closest_on_mesh` / `mesh_distance` say how far one
mesh is from another - Chamfer, Hausdorff, F-score - from area-weighted samples and exact closest-point queries (csrc/mesh_distance.hip;
tools/compare_mesh.py).  `half_edges` / `mesh_topology` say whether a mesh is a valid surface (csrc/mesh_topology.hip; tools/check_mesh.py), and
`repair_manifold` - extract_mesh(repair=True) - makes it one: non-manifold edges and bow-tie vertices are cut and stitched (csrc/mesh_repair.hip).
None of it is on the render or train path.
"""
import types

import numpy as np
import torch


def grid_points(N: int, volume_size: float, device, start: int = 0, stop: int = None, reference_shear: bool = False):
    """Points start..stop of the flattened N^3 grid [M, 3] (float32 on `device`)."""
    stop = N ** 3 if stop is None else stop
    idx = torch.arange(start, stop, device=device, dtype=torch.int64)
    step = volume_size / (N - 1)
    org = -volume_size / 2.0
    if reference_shear:
        f = idx.double()
        iz, iy, ix = f % N, (f / N) % N, ((f / N) / N) % N
    else:
        iz, iy, ix = (idx % N).double(), ((idx // N) % N).double(), ((idx // (N * N)) % N).double()
    return torch.stack([ix * step + org, iy * step + org, iz * step + org], dim=-1).float()


BAND_LIPSCHITZ = 1.8          # default bound on |grad sdf| of the narrow-band sweep: how it was chosen is in DESIGN.md 4.7


def band_threshold(N: int, volume_size: float, brick: int, lipschitz: float) -> float:
    """The narrow-band test's threshold: lipschitz * reach with reach = sqrt(3) * max(B // 2 + 1, B - B // 2) * step - the largest distance from a
    brick's probe to a point of the brick's box extended by one grid step on every side.  Computed in double, rounded to float32."""
    reach_steps = max(brick // 2 + 1, brick - brick // 2)
    return float(np.float32(float(lipschitz) * (np.sqrt(3.0) * reach_steps * (volume_size / (N - 1)))))


@torch.no_grad()
def banded_volume(query_fn, N: int, volume_size: float, level: float = 0.0, brick: int = 8, lipschitz: float = BAND_LIPSCHITZ,
                  max_repair_rounds: int = 4, chunk: int = 1 << 24, device=None):
    """The [N, N, N] float32 volume of sdf_volume's regular grid with query_fn (pts [M, 3] float32 on the GPU -> values [M] float32) spent only where
    the level set can be (csrc/mesh_band.hip): (vol, info).

    The grid is cut into bricks of brick^3 points (the last of an axis ragged).  Each brick is queried once, at its probe point
    min(b * brick + brick // 2, N - 1); it is ACTIVE iff NOT |f(probe) - level| > band_threshold(...) (float32; a NaN probe is active).  Every owned
    point of every active brick is queried (bricks ascending, inside a brick z fastest, at most `chunk` points per call) and stored; every point of
    an inactive brick gets its brick's probe value.  Then the volume is checked: an edge of the grid whose ends differ in `value < level` and that
    has an end in an inactive brick makes that brick wanted; the wanted bricks are activated and queried and the check runs again, at most
    max_repair_rounds times, after which every remaining brick is activated (the volume is then the dense one).  Host reads: one after the
    probe test, one per check.

    At exit no sign-changing edge has a filled end.  If every filled value also has the true sign - which holds whenever lipschitz bounds
    |grad f| - the volume has the dense sweep's case index in every cell and its values at both ends of every crossing edge, so marching_cubes,
    hip.mc_emit_edges and everything after them give the dense sweep's bits (query_fn must give a point the same value in any batch: K2 does).
    The repair loop is a safety net for a bound that fails along a connected piece of surface, not a proof: a piece of surface that lies wholly
    inside inactive bricks of one sign is NOT found.  A trained field may need a larger lipschitz than the default.

    info: bricks (their number), active (newly active bricks: after the probe test, then per repair round, then of the dense completion if it
    ran), evaluated_points (owned points queried, the `bricks` probe queries not counted), repair_rounds, completed_dense, threshold."""
    from . import hip
    N, B, chunk, max_repair_rounds = int(N), int(brick), int(chunk), int(max_repair_rounds)
    if chunk < 1 or max_repair_rounds < 0:
        raise ValueError(f"banded_volume: chunk must be >= 1 and max_repair_rounds >= 0 (got {chunk}, {max_repair_rounds})")
    if not (float(lipschitz) > 0.0 and np.isfinite(lipschitz)):
        raise ValueError(f"banded_volume: lipschitz must be positive and finite (got {lipschitz})")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    state = hip.BandState(N, B, dev)                                 # refuses N < 2, brick outside 2 .. 64, N^3 >= 2^31
    step, org = volume_size / (N - 1), -volume_size / 2.0           # grid_points' expressions
    thr = band_threshold(N, volume_size, B, lipschitz)
    query = lambda pts: query_fn(pts).reshape(-1)
    ppts = hip.band_probe_points(N, B, step, org, dev)
    probe = torch.cat([query(ppts[s:s + chunk]) for s in range(0, state.bricks, chunk)]).contiguous()
    vol = torch.empty(N, N, N, dtype=torch.float32, device=dev)
    info = {"bricks": state.bricks, "active": [], "evaluated_points": 0, "repair_rounds": 0, "completed_dense": False, "threshold": thr}

    def evaluate(n_list, n_points):
        info["active"].append(n_list)
        info["evaluated_points"] += n_points
        for s in range(0, n_points, chunk):
            pts, idx = hip.band_brick_points(state, n_list, n_points, s, min(chunk, n_points - s), step, org)
            hip.band_scatter(query(pts), idx, vol)

    n_list, n_points = (int(c) for c in hip.band_select(state, 0, probe, level, thr).cpu())
    hip.band_fill(state, probe, vol)
    evaluate(n_list, n_points)
    while True:
        n_list, n_points = (int(c) for c in hip.band_check(state, vol, level).cpu())
        if n_list == 0:
            break
        if info["repair_rounds"] < max_repair_rounds:
            hip.band_select(state, 1)
            info["repair_rounds"] += 1
            evaluate(n_list, n_points)
        else:
            hip.band_select(state, 2)
            info["completed_dense"] = True
            evaluate(state.bricks - sum(info["active"]), N ** 3 - info["evaluated_points"])
            break
    return vol, info


@torch.no_grad()
def sdf_volume(implicit_surface, volume_size: float = 2.0, N: int = 512, chunk: int = 1 << 24, reference_shear: bool = False,
               narrow_band: bool = False, band_brick: int = 8, band_lipschitz: float = BAND_LIPSCHITZ, level: float = 0.0, band_info: dict = None):
    """[N, N, N] float32 (on the GPU): sdf at the grid points (mesh_util.py:82-111).  narrow_band=True (regular grid only): banded_volume with
    implicit_surface.forward around `level` - true values wherever marching cubes reads them, probe values of the right sign elsewhere; a dict
    passed as band_info receives banded_volume's info.  narrow_band=False: the dense sweep, untouched."""
    dev = next(implicit_surface.parameters()).device
    if narrow_band:
        if reference_shear:
            raise ValueError("sdf_volume: narrow_band needs the regular grid (the bound of the band test is stated on its lattice, not on the "
                             "sheared one)")
        vol, info = banded_volume(implicit_surface.forward, N, volume_size, level=level, brick=band_brick, lipschitz=band_lipschitz, chunk=chunk,
                                  device=dev)
        if band_info is not None:
            band_info.update(info)
        return vol
    out = torch.empty(N ** 3, dtype=torch.float32, device=dev)
    for s in range(0, N ** 3, chunk):
        e = min(s + chunk, N ** 3)
        out[s:e] = implicit_surface.forward(grid_points(N, volume_size, dev, s, e, reference_shear))
    return out.reshape(N, N, N)


def marching_cubes(vol, level: float = 0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """Isosurface of vol [nx, ny, nz] (float32, on the GPU) at `level`: (verts [V, 3] float32, faces [F, 3] int32), both on vol's device.
    A grid point (i, j, k) sits at origin + (i, j, k) * spacing; a point is inside iff its value < level, and the triangles are wound so that
    (v1 - v0) x (v2 - v0) points to the outside (outward for a signed distance).  Vertex and face order are defined (points resp. cells in linear
    order), so two calls give identical tensors.  One host read (the two sizes and the non-finite flag) sits between counting and emitting;
    a non-finite value raises ValueError; no crossing gives (0, 3) tensors.  CPU tensors are refused: there is no CPU path."""
    return _count_and_emit(vol, level, origin, spacing)[:2]


def _count_and_emit(vol, level, origin, spacing):
    """marching_cubes keeping what hip.mc_emit_edges and refine_vertices read to give its V vertices as (grid edge, t): (verts, faces, ws, V)."""
    from . import hip                                              # here, not at import: grid_points and write_ply need no library
    ws, counts = hip.mc_count(vol, level)
    V, F, bad = (int(c) for c in counts.cpu())
    if bad:
        raise ValueError("marching_cubes: the volume holds non-finite values")
    verts, faces = hip.mc_emit(vol, level, origin, spacing, ws, V, F)
    return verts, faces, ws, V


def model_frame(N: int, volume_size: float):
    """(origin, spacing) of the grid sdf_volume sweeps - the frame every network query of a mesh vertex is made in."""
    return [-volume_size / 2.0] * 3, [volume_size / (N - 1)] * 3


def grid_to_frame(grid, origin, spacing):
    """Grid coordinates [V, 3] (float32) in the frame (origin, spacing): origin + spacing * grid, one float32 product and one float32 sum per
    coordinate - how extract_mesh(simplify_factor=) places the representatives simplify_clusters returns."""
    o, s = (torch.tensor([float(x) for x in a], dtype=torch.float32, device=grid.device) for a in (origin, spacing))
    return o + s * grid


def placement_frame(N: int, volume_size: float):
    """(origin, spacing) the reference places its mesh with: spacing volume_size / N, offset -volume_size / 2 (mesh_util.py:112)."""
    return [-volume_size / 2.0] * 3, [volume_size / N] * 3


@torch.no_grad()
def refine_vertices(implicit_surface, vol, level, ws, V: int, volume_size: float, n_evals: int):
    """Moves the V marching-cubes vertices of vol [N, N, N] (= sdf_volume(implicit_surface, volume_size, N); ws: the workspace hip.mc_count filled
    for it) along their grid edges toward sdf == level: hip.mc_emit_edges once, then n_evals times hip.mesh_edge_points in the model's frame ->
    implicit_surface.forward (the function the volume was swept with; all V points in one batch, in vertex order) -> hip.mesh_edge_refine_step
    (bracket-keeping false position, Illinois; the rule is in include/nerfart_hip.h).  Returns (edge [V] int32, t_best [V], g_best [V]): the best
    parameter that was actually evaluated and its residual sdf - level.  The first evaluation sits at the interpolated vertex, so n_evals = 1
    reproduces marching_cubes' vertices and measures their residual; no vertex ever leaves its edge."""
    from . import hip
    if n_evals < 1:
        raise ValueError(f"refine_vertices: n_evals must be >= 1 (got {n_evals})")
    edge, bracket, t, best, side = hip.mc_emit_edges(vol, level, ws, V)
    origin, spacing = model_frame(vol.shape[0], volume_size)
    pts = torch.zeros(V, 3, dtype=torch.float32, device=vol.device)
    for _ in range(n_evals if V else 0):
        hip.mesh_edge_points(edge, t, vol.shape, origin, spacing, out=pts)
        f = implicit_surface.forward(pts)
        hip.mesh_edge_refine_step(f, level, bracket, t, best, side)
    return edge, best[:, 0].contiguous(), best[:, 1].contiguous()


def quantize_colors(rgb):
    """[..., 3] float -> uint8: floor(clamp(rgb, 0, 1) * 255 + 0.5), NaN -> 0."""
    return torch.floor(torch.nan_to_num(rgb, nan=0.0).clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)


@torch.no_grad()
def normal_view_radiance(model, pts):
    """(normals [V, 3] float32, rgb [V, 3] float32) of a VolSDF / NeuS model at the points pts [V, 3] (the model's frame), V >= 1: the colour rule
    of vertex_attributes before it is quantised - what the per-vertex colours and the texels of bake_texture share."""
    from . import hip
    view = -hip.normalize_dirs(model.implicit_surface.forward_with_nablas(pts)[1].contiguous())
    rgb, _, nabla = model.forward(pts, view_dirs=view)
    return hip.normalize_dirs(nabla.contiguous()), rgb


@torch.no_grad()
def vertex_attributes(model, pts):
    """(normals [V, 3] float32, colors [V, 3] uint8) of a VolSDF / NeuS model at the points pts [V, 3] (the model's frame).  The normal is
    hip.normalize_dirs(grad sdf) (F.normalize semantics); the colour is the radiance seen looking straight down the normal, view_dirs = -normal -
    the one choice without a free parameter.  Both are read from ONE model.forward(pts, view_dirs); the view direction it is handed needs the
    gradient first, which a query of the SDF net alone supplies (the same kernel on the same points: the same gradient)."""
    if pts.shape[0] == 0:
        return torch.zeros(0, 3, dtype=torch.float32, device=pts.device), torch.zeros(0, 3, dtype=torch.uint8, device=pts.device)
    normals, rgb = normal_view_radiance(model, pts)
    return normals, quantize_colors(rgb)


def mesh_components(faces, n_verts: int):
    """Connected components of the indexed mesh faces [F, 3] (int32, on the GPU) over n_verts vertices (csrc/mesh_components.hip; two vertices
    are connected when a face contains both, so triangles sharing one vertex are one component; a vertex in no face is its own):
    (label [V] int32 - the smallest vertex index of the vertex's component -, roots [C] int32 - the labels in RANK order: face count descending,
    ties broken by the smaller label -, n_faces [C] int32 - the face counts in that order), all on faces' device.  One host read (the flag);
    a face with an index outside [0, n_verts) raises ValueError.  CPU tensors are refused: there is no CPU path."""
    from . import hip
    label, n_faces, info = hip.mesh_components(faces, n_verts)
    if int(info.cpu()[2]):
        raise ValueError(f"mesh_components: a face holds a vertex index outside [0, {int(n_verts)})")
    roots = torch.nonzero(label == torch.arange(int(n_verts), dtype=torch.int32, device=label.device)).reshape(-1)      # ascending
    count, order = torch.sort(n_faces[roots], stable=True, descending=True)           # stable over ascending roots: ties keep the smaller label first
    return label, roots[order].to(torch.int32), count


def filter_components(verts, faces, keep_largest=None, min_faces=None):
    """Drops connected components of the mesh (verts [V, ...], faces [F, 3] int32, on the GPU): a component survives iff
    (keep_largest is None or its rank < keep_largest) and (min_faces is None or its face count >= min_faces), rank as mesh_components orders
    them.  Returns (verts', faces', src_vertex): the surviving vertices and faces in their old order, faces renumbered, and src_vertex [V'] int32
    with verts' = verts[src_vertex] - any other per-vertex array is gathered with it.  Nothing surviving gives (0, ...) tensors."""
    from . import hip
    if keep_largest is None and min_faces is None:
        raise ValueError("filter_components: give keep_largest and / or min_faces")
    if keep_largest is not None and keep_largest < 1:
        raise ValueError(f"filter_components: keep_largest must be >= 1 (got {keep_largest})")
    if min_faces is not None and min_faces < 1:
        raise ValueError(f"filter_components: min_faces must be >= 1 (got {min_faces})")
    V = int(verts.shape[0])
    label, roots, count = mesh_components(faces, V)
    survives = torch.ones_like(roots, dtype=torch.bool)
    if keep_largest is not None:
        survives &= torch.arange(roots.shape[0], device=roots.device) < int(keep_largest)
    if min_faces is not None:
        survives &= count >= int(min_faces)
    keep = torch.zeros(V, dtype=torch.uint8, device=faces.device)
    keep[roots[survives].long()] = 1
    src_vertex, faces_out = hip.mesh_compact(label, keep, faces, V)
    return verts[src_vertex.long()], faces_out, src_vertex


TOPOLOGY_INFO = ("proper_faces", "degenerate_faces", "bad_faces", "referenced_vertices", "edges", "boundary_edges", "flipped_edges",
                 "nonmanifold_edges", "bowtie_vertices", "boundary_loops", "longest_loop", "overflow")      # info [0 .. 11] of nerfart_mesh_half_edges


def _topology_faces(faces, who):
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise ValueError(f"{who}: faces must be a tensor on the GPU (there is no CPU path)")
    if faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces must be {torch.int32} (got {faces.dtype})")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{who}: faces must be [n, 3] (got {tuple(faces.shape)})")
    return faces.contiguous()


def half_edges(faces, V: int, table_log2: int = 0):
    """The half-edge adjacency of the indexed mesh faces [F, 3] (int32, on the GPU) over V vertices (csrc/mesh_topology.hip; the definitions are
    in include/nerfart_hip.h): (twin [3 F] int32 - half-edge 3 f + i runs from faces[f][i] to faces[f][(i + 1) % 3]; the other half-edge of a
    manifold edge, -1 on a boundary edge, -2 on a flipped edge (its two faces run through it the same way), -3 on an edge of more than two
    faces, -4 for a face with an index outside [0, V) or with two equal indices -, edge_uses [3 F] int32 - the faces at the half-edge's edge -,
    vertex_fans [V] int32 - the fans of faces around the vertex: 0 unreferenced, 1 regular, more: a bow-tie -, info [16] int32 - TOPOLOGY_INFO
    names its counts), all on faces' device.  No host read.  table_log2 sizes the edge table (0: the default); the answers do not depend on it."""
    from . import hip
    faces = _topology_faces(faces, "half_edges")
    if int(V) < 0:
        raise ValueError(f"half_edges: V must be >= 0 (got {V})")
    return hip.mesh_half_edges(faces, int(V), int(table_log2))[1:]


def mesh_topology(verts, faces, components: bool = True):
    """Is the mesh (verts [V, 3] float32, faces [F, 3] int32, on the GPU) a valid surface?  A dict of Python numbers and booleans after ONE host
    read: the counts TOPOLOGY_INFO names (faces that are proper / degenerate / bad, referenced vertices, distinct edges, boundary / flipped /
    non-manifold edges, vertices with more than one fan, boundary loops and the longest one's edges), euler = referenced vertices - edges + proper
    faces, closed (no boundary edge), oriented (no flipped edge), manifold (no non-manifold edge, no bow-tie vertex) and watertight = closed and
    oriented and manifold with no bad or degenerate face.  components=True adds "components": one dict per connected component (mesh_components'
    labels and order: most faces first, ties to the smaller label; an unreferenced vertex is a component without faces) with label, vertices,
    edges, faces, boundary_edges, flipped_edges, nonmanifold_edges, bowtie_vertices, euler, closed, area, volume (signed; fp64 sums over the
    component's faces) and genus = (2 - euler) / 2 - only where the component is closed, oriented and manifold, otherwise None; and "tensors":
    label [V] int32, counts [V, 6] int32 and measure [V, 2] float64, both indexed by label, on the device.  Nothing is repaired here: repair_manifold does that."""
    from . import hip
    verts, faces = _distance_mesh(verts, faces, "mesh_topology")
    V = int(verts.shape[0])
    ws, twin, uses, fans, info = hip.mesh_half_edges(faces, V)
    if not components:
        got = info.cpu().tolist()
    else:
        label, n_faces, _ = hip.mesh_components(faces, V)
        counts, measure = hip.mesh_component_stats(verts, faces, label, ws)
        bow = torch.zeros(V, dtype=torch.int32, device=faces.device).index_add_(0, label.long(), (fans > 1).to(torch.int32))
        packed = torch.cat([info, label, bow, n_faces, counts.reshape(-1), measure.reshape(-1).view(torch.int32)]).cpu().numpy()      # the one host read
        got = packed[:16].tolist()
    out = {k: int(x) for k, x in zip(TOPOLOGY_INFO, got)}
    # the flag is known only after the one host read: the stats above have then run on a table that is not valid, which is harmless (every index
    # they take from the workspace is checked against the arrays) - nothing of it is returned
    if out["overflow"]:
        raise RuntimeError("mesh_topology: the edge table overflowed (nerfart_mesh_half_edges info[11]); the counts are not valid")
    out["euler"] = out["referenced_vertices"] - out["edges"] + out["proper_faces"]
    out["closed"] = out["boundary_edges"] == 0
    out["oriented"] = out["flipped_edges"] == 0
    out["manifold"] = out["nonmanifold_edges"] == 0 and out["bowtie_vertices"] == 0
    out["watertight"] = out["closed"] and out["oriented"] and out["manifold"] and out["bad_faces"] == 0 and out["degenerate_faces"] == 0
    if components:
        lab, bw, nf = packed[16:16 + V], packed[16 + V:16 + 2 * V], packed[16 + 2 * V:16 + 3 * V]
        cnt = packed[16 + 3 * V:16 + 9 * V].reshape(V, 6)
        msr = packed[16 + 9 * V:].copy().view(np.float64).reshape(V, 2)
        roots = np.nonzero(lab == np.arange(V, dtype=np.int32))[0]
        roots = roots[np.argsort(-nf[roots].astype(np.int64), kind="stable")]      # mesh_components' ranking: stable over ascending labels
        out["components"] = []
        for r in roots.tolist():
            v, e, f, b, fl, nm = (int(x) for x in cnt[r])
            euler = v - e + f
            ok = b == 0 and fl == 0 and nm == 0 and bw[r] == 0
            out["components"].append({"label": r, "vertices": v, "edges": e, "faces": f, "boundary_edges": b, "flipped_edges": fl,
                                      "nonmanifold_edges": nm, "bowtie_vertices": int(bw[r]), "euler": euler, "closed": b == 0,
                                      "area": float(msr[r, 0]), "volume": float(msr[r, 1]), "genus": (2 - euler) // 2 if ok else None})
        out["tensors"] = {"label": label, "counts": counts, "measure": measure}
    return out


REPAIR_INFO = ("dropped_bad", "dropped_degenerate", "dropped_cancelled", "nonmanifold_edges", "edges_paired", "unpaired_half_edges", "wide_edges",
               "vertices_split", "pairs_subdivided", "sort_ties", "overflow")      # info [0 .. 10] of nerfart_mesh_repair_count
REPAIR_WEDGES = ("void", "solid")


def repair_manifold(verts, faces, wedge: str = "void", table_log2: int = 0):
    """Cut and stitch the non-manifold edges of the mesh (verts [V, 3] float32, faces [F, 3] int32, on the GPU; csrc/mesh_repair.hip, the rules are
    in include/nerfart_hip.h): bad, degenerate and mutually cancelling faces are dropped, the faces around every edge of more than two are paired
    in angular order - wedge="void": the pairs bound the empty wedges, so solids that touch along an edge become one; wedge="solid": they are
    separated -, every vertex is split into one copy per fan of faces, and where two pairs of one edge would still share both ends one of them
    is split at the edge's midpoint.  No other triangle changes.  Returns (verts' [V', 3], faces' [F', 3], src_vertex [V'] int32 - the original
    vertex of every new one, -1 for a midpoint -, mid_ends [M, 2] int32 - the new indices of a midpoint's edge ends, the midpoints being the last
    M vertices: any per-vertex attribute is attr[src_vertex] with the mean of attr'[mid_ends] at the midpoints -, info: a dict of the counts
    REPAIR_INFO names).  With info["wide_edges"] == 0 the output has no non-manifold edge and no bow-tie vertex; with no unpaired half-edge, and
    neither boundary nor flipped edges in the input, it is watertight.  Flipped edges are left as they are.  Small closed pieces that splitting
    sets free are the caller's to drop (filter_components).  Everything stays on the GPU; ONE host read (the sizes and info) between counting
    and emitting; two calls give identical tensors, whatever table_log2 (the edge table's size; 0: the default)."""
    from . import hip
    if wedge not in REPAIR_WEDGES:
        raise ValueError(f"repair_manifold: wedge must be one of {REPAIR_WEDGES} (got {wedge!r})")
    verts, faces = _distance_mesh(verts, faces, "repair_manifold")
    ws, counts, info = hip.mesh_repair_count(verts, faces, wedge, int(table_log2))
    got = torch.cat([counts, info]).cpu().tolist()                              # the one host read
    V1, M, Fa, Fx = got[:4]
    report = {k: int(x) for k, x in zip(REPAIR_INFO, got[4:])}
    if report["overflow"]:
        raise RuntimeError("repair_manifold: a table overflowed (nerfart_mesh_repair_count info[10]); nothing was emitted")
    return hip.mesh_repair_emit(verts, faces, ws, V1, M, Fa + Fx, int(table_log2)) + (report,)


def simplify_clusters(verts_grid, faces, shape, factor, reg: float = 0.01):
    """Vertex clustering with quadric error metrics (csrc/mesh_simplify.hip; the rules are in include/nerfart_hip.h): the vertices verts_grid [V, 3]
    (float32, on the GPU, in GRID coordinates of a grid of shape = (nx, ny, nz): grid point (i, j, k) sits at (i, j, k)) are merged per block of
    factor^3 grid cells; every occupied block becomes one vertex, placed at the minimum of its faces' plane quadrics, pulled toward the members'
    mean by reg and kept inside the block.  Returns (verts' [V', 3] float32 in grid coordinates, faces' [F', 3] int32 - renumbered, rotated to
    smallest index first, degenerate and duplicate faces dropped, in input order -, cluster [V] int32 - the new vertex of every old one).
    Everything stays on the GPU; one host read (V', F', the flag) between counting and emitting; two calls give identical tensors.  ValueError:
    factor < 2, reg not positive, CPU tensors, and a mesh the kernels flag - a face index outside [0, V), a non-finite vertex or one outside the
    grid, or a cluster whose sums would leave their guards (edges longer than a few blocks, more than 2^16 faces in one block)."""
    from . import hip
    if int(factor) != factor or int(factor) < 2:
        raise ValueError(f"simplify_clusters: factor must be an integer >= 2 (got {factor})")
    if not (float(reg) > 0.0 and np.isfinite(reg)):
        raise ValueError(f"simplify_clusters: reg must be positive and finite (got {reg})")
    if not (torch.is_tensor(verts_grid) and torch.is_tensor(faces) and verts_grid.is_cuda and faces.is_cuda):
        raise ValueError("simplify_clusters: verts_grid and faces must be tensors on the GPU (there is no CPU path)")
    ws, cluster, counts = hip.mesh_simplify_count(verts_grid, faces, shape, int(factor))
    V_out, F_out, bad = (int(c) for c in counts.cpu())
    if bad:
        raise ValueError(f"simplify_clusters: the mesh cannot be clustered - a face index outside [0, {int(verts_grid.shape[0])}), a vertex that is not "
                         f"finite or not inside the grid {tuple(int(d) for d in shape)}, or a cluster whose sums would leave their guards")
    out_v, out_f = hip.mesh_simplify_emit(verts_grid, faces, shape, int(factor), float(reg), ws, cluster, V_out, F_out)
    return out_v, out_f, cluster


ATLAS_MAX_SIDE = 16384       # the largest image side of a texture atlas (csrc/mesh_texture.hip MAX_SIDE)
TEXEL_CHUNK = 1 << 20        # texels per network query of texel_points / bake_texture


def atlas_layout(F: int, patch: int):
    """(S, Cw, Ch, W, H) of the per-face texture atlas of F faces at patch size `patch` - the closed form of include/nerfart_hip.h
    (nerfart_mesh_atlas_layout gives the same five numbers): two faces per square cell of side S = patch + 3, Cw x Ch cells, image W x H.
    ValueError: patch < 1, F < 1, an image side above ATLAS_MAX_SIDE."""
    import math
    F, P = int(F), int(patch)
    if P < 1:
        raise ValueError(f"atlas_layout: patch must be >= 1 (got {patch})")
    if F < 1:
        raise ValueError(f"atlas_layout: the mesh has no faces to texture (F = {F})")
    S, cells = P + 3, (F + 1) // 2
    Cw = math.isqrt(cells - 1) + 1                                  # the smallest integer with Cw^2 >= cells
    Ch = (cells + Cw - 1) // Cw
    if Cw * S > ATLAS_MAX_SIDE or Ch * S > ATLAS_MAX_SIDE:
        raise ValueError(f"atlas_layout: F = {F} faces at patch P = {P} need an image of {Cw * S} x {Ch * S} texels, above the limit of "
                         f"{ATLAS_MAX_SIDE} x {ATLAS_MAX_SIDE}: decimate the mesh first (simplify_factor) or use a smaller patch")
    return S, Cw, Ch, Cw * S, Ch * S


def atlas_uvs(F: int, patch: int):
    """[F, 3, 2] float64 numpy: the UV of every face corner in PIXEL units (x to the right, y down from the top row, texel centres at + 0.5).  In
    its cell the lower face 2 q has (0.5, 0.5), (0.5 + P, 0.5), (0.5, 0.5 + P), the upper face 2 q + 1 has S minus those; the cell's origin is
    ((q % Cw) S, (q // Cw) S).  Closed form: no kernel."""
    S, Cw, _, _, _ = atlas_layout(F, patch)
    P = int(patch)
    f = np.arange(int(F))
    q = f // 2
    origin = np.stack([(q % Cw) * S, (q // Cw) * S], axis=-1).astype(np.float64)[:, None, :]
    lower = np.array([[0.5, 0.5], [0.5 + P, 0.5], [0.5, 0.5 + P]], dtype=np.float64)
    local = np.where((f % 2 == 0)[:, None, None], lower[None], S - lower[None])
    return origin + local


@torch.no_grad()
def texel_points(verts, faces, patch: int, query_fn=None, project: int = 0, level: float = 0.0, max_step: float = None):
    """Where every texel of the atlas of the mesh (verts [V, 3] float32, faces [F, 3] int32, on the GPU) sits in space (csrc/mesh_texture.hip; the
    rules are in include/nerfart_hip.h): (points [H * W, 3] float32, face_of [H, W] int32), on the GPU, rows in texel order y W + x.  face_of is
    the owning face, -1 for a texel no face owns (its point is 0).  A texel outside its triangle - the gutter bilinear filtering reads - is a
    point of the face's plane at extrapolated barycentrics.

    project = k > 0 moves every valid texel k Newton steps toward sdf == level, each at most max_step long: query_fn(pts [M, 3]) ->
    (sdf [M], nabla [M, 3], ...) is asked in chunks of at most TEXEL_CHUNK points (hip.mesh_project_step).  A face of a decimated mesh is a
    chord of the true surface; this puts its texels back where the radiance net was trained.  One host read (the flag).
    ValueError: a face index outside [0, V), patch < 1, no faces, an atlas above the size limit, project < 0, project > 0 without query_fn or
    a positive max_step.  CPU tensors are refused: there is no CPU path."""
    from . import hip
    project = int(project)
    if project < 0:
        raise ValueError(f"texel_points: project must be >= 0 (got {project})")
    if project > 0 and (query_fn is None or max_step is None or not float(max_step) > 0.0):
        raise ValueError(f"texel_points: project = {project} needs query_fn and a positive max_step (got query_fn = {query_fn}, max_step = {max_step})")
    if not (torch.is_tensor(faces) and faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError("texel_points: faces must be a tensor [F, 3]")
    atlas_layout(int(faces.shape[0]), patch)                        # ValueError before anything is allocated
    points, face_of, info = hip.mesh_atlas_points(verts, faces, int(patch))
    if int(info.cpu()[0]):
        raise ValueError(f"texel_points: a face holds a vertex index outside [0, {int(verts.shape[0])})")
    if project > 0:
        valid = torch.nonzero(face_of.reshape(-1) >= 0).reshape(-1)
        pts = points[valid]
        for _ in range(project):
            for s in range(0, pts.shape[0], TEXEL_CHUNK):
                part = pts[s:s + TEXEL_CHUNK]                       # a view: the step is taken in place
                out = query_fn(part)
                hip.mesh_project_step(part, out[0].reshape(-1).contiguous(), out[1].reshape(-1, 3).contiguous(), level, max_step)
        points[valid] = pts
    return points, face_of


@torch.no_grad()
def bake_texture(verts, faces, color_fn, patch: int = 4, query_fn=None, project: int = 0, level: float = 0.0, max_step: float = None):
    """The texture of the mesh (verts [V, 3], faces [F, 3] int32, on the GPU): (image [H, W, 3] uint8 on the GPU, uv [F, 3, 2] float64 numpy in pixel
    units = atlas_uvs(F, patch)).  Every valid texel is quantize_colors(color_fn(its point)) - color_fn(pts [M, 3]) -> rgb [M, 3] is asked in
    chunks of at most TEXEL_CHUNK points, at texel_points(verts, faces, patch, query_fn, project, level, max_step) -, every other texel is 0.
    Bilinear sampling at a face's UVs reads that face's texels only, and reproduces a colour that is affine over the face exactly (up to the
    quantisation): no dilation pass is needed.  Mip-mapping would mix neighbouring cells."""
    points, face_of = texel_points(verts, faces, patch, query_fn=query_fn, project=project, level=level, max_step=max_step)
    H, W = face_of.shape
    valid = torch.nonzero(face_of.reshape(-1) >= 0).reshape(-1)
    pts = points[valid]
    image = torch.zeros(H * W, 3, dtype=torch.uint8, device=points.device)
    image[valid] = torch.cat([quantize_colors(color_fn(pts[s:s + TEXEL_CHUNK]).reshape(-1, 3)) for s in range(0, pts.shape[0], TEXEL_CHUNK)])
    return image.reshape(H, W, 3), atlas_uvs(int(faces.shape[0]), patch)


def write_obj(path, verts, faces, uv, image, normals=None):
    """Wavefront OBJ with a material and a texture: writes <stem>.obj, <stem>.mtl and <stem>.png next to each other (path must end in .obj) and
    returns path.  verts [V, 3], faces [F, 3], normals [V, 3] or None: tensors or arrays; uv [F, 3, 2] in PIXEL units of image [H, W, 3] uint8
    (atlas_uvs: y down from the top row).  The OBJ holds `mtllib`, `usemtl`, V `v` lines, 3 F `vt` lines (u = X / W, v = 1 - Y / H: OBJ's v
    runs up from the bottom row), V `vn` lines if normals are given, and F faces `f v/vt` or `f v/vt/vn`, all indices 1-based; the MTL
    `newmtl` and `map_Kd <stem>.png`; the PNG is written with PIL.  Floats are printed with %.9g: enough digits to give every fp32 back."""
    import os
    from PIL import Image
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    path = str(path)
    if not path.endswith(".obj"):
        raise ValueError(f"write_obj: the path must end in .obj (got {path!r})")
    v = host(verts).reshape(-1, 3)
    f = host(faces).reshape(-1, 3).astype(np.int64)
    img = np.ascontiguousarray(host(image))
    uv = np.asarray(host(uv), dtype=np.float64)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"write_obj: image must be uint8 [H, W, 3] (got {img.dtype} {img.shape})")
    if uv.shape != (len(f), 3, 2):
        raise ValueError(f"write_obj: uv must be [{len(f)}, 3, 2] (got {uv.shape})")
    n = None if normals is None else host(normals)
    if n is not None and n.shape != (len(v), 3):
        raise ValueError(f"write_obj: normals must be [{len(v)}, 3] (got {n.shape})")
    H, W = img.shape[:2]
    stem = path[:-len(".obj")]
    name = os.path.basename(stem)
    lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += ["v %.9g %.9g %.9g" % tuple(float(c) for c in p) for p in v]
    lines += ["vt %.9g %.9g" % (x / W, 1.0 - y / H) for x, y in uv.reshape(-1, 2)]
    if n is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(float(c) for c in p) for p in n]
        lines += ["f " + " ".join(f"{int(a) + 1}/{3 * k + c + 1}/{int(a) + 1}" for c, a in enumerate(tri)) for k, tri in enumerate(f)]
    else:
        lines += ["f " + " ".join(f"{int(a) + 1}/{3 * k + c + 1}" for c, a in enumerate(tri)) for k, tri in enumerate(f)]
    with open(path, "w") as out:
        out.write("\n".join(lines) + "\n")
    with open(stem + ".mtl", "w") as out:
        out.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    Image.fromarray(img).save(stem + ".png")
    return path


def write_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY: `element vertex` with float x, y, z and `element face` with `property list uchar int vertex_indices` - the file
    plyfile writes for the reference's two elements (mesh_util.py:57-80).  verts [V, 3], faces [F, 3]: tensors or arrays.  Optional per-vertex
    properties, after x y z in this order: normals [V, 3] as float nx ny nz, colors [V, 3] uint8 as uchar red green blue (the names MeshLab,
    Open3D and Blender read); with both None the file is the two-element file byte for byte."""
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    v = np.ascontiguousarray(host(verts), dtype="<f4").reshape(-1, 3)
    f = host(faces).reshape(-1, 3)
    rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"], rec["i"] = 3, f
    props, fields = "property float x\nproperty float y\nproperty float z\n", [("p", "<f4", (3,))]
    if normals is not None:
        props += "property float nx\nproperty float ny\nproperty float nz\n"
        fields.append(("n", "<f4", (3,)))
    if colors is not None:
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        fields.append(("c", "u1", (3,)))
    if len(fields) > 1:
        vrec = np.empty(len(v), dtype=fields)                            # packed: no padding between the fields
        vrec["p"] = v
        for key, a in (("n", normals), ("c", colors)):
            if a is not None:
                a = host(a)
                if a.shape != (len(v), 3) or (key == "c" and a.dtype != np.uint8):
                    raise ValueError(f"write_ply: {'colors must be uint8' if key == 'c' else 'normals must be'} [{len(v)}, 3] "
                                     f"(got {a.dtype} {a.shape})")
                vrec[key] = a
        v = vrec
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\n{props}"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(rec.tobytes())
    return path


def read_ply(path):
    """Reads back exactly the files write_ply writes, and nothing more general: dict of verts [V, 3] float32, faces [F, 3] int32, normals [V, 3]
    float32 or None, colors [V, 3] uint8 or None (numpy).  ValueError for any other header."""
    with open(path, "rb") as src:
        data = src.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"read_ply: {path!r} has no PLY header")
    lines = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    xyz, nrm, rgb = ["property float x", "property float y", "property float z"], ["property float nx", "property float ny", "property float nz"], \
        ["property uchar red", "property uchar green", "property uchar blue"]
    if lines[:2] != ["ply", "format binary_little_endian 1.0"] or len(lines) < 8 or not lines[2].startswith("element vertex "):
        raise ValueError(f"read_ply: {path!r} is not a file write_ply wrote")
    props = lines[3:-3]
    fields = [("p", "<f4", (3,))]
    rest = props[3:]
    if props[:3] != xyz:
        raise ValueError(f"read_ply: {path!r} is not a file write_ply wrote (vertex properties {props})")
    if rest[:3] == nrm:
        fields.append(("n", "<f4", (3,)))
        rest = rest[3:]
    if rest[:3] == rgb:
        fields.append(("c", "u1", (3,)))
        rest = rest[3:]
    if rest or not lines[-3].startswith("element face ") or lines[-2] != "property list uchar int vertex_indices" or lines[-1] != "":
        raise ValueError(f"read_ply: {path!r} is not a file write_ply wrote (header {lines})")
    V, F = int(lines[2].split()[2]), int(lines[-3].split()[2])
    vdt, fdt = np.dtype(fields), np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    if len(body) != V * vdt.itemsize + F * fdt.itemsize:
        raise ValueError(f"read_ply: {path!r} holds {len(body)} bytes of data, its header asks for {V * vdt.itemsize + F * fdt.itemsize}")
    v = np.frombuffer(body, dtype=vdt, count=V)
    f = np.frombuffer(body, dtype=fdt, count=F, offset=V * vdt.itemsize)
    if F and not np.all(f["n"] == 3):
        raise ValueError(f"read_ply: {path!r} holds a face that is not a triangle")
    names = vdt.names
    return {"verts": np.array(v["p"], dtype=np.float32), "faces": np.array(f["i"], dtype=np.int32),
            "normals": np.array(v["n"], dtype=np.float32) if "n" in names else None, "colors": np.array(v["c"], dtype=np.uint8) if "c" in names else None}


UV_SNAP = 1024               # read_obj rounds pixel UVs to 1 / UV_SNAP of a texel


def read_obj(path):
    """Reads back exactly the files write_obj writes, and nothing more general: dict of verts [V, 3] float32, faces [F, 3] int32, uv [F, 3, 2]
    float64 in PIXEL units of image (the v flip undone: X = u W, Y = (1 - v) H), image [H, W, 3] uint8 (the MTL's map_Kd, next to the OBJ, read
    with PIL), normals [V, 3] float32 or None (numpy).  %.9g gives every fp32 of v and vn back; u and v were printed with nine digits too, which
    leaves X and Y off by up to 16384 * 5e-10 texels, so they are rounded to the nearest 1 / UV_SNAP of a texel: atlas_uvs (multiples of 1 / 2)
    come back exactly.  ValueError for any other line."""
    import os
    from PIL import Image
    path = str(path)
    v, vt, vn, f, mtllib = [], [], [], [], None
    for line in open(path):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "mtllib":
            mtllib = tok[1]
        elif tok[0] == "usemtl":
            pass
        elif tok[0] in ("v", "vt", "vn"):
            {"v": v, "vt": vt, "vn": vn}[tok[0]].append([float(t) for t in tok[1:]])
        elif tok[0] == "f" and len(tok) == 4:
            f.append([[int(i) for i in t.split("/")] for t in tok[1:]])
        else:
            raise ValueError(f"read_obj: unexpected line {line!r}")
    if mtllib is None:
        raise ValueError(f"read_obj: {path!r} names no material library")
    folder = os.path.dirname(path)
    png = None
    for line in open(os.path.join(folder, mtllib)):
        tok = line.split()
        if tok and tok[0] == "map_Kd":
            png = tok[1]
    if png is None:
        raise ValueError(f"read_obj: {mtllib!r} names no texture (map_Kd)")
    image = np.array(Image.open(os.path.join(folder, png)).convert("RGB"), dtype=np.uint8)
    H, W = image.shape[:2]
    f = np.array(f, dtype=np.int64).reshape(len(f), 3, -1)
    F = len(f)
    vt = np.array(vt, dtype=np.float64).reshape(-1, 2)
    if f.shape[2] not in (2, 3) or len(vt) != 3 * F or not np.array_equal(f[..., 1], np.arange(3 * F).reshape(F, 3) + 1) or \
            (f.shape[2] == 3 and not np.array_equal(f[..., 2], f[..., 0])):
        raise ValueError(f"read_obj: {path!r} is not a file write_obj wrote (one vt per face corner, in order; vn indexed as v)")
    pix = np.stack([vt[:, 0] * W, (1.0 - vt[:, 1]) * H], axis=-1)
    uv = (np.round(pix * UV_SNAP) / UV_SNAP).reshape(F, 3, 2)
    return {"verts": np.array(v, dtype=np.float64).reshape(-1, 3).astype(np.float32), "faces": (f[..., 0] - 1).astype(np.int32), "uv": uv, "image": image,
            "normals": np.array(vn, dtype=np.float64).reshape(-1, 3).astype(np.float32) if vn else None}


RASTER_MAX_SIDE = 16384      # the largest image side of the rasteriser (csrc/mesh_raster.hip MAX_SIDE)


def _gpu_mesh(verts, faces, who):
    if not (torch.is_tensor(verts) and torch.is_tensor(faces) and verts.is_cuda and faces.is_cuda):
        raise ValueError(f"{who}: verts and faces must be tensors on the GPU (there is no CPU path)")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{who}: verts must be [V, 3] and faces [F, 3] (got {tuple(verts.shape)}, {tuple(faces.shape)})")


@torch.no_grad()
def rasterize(verts, faces, c2w, intrinsics, H: int, W: int, near: float = 1e-3):
    """The mesh (verts [V, 3] float32, faces [F, 3] int32, on the GPU) seen by the camera (c2w [4, 4], intrinsics [4, 4]: rend_util.get_rays'
    conventions - pixel (column i, row j) sampled at its integer coordinates, ray index j W + i) - csrc/mesh_raster.hip, the rules are in
    include/nerfart_hip.h.  dict, every array over the H W pixels: face_id int32 (-1: nothing hit), bary [., 3], depth (distance along the unit
    ray: the units of render_fn's depth_volume and surface_render's depths), z (camera z), mask uint8, face_normals [., 3] (world space,
    geometric, turned toward the camera); n_skipped (int: faces dropped whole because a vertex is behind `near` or projects beyond 2^15 pixels -
    there is no polygon clipping) and n_rejected (int: covered samples whose plane depth is not >= near).  Coverage is exact (integer edge
    functions on positions snapped to 1/256 pixel, top-left rule): faces sharing an edge neither overlap nor leave a gap, and the image does not
    depend on the order of the faces or of the work.  One host read (the counts and the flag); a face index outside [0, V) raises ValueError."""
    from . import hip
    _gpu_mesh(verts, faces, "rasterize")
    H, W = int(H), int(W)
    if not (1 <= H <= RASTER_MAX_SIDE and 1 <= W <= RASTER_MAX_SIDE):
        raise ValueError(f"rasterize: H and W must be in 1 .. {RASTER_MAX_SIDE} (got {H}, {W})")
    if not (float(near) > 0.0 and np.isfinite(near)):
        raise ValueError(f"rasterize: near must be positive and finite (got {near})")
    camera = hip.mesh_camera(c2w, intrinsics)
    xy_fix, cam, valid = hip.mesh_project(verts, camera, near)
    zbuf, info = hip.mesh_raster(xy_fix, cam, valid, faces, camera, near, H, W)
    out = hip.mesh_resolve(zbuf, cam, faces, camera, H, W)
    bad, n_skipped, n_rejected, _ = (int(c) for c in info.cpu())
    if bad:
        raise ValueError(f"rasterize: a face holds a vertex index outside [0, {int(verts.shape[0])})")
    out["n_skipped"], out["n_rejected"] = n_skipped, n_rejected
    return out


@torch.no_grad()
def render_mesh(verts, faces, c2w, intrinsics, H: int, W: int, colors=None, uv=None, image=None, normals=None, background=(0, 0, 0), near: float = 1e-3):
    """A frame of the mesh, in render_fn's triple shape: (rgb [H W, 3] float32, depth [H W] float32, extras).  rasterize(...) decides what every
    pixel sees; then the pixel is shaded from exactly one of: colors [V, 3] per vertex (uint8 levels, taken / 255, or float) interpolated over
    the face; uv [F, 3, 2] (pixel units, atlas_uvs' convention) with image [Ht, Wt, 3] uint8 - what bake_texture returns and read_obj reads -,
    the interpolated uv sampled bilinearly; neither: the face normal as a colour, (n + 1) / 2.  A pixel that sees nothing gets `background` and
    depth 0.  extras: mask_mesh [H W] bool, normals_mesh [H W, 3] (normals [V, 3] interpolated and renormalised when given, otherwise the face
    normal; 0 on a miss), face_id, bary, n_skipped."""
    from . import hip
    if (uv is None) != (image is None):
        raise ValueError("render_mesh: uv and image go together")
    if colors is not None and uv is not None:
        raise ValueError("render_mesh: give colors or uv + image, not both")
    r = rasterize(verts, faces, c2w, intrinsics, H, W, near)
    dev = verts.device
    bg = [float(b) for b in background]
    face_id, bary, mask = r["face_id"], r["bary"], r["mask"]
    if normals is not None:
        n_mesh = hip.normalize_dirs(hip.mesh_interp(face_id, bary, torch.as_tensor(normals, device=dev).float().contiguous(), faces))
    else:
        n_mesh = r["face_normals"]
    if uv is not None:
        uv_t = torch.as_tensor(np.asarray(uv, dtype=np.float32) if not torch.is_tensor(uv) else uv, device=dev).float().contiguous()
        img = torch.as_tensor(image, device=dev).contiguous()
        if tuple(uv_t.shape) != (int(faces.shape[0]), 3, 2) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError(f"render_mesh: uv must be [{int(faces.shape[0])}, 3, 2] and image uint8 [Ht, Wt, 3] (got {tuple(uv_t.shape)}, {img.dtype} "
                             f"{tuple(img.shape)})")
        rgb = hip.mesh_sample_bilinear(hip.mesh_interp(face_id, bary, uv_t), img, mask, bg)
    else:
        if colors is not None:
            col = torch.as_tensor(colors, device=dev)
            col = (col.float() / 255.0 if col.dtype == torch.uint8 else col.float()).contiguous()
            if tuple(col.shape) != (int(verts.shape[0]), 3):
                raise ValueError(f"render_mesh: colors must be [{int(verts.shape[0])}, 3] (got {tuple(col.shape)})")
            rgb = hip.mesh_interp(face_id, bary, col, faces)
        else:
            rgb = 0.5 * n_mesh + 0.5
        hit = mask.bool()[:, None]
        rgb = torch.where(hit, rgb, torch.tensor(bg, dtype=torch.float32, device=dev))
    extras = {"mask_mesh": mask.bool(), "normals_mesh": n_mesh, "face_id": face_id, "bary": bary, "n_skipped": r["n_skipped"]}
    return rgb, r["depth"], extras


DISTANCE_GRID_MAX = 256      # cells per axis of closest_on_mesh's default grid (256^3 = the 2^24 cells csrc/mesh_distance.hip accepts)


def _distance_mesh(verts, faces, who, names=("verts", "faces")):
    """The refusals the distance functions share, by name: tensors on the GPU, [V, 3] float32 and [F, 3] int32, contiguous."""
    for t, name, dtype in ((verts, names[0], torch.float32), (faces, names[1], torch.int32)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{who}: {name} must be a tensor on the GPU (there is no CPU path)")
        if t.dtype != dtype:
            raise ValueError(f"{who}: {name} must be {dtype} (got {t.dtype})")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} must be [n, 3] (got {tuple(t.shape)})")
    if verts.device != faces.device:
        raise ValueError(f"{who}: {names[0]} and {names[1]} must be on the same device (got {verts.device}, {faces.device})")
    return verts.contiguous(), faces.contiguous()


def default_distance_grid(F: int):
    """The grid closest_on_mesh builds when none is given: g = ceil(sqrt(F / 8)) cells per axis, at most DISTANCE_GRID_MAX - a surface of F faces
    occupies a few g^2 of the g^3 cells, which leaves a handful of faces per occupied cell.  A heuristic for speed only: the answer does not
    depend on the grid."""
    g = int(min(max(int(np.ceil(np.sqrt(max(int(F), 1) / 8.0))), 1), DISTANCE_GRID_MAX))
    return (g, g, g)


@torch.no_grad()
def sample_surface(verts, faces, n=None, density=None, seed: int = 0):
    """Area-weighted random points on the mesh (verts [V, 3] float32, faces [F, 3] int32, on the GPU): (points [N, 3] float32, face [N] int32), face
    by face (csrc/mesh_distance.hip; the rules are in include/nerfart_hip.h).  Give the density (samples per unit area) or n, which makes the
    density n / total area (the areas summed by torch in float64): N is then n in expectation, not exactly - every face f draws
    floor(density area_f + h(seed, f)) samples, independently of every other face, so that a set of samples is a pure function of (mesh, density,
    seed).  A face with an index outside [0, V) or a non-finite vertex gets no samples.  One host read (N)."""
    from . import hip
    verts, faces = _distance_mesh(verts, faces, "sample_surface")
    if (n is None) == (density is None):
        raise ValueError("sample_surface: give n or density, not both")
    if density is None:
        if int(n) < 0:
            raise ValueError(f"sample_surface: n must be >= 0 (got {n})")
        V = int(verts.shape[0])
        idx = faces.long()
        ok = ((idx >= 0) & (idx < V)).all(1)
        tri = verts.double()[idx[ok]] if V else verts.new_zeros((0, 3, 3), dtype=torch.float64)
        tri = tri[torch.isfinite(tri).reshape(-1, 9).all(1)]
        area = 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1).sum()
        area = float(area)
        density = float(n) / area if area > 0.0 else 0.0
    if not (np.isfinite(density) and density >= 0.0):
        raise ValueError(f"sample_surface: the density must be finite and >= 0 (got {density})")
    ws, info = hip.mesh_sample_count(verts, faces, density, seed)
    N, _, overflow, _ = (int(c) for c in info.cpu())
    if overflow:
        raise ValueError(f"sample_surface: density {density} asks for 2^31 samples or more")
    return hip.mesh_sample_emit(verts, faces, seed, ws, N)


@torch.no_grad()
def closest_on_mesh(points, verts, faces, max_distance: float = float("inf"), grid=None):
    """For every point [n, 3] (float32, on the GPU) the distance to the mesh and the face that attains it: (dist [n] float32, face [n] int32) -
    the exact minimum over all faces, computed in float64 and rounded once; ties go to the lowest face index (csrc/mesh_distance.hip).  A point
    farther than max_distance reports (max_distance, -1), and so does every point when the mesh has no usable face.  grid = (gx, gy, gz) sets the
    broad phase's uniform grid (default: default_distance_grid); the answer does not depend on it.  One host read (the grid's entries)."""
    from . import hip
    verts, faces = _distance_mesh(verts, faces, "closest_on_mesh")
    if not torch.is_tensor(points) or not points.is_cuda:
        raise ValueError("closest_on_mesh: points must be a tensor on the GPU (there is no CPU path)")
    if points.dtype != torch.float32:
        raise ValueError(f"closest_on_mesh: points must be torch.float32 (got {points.dtype})")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"closest_on_mesh: points must be [n, 3] (got {tuple(points.shape)})")
    if not float(max_distance) >= 0.0:
        raise ValueError(f"closest_on_mesh: max_distance must be >= 0 (got {max_distance})")
    g = hip.mesh_grid_build(verts, faces, default_distance_grid(int(faces.shape[0])) if grid is None else grid)
    return hip.mesh_closest(points.contiguous(), verts, faces, g, max_distance)


def _direction_stats(d, threshold):
    d = d.double()
    if d.numel() == 0:
        return {"n": 0, "mean": 0.0, "rms": 0.0, "max": 0.0, "within": None if threshold is None else 0.0}
    return {"n": int(d.numel()), "mean": float(d.mean()), "rms": float((d * d).mean().sqrt()), "max": float(d.max()),
            "within": None if threshold is None else int((d <= float(threshold)).sum()) / int(d.numel())}      # an integer count: exactly 1 when all are


def distance_summary(d_ab, d_ba, threshold=None):
    """The dict mesh_distance returns, from the per-sample distances of the two directions (tensors; reduced by torch in float64)."""
    ab, ba = _direction_stats(d_ab, threshold), _direction_stats(d_ba, threshold)
    out = {"a_to_b": ab, "b_to_a": ba, "chamfer": 0.5 * (ab["mean"] + ba["mean"]), "hausdorff": max(ab["max"], ba["max"]),
           "threshold": None if threshold is None else float(threshold), "precision": ab["within"], "recall": ba["within"], "fscore": None}
    if threshold is not None:
        s = ab["within"] + ba["within"]
        out["fscore"] = 2.0 * ab["within"] * ba["within"] / s if s > 0.0 else 0.0
    return out


@torch.no_grad()
def mesh_distance(verts_a, faces_a, verts_b, faces_b, samples: int = 1 << 20, threshold=None, max_distance: float = float("inf"), seed: int = 0):
    """How far surface A is from surface B: about `samples` area-weighted points of each (sample_surface, the same seed) and their exact distances
    to the other mesh (closest_on_mesh).  dict:
      a_to_b, b_to_a   per direction n (samples drawn), mean, rms, max (the one-sided Hausdorff distance) and within (the share of samples with
                       distance <= threshold; None without a threshold);
      chamfer          the mean of the two means;      hausdorff   the larger of the two maxima;
      precision        a_to_b's within (A as the prediction, B as the truth), recall = b_to_a's, fscore = their harmonic mean.
    A sample farther than max_distance counts as max_distance.  The reductions are torch's, in float64."""
    verts_a, faces_a = _distance_mesh(verts_a, faces_a, "mesh_distance", ("verts_a", "faces_a"))
    verts_b, faces_b = _distance_mesh(verts_b, faces_b, "mesh_distance", ("verts_b", "faces_b"))
    if int(samples) < 1:
        raise ValueError(f"mesh_distance: samples must be >= 1 (got {samples})")
    if threshold is not None and not float(threshold) >= 0.0:
        raise ValueError(f"mesh_distance: threshold must be >= 0 (got {threshold})")
    pa, _ = sample_surface(verts_a, faces_a, n=samples, seed=seed)
    pb, _ = sample_surface(verts_b, faces_b, n=samples, seed=seed)
    d_ab, _ = closest_on_mesh(pa, verts_b, faces_b, max_distance)
    d_ba, _ = closest_on_mesh(pb, verts_a, faces_a, max_distance)
    return distance_summary(d_ab, d_ba, threshold)


def _check_extract_options(o):
    """Every refusal of extract_mesh for its arguments o (+ o.edges: stage 3 is wanted); the first rule broken names the ValueError: the order is behaviour."""
    if o.texture_model is not None:
        if not str(o.filepath).endswith(".obj"):
            raise ValueError(f"extract_mesh: texture_model writes OBJ + MTL + PNG: filepath must end in .obj (got {o.filepath!r})")
        if o.color_model is not None:
            raise ValueError("extract_mesh: texture_model and color_model exclude each other (OBJ has no standard vertex colours)")
        if o.reference_shear:
            raise ValueError("extract_mesh: texture_model needs the regular grid (reference_shear=True samples a sheared lattice, which has no "
                             "regular frame to query the model in)")
        if o.backend == "skimage":
            raise ValueError("extract_mesh: texture_model needs backend='native' (the atlas is baked on the GPU, on the native extractor's mesh)")
        if int(o.texture_patch) < 1 or int(o.texture_project) < 0:
            raise ValueError(f"extract_mesh: texture_patch must be >= 1 and texture_project >= 0 (got {o.texture_patch}, {o.texture_project})")
    if o.simplify_factor is not None and o.reference_shear:
        raise ValueError("extract_mesh: simplify_factor needs the regular grid (reference_shear=True samples a sheared lattice, whose cells are not "
                         "the blocks the clusters are made of)")
    if o.simplify_factor is not None and o.backend == "skimage":
        raise ValueError("extract_mesh: simplify_factor needs backend='native' (the clustering runs on the GPU, on the native extractor's vertices)")
    if o.narrow_band and o.reference_shear:
        raise ValueError("extract_mesh: narrow_band needs the regular grid (reference_shear=True samples a sheared lattice, on which the bound of "
                         "the band test is not stated)")
    if o.narrow_band and o.backend == "skimage":
        raise ValueError("extract_mesh: narrow_band needs backend='native' (scikit-image's Lewiner variant reads corner values that would be fill values)")
    if (o.keep_largest is not None or o.min_component_faces is not None) and o.backend != "native":
        raise ValueError("extract_mesh: keep_largest / min_component_faces need backend='native' (the components are found on the GPU)")
    if o.edges and (o.reference_shear or o.backend != "native"):
        raise ValueError("extract_mesh: refine_evals / vertex_normals / color_model need backend='native' and the regular grid "
                         "(the sheared grid has no regular frame, scikit-image gives no edge table)")
    if o.backend not in ("native", "skimage"):
        raise ValueError(f"extract_mesh: backend must be 'native' or 'skimage' (got {o.backend!r})")
    if int(o.refine_evals) < 0:
        raise ValueError(f"extract_mesh: refine_evals must be >= 0 (got {int(o.refine_evals)})")
    if o.repair_wedge not in REPAIR_WEDGES:
        raise ValueError(f"extract_mesh: repair_wedge must be one of {REPAIR_WEDGES} (got {o.repair_wedge!r})")
    if o.repair and o.backend != "native":
        raise ValueError("extract_mesh: repair needs backend='native' (the mesh is repaired on the GPU)")


def _extract_skimage(implicit_surface, volume_size, level, N, filepath, chunk, reference_shear):
    """The reference's route: the volume on the host, scikit-image's marching cubes, plyfile's two elements."""
    try:
        from skimage import measure
        import plyfile
    except ImportError as e:                                        # pragma: no cover - third-party, absent in this image
        raise ImportError("extract_mesh needs scikit-image (marching cubes) and plyfile; sdf_volume() returns the SDF grid without them") from e
    vol = sdf_volume(implicit_surface, volume_size, N, chunk, reference_shear=reference_shear).cpu().numpy()
    spacing = volume_size / N                                        # the reference passes volume_size / N (not / (N - 1)), mesh_util.py:112
    verts, faces, _, _ = measure.marching_cubes(vol, level=level, spacing=[spacing] * 3)
    verts = verts + np.array([-volume_size / 2.0] * 3)
    v = np.array([tuple(p) for p in verts], dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    f = np.array([(list(t),) for t in faces], dtype=[("vertex_indices", "i4", (3,))])
    plyfile.PlyData([plyfile.PlyElement.describe(v, "vertex"), plyfile.PlyElement.describe(f, "face")]).write(filepath)
    return filepath


class _Mesh:
    """The mesh between the stages of the native pipeline: verts [V, 3] in the placement frame - what is written -, faces [F, 3] int32, optional
    normals and colors [V, 3], and place(origin, spacing) -> the vertices [V0, 3] in any other frame, from their edge records or their grid
    coordinates (None on the plain path, which keeps neither); src: the rows of place's result that stage 6 left (None: all of them)."""
    def __init__(self, verts, faces, place=None):
        self.verts, self.faces, self.place, self.normals, self.colors, self.src = verts, faces, place, None, None, None

    def points(self, origin, spacing):
        pts = self.place(origin, spacing)
        return pts if self.src is None else pts[self.src.long()]


def _normals_and_colors(implicit_surface, color_model, pts):
    """(normals, colors) at the model-frame pts [V, 3]: vertex_attributes, or with no color_model the normalised SDF gradient and None; V = 0: no query."""
    from . import hip
    if pts.shape[0] == 0:
        return pts, (None if color_model is None else torch.zeros(0, 3, dtype=torch.uint8, device=pts.device))
    if color_model is not None:
        return vertex_attributes(color_model, pts)
    return hip.normalize_dirs(implicit_surface.forward_with_nablas(pts)[1].contiguous()), None


def _repaired_rows(rows, src_vertex, mid_ends):
    """A per-vertex array [V, k] carried through repair_manifold: rows[src_vertex], and at the midpoints - the last M rows, src_vertex -1 -
    the mean of the two ends' rows."""
    M = int(mid_ends.shape[0])
    out = rows[src_vertex.clamp(min=0).long()]
    if M:
        out[out.shape[0] - M:] = (out[mid_ends[:, 0].long()] + out[mid_ends[:, 1].long()]) * 0.5
    return out


def _repair_stage(mesh, o):
    """Stage 4b on a mesh no vertex of which has been queried yet: repair_manifold in the placement frame; the vertices in any other frame are
    the old ones' copies, the midpoints the means of their ends there."""
    verts, faces, src, ends, info = repair_manifold(mesh.verts, mesh.faces, o.repair_wedge)
    if o.repair_info is not None:
        o.repair_info.update(info)
    old = mesh
    return _Mesh(verts, faces, None if old.place is None else (lambda origin, spacing: _repaired_rows(old.points(origin, spacing), src, ends)))


@torch.no_grad()
def _extract_native(implicit_surface, o):
    """extract_mesh(backend="native") after validation, o its arguments: the stages of extract_mesh's docstring, in its order."""
    from . import hip
    N, volume_size, level, filtering = o.N, o.volume_size, o.level, o.keep_largest is not None or o.min_component_faces is not None
    placement, model = placement_frame(N, volume_size), model_frame(N, volume_size)
    vol = sdf_volume(implicit_surface, volume_size, N, o.chunk, o.reference_shear, o.narrow_band, o.band_brick, o.band_lipschitz, level, o.band_info)
    verts, faces, ws, V = _count_and_emit(vol, level, *placement)
    mesh = _Mesh(verts, faces)
    if o.edges:
        if int(o.refine_evals) >= 1:
            edge, t, _ = refine_vertices(implicit_surface, vol, level, ws, V, volume_size, int(o.refine_evals))
        else:
            edge, _, t, _, _ = hip.mc_emit_edges(vol, level, ws, V)
        mesh.place = lambda origin, spacing: hip.mesh_edge_points(edge, t, vol.shape, origin, spacing)
        if int(o.refine_evals) >= 1:
            mesh.verts = mesh.place(*placement)
    if o.simplify_factor is not None:
        grid = mesh.place([0.0] * 3, [1.0] * 3)
        if filtering:                                               # before clustering can weld a floater to the surface
            grid, faces, _ = filter_components(grid, faces, o.keep_largest, o.min_component_faces)
        grid, faces, _ = simplify_clusters(grid, faces, vol.shape, o.simplify_factor, o.simplify_reg)
        if o.repair:                                                # on grid coordinates: the midpoints are vertices like the others
            grid, faces, _, _, info = repair_manifold(grid, faces, o.repair_wedge)
            if o.repair_info is not None:
                o.repair_info.update(info)
        mesh = _Mesh(grid_to_frame(grid, *placement), faces, lambda origin, spacing: grid_to_frame(grid, origin, spacing))
    elif o.repair:                                                  # stage 6 first, then the repair, both before any vertex is queried
        if filtering:
            mesh.verts, mesh.faces, mesh.src = filter_components(mesh.verts, mesh.faces, o.keep_largest, o.min_component_faces)
        mesh = _repair_stage(mesh, o)
    if o.vertex_normals or o.color_model is not None:
        mesh.normals, mesh.colors = _normals_and_colors(implicit_surface, o.color_model, mesh.points(*model))
    if filtering and o.simplify_factor is None and not o.repair:
        mesh.verts, mesh.faces, mesh.src = filter_components(mesh.verts, mesh.faces, o.keep_largest, o.min_component_faces)
        mesh.normals, mesh.colors = (a if a is None else a[mesh.src.long()] for a in (mesh.normals, mesh.colors))
    normals = mesh.normals if o.vertex_normals else None
    if o.texture_model is None:
        return write_ply(o.filepath, mesh.verts, mesh.faces, normals, mesh.colors)
    image, uv = bake_texture(mesh.points(*model), mesh.faces, lambda p: normal_view_radiance(o.texture_model, p)[1], patch=int(o.texture_patch),
                             query_fn=implicit_surface.forward_with_nablas, project=int(o.texture_project), level=level,
                             max_step=(o.simplify_factor or 1) * volume_size / N)
    return write_obj(o.filepath, mesh.verts, mesh.faces, uv, image, normals)


def extract_mesh(implicit_surface, volume_size=2.0, level=0.0, N=512, filepath="./surface.ply", show_progress=True, chunk=1 << 24,
                 reference_shear: bool = False, backend: str = "native", refine_evals: int = 0, vertex_normals: bool = False, color_model=None,
                 keep_largest: int = None, min_component_faces: int = None, narrow_band: bool = False, band_brick: int = 8,
                 band_lipschitz: float = BAND_LIPSCHITZ, band_info: dict = None, simplify_factor: int = None, simplify_reg: float = 0.01,
                 texture_model=None, texture_patch: int = 4, texture_project: int = 0, repair: bool = False, repair_wedge: str = "void",
                 repair_info: dict = None):
    """mesh_util.extract_mesh: SDF volume -> marching cubes -> a mesh file; returns filepath.  At the defaults: the reference's call and its
    two-element PLY.  Two frames: the mesh is PLACED as the reference places it, spacing volume_size / N, offset -volume_size / 2 (mesh_util.py:112;
    placement_frame); every network query of a vertex or texel is made in the MODEL's frame, the swept grid's, spacing volume_size / (N - 1)
    (model_frame), so no query depends on the placement.  show_progress is accepted for call compatibility: the sweep is a handful of kernel
    launches, there is nothing to show.  The arguments are checked first (last paragraph): a refused call imports, queries and writes nothing.

    backend="skimage": the reference's route (needs scikit-image and plyfile) - the volume goes to the host, Lewiner's marching cubes, plyfile;
    of the options it takes reference_shear alone.  backend="native" (default; nothing third-party, the volume stays on the GPU) is one
    sequence, a stage whose options are off being skipped; all off, stages 1, 2 and 7 are marching_cubes + write_ply:
      1. sdf_volume.  reference_shear=True samples the sheared grid the reference's true-division index arithmetic produces under Python 3
         (vertex-for-vertex parity with its meshes); the default is the regular grid ("deviations").  narrow_band=True sweeps
         only the bricks of band_brick^3 grid points that can hold the level set, given |grad sdf| <= band_lipschitz (banded_volume;
         csrc/mesh_band.hip): the file is the dense sweep's byte for byte when the bound holds; a piece of surface lying wholly inside bricks the
         bound wrongly ruled out is not found; a dict passed as band_info receives the sweep's counts.
      2. Marching cubes at `level` (a non-finite volume: ValueError), vertices in the placement frame; faces: these until stage 4 or 6 changes them.
      3. With any of refine_evals, vertex_normals, color_model, simplify_factor, texture_model: every vertex as (grid edge, t).  refine_evals >= 1
         moves t to the best of that many SDF evaluations (refine_vertices; 1 = the interpolated vertex) and the positions are emitted anew.
      4. simplify_factor=c >= 2, on grid coordinates: keep_largest / min_component_faces drop the floaters first - clustering could weld them to
         the surface -, then the vertices of every block of c^3 grid cells become one, placed by the quadrics of the block's faces
         (simplify_clusters; csrc/mesh_simplify.hip; simplify_reg pulls it toward the members' mean): roughly c^2 times fewer triangles.
         repair=True (off by default: every file stays the same byte for byte) then makes the mesh a 2-manifold: repair_manifold
         (csrc/mesh_repair.hip) cuts and stitches the non-manifold edges and bow-tie vertices clustering leaves - simplify_clusters keeps a
         surface closed and oriented, not manifold -, repair_wedge="void" (solids touching along an edge become one) or "solid" (they are
         separated); a dict passed as repair_info receives its counts.  Without simplify_factor the repair runs after stage 6's filter, which
         then comes before stage 5.  Small closed pieces the splitting sets free stay: keep_largest / min_component_faces run BEFORE the repair;
         filter_components on the written mesh is the caller's tool for them.  Flipped edges are left as they are.
      5. At the vertices there are now: vertex_normals writes nx ny nz = the normalised SDF gradient, color_model (the whole VolSDF / NeuS model)
         red green blue = its radiance looking down the normal (vertex_attributes).
      6. Without simplify_factor, keep_largest / min_component_faces (the sheared grid included): only the keep_largest largest connected components,
         and / or those of at least min_component_faces faces, survive (filter_components; csrc/mesh_components.hip), with normals and colours.
      7. write_ply; with texture_model (the whole model) write_obj instead: <stem>.obj, .mtl and .png, the .obj path returned, vertex_normals as
         the OBJ's vn.  bake_texture runs on the final mesh in the model's frame: every face owns a patch of texture_patch texel intervals along
         its legs in a per-face atlas, every texel is vertex_attributes' colour rule at the texel's own point; texture_project = k first moves the
         texels k Newton steps onto the level set, each at most (simplify_factor or 1) * volume_size / N long - a decimated face is a chord of
         the surface.  A mesh without faces, or an atlas past 16384 texels a side (use simplify_factor or a smaller patch): ValueError.

    Refused, the first that applies: texture_model with a filepath not ending in .obj, with color_model (OBJ has no standard vertex colours), with
    reference_shear, with backend="skimage", with texture_patch < 1 or texture_project < 0; simplify_factor, then narrow_band, with reference_shear
    (clusters and bricks are blocks of the regular lattice) or backend="skimage" (the clustering runs on the native extractor's vertices; Lewiner's
    ambiguity tests would read fill values); keep_largest / min_component_faces off the native backend (the components are found on the GPU);
    stage 3 with reference_shear or off the native backend (no regular frame; no edge table); an unknown backend; refine_evals < 0; a
    repair_wedge that is neither "void" nor "solid"; repair off the native backend."""
    o = types.SimpleNamespace(**locals())                            # the arguments as one value: the checks and the stages read them by name
    o.edges = bool(refine_evals or vertex_normals or color_model is not None or simplify_factor is not None or texture_model is not None)   # stage 3
    _check_extract_options(o)
    if backend == "skimage":
        return _extract_skimage(implicit_surface, volume_size, level, N, filepath, chunk, reference_shear)
    return _extract_native(implicit_surface, o)
