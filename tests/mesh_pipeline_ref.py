"""mesh_util.extract_mesh's native pipeline stated by hand, from the public stage functions only - it never calls extract_mesh - and the small
pieces the mesh tests share: the decimated mesh tests/test_gpu_mesh_texture.py and tests/test_gpu_mesh_raster.py look at, and a surface with
floaters.  tests/test_gpu_mesh_pipeline.py compares the files of `extract_by_hand` with extract_mesh's byte for byte."""
import torch


class WithFloaters(torch.nn.Module):
    """The model's SDF with two small spheres far from the object united to it: the floaters of a fine-tuned field, made on purpose."""
    SPHERES = (((1.2, 1.2, 1.2), 0.15), ((-1.2, 1.1, -1.2), 0.1))

    def __init__(self, surface):
        super().__init__()
        self.surface = surface

    def forward(self, x):
        d = self.surface.forward(x)
        for c, r in self.SPHERES:
            d = torch.minimum(d, (x - torch.tensor(c, device=x.device)).norm(dim=-1) - r)
        return d


def decimated(surface, N, volume_size, factor):
    """(vertices in the model's frame, in the placement frame, faces) of extract_mesh(simplify_factor=factor), by hand."""
    from nerfart_amd import mesh_util
    vol = mesh_util.sdf_volume(surface, volume_size, N)
    verts, faces = mesh_util.marching_cubes(vol, 0.0)
    g, f, _ = mesh_util.simplify_clusters(verts, faces, vol.shape, factor)
    return (mesh_util.grid_to_frame(g, *mesh_util.model_frame(N, volume_size)), mesh_util.grid_to_frame(g, *mesh_util.placement_frame(N, volume_size)), f)


@torch.no_grad()
def extract_by_hand(surface, filepath, N, volume_size, refine_evals=0, vertex_normals=False, color_model=None, keep_largest=None, narrow_band=False,
                    band_brick=8, simplify_factor=None, texture_model=None, texture_patch=4, texture_project=0):
    """The file(s) extract_mesh(surface, volume_size, 0.0, N, filepath, backend="native", <the same options>) writes; returns filepath.  The
    numbers are the stages of extract_mesh's docstring.  The vertices in the model's frame are computed once here and carried along; what
    extract_mesh does instead is its own business as long as the bytes are these."""
    from nerfart_amd import hip, mesh_util as mu
    level = 0.0
    placement, model = mu.placement_frame(N, volume_size), mu.model_frame(N, volume_size)
    vol = mu.sdf_volume(surface, volume_size, N, narrow_band=narrow_band, band_brick=band_brick, level=level)                            # 1
    ws, counts = hip.mc_count(vol, level)                                                                                                # 2
    V, F, bad = (int(c) for c in counts.cpu())
    assert not bad
    verts, faces = hip.mc_emit(vol, level, *placement, ws, V, F)
    pts = normals = colors = None
    if refine_evals or vertex_normals or color_model is not None or simplify_factor is not None or texture_model is not None:            # 3
        if refine_evals >= 1:
            edge, t, _ = mu.refine_vertices(surface, vol, level, ws, V, volume_size, refine_evals)
            verts = hip.mesh_edge_points(edge, t, vol.shape, *placement)
        else:
            edge, _, t, _, _ = hip.mc_emit_edges(vol, level, ws, V)
        if simplify_factor is not None:                                                                                                  # 4
            grid = hip.mesh_edge_points(edge, t, vol.shape, [0.0] * 3, [1.0] * 3)
            if keep_largest is not None:
                grid, faces, _ = mu.filter_components(grid, faces, keep_largest)
            grid, faces, _ = mu.simplify_clusters(grid, faces, vol.shape, simplify_factor)
            verts, pts = mu.grid_to_frame(grid, *placement), mu.grid_to_frame(grid, *model)
        else:
            pts = hip.mesh_edge_points(edge, t, vol.shape, *model)
    if color_model is not None:                                                                                                          # 5
        normals, colors = mu.vertex_attributes(color_model, pts)
    elif vertex_normals:
        normals = hip.normalize_dirs(surface.forward_with_nablas(pts)[1].contiguous())
    if not vertex_normals:
        normals = None
    if keep_largest is not None and simplify_factor is None:                                                                             # 6
        verts, faces, src = mu.filter_components(verts, faces, keep_largest)
        normals, colors, pts = (a if a is None else a[src.long()] for a in (normals, colors, pts))
    if texture_model is None:                                                                                                            # 7
        return mu.write_ply(filepath, verts, faces, normals, colors)
    image, uv = mu.bake_texture(pts, faces, lambda p: mu.normal_view_radiance(texture_model, p)[1], patch=texture_patch,
                                query_fn=surface.forward_with_nablas, project=texture_project, level=level,
                                max_step=(simplify_factor or 1) * volume_size / N)
    return mu.write_obj(filepath, verts, faces, uv, image, normals)
