#!/usr/bin/env python
"""Mesh extraction timing on one MI355X: the N^3 SDF sweep of the sphere-initialised VolSDF model (mesh_util.sdf_volume) beside the native
marching cubes on the same grid (nerfart_mc_count = classify + scans, nerfart_mc_emit).  Warm, HIP events, median of --iters runs.  Prints one
JSON line (NOT the driver's bench contract - that is bench.py).  Per-kernel times (classify apart from the scans) come from running this file
under `rocprofv3 --kernel-trace --stats` with --no-sdf.  `--narrow_band [--band_brick B]` adds, in the same job, the narrow-band sweep's median
time (banded_volume_ms, beside the dense sdf_volume_ms), the share of grid points it queried, its repair rounds and whether marching cubes gives
the dense sweep's mesh bit for bit.  `--simplify C` adds the simplify stage on the same mesh: mesh_util.simplify_clusters' median time, its two
halves (nerfart_mesh_simplify_count, _emit) and V, F -> V', F'.  `--texture P [--texture_project K]` adds the texture bake of that mesh (the
simplified one with --simplify, else marching cubes' own) in the model's frame: nerfart_mesh_atlas_points, the K projection steps (SDF + gradient
queries and nerfart_mesh_project_step; the step kernel also alone), the colour queries, mesh_util.bake_texture as a whole, and - once, on the
host's clock - mesh_util.write_obj.  `--render H W` adds the rasteriser (csrc/mesh_raster.hip) on that mesh (the simplified one with --simplify) in
the model's frame, seen by scene.camera(H, W): the three raster stages each alone (nerfart_mesh_project, _raster, _resolve), mesh_util.rasterize as
a whole (with its one host read), and the shading calls - nerfart_mesh_interp of per-corner UVs and nerfart_mesh_sample_bilinear on an atlas of
patch --texture (default 4) filled with noise: the sampling cost does not depend on what the texels hold.  DESIGN.md 4.7 says which of these
figures have been taken.  `--distance [--distance_samples S]` (with --simplify) adds the mesh distance (csrc/mesh_distance.hip) of the simplified mesh
against marching cubes' own, in grid cells: the stages each alone - sampling (nerfart_mesh_sample_count, _emit), the grid build of the undecimated
mesh (nerfart_mesh_grid_count + _fill, with its host read) and the query (nerfart_mesh_closest) of S samples of the simplified mesh -,
mesh_util.mesh_distance as a whole (both directions), and the distances it found; with --narrow_band also the distance between the banded
sweep's mesh and the dense one.  `--topology` adds the half-edge adjacency and manifold report (csrc/mesh_topology.hip) of the
extracted mesh, and of the simplified one with --simplify: nerfart_mesh_half_edges and nerfart_mesh_component_stats each alone, beside
nerfart_mesh_components on the same mesh (the yardstick for "a pass over the faces"), the edge table's size, mesh_util.mesh_topology as a whole
(with its one host read) and the dict it returns (components cut to the five largest).  `--repair [--repair_wedge W]` adds the manifold repair
(csrc/mesh_repair.hip) of the extracted mesh, and of the simplified one with --simplify: mesh_util.repair_manifold as a whole (with its one host
read), nerfart_mesh_repair_count and _emit each alone, nerfart_mesh_half_edges on the same mesh in the same run (the yardstick: the pass
contains one half-edge build), the workspace, the counts it reports, and mesh_util.mesh_topology of the repaired mesh."""
import argparse, json, os, statistics, sys, tempfile, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--volume_size", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--no-sdf", action="store_true", help="time the extractor only (the volume is still swept once)")
    ap.add_argument("--narrow_band", action="store_true", help="also time the narrow-band sweep (mesh_util.banded_volume) and compare its mesh")
    ap.add_argument("--band_brick", type=int, default=8)
    ap.add_argument("--simplify", type=int, default=None, help="also time mesh_util.simplify_clusters with this cluster factor on the extracted mesh")
    ap.add_argument("--texture", type=int, default=None, help="also time the texture bake (mesh_util.bake_texture) with this patch size")
    ap.add_argument("--texture_project", type=int, default=2, help="projection steps of --texture")
    ap.add_argument("--render", type=int, nargs=2, default=None, metavar=("H", "W"), help="also time the rasteriser on the extracted mesh at this image size")
    ap.add_argument("--distance", action="store_true", help="also time mesh_util.mesh_distance of the simplified mesh against the extracted one (needs --simplify)")
    ap.add_argument("--distance_samples", type=int, default=1 << 20)
    ap.add_argument("--topology", action="store_true", help="also time mesh_util.half_edges / component_stats and report the topology of the mesh(es)")
    ap.add_argument("--repair", action="store_true", help="also time mesh_util.repair_manifold on the mesh(es) and report the repaired topology")
    ap.add_argument("--repair_wedge", default="void", choices=["void", "solid"])
    args = ap.parse_args()
    if args.distance and not args.simplify:
        ap.error("--distance compares the simplified mesh with the extracted one: give --simplify C")
    from nerfart_amd import scene, mesh_util, hip
    dev = torch.device("cuda", 0)
    model, _, _ = scene.build_model("VolSDF", seed=0, beta=0.01, device=dev, precision="mixed")
    N, vs = args.N, args.volume_size
    sweep = lambda: mesh_util.sdf_volume(model.implicit_surface, volume_size=vs, N=N)
    vol = sweep()                                                  # warm-up of the SDF kernel
    res = {"workload": f"extract_mesh stages, VolSDF sphere initialisation, {N}^3 grid over [-{vs / 2}, {vs / 2}]^3"}
    if not args.no_sdf:
        res["sdf_volume_ms"], vol = timed(sweep, max(3, args.iters // 4))
    ws = torch.empty(hip.mc_workspace_bytes(N, N, N), dtype=torch.uint8, device=dev)
    _, counts = hip.mc_count(vol, 0.0, ws=ws)                      # warm-up
    V, F, bad = (int(c) for c in counts.cpu())
    assert not bad
    hip.mc_emit(vol, 0.0, [-vs / 2] * 3, [vs / N] * 3, ws, V, F)
    res["mc_count_ms"], _ = timed(lambda: hip.mc_count(vol, 0.0, ws=ws), args.iters)
    res["mc_emit_ms"], _ = timed(lambda: hip.mc_emit(vol, 0.0, [-vs / 2] * 3, [vs / N] * 3, ws, V, F), args.iters)
    res.update(vertices=V, triangles=F, workspace_MiB=round(ws.numel() / 2 ** 20, 1),
               classify_bytes=N ** 3 * (4 + 2))                    # the volume read once + two bytes written per point
    if args.narrow_band:                                           # the banded sweep beside the dense one above: same job, same model, same grid
        info = {}
        banded = lambda: mesh_util.sdf_volume(model.implicit_surface, volume_size=vs, N=N, narrow_band=True, band_brick=args.band_brick, band_info=info)
        bvol = banded()                                            # warm-up
        verts, faces = hip.mc_emit(vol, 0.0, [-vs / 2] * 3, [vs / N] * 3, ws, V, F)
        res["mesh_equal"] = False                                  # stays False if the banded volume raises in marching_cubes
        bverts, bfaces = mesh_util.marching_cubes(bvol, 0.0, spacing=[vs / N] * 3, origin=[-vs / 2] * 3)
        res["mesh_equal"] = bool(torch.equal(verts.view(torch.int32), bverts.view(torch.int32)) and torch.equal(faces, bfaces))
        if args.distance:
            d = mesh_util.mesh_distance(bverts, bfaces, verts, faces, samples=args.distance_samples)
            res["distance_banded_vs_dense"] = {"chamfer": d["chamfer"], "hausdorff": d["hausdorff"]}
        del bvol, verts, faces, bverts, bfaces
        res["banded_volume_ms"], _ = timed(banded, max(3, args.iters // 4))
        res.update(band_brick=args.band_brick, band_lipschitz=mesh_util.BAND_LIPSCHITZ, evaluated_share=round(info["evaluated_points"] / N ** 3, 5),
                   probe_share=round(info["bricks"] / N ** 3, 5), repair_rounds=info["repair_rounds"], completed_dense=info["completed_dense"],
                   active_bricks=info["active"], bricks=info["bricks"])
    if args.simplify:                                              # the simplify stage on the mesh above, in grid coordinates
        c = args.simplify
        gverts, gfaces = hip.mc_emit(vol, 0.0, [0.0] * 3, [1.0] * 3, ws, V, F)
        sws = torch.empty(hip.mesh_simplify_workspace_bytes(V, F, c, vol.shape), dtype=torch.uint8, device=dev)
        out_v, out_f, cluster = mesh_util.simplify_clusters(gverts, gfaces, vol.shape, c)      # warm-up; the sizes
        res["simplify_ms"], _ = timed(lambda: mesh_util.simplify_clusters(gverts, gfaces, vol.shape, c), args.iters)
        res["simplify_count_ms"], _ = timed(lambda: hip.mesh_simplify_count(gverts, gfaces, vol.shape, c, ws=sws), args.iters)
        res["simplify_emit_ms"], _ = timed(lambda: hip.mesh_simplify_emit(gverts, gfaces, vol.shape, c, 0.01, sws, cluster, out_v.shape[0], out_f.shape[0]),
                                           args.iters)
        res.update(simplify_factor=c, simplified_vertices=int(out_v.shape[0]), simplified_triangles=int(out_f.shape[0]),
                   simplify_workspace_MiB=round(sws.numel() / 2 ** 20, 1))
    if args.topology:                                              # adjacency and manifold report, in grid coordinates
        def topology(tag, tv, tf):
            Vt, Ft = int(tv.shape[0]), int(tf.shape[0])
            tws = torch.empty(hip.mesh_topology_workspace_bytes(Vt, Ft), dtype=torch.uint8, device=dev)
            hip.mesh_half_edges(tf, Vt, ws=tws)                    # warm-ups
            label, _, _ = hip.mesh_components(tf, Vt)
            hip.mesh_component_stats(tv, tf, label, tws)
            res[tag + "half_edges_ms"], _ = timed(lambda: hip.mesh_half_edges(tf, Vt, ws=tws), args.iters)
            res[tag + "component_stats_ms"], _ = timed(lambda: hip.mesh_component_stats(tv, tf, label, tws), args.iters)
            res[tag + "mesh_components_ms"], _ = timed(lambda: hip.mesh_components(tf, Vt), args.iters)
            res[tag + "mesh_topology_ms"], report = timed(lambda: mesh_util.mesh_topology(tv, tf), max(3, args.iters // 4))
            del report["tensors"]
            report["n_components"], report["components"] = len(report["components"]), report["components"][:5]
            # the default table's size, asked of the library: the table_log2 whose workspace is the default's (at these sizes every table is a
            # multiple of 256 bytes, so exactly one matches)
            slots = 1 << [k for k in range(1, 32) if int(hip.lib.nerfart_mesh_topology_workspace_bytes(Vt, Ft, k)) == tws.numel()][-1]
            res.update({tag + "topology": report, tag + "topology_workspace_MiB": round(tws.numel() / 2 ** 20, 1), tag + "topology_table_slots": slots,
                        tag + "topology_table_MiB": round(slots * 24 / 2 ** 20, 1), tag + "topology_table_load": round(report["edges"] / slots, 4),
                        tag + "topology_probe_length": "not measured"})
        topology("", *hip.mc_emit(vol, 0.0, [0.0] * 3, [1.0] * 3, ws, V, F))
        if args.simplify:
            topology("simplified_", out_v, out_f)
    if args.repair:                                                # cut and stitch, in grid coordinates
        def repair(tag, tv, tf):
            Vt, Ft, wedge = int(tv.shape[0]), int(tf.shape[0]), args.repair_wedge
            rws = torch.empty(hip.mesh_repair_workspace_bytes(Vt, Ft), dtype=torch.uint8, device=dev)
            tws = torch.empty(hip.mesh_topology_workspace_bytes(Vt, Ft), dtype=torch.uint8, device=dev)
            _, counts, _ = hip.mesh_repair_count(tv, tf, wedge, ws=rws)     # warm-ups; the sizes
            V1, M, Fa, Fx = (int(c) for c in counts.cpu())
            hip.mesh_repair_emit(tv, tf, rws, V1, M, Fa + Fx)
            hip.mesh_half_edges(tf, Vt, ws=tws)
            res[tag + "repair_manifold_ms"], out = timed(lambda: mesh_util.repair_manifold(tv, tf, wedge), args.iters)
            res[tag + "repair_count_ms"], _ = timed(lambda: hip.mesh_repair_count(tv, tf, wedge, ws=rws), args.iters)
            res[tag + "repair_emit_ms"], _ = timed(lambda: hip.mesh_repair_emit(tv, tf, rws, V1, M, Fa + Fx), args.iters)
            res[tag + "repair_half_edges_ms"], _ = timed(lambda: hip.mesh_half_edges(tf, Vt, ws=tws), args.iters)
            report = mesh_util.mesh_topology(out[0], out[1])
            del report["tensors"]
            report["n_components"], report["components"] = len(report["components"]), report["components"][:5]
            res.update({tag + "repair_wedge": wedge, tag + "repair_info": out[4], tag + "repair_workspace_MiB": round(rws.numel() / 2 ** 20, 1),
                        tag + "repaired_vertices": int(out[0].shape[0]), tag + "repaired_triangles": int(out[1].shape[0]),
                        tag + "repaired_topology": report})
        repair("", *hip.mc_emit(vol, 0.0, [0.0] * 3, [1.0] * 3, ws, V, F))
        if args.simplify:
            repair("simplified_", out_v, out_f)
    if args.distance:                                              # the simplified mesh against the extracted one, in grid cells
        S, seed = args.distance_samples, 0
        grid = mesh_util.default_distance_grid(F)
        sample = lambda: mesh_util.sample_surface(out_v, out_f, n=S, seed=seed)
        points, _ = sample()                                       # warm-ups
        g = hip.mesh_grid_build(gverts, gfaces, grid)
        hip.mesh_closest(points, gverts, gfaces, g)
        res["distance_sample_ms"], _ = timed(sample, args.iters)
        res["distance_grid_build_ms"], _ = timed(lambda: hip.mesh_grid_build(gverts, gfaces, grid), args.iters)
        res["distance_closest_ms"], (dist, _, visited) = timed(lambda: hip.mesh_closest(points, gverts, gfaces, g, want_visited=True), args.iters)
        res["distance_total_ms"], d = timed(lambda: mesh_util.mesh_distance(out_v, out_f, gverts, gfaces, samples=S, threshold=0.5, seed=seed),
                                            max(3, args.iters // 4))
        res.update(distance_samples=int(points.shape[0]), distance_grid=list(grid), distance_entries=g.entries,
                   distance_grid_workspace_MiB=round(g.ws.numel() / 2 ** 20, 1), distance_faces_tested_mean=float(visited.double().mean()),
                   distance_faces_tested_max=int(visited.max()), distance_unit="grid cells", distance=d)
    if args.texture:                                               # the bake of the final mesh, in the model's frame
        P, K, c = args.texture, args.texture_project, args.simplify or 1
        if args.simplify:
            tverts, tfaces = mesh_util.grid_to_frame(out_v, *mesh_util.model_frame(N, vs)), out_f
        else:
            tverts, tfaces = hip.mc_emit(vol, 0.0, *mesh_util.model_frame(N, vs), ws, V, F)
        surface, max_step, chunk = model.implicit_surface, c * vs / N, mesh_util.TEXEL_CHUNK
        S, Cw, Ch, W, H = hip.mesh_atlas_layout(tfaces.shape[0], P)
        points, face_of, _ = hip.mesh_atlas_points(tverts, tfaces, P)                           # warm-up
        res["texture_points_ms"], _ = timed(lambda: hip.mesh_atlas_points(tverts, tfaces, P), args.iters)
        start = torch.nonzero(face_of.reshape(-1) >= 0).reshape(-1)
        start = points[start]
        parts = lambda p: [p[s:s + chunk] for s in range(0, p.shape[0], chunk)]

        def project():
            p = start.clone()
            for _ in range(K):
                for part in parts(p):
                    sdf, nabla = surface.forward_with_nablas(part)[:2]
                    hip.mesh_project_step(part, sdf.reshape(-1).contiguous(), nabla.reshape(-1, 3).contiguous(), 0.0, max_step)
            return p
        color = lambda p: [mesh_util.quantize_colors(mesh_util.normal_view_radiance(model, part)[1]) for part in parts(p)]
        at = project()                                             # warm-ups
        color(at)
        res["texture_project_ms"], _ = timed(project, max(3, args.iters // 4))
        queried = [(part, *(t.contiguous() for t in surface.forward_with_nablas(part)[:2])) for part in parts(start.clone())]
        res["texture_project_step_kernel_ms"], _ = timed(lambda: [hip.mesh_project_step(p_, s_, n_, 0.0, max_step) for p_, s_, n_ in queried], args.iters)
        res["texture_color_ms"], _ = timed(lambda: color(at), max(3, args.iters // 4))
        bake = lambda: mesh_util.bake_texture(tverts, tfaces, lambda p: mesh_util.normal_view_radiance(model, p)[1], patch=P,
                                              query_fn=surface.forward_with_nablas, project=K, level=0.0, max_step=max_step)
        res["texture_bake_ms"], (image, uv) = timed(bake, max(3, args.iters // 4))
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            mesh_util.write_obj(os.path.join(tmp, "bench.obj"), tverts, tfaces, uv, image)
            res["texture_write_obj_s"] = round(time.perf_counter() - t0, 2)
            res["texture_png_MiB"] = round(os.path.getsize(os.path.join(tmp, "bench.png")) / 2 ** 20, 2)
        res.update(texture_patch=P, texture_project=K, texture_faces=int(tfaces.shape[0]), texture_image=[W, H], texture_valid_texels=int(start.shape[0]),
                   texture_points_bytes=W * H * 16 + int(tfaces.shape[0]) * 12)      # written per texel: 12 + 4; the faces read once (vertices from cache)
    if args.render:                                                # the rasteriser on the final mesh, in the model's frame
        H, W = args.render
        if args.simplify:
            rverts, rfaces = mesh_util.grid_to_frame(out_v, *mesh_util.model_frame(N, vs)), out_f
        else:
            rverts, rfaces = hip.mc_emit(vol, 0.0, *mesh_util.model_frame(N, vs), ws, V, F)
        c2w, K = scene.camera(H, W)
        camera, near = hip.mesh_camera(c2w, K), 1e-3
        xy_fix, cam, valid = hip.mesh_project(rverts, camera, near)                            # warm-ups
        zbuf, info = hip.mesh_raster(xy_fix, cam, valid, rfaces, camera, near, H, W)
        r = hip.mesh_resolve(zbuf, cam, rfaces, camera, H, W)
        res["render_project_ms"], _ = timed(lambda: hip.mesh_project(rverts, camera, near), args.iters)
        res["render_raster_ms"], _ = timed(lambda: hip.mesh_raster(xy_fix, cam, valid, rfaces, camera, near, H, W), args.iters)
        res["render_resolve_ms"], _ = timed(lambda: hip.mesh_resolve(zbuf, cam, rfaces, camera, H, W), args.iters)
        res["render_rasterize_ms"], _ = timed(lambda: mesh_util.rasterize(rverts, rfaces, c2w, K, H, W, near), args.iters)
        P = args.texture or 4
        _, _, _, Wt, Ht = hip.mesh_atlas_layout(rfaces.shape[0], P)
        uv = torch.from_numpy(mesh_util.atlas_uvs(rfaces.shape[0], P)).float().to(dev).contiguous()
        atlas = torch.randint(0, 256, (Ht, Wt, 3), dtype=torch.uint8, device=dev)
        pix_uv = hip.mesh_interp(r["face_id"], r["bary"], uv)
        hip.mesh_sample_bilinear(pix_uv, atlas, r["mask"])
        res["render_interp_uv_ms"], _ = timed(lambda: hip.mesh_interp(r["face_id"], r["bary"], uv), args.iters)
        res["render_sample_bilinear_ms"], _ = timed(lambda: hip.mesh_sample_bilinear(pix_uv, atlas, r["mask"]), args.iters)
        bad, n_skipped, n_rejected, n_large = (int(c) for c in info.cpu())
        assert not bad
        res.update(render_image=[W, H], render_vertices=int(rverts.shape[0]), render_faces=int(rfaces.shape[0]), render_covered_pixels=int(r["mask"].sum()),
                   render_n_skipped=n_skipped, render_n_rejected=n_rejected, render_large_faces=n_large, render_atlas=[Wt, Ht])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
