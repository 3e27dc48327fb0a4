#!/usr/bin/env python
"""Mesh extraction timing on one MI355X: the N^3 SDF sweep of the sphere-initialised VolSDF model (mesh_util.sdf_volume) beside the native
marching cubes on the same grid (nerfart_mc_count = classify + scans, nerfart_mc_emit).  Warm, HIP events, median of --iters runs.  Prints one
JSON line (NOT the driver's bench contract - that is bench.py).  Per-kernel times (classify apart from the scans) come from running this file
under `rocprofv3 --kernel-trace --stats` with --no-sdf.  `--narrow_band [--band_brick B]` adds, in the same job, the narrow-band sweep's median
time (banded_volume_ms, beside the dense sdf_volume_ms), the share of grid points it queried, its repair rounds and whether marching cubes gives
the dense sweep's mesh bit for bit.  `--simplify C` adds the simplify stage on the same mesh: mesh_util.simplify_clusters' median time, its two
halves (nerfart_mesh_simplify_count, _emit) and V, F -> V', F'.  DESIGN.md 4.7 says which of these figures have been taken."""
import argparse, json, os, statistics, sys
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
    args = ap.parse_args()
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
