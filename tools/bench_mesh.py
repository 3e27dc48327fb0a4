#!/usr/bin/env python
"""Mesh extraction timing on one MI355X: the N^3 SDF sweep of the sphere-initialised VolSDF model (mesh_util.sdf_volume) beside the native
marching cubes on the same grid (nerfart_mc_count = classify + scans, nerfart_mc_emit).  Warm, HIP events, median of --iters runs.  Prints one
JSON line (NOT the driver's bench contract - that is bench.py).  Per-kernel times (classify apart from the scans) come from running this file
under `rocprofv3 --kernel-trace --stats` with --no-sdf.  DESIGN.md 4.7 says which of these figures have been taken."""
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
