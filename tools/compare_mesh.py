#!/usr/bin/env python
"""How far one mesh is from another, on the GPU (nerfart_amd.mesh_util.mesh_distance; csrc/mesh_distance.hip): Chamfer, Hausdorff and F-score
between two files extract_mesh wrote - a decimated mesh against the undecimated one, two extraction settings, the surface before and after a
style fine-tune.

    python tools/compare_mesh.py --a before.ply --b after.ply --samples 1000000 --threshold 0.01 --heatmap moved.ply

`--a` / `--b` are .ply or .obj files exactly as mesh_util.write_ply / write_obj write them.  About `--samples` area-weighted points are drawn on
each surface (`--seed`), and each is measured against the other mesh: exactly, in float64, every face a candidate.  Prints ONE JSON line: per
direction (a_to_b, b_to_a) n, mean, rms, max and - with `--threshold T` - the share within T; chamfer (the mean of the two means), hausdorff (the
larger maximum), precision / recall / fscore at T.  `--max_distance D` stops every search at D: a sample farther away counts as D.
`--heatmap OUT.ply` writes mesh A with per-vertex colours coding each VERTEX's distance to B: black at 0 through red and yellow to white at the
largest distance found (or at D); the JSON line then also holds heatmap_max, the distance white stands for."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--a", type=str, required=True, help="mesh A (.ply or .obj)")
    ap.add_argument("--b", type=str, required=True, help="mesh B (.ply or .obj)")
    ap.add_argument("--samples", type=int, default=1 << 20, help="points drawn on each surface (in expectation)")
    ap.add_argument("--threshold", type=float, default=None, help="distance for precision / recall / fscore")
    ap.add_argument("--max_distance", type=float, default=float("inf"), help="bound of every search; farther samples count as this")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--heatmap", type=str, default=None, help="write A with per-vertex colours coding the distance to B (.ply)")
    return ap.parse_args(argv)


def load_mesh(path, dev):
    """(verts [V, 3] float32, faces [F, 3] int32) on the GPU"""
    from nerfart_amd import mesh_util
    if path.endswith(".obj"):
        m = mesh_util.read_obj(path)
    elif path.endswith(".ply"):
        m = mesh_util.read_ply(path)
    else:
        raise ValueError(f"a mesh file must end in .ply or .obj (got {path!r})")
    return torch.from_numpy(m["verts"]).to(dev).contiguous(), torch.from_numpy(m["faces"]).to(dev).contiguous()


def heat_colors(dist, top):
    """[n, 3] uint8: black (0) - red - yellow - white (top), linear in the distance"""
    t = (dist.double() / top if top > 0.0 else torch.zeros_like(dist, dtype=torch.float64)).clamp(0.0, 1.0) * 3.0
    rgb = torch.stack([t, t - 1.0, t - 2.0], dim=1).clamp(0.0, 1.0)
    return (rgb * 255.0 + 0.5).floor().to(torch.uint8)


def finite(o):
    """The dict with every non-finite number as None: JSON has no infinity (an empty B with no --max_distance gives one)."""
    if isinstance(o, dict):
        return {k: finite(v) for k, v in o.items()}
    return None if isinstance(o, float) and not np.isfinite(o) else o


def main(argv=None):
    from nerfart_amd import mesh_util
    args = parse(argv)
    if args.heatmap is not None and not args.heatmap.endswith(".ply"):
        raise ValueError(f"--heatmap writes a PLY: the path must end in .ply (got {args.heatmap!r})")
    assert torch.cuda.is_available(), "compare_mesh needs the GPU (nerfart_amd has no CPU path)"
    dev = torch.device("cuda", 0)
    va, fa = load_mesh(args.a, dev)
    vb, fb = load_mesh(args.b, dev)
    out = mesh_util.mesh_distance(va, fa, vb, fb, samples=args.samples, threshold=args.threshold, max_distance=args.max_distance, seed=args.seed)
    out.update(a={"path": args.a, "vertices": int(va.shape[0]), "faces": int(fa.shape[0])},
               b={"path": args.b, "vertices": int(vb.shape[0]), "faces": int(fb.shape[0])}, seed=args.seed)
    out["max_distance"] = args.max_distance
    if args.heatmap is not None:
        dist, _ = mesh_util.closest_on_mesh(va, vb, fb, args.max_distance)
        known = dist[torch.isfinite(dist)]
        top = float(known.max()) if known.numel() else 0.0
        mesh_util.write_ply(args.heatmap, va, fa, colors=heat_colors(torch.nan_to_num(dist, nan=top, posinf=top), top).cpu().numpy())
        out.update(heatmap=args.heatmap, heatmap_max=top)
    print(json.dumps(finite(out)))


if __name__ == "__main__":
    main()
