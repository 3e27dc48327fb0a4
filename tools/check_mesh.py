#!/usr/bin/env python
"""Is a mesh a valid surface?  On the GPU (nerfart_amd.mesh_util.mesh_topology; csrc/mesh_topology.hip): watertight or not, how many holes, which
genus, how large - for a file extract_mesh wrote, before it goes to a printer, a simulation or any tool that needs a closed manifold surface.

    python tools/check_mesh.py --mesh surface.ply --components 5 --defects defects.ply

`--mesh` is a .ply or .obj file exactly as mesh_util.write_ply / write_obj write them.  Prints ONE JSON line: mesh_topology's dict - the counts
of proper / degenerate / bad faces, referenced vertices, edges, boundary / flipped / non-manifold edges, vertices with more than one fan,
boundary loops and the longest one; euler; closed, oriented, manifold, watertight - with the component list (most faces first: label, vertices,
edges, faces, boundary_edges, euler, closed, area, volume, genus, ...) cut to `--components K` entries (default 10; n_components says how many
there are), and the file under "mesh".  Nothing is repaired unless `--repair` is given.
`--repair OUT.ply [--repair_wedge void|solid]` writes the mesh after mesh_util.repair_manifold (csrc/mesh_repair.hip: non-manifold edges and bow-tie
vertices cut and stitched; positions and faces only, no per-vertex attribute is carried over) and prints a SECOND JSON line: {"repair": its
counts, "repaired": the same report of the repaired mesh}.
`--defects OUT.ply` writes the mesh with per-vertex colours; the first rule that applies decides:
    red      the vertices of boundary edges (edges in one face);
    magenta  the vertices of non-manifold edges (in more than two faces) and of flipped edges (their two faces run through them the same way);
    yellow   vertices with more than one fan of faces (bow-ties);
    grey     everything else."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RED, MAGENTA, YELLOW, GREY = (255, 0, 0), (255, 0, 255), (255, 255, 0), (160, 160, 160)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mesh", type=str, required=True, help="the mesh (.ply or .obj)")
    ap.add_argument("--components", type=int, default=10, help="how many components to list, largest first")
    ap.add_argument("--defects", type=str, default=None, help="write the mesh with per-vertex colours marking its defects (.ply)")
    ap.add_argument("--repair", type=str, default=None, help="write the mesh after repair_manifold (.ply) and print its report as a second line")
    ap.add_argument("--repair_wedge", type=str, default="void", choices=["void", "solid"], help="the pairing rule of --repair")
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


def defect_colors(faces, V):
    """[V, 3] uint8 on faces' device: the docstring's rule, from the twins and the fans"""
    from nerfart_amd import mesh_util
    twin, _, fans, _ = mesh_util.half_edges(faces, V)
    origin = faces.reshape(-1).long()
    target = faces[:, [1, 2, 0]].reshape(-1).long()
    colors = torch.tensor(GREY, dtype=torch.uint8, device=faces.device).repeat(V, 1)
    colors[fans > 1] = torch.tensor(YELLOW, dtype=torch.uint8, device=faces.device)
    for code, rgb in (((-2, -3), MAGENTA), ((-1,), RED)):                    # later rules win: red over magenta over yellow
        hit = torch.zeros_like(twin, dtype=torch.bool)
        for c in code:
            hit |= twin == c
        colors[torch.cat([origin[hit], target[hit]])] = torch.tensor(rgb, dtype=torch.uint8, device=faces.device)
    return colors


def report(verts, faces, components):
    """mesh_topology's dict without its tensors, the component list cut to `components` entries"""
    from nerfart_amd import mesh_util
    out = mesh_util.mesh_topology(verts, faces)
    del out["tensors"]
    out["n_components"] = len(out["components"])
    out["components"] = out["components"][:components]
    return out


def main(argv=None):
    from nerfart_amd import mesh_util
    args = parse(argv)
    if args.repair is not None and not args.repair.endswith(".ply"):
        raise ValueError(f"--repair writes a PLY: the path must end in .ply (got {args.repair!r})")
    if args.defects is not None and not args.defects.endswith(".ply"):
        raise ValueError(f"--defects writes a PLY: the path must end in .ply (got {args.defects!r})")
    if args.components < 0:
        raise ValueError(f"--components must be >= 0 (got {args.components})")
    assert torch.cuda.is_available(), "check_mesh needs the GPU (nerfart_amd has no CPU path)"
    dev = torch.device("cuda", 0)
    verts, faces = load_mesh(args.mesh, dev)
    out = report(verts, faces, args.components)
    out["mesh"] = {"path": args.mesh, "vertices": int(verts.shape[0]), "faces": int(faces.shape[0])}
    if args.defects is not None:
        mesh_util.write_ply(args.defects, verts, faces, colors=defect_colors(faces, int(verts.shape[0])).cpu().numpy())
        out["defects"] = args.defects
    print(json.dumps(out))
    if args.repair is not None:
        rverts, rfaces, _, _, info = mesh_util.repair_manifold(verts, faces, args.repair_wedge)
        mesh_util.write_ply(args.repair, rverts, rfaces)
        fixed = report(rverts, rfaces, args.components)
        fixed["mesh"] = {"path": args.repair, "vertices": int(rverts.shape[0]), "faces": int(rfaces.shape[0])}
        print(json.dumps({"repair": dict(info, wedge=args.repair_wedge), "repaired": fixed}))


if __name__ == "__main__":
    main()
