#!/usr/bin/env python
"""Counterpart of the reference's tools/extract_surface.py: config (+ checkpoint) -> SDF grid -> marching cubes -> .ply, all on
the GPU (nerfart_amd.mesh_util.extract_mesh: the SDF kernel, csrc/marching_cubes.hip, a numpy PLY writer; nothing third-party).

    python tools/extract_surface.py --config configs/volsdf.yaml --load_pt ckpts/latest.pt --N 512 --volume_size 2.0 --out surface.ply

`--refine 5 --normals --colors` (no reference counterpart) moves the vertices onto the surface along their grid edges and adds per-vertex normals and
colours to the file; without them the file is the reference's two elements.  `--keep_largest 1` (or `--min_faces M`) drops the floaters: only the
largest connected components of the surface are written.  `--narrow_band [--band_brick B --band_lipschitz L]` sweeps the SDF only near the surface
(mesh_util.banded_volume; the same file when L bounds |grad sdf|) and prints the sweep's counts as one JSON line.  `--simplify C [--simplify_reg R]`
decimates the mesh on the GPU before it is written: the vertices of every block of C^3 grid cells become one, placed by the quadric error metric of
the block's faces (mesh_util.simplify_clusters), after the floaters are gone and before normals and colours are queried.  `--texture
[--texture_patch P --texture_project K]` with `--out mesh.obj` writes a textured mesh instead of a PLY - mesh.obj, mesh.mtl, mesh.png: every face
of the final mesh gets a patch of P texel intervals along its legs in a per-face atlas, baked on the GPU from the radiance net looking down the
normal (mesh_util.bake_texture); K Newton steps put the texels of a decimated face back onto the surface first.  `--repair [--repair_wedge
void|solid]` makes the mesh a 2-manifold before it is written (mesh_util.repair_manifold: the non-manifold edges and bow-tie vertices --simplify
leaves are cut and stitched; solids touching along an edge become one with `void`, are separated with `solid`) and prints its counts as one JSON
line.  Without --load_pt the mesh is the model's sphere initialisation.  `--k1:k2 v` overrides of the config work as everywhere (nerfart_amd.config)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    """(args, config) from the command line: the reference's parser (--config / --resume_dir) plus this tool's options."""
    from nerfart_amd import config as cfg
    from nerfart_amd.mesh_util import BAND_LIPSCHITZ
    parser = cfg.create_args_parser()
    parser.add_argument("--load_pt", type=str, default=None, help="checkpoint (torch.save({'model': state_dict, ...})); default: the initialisation")
    parser.add_argument("--N", type=int, default=512, help="grid points per axis")
    parser.add_argument("--volume_size", type=float, default=2.0, help="edge length of the cube, centred at the origin")
    parser.add_argument("--level", type=float, default=0.0)
    parser.add_argument("--chunk", type=int, default=1 << 24, help="grid points per SDF launch")
    parser.add_argument("--out", type=str, default="surface.ply")
    parser.add_argument("--refine", type=int, default=0, help="SDF evaluations per vertex moving it along its grid edge onto the surface (0: the "
                                                              "interpolated vertices, the reference's; 5 is plenty)")
    parser.add_argument("--normals", action="store_true", help="write nx ny nz: the normalised SDF gradient at every vertex")
    parser.add_argument("--colors", action="store_true", help="write red green blue: the radiance net's colour looking down the normal")
    parser.add_argument("--keep_largest", type=int, default=None, help="keep only the K largest connected components of the mesh (by faces): "
                                                                       "drops the floaters")
    parser.add_argument("--min_faces", type=int, default=None, help="keep only the connected components of at least M faces")
    parser.add_argument("--narrow_band", action="store_true", help="query the SDF only in the bricks of the grid that can hold the surface (the same "
                                                                   "file when --band_lipschitz bounds |grad sdf|); prints the sweep's counts")
    parser.add_argument("--band_brick", type=int, default=8, help="grid points per brick edge of --narrow_band (2 .. 64)")
    parser.add_argument("--band_lipschitz", type=float, default=BAND_LIPSCHITZ, help="the bound on |grad sdf| --narrow_band relies on; a trained "
                                                                                     "checkpoint may need more than the default")
    parser.add_argument("--simplify", type=int, default=None, help="merge the vertices of every block of C^3 grid cells into one (C >= 2): roughly "
                                                                   "C^2 times fewer triangles")
    parser.add_argument("--simplify_reg", type=float, default=0.01, help="how strongly --simplify pulls a merged vertex toward the mean of its members "
                                                                         "where the faces' planes do not fix it")
    parser.add_argument("--texture", action="store_true", help="write a textured mesh, <out>.obj + .mtl + .png (--out must end in .obj), instead of "
                                                               "a PLY: a per-face atlas baked from the radiance net; not together with --colors")
    parser.add_argument("--texture_patch", type=int, default=4, help="texel intervals along a triangle's legs in the atlas of --texture (>= 1)")
    parser.add_argument("--texture_project", type=int, default=0, help="Newton steps that move the texels of --texture onto the level set before "
                                                                       "they are coloured (2 is plenty after --simplify)")
    parser.add_argument("--repair", action="store_true", help="cut and stitch non-manifold edges and bow-tie vertices (what --simplify leaves) before "
                                                              "normals, colours and texture are queried; prints the repair's counts")
    parser.add_argument("--repair_wedge", type=str, default="void", choices=["void", "solid"], help="how --repair pairs the faces around an edge of "
                        "more than two: 'void' joins solids that touch along it, 'solid' separates them")
    args, unknown = parser.parse_known_args(argv)
    return args, cfg.load_config(args, unknown)


def main():
    from nerfart_amd import frameworks, mesh_util
    args, conf = parse()
    assert torch.cuda.is_available(), "extract_surface needs the GPU (nerfart_amd has no CPU path)"
    dev = torch.device("cuda", conf.device_ids[0])
    model = frameworks.get_model(conf)[0]
    if args.load_pt is not None:
        state = torch.load(args.load_pt, map_location="cpu")
        model.load_state_dict(state["model"] if "model" in state else state)
    model.to(dev)
    info, repair_info = {}, {}
    path = mesh_util.extract_mesh(model.implicit_surface, volume_size=args.volume_size, level=args.level, N=args.N, filepath=args.out, chunk=args.chunk,
                                  refine_evals=args.refine, vertex_normals=args.normals, color_model=model if args.colors else None,
                                  keep_largest=args.keep_largest, min_component_faces=args.min_faces, narrow_band=args.narrow_band,
                                  band_brick=args.band_brick, band_lipschitz=args.band_lipschitz, band_info=info, simplify_factor=args.simplify,
                                  simplify_reg=args.simplify_reg, texture_model=model if args.texture else None, texture_patch=args.texture_patch,
                                  texture_project=args.texture_project, repair=args.repair, repair_wedge=args.repair_wedge, repair_info=repair_info)
    if args.narrow_band:
        print(json.dumps(info))
    if args.repair:
        print(json.dumps(repair_info))
    print(path)


if __name__ == "__main__":
    main()
