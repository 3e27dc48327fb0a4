#!/usr/bin/env python
"""Looks at a mesh extract_mesh wrote: rasterises it on the GPU (nerfart_amd.mesh_util.render_mesh; csrc/mesh_raster.hip) from an orbit of cameras
and writes PNG frames - rgb, depth, normals.

    python tools/render_mesh.py --mesh mesh.obj --H 270 --W 480 --views 8 --out frames/

`--mesh` is a .ply (per-vertex colours if the file has them, else the normals as colours) or a textured .obj, exactly as mesh_util.write_ply /
write_obj write them.  The cameras are scene.camera's look-at at `--views` angles around the origin (`--cam_dist`, `--focal_scale`), with
rend_util.get_rays' conventions, so a frame lines up pixel for pixel with a render_fn or surface_render frame of the same camera.  Frames:
<out>/rgb_000.png, depth_000.png (near is white, a miss black, scaled over the frame's hits), normal_000.png ((n + 1) / 2).

With `--config cfg.yaml [--load_pt ckpt.pt] --compare` the same cameras are also rendered with ray_casting.surface_render (sphere tracing) and,
per view, one JSON line says: pixels hit by both, by the mesh only, by the field only; median / p99 / max |depth difference| in grid steps
(volume_size / N) over the pixels hit by both; PSNR of rgb over all pixels.  extract_mesh places its files with spacing volume_size / N while the
model's grid has volume_size / (N - 1) (mesh_util.placement_frame / model_frame): `--N` and `--volume_size` of the extraction put the mesh back into
the model's frame for the comparison (and for the frames written alongside it).  `--scene VolSDF|NeuS` takes the synthetic scene's model
(scene.build_model, the one the tests and bench.py render) in place of --config / --load_pt."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    from nerfart_amd import config as cfg
    parser = cfg.create_args_parser()
    parser.add_argument("--mesh", type=str, required=True, help=".ply or .obj written by extract_mesh")
    parser.add_argument("--H", type=int, default=270)
    parser.add_argument("--W", type=int, default=480)
    parser.add_argument("--views", type=int, default=8, help="cameras on a circle around the origin")
    parser.add_argument("--cam_dist", type=float, default=2.5)
    parser.add_argument("--focal_scale", type=float, default=1.25, help="fx = fy = focal_scale * W")
    parser.add_argument("--near", type=float, default=1e-3)
    parser.add_argument("--out", type=str, default=None, help="directory for the PNG frames (none are written without it)")
    parser.add_argument("--load_pt", type=str, default=None, help="checkpoint for --compare; default: the initialisation")
    parser.add_argument("--compare", action="store_true", help="also render the cameras with surface_render and print the differences (needs --config "
                                                               "or --scene)")
    parser.add_argument("--scene", choices=["VolSDF", "NeuS"], default=None, help="--compare against the synthetic scene's model instead of --config")
    parser.add_argument("--N", type=int, default=512, help="grid points per axis the mesh was extracted with (--compare)")
    parser.add_argument("--volume_size", type=float, default=2.0, help="the cube the mesh was extracted from (--compare)")
    args, unknown = parser.parse_known_args(argv)
    return args, (cfg.load_config(args, unknown) if args.compare and args.scene is None else None)


def load_mesh(path, dev):
    """dict of GPU tensors / arrays for render_mesh: verts, faces and whichever of colors, uv + image, normals the file holds."""
    from nerfart_amd import mesh_util
    if path.endswith(".obj"):
        m = mesh_util.read_obj(path)
        out = {"uv": m["uv"], "image": torch.from_numpy(m["image"]).to(dev)}
    elif path.endswith(".ply"):
        m = mesh_util.read_ply(path)
        out = {"colors": None if m["colors"] is None else torch.from_numpy(m["colors"]).to(dev)}
    else:
        raise ValueError(f"--mesh must end in .ply or .obj (got {path!r})")
    out.update(verts=torch.from_numpy(m["verts"]).to(dev), faces=torch.from_numpy(m["faces"]).to(dev),
               normals=None if m["normals"] is None else torch.from_numpy(m["normals"]).to(dev))
    return out


def save_frames(out, k, rgb, depth, normals, mask, H, W):
    from PIL import Image
    to8 = lambda a: (a.clamp(0.0, 1.0) * 255.0 + 0.5).floor().to(torch.uint8).cpu().numpy()
    Image.fromarray(to8(rgb).reshape(H, W, 3)).save(os.path.join(out, f"rgb_{k:03d}.png"))
    shade = torch.zeros_like(depth)
    if bool(mask.any()):
        lo, hi = depth[mask].min(), depth[mask].max()
        shade[mask] = 1.0 - 0.9 * (depth[mask] - lo) / (hi - lo).clamp_min(1e-12)
    Image.fromarray(to8(shade).reshape(H, W)).save(os.path.join(out, f"depth_{k:03d}.png"))
    Image.fromarray(to8(torch.where(mask[:, None], 0.5 * normals + 0.5, torch.zeros_like(normals))).reshape(H, W, 3)).save(
        os.path.join(out, f"normal_{k:03d}.png"))


def compare_view(model, c2w, K, H, W, rgb, depth, mask, step, dev):
    """The figures of one view: the mesh frame against surface_render (sphere tracing) of the same camera."""
    from nerfart_amd import ray_casting, rend_util
    rays_o, rays_d, _ = rend_util.get_rays(c2w[None].to(dev), K[None].to(dev), H, W)
    rgb_s, depth_s, ex = ray_casting.surface_render(rays_o, rays_d, model, calc_normal=False, ray_casting_algo="sphere_tracing",
                                                    ray_casting_cfgs=dict(near=0.0, far=6.0, N_iters=20))
    mask_s = ex["mask_surface"].reshape(-1)
    both = mask & mask_s
    diff = ((depth - depth_s.reshape(-1)).abs()[both] / step).double().cpu().numpy()
    mse = float(((rgb - rgb_s.reshape(-1, 3)).double() ** 2).mean())
    q = lambda f: None if diff.size == 0 else round(float(f(diff)), 5)
    return {"both": int(both.sum()), "mesh_only": int((mask & ~mask_s).sum()), "field_only": int((~mask & mask_s).sum()),
            "depth_diff_steps_median": q(np.median), "depth_diff_steps_p99": q(lambda d: np.quantile(d, 0.99)), "depth_diff_steps_max": q(np.max),
            "psnr_rgb": None if mse == 0.0 else round(-10.0 * math.log10(mse), 3)}


def main():
    from nerfart_amd import mesh_util, scene
    args, conf = parse()
    assert torch.cuda.is_available(), "render_mesh needs the GPU (nerfart_amd has no CPU path)"
    dev = torch.device("cuda", conf.device_ids[0] if conf is not None else 0)
    mesh = load_mesh(args.mesh, dev)
    model = None
    if args.compare:
        if args.scene is not None:
            model = scene.build_model(args.scene, seed=0, beta=0.01 if args.scene == "VolSDF" else None, device=dev, precision="mixed")[0]
        else:
            from nerfart_amd import frameworks
            model = frameworks.get_model(conf)[0]
            if args.load_pt is not None:
                state = torch.load(args.load_pt, map_location="cpu")
                model.load_state_dict(state["model"] if "model" in state else state)
            model.to(dev)
        o = -args.volume_size / 2.0                                   # placement frame -> model frame: the two share the origin
        mesh["verts"] = (o + (mesh["verts"].double() - o) * (args.N / (args.N - 1.0))).float().contiguous()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    shading = {k: mesh[k] for k in ("colors", "uv", "image") if mesh.get(k) is not None}
    for k, angle in enumerate(scene.spiral(args.views, args.cam_dist)):
        c2w, K = scene.camera(args.H, args.W, cam_dist=args.cam_dist, focal_scale=args.focal_scale, angle=angle)
        rgb, depth, extras = mesh_util.render_mesh(mesh["verts"], mesh["faces"], c2w, K, args.H, args.W, normals=mesh["normals"], near=args.near, **shading)
        if args.out:
            save_frames(args.out, k, rgb, depth, extras["normals_mesh"], extras["mask_mesh"], args.H, args.W)
        line = {"view": k, "angle": round(angle, 6), "covered": int(extras["mask_mesh"].sum()), "n_skipped": extras["n_skipped"]}
        if model is not None:
            line.update(compare_view(model, c2w, K, args.H, args.W, rgb, depth, extras["mask_mesh"], args.volume_size / args.N, dev))
        print(json.dumps(line))


if __name__ == "__main__":
    main()
