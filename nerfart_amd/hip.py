"""ctypes binding of libnerfart_hip.so (include/nerfart_hip.h) for PyTorch-ROCm tensors.

PyTorch supplies device memory and the current HIP stream; every arithmetic step of the hot path
runs in the library.  If the library is missing this module raises at import - there is no
fallback path.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NERFART_HIP_LIB", os.path.join(_HERE, "csrc", "libnerfart_hip.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the gfx950 kernels first "
        f"(python -c 'import __graft_entry__ as g; g.build()'  or  python -m nerfart_amd.build). "
        f"nerfart_amd has no CPU / eager-PyTorch fallback.")

lib = C.CDLL(LIB_PATH)


def csrc_sha256() -> str:
    """SHA-256 over the kernel sources (csrc/*.hip, *.h, *.cpp, sorted by name): stamps profiles so that a bench line can say
    whether a committed PMC summary was taken on the code it runs."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h"))
                    + glob.glob(os.path.join(_HERE, "csrc", "*.cpp"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()

_p, _i, _f, _ll, _d = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_double
_SIGS = {
    "nerfart_abi_version": (_i, []),
    "nerfart_last_error": (C.c_char_p, []),
    "nerfart_linspace": (None, [_f, _f, _i, _p]),
    "nerfart_profile_begin": (_i, []),
    "nerfart_profile_end": (_i, [_p, _p, _p]),
    "nerfart_profile_end5": (_i, [_p, _p, _p]),
    "nerfart_sdf_fwd": (_i, [_p, _i, _p, _ll, _f, _p, _p]),
    "nerfart_sdf_fwd_rays": (_i, [_p, _i, _p, _p, _p, _p, _i, _i, _i, _f, _p, _i, _p]),
    "nerfart_sdf_nabla_workspace_bytes": (_ll, [_i]),
    "nerfart_sdf_nabla_fwd": (_i, [_p, _i, _p, _ll, _f, _p, _p, _p, _p, _ll, _p]),
    "nerfart_sdf_nabla_fwd_rays": (_i, [_p, _i, _p, _p, _p, _p, _i, _i, _i, _f, _p, _p, _p, _p, _ll, _p]),
    "nerfart_wgrad_workspace_bytes": (_ll, [_i, _ll, _i]),
    "nerfart_wgrad_bf16": (_i, [_p, _ll, _p, _ll, _i, _ll, _i, _ll, _p, _p, _i, _p, _ll, _p]),
    "nerfart_ray_points": (_i, [_p, _p, _p, _ll, _i, _p, _p, _p]),
    "nerfart_volsdf_pass2_cotangents": (_i, [_p, _p, _p, _p, _p, _p, _ll, _i, _f, _f, _ll, _p, _p, _p, _p]),
    "nerfart_wgrad_operand_embed_pair": (_i, [_p, _p, _ll, _ll, _i, _p, _p]),
    "nerfart_wgrad_operand_inputs": (_i, [_p, _i, _p, _i, _p, _ll, _ll, _p, _p]),
    "nerfart_wgrad_operand_rgb_delta": (_i, [_p, _p, _ll, _ll, _p, _p, _p, _p]),
    "nerfart_wgrad_operand_sbar_ones": (_i, [_p, _ll, _ll, _p, _p]),
    "nerfart_radiance_fwd": (_i, [_p, _i, _i, _p, _p, _ll, _p, _p, _p, _p]),
    "nerfart_radiance_fwd_rays": (_i, [_p, _i, _i, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "nerfart_get_rays": (_i, [_p, _p, _i, _i, _p, _i, _p, _p, _p]),
    "nerfart_normalize_dirs": (_i, [_p, _p, _i, _p]),
    "nerfart_linspace_depths": (_i, [_p, _i, _p, _p, _f, _f, _i, _p, _i, _p]),
    "nerfart_volsdf_first_check": (_i, [_i, _i, _i, _i, _f, _f, _f, _p, _p, _p, _i, _f, _p, _f, _p, _p, _p, _p, _p, _p, _p]),
    "nerfart_volsdf_upsample": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p, _i, _p, _p]),
    "nerfart_volsdf_merge_check": (_i, [_i, _i, _i, _i, _i, _i, _i, _f, _f, _f] + [_p] * 8 + [_i] + [_p] * 7),
    "nerfart_volsdf_finalize": (_i, [_i, _i, _i, _i] + [_p] * 4 + [_i] + [_p] * 5),
    "nerfart_volsdf_sampler_workspace_bytes": (_ll, [_i, _i, _i, _i, _i]),
    "nerfart_volsdf_fine_sample": (_i, [_p, _i, _p, _p, _i, _p, _p, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _p, _ll, _p]),
    "nerfart_volsdf_fine_sample_guarded": (_i, [_p, _i, _p, _i, _f, _p, _p, _i, _p, _p, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _p, _p, _ll, _p]),
    "nerfart_volsdf_fine_sample_guarded2": (_i, [_p, _i, _p, _i, _f, _i, _p, _p, _i, _p, _p, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _p, _p, _ll, _p]),
    "nerfart_sort_concat": (_i, [_i, _p, _i, _i, _p, _i, _i, _p, _i, _p]),
    "nerfart_volsdf_composite": (_i, [_i, _i, _p, _p, _p, _p, _f, _f, _i] + [_p] * 8),
    "nerfart_volsdf_composite_bwd": (_i, [_i, _i, _p, _p, _p, _f, _f, _i, _p, _p, _p, _p, _p, _p]),
    "nerfart_neus_composite_bwd": (_i, [_i, _i, _p, _p, _f, _i, _p, _p, _p, _p, _p, _p]),
    "nerfart_volsdf_composite_geo_bwd": (_i, [_i, _i, _p, _p, _p, _f, _f, _p, _p, _p, _i, _p, _p, _p, _p]),
    "nerfart_sdf_fwd2_dump_bytes": (_ll, [_ll]),
    "nerfart_sdf_bwd2_dump_bytes": (_ll, [_ll]),
    "nerfart_sdf_fwd2": (_i, [_p, _p, _p, _ll, _p, _p]),
    "nerfart_sdf_bwd2": (_i, [_p, _ll, _p, _p, _p, _p, _p]),
    "nerfart_radiance_dump_bytes": (_ll, [_ll]),
    "nerfart_radiance_fwd_dump": (_i, [_p, _i, _p, _p, _ll, _p, _p, _p, _p, _p]),
    "nerfart_radiance_bwd": (_i, [_p, _ll, _p, _p, _p, _p, _p, _p, _p]),
    "nerfart_volsdf_render_workspace_bytes": (_ll, [_i, _i, _i, _i, _i]),
    "nerfart_volsdf_render_fwd": (_i, [_p, _p, _i, _i, _p, _p, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i] + [_p] * 4 + [_i] + [_p] * 13 + [_p, _ll, _p]),
    "nerfart_volsdf_render_mixed_fwd": (_i, [_p, _p, _i, _p, _i, _i, _p, _p, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i] + [_p] * 4 + [_i] + [_p] * 13 + [_p, _ll, _p]),
    "nerfart_volsdf_render_staged_fwd": (_i, [_p, _i, _p, _i, _p, _i, _f, _i, _p, _p, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i] + [_p] * 4 + [_i] + [_p] * 13 + [_p, _p, _ll, _p]),
    "nerfart_volsdf_render_staged2_fwd": (_i, [_p, _i, _p, _i, _p, _i, _f, _i, _i, _p, _p, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i] + [_p] * 4 + [_i] + [_p] * 13 + [_p, _p, _ll, _p]),
    "nerfart_near_far_from_sphere": (_i, [_p, _p, _i, _f, _p, _p, _p]),
    "nerfart_neus_upsample_step": (_i, [_i, _i, _i, _i, _f, _p, _p, _p, _i, _p, _p]),
    "nerfart_merge_sorted_pairs": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p]),
    "nerfart_neus_composite": (_i, [_i, _i, _p, _p, _p, _p, _f, _i] + [_p] * 9),
    "nerfart_neus_render_workspace_bytes": (_ll, [_i, _i, _i, _i]),
    "nerfart_neus_render_fwd": (_i, [_p, _p, _i, _i, _p, _p, _i, _f, _f, _i, _i, _i, _i, _i] + [_p] * 2 + [_i] + [_p] * 12 + [_p, _ll, _p]),
    "nerfart_neus_direct_upsample_step": (_i, [_i, _i, _i, _i, _f, _p, _p, _p, _i, _p, _p]),
    "nerfart_neus_render_algo_workspace_bytes": (_ll, [_i, _i, _i, _i, _i, _i]),
    "nerfart_neus_render_algo_fwd": (_i, [_p, _p, _i, _i, _p, _p, _i, _f, _f, _i, _i, _i, _i, _i, _f, _i, _i] + [_p] * 3 + [_i] + [_p] * 12 + [_p, _ll, _p]),
    "nerfart_clip_vitb32_blob_layout": (_ll, [_p]),
    "nerfart_clip_vitb32_workspace_bytes": (_ll, [_i, _i]),
    "nerfart_clip_vitb32_image_fwd": (_i, [_p, _ll, _p, _i, _p, _i, _p, _ll, _p]),
    "nerfart_clip_vitb32_image_bwd": (_i, [_p, _ll, _i, _p, _p, _p, _ll, _p]),
    "nerfart_clip_vitb32_workspace_layout": (_ll, [_i, _i, _p]),
    "nerfart_clip_vitb32_image_bwd_partial": (_i, [_p, _ll, _i, _p, _p, _p, _ll, _i, _p]),
    "nerfart_gemm_f16_nt": (_i, [_p, _p, _i, _i, _i, _p, _p]),
    "nerfart_gemm_f16_nn": (_i, [_p, _p, _i, _i, _i, _p, _p]),
    "nerfart_vgg16_blob_layout": (_ll, [_p]),
    "nerfart_vgg16_workspace_bytes": (_ll, [_i, _i, _i]),
    "nerfart_vgg16_workspace_layout": (_ll, [_i, _i, _i, _p]),
    "nerfart_vgg16_l1_fwd": (_i, [_p, _ll, _p, _i, _i, _p, _i, _p, _ll, _p]),
    "nerfart_vgg16_l1_bwd": (_i, [_p, _ll, _i, _i, _p, _p, _p, _ll, _p]),
    "nerfart_first_crossing": (_i, [_p, _p, _i, _i, _f, _p, _p, _p, _p, _p, _p]),
    "nerfart_secant_update": (_i, [_p, _i, _f, _p, _p, _p, _p]),
    "nerfart_root_finish": (_i, [_p, _p, _i, _p, _p, _p, _p, _f, _i, _p, _p, _p]),
    "nerfart_sphere_trace_step": (_i, [_p, _i, _p, _f, _p, _p, _p]),
    "nerfart_resample_fwd": (_i, [_p] + [_i] * 11 + [_p, _p, _p, _p, _i, _i, _i, _p]),
    "nerfart_resample_bwd": (_i, [_p] + [_i] * 11 + [_p, _p, _p, _p, _i, _i, _i, _p]),
    "nerfart_clip_style_heads": (_i, [_p, _i, _p, _p, _p, _p, _i, _i, _f, _f, _f, _f, _f, _p, _p, _p]),
    "nerfart_pass2_raw_layout": (_ll, [_p]),
    "nerfart_volsdf_render_bwd_workspace_bytes": (_ll, [_i, _i, _i]),
    "nerfart_volsdf_render_bwd": (_i, [_p, _p, _i, _i, _p, _p, _i, _i] + [_p] * 7 + [_f, _f, _f, _i, _f, _i, _i, _p, _p, _ll, _p]),
    "nerfart_volsdf_render_bwd2_workspace_bytes": (_ll, [_i, _i, _i, _i]),
    "nerfart_volsdf_render_bwd2": (_i, [_p, _p, _i, _i, _p, _p, _i, _i] + [_p] * 9 + [_f, _f, _f, _i, _f, _i, _i, _p, _p, _ll, _p]),
    "nerfart_neus_render_bwd_workspace_bytes": (_ll, [_i, _i, _i]),
    "nerfart_neus_render_bwd": (_i, [_p, _p, _i, _i, _p, _p, _i, _i] + [_p] * 5 + [_f, _i, _f, _i, _i, _p, _p, _ll, _p]),
    "nerfart_sdf_param_bwd_workspace_bytes": (_ll, [_ll]),
    "nerfart_sdf_param_bwd": (_i, [_p, _i, _p, _ll, _p, _p, _p, _p, _p, _ll, _p]),
    "nerfart_radiance_param_bwd_workspace_bytes": (_ll, [_ll]),
    "nerfart_radiance_param_bwd": (_i, [_p, _i, _p, _p, _p, _p, _ll, _p, _p, _p, _p, _i, _p, _p, _ll, _p]),
    "nerfart_folded_grads_layout": (_ll, [_i, _i, _p]),
    "nerfart_fold_weight_grads": (_i, [_p, _i, _i, _p, _p]),
    "nerfart_weight_norm_bwd": (_i, [_p, _p, _p, _i, _i, _p, _p, _i, _p]),
    "nerfart_surface_blob_floats": (_ll, [_i, _i]),
    "nerfart_radiance_blob_floats": (_ll, [_i, _i]),
    "nerfart_pack_workspace_bytes": (_ll, []),
    "nerfart_pack_layer_dims": (_i, [_i, _i, _p, _p]),
    "nerfart_geometry_feature_workspace_bytes": (_ll, []),
    "nerfart_geometry_feature": (_i, [_p, _p, _p, _p, _ll, _p, _p, _ll, _p]),
    "nerfart_mc_workspace_bytes": (_ll, [_i, _i, _i]),
    "nerfart_mc_count": (_i, [_p, _i, _i, _i, _f, _p, _ll, _p, _p]),
    "nerfart_mc_emit": (_i, [_p, _i, _i, _i, _f, _p, _p, _p, _ll, _p, _p, _i, _i, _p]),
    "nerfart_mc_emit_edges": (_i, [_p, _i, _i, _i, _f, _p, _ll, _p, _p, _p, _p, _p, _i, _p]),
    "nerfart_mesh_edge_points": (_i, [_p, _p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "nerfart_mesh_edge_refine_step": (_i, [_p, _f, _i, _p, _p, _p, _p, _p]),
    "nerfart_mesh_components": (_i, [_p, _i, _i, _p, _p, _p, _p]),
    "nerfart_mesh_compact_workspace_bytes": (_ll, [_i, _i]),
    "nerfart_mesh_compact_count": (_i, [_p, _p, _p, _i, _i, _p, _ll, _p, _p]),
    "nerfart_mesh_compact_emit": (_i, [_p, _p, _p, _i, _i, _p, _ll, _p, _p, _i, _i, _p]),
    "nerfart_mesh_topology_workspace_bytes": (_ll, [_i, _i, _i]),
    "nerfart_mesh_half_edges": (_i, [_p, _i, _i, _i, _p, _ll, _p, _p, _p, _p, _p]),
    "nerfart_mesh_component_stats": (_i, [_p, _p, _i, _i, _p, _p, _ll, _p, _p, _p]),
    "nerfart_mesh_repair_workspace_bytes": (_ll, [_i, _i, _i]),
    "nerfart_mesh_repair_count": (_i, [_p, _p, _i, _i, _i, _i, _p, _ll, _p, _p, _p]),
    "nerfart_mesh_repair_emit": (_i, [_p, _p, _i, _i, _i, _p, _ll, _p, _p, _p, _p, _i, _i, _i, _p]),
    "nerfart_mesh_simplify_workspace_bytes": (_ll, [_i, _i, _i, _i, _i, _i]),
    "nerfart_mesh_simplify_count": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _ll, _p, _p, _p]),
    "nerfart_mesh_simplify_emit": (_i, [_p, _i, _i, _i, _i, _i, _i, _d, _p, _ll, _p, _p, _p, _i, _i, _p]),
    "nerfart_mesh_atlas_layout": (_i, [_ll, _ll, _p]),
    "nerfart_mesh_atlas_points": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "nerfart_mesh_project_step": (_i, [_p, _p, _p, _i, _f, _f, _p]),
    "nerfart_mesh_project": (_i, [_p, _i, _p, _p, _f, _p, _p, _p, _p]),
    "nerfart_mesh_raster": (_i, [_p, _p, _p, _p, _i, _i, _p, _f, _i, _i, _p, _p, _p, _p]),
    "nerfart_mesh_resolve": (_i, [_p, _p, _p, _i, _i, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "nerfart_mesh_interp": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _f, _p, _p]),
    "nerfart_mesh_sample_bilinear": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _p]),
    "nerfart_mesh_sample_workspace_bytes": (_ll, [_i]),
    "nerfart_mesh_sample_count": (_i, [_p, _p, _i, _i, _d, _i, _p, _ll, _p, _p]),
    "nerfart_mesh_sample_emit": (_i, [_p, _p, _i, _i, _i, _p, _ll, _p, _p, _i, _p]),
    "nerfart_mesh_grid_workspace_bytes": (_ll, [_i, _i, _i]),
    "nerfart_mesh_grid_count": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _ll, _p, _p]),
    "nerfart_mesh_grid_fill": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _ll, _p, _ll, _p]),
    "nerfart_mesh_closest": (_i, [_p, _i, _p, _p, _i, _i, _i, _i, _i, _p, _ll, _p, _ll, _d, _p, _p, _p, _p]),
    "nerfart_band_workspace_bytes": (_ll, [_i, _i]),
    "nerfart_band_probe_points": (_i, [_i, _i, _d, _d, _p, _p]),
    "nerfart_band_select": (_i, [_i, _p, _f, _f, _i, _i, _p, _p, _p, _p, _p, _ll, _p, _p]),
    "nerfart_band_brick_points": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _d, _d, _p, _p, _p]),
    "nerfart_band_scatter": (_i, [_p, _p, _i, _i, _p, _p]),
    "nerfart_band_fill": (_i, [_p, _p, _i, _i, _p, _p]),
    "nerfart_band_check": (_i, [_p, _f, _p, _i, _i, _p, _p, _p]),
    "nerfart_pack_surface_blob": (_i, [_i, _i, _p, _p, _p, _p, _ll, _p, _ll, _p]),
    "nerfart_pack_radiance_blob": (_i, [_i, _i, _p, _p, _p, _p, _p, _p, _p, _ll, _p, _ll, _p]),
    "nerfart_pack_plan_debug": (_i, [_i, _i, _i] + [_p] * 6),
    "nerfart_clip_vitb32_n_tensors": (_i, []),
    "nerfart_clip_vitb32_tensor_name": (_ll, [_i, _p, _i]),
    "nerfart_clip_vitb32_pack": (_i, [_p, _p, _ll, _p]),
    "nerfart_vgg16_pack": (_i, [_p, _p, _p, _ll, _p]),
}
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)          # AttributeError here = header / library mismatch
    _fn.restype, _fn.argtypes = _res, _args

ABI_VERSION = lib.nerfart_abi_version()


class NerfartHipError(RuntimeError):
    pass


def _check(rc: int, what: str):
    if rc != 0:
        raise NerfartHipError(f"{what} failed (code {rc}): {lib.nerfart_last_error().decode(errors='replace')}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, dtype=torch.float32, name="tensor") -> int:
    if t is None:
        return None
    if not t.is_cuda:
        raise NerfartHipError(f"{name} must live on the GPU (got {t.device}); nerfart_amd has no CPU path")
    if t.dtype != dtype:
        raise NerfartHipError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise NerfartHipError(f"{name} must be contiguous")
    return t.data_ptr()


def _ptr_table(tensors, name):
    """HOST array of device pointers (what the pack entry points take for per-layer tensors)."""
    return (C.c_void_p * len(tensors))(*[_dev(t, name=f"{name}[{i}]") for i, t in enumerate(tensors)])


def pack_layer_dims(radiance: bool, arg: int):
    """[(rows, cols)] of the weight_v tensors the packers expect (nerfart_pack_layer_dims): the SDF net for embed_multires = arg, or the
    radiance net for view_tiles = arg."""
    rows, cols = (C.c_int * 9)(), (C.c_int * 9)()
    n = int(lib.nerfart_pack_layer_dims(int(bool(radiance)), int(arg), rows, cols))
    if n <= 0:
        raise NotImplementedError(f"nerfart_pack_layer_dims: {lib.nerfart_last_error().decode(errors='replace')}")
    return [(int(rows[l]), int(cols[l])) for l in range(n)]


def check_layers(what: str, dims, weight_g, weight_v, bias):
    """The pack entry points index HOST pointer tables and DEVICE tensors with the fixed dims of the architecture the kernels are written for:
    refuse anything else here (NotImplementedError, as the reference-config guard of the packing plans did) instead of reading out of bounds."""
    if not (len(weight_g) == len(weight_v) == len(bias) == len(dims)):
        raise NotImplementedError(f"{what}: the kernels are written for {len(dims)} layers (got {len(weight_g)} / {len(weight_v)} / {len(bias)} "
                                  f"weight_g / weight_v / bias tensors) - SURVEY.md 2: the four shipped configs")
    for l, (r, c) in enumerate(dims):
        if tuple(weight_v[l].shape) != (r, c) or weight_g[l].numel() != r or tuple(bias[l].shape) != (r,):
            raise NotImplementedError(f"{what}: layer {l} must be weight_v [{r}, {c}], weight_g [{r}, 1], bias [{r}] (got {tuple(weight_v[l].shape)}, "
                                      f"{tuple(weight_g[l].shape)}, {tuple(bias[l].shape)}): W 256, D 8, skips [4], embed_multires 6, W_geo_feat 256 / "
                                      f"radiance W 256, D 4 are the architectures the kernels are written for")


def pack_surface_blob(precision: int, multires: int, weight_g, weight_v, bias) -> torch.Tensor:
    """nerfart_pack_surface_blob: the SDF net's blob for C-ABI `precision` (0 fp32, 1 split bf16, 4 fp16 hi + lo) from the state dict's
    per-layer weight_g [out, 1] / weight_v [out, in] / bias [out] (9 layers) - weight_norm fold, unit-order permutation and hi / lo split on
    the device.  The returned tensor carries `.nerfart_term` ('fp32' | 'bf16' | 'fp16') for the wrappers of entry points that read one encoding only."""
    check_layers("pack_surface_blob", pack_layer_dims(False, multires), weight_g, weight_v, bias)
    dev = weight_v[0].device
    n = int(lib.nerfart_surface_blob_floats(int(precision), int(multires)))
    if n <= 0:
        raise NerfartHipError(f"nerfart_surface_blob_floats: {lib.nerfart_last_error().decode(errors='replace')}")
    blob = torch.empty(n, dtype=torch.float32, device=dev)
    ws = _workspace(int(lib.nerfart_pack_workspace_bytes()), dev)
    g = [t.detach().reshape(-1).contiguous() for t in weight_g]
    v = [t.detach().contiguous() for t in weight_v]
    b = [t.detach().contiguous() for t in bias]
    _check(lib.nerfart_pack_surface_blob(int(precision), int(multires), _ptr_table(g, "weight_g"), _ptr_table(v, "weight_v"), _ptr_table(b, "bias"),
                                         _dev(blob), n, ws.data_ptr(), ws.numel(), _stream()), "nerfart_pack_surface_blob")
    blob.nerfart_term = {0: "fp32", 1: "bf16", 4: "fp16", 5: "fp16 (softplus-scaled, precision 5)"}[int(precision)]
    return blob


def pack_radiance_blob(precision: int, view_tiles: int, surf8, weight_g, weight_v, bias) -> torch.Tensor:
    """nerfart_pack_radiance_blob: surf8 = (weight_g, weight_v, bias) of the SDF net's last layer (its rows 1.. make the geometry feature),
    then the 5 radiance layers' tensors."""
    check_layers("pack_radiance_blob", pack_layer_dims(True, view_tiles), weight_g, weight_v, bias)
    check_layers("pack_radiance_blob (the SDF net's last layer)", pack_layer_dims(False, 6)[8:], [surf8[0]], [surf8[1]], [surf8[2]])
    dev = weight_v[0].device
    n = int(lib.nerfart_radiance_blob_floats(int(precision), int(view_tiles)))
    if n <= 0:
        raise NerfartHipError(f"nerfart_radiance_blob_floats: {lib.nerfart_last_error().decode(errors='replace')}")
    blob = torch.empty(n, dtype=torch.float32, device=dev)
    ws = _workspace(int(lib.nerfart_pack_workspace_bytes()), dev)
    s8 = [surf8[0].detach().reshape(-1).contiguous(), surf8[1].detach().contiguous(), surf8[2].detach().contiguous()]
    g = [t.detach().reshape(-1).contiguous() for t in weight_g]
    v = [t.detach().contiguous() for t in weight_v]
    b = [t.detach().contiguous() for t in bias]
    _check(lib.nerfart_pack_radiance_blob(int(precision), int(view_tiles), _dev(s8[0], name="surf8_g"), _dev(s8[1], name="surf8_v"), _dev(s8[2], name="surf8_bias"),
                                          _ptr_table(g, "weight_g"), _ptr_table(v, "weight_v"), _ptr_table(b, "bias"), _dev(blob), n, ws.data_ptr(), ws.numel(),
                                          _stream()), "nerfart_pack_radiance_blob")
    blob.nerfart_term = {0: "fp32", 1: "bf16", 4: "fp16"}[int(precision)]
    return blob


def need_term(blob, term: str, who: str):
    """Entry points that read ONE fragment encoding (the training kernels: split bf16) refuse a blob packed for another - the sizes and the
    program id of a bf16 and an fp16 blob coincide, only header word 10 differs."""
    have = getattr(blob, "nerfart_term", None)
    if have is not None and have != term:
        raise NerfartHipError(f"{who} reads {term} blobs; this blob was packed as {have}")


def linspace(start: float, end: float, n: int) -> torch.Tensor:
    """Host helper: the library's restatement of torch.linspace (used for its own tables)."""
    out = torch.empty(n, dtype=torch.float32)
    lib.nerfart_linspace(start, end, n, out.data_ptr())
    return out


def profile_begin():
    lib.nerfart_profile_begin()


def profile_end():
    """-> {kernel: (ms, launches, units)} for the chained-MLP kernels (units = points) and k_wgrad<256> (units = algorithmic bytes)
    launched since profile_begin(); k_sdf_only_escalation: the SDF queries of the guarded sampler's second run (the re-sampled rays, at the
    escalation precision) - kept apart from k_sdf_only, the dominant kernel's own launches."""
    ms = (C.c_double * 5)(); ln = (C.c_longlong * 5)(); un = (C.c_longlong * 5)()
    lib.nerfart_profile_end5(ms, ln, un)
    return {k: (ms[i], ln[i], un[i]) for i, k in enumerate(("k_sdf_only", "k_sdf_nabla", "k_radiance", "k_wgrad256", "k_sdf_only_escalation"))}


# ---- point queries -----------------------------------------------------------------------
PRECISIONS = {"fp32": 0, "bf16x3": 1, "fp16x2": 4}      # 4: the 2-MFMA kernels: the sampler of the shipped "mixed" mode (nets.set_precision); everywhere: a measurement variant
# Precisions that exist for Algorithm 1's no-gradient SDF queries ONLY (nerfart_sdf_fwd[_rays] and the sampler stage of the renderers refuse them
# nowhere else): 5 = "fp16x1", one MFMA per product on the precision-4 blob (csrc/mlp_chain_f16x1.hip).
SAMPLER_PRECISIONS = dict(PRECISIONS, fp16x1=5, fp16x1c=5)     # fp16x1c: the same kernel on error-compensated one-term weights (nerfart_amd/calibrate.py)


def sdf_fwd(surf_blob, pts, R_bg: float, precision: int = 0):
    M = pts.shape[0]
    out = torch.empty(M, dtype=torch.float32, device=pts.device)
    _check(lib.nerfart_sdf_fwd(_dev(surf_blob, name="surf_blob"), int(precision), _dev(pts, name="pts"), M, float(R_bg), _dev(out), _stream()),
           "nerfart_sdf_fwd")
    return out


def sdf_nabla_fwd(surf_blob, pts, R_bg: float, want_h7: bool = True, precision: int = 0):
    M = pts.shape[0]
    sdf = torch.empty(M, dtype=torch.float32, device=pts.device)
    nab = torch.empty(M, 3, dtype=torch.float32, device=pts.device)
    h7 = torch.empty(M, 256, dtype=torch.float32, device=pts.device) if want_h7 else None
    ws, nb = nabla_workspace(precision, pts.device)
    _check(lib.nerfart_sdf_nabla_fwd(_dev(surf_blob), int(precision), _dev(pts, name="pts"), M, float(R_bg), _dev(sdf), _dev(nab),
                                     _dev(h7), _dev(ws, torch.uint8), nb, _stream()), "nerfart_sdf_nabla_fwd")
    return sdf, nab, h7


def geometry_feature(weight_g, weight_v, bias, h7):
    """feat [M, 256] = W8[1:] h7 + b8[1:] (nerfart_geometry_feature: the SDF net's last layer's feature rows, weight_norm folded on the device)."""
    M = h7.shape[0]
    out = torch.empty(M, 256, dtype=torch.float32, device=h7.device)
    ws = _workspace(int(lib.nerfart_geometry_feature_workspace_bytes()), h7.device)
    _check(lib.nerfart_geometry_feature(_dev(weight_g.detach().reshape(-1).contiguous(), name="weight_g"), _dev(weight_v.detach().contiguous(), name="weight_v"),
                                        _dev(bias.detach().contiguous(), name="bias"), _dev(h7, name="h7"), M, _dev(out), ws.data_ptr(), ws.numel(), _stream()),
           "nerfart_geometry_feature")
    return out


def _mc_volume(vol):
    if vol.dim() != 3:
        raise NerfartHipError(f"the volume must be [nx, ny, nz] (got {tuple(vol.shape)})")
    return _dev(vol, name="vol"), [int(d) for d in vol.shape]


def mc_workspace_bytes(nx: int, ny: int, nz: int) -> int:
    """nerfart_mc_workspace_bytes; bad dimensions (one below 2, 3 nx ny nz >= 2^31) raise with the library's message."""
    n = int(lib.nerfart_mc_workspace_bytes(nx, ny, nz))
    _check(0 if n else 2, "nerfart_mc_workspace_bytes")
    return n


def mc_count(vol, level: float, ws=None):
    """nerfart_mc_count on vol [nx, ny, nz]: (ws, counts) - the filled workspace (uint8; a caller's own, or a fresh one: it must stay untouched until
    mc_emit has run) and the int32 device tensor counts [3] = (vertices, triangles, non-finite flag).  No host synchronisation."""
    ptr, dims = _mc_volume(vol)
    if ws is None:
        ws = torch.empty(mc_workspace_bytes(*dims), dtype=torch.uint8, device=vol.device)
    counts = torch.empty(3, dtype=torch.int32, device=vol.device)
    _check(lib.nerfart_mc_count(ptr, *dims, float(level), _dev(ws, torch.uint8, "ws"), ws.numel(), counts.data_ptr(), _stream()), "nerfart_mc_count")
    return ws, counts


def mc_emit(vol, level: float, origin, spacing, ws, V: int, F: int):
    """nerfart_mc_emit: (verts [V, 3] float32, faces [F, 3] int32) from the workspace mc_count filled for the same volume and level."""
    ptr, dims = _mc_volume(vol)
    verts = torch.empty(V, 3, dtype=torch.float32, device=vol.device)
    faces = torch.empty(F, 3, dtype=torch.int32, device=vol.device)
    o, s = (C.c_float * 3)(*[float(x) for x in origin]), (C.c_float * 3)(*[float(x) for x in spacing])
    _check(lib.nerfart_mc_emit(ptr, *dims, float(level), C.cast(o, C.c_void_p), C.cast(s, C.c_void_p), _dev(ws, torch.uint8, "ws"), ws.numel(),
                               verts.data_ptr(), faces.data_ptr(), V, F, _stream()), "nerfart_mc_emit")
    return verts, faces


def mc_emit_edges(vol, level: float, ws, V: int):
    """nerfart_mc_emit_edges: the edge records of mc_emit's V vertices, in its order, from the same untouched workspace -
    (edge [V] int32 holding the uint32 3 p + axis, bracket [V, 4], t [V], best [V, 2], side [V] uint8): the initial state of mesh_edge_refine_step."""
    ptr, dims = _mc_volume(vol)
    dev = vol.device
    edge = torch.empty(V, dtype=torch.int32, device=dev)
    bracket, t, best = (torch.empty(V, 4, dtype=torch.float32, device=dev), torch.empty(V, dtype=torch.float32, device=dev),
                        torch.empty(V, 2, dtype=torch.float32, device=dev))
    side = torch.empty(V, dtype=torch.uint8, device=dev)
    _check(lib.nerfart_mc_emit_edges(ptr, *dims, float(level), _dev(ws, torch.uint8, "ws"), ws.numel(), edge.data_ptr(), bracket.data_ptr(), t.data_ptr(),
                                     best.data_ptr(), side.data_ptr(), V, _stream()), "nerfart_mc_emit_edges")
    return edge, bracket, t, best, side


def mesh_edge_points(edge, t, dims, origin, spacing, out=None):
    """nerfart_mesh_edge_points: pts [V, 3] float32 = the vertices at parameter t [V] on their grid edges edge [V] (int32) of a volume of
    dims = (nx, ny, nz), in the frame origin / spacing - mc_emit's arithmetic.  out: a caller's [V, 3] buffer (a vertex whose edge is not one of
    the volume's keeps its row), else a fresh, zeroed one."""
    V = edge.shape[0]
    if t.shape != (V,):
        raise NerfartHipError(f"t must be [{V}] (got {tuple(t.shape)})")
    if out is None:
        out = torch.zeros(V, 3, dtype=torch.float32, device=edge.device)
    elif tuple(out.shape) != (V, 3):
        raise NerfartHipError(f"out must be [{V}, 3] (got {tuple(out.shape)})")
    o, s = (C.c_float * 3)(*[float(x) for x in origin]), (C.c_float * 3)(*[float(x) for x in spacing])
    nx, ny, nz = (int(d) for d in dims)
    _check(lib.nerfart_mesh_edge_points(_dev(edge, torch.int32, "edge"), _dev(t, name="t"), V, nx, ny, nz, C.cast(o, C.c_void_p), C.cast(s, C.c_void_p),
                                        _dev(out, name="out"), _stream()), "nerfart_mesh_edge_points")
    return out


def mesh_edge_refine_step(f, level: float, bracket, t, best, side):
    """nerfart_mesh_edge_refine_step, in place on (bracket [V, 4], t [V], best [V, 2], side [V] uint8): one step of bracket-keeping false position
    (Illinois) given f [V] = the SDF at the points of the current t."""
    V = t.shape[0]
    if f.shape != (V,) or tuple(bracket.shape) != (V, 4) or tuple(best.shape) != (V, 2) or side.shape != (V,):
        raise NerfartHipError(f"mesh_edge_refine_step: f [{V}], bracket [{V}, 4], best [{V}, 2], side [{V}] expected "
                              f"(got {tuple(f.shape)}, {tuple(bracket.shape)}, {tuple(best.shape)}, {tuple(side.shape)})")
    _check(lib.nerfart_mesh_edge_refine_step(_dev(f, name="f"), float(level), V, _dev(bracket, name="bracket"), _dev(t, name="t"), _dev(best, name="best"),
                                             _dev(side, torch.uint8, "side"), _stream()), "nerfart_mesh_edge_refine_step")


def _mesh_faces(faces, V: int):
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise NerfartHipError(f"faces must be [F, 3] (got {tuple(faces.shape)})")
    if V < 0:
        raise NerfartHipError(f"the vertex count must be >= 0 (got {V})")
    return _dev(faces, torch.int32, "faces"), int(faces.shape[0])


def mesh_components(faces, V: int):
    """nerfart_mesh_components on faces [F, 3] (int32) over V vertices: (label [V] int32 - the smallest vertex index of the vertex's component -,
    n_faces [V] int32 - at a label the component's face count, 0 elsewhere -, info [3] int32 = (components, components with a face, 1 if a face
    holds an index outside [0, V))), all on faces' device.  No host synchronisation."""
    V = int(V)
    ptr, F = _mesh_faces(faces, V)
    label = torch.empty(V, dtype=torch.int32, device=faces.device)
    n_faces = torch.empty(V, dtype=torch.int32, device=faces.device)
    info = torch.empty(3, dtype=torch.int32, device=faces.device)
    _check(lib.nerfart_mesh_components(ptr, F, V, label.data_ptr(), n_faces.data_ptr(), _dev(info, torch.int32, "info"), _stream()),
           "nerfart_mesh_components")
    return label, n_faces, info


def mesh_compact_workspace_bytes(V: int, F: int) -> int:
    """nerfart_mesh_compact_workspace_bytes; bad sizes (V or F >= 2^31, 3 F >= 2^32) raise with the library's message."""
    n = int(lib.nerfart_mesh_compact_workspace_bytes(V, F))
    _check(0 if n else 2, "nerfart_mesh_compact_workspace_bytes")
    return n


def _mesh_compact_args(label, keep, faces, V: int):
    V = int(V)
    ptr, F = _mesh_faces(faces, V)
    if label.shape != (V,) or keep.shape != (V,):
        raise NerfartHipError(f"label and keep must be [{V}] (got {tuple(label.shape)}, {tuple(keep.shape)})")
    return _dev(label, torch.int32, "label"), _dev(keep, torch.uint8, "keep"), ptr, V, F


def mesh_compact_count(label, keep, faces, V: int, ws=None):
    """nerfart_mesh_compact_count: (ws, counts) - the filled workspace (uint8; a caller's own, or a fresh one: it must stay untouched until
    mesh_compact_emit has run) and the int32 device tensor counts [2] = (surviving vertices, surviving faces).  keep [V] uint8 is indexed by
    label.  No host synchronisation."""
    lp, kp, fp, V, F = _mesh_compact_args(label, keep, faces, V)
    if ws is None:
        ws = torch.empty(mesh_compact_workspace_bytes(V, F), dtype=torch.uint8, device=faces.device)
    counts = torch.empty(2, dtype=torch.int32, device=faces.device)
    _check(lib.nerfart_mesh_compact_count(lp, kp, fp, V, F, _dev(ws, torch.uint8, "ws"), ws.numel(), counts.data_ptr(), _stream()),
           "nerfart_mesh_compact_count")
    return ws, counts


def mesh_compact_emit(label, keep, faces, V: int, ws, V_out: int, F_out: int):
    """nerfart_mesh_compact_emit: (src_vertex [V_out] int32 - the old indices of the surviving vertices, ascending -, faces_out [F_out, 3] int32 -
    the surviving faces in their old order, renumbered) from the workspace mesh_compact_count filled for the same arrays."""
    lp, kp, fp, V, F = _mesh_compact_args(label, keep, faces, V)
    src = torch.empty(int(V_out), dtype=torch.int32, device=faces.device)
    out = torch.empty(int(F_out), 3, dtype=torch.int32, device=faces.device)
    _check(lib.nerfart_mesh_compact_emit(lp, kp, fp, V, F, _dev(ws, torch.uint8, "ws"), ws.numel(), src.data_ptr(), out.data_ptr(), int(V_out), int(F_out),
                                         _stream()), "nerfart_mesh_compact_emit")
    return src, out


def mesh_compact(label, keep, faces, V: int):
    """mesh_compact_count, ONE host read (the two sizes), mesh_compact_emit: (src_vertex [V'], faces_out [F', 3])."""
    ws, counts = mesh_compact_count(label, keep, faces, V)
    V_out, F_out = (int(c) for c in counts.cpu())
    return mesh_compact_emit(label, keep, faces, V, ws, V_out, F_out)


def mesh_topology_workspace_bytes(V: int, F: int, table_log2: int = 0) -> int:
    """nerfart_mesh_topology_workspace_bytes for an edge table of 2^table_log2 slots (0: the default, load factor below 1/4); bad sizes
    (V or F >= 2^31, 3 F >= 2^32, a table of fewer than 3 F + 1 slots) raise with the library's message."""
    n = int(lib.nerfart_mesh_topology_workspace_bytes(int(V), int(F), int(table_log2)))
    _check(0 if n else 2, "nerfart_mesh_topology_workspace_bytes")
    return n


def mesh_half_edges(faces, V: int, table_log2: int = 0, ws=None):
    """nerfart_mesh_half_edges on faces [F, 3] (int32) over V vertices: (ws, twin [3 F] int32, edge_uses [3 F] int32, vertex_fans [V] int32,
    info [16] int32 - include/nerfart_hip.h names every index), all on faces' device.  ws is the filled workspace (uint8; a caller's own, or a
    fresh one): it keeps the edge table and must stay untouched until mesh_component_stats has run.  No host synchronisation."""
    V = int(V)
    ptr, F = _mesh_faces(faces, V)
    if ws is None:
        ws = torch.empty(mesh_topology_workspace_bytes(V, F, table_log2), dtype=torch.uint8, device=faces.device)
    twin = torch.empty(3 * F, dtype=torch.int32, device=faces.device)
    uses = torch.empty(3 * F, dtype=torch.int32, device=faces.device)
    fans = torch.empty(V, dtype=torch.int32, device=faces.device)
    info = torch.empty(16, dtype=torch.int32, device=faces.device)
    _check(lib.nerfart_mesh_half_edges(ptr, F, V, int(table_log2), _dev(ws, torch.uint8, "ws"), ws.numel(), twin.data_ptr(), uses.data_ptr(),
                                       fans.data_ptr(), info.data_ptr(), _stream()), "nerfart_mesh_half_edges")
    return ws, twin, uses, fans, info


def mesh_component_stats(verts, faces, label, ws):
    """nerfart_mesh_component_stats from the workspace mesh_half_edges filled for the same faces and the label [V] of mesh_components:
    (counts [V, 6] int32 - by label: referenced vertices, edges, proper faces, boundary, flipped and non-manifold edges -, measure [V, 2]
    float64 - by label: area, signed volume).  No host synchronisation."""
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise NerfartHipError(f"verts must be [V, 3] (got {tuple(verts.shape)})")
    V = int(verts.shape[0])
    fp, F = _mesh_faces(faces, V)
    if label.shape != (V,):
        raise NerfartHipError(f"label must be [{V}] (got {tuple(label.shape)})")
    counts = torch.empty(V, 6, dtype=torch.int32, device=faces.device)
    measure = torch.empty(V, 2, dtype=torch.float64, device=faces.device)
    _check(lib.nerfart_mesh_component_stats(_dev(verts, torch.float32, "verts"), fp, F, V, _dev(label, torch.int32, "label"),
                                            _dev(ws, torch.uint8, "ws"), ws.numel(), counts.data_ptr(), measure.data_ptr(), _stream()),
           "nerfart_mesh_component_stats")
    return counts, measure


MESH_REPAIR_WEDGES = ("void", "solid")      # nerfart_mesh_repair_count's wedge = the index


def mesh_repair_workspace_bytes(V: int, F: int, table_log2: int = 0) -> int:
    """nerfart_mesh_repair_workspace_bytes for an edge table of 2^table_log2 slots (0: the default); bad sizes (V or F >= 2^31, 3 F >= 2^32, a
    table of fewer than 3 F + 1 slots) raise with the library's message."""
    n = int(lib.nerfart_mesh_repair_workspace_bytes(int(V), int(F), int(table_log2)))
    _check(0 if n else 2, "nerfart_mesh_repair_workspace_bytes")
    return n


def _mesh_repair_args(verts, faces):
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise NerfartHipError(f"verts must be [V, 3] (got {tuple(verts.shape)})")
    V = int(verts.shape[0])
    fp, F = _mesh_faces(faces, V)
    return _dev(verts, torch.float32, "verts"), fp, V, F


def mesh_repair_count(verts, faces, wedge: str = "void", table_log2: int = 0, ws=None):
    """nerfart_mesh_repair_count on verts [V, 3] float32 and faces [F, 3] int32: (ws, counts, info) - the filled workspace (uint8; a caller's
    own, or a fresh one: it must stay untouched until mesh_repair_emit has run), the int32 device tensors counts [4] = (class vertices V1,
    midpoints M, surviving faces, appended faces) and info [16] (include/nerfart_hip.h names every index).  No host synchronisation."""
    if wedge not in MESH_REPAIR_WEDGES:
        raise NerfartHipError(f"wedge must be one of {MESH_REPAIR_WEDGES} (got {wedge!r})")
    vp, fp, V, F = _mesh_repair_args(verts, faces)
    if ws is None:
        ws = torch.empty(mesh_repair_workspace_bytes(V, F, table_log2), dtype=torch.uint8, device=faces.device)
    counts = torch.empty(4, dtype=torch.int32, device=faces.device)
    info = torch.empty(16, dtype=torch.int32, device=faces.device)
    _check(lib.nerfart_mesh_repair_count(vp, fp, V, F, MESH_REPAIR_WEDGES.index(wedge), int(table_log2), _dev(ws, torch.uint8, "ws"), ws.numel(),
                                         counts.data_ptr(), info.data_ptr(), _stream()), "nerfart_mesh_repair_count")
    return ws, counts, info


def mesh_repair_emit(verts, faces, ws, V1: int, M: int, F_out: int, table_log2: int = 0):
    """nerfart_mesh_repair_emit from the workspace mesh_repair_count filled for the same mesh (and the same table_log2): (verts' [V1 + M, 3]
    float32, faces' [F_out, 3] int32, src_vertex [V1 + M] int32, mid_ends [M, 2] int32)."""
    vp, fp, V, F = _mesh_repair_args(verts, faces)
    V_out = int(V1) + int(M)
    out_v = torch.empty(V_out, 3, dtype=torch.float32, device=faces.device)
    out_f = torch.empty(int(F_out), 3, dtype=torch.int32, device=faces.device)
    src = torch.empty(V_out, dtype=torch.int32, device=faces.device)
    ends = torch.empty(int(M), 2, dtype=torch.int32, device=faces.device)
    _check(lib.nerfart_mesh_repair_emit(vp, fp, V, F, int(table_log2), _dev(ws, torch.uint8, "ws"), ws.numel(), out_v.data_ptr(), out_f.data_ptr(),
                                        src.data_ptr(), ends.data_ptr(), V_out, int(M), int(F_out), _stream()), "nerfart_mesh_repair_emit")
    return out_v, out_f, src, ends


def _mesh_simplify_args(verts, faces, dims, factor):
    V = int(verts.shape[0])
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise NerfartHipError(f"verts must be [V, 3] (got {tuple(verts.shape)})")
    fp, F = _mesh_faces(faces, V)
    if len(dims) != 3:
        raise NerfartHipError(f"the grid shape must be (nx, ny, nz) (got {tuple(dims)})")
    return _dev(verts, name="verts"), fp, V, F, [int(factor)] + [int(d) for d in dims]


def mesh_simplify_workspace_bytes(V: int, F: int, factor: int, dims) -> int:
    """nerfart_mesh_simplify_workspace_bytes; a refusal (factor < 2, a lattice of 2^31 cells, V >= 2^31, F >= 2^30) raises with the library's message."""
    n = int(lib.nerfart_mesh_simplify_workspace_bytes(int(V), int(F), int(factor), *[int(d) for d in dims]))
    _check(0 if n else 2, "nerfart_mesh_simplify_workspace_bytes")
    return n


def mesh_simplify_count(verts, faces, dims, factor: int, ws=None):
    """nerfart_mesh_simplify_count on verts [V, 3] (grid coordinates of a grid of dims = (nx, ny, nz)) and faces [F, 3] int32: (ws, cluster, counts)
    - the filled workspace (uint8; a caller's own, or a fresh one: it must stay untouched until mesh_simplify_emit has run), cluster [V] int32 =
    the new vertex of every old one, and the int32 device tensor counts [3] = (V', F', bad flag).  No host synchronisation."""
    vp, fp, V, F, grid = _mesh_simplify_args(verts, faces, dims, factor)
    if ws is None:
        ws = torch.empty(mesh_simplify_workspace_bytes(V, F, factor, dims), dtype=torch.uint8, device=verts.device)
    cluster = torch.empty(V, dtype=torch.int32, device=verts.device)
    counts = torch.empty(3, dtype=torch.int32, device=verts.device)
    _check(lib.nerfart_mesh_simplify_count(vp, fp, V, F, *grid, _dev(ws, torch.uint8, "ws"), ws.numel(), cluster.data_ptr(), counts.data_ptr(), _stream()),
           "nerfart_mesh_simplify_count")
    return ws, cluster, counts


def mesh_simplify_emit(verts, faces, dims, factor: int, reg: float, ws, cluster, V_out: int, F_out: int):
    """nerfart_mesh_simplify_emit: (verts' [V_out, 3] float32 in grid coordinates, faces' [F_out, 3] int32) from the workspace and the cluster array
    mesh_simplify_count filled for the same mesh."""
    _, fp, V, F, grid = _mesh_simplify_args(verts, faces, dims, factor)
    if cluster.shape != (V,):
        raise NerfartHipError(f"cluster must be [{V}] (got {tuple(cluster.shape)})")
    out_v = torch.empty(int(V_out), 3, dtype=torch.float32, device=verts.device)
    out_f = torch.empty(int(F_out), 3, dtype=torch.int32, device=verts.device)
    _check(lib.nerfart_mesh_simplify_emit(fp, V, F, *grid, float(reg), _dev(ws, torch.uint8, "ws"), ws.numel(), _dev(cluster, torch.int32, "cluster"),
                                          out_v.data_ptr(), out_f.data_ptr(), int(V_out), int(F_out), _stream()), "nerfart_mesh_simplify_emit")
    return out_v, out_f


def _mesh_arrays(verts, faces):
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise NerfartHipError(f"verts must be [V, 3] (got {tuple(verts.shape)})")
    V = int(verts.shape[0])
    fp, F = _mesh_faces(faces, V)
    return _dev(verts, name="verts"), fp, V, F


def mesh_sample_workspace_bytes(F: int) -> int:
    """nerfart_mesh_sample_workspace_bytes; F >= 2^31 raises with the library's message."""
    n = int(lib.nerfart_mesh_sample_workspace_bytes(int(F)))
    _check(0 if n else 2, "nerfart_mesh_sample_workspace_bytes")
    return n


def mesh_sample_count(verts, faces, density: float, seed: int, ws=None, info=None):
    """nerfart_mesh_sample_count: (ws, info) - the filled workspace (uint8; a caller's own or a fresh one: it must stay untouched until
    mesh_sample_emit has run) and the int32 device tensor info [4] = (n, bad faces, overflow flag, 0).  No host synchronisation."""
    vp, fp, V, F = _mesh_arrays(verts, faces)
    if ws is None:
        ws = torch.empty(mesh_sample_workspace_bytes(F), dtype=torch.uint8, device=verts.device)
    if info is None:
        info = torch.empty(4, dtype=torch.int32, device=verts.device)
    if tuple(info.shape) != (4,):
        raise NerfartHipError(f"info must be [4] (got {tuple(info.shape)})")
    _check(lib.nerfart_mesh_sample_count(vp, fp, V, F, float(density), int(seed) & 0xffffffff, _dev(ws, torch.uint8, "ws"), ws.numel(),
                                         _dev(info, torch.int32, "info"), _stream()), "nerfart_mesh_sample_count")
    return ws, info


def mesh_sample_offsets(ws, F: int):
    """off [F] int32: the offset of every face's first sample, out of the workspace mesh_sample_count filled (a copy)."""
    return ws[:8 * int(F)].view(torch.int32).view(int(F), 2)[:, 0].clone()


def mesh_sample_emit(verts, faces, seed: int, ws, n: int, points=None, face=None):
    """nerfart_mesh_sample_emit: (points [n, 3] float32, face [n] int32) - the caller's own arrays or fresh ones - from the workspace
    mesh_sample_count filled for the same mesh and seed."""
    vp, fp, V, F = _mesh_arrays(verts, faces)
    n = int(n)
    if points is None:
        points = torch.empty(n, 3, dtype=torch.float32, device=verts.device)
    if face is None:
        face = torch.empty(n, dtype=torch.int32, device=verts.device)
    if tuple(points.shape) != (n, 3) or tuple(face.shape) != (n,):
        raise NerfartHipError(f"points must be [{n}, 3] and face [{n}] (got {tuple(points.shape)}, {tuple(face.shape)})")
    _check(lib.nerfart_mesh_sample_emit(vp, fp, V, F, int(seed) & 0xffffffff, _dev(ws, torch.uint8, "ws"), ws.numel(), _dev(points, name="points"),
                                        _dev(face, torch.int32, "face"), n, _stream()), "nerfart_mesh_sample_emit")
    return points, face


def mesh_grid_workspace_bytes(grid) -> int:
    """nerfart_mesh_grid_workspace_bytes; a refusal (a dimension outside 1 .. 1024, more than 2^24 cells) raises with the library's message."""
    n = int(lib.nerfart_mesh_grid_workspace_bytes(*[int(g) for g in grid]))
    _check(0 if n else 2, "nerfart_mesh_grid_workspace_bytes")
    return n


class MeshGrid:
    """What nerfart_mesh_closest needs of a mesh: the grid, its filled workspace, the per-cell face lists, and the two numbers the host read."""
    __slots__ = ("grid", "ws", "list", "entries", "good")


def mesh_grid_build(verts, faces, grid) -> MeshGrid:
    """nerfart_mesh_grid_count, ONE host read (entries, good faces), nerfart_mesh_grid_fill."""
    vp, fp, V, F = _mesh_arrays(verts, faces)
    if len(grid) != 3:
        raise NerfartHipError(f"the grid must be (gx, gy, gz) (got {tuple(grid)})")
    g = MeshGrid()
    g.grid = tuple(int(x) for x in grid)
    g.ws = torch.empty(mesh_grid_workspace_bytes(g.grid), dtype=torch.uint8, device=verts.device)
    info = torch.empty(2, dtype=torch.int64, device=verts.device)
    _check(lib.nerfart_mesh_grid_count(vp, fp, V, F, *g.grid, g.ws.data_ptr(), g.ws.numel(), info.data_ptr(), _stream()), "nerfart_mesh_grid_count")
    g.entries, g.good = (int(c) for c in info.cpu())
    if g.entries >= 1 << 31:
        raise NerfartHipError(f"mesh_grid_build: {g.entries} entries in a grid of {g.grid} (2^31 or more): use a coarser grid")
    g.list = torch.empty(g.entries, dtype=torch.int32, device=verts.device)
    _check(lib.nerfart_mesh_grid_fill(vp, fp, V, F, *g.grid, g.ws.data_ptr(), g.ws.numel(), g.list.data_ptr(), g.entries, _stream()),
           "nerfart_mesh_grid_fill")
    return g


def mesh_closest(points, verts, faces, g: MeshGrid, max_distance: float = float("inf"), want_visited: bool = False, dist=None, face=None, visited=None):
    """nerfart_mesh_closest: (dist [n] float32, face [n] int32[, visited [n] int32]) for points [n, 3] float32 against the mesh mesh_grid_build
    was given.  dist / face / visited: the caller's own arrays or fresh ones; visited is returned when asked for or given."""
    vp, fp, V, F = _mesh_arrays(verts, faces)
    if points.dim() != 2 or points.shape[1] != 3:
        raise NerfartHipError(f"points must be [n, 3] (got {tuple(points.shape)})")
    n = int(points.shape[0])
    pp = _dev(points, name="points")
    if dist is None:
        dist = torch.empty(n, dtype=torch.float32, device=verts.device)
    if face is None:
        face = torch.empty(n, dtype=torch.int32, device=verts.device)
    if tuple(dist.shape) != (n,) or tuple(face.shape) != (n,):
        raise NerfartHipError(f"dist and face must be [{n}] (got {tuple(dist.shape)}, {tuple(face.shape)})")
    if visited is None and want_visited:
        visited = torch.empty(n, dtype=torch.int32, device=verts.device)
    if visited is not None and tuple(visited.shape) != (n,):
        raise NerfartHipError(f"visited must be [{n}] (got {tuple(visited.shape)})")
    _check(lib.nerfart_mesh_closest(pp, n, vp, fp, V, F, *g.grid, g.ws.data_ptr(), g.ws.numel(), g.list.data_ptr(), g.entries, float(max_distance),
                                    _dev(dist, name="dist"), _dev(face, torch.int32, "face"), _dev(visited, torch.int32, "visited"), _stream()),
           "nerfart_mesh_closest")
    return (dist, face) if visited is None else (dist, face, visited)


def mesh_atlas_layout(F: int, P: int):
    """nerfart_mesh_atlas_layout: (S, Cw, Ch, W, H) of the per-face texture atlas of F faces at patch size P (include/nerfart_hip.h); host only.
    A refusal (F < 1, P < 1, an image side above 16384) raises with the library's message."""
    dims = (C.c_int * 5)()
    _check(lib.nerfart_mesh_atlas_layout(int(F), int(P), C.cast(dims, C.c_void_p)), "nerfart_mesh_atlas_layout")
    return tuple(int(d) for d in dims)


def mesh_atlas_points(verts, faces, P: int):
    """nerfart_mesh_atlas_points on verts [V, 3] float32 and faces [F, 3] int32: (points [W * H, 3] float32, face_of [H, W] int32 - the owning face
    of every texel, -1 for an invalid one, whose point is 0 -, info [1] int32 - 1 if a face holds an index outside [0, V)), all on verts' device.
    No host synchronisation."""
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise NerfartHipError(f"verts must be [V, 3] (got {tuple(verts.shape)})")
    V = int(verts.shape[0])
    vp = _dev(verts, name="verts")
    fp, F = _mesh_faces(faces, V)
    _, _, _, W, H = mesh_atlas_layout(F, P)                          # refuses before anything is allocated
    points = torch.empty(W * H, 3, dtype=torch.float32, device=verts.device)
    face_of = torch.empty(H, W, dtype=torch.int32, device=verts.device)
    info = torch.empty(1, dtype=torch.int32, device=verts.device)
    _check(lib.nerfart_mesh_atlas_points(vp, fp, V, F, int(P), points.data_ptr(), face_of.data_ptr(), info.data_ptr(), _stream()),
           "nerfart_mesh_atlas_points")
    return points, face_of, info


def mesh_project_step(points, sdf, nabla, level: float, max_step: float):
    """nerfart_mesh_project_step, in place on points [n, 3]: one Newton step toward sdf == level along nabla [n, 3], at most max_step long; a row
    with a non-finite sdf or gradient, or |gradient|^2 < 1e-12, stays."""
    n = int(points.shape[0])
    if tuple(points.shape) != (n, 3) or tuple(sdf.shape) != (n,) or tuple(nabla.shape) != (n, 3):
        raise NerfartHipError(f"mesh_project_step: points [{n}, 3], sdf [{n}], nabla [{n}, 3] expected (got {tuple(points.shape)}, {tuple(sdf.shape)}, "
                              f"{tuple(nabla.shape)})")
    _check(lib.nerfart_mesh_project_step(_dev(points, name="points"), _dev(sdf, name="sdf"), _dev(nabla, name="nabla"), n, float(level), float(max_step),
                                         _stream()), "nerfart_mesh_project_step")


def mesh_camera(c2w, intrinsics):
    """The HOST numbers the mesh_raster entry points take, from c2w [4, 4] (row-major, OpenCV) and intrinsics [4, 4] (tensors or arrays, read on
    the host): (w2c [12], rot [9], K5 [5]) as ctypes float arrays.  w2c is the float64 inverse of the fp32 c2w, rounded to fp32 once; rot is c2w's
    rotation; K5 = (fx, sk, cx, fy, cy) = K[0], K[1], K[2], K[5], K[6] as k_get_rays reads them."""
    import numpy as np
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    c = host(c2w).astype(np.float32).reshape(4, 4)
    k = host(intrinsics).astype(np.float32).reshape(-1)
    if k.size < 7:
        raise NerfartHipError(f"intrinsics must hold a 4x4 (or 3x3 padded to it) row-major matrix (got {k.size} numbers)")
    w2c = np.linalg.inv(c.astype(np.float64))[:3].astype(np.float32).reshape(-1)
    rot = np.ascontiguousarray(c[:3, :3]).reshape(-1)
    k5 = np.array([k[0], k[1], k[2], k[5], k[6]], dtype=np.float32)
    return tuple((C.c_float * len(a))(*[float(x) for x in a]) for a in (w2c, rot, k5))


def mesh_project(verts, camera, near: float):
    """nerfart_mesh_project on verts [V, 3] float32 with camera = mesh_camera(c2w, K): (xy_fix [V, 2] int32 - the pixel position in 1/256 pixel -,
    cam [V, 3] float32 - the camera-space point -, valid [V] uint8), on verts' device.  No host synchronisation."""
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise NerfartHipError(f"verts must be [V, 3] (got {tuple(verts.shape)})")
    V = int(verts.shape[0])
    vp = _dev(verts, name="verts")
    xy_fix = torch.empty(V, 2, dtype=torch.int32, device=verts.device)
    cam = torch.empty(V, 3, dtype=torch.float32, device=verts.device)
    valid = torch.empty(V, dtype=torch.uint8, device=verts.device)
    w2c, _, k5 = camera
    _check(lib.nerfart_mesh_project(vp, V, C.cast(w2c, C.c_void_p), C.cast(k5, C.c_void_p), float(near), xy_fix.data_ptr(), cam.data_ptr(),
                                    valid.data_ptr(), _stream()), "nerfart_mesh_project")
    return xy_fix, cam, valid


def mesh_raster(xy_fix, cam, valid, faces, camera, near: float, H: int, W: int):
    """nerfart_mesh_raster: (zbuf [H * W] int64 holding the uint64 keys (depth bits << 32 | face; all ones = no face), info [4] int32 = (1 if a
    face holds an index outside [0, V), faces skipped for an invalid vertex, samples rejected by the depth rule, faces that went through the
    large-face launch)), on faces' device.  No host synchronisation."""
    V = int(xy_fix.shape[0])
    if tuple(xy_fix.shape) != (V, 2) or tuple(cam.shape) != (V, 3) or tuple(valid.shape) != (V,):
        raise NerfartHipError(f"mesh_raster: xy_fix [{V}, 2], cam [{V}, 3], valid [{V}] expected (got {tuple(xy_fix.shape)}, {tuple(cam.shape)}, "
                              f"{tuple(valid.shape)})")
    fp, F = _mesh_faces(faces, V)
    H, W = int(H), int(W)
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise NerfartHipError(f"mesh_raster: H and W must be in 1 .. 16384 (got {H}, {W})")
    zbuf = torch.empty(H * W, dtype=torch.int64, device=faces.device)
    work = torch.empty(max(F, 1), dtype=torch.int32, device=faces.device)
    info = torch.empty(4, dtype=torch.int32, device=faces.device)
    _check(lib.nerfart_mesh_raster(_dev(xy_fix, torch.int32, "xy_fix"), _dev(cam, name="cam"), _dev(valid, torch.uint8, "valid"), fp, V, F,
                                   C.cast(camera[2], C.c_void_p), float(near), H, W, zbuf.data_ptr(), work.data_ptr(), info.data_ptr(), _stream()),
           "nerfart_mesh_raster")
    return zbuf, info


def mesh_resolve(zbuf, cam, faces, camera, H: int, W: int):
    """nerfart_mesh_resolve on mesh_raster's zbuf: dict of face_id [H * W] int32 (-1: no face), bary [H * W, 3], z [H * W] (camera z), depth [H * W]
    (distance along the unit ray), mask [H * W] uint8, face_normals [H * W, 3] (world space, toward the camera); a miss is 0 in all of them."""
    V = int(cam.shape[0])
    fp, F = _mesh_faces(faces, V)
    H, W = int(H), int(W)
    if tuple(zbuf.shape) != (H * W,) or tuple(cam.shape) != (V, 3):
        raise NerfartHipError(f"mesh_resolve: zbuf [{H * W}] and cam [{V}, 3] expected (got {tuple(zbuf.shape)}, {tuple(cam.shape)})")
    dev, n = zbuf.device, H * W
    out = {"face_id": torch.empty(n, dtype=torch.int32, device=dev), "bary": torch.empty(n, 3, dtype=torch.float32, device=dev),
           "z": torch.empty(n, dtype=torch.float32, device=dev), "depth": torch.empty(n, dtype=torch.float32, device=dev),
           "mask": torch.empty(n, dtype=torch.uint8, device=dev), "face_normals": torch.empty(n, 3, dtype=torch.float32, device=dev)}
    _check(lib.nerfart_mesh_resolve(_dev(zbuf, torch.int64, "zbuf"), _dev(cam, name="cam"), fp, V, F, C.cast(camera[2], C.c_void_p),
                                    C.cast(camera[1], C.c_void_p), H, W, *(out[k].data_ptr() for k in ("face_id", "bary", "z", "depth", "mask",
                                                                                                  "face_normals")), _stream()),
           "nerfart_mesh_resolve")
    return out


def mesh_interp(face_id, bary, attr, faces=None, fill: float = 0.0):
    """nerfart_mesh_interp: out [n, C] float32 = sum_k bary[p, k] * (attribute of corner k of face face_id[p]); attr is [V, C] with faces [F, 3] (per
    vertex, gathered through faces) or [F, 3, C] with faces=None (per corner).  C <= 8; a miss (face_id < 0) gets `fill`."""
    n = int(face_id.shape[0])
    if tuple(face_id.shape) != (n,) or tuple(bary.shape) != (n, 3):
        raise NerfartHipError(f"mesh_interp: face_id [{n}] and bary [{n}, 3] expected (got {tuple(face_id.shape)}, {tuple(bary.shape)})")
    if faces is not None:
        if attr.dim() != 2:
            raise NerfartHipError(f"mesh_interp: per-vertex attributes must be [V, C] (got {tuple(attr.shape)})")
        V, Cn = int(attr.shape[0]), int(attr.shape[1])
        fp, F = _mesh_faces(faces, V)
    else:
        if attr.dim() != 3 or attr.shape[1] != 3:
            raise NerfartHipError(f"mesh_interp: per-corner attributes must be [F, 3, C] (got {tuple(attr.shape)})")
        V, F, Cn, fp = 0, int(attr.shape[0]), int(attr.shape[2]), None
    if not 1 <= Cn <= 8:
        raise NerfartHipError(f"mesh_interp: C must be in 1 .. 8 (got {Cn})")
    out = torch.empty(n, Cn, dtype=torch.float32, device=face_id.device)
    _check(lib.nerfart_mesh_interp(_dev(face_id, torch.int32, "face_id"), _dev(bary, name="bary"), fp, _dev(attr, name="attr"), V, F, Cn, n, float(fill),
                                   out.data_ptr(), _stream()), "nerfart_mesh_interp")
    return out


def mesh_sample_bilinear(uv, image, mask=None, background=(0.0, 0.0, 0.0)):
    """nerfart_mesh_sample_bilinear: rgb [n, 3] float32 = the bilinear sample (clamp to edge, level / 255) of image [Ht, Wt, 3] uint8 at uv [n, 2]
    float32 in PIXEL units (texel centres at + 0.5, y down: the atlas_uvs convention); mask [n] uint8 == 0, or a non-finite uv, gives `background`."""
    n = int(uv.shape[0])
    if tuple(uv.shape) != (n, 2) or image.dim() != 3 or image.shape[2] != 3 or (mask is not None and tuple(mask.shape) != (n,)):
        raise NerfartHipError(f"mesh_sample_bilinear: uv [{n}, 2], image [Ht, Wt, 3], mask [{n}] expected (got {tuple(uv.shape)}, {tuple(image.shape)}, "
                              f"{None if mask is None else tuple(mask.shape)})")
    bg = (C.c_float * 3)(*[float(b) for b in background])
    out = torch.empty(n, 3, dtype=torch.float32, device=uv.device)
    _check(lib.nerfart_mesh_sample_bilinear(_dev(uv, name="uv"), _dev(mask, torch.uint8, "mask"), _dev(image, torch.uint8, "image"), int(image.shape[0]),
                                            int(image.shape[1]), n, C.cast(bg, C.c_void_p), out.data_ptr(), _stream()), "nerfart_mesh_sample_bilinear")
    return out


def band_bricks(N: int, B: int) -> int:
    """Bricks of edge B in an N^3 grid: ceil(N / B)^3 (csrc/mesh_band.hip)."""
    return (-(-int(N) // int(B))) ** 3


def band_workspace_bytes(N: int, B: int) -> int:
    """nerfart_band_workspace_bytes; bad dimensions (N < 2, B outside 2 .. 64, N^3 >= 2^31) raise with the library's message."""
    n = int(lib.nerfart_band_workspace_bytes(int(N), int(B)))
    _check(0 if n else 2, "nerfart_band_workspace_bytes")
    return n


def band_probe_points(N: int, B: int, step: float, org: float, device):
    """nerfart_band_probe_points: pts [ceil(N / B)^3, 3] float32 - the probe grid point of every brick, in mesh_util.grid_points' bits."""
    band_workspace_bytes(N, B)                                         # the dimensions, refused before anything is allocated
    pts = torch.empty(band_bricks(N, B), 3, dtype=torch.float32, device=device)
    _check(lib.nerfart_band_probe_points(int(N), int(B), float(step), float(org), _dev(pts, name="pts"), _stream()), "nerfart_band_probe_points")
    return pts


class BandState:
    """The per-brick arrays of one banded sweep, all on `device`: flag / wanted [bricks] uint8, list [bricks] int32, ptoff [bricks] int32 (holding
    uint32), the selection's workspace."""
    def __init__(self, N: int, B: int, device):
        self.N, self.B, self.bricks = int(N), int(B), band_bricks(N, B)
        self.ws = torch.empty(band_workspace_bytes(N, B), dtype=torch.uint8, device=device)
        self.flag = torch.zeros(self.bricks, dtype=torch.uint8, device=device)
        self.wanted = torch.zeros(self.bricks, dtype=torch.uint8, device=device)
        self.list = torch.empty(self.bricks, dtype=torch.int32, device=device)
        self.ptoff = torch.empty(self.bricks, dtype=torch.int32, device=device)


def band_select(state: BandState, mode: int, probe=None, level: float = 0.0, threshold: float = 0.0):
    """nerfart_band_select on state: the int32 device tensor counts [2] = (newly active bricks, their owned points); state.list / state.ptoff hold
    the ascending list, state.flag is updated, state.wanted cleared.  mode 0: the probe test on probe [bricks] (fp32); 1: the wanted bricks;
    2: every brick not yet active.  No host synchronisation."""
    if probe is not None and probe.shape != (state.bricks,):
        raise NerfartHipError(f"probe must be [{state.bricks}] (got {tuple(probe.shape)})")
    counts = torch.empty(2, dtype=torch.int32, device=state.flag.device)
    _check(lib.nerfart_band_select(int(mode), _dev(probe, name="probe"), float(level), float(threshold), state.N, state.B, state.flag.data_ptr(),
                                   state.wanted.data_ptr(), state.list.data_ptr(), state.ptoff.data_ptr(), state.ws.data_ptr(), state.ws.numel(),
                                   counts.data_ptr(), _stream()), "nerfart_band_select")
    return counts


def band_brick_points(state: BandState, n_list: int, n_points: int, first: int, count: int, step: float, org: float):
    """nerfart_band_brick_points: (pts [count, 3] float32, idx [count] int32 - the linear grid indices) of the points first .. first + count of
    the evaluation order of band_select's list (n_list bricks, n_points points)."""
    dev = state.flag.device
    pts = torch.empty(int(count), 3, dtype=torch.float32, device=dev)
    idx = torch.empty(int(count), dtype=torch.int32, device=dev)
    _check(lib.nerfart_band_brick_points(state.list.data_ptr(), state.ptoff.data_ptr(), int(n_list), int(n_points), int(first), int(count), state.N,
                                         state.B, float(step), float(org), pts.data_ptr(), idx.data_ptr(), _stream()), "nerfart_band_brick_points")
    return pts, idx


def _band_volume(vol, N: int):
    if tuple(vol.shape) != (N, N, N):
        raise NerfartHipError(f"the volume must be [{N}, {N}, {N}] (got {tuple(vol.shape)})")
    return _dev(vol, name="vol")


def band_scatter(val, idx, vol):
    """nerfart_band_scatter: vol.view(-1)[idx] = val (val [M] float32, idx [M] int32 from band_brick_points), in place."""
    M = idx.shape[0]
    if val.shape != (M,):
        raise NerfartHipError(f"val must be [{M}] (got {tuple(val.shape)})")
    _check(lib.nerfart_band_scatter(_dev(val, name="val"), _dev(idx, torch.int32, "idx"), M, int(vol.shape[0]), _band_volume(vol, int(vol.shape[0])),
                                    _stream()), "nerfart_band_scatter")


def band_fill(state: BandState, probe, vol):
    """nerfart_band_fill: every point of a brick that is not active gets probe [bricks] of its brick, in place on vol [N, N, N]."""
    if probe.shape != (state.bricks,):
        raise NerfartHipError(f"probe must be [{state.bricks}] (got {tuple(probe.shape)})")
    _check(lib.nerfart_band_fill(_dev(probe, name="probe"), state.flag.data_ptr(), state.N, state.B, _band_volume(vol, state.N), _stream()),
           "nerfart_band_fill")


def band_check(state: BandState, vol, level: float):
    """nerfart_band_check: marks in state.wanted the inactive bricks that hold an end of a sign-changing edge of vol; the int32 device tensor
    counts [2] = (wanted bricks, their owned points).  No host synchronisation."""
    counts = torch.empty(2, dtype=torch.int32, device=vol.device)
    _check(lib.nerfart_band_check(_band_volume(vol, state.N), float(level), state.flag.data_ptr(), state.N, state.B, state.wanted.data_ptr(),
                                  counts.data_ptr(), _stream()), "nerfart_band_check")
    return counts


def nabla_workspace(precision: int, device):
    """The reverse-mode grad(SDF) kernels' scratch (softplus' of the forward sweep), from PyTorch's caching allocator: visible
    to torch.cuda.max_memory_allocated(), stream-ordered like every other tensor of the call."""
    nb = int(lib.nerfart_sdf_nabla_workspace_bytes(int(precision)))
    return (torch.empty(nb, dtype=torch.uint8, device=device) if nb else None), nb


def wgrad(Z, A, n_mats: int, rows: int, a_cols: int, z_stride: int, a_stride: int, cs_rows: int = 0, want_cs: bool = False):
    """dW [n_mats, 256, a_cols] fp32 = Z_m^T A_m (+ cs [n_mats, 256] = column sums of the first cs_rows rows of Z_m) over bf16
    row-major operands: Z / A are tensors whose data_ptr() is matrix 0 ([rows, 256] / [rows, a_cols]); strides in BYTES between
    matrices (0 = shared operand).  nerfart_wgrad_bf16 (csrc/wgrad.hip)."""
    dev = Z.device
    assert Z.dtype == torch.bfloat16 and A.dtype == torch.bfloat16 and Z.is_cuda and A.is_cuda
    dW = torch.empty(n_mats, 256, a_cols, dtype=torch.float32, device=dev)
    cs = torch.empty(n_mats, 256, dtype=torch.float32, device=dev) if want_cs else None
    nb = int(lib.nerfart_wgrad_workspace_bytes(n_mats, rows, a_cols))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _check(lib.nerfart_wgrad_bf16(Z.data_ptr(), int(z_stride), A.data_ptr(), int(a_stride), n_mats, rows, a_cols, int(cs_rows),
                                  _dev(dW), _dev(cs), 0, _dev(ws, torch.uint8), nb, _stream()), "nerfart_wgrad_bf16")
    return dW, cs


# ---- per-point glue of pass 2 (csrc/pass2_operands.hip) ------------------------------------------
def ray_points(rays_o, rays_dn, depth, want_view: bool = True):
    """pts [R P, 3] = o + dn * depth, view [R P, 3] = dn per sample."""
    R, P = depth.shape
    pts = torch.empty(R * P, 3, dtype=torch.float32, device=depth.device)
    view = torch.empty(R * P, 3, dtype=torch.float32, device=depth.device) if want_view else None
    _check(lib.nerfart_ray_points(_dev(rays_o, name="rays_o"), _dev(rays_dn, name="rays_dn"), _dev(depth, name="depth"), R, P, _dev(pts),
                                  _dev(view), _stream()), "nerfart_ray_points")
    return pts, view


def volsdf_pass2_cotangents(pts, sdf, g_sdf, nabla, g_n, R: int, P: int, R_bg: float, w_eikonal: float, eik_group_rays=None, g_n_extra=None):
    """(sbar [R P], nbar [R P, 3], eik_ray [R]) - see include/nerfart_hip.h."""
    dev = pts.device
    sbar = torch.empty(R * P, dtype=torch.float32, device=dev)
    nbar = torch.empty(R * P, 3, dtype=torch.float32, device=dev)
    eik_ray = torch.empty(R, dtype=torch.float32, device=dev)
    _check(lib.nerfart_volsdf_pass2_cotangents(_dev(pts, name="pts"), _dev(sdf, name="sdf"), _dev(g_sdf, name="g_sdf"), _dev(nabla, name="nabla"),
                                               _dev(g_n, name="g_n"), _dev(g_n_extra, name="g_n_extra"), R, P, float(R_bg), float(w_eikonal),
                                               int(eik_group_rays or 0), _dev(sbar), _dev(nbar), _dev(eik_ray), _stream()),
           "nerfart_volsdf_pass2_cotangents")
    return sbar, nbar, eik_ray


def _operand(rows: int, device):
    return torch.empty(rows, 64, dtype=torch.bfloat16, device=device)


def wgrad_operand_embed_pair(pts, direction, rows_pad: int, multires: int):
    out = _operand(2 * rows_pad, pts.device)
    _check(lib.nerfart_wgrad_operand_embed_pair(_dev(pts, name="pts"), _dev(direction, name="dir"), pts.shape[0], rows_pad, int(multires),
                                                out.data_ptr(), _stream()), "nerfart_wgrad_operand_embed_pair")
    return out


def wgrad_operand_inputs(x, multires_x: int, view, multires_view: int, normals, rows_pad: int):
    out = _operand(rows_pad, x.device)
    _check(lib.nerfart_wgrad_operand_inputs(_dev(x, name="x"), int(multires_x), _dev(view, name="view"), int(multires_view),
                                            _dev(normals, name="normals"), x.shape[0], rows_pad, out.data_ptr(), _stream()),
           "nerfart_wgrad_operand_inputs")
    return out


def wgrad_operand_rgb_delta(rgb, g_rgb, rows_pad: int, want_d4: bool = False):
    """(operand [rows_pad, 64] bf16, column sums of d4 = g_rgb rgb (1 - rgb) [3], d4 [M, 3] or None)"""
    out = _operand(rows_pad, rgb.device)
    d4 = torch.empty(rgb.shape[0], 3, dtype=torch.float32, device=rgb.device) if want_d4 else None
    sums = torch.empty((rows_pad + 31) // 32, 3, dtype=torch.float32, device=rgb.device)
    _check(lib.nerfart_wgrad_operand_rgb_delta(_dev(rgb, name="rgb"), _dev(g_rgb, name="g_rgb"), rgb.shape[0], rows_pad, out.data_ptr(),
                                               _dev(d4), _dev(sums), _stream()), "nerfart_wgrad_operand_rgb_delta")
    return out, sums.sum(0), d4


def wgrad_operand_sbar_ones(sbar, rows_pad: int):
    out = _operand(2 * rows_pad, sbar.device)
    _check(lib.nerfart_wgrad_operand_sbar_ones(_dev(sbar, name="sbar"), sbar.shape[0], rows_pad, out.data_ptr(), _stream()),
           "nerfart_wgrad_operand_sbar_ones")
    return out


def radiance_fwd(rad_blob, view_tiles: int, pts, view, nabla, h7, precision: int = 0):
    M = pts.shape[0]
    rgb = torch.empty(M, 3, dtype=torch.float32, device=pts.device)
    _check(lib.nerfart_radiance_fwd(_dev(rad_blob), int(precision), int(view_tiles), _dev(pts, name="pts"), _dev(view, name="view"), M,
                                    _dev(nabla, name="nabla"), _dev(h7, name="h7"), _dev(rgb), _stream()),
           "nerfart_radiance_fwd")
    return rgb


def sdf_fwd_rays(surf_blob, rays_o, rays_dn, depth, R_bg: float, ray_idx=None, n_per_ray=None, precision: int = 0):
    """depth [n_slots, stride >= n_per_ray] -> sdf [n_slots, n_per_ray]"""
    n_slots, stride = depth.shape
    n_per_ray = stride if n_per_ray is None else n_per_ray
    out = torch.empty(n_slots, n_per_ray, dtype=torch.float32, device=depth.device)
    _check(lib.nerfart_sdf_fwd_rays(_dev(surf_blob), int(precision), _dev(rays_o), _dev(rays_dn), _dev(ray_idx, torch.int32),
                                    _dev(depth), n_slots, n_per_ray, stride, float(R_bg), _dev(out), n_per_ray, _stream()),
           "nerfart_sdf_fwd_rays")
    return out


# ---- rays ------------------------------------------------------------------------------------
def get_rays(pose, K, H: int, W: int, select=None):
    n = H * W if select is None else select.numel()
    o = torch.empty(n, 3, dtype=torch.float32, device=pose.device)
    d = torch.empty(n, 3, dtype=torch.float32, device=pose.device)
    _check(lib.nerfart_get_rays(_dev(pose, name="pose"), _dev(K, name="K"), H, W, _dev(select, torch.int64), n, _dev(o), _dev(d),
                                _stream()), "nerfart_get_rays")
    return o, d


def normalize_dirs(d):
    out = torch.empty_like(d)
    _check(lib.nerfart_normalize_dirs(_dev(d), _dev(out), d.shape[0], _stream()), "nerfart_normalize_dirs")
    return out


_lin_cache = {}


def lin_table(n: int, device) -> torch.Tensor:
    """torch.linspace(0, 1, n) as the reference builds it (CPU kernel, then moved; volsdf.py:472,483), cached."""
    key = (n, str(device))
    if key not in _lin_cache:
        _lin_cache[key] = torch.linspace(0, 1, n).float().to(device)
    return _lin_cache[key]


_ws_cache = {}
_ws_lock = __import__("threading").Lock()


def _workspace(nbytes: int, device) -> torch.Tensor:
    """One cached byte buffer per (device, stream), grown on demand (288 GB of HBM: keep it resident).  Per stream: the entry points
    run asynchronously on torch's current stream, so two streams (or two host threads on their own streams) must not share scratch."""
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    with _ws_lock:                                                 # two host threads on their own streams may grow / evict at once
        ws = _ws_cache.get(key)
        if ws is None or ws.numel() < nbytes:
            _ws_cache.pop(key, None)
            while len(_ws_cache) >= 8:                             # short-lived streams must not pin memory for good
                _ws_cache.pop(next(iter(_ws_cache)), None)
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            _ws_cache[key] = ws
    return ws


def volsdf_fine_sample(surf_blob, rays_o, rays_dn, near: float, far: float, R_bg: float, alpha: float, beta: float,
                       eps: float, n_init: int, n_up: int, n_final: int, max_iter: int, max_bisect: int, precision: int = 0,
                       u_final=None, escalate=None, guard: float = 0.0, stats=None, late_round: int = 0):
    """u_final [R, n_final]: the caller's uniform random numbers for the final inverse-CDF samples (perturb=True:
    sample_cdf(det=False), rend_util.py:306-307); None: the deterministic linspace table.
    escalate = (surface blob, precision id) + guard > 0: the GUARDED sampler (nerfart_volsdf_fine_sample_guarded): rays whose convergence decision
    lies within guard * eps of eps, and rays that never converge, are sampled again on that blob.  stats (dict): 'escalated' += rays that ran twice.
    late_round > 0 (with the guard): rays still active after that up-sampling round are escalated there (nerfart_volsdf_fine_sample_guarded2)."""
    R = rays_o.shape[0]
    dev = rays_o.device
    if u_final is not None and tuple(u_final.shape) != (R, n_final):
        raise ValueError(f"u_final must be [{R}, {n_final}]")
    d_fine = torch.empty(R, n_final, dtype=torch.float32, device=dev)
    beta_map = torch.empty(R, dtype=torch.float32, device=dev)
    usage = torch.empty(R, dtype=torch.float32, device=dev)
    nb = lib.nerfart_volsdf_sampler_workspace_bytes(R, n_init, n_up, n_final, max_iter)
    ws = _workspace(nb, dev)
    esc_blob, esc_prec = escalate if (escalate is not None and guard > 0) else (None, 0)
    n_esc = C.c_int(0)
    _check(lib.nerfart_volsdf_fine_sample_guarded2(_dev(surf_blob), int(precision), _dev(esc_blob, name="esc_blob"), int(esc_prec), float(guard), int(late_round),
                                                  _dev(rays_o), _dev(rays_dn), R, None, None, float(near), float(far),
                                                  float(R_bg), float(alpha), float(beta), float(eps), n_init, n_up, n_final, max_iter,
                                                  max_bisect, _dev(lin_table(n_init, dev)), _dev(lin_table(n_up + 2, dev)),
                                                  _dev(lin_table(n_final, dev) if u_final is None else u_final, name="u_final"),
                                                  int(u_final is not None), _dev(d_fine), _dev(beta_map), _dev(usage), C.byref(n_esc), ws.data_ptr(),
                                                  ws.numel(), _stream()), "nerfart_volsdf_fine_sample_guarded2")
    if stats is not None:
        stats["escalated"] = stats.get("escalated", 0) + n_esc.value
        stats["rays"] = stats.get("rays", 0) + R
    return d_fine, beta_map, usage


def sdf_fwd2(surf_blob, pts, direction):
    """Forward sweep of the second-order SDF backward: (value, tangent along `direction`) column pairs; returns the dump
    (uint8) with the activations / tangents (bf16) and softplus' (unorm16) of all 8 layers."""
    M = pts.shape[0]
    dump = torch.empty(int(lib.nerfart_sdf_fwd2_dump_bytes(M)), dtype=torch.uint8, device=pts.device)
    _check(lib.nerfart_sdf_fwd2(_dev(surf_blob), _dev(pts, name="pts"), _dev(direction, name="direction"), M, dump.data_ptr(), _stream()),
           "nerfart_sdf_fwd2")
    return dump


def sdf_bwd2(surf_blob, gbar_h7, gbar_sdf, f2_dump):
    """Reverse sweep: cotangents of h7 [M,256] and sdf [M] -> dump (uint8) of 65535 * (t_l d_l | zbar_l), bf16."""
    M = gbar_sdf.shape[0]
    dump = torch.empty(int(lib.nerfart_sdf_bwd2_dump_bytes(M)), dtype=torch.uint8, device=gbar_sdf.device)
    _check(lib.nerfart_sdf_bwd2(_dev(surf_blob), M, _dev(gbar_h7, name="gbar_h7"), _dev(gbar_sdf, name="gbar_sdf"), f2_dump.data_ptr(),
                                dump.data_ptr(), _stream()), "nerfart_sdf_bwd2")
    return dump


def radiance_fwd_dump(rad_blob, view_tiles: int, pts, view, nabla, h7):
    """Radiance net forward (split-bf16 blob) that also dumps the layer activations (bf16, unit order) for
    radiance_bwd / the weight-gradient GEMMs.  Returns (rgb [M,3], dump uint8)."""
    M = pts.shape[0]
    rgb = torch.empty(M, 3, dtype=torch.float32, device=pts.device)
    dump = torch.empty(int(lib.nerfart_radiance_dump_bytes(M)), dtype=torch.uint8, device=pts.device)
    _check(lib.nerfart_radiance_fwd_dump(_dev(rad_blob), int(view_tiles), _dev(pts, name="pts"), _dev(view, name="view"), M,
                                         _dev(nabla, name="nabla"), _dev(h7, name="h7"), _dev(rgb), dump.data_ptr(), _stream()),
           "nerfart_radiance_fwd_dump")
    return rgb, dump


def radiance_bwd(rad_blob, rgb, g_rgb, fwd_dump):
    """(g_h7 [M,256], g_n [M,3], delta dump uint8) for d loss / d rgb = g_rgb [M,3]."""
    M = rgb.shape[0]
    g_h7 = torch.empty(M, 256, dtype=torch.float32, device=rgb.device)
    g_n = torch.empty(M, 3, dtype=torch.float32, device=rgb.device)
    bwd_dump = torch.empty_like(fwd_dump)
    _check(lib.nerfart_radiance_bwd(_dev(rad_blob), M, _dev(rgb), _dev(g_rgb), fwd_dump.data_ptr(), bwd_dump.data_ptr(), _dev(g_h7),
                                    _dev(g_n), _stream()), "nerfart_radiance_bwd")
    return g_h7, g_n, bwd_dump


def volsdf_composite(d_all, sdf, radiance, alpha: float, beta: float, white_bkgd: bool = False, nabla=None):
    """rgb [R,3], depth [R], acc [R] of nerfart_volsdf_composite for d_all / sdf [R,P], radiance [R,P,3]; with nabla [R,P,3] also normals [R,3]
    (a 4-tuple)."""
    R, P = d_all.shape
    dev = d_all.device
    rgb = torch.empty(R, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(R, dtype=torch.float32, device=dev)
    acc = torch.empty(R, dtype=torch.float32, device=dev)
    normals = None if nabla is None else torch.empty(R, 3, dtype=torch.float32, device=dev)
    _check(lib.nerfart_volsdf_composite(R, P, _dev(d_all), _dev(sdf), _dev(radiance), _dev(nabla, name="nabla"), float(alpha), float(beta),
                                        int(bool(white_bkgd)), _dev(rgb), _dev(depth), _dev(acc), _dev(normals), None, None, None, _stream()),
           "nerfart_volsdf_composite")
    return (rgb, depth, acc) if nabla is None else (rgb, depth, acc, normals)


def volsdf_composite_bwd(d_all, sdf, radiance, alpha: float, beta: float, g_rgb, white_bkgd: bool = False, g_acc=None):
    """Cotangents (g_sdf [R,P], g_radiance [R,P,3], g_alpha_beta [2]) for d loss / d rgb = g_rgb [R,3] (and d loss / d acc
    = g_acc [R], the opacity / mask_volume output, if given)."""
    R, P = d_all.shape
    dev = d_all.device
    g_sdf = torch.empty(R, P, dtype=torch.float32, device=dev)
    g_rad = torch.empty(R, P, 3, dtype=torch.float32, device=dev)
    g_ab = torch.zeros(2, dtype=torch.float32, device=dev)
    _check(lib.nerfart_volsdf_composite_bwd(R, P, _dev(d_all), _dev(sdf), _dev(radiance), float(alpha), float(beta),
                                            int(bool(white_bkgd)), _dev(g_rgb), _dev(g_acc, name="g_acc"), _dev(g_sdf), _dev(g_rad), _dev(g_ab),
                                            _stream()), "nerfart_volsdf_composite_bwd")
    return g_sdf, g_rad, g_ab


def volsdf_composite_geo_bwd(d_all, sdf, alpha: float, beta: float, g_depth=None, g_normals=None, nabla=None, g_n_in=None, g_sdf=None,
                             g_nabla=None, g_alpha_beta=None, accumulate: bool = False):
    """nerfart_volsdf_composite_geo_bwd: the cotangents of the depth map (g_depth [R]) and of the normals map (g_normals [R,3], needs nabla [R,P,3]) of
    the VolSDF compositor -> (g_sdf [R,P], g_nabla [R,P,3] or None, g_alpha_beta [2]).  g_sdf / g_nabla / g_alpha_beta: the caller's buffers (g_sdf is
    added to when `accumulate`, g_alpha_beta always); None: fresh ones (g_alpha_beta zeroed).  g_n_in [R,P,3]: added into g_nabla.  A depth cotangent on
    an empty ray is amplified by 1 / (acc + 1e-10), as in the reference's autograd: weight it with the opacity."""
    R, P = d_all.shape
    dev = d_all.device
    if g_sdf is None:
        if accumulate:
            raise ValueError("volsdf_composite_geo_bwd: accumulate=True needs the g_sdf to add to")
        g_sdf = torch.empty(R, P, dtype=torch.float32, device=dev)
    if g_nabla is None and g_normals is not None:
        g_nabla = torch.empty(R, P, 3, dtype=torch.float32, device=dev)
    if g_alpha_beta is None:
        g_alpha_beta = torch.zeros(2, dtype=torch.float32, device=dev)
    _check(lib.nerfart_volsdf_composite_geo_bwd(R, P, _dev(d_all, name="d_all"), _dev(sdf, name="sdf"), _dev(nabla, name="nabla"), float(alpha), float(beta),
                                                _dev(g_depth, name="g_depth"), _dev(g_normals, name="g_normals"), _dev(g_n_in, name="g_n_in"),
                                                int(bool(accumulate)), _dev(g_sdf, name="g_sdf"), _dev(g_nabla, name="g_nabla"),
                                                _dev(g_alpha_beta, name="g_alpha_beta"), _stream()), "nerfart_volsdf_composite_geo_bwd")
    return g_sdf, (g_nabla if g_normals is not None else None), g_alpha_beta


def neus_composite_bwd(sdf, rad_mid, s: float, g_rgb, white_bkgd: bool = False, g_acc=None):
    """(g_sdf [R,P], g_rad_mid [R,P-1,3], g_s [1]) for d loss / d rgb = g_rgb [R,3] (and d loss / d acc = g_acc [R])."""
    R, P = sdf.shape
    dev = sdf.device
    g_sdf = torch.empty(R, P, dtype=torch.float32, device=dev)
    g_rad = torch.empty(R, P - 1, 3, dtype=torch.float32, device=dev)
    g_s = torch.zeros(1, dtype=torch.float32, device=dev)
    _check(lib.nerfart_neus_composite_bwd(R, P, _dev(sdf), _dev(rad_mid), float(s), int(bool(white_bkgd)), _dev(g_rgb), _dev(g_acc, name="g_acc"),
                                          _dev(g_sdf), _dev(g_rad), _dev(g_s), _stream()), "nerfart_neus_composite_bwd")
    return g_sdf, g_rad, g_s


# ---- B1 "bwd": the ray-level backward (csrc/render_backward.hip) --------------------------------------------------
RAW_SECTIONS = ("surf_ww", "surf_we", "surf_cs0", "surf_cs17", "surf_w8", "surf_b8", "rad_ww", "rad_cs", "rad_w4", "rad_b4", "rad_wex", "rad_wh7",
                "scalars")
RAW_G_ALPHA, RAW_G_BETA, RAW_G_S, RAW_EIKONAL = 0, 1, 2, 3            # entries of the `scalars` section


def raw_layout():
    """({section: float offset}, total floats) of the raw parameter-gradient buffer (nerfart_pass2_raw_layout)."""
    offs = (C.c_longlong * (len(RAW_SECTIONS) + 1))()
    total = int(lib.nerfart_pass2_raw_layout(offs))
    return {k: int(offs[i]) for i, k in enumerate(RAW_SECTIONS)}, total


def new_raw(device) -> torch.Tensor:
    """A zeroed raw buffer: the entry points below ACCUMULATE into it (one buffer per optimiser step)."""
    return torch.zeros(raw_layout()[1], dtype=torch.float32, device=device)


def volsdf_render_bwd(surf_blob, rad_blob, view_tiles: int, multires: int, rays_o, rays_d, d_all, g_rgb, raw, *, R_bg: float, alpha: float,
                      beta: float, white_bkgd: bool = False, w_eikonal: float = 0.0, eik_group_rays: int = 0, train_radiance: bool = True,
                      g_acc=None, g_n_extra=None, state=None, g_depth=None, g_normals=None):
    """rgb.backward(g_rgb) + eikonal.backward() of one launch group of VolSDF rays (volsdf.py:759-770) -> accumulated into `raw`.
    rays_d un-normalised; d_all [R, P] from pass 1; state = (sdf [R P], nabla [R P, 3], h7 [R P, 256]) kept from pass 1 or None.
    g_depth [R] / g_normals [R, 3]: cotangents of the depth and normals maps (nerfart_volsdf_render_bwd2; either given selects that entry point)."""
    R, P = d_all.shape
    sdf, nab, h7 = state if state is not None else (None, None, None)
    if g_depth is None and g_normals is None:
        need_term(surf_blob, "bf16", "nerfart_volsdf_render_bwd"); need_term(rad_blob, "bf16", "nerfart_volsdf_render_bwd")
        nb = int(lib.nerfart_volsdf_render_bwd_workspace_bytes(R, P, int(state is not None)))
        ws = _workspace(nb, d_all.device)
        _check(lib.nerfart_volsdf_render_bwd(
            _dev(surf_blob), _dev(rad_blob), int(view_tiles), int(multires), _dev(rays_o, name="rays_o"), _dev(rays_d, name="rays_d"), R, P,
            _dev(d_all, name="d_all"), _dev(g_rgb, name="g_rgb"), _dev(g_acc, name="g_acc"), _dev(g_n_extra, name="g_n_extra"),
            _dev(sdf, name="sdf_state"), _dev(nab, name="nabla_state"), _dev(h7, name="h7_state"), float(R_bg), float(alpha), float(beta),
            int(bool(white_bkgd)), float(w_eikonal), int(eik_group_rays or 0), int(bool(train_radiance)), _dev(raw, name="raw"), ws.data_ptr(),
            ws.numel(), _stream()), "nerfart_volsdf_render_bwd")
        return
    need_term(surf_blob, "bf16", "nerfart_volsdf_render_bwd2"); need_term(rad_blob, "bf16", "nerfart_volsdf_render_bwd2")
    nb = int(lib.nerfart_volsdf_render_bwd2_workspace_bytes(R, P, int(state is not None), int(g_normals is not None)))
    ws = _workspace(nb, d_all.device)
    _check(lib.nerfart_volsdf_render_bwd2(
        _dev(surf_blob), _dev(rad_blob), int(view_tiles), int(multires), _dev(rays_o, name="rays_o"), _dev(rays_d, name="rays_d"), R, P,
        _dev(d_all, name="d_all"), _dev(g_rgb, name="g_rgb"), _dev(g_acc, name="g_acc"), _dev(g_n_extra, name="g_n_extra"),
        _dev(g_depth, name="g_depth"), _dev(g_normals, name="g_normals"),
        _dev(sdf, name="sdf_state"), _dev(nab, name="nabla_state"), _dev(h7, name="h7_state"), float(R_bg), float(alpha), float(beta),
        int(bool(white_bkgd)), float(w_eikonal), int(eik_group_rays or 0), int(bool(train_radiance)), _dev(raw, name="raw"), ws.data_ptr(),
        ws.numel(), _stream()), "nerfart_volsdf_render_bwd2")


def neus_render_bwd(surf_blob, rad_blob, view_tiles: int, multires: int, rays_o, rays_d, d_all, g_rgb, raw, *, s: float, white_bkgd: bool = False,
                    w_eikonal: float = 0.0, eik_group_rays: int = 0, train_radiance: bool = False, g_acc=None, state=None):
    """The same for NeuS (neus.py:520-576): state = (sdf [R P], nabla [R P, 3]) at the samples or None."""
    R, P = d_all.shape
    need_term(surf_blob, "bf16", "nerfart_neus_render_bwd"); need_term(rad_blob, "bf16", "nerfart_neus_render_bwd")
    sdf, nab = state if state is not None else (None, None)
    nb = int(lib.nerfart_neus_render_bwd_workspace_bytes(R, P, int(state is not None)))
    ws = _workspace(nb, d_all.device)
    _check(lib.nerfart_neus_render_bwd(
        _dev(surf_blob), _dev(rad_blob), int(view_tiles), int(multires), _dev(rays_o, name="rays_o"), _dev(rays_d, name="rays_d"), R, P,
        _dev(d_all, name="d_all"), _dev(g_rgb, name="g_rgb"), _dev(g_acc, name="g_acc"), _dev(sdf, name="sdf_state"), _dev(nab, name="nabla_state"),
        float(s), int(bool(white_bkgd)), float(w_eikonal), int(eik_group_rays or 0), int(bool(train_radiance)), _dev(raw, name="raw"),
        ws.data_ptr(), ws.numel(), _stream()), "nerfart_neus_render_bwd")


def sdf_param_bwd(surf_blob, multires: int, pts, nbar, raw, sbar=None, hbar7=None):
    """Parameter gradients of sbar . sdf + hbar7 . h7 + nbar . grad_x sdf at pts [M, 3], accumulated into `raw`."""
    M = pts.shape[0]
    need_term(surf_blob, "bf16", "nerfart_sdf_param_bwd")
    nb = int(lib.nerfart_sdf_param_bwd_workspace_bytes(M))
    ws = _workspace(nb, pts.device)
    _check(lib.nerfart_sdf_param_bwd(_dev(surf_blob), int(multires), _dev(pts, name="pts"), M, _dev(sbar, name="sbar"), _dev(hbar7, name="hbar7"),
                                     _dev(nbar, name="nbar"), _dev(raw, name="raw"), ws.data_ptr(), ws.numel(), _stream()), "nerfart_sdf_param_bwd")


def radiance_param_bwd(rad_blob, view_tiles: int, pts, view, nabla, h7, g_rgb, raw, train_radiance: bool = True):
    """(rgb [M,3], g_h7 [M,256], g_n [M,3]); the radiance net's (and the geometry-feature rows') gradients accumulated into `raw`."""
    M = pts.shape[0]
    dev = pts.device
    rgb = torch.empty(M, 3, dtype=torch.float32, device=dev)
    g_h7 = torch.empty(M, 256, dtype=torch.float32, device=dev)
    g_n = torch.empty(M, 3, dtype=torch.float32, device=dev)
    nb = int(lib.nerfart_radiance_param_bwd_workspace_bytes(M))
    ws = _workspace(nb, dev)
    _check(lib.nerfart_radiance_param_bwd(_dev(rad_blob), int(view_tiles), _dev(pts, name="pts"), _dev(view, name="view"), _dev(nabla, name="nabla"),
                                          _dev(h7, name="h7"), M, _dev(g_rgb, name="g_rgb"), _dev(rgb), _dev(g_h7), _dev(g_n), int(bool(train_radiance)),
                                          _dev(raw, name="raw"), ws.data_ptr(), ws.numel(), _stream()), "nerfart_radiance_param_bwd")
    return rgb, g_h7, g_n


def folded_grads_layout(multires: int, multires_view: int):
    """(offsets [29], total): float offsets of (dW_l, db_l) for the SDF net's layers 0..8, then the radiance net's 0..4."""
    offs = (C.c_longlong * 29)()
    total = int(lib.nerfart_folded_grads_layout(int(multires), int(multires_view), offs))
    return [int(o) for o in offs], total


def fold_weight_grads(raw, multires: int, multires_view: int):
    """raw -> (folded [total] fp32, offsets): gradients of the folded weights / biases in the reference's feature order."""
    offs, total = folded_grads_layout(multires, multires_view)
    folded = torch.empty(total, dtype=torch.float32, device=raw.device)
    _check(lib.nerfart_fold_weight_grads(_dev(raw, name="raw"), int(multires), int(multires_view), _dev(folded), _stream()), "nerfart_fold_weight_grads")
    return folded, offs


def weight_norm_bwd(dW, weight_v, weight_g):
    """(g_weight_v [out, in], g_weight_g [out, 1]) of nn.utils.weight_norm for d loss / d W = dW [out, in]."""
    out_f, in_f = weight_v.shape
    g_v = torch.empty_like(weight_v)
    g_g = torch.empty_like(weight_g)
    _check(lib.nerfart_weight_norm_bwd(_dev(dW, name="dW"), _dev(weight_v, name="weight_v"), _dev(weight_g, name="weight_g"), out_f, in_f, _dev(g_v),
                                       _dev(g_g), 0, _stream()), "nerfart_weight_norm_bwd")
    return g_v, g_g


def volsdf_render(surf_blob, rad_blob, view_tiles, rays_o, rays_d, *, near, far, R_bg, alpha, beta, eps=0.1,
                  n_samples=128, n_importance=64, max_upsample_steps=5, max_bisection_steps=10, white_bkgd=False,
                  calc_normal=True, detailed=False, k3_rays_chunk=8192, precision=0, u_final=None, sampler=None, guard: float = 0.0,
                  radiance=None, stats=None, late_round: int = 0):
    """One chunk of rays through nerfart_volsdf_render_staged2_fwd (late_round: the guarded sampler's third rule, hip.volsdf_fine_sample).  Returns a dict of flat [R, ...] tensors.
    u_final [R, n_importance]: uniform random numbers of the final samples (perturb=True); None: deterministic.
    sampler = (surface blob, precision id): Algorithm 1 on its own blob / precision; None: the model's.  guard > 0: the guarded sampler (marginal
    and never-converged rays sampled again on (surf_blob, precision)).  radiance = (radiance blob, precision id): the radiance net of the final
    samples on its own blob / precision; None: (rad_blob, precision).  stats (dict): 'escalated' / 'rays' accumulated."""
    R = rays_o.shape[0]
    dev = rays_o.device
    P = n_samples + n_importance
    if u_final is not None and tuple(u_final.shape) != (R, n_importance):
        raise ValueError(f"u_final must be [{R}, {n_importance}]")
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out = {"rgb": f(R, 3), "depth_volume": f(R), "mask_volume": f(R)}
    if calc_normal:
        out["normals_volume"] = f(R, 3)
    det = {}
    if detailed:
        det = {"d_vals": f(R, P), "implicit_surface": f(R, P), "implicit_nablas": f(R, P, 3), "radiance": f(R, P, 3),
               "sigma": f(R, P), "p_i": f(R, P - 1), "visibility_weights": f(R, P - 1), "beta_map": f(R), "iter_usage": f(R)}
    nb = lib.nerfart_volsdf_render_workspace_bytes(R, n_samples, n_importance, max_upsample_steps, k3_rays_chunk)
    ws = _workspace(nb, dev)
    g = lambda k: _dev(det.get(k))
    samp_blob, samp_prec = sampler if sampler is not None else (surf_blob, precision)
    rblob, rprec = radiance if radiance is not None else (rad_blob, precision)
    n_esc = C.c_int(0)
    _check(lib.nerfart_volsdf_render_staged2_fwd(
        _dev(surf_blob), int(precision), _dev(rblob, name="rad_blob"), int(rprec), _dev(samp_blob, name="sampler_blob"), int(samp_prec), float(guard),
        int(late_round), int(view_tiles), _dev(rays_o, name="rays_o"), _dev(rays_d, name="rays_d"), R,
        float(near), float(far), float(R_bg), float(alpha), float(beta), float(eps), n_samples, n_importance,
        max_upsample_steps, max_bisection_steps, int(bool(white_bkgd)), k3_rays_chunk,
        _dev(lin_table(n_samples, dev)), _dev(lin_table(4 * n_samples, dev)), _dev(lin_table(4 * n_samples + 2, dev)),
        _dev(lin_table(n_importance, dev) if u_final is None else u_final, name="u_final"), int(u_final is not None),
        _dev(out["rgb"]), _dev(out["depth_volume"]), _dev(out["mask_volume"]), _dev(out.get("normals_volume")),
        g("d_vals"), g("implicit_surface"), g("implicit_nablas"), g("radiance"), g("sigma"), g("p_i"),
        g("visibility_weights"), g("beta_map"), g("iter_usage"), C.byref(n_esc), ws.data_ptr(), ws.numel(), _stream()),
        "nerfart_volsdf_render_staged2_fwd")
    if stats is not None:
        stats["escalated"] = stats.get("escalated", 0) + n_esc.value
        stats["rays"] = stats.get("rays", 0) + R
    out.update(det)
    return out


def volsdf_render_mixed(surf_blob, rad_blob, sampler_blob, sampler_precision: int, view_tiles, rays_o, rays_d, *, near, far, R_bg, alpha, beta, eps=0.1,
                        n_samples=128, n_importance=64, max_upsample_steps=5, max_bisection_steps=10, white_bkgd=False, calc_normal=True,
                        detailed=False, k3_rays_chunk=8192, precision=1, u_final=None, guard: float = 0.0, late_round: int = 0):
    """volsdf_render(..., sampler=(sampler_blob, sampler_precision), guard=guard) restated on the PER-STAGE entry points, in the fused renderer's own order
    (tests: the two must agree bit for bit, every output): the SAMPLER (Algorithm 1: 512 (1 + rounds) SDF queries per ray, no gradient,
    volsdf.py:479) on another blob / precision than the 192 final samples.  The final samples -
    sdf, nabla, radiance, compositing, i.e. every number that reaches a pixel - run at `precision` on (surf_blob, rad_blob); only WHERE the
    64 fine samples sit comes from the cheaper arithmetic.  Same return dict as volsdf_render."""
    R = rays_o.shape[0]
    dev = rays_o.device
    P = n_samples + n_importance
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    dn = normalize_dirs(rays_d)
    d_fine, beta_map, usage = volsdf_fine_sample(sampler_blob, rays_o, dn, near, far, R_bg, alpha, beta, eps, 4 * n_samples, 4 * n_samples, n_importance,
                                                 max_upsample_steps, max_bisection_steps, precision=sampler_precision, u_final=u_final,
                                                 escalate=(surf_blob, precision), guard=guard, late_round=late_round)
    d_coarse = f(R, n_samples)
    _check(lib.nerfart_linspace_depths(_dev(lin_table(n_samples, dev)), n_samples, None, None, float(near), float(far), R, _dev(d_coarse), n_samples,
                                       _stream()), "nerfart_linspace_depths")
    d_all = f(R, P)
    _check(lib.nerfart_sort_concat(R, _dev(d_coarse), n_samples, n_samples, _dev(d_fine), n_importance, n_importance, _dev(d_all), P, _stream()),
           "nerfart_sort_concat")
    sdf, nab, rad = f(R, P), f(R, P, 3), f(R, P, 3)
    ws, nb = nabla_workspace(precision, dev)
    h7 = f(min(k3_rays_chunk, R) * P, 256)
    for c0 in range(0, R, k3_rays_chunk):
        rk = min(k3_rays_chunk, R - c0)
        sl = slice(c0, c0 + rk)
        _check(lib.nerfart_sdf_nabla_fwd_rays(_dev(surf_blob), int(precision), _dev(rays_o[sl]), _dev(dn[sl]), None, _dev(d_all[sl]), rk, P, P, float(R_bg),
                                              _dev(sdf[sl]), _dev(nab[sl]), _dev(h7), _dev(ws, torch.uint8), nb, _stream()), "nerfart_sdf_nabla_fwd_rays")
        _check(lib.nerfart_radiance_fwd_rays(_dev(rad_blob), int(precision), int(view_tiles), _dev(rays_o[sl]), _dev(dn[sl]), None, _dev(d_all[sl]), rk, P, P,
                                             _dev(nab[sl]), _dev(h7), _dev(rad[sl]), _stream()), "nerfart_radiance_fwd_rays")
    out = {"rgb": f(R, 3), "depth_volume": f(R), "mask_volume": f(R)}
    if calc_normal:
        out["normals_volume"] = f(R, 3)
    det = {}
    if detailed:
        det = {"d_vals": d_all, "implicit_surface": sdf, "implicit_nablas": nab, "radiance": rad, "sigma": f(R, P), "p_i": f(R, P - 1),
               "visibility_weights": f(R, P - 1), "beta_map": beta_map, "iter_usage": usage}
    _check(lib.nerfart_volsdf_composite(R, P, _dev(d_all), _dev(sdf), _dev(rad), _dev(nab), float(alpha), float(beta), int(bool(white_bkgd)), _dev(out["rgb"]),
                                        _dev(out["depth_volume"]), _dev(out["mask_volume"]), _dev(out.get("normals_volume")), _dev(det.get("sigma")),
                                        _dev(det.get("p_i")), _dev(det.get("visibility_weights")), _stream()), "nerfart_volsdf_composite")
    out.update(det)
    return out


NEUS_UPSAMPLE_ALGOS = {"official_solution": 0, "direct_use": 1, "direct_more": 2}      # neus.py:242-303


def neus_sample(surf_blob, rays_o, rays_d, *, obj_bounding_radius, n_samples=64, n_importance=64, n_upsample_iters=4, precision=0, u_new=None,
                upsample_algo="official_solution", n_nograd_samples=2048, fixed_s_recp=1 / 64.):
    """The SAMPLER of nerfart_neus_render_algo_fwd on its own, on the stage entry points in the fused renderer's order (near / far, coarse depths,
    SDF queries, up-sampling steps, merges): the P = n_samples + n_importance sorted sample depths [R, P] of every ray, bit-identical to the
    renderer's `d_all` (tests) - what pass 2 of a perturb=True NeuS fine-tune step needs, without rendering a frame to get it (neus.py:240-303 run
    under no_grad: only the depths leave the block)."""
    if upsample_algo not in NEUS_UPSAMPLE_ALGOS:
        raise ValueError(f"upsample_algo must be one of {list(NEUS_UPSAMPLE_ALGOS)}")
    algo = NEUS_UPSAMPLE_ALGOS[upsample_algo]
    if algo == 2 and (4 * int(n_nograd_samples) + max(64, n_importance)) * 4 > 160 * 1024:
        raise NerfartHipError("upsample_algo 'direct_more' keeps 4 x N_nograd_samples floats per ray in the 160 KiB LDS: N_nograd_samples must be <= 10,200")
    R, dev = rays_o.shape[0], rays_o.device
    P = n_samples + n_importance
    if u_new is not None and tuple(u_new.shape) != (R, n_importance):
        raise ValueError(f"u_new must be [{R}, {n_importance}]")
    f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    if R == 0:
        return f(0, P)
    dn = normalize_dirs(rays_d)
    near, far = f(R), f(R)
    _check(lib.nerfart_near_far_from_sphere(_dev(rays_o, name="rays_o"), _dev(dn), R, float(obj_bounding_radius), _dev(near), _dev(far), _stream()),
           "nerfart_near_far_from_sphere")
    d, sd = f(R, P), f(R, P)

    def depths(table, n, out, stride):
        _check(lib.nerfart_linspace_depths(_dev(table), n, _dev(near), _dev(far), 0.0, 0.0, R, _dev(out), stride, _stream()), "nerfart_linspace_depths")

    def query(depth, n, stride, out, out_stride):
        _check(lib.nerfart_sdf_fwd_rays(_dev(surf_blob), int(precision), _dev(rays_o), _dev(dn), None, _dev(depth), R, n, stride, 0.0, _dev(out), out_stride,
                                        _stream()), "nerfart_sdf_fwd_rays")

    def merge(n, d_new, s_new, n_new):
        _check(lib.nerfart_merge_sorted_pairs(R, n, P, n_new, _dev(d), _dev(sd), _dev(d_new), _dev(s_new), _stream()), "nerfart_merge_sorted_pairs")
    depths(lin_table(n_samples, dev), n_samples, d, P)
    query(d, n_samples, P, sd, P)
    n = n_samples
    if algo == 0:
        n_new = n_importance // n_upsample_iters
        table = lin_table(n_new, dev) if u_new is None else u_new.contiguous()
        d_new, s_new = f(R, n_new), f(R, n_new)
        for i in range(n_upsample_iters):
            u_ptr = table.data_ptr() + (4 * i * n_new if u_new is not None else 0)
            _check(lib.nerfart_neus_upsample_step(R, n, P, n_new, 64.0 * (1 << i), _dev(d), _dev(sd), u_ptr, n_importance if u_new is not None else 0,
                                                  _dev(d_new), _stream()), "nerfart_neus_upsample_step")
            query(d_new, n_new, n_new, s_new, n_new)
            merge(n, d_new, s_new, n_new)
            n += n_new
    else:
        bins_d, bins_s, n_bins, cap = d, sd, n_samples, P
        if algo == 2:
            bins_d, bins_s, n_bins, cap = f(R, n_nograd_samples), f(R, n_nograd_samples), int(n_nograd_samples), int(n_nograd_samples)
            depths(lin_table(n_bins, dev), n_bins, bins_d, n_bins)
            query(bins_d, n_bins, n_bins, bins_s, n_bins)
        table = lin_table(n_importance, dev) if u_new is None else u_new.contiguous()
        d_new, s_new = f(R, n_importance), f(R, n_importance)
        _check(lib.nerfart_neus_direct_upsample_step(R, n_bins, cap, n_importance, 1.0 / float(fixed_s_recp), _dev(bins_d), _dev(bins_s), _dev(table),
                                                     n_importance if u_new is not None else 0, _dev(d_new), _stream()), "nerfart_neus_direct_upsample_step")
        query(d_new, n_importance, n_importance, s_new, n_importance)
        merge(n, d_new, s_new, n_importance)
    return d


def neus_render(surf_blob, rad_blob, view_tiles, rays_o, rays_d, *, obj_bounding_radius, s, n_samples=64, n_importance=64,
                n_upsample_iters=4, white_bkgd=False, calc_normal=True, detailed=False, k3_rays_chunk=8192, precision=0,
                u_new=None, upsample_algo="official_solution", n_nograd_samples=2048, fixed_s_recp=1 / 64.):
    """One chunk of rays through nerfart_neus_render_algo_fwd.  u_new [R, n_importance]: uniform random numbers of the
    up-sampling (perturb=True; 'official_solution': round i takes columns i * n_new ..; 'direct_use' / 'direct_more': one inversion
    of all n_importance); None: deterministic."""
    R = rays_o.shape[0]
    dev = rays_o.device
    P = n_samples + n_importance
    if upsample_algo not in NEUS_UPSAMPLE_ALGOS:
        raise ValueError(f"upsample_algo must be one of {list(NEUS_UPSAMPLE_ALGOS)}")
    algo = NEUS_UPSAMPLE_ALGOS[upsample_algo]
    if u_new is not None and tuple(u_new.shape) != (R, n_importance):
        raise ValueError(f"u_new must be [{R}, {n_importance}]")
    f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    out = {"rgb": f(R, 3), "depth_volume": f(R), "mask_volume": f(R)}
    if calc_normal:
        out["normals_volume"] = f(R, 3)
    det = {}
    if detailed:
        det = {"d_all": f(R, P), "implicit_surface": f(R, P), "implicit_nablas": f(R, P, 3), "radiance": f(R, P - 1, 3),
               "cdf": f(R, P), "alpha": f(R, P - 1), "visibility_weights": f(R, P - 1), "d_final": f(R, P - 1)}
    nb = lib.nerfart_neus_render_algo_workspace_bytes(R, n_samples, n_importance, k3_rays_chunk, algo, int(n_nograd_samples))
    ws = _workspace(nb, dev)
    g = lambda k: _dev(det.get(k))
    n_new = n_importance // n_upsample_iters if algo == 0 else n_importance
    _check(lib.nerfart_neus_render_algo_fwd(
        _dev(surf_blob), _dev(rad_blob), int(precision), int(view_tiles), _dev(rays_o, name="rays_o"), _dev(rays_d, name="rays_d"), R,
        float(obj_bounding_radius), float(s), n_samples, n_importance, n_upsample_iters, algo, int(n_nograd_samples), float(fixed_s_recp),
        int(bool(white_bkgd)), k3_rays_chunk,
        _dev(lin_table(n_samples, dev)), _dev(lin_table(int(n_nograd_samples), dev) if algo == 2 else None),
        _dev(lin_table(n_new, dev) if u_new is None else u_new, name="u_new"),
        int(u_new is not None), _dev(out["rgb"]), _dev(out["depth_volume"]), _dev(out["mask_volume"]), _dev(out.get("normals_volume")),
        g("d_all"), g("implicit_surface"), g("implicit_nablas"), g("radiance"), g("cdf"), g("alpha"),
        g("visibility_weights"), g("d_final"), ws.data_ptr(), ws.numel(), _stream()), "nerfart_neus_render_algo_fwd")
    out.update(det)
    return out
