"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/nerfart_hip.h declares,
and its host helper reproduces torch.linspace bit for bit.  No compute calls (no GPU here)."""
import os
import re
import subprocess

import numpy as np
import torch

from conftest import REPO


def _header_symbols():
    src = open(os.path.join(REPO, "include", "nerfart_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nerfart_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from nerfart_amd import hip
    syms = _header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(hip.lib, s), f"{s} declared in include/nerfart_hip.h but not exported by {hip.LIB_PATH}"
    assert set(hip._SIGS) == set(syms), "ctypes signature table and header disagree"
    assert hip.ABI_VERSION == 5


def test_library_is_gfx950_code_object():
    from nerfart_amd import hip
    out = subprocess.run(["strings", "-n", "6", hip.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_linspace_helper():
    """nerfart_linspace implements the scalar ATen formula (the one torch's GPU kernel uses): step =
    (end-start)/(n-1), first half start + step*i, second half end - step*(n-1-i).  torch's CPU kernel is
    vectorised and may differ by one ulp on some entries, which is why the render entry points accept the
    host framework's own tables."""
    from nerfart_amd import hip
    for n in (2, 3, 16, 64, 66, 128, 512, 514, 2048):
        for a, b in ((0.0, 1.0), (0.0, 6.0), (-1.5, 2.25)):
            mine = hip.linspace(a, b, n).numpy()
            step = (np.float32(b) - np.float32(a)) / np.float32(n - 1)
            i = np.arange(n)
            ref = np.where(i < n // 2, np.float32(a) + step * i.astype(np.float32),
                           np.float32(b) - step * (n - 1 - i).astype(np.float32)).astype(np.float32)
            assert np.array_equal(mine, ref), (n, a, b)
            t = torch.linspace(a, b, n).numpy()
            assert np.max(np.abs(mine - t)) <= 2 * np.spacing(np.float32(max(abs(a), abs(b))))


def test_errors_are_reported_not_swallowed():
    from nerfart_amd import hip
    import pytest
    with pytest.raises(hip.NerfartHipError):
        hip.sdf_fwd(torch.zeros(8), torch.zeros(4, 3), 3.0)      # CPU tensors are refused: no CPU path


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    """Argument checks of the round-2 entry points run before any launch: bad shapes / null buffers are errors with a message."""
    import ctypes as C
    from nerfart_amd import hip
    lib = hip.lib
    null = C.c_void_p(0)

    def err():
        return lib.nerfart_last_error().decode()
    assert lib.nerfart_gemm_f16_nt(null, null, 65, 64, 64, null, null) != 0 and "multiples of 64" in err()
    assert lib.nerfart_vgg16_l1_fwd(null, 0, null, 100, 100, null, 0, null, 0, null) != 0 and "H and W" in err()
    assert lib.nerfart_vgg16_l1_fwd(null, 0, null, 224, 224, null, 0, null, 0, null) != 0 and "workspace" in err()
    assert lib.nerfart_clip_vitb32_image_fwd(null, 0, null, 4, null, 1, null, 0, null) != 0 and "null" in err()
    assert lib.nerfart_clip_vitb32_workspace_bytes(0, 1) == 0
    assert lib.nerfart_clip_vitb32_workspace_bytes(16, 1) > 12 * 16 * 50 * 768 * 4
    # the workspace's buffers (host arithmetic only) and the partial backward's refusals, before any launch
    co = (C.c_longlong * 21)()
    for keep in (0, 1):
        ctotal = lib.nerfart_clip_vitb32_workspace_layout(3, keep, C.cast(co, C.c_void_p))
        assert ctotal == co[20] == lib.nerfart_clip_vitb32_workspace_bytes(3, keep) == lib.nerfart_clip_vitb32_workspace_layout(3, keep, null)
        assert list(co[:15]) == sorted(co[:15]) and co[0] == 0 and co[1] == 256 and all(v % 256 == 0 for v in co)
        assert co[2] - co[1] == 2 * 192 * 3072 and co[3] - co[2] == 4 * 192 * 3072 and co[9] - co[8] == 4 * 192 * 768 and co[16] == 0
        assert co[15] == co[19] + 2 * 192 * 3072 and ctotal == co[14] + (12 * co[15] if keep else co[15] + 4 * 192 * 768)
    assert lib.nerfart_clip_vitb32_workspace_layout(0, 1, null) == 0 == lib.nerfart_clip_vitb32_workspace_layout(0, 1, C.cast(co, C.c_void_p))
    assert lib.nerfart_clip_vitb32_image_bwd_partial(null, 0, 1, null, null, null, 0, 0, null) != 0 and "null" in err()
    one_ = C.c_void_p(16)                                          # non-null, never dereferenced: the checks come first
    n1 = lib.nerfart_clip_vitb32_workspace_bytes(1, 1)
    nb = lib.nerfart_clip_vitb32_blob_layout(null)
    for bad in (-1, 13):
        assert lib.nerfart_clip_vitb32_image_bwd_partial(one_, nb, 1, one_, one_, one_, n1, bad, null) != 0 and "stop_layer" in err()
    assert lib.nerfart_clip_vitb32_image_bwd_partial(one_, nb, 1, one_, one_, one_, n1 - 1, 12, null) != 0 and "workspace too small" in err()
    assert lib.nerfart_clip_vitb32_image_bwd_partial(one_, nb, 1, null, one_, one_, n1, 12, null) != 0 and "null g_feat" in err()
    assert lib.nerfart_clip_vitb32_image_bwd_partial(one_, nb, 1, one_, null, one_, n1, 0, null) != 0 and "null g_feat" in err()
    assert lib.nerfart_clip_vitb32_image_bwd(one_, nb, 1, one_, null, one_, n1, null) != 0 and "null g_feat" in err()
    assert lib.nerfart_resample_fwd(null, 2, 3, 8, 8, 0, 0, 8, 8, 4, 4, 1, null, null, null, null, 3, 4, 4, null) != 0 and "n_src" in err()
    assert lib.nerfart_resample_fwd(null, 1, 3, 8, 8, 0, 0, 8, 8, 4, 4, 7, null, null, null, null, 1, 4, 4, null) != 0 and "mode" in err()
    assert lib.nerfart_clip_style_heads(null, 17, null, null, null, null, 8, 79, 1.0, 0.2, 0.1, 2.0, 0.07, null, null, null) != 0 and "n_patches" in err()
    assert lib.nerfart_first_crossing(null, null, 5, 1, 0.0, null, null, null, null, null, null) != 0 and "n_steps" in err()
    assert lib.nerfart_first_crossing(null, null, 0, 256, 0.0, null, null, null, null, null, null) == 0          # no rays: nothing to do
    # round 3: the reverse-mode grad(SDF) scratch is the caller's (no hipMalloc inside the library)
    assert lib.nerfart_sdf_nabla_workspace_bytes(1) == 256 * 7 * 8 * 8 * 1024 and lib.nerfart_sdf_nabla_workspace_bytes(0) > 0
    assert lib.nerfart_sdf_nabla_workspace_bytes(2) == 0 and lib.nerfart_sdf_nabla_workspace_bytes(3) == 0
    one = C.c_void_p(16)                                           # a non-null, never dereferenced pointer: the checks come first
    assert lib.nerfart_sdf_nabla_fwd(one, 1, one, 4, 3.0, one, one, null, null, 0, null) != 0 and "workspace" in err()
    assert lib.nerfart_sdf_nabla_fwd(one, 1, one, 4, 3.0, one, one, null, one, 1024, null) != 0 and "workspace" in err()
    offs = (C.c_longlong * 22)()
    total = lib.nerfart_vgg16_blob_layout(C.cast(offs, C.c_void_p))
    assert offs[21] == total and total > 2 * 2 * (64 * 64 + 9 * (64 * 64 + 64 * 128 + 128 * 128 + 128 * 256 + 2 * 256 * 256))
    # the workspace's buffers (host arithmetic only): loss, cols, y[0..6], p[0], p[1], ga, gb, dcols, total - the total is _workspace_bytes'
    wo = (C.c_longlong * 15)()
    for keep in (0, 1):
        wtotal = lib.nerfart_vgg16_workspace_layout(32, 64, keep, C.cast(wo, C.c_void_p))
        assert wtotal == wo[14] == lib.nerfart_vgg16_workspace_bytes(32, 64, keep) == lib.nerfart_vgg16_workspace_layout(32, 64, keep, null)
        assert list(wo) == sorted(wo) and wo[0] == 0 and wo[1] == 256 and wo[2] - wo[1] == 4 * 2 * 32 * 64 * 32 and wo[3] - wo[2] == 4 * 2 * 32 * 64 * 64
        assert wo[10] - wo[9] == 4 * 2 * 16 * 32 * 64 and wo[11] - wo[10] == 4 * 2 * 8 * 16 * 128
        assert (wo[12] - wo[11] == wo[13] - wo[12] == wo[14] - wo[13] == 4 * 32 * 64 * 64) if keep else (wo[11] == wo[14])
    assert lib.nerfart_vgg16_workspace_layout(4, 64, 1, null) == 0


def test_ctypes_signatures_have_the_headers_argument_counts_and_kinds():
    """Every prototype of include/nerfart_hip.h against hip._SIGS: same number of arguments, pointers where the header has pointers,
    64-bit integers where it says `long long`, floats where it says `float` - an argument added to the header (the workspace pair of
    nerfart_sdf_nabla_fwd, round 3) cannot be forgotten in the binding."""
    import ctypes as C
    from nerfart_amd import hip
    src = open(os.path.join(REPO, "include", "nerfart_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = re.findall(r"\b([a-z][a-z ]*?[\s\*]+)(nerfart_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert len(protos) >= 55
    for ret, name, args in protos:
        args = " ".join(args.split())
        params = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
        restype, argtypes = hip._SIGS[name]
        assert len(argtypes) == len(params), f"{name}: header has {len(params)} arguments, hip._SIGS {len(argtypes)}"
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p or t is C.c_char_p, (name, p, t)
            elif p.startswith("long long") or p.startswith("unsigned long long") or p.startswith("size_t"):
                assert t is C.c_longlong, (name, p, t)
            elif p.startswith("float"):
                assert t is C.c_float, (name, p, t)
            elif p.startswith("int") or p.startswith("unsigned"):
                assert t is C.c_int, (name, p, t)


def test_render_bwd_entry_points_validate_their_arguments_without_a_gpu():
    from nerfart_amd import hip
    lib, null = hip.lib, None
    assert lib.nerfart_volsdf_render_bwd(null, null, 1, 6, null, null, 4, 192, null, null, null, null, null, null, null, 3.0, 100.0, 0.01, 0, 0.1, 0, 1,
                                         null, null, 0, null) != 0 and b"null" in lib.nerfart_last_error()
    assert lib.nerfart_volsdf_render_bwd(null, null, 1, 6, null, null, 20000, 192, null, null, null, null, null, null, null, 3.0, 100.0, 0.01, 0, 0.1, 0, 1,
                                         null, null, 0, null) != 0 and b"2^21" in lib.nerfart_last_error()
    assert lib.nerfart_neus_render_bwd(null, null, 2, 6, null, null, 4, 128, null, null, null, null, null, 20.0, 0, 0.1, 0, 0, null, null, 0, null) != 0
    assert b"view_tiles" in lib.nerfart_last_error()
    assert lib.nerfart_volsdf_render_bwd_workspace_bytes(1200, 192, 1) < lib.nerfart_volsdf_render_bwd_workspace_bytes(1200, 192, 0)


def test_an_architecture_the_kernels_are_not_written_for_is_refused_before_packing():
    """nerfart_pack_*_blob index their pointer tables and the device tensors with the fixed dims of the four shipped configs; a
    YAML-reachable variant (surface.W 512, D 6, skips [], W_geometry_feature 128, radiance W / D) must be a NotImplementedError at model
    construction - from the library's own dims (nerfart_pack_layer_dims) - not an out-of-bounds read on the GPU."""
    import pytest
    from nerfart_amd import hip, nets
    assert hip.pack_layer_dims(False, 6) == [(256, 39), (256, 256), (256, 256), (217, 256)] + [(256, 256)] * 4 + [(257, 256)]
    assert hip.pack_layer_dims(True, 1) == [(256, 265)] + [(256, 256)] * 3 + [(3, 256)]
    assert hip.pack_layer_dims(True, 3)[0] == (256, 289)
    with pytest.raises(NotImplementedError):
        hip.pack_layer_dims(False, 4)
    nets.VolSDF(W_geo_feat=256)                                                       # the shipped architecture constructs
    nets.NeuS(W_geo_feat=256, radiance_cfg={"embed_multires_view": 4})
    for bad in (dict(surface_cfg={"W": 512}), dict(surface_cfg={"D": 6}), dict(surface_cfg={"skips": []}), dict(surface_cfg={"skips": [3]}),
                dict(W_geo_feat=128), dict(radiance_cfg={"W": 128}), dict(radiance_cfg={"D": 3}), dict(surface_cfg={"embed_multires": 4})):
        with pytest.raises(NotImplementedError):
            nets.VolSDF(**dict(dict(W_geo_feat=256), **bad))
    # the pack wrappers hold the tensors themselves to the same dims (a state dict loaded into a hand-built module list)
    g = [torch.zeros(256, 1)] * 9; v = [torch.zeros(256, 256)] * 9; b = [torch.zeros(256)] * 9
    with pytest.raises(NotImplementedError):
        hip.pack_surface_blob(1, 6, g, v, b)
    with pytest.raises(NotImplementedError):
        hip.pack_surface_blob(1, 6, g[:7], v[:7], b[:7])


def test_rayschunk_is_read_as_the_memory_hint_it_is():
    """volsdf.launch_rays: the reference's rayschunk values (1024 / 2048 / 2000: render.py:488,614, volsdf.py:720,990) never shrink a launch below the
    library's own size unless the caller insists or the chunking is observable (perturb=True drawing from torch's generator per chunk)."""
    from nerfart_amd.volsdf import launch_rays, DEFAULT_RAYSCHUNK
    assert launch_rays(None, DEFAULT_RAYSCHUNK) == DEFAULT_RAYSCHUNK
    assert launch_rays(1024, DEFAULT_RAYSCHUNK) == DEFAULT_RAYSCHUNK and launch_rays(2048, DEFAULT_RAYSCHUNK) == DEFAULT_RAYSCHUNK
    assert launch_rays(1 << 20, DEFAULT_RAYSCHUNK) == 1 << 20                       # a LARGER request is honoured
    assert launch_rays(1024, DEFAULT_RAYSCHUNK, honor_rayschunk=True) == 1024
    assert launch_rays(1024, DEFAULT_RAYSCHUNK, perturb=True) == 1024                # draws per chunk: keep the caller's chunking
    assert launch_rays(1024, DEFAULT_RAYSCHUNK, perturb=True, uniforms=torch.zeros(1, 64)) == DEFAULT_RAYSCHUNK


def test_direct_more_refuses_a_bin_count_that_cannot_fit_the_lds():
    """N_nograd_samples is YAML-reachable (neus.py:735); ~10k+ bins per ray exceed the 160 KiB LDS of k_neus_upsample - refused up
    front with the limit in the message, not as a generic launch error from inside a render."""
    import ctypes as C
    from nerfart_amd import hip
    null = C.c_void_p(0)
    args = lambda nn: [null, null, 1, 3, null, null, 8, 1.0, 64.0, 64, 64, 4, 2, nn, 1 / 64., 0, 8192] + [null] * 3 + [0] + [null] * 12 + [null, 0, null]
    assert hip.lib.nerfart_neus_render_algo_fwd(*args(20000)) != 0 and "10,200" in hip.lib.nerfart_last_error().decode()
    assert hip.lib.nerfart_neus_render_algo_fwd(*args(2048)) != 0 and "10,200" not in hip.lib.nerfart_last_error().decode()      # passes THIS check (then: no workspace)


def test_stage_entry_points_refuse_rows_that_do_not_fit_their_stride():
    """The exported per-ray stage entry points take the row stride `cap` from the caller: n < 2, n > cap and (merge check) n + n_up > cap are refused
    with a message before any HIP call - here with null buffers, so nothing is launched."""
    import ctypes as C
    from nerfart_amd import hip
    lib, null = hip.lib, C.c_void_p(0)

    def err():
        return lib.nerfart_last_error().decode()

    def first_check(n, cap):
        return lib.nerfart_volsdf_first_check(1, n, cap, 64, 0.1, 100.0, 0.01, null, null, null, 0, 1.0, null, 6.0, null, null, null, null, null, null, null)

    def upsample(n, cap):
        return lib.nerfart_volsdf_upsample(1, n, cap, 512, null, null, null, null, null, 1, null, null)

    def merge_check(n, cap, n_up):
        return lib.nerfart_volsdf_merge_check(1, n, cap, n_up, 64, 10, 1, 0.1, 100.0, 0.01, null, null, null, null, null, null, null, null, 0,
                                              null, null, null, null, null, null, null)

    def finalize(n, cap):
        return lib.nerfart_volsdf_finalize(1, n, cap, 64, null, null, null, null, 0, null, null, null, null, null)

    for name, call in (("volsdf_first_check", first_check), ("volsdf_upsample", upsample), ("volsdf_finalize", finalize),
                       ("volsdf_merge_check", lambda n, cap: merge_check(n, cap + 512, 512))):
        for n, cap in ((1, 512), (0, 512), (513, 512), (4096, 2048)):
            assert call(n, cap) == 2, (name, n, cap)
            assert name in err() and "cap" in err(), err()
    assert lib.nerfart_volsdf_upsample(0, 1, 0, 512, null, null, null, null, null, 1, null, null) == 0     # an empty launch stays a no-op
    assert lib.nerfart_volsdf_finalize(0, 0, 0, 64, null, null, null, null, 0, null, null, null, null, null) == 0
    assert merge_check(512, 1023, 512) == 2 and "exceeds the row capacity" in err()
    assert merge_check(1536, 2047, 512) == 2 and "exceeds the row capacity" in err()
    for direct in (0, 1):
        step = lib.nerfart_neus_direct_upsample_step if direct else lib.nerfart_neus_upsample_step
        assert step(1, 65, 64, 16, 64.0, null, null, null, 0, null, null) == 2 and "cap" in err()
        assert step(1, 1, 64, 16, 64.0, null, null, null, 0, null, null) == 2 and "n >= 2" in err()


def test_render_workspace_sizes_are_the_sums_of_their_documented_buffers():
    """The forward renderers' workspaces are caller-allocated and carved in a fixed order, every buffer rounded up to 256 bytes (and the
    sampler's escalation run relies on its buffers sitting behind everything a smaller run carves): the four byte-count queries against the
    layouts written out here, buffer by buffer in carving order.  Host arithmetic only."""
    from nerfart_amd import hip
    lib = hip.lib
    total = lambda sizes: sum((b + 255) // 256 * 256 for b in sizes)
    nabla_ws = 256 << 20        # grad(SDF) scratch, sized for either precision: the fp32 kernel's 1 MiB per CU, 256 CUs (also the count assumed without a GPU)

    def sampler(R, n_init, n_up, n_final, max_iter):
        cap = n_init + max_iter * n_up
        return total([4 * R * cap] * 4                              # dA, sA, dB, sB
                     + [4 * R * n_up] * 2 + [4 * R]                 # d_new, s_new, beta_plus
                     + [4 * R] * 2 + [4 * 64]                       # act0, act1, count (64 counters)
                     + [4 * n_init, 4 * (n_up + 2), 4 * n_final]    # t_init, u_up, u_final
                     + [4 * R]                                      # esc_list; then the compacted rays of the escalation run and its outputs:
                     + [12 * R] * 2 + [4 * R] * 2                   # c_o, c_dn, c_near, c_far
                     + [4 * R * n_final] * 2 + [4 * R] * 2)         # c_u, c_d_fine, c_beta, c_iter

    def volsdf(R, ns, ni, max_iter, k3):
        P, rk = ns + ni, min(k3, R)
        return total([12 * R, 4 * R * ni, 4 * R * ns, 4 * ns]       # rays_dn, d_fine, d_coarse, t_coarse
                     + [4 * R * P] * 2 + [12 * R * P] * 2           # d_all, sdf, nabla, rad
                     + [4 * R] * 2                                  # beta_map, iter_usage
                     + [4 * rk * P * 256]                           # h7 of one radiance chunk
                     + [sampler(R, 4 * ns, 4 * ns, ni, max_iter), nabla_ws])

    def neus(R, ns, ni, k3, n_more):
        P, rk = ns + ni, min(k3, R)
        return total([12 * R, 4 * R, 4 * R, 4 * ns, 4 * (ni + 64)]  # rays_dn, near, far, t_coarse, u_new
                     + [4 * R * P] * 2 + [4 * R * ni] * 2           # d, s, d_new, s_new
                     + [4 * R * (P - 1), 4 * R * P, 12 * R * P]     # d_mid, sdf, nabla
                     + [12 * rk * (P - 1), 4 * rk * (P - 1)]        # nabla_mid, sdf_mid of one radiance chunk
                     + [12 * R * (P - 1), 4 * rk * (P - 1) * 256]   # rad, h7
                     + [nabla_ws]
                     + [4 * n_more] + [4 * R * n_more] * 2)         # 'direct_more' only: t_more, d_more, s_more

    for R, ns, ni, max_iter, k3 in ((1, 2, 1, 0, 1), (3, 8, 5, 2, 2), (1200, 128, 64, 5, 512)):
        assert lib.nerfart_volsdf_sampler_workspace_bytes(R, 4 * ns, 4 * ns, ni, max_iter) == sampler(R, 4 * ns, 4 * ns, ni, max_iter)
        assert lib.nerfart_volsdf_render_workspace_bytes(R, ns, ni, max_iter, k3) == volsdf(R, ns, ni, max_iter, k3)
        assert lib.nerfart_neus_render_workspace_bytes(R, ns, ni, k3) == neus(R, ns, ni, k3, 0)
        for n_nograd in (2, 2048):
            assert lib.nerfart_neus_render_algo_workspace_bytes(R, ns, ni, k3, 2, n_nograd) == neus(R, ns, ni, k3, n_nograd)


def test_composite_entry_points_refuse_rows_without_an_interval():
    """nerfart_volsdf_composite / nerfart_neus_composite integrate P - 1 intervals: P < 2 is refused with a message after the empty-launch return and
    before any HIP call (with P <= 0 and the detail outputs set, lane 0 would read and write outside the row) - here with null buffers.  The two
    backwards refuse P < 2 and P > 513 the same way."""
    import ctypes as C
    from nerfart_amd import hip
    lib, null = hip.lib, C.c_void_p(0)

    def err():
        return lib.nerfart_last_error().decode()

    def volsdf(n_rays, P):
        return lib.nerfart_volsdf_composite(n_rays, P, null, null, null, null, 100.0, 0.01, 0, null, null, null, null, null, null, null, null)

    def neus(n_rays, P):
        return lib.nerfart_neus_composite(n_rays, P, null, null, null, null, 64.0, 0, null, null, null, null, null, null, null, null, null)

    def volsdf_bwd(n_rays, P):
        return lib.nerfart_volsdf_composite_bwd(n_rays, P, null, null, null, 100.0, 0.01, 0, null, null, null, null, null, null)

    def neus_bwd(n_rays, P):
        return lib.nerfart_neus_composite_bwd(n_rays, P, null, null, 64.0, 0, null, null, null, null, null, null)

    for name, call in (("volsdf_composite", volsdf), ("neus_composite", neus)):
        for P in (1, 0, -1, -2147483647):
            assert call(1, P) == 2, (name, P)
            assert name in err() and "P >= 2" in err(), err()
        assert call(0, 0) == 0 and call(0, 192) == 0 and call(-1, 1) == 0           # an empty launch stays a no-op
    for call in (volsdf_bwd, neus_bwd):
        for P in (1, 0, 514, 1025):
            assert call(1, P) == 2 and "2 <= P <= 513" in err(), (P, err())
        assert call(0, 0) == 0


def test_per_sample_backward_entry_points_refuse_null_pointers_without_a_gpu():
    """nerfart_sdf_fwd2 / nerfart_sdf_bwd2 / nerfart_radiance_fwd_dump / nerfart_radiance_bwd refuse every NULL pointer argument, blob included, with a
    message that names it, and more than 2^21 points, before any launch: non-null dummies that are never dereferenced, one NULL at a time."""
    import ctypes as C
    from nerfart_amd import hip
    lib, null, one = hip.lib, None, C.c_void_p(16)

    def err():
        return lib.nerfart_last_error().decode()

    M = 4
    calls = {
        "sdf_fwd2": (("surf_blob", "pts", "dir", "f2_dump"),
                     lambda p, m: lib.nerfart_sdf_fwd2(p["surf_blob"], p["pts"], p["dir"], m, p["f2_dump"], null)),
        "sdf_bwd2": (("surf_blob", "gbar_h7", "gbar_sdf", "f2_dump", "r2_dump"),
                     lambda p, m: lib.nerfart_sdf_bwd2(p["surf_blob"], m, p["gbar_h7"], p["gbar_sdf"], p["f2_dump"], p["r2_dump"], null)),
        "radiance_fwd_dump": (("rad_blob", "pts", "view", "nabla", "h7", "rgb_out", "dump"),
                              lambda p, m: lib.nerfart_radiance_fwd_dump(p["rad_blob"], 1, p["pts"], p["view"], m, p["nabla"], p["h7"], p["rgb_out"],
                                                                         p["dump"], null)),
        "radiance_bwd": (("rad_blob", "rgb", "g_rgb", "fwd_dump", "bwd_dump", "g_h7_out", "g_n_out"),
                         lambda p, m: lib.nerfart_radiance_bwd(p["rad_blob"], m, p["rgb"], p["g_rgb"], p["fwd_dump"], p["bwd_dump"], p["g_h7_out"],
                                                               p["g_n_out"], null)),
    }
    for who, (names, call) in calls.items():
        for bad in names:
            ptrs = {n: (null if n == bad else one) for n in names}
            assert call(ptrs, M) != 0, (who, bad)
            assert who in err() and bad + " is NULL" in err(), (who, bad, err())
        ptrs = {n: one for n in names}
        for m in ((1 << 21) + 1, 1 << 30):
            assert call(ptrs, m) != 0 and who in err() and "2^21" in err(), (who, m, err())
        assert call(ptrs, -1) != 0 and "M out of range" in err()
        assert call({n: null for n in names}, 0) == 0                               # no points: nothing to do
