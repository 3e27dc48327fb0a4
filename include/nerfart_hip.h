/* nerfart_hip.h - C ABI of libnerfart_hip.so: the MI355X (gfx950) hot path of cassiePython/NeRF-Art.
 *
 * The reference (pure Python/PyTorch, no FFI of its own) exposes this path as Python callables;
 * each entry point below names the reference callable (file:line under the reference tree) it
 * replaces.  SURVEY.md section 8b lists the boundaries B1-B3; INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 (int32 / int64 where typed so) unless a
 *     parameter is documented as host; outputs are caller-allocated; nothing is retained.
 *   - `stream` is a hipStream_t (0 = default stream); all work is enqueued on it.  Entry points
 *     with a data-dependent loop (fine_sample, render) synchronise that stream internally.
 *   - return value 0 = success; non-zero = failure, message via nerfart_last_error() (thread local).
 *   - `blob` arguments are weight blobs produced by nerfart_amd/packing.py (layout documented
 *     there and in DESIGN.md): `surf_blob` = SDF net, `rad_blob` = geometry-feature rows + radiance net.
 *   - `precision` selects the matrix-core path AND the blob format it expects:
 *       0 = fp32-exact (v_mfma_f32_16x16x4_f32; blobs from surface_plan()/radiance_plan()).  nerfart_sdf_nabla_fwd* runs
 *           REVERSE mode (k_sdf_grad: forward sweep + transposed chunks of the same blob, softplus' parked as fp32 in the
 *           caller's workspace); precision 3 (these two entry points only) selects the forward-mode tangent quads of
 *           k_sdf_nabla on the same blob (cross-checks),
 *       1 = split bf16 "bf16x3" (3 x v_mfma_f32_16x16x32_bf16 per k-step on hi/lo operand splits, ~2^-16
 *           relative per product; blobs from surface_plan_bf16()/radiance_plan_bf16()).  nerfart_sdf_nabla_fwd*
 *           then runs REVERSE mode too (forward sweep + transposed-weight sweep in one kernel, softplus' as unorm16 in the
 *           caller's workspace); precision 2 (these two entry points only) selects the forward-mode tangent kernel on the
 *           same blob (cross-checks).
 *       4 = "fp16x2" (csrc/mlp_chain_f16x2.hip): the split-bf16 kernels' data flow with the 2-MFMA split - ONE fp16 activation term
 *           x fp16 hi + lo weight terms, 2 x v_mfma_f32_16x16x32_f16 per product (11-bit activations, TF32 class; blobs from
 *           surface_plan_bf16(term="fp16") / radiance_plan_bf16(term="fp16")).  A MEASUREMENT variant of the three forward
 *           kernels (inference entry points only; workspace as precision 1), never a default - DESIGN.md 4.1b.  It is the arithmetic of
 *           Algorithm 1's sampler in the shipped `mixed` mode (nerfart_volsdf_render_staged_fwd's sampler_precision, guarded).
 *       5 = "fp16x1" (csrc/mlp_chain_f16x1.hip; nerfart_sdf_fwd / nerfart_sdf_fwd_rays and the SAMPLER arguments of nerfart_volsdf_fine_sample[_guarded] /
 *           nerfart_volsdf_render_mixed_fwd / _staged_fwd only - every other entry point refuses it): K2 with ONE v_mfma_f32_16x16x32_f16 per
 *           product (one fp16 activation term x one fp16 weight term) in a SCALED softplus recursion (accumulators z' = c z, activations a' = c softplus(z),
 *           c = 100 log2 e).  Its blob: nerfart_pack_surface_blob(precision = 5, ...) - the precision-4 layout under encoding word 3 - from tensors the CALLER
 *           hands over in that recursion (layer 0's weights, the skip layer's encoding columns and the hidden biases times c, the last layer's rows / c) with the
 *           hidden layers' folded weights on the fp16 grid; for rendering, ERROR-COMPENSATED ones (nerfart_amd/calibrate.py).  The library
 *           refuses a precision-4 blob at precision 5 and vice versa.  No value that reaches a pixel and no gradient is computed in it.
 *   - point sources: either an explicit array pts[M,3], or ("_rays" variants) rays + per-ray depths:
 *     point m = slot m / n_per_ray, sample m % n_per_ray, ray = ray_idx ? ray_idx[slot] : slot,
 *     x = rays_o[ray] + rays_d[ray] * depth[slot * depth_stride + sample]  (two roundings, as the
 *     reference's separate mul and add).
 */
#ifndef NERFART_HIP_H
#define NERFART_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (round 6, second session; since then additions only, marked "addition to ABI 5" where they are declared: the mesh entry points,
 * nerfart_volsdf_composite_geo_bwd, nerfart_volsdf_render_bwd2).  History: 4 -> 5, additions only: nerfart_volsdf_fine_sample_guarded2 / nerfart_volsdf_render_staged2_fwd (the guarded sampler's
 * `late_round`), C-ABI precision 5 on the SDF-only entry points.
 * 3 -> 4, additions only: the guarded sampler (nerfart_volsdf_fine_sample_guarded) and the per-stage-precision renderer
 * (nerfart_volsdf_render_staged_fwd), nerfart_pack_layer_dims, nerfart_geometry_feature.
 * 2 -> 3, additions only (every version-2 entry point keeps its signature): the weight-blob packers
 * (nerfart_pack_surface_blob / nerfart_pack_radiance_blob + size queries; header word 10 of a split blob now names its fragment encoding),
 * nerfart_neus_render_algo_fwd / nerfart_neus_direct_upsample_step (upsample_algo 'direct_use' / 'direct_more').  1 -> 2: nerfart_sdf_nabla_fwd[_rays] take a caller-owned workspace; the CLIP blob stores every matrix once; the
 * VGG blob is fp32; the CLIP / VGG entry points take blob_bytes and reject blobs of another layout; new: the ray-level backward
 * (nerfart_*_render_bwd, nerfart_sdf_param_bwd, nerfart_fold_weight_grads, nerfart_weight_norm_bwd). */
int nerfart_abi_version(void);
const char* nerfart_last_error(void);

/* Optional launch profiling (bench.py): between begin and end every chained-MLP launch and every 256-column weight-gradient
 * launch is bracketed by HIP events on its own stream; end() returns per kernel class c = 0 k_sdf_only, 1 k_sdf_nabla / k_sdf_grad,
 * 2 k_radiance (units = points processed), 3 k_wgrad<256> (units = algorithmic bytes: both bf16 operands read once) the summed
 * elapsed ms, launch count and units (host arrays of 4). */
int nerfart_profile_begin(void);
int nerfart_profile_end(double* ms, long long* launches, long long* units);
/* (ABI 4) The same with host arrays of 5: class 4 = the SDF queries of the guarded sampler's ESCALATION run (nerfart_volsdf_fine_sample_guarded: the rays
 * sampled again, on the escalation blob) - kept out of class 0, so that class 0 is the dominant kernel's own launches; nerfart_profile_end drops it. */
int nerfart_profile_end5(double* ms, long long* launches, long long* units);

/* host helper: torch.linspace(start, end, n) in fp32, bit for bit (out is a HOST array). */
void nerfart_linspace(float start, float end, int n, float* out);

/* ---- B3: SDF query.  ImplicitSurface.forward (models/base.py:243-263) + VolSDF.forward_surface
 * sphere clamp sdf = min(sdf, R_bg - |x|) (models/frameworks/volsdf.py:341-347); R_bg <= 0: no clamp
 * (NeuS, neus.py:277,299). */
int nerfart_sdf_fwd(const float* surf_blob, int precision, const float* pts, long long M, float R_bg, float* sdf_out, void* stream);
int nerfart_sdf_fwd_rays(const float* surf_blob, int precision, const float* rays_o, const float* rays_d, const int* ray_idx,
                         const float* depth, int n_slots, int n_per_ray, int depth_stride, float R_bg,
                         float* sdf_out, int out_stride, void* stream);

/* ---- B2 (first half): ImplicitSurface.forward_with_nablas (models/base.py:265-282) + the clamp of
 * VolSDF.forward_surface_with_nablas (volsdf.py:349-357; nabla is NOT replaced).  Outputs sdf[M],
 * nabla[M,3] and, if h7_out != NULL, the layer-7 activation h7[M,256] consumed by nerfart_radiance_fwd.
 * workspace: nerfart_sdf_nabla_workspace_bytes(precision) bytes of device memory owned by the CALLER (PyTorch's caching
 * allocator in the Python host), uninitialised, private to the call until the stream has passed it: the
 * reverse-mode kernels park softplus'(z_l) of the forward sweep there (one region per resident workgroup; precisions 2 / 3
 * need none and accept NULL).  The library allocates no device memory. */
long long nerfart_sdf_nabla_workspace_bytes(int precision);
int nerfart_sdf_nabla_fwd(const float* surf_blob, int precision, const float* pts, long long M, float R_bg, float* sdf_out,
                          float* nabla_out, float* h7_out, void* workspace, long long workspace_bytes, void* stream);
int nerfart_sdf_nabla_fwd_rays(const float* surf_blob, int precision, const float* rays_o, const float* rays_d, const int* ray_idx,
                               const float* depth, int n_slots, int n_per_ray, int depth_stride, float R_bg,
                               float* sdf_out, float* nabla_out, float* h7_out, void* workspace, long long workspace_bytes, void* stream);

/* ---- B2 (second half): geometry feature (last SDF layer rows 1..256, base.py:253-256) + RadianceNet.forward
 * (models/base.py:372-391) on [x, view (raw: view_tiles=1 | embed 4: view_tiles=3), nabla, feat]. */
int nerfart_radiance_fwd(const float* rad_blob, int precision, int view_tiles, const float* pts, const float* view, long long M,
                         const float* nabla, const float* h7, float* rgb_out, void* stream);
int nerfart_radiance_fwd_rays(const float* rad_blob, int precision, int view_tiles, const float* rays_o, const float* rays_d,
                              const int* ray_idx, const float* depth, int n_slots, int n_per_ray, int depth_stride,
                              const float* nabla, const float* h7, float* rgb_out, void* stream);

/* ---- B2 "bwd", radiance half (row a19; split-bf16 blobs only).  nerfart_radiance_fwd_dump = nerfart_radiance_fwd
 * that also writes the activations of the five layers (geometry feature f, four ReLU outputs r0..r3) into `dump`
 * (nerfart_radiance_dump_bytes(M) bytes): a bf16 matrix [5][Mp][256], Mp = M rounded up to 128, rows = points, the 256
 * features in the kernels' unit order (nerfart_amd/packing.py: unit_feature_hidden) - GEMM operands, read in place.
 * nerfart_radiance_bwd: d loss / d rgb[M,3] -> g_h7[M,256] (cotangent of the SDF net's layer-7 activation through the
 * geometry-feature rows), g_n[M,3] (cotangent of the normal input), and bwd_dump (same layout: the deltas of
 * R0, R1, R2, R3 - each in the slot of the activation it multiplies - and the geometry-feature cotangent): the operands
 * of the weight-gradient reductions (dW_l = delta_l^T act_{l-1}: nerfart_wgrad_bf16 below; call sequence in nerfart_amd/autodiff.py).
 * Padded rows (M .. Mp-1; the reductions run over all Mp rows unmasked): a padded point is evaluated with every input 0 and
 * d loss / d rgb = 0, so its activations (forward dump) are finite and its deltas and g_f (backward dump) are exactly 0 - every
 * product row of a padded point is exactly 0.  A real point with d loss / d rgb = 0 has deltas, g_f, g_h7 and g_n exactly 0.  Both
 * calls write every row of their dump and nothing past nerfart_radiance_dump_bytes(M); rgb_out, g_h7_out, g_n_out: rows 0..M-1 only.
 * At most 2^21 points per call; every pointer argument must be non-NULL (refused by name before any launch).
 * (tests/mlp_bwd_ref.py, tests/test_gpu_mlp_bwd.py) */
long long nerfart_radiance_dump_bytes(long long M);
int nerfart_radiance_fwd_dump(const float* rad_blob, int view_tiles, const float* pts, const float* view, long long M,
                              const float* nabla, const float* h7, float* rgb_out, void* dump, void* stream);
int nerfart_radiance_bwd(const float* rad_blob, long long M, const float* rgb, const float* g_rgb, void* fwd_dump, void* bwd_dump,
                         float* g_h7_out, float* g_n_out, void* stream);

/* ---- B2 "bwd", SDF half (row a19; split-bf16 surface blob).  Parameter gradients of
 *        sbar * sdf + hbar7 . h7 + nbar . grad_x sdf        (what rgb.backward + eikonal.backward ask of the SDF net,
 * volsdf.py:766-770, through ImplicitSurface.forward_with_nablas' create_graph=True, base.py:272-279) need, per layer,
 * the operands of  dW_l = sum_p zbar_l (x) a_{l-1} + (t_l d_l) (x) adot_{l-1}  (see csrc/mlp_chain_bf16.hip):
 *   nerfart_sdf_fwd2: pts[M,3], dir[M,3] = nbar -> f2_dump: [a_l; adot_l] bf16 (slots l = 0..7) and softplus'(z_l) unorm16
 *                     (slots 8 + l)
 *   nerfart_sdf_bwd2: gbar_h7[M,256], gbar_sdf[M], f2_dump -> r2_dump: 65535 * [zbar_l; t_l d_l] bf16, l = 0..7
 * Both dumps are matrices [slot][2 Mp][256], Mp = M rounded up to 64: rows 0..Mp-1 of a slot hold the first, rows Mp..
 * the second quantity of the pair, per point; features in unit order; so dW_l is ONE GEMM over the stacked rows, read in
 * place.  (The softplus' slots 8..15 of f2_dump hold one value per point: rows 0..Mp-1 only, rows Mp.. are never written or read.)
 * SDF layer 3 has 217 outputs: columns of features 217..255 of its slots (3, 11) are finite and meet zero weights; unit 7 (features
 * 224..255) is written as zero bits.
 * Padded rows (M .. Mp-1 of either half; the reductions run over all 2 Mp rows unmasked): a padded point is evaluated at pts = 0 with
 * dir = 0 and zero cotangents, so its adot_l rows and its zbar_l rows are exactly 0 while their partners a_l and t_l d_l are finite
 * - every product row of a padded point, zbar_l (x) a_{l-1} and (t_l d_l) (x) adot_{l-1}, is exactly 0.  The same holds for a real point:
 * dir = 0 gives adot_l = 0, and dir = 0 with gbar_h7 = 0, gbar_sdf = 0 gives zbar_l = 0.  Neither call writes past its _dump_bytes(M).
 * At most 2^21 points per call; every pointer argument must be non-NULL (refused by name before any launch).
 * The reductions are nerfart_wgrad_bf16 calls; the whole sequence - these two sweeps, the reductions, the un-permutation and the weight_norm chain
 * rule - is behind nerfart_sdf_param_bwd / nerfart_*_render_bwd + nerfart_fold_weight_grads / nerfart_weight_norm_bwd (csrc/render_backward.hip). */
long long nerfart_sdf_fwd2_dump_bytes(long long M);
long long nerfart_sdf_bwd2_dump_bytes(long long M);
int nerfart_sdf_fwd2(const float* surf_blob, const float* pts, const float* dir, long long M, void* f2_dump, void* stream);
int nerfart_sdf_bwd2(const float* surf_blob, long long M, const float* gbar_h7, const float* gbar_sdf, void* f2_dump, void* r2_dump,
                     void* stream);

/* ---- rays.  rend_util.get_rays (utils/rend_util.py:112-165) for one camera: pose/K are row-major 4x4
 * on the device; select (int64, may be NULL = all H*W pixels in row-major order) picks pixel indices. */
int nerfart_get_rays(const float* pose_dev, const float* K_dev, int H, int W, const long long* select_dev, int n,
                     float* rays_o, float* rays_d, void* stream);
/* F.normalize(rays_d, dim=-1) (volsdf.py:442, neus.py:196) */
int nerfart_normalize_dirs(const float* in, float* out, int n, void* stream);
/* out[r, k] = near[r]*(1 - t[k]) + far[r]*t[k] (volsdf.py:472-484, neus.py:235-236); near/far NULL -> scalars */
int nerfart_linspace_depths(const float* t_dev, int n, const float* near, const float* far, float near_s, float far_s,
                            int n_rays, float* out, int stride, void* stream);

/* ---- VolSDF sampler stages (models/frameworks/volsdf.py fine_sample :97-302; error_bound :56-94;
 * utils/rend_util.py sample_pdf :256-293, sample_cdf :295-328).  Exposed one by one for parity tests;
 * nerfart_volsdf_fine_sample chains them.  Rows of n samples at row stride cap: n < 2, n > cap and (merge_check) n + n_up > cap are
 * refused with 2 before any HIP call. */
int nerfart_volsdf_first_check(int n_rays, int n, int cap, int n_final, float eps, float alpha_net, float beta_net,
                               const float* dA, const float* sA, const float* u_final, int u_final_stride,
                               float beta_plus0_denom, const float* far, float far_s, float* d_fine, float* beta_plus,
                               float* beta_map, float* iter_usage, int* act_out, int* act_count, void* stream);
int nerfart_volsdf_upsample(int n_active, int n, int cap, int n_up, const float* dA, const float* sA, const int* act,
                            const float* beta_plus, const float* u_up, int clamp_bounds, float* d_new, void* stream);
int nerfart_volsdf_merge_check(int n_active, int n, int cap, int n_up, int n_final, int max_bisect, int it, float eps,
                               float alpha_net, float beta_net, const float* dA, const float* sA, float* dB, float* sB,
                               const int* act, const float* d_new, const float* s_new, const float* u_final,
                               int u_final_stride, float* d_fine, float* beta_plus, float* beta_map, float* iter_usage,
                               int* act_out, int* act_count, void* stream);
int nerfart_volsdf_finalize(int n_active, int n, int cap, int n_final, const float* dA, const float* sA, const int* act,
                            const float* u_final, int u_final_stride, const float* beta_plus, float* d_fine,
                            float* beta_map, float* iter_usage, void* stream);
long long nerfart_volsdf_sampler_workspace_bytes(int n_rays, int n_init, int n_up, int n_final, int max_iter);
int nerfart_volsdf_fine_sample(const float* surf_blob, int precision, const float* rays_o, const float* rays_dn, int n_rays,
                               const float* near, const float* far, float near_s, float far_s, float R_bg,
                               float alpha_net, float beta_net, float eps, int n_init, int n_up, int n_final,
                               int max_iter, int max_bisect, const float* t_init_dev, const float* u_up_dev,
                               const float* u_final_dev, int u_final_per_ray, float* d_fine, float* beta_map,
                               float* iter_usage, void* workspace, long long workspace_bytes, void* stream);
/* t_init_dev / u_up_dev / u_final_dev: device copies of torch.linspace(0,1,n) for n = n_init, n_up+2, n_final
 * (the reference's tables, volsdf.py:483, rend_util.py:269,304); all three NULL -> nerfart_linspace is used.
 * u_final_per_ray != 0 (perturb=True: sample_cdf(det=False), rend_util.py:306-307): u_final_dev is [n_rays, n_final], the
 * caller's uniform random numbers, a row per ray (u_final_stride = n_final in the stage entry points; 0 = shared table). */


/* GUARDED Algorithm 1 (ABI 4): the SDF queries on (surf_blob, precision) - the cheap arithmetic, e.g. precision 4 - with every ray whose outcome hangs
 * on a marginal threshold decision sampled AGAIN, from its first query on, on (esc_blob, esc_precision):
 *   (i)  a ray whose max error bound lies within guard * eps of eps at a convergence check (`max B > eps`, volsdf.py:162-163, :240-242);
 *   (ii) a ray still active after the last round (volsdf.py:294-300: it is sampled with its last bisected beta+ - the rays ANY change of rounding
 *        moves, the reference's own on another machine included: DESIGN.md 2).
 * Rays are independent (volsdf.py:112), so the escalated rays' d_fine / beta_map / iter_usage are bit-identical to a run of all rays on esc_blob; the
 * others made every decision with a margin.  *n_escalated (host int, may be NULL): how many rays ran twice.  guard <= 0 or esc_blob NULL:
 * nerfart_volsdf_fine_sample.  Same workspace (nerfart_volsdf_sampler_workspace_bytes). */
int nerfart_volsdf_fine_sample_guarded(const float* surf_blob, int precision, const float* esc_blob, int esc_precision, float guard,
                                       const float* rays_o, const float* rays_dn, int n_rays,
                                       const float* near, const float* far, float near_s, float far_s, float R_bg,
                                       float alpha_net, float beta_net, float eps, int n_init, int n_up, int n_final,
                                       int max_iter, int max_bisect, const float* t_init_dev, const float* u_up_dev,
                                       const float* u_final_dev, int u_final_per_ray, float* d_fine, float* beta_map,
                                       float* iter_usage, int* n_escalated, void* workspace, long long workspace_bytes, void* stream);

/* (ABI 5) The same with a third escalation rule: late_round > 0 - a ray still active after up-sampling round `late_round` is escalated there (its remaining
 * rounds would each start from a 10-step bisection for beta+, volsdf.py:266-275, whose threshold decisions feed the next round's sampling density: the
 * branch-sensitive rays of Algorithm 1) instead of being carried through them on the cheap arithmetic.  late_round = 0: nerfart_volsdf_fine_sample_guarded. */
int nerfart_volsdf_fine_sample_guarded2(const float* surf_blob, int precision, const float* esc_blob, int esc_precision, float guard, int late_round,
                                        const float* rays_o, const float* rays_dn, int n_rays,
                                        const float* near, const float* far, float near_s, float far_s, float R_bg,
                                        float alpha_net, float beta_net, float eps, int n_init, int n_up, int n_final,
                                        int max_iter, int max_bisect, const float* t_init_dev, const float* u_up_dev,
                                        const float* u_final_dev, int u_final_per_ray, float* d_fine, float* beta_map,
                                        float* iter_usage, int* n_escalated, void* workspace, long long workspace_bytes, void* stream);

/* out[r] = sort(cat(a[r, :na], b[r, :nb]))  (volsdf.py:501-502) */
int nerfart_sort_concat(int n_rays, const float* a, int na, int a_stride, const float* b, int nb, int b_stride,
                        float* out, int out_stride, void* stream);

/* sdf_to_sigma + ray integration (volsdf.py:34-53, :544-576).  normals / sigma_out / p_out / tau_out may be NULL; normals needs nabla.
 * P samples per ray are P - 1 intervals: P >= 2 (any length above that); P < 2 is refused with 2 before any HIP call. */
int nerfart_volsdf_composite(int n_rays, int P, const float* d_all, const float* sdf, const float* radiance,
                             const float* nabla, float alpha, float beta, int white_bkgd, float* rgb, float* depth,
                             float* acc, float* normals, float* sigma_out, float* p_out, float* tau_out, void* stream);

/* Backward of nerfart_volsdf_composite w.r.t. the rgb output (volsdf.py:766) and, optionally, the opacity output acc
 * (g_acc [R] or NULL: the cotangent of mask_volume, the mask BCE of the reconstruction objective, neus.py:600-603):
 * g_rgb [R,3] -> g_sdf [R,P] (through sdf_to_sigma, volsdf.py:34-53), g_rad [R,P,3], and
 * g_alpha_beta[2] += (d loss / d alpha, d loss / d beta) (accumulated with atomics: zero it first; may be NULL).
 * What `rgb.backward(gradient)` (volsdf.py:766) does to the per-ray stage; first hand-written piece of B1 "bwd".
 * 2 <= P <= 513 (a lane holds at most 8 intervals in registers); any other P is refused with 2 before any HIP call. */
int nerfart_volsdf_composite_bwd(int n_rays, int P, const float* d_all, const float* sdf, const float* radiance, float alpha,
                                 float beta, int white_bkgd, const float* g_rgb, const float* g_acc, float* g_sdf, float* g_rad,
                                 float* g_alpha_beta, void* stream);

/* The same for NeuS (neus.py:29-78, :373-395): sdf [R,P] at the samples, radiance [R,P-1,3] at the mid-points, s =
 * exp(ln_s * speed_factor) -> g_sdf [R,P], g_rad_mid [R,P-1,3], g_s[0] += d loss / d s (accumulated with atomics: zero it first; may be NULL).
 * 2 <= P <= 513, as nerfart_volsdf_composite_bwd; any other P is refused with 2 before any HIP call. */
int nerfart_neus_composite_bwd(int n_rays, int P, const float* sdf, const float* rad_mid, float s, int white_bkgd, const float* g_rgb,
                               const float* g_acc, float* g_sdf, float* g_rad_mid, float* g_s, void* stream);

/* Backward of nerfart_volsdf_composite w.r.t. its DEPTH and NORMALS outputs (csrc/volsdf_geo_backward.hip; an addition to ABI 5, no counterpart in
 * the reference, whose losses read rgb only): the geometry terms of a fine-tune objective - depth preservation, normal consistency, smoothness.
 * VolSDF only.  With tau_k = (1 - p_k + 1e-10) T_k over the first P - 1 samples, acc = sum tau_k, inv = acc + 1e-10, depth = sum tau_k d_k / inv,
 * normals = sum tau_k n_k, n_k = nabla_k / max(|nabla_k|, 1e-12) (the forward's values, recomputed here with its expressions):
 *     g_tau_k   = g_normals . n_k + (g_depth / inv) (d_k - depth)         then g_sdf, d / d alpha, d / d beta as nerfart_volsdf_composite_bwd from ITS g_tau
 *     g_nabla_k = tau_k (g_normals - n_k (n_k . g_normals)) / |nabla_k|    where |nabla_k| >= 1e-12,   tau_k g_normals / 1e-12 below that (F.normalize's
 *                 clamp_min as autograd differentiates it);  0 for the last sample, which carries no weight.   The sample depths carry no gradient.
 *   g_depth [R], g_normals [R,3]: each may be NULL (= zero), not both.  nabla [R,P,3] and g_nabla [R,P,3] are required iff g_normals is given;
 *   without g_normals neither is touched.
 *   g_n_in [R,P,3] or NULL: added into g_nabla when g_nabla is written (g_nabla = g_n_in is allowed: each element is read, then written, by one lane) - the
 *   result goes straight into the g_n_extra slot of nerfart_volsdf_pass2_cotangents.  Not read when g_nabla is not written.
 *   accumulate != 0: g_sdf [R,P] += (the last sample's entry untouched); else g_sdf = , the last sample's entry written as +0.
 *   g_alpha_beta[2] += (d / d alpha, d / d beta), accumulated with atomics as in nerfart_volsdf_composite_bwd; may be NULL.
 *   EMPTY RAYS: (d_k - depth) / inv grows without bound as acc -> 0 (inv -> 1e-10): the depth cotangent of a ray that hits nothing is amplified by up
 *   to 1e10, as autograd through the reference's tau / (acc + 1e-10) amplifies it.  Nothing is clamped: weight a depth loss with the opacity.
 * n_rays <= 0 is a no-op.  P < 2, P > 513 (a lane holds at most 8 intervals in registers) or a missing required pointer is refused with 2 and
 * nerfart_last_error set, before any HIP call. */
int nerfart_volsdf_composite_geo_bwd(int n_rays, int P, const float* d_all, const float* sdf, const float* nabla, float alpha, float beta,
                                     const float* g_depth, const float* g_normals, const float* g_n_in, int accumulate, float* g_sdf,
                                     float* g_nabla, float* g_alpha_beta, void* stream);

/* ---- B1: VolSDF volume_render (volsdf.py:389-615) for one chunk of rays (rays_d un-normalised). */
long long nerfart_volsdf_render_workspace_bytes(int n_rays, int n_samples, int n_importance, int max_upsample_steps,
                                                int k3_rays_chunk);
int nerfart_volsdf_render_fwd(const float* surf_blob, const float* rad_blob, int precision, int view_tiles, const float* rays_o,
                              const float* rays_d, int n_rays, float near_s, float far_s, float R_bg, float alpha,
                              float beta, float eps, int n_samples, int n_importance, int max_upsample_steps,
                              int max_bisection_steps, int white_bkgd, int k3_rays_chunk, const float* t_coarse_dev,
                              const float* t_init_dev, const float* u_up_dev, const float* u_final_dev, int u_final_per_ray,
                              float* rgb, float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out, float* nabla_out,
                              float* radiance_out, float* sigma_out, float* p_out, float* tau_out, float* beta_map_out,
                              float* iter_usage_out, void* workspace, long long workspace_bytes, void* stream);

/* The same with Algorithm 1's SDF queries (the no-gradient sampling stage, volsdf.py:479: 512 (1 + rounds) queries per ray, 70 % of a frame) on
 * their OWN blob and precision - e.g. precision 4 (the 2-MFMA kernels) for the sampler and precision 1 for the 192 final samples, whose sdf / nabla /
 * radiance / compositing produce every number that reaches a pixel (+15 % frame rate inside the shipped mode's pixel budgets).  The
 * workspace is nerfart_volsdf_render_workspace_bytes'.  nerfart_volsdf_render_fwd = this with (sampler_blob, sampler_precision) = (surf_blob, precision). */
int nerfart_volsdf_render_mixed_fwd(const float* surf_blob, const float* rad_blob, int precision, const float* sampler_blob, int sampler_precision,
                                    int view_tiles, const float* rays_o, const float* rays_d, int n_rays, float near_s, float far_s, float R_bg, float alpha,
                                    float beta, float eps, int n_samples, int n_importance, int max_upsample_steps,
                                    int max_bisection_steps, int white_bkgd, int k3_rays_chunk, const float* t_coarse_dev,
                                    const float* t_init_dev, const float* u_up_dev, const float* u_final_dev, int u_final_per_ray,
                                    float* rgb, float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out, float* nabla_out,
                                    float* radiance_out, float* sigma_out, float* p_out, float* tau_out, float* beta_map_out,
                                    float* iter_usage_out, void* workspace, long long workspace_bytes, void* stream);

/* Every stage on its own blob / precision (ABI 4; what the shipped `mixed` mode calls): Algorithm 1 on (sampler_blob, sampler_precision), GUARDED by
 * sampler_guard (> 0: nerfart_volsdf_fine_sample_guarded with (surf_blob, precision) as the escalation arithmetic; <= 0: off); sdf + nabla of the 192 final
 * samples on (surf_blob, precision); the radiance net there on (rad_blob, rad_precision); compositing in fp32.  *n_escalated: host int or NULL.
 * nerfart_volsdf_render_mixed_fwd = this with rad_precision = precision and sampler_guard = 0. */
int nerfart_volsdf_render_staged_fwd(const float* surf_blob, int precision, const float* rad_blob, int rad_precision, const float* sampler_blob,
                                     int sampler_precision, float sampler_guard, int view_tiles, const float* rays_o, const float* rays_d, int n_rays,
                                     float near_s, float far_s, float R_bg, float alpha, float beta, float eps, int n_samples, int n_importance,
                                     int max_upsample_steps, int max_bisection_steps, int white_bkgd, int k3_rays_chunk, const float* t_coarse_dev,
                                     const float* t_init_dev, const float* u_up_dev, const float* u_final_dev, int u_final_per_ray,
                                     float* rgb, float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out, float* nabla_out,
                                     float* radiance_out, float* sigma_out, float* p_out, float* tau_out, float* beta_map_out,
                                     float* iter_usage_out, int* n_escalated, void* workspace, long long workspace_bytes, void* stream);

/* (ABI 5) nerfart_volsdf_render_staged_fwd with the sampler's late_round (nerfart_volsdf_fine_sample_guarded2); 0 = that function. */
int nerfart_volsdf_render_staged2_fwd(const float* surf_blob, int precision, const float* rad_blob, int rad_precision, const float* sampler_blob,
                                      int sampler_precision, float sampler_guard, int sampler_late_round, int view_tiles, const float* rays_o, const float* rays_d,
                                      int n_rays, float near_s, float far_s, float R_bg, float alpha, float beta, float eps, int n_samples, int n_importance,
                                      int max_upsample_steps, int max_bisection_steps, int white_bkgd, int k3_rays_chunk, const float* t_coarse_dev,
                                      const float* t_init_dev, const float* u_up_dev, const float* u_final_dev, int u_final_per_ray,
                                      float* rgb, float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out, float* nabla_out,
                                      float* radiance_out, float* sigma_out, float* p_out, float* tau_out, float* beta_map_out,
                                      float* iter_usage_out, int* n_escalated, void* workspace, long long workspace_bytes, void* stream);

/* ---- NeuS (models/frameworks/neus.py): up-sampling 'official_solution' :275-303 ('direct_use' / 'direct_more' :242-269 below), helpers :29-78,
 * volume_render :142-424; near_far_from_sphere utils/rend_util.py:168-186. */
int nerfart_near_far_from_sphere(const float* rays_o, const float* rays_dn, int n_rays, float r, float* near,
                                 float* far, void* stream);
int nerfart_neus_upsample_step(int n_rays, int n, int cap, int n_new, float inv_s, const float* d, const float* sdf,
                               const float* u_new, int u_new_stride, float* d_new, void* stream);
int nerfart_merge_sorted_pairs(int n_rays, int n, int cap, int n_new, float* d, float* sdf, const float* d_new,
                               const float* s_new, void* stream);
/* NeuS ray integration (neus.py:322, :373-395): P >= 2 as nerfart_volsdf_composite (P < 2 is refused with 2); every output after acc may be NULL. */
int nerfart_neus_composite(int n_rays, int P, const float* d_all, const float* sdf, const float* radiance_mid,
                           const float* nabla, float s, int white_bkgd, float* rgb, float* depth, float* acc,
                           float* normals, float* cdf_out, float* alpha_out, float* w_out, float* d_mid_out,
                           void* stream);
long long nerfart_neus_render_workspace_bytes(int n_rays, int n_samples, int n_importance, int k3_rays_chunk);
int nerfart_neus_render_fwd(const float* surf_blob, const float* rad_blob, int precision, int view_tiles, const float* rays_o,
                            const float* rays_d, int n_rays, float obj_bounding_radius, float s, int n_samples,
                            int n_importance, int n_upsample_iters, int white_bkgd, int k3_rays_chunk,
                            const float* t_coarse_dev, const float* u_new_dev, int u_new_per_ray, float* rgb,
                            float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out,
                            float* nabla_out, float* radiance_out, float* cdf_out, float* alpha_out, float* w_out,
                            float* d_mid_out, void* workspace, long long workspace_bytes, void* stream);
/* u_new_per_ray != 0 (perturb=True: sample_pdf(det=False), rend_util.py:269-272): u_new_dev is [n_rays, n_importance], the
 * caller's uniform random numbers - up-sampling round i uses columns [i * n_new, (i + 1) * n_new); 0: the shared
 * linspace(0, 1, n_new) table (u_new_dev [n_new] or NULL). */

/* ABI 3: the other two up-sampling algorithms of neus.py (:242-269; `model.upsample_algo` in the YAML, :735) behind the same renderer.
 *   upsample_algo 0 'official_solution' (= nerfart_neus_render_fwd), 1 'direct_use' (:242-255: all n_importance fine samples at once from the
 *   coarse samples' own visibility weights sdf_to_w(sdf, 1 / fixed_s_recp), :47-63), 2 'direct_more' (:259-269: the same from n_nograd_samples
 *   evenly spaced no-gradient samples).  For 1 and 2 n_upsample_iters is ignored and the uniform numbers are ONE table of n_importance values
 *   (u_new_per_ray == 0: u_new_dev [n_importance] = linspace(0, 1, n_importance), or NULL) or [n_rays, n_importance].
 *   t_nograd_dev: linspace(0, 1, n_nograd_samples) on the device or NULL (built inside: one stream synchronisation).
 *   nerfart_neus_direct_upsample_step: one inversion (n bins with row stride cap -> n_new sorted samples per ray), the stage entry. */
int nerfart_neus_direct_upsample_step(int n_rays, int n, int cap, int n_new, float inv_s, const float* d, const float* sdf,
                                      const float* u_new, int u_new_stride, float* d_new, void* stream);
long long nerfart_neus_render_algo_workspace_bytes(int n_rays, int n_samples, int n_importance, int k3_rays_chunk, int upsample_algo,
                                                   int n_nograd_samples);
int nerfart_neus_render_algo_fwd(const float* surf_blob, const float* rad_blob, int precision, int view_tiles, const float* rays_o,
                                 const float* rays_d, int n_rays, float obj_bounding_radius, float s, int n_samples,
                                 int n_importance, int n_upsample_iters, int upsample_algo, int n_nograd_samples, float fixed_s_recp,
                                 int white_bkgd, int k3_rays_chunk,
                                 const float* t_coarse_dev, const float* t_nograd_dev, const float* u_new_dev, int u_new_per_ray, float* rgb,
                                 float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out,
                                 float* nabla_out, float* radiance_out, float* cdf_out, float* alpha_out, float* w_out,
                                 float* d_mid_out, void* workspace, long long workspace_bytes, void* stream);

/* ---- B4: CLIP ViT-B/32 image encoder (third-party `clip`: `model.encode_image(img)` of `clip.load("ViT-B/32", device="cuda")`,
 * reference call sites criteria/clip_loss.py:204-216, contrastive_loss.py:110-114, patchnce_loss.py:124-128) and its
 * backward w.r.t. the image (what autograd does there when the style loss is back-propagated, volsdf.py:912-915; the CLIP
 * weights are frozen).  csrc/clip_vit.hip: fp16 weights / GEMM operands on v_mfma_f32_32x32x16_f16, fp32 accumulation,
 * LayerNorm / softmax / residual stream in fp32.
 *   blob      : the `visual.*` parameters packed by nerfart_amd/clip_native.py in the section order
 *               nerfart_clip_vitb32_blob_layout() reports (offsets[203] in bytes, last = total size; returns the total):
 *               fp16 matrices, each stored once (0 conv1, 2 + 8 l + {0, 2, 4, 6} the four linear maps of block l, 99 proj; the odd
 *               sections, once the transposed copies, are empty: the backward GEMMs read the forward matrices in place), then
 *               fp32 vectors (100 class / positional embeddings, LayerNorm parameters, biases) - list in csrc/clip_vit.hip.
 *   blob_bytes: the size of the caller's blob; must equal the layout's total, so a blob packed to an older layout (ABI 1 stored
 *               transposed copies too) is rejected instead of read.
 *   img       : [B, 3, 224, 224] fp32, already resized and normalised (the reference's `preprocess`).
 *   feat_out  : [B, 512] fp32 (un-normalised features, as encode_image returns them).
 *   workspace : nerfart_clip_vitb32_workspace_bytes(B, keep_for_bwd) bytes of device memory.  With keep_for_bwd != 0 the
 *               forward leaves the per-block activations there and nerfart_clip_vitb32_image_bwd(g_feat [B,512] ->
 *               g_img [B,3,224,224]) must be given the SAME workspace, untouched; several forwards may be outstanding,
 *               each with its own workspace.
 *
 * nerfart_clip_vitb32_workspace_layout (host arithmetic only) returns the same total as nerfart_clip_vitb32_workspace_bytes (0 for B < 1) and, with
 * offsets != NULL, the byte offsets of the workspace's buffers, offsets[21] (each a multiple of 256), in this order.  M = 50 B token rows (row
 * b 50 + t: t = 0 the class token, t >= 1 patch t - 1), P = 49 B patch rows; Mp, Pp, Bp = M, P, B rounded up to 64 (the GEMM tile).  Every
 * buffer is row-major with the row stride of its logical width; rows past the logical count are padding the kernels never store.
 *    0 scale   fp32 [2]            backward: s, the power of two the cotangent is multiplied by, and 1 / s.  s = min(2^floor(log2(16 / max|g_feat|)),
 *                                  2^126), 1 for an all-zero g_feat or a non-finite max-abs (a non-finite g_feat gives a non-finite g_img)
 *    1 patches fp16 [P, 3072]  Pp  forward: the image's patches, column c 1024 + kh 32 + kw
 *    2 pe      fp32 [P, 768]   Pp  forward: patches . conv1^T;  after a backward to stop_layer 0: fp32 [P, 3072] s d patches (the buffer has
 *                                  Pp x 3072 floats)
 *    3 xemb    fp32 [M, 768]   Mp  forward: class / patch embedding + positional embedding (ln_pre's input)
 *    4 xfin    fp32 [M, 768]   Mp  forward: the residual stream after block 11
 *    5 y       fp16 [M, 768]   Mp  forward: the last LayerNorm output (ln_2 of block 11);  after a backward to 0: fp16 [P, 768] (Pp rows)
 *                                  s d patch embedding
 *    6 att     fp16 [M, 768]   Mp  forward: block 11's attention output (heads side by side);  backward: the last block run's d of that
 *    7 act     fp16 [M, 3072]  Mp  forward: block 11's QuickGELU output;  backward: the last block run's d pre-activation (d act . gelu'(pre))
 *    8 t       fp32 [M, 768]   Mp  backward only: the last block run's d ln_1 output (dqkv . in_proj)
 *    9 dx      fp32 [M, 768]   Mp  backward only: s d residual stream entering the last block run, from above (= d xin of that block)
 *   10 dqkv    fp16 [M, 2304]  Mp  backward only: the last block run's d qkv
 *   11 x0      fp16 [B, 768]   Bp  forward: ln_post of the class rows
 *   12 g16     fp16 [B, 512]   Bp  backward: fp16(s g_feat)
 *   13 t0      fp32 [B, 768]   Bp  backward: g16 . proj^T
 *   14 saved   the per-block buffers: block l at saved + l layer_bytes with keep_for_bwd != 0; with 0 one block reused by all, followed by
 *              an fp32 [Mp, 768] buffer the residual stream ping-pongs through
 *   15 layer_bytes (a size, not an offset)
 *   16 xin  fp32 [M, 768]   17 xmid  fp32 [M, 768] (after the attention branch)   18 qkv  fp16 [M, 2304] (q | k | v, head h at columns
 *   64 h)   19 pre  fp16 [M, 3072] (c_fc output before QuickGELU) - offsets inside a block, Mp rows each
 *   20 total
 * The forward zeroes [0, saved) (everything with keep_for_bwd == 0); the padding rows of the saved blocks keep the caller's bytes: they are read
 * as GEMM / LayerNorm operands of padding rows only, whose results are never stored.
 *
 * nerfart_clip_vitb32_image_bwd_partial is the backward with its block loop ending at stop_layer (0 .. 12, else refused before any launch): the
 * head (scale, g16, t0, the class rows of dx), blocks 11 .. stop_layer, and only for stop_layer == 0 the tail (y, d patches, g_img) - with 0 it IS
 * nerfart_clip_vitb32_image_bwd.  For stop_layer > 0 g_img may be NULL and is never touched.  No kernel uses atomics: runs on the same saved
 * forward repeat bit for bit, so a run to l + 1 and a run to l give block l's incoming dx and everything block l leaves (tests). */
long long nerfart_clip_vitb32_blob_layout(long long* offsets);
long long nerfart_clip_vitb32_workspace_bytes(int B, int keep_for_bwd);
long long nerfart_clip_vitb32_workspace_layout(int B, int keep_for_bwd, long long* offsets);
int nerfart_clip_vitb32_image_bwd_partial(const void* blob, long long blob_bytes, int B, const float* g_feat, float* g_img, void* workspace,
                                          long long workspace_bytes, int stop_layer, void* stream);
int nerfart_clip_vitb32_image_fwd(const void* blob, long long blob_bytes, const float* img, int B, float* feat_out, int keep_for_bwd, void* workspace,
                                  long long workspace_bytes, void* stream);
int nerfart_clip_vitb32_image_bwd(const void* blob, long long blob_bytes, int B, const float* g_feat, float* g_img, void* workspace, long long workspace_bytes,
                                  void* stream);
/* ---- image side of the style losses (rows a20-a22; csrc/style_heads.hip).
 * nerfart_resample_fwd: one stage of the reference's torchvision `preprocess` chains (criteria/clip_loss.py:166-168,
 * contrastive_loss.py:98-101, patchnce_loss.py:98-117, :184-215) as a gather: the source image(s) src [n_src, C, Hs, Ws] (n_src = 1:
 * shared by all outputs, else N) sit at (pad_t, pad_l) inside a zero canvas Hp x Wp (ZeroPad2d), the canvas is resampled to
 * Hr x Wr (mode 1 = bicubic A = -0.75, 0 = bilinear; align_corners = False, no antialias), output image n [C, Ho, Wo] is the
 * window of it at crop_yx[n] = (y0, x0) (int32 [N, 2] on the device; NULL = (0, 0)), then v * affine[c] + affine[C + c]
 * (affine NULL = identity: (x + 1) / 2 and Normalize(mean, std) fold into it).  src_win (int32 [N, 4] = y, x, h, w on the device, or
 * NULL): output n resamples only that sub-window of its source, taps clamping at the window's edges - crop-then-resize, the
 * 112 x 112 -> 224 x 224 patches of patchnce_loss.py:213-215 (the canvas is then the window: no padding, Hp / Wp ignored).
 * nerfart_resample_bwd accumulates J^T g_dst into g_src (fp32 atomics; zero it first). */
int nerfart_resample_fwd(const float* src, int n_src, int C, int Hs, int Ws, int pad_t, int pad_l, int Hp, int Wp, int Hr, int Wr, int mode,
                         const int* crop_yx, const int* src_win, const float* affine, float* dst, int N, int Ho, int Wo, void* stream);
int nerfart_resample_bwd(const float* g_dst, int n_src, int C, int Hs, int Ws, int pad_t, int pad_l, int Hp, int Wp, int Hr, int Wr, int mode,
                         const int* crop_yx, const int* src_win, const float* affine, float* g_src, int N, int Ho, int Wo, void* stream);
/* The three CLIP heads from image features feats [4 + P, 512] (rows: 0 directional prediction, 1 directional source, 2 contrastive
 * prediction, 3 contrastive source, 4.. PatchNCE crops) and cached unit text features: text_dir [512] (clip_loss.py:234-246),
 * t_tgt / t_con [T, 512] (templates of the target / of the contrastive negative prompt), t_neg [S, T, 512]:
 *   out4 = {w_dir L_dir + w_con L_con + w_nce L_nce, L_dir (clip_loss.py:244-254), L_con (contrastive_loss.py:146-153, margin),
 *           L_nce (patchnce_loss.py:153-173, temperature tau, summed over the P crops)},  g_feats [4 + P, 512] = d out4[0] / d feats
 * (rows 1 and 3 are constants of the loss: zero). */
int nerfart_clip_style_heads(const float* feats, int n_patches, const float* text_dir, const float* t_tgt, const float* t_con, const float* t_neg,
                             int n_neg, int n_templates, float w_dir, float w_con, float w_nce, float margin, float tau, float* out4,
                             float* g_feats, void* stream);

/* ---- surface renderer (models/ray_casting.py): per-ray stages around the SDF query B3 (the marching and
 * refinement points are evaluated with nerfart_sdf_fwd_rays).  Masks are uint8 [R].
 * nerfart_first_crossing: root_finding_surface_points' analysis of the marched values val [R, n_steps] at depths depth [R, n_steps]
 *   (ray_casting.py:79-126): mask = first sign change of (val - tau) exists & goes outside -> inside & the ray starts outside;
 *   bracket [R, 4] = (d_low, f_low, d_high, f_high) around it; d_pred = first secant estimate (1 where mask is false).
 * nerfart_secant_update: one run_secant_method iteration (ray_casting.py:15-29) given f_mid [R] = sdf at the current d_pred.
 * nerfart_root_finish: depth / point outputs with the reference's fill values (ray_casting.py:137-152): inf (fill_inf) or far where
 *   nothing was hit, 0 where the ray starts inside, pt = 1 where mask is false.
 * nerfart_sphere_trace_step: one iteration of sphere_tracing_surface_points (ray_casting.py:175-180). */
int nerfart_first_crossing(const float* val, const float* depth, int n_rays, int n_steps, float logit_tau, unsigned char* mask,
                           unsigned char* mask_sign_change, unsigned char* mask_start_outside, float* bracket, float* d_pred, void* stream);
int nerfart_secant_update(const float* f_mid, int n_rays, float logit_tau, const unsigned char* mask, float* bracket, float* d_pred, void* stream);
int nerfart_root_finish(const float* rays_o, const float* rays_dn, int n_rays, const unsigned char* mask, const unsigned char* mask_start_outside,
                        const float* d_pred, const float* far, float far_s, int fill_inf, float* d_out, float* pt_out, void* stream);
int nerfart_sphere_trace_step(const float* sdf, int n_rays, const float* far, float far_s, float* d, unsigned char* mask, void* stream);

/* ---- isosurface extraction (utils/mesh_util.py:112 hands the SDF grid to skimage.measure.marching_cubes on the host;
 * csrc/marching_cubes.hip: classify / scan / emit on the device, table-based marching cubes on the case table nerfart_amd/mc_table.py generates).
 * An addition to ABI 5.  vol [nx, ny, nz] fp32, z fastest (mesh_util.sdf_volume's grid).  A corner is inside iff value < level; every vertex lies on a
 * grid edge, owned by the edge's lower end point.
 *   nerfart_mc_workspace_bytes: the size of the caller's workspace (0 = bad dimensions, see nerfart_last_error).
 *   nerfart_mc_count: fills the workspace (per-point edge flags and case index, scanned vertex / triangle offsets) and counts [3] (DEVICE, 8-byte
 *     aligned) = {V vertices, F triangles, 1 if any value of the volume is non-finite (such values count as outside)}.  Asynchronous.
 *   nerfart_mc_emit: from the SAME, untouched workspace: verts [V, 3] on the sign-changing edges - with a, b the values at the edge's end points (a at the owner),
 *     t = (level - a) / (b - a), pa = fma(index, spacing, origin), pb = fma(index + 1, spacing, origin) along the edge's axis, the vertex is
 *     fma(t, pb - pa, pa) there and pa on the other two axes (fp32, each fma ONE rounding: what a second implementation must do to get the same
 *     bits) - in the order (point in linear order, then axis x, y, z); faces [F, 3] int32 in the order (cell in linear order, then the table's
 *     triangles), wound so that (v1 - v0) x (v2 - v0) points to the outside (value >= level).  origin / spacing: HOST arrays of 3.  V and F are the
 *     sizes of the caller's arrays (every write is checked against them); V == 0 or F == 0 launches nothing.  No atomics: two runs are bit-identical.
 * Refused with 2 before any launch: a null pointer, a dimension < 2, 3 nx ny nz >= 2^31, nx * ceil(ny / 4) * ceil(nz / 64) >= 2^24 (a volume
 * long in x and thin in y / z: more blocks than one launch takes; put the long axis last), a workspace smaller than the query's answer (or not
 * 16-byte aligned). */
size_t nerfart_mc_workspace_bytes(int nx, int ny, int nz);
int nerfart_mc_count(const float* vol, int nx, int ny, int nz, float level, void* ws, size_t ws_bytes, unsigned* counts, void* stream);
int nerfart_mc_emit(const float* vol, int nx, int ny, int nz, float level, const float* origin, const float* spacing, const void* ws, size_t ws_bytes,
                    float* verts, int* faces, unsigned V, unsigned F, void* stream);

/* ---- mesh vertices on their grid edges (csrc/marching_cubes.hip, csrc/mesh_vertices.hip; mesh_util.refine_vertices): which edge a vertex of
 * nerfart_mc_emit sits on, its position from the edge parameter t, and a refinement of t against the SDF that never leaves the edge - so faces stay
 * valid unchanged.  Additions to ABI 5; no counterpart in the reference.  One thread per vertex, no atomics: two runs give the same bits.  V == 0
 * launches nothing and returns 0; a null pointer is refused with 2.
 *   nerfart_mc_emit_edges: from the SAME, untouched workspace nerfart_mc_count filled, in nerfart_mc_emit's vertex order (point in linear order,
 *     then axis x, y, z, at the scanned offset), every write checked against V.  For vertex i on the edge owned by point p (linear index) toward
 *     +axis, with a = vol[p], b = vol[p + stride[axis]]:
 *       edge[i] = 3 p + axis (uint32);  bracket[i] = (t0, g0, t1, g1) = (0, a - level, 1, b - level) ([V, 4] fp32);
 *       t[i] = (level - a) / (b - a), nerfart_mc_emit's expression;  best[i] = (t_best, g_best) = (t[i], +inf) ([V, 2] fp32);  side[i] = 0 (uint8).
 *     Refusals as nerfart_mc_emit: dimensions, workspace size and alignment.
 *   nerfart_mesh_edge_points: pts_out [V, 3] in the frame origin / spacing (HOST arrays of 3), with nerfart_mc_emit's arithmetic: idx = the
 *     point's (x, y, z), pa[c] = fma(idx[c], spacing[c], origin[c]), pb = fma(idx[axis] + 1, spacing[axis], origin[axis]),
 *     q[axis] = fma(t, pb - pa[axis], pa[axis]), the other two components pa - so t as nerfart_mc_emit_edges left it and the same frame give
 *     nerfart_mc_emit's verts bit for bit.  An edge whose point index is >= nx ny nz, or whose far end is outside the volume, writes nothing for
 *     that vertex (and nothing is read or written out of bounds).  Refused: a dimension < 2, 3 nx ny nz >= 2^31.
 *   nerfart_mesh_edge_refine_step: one step of bracket-keeping false position with the Illinois modification.  f [V] = the SDF at the points of
 *     the current t.  Per vertex, with g = f - level, in this order (fp32, every operation rounded once, in the order written):
 *       1. if |g| < |g_best|: best = (t, g).  NaN never wins; the first finite evaluation always does.
 *       2. if g is NaN: nothing else of this vertex changes.
 *       3. if g == 0: bracket = (t, 0, t, 0), side = 0, t stays.
 *       4. if (g < 0) == (g0 < 0): if side == 1, g1 *= 0.5; then (t0, g0) = (t, g), side = 1.
 *          else:                   if side == 2, g0 *= 0.5; then (t1, g1) = (t, g), side = 2.
 *       5. t = t0 - (g0 * (t1 - t0)) / (g1 - g0); a non-finite result becomes 0.5 * (t0 + t1); the result is clamped into
 *          [min(t0, t1), max(t0, t1)].
 *     The refined vertex is t_best: its residual g_best was actually evaluated, |g_best| never grows, and t, t_best stay in [0, 1]. */
int nerfart_mc_emit_edges(const float* vol, int nx, int ny, int nz, float level, const void* ws, size_t ws_bytes, unsigned* edge, float* bracket,
                          float* t, float* best, unsigned char* side, unsigned V, void* stream);
int nerfart_mesh_edge_points(const unsigned* edge, const float* t, unsigned V, int nx, int ny, int nz, const float* origin, const float* spacing,
                             float* pts_out, void* stream);
int nerfart_mesh_edge_refine_step(const float* f, float level, unsigned V, float* bracket, float* t, float* best, unsigned char* side, void* stream);

/* ---- connected components of an indexed mesh and the compaction that drops some of them (csrc/mesh_components.hip;
 * mesh_util.mesh_components / filter_components, extract_mesh(keep_largest=, min_component_faces=): the floaters of a fine-tuned field are removed
 * without the mesh leaving the GPU).  Additions to ABI 5; no counterpart in the reference.  faces [F, 3] int32 indexes V vertices - nerfart_mc_emit's
 * mesh is indexed, one vertex per grid edge, so nothing has to be welded.  Everything is integers: the results below are defined uniquely.
 *   THE RULE: two vertices are connected when a face contains both, and components are the classes of the transitive closure - VERTEX
 *     connectivity: two triangles that share a single vertex are one component.  A vertex in no face is a component of its own.  A face with an
 *     index outside [0, V) is BAD: it joins nothing, is counted nowhere, never survives a compaction, and nothing is read or written outside the
 *     arrays because of it.
 *   nerfart_mesh_components: label [V] int32, label[v] = the smallest vertex index of v's component;  n_faces [V] uint32, n_faces[r] = the number
 *     of (good) faces of the component whose label is r, 0 at every index that is not a label;  info [3] uint32 (DEVICE) = {components, components
 *     with at least one face, 1 if any face is bad}.  Asynchronous, no host read inside.  V == 0 zeroes info and launches nothing; F == 0 labels
 *     every vertex with itself.  (A lock-free union-find that links the larger root under the smaller, so parent[v] <= v throughout: the
 *     smallest index of a component is the one root left, whatever the order of work - csrc/mesh_components.hip.)
 *   nerfart_mesh_compact_workspace_bytes: the size of the caller's workspace for the two calls below (the scanned (vertex, face) offsets of
 *     max(V, F, 1) items plus their block sums; 0 = bad sizes, see nerfart_last_error).
 *   nerfart_mesh_compact_count: keep [V] uint8 is indexed BY LABEL: component r survives iff keep[r] != 0.  Vertex v survives iff
 *     keep[label[v]]; face f survives iff it is good and keep[label[faces[f][0]]] (a label outside [0, V) survives nothing).  Fills the workspace
 *     and counts [2] (DEVICE, 8-byte aligned) = {V' surviving vertices, F' surviving faces}.  Asynchronous.
 *   nerfart_mesh_compact_emit: from the SAME, untouched workspace: src_vertex [V'] int32 = the old indices of the surviving vertices, ascending
 *     (so new vertex i is old vertex src_vertex[i]: any per-vertex array is gathered with it);  faces_out [F', 3] int32 = the surviving faces in
 *     their old order, every index replaced by the number of surviving vertices before it.  V_out and F_out are the sizes of the caller's arrays
 *     (every write is checked against them); both 0 launches nothing.  No atomics: two runs give the same bits.
 * Refused with 2 before any launch: a null pointer (of an array that is not empty), V or F >= 2^31, 3 F >= 2^32, counts not 8-byte aligned, a
 * workspace smaller than the query's answer (or not 16-byte aligned). */
int nerfart_mesh_components(const int* faces, unsigned F, unsigned V, int* label, unsigned* n_faces, unsigned* info, void* stream);
size_t nerfart_mesh_compact_workspace_bytes(unsigned V, unsigned F);
int nerfart_mesh_compact_count(const int* label, const unsigned char* keep, const int* faces, unsigned V, unsigned F, void* ws, size_t ws_bytes,
                               unsigned* counts, void* stream);
int nerfart_mesh_compact_emit(const int* label, const unsigned char* keep, const int* faces, unsigned V, unsigned F, const void* ws, size_t ws_bytes,
                              int* src_vertex, int* faces_out, unsigned V_out, unsigned F_out, void* stream);

/* ---- half-edge adjacency, manifold checks and per-component measures of an indexed mesh (csrc/mesh_topology.hip; mesh_util.half_edges /
 * mesh_topology, tools/check_mesh.py: is the mesh a valid surface - watertight, how many holes, what genus).  Additions to ABI 5; no counterpart
 * in the reference.  faces [F, 3] int32 over V vertices.  tests/mesh_topology_ref.py states all of this in numpy.  Everything but `measure` is
 * integers: the results below are defined uniquely and do not depend on the table's size or on the order of work.
 *   FACES: a face is BAD if an index lies outside [0, V); DEGENERATE if it is good but two of its indices are equal; otherwise PROPER.  Only
 *     proper faces take part below; nothing is read or written outside the arrays because of the others.
 *   HALF-EDGES: h = 3 f + i runs from faces[f][i] to faces[f][(i + 1) % 3]; it is also the CORNER of face f at vertex faces[f][i].
 *   EDGES: for an undirected edge {a < b}, n_fwd and n_bwd count the proper half-edges a -> b and b -> a, n = n_fwd + n_bwd.  The edge is
 *     BOUNDARY when n == 1; MANIFOLD when n_fwd == n_bwd == 1; FLIPPED when n == 2 otherwise (the two faces run through it the same way);
 *     NON-MANIFOLD when n > 2.
 *   FANS: across every edge with n == 2 (manifold or flipped) the two faces' corners at a are united, and likewise their corners at b.
 *     vertex_fans[v] = the number of corner classes at v, 0 for a vertex in no proper face; more than one: a bow-tie.
 *   BOUNDARY LOOPS: two boundary edges are joined when they share a vertex; loops are the classes of the closure, a loop's size its edges.
 *   COMPONENTS are nerfart_mesh_components' labels; an edge or a face belongs to the component of its first vertex (a of {a < b}; faces[f][0]).
 *   nerfart_mesh_topology_workspace_bytes: the caller's workspace for a table of 2^table_log2 slots, 1 <= table_log2 <= 31; table_log2 == 0
 *     chooses the default, the smallest power of two >= 4 (3 F + 1) (at most 2^31): the distinct edges are at most 3 F, so the LOAD FACTOR
 *     stays below 1/4, and is 1/16 .. 1/8 on a closed manifold mesh (E = 3 F / 2).  Carved in this order, each buffer rounded up to 256 bytes:
 *     slot_of [3 F] u32, corner parents [3 F] u32, vertex parents [V] u32, loop sizes [V] u32, referenced [V] u32 (each of at least one word),
 *     then the table, 24 bytes per slot {u64 key (a << 32) | b, u32 n_fwd, n_bwd, u32 smallest half-edge id fwd, bwd}.  Returns 0 (refused, see
 *     nerfart_last_error) for V or F >= 2^31, 3 F >= 2^32, a table_log2 outside 0 .. 31 and a table of fewer than 3 F + 1 slots (so no table
 *     at all once 3 F + 1 > 2^31: half-edge ids stay below 2^31 and never meet the codes of `twin`).
 *   nerfart_mesh_half_edges: twin [3 F] int32 = the other half-edge of a manifold edge, -1 on a boundary edge, -2 on a flipped edge, -3 on a
 *     non-manifold edge, -4 for the half-edges of a face that is not proper;  edge_uses [3 F] uint32 = n of the half-edge's edge, 0 for a face
 *     that is not proper;  vertex_fans [V] uint32;  info [16] uint32 (DEVICE):
 *       [0] proper faces  [1] degenerate faces  [2] bad faces  [3] referenced vertices (in a proper face)  [4] distinct edges E
 *       [5] boundary edges  [6] flipped edges  [7] non-manifold edges  [8] vertices with more than one fan  [9] boundary loops
 *       [10] edges of the longest loop  [11] OVERFLOW: 1 if a probe sequence visited every slot without finding room - it must read 0, and
 *       does for every table this call accepts; with 1 the other outputs are not valid  [12 .. 15] zero.
 *     Asynchronous, no host read inside.  Fills the workspace: it keeps the edge table for the call below.  F == 0 zeroes vertex_fans and
 *     info; V == 0 counts every face as bad and writes -4 / 0.  Every loop is bounded whatever the faces hold: a probe sequence by the
 *     table's size, the union-finds (csrc/union_find.h) by the indices.
 *   nerfart_mesh_component_stats: from the SAME, untouched workspace and label [V] of nerfart_mesh_components:  counts [V, 6] uint32, indexed
 *     BY LABEL, zero at every index that is not a label = {referenced vertices, edges, proper faces, boundary edges, flipped edges,
 *     non-manifold edges};  measure [V, 2] fp64 (8-byte aligned) = {area, signed volume} summed over the component's proper faces.  verts
 *     [V, 3] fp32 are promoted to fp64 first; then every operation is rounded once (no contraction), in this order, with a = v0, b = v1, c = v2:
 *       u = b - a, w = c - a;  n = (uy wz - uz wy, uz wx - ux wz, ux wy - uy wx);  area term = 0.5 sqrt((nx nx + ny ny) + nz nz)
 *       m = (by cz - bz cy, bz cx - bx cz, bx cy - by cx);  volume term = ((ax mx + ay my) + az mz) / 6
 *     The terms are added with fp64 atomics (combined within a wave first): the order of the sum is not fixed, so a sum is within
 *     m 2^-53 sum|term| of the exact sum of its m terms, and two runs can differ by that much.  The integer outputs are exact.
 * Refused with 2 before any launch: a null pointer (of an array that is not empty), the sizes above, measure not 8-byte aligned, a workspace
 * smaller than the query's answer (for nerfart_mesh_component_stats: than the answer for the smallest legal table) or not 16-byte aligned. */
size_t nerfart_mesh_topology_workspace_bytes(unsigned V, unsigned F, int table_log2);
int nerfart_mesh_half_edges(const int* faces, unsigned F, unsigned V, int table_log2, void* ws, size_t ws_bytes, int* twin, unsigned* edge_uses,
                            unsigned* vertex_fans, unsigned* info, void* stream);
int nerfart_mesh_component_stats(const float* verts, const int* faces, unsigned F, unsigned V, const int* label, const void* ws, size_t ws_bytes,
                                 unsigned* counts, double* measure, void* stream);

/* ---- manifold repair: cut and stitch of non-manifold edges (csrc/mesh_repair.hip; mesh_util.repair_manifold, extract_mesh(repair=)).  Additions
 * to ABI 5; no counterpart in the reference.  verts [V, 3] fp32, faces [F, 3] int32.  The output has no non-manifold edge and no bow-tie
 * vertex; no triangle's geometry changes, except that a few triangles are split at an edge midpoint where an indexed mesh forces it (rule 5).
 * tests/mesh_repair_ref.py states all of this in numpy.  Everything but the midpoints is integers and the midpoints are two correctly rounded
 * fp32 operations: every output is defined uniquely and depends neither on the order of work nor on the table's size.  Faces, half-edges,
 * corners and edges are those of the topology block above.
 *   0. FACES: bad and degenerate faces are dropped.
 *   1. CANCEL: the proper faces are grouped by vertex set {a, b, c}.  Of a set with p faces of one orientation and q of the other, |p - q| faces
 *      of the majority orientation survive, the first in input order; the rest are dropped - zero-thickness fins (a, b, c) + (a, c, b) go in
 *      pairs, each pair taking one forward and one backward use from each of the three edges, so an edge's balance is kept.  (Faces of ONE
 *      orientation only all survive: dropping a duplicate would break the balance.  Their edges are flipped edges, see below.)  The groups are
 *      found with an open-addressing table of face indices keyed on the sorted triple (atomicCAS from empty, atomicMin among equal keys, as the
 *      duplicate table of the simplify block); a slot's counts are sums and its members a set: the outcome does not depend on the order of work.
 *      Only the surviving faces take part below.
 *   2. RADIAL PAIRING of every non-manifold edge {a < b} with 2 < n <= 64 half-edges.  Its half-edges are ordered around the axis
 *      d = v_b - v_a by the direction of their APEX, the face's third vertex.  Vertices are promoted to fp64; then every operation is rounded
 *      once (no contraction), in this order; no division, square root or atan2:
 *        sub(p, q) = (px - qx, py - qy, pz - qz);  cross(p, q) = (py qz - pz qy, pz qx - px qz, px qy - py qx);  dot(p, q) = (px qx + py qy) + pz qz
 *        d = sub(v_b, v_a);  w = sub(apex, v_a);  w0 = the w of the edge's smallest half-edge id;  u1 = cross(d, w0);  u2 = cross(d, u1)
 *        (x, y) = (-dot(w, u2), dot(w, u1)); the half-edge with the smallest id is given (1, 0) exactly.  (Scaling y by a positive constant
 *        keeps the cyclic order: nothing is normalised.)
 *      i COMES BEFORE j: by half-plane first - "y < 0, or y == 0 and x < 0" is the second -; within a half-plane when
 *      c = x_i y_j - x_j y_i > 0, not when c < 0; any other outcome (c == 0, a NaN) is a TIE, which goes to the smaller half-edge id - so
 *      degenerate and non-finite geometry orders by id alone.  A half-edge's position is the NUMBER of half-edges of its edge that come before
 *      it, equal numbers in ascending id: defined whatever rounding does to the transitivity of the comparison, and independent of any sorting
 *      algorithm.  The order starts at the smallest id.  A backward half-edge b -> a has the solid just after it in this order, a forward one
 *      just before it.  wedge 0 = VOID: forward half-edges open, backward ones close - a pair bounds an empty wedge, solids touching along the
 *      edge become one solid.  wedge 1 = SOLID: backward opens, forward closes - the solids are separated.  Bracket matching over the cyclic
 *      sequence: an opener is pushed (first turn only), a closer pops the last opener and the two are a PAIR; two turns around the cycle.
 *      Unmatched half-edges stay UNPAIRED (an unbalanced edge) and end as boundary edges.  An edge with n > 64 is WIDE: left entirely unpaired.
 *   3. CORNER CLASSES: across every edge with n == 2 (manifold, or flipped: a flipped edge is LEFT AS IT IS, orientation repair is out of
 *      scope) and across every pair, the two faces' corners at a are united, and their corners at b.  Every class is one output vertex; the
 *      classes are numbered ascending by (original vertex, smallest corner id of the class): V1 of them.  Unreferenced vertices vanish.
 *   4. MULTI-EDGES: the UNITS of an edge with 2 < n <= 64 are its pairs and its unpaired half-edges.  Two units can land on the same (class at
 *      a, class at b) - the umbrellas at both ends are connected through other faces -, which an indexed mesh cannot express.  Of the units
 *      with one class pair, the one holding the smallest half-edge id keeps the edge; every other unit is SUBDIVIDED.
 *   5. SUBDIVISION: a subdivided unit gets one new vertex m = (v_a + v_b) * 0.5f - fp32, the add, then the multiply.  The M new vertices follow
 *      the V1 class vertices, ordered by the unit's smallest half-edge id.  A face with k = 1 .. 3 subdivided half-edges becomes k + 1 faces:
 *      its polygon is its corners in order with the midpoint of half-edge i inserted after corner i, rotated to start at the midpoint of the
 *      face's lowest subdivided half-edge, and fanned from there: (P0, Pj, Pj+1), j = 1 .. k + 1 - no triangle of that fan is collinear.  The
 *      first triangle takes the face's place, the others are appended after all surviving faces in (face, fan) order.
 *   6. OUTPUT: verts_out [V1 + M, 3]; src_vertex [V1 + M] int32 = the original vertex of a class, -1 for a midpoint; mid_ends [M, 2] int32 =
 *      the output indices of a midpoint's edge ends (at a, at b), for interpolating per-vertex attributes; faces_out = the surviving faces in
 *      input order with the new indices (not rotated), then the appended ones.  Positions come from scans (csrc/pair_scan.h): no atomic
 *      decides one.
 *   GUARANTEE: with wide == 0 and overflow == 0, nerfart_mesh_half_edges of the output reports no non-manifold edge, no bow-tie vertex, no
 *      degenerate and no bad face; if moreover unpaired == 0 and the surviving faces had no boundary and no flipped edge, the output is
 *      watertight.  Repairing the output again returns it unchanged.
 *   nerfart_mesh_repair_workspace_bytes: as nerfart_mesh_topology_workspace_bytes (the same table, the same table_log2 rule, the same
 *     refusals); about 80 bytes per half-edge beside the table.
 *   nerfart_mesh_repair_count: fills the workspace, counts [4] (DEVICE, 8-byte aligned) = {V1, M, surviving faces, appended faces} and info [16]
 *     uint32 (DEVICE): [0] bad faces dropped  [1] degenerate faces dropped  [2] faces cancelled  [3] non-manifold edges met  [4] of them,
 *     edges in which at least one pair was made  [5] half-edges left unpaired (those of wide edges included)  [6] wide edges
 *     [7] vertices split: V1 minus the vertices referenced by a surviving face  [8] units subdivided = M  [9] ties met in the angular
 *     comparisons, one per unordered pair of half-edges  [10] OVERFLOW of a table: must read 0, and does for every table this call accepts
 *     [11 .. 15] zero.  Asynchronous, no host read inside.  Every loop is bounded whatever the faces hold: probe sequences by the tables'
 *     sizes, the walk of a cancel group by its size (only a face of a group with both orientations and p != q walks), the per-edge loops by
 *     64, the ranking of a vertex's classes by their number, the union-finds by the indices.
 *   nerfart_mesh_repair_emit: from the SAME, untouched workspace, the same mesh and table_log2: the four output arrays.  V_out = V1 + M rows
 *     of verts_out and src_vertex, M_out rows of mid_ends, F_out rows of faces_out are the sizes of the caller's arrays (every write is
 *     checked against them).
 * Refused with 2 before any launch: a null pointer (of an array that is not empty), V or F >= 2^31, 3 F >= 2^32, a table_log2 outside 0 .. 31
 * or a table of fewer than 3 F + 1 slots, wedge not 0 or 1, counts not 8-byte aligned, M_out > V_out, V_out > 6 F, F_out > 4 F, a workspace
 * smaller than the query's answer (or not 16-byte aligned). */
size_t nerfart_mesh_repair_workspace_bytes(unsigned V, unsigned F, int table_log2);
int nerfart_mesh_repair_count(const float* verts, const int* faces, unsigned V, unsigned F, int wedge, int table_log2, void* ws, size_t ws_bytes,
                              unsigned* counts, unsigned* info, void* stream);
int nerfart_mesh_repair_emit(const float* verts, const int* faces, unsigned V, unsigned F, int table_log2, const void* ws, size_t ws_bytes,
                             float* verts_out, int* faces_out, int* src_vertex, int* mid_ends, unsigned V_out, unsigned M_out, unsigned F_out,
                             void* stream);

/* ---- mesh simplification by vertex clustering with quadric error metrics (csrc/mesh_simplify.hip; mesh_util.simplify_clusters,
 * extract_mesh(simplify_factor=); Lindstrom 2000, the representative placed as in dual contouring).  Additions to ABI 5; no counterpart in the
 * reference.  verts [V, 3] fp32 in GRID coordinates - grid point (i, j, k) sits at (i, j, k), nerfart_mc_emit with spacing 1, origin 0 -,
 * faces [F, 3] int32, the cluster factor c >= 2, the grid (nx, ny, nz).  tests/mesh_simplify_ref.py states all of this in numpy.
 *   THE CLUSTER of a vertex: per axis min((int)floorf(x), n - 1) / c in INTEGER division - no floating-point division decides a cluster, so a
 *     vertex exactly on a grid point lands in the same cluster in any implementation.  The lattice has l = ceil(n / c) cells per axis (the last
 *     ragged when n % c != 0); the linear cell index is x-major like the volume: (kx ly + ky) lz + kz.  A vertex with a non-finite coordinate or
 *     one outside [0, n - 1] is BAD: it joins nothing and sets the flag.
 *   THE NUMBERING: the occupied cells in ascending linear order are the new vertices 0 .. V' - 1; cluster [V] int32 = the new vertex of every
 *     old one (-1 for a bad one).
 *   THE QUADRICS, per cluster in its local frame - origin at the cell's centre, unit = the cell's edge: p = (g - c (k + 1/2)) / c.  Every face
 *     with (all indices in [0, V) and) n = (b - a) x (c - a) != 0 (edges in local units) adds the plane quadric (n . (x - a))^2, i.e.
 *     A += n n^T and b += n (n . a), once to every DISTINCT cluster among its three vertices, `a` taken in that cluster's frame.  (The
 *     constant a . A a does not enter the argmin and is not accumulated.)  Every cluster also sums its members' local positions and counts them.
 *     The sums are ORDER-INDEPENDENT: every fp32 term enters a 64-bit integer sum as round(term 2^40) by an integer atomicAdd.  The quantum is
 *     2^-40; a term with NOT |term| <= 2^6, or more than 2^16 face contributions or member vertices in one cluster, sets the flag - within the
 *     guards every sum stays below 2^62 and cannot wrap.  Two runs give the same bits.
 *   THE REPRESENTATIVE (fp64, one thread per cluster): x* = argmin x^T A x - 2 b^T x + lambda |x - m|^2 with m the mean member position and
 *     lambda = reg tr(A) / 3 - so cond(A + lambda I) <= 1 + 3 / reg and no rank decision is made; tr(A) == 0 gives x* = m.  x* is clamped
 *     component-wise to the cell [-1/2, 1/2]^3 and mapped back: verts_out [V', 3] fp32 = c (k + 1/2) + c x*, in grid coordinates.
 *   THE FACES: every index goes through `cluster`; the triple is rotated so that its smallest index comes first (the orientation is kept);
 *     a face with fewer than three distinct indices is dropped; of faces with the same rotated triple only the FIRST in input order survives;
 *     the survivors are compacted in input order (csrc/pair_scan.h, no atomics): faces_out [F', 3] int32.  The duplicates are found with an
 *     open-addressing table of face indices (atomicCAS from empty, atomicMin among equal keys) whose outcome - the smallest index per key -
 *     does not depend on the order of work.
 *   nerfart_mesh_simplify_workspace_bytes: the size of the caller's workspace for the two calls below (0 = refused, see nerfart_last_error).
 *   nerfart_mesh_simplify_count: fills the workspace, cluster [V] and counts [3] (DEVICE, 8-byte aligned) = {V', F', 1 if anything was bad: a face
 *     index outside [0, V), a bad vertex, a guard of the sums}.  Asynchronous.  With the flag set the other outputs mean nothing.
 *   nerfart_mesh_simplify_emit: from the SAME, untouched workspace and cluster array: verts_out [V_out, 3] and faces_out [F_out, 3]; V_out and
 *     F_out are the sizes of the caller's arrays (every write is checked against them); both 0 launches nothing.
 * Refused with 2 before any launch: a null pointer (of an array that is not empty), c < 2, a grid dimension outside 1 .. 2^24, a lattice of 2^31
 * cells or more, V >= 2^31, F >= 2^30, counts not 8-byte aligned, reg outside (0, 1e6], V_out > min(V, cells) or F_out > F, a workspace smaller
 * than the query's answer (or not 16-byte aligned). */
size_t nerfart_mesh_simplify_workspace_bytes(unsigned V, unsigned F, int c, int nx, int ny, int nz);
int nerfart_mesh_simplify_count(const float* verts, const int* faces, unsigned V, unsigned F, int c, int nx, int ny, int nz, void* ws, size_t ws_bytes,
                                int* cluster, unsigned* counts, void* stream);
int nerfart_mesh_simplify_emit(const int* faces, unsigned V, unsigned F, int c, int nx, int ny, int nz, double reg, const void* ws, size_t ws_bytes,
                               const int* cluster, float* verts_out, int* faces_out, unsigned V_out, unsigned F_out, void* stream);

/* ---- per-face texture atlas of an indexed mesh (csrc/mesh_texture.hip; mesh_util.texel_points / bake_texture / write_obj,
 * extract_mesh(texture_model=)): where every texel of the atlas sits in space, and a Newton step that puts such points back onto the level set.
 * Additions to ABI 5; no counterpart in the reference.  The colours are the caller's queries of the radiance net at these points.
 * tests/mesh_texture_ref.py states all of this in numpy.
 *   THE LAYOUT of F >= 1 faces at patch size P >= 1 (texel intervals along a triangle's legs): cell side S = P + 3; n_cells = ceil(F / 2); Cw the
 *     smallest integer with Cw^2 >= n_cells; Ch = ceil(n_cells / Cw); image width W = Cw S, height H = Ch S, row 0 the TOP row.  Cell q sits at
 *     column q % Cw, row q / Cw, and holds the faces 2 q (lower) and 2 q + 1 (upper).  Texel (x, y) has the cell (x / S, y / S) and the local
 *     coordinates (i, j) = (x % S, y % S): with i + j <= P + 2 it belongs to the lower face with (a, b) = (i, j), otherwise to the upper face with
 *     (a, b) = (S - 1 - i, S - 1 - j).  It is VALID iff its face index is < F (with an odd F the last upper half is not).
 *   THE POINT of a valid texel: w1 = a / P, w2 = b / P, w0 = (P - a - b) / P (= 1 - w1 - w2; each one correctly rounded fp32 division of small
 *     integers), p = fma(w2, v2, fma(w1, v1, w0 * v0)) per coordinate, v0 v1 v2 the face's vertices in face order.  The weights run from -2 / P
 *     to (P + 2) / P: texels outside the triangle are the GUTTER, points of the face's plane at extrapolated barycentrics.
 *   THE UVS (pixel units, texel centres at + 0.5, relative to the cell's origin): lower face (0.5, 0.5), (0.5 + P, 0.5), (0.5, 0.5 + P); upper
 *     face S minus those.  With them, bilinear sampling at the UV of any point of a face (edges and corners included) reads, with non-zero
 *     weight, only texels of that face, and texels carrying an affine function of their points return that function at the surface point.
 *     OBJ's vt is u = X / W, v = 1 - Y / H.  Mip-mapping would read across cells: the atlas is for bilinear filtering at full resolution.
 *   nerfart_mesh_atlas_layout: HOST only.  dims [5] (HOST) = {S, Cw, Ch, W, H}.  Refused with 2: P < 1, F < 1, W or H above 16384.
 *   nerfart_mesh_atlas_points: verts [V, 3] fp32, faces [F, 3] int32; points [W H, 3] fp32 and face_of [W H] int32 in row-major texel order
 *     (y W + x).  face_of = the owning face, -1 for an invalid texel, whose point is written as 0: every element of both arrays is written.
 *     info [1] int32 (DEVICE) is zeroed, then set to 1 when a face holds an index outside [0, V): the texels of such a face are written as
 *     invalid and nothing is read out of bounds.  One thread per texel, lanes along x, no atomics: two runs give the same bits.  Refusals as
 *     the layout's, plus a null pointer and V >= 2^31.
 *   nerfart_mesh_project_step: points [n, 3] in place, given sdf [n] and nabla [n, 3] at them: one Newton step toward sdf == level,
 *     d = -(sdf - level) g / |g|^2, no longer than max_step.  Per point (fp32, every operation rounded once, in the order written):
 *       1. sdf or a component of g not finite: the point stays.  g2 = fma(gz, gz, fma(gy, gy, gx * gx)); g2 < 1e-12 or not finite: it stays.
 *       2. e = sdf - level;  gn = sqrt(g2);  m = min(|e| / gn, max_step);  c = copysign(m, -e) / gn;  c not finite: it stays.
 *       3. p[k] = p[k] + c * g[k].
 *     n == 0 launches nothing.  Refused with 2: a null pointer, max_step not positive. */
int nerfart_mesh_atlas_layout(long long F, long long P, int* dims);
int nerfart_mesh_atlas_points(const float* verts, const int* faces, unsigned V, unsigned F, int P, float* points, int* face_of, int* info,
                              void* stream);
int nerfart_mesh_project_step(float* points, const float* sdf, const float* nabla, unsigned n, float level, float max_step, void* stream);

/* ---- rasteriser for an indexed mesh (csrc/mesh_raster.hip; mesh_util.rasterize / render_mesh, tools/render_mesh.py): what a rend_util.get_rays
 * camera sees of the mesh extract_mesh wrote.  Additions to ABI 5; no counterpart in the reference.  Every decision is an integer, every float
 * result is computed once in the order written here, and nothing depends on the order of work: tests/mesh_raster_ref.py states all of this in
 * numpy and the GPU tests compare for equality.
 *   THE CAMERA: c2w is a 4x4 row-major OpenCV camera; the HOST inverts it in float64 and passes w2c [12] (the 3x4, rounded to fp32 once), rot [9]
 *     (c2w's rotation) and K5 [5] = (fx, sk, cx, fy, cy) = K[0], K[1], K[2], K[5], K[6] of the 4x4 K, as k_get_rays reads it - all HOST arrays.
 *     Pixel (column i, row j) is sampled at its integer coordinates, NO half-pixel offset, index j W + i (csrc/raygen.hip).  A camera-space
 *     point (X, Y, Z) projects to u = fx X/Z + sk Y/Z + cx, v = fy Y/Z + cy: the inverse of lift.  The ray of pixel (i, j) is r = (x, y, 1),
 *     x = ((i - cx + cy sk / fy) - sk j / fy) / fx, y = (j - cy) / fy: k_get_rays' expressions.  All of it in double from the fp32 numbers,
 *     every operation rounded once (no fma), sums left to right.
 *   nerfart_mesh_project, one thread per vertex: (X, Y, Z) = w2c (p, 1) per row ((m0 px + m1 py) + m2 pz) + m3; xz = X / Z, yz = Y / Z;
 *     u = (fx xz + sk yz) + cx, v = fy yz + cy.  The vertex is INVALID when NOT Z >= near (NaN included) or NOT |u| <= 2^15 or NOT |v| <= 2^15.
 *     xy_fix [V, 2] int32 = rint(256 u), rint(256 v) (round half to even; 8 sub-pixel bits; 0 0 for an invalid vertex); cam [V, 3] fp32 = the
 *     double (X, Y, Z) rounded once (written for every vertex); valid [V] uint8.
 *   nerfart_mesh_raster: sets zbuf [H W] uint64 to all ones and info [4] int32 to 0 on the caller's stream, then per face:
 *       1. an index outside [0, V): info[0] = 1, the face is skipped.
 *       2. an invalid vertex: the face is skipped WHOLE and counted in info[1] (integer atomic).  THERE IS NO POLYGON CLIPPING: a face that
 *          crosses the near plane, or reaches beyond 2^15 pixels, is not drawn at all.
 *       3. A = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) in int64 from xy_fix; A == 0: skipped.  A < 0: corners 1 and 2 are swapped, so that
 *          A > 0 (both orientations are drawn; there is no back-face culling).
 *       4. COVERAGE of pixel (i, j), sample s = (256 i, 256 j): for each directed edge a -> b of (0 1, 1 2, 2 0),
 *          E = (xb - xa)(sy - ya) - (yb - ya)(sx - xa) in int64 (|coordinate| <= 2^23, |difference| <= 2^24, |product| <= 2^48).  The pixel
 *          is covered iff for every edge E > 0, or E == 0 and the edge is a TOP or LEFT edge.  y runs down and A > 0, so the corners run
 *          clockwise on screen: TOP is yb == ya and xb > xa (horizontal, the face below it), LEFT is yb < ya (running up, the face to its
 *          right).  A sample on an edge two faces share belongs to exactly one of them; nothing about coverage is floating point.
 *       5. at a covered pixel, in double: n = (b - a) x (c - a) from the three cam vertices in the face's own order (fp32 values, unsnapped),
 *          z = ((nx ax + ny ay) + nz az) / ((nx x + ny y) + nz).  NOT z >= near, or z not finite: nothing is written, info[2] counts it.
 *       6. key = (bits(float(z)) << 32) | face, atomicMin on unsigned long long.  z > 0, so the bit patterns order as the floats do; equal
 *          depths go to the smaller face index; the winner does not depend on the order of the faces.  No float atomics.
 *     Work: one thread per face; the clipped box i in [ceil(xmin / 256), floor(xmax / 256)] x the same in j, cut to the image, is walked by that
 *     thread when it holds at most 256 pixels; otherwise the face is appended to list [F] int32 (integer atomic, info[3] counts; the image
 *     does not depend on the list's order) and a second launch works the list one workgroup per face, threads across the box.
 *   nerfart_mesh_resolve, one thread per pixel, lanes along x: face = low word of the key, -1 for all ones.  z as in 5 (the same bits), the hit
 *     point h = z r, and the barycentrics as signed areas against the face's own normal:
 *       w0 = n . ((b - h) x (c - h)) / (n . n),  w1 = n . ((c - h) x (a - h)) / (n . n),  w2 = n . ((a - h) x (b - h)) / (n . n).
 *     They may leave [0, 1] by what the 1/256-pixel snap allows - harmless: the atlas's gutter texels exist for extrapolated weights.
 *     Outputs, each rounded to fp32 once: face_id [H W] int32, bary [H W, 3], z [H W], depth [H W] = z sqrt((x x + y y) + 1) - the distance
 *     along the UNIT ray, which is what render_fn's depth_volume and surface_render's depths are (both normalise rays_d before they march) -,
 *     mask [H W] uint8, normals [H W, 3] = rot (s n / |n|) with s = -1 if n . r > 0 else 1: the geometric normal in world space, turned
 *     toward the camera.  A miss writes -1 and zeros.
 *   nerfart_mesh_interp, one thread per pixel: out [n, C] fp32 = fma(w2, a2, fma(w1, a1, w0 * a0)) with a_k the attribute of corner k of the
 *     pixel's face: attr [V, C] gathered through faces [F, 3] (per vertex), or attr [F, 3, C] with faces == NULL (per corner, e.g. UVs).
 *     1 <= C <= 8.  face_id < 0 (or a face / vertex index out of range): every channel = fill.
 *   nerfart_mesh_sample_bilinear, one thread per sample: uv [n, 2] fp32 in PIXEL units of image [Ht, Wt, 3] uint8 under the atlas_uvs /
 *     write_obj convention (the centre of texel (x, y) is at (x + 0.5, y + 0.5), y runs down).  fp32, every operation rounded once:
 *     X = u - 0.5, x0 = floor(X) (clamped to [-1, Wt]), tx = X - x0 (clamped to [0, 1]); likewise Y, y0, ty; texel columns x0 and x0 + 1 and
 *     rows y0 and y0 + 1 clamped into the image (clamp to edge); per channel top = fma(tx, t10 - t00, t00), bot = fma(tx, t11 - t01, t01),
 *     out = fma(ty, bot - top, top) / 255.  mask [n] uint8 (may be NULL) == 0, or a non-finite uv: out = background [3] (HOST).
 * Refused with 2 before any launch: a null pointer (of an array that is not empty), H or W (Ht or Wt) outside 1 .. 16384, fx or fy zero, a
 * non-finite camera number, near not positive and finite, V or F >= 2^31, C outside 1 .. 8. */
int nerfart_mesh_project(const float* verts, unsigned V, const float* w2c, const float* K5, float near, int* xy_fix, float* cam,
                         unsigned char* valid, void* stream);
int nerfart_mesh_raster(const int* xy_fix, const float* cam, const unsigned char* valid, const int* faces, unsigned V, unsigned F, const float* K5,
                        float near, int H, int W, unsigned long long* zbuf, int* list, int* info, void* stream);
int nerfart_mesh_resolve(const unsigned long long* zbuf, const float* cam, const int* faces, unsigned V, unsigned F, const float* K5, const float* rot,
                         int H, int W, int* face_id, float* bary, float* z, float* depth, unsigned char* mask, float* normals, void* stream);
int nerfart_mesh_interp(const int* face_id, const float* bary, const int* faces, const float* attr, unsigned V, unsigned F, int C, unsigned n,
                        float fill, float* out, void* stream);
int nerfart_mesh_sample_bilinear(const float* uv, const unsigned char* mask, const unsigned char* image, int Ht, int Wt, unsigned n,
                                 const float* background, float* out, void* stream);

/* ---- distance between two meshes (csrc/mesh_distance.hip; mesh_util.sample_surface / closest_on_mesh / mesh_distance, tools/compare_mesh.py):
 * area-weighted samples of one indexed mesh and, for any points, the exact closest point of another.  Additions to ABI 5; no counterpart in the
 * reference.  verts [V, 3] fp32, faces [F, 3] int32.  tests/mesh_distance_ref.py states all of this in numpy.  All floating point here is fp64 from
 * the fp32 inputs, every operation rounded once (no fused multiply-add), sums of three as (x + y) + z, in the order written.  No float atomics;
 * results are a pure function of the inputs: two calls give the same bits.  Everything runs on the caller's stream in the caller's workspace.
 *   A BAD face has an index outside [0, V) or a non-finite vertex coordinate; every other face is GOOD (a zero-area face is good).
 *   THE HASHES, in wrapping 32-bit unsigned arithmetic:
 *       mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *       key(seed, f) = mix(mix(seed) ^ mix(f + 0x9e3779b9))
 *       h(seed, f) = mix(key ^ 0x68e31da4) / 2^32                                  - in [0, 1), exact in fp64
 *       s(seed, f, j) = mix(key + 0x85ebca6b (j + 1));  u = mix(s ^ 0xb5297a4d) / 2^32,  v = mix(s ^ 0x1b56c4e9) / 2^32
 *   SAMPLING, count: per good face e1 = b - a, e2 = c - a; n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x);
 *     a_f = 0.5 sqrt((nx nx + ny ny) + nz nz); x_f = density a_f + h(seed, f); n_f = floor(x_f) samples - stochastic rounding: the expected count
 *     is density a_f, every face independent of every other.  A bad face gets none; a zero-area face gets none by the rule (h < 1).  x_f >= 2^31:
 *     none, and the overflow flag.  The offsets are the exclusive scan of n_f (csrc/pair_scan.h, no atomics).
 *   SAMPLING, emit: sample i belongs to the face f with off[f] <= i < off[f] + n_f, j = i - off[f]; (u, v) from the hash; u + v > 1: u = 1 - u,
 *     v = 1 - v (reflected into the triangle); point[k] = float((a[k] + u e1[k]) + v e2[k]).  Samples come face by face: spatially coherent.
 *   nerfart_mesh_sample_workspace_bytes(F): the workspace of the two calls below (0 = refused, see nerfart_last_error).  It BEGINS with
 *     off [max(F, 1)][2] uint32: off[f][0] = the offset of face f's first sample, off[f][1] = the bad faces before f.
 *   nerfart_mesh_sample_count: fills the workspace and info [4] uint32 (DEVICE, 8-byte aligned) = {n, bad faces, 1 if a count or their sum
 *     reached 2^31 (the other outputs then mean nothing), 0}.  Asynchronous.
 *   nerfart_mesh_sample_emit, after a host read of n, from the SAME untouched workspace and the same mesh and seed: points [n, 3] fp32,
 *     face [n] int32.  n is the size of the caller's arrays: every write is checked against it, and an element beyond the workspace's own total
 *     is written as (0, 0, 0), -1.  n == 0 launches nothing.
 *   THE DISTANCE of a point p to a good face (a, b, c), squared: the minimum of
 *       the three point-segment terms, for (a, b), (b, c), (c, a): e = end - start, w = p - start, ee = e . e, t = clamp((w . e) / ee, 0, 1)
 *         (t = 0 when ee == 0), q = w - t e, the term q . q; and,
 *       when nn = n . n > 0 with n = (b - a) x (c - a), and the three edge functions n . ((b - a) x (p - a)), n . ((c - b) x (p - b)),
 *         n . ((a - c) x (p - c)) are all >= 0: the plane term (n . (p - a))^2 / nn.
 *     A degenerate face is thus its edges.  The RESULT for p is the lexicographic minimum of (d^2, face) over all good faces: ties go to the
 *     lowest face index, and the order in which faces are visited does not matter.
 *   THE GRID (gx, gy, gz) spans the box [lo, hi] of the good faces' vertices (exact: integer atomicMin / atomicMax on the order-preserving
 *     encoding of the fp32 bits).  Per axis: cell size s = (hi - lo) / g, inv = g / (hi - lo), the cell of x = clamp(floor((x - lo) inv), 0, g - 1);
 *     an axis with hi == lo has ONE cell whatever g says, and so has every axis when there is no good face.  The linear index is
 *     (cx gy + cy) gz + cz.  A good face is entered into every cell its axis-aligned box overlaps (cell of its min .. cell of its max per axis:
 *     conservative): counted per cell by integer atomicAdd, scanned, then written through per-cell integer cursors.  The order within a cell is
 *     free because the query takes a minimum.
 *   THE SEARCH, per point: its own cell c (clamped, so a point outside the box starts at the nearest boundary cell); for r = 0, 1, ... the cells
 *     of Chebyshev distance exactly r from c that exist; after ring r the visited box is [c - r, c + r] cut to the grid, and nothing unvisited
 *     is nearer than B = the smallest of p[k] - (lo[k] + (c[k] - r) s[k]) over the axes with c[k] - r > 0 and (lo[k] + (c[k] + r + 1) s[k]) - p[k]
 *     over those with c[k] + r < g[k] - 1: the inward distances to the sides of the visited box that are not the grid's own boundary (no such
 *     side: everything has been visited).  B is made conservative against the rounding of the cell rule: B' = max(B (1 - 2^-20) - 2^-30 m, 0),
 *     m = the largest |coordinate| of the box + the largest of p.  The search STOPS after the ring at which min(best d, max_distance) < B',
 *     strictly, so that an unvisited face can never tie with the reported one: the answer does not depend on the grid.
 *   nerfart_mesh_grid_workspace_bytes(gx, gy, gz): the grid's workspace (0 = refused).
 *   nerfart_mesh_grid_count: box, cell counts and offsets into the workspace; info [2] uint64 (DEVICE, 8-byte aligned) = {entries, good faces}.
 *     With 2^31 entries or more nothing is counted per cell, and nerfart_mesh_grid_fill / nerfart_mesh_closest refuse such a number.
 *   nerfart_mesh_grid_fill, after a host read of `entries`, same mesh, grid and workspace: list [entries] int32, the faces cell by cell.
 *   nerfart_mesh_closest: points [n, 3] fp32 against the mesh through the filled workspace and list (neither is modified).  dist [n] fp32 = the
 *     fp64 square root of the minimum, rounded once; face [n] int32.  max_distance (double >= 0, infinity allowed) bounds the search: a point
 *     with d > max_distance reports dist = float(max_distance), face = -1, and so does every point when the mesh has no good face.  A point
 *     with a non-finite coordinate reports NaN, -1.  visited [n] uint32 (may be NULL) = the faces tested for the point, with repetition.
 *     One thread per point; every loop is bounded by the grid, the ring and the cell's count; every read of list is checked against entries.
 * Refused with 2 before any launch: a null pointer (of an array that is not empty), V, F or n >= 2^31, info not 8-byte aligned, a density that
 * is negative or not finite, n > 0 with F == 0 (emit), a grid dimension outside 1 .. 1024 or more than 2^24 cells, entries >= 2^31,
 * max_distance negative or NaN, a workspace smaller than the query's answer (or not 16-byte aligned). */
size_t nerfart_mesh_sample_workspace_bytes(unsigned F);
int nerfart_mesh_sample_count(const float* verts, const int* faces, unsigned V, unsigned F, double density, unsigned seed, void* ws, size_t ws_bytes,
                              unsigned* info, void* stream);
int nerfart_mesh_sample_emit(const float* verts, const int* faces, unsigned V, unsigned F, unsigned seed, const void* ws, size_t ws_bytes, float* points,
                             int* face, unsigned n, void* stream);
size_t nerfart_mesh_grid_workspace_bytes(int gx, int gy, int gz);
int nerfart_mesh_grid_count(const float* verts, const int* faces, unsigned V, unsigned F, int gx, int gy, int gz, void* ws, size_t ws_bytes,
                            unsigned long long* info, void* stream);
int nerfart_mesh_grid_fill(const float* verts, const int* faces, unsigned V, unsigned F, int gx, int gy, int gz, void* ws, size_t ws_bytes, int* list,
                           unsigned long long entries, void* stream);
int nerfart_mesh_closest(const float* points, unsigned n, const float* verts, const int* faces, unsigned V, unsigned F, int gx, int gy, int gz,
                         const void* ws, size_t ws_bytes, const int* list, unsigned long long entries, double max_distance, float* dist, int* face,
                         unsigned* visited, void* stream);

/* ---- narrow-band SDF sweep (csrc/mesh_band.hip; mesh_util.banded_volume, extract_mesh(narrow_band=True)): the device side of a sweep that
 * queries the SDF only in the bricks of the grid that can hold the isosurface.  Additions to ABI 5; no counterpart in the reference.  The SDF
 * queries themselves are the caller's: these entry points make points, keep per-brick flags and move values.
 *   THE GRID: points (i, j, k) in 0 .. N - 1, z fastest, vol [N, N, N] fp32.  Brick edge B in 2 .. 64; brick (bx, by, bz) owns the points with
 *     i / B == bx, j / B == by, k / B == bz; nb = ceil(N / B) per axis (the last ragged when N % B != 0); n_bricks = nb^3; linear brick index
 *     (bx nb + by) nb + bz.  A brick's probe is the grid point min(b B + B / 2, N - 1) per axis.  The coordinate of index i is
 *     (float)((double)i * step + org) with the product and the sum rounded separately (NO fma): mesh_util.grid_points' bits.
 *   nerfart_band_workspace_bytes: the size of nerfart_band_select's workspace (0 = bad dimensions, see nerfart_last_error).
 *   nerfart_band_probe_points: pts [n_bricks, 3] = the probe points in brick order.
 *   nerfart_band_select: which bricks become active now, as the ascending list of them.  NEWLY ACTIVE is, by mode: 0 = NOT (|probe[b] - level| >
 *     threshold) in fp32 (a NaN probe is active), flag is overwritten;  1 = wanted[b] != 0 and flag[b] == 0;  2 = flag[b] == 0 (everything left).
 *     Writes list [n] int32 (ascending brick indices), ptoff [n] uint32 (the number of owned points of the list's earlier bricks: where the
 *     brick's points start in the evaluation order), counts [2] (DEVICE, 8-byte aligned) = {n, the owned points of the n bricks}; sets
 *     flag[b] = 1 for them (flag, wanted: [n_bricks] uint8; list, ptoff: room for n_bricks) and clears wanted.  Scan and emit, no atomics.
 *   nerfart_band_brick_points: the batch [first, first + count) of the evaluation order (bricks in list order, inside a brick x slowest / z
 *     fastest over its OWNED points): pts [count, 3] and idx [count] uint32 = the linear grid index (i N + j) N + k.  n_list and n_points are
 *     nerfart_band_select's counts.  A row that list / ptoff do not resolve gets idx = 0xffffffff.  count == 0 launches nothing.
 *   nerfart_band_scatter: vol[idx[t]] = val[t] for t < count; an idx >= N^3 writes nothing.
 *   nerfart_band_fill: every point of a brick with flag == 0 becomes probe[brick]; points of active bricks are not touched.  float4 stores when
 *     N % 4 == 0, B % 4 == 0 and vol is 16-byte aligned.  A ragged last brick writes its owned points only.
 *   nerfart_band_check: over all grid edges (per point toward +x, +y, +z where the neighbour exists), with marching cubes' predicate (inside iff
 *     value < level; NaN is outside): an edge whose ends differ sets wanted[b] = 1 for every brick b with flag[b] == 0 that holds one of its ends
 *     (plain byte stores).  Then counts [2] (DEVICE) = {bricks with wanted != 0, their owned points}: zeroed, summed per block, one integer
 *     atomicAdd per block and counter - integer adds commute, two runs give the same numbers.  wanted must come in cleared
 *     (nerfart_band_select leaves it so).
 * Refused with 2 before any launch: a null pointer, N < 2, B outside 2 .. 64, N^3 >= 2^31, a mode outside 0 .. 2, counts not 8-byte aligned
 * (select), a workspace smaller than the query's answer (or not 16-byte aligned), n_list == 0 or > n_bricks, n_points > N^3 or
 * first + count > n_points (brick_points). */
size_t nerfart_band_workspace_bytes(int N, int B);
int nerfart_band_probe_points(int N, int B, double step, double org, float* pts, void* stream);
int nerfart_band_select(int mode, const float* probe, float level, float threshold, int N, int B, unsigned char* flag, unsigned char* wanted,
                        int* list, unsigned* ptoff, void* ws, size_t ws_bytes, unsigned* counts, void* stream);
int nerfart_band_brick_points(const int* list, const unsigned* ptoff, unsigned n_list, unsigned n_points, unsigned first, unsigned count, int N, int B,
                              double step, double org, float* pts, unsigned* idx, void* stream);
int nerfart_band_scatter(const float* val, const unsigned* idx, unsigned count, int N, float* vol, void* stream);
int nerfart_band_fill(const float* probe, const unsigned char* flag, int N, int B, float* vol, void* stream);
int nerfart_band_check(const float* vol, float level, const unsigned char* flag, int N, int B, unsigned char* wanted, unsigned* counts, void* stream);

/* ---- VGG16 perceptual term (criteria/perp_loss.py:9-57): torchvision vgg16.features[:16] (through relu3_3) as
 * implicit-GEMM 3 x 3 convolutions on v_mfma_f32_32x32x2_f32 (fp32 operands as the reference's net; csrc/vgg_conv.hip), L1
 * between prediction and target features.
 *   blob : nerfart_vgg16_blob_layout() sections (offsets[22] bytes; packed by nerfart_amd/vgg.py): per conv l = 0..6 forward
 *          weights, backward (tap-flipped, channel-transposed) weights, bias - all fp32; blob_bytes must equal the layout's total.
 *   img2 : [2, 3, H, W] fp32 = the ImageNet-normalised, resized prediction then target (perp_loss.py:41-45); H, W multiples of 4,
 *          H W / 16 a multiple of 64 (224 x 224 in the reference).
 * nerfart_vgg16_l1_fwd writes loss_out[0] (device) = mean |relu3_3(pred) - relu3_3(target)|; with keep_for_bwd the workspace
 * (nerfart_vgg16_workspace_bytes) keeps the activations and nerfart_vgg16_l1_bwd turns upstream[0] (device scalar, NULL = 1)
 * into g_img [1, 3, H, W] = d loss / d img2[0].
 *
 * nerfart_vgg16_workspace_layout returns the same total as nerfart_vgg16_workspace_bytes (0 for H < 8 or W < 8) and, with offsets != NULL,
 * fills offsets[15] with the byte offsets (256-byte aligned) of the workspace's buffers, in this order.  Every activation is NHWC fp32 and
 * holds BOTH images, the prediction's rows first (image b, pixel (y, x), channel c at ((b h + y) w + x) C + c); h = H / 2^level, w = W / 2^level:
 *    0  loss    64 floats: [0] the loss the forward accumulates, [8] the backward's scale = upstream / n, n = (H / 4)(W / 4) 256
 *    1  cols    [2 H W, 32]    im2col of img2: column c 9 + ky 3 + kx < 27 = img2[b, c, y + ky - 1, x + kx - 1] (0 outside), columns 27..31 = 0
 *    2  y[0]    [2, H, W, 64]            relu(conv1_1)        3  y[1]  [2, H, W, 64]           relu(conv1_2)
 *    4  y[2]    [2, H/2, W/2, 128]       relu(conv2_1)        5  y[3]  [2, H/2, W/2, 128]      relu(conv2_2)
 *    6  y[4]    [2, H/4, W/4, 256]       relu(conv3_1)        7  y[5]  [2, H/4, W/4, 256]      relu(conv3_2)
 *    8  y[6]    [2, H/4, W/4, 256]       relu(conv3_3): the features the L1 is taken over
 *    9  p[0]    [2, H/2, W/2, 64]        2 x 2 max-pool of y[1]       10  p[1]  [2, H/4, W/4, 128]   2 x 2 max-pool of y[3]
 *   11  ga      keep_for_bwd only (else empty, as gb and dcols); after the forward [H/4, W/4, 256] = sign(fp - ft) [fp > 0] of y[6]
 *               (prediction only; sign(0) = 0).  ga and gb are the backward's ping-pong cotangent buffers, H W x 64 floats each: the backward
 *               OVERWRITES ga (run the forward again before a second backward) and leaves in it [H W, 64] = the cotangent of y[0], masked
 *   12  gb      after the backward [H, W, 64] = the un-pooled cotangent of y[1], masked by y[1] > 0 (what conv1_2's backward read)
 *   13  dcols   [H W, 64]  after the backward: column k = c 9 + ky 3 + kx < 27 = d loss n / d cols[pixel, k] of the prediction (before the
 *               scale), columns 27..63 = 0; g_img[c, y, x] = scale * sum of the nine dcols entries whose window tap reads pixel (y, x)
 *   14  total
 * The backward decides from the stored fp32 activations: ReLU mask y > 0; un-pool to the first maximum of the 2 x 2 window in row-major
 * scan (strict >), and only if that maximum is > 0. */
long long nerfart_vgg16_blob_layout(long long* offsets);
long long nerfart_vgg16_workspace_bytes(int H, int W, int keep_for_bwd);
long long nerfart_vgg16_workspace_layout(int H, int W, int keep_for_bwd, long long* offsets);
int nerfart_vgg16_l1_fwd(const void* blob, long long blob_bytes, const float* img2, int H, int W, float* loss_out, int keep_for_bwd, void* workspace,
                         long long workspace_bytes, void* stream);
int nerfart_vgg16_l1_bwd(const void* blob, long long blob_bytes, int H, int W, const float* upstream, float* g_img, void* workspace, long long workspace_bytes, void* stream);

/* ---- weight-gradient reductions of pass 2 (row a19; what autograd accumulates through volsdf.py:759-770): for n_mats matrix
 * pairs, dW[m] [256, a_cols] fp32 = Z_m^T A_m over `rows` rows and, if cs != NULL, cs[m] [256] = column sums of the first cs_rows
 * rows of Z_m (the bias gradients).  Z_m [rows, 256] and A_m [rows, a_cols] (a_cols = 256 or 64) are bf16 row-major matrices
 * z_stride / a_stride BYTES apart (the point-major dumps of the backward kernels, read in place; a stride of 0 shares one
 * operand); 16-byte aligned.  accumulate != 0 adds to dW / cs.  workspace = nerfart_wgrad_workspace_bytes(n_mats, rows, a_cols)
 * bytes, caller owned (split-K partial results).  csrc/wgrad.hip: v_mfma_f32_32x32x16_bf16 on ds_read_b64_tr_b16 fragments. */
long long nerfart_wgrad_workspace_bytes(int n_mats, long long rows, int a_cols);
int nerfart_wgrad_bf16(const void* Z, long long z_stride, const void* A, long long a_stride, int n_mats, long long rows, int a_cols,
                       long long cs_rows, float* dW, float* cs, int accumulate, void* workspace, long long workspace_bytes, void* stream);

/* ---- per-point glue of pass 2 (row a19; csrc/pass2_operands.hip): what autograd does between the network calls of
 * volsdf.py:759-770, one pass each.
 *   nerfart_ray_points: pts[R P,3] = rays_o + rays_dn * depth[R,P] (volsdf.py:503-506), view[R P,3] = rays_dn per sample (NULL: skip).
 *   nerfart_volsdf_pass2_cotangents: from the compositor's g_sdf[R P], the radiance net's g_n[R P,3] (+ g_n_extra; either may be NULL = zero) and
 *     pass 1's pts / sdf / nabla: sbar[R P] = g_sdf where the sphere clamp sdf = min(net, R_bg - |x|) kept the net (volsdf.py:97-100,
 *     else 0; R_bg <= 0: no sphere, NeuS), nbar[R P,3] = g_n + the eikonal term's gradient w 2 (|n| - 1) n / (|n| N) with N = the points of the ray's reference
 *     patch (eik_group_rays rays per patch inside this launch, the last one ragged; <= 0: one patch), eik_ray[R] = each ray's share
 *     of w * mean_patch((|n| - 1)^2) (their sum = the sum of the patches' eikonal losses).  w_eikonal = 0: no eikonal term.
 *     A sample with n = 0 gets no eikonal gradient (the zero subgradient of |n|, as torch's norm backward) and still counts (0 - 1)^2 in eik_ray.
 *   nerfart_wgrad_operand_*: the narrow (a_cols = 64) operands of nerfart_wgrad_bf16 from fp32 data: hi parts bf16(x) in columns
 *     0..c-1 and, when c <= 32, lo parts bf16(x - hi) in columns 32..32+c-1 (add the two halves of dW); rows M.. zero.
 *       _embed_pair: [2 rows_pad, 64]: embed(pts) (models/base.py:46-64, multires < 0: identity) in rows 0.., its tangent along dir in
 *                    rows rows_pad.. (the input side of SDF layers 0 and 4 for the stacked [value; tangent] dumps)
 *       _inputs:     [rows_pad, 64]: [embed(x, multires_x) | embed(view, multires_view) | normals] (radiance layer 0)
 *       _rgb_delta:  [rows_pad, 64]: g_rgb rgb (1 - rgb) (the output sigmoid's delta, 3 columns); also in fp32 to d4[M,3] (NULL: skip)
 *                    and its sums over each block of 32 rows to block_sums[ceil(rows_pad / 32), 3] (their sum = the bias gradient)
 *       _sbar_ones:  [2 rows_pad, 64]: sbar (1 column) in rows 0.., 1 in rows rows_pad.. (the sdf row of the last SDF layer) */
int nerfart_ray_points(const float* rays_o, const float* rays_dn, const float* depth, long long n_rays, int P, float* pts, float* view,
                       void* stream);
int nerfart_volsdf_pass2_cotangents(const float* pts, const float* sdf, const float* g_sdf, const float* nabla, const float* g_n,
                                    const float* g_n_extra, long long n_rays, int P, float R_bg, float w_eikonal,
                                    long long eik_group_rays, float* sbar, float* nbar, float* eik_ray, void* stream);
int nerfart_wgrad_operand_embed_pair(const float* pts, const float* dir, long long M, long long rows_pad, int multires, void* out,
                                     void* stream);
int nerfart_wgrad_operand_inputs(const float* x, int multires_x, const float* view, int multires_view, const float* normals, long long M,
                                 long long rows_pad, void* out, void* stream);
int nerfart_wgrad_operand_rgb_delta(const float* rgb, const float* g_rgb, long long M, long long rows_pad, void* out, float* d4,
                                    float* block_sums, void* stream);
int nerfart_wgrad_operand_sbar_ones(const float* sbar, long long M, long long rows_pad, void* out, void* stream);

/* ---- B1 "bwd": the RAY-LEVEL backward of the renderer (csrc/render_backward.hip).  What `rgb.backward(gradient)` +
 * `eikonal.backward()` through render_fn do for one patch of rays in the reference (models/frameworks/volsdf.py:759-770,
 * neus.py:520-576) is one call: the whole pass-2 kernel sequence above (points, [SDF + nabla + h7], radiance forward with dumps,
 * compositor backward, radiance backward, cotangents, second-order SDF sweeps, weight-gradient reductions) on the caller's stream,
 * out of one caller-owned workspace.  Split-bf16 blobs (precision 1) only.
 *
 *   raw       : the RAW parameter-gradient buffer, nerfart_pass2_raw_layout(offsets[14]) floats (offsets = float offset of each
 *               section, last = total; returns the total): the fp32 results of the reductions in the kernels' unit order, bias column
 *               sums, and 4 scalars (section 12: d loss / d alpha, d loss / d beta [VolSDF], d loss / d s [NeuS], the sum of the
 *               patches' eikonal losses).  Every call ACCUMULATES into it: zero it once per optimiser step, call once per launch group
 *               (n_rays * P <= 2^21), then nerfart_fold_weight_grads once.  Everything downstream is linear in it, so ranks may also
 *               all-reduce the raw buffer instead of the parameter gradients.
 *   rays_d    : un-normalised, as nerfart_*_render_fwd takes them; d_all [n_rays, P]: the sample depths pass 1 drew (d_all_out of
 *               the forward; sampling carries no gradient, volsdf.py:479).
 *   g_rgb     : d loss / d rgb [n_rays, 3]; g_acc [n_rays] or NULL: d loss / d mask_volume (the mask BCE of neus.py:600-603);
 *               g_n_extra [n_rays, P, 3] or NULL: a further cotangent of the nablas (VolSDF reconstruction objective, volsdf.py:803-806).
 *   *_state   : what pass 1 computed at these samples (sdf_out / nabla_out of the forward, and for VolSDF the layer-7 activation h7
 *               [n_rays P, 256] of nerfart_sdf_nabla_fwd) - same weights, identical values; all NULL: recomputed here.
 *   w_eikonal : weight of mean((|nabla| - 1)^2) (0: no eikonal term); eik_group_rays: the rays are several reference patches of
 *               that many rays in one launch, each with its OWN mean (<= 0: one patch).
 *   train_radiance == 0: the radiance net is frozen (neus.py:455-456): only the SDF net's gradients (incl. the geometry-feature
 *               rows of its last layer) are produced.
 * nerfart_sdf_param_bwd: the SDF net's share on its own - parameter gradients of  sbar . sdf + hbar7 . h7 + nbar . grad_x sdf  at
 *   pts [M, 3] (sbar [M] / hbar7 [M, 256] may be NULL = zero; M <= 2^21): the free eikonal points of volsdf.py:799-806.
 * nerfart_fold_weight_grads: raw -> `folded`, the gradients of the FOLDED weights W = g v / |v| and of the biases in the reference's
 *   feature order, laid out by nerfart_folded_grads_layout(multires, multires_view, offsets[29]): (dW_l [out_l, in_l], db_l [out_l])
 *   for the SDF net's layers 0..8, then the radiance net's 0..4; offsets in floats, last = total (returned).  multires = the SDF
 *   net's embed_multires (6), multires_view = the radiance net's embed_multires_view (-1 | 4).
 * nerfart_weight_norm_bwd: nn.utils.weight_norm's chain rule for one layer (models/base.py:226-227): dW [out, in] ->
 *   g_weight_v [out, in], g_weight_g [out] (either may be NULL; accumulate != 0 adds to them).
 *
 * The raw buffer, slot by slot (tests/param_grad_ref.py holds every element of it to fp64 products of the dumps and operands; unit order
 * throughout; Mp = the padded point count of the dumps):
 *   - EVERY call ADDS to the sections it reduces into - nerfart_sdf_param_bwd: sections 0..5; nerfart_radiance_param_bwd: 6..11; the ray-level
 *     calls: all of them - and touches no other section.  Two calls over disjoint halves of the points give the sums of one call over all of
 *     them (not the same bits: the padding differs).
 *   - written and never read: row 1 of SURF_CS0 (the column sums of zbar_4 once more: the bias of layer 4 is folded from SURF_CS17); the rows
 *     (SURF_WW[2], SURF_CS17[2]) and columns (SURF_WW[3]) at the unit positions of features 217..255 of SDF layer 3, which has 217 outputs
 *     (finite: products of whatever the dumps hold there).
 *   - only zero is added, never read: the columns of the 64-wide sections that no operand column fills (SURF_WE 39..63; SURF_W8 1..31,
 *     33..63; RAD_W4 3..31, 35..63; RAD_WEX nex..31, 32 + nex..63 for nex = 9, 33..63 for nex = 33).  The reduction runs over all 64 columns
 *     and the operands hold 0 there, so each call rewrites them as old + 0: the value is kept (a -0 becomes +0) as long as the dumps are finite.
 *   - never written, never read: SURF_B8[1..3], RAD_B4[3].
 *   - nerfart_fold_weight_grads reads none of the slots of the last three items (NaN there does not reach `folded`) and writes every
 *     element of `folded` up to offsets[28], nothing behind it.
 *   - train_radiance == 0: only RAD_WH7 and row 4 of RAD_CS (the geometry-feature rows of the last SDF layer and their bias) are added to,
 *     with the same bits as with train_radiance != 0; RAD_WW, rows 0..3 of RAD_CS, RAD_W4, RAD_B4 and RAD_WEX are left untouched.
 *   - after the radiance-only route (nerfart_radiance_param_bwd into a zeroed buffer) SURF_W8 and SURF_B8 are 0, so row 0 of dW_8 - the sdf
 *     row of the last SDF layer - its bias entry and their weight_norm gradients come out exactly 0.
 *   - the scalars d loss / d alpha, d beta, d s are sums over the rays formed with atomicAdd (one value per ray, k_composite_*_bwd): no fixed
 *     summation order, so two runs may differ in the last bit.  Every other slot is bit-reproducible; the eikonal scalar is a two-stage sum. */
long long nerfart_pass2_raw_layout(long long* offsets);
long long nerfart_volsdf_render_bwd_workspace_bytes(int n_rays, int P, int have_state);
int nerfart_volsdf_render_bwd(const float* surf_blob, const float* rad_blob, int view_tiles, int multires, const float* rays_o, const float* rays_d,
                              int n_rays, int P, const float* d_all, const float* g_rgb, const float* g_acc, const float* g_n_extra,
                              const float* sdf_state, const float* nabla_state, const float* h7_state, float R_bg, float alpha, float beta,
                              int white_bkgd, float w_eikonal, int eik_group_rays, int train_radiance, float* raw, void* workspace,
                              long long workspace_bytes, void* stream);
/* (addition to ABI 5) nerfart_volsdf_render_bwd plus the cotangents of the depth and normals maps: g_depth [n_rays] / g_normals [n_rays, 3], each may be NULL.
 * After nerfart_volsdf_composite_bwd, nerfart_volsdf_composite_geo_bwd (above: formulas, the empty-ray caveat) adds their share to g_sdf and to the
 * (alpha, beta) scalars of raw, and its nabla cotangent (which already includes g_n_extra) takes g_n_extra's place in nerfart_volsdf_pass2_cotangents;
 * everything after that is nerfart_volsdf_render_bwd's sequence.  Workspace: nerfart_volsdf_render_bwd2_workspace_bytes(n_rays, P, have_state,
 * have_normals = g_normals != NULL) - nerfart_volsdf_render_bwd's plus, with normals, one [n_rays P, 3] buffer.  Both NULL: exactly
 * nerfart_volsdf_render_bwd (same launches, same order, same workspace size).  VolSDF only: the NeuS entry point has no such cotangents. */
long long nerfart_volsdf_render_bwd2_workspace_bytes(int n_rays, int P, int have_state, int have_normals);
int nerfart_volsdf_render_bwd2(const float* surf_blob, const float* rad_blob, int view_tiles, int multires, const float* rays_o, const float* rays_d,
                               int n_rays, int P, const float* d_all, const float* g_rgb, const float* g_acc, const float* g_n_extra,
                               const float* g_depth, const float* g_normals, const float* sdf_state, const float* nabla_state, const float* h7_state,
                               float R_bg, float alpha, float beta, int white_bkgd, float w_eikonal, int eik_group_rays, int train_radiance,
                               float* raw, void* workspace, long long workspace_bytes, void* stream);
long long nerfart_neus_render_bwd_workspace_bytes(int n_rays, int P, int have_state);
int nerfart_neus_render_bwd(const float* surf_blob, const float* rad_blob, int view_tiles, int multires, const float* rays_o, const float* rays_d,
                            int n_rays, int P, const float* d_all, const float* g_rgb, const float* g_acc, const float* sdf_state,
                            const float* nabla_state, float s, int white_bkgd, float w_eikonal, int eik_group_rays, int train_radiance, float* raw,
                            void* workspace, long long workspace_bytes, void* stream);
long long nerfart_sdf_param_bwd_workspace_bytes(long long M);
int nerfart_sdf_param_bwd(const float* surf_blob, int multires, const float* pts, long long M, const float* sbar, const float* hbar7, const float* nbar,
                          float* raw, void* workspace, long long workspace_bytes, void* stream);
/* the radiance net's share on its own (B2 "bwd", parameter level): RadianceNet.forward (models/base.py:372-391) on [pts, view, nabla,
 * W8[1:] h7 + b8[1:]] with its backward - rgb_out [M,3], g_h7_out [M,256], g_n_out [M,3] (each may be NULL) and, accumulated into
 * raw, the gradients of the radiance net (train_radiance != 0) and of the geometry-feature rows of the last SDF layer. */
long long nerfart_radiance_param_bwd_workspace_bytes(long long M);
int nerfart_radiance_param_bwd(const float* rad_blob, int view_tiles, const float* pts, const float* view, const float* nabla, const float* h7,
                               long long M, const float* g_rgb, float* rgb_out, float* g_h7_out, float* g_n_out, int train_radiance, float* raw,
                               void* workspace, long long workspace_bytes, void* stream);
long long nerfart_folded_grads_layout(int multires, int multires_view, long long* offsets);
int nerfart_fold_weight_grads(const float* raw, int multires, int multires_view, float* folded, void* stream);
int nerfart_weight_norm_bwd(const float* dW, const float* weight_v, const float* weight_g, int out_features, int in_features, float* g_weight_v,
                            float* g_weight_g, int accumulate, void* stream);

/* ---- B5: checkpoint -> blobs (reference render.py:266-267 `model.load_state_dict(torch.load(p)['model'])`, models/base.py:226-227
 * `nn.utils.weight_norm`: the state dict holds weight_g [out, 1], weight_v [out, in], bias [out] per layer).  csrc/pack_blob.hip turns
 * those tensors into the blobs every entry point above reads, entirely on the device and on the caller's stream: the weight_norm fold
 * w = g * v / ||v||_row, the permutation into the kernels' fragment order (a closed form the library owns; tests/test_pack_plan.py holds it
 * equal, entry for entry, to the numpy plans of nerfart_amd/packing.py that the CPU emulation walks) and, for the split programs, hi = rne(w),
 * lo = rne(w - hi) in bf16 (precision 1) or fp16 (precision 4).  Call once per weight update (two launches per blob).
 *   precision       : the C-ABI precision the blob is for (5: nerfart_pack_surface_blob only, see the precision list above): 0 fp32, 1 split bf16 ("bf16x3"; also what every training entry point reads),
 *                     4 fp16 hi + lo ("fp16x2"; the sampler blob of nerfart_volsdf_render_mixed_fwd)
 *   weight_g/_v/bias: HOST arrays of DEVICE pointers, one per layer: `implicit_surface.surface_fc_layers.{0..8}.*` (W 256, D 8, skips [4],
 *                     embed_multires 6, W_geo_feat 256 - the four shipped configs) resp. `radiance_net.layers.{0..4}.*` (W 256, D 4;
 *                     view_tiles 1: raw view directions, input 265; 3: embed_multires_view 4, input 289); surf8_*: the SDF net's LAST
 *                     layer, whose rows 1..256 (the geometry feature) the radiance kernels evaluate
 *   blob_out        : nerfart_*_blob_floats(precision, ...) floats (0 = bad arguments, see nerfart_last_error)
 *   workspace       : nerfart_pack_workspace_bytes() bytes of scratch (the rows' 1 / ||v||)
 * nerfart_pack_plan_debug is HOST-only (tests): the layout as plain gather tables - sizes[4] = {chunk elements, aux elements, total floats,
 * chunks}; cindex / cmul (second factor) / aindex: flat indices into [tensors in state-dict order w0, b0, w1, ... | 0.0 | 1.0]; cscale per
 * chunk element; header: the 512 header words.  Any table may be NULL. */
long long nerfart_surface_blob_floats(int precision, int multires);
long long nerfart_radiance_blob_floats(int precision, int view_tiles);
long long nerfart_pack_workspace_bytes(void);
/* (ABI 4) The geometry feature of ImplicitSurface.forward(x, return_h=True) / forward_with_nablas (models/base.py:243-282): rows 1..256 of the SDF net's
 * LAST linear layer on the layer-7 activations, feat = W8[1:] h7 + b8[1:] with W8 = weight_g * weight_v / ||weight_v|| folded on the device (ATen's
 * summation order) and the product on v_mfma_f32_32x32x2_f32 (exact fp32 products; csrc/geo_feature.hip).  weight_g [257], weight_v [257, 256],
 * bias [257]: `implicit_surface.surface_fc_layers.8.*`; h7 [M, 256]: nerfart_sdf_nabla_fwd's output; feat_out [M, 256].  The render path never calls
 * it (the radiance kernels evaluate these rows from their own blob): it serves the reference's other consumers of the callable (boundary B3). */
long long nerfart_geometry_feature_workspace_bytes(void);
int nerfart_geometry_feature(const float* weight_g, const float* weight_v, const float* bias, const float* h7, long long M, float* feat_out,
                             void* workspace, long long workspace_bytes, void* stream);

/* (ABI 4) The architecture the packers index their pointer tables with, as data: radiance == 0 -> the SDF net's 9 layers for embed_multires = arg (6);
 * != 0 -> the radiance net's 5 layers for view_tiles = arg (1 | 3).  rows[l] x cols[l] = weight_v[l]'s shape (weight_g [rows, 1], bias [rows]); the
 * return value is the layer count, 0 on a bad argument.  A host checks a checkpoint against it BEFORE calling nerfart_pack_*_blob (any other W / D /
 * skips / W_geo_feat would be read out of bounds). */
int nerfart_pack_layer_dims(int radiance, int arg, int* rows, int* cols);
int nerfart_pack_surface_blob(int precision, int multires, const float* const* weight_g, const float* const* weight_v, const float* const* bias,
                              float* blob_out, long long blob_floats, void* workspace, long long workspace_bytes, void* stream);
int nerfart_pack_radiance_blob(int precision, int view_tiles, const float* surf8_g, const float* surf8_v, const float* surf8_bias,
                               const float* const* weight_g, const float* const* weight_v, const float* const* bias, float* blob_out, long long blob_floats,
                               void* workspace, long long workspace_bytes, void* stream);
int nerfart_pack_plan_debug(int program, int view_tiles, int fp16, long long* sizes, int* header, int* cindex, int* cmul, float* cscale, int* aindex);

/* The packers of the CLIP / VGG blobs (ABI 3; the weights are frozen: once per run).  CLIP: `tensors` = HOST array of
 * nerfart_clip_vitb32_n_tensors() (= 152) DEVICE pointers to fp32 copies of the `visual.*` entries of the CLIP state dict, tensor i being
 * `visual.` + the name nerfart_clip_vitb32_tensor_name(i, buf, len) writes (its return value: the element count; 0 = bad index) - matrices are
 * stored fp16 (round to nearest even, like `clip.load(device="cuda")`'s weights), vectors fp32.  VGG16: weight[l] [Cout, Cin, 3, 3] / bias[l] of
 * torchvision's `features.{0, 2, 5, 7, 10, 12, 14}` (criteria/perp_loss.py:9-33), fp32 -> the forward / transposed-flipped backward / bias sections. */
int nerfart_clip_vitb32_n_tensors(void);
long long nerfart_clip_vitb32_tensor_name(int i, char* name_out, int name_len);
int nerfart_clip_vitb32_pack(const float* const* tensors, void* blob, long long blob_bytes, void* stream);
int nerfart_vgg16_pack(const float* const* weight, const float* const* bias, void* blob, long long blob_bytes, void* stream);

/* The GEMM kernel of the encoder on its own (tests): C[M,N] fp32 = A[M,K] fp16 . W[N,K]^T fp16; M, N, K multiples of 64. */
int nerfart_gemm_f16_nt(const void* A, const void* W, int M, int N, int K, float* C, void* stream);
/* ... and C[M,N] = A[M,K] . Wt[K,N] (second operand read with its reduction index as the row: the backward GEMMs on the forward
 * weight matrices, through ds_read_b64_tr_b16). */
int nerfart_gemm_f16_nn(const void* A, const void* Wt, int M, int N, int K, float* C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFART_HIP_H */
