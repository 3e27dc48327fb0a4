// volsdf_render.hip - VolSDF Algorithm-1 sampler, sample merge, compositor and the render
// orchestrator (reference models/frameworks/volsdf.py: error_bound :56-94, fine_sample :97-302,
// volume_render :389-615; utils/rend_util.py sample_pdf/sample_cdf :256-328).
//
// All per-ray kernels: one 64-lane wave (= one workgroup) per ray, the ray's samples in LDS.
// The data-dependent up-sampling loop keeps a compacted list of still-active rays; per round it
// runs   upsample (inverse CDF of the error bound, 512 new depths)
//     -> k_sdf_only over (active rays x 512 new points)           [mlp_chain.hip]
//     -> merge + bound check at the net's beta + (converged: 64 inverse-CDF samples of the opacity
//        | else: 10-step bisection for beta+ and re-queue).
// One 4-byte device->host read of the active count per round is the only host synchronisation.
#include "ray_common.h"
#include "host_util.h"
#include <cstdlib>

namespace nerfart {

struct SamplerParams {
    int n;            // samples currently held per active ray
    int cap;          // row stride of the d/s arrays
    int n_up;         // new samples per round (512)
    int n_final;      // N_importance (64)
    int max_bisect;   // 10
    int it;           // round number written to iter_usage on convergence
    float eps;
    float alpha_net, beta_net;
    int u_final_stride;   // 0: one shared table u_final[n_final] (det = True: linspace); n_final: a row per ray (perturb: rand)
    // guard band of the convergence decision `max B > eps` (volsdf.py:162-163, :240-242): a ray whose max B lies within guard * eps of eps is
    // neither sampled nor re-queued here - it is appended to esc_list and Algorithm 1 runs again for it on the escalation blob (fine_sample_run)
    float guard;          // <= 0: off
    int* esc_list;
    int* esc_count;
};

// wave-uniform: is the decision `mx > eps` inside the guard band?  (mx = +inf - a NaN bound - is a clear "not converged")
__device__ __forceinline__ bool in_guard_band(const SamplerParams& P, float mx) {
    return P.guard > 0.f && fabsf(mx - P.eps) <= P.guard * P.eps;
}
__device__ __forceinline__ void escalate(const SamplerParams& P, int ray) {
    if (threadIdx.x == 0) P.esc_list[atomicAdd(P.esc_count, 1)] = ray;
}

// d = near * (1 - t) + far * t with the reference's three roundings (volsdf.py:474, :484)
__global__ void k_linspace_depths(const float* __restrict__ t, int n, const float* __restrict__ near,
                                  const float* __restrict__ far, float near_s, float far_s, int n_rays,
                                  float* __restrict__ out, int stride) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n_rays * n) return;
    const int r = (int)(i / n), k = (int)(i - (long long)r * n);
    const float nr = near ? near[r] : near_s, fr = far ? far[r] : far_s;
    const float tk = t[k];
    out[(size_t)r * stride + k] = __fadd_rn(__fmul_rn(nr, __fsub_rn(1.f, tk)), __fmul_rn(fr, tk));
}

// F.normalize(rays_d, dim=-1): v / max(||v||, 1e-12)   (volsdf.py:442)
__global__ void k_normalize_dirs(const float* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    const float nrm = fmaxf(sqrtf(x * x + y * y + z * z), 1e-12f);
    out[3 * i] = x / nrm; out[3 * i + 1] = y / nrm; out[3 * i + 2] = z / nrm;
}

__device__ __forceinline__ void load_row(float* dst, const float* src, int n) {
    for (int i = threadIdx.x; i < n; i += 64) dst[i] = src[i];
}

__device__ __forceinline__ void emit_final_samples(const float* d, const float* cdf, int n, const float* u_final,
                                                   int n_final, float* out) {
    for (int j = threadIdx.x; j < n_final; j += 64) out[j] = invert_cdf_at(d, cdf, n, u_final[j]);
}

// Round 0: bound check of the initial 512 uniform samples at the net's beta (volsdf.py:159-177).
// Converged rays get their 64 fine samples now; the others are queued with beta+ = beta+_0.  MAXSEG: ray_common.h::scan_maxseg(n).
template <int MAXSEG>
__global__ void __launch_bounds__(64)
k_first_check(SamplerParams P, const float* __restrict__ dA, const float* __restrict__ sA,
              const float* __restrict__ u_final, float beta_plus0_denom, const float* __restrict__ far,
              float far_s, float* __restrict__ d_fine, float* __restrict__ beta_plus, float* __restrict__ beta_map,
              float* __restrict__ iter_usage, int* __restrict__ act_out, int* __restrict__ act_count) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int ray = blockIdx.x;
    float* d = sm; float* s = sm + P.n; float* cdf = sm + 2 * P.n;
    load_row(d, dA + (size_t)ray * P.cap, P.n);
    load_row(s, sA + (size_t)ray * P.cap, P.n);
    __syncthreads();
    const float mx = error_bound_scan<MAXSEG>(d, s, P.n, P.alpha_net, P.beta_net, nullptr, false);
    const float fr = far ? far[ray] : far_s;
    if (in_guard_band(P, mx)) { escalate(P, ray); return; }
    if (!(mx > P.eps)) {
        opacity_cdf(d, s, P.n, P.alpha_net, P.beta_net, cdf);
        __syncthreads();
        emit_final_samples(d, cdf, P.n, u_final + (size_t)ray * P.u_final_stride, P.n_final, d_fine + (size_t)ray * P.n_final);
        if (threadIdx.x == 0) { iter_usage[ray] = 0.f; beta_map[ray] = P.beta_net; }
    } else if (threadIdx.x == 0) {
        beta_plus[ray] = sqrtf((fr * fr) / beta_plus0_denom);           // volsdf.py:149
        act_out[atomicAdd(act_count, 1)] = ray;
    }
}

// Up-sample an active ray: 512 new depths by inverting the CDF of the current error bound
// (sample_pdf(d, bounds, N_up + 2, det=True)[1:-1], volsdf.py:196), sorted.  The inversion of an ascending u over one CDF comes out ascending except
// for last-place effects at bin boundaries and NaN rows: the 45-stage sort runs only for a row that fails lane_row_in_order (sample_cdf.h), or always
// (always_sort: NERFART_UPSAMPLE_SORT=always) - the same bits either way.
// MAXSEG: ray_common.h::scan_maxseg(n).
template <int MAXSEG, bool S_IN_LDS>
__global__ void __launch_bounds__(64)
k_upsample(SamplerParams P, const float* __restrict__ dA, const float* __restrict__ sA,
           const int* __restrict__ act, const float* __restrict__ beta_plus, const float* __restrict__ u_up,
           int clamp_bounds, int always_sort, float* __restrict__ d_new) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int slot = blockIdx.x, ray = act[slot];
    const int n = P.n;
    // LDS: d, cdf, w (n each), out (n_up).  The sdf row is read by the one error-bound scan only and stays in global memory: 3 n + n_up floats
    // instead of 4 n + n_up - the kernel waits on occupancy.  S_IN_LDS: the earlier form, a copy of the row behind `out`.
    float* d = sm; float* cdf = sm + n; float* w = sm + 2 * n; float* out = sm + 3 * n;
    const float* s = sA + (size_t)ray * P.cap;
    load_row(d, dA + (size_t)ray * P.cap, n);
    if constexpr (S_IN_LDS) { float* sl = out + P.n_up; load_row(sl, s, n); s = sl; }
    __syncthreads();
    const float bp = beta_plus[ray];
    error_bound_scan<MAXSEG>(d, s, n, 1.f / bp, bp, w, clamp_bounds != 0);
    __syncthreads();
    // pdf = (w + 1e-5) / sum; cdf = [0, cumsum(pdf)]   (rend_util.py:260-265)
    // (round 6 b, measured and not kept: the bounds, the pdf and the running cdf of a lane's segment in registers instead of three passes over the LDS
    // row w - 264 VGPRs at 16 intervals per lane, spills at 24: one wave per SIMD where this kernel, which waits on dependent binary-search reads, has two)
    const int lane = threadIdx.x;
    const int nint = n - 1, seg = (nint + 63) >> 6, k0 = lane * seg, k1 = (k0 + seg < nint) ? k0 + seg : nint;
    float part = 0.f;
    for (int k = k0; k < k1; ++k) { const float wk = w[k] + 1e-5f; w[k] = wk; part += wk; }
    const float total = wave_sum(part);
    float ps = 0.f;
    for (int k = k0; k < k1; ++k) ps += w[k] / total;
    float run = wave_excl_sum(ps);
    if (lane == 0) cdf[0] = 0.f;
    for (int k = k0; k < k1; ++k) { run += w[k] / total; cdf[k + 1] = run; }
    __syncthreads();
    for (int j = lane; j < P.n_up; j += 64) out[j] = invert_cdf_at(d, cdf, n, u_up[j + 1]);
    __syncthreads();
    if (always_sort || !__all((int)lane_row_in_order(out, P.n_up, lane))) bitonic_sort(out, P.n_up);
    for (int j = lane; j < P.n_up; j += 64) d_new[(size_t)slot * P.n_up + j] = out[j];
}

// What k_merge_check does once the merged rows exist: the bound check at the net's beta, then sampling (converged) or the bisection for beta+.
// MAXSEG > 0: the lane's beta-independent interval constants are loaded once and every scan runs from registers (ray_common.h::SegConsts);
// MAXSEG = 0: every scan through the generic error-bound scan (any row length; NERFART_SCAN_GENERIC builds this form everywhere).
// ROWS_IN_LDS (the earlier form): d, s = the merged rows in LDS, r0 = a third free row of nm floats (the cdf), r1 unused.
// Otherwise d, s = the merged rows in GLOBAL memory (dB / sB, written by this workgroup and fenced) and r0, r1 = the only two LDS rows of nm
// floats, both free: they take a copy of d, s (coalesced; a lane's segment read straight from global memory touches 64 cache lines per load),
// from which the constants are loaded or the generic scans run; the converged path keeps d in r0, puts the cdf in r1 and reads s, twice and in
// order, from global memory.  The same lane owns the same intervals in the same order.
template <int MAXSEG, bool ROWS_IN_LDS>
__device__ __forceinline__ void merge_check_tail(const SamplerParams& P, int ray, const float* d, const float* s, float* r0, float* r1, int nm,
                                                 const float* __restrict__ u_final, float* __restrict__ d_fine, float* __restrict__ beta_plus,
                                                 float* __restrict__ beta_map, float* __restrict__ iter_usage, int* __restrict__ act_out,
                                                 int* __restrict__ act_count) {
    constexpr int NS = MAXSEG > 0 ? MAXSEG : 1;
    const float *dl = d, *sl = s;                                 // the merged rows in LDS
    if constexpr (!ROWS_IN_LDS) { load_row(r0, d, nm); load_row(r1, s, nm); __syncthreads(); dl = r0; sl = r1; }
    SegConsts<NS> C;
    if constexpr (MAXSEG > 0) load_seg_consts<NS>(dl, sl, nm, C);
    auto scan = [&](float alpha, float beta) -> float {
        if constexpr (MAXSEG > 0) return scan_consts<NS>(C, alpha, beta);
        else return error_bound_scan<0>(dl, sl, nm, alpha, beta, nullptr, false);
    };
    const float mx = scan(P.alpha_net, P.beta_net);
    if (in_guard_band(P, mx)) { escalate(P, ray); return; }
    if (!(mx > P.eps)) {
        if constexpr (ROWS_IN_LDS) {
            // cdf = the two depth rows of the merge: dead by now, exactly n + nu = nm floats
            opacity_cdf(d, s, nm, P.alpha_net, P.beta_net, r0);
            __syncthreads();
            emit_final_samples(d, r0, nm, u_final + (size_t)ray * P.u_final_stride, P.n_final, d_fine + (size_t)ray * P.n_final);
        } else {
            __syncthreads();                                      // r0 holds d; nobody reads the copy of s in r1 any more
            opacity_cdf(r0, s, nm, P.alpha_net, P.beta_net, r1);
            __syncthreads();
            emit_final_samples(r0, r1, nm, u_final + (size_t)ray * P.u_final_stride, P.n_final, d_fine + (size_t)ray * P.n_final);
        }
        if (threadIdx.x == 0) { iter_usage[ray] = (float)P.it; beta_map[ray] = P.beta_net; }
    } else {
        float hi = beta_plus[ray], lo = P.beta_net;
        for (int b = 0; b < P.max_bisect; ++b) {
            const float mid = 0.5f * (lo + hi);
            const float m = scan(1.f / mid, mid);
            if (m <= P.eps) hi = mid; else lo = mid;
        }
        if (threadIdx.x == 0) {
            beta_plus[ray] = hi;
            act_out[atomicAdd(act_count, 1)] = ray;
        }
    }
}

// Merge the 512 new (depth, sdf) pairs into the ray's sorted sample set, re-check the bound at the
// net's beta; converged -> 64 fine samples; else bisection for beta+ and re-queue (volsdf.py:211-285).
// One kernel per scan form (MAXSEG: merge_check_tail; merge_check_kernel picks it from the row length): as one kernel with a branch, every round
// ran with the 194 VGPRs of the 24-interval register scan - 2 waves per SIMD, 8 rays per CU, whatever the LDS allowed.
// LDS: the two depth rows (searched by the rank merge) and ONE more row of n + n_up floats: 2 (n + n_up) floats per ray.  The merged (d, s) pairs go
// straight to dB / sB - the next round reads them there anyway - and come back as the scans' copy in the same two rows (merge_check_tail).  The
// sdf values are read once each, from global memory.  ROWS_IN_LDS: the earlier form (NERFART_PERRAY_LDS=ref), the merged rows behind the depth
// rows, 3 (n + n_up) floats: 13 / 8 / 6 rays per CU in rounds 1 / 2 / 3 where the registers allow 16 / 12 / 32.
template <int MAXSEG, bool ROWS_IN_LDS>
__global__ void __launch_bounds__(64)
k_merge_check(SamplerParams P, const float* __restrict__ dA, const float* __restrict__ sA, float* dB, float* sB, const int* __restrict__ act,
              const float* __restrict__ d_new, const float* __restrict__ s_new, const float* __restrict__ u_final, float* __restrict__ d_fine,
              float* __restrict__ beta_plus, float* __restrict__ beta_map, float* __restrict__ iter_usage, int* __restrict__ act_out,
              int* __restrict__ act_count) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int slot = blockIdx.x, ray = act[slot];
    const int n = P.n, nu = P.n_up, nm = n + nu;
    float* d_old = sm; float* dn = sm + n;
    float* row1 = dn + nu;                       // nm floats
    float* dg = dB + (size_t)ray * P.cap; float* sg = sB + (size_t)ray * P.cap;
    float* d = ROWS_IN_LDS ? row1 : dg;          // merged
    float* s = ROWS_IN_LDS ? row1 + nm : sg;
    const float* s_old = sA + (size_t)ray * P.cap;
    const float* sn = s_new + (size_t)slot * nu;
    load_row(d_old, dA + (size_t)ray * P.cap, n);
    load_row(dn, d_new + (size_t)slot * nu, nu);
    __syncthreads();
    // stable merge by rank: old element i goes to i + #{new < d_old[i]}; new element k to k + #{old <= d_new[k]}
    for (int i = threadIdx.x; i < n; i += 64) {
        const int r = i + lower_bound(dn, nu, d_old[i]);
        d[r] = d_old[i]; s[r] = s_old[i];
    }
    for (int k = threadIdx.x; k < nu; k += 64) {
        const int r = k + upper_bound(d_old, n, dn[k]);
        d[r] = dn[k]; s[r] = sn[k];
    }
    if constexpr (!ROWS_IN_LDS) __threadfence_block();            // the merged rows are read back below by other lanes
    __syncthreads();
    if constexpr (ROWS_IN_LDS) {
        for (int i = threadIdx.x; i < nm; i += 64) { dg[i] = d[i]; sg[i] = s[i]; }
    }
    merge_check_tail<MAXSEG, ROWS_IN_LDS>(P, ray, d, s, d_old, row1, nm, u_final, d_fine, beta_plus, beta_map, iter_usage, act_out, act_count);
}

// Rays still active after the last round: sample with the last beta+ (volsdf.py:294-300).
__global__ void __launch_bounds__(64)
k_finalize_unconverged(SamplerParams P, const float* __restrict__ dA, const float* __restrict__ sA,
                       const int* __restrict__ act, const float* __restrict__ u_final,
                       const float* __restrict__ beta_plus, float* __restrict__ d_fine,
                       float* __restrict__ beta_map, float* __restrict__ iter_usage) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int ray = act[blockIdx.x];
    const int n = P.n;
    float* d = sm; float* s = sm + n; float* cdf = sm + 2 * n;
    load_row(d, dA + (size_t)ray * P.cap, n);
    load_row(s, sA + (size_t)ray * P.cap, n);
    __syncthreads();
    const float bp = beta_plus[ray];
    opacity_cdf(d, s, n, 1.f / bp, bp, cdf);
    __syncthreads();
    emit_final_samples(d, cdf, n, u_final + (size_t)ray * P.u_final_stride, P.n_final, d_fine + (size_t)ray * P.n_final);
    if (threadIdx.x == 0) { iter_usage[ray] = -1.f; beta_map[ray] = bp; }
}

// d_all = sort(cat(d_coarse, d_fine))  (volsdf.py:501-502); npad = next power of two >= na + nb
__global__ void __launch_bounds__(64)
k_sort_concat(const float* __restrict__ a, int na, int a_stride, const float* __restrict__ b, int nb, int b_stride,
              int npad, float* __restrict__ out, int out_stride) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int ray = blockIdx.x;
    for (int i = threadIdx.x; i < npad; i += 64) {
        float v = INFINITY;
        if (i < na) v = a[(size_t)ray * a_stride + i];
        else if (i < na + nb) v = b[(size_t)ray * b_stride + (i - na)];
        sm[i] = v;
    }
    bitonic_sort(sm, npad);
    for (int i = threadIdx.x; i < na + nb; i += 64) out[(size_t)ray * out_stride + i] = sm[i];
}

// a16 compositing (volsdf.py:544-576): one wave per ray, P points -> P-1 intervals.
__global__ void __launch_bounds__(64)
k_composite_volsdf(int P, const float* __restrict__ d_all, const float* __restrict__ sdf,
                   const float* __restrict__ radiance, const float* __restrict__ nabla, float alpha, float beta,
                   int white_bkgd, float* __restrict__ rgb, float* __restrict__ depth, float* __restrict__ acc,
                   float* __restrict__ normals, float* __restrict__ sigma_out, float* __restrict__ p_out,
                   float* __restrict__ tau_out) {
    const int ray = blockIdx.x, lane = threadIdx.x;
    const int nint = P - 1;
    const int seg = (nint + 63) >> 6;
    const int k0 = lane * seg, k1 = (k0 + seg < nint) ? k0 + seg : nint;
    const float* dr = d_all + (size_t)ray * P;
    const float* sr = sdf + (size_t)ray * P;
    // pass 1: local product of p_i
    float lp = 1.f;
    for (int k = k0; k < k1; ++k) {
        const float sg = sdf_to_sigma(sr[k], alpha, beta);
        lp *= expf(-fmaxf(sg * (dr[k + 1] - dr[k]), 0.f));
    }
    float T = wave_excl_prod(lp);
    float r = 0.f, g = 0.f, b = 0.f, a = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = k0; k < k1; ++k) {
        const float sg = sdf_to_sigma(sr[k], alpha, beta);
        const float p = expf(-fmaxf(sg * (dr[k + 1] - dr[k]), 0.f));
        const float tau = (1.f - p + 1e-10f) * T;
        const size_t q = (size_t)ray * P + k;
        r += tau * radiance[3 * q]; g += tau * radiance[3 * q + 1]; b += tau * radiance[3 * q + 2];
        a += tau;
        if (normals) {
            const float vx = nabla[3 * q], vy = nabla[3 * q + 1], vz = nabla[3 * q + 2];
            const float nr = fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);     // F.normalize eps
            nx += vx / nr * tau; ny += vy / nr * tau; nz += vz / nr * tau;
        }
        if (sigma_out) sigma_out[q] = sg;
        if (p_out) p_out[(size_t)ray * nint + k] = p;
        if (tau_out) tau_out[(size_t)ray * nint + k] = tau;
        T *= p;
    }
    if (sigma_out && lane == 0) sigma_out[(size_t)ray * P + P - 1] = sdf_to_sigma(sr[P - 1], alpha, beta);
    r = wave_sum(r); g = wave_sum(g); b = wave_sum(b); a = wave_sum(a);
    // depth = sum tau / (sum tau + 1e-10) * d   (second pass needs the total)
    T = wave_excl_prod(lp);
    float dp = 0.f;
    const float inv = a + 1e-10f;
    for (int k = k0; k < k1; ++k) {
        const float sg = sdf_to_sigma(sr[k], alpha, beta);
        const float p = expf(-fmaxf(sg * (dr[k + 1] - dr[k]), 0.f));
        const float tau = (1.f - p + 1e-10f) * T;
        dp += tau / inv * dr[k];
        T *= p;
    }
    dp = wave_sum(dp);
    if (normals) { nx = wave_sum(nx); ny = wave_sum(ny); nz = wave_sum(nz); }
    if (lane == 0) {
        if (white_bkgd) { r += 1.f - a; g += 1.f - a; b += 1.f - a; }
        rgb[3 * (size_t)ray] = r; rgb[3 * (size_t)ray + 1] = g; rgb[3 * (size_t)ray + 2] = b;
        depth[ray] = dp; acc[ray] = a;
        if (normals) { normals[3 * (size_t)ray] = nx; normals[3 * (size_t)ray + 1] = ny; normals[3 * (size_t)ray + 2] = nz; }
    }
}

// ---- escalation of guard-band / never-converged rays (fine_sample_run): compact the listed rays, run Algorithm 1 on them again, scatter --------
__global__ void k_gather_rays(const int* __restrict__ list, int n, const float* __restrict__ rays_o, const float* __restrict__ rays_dn,
                              const float* __restrict__ near, const float* __restrict__ far, const float* __restrict__ u_final, int n_final,
                              float* __restrict__ c_o, float* __restrict__ c_dn, float* __restrict__ c_near, float* __restrict__ c_far,
                              float* __restrict__ c_u) {
    const int slot = blockIdx.x, ray = list[slot], t = threadIdx.x;
    if (slot >= n) return;
    if (t < 3) { c_o[3 * slot + t] = rays_o[3 * (size_t)ray + t]; c_dn[3 * slot + t] = rays_dn[3 * (size_t)ray + t]; }
    if (t == 0 && near) c_near[slot] = near[ray];
    if (t == 0 && far) c_far[slot] = far[ray];
    if (u_final) for (int j = t; j < n_final; j += 64) c_u[(size_t)slot * n_final + j] = u_final[(size_t)ray * n_final + j];
}

__global__ void k_scatter_samples(const int* __restrict__ list, int n, int n_final, const float* __restrict__ c_d_fine,
                                  const float* __restrict__ c_beta, const float* __restrict__ c_iter, float* __restrict__ d_fine,
                                  float* __restrict__ beta_map, float* __restrict__ iter_usage) {
    const int slot = blockIdx.x, ray = list[slot], t = threadIdx.x;
    if (slot >= n) return;
    for (int j = t; j < n_final; j += 64) d_fine[(size_t)ray * n_final + j] = c_d_fine[(size_t)slot * n_final + j];
    if (t == 0) { beta_map[ray] = c_beta[slot]; iter_usage[ray] = c_iter[slot]; }
}

// ---- segment-ordered final stage (final_stage_skipping): the P final samples of a ray in depth segments of SKIP_SEG, front to back; a ray whose
// transmittance has reached exactly 0 in fp32 leaves the live list and the samples behind that point are never evaluated -----------------------
//
// The rule.  x_k = fmaxf(sdf_to_sigma(sdf_k) * (d_{k+1} - d_k), 0) is the optical depth of interval k, the very expression k_composite_volsdf
// exponentiates.  A ray is DEAD FROM SAMPLE s ON when the fp32 running sum of x_k over k < s, added in ascending k, is >= SKIP_THETA.
// Why that makes every tau_k, k >= s, exactly +0 whatever sdf_k, nabla_k and radiance_k are (finite):
//   - k_composite_volsdf forms T_k as a product of p_j = expf(-x_j), j < k: a lane-local product of ceil((P-1)/64) factors, the six levels of
//     wave_excl_prod's shuffle tree, then `T *= p` inside the lane - about 12 multiplications deep for P = 192.  Every factor lies in [0, 1].
//   - fp32 denormals are on: the smallest positive value is 2^-149 = e^-103.28 and a product rounds to 0 once it is below half of that, e^-103.97.
//     A multiplication that lands in the denormal range can round UP, by at most x2 (e^0.69) per level; above it the error is 2^-24 relative.
//     expf's own last-place error in the denormal range is another factor of at most 2.  So a computed T can be non-zero only if the exact
//     product of the factors it contains is at least about e^(-103.97 - 13 * 0.69) = e^-113.
//   - T_k for k >= s contains every factor j < s (and possibly more factors <= 1, which cannot raise it).  Their exact product is
//     exp(-sum x_j), and the fp32 running sum differs from the exact sum by less than 0.01 at this size (P additions, ulp(128) = 1.5e-5).
//   - THETA = 128 therefore leaves more than 14 units of margin over the 113 + 0.01 needed (tests/test_skip_threshold.py emulates the
//     composite's product order over adversarial sequences).
// With T_k = +0, tau_k = (1 - p_k + 1e-10f) * 0 = +0, and adding +0 (or the -0 of a negative nabla component times 0, to a sum that started at
// +0) leaves every accumulator's bits unchanged; the product never recovers.  A NaN sum compares false: the ray stays alive, as before.
// The samples not evaluated are ZERO-FILLED (sdf, nabla, radiance) when the ray is marked, so the composite - untouched - reads finite values
// there whatever the workspace held (a caller may hand in a NaN-filled one: 0 * NaN would poison the pixel).
enum { SKIP_SEG = 32 };
constexpr float SKIP_THETA = 128.0f;

__global__ void k_live_init(int c0, int n, int* __restrict__ live, float* __restrict__ osum) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { live[i] = c0 + i; osum[c0 + i] = 0.f; }
}

// compact depth block [n_live, len] of the segment's samples e0 .. e0 + len - 1 of the listed rays
__global__ void k_gather_segment_depths(const int* __restrict__ live, int n_live, int P, int e0, int len, const float* __restrict__ d_all,
                                        float* __restrict__ c_d) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n_live * len) return;
    const int slot = (int)(i / len), j = (int)(i - (long long)slot * len);
    c_d[i] = d_all[(size_t)live[slot] * P + e0 + j];
}

// After a segment launch: one wave per live ray.  (1) The slot-major compact outputs of segment [e0, e0 + len) go to their [R, P] places.
// (2) advance != 0 (every segment but the last; len <= SKIP_SEG < 64, and e0 + len < P, so d_{k+1} exists): the wave adds x_k, k = e0 .. e0 + len - 1
// (every interval that starts inside the segment), to the ray's running optical depth - lane j computes x_{e0+j} from the sdf value it has just
// placed, the sum itself runs in ascending k as one fp32 chain - and decides the rule above for s = e0 + len.  A ray found dead has its samples
// s .. P - 1 zero-filled.  alive[slot] = 0 / 1 feeds k_compact_live.
__global__ void __launch_bounds__(256)
k_scatter_advance(const int* __restrict__ live, int n_live, int P, int e0, int len, int advance, const float* __restrict__ c_sdf,
                  const float* __restrict__ c_nabla, const float* __restrict__ c_rad, const float* __restrict__ d_all, float alpha, float beta,
                  float* __restrict__ osum, int* __restrict__ alive, float* __restrict__ sdf, float* __restrict__ nabla, float* __restrict__ rad) {
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= n_live) return;                                   // wave-uniform
    const int ray = live[slot];
    const size_t c0 = (size_t)slot * len, q = (size_t)ray * P + e0;
    float sk = 0.f;
    if (lane < len) { sk = c_sdf[c0 + lane]; sdf[q + lane] = sk; }
    for (int i = lane; i < 3 * len; i += 64) { nabla[3 * q + i] = c_nabla[3 * c0 + i]; rad[3 * q + i] = c_rad[3 * c0 + i]; }
    if (!advance) return;
    const float* dr = d_all + (size_t)ray * P;
    float x = 0.f;
    if (lane < len) {
        const int k = e0 + lane;
        x = fmaxf(sdf_to_sigma(sk, alpha, beta) * (dr[k + 1] - dr[k]), 0.f);
    }
    float sum = osum[ray];
    for (int j = 0; j < len; ++j) sum = __fadd_rn(sum, __shfl(x, j, 64));
    const bool dead = sum >= SKIP_THETA;
    if (lane == 0) { osum[ray] = sum; alive[slot] = dead ? 0 : 1; }
    if (dead) {
        const size_t q0 = q + len;
        const int n = P - (e0 + len);
        for (int i = lane; i < n; i += 64) sdf[q0 + i] = 0.f;
        for (int i = lane; i < 3 * n; i += 64) { nabla[3 * q0 + i] = 0.f; rad[3 * q0 + i] = 0.f; }
    }
}

// Stable compaction of the live list (ascending ray order is kept, so a run is reproducible): block b owns slots [1024 b, 1024 b + 1024); its base
// is the number of alive slots before them, counted by the block itself; ranks inside the block by ballot + LDS.  The last block writes the count.
__global__ void __launch_bounds__(1024)
k_compact_live(const int* __restrict__ live, const int* __restrict__ alive, int n_live, int* __restrict__ live_next, int* __restrict__ n_next) {
    __shared__ int wsum[16];
    __shared__ int base_sh;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int first = blockIdx.x * 1024;
    int part = 0;
    for (int i = t; i < first; i += 1024) part += alive[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (lane == 0) wsum[wv] = part;
    __syncthreads();
    if (t == 0) { int b = 0; for (int w = 0; w < 16; ++w) b += wsum[w]; base_sh = b; }
    __syncthreads();
    const int base = base_sh;
    const int slot = first + t;
    const bool keep = slot < n_live && alive[slot] != 0;
    const unsigned long long mask = __ballot(keep);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();                                              // wsum is reused
    if (lane == 0) wsum[wv] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < 16; ++w) { const int c = wsum[w]; if (w < wv) before += c; total += c; }
    if (keep) live_next[base + before + rank] = live[slot];
    if (t == 0 && first + 1024 >= n_live) *n_next = base + total;
}

}  // namespace nerfart

using namespace nerfart;

extern "C" {

// torch.linspace(start, end, n) in fp32: step = (end-start)/(n-1); the first half counts up from
// start, the second half down from end (ATen RangeFactories linspace kernel).  Host helper.
void nerfart_linspace(float start, float end, int n, float* out) {
    if (n == 1) { out[0] = start; return; }
    const float step = (end - start) / (float)(n - 1);
    const int half = n / 2;
    for (int i = 0; i < n; ++i) out[i] = (i < half) ? start + step * (float)i : end - step * (float)(n - i - 1);
}

// ---- stage entry points (also used one by one by the parity tests) --------------------
int nerfart_normalize_dirs(const float* in, float* out, int n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_normalize_dirs, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, in, out, n);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_linspace_depths(const float* t_dev, int n, const float* near, const float* far, float near_s, float far_s,
                            int n_rays, float* out, int stride, void* stream) {
    const long long tot = (long long)n_rays * n;
    if (tot <= 0) return 0;
    hipLaunchKernelGGL(k_linspace_depths, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       t_dev, n, near, far, near_s, far_s, n_rays, out, stride);
    NERFART_HIP(hipGetLastError());
    return 0;
}

// The exported stage entry points take a row stride `cap` from the caller: a row length they could not hold is refused before any HIP call,
// after the empty launch returns 0 as before (the order of neus_render.hip's upsample_step).  The internal calls of fine_sample_run size cap
// themselves and go straight to the *_launch functions.
static int check_rows(const char* who, int n, int cap, int n_extra) {
    char msg[160];
    if (n < 2 || n > cap) snprintf(msg, sizeof(msg), "%s: needs 2 <= n <= cap (n = %d, cap = %d)", who, n, cap);
    else if ((long long)n + n_extra > cap) snprintf(msg, sizeof(msg), "%s: n + n_up = %lld exceeds the row capacity cap = %d", who, (long long)n + n_extra, cap);
    else return 0;
    set_last_error(msg);
    return 2;
}

static const char kLdsRefusal[] = "per-ray kernel needs more than 160 KiB of LDS (too many samples per ray)";

// guard / esc_list / esc_count: see SamplerParams (the exported stage entry point runs with the guard off)
static int first_check_launch(int n_rays, int n, int cap, int n_final, float eps, float alpha_net, float beta_net,
                              const float* dA, const float* sA, const float* u_final, int u_final_stride,
                              float beta_plus0_denom, const float* far, float far_s, float* d_fine, float* beta_plus,
                              float* beta_map, float* iter_usage, int* act_out, int* act_count, float guard, int* esc_list, int* esc_count,
                              void* stream) {
    if (n_rays <= 0) return 0;
    SamplerParams P{n, cap, 0, n_final, 0, 0, eps, alpha_net, beta_net, u_final_stride, guard, esc_list, esc_count};
    const size_t lds = (size_t)3 * n * sizeof(float);
    const int m = scan_maxseg(n);
    auto* const kernel = m == 8 ? k_first_check<8> : m == 16 ? k_first_check<16> : m == 24 ? k_first_check<24> : k_first_check<0>;
    if (int rc = set_lds((const void*)kernel, lds, kLdsRefusal)) return rc;
    hipLaunchKernelGGL(kernel, dim3(n_rays), dim3(64), lds, (hipStream_t)stream, P, dA, sA, u_final,
                       beta_plus0_denom, far, far_s, d_fine, beta_plus, beta_map, iter_usage, act_out, act_count);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_volsdf_first_check(int n_rays, int n, int cap, int n_final, float eps, float alpha_net, float beta_net,
                               const float* dA, const float* sA, const float* u_final, int u_final_stride,
                               float beta_plus0_denom, const float* far, float far_s, float* d_fine, float* beta_plus,
                               float* beta_map, float* iter_usage, int* act_out, int* act_count, void* stream) {
    if (n_rays <= 0) return 0;
    if (int rc = check_rows("volsdf_first_check", n, cap, 0)) return rc;
    return first_check_launch(n_rays, n, cap, n_final, eps, alpha_net, beta_net, dA, sA, u_final, u_final_stride, beta_plus0_denom, far, far_s, d_fine,
                              beta_plus, beta_map, iter_usage, act_out, act_count, 0.f, nullptr, nullptr, stream);
}

// NERFART_PERRAY_LDS=ref: k_upsample and k_merge_check in their earlier form, with the sdf row / the merged rows in LDS (one more row of LDS per ray,
// the same bits).  Read at every call, so that one process can run both (tests/test_gpu_perray_lds.py).
static bool perray_lds_ref() {
    const char* e = std::getenv("NERFART_PERRAY_LDS");
    return e != nullptr && e[0] == 'r';
}

typedef void (*upsample_fn)(SamplerParams, const float*, const float*, const int*, const float*, const float*, int, int, float*);
static upsample_fn upsample_kernel(int maxseg, bool ref) {
    switch (maxseg) {
    case 8: return ref ? k_upsample<8, true> : k_upsample<8, false>;
    case 16: return ref ? k_upsample<16, true> : k_upsample<16, false>;
    case 24: return ref ? k_upsample<24, true> : k_upsample<24, false>;
    default: return ref ? k_upsample<0, true> : k_upsample<0, false>;
    }
}

static int upsample_launch(int n_active, int n, int cap, int n_up, const float* dA, const float* sA, const int* act,
                           const float* beta_plus, const float* u_up, int clamp_bounds, float* d_new, void* stream) {
    if (n_active <= 0) return 0;
    if (n_up & (n_up - 1)) { set_last_error("n_up must be a power of two"); return 2; }
    SamplerParams P{n, cap, n_up, 0, 0, 0, 0.f, 0.f, 0.f};
    const bool ref = perray_lds_ref();
    const size_t lds = ((size_t)(ref ? 4 : 3) * n + n_up) * sizeof(float);
    const upsample_fn kernel = upsample_kernel(scan_maxseg(n), ref);
    if (int rc = set_lds((const void*)kernel, lds, kLdsRefusal)) return rc;
    // NERFART_UPSAMPLE_SORT=always sorts every row; read at every call, so that one process can run both (tests/test_gpu_upsample_sorted.py)
    const char* e = std::getenv("NERFART_UPSAMPLE_SORT");
    const int always_sort = (e != nullptr && e[0] == 'a') ? 1 : 0;
    hipLaunchKernelGGL(kernel, dim3(n_active), dim3(64), lds, (hipStream_t)stream, P, dA, sA, act, beta_plus, u_up,
                       clamp_bounds, always_sort, d_new);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_volsdf_upsample(int n_active, int n, int cap, int n_up, const float* dA, const float* sA, const int* act,
                            const float* beta_plus, const float* u_up, int clamp_bounds, float* d_new, void* stream) {
    if (n_active <= 0) return 0;
    if (int rc = check_rows("volsdf_upsample", n, cap, 0)) return rc;
    return upsample_launch(n_active, n, cap, n_up, dA, sA, act, beta_plus, u_up, clamp_bounds, d_new, stream);
}

typedef void (*merge_check_fn)(SamplerParams, const float*, const float*, float*, float*, const int*, const float*, const float*, const float*, float*,
                               float*, float*, float*, int*, int*);
// rounds 1 and 2 (1,024 / 1,536 merged samples: every undecided ray of a frame / 78 % of them): the check and the 10 bisection scans from registers
static merge_check_fn merge_check_kernel(int nm, bool ref) {
    const int m = scan_maxseg(nm);
    if (m == 8 || m == 16) return ref ? k_merge_check<16, true> : k_merge_check<16, false>;
    if (m == 24) return ref ? k_merge_check<24, true> : k_merge_check<24, false>;
    return ref ? k_merge_check<0, true> : k_merge_check<0, false>;
}

static int merge_check_launch(int n_active, int n, int cap, int n_up, int n_final, int max_bisect, int it, float eps,
                              float alpha_net, float beta_net, const float* dA, const float* sA, float* dB, float* sB,
                              const int* act, const float* d_new, const float* s_new, const float* u_final,
                              int u_final_stride, float* d_fine, float* beta_plus, float* beta_map, float* iter_usage,
                              int* act_out, int* act_count, float guard, int* esc_list, int* esc_count, void* stream) {
    if (n_active <= 0) return 0;
    SamplerParams P{n, cap, n_up, n_final, max_bisect, it, eps, alpha_net, beta_net, u_final_stride, guard, esc_list, esc_count};
    const bool ref = perray_lds_ref();
    const merge_check_fn kernel = merge_check_kernel(n + n_up, ref);
    const size_t lds = (size_t)(ref ? 3 : 2) * ((size_t)n + n_up) * sizeof(float);
    if (int rc = set_lds((const void*)kernel, lds, kLdsRefusal)) return rc;
    hipLaunchKernelGGL(kernel, dim3(n_active), dim3(64), lds, (hipStream_t)stream, P, dA, sA, dB, sB, act, d_new,
                       s_new, u_final, d_fine, beta_plus, beta_map, iter_usage, act_out, act_count);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_volsdf_merge_check(int n_active, int n, int cap, int n_up, int n_final, int max_bisect, int it, float eps,
                               float alpha_net, float beta_net, const float* dA, const float* sA, float* dB, float* sB,
                               const int* act, const float* d_new, const float* s_new, const float* u_final,
                               int u_final_stride, float* d_fine, float* beta_plus, float* beta_map, float* iter_usage,
                               int* act_out, int* act_count, void* stream) {
    if (n_active <= 0) return 0;
    if (int rc = check_rows("volsdf_merge_check", n, cap, n_up)) return rc;
    return merge_check_launch(n_active, n, cap, n_up, n_final, max_bisect, it, eps, alpha_net, beta_net, dA, sA, dB, sB, act, d_new, s_new, u_final,
                              u_final_stride, d_fine, beta_plus, beta_map, iter_usage, act_out, act_count, 0.f, nullptr, nullptr, stream);
}

static int finalize_launch(int n_active, int n, int cap, int n_final, const float* dA, const float* sA, const int* act,
                           const float* u_final, int u_final_stride, const float* beta_plus, float* d_fine,
                           float* beta_map, float* iter_usage, void* stream) {
    if (n_active <= 0) return 0;
    SamplerParams P{n, cap, 0, n_final, 0, 0, 0.f, 0.f, 0.f, u_final_stride};
    const size_t lds = (size_t)3 * n * sizeof(float);
    if (int rc = set_lds((const void*)k_finalize_unconverged, lds, kLdsRefusal)) return rc;
    hipLaunchKernelGGL(k_finalize_unconverged, dim3(n_active), dim3(64), lds, (hipStream_t)stream, P, dA, sA, act,
                       u_final, beta_plus, d_fine, beta_map, iter_usage);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_volsdf_finalize(int n_active, int n, int cap, int n_final, const float* dA, const float* sA, const int* act,
                            const float* u_final, int u_final_stride, const float* beta_plus, float* d_fine,
                            float* beta_map, float* iter_usage, void* stream) {
    if (n_active <= 0) return 0;
    if (int rc = check_rows("volsdf_finalize", n, cap, 0)) return rc;
    return finalize_launch(n_active, n, cap, n_final, dA, sA, act, u_final, u_final_stride, beta_plus, d_fine, beta_map, iter_usage, stream);
}

int nerfart_sort_concat(int n_rays, const float* a, int na, int a_stride, const float* b, int nb, int b_stride,
                        float* out, int out_stride, void* stream) {
    if (n_rays <= 0) return 0;
    const int npad = next_pow2(na + nb);
    const size_t lds = (size_t)npad * sizeof(float);
    if (int rc = set_lds((const void*)k_sort_concat, lds, kLdsRefusal)) return rc;
    hipLaunchKernelGGL(k_sort_concat, dim3(n_rays), dim3(64), lds, (hipStream_t)stream, a, na, a_stride, b, nb, b_stride,
                       npad, out, out_stride);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_volsdf_composite(int n_rays, int P, const float* d_all, const float* sdf, const float* radiance,
                             const float* nabla, float alpha, float beta, int white_bkgd, float* rgb, float* depth,
                             float* acc, float* normals, float* sigma_out, float* p_out, float* tau_out, void* stream) {
    if (n_rays <= 0) return 0;
    if (P < 2) { set_last_error("volsdf_composite: needs P >= 2 samples per ray (P - 1 intervals)"); return 2; }
    if (normals && !nabla) { set_last_error("composite: normals requested without nablas"); return 2; }
    hipLaunchKernelGGL(k_composite_volsdf, dim3(n_rays), dim3(64), 0, (hipStream_t)stream, P, d_all, sdf, radiance, nabla,
                       alpha, beta, white_bkgd, rgb, depth, acc, normals, sigma_out, p_out, tau_out);
    NERFART_HIP(hipGetLastError());
    return 0;
}

// ---- fine_sample (Algorithm 1) on the device --------------------------------------------
// Workspace (caller-allocated, device): see nerfart_volsdf_sampler_workspace_bytes.
typedef struct {
    float *dA, *sA, *dB, *sB, *d_new, *s_new, *beta_plus;
    int *act0, *act1, *count;
    float *t_init, *u_up, *u_final;
    // escalation (behind everything a run on <= n_rays rays carves, so the second run may reuse the front of the same workspace)
    int* esc_list;
    float *c_o, *c_dn, *c_near, *c_far, *c_u, *c_d_fine, *c_beta, *c_iter;
} sampler_ws_t;

enum { COUNT_SLOTS = 64, ESC_SLOT = COUNT_SLOTS - 1 };     // w.count: one active-ray counter per round + the escalation list's length

static sampler_ws_t carve_sampler(Carver& c, int R, int cap, int n_up, int n0, int n_final) {
    sampler_ws_t w;
    const size_t row = (size_t)R * cap;
    w.dA = c.take<float>(row);
    w.sA = c.take<float>(row);
    w.dB = c.take<float>(row);
    w.sB = c.take<float>(row);
    w.d_new = c.take<float>((size_t)R * n_up);
    w.s_new = c.take<float>((size_t)R * n_up);
    w.beta_plus = c.take<float>((size_t)R);
    w.act0 = c.take<int>((size_t)R);
    w.act1 = c.take<int>((size_t)R);
    w.count = c.take<int>(COUNT_SLOTS);
    w.t_init = c.take<float>((size_t)n0);
    w.u_up = c.take<float>((size_t)(n_up + 2));
    w.u_final = c.take<float>((size_t)n_final);
    w.esc_list = c.take<int>((size_t)R);
    w.c_o = c.take<float>((size_t)R * 3);
    w.c_dn = c.take<float>((size_t)R * 3);
    w.c_near = c.take<float>((size_t)R);
    w.c_far = c.take<float>((size_t)R);
    w.c_u = c.take<float>((size_t)R * n_final);
    w.c_d_fine = c.take<float>((size_t)R * n_final);
    w.c_beta = c.take<float>((size_t)R);
    w.c_iter = c.take<float>((size_t)R);
    return w;
}

static size_t sampler_bytes(int R, int cap, int n_up, int n0, int n_final) {
    Carver c(nullptr);
    carve_sampler(c, R, cap, n_up, n0, n_final);
    return c.off;
}

long long nerfart_volsdf_sampler_workspace_bytes(int n_rays, int n_init, int n_up, int n_final, int max_iter) {
    return (long long)sampler_bytes(n_rays, n_init + max_iter * n_up, n_up, n_init, n_final);
}

// fine_sample (volsdf.py:97-302) for n_rays rays with already normalised directions.
//   near/far: per-ray device arrays or nullptr + scalars.  Outputs: d_fine [R, n_final],
//   beta_map [R], iter_usage [R] (float: 0..max_iter, -1 = never converged).
// GUARDED form (esc_blob != nullptr && guard > 0; nerfart_volsdf_fine_sample_guarded): the SDF queries run on (surf_blob, precision) - the cheap
// arithmetic - but every ray whose outcome hangs on a marginal threshold decision is sampled AGAIN, from its first query on, on (esc_blob,
// esc_precision):  (i) a ray whose max B lies within guard * eps of eps at a convergence check (volsdf.py:162-163, :240-242) stops there;
// (ii) a ray still active after the last round (volsdf.py:294-300: sampled with its last bisected beta+, the rays any change of rounding moves).
// (iii) late_round > 0 (ABI 5): a ray still active after round `late_round` - from there on every further round starts from a 10-step bisection for
// beta+ whose threshold decisions (volsdf.py:266-275) feed the next round's sampling density: the branch-sensitive rays of Algorithm 1, 3.6 % of a
// frame at late_round = 3 - is escalated there instead of being carried through the remaining rounds on the cheap arithmetic.
// Rays are independent, so the escalated rays' samples are bit-identical to a run of the whole batch on esc_blob.
static int fine_sample_run(const float* surf_blob, int precision, const float* esc_blob, int esc_precision, float guard, int late_round,
                           const float* rays_o, const float* rays_dn, int n_rays,
                           const float* near, const float* far, float near_s, float far_s, float R_bg,
                           float alpha_net, float beta_net, float eps, int n_init, int n_up, int n_final,
                           int max_iter, int max_bisect, const float* t_init_dev, const float* u_up_dev,
                           const float* u_final_dev, int u_final_per_ray, float* d_fine, float* beta_map,
                           float* iter_usage, void* workspace, long long workspace_bytes, int* n_escalated, hipStream_t stream) {
    if (n_escalated) *n_escalated = 0;
    if (n_rays <= 0) return 0;
    if (u_final_per_ray && !u_final_dev) { set_last_error("fine_sample: u_final_per_ray needs u_final_dev [n_rays, n_final]"); return 2; }
    if (max_iter < 0 || max_iter >= ESC_SLOT) { set_last_error("fine_sample: max_iter must be in [0, 62]"); return 2; }
    const bool guarded = esc_blob != nullptr && guard > 0.f;
    if (!guarded) guard = 0.f;
    const int u_stride = u_final_per_ray ? n_final : 0;
    const int cap = n_init + max_iter * n_up;
    Carver carver(workspace);
    sampler_ws_t w = carve_sampler(carver, n_rays, cap, n_up, n_init, n_final);
    if (!workspace || (size_t)workspace_bytes < carver.off) { set_last_error("fine_sample: workspace too small"); return 2; }
    // linspace tables: torch.linspace(0, 1, n) for n = n_init, n_up + 2, n_final.  Callers that hold the
    // host framework's own tables pass them (torch's CPU kernel is vectorised and differs from the scalar
    // formula by an ulp on some entries); otherwise the library's nerfart_linspace is used.
    const bool own_tables = !(t_init_dev && u_up_dev && u_final_dev);
    if (!own_tables) {
        w.t_init = const_cast<float*>(t_init_dev); w.u_up = const_cast<float*>(u_up_dev); w.u_final = const_cast<float*>(u_final_dev);
    } else {
        if (int rc = upload_linspace_tables({{w.t_init, n_init}, {w.u_up, n_up + 2}, {w.u_final, n_final}}, stream)) return rc;
        if (u_final_per_ray) w.u_final = const_cast<float*>(u_final_dev);
    }
    if (int rc = nerfart_linspace_depths(w.t_init, n_init, near, far, near_s, far_s, n_rays, w.dA, cap, stream)) return rc;
    if (int rc = nerfart_sdf_fwd_rays(surf_blob, precision, rays_o, rays_dn, nullptr, w.dA, n_rays, n_init, cap, R_bg, w.sA, cap, stream)) return rc;
    NERFART_HIP(hipMemsetAsync(w.count, 0, COUNT_SLOTS * sizeof(int), stream));
    const float denom = (float)(4.0 * (double)(n_init - 1) * log(1.0 + (double)eps));     // volsdf.py:149
    if (int rc = first_check_launch(n_rays, n_init, cap, n_final, eps, alpha_net, beta_net, w.dA, w.sA, w.u_final,
                                    u_stride, denom, far, far_s, d_fine, w.beta_plus, beta_map, iter_usage, w.act0,
                                    w.count, guard, w.esc_list, w.count + ESC_SLOT, stream)) return rc;
    // one read of the counter block per round (the active count of the round + the escalation list's length so far): the only host synchronisation
    int h_count[COUNT_SLOTS];
    NERFART_HIP(hipMemcpyAsync(h_count, w.count, sizeof(h_count), hipMemcpyDeviceToHost, stream));
    NERFART_HIP(hipStreamSynchronize(stream));
    int n_act = h_count[0];
    float *dA = w.dA, *sA = w.sA, *dB = w.dB, *sB = w.sB;
    int *act = w.act0, *act_next = w.act1;
    int n = n_init;
    for (int it = 1; it <= max_iter && n_act > 0; ++it) {
        if (int rc = upsample_launch(n_act, n, cap, n_up, dA, sA, act, w.beta_plus, w.u_up, it > 1, w.d_new, stream)) return rc;
        if (int rc = nerfart_sdf_fwd_rays(surf_blob, precision, rays_o, rays_dn, act, w.d_new, n_act, n_up, n_up, R_bg, w.s_new, n_up, stream)) return rc;
        // a guarded run escalates every ray still active after its last round (late_round, or max_iter): their beta+ is never read again (the
        // second run starts from its own first check), so that round's rays skip the bisection
        const bool last_round = guarded && (it == max_iter || (late_round > 0 && it >= late_round));
        if (int rc = merge_check_launch(n_act, n, cap, n_up, n_final, last_round ? 0 : max_bisect, it, eps, alpha_net, beta_net, dA, sA,
                                        dB, sB, act, w.d_new, w.s_new, w.u_final, u_stride, d_fine, w.beta_plus,
                                        beta_map, iter_usage, act_next, w.count + it, guard, w.esc_list, w.count + ESC_SLOT, stream)) return rc;
        NERFART_HIP(hipMemcpyAsync(h_count, w.count, sizeof(h_count), hipMemcpyDeviceToHost, stream));
        NERFART_HIP(hipStreamSynchronize(stream));
        n_act = h_count[it];
        float* t;
        t = dA; dA = dB; dB = t;
        t = sA; sA = sB; sB = t;
        int* ti = act; act = act_next; act_next = ti;
        n += n_up;
        if (last_round) break;                                          // the rays still active go to the escalation list below
    }
    if (!guarded) {
        if (n_act > 0)
            if (int rc = finalize_launch(n_act, n, cap, n_final, dA, sA, act, w.u_final, u_stride, w.beta_plus, d_fine,
                                         beta_map, iter_usage, stream)) return rc;
        return 0;
    }
    // ---- escalation: the guard-band rays listed so far + the rays that never converged -> Algorithm 1 again, on the escalation blob ----
    int n_esc = h_count[ESC_SLOT];
    if (n_act > 0) {
        NERFART_HIP(hipMemcpyAsync(w.esc_list + n_esc, act, sizeof(int) * (size_t)n_act, hipMemcpyDeviceToDevice, stream));
        n_esc += n_act;
    }
    if (n_escalated) *n_escalated = n_esc;
    if (n_esc == 0) return 0;
    hipLaunchKernelGGL(k_gather_rays, dim3(n_esc), dim3(64), 0, stream, w.esc_list, n_esc, rays_o, rays_dn, near, far,
                       u_final_per_ray ? u_final_dev : (const float*)nullptr, n_final, w.c_o, w.c_dn, w.c_near, w.c_far, w.c_u);
    NERFART_HIP(hipGetLastError());
    // the second run carves the FRONT of this workspace (its n_esc <= n_rays rays need no more than this run's, whose contents are dead); the
    // compacted rays, their outputs and the list sit behind it.  Tables the library built itself sit in the front too: the second run rebuilds them.
    const float* u2 = u_final_per_ray ? w.c_u : (own_tables ? nullptr : u_final_dev);
    const int* esc_list = w.esc_list;
    float *c_d_fine = w.c_d_fine, *c_beta = w.c_beta, *c_iter = w.c_iter;
    profile_class0_as(4);                     // launch profiling: the escalation run's SDF queries are their own class (nerfart_profile_end5)
    const int rc_esc = fine_sample_run(esc_blob, esc_precision, nullptr, 0, 0.f, 0, w.c_o, w.c_dn, n_esc, near ? w.c_near : nullptr, far ? w.c_far : nullptr,
                                       near_s, far_s, R_bg, alpha_net, beta_net, eps, n_init, n_up, n_final, max_iter, max_bisect,
                                       own_tables ? nullptr : t_init_dev, own_tables ? nullptr : u_up_dev, u2, u_final_per_ray, c_d_fine, c_beta, c_iter,
                                       workspace, workspace_bytes, nullptr, stream);
    profile_class0_as(0);
    if (rc_esc) return rc_esc;
    hipLaunchKernelGGL(k_scatter_samples, dim3(n_esc), dim3(64), 0, stream, esc_list, n_esc, n_final, c_d_fine, c_beta, c_iter, d_fine, beta_map,
                       iter_usage);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_volsdf_fine_sample(const float* surf_blob, int precision, const float* rays_o, const float* rays_dn, int n_rays,
                               const float* near, const float* far, float near_s, float far_s, float R_bg,
                               float alpha_net, float beta_net, float eps, int n_init, int n_up, int n_final,
                               int max_iter, int max_bisect, const float* t_init_dev, const float* u_up_dev,
                               const float* u_final_dev, int u_final_per_ray, float* d_fine, float* beta_map,
                               float* iter_usage, void* workspace, long long workspace_bytes, void* stream) {
    return fine_sample_run(surf_blob, precision, nullptr, 0, 0.f, 0, rays_o, rays_dn, n_rays, near, far, near_s, far_s, R_bg, alpha_net, beta_net, eps, n_init,
                           n_up, n_final, max_iter, max_bisect, t_init_dev, u_up_dev, u_final_dev, u_final_per_ray, d_fine, beta_map, iter_usage, workspace,
                           workspace_bytes, nullptr, (hipStream_t)stream);
}

int nerfart_volsdf_fine_sample_guarded2(const float* surf_blob, int precision, const float* esc_blob, int esc_precision, float guard, int late_round,
                                       const float* rays_o, const float* rays_dn, int n_rays,
                                       const float* near, const float* far, float near_s, float far_s, float R_bg,
                                       float alpha_net, float beta_net, float eps, int n_init, int n_up, int n_final,
                                       int max_iter, int max_bisect, const float* t_init_dev, const float* u_up_dev,
                                       const float* u_final_dev, int u_final_per_ray, float* d_fine, float* beta_map,
                                       float* iter_usage, int* n_escalated, void* workspace, long long workspace_bytes, void* stream) {
    return fine_sample_run(surf_blob, precision, esc_blob, esc_precision, guard, late_round, rays_o, rays_dn, n_rays, near, far, near_s, far_s, R_bg, alpha_net, beta_net, eps,
                           n_init, n_up, n_final, max_iter, max_bisect, t_init_dev, u_up_dev, u_final_dev, u_final_per_ray, d_fine, beta_map, iter_usage,
                           workspace, workspace_bytes, n_escalated, (hipStream_t)stream);
}

int nerfart_volsdf_fine_sample_guarded(const float* surf_blob, int precision, const float* esc_blob, int esc_precision, float guard,
                                       const float* rays_o, const float* rays_dn, int n_rays,
                                       const float* near, const float* far, float near_s, float far_s, float R_bg,
                                       float alpha_net, float beta_net, float eps, int n_init, int n_up, int n_final,
                                       int max_iter, int max_bisect, const float* t_init_dev, const float* u_up_dev,
                                       const float* u_final_dev, int u_final_per_ray, float* d_fine, float* beta_map,
                                       float* iter_usage, int* n_escalated, void* workspace, long long workspace_bytes, void* stream) {
    return nerfart_volsdf_fine_sample_guarded2(surf_blob, precision, esc_blob, esc_precision, guard, 0, rays_o, rays_dn, n_rays, near, far, near_s, far_s, R_bg,
                                               alpha_net, beta_net, eps, n_init, n_up, n_final, max_iter, max_bisect, t_init_dev, u_up_dev, u_final_dev,
                                               u_final_per_ray, d_fine, beta_map, iter_usage, n_escalated, workspace, workspace_bytes, stream);
}

// ---- whole-chunk VolSDF render (boundary B1: render_fn / volume_render, volsdf.py:389-615) ----
typedef struct {
    float *rays_dn, *d_fine, *d_coarse, *t_coarse, *d_all, *sdf, *nabla, *rad, *beta_map, *iter_usage, *h7;
    char* sampler;
    size_t sampler_bytes;
    char* nabla_ws;           // softplus' scratch of the reverse-mode grad(SDF) kernel (nerfart_sdf_nabla_workspace_bytes)
    size_t nabla_ws_bytes;
} render_ws_t;

// Buffers of the segment-ordered final stage (final_stage_skipping): the live lists of a ray group, alive flags, the live count, the per-ray running
// optical depths, the compact depth / sdf / nabla / radiance blocks of one segment launch and - own_h7 - that launch's h7 rows.  They are carved
// out of the SAMPLER's region of the render workspace: Algorithm 1 has finished by then and its rows (16 bytes x 512 (1 + rounds) per ray) are
// dead, so the workspace does not grow.
typedef struct {
    int *live0, *live1, *alive, *n_live;
    float *osum, *c_depth, *c_sdf, *c_nabla, *c_rad, *h7;
} skip_ws_t;

static skip_ws_t carve_skip(Carver& c, int R, int P, int G, bool own_h7) {
    skip_ws_t k;
    const size_t gpts = (size_t)G * (P < SKIP_SEG ? P : SKIP_SEG);
    k.live0 = c.take<int>((size_t)G);
    k.live1 = c.take<int>((size_t)G);
    k.alive = c.take<int>((size_t)G);
    k.n_live = c.take<int>(1);
    k.osum = c.take<float>((size_t)R);
    k.c_depth = c.take<float>(gpts);
    k.c_sdf = c.take<float>(gpts);
    k.c_nabla = c.take<float>(gpts * 3);
    k.c_rad = c.take<float>(gpts * 3);
    k.h7 = own_h7 ? c.take<float>(gpts * 256) : nullptr;
    return k;
}

// Rays per group.  The groups exist only because a segment launch needs 1 KiB of h7 per point, and every launch of the two MLP kernels pays its own
// fill, drain and tile quantisation, every segment of every group a host read: so ONE group of all R rays where the segment's h7 rows
// (R min(SKIP_SEG, P) x 1 KiB; P = 192, 5 rounds: 33 KiB of the 48 KiB per ray) fit the sampler's dead region beside the buffers above (own_h7) -
// halved while they do not.  Below G = min(k3_rays, R) P / min(SKIP_SEG, P) rays (P = 192: 6 k3_rays) the render workspace's own h7 carve holds
// a segment launch as it is, and the group is halved only until the small buffers fit (with one ray per group they always do: the sampler holds
// several [R] arrays itself).  The workspace's size is what it was.
static int skip_group_rays(int R, int P, int k3_rays, size_t room, bool* own_h7) {
    const long long rk = k3_rays < R ? k3_rays : R;
    long long g_shared = rk * P / (P < SKIP_SEG ? P : SKIP_SEG);
    if (g_shared > R) g_shared = R;
    const auto fits = [&](long long g, bool own) {
        Carver c(nullptr);
        carve_skip(c, R, P, (int)g, own);
        return c.off <= room;
    };
    *own_h7 = true;
    for (long long g = R; g > g_shared; g /= 2)
        if (fits(g, true)) return (int)g;
    *own_h7 = false;
    long long g = g_shared;
    for (; g > 1 && !fits(g, false); g /= 2) {}
    return (int)g;
}

static render_ws_t carve_render(Carver& c, int R, int n_samples, int n_imp, int max_iter, int k3_rays) {
    render_ws_t w;
    const int P = n_samples + n_imp;
    const int n_init = 4 * n_samples, n_up = 4 * n_samples;
    w.rays_dn = c.take<float>((size_t)R * 3);
    w.d_fine = c.take<float>((size_t)R * n_imp);
    w.d_coarse = c.take<float>((size_t)R * n_samples);
    w.t_coarse = c.take<float>((size_t)n_samples);
    w.d_all = c.take<float>((size_t)R * P);
    w.sdf = c.take<float>((size_t)R * P);
    w.nabla = c.take<float>((size_t)R * P * 3);
    w.rad = c.take<float>((size_t)R * P * 3);
    w.beta_map = c.take<float>((size_t)R);
    w.iter_usage = c.take<float>((size_t)R);
    const int rk = k3_rays < R ? k3_rays : R;
    w.h7 = c.take<float>((size_t)rk * P * 256);
    w.sampler_bytes = sampler_bytes(R, n_init + max_iter * n_up, n_up, n_init, n_imp);
    w.sampler = c.take<char>(w.sampler_bytes);
    const long long nb0 = nerfart_sdf_nabla_workspace_bytes(0), nb1 = nerfart_sdf_nabla_workspace_bytes(1);
    w.nabla_ws_bytes = (size_t)(nb0 > nb1 ? nb0 : nb1);         // sized for either precision
    w.nabla_ws = c.take<char>(w.nabla_ws_bytes);
    return w;
}

long long nerfart_volsdf_render_workspace_bytes(int n_rays, int n_samples, int n_importance, int max_upsample_steps,
                                                int k3_rays_chunk) {
    Carver c(nullptr);
    carve_render(c, n_rays, n_samples, n_importance, max_upsample_steps, k3_rays_chunk);
    return (long long)c.off;
}

// The final samples of every ray WITHOUT the ones behind full opacity (the rule and its derivation: next to SKIP_THETA).  Rays in groups
// (skip_group_rays: one group of all the rays where the workspace allows); per group the depth segments front to back: gather the live rays'
// depths of the segment, sdf + nabla and radiance on the live list (slot-major compact outputs), then one launch scatters them to [R, P],
// advances the running optical depths, marks and zero-fills the dead, and the list is compacted (stable: ascending ray order).  The live count
// reaches the host with ONE 4-byte read per segment per group (as the sampler's rounds do); no live ray left ends the group; there are no
// zero-size launches.  Every stored value of an evaluated sample is what the plain loop stores.
static int final_stage_skipping(const render_ws_t& w, const float* surf_blob, int precision, const float* rad_blob, int rad_precision, int view_tiles,
                                const float* rays_o, int n_rays, int P, float R_bg, float alpha, float beta, const float* d_all, float* sdf,
                                float* nabla, float* rad, int k3_rays, hipStream_t stream) {
    bool own_h7 = false;
    const int G = skip_group_rays(n_rays, P, k3_rays, w.sampler_bytes, &own_h7);
    Carver carver(w.sampler);
    const skip_ws_t k = carve_skip(carver, n_rays, P, G, own_h7);
    if (carver.off > w.sampler_bytes) { set_last_error("render: workspace too small"); return 2; }
    float* h7 = own_h7 ? k.h7 : w.h7;
    int *live = k.live0, *live_next = k.live1;
    for (int c0 = 0; c0 < n_rays; c0 += G) {
        int n_live = (n_rays - c0 < G) ? n_rays - c0 : G;
        hipLaunchKernelGGL(k_live_init, dim3((n_live + 255) / 256), dim3(256), 0, stream, c0, n_live, live, k.osum);
        NERFART_HIP(hipGetLastError());
        for (int e0 = 0; e0 < P && n_live > 0; e0 += SKIP_SEG) {
            const int len = (P - e0 < SKIP_SEG) ? P - e0 : SKIP_SEG;
            const unsigned nb = (unsigned)(((long long)n_live * len + 255) / 256);
            hipLaunchKernelGGL(k_gather_segment_depths, dim3(nb), dim3(256), 0, stream, live, n_live, P, e0, len, d_all, k.c_depth);
            NERFART_HIP(hipGetLastError());
            if (int rc = nerfart_sdf_nabla_fwd_rays(surf_blob, precision, rays_o, w.rays_dn, live, k.c_depth, n_live, len, len, R_bg, k.c_sdf, k.c_nabla,
                                                    h7, w.nabla_ws, (long long)w.nabla_ws_bytes, stream)) return rc;
            if (int rc = nerfart_radiance_fwd_rays(rad_blob, rad_precision, view_tiles, rays_o, w.rays_dn, live, k.c_depth, n_live, len, len, k.c_nabla,
                                                   h7, k.c_rad, stream)) return rc;
            const bool last = e0 + len >= P;                          // the last segment: nothing behind it to skip
            hipLaunchKernelGGL(k_scatter_advance, dim3((n_live + 3) / 4), dim3(256), 0, stream, live, n_live, P, e0, len, last ? 0 : 1, k.c_sdf, k.c_nabla,
                               k.c_rad, d_all, alpha, beta, k.osum, k.alive, sdf, nabla, rad);
            NERFART_HIP(hipGetLastError());
            if (last) break;
            hipLaunchKernelGGL(k_compact_live, dim3((n_live + 1023) / 1024), dim3(1024), 0, stream, live, k.alive, n_live, live_next, k.n_live);
            NERFART_HIP(hipGetLastError());
            NERFART_HIP(hipMemcpyAsync(&n_live, k.n_live, sizeof(int), hipMemcpyDeviceToHost, stream));
            NERFART_HIP(hipStreamSynchronize(stream));
            int* t = live; live = live_next; live_next = t;
        }
    }
    return 0;
}

// Renders n_rays rays (rays_d un-normalised, as get_rays returns them).  Outputs rgb [R,3], depth [R],
// acc [R] always; every other output pointer may be null:  normals [R,3]; detailed per-sample
// arrays d_all/sdf/sigma [R,P], nabla/radiance [R,P,3], p_i/tau [R,P-1]; beta_map/iter_usage [R].
// Every stage on its own blob / precision (nerfart_volsdf_render_staged_fwd):
//   sampler_blob / sampler_precision: Algorithm 1's SDF queries (the no-gradient sampling stage, volsdf.py:479), with sampler_guard > 0: guarded -
//     rays whose convergence decision is marginal or that never converge are sampled again on (surf_blob, precision) (fine_sample_run);
//   surf_blob / precision: sdf + nabla of the 192 final samples;   rad_blob / rad_precision: the radiance net there;   compositing: fp32.
// nerfart_volsdf_render_mixed_fwd = this with rad_precision = precision and the guard off; nerfart_volsdf_render_fwd passes the same blob and
// precision everywhere.
int nerfart_volsdf_render_staged2_fwd(const float* surf_blob, int precision, const float* rad_blob, int rad_precision, const float* sampler_blob,
                                     int sampler_precision, float sampler_guard, int sampler_late_round, int view_tiles, const float* rays_o,
                              const float* rays_d, int n_rays, float near_s, float far_s, float R_bg, float alpha,
                              float beta, float eps, int n_samples, int n_importance, int max_upsample_steps,
                              int max_bisection_steps, int white_bkgd, int k3_rays_chunk, const float* t_coarse_dev,
                              const float* t_init_dev, const float* u_up_dev, const float* u_final_dev, int u_final_per_ray,
                              float* rgb, float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out, float* nabla_out,
                              float* radiance_out, float* sigma_out, float* p_out, float* tau_out, float* beta_map_out,
                              float* iter_usage_out, int* n_escalated, void* workspace, long long workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rays <= 0) return 0;
    if (!sampler_blob) { set_last_error("render: sampler_blob is NULL"); return 2; }
    if (n_samples < 2 || n_importance < 1 || k3_rays_chunk < 1) { set_last_error("render: bad sample counts"); return 2; }
    const int P = n_samples + n_importance;
    Carver carver(workspace);
    render_ws_t w = carve_render(carver, n_rays, n_samples, n_importance, max_upsample_steps, k3_rays_chunk);
    if (!workspace || (size_t)workspace_bytes < carver.off) { set_last_error("render: workspace too small"); return 2; }
    float* d_all = d_all_out ? d_all_out : w.d_all;
    float* sdf = sdf_out ? sdf_out : w.sdf;
    float* nabla = nabla_out ? nabla_out : w.nabla;
    float* rad = radiance_out ? radiance_out : w.rad;
    float* beta_map = beta_map_out ? beta_map_out : w.beta_map;
    float* iter_usage = iter_usage_out ? iter_usage_out : w.iter_usage;

    if (int rc = nerfart_normalize_dirs(rays_d, w.rays_dn, n_rays, stream)) return rc;
    const bool guarded = sampler_guard > 0.f && (sampler_blob != surf_blob || sampler_precision != precision);
    if (int rc = fine_sample_run(sampler_blob, sampler_precision, guarded ? surf_blob : nullptr, precision, sampler_guard, sampler_late_round, rays_o, w.rays_dn, n_rays,
                                 nullptr, nullptr, near_s, far_s, R_bg, alpha, beta, eps, 4 * n_samples, 4 * n_samples, n_importance,
                                 max_upsample_steps, max_bisection_steps, t_init_dev, u_up_dev, u_final_dev,
                                 u_final_per_ray, w.d_fine, beta_map, iter_usage, w.sampler, (long long)w.sampler_bytes, n_escalated, stream)) return rc;
    if (t_coarse_dev) {
        w.t_coarse = const_cast<float*>(t_coarse_dev);
    } else if (int rc = upload_linspace_tables({{w.t_coarse, n_samples}}, stream)) {
        return rc;
    }
    if (int rc = nerfart_linspace_depths(w.t_coarse, n_samples, nullptr, nullptr, near_s, far_s, n_rays, w.d_coarse, n_samples, stream)) return rc;
    if (int rc = nerfart_sort_concat(n_rays, w.d_coarse, n_samples, n_samples, w.d_fine, n_importance, n_importance, d_all, P, stream)) return rc;
    // no per-sample output asked for: the samples behind full opacity reach no output and are not evaluated (final_stage_skipping); with any of
    // them the plain loop evaluates every sample, so the detailed outputs stay the reference's everywhere
    const bool skipping = !sdf_out && !nabla_out && !radiance_out && !sigma_out && !p_out && !tau_out;
    if (skipping)
        if (int rc = final_stage_skipping(w, surf_blob, precision, rad_blob, rad_precision, view_tiles, rays_o, n_rays, P, R_bg, alpha, beta, d_all, sdf,
                                          nabla, rad, k3_rays_chunk, stream)) return rc;
    for (int c0 = 0; c0 < n_rays && !skipping; c0 += k3_rays_chunk) {
        const int rk = (n_rays - c0 < k3_rays_chunk) ? n_rays - c0 : k3_rays_chunk;
        const size_t po = (size_t)c0 * P;
        if (int rc = nerfart_sdf_nabla_fwd_rays(surf_blob, precision, rays_o + 3 * (size_t)c0, w.rays_dn + 3 * (size_t)c0, nullptr,
                                                d_all + po, rk, P, P, R_bg, sdf + po, nabla + 3 * po, w.h7, w.nabla_ws, (long long)w.nabla_ws_bytes, stream)) return rc;
        if (int rc = nerfart_radiance_fwd_rays(rad_blob, rad_precision, view_tiles, rays_o + 3 * (size_t)c0, w.rays_dn + 3 * (size_t)c0,
                                               nullptr, d_all + po, rk, P, P, nabla + 3 * po, w.h7, rad + 3 * po, stream)) return rc;
    }
    return nerfart_volsdf_composite(n_rays, P, d_all, sdf, rad, nabla, alpha, beta, white_bkgd, rgb, depth, acc, normals,
                                    sigma_out, p_out, tau_out, stream);
}

int nerfart_volsdf_render_staged_fwd(const float* surf_blob, int precision, const float* rad_blob, int rad_precision, const float* sampler_blob,
                                     int sampler_precision, float sampler_guard, int view_tiles, const float* rays_o,
                              const float* rays_d, int n_rays, float near_s, float far_s, float R_bg, float alpha,
                              float beta, float eps, int n_samples, int n_importance, int max_upsample_steps,
                              int max_bisection_steps, int white_bkgd, int k3_rays_chunk, const float* t_coarse_dev,
                              const float* t_init_dev, const float* u_up_dev, const float* u_final_dev, int u_final_per_ray,
                              float* rgb, float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out, float* nabla_out,
                              float* radiance_out, float* sigma_out, float* p_out, float* tau_out, float* beta_map_out,
                              float* iter_usage_out, int* n_escalated, void* workspace, long long workspace_bytes, void* stream_) {
    return nerfart_volsdf_render_staged2_fwd(surf_blob, precision, rad_blob, rad_precision, sampler_blob, sampler_precision, sampler_guard, 0, view_tiles, rays_o,
                                             rays_d, n_rays, near_s, far_s, R_bg, alpha, beta, eps, n_samples, n_importance, max_upsample_steps,
                                             max_bisection_steps, white_bkgd, k3_rays_chunk, t_coarse_dev, t_init_dev, u_up_dev, u_final_dev, u_final_per_ray,
                                             rgb, depth, acc, normals, d_all_out, sdf_out, nabla_out, radiance_out, sigma_out, p_out, tau_out, beta_map_out,
                                             iter_usage_out, n_escalated, workspace, workspace_bytes, stream_);
}

int nerfart_volsdf_render_mixed_fwd(const float* surf_blob, const float* rad_blob, int precision, const float* sampler_blob, int sampler_precision,
                                    int view_tiles, const float* rays_o,
                              const float* rays_d, int n_rays, float near_s, float far_s, float R_bg, float alpha,
                              float beta, float eps, int n_samples, int n_importance, int max_upsample_steps,
                              int max_bisection_steps, int white_bkgd, int k3_rays_chunk, const float* t_coarse_dev,
                              const float* t_init_dev, const float* u_up_dev, const float* u_final_dev, int u_final_per_ray,
                              float* rgb, float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out, float* nabla_out,
                              float* radiance_out, float* sigma_out, float* p_out, float* tau_out, float* beta_map_out,
                              float* iter_usage_out, void* workspace, long long workspace_bytes, void* stream_) {
    return nerfart_volsdf_render_staged_fwd(surf_blob, precision, rad_blob, precision, sampler_blob, sampler_precision, 0.f, view_tiles, rays_o, rays_d, n_rays,
                                            near_s, far_s, R_bg, alpha, beta, eps, n_samples, n_importance, max_upsample_steps, max_bisection_steps, white_bkgd,
                                            k3_rays_chunk, t_coarse_dev, t_init_dev, u_up_dev, u_final_dev, u_final_per_ray, rgb, depth, acc, normals, d_all_out,
                                            sdf_out, nabla_out, radiance_out, sigma_out, p_out, tau_out, beta_map_out, iter_usage_out, nullptr, workspace,
                                            workspace_bytes, stream_);
}

int nerfart_volsdf_render_fwd(const float* surf_blob, const float* rad_blob, int precision, int view_tiles, const float* rays_o,
                              const float* rays_d, int n_rays, float near_s, float far_s, float R_bg, float alpha,
                              float beta, float eps, int n_samples, int n_importance, int max_upsample_steps,
                              int max_bisection_steps, int white_bkgd, int k3_rays_chunk, const float* t_coarse_dev,
                              const float* t_init_dev, const float* u_up_dev, const float* u_final_dev, int u_final_per_ray,
                              float* rgb, float* depth, float* acc, float* normals, float* d_all_out, float* sdf_out, float* nabla_out,
                              float* radiance_out, float* sigma_out, float* p_out, float* tau_out, float* beta_map_out,
                              float* iter_usage_out, void* workspace, long long workspace_bytes, void* stream_) {
    return nerfart_volsdf_render_mixed_fwd(surf_blob, rad_blob, precision, surf_blob, precision, view_tiles, rays_o, rays_d, n_rays, near_s, far_s, R_bg, alpha,
                                           beta, eps, n_samples, n_importance, max_upsample_steps, max_bisection_steps, white_bkgd, k3_rays_chunk,
                                           t_coarse_dev, t_init_dev, u_up_dev, u_final_dev, u_final_per_ray, rgb, depth, acc, normals, d_all_out, sdf_out,
                                           nabla_out, radiance_out, sigma_out, p_out, tau_out, beta_map_out, iter_usage_out, workspace, workspace_bytes,
                                           stream_);
}

}  // extern "C"
