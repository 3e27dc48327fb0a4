// volsdf_geo_backward.hip - backward of the per-ray stage of the VolSDF renderer w.r.t. its DEPTH and NORMALS maps (the geometry terms of a
// fine-tune objective: depth preservation, normal consistency, smoothness).  The sibling k_composite_volsdf_bwd (volsdf_backward.hip) takes the
// rgb and opacity cotangents; the per-ray backward is linear in the cotangent of the weights tau_k, so this kernel only ADDS what the two maps
// contribute and leaves the rest of pass 2 (sphere-clamp mask, second-order SDF sweeps, reductions, the nabla cotangent path) as it is.
//
//   forward (k_composite_volsdf, volsdf.py:544-576):  tau_k = (1 - p_k + 1e-10) T_k over the first P - 1 samples,  acc = sum tau_k,
//       inv = acc + 1e-10,  depth = sum tau_k d_k / inv,  normals = sum tau_k n_k,  n_k = nabla_k / max(|nabla_k|, 1e-12)   (F.normalize)
//       The sample depths carry no gradient (volsdf.py:479).
//   backward:  g_tau_k = g_normals . n_k + (g_depth / inv) (d_k - depth)
//       then as the sibling, formula for formula:  g_x_k = p_k T_k g_tau_k - sum_{i>k} tau_i g_tau_i,  g_sigma_k = [x_k > 0] delta_k g_x_k,
//       g_s_k = -g_sigma_k alpha e / beta,  g_alpha += g_sigma_k psi_k,  g_beta += g_sigma_k alpha e s / beta^2,  e = 0.5 exp(-|s| / beta)
//       g_nabla_k = tau_k (g_normals - n_k (n_k . g_normals)) / |nabla_k|   where |nabla_k| >= 1e-12
//                 = tau_k g_normals / 1e-12                                  below that (the clamp_min of F.normalize, as autograd differentiates it)
//       The last sample carries no weight: its g_sdf and g_nabla are 0 (+ g_n_in).
// EMPTY RAYS: (d_k - depth) / inv grows without bound as acc -> 0 (inv -> 1e-10): a depth cotangent on a ray that hits nothing is amplified by
// up to 1e10, exactly as autograd through the reference's `tau / (acc + 1e-10)` amplifies it.  Nothing is clamped here; a loss on the depth map
// should weight its cotangent with the opacity (or zero it on empty rays).
// One wave per ray, seg = ceil((P - 1) / 64) <= 8 intervals per lane held in registers (every loop over them is fully unrolled with constant
// indices: no scratch).  Three passes: A recomputes p, T, tau, acc, depth with the forward's expressions in the forward's order; B forms g_tau and
// the segment sums of tau g_tau, then their exclusive suffix over the lanes; C walks each segment backwards.
#include "ray_common.h"

namespace nerfart {

__global__ void __launch_bounds__(64)
k_composite_volsdf_geo_bwd(int P, const float* __restrict__ d_all, const float* __restrict__ sdf, const float* __restrict__ nabla, float alpha,
                           float beta, const float* __restrict__ g_depth, const float* __restrict__ g_normals, const float* g_n_in, int accumulate,
                           float* __restrict__ g_sdf, float* g_nabla, float* __restrict__ g_alpha_beta) {
    constexpr int MAXSEG = 8;                                  // P <= 513
    const int ray = blockIdx.x, lane = threadIdx.x;
    const int nint = P - 1;
    const int seg = (nint + 63) >> 6;
    const int k0 = lane * seg, k1 = (k0 + seg < nint) ? k0 + seg : nint;
    const int cnt = k1 - k0;                                   // <= 0 on the lanes past the last interval
    const float* dr = d_all + (size_t)ray * P;
    const float* sr = sdf + (size_t)ray * P;
    const size_t row = (size_t)ray * P;
    const bool have_n = g_normals != nullptr;
    const float gd = g_depth ? g_depth[ray] : 0.f;
    float gnx = 0.f, gny = 0.f, gnz = 0.f;
    if (have_n) { gnx = g_normals[3 * (size_t)ray]; gny = g_normals[3 * (size_t)ray + 1]; gnz = g_normals[3 * (size_t)ray + 2]; }

    // ---- pass A: the forward's p, T, tau, acc, depth (k_composite_volsdf's expressions in its order)
    float ps[MAXSEG], Ts[MAXSEG], gt[MAXSEG];
    float lp = 1.f;
#pragma unroll
    for (int i = 0; i < MAXSEG; ++i) {
        ps[i] = 1.f; Ts[i] = 0.f; gt[i] = 0.f;
        if (i < cnt) {
            const int k = k0 + i;
            const float sg = sdf_to_sigma(sr[k], alpha, beta);
            ps[i] = expf(-fmaxf(sg * (dr[k + 1] - dr[k]), 0.f));
            lp *= ps[i];
        }
    }
    const float T0 = wave_excl_prod(lp);
    float T = T0, a = 0.f;
#pragma unroll
    for (int i = 0; i < MAXSEG; ++i) {
        if (i < cnt) {
            Ts[i] = T;
            a += (1.f - ps[i] + 1e-10f) * T;
            T *= ps[i];
        }
    }
    a = wave_sum(a);
    const float inv = a + 1e-10f;
    float dp = 0.f;
#pragma unroll
    for (int i = 0; i < MAXSEG; ++i) {
        if (i < cnt) {
            const float tau = (1.f - ps[i] + 1e-10f) * Ts[i];
            dp += tau / inv * dr[k0 + i];
        }
    }
    const float depth = wave_sum(dp);

    // ---- pass B: g_tau and the sum of tau g_tau over the intervals AFTER this lane's segment
    const float gdi = gd / inv;
    float hsum = 0.f;
#pragma unroll
    for (int i = 0; i < MAXSEG; ++i) {
        if (i < cnt) {
            const int k = k0 + i;
            float dot = 0.f;
            if (have_n) {
                const size_t q = row + k;
                const float vx = nabla[3 * q], vy = nabla[3 * q + 1], vz = nabla[3 * q + 2];
                const float nr = fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);     // F.normalize eps, as the forward
                dot = fmaf(gnz, vz / nr, fmaf(gny, vy / nr, gnx * (vx / nr)));
            }
            gt[i] = fmaf(gdi, dr[k] - depth, dot);
            const float tau = (1.f - ps[i] + 1e-10f) * Ts[i];
            hsum = fmaf(tau, gt[i], hsum);
        }
    }
    float S = wave_excl_suffix_sum(hsum);

    // ---- pass C (descending inside the segment): cotangents
    float ga = 0.f, gbeta = 0.f;
#pragma unroll
    for (int i = MAXSEG - 1; i >= 0; --i) {
        if (i < cnt) {
            const int k = k0 + i;
            const size_t q = row + k;
            const float s = sr[k], delta = dr[k + 1] - dr[k];
            const float e = 0.5f * expf(-fabsf(s) / beta);
            const float psi = (s >= 0.f) ? e : 1.f - e;
            const float sg = alpha * psi;
            const float p = ps[i], Tk = Ts[i], gtau = gt[i];
            const float tau = (1.f - p + 1e-10f) * Tk;
            const float gx = fmaf(p * Tk, gtau, -S);
            const float gsig = (sg * delta > 0.f) ? gx * delta : 0.f;
            const float v = gsig * alpha * (-e / beta);
            g_sdf[q] = accumulate ? g_sdf[q] + v : v;
            ga = fmaf(gsig, psi, ga);
            gbeta = fmaf(gsig * alpha, e * s / (beta * beta), gbeta);
            S = fmaf(tau, gtau, S);
            if (have_n) {
                const float vx = nabla[3 * q], vy = nabla[3 * q + 1], vz = nabla[3 * q + 2];
                const float nrm = sqrtf(vx * vx + vy * vy + vz * vz);
                float ox, oy, oz;
                if (nrm >= 1e-12f) {
                    const float nx = vx / nrm, ny = vy / nrm, nz = vz / nrm;
                    const float dn = fmaf(gnz, nz, fmaf(gny, ny, gnx * nx));
                    const float w = tau / nrm;
                    ox = w * fmaf(-nx, dn, gnx); oy = w * fmaf(-ny, dn, gny); oz = w * fmaf(-nz, dn, gnz);
                } else {
                    const float w = tau / 1e-12f;
                    ox = w * gnx; oy = w * gny; oz = w * gnz;
                }
                if (g_n_in) { ox += g_n_in[3 * q]; oy += g_n_in[3 * q + 1]; oz += g_n_in[3 * q + 2]; }
                g_nabla[3 * q] = ox; g_nabla[3 * q + 1] = oy; g_nabla[3 * q + 2] = oz;
            }
        }
    }
    if (lane == 0) {
        const size_t q = row + P - 1;
        if (!accumulate) g_sdf[q] = 0.f;
        if (have_n) {
            g_nabla[3 * q] = g_n_in ? g_n_in[3 * q] : 0.f;
            g_nabla[3 * q + 1] = g_n_in ? g_n_in[3 * q + 1] : 0.f;
            g_nabla[3 * q + 2] = g_n_in ? g_n_in[3 * q + 2] : 0.f;
        }
    }
    ga = wave_sum(ga); gbeta = wave_sum(gbeta);
    if (lane == 0 && g_alpha_beta) { atomicAdd(g_alpha_beta, ga); atomicAdd(g_alpha_beta + 1, gbeta); }
}

}  // namespace nerfart

using namespace nerfart;

extern "C" {
int nerfart_volsdf_composite_geo_bwd(int n_rays, int P, const float* d_all, const float* sdf, const float* nabla, float alpha, float beta,
                                     const float* g_depth, const float* g_normals, const float* g_n_in, int accumulate, float* g_sdf,
                                     float* g_nabla, float* g_alpha_beta, void* stream) {
    if (n_rays <= 0) return 0;
    if (P < 2 || P > 513) { set_last_error("composite_geo_bwd: 2 <= P <= 513"); return 2; }
    if (!g_depth && !g_normals) { set_last_error("composite_geo_bwd: pass g_depth, g_normals or both (both are NULL)"); return 2; }
    if (!d_all || !sdf || !g_sdf) { set_last_error("composite_geo_bwd: null argument (d_all / sdf / g_sdf)"); return 2; }
    if (g_normals && !(nabla && g_nabla)) { set_last_error("composite_geo_bwd: g_normals needs nabla and g_nabla"); return 2; }
    hipLaunchKernelGGL(k_composite_volsdf_geo_bwd, dim3(n_rays), dim3(64), 0, (hipStream_t)stream, P, d_all, sdf, nabla, alpha, beta, g_depth,
                       g_normals, g_n_in, accumulate, g_sdf, g_nabla, g_alpha_beta);
    NERFART_HIP(hipGetLastError());
    return 0;
}
}
