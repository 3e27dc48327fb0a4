// mesh_texture.hip - the device side of extract_mesh's texture bake (mesh_util.texel_points / bake_texture): where every texel of a per-face
// atlas sits in space, and one Newton step that puts such a point back onto the level set.  The radiance and SDF queries between them are the
// caller's (the MLP kernels); these kernels make points and move them.  The layout is the closed form of (F, P) in include/nerfart_hip.h
// (nerfart_mesh_atlas_layout): two faces per square cell of side S = P + 3, no chart, no rasteriser, no dilation - the gutter texels bilinear
// filtering reads are points at extrapolated barycentrics of the same face.
//   k_atlas_points   one thread per texel, lanes along x: owner face, barycentric weights from the integer local coordinates, the point.
//   k_project_step   one thread per point: p -= clamp(|e| / |g|, max_step) sign(e) g / |g|, e = sdf - level.
// No atomics, no scratch: two runs give the same bits.  Every rounding of the two rules is written out (fmaf, __f*_rn), so no contraction can
// change the documented order of operations - tests/mesh_texture_ref.py derives its bounds from exactly these expressions.
#include "nerfart_common.h"
#include <cmath>
#include <stdio.h>

namespace nerfart {
namespace mt {

constexpr int MAX_SIDE = 16384;          // W, H <= MAX_SIDE: W H <= 2^28 texels, 3 W H floats index well inside 32 bits

struct Layout { int S, Cw, Ch, W, H; };

// The closed form of include/nerfart_hip.h.  false: P < 1, F < 1 or an image side above MAX_SIDE (nothing else can overflow: see the guards).
static bool layout(long long F, long long P, Layout* L, char* why, size_t n) {
    if (P < 1 || F < 1) {
        snprintf(why, n, "mesh_atlas_layout: F and P must be >= 1 (got F = %lld, P = %lld)", F, P);
        return false;
    }
    if (P > MAX_SIDE - 3 || F > 2ll * MAX_SIDE * MAX_SIDE) {                      // S > MAX_SIDE resp. more cells than texels: over the limit whatever the rest
        snprintf(why, n, "mesh_atlas_layout: F = %lld faces at P = %lld do not fit an image of %d x %d texels", F, P, MAX_SIDE, MAX_SIDE);
        return false;
    }
    const long long S = P + 3, cells = (F + 1) / 2;
    long long Cw = (long long)sqrt((double)cells);
    while (Cw * Cw < cells) ++Cw;
    while (Cw > 1 && (Cw - 1) * (Cw - 1) >= cells) --Cw;
    const long long Ch = (cells + Cw - 1) / Cw;
    if (Cw * S > MAX_SIDE || Ch * S > MAX_SIDE) {
        snprintf(why, n, "mesh_atlas_layout: F = %lld faces at P = %lld need an image of %lld x %lld texels, above the limit of %d x %d", F, P, Cw * S,
                 Ch * S, MAX_SIDE, MAX_SIDE);
        return false;
    }
    L->S = (int)S; L->Cw = (int)Cw; L->Ch = (int)Ch; L->W = (int)(Cw * S); L->H = (int)(Ch * S);
    return true;
}

// The rule of include/nerfart_hip.h (nerfart_mesh_atlas_points), step for step.  x < W and y < H bound every store; a face index is used only
// after it was found inside [0, V).
__global__ void __launch_bounds__(256) k_atlas_points(const float* __restrict__ verts, const int* __restrict__ faces, unsigned V, unsigned F, int P,
                                                      Layout L, float* __restrict__ points, int* __restrict__ face_of, int* __restrict__ info) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= L.W || y >= L.H) return;
    const int cx = x / L.S, cy = y / L.S, i = x - cx * L.S, j = y - cy * L.S;
    const unsigned q = (unsigned)cy * (unsigned)L.Cw + (unsigned)cx;              // < Cw Ch <= 2^28
    const bool lower = i + j <= P + 2;
    const unsigned face = 2u * q + (lower ? 0u : 1u);
    const int a = lower ? i : L.S - 1 - i, b = lower ? j : L.S - 1 - j;
    const size_t t = (size_t)y * (size_t)L.W + (size_t)x;
    float px = 0.f, py = 0.f, pz = 0.f;
    int owner = -1;
    if (face < F) {                                                               // q < n_cells follows: face < F <= 2 n_cells
        const int* f = faces + 3 * (size_t)face;
        const int i0 = f[0], i1 = f[1], i2 = f[2];
        if ((unsigned)i0 < V && (unsigned)i1 < V && (unsigned)i2 < V) {
            const float fp = (float)P;
            const float w0 = __fdiv_rn((float)(P - a - b), fp), w1 = __fdiv_rn((float)a, fp), w2 = __fdiv_rn((float)b, fp);
            const float *v0 = verts + 3 * (size_t)i0, *v1 = verts + 3 * (size_t)i1, *v2 = verts + 3 * (size_t)i2;
            px = fmaf(w2, v2[0], fmaf(w1, v1[0], __fmul_rn(w0, v0[0])));
            py = fmaf(w2, v2[1], fmaf(w1, v1[1], __fmul_rn(w0, v0[1])));
            pz = fmaf(w2, v2[2], fmaf(w1, v1[2], __fmul_rn(w0, v0[2])));
            owner = (int)face;
        } else {
            info[0] = 1;                                                          // every writer stores the same value
        }
    }
    float* out = points + 3 * t;
    out[0] = px; out[1] = py; out[2] = pz;
    face_of[t] = owner;
}

// The rule of include/nerfart_hip.h (nerfart_mesh_project_step), step for step.
__global__ void __launch_bounds__(256) k_project_step(float* __restrict__ points, const float* __restrict__ sdf, const float* __restrict__ nabla,
                                                      unsigned n, float level, float max_step) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float s = sdf[i];
    const float* g = nabla + 3 * (size_t)i;
    const float gx = g[0], gy = g[1], gz = g[2];
    if (!(isfinite(s) && isfinite(gx) && isfinite(gy) && isfinite(gz))) return;
    const float g2 = fmaf(gz, gz, fmaf(gy, gy, __fmul_rn(gx, gx)));
    if (!(g2 >= 1e-12f) || !isfinite(g2)) return;
    const float e = __fsub_rn(s, level);
    const float gn = __fsqrt_rn(g2);
    const float m = fminf(__fdiv_rn(fabsf(e), gn), max_step);                    // the step's length: |e| / |g|, at most max_step
    const float c = __fdiv_rn(copysignf(m, -e), gn);                             // d = c g = -sign(e) m g / |g|
    if (!isfinite(c)) return;                                                     // a non-finite level
    float* p = points + 3 * (size_t)i;
    p[0] = __fadd_rn(p[0], __fmul_rn(c, gx));
    p[1] = __fadd_rn(p[1], __fmul_rn(c, gy));
    p[2] = __fadd_rn(p[2], __fmul_rn(c, gz));
}

}  // namespace mt
}  // namespace nerfart

using namespace nerfart;

extern "C" {

int nerfart_mesh_atlas_layout(long long F, long long P, int* dims) {
    if (!dims) { set_last_error("mesh_atlas_layout: null pointer"); return 2; }
    mt::Layout L;
    char why[256];
    if (!mt::layout(F, P, &L, why, sizeof(why))) { set_last_error(why); return 2; }
    dims[0] = L.S; dims[1] = L.Cw; dims[2] = L.Ch; dims[3] = L.W; dims[4] = L.H;
    return 0;
}

int nerfart_mesh_atlas_points(const float* verts, const int* faces, unsigned V, unsigned F, int P, float* points, int* face_of, int* info,
                              void* stream) {
    mt::Layout L;
    char why[256];
    if (!mt::layout((long long)F, (long long)P, &L, why, sizeof(why))) { set_last_error(why); return 2; }
    if (!faces || !points || !face_of || !info || (V && !verts)) { set_last_error("mesh_atlas_points: null pointer"); return 2; }
    if (V >= 2147483648u) { set_last_error("mesh_atlas_points: V must be below 2^31"); return 2; }
    NERFART_HIP(hipMemsetAsync(info, 0, sizeof(int), (hipStream_t)stream));
    hipLaunchKernelGGL(mt::k_atlas_points, dim3(((unsigned)L.W + 63u) / 64u, ((unsigned)L.H + 3u) / 4u), dim3(64, 4), 0, (hipStream_t)stream, verts,
                       faces, V, F, P, L, points, face_of, info);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mesh_project_step(float* points, const float* sdf, const float* nabla, unsigned n, float level, float max_step, void* stream) {
    if (n == 0) return 0;
    if (!points || !sdf || !nabla) { set_last_error("mesh_project_step: null pointer"); return 2; }
    if (!(max_step > 0.f)) { set_last_error("mesh_project_step: max_step must be positive"); return 2; }
    hipLaunchKernelGGL(mt::k_project_step, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, points, sdf, nabla, n, level, max_step);
    NERFART_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
