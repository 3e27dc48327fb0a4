// mesh_vertices.hip - the mesh-side stages of extract_mesh's vertex refinement (mesh_util.refine_vertices): small per-vertex kernels around the
// SDF query, as the surface renderer's stages in ray_casting.hip are per-ray kernels around it.  A mesh vertex lives on a grid edge
// (csrc/marching_cubes.hip: k_mc_emit_edges records which, edge = 3 p + axis, p the owning point's linear index) at the parameter t in [0, 1];
// refinement moves t and nothing else, so the faces of nerfart_mc_emit stay valid and a closed mesh stays closed.
//   k_edge_points   t -> position, with k_mc_emit's arithmetic operation for operation (the same t and frame give the same bits).
//   k_refine_step   one step of bracket-keeping false position with the Illinois modification, given the SDF at the current t.
// One thread per vertex, no atomics: two runs give the same bits.  Every rounding of the two rules is written out (fmaf, __f*_rn), so no
// contraction can change the documented order of operations.
#include "nerfart_common.h"
#include <cmath>
#include <stdio.h>

namespace nerfart {
namespace mv {

struct Frame { float o[3], s[3]; };

__global__ void __launch_bounds__(256) k_edge_points(const unsigned* __restrict__ edge, const float* __restrict__ t, unsigned V, int nx, int ny, int nz,
                                                     Frame fr, float* __restrict__ pts) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= V) return;
    const unsigned e = edge[i], p = e / 3u, ax = e - 3u * p;
    const unsigned n = (unsigned)nx * (unsigned)ny * (unsigned)nz;        // 3 n < 2^31: checked by the host
    if (p >= n) return;
    const unsigned plane = (unsigned)ny * (unsigned)nz, r = p % plane;
    const int idx[3] = {(int)(p / plane), (int)(r / (unsigned)nz), (int)(r % (unsigned)nz)}, dim[3] = {nx, ny, nz};
    float q[3];
    int ia = 0, da = 0;
    float sa = 0.f, oa = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q[c] = fmaf((float)idx[c], fr.s[c], fr.o[c]);
        if ((unsigned)c == ax) { ia = idx[c]; da = dim[c]; sa = fr.s[c]; oa = fr.o[c]; }
    }
    if (ia + 1 >= da) return;                                             // the edge's far end is outside the volume
    const float pa = ax == 0 ? q[0] : ax == 1 ? q[1] : q[2];
    const float pb = fmaf((float)(ia + 1), sa, oa);
    const float qa = fmaf(t[i], __fsub_rn(pb, pa), pa);
    float* out = pts + 3 * (size_t)i;
    out[0] = ax == 0 ? qa : q[0];
    out[1] = ax == 1 ? qa : q[1];
    out[2] = ax == 2 ? qa : q[2];
}

// The rule of include/nerfart_hip.h (nerfart_mesh_edge_refine_step), step for step.
__global__ void __launch_bounds__(256) k_refine_step(const float* __restrict__ f, float level, unsigned V, float* __restrict__ bracket,
                                                     float* __restrict__ t_io, float* __restrict__ best, unsigned char* __restrict__ side) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= V) return;
    const float t = t_io[i];
    const float g = __fsub_rn(f[i], level);
    float* bs = best + 2 * (size_t)i;
    if (fabsf(g) < fabsf(bs[1])) { bs[0] = t; bs[1] = g; }               // 1: NaN never wins; +inf (the initial g_best) loses to every finite g
    if (g != g) return;                                                   // 2
    float* br = bracket + 4 * (size_t)i;
    if (g == 0.f) {                                                       // 3
        br[0] = t; br[1] = 0.f; br[2] = t; br[3] = 0.f;
        side[i] = 0;
        return;
    }
    float t0 = br[0], g0 = br[1], t1 = br[2], g1 = br[3];
    const unsigned char s = side[i];
    if ((g < 0.f) == (g0 < 0.f)) {                                        // 4
        if (s == 1) g1 = __fmul_rn(g1, 0.5f);
        t0 = t; g0 = g;
        side[i] = 1;
    } else {
        if (s == 2) g0 = __fmul_rn(g0, 0.5f);
        t1 = t; g1 = g;
        side[i] = 2;
    }
    br[0] = t0; br[1] = g0; br[2] = t1; br[3] = g1;
    float tn = __fsub_rn(t0, __fdiv_rn(__fmul_rn(g0, __fsub_rn(t1, t0)), __fsub_rn(g1, g0)));      // 5
    if (!isfinite(tn)) tn = __fmul_rn(0.5f, __fadd_rn(t0, t1));
    t_io[i] = fminf(fmaxf(tn, fminf(t0, t1)), fmaxf(t0, t1));
}

}  // namespace mv
}  // namespace nerfart

using namespace nerfart;

extern "C" {

int nerfart_mesh_edge_points(const unsigned* edge, const float* t, unsigned V, int nx, int ny, int nz, const float* origin, const float* spacing,
                             float* pts_out, void* stream) {
    if (V == 0) return 0;
    if (!edge || !t || !origin || !spacing || !pts_out) { set_last_error("mesh_edge_points: null pointer"); return 2; }
    if (nx < 2 || ny < 2 || nz < 2 || 3.0 * (double)nx * (double)ny * (double)nz >= 2147483648.0) {
        char msg[200];
        snprintf(msg, sizeof(msg), "mesh_edge_points: every dimension must be >= 2 and 3 nx ny nz below 2^31 (got %d x %d x %d)", nx, ny, nz);
        set_last_error(msg);
        return 2;
    }
    mv::Frame fr;
    for (int a = 0; a < 3; ++a) { fr.o[a] = origin[a]; fr.s[a] = spacing[a]; }
    hipLaunchKernelGGL(mv::k_edge_points, dim3((V + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, edge, t, V, nx, ny, nz, fr, pts_out);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mesh_edge_refine_step(const float* f, float level, unsigned V, float* bracket, float* t, float* best, unsigned char* side, void* stream) {
    if (V == 0) return 0;
    if (!f || !bracket || !t || !best || !side) { set_last_error("mesh_edge_refine_step: null pointer"); return 2; }
    hipLaunchKernelGGL(mv::k_refine_step, dim3((V + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, f, level, V, bracket, t, best, side);
    NERFART_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
