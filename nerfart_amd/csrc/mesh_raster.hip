// mesh_raster.hip - the device side of mesh_util.rasterize / render_mesh: an indexed triangle mesh seen through a rend_util.get_rays camera.
// Every decision is an integer, every float result is computed once, in the order include/nerfart_hip.h writes out, so that the image does not
// depend on the order the faces were worked in and tests/mesh_raster_ref.py can state the same rules in numpy and compare for equality.
//   k_project        one thread per vertex: camera space in double, the pixel position snapped to 1/256 pixel (int32), a validity flag.
//   k_raster_small   one thread per face: index and validity checks, the doubled area in int64, the clipped box; a box of at most 256 pixels is
//                    walked here, a larger one is appended to a list (integer atomic; the image does not depend on the list's order).
//   k_raster_large   one workgroup per listed face (grid-stride over the list), threads across the box.
//   k_resolve        one thread per pixel, lanes along x: the winning face, its depth again, barycentrics, the face normal.
//   k_interp         one thread per pixel: barycentric interpolation of per-vertex or per-corner attributes.
//   k_sample_bilinear one thread per sample: clamp-to-edge bilinear read of a uint8 rgb image.
// Coverage is three int64 edge functions with the top-left rule; the depth test is atomicMin on (bits(float z) << 32 | face): integer atomics only,
// no float atomics, no scratch, no workgroup waits for another.  fp64 is used where the header says so and nowhere else; contraction is off in this
// file, so a * b + c below is two roundings, as in numpy.
#include "nerfart_common.h"
#include <cmath>

#pragma clang fp contract(off)

namespace nerfart {
namespace mr {

constexpr int MAX_SIDE = 16384;            // H, W <= MAX_SIDE: H W <= 2^28 pixels
constexpr int SMALL_BOX = 256;             // a face whose clipped box holds at most this many pixels is walked by its own thread
constexpr int FIX = 256;                   // sub-pixel steps per pixel (8 bits)
constexpr double MAX_PIXEL = 32768.0;      // |u|, |v| <= 2^15 pixels: |xy_fix| <= 2^23, differences <= 2^24, products <= 2^48

struct Cam {                               // by value to every kernel: the host's numbers, nothing is read from device memory
    float w2c[12];                         // rows of the world-to-camera 3x4 (the host's float64 inverse of c2w, rounded once)
    float rot[9];                          // the rotation of c2w, row-major (camera -> world, for the normals)
    float fx, sk, cx, fy, cy, near;
};

struct Plane { double nx, ny, nz, na; };   // n = (b - a) x (c - a), na = n . a

// The ray of pixel (column i, row j) in camera space, r = (x, y, 1): k_get_rays' expressions (csrc/raygen.hip), in double.
__device__ __forceinline__ void pixel_ray(const Cam& C, int i, int j, double* x, double* y) {
    const double fx = C.fx, sk = C.sk, cx = C.cx, fy = C.fy, cy = C.cy, di = (double)i, dj = (double)j;
    *x = ((di - cx + cy * sk / fy) - sk * dj / fy) / fx;
    *y = (dj - cy) / fy;
}

__device__ __forceinline__ Plane face_plane(const float* __restrict__ cam, int i0, int i1, int i2, double* a, double* b, double* c) {
    const float *pa = cam + 3 * (size_t)i0, *pb = cam + 3 * (size_t)i1, *pc = cam + 3 * (size_t)i2;
    a[0] = pa[0]; a[1] = pa[1]; a[2] = pa[2];
    b[0] = pb[0]; b[1] = pb[1]; b[2] = pb[2];
    c[0] = pc[0]; c[1] = pc[1]; c[2] = pc[2];
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    Plane P;
    P.nx = uy * vz - uz * vy;
    P.ny = uz * vx - ux * vz;
    P.nz = ux * vy - uy * vx;
    P.na = P.nx * a[0] + P.ny * a[1] + P.nz * a[2];
    return P;
}

__device__ __forceinline__ double plane_z(const Plane& P, double x, double y) { return P.na / (P.nx * x + P.ny * y + P.nz); }

__global__ void __launch_bounds__(256) k_project(const float* __restrict__ verts, unsigned V, Cam C, int* __restrict__ xy_fix, float* __restrict__ cam,
                                                 unsigned char* __restrict__ valid) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= V) return;
    const float* p = verts + 3 * (size_t)i;
    const double px = p[0], py = p[1], pz = p[2];
    const double X = (double)C.w2c[0] * px + (double)C.w2c[1] * py + (double)C.w2c[2] * pz + (double)C.w2c[3];
    const double Y = (double)C.w2c[4] * px + (double)C.w2c[5] * py + (double)C.w2c[6] * pz + (double)C.w2c[7];
    const double Z = (double)C.w2c[8] * px + (double)C.w2c[9] * py + (double)C.w2c[10] * pz + (double)C.w2c[11];
    const double xz = X / Z, yz = Y / Z;
    const double u = (double)C.fx * xz + (double)C.sk * yz + (double)C.cx, v = (double)C.fy * yz + (double)C.cy;
    const bool ok = Z >= (double)C.near && fabs(u) <= MAX_PIXEL && fabs(v) <= MAX_PIXEL;       // a NaN fails every comparison
    xy_fix[2 * (size_t)i] = ok ? (int)rint(u * (double)FIX) : 0;                                // rint: round half to even, |.| <= 2^23
    xy_fix[2 * (size_t)i + 1] = ok ? (int)rint(v * (double)FIX) : 0;
    float* o = cam + 3 * (size_t)i;
    o[0] = (float)X; o[1] = (float)Y; o[2] = (float)Z;
    valid[i] = ok ? 1 : 0;
}

struct Setup {                             // a face ready to be walked: the oriented corners (A > 0), the clipped box, the plane
    long long x0, y0, x1, y1, x2, y2;
    int i_lo, i_hi, j_lo, j_hi;
    Plane P;
};

// false: the face draws nothing (bad index - flagged -, an invalid vertex - counted when `count` -, A == 0, a box off the image).
__device__ __forceinline__ bool setup_face(const int* __restrict__ xy_fix, const float* __restrict__ cam, const unsigned char* __restrict__ valid,
                                           const int* __restrict__ faces, unsigned V, unsigned face, int H, int W, int* __restrict__ info, bool count,
                                           Setup* S) {
    const int* f = faces + 3 * (size_t)face;
    const int i0 = f[0], i1 = f[1], i2 = f[2];
    if (!((unsigned)i0 < V && (unsigned)i1 < V && (unsigned)i2 < V)) {
        if (count) info[0] = 1;                                                   // every writer stores the same value
        return false;
    }
    if (!(valid[i0] && valid[i1] && valid[i2])) {
        if (count) atomicAdd(info + 1, 1);
        return false;
    }
    long long x0 = xy_fix[2 * (size_t)i0], y0 = xy_fix[2 * (size_t)i0 + 1];
    long long x1 = xy_fix[2 * (size_t)i1], y1 = xy_fix[2 * (size_t)i1 + 1];
    long long x2 = xy_fix[2 * (size_t)i2], y2 = xy_fix[2 * (size_t)i2 + 1];
    const long long A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);            // |factor| <= 2^24: |product| <= 2^48
    if (A == 0) return false;
    if (A < 0) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }   // both orientations are drawn
    const long long xmin = min(x0, min(x1, x2)), xmax = max(x0, max(x1, x2)), ymin = min(y0, min(y1, y2)), ymax = max(y0, max(y1, y2));
    // samples sit at (256 i, 256 j): i from ceil(xmin / 256) to floor(xmax / 256); >> of a negative long long is the arithmetic shift (floor)
    const long long i_lo = max((xmin + (FIX - 1)) >> 8, 0ll), i_hi = min(xmax >> 8, (long long)W - 1);
    const long long j_lo = max((ymin + (FIX - 1)) >> 8, 0ll), j_hi = min(ymax >> 8, (long long)H - 1);
    if (i_lo > i_hi || j_lo > j_hi) return false;
    S->x0 = x0; S->y0 = y0; S->x1 = x1; S->y1 = y1; S->x2 = x2; S->y2 = y2;
    S->i_lo = (int)i_lo; S->i_hi = (int)i_hi; S->j_lo = (int)j_lo; S->j_hi = (int)j_hi;
    double a[3], b[3], c[3];
    S->P = face_plane(cam, i0, i1, i2, a, b, c);                                  // the face's own order, whatever the orientation on screen
    return true;
}

// E of the directed edge (xa, ya) -> (xb, yb) at the sample (px, py); with A > 0 the inside is E > 0.  y runs down, so with A > 0 the corners run
// clockwise on screen: a TOP edge is horizontal and runs to the right (dy == 0, dx > 0), a LEFT edge runs up (dy < 0).
__device__ __forceinline__ bool edge_covers(long long xa, long long ya, long long xb, long long yb, long long px, long long py) {
    const long long dx = xb - xa, dy = yb - ya;
    const long long E = dx * (py - ya) - dy * (px - xa);
    return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// One sample of one face: coverage, depth, the atomic.  (i, j) is inside the image (the box was clipped).
__device__ __forceinline__ void shade_sample(const Setup& S, const Cam& C, unsigned face, int i, int j, int W, unsigned long long* __restrict__ zbuf,
                                             int* __restrict__ info) {
    const long long px = (long long)i * FIX, py = (long long)j * FIX;
    if (!(edge_covers(S.x0, S.y0, S.x1, S.y1, px, py) && edge_covers(S.x1, S.y1, S.x2, S.y2, px, py) && edge_covers(S.x2, S.y2, S.x0, S.y0, px, py)))
        return;
    double x, y;
    pixel_ray(C, i, j, &x, &y);
    const double z = plane_z(S.P, x, y);
    if (!(z >= (double)C.near) || !isfinite(z)) { atomicAdd(info + 2, 1); return; }
    const float zf = (float)z;                                                    // z > 0: the bit patterns order as the floats do
    const unsigned long long key = ((unsigned long long)__float_as_uint(zf) << 32) | (unsigned long long)face;
    atomicMin(zbuf + (size_t)j * (size_t)W + (size_t)i, key);
}

__global__ void __launch_bounds__(256) k_raster_small(const int* __restrict__ xy_fix, const float* __restrict__ cam, const unsigned char* __restrict__ valid,
                                                      const int* __restrict__ faces, unsigned V, unsigned F, Cam C, int H, int W,
                                                      unsigned long long* __restrict__ zbuf, int* __restrict__ list, int* __restrict__ info) {
    const unsigned face = blockIdx.x * 256u + threadIdx.x;
    if (face >= F) return;
    Setup S;
    if (!setup_face(xy_fix, cam, valid, faces, V, face, H, W, info, true, &S)) return;
    const int bw = S.i_hi - S.i_lo + 1, bh = S.j_hi - S.j_lo + 1;
    if ((long long)bw * bh > SMALL_BOX) {
        const int slot = atomicAdd(info + 3, 1);                                  // < F: every face appends at most once
        list[slot] = (int)face;
        return;
    }
    for (int j = S.j_lo; j <= S.j_hi; ++j)                                        // bh * bw <= SMALL_BOX iterations in all
        for (int i = S.i_lo; i <= S.i_hi; ++i) shade_sample(S, C, face, i, j, W, zbuf, info);
}

__global__ void __launch_bounds__(256) k_raster_large(const int* __restrict__ xy_fix, const float* __restrict__ cam, const unsigned char* __restrict__ valid,
                                                      const int* __restrict__ faces, unsigned V, unsigned F, Cam C, int H, int W,
                                                      unsigned long long* __restrict__ zbuf, const int* __restrict__ list, int* __restrict__ info) {
    const unsigned n = min((unsigned)info[3], F);                                 // written by the launch before this one
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {                        // at most ceil(F / gridDim.x) rounds
        const unsigned face = (unsigned)list[e];
        if (face >= F) continue;
        Setup S;
        if (!setup_face(xy_fix, cam, valid, faces, V, face, H, W, info, false, &S)) continue;          // counted and flagged by k_raster_small
        const unsigned bw = (unsigned)(S.i_hi - S.i_lo + 1), bh = (unsigned)(S.j_hi - S.j_lo + 1), box = bw * bh;        // <= H W <= 2^28
        for (unsigned t = threadIdx.x; t < box; t += 256u)                        // ceil(box / 256) rounds
            shade_sample(S, C, face, S.i_lo + (int)(t % bw), S.j_lo + (int)(t / bw), W, zbuf, info);
    }
}

__global__ void __launch_bounds__(256) k_resolve(const unsigned long long* __restrict__ zbuf, const float* __restrict__ cam, const int* __restrict__ faces,
                                                 unsigned V, unsigned F, Cam C, int H, int W, int* __restrict__ face_id, float* __restrict__ bary,
                                                 float* __restrict__ zout, float* __restrict__ depth, unsigned char* __restrict__ mask,
                                                 float* __restrict__ normals) {
    const int i = (int)(blockIdx.x * 64u + threadIdx.x), j = (int)(blockIdx.y * 4u + threadIdx.y);
    if (i >= W || j >= H) return;
    const size_t p = (size_t)j * (size_t)W + (size_t)i;
    const unsigned long long key = zbuf[p];
    int fid = -1;
    float w0 = 0.f, w1 = 0.f, w2 = 0.f, zf = 0.f, df = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
    const unsigned face = (unsigned)(key & 0xffffffffull);
    if (key != ~0ull && face < F) {
        const int* f = faces + 3 * (size_t)face;
        const int i0 = f[0], i1 = f[1], i2 = f[2];
        if ((unsigned)i0 < V && (unsigned)i1 < V && (unsigned)i2 < V) {           // raster drew the face, so this holds; nothing is read unchecked
            double a[3], b[3], c[3], x, y;
            const Plane P = face_plane(cam, i0, i1, i2, a, b, c);
            pixel_ray(C, i, j, &x, &y);
            const double z = plane_z(P, x, y);
            const double hx = z * x, hy = z * y, hz = z;                         // the hit point
            const double ax = a[0] - hx, ay = a[1] - hy, az = a[2] - hz, bx = b[0] - hx, by = b[1] - hy, bz = b[2] - hz;
            const double cx = c[0] - hx, cy = c[1] - hy, cz = c[2] - hz;
            const double nn = P.nx * P.nx + P.ny * P.ny + P.nz * P.nz;
            // w0 = n . ((b - h) x (c - h)) / (n . n), and cyclically: signed areas against the face's own normal
            const double s0 = P.nx * (by * cz - bz * cy) + P.ny * (bz * cx - bx * cz) + P.nz * (bx * cy - by * cx);
            const double s1 = P.nx * (cy * az - cz * ay) + P.ny * (cz * ax - cx * az) + P.nz * (cx * ay - cy * ax);
            const double s2 = P.nx * (ay * bz - az * by) + P.ny * (az * bx - ax * bz) + P.nz * (ax * by - ay * bx);
            w0 = (float)(s0 / nn); w1 = (float)(s1 / nn); w2 = (float)(s2 / nn);
            zf = (float)z;
            df = (float)(z * sqrt(x * x + y * y + 1.0));               // along the UNIT ray: render_fn's and surface_render's depths (both normalise rays_d)
            // the geometric normal, turned toward the camera (n . r < 0), taken to world space by c2w's rotation
            const double s = (P.nx * x + P.ny * y + P.nz > 0.0 ? -1.0 : 1.0) / sqrt(nn);
            const double mx = s * P.nx, my = s * P.ny, mz = s * P.nz;
            n0 = (float)((double)C.rot[0] * mx + (double)C.rot[1] * my + (double)C.rot[2] * mz);
            n1 = (float)((double)C.rot[3] * mx + (double)C.rot[4] * my + (double)C.rot[5] * mz);
            n2 = (float)((double)C.rot[6] * mx + (double)C.rot[7] * my + (double)C.rot[8] * mz);
            fid = (int)face;
        }
    }
    face_id[p] = fid;
    float* bo = bary + 3 * p;
    bo[0] = w0; bo[1] = w1; bo[2] = w2;
    zout[p] = zf;
    depth[p] = df;
    mask[p] = fid >= 0 ? 1 : 0;
    float* no = normals + 3 * p;
    no[0] = n0; no[1] = n1; no[2] = n2;
}

// out[p, c] = fma(w2, a2[c], fma(w1, a1[c], w0 * a0[c])) in fp32; a_k the attribute of corner k: attr[faces[f, k], c] (per vertex) or attr[f, k, c]
// (per corner, faces == nullptr).
__global__ void __launch_bounds__(256) k_interp(const int* __restrict__ face_id, const float* __restrict__ bary, const int* __restrict__ faces,
                                                const float* __restrict__ attr, unsigned V, unsigned F, int Cn, unsigned n, float fill,
                                                float* __restrict__ out) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    float* o = out + (size_t)Cn * p;
    const int fid = face_id[p];
    const float *a0 = nullptr, *a1 = nullptr, *a2 = nullptr;
    if (fid >= 0 && (unsigned)fid < F) {
        if (faces) {
            const int* f = faces + 3 * (size_t)fid;
            const int i0 = f[0], i1 = f[1], i2 = f[2];
            if ((unsigned)i0 < V && (unsigned)i1 < V && (unsigned)i2 < V) {
                a0 = attr + (size_t)Cn * i0; a1 = attr + (size_t)Cn * i1; a2 = attr + (size_t)Cn * i2;
            }
        } else {
            a0 = attr + (size_t)Cn * 3 * fid; a1 = a0 + Cn; a2 = a1 + Cn;
        }
    }
    if (!a0) {
        for (int c = 0; c < Cn; ++c) o[c] = fill;                                 // Cn <= 8
        return;
    }
    const float* w = bary + 3 * (size_t)p;
    const float w0 = w[0], w1 = w[1], w2 = w[2];
    for (int c = 0; c < Cn; ++c) o[c] = fmaf(w2, a2[c], fmaf(w1, a1[c], __fmul_rn(w0, a0[c])));      // Cn <= 8
}

// The rule of include/nerfart_hip.h (nerfart_mesh_sample_bilinear), step for step.  Every texel index is clamped into the image before it is used.
__global__ void __launch_bounds__(256) k_sample_bilinear(const float* __restrict__ uv, const unsigned char* __restrict__ mask,
                                                         const unsigned char* __restrict__ image, int Ht, int Wt, unsigned n, float bg0, float bg1,
                                                         float bg2, float* __restrict__ out) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    float* o = out + 3 * (size_t)p;
    const float u = uv[2 * (size_t)p], v = uv[2 * (size_t)p + 1];
    if ((mask && !mask[p]) || !isfinite(u) || !isfinite(v)) { o[0] = bg0; o[1] = bg1; o[2] = bg2; return; }
    const float X = __fsub_rn(u, 0.5f), Y = __fsub_rn(v, 0.5f);
    const float xf = fminf(fmaxf(floorf(X), -1.f), (float)Wt), yf = fminf(fmaxf(floorf(Y), -1.f), (float)Ht);       // the clamp makes the cast safe
    const float tx = fminf(fmaxf(__fsub_rn(X, xf), 0.f), 1.f), ty = fminf(fmaxf(__fsub_rn(Y, yf), 0.f), 1.f);
    const int xi = (int)xf, yi = (int)yf;
    const int xa = min(max(xi, 0), Wt - 1), xb = min(max(xi + 1, 0), Wt - 1), ya = min(max(yi, 0), Ht - 1), yb = min(max(yi + 1, 0), Ht - 1);
    const unsigned char *t00 = image + 3 * ((size_t)ya * Wt + xa), *t10 = image + 3 * ((size_t)ya * Wt + xb);
    const unsigned char *t01 = image + 3 * ((size_t)yb * Wt + xa), *t11 = image + 3 * ((size_t)yb * Wt + xb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float c00 = (float)t00[c], c10 = (float)t10[c], c01 = (float)t01[c], c11 = (float)t11[c];
        const float top = fmaf(tx, __fsub_rn(c10, c00), c00), bot = fmaf(tx, __fsub_rn(c11, c01), c01);
        o[c] = __fdiv_rn(fmaf(ty, __fsub_rn(bot, top), top), 255.f);
    }
}

static bool make_cam(const float* w2c, const float* rot, const float* K5, float near, Cam* C) {
    if (!K5) { set_last_error("mesh_raster: null camera pointer"); return false; }
    for (int k = 0; k < 12; ++k) C->w2c[k] = w2c ? w2c[k] : 0.f;
    for (int k = 0; k < 9; ++k) C->rot[k] = rot ? rot[k] : 0.f;
    C->fx = K5[0]; C->sk = K5[1]; C->cx = K5[2]; C->fy = K5[3]; C->cy = K5[4]; C->near = near;
    if (!(std::isfinite(C->fx) && std::isfinite(C->fy) && C->fx != 0.f && C->fy != 0.f && std::isfinite(C->sk) && std::isfinite(C->cx) &&
          std::isfinite(C->cy))) {
        set_last_error("mesh_raster: fx and fy must be finite and non-zero, sk, cx and cy finite");
        return false;
    }
    if (!(near > 0.f) || !std::isfinite(near)) { set_last_error("mesh_raster: near must be positive and finite"); return false; }
    return true;
}

static bool image_ok(int H, int W) {
    if (H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) { set_last_error("mesh_raster: H and W must be in 1 .. 16384"); return false; }
    return true;
}

}  // namespace mr
}  // namespace nerfart

using namespace nerfart;

extern "C" {

int nerfart_mesh_project(const float* verts, unsigned V, const float* w2c, const float* K5, float near, int* xy_fix, float* cam,
                         unsigned char* valid, void* stream) {
    mr::Cam C;
    if (!w2c) { set_last_error("mesh_project: null pointer"); return 2; }
    if (!mr::make_cam(w2c, nullptr, K5, near, &C)) return 2;
    if (V == 0) return 0;
    if (!verts || !xy_fix || !cam || !valid) { set_last_error("mesh_project: null pointer"); return 2; }
    if (V >= 2147483648u) { set_last_error("mesh_project: V must be below 2^31"); return 2; }
    hipLaunchKernelGGL(mr::k_project, dim3((V + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, verts, V, C, xy_fix, cam, valid);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mesh_raster(const int* xy_fix, const float* cam, const unsigned char* valid, const int* faces, unsigned V, unsigned F, const float* K5,
                        float near, int H, int W, unsigned long long* zbuf, int* list, int* info, void* stream) {
    mr::Cam C;
    if (!mr::make_cam(nullptr, nullptr, K5, near, &C) || !mr::image_ok(H, W)) return 2;
    if (!zbuf || !info || (F && (!faces || !list)) || (F && V && (!xy_fix || !cam || !valid))) { set_last_error("mesh_raster: null pointer"); return 2; }
    if (V >= 2147483648u || F >= 2147483648u) { set_last_error("mesh_raster: V and F must be below 2^31"); return 2; }
    NERFART_HIP(hipMemsetAsync(zbuf, 0xff, sizeof(unsigned long long) * (size_t)H * (size_t)W, (hipStream_t)stream));
    NERFART_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int), (hipStream_t)stream));
    if (F == 0) return 0;
    hipLaunchKernelGGL(mr::k_raster_small, dim3((F + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, xy_fix, cam, valid, faces, V, F, C, H, W, zbuf, list,
                       info);
    NERFART_HIP(hipGetLastError());
    hipLaunchKernelGGL(mr::k_raster_large, dim3(F < 1024u ? F : 1024u), dim3(256), 0, (hipStream_t)stream, xy_fix, cam, valid, faces, V, F, C, H, W, zbuf,
                       list, info);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mesh_resolve(const unsigned long long* zbuf, const float* cam, const int* faces, unsigned V, unsigned F, const float* K5, const float* rot,
                         int H, int W, int* face_id, float* bary, float* z, float* depth, unsigned char* mask, float* normals, void* stream) {
    mr::Cam C;
    if (!rot) { set_last_error("mesh_resolve: null pointer"); return 2; }
    if (!mr::make_cam(nullptr, rot, K5, 1.f, &C) || !mr::image_ok(H, W)) return 2;
    if (!zbuf || !face_id || !bary || !z || !depth || !mask || !normals || (F && (!faces || !cam))) { set_last_error("mesh_resolve: null pointer"); return 2; }
    hipLaunchKernelGGL(mr::k_resolve, dim3(((unsigned)W + 63u) / 64u, ((unsigned)H + 3u) / 4u), dim3(64, 4), 0, (hipStream_t)stream, zbuf, cam, faces, V, F,
                       C, H, W, face_id, bary, z, depth, mask, normals);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mesh_interp(const int* face_id, const float* bary, const int* faces, const float* attr, unsigned V, unsigned F, int C, unsigned n,
                        float fill, float* out, void* stream) {
    if (C < 1 || C > 8) { set_last_error("mesh_interp: C must be in 1 .. 8"); return 2; }
    if (n == 0) return 0;
    if (!face_id || !bary || !out || (F && !attr)) { set_last_error("mesh_interp: null pointer"); return 2; }
    if (n > 268435456u || F >= 268435456u) { set_last_error("mesh_interp: n must be at most 2^28 and F below 2^28"); return 2; }
    hipLaunchKernelGGL(mr::k_interp, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, face_id, bary, faces, attr, V, F, C, n, fill, out);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mesh_sample_bilinear(const float* uv, const unsigned char* mask, const unsigned char* image, int Ht, int Wt, unsigned n,
                                 const float* background, float* out, void* stream) {
    if (Ht < 1 || Wt < 1 || Ht > mr::MAX_SIDE || Wt > mr::MAX_SIDE) { set_last_error("mesh_sample_bilinear: the image sides must be in 1 .. 16384"); return 2; }
    if (n == 0) return 0;
    if (!uv || !image || !background || !out) { set_last_error("mesh_sample_bilinear: null pointer"); return 2; }
    hipLaunchKernelGGL(mr::k_sample_bilinear, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, uv, mask, image, Ht, Wt, n, background[0],
                       background[1], background[2], out);
    NERFART_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
