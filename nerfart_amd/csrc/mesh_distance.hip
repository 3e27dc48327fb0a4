// mesh_distance.hip - how far one surface is from another (mesh_util.sample_surface / closest_on_mesh / mesh_distance, tools/compare_mesh.py):
// area-weighted samples of an indexed mesh, and the exact closest point of a second mesh for each of them.  The rules are in
// include/nerfart_hip.h; the numpy statement is tests/mesh_distance_ref.py.
//
// SAMPLING  verts [V, 3] fp32, faces [F, 3] int32, density rho, a 32-bit seed.
//   k_ms_count     the first level of the exclusive scan (csrc/pair_scan.h) whose item f is (n_f, 1 if face f is bad): the area in fp64 in the
//                  header's order, n_f = floor(rho a_f + h(seed, f)).  The totals (n, bad faces) land in the workspace.
//   k_ms_check     one thread per face: an offset that is smaller than its predecessor, or a total of 2^31 or more, is a wrapped 32-bit sum and
//                  sets info[2]; thread 0 copies the totals to info.
//   (one host read of info)
//   k_ms_emit      one thread per sample i: its face by bisection of the offsets (at most 32 steps), j = i - off[f], the point in fp64.
// CLOSEST POINT  mesh B = (verts, faces), a grid (gx, gy, gz), query points [n, 3] fp32.
//   k_md_bbox      one thread per face: the box of the GOOD faces' vertices by integer atomicMin / atomicMax on the order-preserving encoding of
//                  the fp32 bits, reduced over the wave first (one atomic per wave and word); the good faces are counted the same way.
//   k_md_params    one thread: lo, cell size and its inverse per axis in fp64; an axis without extent has one cell.
//   k_md_total     one thread per face: the cells its box overlaps, summed in 64 bits (wave first) - the number of entries.
//   k_md_cells<0>  one thread per face: +1 on every cell it overlaps (integer atomicAdd).  With 2^31 entries or more it does nothing.
//   k_md_scan      exclusive scan of the cell counts.
//   (one host read of info = (entries, good faces))
//   k_md_cells<1>  one thread per face: list[off[cell] + cursor[cell]++] = f.  The order within a cell is free: the query takes a minimum.
//   k_md_closest   one thread per point (points in emit order are spatially coherent: neighbouring lanes walk the same cells): rings of growing
//                  Chebyshev radius around the point's clamped cell, the lexicographic minimum of (d^2, face) in fp64 registers, the stop rule
//                  of the header.  Every loop is bounded: rings by the grid's size, cells by the ring, entries by the cell's count.
//
// No float atomics; integer atomics only where the outcome does not depend on their order (min, max, sums, and cursors whose order is free).  No
// workgroup waits for another.  Every write is checked against the caller's sizes (n, entries).  This file is compiled without contraction: the
// fp64 expressions are evaluated as written, every operation rounded once.
#include "pair_scan.h"
#include <string>

#pragma clang fp contract(off)

namespace nerfart {
namespace md {

constexpr double TWO_M32 = 1.0 / 4294967296.0;
constexpr double REL_SLACK = 1.0 - 1.0 / 1048576.0;      // the stop bound is shrunk by 2^-20 of itself and by 2^-30 of the coordinates' size
constexpr double ABS_SLACK = 1.0 / 1073741824.0;
constexpr int GRID_MAX = 1024;                           // cells per axis
constexpr unsigned CELLS_MAX = 1u << 24;

// ---- the hashes (32-bit integer arithmetic, wrapping) ---------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__host__ __device__ __forceinline__ unsigned face_key(unsigned seed, unsigned f) { return mix32(mix32(seed) ^ mix32(f + 0x9e3779b9u)); }
__host__ __device__ __forceinline__ unsigned count_bits(unsigned key) { return mix32(key ^ 0x68e31da4u); }
__host__ __device__ __forceinline__ unsigned sample_state(unsigned key, unsigned j) { return mix32(key + 0x85ebca6bu * (j + 1u)); }
__host__ __device__ __forceinline__ unsigned u_bits(unsigned s) { return mix32(s ^ 0xb5297a4du); }
__host__ __device__ __forceinline__ unsigned v_bits(unsigned s) { return mix32(s ^ 0x1b56c4e9u); }

struct Tri { double a[3], b[3], c[3]; };

// the three vertices of face f in fp64; false for a bad face: an index outside [0, V) or a non-finite coordinate
__device__ __forceinline__ bool load_face(const float* __restrict__ verts, const int* __restrict__ faces, unsigned V, unsigned f, Tri& t) {
    const int* i = faces + 3 * (size_t)f;
    const unsigned ia = (unsigned)i[0], ib = (unsigned)i[1], ic = (unsigned)i[2];       // a negative index is >= 2^31 > V as unsigned
    if (ia >= V || ib >= V || ic >= V) return false;
    const float* pa = verts + 3 * (size_t)ia;
    const float* pb = verts + 3 * (size_t)ib;
    const float* pc = verts + 3 * (size_t)ic;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = pa[k], y = pb[k], z = pc[k];
        fin = fin && isfinite(x) && isfinite(y) && isfinite(z);
        t.a[k] = (double)x; t.b[k] = (double)y; t.c[k] = (double)z;
    }
    return fin;
}

// ---- sampling --------------------------------------------------------------------------------------------------------------------------------
struct SampleWs {
    unsigned* off;            // [max(F, 1)][2] (offset of the face's first sample, bad faces before it): FIRST in the workspace, the header says so
    PairScanLevels lvl;
    unsigned* tot;            // [2] (n, bad faces)
    size_t n, bytes;
};
static SampleWs carve_sample(void* base, unsigned F) {
    SampleWs w{};
    Carver c(base);
    w.n = F ? F : 1;
    w.off = c.take<unsigned>(2 * w.n);
    pair_scan_carve(c, w.n, w.lvl);
    w.tot = c.take<unsigned>(2);
    w.bytes = c.off;
    return w;
}

// a_f = 0.5 sqrt(n . n), n = (b - a) x (c - a): the header's order
__device__ __forceinline__ double face_area(const Tri& t) {
    const double ux = t.b[0] - t.a[0], uy = t.b[1] - t.a[1], uz = t.b[2] - t.a[2];
    const double wx = t.c[0] - t.a[0], wy = t.c[1] - t.a[1], wz = t.c[2] - t.a[2];
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    return 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
}

__global__ void __launch_bounds__(256) k_ms_count(const float* __restrict__ verts, const int* __restrict__ faces, unsigned V, unsigned F, double rho,
                                                  unsigned seed, uint2* __restrict__ off, unsigned n, uint2* __restrict__ sums,
                                                  unsigned* __restrict__ info) {
    pair_scan_block([&](size_t i) {
        if (i >= F) return make_uint2(0u, 0u);
        Tri t;
        if (!load_face(verts, faces, V, (unsigned)i, t)) return make_uint2(0u, 1u);
        const double x = rho * face_area(t) + (double)count_bits(face_key(seed, (unsigned)i)) * TWO_M32;
        if (!(x < 2147483648.0)) { info[2] = 1u; return make_uint2(0u, 0u); }     // more samples than an index holds: none, and the flag
        return make_uint2((unsigned)x, 0u);                                         // x >= 0: the conversion truncates = floor
    }, off, n, sums);
}

__global__ void __launch_bounds__(256) k_ms_check(const uint2* __restrict__ off, unsigned F, const unsigned* __restrict__ tot, unsigned* __restrict__ info) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f == 0) { info[0] = tot[0]; info[1] = tot[1]; if (tot[0] >= 2147483648u) info[2] = 1u; }
    if (f >= F) return;
    const unsigned next = f + 1 < F ? off[f + 1].x : tot[0];
    if (next < off[f].x) info[2] = 1u;                   // every n_f < 2^31: the first wrap of the running sum shows as a decrease
}

__global__ void __launch_bounds__(256) k_ms_emit(const float* __restrict__ verts, const int* __restrict__ faces, unsigned V, unsigned F, unsigned seed,
                                                 const uint2* __restrict__ off, const unsigned* __restrict__ tot, float* __restrict__ points,
                                                 int* __restrict__ face, unsigned n) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float* o = points + 3 * (size_t)i;
    Tri t;
    unsigned lo = 0, hi = F;                             // the last f with off[f] <= i; off[0] = 0, so lo >= 1 at the end
    // BOUND: 32 steps (hi - lo halves)
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (off[mid].x <= i) lo = mid + 1; else hi = mid;
    }
    const unsigned f = lo ? lo - 1 : 0;
    if (i >= tot[0] || !load_face(verts, faces, V, f, t)) {          // not a sample of this workspace: written, as nothing
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; face[i] = -1;
        return;
    }
    const unsigned s = sample_state(face_key(seed, f), i - off[f].x);
    double u = (double)u_bits(s) * TWO_M32, v = (double)v_bits(s) * TWO_M32;
    if (u + v > 1.0) { u = 1.0 - u; v = 1.0 - v; }       // the other half of the parallelogram, reflected into the triangle
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (float)((t.a[k] + u * (t.b[k] - t.a[k])) + v * (t.c[k] - t.a[k]));
    face[i] = (int)f;
}

// ---- the grid --------------------------------------------------------------------------------------------------------------------------------
struct GridParams {
    double lo[3], s[3], inv[3], slack;
    int g[3];                 // the cells per axis in use: the caller's, or 1 on an axis without extent (and on every axis without a good face)
    unsigned good;
};
struct GridWs {
    GridParams* par;
    unsigned* box;            // [8]: min x y z, max x y z (encoded), good faces, -
    unsigned* tot;            // [2] the scan's totals
    unsigned long long* ent;  // [1] the entries, in 64 bits
    unsigned* off;            // [L][2]
    PairScanLevels lvl;
    unsigned* cnt;            // [L]
    unsigned* cur;            // [L]
    size_t L, bytes;
};
static GridWs carve_grid(void* base, size_t L) {
    GridWs w{};
    Carver c(base);
    w.L = L;
    w.par = c.take<GridParams>(1);
    w.box = c.take<unsigned>(8);
    w.tot = c.take<unsigned>(2);
    w.ent = c.take<unsigned long long>(1);
    w.off = c.take<unsigned>(2 * L);
    pair_scan_carve(c, L, w.lvl);
    w.cnt = c.take<unsigned>(L);
    w.cur = c.take<unsigned>(L);
    w.bytes = c.off;
    return w;
}

// fp32 bits -> unsigned that orders as the floats do (finite values), and back
__device__ __forceinline__ unsigned enc(float x) { const unsigned b = __float_as_uint(x); return b & 0x80000000u ? ~b : b | 0x80000000u; }
__device__ __forceinline__ float dec(unsigned e) { return __uint_as_float(e & 0x80000000u ? e & 0x7fffffffu : ~e); }

__device__ __forceinline__ unsigned wave_min(unsigned x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned y = __shfl_xor(x, d, 64); x = y < x ? y : x; }
    return x;
}
__device__ __forceinline__ unsigned wave_max(unsigned x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned y = __shfl_xor(x, d, 64); x = y > x ? y : x; }
    return x;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

__global__ void __launch_bounds__(256) k_md_bbox(const float* __restrict__ verts, const int* __restrict__ faces, unsigned V, unsigned F, unsigned* box) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    unsigned long long good = 0;
    Tri t;
    if (f < F && load_face(verts, faces, V, f, t)) {
        good = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned ea = enc((float)t.a[k]), eb = enc((float)t.b[k]), ec = enc((float)t.c[k]);      // exact: they were fp32
            mn[k] = min(ea, min(eb, ec));
            mx[k] = max(ea, max(eb, ec));
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { mn[k] = wave_min(mn[k]); mx[k] = wave_max(mx[k]); }     // every lane of the wave takes part
    good = wave_sum(good);
    if ((threadIdx.x & 63) == 0 && good) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(box + k, mn[k]); atomicMax(box + 3 + k, mx[k]); }
        atomicAdd(box + 6, (unsigned)good);
    }
}

__global__ void k_md_params(const unsigned* __restrict__ box, int gx, int gy, int gz, GridParams* __restrict__ par, unsigned long long* __restrict__ info) {
    if (blockIdx.x || threadIdx.x) return;
    const int g[3] = {gx, gy, gz};
    GridParams p;
    p.good = box[6];
    double size = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double lo = p.good ? (double)dec(box[k]) : 0.0, hi = p.good ? (double)dec(box[3 + k]) : 0.0;
        const double ext = hi - lo;
        const bool flat = !(ext > 0.0);
        p.lo[k] = lo;
        p.g[k] = flat ? 1 : g[k];
        p.s[k] = flat ? 0.0 : ext / (double)g[k];
        p.inv[k] = flat ? 0.0 : (double)g[k] / ext;
        size = fmax(size, fmax(fabs(lo), fabs(hi)));
    }
    p.slack = ABS_SLACK * size;
    *par = p;
    info[1] = p.good;
}

// the cell of coordinate x on axis k: monotone in x, clamped into the grid (a NaN goes to cell 0)
__device__ __forceinline__ int axis_cell(const GridParams& p, int k, double x) {
    const double t = floor((x - p.lo[k]) * p.inv[k]);
    return (int)fmin(fmax(t, 0.0), (double)(p.g[k] - 1));
}

// the cells the box of a good face overlaps: [c0, c1] per axis
__device__ __forceinline__ void face_cells(const GridParams& p, const Tri& t, int c0[3], int c1[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c0[k] = axis_cell(p, k, fmin(t.a[k], fmin(t.b[k], t.c[k])));
        c1[k] = axis_cell(p, k, fmax(t.a[k], fmax(t.b[k], t.c[k])));
    }
}

__global__ void __launch_bounds__(256) k_md_total(const float* __restrict__ verts, const int* __restrict__ faces, unsigned V, unsigned F,
                                                  const GridParams* __restrict__ par, unsigned long long* ent) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    unsigned long long mine = 0;
    Tri t;
    if (f < F && load_face(verts, faces, V, f, t)) {
        const GridParams p = *par;
        int c0[3], c1[3];
        face_cells(p, t, c0, c1);
        mine = (unsigned long long)(c1[0] - c0[0] + 1) * (unsigned long long)(c1[1] - c0[1] + 1) * (unsigned long long)(c1[2] - c0[2] + 1);
    }
    mine = wave_sum(mine);                               // at most 2^24 cells per face, F < 2^31 faces: below 2^55
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(ent, mine);
}

// fill == false: counts; fill == true: writes the face into its cells' lists through the cursors
template <bool fill>
__global__ void __launch_bounds__(256) k_md_cells(const float* __restrict__ verts, const int* __restrict__ faces, unsigned V, unsigned F,
                                                  const GridParams* __restrict__ par, const unsigned long long* __restrict__ ent, unsigned* cnt,
                                                  const uint2* __restrict__ off, int* __restrict__ list, unsigned entries) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F || ent[0] >= 2147483648ull) return;       // too many entries: refused by the host after its read
    Tri t;
    if (!load_face(verts, faces, V, f, t)) return;
    const GridParams p = *par;
    int c0[3], c1[3];
    face_cells(p, t, c0, c1);
    // BOUND: the face's cells, at most the grid's
    for (int x = c0[0]; x <= c1[0]; ++x)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int z = c0[2]; z <= c1[2]; ++z) {
                const size_t q = ((size_t)x * p.g[1] + y) * p.g[2] + z;
                const unsigned at = atomicAdd(cnt + q, 1u);
                if (fill) {
                    const unsigned long long e = (unsigned long long)off[q].x + at;
                    if (e < entries) list[e] = (int)f;
                }
            }
}

__global__ void __launch_bounds__(256) k_md_scan(const unsigned* __restrict__ cnt, uint2* __restrict__ off, unsigned L, uint2* __restrict__ sums) {
    pair_scan_block([&](size_t i) { const unsigned c = cnt[i]; return make_uint2(c, c ? 1u : 0u); }, off, L, sums);
}

// ---- the narrow phase ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// squared distance from p to the segment a + t e, t in [0, 1], given w = p - a
__device__ __forceinline__ double segment_d2(double wx, double wy, double wz, double ex, double ey, double ez) {
    const double ee = dot3(ex, ey, ez, ex, ey, ez);
    double t = 0.0;
    if (ee > 0.0) t = fmin(fmax(dot3(wx, wy, wz, ex, ey, ez) / ee, 0.0), 1.0);
    const double qx = wx - t * ex, qy = wy - t * ey, qz = wz - t * ez;
    return dot3(qx, qy, qz, qx, qy, qz);
}

__device__ __forceinline__ double face_d2(const double p[3], const Tri& t) {
    const double ux = t.b[0] - t.a[0], uy = t.b[1] - t.a[1], uz = t.b[2] - t.a[2];        // b - a
    const double vx = t.c[0] - t.b[0], vy = t.c[1] - t.b[1], vz = t.c[2] - t.b[2];        // c - b
    const double sx = t.a[0] - t.c[0], sy = t.a[1] - t.c[1], sz = t.a[2] - t.c[2];        // a - c
    const double wax = p[0] - t.a[0], way = p[1] - t.a[1], waz = p[2] - t.a[2];
    const double wbx = p[0] - t.b[0], wby = p[1] - t.b[1], wbz = p[2] - t.b[2];
    const double wcx = p[0] - t.c[0], wcy = p[1] - t.c[1], wcz = p[2] - t.c[2];
    double d2 = fmin(segment_d2(wax, way, waz, ux, uy, uz), fmin(segment_d2(wbx, wby, wbz, vx, vy, vz), segment_d2(wcx, wcy, wcz, sx, sy, sz)));
    const double ex = t.c[0] - t.a[0], ey = t.c[1] - t.a[1], ez = t.c[2] - t.a[2];        // c - a
    const double nx = uy * ez - uz * ey, ny = uz * ex - ux * ez, nz = ux * ey - uy * ex;
    const double nn = dot3(nx, ny, nz, nx, ny, nz);
    if (nn > 0.0) {
        const double e0 = dot3(nx, ny, nz, uy * waz - uz * way, uz * wax - ux * waz, ux * way - uy * wax);
        const double e1 = dot3(nx, ny, nz, vy * wbz - vz * wby, vz * wbx - vx * wbz, vx * wby - vy * wbx);
        const double e2 = dot3(nx, ny, nz, sy * wcz - sz * wcy, sz * wcx - sx * wcz, sx * wcy - sy * wcx);
        if (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) {
            const double h = dot3(nx, ny, nz, wax, way, waz);
            d2 = fmin(d2, h * h / nn);
        }
    }
    return d2;
}

__global__ void __launch_bounds__(256) k_md_closest(const float* __restrict__ points, unsigned n, const float* __restrict__ verts,
                                                    const int* __restrict__ faces, unsigned V, unsigned F, const GridParams* __restrict__ par,
                                                    const uint2* __restrict__ off, const unsigned* __restrict__ cnt, const int* __restrict__ list,
                                                    unsigned entries, double maxd, float* __restrict__ dist, int* __restrict__ face,
                                                    unsigned* __restrict__ visited) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* q = points + 3 * (size_t)i;
    const float fx = q[0], fy = q[1], fz = q[2];
    if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) {
        dist[i] = __uint_as_float(0x7fc00000u); face[i] = -1;
        if (visited) visited[i] = 0u;
        return;
    }
    const GridParams g = *par;
    const double p[3] = {(double)fx, (double)fy, (double)fz};
    int c[3], R = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = axis_cell(g, k, p[k]);
        R = max(R, max(c[k], g.g[k] - 1 - c[k]));
    }
    const double slack = g.slack + ABS_SLACK * fmax(fabs(p[0]), fmax(fabs(p[1]), fabs(p[2])));
    double best = __longlong_as_double(0x7ff0000000000000ll);
    int best_f = -1;
    unsigned tested = 0;
    // BOUND: R + 1 <= 1024 rings; a ring's cells; a cell's entries
    for (int r = 0; r <= R; ++r) {
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.g[0] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.g[1] - 1);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.g[2] - 1);
        for (int x = x0; x <= x1; ++x) {
            for (int y = y0; y <= y1; ++y) {
                // a column of the box: whole on the ring's four x / y sides, otherwise its two ends
                const bool side = x == c[0] - r || x == c[0] + r || y == c[1] - r || y == c[1] + r;
                const int zs = side ? z0 : c[2] - r, ze = side ? z1 : c[2] + r, dz = side ? 1 : 2 * r;      // not side: r >= 1
                for (int z = zs; z <= ze; z += dz) {
                    if (z < 0 || z >= g.g[2]) continue;
                    const size_t cell = ((size_t)x * g.g[1] + y) * g.g[2] + z;
                    const unsigned m = cnt[cell];
                    if (!m) continue;
                    const unsigned start = off[cell].x;
                    for (unsigned e = 0; e < m; ++e) {
                        const unsigned long long at = (unsigned long long)start + e;
                        if (at >= entries) break;
                        const unsigned f = (unsigned)list[at];
                        Tri t;
                        if (f >= F || !load_face(verts, faces, V, f, t)) continue;
                        ++tested;
                        const double d2 = face_d2(p, t);
                        if (d2 < best || (d2 == best && (int)f < best_f)) { best = d2; best_f = (int)f; }
                    }
                }
            }
        }
        // everything not yet visited lies beyond the visited box: at least as far as the nearest of its sides that is not the grid's own
        double b = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (c[k] - r > 0) b = fmin(b, p[k] - (g.lo[k] + (double)(c[k] - r) * g.s[k]));
            if (c[k] + r < g.g[k] - 1) b = fmin(b, (g.lo[k] + (double)(c[k] + r + 1) * g.s[k]) - p[k]);
        }
        b = fmax(b * REL_SLACK - slack, 0.0);
        if (fmin(sqrt(best), maxd) < b) break;           // strictly: a tie with an unvisited face must still be seen
    }
    const double d = sqrt(best);
    const bool found = best_f >= 0 && d <= maxd;
    dist[i] = (float)(found ? d : maxd);
    face[i] = found ? best_f : -1;
    if (visited) visited[i] = tested;
}

static dim3 blocks256(unsigned n) { return dim3((unsigned)(((size_t)n + 255) / 256)); }

static int refuse(const char* who, const char* what) {
    set_last_error((std::string(who) + ": " + what).c_str());
    return 2;
}
static int check_mesh(const char* who, unsigned V, unsigned F) {
    if (V >= 2147483648u || F >= 2147483648u) return refuse(who, "V and F must stay below 2^31");
    return 0;
}
static int check_grid(const char* who, int gx, int gy, int gz, size_t& L) {
    if (gx < 1 || gy < 1 || gz < 1 || gx > GRID_MAX || gy > GRID_MAX || gz > GRID_MAX) return refuse(who, "every grid dimension must be in 1 .. 1024");
    L = (size_t)gx * gy * gz;
    if (L > CELLS_MAX) return refuse(who, "the grid must have at most 2^24 cells");
    return 0;
}
static int check_ws(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (!ws) return refuse(who, "null pointer");
    if (ws_bytes < need || ((size_t)ws & 15)) return refuse(who, "workspace smaller than its *_workspace_bytes() or not 16-byte aligned");
    return 0;
}

}  // namespace md
}  // namespace nerfart

using namespace nerfart;

extern "C" {

size_t nerfart_mesh_sample_workspace_bytes(unsigned F) {
    if (md::check_mesh("mesh_sample_workspace_bytes", 0, F)) return 0;
    return md::carve_sample(nullptr, F).bytes;
}

int nerfart_mesh_sample_count(const float* verts, const int* faces, unsigned V, unsigned F, double density, unsigned seed, void* ws, size_t ws_bytes,
                              unsigned* info, void* stream) {
    const char* who = "mesh_sample_count";
    if (!info || (F && !faces) || (V && !verts)) return md::refuse(who, "null pointer");
    if ((size_t)info & 7) return md::refuse(who, "info must be 8-byte aligned");
    if (int rc = md::check_mesh(who, V, F)) return rc;
    if (!(density >= 0.0) || !(density < __builtin_inf())) return md::refuse(who, "the density must be finite and not negative");
    if (int rc = md::check_ws(who, ws, ws_bytes, md::carve_sample(nullptr, F).bytes)) return rc;
    const md::SampleWs w = md::carve_sample(ws, F);
    hipStream_t st = (hipStream_t)stream;
    NERFART_HIP(hipMemsetAsync(info, 0, 4 * sizeof(unsigned), st));
    hipLaunchKernelGGL(md::k_ms_count, pair_scan_blocks((unsigned)w.n), dim3(256), 0, st, verts, faces, V, F, density, seed, (uint2*)w.off, (unsigned)w.n,
                       pair_scan_sums(w.lvl, 0, w.tot), info);
    NERFART_HIP(hipGetLastError());
    if (int rc = pair_scan_finish(w.off, (unsigned)w.n, w.lvl, w.tot, st)) return rc;
    hipLaunchKernelGGL(md::k_ms_check, md::blocks256((unsigned)w.n), dim3(256), 0, st, (const uint2*)w.off, F, (const unsigned*)w.tot, info);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mesh_sample_emit(const float* verts, const int* faces, unsigned V, unsigned F, unsigned seed, const void* ws, size_t ws_bytes, float* points,
                             int* face, unsigned n, void* stream) {
    const char* who = "mesh_sample_emit";
    if ((F && !faces) || (V && !verts) || (n && (!points || !face))) return md::refuse(who, "null pointer");
    if (int rc = md::check_mesh(who, V, F)) return rc;
    if (n >= 2147483648u) return md::refuse(who, "n must stay below 2^31");
    if (int rc = md::check_ws(who, ws, ws_bytes, md::carve_sample(nullptr, F).bytes)) return rc;
    if (!n) return 0;
    if (!F) return md::refuse(who, "a mesh without faces has no samples (n must be 0)");
    const md::SampleWs w = md::carve_sample(const_cast<void*>(ws), F);
    hipLaunchKernelGGL(md::k_ms_emit, md::blocks256(n), dim3(256), 0, (hipStream_t)stream, verts, faces, V, F, seed, (const uint2*)w.off,
                       (const unsigned*)w.tot, points, face, n);
    NERFART_HIP(hipGetLastError());
    return 0;
}

size_t nerfart_mesh_grid_workspace_bytes(int gx, int gy, int gz) {
    size_t L;
    if (md::check_grid("mesh_grid_workspace_bytes", gx, gy, gz, L)) return 0;
    return md::carve_grid(nullptr, L).bytes;
}

int nerfart_mesh_grid_count(const float* verts, const int* faces, unsigned V, unsigned F, int gx, int gy, int gz, void* ws, size_t ws_bytes,
                            unsigned long long* info, void* stream) {
    const char* who = "mesh_grid_count";
    if (!info || (F && !faces) || (V && !verts)) return md::refuse(who, "null pointer");
    if ((size_t)info & 7) return md::refuse(who, "info must be 8-byte aligned");
    if (int rc = md::check_mesh(who, V, F)) return rc;
    size_t L;
    if (int rc = md::check_grid(who, gx, gy, gz, L)) return rc;
    if (int rc = md::check_ws(who, ws, ws_bytes, md::carve_grid(nullptr, L).bytes)) return rc;
    const md::GridWs w = md::carve_grid(ws, L);
    hipStream_t st = (hipStream_t)stream;
    NERFART_HIP(hipMemsetAsync(info, 0, 2 * sizeof(unsigned long long), st));
    NERFART_HIP(hipMemsetAsync(w.box, 0xff, 3 * sizeof(unsigned), st));
    NERFART_HIP(hipMemsetAsync(w.box + 3, 0, 5 * sizeof(unsigned), st));
    NERFART_HIP(hipMemsetAsync(w.cnt, 0, sizeof(unsigned) * L, st));
    NERFART_HIP(hipMemsetAsync(w.ent, 0, sizeof(unsigned long long), st));
    if (F) {
        hipLaunchKernelGGL(md::k_md_bbox, md::blocks256(F), dim3(256), 0, st, verts, faces, V, F, w.box);
        NERFART_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(md::k_md_params, dim3(1), dim3(64), 0, st, (const unsigned*)w.box, gx, gy, gz, w.par, info);
    NERFART_HIP(hipGetLastError());
    if (F) {
        hipLaunchKernelGGL(md::k_md_total, md::blocks256(F), dim3(256), 0, st, verts, faces, V, F, (const md::GridParams*)w.par, w.ent);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(md::k_md_cells<false>, md::blocks256(F), dim3(256), 0, st, verts, faces, V, F, (const md::GridParams*)w.par,
                           (const unsigned long long*)w.ent, w.cnt, (const uint2*)nullptr, (int*)nullptr, 0u);
        NERFART_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(md::k_md_scan, pair_scan_blocks((unsigned)L), dim3(256), 0, st, (const unsigned*)w.cnt, (uint2*)w.off, (unsigned)L,
                       pair_scan_sums(w.lvl, 0, w.tot));
    NERFART_HIP(hipGetLastError());
    if (int rc = pair_scan_finish(w.off, (unsigned)L, w.lvl, w.tot, st)) return rc;
    NERFART_HIP(hipMemcpyAsync(info, w.ent, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    return 0;
}

int nerfart_mesh_grid_fill(const float* verts, const int* faces, unsigned V, unsigned F, int gx, int gy, int gz, void* ws, size_t ws_bytes, int* list,
                           unsigned long long entries, void* stream) {
    const char* who = "mesh_grid_fill";
    if ((F && !faces) || (V && !verts) || (entries && !list)) return md::refuse(who, "null pointer");
    if (int rc = md::check_mesh(who, V, F)) return rc;
    if (entries >= 2147483648ull) return md::refuse(who, "2^31 entries or more: use a coarser grid");
    size_t L;
    if (int rc = md::check_grid(who, gx, gy, gz, L)) return rc;
    if (int rc = md::check_ws(who, ws, ws_bytes, md::carve_grid(nullptr, L).bytes)) return rc;
    if (!entries || !F) return 0;
    const md::GridWs w = md::carve_grid(ws, L);
    hipStream_t st = (hipStream_t)stream;
    NERFART_HIP(hipMemsetAsync(w.cur, 0, sizeof(unsigned) * L, st));
    hipLaunchKernelGGL(md::k_md_cells<true>, md::blocks256(F), dim3(256), 0, st, verts, faces, V, F, (const md::GridParams*)w.par,
                       (const unsigned long long*)w.ent, w.cur, (const uint2*)w.off, list, (unsigned)entries);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mesh_closest(const float* points, unsigned n, const float* verts, const int* faces, unsigned V, unsigned F, int gx, int gy, int gz,
                         const void* ws, size_t ws_bytes, const int* list, unsigned long long entries, double max_distance, float* dist, int* face,
                         unsigned* visited, void* stream) {
    const char* who = "mesh_closest";
    if ((n && (!points || !dist || !face)) || (F && !faces) || (V && !verts) || (entries && !list)) return md::refuse(who, "null pointer");
    if (int rc = md::check_mesh(who, V, F)) return rc;
    if (n >= 2147483648u) return md::refuse(who, "n must stay below 2^31");
    if (entries >= 2147483648ull) return md::refuse(who, "2^31 entries or more: use a coarser grid");
    if (!(max_distance >= 0.0)) return md::refuse(who, "max_distance must be >= 0 (infinity allowed)");
    size_t L;
    if (int rc = md::check_grid(who, gx, gy, gz, L)) return rc;
    if (int rc = md::check_ws(who, ws, ws_bytes, md::carve_grid(nullptr, L).bytes)) return rc;
    if (!n) return 0;
    const md::GridWs w = md::carve_grid(const_cast<void*>(ws), L);
    hipLaunchKernelGGL(md::k_md_closest, md::blocks256(n), dim3(256), 0, (hipStream_t)stream, points, n, verts, faces, V, F,
                       (const md::GridParams*)w.par, (const uint2*)w.off, (const unsigned*)w.cnt, list, (unsigned)entries, max_distance, dist, face,
                       visited);
    NERFART_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
