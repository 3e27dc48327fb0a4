// marching_cubes.hip - isosurface extraction from the SDF volume (the reference's utils/mesh_util.py:112 hands the grid to
// skimage.measure.marching_cubes on the host): classify, scan, emit on the device, the volume never leaves the GPU.
//
// vol[nx][ny][nz] fp32, z fastest.  A corner is inside iff value < level.  Every mesh vertex lies on a grid edge; grid point p OWNS its three
// edges toward +x, +y, +z.  Corner / cube-edge numbering and the case table: nerfart_amd/mc_table.py (mc_table.h is generated from it).
//   k_mc_classify  one thread per grid point, lanes along z: byte 1 = which owned edges change sign (bit axis), byte 2 = the case index of the
//                  cell whose origin the point is (0 for the points of the last layers, which are no cell origin); a flag for non-finite values.
//   k_mc_scan      exclusive scan of (vertices per point 0..3, triangles per cell) over all points in linear order: per 512-item block
//                  (wave64 shuffles + LDS) with block sums, the same scan on the block sums until one block is left, an add-back on the
//                  way down (csrc/pair_scan.h, shared with csrc/mesh_components.hip).  Every kernel runs to completion on its own: no
//                  workgroup ever waits for another.
//   k_mc_emit      a point writes its vertices at its scanned offset in axis order; a cell writes its triangles at its scanned offset in table
//                  order, a vertex index being the owner's scanned offset + the rank of the edge among the owner's flagged edges.  No atomics:
//                  the output is a pure function of the volume, so two runs are bit-identical.  Every write is checked against V / F.
//   k_mc_emit_edges  the same walk, writing per vertex which grid edge it sits on and the initial state of the vertex refinement
//                  (csrc/mesh_vertices.hip) instead of a position.
#include "pair_scan.h"
#include <cmath>
#include <string>
#define MC_TABLE_DECL static __device__ const
#include "mc_table.h"

namespace nerfart {

constexpr int MC_TILE_Z = 64, MC_TILE_Y = 4;       // a 256-thread block covers 64 points along z (one wave = one coalesced row) x 4 rows
constexpr int MC_X_CHUNK = 8;            // ... and, in k_mc_classify, 8 slabs along x, carrying the shared slab in registers

// the workspace, carved in this order (each buffer rounded up to 256 bytes): flags [n] bytes, cases [n] bytes, off [n][2] (vertex offset,
// triangle offset), then per block-sum level k its [m_k][2] sums, m_0 = ceil(n / 512), m_{k+1} = ceil(m_k / 512), while m_k > 1
struct McWorkspace {
    unsigned char *flags, *cases;
    unsigned* off;
    PairScanLevels lvl;
    size_t bytes;
};
static McWorkspace mc_carve(void* base, size_t n) {
    McWorkspace w{};
    Carver c(base);
    w.flags = c.take<unsigned char>(n);
    w.cases = c.take<unsigned char>(n);
    w.off = c.take<unsigned>(2 * n);
    pair_scan_carve(c, n, w.lvl);
    w.bytes = c.off;
    return w;
}

// bit i of a nibble -> bit 2 i
__device__ __forceinline__ unsigned mc_spread(unsigned n) { return (n & 1u) | ((n & 2u) << 1) | ((n & 4u) << 2) | ((n & 8u) << 3); }

// block b of the 1-D grid -> (x tile, y tile, z tile)
__device__ __forceinline__ void mc_tile(int by, int bz, int& tx, int& ty, int& tz) {
    int b = blockIdx.x;
    tz = b % bz; b /= bz;
    ty = b % by; tx = b / by;
}

// Each thread walks MC_X_CHUNK slabs at its (y, z).  Per slab it loads the four values at (y, z), (y + 1, z), (y, z + 1), (y + 1, z + 1) - rows
// its own block's neighbouring lanes / waves load too, so three of the four are EXPECTED to come out of the vector cache (what the memory
// system did with them is in DESIGN.md 4.7, as far as it was measured) - and keeps their inside bits for the next slab.  Indices past the volume are clamped to the point itself (never read out of bounds); the bits they give are masked.
__global__ void __launch_bounds__(256) k_mc_classify(const float* __restrict__ vol, int nx, int ny, int nz, float level, int by, int bz,
                                                     unsigned char* __restrict__ flags, unsigned char* __restrict__ cases, unsigned* __restrict__ nonfinite) {
    int tx, ty, tz;
    mc_tile(by, bz, tx, ty, tz);
    const int z = tz * MC_TILE_Z + (threadIdx.x & 63), y = ty * MC_TILE_Y + (threadIdx.x >> 6);
    if (z >= nz || y >= ny) return;
    const int x0 = tx * MC_X_CHUNK, x1 = min(x0 + MC_X_CHUNK, nx);
    const bool hy = y + 1 < ny, hz = z + 1 < nz;
    const size_t sx = (size_t)ny * nz;
    const size_t o00 = (size_t)y * nz + z, o10 = o00 + (hy ? nz : 0), o01 = o00 + (hz ? 1 : 0), o11 = o10 + (hz ? 1 : 0);
    bool bad = false;
    auto slab = [&](int x) -> unsigned {       // bit 0 (y, z), bit 1 (y + 1, z), bit 2 (y, z + 1), bit 3 (y + 1, z + 1)
        const float* p = vol + (size_t)x * sx;
        const float v00 = p[o00], v10 = p[o10], v01 = p[o01], v11 = p[o11];
        bad |= !isfinite(v00);
        return (unsigned)(v00 < level) | ((unsigned)(v10 < level) << 1) | ((unsigned)(v01 < level) << 2) | ((unsigned)(v11 < level) << 3);
    };
    unsigned cur = slab(x0);
    for (int x = x0; x < x1; ++x) {
        const bool hx = x + 1 < nx;
        const unsigned nxt = hx ? slab(x + 1) : cur;      // slab x1 is classified by the next block: only its own-point finiteness is rechecked there
        const unsigned own = cur & 1u;
        unsigned f = 0;
        if (hx) f |= own ^ (nxt & 1u);
        if (hy) f |= (own ^ ((cur >> 1) & 1u)) << 1;
        if (hz) f |= (own ^ ((cur >> 2) & 1u)) << 2;
        const unsigned c = (hx && hy && hz) ? (mc_spread(cur) | (mc_spread(nxt) << 1)) : 0u;      // corner dx + 2 dy + 4 dz
        const size_t p = (size_t)x * sx + o00;
        flags[p] = (unsigned char)f;
        cases[p] = (unsigned char)c;
        cur = nxt;
    }
    if (bad) *nonfinite = 1u;
}

// The first level of the scan (csrc/pair_scan.h): the items are (vertices of point i, triangles of cell i) read from the classify bytes.
__global__ void __launch_bounds__(256) k_mc_scan(const unsigned char* __restrict__ flags, const unsigned char* __restrict__ cases, uint2* __restrict__ off,
                                                 unsigned n, uint2* __restrict__ sums) {
    pair_scan_block([&](size_t i) { return make_uint2(__popc(flags[i] & 7u), mc_tri_count[cases[i]]); }, off, n, sums);
}

struct McFrame { float o[3], s[3]; };

// One thread per grid point (the tile of k_mc_classify, one slab).  The bytes and offsets come from the caller's workspace: a cell is emitted
// only where it IS a cell and an edge only where its far end exists, so a workspace that does not belong to this volume can give a wrong mesh but
// no read or write outside the buffers.
__global__ void __launch_bounds__(256) k_mc_emit(const float* __restrict__ vol, int nx, int ny, int nz, float level, int by, int bz, McFrame fr,
                                                 const unsigned char* __restrict__ flags, const unsigned char* __restrict__ cases,
                                                 const uint2* __restrict__ off, float* __restrict__ verts, int* __restrict__ faces, unsigned V, unsigned F) {
    int x, ty, tz;
    mc_tile(by, bz, x, ty, tz);
    const int z = tz * MC_TILE_Z + (threadIdx.x & 63), y = ty * MC_TILE_Y + (threadIdx.x >> 6);
    if (z >= nz || y >= ny) return;
    const size_t stride[3] = {(size_t)ny * nz, (size_t)nz, 1};
    const size_t p = (size_t)x * stride[0] + (size_t)y * stride[1] + z;
    const unsigned f = flags[p] & 7u, c = cases[p];
    if (!(f | c)) return;
    const uint2 o = off[p];
    const int idx[3] = {x, y, z}, dim[3] = {nx, ny, nz};
    if (f) {
        const float a = vol[p];
        float pa[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) pa[ax] = fmaf((float)idx[ax], fr.s[ax], fr.o[ax]);        // one rounding
        unsigned vi = o.x;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!((f >> ax) & 1u)) continue;
            if (idx[ax] + 1 < dim[ax] && vi < V) {
                const float b = vol[p + stride[ax]];
                const float t = (level - a) / (b - a);
                const float pb = fmaf((float)(idx[ax] + 1), fr.s[ax], fr.o[ax]);
                float q[3] = {pa[0], pa[1], pa[2]};
                q[ax] = fmaf(t, pb - pa[ax], pa[ax]);
                float* out = verts + 3 * (size_t)vi;
                out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
            }
            ++vi;
        }
    }
    const unsigned nt = mc_tri_count[c];
    if (nt == 0 || x + 1 >= nx || y + 1 >= ny || z + 1 >= nz) return;
    for (unsigned k = 0; k < nt; ++k) {
        const unsigned ti = o.y + k;
        if (ti >= F) break;
        int* out = faces + 3 * (size_t)ti;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = mc_tri_edges[c][3 * k + j], ax = e >> 2, lo = e & 1, hi = (e >> 1) & 1;      // mc_table.py: the owner's offset from the cell origin
            const size_t q = p + (ax == 0 ? lo * stride[1] + hi : ax == 1 ? lo * stride[0] + hi : lo * stride[0] + hi * stride[1]);
            out[j] = (int)(off[q].x + __popc(flags[q] & ((1u << ax) - 1u)));
        }
    }
}

// The edge records of k_mc_emit's vertices, in its order (the tile and the walk of k_mc_emit): vertex i on the edge point p owns toward +axis gets
// edge = 3 p + axis, the bracket (0, a - level, 1, b - level) of the edge parameter, t = k_mc_emit's very expression, best = (t, +inf), side = 0 -
// the initial state of the refinement in csrc/mesh_vertices.hip.  Same guards as k_mc_emit: a foreign workspace gives wrong records, no access
// outside the buffers.
__global__ void __launch_bounds__(256) k_mc_emit_edges(const float* __restrict__ vol, int nx, int ny, int nz, float level, int by, int bz,
                                                       const unsigned char* __restrict__ flags, const uint2* __restrict__ off,
                                                       unsigned* __restrict__ edge, float* __restrict__ bracket, float* __restrict__ t_out,
                                                       float* __restrict__ best, unsigned char* __restrict__ side, unsigned V) {
    int x, ty, tz;
    mc_tile(by, bz, x, ty, tz);
    const int z = tz * MC_TILE_Z + (threadIdx.x & 63), y = ty * MC_TILE_Y + (threadIdx.x >> 6);
    if (z >= nz || y >= ny) return;
    const size_t stride[3] = {(size_t)ny * nz, (size_t)nz, 1};
    const size_t p = (size_t)x * stride[0] + (size_t)y * stride[1] + z;
    const unsigned f = flags[p] & 7u;
    if (!f) return;
    const int idx[3] = {x, y, z}, dim[3] = {nx, ny, nz};
    const float a = vol[p];
    unsigned vi = off[p].x;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!((f >> ax) & 1u)) continue;
        if (idx[ax] + 1 < dim[ax] && vi < V) {
            const float b = vol[p + stride[ax]];
            const float t = (level - a) / (b - a);
            edge[vi] = 3u * (unsigned)p + (unsigned)ax;
            float* br = bracket + 4 * (size_t)vi;
            br[0] = 0.f; br[1] = a - level; br[2] = 1.f; br[3] = b - level;
            t_out[vi] = t;
            best[2 * (size_t)vi] = t; best[2 * (size_t)vi + 1] = INFINITY;
            side[vi] = 0;
        }
        ++vi;
    }
}

// 0 = fine; else the refusal is in last_error
static int mc_check_dims(const char* who, int nx, int ny, int nz) {
    char msg[200];
    if (nx < 2 || ny < 2 || nz < 2) {
        snprintf(msg, sizeof(msg), "%s: every dimension must be >= 2 (got %d x %d x %d)", who, nx, ny, nz);
        set_last_error(msg);
        return 2;
    }
    if (3.0 * (double)nx * (double)ny * (double)nz >= 2147483648.0) {
        snprintf(msg, sizeof(msg), "%s: volume too large: 3 nx ny nz must stay below 2^31 (got %d x %d x %d)", who, nx, ny, nz);
        set_last_error(msg);
        return 2;
    }
    // the per-point kernels run on 1-D grids of 256-thread blocks, one per (x, 4 rows, 64 points along z): a volume that is long in x and thin in
    // y / z can stay below the size limit and still need more blocks than one launch takes (blocks x 256 threads < 2^32)
    const double blocks = (double)nx * ((ny + MC_TILE_Y - 1) / MC_TILE_Y) * ((nz + MC_TILE_Z - 1) / MC_TILE_Z);
    if (blocks >= 16777216.0) {
        snprintf(msg, sizeof(msg), "%s: nx * ceil(ny / %d) * ceil(nz / %d) must stay below 2^24 blocks (got %d x %d x %d): put the long axis last",
                 who, MC_TILE_Y, MC_TILE_Z, nx, ny, nz);
        set_last_error(msg);
        return 2;
    }
    return 0;
}

static int mc_check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (ws_bytes < need || ((size_t)ws & 15)) {
        set_last_error((std::string(who) + ": workspace smaller than nerfart_mc_workspace_bytes() or not 16-byte aligned").c_str());
        return 2;
    }
    return 0;
}

}  // namespace nerfart

using namespace nerfart;

extern "C" {

size_t nerfart_mc_workspace_bytes(int nx, int ny, int nz) {
    if (mc_check_dims("mc_workspace_bytes", nx, ny, nz)) return 0;
    return mc_carve(nullptr, (size_t)nx * ny * nz).bytes;
}

int nerfart_mc_count(const float* vol, int nx, int ny, int nz, float level, void* ws, size_t ws_bytes, unsigned* counts, void* stream) {
    if (!vol || !ws || !counts) { set_last_error("mc_count: null pointer"); return 2; }
    if ((size_t)counts & 7) { set_last_error("mc_count: counts must be 8-byte aligned"); return 2; }
    if (int rc = mc_check_dims("mc_count", nx, ny, nz)) return rc;
    const size_t n = (size_t)nx * ny * nz;
    if (int rc = mc_check_workspace("mc_count", ws, ws_bytes, mc_carve(nullptr, n).bytes)) return rc;
    const McWorkspace w = mc_carve(ws, n);
    hipStream_t st = (hipStream_t)stream;
    NERFART_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(unsigned), st));
    const int by = (ny + MC_TILE_Y - 1) / MC_TILE_Y, bz = (nz + MC_TILE_Z - 1) / MC_TILE_Z, bx = (nx + MC_X_CHUNK - 1) / MC_X_CHUNK;
    hipLaunchKernelGGL(k_mc_classify, dim3((unsigned)((size_t)bx * by * bz)), dim3(256), 0, st, vol, nx, ny, nz, level, by, bz, w.flags, w.cases, counts + 2);
    NERFART_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mc_scan, pair_scan_blocks((unsigned)n), dim3(256), 0, st, w.flags, w.cases, (uint2*)w.off, (unsigned)n,
                       pair_scan_sums(w.lvl, 0, counts));
    NERFART_HIP(hipGetLastError());
    if (int rc = pair_scan_finish(w.off, (unsigned)n, w.lvl, counts, st)) return rc;      // the totals (V, F) land in counts[0..1]
    return 0;
}

int nerfart_mc_emit(const float* vol, int nx, int ny, int nz, float level, const float* origin, const float* spacing, const void* ws, size_t ws_bytes,
                    float* verts, int* faces, unsigned V, unsigned F, void* stream) {
    if (V == 0 || F == 0) return 0;
    if (!vol || !origin || !spacing || !ws || !verts || !faces) { set_last_error("mc_emit: null pointer"); return 2; }
    if (int rc = mc_check_dims("mc_emit", nx, ny, nz)) return rc;
    const size_t n = (size_t)nx * ny * nz;
    if (int rc = mc_check_workspace("mc_emit", ws, ws_bytes, mc_carve(nullptr, n).bytes)) return rc;
    const McWorkspace w = mc_carve(const_cast<void*>(ws), n);
    McFrame fr;
    for (int a = 0; a < 3; ++a) { fr.o[a] = origin[a]; fr.s[a] = spacing[a]; }
    const int by = (ny + MC_TILE_Y - 1) / MC_TILE_Y, bz = (nz + MC_TILE_Z - 1) / MC_TILE_Z;
    hipLaunchKernelGGL(k_mc_emit, dim3((unsigned)((size_t)nx * by * bz)), dim3(256), 0, (hipStream_t)stream, vol, nx, ny, nz, level, by, bz, fr,
                       (const unsigned char*)w.flags, (const unsigned char*)w.cases, (const uint2*)w.off, verts, faces, V, F);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mc_emit_edges(const float* vol, int nx, int ny, int nz, float level, const void* ws, size_t ws_bytes, unsigned* edge, float* bracket,
                          float* t, float* best, unsigned char* side, unsigned V, void* stream) {
    if (V == 0) return 0;
    if (!vol || !ws || !edge || !bracket || !t || !best || !side) { set_last_error("mc_emit_edges: null pointer"); return 2; }
    if (int rc = mc_check_dims("mc_emit_edges", nx, ny, nz)) return rc;
    const size_t n = (size_t)nx * ny * nz;
    if (int rc = mc_check_workspace("mc_emit_edges", ws, ws_bytes, mc_carve(nullptr, n).bytes)) return rc;
    const McWorkspace w = mc_carve(const_cast<void*>(ws), n);
    const int by = (ny + MC_TILE_Y - 1) / MC_TILE_Y, bz = (nz + MC_TILE_Z - 1) / MC_TILE_Z;
    hipLaunchKernelGGL(k_mc_emit_edges, dim3((unsigned)((size_t)nx * by * bz)), dim3(256), 0, (hipStream_t)stream, vol, nx, ny, nz, level, by, bz,
                       (const unsigned char*)w.flags, (const uint2*)w.off, edge, bracket, t, best, side, V);
    NERFART_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
