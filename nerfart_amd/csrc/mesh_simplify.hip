// mesh_simplify.hip - vertex clustering with quadric error metrics on the grid a marching-cubes mesh lives on (mesh_util.simplify_clusters,
// extract_mesh(simplify_factor=); Lindstrom 2000, the representative placed as in dual contouring).  The rules are in include/nerfart_hip.h; the
// numpy statement is tests/mesh_simplify_ref.py.
//
// verts [V, 3] fp32 in GRID coordinates (grid point (i, j, k) sits at (i, j, k)), faces [F, 3] int32, cluster factor c >= 2, grid (nx, ny, nz).
// The cluster lattice has l = ceil(n / c) cells per axis, L = lx ly lz cells, linear index (kx ly + ky) lz + kz.
//   k_sm_mark      one thread per vertex: cell[v] = its lattice cell from min((int)floorf(x), n - 1) / c per axis - integer division only - and
//                  occ[cell] = 1 (plain byte stores of the same value).  A non-finite coordinate or one outside [0, n - 1]: cell[v] = -1, `bad`.
//   k_sm_hash      one thread per face: its rotated triple of cells (smallest first, cyclic order kept); a face with an index outside [0, V) or
//                  a vertex without a cell sets `bad`; a face with fewer than three distinct cells is dropped; every other face enters the
//                  open-addressing table tab [T] of FACE INDICES, T = the power of two >= max(2 F, 2): a slot goes from EMPTY to f by atomicCAS, an
//                  occupied slot is compared through its occupant's rotated triple - equal: atomicMin(slot, f) and stop, different: next slot.
//                  A slot never empties and never changes its key, so every key owns exactly one slot, whatever the order of work, and that
//                  slot ends holding the key's smallest face index: face f survives iff tab[slot[f]] == f - canonical.
//   k_sm_scan      exclusive scan (csrc/pair_scan.h) of (cell i occupied, face i survives) over i < max(L, F): the totals are (V', F'), the x
//                  lane numbers the occupied cells in ascending linear order, the y lane compacts the surviving faces in input order.
//   k_sm_assign    one thread per vertex: cluster[v] = off[cell[v]].x (-1 without a cell), cell_of[cluster] = cell (same-value stores), and
//                  the vertex's local position and 1 into the cluster's sums.
//   k_sm_quadric   one thread per face: n = e1 x e2 with e1 = (b - a) / c, e2 = (c - a) / c (local units); n != 0: A = n n^T (6 numbers) and
//                  b = n (n . a) with `a` in the frame of the cluster, once to every DISTINCT cluster among the three.
//   (one host read of counts = (V', F', bad))
//   k_sm_solve     one thread per cluster, fp64 in registers: x* = argmin x^T A x - 2 b^T x + lambda |x - m|^2, lambda = reg tr(A) / 3
//                  (tr(A) == 0: x* = m), a 3 x 3 Cholesky of A + lambda I, clamped to [-1/2, 1/2]^3, mapped back: g' = c (k + 1/2) + c x*.
//   k_sm_faces     one thread per face: a survivor writes the rotated triple of its three cluster numbers at off[f].y.  No atomics.
//
// ACCUMULATION is order-independent: every fp32 term t goes into a 64-bit integer sum as llrint(t * 2^40) by an integer atomicAdd (integer adds
// commute: two runs give the same bits).  QUANTUM 2^-40 (in local units: of n_i n_j, of n_i (n . a), of a local coordinate); t * 2^40 is an
// exact fp32 product, the conversion rounds to nearest: at most half a quantum per term.  GUARDS, both checked, a violation sets `bad`:
//   |t| <= TERM_MAX = 2^6 for every term (tested as !(|t| <= 2^6), so a NaN fails it; a term that fails is not added), and
//   at most COUNT_MAX = 2^16 face contributions and 2^16 member vertices per cluster (counted by integer atomicAdd; the contribution that finds
//   the counter at 2^16 or above sets `bad`).
// So while `bad` is clear every sum is at most 2^6 * 2^40 * 2^16 = 2^62 < 2^63 in magnitude: no wrap.  A marching-cubes triangle has edges of
// at most sqrt(3) / c <= 0.87 local units and vertices within 1.37 of a cluster centre it touches, so |n_i| <= 0.75, |A_ij| <= 0.57 and
// |b_i| <= 2.4: far inside.  A cluster of c^3 cells is touched by the triangles of (c + 2)^3 cells, five at the most each: 29,160 for c = 16.
// The constant a . A a of the quadric does not enter the argmin and is not accumulated.
//
// Every probe loop is bounded by the table size (written next to it).  No workgroup waits for another, no kernel spins on a flag.  Every
// output write is checked against V' / F'.  No kernel uses scratch: the compiler's resource output (-Rpass-analysis=kernel-resource-usage)
// gives ScratchSize 0, .private_segment_fixed_size 0, for each of the seven kernels here.
#include "pair_scan.h"
#include <string>

namespace nerfart {
namespace sm {

constexpr unsigned EMPTY = 0xffffffffu;          // of a table slot and of slot[f]
constexpr float FIX_SCALE = 1099511627776.f;     // 2^40: 1 / quantum
constexpr double FIX_QUANTUM = 1.0 / 1099511627776.0;
constexpr float TERM_MAX = 64.f;                 // 2^6
constexpr unsigned COUNT_MAX = 65536u;           // 2^16
constexpr int ACC = 12;                          // per cluster: A00 A01 A02 A11 A12 A22, b0 b1 b2, s0 s1 s2

struct Grid {
    int c, nx, ny, nz, lx, ly, lz;
    unsigned L;
};

// the workspace, carved in this order (each buffer rounded up to 256 bytes); n = max(L, F, 1), K = min(V, L) bounds the clusters
struct Workspace {
    unsigned* off;            // [n][2] (cluster number of a cell, offset of a surviving face)
    PairScanLevels lvl;
    int* cell;                // [V]
    unsigned char* occ;       // [L]
    unsigned* tab;            // [T]
    unsigned* slot;           // [F]
    long long* acc;           // [K][ACC]
    unsigned* cnt;            // [K][2] (face contributions, member vertices)
    int* cell_of;             // [K]
    unsigned T;
    size_t n, K, bytes;
};
static unsigned table_size(unsigned F) { unsigned t = 2; while (t < 2u * F) t <<= 1; return t; }      // F < 2^30: t <= 2^31
static Workspace carve(void* base, unsigned V, unsigned F, const Grid& g) {
    Workspace w{};
    Carver c(base);
    w.n = g.L > F ? g.L : F;
    if (w.n == 0) w.n = 1;
    w.K = V < g.L ? V : g.L;
    w.T = table_size(F);
    w.off = c.take<unsigned>(2 * w.n);
    pair_scan_carve(c, w.n, w.lvl);
    w.cell = c.take<int>(V);
    w.occ = c.take<unsigned char>(g.L);
    w.tab = c.take<unsigned>(w.T);
    w.slot = c.take<unsigned>(F);
    w.acc = c.take<long long>(w.K * ACC);
    w.cnt = c.take<unsigned>(2 * w.K);
    w.cell_of = c.take<int>(w.K);
    w.bytes = c.off;
    return w;
}

// the lattice cell of one axis: integer arithmetic decides it.  The caller has checked 0 <= x <= n - 1.
__device__ __forceinline__ int axis_cell(float x, int n, int c) {
    const int i = (int)floorf(x);
    return (i < n - 1 ? i : n - 1) / c;
}
__device__ __forceinline__ bool in_range(float x, int n) { return x >= 0.f && x <= (float)(n - 1); }      // false for a NaN

__global__ void __launch_bounds__(256) k_sm_mark(const float* __restrict__ verts, unsigned V, Grid g, int* __restrict__ cell,
                                                 unsigned char* __restrict__ occ, unsigned* __restrict__ counts) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V) return;
    const float* p = verts + 3 * (size_t)v;
    const float x = p[0], y = p[1], z = p[2];
    if (!(in_range(x, g.nx) && in_range(y, g.ny) && in_range(z, g.nz))) { cell[v] = -1; counts[2] = 1u; return; }
    const unsigned q = ((unsigned)axis_cell(x, g.nx, g.c) * (unsigned)g.ly + (unsigned)axis_cell(y, g.ny, g.c)) * (unsigned)g.lz
                       + (unsigned)axis_cell(z, g.nz, g.c);
    cell[v] = (int)q;                                                      // q < L by construction
    occ[q] = 1;
}

// (a, b, c) with the smallest first, the cyclic order kept.  For three distinct numbers the result is unique.
__device__ __forceinline__ void rotate(int& a, int& b, int& c) {
    if (a <= b && a <= c) return;
    if (b <= a && b <= c) { const int t = a; a = b; b = c; c = t; return; }
    const int t = c; c = b; b = a; a = t;
}

// The rotated triple of the cells of face f; false when the face joins nothing (a bad index, a vertex without a cell) or is degenerate.
__device__ __forceinline__ bool face_key(const int* __restrict__ faces, const int* __restrict__ cell, unsigned V, unsigned f, int& a, int& b, int& c,
                                         bool& bad) {
    const int* t = faces + 3 * (size_t)f;
    const unsigned ia = (unsigned)t[0], ib = (unsigned)t[1], ic = (unsigned)t[2];      // a negative index is >= 2^31 > V as unsigned
    bad = true;
    if (ia >= V || ib >= V || ic >= V) return false;
    a = cell[ia]; b = cell[ib]; c = cell[ic];
    if (a < 0 || b < 0 || c < 0) return false;
    bad = false;
    if (a == b || b == c || a == c) return false;
    rotate(a, b, c);
    return true;
}

__device__ __forceinline__ unsigned key_hash(int a, int b, int c) {
    unsigned h = (unsigned)a * 0x9E3779B1u ^ (unsigned)b * 0x85EBCA77u ^ (unsigned)c * 0xC2B2AE3Du;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
    return h;
}

__global__ void __launch_bounds__(256) k_sm_hash(const int* __restrict__ faces, const int* __restrict__ cell, unsigned V, unsigned F, unsigned* tab,
                                                 unsigned T, unsigned* __restrict__ slot, unsigned* __restrict__ counts) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F) return;
    int a, b, c;
    bool bad;
    unsigned mine = EMPTY;
    if (face_key(faces, cell, V, f, a, b, c, bad)) {
        unsigned h = key_hash(a, b, c) & (T - 1);
        // BOUND: T probes.  At most F <= T / 2 slots are ever occupied, so an empty slot - or this key's - is met before the probes wrap around.
        for (unsigned probe = 0; probe < T; ++probe, h = (h + 1) & (T - 1)) {
            const unsigned cur = atomicCAS(tab + h, EMPTY, f);
            if (cur == EMPTY) { mine = h; break; }
            int oa, ob, oc;
            bool obad;
            // cur < F is a face that passed face_key (nothing else is ever stored); a concurrent atomicMin replaces it by a face of the same key
            if (cur < F && face_key(faces, cell, V, cur, oa, ob, oc, obad) && oa == a && ob == b && oc == c) {
                atomicMin(tab + h, f);
                mine = h;
                break;
            }
        }
        if (mine == EMPTY) counts[2] = 1u;                                 // cannot happen (the bound above); never silent
    } else if (bad) {
        counts[2] = 1u;
    }
    slot[f] = mine;
}

__device__ __forceinline__ unsigned survives(const unsigned* __restrict__ tab, unsigned T, const unsigned* __restrict__ slot, unsigned F, size_t i) {
    if (i >= F) return 0u;
    const unsigned s = slot[i];
    return s < T && tab[s] == (unsigned)i ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_sm_scan(const unsigned char* __restrict__ occ, unsigned L, const unsigned* __restrict__ tab, unsigned T,
                                                 const unsigned* __restrict__ slot, unsigned F, uint2* __restrict__ off, unsigned n,
                                                 uint2* __restrict__ sums) {
    pair_scan_block([&](size_t i) { return make_uint2(i < L && occ[i] ? 1u : 0u, survives(tab, T, slot, F, i)); }, off, n, sums);
}

// One term into its 64-bit sum.  Exact scaling, rounding to nearest; a term outside the guard (or a NaN) is not added and sets `bad`.
__device__ __forceinline__ void add_term(long long* dst, float t, unsigned* __restrict__ counts) {
    if (!(fabsf(t) <= TERM_MAX)) { counts[2] = 1u; return; }
    atomicAdd((unsigned long long*)dst, (unsigned long long)__float2ll_rn(t * FIX_SCALE));      // two's complement: the signed sum
}

__device__ __forceinline__ void cell_coords(const Grid& g, int q, int& kx, int& ky, int& kz) {
    kz = q % g.lz; q /= g.lz;
    ky = q % g.ly;
    kx = q / g.ly;
}
// the centre of lattice cell k of one axis, in grid coordinates: c (k + 1/2), exact in fp32
__device__ __forceinline__ float centre(int k, int c) { return (float)c * ((float)k + 0.5f); }

__global__ void __launch_bounds__(256) k_sm_assign(const float* __restrict__ verts, const int* __restrict__ cell, unsigned V, Grid g,
                                                   const uint2* __restrict__ off, unsigned K, int* __restrict__ cluster, int* __restrict__ cell_of,
                                                   long long* acc, unsigned* cnt, unsigned* __restrict__ counts) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V) return;
    const int q = cell[v];
    if (q < 0) { cluster[v] = -1; return; }
    const unsigned k = off[q].x;
    if (k >= K) { cluster[v] = -1; counts[2] = 1u; return; }             // cannot happen: at most min(V, L) cells are occupied
    cluster[v] = (int)k;
    cell_of[k] = q;
    if (atomicAdd(cnt + 2 * (size_t)k + 1, 1u) >= COUNT_MAX) counts[2] = 1u;
    int kx, ky, kz;
    cell_coords(g, q, kx, ky, kz);
    const float* p = verts + 3 * (size_t)v;
    const float cf = (float)g.c;
    long long* a = acc + (size_t)k * ACC;
    add_term(a + 9, (p[0] - centre(kx, g.c)) / cf, counts);
    add_term(a + 10, (p[1] - centre(ky, g.c)) / cf, counts);
    add_term(a + 11, (p[2] - centre(kz, g.c)) / cf, counts);
}

__global__ void __launch_bounds__(256) k_sm_quadric(const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ cluster,
                                                    const int* __restrict__ cell_of, unsigned V, unsigned F, Grid g, unsigned K, long long* acc,
                                                    unsigned* cnt, unsigned* __restrict__ counts) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F) return;
    const int* t = faces + 3 * (size_t)f;
    const unsigned ia = (unsigned)t[0], ib = (unsigned)t[1], ic = (unsigned)t[2];
    if (ia >= V || ib >= V || ic >= V) return;                             // k_sm_hash has set `bad`
    const int ka = cluster[ia], kb = cluster[ib], kc = cluster[ic];
    if (ka < 0 || kb < 0 || kc < 0) return;                                // k_sm_mark has set `bad`
    const float* pa = verts + 3 * (size_t)ia;
    const float* pb = verts + 3 * (size_t)ib;
    const float* pc = verts + 3 * (size_t)ic;
    const float cf = (float)g.c;
    const float ax = pa[0], ay = pa[1], az = pa[2];
    const float ux = (pb[0] - ax) / cf, uy = (pb[1] - ay) / cf, uz = (pb[2] - az) / cf;
    const float wx = (pc[0] - ax) / cf, wy = (pc[1] - ay) / cf, wz = (pc[2] - az) / cf;
    const float n0 = uy * wz - uz * wy, n1 = uz * wx - ux * wz, n2 = ux * wy - uy * wx;
    if (n0 == 0.f && n1 == 0.f && n2 == 0.f) return;
    const int ks[3] = {ka, kb, kc};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int k = ks[j];
        if ((j >= 1 && k == ks[0]) || (j == 2 && k == ks[1])) continue;    // once per distinct cluster
        if ((unsigned)k >= K) { counts[2] = 1u; continue; }
        if (atomicAdd(cnt + 2 * (size_t)k, 1u) >= COUNT_MAX) counts[2] = 1u;
        int kx, ky, kz;
        cell_coords(g, cell_of[k], kx, ky, kz);
        const float lx = (ax - centre(kx, g.c)) / cf, ly = (ay - centre(ky, g.c)) / cf, lz = (az - centre(kz, g.c)) / cf;
        const float d = (n0 * lx + n1 * ly) + n2 * lz;
        long long* a = acc + (size_t)k * ACC;
        add_term(a + 0, n0 * n0, counts); add_term(a + 1, n0 * n1, counts); add_term(a + 2, n0 * n2, counts);
        add_term(a + 3, n1 * n1, counts); add_term(a + 4, n1 * n2, counts); add_term(a + 5, n2 * n2, counts);
        add_term(a + 6, n0 * d, counts); add_term(a + 7, n1 * d, counts); add_term(a + 8, n2 * d, counts);
    }
}

__global__ void __launch_bounds__(256) k_sm_solve(const long long* __restrict__ acc, const unsigned* __restrict__ cnt, const int* __restrict__ cell_of,
                                                  Grid g, double reg, float* __restrict__ verts_out, unsigned Vout) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= Vout) return;
    const long long* s = acc + (size_t)k * ACC;
    const double q = FIX_QUANTUM;
    const double a00 = s[0] * q, a01 = s[1] * q, a02 = s[2] * q, a11 = s[3] * q, a12 = s[4] * q, a22 = s[5] * q;
    const double b0 = s[6] * q, b1 = s[7] * q, b2 = s[8] * q;
    const unsigned members = cnt[2 * (size_t)k + 1];
    const double inv = members ? 1.0 / (double)members : 0.0;
    const double m0 = s[9] * q * inv, m1 = s[10] * q * inv, m2 = s[11] * q * inv;
    double x0 = m0, x1 = m1, x2 = m2;
    const double tr = a00 + a11 + a22;
    if (tr > 0.0) {
        const double lam = reg * tr / 3.0;
        // Cholesky of M = A + lam I (lower factor l), then the two triangular solves of M x = b + lam m
        const double r0 = b0 + lam * m0, r1 = b1 + lam * m1, r2 = b2 + lam * m2;
        const double d0 = a00 + lam;
        const double l00 = sqrt(d0), l10 = a01 / l00, l20 = a02 / l00;
        const double d1 = a11 + lam - l10 * l10;
        const double l11 = sqrt(d1), l21 = (a12 - l20 * l10) / l11;
        const double d2 = a22 + lam - l20 * l20 - l21 * l21;
        const double l22 = sqrt(d2);
        // cond(A + lam I) <= 1 + 3 / reg for a positive semi-definite A, so the pivots are positive; the sums are A plus at most half a quantum
        // per term, and a pivot that this noise has pushed to zero or below leaves the mean in place rather than a NaN.
        if (d0 > 0.0 && d1 > 0.0 && d2 > 0.0) {
            const double y0 = r0 / l00, y1 = (r1 - l10 * y0) / l11, y2 = (r2 - l20 * y0 - l21 * y1) / l22;
            x2 = y2 / l22;
            x1 = (y1 - l21 * x2) / l11;
            x0 = (y0 - l10 * x1 - l20 * x2) / l00;
        }
    }
    x0 = fmin(fmax(x0, -0.5), 0.5); x1 = fmin(fmax(x1, -0.5), 0.5); x2 = fmin(fmax(x2, -0.5), 0.5);      // fmax(NaN, -0.5) = -0.5: inside the cell
    int kx, ky, kz;
    cell_coords(g, cell_of[k], kx, ky, kz);
    const double c = (double)g.c;
    float* o = verts_out + 3 * (size_t)k;
    o[0] = (float)(c * ((double)kx + 0.5) + c * x0);
    o[1] = (float)(c * ((double)ky + 0.5) + c * x1);
    o[2] = (float)(c * ((double)kz + 0.5) + c * x2);
}

// One thread per face.  The survivors and their offsets come from the caller's workspace, the numbers from the caller's cluster array: arrays
// that do not belong to this mesh can give a wrong mesh, but no write outside faces_out [Fout] and no read outside the arrays' own sizes.
__global__ void __launch_bounds__(256) k_sm_faces(const int* __restrict__ faces, const int* __restrict__ cluster, unsigned V, unsigned F,
                                                  const unsigned* __restrict__ tab, unsigned T, const unsigned* __restrict__ slot,
                                                  const uint2* __restrict__ off, int* __restrict__ faces_out, unsigned Fout) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F || !survives(tab, T, slot, F, f)) return;
    const unsigned o = off[f].y;
    if (o >= Fout) return;
    const int* t = faces + 3 * (size_t)f;
    const unsigned ia = (unsigned)t[0], ib = (unsigned)t[1], ic = (unsigned)t[2];
    if (ia >= V || ib >= V || ic >= V) return;
    int a = cluster[ia], b = cluster[ib], c = cluster[ic];
    rotate(a, b, c);                        // the clusters are numbered in ascending cell order: the rotation k_sm_hash made on the cells
    int* out = faces_out + 3 * (size_t)o;
    out[0] = a; out[1] = b; out[2] = c;
}

// 0 = fine; else the refusal is in last_error
static int make_grid(const char* who, unsigned V, unsigned F, int c, int nx, int ny, int nz, Grid& g) {
    char msg[240];
    if (c < 2) {
        snprintf(msg, sizeof(msg), "%s: the cluster factor must be >= 2 (got %d)", who, c);
        set_last_error(msg);
        return 2;
    }
    if (nx < 1 || ny < 1 || nz < 1 || nx > 16777216 || ny > 16777216 || nz > 16777216) {      // n - 1 is exact as a float
        snprintf(msg, sizeof(msg), "%s: every grid dimension must be in 1 .. 2^24 (got %d x %d x %d)", who, nx, ny, nz);
        set_last_error(msg);
        return 2;
    }
    g.c = c; g.nx = nx; g.ny = ny; g.nz = nz;
    g.lx = (nx + c - 1) / c; g.ly = (ny + c - 1) / c; g.lz = (nz + c - 1) / c;
    const unsigned long long L = (unsigned long long)g.lx * g.ly * g.lz;                     // < 2^72 / 8: no overflow in 64 bits
    if (L >= 2147483648ull) {
        snprintf(msg, sizeof(msg), "%s: the cluster lattice must stay below 2^31 cells (got %d x %d x %d)", who, g.lx, g.ly, g.lz);
        set_last_error(msg);
        return 2;
    }
    g.L = (unsigned)L;
    if (V >= 2147483648u || F >= 1073741824u) {
        snprintf(msg, sizeof(msg), "%s: V must stay below 2^31 and F below 2^30 (got V = %u, F = %u)", who, V, F);
        set_last_error(msg);
        return 2;
    }
    return 0;
}

static int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (ws_bytes < need || ((size_t)ws & 15)) {
        set_last_error((std::string(who) + ": workspace smaller than nerfart_mesh_simplify_workspace_bytes() or not 16-byte aligned").c_str());
        return 2;
    }
    return 0;
}

static dim3 blocks256(unsigned n) { return dim3((unsigned)(((size_t)n + 255) / 256)); }

}  // namespace sm
}  // namespace nerfart

using namespace nerfart;

extern "C" {

size_t nerfart_mesh_simplify_workspace_bytes(unsigned V, unsigned F, int c, int nx, int ny, int nz) {
    sm::Grid g;
    if (sm::make_grid("mesh_simplify_workspace_bytes", V, F, c, nx, ny, nz, g)) return 0;
    return sm::carve(nullptr, V, F, g).bytes;
}

int nerfart_mesh_simplify_count(const float* verts, const int* faces, unsigned V, unsigned F, int c, int nx, int ny, int nz, void* ws, size_t ws_bytes,
                                int* cluster, unsigned* counts, void* stream) {
    if (!ws || !counts || (F && !faces) || (V && (!verts || !cluster))) { set_last_error("mesh_simplify_count: null pointer"); return 2; }
    if ((size_t)counts & 7) { set_last_error("mesh_simplify_count: counts must be 8-byte aligned"); return 2; }
    sm::Grid g;
    if (int rc = sm::make_grid("mesh_simplify_count", V, F, c, nx, ny, nz, g)) return rc;
    if (int rc = sm::check_workspace("mesh_simplify_count", ws, ws_bytes, sm::carve(nullptr, V, F, g).bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    NERFART_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(unsigned), st));
    const sm::Workspace w = sm::carve(ws, V, F, g);
    NERFART_HIP(hipMemsetAsync(w.occ, 0, g.L, st));
    NERFART_HIP(hipMemsetAsync(w.tab, 0xff, sizeof(unsigned) * (size_t)w.T, st));
    if (w.K) {
        NERFART_HIP(hipMemsetAsync(w.acc, 0, sizeof(long long) * w.K * sm::ACC, st));
        NERFART_HIP(hipMemsetAsync(w.cnt, 0, sizeof(unsigned) * 2 * w.K, st));
    }
    if (V) {
        hipLaunchKernelGGL(sm::k_sm_mark, sm::blocks256(V), dim3(256), 0, st, verts, V, g, w.cell, w.occ, counts);
        NERFART_HIP(hipGetLastError());
    }
    if (F) {
        hipLaunchKernelGGL(sm::k_sm_hash, sm::blocks256(F), dim3(256), 0, st, faces, (const int*)w.cell, V, F, w.tab, w.T, w.slot, counts);
        NERFART_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(sm::k_sm_scan, pair_scan_blocks((unsigned)w.n), dim3(256), 0, st, (const unsigned char*)w.occ, g.L, (const unsigned*)w.tab, w.T,
                       (const unsigned*)w.slot, F, (uint2*)w.off, (unsigned)w.n, pair_scan_sums(w.lvl, 0, counts));
    NERFART_HIP(hipGetLastError());
    if (int rc = pair_scan_finish(w.off, (unsigned)w.n, w.lvl, counts, st)) return rc;       // the totals (V', F') land in counts[0], counts[1]
    if (V) {
        hipLaunchKernelGGL(sm::k_sm_assign, sm::blocks256(V), dim3(256), 0, st, verts, (const int*)w.cell, V, g, (const uint2*)w.off, (unsigned)w.K, cluster,
                           w.cell_of, w.acc, w.cnt, counts);
        NERFART_HIP(hipGetLastError());
    }
    if (F && V) {
        hipLaunchKernelGGL(sm::k_sm_quadric, sm::blocks256(F), dim3(256), 0, st, verts, faces, (const int*)cluster, (const int*)w.cell_of, V, F, g,
                           (unsigned)w.K, w.acc, w.cnt, counts);
        NERFART_HIP(hipGetLastError());
    }
    return 0;
}

int nerfart_mesh_simplify_emit(const int* faces, unsigned V, unsigned F, int c, int nx, int ny, int nz, double reg, const void* ws, size_t ws_bytes,
                               const int* cluster, float* verts_out, int* faces_out, unsigned V_out, unsigned F_out, void* stream) {
    if (!ws || (F && !faces) || (V && !cluster) || (V_out && !verts_out) || (F_out && !faces_out)) {
        set_last_error("mesh_simplify_emit: null pointer");
        return 2;
    }
    if (!(reg > 0.0) || !(reg <= 1e6)) { set_last_error("mesh_simplify_emit: reg must be in (0, 1e6]"); return 2; }
    sm::Grid g;
    if (int rc = sm::make_grid("mesh_simplify_emit", V, F, c, nx, ny, nz, g)) return rc;
    if (int rc = sm::check_workspace("mesh_simplify_emit", ws, ws_bytes, sm::carve(nullptr, V, F, g).bytes)) return rc;
    const sm::Workspace w = sm::carve(const_cast<void*>(ws), V, F, g);
    if (V_out > w.K || F_out > F) { set_last_error("mesh_simplify_emit: V_out / F_out larger than any count of this mesh"); return 2; }
    hipStream_t st = (hipStream_t)stream;
    if (V_out) {
        hipLaunchKernelGGL(sm::k_sm_solve, sm::blocks256(V_out), dim3(256), 0, st, (const long long*)w.acc, (const unsigned*)w.cnt, (const int*)w.cell_of,
                           g, reg, verts_out, V_out);
        NERFART_HIP(hipGetLastError());
    }
    if (F_out) {
        hipLaunchKernelGGL(sm::k_sm_faces, sm::blocks256(F), dim3(256), 0, st, faces, cluster, V, F, (const unsigned*)w.tab, w.T, (const unsigned*)w.slot,
                           (const uint2*)w.off, faces_out, F_out);
        NERFART_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
