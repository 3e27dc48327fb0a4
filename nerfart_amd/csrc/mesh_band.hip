// mesh_band.hip - the device side of mesh_util.banded_volume: the narrow-band sweep of extract_mesh, which spends the SDF kernel only on the
// bricks of the N^3 grid that can hold the isosurface, fills the others with a value of the right sign, and checks its own result.  The network
// queries are the caller's (the kernels here never see the model); these kernels make the points, keep the brick flags, move values into the
// dense volume and find the edges the fill got wrong.
//
// Grid points (i, j, k) in 0 .. N - 1, z fastest.  With brick edge B (2 .. 64), brick (bx, by, bz) owns the points with i / B == bx, j / B == by,
// k / B == bz; nb = ceil(N / B) bricks per axis (the last one ragged when N % B != 0); linear brick index (bx nb + by) nb + bz.  The probe of a
// brick is the grid point min(b B + B / 2, N - 1) per axis.
//   k_probe_points   one thread per brick: its probe point [3] fp32.
//   k_select_scan    the first level of csrc/pair_scan.h over the bricks, item = (brick is NEWLY active, its owned points if so) - so one scan gives
//                    a newly active brick both its place in the ascending list and the offset of its first point in the evaluation order.
//                    newly active: mode 0 = NOT (|probe - level| > threshold) (fp32; a NaN probe is active), mode 1 = wanted and not yet active,
//                    mode 2 = not yet active (the dense completion).
//   k_select_emit    one thread per brick: list[place] = brick, ptoff[place] = point offset, flag updated, wanted cleared.  Each thread touches
//                    only its own brick's bytes.  No atomics: the list is ascending and the same in two runs.
//   k_brick_points   one thread per point of a batch [first, first + count) of the evaluation order (bricks in list order, inside a brick z
//                    fastest): a binary search of ptoff finds the brick; writes the point [3] fp32 and its linear grid index.
//   k_scatter        vol[idx[t]] = val[t], checked against N^3.
//   k_fill           every point of an INACTIVE brick = the brick's probe value; z on the fastest thread index, float4 stores when N % 4 == 0 and
//                    B % 4 == 0 (then four consecutive z never straddle a brick or leave 16-byte alignment), scalar otherwise.
//   k_check          one thread per 4 (or 1) points along z: for the three edges toward +x, +y, +z of each (where the neighbour exists), with
//                    marching cubes' predicate inside = value < level: ends that differ mark every INACTIVE brick holding an end - a plain byte
//                    store of 1 (many threads may store the same 1).
//   k_count          wanted bricks and their owned points, summed per block, one integer atomicAdd per block and counter.  Integer adds commute.
// The coordinates are mesh_util.grid_points' bits: (double)index * step, + org, each rounded ONCE in double, then rounded to fp32 - torch runs
// the multiply and the add as two kernels, so they must not be contracted into an fma here: contraction is off for this file.
// No workgroup waits for another; every launch runs to completion on its own.
#include "pair_scan.h"
#include <string>

#pragma clang fp contract(off)

namespace nerfart {
namespace band {

struct Dims { int N, B, nb; unsigned n_bricks; };

__host__ __device__ __forceinline__ int owned(int b, int N, int B) { const int r = N - b * B; return r < B ? r : B; }
__host__ __device__ __forceinline__ int probe_index(int b, int N, int B) { const int p = b * B + B / 2; return p < N - 1 ? p : N - 1; }

__device__ __forceinline__ void brick_xyz(unsigned brick, int nb, int& bx, int& by, int& bz) {
    bz = (int)(brick % (unsigned)nb);
    by = (int)((brick / (unsigned)nb) % (unsigned)nb);
    bx = (int)(brick / ((unsigned)nb * (unsigned)nb));
}
__device__ __forceinline__ unsigned brick_points(unsigned brick, const Dims& d) {      // <= 64^3
    int bx, by, bz;
    brick_xyz(brick, d.nb, bx, by, bz);
    return (unsigned)(owned(bx, d.N, d.B) * owned(by, d.N, d.B) * owned(bz, d.N, d.B));
}
// grid_points' arithmetic: two double roundings, then one to fp32.  Written with the plain operators, HERE, under this file's pragma: HIP's
// __dmul_rn / __dadd_rn are inline functions of a header compiled with contraction on, and the two were fused into one v_fma_f64.
__device__ __forceinline__ float coord(int idx, double step, double org) {
    const double m = (double)idx * step;
    return (float)(m + org);
}

__global__ void __launch_bounds__(256) k_probe_points(Dims d, double step, double org, float* __restrict__ pts) {
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= d.n_bricks) return;
    int bx, by, bz;
    brick_xyz(b, d.nb, bx, by, bz);
    float* o = pts + 3 * (size_t)b;
    o[0] = coord(probe_index(bx, d.N, d.B), step, org);
    o[1] = coord(probe_index(by, d.N, d.B), step, org);
    o[2] = coord(probe_index(bz, d.N, d.B), step, org);
}

__device__ __forceinline__ bool newly_active(int mode, unsigned b, const float* __restrict__ probe, float level, float threshold,
                                             const unsigned char* flag, const unsigned char* wanted) {
    if (mode == 0) return !(fabsf(probe[b] - level) > threshold);
    if (mode == 1) return wanted[b] != 0 && flag[b] == 0;
    return flag[b] == 0;
}

__global__ void __launch_bounds__(256) k_select_scan(int mode, const float* __restrict__ probe, float level, float threshold, Dims d,
                                                     const unsigned char* __restrict__ flag, const unsigned char* __restrict__ wanted,
                                                     uint2* __restrict__ off, uint2* __restrict__ sums) {
    pair_scan_block([&](size_t i) {
        const bool nw = newly_active(mode, (unsigned)i, probe, level, threshold, flag, wanted);
        return make_uint2(nw ? 1u : 0u, nw ? brick_points((unsigned)i, d) : 0u);
    }, off, d.n_bricks, sums);
}

// flag and wanted are read and written by the thread of their own brick only.  Every write of list / ptoff is checked against n_bricks.
__global__ void __launch_bounds__(256) k_select_emit(int mode, const float* __restrict__ probe, float level, float threshold, Dims d,
                                                     unsigned char* flag, unsigned char* wanted, const uint2* __restrict__ off,
                                                     int* __restrict__ list, unsigned* __restrict__ ptoff) {
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= d.n_bricks) return;
    const bool nw = newly_active(mode, b, probe, level, threshold, flag, wanted);
    if (nw) {
        const uint2 o = off[b];
        if (o.x < d.n_bricks) { list[o.x] = (int)b; ptoff[o.x] = o.y; }
    }
    if (mode == 0) flag[b] = nw ? 1 : 0;
    else if (nw) flag[b] = 1;
    wanted[b] = 0;
}

// A list or ptoff that is not k_select_emit's can give wrong points but no access outside list / ptoff [n_list] and pts / idx [count]: a row that
// cannot be resolved gets the index 0xffffffff, which k_scatter skips.
__global__ void __launch_bounds__(256) k_brick_points(const int* __restrict__ list, const unsigned* __restrict__ ptoff, unsigned n_list,
                                                      unsigned first, unsigned count, Dims d, double step, double org, float* __restrict__ pts,
                                                      unsigned* __restrict__ idx) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const unsigned g = first + t;
    unsigned lo = 0, hi = n_list - 1;                                  // the largest e with ptoff[e] <= g (ptoff[0] == 0); <= 32 steps
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo + 1) / 2;
        if (ptoff[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const unsigned brick = (unsigned)list[lo], local = g - ptoff[lo];
    idx[t] = 0xffffffffu;
    if (brick >= d.n_bricks || ptoff[lo] > g) return;
    int bx, by, bz;
    brick_xyz(brick, d.nb, bx, by, bz);
    const unsigned sy = (unsigned)owned(by, d.N, d.B), sz = (unsigned)owned(bz, d.N, d.B);
    if (local >= (unsigned)owned(bx, d.N, d.B) * sy * sz) return;
    const int i = bx * d.B + (int)(local / (sy * sz)), j = by * d.B + (int)((local / sz) % sy), k = bz * d.B + (int)(local % sz);
    float* o = pts + 3 * (size_t)t;
    o[0] = coord(i, step, org);
    o[1] = coord(j, step, org);
    o[2] = coord(k, step, org);
    idx[t] = ((unsigned)i * (unsigned)d.N + (unsigned)j) * (unsigned)d.N + (unsigned)k;          // < N^3 < 2^31
}

__global__ void __launch_bounds__(256) k_scatter(const float* __restrict__ val, const unsigned* __restrict__ idx, unsigned count, unsigned n_vol,
                                                 float* __restrict__ vol) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const unsigned p = idx[t];
    if (p < n_vol) vol[p] = val[t];
}

// thread q -> row (i, j) and the first of its VEC points along z: nq = ceil(N / VEC) threads per row, z fastest
template <int VEC>
__device__ __forceinline__ bool row_of(size_t q, int N, int& i, int& j, int& k0) {
    const unsigned nq = (unsigned)(N + VEC - 1) / VEC;
    if (q >= (size_t)N * N * nq) return false;
    const unsigned row = (unsigned)(q / nq);
    k0 = (int)(q % nq) * VEC;
    j = (int)(row % (unsigned)N);
    i = (int)(row / (unsigned)N);
    return true;
}

// VEC == 4 only when N % 4 == 0 and B % 4 == 0 and vol is 16-byte aligned (the entry point decides)
template <int VEC>
__global__ void __launch_bounds__(256) k_fill(const float* __restrict__ probe, const unsigned char* __restrict__ flag, Dims d, float* __restrict__ vol) {
    int i, j, k0;
    if (!row_of<VEC>((size_t)blockIdx.x * 256u + threadIdx.x, d.N, i, j, k0)) return;
    const unsigned brick = ((unsigned)(i / d.B) * d.nb + (unsigned)(j / d.B)) * d.nb + (unsigned)(k0 / d.B);
    if (flag[brick]) return;
    const float v = probe[brick];
    float* o = vol + ((size_t)i * d.N + j) * d.N + k0;
    if (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(v, v, v, v);
    else *o = v;
}

__device__ __forceinline__ void want(unsigned brick, const unsigned char* __restrict__ flag, unsigned char* __restrict__ wanted) {
    if (!flag[brick]) wanted[brick] = 1;
}

// VEC == 4 only when N % 4 == 0 and vol is 16-byte aligned: then every thread's four points exist and every float4 load is aligned
template <int VEC>
__global__ void __launch_bounds__(256) k_check(const float* __restrict__ vol, float level, const unsigned char* __restrict__ flag, Dims d,
                                               unsigned char* __restrict__ wanted) {
    int i, j, k0;
    if (!row_of<VEC>((size_t)blockIdx.x * 256u + threadIdx.x, d.N, i, j, k0)) return;
    const int N = d.N;
    const size_t p = ((size_t)i * N + j) * N + k0;
    const bool has_x = i + 1 < N, has_y = j + 1 < N;
    float a[VEC + 1], ay[VEC], ax[VEC];
    if (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4*>(vol + p);
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
        if (has_y) { const float4 w = *reinterpret_cast<const float4*>(vol + p + N); ay[0] = w.x; ay[1] = w.y; ay[2] = w.z; ay[3] = w.w; }
        if (has_x) { const float4 w = *reinterpret_cast<const float4*>(vol + p + (size_t)N * N); ax[0] = w.x; ax[1] = w.y; ax[2] = w.z; ax[3] = w.w; }
    } else {
        a[0] = vol[p];
        if (has_y) ay[0] = vol[p + N];
        if (has_x) ax[0] = vol[p + (size_t)N * N];
    }
    const bool has_z = k0 + VEC < N;                                   // the neighbour of the thread's LAST point
    a[VEC] = has_z ? vol[p + VEC] : 0.f;
    const unsigned bx0 = (unsigned)(i / d.B), bx1 = (unsigned)((i + 1) / d.B), by0 = (unsigned)(j / d.B), by1 = (unsigned)((j + 1) / d.B);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const bool in = a[e] < level;
        const unsigned bz0 = (unsigned)((k0 + e) / d.B);
        const unsigned here = (bx0 * d.nb + by0) * d.nb + bz0;
        if (has_x && in != (ax[e] < level)) { want(here, flag, wanted); want((bx1 * d.nb + by0) * d.nb + bz0, flag, wanted); }
        if (has_y && in != (ay[e] < level)) { want(here, flag, wanted); want((bx0 * d.nb + by1) * d.nb + bz0, flag, wanted); }
        if ((e + 1 < VEC || has_z) && in != (a[e + 1] < level)) {
            want(here, flag, wanted);
            want((bx0 * d.nb + by0) * d.nb + (unsigned)((k0 + e + 1) / d.B), flag, wanted);
        }
    }
}

// counts[0] += wanted bricks, counts[1] += their owned points: summed over the block first (wave shuffles, then LDS)
__global__ void __launch_bounds__(256) k_count(const unsigned char* __restrict__ wanted, Dims d, unsigned* __restrict__ counts) {
    __shared__ unsigned part[4][2];
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    const bool w = b < d.n_bricks && wanted[b] != 0;
    unsigned nbk = w ? 1u : 0u, npt = w ? brick_points(b, d) : 0u;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { nbk += __shfl_down(nbk, s, 64); npt += __shfl_down(npt, s, 64); }
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = nbk; part[threadIdx.x >> 6][1] = npt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tb = part[0][0] + part[1][0] + part[2][0] + part[3][0], tp = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        if (tb) { atomicAdd(counts, tb); atomicAdd(counts + 1, tp); }
    }
}

// the selection's workspace, carved in this order (each buffer rounded up to 256 bytes): off [n_bricks][2] (list place, point offset), then the
// block-sum levels of csrc/pair_scan.h
struct Workspace {
    unsigned* off;
    PairScanLevels lvl;
    size_t bytes;
};
static Workspace carve(void* base, size_t n) {
    Workspace w{};
    Carver c(base);
    w.off = c.take<unsigned>(2 * n);
    pair_scan_carve(c, n, w.lvl);
    w.bytes = c.off;
    return w;
}

// 0 = fine and d filled; else the refusal is in last_error
static int check_dims(const char* who, int N, int B, Dims& d) {
    char msg[200];
    if (N < 2) { snprintf(msg, sizeof(msg), "%s: N must be >= 2 (got %d)", who, N); set_last_error(msg); return 2; }
    if (B < 2 || B > 64) { snprintf(msg, sizeof(msg), "%s: the brick edge B must be in 2 .. 64 (got %d)", who, B); set_last_error(msg); return 2; }
    if ((unsigned long long)N * N * N >= 2147483648ull) {
        snprintf(msg, sizeof(msg), "%s: N^3 must stay below 2^31 (got N = %d)", who, N);
        set_last_error(msg);
        return 2;
    }
    d.N = N; d.B = B; d.nb = (N + B - 1) / B;
    d.n_bricks = (unsigned)d.nb * d.nb * d.nb;
    return 0;
}

static dim3 blocks256(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
static bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace band
}  // namespace nerfart

using namespace nerfart;

extern "C" {

size_t nerfart_band_workspace_bytes(int N, int B) {
    band::Dims d;
    if (band::check_dims("band_workspace_bytes", N, B, d)) return 0;
    return band::carve(nullptr, d.n_bricks).bytes;
}

int nerfart_band_probe_points(int N, int B, double step, double org, float* pts, void* stream) {
    band::Dims d;
    if (!pts) { set_last_error("band_probe_points: null pointer"); return 2; }
    if (int rc = band::check_dims("band_probe_points", N, B, d)) return rc;
    hipLaunchKernelGGL(band::k_probe_points, band::blocks256(d.n_bricks), dim3(256), 0, (hipStream_t)stream, d, step, org, pts);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_band_select(int mode, const float* probe, float level, float threshold, int N, int B, unsigned char* flag, unsigned char* wanted,
                        int* list, unsigned* ptoff, void* ws, size_t ws_bytes, unsigned* counts, void* stream) {
    band::Dims d;
    if (!flag || !wanted || !list || !ptoff || !ws || !counts || (mode == 0 && !probe)) { set_last_error("band_select: null pointer"); return 2; }
    if (mode < 0 || mode > 2) { set_last_error("band_select: mode must be 0 (probe test), 1 (wanted bricks) or 2 (every remaining brick)"); return 2; }
    if ((size_t)counts & 7) { set_last_error("band_select: counts must be 8-byte aligned"); return 2; }
    if (int rc = band::check_dims("band_select", N, B, d)) return rc;
    if (ws_bytes < band::carve(nullptr, d.n_bricks).bytes || !band::aligned16(ws)) {
        set_last_error("band_select: workspace smaller than nerfart_band_workspace_bytes() or not 16-byte aligned");
        return 2;
    }
    hipStream_t st = (hipStream_t)stream;
    const band::Workspace w = band::carve(ws, d.n_bricks);
    hipLaunchKernelGGL(band::k_select_scan, pair_scan_blocks(d.n_bricks), dim3(256), 0, st, mode, probe, level, threshold, d,
                       (const unsigned char*)flag, (const unsigned char*)wanted, (uint2*)w.off, pair_scan_sums(w.lvl, 0, counts));
    NERFART_HIP(hipGetLastError());
    if (int rc = pair_scan_finish(w.off, d.n_bricks, w.lvl, counts, st)) return rc;      // the totals (bricks, points) land in counts
    hipLaunchKernelGGL(band::k_select_emit, band::blocks256(d.n_bricks), dim3(256), 0, st, mode, probe, level, threshold, d, flag, wanted,
                       (const uint2*)w.off, list, ptoff);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_band_brick_points(const int* list, const unsigned* ptoff, unsigned n_list, unsigned n_points, unsigned first, unsigned count, int N, int B,
                              double step, double org, float* pts, unsigned* idx, void* stream) {
    band::Dims d;
    if (int rc = band::check_dims("band_brick_points", N, B, d)) return rc;
    if (count == 0) return 0;
    if (!list || !ptoff || !pts || !idx) { set_last_error("band_brick_points: null pointer"); return 2; }
    if (n_list == 0 || n_list > d.n_bricks || n_points > (unsigned)N * N * N || first > n_points || count > n_points - first) {
        char msg[240];
        snprintf(msg, sizeof(msg), "band_brick_points: need 1 <= n_list <= %u bricks, n_points <= N^3 and first + count <= n_points "
                 "(got n_list = %u, n_points = %u, first = %u, count = %u)", d.n_bricks, n_list, n_points, first, count);
        set_last_error(msg);
        return 2;
    }
    hipLaunchKernelGGL(band::k_brick_points, band::blocks256(count), dim3(256), 0, (hipStream_t)stream, list, ptoff, n_list, first, count, d, step, org,
                       pts, idx);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_band_scatter(const float* val, const unsigned* idx, unsigned count, int N, float* vol, void* stream) {
    band::Dims d;
    if (int rc = band::check_dims("band_scatter", N, 2, d)) return rc;
    if (count == 0) return 0;
    if (!val || !idx || !vol) { set_last_error("band_scatter: null pointer"); return 2; }
    hipLaunchKernelGGL(band::k_scatter, band::blocks256(count), dim3(256), 0, (hipStream_t)stream, val, idx, count, (unsigned)N * N * N, vol);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_band_fill(const float* probe, const unsigned char* flag, int N, int B, float* vol, void* stream) {
    band::Dims d;
    if (!probe || !flag || !vol) { set_last_error("band_fill: null pointer"); return 2; }
    if (int rc = band::check_dims("band_fill", N, B, d)) return rc;
    if (N % 4 == 0 && B % 4 == 0 && band::aligned16(vol))
        hipLaunchKernelGGL(band::k_fill<4>, band::blocks256((size_t)N * N * (N / 4)), dim3(256), 0, (hipStream_t)stream, probe, flag, d, vol);
    else
        hipLaunchKernelGGL(band::k_fill<1>, band::blocks256((size_t)N * N * N), dim3(256), 0, (hipStream_t)stream, probe, flag, d, vol);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_band_check(const float* vol, float level, const unsigned char* flag, int N, int B, unsigned char* wanted, unsigned* counts, void* stream) {
    band::Dims d;
    if (!vol || !flag || !wanted || !counts) { set_last_error("band_check: null pointer"); return 2; }
    if (int rc = band::check_dims("band_check", N, B, d)) return rc;
    hipStream_t st = (hipStream_t)stream;
    NERFART_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned), st));
    if (N % 4 == 0 && band::aligned16(vol))
        hipLaunchKernelGGL(band::k_check<4>, band::blocks256((size_t)N * N * (N / 4)), dim3(256), 0, st, vol, level, flag, d, wanted);
    else
        hipLaunchKernelGGL(band::k_check<1>, band::blocks256((size_t)N * N * N), dim3(256), 0, st, vol, level, flag, d, wanted);
    NERFART_HIP(hipGetLastError());
    hipLaunchKernelGGL(band::k_count, band::blocks256(d.n_bricks), dim3(256), 0, st, (const unsigned char*)wanted, d, counts);
    NERFART_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
