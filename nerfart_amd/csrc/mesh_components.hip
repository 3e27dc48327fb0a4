// mesh_components.hip - connected components of an indexed triangle mesh and the stable compaction that drops some of them
// (mesh_util.mesh_components / filter_components: extract_mesh's "keep the largest component(s)", the floaters of a VolSDF / NeuS field never
// leave the GPU).  nerfart_mc_emit gives one vertex per grid edge, shared by every face that touches it, so connectivity is in `faces` alone.
//
// The rule: two vertices are connected when a face contains both (VERTEX connectivity: two triangles sharing one vertex are one component);
// label[v] = the smallest vertex index of v's component; a vertex in no face is its own component.  A face with an index outside [0, V) joins
// nothing, is counted nowhere, and sets `bad`.  All integers: a second implementation gives the same numbers, whatever its order of work.
//   k_cc_init      parent[v] = v (the parent array IS the label array), n_faces[v] = 0.
//   k_cc_hook      one thread per face unites (a, b) and (a, c): lock-free union-find, the larger root linked under the smaller with one
//                  atomicCAS(&parent[hi], hi, lo).  INVARIANT parent[v] <= v, at every moment: so the smallest index of a component can never be
//                  linked under anything and is the one root left - the result is canonical - and every loop has a bound that follows from the
//                  data (written next to the loops).
//   k_cc_flatten   label[v] = find(v), in place (a root is an ancestor, so a concurrent find through v still ends at the root); counts the roots.
//   k_cc_count     one thread per face: n_faces[label[a]] += 1, equal labels combined within the wave, so one integer atomicAdd per distinct
//                  label per wave (nearly every face belongs to one component: a million adds would queue on one address).  The add that finds
//                  0 is the component's first: it counts the components with faces.  Integer adds commute: the counts are exact.
//   k_cp_scan      exclusive scan of (vertex survives, face survives) over i < max(V, F): the flags are computed on the fly at the first level
//                  (a vertex survives iff keep[label[v]]; a face iff its three indices are in range and keep[label[faces[f][0]]]); the block
//                  scan, the block-sum levels and the add-back are csrc/pair_scan.h, shared with csrc/marching_cubes.hip; the totals are (V', F').
//   k_cp_emit      a surviving vertex writes its old index at its scanned offset; a surviving face writes its three scanned vertex offsets at
//                  its scanned offset.  No atomics in the compaction: two runs give the same bits.  Every write is checked against V' / F'.
// No workgroup waits for another, no kernel spins on a flag: every launch runs to completion on its own.
#include "pair_scan.h"
#include "union_find.h"
#include <string>

namespace nerfart {
namespace cc {

// the compaction's workspace, carved in this order (each buffer rounded up to 256 bytes): off [n][2] (vertex offset, face offset), n = max(V, F, 1),
// then per block-sum level k its [m_k][2] sums, m_0 = ceil(n / 512), m_{k+1} = ceil(m_k / 512), while m_k > 1
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

// the union-find (load_parent, find, unite and their bounds): csrc/union_find.h, shared with csrc/mesh_topology.hip
using uf::find;
using uf::unite;

__global__ void __launch_bounds__(256) k_cc_init(unsigned* __restrict__ parent, unsigned* __restrict__ n_faces, unsigned V) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V) return;
    parent[v] = v;
    n_faces[v] = 0u;
}

__global__ void __launch_bounds__(256) k_cc_hook(const int* __restrict__ faces, unsigned F, unsigned V, unsigned* parent, unsigned* __restrict__ info) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F) return;
    const int* t = faces + 3 * (size_t)f;
    const unsigned a = (unsigned)t[0], b = (unsigned)t[1], c = (unsigned)t[2];      // a negative index is >= 2^31 > V as unsigned
    if (a >= V || b >= V || c >= V) { info[2] = 1u; return; }
    unite(parent, a, b);
    unite(parent, a, c);
}

// In place: parent[v] becomes the root.  A find of another thread that passes through v reads either the old parent or the root: both ancestors.
__global__ void __launch_bounds__(256) k_cc_flatten(unsigned* parent, unsigned V, unsigned* __restrict__ info) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    bool root = false;
    if (v < V) {
        const unsigned r = find(parent, v);
        root = r == v;
        if (!root) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long m = __ballot(root);                           // one add per wave
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(info, (unsigned)__popcll(m));
}

__global__ void __launch_bounds__(256) k_cc_count(const int* __restrict__ faces, unsigned F, unsigned V, const unsigned* __restrict__ label,
                                                  unsigned* __restrict__ n_faces, unsigned* __restrict__ info) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned r = 0u;
    bool pending = false;
    if (f < F) {
        const int* t = faces + 3 * (size_t)f;
        const unsigned a = (unsigned)t[0], b = (unsigned)t[1], c = (unsigned)t[2];
        if (a < V && b < V && c < V) {
            r = label[a];
            pending = r < V;                                               // a label is a vertex index: nothing is written outside n_faces
        }
    }
    // Every lane of the wave runs the loop (the ballots are wave-wide); each round retires the first pending lane and every lane with its
    // label: at most 64 rounds, one for nearly every wave.
    for (;;) {
        const unsigned long long m = __ballot(pending);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const unsigned rl = __shfl(r, leader, 64);
        const bool mine = pending && r == rl;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) {
            if (atomicAdd(n_faces + rl, (unsigned)__popcll(same)) == 0u) atomicAdd(info + 1, 1u);      // the component's first faces
        }
        if (mine) pending = false;
    }
}

// does component `lab` survive?  A label outside [0, V) (an array that is not nerfart_mesh_components') survives nothing and reads nothing.
__device__ __forceinline__ bool kept(const unsigned char* __restrict__ keep, unsigned lab, unsigned V) { return lab < V && keep[lab] != 0; }

__device__ __forceinline__ unsigned vertex_flag(const int* __restrict__ label, const unsigned char* __restrict__ keep, unsigned V, size_t i) {
    return i < V && kept(keep, (unsigned)label[i], V) ? 1u : 0u;
}
__device__ __forceinline__ unsigned face_flag(const int* __restrict__ label, const unsigned char* __restrict__ keep, const int* __restrict__ faces,
                                              unsigned V, unsigned F, size_t i) {
    if (i >= F) return 0u;
    const int* t = faces + 3 * i;
    const unsigned a = (unsigned)t[0], b = (unsigned)t[1], c = (unsigned)t[2];
    return a < V && b < V && c < V && kept(keep, (unsigned)label[a], V) ? 1u : 0u;
}

// The first level of the scan (csrc/pair_scan.h): item i = (vertex i survives, face i survives).
__global__ void __launch_bounds__(256) k_cp_scan(const int* __restrict__ label, const unsigned char* __restrict__ keep, const int* __restrict__ faces,
                                                 unsigned V, unsigned F, uint2* __restrict__ off, unsigned n, uint2* __restrict__ sums) {
    pair_scan_block([&](size_t i) { return make_uint2(vertex_flag(label, keep, V, i), face_flag(label, keep, faces, V, F, i)); }, off, n, sums);
}

// One thread per i < max(V, F): vertex i and face i.  The flags are computed again as k_cp_scan computed them; the offsets come from the caller's
// workspace, so a workspace that does not belong to these arrays can give a wrong mesh but no write outside src_vertex [Vout] / faces_out [Fout]
// and no read outside off [max(V, F)].
__global__ void __launch_bounds__(256) k_cp_emit(const int* __restrict__ label, const unsigned char* __restrict__ keep, const int* __restrict__ faces,
                                                 unsigned V, unsigned F, const uint2* __restrict__ off, int* __restrict__ src_vertex,
                                                 int* __restrict__ faces_out, unsigned Vout, unsigned Fout) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (vertex_flag(label, keep, V, i)) {
        const unsigned o = off[i].x;
        if (o < Vout) src_vertex[o] = (int)i;
    }
    if (face_flag(label, keep, faces, V, F, i)) {
        const unsigned o = off[i].y;
        if (o < Fout) {
            const int* t = faces + 3 * i;
            int* out = faces_out + 3 * (size_t)o;
            out[0] = (int)off[t[0]].x; out[1] = (int)off[t[1]].x; out[2] = (int)off[t[2]].x;       // in range: face_flag checked the three
        }
    }
}

// 0 = fine; else the refusal is in last_error
static int check_sizes(const char* who, unsigned V, unsigned F) {
    char msg[200];
    if (V >= 2147483648u || F >= 2147483648u) {
        snprintf(msg, sizeof(msg), "%s: V and F must stay below 2^31 (got V = %u, F = %u)", who, V, F);
        set_last_error(msg);
        return 2;
    }
    if (3ull * F >= 4294967296ull) {
        snprintf(msg, sizeof(msg), "%s: 3 F must stay below 2^32 (got F = %u)", who, F);
        set_last_error(msg);
        return 2;
    }
    return 0;
}

static size_t items(unsigned V, unsigned F) { const unsigned n = V > F ? V : F; return n ? n : 1; }

static int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (ws_bytes < need || ((size_t)ws & 15)) {
        set_last_error((std::string(who) + ": workspace smaller than nerfart_mesh_compact_workspace_bytes() or not 16-byte aligned").c_str());
        return 2;
    }
    return 0;
}

static dim3 blocks256(unsigned n) { return dim3((unsigned)(((size_t)n + 255) / 256)); }

}  // namespace cc
}  // namespace nerfart

using namespace nerfart;

extern "C" {

int nerfart_mesh_components(const int* faces, unsigned F, unsigned V, int* label, unsigned* n_faces, unsigned* info, void* stream) {
    if (!info || (F && !faces) || (V && (!label || !n_faces))) { set_last_error("mesh_components: null pointer"); return 2; }
    if (int rc = cc::check_sizes("mesh_components", V, F)) return rc;
    hipStream_t st = (hipStream_t)stream;
    NERFART_HIP(hipMemsetAsync(info, 0, 3 * sizeof(unsigned), st));
    if (V == 0) return 0;
    unsigned* parent = (unsigned*)label;
    hipLaunchKernelGGL(cc::k_cc_init, cc::blocks256(V), dim3(256), 0, st, parent, n_faces, V);
    NERFART_HIP(hipGetLastError());
    if (F) {
        hipLaunchKernelGGL(cc::k_cc_hook, cc::blocks256(F), dim3(256), 0, st, faces, F, V, parent, info);
        NERFART_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(cc::k_cc_flatten, cc::blocks256(V), dim3(256), 0, st, parent, V, info);
    NERFART_HIP(hipGetLastError());
    if (F) {
        hipLaunchKernelGGL(cc::k_cc_count, cc::blocks256(F), dim3(256), 0, st, faces, F, V, (const unsigned*)parent, n_faces, info);
        NERFART_HIP(hipGetLastError());
    }
    return 0;
}

size_t nerfart_mesh_compact_workspace_bytes(unsigned V, unsigned F) {
    if (cc::check_sizes("mesh_compact_workspace_bytes", V, F)) return 0;
    return cc::carve(nullptr, cc::items(V, F)).bytes;
}

int nerfart_mesh_compact_count(const int* label, const unsigned char* keep, const int* faces, unsigned V, unsigned F, void* ws, size_t ws_bytes,
                               unsigned* counts, void* stream) {
    if (!ws || !counts || (F && !faces) || (V && (!label || !keep))) { set_last_error("mesh_compact_count: null pointer"); return 2; }
    if ((size_t)counts & 7) { set_last_error("mesh_compact_count: counts must be 8-byte aligned"); return 2; }
    if (int rc = cc::check_sizes("mesh_compact_count", V, F)) return rc;
    const size_t n = cc::items(V, F);
    if (int rc = cc::check_workspace("mesh_compact_count", ws, ws_bytes, cc::carve(nullptr, n).bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) {                                    // no vertex, so no face in range: nothing survives, nothing is launched
        NERFART_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned), st));
        return 0;
    }
    const cc::Workspace w = cc::carve(ws, n);
    hipLaunchKernelGGL(cc::k_cp_scan, pair_scan_blocks((unsigned)n), dim3(256), 0, st, label, keep, faces, V, F, (uint2*)w.off, (unsigned)n,
                       pair_scan_sums(w.lvl, 0, counts));
    NERFART_HIP(hipGetLastError());
    if (int rc = pair_scan_finish(w.off, (unsigned)n, w.lvl, counts, st)) return rc;      // the totals (V', F') land in counts
    return 0;
}

int nerfart_mesh_compact_emit(const int* label, const unsigned char* keep, const int* faces, unsigned V, unsigned F, const void* ws, size_t ws_bytes,
                              int* src_vertex, int* faces_out, unsigned V_out, unsigned F_out, void* stream) {
    if (!ws || (F && !faces) || (V && (!label || !keep)) || (V_out && !src_vertex) || (F_out && !faces_out)) {
        set_last_error("mesh_compact_emit: null pointer");
        return 2;
    }
    if (int rc = cc::check_sizes("mesh_compact_emit", V, F)) return rc;
    if (int rc = cc::check_sizes("mesh_compact_emit", V_out, F_out)) return rc;
    const size_t n = cc::items(V, F);
    if (int rc = cc::check_workspace("mesh_compact_emit", ws, ws_bytes, cc::carve(nullptr, n).bytes)) return rc;
    if (V == 0 || (V_out == 0 && F_out == 0)) return 0;
    const cc::Workspace w = cc::carve(const_cast<void*>(ws), n);
    hipLaunchKernelGGL(cc::k_cp_emit, cc::blocks256((unsigned)n), dim3(256), 0, (hipStream_t)stream, label, keep, faces, V, F, (const uint2*)w.off,
                       src_vertex, faces_out, V_out, F_out);
    NERFART_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
