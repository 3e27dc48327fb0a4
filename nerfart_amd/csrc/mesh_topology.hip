// mesh_topology.hip - half-edge adjacency, manifold checks and per-component measures of an indexed triangle mesh (mesh_util.half_edges /
// mesh_topology, tools/check_mesh.py: "is it watertight, how many holes, what genus").  The definitions - proper / degenerate / bad faces,
// boundary / manifold / flipped / non-manifold edges, fans, boundary loops - are in include/nerfart_hip.h; tests/mesh_topology_ref.py states them
// in numpy.  Everything but `measure` is integers and independent of where a key landed in the table and of the order of work.
//
// THE EDGE TABLE (csrc/edge_table.h, shared with csrc/mesh_repair.hip): open addressing, linear probing, C = 2^table_log2 slots of 24 bytes {key, cnt[2], minh[2]}.  key = (a << 32) | b of the
// undirected edge a < b, claimed with one 64-bit atomicCAS on an empty slot (all ones: never a key, a < 2^31); cnt[d] counts the proper
// half-edges running a -> b (d = 0) and b -> a (d = 1) with atomicAdd; minh[d] is the smallest half-edge id of direction d with atomicMin.
// A probe sequence visits at most C slots, then sets the overflow flag and gives up: it cannot spin, whatever the faces hold (the host refuses
// a table of fewer than 3 F + 1 slots, so with the table initialised by this call an empty slot is always met first).
//   k_mt_init      table slots empty, parent of every corner and every vertex = itself, loop_size = 0.
//   k_mt_insert    one thread per face: classifies it (tallies per wave, one atomicAdd each), inserts the three half-edges of a proper face and
//                  remembers each one's slot in slot_of [3 F] (NOSLOT for a face that is not proper), so no later pass probes again.
//   k_mt_resolve   one thread per half-edge, after every count is final: edge_uses, twin; the half-edge with the smallest id of its edge is the
//                  edge's OWNER and tallies the edge (E, boundary, flipped, non-manifold).  Every other half-edge of an edge with n == 2 unites
//                  its two corners with the owner's (fans; union-find over corners, csrc/union_find.h); a boundary edge unites its two vertices
//                  (boundary loops; union-find over vertices: two boundary edges are joined when they share a vertex).
//   k_mt_roots     one thread per half-edge = corner: a corner that is the root of its class adds 1 to vertex_fans of its vertex; a boundary
//                  half-edge adds 1 to loop_size at the root of its loop.  Integer adds commute.
//   k_mt_vertex    one thread per vertex: referenced (fans > 0, kept in the workspace for the stats), more than one fan, loops and the longest.
//   k_cs_*         nerfart_mesh_component_stats: per vertex, per face, per half-edge; equal labels are combined within the wave first (nearly
//                  every face belongs to one component: a million adds would queue on one address), then one atomicAdd per label per wave.
//                  The fp64 sums are the one result whose last bits depend on the order of the atomics.
// No workgroup waits for another, no kernel spins on a flag.  Every write is checked against the caller's sizes; every index read from the
// workspace is checked before it is used, so a workspace that does not belong to the arrays gives wrong numbers but touches nothing outside.
// Compiled without contraction: the fp64 per-face terms are evaluated as written, every operation rounded once.
#include "edge_table.h"
#include "union_find.h"

#pragma clang fp contract(off)

namespace nerfart {
namespace mt {

using et::Slot; using et::EMPTY; using et::NOSLOT; using et::NONE; using et::MAX_LOG2;
using et::tally; using et::next_in_face; using et::check_sizes; using et::smallest_log2; using et::resolve_log2; using et::blocks256;

// info [16]
enum { I_PROPER = 0, I_DEGENERATE, I_BAD, I_REFERENCED, I_EDGES, I_BOUNDARY, I_FLIPPED, I_NONMANIFOLD, I_BOWTIE, I_LOOPS, I_LONGEST, I_OVERFLOW };

// the workspace, carved in this order (each buffer rounded up to 256 bytes); the table comes LAST, so that the offsets of the others do not
// depend on its size and nerfart_mesh_component_stats needs no table_log2
struct Workspace {
    unsigned* slot_of;        // [max(3 F, 1)]
    unsigned* parent_c;       // [max(3 F, 1)] corners
    unsigned* parent_v;       // [max(V, 1)] vertices (boundary loops)
    unsigned* loop_size;      // [max(V, 1)]
    unsigned* refd;           // [max(V, 1)] 1 = in a proper face
    Slot* table;              // [slots]
    size_t table_off, bytes;
};
static Workspace carve(void* base, unsigned V, unsigned F, size_t slots) {
    Workspace w{};
    Carver c(base);
    const size_t nh = F ? 3 * (size_t)F : 1, nv = V ? V : 1;
    w.slot_of = c.take<unsigned>(nh);
    w.parent_c = c.take<unsigned>(nh);
    w.parent_v = c.take<unsigned>(nv);
    w.loop_size = c.take<unsigned>(nv);
    w.refd = c.take<unsigned>(nv);
    w.table_off = c.off;
    w.table = c.take<Slot>(slots);
    w.bytes = c.off;
    return w;
}

__global__ void __launch_bounds__(256) k_mt_init(Slot* __restrict__ table, size_t slots, unsigned* __restrict__ parent_c, unsigned n_he,
                                                 unsigned* __restrict__ parent_v, unsigned* __restrict__ loop_size, unsigned V) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < slots) et::init_slot(table, i);
    if (i < n_he) parent_c[i] = (unsigned)i;
    if (i < V) { parent_v[i] = (unsigned)i; loop_size[i] = 0u; }
}

__global__ void __launch_bounds__(256) k_mt_insert(const int* __restrict__ faces, unsigned F, unsigned V, Slot* table, size_t mask,
                                                   unsigned* __restrict__ slot_of, unsigned* __restrict__ info) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    bool proper = false, degenerate = false, bad = false;
    unsigned v[3] = {0u, 0u, 0u};
    if (f < F) {
        const int* t = faces + 3 * (size_t)f;
        v[0] = (unsigned)t[0]; v[1] = (unsigned)t[1]; v[2] = (unsigned)t[2];      // a negative index is >= 2^31 > V as unsigned
        bad = v[0] >= V || v[1] >= V || v[2] >= V;
        degenerate = !bad && (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]);
        proper = !bad && !degenerate;
    }
    tally(proper, info + I_PROPER);
    tally(degenerate, info + I_DEGENERATE);
    tally(bad, info + I_BAD);
    if (f >= F) return;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const unsigned he = 3u * f + (unsigned)i;
        unsigned slot = NOSLOT;
        if (proper) {
            slot = et::insert(table, mask, v[i], v[(i + 1) % 3], he);
            if (slot == NOSLOT) atomicOr(info + I_OVERFLOW, 1u);
        }
        slot_of[he] = slot;
    }
}

__global__ void __launch_bounds__(256) k_mt_resolve(const int* __restrict__ faces, const Slot* __restrict__ table, size_t slots,
                                                    const unsigned* __restrict__ slot_of, unsigned n_he, unsigned V, int* __restrict__ twin,
                                                    unsigned* __restrict__ edge_uses, unsigned* parent_c, unsigned* parent_v,
                                                    unsigned* __restrict__ info) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    bool owner = false, boundary = false, flipped = false, nonmanifold = false;
    if (he < n_he) {
        const unsigned s = slot_of[he];
        int tw = -4;
        unsigned n = 0u;
        if (s < slots) {
            const Slot e = table[s];
            const unsigned a = (unsigned)(e.key >> 32), b = (unsigned)e.key;
            const int dir = (unsigned)faces[he] != a;                            // this half-edge runs b -> a
            const int odir = e.minh[1] < e.minh[0];                               // the direction of the smallest id (NONE is the largest value)
            const unsigned oh = e.minh[odir];
            n = e.cnt[0] + e.cnt[1];
            owner = oh == he;
            if (n == 1u) {
                tw = -1;
                boundary = true;
                if (a < V && b < V) uf::unite(parent_v, a, b);
            } else if (n == 2u) {
                if (e.cnt[0] == 1u && e.cnt[1] == 1u) tw = (int)e.minh[1 - dir];
                else { tw = -2; flipped = owner; }
                if (!owner && oh < n_he) {
                    // corner at a / at b of this half-edge's face and of the owner's: a half-edge is the corner at its origin
                    const unsigned nx = next_in_face(he), onx = next_in_face(oh);
                    uf::unite(parent_c, dir ? nx : he, odir ? onx : oh);
                    uf::unite(parent_c, dir ? he : nx, odir ? oh : onx);
                }
            } else {
                tw = -3;
                nonmanifold = owner;
            }
            boundary = boundary && owner;
        }
        twin[he] = tw;
        edge_uses[he] = n;
    }
    tally(owner, info + I_EDGES);
    tally(boundary, info + I_BOUNDARY);
    tally(flipped, info + I_FLIPPED);
    tally(nonmanifold, info + I_NONMANIFOLD);
}

__global__ void __launch_bounds__(256) k_mt_roots(const int* __restrict__ faces, const Slot* __restrict__ table, size_t slots,
                                                  const unsigned* __restrict__ slot_of, unsigned n_he, unsigned V, const unsigned* parent_c,
                                                  const unsigned* parent_v, unsigned* __restrict__ vertex_fans, unsigned* __restrict__ loop_size) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    if (he >= n_he) return;
    const unsigned s = slot_of[he];
    if (s >= slots) return;                                                       // not a corner of a proper face
    if (uf::find(parent_c, he) == he) {
        const unsigned v = (unsigned)faces[he];
        if (v < V) atomicAdd(vertex_fans + v, 1u);
    }
    const Slot e = table[s];
    if (e.cnt[0] + e.cnt[1] == 1u) {
        const unsigned a = (unsigned)(e.key >> 32);
        if (a < V) atomicAdd(loop_size + uf::find(parent_v, a), 1u);               // a root is <= a < V
    }
}

__global__ void __launch_bounds__(256) k_mt_vertex(const unsigned* __restrict__ vertex_fans, const unsigned* __restrict__ loop_size, unsigned V,
                                                   unsigned* __restrict__ refd, unsigned* __restrict__ info) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    unsigned fans = 0u, loop = 0u;
    if (v < V) {
        fans = vertex_fans[v];
        loop = loop_size[v];
        refd[v] = fans > 0u ? 1u : 0u;
        if (loop) atomicMax(info + I_LONGEST, loop);                               // one per boundary loop
    }
    tally(fans > 0u, info + I_REFERENCED);
    tally(fans > 1u, info + I_BOWTIE);
    tally(loop > 0u, info + I_LOOPS);
}

// ---- per-component sums -------------------------------------------------------------------------------------------------------------------------

// counts[label][col] += 1 for every pending lane, equal labels combined: every lane of the wave runs the loop (the ballots are wave-wide); each
// round retires the first pending lane and every lane with its label: at most 64 rounds, one for nearly every wave.
__device__ __forceinline__ void count_by_label(bool pending, unsigned lab, unsigned* __restrict__ counts, int col) {
    const int lane = threadIdx.x & 63;
    for (;;) {
        const unsigned long long m = __ballot(pending);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const unsigned ll = __shfl(lab, leader, 64);
        const bool mine = pending && lab == ll;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(counts + 6 * (size_t)ll + col, (unsigned)__popcll(same));
        if (mine) pending = false;
    }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__global__ void __launch_bounds__(256) k_cs_vertex(const int* __restrict__ label, const unsigned* __restrict__ refd, unsigned V,
                                                   unsigned* __restrict__ counts) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    unsigned lab = 0u;
    bool pending = false;
    if (v < V) {
        lab = (unsigned)label[v];
        pending = refd[v] != 0u && lab < V;                                        // a label is a vertex index: nothing is written outside counts
    }
    count_by_label(pending, lab, counts, 0);
}

// area and volume terms of the header, in its operation order
__global__ void __launch_bounds__(256) k_cs_face(const float* __restrict__ verts, const int* __restrict__ faces, unsigned F, unsigned V,
                                                 const int* __restrict__ label, unsigned* __restrict__ counts, double* __restrict__ measure) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned lab = 0u;
    bool pending = false;
    double area = 0.0, vol = 0.0;
    if (f < F) {
        const int* t = faces + 3 * (size_t)f;
        const unsigned ia = (unsigned)t[0], ib = (unsigned)t[1], ic = (unsigned)t[2];
        if (ia < V && ib < V && ic < V && ia != ib && ib != ic && ia != ic) {
            lab = (unsigned)label[ia];
            pending = lab < V;
            const float* pa = verts + 3 * (size_t)ia;
            const float* pb = verts + 3 * (size_t)ib;
            const float* pc = verts + 3 * (size_t)ic;
            const double a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2], c0 = pc[0], c1 = pc[1], c2 = pc[2];
            const double ux = b0 - a0, uy = b1 - a1, uz = b2 - a2, wx = c0 - a0, wy = c1 - a1, wz = c2 - a2;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
            const double cx = b1 * c2 - b2 * c1, cy = b2 * c0 - b0 * c2, cz = b0 * c1 - b1 * c0;
            vol = ((a0 * cx + a1 * cy) + a2 * cz) / 6.0;
        }
    }
    // as count_by_label, with the two fp64 sums of the lanes that share the leader's label (a fixed tree over the wave), then one atomicAdd each
    for (;;) {
        const unsigned long long m = __ballot(pending);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const unsigned ll = __shfl(lab, leader, 64);
        const bool mine = pending && lab == ll;
        const unsigned long long same = __ballot(mine);
        const double sa = wave_sum(mine ? area : 0.0), sv = wave_sum(mine ? vol : 0.0);
        if (lane == leader) {
            atomicAdd(counts + 6 * (size_t)ll + 2, (unsigned)__popcll(same));
            atomicAdd(measure + 2 * (size_t)ll, sa);
            atomicAdd(measure + 2 * (size_t)ll + 1, sv);
        }
        if (mine) pending = false;
    }
}

__global__ void __launch_bounds__(256) k_cs_edge(const Slot* __restrict__ table, size_t slots, const unsigned* __restrict__ slot_of, unsigned n_he,
                                                 unsigned V, const int* __restrict__ label, unsigned* __restrict__ counts) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    unsigned lab = 0u, n = 0u;
    bool owner = false, opposite = false;
    if (he < n_he) {
        const unsigned s = slot_of[he];
        if (s < slots) {
            const Slot e = table[s];
            const unsigned a = (unsigned)(e.key >> 32);                            // the edge's first vertex
            n = e.cnt[0] + e.cnt[1];
            opposite = e.cnt[0] == 1u && e.cnt[1] == 1u;
            if (a < V) {
                lab = (unsigned)label[a];
                owner = (e.minh[1] < e.minh[0] ? e.minh[1] : e.minh[0]) == he && lab < V;
            }
        }
    }
    count_by_label(owner, lab, counts, 1);
    count_by_label(owner && n == 1u, lab, counts, 3);
    count_by_label(owner && n == 2u && !opposite, lab, counts, 4);
    count_by_label(owner && n > 2u, lab, counts, 5);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------

static int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (ws_bytes < need || ((size_t)ws & 15)) {
        set_last_error((std::string(who) + ": workspace smaller than nerfart_mesh_topology_workspace_bytes() or not 16-byte aligned").c_str());
        return 2;
    }
    return 0;
}

}  // namespace mt
}  // namespace nerfart

using namespace nerfart;

extern "C" {

size_t nerfart_mesh_topology_workspace_bytes(unsigned V, unsigned F, int table_log2) {
    if (mt::check_sizes("mesh_topology_workspace_bytes", V, F)) return 0;
    const int k = mt::resolve_log2("mesh_topology_workspace_bytes", F, table_log2);
    if (!k) return 0;
    return mt::carve(nullptr, V, F, (size_t)1 << k).bytes;
}

int nerfart_mesh_half_edges(const int* faces, unsigned F, unsigned V, int table_log2, void* ws, size_t ws_bytes, int* twin, unsigned* edge_uses,
                            unsigned* vertex_fans, unsigned* info, void* stream) {
    if (!ws || !info || (F && (!faces || !twin || !edge_uses)) || (V && !vertex_fans)) { set_last_error("mesh_half_edges: null pointer"); return 2; }
    if (int rc = mt::check_sizes("mesh_half_edges", V, F)) return rc;
    const int k = mt::resolve_log2("mesh_half_edges", F, table_log2);
    if (!k) return 2;
    const size_t slots = (size_t)1 << k;
    if (int rc = mt::check_workspace("mesh_half_edges", ws, ws_bytes, mt::carve(nullptr, V, F, slots).bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const mt::Workspace w = mt::carve(ws, V, F, slots);
    const unsigned n_he = 3u * F;
    NERFART_HIP(hipMemsetAsync(info, 0, 16 * sizeof(unsigned), st));
    if (V) NERFART_HIP(hipMemsetAsync(vertex_fans, 0, (size_t)V * sizeof(unsigned), st));
    const size_t n_init = slots > n_he ? (slots > V ? slots : V) : (n_he > V ? n_he : V);
    hipLaunchKernelGGL(mt::k_mt_init, mt::blocks256(n_init), dim3(256), 0, st, w.table, slots, w.parent_c, n_he, w.parent_v, w.loop_size, V);
    NERFART_HIP(hipGetLastError());
    if (F) {                                         // V == 0: every face is bad; these index faces and the [3 F] arrays only
        hipLaunchKernelGGL(mt::k_mt_insert, mt::blocks256(F), dim3(256), 0, st, faces, F, V, w.table, slots - 1, w.slot_of, info);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mt::k_mt_resolve, mt::blocks256(n_he), dim3(256), 0, st, faces, (const mt::Slot*)w.table, slots, (const unsigned*)w.slot_of,
                           n_he, V, twin, edge_uses, w.parent_c, w.parent_v, info);
        NERFART_HIP(hipGetLastError());
        if (V) {
            hipLaunchKernelGGL(mt::k_mt_roots, mt::blocks256(n_he), dim3(256), 0, st, faces, (const mt::Slot*)w.table, slots,
                               (const unsigned*)w.slot_of, n_he, V, (const unsigned*)w.parent_c, (const unsigned*)w.parent_v, vertex_fans, w.loop_size);
            NERFART_HIP(hipGetLastError());
        }
    }
    if (V) {
        hipLaunchKernelGGL(mt::k_mt_vertex, mt::blocks256(V), dim3(256), 0, st, (const unsigned*)vertex_fans, (const unsigned*)w.loop_size, V, w.refd,
                           info);
        NERFART_HIP(hipGetLastError());
    }
    return 0;
}

int nerfart_mesh_component_stats(const float* verts, const int* faces, unsigned F, unsigned V, const int* label, const void* ws, size_t ws_bytes,
                                 unsigned* counts, double* measure, void* stream) {
    if (!ws || (F && !faces) || (V && (!verts || !label || !counts || !measure))) { set_last_error("mesh_component_stats: null pointer"); return 2; }
    if ((size_t)measure & 7) { set_last_error("mesh_component_stats: measure must be 8-byte aligned"); return 2; }
    if (int rc = mt::check_sizes("mesh_component_stats", V, F)) return rc;
    const int least = mt::smallest_log2(F);
    if (least > mt::MAX_LOG2) { mt::resolve_log2("mesh_component_stats", F, 0); return 2; }
    if (int rc = mt::check_workspace("mesh_component_stats", ws, ws_bytes, mt::carve(nullptr, V, F, (size_t)1 << least).bytes)) return rc;
    if (V == 0) return 0;                            // counts and measure are empty
    hipStream_t st = (hipStream_t)stream;
    const mt::Workspace w = mt::carve(const_cast<void*>(ws), V, F, 0);
    size_t slots = (ws_bytes - w.table_off) / sizeof(mt::Slot);                    // no slot beyond the caller's bytes is read, whatever slot_of holds
    if (slots > ((size_t)1 << mt::MAX_LOG2)) slots = (size_t)1 << mt::MAX_LOG2;
    const unsigned n_he = 3u * F;
    NERFART_HIP(hipMemsetAsync(counts, 0, 6 * (size_t)V * sizeof(unsigned), st));
    NERFART_HIP(hipMemsetAsync(measure, 0, 2 * (size_t)V * sizeof(double), st));
    hipLaunchKernelGGL(mt::k_cs_vertex, mt::blocks256(V), dim3(256), 0, st, label, (const unsigned*)w.refd, V, counts);
    NERFART_HIP(hipGetLastError());
    if (F) {
        hipLaunchKernelGGL(mt::k_cs_face, mt::blocks256(F), dim3(256), 0, st, verts, faces, F, V, label, counts, measure);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mt::k_cs_edge, mt::blocks256(n_he), dim3(256), 0, st, (const mt::Slot*)w.table, slots, (const unsigned*)w.slot_of, n_he, V,
                           label, counts);
        NERFART_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
