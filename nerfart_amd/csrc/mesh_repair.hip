// mesh_repair.hip - cut and stitch of the non-manifold edges of an indexed triangle mesh (mesh_util.repair_manifold, extract_mesh(repair=)): the
// output has no non-manifold edge and no bow-tie vertex, and no triangle's geometry changes but for a few splits at an edge midpoint.  The
// rules - cancel, radial pairing, corner classes, multi-edges, subdivision - are in include/nerfart_hip.h; tests/mesh_repair_ref.py states them
// in numpy.  Everything but the midpoints is integers, the midpoints one fp32 add and one multiply: every output is defined uniquely and
// depends neither on the order of work nor on the size of the edge table.
//
// COUNT (nerfart_mesh_repair_count), every kernel 256 threads, one thread per item:
//   k_mr_init      per index: edge table empty, corner parents = themselves, unit_min[h] = h.
//   k_mr_cancel    per face: bad / degenerate tallied; a proper face enters the CANCEL TABLE, open addressing over T = the power of two >= 2 F
//                  slots of face indices keyed on the sorted triple - a slot goes from EMPTY to f by atomicCAS, an occupied slot is compared
//                  through its occupant's sorted triple, equal: atomicMin, as csrc/mesh_simplify.hip's duplicate table -, counts its orientation
//                  (atomicAdd) and links itself into the slot's list (atomicExch on the head).  The list is a SET: its order is never used.
//   k_mr_alive     per face: p, q of its slot; the |p - q| first faces of the majority survive.  Only a face of a mixed majority (both counts
//                  non-zero and different) walks the list, at most p + q steps, to count the same-orientation faces before it.
//   k_mr_insert    per face: the three half-edges of a surviving face enter the edge table (csrc/edge_table.h).
//   k_mr_resolve   per half-edge: across an edge with n == 2 the corners are united with the owner's (csrc/union_find.h); n > 2 is tallied.
//   k_mr_scan_nm   scan (csrc/pair_scan.h) over the half-edges of (n, 1) at the owner of every edge with 2 < n <= 64: CSR offsets.
//   k_mr_fill      per half-edge of such an edge: its id into the edge's CSR segment, at a position an atomicAdd hands out - the next kernel
//                  sorts the segment, so that order is never seen.
//   k_mr_pair      per such edge (its owner's thread; an edge has at most 64 half-edges, everything lives in the edge's own CSR segment of
//                  the workspace - no scratch): ids ascending by counting; (x, y) of every half-edge in fp64, the header's operation order, no
//                  contraction; position in angular order = the number of half-edges that compare before it (ties to the smaller id), so the
//                  result is defined even where rounding makes the comparison intransitive; bracket matching over two turns of the cycle with
//                  a stack in the segment; every pair's corners united, unit_min of both = the smaller id.
//   k_mr_roots / scan over the vertices / k_mr_vfill / k_mr_vrank: classes per vertex, their base by scan, the class roots of a vertex into its
//                  CSR segment (atomics), cls[root] = base + the number of smaller roots in the segment: ascending (vertex, smallest corner).
//   k_mr_multi     per edge with 2 < n <= 64: the class pair of every unit; a unit is subdivided when a unit with a smaller id has its pair.
//   scan over the half-edges (subdivided unit at its smallest id), scan over the faces (survives, subdivided half-edges), k_mr_totals.
// EMIT (nerfart_mesh_repair_emit) after the caller has read counts: k_mr_emit_verts per corner (class vertices, midpoints, src_vertex,
// mid_ends), k_mr_emit_faces per face (the fan).  Positions come from the scans: no atomic decides one.
//
// Every loop is bounded whatever the faces hold - probe sequences by the tables' sizes, list walks by the slot's counts, the per-edge loops by
// 64, the union-finds by the indices.  No workgroup waits for another.  Every write is checked against the caller's sizes, every index read
// from the workspace against the array it enters.
#include "edge_table.h"
#include "pair_scan.h"
#include "union_find.h"

#pragma clang fp contract(off)

namespace nerfart {
namespace mr {

using et::Slot; using et::NOSLOT; using et::tally; using et::next_in_face; using et::blocks256;

constexpr unsigned EMPTY = 0xFFFFFFFFu;      // of a cancel-table slot, a list end, cslot[f]
constexpr unsigned WIDE = 64u;               // an edge with more half-edges is left unpaired
// info [16]
enum { I_BAD = 0, I_DEGENERATE, I_CANCELLED, I_NONMANIFOLD, I_PAIRED, I_UNPAIRED, I_WIDE, I_SPLIT, I_SUBDIVIDED, I_TIES, I_OVERFLOW };
// tot [8] in the workspace: the totals of the four scans
enum { T_CSR = 0, T_NM, T_V1, T_REF, T_M, T_UNUSED, T_FA, T_FX };

// the workspace, carved in this order (each buffer rounded up to 256 bytes); nh = max(3 F, 1), nf = max(F, 1), nv = max(V, 1); the edge table
// comes last
struct Workspace {
    unsigned* tot;            // [8]
    unsigned* ctab;           // [T] cancel table: the smallest face index of the key
    unsigned* ccnt;           // [T][2] faces of the key per orientation
    unsigned* chead;          // [T] list head
    unsigned* cnext;          // [nf]
    unsigned* cslot;          // [nf]
    unsigned* alive;          // [nf]
    unsigned* slot_of;        // [nh]
    unsigned* parent_c;       // [nh]
    unsigned* off_he;         // [nh][2] scan over the half-edges: first the CSR offsets, later the subdivided units
    PairScanLevels lvl_he;
    unsigned* cursor;         // [nh] by owner
    unsigned* list;           // [nh] CSR: half-edge ids, ascending within an edge after k_mr_pair
    unsigned* seq;            // [nh] CSR: the same in angular order
    unsigned* rnk;            // [nh] CSR: rank, then matched flag, then class at a
    unsigned* stk;            // [nh] CSR: the stack, then class at b
    double* ang;              // [nh][2] CSR: (x, y)
    unsigned* unit_min;       // [nh] the smallest half-edge id of the half-edge's unit
    unsigned* sub;            // [nh] 1 at the smallest id of a subdivided unit
    unsigned* cls;            // [nh] at a class root: the output vertex
    unsigned* vlist;          // [nh] CSR by vertex: class roots
    unsigned* vcount;         // [nv]
    unsigned* vcursor;        // [nv]
    unsigned* off_v;          // [nv][2]
    PairScanLevels lvl_v;
    unsigned* off_f;          // [nf][2]
    PairScanLevels lvl_f;
    Slot* table;              // [slots]
    unsigned T;
    size_t nh, nf, nv, bytes;
};
static unsigned cancel_slots(unsigned F) { unsigned t = 2; while (t < 2u * F) t <<= 1; return t; }      // 3 F + 1 <= 2^31: 2 F < 2^31
static Workspace carve(void* base, unsigned V, unsigned F, size_t slots) {
    Workspace w{};
    Carver c(base);
    w.nh = F ? 3 * (size_t)F : 1; w.nf = F ? F : 1; w.nv = V ? V : 1;
    w.T = cancel_slots(F);
    w.tot = c.take<unsigned>(8);
    w.ctab = c.take<unsigned>(w.T);
    w.ccnt = c.take<unsigned>(2 * (size_t)w.T);
    w.chead = c.take<unsigned>(w.T);
    w.cnext = c.take<unsigned>(w.nf);
    w.cslot = c.take<unsigned>(w.nf);
    w.alive = c.take<unsigned>(w.nf);
    w.slot_of = c.take<unsigned>(w.nh);
    w.parent_c = c.take<unsigned>(w.nh);
    w.off_he = c.take<unsigned>(2 * w.nh);
    pair_scan_carve(c, w.nh, w.lvl_he);
    w.cursor = c.take<unsigned>(w.nh);
    w.list = c.take<unsigned>(w.nh);
    w.seq = c.take<unsigned>(w.nh);
    w.rnk = c.take<unsigned>(w.nh);
    w.stk = c.take<unsigned>(w.nh);
    w.ang = c.take<double>(2 * w.nh);
    w.unit_min = c.take<unsigned>(w.nh);
    w.sub = c.take<unsigned>(w.nh);
    w.cls = c.take<unsigned>(w.nh);
    w.vlist = c.take<unsigned>(w.nh);
    w.vcount = c.take<unsigned>(w.nv);
    w.vcursor = c.take<unsigned>(w.nv);
    w.off_v = c.take<unsigned>(2 * w.nv);
    pair_scan_carve(c, w.nv, w.lvl_v);
    w.off_f = c.take<unsigned>(2 * w.nf);
    pair_scan_carve(c, w.nf, w.lvl_f);
    w.table = c.take<Slot>(slots);
    w.bytes = c.off;
    return w;
}

// the read-only view the kernels take by value
struct View {
    const int* faces;
    const Slot* table;
    const unsigned* slot_of;
    size_t slots;
    unsigned n_he, V, F;
};

// The sorted triple of face f and whether the face is an odd permutation of it; false for a face that is not proper.
__device__ __forceinline__ bool sorted_triple(const int* __restrict__ faces, unsigned V, unsigned f, unsigned& a, unsigned& b, unsigned& c, int& odd,
                                              bool& bad) {
    const int* t = faces + 3 * (size_t)f;
    const unsigned x = (unsigned)t[0], y = (unsigned)t[1], z = (unsigned)t[2];            // a negative index is >= 2^31 > V as unsigned
    bad = x >= V || y >= V || z >= V;
    if (bad || x == y || y == z || x == z) return false;
    // rotate the smallest to the front (the orientation is kept), then the face is even iff the other two ascend
    unsigned p = x, q = y, r = z;
    if (y < x && y < z) { p = y; q = z; r = x; }
    else if (z < x && z < y) { p = z; q = x; r = y; }
    odd = q > r;
    a = p; b = odd ? r : q; c = odd ? q : r;
    return true;
}

__device__ __forceinline__ unsigned triple_hash(unsigned a, unsigned b, unsigned c) {
    unsigned h = a * 0x9E3779B1u ^ b * 0x85EBCA77u ^ c * 0xC2B2AE3Du;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
    return h;
}

__global__ void __launch_bounds__(256) k_mr_init(Slot* __restrict__ table, size_t slots, unsigned* __restrict__ parent_c,
                                                 unsigned* __restrict__ unit_min, unsigned n_he) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < slots) et::init_slot(table, i);
    if (i < n_he) { parent_c[i] = (unsigned)i; unit_min[i] = (unsigned)i; }
}

__global__ void __launch_bounds__(256) k_mr_cancel(const int* __restrict__ faces, unsigned F, unsigned V, unsigned* ctab, unsigned T, unsigned* ccnt,
                                                   unsigned* chead, unsigned* __restrict__ cnext, unsigned* __restrict__ cslot,
                                                   unsigned* __restrict__ info) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    unsigned a = 0, b = 0, c = 0;
    int odd = 0;
    bool bad = false, proper = false;
    if (f < F) proper = sorted_triple(faces, V, f, a, b, c, odd, bad);
    tally(f < F && bad, info + I_BAD);
    tally(f < F && !bad && !proper, info + I_DEGENERATE);
    if (f >= F) return;
    unsigned mine = EMPTY;
    if (proper) {
        unsigned h = triple_hash(a, b, c) & (T - 1);
        // BOUND: T probes.  At most F <= T / 2 slots are ever occupied, so an empty slot - or this key's - is met before the probes wrap around.
        for (unsigned probe = 0; probe < T; ++probe, h = (h + 1) & (T - 1)) {
            const unsigned cur = atomicCAS(ctab + h, EMPTY, f);
            if (cur == EMPTY) { mine = h; break; }
            unsigned oa, ob, oc;
            int oodd;
            bool obad;
            // cur < F is a proper face (nothing else is ever stored); a concurrent atomicMin replaces it by a face of the same key
            if (cur < F && sorted_triple(faces, V, cur, oa, ob, oc, oodd, obad) && oa == a && ob == b && oc == c) {
                atomicMin(ctab + h, f);
                mine = h;
                break;
            }
        }
        if (mine == EMPTY) {
            atomicOr(info + I_OVERFLOW, 1u);                                  // cannot happen (the bound above); never silent
        } else {
            atomicAdd(ccnt + 2 * (size_t)mine + odd, 1u);
            cnext[f] = atomicExch(chead + mine, f);
        }
    }
    cslot[f] = mine;
}

__global__ void __launch_bounds__(256) k_mr_alive(const int* __restrict__ faces, unsigned F, unsigned V, unsigned T, const unsigned* __restrict__ ccnt,
                                                  const unsigned* __restrict__ chead, const unsigned* __restrict__ cnext,
                                                  const unsigned* __restrict__ cslot, unsigned* __restrict__ alive, unsigned* __restrict__ info) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    bool cancelled = false;
    if (f < F) {
        const unsigned s = cslot[f];
        unsigned live = 0u;
        unsigned a, b, c;
        int odd;
        bool bad;
        if (s < T && sorted_triple(faces, V, f, a, b, c, odd, bad)) {
            const unsigned mine = ccnt[2 * (size_t)s + odd], other = ccnt[2 * (size_t)s + 1 - odd];
            if (mine > other) {
                const unsigned keep = mine - other;
                unsigned before = 0u;
                if (other) {
                    // BOUND: the list holds mine + other faces; a step that leaves [0, F) ends the walk
                    unsigned g = chead[s];
                    for (unsigned step = 0; step < mine + other && g < F; ++step, g = cnext[g]) {
                        unsigned ga, gb, gc;
                        int godd;
                        bool gbad;
                        if (g < f && sorted_triple(faces, V, g, ga, gb, gc, godd, gbad) && godd == odd) ++before;
                    }
                }
                live = before < keep ? 1u : 0u;
            }
            cancelled = !live;
        }
        alive[f] = live;
    }
    tally(cancelled, info + I_CANCELLED);
}

__global__ void __launch_bounds__(256) k_mr_insert(const int* __restrict__ faces, unsigned F, const unsigned* __restrict__ alive, Slot* table,
                                                   size_t mask, unsigned* __restrict__ slot_of, unsigned* __restrict__ info) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F) return;
    const bool live = alive[f] != 0u;                                          // a surviving face is proper
    const int* t = faces + 3 * (size_t)f;
    const unsigned v[3] = {(unsigned)t[0], (unsigned)t[1], (unsigned)t[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const unsigned he = 3u * f + (unsigned)i;
        unsigned slot = NOSLOT;
        if (live) {
            slot = et::insert(table, mask, v[i], v[(i + 1) % 3], he);
            if (slot == NOSLOT) atomicOr(info + I_OVERFLOW, 1u);
        }
        slot_of[he] = slot;
    }
}

// what a half-edge knows of its edge
struct Edge {
    unsigned a, b, n, owner;      // {a < b}, its half-edges, the smallest id among them
    int dir, odir;                // this half-edge / the owner runs b -> a
    bool ok;                      // the half-edge belongs to a surviving face
};
__device__ __forceinline__ Edge edge_of(const View& m, unsigned he) {
    Edge e{};
    if (he >= m.n_he) return e;
    const unsigned s = m.slot_of[he];
    if (s >= m.slots) return e;
    const Slot t = m.table[s];
    e.a = (unsigned)(t.key >> 32); e.b = (unsigned)t.key;
    e.n = t.cnt[0] + t.cnt[1];
    e.dir = (unsigned)m.faces[he] != e.a;
    e.odir = t.minh[1] < t.minh[0];                                            // NONE is the largest value
    e.owner = t.minh[e.odir];
    e.ok = e.a < m.V && e.b < m.V && e.owner < m.n_he;
    return e;
}
__device__ __forceinline__ bool pairable(const Edge& e) { return e.ok && e.n > 2u && e.n <= WIDE; }

// the corners at a / at b of the face of half-edge h, which runs a -> b (dir 0) or b -> a (dir 1): a half-edge is the corner at its origin
__device__ __forceinline__ unsigned corner_a(unsigned h, int dir) { return dir ? next_in_face(h) : h; }
__device__ __forceinline__ unsigned corner_b(unsigned h, int dir) { return dir ? h : next_in_face(h); }

__global__ void __launch_bounds__(256) k_mr_resolve(View m, unsigned* parent_c, unsigned* __restrict__ info) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    const Edge e = edge_of(m, he);
    bool owner = false;
    if (e.ok) {
        owner = e.owner == he;
        if (e.n == 2u && !owner) {
            uf::unite(parent_c, corner_a(he, e.dir), corner_a(e.owner, e.odir));
            uf::unite(parent_c, corner_b(he, e.dir), corner_b(e.owner, e.odir));
        }
    }
    tally(owner && e.n > 2u, info + I_NONMANIFOLD);
    tally(owner && e.n > WIDE, info + I_WIDE);
    tally(e.ok && e.n > WIDE, info + I_UNPAIRED);
}

__global__ void __launch_bounds__(256) k_mr_scan_nm(View m, uint2* __restrict__ off, uint2* __restrict__ sums) {
    pair_scan_block([&](size_t i) {
        const Edge e = edge_of(m, (unsigned)i);
        return pairable(e) && e.owner == (unsigned)i ? make_uint2(e.n, 1u) : make_uint2(0u, 0u);
    }, off, m.n_he, sums);
}

__global__ void __launch_bounds__(256) k_mr_fill(View m, const uint2* __restrict__ off, unsigned* cursor, unsigned* __restrict__ list) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    const Edge e = edge_of(m, he);
    if (!pairable(e)) return;
    const unsigned k = atomicAdd(cursor + e.owner, 1u);
    const size_t pos = (size_t)off[e.owner].x + k;
    if (k < e.n && pos < m.n_he) list[pos] = he;
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 sub3(const D3& p, const D3& q) { return D3{p.x - q.x, p.y - q.y, p.z - q.z}; }
__device__ __forceinline__ D3 cross3(const D3& p, const D3& q) { return D3{p.y * q.z - p.z * q.y, p.z * q.x - p.x * q.z, p.x * q.y - p.y * q.x}; }
__device__ __forceinline__ double dot3(const D3& p, const D3& q) { return (p.x * q.x + p.y * q.y) + p.z * q.z; }
__device__ __forceinline__ D3 load3(const float* __restrict__ verts, unsigned v) {
    const float* p = verts + 3 * (size_t)v;
    return D3{(double)p[0], (double)p[1], (double)p[2]};
}

// does the half-edge at position i of the segment come before the one at position j (positions in ascending id order)?
__device__ __forceinline__ bool comes_before(const double* __restrict__ ang, unsigned i, unsigned j, bool& tie) {
    const double xi = ang[2 * (size_t)i], yi = ang[2 * (size_t)i + 1], xj = ang[2 * (size_t)j], yj = ang[2 * (size_t)j + 1];
    const bool si = yi < 0.0 || (yi == 0.0 && xi < 0.0), sj = yj < 0.0 || (yj == 0.0 && xj < 0.0);
    tie = false;
    if (si != sj) return sj;
    const double c = xi * yj - xj * yi;
    if (c > 0.0) return true;
    if (c < 0.0) return false;
    tie = true;
    return i < j;
}

// One thread per edge with 2 < n <= 64, the thread of its owner.  The arrays list, seq, rnk, stk, ang are touched in [start, start + n) only:
// the edge's own CSR segment.
__global__ void __launch_bounds__(256) k_mr_pair(View m, const float* __restrict__ verts, int solid, const uint2* __restrict__ off,
                                                 unsigned* __restrict__ list, unsigned* __restrict__ seq, unsigned* __restrict__ rnk,
                                                 unsigned* __restrict__ stk, double* __restrict__ ang, unsigned* parent_c,
                                                 unsigned* __restrict__ unit_min, unsigned* __restrict__ info) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    const Edge e = edge_of(m, he);
    if (!pairable(e) || e.owner != he) return;
    const unsigned n = e.n;
    const size_t start = off[he].x;
    if (start + n > m.n_he) return;
    unsigned* L = list + start; unsigned* S = seq + start; unsigned* R = rnk + start; unsigned* K = stk + start;
    double* A = ang + 2 * start;
    // every entry must be a half-edge of this edge (a workspace that is not this mesh's stops here)
    for (unsigned i = 0; i < n; ++i) {
        const Edge o = edge_of(m, L[i]);
        if (!o.ok || o.a != e.a || o.b != e.b) return;
    }
    // 1. ids ascending: position = the number of smaller ids (the ids are distinct)
    for (unsigned i = 0; i < n; ++i) {
        const unsigned h = L[i];
        unsigned pos = 0u;
        for (unsigned j = 0; j < n; ++j) pos += L[j] < h;
        if (pos < n) S[pos] = h;
    }
    for (unsigned i = 0; i < n; ++i) L[i] = S[i];
    // 2. (x, y) of every apex in the frame of the smallest id
    const D3 va = load3(verts, e.a);
    const D3 d = sub3(load3(verts, e.b), va);
    D3 u1{}, u2{};
    for (unsigned i = 0; i < n; ++i) {
        const unsigned apex = (unsigned)m.faces[next_in_face(next_in_face(L[i]))];
        const D3 w = apex < m.V ? sub3(load3(verts, apex), va) : D3{0.0, 0.0, 0.0};
        if (i == 0u) {
            u1 = cross3(d, w);
            u2 = cross3(d, u1);
            A[0] = 1.0; A[1] = 0.0;
        } else {
            A[2 * i] = -dot3(w, u2);
            A[2 * i + 1] = dot3(w, u1);
        }
    }
    // 3. rank = the number of half-edges that come before; a tie is counted once per unordered pair
    unsigned ties = 0u;
    for (unsigned i = 0; i < n; ++i) {
        unsigned r = 0u;
        for (unsigned j = 0; j < n; ++j) {
            if (j == i) continue;
            bool tie;
            r += comes_before(A, j, i, tie);
            ties += tie && j < i;
        }
        R[i] = r;
    }
    // 4. angular order: ascending (rank, id)
    for (unsigned i = 0; i < n; ++i) {
        unsigned pos = 0u;
        for (unsigned j = 0; j < n; ++j) pos += R[j] < R[i] || (R[j] == R[i] && j < i);
        if (pos < n) S[pos] = L[i];
    }
    // 5. brackets over two turns of the cycle: R = matched flag by position in S, K = the stack of positions
    for (unsigned i = 0; i < n; ++i) R[i] = 0u;
    unsigned depth = 0u, pairs = 0u;
    for (unsigned t = 0; t < 2u * n; ++t) {
        const unsigned p = t < n ? t : t - n;
        if (R[p]) continue;
        const unsigned h = S[p];
        const int dir = (unsigned)m.faces[h] != e.a;
        const bool opens = solid ? dir == 1 : dir == 0;
        if (opens) {
            if (t < n && depth < n) K[depth++] = p;
        } else if (depth) {
            const unsigned q = K[--depth];
            const unsigned ho = S[q];
            const int odir = 1 - dir;
            R[p] = R[q] = 1u;
            ++pairs;
            uf::unite(parent_c, corner_a(h, dir), corner_a(ho, odir));
            uf::unite(parent_c, corner_b(h, dir), corner_b(ho, odir));
            const unsigned lo = h < ho ? h : ho;
            unit_min[h] = lo; unit_min[ho] = lo;
        }
    }
    if (pairs) atomicAdd(info + I_PAIRED, 1u);
    if (n > 2u * pairs) atomicAdd(info + I_UNPAIRED, n - 2u * pairs);
    if (ties) atomicAdd(info + I_TIES, ties);
}

__device__ __forceinline__ bool is_root(const View& m, const unsigned* parent_c, unsigned he) {
    return he < m.n_he && m.slot_of[he] < m.slots && uf::find(parent_c, he) == he;
}

__global__ void __launch_bounds__(256) k_mr_roots(View m, const unsigned* parent_c, unsigned* vcount) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    if (!is_root(m, parent_c, he)) return;
    const unsigned v = (unsigned)m.faces[he];
    if (v < m.V) atomicAdd(vcount + v, 1u);
}

__global__ void __launch_bounds__(256) k_mr_scan_v(const unsigned* __restrict__ vcount, unsigned V, uint2* __restrict__ off, uint2* __restrict__ sums) {
    pair_scan_block([&](size_t i) { const unsigned k = vcount[i]; return make_uint2(k, k ? 1u : 0u); }, off, V, sums);
}

__global__ void __launch_bounds__(256) k_mr_vfill(View m, const unsigned* parent_c, const unsigned* __restrict__ vcount, const uint2* __restrict__ off_v,
                                                  unsigned* vcursor, unsigned* __restrict__ vlist) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    if (!is_root(m, parent_c, he)) return;
    const unsigned v = (unsigned)m.faces[he];
    if (v >= m.V) return;
    const unsigned k = atomicAdd(vcursor + v, 1u);
    const size_t pos = (size_t)off_v[v].x + k;
    if (k < vcount[v] && pos < m.n_he) vlist[pos] = he;
}

__global__ void __launch_bounds__(256) k_mr_vrank(View m, const unsigned* parent_c, const unsigned* __restrict__ vcount, const uint2* __restrict__ off_v,
                                                  const unsigned* __restrict__ vlist, unsigned* __restrict__ cls) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    if (!is_root(m, parent_c, he)) return;
    const unsigned v = (unsigned)m.faces[he];
    if (v >= m.V) return;
    const unsigned k = vcount[v];
    const size_t base = off_v[v].x;
    unsigned before = 0u;
    // BOUND: the classes at this vertex, at most its corners
    for (unsigned j = 0; j < k && base + j < m.n_he; ++j) before += vlist[base + j] < he;
    cls[he] = (unsigned)base + before;
}

// the output vertex of corner h (EMPTY when the workspace does not hold one)
__device__ __forceinline__ unsigned class_of(const View& m, const unsigned* parent_c, const unsigned* __restrict__ cls, unsigned h) {
    if (h >= m.n_he) return EMPTY;
    return cls[uf::find(parent_c, h)];
}

__global__ void __launch_bounds__(256) k_mr_multi(View m, const uint2* __restrict__ off, const unsigned* __restrict__ list, unsigned* __restrict__ rnk,
                                                  unsigned* __restrict__ stk, const unsigned* parent_c, const unsigned* __restrict__ cls,
                                                  const unsigned* __restrict__ unit_min, unsigned* __restrict__ sub) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    const Edge e = edge_of(m, he);
    if (!pairable(e) || e.owner != he) return;
    const unsigned n = e.n;
    const size_t start = off[he].x;
    if (start + n > m.n_he) return;
    const unsigned* L = list + start;
    unsigned* CA = rnk + start; unsigned* CB = stk + start;
    for (unsigned i = 0; i < n; ++i) {
        const unsigned h = L[i];
        const bool leader = h < m.n_he && unit_min[h] == h;
        const int dir = leader ? (unsigned)m.faces[h] != e.a : 0;
        CA[i] = leader ? class_of(m, parent_c, cls, corner_a(h, dir)) : EMPTY;
        CB[i] = leader ? class_of(m, parent_c, cls, corner_b(h, dir)) : EMPTY;
    }
    // L is ascending: a unit at a smaller position has the smaller id
    for (unsigned i = 1; i < n; ++i) {
        if (CA[i] == EMPTY) continue;
        bool taken = false;
        for (unsigned j = 0; j < i; ++j) taken = taken || (CA[j] == CA[i] && CB[j] == CB[i]);
        if (taken) sub[L[i]] = 1u;
    }
}

__global__ void __launch_bounds__(256) k_mr_scan_sub(const unsigned* __restrict__ sub, unsigned n_he, uint2* __restrict__ off, uint2* __restrict__ sums) {
    pair_scan_block([&](size_t i) { return make_uint2(sub[i] ? 1u : 0u, 0u); }, off, n_he, sums);
}

// is half-edge h subdivided, and by which midpoint (its number among the midpoints)?
__device__ __forceinline__ bool midpoint_of(const unsigned* __restrict__ unit_min, const unsigned* __restrict__ sub, const uint2* __restrict__ off_he,
                                            unsigned n_he, unsigned h, unsigned& mid) {
    const unsigned u = unit_min[h];
    if (u >= n_he || !sub[u]) return false;
    mid = off_he[u].x;
    return true;
}

__global__ void __launch_bounds__(256) k_mr_scan_f(const unsigned* __restrict__ alive, const unsigned* __restrict__ unit_min,
                                                   const unsigned* __restrict__ sub, unsigned F, unsigned n_he, uint2* __restrict__ off,
                                                   uint2* __restrict__ sums) {
    pair_scan_block([&](size_t f) {
        if (!alive[f]) return make_uint2(0u, 0u);
        unsigned k = 0u;
        for (unsigned i = 0; i < 3u; ++i) {
            const unsigned u = unit_min[3 * f + i];
            k += u < n_he && sub[u] ? 1u : 0u;
        }
        return make_uint2(1u, k);
    }, off, F, sums);
}

__global__ void k_mr_totals(const unsigned* __restrict__ tot, unsigned* __restrict__ counts, unsigned* __restrict__ info) {
    if (threadIdx.x || blockIdx.x) return;
    counts[0] = tot[T_V1]; counts[1] = tot[T_M]; counts[2] = tot[T_FA]; counts[3] = tot[T_FX];
    info[I_SPLIT] = tot[T_V1] - tot[T_REF];
    info[I_SUBDIVIDED] = tot[T_M];
}

// ---- emit -------------------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_mr_emit_verts(View m, const float* __restrict__ verts, const unsigned* parent_c, const unsigned* __restrict__ cls,
                                                       const unsigned* __restrict__ sub, const uint2* __restrict__ off_he,
                                                       const unsigned* __restrict__ tot, float* __restrict__ verts_out, int* __restrict__ src_vertex,
                                                       int* __restrict__ mid_ends, unsigned V_out, unsigned M_out) {
    const unsigned he = blockIdx.x * 256u + threadIdx.x;
    if (he >= m.n_he || m.slot_of[he] >= m.slots) return;
    const unsigned V1 = tot[T_V1];
    if (uf::find(parent_c, he) == he) {                                        // a class: one output vertex
        const unsigned c = cls[he], v = (unsigned)m.faces[he];
        if (c < V1 && c < V_out && v < m.V) {
            for (int k = 0; k < 3; ++k) verts_out[3 * (size_t)c + k] = verts[3 * (size_t)v + k];
            src_vertex[c] = (int)v;
        }
    }
    if (sub[he]) {                                                             // the smallest id of a subdivided unit: one midpoint
        const Edge e = edge_of(m, he);
        const unsigned mi = off_he[he].x;
        const size_t o = (size_t)V1 + mi;
        if (e.ok && mi < M_out && o < V_out) {
            const unsigned ca = class_of(m, parent_c, cls, corner_a(he, e.dir)), cb = class_of(m, parent_c, cls, corner_b(he, e.dir));
            mid_ends[2 * (size_t)mi] = (int)ca;
            mid_ends[2 * (size_t)mi + 1] = (int)cb;
            for (int k = 0; k < 3; ++k) verts_out[3 * o + k] = (verts[3 * (size_t)e.a + k] + verts[3 * (size_t)e.b + k]) * 0.5f;
            src_vertex[o] = -1;
        }
    }
}

__global__ void __launch_bounds__(256) k_mr_emit_faces(View m, const unsigned* __restrict__ alive, const unsigned* parent_c,
                                                       const unsigned* __restrict__ cls, const unsigned* __restrict__ unit_min,
                                                       const unsigned* __restrict__ sub, const uint2* __restrict__ off_he,
                                                       const uint2* __restrict__ off_f, const unsigned* __restrict__ tot, int* __restrict__ faces_out,
                                                       unsigned F_out) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= m.F || !alive[f]) return;
    const unsigned V1 = tot[T_V1], Fa = tot[T_FA];
    unsigned poly[6];
    int len = 0, at = -1;
    for (unsigned i = 0; i < 3u; ++i) {
        const unsigned h = 3u * f + i;
        poly[len++] = class_of(m, parent_c, cls, h);
        unsigned mid;
        if (midpoint_of(unit_min, sub, off_he, m.n_he, h, mid)) {
            if (at < 0) at = len;
            poly[len++] = V1 + mid;
        }
    }
    const uint2 o = off_f[f];
    if (at < 0) {
        if (o.x < F_out) { int* t = faces_out + 3 * (size_t)o.x; t[0] = (int)poly[0]; t[1] = (int)poly[1]; t[2] = (int)poly[2]; }
        return;
    }
    // the fan from the midpoint of the lowest subdivided half-edge: triangle j is (P0, Pj, Pj+1) of the polygon rotated to start there
    for (int j = 1; j + 1 < len; ++j) {
        const size_t dst = j == 1 ? (size_t)o.x : (size_t)Fa + o.y + (size_t)(j - 2);
        if (dst >= F_out) continue;
        int* t = faces_out + 3 * dst;
        t[0] = (int)poly[at % len]; t[1] = (int)poly[(at + j) % len]; t[2] = (int)poly[(at + j + 1) % len];
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------

static int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (ws_bytes < need || ((size_t)ws & 15)) {
        set_last_error((std::string(who) + ": workspace smaller than nerfart_mesh_repair_workspace_bytes() or not 16-byte aligned").c_str());
        return 2;
    }
    return 0;
}

static View view_of(const Workspace& w, const int* faces, unsigned V, unsigned F, size_t slots) {
    View m;
    m.faces = faces; m.table = w.table; m.slot_of = w.slot_of; m.slots = slots; m.n_he = 3u * F; m.V = V; m.F = F;
    return m;
}

}  // namespace mr
}  // namespace nerfart

using namespace nerfart;

extern "C" {

size_t nerfart_mesh_repair_workspace_bytes(unsigned V, unsigned F, int table_log2) {
    if (et::check_sizes("mesh_repair_workspace_bytes", V, F)) return 0;
    const int k = et::resolve_log2("mesh_repair_workspace_bytes", F, table_log2);
    if (!k) return 0;
    return mr::carve(nullptr, V, F, (size_t)1 << k).bytes;
}

int nerfart_mesh_repair_count(const float* verts, const int* faces, unsigned V, unsigned F, int wedge, int table_log2, void* ws, size_t ws_bytes,
                              unsigned* counts, unsigned* info, void* stream) {
    if (!ws || !counts || !info || (F && !faces) || (V && !verts)) { set_last_error("mesh_repair_count: null pointer"); return 2; }
    if ((size_t)counts & 7) { set_last_error("mesh_repair_count: counts must be 8-byte aligned"); return 2; }
    if (wedge != 0 && wedge != 1) { set_last_error("mesh_repair_count: wedge must be 0 (void) or 1 (solid)"); return 2; }
    if (int rc = et::check_sizes("mesh_repair_count", V, F)) return rc;
    const int k = et::resolve_log2("mesh_repair_count", F, table_log2);
    if (!k) return 2;
    const size_t slots = (size_t)1 << k;
    if (int rc = mr::check_workspace("mesh_repair_count", ws, ws_bytes, mr::carve(nullptr, V, F, slots).bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const mr::Workspace w = mr::carve(ws, V, F, slots);
    const unsigned n_he = 3u * F;
    const mr::View m = mr::view_of(w, faces, V, F, slots);
    NERFART_HIP(hipMemsetAsync(info, 0, 16 * sizeof(unsigned), st));
    NERFART_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(unsigned), st));
    NERFART_HIP(hipMemsetAsync(w.tot, 0, 8 * sizeof(unsigned), st));
    NERFART_HIP(hipMemsetAsync(w.ctab, 0xff, sizeof(unsigned) * (size_t)w.T, st));
    NERFART_HIP(hipMemsetAsync(w.chead, 0xff, sizeof(unsigned) * (size_t)w.T, st));
    NERFART_HIP(hipMemsetAsync(w.ccnt, 0, sizeof(unsigned) * 2 * (size_t)w.T, st));
    NERFART_HIP(hipMemsetAsync(w.cnext, 0xff, sizeof(unsigned) * w.nf, st));
    NERFART_HIP(hipMemsetAsync(w.cursor, 0, sizeof(unsigned) * w.nh, st));
    NERFART_HIP(hipMemsetAsync(w.sub, 0, sizeof(unsigned) * w.nh, st));
    NERFART_HIP(hipMemsetAsync(w.cls, 0xff, sizeof(unsigned) * w.nh, st));
    NERFART_HIP(hipMemsetAsync(w.vcount, 0, sizeof(unsigned) * w.nv, st));
    NERFART_HIP(hipMemsetAsync(w.vcursor, 0, sizeof(unsigned) * w.nv, st));
    hipLaunchKernelGGL(mr::k_mr_init, et::blocks256(slots > n_he ? slots : n_he), dim3(256), 0, st, w.table, slots, w.parent_c, w.unit_min, n_he);
    NERFART_HIP(hipGetLastError());
    if (F) {
        hipLaunchKernelGGL(mr::k_mr_cancel, et::blocks256(F), dim3(256), 0, st, faces, F, V, w.ctab, w.T, w.ccnt, w.chead, w.cnext, w.cslot, info);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mr::k_mr_alive, et::blocks256(F), dim3(256), 0, st, faces, F, V, w.T, (const unsigned*)w.ccnt, (const unsigned*)w.chead,
                           (const unsigned*)w.cnext, (const unsigned*)w.cslot, w.alive, info);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mr::k_mr_insert, et::blocks256(F), dim3(256), 0, st, faces, F, (const unsigned*)w.alive, w.table, slots - 1, w.slot_of, info);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mr::k_mr_resolve, et::blocks256(n_he), dim3(256), 0, st, m, w.parent_c, info);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mr::k_mr_scan_nm, pair_scan_blocks(n_he), dim3(256), 0, st, m, (uint2*)w.off_he, pair_scan_sums(w.lvl_he, 0, w.tot + mr::T_CSR));
        NERFART_HIP(hipGetLastError());
        if (int rc = pair_scan_finish(w.off_he, n_he, w.lvl_he, w.tot + mr::T_CSR, st)) return rc;
        hipLaunchKernelGGL(mr::k_mr_fill, et::blocks256(n_he), dim3(256), 0, st, m, (const uint2*)w.off_he, w.cursor, w.list);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mr::k_mr_pair, et::blocks256(n_he), dim3(256), 0, st, m, verts, wedge, (const uint2*)w.off_he, w.list, w.seq, w.rnk, w.stk,
                           w.ang, w.parent_c, w.unit_min, info);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mr::k_mr_roots, et::blocks256(n_he), dim3(256), 0, st, m, (const unsigned*)w.parent_c, w.vcount);
        NERFART_HIP(hipGetLastError());
    }
    if (V) {
        hipLaunchKernelGGL(mr::k_mr_scan_v, pair_scan_blocks(V), dim3(256), 0, st, (const unsigned*)w.vcount, V, (uint2*)w.off_v,
                           pair_scan_sums(w.lvl_v, 0, w.tot + mr::T_V1));
        NERFART_HIP(hipGetLastError());
        if (int rc = pair_scan_finish(w.off_v, V, w.lvl_v, w.tot + mr::T_V1, st)) return rc;
    }
    if (F && V) {
        hipLaunchKernelGGL(mr::k_mr_vfill, et::blocks256(n_he), dim3(256), 0, st, m, (const unsigned*)w.parent_c, (const unsigned*)w.vcount,
                           (const uint2*)w.off_v, w.vcursor, w.vlist);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mr::k_mr_vrank, et::blocks256(n_he), dim3(256), 0, st, m, (const unsigned*)w.parent_c, (const unsigned*)w.vcount,
                           (const uint2*)w.off_v, (const unsigned*)w.vlist, w.cls);
        NERFART_HIP(hipGetLastError());
        hipLaunchKernelGGL(mr::k_mr_multi, et::blocks256(n_he), dim3(256), 0, st, m, (const uint2*)w.off_he, (const unsigned*)w.list, w.rnk, w.stk,
                           (const unsigned*)w.parent_c, (const unsigned*)w.cls, (const unsigned*)w.unit_min, w.sub);
        NERFART_HIP(hipGetLastError());
    }
    if (F) {
        hipLaunchKernelGGL(mr::k_mr_scan_sub, pair_scan_blocks(n_he), dim3(256), 0, st, (const unsigned*)w.sub, n_he, (uint2*)w.off_he,
                           pair_scan_sums(w.lvl_he, 0, w.tot + mr::T_M));
        NERFART_HIP(hipGetLastError());
        if (int rc = pair_scan_finish(w.off_he, n_he, w.lvl_he, w.tot + mr::T_M, st)) return rc;
        hipLaunchKernelGGL(mr::k_mr_scan_f, pair_scan_blocks(F), dim3(256), 0, st, (const unsigned*)w.alive, (const unsigned*)w.unit_min,
                           (const unsigned*)w.sub, F, n_he, (uint2*)w.off_f, pair_scan_sums(w.lvl_f, 0, w.tot + mr::T_FA));
        NERFART_HIP(hipGetLastError());
        if (int rc = pair_scan_finish(w.off_f, F, w.lvl_f, w.tot + mr::T_FA, st)) return rc;
    }
    hipLaunchKernelGGL(mr::k_mr_totals, dim3(1), dim3(64), 0, st, (const unsigned*)w.tot, counts, info);
    NERFART_HIP(hipGetLastError());
    return 0;
}

int nerfart_mesh_repair_emit(const float* verts, const int* faces, unsigned V, unsigned F, int table_log2, const void* ws, size_t ws_bytes,
                             float* verts_out, int* faces_out, int* src_vertex, int* mid_ends, unsigned V_out, unsigned M_out, unsigned F_out,
                             void* stream) {
    if (!ws || (F && !faces) || (V && !verts) || (V_out && (!verts_out || !src_vertex)) || (M_out && !mid_ends) || (F_out && !faces_out)) {
        set_last_error("mesh_repair_emit: null pointer");
        return 2;
    }
    if (int rc = et::check_sizes("mesh_repair_emit", V, F)) return rc;
    const int k = et::resolve_log2("mesh_repair_emit", F, table_log2);
    if (!k) return 2;
    const size_t slots = (size_t)1 << k;
    if (int rc = mr::check_workspace("mesh_repair_emit", ws, ws_bytes, mr::carve(nullptr, V, F, slots).bytes)) return rc;
    // at most one class per corner and one midpoint per half-edge; a face with k subdivided half-edges becomes k + 1 <= 4 faces
    if (M_out > V_out || (size_t)V_out > 6 * (size_t)F || (size_t)F_out > 4 * (size_t)F) {
        set_last_error("mesh_repair_emit: V_out / M_out / F_out larger than any count of this mesh");
        return 2;
    }
    if (!F || !V || (!V_out && !F_out)) return 0;
    hipStream_t st = (hipStream_t)stream;
    const mr::Workspace w = mr::carve(const_cast<void*>(ws), V, F, slots);
    const mr::View m = mr::view_of(w, faces, V, F, slots);
    const unsigned n_he = 3u * F;
    if (V_out) {
        hipLaunchKernelGGL(mr::k_mr_emit_verts, et::blocks256(n_he), dim3(256), 0, st, m, verts, (const unsigned*)w.parent_c, (const unsigned*)w.cls,
                           (const unsigned*)w.sub, (const uint2*)w.off_he, (const unsigned*)w.tot, verts_out, src_vertex, mid_ends, V_out, M_out);
        NERFART_HIP(hipGetLastError());
    }
    if (F_out) {
        hipLaunchKernelGGL(mr::k_mr_emit_faces, et::blocks256(F), dim3(256), 0, st, m, (const unsigned*)w.alive, (const unsigned*)w.parent_c,
                           (const unsigned*)w.cls, (const unsigned*)w.unit_min, (const unsigned*)w.sub, (const uint2*)w.off_he, (const uint2*)w.off_f,
                           (const unsigned*)w.tot, faces_out, F_out);
        NERFART_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
