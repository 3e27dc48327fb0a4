// union_find.h - the lock-free union-find csrc/mesh_components.hip (vertices of a component) and csrc/mesh_topology.hip (corners of a fan, vertices
// of a boundary loop) share.  parent [n] uint32 starts as parent[x] = x; unite links the LARGER root under the SMALLER with one
// atomicCAS(&parent[hi], hi, lo).  INVARIANT parent[x] <= x, at every moment: the smallest index of a class can never be linked under anything and
// is the one root left - the result is canonical, whatever the order of work - and every loop has a bound that follows from the data alone
// (written next to the loops).  No thread waits for another.
#pragma once
#include "nerfart_common.h"

namespace nerfart {
namespace uf {

// parent is read while other workgroups link under it: relaxed, agent scope - the value comes from the memory all of them write.
__device__ __forceinline__ unsigned load_parent(const unsigned* parent, unsigned v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of v's tree as this thread sees it.  BOUND: parent[x] <= x for every x at every moment - the initialisation writes x, the only other
// writes are the CAS of unite (lo < hi into parent[hi]) and a flattening store of a root that find reached from x, hence <= x - so every step that
// does not end the loop goes to a strictly smaller index: at most v steps.  A stale value is an older parent, still an ancestor and still <= x.
__device__ __forceinline__ unsigned find(const unsigned* parent, unsigned v) {
    for (;;) {
        const unsigned p = load_parent(parent, v);
        if (p >= v) return v;                      // p == v: a root (p > v cannot be; it would end the loop all the same)
        v = p;
    }
}

// Joins the trees of a and b.  The CAS links hi under lo only while hi is still a root, so a tree is never cut.  BOUND: when the CAS fails it
// returns the parent another thread gave hi, old < hi (the invariant; it is not hi, or the CAS had succeeded); the retry goes on from (old, lo),
// whose roots are <= old and <= lo, both < hi: max(hi, lo) strictly decreases on every retry - at most max(a, b) retries.
__device__ __forceinline__ void unite(unsigned* parent, unsigned a, unsigned b) {
    for (;;) {
        a = find(parent, a);
        b = find(parent, b);
        if (a == b) return;
        const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
        const unsigned old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

}  // namespace uf
}  // namespace nerfart
