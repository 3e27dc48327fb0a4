// edge_table.h - the undirected-edge table csrc/mesh_topology.hip (half-edge adjacency, manifold checks) and csrc/mesh_repair.hip (cut and stitch
// of non-manifold edges) share, with the size checks both entry-point families make before any launch.
//
// Open addressing, linear probing, C = 2^table_log2 slots of 24 bytes {key, cnt[2], minh[2]}.  key = (a << 32) | b of the undirected edge a < b,
// claimed with one 64-bit atomicCAS on an empty slot (all ones: never a key, a < 2^31); cnt[d] counts the half-edges running a -> b (d = 0) and
// b -> a (d = 1) with atomicAdd; minh[d] is the smallest half-edge id of direction d with atomicMin.  A probe sequence visits at most C slots,
// then gives up (the caller sets its overflow flag): it cannot spin, whatever the faces hold - the host refuses a table of fewer than 3 F + 1
// slots, so with the table initialised by the same call an empty slot is always met first.  Counts and smallest ids are sums and minima: what a
// slot ends up holding does not depend on the order of work, and nothing a caller derives from it depends on where the key landed.
#pragma once
#include "host_util.h"
#include <string>

namespace nerfart {
namespace et {

struct Slot {
    unsigned long long key;
    unsigned cnt[2];
    unsigned minh[2];
};
static_assert(sizeof(Slot) == 24, "the header states 24 bytes per slot");

constexpr unsigned long long EMPTY = ~0ull;
constexpr unsigned NOSLOT = 0xFFFFFFFFu;       // slot_of: the half-edge of a face that takes no part (or of an overflowed insert)
constexpr unsigned NONE = 0xFFFFFFFFu;         // minh: no half-edge of that direction (ids stay below 3 F < 2^31)
constexpr int MAX_LOG2 = 31;                  // slot indices are kept as u32 in slot_of, and NOSLOT must not be one of them
static_assert(MAX_LOG2 <= 31, "slot_of [3 F] holds a slot index in 32 bits, 0xFFFFFFFF set aside");

// fmix64 of MurmurHash3: where a key lands decides the speed only
__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

// every lane of the wave calls this (no early return before it: the ballot is wave-wide and lane 0 does the add)
__device__ __forceinline__ void tally(bool flag, unsigned* addr) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(addr, (unsigned)__popcll(m));
}

__device__ __forceinline__ unsigned next_in_face(unsigned he) { return he % 3u == 2u ? he - 2u : he + 1u; }

__device__ __forceinline__ void init_slot(Slot* table, size_t i) {
    Slot s;
    s.key = EMPTY; s.cnt[0] = s.cnt[1] = 0u; s.minh[0] = s.minh[1] = NONE;
    table[i] = s;
}

// Half-edge `he` running x -> y (x != y, both below 2^31) enters the table: its slot, or NOSLOT when the probe sequence found no room.
__device__ __forceinline__ unsigned insert(Slot* table, size_t mask, unsigned x, unsigned y, unsigned he) {
    const int dir = x > y;
    const unsigned long long key = dir ? ((unsigned long long)y << 32) | x : ((unsigned long long)x << 32) | y;
    size_t h = (size_t)mix64(key) & mask;
    // BOUND: at most `mask + 1` = C steps, whatever the table holds.  No step waits for another thread: a CAS that loses has read the winner's
    // key and goes on.
    for (size_t step = 0; step <= mask; ++step) {
        unsigned long long cur = __hip_atomic_load(&table[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == EMPTY) {
            cur = atomicCAS(&table[h].key, EMPTY, key);
            if (cur == EMPTY) cur = key;
        }
        if (cur == key) {
            atomicAdd(&table[h].cnt[dir], 1u);
            atomicMin(&table[h].minh[dir], he);
            return (unsigned)h;
        }
        h = (h + 1) & mask;
    }
    return NOSLOT;
}

// ---- host: the refusals both families share ----------------------------------------------------------------------------------------------------

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

static int smallest_log2(unsigned F) {                       // the smallest k >= 1 with 2^k >= 3 F + 1; above MAX_LOG2 when there is none
    const unsigned long long need = 3ull * F + 1;
    int k = 1;
    while (k <= MAX_LOG2 && (1ull << k) < need) ++k;
    return k;
}

// the table's log2 for the caller's table_log2 (0 = default: the smallest power of two >= 4 (3 F + 1), at most 2^31); 0 = refused, last_error set
static int resolve_log2(const char* who, unsigned F, int table_log2) {
    char msg[240];
    const int least = smallest_log2(F);
    int k = table_log2;
    if (k == 0) k = least + 2 > MAX_LOG2 ? MAX_LOG2 : least + 2;
    if (k < 1 || k > MAX_LOG2) {
        snprintf(msg, sizeof(msg), "%s: table_log2 must be 0 (default) or in 1 .. %d (got %d)", who, MAX_LOG2, table_log2);
        set_last_error(msg);
        return 0;
    }
    if (k < least) {
        snprintf(msg, sizeof(msg), "%s: a table of 2^%d slots holds fewer than 3 F + 1 = %llu slots (F = %u; the largest table is 2^%d)", who, k,
                 3ull * F + 1, F, MAX_LOG2);
        set_last_error(msg);
        return 0;
    }
    return k;
}

static dim3 blocks256(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace et
}  // namespace nerfart
