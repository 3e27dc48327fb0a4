// host_util.h - host-side plumbing shared by the render entry points (volsdf_render.hip, neus_render.hip, render_backward.hip):
// workspace carving, the dynamic-LDS attribute of the per-ray kernels, and the linspace tables a caller did not supply.
#pragma once
#include "nerfart_common.h"
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>

namespace nerfart {

// Cuts a caller-allocated workspace into buffers, each rounded up to 256 bytes, in the order of the take() calls.  A null base is the size
// query: every pointer comes back null and `off` ends as the bytes the same sequence of calls needs.
struct Carver {
    char* base; size_t off;
    explicit Carver(void* p) : base((char*)p), off(0) {}
    template <class T> T* take(size_t n) { T* r = base ? (T*)(base + off) : nullptr; off += (n * sizeof(T) + 255) & ~(size_t)255; return r; }
    void* bytes(size_t n) { return take<char>(n); }
};

inline int next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// Dynamic LDS of a one-wave-per-ray kernel: more than the CU's 160 KiB is refused with the caller's text before any HIP call.
inline int set_lds(const void* k, size_t bytes, const char* refusal) {
    if (bytes > 160 * 1024) { set_last_error(refusal); return 2; }
    NERFART_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

// torch.linspace(0, 1, n) (nerfart_linspace) into each listed device buffer: one host staging buffer, one copy per table and ONE stream
// synchronisation, after which the staging buffer is freed.  Only then is the first HIP error reported, named e1, e2, ... in call order.
struct LinspaceTable { float* dev; int n; };
inline int upload_linspace_tables(std::initializer_list<LinspaceTable> tables, hipStream_t stream) {
    size_t total = 0;
    for (const LinspaceTable& t : tables) total += (size_t)t.n;
    float* h = (float*)malloc(sizeof(float) * total);
    if (!h) { set_last_error("out of host memory"); return 3; }
    int rc = 0, calls = 0;
    auto note = [&](hipError_t e) {
        char what[16];
        snprintf(what, sizeof(what), "e%d", ++calls);
        if (!rc) rc = check_hip(e, what);
    };
    float* p = h;
    for (const LinspaceTable& t : tables) {
        nerfart_linspace(0.f, 1.f, t.n, p);
        note(hipMemcpyAsync(t.dev, p, sizeof(float) * t.n, hipMemcpyHostToDevice, stream));
        p += t.n;
    }
    note(hipStreamSynchronize(stream));
    free(h);
    return rc;
}

}  // namespace nerfart
