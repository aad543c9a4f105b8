// fdcm_unionfind.h -- lock-free union-find on one int32 parent per pixel (device code), shared by the edge components
// (fdcm_image.hip) and the line components (fdcm_lines.hip).  SCOPE is the memory scope of the reads: the agent for parents in
// global memory that other workgroups link meanwhile (the default), the workgroup for a tile's parents in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fdcm {

static constexpr int kNoParent = -1;  // parent of a pixel that is in no component

// Union-find on `parent` (a candidate's parent is a candidate of its component with a smaller or the same index; a root is its
// own).  Other workgroups link roots meanwhile, so every read is an atomic load: a stale parent is still an ancestor.
template <int SCOPE = __HIP_MEMORY_SCOPE_AGENT>
__device__ __forceinline__ int uf_load(const int32_t* parent, int p) { return __hip_atomic_load(parent + p, __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE = __HIP_MEMORY_SCOPE_AGENT>
__device__ __forceinline__ int uf_find(const int32_t* parent, int p) {
    for (int q = uf_load<SCOPE>(parent, p); q != p; q = uf_load<SCOPE>(parent, p)) p = q;
    return p;
}
// Links the larger root under the smaller.  When the larger one stopped being a root meanwhile, atomicMin has either changed
// nothing or replaced its parent, which is then merged in its turn: no link is lost, and every step lowers a parent.
template <int SCOPE = __HIP_MEMORY_SCOPE_AGENT>
__device__ __forceinline__ void uf_union(int32_t* parent, int a, int b) {
    for (;;) {
        a = uf_find<SCOPE>(parent, a); b = uf_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }  // a > b
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

}  // namespace fdcm
