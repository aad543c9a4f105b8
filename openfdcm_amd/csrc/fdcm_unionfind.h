// fdcm_unionfind.h -- lock-free union-find on one int32 parent per pixel (device code), and on top of it the labeller of
// 8-connected pixels of equal key that the edge components (fdcm_image.hip) and the line components (fdcm_lines.hip) share: a
// 64 x 16 tile merged in LDS (uf_tile_merge), then the pairs that straddle two tiles linked in global memory
// (uf_border_merge).  SCOPE is the memory scope of the reads: the agent for parents in global memory that other workgroups link
// meanwhile (the default), the workgroup for a tile's parents in LDS.
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

// ------------------------------------------------------------------------------------------ components of a label image
// A key policy K says which pixels hang together: K::P partitions (1 or 2) of the same pixels, and key(partition, label byte),
// a byte, kNoKey for a pixel that is in no component of that partition (label 255 in every partition).  Neighbours of equal key
// belong to one component.  The parents of partition i are parent + i * n (n = W * H), global pixel indices (< 2^24).
static constexpr int kTileW = 64, kTileH = 16, kTilePixels = kTileW * kTileH;  // pixels a workgroup merges in LDS
static constexpr int kNoKey = 255;
static constexpr int kBorderThreads = 128;  // uf_border_merge's workgroup: kTileW + 2 * kTileH of them work

// Workgroup (bx, by) of 256 threads merges its tile in LDS: uf_union at workgroup scope on tile-local indices (row-major in the
// tile, so their order is that of the global indices of the same pixels).  Per pixel and partition the tile's root goes out as
// a global index, kNoParent where the key is kNoKey: every pixel of the image gets a parent, so `parent` needs no clearing.
template <class K>
__device__ __forceinline__ void uf_tile_merge(const K keys, const uint8_t* __restrict__ labels, int W, int H, int32_t* __restrict__ parent) {
    constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
    __shared__ unsigned char sk[K::P][kTilePixels];
    __shared__ int lp[K::P][kTilePixels];
    const int tid = threadIdx.x, lx = tid & 63;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
#pragma unroll
    for (int i = 0; i < kTileH / 4; ++i) {
        const int ly = (tid >> 6) + 4 * i, li = ly * kTileW + lx;
        const int x = x0 + lx, y = y0 + ly;
        const int l = x < W && y < H ? labels[(size_t)y * W + x] : 255;
#pragma unroll
        for (int part = 0; part < K::P; ++part) {
            const int k = keys.key(part, l);
            sk[part][li] = (unsigned char)k;
            lp[part][li] = k != kNoKey ? li : kNoParent;
        }
    }
    __syncthreads();
    // a pixel with the pixels of its key among its west, north-west, north and north-east neighbours inside the tile
#pragma unroll
    for (int i = 0; i < kTileH / 4; ++i) {
        const int ly = (tid >> 6) + 4 * i, li = ly * kTileW + lx;
#pragma unroll
        for (int part = 0; part < K::P; ++part) {
            const int k = sk[part][li];
            if (k == kNoKey) continue;
            if (lx > 0 && sk[part][li - 1] == k) uf_union<kScope>(lp[part], li, li - 1);
            if (ly > 0) {
                if (lx > 0 && sk[part][li - kTileW - 1] == k) uf_union<kScope>(lp[part], li, li - kTileW - 1);
                if (sk[part][li - kTileW] == k) uf_union<kScope>(lp[part], li, li - kTileW);
                if (lx + 1 < kTileW && sk[part][li - kTileW + 1] == k) uf_union<kScope>(lp[part], li, li - kTileW + 1);
            }
        }
    }
    __syncthreads();
    const int n = W * H;
#pragma unroll
    for (int i = 0; i < kTileH / 4; ++i) {
        const int ly = (tid >> 6) + 4 * i, li = ly * kTileW + lx;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int p = y * W + x;
#pragma unroll
        for (int part = 0; part < K::P; ++part) {
            int r = kNoParent;
            if (sk[part][li] != kNoKey) {
                const int t = uf_find<kScope>(lp[part], li);
                r = (y0 + (t >> 6)) * W + x0 + (t & 63);
            }
            parent[part * n + p] = r;
        }
    }
}

// pixel p with its neighbour q = (xq, yq) of the row above or the column before, in another tile: merged per partition where
// the keys agree (kp: p's keys)
template <class K>
__device__ __forceinline__ void uf_border_link(const K& keys, const uint8_t* __restrict__ labels, int W, int n, int p, const int* kp, int xq, int yq,
                                               int32_t* parent) {
    const int q = yq * W + xq;
    const int l = labels[q];
#pragma unroll
    for (int part = 0; part < K::P; ++part)
        if (kp[part] != kNoKey && keys.key(part, l) == kp[part]) uf_union(parent + part * n, p, q);
}
// Workgroup (bx, by) of kBorderThreads threads, one per pixel of its tile's top row (north-west, north, north-east; west at the
// corner), its left column (west, north-west) and its right column (north-east) below the top row: every 8-neighbour pair
// across a tile border once, merged in global memory.
template <class K>
__device__ __forceinline__ void uf_border_merge(const K keys, const uint8_t* __restrict__ labels, int W, int H, int32_t* parent) {
    const int t = threadIdx.x;
    if (t >= kTileW + 2 * kTileH) return;
    int lx, ly;
    if (t < kTileW) { lx = t; ly = 0; }
    else if (t < kTileW + kTileH) { lx = 0; ly = t - kTileW; }
    else { lx = kTileW - 1; ly = t - kTileW - kTileH; }
    if (t >= kTileW && ly == 0) return;  // the corners belong to the top row
    const int x = blockIdx.x * kTileW + lx, y = blockIdx.y * kTileH + ly;
    if (x >= W || y >= H) return;
    const int n = W * H, p = y * W + x;
    const int l = labels[p];
    int kp[K::P];
    bool any = false;
#pragma unroll
    for (int part = 0; part < K::P; ++part) { kp[part] = keys.key(part, l); any |= kp[part] != kNoKey; }
    if (!any) return;
    const bool west = lx == 0 && x > 0, north = ly == 0 && y > 0, east = x + 1 < W;
    if (t < kTileW) {
        if (west) uf_border_link(keys, labels, W, n, p, kp, x - 1, y, parent);
        if (north) {
            if (x > 0) uf_border_link(keys, labels, W, n, p, kp, x - 1, y - 1, parent);
            uf_border_link(keys, labels, W, n, p, kp, x, y - 1, parent);
            if (east) uf_border_link(keys, labels, W, n, p, kp, x + 1, y - 1, parent);
        }
    } else if (t < kTileW + kTileH) {
        if (west) {
            uf_border_link(keys, labels, W, n, p, kp, x - 1, y, parent);
            uf_border_link(keys, labels, W, n, p, kp, x - 1, y - 1, parent);  // (ly >= 1: the row above is the image's)
        }
    } else if (east) {
        uf_border_link(keys, labels, W, n, p, kp, x + 1, y - 1, parent);
    }
}
// the grid of both: a workgroup per tile
inline dim3 uf_tile_grid(int W, int H) { return dim3((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH)); }

}  // namespace fdcm
