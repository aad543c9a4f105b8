// fdcm_mesh.hip -- line templates from a triangle mesh on gfx950 (include/fdcm.h, "Templates from a mesh"): per view the visible
// sharp edges and occluding contours, as float line segments.
//
//   mesh_create        host: the edge table (sorted vertex pairs, their one or two faces) and the sharp flags in float64
//   k_mesh_boxes       a thread per (view, vertex): the view's pixel box by wave reductions and four integer atomics per wave
//   k_mesh_raster      16 lanes per (view, face): the face's box in 4 x 4 pixel tiles, one 64-bit atomicMax per covered
//                      centre; a face of more than kSmallTiles tiles goes onto the part's list instead
//   k_mesh_raster_big  the list: a workgroup per (entry, slice), 16 x 16 pixel tiles, so that one face of 2000 pixels is
//                      spread over kBigSlices workgroups
//   k_mesh_edges<0>    a lane per (view, edge): candidate test, the walk along the samples, the lines counted; per 256 edges a sum
//   k_mesh_scan        exclusive scan of the sums in place (one workgroup), the total behind them
//   k_mesh_edges<1>    the same walk, the lines written at their positions, in runs of views whose lines fit 256 MB
// Exact visibility (include/fdcm.h, "exact visibility and joined lines") builds no item buffer: the faces go into lists per
// 8 x 8 pixel tile of the view's box, and the walk tests a sample against the faces of its tile.
//   k_mesh_tiles<0>    a lane per (view, face), all views: the tiles of the face's box, summed per view (the host cuts the
//                      parts from these totals)
//   k_mesh_tiles<1>    the part's views: one atomic add per (face, tile), the tiles' counts
//   k_mesh_tile_starts per 256 tiles: the counts' exclusive prefix inside the block and the block's sum; k_mesh_scan follows
//   k_mesh_tiles<2>    the same loop, the face stored at the tile's atomic cursor (the order inside a tile is free: an OR)
//   k_mesh_edges<., 1> the walk with the rule of the definition in place of the item buffer's
// Joined lines: k_mesh_edges writes the runs before the length test, with (edge, end flags, view) beside them, and then
//   k_mesh_links       a lane per (line, end): an end at a vertex counts at (view, vertex) and takes one of its two slots
//   k_mesh_chains<0>   a lane per line: does it start a chain (walk to the other free end, or once round), and if so the chain
//                      simplified, its lines counted; per 256 lines a sum; k_mesh_scan follows
//   k_mesh_starts      a lane per view: where its lines begin among the run's (the host reads these alone)
//   k_mesh_chains<1>   the same walk, the lines written
// Nothing stores a projection: every kernel projects the vertices it reads with mesh_project, the one statement of the view, so
// the passes agree to the bit and a part of the views costs its item buffers, counts and list alone.  The projection is a type
// parameter of those kernels: MeshOrtho, or MeshPinhole ("Templates from a mesh: pinhole views"), whose depth coordinate is
// Z = 1 / depth, so that nothing but the projection and the depth-tolerance compare differs between the two.
// Bounds: a face's box lies in its view's box (both are floors of the same projected values), and every access of the item
// buffer tests the pixel against the view's box all the same; a list entry is below the part's views times F, the list's size;
// counts and sums are indexed by (view, block) below the grid's size; a line's position is below the total the host read back.
// A tile index is clamped into its view's tiles, a face list position is tested against the list's size; a link table entry
// is indexed by (view of the run, vertex), a link slot holds a line of the same run, and every chain walk stops after as many
// steps as the run has lines.
#include <algorithm>
#include <cmath>
#include <memory>

#include "fdcm_internal.h"

namespace fdcm {

static constexpr int kSmallTiles = 64;     // 4 x 4 tiles a 16-lane group walks itself (a box of 32 x 32 pixels, or 256 x 4)
static constexpr int kBigSlices = 16;      // workgroups a listed face is spread over
static constexpr int kBigGrid = 2048;      // workgroups of k_mesh_raster_big, which strides over (entry, slice)
static constexpr size_t kMeshPartBytes = (size_t)512 << 20;  // item buffers, list and counts of a part of the views
static constexpr size_t kMeshWriteBytes = (size_t)256 << 20; // lines of one writing pass (a view's own lines whatever they take)
static constexpr int kMeshMaxSpan = 4096;
static constexpr float kMeshMaxCoord = 1073741824.f;  // 2^30

struct MeshView { int32_t x0, y0, w, h; long long off; };  // the view's box and where its item buffer begins in the part's (keys)
struct MeshPoint { float X, Y, Z; };

// The projection is a type parameter of every kernel that projects: the orthographic one is the block "Templates from a mesh",
// the pinhole one "Templates from a mesh: pinhole views".  A projection travels in a kernel's arguments where `scale` did (so
// MeshOrtho's argument blocks are the ones a float gave); `at` is what one view adds to its matrix R, `from` the projection of
// a part or a run that begins at view v0, and the depth-tolerance compares are the projection's too: `limit` once per sample, then
// `visible` (the item buffer's rule: false for a NaN) or `hidden` (the exact rule: false for a NaN).
struct MeshOrtho {
    float scale;
    struct View { float scale; };
    __device__ __forceinline__ View at(int) const { return View{scale}; }
    __device__ __forceinline__ bool admits(const float* __restrict__, const View&, const float* __restrict__) const { return true; }
    MeshOrtho from(int64_t) const { return *this; }
    static __device__ __forceinline__ float limit(float tol, float sz) { return sz + tol; }
    static __device__ __forceinline__ bool visible(float limit, float, float zf) { return limit >= zf; }
    static __device__ __forceinline__ bool hidden(float limit, float, float zf) { return zf > limit; }
};
struct MeshPinhole {
    float focal, near;
    const float* positions;  // 3 per view, beside the views
    struct View { float tx, ty, tz, focal, ox, oy; };
    __device__ __forceinline__ View at(int view) const {
        const float* t = positions + 3 * (size_t)view;
        View w{t[0], t[1], t[2], focal, 0.f, 0.f};
        const float zo = 1.0f / (-w.tz);
        w.ox = (focal * w.tx) * zo;
        w.oy = (focal * w.ty) * zo;
        return w;
    }
    // the vertex is at depth d >= near (false for a NaN): the one test k_mesh_boxes adds, every other pass sees admitted views only
    __device__ __forceinline__ bool admits(const float* __restrict__ R, const View& w, const float* __restrict__ v) const {
        const float d = -(((R[6] * v[0] + R[7] * v[1]) + R[8] * v[2]) + w.tz);
        return d >= near;
    }
    MeshPinhole from(int64_t v0) const { return MeshPinhole{focal, near, positions + 3 * (size_t)v0}; }
    static __device__ __forceinline__ float limit(float tol, float sz) { return tol * sz; }
    static __device__ __forceinline__ bool visible(float limit, float sz, float zf) { return limit * zf >= zf - sz; }
    static __device__ __forceinline__ bool hidden(float limit, float sz, float zf) { return zf - sz > limit * zf; }
};

__device__ __forceinline__ MeshPoint mesh_project(const float* __restrict__ R, const MeshOrtho::View& w, const float* __restrict__ v) {
    const float x = v[0], y = v[1], z = v[2];
    MeshPoint p;
    p.X = w.scale * ((R[0] * x + R[1] * y) + R[2] * z);
    p.Y = w.scale * ((R[3] * x + R[4] * y) + R[5] * z);
    p.Z = (R[6] * x + R[7] * y) + R[8] * z;
    return p;
}
// Z = 1 / depth: larger is nearer, as above, and linear in X and Y across a face and along an edge
__device__ __forceinline__ MeshPoint mesh_project(const float* __restrict__ R, const MeshPinhole::View& w, const float* __restrict__ v) {
    const float x = v[0], y = v[1], z = v[2];
    const float px = ((R[0] * x + R[1] * y) + R[2] * z) + w.tx;
    const float py = ((R[3] * x + R[4] * y) + R[5] * z) + w.ty;
    const float pz = ((R[6] * x + R[7] * y) + R[8] * z) + w.tz;
    MeshPoint p;
    p.Z = 1.0f / (-pz);
    p.X = (w.focal * px) * p.Z - w.ox;
    p.Y = (w.focal * py) * p.Z - w.oy;
    return p;
}
__device__ __forceinline__ float mesh_orient(float ax, float ay, float bx, float by, float cx, float cy) {
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}
__device__ __forceinline__ unsigned mesh_ord(float z) {
    const unsigned u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// A projected face: whether it covers the point (x, y) and its depth there.
struct MeshFace {
    MeshPoint A, B, C;
    float a;
    __device__ __forceinline__ bool solid() const { return a > 0.f || a < 0.f; }  // (neither for a NaN)
    __device__ __forceinline__ bool depth(float x, float y, float& z) const {
        const float e0 = mesh_orient(B.X, B.Y, C.X, C.Y, x, y), e1 = mesh_orient(C.X, C.Y, A.X, A.Y, x, y),
                    e2 = mesh_orient(A.X, A.Y, B.X, B.Y, x, y);
        z = ((e0 * A.Z + e1 * B.Z) + e2 * C.Z) / a;
        return a > 0.f ? (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) : (a < 0.f && e0 <= 0.f && e1 <= 0.f && e2 <= 0.f);
    }
};
template <class View>
__device__ __forceinline__ MeshFace mesh_face(const float* __restrict__ R, const View& w, const float* __restrict__ verts,
                                              const int32_t* __restrict__ faces, int f) {
    MeshFace t;
    t.A = mesh_project(R, w, verts + 3 * (size_t)faces[3 * (size_t)f]);
    t.B = mesh_project(R, w, verts + 3 * (size_t)faces[3 * (size_t)f + 1]);
    t.C = mesh_project(R, w, verts + 3 * (size_t)faces[3 * (size_t)f + 2]);
    t.a = mesh_orient(t.A.X, t.A.Y, t.B.X, t.B.Y, t.C.X, t.C.Y);
    return t;
}
struct MeshBox { int i0, j0, i1, j1; };
__device__ __forceinline__ MeshBox mesh_face_box(const MeshFace& t) {  // (the views that reach a raster pass have |X|, |Y| < 2^30)
    MeshBox b;
    b.i0 = (int)floorf(fminf(fminf(t.A.X, t.B.X), t.C.X)); b.i1 = (int)floorf(fmaxf(fmaxf(t.A.X, t.B.X), t.C.X));
    b.j0 = (int)floorf(fminf(fminf(t.A.Y, t.B.Y), t.C.Y)); b.j1 = (int)floorf(fmaxf(fmaxf(t.A.Y, t.B.Y), t.C.Y));
    return b;
}
// the face's key into pixel (i, j) of the view's item buffer, where it covers the centre
__device__ __forceinline__ void mesh_shade(const MeshFace& t, int f, const MeshView& d, unsigned long long* __restrict__ items, int i, int j) {
    const unsigned ui = (unsigned)(i - d.x0), uj = (unsigned)(j - d.y0);
    if (ui >= (unsigned)d.w || uj >= (unsigned)d.h) return;
    float z;
    if (!t.depth((float)i + 0.5f, (float)j + 0.5f, z) || z != z) return;
    atomicMax(items + d.off + (long long)uj * d.w + ui, ((unsigned long long)mesh_ord(z) << 32) | (unsigned)f);
}

// ------------------------------------------------------------------------------------------ projection pass
// boxes: 4 ints per view, x0 y0 x1 y1, from (INT_MAX, INT_MAX, INT_MIN, INT_MIN).  A coordinate that is not below 2^30 in
// magnitude (a NaN too) makes the box span everything, which the host refuses like any box above 4096; so does a vertex the
// projection does not admit (the pinhole's: one nearer than `near`).
template <class Proj>
__global__ void __launch_bounds__(256) k_mesh_boxes(const float* __restrict__ verts, int V, int nbV, const float* __restrict__ views,
                                                    Proj pj, int32_t* boxes) {
    const int view = blockIdx.x / nbV, v = (blockIdx.x % nbV) * 256 + threadIdx.x;
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
    if (v < V) {
        const float* R = views + 9 * (size_t)view;
        const typename Proj::View w = pj.at(view);
        const MeshPoint p = mesh_project(R, w, verts + 3 * (size_t)v);
        if (pj.admits(R, w, verts + 3 * (size_t)v) && fabsf(p.X) < kMeshMaxCoord && fabsf(p.Y) < kMeshMaxCoord) {
            x0 = x1 = (int)floorf(p.X);
            y0 = y1 = (int)floorf(p.Y);
        } else {
            x0 = y0 = INT32_MIN; x1 = y1 = INT32_MAX;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        x0 = min(x0, __shfl_xor(x0, d)); y0 = min(y0, __shfl_xor(y0, d));
        x1 = max(x1, __shfl_xor(x1, d)); y1 = max(y1, __shfl_xor(y1, d));
    }
    if ((threadIdx.x & 63) == 0 && x0 <= x1) {  // (a wave past V holds no vertex)
        int32_t* b = boxes + 4 * (size_t)view;
        atomicMin(b, x0); atomicMin(b + 1, y0); atomicMax(b + 2, x1); atomicMax(b + 3, y1);
    }
}

// ------------------------------------------------------------------------------------------ raster pass
// views, descs: the part's.  list: its count in the first 8 bytes, then (view in the part, face) pairs.
template <class Proj>
__global__ void __launch_bounds__(256) k_mesh_raster(const float* __restrict__ verts, const int32_t* __restrict__ faces, int F, int nbF,
                                                     const float* __restrict__ views, Proj pj, const MeshView* __restrict__ descs,
                                                     unsigned long long* __restrict__ items, unsigned long long* list) {
    const int view = blockIdx.x / nbF, f = (blockIdx.x % nbF) * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
    if (f >= F) return;
    const MeshFace t = mesh_face(views + 9 * (size_t)view, pj.at(view), verts, faces, f);
    if (!t.solid()) return;
    const MeshBox b = mesh_face_box(t);
    const int tx = ((b.i1 - b.i0) >> 2) + 1, ty = ((b.j1 - b.j0) >> 2) + 1;  // (a view's box spans 4096 at most: 1024 x 1024 tiles)
    const int tiles = tx * ty;
    if (tiles > kSmallTiles) {
        if (l == 0) {
            const unsigned long long at = atomicAdd(list, 1ull);
            reinterpret_cast<int2*>(list + 1)[at] = make_int2(view, f);
        }
        return;
    }
    const MeshView d = descs[view];
    for (int k = 0; k < tiles; ++k) {
        const int i = b.i0 + (k % tx) * 4 + (l & 3), j = b.j0 + (k / tx) * 4 + (l >> 2);
        if (i <= b.i1 && j <= b.j1) mesh_shade(t, f, d, items, i, j);
    }
}
template <class Proj>
__global__ void __launch_bounds__(256) k_mesh_raster_big(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                         const float* __restrict__ views, Proj pj, const MeshView* __restrict__ descs,
                                                         unsigned long long* __restrict__ items, const unsigned long long* __restrict__ list) {
    const long long units = (long long)list[0] * kBigSlices;
    const int2* entries = reinterpret_cast<const int2*>(list + 1);
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int2 en = entries[u / kBigSlices];
        const MeshFace t = mesh_face(views + 9 * (size_t)en.x, pj.at(en.x), verts, faces, en.y);
        const MeshBox b = mesh_face_box(t);
        const MeshView d = descs[en.x];
        const int tx = ((b.i1 - b.i0) >> 4) + 1, ty = ((b.j1 - b.j0) >> 4) + 1;
        for (int k = (int)(u % kBigSlices); k < tx * ty; k += kBigSlices) {
            const int i = b.i0 + (k % tx) * 16 + (threadIdx.x & 15), j = b.j0 + (k / tx) * 16 + (threadIdx.x >> 4);
            if (i <= b.i1 && j <= b.j1) mesh_shade(t, en.y, d, items, i, j);
        }
    }
}

// exclusive prefix of v over the 256 threads of a workgroup and their total (`sw`: 4 words of LDS; a barrier inside)
__device__ __forceinline__ int mesh_block_scan(int v, int tid, int* sw, int& total);

// ------------------------------------------------------------------------------------------ tile pass (exact visibility)
// The part's tiles, view after view (MeshView::off is the view's first tile, a view has tiles_across(w) a row): per tile the
// number of its faces, their exclusive prefix inside the tile's block of 256 and the fill pass's cursor; per block the prefix
// of the blocks' sums (k_mesh_scan); the faces of tile t are pairs[sums[t >> 8] + start[t] ..) count[t] of them.
struct MeshTiles {
    int *count, *cursor, *start;
    long long* sums;
    int* pairs;
    long long n_pairs;   // the list's size: the host's sum of the views' totals
};
__device__ __host__ __forceinline__ int mesh_tiles_across(int w) { return (w + 7) >> 3; }
// PASS 0: boxes and totals of all views, nothing else is read.  PASS 1, 2: views, boxes and descs are the part's.
// Bounds: a tile index is clamped into the view's own tiles, so it is below the part's number of tiles; a list position is
// tested against n_pairs (it is below it: the fill pass repeats the count pass's loop).
template <int PASS, class Proj>
__global__ void __launch_bounds__(256) k_mesh_tiles(const float* __restrict__ verts, const int32_t* __restrict__ faces, int F, int nbF,
                                                    const float* __restrict__ views, Proj pj, const int32_t* __restrict__ boxes,
                                                    const MeshView* __restrict__ descs, MeshTiles T, unsigned long long* totals) {
    const int view = blockIdx.x / nbF, f = (blockIdx.x % nbF) * 256 + threadIdx.x;
    long long mine = 0;
    if (f < F) {
        const MeshFace t = mesh_face(views + 9 * (size_t)view, pj.at(view), verts, faces, f);
        const int32_t* vb = boxes + 4 * (size_t)view;
        const int w = vb[2] - vb[0] + 1, h = vb[3] - vb[1] + 1;
        if (t.solid()) {
            const MeshBox b = mesh_face_box(t);
            const int ti0 = max(b.i0 - vb[0], 0) >> 3, ti1 = min(b.i1 - vb[0], w - 1) >> 3;
            const int tj0 = max(b.j0 - vb[1], 0) >> 3, tj1 = min(b.j1 - vb[1], h - 1) >> 3;
            if (ti0 <= ti1 && tj0 <= tj1) {
                if (PASS == 0) {
                    mine = (long long)(ti1 - ti0 + 1) * (tj1 - tj0 + 1);
                } else {
                    const int tw = mesh_tiles_across(w);
                    const long long base = descs[view].off;
                    for (int tj = tj0; tj <= tj1; ++tj)
                        for (int ti = ti0; ti <= ti1; ++ti) {
                            const long long tile = base + (long long)tj * tw + ti;
                            if (PASS == 1) {
                                atomicAdd(T.count + tile, 1);
                            } else {
                                const long long at = T.sums[tile >> 8] + T.start[tile] + atomicAdd(T.cursor + tile, 1);
                                if (at < T.n_pairs) T.pairs[at] = f;
                            }
                        }
                }
            }
        }
    }
    if (PASS == 0) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(totals + view, (unsigned long long)mine);
    }
}
__global__ void __launch_bounds__(256) k_mesh_tile_starts(MeshTiles T, long long n_tiles) {
    __shared__ int sw[4];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    int total;
    const int ex = mesh_block_scan(t < n_tiles ? T.count[t] : 0, threadIdx.x, sw, total);
    if (t < n_tiles) T.start[t] = ex;
    if (threadIdx.x == 0) T.sums[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------ edge pass
__device__ __forceinline__ int mesh_block_scan(int v, int tid, int* sw, int& total) {
    const int lane = tid & 63, wave = tid >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) sw[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = sw[k];
        if (k < wave) before += s;
        total += s;
    }
    return before + incl - v;
}
template <class Proj>
struct MeshEdgeArgs {
    const float* verts;
    const int32_t* faces;
    const int4* edges;      // i, j, f0, f1 (-1: none)
    const uint8_t* sharp;
    int E, nbE;
    const float* views;     // the part's
    Proj proj;
    float depth_tol, min_length;
    const MeshView* descs;
    const unsigned long long* items;
    int* counts;            // per (view, block, thread)
    long long* sums;        // per (view, block); scanned before the writing pass
    float4* out;            // the writing pass: the lines of the blocks from block0 on, the first of them at out[0]
    int block0;
    long long out0;         // sums[block0]
    MeshTiles tiles;        // exact visibility: in place of items
    int join;               // the lines before the length test, and with them
    int2* meta;             // (edge << 2 | k0 == 0 | (k1 == n) << 1, the view's index in the writing run), beside out
};
// Exact visibility: whether some face of the sample's tile hides sample k of n of edge ed at (sx, sy, sz)
template <class Proj>
__device__ __forceinline__ bool mesh_hidden(const MeshEdgeArgs<Proj>& g, const float* __restrict__ R, const typename Proj::View& w,
                                            const MeshView& d, const int4& ed, int k, int n, float sx, float sy, float sz) {
    const unsigned ui = (unsigned)((int)floorf(sx) - d.x0), uj = (unsigned)((int)floorf(sy) - d.y0);
    if (ui >= (unsigned)d.w || uj >= (unsigned)d.h) return false;  // (beyond every face's X or Y range)
    const long long tile = d.off + (long long)(uj >> 3) * mesh_tiles_across(d.w) + (ui >> 3);
    const int* list = g.tiles.pairs + (g.tiles.sums[tile >> 8] + g.tiles.start[tile]);
    const int nf = g.tiles.count[tile];
    const float limit = Proj::limit(g.depth_tol, sz);
    for (int q = 0; q < nf; ++q) {
        const int f = list[q];
        if (f == ed.z || f == ed.w) continue;
        const int p0 = g.faces[3 * (size_t)f], p1 = g.faces[3 * (size_t)f + 1], p2 = g.faces[3 * (size_t)f + 2];
        if (k == 0 && (p0 == ed.x || p1 == ed.x || p2 == ed.x)) continue;
        if (k == n && (p0 == ed.y || p1 == ed.y || p2 == ed.y)) continue;
        const MeshFace t = mesh_face(R, w, g.verts, g.faces, f);
        if (!t.solid()) continue;
        if (!(sx >= fminf(fminf(t.A.X, t.B.X), t.C.X) && sx <= fmaxf(fmaxf(t.A.X, t.B.X), t.C.X))) continue;
        if (!(sy >= fminf(fminf(t.A.Y, t.B.Y), t.C.Y) && sy <= fmaxf(fmaxf(t.A.Y, t.B.Y), t.C.Y))) continue;
        const float e0 = mesh_orient(t.B.X, t.B.Y, t.C.X, t.C.Y, sx, sy), e1 = mesh_orient(t.C.X, t.C.Y, t.A.X, t.A.Y, sx, sy),
                    e2 = mesh_orient(t.A.X, t.A.Y, t.B.X, t.B.Y, sx, sy);
        if (!((e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f))) continue;
        const float zf = ((e0 * t.A.Z + e1 * t.B.Z) + e2 * t.C.Z) / t.a;
        if (Proj::hidden(limit, sz, zf)) return true;  // (false for a NaN)
    }
    return false;
}
// The vertex of face f opposite the edge (i, j): the one index that is neither.  (For a face that names a vertex twice this is
// not the header's "index at the position the pair leaves out" -- but such a face has no normal, so its edges are sharp and
// the walk never asks for their opposite vertices: mesh_create's flags are what makes the shortcut safe.)
__device__ __forceinline__ int mesh_opposite(const int32_t* __restrict__ faces, int f, int i, int j) {
    const int p0 = faces[3 * (size_t)f], p1 = faces[3 * (size_t)f + 1], p2 = faces[3 * (size_t)f + 2];
    return p0 != i && p0 != j ? p0 : (p1 != i && p1 != j ? p1 : p2);
}
// the lines of edge e in the view: counted, and with WRITE stored from out[at] on; EXACT: the visibility rule.  One body for
// both passes and both rules, so the count and the writing pass cannot disagree.
template <bool WRITE, bool EXACT, class Proj>
__device__ __forceinline__ int mesh_walk(const MeshEdgeArgs<Proj>& g, const float* __restrict__ R, const typename Proj::View& w,
                                         const MeshView& d, int view_in_run, int e, long long at) {
    const int4 ed = g.edges[e];
    const MeshPoint A = mesh_project(R, w, g.verts + 3 * (size_t)ed.x), B = mesh_project(R, w, g.verts + 3 * (size_t)ed.y);
    if (!g.sharp[e]) {
        const MeshPoint c0 = mesh_project(R, w, g.verts + 3 * (size_t)mesh_opposite(g.faces, ed.z, ed.x, ed.y));
        const MeshPoint c1 = mesh_project(R, w, g.verts + 3 * (size_t)mesh_opposite(g.faces, ed.w, ed.x, ed.y));
        const float o0 = mesh_orient(A.X, A.Y, B.X, B.Y, c0.X, c0.Y), o1 = mesh_orient(A.X, A.Y, B.X, B.Y, c1.X, c1.Y);
        if ((o0 > 0.f && o1 < 0.f) || (o0 < 0.f && o1 > 0.f)) return 0;
    }
    const float dx = B.X - A.X, dy = B.Y - A.Y, dz = B.Z - A.Z;
    const int n = max(1, (int)ceilf(fmaxf(fabsf(dx), fabsf(dy))));  // (at most 4097: the view's box)
    const float fn = (float)n;
    int count = 0, k0 = 0, k1 = 0;
    bool open = false;
    float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
    auto close = [&] {
        if (k1 > k0) {
            const float ddx = x1 - x0, ddy = y1 - y0;
            const float len = sqrtf(ddx * ddx + ddy * ddy);
            if (len > 0.f && (g.join || len >= g.min_length)) {
                if (WRITE) {
                    g.out[at + count] = make_float4(x0, y0, x1, y1);
                    if (g.join) g.meta[at + count] = make_int2((e << 2) | (k0 == 0 ? 1 : 0) | (k1 == n ? 2 : 0), view_in_run);
                }
                ++count;
            }
        }
        open = false;
    };
    for (int k = 0; k <= n; ++k) {
        const float t = (float)k / fn;
        const float sx = A.X + t * dx, sy = A.Y + t * dy, sz = A.Z + t * dz;
        const unsigned ui = (unsigned)((int)floorf(sx) - d.x0), uj = (unsigned)((int)floorf(sy) - d.y0);
        bool vis = true;
        if (EXACT) {
            vis = !mesh_hidden(g, R, w, d, ed, k, n, sx, sy, sz);
        } else if (ui < (unsigned)d.w && uj < (unsigned)d.h) {
            const unsigned long long key = g.items[d.off + (long long)uj * d.w + ui];
            const int f = (int)(unsigned)key;
            if (key != 0 && f != ed.z && f != ed.w) {
                const MeshFace occ = mesh_face(R, w, g.verts, g.faces, f);
                float zf;
                (void)occ.depth(sx, sy, zf);
                vis = Proj::visible(Proj::limit(g.depth_tol, sz), sz, zf);
            }
        }
        if (vis) {
            if (!open) { open = true; k0 = k; x0 = sx; y0 = sy; }
            k1 = k; x1 = sx; y1 = sy;
        } else if (open) {
            close();
        }
    }
    if (open) close();
    return count;
}
template <bool WRITE, bool EXACT, class Proj>
__global__ void __launch_bounds__(256) k_mesh_edges(MeshEdgeArgs<Proj> g) {
    __shared__ int sw[4];
    const int block = (WRITE ? g.block0 : 0) + (int)blockIdx.x;
    const int view = block / g.nbE, e = (block % g.nbE) * 256 + threadIdx.x;
    const size_t slot = (size_t)block * 256 + threadIdx.x;
    int total;
    if (!WRITE) {
        const int c = e < g.E ? mesh_walk<false, EXACT>(g, g.views + 9 * (size_t)view, g.proj.at(view), g.descs[view], 0, e, 0) : 0;
        g.counts[slot] = c;
        mesh_block_scan(c, threadIdx.x, sw, total);
        if (threadIdx.x == 0) g.sums[block] = total;
    } else {
        const int c = g.counts[slot];
        const long long at = g.sums[block] - g.out0 + mesh_block_scan(c, threadIdx.x, sw, total);
        if (c) mesh_walk<true, EXACT>(g, g.views + 9 * (size_t)view, g.proj.at(view), g.descs[view], view - g.block0 / g.nbE, e, at);
    }
}
// sums[0 .. nb) -> their exclusive prefix sums in place, sums[nb] = the total (a block's sum is below 2^20: 256 edges of at most
// 2049 lines)
__global__ void __launch_bounds__(256) k_mesh_scan(long long* sums, int nb) {
    __shared__ int sw[4];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int base = 0; base < nb; base += 256) {
        const int i = base + tid;
        const int v = i < nb ? (int)sums[i] : 0;
        int total;
        const int ex = mesh_block_scan(v, tid, sw, total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) sums[nb] = carry;
}

// ------------------------------------------------------------------------------------------ joining pass
// One writing run of views: its L lines before the length test (pre, meta) in (view, edge, k0) order, so that a lower index
// within a view is the definition's lower index.  An end is (line << 1 | end), end 0 the start (k0), 1 the finish (k1).
// links: 3 words per (view of the run, vertex): the number of ends there and the first two of them.
static constexpr int kMeshJoinSpan = 256;  // the most segments one joined line replaces
template <class Proj>
struct MeshJoinArgs {
    const float* verts;
    const int4* edges;
    const float* views;     // the run's
    Proj proj;
    float tol2, min_length;
    const float4* pre;
    const int2* meta;
    int* links;
    int V, L;
    int* counts;            // per line: the lines of the chain it starts (0: it starts none)
    long long* sums;        // per 256 lines; scanned before the writing pass
    float4* out;
};
template <class Args>
__device__ __forceinline__ int mesh_end_vertex(const Args& g, int i, int end) {  // -1: the end lies inside its edge
    const int m = g.meta[i].x;
    if (!((m >> end) & 1)) return -1;
    const int4 ed = g.edges[m >> 2];
    return end ? ed.y : ed.x;
}
// the end linked to end `end` of line i, if there is one
template <class Args>
__device__ __forceinline__ bool mesh_linked(const Args& g, int i, int end, int& j, int& ej) {
    const int v = mesh_end_vertex(g, i, end);
    if (v < 0) return false;
    const int* l = g.links + 3 * ((size_t)g.meta[i].y * g.V + v);
    if (l[0] != 2) return false;
    const int s = l[1] == ((i << 1) | end) ? l[2] : l[1];
    j = s >> 1; ej = s & 1;
    return true;
}
template <class Args>
__device__ __forceinline__ float2 mesh_end_point(const Args& g, int i, int end) {
    const int v = mesh_end_vertex(g, i, end);
    if (v >= 0) {
        const MeshPoint p = mesh_project(g.views + 9 * (size_t)g.meta[i].y, g.proj.at(g.meta[i].y), g.verts + 3 * (size_t)v);
        return make_float2(p.X, p.Y);
    }
    const float4 l = g.pre[i];
    return end ? make_float2(l.z, l.w) : make_float2(l.x, l.y);
}
template <class Proj>
__global__ void __launch_bounds__(256) k_mesh_links(MeshJoinArgs<Proj> g) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= 2ll * g.L) return;
    const int i = (int)(u >> 1), end = (int)(u & 1);
    const int v = mesh_end_vertex(g, i, end);
    if (v < 0) return;
    int* l = g.links + 3 * ((size_t)g.meta[i].y * g.V + v);
    const int c = atomicAdd(l, 1);
    if (c < 2) l[1 + c] = (int)u;
}
// Whether line i starts a chain, and the end the chain enters it at.  Every walk follows links, which pair ends two by two, so
// it ends at a free end or where it began; the step limit L only keeps a damaged table from hanging the lane.
template <class Args>
__device__ __forceinline__ bool mesh_chain_start(const Args& g, int i, int& enter) {
    int j, ej;
    const bool linked0 = mesh_linked(g, i, 0, j, ej), linked1 = mesh_linked(g, i, 1, j, ej);
    if (!linked0 || !linked1) {  // an end line of a path: it starts it when the line at the other free end has no lower index
        enter = !linked0 ? 0 : 1;
        int c = i, ce = enter;
        for (int steps = 0; steps < g.L && mesh_linked(g, c, 1 - ce, j, ej); ++steps) { c = j; ce = ej; }
        return i <= c;
    }
    enter = 0;  // inside a path, or on a cycle: that one starts with its lowest line
    int c = i, ce = 0;
    for (int steps = 0; steps < g.L; ++steps) {
        if (!mesh_linked(g, c, 1 - ce, j, ej) || j < i) return false;
        if (j == i) return true;
        c = j; ce = ej;
    }
    return false;
}
// A chain point: an end of a line.  P_0 is the end the chain enters its first line at; every later point is the far end of
// the next line.
struct MeshChainAt { int line, end; bool first; };
template <class Args>
__device__ __forceinline__ bool mesh_chain_next(const Args& g, int i0, int enter0, MeshChainAt& p) {
    if (p.first) { p.end = 1 - p.end; p.first = false; return true; }
    int j, ej;
    if (!mesh_linked(g, p.line, p.end, j, ej) || (j == i0 && ej == enter0)) return false;  // a free end, or the cycle is closed
    p.line = j; p.end = 1 - ej;
    return true;
}
// the greedy simplification of the chain that starts with line i0: its lines counted, and with WRITE stored from out[at] on
template <bool WRITE, class Args>
__device__ __forceinline__ int mesh_chain_lines(const Args& g, int i0, int enter0, long long at) {
    int count = 0;
    auto emit = [&](float2 p, float2 q) {
        const float ddx = q.x - p.x, ddy = q.y - p.y;
        const float len = sqrtf(ddx * ddx + ddy * ddy);
        if (len > 0.f && len >= g.min_length) {
            if (WRITE) g.out[at + count] = make_float4(p.x, p.y, q.x, q.y);
            ++count;
        }
    };
    MeshChainAt a{i0, enter0, true};
    float2 Pa = mesh_end_point(g, i0, enter0);
    MeshChainAt cur = a;
    mesh_chain_next(g, i0, enter0, cur);  // P_1
    float2 Pc = mesh_end_point(g, cur.line, cur.end);
    int span = 1;  // cur is P_(a + span)
    for (int steps = 0; steps < g.L; ++steps) {
        MeshChainAt nxt = cur;
        if (!mesh_chain_next(g, i0, enter0, nxt)) break;
        const float2 Pj = mesh_end_point(g, nxt.line, nxt.end);
        const float dx = Pj.x - Pa.x, dy = Pj.y - Pa.y;
        const float L2 = dx * dx + dy * dy;
        bool ok = L2 > 0.f && span + 1 <= kMeshJoinSpan;
        MeshChainAt q = a;
        for (int t = 0; t < span && ok; ++t) {
            mesh_chain_next(g, i0, enter0, q);
            const float2 Pi = mesh_end_point(g, q.line, q.end);
            const float wx = Pi.x - Pa.x, wy = Pi.y - Pa.y;
            const float s = dx * wx + dy * wy, c = dx * wy - dy * wx;
            ok = 0.f <= s && s <= L2 && c * c <= g.tol2 * L2;
        }
        if (ok) {
            ++span;
        } else {
            emit(Pa, Pc);
            a = cur; Pa = Pc; span = 1;
        }
        cur = nxt; Pc = Pj;
    }
    emit(Pa, Pc);
    return count;
}
template <bool WRITE, class Proj>
__global__ void __launch_bounds__(256) k_mesh_chains(MeshJoinArgs<Proj> g) {
    __shared__ int sw[4];
    const int i = (int)blockIdx.x * 256 + threadIdx.x;  // (counts holds 256 words per block)
    int total, enter;
    if (!WRITE) {
        const int c = i < g.L && mesh_chain_start(g, i, enter) ? mesh_chain_lines<false>(g, i, enter, 0) : 0;
        g.counts[i] = c;
        mesh_block_scan(c, threadIdx.x, sw, total);
        if (threadIdx.x == 0) g.sums[blockIdx.x] = total;
    } else {
        const int c = g.counts[i];
        const long long at = g.sums[blockIdx.x] + mesh_block_scan(c, threadIdx.x, sw, total);
        if (c && mesh_chain_start(g, i, enter)) mesh_chain_lines<true>(g, i, enter, at);
    }
}
// starts[q] (a line index of the run, 0 .. L) -> the number of joined lines before it, in place
__global__ void __launch_bounds__(256) k_mesh_starts(const int* __restrict__ counts, const long long* __restrict__ sums, long long* starts, int n) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const long long idx = starts[q];
    long long s = sums[idx >> 8];
    for (long long k = idx & ~255ll; k < idx; ++k) s += counts[k];
    starts[q] = s;
}

// ------------------------------------------------------------------------------------------ host: the mesh
namespace {
struct Incidence { uint64_t pair; int32_t face; };
void face_normal(const float* v, const int32_t* tri, double n[3]) {
    const float *p0 = v + 3 * (size_t)tri[0], *p1 = v + 3 * (size_t)tri[1], *p2 = v + 3 * (size_t)tri[2];
    const double u[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
    const double w[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
    n[0] = u[1] * w[2] - u[2] * w[1]; n[1] = u[2] * w[0] - u[0] * w[2]; n[2] = u[0] * w[1] - u[1] * w[0];
}
double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
}  // namespace

fdcm_mesh* mesh_create(const float* vertices, int64_t V, const int32_t* faces, int64_t F, double crease_cos) {
    for (int64_t i = 0; i < 3 * V; ++i)
        if (!std::isfinite(vertices[i])) throw std::string("vertex " + std::to_string(i / 3) + " is not finite");
    for (int64_t i = 0; i < 3 * F; ++i)
        if (faces[i] < 0 || faces[i] >= V) throw std::string("face " + std::to_string(i / 3) + " has an index outside 0 .. n_vertices - 1");
    std::unique_ptr<fdcm_mesh> m(new fdcm_mesh);
    m->V = V; m->F = F;
    m->vertices.assign(vertices, vertices + 3 * V);
    m->faces.assign(faces, faces + 3 * F);
    std::vector<Incidence> inc;
    inc.reserve((size_t)3 * F);
    for (int64_t f = 0; f < F; ++f) {
        const int32_t* t = faces + 3 * f;
        uint64_t seen[3];
        int ns = 0;
        for (int k = 0; k < 3; ++k) {
            const int32_t a = t[k], b = t[(k + 1) % 3];
            if (a == b) continue;
            const uint64_t pair = ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
            if (std::find(seen, seen + ns, pair) != seen + ns) continue;
            seen[ns++] = pair;
            inc.push_back({pair, (int32_t)f});
        }
    }
    std::sort(inc.begin(), inc.end(), [](const Incidence& a, const Incidence& b) { return a.pair != b.pair ? a.pair < b.pair : a.face < b.face; });
    for (size_t i = 0; i < inc.size();) {
        size_t j = i;
        while (j < inc.size() && inc[j].pair == inc[i].pair) ++j;
        const int32_t a = (int32_t)(inc[i].pair >> 32), b = (int32_t)(inc[i].pair & 0xffffffffu);
        if (j - i > 2)
            throw std::string("non-manifold edge (" + std::to_string(a) + ", " + std::to_string(b) + "): " + std::to_string(j - i) + " faces");
        const int32_t f0 = inc[i].face, f1 = j - i == 2 ? inc[i + 1].face : -1;
        bool sharp = f1 < 0;
        if (sharp) {
            ++m->n_boundary;
        } else {
            double n0[3], n1[3];
            face_normal(vertices, faces + 3 * (size_t)f0, n0);
            face_normal(vertices, faces + 3 * (size_t)f1, n1);
            const bool zero0 = n0[0] == 0 && n0[1] == 0 && n0[2] == 0, zero1 = n1[0] == 0 && n1[1] == 0 && n1[2] == 0;
            sharp = zero0 || zero1 || std::fabs(dot3(n0, n1)) < (crease_cos * std::sqrt(dot3(n0, n0))) * std::sqrt(dot3(n1, n1));
        }
        m->edges.insert(m->edges.end(), {a, b, f0, f1});
        m->sharp.push_back(sharp ? 1 : 0);
        m->n_sharp += sharp;
        i = j;
    }
    m->E = (int64_t)m->sharp.size();
    return m.release();
}

// ------------------------------------------------------------------------------------------ host: the views
namespace {
size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
// What a call holds on the device, in PixelScratch's members: keys -- the views, the mesh's tables and the part's view
// records; comps -- the boxes; pixels -- the part's item buffers; parent -- its list of large faces; counts -- its per-edge
// counts and block sums; out -- its lines.
// The pinhole's positions, where it has them, lie behind the view records in keys.
template <class Proj>
struct MeshDevice {
    PixelScratch s;
    const fdcm_mesh* m;
    int64_t n_views;
    Proj proj;                   // of view 0 on: a part or a run takes proj.from(its first view)
    const float *views, *verts;
    const int32_t* faces;
    const int4* edges;
    const uint8_t* sharp;
    MeshView* descs;
    std::vector<int32_t> boxes;  // 4 per view, checked
    bool exact, join;            // the call's mode: tile lists in place of item buffers; link tables per view
    std::vector<long long> pairs;  // exact: (face, tile) pairs per view
    MeshTiles tiles{};           // exact: the part's, in pixels and parent
    int nbE() const { return (int)((m->E + 255) / 256); }
    int nbF() const { return (int)((m->F + 15) / 16); }
    int nbF256() const { return (int)((m->F + 255) / 256); }

    // uploads the mesh and the views, runs the projection pass and refuses the views it must
    MeshDevice(const fdcm_mesh* mesh, const float* host_views, const float* host_positions, int64_t n, Proj pj, bool exact_ = false,
               bool join_ = false)
        : m(mesh), n_views(n), proj(pj), exact(exact_), join(join_) {
        const size_t o_views = 0, o_verts = align16((size_t)n * 36), o_faces = align16(o_verts + (size_t)m->V * 12),
                     o_edges = align16(o_faces + (size_t)m->F * 12), o_sharp = o_edges + (size_t)m->E * 16,
                     o_descs = align16(o_sharp + (size_t)m->E), o_positions = align16(o_descs + (size_t)n * sizeof(MeshView)),
                     bytes = host_positions ? o_positions + (size_t)n * 12 : o_descs + (size_t)n * sizeof(MeshView);
        s.take(s.keys, bytes, FDCM_FILL_PIXEL_KEYS);
        char* base = (char*)s.keys.p;
        if constexpr (std::is_same<Proj, MeshPinhole>::value) {
            FDCM_HIP(hipMemcpy(base + o_positions, host_positions, (size_t)n * 12, hipMemcpyHostToDevice));
            proj.positions = (const float*)(base + o_positions);
        }
        FDCM_HIP(hipMemcpy(base + o_views, host_views, (size_t)n * 36, hipMemcpyHostToDevice));
        FDCM_HIP(hipMemcpy(base + o_verts, m->vertices.data(), (size_t)m->V * 12, hipMemcpyHostToDevice));
        FDCM_HIP(hipMemcpy(base + o_faces, m->faces.data(), (size_t)m->F * 12, hipMemcpyHostToDevice));
        FDCM_HIP(hipMemcpy(base + o_edges, m->edges.data(), (size_t)m->E * 16, hipMemcpyHostToDevice));
        FDCM_HIP(hipMemcpy(base + o_sharp, m->sharp.data(), (size_t)m->E, hipMemcpyHostToDevice));
        views = (const float*)(base + o_views); verts = (const float*)(base + o_verts); faces = (const int32_t*)(base + o_faces);
        edges = (const int4*)(base + o_edges); sharp = (const uint8_t*)(base + o_sharp); descs = (MeshView*)(base + o_descs);
        boxes.resize((size_t)4 * n);
        for (int64_t v = 0; v < n; ++v) { boxes[4 * v] = boxes[4 * v + 1] = INT32_MAX; boxes[4 * v + 2] = boxes[4 * v + 3] = INT32_MIN; }
        s.take(s.comps, boxes.size() * 4 + (exact ? (size_t)n * 8 : 0), FDCM_FILL_PIXEL_COMPS);  // (exact: the views' pair totals behind)
        FDCM_HIP(hipMemcpy(s.comps.p, boxes.data(), boxes.size() * 4, hipMemcpyHostToDevice));
        const int nbV = (int)((m->V + 255) / 256);  // (at most 2^14 blocks a view and 2^16 views: one grid)
        hipLaunchKernelGGL(k_mesh_boxes<Proj>, dim3((unsigned)(nbV * n)), dim3(256), 0, nullptr, verts, (int)m->V, nbV, views, proj,
                           s.comps.as<int32_t>());
        FDCM_HIP(hipGetLastError());
        FDCM_HIP(hipMemcpy(boxes.data(), s.comps.p, boxes.size() * 4, hipMemcpyDeviceToHost));
        for (int64_t v = 0; v < n; ++v) {
            const int64_t w = (int64_t)boxes[4 * v + 2] - boxes[4 * v] + 1, h = (int64_t)boxes[4 * v + 3] - boxes[4 * v + 1] + 1;
            if (w > kMeshMaxSpan || h > kMeshMaxSpan)
                throw std::string("view " + std::to_string(v) + " spans more than 4096 pixels on a side (or a coordinate is not below 2^30" +
                                  (std::is_same<Proj, MeshPinhole>::value ? ", or a vertex is nearer than `near`)" : ")"));
        }
        if (!exact) return;
        // the (face, tile) pairs of every view: what its lists take
        unsigned long long* totals = reinterpret_cast<unsigned long long*>(s.comps.as<int32_t>() + boxes.size());
        FDCM_HIP(hipMemsetAsync(totals, 0, (size_t)n * 8, nullptr));
        hipLaunchKernelGGL((k_mesh_tiles<0, Proj>), dim3((unsigned)(nbF256() * n)), dim3(256), 0, nullptr, verts, faces, (int)m->F, nbF256(), views, proj,
                           (const int32_t*)s.comps.as<int32_t>(), (const MeshView*)nullptr, MeshTiles{}, totals);
        FDCM_HIP(hipGetLastError());
        pairs.resize((size_t)n);
        FDCM_HIP(hipMemcpy(pairs.data(), totals, (size_t)n * 8, hipMemcpyDeviceToHost));
        for (int64_t v = 0; v < n; ++v)
            if (pairs[(size_t)v] > (1ll << 28))
                throw std::string("view " + std::to_string(v) + " needs more than 2^28 entries in its tiles' face lists");
    }
    size_t view_items(int64_t v) const { return (size_t)(boxes[4 * v + 2] - boxes[4 * v] + 1) * (size_t)(boxes[4 * v + 3] - boxes[4 * v + 1] + 1); }
    size_t view_tiles(int64_t v) const {
        return (size_t)mesh_tiles_across(boxes[4 * v + 2] - boxes[4 * v] + 1) * (size_t)mesh_tiles_across(boxes[4 * v + 3] - boxes[4 * v + 1] + 1);
    }
    // what a view adds to its part: item buffer and list of large faces, or tiles (12 bytes each, and their share of the block
    // sums) and face lists; the edge pass's counts; with joining its link table
    size_t view_bytes(int64_t v) const {
        return (exact ? view_tiles(v) * 13 + (size_t)pairs[(size_t)v] * 4 : view_items(v) * 8 + (size_t)m->F * 8) + (size_t)nbE() * (256 * 4 + 8) +
               (join ? (size_t)m->V * 12 : 0);
    }
    // the views [v0, v0 + P) of one part: at most kMeshPartBytes (one view whatever it takes), FDCM_MESH_PART views at most
    int64_t part_views(int64_t v0) const {
        const int forced = test_switches().mesh_part;
        size_t bytes = 0;
        int64_t P = 0;
        while (v0 + P < n_views && (P == 0 || (bytes + view_bytes(v0 + P) <= kMeshPartBytes && (forced == 0 || P < forced)))) bytes += view_bytes(v0 + P++);
        return P;
    }
    // the item buffers of the part, rastered; returns their total of keys
    size_t raster(int64_t v0, int64_t P) {
        std::vector<MeshView> d((size_t)P);
        size_t total = 0;
        for (int64_t i = 0; i < P; ++i) {
            const int32_t* b = &boxes[4 * (v0 + i)];
            d[i] = MeshView{b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1, (long long)total};
            total += view_items(v0 + i);
        }
        s.take(s.pixels, total * 8, FDCM_FILL_PIXEL_PIXELS);
        s.take(s.parent, 8 + (size_t)P * (size_t)m->F * 8, FDCM_FILL_PIXEL_PARENT);
        FDCM_HIP(hipMemcpy(descs, d.data(), (size_t)P * sizeof(MeshView), hipMemcpyHostToDevice));
        FDCM_HIP(hipMemsetAsync(s.pixels.p, 0, total * 8, nullptr));
        FDCM_HIP(hipMemsetAsync(s.parent.p, 0, 8, nullptr));
        const float* pv = views + 9 * (size_t)v0;
        const Proj pp = proj.from(v0);
        hipLaunchKernelGGL(k_mesh_raster<Proj>, dim3((unsigned)(P * nbF())), dim3(256), 0, nullptr, verts, faces, (int)m->F, nbF(), pv, pp,
                           (const MeshView*)descs, s.pixels.as<unsigned long long>(), s.parent.as<unsigned long long>());
        hipLaunchKernelGGL(k_mesh_raster_big<Proj>, dim3(kBigGrid), dim3(256), 0, nullptr, verts, faces, pv, pp, (const MeshView*)descs,
                           s.pixels.as<unsigned long long>(), (const unsigned long long*)s.parent.as<unsigned long long>());
        FDCM_HIP(hipGetLastError());
        return total;
    }
    // exact visibility: the faces of the part's views binned into `tiles` (pixels: block sums, counts, cursors, starts; parent:
    // the lists)
    void bin(int64_t v0, int64_t P) {
        std::vector<MeshView> d((size_t)P);
        size_t T = 0;
        long long n_pairs = 0;
        for (int64_t i = 0; i < P; ++i) {
            const int32_t* b = &boxes[4 * (v0 + i)];
            d[i] = MeshView{b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1, (long long)T};
            T += view_tiles(v0 + i);
            n_pairs += pairs[(size_t)(v0 + i)];
        }
        const size_t nbT = (T + 255) / 256, o_count = align16((nbT + 1) * 8);
        s.take(s.pixels, o_count + T * 12, FDCM_FILL_PIXEL_PIXELS);
        s.take(s.parent, std::max<size_t>(1, (size_t)n_pairs) * 4, FDCM_FILL_PIXEL_PARENT);
        tiles.sums = s.pixels.as<long long>();
        tiles.count = (int*)((char*)s.pixels.p + o_count); tiles.cursor = tiles.count + T; tiles.start = tiles.cursor + T;
        tiles.pairs = s.parent.as<int>(); tiles.n_pairs = n_pairs;
        FDCM_HIP(hipMemcpy(descs, d.data(), (size_t)P * sizeof(MeshView), hipMemcpyHostToDevice));
        FDCM_HIP(hipMemsetAsync(tiles.count, 0, T * 8, nullptr));  // (counts and cursors)
        const float* pv = views + 9 * (size_t)v0;
        const int32_t* pb = s.comps.as<int32_t>() + 4 * (size_t)v0;
        const dim3 grid((unsigned)(P * nbF256()));
        const Proj pp = proj.from(v0);
        hipLaunchKernelGGL((k_mesh_tiles<1, Proj>), grid, dim3(256), 0, nullptr, verts, faces, (int)m->F, nbF256(), pv, pp, pb, (const MeshView*)descs, tiles,
                           (unsigned long long*)nullptr);
        hipLaunchKernelGGL(k_mesh_tile_starts, dim3((unsigned)nbT), dim3(256), 0, nullptr, tiles, (long long)T);
        hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(256), 0, nullptr, tiles.sums, (int)nbT);
        hipLaunchKernelGGL((k_mesh_tiles<2, Proj>), grid, dim3(256), 0, nullptr, verts, faces, (int)m->F, nbF256(), pv, pp, pb, (const MeshView*)descs, tiles,
                           (unsigned long long*)nullptr);
        FDCM_HIP(hipGetLastError());
    }
};
struct HostLines {  // the call's lines until they are the caller's
    float* p = nullptr;
    ~HostLines() { std::free(p); }
    void grow(size_t lines) {
        float* q = (float*)std::realloc(p, std::max<size_t>(1, lines) * 16);
        if (!q) throw std::bad_alloc();
        p = q;
    }
};
}  // namespace

namespace {
// One writing run with joining: the run's `lines` lines before the length test are in `labels` (pre, meta), written by the edge
// pass; links, chains and the joined lines follow.  starts: where the run's views begin among those lines, and their total
// behind; on return the same for the joined lines, which are in `out`.  labels: pre, meta, the block sums, the starts, the
// counts and the link table, each written here before it is read.
struct JoinRun {
    size_t o_meta, o_sums, o_starts, o_counts, o_links, bytes;
    int nbL;
    JoinRun(long long lines, int64_t views, int64_t V) {
        nbL = (int)((lines + 255) / 256);
        o_meta = (size_t)lines * 16;
        o_sums = align16(o_meta + (size_t)lines * 8);
        o_starts = o_sums + ((size_t)nbL + 1) * 8;
        o_counts = o_starts + ((size_t)views + 1) * 8;
        o_links = align16(o_counts + (size_t)nbL * 256 * 4);
        bytes = o_links + (size_t)views * (size_t)V * 12;
    }
};
template <class Proj>
void join_run(MeshDevice<Proj>& dev, const JoinRun& r, const float* run_views, const Proj& run_proj, long long lines, std::vector<long long>& starts,
              float tol, float min_length) {
    char* base = (char*)dev.s.labels.p;
    const size_t views = starts.size() - 1;
    MeshJoinArgs<Proj> j;
    j.verts = dev.verts; j.edges = dev.edges; j.views = run_views; j.proj = run_proj; j.tol2 = tol * tol; j.min_length = min_length;
    j.pre = (const float4*)base; j.meta = (const int2*)(base + r.o_meta); j.links = (int*)(base + r.o_links); j.V = (int)dev.m->V; j.L = (int)lines;
    j.counts = (int*)(base + r.o_counts); j.sums = (long long*)(base + r.o_sums); j.out = nullptr;
    long long* d_starts = (long long*)(base + r.o_starts);
    FDCM_HIP(hipMemsetAsync(j.links, 0, views * (size_t)dev.m->V * 12, nullptr));
    FDCM_HIP(hipMemcpy(d_starts, starts.data(), starts.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_mesh_links<Proj>, dim3((unsigned)((2 * lines + 255) / 256)), dim3(256), 0, nullptr, j);
    hipLaunchKernelGGL((k_mesh_chains<false, Proj>), dim3((unsigned)r.nbL), dim3(256), 0, nullptr, j);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(256), 0, nullptr, j.sums, r.nbL);
    hipLaunchKernelGGL(k_mesh_starts, dim3((unsigned)((starts.size() + 255) / 256)), dim3(256), 0, nullptr, (const int*)j.counts, (const long long*)j.sums,
                       d_starts, (int)starts.size());
    FDCM_HIP(hipGetLastError());
    FDCM_HIP(hipMemcpy(starts.data(), d_starts, starts.size() * 8, hipMemcpyDeviceToHost));
    const long long joined = starts.back();
    if (joined == 0) return;
    dev.s.take(dev.s.out, (size_t)joined * 16, FDCM_FILL_PIXEL_OUT);
    j.out = dev.s.out.template as<float4>();
    hipLaunchKernelGGL((k_mesh_chains<true, Proj>), dim3((unsigned)r.nbL), dim3(256), 0, nullptr, j);
    FDCM_HIP(hipGetLastError());
}
template <class Proj>
void launch_edges(const MeshEdgeArgs<Proj>& g, bool write, bool exact, int blocks) {
    const dim3 grid((unsigned)blocks), wg(256);
    if (write && exact) hipLaunchKernelGGL((k_mesh_edges<true, true, Proj>), grid, wg, 0, nullptr, g);
    else if (write) hipLaunchKernelGGL((k_mesh_edges<true, false, Proj>), grid, wg, 0, nullptr, g);
    else if (exact) hipLaunchKernelGGL((k_mesh_edges<false, true, Proj>), grid, wg, 0, nullptr, g);
    else hipLaunchKernelGGL((k_mesh_edges<false, false, Proj>), grid, wg, 0, nullptr, g);
}

// the driver of both projections: parts, writing runs, join passes
template <class Proj>
void view_lines(int device, const fdcm_mesh* m, const float* views, const float* positions, int64_t n_views, Proj pj, const fdcm_mesh_line_params& p,
                float** lines_out, int64_t* offsets_out) {
    FDCM_HIP(hipSetDevice(device));
    const bool exact = p.visibility == FDCM_MESH_VIS_EXACT, join = p.join_tolerance >= 0.f;
    MeshDevice<Proj> dev(m, views, positions, n_views, pj, exact, join);
    HostLines host;
    std::vector<int64_t> offsets((size_t)n_views + 1, 0);
    std::vector<long long> view_at, starts;
    int64_t done = 0;
    const int nbE = dev.nbE();
    for (int64_t v0 = 0; v0 < n_views;) {
        const int64_t P = dev.part_views(v0);
        if (exact) dev.bin(v0, P); else dev.raster(v0, P);
        const int nb = (int)(P * nbE);
        dev.s.take(dev.s.counts, (size_t)nb * 256 * 4 + ((size_t)nb + 1) * 8, FDCM_FILL_PIXEL_COUNTS);
        MeshEdgeArgs<Proj> g;
        g.verts = dev.verts; g.faces = dev.faces; g.edges = dev.edges; g.sharp = dev.sharp; g.E = (int)m->E; g.nbE = nbE;
        g.views = dev.views + 9 * (size_t)v0; g.proj = dev.proj.from(v0); g.depth_tol = p.depth_tol; g.min_length = p.min_length;
        g.descs = dev.descs; g.items = exact ? nullptr : dev.s.pixels.template as<unsigned long long>(); g.tiles = dev.tiles;
        g.join = join ? 1 : 0; g.meta = nullptr;
        g.sums = dev.s.counts.template as<long long>(); g.counts = (int*)(g.sums + nb + 1); g.out = nullptr; g.block0 = 0; g.out0 = 0;
        launch_edges(g, false, exact, nb);
        hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(256), 0, nullptr, g.sums, nb);
        FDCM_HIP(hipGetLastError());
        // where each view of the part begins among its lines, and their total
        view_at.assign((size_t)P + 1, 0);
        FDCM_HIP(hipMemcpy2D(view_at.data(), 8, g.sums, (size_t)nbE * 8, 8, (size_t)P, hipMemcpyDeviceToHost));
        FDCM_HIP(hipMemcpy(&view_at[(size_t)P], g.sums + nb, 8, hipMemcpyDeviceToHost));
        const long long total = view_at[(size_t)P];
        if (done + total >= ((int64_t)1 << 31)) throw std::string("the views give 2^31 lines or more");
        if (!join) {
            for (int64_t i = 0; i < P; ++i) offsets[(size_t)(v0 + i)] = done + view_at[(size_t)i];
            if (total > 0) host.grow((size_t)(done + total));
        }
        // the writing passes: runs of the part's views whose lines fit kMeshWriteBytes (FDCM_MESH_PART = N: 16 N lines), a view
        // with more than that on its own, so that `out` is bounded like the part's other buffers.  With joining a line of the run
        // takes 44 bytes: itself, its edge and view, its count and the joined line.
        const int forced = test_switches().mesh_part;
        const long long room = forced ? 16ll * forced : (long long)(kMeshWriteBytes / (join ? 44 : 16));
        for (int64_t a = 0; a < P && (total > 0 || join);) {
            int64_t b = a + 1;
            while (b < P && view_at[(size_t)b + 1] - view_at[(size_t)a] <= room) ++b;
            const long long lines = view_at[(size_t)b] - view_at[(size_t)a];
            if (join) {
                if (lines >= (1ll << 30)) throw std::string("a run of views gives 2^30 lines or more before joining");
                starts.resize((size_t)(b - a) + 1);
                for (int64_t i = a; i <= b; ++i) starts[(size_t)(i - a)] = view_at[(size_t)i] - view_at[(size_t)a];
                if (lines > 0) {
                    const JoinRun r(lines, b - a, m->V);
                    dev.s.take(dev.s.labels, r.bytes, FDCM_FILL_PIXEL_LABELS);
                    g.out = dev.s.labels.template as<float4>(); g.meta = (int2*)((char*)dev.s.labels.p + r.o_meta);
                    g.block0 = (int)(a * nbE); g.out0 = view_at[(size_t)a];
                    launch_edges(g, true, exact, (int)((b - a) * nbE));
                    FDCM_HIP(hipGetLastError());
                    join_run(dev, r, g.views + 9 * (size_t)a, g.proj.from(a), lines, starts, p.join_tolerance, p.min_length);
                }
                const long long joined = starts.back();
                if (done + joined >= ((int64_t)1 << 31)) throw std::string("the views give 2^31 lines or more");
                for (int64_t i = a; i < b; ++i) offsets[(size_t)(v0 + i)] = done + starts[(size_t)(i - a)];
                if (joined > 0) {
                    host.grow((size_t)(done + joined));
                    FDCM_HIP(hipMemcpy(host.p + 4 * (size_t)done, dev.s.out.p, (size_t)joined * 16, hipMemcpyDeviceToHost));
                }
                done += joined;
            } else if (lines > 0) {
                dev.s.take(dev.s.out, (size_t)lines * 16, FDCM_FILL_PIXEL_OUT);
                g.out = dev.s.out.template as<float4>(); g.block0 = (int)(a * nbE); g.out0 = view_at[(size_t)a];
                launch_edges(g, true, exact, (int)((b - a) * nbE));
                FDCM_HIP(hipGetLastError());
                FDCM_HIP(hipMemcpy(host.p + 4 * (size_t)(done + view_at[(size_t)a]), dev.s.out.p, (size_t)lines * 16, hipMemcpyDeviceToHost));
            }
            a = b;
        }
        if (!join) done += total;
        v0 += P;
    }
    offsets[(size_t)n_views] = done;
    std::copy(offsets.begin(), offsets.end(), offsets_out);
    if (done > 0) { *lines_out = host.p; host.p = nullptr; }
}
template <class Proj>
void view_items(int device, const fdcm_mesh* m, const float* view, const float* position, Proj pj, int32_t* box_out, uint64_t* keys_out,
                int64_t capacity) {
    FDCM_HIP(hipSetDevice(device));
    MeshDevice<Proj> dev(m, view, position, 1, pj);
    std::copy(dev.boxes.begin(), dev.boxes.end(), box_out);
    if (!keys_out) return;
    if ((int64_t)dev.view_items(0) > capacity)
        throw std::string("keys_out holds " + std::to_string(capacity) + " keys, the view's box has " + std::to_string(dev.view_items(0)));
    const size_t total = dev.raster(0, 1);
    FDCM_HIP(hipMemcpy(keys_out, dev.s.pixels.p, total * 8, hipMemcpyDeviceToHost));
}
}  // namespace

void mesh_view_lines(int device, const fdcm_mesh* m, const float* views, int64_t n_views, float scale, const fdcm_mesh_line_params& p,
                     float** lines_out, int64_t* offsets_out) {
    view_lines(device, m, views, nullptr, n_views, MeshOrtho{scale}, p, lines_out, offsets_out);
}
void mesh_view_items(int device, const fdcm_mesh* m, const float* view, float scale, int32_t* box_out, uint64_t* keys_out, int64_t capacity) {
    view_items(device, m, view, nullptr, MeshOrtho{scale}, box_out, keys_out, capacity);
}
void mesh_view_lines_cam(int device, const fdcm_mesh* m, const float* views, const float* positions, int64_t n_views, const fdcm_mesh_camera& cam,
                         const fdcm_mesh_line_params& p, float** lines_out, int64_t* offsets_out) {
    view_lines(device, m, views, positions, n_views, MeshPinhole{cam.focal, cam.near, nullptr}, p, lines_out, offsets_out);
}
void mesh_view_items_cam(int device, const fdcm_mesh* m, const float* view, const float* position, const fdcm_mesh_camera& cam, int32_t* box_out,
                         uint64_t* keys_out, int64_t capacity) {
    view_items(device, m, view, position, MeshPinhole{cam.focal, cam.near, nullptr}, box_out, keys_out, capacity);
}

}  // namespace fdcm
