// fdcm_image.hip -- DT3 seeds from pixels on gfx950: oriented edge pixels of a grey image as a label image, and pass 1 of the
// distance transform with its seeds taken from a label image (include/fdcm.h, "feature maps from images").
//
//   edge_tile<S, HYST> the one body of the two edge kernels: the tile and its halo into LDS (load_clamped_tile), smoothed for
//                      S > 0, integer Sobel, thresholded and thinned along the gradient, the edge's tangent binned by
//                      closest_orientation over the build's keys
//   k_edge_labels      edge_tile<0, false>: uint8 image -> label image by one threshold    read W H, write W H
//   k_coldesc_labels   k_coldesc_tile's sibling: the bitmap tile in LDS comes from the label image instead of RasterLines, the
//                      descriptor step (coldesc_from_bits) is shared                     read m W H (from L2), write ~V/16
//   k_edge_candidates<S>, k_edge_tiles, k_edge_borders, k_edge_roots, k_edge_resolve
//                      the same label image with smoothing, hysteresis and a minimum component size: candidates
//                      (edge_tile<S, true>: thinned, m2 >= low^2) with their provisional labels and strong flags, their
//                      8-connected components by the tiled labeller of fdcm_unionfind.h with one partition (a tile merged in
//                      LDS, the pairs across tile borders in global memory), strong flag and size per root, and the candidates
//                      of the other roots back to 255
//   k_pyr_down         the next level of the image pyramid: the smooth = 2 image at the even coordinates (include/fdcm.h, "image
//                      pyramid"); a level-l build runs it l times in front of the edge kernels   read W H, write W H / 4
// All index with the caller's sizes only: every load is of a pixel inside [0, width) x [0, height), every store inside the label
// image, the words of the image's own pixels or the descriptors of the block's own columns.
#include <algorithm>

#include "fdcm_build_dev.h"
#include "fdcm_internal.h"
#include "fdcm_unionfind.h"

namespace fdcm {

// ------------------------------------------------------------------------------------------ image -> labels
static constexpr int kEdgeTW = kTileW, kEdgeTH = kTileH;  // pixels a workgroup labels: the tiles of the component kernels
static constexpr int kEdgeHalo = 2;                       // 1 for Sobel + 1 for the neighbours' m2
static constexpr int kEdgePW = kEdgeTW + 2 * kEdgeHalo, kEdgePH = kEdgeTH + 2 * kEdgeHalo;  // pixels held
static constexpr int kEdgeMW = kEdgeTW + 2, kEdgeMH = kEdgeTH + 2;                          // squared magnitudes held
static constexpr unsigned kStrongBit = 0x80000000u;  // roots[]: bit 31 strong, bits 0-30 the component's candidates

// Sobel at tile position (r, c) of the held pixels (replicate border: the loads clamped the coordinates)
__device__ __forceinline__ void sobel_at(const unsigned char (*px)[kEdgePW + 4], int r, int c, int& gx, int& gy) {
    const int a = px[r - 1][c - 1], b = px[r - 1][c], d = px[r - 1][c + 1];
    const int e = px[r][c - 1], f = px[r][c + 1];
    const int g = px[r + 1][c - 1], h = px[r + 1][c], i = px[r + 1][c + 1];
    gx = (d + 2 * f + i) - (a + 2 * e + g);
    gy = (g + 2 * h + i) - (a + 2 * b + d);
}

// PH x PW pixels of the image from (xa, ya) on into LDS: the pixels inside the image as aligned dwords where all four bytes are
// the row's and single bytes at the ragged ends, the columns and rows outside it replicated (the row's first / last pixel).
template <int PH, int PW, int STR>
__device__ __forceinline__ void load_clamped_tile(unsigned char (*px)[STR], const uint8_t* __restrict__ image, int W, int H, int stride,
                                                  int xa, int ya, int tid) {
    constexpr int kRowDwords = (PW + 3 + 3) / 4;      // aligned dwords that cover a row of held pixels wherever it starts
    const int lo = max(xa, 0), hi = min(xa + PW, W);  // the held columns inside the image: [lo, hi), never empty
    for (int idx = tid; idx < PH * kRowDwords; idx += 256) {
        const int r = idx / kRowDwords, j = idx - r * kRowDwords;
        const int y = min(max(ya + r, 0), H - 1);
        const uint8_t* rp = image + (size_t)y * stride;
        const int mis = (int)((uintptr_t)(rp + lo) & 3u);  // bytes between the aligned address below the first pixel and it
        const int xf = lo - mis + 4 * j;                   // column of the dword's first byte
        if (xf >= hi) continue;
        if (xf >= lo && xf + 4 <= hi) {
            const unsigned v = *reinterpret_cast<const unsigned*>(rp + xf);
            unsigned char* dst = &px[r][xf - xa];
            dst[0] = (unsigned char)v; dst[1] = (unsigned char)(v >> 8); dst[2] = (unsigned char)(v >> 16); dst[3] = (unsigned char)(v >> 24);
        } else {
            for (int b = 0; b < 4; ++b) {
                const int x = xf + b;
                if (x >= lo && x < hi) px[r][x - xa] = rp[x];
            }
        }
    }
    for (int idx = tid; idx < PH * PW; idx += 256) {
        const int r = idx / PW, c = idx - r * PW, x = xa + c;
        if (x >= 0 && x < W) continue;
        const int y = min(max(ya + r, 0), H - 1);
        px[r][c] = image[(size_t)y * stride + (x < 0 ? 0 : W - 1)];
    }
}

// The edge detector of one 64 x 16 tile (include/fdcm.h, "edges with smoothing, hysteresis and a minimum chain length"): S is the
// image smoothed S times (S = 0: the image), a candidate passes low2 and thinning, and its label is the bin of its tangent.
// Every pixel of the tile inside the image gets its label (255: no candidate); with HYST also its root word (the pixel's own
// strong flag, m2 >= high2, and count 0), so `roots` needs no clearing.  Without HYST low2 is the one threshold.
template <int S, bool HYST>
__device__ __forceinline__ void edge_tile(const uint8_t* __restrict__ image, int W, int H, int stride, const float* __restrict__ keys, int m,
                                          int low2, int high2, uint8_t* __restrict__ labels, uint32_t* __restrict__ roots) {
    constexpr int HALO = kEdgeHalo + S, RH = kEdgeTH + 2 * HALO, RW = kEdgeTW + 2 * HALO;
    __shared__ unsigned char raw[S ? RH : 1][S ? RW + 4 : 4];  // the image around the tile (smoothing only)
    __shared__ unsigned char px[kEdgePH][kEdgePW + 4];         // S on the tile and kEdgeHalo pixels around it
    __shared__ int sm2[kEdgeMH][kEdgeMW];
    __shared__ float skeys[256];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kEdgeTW, y0 = blockIdx.y * kEdgeTH;
    if (tid < m) skeys[tid] = keys[tid];
    if constexpr (S == 0) {
        load_clamped_tile<kEdgePH, kEdgePW>(px, image, W, H, stride, x0 - kEdgeHalo, y0 - kEdgeHalo, tid);
    } else {
        load_clamped_tile<RH, RW>(raw, image, W, H, stride, x0 - HALO, y0 - HALO, tid);
        __syncthreads();
        // S at the clamped coordinate of every held pixel: its taps are inside `raw` (the clamped coordinate is at most
        // kEdgeHalo outside the tile), and `raw` holds I clamped
        for (int idx = tid; idx < kEdgePH * kEdgePW; idx += 256) {
            const int r = idx / kEdgePW, c = idx - r * kEdgePW;
            const int cx = min(max(x0 - kEdgeHalo + c, 0), W - 1) - (x0 - HALO), cy = min(max(y0 - kEdgeHalo + r, 0), H - 1) - (y0 - HALO);
            int sum = 0;
#pragma unroll
            for (int j = -S; j <= S; ++j) {
                int row = 0;
#pragma unroll
                for (int i = -S; i <= S; ++i) {
                    const int w = S == 1 ? 2 - abs(i) : (i == 0 ? 6 : (abs(i) == 1 ? 4 : 1));
                    row += w * raw[cy + j][cx + i];
                }
                sum += (S == 1 ? 2 - abs(j) : (j == 0 ? 6 : (abs(j) == 1 ? 4 : 1))) * row;
            }
            px[r][c] = (unsigned char)(S == 1 ? (sum + 8) >> 4 : (sum + 128) >> 8);
        }
    }
    __syncthreads();
    // squared gradient magnitude of the tile and one pixel around it; 0 outside the image
    for (int idx = tid; idx < kEdgeMH * kEdgeMW; idx += 256) {
        const int rr = idx / kEdgeMW, cc = idx - rr * kEdgeMW;
        const int x = x0 - 1 + cc, y = y0 - 1 + rr;
        int v = 0;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            int gx, gy;
            sobel_at(px, rr + 1, cc + 1, gx, gy);
            v = gx * gx + gy * gy;  // <= 2 * 1020^2
        }
        sm2[rr][cc] = v;
    }
    __syncthreads();
    const int lx = tid & 63;
#pragma unroll
    for (int i = 0; i < kEdgeTH / 4; ++i) {
        const int ly = (tid >> 6) + 4 * i;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        int gx, gy;
        sobel_at(px, ly + kEdgeHalo, lx + kEdgeHalo, gx, gy);
        const int m2 = sm2[ly + 1][lx + 1];
        const int a = abs(gx), b = abs(gy);
        int dx, dy;  // the step along the gradient, quantised to 8 neighbours (12 / 29 ~ tan 22.5 deg)
        if (29 * b < 12 * a) { dx = 1; dy = 0; }
        else if (29 * a < 12 * b) { dx = 0; dy = 1; }
        else { dx = 1; dy = ((gx >= 0) == (gy >= 0)) ? 1 : -1; }
        const int before = sm2[ly + 1 - dy][lx + 1 - dx], after = sm2[ly + 1 + dy][lx + 1 + dx];
        const bool cand = m2 >= low2 && m2 > before && m2 >= after;
        unsigned char label = 255;
        if (cand) {
            // the edge's tangent (-gy, gx) as getAngle sees a line from the origin to it (math.h:295-299); the integer is negated, so gy = 0 gives +0
            const float tdx = (float)(-gy), tdy = (float)gx;
            label = (unsigned char)closest_orientation(skeys, m, atanf_glibc(tdy / tdx));
        }
        const int p = y * W + x;  // < 2^24
        labels[p] = label;
        if constexpr (HYST) roots[p] = cand && m2 >= high2 ? kStrongBit : 0u;
    }
}

__global__ void __launch_bounds__(256) k_edge_labels(const uint8_t* __restrict__ image, int W, int H, int stride, const float* __restrict__ keys,
                                                     int m, int thr2, uint8_t* __restrict__ labels) {
    edge_tile<0, false>(image, W, H, stride, keys, m, thr2, 0, labels, nullptr);
}
template <int S>
__global__ void __launch_bounds__(256) k_edge_candidates(const uint8_t* __restrict__ image, int W, int H, int stride, const float* __restrict__ keys,
                                                         int m, int low2, int high2, uint8_t* __restrict__ labels, uint32_t* __restrict__ roots) {
    edge_tile<S, true>(image, W, H, stride, keys, m, low2, high2, labels, roots);
}

// The candidates' 8-connected components: the shared labeller with one partition, whose key says "a candidate".  k_edge_tiles
// writes a parent for every pixel of the image (kNoParent off the candidates), as k_line_tiles does, so `parent` needs no
// clearing and holds nothing of an earlier call when the kernels below read it.
struct EdgeKeys {
    static constexpr int P = 1;
    __device__ __forceinline__ int key(int, int label) const { return label < 255 ? 0 : kNoKey; }
};
__global__ void __launch_bounds__(256) k_edge_tiles(const uint8_t* __restrict__ labels, int W, int H, int32_t* __restrict__ parent) {
    uf_tile_merge(EdgeKeys{}, labels, W, H, parent);
}
__global__ void __launch_bounds__(kBorderThreads) k_edge_borders(const uint8_t* __restrict__ labels, int W, int H, int32_t* parent) {
    uf_border_merge(EdgeKeys{}, labels, W, H, parent);
}
// flatten, and per root the candidates' count and strong flag.  Bit 31 of roots[p] is p's own flag until this kernel adds to a
// root's word; a root that reads its component's flag for its own ORs it into itself.
__global__ void __launch_bounds__(256) k_edge_roots(int n, int32_t* parent, uint32_t* roots) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n || uf_load(parent, p) == kNoParent) return;
    const int r = uf_find(parent, p);
    if (r != p) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned own = __hip_atomic_load(roots + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kStrongBit;
    atomicAdd(&roots[r], 1u);
    if (own) atomicOr(&roots[r], kStrongBit);
}
// the candidates of a component without a strong pixel or with fewer than min_pixels: no edge
__global__ void __launch_bounds__(256) k_edge_resolve(int n, const int32_t* __restrict__ parent, const uint32_t* __restrict__ roots, int min_pixels,
                                                      uint8_t* __restrict__ labels) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int r = parent[p];
    if (r == kNoParent) return;
    const unsigned w = roots[r];
    if (!(w & kStrongBit) || (int)(w & ~kStrongBit) < min_pixels) labels[p] = 255;
}

void launch_edge_labels(hipStream_t st, const uint8_t* image, int width, int height, int row_stride, const float* keys, int m,
                        const fdcm_edge_params& e, uint8_t* labels, int32_t* parent, uint32_t* roots) {
    const dim3 grid = uf_tile_grid(width, height);
    const int low2 = e.low * e.low, high2 = e.high * e.high, n = width * height;
    if (!parent) {
        hipLaunchKernelGGL(k_edge_labels, grid, dim3(256), 0, st, image, width, height, row_stride, keys, m, high2, labels);
        return;
    }
    switch (e.smooth) {
    case 0: hipLaunchKernelGGL(k_edge_candidates<0>, grid, dim3(256), 0, st, image, width, height, row_stride, keys, m, low2, high2, labels, roots); break;
    case 1: hipLaunchKernelGGL(k_edge_candidates<1>, grid, dim3(256), 0, st, image, width, height, row_stride, keys, m, low2, high2, labels, roots); break;
    default: hipLaunchKernelGGL(k_edge_candidates<2>, grid, dim3(256), 0, st, image, width, height, row_stride, keys, m, low2, high2, labels, roots); break;
    }
    // launch counts and grids depend on the size alone: the components are resolved without a look at them from the host
    const dim3 flat((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(k_edge_tiles, grid, dim3(256), 0, st, (const uint8_t*)labels, width, height, parent);
    hipLaunchKernelGGL(k_edge_borders, grid, dim3(kBorderThreads), 0, st, (const uint8_t*)labels, width, height, parent);
    hipLaunchKernelGGL(k_edge_roots, flat, dim3(256), 0, st, n, parent, roots);
    hipLaunchKernelGGL(k_edge_resolve, flat, dim3(256), 0, st, n, (const int32_t*)parent, (const uint32_t*)roots, e.min_pixels, labels);
}

// ------------------------------------------------------------------------------------------ labels -> column descriptors
// k_coldesc_tile (fdcm_build.hip) with another seed source: bit (y + border) of column (x + border) of slice k is set when
// labels[y][x] == k.  A thread builds whole words (64 rows of one column; neighbouring threads take neighbouring columns, so a
// wave reads 64 contiguous label bytes per row), so the tile needs no clearing and no atomics.
// cost (or null): per (slice, 64-row chunk) the proxy of the L2 sweep's time that sweep_cost_proxy makes of line boxes, counted
// here: twice the slice's seeded columns less those with a seed inside the chunk, summed over the slice's blocks.
template <int SEG, int XT>
__global__ void __launch_bounds__(256) k_coldesc_labels(const uint8_t* __restrict__ labels, int lw, int lh, int border, ColDesc* __restrict__ desc,
                                                        int W, int H, int HW64, unsigned* __restrict__ colmask, int* __restrict__ cost) {
    extern __shared__ uint4 tile[];  // as k_coldesc_tile's
    constexpr int STR = XT + 1;
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(tile + (size_t)HW64 * STR);
    const long k = blockIdx.y;
    const int x0 = blockIdx.x * XT;
    for (int idx = threadIdx.x; idx < HW64 * XT; idx += 256) {
        const int w = idx / XT, xl = idx - w * XT;
        const int x = x0 + xl - border;  // the label image's column
        unsigned long long word = 0ull;
        if (x >= 0 && x < lw) {
            const int r0 = w * 64 - border;  // the label image's row of the word's bit 0
            const int ya = max(r0, 0), yb = min(r0 + 64, lh);
            for (int y = ya; y < yb; ++y)
                if (labels[(size_t)y * lw + x] == (uint8_t)k) word |= 1ull << (y - r0);
        }
        bits[idx] = word;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    coldesc_from_bits<SEG, XT>(tile, bits, desc, W, HW64, colmask, k, x0, lane, wave);
    if (cost) {  // (the descriptors are still in `tile`: nothing writes it after coldesc_from_bits' barrier)
        const bool col = lane < XT && x0 + lane < W;
        const int seeded = __popcll(__ballot(col && !desc_seedless(tile[min(lane, XT - 1)])));
        for (int w = wave; w < HW64; w += 4) {
            const uint4 d = tile[w * STR + min(lane, XT - 1)];
            const int inside = __popcll(__ballot(col && (d.x | d.y) != 0u));
            if (lane == 0 && seeded > 0) atomicAdd(&cost[k * HW64 + w], 2 * seeded - inside);
        }
    }
}

void launch_coldesc_labels(hipStream_t st, const uint8_t* labels, int width, int height, int border, void* desc, int W, int H,
                           int HW64, int m, unsigned* colmask, int* cost) {
    const int XT = HW64 > 32 ? 32 : 64;
    const dim3 grid((unsigned)((W + XT - 1) / XT), (unsigned)m);
    const size_t lds = (size_t)HW64 * (XT + 1) * sizeof(uint4) + (size_t)HW64 * XT * 8;
    ColDesc* d = (ColDesc*)desc;
    if (HW64 <= 16) hipLaunchKernelGGL((k_coldesc_labels<16, 64>), grid, dim3(256), lds, st, labels, width, height, border, d, W, H, HW64, colmask, cost);
    else if (HW64 <= 32) hipLaunchKernelGGL((k_coldesc_labels<32, 64>), grid, dim3(256), lds, st, labels, width, height, border, d, W, H, HW64, colmask, cost);
    else hipLaunchKernelGGL((k_coldesc_labels<64, 32>), grid, dim3(256), lds, st, labels, width, height, border, d, W, H, HW64, colmask, cost);
}

// ------------------------------------------------------------------------------------------ image -> the next level's image
// P_(l+1)(x, y) = S2(P_l)(2x, 2y) (include/fdcm.h, "image pyramid"): the smooth = 2 image of edge_tile<2, ..>, sampled at the even
// coordinates.  A workgroup makes one kTileW x kTileH tile of P_(l+1) from the (2 kTileW + 3) x (2 kTileH + 3) pixels of P_l
// around it, which load_clamped_tile holds with the replicate border; a thread makes four pixels, a wave 64 neighbours of a row.
static constexpr int kPyrPW = 2 * kTileW + 3, kPyrPH = 2 * kTileH + 3;
__global__ void __launch_bounds__(256) k_pyr_down(const uint8_t* __restrict__ src, int W, int H, int stride, uint8_t* __restrict__ dst, int Wn,
                                                  int Hn) {
    __shared__ unsigned char raw[kPyrPH][kPyrPW + 5];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;  // 2 x0 <= W - 1 and 2 y0 <= H - 1: the held region meets the image
    load_clamped_tile<kPyrPH, kPyrPW>(raw, src, W, H, stride, 2 * x0 - 2, 2 * y0 - 2, tid);
    __syncthreads();
    const int lx = tid & 63;
#pragma unroll
    for (int i = 0; i < kTileH / 4; ++i) {
        const int ly = (tid >> 6) + 4 * i;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= Wn || y >= Hn) continue;
        int sum = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            int row = 0;
#pragma unroll
            for (int t = 0; t < 5; ++t) row += (t == 2 ? 6 : (t == 1 || t == 3 ? 4 : 1)) * raw[2 * ly + j][2 * lx + t];
            sum += (j == 2 ? 6 : (j == 1 || j == 3 ? 4 : 1)) * row;
        }
        dst[(size_t)y * Wn + x] = (unsigned char)((sum + 128) >> 8);
    }
}

void pyramid_size(int64_t width, int64_t height, int level, int64_t* w_out, int64_t* h_out) {
    for (int l = 0; l < level; ++l) { width = (width + 1) >> 1; height = (height + 1) >> 1; }
    *w_out = width; *h_out = height;
}

// level 0 of the call without a handle: the image's rows, packed (the caller's device memory is read and written by kernels only)
__global__ void __launch_bounds__(256) k_pack_rows(const uint8_t* __restrict__ src, int W, int H, int stride, uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x < W && y < H) dst[(size_t)y * W + x] = src[(size_t)y * stride + x];
}

const uint8_t* launch_pyramid(hipStream_t st, const uint8_t* image, int width, int height, int row_stride, int level, uint8_t* a, uint8_t* b,
                              uint8_t* last) {
    const uint8_t* src = image;
    for (int l = 0; l < level; ++l) {
        const int wn = (width + 1) >> 1, hn = (height + 1) >> 1;
        uint8_t* dst = (last && l == level - 1) ? last : ((l & 1) ? b : a);
        hipLaunchKernelGGL(k_pyr_down, uf_tile_grid(wn, hn), dim3(256), 0, st, src, width, height, row_stride, dst, wn, hn);
        src = dst; width = wn; height = hn; row_stride = wn;
    }
    return src;
}

// ------------------------------------------------------------------------------------------ the calls without a handle
PixelScratch::~PixelScratch() { for (DevBuf* b : {&pixels, &labels, &keys, &parent, &counts, &comps, &out}) b->release(); }

void PixelScratch::take(DevBuf& b, size_t bytes, int id) {
    const void* before = b.p;
    b.reserve(bytes);
    if (b.p != before) poison_fill(b, nullptr, id);
}

const uint8_t* PixelScratch::upload(const uint8_t* host_or_device, int width, int height, int& row_stride, bool on_device,
                                    const std::vector<float>* host_keys) {
    if (host_keys) {
        take(keys, std::max<size_t>(1, host_keys->size()) * sizeof(float), FDCM_FILL_PIXEL_KEYS);
        FDCM_HIP(hipMemcpy(keys.p, host_keys->data(), host_keys->size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (on_device) return host_or_device;
    take(pixels, (size_t)width * height, FDCM_FILL_PIXEL_PIXELS);
    FDCM_HIP(hipMemcpy2D(pixels.p, (size_t)width, host_or_device, (size_t)row_stride, (size_t)width, (size_t)height, hipMemcpyHostToDevice));
    row_stride = width;
    return pixels.as<uint8_t>();
}

void image_pyramid_host(int device, const uint8_t* image, int width, int height, int row_stride, bool on_device, int level, uint8_t* out,
                        bool out_on_device) {
    FDCM_HIP(hipSetDevice(device));
    PixelScratch s;
    int64_t w1, h1, w2, h2, wl, hl;
    pyramid_size(width, height, 1, &w1, &h1);
    pyramid_size(w1, h1, 1, &w2, &h2);
    pyramid_size(width, height, level, &wl, &hl);
    const size_t n = (size_t)(wl * hl);
    const uint8_t* d = s.upload(image, width, height, row_stride, on_device, nullptr);
    const size_t off_b = ((size_t)(w1 * h1) + 15) & ~(size_t)15;
    if (level > 1) s.take(s.labels, off_b + (size_t)(w2 * h2), FDCM_FILL_PIXEL_LABELS);  // (the two buffers of the levels between)
    if (!out_on_device) s.take(s.out, n, FDCM_FILL_PIXEL_OUT);
    uint8_t* dst = out_on_device ? out : s.out.as<uint8_t>();  // the last level goes where it is wanted: device memory of the caller's is written by a kernel
    if (level == 0)
        hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)((width + 255) / 256), (unsigned)height), dim3(256), 0, nullptr, d, width, height, row_stride, dst);
    else
        launch_pyramid(nullptr, d, width, height, row_stride, level, s.labels.as<uint8_t>(), s.labels.as<uint8_t>() + off_b, dst);
    FDCM_HIP(hipGetLastError());
    FDCM_HIP(hipDeviceSynchronize());
    if (!out_on_device) FDCM_HIP(hipMemcpy(out, s.out.p, n, hipMemcpyDeviceToHost));
}

void edge_labels_host(int device, const uint8_t* image, int width, int height, int row_stride, int64_t depth, const fdcm_edge_params& e,
                      bool hysteresis, uint8_t* labels_out) {
    std::vector<float> keys;
    plan_keys(depth, keys);
    FDCM_HIP(hipSetDevice(device));
    PixelScratch s;
    const size_t n = (size_t)width * height;
    const uint8_t* d = s.upload(image, width, height, row_stride, false, &keys);
    s.take(s.labels, n, FDCM_FILL_PIXEL_LABELS);
    if (hysteresis) s.take(s.comps, n * 8, FDCM_FILL_PIXEL_COMPS);  // a parent and a root word per pixel
    launch_edge_labels(nullptr, d, width, height, row_stride, s.keys.as<float>(), (int)keys.size(), e, s.labels.as<uint8_t>(),
                       hysteresis ? s.comps.as<int32_t>() : nullptr, hysteresis ? s.comps.as<uint32_t>() + n : nullptr);
    FDCM_HIP(hipGetLastError());
    FDCM_HIP(hipDeviceSynchronize());
    FDCM_HIP(hipMemcpy(labels_out, s.labels.p, n, hipMemcpyDeviceToHost));
}

}  // namespace fdcm
