// fdcm_image.hip -- DT3 seeds from pixels on gfx950: oriented edge pixels of a grey image as a label image, and pass 1 of the
// distance transform with its seeds taken from a label image (include/fdcm.h, "feature maps from images").
//
//   k_edge_labels      uint8 image -> label image: integer Sobel, thresholded and thinned along the gradient, the edge's tangent
//                      binned by closest_orientation over the build's keys               read W H, write W H
//   k_coldesc_labels   k_coldesc_tile's sibling: the bitmap tile in LDS comes from the label image instead of RasterLines, the
//                      descriptor step (coldesc_from_bits) is shared                     read m W H (from L2), write ~V/16
// Both index with the caller's sizes only: every load is of a pixel inside [0, width) x [0, height), every store inside the label
// image or the descriptors of the block's own columns.
#include <algorithm>

#include "fdcm_build_dev.h"
#include "fdcm_internal.h"

namespace fdcm {

// ------------------------------------------------------------------------------------------ image -> labels
static constexpr int kEdgeTW = 64, kEdgeTH = 16;  // pixels a workgroup labels
static constexpr int kEdgeHalo = 2;               // 1 for Sobel + 1 for the neighbours' m2
static constexpr int kEdgePW = kEdgeTW + 2 * kEdgeHalo, kEdgePH = kEdgeTH + 2 * kEdgeHalo;  // pixels held
static constexpr int kEdgeMW = kEdgeTW + 2, kEdgeMH = kEdgeTH + 2;                          // squared magnitudes held
static constexpr int kEdgeRowDwords = (kEdgePW + 3 + 3) / 4;  // aligned dwords that cover a row of held pixels wherever it starts

// Sobel at tile position (r, c) of the held pixels (replicate border: the loads clamped the coordinates)
__device__ __forceinline__ void sobel_at(const unsigned char (*px)[kEdgePW + 4], int r, int c, int& gx, int& gy) {
    const int a = px[r - 1][c - 1], b = px[r - 1][c], d = px[r - 1][c + 1];
    const int e = px[r][c - 1], f = px[r][c + 1];
    const int g = px[r + 1][c - 1], h = px[r + 1][c], i = px[r + 1][c + 1];
    gx = (d + 2 * f + i) - (a + 2 * e + g);
    gy = (g + 2 * h + i) - (a + 2 * b + d);
}

__global__ void __launch_bounds__(256) k_edge_labels(const uint8_t* __restrict__ image, int W, int H, int stride, const float* __restrict__ keys,
                                                     int m, int thr2, uint8_t* __restrict__ labels) {
    __shared__ unsigned char px[kEdgePH][kEdgePW + 4];
    __shared__ int sm2[kEdgeMH][kEdgeMW];
    __shared__ float skeys[256];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kEdgeTW, y0 = blockIdx.y * kEdgeTH;
    const int xa = x0 - kEdgeHalo;                           // image column of held column 0
    const int lo = max(xa, 0), hi = min(xa + kEdgePW, W);    // the held columns inside the image: [lo, hi), never empty (x0 < W)
    if (tid < m) skeys[tid] = keys[tid];
    // the pixels inside the image: aligned dwords where all four bytes are the row's, single bytes at the ragged ends
    for (int idx = tid; idx < kEdgePH * kEdgeRowDwords; idx += 256) {
        const int r = idx / kEdgeRowDwords, j = idx - r * kEdgeRowDwords;
        const int y = min(max(y0 - kEdgeHalo + r, 0), H - 1);
        const uint8_t* rp = image + (size_t)y * stride;
        const int mis = (int)((uintptr_t)(rp + lo) & 3u);    // bytes between the aligned address below the first pixel and it
        const int xf = lo - mis + 4 * j;                     // column of the dword's first byte
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
    // the held columns outside it: the row's first / last pixel (replicate border)
    for (int idx = tid; idx < kEdgePH * kEdgePW; idx += 256) {
        const int r = idx / kEdgePW, c = idx - r * kEdgePW, x = xa + c;
        if (x >= 0 && x < W) continue;
        const int y = min(max(y0 - kEdgeHalo + r, 0), H - 1);
        px[r][c] = image[(size_t)y * stride + (x < 0 ? 0 : W - 1)];
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
        unsigned char label = 255;
        if (m2 >= thr2 && m2 > before && m2 >= after) {
            // the edge's tangent (-gy, gx) as getAngle sees a line from the origin to it (math.h:295-299); the integer is negated, so gy = 0 gives +0
            const float tdx = (float)(-gy), tdy = (float)gx;
            label = (unsigned char)closest_orientation(skeys, m, atanf_glibc(tdy / tdx));
        }
        labels[(size_t)y * W + x] = label;
    }
}

void launch_edge_labels(hipStream_t st, const uint8_t* image, int width, int height, int row_stride, const float* keys, int m,
                        int threshold, uint8_t* labels) {
    const dim3 grid((unsigned)((width + kEdgeTW - 1) / kEdgeTW), (unsigned)((height + kEdgeTH - 1) / kEdgeTH));
    hipLaunchKernelGGL(k_edge_labels, grid, dim3(256), 0, st, image, width, height, row_stride, keys, m, threshold * threshold, labels);
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

// ------------------------------------------------------------------------------------------ fdcm_edge_labels
void edge_labels_host(int device, const uint8_t* image, int width, int height, int row_stride, int64_t depth, int threshold,
                      uint8_t* labels_out) {
    std::vector<float> keys;
    plan_keys(depth, keys);
    FDCM_HIP(hipSetDevice(device));
    struct Scratch { DevBuf image, labels, keys; ~Scratch() { image.release(); labels.release(); keys.release(); } } s;
    const size_t n = (size_t)width * height;
    s.image.reserve(n); s.labels.reserve(n); s.keys.reserve(std::max<size_t>(1, keys.size()) * sizeof(float));
    FDCM_HIP(hipMemcpy2D(s.image.p, (size_t)width, image, (size_t)row_stride, (size_t)width, (size_t)height, hipMemcpyHostToDevice));
    FDCM_HIP(hipMemcpy(s.keys.p, keys.data(), keys.size() * sizeof(float), hipMemcpyHostToDevice));
    launch_edge_labels(nullptr, s.image.as<uint8_t>(), width, height, width, s.keys.as<float>(), (int)keys.size(), threshold, s.labels.as<uint8_t>());
    FDCM_HIP(hipGetLastError());
    FDCM_HIP(hipDeviceSynchronize());
    FDCM_HIP(hipMemcpy(labels_out, s.labels.p, n, hipMemcpyDeviceToHost));
}

}  // namespace fdcm
