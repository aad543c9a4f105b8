// fdcm_lines.hip -- line segments from a label image on gfx950 (include/fdcm.h, "line segments from images"): the 8-connected
// components of equal orientation bucket in two overlapping partitions of the labels, a vote per pixel for the partition in
// which its component is larger, and an exact least-squares segment per component that keeps a strict majority.
//
//   k_line_tiles     labels -> both buckets per pixel; union-find of a 64 x 16 tile in LDS, both partitions; per pixel the
//                    tile-local root as a global index (kNoParent off the edges)                     read W H, write 8 W H
//   k_line_borders   the 8-neighbour pairs that straddle two tiles, merged in global memory (uf_union)
//                    (both are the tiled labeller of fdcm_unionfind.h with LineKeys: two partitions, the key a bucket)
//   k_line_roots     flatten, and the roots of every 1024 pixels counted
//   k_line_scan      exclusive scan of block counts in place, the total behind them (one workgroup; used twice)
//   k_line_number    a root's parent becomes -(id + 2): ids ascend with 2 * root + partition
//   k_line_sums      per edge pixel and partition: count, box and the five sums of its component, integer atomics
//   k_line_votes     per edge pixel: one vote for the partition whose component holds more pixels (A on a tie)
//   k_line_keep      per component: the three rules; kept ones counted per 256 components
//   k_line_fit       per kept component: the segment, written at its rank among the kept (ascending id)
// Every index is a pixel below width * height or a component below the count the host read back: k_line_tiles writes a parent
// for every pixel of the image, so nothing here reads a word that this call has not written.
#include <algorithm>

#include "fdcm_internal.h"
#include "fdcm_unionfind.h"

namespace fdcm {

static constexpr int kLineBlock = 1024;     // pixels per workgroup of the flat kernels that scan (4 per thread)

// The two partitions of the labels: partition A cuts the m orientations into buckets of w from 0 on, partition B from w / 2 on
// (cyclic).  A label < m <= 255 has a bucket <= 254 in both; any other byte is no edge pixel.
struct LineKeys {
    static constexpr int P = 2;
    int m, w;
    __device__ __forceinline__ int key(int part, int l) const {
        const int s = l + w / 2;  // < 2 m for an edge pixel
        const int k = (part == 0 ? l : (s >= m ? s - m : s)) / w;  // (divided whatever l is: every call shares one reciprocal of w)
        return l < m ? k : kNoKey;
    }
};
__global__ void __launch_bounds__(256) k_line_tiles(const uint8_t* __restrict__ labels, int W, int H, LineKeys keys, int32_t* __restrict__ parent) {
    uf_tile_merge(keys, labels, W, H, parent);
}
__global__ void __launch_bounds__(kBorderThreads) k_line_borders(const uint8_t* __restrict__ labels, int W, int H, LineKeys keys, int32_t* parent) {
    uf_border_merge(keys, labels, W, H, parent);
}

// ------------------------------------------------------------------------------------------ numbering
// exclusive prefix of v over the 256 threads of a workgroup and their total (`sw`: 4 words of LDS; a barrier inside, one before
// the next use of `sw` is the caller's)
__device__ __forceinline__ int block_scan_excl(int v, int tid, int* sw, int& total) {
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

// flatten, and the roots among the workgroup's 1024 pixels (both partitions) into counts[block]
__global__ void __launch_bounds__(256) k_line_roots(int n, int32_t* parent_a, int32_t* parent_b, int* __restrict__ counts) {
    __shared__ int sw[4];
    const int tid = threadIdx.x;
    const int p0 = (blockIdx.x * 256 + tid) * 4;
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + j;
        if (p >= n || uf_load(parent_a, p) == kNoParent) continue;
        const int ra = uf_find(parent_a, p), rb = uf_find(parent_b, p);
        if (ra != p) __hip_atomic_store(parent_a + p, ra, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else ++c;
        if (rb != p) __hip_atomic_store(parent_b + p, rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else ++c;
    }
    int total;
    block_scan_excl(c, tid, sw, total);
    if (tid == 0) counts[blockIdx.x] = total;
}

// counts[0 .. nb) -> their exclusive prefix sums in place, counts[nb] = the total
__global__ void __launch_bounds__(256) k_line_scan(int* counts, int nb) {
    __shared__ int sw[4];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < nb; base += 256) {
        const int i = base + tid;
        const int v = i < nb ? counts[i] : 0;
        int total;
        const int e = block_scan_excl(v, tid, sw, total);
        if (i < nb) counts[i] = carry + e;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) counts[nb] = carry;
}

// roots in ascending 2 * p + partition get ascending ids; a root's own parent word carries -(id + 2) from here on
__global__ void __launch_bounds__(256) k_line_number(int n, int32_t* parent_a, int32_t* parent_b, const int* __restrict__ offsets) {
    __shared__ int sw[4];
    const int tid = threadIdx.x;
    const int p0 = (blockIdx.x * 256 + tid) * 4;
    bool root_a[4], root_b[4];
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + j;
        root_a[j] = p < n && parent_a[p] == p;
        root_b[j] = p < n && parent_b[p] == p;
        c += (int)root_a[j] + (int)root_b[j];
    }
    int total;
    int id = offsets[blockIdx.x] + block_scan_excl(c, tid, sw, total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (root_a[j]) parent_a[p0 + j] = -(id++ + 2);
        if (root_b[j]) parent_b[p0 + j] = -(id++ + 2);
    }
}
// the component of pixel p, whose parent word is q: p is a root itself, or q is its root
__device__ __forceinline__ int component_of(const int32_t* __restrict__ parent, int q) { return q <= -2 ? -q - 2 : -parent[q] - 2; }

// ------------------------------------------------------------------------------------------ per component
// Arrays of `nc` entries each, in one buffer: the 64-bit sums first, then the words.  Zeroed by the host but for x0 and y0,
// which start at all ones.
struct LineComps {
    unsigned long long *sxx, *syy, *sxy;
    unsigned *n, *votes, *sx, *sy, *x1, *y1, *x0, *y0;
    int* keep;  // k_line_keep: 1 kept, 0 not
    static constexpr size_t kBytes = 3 * 8 + 9 * 4;  // per component
    static size_t bytes(size_t nc) { return nc * kBytes; }
    static LineComps at(void* base, size_t nc) {
        LineComps c;
        c.sxx = (unsigned long long*)base; c.syy = c.sxx + nc; c.sxy = c.syy + nc;
        c.n = (unsigned*)(c.sxy + nc); c.votes = c.n + nc; c.sx = c.votes + nc; c.sy = c.sx + nc;
        c.x1 = c.sy + nc; c.y1 = c.x1 + nc; c.x0 = c.y1 + nc; c.y0 = c.x0 + nc;
        c.keep = (int*)(c.y0 + nc);
        return c;
    }
};

__device__ __forceinline__ void add_pixel(const LineComps& c, int id, unsigned x, unsigned y) {
    atomicAdd(&c.n[id], 1u);
    atomicAdd(&c.sx[id], x); atomicAdd(&c.sy[id], y);  // exact while n <= 65535: below 2^28
    atomicAdd(&c.sxx[id], (unsigned long long)(x * x)); atomicAdd(&c.syy[id], (unsigned long long)(y * y));
    atomicAdd(&c.sxy[id], (unsigned long long)(x * y));
    atomicMin(&c.x0[id], x); atomicMax(&c.x1[id], x);
    atomicMin(&c.y0[id], y); atomicMax(&c.y1[id], y);
}
__global__ void __launch_bounds__(256) k_line_sums(int W, int n, const int32_t* __restrict__ parent_a, const int32_t* __restrict__ parent_b, LineComps c) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int qa = parent_a[p];
    if (qa == kNoParent) return;
    const int y = p / W, x = p - y * W;
    add_pixel(c, component_of(parent_a, qa), (unsigned)x, (unsigned)y);
    add_pixel(c, component_of(parent_b, parent_b[p]), (unsigned)x, (unsigned)y);
}
__global__ void __launch_bounds__(256) k_line_votes(int n, const int32_t* __restrict__ parent_a, const int32_t* __restrict__ parent_b, LineComps c) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int qa = parent_a[p];
    if (qa == kNoParent) return;
    const int ia = component_of(parent_a, qa), ib = component_of(parent_b, parent_b[p]);
    atomicAdd(&c.votes[c.n[ia] >= c.n[ib] ? ia : ib], 1u);
}

// The exact part of the fit: the major axis and the extent along it.
struct LineMoments { long long n, sx, sy, dmaj, dxy; bool xmajor; int lo, hi; };
__device__ __forceinline__ LineMoments line_moments(const LineComps& c, int id) {
    LineMoments r;
    r.n = c.n[id]; r.sx = c.sx[id]; r.sy = c.sy[id];
    const long long dxx = r.n * (long long)c.sxx[id] - r.sx * r.sx, dyy = r.n * (long long)c.syy[id] - r.sy * r.sy;
    r.dxy = r.n * (long long)c.sxy[id] - r.sx * r.sy;
    r.xmajor = dxx >= dyy;
    r.dmaj = r.xmajor ? dxx : dyy;
    r.lo = (int)(r.xmajor ? c.x0[id] : c.y0[id]);
    r.hi = (int)(r.xmajor ? c.x1[id] : c.y1[id]);
    return r;
}
__global__ void __launch_bounds__(256) k_line_keep(int nc, LineComps c, int min_pixels, int min_length, int* __restrict__ counts) {
    __shared__ int sw[4];
    const int id = blockIdx.x * 256 + threadIdx.x;
    int keep = 0;
    if (id < nc) {
        const unsigned n = c.n[id];
        if (2u * c.votes[id] > n && n >= (unsigned)min_pixels && n <= 65535u) {  // (votes <= n <= 65535 here: no wrap)
            const LineMoments mo = line_moments(c, id);
            keep = mo.hi - mo.lo + 1 >= min_length;
        }
        c.keep[id] = keep;
    }
    int total;
    block_scan_excl(keep, threadIdx.x, sw, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}
// every operation one IEEE float64 operation in the definition's order (the library is built with -ffp-contract=off)
__global__ void __launch_bounds__(256) k_line_fit(int nc, LineComps c, const int* __restrict__ offsets, float4* __restrict__ out) {
    __shared__ int sw[4];
    const int id = blockIdx.x * 256 + threadIdx.x;
    const int keep = id < nc ? c.keep[id] : 0;
    int total;
    const int at = offsets[blockIdx.x] + block_scan_excl(keep, threadIdx.x, sw, total);
    if (!keep) return;
    const LineMoments mo = line_moments(c, id);
    const double s = (double)mo.dxy / (double)mo.dmaj;
    const double xb = (double)mo.sx / (double)mo.n, yb = (double)mo.sy / (double)mo.n;
    const double ub = mo.xmajor ? xb : yb, vb = mo.xmajor ? yb : xb;  // mean along the major axis, mean across it
    const double v0 = vb + s * ((double)mo.lo - ub), v1 = vb + s * ((double)mo.hi - ub);
    out[at] = mo.xmajor ? make_float4((float)mo.lo, (float)v0, (float)mo.hi, (float)v1)
                        : make_float4((float)v0, (float)mo.lo, (float)v1, (float)mo.hi);
}

// ------------------------------------------------------------------------------------------ host
namespace {
// The events of a call, for fdcm_lines_last_timing: one behind every stage, and one in front of the two stages that follow host
// work (a count read back, buffers sized by it), so that a stage's time is its kernels' alone.
enum Mark { kStart, kEdges, kTiles, kBorders, kNumber, kSumsBegin, kSums, kVotes, kKeep, kFitBegin, kFit, kMarks };
struct StageClock {
    hipEvent_t ev[kMarks] = {};
    bool set[kMarks] = {};
    ~StageClock() { for (int i = 0; i < kMarks; ++i) if (set[i]) (void)hipEventDestroy(ev[i]); }
    void mark(Mark i) { FDCM_HIP(hipEventCreate(&ev[i])); set[i] = true; FDCM_HIP(hipEventRecord(ev[i], nullptr)); }
    // milliseconds from a to b; 0 where the call never came to one of them
    float ms(Mark a, Mark b) const {
        float t = 0.f;
        return set[a] && set[b] && hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? t : 0.f;
    }
};
thread_local fdcm_lines_timing g_last_timing = {};

int read_int(const int* device_word) {
    int v = 0;
    FDCM_HIP(hipMemcpy(&v, device_word, sizeof(int), hipMemcpyDeviceToHost));  // (waits for the kernels before it)
    return v;
}

// labels (device, packed rows) -> segments on the host; marks are taken on the null stream, where everything runs
void lines_of_device_labels(PixelScratch& s, StageClock& clk, const uint8_t* labels, int W, int H, int m, const fdcm_line_params& lp,
                            float** lines, int64_t* n_lines) {
    *lines = nullptr; *n_lines = 0;
    const int n = W * H, nb = (n + kLineBlock - 1) / kLineBlock;
    s.take(s.parent, (size_t)n * 8, FDCM_FILL_PIXEL_PARENT);
    int32_t* pa = s.parent.as<int32_t>();
    int32_t* pb = pa + n;
    // block counts of the pixels' scan and of the components' (at most 2 n components, 256 per block), a total behind each
    s.take(s.counts, ((size_t)nb + 1 + (2 * (size_t)n + 255) / 256 + 1) * sizeof(int), FDCM_FILL_PIXEL_COUNTS);
    int* counts = s.counts.as<int>();
    const dim3 tiles = uf_tile_grid(W, H);
    const LineKeys keys{m, lp.bucket};
    hipLaunchKernelGGL(k_line_tiles, tiles, dim3(256), 0, nullptr, labels, W, H, keys, pa);
    clk.mark(kTiles);
    hipLaunchKernelGGL(k_line_borders, tiles, dim3(kBorderThreads), 0, nullptr, labels, W, H, keys, pa);
    clk.mark(kBorders);
    hipLaunchKernelGGL(k_line_roots, dim3((unsigned)nb), dim3(256), 0, nullptr, n, pa, pb, counts);
    hipLaunchKernelGGL(k_line_scan, dim3(1), dim3(256), 0, nullptr, counts, nb);
    hipLaunchKernelGGL(k_line_number, dim3((unsigned)nb), dim3(256), 0, nullptr, n, pa, pb, (const int*)counts);
    clk.mark(kNumber);
    FDCM_HIP(hipGetLastError());
    const int nc = read_int(counts + nb);
    if (nc == 0) return;
    s.take(s.comps, LineComps::bytes((size_t)nc), FDCM_FILL_PIXEL_COMPS);  // (lines_from_image_host: the edge kernels' words unless it has to grow)
    const LineComps c = LineComps::at(s.comps.p, (size_t)nc);
    FDCM_HIP(hipMemsetAsync(s.comps.p, 0, LineComps::bytes((size_t)nc), nullptr));
    FDCM_HIP(hipMemsetAsync(c.x0, 0xFF, (size_t)nc * 8, nullptr));  // x0 and y0
    clk.mark(kSumsBegin);
    const dim3 flat((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(k_line_sums, flat, dim3(256), 0, nullptr, W, n, (const int32_t*)pa, (const int32_t*)pb, c);
    clk.mark(kSums);
    hipLaunchKernelGGL(k_line_votes, flat, dim3(256), 0, nullptr, n, (const int32_t*)pa, (const int32_t*)pb, c);
    clk.mark(kVotes);
    const int cb = (nc + 255) / 256;
    int* ccounts = counts + nb + 1;
    hipLaunchKernelGGL(k_line_keep, dim3((unsigned)cb), dim3(256), 0, nullptr, nc, c, lp.min_pixels, lp.min_length, ccounts);
    hipLaunchKernelGGL(k_line_scan, dim3(1), dim3(256), 0, nullptr, ccounts, cb);
    clk.mark(kKeep);
    FDCM_HIP(hipGetLastError());
    const int kept = read_int(ccounts + cb);
    if (kept == 0) return;
    s.take(s.out, (size_t)kept * sizeof(float4), FDCM_FILL_PIXEL_OUT);
    clk.mark(kFitBegin);
    hipLaunchKernelGGL(k_line_fit, dim3((unsigned)cb), dim3(256), 0, nullptr, nc, c, (const int*)ccounts, s.out.as<float4>());
    clk.mark(kFit);
    FDCM_HIP(hipGetLastError());
    float* host = (float*)std::malloc((size_t)kept * sizeof(float4));
    if (!host) throw std::bad_alloc();
    const hipError_t e = hipMemcpy(host, s.out.p, (size_t)kept * sizeof(float4), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { std::free(host); throw HipError{e, "hipMemcpy(lines)", __LINE__}; }
    *lines = host; *n_lines = kept;
}

// Never throws: the segments are the caller's by now, and a timing that could not be read is zero.
void finish_timing(const StageClock& clk, bool edges, int64_t n_lines) noexcept {
    Mark last = kNumber;
    for (Mark i : {kVotes, kKeep, kFit}) if (clk.set[i]) last = i;
    fdcm_lines_timing t = {};
    if (clk.set[last] && hipEventSynchronize(clk.ev[last]) == hipSuccess) {
        t.edges_ms = edges ? clk.ms(kStart, kEdges) : 0.f;
        t.tiles_ms = clk.ms(kEdges, kTiles); t.borders_ms = clk.ms(kTiles, kBorders); t.number_ms = clk.ms(kBorders, kNumber);
        t.sums_ms = clk.ms(kSumsBegin, kSums); t.votes_ms = clk.ms(kSums, kVotes); t.keep_ms = clk.ms(kVotes, kKeep);
        t.fit_ms = clk.ms(kFitBegin, kFit);
        t.total_ms = clk.ms(edges ? kStart : kEdges, last);
    }
    t.n_lines = n_lines;
    g_last_timing = t;
}
}  // namespace

void lines_last_timing(fdcm_lines_timing* out) { *out = g_last_timing; }

void lines_from_labels_host(int device, const uint8_t* labels, int width, int height, bool on_device, int m, const fdcm_line_params& lp,
                            float** lines, int64_t* n_lines) {
    FDCM_HIP(hipSetDevice(device));
    PixelScratch s;
    StageClock clk;
    int stride = width;
    const uint8_t* d = s.upload(labels, width, height, stride, on_device, nullptr);
    clk.mark(kEdges);  // (no edge stage)
    lines_of_device_labels(s, clk, d, width, height, m, lp, lines, n_lines);
    finish_timing(clk, false, *n_lines);
}

void lines_from_image_host(int device, const uint8_t* image, int width, int height, int row_stride, bool on_device, int64_t depth,
                           const fdcm_edge_params& e, const fdcm_line_params& lp, float** lines, int64_t* n_lines) {
    std::vector<float> keys;
    plan_keys(depth, keys);
    FDCM_HIP(hipSetDevice(device));
    PixelScratch s;
    StageClock clk;
    const size_t n = (size_t)width * height;
    const uint8_t* d = s.upload(image, width, height, row_stride, on_device, &keys);
    s.take(s.labels, n, FDCM_FILL_PIXEL_LABELS);
    s.take(s.comps, n * 8, FDCM_FILL_PIXEL_COMPS);  // the edge kernels' parent and root words; the components' sums take their place afterwards
    clk.mark(kStart);
    launch_edge_labels(nullptr, d, width, height, row_stride, s.keys.as<float>(), (int)keys.size(), e, s.labels.as<uint8_t>(),
                       s.comps.as<int32_t>(), s.comps.as<uint32_t>() + n);
    clk.mark(kEdges);
    lines_of_device_labels(s, clk, s.labels.as<uint8_t>(), width, height, (int)keys.size(), lp, lines, n_lines);
    finish_timing(clk, true, *n_lines);
}

}  // namespace fdcm
