// fdcm_build_dev.h -- device helpers shared by the build kernels (fdcm_build.hip, fdcm_sweep.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "fdcm_internal.h"

namespace fdcm {

static constexpr int kWave = 64;

__device__ __forceinline__ int wave_scan_max_excl(int v, int lane) {  // exclusive prefix max
    int incl = v;
    for (int d = 1; d < kWave; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl = max(incl, o);
    }
    const int prev = __shfl_up(incl, 1);
    return lane == 0 ? INT_MIN : prev;
}
__device__ __forceinline__ int wave_scan_min_excl_rev(int v, int lane) {  // exclusive suffix min
    int incl = v;
    for (int d = 1; d < kWave; d <<= 1) {
        const int o = __shfl_down(incl, d);
        if (lane + d < kWave) incl = min(incl, o);
    }
    const int nxt = __shfl_down(incl, 1);
    return lane == kWave - 1 ? INT_MAX : nxt;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}

// Column-chunk descriptor: for column (k, x) and the 64 rows [64c, 64c+64): the seed bits of the
// chunk, the last seed row before it and the first seed row after it.  16 bytes per 64 pixels,
// stored [k][c][x] so that a wave sweeping along x prefetches 64 columns with one coalesced load.
static constexpr int kFar = 1 << 30;  // "no seed on that side": a row 2^30 away (rows are < 2^14)
struct __attribute__((aligned(16))) ColDesc {
    unsigned long long word;
    int prev;  // -kFar: none
    int next;  // +kFar: none
};
// a column without any seed in the slice (all its chunks say the same)
__device__ __forceinline__ bool desc_seedless(const uint4& d) {
    return (d.x | d.y) == 0u && (int)d.z == -kFar && (int)d.w == kFar;
}

// Pass 1 of distanceTransform (imgproc.h:178 / :186, along y) evaluated on the fly.  On a
// 0 / FLT_MAX image the lower-envelope pass yields exactly the squared distance to the nearest
// seed of the column (every envelope owner is a seed and owns itself), or FLT_MAX for a seedless
// column; the L1 sweeps yield the plain distance.  Both are integers < 2^24, so this bit-scan
// gives the reference's bits.  y = 64c + lane.
template <bool SQUARED>
__device__ __forceinline__ float column_value(unsigned long long wc, int pc, int nc, int lane, int y) {
    // branch-free: a missing neighbour chunk seed is a position 2^30 away (the descriptor says so), so "no seed
    // in the column" is d >= 2^29 (rows are < 2^14)
    const unsigned long long dnw = wc >> lane;         // bit 0 = own row, upwards = rows below it in the image
    const unsigned long long upw = wc << (63 - lane);  // bit 63 = own row
    const int d_dn = dnw ? __ffsll((long long)dnw) - 1 : nc - y;
    const int d_up = upw ? __clzll(upw) : y - pc;
    const int d = min(d_up, d_dn);
    const float df = (float)d;
    return d >= (1 << 29) ? FLT_MAX : (SQUARED ? df * df : df);  // d < 2^14: df * df is the exact integer
}

// The squared value for a SEEDED column whose descriptor fields are wave-uniform (read with v_readlane): most columns of
// a chunk have no seed inside the chunk's 64 rows (a line crosses a chunk in a few columns), and then the value is the
// distance to the neighbour seeds alone -- 5 vector instructions behind a scalar branch instead of ~22.  (A seeded
// column has a seed in some chunk, so a missing side is 2^30 away and the other one decides: never FLT_MAX here.)
__device__ __forceinline__ float column_value_sq_seeded(unsigned long long wc, int pc, int nc, int lane, int y) {
    if (wc == 0ull) {
        const int d = min(y - pc, nc - y);
        const float df = (float)d;
        return df * df;
    }
    return column_value<true>(wc, pc, nc, lane, y);
}

__device__ __forceinline__ void desc_lane(const ColDesc& d, int j, unsigned long long& wc, int& pc, int& nc) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(d.word & 0xffffffffull), j);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(d.word >> 32), j);
    wc = ((unsigned long long)hi << 32) | lo;
    pc = __builtin_amdgcn_readlane(d.prev, j);
    nc = __builtin_amdgcn_readlane(d.next, j);
}

// The descriptor step of pass 1 for H <= 4096 (k_coldesc_tile, k_coldesc_labels): a block of 256 threads holds the seed bits of
// XT neighbouring columns of slice k in LDS (bits[word][XT]); SEG lanes (16 / 32 / 64: the words of a column) scan one column
// each, 64 / SEG columns per wave pass, and the descriptors go through LDS (tile[word][XT + 1]) so that every store covers the
// block's columns of one chunk.  Behind a barrier that follows the last write of `bits`.
template <int SEG, int XT>
__device__ __forceinline__ void coldesc_from_bits(uint4* tile, unsigned long long* bits, ColDesc* desc, int W, int HW64,
                                                  unsigned* colmask, long k, int x0, int lane, int wave) {
    constexpr int STR = XT + 1;
    const int wi = lane & (SEG - 1), ci = lane / SEG;
    constexpr int CPP = 64 / SEG, CPW = XT / 4;  // columns per wave pass, columns per wave
    for (int pass = 0; pass < CPW / CPP; ++pass) {
        const int xl = wave * CPW + pass * CPP + ci, x = x0 + xl;
        const bool valid = x < W && wi < HW64;
        const unsigned long long word = valid ? bits[wi * XT + xl] : 0ull;
        const int last_i = word ? wi * 64 + 63 - __clzll(word) : INT_MIN;
        const int first_i = word ? wi * 64 + (__ffsll((long long)word) - 1) : INT_MAX;
        int pmax = last_i, smin = first_i;  // inclusive scans inside the SEG lanes of a column
#pragma unroll
        for (int d = 1; d < SEG; d <<= 1) {
            const int a = __shfl_up(pmax, d), b = __shfl_down(smin, d);
            if (wi >= d) pmax = max(pmax, a);
            if (wi + d < SEG) smin = min(smin, b);
        }
        const int pe = __shfl_up(pmax, 1), se = __shfl_down(smin, 1);
        const int pv = wi == 0 ? INT_MIN : pe, nx = wi == SEG - 1 ? INT_MAX : se;
        if (wi < HW64)
            tile[wi * STR + xl] = make_uint4((unsigned)(word & 0xffffffffull), (unsigned)(word >> 32),
                                             (unsigned)(pv == INT_MIN ? -kFar : pv), (unsigned)(nx == INT_MAX ? kFar : nx));
    }
    __syncthreads();
    uint4* out = reinterpret_cast<uint4*>(desc);
    for (int idx = threadIdx.x; idx < HW64 * XT; idx += 256) {
        const int w = idx / XT, xl = idx - w * XT;
        if (x0 + xl < W) out[((size_t)k * HW64 + w) * W + x0 + xl] = tile[w * STR + xl];
    }
    // The slice's seeded columns, one bit per column ((W + 63) / 64 words of 64 bits per slice, written as 32-bit halves):
    // the L2 sweep skips the others, and every one of its workgroups used to rebuild this mask from the descriptors.
    if (colmask && wave == 0) {
        const bool seeded = lane < XT && x0 + lane < W && !desc_seedless(tile[min(lane, XT - 1)]);  // chunk 0's descriptor says it for the column
        const unsigned long long mk = __ballot(seeded);
        unsigned* dst = colmask + ((size_t)k * ((W + 63) >> 6) + (x0 >> 6)) * 2;
        if (XT == 64) { if (lane < 2) dst[lane] = lane ? (unsigned)(mk >> 32) : (unsigned)mk; }
        else {
            const int half = (x0 >> 5) & 1;
            if (lane == 0) dst[half] = (unsigned)mk;
            if (lane == 1 && half == 0 && x0 + 32 >= W) dst[1] = 0u;  // no block for the word's upper half
        }
    }
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct EnvEntry { float v2; float P; float z; };     // one stack entry (imgproc.h: v[k], f[v[k]], z[k]) as the sweep's tests use it: 2 v, f[v] + v^2, z
struct OwnEntry { unsigned pk; float b; };          // (first pixel << 16 | column), addend

__device__ __forceinline__ unsigned long long uni64(unsigned long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ void desc_lane4(const uint4& d, int j, unsigned long long& wc, int& pc, int& nc) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)d.x, j);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)d.y, j);
    wc = ((unsigned long long)hi << 32) | lo;
    pc = __builtin_amdgcn_readlane((int)d.z, j);
    nc = __builtin_amdgcn_readlane((int)d.w, j);
}

}  // namespace fdcm
