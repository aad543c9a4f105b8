// fdcm_build.hip -- DT3 feature-map build on gfx950 (buildCpuFeaturemap<D>, dt3cpu.h:174-234).
//
// Volume layout in HBM, from the sweeps on: interleaved, [k][x/4][y][x%4] (ivol_index, fdcm_internal.h): 16 bytes hold 4
// neighbouring columns of one row, and no kernel reads or writes another.  The sweeps write the transforms into `vol`, the
// propagation reads them and writes `ivol`, the line integral reads `ivol` and writes its sums back into `vol`, which is
// what the search gathers from.
//
// Kernels (W x H = feature size, m = slices, V = 4*m*W*H bytes):
//   K0 k_seeds          clipped scene lines -> seed bitmap (1 bit per pixel, bits along y)   ~V/32
//   K1 k_coldesc_tile   per column and 64-row chunk: seed bits + nearest seed before/after   ~V/16
//   K2 L2 / L2^2        both 1-D passes in one sweep along x, pass 1 from the descriptors: fdcm_sweep.hip (column ranges of
//                       equal count, merged) where W^2 + H^2 <= 2^24, fdcm_sweep_literal.hip (one wave per chunk) above   write V
//      L1  k_l1_*       both sweeps with one pass over the volume (minima per word from the descriptors, carries, word by word)   write V
//   K3 k_propagate_reg<M> / k_propagate   orientation propagation, 4m steps per pixel in
//                       registers (generic depth: LDS) (+ sqrt for L2)                        read V, write V
//   K4 k_integral       directional prefix sum per slice, one sequential float chain per row / column of 16-byte
//                       units; shallow and steep sweeps (the latter through LDS tiles) in one launch  read V, write V
// Compiled with -ffp-contract=off; divide and sqrt are the correctly rounded forms.
#include <atomic>
#include <chrono>
#include <cstring>

#include "fdcm_build_dev.h"
#include "fdcm_internal.h"
#include "fdcm_sweep.h"

namespace fdcm {

// ------------------------------------------------------------------------------------------ K0
// drawLines (drawing.h:111-125): one block per clipped line, threads over its raster points.
__global__ void k_seeds(const RasterLine* __restrict__ lines, unsigned long long* __restrict__ bitmap, int W, int H,
                        int HW64) {
    const RasterLine r = lines[blockIdx.x];
    for (int i = threadIdx.x; i < r.n; i += blockDim.x) {
        const float fx = lin_spaced_value(r.xmode, r.xlow, r.xhigh, r.xstep, r.n, i);
        const float fy = lin_spaced_value(r.ymode, r.ylow, r.yhigh, r.ystep, r.n, i);
        const long x = (long)roundf(fx);  // .round().cast<Eigen::Index>(): half away from zero
        const long y = (long)roundf(fy);
        if (x < 0 || x >= W || y < 0 || y >= H) continue;  // the reference would write out of bounds
        atomicOr(&bitmap[((size_t)r.slice * W + x) * HW64 + (y >> 6)], 1ull << (y & 63));
    }
}

// ------------------------------------------------------------------------------------------ K1
// Pass 1 of distanceTransform (imgproc.h:178 / :186 along y).  On a 0 / FLT_MAX image the
// lower-envelope pass yields exactly the squared distance to the nearest seed of the column
// (every envelope owner is a seed and owns itself), or FLT_MAX for a seedless column; the L1
// sweeps yield the plain distance.  Both are integers < 2^24, so any exact method gives the
// reference's bits.  One wave per column (k, x); lanes are 64 consecutive y.
// The seed words are cleared as they are read (when one pass reads each word once), so the next build of
// the same size starts from a zero bitmap without a separate fill.
__global__ void __launch_bounds__(256) k_coldesc(unsigned long long* __restrict__ bitmap,
                                                 ColDesc* __restrict__ desc, int W, int HW64, long ncols) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long col = (long)blockIdx.x * (blockDim.x >> 6) + wave;  // = k * W + x
    if (col >= ncols) return;
    const long k = col / W, x = col - k * W;
    unsigned long long* bw = bitmap + (size_t)col * HW64;
    const int ngroups = (HW64 + 63) >> 6;  // groups of 64 words = 4096 rows
    int carry_prev = INT_MIN;              // last seed row in earlier groups
    for (int g = 0; g < ngroups; ++g) {
        const int wi = g * 64 + lane;
        const unsigned long long word = wi < HW64 ? bw[wi] : 0ull;
        if (ngroups == 1 && word) bw[wi] = 0ull;
        const int last_i = word ? wi * 64 + 63 - __clzll(word) : INT_MIN;
        const int first_i = word ? wi * 64 + (__ffsll((long long)word) - 1) : INT_MAX;
        int carry_next = INT_MAX;  // first seed row in later groups (only when H > 4096)
        for (int g2 = ngroups - 1; g2 > g; --g2) {
            const int wj = g2 * 64 + lane;
            const unsigned long long w2 = wj < HW64 ? bw[wj] : 0ull;
            carry_next = min(carry_next, wave_min(w2 ? wj * 64 + (__ffsll((long long)w2) - 1) : INT_MAX));
        }
        ColDesc d;
        d.word = word;
        const int pv = max(wave_scan_max_excl(last_i, lane), carry_prev);
        const int nx = min(wave_scan_min_excl_rev(first_i, lane), carry_next);
        d.prev = pv == INT_MIN ? -kFar : pv;
        d.next = nx == INT_MAX ? kFar : nx;
        if (wi < HW64) desc[((size_t)k * HW64 + wi) * W + x] = d;
        carry_prev = max(carry_prev, wave_max(last_i));
    }
}

// The same for H <= 4096 (one group of words per column), with coalesced stores: a block takes 64 neighbouring
// columns of a slice, SEG lanes (16 / 32 / 64: the words of a column) scan one column each, 64 / SEG columns per wave
// pass, and the descriptors go through LDS so that every store covers the block's columns of one chunk (1 KB or 512 B
// contiguous; the wave-per-column kernel writes 16 bytes every W * 16).
// The seeds come straight from the slice's clipped lines (drawLines, drawing.h:111-125: k_seeds' points): every block
// rasterises the lines of its slice that can reach its XT columns into a bitmap tile in LDS -- no seed bitmap in memory, no
// launch of its own for a few thousand points, no atomics on HBM.
template <int SEG, int XT>  // XT columns per block: 64, or 32 when a column has 64 words (32 KB of LDS instead of 64)
__global__ void __launch_bounds__(256) k_coldesc_tile(const RasterLine* __restrict__ lines, const int* __restrict__ slice_first,
                                                      ColDesc* __restrict__ desc, int W, int H, int HW64, unsigned* __restrict__ colmask) {
    extern __shared__ uint4 tile[];  // [word][XT columns], rows padded by one unit (bank spread); behind it the seed bits [word][XT]
    constexpr int STR = XT + 1;
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(tile + (size_t)HW64 * STR);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long k = blockIdx.y;
    const int x0 = blockIdx.x * XT;
    for (int i = threadIdx.x; i < HW64 * XT; i += 256) bits[i] = 0ull;
    __syncthreads();
    for (int li = slice_first[k]; li < slice_first[k + 1]; ++li) {
        const RasterLine r = lines[li];
        // the line's columns: between its two ends (a constant when xmode == 0), half a pixel of rounding on either side
        const float xa = r.xmode == 0 ? r.xlow : fminf(r.xlow, r.xhigh), xb = r.xmode == 0 ? r.xlow : fmaxf(r.xlow, r.xhigh);
        if (xb + 1.f < (float)x0 || xa - 1.f > (float)(x0 + XT - 1)) continue;
        for (int i = threadIdx.x; i < r.n; i += 256) {
            const float fx = lin_spaced_value(r.xmode, r.xlow, r.xhigh, r.xstep, r.n, i);
            const long x = (long)roundf(fx);  // .round().cast<Eigen::Index>(): half away from zero
            if (x < x0 || x >= x0 + XT || x >= W) continue;
            const float fy = lin_spaced_value(r.ymode, r.ylow, r.yhigh, r.ystep, r.n, i);
            const long y = (long)roundf(fy);
            if (y < 0 || y >= H) continue;  // the reference would write out of bounds
            atomicOr(&bits[(y >> 6) * XT + (int)(x - x0)], 1ull << (y & 63));
        }
    }
    __syncthreads();
    coldesc_from_bits<SEG, XT>(tile, bits, desc, W, HW64, colmask, k, x0, lane, wave);
}

// ---- The two L1 sweeps with ONE pass over the volume (round 3).
// The forward sweep is F[x] = min(c[x], F[x-1] + 1) on the column values c (exact integers, or FLT_MAX for a seedless column,
// which absorbs every +1 and +-x), the backward one R[x] = min(F[x], R[x+1] + 1) on its result (imgproc.h:138-145).  As two
// kernels they write V, read V and write V again; the 24 GB of config 5 went at the rate of a plain copy (2.4 + 4.9 ms).
// Both recurrences only carry one number per row across a cut: F[x0 - 1] = min over x' < x0 of (c[x'] - x') + (x0 - 1), and
// for the backward one R[x1 + 1] may be replaced by B[x1 + 1] = min over x' > x1 of (c[x'] + x') - (x1 + 1), the plain
// backward scan of c (R[x1] = min(F[x1], F[x1+1] + 1, B[x1+1] + 1) and F[x1+1] + 1 = min(c[x1+1] + 1, F[x1] + 2) is never
// below min(F[x1], B[x1+1] + 1)).  All terms are integers below 2^24 or FLT_MAX: every float operation is exact, so the
// regrouping changes no bit.  So: the two minima per (row, 64-column word) from the descriptors alone (k_l1_word_mins),
// their exclusive prefix / suffix minima over the words of a row (k_l1_carries, 3 % of V), and then every word by itself:
// c from the descriptors, forward from its carry into 64 registers, backward from its carry, one store (k_l1_word).
__device__ __forceinline__ float l1_column_value(const ColDesc& dcur, unsigned long long nz, int j, int lane, int y) {
    if ((nz >> j) & 1ull) {  // a seed inside the chunk's 64 rows (wave-uniform): the bit scans
        unsigned long long wc;
        int pc, nc;
        desc_lane(dcur, j, wc, pc, nc);
        return column_value<false>(wc, pc, nc, lane, y);
    }
    const int pc = __builtin_amdgcn_readlane(dcur.prev, j), nc = __builtin_amdgcn_readlane(dcur.next, j);
    const int d = min(y - pc, nc - y);
    return d >= (1 << 29) ? FLT_MAX : (float)d;  // no seed in the whole column
}
__global__ void __launch_bounds__(256) k_l1_word_mins(const ColDesc* __restrict__ desc, float2* __restrict__ mins, int W, int HW64,
                                                      int nwords, long nwaves) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (wid >= nwaves) return;
    const long kc = wid / nwords;  // slice * HW64 + chunk
    const int w = (int)(wid - kc * nwords), c = (int)(kc % HW64), y = c * 64 + lane;
    const int x0 = w * 64, jn = min(64, W - x0);
    const ColDesc dcur = desc[(size_t)kc * W + min(x0 + lane, W - 1)];
    const unsigned long long valid = jn == 64 ? ~0ull : (1ull << jn) - 1ull;
    const unsigned long long nz = __builtin_amdgcn_ballot_w64(dcur.word != 0ull) & valid;
    // A column without a seed inside the chunk is worth min(y - prev, next - y) in every row y of the chunk, so over such
    // columns  min (c - x) = min(y - max (prev + x), min (next - x) - y)  and  min (c + x) = min(y - max (prev - x), min (next + x) - y):
    // four reductions over the word's descriptors (lane = column) and six instructions per row, for 64 columns x 18.  The
    // integers are exact (missing sides are 2^30 away; a result of that size means "no seed at all" = FLT_MAX, as the
    // per-column form says it).  Columns with a seed inside the chunk (one word in seven has any) go one by one.
    const bool far = lane < jn && dcur.word == 0ull;
    const int xj = x0 + lane;
    const int a1 = wave_max(far ? dcur.prev + xj : -(1 << 30)), a2 = wave_min(far ? dcur.next - xj : (1 << 30));
    const int b1 = wave_max(far ? dcur.prev - xj : -(1 << 30)), b2 = wave_min(far ? dcur.next + xj : (1 << 30));
    const int ai = min(y - a1, a2 - y), bi = min(y - b1, b2 - y);
    float a = ai >= (1 << 28) ? FLT_MAX : (float)ai, b = bi >= (1 << 28) ? FLT_MAX : (float)bi;
    for (unsigned long long m = nz; m; m &= m - 1ull) {
        const int j = __ffsll((long long)m) - 1;
        const float cq = l1_column_value(dcur, nz, j, lane, y), xf = (float)(x0 + j);
        a = std_min(a, cq - xf);
        b = std_min(b, cq + xf);
    }
    mins[(size_t)wid * 64 + lane] = make_float2(a, b);
}
// in place: .x <- min of the .x of the words before, .y <- min of the .y of the words behind (FLT_MAX where there is none)
__global__ void __launch_bounds__(256) k_l1_carries(float2* __restrict__ mins, int nwords, long nrows) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;  // (slice * HW64 + chunk) * 64 + row
    if (gid >= nrows) return;
    float2* m = mins + (size_t)(gid >> 6) * nwords * 64 + (gid & 63);
    float p = FLT_MAX;
    for (int w = 0; w < nwords; ++w) { const float t = m[(size_t)w * 64].x; m[(size_t)w * 64].x = p; p = std_min(p, t); }
    float q = FLT_MAX;
    for (int w = nwords - 1; w >= 0; --w) { const float t = m[(size_t)w * 64].y; m[(size_t)w * 64].y = q; q = std_min(q, t); }
}
template <bool FULL>  // FULL: the word has all 64 columns (every word but a row's last one)
__device__ __forceinline__ void l1_word(const ColDesc& dcur, unsigned long long nz, float2 carry, int x0, int jn, int lane, int y,
                                        __amdgpu_buffer_rsrc_t rs, unsigned vrow, int grpB) {
    float f[64];
    float run = carry.x + (float)(x0 - 1);  // F[x0 - 1]; FLT_MAX in front of the row's first column: min(c, FLT_MAX + 1) = c
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        f[j] = 0.f;  // (columns past W are padding and hold 0)
        if (FULL || j < jn) {
            run = std_min(l1_column_value(dcur, nz, j, lane, y), run + 1);
            f[j] = run;
        }
    }
    float r = carry.y - (float)(x0 + jn);  // B[x1 + 1]; FLT_MAX behind the row's last column: min(F, FLT_MAX + 1) = F
#pragma unroll
    for (int j = 63; j >= 0; --j) {
        if (FULL || j < jn) {
            r = std_min(f[j], r + 1);
            f[j] = r;
        }
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        if (FULL || 4 * g < jn) {
            u32x4 out;
            out.x = __float_as_uint(f[4 * g]); out.y = __float_as_uint(f[4 * g + 1]); out.z = __float_as_uint(f[4 * g + 2]); out.w = __float_as_uint(f[4 * g + 3]);
            __builtin_amdgcn_raw_buffer_store_b128(out, rs, vrow + (unsigned)(((x0 >> 2) + g) * grpB), 0, 0);  // (no scalar offset: see store_unit_note)
        }
    }
}
__global__ void __launch_bounds__(256) k_l1_word(const ColDesc* __restrict__ desc, const float2* __restrict__ carries, float* __restrict__ vol,
                                                 int W, int H, int HW64, int nwords, long nwaves) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (wid >= nwaves) return;
    const long kc = wid / nwords;
    const long k = kc / HW64;
    const int w = (int)(wid - kc * nwords), c = (int)(kc - k * HW64), y = c * 64 + lane;
    const int x0 = w * 64, jn = min(64, W - x0);
    const ColDesc dcur = desc[(size_t)kc * W + min(x0 + lane, W - 1)];
    const float2 carry = carries[(size_t)wid * 64 + lane];
    const unsigned long long nz = __builtin_amdgcn_ballot_w64(dcur.word != 0ull);
    const size_t sl = ivol_slice_floats(W, H);
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(vol + (size_t)k * sl, 0, (unsigned)(sl * 4), 0x00020000);
    const unsigned vrow = y < H ? (unsigned)y * 16u : 0x80000000u;  // rows past the image: dropped stores
    if (jn == 64) l1_word<true>(dcur, nz, carry, x0, jn, lane, y, rs, vrow, H * 16);
    else l1_word<false>(dcur, nz, carry, x0, jn, lane, y, rs, vrow, H * 16);
}

__global__ void k_sqrt(float* __restrict__ vol, size_t n) {  // only for staged (test) builds
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) vol[i] = sqrtf(vol[i]);
}

// ------------------------------------------------------------------------------------------ K3
// propagateOrientation (dt3cpu.cpp:77-107): each pixel's m-vector is loaded once into LDS
// ([slice][thread], conflict free), the 4m steps S[c2] = min(S[c2], S[c1] + w) run there, and it
// is stored once.  L2's final sqrt (imgproc.h:191-192) is applied on load.
// Both variants read the transforms and write the propagated volume in the same interleaved layout (ivol_index): a thread
// is a position q of the slice and touches position q of every slice, 64 consecutive threads 256 contiguous bytes of each.
// The padding (columns of the last group past W, the kSlicePad tail) is propagated like any pixel and never read as one.
__global__ void k_propagate(const float* __restrict__ vol, float* __restrict__ ivol, int W, int H, int m,
                            const PropStep* __restrict__ steps, int nsteps, int apply_sqrt) {
    extern __shared__ float S[];
    const int bd = blockDim.x, tid = threadIdx.x;
    const size_t q = (size_t)blockIdx.x * bd + tid, nq = ivol_slice_floats(W, H);
    const bool ok = q < nq;
    for (int j = 0; j < m; ++j) {
        float v = ok ? vol[(size_t)j * nq + q] : 0.f;
        if (apply_sqrt) v = sqrtf(v);
        S[j * bd + tid] = v;
    }
    for (int s = 0; s < nsteps; ++s) {
        const PropStep st = steps[s];
        const float a = S[st.c2 * bd + tid];
        const float b = S[st.c1 * bd + tid] + st.w;
        S[st.c2 * bd + tid] = std_min(a, b);
    }
    if (ok)
        for (int j = 0; j < m; ++j) ivol[(size_t)j * nq + q] = S[j * bd + tid];
}

// Register-resident variant for the common depths: the ring indices of propagateOrientation's
// 4M steps (dt3cpu.cpp:88-89) are compile-time constants, so the pixel's M-vector stays in VGPRs
// and the kernel is a pure stream (read V, write V) at full occupancy.
template <int M>
__global__ void __launch_bounds__(256) k_propagate_reg(const float* __restrict__ vol, float* __restrict__ ivol, int W, int H,
                                                       const PropStep* __restrict__ steps, int apply_sqrt) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nq = ivol_slice_floats(W, H);
    if (q >= nq) return;
    // One buffer descriptor per slice (scalar registers) + one 32-bit lane byte offset: addresses
    // cost no vector registers, so the M values are the kernel's whole register footprint.
    const unsigned off = (unsigned)q * 4u, slice_bytes = (unsigned)(nq * 4u);  // slices are < 2^30 pixels
    // The loads' copies of stride and offset are opaque to the compiler: knowing them equal to the stores', it keeps all M slice offsets
    // in SGPRs from the loads to the stores (106, 30 to 270 of them spilled from M = 60 on, against 28); one alone hidden, M = 60 loses a wave.
    size_t nq_in = nq; asm volatile("" : "+s"(nq_in));
    unsigned off_in = off; asm volatile("" : "+v"(off_in));
    const unsigned in_bytes = (unsigned)(nq_in * 4u);
    float S[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(vol) + (size_t)j * nq_in, 0, in_bytes, 0x00020000);
        S[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off_in, 0, 0));
    }
    if (apply_sqrt) {
#pragma unroll
        for (int j = 0; j < M; ++j) S[j] = sqrtf(S[j]);
    }
    constexpr int FWD = (3 * M + 1) / 2;  // ceil(1.5 M)
    constexpr int BWD = (3 * M) / 2;      // floor(1.5 M)
    int s = 0;
#pragma unroll
    for (int c = 0; c < FWD; ++c, ++s) {  // propagate(0, ceil(1.5 m), +1)
        const int c1 = (M + ((c - 1) % M)) % M, c2 = (M + (c % M)) % M;
        S[c2] = std_min(S[c2], S[c1] + steps[s].w);
    }
#pragma unroll
    for (int i = 0; i < M + BWD; ++i, ++s) {  // propagate(m, -floor(1.5 m), -1): c = M - i
        const int c = M - i;
        const int c1 = (M + ((c + 1) % M)) % M, c2 = (M + (c % M)) % M;
        S[c2] = std_min(S[c2], S[c1] + steps[s].w);
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(ivol + (size_t)j * nq, 0, slice_bytes, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(S[j]), rs, off, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------ K4
// lineIntegral (imgproc.h:38-84).  The reference adds the previous (already integrated) line,
// shifted by dy_i = round(i r) - round((i-1) r), into the current one; the shifts telescope, so
// pixel (x_i, c + round(i r)) belongs to chain c and each chain is one sequential float32 sum, added in the
// reference's order.  Input and output are interleaved volumes (ivol_index: 16 bytes = 4 neighbouring columns of
// one row), the kernel reads one and writes the other, and every memory operation moves whole 16-byte units:
// a unit is stored by exactly one wave (shallow) or block (steep), which computes the up to three chains of a
// neighbour that cross its units itself (3 of 61 / 64 chains are such a halo) instead of sharing units.

// ---- shallow slices (mode 1: the sweep runs along x, a wave's chains are neighbouring rows)
// Per group of 4 columns (4 sweep steps) a wave issues one 16-byte load and one 16-byte store per lane: lane rho is
// the row where its chain sits at the group's first step.  During the group a chain moves on by 0 or 1 row per
// step (|r| <= 1), always in the direction of sign(r), so the running sums are kept in row coordinates: after a
// step that moves the chains the accumulator is shifted by one lane (DPP wave_shr), inputs and outputs need no
// shuffling, and at the end of the group the accumulator is shifted back by the group's total.
// Lane rho <-> chain a + sg*(rho - 3), sg = sign(r): lanes 0..2 are the halo (the chains that reach the wave's
// first rows during a group), lanes 3..60 the 58 chains whose rows the wave stores, lanes 61..63 would fall off
// the 64-row window after 3 moves and are not used.
static constexpr int kShP = 12;                       // groups (loads of 1 KB) in flight per wave
static constexpr int kShOwn = 58, kShHalo = 3;
// Table per slice, one word per group in sweep order: 16 * (chain offset round(i r) at the group's first step) |
// bit j: the chains move between the group's steps j and j+1.  Steps outside the image (the padding columns of
// the last group) repeat the nearest offset.  Past the last group: 2^30, an out-of-range row for every lane.
__host__ __device__ inline int sh_tab_stride(int W) { return (((W + 3) / 4 + 2 * kShP) + 3) & ~3; }
__global__ void k_groups(const IntegralDesc* __restrict__ desc, int* __restrict__ tab, int W, int stride) {
    const int G = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (G >= stride) return;
    const IntegralDesc d = desc[k];
    const int W4 = (W + 3) / 4;
    int word = 0x40000000;
    if (d.mode == 1 && G < W4) {
        int o[4];
        for (int j = 0; j < 4; ++j) {
            const int x = d.s > 0 ? 4 * G + j : 4 * (W4 - 1 - G) + 3 - j;
            const int i = min(max(d.s > 0 ? x : W - 1 - x, 0), W - 1);      // sweep step of column x (imgproc.h:54-55)
            o[j] = (int)roundf((float)i * d.r);
        }
        word = o[0] * 16 | (o[1] != o[0] ? 1 : 0) | (o[2] != o[1] ? 2 : 0) | (o[3] != o[2] ? 4 : 0);
    }
    tab[(size_t)k * stride + G] = word;
}

__device__ __forceinline__ float lane_shr1(float v) {  // lane i <- lane i-1 (lane 0 <- 0)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float lane_shl1(float v) {  // lane i <- lane i+1 (lane 63 <- 0)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true));
}

__device__ __forceinline__ void integral_shallow(const float* __restrict__ src, float* __restrict__ dst, int W, int H,
                                                 const IntegralDesc& d, int k, const int* __restrict__ tab, int shw) {
    constexpr int P = kShP;
    static_assert(P % 4 == 0, "the table is read four groups at a time");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W4 = (W + 3) >> 2;
    const int last_off = (int)roundf((float)(W - 1) * d.r);
    const int cmin = -max(0, last_off), cmax = H - 1 - min(0, last_off);
    if (wave >= shw) return;  // shw = 1 (one working wave per workgroup) or 4: see k_integral
    const int lo = cmin + ((int)blockIdx.x * shw + wave) * kShOwn;  // the wave stores the rows of chains lo .. lo + 57
    if (lo > cmax) return;
    const int sg = d.r < 0.f ? -1 : 1;
    const int a = sg > 0 ? lo : lo + kShOwn - 1;
    const int lanebase = (a + sg * (lane - kShHalo)) * 16;  // byte offset of the lane's row inside a group at chain offset 0
    const bool own = lane >= kShHalo && lane < kShHalo + kShOwn;
    const int* tb = tab + (size_t)k * sh_tab_stride(W);
    const size_t sl = ivol_slice_floats(W, H);
    const long gstride = (long)d.s * H * 4;  // floats from a group to the next one of the sweep
    const size_t g0 = d.s > 0 ? 0 : (size_t)(W4 - 1) * H * 4;
    const float* gf = src + (size_t)k * sl + g0;  // group of the next fetch
    float* gc = dst + (size_t)k * sl + g0;        // group of the next store
    const bool up = d.s > 0;                      // columns of a group in sweep order: x y z w, or w z y x
    constexpr unsigned OOB = 0x80000000u;
    u32x4 v[P];
    auto fetch = [&](int word, u32x4& r) {
        // one descriptor per group: base = the group, size = one group, so rows outside the image (and every row of
        // the groups past the end) read as 0 and their stores are dropped
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gf), 0, (unsigned)H * 16u, 0x00020000);
        r = __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(lanebase + (word & ~15)), 0, 0);
        gf += gstride;
    };
#pragma unroll
    for (int p = 0; p < P; p += 4) {
        const int4 w4 = *reinterpret_cast<const int4*>(tb + p);
        fetch(w4.x, v[p]); fetch(w4.y, v[p + 1]); fetch(w4.z, v[p + 2]); fetch(w4.w, v[p + 3]);
    }
    // The first fetches are waited for here, once: the compiler orders them freely, and its wait at the loop header has
    // to cover the entry as well as the back edge -- with anything pending on entry it waits for (nearly) all memory
    // operations in every iteration.
#pragma unroll
    for (int p = 0; p < P; ++p) asm volatile("" : "+v"(v[p]));
    float acc = 0.f;
    for (int G0 = 0; G0 < W4; G0 += P) {
#pragma unroll
        for (int p = 0; p < P; p += 4) {
            const int4 wc = *reinterpret_cast<const int4*>(tb + G0 + p);
            const int4 wn = *reinterpret_cast<const int4*>(tb + G0 + p + P);
            const int wcur[4] = {wc.x, wc.y, wc.z, wc.w}, wnext[4] = {wn.x, wn.y, wn.z, wn.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int word = wcur[q];
                const u32x4 in = v[p + q];
                const float i0 = __uint_as_float(up ? in.x : in.w), i1 = __uint_as_float(up ? in.y : in.z),
                            i2 = __uint_as_float(up ? in.z : in.y), i3 = __uint_as_float(up ? in.w : in.x);
                // out-of-image elements are +0: 0 + acc == acc exactly (acc >= +0)
                acc = i0 + acc; const float o0 = acc; if (word & 1) acc = lane_shr1(acc);
                acc = i1 + acc; const float o1 = acc; if (word & 2) acc = lane_shr1(acc);
                acc = i2 + acc; const float o2 = acc; if (word & 4) acc = lane_shr1(acc);
                acc = i3 + acc; const float o3 = acc;
                const int moved = __builtin_popcount(word & 7);
                if (moved > 0) acc = lane_shl1(acc);
                if (moved > 1) acc = lane_shl1(acc);
                if (moved > 2) acc = lane_shl1(acc);
                u32x4 out;
                out.x = __float_as_uint(up ? o0 : o3); out.y = __float_as_uint(up ? o1 : o2);
                out.z = __float_as_uint(up ? o2 : o1); out.w = __float_as_uint(up ? o3 : o0);
                const auto rs = __builtin_amdgcn_make_buffer_rsrc(gc, 0, (unsigned)H * 16u, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b128(out, rs, own ? (unsigned)(lanebase + (word & ~15)) : OOB, 0, 0);
                gc += gstride;
                fetch(wnext[q], v[p + q]);
            }
        }
    }
}

// ---- steep slices (mode 2: the sweep runs along y, chains run across x)
// They go through LDS tiles: a block computes 64 neighbouring chains, loads [64 + 32 (+4 to start on a group)
// columns] x [32 sweep steps] as 16-byte units (4 columns of one row), wave 0 runs the 64 sequential sums on the
// tile, and the units whose first column belongs to one of the block's first 60 chains are stored (their other
// three columns belong to the next three chains at most: the halo).  The next tile's loads are in flight while
// the current one is summed and stored.
// XC chains per block (XC / 64 waves run them), of which the first XC - 4 are the block's own: 64 while the launch is
// small (more blocks, shorter critical path), 256 when the slices are large -- a tile is XC + drift + 4 columns wide,
// so the columns read per column stored fall from (64 + 36) / 60 = 1.67 to (256 + 36) / 252 = 1.16, and the drift is
// sized per slice: the chains of a slice move by at most ceil(31 |r|) + 1 columns over a tile's 32 steps, not by 32.
template <int XC>
__device__ __forceinline__ void integral_steep(const float* __restrict__ src, float* __restrict__ dst, int W, int H,
                                               const IntegralDesc& d, int k, float* lds_tiles) {
    constexpr int TS = 32, TW = XC + TS + 4, NG = TW / 4, PASSES = (NG + 7) / 8, OWN = XC - 4;
    float (*tile)[TW][TS + 1] = reinterpret_cast<float (*)[TW][TS + 1]>(lds_tiles);  // [2][TW][TS + 1]
    const int steps = H, span = W, W4 = (W + 3) >> 2;
    const int last_off = (int)roundf((float)(steps - 1) * d.r);
    const int cmin = -max(0, last_off), cmax = span - 1 - min(0, last_off);
    const int c0 = cmin + (int)blockIdx.x * OWN;
    if (c0 > cmax) return;
    const int start = d.s < 0 ? steps - 1 : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int prow = tid & 31, pgrp = tid >> 5;  // load/store mapping: 8 groups x 32 rows per pass
    const int ntiles = (steps + TS - 1) / TS;
    // groups of a tile that this slice can touch: chains + the drift over TS - 1 steps (|round(a) - round(b)| <=
    // ceil(|a - b|) + 1) + up to 3 columns in front of the first chain (tiles start on a group)
    const int ng = min(NG, (XC + (int)ceilf((float)(TS - 1) * fabsf(d.r)) + 1 + 3 + 3) >> 2);
    // Units outside the image get an out-of-range offset: loads return 0, stores are dropped, and no memory
    // operation sits behind a branch, so the compiler counts them exactly and the loads of two tiles stay in
    // flight behind the stores of the previous ones.
    const size_t sl = ivol_slice_floats(W, H);
    const auto rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src) + (size_t)k * sl, 0, (unsigned)(sl * 4), 0x00020000);
    const auto rs_out = __builtin_amdgcn_make_buffer_rsrc(dst + (size_t)k * sl, 0, (unsigned)(sl * 4), 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    auto off_at = [&](int i) { return (int)roundf((float)i * d.r); };  // chain offset at step i (imgproc.h:70-71)
    // first column of tile t: the leftmost column of the block's chains over the tile's steps, rounded down to a group
    auto xbase = [&](int t) { return (c0 + min(off_at(t * TS), off_at(min(t * TS + TS - 1, steps - 1)))) & ~3; };
    auto unit_off = [&](int xg, int i) {  // byte offset of the unit of group xg at sweep step i
        return (xg >= 0 && xg < W4 && i < steps) ? (unsigned)((xg * H + start + i * d.s) << 4) : OOB;
    };
    auto load_tile = [&](int t, u32x4 (&regs)[PASSES]) {
        const int i = t * TS + prow, xg0 = xbase(t) >> 2;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int g = p * 8 + pgrp;
            regs[p] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, g < ng ? unit_off(xg0 + g, i) : OOB, 0, 0);
        }
    };
    float acc = 0.f;
    auto process = [&](int t, u32x4 (&regs)[PASSES]) {  // regs hold tile t on entry, tile t + 2 on exit
        const int buf = t & 1, i0 = t * TS, xb = xbase(t);
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int g = p * 8 + pgrp;
            if (g < NG) {
                tile[buf][4 * g + 0][prow] = __uint_as_float(regs[p].x);
                tile[buf][4 * g + 1][prow] = __uint_as_float(regs[p].y);
                tile[buf][4 * g + 2][prow] = __uint_as_float(regs[p].z);
                tile[buf][4 * g + 3][prow] = __uint_as_float(regs[p].w);
            }
        }
        __syncthreads();
        load_tile(t + 2, regs);  // past the last tile every load is out of range
        if (wave < XC / 64) {
            // Chain c0 + ch, ch = 64 wave + lane.  At step ii it sits in tile column ch + off_ii - (xb - c0): always
            // inside the tile.  No validity test is needed here: elements outside the image or past the last
            // step were loaded as +0 (acc + 0 == acc exactly) and every tile element belongs to exactly one chain.
            const int ch = wave * 64 + lane;
            const int my_d = off_at(min(i0 + (lane & 31), steps - 1)) - (xb - c0);  // lane j < 32: step i0 + j
            // all 32 reads are issued before the dependent chain of adds (they never alias: one element per
            // step), so the chain costs 32 adds, not 32 LDS round trips
            float v[TS];
            float* cell[TS];
#pragma unroll
            for (int ii = 0; ii < TS; ++ii) {
                cell[ii] = &tile[buf][ch + __builtin_amdgcn_readlane(my_d, ii)][ii];
                v[ii] = *cell[ii];
            }
#pragma unroll
            for (int ii = 0; ii < TS; ++ii) {
                acc = v[ii] + acc;
                *cell[ii] = acc;
            }
        }
        __syncthreads();
        {  // a unit is stored by the block that owns the chain of its first column
            const int i = i0 + prow;
            const int o = off_at(min(i, steps - 1));
#pragma unroll
            for (int p = 0; p < PASSES; ++p) {
                const int g = p * 8 + pgrp;
                const int fc = xb + 4 * g - o;  // chain of the unit's first column
                u32x4 out;
                const int gg = g < NG ? g : 0;
                out.x = __float_as_uint(tile[buf][4 * gg + 0][prow]); out.y = __float_as_uint(tile[buf][4 * gg + 1][prow]);
                out.z = __float_as_uint(tile[buf][4 * gg + 2][prow]); out.w = __float_as_uint(tile[buf][4 * gg + 3][prow]);
                const bool mine = g < ng && fc >= c0 && fc < c0 + OWN;
                __builtin_amdgcn_raw_buffer_store_b128(out, rs_out, mine ? unit_off((xb >> 2) + g, i) : OOB, 0, 0);
            }
        }
    };
    u32x4 ra[PASSES], rb[PASSES];
    load_tile(0, ra);
    load_tile(1, rb);
    for (int t = 0; t < ntiles; t += 2) {
        process(t, ra);
        if (t + 1 < ntiles) process(t + 1, rb);
    }
}
template <int XC>
constexpr size_t integral_lds_bytes() { return (size_t)2 * (XC + 32 + 4) * 33 * sizeof(float); }

// One launch for all slices: blockIdx.y = slice, and the slice's mode picks the sweep.  Shallow and
// steep slices are independent, so their (latency-bound) blocks overlap instead of running as two
// kernels back to back.  A workgroup takes 60 chains of a steep slice, or 58 chains of a shallow one on one wave
// (the other three exit at once) while the launch is small: a CU can only have so many cache misses outstanding, and
// four such waves on one CU (105 of 256 CUs busy at config 2) ran at 0.061 ms where one per workgroup, spread over
// all CUs, runs at 0.051.  Large launches (config 5: 25 000 workgroups) fill every CU anyway and put 4 x 58 chains on a
// workgroup (5.9 against 6.4 ms).
template <int XC>
__global__ void __launch_bounds__(256) k_integral(const float* __restrict__ src, float* __restrict__ dst, int W, int H,
                                                  const IntegralDesc* __restrict__ desc,
                                                  const int* __restrict__ tab, int shw, int kstride) {
    extern __shared__ float lds_tiles[];
    // Slices are taken in a strided order (kstride is coprime to the slice count and close to half of it): in index order
    // all steep slices of one angular range run before the shallow ones, and the two kinds stress different things (LDS
    // tiles against straight 1 KB streams), so mixing them over the launch overlaps them.
    const int k = (int)(((long)blockIdx.y * kstride) % (long)gridDim.y);
    const IntegralDesc d = desc[k];
    if (d.mode == 1) integral_shallow(src, dst, W, H, d, k, tab, shw);
    else if (d.mode == 2) integral_steep<XC>(src, dst, W, H, d, k, lds_tiles);
    else {  // nothing to integrate (imgproc.h:43): the slice moves as it is
        const size_t sl = ivol_slice_floats(W, H);
        for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < sl; q += (size_t)gridDim.x * 256)
            dst[(size_t)k * sl + q] = src[(size_t)k * sl + q];
    }
}

// ------------------------------------------------------------------------------------------ driver
void ensure_stream(fdcm_featuremap* fm) {
    if (!fm->stream) FDCM_HIP(hipStreamCreateWithFlags(&fm->stream, hipStreamNonBlocking));
    if (fm->timing.created) return;
    for (auto& e : fm->timing.ev) FDCM_HIP(hipEventCreate(&e));
    fm->timing.created = true;
}

// builds of this process whose L2 sweep took its launch order from the handle's previous build / from the host's proxy
static std::atomic<int64_t> g_order_from_history{0}, g_order_from_proxy{0};
void sweep_order_counts(int64_t* from_history, int64_t* from_proxy) {
    *from_history = g_order_from_history.load();
    *from_proxy = g_order_from_proxy.load();
}

BuildLayout build_layout(const BuildPlan& plan, int distance, int stop_after) {
    const int64_t W = plan.W, H = plan.H, m = plan.m;
    BuildLayout L;
    L.empty = m == 0 || W == 0;
    if (!L.empty && (W > 16384 || H > 16384)) throw std::string("feature size above 16384 is not supported");  // 32-bit byte offsets inside a slice
    const int HW64 = L.empty ? 0 : (int)((H + 63) / 64);
    L.HW64 = HW64; L.nchunks = (long)m * HW64;
    // the plan blob (its proxy cost region is only uploaded when the sweep's launch order takes it)
    auto align16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    L.off_prop = align16(plan.raster.size() * sizeof(RasterLine));
    L.off_integral = L.off_prop + align16(plan.prop.size() * sizeof(PropStep));
    L.off_keys = L.off_integral + align16(plan.integral.size() * sizeof(IntegralDesc));
    L.off_slice = L.off_keys + align16(plan.keys.size() * sizeof(float));
    L.off_pixels = L.off_slice + align16(plan.slice_first.size() * sizeof(int32_t));
    L.off_cost = L.off_pixels + align16(plan.seeds.on_device ? 0 : plan.seeds.source_bytes());  // (pixels in front of the cost: one copy takes them)
    L.plan = L.off_cost + align16((size_t)L.nchunks * sizeof(int32_t));
    if (L.empty) return L;
    if (plan.seeds.kind != SeedKind::lines && HW64 > 64) throw std::string("feature maps from images or labels are limited to 4096 x 4096");
    if (plan.seeds.kind == SeedKind::image) L.labels = plan.seeds.bytes();
    if (plan.seeds.kind == SeedKind::image && !plan.seeds.edge_plain()) L.edge_parent = L.edge_roots = plan.seeds.bytes() * 4;
    if (plan.seeds.level > 0) {
        int64_t w1, h1, w2, h2;
        pyramid_size(plan.seeds.width0, plan.seeds.height0, 1, &w1, &h1);
        pyramid_size(w1, h1, 1, &w2, &h2);
        L.pyr_b = align16((size_t)(w1 * h1));
        L.pyr = L.pyr_b + (size_t)(w2 * h2);
    }
    const size_t ncols = (size_t)m * W, islices = (size_t)m * ivol_slice_floats(W, H);
    L.vol = islices * sizeof(float);  // the transforms, and later the integrated volume, interleaved (>= m W H floats)
    if (HW64 > 64) L.bitmap = ncols * HW64 * 8;        // (feature sizes above 4096 only: k_seeds + k_coldesc)
    if (stop_after >= 2) L.ivol = islices * sizeof(float);
    if (stop_after >= 3) L.offtab = (size_t)m * sh_tab_stride((int)W) * sizeof(int);
    L.coldesc = ncols * HW64 * sizeof(ColDesc);
    L.colmask = (size_t)m * ((W + 63) / 64) * 8;
    // Which L2 / L2^2 sweep: ranges of equal column count, merged (fdcm_sweep.hip) where every value of the pass is an exact
    // integer, the literal pass one wave per chunk (fdcm_sweep_literal.hip) otherwise.
    const bool l2 = distance != FDCM_L1;
    L.balanced = l2 && HW64 <= 64 && sweep_balanced_applies(W, H) && !test_switches().literal_sweep;
    if (!l2) {
        L.stack = (size_t)m * HW64 * ((W + 63) / 64) * 64 * sizeof(float2);  // the L1 pass's minima / carries
    } else if (!L.balanced) {
        L.stack = sweep_literal_scratch_bytes((int)W, L.nchunks);
    } else {
        // scratch of the balanced sweep, per chunk and slot-major: stack entries (W + 2 slots per row, 12 B), owner list (W + 2 entries per
        // row, 8 B), launch order, per-chunk cost and the steal counter
        L.slots = (int)W + 2;
        const size_t NRr = (size_t)L.nchunks * 64;
        auto take = [&](size_t bytes) { const size_t o = L.stack; L.stack += (bytes + 255) & ~(size_t)255; return o; };
        L.o_ent = take(L.slots * NRr * sizeof(EnvEntry)), L.o_own = take(L.slots * NRr * sizeof(OwnEntry));
        L.o_ord = take((size_t)L.nchunks * 4), L.o_cost = take((size_t)L.nchunks * 4), L.o_steals = take(256);
    }
    return L;
}

void reserve_build(fdcm_featuremap* fm, const BuildLayout& L) {
    FDCM_HIP(hipSetDevice(fm->device));
    ensure_stream(fm);
    finish_build(fm);  // the previous build's staging and events are reused by the next
    if (L.empty) return;
    // every buffer of the build is reserved before its first kernel is queued: an allocation between two stages (a
    // handle's first build) stalls the host for 0.5 - 1 ms while the GPU idles inside the stage events' span
    BuildBuffers& b = fm->build;
    fm->vol.reserve(L.vol); b.bitmap.reserve(L.bitmap); fm->ivol.reserve(L.ivol);
    b.coldesc.reserve(L.coldesc); b.colmask.reserve(L.colmask); b.labels.reserve(L.labels);
    b.edge_parent.reserve(L.edge_parent); b.edge_roots.reserve(L.edge_roots); b.pyr.reserve(L.pyr);
    const void *stack_before = b.stack.p, *offtab_before = b.offtab.p;
    b.stack.reserve(L.stack); b.offtab.reserve(L.offtab);
    if (b.stack.p != stack_before) fm->sweep.reset();  // a new scratch: no cost table, no steal counter
    if (b.offtab.p != offtab_before) fm->groups.reset();
    b.stage.reserve(L.plan); b.plan.reserve(L.plan);
}

// ---- the stages of a build, in run_build's order: each takes the layout, the plan's device pointers and the handle, and queues on its stream
struct PlanOnDevice {  // the uploaded blob's parts (BuildLayout::off_*)
    const RasterLine* raster; const int* slice_first; const PropStep* prop; const IntegralDesc* integral; int n_raster, n_prop;
    const float* keys; const uint8_t* pixels; int pixel_stride;  // the seed source's pixels on the device (SeedKind::labels / image)
};
static void mark(fdcm_featuremap* fm, int i, bool on) { if (on) FDCM_HIP(hipEventRecord(fm->timing.ev[i], fm->stream)); }

// The balanced sweep's launch order and dynamic cuts.  Queues the order from the previous build's costs and the steal counter's
// reset, both in front of the plan's upload; fills proxy_cost when the order takes the proxy instead, which travels with the plan.
// A build whose seeds are pixels has no line boxes for the host's proxy: pass 1 counts it on the device (device_proxy: the
// cost region is cleared here, k_coldesc_labels adds to it, and stage_pass1 queues the order behind it -- no read-back).
static SweepBuf setup_balanced_sweep(fdcm_featuremap* fm, const BuildLayout& L, const BuildPlan& plan, std::vector<int32_t>& proxy_cost,
                                     bool& device_proxy) {
    SweepBuf sb{};
    hipStream_t st = fm->stream;
    char* sp = (char*)fm->build.stack.p;
    const int W = (int)plan.W;
    const long nchunks = L.nchunks, resident = 2L * device_cus(fm->device);
    // Launch order: workgroups are dispatched in index order, and when there are more of them than the GPU holds at once
    // (two per CU) the long ones must not start last.  Nothing cheap predicts a chunk's time well enough, the previous
    // build of the same shape does: scenes of a stream change little from frame to frame.  A handle's first build, and
    // every build after a change of size, takes the host's proxy per chunk (sweep_cost_proxy), which arrives with the plan.
    const bool want_order = test_switches().sweep_order || nchunks > resident;
    const bool have_cost = want_order && fm->sweep.cost_chunks == nchunks && fm->sweep.cost_w == W;
    device_proxy = want_order && !have_cost && plan.seeds.kind != SeedKind::lines;
    if (device_proxy) FDCM_HIP(hipMemsetAsync(sp + L.o_cost, 0, (size_t)nchunks * 4, st));
    else if (want_order && !have_cost) sweep_cost_proxy(plan, proxy_cost);
    if (have_cost) launch_sweep_order(st, (const int*)(sp + L.o_cost), (int)nchunks, (int*)(sp + L.o_ord));
    if (want_order) (have_cost ? g_order_from_history : g_order_from_proxy).fetch_add(1, std::memory_order_relaxed);
    sb.ent = (EnvEntry*)(sp + L.o_ent); sb.own = (OwnEntry*)(sp + L.o_own); sb.cost = (int*)(sp + L.o_cost);
    sb.order = want_order ? (const int*)(sp + L.o_ord) : nullptr;
    // Dynamic cuts (a wave out of columns begins a new range in what nobody has started): they shorten the heaviest
    // workgroup's chain and add junctions, i.e. work -- worth it where the kernel lasts as long as its slowest workgroup
    // (all workgroups resident at once, the GPU to this handle), not where workgroups queue for the CUs or frames of a
    // pipeline share them (config 2: one blocking build 0.354 -> 0.333 ms over four scenes; four frames in flight 69.7 ->
    // 68.4 M matches/s; config 3: 0.76 -> 0.81 ms).  FDCM_SWEEP_STEAL=<blocks> forces a threshold (0: never) for the tests.
    sb.steal_min = -1;  // the kernel's default threshold
    sb.steal_heavy_only = (!fm->shares_gpu && nchunks <= resident) ? 0 : 1;
    sb.steals = (int*)(sp + L.o_steals);
    if (fm->sweep.steals_off != L.o_steals) FDCM_HIP(hipMemsetAsync(sb.steals, 0, 256, st));  // a new scratch (or shape): count from 0
    sb.eslots = L.slots; sb.lslots = L.slots; sb.colmask = (const unsigned long long*)fm->build.colmask.p;
    fm->sweep.steals_off = L.o_steals; fm->sweep.cost_chunks = nchunks; fm->sweep.cost_w = W;
    return sb;
}
// plan upload: one pinned blob, one async copy (the proxy cost region only when the sweep's launch order takes it)
static PlanOnDevice upload_plan(fdcm_featuremap* fm, const BuildLayout& L, const BuildPlan& plan, const std::vector<int32_t>& proxy_cost) {
    const bool proxy_order = !proxy_cost.empty();
    fm->off_keys = L.off_keys;
    char* hs = (char*)fm->build.stage.p;
    auto put = [hs](size_t off, const auto& v) { if (!v.empty()) std::memcpy(hs + off, v.data(), v.size() * sizeof(v[0])); };
    put(L.off_raster, plan.raster); put(L.off_prop, plan.prop); put(L.off_integral, plan.integral);
    put(L.off_keys, plan.keys); put(L.off_slice, plan.slice_first); put(L.off_cost, proxy_cost);
    const SeedSource& src = plan.seeds;
    if (src.source_bytes() && !src.on_device)  // rows packed: the kernels read them with a stride of `width0`
        for (int y = 0; y < src.height0; ++y) std::memcpy(hs + L.off_pixels + (size_t)y * src.width0, src.pixels + (size_t)y * src.row_stride, (size_t)src.width0);
    const char* dp = (const char*)fm->build.plan.p;
    FDCM_HIP(hipMemcpyAsync(fm->build.plan.p, hs, proxy_order ? L.plan : L.off_cost, hipMemcpyHostToDevice, fm->stream));
    if (proxy_order)
        launch_sweep_order(fm->stream, (const int*)(dp + L.off_cost), (int)L.nchunks, (int*)((char*)fm->build.stack.p + L.o_ord));
    return PlanOnDevice{(const RasterLine*)(dp + L.off_raster), (const int*)(dp + L.off_slice), (const PropStep*)(dp + L.off_prop),
                        (const IntegralDesc*)(dp + L.off_integral), (int)plan.raster.size(), (int)plan.prop.size(),
                        (const float*)(dp + L.off_keys), src.on_device ? src.pixels : (const uint8_t*)(dp + L.off_pixels),
                        src.on_device ? src.row_stride : src.width0};
}
// pass 1: the seeds and the column descriptors
static void stage_pass1(fdcm_featuremap* fm, const BuildLayout& L, const PlanOnDevice& P, const SeedSource& src, bool device_proxy) {
    hipStream_t st = fm->stream;
    const int W = (int)fm->W, H = (int)fm->H, m = (int)fm->m, HW64 = L.HW64;
    ColDesc* d_desc = fm->build.coldesc.as<ColDesc>();
    if (src.kind != SeedKind::lines) {
        // pixels: an image becomes labels first (the seeds stage), and the tile kernel's sibling fills its bitmap tile from the labels
        const uint8_t* labels = P.pixels;
        fm->built.seeds_fused = src.kind == SeedKind::labels;
        if (src.kind == SeedKind::image) {
            const bool hyst = !src.edge_plain();  // (the scratch of an earlier build with hysteresis may still be there)
            // the image of the build's level: the caller's pixels, or its reduction in the handle's two level buffers
            uint8_t* pyr = fm->build.pyr.as<uint8_t>();
            const uint8_t* pixels = launch_pyramid(st, P.pixels, src.width0, src.height0, P.pixel_stride, src.level, pyr, pyr + L.pyr_b);
            launch_edge_labels(st, pixels, src.width, src.height, src.level > 0 ? src.width : P.pixel_stride, P.keys, m, src.edge, fm->build.labels.as<uint8_t>(),
                               hyst ? fm->build.edge_parent.as<int32_t>() : nullptr, hyst ? fm->build.edge_roots.as<uint32_t>() : nullptr);
            labels = fm->build.labels.as<uint8_t>();
            mark(fm, 1, fm->built.stage_events);
        }
        char* sp = (char*)fm->build.stack.p;
        launch_coldesc_labels(st, labels, src.width, src.height, src.border, d_desc, W, H, HW64, m, (unsigned*)fm->build.colmask.p,
                              device_proxy ? (int*)(sp + L.o_cost) : nullptr);
        if (device_proxy) launch_sweep_order(st, (const int*)(sp + L.o_cost), (int)L.nchunks, (int*)(sp + L.o_ord));
        return;
    }
    fm->built.seeds_fused = HW64 <= 64;
    if (fm->built.seeds_fused) {
        // the tile kernel rasterises the seeds of its columns itself (LDS): no bitmap, no k_seeds, no stage of its own
        const int XT = HW64 > 32 ? 32 : 64;
        const dim3 grid((unsigned)((W + XT - 1) / XT), (unsigned)m);
        const size_t lds = (size_t)HW64 * (XT + 1) * sizeof(uint4) + (size_t)HW64 * XT * 8;
        unsigned* cm = (unsigned*)fm->build.colmask.p;
        if (HW64 <= 16) hipLaunchKernelGGL((k_coldesc_tile<16, 64>), grid, dim3(256), lds, st, P.raster, P.slice_first, d_desc, W, H, HW64, cm);
        else if (HW64 <= 32) hipLaunchKernelGGL((k_coldesc_tile<32, 64>), grid, dim3(256), lds, st, P.raster, P.slice_first, d_desc, W, H, HW64, cm);
        else hipLaunchKernelGGL((k_coldesc_tile<64, 32>), grid, dim3(256), lds, st, P.raster, P.slice_first, d_desc, W, H, HW64, cm);
        return;
    }
    const long ncols = (long)m * W;
    unsigned long long* bitmap = fm->build.bitmap.as<unsigned long long>();
    FDCM_HIP(hipMemsetAsync(bitmap, 0, (size_t)ncols * HW64 * 8, st));
    if (P.n_raster > 0) hipLaunchKernelGGL(k_seeds, dim3((unsigned)P.n_raster), dim3(256), 0, st, P.raster, bitmap, W, H, HW64);
    mark(fm, 1, fm->built.stage_events);
    hipLaunchKernelGGL(k_coldesc, dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, st, bitmap, d_desc, W, HW64, ncols);
}
// the sweep: both 1-D passes of the distance transform, from the descriptors into `vol`
static void stage_sweep(fdcm_featuremap* fm, const BuildLayout& L, const SweepBuf& sb) {
    hipStream_t st = fm->stream;
    const int W = (int)fm->W, H = (int)fm->H, m = (int)fm->m, HW64 = L.HW64;
    const ColDesc* d_desc = fm->build.coldesc.as<ColDesc>();
    float* vol = fm->vol.as<float>();
    if (fm->distance == FDCM_L1) {
        // both L1 sweeps with one pass over the volume: minima per (row, word), their prefix / suffix over the row's words, then word by word
        const int nwords = (W + 63) / 64;
        const long wwaves = (long)m * HW64 * nwords, nrows = (long)m * HW64 * 64;
        float2* mins = (float2*)fm->build.stack.p;
        hipLaunchKernelGGL(k_l1_word_mins, dim3((unsigned)((wwaves + 3) / 4)), dim3(256), 0, st, d_desc, mins, W, HW64, nwords, wwaves);
        hipLaunchKernelGGL(k_l1_carries, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, mins, nwords, nrows);
        hipLaunchKernelGGL(k_l1_word, dim3((unsigned)((wwaves + 3) / 4)), dim3(256), 0, st, d_desc, (const float2*)mins, vol, W, H, HW64, nwords, wwaves);
    } else if (L.balanced) launch_sweep_balanced(st, d_desc, vol, W, H, HW64, L.nchunks, sb);
    else launch_sweep_literal(st, d_desc, vol, W, H, HW64, L.nchunks, fm->build.stack.p);
}
// orientation propagation, `vol` -> `ivol`, with L2's sqrt; a staged (test) build that stops at the transforms only takes the sqrt
static void stage_propagate(fdcm_featuremap* fm, const PlanOnDevice& P, bool transforms_only) {
    hipStream_t st = fm->stream;
    const int W = (int)fm->W, H = (int)fm->H, m = (int)fm->m;
    const size_t nq = ivol_slice_floats(W, H);
    float *vol = fm->vol.as<float>(), *ivol = fm->ivol.as<float>();
    const int apply_sqrt = fm->distance == FDCM_L2;
    if (transforms_only) {
        const size_t nel = (size_t)m * nq;  // (padding elements: harmless)
        if (apply_sqrt) hipLaunchKernelGGL(k_sqrt, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st, vol, nel);
        return;
    }
    const dim3 grid((unsigned)((nq + 255) / 256));
    switch (m) {  // the depths with a register kernel
#define FDCM_PROPAGATE(M) \
    case M: hipLaunchKernelGGL(k_propagate_reg<M>, grid, dim3(256), 0, st, (const float*)vol, ivol, W, H, P.prop, apply_sqrt); return;
        FDCM_PROPAGATE(30) FDCM_PROPAGATE(60) FDCM_PROPAGATE(90) FDCM_PROPAGATE(120) FDCM_PROPAGATE(180)
#undef FDCM_PROPAGATE
    }
    int bd = 256;
    while (bd > 64 && (size_t)m * bd * sizeof(float) > 64 * 1024) bd >>= 1;
    const size_t lds = (size_t)m * bd * sizeof(float);
    if (lds > 64 * 1024) FDCM_HIP(hipFuncSetAttribute((const void*)k_propagate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_propagate, dim3((unsigned)((nq + bd - 1) / bd)), dim3(bd), lds, st, (const float*)vol, ivol, W, H, m, P.prop, P.n_prop, apply_sqrt);
}
// line integral, `ivol` -> `vol`
static void stage_integral(fdcm_featuremap* fm, const PlanOnDevice& P) {
    hipStream_t st = fm->stream;
    const int W = (int)fm->W, H = (int)fm->H, m = (int)fm->m;
    const int chains = 2 * (W > H ? W : H), tab_stride = sh_tab_stride(W);
    int* d_tab = fm->build.offtab.as<int>();
    if (!(fm->groups.m == m && fm->groups.steps == W)) {  // the table only depends on the keys (fixed per handle) and the size
        hipLaunchKernelGGL(k_groups, dim3((unsigned)((tab_stride + 255) / 256), (unsigned)m), dim3(256), 0, st, P.integral, d_tab, W, tab_stride);
        fm->groups.m = m; fm->groups.steps = W;
    }
    const int shw = (long)m * ((chains + kShOwn - 1) / kShOwn) > 8192 ? 4 : 1;  // working waves per workgroup of a shallow slice
    // steep slices: 60 own chains per block while the launch is small, 124 / 252 once such blocks would outnumber
    // what the GPU holds several times over (fewer columns read twice; see integral_steep).
    const long narrow_blocks = (long)m * ((chains + 59) / 60), cus = device_cus(fm->device);
    const int xc = test_switches().int_xc ? test_switches().int_xc : (narrow_blocks > 64 * cus ? 256 : (narrow_blocks > 12 * cus ? 128 : 64));
    const dim3 igrid((unsigned)((chains + kShOwn - 1) / kShOwn), (unsigned)m);
    int kstride = 1;
    // slices are visited in a strided order (coprime to the depth, near half of it) so that steep and shallow ones
    // overlap -- once the blocks queue for the CUs (config 3: 4 260 blocks, 0.45 - 0.49 against 0.50 - 0.51 ms); a small
    // launch (config 2: 1 080 blocks, four per CU) is faster in index order (0.070 against 0.077 ms)
    const bool small_launch = (long)m * igrid.x <= 6L * cus;
    if (m > 2 && !small_launch) {
        auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
        kstride = m / 2 + 1;
        while (gcd(kstride, m) != 1) ++kstride;
    }
#define FDCM_INTEGRAL(XC)                                                                                                    \
    do {                                                                                                                     \
        constexpr size_t lds = integral_lds_bytes<XC>();                                                                     \
        static_assert(lds <= 160 * 1024, "tile pair must fit a CU's LDS");                                                   \
        if (lds > 64 * 1024)                                                                                                 \
            FDCM_HIP(hipFuncSetAttribute((const void*)k_integral<XC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL(k_integral<XC>, igrid, dim3(256), lds, st, (const float*)fm->ivol.as<float>(), fm->vol.as<float>(), \
                           W, H, P.integral, d_tab, shw, kstride);                                                           \
    } while (0)
    if (xc == 256) FDCM_INTEGRAL(256); else if (xc == 128) FDCM_INTEGRAL(128); else FDCM_INTEGRAL(64);
#undef FDCM_INTEGRAL
}

// FDCM_POISON: every buffer of the build, behind reserve_build and in front of the first command of run_build.  Three regions
// are state and stay while the handle's record says they are valid: the balanced sweep's per-chunk
// costs, its steal counter, and the line integral's group table.  A record that does not cover this build's shape leaves the
// region to the fill like the rest -- except a group table this build will not rewrite (it stops before the line integral):
// that one stays for the build its record names.  The records themselves are not touched.
static void poison_build(fdcm_featuremap* fm, const BuildLayout& L, int stop_after) {
    hipStream_t st = fm->stream;
    BuildBuffers& b = fm->build;
    FDCM_HIP(hipStreamSynchronize(st));  // (nothing queued still reads the pinned staging)
    poison_fill(fm->vol, st, FDCM_FILL_VOL); poison_fill(fm->ivol, st, FDCM_FILL_IVOL);
    poison_fill(b.bitmap, st, FDCM_FILL_BITMAP); poison_fill(b.coldesc, st, FDCM_FILL_COLDESC); poison_fill(b.colmask, st, FDCM_FILL_COLMASK);
    poison_fill(b.labels, st, FDCM_FILL_LABELS); poison_fill(b.edge_parent, st, FDCM_FILL_EDGE_PARENT);
    poison_fill(b.edge_roots, st, FDCM_FILL_EDGE_ROOTS); poison_fill(b.pyr, st, FDCM_FILL_PYR);
    const bool table_valid = fm->groups.m == (int)fm->m && fm->groups.steps == (int)fm->W;
    const bool table_of_another_build = fm->groups.m != 0 && stop_after < 3;
    if (!table_valid && !table_of_another_build) poison_fill(b.offtab, st, FDCM_FILL_OFFTAB);
    KeepRange keep[2];
    int n_keep = 0;
    if (L.balanced && fm->sweep.cost_chunks == L.nchunks && fm->sweep.cost_w == (int)fm->W) keep[n_keep++] = KeepRange{L.o_cost, L.o_cost + 4 * (size_t)L.nchunks};
    if (L.balanced && fm->sweep.steals_off == L.o_steals) keep[n_keep++] = KeepRange{L.o_steals, L.o_steals + 256};
    poison_fill(b.stack, st, FDCM_FILL_STACK, keep, n_keep);
    poison_fill(b.plan, st, FDCM_FILL_PLAN);
    poison_fill(b.stage, FDCM_FILL_BUILD_STAGE);
}

void run_build(fdcm_featuremap* fm, const BuildPlan& plan, int stop_after) {
    const auto t0 = std::chrono::steady_clock::now();
    const BuildLayout L = build_layout(plan, fm->distance, stop_after);
    reserve_build(fm, L);
    fm->W = plan.W; fm->H = plan.H; fm->m = plan.m; fm->tx = plan.tx; fm->ty = plan.ty; fm->keys = plan.keys;
    fm->pixel_seeded = plan.seeds.kind != SeedKind::lines;
    fm->last_build = fdcm_build_timing{}; fm->built.reset(); fm->holds = VolStage::none;
    if (L.empty) return;
    // FDCM_POISON (fdcm_internal.h, "the tests' switches"): the whole allocation of the volume, the columns and the rows of
    // padding included, and of every scratch buffer holds the word before the first stage writes; what the search reads
    // afterwards the build has written
    if (test_switches().poison) poison_build(fm, L, stop_after);
    SweepBuf sb{};
    std::vector<int32_t> proxy_cost;  // (stays empty unless the sweep's launch order takes it)
    bool device_proxy = false;        // the launch order's costs are counted by pass 1
    if (L.balanced) sb = setup_balanced_sweep(fm, L, plan, proxy_cost, device_proxy);
    else fm->sweep.reset();  // the L1 minima or the literal pass's scratch take the whole of `stack`
    const PlanOnDevice P = upload_plan(fm, L, plan, proxy_cost);
    BuildRecord& b = fm->built;
    b.host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    b.stage_events = fm->want_stage_events == 1;  // (an event between two kernels costs a blocking frame 3 - 5 us: fdcm_featuremap_stage_timing)
    b.total_events = fm->want_stage_events != 0;
    mark(fm, 0, b.total_events);
    stage_pass1(fm, L, P, plan.seeds, device_proxy);  // (event 1 behind its seeds, where they are a kernel of their own)
    mark(fm, 2, b.stage_events);
    stage_sweep(fm, L, sb);
    mark(fm, 3, b.stage_events);
    stage_propagate(fm, P, stop_after < 2);
    mark(fm, 4, b.stage_events);
    if (stop_after >= 3) stage_integral(fm, P);
    fm->holds = stop_after >= 3 ? VolStage::integrated : (stop_after == 2 ? VolStage::propagated : VolStage::transforms);
    mark(fm, 5, b.total_events);
    FDCM_HIP(hipGetLastError());
    b.pending = true;  // not waited for here: see finish_build
}

void finish_build(fdcm_featuremap* fm) {
    if (!fm->built.pending) return;
    fm->built.pending = false;
    FDCM_HIP(hipSetDevice(fm->device));
    FDCM_HIP(hipStreamSynchronize(fm->stream));
    hipEvent_t* ev = fm->timing.ev;
    fdcm_build_timing& bt = fm->last_build;
    if (fm->built.stage_events) {
        if (!fm->built.seeds_fused) FDCM_HIP(hipEventElapsedTime(&bt.seeds_ms, ev[0], ev[1]));  // (else 0: k_coldesc_tile draws them)
        FDCM_HIP(hipEventElapsedTime(&bt.pass1_ms, ev[fm->built.seeds_fused ? 0 : 1], ev[2]));
        FDCM_HIP(hipEventElapsedTime(&bt.pass2_ms, ev[2], ev[3]));
        FDCM_HIP(hipEventElapsedTime(&bt.propagate_ms, ev[3], ev[4]));
        FDCM_HIP(hipEventElapsedTime(&bt.integral_ms, ev[4], ev[5]));
    }
    if (fm->built.total_events) FDCM_HIP(hipEventElapsedTime(&bt.span_ms, ev[0], ev[5]));  // (0 without events: run_build cleared it)
    bt.total_ms = fm->built.host_ms + bt.span_ms;  // host preparation + the kernels' span on the device
}

}  // namespace fdcm
