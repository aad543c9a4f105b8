// fdcm_exhaustive.hip -- exhaustive search: the score of every template at every point of a translation grid (a dense
// chamfer score map), the k best grid points of every template, the peaks, and both over rotations (include/fdcm.h,
// "exhaustive search").  A score is evaluate<Dt3Cpu> (dt3cpu.cpp:126-179) at one translation: the bits
// fdcm_featuremap_evaluate returns there.
//
//   k_exhaustive<BUF32, MODE>         a workgroup takes a contiguous run of 16 x 64 sub-tiles of the grid (a portion) and a
//                                     chunk of kChunk templates; for every sub-tile it scores every template of the chunk (a
//                                     lane per 4 translations), then writes the scores (map), offers them to a running
//                                     k-best list per wave and template kept in LDS (top-k), or keeps per point the smallest
//                                     (normalised score, pair) key of the chunk and merges it into one plane of keys (best);
//                                     kBestBound: best for the points at or below a score, with rows_score's early exit;
//                                     kBestGate, kBestBoundGate: both with the matched-fraction gate inside the minimum
//   k_best_unpack, k_best_gather      best map: the key plane as row-major score and pair planes; the pairs of k points
//   k_nms_round<LIST, HULL, OBJ>      detections by footprint overlap: one round of the greedy rule, the previous round's
//                                     winner reduced from per-workgroup minima, its victims erased.  The one round of every
//                                     detection call: on G key planes or (LIST) on the winners' list of the windows' calls,
//                                     by boxes or (HULL) by hull shapes, and (OBJ) with one overlap limit within an object
//                                     and one across objects; six instantiations (nms_rounds)
//   k_exhaustive_peaks<R, ANGLES>     peaks: reads the score planes k_exhaustive<., false> wrote and offers every point whose
//                                     key is the minimum of its window to a per-wave k-best list; ANGLES: the window spans
//                                     several angles' planes (64-bit keys in LDS), else one plane (32-bit score bits)
//   k_exhaustive_merge_groups         one wave per template of a batch: its merged list so far and its units' lists
//   k_exhaustive_windows<BUF32>       pose windows: a wave takes a run of 4 x 16 patches of the clipped boxes of a batch's
//                                     (job, rotation) planes, a lane per translation, and keeps a k-best list per job
//   k_line_costs<BUF32>               line costs: a wave per pose, a lane per line of its template: the terms of the sum
//   k_matched_gate<BUF32>, k_matched_list<BUF32>, k_matched_fractions<BUF32>, k_matched_plane<BUF32>
//                                     matched fraction: a thread per point of the key plane (the gate before the rounds of
//                                     k_nms_round), per entry of the result list, per pose of a list, per grid point (the
//                                     gated best map's fractions); all through matched_length<BUF32>, the one statement of
//                                     the matched length for a pose on its own
//   k_window_winners<BUF32>, k_window_winners_objects<BUF32>
//                                     detections over pose windows: a thread per job turns the job's merged k = 1 list into
//                                     its entry of the winners' list (normalised key, footprint), for the list forms of
//                                     k_nms_round; objects (include/fdcm.h, "Objects"): the same pass with a threshold per pair
//   k_matches_verify<BUF32, CAP, OBJ>, k_matches_gather
//                                     match lists (include/fdcm.h, "Match lists"): a wave per record of search() turns it into
//                                     line costs, a score, a matched fraction, a box and a key for the list form of
//                                     k_nms_round; the gather writes the result records into pinned memory (at the file's end)
//   k_shape_rows<PHASE>, k_matches_shapes
//                                     match lists with hull shapes ("Match lists: objects and hull shapes"): the rows of every
//                                     candidate record by a scan, and a wave per record that wraps the hull of its posed end
//                                     points and writes its row spans and area, what hull_rows writes on the host
//   hull_suppresses, hull_stage       hull footprints (include/fdcm.h, "Hull footprints"): the overlap test on shapes, the
//                                     lattice points of the convex hull of a pair's end points as row spans, for template
//                                     sets of that kind; sets of kind BOX run the round's box forms
//
// Both scoring kernels evaluate through rows_score<BUF32, ROWS, CAP, EXIT, GATE>, the one statement of the sum (4 rows per lane
// in k_exhaustive, 1 in k_exhaustive_windows).  GATE: the matched length of every slot beside its sum, by matched_length's
// rule (include/fdcm.h, "Gate inside the minimum").  CAP: every term clamped to its line's cap (include/fdcm.h, "Per-line caps and
// line costs"); the kernels are instantiated both ways and a set without a finite cap launches the ones without the clamp,
// which are the code they were before caps existed.  On the host every call prepares its templates through prepare_pairs: the
// lines, bins and admissible box of (template, rotation) pairs, every pair of the set for the dense calls and the pairs a
// job list names for the pose windows; the drivers clip a pair's box to their grid (grid_range).
//
// Keys of the top-k are (score bits << 32) | grid index: scores are >= +0 (+inf included), so the key order is the
// (score, g) order, which is total -- the result does not depend on which wave saw which point first.  A NaN score has
// no key.  No atomics there.  The best map ("Best map and detections") is the one place with atomics: a 64-bit minimum per
// point across the workgroups of different template chunks, whose result does not depend on the order they arrive in.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <thread>
#include <type_traits>

#include "fdcm_internal.h"
#include "fdcm_score.h"

namespace fdcm {

namespace {

constexpr int kChunk = 8;                 // templates per workgroup
constexpr int kTileX = 16, kTileY = 64;   // a sub-tile: 4 waves x 4 columns (i) by 16 lanes x 4 rows (j) per wave
constexpr int kRows = kTileY / 16;        // translations per lane
constexpr int kMaxK = 64;
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kMaxCoord = (1 << 24) - 1;  // valid translations: |t| < 2^24

struct ExLine {  // one template line: end points, the line's slice (bin * floats per slice, or the bin: see VolRef), its cap
    float x1, y1, x2, y2;
    int se;
    float cap;  // +inf: none
    float len;  // its template line's length (P.len's float): read by the gated forms of rows_score alone
    int pad;
};
static_assert(sizeof(ExLine) == 32, "ExLine is 32 bytes");

// One term of the sum: |a - b|, clamped to the line's cap when CAP.  A compare and a select, not fminf: a NaN term stays NaN.
template <bool CAP>
__device__ __forceinline__ float line_term(float a, float b, float cap) {
    const float v = f_abs(a - b);
    return CAP && v > cap ? cap : v;
}
// The matched length after one more line (include/fdcm.h, "Gate inside the minimum"): matched_length's compare, on the
// uncapped term, and its add.  A NaN term is not matched.
__device__ __forceinline__ float line_matched(float ml, float a, float b, float cap, float len) {
    return f_abs(a - b) <= cap ? ml + len : ml;
}
struct ExTmpl {    // one template of a launch
    int line0, n;  // its lines in the line array
    int i0, i1, j0, j1;  // grid indices of its admissible translations: [i0, i1] x [j0, j1] (empty when i0 > i1 or j0 > j1)
    int slot;            // where its output goes: map plane / candidate lists
    unsigned koff;       // added to the grid index of its keys (a rotation's a * nx * ny; 0 otherwise); best map: the
                         // bits of the float32 its scores are divided by
};
// kBestGate, kBestBoundGate: kBest and kBestBound with the matched-fraction gate inside the minimum ("Gate inside the minimum")
enum ExMode { kMap = 0, kTopK = 1, kBest = 2, kBestBound = 3, kBestGate = 4, kBestBoundGate = 5 };
constexpr bool ex_bound(int mode) { return mode == kBestBound || mode == kBestBoundGate; }
constexpr bool ex_gate(int mode) { return mode == kBestGate || mode == kBestBoundGate; }
// k_exhaustive's last argument: nothing, (BOUND) the pairs' exit bounds and the threshold on q, (GATE) the pairs' needs
template <bool BOUND, bool GATE = false>
struct ExBound {};
template <>
struct ExBound<true, false> {
    const float* bc;
    float max_score;
};
template <>
struct ExBound<false, true> {
    const float* need;
};
template <>
struct ExBound<true, true> {
    const float* bc;
    float max_score;
    const float* need;
};
template <bool GATE>
__device__ __forceinline__ bool under(float, const ExBound<false, GATE>&) { return true; }
template <bool GATE>
__device__ __forceinline__ bool under(float q, const ExBound<true, GATE>& b) { return q <= b.max_score; }

// Best map: where the key of grid point (i, j) lies in the key plane.  The plane is kept in the order k_exhaustive walks
// it, sub-tile by sub-tile and inside one [row group j / 16][wave][lane], so the 64 keys a wave merges at once are 512
// contiguous bytes.
__device__ __forceinline__ long long best_key_index(int i, int j, int tiles_x) {
    const int ti = i / kTileX, tj = j / kTileY, li = i % kTileX, lj = j % kTileY;
    return ((long long)tj * tiles_x + ti) * (kTileX * kTileY) + (lj / 16) * 256 + (li / 4) * 64 + (lj % 16) * 4 + (li % 4);
}
// best_key_index backwards, the one statement of it: 1024 keys per sub-tile, [row group][wave][row % 16][column % 4].
__device__ __forceinline__ void best_key_point(long long idx, int tiles_x, int& i, int& j) {
    const int tile = (int)(idx >> 10), r = (int)(idx & 1023);
    i = (tile % tiles_x) * kTileX + ((r >> 6) & 3) * 4 + (r & 3);
    j = (tile / tiles_x) * kTileY + (r >> 8) * 16 + ((r >> 2) & 15);
}

// One read of the interleaved volume (ivol_index) at column x, row y of the line's slice.  xw: the column's part of the
// element index (with the slice) from ex_column.  The 64-bit form clamps to the slice: its translations are admissible,
// so the clamp never changes a value -- it only keeps a wrong interval from reading outside the volume (the 32-bit
// form's buffer descriptor returns 0 outside it).
template <bool BUF32>
__device__ __forceinline__ size_t ex_column(int x, int se, int W, unsigned H, size_t SL) {
    if (BUF32) return (size_t)((((__umul24((unsigned)x >> 2, H)) << 2) | ((unsigned)x & 3u)) + (unsigned)se);
    x = min(max(x, 0), W - 1);
    return (size_t)se * SL + (size_t)((unsigned)x >> 2) * H * 4 + (unsigned)(x & 3);
}
template <bool BUF32>
__device__ __forceinline__ float ex_read(const VolRef& V, size_t xw, int y, unsigned H) {
    if (BUF32) return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(V.rs, ((unsigned)xw + ((unsigned)y << 2)) << 2, 0, 0));
    y = min(max(y, 0), (int)H - 1);
    return V.vol[xw + (size_t)y * 4];
}

// The wave's sorted list of its k best keys, lane l holding entry l; insert key K (< entry k - 1).
__device__ __forceinline__ unsigned long long list_insert(unsigned long long e, unsigned long long K, int lane) {
    const int pos = __popcll(__ballot(e < K));
    const unsigned long long up = __shfl_up(e, 1);
    return lane > pos ? up : (lane == pos ? K : e);
}
__device__ __forceinline__ unsigned long long read_lane64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
// Offers one key per lane (kNoKey: none) to the list e with threshold thr = entry k - 1; returns the new threshold.
__device__ __forceinline__ unsigned long long list_offer(unsigned long long& e, unsigned long long key, unsigned long long thr,
                                                         int k, int lane) {
    unsigned long long mask = __ballot(key < thr);
    while (mask) {  // wave-uniform
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const unsigned long long K = read_lane64(key, src);
        if (K < thr) {
            e = list_insert(e, K, lane);
            thr = read_lane64(e, k - 1);
        }
    }
    return thr;
}

// evaluate at ROWS translations of one column per lane, rows offy[r]: score_per_line.sum(), dt3cpu.cpp:175, in Eigen
// 3.4.0's order (as pair_score, fdcm_score.h): packets p0 = lines 8b..8b+3 and p1 = 8b+4..8b+7 summed over the blocks of
// 8, p0 += p1, the trailing packet, predux (p0[0] + p0[2]) + (p0[1] + p0[3]), then the scalar tail.  Zero-initialised
// accumulators give the same bits (0 + v == v for v >= +0), so one code path serves every n.  The one statement of the
// sum for every kernel of this file.  res: zero on entry (the caller's initialiser: zeroing it here costs k_exhaustive
// registers).  CAP: term i is line_term's clamp of it to Lt[i].cap.
//
// EXIT (detections below a score): after a block of 8 and after the trailing packet, when lines remain,
// the wave abandons the sum -- true is returned and res means nothing -- if every one of its 64 x ROWS slots is masked
// (!act[r]) or proved over the bound: C > bc, C the float32 sum of the slot's accumulators so far.  Terms are >= +0 or NaN,
// so the finished sum of such a slot would be above bc (1 - 2 n u), u = 2^-24, or NaN; the host chose bc for that to mean
// "no key".  A NaN C fails the comparison and the slot scores on.  One __ballot, wave-uniform.  Without EXIT: false.
template <int ROWS, bool TWO>
__device__ __forceinline__ bool rows_over(const float (&p0)[ROWS][4], const float (&p1)[ROWS][4], const bool* act, float bc) {
    bool live = false;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const float C = TWO ? ((p0[r][0] + p1[r][0]) + (p0[r][1] + p1[r][1])) + ((p0[r][2] + p1[r][2]) + (p0[r][3] + p1[r][3]))
                            : (p0[r][0] + p0[r][2]) + (p0[r][1] + p0[r][3]);
        live = live || (act[r] && !(C > bc));
    }
    return __ballot(live) == 0;
}

//
// GATE (include/fdcm.h, "Gate inside the minimum"): beside the sum, ml[r] (zero on entry, as res) becomes ML of the slot, the
// matched length by matched_length's rule: after the loads of a block, of the trailing packet and of each tail line the
// lines are walked in line order, one line_matched each, so the float32 sum is sequential from +0 whatever the score's
// own order.  The score's sum is untouched.  A wave that leaves through EXIT leaves ml without meaning, as res.
template <bool BUF32, int ROWS, bool CAP, bool EXIT = false, bool GATE = false>
__device__ __forceinline__ bool rows_score(const VolRef& V, const ExLine* __restrict__ Lt, int n, float offx, const float (&offy)[ROWS],
                                           int W, unsigned uH, size_t SL, float (&res)[ROWS], const bool* act = nullptr,
                                           float bc = 0.f, float* ml = nullptr) {
    const int aligned2 = (n / 8) * 8, aligned = (n / 4) * 4;
    float p0[ROWS][4], p1[ROWS][4];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int l = 0; l < 4; ++l) p0[r][l] = p1[r][l] = 0.f;
    bool gone = false;  // (EXIT) part of the loop's condition, so the loop keeps its one block and its one way out
    for (int b = 0; b < aligned2 && !(EXIT && gone); b += 8) {
        float va[8][ROWS], vb[8][ROWS], cp[8], ll[GATE ? 8 : 1];
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const ExLine ln = Lt[b + l];
            cp[l] = ln.cap;
            if constexpr (GATE) ll[l] = ln.len;
            const size_t c1 = ex_column<BUF32>((int)(ln.x1 + offx), ln.se, W, uH, SL);
            const size_t c2 = ex_column<BUF32>((int)(ln.x2 + offx), ln.se, W, uH, SL);
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {  // translate then cast<int>()
                va[l][r] = ex_read<BUF32>(V, c1, (int)(ln.y1 + offy[r]), uH);
                vb[l][r] = ex_read<BUF32>(V, c2, (int)(ln.y2 + offy[r]), uH);
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                p0[r][l] = p0[r][l] + line_term<CAP>(va[l][r], vb[l][r], cp[l]);
                p1[r][l] = p1[r][l] + line_term<CAP>(va[l + 4][r], vb[l + 4][r], cp[l + 4]);
            }
        if constexpr (GATE) {
#pragma unroll
            for (int l = 0; l < 8; ++l)
#pragma unroll
                for (int r = 0; r < ROWS; ++r) ml[r] = line_matched(ml[r], va[l][r], vb[l][r], cp[l], ll[l]);
        }
        if constexpr (EXIT) gone = b + 8 < n && rows_over<ROWS, true>(p0, p1, act, bc);
    }
    if (EXIT && gone) return true;
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int l = 0; l < 4; ++l) p0[r][l] = p0[r][l] + p1[r][l];
    if (aligned > aligned2) {  // the trailing packet
        float va[4][ROWS], vb[4][ROWS], cp[4], ll[GATE ? 4 : 1];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const ExLine ln = Lt[aligned2 + l];
            cp[l] = ln.cap;
            if constexpr (GATE) ll[l] = ln.len;
            const size_t c1 = ex_column<BUF32>((int)(ln.x1 + offx), ln.se, W, uH, SL);
            const size_t c2 = ex_column<BUF32>((int)(ln.x2 + offx), ln.se, W, uH, SL);
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                va[l][r] = ex_read<BUF32>(V, c1, (int)(ln.y1 + offy[r]), uH);
                vb[l][r] = ex_read<BUF32>(V, c2, (int)(ln.y2 + offy[r]), uH);
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int l = 0; l < 4; ++l) p0[r][l] = p0[r][l] + line_term<CAP>(va[l][r], vb[l][r], cp[l]);
        if constexpr (GATE) {
#pragma unroll
            for (int l = 0; l < 4; ++l)
#pragma unroll
                for (int r = 0; r < ROWS; ++r) ml[r] = line_matched(ml[r], va[l][r], vb[l][r], cp[l], ll[l]);
        }
        if constexpr (EXIT)
            if (aligned < n && rows_over<ROWS, false>(p0, p1, act, bc)) return true;
    }
    if (aligned)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) res[r] = (p0[r][0] + p0[r][2]) + (p0[r][1] + p0[r][3]);  // predux
    for (int idx = aligned; idx < n; ++idx) {  // the scalar tail, in order
        const ExLine ln = Lt[idx];
        const size_t c1 = ex_column<BUF32>((int)(ln.x1 + offx), ln.se, W, uH, SL);
        const size_t c2 = ex_column<BUF32>((int)(ln.x2 + offx), ln.se, W, uH, SL);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if constexpr (GATE) {
                const float a = ex_read<BUF32>(V, c1, (int)(ln.y1 + offy[r]), uH), b = ex_read<BUF32>(V, c2, (int)(ln.y2 + offy[r]), uH);
                res[r] = res[r] + line_term<CAP>(a, b, ln.cap);
                ml[r] = line_matched(ml[r], a, b, ln.cap, ln.len);
            } else {
                res[r] = res[r] + line_term<CAP>(ex_read<BUF32>(V, c1, (int)(ln.y1 + offy[r]), uH), ex_read<BUF32>(V, c2, (int)(ln.y2 + offy[r]), uH), ln.cap);
            }
        }
    }
    return false;
}

// MODE kBestBound (include/fdcm.h, "All detections below a score") is kBest with a threshold: a point's key enters the plane
// only when q <= bound.max_score, and rows_score may abandon a template for the sub-tile (its EXIT) against bound.bc[slot],
// the pair's bound.  The other modes take an empty argument in bound's place and are the code they were without it.
// MODE kBestGate / kBestBoundGate (include/fdcm.h, "Gate inside the minimum"): kBest / kBestBound whose keys enter bk only when
// the slot's ML, from rows_score's GATE, is >= bound.need[slot], the pair's need.  The exit stays as it is: a slot proved
// over its score bound is no candidate under any gate.
template <bool BUF32, int MODE, bool CAP>
__global__ void __launch_bounds__(256) k_exhaustive(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx,
                                                    float ty, const ExLine* __restrict__ lines, const ExTmpl* __restrict__ tm,
                                                    int T, int x0, int y0, int nx, int ny, int sx, int sy, int tiles_x,
                                                    int n_subtiles, int portions, int k, float* __restrict__ map,
                                                    long long plane, unsigned long long* __restrict__ cand,
                                                    ExBound<ex_bound(MODE), ex_gate(MODE)> bound) {
    constexpr bool BOUND = ex_bound(MODE), GATE = ex_gate(MODE);
    constexpr bool TOPK = MODE == kTopK, BEST = MODE == kBest || BOUND || GATE;
    __shared__ unsigned long long lists[TOPK ? 4 * kChunk * kMaxK : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // Workgroup b -> (portion, template chunk).  Workgroups are observed to be dealt round-robin over the 8 XCDs (b and
    // b + 8 share one): all chunks of portion p go to one XCD, next to each other in dispatch order, so they walk the same
    // sub-tiles together and read one window of the volume through that XCD's L2.  Placement only affects speed.
    const int n_chunks = (T + kChunk - 1) / kChunk;
    const int r = (int)blockIdx.x / 8;
    const int chunk = r % n_chunks, portion = (r / n_chunks) * 8 + (int)blockIdx.x % 8;
    const int t_first = chunk * kChunk, t_end = min(T, t_first + kChunk);
    const VolRef V = make_volref(vol, SL, m, BUF32);
    const unsigned uH = (unsigned)H;
    unsigned long long* L = lists + (TOPK ? wave * kChunk * kMaxK : 0);
    if (TOPK)
        for (int c = 0; c < kChunk; ++c) L[c * kMaxK + lane] = kNoKey;  // each wave owns its lists: no barrier

    // a portion is a contiguous run of sub-tiles (row-major): the next sub-tile's window overlaps the last one's
    const int s_begin = (int)((long long)n_subtiles * portion / portions);
    const int s_end = (int)((long long)n_subtiles * (portion + 1) / portions);
    for (int s = s_begin; s < s_end; ++s) {
        const int ti = s % tiles_x, tj = s / tiles_x;
        const int i = ti * kTileX + wave * 4 + (lane & 3);
        const int jb = tj * kTileY + (lane >> 2);
        const int tile_i0 = ti * kTileX, tile_j0 = tj * kTileY;
        unsigned long long bk[kRows] = {kNoKey, kNoKey, kNoKey, kNoKey};  // (best) the chunk's smallest key per point
        for (int t = t_first; t < t_end; ++t) {
            const ExTmpl P = tm[t];
            // the sub-tile against the template's admissible box (all wave-uniform)
            const bool meets = P.i0 <= P.i1 && P.j0 <= P.j1 && P.i0 < tile_i0 + kTileX && P.i1 >= tile_i0 &&
                               P.j0 < tile_j0 + kTileY && P.j1 >= tile_j0;
            if ((TOPK || BEST) && !meets) continue;
            bool act[kRows];
            float offy[kRows];
            // translate(tmpl, sceneTranslation + translation), dt3cpu.cpp:153.  A translation outside the box is
            // replaced by the box's first corner, which is admissible: every read stays inside the volume
            const bool act_i = i >= P.i0 && i <= P.i1;
            const float offx = tx + (float)(x0 + (act_i ? i : P.i0) * sx);
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const int j = jb + 16 * r;
                act[r] = act_i && j >= P.j0 && j <= P.j1;
                offy[r] = ty + (float)(y0 + (act[r] ? j : P.j0) * sy);
            }
            float res[kRows] = {0.f, 0.f, 0.f, 0.f};
            float ml[GATE ? kRows : 1] = {};
            if constexpr (BOUND && GATE) {
                if (rows_score<BUF32, kRows, CAP, true, true>(V, lines + P.line0, P.n, offx, offy, W, uH, SL, res, act, bound.bc[P.slot], ml)) continue;
            } else if constexpr (GATE) {
                rows_score<BUF32, kRows, CAP, false, true>(V, lines + P.line0, P.n, offx, offy, W, uH, SL, res, nullptr, 0.f, ml);
            } else if constexpr (BOUND) {  // (meets: a sub-tile that does not was skipped above)
                if (rows_score<BUF32, kRows, CAP, true>(V, lines + P.line0, P.n, offx, offy, W, uH, SL, res, act, bound.bc[P.slot])) continue;
            } else {
                if (meets) rows_score<BUF32, kRows, CAP>(V, lines + P.line0, P.n, offx, offy, W, uH, SL, res);
            }
            if (BEST) {
                // q = score / the template's denominator, one IEEE division; pairkey = (bits of q << 32) | pair.  q >= +0
                // or NaN, so the key order is (q, pair); a NaN q is no candidate
                const float den = __uint_as_float(P.koff);
                float need = 0.f;
                if constexpr (GATE) need = bound.need[P.slot];
#pragma unroll
                for (int r = 0; r < kRows; ++r) {
                    const float q = res[r] / den;
                    bool cand_r = act[r] && !(q != q) && under(q, bound);
                    if constexpr (GATE) cand_r = cand_r && ml[r] >= need;
                    if (cand_r) bk[r] = min(bk[r], ((unsigned long long)__float_as_uint(q) << 32) | (unsigned)P.slot);
                }
            } else if (!TOPK) {
                if (i < nx) {
                    float* out = map + (long long)P.slot * plane;
#pragma unroll
                    for (int r = 0; r < kRows; ++r) {
                        const int j = jb + 16 * r;
                        if (j < ny) out[(long long)j * nx + i] = act[r] ? res[r] : f_nan();
                    }
                }
            } else {
                unsigned long long* Lc = L + (t - t_first) * kMaxK;
                unsigned long long thr = Lc[k - 1];
                unsigned long long key[kRows];
                bool any = false;
#pragma unroll
                for (int r = 0; r < kRows; ++r) {
                    // a NaN score (NaN or inf - inf in the volume's data) has no key, as in the peaks kernel
                    key[r] = act[r] && !(res[r] != res[r]) ? ((unsigned long long)__float_as_uint(res[r]) << 32) |
                                          ((unsigned)((jb + 16 * r) * nx + i) + P.koff)
                                    : kNoKey;
                    any = any || key[r] < thr;
                }
                if (__ballot(any)) {  // rare once the list has filled: the k-th best only falls
                    unsigned long long e = Lc[lane];
#pragma unroll
                    for (int r = 0; r < kRows; ++r) thr = list_offer(e, key[r], thr, k, lane);
                    Lc[lane] = e;
                }
            }
        }
        if (BEST) {
            // The minimum across the workgroups that meet at this sub-tile (other chunks, other launches of the call): a
            // 64-bit atomic minimum at agent scope.  The plain load before it may be stale, but keys only fall, so a key
            // that does not beat it cannot beat the current one either.  The plane holds whole sub-tiles.
            unsigned long long* kp = cand + (long long)s * (kTileX * kTileY) + threadIdx.x;
#pragma unroll
            for (int r = 0; r < kRows; ++r)
                if (bk[r] < kp[r * 256]) atomicMin(kp + r * 256, bk[r]);
        }
    }
    if (TOPK) {
        // candidate lists: [slot][blockIdx.x * 4 + wave][k]
        const long long n_lists = (long long)portions * 4;
        for (int t = t_first; t < t_end; ++t) {
            const unsigned long long v = L[(t - t_first) * kMaxK + lane];
            if (lane < k) cand[((long long)tm[t].slot * n_lists + portion * 4 + wave) * k + lane] = v;
        }
    }
}

// Peaks (include/fdcm.h, "peaks" and "Rotations"): a point is a peak when its key (score bits << 32) | (a N + g) is the
// minimum of the keys in its window, a box of (2ra+1) x (2ry+1) x (2rx+1) over (angle, row, column), so the minimum is
// separable: angle first, then rows, then columns.  A workgroup takes tiles of kPkTX x kPkTY points of one decided
// (template, angle) unit and loads each with its rx / ry halo into LDS:
//   ANGLES   already reduced over the angle window: per halo point the smallest key over the planes of the angles
//            a - ra .. a + ra (circular when wrap is set; angles outside [0, n_rot) otherwise ignored), kNoKey where none
//            is admissible (NaN).  The planes of a group (one template's angles lo, lo + 1, ... of the batch, mod n_rot)
//            are consecutive: the plane of angle a' is D.x + ((a' - lo) mod n_rot).
//   !ANGLES  the window holds the unit's own plane alone: its score bits, kPkNone for no key (outside the plane or the
//            template's box, or NaN).  Every key of the window has the same angle term, so the score bits and the column
//            order the row's keys: the row pass keeps the first column of the smallest bits.
// Row pass: per halo row and tile column the minimum key of the row's 2rx+1 window.  Column pass: per tile point the
// minimum of the 2ry+1 row minima; the point is a peak when that is its own key.  Peaks go to the wave's sorted k-best
// list (registers, lane l holding entry l) with list_offer; k_exhaustive_merge_groups folds the lists.  R: the largest
// radius the LDS is sized for: (4 or 8) kH kW + 8 kH kPkTX bytes.
constexpr int kPkTX = 64, kPkTY = 32;  // tile: a wave per row, kPkTY / 4 rows per wave
constexpr unsigned kPkNone = ~0u;      // no key: above the bits of every score >= +0 (NaN included)
constexpr int kMaxRadius = 32;
constexpr int kPeakWorkgroups = 2048;  // peak workgroups of a launch, about: parts per unit

template <int R, bool ANGLES>
__global__ void __launch_bounds__(256) k_exhaustive_peaks(const float* __restrict__ map, int w, int h, const ExTmpl* __restrict__ pl,
                                                          const int4* __restrict__ dec, int parts, int rx, int ry, int ra, int n_rot,
                                                          int wrap, int di0, int di1, int dj0, int dj1, int ia, int ja, int nx,
                                                          unsigned N, int k, unsigned long long* __restrict__ cand) {
    using Key = typename std::conditional<ANGLES, unsigned long long, unsigned>::type;
    constexpr int kW = kPkTX + 2 * R, kH = kPkTY + 2 * R;
    __shared__ Key S[kH * kW];                    // score bits (ANGLES: angle-window minimum keys) of the tile and halo
    __shared__ unsigned long long B[kH * kPkTX];  // row-window minimum keys
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = (int)blockIdx.x / parts, part = (int)blockIdx.x % parts;
    // x: the group's first plane, y: its first angle lo, z: its planes, w: the unit's angle
    const int4 D = ANGLES ? dec[u] : make_int4(0, 0, 0, 0);
    const long long wh = (long long)w * h;
    auto plane_of = [&](int a2) {
        const int o = a2 - D.y;
        return D.x + (o < 0 ? o + n_rot : o);
    };
    const ExTmpl P = pl[ANGLES ? plane_of(D.w) : u];  // one plane per window: the batch's units are its planes
    const float* own = map + (long long)P.slot * wh;
    const unsigned akey = ANGLES ? (unsigned)D.w * N : P.koff;  // a N
    const int W2 = kPkTX + 2 * rx, H2 = kPkTY + 2 * ry;
    // the points this launch decides for the unit: its box (plane coordinates) within the decision rectangle
    const int bi0 = max(P.i0, di0), bi1 = min(P.i1, di1), bj0 = max(P.j0, dj0), bj1 = min(P.j1, dj1);
    const int ntx = bi0 <= bi1 ? (bi1 - bi0) / kPkTX + 1 : 0, nty = bj0 <= bj1 ? (bj1 - bj0) / kPkTY + 1 : 0;
    unsigned long long e = kNoKey, thr = kNoKey;
    for (int tile = part; tile < ntx * nty; tile += parts) {  // workgroup-uniform
        const int li0 = bi0 + (tile % ntx) * kPkTX, lj0 = bj0 + (tile / ntx) * kPkTY;
        for (int idx = threadIdx.x; idx < H2 * W2; idx += 256) {
            const int hr = idx / W2, hc = idx - hr * W2;
            const int li = li0 - rx + hc, lj = lj0 - ry + hr;
            Key v = (Key)kNoKey;
            if constexpr (ANGLES) {
                if (li >= 0 && li < w && lj >= 0 && lj < h) {  // every plane of the launch covers the region's plane
                    const unsigned g = (unsigned)(ja + lj) * (unsigned)nx + (unsigned)(ia + li);
                    const long long off = (long long)lj * w + li;
                    for (int d = -ra; d <= ra; ++d) {
                        int a2 = D.w + d;
                        if (a2 < 0 || a2 >= n_rot) {
                            if (!wrap) continue;
                            a2 = (a2 % n_rot + n_rot) % n_rot;
                        }
                        const float s = map[(long long)plane_of(a2) * wh + off];
                        if (!(s != s)) v = min(v, ((unsigned long long)__float_as_uint(s) << 32) | ((unsigned)a2 * N + g));
                    }
                }
            } else if (li >= P.i0 && li <= P.i1 && lj >= P.j0 && lj <= P.j1) {  // the box lies inside the plane
                const float s = own[(long long)lj * w + li];
                if (!(s != s)) v = __float_as_uint(s);
            }
            S[hr * kW + hc] = v;
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < H2 * kPkTX; idx += 256) {
            const int hr = idx / kPkTX, c = idx % kPkTX;
            const Key* row = S + hr * kW + c;
            Key best = row[0];
            int at = 0;
            for (int d = 1; d <= 2 * rx; ++d) {
                const Key v = row[d];
                if (v < best) { best = v; at = d; }
            }
            if constexpr (ANGLES) {
                B[hr * kPkTX + c] = best;
            } else {
                const unsigned g = akey + (unsigned)(ja + lj0 - ry + hr) * (unsigned)nx + (unsigned)(ia + li0 - rx + c + at);
                B[hr * kPkTX + c] = best == kPkNone ? kNoKey : ((unsigned long long)best << 32) | g;
            }
        }
        __syncthreads();
        for (int r = wave; r < kPkTY; r += 4) {  // wave-uniform: every lane takes part in list_offer
            const int li = li0 + lane, lj = lj0 + r;
            unsigned long long m = kNoKey;
            for (int d = 0; d <= 2 * ry; ++d) m = min(m, B[(r + d) * kPkTX + lane]);
            // the point's own key, from its score bits
            auto own_key = [&](unsigned s) {
                return ((unsigned long long)s << 32) | (akey + (unsigned)(ja + lj) * (unsigned)nx + (unsigned)(ia + li));
            };
            unsigned long long key = kNoKey;
            if constexpr (ANGLES) {  // the score from the unit's plane
                if (li <= bi1 && lj <= bj1) {
                    const float s = own[(long long)lj * w + li];
                    if (!(s != s)) {
                        const unsigned long long k3 = own_key(__float_as_uint(s));
                        if (k3 == m) key = k3;
                    }
                }
            } else {  // the score bits in LDS
                const unsigned s = S[(r + ry) * kW + rx + lane];
                if (s != kPkNone && li <= bi1 && lj <= bj1) {
                    const unsigned long long k2 = own_key(s);
                    if (k2 == m) key = k2;
                }
            }
            thr = list_offer(e, key, thr, k, lane);
        }
        __syncthreads();  // the next tile overwrites S and B
    }
    // candidate lists: [u][part * 4 + wave][k], 4 * parts per unit
    if (lane < k) cand[((long long)u * 4 * parts + part * 4 + wave) * k + lane] = e;
}

// One wave per group (one template's units of a batch): its merged list so far best[q] and the group's units * lpu
// candidate lists, from list unit0 * lpu on, folded into best[q].  seg: x unit0, y units, z q.
__global__ void __launch_bounds__(256) k_exhaustive_merge_groups(const unsigned long long* __restrict__ cand, const int4* __restrict__ seg,
                                                                 int n_groups, int lpu, int k, unsigned long long* __restrict__ best) {
    const int lane = threadIdx.x & 63;
    const int gi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= n_groups) return;  // wave-uniform
    const int4 G = seg[gi];
    unsigned long long* b = best + (long long)G.z * k;
    unsigned long long e = kNoKey, thr = kNoKey;
    thr = list_offer(e, lane < k ? b[lane] : kNoKey, thr, k, lane);
    const unsigned long long* c = cand + (long long)G.x * lpu * k;
    const long long n_lists = (long long)G.y * lpu;
    for (long long q = 0; q < n_lists; ++q) thr = list_offer(e, lane < k ? c[q * k + lane] : kNoKey, thr, k, lane);
    if (lane < k) b[lane] = e;
}

// ---- best map (include/fdcm.h, "Best map and detections")
// The key plane k_exhaustive<., kBest> merged (best_key_index's order) as row-major planes of the grid: the normalised
// score, NaN where no pair has a key, and the pair, -1 there.  Either output may be null.
__global__ void __launch_bounds__(256) k_best_unpack(const unsigned long long* __restrict__ keys, int nx, int ny, int tiles_x,
                                                     float* __restrict__ score, int* __restrict__ pair) {
    const int i = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), j = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (i >= nx || j >= ny) return;
    const unsigned long long v = keys[best_key_index(i, j, tiles_x)];
    const long long g = (long long)j * nx + i;
    if (score) score[g] = v == kNoKey ? f_nan() : __uint_as_float((unsigned)(v >> 32));
    if (pair) pair[g] = v == kNoKey ? -1 : (int)(unsigned)v;
}

// The pairs of the detections: best[l] is a key (score bits << 32) | g of the merged list, kNoKey from its end on.
__global__ void k_best_gather(const unsigned long long* __restrict__ best, int k, const unsigned long long* __restrict__ keys, int nx,
                              int tiles_x, int* __restrict__ pair) {
    const int l = threadIdx.x;
    if (l >= k) return;
    const unsigned long long v = best[l];
    if (v == kNoKey) { pair[l] = -1; return; }
    const unsigned g = (unsigned)v;
    pair[l] = (int)(unsigned)keys[best_key_index((int)(g % (unsigned)nx), (int)(g / (unsigned)nx), tiles_x)];
}

// ---- detections by footprint overlap (include/fdcm.h, "Detections suppressed by footprint overlap")
// The greedy rule on the key plane k_exhaustive<., kBest> merged, one launch per round, k + 1 launches on one stream and no
// host round trip between them.  A launch has at most kNmsWorkgroups workgroups; workgroup b owns a contiguous run of the
// plane in storage order and leaves its partial minimum, a key (bits of q << 32) | g and the pair of that point, in entry
// b of the arrays of this round (two sets, used in turn).  Round r:
//   1. every workgroup reduces the partials of round r - 1 to the same winner d(r-1), key and pair (round 0: none)
//   2. workgroup 0 writes them to the result list; a winner kNoKey ends the list: the workgroups leave kNoKey partials
//      behind (the next launches read them) and return.  The last launch (r = k) returns here too: it only reduces.
//   3. each workgroup walks its run, consecutive lanes reading consecutive keys: (i, j) from the storage index
//      (best_key_point), the point's footprint from its pair's box and its translation; the winner's once per workgroup
//   4. the winner and every point it suppresses (1000 I > permille U, int64) become kNoKey, a plain store by the one
//      thread that owns the entry in every round; each surviving key enters the workgroup's minimum as (q bits << 32) | g
// The pair travels with the partial because the winner's entry of the plane is erased in the launch that needs its box.
// A minimum does not depend on the order of its operands and suppression is a function of d(r-1) alone: no atomics, no
// cooperative launch, and the bytes do not depend on scheduling.  The launch is k_nms_round<LIST, HULL, OBJ>, below the
// overlap tests; what follows here is what it is made of.
constexpr int kNmsWorkgroups = 256;

// The minimum key of the workgroup and its pair, in every thread.  sk, sp: 4 entries of LDS, free on entry.
__device__ __forceinline__ void nms_block_min(unsigned long long& key, int& pair, unsigned long long* sk, int* sp) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long k2 = __shfl_xor(key, d);
        const int p2 = __shfl_xor(pair, d);
        if (k2 < key) { key = k2; pair = p2; }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sk[wave] = key; sp[wave] = pair; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (sk[w] < key) { key = sk[w]; pair = sp[w]; }
    __syncthreads();  // sk and sp are free again
}

// The same for partials that are keys alone (the list forms of the round): no pair is reduced.
__device__ __forceinline__ void nms_block_min(unsigned long long& key, unsigned long long* sk) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) key = min(key, __shfl_xor(key, d));
    if ((threadIdx.x & 63) == 0) sk[threadIdx.x >> 6] = key;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) key = min(key, sk[w]);
    __syncthreads();  // sk is free again
}

// The overlap test, the one statement of it: the footprint [fx0, fx1] x [fy0, fy1] against the winner's, whose area is Aw.
// 1000 I > permille U in int64, U = A + Aw - I; boxes that share no pixel never suppress each other.
__device__ __forceinline__ bool nms_suppresses(int fx0, int fy0, int fx1, int fy1, int wx0, int wy0, int wx1, int wy1, long long Aw,
                                               int permille) {
    const int ix = min(fx1, wx1) - max(fx0, wx0) + 1, iy = min(fy1, wy1) - max(fy0, wy0) + 1;
    if (ix <= 0 || iy <= 0) return false;
    const long long I = (long long)ix * (long long)iy;
    const long long U = (long long)(fx1 - fx0 + 1) * (long long)(fy1 - fy0 + 1) + Aw - I;
    return 1000ll * I > (long long)permille * U;
}

// ---- objects (include/fdcm.h, "Objects"): G key planes, one behind the other, plane o holding best(g, o)
// nms_block_min with the pair as the second part of the order: two objects can tie on (bits of q, g), and their pairs differ.
// kNoKey travels with the pair -1, the largest as unsigned.
__device__ __forceinline__ bool nms_pair_less(unsigned long long k2, int p2, unsigned long long key, int pair) {
    return k2 < key || (k2 == key && (unsigned)p2 < (unsigned)pair);
}
__device__ __forceinline__ void nms_block_min_pair(unsigned long long& key, int& pair, unsigned long long* sk, int* sp) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long k2 = __shfl_xor(key, d);
        const int p2 = __shfl_xor(pair, d);
        if (nms_pair_less(k2, p2, key, pair)) { key = k2; pair = p2; }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sk[wave] = key; sp[wave] = pair; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (nms_pair_less(sk[w], sp[w], key, pair)) { key = sk[w]; pair = sp[w]; }
    __syncthreads();  // sk and sp are free again
}

// ---- pose windows (include/fdcm.h, "Pose windows"): a list of jobs, each one template, a run of rotations and a small grid
// of its own.  A plane is one (job, run position e) whose admissible box, clipped to the job's grid, is not empty; the host
// cuts every plane's clipped box into patches of 4 (i) x 16 (j) grid points and lists them, job by job, in one table.  Wave w
// of a launch takes the patches [w ipw, (w + 1) ipw) of the table, a lane per point (lane & 3 along i, lane >> 2 along j: at
// stride 1 the 64 reads of one line end are 16 rows of 4 columns, whole 256-byte runs of the volume when the column is a
// multiple of 4).  Nothing exists for the part of a window outside the box.  The plane and its lines are wave-uniform and
// come through scalar loads.  A wave keeps the sorted k-best list of the job it is in (list_offer) and writes it when the
// job changes: the waves that hold patches of job j are consecutive, wave0 .. wave0 + lists - 1, and wave w's list of job j
// is candidate list list0 + (w - wave0), so k_exhaustive_merge_groups folds a job's lists as one group.
// GATE (include/fdcm.h, "Gate inside the minimum"): a pose's key is offered to the list only when its ML, from rows_score's
// GATE, is >= the plane's need: the job's winner is then the smallest key among the poses that pass.
struct WinPlane {
    int line0, n;        // its lines in the line array
    int i0, i1, j0, j1;  // the admissible box clipped to the job's grid, in grid indices (never empty)
    int x0, y0, nx;      // the job's grid: origin and points per row
    unsigned koff;       // e * N_j, added to the grid index of its keys
    int job;             // the job's place in the batch
    float need;          // (GATE) need of its template
};
struct WinJob { int wave0, list0; };
constexpr int kPatchX = 4, kPatchY = 16;

template <bool BUF32, bool CAP, bool GATE = false>
__global__ void __launch_bounds__(256) k_exhaustive_windows(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx,
                                                            float ty, const ExLine* __restrict__ lines,
                                                            const WinPlane* __restrict__ planes, const int2* __restrict__ items,
                                                            const WinJob* __restrict__ jobs, int n_items, int ipw, int sx, int sy,
                                                            int k, unsigned long long* __restrict__ cand) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int it0 = w * ipw, it1 = min(n_items, it0 + ipw);
    if (it0 >= it1) return;  // wave-uniform
    const VolRef V = make_volref(vol, SL, m, BUF32);
    const unsigned uH = (unsigned)H;
    unsigned long long e = kNoKey, thr = kNoKey;
    int job = -1;
    auto flush = [&]() {
        const WinJob J = jobs[job];
        if (lane < k) cand[(long long)(J.list0 + (w - J.wave0)) * k + lane] = e;
    };
    for (int it = it0; it < it1; ++it) {
        const int2 I = items[it];  // x: the plane, y: the patch in its clipped box, pj << 16 | pi
        const WinPlane P = planes[I.x];
        if (P.job != job) {
            if (job >= 0) flush();
            job = P.job;
            e = thr = kNoKey;
        }
        const int i = P.i0 + (I.y & 0xffff) * kPatchX + (lane & 3), j = P.j0 + (int)((unsigned)I.y >> 16) * kPatchY + (lane >> 2);
        // a lane outside the clipped box reads at the box's corner, which is admissible: every read stays inside the volume
        const bool act = i <= P.i1 && j <= P.j1;
        const float offx = tx + (float)(P.x0 + (act ? i : P.i0) * sx);  // translate(tmpl, sceneTranslation + translation)
        const float offy[1] = {ty + (float)(P.y0 + (act ? j : P.j0) * sy)};
        float res[1] = {0.f};
        float ml[1] = {0.f};
        if constexpr (GATE) rows_score<BUF32, 1, CAP, false, true>(V, lines + P.line0, P.n, offx, offy, W, uH, SL, res, nullptr, 0.f, ml);
        else rows_score<BUF32, 1, CAP>(V, lines + P.line0, P.n, offx, offy, W, uH, SL, res);
        const unsigned long long key = act && !(res[0] != res[0]) && (!GATE || ml[0] >= P.need)  // a NaN score has no key
                                           ? ((unsigned long long)__float_as_uint(res[0]) << 32) | ((unsigned)(j * P.nx + i) + P.koff)
                                           : kNoKey;
        thr = list_offer(e, key, thr, k, lane);
    }
    flush();
}

// ---- line costs (include/fdcm.h, "Per-line caps and line costs"): the uncapped terms of rows_score's sum at a list of
// poses.  A wave per pose, a lane per line, in rounds of 64 lines; the pose and where its lines and its floats are come
// through scalar loads.  The host decided admissibility: a pose that is not writes NaN and reads nothing of the volume.
struct CostPose {
    int line0, n;   // its pair's lines in the line array
    int x, y;       // the translation
    long long out;  // where its n floats go
    int adm, pad;
};

template <bool BUF32>
__global__ void __launch_bounds__(256) k_line_costs(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx, float ty,
                                                    const ExLine* __restrict__ lines, const CostPose* __restrict__ poses, int n_poses,
                                                    float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (w >= n_poses) return;  // wave-uniform
    const CostPose P = poses[w];
    const VolRef V = make_volref(vol, SL, m, BUF32);
    const unsigned uH = (unsigned)H;
    const float offx = tx + (float)P.x, offy = ty + (float)P.y;  // translate(tmpl, sceneTranslation + translation)
    for (int l = lane; l < P.n; l += 64) {
        float v = f_nan();
        if (P.adm) {  // wave-uniform
            const ExLine ln = lines[P.line0 + l];
            const size_t c1 = ex_column<BUF32>((int)(ln.x1 + offx), ln.se, W, uH, SL);
            const size_t c2 = ex_column<BUF32>((int)(ln.x2 + offx), ln.se, W, uH, SL);
            v = line_term<false>(ex_read<BUF32>(V, c1, (int)(ln.y1 + offy), uH), ex_read<BUF32>(V, c2, (int)(ln.y2 + offy), uH), 0.f);
        }
        out[P.out + l] = v;
    }
}

// ---- matched length (include/fdcm.h, "Detections by matched fraction"): the one statement of ML for every kernel below.
// Line i of the n lines at Lt is matched at the translation when its uncapped cost, k_line_costs' float, is <= its cap: one
// float32 compare, so a NaN cost is not matched and an infinite one under a cap of +inf is.  ML is the float32 sum of the
// matched lines' lengths len[i] (an array parallel to the lines) in line order, from +0: sequential by definition, so a
// thread walks its pose's lines alone.  The translation is admissible: every read stays inside the volume.
template <bool BUF32>
__device__ __forceinline__ float matched_length(const VolRef& V, const ExLine* __restrict__ Lt, const float* __restrict__ len, int n,
                                                float offx, float offy, int W, unsigned uH, size_t SL) {
    float ml = 0.f;
    for (int i = 0; i < n; ++i) {
        const ExLine ln = Lt[i];
        const size_t c1 = ex_column<BUF32>((int)(ln.x1 + offx), ln.se, W, uH, SL);
        const size_t c2 = ex_column<BUF32>((int)(ln.x2 + offx), ln.se, W, uH, SL);
        const float c = line_term<false>(ex_read<BUF32>(V, c1, (int)(ln.y1 + offy), uH), ex_read<BUF32>(V, c2, (int)(ln.y2 + offy), uH), 0.f);
        if (c <= ln.cap) ml = ml + len[i];
    }
    return ml;
}
// frac = ML / TL, one IEEE division; 1 for a template whose lengths sum to 0
__device__ __forceinline__ float matched_fraction(float ml, float tl) { return tl == 0.f ? 1.f : ml / tl; }

// The gate: one thread per entry of the key plane k_exhaustive<., kBest> merged, in the plane's own order
// (best_key_point).  An entry with a key computes ML of its pair at its point and loses its key unless
// ML >= need[pair].  Each entry is read and written by its one thread; lanes of a wave hold different pairs.
template <bool BUF32>
__global__ void __launch_bounds__(256) k_matched_gate(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx, float ty,
                                                      const ExLine* __restrict__ lines, const float* __restrict__ len,
                                                      const ExTmpl* __restrict__ tm, const float* __restrict__ need,
                                                      unsigned long long* keys, long long n_keys, int x0, int y0, int sx, int sy,
                                                      int tiles_x) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_keys) return;
    const unsigned long long v = keys[idx];
    if (v == kNoKey) return;
    int i, j;
    best_key_point(idx, tiles_x, i, j);
    const int u = (int)(unsigned)v;
    const int line0 = tm[u].line0, n = tm[u].n;
    const VolRef V = make_volref(vol, SL, m, BUF32);
    const float ml = matched_length<BUF32>(V, lines + line0, len + line0, n, tx + (float)(x0 + i * sx), ty + (float)(y0 + j * sy), W,
                                           (unsigned)H, SL);
    if (!(ml >= need[u])) keys[idx] = kNoKey;
}

// The fractions of the gated best map (include/fdcm.h, "Gate inside the minimum"): one thread per grid point, row-major.  A
// point with a key writes frac of its pair there, ML / TL by matched_length; a point without one NaN.
template <bool BUF32>
__global__ void __launch_bounds__(256) k_matched_plane(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx, float ty,
                                                       const ExLine* __restrict__ lines, const float* __restrict__ len,
                                                       const ExTmpl* __restrict__ tm, const float* __restrict__ tl,
                                                       const unsigned long long* __restrict__ keys, int x0, int y0, int sx, int sy, int nx,
                                                       int ny, int tiles_x, float* __restrict__ frac) {
    const int i = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), j = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (i >= nx || j >= ny) return;
    const unsigned long long v = keys[best_key_index(i, j, tiles_x)];
    const long long g = (long long)j * nx + i;
    if (v == kNoKey) { frac[g] = f_nan(); return; }
    const int u = (int)(unsigned)v;
    const int line0 = tm[u].line0, n = tm[u].n;
    const VolRef V = make_volref(vol, SL, m, BUF32);
    const float ml = matched_length<BUF32>(V, lines + line0, len + line0, n, tx + (float)(x0 + i * sx), ty + (float)(y0 + j * sy), W,
                                           (unsigned)H, SL);
    frac[g] = matched_fraction(ml, tl[u]);
}

// The fractions of the result list: entry l < k of best (a key (bits of q << 32) | g, kNoKey from the list's end on) with
// its pair; tl: TL of every pair's template.  NaN from the end of the list on.
template <bool BUF32>
__global__ void __launch_bounds__(256) k_matched_list(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx, float ty,
                                                      const ExLine* __restrict__ lines, const float* __restrict__ len,
                                                      const ExTmpl* __restrict__ tm, const float* __restrict__ tl,
                                                      const unsigned long long* __restrict__ best, const int* __restrict__ pair, int k,
                                                      int x0, int y0, int sx, int sy, int nx, float* __restrict__ frac) {
    const int l = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (l >= k) return;
    const unsigned long long v = best[l];
    if (v == kNoKey) { frac[l] = f_nan(); return; }
    const unsigned g = (unsigned)v;
    const int i = (int)(g % (unsigned)nx), j = (int)(g / (unsigned)nx);
    const int u = pair[l];
    const int line0 = tm[u].line0, n = tm[u].n;
    const VolRef V = make_volref(vol, SL, m, BUF32);
    const float ml = matched_length<BUF32>(V, lines + line0, len + line0, n, tx + (float)(x0 + i * sx), ty + (float)(y0 + j * sy), W,
                                           (unsigned)H, SL);
    frac[l] = matched_fraction(ml, tl[u]);
}

// The fractions of a pose list (fdcm_matched_fractions): a thread per pose.  The host decided admissibility, as for
// k_line_costs: a pose that is not admissible writes NaN and reads nothing of the volume.
struct FracPose {
    int line0, n;  // its pair's lines in the line array
    int x, y;      // the translation
    float tl;      // TL of its template
    int adm;
};

template <bool BUF32>
__global__ void __launch_bounds__(256) k_matched_fractions(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx,
                                                           float ty, const ExLine* __restrict__ lines, const float* __restrict__ len,
                                                           const FracPose* __restrict__ poses, int n_poses, float* __restrict__ out) {
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= n_poses) return;
    const FracPose P = poses[q];
    if (!P.adm) { out[q] = f_nan(); return; }
    const VolRef V = make_volref(vol, SL, m, BUF32);
    const float ml = matched_length<BUF32>(V, lines + P.line0, len + P.line0, P.n, tx + (float)P.x, ty + (float)P.y, W, (unsigned)H, SL);
    out[q] = matched_fraction(ml, P.tl);
}

// ---- detections over pose windows (include/fdcm.h, "Detections over pose windows")
// The winners of a part of the job list: one thread per job, after the part's last merge.  best[j] is the job's merged list
// at k = 1, its winner's key (score bits << 32) | (e N_j + g) or kNoKey.  The thread decodes it to the run position, the grid
// point and the translation, finds the prepared pair of that run position (run[run0 + e]: its lines, the bits of its
// denominator in koff, its footprint, its need), divides once, applies the threshold and, with a gate (need not null),
// matched_length at the translation, and writes the job's entry of the list: key (bits of q << 32) | the job's index in the
// call, kNoKey for a job without a winner or one the threshold or the gate removes, and the footprint F(j).  An entry has one
// writer; lanes of a wave hold different pairs.
struct WinnerJob {
    int run0;        // where its run's pairs begin in `run`
    int x0, y0, nx;  // its grid
    unsigned N;      // nx ny
    int pad[3];
};
static_assert(sizeof(WinnerJob) == 32, "WinnerJob is 32 bytes");

// The one statement of a job's entry of the winners' list, for both kernels below.  limit(u): the threshold of pair u.
template <bool BUF32, class Limit>
__device__ __forceinline__ void window_winner(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx, float ty,
                                              const ExLine* __restrict__ lines, const float* __restrict__ len,
                                              const ExTmpl* __restrict__ tm, const int4* __restrict__ foot,
                                              const float* __restrict__ need, const WinnerJob* __restrict__ jobs,
                                              const int* __restrict__ run, const unsigned long long* __restrict__ best, int n_jobs,
                                              unsigned job0, int sx, int sy, Limit limit, unsigned long long* __restrict__ keys,
                                              int4* __restrict__ boxes) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= n_jobs) return;
    const unsigned long long v = best[j];
    if (v == kNoKey) {
        keys[j] = kNoKey;
        boxes[j] = make_int4(0, 0, -1, -1);
        return;
    }
    const WinnerJob J = jobs[j];
    const unsigned low = (unsigned)v, e = low / J.N, g = low % J.N;
    const int x = J.x0 + (int)(g % (unsigned)J.nx) * sx, y = J.y0 + (int)(g / (unsigned)J.nx) * sy;
    const int u = run[J.run0 + (int)e];
    const ExTmpl P = tm[u];
    const float q = __uint_as_float((unsigned)(v >> 32)) / __uint_as_float(P.koff);  // one IEEE division, as the best map's
    bool keep = !(q != q) && q <= limit(u);
    if (keep && need) {
        const VolRef V = make_volref(vol, SL, m, BUF32);
        const float ml = matched_length<BUF32>(V, lines + P.line0, len + P.line0, P.n, tx + (float)x, ty + (float)y, W, (unsigned)H, SL);
        keep = ml >= need[u];
    }
    const int4 b = foot[u];
    keys[j] = keep ? ((unsigned long long)__float_as_uint(q) << 32) | (job0 + (unsigned)j) : kNoKey;
    boxes[j] = make_int4(b.x + x, b.y + y, b.z + x, b.w + y);
}

template <bool BUF32>
__global__ void __launch_bounds__(256) k_window_winners(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx, float ty,
                                                        const ExLine* __restrict__ lines, const float* __restrict__ len,
                                                        const ExTmpl* __restrict__ tm, const int4* __restrict__ foot,
                                                        const float* __restrict__ need, const WinnerJob* __restrict__ jobs,
                                                        const int* __restrict__ run, const unsigned long long* __restrict__ best,
                                                        int n_jobs, unsigned job0, int sx, int sy, float max_score,
                                                        unsigned long long* __restrict__ keys, int4* __restrict__ boxes) {
    window_winner<BUF32>(vol, SL, m, W, H, tx, ty, lines, len, tm, foot, need, jobs, run, best, n_jobs, job0, sx, sy,
                         [=](int) { return max_score; }, keys, boxes);
}

// Objects (include/fdcm.h, "Objects"), the windows' call.  k_window_winners with the threshold of the job's object: ms[u] is
// max_score[objects[template of pair u]], as need[u] is that object's need; everything else is k_window_winners'.
template <bool BUF32>
__global__ void __launch_bounds__(256) k_window_winners_objects(const float* __restrict__ vol, size_t SL, int m, int W, int H, float tx,
                                                                float ty, const ExLine* __restrict__ lines, const float* __restrict__ len,
                                                                const ExTmpl* __restrict__ tm, const int4* __restrict__ foot,
                                                                const float* __restrict__ need, const float* __restrict__ ms,
                                                                const WinnerJob* __restrict__ jobs, const int* __restrict__ run,
                                                                const unsigned long long* __restrict__ best, int n_jobs, unsigned job0,
                                                                int sx, int sy, unsigned long long* __restrict__ keys,
                                                                int4* __restrict__ boxes) {
    window_winner<BUF32>(vol, SL, m, W, H, tx, ty, lines, len, tm, foot, need, jobs, run, best, n_jobs, job0, sx, sy,
                         [=](int u) { return ms[u]; }, keys, boxes);
}

// ---- hull footprints (include/fdcm.h, "Hull footprints"): the rounds with the shape of an entry the lattice points of
// the convex hull of its pair's posed end points, row by row.  A shape is its box (the rounds' own), its area and a run of
// the span table: row r of the box is the pixels xl .. xr in the box's frame, (0, -1) when it is empty.  Two forms of the
// round below, the plane form and the list form with objects; a call without objects runs them with one object (no table
// of objects: every entry's object is 0), which gives the same list since one plane holds no two equal keys.
struct HullShape {
    long long area;  // A(u) = |P(u)|
    int row0;        // its first row of the span table; it has y1 - y0 + 1 rows
    int pad;
};
static_assert(sizeof(HullShape) == 16, "HullShape is 16 bytes");

constexpr int kHullStagedRows = 1024;  // rows of the winner's spans a workgroup keeps in LDS (8 KB); a taller winner is read from memory

// The winner's spans for its workgroup: staged when they fit.  Every thread of the workgroup calls it (round > 0).
__device__ __forceinline__ bool hull_stage(const int2* __restrict__ spans, int row0, int rows, int2* ws) {
    const bool staged = rows <= kHullStagedRows;  // workgroup-uniform
    if (staged) {
        for (int r = threadIdx.x; r < rows; r += 256) ws[r] = spans[row0 + r];
        __syncthreads();
    }
    return staged;
}

// The overlap test on shapes, the one statement of it: the entry's shape (box f, area A, rows from f_row0) against the
// winner's (box w, area Aw, rows from w_row0 or in ws).  Boxes that share no pixel never suppress each other; I <= I_box, so
// 1000 I_box <= permille (A + Aw - I_box) proves the same without a span; else I is the sum over the common rows, in int64.
__device__ __forceinline__ bool hull_suppresses(int fx0, int fy0, int fx1, int fy1, long long A, int f_row0, int wx0, int wy0, int wx1,
                                                int wy1, long long Aw, int w_row0, bool staged, const int2* ws,
                                                const int2* __restrict__ spans, int permille) {
    const int ya = max(fy0, wy0), yb = min(fy1, wy1);
    const int ix = min(fx1, wx1) - max(fx0, wx0) + 1, iy = yb - ya + 1;
    if (ix <= 0 || iy <= 0) return false;
    const long long Ibox = (long long)ix * (long long)iy;
    if (1000ll * Ibox <= (long long)permille * (A + Aw - Ibox)) return false;
    long long I = 0;
    for (int y = ya; y <= yb; ++y) {
        const int2 a = spans[f_row0 + (y - fy0)];
        const int2 b = staged ? ws[y - wy0] : spans[w_row0 + (y - wy0)];
        I += max(0, min(a.y + fx0, b.y + wx0) - max(a.x + fx0, b.x + wx0) + 1);
    }
    return 1000ll * I > (long long)permille * (A + Aw - I);
}

// ---- the round of the greedy rule, every form of it: one launch of the scheme under "detections by footprint overlap".
//   LIST  the entries.  Plane forms: G key planes, one behind the other, plane o holding best(g, o) (G = 1 without objects):
//         one array of n_chunks runs of 256 keys, plane_chunks of them per plane (a plane is whole sub-tiles, so a run lies
//         in one plane).  An entry's object is its run's plane, its point best_key_point inside the plane, its pair its key's
//         low half; boxes, shapes and obj are per pair, and a footprint is the pair's box moved to the point's translation.
//         The winner's entry is the one at its point in its object's plane: it is erased by object and point, an entry of
//         another object at the same point only when the cross limit says so.  A partial carries the pair with the key,
//         because the winner's entry of the plane is erased in the launch that needs its box.
//         List forms: the winners' list of the windows' calls, n entries.  Entry j is (keys[j], boxes[j]), its key's low half
//         j itself and its footprint its own, in the scene already; boxes, shapes and obj are per entry, so nothing goes
//         through a pair.  No two keys are equal, so the partials are keys alone, ordered by key, and `pair` is not written.
//         The winner's box is read from the list: a round erases keys, never boxes.
//   HULL  the overlap test: hull_suppresses on shapes, else nms_suppresses on boxes.
//   OBJ   objects (include/fdcm.h, "Objects"): the limit of an entry is `permille` when its object is the winner's and `cross`
//         otherwise, and the plane forms order their partials as (key, pair); without, `permille` and by key.  The hull
//         forms exist with objects alone: a null obj is "every entry's object is 0", which gives the list of a call without
//         objects since one plane holds no two equal keys.
// The instantiations are the six nms_rounds launches.  One writer per entry, no atomics, no cooperative launch.
struct NmsArgs {
    unsigned long long* keys;
    const int4* boxes;
    const HullShape* shapes;  // (HULL)
    const int2* spans;        // (HULL) the span table
    const int* obj;           // (OBJ) the objects' table; (HULL) or null
    long long n;              // (LIST) entries
    long long n_chunks, plane_chunks;  // runs of 256 entries: all of them, (plane forms) per plane
    int x0, y0, sx, sy, nx, tiles_x;   // (plane forms) the grid
    int permille, cross, round, last;
    const unsigned long long* pk_in;  // the partials of round - 1 and of this round: keys, (plane forms) pairs
    const int* pp_in;
    unsigned long long* pk_out;
    int* pp_out;
    unsigned long long* best;  // the result list: keys, (plane forms) pairs
    int* pair;
};

template <bool LIST, bool OBJ>
__device__ __forceinline__ void nms_min(unsigned long long& key, int& pair, unsigned long long* sk, int* sp) {
    if (LIST) nms_block_min(key, sk);
    else if (OBJ) nms_block_min_pair(key, pair, sk, sp);
    else nms_block_min(key, pair, sk, sp);
}
// An entry's footprint in the scene: entry u of boxes, in a plane form moved to grid point (i, j).
template <bool LIST>
__device__ __forceinline__ int4 nms_footprint(const NmsArgs& a, long long u, int i, int j) {
    const int4 b = a.boxes[u];
    if (LIST) return b;
    const int tx = a.x0 + i * a.sx, ty = a.y0 + j * a.sy;
    return make_int4(b.x + tx, b.y + ty, b.z + tx, b.w + ty);
}
template <bool HULL>
__device__ __forceinline__ int nms_object(const NmsArgs& a, long long u) {
    return HULL && !a.obj ? 0 : a.obj[u];
}

template <bool LIST, bool HULL, bool OBJ>
__global__ void __launch_bounds__(256) k_nms_round(const NmsArgs a) {
    static_assert(OBJ || !HULL, "the hull forms exist with objects alone");
    __shared__ unsigned long long sk[4];
    __shared__ int sp[4];
    __shared__ int2 ws[HULL ? kHullStagedRows : 1];
    unsigned long long W = kNoKey;
    int Wp = -1;
    if (a.round > 0) {
        if (threadIdx.x < gridDim.x) {
            W = a.pk_in[threadIdx.x];
            if (!LIST) Wp = a.pp_in[threadIdx.x];
        }
        nms_min<LIST, OBJ>(W, Wp, sk, sp);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.best[a.round - 1] = W;
            if (!LIST) a.pair[a.round - 1] = W == kNoKey ? -1 : Wp;
        }
        if (W == kNoKey || a.last) {  // workgroup-uniform
            if (threadIdx.x == 0) {
                a.pk_out[blockIdx.x] = kNoKey;
                if (!LIST) a.pp_out[blockIdx.x] = -1;
            }
            return;
        }
    }
    // the winner: its point or entry gw, its entry uw of the tables, its object, its footprint and area or shape (round 0: unused)
    const unsigned gw = (unsigned)W;
    const long long uw = LIST ? (long long)gw : (long long)Wp;
    int4 w = make_int4(0, 0, -1, -1);
    int ow = -1, w_row0 = 0;
    long long Aw = 0;
    bool staged = false;
    if (a.round > 0) {
        w = nms_footprint<LIST>(a, uw, (int)(gw % (unsigned)a.nx), (int)(gw / (unsigned)a.nx));
        const HullShape s = HULL ? a.shapes[uw] : HullShape{};  // (before the object, as in the walk below)
        if (OBJ) ow = nms_object<HULL>(a, uw);
        if (HULL) {
            Aw = s.area;
            w_row0 = s.row0;
            staged = hull_stage(a.spans, w_row0, w.w - w.y + 1, ws);
        }
    }
    if (!HULL) Aw = (long long)(w.z - w.x + 1) * (long long)(w.w - w.y + 1);
    const long long c0 = a.n_chunks * (long long)blockIdx.x / (long long)gridDim.x;
    const long long c1 = a.n_chunks * ((long long)blockIdx.x + 1) / (long long)gridDim.x;
    unsigned long long mk = kNoKey;
    int mp = -1;
    for (long long c = c0; c < c1; ++c) {
        const long long idx = c * 256 + threadIdx.x;
        if (LIST && idx >= a.n) continue;
        const unsigned long long v = a.keys[idx];
        if (v == kNoKey) continue;
        // the entry: its plane, its point (i, j) = g or its place in the list, its entry u of the tables
        const int plane = !LIST && OBJ ? (int)(c / a.plane_chunks) : 0;  // (wave-uniform)
        int i = 0, j = 0;
        if (!LIST) best_key_point(idx - (long long)plane * a.plane_chunks * 256, a.tiles_x, i, j);
        const unsigned g = LIST ? (unsigned)idx : (unsigned)(j * a.nx + i);
        const long long u = LIST ? idx : (long long)(int)(unsigned)v;
        bool drop = false;
        if (a.round > 0) {
            drop = g == gw && (LIST || !OBJ || plane == ow);
            if (!drop) {
                // (the box and the shape before the object: their loads then go out together, ahead of the table's null test)
                const int4 f = nms_footprint<LIST>(a, u, i, j);
                const HullShape s = HULL ? a.shapes[u] : HullShape{};
                const int limit = !OBJ || (LIST ? nms_object<HULL>(a, u) : plane) == ow ? a.permille : a.cross;
                drop = HULL ? hull_suppresses(f.x, f.y, f.z, f.w, s.area, s.row0, w.x, w.y, w.z, w.w, Aw, w_row0, staged, ws, a.spans, limit)
                            : nms_suppresses(f.x, f.y, f.z, f.w, w.x, w.y, w.z, w.w, Aw, limit);
            }
        }
        if (drop) {
            a.keys[idx] = kNoKey;
        } else if (LIST) {
            if (v < mk) mk = v;
        } else {
            const unsigned long long key = (v & 0xffffffff00000000ull) | g;
            if (OBJ ? nms_pair_less(key, (int)u, mk, mp) : key < mk) { mk = key; mp = (int)u; }
        }
    }
    nms_min<LIST, OBJ>(mk, mp, sk, sp);
    if (threadIdx.x == 0) {
        a.pk_out[blockIdx.x] = mk;
        if (!LIST) a.pp_out[blockIdx.x] = mp;
    }
}

long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// The integer translations t in [-kMaxCoord, kMaxCoord] with lo < fl(p + fl(off + t)) < hi for p = pmin and p = pmax, i.e.
// for every end point coordinate p of the template: the seam's rule (fdcm_seam.hip, k_evaluate) along one axis, with
// lo = -1 and hi = the feature size.  Float addition is monotone, so the set is an interval; found by bisection on the
// same float operations the kernels do.  Returns false when it is empty.
bool axis_interval(float pmin, float pmax, float off, float size, int& a0, int& a1) {
    auto above = [&](int t) { return pmin + (off + (float)t) > -1.f; };  // rises with t
    auto below = [&](int t) { return pmax + (off + (float)t) < size; };  // falls with t
    if (!above(kMaxCoord) || !below(-kMaxCoord)) return false;
    int lo = -kMaxCoord, hi = kMaxCoord;  // the first t that is above
    while (lo < hi) {
        const int mid = (int)floor_div((long long)lo + hi, 2);
        if (above(mid)) hi = mid; else lo = mid + 1;
    }
    a0 = lo;
    lo = -kMaxCoord; hi = kMaxCoord;  // the last t that is below
    while (lo < hi) {
        const int mid = (int)floor_div((long long)lo + hi + 1, 2);
        if (below(mid)) lo = mid; else hi = mid - 1;
    }
    a1 = lo;
    return a0 <= a1;
}

struct Box { bool any; int x0, x1, y0, y1; };

// The admissible translations of a template (lines [l0, l0 + n) of t): a box, or none.  A template without lines is
// admissible everywhere.
Box admissible_box(const fdcm_featuremap* fm, const fdcm_templates* t, int64_t l0, int64_t n) {
    Box b{true, -kMaxCoord, kMaxCoord, -kMaxCoord, kMaxCoord};
    if (n == 0) return b;
    if (fm->W == 0 || fm->H == 0 || fm->m == 0) { b.any = false; return b; }
    float mnx = f_inf(), mxx = -f_inf(), mny = f_inf(), mxy = -f_inf();
    for (int64_t q = l0; q < l0 + n; ++q) {
        const float* p = &t->lines[(size_t)q * 4];
        for (int c = 0; c < 2; ++c) {
            if (std::isnan(p[2 * c]) || std::isnan(p[2 * c + 1])) { b.any = false; return b; }
            mnx = std::min(mnx, p[2 * c]); mxx = std::max(mxx, p[2 * c]);
            mny = std::min(mny, p[2 * c + 1]); mxy = std::max(mxy, p[2 * c + 1]);
        }
    }
    b.any = axis_interval(mnx, mxx, fm->tx, (float)fm->W, b.x0, b.x1) && axis_interval(mny, mxy, fm->ty, (float)fm->H, b.y0, b.y1);
    return b;
}

// grid indices [i0, i1] of the points x0 + i * s inside [a0, a1]
void grid_range(int a0, int a1, int x0, int n, int s, int& i0, int& i1) {
    i0 = (int)std::max<long long>(0, -floor_div((long long)x0 - a0, s));  // ceil((a0 - x0) / s)
    i1 = (int)std::min<long long>(n - 1, floor_div((long long)a1 - x0, s));
}

void check_grid(const fdcm_grid& g) {
    if (g.nx < 1 || g.ny < 1) throw std::string("grid: nx and ny must be >= 1");
    if (g.sx < 1 || g.sy < 1) throw std::string("grid: strides sx and sy must be >= 1");
    if ((long long)g.nx * g.ny >= (1ll << 31)) throw std::string("grid: nx * ny must be below 2^31");
    const long long xe = (long long)g.x0 + (long long)(g.nx - 1) * g.sx, ye = (long long)g.y0 + (long long)(g.ny - 1) * g.sy;
    if (g.x0 < -kMaxCoord || xe > kMaxCoord || g.y0 < -kMaxCoord || ye > kMaxCoord)
        throw std::string("grid: every translation must satisfy |t| < 2^24");
}

// One line for the kernels: closestOrientation with the host libm (dt3cpu.cpp:144-148, as fdcm_seam.hip's run_evaluate).
ExLine line_record(const fdcm_featuremap* fm, const float* p, float cap, float len, bool buf32, size_t SL) {
    const float angle = std::atan((p[3] - p[1]) / (p[2] - p[0]));  // getAngle, math.h:295-299
    const int bin = closest_orientation(fm->keys.data(), (int)fm->m, angle);
    return ExLine{p[0], p[1], p[2], p[3], buf32 ? (int)((unsigned)bin * (unsigned)SL) : bin, cap, len, 0};
}

void begin(fdcm_featuremap* fm) {
    if (fm->holds != VolStage::integrated) throw std::string("the feature map holds a partial build (no line integral): nothing to search");
    finish_build(fm);
    FDCM_HIP(hipSetDevice(fm->device));
    if (!fm->stream) FDCM_HIP(hipStreamCreateWithFlags(&fm->stream, hipStreamNonBlocking));
}

size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- rotations (include/fdcm.h, "Rotations")
// M_a = [R | m] of rotate(lines, R, rot_point), math.h:372-378, with R = [[c, -s], [s, c]] and m = p - R p: every product
// and sum rounded to float32, left to right (the Makefile's -ffp-contract=off keeps them unfused on the host too).
struct RotM { float c, ns, s, mx, my; };

RotM rot_matrix(float c, float s, float px, float py) {
    const float ns = -s;
    return RotM{c, ns, s, px - (c * px + ns * py), py - (s * px + c * py)};
}

// The line sets M_a(t) of the templates [t0, t1) of t under every rotation, as one template set: (t, a) is its template
// (t - t0) * n + a.  M: the transform of each.
void rotated_set(const fdcm_templates* t, const fdcm_rotations& rot, int64_t t0, int64_t t1, fdcm_templates& out, RotM* M) {
    const int n = rot.n;
    out.device = t->device;
    out.T = (t1 - t0) * n;
    out.n_lines = (t->offsets[(size_t)t1] - t->offsets[(size_t)t0]) * n;
    out.lines.resize((size_t)out.n_lines * 4);
    out.offsets.assign((size_t)out.T + 1, 0);
    int64_t w = 0;
    for (int64_t i = t0; i < t1; ++i) {
        const int64_t l0 = t->offsets[(size_t)i], l1 = t->offsets[(size_t)i + 1];
        const float px = rot.pivots ? rot.pivots[2 * i] : 0.f, py = rot.pivots ? rot.pivots[2 * i + 1] : 0.f;
        for (int a = 0; a < n; ++a) {
            const RotM m = rot_matrix(rot.cs[2 * a], rot.cs[2 * a + 1], px, py);
            M[(i - t0) * n + a] = m;
            for (int64_t q = l0; q < l1; ++q, ++w) {
                const float* p = &t->lines[(size_t)q * 4];
                float* o = &out.lines[(size_t)w * 4];
                for (int c = 0; c < 2; ++c) {  // transform, math.h:341-344
                    const float x = p[2 * c], y = p[2 * c + 1];
                    o[2 * c] = (m.c * x + m.ns * y) + m.mx;
                    o[2 * c + 1] = (m.s * x + m.c * y) + m.my;
                }
            }
            out.offsets[(size_t)((i - t0) * n + a) + 1] = w;
        }
    }
}

void check_rotated_size(const fdcm_templates* t, int n) {
    if (t->T * (int64_t)n > 0x7fffffffll || t->n_lines * (int64_t)n > 0x7fffffffll)
        throw std::string("too many rotated templates or template lines for one call");
}

// part(c) for every c < nth, on nth threads (on the caller's when nth is 1).  A part that throws stops alone; the first
// error is thrown again after all have joined (`what`: the message of an error that is not the library's own).
template <class F>
void on_threads(int nth, const char* what, F part) {
    std::vector<std::string> err((size_t)nth);
    auto job = [&](int c) {
        try {
            part(c);
        } catch (const std::string& e) {
            err[(size_t)c] = e;
        } catch (...) {
            err[(size_t)c] = what;
        }
    };
    if (nth == 1) {
        job(0);
    } else {
        std::vector<std::thread> pool;
        for (int c = 0; c < nth; ++c) pool.emplace_back(job, c);
        for (std::thread& th : pool) th.join();
    }
    for (const std::string& e : err)
        if (!e.empty()) throw e;
}

// The footprint of a pair (include/fdcm.h, "Detections suppressed by footprint overlap"): x0, y0, x1, y1.
struct Foot { int32_t x0, y0, x1, y1; };
static_assert(sizeof(Foot) == 16, "Foot is 16 bytes");
Foot footprint(const float* p, size_t stride, int64_t n, int margin);

// ---- the host preparation, the one of every call
// (template, rotation) pairs, each prepared once: its rotated lines (RotM's rule; the caller's own lines when there is no
// table), their bins (line_record), their caps (the line's own under every rotation) and its admissible box in translation
// coordinates.  The dense calls prepare every pair
// of the set; the pose windows the distinct pairs a run of jobs names.
struct Pairs {
    std::vector<int64_t> key;    // tmpl * n + a, ascending; empty: every pair of the set, pair u being tmpl * n + a = u
    std::vector<ExLine> lines;   // (never empty)
    bool lens = false;           // set before prepare_pairs: also fill len (the matched fraction's calls)
    std::vector<float> len;      // per line of `lines`: its template line's length, kept under every rotation (or empty)
    std::vector<int> line0, nl;  // per pair: its lines
    std::vector<Box> box;
    std::vector<RotM> M;  // (rotations only)
    int foot_margin = -1;    // set >= 0 before prepare_pairs: also fill foot, the pairs' footprints at that margin
    std::vector<Foot> foot;  // (or empty)
    bool buf32 = true;    // VolRef's form for the kernels that read the lines
    bool capped = false;  // the set has a finite cap: the scoring kernels that clamp
    size_t SL = 0;
    size_t find(int64_t k) const { return (size_t)(std::lower_bound(key.begin(), key.end(), k) - key.begin()); }
};

// rotated_set, line_record and admissible_box of every pair of W.key, in up to 16 threads over ranges of pairs of about
// 2^12 lines or more.  Inside a range the pairs of one template are one rotated_set over their rotations, so a template's
// lines are read once; every output is written by pair index, so the result does not depend on the cuts.  rot null: the
// translations, a table of one rotation (n = 1).  flat: the 64-bit form of VolRef whatever the volume's size.
void prepare_pairs(const fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, bool flat, Pairs& W) {
    const int n = rot ? rot->n : 1;
    const bool all = W.key.empty();
    const size_t np = all ? (size_t)(t->T * n) : W.key.size();
    auto key_of = [&](size_t u) { return all ? (int64_t)u : W.key[u]; };
    W.SL = ivol_slice_floats(fm->W, fm->H);
    W.capped = t->capped;
    W.buf32 = !flat && (size_t)fm->m * W.SL * sizeof(float) < ((size_t)1 << 32);  // the rule k_search uses
    W.line0.assign(np, 0);
    W.nl.assign(np, 0);
    W.box.assign(np, Box{false, 0, 0, 0, 0});
    if (rot) W.M.resize(np);
    if (W.foot_margin >= 0) W.foot.assign(np, Foot{0, 0, -1, -1});
    int64_t total = 0;
    for (size_t u = 0; u < np; ++u) {  // pair u's lines follow pair u - 1's
        const int64_t i = key_of(u) / n;
        W.line0[u] = (int)total;  // (in range once total is, below)
        W.nl[u] = (int)(t->offsets[(size_t)i + 1] - t->offsets[(size_t)i]);
        total += W.nl[u];
    }
    if (total > 0x7fffffffll)
        throw std::string(all && !rot ? "too many template lines for one exhaustive search"
                                      : "too many rotated template lines for one call");
    W.lines.assign((size_t)std::max<int64_t>(1, total), ExLine{});
    if (W.lens) {
        W.len.assign(W.lines.size(), 0.f);
        for (size_t u = 0; u < np; ++u)
            std::copy_n(t->lengths.begin() + t->offsets[(size_t)(key_of(u) / n)], W.nl[u], W.len.begin() + W.line0[u]);
    }
    const int nth = (int)std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)np, total >> 12}));
    std::vector<size_t> cut((size_t)nth + 1);
    for (int c = 0; c <= nth; ++c) cut[(size_t)c] = np * (size_t)c / (size_t)nth;
    const char* what = all ? "host preparation of the rotated templates failed" : "host preparation of the pose windows failed";
    on_threads(nth, what, [&](int c) {
        std::vector<float> cs;
        fdcm_templates rt;
        for (size_t p = cut[(size_t)c]; p < cut[(size_t)c + 1];) {
            const int64_t i = key_of(p) / n;
            size_t q = p;
            cs.clear();
            for (; q < cut[(size_t)c + 1] && key_of(q) / n == i; ++q)
                if (rot) {
                    const int64_t a = key_of(q) % n;
                    cs.push_back(rot->cs[2 * a]);
                    cs.push_back(rot->cs[2 * a + 1]);
                }
            if (rot) {
                const fdcm_rotations sub{cs.data(), (int32_t)(q - p), rot->pivots};
                rotated_set(t, sub, i, i + 1, rt, W.M.data() + p);
            }
            const fdcm_templates* src = rot ? &rt : t;  // the caller's lines as they are (run_search_exhaustive_peaks' note on -0)
            for (size_t u = p; u < q; ++u) {
                const int64_t l0 = rot ? rt.offsets[u - p] : t->offsets[(size_t)i];
                W.box[u] = admissible_box(fm, src, l0, W.nl[u]);
                for (int x = 0; x < W.nl[u] && fm->m > 0; ++x)  // (an empty map has no bins: no line is read there)
                    W.lines[(size_t)W.line0[u] + x] =
                        line_record(fm, &src->lines[(size_t)(l0 + x) * 4], t->caps[(size_t)(t->offsets[(size_t)i] + x)],
                                    t->lengths[(size_t)(t->offsets[(size_t)i] + x)], W.buf32, W.SL);
                if (W.foot_margin >= 0) W.foot[u] = footprint(&src->lines[(size_t)l0 * 4], 4, W.nl[u], W.foot_margin);
            }
            p = q;
        }
    });
}

// Pair u of W on the grid g as a template of a launch: its admissible box in grid indices.
ExTmpl grid_tmpl(const Pairs& W, size_t u, const fdcm_grid& g, int slot) {
    ExTmpl e{W.line0[u], W.nl[u], 0, -1, 0, -1, slot, 0};
    if (W.box[u].any) {
        grid_range(W.box[u].x0, W.box[u].x1, g.x0, g.nx, g.sx, e.i0, e.i1);
        grid_range(W.box[u].y0, W.box[u].y1, g.y0, g.ny, g.sy, e.j0, e.j1);
    }
    return e;
}

// The records of the merged lists best[q][k], q < Q (kNoKey ends a list).  List q is template tmpl_of(q)'s on the grid
// grid_of(q) with N = nx ny points: key a N + g -> transform [R | m + (tx, ty)], R | m = *rot_of(q, a), or the pure translation
// when that is null.  offsets (Q + 1, or null): where each list's records begin.
template <class TmplOf, class GridOf, class RotOf>
void emit_records(const std::vector<unsigned long long>& best, int k, int64_t Q, TmplOf tmpl_of, GridOf grid_of, RotOf rot_of,
                  fdcm_match** out, int64_t* n_out, int64_t* offsets) {
    int64_t cnt = 0;
    for (unsigned long long v : best) cnt += v != kNoKey;
    fdcm_match* m = result_acquire((size_t)std::max<int64_t>(1, cnt) * sizeof(fdcm_match));
    int64_t w = 0;
    for (int64_t q = 0; q < Q; ++q) {
        if (offsets) offsets[q] = w;
        const fdcm_grid& g = grid_of(q);
        const unsigned long long N = (unsigned long long)g.nx * g.ny;
        for (int r = 0; r < k; ++r) {
            const unsigned long long v = best[(size_t)q * k + r];
            if (v == kNoKey) break;
            const unsigned long long low = v & 0xffffffffull;
            const int a = (int)(low / N);
            const unsigned gi = (unsigned)(low % N);
            const int i = (int)(gi % (unsigned)g.nx), j = (int)(gi / (unsigned)g.nx);
            const float tx = (float)(g.x0 + i * g.sx), ty = (float)(g.y0 + j * g.sy);
            fdcm_match& rec = m[w++];
            rec.tmpl_idx = tmpl_of(q);
            rec.score = f_from_bits((uint32_t)(v >> 32));
            if (const RotM* R = rot_of(q, a)) {  // combine(translation, M_a), float32 adds
                rec.transform[0] = R->c; rec.transform[1] = R->ns; rec.transform[2] = R->mx + tx;
                rec.transform[3] = R->s; rec.transform[4] = R->c; rec.transform[5] = R->my + ty;
            } else {  // combine(t, identity): the transform of a pure translation (Match.transform)
                rec.transform[0] = 1.f; rec.transform[1] = 0.f; rec.transform[2] = tx;
                rec.transform[3] = 0.f; rec.transform[4] = 1.f; rec.transform[5] = ty;
            }
        }
    }
    if (offsets) offsets[Q] = w;
    *out = m;
    *n_out = cnt;
}

// The dense searches' lists: template index[q] on the one grid g, R | m the transform M[index[q] n + a] of the rotation
// search, or a pure translation when M is null.
void emit_records(const std::vector<unsigned long long>& best, int k, const std::vector<int32_t>& index, int n, const fdcm_grid& g,
                  int32_t base, const RotM* M, fdcm_match** out, int64_t* n_out) {
    emit_records(
        best, k, (int64_t)index.size(), [&](int64_t q) { return base + index[(size_t)q]; }, [&](int64_t) -> const fdcm_grid& { return g; },
        [&](int64_t q, int a) { return M ? &M[(size_t)index[(size_t)q] * n + a] : nullptr; }, out, n_out, nullptr);
}

// Launches k_exhaustive over the templates tm (already on the device at d_tm) with the lines at d_lines.
// d_bc (best map only, or null): the pairs' exit bounds, with max_score: k_exhaustive<., kBestBound, .> in place of kBest.
template <int MODE>
void launch(fdcm_featuremap* fm, const Pairs& P, const fdcm_grid& g, const ExLine* d_lines, const ExTmpl* d_tm, int T, int k,
            int portions, float* map, unsigned long long* cand, const float* d_bc = nullptr, float max_score = 0.f,
            const float* d_need = nullptr) {
    const int tiles_x = (g.nx + kTileX - 1) / kTileX, tiles_y = (g.ny + kTileY - 1) / kTileY;
    const int n_subtiles = tiles_x * tiles_y;
    const float* vol = fm->vol.as<float>();
    const long long plane = (long long)g.nx * g.ny;
    const int per_launch = (1 << 20) * kChunk;  // keeps portions x chunks in range; outputs go by slot
    for (int t0 = 0; t0 < T; t0 += per_launch) {
        const int nt = std::min(per_launch, T - t0);
        const dim3 grid((unsigned)(portions * ((nt + kChunk - 1) / kChunk)));  // portions: a multiple of 8
        if constexpr (MODE == kBest) {
            if (d_need) {  // the gate inside the minimum (these forms always clamp too: caps of +inf change no term)
                auto args = [&](auto kern, auto bound) {
                    hipLaunchKernelGGL(kern, grid, dim3(256), 0, fm->stream, vol, P.SL, (int)fm->m, (int)fm->W, (int)fm->H, fm->tx, fm->ty,
                                       d_lines, d_tm + t0, nt, g.x0, g.y0, g.nx, g.ny, g.sx, g.sy, tiles_x, n_subtiles, portions, k, map,
                                       plane, cand, bound);
                };
                if (d_bc)
                    args(P.buf32 ? k_exhaustive<true, kBestBoundGate, true> : k_exhaustive<false, kBestBoundGate, true>,
                         ExBound<true, true>{d_bc, max_score, d_need});
                else
                    args(P.buf32 ? k_exhaustive<true, kBestGate, true> : k_exhaustive<false, kBestGate, true>, ExBound<false, true>{d_need});
                FDCM_HIP(hipGetLastError());
                continue;
            }
            if (d_bc) {
                // (the 64-bit form always clamps: caps of +inf change no term, and without the clamp that form takes 130
                // registers, a wave per SIMD fewer than the best map's -- DESIGN.md section 20)
                auto kern = !P.buf32 ? k_exhaustive<false, kBestBound, true>
                                     : (P.capped ? k_exhaustive<true, kBestBound, true> : k_exhaustive<true, kBestBound, false>);
                hipLaunchKernelGGL(kern, grid, dim3(256), 0, fm->stream, vol, P.SL, (int)fm->m, (int)fm->W, (int)fm->H, fm->tx, fm->ty,
                                   d_lines, d_tm + t0, nt, g.x0, g.y0, g.nx, g.ny, g.sx, g.sy, tiles_x, n_subtiles, portions, k, map, plane,
                                   cand, ExBound<true>{d_bc, max_score});
                FDCM_HIP(hipGetLastError());
                continue;
            }
        }
        auto kern = P.capped ? (P.buf32 ? k_exhaustive<true, MODE, true> : k_exhaustive<false, MODE, true>)
                             : (P.buf32 ? k_exhaustive<true, MODE, false> : k_exhaustive<false, MODE, false>);
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, fm->stream, vol, P.SL, (int)fm->m, (int)fm->W, (int)fm->H, fm->tx, fm->ty, d_lines,
                           d_tm + t0, nt, g.x0, g.y0, g.nx, g.ny, g.sx, g.sy, tiles_x, n_subtiles, portions, k, map, plane, cand,
                           ExBound<false>{});
        FDCM_HIP(hipGetLastError());
    }
}

// Workgroups along the grid (a multiple of 8, one group per XCD): about as many workgroups of all template chunks as are
// resident at once (4 per compute unit: 128 VGPRs), no more groups than sub-tiles.
int portions_for(const fdcm_featuremap* fm, const fdcm_grid& g, int T) {
    const long long n_subtiles = (long long)((g.nx + kTileX - 1) / kTileX) * ((g.ny + kTileY - 1) / kTileY);
    const long long chunks = (std::min(T, (1 << 20) * kChunk) + kChunk - 1) / kChunk;
    const long long per_xcd = std::max<long long>(1, (4ll * device_cus(fm->device) / 8) / chunks);
    return 8 * (int)std::max<long long>(1, std::min<long long>(per_xcd, (n_subtiles + 7) / 8));
}

constexpr size_t kMapBytes = (size_t)768 << 20;     // the score planes of one batch (peaks): translations
constexpr size_t kRotMapBytes = (size_t)512 << 20;  // .. rotations (n > 1): larger batches slow their stride-2 passes
constexpr size_t kCandBytes = (size_t)128 << 20;  // the candidate lists of one batch (top-k)

// The search driver, the top-k when rx = ry = ra = 0 and the peaks otherwise.  P: every pair of T templates and n angles,
// prepared: T x n planes, plane t n + a being template t at angle a (n = 1: the translations).  Out: index, the templates
// that can emit -- lines, and an admissible grid point under some angle -- in ascending order, and best[q][k], the merged
// list of template index[q] (kNoKey ends a list).
void search(fdcm_featuremap* fm, const Pairs& P, int n, const fdcm_grid& g, int k, int rx, int ry, int ra, int wrap,
            std::vector<unsigned long long>& best, std::vector<int32_t>& index) {
    std::vector<ExTmpl> tm(P.nl.size());  // every plane on the full grid, slot = its index
    for (size_t u = 0; u < tm.size(); ++u) tm[u] = grid_tmpl(P, u, g, (int)u);
    const int64_t T = (int64_t)tm.size() / n;
    const unsigned long long N = (unsigned long long)g.nx * g.ny;
    for (int64_t i = 0; i < T; ++i) {
        if (tm[(size_t)(i * n)].n == 0) continue;
        for (int a = 0; a < n; ++a) {
            const ExTmpl& e = tm[(size_t)(i * n + a)];
            if (e.i0 <= e.i1 && e.j0 <= e.j1) { index.push_back((int32_t)i); break; }
        }
    }
    if (index.empty()) return;
    const int TA = (int)index.size();
    const bool topk = rx == 0 && ry == 0 && ra == 0;  // every point is a peak: the fused top-k, no planes written

    // Regions (peaks only): the whole grid when a batch of min(n, 2ra + 1) planes -- one decided angle and its angle
    // halo -- fits the map workspace, else rectangles whose planes with their rx / ry halo do.
    const long long pts = (long long)((n == 1 ? kMapBytes : kRotMapBytes) / sizeof(float));
    const int need = std::min(n, 2 * ra + 1);
    int DX = g.nx, DY = g.ny;
    if (!topk && (long long)g.nx * g.ny * need > pts) {
        DY = std::min(g.ny, 2048);
        DX = (int)std::max<long long>(1, std::min<long long>(g.nx, pts / need / (DY + 2 * ry) - 2 * rx));
    }
    struct Region { int ia, ja, w, h, di0, di1, dj0, dj1; };
    std::vector<Region> regions;
    if (topk) {
        regions.push_back(Region{0, 0, g.nx, g.ny, 0, g.nx - 1, 0, g.ny - 1});
    } else {
        for (int rj = 0; rj < g.ny; rj += DY)
            for (int ri = 0; ri < g.nx; ri += DX) {
                const int ia = std::max(0, ri - rx), ib = std::min(g.nx - 1, ri + DX - 1 + rx);
                const int ja = std::max(0, rj - ry), jb = std::min(g.ny - 1, rj + DY - 1 + ry);
                regions.push_back(Region{ia, ja, ib - ia + 1, jb - ja + 1, ri - ia, std::min(g.nx - 1, ri + DX - 1) - ia, rj - ja,
                                         std::min(g.ny - 1, rj + DY - 1) - ja});
            }
    }
    long long plane_max = 0;
    for (const Region& R : regions) plane_max = std::max(plane_max, (long long)R.w * R.h);
    // planes per batch: the map workspace (peaks) or the candidate lists, (8 units + 8192) * 4 lists of k keys at most (top-k)
    int cap;
    if (topk)
        cap = (int)std::max<long long>(1, std::min<long long>(65536, ((long long)(kCandBytes / (32ull * k)) - 8192) / 8));
    else
        cap = (int)std::max<long long>(need, std::min<long long>(65536, pts / plane_max));

    // Batches: groups (one template's decided angles [a0, a1) and the planes of their angle halo, lo, lo + 1, ... mod n)
    // filled in template order; a template's angles are cut across batches when they do not fit.
    struct Group { int q, a0, a1, lo, np, plane0, unit0; };
    struct Batch { size_t g0, g1; int planes, units; };
    auto n_planes = [&](int a0, int a1) { return wrap ? std::min(n, a1 - a0 + 2 * ra) : std::min(n, a1 + ra) - std::max(0, a0 - ra); };
    std::vector<Group> groups;
    std::vector<Batch> batches;
    Batch cur{0, 0, 0, 0};
    for (int q = 0; q < TA; ++q) {
        int a0 = 0;
        while (a0 < n) {
            const int room = cap - cur.planes;
            int a1 = std::min(n, a0 + room);
            while (a1 > a0 && n_planes(a0, a1) > room) --a1;
            if (a1 == a0) {  // (cap >= need: an empty batch takes one angle)
                cur.g1 = groups.size();
                batches.push_back(cur);
                cur = Batch{groups.size(), 0, 0, 0};
                continue;
            }
            const int np = n_planes(a0, a1);
            const int lo = wrap ? (np == n ? 0 : ((a0 - ra) % n + n) % n) : std::max(0, a0 - ra);
            groups.push_back(Group{q, a0, a1, lo, np, cur.planes, cur.units});
            cur.planes += np;
            cur.units += a1 - a0;
            a0 = a1;
        }
    }
    if (cur.planes > 0) {
        cur.g1 = groups.size();
        batches.push_back(cur);
    }

    // Host arrays of every batch: per region its planes (boxes in the region's plane coordinates, lines in P.lines, slot =
    // the plane's place in the batch, koff = a * N), its decided units and its groups.
    std::vector<size_t> bt0(batches.size() + 1, 0), bd0(batches.size() + 1, 0), bs0(batches.size() + 1, 0);
    std::vector<ExTmpl> btm;
    std::vector<int4> bdec, bseg;
    std::vector<int> parts;  // workgroups per unit of each (batch, region)
    size_t max_planes = 1, max_cand = 1;
    for (size_t b = 0; b < batches.size(); ++b) {
        const Batch& B = batches[b];
        std::vector<ExTmpl> planes;  // full-grid boxes
        for (size_t gi = B.g0; gi < B.g1; ++gi) {
            const Group& G = groups[gi];
            const int64_t ti = index[(size_t)G.q];
            for (int p = 0; p < G.np; ++p) {
                const int a2 = (G.lo + p) % n;
                ExTmpl e = tm[(size_t)(ti * n + a2)];
                e.slot = G.plane0 + p;
                e.koff = (unsigned)((unsigned long long)a2 * N);
                planes.push_back(e);
            }
            bseg.push_back(make_int4(G.unit0, G.a1 - G.a0, G.q, 0));
            for (int a = G.a0; a < G.a1; ++a) bdec.push_back(make_int4(G.plane0, G.lo, G.np, a));
        }
        for (const Region& R : regions) {
            int max_tiles = 0;
            for (ExTmpl e : planes) {
                if (!topk) {
                    const int i0 = std::max(e.i0, R.ia) - R.ia, i1 = std::min(e.i1, R.ia + R.w - 1) - R.ia;
                    const int j0 = std::max(e.j0, R.ja) - R.ja, j1 = std::min(e.j1, R.ja + R.h - 1) - R.ja;
                    if (i0 <= i1 && j0 <= j1) {
                        e.i0 = i0; e.i1 = i1; e.j0 = j0; e.j1 = j1;
                        const int ci0 = std::max(i0, R.di0), ci1 = std::min(i1, R.di1), cj0 = std::max(j0, R.dj0),
                                  cj1 = std::min(j1, R.dj1);
                        if (ci0 <= ci1 && cj0 <= cj1)
                            max_tiles = std::max(max_tiles, ((ci1 - ci0) / kPkTX + 1) * ((cj1 - cj0) / kPkTY + 1));
                    } else {
                        e.i0 = 0; e.i1 = -1; e.j0 = 0; e.j1 = -1;
                    }
                }
                btm.push_back(e);
            }
            parts.push_back(topk ? 4 * portions_for(fm, g, B.planes)  // lists per unit
                                 : std::max(1, std::min(max_tiles, (kPeakWorkgroups + B.units - 1) / B.units)));
            max_cand = std::max(max_cand, (size_t)B.units * (topk ? parts.back() : 4 * parts.back()));
        }
        bt0[b + 1] = btm.size();
        bd0[b + 1] = bdec.size();
        bs0[b + 1] = bseg.size();
        max_planes = std::max(max_planes, (size_t)B.planes);
    }
    // Workspace: P's lines, the planes (all regions), units and groups of every batch and the merged lists, then the maps
    // and candidate lists.  The first part goes up in one asynchronous copy from pinned memory before any kernel of the
    // call, so no copy waits behind the call's own kernels.
    const size_t o_tm = al256(P.lines.size() * sizeof(ExLine)), o_dec = o_tm + al256(btm.size() * sizeof(ExTmpl)),
                 o_seg = o_dec + al256(bdec.size() * sizeof(int4)), o_best = o_seg + al256(bseg.size() * sizeof(int4)),
                 o_map = o_best + al256((size_t)TA * k * 8),
                 o_cand = o_map + (topk ? 0 : al256(max_planes * plane_max * sizeof(float))), total = o_cand + al256(max_cand * k * 8);
    reserve_eval(fm, total, o_map);
    char* d = (char*)fm->search.eval.p;
    char* h = (char*)fm->search.eval_stage.p;
    std::memcpy(h, P.lines.data(), P.lines.size() * sizeof(ExLine));
    std::memcpy(h + o_tm, btm.data(), btm.size() * sizeof(ExTmpl));
    std::memcpy(h + o_dec, bdec.data(), bdec.size() * sizeof(int4));
    std::memcpy(h + o_seg, bseg.data(), bseg.size() * sizeof(int4));
    std::memset(h + o_best, 0xff, (size_t)TA * k * 8);  // kNoKey
    hipStream_t st = fm->stream;
    FDCM_HIP(hipMemcpyAsync(d, h, o_map, hipMemcpyHostToDevice, st));
    float* map = (float*)(d + o_map);
    unsigned long long* cand = (unsigned long long*)(d + o_cand);
    unsigned long long* d_best = (unsigned long long*)(d + o_best);
    size_t at = 0;  // (batch, region) launches so far
    for (size_t b = 0; b < batches.size(); ++b) {
        const Batch& B = batches[b];
        const int n_groups = (int)(B.g1 - B.g0);
        const ExTmpl* d_tm = (const ExTmpl*)(d + o_tm) + bt0[b];
        const int4* d_dec = (const int4*)(d + o_dec) + bd0[b];
        const int4* d_seg = (const int4*)(d + o_seg) + bs0[b];
        for (size_t r = 0; r < regions.size(); ++r) {
            const Region& R = regions[r];
            const ExTmpl* tm = d_tm + r * (size_t)B.planes;
            const int G = parts[at++];
            int lpu;
            if (topk) {
                lpu = G;
                launch<kTopK>(fm, P, g, (const ExLine*)d, tm, B.planes, k, G / 4, nullptr, cand);
            } else {
                lpu = 4 * G;
                const fdcm_grid rg{g.x0 + R.ia * g.sx, g.y0 + R.ja * g.sy, R.w, R.h, g.sx, g.sy};
                launch<kMap>(fm, P, rg, (const ExLine*)d, tm, B.planes, 0, portions_for(fm, rg, B.planes), map, nullptr);
                // 32-bit keys in LDS when the angle window holds one plane: 4 workgroups per CU at R = 8 instead of 2.
                // That kernel reads plane u for unit u: with one plane per window every group has as many planes as units.
                if (need == 1 && B.planes != B.units) throw std::string("exhaustive search: batch planes and units differ");
                const bool small = std::max(rx, ry) <= 8;
                auto peaks = need > 1 ? (small ? k_exhaustive_peaks<8, true> : k_exhaustive_peaks<kMaxRadius, true>)
                                      : (small ? k_exhaustive_peaks<8, false> : k_exhaustive_peaks<kMaxRadius, false>);
                hipLaunchKernelGGL(peaks, dim3((unsigned)(B.units * G)), dim3(256), 0, st, map, R.w, R.h, tm, d_dec, G, rx, ry, ra, n,
                                   wrap, R.di0, R.di1, R.dj0, R.dj1, R.ia, R.ja, g.nx, (unsigned)N, k, cand);
                FDCM_HIP(hipGetLastError());
            }
            hipLaunchKernelGGL(k_exhaustive_merge_groups, dim3((unsigned)((n_groups + 3) / 4)), dim3(256), 0, st,
                               (const unsigned long long*)cand, d_seg, n_groups, lpu, k, d_best);
            FDCM_HIP(hipGetLastError());
        }
    }
    best.resize((size_t)TA * k);
    FDCM_HIP(hipMemcpyAsync(best.data(), d_best, best.size() * 8, hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipStreamSynchronize(st));  // (the host arrays stay alive until here)
}

// ---- best map and detections: the host driver (include/fdcm.h, "Best map and detections")
constexpr int kBestPeakWorkgroups = 256;  // peak workgroups of the one plane: one wave folds their 4 lists each

// The penalty's denominator per template, on the host as run_topk_device's: max(len, 1e-6f), or std::pow of that and tau;
// 1 without a penalty (a division by 1 leaves every score as it is).
std::vector<float> best_denominators(const fdcm_templates* t, int penalty, float tau) {
    std::vector<float> den((size_t)t->T, 1.f);
    if (penalty < 0 || t->T == 0) return den;
    if (fdcm_templates_lengths(t, den.data()) != FDCM_OK) throw std::string(fdcm_last_error());
    for (float& v : den) {
        const float l = std::max(v, 1e-6f);
        v = penalty == FDCM_DEFAULT_PENALTY ? l : std::pow(l, tau);
    }
    return den;
}

// B of include/fdcm.h, "All detections below a score": the largest float32 s >= +0, possibly +inf, whose IEEE float32
// quotient s / den is <= max_score.  The quotient rises with s, so the patterns that pass are a prefix of 0 .. +inf's: the
// last one by bisection, as axis_interval.  (A denominator that is 0, infinite or NaN breaks that at the ends alone: +inf
// when +inf passes, 0 when +0 does not.)
float score_bound(float den, float max_score) {
    auto ok = [&](uint32_t b) { return f_from_bits(b) / den <= max_score; };
    const uint32_t inf = 0x7f800000u;
    if (ok(inf)) return f_inf();
    if (!ok(0)) return 0.f;
    uint32_t lo = 0, hi = inf - 1;  // the last pattern that passes
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (ok(mid)) lo = mid; else hi = mid - 1;
    }
    return f_from_bits(lo);
}

// The bound rows_score's exit compares a partial sum with: B / (1 - 2 n u), u = 2^-24, rounded
// upward, for a template of n lines.  A partial sum C of terms >= +0 is at most (1 + u)^(n-1) times their exact sum and the
// finished float32 sum at least (1 - u)^(n-1) times the exact sum of all terms, so C > this bound puts the finished sum
// above B.  +inf, the exit switched off, for an infinite B, for n > 2^20 (the factor has lost its meaning long before 2 n u
// reaches 1) and for a bound above 1e38 (a partial sum that overflowed then still proves its point).
constexpr int kExitMaxLines = 1 << 20;
float exit_bound(float B, int n) {
    if (!(B < f_inf()) || n > kExitMaxLines) return f_inf();
    const double f = (double)B / (1.0 - 2.0 * (double)n * 0x1p-24);
    float c = (float)f;
    if ((double)c < f) c = std::nextafter(c, f_inf());
    c = std::nextafter(c, f_inf());  // the double quotient's own rounding
    return c > 1e38f ? f_inf() : c;
}

// What the calls with objects (include/fdcm.h, "Objects") take beside their siblings' arguments.
struct ObjectsIn {
    const int32_t* objects;    // per template
    int G;
    const float* max_score;    // per object
    const float* min_matched;  // per object, or null: all 0
    int cross;                 // the limit between entries of different objects, in permille
};

// TL and the gate's need for every entry e < T n of a call, entry e being template e / n's (the pairs of a dense call; n = 1:
// the templates themselves): tl[e] = TL of its template and, with `needs`, need[e] = float32(min_matched_of(template) * TL),
// one multiply.
template <class MinMatchedOf>
static void matched_needs(const fdcm_templates* t, size_t n, bool needs, MinMatchedOf min_matched_of, std::vector<float>& tl,
                          std::vector<float>& need) {
    std::vector<float> totals((size_t)t->T);
    templates_matched_totals(t, totals.data());
    tl.resize(totals.size() * n);
    for (size_t e = 0; e < tl.size(); ++e) tl[e] = totals[e / n];
    if (!needs) return;
    need.resize(tl.size());
    for (size_t e = 0; e < tl.size(); ++e) need[e] = min_matched_of(e / n) * tl[e];
}

constexpr size_t kNmsPartialBytes = 2 * kNmsWorkgroups * (8 + 4);  // two sets of partial minima: the keys, then the pairs

// ---- the key planes of a dense call, and its workspace
// What a dense call asks of dense_keys.  The single calls are the case G = 1 of the calls with objects: without `ob` the one
// object has all templates, the threshold max_score (+inf: none) and the gate min_matched.
struct DenseIn {
    const ObjectsIn* ob = nullptr;
    float max_score = f_inf(), min_matched = 0.f;  // (without ob)
    bool gate_all = false;  // the kind of gate, "Gate inside the minimum": the needs go to the scoring kernel, its gated form;
                            // else they wait for k_matched_gate
    const std::vector<Foot>* foot = nullptr;  // a footprint per pair, for the rounds of the overlap rule
    int list = kMaxK;                         // the entries of the result list and of its pairs
    int k = 0;                                // > 0: also what the peak pass needs (run_search_exhaustive_detect)
    bool planes4 = false;                     // the G 4-byte planes a best map stages its downloads in
    bool want_tl = false;                     // the fractions: TL per pair, and a float per entry of the list
    size_t hull_bytes = 0;                    // (hull footprints) HullRun's tables
};

// Where dense_keys left what: offsets into d = search.eval.  Everything before o_pair is written by the one upload.
struct DenseRun {
    char* d = nullptr;
    size_t o_tm = 0, o_unit = 0, o_seg = 0, o_foot = 0, o_pobj = 0, o_len = 0, o_need = 0, o_tl = 0, o_best = 0;
    size_t o_pair = 0, o_frac = 0, o_keys = 0, o_plane = 0, o_cand = 0, o_hull = 0;
    size_t n_keys = 0;
    int tiles_x = 0, parts = 0, G = 1;
    bool objects = false;  // the call has objects: their per-pair table is at o_pobj when there are footprints
};

// Scores every pair of P (T templates x n rotations, prepared) on the grid and leaves, on the device, the G merged key
// planes of the call, one per object, one behind the other at o_keys: n_keys keys each in sub-tile order, all set to "no key"
// once, then one launch chain of k_exhaustive<., kBest*> per object over that object's pairs into that object's plane, with
// that object's threshold (only the points with q <= max_score get a key; +inf: the kernel without the checks) and, under
// gate_all, that object's needs.  Pairs of templates without lines take no part; an object without templates queues nothing
// and keeps an empty plane.  Returns false, with nothing queued or reserved, when no pair has a grid point: every point is
// then without a candidate.
//
// The workspace is the list `blocks` below, in that order, each block aligned to 256 bytes and absent (0 bytes) unless its
// condition holds.  One upload writes the blocks up to the result list: the lines (at 0); the template records by pair,
// each with slot = its pair, which the kernels that look a pair up read (k_matched_gate, k_matched_plane, k_matched_list),
// followed by the peak pass's unit; with objects the same records object by object, for the launch chains (the scoring
// kernels read their bounds and needs by slot and write the slot into the key; without objects pair order is that order, and
// the chain reads the records by pair); the peak pass's group; the footprints and with objects the object of every pair,
// for the rounds; the exit bound of every pair when an object has a threshold; P.len; the needs when an object has a gate;
// TL; the result list, all "no key".  Behind them, written by kernels alone: the pairs and the fractions of the list's
// entries, the key planes, the 4-byte planes (the peak pass's score plane is one), the partial minima of the rounds or the
// peak pass's candidate lists, and the hull tables, which go up in a second copy staged behind the first one's bytes.
bool dense_keys(fdcm_featuremap* fm, const Pairs& P, const fdcm_templates* t, int n, const fdcm_grid& g, int penalty, float tau,
                const DenseIn& in, DenseRun& R) {
    const std::vector<float> den = best_denominators(t, penalty, tau);
    const size_t np = P.nl.size();
    const ObjectsIn* ob = in.ob;
    const int G = ob ? ob->G : 1;
    const float* ms = ob ? ob->max_score : &in.max_score;
    const float* mm = ob ? ob->min_matched : &in.min_matched;
    auto obj_of = [&](size_t u) { return ob ? ob->objects[u / (size_t)n] : 0; };
    const bool bounded = std::any_of(ms, ms + G, [](float v) { return v < f_inf(); });
    const bool gated = mm && std::any_of(mm, mm + G, [](float v) { return v > 0.f; });
    std::vector<float> bc(bounded ? np : 0);
    for (size_t u = 0; u < bc.size(); ++u) bc[u] = exit_bound(score_bound(den[u / (size_t)n], ms[obj_of(u)]), P.nl[u]);
    std::vector<ExTmpl> tm(np + 1), sorted(ob ? np : 0);
    std::vector<int32_t> pobj(ob ? np : 0);
    std::vector<size_t> start((size_t)G + 1, 0);  // the pairs of object o: [start[o], start[o + 1]) of the records by object
    bool any = false;
    for (size_t u = 0; u < np; ++u) {
        ExTmpl e = grid_tmpl(P, u, g, (int)u);
        if (e.n == 0) { e.i0 = 0; e.i1 = -1; e.j0 = 0; e.j1 = -1; }
        e.koff = bits_from_f(den[u / (size_t)n]);
        any = any || (e.i0 <= e.i1 && e.j0 <= e.j1);
        tm[u] = e;
        if (ob) pobj[u] = obj_of(u);
        ++start[(size_t)obj_of(u) + 1];
    }
    if (!any) return false;
    for (int o = 0; o < G; ++o) start[(size_t)o + 1] += start[(size_t)o];
    if (ob) {
        std::vector<size_t> at(start.begin(), start.end() - 1);
        for (size_t u = 0; u < np; ++u) sorted[at[(size_t)pobj[u]]++] = tm[u];  // (pair order inside an object)
    }
    tm[np] = ExTmpl{0, 0, 0, g.nx - 1, 0, g.ny - 1, 0, 0};  // the peak pass's unit: the score plane, its box the whole grid
    const int4 seg = make_int4(0, 1, 0, 0);
    std::vector<float> need, tl;
    if (gated || in.want_tl) matched_needs(t, (size_t)n, gated, [&](size_t i) { return mm[ob ? ob->objects[i] : 0]; }, tl, need);
    R.G = G;
    R.objects = ob != nullptr;
    R.tiles_x = (g.nx + kTileX - 1) / kTileX;
    const size_t n_keys = R.n_keys = (size_t)R.tiles_x * (size_t)((g.ny + kTileY - 1) / kTileY) * (kTileX * kTileY);
    const size_t N = (size_t)g.nx * g.ny, list = (size_t)in.list;
    const int max_tiles = ((g.nx - 1) / kPkTX + 1) * ((g.ny - 1) / kPkTY + 1);
    R.parts = std::max(1, std::min(max_tiles, kBestPeakWorkgroups));
    const bool peaks = in.k > 0, foot = in.foot != nullptr;
    size_t o_lines = 0, o_sorted = 0, o_bc = 0;
    struct Block { size_t* at; size_t bytes; const void* src; };  // src: what the upload carries there
    const Block blocks[] = {
        {&o_lines, P.lines.size() * sizeof(ExLine), P.lines.data()},
        {&R.o_tm, (np + (peaks ? 1 : 0)) * sizeof(ExTmpl), tm.data()},
        {&o_sorted, sorted.size() * sizeof(ExTmpl), sorted.data()},  // (np records with objects, else none)
        {&R.o_seg, peaks ? sizeof seg : 0, &seg},
        {&R.o_foot, foot ? np * sizeof(Foot) : 0, foot ? in.foot->data() : nullptr},
        {&R.o_pobj, foot ? pobj.size() * sizeof(int32_t) : 0, pobj.data()},  // (np entries with objects, else none)
        {&o_bc, bc.size() * sizeof(float), bc.data()},             // (np floats when an object has a threshold, else none)
        {&R.o_len, P.len.size() * sizeof(float), P.len.data()},    // (a float per line when the caller set P.lens, else none)
        {&R.o_need, need.size() * sizeof(float), need.data()},     // (np floats when an object has min_matched > 0, else none)
        {&R.o_tl, in.want_tl ? np * sizeof(float) : 0, tl.data()},
        {&R.o_best, list * 8, nullptr},  // kNoKey, below
        {&R.o_pair, list * 4, nullptr},  // the upload ends here
        {&R.o_frac, in.want_tl ? list * 4 : 0, nullptr},
        {&R.o_keys, (size_t)G * n_keys * 8, nullptr},
        {&R.o_plane, in.planes4 || peaks ? (size_t)G * N * 4 : 0, nullptr},
        {&R.o_cand, foot ? kNmsPartialBytes : peaks ? (size_t)4 * R.parts * in.k * 8 : 0, nullptr},
        {&R.o_hull, in.hull_bytes, nullptr},
    };
    size_t end = 0;
    for (const Block& b : blocks) {
        *b.at = end;
        end += al256(b.bytes);
    }
    R.o_unit = R.o_tm + np * sizeof(ExTmpl);
    reserve_eval(fm, end, R.o_pair + in.hull_bytes);
    char* d = R.d = (char*)fm->search.eval.p;
    char* h = (char*)fm->search.eval_stage.p;
    for (const Block& b : blocks)
        if (b.src && b.bytes) std::memcpy(h + *b.at, b.src, b.bytes);
    std::memset(h + R.o_best, 0xff, list * 8);  // kNoKey
    hipStream_t st = fm->stream;
    FDCM_HIP(hipMemcpyAsync(d, h, R.o_pair, hipMemcpyHostToDevice, st));
    FDCM_HIP(hipMemsetAsync(d + R.o_keys, 0xff, (size_t)G * n_keys * 8, st));  // no key anywhere, in any plane
    const ExTmpl* by_object = (const ExTmpl*)(d + (ob ? o_sorted : R.o_tm));
    for (int o = 0; o < G; ++o) {
        const int cnt = (int)(start[(size_t)o + 1] - start[(size_t)o]);
        if (cnt == 0) continue;
        const bool bound_o = ms[o] < f_inf(), need_o = in.gate_all && gated && mm[o] > 0.f;
        launch<kBest>(fm, P, g, (const ExLine*)d, by_object + start[(size_t)o], cnt, 0, portions_for(fm, g, cnt), nullptr,
                      (unsigned long long*)(d + R.o_keys) + (size_t)o * n_keys, bound_o ? (const float*)(d + o_bc) : nullptr,
                      bound_o ? ms[o] : 0.f, need_o ? (const float*)(d + R.o_need) : nullptr);
    }
    return true;
}

// Plane o of the call's key planes as a plane of scores or of pairs (k_best_unpack).
void best_unpack(fdcm_featuremap* fm, const DenseRun& R, const fdcm_grid& g, int o, float* score, int* pair) {
    hipLaunchKernelGGL(k_best_unpack, dim3((unsigned)((g.nx + 63) / 64), (unsigned)((g.ny + 3) / 4)), dim3(256), 0, fm->stream,
                       (const unsigned long long*)(R.d + R.o_keys) + (size_t)o * R.n_keys, g.nx, g.ny, R.tiles_x, score, pair);
    FDCM_HIP(hipGetLastError());
}

// The records of the detections (include/fdcm.h, "Best map and detections"): downloads the list of k keys (bits of q << 32)
// | g at o_best and the pairs of its entries at o_pair, waits for the stream, and emits entry l as the pair t n + a = pair[l]
// at the grid point of its key (kNoKey ends the list).  foot and boxes_out (or null): the footprint of each pair; the
// footprint of record l, F(g) = foot[pair[l]] + t_g, goes to boxes_out[4 l ..].  matched_out (or null): the k floats
// k_matched_list left at o_frac, of which the first *n_out are the records' fractions.
void detect_records(fdcm_featuremap* fm, const DenseRun& R, const Pairs& P, bool rotated, int n, const fdcm_grid& g, int k, int32_t base,
                    fdcm_match** out, int64_t* n_out, const Foot* foot, int32_t* boxes_out, float* matched_out = nullptr) {
    hipStream_t st = fm->stream;
    std::vector<unsigned long long> best((size_t)k);
    std::vector<int32_t> pair((size_t)k);
    FDCM_HIP(hipMemcpyAsync(best.data(), R.d + R.o_best, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipMemcpyAsync(pair.data(), R.d + R.o_pair, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    if (matched_out) FDCM_HIP(hipMemcpyAsync(matched_out, R.d + R.o_frac, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipStreamSynchronize(st));
    int64_t cnt = 0;
    while (cnt < k && best[(size_t)cnt] != kNoKey) ++cnt;
    fdcm_match* m = result_acquire((size_t)std::max<int64_t>(1, cnt) * sizeof(fdcm_match));
    for (int64_t l = 0; l < cnt; ++l) {
        const unsigned gi = (unsigned)best[(size_t)l];
        const int px = g.x0 + (int)(gi % (unsigned)g.nx) * g.sx, py = g.y0 + (int)(gi / (unsigned)g.nx) * g.sy;
        const float tx = (float)px, ty = (float)py;
        fdcm_match& rec = m[l];
        rec.tmpl_idx = base + pair[(size_t)l] / n;
        rec.score = f_from_bits((uint32_t)(best[(size_t)l] >> 32));
        if (rotated) {  // combine(translation, M_a), float32 adds: emit_records' rule
            const RotM& M = P.M[(size_t)pair[(size_t)l]];
            rec.transform[0] = M.c; rec.transform[1] = M.ns; rec.transform[2] = M.mx + tx;
            rec.transform[3] = M.s; rec.transform[4] = M.c; rec.transform[5] = M.my + ty;
        } else {
            rec.transform[0] = 1.f; rec.transform[1] = 0.f; rec.transform[2] = tx;
            rec.transform[3] = 0.f; rec.transform[4] = 1.f; rec.transform[5] = ty;
        }
        if (boxes_out) {
            const Foot& F = foot[(size_t)pair[(size_t)l]];
            int32_t* b = boxes_out + 4 * l;
            b[0] = F.x0 + px; b[1] = F.y0 + py; b[2] = F.x1 + px; b[3] = F.y1 + py;
        }
    }
    *out = m;
    *n_out = cnt;
}

// The footprint of the n lines at p (4 floats each, `stride` floats apart) with a margin: floor of the smallest and the
// largest end point coordinate, widened by the margin, clamped to +-2^25; (0, 0, -1, -1) without lines or with a NaN.
Foot footprint(const float* p, size_t stride, int64_t n, int margin) {
    const Foot none{0, 0, -1, -1};
    if (n == 0) return none;
    float mnx = f_inf(), mxx = -f_inf(), mny = f_inf(), mxy = -f_inf();
    for (int64_t q = 0; q < n; ++q, p += stride)
        for (int c = 0; c < 2; ++c) {
            if (std::isnan(p[2 * c]) || std::isnan(p[2 * c + 1])) return none;
            mnx = std::min(mnx, p[2 * c]); mxx = std::max(mxx, p[2 * c]);
            mny = std::min(mny, p[2 * c + 1]); mxy = std::max(mxy, p[2 * c + 1]);
        }
    const int64_t lim = (int64_t)1 << 25;
    auto at = [&](float v, int64_t d) {  // floor(v) + d in int64 (an infinite v: far outside the clamp), clamped
        const double f = std::min(std::max(std::floor((double)v), -1099511627776.0), 1099511627776.0);
        return (int32_t)std::min(std::max((int64_t)f + d, -lim), lim);
    };
    return Foot{at(mnx, -margin), at(mny, -margin), at(mxx, margin), at(mxy, margin)};
}

// ---- hull footprints: the host's tables (include/fdcm.h, "Hull footprints")
struct HullPt { int64_t x, y; };

// The convex hull of the vertices of the n lines at p (footprint's arguments): per end point the four corners
// clamp(floor(v) -+ margin), the box's own arithmetic, so the hull's box is the footprint.  Counter-clockwise without
// collinear points (monotone chain, cross products below 2^55); one point, or two for collinear vertices; empty for the
// empty shape.
void hull_of(const float* p, size_t stride, int64_t n, int margin, std::vector<HullPt>& h) {
    h.clear();
    std::vector<HullPt> v;
    const int64_t lim = (int64_t)1 << 25;
    auto at = [&](float c, int64_t d) {  // (footprint's)
        const double f = std::min(std::max(std::floor((double)c), -1099511627776.0), 1099511627776.0);
        return std::min(std::max((int64_t)f + d, -lim), lim);
    };
    for (int64_t q = 0; q < n; ++q, p += stride)
        for (int c = 0; c < 2; ++c) {
            if (std::isnan(p[2 * c]) || std::isnan(p[2 * c + 1])) return;
            for (int k = 0; k < (margin ? 4 : 1); ++k)
                v.push_back(HullPt{at(p[2 * c], k & 1 ? margin : -margin), at(p[2 * c + 1], k & 2 ? margin : -margin)});
        }
    std::sort(v.begin(), v.end(), [](const HullPt& a, const HullPt& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
    v.erase(std::unique(v.begin(), v.end(), [](const HullPt& a, const HullPt& b) { return a.x == b.x && a.y == b.y; }), v.end());
    if (v.size() < 3) { h = v; return; }
    auto cross = [](const HullPt& o, const HullPt& a, const HullPt& b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); };
    h.resize(2 * v.size());
    size_t k = 0;
    for (size_t i = 0; i < v.size(); ++i) {  // lower chain
        while (k >= 2 && cross(h[k - 2], h[k - 1], v[i]) <= 0) --k;
        h[k++] = v[i];
    }
    for (size_t i = v.size() - 1, t = k + 1; i > 0; --i) {  // upper chain
        while (k >= t && cross(h[k - 2], h[k - 1], v[i - 1]) <= 0) --k;
        h[k++] = v[i - 1];
    }
    h.resize(k - 1);  // (the last point is the first)
}

// The rows of the shape whose box is F (footprint's, at the same margin): per row of the box xl = ceil(min x*), xr =
// floor(max x*) over the hull's edges that reach the row, in the box's frame, (0, -1) for an empty row; into spans (2 int32
// per row, or null).  The ends of a row of a convex polygon lie on its boundary, so the edges give what all vertex pairs give.
// Returns the area.
int64_t hull_rows(const std::vector<HullPt>& h, const Foot& F, int32_t* spans) {
    int64_t area = 0;
    const size_t m = h.size();
    for (int64_t y = F.y0; y <= F.y1 && m > 0; ++y) {
        int64_t xl = INT64_MAX, xr = INT64_MIN;
        for (size_t e = 0; e < m; ++e) {
            HullPt a = h[e], b = h[(e + 1) % m];
            if (a.y > b.y) std::swap(a, b);
            if (y < a.y || y > b.y) continue;
            if (a.y == b.y) {
                xl = std::min({xl, a.x, b.x});
                xr = std::max({xr, a.x, b.x});
            } else {  // x* = num / dy, exact
                const int64_t dy = b.y - a.y, num = a.x * dy + (b.x - a.x) * (y - a.y);
                xl = std::min<int64_t>(xl, -floor_div(-num, dy));
                xr = std::max<int64_t>(xr, floor_div(num, dy));
            }
        }
        const bool none = xl > xr;
        if (!none) area += xr - xl + 1;
        if (spans) {
            int32_t* s = spans + 2 * (y - F.y0);
            s[0] = none ? 0 : (int32_t)(xl - F.x0);
            s[1] = none ? -1 : (int32_t)(xr - F.x0);
        }
    }
    return area;
}

int64_t foot_rows(const Foot& F) { return F.y1 < F.y0 ? 0 : (int64_t)F.y1 - F.y0 + 1; }

constexpr int64_t kHullMaxRows = (int64_t)1 << 26;  // of one call's span table: 512 MB

// The shapes of the pairs of P, whose boxes are foot: the rows each has in the table (row0) first, so that the table can be
// sized; then, while the device scores, the areas and the spans, written where the upload reads them.
size_t hull_layout(const std::vector<Foot>& foot, std::vector<HullShape>& shapes) {
    shapes.assign(foot.size(), HullShape{0, 0, 0});
    int64_t rows = 0;
    for (size_t u = 0; u < foot.size(); ++u) {
        shapes[u].row0 = (int)rows;
        rows += foot_rows(foot[u]);
        if (rows > kHullMaxRows) throw std::string("hull footprints: the span table of the call has more than 2^26 rows");
    }
    return (size_t)rows;
}

void hull_fill(const Pairs& P, const std::vector<Foot>& foot, int margin, HullShape* shapes, int32_t* spans) {
    const size_t np = foot.size();
    const int nth = (int)std::max<size_t>(1, std::min<size_t>({16, np, P.lines.size() >> 10}));
    on_threads(nth, "host preparation of the hull footprints failed", [&](int c) {
        std::vector<HullPt> h;
        for (size_t u = np * (size_t)c / (size_t)nth; u < np * (size_t)(c + 1) / (size_t)nth; ++u) {
            hull_of((const float*)(P.lines.data() + P.line0[u]), sizeof(ExLine) / sizeof(float), P.nl[u], margin, h);
            shapes[u].area = hull_rows(h, foot[u], spans + 2 * (size_t)shapes[u].row0);
        }
    });
}

// ---- pose windows: the host driver
constexpr int kWinPlanes = 65536;       // planes of a batch, at most (a batch always takes one job)
constexpr int kWinItems = 1 << 20;      // patches of a batch, at most (a job has 2^16 at most)
constexpr int kWinWaves = 16384;        // waves of a launch, about: twice what is resident at 8 waves per SIMD
constexpr size_t kWinStageBytes = (size_t)256 << 20;  // what one upload holds, about: longer job lists go in rounds

// What the detections over pose windows add to a round (k = 1): after the last merge k_window_winners turns the round's
// merged lists into the jobs' entries of the winners' list, which come down with the lists.
struct WinnersIn {
    const float* den;          // per template: the denominator of q
    const float* need;         // per template: the gate's need, or null without a gate
    bool gate_all;             // the gate inside the minimum (k_exhaustive_windows' GATE); else k_window_winners applies it
    int margin;                // of the footprints
    float max_score;
    unsigned long long* keys;  // per job of the call, on the host: (bits of q << 32) | job, or kNoKey
    Foot* boxes;               // .. F(job)
    const float* ms = nullptr;  // ("Objects") per template: the threshold of its object, in max_score's place (k_window_winners_objects)
};

// The jobs [j0, j1) of a call: their pairs prepared, their planes cut into batches, one upload, two kernels per batch and
// the download of the jobs' merged lists into best[j0 k ..].  Mjob[m0[j] + e]: the transform of job j's run position e.
// flat: the 64-bit form of VolRef whatever the volume's size.  wn (or null): the winners' pass, see WinnersIn.
void windows_round(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_pose_window* jobs, int64_t j0,
                   int64_t j1, int sx, int sy, int k, unsigned long long* best, const std::vector<int64_t>& m0, std::vector<RotM>& Mjob,
                   bool flat, const WinnersIn* wn = nullptr) {
    const int n = rot ? rot->n : 1;
    Pairs W;
    const bool gate_all = wn && wn->need && wn->gate_all;
    W.lens = wn && wn->need && !gate_all;
    if (wn) W.foot_margin = wn->margin;
    for (int64_t j = j0; j < j1; ++j)
        for (int e = 0; e < jobs[j].na; ++e) W.key.push_back((int64_t)jobs[j].tmpl * n + (jobs[j].a0 + e) % n);
    std::sort(W.key.begin(), W.key.end());
    W.key.erase(std::unique(W.key.begin(), W.key.end()), W.key.end());
    prepare_pairs(fm, t, rot, flat, W);
    std::vector<WinnerJob> wjob;  // (winners only) per job of the round, and the pair of each of its run positions
    std::vector<int> wrun;

    // Batches of whole jobs.  Per batch: its planes and their patches (job by job, run position by run position, a box's
    // patches along j first), per job with patches its first wave and candidate list, and its group for the merge
    // (x: first list, y: lists, z: the job's merged list).
    struct Batch { size_t p0, i0, b0, s0; int items, jobs, groups, ipw, waves, lists; };
    std::vector<Batch> batches;
    std::vector<WinPlane> planes;
    std::vector<int2> items;
    std::vector<WinJob> jtab;
    std::vector<int4> seg;
    struct Span { int first, count, job; };
    std::vector<Span> span;  // per job of the open batch: its first patch, its patches, its place in the round
    const int cap = test_switches().windows_batch > 0 ? test_switches().windows_batch : kWinPlanes;
    Batch cur{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int cur_planes = 0;
    size_t max_lists = 1;
    auto close = [&]() {
        if (cur.items > 0) {
            cur.ipw = std::max(1, (cur.items + kWinWaves - 1) / kWinWaves);
            cur.waves = (cur.items + cur.ipw - 1) / cur.ipw;
            for (int b = 0; b < cur.jobs; ++b) {
                const Span sp = span[(size_t)b];
                const int wave0 = sp.first / cur.ipw, lists = sp.count ? (sp.first + sp.count - 1) / cur.ipw - wave0 + 1 : 0;
                jtab.push_back(WinJob{wave0, cur.lists});
                if (lists) seg.push_back(make_int4(cur.lists, lists, sp.job, 0));
                cur.lists += lists;
            }
            cur.groups = (int)(seg.size() - cur.s0);
            max_lists = std::max(max_lists, (size_t)cur.lists);
            batches.push_back(cur);
        }  // (no patches: no planes either, nothing to launch, the jobs' lists stay empty)
        cur = Batch{planes.size(), items.size(), jtab.size(), seg.size(), 0, 0, 0, 0, 0, 0};
        cur_planes = 0;
        span.clear();
    };
    for (int64_t j = j0; j < j1; ++j) {
        const fdcm_pose_window& J = jobs[j];
        std::vector<WinPlane> jp;
        long long ji = 0;
        if (wn) wjob.push_back(WinnerJob{(int)wrun.size(), J.x0, J.y0, J.nx, (unsigned)(J.nx * J.ny), {0, 0, 0}});
        for (int e = 0; e < J.na; ++e) {
            const size_t u = W.find((int64_t)J.tmpl * n + (J.a0 + e) % n);
            if (wn) wrun.push_back((int)u);
            if (rot) Mjob[(size_t)(m0[(size_t)j] + e)] = W.M[u];
            if (W.nl[u] == 0 || !W.box[u].any) continue;  // a template without lines gives nothing
            WinPlane P{W.line0[u], W.nl[u], 0, -1, 0, -1, J.x0, J.y0, J.nx, (unsigned)((long long)e * J.nx * J.ny), 0,
                       gate_all ? wn->need[(size_t)J.tmpl] : 0.f};
            grid_range(W.box[u].x0, W.box[u].x1, J.x0, J.nx, sx, P.i0, P.i1);
            grid_range(W.box[u].y0, W.box[u].y1, J.y0, J.ny, sy, P.j0, P.j1);
            if (P.i0 > P.i1 || P.j0 > P.j1) continue;
            ji += (long long)((P.i1 - P.i0) / kPatchX + 1) * ((P.j1 - P.j0) / kPatchY + 1);
            jp.push_back(P);
        }
        if (cur.jobs > 0 && (cur_planes + J.na > cap || cur.items + ji > kWinItems)) close();
        span.push_back(Span{cur.items, (int)ji, (int)(j - j0)});
        for (WinPlane& P : jp) {
            P.job = cur.jobs;
            const int npi = (P.i1 - P.i0) / kPatchX + 1, npj = (P.j1 - P.j0) / kPatchY + 1;
            for (int pi = 0; pi < npi; ++pi)
                for (int pj = 0; pj < npj; ++pj) items.push_back(make_int2((int)(planes.size() - cur.p0), (pj << 16) | pi));
            planes.push_back(P);
        }
        cur.items += (int)ji;
        cur.jobs += 1;
        cur_planes += J.na;
    }
    close();
    const size_t nj = (size_t)(j1 - j0);
    if (batches.empty()) return;  // (best is kNoKey already)

    // One pinned buffer, one asynchronous copy: lines, planes, patches, job and group tables and the merged lists; the
    // candidate lists of one batch follow on the device.
    // The winners' pass: per pair its lines, denominator (koff), footprint and need, the line lengths (with a gate), the
    // jobs' grids and runs go up with the rest; the round's part of the list follows the candidate lists on the device.
    const size_t np = W.nl.size();
    std::vector<ExTmpl> wtm(wn ? np : 0);
    std::vector<float> wneed(wn && wn->need && !gate_all ? np : 0);
    std::vector<float> wms(wn && wn->ms ? np : 0);
    for (size_t u = 0; u < wtm.size(); ++u) {
        const size_t tmpl = (size_t)(W.key[u] / n);
        wtm[u] = ExTmpl{W.line0[u], W.nl[u], 0, -1, 0, -1, 0, bits_from_f(wn->den[tmpl])};
        if (!wneed.empty()) wneed[u] = wn->need[tmpl];
        if (!wms.empty()) wms[u] = wn->ms[tmpl];
    }
    const size_t o_pl = al256(W.lines.size() * sizeof(ExLine)), o_it = o_pl + al256(planes.size() * sizeof(WinPlane)),
                 o_jt = o_it + al256(items.size() * sizeof(int2)), o_seg = o_jt + al256(jtab.size() * sizeof(WinJob)),
                 o_wtm = o_seg + al256(seg.size() * sizeof(int4)), o_wfoot = o_wtm + al256(wtm.size() * sizeof(ExTmpl)),
                 o_wneed = o_wfoot + al256(W.foot.size() * sizeof(Foot)), o_wlen = o_wneed + al256(wneed.size() * sizeof(float)),
                 o_wjob = o_wlen + (W.lens ? al256(W.len.size() * sizeof(float)) : 0), o_wrun = o_wjob + al256(wjob.size() * sizeof(WinnerJob)),
                 o_wms = o_wrun + al256(wrun.size() * sizeof(int)), o_best = o_wms + al256(wms.size() * sizeof(float)),
                 o_cand = o_best + al256(nj * k * 8),
                 o_wkeys = o_cand + al256(max_lists * k * 8), o_wboxes = o_wkeys + (wn ? al256(nj * 8) : 0),
                 total = o_wboxes + (wn ? al256(nj * sizeof(Foot)) : 0);
    reserve_eval(fm, total, o_cand);
    char* d = (char*)fm->search.eval.p;
    char* h = (char*)fm->search.eval_stage.p;
    std::memcpy(h, W.lines.data(), W.lines.size() * sizeof(ExLine));
    std::memcpy(h + o_pl, planes.data(), planes.size() * sizeof(WinPlane));
    std::memcpy(h + o_it, items.data(), items.size() * sizeof(int2));
    std::memcpy(h + o_jt, jtab.data(), jtab.size() * sizeof(WinJob));
    std::memcpy(h + o_seg, seg.data(), seg.size() * sizeof(int4));
    if (wn) {
        std::memcpy(h + o_wtm, wtm.data(), wtm.size() * sizeof(ExTmpl));
        std::memcpy(h + o_wfoot, W.foot.data(), W.foot.size() * sizeof(Foot));
        std::memcpy(h + o_wneed, wneed.data(), wneed.size() * sizeof(float));
        if (W.lens) std::memcpy(h + o_wlen, W.len.data(), W.len.size() * sizeof(float));
        std::memcpy(h + o_wjob, wjob.data(), wjob.size() * sizeof(WinnerJob));
        std::memcpy(h + o_wrun, wrun.data(), wrun.size() * sizeof(int));
        std::memcpy(h + o_wms, wms.data(), wms.size() * sizeof(float));
    }
    std::memset(h + o_best, 0xff, nj * k * 8);  // kNoKey
    hipStream_t st = fm->stream;
    FDCM_HIP(hipMemcpyAsync(d, h, o_cand, hipMemcpyHostToDevice, st));
    unsigned long long* cand = (unsigned long long*)(d + o_cand);
    unsigned long long* d_best = (unsigned long long*)(d + o_best);
    const float* vol = fm->vol.as<float>();
    for (const Batch& B : batches) {
        // (the gated form always clamps: caps of +inf change no term)
        auto kern = gate_all ? (W.buf32 ? k_exhaustive_windows<true, true, true> : k_exhaustive_windows<false, true, true>)
                    : W.capped ? (W.buf32 ? k_exhaustive_windows<true, true> : k_exhaustive_windows<false, true>)
                               : (W.buf32 ? k_exhaustive_windows<true, false> : k_exhaustive_windows<false, false>);
        hipLaunchKernelGGL(kern, dim3((unsigned)((B.waves + 3) / 4)), dim3(256), 0, st, vol, W.SL, (int)fm->m, (int)fm->W, (int)fm->H, fm->tx,
                           fm->ty, (const ExLine*)d, (const WinPlane*)(d + o_pl) + B.p0, (const int2*)(d + o_it) + B.i0,
                           (const WinJob*)(d + o_jt) + B.b0, B.items, B.ipw, sx, sy, k, cand);
        FDCM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_exhaustive_merge_groups, dim3((unsigned)((B.groups + 3) / 4)), dim3(256), 0, st,
                           (const unsigned long long*)cand, (const int4*)(d + o_seg) + B.s0, B.groups, 1, k, d_best);
        FDCM_HIP(hipGetLastError());
    }
    if (wn && wn->ms) {  // (objects: the threshold per pair)
        auto kern = W.buf32 ? k_window_winners_objects<true> : k_window_winners_objects<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)((nj + 255) / 256)), dim3(256), 0, st, vol, W.SL, (int)fm->m, (int)fm->W, (int)fm->H, fm->tx,
                           fm->ty, (const ExLine*)d, (const float*)(d + o_wlen), (const ExTmpl*)(d + o_wtm), (const int4*)(d + o_wfoot),
                           wneed.empty() ? (const float*)nullptr : (const float*)(d + o_wneed), (const float*)(d + o_wms),
                           (const WinnerJob*)(d + o_wjob), (const int*)(d + o_wrun), (const unsigned long long*)d_best, (int)nj,
                           (unsigned)j0, sx, sy, (unsigned long long*)(d + o_wkeys), (int4*)(d + o_wboxes));
        FDCM_HIP(hipGetLastError());
    } else if (wn) {  // (k = 1: a job's merged list is its winner)
        auto kern = W.buf32 ? k_window_winners<true> : k_window_winners<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)((nj + 255) / 256)), dim3(256), 0, st, vol, W.SL, (int)fm->m, (int)fm->W, (int)fm->H, fm->tx,
                           fm->ty, (const ExLine*)d, (const float*)(d + o_wlen), (const ExTmpl*)(d + o_wtm), (const int4*)(d + o_wfoot),
                           wneed.empty() ? (const float*)nullptr : (const float*)(d + o_wneed), (const WinnerJob*)(d + o_wjob),
                           (const int*)(d + o_wrun), (const unsigned long long*)d_best, (int)nj, (unsigned)j0, sx, sy, wn->max_score,
                           (unsigned long long*)(d + o_wkeys), (int4*)(d + o_wboxes));
        FDCM_HIP(hipGetLastError());
    }
    if (wn) {
        FDCM_HIP(hipMemcpyAsync(wn->keys + j0, d + o_wkeys, nj * 8, hipMemcpyDeviceToHost, st));
        FDCM_HIP(hipMemcpyAsync(wn->boxes + j0, d + o_wboxes, nj * sizeof(Foot), hipMemcpyDeviceToHost, st));
    }
    FDCM_HIP(hipMemcpyAsync(best, d_best, nj * k * 8, hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipStreamSynchronize(st));  // (the host arrays stay alive until here)
}

// Where the round that begins at job j0 ends: jobs of about kWinStageBytes of tables, one job at least.  winners: with the
// tables of the winners' pass.
int64_t windows_round_end(const fdcm_templates* t, const fdcm_pose_window* jobs, int64_t j0, int64_t n_jobs, int k, bool winners = false) {
    // (a forced batch size also shrinks the rounds, to 4 KB a plane: the tests' small lists then go in several)
    const size_t round_bytes = test_switches().windows_batch > 0 ? (size_t)test_switches().windows_batch << 12 : kWinStageBytes;
    int64_t j1 = j0;
    size_t bytes = 0;
    do {  // an upper bound of the job's share of the upload: no pair counted as shared
        const fdcm_pose_window& J = jobs[j1];
        const size_t nl = (size_t)(t->offsets[(size_t)J.tmpl + 1] - t->offsets[(size_t)J.tmpl]);
        bytes += (size_t)J.na * (sizeof(WinPlane) + nl * sizeof(ExLine) +
                                 (size_t)((J.nx + kPatchX - 1) / kPatchX) * (size_t)((J.ny + kPatchY - 1) / kPatchY) * sizeof(int2)) +
                 sizeof(WinJob) + sizeof(int4) + (size_t)k * 8;
        if (winners) bytes += (size_t)J.na * (sizeof(ExTmpl) + sizeof(Foot) + 2 * sizeof(float) + nl * sizeof(float)) + sizeof(WinnerJob);
        ++j1;
    } while (j1 < n_jobs && bytes < round_bytes);
    return j1;
}

}  // namespace

void exhaustive_window(fdcm_featuremap* fm, const fdcm_templates* t, int32_t sx, int32_t sy, fdcm_grid* out) {
    if (sx < 1 || sy < 1) throw std::string("strides sx and sy must be >= 1");
    long long X0 = 0, X1 = -1, Y0 = 0, Y1 = -1;
    bool any = false;
    for (int64_t i = 0; i < t->T; ++i) {
        const int64_t l0 = t->offsets[(size_t)i], n = t->offsets[(size_t)i + 1] - l0;
        if (n == 0) continue;  // a template without lines emits nothing: it does not widen the window
        const Box b = admissible_box(fm, t, l0, n);
        if (!b.any) continue;
        X0 = any ? std::min<long long>(X0, b.x0) : b.x0; X1 = any ? std::max<long long>(X1, b.x1) : b.x1;
        Y0 = any ? std::min<long long>(Y0, b.y0) : b.y0; Y1 = any ? std::max<long long>(Y1, b.y1) : b.y1;
        any = true;
    }
    fdcm_grid g{0, 0, 0, 0, sx, sy};
    if (any) {
        const long long x0 = floor_div(X0, sx) * sx, y0 = floor_div(Y0, sy) * sy;
        g.x0 = (int32_t)x0; g.y0 = (int32_t)y0;
        g.nx = (int32_t)(floor_div(X1 - x0, sx) + 1);
        g.ny = (int32_t)(floor_div(Y1 - y0, sy) + 1);
    }
    *out = g;
}

// rot null: the translations, a plane per template; else [t][a][ny][nx]: (t, a) is plane t * n_rot + a.
void run_score_map(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, float* out_host,
                   float* out_device) {
    check_grid(g);
    if (rot) check_rotated_size(t, rot->n);
    if (t->T == 0) return;
    std::lock_guard<std::mutex> turn(fm->seam_mutex);  // concurrent callers of one feature map take turns (shared search.eval)
    begin(fm);
    Pairs P;
    prepare_pairs(fm, t, rot, test_switches().exhaustive_flat, P);
    const int64_t T = (int64_t)P.nl.size();
    const size_t plane_bytes = (size_t)g.nx * g.ny * sizeof(float);
    // host output: templates in batches whose maps fit a 256 MB workspace; device output: one launch
    const int64_t batch = out_device ? T : std::max<int64_t>(1, std::min<int64_t>(T, ((size_t)256 << 20) / plane_bytes));
    std::vector<ExTmpl> tm((size_t)T);
    for (int64_t i = 0; i < T; ++i) tm[(size_t)i] = grid_tmpl(P, (size_t)i, g, (int)(out_device ? i : i % batch));
    const size_t o_lines = 0, o_tm = al256(P.lines.size() * sizeof(ExLine)), o_map = o_tm + al256(tm.size() * sizeof(ExTmpl));
    reserve_eval(fm, o_map + (out_device ? 0 : (size_t)batch * plane_bytes), 0);
    char* d = (char*)fm->search.eval.p;
    hipStream_t st = fm->stream;
    FDCM_HIP(hipMemcpyAsync(d + o_lines, P.lines.data(), P.lines.size() * sizeof(ExLine), hipMemcpyHostToDevice, st));
    FDCM_HIP(hipMemcpyAsync(d + o_tm, tm.data(), tm.size() * sizeof(ExTmpl), hipMemcpyHostToDevice, st));
    for (int64_t b0 = 0; b0 < T; b0 += batch) {
        const int nb = (int)std::min<int64_t>(batch, T - b0);
        float* map = out_device ? out_device : (float*)(d + o_map);
        launch<kMap>(fm, P, g, (const ExLine*)(d + o_lines), (const ExTmpl*)(d + o_tm) + b0, nb, 0, portions_for(fm, g, nb), map,
                      nullptr);
        if (!out_device)
            FDCM_HIP(hipMemcpyAsync(out_host + (size_t)b0 * g.nx * g.ny, map, (size_t)nb * plane_bytes, hipMemcpyDeviceToHost, st));
    }
    FDCM_HIP(hipStreamSynchronize(st));  // (P and tm stay alive until here)
}

void run_search_exhaustive(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_grid& g, int k, int32_t base,
                           fdcm_match** out, int64_t* n_out) {
    run_search_exhaustive_peaks(fm, t, g, k, 0, 0, base, out, n_out);  // radius 0: every point is a peak
}

// The driver on the caller's lines (prepare_pairs without a table), not on rotated_set's identity rotation: that turns a
// -0 coordinate into +0, which can change the sign of x2 - x1 and with it a line's orientation bin.
void run_search_exhaustive_peaks(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_grid& g, int k, int rx, int ry,
                                 int32_t base, fdcm_match** out, int64_t* n_out) {
    check_grid(g);
    if (k < 1 || k > kMaxK) throw std::string("k must be in [1, 64]");
    if (rx < 0 || rx > kMaxRadius || ry < 0 || ry > kMaxRadius) throw std::string("radii rx and ry must be in [0, 32]");
    *n_out = 0;
    if (t->T == 0) return;
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    begin(fm);
    Pairs P;
    prepare_pairs(fm, t, nullptr, test_switches().exhaustive_flat, P);
    std::vector<unsigned long long> best;
    std::vector<int32_t> index;
    search(fm, P, 1, g, k, rx, ry, 0, 0, best, index);
    emit_records(best, k, index, 1, g, base, nullptr, out, n_out);
}

// What every dense call does under the handle's lock before its keys: the pairs of the whole set, prepared.  Returns the
// number of rotations (rot null: 1, the caller's lines as they are -- run_search_exhaustive_peaks' note on -0).
static int dense_begin(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, bool flat, bool lens, Pairs& P) {
    begin(fm);
    const int n = rot ? rot->n : 1;
    if (rot) check_rotated_size(t, n);
    P.lens = lens;
    prepare_pairs(fm, t, rot, flat, P);
    return n;
}

// The best maps (include/fdcm.h, "Best map and detections", "Gate inside the minimum", "Objects"): the arguments are checked
// (fdcm_capi.cpp).  G planes per output, object after object (ob null: the one object with the gate min_matched).  The needs go
// to the scoring kernel (none for an object with min_matched = 0: the best map's own kernel).  Each output wanted is unpacked
// from the key planes into the G 4-byte planes at o_plane, the fractions of the points' pairs by k_matched_plane, and comes
// down before the next one takes its place.
static void best_maps(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int penalty, float tau,
                      bool flat, const ObjectsIn* ob, float min_matched, float* score_out, int32_t* pair_out, float* matched_out) {
    check_grid(g);
    const int G = ob ? ob->G : 1;
    const size_t N = (size_t)g.nx * g.ny, GN = (size_t)G * N;
    auto none = [&]() {
        if (score_out) std::fill(score_out, score_out + GN, f_nan());
        if (pair_out) std::fill(pair_out, pair_out + GN, (int32_t)-1);
        if (matched_out) std::fill(matched_out, matched_out + GN, f_nan());
    };
    if (t->T == 0) return none();
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    Pairs P;
    const int n = dense_begin(fm, t, rot, flat, matched_out != nullptr, P);
    DenseIn in;
    in.ob = ob;
    in.min_matched = min_matched;
    in.gate_all = true;
    in.planes4 = true;
    in.want_tl = matched_out != nullptr;
    DenseRun R;
    if (!dense_keys(fm, P, t, n, g, penalty, tau, in, R)) return none();
    hipStream_t st = fm->stream;
    char* plane = R.d + R.o_plane;
    auto down = [&](void* out) { FDCM_HIP(hipMemcpyAsync(out, plane, GN * 4, hipMemcpyDeviceToHost, st)); };
    if (score_out) {
        for (int o = 0; o < G; ++o) best_unpack(fm, R, g, o, (float*)plane + (size_t)o * N, nullptr);
        down(score_out);
    }
    if (pair_out) {
        for (int o = 0; o < G; ++o) best_unpack(fm, R, g, o, nullptr, (int*)plane + (size_t)o * N);
        down(pair_out);
    }
    if (matched_out) {
        auto kern = P.buf32 ? k_matched_plane<true> : k_matched_plane<false>;
        for (int o = 0; o < G; ++o) {
            hipLaunchKernelGGL(kern, dim3((unsigned)((g.nx + 63) / 64), (unsigned)((g.ny + 3) / 4)), dim3(256), 0, st, fm->vol.as<float>(),
                               P.SL, (int)fm->m, (int)fm->W, (int)fm->H, fm->tx, fm->ty, (const ExLine*)R.d, (const float*)(R.d + R.o_len),
                               (const ExTmpl*)(R.d + R.o_tm), (const float*)(R.d + R.o_tl),
                               (const unsigned long long*)(R.d + R.o_keys) + (size_t)o * R.n_keys, g.x0, g.y0, g.sx, g.sy, g.nx, g.ny,
                               R.tiles_x, (float*)plane + (size_t)o * N);
            FDCM_HIP(hipGetLastError());
        }
        down(matched_out);
    }
    FDCM_HIP(hipStreamSynchronize(st));
}

void run_best_map(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int penalty, float tau,
                  float* score_out, int32_t* pair_out) {
    best_maps(fm, t, rot, g, penalty, tau, test_switches().exhaustive_flat, nullptr, 0.f, score_out, pair_out, nullptr);
}

// The 64-bit form of the gated and the object best maps follows FDCM_MATCHED_FLAT, as the calls by matched fraction.
void run_best_map_gated(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int penalty, float tau,
                        float min_matched, float* score_out, int32_t* pair_out, float* matched_out) {
    best_maps(fm, t, rot, g, penalty, tau, test_switches().matched_flat, nullptr, min_matched, score_out, pair_out, matched_out);
}

void run_best_map_objects(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int penalty,
                          float tau, const int32_t* objects, int n_objects, const float* min_matched, float* score_out, int32_t* pair_out,
                          float* matched_out) {
    const std::vector<float> inf((size_t)n_objects, f_inf());
    const ObjectsIn ob{objects, n_objects, inf.data(), min_matched, 0};
    best_maps(fm, t, rot, g, penalty, tau, test_switches().matched_flat, &ob, 0.f, score_out, pair_out, matched_out);
}

void run_search_exhaustive_detect(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int k,
                                  int rx, int ry, int penalty, float tau, int32_t base, fdcm_match** out, int64_t* n_out) {
    check_grid(g);
    *n_out = 0;
    if (t->T == 0) return;
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    Pairs P;
    const int n = dense_begin(fm, t, rot, test_switches().exhaustive_flat, false, P);
    DenseIn in;
    in.k = k;
    DenseRun R;
    if (!dense_keys(fm, P, t, n, g, penalty, tau, in, R)) return;
    hipStream_t st = fm->stream;
    char* d = R.d;
    float* plane = (float*)(d + R.o_plane);
    unsigned long long* cand = (unsigned long long*)(d + R.o_cand);
    unsigned long long* d_best = (unsigned long long*)(d + R.o_best);
    best_unpack(fm, R, g, 0, plane, nullptr);
    // the peaks of the score plane: one unit of one plane, its 32-bit form (k_exhaustive_peaks' !ANGLES)
    auto peaks = std::max(rx, ry) <= 8 ? k_exhaustive_peaks<8, false> : k_exhaustive_peaks<kMaxRadius, false>;
    hipLaunchKernelGGL(peaks, dim3((unsigned)R.parts), dim3(256), 0, st, (const float*)plane, g.nx, g.ny, (const ExTmpl*)(d + R.o_unit),
                       (const int4*)nullptr, R.parts, rx, ry, 0, 1, 0, 0, g.nx - 1, 0, g.ny - 1, 0, 0, g.nx, (unsigned)(g.nx * g.ny), k, cand);
    FDCM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_exhaustive_merge_groups, dim3(1), dim3(256), 0, st, (const unsigned long long*)cand, (const int4*)(d + R.o_seg),
                       1, 4 * R.parts, k, d_best);
    FDCM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_best_gather, dim3(1), dim3(64), 0, st, (const unsigned long long*)d_best, k,
                       (const unsigned long long*)(d + R.o_keys), g.nx, R.tiles_x, (int*)(d + R.o_pair));
    FDCM_HIP(hipGetLastError());
    detect_records(fm, R, P, rot != nullptr, n, g, k, base, out, n_out, nullptr, nullptr);
}

// The footprints of every pair of a set given by its packed lines and offsets (no handle, no device): the lines rotated_set
// makes, which are prepare_pairs'.
void lines_footprints(const float* lines, const int64_t* offsets, int64_t T, const fdcm_rotations* rot, int margin, int32_t* boxes_out) {
    const int n = rot ? rot->n : 1;
    Foot* out = (Foot*)boxes_out;
    std::vector<RotM> M((size_t)n);
    fdcm_templates one, rt;  // one template at a time, as a set of its own (pivot 2 i is its pivot 0)
    one.T = 1;
    for (int64_t i = 0; i < T; ++i) {
        const int64_t l0 = offsets[i], nl = offsets[i + 1] - l0;
        if (rot) {
            one.lines.assign(lines + 4 * l0, lines + 4 * (l0 + nl));
            one.offsets = {0, nl};
            one.n_lines = nl;
            const fdcm_rotations sub{rot->cs, rot->n, rot->pivots ? rot->pivots + 2 * i : nullptr};
            rotated_set(&one, sub, 0, 1, rt, M.data());
        }
        for (int a = 0; a < n; ++a)
            out[i * n + a] = rot ? footprint(rt.lines.data() + (size_t)rt.offsets[(size_t)a] * 4, 4, nl, margin)
                                 : footprint(lines + 4 * l0, 4, nl, margin);
    }
}

void templates_footprints(const fdcm_templates* t, const fdcm_rotations* rot, int margin, int32_t* boxes_out) {
    lines_footprints(t->lines.data(), t->offsets.data(), t->T, rot, margin, boxes_out);
}

// Hull footprints (include/fdcm.h): the shapes of every pair of a set given by its packed lines, as lines_footprints.
void lines_footprint_spans(const float* lines, const int64_t* offsets, int64_t T, const fdcm_rotations* rot, int margin,
                           int64_t* row_offsets, int64_t* areas, int32_t* spans) {
    const int n = rot ? rot->n : 1;
    std::vector<RotM> M((size_t)n);
    std::vector<HullPt> h;
    fdcm_templates one, rt;  // one template at a time, as lines_footprints
    one.T = 1;
    row_offsets[0] = 0;
    for (int64_t i = 0; i < T; ++i) {
        const int64_t l0 = offsets[i], nl = offsets[i + 1] - l0;
        if (rot) {
            one.lines.assign(lines + 4 * l0, lines + 4 * (l0 + nl));
            one.offsets = {0, nl};
            one.n_lines = nl;
            const fdcm_rotations sub{rot->cs, rot->n, rot->pivots ? rot->pivots + 2 * i : nullptr};
            rotated_set(&one, sub, 0, 1, rt, M.data());
        }
        for (int a = 0; a < n; ++a) {
            const float* p = rot ? rt.lines.data() + (size_t)rt.offsets[(size_t)a] * 4 : lines + 4 * l0;
            const Foot F = footprint(p, 4, nl, margin);
            const int64_t u = i * n + a;
            row_offsets[u + 1] = row_offsets[u] + foot_rows(F);
            if (!areas && !spans) continue;
            hull_of(p, 4, nl, margin, h);
            const int64_t A = hull_rows(h, F, spans ? spans + 2 * row_offsets[u] : nullptr);
            if (areas) areas[u] = A;
        }
    }
}

void templates_footprint_spans(const fdcm_templates* t, const fdcm_rotations* rot, int margin, int64_t* row_offsets, int64_t* areas,
                               int32_t* spans) {
    lines_footprint_spans(t->lines.data(), t->offsets.data(), t->T, rot, margin, row_offsets, areas, spans);
}

// The rows the span table of a dense call on a hull set would have: host only, for the check before any device work.
void check_hull_rows(const fdcm_templates* t, const fdcm_rotations* rot, int margin) {
    if (t->footprint != FDCM_FOOTPRINT_HULL || t->T == 0) return;
    std::vector<int64_t> off((size_t)(t->T * (rot ? rot->n : 1)) + 1);
    templates_footprint_spans(t, rot, margin, off.data(), nullptr, nullptr);
    if (off.back() > kHullMaxRows) throw std::string("hull footprints: the span table of the call has more than 2^26 rows");
}

// Hull sets, the dense calls: the shapes of the call's pairs.  plan() before dense_keys, which reserves bytes() as the last
// block of its layout; upload() after it: the tables are built in the staging behind the first upload's bytes while the
// scoring launches run, and go up on the same stream before the rounds (plane_rounds).
struct HullRun {
    std::vector<HullShape> shapes;
    size_t rows = 0;
    size_t o_spans() const { return al256(shapes.size() * sizeof(HullShape)); }
    size_t bytes() const { return o_spans() + al256(rows * 8); }
    void plan(const std::vector<Foot>& foot) { rows = hull_layout(foot, shapes); }
    void upload(fdcm_featuremap* fm, const DenseRun& R, const Pairs& P, const std::vector<Foot>& foot, int margin) {
        char* h = (char*)fm->search.eval_stage.p + R.o_pair;
        std::memcpy(h, shapes.data(), shapes.size() * sizeof(HullShape));
        hull_fill(P, foot, margin, (HullShape*)h, (int32_t*)(h + o_spans()));
        FDCM_HIP(hipMemcpyAsync(R.d + R.o_hull, h, bytes(), hipMemcpyHostToDevice, fm->stream));
    }
};

// The rounds of the overlap rule, for every call that has them: round r = 0 .. max_det writes winner r - 1, and the last one
// only reduces.  They are queued kNmsBatch at a time: after each batch the host reads the batch's last winner and stops when
// the list has ended, so a short list costs one batch and no round costs a host round trip.  a: everything but round, last
// and the partials of round - 1; pk_out, pp_out (null for a list form): the first of the two sets of partials, the second
// kNmsWorkgroups entries behind it, used in turn.  The form is the arguments': a list form has no planes (plane_chunks 0),
// a hull form has shapes, and a form with objects is a hull form or one with a table of objects.
constexpr int kNmsBatch = 64;
// so fdcm_search_exhaustive_detect_nms, whose k is at most kMaxK, queues its k + 1 launches with no host synchronisation
static_assert(kMaxK <= kNmsBatch, "a call with k <= kMaxK results is one batch");

static void nms_rounds(NmsArgs a, unsigned wgs, int max_det, hipStream_t st) {
    const bool list = a.plane_chunks == 0, hull = a.shapes != nullptr, obj = hull || a.obj != nullptr;
    auto kern = list ? (hull ? k_nms_round<true, true, true> : obj ? k_nms_round<true, false, true> : k_nms_round<true, false, false>)
                     : (hull ? k_nms_round<false, true, true> : obj ? k_nms_round<false, false, true> : k_nms_round<false, false, false>);
    unsigned long long* const pk = a.pk_out;
    int* const pp = a.pp_out;
    for (int r = 0; r <= max_det;) {
        const int r1 = std::min(max_det, r + kNmsBatch - (r == 0 ? 0 : 1));  // winners [.., r1) after this batch: whole batches
        for (; r <= r1; ++r) {
            const int in = (r + 1) & 1, to = r & 1;
            a.round = r;
            a.last = (int)(r == max_det);
            a.pk_in = pk + in * kNmsWorkgroups;
            a.pk_out = pk + to * kNmsWorkgroups;
            a.pp_in = pp ? pp + in * kNmsWorkgroups : nullptr;
            a.pp_out = pp ? pp + to * kNmsWorkgroups : nullptr;
            hipLaunchKernelGGL(kern, dim3(wgs), dim3(256), 0, st, a);
            FDCM_HIP(hipGetLastError());
        }
        if (r > max_det) break;
        unsigned long long last = kNoKey;  // winner r1 - 1, the batch's last
        FDCM_HIP(hipMemcpyAsync(&last, a.best + (r1 - 1), 8, hipMemcpyDeviceToHost, st));
        FDCM_HIP(hipStreamSynchronize(st));
        if (last == kNoKey) break;  // the list has ended: the entries from there on are kNoKey (written, or the upload's)
    }
}

// The rounds of a dense call on the G key planes dense_keys left at R.o_keys, with the pairs' footprints at o_foot, the
// partials at o_cand and the result list at o_best and o_pair.  H (or null): the set's shapes, uploaded.  A call with objects
// reads their per-pair table; one without runs the round kernel without objects (or the hull form).
static void plane_rounds(fdcm_featuremap* fm, const DenseRun& R, const fdcm_grid& g, const HullRun* H, int permille, int cross,
                         int max_det) {
    char* d = R.d;
    NmsArgs a{};
    a.keys = (unsigned long long*)(d + R.o_keys);
    a.boxes = (const int4*)(d + R.o_foot);
    if (H) {
        a.shapes = (const HullShape*)(d + R.o_hull);
        a.spans = (const int2*)(d + R.o_hull + H->o_spans());
    }
    a.obj = R.objects ? (const int*)(d + R.o_pobj) : nullptr;
    a.plane_chunks = (long long)(R.n_keys / 256);  // whole sub-tiles: a multiple of 4
    a.n_chunks = a.plane_chunks * R.G;
    a.n = a.n_chunks * 256;
    a.x0 = g.x0; a.y0 = g.y0; a.sx = g.sx; a.sy = g.sy; a.nx = g.nx; a.tiles_x = R.tiles_x;
    a.permille = permille;
    a.cross = cross;
    a.pk_out = (unsigned long long*)(d + R.o_cand);
    a.pp_out = (int*)(d + R.o_cand + 2 * kNmsWorkgroups * 8);
    a.best = (unsigned long long*)(d + R.o_best);
    a.pair = (int*)(d + R.o_pair);
    nms_rounds(a, (unsigned)std::min<long long>(kNmsWorkgroups, a.n_chunks), max_det, fm->stream);
}

// The footprints of the pairs of a dense call, from the lines the kernels score (a pair without a grid point is never read).
static std::vector<Foot> pair_footprints(const Pairs& P, int margin) {
    std::vector<Foot> foot(P.nl.size());
    for (size_t u = 0; u < foot.size(); ++u)
        foot[u] = footprint((const float*)(P.lines.data() + P.line0[u]), sizeof(ExLine) / sizeof(float), P.nl[u], margin);
    return foot;
}

// TL_t (include/fdcm.h, "Detections by matched fraction"): the float32 sum of the template's line lengths in line order, from +0.
void templates_matched_totals(const fdcm_templates* t, float* totals) {
    for (int64_t i = 0; i < t->T; ++i) {
        float tl = 0.f;
        for (int64_t q = t->offsets[(size_t)i]; q < t->offsets[(size_t)i + 1]; ++q) tl = tl + t->lengths[(size_t)q];
        totals[i] = tl;
    }
}

// The fractions of the result list of a dense call, at R.o_frac: k_matched_list on the max_det entries at o_best and o_pair.
static void matched_list(fdcm_featuremap* fm, const Pairs& P, const DenseRun& R, const fdcm_grid& g, int max_det) {
    char* d = R.d;
    auto kern = P.buf32 ? k_matched_list<true> : k_matched_list<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((max_det + 255) / 256)), dim3(256), 0, fm->stream, fm->vol.as<float>(), P.SL, (int)fm->m,
                       (int)fm->W, (int)fm->H, fm->tx, fm->ty, (const ExLine*)d, (const float*)(d + R.o_len), (const ExTmpl*)(d + R.o_tm),
                       (const float*)(d + R.o_tl), (const unsigned long long*)(d + R.o_best), (const int*)(d + R.o_pair), max_det, g.x0,
                       g.y0, g.sx, g.sy, g.nx, (float*)(d + R.o_frac));
    FDCM_HIP(hipGetLastError());
}

// The gate pass of FDCM_GATE_WINNER before the first round: k_matched_gate on the key plane of every object with
// min_matched > 0 (mm: per object).
static void gate_pass(fdcm_featuremap* fm, const Pairs& P, const DenseRun& R, const fdcm_grid& g, const float* mm) {
    char* d = R.d;
    auto kern = P.buf32 ? k_matched_gate<true> : k_matched_gate<false>;
    for (int o = 0; o < R.G; ++o) {
        if (!(mm[o] > 0.f)) continue;
        hipLaunchKernelGGL(kern, dim3((unsigned)(R.n_keys / 256)), dim3(256), 0, fm->stream, fm->vol.as<float>(), P.SL, (int)fm->m,
                           (int)fm->W, (int)fm->H, fm->tx, fm->ty, (const ExLine*)d, (const float*)(d + R.o_len),
                           (const ExTmpl*)(d + R.o_tm), (const float*)(d + R.o_need),
                           (unsigned long long*)(d + R.o_keys) + (size_t)o * R.n_keys, (long long)R.n_keys, g.x0, g.y0, g.sx, g.sy, R.tiles_x);
        FDCM_HIP(hipGetLastError());
    }
}

// What a dense detection call passes that is its own.  keys: its objects or its one threshold and gate, and the entries of its
// result list; dense_detect fills in the rest.
struct DetectIn {
    DenseIn keys;
    bool flat = false;                 // the 64-bit form of VolRef: the call's test switch
    int gate_kind = FDCM_GATE_WINNER;
    int max_det = 0;                   // the rounds and the records, at most
    int permille = 0, cross = 0, margin = 0;
};

// The dense detections by footprint overlap (include/fdcm.h, "Detections suppressed by footprint overlap", "All detections
// below a score", "Detections by matched fraction", "Objects"): the arguments are checked (fdcm_capi.cpp).  The key planes
// are dense_keys', one per object, each holding the points with q <= its object's max_score alone; the hull tables go up
// behind the scoring launches; with FDCM_GATE_WINNER the gate pass runs over the planes of the objects with min_matched > 0
// (FDCM_GATE_ALL: the gate was inside the minimum); the rounds are plane_rounds' over all planes; with matched_out the
// fractions of the result list follow the last round; the records are run_search_exhaustive_detect's.  min_matched = 0
// and no matched_out queue what the call without a gate queues.
static void dense_detect(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, const DetectIn& c,
                         int penalty, float tau, int32_t base, fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out) {
    check_grid(g);
    *n_out = 0;
    if (t->T == 0) return;
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    const ObjectsIn* ob = c.keys.ob;
    const float* mm = ob ? ob->min_matched : &c.keys.min_matched;
    const bool gate = mm && std::any_of(mm, mm + (ob ? ob->G : 1), [](float v) { return v > 0.f; });
    const bool fracs = matched_out != nullptr, gate_all = gate && c.gate_kind == FDCM_GATE_ALL;
    Pairs P;
    const int n = dense_begin(fm, t, rot, c.flat, gate || fracs, P);
    const std::vector<Foot> foot = pair_footprints(P, c.margin);
    const bool hull = t->footprint == FDCM_FOOTPRINT_HULL;
    HullRun H;
    if (hull) H.plan(foot);
    DenseIn in = c.keys;
    in.gate_all = gate_all;
    in.foot = &foot;
    in.want_tl = fracs;
    in.hull_bytes = hull ? H.bytes() : 0;
    DenseRun R;
    if (!dense_keys(fm, P, t, n, g, penalty, tau, in, R)) return;
    if (hull) H.upload(fm, R, P, foot, c.margin);
    if (gate && !gate_all) gate_pass(fm, P, R, g, mm);
    plane_rounds(fm, R, g, hull ? &H : nullptr, c.permille, c.cross, c.max_det);
    if (fracs) matched_list(fm, P, R, g, c.max_det);
    detect_records(fm, R, P, rot != nullptr, n, g, c.max_det, base, out, n_out, foot.data(), boxes_out, matched_out);
}

void run_search_exhaustive_detect_nms(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int k,
                                      int permille, int margin, int penalty, float tau, int32_t base, fdcm_match** out,
                                      int32_t* boxes_out, int64_t* n_out) {
    DetectIn c;  // no threshold, no gate, a list of kMaxK entries
    c.flat = test_switches().exhaustive_flat;
    c.max_det = k;
    c.permille = c.cross = permille;
    c.margin = margin;
    dense_detect(fm, t, rot, g, c, penalty, tau, base, out, n_out, boxes_out, nullptr);
}

void run_search_exhaustive_detect_all(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g,
                                      float max_score, int max_det, int permille, int margin, int penalty, float tau, int32_t base,
                                      fdcm_match** out, int64_t* n_out, int32_t* boxes_out) {
    DetectIn c;
    c.keys.max_score = max_score;
    c.keys.list = c.max_det = max_det;
    c.flat = test_switches().exhaustive_flat;
    c.permille = c.cross = permille;
    c.margin = margin;
    dense_detect(fm, t, rot, g, c, penalty, tau, base, out, n_out, boxes_out, nullptr);
}

void run_search_exhaustive_detect_all_matched(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g,
                                              float max_score, int max_det, int permille, int margin, int penalty, float tau,
                                              float min_matched, int gate, int32_t base, fdcm_match** out, int64_t* n_out,
                                              int32_t* boxes_out, float* matched_out) {
    DetectIn c;
    c.keys.max_score = max_score;
    c.keys.min_matched = min_matched;
    c.keys.list = c.max_det = max_det;
    c.flat = test_switches().matched_flat;
    c.gate_kind = gate;
    c.permille = c.cross = permille;
    c.margin = margin;
    dense_detect(fm, t, rot, g, c, penalty, tau, base, out, n_out, boxes_out, matched_out);
}

void run_search_exhaustive_detect_objects(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g,
                                          const int32_t* objects, int n_objects, const float* max_score, const float* min_matched,
                                          int max_det, int permille, int cross, int margin, int penalty, float tau, int gate_kind,
                                          int32_t base, fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out) {
    const ObjectsIn ob{objects, n_objects, max_score, min_matched, cross};
    DetectIn c;
    c.keys.ob = &ob;
    c.keys.list = c.max_det = max_det;
    c.flat = test_switches().matched_flat;
    c.gate_kind = gate_kind;
    c.permille = permille;
    c.cross = cross;
    c.margin = margin;
    dense_detect(fm, t, rot, g, c, penalty, tau, base, out, n_out, boxes_out, matched_out);
}

float detect_score_bound(float den, float max_score) { return score_bound(den, max_score); }

// B_t per template (include/fdcm.h): score_bound of best_denominators' den_t; 0 for a template without lines.  Host only.
void detect_score_bounds(const fdcm_templates* t, int penalty, float tau, float max_score, float* bounds) {
    const std::vector<float> den = best_denominators(t, penalty, tau);
    for (int64_t i = 0; i < t->T; ++i)
        bounds[i] = t->offsets[(size_t)i + 1] == t->offsets[(size_t)i] ? 0.f : score_bound(den[(size_t)i], max_score);
}

void exhaustive_rotations_window(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations& rot, int32_t sx, int32_t sy,
                                 fdcm_grid* out) {
    if (sx < 1 || sy < 1) throw std::string("strides sx and sy must be >= 1");
    check_rotated_size(t, rot.n);
    fdcm_templates rt;
    std::vector<RotM> M((size_t)(t->T * rot.n));
    rotated_set(t, rot, 0, t->T, rt, M.data());
    exhaustive_window(fm, &rt, sx, sy, out);
}

void run_search_exhaustive_rotations(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations& rot, const fdcm_grid& g,
                                     int k, int rx, int ry, int ra, int wrap, int32_t base, fdcm_match** out, int64_t* n_out) {
    check_grid(g);
    if (k < 1 || k > kMaxK) throw std::string("k must be in [1, 64]");
    if (rx < 0 || rx > kMaxRadius || ry < 0 || ry > kMaxRadius || ra < 0 || ra > kMaxRadius)
        throw std::string("radii rx, ry and ra must be in [0, 32]");
    if (wrap != 0 && wrap != 1) throw std::string("wrap must be 0 or 1");
    const int n = rot.n;
    if (n < 1) throw std::string("rotations: n must be >= 1");
    if ((unsigned long long)n * g.nx * g.ny > (1ull << 32)) throw std::string("n_rot * nx * ny must be at most 2^32");
    *n_out = 0;
    if (t->T == 0) return;
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    begin(fm);
    check_rotated_size(t, n);
    Pairs P;
    prepare_pairs(fm, t, &rot, test_switches().exhaustive_flat, P);
    std::vector<unsigned long long> best;
    std::vector<int32_t> index;
    search(fm, P, n, g, k, rx, ry, ra, wrap, best, index);
    emit_records(best, k, index, n, g, base, P.M.data(), out, n_out);
}

// Pose windows (include/fdcm.h): the arguments are checked (fdcm_capi.cpp).  Jobs go in rounds of about kWinStageBytes of
// tables, one in practice; a job is never cut, so the lines of one job's run are the one part no round bounds.
void run_search_exhaustive_windows(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_pose_window* jobs,
                                   int64_t n_jobs, int sx, int sy, int k, int32_t base, fdcm_match** out, int64_t* n_out,
                                   int64_t* job_offsets) {
    *n_out = 0;
    if (job_offsets) std::fill(job_offsets, job_offsets + n_jobs + 1, (int64_t)0);
    if (n_jobs == 0 || t->T == 0) return;
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    begin(fm);
    std::vector<unsigned long long> best((size_t)n_jobs * k, kNoKey);
    std::vector<int64_t> m0((size_t)n_jobs + 1, 0);
    for (int64_t j = 0; j < n_jobs; ++j) m0[(size_t)j + 1] = m0[(size_t)j] + jobs[j].na;
    std::vector<RotM> Mjob(rot ? (size_t)m0[(size_t)n_jobs] : 0);
    for (int64_t j0 = 0; j0 < n_jobs;) {
        const int64_t j1 = windows_round_end(t, jobs, j0, n_jobs, k);
        windows_round(fm, t, rot, jobs, j0, j1, sx, sy, k, best.data() + (size_t)j0 * k, m0, Mjob, test_switches().windows_flat);
        j0 = j1;
    }
    std::vector<fdcm_grid> grids((size_t)n_jobs);
    for (int64_t j = 0; j < n_jobs; ++j) grids[(size_t)j] = fdcm_grid{jobs[j].x0, jobs[j].y0, jobs[j].nx, jobs[j].ny, sx, sy};
    emit_records(
        best, k, n_jobs, [&](int64_t q) { return base + jobs[q].tmpl; }, [&](int64_t q) -> const fdcm_grid& { return grids[(size_t)q]; },
        [&](int64_t q, int e) { return rot ? &Mjob[(size_t)(m0[(size_t)q] + e)] : nullptr; }, out, n_out, job_offsets);
}

static void matched_fractions_rounds(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses,
                                     int64_t n, float* fractions);

// Detections over pose windows (include/fdcm.h): the arguments are checked (fdcm_capi.cpp).  The job list goes through
// windows_round at k = 1 in the pose windows' rounds, each with the winners' pass behind its last merge; the rounds leave
// the winners' list on the host, a key and a footprint per job, which goes up whole for the rounds of the list
// forms of k_nms_round, queued by nms_rounds as the dense calls' are.  A record is emit_records' for the key (bits of q << 32) |
// (e N_j + g) of its job's winner; its box is the list's; its fraction k_matched_fractions' at the record's pose, in a
// round of its own after the last launch.  The 64-bit form follows FDCM_WINDOWS_FLAT and FDCM_MATCHED_FLAT.  gate
// FDCM_GATE_ALL ("Gate inside the minimum") with min_matched > 0: the scoring kernel's gated form, and the winners' pass without need.
//
// ob (ObjectsIn, or null): the threshold and the need of a job are its object's (max_score and min_matched are then unused),
// the winners' pass is k_window_winners_objects and the rounds are the list form's with objects, the jobs' objects behind
// the boxes in the same upload.  Without it the call queues what it queued before objects existed.
static void detect_windows(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_pose_window* jobs,
                           int64_t n_jobs, int sx, int sy, float max_score, int max_det, int permille, int margin, int penalty, float tau,
                           float min_matched, int gate, int32_t base, fdcm_match** out, int64_t* n_out, int32_t* boxes_out,
                           float* matched_out, int32_t* jobs_out, const ObjectsIn* ob) {
    *n_out = 0;
    if (n_jobs == 0 || t->T == 0) return;
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    begin(fm);
    const int n = rot ? rot->n : 1;
    const size_t nj = (size_t)n_jobs;
    std::vector<unsigned long long> raw(nj, kNoKey), keys(nj, kNoKey);  // the winners' window keys; the list's keys
    std::vector<Foot> boxes(nj, Foot{0, 0, -1, -1});
    std::vector<int64_t> m0(nj + 1, 0);
    for (int64_t j = 0; j < n_jobs; ++j) m0[(size_t)j + 1] = m0[(size_t)j] + jobs[j].na;
    std::vector<RotM> Mjob(rot ? (size_t)m0[nj] : 0);
    const std::vector<float> den = best_denominators(t, penalty, tau);
    std::vector<float> totals, need;  // per template
    std::vector<float> ms;  // (objects) per template: its object's threshold
    bool gated = min_matched > 0.f;
    if (ob) {
        gated = ob->min_matched && std::any_of(ob->min_matched, ob->min_matched + ob->G, [](float v) { return v > 0.f; });
        ms.resize((size_t)t->T);
        for (size_t i = 0; i < ms.size(); ++i) ms[i] = ob->max_score[ob->objects[i]];
    }
    if (gated) matched_needs(t, 1, true, [&](size_t i) { return ob ? ob->min_matched[ob->objects[i]] : min_matched; }, totals, need);
    const WinnersIn wn{den.data(), need.empty() ? nullptr : need.data(), gate == FDCM_GATE_ALL, margin, max_score, keys.data(),
                       boxes.data(), ob ? ms.data() : nullptr};
    const bool flat = test_switches().windows_flat || test_switches().matched_flat;
    for (int64_t j0 = 0; j0 < n_jobs;) {
        const int64_t j1 = windows_round_end(t, jobs, j0, n_jobs, 1, true);
        windows_round(fm, t, rot, jobs, j0, j1, sx, sy, 1, raw.data() + j0, m0, Mjob, flat, &wn);
        j0 = j1;
    }
    if (std::all_of(keys.begin(), keys.end(), [](unsigned long long v) { return v == kNoKey; })) return;

    // Hull sets: the shapes of the entries of S_0 alone, built here on the host once the winners are known.  An entry's shape
    // is its pair's (tmpl, a_j), a function of the pair and the margin: distinct pairs are built once, from the lines
    // prepare_pairs makes, and every entry of a pair points at the same rows.
    const bool hull = t->footprint == FDCM_FOOTPRINT_HULL;
    std::vector<HullShape> shapes;
    std::vector<int32_t> spans;
    if (hull) {
        shapes.assign(nj, HullShape{0, 0, 0});
        std::map<int64_t, HullShape> done;
        std::vector<HullPt> hp;
        fdcm_templates rt;
        RotM M1;
        for (size_t j = 0; j < nj; ++j) {
            if (keys[j] == kNoKey) continue;
            const fdcm_pose_window& J = jobs[j];
            const int a = (int)((J.a0 + (int64_t)((uint32_t)raw[j] / (uint32_t)(J.nx * J.ny))) % n);
            const int64_t u = (int64_t)J.tmpl * n + a;
            auto it = done.find(u);
            if (it == done.end()) {
                const int64_t l0 = t->offsets[(size_t)J.tmpl], nl = t->offsets[(size_t)J.tmpl + 1] - l0;
                const float* p = t->lines.data() + 4 * l0;
                if (rot) {
                    const fdcm_rotations sub{rot->cs + 2 * a, 1, rot->pivots};
                    rotated_set(t, sub, J.tmpl, J.tmpl + 1, rt, &M1);
                    p = rt.lines.data();
                }
                const Foot F = footprint(p, 4, nl, margin);
                const size_t row0 = spans.size() / 2;
                if ((int64_t)row0 + foot_rows(F) > kHullMaxRows)
                    throw std::string("hull footprints: the span table of the call has more than 2^26 rows");
                spans.resize(spans.size() + 2 * (size_t)foot_rows(F));
                hull_of(p, 4, nl, margin, hp);
                const int64_t A = hull_rows(hp, F, spans.data() + 2 * row0);
                it = done.emplace(u, HullShape{A, (int)row0, 0}).first;
            }
            shapes[j] = it->second;
        }
    }

    // The rounds: the list (keys, boxes) and the result list (kNoKey) by one upload; two sets of partial minima behind them.
    const size_t o_box = al256(nj * 8), o_obj = o_box + al256(nj * sizeof(Foot)), o_shape = o_obj + (ob ? al256(nj * 4) : 0),
                 o_spans = o_shape + (hull ? al256(nj * sizeof(HullShape)) : 0), o_best = o_spans + (hull ? al256(spans.size() * 4) : 0),
                 o_pk = o_best + al256((size_t)max_det * 8);
    reserve_eval(fm, o_pk + 2 * kNmsWorkgroups * 8, o_pk);
    char* d = (char*)fm->search.eval.p;
    char* h = (char*)fm->search.eval_stage.p;
    std::memcpy(h, keys.data(), nj * 8);
    std::memcpy(h + o_box, boxes.data(), nj * sizeof(Foot));
    if (ob)
        for (size_t j = 0; j < nj; ++j) ((int32_t*)(h + o_obj))[j] = ob->objects[jobs[j].tmpl];
    if (hull) {
        std::memcpy(h + o_shape, shapes.data(), nj * sizeof(HullShape));
        std::memcpy(h + o_spans, spans.data(), spans.size() * 4);
    }
    std::memset(h + o_best, 0xff, (size_t)max_det * 8);  // kNoKey
    hipStream_t st = fm->stream;
    FDCM_HIP(hipMemcpyAsync(d, h, o_pk, hipMemcpyHostToDevice, st));
    unsigned long long* d_best = (unsigned long long*)(d + o_best);
    NmsArgs a{};  // a list form: no planes, no pairs
    a.keys = (unsigned long long*)d;
    a.boxes = (const int4*)(d + o_box);
    if (hull) {
        a.shapes = (const HullShape*)(d + o_shape);
        a.spans = (const int2*)(d + o_spans);
    }
    if (ob) a.obj = (const int*)(d + o_obj);
    a.n = (long long)n_jobs;
    a.n_chunks = (a.n + 255) / 256;
    a.permille = permille;
    a.cross = ob ? ob->cross : permille;
    a.pk_out = (unsigned long long*)(d + o_pk);
    a.best = d_best;
    nms_rounds(a, (unsigned)std::min<long long>(kNmsWorkgroups, a.n_chunks), max_det, st);
    std::vector<unsigned long long> best((size_t)max_det);
    FDCM_HIP(hipMemcpyAsync(best.data(), d_best, (size_t)max_det * 8, hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipStreamSynchronize(st));

    // Record l is job jl[l]'s winner with q for its score: emit_records on lists of one key each.
    std::vector<int64_t> jl;
    std::vector<unsigned long long> rk;
    for (int l = 0; l < max_det && best[(size_t)l] != kNoKey; ++l) {
        const size_t j = (size_t)(uint32_t)best[(size_t)l];
        jl.push_back((int64_t)j);
        rk.push_back((best[(size_t)l] & 0xffffffff00000000ull) | (raw[j] & 0xffffffffull));
    }
    std::vector<fdcm_grid> grids(jl.size());
    for (size_t l = 0; l < jl.size(); ++l) {
        const fdcm_pose_window& J = jobs[jl[l]];
        grids[l] = fdcm_grid{J.x0, J.y0, J.nx, J.ny, sx, sy};
    }
    emit_records(
        rk, 1, (int64_t)jl.size(), [&](int64_t q) { return base + jobs[jl[(size_t)q]].tmpl; },
        [&](int64_t q) -> const fdcm_grid& { return grids[(size_t)q]; },
        [&](int64_t q, int e) { return rot ? &Mjob[(size_t)(m0[(size_t)jl[(size_t)q]] + e)] : nullptr; }, out, n_out, nullptr);
    std::vector<int32_t> poses(matched_out ? 4 * jl.size() : 0);
    for (size_t l = 0; l < jl.size(); ++l) {
        const size_t j = (size_t)jl[l];
        if (boxes_out) std::memcpy(boxes_out + 4 * l, &boxes[j], sizeof(Foot));
        if (jobs_out) jobs_out[l] = (int32_t)j;
        if (matched_out) {
            const fdcm_pose_window& J = jobs[j];
            const uint32_t low = (uint32_t)raw[j], N = (uint32_t)(J.nx * J.ny), g = low % N;
            int32_t* p = &poses[4 * l];
            p[0] = J.tmpl; p[1] = (int32_t)((J.a0 + (int64_t)(low / N)) % n);
            p[2] = J.x0 + (int32_t)(g % (uint32_t)J.nx) * sx; p[3] = J.y0 + (int32_t)(g / (uint32_t)J.nx) * sy;
        }
    }
    if (matched_out && !jl.empty()) matched_fractions_rounds(fm, t, rot, poses.data(), (int64_t)jl.size(), matched_out);
}

void run_search_exhaustive_detect_windows(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot,
                                          const fdcm_pose_window* jobs, int64_t n_jobs, int sx, int sy, float max_score, int max_det,
                                          int permille, int margin, int penalty, float tau, float min_matched, int gate, int32_t base,
                                          fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out, int32_t* jobs_out) {
    detect_windows(fm, t, rot, jobs, n_jobs, sx, sy, max_score, max_det, permille, margin, penalty, tau, min_matched, gate, base, out, n_out,
                   boxes_out, matched_out, jobs_out, nullptr);
}

// Objects (include/fdcm.h, "Objects"): the arguments are checked (fdcm_capi.cpp), objects against the set included.
void run_search_exhaustive_detect_windows_objects(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot,
                                                  const fdcm_pose_window* jobs, int64_t n_jobs, int sx, int sy, const int32_t* objects,
                                                  int n_objects, const float* max_score, const float* min_matched, int max_det,
                                                  int permille, int cross, int margin, int penalty, float tau, int gate, int32_t base,
                                                  fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out,
                                                  int32_t* jobs_out) {
    const ObjectsIn ob{objects, n_objects, max_score, min_matched, cross};
    detect_windows(fm, t, rot, jobs, n_jobs, sx, sy, 0.f, max_det, permille, margin, penalty, tau, 0.f, gate, base, out, n_out, boxes_out,
                   matched_out, jobs_out, &ob);
}

// Line costs (include/fdcm.h): the arguments are checked (fdcm_capi.cpp).  Poses go in rounds of kCostPoses; a round
// prepares the distinct pairs its poses name as the pose windows prepare theirs, uploads lines and poses in one copy,
// runs k_line_costs and downloads its floats.  rot null: the caller's lines as they are.
constexpr int64_t kCostPoses = 1 << 20;

void run_line_costs(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                    float** costs, int64_t* offsets) {
    std::fill(offsets, offsets + n + 1, (int64_t)0);
    *costs = (float*)std::malloc(sizeof(float));
    if (!*costs) throw std::string("out of memory");
    if (n == 0 || t->T == 0 || fm->W == 0 || fm->H == 0 || fm->m == 0) return;
    for (int64_t q = 0; q < n; ++q) {
        const int64_t i = poses[4 * q];
        offsets[q + 1] = offsets[q] + (t->offsets[(size_t)i + 1] - t->offsets[(size_t)i]);
    }
    const int64_t total = offsets[n];
    if (total == 0) return;
    std::free(*costs);
    *costs = (float*)std::malloc((size_t)total * sizeof(float));
    if (!*costs) throw std::string("out of memory");
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    begin(fm);
    const int nr = rot ? rot->n : 1;
    const float* vol = fm->vol.as<float>();
    hipStream_t st = fm->stream;
    for (int64_t q0 = 0; q0 < n; q0 += kCostPoses) {
        const int64_t q1 = std::min(n, q0 + kCostPoses), floats = offsets[q1] - offsets[q0];
        if (floats == 0) continue;
        Pairs W;
        for (int64_t q = q0; q < q1; ++q) W.key.push_back((int64_t)poses[4 * q] * nr + poses[4 * q + 1]);
        std::sort(W.key.begin(), W.key.end());
        W.key.erase(std::unique(W.key.begin(), W.key.end()), W.key.end());
        prepare_pairs(fm, t, rot, test_switches().exhaustive_flat, W);
        std::vector<CostPose> tab((size_t)(q1 - q0));
        for (int64_t q = q0; q < q1; ++q) {
            const int32_t* p = poses + 4 * q;
            const size_t u = W.find((int64_t)p[0] * nr + p[1]);
            const Box& b = W.box[u];
            const bool adm = b.any && p[2] >= b.x0 && p[2] <= b.x1 && p[3] >= b.y0 && p[3] <= b.y1;
            tab[(size_t)(q - q0)] = CostPose{W.line0[u], W.nl[u], p[2], p[3], (long long)(offsets[q] - offsets[q0]), adm ? 1 : 0, 0};
        }
        const size_t o_tab = al256(W.lines.size() * sizeof(ExLine)), o_out = o_tab + al256(tab.size() * sizeof(CostPose));
        reserve_eval(fm, o_out + al256((size_t)floats * sizeof(float)), o_out);
        char* d = (char*)fm->search.eval.p;
        char* h = (char*)fm->search.eval_stage.p;
        std::memcpy(h, W.lines.data(), W.lines.size() * sizeof(ExLine));
        std::memcpy(h + o_tab, tab.data(), tab.size() * sizeof(CostPose));
        FDCM_HIP(hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, st));
        auto kern = W.buf32 ? k_line_costs<true> : k_line_costs<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)((tab.size() + 3) / 4)), dim3(256), 0, st, vol, W.SL, (int)fm->m, (int)fm->W, (int)fm->H,
                           fm->tx, fm->ty, (const ExLine*)d, (const CostPose*)(d + o_tab), (int)tab.size(), (float*)(d + o_out));
        FDCM_HIP(hipGetLastError());
        FDCM_HIP(hipMemcpyAsync(*costs + offsets[q0], d + o_out, (size_t)floats * sizeof(float), hipMemcpyDeviceToHost, st));
        FDCM_HIP(hipStreamSynchronize(st));  // (the host arrays stay alive until here; the next round reuses the staging)
    }
}

// Matched fractions (include/fdcm.h, "Detections by matched fraction"): the arguments are checked (fdcm_capi.cpp).  The rounds,
// the pairs and admissibility are run_line_costs'; a round uploads lines, lengths and poses in one copy, runs
// k_matched_fractions and downloads a float per pose.
void run_matched_fractions(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                           float* fractions) {
    if (n == 0 || t->T == 0 || fm->W == 0 || fm->H == 0 || fm->m == 0) return;
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    begin(fm);
    matched_fractions_rounds(fm, t, rot, poses, n, fractions);
}

// The rounds of run_matched_fractions, for a caller that holds the feature map's turn and has begun.
static void matched_fractions_rounds(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses,
                                     int64_t n, float* fractions) {
    const int nr = rot ? rot->n : 1;
    const float* vol = fm->vol.as<float>();
    hipStream_t st = fm->stream;
    std::vector<float> totals((size_t)t->T);
    templates_matched_totals(t, totals.data());
    for (int64_t q0 = 0; q0 < n; q0 += kCostPoses) {
        const int64_t q1 = std::min(n, q0 + kCostPoses);
        Pairs W;
        W.lens = true;
        for (int64_t q = q0; q < q1; ++q) W.key.push_back((int64_t)poses[4 * q] * nr + poses[4 * q + 1]);
        std::sort(W.key.begin(), W.key.end());
        W.key.erase(std::unique(W.key.begin(), W.key.end()), W.key.end());
        prepare_pairs(fm, t, rot, test_switches().matched_flat, W);
        std::vector<FracPose> tab((size_t)(q1 - q0));
        for (int64_t q = q0; q < q1; ++q) {
            const int32_t* p = poses + 4 * q;
            const size_t u = W.find((int64_t)p[0] * nr + p[1]);
            const Box& b = W.box[u];
            const bool adm = b.any && p[2] >= b.x0 && p[2] <= b.x1 && p[3] >= b.y0 && p[3] <= b.y1;
            tab[(size_t)(q - q0)] = FracPose{W.line0[u], W.nl[u], p[2], p[3], totals[(size_t)p[0]], adm ? 1 : 0};
        }
        const size_t o_len = al256(W.lines.size() * sizeof(ExLine)), o_tab = o_len + al256(W.len.size() * sizeof(float)),
                     o_out = o_tab + al256(tab.size() * sizeof(FracPose));
        reserve_eval(fm, o_out + al256(tab.size() * sizeof(float)), o_out);
        char* d = (char*)fm->search.eval.p;
        char* h = (char*)fm->search.eval_stage.p;
        std::memcpy(h, W.lines.data(), W.lines.size() * sizeof(ExLine));
        std::memcpy(h + o_len, W.len.data(), W.len.size() * sizeof(float));
        std::memcpy(h + o_tab, tab.data(), tab.size() * sizeof(FracPose));
        FDCM_HIP(hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, st));
        auto kern = W.buf32 ? k_matched_fractions<true> : k_matched_fractions<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)((tab.size() + 255) / 256)), dim3(256), 0, st, vol, W.SL, (int)fm->m, (int)fm->W,
                           (int)fm->H, fm->tx, fm->ty, (const ExLine*)d, (const float*)(d + o_len), (const FracPose*)(d + o_tab),
                           (int)tab.size(), (float*)(d + o_out));
        FDCM_HIP(hipGetLastError());
        FDCM_HIP(hipMemcpyAsync(fractions + q0, d + o_out, tab.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        FDCM_HIP(hipStreamSynchronize(st));  // (the host arrays stay alive until here; the next round reuses the staging)
    }
}

// Scene coverage (include/fdcm.h, "Scene coverage"; fdcm_coverage.hip): prepare_pairs of the distinct pairs a checked pose list
// names, as run_line_costs prepares them, with their footprints at `margin`.  The lines come in the 64-bit form, whose `se` is
// the bin itself.  Host only.
void coverage_pairs(const fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                    int margin, CoveragePairs& out) {
    const int nr = rot ? rot->n : 1;
    Pairs W;
    W.foot_margin = margin;
    for (int64_t q = 0; q < n; ++q) W.key.push_back((int64_t)poses[4 * q] * nr + poses[4 * q + 1]);
    std::sort(W.key.begin(), W.key.end());
    W.key.erase(std::unique(W.key.begin(), W.key.end()), W.key.end());
    prepare_pairs(fm, t, rot, true, W);
    const size_t np = W.key.size();
    out.key = W.key;
    out.line0 = W.line0;
    out.nl = W.nl;
    out.lines.resize(W.lines.size());
    for (size_t i = 0; i < W.lines.size(); ++i) out.lines[i] = CoverageLine{W.lines[i].x1, W.lines[i].y1, W.lines[i].x2, W.lines[i].y2, W.lines[i].se};
    out.adm.resize(np * 5);
    out.foot.resize(np * 4);
    for (size_t u = 0; u < np; ++u) {
        const Box& b = W.box[u];
        const int32_t a[5] = {b.any ? 1 : 0, b.x0, b.x1, b.y0, b.y1};
        std::copy_n(a, 5, out.adm.begin() + 5 * u);
        const Foot& f = W.foot[u];
        const int32_t g[4] = {f.x0, f.y0, f.x1, f.y1};
        std::copy_n(g, 4, out.foot.begin() + 4 * u);
    }
}

// ---- match lists (include/fdcm.h, "Match lists"): the records of the reference's own path, {tmpl_idx, score, transform[6]}
// with a free float transform, verified and suppressed on the device.
//   k_matches_verify<BUF32, CAP, OBJ>  a wave per record, a lane per line of its template in rounds of 64.  The record comes by
//                                  wave-uniform loads; the lines and lengths are the set's resident d_lines and d_lengths.
//                                  Pass 1 poses every end point (transform, math.h:341-344: unfused float32), decides
//                                  admissibility by the seam's rule (k_evaluate at translation (0, 0)) and reduces the box
//                                  (footprint()'s arithmetic) -- before any read of the volume.  Pass 2, admissible records
//                                  alone: the bin by atanf_glibc + closest_orientation as k_search (or the host's bins), the
//                                  uncapped cost by ex_column / ex_read, s in Eigen's order (rows_score's statement of it,
//                                  with the lines spread over the lanes: line i is lane i % 64, whose class i % 8 is fixed,
//                                  so the eight accumulators are eight sequential sums over the lanes of a class, round
//                                  after round), ML in line order (matched_length's rule).  Lane 0 writes the record's
//                                  score, fraction, q, key and box straight into the list form's arrays.
//   k_matches_gather               the result keys as 64-byte entries (record with q, box, fraction, position) in pinned memory
// The rounds between them are nms_rounds' list form, k_nms_round<true, false, false>, unchanged (with objects <true, false, true>,
// on a hull set <true, true, true>).
namespace {

struct MatchesArgs {
    const float* vol;
    size_t SL;
    int m, W, H;
    float tx, ty;
    const float* keys;  // the map's m orientation keys
    const float4* tlines;  // the set's resident lines, lengths and offsets
    const float* tlen;
    const long long* toff;
    const float* caps;  // (CAP) per line of the set, the call's upload
    const float* den;   // per template: the penalty's denominator
    const float* need;  // per template: float32(min_matched * TL), or null for no gate
    const float* tl;    // per template: TL
    const unsigned short* bins;  // [record][Lmax] bins from the host libm, or null
    const fdcm_match* rec;
    int n, base, T, Lmax, margin, rescore;
    float max_score;
    float* score;  // s(r)
    float* frac;
    float* costs;  // [record][Lmax], or null
    float* q;
    unsigned long long* keys_out;
    int4* boxes;
};

// (OBJ) what the pass with objects reads and writes beside MatchesArgs ("Match lists: objects and hull shapes"): the threshold
// of a record is its template's object's, as its need is (host-made tables, as detect_windows makes ms and need), and the
// record's object goes to the rounds.  Without OBJ nothing of it is read.
struct MatchesObjArgs {
    const float* ms;   // per template: max_score[objects[t]]
    const int* tobj;   // per template: objects[t]
    int* obj;          // per record: its object when it is valid, admissible and has lines (it may need a shape), else -1
};

template <bool BUF32, bool CAP, bool OBJ>
__global__ void __launch_bounds__(256) k_matches_verify(const MatchesArgs a, const MatchesObjArgs ob) {
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (j >= a.n) return;  // wave-uniform
    const fdcm_match R = a.rec[j];
    const long long t = (long long)R.tmpl_idx - (long long)a.base;
    float* const crow = a.costs ? a.costs + (size_t)j * (size_t)a.Lmax : nullptr;
    if (t < 0 || t >= a.T) {  // not a valid record: it takes part in nothing
        if (crow)
            for (int i = lane; i < a.Lmax; i += 64) crow[i] = f_nan();
        if (lane == 0) {
            a.score[j] = f_nan(); a.frac[j] = f_nan(); a.q[j] = f_nan();
            a.keys_out[j] = kNoKey;
            a.boxes[j] = make_int4(0, 0, -1, -1);
            if (OBJ) ob.obj[j] = -1;
        }
        return;
    }
    const long long l0 = a.toff[t];
    const int nl = (int)(a.toff[t + 1] - l0);
    const MatchTransform M{R.transform[0], R.transform[1], R.transform[2], R.transform[3], R.transform[4], R.transform[5]};
    const float offx = a.tx + 0.f, offy = a.ty + 0.f;  // sceneTranslation + translation, the translation (0, 0)
    // ---- pass 1: admissibility and the box (fdcm_score.h)
    const MatchFrame F = match_frame(a.tlines, l0, nl, M, offx, offy, a.W, a.H, a.margin, lane);
    const bool adm = F.adm;
    const int4 box = F.box;
    // ---- pass 2: costs, s in Eigen's order, ML in line order
    const VolRef V = make_volref(a.vol, a.SL, a.m, BUF32);
    const unsigned uH = (unsigned)a.H;
    const int aligned2 = (nl / 8) * 8, aligned = (nl / 4) * 4;
    float acc = 0.f, res = 0.f, ml = 0.f;
    for (int r0 = 0; r0 < nl; r0 += 64) {  // wave-uniform
        const int i = r0 + lane;
        float cost = f_nan(), cap = f_inf(), len = 0.f;
        if (i < nl) {
            if (adm) {
                const float4 p = match_pose_line(M, a.tlines[l0 + i]);
                const float x1 = p.x, y1 = p.y, x2 = p.z, y2 = p.w;
                int bin;
                if (a.bins) {
                    bin = (int)a.bins[(size_t)j * (size_t)a.Lmax + i];
                } else {
                    const float angle = atanf_glibc((y2 - y1) / (x2 - x1));  // getAngle, math.h:295-299
                    bin = closest_orientation(a.keys, a.m, angle);           // dt3cpu.cpp:144-148
                }
                const int se = BUF32 ? (int)((unsigned)bin * (unsigned)a.SL) : bin;
                const size_t c1 = ex_column<BUF32>((int)(x1 + offx), se, a.W, uH, a.SL);
                const size_t c2 = ex_column<BUF32>((int)(x2 + offx), se, a.W, uH, a.SL);
                cost = line_term<false>(ex_read<BUF32>(V, c1, (int)(y1 + offy), uH), ex_read<BUF32>(V, c2, (int)(y2 + offy), uH), 0.f);
                if (CAP) cap = a.caps[l0 + i];
                len = a.tlen[l0 + i];
            }
            if (crow) crow[i] = cost;
        }
        if (!adm) continue;  // wave-uniform
        const float capped = CAP && cost > cap ? cap : cost;
        // the blocks of 8: lane c < 8 of a class sums the lines 8 b + c of this round, b ascending
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int src = (lane & 7) + 8 * k;
            const float v = __shfl(capped, src);
            if (r0 + src < aligned2) acc = acc + v;
        }
        // ML: the matched lines of this round in line order
        unsigned long long mm = __ballot(i < nl && cost <= cap);
        while (mm) {  // wave-uniform
            const int src = __ffsll((long long)mm) - 1;
            mm &= mm - 1;
            ml = ml + __shfl(len, src);
        }
        if (r0 + 64 >= nl) {  // the last round holds the trailing packet and the scalar tail
            float p = __shfl(acc, lane & 3) + __shfl(acc, (lane & 3) + 4);  // p0 += p1
            if (aligned > aligned2) p = p + __shfl(capped, (aligned2 - r0) + (lane & 3));
            if (aligned) res = (__shfl(p, 0) + __shfl(p, 2)) + (__shfl(p, 1) + __shfl(p, 3));  // predux
            for (int idx = aligned; idx < nl; ++idx) res = res + __shfl(capped, idx - r0);
        }
    }
    if (crow)
        for (int i = nl + lane; i < a.Lmax; i += 64) crow[i] = f_nan();
    if (lane == 0) {
        const float s = adm ? res : f_nan();
        const float qv = (a.rescore ? s : R.score) / a.den[t];
        bool cand = nl > 0 && adm && !f_isnan(qv) && !f_signbit(qv) && qv <= (OBJ ? ob.ms[t] : a.max_score);
        if (cand && a.need) cand = ml >= a.need[t];
        a.score[j] = s;
        a.frac[j] = adm ? matched_fraction(ml, a.tl[t]) : f_nan();
        a.q[j] = qv;
        a.keys_out[j] = cand ? ((unsigned long long)__float_as_uint(qv) << 32) | (unsigned)j : kNoKey;
        a.boxes[j] = box;
        if (OBJ) ob.obj[j] = nl > 0 && adm ? ob.tobj[t] : -1;
    }
}


struct MatchOut {  // one result of the detect call
    fdcm_match rec;  // the record with q for its score
    int4 box;
    float frac;
    int idx;  // its position in the list; -1: the result list ended before this entry
    int pad[2];
};
static_assert(sizeof(MatchOut) == 64, "MatchOut is 64 bytes");

__global__ void __launch_bounds__(256) k_matches_gather(const unsigned long long* __restrict__ best, int max_det,
                                                        const fdcm_match* __restrict__ rec, const float* __restrict__ q,
                                                        const int4* __restrict__ boxes, const float* __restrict__ frac,
                                                        MatchOut* __restrict__ out) {
    const int l = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (l >= max_det) return;
    const unsigned long long key = best[l];
    MatchOut o{};
    o.idx = -1;
    if (key != kNoKey) {
        const unsigned j = (unsigned)key;
        o.rec = rec[j];
        o.rec.score = q[j];
        o.box = boxes[j];
        o.frac = frac[j];
        o.idx = (int)j;
    }
    out[l] = o;
}

// ---- the shapes of a match list on the device (include/fdcm.h, "Match lists: objects and hull shapes"): per record that
// needs one, the rows and the area of the convex hull of its posed end points, what hull_of and hull_rows make on the host.
//   k_shape_rows<PHASE>   the rows each record has in the span table, by a scan over the box heights in three launches:
//                         0: the sum of each run of 256 records; 1: one workgroup turns the sums into their exclusive prefix
//                         and writes the total behind them; 2: HullShape{0, row0, 0} of every record.
//   k_matches_shapes      a wave per record.  Gift wrapping from the lowest, leftmost vertex: each step poses the template's
//                         resident lines again, a lane per line, and takes the vertex that has no other to its right, the
//                         farthest of collinear ones, by a wave reduction on exact cross products.  Every hull edge updates
//                         xl / xr of the rows it reaches; row r of the box belongs to lane r % 64 from the first write to the
//                         last, so nothing is shared.  A last pass moves the rows into the box's frame and sums the area.
// Every loop is bounded by the vertex count or the box height; nothing waits, nothing is atomic.
struct ShapesArgs {
    const float4* tlines;
    const long long* toff;
    const fdcm_match* rec;
    const unsigned long long* keys;  // the records with a key need a shape; null: those with an object
    const int* obj;
    const int4* boxes;
    HullShape* shapes;
    long long* sums;  // ceil(n / 256) + 1
    int2* spans;
    int n, base, margin;
};

__device__ __forceinline__ long long shape_rows_of(const ShapesArgs& a, int j) {
    if (j >= a.n || !(a.keys ? a.keys[j] != kNoKey : a.obj[j] >= 0)) return 0;
    const int4 b = a.boxes[j];
    return b.w < b.y ? 0 : (long long)b.w - b.y + 1;
}

// exclusive prefix of v over the 256 threads of a workgroup and their total (sw: 4 words of LDS, a barrier inside)
__device__ __forceinline__ long long block_scan_excl64(long long v, long long* sw, long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) sw[wave] = incl;
    __syncthreads();
    long long before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long s = sw[k];
        if (k < wave) before += s;
        total += s;
    }
    return before + incl - v;
}

template <int PHASE>
__global__ void __launch_bounds__(256) k_shape_rows(const ShapesArgs a) {
    __shared__ long long sw[4];
    const int nb = (a.n + 255) / 256;
    long long total;
    if (PHASE == 1) {  // one workgroup: thread i owns the sums [i per, (i + 1) per)
        const int per = (nb + 255) / 256, b0 = min(nb, (int)threadIdx.x * per), b1 = min(nb, b0 + per);
        long long mine = 0;
        for (int b = b0; b < b1; ++b) mine += a.sums[b];
        long long at = block_scan_excl64(mine, sw, total);
        for (int b = b0; b < b1; ++b) {
            const long long v = a.sums[b];
            a.sums[b] = at;
            at += v;
        }
        if (threadIdx.x == 0) a.sums[nb] = total;
        return;
    }
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const long long rows = shape_rows_of(a, j);
    const long long before = block_scan_excl64(rows, sw, total);
    if (PHASE == 0) {
        if (threadIdx.x == 0) a.sums[blockIdx.x] = total;
    } else if (j < a.n) {  // (a table of more than 2^26 rows is refused before a row0 is read)
        a.shapes[j] = HullShape{0, (int)min(a.sums[blockIdx.x] + before, 0x7fffffffll), 0};
    }
}

__device__ __forceinline__ long long floor_div_dev(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// The candidate (px, py) against the best (bx, by) of a step from (cx, cy); (bx, by) == (cx, cy): none yet.  All vertices lie
// in a cone of less than 180 degrees at a hull vertex, so "to the right of" orders their directions.
__device__ __forceinline__ void shape_better(int cx, int cy, int px, int py, int& bx, int& by) {
    if (px == cx && py == cy) return;
    const long long ux = bx - cx, uy = by - cy, vx = px - cx, vy = py - cy;
    const long long cr = ux * vy - uy * vx;  // < 0: p lies to the right of c -> b
    if ((ux == 0 && uy == 0) || cr < 0 || (cr == 0 && vx * vx + vy * vy > ux * ux + uy * uy)) { bx = px; by = py; }
}

// xl / xr of the rows the edge (ax, ay) - (ex, ey) reaches, hull_rows' arithmetic; sp: the record's rows, y0 its first.
__device__ __forceinline__ void shape_edge(int ax, int ay, int ex, int ey, int y0, int rows, int2* sp, int lane) {
    if (ay > ey) { int t = ax; ax = ex; ex = t; t = ay; ay = ey; ey = t; }
    const int r0 = ay - y0, r1 = ey - y0;
    const int first = r0 + ((lane - r0) & 63);  // the first row >= r0 of this lane
    const int iters = first > r1 ? 0 : (r1 - first) / 64 + 1;
    const long long dy = (long long)ey - ay, dx = (long long)ex - ax;
    for (int k = 0; k < iters; ++k) {
        const int r = first + 64 * k;
        if ((unsigned)r >= (unsigned)rows) continue;  // (never: the box is the vertices' own)
        int lo, hi;
        if (dy == 0) {
            lo = min(ax, ex); hi = max(ax, ex);
        } else {  // x* = num / dy, exact
            const long long num = (long long)ax * dy + dx * (long long)(r - r0);
            const long long q = floor_div_dev(num, dy);
            hi = (int)q;
            lo = (int)(q + (num - q * dy != 0 ? 1 : 0));
        }
        int2 s = sp[r];
        s.x = min(s.x, lo); s.y = max(s.y, hi);
        sp[r] = s;
    }
}

__global__ void __launch_bounds__(256) k_matches_shapes(const ShapesArgs a) {
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (j >= a.n) return;  // wave-uniform
    const int4 box = a.boxes[j];
    const int rows = (int)shape_rows_of(a, j);
    if (rows <= 0) return;  // wave-uniform: no shape
    const fdcm_match R = a.rec[j];
    const long long t = (long long)R.tmpl_idx - (long long)a.base;  // valid: the record has a key or an object
    const long long l0 = a.toff[t];
    const int nl = (int)(a.toff[t + 1] - l0);
    const MatchTransform M{R.transform[0], R.transform[1], R.transform[2], R.transform[3], R.transform[4], R.transform[5]};
    int2* const sp = a.spans + a.shapes[j].row0;
    const int m = a.margin, corners = m > 0 ? 4 : 1;
    for (int r = lane; r < rows; r += 64) sp[r] = make_int2(0x7fffffff, (int)0x80000000);
    // every vertex of the lines of this lane: per end point the corners clamp(floor(v) -+ m), hull_of's
    auto vertices = [&](auto&& f) {
        for (int i = lane; i < nl; i += 64) {
            const float4 p = match_pose_line(M, a.tlines[l0 + i]);
            for (int e = 0; e < 2; ++e) {
                const float fx = e ? p.z : p.x, fy = e ? p.w : p.y;
                for (int k = 0; k < corners; ++k) f(matches_side(fx, k & 1 ? m : -m), matches_side(fy, k & 2 ? m : -m));
            }
        }
    };
    // the start: the lowest vertex, the leftmost of those
    long long sk = 0x7fffffffffffffffll;
    vertices([&](int x, int y) { sk = min(sk, (long long)(((unsigned long long)(unsigned)(y + (1 << 26)) << 32) | (unsigned)(x + (1 << 26)))); });
    for (int d = 32; d >= 1; d >>= 1) sk = min(sk, (long long)__shfl_xor(sk, d));
    const int sx = __builtin_amdgcn_readfirstlane((int)(unsigned)sk - (1 << 26));
    const int sy = __builtin_amdgcn_readfirstlane((int)(unsigned)(sk >> 32) - (1 << 26));
    const long long steps = (long long)nl * 2 * corners + 1;  // the hull has at most V vertices
    int cx = sx, cy = sy;
    for (long long step = 0; step < steps; ++step) {
        int bx = cx, by = cy;
        vertices([&](int x, int y) { shape_better(cx, cy, x, y, bx, by); });
        for (int d = 32; d >= 1; d >>= 1) {
            const int ox = __shfl_xor(bx, d), oy = __shfl_xor(by, d);
            shape_better(cx, cy, ox, oy, bx, by);
        }
        bx = __builtin_amdgcn_readfirstlane(bx);
        by = __builtin_amdgcn_readfirstlane(by);
        shape_edge(cx, cy, bx, by, box.y, rows, sp, lane);  // (one vertex: the edge from it to itself)
        if ((bx == cx && by == cy) || (bx == sx && by == sy)) break;  // wave-uniform
        cx = bx; cy = by;
    }
    long long area = 0;
    for (int r = lane; r < rows; r += 64) {
        const int2 s = sp[r];
        const bool none = s.x > s.y;
        if (!none) area += (long long)s.y - s.x + 1;
        sp[r] = none ? make_int2(0, -1) : make_int2(s.x - box.x, s.y - box.x);
    }
    for (int d = 32; d >= 1; d >>= 1) area += __shfl_xor(area, d);
    if (lane == 0) a.shapes[j].area = area;
}

// P(r) of a valid record on the host: the kernel's arithmetic (the Makefile's -ffp-contract=off keeps it unfused here too).
// Q: a rotation in front of M, "Rotations"' arithmetic (the refinement's delta), or null.
void pose_lines(const fdcm_templates* t, int64_t tmpl, const float* M, std::vector<float>& out, const RotM* Q = nullptr) {
    const int64_t l0 = t->offsets[(size_t)tmpl], nl = t->offsets[(size_t)tmpl + 1] - l0;
    out.resize((size_t)nl * 4);
    for (int64_t i = 0; i < nl; ++i) {
        const float* p = &t->lines[(size_t)(l0 + i) * 4];
        float* o = &out[(size_t)i * 4];
        for (int c = 0; c < 2; ++c) {
            float x = p[2 * c], y = p[2 * c + 1];
            if (Q) {
                const float qx = (Q->c * x + Q->ns * y) + Q->mx, qy = (Q->s * x + Q->c * y) + Q->my;
                x = qx;
                y = qy;
            }
            o[2 * c] = (M[0] * x + M[1] * y) + M[2];
            o[2 * c + 1] = (M[3] * x + M[4] * y) + M[5];
        }
    }
}

// The bins of posed lines from the host libm, one per line.
void posed_bins(const fdcm_featuremap* fm, const std::vector<float>& posed, unsigned short* out) {
    for (size_t i = 0; i < posed.size() / 4; ++i) {
        const float* p = &posed[4 * i];
        const float angle = std::atan((p[3] - p[1]) / (p[2] - p[0]));  // getAngle, math.h:295-299
        out[i] = (unsigned short)closest_orientation(fm->keys.data(), (int)fm->m, angle);
    }
}

// P(r) and F(r) of record r; false, with F empty, for a record that is not valid.
bool pose_record(const fdcm_templates* t, const fdcm_match& r, int32_t base, int margin, std::vector<float>& posed, Foot& F) {
    const int64_t tm = (int64_t)r.tmpl_idx - base;
    F = Foot{0, 0, -1, -1};
    if (tm < 0 || tm >= t->T) return false;
    pose_lines(t, tm, r.transform, posed);
    F = footprint(posed.data(), 4, (int64_t)(posed.size() / 4), margin);
    return true;
}

}  // namespace

// Host only: F(r) of every record (include/fdcm.h, "Match lists").
void matches_footprints(const fdcm_templates* t, const fdcm_match* matches, int64_t n, int32_t base, int margin, int32_t* boxes_out) {
    std::vector<float> posed;
    for (int64_t j = 0; j < n; ++j) {
        Foot F;
        pose_record(t, matches[j], base, margin, posed, F);
        std::memcpy(boxes_out + 4 * j, &F, sizeof F);
    }
}

// Host only: the hull shape of every record ("Match lists: objects and hull shapes"), hull_of and hull_rows on P(r).
void matches_footprint_spans(const fdcm_templates* t, const fdcm_match* matches, int64_t n, int32_t base, int margin, int64_t* row_offsets,
                             int64_t* areas, int32_t* spans) {
    std::vector<float> posed;
    std::vector<HullPt> h;
    row_offsets[0] = 0;
    for (int64_t j = 0; j < n; ++j) {
        Foot F;
        pose_record(t, matches[j], base, margin, posed, F);
        row_offsets[j + 1] = row_offsets[j] + foot_rows(F);
        if (areas) areas[j] = 0;
        if ((!areas && !spans) || foot_rows(F) == 0) continue;
        hull_of(posed.data(), 4, (int64_t)(posed.size() / 4), margin, h);
        const int64_t A = hull_rows(h, F, spans ? spans + 2 * row_offsets[j] : nullptr);
        if (areas) areas[j] = A;
    }
}

// Host-libm bins (fdcm_orientation_bins_mode() == 1; empty otherwise): the bins of every posed line as [record][max_lines], on
// the host, from host records; device records cost one download on the handle's stream.
void matches_host_bins(fdcm_featuremap* fm, const fdcm_templates* t, const MatchList& m, std::vector<unsigned short>& bins) {
    bins.clear();
    if (!orientation_bins_on_host()) return;
    if (fm->m > 65535) throw std::string("host-side orientation bins need depth <= 65535");
    const size_t N = (size_t)m.n, Lmax = (size_t)t->max_lines;
    std::vector<fdcm_match> fetched;
    const fdcm_match* h = m.rec;
    if (m.on_device) {
        fetched.resize(N);
        FDCM_HIP(hipMemcpyAsync(fetched.data(), m.rec, N * sizeof(fdcm_match), hipMemcpyDeviceToHost, fm->stream));
        FDCM_HIP(hipStreamSynchronize(fm->stream));
        h = fetched.data();
    }
    bins.assign(std::max<size_t>(1, N * Lmax), 0);
    std::vector<float> posed;
    for (size_t j = 0; j < N; ++j) {
        const int64_t tm = (int64_t)h[j].tmpl_idx - m.base;
        if (tm < 0 || tm >= t->T) continue;
        pose_lines(t, tm, h[j].transform, posed);
        posed_bins(fm, posed, &bins[j * Lmax]);
    }
}

// ---- the device calls on match lists (include/fdcm.h, "Match lists"): run_matches and its stages
namespace {

// Where the stages left what: offsets into d = search.eval.  Everything before o_score is written by the one upload.
struct MatchesRun {
    const MatchesObjectsIn* ob = nullptr;  // the objects of the pass: the caller's, or the shapes call's one object; null: none
    bool hull = false;                     // the records' hull shapes are built
    size_t N = 0, Lmax = 0;
    char* d = nullptr;
    size_t o_ms = 0, o_tobj = 0, o_score = 0, o_frac = 0, o_costs = 0, o_best = 0, o_pk = 0, o_obj = 0, o_shape = 0, o_sums = 0;
    MatchesArgs a{};  // the verify pass's: the records, and the scores, keys and boxes it leaves
    ShapesArgs sa{};  // the hull shapes', with the span table
};

// Stage 1.  One reserve_eval lays out the whole call: the upload (host records, caps, denominators, needs, totals, the
// objects' tables, host bins), the list's arrays, the result list, the rounds' partials, and with objects or shapes the
// records' objects, shapes and the scan's sums.  One copy takes the upload to the device.
void matches_upload(fdcm_featuremap* fm, const fdcm_templates* t, const MatchesIn& in, MatchesRun& R) {
    const MatchList& m = in.list;
    const MatchesDetect* det = in.det;
    const MatchesObjectsIn* ob = R.ob;
    const size_t N = R.N = (size_t)m.n, T = (size_t)t->T, Lmax = R.Lmax = (size_t)t->max_lines;
    const bool gated = ob ? ob->min_matched && std::any_of(ob->min_matched, ob->min_matched + ob->G, [](float v) { return v > 0.f; })
                          : det && det->min_matched > 0.f;
    const std::vector<float> den = best_denominators(t, det ? det->penalty : -1, det ? det->tau : 1.f);
    std::vector<float> totals(T);
    templates_matched_totals(t, totals.data());
    std::vector<unsigned short> bins;
    matches_host_bins(fm, t, m, bins);
    const int max_det = det ? det->max_detections : 0;
    const bool costs = in.verify.costs != nullptr;
    const size_t o_caps = m.on_device ? 0 : al256(N * sizeof(fdcm_match)), o_den = o_caps + (t->capped ? al256((size_t)t->n_lines * 4) : 0),
                 o_need = o_den + al256(T * 4), o_tl = o_need + (gated ? al256(T * 4) : 0), o_ms = R.o_ms = o_tl + al256(T * 4),
                 o_tobj = R.o_tobj = o_ms + (ob ? al256(T * 4) : 0), o_bins = o_tobj + (ob ? al256(T * 4) : 0),
                 o_score = R.o_score = o_bins + (bins.empty() ? 0 : al256(bins.size() * 2)), o_frac = R.o_frac = o_score + al256(N * 4),
                 o_q = o_frac + al256(N * 4), o_keys = o_q + al256(N * 4), o_box = o_keys + al256(N * 8),
                 o_costs = R.o_costs = o_box + al256(N * 16), o_best = R.o_best = o_costs + (costs ? al256(N * Lmax * 4) : 0),
                 o_pk = R.o_pk = o_best + al256((size_t)max_det * 8), o_obj = R.o_obj = o_pk + 2 * kNmsWorkgroups * 8,
                 o_shape = R.o_shape = o_obj + (ob ? al256(N * 4) : 0), o_sums = R.o_sums = o_shape + (R.hull ? al256(N * sizeof(HullShape)) : 0),
                 total = o_sums + (R.hull ? al256(((N + 255) / 256 + 1) * 8) : 0);
    reserve_eval(fm, total, o_score);
    char* d = R.d = (char*)fm->search.eval.p;
    char* h = (char*)fm->search.eval_stage.p;
    if (!m.on_device) std::memcpy(h, m.rec, N * sizeof(fdcm_match));
    if (t->capped) std::memcpy(h + o_caps, t->caps.data(), (size_t)t->n_lines * 4);
    std::memcpy(h + o_den, den.data(), T * 4);
    if (gated && !ob)
        for (size_t i = 0; i < T; ++i) ((float*)(h + o_need))[i] = det->min_matched * totals[i];  // need = float32(min_matched * TL)
    if (gated && ob)  // the need of the template's object; an object without a gate: every ML passes
        for (size_t i = 0; i < T; ++i) {
            const float mm = ob->min_matched[ob->objects[i]];
            ((float*)(h + o_need))[i] = mm > 0.f ? mm * totals[i] : -f_inf();
        }
    if (ob)
        for (size_t i = 0; i < T; ++i) {
            ((float*)(h + o_ms))[i] = ob->max_score[ob->objects[i]];
            ((int32_t*)(h + o_tobj))[i] = ob->objects[i];
        }
    std::memcpy(h + o_tl, totals.data(), T * 4);
    if (!bins.empty()) std::memcpy(h + o_bins, bins.data(), bins.size() * 2);
    FDCM_HIP(hipMemcpyAsync(d, h, o_score, hipMemcpyHostToDevice, fm->stream));
    MatchesArgs& a = R.a;
    a.vol = fm->vol.as<float>(); a.SL = ivol_slice_floats(fm->W, fm->H); a.m = (int)fm->m; a.W = (int)fm->W; a.H = (int)fm->H;
    a.tx = fm->tx; a.ty = fm->ty; a.keys = (const float*)((const char*)fm->build.plan.p + fm->off_keys);
    a.tlines = t->d_lines.as<float4>(); a.tlen = t->d_lengths.as<float>(); a.toff = t->d_offsets.as<long long>();
    a.caps = t->capped ? (const float*)(d + o_caps) : nullptr;
    a.den = (const float*)(d + o_den);
    a.need = gated ? (const float*)(d + o_need) : nullptr;
    a.tl = (const float*)(d + o_tl);
    a.bins = bins.empty() ? nullptr : (const unsigned short*)(d + o_bins);
    a.rec = m.on_device ? m.rec : (const fdcm_match*)d;
    a.n = (int)m.n; a.base = m.base; a.T = (int)std::min<int64_t>(t->T, 0x7fffffff); a.Lmax = (int)Lmax;
    a.margin = det ? det->margin : in.shapes ? in.shapes->margin : 0; a.rescore = det ? det->rescore : 0;
    a.max_score = det ? det->max_score : f_inf();
    a.score = (float*)(d + o_score); a.frac = (float*)(d + o_frac); a.q = (float*)(d + o_q);
    a.costs = costs ? (float*)(d + o_costs) : nullptr;
    a.keys_out = (unsigned long long*)(d + o_keys);
    a.boxes = (int4*)(d + o_box);
}

// Stage 2.  The verify pass: s, frac, q, the key and the box of every record, with objects the record's object.
void matches_verify_pass(fdcm_featuremap* fm, const fdcm_templates* t, const MatchesRun& R) {
    const bool buf32 = !test_switches().matched_flat && (size_t)fm->m * R.a.SL * sizeof(float) < ((size_t)1 << 32);  // the rule k_search uses
    auto kern = buf32 ? (t->capped ? k_matches_verify<true, true, false> : k_matches_verify<true, false, false>)
                      : (t->capped ? k_matches_verify<false, true, false> : k_matches_verify<false, false, false>);
    auto kern_ob = buf32 ? (t->capped ? k_matches_verify<true, true, true> : k_matches_verify<true, false, true>)
                         : (t->capped ? k_matches_verify<false, true, true> : k_matches_verify<false, false, true>);
    const MatchesObjArgs oa{(const float*)(R.d + R.o_ms), (const int*)(R.d + R.o_tobj), (int*)(R.d + R.o_obj)};
    hipLaunchKernelGGL(R.ob ? kern_ob : kern, dim3((unsigned)((R.N + 3) / 4)), dim3(256), 0, fm->stream, R.a, R.ob ? oa : MatchesObjArgs{});
    FDCM_HIP(hipGetLastError());
}

// Stage 3.  Hull shapes: the rows of every record that needs a shape by a scan on the device, whose total alone comes to the
// host, for the limit and for the size of the span table; then the shapes.  The table is a buffer of its own, so nothing here
// moves the workspace the pass has written; under FDCM_POISON it holds the word wherever the kernel does not write.
// Returns the rows of the table.
long long matches_hull_shapes(fdcm_featuremap* fm, const MatchesIn& in, MatchesRun& R) {
    hipStream_t st = fm->stream;
    ShapesArgs& sa = R.sa;
    sa.tlines = R.a.tlines; sa.toff = R.a.toff; sa.rec = R.a.rec;
    sa.keys = in.shapes ? nullptr : R.a.keys_out; sa.obj = (const int*)(R.d + R.o_obj); sa.boxes = R.a.boxes;
    sa.shapes = (HullShape*)(R.d + R.o_shape); sa.sums = (long long*)(R.d + R.o_sums);
    sa.n = R.a.n; sa.base = R.a.base; sa.margin = R.a.margin;
    const unsigned nb = (unsigned)((R.N + 255) / 256);
    hipLaunchKernelGGL(k_shape_rows<0>, dim3(nb), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_shape_rows<1>, dim3(1), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_shape_rows<2>, dim3(nb), dim3(256), 0, st, sa);
    FDCM_HIP(hipGetLastError());
    long long rows = 0;
    FDCM_HIP(hipMemcpyAsync(&rows, sa.sums + nb, 8, hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipStreamSynchronize(st));
    if (rows > kHullMaxRows)
        throw std::string("match lists: the span table of the candidates has more than 2^26 rows: cut the list with max_score or "
                          "fdcm_topk first");
    DevBuf& table = fm->search.eval_spans;
    table.reserve(std::max<size_t>(8, (size_t)rows * 8));
    poison_fill(table, st, FDCM_FILL_EVAL);  // (counted with the workspace it belongs to)
    sa.spans = table.as<int2>();
    if (!in.shapes || in.shapes->areas || in.shapes->spans) {
        hipLaunchKernelGGL(k_matches_shapes, dim3((unsigned)((R.N + 3) / 4)), dim3(256), 0, st, sa);
        FDCM_HIP(hipGetLastError());
    }
    return rows;
}

// The shapes call's delivery: the rows and areas of every record, and the table.
void matches_shapes_to_host(fdcm_featuremap* fm, const MatchesShapesOut& out, const MatchesRun& R, long long rows) {
    hipStream_t st = fm->stream;
    std::vector<HullShape> shapes(R.N);
    FDCM_HIP(hipMemcpyAsync(shapes.data(), R.sa.shapes, R.N * sizeof(HullShape), hipMemcpyDeviceToHost, st));
    if (out.spans && rows) FDCM_HIP(hipMemcpyAsync(out.spans, R.sa.spans, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipStreamSynchronize(st));
    for (size_t j = 0; j < R.N; ++j) {
        out.row_offsets[j] = shapes[j].row0;
        if (out.areas) out.areas[j] = shapes[j].area;
    }
    out.row_offsets[R.N] = rows;
}

// The verify call's delivery: what the pass wrote, to the outputs that are not null.
void matches_verify_to_host(fdcm_featuremap* fm, const MatchesIn& in, const MatchesRun& R) {
    hipStream_t st = fm->stream;
    if (in.verify.scores) FDCM_HIP(hipMemcpyAsync(in.verify.scores, R.d + R.o_score, R.N * 4, hipMemcpyDeviceToHost, st));
    if (in.verify.fractions) FDCM_HIP(hipMemcpyAsync(in.verify.fractions, R.d + R.o_frac, R.N * 4, hipMemcpyDeviceToHost, st));
    if (in.verify.costs && R.Lmax) FDCM_HIP(hipMemcpyAsync(in.verify.costs, R.d + R.o_costs, R.N * R.Lmax * 4, hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipStreamSynchronize(st));  // (the host arrays stay alive until here)
}

// The detect calls' delivery: the rounds, the list form on the keys and boxes the pass wrote (the result list begins as kNoKey
// throughout); the gather into pinned memory, 64-byte entries; and the host's packing of them into the records at the array's front.
void matches_detect_to_host(fdcm_featuremap* fm, const MatchesIn& in, const MatchesRun& R) {
    hipStream_t st = fm->stream;
    const MatchesDetect& det = *in.det;
    const int max_det = det.max_detections;
    unsigned long long* d_best = (unsigned long long*)(R.d + R.o_best);
    FDCM_HIP(hipMemsetAsync(d_best, 0xff, (size_t)max_det * 8, st));
    NmsArgs r{};  // a list form: no planes, no pairs, boxes whatever the set's kind
    r.keys = R.a.keys_out; r.boxes = R.a.boxes;
    r.n = (long long)R.N; r.n_chunks = (r.n + 255) / 256;
    r.permille = det.overlap_permille; r.cross = R.ob ? R.ob->cross : det.overlap_permille;
    if (R.ob) r.obj = (const int*)(R.d + R.o_obj);
    if (R.hull) { r.shapes = R.sa.shapes; r.spans = R.sa.spans; }
    r.pk_out = (unsigned long long*)(R.d + R.o_pk); r.best = d_best;
    nms_rounds(r, (unsigned)std::min<long long>(kNmsWorkgroups, r.n_chunks), max_det, st);
    fdcm_match*& out = *in.detect.out;
    out = result_acquire((size_t)max_det * sizeof(MatchOut));
    MatchOut* out_dev = nullptr;
    FDCM_HIP(hipHostGetDevicePointer((void**)&out_dev, out, 0));
    hipLaunchKernelGGL(k_matches_gather, dim3((unsigned)((max_det + 255) / 256)), dim3(256), 0, st, (const unsigned long long*)d_best, max_det,
                       R.a.rec, (const float*)R.a.q, (const int4*)R.a.boxes, (const float*)R.a.frac, out_dev);
    FDCM_HIP(hipGetLastError());
    FDCM_HIP(hipStreamSynchronize(st));  // (the host arrays stay alive until here)
    int64_t k = 0;
    for (; k < max_det; ++k) {
        MatchOut o;
        std::memcpy(&o, (const char*)out + (size_t)k * sizeof(MatchOut), sizeof o);
        if (o.idx < 0) break;
        std::memcpy((char*)out + (size_t)k * sizeof(fdcm_match), &o.rec, sizeof(fdcm_match));  // (in front of entry k, or in it)
        if (in.detect.indices) in.detect.indices[k] = o.idx;
        if (in.detect.boxes) std::memcpy(in.detect.boxes + 4 * k, &o.box, 16);
        if (in.detect.matched) in.detect.matched[k] = o.frac;
    }
    *in.detect.n_out = k;
}

}  // namespace

// The device calls on match lists: the arguments are checked (fdcm_capi.cpp).  What `in` names selects the call
// (fdcm_internal.h): the verify call, the detect call, with objects or without, or the shapes call.  Every call is the upload
// and the verify pass; the hull shapes where the overlap rule or the caller needs them -- with neither objects nor shapes,
// nothing of "Match lists: objects and hull shapes" is laid out, launched or read --; and its own delivery.
void run_matches(fdcm_featuremap* fm, const fdcm_templates* t, const MatchesIn& in) {
    const int64_t n = in.list.n;
    if (in.detect.n_out) *in.detect.n_out = 0;
    if (in.shapes) std::fill_n(in.shapes->row_offsets, n + 1, (int64_t)0);
    if (in.shapes && in.shapes->areas) std::fill_n(in.shapes->areas, n, (int64_t)0);
    if (n == 0 || t->T == 0 || fm->W == 0 || fm->H == 0 || fm->m == 0) return;
    // The shapes call is the pass with one object and no threshold, whose table of objects says which records are valid and
    // admissible and have lines.
    const std::vector<int32_t> one_object(in.shapes ? (size_t)t->T : 0, 0);
    const float no_limit = f_inf();
    const MatchesObjectsIn all{one_object.data(), 1, &no_limit, nullptr, 1000};
    MatchesRun R;
    R.ob = in.shapes ? &all : in.objects;
    R.hull = in.shapes || (R.ob && t->footprint == FDCM_FOOTPRINT_HULL);
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    begin(fm);
    matches_upload(fm, t, in, R);
    matches_verify_pass(fm, t, R);
    const long long rows = R.hull ? matches_hull_shapes(fm, in, R) : 0;
    if (in.shapes) return matches_shapes_to_host(fm, *in.shapes, R, rows);
    if (!in.det) return matches_verify_to_host(fm, in, R);
    matches_detect_to_host(fm, in, R);
}

// ---- match lists: refinement (include/fdcm.h, "Match lists: refinement"): every record's own box of (delta rotation, dx, dy)
// searched exhaustively, the record replaced by its best pose.  Nothing per record comes from the host (but the bins, where
// the host's libm makes them).  A plane is one (record, run position e); every record has the same window, so the table of
// patches is implicit: item = plane * patches per plane + patch.
//   k_refine_pose                 a wave per plane, a lane per line in rounds of 64: the ExLine entries of P_e(r) (Q_e(t) by
//                                 "Rotations"' arithmetic, posed by M as match_pose_line; the bin by atanf_glibc +
//                                 closest_orientation as k_matches_verify, or the host's), the extremes of the posed coordinates
//                                 by wave reductions, and from them the admissible box in window indices: float addition is
//                                 monotone, so a column or a row is admissible exactly when its two extreme coordinates are
//                                 -- decided before any read of the volume
//   k_refine_score<BUF32, CAP>    a wave per item, a lane per translation of a 4 x 16 patch of the window as
//                                 k_exhaustive_windows; a patch that misses the box reads nothing, a lane outside the box
//                                 reads at the box's corner; rows_score<BUF32, 1, CAP>, unchanged; the patch's smallest key by a
//                                 wave reduction, one 8-byte store per item
//   k_refine_write                a wave per record: the smallest of its items' keys, then lane 0 writes the record and its pose
// No atomics: an item's key has one writer, and the minimum of a record's keys does not depend on an order.
namespace {

struct RefinePlane {
    int n;               // lines to score; 0: nothing (invalid record, no lines, an empty box)
    int i0, i1, j0, j1;  // the admissible box in window indices, i in [0, 2 hx], j in [0, 2 hy]
    int pad[3];
};
static_assert(sizeof(RefinePlane) == 32, "RefinePlane is 32 bytes");

struct RefineArgs {
    const float* vol;
    size_t SL;
    int m, W, H;
    float tx, ty;
    const float* keys;           // the map's m orientation keys
    const float4* tlines;        // the set's resident lines and offsets
    const long long* toff;
    const float* caps;           // per line of the set, or null: none
    const float* cs;             // na pairs (c, s), or null: nothing rotated
    const float* pivots;         // T pairs, or null: the origin
    const unsigned short* bins;  // [record of the part][e][Lmax] from the host libm, or null
    const fdcm_match* rec;       // the whole list
    int r0, nr;                  // the part: records r0 .. r0 + nr - 1
    int base, T, Lmax, na, centre, hx, hy, sx, sy;
    int ppx, ppp;                // patches per window row, per plane
    bool buf32;
    ExLine* lines;               // [plane of the part][Lmax]
    RefinePlane* planes;
    unsigned long long* ikeys;   // per item of the part
    fdcm_match* out;             // the whole list's
    int* pose;                   // n x 3, or null
};

// [R | m] of run position e for template t, rot_matrix's arithmetic
__device__ __forceinline__ RotM refine_rot(const RefineArgs& a, int e, long long t) {
    const float c = a.cs[2 * e], s = a.cs[2 * e + 1];
    const float px = a.pivots ? a.pivots[2 * t] : 0.f, py = a.pivots ? a.pivots[2 * t + 1] : 0.f;
    const float ns = -s;
    return RotM{c, ns, s, px - (c * px + ns * py), py - (s * px + c * py)};
}

__global__ void __launch_bounds__(256) k_refine_pose(const RefineArgs a) {
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (p >= a.nr * a.na) return;  // wave-uniform
    const int rl = p / a.na, e = p - rl * a.na;
    const fdcm_match R = a.rec[a.r0 + rl];
    const long long t = (long long)R.tmpl_idx - (long long)a.base;
    RefinePlane P{0, 0, -1, 0, -1, {0, 0, 0}};
    const bool valid = t >= 0 && t < a.T;
    const long long l0 = valid ? a.toff[t] : 0;
    const int nl = valid ? (int)(a.toff[t + 1] - l0) : 0;
    if (nl == 0) {  // wave-uniform
        if (lane == 0) a.planes[p] = P;
        return;
    }
    const MatchTransform M{R.transform[0], R.transform[1], R.transform[2], R.transform[3], R.transform[4], R.transform[5]};
    RotM Q{};
    if (a.cs) Q = refine_rot(a, e, t);
    ExLine* const L = a.lines + (size_t)p * (size_t)a.Lmax;
    bool has_nan = false;
    float mnx = f_inf(), mny = f_inf(), mxx = -f_inf(), mxy = -f_inf();
    for (int i = lane; i < nl; i += 64) {
        float4 q = a.tlines[l0 + i];
        if (a.cs)  // Q_e(t): transform, math.h:341-344, as rotated_set
            q = make_float4((Q.c * q.x + Q.ns * q.y) + Q.mx, (Q.s * q.x + Q.c * q.y) + Q.my, (Q.c * q.z + Q.ns * q.w) + Q.mx,
                            (Q.s * q.z + Q.c * q.w) + Q.my);
        const float4 v = match_pose_line(M, q);
        int bin;
        if (a.bins) {
            bin = (int)a.bins[(size_t)p * (size_t)a.Lmax + i];
        } else {
            const float angle = atanf_glibc((v.w - v.y) / (v.z - v.x));  // getAngle, math.h:295-299
            bin = closest_orientation(a.keys, a.m, angle);              // dt3cpu.cpp:144-148
        }
        L[i] = ExLine{v.x, v.y, v.z, v.w, a.buf32 ? (int)((unsigned)bin * (unsigned)a.SL) : bin, a.caps ? a.caps[l0 + i] : f_inf(), 0.f, 0};
        has_nan = has_nan || f_isnan(v.x) || f_isnan(v.y) || f_isnan(v.z) || f_isnan(v.w);
        mnx = std_min(mnx, std_min(v.x, v.z)); mxx = std_max(mxx, std_max(v.x, v.z));
        mny = std_min(mny, std_min(v.y, v.w)); mxy = std_max(mxy, std_max(v.y, v.w));
    }
    const bool any_nan = __ballot(has_nan) != 0;
    mnx = wave_min_f(mnx); mny = wave_min_f(mny); mxx = wave_max_f(mxx); mxy = wave_max_f(mxy);
    // the admissible columns and rows: the seam's rule on the extremes, offset = T + tau summed first
    int i0 = 0x7fffffff, i1 = -1, j0 = 0x7fffffff, j1 = -1;
    if (!any_nan) {
        for (int i = lane; i <= 2 * a.hx; i += 64) {
            const float off = a.tx + (float)((i - a.hx) * a.sx);
            if (mnx + off > -1.f && mxx + off < (float)a.W) { i0 = min(i0, i); i1 = max(i1, i); }
        }
        for (int j = lane; j <= 2 * a.hy; j += 64) {
            const float off = a.ty + (float)((j - a.hy) * a.sy);
            if (mny + off > -1.f && mxy + off < (float)a.H) { j0 = min(j0, j); j1 = max(j1, j); }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        i0 = min(i0, __shfl_xor(i0, d)); i1 = max(i1, __shfl_xor(i1, d));
        j0 = min(j0, __shfl_xor(j0, d)); j1 = max(j1, __shfl_xor(j1, d));
    }
    if (i0 <= i1 && j0 <= j1) P = RefinePlane{nl, i0, i1, j0, j1, {0, 0, 0}};
    if (lane == 0) a.planes[p] = P;
}

template <bool BUF32, bool CAP>
__global__ void __launch_bounds__(256) k_refine_score(const RefineArgs a) {
    const int lane = threadIdx.x & 63;
    const long long w = ((long long)blockIdx.x * 4 + (long long)(threadIdx.x >> 6));
    const long long n_items = (long long)a.nr * a.na * a.ppp;
    if (w >= n_items) return;  // wave-uniform
    const int p = __builtin_amdgcn_readfirstlane((int)(w / a.ppp)), patch = __builtin_amdgcn_readfirstlane((int)(w % a.ppp));
    const RefinePlane P = a.planes[p];
    const int ib = (patch % a.ppx) * kPatchX, jb = (patch / a.ppx) * kPatchY;
    unsigned long long key = kNoKey;
    if (P.n > 0 && ib <= P.i1 && ib + kPatchX > P.i0 && jb <= P.j1 && jb + kPatchY > P.j0) {  // wave-uniform
        const VolRef V = make_volref(a.vol, a.SL, a.m, BUF32);
        const int i = ib + (lane & 3), j = jb + (lane >> 2);
        // a lane outside the box reads at the box's corner, which is admissible: every read stays inside the volume
        const bool act = i >= P.i0 && i <= P.i1 && j >= P.j0 && j <= P.j1;
        const float offx = a.tx + (float)(((act ? i : P.i0) - a.hx) * a.sx);  // sceneTranslation + translation
        const float offy[1] = {a.ty + (float)(((act ? j : P.j0) - a.hy) * a.sy)};
        float res[1] = {0.f};
        rows_score<BUF32, 1, CAP>(V, a.lines + (size_t)p * (size_t)a.Lmax, P.n, offx, offy, a.W, (unsigned)a.H, a.SL, res);
        const int e = p % a.na, nxw = 2 * a.hx + 1;
        const unsigned N = (unsigned)nxw * (unsigned)(2 * a.hy + 1);
        const unsigned low = e == a.centre && i == a.hx && j == a.hy ? 0u : 1u + (unsigned)e * N + (unsigned)(j * nxw + i);
        if (act && !(res[0] != res[0])) key = ((unsigned long long)__float_as_uint(res[0]) << 32) | low;  // a NaN score has no key
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) key = min(key, __shfl_xor(key, d));
    }
    if (lane == 0) a.ikeys[w] = key;
}

__global__ void __launch_bounds__(256) k_refine_write(const RefineArgs a) {
    const int lane = threadIdx.x & 63;
    const int rl = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (rl >= a.nr) return;  // wave-uniform
    const long long per = (long long)a.na * a.ppp;
    const unsigned long long* const K = a.ikeys + (long long)rl * per;
    unsigned long long key = kNoKey;
    for (long long q = lane; q < per; q += 64) key = min(key, K[q]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) key = min(key, __shfl_xor(key, d));
    if (lane != 0) return;
    const int j = a.r0 + rl;
    fdcm_match R = a.rec[j];
    int e = -1, di = 0, dj = 0;
    if (key == kNoKey) {
        R.score = f_nan();
    } else {
        const unsigned low = (unsigned)key;
        const int nxw = 2 * a.hx + 1;
        const unsigned N = (unsigned)nxw * (unsigned)(2 * a.hy + 1);
        if (low == 0) {
            e = a.centre;
        } else {
            e = (int)((low - 1) / N);
            const int g = (int)((low - 1) % N);
            di = g % nxw - a.hx;
            dj = g / nxw - a.hy;
        }
        R.score = __uint_as_float((unsigned)(key >> 32));
        const float fx = (float)(di * a.sx), fy = (float)(dj * a.sy);
        const float M0 = R.transform[0], M1 = R.transform[1], M2 = R.transform[2], M3 = R.transform[3], M4 = R.transform[4], M5 = R.transform[5];
        if (a.cs) {
            const RotM Q = refine_rot(a, e, (long long)R.tmpl_idx - (long long)a.base);
            R.transform[0] = (M0 * Q.c + M1 * Q.s);
            R.transform[1] = (M0 * Q.ns + M1 * Q.c);
            R.transform[2] = ((M0 * Q.mx + M1 * Q.my) + M2) + fx;
            R.transform[3] = (M3 * Q.c + M4 * Q.s);
            R.transform[4] = (M3 * Q.ns + M4 * Q.c);
            R.transform[5] = ((M3 * Q.mx + M4 * Q.my) + M5) + fy;
        } else {
            R.transform[2] = M2 + fx;
            R.transform[5] = M5 + fy;
        }
    }
    a.out[j] = R;
    if (a.pose) { a.pose[3 * j] = e; a.pose[3 * j + 1] = di; a.pose[3 * j + 2] = dj; }
}

constexpr size_t kRefinePartBytes = (size_t)512 << 20;  // a part's lines, planes, keys and bins

}  // namespace

// fdcm_matches_refine: the arguments are checked (fdcm_capi.cpp).  One reserve_eval lays out the whole call: the upload (host
// records, caps, the delta table, the pivots, a part's host bins), the output records and poses of a list that leaves for the
// host, and a part's lines, planes and keys.  The list is walked in parts of at most kRefinePartBytes of those
// (FDCM_REFINE_PART: of that many records); a record is never cut.
void run_matches_refine(fdcm_featuremap* fm, const fdcm_templates* t, const MatchList& m, const fdcm_rotations* rot, int32_t centre,
                        int32_t hx, int32_t hy, int32_t sx, int32_t sy, fdcm_match* out, bool out_on_device, int32_t* pose_out) {
    if (m.n == 0 || t->T == 0 || fm->W == 0 || fm->H == 0 || fm->m == 0) return;
    std::lock_guard<std::mutex> turn(fm->seam_mutex);
    begin(fm);
    hipStream_t st = fm->stream;
    const size_t N = (size_t)m.n, T = (size_t)t->T, Lmax = (size_t)std::max<int64_t>(1, t->max_lines), na = rot ? (size_t)rot->n : 1;
    const size_t SL = ivol_slice_floats(fm->W, fm->H);
    const bool buf32 = !test_switches().matched_flat && (size_t)fm->m * SL * sizeof(float) < ((size_t)1 << 32);  // the rule k_search uses
    const bool host_bins = orientation_bins_on_host();
    if (host_bins && fm->m > 65535) throw std::string("host-side orientation bins need depth <= 65535");
    const int ppx = (2 * hx + kPatchX) / kPatchX, ppp = ppx * ((2 * hy + kPatchY) / kPatchY);  // ceil((2 h + 1) / patch)
    const size_t per = na * Lmax * sizeof(ExLine) + na * sizeof(RefinePlane) + na * (size_t)ppp * 8 + (host_bins ? na * Lmax * 2 : 0);
    size_t pn = std::max<size_t>(1, std::min(N, kRefinePartBytes / per));
    if (test_switches().refine_part > 0) pn = std::min(pn, (size_t)test_switches().refine_part);
    const bool pivots = rot && rot->pivots;
    const size_t o_caps = m.on_device ? 0 : al256(N * sizeof(fdcm_match)), o_cs = o_caps + (t->capped ? al256((size_t)t->n_lines * 4) : 0),
                 o_piv = o_cs + (rot ? al256(na * 8) : 0), o_bins = o_piv + (pivots ? al256(T * 8) : 0),
                 o_out = o_bins + (host_bins ? al256(pn * na * Lmax * 2) : 0), o_pose = o_out + (out_on_device ? 0 : al256(N * sizeof(fdcm_match))),
                 o_lines = o_pose + (pose_out ? al256(N * 12) : 0), o_planes = o_lines + al256(pn * na * Lmax * sizeof(ExLine)),
                 o_ikeys = o_planes + al256(pn * na * sizeof(RefinePlane)), total = o_ikeys + al256(pn * na * (size_t)ppp * 8);
    reserve_eval(fm, total, std::max<size_t>(o_out, 256));
    char* d = (char*)fm->search.eval.p;
    char* h = (char*)fm->search.eval_stage.p;
    if (!m.on_device) std::memcpy(h, m.rec, N * sizeof(fdcm_match));
    if (t->capped) std::memcpy(h + o_caps, t->caps.data(), (size_t)t->n_lines * 4);
    if (rot) std::memcpy(h + o_cs, rot->cs, na * 8);
    if (pivots) std::memcpy(h + o_piv, rot->pivots, T * 8);
    if (o_bins) FDCM_HIP(hipMemcpyAsync(d, h, o_bins, hipMemcpyHostToDevice, st));
    RefineArgs a{};
    a.vol = fm->vol.as<float>(); a.SL = SL; a.m = (int)fm->m; a.W = (int)fm->W; a.H = (int)fm->H; a.tx = fm->tx; a.ty = fm->ty;
    a.keys = (const float*)((const char*)fm->build.plan.p + fm->off_keys);
    a.tlines = t->d_lines.as<float4>(); a.toff = t->d_offsets.as<long long>();
    a.caps = t->capped ? (const float*)(d + o_caps) : nullptr;
    a.cs = rot ? (const float*)(d + o_cs) : nullptr;
    a.pivots = pivots ? (const float*)(d + o_piv) : nullptr;
    a.bins = host_bins ? (const unsigned short*)(d + o_bins) : nullptr;
    a.rec = m.on_device ? m.rec : (const fdcm_match*)d;
    a.base = m.base; a.T = (int)std::min<int64_t>(t->T, 0x7fffffff); a.Lmax = (int)Lmax; a.na = (int)na; a.centre = centre;
    a.hx = hx; a.hy = hy; a.sx = sx; a.sy = sy; a.ppx = ppx; a.ppp = ppp; a.buf32 = buf32;
    a.lines = (ExLine*)(d + o_lines); a.planes = (RefinePlane*)(d + o_planes); a.ikeys = (unsigned long long*)(d + o_ikeys);
    a.out = out_on_device ? out : (fdcm_match*)(d + o_out);
    a.pose = pose_out ? (int*)(d + o_pose) : nullptr;
    auto score = buf32 ? (t->capped ? k_refine_score<true, true> : k_refine_score<true, false>)
                       : (t->capped ? k_refine_score<false, true> : k_refine_score<false, false>);
    std::vector<fdcm_match> fetched;
    std::vector<float> posed;
    for (size_t r0 = 0; r0 < N; r0 += pn) {
        const size_t nr = std::min(pn, N - r0);
        a.r0 = (int)r0; a.nr = (int)nr;
        if (host_bins) {  // the bins of this part's planes from the host libm; device records cost one download per part
            const fdcm_match* hr = m.rec + r0;
            if (m.on_device) {
                fetched.resize(nr);
                FDCM_HIP(hipMemcpyAsync(fetched.data(), m.rec + r0, nr * sizeof(fdcm_match), hipMemcpyDeviceToHost, st));
                hr = fetched.data();
            }
            FDCM_HIP(hipStreamSynchronize(st));  // (the records are here, and nothing queued still reads the staging)
            unsigned short* hb = (unsigned short*)(h + o_bins);
            std::fill_n(hb, nr * na * Lmax, (unsigned short)0);
            for (size_t rl = 0; rl < nr; ++rl) {
                const int64_t tm = (int64_t)hr[rl].tmpl_idx - m.base;
                if (tm < 0 || tm >= t->T) continue;
                for (size_t e = 0; e < na; ++e) {  // P_e(r): the delta in front of the record's transform
                    RotM Q{};
                    if (rot) Q = rot_matrix(rot->cs[2 * e], rot->cs[2 * e + 1], pivots ? rot->pivots[2 * tm] : 0.f, pivots ? rot->pivots[2 * tm + 1] : 0.f);
                    pose_lines(t, tm, hr[rl].transform, posed, rot ? &Q : nullptr);
                    posed_bins(fm, posed, hb + (rl * na + e) * Lmax);
                }
            }
            FDCM_HIP(hipMemcpyAsync(d + o_bins, hb, nr * na * Lmax * 2, hipMemcpyHostToDevice, st));
        }
        const size_t planes = nr * na, items = planes * (size_t)ppp;
        hipLaunchKernelGGL(k_refine_pose, dim3((unsigned)((planes + 3) / 4)), dim3(256), 0, st, a);
        hipLaunchKernelGGL(score, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_refine_write, dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, st, a);
        FDCM_HIP(hipGetLastError());
    }
    if (!out_on_device) FDCM_HIP(hipMemcpyAsync(out, d + o_out, N * sizeof(fdcm_match), hipMemcpyDeviceToHost, st));
    if (pose_out) FDCM_HIP(hipMemcpyAsync(pose_out, d + o_pose, N * 12, hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipStreamSynchronize(st));  // the call blocks (and the host arrays stay alive until here)
}

}  // namespace fdcm
