// fdcm_coverage.hip -- scene coverage (include/fdcm.h, "Scene coverage"): which edge pixels of a label image the posed
// templates explain, per pose the counts (edges, explained), and the label image without the explained pixels.
//
//   k_scene_coverage    a workgroup per item (pose, strip of rows of its window).  The items are a 1-D list the poses'
//                       prefix sums describe: item e belongs to the pose p with item0[p] <= e < item0[p + 1], found by
//                       bisection on scalar loads, and is strip e - item0[p] of that pose's clipped window.  The workgroup
//                         1. stages the pose's segments in LDS: per line the two map pixels k_line_costs reads (its float
//                            adds and truncation), moved to the label frame, the segment's bounding box widened by the
//                            radius, len2 and the bin; in chunks of kCovLines when the template has more;
//                         2. scans its strip with aligned dword loads, 4 label bytes per lane (the head and tail words of
//                            the image byte by byte), and compacts the edge pixels into a queue in LDS: a ballot and a
//                            popcount per byte position, one LDS atomic per wave for the queue's space;
//                         3. once the queue holds 256 pixels or the strip ends, gives every thread one queued pixel and
//                            walks the segments at a wave-uniform index (an LDS broadcast): bin test, box test, then the
//                            exact squared distance in int64.
//                       Counts: wave-uniform popcounts, one atomicAdd per wave and counter at the item's end.  Residual:
//                       byte stores of 255 into a copy of the labels; the decision reads the labels alone.
//
// Scene selection (include/fdcm.h, "Scene selection") runs the same body, coverage_item, in two more modes, with the residual as
// the claim plane (an edge pixel whose residual byte is 255 is claimed):
//
//   k_select_claim      a workgroup per strip of the pose the round accepted, sel[round], read from device memory: stores 255
//                       at the pixels it explains.
//   k_select_recount    the grid of k_scene_coverage; a workgroup leaves at once unless its pose comes after the accepted one,
//                       survives and has a window that meets the accepted one's: counts the explained pixels not claimed.
//   k_select_decide     a thread per pose: takes the recount, drops the pose when it fails the rule's test, and the smallest
//                       survivor's index becomes sel[round + 1] (atomicMin, one per wave).  Its first form makes S_0.
//
// Both run as well on match records (include/fdcm.h, "Match lists: scene coverage and selection"), whose table is made on the
// device:
//
//   k_matches_table     a wave per record, a lane per line in rounds of 64, as k_matches_verify: poses the template's resident
//                       lines with the record's matrix, decides admissibility and reduces the box (match_frame, fdcm_score.h,
//                       the verify kernel's own pass 1), computes the bins (atanf_glibc + closest_orientation, or the host's),
//                       and writes the record's CoverageLines, its CovPose with x = y = 0 and the window F(r) cut to the image,
//                       its number of strips and its counts' initial value, (0, 0) or (-1, -1).
//   k_strip_scan        one workgroup: item0 = the exclusive prefix sums of the strips, their total and their largest.
//
// Entries without strips stay in the table: pose_of_item returns the last entry whose first item is <= the item, and an entry
// without strips that shares its offset with its successor is never the last such entry.
//
// The pose fit of match records (include/fdcm.h, "Match lists: pose fit") runs the body in a fourth mode and adds a kernel:
//
//   k_fit_moments       the grid of k_scene_coverage on the table of the records' current transforms; a workgroup leaves at once
//                       when its record has stopped.  Every queued pixel walks all the segments for the nearest qualifying
//                       one (exact in int64, carried across chunks) and adds its six moments to that line's int64 accumulators
//                       in LDS (global atomics for the lines beyond the first chunk); the non-zero accumulators are flushed once
//                       per workgroup with 64-bit atomics.  Integer sums: the result does not depend on the schedule.
//   k_fit_step          a thread per record: the normal equations in line order, the damped LDL^T solve, the fold and the
//                       status, all in unfused float64; the transform a step replaces is kept, and put back when the next
//                       table pass finds the stepped one outside the map.
//
// All arithmetic of the decision is integer; the float adds of step 1 are the cost rule's own (-ffp-contract=off as everywhere).
//
// The host side: five drivers made of stages that each exist once.  CovCall is the frame of a call (turn, device, stream, the
// labels and their upload, the residual and the claim plane, a host list's records, the buffers and their poison; the workspace
// layout is stated beside it); DevTable a table on the device, from upload_table (a pose list's HostTable) or make_table (a part
// of a match list); for_items the items in launches of at most kCovMaxGrid; select_stage the selection on a table, counts_down
// the coverage calls' way down, both with a map from table entry to list position.
//   run_scene_coverage    HostTable, upload_table, launch_coverage, counts_down      run_scene_select    .., select_stage
//   run_matches_coverage  records; per part make_table, launch_coverage; counts_down  run_matches_select  .., make_table, select_stage
//   run_matches_fit       records; per part and pass make_table, k_fit_moments through for_items, k_fit_step
#include <algorithm>
#include <cstring>

#include "fdcm_internal.h"
#include "fdcm_score.h"

namespace fdcm {

namespace {

constexpr int kCovThreads = 256;
constexpr int kCovLines = 256;                      // segments per LDS chunk
constexpr int kCovQueue = kCovThreads + 4 * kCovThreads;  // what a scan pass finds at most, on top of an unprocessed rest
constexpr int kCovStripPixels = 2048;               // window pixels per item, about (at least one row)
constexpr long long kCovMaxGrid = 1ll << 30;        // items per launch

struct CovPose {  // one admissible pose with a window: its pair's lines, its translation, its clipped window, rows per strip
    int line0, n;
    int x, y;
    int wx0, wy0, wx1, wy1;
    int rows, pad[3];
};
static_assert(sizeof(CovPose) == 48, "CovPose is 48 bytes");

struct alignas(16) CovSeg {  // one segment in the label frame
    int ax, ay, bx, by;
    int x0, y0, x1, y1;  // its bounding box widened by the radius: outside it no pixel is within the radius
    long long len2;
    int bin, pad;
};
static_assert(sizeof(CovSeg) == 48, "CovSeg is 48 bytes");

// Is P = (px, py) within r of the segment?  include/fdcm.h, "Scene coverage": exact in int64.  P lies in the widened box, the
// segment's ends in the map, so |w|, |d| stay below 2^31; a cross product of 2^31 or more is farther than any radius.
__device__ __forceinline__ bool near_segment(const CovSeg& s, int px, int py, long long r2) {
    const long long dx = (long long)s.bx - s.ax, dy = (long long)s.by - s.ay;
    const long long wx = (long long)px - s.ax, wy = (long long)py - s.ay;
    const long long dot = wx * dx + wy * dy;
    if (dot <= 0) return wx * wx + wy * wy <= r2;
    if (dot >= s.len2) {
        const long long ux = (long long)px - s.bx, uy = (long long)py - s.by;
        return ux * ux + uy * uy <= r2;
    }
    const long long cross = wx * dy - wy * dx;
    if (cross >= (1ll << 31) || cross <= -(1ll << 31)) return false;
    return cross * cross <= r2 * s.len2;
}

enum { kCovCount = 0, kCovClaim = 1, kCovRecount = 2, kCovFit = 3 };

// The pose fit's choice of a line for P (include/fdcm.h, "Match lists: pose fit"): segment i qualifies when P projects
// strictly inside it and lies within the radius of its line; the nearest by cross^2 / len2 wins, compared exactly
// (cross^2 <= 2^10 len2 and len2 <= 2^25, so the products stay below 2^60), ties to the segment seen first.  (wx, wy) = P - A.
struct FitBest {
    int i, wx, wy;
    long long c2, l2;
};
__device__ __forceinline__ void fit_nearest(const CovSeg& s, int i, int px, int py, long long r2, FitBest& b) {
    const long long dx = (long long)s.bx - s.ax, dy = (long long)s.by - s.ay;
    const long long wx = (long long)px - s.ax, wy = (long long)py - s.ay;
    const long long dot = wx * dx + wy * dy;
    if (dot <= 0 || dot >= s.len2) return;  // (also A = B)
    const long long cross = wx * dy - wy * dx;
    if (cross >= (1ll << 31) || cross <= -(1ll << 31)) return;
    const long long c2 = cross * cross;
    if (c2 > r2 * s.len2) return;
    if (b.i < 0 || c2 * b.l2 < b.c2 * s.len2) b = FitBest{i, (int)wx, (int)wy, c2, s.len2};
}
// S1, Sx, Sy, Sxx, Sxy, Syy of the line += the pixel's: LDS for a line of the first chunk, else global
__device__ __forceinline__ void fit_add(const FitBest& b, long long* __restrict__ lds, unsigned long long* __restrict__ out) {
    const long long wx = b.wx, wy = b.wy;
    const long long v[6] = {1, wx, wy, wx * wx, wx * wy, wy * wy};
    if (b.i < kCovLines) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (v[k]) atomicAdd(reinterpret_cast<unsigned long long*>(lds + 6 * b.i + k), (unsigned long long)v[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (v[k]) atomicAdd(out + 6 * (size_t)b.i + k, (unsigned long long)v[k]);
    }
}

// Strip `strip` of the pose P: steps 1 to 3 above.  kCovCount: edges and explained, of this wave (wave-uniform), and 255 into
// the residual, if there is one.  kCovClaim: the stores alone.  kCovRecount: explained counts the pixels the pose explains
// whose residual byte is not 255, and nothing is stored.  The decision reads the labels alone in every mode.  kCovFit: nothing
// is counted or stored but the moments of the pixels, at fit_lds (zeroed by the caller, 6 per line of the first chunk) and fit_out.
template <int kMode>
__device__ __forceinline__ void coverage_item(const uint8_t* __restrict__ labels, int width, int height, int m, float tx, float ty, int bx,
                                              int by, int radius, int tol, const CoverageLine* __restrict__ lines, const CovPose& P,
                                              int strip, uint8_t* __restrict__ residual, int& edges, int& explained,
                                              long long* __restrict__ fit_lds = nullptr, unsigned long long* __restrict__ fit_out = nullptr) {
    __shared__ CovSeg seg[kCovLines];
    __shared__ unsigned queue[kCovQueue];
    __shared__ int q_count;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int r0 = P.wy0 + strip * P.rows, r1 = min(P.wy1 + 1, r0 + P.rows);  // rows [r0, r1) of the image
    const int w = P.wx1 - P.wx0 + 1;
    const float offx = tx + (float)P.x, offy = ty + (float)P.y;  // translate(tmpl, sceneTranslation + translation)
    const long long r2 = (long long)radius * radius;

    auto stage = [&](int c0) {  // segments [c0, c0 + kCovLines) of the pose into LDS
        for (int i = tid; i < min(kCovLines, P.n - c0); i += kCovThreads) {
            const CoverageLine ln = lines[P.line0 + c0 + i];
            CovSeg s;
            s.ax = (int)(ln.x1 + offx) - bx; s.ay = (int)(ln.y1 + offy) - by;
            s.bx = (int)(ln.x2 + offx) - bx; s.by = (int)(ln.y2 + offy) - by;
            s.x0 = min(s.ax, s.bx) - radius; s.x1 = max(s.ax, s.bx) + radius;
            s.y0 = min(s.ay, s.by) - radius; s.y1 = max(s.ay, s.by) + radius;
            const long long dx = (long long)s.bx - s.ax, dy = (long long)s.by - s.ay;
            s.len2 = dx * dx + dy * dy;
            s.bin = ln.bin; s.pad = 0;
            seg[i] = s;
        }
    };
    int resident = 0;  // the chunk in LDS
    if (tid == 0) q_count = 0;
    stage(0);
    __syncthreads();

    // the strip as words of 4 bytes at addresses that are multiples of 4: row y spans the words [wf, wf + nw) of the image's
    // byte string, nw <= nwm; slot s of the strip is word s % nwm of row r0 + s / nwm
    const int al = (int)((size_t)labels & 3);
    const int N = width * height;  // (<= 2^24)
    const int nwm = (w + 2) / 4 + 1;
    const int slots = (r1 - r0) * nwm;
    const int passes = (slots + kCovThreads - 1) / kCovThreads;
    edges = explained = 0;
    for (int pass = 0; pass < passes; ++pass) {
        const int s = pass * kCovThreads + tid;
        unsigned word = 0xffffffffu;
        int valid = 0, y = 0, f0 = 0;
        if (s < slots) {
            y = r0 + s / nwm;
            const int fs = y * width + P.wx0, fe = fs + w - 1;  // the row's bytes of the window
            f0 = ((((fs + al) >> 2) + s % nwm) << 2) - al;      // this word's first byte
            for (int j = 0; j < 4; ++j) valid |= (f0 + j >= fs && f0 + j <= fe) ? 1 << j : 0;
            if (valid) {
                if (f0 >= 0 && f0 + 3 < N) {
                    word = *reinterpret_cast<const unsigned*>(labels + f0);
                } else {  // the first or last word of the image: only the bytes that exist
                    word = 0;
                    for (int j = 0; j < 4; ++j) word |= (unsigned)((valid >> j) & 1 ? labels[f0 + j] : 255) << (8 * j);
                }
            }
        }
        // compaction: per byte position a ballot; the wave takes its space in the queue with one LDS atomic
        unsigned long long bal[4];
        int tot = 0;
        for (int j = 0; j < 4; ++j) {
            bal[j] = __ballot(((valid >> j) & 1) && (int)((word >> (8 * j)) & 255u) < m);
            tot += __popcll(bal[j]);
        }
        if (kMode == kCovCount) edges += tot;
        if (tot) {  // wave-uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(&q_count, tot);
            base = __builtin_amdgcn_readfirstlane(base);
            const unsigned long long below = (1ull << lane) - 1ull;
            for (int j = 0; j < 4; ++j) {
                if ((bal[j] >> lane) & 1ull) {
                    const int x = f0 + j - y * width;
                    queue[base + __popcll(bal[j] & below)] = (unsigned)x | ((unsigned)y << 12) | (((word >> (8 * j)) & 255u) << 24);
                }
                base += __popcll(bal[j]);
            }
        }
        __syncthreads();
        const int cnt = q_count;
        __syncthreads();  // (everyone has read the count before anyone changes it)
        const bool last = pass == passes - 1;
        const int rounds = last ? (cnt + kCovThreads - 1) / kCovThreads : cnt / kCovThreads;
        for (int r = 0; r < rounds; ++r) {
            const int e = r * kCovThreads + tid;
            const bool have = e < cnt;
            const unsigned q = have ? queue[e] : 0u;
            const int px = (int)(q & 4095u), py = (int)((q >> 12) & 4095u), lab = (int)(q >> 24);
            bool hit = false;
            FitBest best{-1, 0, 0, 0, 1};
            for (int c0 = 0; c0 < P.n; c0 += kCovLines) {
                if (c0 != resident) {  // (templates of more than one chunk only)
                    __syncthreads();
                    stage(c0);
                    __syncthreads();
                    resident = c0;
                }
                const int nc = min(kCovLines, P.n - c0);
                for (int i = 0; i < nc; ++i) {
                    const CovSeg sg = seg[i];  // wave-uniform index: a broadcast
                    int d = lab - sg.bin;
                    d = d < 0 ? -d : d;
                    d = min(d, m - d);
                    if (kMode == kCovFit) {
                        if (have && d <= tol && px >= sg.x0 && px <= sg.x1 && py >= sg.y0 && py <= sg.y1) fit_nearest(sg, c0 + i, px, py, r2, best);
                    } else if (have && !hit && d <= tol && px >= sg.x0 && px <= sg.x1 && py >= sg.y0 && py <= sg.y1) hit = near_segment(sg, px, py, r2);
                }
            }
            if (kMode == kCovFit) {
                if (best.i >= 0) fit_add(best, fit_lds, fit_out);
                continue;
            }
            if (kMode == kCovRecount) hit = hit && residual[py * width + px] != 255;
            if (kMode != kCovClaim) explained += __popcll(__ballot(hit));
            if (kMode != kCovRecount && hit && residual) residual[py * width + px] = 255;
        }
        if (!last && rounds > 0) {  // the rest moves to the queue's front
            const int rest = cnt - rounds * kCovThreads;
            const unsigned v = tid < rest ? queue[rounds * kCovThreads + tid] : 0u;
            __syncthreads();
            if (tid < rest) queue[tid] = v;
            if (tid == 0) q_count = rest;
            __syncthreads();
        }
    }
}

// the last pose whose first item is <= item (item0[0] = 0 <= item < item0[n_poses])
__device__ __forceinline__ int pose_of_item(const long long* __restrict__ item0, int n_poses, long long item) {
    int lo = 0, hi = n_poses - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (item0[mid] <= item) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(kCovThreads) k_scene_coverage(const uint8_t* __restrict__ labels, int width, int height, int m, float tx,
                                                                float ty, int bx, int by, int radius, int tol,
                                                                const CoverageLine* __restrict__ lines, const CovPose* __restrict__ poses,
                                                                const long long* __restrict__ item0, int n_poses, long long item_base,
                                                                int* __restrict__ counts, uint8_t* __restrict__ residual) {
    const long long item = item_base + (long long)blockIdx.x;
    const int lo = pose_of_item(item0, n_poses, item);
    const CovPose P = poses[lo];
    int edges, explained;
    coverage_item<kCovCount>(labels, width, height, m, tx, ty, bx, by, radius, tol, lines, P, (int)(item - item0[lo]), residual, edges,
                             explained);
    if ((threadIdx.x & 63) == 0) {
        if (edges) atomicAdd(&counts[2 * lo], edges);
        if (explained) atomicAdd(&counts[2 * lo + 1], explained);
    }
}

// ---------------------------------------------------------------------------------------------- scene selection
// The rule of include/fdcm.h, "Scene selection", in rounds.  Poses are the entries of the pose table, in
// list order.  sel[r] is the pose round r accepts, kSelNone or more when the list has ended: every kernel of a round reads it
// and leaves when it has.  alive[i]: i is in S_0 and has not failed its test yet.  cur[i]: |E_i \ C| as last counted, exact for
// every i alive, because only an accepted pose whose window meets i's can change it.  fresh[i]: the recount's counter, 0
// between rounds.  Nothing waits on another workgroup: claim, recount and decide are three launches.
constexpr int kSelNone = 0x7f7f7f7f;  // (what hipMemsetAsync writes with 0x7f: above any pose index)

struct SelArgs {  // k_scene_coverage's arguments, the counters aside
    const uint8_t* labels;
    int width, height, m;
    float tx, ty;
    int bx, by, radius, tol;
    const CoverageLine* lines;
    const CovPose* poses;
    const long long* item0;
    int n_poses;
};

__device__ __forceinline__ bool windows_meet(const CovPose& a, const CovPose& b) {
    return a.wx0 <= b.wx1 && b.wx0 <= a.wx1 && a.wy0 <= b.wy1 && b.wy0 <= a.wy1;
}

// Grid: the largest number of strips a pose has.  Stores 255 into the claim plane at every pixel of E_d, d = sel[round], and
// writes the new count d was accepted with.
__global__ void __launch_bounds__(kCovThreads) k_select_claim(SelArgs a, const int* __restrict__ sel, int round, const int* __restrict__ cur,
                                                              int* __restrict__ sel_new, uint8_t* __restrict__ plane) {
    const int d = sel[round];
    if (d >= a.n_poses) return;
    const long long i0 = a.item0[d];
    if ((long long)blockIdx.x >= a.item0[d + 1] - i0) return;
    const CovPose P = a.poses[d];
    if (blockIdx.x == 0 && threadIdx.x == 0) sel_new[round] = cur[d];
    int edges, explained;
    coverage_item<kCovClaim>(a.labels, a.width, a.height, a.m, a.tx, a.ty, a.bx, a.by, a.radius, a.tol, a.lines, P, (int)blockIdx.x, plane,
                             edges, explained);
}

// Grid: k_scene_coverage's.  fresh[i] += the pixels of the item that pose i explains and nobody has claimed, for the poses i
// after d = sel[round] that are alive and whose window meets d's.
__global__ void __launch_bounds__(kCovThreads) k_select_recount(SelArgs a, long long item_base, const int* __restrict__ sel, int round,
                                                                const uint8_t* __restrict__ alive, int* __restrict__ fresh,
                                                                uint8_t* __restrict__ plane) {
    const int d = sel[round];
    if (d >= a.n_poses) return;
    const long long item = item_base + (long long)blockIdx.x;
    if (item < a.item0[d + 1]) return;  // a pose at or before d
    const int i = pose_of_item(a.item0, a.n_poses, item);
    if (!alive[i]) return;
    const CovPose P = a.poses[i], D = a.poses[d];
    if (!windows_meet(P, D)) return;
    int edges, explained;
    coverage_item<kCovRecount>(a.labels, a.width, a.height, a.m, a.tx, a.ty, a.bx, a.by, a.radius, a.tol, a.lines, P, (int)(item - a.item0[i]),
                               plane, edges, explained);
    if ((threadIdx.x & 63) == 0 && explained) atomicAdd(&fresh[i], explained);
}

// Grid: a thread per pose.  round < 0: S_0 from the counts (edges, explained), cur = explained; with C empty every pose of S_0
// passes its test.  round >= 0: the poses the recount visited take their count, leave fresh at 0, and fail or stay.  The
// smallest pose alive after d goes to *next, which holds kSelNone: one atomicMin per wave.
__global__ void __launch_bounds__(256) k_select_decide(const CovPose* __restrict__ poses, int n_poses, const int* __restrict__ counts,
                                                       const int* __restrict__ sel, int round, fdcm_select_params par,
                                                       uint8_t* __restrict__ alive, int* __restrict__ fresh, int* __restrict__ cur,
                                                       int* __restrict__ next) {
    int d = -1;
    if (round >= 0) {
        d = sel[round];
        if (d >= n_poses) return;
    }
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    bool live = false;
    if (i < n_poses && i > d) {
        const long long explained = counts[2 * i + 1];
        if (round < 0) {
            live = explained >= par.min_pixels && 1000ll * explained >= (long long)par.min_coverage_permille * counts[2 * i];
            cur[i] = (int)explained;
            alive[i] = live;
        } else if (alive[i]) {
            live = true;
            if (windows_meet(poses[i], poses[d])) {
                const long long c = fresh[i];
                fresh[i] = 0;
                cur[i] = (int)c;
                live = c >= par.min_pixels && 1000ll * c >= (long long)par.min_new_permille * explained;
                if (!live) alive[i] = 0;
            }
        }
    }
    const unsigned long long any = __ballot(live);
    if (any && (threadIdx.x & 63) == 0) atomicMin(next, i + (int)__builtin_ctzll(any));
}

// ---------------------------------------------------------------------------------------------- the table of a match list
struct TableArgs {
    const float4* tlines;  // the set's resident lines and offsets
    const long long* toff;
    const float* keys;            // the map's m orientation keys
    const unsigned short* bins;   // [record][Lmax] bins from the host libm, or null
    const fdcm_match* rec;        // the part's records
    int n, base, T, Lmax, m, W, H;
    float tx, ty;
    int margin, width, height;
    CoverageLine* lines;  // [record][Lmax]
    CovPose* poses;
    int* strips;
    int* counts;  // [record][2]
};

__global__ void __launch_bounds__(256) k_matches_table(const TableArgs a) {
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (j >= a.n) return;  // wave-uniform
    const fdcm_match R = a.rec[j];
    const long long t = (long long)R.tmpl_idx - (long long)a.base;
    CovPose P{j * a.Lmax, 0, 0, 0, 0, 0, -1, -1, 1, {0, 0, 0}};
    int strips = 0, count = -1;  // not valid or not admissible: (-1, -1), no strips
    if (t >= 0 && t < a.T) {
        const long long l0 = a.toff[t];
        const int nl = (int)(a.toff[t + 1] - l0);
        const MatchTransform M{R.transform[0], R.transform[1], R.transform[2], R.transform[3], R.transform[4], R.transform[5]};
        const float offx = a.tx + 0.f, offy = a.ty + 0.f;  // sceneTranslation + translation, the translation (0, 0)
        const MatchFrame F = match_frame(a.tlines, l0, nl, M, offx, offy, a.W, a.H, a.margin, lane);
        if (F.adm) {  // wave-uniform
            count = 0;
            const int x0 = max(0, F.box.x), y0 = max(0, F.box.y), x1 = min(a.width - 1, F.box.z), y1 = min(a.height - 1, F.box.w);
            if (x0 <= x1 && y0 <= y1) {  // (an empty window: (0, 0), and nobody reads its lines)
                for (int i = lane; i < nl; i += 64) {
                    const float4 p = match_pose_line(M, a.tlines[l0 + i]);
                    int bin;
                    if (a.bins) {
                        bin = (int)a.bins[(size_t)j * (size_t)a.Lmax + i];
                    } else {
                        const float angle = atanf_glibc((p.w - p.y) / (p.z - p.x));  // getAngle, math.h:295-299
                        bin = closest_orientation(a.keys, a.m, angle);               // dt3cpu.cpp:144-148
                    }
                    a.lines[(size_t)P.line0 + i] = CoverageLine{p.x, p.y, p.z, p.w, bin};
                }
                P.n = nl;
                P.wx0 = x0; P.wy0 = y0; P.wx1 = x1; P.wy1 = y1;
                P.rows = max(1, kCovStripPixels / (x1 - x0 + 1));
                strips = (y1 - y0 + P.rows) / P.rows;
            }
        }
    }
    if (lane == 0) {
        a.poses[j] = P;
        a.strips[j] = strips;
        a.counts[2 * j] = a.counts[2 * j + 1] = count;
    }
}

// One workgroup: item0[i] = strips[0] + .. + strips[i - 1] for i <= n, out[0] = item0[n], out[1] = the largest of the strips.
__global__ void __launch_bounds__(1024) k_strip_scan(const int* __restrict__ strips, int n, long long* __restrict__ item0,
                                                     long long* __restrict__ out) {
    __shared__ int wsum[16], wmax[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    int mx = 0;
    for (int base = 0; base < n; base += 1024) {  // uniform
        const int i = base + tid;
        const int v = i < n ? strips[i] : 0;  // (<= 4096 each: a wave's sum stays an int)
        int inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(inc, d);
            if (lane >= d) inc += u;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long long before = 0, all = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (i < n) item0[i] = carry + before + (long long)(inc - v);
        carry += all;
        mx = max(mx, v);
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d));
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) mx = max(mx, wmax[w]);
        item0[n] = carry;
        out[0] = carry;
        out[1] = mx;
    }
}

// ---------------------------------------------------------------------------------------------- the pose fit of a match list
// include/fdcm.h, "Match lists: pose fit".  info[record] = (status, steps, fit pixels at the first pass, at the last pass); a
// record still stepping holds kFitActive as its status (what hipMemsetAsync writes with 0x7f).
constexpr int kFitActive = 0x7f7f7f7f;

// Grid: k_scene_coverage's, on the table of the current transforms.  mom: [record][Lmax][6], zero before the launch.
__global__ void __launch_bounds__(kCovThreads) k_fit_moments(const uint8_t* __restrict__ labels, int width, int height, int m, float tx,
                                                             float ty, int bx, int by, int radius, int tol,
                                                             const CoverageLine* __restrict__ lines, const CovPose* __restrict__ poses,
                                                             const long long* __restrict__ item0, int n_poses, long long item_base,
                                                             const int* __restrict__ info, unsigned long long* __restrict__ mom, int Lmax) {
    __shared__ long long acc[kCovLines * 6];
    const long long item = item_base + (long long)blockIdx.x;
    const int lo = pose_of_item(item0, n_poses, item);
    if (info[4 * lo] != kFitActive) return;  // (uniform: the record has stopped)
    const CovPose P = poses[lo];
    const int na = min(P.n, kCovLines) * 6;
    for (int e = (int)threadIdx.x; e < na; e += kCovThreads) acc[e] = 0;  // (coverage_item's first barrier is before its first pixel)
    unsigned long long* out = mom + (size_t)lo * (size_t)Lmax * 6;
    int edges, explained;
    coverage_item<kCovFit>(labels, width, height, m, tx, ty, bx, by, radius, tol, lines, P, (int)(item - item0[lo]), nullptr, edges, explained,
                           acc, out);
    __syncthreads();
    for (int e = (int)threadIdx.x; e < na; e += kCovThreads)
        if (acc[e]) atomicAdd(out + e, (unsigned long long)acc[e]);
}

struct FitArgs {
    const CoverageLine* lines;  // the part's table, at the current transforms
    const CovPose* poses;
    const int* counts;          // [record][2]: -1 where the current transform is not admissible
    const long long* mom;       // [record][Lmax][6]
    fdcm_match* cur;            // the part's records
    float* prev;                // [record][6]: the transform the last step replaced
    int* info;                  // [record][4]
    float* rms;                 // [record][2]
    int n, Lmax, pass;
    fdcm_fit_params par;
    float tx, ty;
    int bx, by;
};

// S(p, q) of the section: the sum over a line's pixels of p(u) q(u) for affine p, q with coefficients (f0, fx, fy), from the
// line's moments, left to right.
__device__ __forceinline__ double fit_S(const double* p, const double* q, const double* S) {
    return p[0] * q[0] * S[0] + (p[0] * q[1] + p[1] * q[0]) * S[1] + (p[0] * q[2] + p[2] * q[0]) * S[2] + p[1] * q[1] * S[3] +
           (p[1] * q[2] + p[2] * q[1]) * S[4] + p[2] * q[2] * S[5];
}
__device__ __forceinline__ bool fit_finite(double v) { return fabs(v) < __builtin_inf(); }  // false for a NaN

// Grid: a thread per record of the part.  Pass `pass` of 0 .. iterations: the last one only measures.
__global__ void __launch_bounds__(256) k_fit_step(const FitArgs a) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= a.n) return;
    int* info = a.info + 4 * (size_t)j;
    if (a.pass == 0) info[1] = info[2] = info[3] = 0;
    else if (info[0] != kFitActive) return;
    float* M = a.cur[j].transform;
    if (a.counts[2 * j] < 0) {
        if (a.pass == 0) {  // not valid or not admissible: untouched
            info[0] = -1;
            a.rms[2 * j] = a.rms[2 * j + 1] = __int_as_float(0x7fc00000);
        } else {  // the step left the map: it is not taken, and the last pass's figures stand
            for (int k = 0; k < 6; ++k) M[k] = a.prev[6 * (size_t)j + k];
            info[0] = 4;
            info[1] -= 1;
        }
        return;
    }
    const CovPose P = a.poses[j];
    const CoverageLine* lines = a.lines + P.line0;
    const long long* mom = a.mom + (size_t)j * (size_t)a.Lmax * 6;
    const float offx = a.tx + 0.f, offy = a.ty + 0.f;  // k_matches_table's, coverage_item's
    int mnx = 0x7fffffff, mny = 0x7fffffff, mxx = -0x7fffffff, mxy = -0x7fffffff;
    for (int i = 0; i < P.n; ++i) {
        const CoverageLine ln = lines[i];
        const int ax = (int)(ln.x1 + offx) - a.bx, ay = (int)(ln.y1 + offy) - a.by;
        const int ex = (int)(ln.x2 + offx) - a.bx, ey = (int)(ln.y2 + offy) - a.by;
        mnx = min(mnx, min(ax, ex)); mxx = max(mxx, max(ax, ex));
        mny = min(mny, min(ay, ey)); mxy = max(mxy, max(ay, ey));
    }
    const double cx = (double)((mnx + mxx) >> 1), cy = (double)((mny + mxy) >> 1);  // the pivot (unused without lines)
    double N00 = 0, N01 = 0, N02 = 0, N11 = 0, N12 = 0, N22 = 0, v0 = 0, v1 = 0, v2 = 0, See = 0;
    long long n = 0;
    for (int i = 0; i < P.n; ++i) {
        const long long* Si = mom + 6 * (size_t)i;
        if (Si[0] == 0) continue;
        const CoverageLine ln = lines[i];
        const float fax = ln.x1 + offx, fay = ln.y1 + offy, fbx = ln.x2 + offx, fby = ln.y2 + offy;
        const double pax = (double)fax - (double)a.bx, pay = (double)fay - (double)a.by;
        const double pbx = (double)fbx - (double)a.bx, pby = (double)fby - (double)a.by;
        const double tx = pbx - pax, ty = pby - pay;
        const double L = sqrt(tx * tx + ty * ty);
        if (L == 0.0) continue;
        const double nx = ty / L, ny = -tx / L;
        const double ox = (double)((int)fax - a.bx), oy = (double)((int)fay - a.by);
        const double e0 = nx * (ox - pax) + ny * (oy - pay);
        const double g0 = ny * (ox - cx) - nx * (oy - cy);
        const double fa[3] = {nx, 0.0, 0.0}, fb[3] = {ny, 0.0, 0.0}, fg[3] = {g0, ny, -nx}, fe[3] = {e0, nx, ny};
        const double S[6] = {(double)Si[0], (double)Si[1], (double)Si[2], (double)Si[3], (double)Si[4], (double)Si[5]};
        N00 += fit_S(fa, fa, S); N01 += fit_S(fa, fb, S); N02 += fit_S(fa, fg, S);
        N11 += fit_S(fb, fb, S); N12 += fit_S(fb, fg, S); N22 += fit_S(fg, fg, S);
        v0 += fit_S(fa, fe, S); v1 += fit_S(fb, fe, S); v2 += fit_S(fg, fe, S);
        See += fit_S(fe, fe, S);
        n += Si[0];
    }
    const float rms = n > 0 ? (float)sqrt(fmax(See, 0.0) / (double)n) : __int_as_float(0x7fc00000);
    if (a.pass == 0) {
        info[2] = (int)n;
        a.rms[2 * j] = rms;
    }
    info[3] = (int)n;
    a.rms[2 * j + 1] = rms;
    if (a.pass == a.par.iterations) { info[0] = 0; return; }
    if (n < a.par.min_pixels) { info[0] = 1; return; }
    const double tr = N00 + N11;
    N00 += a.par.damping * tr; N11 += a.par.damping * tr; N22 += a.par.damping * N22;
    const double d0 = N00, l10 = N01 / d0, l20 = N02 / d0;
    const double d1 = N11 - l10 * N01, m21 = N12 - l20 * N01, l21 = m21 / d1;
    const double d2 = N22 - l20 * N02 - l21 * m21;
    if (!(d0 > 0.0 && d1 > 0.0 && d2 > 0.0)) { info[0] = 2; return; }
    const double y0 = v0, y1 = v1 - l10 * y0, y2 = v2 - l20 * y0 - l21 * y1;
    const double x2 = y2 / d2, x1 = y1 / d1 - l21 * x2, x0 = y0 / d0 - l10 * x1 - l20 * x2;
    if (!(fit_finite(x0) && fit_finite(x1) && fit_finite(x2))) { info[0] = 2; return; }
    if (fabs(x0) > a.par.max_shift || fabs(x1) > a.par.max_shift || fabs(x2) > a.par.max_angle) { info[0] = 3; return; }
    const double h = x2 / 2.0, q = h * h, cc = (1.0 - q) / (1.0 + q), ss = (h + h) / (1.0 + q);
    const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5];
    const float r[6] = {(float)(cc * m0 - ss * m3), (float)(cc * m1 - ss * m4), (float)(((cc * (m2 - cx) - ss * (m5 - cy)) + cx) + x0),
                        (float)(ss * m0 + cc * m3), (float)(ss * m1 + cc * m4), (float)(((ss * (m2 - cx) + cc * (m5 - cy)) + cy) + x1)};
    bool fin = true;
    for (int k = 0; k < 6; ++k) fin = fin && fabsf(r[k]) < __builtin_inff();
    if (!fin) { info[0] = 2; return; }
    const bool still = x0 == 0.0 && x1 == 0.0 && x2 == 0.0;  // the transform stays byte for byte
    for (int k = 0; k < 6; ++k) {
        a.prev[6 * (size_t)j + k] = M[k];
        if (!still) M[k] = r[k];
    }
    info[1] += 1;
}

// ---------------------------------------------------------------------------------------------- the host side
// The workspace of the coverage calls, stated once.  The buffers are the handle's own (coverage, coverage_stage), not the
// exhaustive calls' shared workspace; every block is a multiple of 256 bytes, and a block in brackets is there for some calls only:
//
//   device    [records: a host list; the fit's own copy of any list, with replaced transforms | info | rms behind it]
//             | the table: lines | poses | item offsets (HostTable, made on the host), or
//                          [host bins] | lines | poses | strips | item offsets | total and largest (TableLayout, made on the device)
//             | counters, (edges, explained) per entry
//             | [selection: sel | sel_new | fresh | cur | alive (SelLayout)]   [fit: the part's moments]
//             | [labels: host callers] | [the output plane: the residual of a host caller, the claim plane]
//   staging   what goes up -- the host-made table, or [host records] | [a part's host bins] -- and then, the upload done, what
//             comes down: the counters (with sel and sel_new), or the fit's records | info | rms
size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// The frame of a call: the handle's turn, its device and stream, the label image with its frame (bx, by) and the call's
// parameters.  It owns the labels -- the one place where a host caller's image goes up -- and the two ways a call treats its
// output plane: the coverage calls' residual (optional, a copy of the labels where the labels are) and the selection calls'
// claim plane (always there, the caller's own buffer when that is on the device).
struct CovCall {
    fdcm_featuremap* const fm;
    const uint8_t* const image;
    const int width, height;
    const bool on_device;
    const int bx, by;
    const fdcm_coverage_params& par;
    const size_t npix;
    std::lock_guard<std::mutex> turn;
    hipStream_t st = nullptr;
    char *d = nullptr, *h = nullptr;    // the two buffers, after reserve
    const uint8_t* d_labels = nullptr;  // after labels

    CovCall(fdcm_featuremap* fm, const uint8_t* image, int width, int height, bool on_device, int bx, int by, const fdcm_coverage_params& par)
        : fm(fm), image(image), width(width), height(height), on_device(on_device), bx(bx), by(by), par(par),
          npix((size_t)width * (size_t)height), turn(fm->seam_mutex) {
        FDCM_HIP(hipSetDevice(fm->device));
        ensure_stream(fm);
        st = fm->stream;
    }
    // no entries, an empty set or an empty map: nothing is explained
    bool nothing(int64_t n, const fdcm_templates* t) const { return n == 0 || t->T == 0 || fm->W == 0 || fm->H == 0 || fm->m == 0; }
    // what the last blocks of the device layout take
    size_t labels_bytes() const { return on_device ? 0 : al256(npix); }
    size_t residual_bytes(const uint8_t* residual) const { return on_device || !residual ? 0 : al256(npix); }
    size_t claim_bytes(const uint8_t* residual) const { return on_device && residual ? 0 : al256(npix); }
    // FDCM_POISON (fdcm_internal.h, "the tests' switches"): the buffers hold the word at the head of a call, before anything goes up
    void reserve(size_t device, size_t staging) {
        fm->coverage.reserve(device);
        fm->coverage_stage.reserve(staging);
        if (test_switches().poison) {
            FDCM_HIP(hipStreamSynchronize(st));  // (nothing queued still reads the staging)
            poison_fill(fm->coverage, st, FDCM_FILL_COVERAGE);
            poison_fill(fm->coverage_stage, FDCM_FILL_COVERAGE_STAGE);
        }
        d = (char*)fm->coverage.p;
        h = (char*)fm->coverage_stage.p;
    }
    void labels(size_t o_lab) {
        d_labels = image;
        if (on_device) return;
        FDCM_HIP(hipMemcpyAsync(d + o_lab, image, npix, hipMemcpyHostToDevice, st));
        d_labels = (const uint8_t*)(d + o_lab);
    }
    uint8_t* plane_copy(uint8_t* plane) {
        if (plane) FDCM_HIP(hipMemcpyAsync(plane, d_labels, npix, hipMemcpyDeviceToDevice, st));
        return plane;
    }
    uint8_t* residual_plane(uint8_t* residual, size_t o_res) { return plane_copy(on_device || !residual ? residual : (uint8_t*)(d + o_res)); }
    uint8_t* claim_plane(uint8_t* residual, size_t o_plane) { return plane_copy(on_device && residual ? residual : (uint8_t*)(d + o_plane)); }
    void plane_down(uint8_t* residual, const uint8_t* plane) {  // queued; the caller waits
        if (residual && !on_device) FDCM_HIP(hipMemcpyAsync(residual, plane, npix, hipMemcpyDeviceToHost, st));
    }
    // no window holds a pixel: the residual is a copy
    void copy_labels(uint8_t* residual) {
        if (residual && on_device) {
            FDCM_HIP(hipMemcpyAsync(residual, image, npix, hipMemcpyDeviceToDevice, st));
            FDCM_HIP(hipStreamSynchronize(st));
        } else if (residual) {
            std::memcpy(residual, image, npix);
        }
    }
    // the records of a host list go up through the staging's head to the device buffer's; a device list stays where it is
    static size_t records_bytes(const MatchList& m) { return m.on_device ? 0 : al256((size_t)m.n * sizeof(fdcm_match)); }
    const fdcm_match* records(const MatchList& m) {
        if (m.on_device) return m.rec;
        std::memcpy(h, m.rec, (size_t)m.n * sizeof(fdcm_match));
        FDCM_HIP(hipMemcpyAsync(d, h, (size_t)m.n * sizeof(fdcm_match), hipMemcpyHostToDevice, st));
        return (const fdcm_match*)d;
    }
};

// A table on the device: the lines, one CovPose per entry, the items' prefix sums, the entries, the items (strips) in all and
// of the entry with most.  Two producers: upload_table (a pose list's, made on the host) and make_table (a part of a match list).
struct DevTable {
    const CoverageLine* lines;
    const CovPose* poses;
    const long long* item0;
    int n;
    long long items, most;
    SelArgs args(const CovCall& c) const {
        return SelArgs{c.d_labels, c.width, c.height, (int)c.fm->m, c.fm->tx, c.fm->ty, c.bx, c.by, (int)c.par.radius, (int)c.par.bin_tolerance,
                       lines, poses, item0, n};
    }
};

// The items in launches of at most kCovMaxGrid: launch(grid, first item).
template <class Launch>
void for_items(long long items, Launch launch) {
    for (long long base = 0; base < items; base += kCovMaxGrid) {
        launch((unsigned)std::min(kCovMaxGrid, items - base), base);
        FDCM_HIP(hipGetLastError());
    }
}

void launch_coverage(hipStream_t st, const SelArgs& a, long long items, int* d_cnt, uint8_t* d_res) {
    for_items(items, [&](unsigned grid, long long base) {
        hipLaunchKernelGGL(k_scene_coverage, dim3(grid), dim3(kCovThreads), 0, st, a.labels, a.width, a.height, a.m, a.tx, a.ty, a.bx, a.by,
                           a.radius, a.tol, a.lines, a.poses, a.item0, a.n_poses, base, d_cnt, d_res);
    });
}

// What both calls make of a checked pose list: the pairs, one CovPose per admissible pose with a window that holds a pixel, in
// list order, the items' prefix sums and, per entry, its pose.  adm[q]: pose q is admissible.  On the device the table is
// lines | poses | item offsets from the buffer's head, and `end` is where the counters go.
struct HostTable {
    CoveragePairs W;
    std::vector<CovPose> tab;
    std::vector<long long> item0{0};
    std::vector<int64_t> pose_of;
    std::vector<char> adm;
    long long most = 1;
    size_t o_tab = 0, o_item = 0, end = 0;
    void make(const fdcm_featuremap* fm, int width, int height, const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses,
              int64_t n, int margin) {
        coverage_pairs(fm, t, rot, poses, n, margin, W);
        const int nr = rot ? rot->n : 1;
        adm.assign((size_t)n, 0);
        for (int64_t q = 0; q < n; ++q) {
            const int32_t* p = poses + 4 * q;
            const size_t u = W.find((int64_t)p[0] * nr + p[1]);
            const int32_t* a = &W.adm[5 * u];
            adm[q] = a[0] && p[2] >= a[1] && p[2] <= a[2] && p[3] >= a[3] && p[3] <= a[4];
            if (!adm[q]) continue;
            const int32_t* f = &W.foot[4 * u];  // (|f| <= 2^25, |p| < 2^24)
            const int x0 = std::max(0, f[0] + p[2]), y0 = std::max(0, f[1] + p[3]);
            const int x1 = std::min(width - 1, f[2] + p[2]), y1 = std::min(height - 1, f[3] + p[3]);
            if (x0 > x1 || y0 > y1) continue;  // an empty window: (0, 0)
            const int rows = std::max(1, kCovStripPixels / (x1 - x0 + 1));
            const long long strips = (y1 - y0 + rows) / rows;
            tab.push_back(CovPose{W.line0[u], W.nl[u], p[2], p[3], x0, y0, x1, y1, rows, {0, 0, 0}});
            pose_of.push_back(q);
            item0.push_back(item0.back() + strips);
            most = std::max(most, strips);
        }
        o_tab = al256(W.lines.size() * sizeof(CoverageLine));
        o_item = o_tab + al256(tab.size() * sizeof(CovPose));
        end = o_item + al256(item0.size() * sizeof(long long));
    }
};

// One upload of lines, poses and item offsets through the staging, and the counters behind them zeroed.
DevTable upload_table(CovCall& c, const HostTable& T) {
    std::memcpy(c.h, T.W.lines.data(), T.W.lines.size() * sizeof(CoverageLine));
    std::memcpy(c.h + T.o_tab, T.tab.data(), T.tab.size() * sizeof(CovPose));
    std::memcpy(c.h + T.o_item, T.item0.data(), T.item0.size() * sizeof(long long));
    FDCM_HIP(hipMemcpyAsync(c.d, c.h, T.end, hipMemcpyHostToDevice, c.st));
    FDCM_HIP(hipMemsetAsync(c.d + T.end, 0, T.tab.size() * 2 * sizeof(int32_t), c.st));
    return DevTable{(const CoverageLine*)c.d, (const CovPose*)(c.d + T.o_tab), (const long long*)(c.d + T.o_item), (int)T.tab.size(),
                    T.item0.back(), T.most};
}

// The counters of `entries` table entries come down through the staging (free again: the copy is behind the upload on the
// stream), with a host caller's residual, and go to the list positions pose_of gives (null: the entry's own).
void counts_down(CovCall& c, const int* d_cnt, size_t entries, const int64_t* pose_of, int32_t* counts, uint8_t* residual, const uint8_t* d_res) {
    const int32_t* h_cnt = (const int32_t*)c.h;
    FDCM_HIP(hipMemcpyAsync(c.h, d_cnt, entries * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
    c.plane_down(residual, d_res);
    FDCM_HIP(hipStreamSynchronize(c.st));
    for (size_t i = 0; i < entries; ++i) {
        const size_t q = pose_of ? (size_t)pose_of[i] : i;
        counts[2 * q] = h_cnt[2 * i];
        counts[2 * q + 1] = h_cnt[2 * i + 1];
    }
}

// ---- the selection stage
// Rounds are queued kSelBatch at a time, as nms_rounds queues its own: after a batch the host reads the pose the next round
// would accept and stops when there is none, so no round costs a host round trip, and the launches queued behind the list's
// end leave at their first load.
constexpr int kSelBatch = 64;

// The selection's arrays, from the table's counters on: counters | sel | sel_new (what comes down) | fresh | cur | alive
struct SelLayout {
    size_t o_cnt, o_sel, o_new, o_fresh, o_cur, o_alive, end;
    SelLayout(size_t at, size_t entries, size_t ms)
        : o_cnt(at), o_sel(o_cnt + al256(entries * 2 * sizeof(int32_t))), o_new(o_sel + al256(ms * sizeof(int32_t))),
          o_fresh(o_new + al256(ms * sizeof(int32_t))), o_cur(o_fresh + al256(entries * sizeof(int32_t))),
          o_alive(o_cur + al256(entries * sizeof(int32_t))), end(o_alive + al256(entries)) {}
    size_t down() const { return o_fresh - o_cnt; }
};

// The launches of the rule on a table that is on the device with its counters (zero, or what k_matches_table left), sel at
// kSelNone and fresh at 0: one k_scene_coverage launch for the counts, k_select_decide's first form for S_0, and per round
// claim, recount, decide.
void select_rounds(hipStream_t st, const SelArgs& a, const DevTable& T, const fdcm_select_params& sel, char* d, const SelLayout& S,
                   uint8_t* plane) {
    int *d_cnt = (int*)(d + S.o_cnt), *d_sel = (int*)(d + S.o_sel), *d_new = (int*)(d + S.o_new), *d_fresh = (int*)(d + S.o_fresh),
        *d_cur = (int*)(d + S.o_cur);
    uint8_t* d_alive = (uint8_t*)(d + S.o_alive);
    const unsigned pose_wgs = (unsigned)(((size_t)a.n_poses + 255) / 256);
    launch_coverage(st, a, T.items, d_cnt, nullptr);
    hipLaunchKernelGGL(k_select_decide, dim3(pose_wgs), dim3(256), 0, st, a.poses, a.n_poses, d_cnt, d_sel, -1, sel, d_alive, d_fresh, d_cur,
                       d_sel);
    FDCM_HIP(hipGetLastError());
    const int rounds = (int)std::min((size_t)sel.max_selected, (size_t)a.n_poses);  // a round accepts a pose of the table or finds the list ended
    for (int r = 0; r < rounds;) {
        for (const int r1 = std::min(rounds, r + kSelBatch); r < r1; ++r) {
            hipLaunchKernelGGL(k_select_claim, dim3((unsigned)T.most), dim3(kCovThreads), 0, st, a, d_sel, r, d_cur, d_new, plane);
            FDCM_HIP(hipGetLastError());
            if (r + 1 == rounds) continue;  // the last pose the call may accept: nobody asks who is next
            for_items(T.items, [&](unsigned grid, long long base) {
                hipLaunchKernelGGL(k_select_recount, dim3(grid), dim3(kCovThreads), 0, st, a, base, d_sel, r, d_alive, d_fresh, plane);
            });
            hipLaunchKernelGGL(k_select_decide, dim3(pose_wgs), dim3(256), 0, st, a.poses, a.n_poses, d_cnt, d_sel, r, sel, d_alive, d_fresh,
                               d_cur, d_sel + r + 1);
            FDCM_HIP(hipGetLastError());
        }
        if (r == rounds) break;
        int next = kSelNone;  // the pose round r would accept
        FDCM_HIP(hipMemcpyAsync(&next, d_sel + r, sizeof(int), hipMemcpyDeviceToHost, st));
        FDCM_HIP(hipStreamSynchronize(st));
        if (next >= a.n_poses) break;
    }
}

// The selection on a table that is on the device, its counters at S.o_cnt: sel at kSelNone, fresh at 0, the claim plane a copy
// of the labels, the rounds (none when no entry has a strip: nothing is accepted, and the plane is the labels), one download of
// counters, sel and sel_new, and the accepted entries as positions of the list (pose_of; null: the entry's own).
void select_stage(CovCall& c, const DevTable& T, const SelLayout& S, const fdcm_select_params& sel, uint8_t* residual, size_t o_plane,
                  const int64_t* pose_of, int32_t* selected, int32_t* counts, int64_t* n_out) {
    const size_t ms = (size_t)sel.max_selected;
    FDCM_HIP(hipMemsetAsync(c.d + S.o_sel, 0x7f, ms * sizeof(int32_t), c.st));  // kSelNone
    FDCM_HIP(hipMemsetAsync(c.d + S.o_fresh, 0, (size_t)T.n * sizeof(int32_t), c.st));
    uint8_t* plane = c.claim_plane(residual, o_plane);
    if (T.items > 0) select_rounds(c.st, T.args(c), T, sel, c.d, S, plane);
    FDCM_HIP(hipMemcpyAsync(c.h, c.d + S.o_cnt, S.down(), hipMemcpyDeviceToHost, c.st));  // (the staging is free again)
    c.plane_down(residual, plane);
    FDCM_HIP(hipStreamSynchronize(c.st));
    const int32_t* h_cnt = (const int32_t*)c.h;
    const int32_t* h_sel = (const int32_t*)(c.h + (S.o_sel - S.o_cnt));
    const int32_t* h_new = (const int32_t*)(c.h + (S.o_new - S.o_cnt));
    size_t k = 0;
    for (; k < ms && h_sel[k] < (int32_t)T.n; ++k) {
        const int32_t i = h_sel[k];
        selected[k] = pose_of ? (int32_t)pose_of[i] : i;
        counts[3 * k] = h_cnt[2 * i];
        counts[3 * k + 1] = h_cnt[2 * i + 1];
        counts[3 * k + 2] = h_new[k];
    }
    *n_out = (int64_t)k;
}

// ---- the table of a part of a match list
constexpr size_t kCovPartBytes = (size_t)768 << 20;  // what a part's table may take (lines, host bins, poses, strips, offsets)

size_t table_record_bytes(const fdcm_templates* t, bool host_bins) {
    return (size_t)t->max_lines * (sizeof(CoverageLine) + (host_bins ? 2 : 0)) + sizeof(CovPose) + sizeof(int) + sizeof(long long);
}

// The records a part holds: what per_record bytes each allow in kCovPartBytes, FDCM_COVERAGE_PART at most.
size_t part_records(size_t N, size_t per_record) {
    const size_t pn = std::max<size_t>(1, std::min(N, kCovPartBytes / per_record));
    return test_switches().coverage_part > 0 ? std::min(pn, (size_t)test_switches().coverage_part) : pn;
}

// What the calls on match lists lay out for a table of pn records, from `at` on: host bins | lines | poses | strips | item
// offsets | total and largest
struct TableLayout {
    size_t o_bins, o_lines, o_tab, o_strips, o_item, o_tot, end;
    TableLayout(size_t at, size_t pn, size_t Lmax, bool host_bins) {
        o_bins = at;
        o_lines = o_bins + (host_bins ? al256(pn * Lmax * 2) : 0);
        o_tab = o_lines + al256(pn * Lmax * sizeof(CoverageLine));
        o_strips = o_tab + al256(pn * sizeof(CovPose));
        o_item = o_strips + al256(pn * sizeof(int));
        o_tot = o_item + al256((pn + 1) * sizeof(long long));
        end = o_tot + 256;
    }
    size_t bins_bytes() const { return o_lines - o_bins; }  // (of the staging as well)
};

// Queues k_matches_table and k_strip_scan for the records [q0, q0 + cnt) of the list at d_rec (the host bins of the part are
// uploaded through h_bins first), waits, and returns the part's table; its counters go to d_cnt + 2 q0.
DevTable make_table(CovCall& c, const fdcm_templates* t, const fdcm_match* d_rec, size_t q0, size_t cnt, int32_t base,
                    const std::vector<unsigned short>& bins, char* h_bins, const TableLayout& L, int* d_cnt) {
    fdcm_featuremap* fm = c.fm;
    char* d = c.d;
    const size_t Lmax = (size_t)t->max_lines;
    if (!bins.empty() && Lmax) {
        std::memcpy(h_bins, bins.data() + q0 * Lmax, cnt * Lmax * 2);
        FDCM_HIP(hipMemcpyAsync(d + L.o_bins, h_bins, cnt * Lmax * 2, hipMemcpyHostToDevice, c.st));
    }
    TableArgs a{};
    a.tlines = t->d_lines.as<float4>(); a.toff = t->d_offsets.as<long long>();
    a.keys = (const float*)((const char*)fm->build.plan.p + fm->off_keys);
    a.bins = bins.empty() ? nullptr : (const unsigned short*)(d + L.o_bins);
    a.rec = d_rec + q0;
    a.n = (int)cnt; a.base = base; a.T = (int)std::min<int64_t>(t->T, 0x7fffffff); a.Lmax = (int)Lmax;
    a.m = (int)fm->m; a.W = (int)fm->W; a.H = (int)fm->H; a.tx = fm->tx; a.ty = fm->ty;
    a.margin = (int)c.par.margin; a.width = c.width; a.height = c.height;
    a.lines = (CoverageLine*)(d + L.o_lines); a.poses = (CovPose*)(d + L.o_tab); a.strips = (int*)(d + L.o_strips);
    a.counts = d_cnt + 2 * q0;
    hipLaunchKernelGGL(k_matches_table, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, c.st, a);
    FDCM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_strip_scan, dim3(1), dim3(1024), 0, c.st, (const int*)a.strips, (int)cnt, (long long*)(d + L.o_item),
                       (long long*)(d + L.o_tot));
    FDCM_HIP(hipGetLastError());
    long long tot[2] = {0, 0};
    FDCM_HIP(hipMemcpyAsync(tot, d + L.o_tot, sizeof tot, hipMemcpyDeviceToHost, c.st));
    FDCM_HIP(hipStreamSynchronize(c.st));
    return DevTable{a.lines, a.poses, (const long long*)(d + L.o_item), (int)cnt, tot[0], tot[1]};
}

}  // namespace

// ---------------------------------------------------------------------------------------------- pose lists
// The arguments are checked (fdcm_capi.cpp).  One prepare_pairs for the distinct pairs of the list (n <= 2^20), one upload of
// lines, poses and item offsets (and a host caller's labels), the counters zeroed and the residual copied on the stream, then
// the launches and the counts' way down.
void run_scene_coverage(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                        const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                        const fdcm_coverage_params& params, int32_t* counts, uint8_t* residual) {
    CovCall c(fm, labels, width, height, on_device, bx, by, params);
    HostTable T;
    if (!c.nothing(n, t)) {  // (else the residual is the labels and the counts stay unwritten)
        T.make(fm, width, height, t, rot, poses, n, params.margin);
        for (int64_t q = 0; q < n; ++q) counts[2 * q] = counts[2 * q + 1] = T.adm[q] ? 0 : -1;
    }
    if (T.tab.empty()) return c.copy_labels(residual);
    const size_t o_lab = T.end + al256(T.tab.size() * 2 * sizeof(int32_t)), o_res = o_lab + c.labels_bytes();
    c.reserve(o_res + c.residual_bytes(residual), T.end);
    c.labels(o_lab);
    const DevTable D = upload_table(c, T);
    int* d_cnt = (int*)(c.d + T.end);
    uint8_t* d_res = c.residual_plane(residual, o_res);
    launch_coverage(c.st, D.args(c), D.items, d_cnt, d_res);
    counts_down(c, d_cnt, T.tab.size(), T.pose_of.data(), counts, residual, d_res);
}

// The arguments are checked (fdcm_capi.cpp).  run_scene_coverage's table, then the selection on it.
void run_scene_select(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                      const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                      const fdcm_coverage_params& params, const fdcm_select_params& sel, int32_t* selected, int32_t* counts,
                      int64_t* n_out, uint8_t* residual) {
    CovCall c(fm, labels, width, height, on_device, bx, by, params);
    *n_out = 0;
    HostTable T;
    if (!c.nothing(n, t)) T.make(fm, width, height, t, rot, poses, n, params.margin);
    if (T.tab.empty()) return c.copy_labels(residual);  // nothing explains a pixel: nothing is accepted
    const SelLayout S(T.end, T.tab.size(), (size_t)sel.max_selected);
    const size_t o_lab = S.end, o_plane = o_lab + c.labels_bytes();
    c.reserve(o_plane + c.claim_bytes(residual), std::max(T.end, S.down()));
    c.labels(o_lab);
    const DevTable D = upload_table(c, T);
    select_stage(c, D, S, sel, residual, o_plane, T.pose_of.data(), selected, counts, n_out);
}

// ---------------------------------------------------------------------------------------------- match lists
// Scene coverage of match records (include/fdcm.h, "Match lists: scene coverage and selection"): the arguments are checked
// (fdcm_capi.cpp).  The list is walked in parts of at most kCovPartBytes of table (FDCM_COVERAGE_PART: of that many records):
// per part the table pass, the scan, one download of the number of items, and k_scene_coverage on it; the counts are per
// record and the residual is an OR, so parts compose.  Only host records and the host's bins go up; counts and residual come down.
void run_matches_coverage(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                          const fdcm_templates* t, const MatchList& m, const fdcm_coverage_params& params, int32_t* counts,
                          uint8_t* residual) {
    CovCall c(fm, labels, width, height, on_device, bx, by, params);
    if (c.nothing(m.n, t)) return c.copy_labels(residual);
    const size_t N = (size_t)m.n;
    std::vector<unsigned short> bins;
    matches_host_bins(fm, t, m, bins);
    const size_t pn = part_records(N, table_record_bytes(t, !bins.empty()));
    const size_t s_bins = c.records_bytes(m);  // (the staging: host records | the part's bins; then the counters)
    const TableLayout L(s_bins, pn, (size_t)t->max_lines, !bins.empty());
    const size_t o_cnt = L.end, o_lab = o_cnt + al256(N * 2 * sizeof(int32_t)), o_res = o_lab + c.labels_bytes();
    c.reserve(o_res + c.residual_bytes(residual), std::max(s_bins + L.bins_bytes(), N * 2 * sizeof(int32_t)));
    c.labels(o_lab);
    const fdcm_match* d_rec = c.records(m);
    uint8_t* d_res = c.residual_plane(residual, o_res);
    int* d_cnt = (int*)(c.d + o_cnt);
    for (size_t q0 = 0; q0 < N; q0 += pn) {
        const size_t cnt = std::min(pn, N - q0);
        const DevTable D = make_table(c, t, d_rec, q0, cnt, m.base, bins, c.h + s_bins, L, d_cnt);
        launch_coverage(c.st, D.args(c), D.items, d_cnt + 2 * q0, d_res);
    }
    counts_down(c, d_cnt, N, nullptr, counts, residual, d_res);  // (the staging is free: every part has waited)
}

// Scene selection of match records: the arguments are checked (fdcm_capi.cpp), n <= 2^16.  The table is whole, every record an
// entry: a record that is not admissible holds (-1, -1) and one without a window (0, 0), so neither is in S_0, and the indices
// the rounds accept are the list's own.  Then run_scene_select's selection.
void run_matches_select(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                        const fdcm_templates* t, const MatchList& m, const fdcm_coverage_params& params, const fdcm_select_params& sel,
                        int32_t* selected, int32_t* counts, int64_t* n_out, uint8_t* residual) {
    CovCall c(fm, labels, width, height, on_device, bx, by, params);
    *n_out = 0;
    if (c.nothing(m.n, t)) return c.copy_labels(residual);
    const size_t N = (size_t)m.n;
    if (N * table_record_bytes(t, orientation_bins_on_host()) > ((size_t)2 << 30))  // (FDCM_EINVAL, before any GPU work)
        throw std::string("the selection's table, n records of max_lines lines each, would exceed 2 GB: cut the list with "
                          "fdcm_matches_detect first");
    std::vector<unsigned short> bins;
    matches_host_bins(fm, t, m, bins);
    const size_t s_bins = c.records_bytes(m);
    const TableLayout L(s_bins, N, (size_t)t->max_lines, !bins.empty());
    const SelLayout S(L.end, N, (size_t)sel.max_selected);
    const size_t o_lab = S.end, o_plane = o_lab + c.labels_bytes();
    c.reserve(o_plane + c.claim_bytes(residual), std::max(s_bins + L.bins_bytes(), S.down()));
    c.labels(o_lab);
    const DevTable D = make_table(c, t, c.records(m), 0, N, m.base, bins, c.h + s_bins, L, (int*)(c.d + S.o_cnt));
    select_stage(c, D, S, sel, residual, o_plane, nullptr, selected, counts, n_out);
}

// The pose fit of match records (include/fdcm.h, "Match lists: pose fit"): the arguments are checked (fdcm_capi.cpp).  The
// records are copied into the handle's buffer once and stay there; the list is walked in parts of at most kCovPartBytes of
// table and moments (FDCM_COVERAGE_PART: of that many records), and per part iterations + 1 passes are queued: the table of the
// current transforms and its scan (one download of the number of items, as in run_matches_coverage), the moments zeroed,
// k_fit_moments, k_fit_step.  Where the host's libm makes the bins, every pass downloads the part's records for them
// (matches_host_bins).  Records, info and rms come down once, at the end.
void run_matches_fit(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                     const fdcm_templates* t, const MatchList& m, const fdcm_coverage_params& params, const fdcm_fit_params& fit,
                     fdcm_match* out, bool out_on_device, int32_t* info_out, float* rms_out) {
    CovCall c(fm, labels, width, height, on_device, bx, by, params);
    if (c.nothing(m.n, t)) return;  // nothing is written, as the coverage call's counts
    const size_t N = (size_t)m.n, Lmax = (size_t)t->max_lines;
    const bool host_bins = orientation_bins_on_host();
    const size_t pn = part_records(N, table_record_bytes(t, host_bins) + Lmax * 6 * sizeof(long long) + 2 * sizeof(int32_t));
    // records | replaced transforms | info | rms (what comes down), then the part's table, counters and moments
    const size_t o_prev = al256(N * sizeof(fdcm_match)), o_info = o_prev + al256(N * 6 * sizeof(float)),
                 o_rms = o_info + al256(N * 4 * sizeof(int32_t));
    const TableLayout L(o_rms + al256(N * 2 * sizeof(float)), pn, Lmax, host_bins);
    const size_t o_cnt = L.end, o_mom = o_cnt + al256(pn * 2 * sizeof(int32_t)), o_lab = o_mom + al256(pn * Lmax * 6 * sizeof(long long));
    const size_t s_bins = L.o_bins;  // (the staging: host records up, then the results down; behind them the part's bins)
    c.reserve(o_lab + c.labels_bytes(), s_bins + L.bins_bytes());
    c.labels(o_lab);
    char *d = c.d, *h = c.h;
    hipStream_t st = c.st;
    fdcm_match* d_cur = (fdcm_match*)d;
    if (m.on_device) FDCM_HIP(hipMemcpyAsync(d_cur, m.rec, N * sizeof(fdcm_match), hipMemcpyDeviceToDevice, st));
    else c.records(m);
    FDCM_HIP(hipMemsetAsync(d + o_info, 0x7f, N * 4 * sizeof(int32_t), st));  // kFitActive
    std::vector<unsigned short> bins;
    for (size_t q0 = 0; q0 < N; q0 += pn) {
        const size_t cnt = std::min(pn, N - q0);
        FitArgs a{};
        a.counts = (const int*)(d + o_cnt); a.mom = (const long long*)(d + o_mom);
        a.cur = d_cur + q0; a.prev = (float*)(d + o_prev) + 6 * q0; a.info = (int*)(d + o_info) + 4 * q0; a.rms = (float*)(d + o_rms) + 2 * q0;
        a.n = (int)cnt; a.Lmax = (int)Lmax; a.par = fit; a.tx = fm->tx; a.ty = fm->ty; a.bx = bx; a.by = by;
        for (int pass = 0; pass <= fit.iterations; ++pass) {
            matches_host_bins(fm, t, MatchList{d_cur + q0, (int64_t)cnt, true, m.base}, bins);  // (empty unless the host's libm makes them)
            const DevTable D = make_table(c, t, d_cur + q0, 0, cnt, m.base, bins, h + s_bins, L, (int*)(d + o_cnt));
            const SelArgs s = D.args(c);
            if (Lmax) FDCM_HIP(hipMemsetAsync(d + o_mom, 0, cnt * Lmax * 6 * sizeof(long long), st));
            for_items(D.items, [&](unsigned grid, long long base) {
                hipLaunchKernelGGL(k_fit_moments, dim3(grid), dim3(kCovThreads), 0, st, s.labels, s.width, s.height, s.m, s.tx, s.ty, s.bx, s.by,
                                   s.radius, s.tol, s.lines, s.poses, s.item0, s.n_poses, base, (const int*)a.info,
                                   (unsigned long long*)(d + o_mom), (int)Lmax);
            });
            a.lines = D.lines; a.poses = D.poses; a.pass = pass;
            hipLaunchKernelGGL(k_fit_step, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, a);
            FDCM_HIP(hipGetLastError());
        }
    }
    // down: info and rms through the staging (free: every part has waited behind the upload), the records to where they go
    FDCM_HIP(hipMemcpyAsync(h + o_info, d + o_info, N * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipMemcpyAsync(h + o_rms, d + o_rms, N * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_on_device) FDCM_HIP(hipMemcpyAsync(out, d_cur, N * sizeof(fdcm_match), hipMemcpyDeviceToDevice, st));
    else FDCM_HIP(hipMemcpyAsync(h, d_cur, N * sizeof(fdcm_match), hipMemcpyDeviceToHost, st));
    FDCM_HIP(hipStreamSynchronize(st));
    if (!out_on_device) std::memcpy(out, h, N * sizeof(fdcm_match));
    if (info_out) std::memcpy(info_out, h + o_info, N * 4 * sizeof(int32_t));
    if (rms_out) std::memcpy(rms_out, h + o_rms, N * 2 * sizeof(float));
}

}  // namespace fdcm
