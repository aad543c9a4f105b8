// fdcm_sweep.h -- the balanced L2 / L2^2 sweep (fdcm_sweep.hip), as run_build (fdcm_build.hip) sees it.
#pragma once
#include <hip/hip_runtime.h>

namespace fdcm {

struct EnvEntry;
struct OwnEntry;

static constexpr int kSweepSegments = 8;  // column ranges per row = waves per workgroup
static constexpr int kSweepMinCols = 16;  // seeded columns a range holds at least (fewer ranges on small slices)
static constexpr int kSweepMaxBlocks = 128;  // claim blocks of columns per slice at most

// Scratch of the sweep, per chunk and slot-major: the 64 rows of a chunk side by side in every slot (rows of a chunk stand at
// similar depths: what a wave appends, lane = row, shares a few lines).
struct SweepBuf {
    EnvEntry* ent;                        // stack entries [chunk][slot][row], eslots per row (>= W)
    OwnEntry* own;                        // owner list [chunk][index][row], lslots per row (>= W + 2)
    const int* order;                     // launch position -> chunk (longest chunks of the previous build first), or null
    int* cost;                            // per chunk: 100 MHz ticks from the block's start to the end of its owner walk
    int eslots, lslots;
    const unsigned long long* colmask;    // [slice][(W + 63) / 64]: the slice's seeded columns (k_coldesc_tile)
    int min_cols;                         // seeded columns a range holds at least (set by the launcher)
    int steal_min;                        // a wave out of columns starts a new range in a stretch of at least this many unclaimed blocks
                                          // (0: never, ranges of equal count only; < 0: the launcher's default; FDCM_SWEEP_STEAL overrides both)
    int steal_heavy_only;                 // 1: only the heaviest workgroups (launch rank / seeded columns) cut dynamically
    int steal_cols;                       // .. that holds this many columns at least
    int* steals;                          // [0]: ranges taken over so far (all launches of the handle), or null
};

// column ranges per row of a slice with n seeded columns: at most kSweepSegments, each with min_cols columns at least
// (the kernel and fdcm_selftest_sweep_ranges use this one function)
__host__ __device__ inline int sweep_ranges(int n, int min_cols) {
    const int s = n / (min_cols > 1 ? min_cols : 1);
    return s < 1 ? 1 : (s > kSweepSegments ? kSweepSegments : s);
}

// the sweep applies when every value of the pass is an exact integer (see fdcm_sweep.hip)
inline bool sweep_balanced_applies(long W, long H) { return W * W + H * H <= (1L << 24); }

// queues the sweep of nchunks (slice, 64-row chunk) pairs on st; vol receives the transforms in the interleaved layout
void launch_sweep_balanced(hipStream_t st, const void* desc, float* vol, int W, int H, int HW64, long nchunks, const SweepBuf& B);
// launch order of the next sweep: chunks by decreasing cost (one workgroup; order = a permutation of 0 .. n - 1 whatever the costs are)
void launch_sweep_order(hipStream_t st, const int* cost, int n, int* order);

// fdcm_sweep_literal.hip: the reference's pass followed literally, one wave per chunk -- any feature size
size_t sweep_literal_scratch_bytes(int W, long nchunks);
void launch_sweep_literal(hipStream_t st, const void* desc, float* vol, int W, int H, int HW64, long nchunks, void* scratch);

}  // namespace fdcm
