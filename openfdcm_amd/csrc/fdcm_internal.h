// fdcm_internal.h -- shared declarations of libfdcm_hip.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fdcm.h"
#include "fdcm_math.h"

namespace fdcm {

// ---------------------------------------------------------------- error plumbing
void set_error(const std::string& msg);
struct HipError { hipError_t code; const char* what; int line; };
#define FDCM_HIP(call)                                                              \
    do {                                                                            \
        hipError_t e__ = (call);                                                    \
        if (e__ != hipSuccess) throw ::fdcm::HipError{e__, #call, __LINE__};        \
    } while (0)

// ---------------------------------------------------------------- the tests' switches
// Environment variables that make the library take, at the tests' small sizes, a path that only other sizes or other hosts
// select.  test_switches() (fdcm_host.cpp) reads and checks them once per process; nothing else reads the environment.
// An unset or invalid switch leaves the default.
//   FDCM_L2_SWEEP=literal      the literal L2 sweep, one wave per chunk, at every size (build_layout)
//   FDCM_SWEEP_ORDER           the L2 sweep's launch order from a cost table at every size (setup_balanced_sweep)
//   FDCM_SWEEP_MINCOLS=1..64   seeded columns a sweep range holds at least, instead of 16 (launch_sweep_balanced)
//   FDCM_SWEEP_STEAL=0..128    the sweep's dynamic cuts on every workgroup, in unclaimed stretches of at least this many
//                              blocks; 0: never (launch_sweep_balanced)
//   FDCM_INT_XC=64|128|256     the steep line integral's chains per workgroup (stage_integral)
//   FDCM_FORCE_HOST_BINS       the candidates' orientation bins from the host libm (orientation_bins_on_host)
//   FDCM_SEARCH_FLAT           the search with 64-bit flat addresses (run_search)
//   FDCM_SEARCH_COMPACT2       the search's two-kernel compaction at every size (run_search)
//   FDCM_WINDOWS_BATCH=1..     planes a batch of the pose-window search holds at most, instead of 65536 (windows_round),
//                              and 4 KB of tables per such plane a round, instead of 256 MB (run_search_exhaustive_windows)
//   FDCM_WINDOWS_FLAT          the pose-window search with 64-bit flat addresses (windows_round), the scoring and the winners'
//                              pass of the detections over pose windows with it
//   FDCM_MATCHED_FLAT          the calls by matched fraction with 64-bit flat addresses (dense_detect and best_maps with a
//                              gate or objects, run_matched_fractions, run_search_exhaustive_detect_windows: its scoring,
//                              its winners' pass and its fractions; run_matches: the verify pass of the calls on match
//                              lists, which also take their bins from the host under FDCM_FORCE_HOST_BINS)
//   FDCM_COVERAGE_PART=1..     records a part of the scene coverage of a match list holds at most, instead of what 768 MB of
//                              table hold (run_matches_coverage; run_matches_fit: of table and moments)
//   FDCM_REFINE_PART=1..       records a part of the refinement of a match list holds at most, instead of what 512 MB of lines,
//                              planes and keys hold (run_matches_refine)
//   FDCM_MESH_PART=1..         views a part of the templates from a mesh holds at most, instead of what 512 MB of item buffers,
//                              lists and counts hold, and 16 lines per such view a writing pass, instead of 256 MB of them
//                              (mesh_view_lines)
//   FDCM_EXHAUSTIVE_FLAT       the dense exhaustive calls with 64-bit flat addresses: every prepare_pairs call that otherwise
//                              takes that form for a volume of 4 GB or more alone (score maps, top-k, peaks, rotations, best
//                              map, the detections, line costs); the pose windows and the calls by matched fraction keep
//                              their own switches
//   FDCM_POISON=<uint32>       (decimal or 0x-hex) what a call finds in memory it did not write: the whole capacity of a
//                              buffer holds the word before the call's first write (poison_fill; DESIGN.md sections 22 and
//                              32).  reserve_eval: search.eval and search.eval_stage (and run_matches the span table of a match
//                              list's shapes, search.eval_spans, counted as a fill of eval).  run_build: the whole allocation of the
//                              volume, padding included (an adopted volume is not touched), ivol, bitmap, coldesc, colmask,
//                              labels, edge_parent, edge_roots, pyr, offtab, stack, plan and the pinned build.stage.
//                              run_search: scene, pairs, records, flags, work, counter, bins, the pinned stage, bins_stage
//                              and cnt, and search.out in a host-output search.  run_topk_device / run_topk: search.tail,
//                              search.stage, search.tail_out.  The coverage calls: coverage, coverage_stage.  The calls
//                              without a handle: every member of PixelScratch as it is allocated.  What is state stays
//                              while the handle's record says it is valid: the balanced sweep's per-chunk costs
//                              (sweep.cost_chunks, cost_w) and steal counter (sweep.steals_off) in stack, the line integral's
//                              group table (groups) in offtab, and the last search's matches in search.out, which only the
//                              host-output search that overwrites them fills.  Without the switch nothing is queued, copied,
//                              waited for or allocated that was not before.  The tests use the words 0 and 1 alone.  1 is
//                              the smallest denormal as a float (a near-perfect score), 0x0000000100000001 as a 64-bit key
//                              (below every real key in every min and atomicMin), one too many as a count and in bounds as
//                              an index, and as a union-find parent (parent[0] == 0, parent[1] == 1) a root that ends the
//                              walk: a kernel that reads what nobody wrote reads a wrong value from a valid place.  Words
//                              that are large as integers (0xFFFFFFFF, NaN patterns) hide a missing "no key" initialisation
//                              and leave the allocation as an index; they are not for the GPU machines.
struct TestSwitches {
    bool literal_sweep, sweep_order;
    int sweep_min_cols;  // 16 unless forced
    int sweep_steal;     // -1: not forced
    int int_xc;          // 0: not forced
    bool host_bins, search_flat, search_compact2;
    int windows_batch;  // 0: not forced
    bool windows_flat, matched_flat, exhaustive_flat;
    int coverage_part;  // 0: not forced
    int refine_part;    // 0: not forced
    int mesh_part;      // 0: not forced
    bool poison;           // FDCM_POISON holds a valid word
    uint32_t poison_word;
};
const TestSwitches& test_switches();

// ---------------------------------------------------------------- device buffers (grow-only)
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    void reserve(size_t bytes);
    void release();
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    void reserve(size_t bytes);
    void release();
};
// While a thread holds a NoGrowScope, a DevBuf / PinnedBuf reserve that would have to grow throws (std::logic_error)
// instead of allocating.  The sharded engine's slot workers run their frames inside one: every allocation of a frame
// happens on the caller's thread before the workers get it (fdcm_sharded.cpp, submit_frame).
struct NoGrowScope { NoGrowScope(); ~NoGrowScope(); };
// FDCM_POISON's fill (above): the whole capacity of a buffer holds the word -- a device buffer by one
// fill queued on `st`, which must be the stream whose work touches the buffer first; a pinned one by the host, and nothing in
// flight may still read it (the caller has waited).  `keep`: byte ranges of the buffer, ascending and disjoint, that are
// state and stay as they are.  `id` (fdcm_poison_buffer) counts the fill for fdcm_selftest_poison_fills.  Without the switch,
// and for a buffer without capacity, they do nothing; they allocate nothing.
struct KeepRange { size_t begin, end; };
void poison_fill(DevBuf& b, hipStream_t st, int id, const KeepRange* keep = nullptr, int n_keep = 0);
void poison_fill(PinnedBuf& b, int id);
int64_t poison_fill_count(int id);

// ---------------------------------------------------------------- build plan (host -> device)
// One clipped scene line to rasterise (drawLines, drawing.h:111-125).  Each axis is either a
// constant or Eigen's LinSpaced(n, low, high) (restated in lin_spaced_value below).
struct RasterLine {
    int32_t slice;
    int32_t n;
    float xlow, xhigh, xstep;
    float ylow, yhigh, ystep;
    int32_t xmode, ymode;  // 0 = constant (xlow / ylow), 1 = LinSpaced, 2 = LinSpaced flipped
};
// One step of propagateOrientation (dt3cpu.cpp:86-101): S[c2] = min(S[c2], S[c1] + w).
struct PropStep {
    int32_t c1, c2;
    float w;
    int32_t pad;
};
// lineIntegral of one slice (imgproc.h:38-84): mode 1 sweeps along x (|rastvec.x| == 1), mode 2
// along y (|rastvec.y| == 1), mode 0 does nothing.  s = +-1 sweep direction, r = the other
// rastvec component (chain offset at step i is round(float(i) * r)).
struct IntegralDesc {
    int32_t mode, s;
    float r;
    int32_t pad;
};

struct LineBox { int32_t slice; float xlo, xhi, ylo, yhi; };

// Where the seeds of a build come from: the plan's clipped scene lines, a label image (one byte per pixel, row-major, value k
// < m: a seed of slice k, anything else: none), or a grey image whose oriented edge pixels become the labels first
// (k_edge_labels; `edge` holds the detector's parameters, and unless they are k_edge_labels' own -- edge_plain -- the
// candidate kernel and the component kernels make the labels).  Pixel (x, y) seeds map pixel (x + border, y + border).  The
// pixels are host memory, which travels in the plan's blob with rows packed, or memory of the handle's device, which is read
// in place while the build runs.  An image build of level l > 0 (include/fdcm.h, "image pyramid") takes its seeds from P_l: the
// caller's pixels are width0 x height0, the build reduces them l times in the handle's workspace, and width x height is P_l's size.
enum class SeedKind { lines, labels, image };
struct SeedSource {
    SeedKind kind = SeedKind::lines;
    const uint8_t* pixels = nullptr;
    bool on_device = false;
    int width = 0, height = 0, row_stride = 0, border = 0;
    int level = 0, width0 = 0, height0 = 0;  // the caller's pixels: width0 x height0 with row_stride (level 0: width x height)
    fdcm_edge_params edge = {0, 0, 0, 1};  // (image only; one threshold t: {0, t, t, 1})
    bool edge_plain() const { return edge.smooth == 0 && edge.low == edge.high && edge.min_pixels == 1; }
    size_t bytes() const { return kind == SeedKind::lines ? 0 : (size_t)width * (size_t)height; }
    size_t source_bytes() const { return kind == SeedKind::lines ? 0 : (size_t)width0 * (size_t)height0; }
};

struct BuildPlan {
    int64_t W = 0, H = 0, m = 0;
    float tx = 0, ty = 0;
    std::vector<float> keys;
    std::vector<RasterLine> raster;      // ordered by slice
    std::vector<int32_t> slice_first;    // m + 1: the lines of slice k are raster[slice_first[k] .. slice_first[k + 1])
    std::vector<PropStep> prop;
    std::vector<IntegralDesc> integral;
    std::vector<LineBox> boxes;       // the clipped lines' bounding boxes (what sweep_cost_proxy works from)
    SeedSource seeds;                 // (lines: raster / slice_first / boxes above; else they stay empty)
};

// Every size and offset (bytes) a build of one shape takes: reserve_build sizes the buffers from it, run_build takes its
// offsets from it.  A size of 0: the build does not use that buffer.
struct BuildLayout {
    bool empty = true;      // no slices or no pixels: nothing to build
    bool balanced = false;  // the L2 / L2^2 sweep of equal column ranges (fdcm_sweep.hip); the literal one otherwise (L2 builds)
    int HW64 = 0, slots = 0;  // 64-row chunks per column; stack and owner entries per row of the balanced sweep
    long nchunks = 0;       // (slice, 64-row chunk) pairs
    size_t vol = 0, ivol = 0, bitmap = 0, coldesc = 0, colmask = 0, offtab = 0, stack = 0;
    size_t labels = 0;      // the label image an image build makes of its pixels
    size_t edge_parent = 0, edge_roots = 0;  // image builds with hysteresis: a parent and a (strong flag | count) word per pixel
    size_t pyr = 0, pyr_b = 0;  // image builds of a level > 0: the two buffers the levels go through, and where the second begins
    size_t o_ent = 0, o_own = 0, o_ord = 0, o_cost = 0, o_steals = 0;  // inside `stack` (balanced sweep)
    // plan blob: RasterLine[] | PropStep[] | IntegralDesc[] | keys[] | slice_first[] | host pixels of the seed source | per-chunk proxy cost[]
    size_t off_raster = 0, off_prop = 0, off_integral = 0, off_keys = 0, off_slice = 0, off_pixels = 0, off_cost = 0, plan = 0;
};
// Host side of buildCpuFeaturemap (dt3cpu.h:174-198 + the scalar parts of :227-231).
void make_build_plan(const float* lines, int64_t n, int64_t depth, float coeff, float padding, BuildPlan& plan);
// The parts of a plan that the shape alone decides: the distinct angle keys of `depth`, the propagation's steps and the line
// integral's direction per slice (make_build_plan's, and all of the plan of a build whose seeds are pixels).
void plan_keys(int64_t depth, std::vector<float>& keys);
void make_shape_plan(int64_t depth, float coeff, int64_t W, int64_t H, BuildPlan& plan);
// per (slice, 64-row chunk): a proxy of the L2 sweep's time, for the launch order of a build without history
void sweep_cost_proxy(const BuildPlan& plan, std::vector<int32_t>& cost);

FDCM_HD float lin_spaced_value(int mode, float low, float high, float step, int n, int i) {
    // Eigen 3.4.0 linspaced_op_impl<float>::operator() (NullaryFunctors.h), scalar path.
    if (mode == 0) return low;
    const int size1 = (n == 1) ? 1 : n - 1;
    if (mode == 2) return (i == 0) ? low : (high - (float)(size1 - i) * step);
    return (i == size1) ? high : (low + (float)i * step);
}

// ---------------------------------------------------------------- the volume
// The volume lives in one layout from the sweeps' first store on: interleaved, [k][x/4][y][x%4], so that a 64-byte sector
// holds 4 x by 4 y pixels (columns of the last group past W are padding).  The search gathers single floats at positions
// that step by about one pixel per translation, in any direction: 16 steps along x touch 4 to 8 sectors here, 16 in a volume
// whose columns are contiguous.
// Slices are 4352 bytes longer than their pixels: feature sizes are powers of two in practice, and a candidate's
// gathers read the same place of up to `depth` slices -- with slices a power of two apart they all fall on the same
// memory channels (config 2': the search kernels took 0.24 - 0.36 ms depending on where the allocation landed,
// 0.21 - 0.22 ms with the padding; 256 bytes of padding were not enough, 2 to 20 KB all the same).
static constexpr size_t kSlicePad = 1088;  // floats
FDCM_HD size_t ivol_slice_floats(int64_t W, int64_t H) { return (size_t)((W + 3) / 4) * (size_t)H * 4 + kSlicePad; }
FDCM_HD size_t ivol_index(int x, int y, int64_t H) { return ((size_t)(x >> 2) * (size_t)H + (size_t)y) * 4 + (size_t)(x & 3); }
// one slice between the interleaved layout and the caller's [x][y] (host side of fdcm_featuremap_slice / _from_slices)
inline void slice_to_xy(const float* il, float* xy, int64_t W, int64_t H) {
    for (int64_t x = 0; x < W; ++x)
        for (int64_t y = 0; y < H; ++y) xy[(size_t)x * H + y] = il[ivol_index((int)x, (int)y, H)];
}
inline void slice_from_xy(const float* xy, float* il, int64_t W, int64_t H) {
    for (int64_t x = 0; x < W; ++x)
        for (int64_t y = 0; y < H; ++y) il[ivol_index((int)x, (int)y, H)] = xy[(size_t)x * H + y];
}
// what a handle holds: nothing (no pixels), or the volume after the sweeps / the propagation (staged test builds) / the line integral
enum class VolStage { none, transforms, propagated, integrated };

// ---------------------------------------------------------------- handles
struct Timing { hipEvent_t ev[9] = {}; bool created = false; };  // events 0-5 build stages, 6-7 search kernels, 8 search download

// What the balanced L2 sweep left in `stack` for the next one, until the scratch moves or another sweep writes it: per-chunk costs of a
// build with this shape (0 chunks: none), and at this offset the count of ranges its waves took over (0: none; fdcm_selftest_sweep_steals).
struct SweepHistory { long cost_chunks = 0; int cost_w = 0; size_t steals_off = 0; void reset() { *this = SweepHistory{}; } };
// The line integral's group table in `offtab` is that of this depth and feature width (the keys are fixed per handle).
struct GroupTable { int m = 0, steps = 0; void reset() { *this = GroupTable{}; } };
// The last build of the handle, from run_build to finish_build.
struct BuildRecord {
    bool pending = false;       // queued on `stream` but not waited for
    bool seeds_fused = false;   // it drew its seeds inside k_coldesc_tile / took them from labels (no seeds stage, no event for it)
    bool stage_events = false, total_events = false;  // it recorded an event between its stages (per-stage times) / its first and last one (span)
    float host_ms = 0.f;        // host time of the call up to its first kernel launch
    void reset() { *this = BuildRecord{}; }
};
struct BuildBuffers {  // what a build needs besides the volume, sized by BuildLayout
    DevBuf bitmap;   // m*W*ceil(H/64) uint64 seed bits along y (feature sizes above 4096 only: k_seeds + k_coldesc)
    DevBuf coldesc;  // m*ceil(H/64)*W column-chunk descriptors (16 B)
    DevBuf colmask;  // m*ceil(W/64) words: the seeded columns of every slice (k_coldesc_tile, for the L2 sweep)
    DevBuf labels;   // image builds: the label image k_edge_labels writes and k_coldesc_labels reads
    DevBuf edge_parent, edge_roots;  // image builds with hysteresis: the union-find of the candidates (launch_edge_labels)
    DevBuf pyr;      // image builds of a level > 0: P_1, P_3, .. at its start and P_2, P_4, .. at BuildLayout::pyr_b (launch_pyramid)
    DevBuf offtab;   // per slice: one word per group of 4 columns for the shallow sweeps of the line integral (k_groups)
    DevBuf stack;    // the sweep's scratch: the balanced sweep's stack and owner entries (slot-major per chunk), launch order,
                     // per-chunk costs and steal counter; or the literal pass's scratch; or the L1 pass's minima / carries
    DevBuf plan; PinnedBuf stage;  // the last build's plan (BuildLayout's blob) or the keys of an adopted volume; its host staging
    void release() { for (DevBuf* b : {&bitmap, &coldesc, &colmask, &labels, &edge_parent, &edge_roots, &pyr, &offtab, &stack, &plan}) b->release(); stage.release(); }
};
struct SearchBuffers {
    DevBuf scene;     // scene lines + sorted lengths + sorted idx + candidate offsets
    DevBuf pairs;     // (template line, scene line) per search combination
    DevBuf records, flags;  // per candidate: result record; valid flag + scan scratch
    DevBuf out;       // compacted matches
    DevBuf work;      // search work list: valid pairs grouped by scene line
    DevBuf tail, tail_out;  // device tail (penalise + sort + top k): workspace; the k best before their download
    DevBuf eval;      // fdcm_featuremap_evaluate / _minmax_translation, exhaustive search: lines, translations, work items, results
    DevBuf counter;   // the search's counters
    DevBuf bins;      // orientation bins per candidate line from the host libm (only when it differs from the device's atanf)
    DevBuf eval_spans;  // the span table of the shapes of a match list: sized once the device has counted its rows, while eval
                        // holds the pass's results (reserve_eval could move them); FDCM_POISON fills it as a part of eval
    PinnedBuf stage, bins_stage, eval_stage;  // host side of the uploads into scene (and the tail's denominators), bins, eval
    PinnedBuf cnt;    // the search's counters, written by k_scatter (device-output searches)
    void release() {
        for (DevBuf* b : {&scene, &pairs, &records, &flags, &out, &work, &tail, &tail_out, &eval, &eval_spans, &counter, &bins}) b->release();
        for (PinnedBuf* b : {&stage, &bins_stage, &eval_stage, &cnt}) b->release();
    }
};

}  // namespace fdcm

struct fdcm_featuremap {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t prep_stream = nullptr;  // the search's preparation beside a running build (handles that have the GPU to themselves)
    hipEvent_t prep_done = nullptr;
    // parameters
    int64_t depth_param = 0;
    float coeff = 0, padding = 0;
    int distance = 0;
    bool pixel_seeded = false;  // the last build took its seeds from an image or labels: no padding went into its geometry
    int want_stage_events = 1;  // fdcm_featuremap_stage_timing: 0 no events, 1 an event between the build's stages, 2 around the build and the search only
    bool shares_gpu = false;    // a frame slot of a pipeline with several frames in flight: other frames' kernels run beside this handle's
    // geometry
    int64_t W = 0, H = 0, m = 0;
    float tx = 0, ty = 0;
    std::vector<float> keys;
    size_t off_keys = 0;  // where the keys are in `build.plan` (the search reads them there)
    // The volume, interleaved (ivol_index) in either buffer: the sweeps write the distance transforms into `vol`, the
    // propagation reads them and writes `ivol`, the line integral reads `ivol` and writes its sums back into `vol` --
    // which is what the search gathers from.
    fdcm::DevBuf vol;   // m*ivol_slice_floats floats
    fdcm::DevBuf ivol;  // the same (builds that go past the sweeps)
    fdcm::VolStage holds = fdcm::VolStage::none;
    const float* current() const { return holds == fdcm::VolStage::propagated ? ivol.as<float>() : vol.as<float>(); }
    fdcm::BuildBuffers build;
    fdcm::SweepHistory sweep;
    fdcm::GroupTable groups;
    fdcm::BuildRecord built;
    int* steal_counter() const { return sweep.steals_off ? (int*)((char*)build.stack.p + sweep.steals_off) : nullptr; }
    fdcm::SearchBuffers search;
    fdcm::DevBuf coverage;            // fdcm_scene_coverage, fdcm_scene_select: lines, poses, item offsets, counters, and a host caller's labels and residual
    fdcm::PinnedBuf coverage_stage;   // its upload and the counters' download
    std::mutex seam_mutex;  // evaluate / minmax_translation (called from pool threads on one feature map, batchoptimize.cpp:102-110) and
                            // the exhaustive search share search.eval and the stream: they take turns
    int64_t last_n_out = 0; // matches of the last host-output search, still in search.out
    fdcm::Timing timing;
    fdcm_build_timing last_build = {};
    fdcm_search_timing last_search = {};
};

struct fdcm_templates {
    int device = 0;
    int64_t T = 0, n_lines = 0, max_lines = 0;
    std::vector<float> lines;       // host copy
    std::vector<int64_t> offsets;   // T+1
    std::vector<float> lengths;     // per line: getLength, math.h:306-308
    std::vector<float> caps;        // per line: the cap of its cost in the exhaustive calls, +inf for none (include/fdcm.h)
    bool capped = false;            // some cap is finite: the exhaustive calls take their clamping kernels
    int32_t footprint = 0;          // FDCM_FOOTPRINT_BOX or _HULL: the shape the overlap rule gives its pairs (include/fdcm.h)
    std::vector<int32_t> sorted;   // per template: line indices by descending length (argsort, math.h:106-116)
    fdcm::DevBuf d_lines, d_offsets, d_lengths, d_sorted;
};

// A triangle mesh with its edge table (include/fdcm.h, "Templates from a mesh"): host memory alone; a view call uploads it.
struct fdcm_mesh {
    int64_t V = 0, F = 0, E = 0, n_sharp = 0, n_boundary = 0;
    std::vector<float> vertices;   // 3 V
    std::vector<int32_t> faces;    // 3 F
    std::vector<int32_t> edges;    // 4 E: i < j, f0 < f1 (-1: a boundary edge), ascending (i, j)
    std::vector<uint8_t> sharp;    // E
};

namespace fdcm {
// implemented in fdcm_mesh.hip: the arguments are checked but for what needs the table (indices, finiteness, manifoldness),
// which mesh_create refuses with a std::string.  The view calls block, on the null stream of `device`, and hold what they need
// there in a PixelScratch of their own; n_views >= 1.  *lines_out is malloc'ed (fdcm_lines_free), untouched when there is no line.
fdcm_mesh* mesh_create(const float* vertices, int64_t V, const int32_t* faces, int64_t F, double crease_cos);
void mesh_view_lines(int device, const fdcm_mesh* m, const float* views, int64_t n_views, float scale, const fdcm_mesh_line_params& p,
                     float** lines_out, int64_t* offsets_out);
void mesh_view_items(int device, const fdcm_mesh* m, const float* view, float scale, int32_t* box_out, uint64_t* keys_out, int64_t capacity);
// the same two through a pinhole camera ("Templates from a mesh: pinhole views"): positions, 3 floats per view, beside the views
void mesh_view_lines_cam(int device, const fdcm_mesh* m, const float* views, const float* positions, int64_t n_views, const fdcm_mesh_camera& cam,
                         const fdcm_mesh_line_params& p, float** lines_out, int64_t* offsets_out);
void mesh_view_items_cam(int device, const fdcm_mesh* m, const float* view, const float* position, const fdcm_mesh_camera& cam, int32_t* box_out,
                         uint64_t* keys_out, int64_t capacity);
// implemented in fdcm_build.hip
void ensure_stream(fdcm_featuremap* fm);  // the handle's stream and timing events, made on first use (on fm's device)
BuildLayout build_layout(const BuildPlan& plan, int distance, int stop_after);  // from the plan's shape and counts
// grows the handle's buffers to the layout and queues nothing (its geometry, plan offsets and content stay; a scratch that
// had to move drops the sweep's cost history and steal counter)
void reserve_build(fdcm_featuremap* fm, const BuildLayout& L);
void run_build(fdcm_featuremap* fm, const BuildPlan& plan, int stop_after);
// implemented in fdcm_image.hip: image -> label image by `e` (include/fdcm.h, "edges with smoothing, hysteresis and a minimum
// chain length"), queued on st.  With `parent` and `roots` (width * height words each): candidates, their components by
// union-find in `parent`, strong flag and size per root in `roots`.  With both null: k_edge_labels with the one threshold
// e.high, which is the same for {0, t, t, 1} and needs no scratch.
void launch_edge_labels(hipStream_t st, const uint8_t* image, int width, int height, int row_stride, const float* keys, int m,
                        const fdcm_edge_params& e, uint8_t* labels, int32_t* parent, uint32_t* roots);
// The image pyramid (include/fdcm.h, "image pyramid"): the size of P_level, and `level` launches of k_pyr_down queued on st, level
// l + 1 from level l, the odd levels into `a` (W_1 H_1 bytes) and the even ones into `b` (W_2 H_2 bytes).  Returns where P_level
// is, rows contiguous: the image itself for level 0.  The caller's device memory is only ever read and written by kernels.
void pyramid_size(int64_t width, int64_t height, int level, int64_t* w_out, int64_t* h_out);
const uint8_t* launch_pyramid(hipStream_t st, const uint8_t* image, int width, int height, int row_stride, int level, uint8_t* a, uint8_t* b,
                              uint8_t* last = nullptr);  // last: where the last level goes in place of its buffer
// host or device image -> P_level into host or device memory, blocking, on the null stream of `device`
void image_pyramid_host(int device, const uint8_t* image, int width, int height, int row_stride, bool on_device, int level, uint8_t* out,
                        bool out_on_device);
// pass 1 with its seeds from a label image (k_coldesc_labels); `cost`, where given, receives the sweep's per-chunk proxy (zeroed
// by the caller)
void launch_coldesc_labels(hipStream_t st, const uint8_t* labels, int width, int height, int border, void* desc, int W, int H,
                           int HW64, int m, unsigned* colmask, int* cost);
// What a call without a handle holds on the device, allocated per call and released at its end: the pixels and keys it
// uploaded, the label image, and the scratch of the edge and line stages.
struct PixelScratch {
    // edge_labels_host: pixels, keys, labels, and comps for the edge kernels' parent and root words.  lines_from_labels_host:
    // pixels (the labels), parent (both partitions), counts, comps (the components' sums), out.  lines_from_image_host: all of
    // them; comps serves the edge kernels first and the components' sums afterwards.  The mesh's view calls (fdcm_mesh.hip):
    // keys (views, mesh tables, view records), comps (boxes), pixels (item buffers), parent (large faces), counts, out; with
    // exact visibility comps (the views' pair totals behind the boxes), pixels (tiles), parent (their face lists); with joining
    // labels (a run's lines before joining, their links and chain counts).
    DevBuf pixels, labels, keys, parent, counts, comps, out;
    ~PixelScratch();
    // reserve of a member: under FDCM_POISON a member that this allocated holds the word throughout, by a fill on the null
    // stream, where the calls' kernels and copies run (id: its fdcm_poison_buffer)
    void take(DevBuf& b, size_t bytes, int id);
    // The caller's image or label array where the kernels read it: device memory stays in place; host memory is copied into
    // `pixels` with rows packed, and row_stride becomes width.  The keys, where given, go into `keys`.
    const uint8_t* upload(const uint8_t* host_or_device, int width, int height, int& row_stride, bool on_device, const std::vector<float>* host_keys);
};
// host image -> host labels, blocking, on the null stream of `device`: the hysteresis kernels, or k_edge_labels by e.high
void edge_labels_host(int device, const uint8_t* image, int width, int height, int row_stride, int64_t depth, const fdcm_edge_params& e,
                      bool hysteresis, uint8_t* labels_out);
// implemented in fdcm_lines.hip: label image -> line segments (include/fdcm.h, "line segments from images"); blocking, on the
// null stream of `device`; *lines is malloc'ed (fdcm_lines_free) or null when nothing is kept
void lines_from_labels_host(int device, const uint8_t* labels, int width, int height, bool on_device, int m, const fdcm_line_params& lp,
                            float** lines, int64_t* n_lines);
void lines_from_image_host(int device, const uint8_t* image, int width, int height, int row_stride, bool on_device, int64_t depth,
                           const fdcm_edge_params& e, const fdcm_line_params& lp, float** lines, int64_t* n_lines);
void lines_last_timing(fdcm_lines_timing* out);
// Waits for a queued build (if any) and fills fm->last_build.  run_build only queues the kernels: the search
// that follows is ordered behind them on the same stream and its host-side preparation runs meanwhile.
void finish_build(fdcm_featuremap* fm);
void sweep_order_counts(int64_t* from_history, int64_t* from_proxy);
// implemented in fdcm_search.hip
int64_t search_capacity(const fdcm_templates* t, int64_t n_scene, int64_t maxT, int64_t maxS);
void run_search(fdcm_featuremap* fm, const fdcm_templates* t, const float* scene, int64_t n_scene, int64_t maxT,
                int64_t maxS, int optimizer, int64_t batch, int32_t base, fdcm_match* out_device, fdcm_match** out_host,
                int64_t* n_out);
// sizes the search's workspaces for this template set and scene size, queues nothing
void reserve_search(fdcm_featuremap* fm, const fdcm_templates* t, int64_t n_scene, int64_t maxT, int64_t maxS);
// the searches of this process take the candidates' orientation bins from the host libm (decided once: see fdcm.h)
bool orientation_bins_on_host();
// The one way a call sizes the workspace the seam and the exhaustive calls share (fdcm_host.cpp): search.eval to device_bytes
// and, where the call stages its upload in pinned memory, search.eval_stage to stage_bytes (0: the call has none).  The
// caller holds seam_mutex and the handle has its stream.  Under FDCM_POISON it then waits for the stream and fills the whole
// capacity of both buffers with the word, so the call finds the word wherever it does not write.
void reserve_eval(fdcm_featuremap* fm, size_t device_bytes, size_t stage_bytes);
// implemented in fdcm_seam.hip: minmaxTranslation<Dt3Cpu> / evaluate<Dt3Cpu> batched over templates
void run_minmax(fdcm_featuremap* fm, const float* lines, const int64_t* offsets, int64_t T, const float* align, float* out);
void run_evaluate(fdcm_featuremap* fm, const float* lines, const int64_t* offsets, int64_t T, const float* translations,
                  const int64_t* tr_offsets, float* scores);
// implemented in fdcm_exhaustive.hip: the exhaustive translation search (include/fdcm.h)
void exhaustive_window(fdcm_featuremap* fm, const fdcm_templates* t, int32_t sx, int32_t sy, fdcm_grid* out);
void run_score_map(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, float* out_host,
                   float* out_device);  // rot null: the translations
void run_search_exhaustive(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_grid& g, int k, int32_t base,
                           fdcm_match** out, int64_t* n_out);
void run_search_exhaustive_peaks(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_grid& g, int k, int rx, int ry,
                                 int32_t base, fdcm_match** out, int64_t* n_out);
void exhaustive_rotations_window(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations& rot, int32_t sx, int32_t sy,
                                 fdcm_grid* out);
void run_search_exhaustive_rotations(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations& rot, const fdcm_grid& g,
                                     int k, int rx, int ry, int ra, int wrap, int32_t base, fdcm_match** out, int64_t* n_out);
// rot: null for translations only; job_offsets: n_jobs + 1, or null
void run_best_map(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int penalty, float tau,
                  float* score_out, int32_t* pair_out);
void run_search_exhaustive_detect(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int k,
                                  int rx, int ry, int penalty, float tau, int32_t base, fdcm_match** out, int64_t* n_out);
// boxes_out: 4 k int32, or null
void run_search_exhaustive_detect_nms(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int k,
                                      int permille, int margin, int penalty, float tau, int32_t base, fdcm_match** out,
                                      int32_t* boxes_out, int64_t* n_out);
// boxes_out: 4 max_det int32, or null
void run_search_exhaustive_detect_all(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g,
                                      float max_score, int max_det, int permille, int margin, int penalty, float tau, int32_t base,
                                      fdcm_match** out, int64_t* n_out, int32_t* boxes_out);
// detect_all with the gate by matched fraction (gate: FDCM_GATE_WINNER or FDCM_GATE_ALL); matched_out: max_det floats, or null
void run_search_exhaustive_detect_all_matched(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g,
                                              float max_score, int max_det, int permille, int margin, int penalty, float tau,
                                              float min_matched, int gate, int32_t base, fdcm_match** out, int64_t* n_out,
                                              int32_t* boxes_out, float* matched_out);
// the best map with the gate inside the minimum (include/fdcm.h, "Gate inside the minimum"): any output may be null
void run_best_map_gated(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int penalty, float tau,
                        float min_matched, float* score_out, int32_t* pair_out, float* matched_out);
// poses as run_line_costs'; fractions: n floats
void run_matched_fractions(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                           float* fractions);
void templates_matched_totals(const fdcm_templates* t, float* totals);  // host only: TL per template
// host only: per template the largest sum whose normalised score is <= max_score
void detect_score_bounds(const fdcm_templates* t, int penalty, float tau, float max_score, float* bounds);
float detect_score_bound(float den, float max_score);  // the same for one denominator
// host only: 4 int32 per pair t n + a (rot null: n = 1, the lines as they are)
void templates_footprints(const fdcm_templates* t, const fdcm_rotations* rot, int margin, int32_t* boxes_out);
void lines_footprints(const float* lines, const int64_t* offsets, int64_t T, const fdcm_rotations* rot, int margin, int32_t* boxes_out);
// host only (include/fdcm.h, "Hull footprints"): the hull shapes of every pair; areas and spans may be null
void templates_footprint_spans(const fdcm_templates* t, const fdcm_rotations* rot, int margin, int64_t* row_offsets, int64_t* areas,
                               int32_t* spans);
void lines_footprint_spans(const float* lines, const int64_t* offsets, int64_t T, const fdcm_rotations* rot, int margin,
                           int64_t* row_offsets, int64_t* areas, int32_t* spans);
// host only: throws when a dense detection call on the hull set t would need a span table of more than 2^26 rows
void check_hull_rows(const fdcm_templates* t, const fdcm_rotations* rot, int margin);
void run_search_exhaustive_windows(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_pose_window* jobs,
                                   int64_t n_jobs, int sx, int sy, int k, int32_t base, fdcm_match** out, int64_t* n_out,
                                   int64_t* job_offsets);
// detections over pose windows (include/fdcm.h): boxes_out, matched_out (max_det entries each) and jobs_out may be null
void run_search_exhaustive_detect_windows(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot,
                                          const fdcm_pose_window* jobs, int64_t n_jobs, int sx, int sy, float max_score, int max_det,
                                          int permille, int margin, int penalty, float tau, float min_matched, int gate, int32_t base,
                                          fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out, int32_t* jobs_out);
// objects (include/fdcm.h, "Objects"): objects has T checked entries in [0, n_objects); max_score has n_objects floats, min_matched
// n_objects floats or is null (all 0); the outputs are the siblings', the best map's planes n_objects times as large
void run_best_map_objects(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g, int penalty,
                          float tau, const int32_t* objects, int n_objects, const float* min_matched, float* score_out, int32_t* pair_out,
                          float* matched_out);
void run_search_exhaustive_detect_objects(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid& g,
                                          const int32_t* objects, int n_objects, const float* max_score, const float* min_matched,
                                          int max_det, int permille, int cross, int margin, int penalty, float tau, int gate, int32_t base,
                                          fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out);
void run_search_exhaustive_detect_windows_objects(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot,
                                                  const fdcm_pose_window* jobs, int64_t n_jobs, int sx, int sy, const int32_t* objects,
                                                  int n_objects, const float* max_score, const float* min_matched, int max_det,
                                                  int permille, int cross, int margin, int penalty, float tau, int gate, int32_t base,
                                                  fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out,
                                                  int32_t* jobs_out);
// poses: n x (tmpl, a, x, y), checked; *costs is malloc'ed; offsets: n + 1
void run_line_costs(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                    float** costs, int64_t* offsets);
// Match lists (include/fdcm.h, "Match lists"), implemented in fdcm_exhaustive.hip: the arguments are checked.
// A record list as every device call on one takes it: n records on the host or (on_device) on the handle's device, whose
// tmpl_idx count from base.
struct MatchList { const fdcm_match* rec; int64_t n; bool on_device; int32_t base; };
struct MatchesDetect {
    float max_score;
    int max_detections, overlap_permille, margin, penalty;
    float tau, min_matched;
    int rescore;
};
// "Match lists: objects and hull shapes".  The objects of the detect call with objects, which honours the set's kind of
// footprint (objects: T checked labels; max_score: G floats; min_matched: G floats or null; det's max_score and min_matched
// are not read).
struct MatchesObjectsIn {
    const int32_t* objects;
    int G;
    const float* max_score;
    const float* min_matched;
    int cross;
};
// The shapes call's outputs: the table of every valid admissible record with lines from the device kernel: row_offsets n + 1,
// areas n or null, spans 2 per row or null.
struct MatchesShapesOut {
    int margin;
    int64_t* row_offsets;
    int64_t* areas;
    int32_t* spans;
};
// What a device call on a match list asks of run_matches; the callers fill the fields by name.  det null and shapes null: the
// verify call.  det: a detect call, with `objects` or without.  shapes (det null): the shapes call.
struct MatchesIn {
    MatchList list{};
    const MatchesDetect* det = nullptr;
    const MatchesObjectsIn* objects = nullptr;
    struct { float *scores, *fractions, *costs; } verify{};  // n floats each, costs n x max_lines floats; each may be null
    // *out acquired (max_detections entries at most), *n_out its count; indices, boxes (4 per entry), matched: max_detections, or null
    struct { fdcm_match** out; int64_t* n_out; int32_t *indices, *boxes; float* matched; } detect{};
    const MatchesShapesOut* shapes = nullptr;
};
// matches_footprints: host only, 4 int32 per record.
void matches_footprints(const fdcm_templates* t, const fdcm_match* matches, int64_t n, int32_t base, int margin, int32_t* boxes_out);
// host only: the hull shape of every record, lines_footprint_spans' layout (an invalid record: no rows)
void matches_footprint_spans(const fdcm_templates* t, const fdcm_match* matches, int64_t n, int32_t base, int margin, int64_t* row_offsets,
                             int64_t* areas, int32_t* spans);
void run_matches(fdcm_featuremap* fm, const fdcm_templates* t, const MatchesIn& in);
// "Match lists: refinement": every record's window of (delta rotation, dx, dy) searched on the device; out: n records on the host
// or (out_on_device) on the handle's device, which may be the list's; pose_out: n x 3 on the host, or null.
void run_matches_refine(fdcm_featuremap* fm, const fdcm_templates* t, const MatchList& m, const fdcm_rotations* rot, int32_t centre,
                        int32_t hx, int32_t hy, int32_t sx, int32_t sy, fdcm_match* out, bool out_on_device, int32_t* pose_out);
// the bins of every posed line from the host libm, [record][max_lines], where fdcm_orientation_bins_mode() is 1 (else empty); the
// handle has its stream
void matches_host_bins(fdcm_featuremap* fm, const fdcm_templates* t, const MatchList& m, std::vector<unsigned short>& bins);
// Scene coverage (include/fdcm.h, "Scene coverage").  What prepare_pairs yields for the distinct pairs of a pose list, in the
// plain form fdcm_coverage.hip takes: pair u = find(tmpl * n_rot + a) has the lines [line0[u], line0[u] + nl[u]) -- the (rotated)
// end points and the bin k_line_costs reads --, its admissible translations adm[5 u ..] = any, x0, x1, y0, y1 and its footprint
// foot[4 u ..] = x0, y0, x1, y1 at the call's margin.
struct CoverageLine { float x1, y1, x2, y2; int32_t bin; };
struct CoveragePairs {
    std::vector<int64_t> key;  // ascending
    std::vector<CoverageLine> lines;
    std::vector<int> line0, nl;
    std::vector<int32_t> adm, foot;
    size_t find(int64_t k) const { return (size_t)(std::lower_bound(key.begin(), key.end(), k) - key.begin()); }
};
// implemented in fdcm_exhaustive.hip (host only; n > 0 checked poses)
void coverage_pairs(const fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                    int margin, CoveragePairs& out);
// implemented in fdcm_coverage.hip: the arguments are checked (fdcm_capi.cpp), the frame (bx, by) included; counts: 2 n int32 on
// the host; residual: width * height bytes where the labels are (host, or the handle's device), or null
void run_scene_coverage(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                        const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                        const fdcm_coverage_params& params, int32_t* counts, uint8_t* residual);
// Scene selection (include/fdcm.h, "Scene selection"), implemented in fdcm_coverage.hip with run_scene_coverage's preparation
// and buffers: the arguments are checked; selected: max_selected int32 and counts: 3 max_selected int32 on the host, *n_out the
// number accepted; residual as above
void run_scene_select(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                      const fdcm_templates* t, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                      const fdcm_coverage_params& params, const fdcm_select_params& sel, int32_t* selected, int32_t* counts,
                      int64_t* n_out, uint8_t* residual);
// Scene coverage and selection of match records (include/fdcm.h, "Match lists: scene coverage and selection"), implemented in
// fdcm_coverage.hip: the siblings' arguments with a record list in place of the poses; the table is made on the device
// (k_matches_table), in parts under FDCM_COVERAGE_PART.  counts: 2 n int32 on the host.
void run_matches_coverage(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                          const fdcm_templates* t, const MatchList& m, const fdcm_coverage_params& params, int32_t* counts,
                          uint8_t* residual);
void run_matches_select(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                        const fdcm_templates* t, const MatchList& m, const fdcm_coverage_params& params, const fdcm_select_params& sel,
                        int32_t* selected, int32_t* counts, int64_t* n_out, uint8_t* residual);
// "Match lists: pose fit": every record fitted to the edge pixels it explains, the records staying on the device between the
// passes; out: n records on the host or (out_on_device) on the handle's device, which may be the list's; info_out: 4 n int32,
// rms_out: 2 n floats, on the host, or null.
void run_matches_fit(fdcm_featuremap* fm, const uint8_t* labels, int width, int height, bool on_device, int bx, int by,
                     const fdcm_templates* t, const MatchList& m, const fdcm_coverage_params& params, const fdcm_fit_params& fit,
                     fdcm_match* out, bool out_on_device, int32_t* info_out, float* rms_out);
// implemented in fdcm_tail.hip
void run_topk(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_match* matches_device, int64_t n, int32_t base,
              int penalty, float tau, int64_t k, fdcm_match** out, int64_t* n_out);
void run_topk_device(fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_match* matches_device, int64_t n, int32_t base,
                     int penalty, float tau, int64_t k, fdcm_match* out_device);
// sizes run_topk_device's workspaces for T templates and n matches (at most), queues nothing
void reserve_topk(fdcm_featuremap* fm, int64_t T, int64_t n);
// records to the host without a copy command (a kernel writes into the mapped pinned destination); queued on st
void records_to_host(hipStream_t st, const fdcm_match* src_device, int64_t n, fdcm_match* dst_pinned);
// the valid records of n_blocks fixed-capacity blocks (count in the trailing record) into a pooled pinned array; waits for st
void blocks_to_host(hipStream_t st, const void* blocks_device, int32_t n_blocks, int64_t cap, fdcm_match** out, int64_t* n_out);
// the device tail's total order on float bit patterns (-0 < +0, NaNs at the ends), for host-side merges
inline unsigned ordered_key_host(float f) {
    unsigned u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the reference's line files (fdcm_lineio.cpp); lines_read hands out malloc'ed memory
void lines_read(const char* path, float** out, int64_t* n_out);
void lines_write(const char* path, const float* lines, int64_t n);
// compute units of a device (cached; fdcm_capi.cpp)
int device_cus(int device);
// pooled pinned host buffers for match arrays returned to the caller (fdcm_host.cpp)
fdcm_match* result_acquire(size_t bytes);
void result_release(fdcm_match* m);
}  // namespace fdcm
