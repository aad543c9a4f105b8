/* fdcm.h -- C ABI of libfdcm_hip.so: the MI355X (gfx950) engine for OpenFDCM's hot path.
 *
 * The reference (Innoptech/OpenFDCM v0.10.0) has no C ABI or plug-in loader: its extension point
 * is a C++ type deriving from FeatureMapInstance (modules/matching/include/openfdcm/matching/
 * featuremap.h:11-15) with getFeatureSize / minmaxTranslation / evaluate specialised
 * (featuremap.h:27-52), driven by search<DefaultMatch> (modules/matching/src/matchstrategies/
 * defaultmatch.cpp:32-89) and optimize<BatchOptimize> (modules/matching/src/optimizestrategies/
 * batchoptimize.cpp:6-123), and exposed to Python by modules/python/src/matching.cpp.  These
 * entry points are what a binding for that path would call; INTEGRATION.md shows the stubs.
 *
 * Conventions: every function returns 0 on success and a negative FDCM_E* code on failure;
 * fdcm_last_error() returns a thread-local message.  No exception crosses the boundary.  Inputs
 * are caller-owned host buffers (plain pointers + counts) unless a parameter says "device".
 * Outputs allocated by the library are released with the matching *_free.  Calls block until the
 * result is complete and are safe to make with the Python GIL released; the one exception is
 * fdcm_featuremap_build / _rebuild, which return once the build is queued on the handle's HIP stream
 * (every later call on the handle that touches the volume -- search, slice, device_volume, timing,
 * free -- is ordered behind it or waits for it, so a kernel failure is reported by that call).  Handles are
 * thread-compatible (one caller at a time per handle).
 *
 * Line arrays are the reference's LineArray (math.h:66): 4 x N float32, column-major, i.e. N
 * consecutive records x1,y1,x2,y2.
 */
#ifndef FDCM_H
#define FDCM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDCM_OK 0
#define FDCM_EINVAL (-1)   /* bad argument */
#define FDCM_EHIP (-2)     /* a HIP runtime call failed (no device, out of memory, launch error) */
#define FDCM_EINTERNAL (-3)

/* core::Distance, modules/core/include/openfdcm/core/imgproc.h:148 */
enum fdcm_distance { FDCM_L2 = 0, FDCM_L2_SQUARED = 1, FDCM_L1 = 2 };
/* optimiser strategies: defaultoptimize.cpp:6-93, batchoptimize.cpp:6-123, indulgentoptimize.cpp:6-102.
 * For FDCM_INDULGENT_OPTIMIZE the batch_size argument of the search calls is the number of passthroughs (it
 * does not change the result: a passed-through score is re-scored at the same translation). */
enum fdcm_optimizer { FDCM_DEFAULT_OPTIMIZE = 0, FDCM_BATCH_OPTIMIZE = 1, FDCM_INDULGENT_OPTIMIZE = 2 };
/* penalty strategies: defaultpenalty.cpp:29-58, exponentialpenalty.cpp:34-64 */
enum fdcm_penalty { FDCM_DEFAULT_PENALTY = 0, FDCM_EXPONENTIAL_PENALTY = 1 };

/* matching::Match, matchstrategy.h:35-44; transform is the 2x3 matrix in row-major order. */
typedef struct fdcm_match {
    int32_t tmpl_idx;
    float score;
    float transform[6];
} fdcm_match;

typedef struct fdcm_featuremap fdcm_featuremap; /* replaces Dt3Cpu, dt3cpu.h:46-63 */
typedef struct fdcm_templates fdcm_templates;   /* a std::vector<LineArray> resident in HBM */

typedef struct fdcm_featuremap_info {
    int64_t width, height; /* getFeatureSize(): Size(x = W, y = H); square when built from scene lines (dt3cpu.cpp:113-115), any
                            * shape when adopted from slices or built from an image or labels */
    int64_t depth;         /* number of orientation slices actually built (distinct keys) */
    float scene_translation[2]; /* getSceneTranslation() */
    int32_t distance;
    float dt3_coeff, padding;
} fdcm_featuremap_info;

/* Per-stage device times of the last build, in milliseconds (HIP events on the build stream). */
typedef struct fdcm_build_timing {
    float total_ms;     /* host preparation + the kernels' span on the device */
    float seeds_ms;     /* K0: rasterise scene lines into the seed bitmap (feature sizes above 4096 only: below, K1 draws the seeds itself);
                         * image builds: the edge-label kernel */
    float pass1_ms;     /* K1: 1-D distance along y */
    float pass2_ms;     /* K2: in-place lower-envelope pass along x (L2/L2^2) or L1 sweeps */
    float propagate_ms; /* K3: orientation propagation (+ sqrt for L2) */
    float integral_ms;  /* K4: directional line integral */
    float span_ms;      /* the kernels' span on the device alone (first to last event; 0 without events) */
} fdcm_build_timing;

typedef struct fdcm_search_timing {
    float total_ms;  /* the search's span on the device: kernels + download of the matches */
    float kernel_ms; /* candidate generation + optimisation + compaction on the device, from the event that precedes them on the
                      * handle's stream.  A handle that has the GPU to itself runs the search's preparation (scene upload,
                      * candidate pairs, work list) on a second stream beside a build that is still running: the part of it
                      * that overlaps the build is then not inside kernel_ms / total_ms */
    int64_t candidates;
    int64_t evaluations; /* translations scored by the reference rule (kept + rejected batches), summed over the candidates;
                          * every translation counts once.  For DefaultOptimize and BatchOptimize that is the number of the
                          * rule's scorings.  IndulgentOptimize(p)'s rule scores a translation it rejects p more times at the
                          * same place before it gives up; those repeats read nothing new and are not counted, so the value is
                          * the number of scorings of IndulgentOptimize(0), which walks and returns the same */
} fdcm_search_timing;

const char* fdcm_last_error(void);
const char* fdcm_version(void);

int fdcm_device_count(int* count);
int fdcm_set_device(int device); /* device used by handles created afterwards on this thread */
int fdcm_get_device(int* device); /* the device fdcm_set_device selected on this thread (0 by default) */

/* ---- DT3 feature map: buildCpuFeaturemap<D>, dt3cpu.h:174-234; Python build_cpu_featuremap,
 *      modules/python/src/matching.cpp:116-130 ---- */
int fdcm_featuremap_build(const float* scene_lines, int64_t n_lines, int64_t depth, float dt3_coeff, float padding,
                          int distance, fdcm_featuremap** out);
/* Rebuild into an existing handle (same depth/distance parameters), reusing its HBM when the
 * feature size allows: the steady-state per-frame call. */
int fdcm_featuremap_rebuild(fdcm_featuremap* fm, const float* scene_lines, int64_t n_lines);
int fdcm_featuremap_free(fdcm_featuremap* fm);
int fdcm_featuremap_get_info(const fdcm_featuremap* fm, fdcm_featuremap_info* info);
int fdcm_featuremap_keys(const fdcm_featuremap* fm, float* keys /* depth floats, ascending */);
/* Slice k as the reference stores it: RawImage<float>(H, W) column-major, (y,x) at x*H + y. */
int fdcm_featuremap_slice(const fdcm_featuremap* fm, int64_t k, float* out_host);
/* Whole volume on the device (read-only view, valid until free/rebuild).  Layout: 4 neighbouring x are
 * interleaved so that a 64-byte sector holds 4 x by 4 y pixels (the search's gathers step about one pixel per
 * translation in any direction), and slices are a little longer than their pixels (power-of-two slice
 * strides would put one pixel of every slice on the same memory channel): pixel (k, x, y) is element
 * k * floats_per_slice + ((x/4) * H + y) * 4 + x%4, floats_per_slice from fdcm_featuremap_device_volume_stride. */
int fdcm_featuremap_device_volume(const fdcm_featuremap* fm, const float** device_ptr);
int fdcm_featuremap_device_volume_stride(const fdcm_featuremap* fm, int64_t* floats_per_slice);
int fdcm_featuremap_last_timing(const fdcm_featuremap* fm, fdcm_build_timing* t);
/* The device-side times of fdcm_build_timing / fdcm_search_timing cost a HIP event between every two kernels of the build and
 * around the search (3 - 5 us each on a blocking frame).  on = 1 (default): per-stage times.  on = 2: events around the
 * build and around the search only (total_ms and the search's kernel_ms; the stage fields are 0).  on = 0: no events: the
 * timings carry the host time and the counters (candidates, evaluations) only, every device time is 0.
 * No counterpart in the reference (it has no timers). */
int fdcm_featuremap_stage_timing(fdcm_featuremap* fm, int on);
/* Dt3Cpu(dt3map, sceneTranslation, featureSize) constructor (dt3cpu.h:55-58): adopt caller slices. */
int fdcm_featuremap_from_slices(const float* keys, int64_t depth, const float* volume_host /* [k][x][y] */,
                                int64_t width, int64_t height, const float scene_translation[2],
                                fdcm_featuremap** out);
/* Test hook: stop the build after stage 1 (distance transform), 2 (propagation) or 3 (all). */
int fdcm_featuremap_build_staged(const float* scene_lines, int64_t n_lines, int64_t depth, float dt3_coeff,
                                 float padding, int distance, int stop_after, fdcm_featuremap** out);

/* ---- feature maps from images: oriented edge pixels as DT3 seeds.  No counterpart in the reference, whose only seed
 *      source is a list of scene lines; these definitions are the project's own.
 *
 * Image: uint8, `height` rows of `width` pixels, `row_stride` >= width bytes between rows; I(x, y) is clamped to the image
 * (replicate border) for the gradient.
 * Gradient (integer Sobel):  gx = [I(x+1,y-1) + 2 I(x+1,y) + I(x+1,y+1)] - [the same at x-1],
 *                            gy = [I(x-1,y+1) + 2 I(x,y+1) + I(x+1,y+1)] - [the same at y-1],  m2 = gx^2 + gy^2 (<= 2 * 1020^2).
 * Direction for thinning, with a = |gx|, b = |gy| (12/29 ~ tan 22.5 deg):  29 b < 12 a: d = (1, 0);  29 a < 12 b: d = (0, 1);
 *   otherwise d = (1, 1) when (gx >= 0) == (gy >= 0), else d = (1, -1).
 * Edge pixel p: m2(p) >= threshold^2 (1 <= threshold <= 1442), m2(p) > m2(p - d) and m2(p) >= m2(p + d); a neighbour outside
 *   the image has m2 = 0.  (Of a two-pixel plateau one pixel wins.)  Smoothing, hysteresis and a minimum chain length are optional:
 *   the _ex entry points below.
 * Orientation label: the edge's tangent (-gy, gx): dx = float(-gy) (the integer is negated, so gy = 0 gives +0), dy = float(gx),
 *   angle = atanf(dy / dx) as getAngle (math.h:295-299; IEEE division, dx = 0 gives +-pi/2), label = closestOrientation
 *   (dt3cpu.h:93-114) over the m distinct keys that a line build of the same depth makes.
 * Label image: one byte per pixel, rows of `width` bytes without gaps; 0 .. m-1 a slice, any value >= m (canonically 255) no
 *   edge -- so m <= 255, and a depth above 255 is FDCM_EINVAL.
 * Feature map of an image, with b = border >= 0: size (width + 2b, height + 2b), scene translation (b, b), padding reported as
 *   0; pixel (x + b, y + b) of slice label(x, y) is a seed, stage 1 is the distance transform of every slice's 0 / FLT_MAX
 *   image, stages 2 and 3 are the line build's (distanceTransform from the drawn image on, propagateOrientation, lineIntegral).
 *   Both sides of the map are at most 4096.  A slice without seeds, or a whole image without edges, is FLT_MAX throughout
 *   stage 1 (its square root for FDCM_L2).
 * on_device = 1: the pointer is memory of the current device; it is read in place while the build runs, so its content must
 *   be complete when the call is made and stay untouched until a later call on the handle has waited for the build.
 * Argument errors (NULL pointers, size 0 or above 4096, row_stride < width, negative border, threshold outside [1, 1442],
 * too many keys) are FDCM_EINVAL before any GPU work.  Like fdcm_featuremap_build, the builds return once queued. ---- */
/* image -> label image; host in, host out, computed on the GPU.  depth >= 1. */
int fdcm_edge_labels(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int64_t depth, int threshold,
                     uint8_t* labels_out);
int fdcm_featuremap_build_image(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device,
                                int threshold, int64_t border, int64_t depth, float dt3_coeff, int distance,
                                fdcm_featuremap** out);
/* The steady-state call: any handle, whatever its last build took its seeds from (its depth, coefficient and distance stay;
 * a handle made from an image has padding 0 for a later build from lines). */
int fdcm_featuremap_rebuild_image(fdcm_featuremap* fm, const uint8_t* image, int64_t width, int64_t height, int64_t row_stride,
                                  int on_device, int threshold, int64_t border);
/* The same from a label image of the caller's own edge detector. */
int fdcm_featuremap_build_labels(const uint8_t* labels, int64_t width, int64_t height, int on_device, int64_t border,
                                 int64_t depth, float dt3_coeff, int distance, fdcm_featuremap** out);
int fdcm_featuremap_rebuild_labels(fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int on_device,
                                   int64_t border);
/* ---- edges with smoothing, hysteresis and a minimum chain length.  Integer arithmetic up to the divide the label has.
 * Smoothing: S = I for smooth = 0;  S(x,y) = (sum_ij w(i) w(j) I(x+i, y+j) + 8) >> 4 with w = [1 2 1] for smooth = 1;
 *   S = (sum ... + 128) >> 8 with w = [1 4 6 4 1] for smooth = 2; I clamped to the image (replicate border).  S is a uint8
 *   image of the same size, and the definitions above apply to S in place of I: the gradient reads S clamped to the image
 *   (the smoothed pixel at the clamped coordinate, not the smoothing of an extended image).  m2 <= 2 * 1020^2 still holds.
 * Candidate: a pixel that passes the thinning rule above (m2(p) > m2(p - d), m2(p) >= m2(p + d), m2 = 0 outside the image)
 *   with m2 >= low^2.  Strong: a candidate with m2 >= high^2.  Component: a maximal 8-connected set of candidates.
 * Edge pixel: a candidate whose component holds at least one strong pixel and at least min_pixels candidates.  Its label is
 *   the one above (tangent (-gy, gx) of S's gradient, atanf, closestOrientation); everything else is 255.
 * smooth = 0, low = high = t, min_pixels = 1 is exactly fdcm_edge_labels(threshold = t), byte for byte.  The result is a
 *   set: it does not depend on the order in which the GPU visits or merges pixels.
 * Argument errors besides their siblings': params NULL, smooth outside {0, 1, 2}, low < 1, high > 1442, low > high,
 * min_pixels < 1: FDCM_EINVAL before any GPU work.  The builds return once queued: the components are resolved on the device. ---- */
typedef struct fdcm_edge_params {
    int32_t smooth;      /* 0, 1 or 2 */
    int32_t low, high;   /* 1 <= low <= high <= 1442 */
    int32_t min_pixels;  /* >= 1 */
} fdcm_edge_params;
int fdcm_edge_labels_ex(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int64_t depth,
                        const fdcm_edge_params* params, uint8_t* labels_out);
int fdcm_featuremap_build_image_ex(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device,
                                   const fdcm_edge_params* params, int64_t border, int64_t depth, float dt3_coeff, int distance,
                                   fdcm_featuremap** out);
int fdcm_featuremap_rebuild_image_ex(fdcm_featuremap* fm, const uint8_t* image, int64_t width, int64_t height,
                                     int64_t row_stride, int on_device, const fdcm_edge_params* params, int64_t border);
/* Test hook: stop the image build after stage 1, 2 or 3. */
int fdcm_featuremap_build_image_staged(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device,
                                       int threshold, int64_t border, int64_t depth, float dt3_coeff, int distance,
                                       int stop_after, fdcm_featuremap** out);

/* ---- image pyramid: the image reduced by 2^level on the device, and the feature map of a level, for coarse-to-fine detection
 *      (Python: exhaustive_detect_pyramid).  All integer.
 * Level images: P_0 = I, the caller's image.  W_(l+1) = (W_l + 1) >> 1, H_(l+1) likewise.  P_(l+1)(x, y) = S2(P_l)(2x, 2y),
 *   S2 the smooth = 2 image above: (sum_ij w(i) w(j) P_l(clamp(2x+i), clamp(2y+j)) + 128) >> 8 with w = [1 4 6 4 1] and the
 *   coordinates clamped to P_l (replicate border).  Pixel x of level l is pixel 2^l x of level 0: there is no half-pixel shift.
 *   0 <= level <= 12; a side of 1 stays 1.
 * Feature map of level l: by definition fdcm_featuremap_build_image_ex of the image P_l with the same params, border, depth,
 *   dt3_coeff and distance -- border in level-l pixels, size (W_l + 2b, H_l + 2b), scene translation (b, b).  level = 0 is
 *   that call, byte for byte.  The levels between live in a workspace of the handle (two buffers, level l + 1 made from level
 *   l by one kernel) and are freed with it.  The input sizes stay within 1 .. 4096.
 * Lifting a level-l record to level 0.  Search the level-l map with every template end point and pivot multiplied by 2^-l
 *   (exact in float32).  Every product and sum of M_a (the record's rotation part and its offset m = p - R p) is then the
 *   level-0 value times 2^-l exactly -- a power of two scales every operand of every rounding alike, and no underflow is
 *   reachable for |coordinate| < 2^24 -- so m_l = 2^-l m, and fl(m_l.x + t_l.x) * 2^l = fl(m.x + 2^l t_l.x).  A level-l
 *   record whose transform[2] and transform[5] are multiplied by 2^l is therefore bit for bit the record a level-0 search
 *   emits for the translation 2^l t_l and the same angle.  Angles, orientation bins and caps given as one scalar follow
 *   exactly: dy / dx is unchanged and lengths are multiplied by 2^-l.  Scores do NOT carry over between levels.
 * Argument errors besides the _ex siblings': level outside [0, 12], a size outside [1, 4096], NULL image, out or params:
 *   FDCM_EINVAL before any GPU work.  Like their siblings the builds return once queued, and with on_device = 1 the image is
 *   read in place while they run. ---- */
/* The size of level `level` of a width x height image.  Host only. */
int fdcm_image_pyramid_size(int64_t width, int64_t height, int32_t level, int64_t* w_out, int64_t* h_out);
/* P_level into out: W_l * H_l bytes, rows contiguous, host memory or (out_on_device = 1) memory of the current device.  Level
 * 0 copies the image with its rows packed.  Blocks until out is written. */
int fdcm_image_pyramid_level(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device,
                             int32_t level, uint8_t* out, int out_on_device);
int fdcm_featuremap_build_image_level(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device,
                                      int32_t level, const fdcm_edge_params* params, int64_t border, int64_t depth,
                                      float dt3_coeff, int distance, fdcm_featuremap** out);
int fdcm_featuremap_rebuild_image_level(fdcm_featuremap* fm, const uint8_t* image, int64_t width, int64_t height,
                                        int64_t row_stride, int on_device, int32_t level, const fdcm_edge_params* params,
                                        int64_t border);

/* ---- the feature-map plug-in seam: what a FeatureMapInstance specialises besides getFeatureSize
 *      (featuremap.h:27-52; FeatureMapModel<T> forwards to them, featuremap.h:80-92) and what every optimiser of the
 *      reference calls (defaultoptimize.cpp:26,49-64, batchoptimize.cpp:27,58-62).  With these three a reference
 *      build can wrap a handle in its own type-erased FeatureMap and run ANY of its optimisers on the HBM volume
 *      (INTEGRATION.md).  Both are batched: one kernel launch per call. ---- */
/* minmaxTranslation<Dt3Cpu>, dt3cpu.cpp:30-75,119-124: the admissible multiplier interval {negative, positive} of
 * align_vec for a template (4 x n_lines, in scene coordinates: the feature map adds its scene translation itself).
 * {inf, inf} for a zero align_vec, {NaN, NaN} when the template's bounding box starts outside the feature map. */
int fdcm_featuremap_minmax_translation(const fdcm_featuremap* fm, const float* tmpl_lines, int64_t n_lines,
                                       const float align_vec[2], float out_minmax[2]);
/* the same for n_templates templates (lines concatenated, line_offsets in lines) with one align_vec each;
 * out_minmax: 2 floats per template */
int fdcm_featuremap_minmax_translation_batch(const fdcm_featuremap* fm, const float* tmpl_lines, const int64_t* line_offsets,
                                             int64_t n_templates, const float* align_vecs, float* out_minmax);
/* evaluate<Dt3Cpu>, dt3cpu.cpp:126-179: scores[t][j] = sum_i |I_bin(i)(p1_i + T + tr_j) - I_bin(i)(p2_i + T + tr_j)| for
 * every template t and each of its translations tr_j (x, y pairs; translation_offsets in translations, n_templates + 1
 * entries), T = the scene translation, coordinates truncated like cast<int>(), terms added in Eigen's sum() order:
 * the reference's bits.  scores_out: one float per translation, in input order.  A translation that puts an end
 * point outside the feature map scores NaN (the reference reads out of bounds there, dt3cpu.cpp:166-167). */
int fdcm_featuremap_evaluate(const fdcm_featuremap* fm, const float* tmpl_lines, const int64_t* line_offsets,
                             int64_t n_templates, const float* translations, const int64_t* translation_offsets,
                             float* scores_out);

/* ---- templates: the `templates` argument of search(), kept resident in HBM ---- */
int fdcm_templates_create(const float* lines, const int64_t* offsets /* n_templates+1, in lines */,
                          int64_t n_templates, fdcm_templates** out);
int fdcm_templates_free(fdcm_templates* t);
int fdcm_templates_count(const fdcm_templates* t, int64_t* n_templates, int64_t* n_lines);
/* getTemplateLengths, math.h:319-324 */
int fdcm_templates_lengths(const fdcm_templates* t, float* lengths /* n_templates */);

/* ---- search<DefaultMatch> with DefaultSearch(max_tmpl_lines, max_scene_lines) and
 *      DefaultOptimize / BatchOptimize(batch_size): defaultmatch.cpp:32-89 ----
 * Returns the matches in the reference's positional order (template order x search-combination
 * order x 2 alignments, candidates without a value skipped).  tmpl_idx is offset by
 * tmpl_index_base (0 for a single GPU; the shard's first template for sharded runs).
 * The limits behave as the reference's min(): max_tmpl_lines above a template's line count means all of its
 * lines (defaultsearch.cpp:38, size_t), max_scene_lines above n_scene_lines means every scene line
 * (defaultsearch.h:42-46; the reference's int casts make values >= 2^31 undefined there, here they also mean
 * "every line"). */
int fdcm_search(const fdcm_featuremap* fm, const fdcm_templates* templates, const float* scene_lines,
                int64_t n_scene_lines, int64_t max_tmpl_lines, int64_t max_scene_lines, int optimizer,
                int64_t batch_size, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out);
/* Same, results left on the device: out_device must hold fdcm_search_capacity() records;
 * *n_out receives the count (host).  For RCCL gathers without a host round trip. */
int fdcm_search_capacity(const fdcm_templates* templates, int64_t n_scene_lines, int64_t max_tmpl_lines,
                         int64_t max_scene_lines, int64_t* capacity);
int fdcm_search_device(const fdcm_featuremap* fm, const fdcm_templates* templates, const float* scene_lines,
                       int64_t n_scene_lines, int64_t max_tmpl_lines, int64_t max_scene_lines, int optimizer,
                       int64_t batch_size, int32_t tmpl_index_base, fdcm_match* out_device, int64_t* n_out);
int fdcm_search_last_timing(const fdcm_featuremap* fm, fdcm_search_timing* t);
void fdcm_matches_free(fdcm_match* m); /* match arrays are pinned host buffers from a pool inside the library */
/* Concatenate the valid records of n_blocks fixed-capacity blocks that sit back to back in device memory into a
 * library-owned host array, in block order.  A block is capacity_records + 1 records; the first int64 of its last
 * record holds its record count -- what a gather of fdcm_search_device outputs assembles when every rank appends its
 * count that way (openfdcm_amd/dist.py).  Queued on `stream` (a hipStream_t of the current device, NULL = the default
 * stream) behind whatever filled the blocks there; returns when the array is complete (a kernel writes it into pinned
 * memory: no copy command).  Release with fdcm_matches_free. */
int fdcm_blocks_to_host(const void* blocks_device, int32_t n_blocks, int64_t capacity_records, void* stream,
                        fdcm_match** out, int64_t* n_out);

/* ---- template shards over several GPUs of one node, from ONE process (the reference's own
 *      parallel seam is the per-candidate task loop, batchoptimize.cpp:102-114) ----
 * The template list is cut into contiguous index ranges, one per device; every device rebuilds the DT3 volume itself
 * from the scene lines (a long-lived host thread per device runs rebuild -> search) and the match records -- in top-k mode the
 * k best of every shard (penalise + stable sort on each device) -- travel to the first device in ONE grouped RCCL
 * send/recv per frame with exact sizes; no count exchange is needed because all shards live in this process.
 * fdcm_sharded_search returns what fdcm_search returns for the whole list on one device (same records, same order);
 * fdcm_sharded_search_topk returns what fdcm_topk returns for it.  devices = NULL means devices 0..n_devices-1.
 * RCCL (librccl.so.1) is bound at run time, only when n_devices > 1 or FDCM_SHARDED_ALWAYS_COLLECTIVE is set (then a
 * single shard also sends its records to itself through RCCL: a test hook for one-GPU machines).  Every entry point
 * leaves the caller's current device (the library's and HIP's) as it found it. */
#define FDCM_SHARDED_ALWAYS_COLLECTIVE 1
/* Test hook for one-GPU machines: `devices` may name a device more than once.  Shards that live on the first shard's
 * device hand their records over with device copies (RCCL cannot put one device into a communicator twice), everything
 * else -- ranges, one worker per shard and frame slot, offsets into the gathered array, the top-k merge -- is the
 * multi-device code. */
#define FDCM_SHARDED_ALLOW_SAME_DEVICE 2
typedef struct fdcm_sharded fdcm_sharded;
int fdcm_sharded_create(const int* devices, int n_devices, const float* tmpl_lines, const int64_t* offsets /* n_templates+1 */,
                        int64_t n_templates, int64_t depth, float dt3_coeff, float padding, int distance, int flags,
                        fdcm_sharded** out);
int fdcm_sharded_search(fdcm_sharded* s, const float* scene_lines, int64_t n_scene_lines, int64_t max_tmpl_lines,
                        int64_t max_scene_lines, int optimizer, int64_t batch_size, fdcm_match** out, int64_t* n_out);
/* penalty: -1 (none), FDCM_DEFAULT_PENALTY or FDCM_EXPONENTIAL_PENALTY(tau); at most k records per shard cross the links */
int fdcm_sharded_search_topk(fdcm_sharded* s, const float* scene_lines, int64_t n_scene_lines, int64_t max_tmpl_lines,
                             int64_t max_scene_lines, int optimizer, int64_t batch_size, int penalty, float tau, int64_t k,
                             fdcm_match** out, int64_t* n_out);
/* Frames in flight (like fdcm_pipeline_* on one device): the engine keeps n_frames frame slots per device, each with its
 * own feature map and a long-lived host thread.  fdcm_sharded_submit copies the scene lines, hands the frame to the
 * workers of every device and returns a ticket (tickets count up from 0; ticket t uses slot t % n_frames, so at most
 * n_frames tickets may be outstanding); fdcm_sharded_wait blocks until the frame is complete on every device, runs its
 * exchange and returns exactly what the blocking call returns -- while the workers compute the frames submitted
 * after it.  fdcm_sharded_search / _search_topk are submit + wait.  One caller thread at a time per engine; n_frames
 * is 1 after create and may be changed (1..16) while no frame is in flight. */
int fdcm_sharded_set_frames_in_flight(fdcm_sharded* s, int n_frames);
/* What the devices share out.  FDCM_SHARD_TEMPLATES (the default): every frame runs on every device,
 * each over its contiguous template range, one exchange per frame -- the way to shorten ONE frame, bounded by the build that
 * every device repeats.  FDCM_SHARD_FRAMES: ticket t runs WHOLE on device t % n_devices over the whole template list (uploaded
 * to every device by this call), slot (t / n_devices) % n_frames there; no exchange at all, results exactly those of
 * fdcm_search / fdcm_topk on one device -- the way to raise the throughput of a STREAM of frames (n_devices * n_frames tickets may be
 * outstanding; wait for them in any order, in submission order to keep every device busy).  Only while no frame is in
 * flight; tickets restart at 0 after a change of mode. */
#define FDCM_SHARD_TEMPLATES 0
#define FDCM_SHARD_FRAMES 1
int fdcm_sharded_set_mode(fdcm_sharded* s, int mode);
int fdcm_sharded_submit(fdcm_sharded* s, const float* scene_lines, int64_t n_scene_lines, int64_t max_tmpl_lines,
                        int64_t max_scene_lines, int optimizer, int64_t batch_size, int64_t* ticket);
int fdcm_sharded_submit_topk(fdcm_sharded* s, const float* scene_lines, int64_t n_scene_lines, int64_t max_tmpl_lines,
                             int64_t max_scene_lines, int optimizer, int64_t batch_size, int penalty, float tau, int64_t k,
                             int64_t* ticket);
int fdcm_sharded_wait(fdcm_sharded* s, int64_t ticket, fdcm_match** out, int64_t* n_out);
/* devices / shard_begin (n_devices + 1 entries: shard i holds templates [shard_begin[i], shard_begin[i+1])) may be NULL;
 * collectives = grouped send/recv operations issued so far, bytes_moved = bytes they carried. */
int fdcm_sharded_info(const fdcm_sharded* s, int* n_devices, int* devices, int64_t* shard_begin, int64_t* collectives,
                      int64_t* bytes_moved);
int fdcm_sharded_last_timing(const fdcm_sharded* s, int shard, fdcm_build_timing* bt, fdcm_search_timing* st);
int fdcm_sharded_free(fdcm_sharded* s);

/* ---- frame pipeline (throughput extension; the reference has no counterpart: its callers loop over frames
 *      and each search() blocks, python/src/matching.cpp:283-300).  One frame at the reference's sizes is
 *      latency bound on this GPU, so n_slots frames are kept in flight: each slot owns a feature map (own
 *      HBM volume, workspaces, HIP stream) and a host worker thread that runs fdcm_featuremap_rebuild +
 *      fdcm_search for the frames it is handed.  Tickets count up from 0; ticket t runs on slot t % n_slots,
 *      so at most n_slots tickets may be outstanding.  Results per frame are exactly those of the blocking
 *      calls.  One caller thread at a time per pipeline. ---- */
typedef struct fdcm_pipeline fdcm_pipeline;
int fdcm_pipeline_create(int64_t depth, float dt3_coeff, float padding, int distance, const fdcm_templates* templates,
                         int64_t max_tmpl_lines, int64_t max_scene_lines, int optimizer, int64_t batch_size,
                         int32_t tmpl_index_base, int n_slots, fdcm_pipeline** out);
/* Copies the scene lines and returns at once.  out_device: NULL (matches are returned by wait as a host
 * array) or a device buffer of fdcm_search_capacity() records that must stay valid until the wait. */
int fdcm_pipeline_submit(fdcm_pipeline* p, const float* scene_lines, int64_t n_lines, fdcm_match* out_device,
                         int64_t* ticket);
/* Blocks until the frame is complete.  *out (host array, release with fdcm_matches_free) is set when the
 * frame was submitted without a device buffer; bt / st may be NULL. */
int fdcm_pipeline_wait(fdcm_pipeline* p, int64_t ticket, fdcm_match** out, int64_t* n_out, fdcm_build_timing* bt,
                       fdcm_search_timing* st);
int fdcm_pipeline_slots(const fdcm_pipeline* p, int* n_slots);
int fdcm_pipeline_free(fdcm_pipeline* p); /* waits for frames in flight */

/* ---- ConcentricRangeStrategy (searchstrategies/concentricrange.h:73-84, concentricrange.cpp:29-60): the
 *      scene lines whose centre lies in the annulus low - FLT_EPSILON < r < high around `center`.  The
 *      strategy is DefaultSearch over those lines, so a caller searches with the filtered line array
 *      (search<DefaultMatch> only uses the geometry of the scene lines, defaultmatch.cpp:57-61). ---- */
int fdcm_filter_in_range(const float* lines, int64_t n_lines, const float center[2], float low_boundary,
                         float high_boundary, int64_t* out_indices, int64_t* n_out);

/* ---- tail: penalize (penaltystrategy.h) + sort_matches (matching.cpp:302-307), host side ---- */
int fdcm_penalize(int penalty, float tau, fdcm_match* matches, int64_t n, const float* template_lengths,
                  int64_t n_templates);
int fdcm_sort_matches(fdcm_match* matches, int64_t n);
/* sortMatches(matches, maxNumCandidates) (matchstrategy.h:52-55): std::partial_sort -- the min(max_num_candidates, n) best in
 * ascending score in front, the rest behind them in the order the algorithm leaves. */
int fdcm_partial_sort_matches(fdcm_match* matches, int64_t n, int64_t max_num_candidates);

/* ---- device tail: penalize + sort_matches + "the k best" on matches resident in HBM (the reference's callers do
 *      penalize(), sort_matches() and slice: README.md:71-72, python/src/matching.cpp:291-307).  matches_device:
 *      a buffer filled by fdcm_search_device (n records), or NULL for the matches of the last fdcm_search on
 *      `fm`.  penalty: FDCM_DEFAULT_PENALTY, FDCM_EXPONENTIAL_PENALTY (tau) or -1 for none.  Returns min(k, n)
 *      records in ascending penalised score, ties in positional order (the reference's std::sort leaves ties
 *      unspecified); scores are the reference's bits (denominators from the host libm, IEEE division on the
 *      device).  A record whose tmpl_idx - tmpl_index_base is outside the template set gets a NaN score and
 *      sorts last (fdcm_penalize on the host reports an error for the same input, like the reference's
 *      templatelengths.at()).  Release with fdcm_matches_free.  In sharded runs each rank sends its k best instead
 *      of all. ---- */
int fdcm_topk(fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches_device, int64_t n,
              int32_t tmpl_index_base, int penalty, float tau, int64_t k, fdcm_match** out, int64_t* n_out);

/* ---- exhaustive translation search: every template scored at every point of a translation grid (the
 *      sliding-window form of FDCM; the reference's search only walks scene lines, defaultmatch.cpp:32-89).
 *      Not in the reference: the definitions are this project's (README.md, "Exhaustive search"). ----
 * A grid is {x0, y0, nx, ny, sx, sy}: nx, ny >= 1, sx, sy >= 1, nx * ny < 2^31, every point inside |t| < 2^24.  Point (i, j)
 * is the translation t = (x0 + i sx, y0 + j sy), row-major index g = j nx + i.  score(template, t) is evaluate<Dt3Cpu>
 * (dt3cpu.cpp:126-179) at t: exactly the bits fdcm_featuremap_evaluate returns for that template and translation.  t is
 * admissible for a template when fdcm_featuremap_evaluate does not return NaN there (every end point + T + t inside
 * (-1, W) x (-1, H)): a product of two integer intervals per template.  A template without lines scores 0 everywhere.
 * An admissible point whose score is NaN (NaN, or +inf and -inf on one line, in the volume's data) is left out of every
 * top-k, peak and rotation search as if it were not admissible; an infinite score is kept and orders after every finite
 * one.  The score maps hold such points' NaN as it is.
 * Concurrent callers of one feature map take turns, as for the seam. */
typedef struct fdcm_grid {
    int32_t x0, y0, nx, ny, sx, sy;
} fdcm_grid;
/* The smallest grid with strides (sx, sy) and x0, y0 multiples of them that holds every admissible integer translation of
 * every template with lines; nx = ny = 0 when there is none. */
int fdcm_exhaustive_window(const fdcm_featuremap* fm, const fdcm_templates* templates, int32_t sx, int32_t sy, fdcm_grid* grid);
/* Per template with lines, in ascending index: its admissible grid points ordered by (score, g), the first min(k, count)
 * of them as records {index + tmpl_index_base, score, {1, 0, t.x, 0, 1, t.y}} (combine(t, identity): penalize,
 * sort_matches and the device tail take them as they are).  1 <= k <= 64.  An empty feature map or template list gives
 * zero records.  Release with fdcm_matches_free. */
int fdcm_search_exhaustive(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_grid* grid, int32_t k,
                           int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out);
/* Peaks: key(p) = (score bits << 32) | g for an admissible point p (a total order; points that are not admissible have no
 * key).  For radii 0 <= rx, ry <= 32 in grid steps, an admissible point p = (i, j) is a peak of its template when
 * key(p) < key(q) for every other admissible point q = (i', j') of the grid with |i' - i| <= rx and |j' - j| <= ry:
 * key(p) is the minimum of the keys in its (2 rx + 1) x (2 ry + 1) window, neighbours outside the grid or not admissible
 * ignored.  Two peaks are never within (rx, ry) of each other; on a plateau of equal scores the lowest grid index wins.
 * Per template with lines, in ascending index: its peaks ordered by key, the first min(k, count) of them (1 <= k <= 64),
 * as the records of fdcm_search_exhaustive.  Templates without lines or without admissible points in the grid give
 * nothing; an empty feature map or template list gives zero records.  rx = ry = 0 is exactly fdcm_search_exhaustive.
 * Device memory stays below 1 GB whatever the templates and the grid.  Release with fdcm_matches_free. */
int fdcm_search_exhaustive_peaks(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_grid* grid, int32_t k,
                                 int32_t rx, int32_t ry, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out);
/* The score map: out[template][j][i] = score at grid point (i, j) where admissible, NaN elsewhere (n_templates * ny * nx
 * floats). */
int fdcm_score_map(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_grid* grid, float* out_host);
/* Same into device memory; returns when the map is complete (as fdcm_search_device). */
int fdcm_score_map_device(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_grid* grid, float* out_device);

/* Rotations: the exhaustive search as a dense pose search over (angle, x, y).  n >= 1 rotations (c, s), float32, no unit
 * norm required (a scale is a rotation of norm != 1), cs holding n pairs; pivots: one (px, py) per template, or NULL for
 * the origin.  The rotated template M_a(t) is rotate(lines, R, rot_point) (math.h:372-378) with R = [[c, -s], [s, c]]:
 * M_a = [R | m], m.x = px - (c px + (-s) py), m.y = py - (s px + c py), and every end point (x, y) goes to
 * ((c x + (-s) y) + m.x, (s x + c y) + m.y), each product and sum rounded to float32 left to right (no fused
 * multiply-add).  score(t, a, g) is the score above of M_a(t) at grid point g, admissible by the rule above applied to
 * M_a(t): every (t, a) has a box of its own.  Records are {t + tmpl_index_base, score, {c, -s, m.x + t.x, s, c,
 * m.y + t.y}} (float32 adds; combine(translation, M_a), the DefaultMatch convention), taken by penalize, sort_matches and
 * the device tail as the alignment search's.  All values c, s and pivots must be finite. */
typedef struct fdcm_rotations {
    const float* cs;
    int32_t n;
    const float* pivots;
} fdcm_rotations;
/* The smallest grid with strides (sx, sy) and x0, y0 multiples of them that holds every admissible integer translation of
 * every (template with lines, rotation); nx = ny = 0 when there is none. */
int fdcm_exhaustive_rotations_window(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                     int32_t sx, int32_t sy, fdcm_grid* grid);
/* Peaks across rotations.  N = nx ny; key(t, a, g) = (score bits << 32) | (a N + g), a total order per template (score,
 * then rotation index, then grid index); n N <= 2^32 is required.  For radii 0 <= rx, ry, ra <= 32 and wrap 0 or 1, the
 * angle distance is d(a, a') = |a - a'|, or min(|a - a'|, n - |a - a'|) with wrap = 1.  An admissible (a, i, j) is a peak
 * when its key is below the key of every other admissible (a', i', j') of the same template with |i' - i| <= rx,
 * |j' - j| <= ry and d(a, a') <= ra.  Per template with lines, in ascending index: its peaks ordered by key, the first
 * min(k, count) (1 <= k <= 64).  rx = ry = ra = 0 is the top-k over all (rotation, grid point) pairs; one rotation (1, 0)
 * gives fdcm_search_exhaustive_peaks' records (transform entry 1 is -0).  Device memory stays below 1 GB whatever the
 * number of templates and rotations and the grid.  Release with fdcm_matches_free. */
int fdcm_search_exhaustive_rotations(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                     const fdcm_grid* grid, int32_t k, int32_t rx, int32_t ry, int32_t ra, int32_t wrap,
                                     int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out);
/* The score maps of every rotated template: out[t][a][j][i], NaN where not admissible (n_templates * n * ny * nx floats). */
int fdcm_score_map_rotations(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                             const fdcm_grid* grid, float* out_host);

/* Pose windows: a list of jobs for refinement (a small box of fine poses around each coarse peak) and tracking (a small box
 * around the last frame's pose).  A job is one template, a run of rotations of the table `rot` (n rotations) and a small
 * translation grid of its own, searched exhaustively.  Job j has the grid G_j = (x0, y0, nx, ny, sx, sy) with the call's
 * strides and N_j = nx ny points; position e of its run is rotation a = (a0 + e) mod n.  score, admissibility and the NaN
 * rule are those of fdcm_search_exhaustive_rotations for template tmpl, rotation a, pivot pivots[tmpl] and grid point
 * g = jj nx + ii of G_j; key(e, g) = (score bits << 32) | (e N_j + g).
 * Output: the jobs in the order given; per job its admissible (e, g) ordered by key, the first min(k, count) of them
 * (1 <= k <= 64), as records {tmpl + tmpl_index_base, score, {c, -s, m.x + t.x, s, c, m.y + t.y}} of rotation a.
 * job_offsets (n_jobs + 1 values, or NULL): the records of job j are job_offsets[j] .. job_offsets[j + 1].  A job whose
 * template has no lines gives nothing, as does a job without an admissible point; duplicate jobs give duplicate records.
 * rot == NULL is the translations only: the table is one rotation, every job must have a0 = 0 and na = 1, the lines are
 * scored as they are (not passed through an identity rotation, which would turn a -0 coordinate into +0) and the records
 * are fdcm_search_exhaustive's {1, 0, t.x, 0, 1, t.y}.
 * By definition job j's records are those of fdcm_search_exhaustive_rotations on the one-template set {tmpl} with that
 * template's pivot, the rotations of the run in run order, the grid G_j, rx = ry = ra = 0 and base tmpl + tmpl_index_base;
 * with rot == NULL those of fdcm_search_exhaustive.
 * FDCM_EINVAL, before any GPU work: jobs NULL with n_jobs > 0, n_jobs < 0; tmpl outside the set; na < 1 or na > n; a0
 * outside 0 .. n - 1; a0 + na > n with wrap = 0 (wrap = 1: the run continues at rotation 0); nx or ny < 1;
 * na nx ny > 65536 (a larger search is the dense call's); a grid point with |t| >= 2^24; sx or sy < 1; k outside 1 .. 64;
 * wrap not 0 or 1; and whatever fdcm_search_exhaustive_rotations rejects about rot.  n_jobs = 0, an empty feature map or an
 * empty template list give zero records and job_offsets all 0.  Device memory stays below 1 GB however many jobs there
 * are: the list is worked through in parts.  One job is never cut, and the rotated lines of its run go up together, na x
 * the template's lines x 32 bytes, as the dense call uploads those of all its rotations: only a job of tens of thousands
 * of rotations of a template of hundreds of lines comes near that bound.  The call blocks; concurrent callers of one
 * feature map take turns.  Release with fdcm_matches_free. */
typedef struct fdcm_pose_window {
    int32_t tmpl;           /* template index, 0 .. n_templates - 1 */
    int32_t a0, na;         /* the run of rotations a0, a0 + 1, .., a0 + na - 1 of the table (mod n when wrap = 1) */
    int32_t x0, y0, nx, ny; /* this job's translation grid, with the call's strides */
} fdcm_pose_window;
int fdcm_search_exhaustive_windows(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                   const fdcm_pose_window* jobs, int64_t n_jobs, int32_t sx, int32_t sy, int32_t wrap,
                                   int32_t k, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                   int64_t* job_offsets /* n_jobs + 1, or NULL */);

/* Best map and detections: the templates compared with each other.  A template set is usually many views or rotations of a
 * few objects, so one object in the scene gives a peak in almost every template's map at about the same place; these two
 * calls reduce over the templates on the device.  The definitions are this project's (README.md, "Best template per point
 * and detections"; numpy statement: tests/detect_ref.py).
 * Inputs as fdcm_search_exhaustive_rotations: a feature map, T templates, a grid.  rot is optional: rot == NULL is one
 * "rotation" (n = 1), the lines scored as they are (not passed through an identity rotation, which would turn a -0
 * coordinate into +0) and the transforms {1, 0, t.x, 0, 1, t.y}.  Pair u = t n + a is template t under rotation a;
 * score(t, a, g) and admissibility are the rotation search's.
 * Normalised score q(t, a, g): the value fdcm_penalize(penalty, tau, ..) gives a record {t, score(t, a, g)} with the
 * lengths of fdcm_templates_lengths: score / max(len_t, 1e-6f) (FDCM_DEFAULT_PENALTY), score / std::pow(max(len_t, 1e-6f),
 * tau) (FDCM_EXPONENTIAL_PENALTY), the denominators computed on the host and one IEEE float32 division on the device;
 * penalty = -1: q = score.  Rotation or scale in rot does not change len_t.
 * Candidates of grid point g: the pairs u of templates with lines that are admissible at g and whose q is not NaN
 * (templates without lines score 0 everywhere and take no part; an infinite q is a candidate and orders last).
 * pairkey(u, g) = (bits of q << 32) | u; best(g) is the candidate with the smallest pairkey: the lowest q, ties to the
 * lowest t, then the lowest a.
 * fdcm_best_map: two planes of ny x nx, row-major: the float32 q of best(g), NaN where g has no candidate, and the int32
 * u of best(g), -1 there.  Either output may be NULL, not both.
 * fdcm_search_exhaustive_detect: the peaks of the best-score plane by the rule of fdcm_search_exhaustive_peaks:
 * key(g) = (bits of q(best(g)) << 32) | g; g is a detection when its key is below the key of every other point with a
 * candidate within rx, ry grid steps (0 <= rx, ry <= 32).  Output: the first min(k, count) detections by key
 * (1 <= k <= 64), as records {t + tmpl_index_base, q, {c, -s, m.x + t.x, s, c, m.y + t.y}} of the pair u = best(g): the
 * score is the normalised one and the records are in ascending order, so the caller neither penalises nor sorts.  The
 * minimum over rotations is taken before the peaks: suppression does not look at angles.  Results are a function of the
 * inputs alone.
 * FDCM_EINVAL, before any GPU work: what fdcm_search_exhaustive_rotations rejects about its handles, grid, rot and
 * pivots (its bound n nx ny <= 2^32 belongs to its keys and does not apply); T n > 2^31 - 1; nx ny > 2^26 (a larger grid
 * is the caller's to cut: 8 bytes of keys and 4 of scores per point stay below 1 GB); penalty not -1, FDCM_DEFAULT_PENALTY
 * or FDCM_EXPONENTIAL_PENALTY; a tau that is not finite; k or a radius out of range; NULL outputs.  An empty feature map,
 * an empty template list or no template with lines give zero records and planes of NaN / -1.  Both calls block;
 * concurrent callers of one feature map take turns.  Release the records with fdcm_matches_free. */
int fdcm_best_map(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                  const fdcm_grid* grid, int penalty, float tau, float* score_out_host, int32_t* pair_out_host);
int fdcm_search_exhaustive_detect(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                                  const fdcm_grid* grid, int32_t k, int32_t rx, int32_t ry, int penalty, float tau,
                                  int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out);

/* Detections suppressed by footprint overlap: the greedy rule of object detectors in place of the radius.  A radius counts
 * grid steps of the template origin and is one for all templates; here a detection suppresses the points whose posed
 * template lies where its own does.  The definitions are this project's (README.md, "Detections by footprint overlap";
 * numpy statement: tests/nms_ref.py).
 * Inputs: those of fdcm_search_exhaustive_detect without rx, ry, with overlap_permille (0 .. 1000) and margin (0 .. 4096
 * pixels).  Candidates, q, pairkey, best(g) and key(g) = (bits of q(best(g)) << 32) | g are the best map's, caps included.
 * Footprint of a pair u = (t, a): over the end points of the lines of M_a(t), the float32 values the searches score (rot ==
 * NULL: the caller's lines as they are), fx0 = floor(min x) - margin, fx1 = floor(max x) + margin, fy0 and fy1 likewise,
 * computed in int64, clamped to [-2^25, 2^25] and stored as int32.  The box is the pixel rectangle [fx0, fx1] x [fy0, fy1],
 * ends inclusive: width and height are at least 1.  A template without lines, or with a NaN end point, has the empty box
 * (0, 0, -1, -1); it is never a candidate, so the box is never read.  Caps and penalties do not enter.  The footprint of
 * grid point g is F(g) = box(best(g)) + t_g with t_g = (x0 + i sx, y0 + j sy); the scene translation T is common to all
 * points and left out.
 * Overlap, exact in int64: I(g, h) is the area of F(g) n F(h), max(0, min(x1) - max(x0) + 1) * max(0, min(y1) - max(y0) + 1);
 * U = A(g) + A(h) - I; h suppresses g when 1000 I > overlap_permille U (sides are at most 2^26 + 1, so 1000 U < 2^63).
 * Greedy rule: S_0 is the set of grid points with a candidate.  For n = 0, 1, ..: stop when n = k or S_n is empty;
 * otherwise d_n is the point of the smallest key in S_n and S_(n+1) = S_n \ {d_n} \ {g : d_n suppresses g}.
 * Output: the d_n in order (1 <= k <= 64), as records {t + tmpl_index_base, q, {c, -s, m.x + t.x, s, c, m.y + t.y}} of
 * best(d_n), exactly the record fdcm_search_exhaustive_detect would emit for that point; keys ascend.  boxes_out (4 k
 * int32, or NULL): F(d_n) as x0, y0, x1, y1 per record.
 * Identities: overlap_permille = 1000 suppresses nothing (I <= U): the call is fdcm_search_exhaustive_detect with rx = ry =
 * 0, record for record, whatever the margin.  overlap_permille = 0 accepts no two detections whose footprints share a
 * pixel.  Results are a function of the inputs alone.
 * fdcm_templates_footprints (host only, no device work): the footprints the call uses, 4 int32 x0, y0, x1, y1 per pair u =
 * t n + a (n = 1 with rot == NULL).  fdcm_lines_footprints: the same for a set given as fdcm_templates_create takes it
 * (packed lines, n_templates + 1 offsets), for callers without a handle: a process without a device has none.
 * FDCM_EINVAL, before any GPU work: everything fdcm_search_exhaustive_detect rejects (nx ny > 2^26 and T n > 2^31 - 1
 * included), overlap_permille outside 0 .. 1000, margin outside 0 .. 4096.  Empty inputs give zero records.  The call
 * blocks; concurrent callers of one feature map take turns.  Release the records with fdcm_matches_free. */
int fdcm_search_exhaustive_detect_nms(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                                      const fdcm_grid* grid, int32_t k, int32_t overlap_permille, int32_t margin, int penalty, float tau,
                                      int32_t tmpl_index_base, fdcm_match** out, int32_t* boxes_out /* 4 k, or NULL */, int64_t* n_out);
int fdcm_templates_footprints(const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */, int32_t margin,
                              int32_t* boxes_out);
int fdcm_lines_footprints(const float* lines, const int64_t* offsets, int64_t n_templates, const fdcm_rotations* rot /* or NULL */,
                          int32_t margin, int32_t* boxes_out);

/* All detections below a score: the detector's threshold.  The two detection calls above return "the k best" (k <= 64),
 * whatever their scores; this call returns every detection that matches at least as well as max_score, up to a bound the
 * caller sets.  The definitions are this project's (README.md, "All detections below a score"; numpy statement:
 * tests/detect_all_ref.py).
 * Inputs: those of fdcm_search_exhaustive_detect_nms with k replaced by max_score (float32, >= +0 or +inf) and
 * max_detections (1 .. 4096).  Candidates, q, pairkey, best(g), key(g), the footprints, the overlap test and the record
 * layout are that call's, caps, rot == NULL and the meaning of margin and overlap_permille included.
 * S_0 is the set of grid points with a candidate whose q(best(g)) <= max_score, compared in float32 on the q fdcm_best_map
 * would hold.  The rule is the greedy rule of fdcm_search_exhaustive_detect_nms on this S_0, stopping when n =
 * max_detections or S_n is empty.  Output: the d_n in order as records, *n_out of them; boxes_out (4 max_detections int32,
 * or NULL): F(d_n) per record.
 * Identities: max_score = +inf and max_detections = k <= 64 give fdcm_search_exhaustive_detect_nms' records, byte for byte.
 * For any max_score the records are the leading records with score <= max_score of the +inf list at the same
 * max_detections: keys ascend, and a point over the threshold never precedes, so never suppresses, one under it.
 * The device skips work the threshold makes pointless: a score is a sum of terms >= +0, so a partial sum that is over the
 * template's bound ends that template for the points of a wave once all of them are over it.  The
 * records do not depend on it.
 * fdcm_detect_score_bounds (host only, no device work): per template B_t, the largest float32 s >= +0, possibly +inf, whose
 * IEEE float32 quotient s / den_t is <= max_score, den_t the denominator of q above (1 with penalty = -1); 0 for a template
 * without lines.  A sum above B_t is exactly a sum whose q is above max_score.  fdcm_score_bound: the same for one
 * denominator given as a number, for callers without a handle (a process without a device has none).
 * FDCM_EINVAL, before any GPU work: everything fdcm_search_exhaustive_detect_nms rejects; max_score NaN or < 0;
 * max_detections outside 1 .. 4096.  Empty inputs give zero records.  The call blocks; concurrent callers of one feature map
 * take turns.  Results are a function of the inputs alone.  Release the records with fdcm_matches_free. */
int fdcm_search_exhaustive_detect_all(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                                      const fdcm_grid* grid, float max_score, int32_t max_detections, int32_t overlap_permille,
                                      int32_t margin, int penalty, float tau, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                      int32_t* boxes_out /* 4 max_detections, or NULL */);
int fdcm_detect_score_bounds(const fdcm_templates* templates, int penalty, float tau, float max_score, float* bounds /* n_templates */);
int fdcm_score_bound(float den, float max_score, float* bound);

/* Per-line caps and line costs: the truncated directional chamfer cost.  A score is a plain sum over the template's lines,
 * so one line whose scene edge is missing (occlusion, a gap in the edges, a line the fit dropped) can cost as much as all
 * the others matched badly.  A template set may carry one cap per line; every exhaustive call above then clamps each
 * line's term to its cap.  The definitions are this project's (README.md, "Per-line caps and line costs"; numpy statement:
 * tests/capped_ref.py); the reference has no counterpart.
 * Line cost: cost_i(t) = |I_bin(i)(floor(p1_i + T + t)) - I_bin(i)(floor(p2_i + T + t))|, the term of evaluate<Dt3Cpu>; the
 * rotation calls use the rotated line.  It is >= +0 or NaN.
 * Cap: one float32 cap_i per template line, cap_i >= 0, finite or +inf, never NaN; +inf: no cap (-0 is stored as +0).
 * Capped cost: capped_i = cost_i > cap_i ? cap_i : cost_i.  A NaN cost stays NaN (the point is left out of top-k, peaks,
 * best map and detections and is NaN in maps, as before); an infinite cost under a finite cap becomes the cap; cap_i = 0
 * switches the line off.
 * Score of a capped set: the sum of capped_i in the order of every score here (Eigen's sum(): blocks of 8 in two packets,
 * the trailing packet, predux, the scalar tail).  Admissibility, default windows, keys, peak rules, the denominators of q
 * and the record layout do not look at caps.  A line keeps its cap under every rotation; a rot entry with scale does not
 * rescale caps, as it does not rescale lengths.  A set without caps, or with every cap +inf, gives the bytes
 * fdcm_templates_create's set gives in every call.  fdcm_search, fdcm_topk, the frame pipeline and the sharded engine
 * ignore caps: their contract is the reference's.
 * What a cap means: cost_i is roughly the sum of the DT3 values under the line's rasterised pixels, so cap_i = tau len_i
 * with len_i = getLength of the line (fdcm_templates_line_lengths) means roughly "a line whose mean directional distance
 * exceeds tau pixels counts as tau" -- approximately, within the rasteriser's factor between pixel count and length.  With
 * FDCM_DEFAULT_PENALTY q then lies in [0, tau] up to rounding.
 * fdcm_templates_create_capped: fdcm_templates_create with caps (one per line, in line order; NULL: all +inf).
 * fdcm_templates_line_caps / _line_lengths: the caps (+inf for a set made by fdcm_templates_create) and the float32
 * lengths of the lines, n_lines floats each.
 * fdcm_line_costs: the uncapped cost of every line at n poses.  A pose is four int32 (tmpl, a, x, y): a is a rotation
 * index of rot and must be 0 with rot == NULL, where the lines are scored as they are; (x, y) is the translation.
 * offsets (n + 1) says where each pose's floats begin in *costs: the cost_i of tmpl's lines in line order, all NaN when the
 * pose is not admissible for (tmpl, a) by the rule of the searches.  A template without lines contributes no floats.
 * Identity: for an admissible pose, clamping the costs with the set's caps and summing in the order above gives exactly the
 * score bits fdcm_search_exhaustive_windows returns for the job {tmpl, a, 1, x, y, 1, 1} at stride 1 (rot == NULL: those
 * of fdcm_search_exhaustive on the one-point grid).
 * FDCM_EINVAL, before any GPU work: a NaN or negative cap; n < 0; poses NULL with n > 0; what the rotation call rejects
 * about rot; a out of range; |x| or |y| >= 2^24; tmpl outside the set; NULL outputs.  n = 0, an empty feature map or an
 * empty template list give offsets of 0.  The call blocks; *costs (never NULL after FDCM_OK) is released with
 * fdcm_lines_free. */
int fdcm_templates_create_capped(const float* lines, const int64_t* offsets /* n_templates+1, in lines */, int64_t n_templates,
                                 const float* caps /* one per line, or NULL */, fdcm_templates** out);
int fdcm_templates_line_caps(const fdcm_templates* t, float* caps /* n_lines */);
int fdcm_templates_line_lengths(const fdcm_templates* t, float* lengths /* n_lines */);
int fdcm_line_costs(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                    const int32_t* poses /* n x 4: tmpl, a, x, y */, int64_t n, float** costs, int64_t* offsets /* n + 1 */);

/* Detections by matched fraction: how much of the template was found.  With caps q lies in [0, tau] and saturates: a view
 * that is mediocre on every line can have the q of a correct view with a third of its lines hidden, and max_score cannot
 * tell them apart.  The matched fraction can, and the gate below applies it before the greedy rule, so that a junk point
 * never suppresses a good neighbour.  The definitions are this project's (README.md, "Detections by matched fraction"; numpy
 * statement: tests/matched_ref.py).  Everything not restated here is fdcm_search_exhaustive_detect_all's, unchanged:
 * candidates, q, pairkey, best(g), key(g), footprints, the overlap test, the record layout, admissibility and rot == NULL.
 * Line quantities: for line i of template t, len_i is the float32 fdcm_templates_line_lengths returns, the length of the
 * unrotated line; like a cap it is kept under every rotation and is not rescaled by a rot entry with scale.  cap_i is the
 * set's cap of line i (+inf for a set without caps).  cost_i(u, t) is the uncapped line cost of the pair u = (t, a) at the
 * translation, exactly the float fdcm_line_costs returns.
 * Matched: line i is matched at (u, t) when cost_i <= cap_i, one float32 compare: a NaN cost is not matched, an infinite
 * cost under cap_i = +inf is, and a line with cap_i = 0 is matched only at cost 0.
 * Matched length: ML(u, t) = (((+0 + w_0) + w_1) + ..) in float32, in line order, w_i = len_i when line i is matched and +0
 * otherwise.  TL_t is the same sum with every line matched, so +0 <= ML <= TL_t (float addition is monotone).
 * Fraction: frac(u, t) = ML / TL_t, one IEEE float32 division; 1 when TL_t == 0 (a template without lines, or with lines of
 * length zero only); NaN when the pose is not admissible for u, whatever TL_t.
 * Gate: min_matched is a float32 in [0, 1]; need_t = float32(min_matched * TL_t), one float32 product.  A grid point g with a
 * candidate passes when ML(best(g), t_g) >= need_t, t the template of best(g).  S_0 is the set of points with a candidate,
 * q(best(g)) <= max_score, that pass the gate; the greedy rule runs on this S_0, stopping at max_detections.
 * What the gate looks at: the pair the best map holds at g, and only that pair.  A point whose best pair fails is dropped,
 * even if another pair at g would pass: the gate is not part of the minimum that chooses best(g).  FDCM_GATE_ALL ("Gate
 * inside the minimum", below) lifts this limitation.
 * fdcm_search_exhaustive_detect_all_matched: fdcm_search_exhaustive_detect_all with the gate.  matched_out (max_detections
 * floats, or NULL): entry l is frac of record l; the entries from *n_out on are not specified.
 * fdcm_matched_fractions: frac at n poses (tmpl, a, x, y); poses, admissibility and rot are fdcm_line_costs'.
 * fdcm_templates_matched_totals (host only, no device work): TL_t per template.
 * Identities: min_matched = 0 gives fdcm_search_exhaustive_detect_all's records and boxes, byte for byte (no gate pass is
 * queued).  A set whose caps are all +inf, on a volume without NaN or infinity, has frac = 1 everywhere, and any
 * min_matched gives those bytes.  At a fixed min_matched the records for any max_score are the leading records with score
 * <= max_score of the +inf list.  With overlap_permille = 1000 and max_detections not reached the records are the
 * min_matched = 0 list without the failing points, order kept.  matched_out[l] is, bit for bit, what
 * fdcm_matched_fractions returns for record l's (tmpl, a, x, y); and for an admissible pose ML computed from
 * fdcm_line_costs' floats, the set's caps and lengths by the rule above is the device's, bit for bit.  Results are a
 * function of the inputs alone.
 * FDCM_EINVAL, before any GPU work: everything fdcm_search_exhaustive_detect_all rejects; min_matched NaN, < 0 or > 1; for
 * fdcm_matched_fractions what fdcm_line_costs rejects about n, poses, rot and the handles, and fractions NULL with n > 0.
 * n = 0, an empty feature map or an empty template list return FDCM_OK and write nothing.  The calls block; concurrent
 * callers of one feature map take turns.  Release the records with fdcm_matches_free. */
int fdcm_search_exhaustive_detect_all_matched(const fdcm_featuremap* fm, const fdcm_templates* templates,
                                              const fdcm_rotations* rot /* or NULL */, const fdcm_grid* grid, float max_score,
                                              int32_t max_detections, int32_t overlap_permille, int32_t margin, int penalty, float tau,
                                              float min_matched, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                              int32_t* boxes_out /* 4 max_detections, or NULL */,
                                              float* matched_out /* max_detections, or NULL */);
int fdcm_matched_fractions(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                           const int32_t* poses /* n x 4: tmpl, a, x, y */, int64_t n, float* fractions /* n */);
int fdcm_templates_matched_totals(const fdcm_templates* templates, float* totals /* n_templates */);

/* Detections over pose windows: the detector's rule applied to the winners of a job list.  The detector above is a dense
 * search of one grid and the whole rotation table; the pose windows are the coarse-to-fine and tracking path, but return raw
 * top-k records per job.  This call joins them: every job is searched as a pose window, its best pose is normalised,
 * thresholded and gated as a point of the detector is, and the jobs' best poses suppress each other by footprint overlap.
 * The definitions are this project's (README.md, "Detections over pose windows"; numpy statement:
 * tests/window_detect_ref.py).  Everything not restated here is taken unchanged from fdcm_search_exhaustive_windows (jobs,
 * runs, wrap, rot == NULL, admissibility, the score with the set's line caps) and from
 * fdcm_search_exhaustive_detect_all_matched (q and its denominators, footprints with margin, the overlap test in int64, ML,
 * TL, need, frac, the record layout).
 * Inputs: a feature map, templates, rot or NULL, pivots; jobs (fdcm_pose_window, n_jobs), sx, sy, wrap; max_score,
 * max_detections (1 .. 4096), overlap_permille, margin, penalty, tau, min_matched, tmpl_index_base.
 * Winner of job j: the admissible (e, g) of the job with the smallest windows key (score bits << 32) | (e N_j + g), exactly
 * the one record fdcm_search_exhaustive_windows returns for that job at k = 1.  A job whose template has no lines, or that
 * has no admissible point, has no winner.  For a job with a winner a_j = (a0 + e) mod n is the winner's rotation, t_j its
 * translation and q_j = score / den(tmpl), one IEEE float32 division with the denominators of fdcm_penalize; penalty = -1
 * gives q = score.  The winner is chosen on the raw score, before the division.
 * Candidates S_0: the jobs that have a winner, whose q_j is not NaN, with q_j <= max_score and ML((tmpl, a_j), t_j) >=
 * need_tmpl.  What the gate looks at: the winner, and only the winner, as the dense call's gate looks at best(g) only.  A
 * job whose winner fails is dropped, even if another pose of its window would pass: the gate is not part of the minimum
 * that chooses the winner.  FDCM_GATE_ALL ("Gate inside the minimum", below) lifts this limitation.
 * key(j) = (bits of q_j << 32) | j.  Duplicate jobs are distinct candidates; the later one loses the tie and is then
 * suppressed by the earlier, unless overlap_permille = 1000.  Footprint F(j) = box(tmpl, a_j) + t_j, box as
 * fdcm_templates_footprints gives it at margin.  The rule is the greedy rule of fdcm_search_exhaustive_detect_nms on S_0 with
 * these keys and footprints, stopping at max_detections.
 * Output: the d_n in order, as records {tmpl + tmpl_index_base, q, {c, -s, m.x + t.x, s, c, m.y + t.y}}; with rot == NULL
 * the transform is {1, 0, t.x, 0, 1, t.y}.  boxes_out (4 max_detections int32, or NULL): F(d_n) per record.  matched_out
 * (max_detections floats, or NULL): frac of record l, bit for bit fdcm_matched_fractions of the record's (tmpl, a, x, y).
 * jobs_out (max_detections int32, or NULL): the job each record came from.  The entries from *n_out on are not specified.
 * Identities: (1) with overlap_permille = 1000, max_score = +inf, min_matched = 0 and max_detections >= the number of
 * winners the records are the k = 1 records of fdcm_search_exhaustive_windows, passed through fdcm_penalize and ordered by
 * (score bits, job), byte for byte.  (2) One-point jobs (na = nx = ny = 1) for every keyed point of fdcm_best_map, carrying
 * that point's best pair, listed by ascending g, give the records, boxes and fractions of
 * fdcm_search_exhaustive_detect_all_matched on that grid with the same parameters, byte for byte.  (3) At fixed other
 * parameters the records for any max_score are the leading records with score <= max_score of the +inf list.  (4)
 * overlap_permille = 0: no two returned boxes share a pixel.  (5) Results are a function of the inputs alone.
 * FDCM_EINVAL, before any GPU work: everything fdcm_search_exhaustive_windows rejects about jobs, rot, strides and wrap;
 * everything fdcm_search_exhaustive_detect_all_matched rejects about max_score, max_detections, overlap_permille, margin,
 * penalty, tau and min_matched; n_jobs > 2^22 (the winners' list is 24 bytes per job and is not cut into parts); NULL out
 * or n_out.  No jobs, an empty feature map or an empty template list give zero records and FDCM_OK.  The call blocks;
 * concurrent callers of one feature map take turns.  Device memory stays below 1 GB: the scoring goes through the job list
 * in parts, as fdcm_search_exhaustive_windows does.  Release the records with fdcm_matches_free. */
int fdcm_search_exhaustive_detect_windows(const fdcm_featuremap* fm, const fdcm_templates* templates,
                                          const fdcm_rotations* rot /* or NULL */, const fdcm_pose_window* jobs, int64_t n_jobs,
                                          int32_t sx, int32_t sy, int32_t wrap, float max_score, int32_t max_detections,
                                          int32_t overlap_permille, int32_t margin, int penalty, float tau, float min_matched,
                                          int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                          int32_t* boxes_out /* 4 max_detections, or NULL */,
                                          float* matched_out /* max_detections, or NULL */,
                                          int32_t* jobs_out /* max_detections, or NULL */);

/* Gate inside the minimum: the matched-fraction gate as a condition on candidates, not a filter on winners.  With line caps q
 * saturates in [0, tau]: at the point where an object lies a wrong view that matches half of its lines perfectly and has the
 * other half capped can win the minimum over the right view, which matches every line moderately.  The gate above then
 * deletes the point although the right view was scored there and would have passed.  Here a pair is a candidate of a point
 * only if it passes the gate there, and a pose is a candidate of its window only if it passes.  The definitions are this
 * project's (README.md, "Gate inside the minimum"; numpy statement: tests/gate_ref.py).  Everything not restated here is
 * taken unchanged from fdcm_search_exhaustive_detect_all_matched and fdcm_search_exhaustive_detect_windows: score, caps,
 * admissibility, rot == NULL, q and its denominators, pairkey, key(g), footprints, the overlap test, the greedy rule, the
 * record layout, len_i, cap_i, the uncapped cost_i, matched (cost_i <= cap_i), ML (sequential float32 sum in line order from
 * +0), TL_t, need_t = float32(min_matched * TL_t) and frac = ML / TL (1 when TL == 0).
 * Gates: FDCM_GATE_WINNER is the gate of the two calls above.  FDCM_GATE_ALL is the gate inside the minimum:
 * Dense, gate ALL: the candidates of grid point g are the pairs u = (t, a) of templates with lines that are admissible at g,
 * whose q is not NaN and with ML(u, t_g) >= need_t.  best(g) is the candidate of the smallest pairkey; a point without a
 * candidate has no key.  S_0 is the set of points with a candidate and q(best(g)) <= max_score; no second gate pass follows.
 * The rest is the greedy rule and the output of fdcm_search_exhaustive_detect_all_matched: records, boxes, fractions.
 * Gated best map (fdcm_best_map_gated): the planes q(best(g)), u(best(g)) and frac(best(g), t_g) for best as just defined,
 * row-major [ny][nx]; NaN, -1 and NaN where g has no candidate.  Any of the three may be NULL, not all of them.
 * Windows, gate ALL: the winner of job j is the admissible (e, g) with the smallest windows key (score bits << 32) | (e N_j +
 * g) whose score is not NaN and whose pose passes ML((tmpl, a_e), t_g) >= need_tmpl.  A job with no such pose has no winner.
 * The winner is still chosen on the raw score.  q_j, the threshold, key(j), footprints, the greedy rule and the outputs are
 * unchanged.
 * Identities: gate = FDCM_GATE_WINNER gives the bytes of the call without the argument (it is that call).  min_matched = 0
 * gives, under either gate, the ungated bytes, and the gated best map at 0 gives fdcm_best_map's planes.  A set whose caps are
 * all +inf, on a volume without NaN or infinity, gives the ungated bytes for any min_matched under either gate.  With
 * overlap_permille = 1000 and max_detections not reached every record of gate WINNER is a record of gate ALL, same bytes: a
 * point whose unrestricted best pair passes keeps it.  At fixed other parameters the records for any max_score are the
 * leading records with score <= max_score of the +inf list.  Every record's fraction is, bit for bit, what
 * fdcm_matched_fractions returns for its (tmpl, a, x, y), and its ML is >= need.  Results are a function of the inputs alone,
 * whatever order workgroups run in.
 * Which gate: WINNER when the gate only has to remove junk and the score alone should choose the view (it costs one pass over
 * the key plane); ALL when caps are in use and occluded or partly matching views compete at one point, so that the object
 * under the junk is kept (it costs a compare, a select and an add per term in the scoring kernel, and no gate pass).
 * FDCM_EINVAL, before any GPU work: everything the call without the argument rejects; gate not FDCM_GATE_WINNER or
 * FDCM_GATE_ALL; for fdcm_best_map_gated what fdcm_best_map rejects, min_matched NaN, < 0 or > 1, and all three planes NULL.
 * Empty inputs give FDCM_OK and zero records (planes of NaN / -1 / NaN), as the siblings do.  The calls block; concurrent
 * callers of one feature map take turns.  Release the records with fdcm_matches_free. */
#define FDCM_GATE_WINNER 0
#define FDCM_GATE_ALL 1
int fdcm_best_map_gated(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                        const fdcm_grid* grid, int penalty, float tau, float min_matched, float* score_out_host /* or NULL */,
                        int32_t* pair_out_host /* or NULL */, float* matched_out_host /* or NULL */);
int fdcm_search_exhaustive_detect_all_gated(const fdcm_featuremap* fm, const fdcm_templates* templates,
                                            const fdcm_rotations* rot /* or NULL */, const fdcm_grid* grid, float max_score,
                                            int32_t max_detections, int32_t overlap_permille, int32_t margin, int penalty, float tau,
                                            float min_matched, int gate, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                            int32_t* boxes_out /* 4 max_detections, or NULL */,
                                            float* matched_out /* max_detections, or NULL */);
int fdcm_search_exhaustive_detect_windows_gated(const fdcm_featuremap* fm, const fdcm_templates* templates,
                                                const fdcm_rotations* rot /* or NULL */, const fdcm_pose_window* jobs, int64_t n_jobs,
                                                int32_t sx, int32_t sy, int32_t wrap, float max_score, int32_t max_detections,
                                                int32_t overlap_permille, int32_t margin, int penalty, float tau, float min_matched,
                                                int gate, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                                int32_t* boxes_out /* 4 max_detections, or NULL */,
                                                float* matched_out /* max_detections, or NULL */,
                                                int32_t* jobs_out /* max_detections, or NULL */);

/* Objects: templates carry an object label, and every stage keeps a best pair per (grid point, object) instead of per grid
 * point.  A set is usually many views of a few parts: with one pair per point two parts at one translation compete for the
 * point, one threshold serves parts of every size, and one overlap limit serves suppression within a part and across parts.
 * The definitions are this project's (README.md, "Objects"; numpy statement: tests/objects_ref.py).  Everything not restated
 * here is taken unchanged from fdcm_search_exhaustive_detect_all_gated, fdcm_best_map_gated and
 * fdcm_search_exhaustive_detect_windows_gated: score, caps, admissibility, rot == NULL, q, its denominators and pairkey,
 * footprints with margin, I and U in int64, len_i, cap_i, matched, ML, TL_t and frac, the record layout and both gates.
 * Inputs: objects, n_templates int32 with objects[t] in [0, G), G = n_objects, 1 <= G <= 256 (an object may hold no template,
 * or only templates without lines: its plane is empty); max_score, G float32, each >= +0 or +inf; min_matched, G float32 in
 * [0, 1], NULL meaning all 0; overlap_permille and cross_permille, 0 .. 1000; gate, margin, penalty, tau, max_detections
 * (1 .. 4096) and tmpl_index_base as in the siblings.
 * Candidates: the candidates of an entry (g, o) are the pairs u = (t, a) with objects[t] = o of templates with lines,
 * admissible at g, with q not NaN; under FDCM_GATE_ALL also ML(u, t_g) >= need_t, need_t = float32(min_matched[objects[t]] *
 * TL_t).  best(g, o) is the candidate of the smallest pairkey.  Under FDCM_GATE_WINNER the entry is dropped unless
 * ML(best(g, o), t_g) >= need; as in the sibling, only that pair is looked at.
 * Object best map (fdcm_best_map_objects): three planes [G][ny][nx], row-major: q(best(g, o)), u(best(g, o)) and
 * frac(best(g, o), t_g); NaN, -1 and NaN mark entries without a candidate.  Any plane may be NULL, not all three.  There is no
 * gate argument: as in fdcm_best_map_gated, min_matched[o] > 0 restricts the minimum.
 * Dense detections (fdcm_search_exhaustive_detect_objects): S_0 is the set of entries (g, o) that have a candidate, pass the
 * gate and have q(best(g, o)) <= max_score[o].  Order: key(g, o) = (bits of q, g, u), u = best(g, o), compared
 * lexicographically: a total order, because the pairs of different objects differ; the label does not enter.  Footprint:
 * F(g, o) = box(best(g, o)) + t_g.  Greedy rule: d_n is the smallest entry of S_n and S_(n+1) = S_n \ {d_n} \ {e : d_n
 * suppresses e}, where d = (g_d, o_d) suppresses e = (g, o) when 1000 I > overlap_permille U and o = o_d, or when 1000 I >
 * cross_permille U and o != o_d; the rule stops at max_detections or when S_n is empty.  Output: the d_n in order, as the
 * sibling's records, with optional boxes_out and matched_out.  The object of a record is objects[tmpl_idx - tmpl_index_base].
 * Windows (fdcm_search_exhaustive_detect_windows_objects): job j's object is objects[tmpl_j]; its winner, q_j, key(j) and
 * footprint are the sibling's; the threshold is max_score[o_j], the need comes from min_matched[o_j], and the suppression
 * test is the two-limit test above.  The outputs are the sibling's, jobs_out included.
 * Identities: G = 1 gives the bytes of the siblings at max_score[0], min_matched[0] and the same gate, whatever
 * cross_permille is.  cross_permille = 1000 with max_detections not reached: objects do not interact, and the records are
 * those of the sibling run once per object on that object's templates, merged in the order (score bits, g, u); plane o of the
 * object best map is fdcm_best_map_gated of object o's sub-set with pairs mapped back.  One-point window jobs for every keyed
 * entry of the object best map, listed by ascending (g, u), give the dense call's records.  Relabelling the objects by a
 * bijection, the per-object arrays permuted alike, changes no output byte.  With one max_score for all objects the records
 * for any max_score are the leading records with score <= max_score of the +inf list.  overlap_permille = cross_permille = 0:
 * no two returned boxes share a pixel.  Every record's fraction is fdcm_matched_fractions of its pose, bit for bit, and its
 * ML >= need.  Results are a function of the inputs alone.
 * FDCM_EINVAL, before any GPU work: everything the siblings reject; n_objects outside 1 .. 256; objects NULL with templates,
 * or an entry outside [0, G); max_score NULL, or an entry NaN or < 0; a min_matched entry NaN or outside [0, 1];
 * cross_permille outside 0 .. 1000; n_objects * nx * ny > 2^26 in the dense calls.  That bound holds G key planes of 8 bytes
 * per point in whole 16 x 64 sub-tiles: a grid much narrower than 16 or much lower than 64 points pads each plane by up to
 * those factors.  Empty inputs give FDCM_OK and nothing.  The calls block; concurrent callers of one feature map take turns. */
int fdcm_best_map_objects(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                          const fdcm_grid* grid, int penalty, float tau, const int32_t* objects /* n_templates */, int32_t n_objects,
                          const float* min_matched /* n_objects, or NULL */, float* score_out_host /* n_objects ny nx, or NULL */,
                          int32_t* pair_out_host /* or NULL */, float* matched_out_host /* or NULL */);
int fdcm_search_exhaustive_detect_objects(const fdcm_featuremap* fm, const fdcm_templates* templates,
                                          const fdcm_rotations* rot /* or NULL */, const fdcm_grid* grid,
                                          const int32_t* objects /* n_templates */, int32_t n_objects,
                                          const float* max_score /* n_objects */, const float* min_matched /* n_objects, or NULL */,
                                          int32_t max_detections, int32_t overlap_permille, int32_t cross_permille, int32_t margin,
                                          int penalty, float tau, int gate, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                          int32_t* boxes_out /* 4 max_detections, or NULL */,
                                          float* matched_out /* max_detections, or NULL */);
int fdcm_search_exhaustive_detect_windows_objects(const fdcm_featuremap* fm, const fdcm_templates* templates,
                                                  const fdcm_rotations* rot /* or NULL */, const fdcm_pose_window* jobs, int64_t n_jobs,
                                                  int32_t sx, int32_t sy, int32_t wrap, const int32_t* objects /* n_templates */,
                                                  int32_t n_objects, const float* max_score /* n_objects */,
                                                  const float* min_matched /* n_objects, or NULL */, int32_t max_detections,
                                                  int32_t overlap_permille, int32_t cross_permille, int32_t margin, int penalty,
                                                  float tau, int gate, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                                  int32_t* boxes_out /* 4 max_detections, or NULL */,
                                                  float* matched_out /* max_detections, or NULL */,
                                                  int32_t* jobs_out /* max_detections, or NULL */);

/* Hull footprints: a second footprint shape for the overlap rule, chosen per template set.  The box of an elongated part
 * changes with its angle and is mostly empty at 45 degrees, so two parallel rods that share no pixel suppress each other
 * there and not at 0 degrees; the hull of the posed end points turns with the part.  The definitions are this project's
 * (README.md, "Hull footprints"; numpy statement: tests/hull_ref.py).  Everything not restated is taken unchanged from
 * "Detections suppressed by footprint overlap" and its descendants: candidates, q, keys, the greedy rule, both limits of the
 * objects' rule, records, gates, boxes_out.
 * Kind: FDCM_FOOTPRINT_BOX (0, the default: today's rule) or FDCM_FOOTPRINT_HULL (1), a property of the template set
 * (fdcm_templates_create_shaped; fdcm_templates_create and _create_capped make BOX sets).
 * Vertices of a pair u = (t, a): the posed end points the searches score (float32; rot == NULL: the caller's lines as they
 * are); with margin m each end point v contributes the four corners (floor(v.x) -+ m, floor(v.y) -+ m), every coordinate
 * floored in int64 and clamped to [-2^25, 2^25] after the margin, which is the box's own arithmetic.  A template without lines,
 * or with a NaN end point, has the empty shape; it is never a candidate.
 * Shape P(u): the integer points of the closed convex hull of the vertices, stated row by row without a hull.  For an
 * integer y between the least and the greatest vertex y take all ordered vertex pairs (p, q), p = q included, with p.y <= y
 * <= q.y: a pair with p.y = q.y contributes both x, any other x* = p.x + (q.x - p.x)(y - p.y) / (q.y - p.y) as an exact
 * rational.  xl(y) = ceil(min x*), xr(y) = floor(max x*); the row holds the pixels xl .. xr and is empty when xl > xr (a
 * segment that passes between lattice points).  All products stay below 2^55: exact in int64.
 * Consequences: the bounding box of P(u) is the box of fdcm_templates_footprints at the same margin, so boxes_out and
 * fdcm_templates_footprints do not change for a hull set; A(u) = |P(u)| >= 1 for a pair with lines and no NaN.
 * Overlap: F(g) = P(best(g)) + t_g;  I(g, h) = |F(g) n F(h)|, the sum over common rows of max(0, min(xr) - max(xl) + 1);
 * U = A(g) + A(h) - I;  h suppresses g when 1000 I > permille U, in int64, permille being overlap_permille within an object
 * and cross_permille across objects.
 * Identities: (1) a BOX set gives the bytes it gave before hull sets existed, in every call.  (2) overlap_permille = 1000 (and
 * cross_permille = 1000) gives the BOX records, whatever the kind.  (3) A set in which every template's posed end points
 * include the four corners of their own bounding box gives the BOX records at any margin and overlap.  (4) overlap = cross
 * = 0: no two returned shapes share a pixel (their boxes may).  (5) Identity (3) of "Objects" holds for a hull set.  (6)
 * Results are a function of the inputs alone.  (7) n_objects = 1 gives the calls without objects, byte for byte.
 * Calls that honour the kind: fdcm_search_exhaustive_detect_nms, _detect_all, _detect_all_matched, _detect_all_gated,
 * _detect_objects, _detect_windows, _detect_windows_gated, _detect_windows_objects, and fdcm_matches_detect_objects ("Match
 * lists: objects and hull shapes").  fdcm_search_exhaustive_detect (radius), fdcm_matches_detect, every call without an overlap,
 * fdcm_search, the pipeline and the shards ignore it.
 * Span tables: fdcm_templates_footprint_spans and fdcm_lines_footprint_spans (host only, whatever the set's kind) give the
 * shapes of every pair u = t n + a.  row_offsets: P + 1 int64 (P = T n); pair u has the rows row_offsets[u] ..
 * row_offsets[u + 1], row r at y = box(u).y0 + (r - row_offsets[u]); areas: P int64, or NULL; spans: 2 int32 (xl, xr) per row
 * in the frame of the box, (0, -1) for an empty row, or NULL to get offsets and areas only.
 * FDCM_EINVAL, before any device work: footprint not 0 or 1; row_offsets NULL; everything the siblings reject; in the dense
 * detection calls on a hull set a span table (the rows of every pair of the call) of more than 2^26 rows.  The windows'
 * calls build the shapes of the winners that enter S_0 alone and apply the same limit to them once they are known. */
#define FDCM_FOOTPRINT_BOX 0
#define FDCM_FOOTPRINT_HULL 1
int fdcm_templates_create_shaped(const float* lines, const int64_t* offsets, int64_t n_templates, const float* caps /* or NULL */,
                                 int32_t footprint, fdcm_templates** out);
int fdcm_templates_footprint_kind(const fdcm_templates* t, int32_t* kind);
int fdcm_templates_footprint_spans(const fdcm_templates* t, const fdcm_rotations* rot /* or NULL */, int32_t margin,
                                   int64_t* row_offsets, int64_t* areas /* or NULL */, int32_t* spans /* or NULL */);
int fdcm_lines_footprint_spans(const float* lines, const int64_t* offsets, int64_t n_templates, const fdcm_rotations* rot /* or NULL */,
                               int32_t margin, int64_t* row_offsets, int64_t* areas /* or NULL */, int32_t* spans /* or NULL */);

/* ---- line segments from images (not in the reference, which reads its lines from .scene / .tmpl files; the definitions are
 *      this project's: README.md, "Line segments from images"; numpy statement: tests/lines_ref.py).  From a label image as
 *      fdcm_edge_labels makes it (m = the distinct keys of `depth`, a byte < m an edge pixel of that label, labels circular)
 *      to the segments of its straight runs, on the device.
 * With w = bucket and h = w / 2, an edge pixel of label l has bucket l / w in partition A and ((l + h) mod m) / w in
 * partition B.  Per partition a component is a maximal 8-connected set of edge pixels of equal bucket; n(C) is its pixel
 * count and its root the smallest index y * width + x among its pixels.  Pixel p votes A when n(A(p)) >= n(B(p)), else B;
 * votes(C) counts the pixels of C that voted for C's partition.  C is kept when 2 votes(C) > n(C),
 * min_pixels <= n(C) <= 65535 and its length is at least min_length.
 * The fit is over all pixels of C, exact in int64: Sx, Sy, Sxx, Syy, Sxy over absolute pixel coordinates,
 * Dxx = n Sxx - Sx^2, Dyy = n Syy - Sy^2, Dxy = n Sxy - Sx Sy; C is x-major when Dxx >= Dyy.  x-major: x0 = min x,
 * x1 = max x, s = f64(Dxy) / f64(Dxx), xb = f64(Sx) / f64(n), yb = f64(Sy) / f64(n), Y(x) = yb + s * (f64(x) - xb), every
 * operation one unfused IEEE float64 operation; the segment is (f32(x0), f32(Y(x0)), f32(x1), f32(Y(x1))) and the length
 * x1 - x0 + 1.  y-major: the same with x and y exchanged and s = f64(Dxy) / f64(Dyy): (f32(X(y0)), f32(y0), f32(X(y1)),
 * f32(y1)), length y1 - y0 + 1.
 * Output: the kept components' segments, 4 floats each (x1 y1 x2 y2, the LineArray record), in ascending
 * 2 * root + partition (A = 0, B = 1).  Coordinates are image pixels: scene coordinates of a feature map built from the
 * same frame, and what fdcm_templates_create takes.  The result is a function of the label image alone.  With bucket = 1
 * the partitions coincide and the result is the same-label components.
 * Both calls block, run on the current device and need no handle.  *lines is released with fdcm_lines_free; when nothing is
 * kept it is NULL, *n_lines is 0 and the call returns FDCM_OK.  1 <= width, height <= 4096; depth >= 1 with at most 255
 * keys; on_device: the pixels are host memory (0) or memory of the current device (1; labels without gaps between rows).
 * fdcm_lines_from_image is fdcm_edge_labels_ex followed by fdcm_lines_from_labels without the label image leaving the
 * device; edge = {0, t, t, 1} is the plain threshold t. ---- */
typedef struct fdcm_line_params {
    int32_t bucket;      /* labels per orientation bucket, 1 .. m */
    int32_t min_pixels;  /* 2 .. 65535 */
    int32_t min_length;  /* 1 .. 4096, pixels along the major axis */
} fdcm_line_params;
int fdcm_lines_from_labels(const uint8_t* labels, int64_t width, int64_t height, int on_device, int64_t depth,
                           const fdcm_line_params* params, float** lines, int64_t* n_lines);
int fdcm_lines_from_image(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device,
                          int64_t depth, const fdcm_edge_params* edge, const fdcm_line_params* params,
                          float** lines, int64_t* n_lines);
/* Diagnostic, not part of the extraction: device times of the calling thread's last fdcm_lines_from_* call in milliseconds,
 * from events the call records around its stages (eleven events per call, whether or not this is read).  Each figure is the
 * time of that stage's kernels alone: the edge kernels (0 for labels), the union-find inside tiles, across tile borders,
 * flatten + numbering of the roots, sums, votes, the keep rule with its scan, the fit.  The host work between stages -- the
 * two counts read back, the buffers sized by them and their clearing -- is in none of them; total_ms spans the call's device
 * work from its first kernel to its last with those gaps.  A stage the call did not reach (nothing to keep) and a time that
 * could not be read are 0. */
typedef struct fdcm_lines_timing {
    float edges_ms, tiles_ms, borders_ms, number_ms, sums_ms, votes_ms, keep_ms, fit_ms, total_ms;
    int64_t n_lines;
} fdcm_lines_timing;
int fdcm_lines_last_timing(fdcm_lines_timing* out);

/* ---- the reference's line files (.lines / .scene / .tmpl): read / write of core/serialization.h:99-132 (Python: openfdcm.read
 *      / openfdcm.write, python/src/core.cpp:41-42).  Host only.  fdcm_lines_read hands out n lines as 4 floats each
 *      (x1 y1 x2 y2 = the 4 x N column-major LineArray), to be released with fdcm_lines_free; a missing file, a file that is
 *      not a line file and an unknown line data format are FDCM_EINVAL with the reference's message in fdcm_last_error().
 *      fdcm_lines_write replaces an existing file, as the reference does. ---- */
int fdcm_lines_read(const char* path, float** lines, int64_t* n_lines);
int fdcm_lines_write(const char* path, const float* lines, int64_t n_lines);
void fdcm_lines_free(float* lines);

/* ---- Scene coverage: which edge pixels of a label image a pose explains, and the label image without them (not in the
 *      reference).  Every other cue runs from the template to the scene -- does each template line lie on scene edges? --, and
 *      in dense texture the answer is yes for any template of few lines.  This one runs from the scene to the template: of the
 *      edge pixels inside a detection's footprint, how many does the posed template account for?  Near all of them for a part
 *      lying alone, few for a hit in clutter.  The same decision per pixel gives the residual: the labels without the pixels
 *      the accepted detections explain, which fdcm_featuremap_rebuild_labels turns into the map of the next round of a
 *      detect, explain away, detect again loop.  All arithmetic is integer; the results are a function of the inputs alone,
 *      whatever order the GPU visits pixels in.  The definition in plain Python integers: tests/coverage_ref.py.
 *
 *      Inputs.  fm is used for its size (W, H), its scene translation T, its m keys and the admissibility rule; the volume is
 *      not read.  labels is a label image as fdcm_edge_labels makes it, width x height bytes without gaps: a byte < m is an
 *      edge pixel of that slice, anything else is no edge.  templates, rot (or NULL) and the n poses (tmpl, a, x, y) are
 *      fdcm_line_costs'.
 *      Frames.  T must be whole pixels, T = (bx, by) with integers bx, by >= 0, and width + 2 bx == W, height + 2 by == H: any
 *      map built from an image or from labels (bx = by = border).  Label pixel (px, py) is map pixel (px + bx, py + by) and
 *      scene point (px, py).
 *      Segment of line i of pair u = (tmpl, a) at (x, y): it joins the two map pixels A_i, B_i whose integral values the line's
 *      cost subtracts -- fdcm_line_costs' rule for the (rotated) line at offset T + t, truncation included --, moved to the
 *      label frame by -(bx, by); its bin b_i is the slice that line reads.
 *      Window of pose q: F = box(tmpl, a) + (x, y), the box fdcm_templates_footprints gives at `margin`, intersected with
 *      [0, width - 1] x [0, height - 1]; it may be empty.  The footprint kind of a set with hull footprints is ignored.
 *      Explained.  An edge pixel P with label l is explained by pose q when some line i of the pair passes both tests:
 *        min(|l - b_i|, m - |l - b_i|) <= bin_tolerance;
 *        the squared distance from P to the segment A_i B_i is <= radius^2, decided exactly in int64: with d = B - A,
 *        w = P - A, dot = w.d and len2 = d.d: if dot <= 0 (also A = B): w.w <= r^2; else if dot >= len2: |P - B|^2 <= r^2;
 *        else cross^2 <= r^2 len2 with cross = w.x d.y - w.y d.x.
 *      Counts.  For an admissible pose, edges[q] is the number of edge pixels in its window and explained[q] the number of
 *      those explained by pose q itself; a template without lines has an empty window: (0, 0).  A pose that is not admissible
 *      for (tmpl, a) gives (-1, -1) and explains nothing.
 *      Residual (optional): the labels, with 255 at every edge pixel P that some admissible pose q of the list has in its
 *      window and explains.  Duplicate poses change nothing.  residual_out must not overlap labels.
 *      Identities: explained <= edges; explained does not fall when radius or bin_tolerance grows at a fixed margin; with
 *      bin_tolerance = m / 2 the labels' values stop mattering beyond "is an edge"; the residual of the concatenation of two
 *      pose lists is the per-pixel "255 if either" of the two residuals; a label image without edges gives (0, 0) for
 *      admissible poses and itself as residual.
 *      FDCM_EINVAL, before any GPU work: what fdcm_line_costs rejects about n, poses, rot, pivots and the handles; n > 2^20;
 *      params NULL, radius outside 0 .. 32, bin_tolerance < 0 or > m / 2, margin outside 0 .. 4096; labels NULL, width or
 *      height outside 1 .. 4096; counts_out NULL with n > 0; a map whose scene translation is not whole non-negative pixels, or
 *      whose size is not (width + 2 bx, height + 2 by) -- the message names which.  n = 0 writes the residual, a copy, and
 *      returns FDCM_OK; so does an empty feature map (no pixels or no keys: it has no frame to check) or an empty template
 *      set, which leave the counts unwritten as the siblings do.  The call blocks.  on_device = 1: labels and residual_out are memory of the handle's device, and labels is read in
 *      place.  The buffers are the handle's own, not the workspace the exhaustive calls share. ---- */
typedef struct fdcm_coverage_params {
    int32_t radius;         /* 0 .. 32 pixels */
    int32_t bin_tolerance;  /* 0 .. m / 2 slices, circular */
    int32_t margin;         /* 0 .. 4096: the footprint's margin */
} fdcm_coverage_params;     /* 12 bytes */
int fdcm_scene_coverage(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int on_device,
                        const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                        const int32_t* poses /* n x 4: tmpl, a, x, y */, int64_t n, const fdcm_coverage_params* params,
                        int32_t* counts_out /* n x 2: edges, explained (host) */,
                        uint8_t* residual_out /* width * height, or NULL; device memory when on_device = 1 */);

/* ---- Scene selection: greedy explain-away over a pose list (not in the reference).  Every detector resolves conflicts
 *      between hypotheses by the template's geometry: radius, box IoU, hull overlap.  For parts that interlock or lie on each
 *      other that is the wrong question: two poses conflict when they claim the same scene edges, not when their boxes
 *      overlap.  This call is the greedy rule of fdcm_search_exhaustive_detect_nms with "footprints overlap" replaced by
 *      "claims the same edge pixels": it takes a pose list in priority order, accepts a pose when enough of what it explains
 *      is not yet claimed by the poses accepted before it, and returns the accepted poses and the residual.  All arithmetic is
 *      integer; the result is a function of the inputs alone, whatever order the GPU visits pixels or poses in.  The rule in
 *      plain Python: tests/select_ref.py, on tests/coverage_ref.py.
 *
 *      Everything not restated is Scene coverage's, unchanged: the inputs and the frame check, segments, bins and windows at
 *      `margin`, "explained" (exact in int64), admissibility, the poses (tmpl, a, x, y) with rot == NULL meaning the lines as
 *      they are.
 *      Per pose q: E_q is the set of edge pixels in its window that it explains; edges_q and explained_q = |E_q| are the two
 *      counts fdcm_scene_coverage returns for it.
 *      Order.  The list order is the priority: pose 0 first.  Detection records ascend by key, so the poses of a detection list
 *      are best first.
 *      Candidates S_0: the admissible poses with explained_q >= min_pixels and
 *      1000 explained_q >= min_coverage_permille * edges_q (int64).
 *      Rule.  C, the set of claimed pixels, is empty at the start.  For q = 0, 1, .., n - 1, stopping once max_selected poses
 *      are accepted: skip q when it is not in S_0; new_q = |E_q \ C|; q is accepted when new_q >= min_pixels and
 *      1000 new_q >= min_new_permille * explained_q (int64); on acceptance C = C u E_q.
 *      Output.  *n_out = k, the number accepted; selected_out[0 .. k) their indices into the list, ascending; counts_out
 *      k x 3 values (edges, explained, new), new as at acceptance; entries from k on are not written.  residual_out
 *      (optional): the labels with 255 at every pixel of the final C.  The caller supplies max_selected entries of
 *      selected_out and 3 max_selected of counts_out.
 *      Identities: the residual is fdcm_scene_coverage's residual of the list poses[selected], and the first two columns of
 *      counts_out are that call's counts; the new column sums to the number of bytes in which the residual differs from the
 *      labels, and the first record has new == explained; the result for max_selected = k is the first k entries of the
 *      result for any larger value; a duplicate of an accepted pose is never accepted (new = 0 < min_pixels); with
 *      min_new_permille = 1000 the accepted poses' explained sets are pairwise disjoint; with min_coverage_permille =
 *      min_new_permille = 0 and min_pixels = 1 a pose is accepted exactly when it explains a pixel nobody before it claimed,
 *      and the residual is fdcm_scene_coverage's of the whole list; one fdcm_scene_coverage call per candidate on the
 *      running residual, after one on the labels for the static test, selects the same poses (explained on the running
 *      residual is new).
 *      Rounds.  edges_q and explained_q are fixed and new_q only falls as C grows, so a candidate that fails its test against
 *      any subset of the final C before its turn also fails at its turn.  The device counts everything once; then, per
 *      accepted pose d, it claims E_d, recounts only the surviving later candidates whose window meets d's window, drops
 *      those that now fail, and accepts the first survivor next.  A round is three launches; rounds are queued 64 at a time
 *      between host synchronisations, and the call stops at the first batch that ends with no survivor.
 *      Measured on one MI355X (tools/select_bench.py, profiles/select_bench_config2p.json; a 1024 x 1024 frame, 100 templates
 *      of 32 lines, radius 2, bin_tolerance 1, min_new_permille 500, labels and residual on the device, median of 5 calls):
 *      1024 candidates, 44 accepted: 3.52 ms, against 76.9 ms for the composition available before, one fdcm_scene_coverage
 *      call per candidate on the running residual; 64 candidates, 7 accepted: 0.71 ms against 5.10 ms.  Not measured: lists
 *      of more than 1024 candidates, calls that accept more than 64 poses, poses with rotations, hardware counters.
 *      FDCM_EINVAL, before any GPU work: everything fdcm_scene_coverage rejects, with its messages (counts_out aside); sel
 *      NULL, min_coverage_permille or min_new_permille outside 0 .. 1000, min_pixels outside 1 .. 2^24, max_selected outside
 *      1 .. 4096; selected_out, counts_out or n_out NULL.  n = 0, an empty feature map or an empty template set give
 *      *n_out = 0, a residual that is a copy, and FDCM_OK.  The call blocks.  on_device is fdcm_scene_coverage's.  The buffers
 *      are the handle's coverage buffers, not the workspace the exhaustive calls share. ---- */
typedef struct fdcm_select_params {
    int32_t min_coverage_permille;  /* 0 .. 1000: the static test, explained / edges */
    int32_t min_new_permille;       /* 0 .. 1000: at the pose's turn, new / explained */
    int32_t min_pixels;             /* 1 .. 2^24: explained and new at least this */
    int32_t max_selected;           /* 1 .. 4096 */
} fdcm_select_params;               /* 16 bytes */
int fdcm_scene_select(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int on_device,
                      const fdcm_templates* templates, const fdcm_rotations* rot /* or NULL */,
                      const int32_t* poses /* n x 4: tmpl, a, x, y, in priority order */, int64_t n,
                      const fdcm_coverage_params* params, const fdcm_select_params* sel,
                      int32_t* selected_out /* max_selected (host) */,
                      int32_t* counts_out /* max_selected x 3: edges, explained, new (host) */, int64_t* n_out,
                      uint8_t* residual_out /* width * height, or NULL; device memory when on_device = 1 */);

/* ---- Match lists: the records of fdcm_search, verified and suppressed on the device.  No counterpart in the reference; these
 *      definitions are the project's own.  fdcm_search, the frame pipeline, the sharded engine and fdcm_topk return records
 *      {tmpl_idx, score, transform[6]} whose transform is a free float matrix; every detection call above takes poses
 *      (tmpl, a, x, y), which only the exhaustive calls produce.  These calls are the detection family's line costs, matched
 *      fraction, caps, threshold and greedy overlap rule for such records: a caller of fdcm_search gets a record for every
 *      pair of aligned lines near a true pose, and fdcm_matches_detect reduces the list to one record per part.  The rule in
 *      numpy: tests/match_ref.py.
 *
 *      r is a record, t = r.tmpl_idx - tmpl_index_base, M = r.transform (row-major 2 x 3), T the set's template count.
 *      Valid record: 0 <= t < T.  Any other record takes part in nothing: its outputs are NaN, its box is empty and it is
 *      never a candidate, on the host and on the device alike (fdcm_topk's rule, not fdcm_penalize's error).
 *      Posed lines P(r): each end point (x, y) of template t becomes ((M0 x + M1 y) + M2, (M3 x + M4 y) + M5), every product and
 *      sum float32 and unfused: the reference's transform (math.h:341-344).  A NaN or an infinity in M flows through.
 *      Bin of posed line i: closestOrientation(keys, atanf(dy / dx)) of the posed line, as evaluate<Dt3Cpu> classifies a line
 *      it is given (dt3cpu.cpp:144-148).
 *      Admissible: fdcm_featuremap_evaluate of P(r) at translation (0, 0) is not NaN: every posed coordinate plus the scene
 *      translation, summed in float32, lies in (-1, W) x (-1, H).  A NaN coordinate: not admissible.  A valid record whose
 *      template has no lines is admissible.
 *      Line cost cost_i(r): the term of evaluate for posed line i at translation (0, 0), uncapped: bit for bit the score
 *      fdcm_featuremap_evaluate returns for the one-line template {posed line i} at (0, 0).  NaN for every line of a record
 *      that is not admissible.
 *      Score s(r): the sum, in Eigen's sum() order, of capped_i = cost_i > cap_i ? cap_i : cost_i with the set's caps (+inf
 *      without caps); +0 for a template without lines, NaN when r is not admissible.  Without caps s(r) is bit for bit
 *      fdcm_featuremap_evaluate(P(r), (0, 0)).
 *      s(r) is not r.score.  The search scores transform(lines, A) at a translation k v along the scene line and then stores A
 *      with that translation folded into M2 and M5; posing again with the folded matrix rounds differently.  s(r) is usually
 *      close to r.score but is not its bits, and a record on the map's border can come out not admissible.
 *      Matched length and fraction: ML, TL and frac of "Detections by matched fraction": w_i = len_i when cost_i <= cap_i, len_i
 *      the unposed line's length; ML the float32 sum in line order from +0; frac = ML / TL, 1 when TL == 0, NaN when r is not
 *      admissible.
 *      Footprint F(r): the footprint's arithmetic ("Detections suppressed by footprint overlap") on the end points of P(r) at
 *      `margin`: floor(min x) - margin, floor(min y) - margin, floor(max x) + margin, floor(max y) + margin in int64, clamped to
 *      [-2^25, 2^25].  A template without lines, a NaN end point or an invalid record: the empty box (0, 0, -1, -1).  An
 *      infinite end point does not empty the box: its floor is far outside the clamp.  The kind of a hull set is ignored, as
 *      Scene coverage ignores it: the shape is the box (fdcm_matches_detect_objects, below, honours it).
 *      Candidates S_0 of fdcm_matches_detect: the records that are valid with a template that has lines, admissible, whose
 *      q_j = v_j / den(t) is not NaN, has a clear sign bit and is <= max_score, and, when min_matched > 0, have
 *      ML >= need_t = float32(min_matched * TL_t).  v_j = r.score with rescore = 0 and s(r) with rescore = 1; the denominators
 *      are fdcm_penalize's (penalty = -1: q = v).  A caller who has penalised already passes -1 and rescore = 0.
 *      Key, rule, output: key(j) = (bits of q_j << 32) | j, j the record's position in the list.  The greedy rule of
 *      fdcm_search_exhaustive_detect_nms runs on S_0 with these keys and footprints and stops at max_detections (1 .. 4096).
 *      *out receives the d_n in order, each {r.tmpl_idx, q, r.transform} (fdcm_matches_free), *n_out their count; optional
 *      indices_out (the position j of each), boxes_out (4 int32 each) and matched_out (frac), max_detections entries each.
 *      Identities.  With overlap_permille = 1000, max_score = +inf, min_matched = 0, rescore = 0 and max_detections >= |S_0|, on
 *      a list whose records are all candidates, the output is fdcm_topk of the same records at the same penalty with k = n,
 *      byte for byte.  At fixed other parameters the records for any max_score are the leading records with score <= max_score
 *      of the +inf list.  With overlap_permille = 0 no two returned boxes share a pixel.  A duplicate of a returned record is
 *      never returned unless overlap_permille = 1000.  For a record with transform {1, 0, x, 0, 1, y}, x and y integers below
 *      2^24 in magnitude, costs, s and frac are fdcm_line_costs, the k = 1 score of fdcm_search_exhaustive_windows for the job
 *      (t, 0, 1, x, y, 1, 1) and fdcm_matched_fractions for the pose (t, 0, x, y), bit for bit wherever every x_i + float32(x) is
 *      exact.  Results are a function of the inputs alone.
 *      matches: n host records (on_device = 0); n records on the handle's device (on_device = 1), such as a buffer filled by
 *      fdcm_search_device; or NULL with on_device = 0: the records of the last fdcm_search on fm, as fdcm_topk takes them (n
 *      is then ignored).
 *      fdcm_matches_verify: scores_out s(r) and fractions_out frac(r), n floats each; costs_out a regular n x Lmax float32 array,
 *      Lmax the set's largest line count, NaN at and beyond a template's line count.  Any output may be NULL, not all of them.
 *      fdcm_matches_footprints: F(r) of n host records, 4 int32 each; host only, no device is touched.
 *      The device.  One pass, a wave per record and a lane per line, writes every record's score, fraction, box and key
 *      straight into the arrays the rounds of the overlap rule read; the rounds are those of the detections over pose windows,
 *      unchanged; a gather kernel writes the result records into pinned memory.  The list never returns to the host between
 *      them.  Where fdcm_orientation_bins_mode() is 1 the bins are computed on the host and uploaded; device records then cost
 *      one download.
 *      FDCM_EINVAL, before any GPU work: n < 0 or n > 2^22; on_device not 0 or 1; matches NULL with n > 0 and on_device = 1;
 *      max_score NaN or < 0; max_detections outside 1 .. 4096; overlap_permille outside 0 .. 1000; margin outside 0 .. 4096; an
 *      unknown penalty or a tau that is not finite; min_matched NaN or outside [0, 1]; rescore not 0 or 1; out or n_out NULL
 *      (verify: every output NULL; footprints: matches or boxes_out NULL with n > 0); NULL handles.  n = 0, an empty feature
 *      map or an empty template set give FDCM_OK and nothing (*n_out = 0; verify's outputs are not written).  The calls block;
 *      concurrent callers of one feature map take turns. ---- */
int fdcm_matches_footprints(const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int32_t tmpl_index_base,
                            int32_t margin, int32_t* boxes_out /* n x 4 */);
int fdcm_matches_verify(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n,
                        int on_device, int32_t tmpl_index_base, float* scores_out /* n, or NULL */,
                        float* fractions_out /* n, or NULL */, float* costs_out /* n x Lmax, or NULL */);
int fdcm_matches_detect(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n,
                        int on_device, int32_t tmpl_index_base, float max_score, int32_t max_detections, int32_t overlap_permille,
                        int32_t margin, int penalty, float tau, float min_matched, int rescore, fdcm_match** out, int64_t* n_out,
                        int32_t* indices_out /* max_detections, or NULL */, int32_t* boxes_out /* max_detections x 4, or NULL */,
                        float* matched_out /* max_detections, or NULL */);

/* ---- Match lists: objects and hull shapes.  fdcm_matches_detect with the template set's objects and its kind of footprint
 *      (README.md, "Match lists: objects and hull shapes"; the referee is tests/match_objects_ref.py).  Everything not restated
 *      is taken unchanged.  From "Match lists": valid record, P(r), bins, admissibility, cost_i, s(r), ML, TL, frac, F(r), q_j,
 *      key(j) = (bits of q_j << 32) | j, the three input forms, rescore.  From "Objects": objects, G, per-object max_score and
 *      min_matched, cross_permille, the suppression test with two limits.  From "Hull footprints": vertices, the shape row by
 *      row, I, U.
 *      Object of record j: o_j = objects[t_j].
 *      Candidates S_0: the valid records whose template has lines, that are admissible, with q_j not NaN, its sign bit clear,
 *      q_j <= max_score[o_j] and, where min_matched[o_j] > 0, ML >= need_t = float32(min_matched[o_j] * TL_t).
 *      Shape of record j: F(j) = F(r_j) at `margin` for a BOX set.  For a HULL set P(j) is "Hull footprints"' shape on the
 *      vertices of the posed end points P(r_j): float32 posing as fdcm_matches_verify, every coordinate floored in int64, the
 *      four corners -+ margin when margin > 0, clamped to [-2^25, 2^25].  Its bounding box is F(r_j), so boxes_out does not
 *      depend on the kind.
 *      Rule: the greedy rule on S_0 by key, stopping at max_detections.  d suppresses e when 1000 I > overlap_permille U and
 *      o_e = o_d, or when 1000 I > cross_permille U and o_e != o_d; I and U on boxes (BOX set) or on shapes (HULL set), in
 *      int64.
 *      Output: fdcm_matches_detect's: the records {r.tmpl_idx, q, r.transform}, indices_out, boxes_out, matched_out.  The object
 *      of a record is objects[tmpl_idx - base]; there is no separate output for it.
 *      Identities.  (1) G = 1 on a BOX set gives fdcm_matches_detect's bytes at max_score[0] and min_matched[0], whatever
 *      cross_permille is.  (2) With cross_permille = 1000 and max_detections not reached, the records are the merge by key of
 *      fdcm_matches_detect, per object, on the list with every record of another object made invalid (tmpl_idx = base - 1, so
 *      positions stay), for a BOX set.  (3) overlap = cross = 1000 on a HULL set gives the BOX set's records.  (4) A HULL set
 *      whose posed end points always contain the four corners of their bounding box gives the BOX records at any overlap and
 *      margin.  (5) overlap = cross = 0 on a HULL set: no two returned shapes share a pixel (their boxes may).  (6)
 *      Relabelling the objects by a bijection, the per-object arrays permuted alike, changes no byte.  (7) For integer
 *      templates and records {1, 0, x, 0, 1, y} with whole x, y and rescore = 1, the records, boxes and fractions are those of
 *      fdcm_search_exhaustive_detect_windows_objects on the one-point jobs (t, 0, 1, x, y, 1, 1) in list order, on the same set
 *      at the same thresholds with rot NULL, byte for byte.  (8) With one max_score for all objects, the records for any
 *      max_score are the leading records with score <= max_score of the +inf list.  (9) The three input forms give the same
 *      bytes; results are a function of the inputs alone.
 *      Span tables, fdcm_lines_footprint_spans' layout with one shape per record: fdcm_matches_footprint_spans (host only,
 *      whatever the set's kind) gives the shape of every record, no rows for an invalid one; fdcm_matches_shapes gives the
 *      same table from the device kernel for the records that are valid and admissible on fm and whose template has lines,
 *      the others with no rows and area 0 (matches NULL is no form of it: n sizes the outputs).
 *      The device.  The pass of fdcm_matches_detect with a threshold and a need per template (its object's) writes the object of
 *      every record beside its key and box.  On a HULL set a scan over the candidates' box heights gives every candidate its
 *      rows of the span table, and one 8-byte read brings their total to the host; k_matches_shapes, a wave per candidate,
 *      then builds rows and area by gift wrapping over the posed end points, in int64 throughout.  The rounds are the list form
 *      of the detections over pose windows with objects and shapes, unchanged; the list never returns to the host.
 *      FDCM_EINVAL, before any GPU work: everything fdcm_matches_detect rejects; n_objects outside 1 .. 256; max_score NULL, or
 *      an entry NaN or < 0; an entry of min_matched NaN or outside [0, 1]; cross_permille outside 0 .. 1000; objects NULL for a
 *      set with templates, or an entry outside [0, n_objects); row_offsets NULL.  After the pass, on a HULL set and in
 *      fdcm_matches_shapes: a span table of the candidates of more than 2^26 rows ("cut the list with max_score or fdcm_topk
 *      first").  Empty inputs give FDCM_OK and nothing (row_offsets and areas all 0). ---- */
int fdcm_matches_detect_objects(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n,
                                int on_device, int32_t tmpl_index_base, const int32_t* objects /* T */, int32_t n_objects,
                                const float* max_score /* G */, const float* min_matched /* G, or NULL */, int32_t max_detections,
                                int32_t overlap_permille, int32_t cross_permille, int32_t margin, int penalty, float tau, int rescore,
                                fdcm_match** out, int64_t* n_out, int32_t* indices_out /* max_detections, or NULL */,
                                int32_t* boxes_out /* max_detections x 4, or NULL */, float* matched_out /* max_detections, or NULL */);
int fdcm_matches_footprint_spans(const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int32_t tmpl_index_base,
                                 int32_t margin, int64_t* row_offsets /* n + 1 */, int64_t* areas /* n, or NULL */,
                                 int32_t* spans /* 2 per row, or NULL */);
int fdcm_matches_shapes(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int on_device,
                        int32_t tmpl_index_base, int32_t margin, int64_t* row_offsets /* n + 1 */, int64_t* areas /* n, or NULL */,
                        int32_t* spans /* 2 per row, or NULL */);

/* ---- Match lists: scene coverage and selection.  fdcm_scene_coverage and fdcm_scene_select for match records instead of
 *      poses: the cue that runs from the scene to the template, for the records of fdcm_search.  Every definition not restated
 *      here is "Scene coverage"'s and "Scene selection"'s, unchanged; "Match lists"' definitions apply unchanged: valid record,
 *      posed lines P(r), bin of a posed line, admissible, footprint F(r).  The referee is tests/match_coverage_ref.py.
 *      Frames.  The frame check is scene coverage's, with its messages: T = (bx, by) whole and non-negative, width + 2 bx == W
 *      and height + 2 by == H.  A transform maps template coordinates to scene coordinates, so a record does not depend on the
 *      map it was searched on; scene point = label pixel.
 *      Segment of line i of record r: it joins the two map pixels whose integral values cost_i(r) subtracts -- each end point
 *      of P(r) plus the scene translation, summed in float32 and truncated, exactly the pixel fdcm_matches_verify reads -- moved
 *      to the label frame by -(bx, by).  Its bin is the posed line's: closestOrientation of atanf(dy / dx) of the posed line.
 *      Window of r: F(r) at params->margin by the footprint arithmetic of fdcm_matches_footprints, cut to
 *      [0, width - 1] x [0, height - 1]; it may be empty.
 *      Explained: scene coverage's test on these segments, bins and window, exact in int64.
 *      Counts: an admissible record gives (edges, explained); a valid record whose template has no lines is admissible with the
 *      empty box and gives (0, 0); an invalid record or one that is not admissible gives (-1, -1), explains nothing and is never
 *      a candidate.  Residual: scene coverage's, over the admissible records of the list.
 *      Selection: E_j, S_0, the rule, the outputs and fdcm_select_params are scene selection's with "pose q" read as "record j";
 *      the list order is the priority (fdcm_matches_detect with overlap_permille = 1000 returns a list that ascends by key).
 *      matches: the forms of fdcm_matches_detect -- n host records (matches_on_device = 0), n records on the handle's device
 *      (1), or NULL with matches_on_device = 0 for the records of the last fdcm_search on fm.  Labels and residual on the host
 *      or the device (labels_on_device) are scene coverage's on_device, independent of the records' form.
 *      Identities.  For a record {1, 0, x, 0, 1, y} with integers |x|, |y| < 2^24, wherever every x_i + float32(x) is exact,
 *      counts and residual are fdcm_scene_coverage's for the pose (t, 0, x, y) with rot NULL and the same parameters, byte for
 *      byte, and the selection is fdcm_scene_select's.  Scene coverage's and scene selection's identities carry over.  The
 *      segment end points of an admissible record are the pixels at which fdcm_featuremap_evaluate reads the one-line template
 *      {posed line i} at (0, 0).  Results are a function of the inputs alone: the three forms of matches give the same bytes,
 *      and so do the host's bins (fdcm_orientation_bins_mode() == 1) wherever they equal the device's.
 *      The device.  One pass, a wave per record and a lane per line (the verify pass's own posing, admissibility and box code),
 *      writes every record's segments' lines, bins and window into the table scene coverage's kernels read; a scan makes the
 *      strip offsets; only the number of strips comes to the host.  Coverage walks a long list in parts of at most 768 MB of
 *      table, one record never cut; selection keeps its table whole, hence its bound on n.
 *      FDCM_EINVAL, before any GPU work, each with its own message: n < 0; n > 2^20 (coverage) or n > 2^16 (select: cut a longer
 *      list with fdcm_matches_detect first; so is a selection whose table, n x Lmax lines of 20 bytes, would exceed 2 GB);
 *      matches_on_device not 0 or 1; matches NULL with n > 0 and matches_on_device = 1;
 *      then everything fdcm_scene_coverage or fdcm_scene_select rejects about params, labels, sizes, sel, the outputs, the overlap
 *      of residual and labels, the handles and the frame.  n = 0, an empty map or an empty template set give FDCM_OK, the
 *      residual as a copy and *n_out = 0; counts_out is not written.  The calls block; concurrent callers of one feature map
 *      take turns. ---- */
int fdcm_matches_coverage(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int labels_on_device,
                          const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int matches_on_device,
                          int32_t tmpl_index_base, const fdcm_coverage_params* params, int32_t* counts_out /* n x 2 */,
                          uint8_t* residual_out /* width * height where the labels are, or NULL */);
int fdcm_matches_select(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int labels_on_device,
                        const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int matches_on_device,
                        int32_t tmpl_index_base, const fdcm_coverage_params* params, const fdcm_select_params* sel,
                        int32_t* selected_out /* max_selected */, int32_t* counts_out /* max_selected x 3 */, int64_t* n_out,
                        uint8_t* residual_out /* width * height where the labels are, or NULL */);

/* ---- Match lists: refinement.  Every record of a match list searched exhaustively in a small box of (delta rotation, dx, dy)
 *      around its own transform and replaced by its best pose, on the device in one call (README.md, "Match lists: refinement";
 *      the referee is tests/refine_ref.py).  fdcm_search takes a record's rotation from one aligned pair of lines and its
 *      translation from a walk along one scene line, so a record near a true pose is typically a degree or two and a few
 *      pixels off; the calls above judge it at that pose.  This is the pose windows' answer for records whose transform is a
 *      free float matrix: fdcm_matches_refine, then fdcm_matches_detect.  "Match lists"' definitions apply unchanged: matches, n,
 *      on_device and tmpl_index_base (matches NULL with on_device = 0: the records of the last fdcm_search on fm), valid record,
 *      t, M, the set's caps.
 *      Delta table: rot holds na = rot->n pairs (c, s) and optional pivots, one per template, in template coordinates (NULL:
 *      the origin); all values finite.  rot NULL: na = 1 and nothing is rotated.
 *      Lines of run position e: Q_e(t) is the rotated template of "Rotations" for (c, s) = cs[e] and the pivot of t: each end
 *      point goes to ((c x + (-s) y) + m.x, (s x + c y) + m.y), float32, unfused.  P_e(r) is Q_e(t) posed by M with the
 *      arithmetic of "Match lists": ((M0 x + M1 y) + M2, (M3 x + M4 y) + M5).  With rot NULL P_0(r) = P(r): the lines go through no
 *      identity rotation.  The bin of a line is closestOrientation of the posed, untranslated line of P_e(r), as
 *      fdcm_matches_verify computes it; where fdcm_orientation_bins_mode() is 1 the bins come from the host.
 *      Window: i in -hx .. hx and j in -hy .. hy; the translation is tau = (i sx, j sy); N = (2 hx + 1)(2 hy + 1);
 *      g = (j + hy)(2 hx + 1) + (i + hx).
 *      Score of (r, e, i, j): the score of the lines P_e(r) at translation tau -- the seam's offset T + tau (summed first in
 *      float32, then added to each coordinate), truncation, the set's caps, Eigen's sum() order.  Without caps it is bit for
 *      bit fdcm_featuremap_evaluate(P_e(r), tau).  The pose is admissible by the seam's rule for P_e(r) at tau.  A NaN score has
 *      no key, as in fdcm_search_exhaustive_windows.
 *      Key: (score bits << 32) | low, low = 0 for the centre pose (e, i, j) = (centre, 0, 0) and 1 + e N + g for every other.
 *      centre is the run position of the unrotated delta, or -1 for none (with rot NULL: 0 or -1).  Ties go to the centre first,
 *      then to the lowest e, then to the lowest g: on a plateau of equal scores (saturated caps) a record stays where it was.
 *      Winner of r: the admissible, keyed pose with the smallest key.  None when r is not valid, its template has no lines, no
 *      pose of its window is admissible, or every admissible pose scores NaN.
 *      Output, aligned with the input: with a winner out[j] = {r.tmpl_idx, score, M'} and pose_out[j] = (e, i, j); without
 *      one out[j] = {r.tmpl_idx, NaN, r.transform} and pose_out[j] = (-1, 0, 0).  A NaN score is never a candidate of
 *      fdcm_matches_detect, so the list can go straight on.  out may be the input buffer.
 *      M', float32, unfused, left to right: M0' = (M0 c + M1 s), M1' = (M0 (-s) + M1 c), M3' = (M3 c + M4 s),
 *      M4' = (M3 (-s) + M4 c), M2' = ((M0 m.x + M1 m.y) + M2) + float32(i sx), M5' = ((M3 m.x + M4 m.y) + M5) + float32(j sy).
 *      With rot NULL the four rotation entries are copied, M2' = M2 + float32(i sx) and M5' = M5 + float32(j sy).
 *      out.score is not s(out).  As with the search, the score is that of the posed lines P_e(r) at a translation, and the
 *      stored matrix has rotation and translation folded in; posing the template again with M' rounds differently.  s(out) is
 *      usually close to out.score but is not its bits, and a record on the map's border can come out not admissible.
 *      Identities.  rot NULL and hx = hy = 0: out.score is s(r) of fdcm_matches_verify bit for bit and the transform is
 *      unchanged as floats.  For records {1, 0, 0, 0, 1, 0} on a set none of whose rotated coordinates is a zero, with
 *      centre = -1, scores and poses are the k = 1 records of fdcm_search_exhaustive_windows for the job (t, 0, na, -hx sx,
 *      -hy sy, 2 hx + 1, 2 hy + 1), bit for bit, and the transforms are equal as floats.  A wider window with the same table
 *      never raises a score; with the centre in the table the refined score of an admissible record is at most s(r).
 *      Permuting the list permutes the output.  Results are a function of the inputs alone: the three forms of matches give
 *      the same bytes.
 *      The device.  Everything is made on the device; no per-record table comes from the host (but the bins, where the host's
 *      libm makes them: device records then cost a download).  A pose pass, a wave per (record, e) and a lane per line, writes
 *      the lines and bins of P_e(r) and, from the extremes of the posed coordinates, the admissible box of the window; a scoring
 *      pass over the implicit table of 4 x 16 patches of every window keeps each patch's smallest key; a last pass takes each
 *      record's smallest key and writes out and pose_out.  Device memory stays below 1 GB for any n: the list is worked through
 *      in parts; one record is never cut, and its na x Lmax lines of 32 bytes go up together, as a job of the pose windows.
 *      FDCM_EINVAL, before any GPU work: everything fdcm_matches_verify rejects about handles, n, on_device and matches; what the
 *      rotations calls reject about rot; centre outside -1 .. na - 1; hx or hy outside 0 .. 4096; sx or sy outside 1 .. 4096;
 *      na N > 65536; out NULL with n > 0; out_on_device not 0 or 1.  n = 0, an empty feature map or an empty template set
 *      give FDCM_OK and write nothing.  The call blocks; concurrent callers of one feature map take turns. ---- */
int fdcm_matches_refine(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n,
                        int on_device, int32_t tmpl_index_base, const fdcm_rotations* rot /* delta table, or NULL */,
                        int32_t centre, int32_t hx, int32_t hy, int32_t sx, int32_t sy, fdcm_match* out /* n records */,
                        int out_on_device, int32_t* pose_out /* n x 3 host, or NULL */);

/* ---- Match lists: pose fit.  A rigid least-squares fit of every record to the edge pixels it explains: the continuous last
 *      stage after fdcm_search and fdcm_matches_refine, whose poses sit on the lattice they were searched on (README.md, "Match
 *      lists: pose fit"; the referee is tests/fit_ref.py, plain Python integers and float64 scalars).  It is no descent on the
 *      chamfer score: each step is a closed-form solve with an exact, order-free definition.
 *      Everything not restated is fdcm_matches_coverage's: the frames rule (a map built from an image or from labels, whole
 *      translation (bx, by)), valid record and admissibility, segment A_i B_i of line i (the truncated map pixels moved to the
 *      label frame) and its bin, the window at margin, radius and bin_tolerance, the three input forms of matches and
 *      tmpl_index_base.  A label pixel P stands for the point (P.x, P.y).
 *      Fit pixels of a record at its current transform.  Candidates are the edge pixels P of its window.  With d = B_i - A_i,
 *      w = P - A_i, dot = w.d, len2 = d.d, cross = w.x d.y - w.y d.x, line i qualifies for P when its bin is within
 *      bin_tolerance of P's label, len2 > 0, 0 < dot < len2 (the coverage rule's interior branch; the end caps take no part)
 *      and cross^2 <= radius^2 len2.  P is assigned to the qualifying line with the smallest cross^2 / len2, compared exactly in
 *      int64 (cross_i^2 len2_j < cross_j^2 len2_i; cross^2 <= 2^10 2^25 and len2 <= 2^25, so the products stay below 2^60), ties
 *      to the lowest i.  A pixel without a qualifying line is no fit pixel; the fit pixels are a subset of the pixels
 *      fdcm_matches_coverage counts as explained.
 *      Moments.  Per line, with o = A_i and u = P - o, six exact int64 sums over its pixels: S1, Sx, Sy, Sxx, Sxy, Syy.  Sums of
 *      small integers: any order of accumulation gives the same value.
 *      Normal equations, one sequential pass in line order, every operation an unfused IEEE float64 operation.  pa, pb: the
 *      float32 sums whose truncation gives A_i, B_i, taken before the truncation, converted to float64, minus the integer
 *      border.  t = pb - pa, L = sqrt(t.x t.x + t.y t.y), nu = (t.y / L, -t.x / L); lines with S1 = 0 or L = 0 are skipped.
 *      Pivot c: the integer point ((min + max) >> 1) per axis over all end pixels A_i, B_i of the record.
 *      e0 = nu.x (o.x - pa.x) + nu.y (o.y - pa.y); g0 = nu.y (o.x - c.x) - nu.x (o.y - c.y).  Four affine functions of u with
 *      coefficients (f0, fx, fy): a = (nu.x, 0, 0), b = (nu.y, 0, 0), g = (g0, nu.y, -nu.x), e = (e0, nu.x, nu.y).
 *      S(p, q) = p0 q0 S1 + (p0 qx + px q0) Sx + (p0 qy + py q0) Sy + px qx Sxx + (px qy + py qx) Sxy + py qy Syy, summed
 *      left to right.  N[r][s] += S(f_r, f_s) and v[r] += S(f_r, e) over f = (a, b, g); See += S(e, e); n += S1.  e is the
 *      signed distance of a pixel to the posed float line; the unknown x = (dx, dy, dtheta) minimises the sum of
 *      (e - nu.dt - dtheta g)^2.
 *      Step.  Damping: tr = N00 + N11; N00 += damping tr; N11 += damping tr; N22 += damping N22.  LDL^T without pivoting:
 *      d0 = N00; l10 = N01 / d0; l20 = N02 / d0; d1 = N11 - l10 N01; m21 = N12 - l20 N01; l21 = m21 / d1;
 *      d2 = N22 - l20 N02 - l21 m21; y0 = v0; y1 = v1 - l10 y0; y2 = v2 - l20 y0 - l21 y1; x2 = y2 / d2;
 *      x1 = y1 / d1 - l21 x2; x0 = y0 / d0 - l10 x1 - l20 x2.  Rotation without libm: h = x2 / 2; q = h h;
 *      cc = (1 - q) / (1 + q); ss = (h + h) / (1 + q).  Fold, in float64 from the record's float32 m0 .. m5, each result rounded
 *      to float32: m0' = cc m0 - ss m3; m1' = cc m1 - ss m4; m3' = ss m0 + cc m3; m4' = ss m1 + cc m4;
 *      m2' = ((cc (m2 - c.x) - ss (m5 - c.y)) + c.x) + x0; m5' = ((ss (m2 - c.x) + cc (m5 - c.y)) + c.y) + x1.  If
 *      x0 = x1 = x2 = 0 exactly, the transform is kept byte for byte.
 *      Iterations and status.  iterations is 1 .. 8.  A record stops early, keeping the transform it has, with status 1:
 *      n < min_pixels at this pass; 2: not (d0 > 0, d1 > 0 and d2 > 0), or an x or a folded float32 that is not finite; 3:
 *      |x0| or |x1| > max_shift, or |x2| > max_angle (tested in this order, after 2's pivots and x); 4: the stepped transform is
 *      not admissible (its posed lines leave the map): the step is not taken and does not count.  Status 0: all steps taken.
 *      Status -1: the input record is invalid or not admissible; it is untouched.  After the last step one more pass at the
 *      final transform gives the final pixel count and rms; a record of status 4 keeps the figures of the transform it keeps.
 *      Output.  n records aligned with the input: tmpl_idx and score unchanged, the transform fitted.  info_out, n x 4 int32:
 *      status, steps taken, fit pixels at the first pass, fit pixels at the final pass.  rms_out, n x 2 float32:
 *      float32(sqrt(max(See, 0) / n)) in float64 at the first and the final pass, NaN when that pass has n = 0 or the status
 *      is -1.  out may be host or device memory, and may be the input's buffer.  Permuting the list permutes the rows; the
 *      three forms of matches and host or device labels give the same bytes.
 *      The device.  The records stay on the device.  Per pass: the table of the current transforms and the strip scan of
 *      fdcm_matches_coverage (only the number of strips comes to the host); a moments pass on the coverage grid, a workgroup
 *      per (record, strip), which adds each fit pixel's six integers to its line's int64 accumulators in LDS and flushes them
 *      with 64-bit atomics; a step pass, a thread per record.  The list is walked in parts under the coverage call's 768 MB,
 *      moments included.  Where fdcm_orientation_bins_mode() is 1 every pass downloads the records for the host's bins.
 *      FDCM_EINVAL, before any GPU work: everything fdcm_matches_coverage rejects (its residual aside); fit NULL; iterations
 *      outside 1 .. 8; min_pixels < 3; damping NaN or < 0; max_shift or max_angle NaN or < 0; out NULL with n > 0;
 *      out_on_device not 0 or 1; n > 2^20.  n = 0, an empty feature map or an empty template set give FDCM_OK and write
 *      nothing.  The call blocks; concurrent callers of one feature map take turns. ---- */
typedef struct fdcm_fit_params {
    int32_t iterations;  /* 1 .. 8 steps */
    int32_t min_pixels;  /* >= 3: fewer fit pixels stop a record (status 1) */
    double damping;      /* >= 0: the share of the diagonal added to it */
    double max_shift;    /* >= 0 pixels: a longer step per axis stops a record (status 3) */
    double max_angle;    /* >= 0 radians */
} fdcm_fit_params;       /* 32 bytes */
int fdcm_matches_fit(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int labels_on_device,
                     const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int matches_on_device,
                     int32_t tmpl_index_base, const fdcm_coverage_params* params, const fdcm_fit_params* fit,
                     fdcm_match* out /* n records */, int out_on_device, int32_t* info_out /* n x 4 host, or NULL */,
                     float* rms_out /* n x 2 host, or NULL */);

/* ---- Templates from a mesh: the visible sharp edges and occluding contours of a triangle mesh, per view, as line templates.
 *      This project's own: the reference samples its templates with an OpenGL renderer outside the library (README, "6-DOF
 *      estimation", step 1).  Every float operation below is float32, rounded once and never fused, in the order written;
 *      floor, ceil, sqrt and division are the correctly rounded ones, and no libm function runs on the device.
 *      Mesh.  vertices: V x 3 float32, finite; faces: F x 3 int32 indices into them, 1 <= V, F <= 2^22; winding is free and a
 *      face may be degenerate.  Edges: the undirected vertex pairs {i < j} of all faces (a pair a face names twice counts
 *      once for it; a pair i = j is none), sorted by (i, j): that position is the edge index e.  An edge has one or two
 *      incident faces f0 < f1; three or more are FDCM_EINVAL ("non-manifold edge").  The vertex of a face opposite an edge is
 *      the index at the position of the face that the pair leaves out.  sharp(e) is decided once, on the host, in float64
 *      (products and sums one operation each, a dot product as (a0 b0 + a1 b1) + a2 b2, the cross product's components as
 *      differences of two products): the edge is a boundary edge (one face); or either face normal n = (v1 - v0) x (v2 - v0)
 *      is the zero vector; or |n0 . n1| < (crease_cos * sqrt(n0 . n0)) * sqrt(n1 . n1).  crease_cos is a double in [-1, 1],
 *      the cosine of the crease angle; the absolute value makes the flag independent of winding.
 *      View.  A 3 x 3 float32 matrix R (row-major, finite, not required to be orthonormal) and one scale > 0, finite, in
 *      pixels per mesh unit, for the call.  Vertex v projects to P = ((r00 x + r01 y) + r02 z, .., ..), X = scale * P.x,
 *      Y = scale * P.y, Z = P.z; the viewer is at Z = +infinity.  Orthographic only.
 *      Orientation.  o(A, B, C) = (B.X - A.X) * (C.Y - A.Y) - (B.Y - A.Y) * (C.X - A.X).
 *      Candidate edge of a view.  A sharp edge; or one that is a contour: with c0, c1 the vertices of f0, f1 opposite
 *      e = (A, B), o0 = o(A, B, c0) and o1 = o(A, B, c1), e is a contour unless o0 and o1 are strictly of opposite sign.
 *      Pixel box of a view.  x0, y0, x1, y1: the least and largest floor(X) and floor(Y) over the vertices.  A view with a
 *      vertex whose |X| or |Y| is not below 2^30, or whose box spans more than 4096 pixels on a side, is FDCM_EINVAL with its
 *      index, after the projection pass and before any raster work.
 *      Item buffer D of a view.  On the integer pixels (i, j) with centre c = (i + 0.5, j + 0.5).  Face f = (A, B, C) is tried
 *      at the pixels of its own box (floor of its vertices' least and largest X and Y) and covers c when a = o(A, B, C) != 0
 *      and e0 = o(B, C, c), e1 = o(C, A, c), e2 = o(A, B, c) are all >= 0 (a > 0) or all <= 0 (a < 0): the edges are
 *      inclusive.  Its depth there is z = ((e0 * A.Z + e1 * B.Z) + e2 * C.Z) / a; a NaN z does not cover.  D(i, j) is the
 *      largest key (ord(z) << 32) | f over the covering faces, ord the order-preserving map of float32 bits to uint32
 *      (negative: all bits flipped; else the sign bit set); D = 0 is "empty", and so is every pixel outside the box.
 *      Samples of a candidate edge (A, B).  dx = B.X - A.X, dy and dz likewise; n = max(1, (int)ceil(max(|dx|, |dy|))); for
 *      k = 0 .. n: t = (float)k / (float)n, S_k = (A.X + t * dx, A.Y + t * dy, A.Z + t * dz), its pixel (floor(S.X),
 *      floor(S.Y)).  Sample k is visible when D of its pixel is empty; or the face f in D is f0 or f1; or S.Z + depth_tol >=
 *      zf, zf being face f's depth formula at (S.X, S.Y) in place of the centre: the plane of the occluder at the sample
 *      itself, so that a coplanar sibling triangle never hides an edge, whatever the slope.  depth_tol >= 0, finite, in mesh
 *      units.
 *      Lines of a view.  Per candidate edge in edge order, the maximal runs k0 < k1 of consecutive visible samples; each gives
 *      the line (S_k0.X, S_k0.Y, S_k1.X, S_k1.Y), kept when its length sqrt(ddx * ddx + ddy * ddy) is > 0 and >= min_length
 *      (>= 0, finite).  Output order is (edge, k0).  Template coordinates have the projection of the mesh origin at (0, 0).
 *      Each view is defined on its own: a list of views equals the views one call each.
 *      The device.  A projection pass, a thread per (view, vertex), leaves each view's box (16 n_views bytes come to the
 *      host).  Per part of the views: a raster pass, 16 lanes per (view, face) over 4 x 4 pixel tiles of the face's box with
 *      64-bit atomic maxima, faces of more than 64 tiles through a list into a pass of 16 x 16 tiles; an edge pass, a lane
 *      per (view, edge), that counts the lines, a scan, and the same pass writing them, in runs of views whose lines fit
 *      256 MB.  Only the boxes and the totals come to the host.  Device memory stays below 1 GB however many views there
 *      are -- one view is never cut, so a single view that alone gives more than 2^24 lines takes what its lines take on top
 *      -- and projections are recomputed where they are used, never stored.
 *      FDCM_EINVAL, before any GPU work: NULL pointers; V or F outside 1 .. 2^22; an index outside 0 .. V - 1; a non-finite
 *      vertex or view entry; scale not finite or <= 0; depth_tol or min_length not finite or < 0; crease_cos NaN or outside
 *      [-1, 1]; n_views outside 0 .. 2^16; a total of 2^31 lines or more (after the count).  Zero views give zero lines
 *      (*lines_out NULL) and FDCM_OK.  The calls block and run on the calling thread's device (fdcm_set_device). ---- */
typedef struct fdcm_mesh fdcm_mesh;
/* host only: the edge table and the flags; no device is needed */
int fdcm_mesh_create(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, double crease_cos,
                     fdcm_mesh** out);
int fdcm_mesh_free(fdcm_mesh* mesh);
int fdcm_mesh_info(const fdcm_mesh* mesh, int64_t* n_edges, int64_t* n_sharp, int64_t* n_boundary);  /* each may be NULL */
/* host only: verts 2 per edge, faces 2 per edge (-1: none), sharp 1 per edge; each may be NULL */
int fdcm_mesh_edges(const fdcm_mesh* mesh, int32_t* verts, int32_t* faces, uint8_t* sharp);
/* *lines_out: 4 floats per line, malloc'ed (fdcm_lines_free), NULL when there is none; offsets_out: n_views + 1 -- what
 * fdcm_templates_create takes as its lines and offsets */
int fdcm_mesh_view_lines(const fdcm_mesh* mesh, const float* views /* 9 per view */, int64_t n_views, float scale,
                         float depth_tol, float min_length, float** lines_out, int64_t* offsets_out);
/* test hook, like the _staged builds: one view's pixel box (x0, y0, x1, y1) and its item buffer, keys_out[(j - y0) * (x1 - x0
 * + 1) + (i - x0)]; keys_out NULL: the box alone; else capacity keys must hold the box (FDCM_EINVAL after box_out is written) */
int fdcm_mesh_view_items(const fdcm_mesh* mesh, const float* view /* 9 */, float scale, int32_t* box_out /* 4 */,
                         uint64_t* keys_out, int64_t capacity);

/* ---- Templates from a mesh: exact visibility and joined lines.  Two options of the call above, each off by default:
 *      {depth_tol, min_length, FDCM_MESH_VIS_ITEMS, -1} gives fdcm_mesh_view_lines' bytes.  Everything not restated here is
 *      that block's: projection, o, candidates, samples S_k, runs, float32 unfused in the order written, each view on its own.
 *      A. visibility = FDCM_MESH_VIS_EXACT.  The item buffer judges a sample by the one face that owns its pixel's centre; on
 *      a finely tessellated smooth surface that face's plane, continued to the sample, lies in front of it, and most of the
 *      outline is lost.  This mode tests every face at the sample itself and builds no item buffer.  Face f = (A, B, C) covers
 *      a sample S when a = o(A, B, C) != 0; S.X lies in [min, max] of the three X and S.Y in that of the three Y (so the
 *      face's pixel box holds S's pixel whatever the rounding); and e0 = o(B, C, S), e1 = o(C, A, S), e2 = o(A, B, S) are all
 *      >= 0 or all <= 0.  Its depth there is zf = ((e0 * A.Z + e1 * B.Z) + e2 * C.Z) / a.  Sample k of edge e = (A, B) is
 *      hidden iff some face f that is neither f0 nor f1 of the edge -- and at k = 0 does not name vertex A, at k = n does not
 *      name B: a face through a vertex cannot hide it, and its zf there is ill-conditioned when the face is edge-on -- covers
 *      S_k with zf > S_k.Z + depth_tol (a NaN zf hides nothing).  Otherwise it is visible: an OR over the faces, independent
 *      of their order.  Runs, the length test and the output order are the other block's.
 *      B. join_tolerance = tol >= 0 (negative: off), with either visibility.  The lines before joining are the runs k0 < k1
 *      of length > 0 in (edge, k0) order, indexed i per view; min_length is not applied to them.  Line i has a start end, at
 *      vertex A when k0 = 0, and a finish end, at vertex B when k1 = n.  An end at a vertex has the point (X_v, Y_v) of the
 *      projected vertex (not S_n, which need not equal it bit for bit); any other end has S_k0 or S_k1.  deg(v) is the number
 *      of ends at vertex v in the view; two ends are linked iff they are at the same vertex with deg = 2; every other end is
 *      free.  A chain is a maximal sequence of lines through links.  A path has two free ends and starts at the free end of
 *      the lower-indexed of its two end lines (a path of one line at its own start end); a cycle has none and starts with
 *      its lowest-indexed line, entered at its start end.  The chain's points P_0 .. P_m are the starting point and then the
 *      far point of each line in turn (a cycle: P_m = P_0); chains are ordered by the index of their first line.  Each chain
 *      is simplified greedily, in float32: a = 0; for j = 2 .. m, with d = P_j - P_a and L2 = d.x * d.x + d.y * d.y, the step
 *      is ok iff L2 > 0, j - a <= 256, and every a < i < j has, with w = P_i - P_a, s = d.x * w.x + d.y * w.y and c = d.x *
 *      w.y - d.y * w.x: 0 <= s, s <= L2 and c * c <= (tol * tol) * L2; when it is not, (P_a, P_(j-1)) is emitted and a = j - 1.
 *      At the end (P_a, P_m) is emitted.  Output: chain order, then emission order; a line is kept when its length is > 0
 *      and >= min_length.  Consequences: every chain point a line skips projects inside the line and lies within tol of it,
 *      up to rounding; tol = 0 joins exactly collinear points only; a polyhedron whose corners turn by more than the tolerance
 *      keeps its line count; a cycle may be cut at P_0 even where it is straight there; a joined line replaces at most 256
 *      segments, which bounds one lane's work on a long straight chain.
 *      The device.  A: the faces are binned into 8 x 8 pixel tiles of the view's box -- a count pass per (view, face) over
 *      the tiles of the face's pixel box, a scan, a fill pass with an atomic cursor -- and the edge pass tests a sample
 *      against the faces of its tile; the raster passes are skipped.  The lists count in the part's 512 MB, the parts being cut
 *      from per-view totals computed first; a single view whose lists alone need more than 2^28 entries is FDCM_EINVAL with
 *      its index.  B: the edge pass writes the lines before joining with (edge, end flags); a link pass counts the ends per
 *      (view, vertex) and keeps two; a chain pass, a lane per line, emits where the line starts a chain, as count, scan and
 *      write.  The link tables count in the 512 MB, a line before joining takes 44 bytes of the writing pass's 256 MB.
 *      FDCM_EINVAL, before any GPU work: what fdcm_mesh_view_lines refuses; params NULL; visibility neither value;
 *      join_tolerance NaN or +infinity. ---- */
typedef struct { float depth_tol, min_length; int32_t visibility; float join_tolerance; } fdcm_mesh_line_params;  /* 16 bytes */
enum { FDCM_MESH_VIS_ITEMS = 0, FDCM_MESH_VIS_EXACT = 1 };
int fdcm_mesh_view_lines_ex(const fdcm_mesh* mesh, const float* views /* 9 per view */, int64_t n_views, float scale,
                            const fdcm_mesh_line_params* params, float** lines_out, int64_t* offsets_out);

/* ---- Templates from a mesh: pinhole views.  A camera mode of the calls above, beside the orthographic one, which stays the
 *      default and keeps its bytes.  Everything not restated here is the two blocks' above: orientation o, candidates, pixel
 *      box, item buffer and its keys (ord(Z)), samples S_k, runs, exact visibility, joining, min_length, output order, "each
 *      view on its own", the memory limits, float32 unfused in the order written.
 *      Camera.  fdcm_mesh_camera {focal, near}: focal in pixels, near in mesh units, both finite and > 0, for the call.
 *      View.  R as above, and a position t of 3 floats, finite, with -t.z > 0: where the mesh origin lies in the camera's
 *      frame.  The camera is at the origin and looks down -Z; X and Y are as in the orthographic mode.
 *      Projection of vertex v = (x, y, z).  P.c = ((r_c0 x + r_c1 y) + r_c2 z) + t.c for c = x, y, z; the depth d = -P.z;
 *      Z = 1.0f / d; X = (focal * P.x) * Z - O.x and Y = (focal * P.y) * Z - O.y, with O.x = (focal * t.x) * (1.0f / (-t.z))
 *      and O.y likewise: the projection of the mesh origin is the template's (0, 0), as above, and a larger Z is nearer, as
 *      above.  Z = 1 / depth is linear in X and Y across a plane, so the orientation tests, the barycentric depth of a face
 *      ((e0 * A.Z + e1 * B.Z) + e2 * C.Z) / a and the interpolation A.Z + t * dz of a sample along a projected edge are
 *      perspective-correct as they stand.  With t = (0, 0, -D), focal = scale * D and D -> infinity the view tends to the
 *      orthographic one.
 *      Refused.  A view with a vertex whose d is not >= near (a NaN d too) is FDCM_EINVAL with the view's index, after the
 *      projection pass and before any raster work, like an oversized box.  There is no clipping.
 *      Depth tolerance.  Still in mesh units: in depth it means d_S <= d_f + depth_tol.  On Z, with zf the occluder's depth
 *      formula at the sample: the item buffer's rule calls the sample visible iff (depth_tol * S.Z) * zf >= zf - S.Z (in
 *      place of S.Z + depth_tol >= zf); the exact rule calls it hidden iff zf - S.Z > (depth_tol * S.Z) * zf (in place of
 *      zf > S.Z + depth_tol; a NaN hides nothing).
 *      The device.  The projection is a type parameter of the kernels above, so the orthographic instantiations are the
 *      code they were; the projection pass marks a view with a vertex nearer than `near` the way it marks an oversized
 *      coordinate.  The positions travel with the views (12 n_views bytes more on the device).
 *      FDCM_EINVAL, before any GPU work: what fdcm_mesh_view_lines_ex refuses (focal in place of scale); camera or positions
 *      NULL; focal, near or a position's entry not finite; focal <= 0, near <= 0 or -t.z <= 0 (with the position's index). ---- */
typedef struct { float focal, near; } fdcm_mesh_camera;  /* 8 bytes */
int fdcm_mesh_view_lines_cam(const fdcm_mesh* mesh, const float* views /* 9 per view */, const float* positions /* 3 per view */,
                             int64_t n_views, const fdcm_mesh_camera* camera, const fdcm_mesh_line_params* params,
                             float** lines_out, int64_t* offsets_out);
/* the test hook fdcm_mesh_view_items through the camera */
int fdcm_mesh_view_items_cam(const fdcm_mesh* mesh, const float* view /* 9 */, const float* position /* 3 */,
                             const fdcm_mesh_camera* camera, int32_t* box_out /* 4 */, uint64_t* keys_out, int64_t capacity);

/* ---- host-side self checks (no GPU needed) ---- */
/* Compare the device-portable atanf restatement with this machine's libm atanf over the float
 * bit patterns first, first+stride, ... (count values); returns the number of mismatches. */
int64_t fdcm_selftest_atanf(uint32_t first, uint32_t stride, uint64_t count);
/* Where the searches of this process take the orientation bins of the aligned template lines from (closestOrientation,
 * dt3cpu.h:93-114, on atanf, math.h:295-299): 0 = the device's restatement of atanf (it agrees with this machine's libm
 * on the sample the first search checks), 1 = this machine's libm on host threads (the sample disagreed -- another
 * glibc -- or FDCM_FORCE_HOST_BINS=1; slower: every search recomputes align / transform / atanf of every candidate
 * line on the host, and says so once on stderr).  Decided at the first call of this function or of a search. */
int fdcm_orientation_bins_mode(void);
/* Column ranges the balanced L2 / L2^2 sweep cuts a row of a slice with n seeded columns into (1 .. 8; csrc/fdcm_sweep.h:
 * the kernel calls the same function).  FDCM_SWEEP_MINCOLS=1..64, the tests' switch, lowers the columns a range holds at
 * least from 16, so that small test images exercise all 8 ranges: this call lets a test see that the switch took. */
int fdcm_selftest_sweep_ranges(int n_seeded_columns);
/* Builds of this process whose L2 / L2^2 sweep took its workgroup launch order from the per-chunk times of the handle's
 * previous build (`from_history`) / from the host's proxy, i.e. a handle's first build of a shape (`from_proxy`); builds
 * small enough to be resident at once take no order and count in neither.  Lets a test see that a frame slot whose buffers
 * are reserved before every frame (fdcm_sharded_submit) keeps its history. */
int fdcm_selftest_sweep_order_counts(int64_t* from_history, int64_t* from_proxy);
/* Column ranges that waves of the balanced L2 / L2^2 sweep took over from slower ones, over all builds of this handle's
 * present scratch (dynamic cuts: a wave out of columns begins a new range in the middle of the longest stretch nobody has
 * started; by default only where one blocking build has the GPU to itself, FDCM_SWEEP_STEAL=<blocks> forces a threshold,
 * 0 = never).  Lets a test see that the path it means to exercise ran. */
int fdcm_selftest_sweep_steals(fdcm_featuremap* fm, int64_t* count);
/* The buffers the test switch FDCM_POISON fills (openfdcm_amd/csrc/fdcm_internal.h, "the tests' switches"; DESIGN.md, section
 * 32), by the names of their members: the exhaustive calls' workspace and the volume, the build's scratch, the reference
 * search's workspaces, the device tail's, scene coverage's and the scratch of the calls without a handle. */
enum fdcm_poison_buffer {
    FDCM_FILL_EVAL = 0, FDCM_FILL_EVAL_STAGE, FDCM_FILL_VOL,
    FDCM_FILL_IVOL, FDCM_FILL_BITMAP, FDCM_FILL_COLDESC, FDCM_FILL_COLMASK, FDCM_FILL_LABELS, FDCM_FILL_EDGE_PARENT,
    FDCM_FILL_EDGE_ROOTS, FDCM_FILL_PYR, FDCM_FILL_OFFTAB, FDCM_FILL_STACK, FDCM_FILL_PLAN, FDCM_FILL_BUILD_STAGE,
    FDCM_FILL_SCENE, FDCM_FILL_PAIRS, FDCM_FILL_RECORDS, FDCM_FILL_FLAGS, FDCM_FILL_WORK, FDCM_FILL_COUNTER, FDCM_FILL_BINS,
    FDCM_FILL_OUT, FDCM_FILL_SEARCH_STAGE, FDCM_FILL_BINS_STAGE, FDCM_FILL_CNT,
    FDCM_FILL_TAIL, FDCM_FILL_TAIL_OUT,
    FDCM_FILL_COVERAGE, FDCM_FILL_COVERAGE_STAGE,
    FDCM_FILL_PIXEL_PIXELS, FDCM_FILL_PIXEL_LABELS, FDCM_FILL_PIXEL_KEYS, FDCM_FILL_PIXEL_PARENT, FDCM_FILL_PIXEL_COUNTS,
    FDCM_FILL_PIXEL_COMPS, FDCM_FILL_PIXEL_OUT,
    FDCM_FILL_BUFFERS  /* how many there are */
};
/* counts[i]: how often this process filled buffer ids[i] (an fdcm_poison_buffer) with FDCM_POISON's word; all 0 without the
 * switch.  A fill of a buffer without capacity does not count.  Lets a test see that the word reached the buffers it means to
 * cover. */
int fdcm_selftest_poison_fills(const int32_t* ids, int64_t n, int64_t* counts);

#ifdef __cplusplus
}
#endif
#endif /* FDCM_H */
