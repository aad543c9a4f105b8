// fdcm_capi.cpp -- extern "C" entry points of libfdcm_hip.so (include/fdcm.h).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <numeric>
#include <thread>

#include "fdcm_internal.h"
#include "fdcm_sweep.h"

namespace fdcm {
int device_cus(int device) {
    static std::mutex mu;
    static int cached[64] = {};
    std::lock_guard<std::mutex> lock(mu);
    int& c = cached[device & 63];
    if (c <= 0) FDCM_HIP(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, device));
    return c;
}
const char* last_error_cstr();
static thread_local int g_device = 0;

template <class F>
static int guarded(F&& f) {
    try {
        f();
        return FDCM_OK;
    } catch (const HipError& e) {
        set_error(std::string("HIP error: ") + hipGetErrorString(e.code) + " in " + e.what);
        return FDCM_EHIP;
    } catch (const std::string& s) {
        set_error(s);
        return FDCM_EINVAL;
    } catch (const std::exception& e) {
        set_error(e.what());
        return FDCM_EINTERNAL;
    } catch (...) {
        set_error("unknown error");
        return FDCM_EINTERNAL;
    }
}

static void require(bool ok, const char* msg) {
    if (!ok) throw std::string(msg);
}
static void check_handles(const fdcm_featuremap* fm, const fdcm_templates* t) {  // the two handles of a call, on one device
    require(fm && t, "null featuremap/templates");
    require(fm->device == t->device, "featuremap and templates live on different devices");
}

// A call that returns records in *out (checked non-null): what it had acquired is released when it throws, and a call
// without records leaves an empty (non-null) array.
template <class F>
static void records_call(fdcm_match** out, F&& call) {
    *out = nullptr;
    try {
        call();
    } catch (...) {
        result_release(*out);
        *out = nullptr;
        throw;
    }
    if (!*out) *out = result_acquire(sizeof(fdcm_match));
}

static void upload_keys_only(fdcm_featuremap* fm) {
    // feature maps adopted from caller slices carry no build plan: the keys go where a plan's keys would be (the search reads them there)
    BuildPlan keys_only;
    keys_only.W = fm->W; keys_only.H = fm->H; keys_only.m = fm->m; keys_only.keys = fm->keys;
    const BuildLayout L = build_layout(keys_only, fm->distance, 3);
    fm->off_keys = L.off_keys;
    fm->build.plan.reserve(std::max<size_t>(16, L.plan));
    if (!fm->keys.empty())
        FDCM_HIP(hipMemcpy((char*)fm->build.plan.p + fm->off_keys, fm->keys.data(), fm->keys.size() * sizeof(float), hipMemcpyHostToDevice));
}

static void destroy(fdcm_featuremap* fm) {
    if (!fm) return;
    (void)hipSetDevice(fm->device);
    if (fm->stream) (void)hipStreamSynchronize(fm->stream);
    if (fm->prep_stream) (void)hipStreamSynchronize(fm->prep_stream);
    fm->vol.release(); fm->ivol.release(); fm->build.release(); fm->search.release();
    fm->coverage.release(); fm->coverage_stage.release();
    if (fm->timing.created)
        for (auto& e : fm->timing.ev) (void)hipEventDestroy(e);
    if (fm->stream) (void)hipStreamDestroy(fm->stream);
    if (fm->prep_stream) { (void)hipStreamDestroy(fm->prep_stream); (void)hipEventDestroy(fm->prep_done); }
    delete fm;
}
}  // namespace fdcm

using namespace fdcm;

extern "C" {

const char* fdcm_last_error(void) { return last_error_cstr(); }
const char* fdcm_version(void) { return "openfdcm_amd 0.1.0 (gfx950)"; }

int fdcm_device_count(int* count) {
    return guarded([&] {
        require(count != nullptr, "count is null");
        FDCM_HIP(hipGetDeviceCount(count));
    });
}

int fdcm_set_device(int device) {
    return guarded([&] {
        FDCM_HIP(hipSetDevice(device));
        g_device = device;
    });
}

int fdcm_get_device(int* device) {
    return guarded([&] {
        require(device != nullptr, "device is null");
        *device = g_device;
    });
}

int fdcm_featuremap_build_staged(const float* scene_lines, int64_t n_lines, int64_t depth, float dt3_coeff,
                                 float padding, int distance, int stop_after, fdcm_featuremap** out) {
    fdcm_featuremap* fm = nullptr;
    int rc = guarded([&] {
        require(out != nullptr, "out is null");
        require(n_lines >= 0 && (n_lines == 0 || scene_lines), "bad scene_lines");
        require(depth >= 0, "depth must be >= 0");
        require(distance >= FDCM_L2 && distance <= FDCM_L1, "unknown distance");
        require(stop_after >= 1 && stop_after <= 3, "stop_after must be 1..3");
        fm = new fdcm_featuremap();
        fm->device = g_device;
        fm->depth_param = depth; fm->coeff = dt3_coeff; fm->padding = padding; fm->distance = distance;
        BuildPlan plan;
        make_build_plan(scene_lines, depth > 0 ? n_lines : 0, depth, dt3_coeff, padding, plan);
        run_build(fm, plan, stop_after);
        *out = fm;
    });
    if (rc != FDCM_OK) { destroy(fm); if (out) *out = nullptr; }
    return rc;
}

int fdcm_featuremap_build(const float* scene_lines, int64_t n_lines, int64_t depth, float dt3_coeff, float padding,
                          int distance, fdcm_featuremap** out) {
    return fdcm_featuremap_build_staged(scene_lines, n_lines, depth, dt3_coeff, padding, distance, 3, out);
}

int fdcm_featuremap_rebuild(fdcm_featuremap* fm, const float* scene_lines, int64_t n_lines) {
    return guarded([&] {
        require(fm != nullptr, "featuremap is null");
        require(n_lines >= 0 && (n_lines == 0 || scene_lines), "bad scene_lines");
        BuildPlan plan;
        make_build_plan(scene_lines, fm->depth_param > 0 ? n_lines : 0, fm->depth_param, fm->coeff, fm->padding, plan);
        run_build(fm, plan, 3);
    });
}

// ------------------------------------------------------------------------------------------ feature maps from images
// Everything an image / label build checks before it touches a device; fills the plan of the shape (no scene is made up).
// An image's edge parameters: `threshold` alone (the entry points without _ex), or `ex`, the caller's fdcm_edge_params.
struct EdgeArg {
    int threshold = 0;
    const fdcm_edge_params* ex = nullptr;
    bool is_ex = false;
    static EdgeArg plain(int t) { EdgeArg a; a.threshold = t; return a; }
    static EdgeArg params(const fdcm_edge_params* p) { EdgeArg a; a.ex = p; a.is_ex = true; return a; }
};
// level > 0 (images only): the seeds come from P_level of the image (include/fdcm.h, "image pyramid"), and border and the map's
// size are in its pixels.
static void pixel_plan(const uint8_t* pixels, int64_t width, int64_t height, int64_t row_stride, int on_device, SeedKind kind,
                       const EdgeArg& edge, int64_t border, int64_t depth, float coeff, BuildPlan& plan, int32_t level = 0) {
    require(level >= 0 && level <= 12, "level must be in [0, 12]");
    require(pixels != nullptr, kind == SeedKind::image ? "image is null" : "labels is null");
    require(width >= 1 && height >= 1, "width and height must be at least 1");
    require(border >= 0, "border must be >= 0");
    require(level == 0 || (width <= 4096 && height <= 4096), "width and height must be at most 4096");
    const int64_t width0 = width, height0 = height;
    pyramid_size(width0, height0, level, &width, &height);
    require(width + 2 * border <= 4096 && height + 2 * border <= 4096, "feature maps from images are limited to 4096 x 4096 (border included)");
    require(row_stride >= width0, "row_stride must be >= width");
    require(on_device == 0 || on_device == 1, "on_device must be 0 or 1");
    fdcm_edge_params e = {0, edge.threshold, edge.threshold, 1};
    if (kind == SeedKind::image && !edge.is_ex) require(edge.threshold >= 1 && edge.threshold <= 1442, "threshold must be in [1, 1442]");
    if (kind == SeedKind::image && edge.is_ex) {
        require(edge.ex != nullptr, "params is null");
        e = *edge.ex;
        require(e.smooth >= 0 && e.smooth <= 2, "params: smooth must be 0, 1 or 2");
        require(e.low >= 1 && e.high <= 1442 && e.low <= e.high, "params: low and high must satisfy 1 <= low <= high <= 1442");
        require(e.min_pixels >= 1, "params: min_pixels must be >= 1");
    }
    require(depth >= 0, "depth must be >= 0");
    require(depth <= 255, "depth gives more than 255 orientation keys: a label is one byte");
    plan = BuildPlan{};
    make_shape_plan(depth, coeff, width + 2 * border, height + 2 * border, plan);
    plan.tx = plan.ty = (float)border;
    plan.seeds.kind = kind; plan.seeds.pixels = pixels; plan.seeds.on_device = on_device != 0;
    plan.seeds.width = (int)width; plan.seeds.height = (int)height; plan.seeds.row_stride = (int)row_stride;
    plan.seeds.border = (int)border; plan.seeds.edge = e;
    plan.seeds.level = level; plan.seeds.width0 = (int)width0; plan.seeds.height0 = (int)height0;
}

static int build_from_pixels(const uint8_t* pixels, int64_t width, int64_t height, int64_t row_stride, int on_device, SeedKind kind,
                             const EdgeArg& edge, int64_t border, int64_t depth, float coeff, int distance, int stop_after, fdcm_featuremap** out,
                             int32_t level = 0) {
    fdcm_featuremap* fm = nullptr;
    int rc = guarded([&] {
        require(out != nullptr, "out is null");
        require(distance >= FDCM_L2 && distance <= FDCM_L1, "unknown distance");
        require(stop_after >= 1 && stop_after <= 3, "stop_after must be 1..3");
        BuildPlan plan;
        pixel_plan(pixels, width, height, row_stride, on_device, kind, edge, border, depth, coeff, plan, level);
        fm = new fdcm_featuremap();
        fm->device = g_device;
        fm->depth_param = depth; fm->coeff = coeff; fm->padding = 0.f; fm->distance = distance;
        run_build(fm, plan, stop_after);
        *out = fm;
    });
    if (rc != FDCM_OK) { destroy(fm); if (out) *out = nullptr; }
    return rc;
}

static int rebuild_from_pixels(fdcm_featuremap* fm, const uint8_t* pixels, int64_t width, int64_t height, int64_t row_stride, int on_device,
                               SeedKind kind, const EdgeArg& edge, int64_t border, int32_t level = 0) {
    return guarded([&] {
        require(fm != nullptr, "featuremap is null");
        BuildPlan plan;
        pixel_plan(pixels, width, height, row_stride, on_device, kind, edge, border, fm->depth_param, fm->coeff, plan, level);
        run_build(fm, plan, 3);
    });
}

int fdcm_edge_labels(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int64_t depth, int threshold,
                     uint8_t* labels_out) {
    return guarded([&] {
        require(labels_out != nullptr, "labels_out is null");
        require(depth >= 1, "depth must be >= 1");
        BuildPlan plan;
        pixel_plan(image, width, height, row_stride, 0, SeedKind::image, EdgeArg::plain(threshold), 0, depth, 0.f, plan);
        edge_labels_host(g_device, image, (int)width, (int)height, (int)row_stride, depth, plan.seeds.edge, false, labels_out);
    });
}

int fdcm_edge_labels_ex(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int64_t depth,
                        const fdcm_edge_params* params, uint8_t* labels_out) {
    return guarded([&] {
        require(labels_out != nullptr, "labels_out is null");
        require(depth >= 1, "depth must be >= 1");
        BuildPlan plan;
        pixel_plan(image, width, height, row_stride, 0, SeedKind::image, EdgeArg::params(params), 0, depth, 0.f, plan);
        edge_labels_host(g_device, image, (int)width, (int)height, (int)row_stride, depth, plan.seeds.edge, true, labels_out);
    });
}

// ------------------------------------------------------------------------------------------ line segments from images
static void check_line_params(const fdcm_line_params* lp, int64_t m, float** lines, int64_t* n_lines) {
    require(lp != nullptr, "line params is null");
    require(lines != nullptr, "lines is null");
    require(n_lines != nullptr, "n_lines is null");
    require(lp->bucket >= 1 && lp->bucket <= m, "line params: bucket must be in [1, the number of orientation keys]");
    require(lp->min_pixels >= 2 && lp->min_pixels <= 65535, "line params: min_pixels must be in [2, 65535]");
    require(lp->min_length >= 1 && lp->min_length <= 4096, "line params: min_length must be in [1, 4096]");
}

int fdcm_lines_from_labels(const uint8_t* labels, int64_t width, int64_t height, int on_device, int64_t depth,
                           const fdcm_line_params* params, float** lines, int64_t* n_lines) {
    return guarded([&] {
        require(depth >= 1, "depth must be >= 1");
        BuildPlan plan;
        pixel_plan(labels, width, height, width, on_device, SeedKind::labels, EdgeArg(), 0, depth, 0.f, plan);
        check_line_params(params, plan.m, lines, n_lines);
        lines_from_labels_host(g_device, labels, (int)width, (int)height, on_device != 0, (int)plan.m, *params, lines, n_lines);
    });
}

int fdcm_lines_from_image(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device,
                          int64_t depth, const fdcm_edge_params* edge, const fdcm_line_params* params,
                          float** lines, int64_t* n_lines) {
    return guarded([&] {
        require(depth >= 1, "depth must be >= 1");
        BuildPlan plan;
        pixel_plan(image, width, height, row_stride, on_device, SeedKind::image, EdgeArg::params(edge), 0, depth, 0.f, plan);
        check_line_params(params, plan.m, lines, n_lines);
        lines_from_image_host(g_device, image, (int)width, (int)height, (int)row_stride, on_device != 0, depth, plan.seeds.edge, *params,
                              lines, n_lines);
    });
}

int fdcm_lines_last_timing(fdcm_lines_timing* out) {
    return guarded([&] {
        require(out != nullptr, "out is null");
        lines_last_timing(out);
    });
}

int fdcm_featuremap_build_image_ex(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device,
                                   const fdcm_edge_params* params, int64_t border, int64_t depth, float dt3_coeff, int distance,
                                   fdcm_featuremap** out) {
    return build_from_pixels(image, width, height, row_stride, on_device, SeedKind::image, EdgeArg::params(params), border, depth, dt3_coeff,
                             distance, 3, out);
}

int fdcm_featuremap_rebuild_image_ex(fdcm_featuremap* fm, const uint8_t* image, int64_t width, int64_t height, int64_t row_stride,
                                     int on_device, const fdcm_edge_params* params, int64_t border) {
    return rebuild_from_pixels(fm, image, width, height, row_stride, on_device, SeedKind::image, EdgeArg::params(params), border);
}

// ------------------------------------------------------------------------------------------ image pyramid
static void check_pyramid_args(int64_t width, int64_t height, int32_t level) {
    require(level >= 0 && level <= 12, "level must be in [0, 12]");
    require(width >= 1 && height >= 1 && width <= 4096 && height <= 4096, "width and height must be in [1, 4096]");
}

int fdcm_image_pyramid_size(int64_t width, int64_t height, int32_t level, int64_t* w_out, int64_t* h_out) {
    return guarded([&] {
        require(w_out != nullptr, "w_out is null");
        require(h_out != nullptr, "h_out is null");
        check_pyramid_args(width, height, level);
        pyramid_size(width, height, level, w_out, h_out);
    });
}

int fdcm_image_pyramid_level(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device, int32_t level,
                             uint8_t* out, int out_on_device) {
    return guarded([&] {
        require(image != nullptr, "image is null");
        require(out != nullptr, "out is null");
        check_pyramid_args(width, height, level);
        require(row_stride >= width, "row_stride must be >= width");
        require(on_device == 0 || on_device == 1, "on_device must be 0 or 1");
        require(out_on_device == 0 || out_on_device == 1, "out_on_device must be 0 or 1");
        image_pyramid_host(g_device, image, (int)width, (int)height, (int)row_stride, on_device != 0, level, out, out_on_device != 0);
    });
}

int fdcm_featuremap_build_image_level(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device, int32_t level,
                                      const fdcm_edge_params* params, int64_t border, int64_t depth, float dt3_coeff, int distance,
                                      fdcm_featuremap** out) {
    return build_from_pixels(image, width, height, row_stride, on_device, SeedKind::image, EdgeArg::params(params), border, depth, dt3_coeff,
                             distance, 3, out, level);
}

int fdcm_featuremap_rebuild_image_level(fdcm_featuremap* fm, const uint8_t* image, int64_t width, int64_t height, int64_t row_stride,
                                        int on_device, int32_t level, const fdcm_edge_params* params, int64_t border) {
    return rebuild_from_pixels(fm, image, width, height, row_stride, on_device, SeedKind::image, EdgeArg::params(params), border, level);
}

int fdcm_featuremap_build_image(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device, int threshold,
                                int64_t border, int64_t depth, float dt3_coeff, int distance, fdcm_featuremap** out) {
    return build_from_pixels(image, width, height, row_stride, on_device, SeedKind::image, EdgeArg::plain(threshold), border, depth, dt3_coeff, distance, 3, out);
}

int fdcm_featuremap_build_image_staged(const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device, int threshold,
                                       int64_t border, int64_t depth, float dt3_coeff, int distance, int stop_after, fdcm_featuremap** out) {
    return build_from_pixels(image, width, height, row_stride, on_device, SeedKind::image, EdgeArg::plain(threshold), border, depth, dt3_coeff, distance,
                             stop_after, out);
}

int fdcm_featuremap_rebuild_image(fdcm_featuremap* fm, const uint8_t* image, int64_t width, int64_t height, int64_t row_stride, int on_device,
                                  int threshold, int64_t border) {
    return rebuild_from_pixels(fm, image, width, height, row_stride, on_device, SeedKind::image, EdgeArg::plain(threshold), border);
}

int fdcm_featuremap_build_labels(const uint8_t* labels, int64_t width, int64_t height, int on_device, int64_t border, int64_t depth,
                                 float dt3_coeff, int distance, fdcm_featuremap** out) {
    return build_from_pixels(labels, width, height, width, on_device, SeedKind::labels, EdgeArg(), border, depth, dt3_coeff, distance, 3, out);
}

int fdcm_featuremap_rebuild_labels(fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int on_device, int64_t border) {
    return rebuild_from_pixels(fm, labels, width, height, width, on_device, SeedKind::labels, EdgeArg(), border);
}

int fdcm_featuremap_free(fdcm_featuremap* fm) {
    destroy(fm);
    return FDCM_OK;
}

int fdcm_featuremap_get_info(const fdcm_featuremap* fm, fdcm_featuremap_info* info) {
    return guarded([&] {
        require(fm && info, "null argument");
        info->width = fm->W; info->height = fm->H; info->depth = fm->m;
        info->scene_translation[0] = fm->tx; info->scene_translation[1] = fm->ty;
        info->distance = fm->distance; info->dt3_coeff = fm->coeff; info->padding = fm->pixel_seeded ? 0.f : fm->padding;
    });
}

int fdcm_featuremap_keys(const fdcm_featuremap* fm, float* keys) {
    return guarded([&] {
        require(fm && (keys || fm->keys.empty()), "null argument");
        if (!fm->keys.empty()) std::memcpy(keys, fm->keys.data(), fm->keys.size() * sizeof(float));
    });
}

int fdcm_featuremap_slice(const fdcm_featuremap* fm, int64_t k, float* out_host) {
    return guarded([&] {
        require(fm && out_host, "null argument");
        require(k >= 0 && k < fm->m, "slice index out of range");
        finish_build(const_cast<fdcm_featuremap*>(fm));
        FDCM_HIP(hipSetDevice(fm->device));
        const size_t sl = ivol_slice_floats(fm->W, fm->H);
        std::vector<float> tmp(sl);
        FDCM_HIP(hipMemcpy(tmp.data(), fm->current() + (size_t)k * sl, sl * sizeof(float), hipMemcpyDeviceToHost));
        slice_to_xy(tmp.data(), out_host, fm->W, fm->H);
    });
}

int fdcm_featuremap_device_volume(const fdcm_featuremap* fm, const float** device_ptr) {
    return guarded([&] {
        require(fm && device_ptr, "null argument");
        finish_build(const_cast<fdcm_featuremap*>(fm));  // the caller may read it from any stream
        *device_ptr = fm->current();
    });
}

int fdcm_featuremap_device_volume_stride(const fdcm_featuremap* fm, int64_t* floats_per_slice) {
    return guarded([&] {
        require(fm && floats_per_slice, "null argument");
        *floats_per_slice = fm->holds == VolStage::none ? 0 : (int64_t)ivol_slice_floats(fm->W, fm->H);  // (no pixels: no slices)
    });
}

int fdcm_featuremap_last_timing(const fdcm_featuremap* fm, fdcm_build_timing* t) {
    return guarded([&] {
        require(fm && t, "null argument");
        finish_build(const_cast<fdcm_featuremap*>(fm));
        *t = fm->last_build;
    });
}

int fdcm_featuremap_stage_timing(fdcm_featuremap* fm, int on) {
    return guarded([&] {
        require(fm != nullptr, "featuremap is null");
        require(on >= 0 && on <= 2, "stage timing: 0 (off), 1 (per stage) or 2 (totals only)");
        fm->want_stage_events = on;
    });
}

int fdcm_featuremap_from_slices(const float* keys, int64_t depth, const float* volume_host, int64_t width,
                                int64_t height, const float scene_translation[2], fdcm_featuremap** out) {
    fdcm_featuremap* fm = nullptr;
    int rc = guarded([&] {
        require(out && scene_translation, "null argument");
        require(depth >= 0 && width >= 0 && height >= 0, "negative size");
        require(depth == 0 || (keys && volume_host), "null keys/volume");
        for (int64_t i = 1; i < depth; ++i) require(keys[i - 1] < keys[i], "keys must be strictly ascending (std::map order)");
        fm = new fdcm_featuremap();
        fm->device = g_device;
        FDCM_HIP(hipSetDevice(fm->device));
        fm->depth_param = depth; fm->m = depth; fm->W = width; fm->H = height;
        fm->tx = scene_translation[0]; fm->ty = scene_translation[1];
        fm->keys.assign(keys, keys + depth);
        require(width <= 16384 && height <= 16384, "feature size above 16384 is not supported");
        const size_t sl = ivol_slice_floats(width, height);
        if (depth && sl) {  // into the interleaved layout the search reads, one slice at a time
            fm->vol.reserve((size_t)depth * sl * sizeof(float));
            std::vector<float> tmp(sl, 0.f);
            for (int64_t k = 0; k < depth; ++k) {
                slice_from_xy(volume_host + (size_t)k * width * height, tmp.data(), width, height);
                FDCM_HIP(hipMemcpy(fm->vol.as<float>() + (size_t)k * sl, tmp.data(), sl * sizeof(float), hipMemcpyHostToDevice));
            }
        }
        fm->holds = VolStage::integrated;
        upload_keys_only(fm);
        *out = fm;
    });
    if (rc != FDCM_OK) { destroy(fm); if (out) *out = nullptr; }
    return rc;
}

// ------------------------------------------------------------------------------------------ feature-map seam
static void check_offsets(const int64_t* off, int64_t n, const char* what) {
    require(off != nullptr, what);
    require(off[0] == 0, "offsets[0] must be 0");
    for (int64_t i = 0; i < n; ++i) require(off[i] <= off[i + 1], "offsets must be ascending");
}

int fdcm_featuremap_minmax_translation_batch(const fdcm_featuremap* fm, const float* tmpl_lines, const int64_t* line_offsets,
                                             int64_t n_templates, const float* align_vecs, float* out_minmax) {
    return guarded([&] {
        require(fm != nullptr, "featuremap is null");
        require(n_templates >= 0, "negative template count");
        if (n_templates == 0) return;
        check_offsets(line_offsets, n_templates, "line_offsets is null");
        require(line_offsets[n_templates] == 0 || tmpl_lines, "tmpl_lines is null");
        require(align_vecs && out_minmax, "null align_vecs/out_minmax");
        run_minmax(const_cast<fdcm_featuremap*>(fm), tmpl_lines, line_offsets, n_templates, align_vecs, out_minmax);
    });
}

int fdcm_featuremap_minmax_translation(const fdcm_featuremap* fm, const float* tmpl_lines, int64_t n_lines,
                                       const float align_vec[2], float out_minmax[2]) {
    const int64_t off[2] = {0, n_lines};
    if (n_lines < 0) { set_error("negative line count"); return FDCM_EINVAL; }
    return fdcm_featuremap_minmax_translation_batch(fm, tmpl_lines, off, 1, align_vec, out_minmax);
}

int fdcm_featuremap_evaluate(const fdcm_featuremap* fm, const float* tmpl_lines, const int64_t* line_offsets,
                             int64_t n_templates, const float* translations, const int64_t* translation_offsets,
                             float* scores_out) {
    return guarded([&] {
        require(fm != nullptr, "featuremap is null");
        require(n_templates >= 0, "negative template count");
        if (n_templates == 0) return;
        check_offsets(line_offsets, n_templates, "line_offsets is null");
        check_offsets(translation_offsets, n_templates, "translation_offsets is null");
        require(line_offsets[n_templates] == 0 || tmpl_lines, "tmpl_lines is null");
        require(translation_offsets[n_templates] == 0 || (translations && scores_out), "null translations/scores_out");
        run_evaluate(const_cast<fdcm_featuremap*>(fm), tmpl_lines, line_offsets, n_templates, translations, translation_offsets,
                     scores_out);
    });
}

// ------------------------------------------------------------------------------------------ templates
// caps: one per line or null (all +inf), checked by the caller
static int create_templates(const float* lines, const int64_t* offsets, int64_t n_templates, const float* caps, fdcm_templates** out,
                            int32_t footprint = FDCM_FOOTPRINT_BOX) {
    fdcm_templates* t = nullptr;
    int rc = guarded([&] {
        require(out != nullptr, "out is null");
        require(n_templates >= 0 && (n_templates == 0 || offsets), "bad offsets");
        t = new fdcm_templates();
        t->device = g_device;
        t->footprint = footprint;
        FDCM_HIP(hipSetDevice(t->device));
        t->T = n_templates;
        t->offsets.assign(n_templates + 1, 0);
        for (int64_t i = 0; i <= n_templates && offsets; ++i) t->offsets[i] = offsets[i];
        require(t->offsets[0] == 0, "offsets[0] must be 0");
        for (int64_t i = 0; i < n_templates; ++i) require(t->offsets[i] <= t->offsets[i + 1], "offsets must be ascending");
        t->n_lines = t->offsets[n_templates];
        require(t->n_lines == 0 || lines, "lines is null");
        t->lines.assign(lines, lines + 4 * t->n_lines);
        t->lengths.resize((size_t)t->n_lines);
        t->sorted.resize((size_t)t->n_lines);
        for (int64_t i = 0; i < t->n_lines; ++i) {  // getLength, math.h:306-308
            const float dx = lines[4 * i + 2] - lines[4 * i], dy = lines[4 * i + 3] - lines[4 * i + 1];
            t->lengths[i] = std::sqrt(dx * dx + dy * dy);
        }
        t->caps.assign((size_t)t->n_lines, f_inf());
        for (int64_t i = 0; i < t->n_lines && caps; ++i) {
            t->caps[i] = caps[i] == 0.f ? 0.f : caps[i];  // (-0 as +0)
            t->capped = t->capped || caps[i] < f_inf();
        }
        // argsort(tmpl_lengths, std::greater<>()), defaultsearch.cpp:35 / math.h:106-116: scene independent
        std::vector<long> ind;
        for (int64_t i = 0; i < n_templates; ++i) {
            const int64_t l0 = t->offsets[i], n = t->offsets[i + 1] - l0;
            t->max_lines = std::max(t->max_lines, n);
            ind.resize((size_t)n);
            std::iota(ind.begin(), ind.end(), 0);
            const float* len = t->lengths.data() + l0;
            std::sort(ind.begin(), ind.end(), [len](long const i1, long const i2) { return len[i1] > len[i2]; });
            for (int64_t j = 0; j < n; ++j) t->sorted[l0 + j] = (int32_t)ind[j];
        }
        t->d_lines.reserve(std::max<size_t>(16, t->lines.size() * 4));
        t->d_offsets.reserve((size_t)(n_templates + 1) * 8);
        t->d_lengths.reserve(std::max<size_t>(16, t->lengths.size() * 4));
        t->d_sorted.reserve(std::max<size_t>(16, t->sorted.size() * 4));
        if (t->n_lines) {
            FDCM_HIP(hipMemcpy(t->d_lines.p, t->lines.data(), t->lines.size() * 4, hipMemcpyHostToDevice));
            FDCM_HIP(hipMemcpy(t->d_lengths.p, t->lengths.data(), t->lengths.size() * 4, hipMemcpyHostToDevice));
            FDCM_HIP(hipMemcpy(t->d_sorted.p, t->sorted.data(), t->sorted.size() * 4, hipMemcpyHostToDevice));
        }
        FDCM_HIP(hipMemcpy(t->d_offsets.p, t->offsets.data(), (size_t)(n_templates + 1) * 8, hipMemcpyHostToDevice));
        *out = t;
    });
    if (rc != FDCM_OK) { if (t) fdcm_templates_free(t); if (out) *out = nullptr; }
    return rc;
}

int fdcm_templates_create(const float* lines, const int64_t* offsets, int64_t n_templates, fdcm_templates** out) {
    return create_templates(lines, offsets, n_templates, nullptr, out);
}

// Per-line caps: include/fdcm.h, "Per-line caps and line costs".  The caps are checked before anything touches the device.
int fdcm_templates_create_capped(const float* lines, const int64_t* offsets, int64_t n_templates, const float* caps,
                                 fdcm_templates** out) {
    int rc = guarded([&] {
        require(out != nullptr, "out is null");
        require(n_templates >= 0 && (n_templates == 0 || offsets), "bad offsets");
        if (!caps || n_templates == 0) return;
        require(offsets[0] == 0, "offsets[0] must be 0");
        for (int64_t i = 0; i < n_templates; ++i) require(offsets[i] <= offsets[i + 1], "offsets must be ascending");
        for (int64_t i = 0; i < offsets[n_templates]; ++i) require(caps[i] >= 0.f, "caps must be >= 0 or +inf, never NaN");
    });
    if (rc != FDCM_OK) { if (out) *out = nullptr; return rc; }
    return create_templates(lines, offsets, n_templates, caps, out);
}

// Hull footprints: include/fdcm.h, "Hull footprints".  fdcm_templates_create_capped with the kind of footprint, checked first.
int fdcm_templates_create_shaped(const float* lines, const int64_t* offsets, int64_t n_templates, const float* caps, int32_t footprint,
                                 fdcm_templates** out) {
    int rc = guarded([&] {
        require(footprint == FDCM_FOOTPRINT_BOX || footprint == FDCM_FOOTPRINT_HULL, "footprint must be FDCM_FOOTPRINT_BOX or FDCM_FOOTPRINT_HULL");
        require(out != nullptr, "out is null");
        require(n_templates >= 0 && (n_templates == 0 || offsets), "bad offsets");
        if (!caps || n_templates == 0) return;
        require(offsets[0] == 0, "offsets[0] must be 0");
        for (int64_t i = 0; i < n_templates; ++i) require(offsets[i] <= offsets[i + 1], "offsets must be ascending");
        for (int64_t i = 0; i < offsets[n_templates]; ++i) require(caps[i] >= 0.f, "caps must be >= 0 or +inf, never NaN");
    });
    if (rc != FDCM_OK) { if (out) *out = nullptr; return rc; }
    return create_templates(lines, offsets, n_templates, caps, out, footprint);
}

int fdcm_templates_footprint_kind(const fdcm_templates* t, int32_t* kind) {
    return guarded([&] {
        require(t && kind, "null argument");
        *kind = t->footprint;
    });
}

int fdcm_templates_line_caps(const fdcm_templates* t, float* caps) {
    return guarded([&] {
        require(t && (caps || t->n_lines == 0), "null argument");
        std::copy(t->caps.begin(), t->caps.end(), caps);
    });
}

int fdcm_templates_line_lengths(const fdcm_templates* t, float* lengths) {
    return guarded([&] {
        require(t && (lengths || t->n_lines == 0), "null argument");
        std::copy(t->lengths.begin(), t->lengths.end(), lengths);
    });
}

int fdcm_templates_free(fdcm_templates* t) {
    if (!t) return FDCM_OK;
    (void)hipSetDevice(t->device);
    t->d_lines.release(); t->d_offsets.release(); t->d_lengths.release(); t->d_sorted.release();
    delete t;
    return FDCM_OK;
}

int fdcm_templates_count(const fdcm_templates* t, int64_t* n_templates, int64_t* n_lines) {
    return guarded([&] {
        require(t != nullptr, "templates is null");
        if (n_templates) *n_templates = t->T;
        if (n_lines) *n_lines = t->n_lines;
    });
}

int fdcm_templates_lengths(const fdcm_templates* t, float* lengths) {
    return guarded([&] {
        require(t && (lengths || t->T == 0), "null argument");
        // getTemplateLengths, math.h:319-324: getLength(tmpl).sum() (Eigen redux order)
        for (int64_t i = 0; i < t->T; ++i) {
            const float* v = t->lengths.data() + t->offsets[i];
            const int64_t n = t->offsets[i + 1] - t->offsets[i];
            float res = 0.f;
            if (n > 0) {
                const int64_t a2 = (n / 8) * 8, a1 = (n / 4) * 4;
                if (a1) {
                    float p0[4] = {v[0], v[1], v[2], v[3]};
                    if (a1 > 4) {
                        float p1[4] = {v[4], v[5], v[6], v[7]};
                        for (int64_t idx = 8; idx < a2; idx += 8)
                            for (int l = 0; l < 4; ++l) { p0[l] = p0[l] + v[idx + l]; p1[l] = p1[l] + v[idx + 4 + l]; }
                        for (int l = 0; l < 4; ++l) p0[l] = p0[l] + p1[l];
                        if (a1 > a2) for (int l = 0; l < 4; ++l) p0[l] = p0[l] + v[a2 + l];
                    }
                    res = (p0[0] + p0[2]) + (p0[1] + p0[3]);
                    for (int64_t idx = a1; idx < n; ++idx) res = res + v[idx];
                } else {
                    res = v[0];
                    for (int64_t idx = 1; idx < n; ++idx) res = res + v[idx];
                }
            }
            lengths[i] = res;
        }
    });
}

// ------------------------------------------------------------------------------------------ search
int fdcm_search_capacity(const fdcm_templates* templates, int64_t n_scene_lines, int64_t max_tmpl_lines,
                         int64_t max_scene_lines, int64_t* capacity) {
    return guarded([&] {
        require(templates && capacity, "null argument");
        *capacity = search_capacity(templates, n_scene_lines, max_tmpl_lines, max_scene_lines);
    });
}

static void check_search_args(const fdcm_featuremap* fm, const fdcm_templates* t, const float* scene, int64_t n_scene,
                              int64_t maxT, int64_t maxS, int optimizer, int64_t batch) {
    require(fm && t, "null featuremap/templates");
    require(n_scene >= 0 && (n_scene == 0 || scene), "bad scene_lines");
    require(maxT >= 0 && maxS >= 0, "negative search window");
    require(optimizer >= FDCM_DEFAULT_OPTIMIZE && optimizer <= FDCM_INDULGENT_OPTIMIZE, "unknown optimizer");
    require(optimizer != FDCM_BATCH_OPTIMIZE || batch >= 1, "batch_size must be >= 1");
    require(fm->device == t->device, "featuremap and templates live on different devices");
}

int fdcm_search_device(const fdcm_featuremap* fm, const fdcm_templates* templates, const float* scene_lines,
                       int64_t n_scene_lines, int64_t max_tmpl_lines, int64_t max_scene_lines, int optimizer,
                       int64_t batch_size, int32_t tmpl_index_base, fdcm_match* out_device, int64_t* n_out) {
    return guarded([&] {
        check_search_args(fm, templates, scene_lines, n_scene_lines, max_tmpl_lines, max_scene_lines, optimizer, batch_size);
        require(out_device && n_out, "null output");
        run_search(const_cast<fdcm_featuremap*>(fm), templates, scene_lines, n_scene_lines, max_tmpl_lines,
                   max_scene_lines, optimizer, batch_size, tmpl_index_base, out_device, nullptr, n_out);
    });
}

int fdcm_search(const fdcm_featuremap* fm, const fdcm_templates* templates, const float* scene_lines,
                int64_t n_scene_lines, int64_t max_tmpl_lines, int64_t max_scene_lines, int optimizer,
                int64_t batch_size, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out) {
    return guarded([&] {
        check_search_args(fm, templates, scene_lines, n_scene_lines, max_tmpl_lines, max_scene_lines, optimizer, batch_size);
        require(out && n_out, "null output");
        fdcm_featuremap* f = const_cast<fdcm_featuremap*>(fm);
        *out = nullptr;
        try {
            run_search(f, templates, scene_lines, n_scene_lines, max_tmpl_lines, max_scene_lines, optimizer, batch_size,
                       tmpl_index_base, nullptr, out, n_out);
        } catch (...) {
            result_release(*out);
            *out = nullptr;
            throw;
        }
        if (!*out) *out = result_acquire(sizeof(fdcm_match));  // no candidates: an empty (non-null) array
        f->last_n_out = *n_out;
    });
}

int fdcm_topk(fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches_device, int64_t n,
              int32_t tmpl_index_base, int penalty, float tau, int64_t k, fdcm_match** out, int64_t* n_out) {
    return guarded([&] {
        require(fm && templates && out && n_out, "null argument");
        require(penalty >= -1 && penalty <= FDCM_EXPONENTIAL_PENALTY, "unknown penalty");
        require(fm->device == templates->device, "featuremap and templates live on different devices");
        require(k >= 0, "k must be >= 0");
        if (!matches_device) {  // the matches of the last fdcm_search on this handle
            matches_device = fm->search.out.as<fdcm_match>();
            n = fm->last_n_out;
        }
        require(n >= 0 && (n == 0 || matches_device), "bad matches");
        try {
            run_topk(fm, templates, matches_device, n, tmpl_index_base, penalty, tau, k, out, n_out);
        } catch (...) {
            result_release(*out);
            *out = nullptr;
            throw;
        }
    });
}

// ------------------------------------------------------------------------------------------ exhaustive search
// Definitions: include/fdcm.h, "exhaustive translation search" (the grid, score, admissible set, window and top-k order).
static void check_exhaustive_args(const fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_grid* grid) {
    require(grid != nullptr, "grid is null");
    require(grid->nx >= 1 && grid->ny >= 1, "grid: nx and ny must be >= 1");
    require(grid->sx >= 1 && grid->sy >= 1, "grid: strides sx and sy must be >= 1");
    require((int64_t)grid->nx * grid->ny < ((int64_t)1 << 31), "grid: nx * ny must be below 2^31");
    check_handles(fm, t);
}

int fdcm_exhaustive_window(const fdcm_featuremap* fm, const fdcm_templates* templates, int32_t sx, int32_t sy, fdcm_grid* grid) {
    return guarded([&] {
        require(sx >= 1 && sy >= 1, "strides sx and sy must be >= 1");
        require(fm && templates && grid, "null featuremap/templates/grid");
        exhaustive_window(const_cast<fdcm_featuremap*>(fm), templates, sx, sy, grid);
    });
}

int fdcm_search_exhaustive(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_grid* grid, int32_t k,
                           int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out) {
    return guarded([&] {
        require(k >= 1 && k <= 64, "k must be in [1, 64]");
        check_exhaustive_args(fm, templates, grid);
        require(out && n_out, "null output");
        records_call(out, [&] {
            run_search_exhaustive(const_cast<fdcm_featuremap*>(fm), templates, *grid, k, tmpl_index_base, out, n_out);
        });
    });
}

int fdcm_search_exhaustive_peaks(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_grid* grid, int32_t k,
                                 int32_t rx, int32_t ry, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out) {
    return guarded([&] {
        require(k >= 1 && k <= 64, "k must be in [1, 64]");
        require(rx >= 0 && rx <= 32 && ry >= 0 && ry <= 32, "radii rx and ry must be in [0, 32]");
        check_exhaustive_args(fm, templates, grid);
        require(out && n_out, "null output");
        records_call(out, [&] {
            run_search_exhaustive_peaks(const_cast<fdcm_featuremap*>(fm), templates, *grid, k, rx, ry, tmpl_index_base, out, n_out);
        });
    });
}

// Rotations: include/fdcm.h, "Rotations".  The rotations are checked before the handles; the pivots, whose count is the
// templates', after the null checks (they read no device state).
static void check_rotations(const fdcm_rotations* rot) {
    require(rot != nullptr, "rotations is null");
    require(rot->n >= 1, "rotations: n must be >= 1");
    require(rot->cs != nullptr, "rotations: cs is null");
    for (int32_t a = 0; a < rot->n; ++a)
        require(std::isfinite(rot->cs[2 * a]) && std::isfinite(rot->cs[2 * a + 1]), "rotations: c and s must be finite");
}
static void check_pivots(const fdcm_templates* t, const fdcm_rotations* rot) {
    if (rot->pivots)
        for (int64_t i = 0; i < 2 * t->T; ++i) require(std::isfinite(rot->pivots[i]), "rotations: pivots must be finite");
}

int fdcm_exhaustive_rotations_window(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                     int32_t sx, int32_t sy, fdcm_grid* grid) {
    return guarded([&] {
        require(sx >= 1 && sy >= 1, "strides sx and sy must be >= 1");
        check_rotations(rot);
        require(fm && templates && grid, "null featuremap/templates/grid");
        require(fm->device == templates->device, "featuremap and templates live on different devices");
        check_pivots(templates, rot);
        exhaustive_rotations_window(const_cast<fdcm_featuremap*>(fm), templates, *rot, sx, sy, grid);
    });
}

int fdcm_search_exhaustive_rotations(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                     const fdcm_grid* grid, int32_t k, int32_t rx, int32_t ry, int32_t ra, int32_t wrap,
                                     int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out) {
    return guarded([&] {
        require(k >= 1 && k <= 64, "k must be in [1, 64]");
        require(rx >= 0 && rx <= 32 && ry >= 0 && ry <= 32 && ra >= 0 && ra <= 32, "radii rx, ry and ra must be in [0, 32]");
        require(wrap == 0 || wrap == 1, "wrap must be 0 or 1");
        require(grid != nullptr, "grid is null");
        check_rotations(rot);
        require((uint64_t)rot->n * (uint64_t)std::max(0, grid->nx) * (uint64_t)std::max(0, grid->ny) <= ((uint64_t)1 << 32),
                "n_rot * nx * ny must be at most 2^32");
        check_exhaustive_args(fm, templates, grid);
        require(out && n_out, "null output");
        check_pivots(templates, rot);
        records_call(out, [&] {
            run_search_exhaustive_rotations(const_cast<fdcm_featuremap*>(fm), templates, *rot, *grid, k, rx, ry, ra, wrap,
                                            tmpl_index_base, out, n_out);
        });
    });
}

// Pose windows: include/fdcm.h, "Pose windows".  Everything that needs no handle is checked first, the jobs' templates
// against the set last: nothing here touches the device.
static void check_pose_windows(const fdcm_pose_window* jobs, int64_t n_jobs, int32_t n, int32_t sx, int32_t sy, int32_t wrap) {
    const int64_t lim = (int64_t)1 << 24;
    for (int64_t j = 0; j < n_jobs; ++j) {
        const fdcm_pose_window& J = jobs[j];
        require(J.tmpl >= 0, "jobs: tmpl is outside the template set");
        require(J.na >= 1 && J.na <= n, "jobs: na must be in [1, n]");
        require(J.a0 >= 0 && J.a0 < n, "jobs: a0 must be in [0, n - 1]");
        require(wrap == 1 || (int64_t)J.a0 + J.na <= n, "jobs: a0 + na must be at most n without wrap");
        require(J.nx >= 1 && J.ny >= 1, "jobs: nx and ny must be >= 1");
        require(J.nx <= 65536 && J.ny <= 65536 && (int64_t)J.na * J.nx * J.ny <= 65536, "jobs: na * nx * ny must be at most 65536");
        const int64_t xe = (int64_t)J.x0 + (int64_t)(J.nx - 1) * sx, ye = (int64_t)J.y0 + (int64_t)(J.ny - 1) * sy;
        require(J.x0 > -lim && xe < lim && J.y0 > -lim && ye < lim, "jobs: every translation must satisfy |t| < 2^24");
    }
}

int fdcm_search_exhaustive_windows(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                   const fdcm_pose_window* jobs, int64_t n_jobs, int32_t sx, int32_t sy, int32_t wrap, int32_t k,
                                   int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out, int64_t* job_offsets) {
    return guarded([&] {
        require(k >= 1 && k <= 64, "k must be in [1, 64]");
        require(sx >= 1 && sy >= 1, "strides sx and sy must be >= 1");
        require(wrap == 0 || wrap == 1, "wrap must be 0 or 1");
        require(n_jobs >= 0 && (n_jobs == 0 || jobs), "jobs is null or n_jobs is negative");
        if (rot) check_rotations(rot);  // null: the translations, a table of one rotation
        check_pose_windows(jobs, n_jobs, rot ? rot->n : 1, sx, sy, wrap);
        check_handles(fm, templates);
        require(out && n_out, "null output");
        if (rot) check_pivots(templates, rot);
        for (int64_t j = 0; j < n_jobs && templates->T > 0; ++j)
            require(jobs[j].tmpl < templates->T, "jobs: tmpl is outside the template set");
        records_call(out, [&] {
            run_search_exhaustive_windows(const_cast<fdcm_featuremap*>(fm), templates, rot, jobs, n_jobs, sx, sy, k, tmpl_index_base, out,
                                          n_out, job_offsets);
        });
    });
}

// The detector's limits, in the order every detection call checks them.  cross_permille: null for a call without objects.
static void check_detect_limits(int32_t max_detections, int32_t overlap_permille, const int32_t* cross_permille, int32_t margin) {
    require(max_detections >= 1 && max_detections <= 4096, "max_detections must be in [1, 4096]");
    require(overlap_permille >= 0 && overlap_permille <= 1000, "overlap_permille must be in [0, 1000]");
    if (cross_permille) require(*cross_permille >= 0 && *cross_permille <= 1000, "cross_permille must be in [0, 1000]");
    require(margin >= 0 && margin <= 4096, "margin must be in [0, 4096]");
}

// What both detection calls over pose windows check behind their limits: the penalty, then the pose windows' checks in
// their order.
static void check_detect_windows_args(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                      const fdcm_pose_window* jobs, int64_t n_jobs, int32_t sx, int32_t sy, int32_t wrap, int penalty,
                                      float tau, fdcm_match** out, int64_t* n_out) {
    require(penalty == -1 || penalty == FDCM_DEFAULT_PENALTY || penalty == FDCM_EXPONENTIAL_PENALTY, "unknown penalty");
    require(std::isfinite(tau), "tau must be finite");
    require(out && n_out, "null output");
    require(sx >= 1 && sy >= 1, "strides sx and sy must be >= 1");
    require(wrap == 0 || wrap == 1, "wrap must be 0 or 1");
    require(n_jobs >= 0 && (n_jobs == 0 || jobs), "jobs is null or n_jobs is negative");
    require(n_jobs <= ((int64_t)1 << 22), "n_jobs must be at most 2^22");
    if (rot) check_rotations(rot);  // null: the translations, a table of one rotation
    check_pose_windows(jobs, n_jobs, rot ? rot->n : 1, sx, sy, wrap);
    check_handles(fm, templates);
    if (rot) check_pivots(templates, rot);
    for (int64_t j = 0; j < n_jobs && templates->T > 0; ++j)
        require(jobs[j].tmpl < templates->T, "jobs: tmpl is outside the template set");
}

// Detections over pose windows: include/fdcm.h, "Detections over pose windows".  The detector's limits, then the pose
// windows' checks in their order: nothing here touches the device.
int fdcm_search_exhaustive_detect_windows(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                          const fdcm_pose_window* jobs, int64_t n_jobs, int32_t sx, int32_t sy, int32_t wrap,
                                          float max_score, int32_t max_detections, int32_t overlap_permille, int32_t margin, int penalty,
                                          float tau, float min_matched, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                          int32_t* boxes_out, float* matched_out, int32_t* jobs_out) {
    return fdcm_search_exhaustive_detect_windows_gated(fm, templates, rot, jobs, n_jobs, sx, sy, wrap, max_score, max_detections,
                                                       overlap_permille, margin, penalty, tau, min_matched, FDCM_GATE_WINNER,
                                                       tmpl_index_base, out, n_out, boxes_out, matched_out, jobs_out);
}

// Gate inside the minimum: include/fdcm.h, "Gate inside the minimum".  The call above with the kind of gate, checked with the
// other limits; FDCM_GATE_WINNER is the call above, the same driver with the same arguments.
int fdcm_search_exhaustive_detect_windows_gated(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                                const fdcm_pose_window* jobs, int64_t n_jobs, int32_t sx, int32_t sy, int32_t wrap,
                                                float max_score, int32_t max_detections, int32_t overlap_permille, int32_t margin,
                                                int penalty, float tau, float min_matched, int gate, int32_t tmpl_index_base,
                                                fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out,
                                                int32_t* jobs_out) {
    return guarded([&] {
        require(gate == FDCM_GATE_WINNER || gate == FDCM_GATE_ALL, "gate must be FDCM_GATE_WINNER or FDCM_GATE_ALL");
        require(max_score >= 0.f, "max_score must be >= 0 or +inf, never NaN");
        check_detect_limits(max_detections, overlap_permille, nullptr, margin);
        require(min_matched >= 0.f && min_matched <= 1.f, "min_matched must be in [0, 1], never NaN");
        check_detect_windows_args(fm, templates, rot, jobs, n_jobs, sx, sy, wrap, penalty, tau, out, n_out);
        records_call(out, [&] {
            run_search_exhaustive_detect_windows(const_cast<fdcm_featuremap*>(fm), templates, rot, jobs, n_jobs, sx, sy,
                                                 max_score == 0.f ? 0.f : max_score, max_detections, overlap_permille, margin, penalty, tau,
                                                 min_matched == 0.f ? 0.f : min_matched, gate, tmpl_index_base, out, n_out, boxes_out,
                                                 matched_out, jobs_out);
        });
    });
}

// Best map and detections: include/fdcm.h, "Best map and detections".  What the rotation call rejects, then the limits of
// these two: nothing here touches the device.
static void check_best_args(const fdcm_featuremap* fm, const fdcm_templates* t, const fdcm_rotations* rot, const fdcm_grid* grid,
                            int penalty, float tau) {
    require(penalty == -1 || penalty == FDCM_DEFAULT_PENALTY || penalty == FDCM_EXPONENTIAL_PENALTY, "unknown penalty");
    require(std::isfinite(tau), "tau must be finite");
    require(grid != nullptr, "grid is null");
    if (rot) check_rotations(rot);  // null: the translations, a table of one rotation
    require((int64_t)std::max(0, grid->nx) * (int64_t)std::max(0, grid->ny) <= ((int64_t)1 << 26), "grid: nx * ny must be at most 2^26");
    check_exhaustive_args(fm, t, grid);
    require(t->T * (int64_t)(rot ? rot->n : 1) <= 0x7fffffffll, "T * n_rot must be at most 2^31 - 1");
    if (rot) check_pivots(t, rot);
}

int fdcm_best_map(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot, const fdcm_grid* grid,
                  int penalty, float tau, float* score_out_host, int32_t* pair_out_host) {
    return guarded([&] {
        require(score_out_host || pair_out_host, "score_out_host and pair_out_host are both null");
        check_best_args(fm, templates, rot, grid, penalty, tau);
        run_best_map(const_cast<fdcm_featuremap*>(fm), templates, rot, *grid, penalty, tau, score_out_host, pair_out_host);
    });
}

int fdcm_search_exhaustive_detect(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                  const fdcm_grid* grid, int32_t k, int32_t rx, int32_t ry, int penalty, float tau,
                                  int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out) {
    return guarded([&] {
        require(k >= 1 && k <= 64, "k must be in [1, 64]");
        require(rx >= 0 && rx <= 32 && ry >= 0 && ry <= 32, "radii rx and ry must be in [0, 32]");
        require(out && n_out, "null output");
        check_best_args(fm, templates, rot, grid, penalty, tau);
        records_call(out, [&] {
            run_search_exhaustive_detect(const_cast<fdcm_featuremap*>(fm), templates, rot, *grid, k, rx, ry, penalty, tau,
                                         tmpl_index_base, out, n_out);
        });
    });
}

// Detections by footprint overlap: include/fdcm.h, "Detections suppressed by footprint overlap".  The detect call's checks
// with the overlap threshold and the margin in place of the radii: nothing here touches the device.
int fdcm_search_exhaustive_detect_nms(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                      const fdcm_grid* grid, int32_t k, int32_t overlap_permille, int32_t margin, int penalty, float tau,
                                      int32_t tmpl_index_base, fdcm_match** out, int32_t* boxes_out, int64_t* n_out) {
    return guarded([&] {
        require(k >= 1 && k <= 64, "k must be in [1, 64]");
        require(overlap_permille >= 0 && overlap_permille <= 1000, "overlap_permille must be in [0, 1000]");
        require(margin >= 0 && margin <= 4096, "margin must be in [0, 4096]");
        require(out && n_out, "null output");
        check_best_args(fm, templates, rot, grid, penalty, tau);
        check_hull_rows(templates, rot, margin);
        records_call(out, [&] {
            run_search_exhaustive_detect_nms(const_cast<fdcm_featuremap*>(fm), templates, rot, *grid, k, overlap_permille, margin, penalty,
                                             tau, tmpl_index_base, out, boxes_out, n_out);
        });
    });
}

// All detections below a score: include/fdcm.h, "All detections below a score".  The overlap call's checks with the threshold
// and the bound on the list in place of k: nothing here touches the device.
int fdcm_search_exhaustive_detect_all(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                      const fdcm_grid* grid, float max_score, int32_t max_detections, int32_t overlap_permille,
                                      int32_t margin, int penalty, float tau, int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out,
                                      int32_t* boxes_out) {
    return guarded([&] {
        require(max_score >= 0.f, "max_score must be >= 0 or +inf, never NaN");
        check_detect_limits(max_detections, overlap_permille, nullptr, margin);
        require(out && n_out, "null output");
        check_best_args(fm, templates, rot, grid, penalty, tau);
        check_hull_rows(templates, rot, margin);
        records_call(out, [&] {
            run_search_exhaustive_detect_all(const_cast<fdcm_featuremap*>(fm), templates, rot, *grid, max_score == 0.f ? 0.f : max_score,
                                             max_detections, overlap_permille, margin, penalty, tau, tmpl_index_base, out, n_out,
                                             boxes_out);
        });
    });
}

// Detections by matched fraction: include/fdcm.h, "Detections by matched fraction".  The threshold call's checks and the
// gate's: nothing here touches the device.
int fdcm_search_exhaustive_detect_all_matched(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                              const fdcm_grid* grid, float max_score, int32_t max_detections, int32_t overlap_permille,
                                              int32_t margin, int penalty, float tau, float min_matched, int32_t tmpl_index_base,
                                              fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out) {
    return fdcm_search_exhaustive_detect_all_gated(fm, templates, rot, grid, max_score, max_detections, overlap_permille, margin, penalty,
                                                   tau, min_matched, FDCM_GATE_WINNER, tmpl_index_base, out, n_out, boxes_out, matched_out);
}

// Gate inside the minimum: include/fdcm.h, "Gate inside the minimum".  The call above with the kind of gate, checked with the
// other limits; FDCM_GATE_WINNER is the call above, the same driver with the same arguments.
int fdcm_search_exhaustive_detect_all_gated(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                            const fdcm_grid* grid, float max_score, int32_t max_detections, int32_t overlap_permille,
                                            int32_t margin, int penalty, float tau, float min_matched, int gate, int32_t tmpl_index_base,
                                            fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out) {
    return guarded([&] {
        require(gate == FDCM_GATE_WINNER || gate == FDCM_GATE_ALL, "gate must be FDCM_GATE_WINNER or FDCM_GATE_ALL");
        require(max_score >= 0.f, "max_score must be >= 0 or +inf, never NaN");
        check_detect_limits(max_detections, overlap_permille, nullptr, margin);
        require(min_matched >= 0.f && min_matched <= 1.f, "min_matched must be in [0, 1], never NaN");
        require(out && n_out, "null output");
        check_best_args(fm, templates, rot, grid, penalty, tau);
        check_hull_rows(templates, rot, margin);
        records_call(out, [&] {
            run_search_exhaustive_detect_all_matched(const_cast<fdcm_featuremap*>(fm), templates, rot, *grid,
                                                     max_score == 0.f ? 0.f : max_score, max_detections, overlap_permille, margin, penalty,
                                                     tau, min_matched == 0.f ? 0.f : min_matched, gate, tmpl_index_base, out, n_out,
                                                     boxes_out, matched_out);
        });
    });
}

int fdcm_best_map_gated(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot, const fdcm_grid* grid,
                        int penalty, float tau, float min_matched, float* score_out_host, int32_t* pair_out_host,
                        float* matched_out_host) {
    return guarded([&] {
        require(score_out_host || pair_out_host || matched_out_host, "score_out_host, pair_out_host and matched_out_host are all null");
        require(min_matched >= 0.f && min_matched <= 1.f, "min_matched must be in [0, 1], never NaN");
        check_best_args(fm, templates, rot, grid, penalty, tau);
        run_best_map_gated(const_cast<fdcm_featuremap*>(fm), templates, rot, *grid, penalty, tau, min_matched == 0.f ? 0.f : min_matched,
                           score_out_host, pair_out_host, matched_out_host);
    });
}

// Objects: include/fdcm.h, "Objects".  The per-object arrays are checked with the other limits, before any handle; the labels,
// whose count is the templates', after the null checks (they read no device state).  The thresholds are copied with -0 as +0,
// as the siblings pass theirs.
static void check_object_limits(int32_t n_objects, const float* max_score, bool with_max_score, const float* min_matched,
                                std::vector<float>& ms, std::vector<float>& mm) {
    require(n_objects >= 1 && n_objects <= 256, "n_objects must be in [1, 256]");
    if (with_max_score) {
        require(max_score != nullptr, "max_score is null");
        ms.assign(max_score, max_score + n_objects);
        for (float& v : ms) {
            require(v >= 0.f, "max_score must be >= 0 or +inf, never NaN");
            if (v == 0.f) v = 0.f;
        }
    }
    if (min_matched) {
        mm.assign(min_matched, min_matched + n_objects);
        for (float& v : mm) {
            require(v >= 0.f && v <= 1.f, "min_matched must be in [0, 1], never NaN");
            if (v == 0.f) v = 0.f;
        }
    }
}
static void check_object_labels(const fdcm_templates* t, const int32_t* objects, int32_t n_objects) {
    require(t->T == 0 || objects != nullptr, "objects is null");
    for (int64_t i = 0; i < t->T; ++i) require(objects[i] >= 0 && objects[i] < n_objects, "objects: an entry is outside [0, n_objects)");
}
static void check_object_planes(const fdcm_grid* grid, int32_t n_objects) {
    require(grid != nullptr, "grid is null");
    require((int64_t)n_objects * (int64_t)std::max(0, grid->nx) * (int64_t)std::max(0, grid->ny) <= ((int64_t)1 << 26),
            "n_objects * nx * ny must be at most 2^26");
}

int fdcm_best_map_objects(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot, const fdcm_grid* grid,
                          int penalty, float tau, const int32_t* objects, int32_t n_objects, const float* min_matched,
                          float* score_out_host, int32_t* pair_out_host, float* matched_out_host) {
    return guarded([&] {
        require(score_out_host || pair_out_host || matched_out_host, "score_out_host, pair_out_host and matched_out_host are all null");
        std::vector<float> ms, mm;
        check_object_limits(n_objects, nullptr, false, min_matched, ms, mm);
        check_object_planes(grid, n_objects);
        check_best_args(fm, templates, rot, grid, penalty, tau);
        check_object_labels(templates, objects, n_objects);
        run_best_map_objects(const_cast<fdcm_featuremap*>(fm), templates, rot, *grid, penalty, tau, objects, n_objects,
                             min_matched ? mm.data() : nullptr, score_out_host, pair_out_host, matched_out_host);
    });
}

int fdcm_search_exhaustive_detect_objects(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                          const fdcm_grid* grid, const int32_t* objects, int32_t n_objects, const float* max_score,
                                          const float* min_matched, int32_t max_detections, int32_t overlap_permille,
                                          int32_t cross_permille, int32_t margin, int penalty, float tau, int gate, int32_t tmpl_index_base,
                                          fdcm_match** out, int64_t* n_out, int32_t* boxes_out, float* matched_out) {
    return guarded([&] {
        require(gate == FDCM_GATE_WINNER || gate == FDCM_GATE_ALL, "gate must be FDCM_GATE_WINNER or FDCM_GATE_ALL");
        std::vector<float> ms, mm;
        check_object_limits(n_objects, max_score, true, min_matched, ms, mm);
        check_detect_limits(max_detections, overlap_permille, &cross_permille, margin);
        require(out && n_out, "null output");
        check_object_planes(grid, n_objects);
        check_best_args(fm, templates, rot, grid, penalty, tau);
        check_object_labels(templates, objects, n_objects);
        check_hull_rows(templates, rot, margin);
        records_call(out, [&] {
            run_search_exhaustive_detect_objects(const_cast<fdcm_featuremap*>(fm), templates, rot, *grid, objects, n_objects, ms.data(),
                                                 min_matched ? mm.data() : nullptr, max_detections, overlap_permille, cross_permille, margin,
                                                 penalty, tau, gate, tmpl_index_base, out, n_out, boxes_out, matched_out);
        });
    });
}

int fdcm_search_exhaustive_detect_windows_objects(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                                                  const fdcm_pose_window* jobs, int64_t n_jobs, int32_t sx, int32_t sy, int32_t wrap,
                                                  const int32_t* objects, int32_t n_objects, const float* max_score,
                                                  const float* min_matched, int32_t max_detections, int32_t overlap_permille,
                                                  int32_t cross_permille, int32_t margin, int penalty, float tau, int gate,
                                                  int32_t tmpl_index_base, fdcm_match** out, int64_t* n_out, int32_t* boxes_out,
                                                  float* matched_out, int32_t* jobs_out) {
    return guarded([&] {
        require(gate == FDCM_GATE_WINNER || gate == FDCM_GATE_ALL, "gate must be FDCM_GATE_WINNER or FDCM_GATE_ALL");
        std::vector<float> ms, mm;
        check_object_limits(n_objects, max_score, true, min_matched, ms, mm);
        check_detect_limits(max_detections, overlap_permille, &cross_permille, margin);
        check_detect_windows_args(fm, templates, rot, jobs, n_jobs, sx, sy, wrap, penalty, tau, out, n_out);
        check_object_labels(templates, objects, n_objects);
        records_call(out, [&] {
            run_search_exhaustive_detect_windows_objects(const_cast<fdcm_featuremap*>(fm), templates, rot, jobs, n_jobs, sx, sy, objects,
                                                         n_objects, ms.data(), min_matched ? mm.data() : nullptr, max_detections,
                                                         overlap_permille, cross_permille, margin, penalty, tau, gate, tmpl_index_base, out,
                                                         n_out, boxes_out, matched_out, jobs_out);
        });
    });
}

// The line costs' checks, with the one output: nothing here touches the device.
int fdcm_matched_fractions(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot, const int32_t* poses,
                           int64_t n, float* fractions) {
    return guarded([&] {
        require(n >= 0, "n is negative");
        require(n == 0 || poses, "poses is null");
        require(n == 0 || fractions, "fractions is null");
        if (rot) check_rotations(rot);  // null: the lines as they are, a table of one rotation
        const int32_t n_rot = rot ? rot->n : 1, lim = 1 << 24;
        for (int64_t q = 0; q < n; ++q) {
            const int32_t* p = poses + 4 * q;
            require(p[0] >= 0, "poses: tmpl is outside the template set");
            require(p[1] >= 0 && p[1] < n_rot, rot ? "poses: a must be in [0, n - 1]" : "poses: a must be 0 without rotations");
            require(p[2] > -lim && p[2] < lim && p[3] > -lim && p[3] < lim, "poses: every translation must satisfy |t| < 2^24");
        }
        check_handles(fm, templates);
        if (rot) check_pivots(templates, rot);
        for (int64_t q = 0; q < n && templates->T > 0; ++q)
            require(poses[4 * q] < templates->T, "poses: tmpl is outside the template set");
        run_matched_fractions(const_cast<fdcm_featuremap*>(fm), templates, rot, poses, n, fractions);
    });
}

int fdcm_templates_matched_totals(const fdcm_templates* templates, float* totals) {
    return guarded([&] {
        require(templates != nullptr, "templates is null");
        require(totals != nullptr || templates->T == 0, "totals is null");
        templates_matched_totals(templates, totals);
    });
}

int fdcm_score_bound(float den, float max_score, float* bound) {
    return guarded([&] {
        require(max_score >= 0.f, "max_score must be >= 0 or +inf, never NaN");
        require(bound != nullptr, "bound is null");
        *bound = detect_score_bound(den, max_score);
    });
}

int fdcm_detect_score_bounds(const fdcm_templates* templates, int penalty, float tau, float max_score, float* bounds) {
    return guarded([&] {
        require(penalty == -1 || penalty == FDCM_DEFAULT_PENALTY || penalty == FDCM_EXPONENTIAL_PENALTY, "unknown penalty");
        require(std::isfinite(tau), "tau must be finite");
        require(max_score >= 0.f, "max_score must be >= 0 or +inf, never NaN");
        require(templates != nullptr, "templates is null");
        require(bounds != nullptr || templates->T == 0, "bounds is null");
        detect_score_bounds(templates, penalty, tau, max_score, bounds);
    });
}

int fdcm_templates_footprints(const fdcm_templates* templates, const fdcm_rotations* rot, int32_t margin, int32_t* boxes_out) {
    return guarded([&] {
        require(margin >= 0 && margin <= 4096, "margin must be in [0, 4096]");
        if (rot) check_rotations(rot);  // null: the lines as they are, a table of one rotation
        require(templates != nullptr, "templates is null");
        require(templates->T * (int64_t)(rot ? rot->n : 1) <= 0x7fffffffll, "T * n_rot must be at most 2^31 - 1");
        require(boxes_out != nullptr || templates->T == 0, "boxes_out is null");
        if (rot) check_pivots(templates, rot);
        templates_footprints(templates, rot, margin, boxes_out);
    });
}

int fdcm_lines_footprints(const float* lines, const int64_t* offsets, int64_t n_templates, const fdcm_rotations* rot, int32_t margin,
                          int32_t* boxes_out) {
    return guarded([&] {
        require(margin >= 0 && margin <= 4096, "margin must be in [0, 4096]");
        if (rot) check_rotations(rot);
        require(n_templates >= 0 && (n_templates == 0 || offsets), "bad offsets");
        if (n_templates == 0) return;
        require(offsets[0] == 0, "offsets[0] must be 0");
        for (int64_t i = 0; i < n_templates; ++i) require(offsets[i] <= offsets[i + 1], "offsets must be ascending");
        require(offsets[n_templates] == 0 || lines, "lines is null");
        require(n_templates * (int64_t)(rot ? rot->n : 1) <= 0x7fffffffll, "T * n_rot must be at most 2^31 - 1");
        require(boxes_out != nullptr, "boxes_out is null");
        if (rot && rot->pivots)
            for (int64_t i = 0; i < 2 * n_templates; ++i) require(std::isfinite(rot->pivots[i]), "rotations: pivots must be finite");
        lines_footprints(lines, offsets, n_templates, rot, margin, boxes_out);
    });
}

// Hull footprints: include/fdcm.h, "Hull footprints".  The footprints' checks with the three outputs: host only.
int fdcm_templates_footprint_spans(const fdcm_templates* templates, const fdcm_rotations* rot, int32_t margin, int64_t* row_offsets,
                                   int64_t* areas, int32_t* spans) {
    return guarded([&] {
        require(margin >= 0 && margin <= 4096, "margin must be in [0, 4096]");
        if (rot) check_rotations(rot);
        require(row_offsets != nullptr, "row_offsets is null");
        require(templates != nullptr, "templates is null");
        require(templates->T * (int64_t)(rot ? rot->n : 1) <= 0x7fffffffll, "T * n_rot must be at most 2^31 - 1");
        if (rot) check_pivots(templates, rot);
        templates_footprint_spans(templates, rot, margin, row_offsets, areas, spans);
    });
}

int fdcm_lines_footprint_spans(const float* lines, const int64_t* offsets, int64_t n_templates, const fdcm_rotations* rot, int32_t margin,
                               int64_t* row_offsets, int64_t* areas, int32_t* spans) {
    return guarded([&] {
        require(margin >= 0 && margin <= 4096, "margin must be in [0, 4096]");
        if (rot) check_rotations(rot);
        require(row_offsets != nullptr, "row_offsets is null");
        require(n_templates >= 0 && (n_templates == 0 || offsets), "bad offsets");
        row_offsets[0] = 0;
        if (n_templates == 0) return;
        require(offsets[0] == 0, "offsets[0] must be 0");
        for (int64_t i = 0; i < n_templates; ++i) require(offsets[i] <= offsets[i + 1], "offsets must be ascending");
        require(offsets[n_templates] == 0 || lines, "lines is null");
        require(n_templates * (int64_t)(rot ? rot->n : 1) <= 0x7fffffffll, "T * n_rot must be at most 2^31 - 1");
        if (rot && rot->pivots)
            for (int64_t i = 0; i < 2 * n_templates; ++i) require(std::isfinite(rot->pivots[i]), "rotations: pivots must be finite");
        lines_footprint_spans(lines, offsets, n_templates, rot, margin, row_offsets, areas, spans);
    });
}

// Line costs: include/fdcm.h, "Per-line caps and line costs".  Everything that needs no handle is checked first, the poses'
// templates against the set last: nothing here touches the device.
int fdcm_line_costs(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot, const int32_t* poses,
                    int64_t n, float** costs, int64_t* offsets) {
    if (costs) *costs = nullptr;
    return guarded([&] {
        require(n >= 0, "n is negative");
        require(n == 0 || poses, "poses is null");
        if (rot) check_rotations(rot);  // null: the lines as they are, a table of one rotation
        const int32_t n_rot = rot ? rot->n : 1, lim = 1 << 24;
        for (int64_t q = 0; q < n; ++q) {
            const int32_t* p = poses + 4 * q;
            require(p[0] >= 0, "poses: tmpl is outside the template set");
            require(p[1] >= 0 && p[1] < n_rot, rot ? "poses: a must be in [0, n - 1]" : "poses: a must be 0 without rotations");
            require(p[2] > -lim && p[2] < lim && p[3] > -lim && p[3] < lim, "poses: every translation must satisfy |t| < 2^24");
        }
        check_handles(fm, templates);
        require(costs && offsets, "null output");
        if (rot) check_pivots(templates, rot);
        for (int64_t q = 0; q < n && templates->T > 0; ++q)
            require(poses[4 * q] < templates->T, "poses: tmpl is outside the template set");
        try {
            run_line_costs(const_cast<fdcm_featuremap*>(fm), templates, rot, poses, n, costs, offsets);
        } catch (...) {
            std::free(*costs);
            *costs = nullptr;
            throw;
        }
    });
}

// Match lists: include/fdcm.h, "Match lists".  Everything that needs no handle is checked first, in the section's order; nothing
// here touches the device.
// the bound a call sets on its list: n <= 2^bits, 22 for the match calls, 20 for coverage and the fit, 16 for the selection
static void check_list_bound(int64_t n, int bits) {
    if (bits == 16) require(n <= ((int64_t)1 << 16), "n must be at most 2^16: cut a longer list with fdcm_matches_detect first");
    else if (bits == 20) require(n <= ((int64_t)1 << 20), "n must be at most 2^20");
    else require(n <= ((int64_t)1 << 22), "n must be at most 2^22");
}

// a list in three forms: host records, device records, or (matches NULL with on_device = 0) the last search's; the host
// calls, which have no last search, pass on_device = 1 for the test of the pointer
static void check_match_list(const fdcm_match* matches, int64_t n, int on_device, int bits = 22) {
    require(n >= 0, "n is negative");
    check_list_bound(n, bits);
    require(on_device == 0 || on_device == 1, "on_device must be 0 or 1");
    require(!(on_device == 1 && n > 0 && !matches), "matches is null");
}

// matches NULL with on_device = 0: the records of the last fdcm_search on the handle, as fdcm_topk takes them, under the
// call's bound.
static void last_search_matches(const fdcm_featuremap* fm, const fdcm_match*& matches, int64_t& n, int& on_device, int bits = 22) {
    if (matches || on_device) return;
    matches = fm->search.out.as<fdcm_match>();
    n = fm->last_n_out;
    on_device = 1;
    check_list_bound(n, 22);
    require(n == 0 || matches, "the handle holds no matches of a search");
    check_list_bound(n, bits);
}

// what both detect calls on a match list check behind their limits (min_matched: the single call's gate, or null)
static void check_matches_detect_args(const fdcm_featuremap* fm, const fdcm_templates* templates, int penalty, float tau,
                                      const float* min_matched, int rescore, fdcm_match** out, int64_t* n_out) {
    require(penalty == -1 || penalty == FDCM_DEFAULT_PENALTY || penalty == FDCM_EXPONENTIAL_PENALTY, "unknown penalty");
    require(std::isfinite(tau), "tau must be finite");
    if (min_matched) require(*min_matched >= 0.f && *min_matched <= 1.f, "min_matched must be in [0, 1], never NaN");
    require(rescore == 0 || rescore == 1, "rescore must be 0 or 1");
    require(out && n_out, "null output");
    check_handles(fm, templates);
}


int fdcm_matches_footprints(const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int32_t tmpl_index_base,
                            int32_t margin, int32_t* boxes_out) {
    return guarded([&] {
        check_match_list(matches, n, 1);
        require(margin >= 0 && margin <= 4096, "margin must be in [0, 4096]");
        require(n == 0 || boxes_out, "boxes_out is null");
        require(templates != nullptr, "templates is null");
        matches_footprints(templates, matches, n, tmpl_index_base, margin, boxes_out);
    });
}

int fdcm_matches_verify(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int on_device,
                        int32_t tmpl_index_base, float* scores_out, float* fractions_out, float* costs_out) {
    return guarded([&] {
        check_match_list(matches, n, on_device);
        require(scores_out || fractions_out || costs_out, "every output is null");
        check_handles(fm, templates);
        last_search_matches(fm, matches, n, on_device);
        MatchesIn in{MatchList{matches, n, on_device != 0, tmpl_index_base}};
        in.verify = {scores_out, fractions_out, costs_out};
        run_matches(const_cast<fdcm_featuremap*>(fm), templates, in);
    });
}

int fdcm_matches_detect(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int on_device,
                        int32_t tmpl_index_base, float max_score, int32_t max_detections, int32_t overlap_permille, int32_t margin,
                        int penalty, float tau, float min_matched, int rescore, fdcm_match** out, int64_t* n_out, int32_t* indices_out,
                        int32_t* boxes_out, float* matched_out) {
    return guarded([&] {
        check_match_list(matches, n, on_device);
        require(max_score >= 0.f, "max_score must be >= 0 or +inf, never NaN");
        check_detect_limits(max_detections, overlap_permille, nullptr, margin);
        check_matches_detect_args(fm, templates, penalty, tau, &min_matched, rescore, out, n_out);
        last_search_matches(fm, matches, n, on_device);
        const MatchesDetect det{max_score == 0.f ? 0.f : max_score, max_detections, overlap_permille, margin, penalty, tau,
                                min_matched == 0.f ? 0.f : min_matched, rescore};
        MatchesIn in{MatchList{matches, n, on_device != 0, tmpl_index_base}};
        in.det = &det;
        in.detect = {out, n_out, indices_out, boxes_out, matched_out};
        records_call(out, [&] { run_matches(const_cast<fdcm_featuremap*>(fm), templates, in); });
    });
}

// Match lists, refinement: include/fdcm.h, "Match lists: refinement".  The list's checks, then the delta table, the window, the
// outputs and last the handles (the pivots need the set's template count).
int fdcm_matches_refine(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int on_device,
                        int32_t tmpl_index_base, const fdcm_rotations* rot, int32_t centre, int32_t hx, int32_t hy, int32_t sx, int32_t sy,
                        fdcm_match* out, int out_on_device, int32_t* pose_out) {
    return guarded([&] {
        check_match_list(matches, n, on_device);
        if (rot) check_rotations(rot);  // null: nothing rotated, a table of one delta
        const int32_t na = rot ? rot->n : 1;
        require(centre >= -1 && centre < na, "centre must be in [-1, na - 1]");
        require(hx >= 0 && hx <= 4096 && hy >= 0 && hy <= 4096, "hx and hy must be in [0, 4096]");
        require(sx >= 1 && sx <= 4096 && sy >= 1 && sy <= 4096, "sx and sy must be in [1, 4096]");
        require((int64_t)na * (2 * hx + 1) * (int64_t)(2 * hy + 1) <= 65536, "na (2 hx + 1) (2 hy + 1) must be at most 65536");
        require(n == 0 || out, "out is null");
        require(out_on_device == 0 || out_on_device == 1, "out_on_device must be 0 or 1");
        check_handles(fm, templates);
        if (rot) check_pivots(templates, rot);
        last_search_matches(fm, matches, n, on_device);
        require(n == 0 || out, "out is null");
        run_matches_refine(const_cast<fdcm_featuremap*>(fm), templates, MatchList{matches, n, on_device != 0, tmpl_index_base}, rot, centre,
                           hx, hy, sx, sy, out, out_on_device != 0, pose_out);
    });
}

// Match lists with objects and hull shapes: include/fdcm.h, "Match lists: objects and hull shapes".  fdcm_matches_detect's
// checks with the per-object arrays in place of its two thresholds, then the labels; the one refusal behind GPU work is the
// span table's size (run_matches).
int fdcm_matches_detect_objects(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n,
                                int on_device, int32_t tmpl_index_base, const int32_t* objects, int32_t n_objects, const float* max_score,
                                const float* min_matched, int32_t max_detections, int32_t overlap_permille, int32_t cross_permille,
                                int32_t margin, int penalty, float tau, int rescore, fdcm_match** out, int64_t* n_out,
                                int32_t* indices_out, int32_t* boxes_out, float* matched_out) {
    return guarded([&] {
        check_match_list(matches, n, on_device);
        std::vector<float> ms, mm;
        check_object_limits(n_objects, max_score, true, min_matched, ms, mm);
        check_detect_limits(max_detections, overlap_permille, &cross_permille, margin);
        check_matches_detect_args(fm, templates, penalty, tau, nullptr, rescore, out, n_out);
        check_object_labels(templates, objects, n_objects);
        last_search_matches(fm, matches, n, on_device);
        const MatchesDetect det{0.f, max_detections, overlap_permille, margin, penalty, tau, 0.f, rescore};
        const MatchesObjectsIn ob{objects, n_objects, ms.data(), min_matched ? mm.data() : nullptr, cross_permille};
        MatchesIn in{MatchList{matches, n, on_device != 0, tmpl_index_base}};
        in.det = &det;
        in.objects = &ob;
        in.detect = {out, n_out, indices_out, boxes_out, matched_out};
        records_call(out, [&] { run_matches(const_cast<fdcm_featuremap*>(fm), templates, in); });
    });
}

int fdcm_matches_footprint_spans(const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int32_t tmpl_index_base,
                                 int32_t margin, int64_t* row_offsets, int64_t* areas, int32_t* spans) {
    return guarded([&] {
        check_match_list(matches, n, 1);
        require(margin >= 0 && margin <= 4096, "margin must be in [0, 4096]");
        require(row_offsets != nullptr, "row_offsets is null");
        require(templates != nullptr, "templates is null");
        matches_footprint_spans(templates, matches, n, tmpl_index_base, margin, row_offsets, areas, spans);
    });
}

int fdcm_matches_shapes(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int on_device,
                        int32_t tmpl_index_base, int32_t margin, int64_t* row_offsets, int64_t* areas, int32_t* spans) {
    return guarded([&] {
        check_match_list(matches, n, on_device);
        require(margin >= 0 && margin <= 4096, "margin must be in [0, 4096]");
        require(row_offsets != nullptr, "row_offsets is null");
        check_handles(fm, templates);
        require(matches || on_device || n == 0, "matches is null");  // (the rows are sized by n: the last search is no form here)
        const MatchesShapesOut so{margin, row_offsets, areas, spans};
        MatchesIn in{MatchList{matches, n, on_device != 0, tmpl_index_base}};
        in.shapes = &so;
        run_matches(const_cast<fdcm_featuremap*>(fm), templates, in);
    });
}

// Scene coverage: include/fdcm.h, "Scene coverage".  The line costs' checks, then the call's own; everything that needs no handle
// first, and nothing on the device.
// The checks fdcm_scene_coverage and fdcm_scene_select share, in the section's order: the pose list, the parameters and the
// image (front), then, after the call's own output pointers, the residual, the handles and the frame (back).
static void check_coverage_front(const uint8_t* labels, int64_t width, int64_t height, const fdcm_rotations* rot, const int32_t* poses,
                                 int64_t n, const fdcm_coverage_params* params) {
    require(n >= 0, "n is negative");
    require(n == 0 || poses, "poses is null");
    if (rot) check_rotations(rot);  // null: the lines as they are, a table of one rotation
    const int32_t n_rot = rot ? rot->n : 1, lim = 1 << 24;
    for (int64_t q = 0; q < n; ++q) {
        const int32_t* p = poses + 4 * q;
        require(p[0] >= 0, "poses: tmpl is outside the template set");
        require(p[1] >= 0 && p[1] < n_rot, rot ? "poses: a must be in [0, n - 1]" : "poses: a must be 0 without rotations");
        require(p[2] > -lim && p[2] < lim && p[3] > -lim && p[3] < lim, "poses: every translation must satisfy |t| < 2^24");
    }
    require(n <= ((int64_t)1 << 20), "n must be at most 2^20");
    require(params != nullptr, "params is null");
    require(params->radius >= 0 && params->radius <= 32, "radius must be in [0, 32]");
    require(params->bin_tolerance >= 0, "bin_tolerance must be in [0, m / 2]");
    require(params->margin >= 0 && params->margin <= 4096, "margin must be in [0, 4096]");
    require(labels != nullptr, "labels is null");
    require(width >= 1 && width <= 4096 && height >= 1 && height <= 4096, "width and height must be in [1, 4096]");
}

static void check_coverage_back(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height,
                                const fdcm_templates* templates, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                                const fdcm_coverage_params* params, const uint8_t* residual_out, float* bx, float* by) {
    if (residual_out)
        require(residual_out + width * height <= labels || labels + width * height <= residual_out, "residual_out must not overlap labels");
    check_handles(fm, templates);
    if (rot) check_pivots(templates, rot);
    for (int64_t q = 0; q < n && templates->T > 0; ++q)
        require(poses[4 * q] < templates->T, "poses: tmpl is outside the template set");
    *bx = *by = 0.f;
    if (fm->W > 0 && fm->H > 0 && fm->m > 0) {  // (an empty map has no frame and no slices: nothing is explained on it)
        require(params->bin_tolerance <= fm->m / 2, "bin_tolerance must be in [0, m / 2]");
        *bx = fm->tx; *by = fm->ty;  // whole pixels below 2^24 are exact floats
        require(*bx >= 0.f && *by >= 0.f && *bx < 16777216.f && *by < 16777216.f && *bx == std::floor(*bx) && *by == std::floor(*by),
                "the map's scene translation must be whole non-negative pixels (a map built from an image or from labels)");
        require(width + 2 * (int64_t)*bx == fm->W && height + 2 * (int64_t)*by == fm->H,
                "the map's size must be (width + 2 bx, height + 2 by) for its scene translation (bx, by)");
    }
}

// the rule's parameters and the outputs of a selection call (fdcm_scene_select, fdcm_matches_select)
static void check_select_params(const fdcm_select_params* sel, const int32_t* selected_out, const int32_t* counts_out, const int64_t* n_out) {
    require(sel != nullptr, "sel is null");
    require(sel->min_coverage_permille >= 0 && sel->min_coverage_permille <= 1000, "min_coverage_permille must be in [0, 1000]");
    require(sel->min_new_permille >= 0 && sel->min_new_permille <= 1000, "min_new_permille must be in [0, 1000]");
    require(sel->min_pixels >= 1 && sel->min_pixels <= (1 << 24), "min_pixels must be in [1, 2^24]");
    require(sel->max_selected >= 1 && sel->max_selected <= 4096, "max_selected must be in [1, 4096]");
    require(selected_out != nullptr, "selected_out is null");
    require(counts_out != nullptr, "counts_out is null");
    require(n_out != nullptr, "n_out is null");
}

// Scene selection: include/fdcm.h, "Scene selection".  Scene coverage's checks around the call's own.
int fdcm_scene_select(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int on_device,
                      const fdcm_templates* templates, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                      const fdcm_coverage_params* params, const fdcm_select_params* sel, int32_t* selected_out, int32_t* counts_out,
                      int64_t* n_out, uint8_t* residual_out) {
    return guarded([&] {
        check_coverage_front(labels, width, height, rot, poses, n, params);
        check_select_params(sel, selected_out, counts_out, n_out);
        float bx, by;
        check_coverage_back(fm, labels, width, height, templates, rot, poses, n, params, residual_out, &bx, &by);
        run_scene_select(const_cast<fdcm_featuremap*>(fm), labels, (int)width, (int)height, on_device != 0, (int)bx, (int)by, templates, rot,
                         poses, n, *params, *sel, selected_out, counts_out, n_out, residual_out);
    });
}

int fdcm_scene_coverage(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int on_device,
                        const fdcm_templates* templates, const fdcm_rotations* rot, const int32_t* poses, int64_t n,
                        const fdcm_coverage_params* params, int32_t* counts_out, uint8_t* residual_out) {
    return guarded([&] {
        check_coverage_front(labels, width, height, rot, poses, n, params);
        require(n == 0 || counts_out, "counts_out is null");
        float bx, by;
        check_coverage_back(fm, labels, width, height, templates, rot, poses, n, params, residual_out, &bx, &by);
        run_scene_coverage(const_cast<fdcm_featuremap*>(fm), labels, (int)width, (int)height, on_device != 0, (int)bx, (int)by, templates, rot,
                           poses, n, *params, counts_out, residual_out);
    });
}

// Match lists: scene coverage and selection (include/fdcm.h).  The match calls' checks of the list with the call's own bound
// on n (check_list_bound's bits: 20, or 16 for the selection), then scene coverage's of the parameters and the image; after the
// call's own outputs the residual, the handles and the frame, and last the records of the last search under the same bound.
static void check_matches_coverage_front(const uint8_t* labels, int64_t width, int64_t height, const fdcm_match* matches, int64_t n,
                                         int on_device, int bits, const fdcm_coverage_params* params) {
    check_match_list(matches, n, on_device, bits);
    check_coverage_front(labels, width, height, nullptr, nullptr, 0, params);
}

int fdcm_matches_coverage(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int labels_on_device,
                          const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int matches_on_device,
                          int32_t tmpl_index_base, const fdcm_coverage_params* params, int32_t* counts_out, uint8_t* residual_out) {
    return guarded([&] {
        check_matches_coverage_front(labels, width, height, matches, n, matches_on_device, 20, params);
        require(n == 0 || counts_out, "counts_out is null");
        float bx, by;
        check_coverage_back(fm, labels, width, height, templates, nullptr, nullptr, 0, params, residual_out, &bx, &by);
        last_search_matches(fm, matches, n, matches_on_device, 20);
        require(n == 0 || counts_out, "counts_out is null");
        run_matches_coverage(const_cast<fdcm_featuremap*>(fm), labels, (int)width, (int)height, labels_on_device != 0, (int)bx, (int)by,
                             templates, MatchList{matches, n, matches_on_device != 0, tmpl_index_base}, *params, counts_out, residual_out);
    });
}

int fdcm_matches_select(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int labels_on_device,
                        const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int matches_on_device,
                        int32_t tmpl_index_base, const fdcm_coverage_params* params, const fdcm_select_params* sel, int32_t* selected_out,
                        int32_t* counts_out, int64_t* n_out, uint8_t* residual_out) {
    return guarded([&] {
        check_matches_coverage_front(labels, width, height, matches, n, matches_on_device, 16, params);
        check_select_params(sel, selected_out, counts_out, n_out);
        float bx, by;
        check_coverage_back(fm, labels, width, height, templates, nullptr, nullptr, 0, params, residual_out, &bx, &by);
        last_search_matches(fm, matches, n, matches_on_device, 16);
        run_matches_select(const_cast<fdcm_featuremap*>(fm), labels, (int)width, (int)height, labels_on_device != 0, (int)bx, (int)by,
                           templates, MatchList{matches, n, matches_on_device != 0, tmpl_index_base}, *params, *sel, selected_out, counts_out,
                           n_out, residual_out);
    });
}

// Match lists, pose fit: include/fdcm.h, "Match lists: pose fit".  The coverage call's checks around the call's own.
int fdcm_matches_fit(const fdcm_featuremap* fm, const uint8_t* labels, int64_t width, int64_t height, int labels_on_device,
                     const fdcm_templates* templates, const fdcm_match* matches, int64_t n, int matches_on_device, int32_t tmpl_index_base,
                     const fdcm_coverage_params* params, const fdcm_fit_params* fit, fdcm_match* out, int out_on_device, int32_t* info_out,
                     float* rms_out) {
    return guarded([&] {
        check_matches_coverage_front(labels, width, height, matches, n, matches_on_device, 20, params);
        require(fit != nullptr, "fit is null");
        require(fit->iterations >= 1 && fit->iterations <= 8, "iterations must be in [1, 8]");
        require(fit->min_pixels >= 3, "min_pixels must be at least 3");
        require(fit->damping >= 0.0, "damping must be a number >= 0");  // (false for a NaN)
        require(fit->max_shift >= 0.0, "max_shift must be a number >= 0");
        require(fit->max_angle >= 0.0, "max_angle must be a number >= 0");
        require(n == 0 || out, "out is null");
        require(out_on_device == 0 || out_on_device == 1, "out_on_device must be 0 or 1");
        float bx, by;
        check_coverage_back(fm, labels, width, height, templates, nullptr, nullptr, 0, params, nullptr, &bx, &by);
        last_search_matches(fm, matches, n, matches_on_device, 20);
        require(n == 0 || out, "out is null");
        run_matches_fit(const_cast<fdcm_featuremap*>(fm), labels, (int)width, (int)height, labels_on_device != 0, (int)bx, (int)by, templates,
                        MatchList{matches, n, matches_on_device != 0, tmpl_index_base}, *params, *fit, out, out_on_device != 0, info_out,
                        rms_out);
    });
}

int fdcm_score_map_rotations(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_rotations* rot,
                             const fdcm_grid* grid, float* out_host) {
    return guarded([&] {
        check_rotations(rot);
        check_exhaustive_args(fm, templates, grid);
        check_pivots(templates, rot);
        require(out_host != nullptr || templates->T == 0, "out_host is null");
        run_score_map(const_cast<fdcm_featuremap*>(fm), templates, rot, *grid, out_host, nullptr);
    });
}

int fdcm_score_map(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_grid* grid, float* out_host) {
    return guarded([&] {
        check_exhaustive_args(fm, templates, grid);
        require(out_host != nullptr || templates->T == 0, "out_host is null");
        run_score_map(const_cast<fdcm_featuremap*>(fm), templates, nullptr, *grid, out_host, nullptr);
    });
}

int fdcm_score_map_device(const fdcm_featuremap* fm, const fdcm_templates* templates, const fdcm_grid* grid, float* out_device) {
    return guarded([&] {
        check_exhaustive_args(fm, templates, grid);
        require(out_device != nullptr || templates->T == 0, "out_device is null");
        run_score_map(const_cast<fdcm_featuremap*>(fm), templates, nullptr, *grid, nullptr, out_device);
    });
}

int fdcm_search_last_timing(const fdcm_featuremap* fm, fdcm_search_timing* t) {
    return guarded([&] {
        require(fm && t, "null argument");
        *t = fm->last_search;
    });
}

void fdcm_matches_free(fdcm_match* m) { result_release(m); }

int fdcm_blocks_to_host(const void* blocks_device, int32_t n_blocks, int64_t capacity_records, void* stream, fdcm_match** out,
                        int64_t* n_out) {
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    int rc = guarded([&] {
        require(out && n_out && n_blocks >= 0 && capacity_records >= 0 && (n_blocks == 0 || blocks_device), "bad arguments");
        require((int64_t)n_blocks * capacity_records < (int64_t)1 << 40, "too many records");
        if (n_blocks == 0 || capacity_records == 0) { *out = result_acquire(64); return; }
        // the kernel runs on the device that holds the blocks (whatever this thread's current device is), and the
        // caller's current device is left as it was
        int prev = -1;
        (void)hipGetDevice(&prev);
        hipPointerAttribute_t attr{};
        const int dev = hipPointerGetAttributes(&attr, blocks_device) == hipSuccess ? attr.device : g_device;
        (void)hipGetLastError();
        FDCM_HIP(hipSetDevice(dev));
        try {
            blocks_to_host((hipStream_t)stream, blocks_device, n_blocks, capacity_records, out, n_out);
        } catch (...) {
            if (prev >= 0) (void)hipSetDevice(prev);
            throw;
        }
        if (prev >= 0) (void)hipSetDevice(prev);
    });
    if (rc != FDCM_OK && out && *out) { result_release(*out); *out = nullptr; }
    return rc;
}

int fdcm_filter_in_range(const float* lines, int64_t n_lines, const float center[2], float low_boundary,
                         float high_boundary, int64_t* out_indices, int64_t* n_out) {
    return guarded([&] {
        require(n_lines >= 0 && (n_lines == 0 || lines) && center && n_out && (n_lines == 0 || out_indices), "bad arguments");
        int64_t k = 0;
        for (int64_t i = 0; i < n_lines; ++i) {  // filterInRange, concentricrange.h:73-84
            const float* p = lines + 4 * i;
            const float cx = (p[2] + p[0]) / 2 - center[0], cy = (p[3] + p[1]) / 2 - center[1];
            const float rad = std::sqrt(cx * cx + cy * cy);
            if (rad > (low_boundary - FLT_EPSILON) && rad < high_boundary) out_indices[k++] = i;
        }
        *n_out = k;
    });
}

// ------------------------------------------------------------------------------------------ tail
int fdcm_penalize(int penalty, float tau, fdcm_match* matches, int64_t n, const float* template_lengths,
                  int64_t n_templates) {
    return guarded([&] {
        require(n >= 0 && (n == 0 || matches), "bad matches");
        require(penalty == FDCM_DEFAULT_PENALTY || penalty == FDCM_EXPONENTIAL_PENALTY, "unknown penalty");
        // defaultpenalty.cpp:37-41 / exponentialpenalty.cpp:42-46; templatelengths.at() -> out_of_range
        for (int64_t i = 0; i < n; ++i)
            if (matches[i].tmpl_idx < 0 || matches[i].tmpl_idx >= n_templates)
                throw std::string("In penalize, the size of templatelengths is not consistent with match template indices");
        if (penalty == FDCM_DEFAULT_PENALTY) {
            for (int64_t i = 0; i < n; ++i) matches[i].score = matches[i].score / std::max(template_lengths[matches[i].tmpl_idx], 1e-6f);
            return;
        }
        // The divisor pow(len, tau) depends on the template only: one powf per template that occurs, not per match
        // (the same float operands give the same float result, so the scores are the reference's bit for bit).
        if (n < n_templates) {
            for (int64_t i = 0; i < n; ++i)
                matches[i].score = matches[i].score / std::pow(std::max(template_lengths[matches[i].tmpl_idx], 1e-6f), tau);
            return;
        }
        std::vector<float> div((size_t)n_templates);
        for (int64_t t = 0; t < n_templates; ++t) div[(size_t)t] = std::pow(std::max(template_lengths[t], 1e-6f), tau);
        for (int64_t i = 0; i < n; ++i) matches[i].score = matches[i].score / div[(size_t)matches[i].tmpl_idx];
    });
}

// sortMatches (matchstrategy.h:46-50): std::sort by score -- unstable, and which of two equal scores comes first is whatever
// libstdc++'s introsort does (a frame of 27 000 matches always holds a few equal scores, so nothing but that algorithm gives the
// reference's list).  Its moves depend on the comparisons only, so (a) sorting (score, position) pairs and gathering the records
// ends in the same permutation, and (b) so does running it on a few threads: introsort recurses on the right part of every
// partition and loops on the left, the parts never exchange elements again, and the closing insertion sort never moves an
// element across a partition boundary (everything left of it is <= everything right of it).  Here the first three partition
// levels hand their right parts to a small persistent pool and every part then runs libstdc++'s own std::__introsort_loop +
// std::__final_insertion_sort: 1.27 -> 0.49 ms for 27 025 records on the GPU box's host (tools/sim/sort_pool_bench.cpp;
// tests/test_matchlist.py compares with std::sort on the reference's Match structs, ties, +-0 and +-inf included).  Lists below
// 8192 records, lists with a NaN score (no strict weak order: the serial scan's behaviour is its own) and calls that find the
// pool busy take the plain std::sort.
namespace {
#if defined(__GLIBCXX__)
struct SortKey { float score; uint32_t pos; };
struct SortKeyLess { bool operator()(const SortKey& a, const SortKey& b) const { return a.score < b.score; } };
class SortPool {
    std::mutex mu;
    std::condition_variable cv_task, cv_done;
    std::deque<std::function<void()>> q;
    int pending = 0;
    void loop() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv_task.wait(lk, [&] { return !q.empty(); });
            auto f = std::move(q.front());
            q.pop_front();
            lk.unlock();
            f();
            lk.lock();
            if (--pending == 0) cv_done.notify_all();
        }
    }
public:
    std::mutex in_use;  // one sort at a time
    explicit SortPool(int helpers) {
        for (int i = 0; i < helpers; ++i) std::thread([this] { loop(); }).detach();  // (they live as long as the process: the pool is never destroyed)
    }
    void submit(std::function<void()> f) {
        { std::lock_guard<std::mutex> lk(mu); ++pending; q.push_back(std::move(f)); }
        cv_task.notify_one();
    }
    void help_and_wait() {  // the caller's thread works the queue too, then waits for the helpers' last tasks
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            if (!q.empty()) {
                auto f = std::move(q.front());
                q.pop_front();
                lk.unlock();
                f();
                lk.lock();
                if (--pending == 0) cv_done.notify_all();
                continue;
            }
            if (pending == 0) return;
            cv_done.wait(lk, [&] { return pending == 0 || !q.empty(); });
        }
    }
};
SortPool* sort_pool() {
    static SortPool* p = [] {
        const unsigned hc = std::thread::hardware_concurrency();
        return hc >= 4 ? new SortPool((int)std::min(7u, hc - 1)) : nullptr;
    }();
    return p;
}
void sort_part(SortKey* first, SortKey* last, long depth, int levels, SortPool* P) {
    auto cmp = __gnu_cxx::__ops::__iter_comp_iter(SortKeyLess{});
    while (levels > 0 && last - first > 2048 && depth > 0) {  // std::__introsort_loop's own steps, the right part to the pool
        --depth; --levels;
        SortKey* cut = std::__unguarded_partition_pivot(first, last, cmp);
        P->submit([=] { sort_part(cut, last, depth, levels, P); });
        last = cut;
    }
    std::__introsort_loop(first, last, depth, cmp);
    std::__final_insertion_sort(first, last, cmp);
}
bool sort_matches_parallel(fdcm_match* matches, int64_t n) {
    if (n < 8192 || n > (int64_t)UINT32_MAX) return false;
    SortPool* P = sort_pool();
    if (!P) return false;
    std::unique_lock<std::mutex> use(P->in_use, std::try_to_lock);
    if (!use.owns_lock()) return false;
    std::vector<SortKey> key((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (matches[i].score != matches[i].score) return false;  // NaN
        key[(size_t)i] = {matches[i].score, (uint32_t)i};
    }
    sort_part(key.data(), key.data() + n, (long)std::__lg(n) * 2, 3, P);
    P->help_and_wait();
    std::vector<fdcm_match> out((size_t)n);
    for (int64_t i = 0; i < n; ++i) out[(size_t)i] = matches[key[(size_t)i].pos];
    std::memcpy(matches, out.data(), (size_t)n * sizeof(fdcm_match));
    return true;
}
#else
bool sort_matches_parallel(fdcm_match*, int64_t) { return false; }
#endif
}  // namespace

int fdcm_sort_matches(fdcm_match* matches, int64_t n) {
    return guarded([&] {
        require(n >= 0 && (n == 0 || matches), "bad matches");
        if (sort_matches_parallel(matches, n)) return;
        std::sort(matches, matches + n, [](const fdcm_match& a, const fdcm_match& b) { return a.score < b.score; });
    });
}

// sortMatches(matches, maxNumCandidates), matchstrategy.h:52-55: std::partial_sort of the first min(k, n) places
int fdcm_partial_sort_matches(fdcm_match* matches, int64_t n, int64_t max_num_candidates) {
    return guarded([&] {
        require(n >= 0 && (n == 0 || matches), "bad matches");
        require(max_num_candidates >= 0, "max_num_candidates must be >= 0");
        std::partial_sort(matches, matches + std::min<int64_t>(max_num_candidates, n), matches + n,
                          [](const fdcm_match& a, const fdcm_match& b) { return a.score < b.score; });
    });
}

// ------------------------------------------------------------------------------------------ line files (fdcm_lineio.cpp)
int fdcm_lines_read(const char* path, float** lines, int64_t* n_lines) {
    return guarded([&] {
        require(path && lines && n_lines, "null argument");
        *lines = nullptr; *n_lines = 0;
        lines_read(path, lines, n_lines);
    });
}
int fdcm_lines_write(const char* path, const float* lines, int64_t n_lines) {
    return guarded([&] {
        require(path && n_lines >= 0 && (n_lines == 0 || lines), "bad arguments");
        lines_write(path, lines, n_lines);
    });
}
void fdcm_lines_free(float* lines) { std::free(lines); }

// ------------------------------------------------------------------------------------------ templates from a mesh (fdcm_mesh.hip)
int fdcm_mesh_create(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, double crease_cos, fdcm_mesh** out) {
    return guarded([&] {
        require(out != nullptr, "out is null");
        *out = nullptr;
        require(vertices != nullptr, "vertices is null");
        require(faces != nullptr, "faces is null");
        require(n_vertices >= 1 && n_vertices <= ((int64_t)1 << 22), "n_vertices must be in [1, 2^22]");
        require(n_faces >= 1 && n_faces <= ((int64_t)1 << 22), "n_faces must be in [1, 2^22]");
        require(crease_cos >= -1.0 && crease_cos <= 1.0, "crease_cos must be in [-1, 1]");
        *out = mesh_create(vertices, n_vertices, faces, n_faces, crease_cos);
    });
}
int fdcm_mesh_free(fdcm_mesh* mesh) {
    delete mesh;
    return FDCM_OK;
}
int fdcm_mesh_info(const fdcm_mesh* mesh, int64_t* n_edges, int64_t* n_sharp, int64_t* n_boundary) {
    return guarded([&] {
        require(mesh != nullptr, "mesh is null");
        if (n_edges) *n_edges = mesh->E;
        if (n_sharp) *n_sharp = mesh->n_sharp;
        if (n_boundary) *n_boundary = mesh->n_boundary;
    });
}
int fdcm_mesh_edges(const fdcm_mesh* mesh, int32_t* verts, int32_t* faces, uint8_t* sharp) {
    return guarded([&] {
        require(mesh != nullptr, "mesh is null");
        for (int64_t e = 0; e < mesh->E; ++e) {
            if (verts) { verts[2 * e] = mesh->edges[4 * e]; verts[2 * e + 1] = mesh->edges[4 * e + 1]; }
            if (faces) { faces[2 * e] = mesh->edges[4 * e + 2]; faces[2 * e + 1] = mesh->edges[4 * e + 3]; }
            if (sharp) sharp[e] = mesh->sharp[e];
        }
    });
}
static void check_view(const fdcm_mesh* mesh, const float* views, int64_t n_views, float scale) {
    require(mesh != nullptr, "mesh is null");
    require(n_views >= 0 && n_views <= 65536, "n_views must be in [0, 2^16]");
    require(views != nullptr || n_views == 0, "views is null");
    require(std::isfinite(scale) && scale > 0.f, "scale must be finite and > 0");
    for (int64_t i = 0; i < 9 * n_views; ++i)
        if (!std::isfinite(views[i])) throw std::string("view " + std::to_string(i / 9) + " has an entry that is not finite");
}
static void check_line_params(const fdcm_mesh_line_params* params) {
    require(params != nullptr, "params is null");
    require(std::isfinite(params->depth_tol) && params->depth_tol >= 0.f, "depth_tol must be finite and >= 0");
    require(std::isfinite(params->min_length) && params->min_length >= 0.f, "min_length must be finite and >= 0");
    require(params->visibility == FDCM_MESH_VIS_ITEMS || params->visibility == FDCM_MESH_VIS_EXACT,
            "visibility must be FDCM_MESH_VIS_ITEMS or FDCM_MESH_VIS_EXACT");
    require(params->join_tolerance < 0.f || std::isfinite(params->join_tolerance), "join_tolerance must be negative (off) or finite");
}
int fdcm_mesh_view_lines_ex(const fdcm_mesh* mesh, const float* views, int64_t n_views, float scale, const fdcm_mesh_line_params* params,
                            float** lines_out, int64_t* offsets_out) {
    return guarded([&] {
        require(lines_out != nullptr, "lines_out is null");
        require(offsets_out != nullptr, "offsets_out is null");
        check_view(mesh, views, n_views, scale);
        check_line_params(params);
        *lines_out = nullptr;
        offsets_out[0] = 0;
        if (n_views > 0) mesh_view_lines(g_device, mesh, views, n_views, scale, *params, lines_out, offsets_out);
    });
}
int fdcm_mesh_view_lines(const fdcm_mesh* mesh, const float* views, int64_t n_views, float scale, float depth_tol, float min_length,
                         float** lines_out, int64_t* offsets_out) {
    const fdcm_mesh_line_params params = {depth_tol, min_length, FDCM_MESH_VIS_ITEMS, -1.f};
    return fdcm_mesh_view_lines_ex(mesh, views, n_views, scale, &params, lines_out, offsets_out);
}
int fdcm_mesh_view_items(const fdcm_mesh* mesh, const float* view, float scale, int32_t* box_out, uint64_t* keys_out, int64_t capacity) {
    return guarded([&] {
        require(box_out != nullptr, "box_out is null");
        require(view != nullptr, "view is null");
        check_view(mesh, view, 1, scale);
        require(capacity >= 0, "capacity must be >= 0");
        mesh_view_items(g_device, mesh, view, scale, box_out, keys_out, capacity);
    });
}
// the pinhole calls: the camera and the positions (check_view's scale is the focal length: both are finite and > 0)
static void check_camera(const fdcm_mesh* mesh, const float* views, const float* positions, int64_t n_views, const fdcm_mesh_camera* camera) {
    require(camera != nullptr, "camera is null");
    require(std::isfinite(camera->focal) && camera->focal > 0.f, "focal must be finite and > 0");
    require(std::isfinite(camera->near) && camera->near > 0.f, "near must be finite and > 0");
    check_view(mesh, views, n_views, camera->focal);
    require(positions != nullptr || n_views == 0, "positions is null");
    for (int64_t v = 0; v < n_views; ++v) {
        const float* t = positions + 3 * v;
        if (!std::isfinite(t[0]) || !std::isfinite(t[1]) || !std::isfinite(t[2]))
            throw std::string("position " + std::to_string(v) + " has an entry that is not finite");
        if (!(-t[2] > 0.f)) throw std::string("position " + std::to_string(v) + " is not in front of the camera (-t.z must be > 0)");
    }
}
int fdcm_mesh_view_lines_cam(const fdcm_mesh* mesh, const float* views, const float* positions, int64_t n_views, const fdcm_mesh_camera* camera,
                             const fdcm_mesh_line_params* params, float** lines_out, int64_t* offsets_out) {
    return guarded([&] {
        require(lines_out != nullptr, "lines_out is null");
        require(offsets_out != nullptr, "offsets_out is null");
        check_camera(mesh, views, positions, n_views, camera);
        check_line_params(params);
        *lines_out = nullptr;
        offsets_out[0] = 0;
        if (n_views > 0) mesh_view_lines_cam(g_device, mesh, views, positions, n_views, *camera, *params, lines_out, offsets_out);
    });
}
int fdcm_mesh_view_items_cam(const fdcm_mesh* mesh, const float* view, const float* position, const fdcm_mesh_camera* camera, int32_t* box_out,
                             uint64_t* keys_out, int64_t capacity) {
    return guarded([&] {
        require(box_out != nullptr, "box_out is null");
        require(view != nullptr, "view is null");
        require(position != nullptr, "position is null");
        check_camera(mesh, view, position, 1, camera);
        require(capacity >= 0, "capacity must be >= 0");
        mesh_view_items_cam(g_device, mesh, view, position, *camera, box_out, keys_out, capacity);
    });
}

// ------------------------------------------------------------------------------------------ self checks
int64_t fdcm_selftest_atanf(uint32_t first, uint32_t stride, uint64_t count) {
    if (stride == 0) stride = 1;
    unsigned nt = std::max(1u, std::thread::hardware_concurrency());
    std::vector<uint64_t> bad(nt, 0);
    std::vector<std::thread> th;
    for (unsigned w = 0; w < nt; ++w)
        th.emplace_back([&, w] {
            for (uint64_t i = w; i < count; i += nt) {
                const uint32_t u = first + (uint32_t)(i * stride);
                const float x = f_from_bits(u);
                const float a = atanf_glibc(x), b = atanf(x);
                if (bits_from_f(a) != bits_from_f(b) && !(f_isnan(a) && f_isnan(b))) ++bad[w];
            }
        });
    for (auto& t : th) t.join();
    uint64_t total = 0;
    for (auto b : bad) total += b;
    return (int64_t)total;
}

int fdcm_orientation_bins_mode(void) { return fdcm::orientation_bins_on_host() ? 1 : 0; }
int fdcm_selftest_sweep_order_counts(int64_t* from_history, int64_t* from_proxy) {
    return guarded([&] {
        require(from_history && from_proxy, "null argument");
        fdcm::sweep_order_counts(from_history, from_proxy);
    });
}
int fdcm_selftest_poison_fills(const int32_t* ids, int64_t n, int64_t* counts) {
    return guarded([&] {
        require(n >= 0 && (n == 0 || (ids && counts)), "null argument");
        for (int64_t i = 0; i < n; ++i) require(ids[i] >= 0 && ids[i] < FDCM_FILL_BUFFERS, "no such buffer");
        for (int64_t i = 0; i < n; ++i) counts[i] = fdcm::poison_fill_count(ids[i]);
    });
}
int fdcm_selftest_sweep_steals(fdcm_featuremap* fm, int64_t* count) {
    return guarded([&] {
        require(fm && count, "null argument");
        *count = 0;
        if (!fm->steal_counter()) return;
        finish_build(fm);
        FDCM_HIP(hipSetDevice(fm->device));
        int v = 0;
        FDCM_HIP(hipMemcpy(&v, fm->steal_counter(), sizeof(int), hipMemcpyDeviceToHost));
        *count = v;
    });
}
int fdcm_selftest_sweep_ranges(int n_seeded_columns) { return fdcm::sweep_ranges(n_seeded_columns, fdcm::test_switches().sweep_min_cols); }

}  // extern "C"
