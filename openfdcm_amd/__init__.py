"""openfdcm_amd -- MI355X-native engine for OpenFDCM's DT3 build + DefaultMatch search.

Mirrors the Python surface of the reference's pybind11 module for this path
(modules/python/src/{openfdcm,core,matching}.cpp): the same class,
function and keyword names, so `import openfdcm_amd as openfdcm` is a drop-in for
build_cpu_featuremap / search / penalize / sort_matches.  All compute runs in libfdcm_hip.so
(HIP kernels for gfx950) through the C ABI in include/fdcm.h; there is no CPU fallback.
"""
import enum as _enum

import numpy as _np

from . import _capi
from .matchlist import Match, MatchList, records_of  # noqa: F401
from . import engine as _engine
from .engine import DeviceFeatureMap, DeviceTemplates, FramePipeline, ShardedEngine, edge_labels, image_pyramid, image_pyramid_size, lines_from_image, lines_from_labels, search_raw, topk  # noqa: F401  (extensions)
from .engine import Mesh, mesh_view_lines, record_rotations, templates_from_mesh, view_rotations  # noqa: F401  (templates from a mesh)
from .engine import mesh_view_items, record_camera_poses, view_positions  # noqa: F401  (pinhole views)

__version__ = "0.10.0"  # API level of the reference this mirrors (openfdcm.cpp:43)


class distance(_enum.IntEnum):
    """core::Distance (imgproc.h:148; core.cpp:45-49)."""
    L2 = 0
    L2_SQUARED = 1
    L1 = 2


L2, L2_SQUARED, L1 = distance.L2, distance.L2_SQUARED, distance.L1


class ThreadPool:
    """Placeholder for BS::thread_pool (matching.cpp:86-101).  The GPU engine does not use host
    threads; the object only carries the count so reference call sites run unchanged."""

    def __init__(self, num_threads=None):
        import os
        self._n = int(num_threads) if num_threads else (os.cpu_count() or 1)

    def get_tasks_queued(self): return 0
    def get_tasks_running(self): return 0
    def get_tasks_total(self): return 0
    def get_thread_count(self): return self._n
    def get_thread_ids(self): return []
    def purge(self): return None
    def __repr__(self): return f"<ThreadPool: threads={self._n}, tasks queued=0, tasks running=0>"


class Dt3CpuParameters:
    """matching.cpp:51-60,103-114.  Keyword `dt3Coeff`, attribute `dt3_coeff`, as in the reference."""

    def __init__(self, depth=30, dt3Coeff=5.0, padding=2.2, distance=distance.L2):
        self.depth = int(depth)
        self.dt3_coeff = float(dt3Coeff)
        self.padding = float(padding)
        self.distance = globals()["distance"](int(distance))

    def __repr__(self):
        return f"<PyDt3CpuParameters: depth={self.depth}, dt3_coeff={self.dt3_coeff:f}, padding={self.padding:f}>"


class Dt3Cpu:
    """The DT3 feature map (dt3cpu.h:46-63), resident in HBM.

    Dt3Cpu(dt3map, scene_translation, feature_size) adopts caller slices like the reference's
    constructor (matching.cpp:73): dt3map is {angle: (H, W) array}.
    """

    _pool_key = None  # set by build_cpu_featuremap: where the device handle goes when this object is dropped

    def __init__(self, dt3map, scene_translation=(0.0, 0.0), feature_size=(0, 0), _device=None):
        if _device is not None:
            self._fm = _device
            return
        keys = sorted(float(_np.float32(k)) for k in dt3map)
        W, H = int(feature_size[0]), int(feature_size[1])
        vol = _np.zeros((len(keys), W, H), dtype=_np.float32)
        by_key = {float(_np.float32(k)): v for k, v in dt3map.items()}
        for i, k in enumerate(keys):
            img = _np.asarray(by_key[k], dtype=_np.float32)
            if img.shape != (H, W):
                raise ValueError(f"slice shape {img.shape} != (H, W) = {(H, W)}")
            vol[i] = img.T
        self._fm = DeviceFeatureMap.from_volume(_np.array(keys, dtype=_np.float32), vol, scene_translation)

    def get_scene_translation(self):
        return self._fm.scene_translation.copy()

    def get_feature_size(self):
        return _np.array([self._fm.width, self._fm.height], dtype=_np.uint64)

    def get_dt3_map(self):
        return {float(k): self._fm.slice(i) for i, k in enumerate(self._fm.keys)}

    def __del__(self):
        try:
            if self._pool_key is not None and self._fm._h:
                _featuremap_pool.give(self._pool_key, self._fm)
        except Exception:  # interpreter shutdown: the handle's own __del__ frees it
            pass

    def __repr__(self):
        t = self._fm.scene_translation
        return (f"<Dt3Cpu: scene translation=({t[0]:f}, {t[1]:f}), "
                f"feature size=({self._fm.width}, {self._fm.height})>")


class FeatureMap:
    """Type-erased feature map (featuremap.h:98-124).  Wraps without copying the volume.

    The reference's Python module binds only the constructor and __repr__ (matching.cpp:66-70); the three
    methods below are the C++ class's (featuremap.h:109-121), served by the HIP kernels of the seam
    (fdcm_featuremap_minmax_translation / fdcm_featuremap_evaluate)."""

    def __init__(self, dt3):
        if isinstance(dt3, FeatureMap):
            dt3 = dt3._dt3
        if not isinstance(dt3, Dt3Cpu):
            raise TypeError("FeatureMap expects a Dt3Cpu")
        self._dt3 = dt3

    def get_feature_size(self):
        return self._dt3.get_feature_size()

    def minmax_translation(self, tmpl, align_vec):
        return self._dt3._fm.minmax_translation(tmpl, align_vec)

    def evaluate(self, templates, translations):
        return self._dt3._fm.evaluate(templates, translations)

    def __repr__(self): return "<FeatureMap>"


class _FeatureMapPool:
    """Device feature maps whose `Dt3Cpu` was dropped, kept for the next `build_cpu_featuremap` with the same
    parameters.  The reference's callers build a new feature map every frame (matching.cpp:116-130: a fresh Dt3Cpu of
    O(V) host memory each call); here a fresh handle is two volumes of HBM, workspaces and a stream -- allocating and
    freeing them costs more than the build -- so `fm = build_cpu_featuremap(scene, params)` in a loop alternates
    between two handles (the old `fm` is dropped after the new one exists) and each call is a rebuild.
    At most PER_KEY idle handles per parameter set and TOTAL in all; `clear_featuremap_pool()` frees them."""
    PER_KEY, TOTAL = 2, 4

    def __init__(self):
        self._idle = {}  # (depth, coeff, padding, distance, device) -> [DeviceFeatureMap]

    def take(self, key):
        lst = self._idle.get(key)
        return lst.pop() if lst else None

    def give(self, key, fm):
        lst = self._idle.setdefault(key, [])
        if len(lst) >= self.PER_KEY or sum(len(v) for v in self._idle.values()) >= self.TOTAL:
            fm.close()
        else:
            lst.append(fm)

    def clear(self):
        idle, self._idle = self._idle, {}
        for lst in idle.values():
            for fm in lst:
                fm.close()


_featuremap_pool = _FeatureMapPool()


def clear_featuremap_pool():
    """Free the idle device feature maps kept for build_cpu_featuremap (extension)."""
    _featuremap_pool.clear()


def build_cpu_featuremap(scene, params=None, pool=None):
    """matching.cpp:116-130.  The name is the reference's; the build runs on the GPU (queued: the call returns once the
    kernels are launched, whatever reads the feature map next is ordered behind them)."""
    import ctypes as C
    params = params if params is not None else Dt3CpuParameters()
    dev = C.c_int()
    _capi.check(_capi.lib().fdcm_get_device(C.byref(dev)))
    key = (int(params.depth), float(params.dt3_coeff), float(params.padding), int(params.distance), dev.value)
    fm = _featuremap_pool.take(key)
    if fm is None:
        fm = DeviceFeatureMap.build(scene, depth=key[0], coeff=key[1], padding=key[2], distance=key[3])
    else:
        try:
            fm.rebuild(scene)
        except Exception:
            fm.close()
            raise
    out = Dt3Cpu(None, _device=fm)
    out._pool_key = key
    return out


def build_image_featuremap(image, params=None, threshold=60, border=0, low=None, smooth=0, min_pixels=1):
    """The DT3 feature map of a camera frame without a line extractor (extension; include/fdcm.h, "feature maps from
    images"): the seeds are the oriented edge pixels of `image`, a 2-D uint8 numpy array or CUDA torch tensor.  Feature size
    (W + 2 border, H + 2 border), scene translation (border, border); params.padding plays no part.  `threshold` is the high
    threshold; low (hysteresis), smooth (0, 1, 2) and min_pixels (smallest component kept) are per call, like it.  Returns a Dt3Cpu
    that exhaustive_*, score_map, FeatureMap.evaluate and search (with the caller's scene lines) take as any other."""
    import ctypes as C
    params = params if params is not None else Dt3CpuParameters()
    dev = C.c_int()
    _capi.check(_capi.lib().fdcm_get_device(C.byref(dev)))
    key = ("image", int(params.depth), float(params.dt3_coeff), int(params.distance), dev.value)
    fm = _featuremap_pool.take(key)
    if fm is None:
        fm = DeviceFeatureMap.build_image(image, threshold, border=border, depth=key[1], coeff=key[2], distance=key[3], low=low,
                                          smooth=smooth, min_pixels=min_pixels)
    else:
        try:
            fm.rebuild_image(image, threshold, border=border, low=low, smooth=smooth, min_pixels=min_pixels)
        except Exception:
            fm.close()
            raise
    out = Dt3Cpu(None, _device=fm)
    out._pool_key = key
    return out


# ---------------------------------------------------------------- optimise strategies
def _pool_arg(pool, num_threads):
    if isinstance(pool, int) and num_threads is None:
        return ThreadPool(pool)
    if num_threads is not None:
        return ThreadPool(num_threads)
    return pool if pool is not None else ThreadPool()


class DefaultOptimize:
    def __init__(self, pool=None, num_threads=None):
        self._pool = _pool_arg(pool, num_threads)

    def get_pool(self): return self._pool
    def __repr__(self): return "<DefaultOptimize>"


class BatchOptimize:
    def __init__(self, batch_size, pool=None, num_threads=None):
        self._batch_size = int(batch_size)
        self._pool = _pool_arg(pool, num_threads)

    def get_batch_size(self): return self._batch_size
    def get_pool(self): return self._pool
    def __repr__(self): return "<BatchOptimize>"


class IndulgentOptimize:
    """optimizestrategies/indulgentoptimize.h:30-47; runs on the device like the other two optimisers."""

    def __init__(self, indulgent_number_of_passthroughs, pool=None, num_threads=None):
        self._n = int(indulgent_number_of_passthroughs)
        self._pool = _pool_arg(pool, num_threads)

    def get_number_of_passthroughs(self): return self._n
    def get_pool(self): return self._pool
    def __repr__(self): return f"<IndulgentOptimize: number_of_passthroughs={self._n}>"


class OptimizeStrategy:
    def __init__(self, impl):
        self._impl = impl._impl if isinstance(impl, OptimizeStrategy) else impl

    def __repr__(self): return "<OptimizeStrategy>"


# ---------------------------------------------------------------- penalties
class DefaultPenalty:
    def __repr__(self): return "<DefaultPenalty>"


class ExponentialPenalty:
    def __init__(self, tau):
        self._tau = float(_np.float32(tau))

    def get_tau(self): return self._tau
    def __repr__(self): return f"<ExponentialPenalty: tau={self._tau:f}>"


class PenaltyStrategy:
    def __init__(self, impl):
        self._impl = impl._impl if isinstance(impl, PenaltyStrategy) else impl

    def __repr__(self): return "<PenaltyStrategy>"


# ---------------------------------------------------------------- search strategies
class DefaultSearch:
    def __init__(self, max_tmpl_lines, max_scene_lines):
        self._t, self._s = int(max_tmpl_lines), int(max_scene_lines)

    def get_max_tmpl_lines(self): return self._t
    def get_max_scene_lines(self): return self._s

    def __repr__(self):
        return f"<DefaultSearch: max tmpl lines={self._t}, max scene lines={self._s}>"


class ConcentricRangeStrategy:
    """DefaultSearch restricted to the scene lines whose centre lies in an annulus
    (searchstrategies/concentricrange.h:36-84, concentricrange.cpp:29-60)."""

    def __init__(self, max_tmpl_lines, max_scene_lines, center_position, low_boundary, high_boundary):
        self._t, self._s = int(max_tmpl_lines), int(max_scene_lines)
        self._c = _np.asarray(center_position, dtype=_np.float32)
        self._lo, self._hi = float(low_boundary), float(high_boundary)

    def get_max_tmpl_lines(self): return self._t
    def get_max_scene_lines(self): return self._s
    def get_center_position(self): return self._c
    def get_low_radius_boundary(self): return self._lo
    def get_high_radius_boundary(self): return self._hi


class SearchStrategy:
    def __init__(self, impl):
        self._impl = impl._impl if isinstance(impl, SearchStrategy) else impl

    def __repr__(self): return "<SearchStrategy>"


class DefaultMatch:
    def __repr__(self): return "<DefaultMatch>"


class MatchStrategy:
    def __init__(self, impl):
        self._impl = impl._impl if isinstance(impl, MatchStrategy) else impl

    def __repr__(self): return "<MatchStrategy>"


def _unwrap(x, wrapper):
    return x._impl if isinstance(x, wrapper) else x


class _TemplateCache:
    """The DeviceTemplates of the template lists `search` / `get_template_lengths` were last called with.  The
    reference's callers pass the same Python list frame after frame (matching.cpp:279-300 copies it into a std::vector
    on every call); here that would be a device upload per call.  A hit needs the same list object with the same
    line counts and the same bytes: the list is packed (one concatenate, ~0.3 ms for 1000 x 32 lines) and compared with
    what was uploaded, so a template edited in place is seen.  The per-line caps of the exhaustive calls (line_caps) are
    part of the key: a list used without caps and then with them gets two handles.  So is the kind of footprint a list
    carries (with_footprint): the same arrays, plain and wrapped, get two handles.  Four entries are remembered;
    `clear_template_cache()` drops them (each holds its list and a device copy alive)."""
    SLOTS = 4

    def __init__(self):
        self._entries = []  # most recent first: (list object, line counts, packed lines, DeviceTemplates, (caps bytes or None, kind))

    def get(self, templates, line_caps=None):
        if isinstance(templates, DeviceTemplates):
            if line_caps is not None:
                raise ValueError("line_caps with a DeviceTemplates: give the caps to DeviceTemplates(templates, line_caps=...)")
            return templates
        if not isinstance(templates, (list, tuple)):
            templates = list(templates)
        if templates and all(type(t) is _np.ndarray and t.ndim == 2 and t.shape[0] == 4 for t in templates):
            counts = [t.shape[1] for t in templates]
            data = _np.concatenate(templates, axis=1)  # (4, sum N_i), the elements' own dtype
            packed = None
        else:
            packed = _capi.pack_templates(templates)
            counts, data = packed[1].tolist(), packed[0]
        caps = _engine.flat_line_caps(templates, line_caps, counts)
        kind = getattr(templates, "footprint", "box")
        _engine.footprint_kind(kind)
        ckey = (None if caps is None else caps.tobytes(), kind)
        for k, (obj, ecounts, edata, tset, ecaps) in enumerate(self._entries):
            if (obj is templates and tset._h and ecaps == ckey and ecounts == counts and edata.dtype == data.dtype
                    and edata.shape == data.shape and _np.array_equal(edata, data)):
                if k:
                    self._entries.insert(0, self._entries.pop(k))
                return tset
        self._entries = [e for e in self._entries if not (e[0] is templates and e[4] == ckey)]
        if packed is None:
            offsets = _np.zeros(len(counts) + 1, dtype=_np.int64)
            _np.cumsum(counts, out=offsets[1:])
            packed = (_np.ascontiguousarray(data.T, dtype=_np.float32).reshape(-1, 4), offsets)
        tset = DeviceTemplates(templates, _packed=packed, _caps=caps, footprint=kind)
        self._entries.insert(0, (templates, counts, data, tset, ckey))
        del self._entries[self.SLOTS:]
        return tset

    def clear(self):
        self._entries.clear()


_template_cache = _TemplateCache()


class _ShapedTemplates(list):
    """A template list that carries its kind of footprint (with_footprint)."""
    footprint = "box"


def with_footprint(templates, footprint):
    """The template list with a kind of footprint, "box" or "hull" (include/fdcm.h, "Hull footprints"): a list of the same
    arrays that every function taking `templates` accepts.  The detection calls with an `overlap` give the pairs of a "hull"
    list the lattice points of the convex hull of their posed line end points as footprint, in place of the bounding box;
    every other call treats the list as the plain one.  A DeviceTemplates takes the kind as its own keyword."""
    _engine.footprint_kind(footprint)
    if isinstance(templates, DeviceTemplates):
        raise ValueError("with_footprint takes a template list: give the kind to DeviceTemplates(templates, footprint=...)")
    out = _ShapedTemplates(templates)
    out.footprint = footprint
    return out


def clear_template_cache():
    """Forget the template lists uploaded on behalf of search() / get_template_lengths() (extension)."""
    _template_cache.clear()
    _scaled_lists.clear()


def search(matcher, searcher, optimizer, featuremap, templates, scene):
    """matching.cpp:279-289 -> search<DefaultMatch> (defaultmatch.cpp:32-89).  Returns the raw, unsorted matches in
    the reference's positional order as a MatchList (matchlist.py: a list[Match] whose elements are made on access)."""
    matcher = _unwrap(matcher, MatchStrategy)
    searcher = _unwrap(searcher, SearchStrategy)
    optimizer = _unwrap(optimizer, OptimizeStrategy)
    if not isinstance(matcher, DefaultMatch):
        raise TypeError("matcher must be a DefaultMatch")
    scene_for_search = scene
    if isinstance(searcher, ConcentricRangeStrategy):
        # The strategy is DefaultSearch over the filtered scene lines, and search<DefaultMatch> only
        # uses the geometry of the scene line of each combination (defaultmatch.cpp:57-61).
        import ctypes as C
        rec = _capi.as_records(scene)
        if rec.shape[0]:
            idx = _np.zeros(rec.shape[0], dtype=_np.int64)
            n = C.c_int64()
            ctr = _np.ascontiguousarray(searcher.get_center_position(), dtype=_np.float32)
            _capi.check(_capi.lib().fdcm_filter_in_range(_capi.fptr(rec), rec.shape[0], _capi.fptr(ctr),
                                                         searcher.get_low_radius_boundary(),
                                                         searcher.get_high_radius_boundary(),
                                                         idx.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n)))
            scene_for_search = _np.ascontiguousarray(rec[idx[:n.value]].T)
    elif not isinstance(searcher, DefaultSearch):
        raise NotImplementedError("only DefaultSearch and ConcentricRangeStrategy run on the GPU path")
    if isinstance(optimizer, BatchOptimize):
        kind, batch = _capi.BATCH_OPTIMIZE, optimizer.get_batch_size()
    elif isinstance(optimizer, DefaultOptimize):
        kind, batch = _capi.DEFAULT_OPTIMIZE, 1
    elif isinstance(optimizer, IndulgentOptimize):
        kind, batch = _capi.INDULGENT_OPTIMIZE, max(1, optimizer.get_number_of_passthroughs())
    else:
        raise TypeError("optimizer must be DefaultOptimize, BatchOptimize or IndulgentOptimize")
    dt3 = featuremap._dt3 if isinstance(featuremap, FeatureMap) else featuremap
    if not isinstance(dt3, Dt3Cpu):
        raise TypeError("featuremap must be a Dt3Cpu or FeatureMap")
    tset = _template_cache.get(templates)
    rec = search_raw(dt3._fm, tset, scene_for_search, searcher.get_max_tmpl_lines(), searcher.get_max_scene_lines(), kind,
                     batch)
    return MatchList(rec)


def get_template_lengths(templates):
    """core::getTemplateLengths (math.h:319-324)."""
    return _template_cache.get(templates).lengths().tolist()


def penalize(penalty, matches, templatelengths):
    """matching.cpp:291-297; returns a new list (a MatchList; `matches` may be one or any list of Match)."""
    import ctypes as C
    penalty = _unwrap(penalty, PenaltyStrategy)
    if isinstance(penalty, ExponentialPenalty):
        kind, tau = _capi.EXPONENTIAL_PENALTY, penalty.get_tau()
    elif isinstance(penalty, DefaultPenalty):
        kind, tau = _capi.DEFAULT_PENALTY, 1.0
    else:
        raise TypeError("penalty must be DefaultPenalty or ExponentialPenalty")
    rec = records_of(matches)
    lens = _np.ascontiguousarray(templatelengths, dtype=_np.float32)
    rc = _capi.lib().fdcm_penalize(kind, tau, C.c_void_p(rec.ctypes.data), len(rec), _capi.fptr(lens), len(lens))
    if rc == -1 and "templatelengths" in _capi.lib().fdcm_last_error().decode():
        raise IndexError(_capi.lib().fdcm_last_error().decode())  # std::out_of_range -> IndexError
    _capi.check(rc)
    return MatchList(rec)


def sort_matches(matches, max_num_candidates=None):
    """matching.cpp:302-307: ascending score (std::sort, unstable on ties; libstdc++'s order between equal scores).
    max_num_candidates (extension: the C++ overload sortMatches(matches, maxNumCandidates), matchstrategy.h:52-55, which the
    reference's Python module does not bind): std::partial_sort -- only that many best matches are put in order in front."""
    import ctypes as C
    rec = records_of(matches)
    if max_num_candidates is None:
        _capi.check(_capi.lib().fdcm_sort_matches(C.c_void_p(rec.ctypes.data), len(rec)))
    else:
        _capi.check(_capi.lib().fdcm_partial_sort_matches(C.c_void_p(rec.ctypes.data), len(rec), int(max_num_candidates)))
    return MatchList(rec)


# ---------------------------------------------------------------- exhaustive translation search (extension)
def _strides(stride):
    sx, sy = (stride, stride) if _np.ndim(stride) == 0 else tuple(stride)
    return int(sx), int(sy)


def _device_map(featuremap):
    dt3 = featuremap._dt3 if isinstance(featuremap, FeatureMap) else featuremap
    if isinstance(dt3, Dt3Cpu):
        return dt3._fm
    if isinstance(dt3, DeviceFeatureMap):
        return dt3
    raise TypeError("featuremap must be a Dt3Cpu, FeatureMap or DeviceFeatureMap")


def exhaustive_window(featuremap, templates, stride=1):
    """The default window of exhaustive_search / score_map: the smallest grid with the given stride (an int or (sx, sy)),
    origin a multiple of it, that holds every admissible integer translation of every template with lines.  Returns
    (x0, y0, nx, ny, sx, sy); nx = ny = 0 when no template fits anywhere."""
    sx, sy = _strides(stride)
    return _device_map(featuremap).exhaustive_window(_template_cache.get(templates), sx, sy).as_tuple()


def _window(fm, tset, stride, window):
    if window is not None:
        return tuple(int(v) for v in window)
    sx, sy = _strides(stride)
    return fm.exhaustive_window(tset, sx, sy).as_tuple()


def exhaustive_search(featuremap, templates, stride=1, k=1, window=None, line_caps=None):
    """Score every template at every translation of a grid and keep the k best of each (1 <= k <= 64), ordered by
    (score, grid index); templates without lines give nothing.  window: (x0, y0, nx, ny, sx, sy), by default
    exhaustive_window(featuremap, templates, stride).  Returns a MatchList whose transforms are the pure translations
    [[1, 0, tx], [0, 1, ty]], ready for penalize / sort_matches.  line_caps: None, a scalar tau or one float array per
    template: every line's cost is clamped to its cap (line_caps(templates, tau) states the scalar's caps)."""
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates, line_caps)
    g = _window(fm, tset, stride, window)
    if g[2] == 0 or g[3] == 0:
        return MatchList(_np.zeros(0, dtype=_capi.MATCH_DTYPE))
    return MatchList(fm.exhaustive_search(tset, g, k=k))


def exhaustive_peaks(featuremap, templates, radius, stride=1, k=1, window=None, line_caps=None):
    """exhaustive_search for detection: per template its k best peaks of the score map, ordered by (score, grid index).  A
    peak is an admissible grid point whose (score, grid index) is the smallest within radius = r or (rx, ry) grid steps
    (0 <= rx, ry <= 32) on either axis, so two peaks of one template are never that close; radius 0 is exhaustive_search.
    Returns a MatchList of pure translations, ready for penalize / sort_matches.  line_caps: exhaustive_search's."""
    rx, ry = _strides(radius)
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates, line_caps)
    g = _window(fm, tset, stride, window)
    if g[2] == 0 or g[3] == 0:
        return MatchList(_np.zeros(0, dtype=_capi.MATCH_DTYPE))
    return MatchList(fm.exhaustive_peaks(tset, g, k=k, rx=rx, ry=ry))


def score_map(featuremap, templates, stride=1, window=None, line_caps=None):
    """The dense chamfer score map: (float32 array [T, ny, nx] of the scores, NaN where a translation puts the template
    outside the feature map; grid (x0, y0, nx, ny, sx, sy)).  Point (i, j) is the translation (x0 + i sx, y0 + j sy).
    line_caps: exhaustive_search's."""
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates, line_caps)
    g = _window(fm, tset, stride, window)
    if g[2] == 0 or g[3] == 0:
        return _np.zeros((tset.count, g[3], g[2]), dtype=_np.float32), g
    return fm.score_map(tset, g), g



# ---------------------------------------------------------------- exhaustive search over rotations (extension)
def _angles(angles):
    """(n, 2) float32 (c, s) of angles in radians: float32(cos(float64)), float32(sin(float64))."""
    a = _np.asarray(angles, dtype=_np.float64).reshape(-1)
    return _np.stack([_np.cos(a), _np.sin(a)], axis=1).astype(_np.float32)


def _pivots(templates, pivot, T):
    """pivot "center": per template the centre of its end points' bounding box in float32 ((0, 0) without lines); None:
    the origin; a (T, 2) array as it is."""
    if pivot is None:
        return None
    if isinstance(pivot, str):
        if pivot != "center":
            raise ValueError('pivot must be "center", None or a (T, 2) array')
        out = _np.zeros((T, 2), dtype=_np.float32)
        for t, tm in enumerate(templates):
            a = _np.asarray(tm, dtype=_np.float32).reshape(4, -1)
            if a.shape[1] == 0:
                continue
            xs, ys = _np.concatenate([a[0], a[2]]), _np.concatenate([a[1], a[3]])
            out[t, 0] = (xs.min() + xs.max()) / _np.float32(2)
            out[t, 1] = (ys.min() + ys.max()) / _np.float32(2)
        return out
    pv = _np.ascontiguousarray(pivot, dtype=_np.float32)
    if pv.shape != (T, 2):
        raise ValueError("pivot array must be (T, 2)")
    return pv


def _rotation_args(featuremap, templates, angles, pivot, line_caps=None):
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates, line_caps)
    return fm, tset, _angles(angles), _pivots(templates, pivot, tset.count)


def _rotation_window(fm, tset, cs, pv, stride, window):
    if window is not None:
        return tuple(int(v) for v in window)
    sx, sy = _strides(stride)
    return fm.exhaustive_rotations_window(tset, cs, pv, sx, sy).as_tuple()


def rotation_window(featuremap, templates, angles, stride=1, pivot="center"):
    """The default window of exhaustive_rotation_search / rotation_score_map: the smallest grid with the given stride,
    origin a multiple of it, that holds every admissible integer translation of every template with lines under every
    rotation.  Returns (x0, y0, nx, ny, sx, sy); nx = ny = 0 when none fits anywhere."""
    fm, tset, cs, pv = _rotation_args(featuremap, templates, angles, pivot)
    sx, sy = _strides(stride)
    return fm.exhaustive_rotations_window(tset, cs, pv, sx, sy).as_tuple()


def exhaustive_rotation_search(featuremap, templates, angles, stride=1, k=1, radius=0, angle_radius=0, wrap=False,
                               pivot="center", window=None, line_caps=None):
    """exhaustive_peaks over rotations: every template rotated by every angle (radians) about its pivot ("center": its
    bounding box centre, None: the origin, or a (T, 2) array) and scored at every translation of the grid.  Per template
    its k best peaks over (angle, x, y), ordered by (score, angle index, grid index); a peak is the smallest within
    radius = r or (rx, ry) grid steps and angle_radius angle steps (0 to 32 each), circular over the angle list with
    wrap.  Radii 0 give the top-k over all poses.  Returns a MatchList whose transforms are [R | m + t], ready for
    penalize / sort_matches.  line_caps: exhaustive_search's; a line keeps its cap under every rotation."""
    rx, ry = _strides(radius)
    fm, tset, cs, pv = _rotation_args(featuremap, templates, angles, pivot, line_caps)
    g = _rotation_window(fm, tset, cs, pv, stride, window)
    if g[2] == 0 or g[3] == 0:
        return MatchList(_np.zeros(0, dtype=_capi.MATCH_DTYPE))
    return MatchList(fm.exhaustive_rotation_search(tset, g, cs, pv, k=k, rx=rx, ry=ry, ra=int(angle_radius), wrap=wrap))


def rotation_score_map(featuremap, templates, angles, stride=1, pivot="center", window=None, line_caps=None):
    """The dense score maps of the rotated templates: (float32 array [T, A, ny, nx], NaN where not admissible; grid).
    line_caps: exhaustive_search's."""
    fm, tset, cs, pv = _rotation_args(featuremap, templates, angles, pivot, line_caps)
    g = _rotation_window(fm, tset, cs, pv, stride, window)
    if g[2] == 0 or g[3] == 0:
        return _np.zeros((tset.count, cs.shape[0], g[3], g[2]), dtype=_np.float32), g
    return fm.rotation_score_map(tset, g, cs, pv), g


# ---------------------------------------------------------------- best template per point and detections (extension)
def _penalty_args(penalty):
    penalty = _unwrap(penalty, PenaltyStrategy)
    if penalty is None:
        return None, 1.0
    if isinstance(penalty, ExponentialPenalty):
        return _capi.EXPONENTIAL_PENALTY, penalty.get_tau()
    if isinstance(penalty, DefaultPenalty):
        return _capi.DEFAULT_PENALTY, 1.0
    raise TypeError("penalty must be None, DefaultPenalty or ExponentialPenalty")


def _detect_args(featuremap, templates, angles, pivot, stride, window, line_caps=None):
    """(device map, template set, cs, pivots, grid): angles None is the translations alone, on exhaustive_window."""
    if angles is None:
        fm, tset = _device_map(featuremap), _template_cache.get(templates, line_caps)
        return fm, tset, None, None, _window(fm, tset, stride, window)
    fm, tset, cs, pv = _rotation_args(featuremap, templates, angles, pivot, line_caps)
    return fm, tset, cs, pv, _rotation_window(fm, tset, cs, pv, stride, window)


def best_score_map(featuremap, templates, stride=1, penalty=None, angles=None, pivot="center", window=None, line_caps=None,
                   min_matched=None, return_matched=False):
    """The templates compared with each other: per grid point the lowest score over all templates with lines and all
    angles, each score divided as penalize(penalty, ...) divides it (None: as it is), and which pair gave it.  Returns
    (scores [ny, nx] float32, NaN where no template fits; pairs [ny, nx] int32, -1 there; grid).  With n = len(angles)
    (1 without angles) pairs // n is the template and pairs % n the angle; equal scores go to the lowest template, then
    the lowest angle.  angles, pivot, window and line_caps are exhaustive_rotation_search's; with caps tau len_i and
    DefaultPenalty the scores lie in [0, tau] up to rounding.  min_matched (0 to 1) or return_matched: the gated best map,
    the plane exhaustive_detect_all(gate="all") works on: only the pairs whose lines that cost at most their caps at the
    point make up at least min_matched of the template's line length compete for it, and a point where none does has NaN
    and -1.  With return_matched the result is (scores, pairs, matched, grid), matched [ny, nx] float32 the winning pair's
    share, NaN where there is none."""
    kind, tau = _penalty_args(penalty)
    fm, tset, cs, pv, g = _detect_args(featuremap, templates, angles, pivot, stride, window, line_caps)
    if g[2] == 0 or g[3] == 0:
        empty = (_np.zeros((g[3], g[2]), dtype=_np.float32), _np.zeros((g[3], g[2]), dtype=_np.int32))
        return empty + ((_np.zeros((g[3], g[2]), dtype=_np.float32),) if return_matched else ()) + (g,)
    if min_matched is None and not return_matched:
        scores, pairs = fm.best_map(tset, g, cs, pv, penalty=kind, tau=tau)
        return scores, pairs, g
    return fm.best_map(tset, g, cs, pv, penalty=kind, tau=tau, min_matched=min_matched, matched=return_matched) + (g,)


def exhaustive_detect(featuremap, templates, radius, stride=1, k=8, penalty=None, angles=None, pivot="center", window=None,
                      line_caps=None):
    """The dense search as a detector: the k best peaks (1 <= k <= 64) of best_score_map's score plane, a peak being a
    grid point whose (score, grid index) is the smallest within radius = r or (rx, ry) grid steps (0 to 32), whichever
    template and angle won each point.  One object in the scene gives one detection, not one per template.  Returns a
    MatchList of the winning templates' poses with the normalised scores, already in ascending score: neither penalize
    nor sort_matches is needed.  line_caps (exhaustive_search's) keeps one occluded line from costing a correct view the
    point; line_costs tells which lines of a detection matched."""
    rx, ry = _strides(radius)
    kind, tau = _penalty_args(penalty)
    fm, tset, cs, pv, g = _detect_args(featuremap, templates, angles, pivot, stride, window, line_caps)
    if g[2] == 0 or g[3] == 0:
        return MatchList(_np.zeros(0, dtype=_capi.MATCH_DTYPE))
    return MatchList(fm.exhaustive_detect(tset, g, cs, pv, k=k, rx=rx, ry=ry, penalty=kind, tau=tau))


def exhaustive_detect_nms(featuremap, templates, overlap=0.3, stride=1, k=8, penalty=None, angles=None, pivot="center", window=None,
                          line_caps=None, margin=0, return_boxes=False):
    """exhaustive_detect with greedy suppression by footprint overlap in place of the radius: the best point of
    best_score_map's plane is a detection, every point whose footprint overlaps the detection's by more than `overlap`
    (intersection over union, 0 to 1, taken in thousandths) is dropped, and so on up to k detections (1 <= k <= 64).  The
    footprint of a point is the bounding box of the winning template's (rotated) line end points, widened by margin pixels
    (0 to 4096), at the point's translation: parts of different sizes lying against each other each keep their
    detections, and one large part is reported once.  overlap=1 suppresses nothing and equals exhaustive_detect(radius=0).
    Returns a MatchList in ascending score, and with return_boxes also the (n, 4) int32 footprints x0, y0, x1, y1 (ends
    inclusive, in the translations' coordinates).  The other arguments are exhaustive_detect's."""
    kind, tau = _penalty_args(penalty)
    permille = int(round(1000 * float(overlap)))
    fm, tset, cs, pv, g = _detect_args(featuremap, templates, angles, pivot, stride, window, line_caps)
    if g[2] == 0 or g[3] == 0:
        empty = MatchList(_np.zeros(0, dtype=_capi.MATCH_DTYPE))
        return (empty, _np.zeros((0, 4), dtype=_np.int32)) if return_boxes else empty
    res = fm.exhaustive_detect_nms(tset, g, cs, pv, k=k, overlap_permille=permille, margin=margin, penalty=kind, tau=tau,
                                   boxes=return_boxes)
    return (MatchList(res[0]), res[1]) if return_boxes else MatchList(res)


def exhaustive_detect_all(featuremap, templates, max_score, overlap=0.3, stride=1, max_detections=1024, penalty=None, angles=None,
                          pivot="center", window=None, line_caps=None, margin=0, return_boxes=False, min_matched=None,
                          return_matched=False, gate="winner"):
    """Every detection that matches at least as well as max_score: exhaustive_detect_nms' greedy rule on the points of
    best_score_map's plane whose score is <= max_score (>= 0 or inf), until they run out or max_detections (1 to 4096) is
    reached.  A scene with two parts gives two detections, not k records of which six are junk, and a bin of 200 small
    parts gives 200.  max_score=inf with max_detections=k is exhaustive_detect_nms(k=k); a lower max_score returns the
    leading part of that list, and costs less: a template is dropped for a patch of points as soon as its partial sums put
    all of them over the threshold.  Returns a MatchList in ascending score, and with return_boxes also the (n, 4) int32
    footprints.  min_matched (0 to 1): a point is dropped, before the greedy rule, unless the lines of its winning template
    that cost at most their caps there make up at least that share of the template's line length; a junk point then never
    suppresses a good neighbour.  Only the winning pair of a point is looked at.  return_matched: that share of every
    detection as an (n,) float32 array, last in the returned tuple: (dets, matched) or (dets, boxes, matched).  gate="all"
    puts min_matched inside the minimum instead: the pairs that fail it at a point do not compete for the point, so a wrong
    view that wins a point on a few perfectly matched lines no longer deletes the right view under it (README, "Gate inside
    the minimum").  The other arguments are exhaustive_detect_nms'."""
    _engine.gate_kind(gate)
    kind, tau = _penalty_args(penalty)
    permille = int(round(1000 * float(overlap)))
    fm, tset, cs, pv, g = _detect_args(featuremap, templates, angles, pivot, stride, window, line_caps)
    if g[2] == 0 or g[3] == 0:
        res = (MatchList(_np.zeros(0, dtype=_capi.MATCH_DTYPE)),) + ((_np.zeros((0, 4), dtype=_np.int32),) if return_boxes else ())
        res += (_np.zeros(0, dtype=_np.float32),) if return_matched else ()
        return res if len(res) > 1 else res[0]
    res = fm.exhaustive_detect_all(tset, g, cs, pv, max_score=max_score, max_detections=max_detections, overlap_permille=permille,
                                   margin=margin, penalty=kind, tau=tau, boxes=return_boxes, min_matched=min_matched,
                                   matched=return_matched, gate=gate)
    return (MatchList(res[0]),) + tuple(res[1:]) if return_boxes or return_matched else MatchList(res)


def detect_score_bounds(templates, penalty, max_score):
    """Per template the largest float32 score sum whose normalised score (penalty: None, DefaultPenalty or
    ExponentialPenalty) is <= max_score: what exhaustive_detect_all's threshold means for each template's raw score.  0 for
    a template without lines.  No device work."""
    kind, tau = _penalty_args(penalty)
    return _template_cache.get(templates).score_bounds(max_score, penalty=kind, tau=tau)


def template_footprint_spans(templates, angles=None, pivot="center", margin=0):
    """The hull shapes of every template and angle (include/fdcm.h, "Hull footprints"), without a device: (row_offsets, spans,
    areas).  Pair u = t A + a (A = 1 without angles) has the rows row_offsets[u] .. row_offsets[u + 1] of the (R, 2) int32
    spans, row r at y = y0 of template_footprints(..)[t, a] + (r - row_offsets[u]), holding the pixels xl .. xr in the frame
    of that box, (0, -1) when empty; areas[u] is its pixel count."""
    from .engine import lines_footprint_spans
    if angles is None:
        return lines_footprint_spans(templates, margin=margin)
    return lines_footprint_spans(templates, _angles(angles), _pivots(templates, pivot, len(templates)), margin=margin)


def template_footprints(templates, angles=None, pivot="center", margin=0):
    """The (T, A, 4) int32 footprints x0, y0, x1, y1 exhaustive_detect_nms uses for every template and angle (A = 1 without
    angles: the lines as they are); (0, 0, -1, -1) for a template without lines.  No device work."""
    from .engine import lines_footprints
    if angles is None:
        return lines_footprints(templates, margin=margin)
    return lines_footprints(templates, _angles(angles), _pivots(templates, pivot, len(templates)), margin=margin)


# ---------------------------------------------------------------- pose windows: refinement and tracking (extension)
def template_pivots(templates, pivot="center"):
    """The (T, 2) float32 pivots the rotation searches use for pivot="center" (each template's bounding box centre), an
    explicit (T, 2) array as it is, or None for the origin: what pose_windows needs to read a record's translation."""
    return _pivots(templates, pivot, len(templates))


def exhaustive_window_search(featuremap, templates, jobs, angles=None, stride=1, k=1, pivot="center", wrap=False,
                             tmpl_index_base=0, line_caps=None):
    """A list of small exhaustive searches in one call: coarse-to-fine refinement and tracking.  jobs is an (n, 7) int32
    array of rows (tmpl, a0, na, x0, y0, nx, ny): template tmpl, the run of angles a0 .. a0 + na - 1 of `angles` (mod
    len(angles) with wrap) and the translations (x0 + i sx, y0 + j sy), 0 <= i < nx, 0 <= j < ny, with na nx ny <= 65536.
    Per job, in the order given, its k best poses (1 <= k <= 64) by (score, position in the run, grid index): exactly what
    exhaustive_rotation_search(radius=0, angle_radius=0) returns for that template, those angles and that window alone.
    angles and pivot are exhaustive_rotation_search's; angles=None searches translations only (a0 = 0, na = 1) and returns
    exhaustive_search's pure translations.  line_caps: exhaustive_search's.  Returns (MatchList, offsets): job j's matches
    are offsets[j] .. offsets[j + 1]."""
    sx, sy = _strides(stride)
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates, line_caps)
    cs = pv = None
    if angles is not None:
        cs, pv = _angles(angles), _pivots(templates, pivot, tset.count)
    rec, offsets = fm.exhaustive_window_search(tset, jobs, cs, pv, sx=sx, sy=sy, wrap=wrap, k=k, tmpl_index_base=tmpl_index_base)
    return MatchList(rec), offsets


def pose_windows(records, coarse_angles, fine_angles, pivots, half_angles, half_x, half_y, stride=1, wrap=False):
    """Jobs for exhaustive_window_search around detections: pure numpy.  records: the matches of
    exhaustive_rotation_search over coarse_angles (a MatchList or its record array, tmpl_idx without a base); pivots: the
    (T, 2) pivots of that search (template_pivots) or None for the origin.  Per record, one row (tmpl, a0, na, x0, y0, nx,
    ny) on the table fine_angles:
      - the coarse angle is the index whose (float32(cos), float32(sin)) equal (transform[0], transform[3]) exactly;
      - the translation is t = rint(float64(transform[2]) - float64(m.x)), likewise y, m the record's float32 offset
        p - R p.  transform[2] is float32(m.x + t.x): the difference is t within half a float32 ulp of transform[2], so
        the result is exact while |transform[2]|, |transform[5]| < 2^22 -- any pose on a map of 4096 x 4096 and beyond;
      - the centre of the run is the fine angle nearest the coarse one on the circle (the lowest index on a tie), the run
        centre - half_angles .. centre + half_angles, cut at 0 and len(fine_angles) - 1, or circular with wrap (a0 taken
        mod the table, at most the whole table);
      - the window holds the multiples of stride (an int or (sx, sy)) from the last one <= t - half to the first one
        >= t + half on each axis: 2 half + 1 points around t at stride 1."""
    rec = records.records() if isinstance(records, MatchList) else _np.asarray(records)
    sx, sy = _strides(stride)
    coarse, fine = _angles(coarse_angles), _np.asarray(fine_angles, dtype=_np.float64).reshape(-1)
    ca = _np.asarray(coarse_angles, dtype=_np.float64).reshape(-1)
    n, ha = fine.shape[0], int(half_angles)
    if n < 1 or ha < 0 or int(half_x) < 0 or int(half_y) < 0 or sx < 1 or sy < 1:
        raise ValueError("pose_windows: an empty fine table, a negative half width or a stride below 1")
    jobs = _np.zeros((rec.shape[0], 7), dtype=_np.int32)
    two_pi = 2 * _np.pi
    pv = None if pivots is None else _np.asarray(pivots, dtype=_np.float32)
    for q in range(rec.shape[0]):
        tr, t = rec["transform"][q], int(rec["tmpl_idx"][q])
        hit = _np.nonzero((coarse[:, 0] == tr[0]) & (coarse[:, 1] == tr[3]))[0]
        if hit.size == 0:
            raise ValueError(f"pose_windows: record {q} has a rotation that is none of coarse_angles")
        c, s = coarse[hit[0]]
        px, py = (_np.float32(0), _np.float32(0)) if pv is None else pv[t]
        ns = -s
        mx, my = px - (c * px + ns * py), py - (s * px + c * py)  # float32, left to right: the library's M_a
        tx = int(_np.rint(_np.float64(tr[2]) - _np.float64(mx)))
        ty = int(_np.rint(_np.float64(tr[5]) - _np.float64(my)))
        d = _np.abs((fine - ca[hit[0]] + _np.pi) % two_pi - _np.pi)
        centre = int(_np.argmin(d))
        if wrap:
            a0, na = (centre - ha) % n, min(2 * ha + 1, n)
        else:
            a0 = max(0, centre - ha)
            na = min(n - 1, centre + ha) - a0 + 1
        x0, y0 = (tx - int(half_x)) // sx * sx, (ty - int(half_y)) // sy * sy
        nx, ny = -((x0 - tx - int(half_x)) // sx) + 1, -((y0 - ty - int(half_y)) // sy) + 1
        jobs[q] = (t, a0, na, x0, y0, nx, ny)
    return jobs


def exhaustive_detect_windows(featuremap, templates, jobs, max_score, overlap=0.3, angles=None, stride=1, max_detections=1024,
                              penalty=None, pivot="center", wrap=False, line_caps=None, margin=0, min_matched=None,
                              return_boxes=False, return_matched=False, return_jobs=False, gate="winner"):
    """exhaustive_detect_all over a job list in place of a dense grid: coarse-to-fine detection and tracking in one call.
    jobs are exhaustive_window_search's (n, 7) rows (tmpl, a0, na, x0, y0, nx, ny).  Each job gives its best pose, exactly
    its record of exhaustive_window_search(k=1); the score is divided as penalize(penalty, ...) divides it; a job stays when
    that score is <= max_score (>= 0 or inf) and, with min_matched (0 to 1), when the lines of its best pose that cost at
    most their caps make up at least that share of the template's line length (only the best pose of a job is looked at).
    The jobs left go through exhaustive_detect_nms' greedy rule in the order (score, job index): a job's footprint is its
    template's box under its best pose's angle, widened by margin, at its best pose's translation, and a detection drops
    every job whose footprint overlaps its own by more than `overlap`; at most max_detections (1 to 4096).  Several jobs
    around one object (neighbouring views in a tracker, overlapping boxes of coarse seeds, duplicates) end up as one
    detection.  Returns a MatchList in ascending score, then with return_boxes the (n, 4) int32 footprints, with
    return_matched the (n,) float32 matched fractions (matched_fractions of each detection's pose) and with return_jobs the
    (n,) int32 index of the job each detection came from, in that order.  gate="all": a job's best pose is the best among
    its poses that pass min_matched, so a job whose overall best pose fails still gives the pose next to it that passes.
    angles, pivot, wrap, stride and line_caps are exhaustive_window_search's."""
    _engine.gate_kind(gate)
    kind, tau = _penalty_args(penalty)
    permille = int(round(1000 * float(overlap)))
    sx, sy = _strides(stride)
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates, line_caps)
    cs = pv = None
    if angles is not None:
        cs, pv = _angles(angles), _pivots(templates, pivot, tset.count)
    res = fm.exhaustive_detect_windows(tset, jobs, cs, pv, sx=sx, sy=sy, wrap=wrap, max_score=max_score, max_detections=max_detections,
                                       overlap_permille=permille, margin=margin, penalty=kind, tau=tau, min_matched=min_matched,
                                       boxes=return_boxes, matched=return_matched, job_index=return_jobs, gate=gate)
    return (MatchList(res[0]),) + tuple(res[1:]) if isinstance(res, tuple) else MatchList(res)


def exhaustive_detect_refined(featuremap, templates, max_score, coarse_angles, fine_angles, coarse_stride, half_angles, half_x, half_y,
                              coarse_max_score=None, coarse_overlap=1.0, coarse_max_detections=1024, overlap=0.3, stride=1,
                              max_detections=1024, penalty=None, pivot="center", wrap=False, line_caps=None, margin=0,
                              min_matched=None, return_boxes=False, return_matched=False, return_jobs=False, gate="winner"):
    """Every part in the frame to the fine table's angle step and `stride` pixels, without the dense fine search: pure
    Python over three calls, and by definition exactly their composition:
      seeds = exhaustive_detect_all(featuremap, templates, coarse_max_score (None: inf), overlap=coarse_overlap,
                                    stride=coarse_stride, max_detections=coarse_max_detections, penalty=penalty,
                                    angles=coarse_angles, pivot=pivot, line_caps=line_caps, margin=margin)
      jobs = pose_windows(seeds, coarse_angles, fine_angles, template_pivots(templates, pivot), half_angles, half_x, half_y,
                          stride=stride, wrap=wrap)
      exhaustive_detect_windows(featuremap, templates, jobs, max_score, overlap=overlap, angles=fine_angles, stride=stride,
                                max_detections=max_detections, penalty=penalty, pivot=pivot, wrap=wrap, line_caps=line_caps,
                                margin=margin, min_matched=min_matched, return_boxes=.., return_matched=.., return_jobs=..,
                                gate=gate)
    The coarse stage has no matched-fraction gate (a pose a few degrees off matches few lines) and by default neither a
    threshold nor suppression: its coarse_max_detections best grid points are the seeds, and the fine stage's rule reduces the
    refined seeds of one object to one detection.  return_jobs indexes the seeds.  gate applies to the fine stage only."""
    _engine.gate_kind(gate)
    seeds = exhaustive_detect_all(featuremap, templates, float("inf") if coarse_max_score is None else coarse_max_score,
                                  overlap=coarse_overlap, stride=coarse_stride, max_detections=coarse_max_detections, penalty=penalty,
                                  angles=coarse_angles, pivot=pivot, line_caps=line_caps, margin=margin)
    jobs = pose_windows(seeds, coarse_angles, fine_angles, template_pivots(templates, pivot), half_angles, half_x, half_y,
                        stride=stride, wrap=wrap)
    return exhaustive_detect_windows(featuremap, templates, jobs, max_score, overlap=overlap, angles=fine_angles, stride=stride,
                                     max_detections=max_detections, penalty=penalty, pivot=pivot, wrap=wrap, line_caps=line_caps,
                                     margin=margin, min_matched=min_matched, return_boxes=return_boxes,
                                     return_matched=return_matched, return_jobs=return_jobs, gate=gate)


# ---------------------------------------------------------------- image pyramid: coarse-to-fine over levels (extension)
def build_image_featuremap_level(image, level, params=None, threshold=60, border=0, low=None, smooth=0, min_pixels=1):
    """build_image_featuremap of level `level` (0 to 12) of `image` (include/fdcm.h, "image pyramid"): by definition the feature
    map of image_pyramid(image, level) with the same options, the levels made on the device in a workspace of the handle.
    border is in the level's pixels: feature size (W_l + 2 border, H_l + 2 border), scene translation (border, border)."""
    import ctypes as C
    params = params if params is not None else Dt3CpuParameters()
    dev = C.c_int()
    _capi.check(_capi.lib().fdcm_get_device(C.byref(dev)))
    key = ("image", int(params.depth), float(params.dt3_coeff), int(params.distance), dev.value, "level", int(level))
    fm = _featuremap_pool.take(key)
    if fm is None:
        fm = DeviceFeatureMap.build_image_level(image, level, threshold, border=border, depth=key[1], coeff=key[2], distance=key[3],
                                                low=low, smooth=smooth, min_pixels=min_pixels)
    else:
        try:
            fm.rebuild_image_level(image, level, threshold, border=border, low=low, smooth=smooth, min_pixels=min_pixels)
        except Exception:
            fm.close()
            raise
    out = Dt3Cpu(None, _device=fm)
    out._pool_key = key
    return out


def _level_factor(level, sign):
    level = int(level)
    if not 0 <= level <= 12:
        raise ValueError("level must be in [0, 12]")
    return _np.float32(2.0 ** (sign * level))


def scaled_templates(templates, level):
    """The template list of pyramid level `level`: the same list with every coordinate multiplied by float32(2^-level), which
    is exact.  A list from with_footprint keeps its kind.  Searched on the level's feature map, its records lift to the
    level-0 records of the unscaled list (lift_records)."""
    if isinstance(templates, DeviceTemplates):
        raise ValueError("scaled_templates takes a template list, not a DeviceTemplates")
    f = _level_factor(level, -1)
    out = [_np.asarray(t, dtype=_np.float32) * f for t in templates]
    kind = getattr(templates, "footprint", None)
    return out if kind is None else with_footprint(out, kind)


def lift_records(records, level):
    """A copy of the records of a search on pyramid level `level` (a MatchList or its record array) as level-0 records:
    transform[2] and transform[5] multiplied by float32(2^level), everything else unchanged.  For a search of
    scaled_templates(templates, level) with pivots scaled alike, the result is bit for bit what a level-0 search of
    `templates` emits for the translation 2^level t and the same angle (include/fdcm.h, "image pyramid")."""
    f = _level_factor(level, 1)
    rec = records_of(records)
    rec["transform"][:, 2] *= f
    rec["transform"][:, 5] *= f
    return MatchList(rec) if isinstance(records, MatchList) else rec


_scaled_lists = []  # most recent first: (list object, level, its scaled list), so that a list searched again finds its upload


def _scaled_cached(templates, level):
    """scaled_templates(templates, level), as the list object an earlier call made when it holds the same bytes: the template
    cache goes by the list object, and a fresh list per call would be a device upload per call."""
    small = scaled_templates(templates, level)
    for k, (obj, lvl, cached) in enumerate(_scaled_lists):
        if (obj is templates and lvl == int(level) and len(cached) == len(small)
                and getattr(cached, "footprint", None) == getattr(small, "footprint", None)
                and all(a.shape == b.shape and _np.array_equal(a.view(_np.uint32), b.view(_np.uint32)) for a, b in zip(cached, small))):
            if k:
                _scaled_lists.insert(0, _scaled_lists.pop(k))
            return cached
    _scaled_lists[:] = [e for e in _scaled_lists if not (e[0] is templates and e[1] == int(level))]
    _scaled_lists.insert(0, (templates, int(level), small))
    del _scaled_lists[_TemplateCache.SLOTS:]
    return small


def _pyramid_coarse_args(templates, level, pivot, half_x, half_y, coarse_max_score, coarse_margin, margin):
    small = _scaled_cached(templates, level)
    pv = template_pivots(templates, pivot)
    pv_small = None if pv is None else pv * _level_factor(level, -1)
    hx = 2 ** int(level) if half_x is None else half_x
    hy = 2 ** int(level) if half_y is None else half_y
    cms = float("inf") if coarse_max_score is None else coarse_max_score
    cm = -(-int(margin) >> int(level)) if coarse_margin is None else coarse_margin
    return small, pv, pv_small, hx, hy, cms, cm


def exhaustive_detect_pyramid(featuremap, level_featuremap, level, templates, max_score, coarse_angles, fine_angles, half_angles,
                              half_x=None, half_y=None, coarse_stride=1, coarse_max_score=None, coarse_overlap=1.0,
                              coarse_max_detections=1024, coarse_line_caps=None, coarse_margin=None, overlap=0.3, stride=1,
                              max_detections=1024, penalty=None, pivot="center", wrap=False, line_caps=None, margin=0,
                              min_matched=None, return_boxes=False, return_matched=False, return_jobs=False, gate="winner"):
    """exhaustive_detect_refined with its coarse pass on a pyramid level: level_featuremap is the map of the frame reduced by
    2^level (build_image_featuremap_level, or build_cpu_featuremap(scene * 2^-level) for a scene given as lines), featuremap the
    full-resolution one.  Pure Python, and by definition exactly this composition:
      small = scaled_templates(templates, level)
      pv = template_pivots(templates, pivot)                     # None stays None; small's pivots are pv * 2^-level, exact
      seeds_L = exhaustive_detect_all(level_featuremap, small, coarse_max_score (None: inf), overlap=coarse_overlap,
                                      stride=coarse_stride, max_detections=coarse_max_detections, penalty=penalty,
                                      angles=coarse_angles, pivot=None if pv is None else pv * 2^-level,
                                      line_caps=coarse_line_caps, margin=coarse_margin (None: -(-margin >> level)))
      seeds = lift_records(seeds_L, level)
      jobs = pose_windows(seeds, coarse_angles, fine_angles, pv, half_angles, half_x (None: 2^level), half_y (None: 2^level),
                          stride=stride, wrap=wrap)
      exhaustive_detect_windows(featuremap, templates, jobs, max_score, overlap=overlap, angles=fine_angles, stride=stride,
                                max_detections=max_detections, penalty=penalty, pivot=pivot, wrap=wrap, line_caps=line_caps,
                                margin=margin, min_matched=min_matched, return_boxes=.., return_matched=.., return_jobs=..,
                                gate=gate)
    The coarse pass runs at stride 1 on a map with 4^-level of the pixels, so neighbouring lanes read neighbouring pixels again.
    A lifted seed is bit for bit the level-0 record of the translation 2^level t, so pose_windows reads it by its own rule; the
    default half widths cover the 2^level pixels a level pixel stands for.  Scores do not carry over between levels: the coarse
    stage has its own threshold, caps and margin.  return_jobs indexes the seeds."""
    _engine.gate_kind(gate)
    small, pv, pv_small, hx, hy, cms, cm = _pyramid_coarse_args(templates, level, pivot, half_x, half_y, coarse_max_score,
                                                                coarse_margin, margin)
    seeds_l = exhaustive_detect_all(level_featuremap, small, cms, overlap=coarse_overlap, stride=coarse_stride,
                                    max_detections=coarse_max_detections, penalty=penalty, angles=coarse_angles, pivot=pv_small,
                                    line_caps=coarse_line_caps, margin=cm)
    jobs = pose_windows(lift_records(seeds_l, level), coarse_angles, fine_angles, pv, half_angles, hx, hy, stride=stride, wrap=wrap)
    return exhaustive_detect_windows(featuremap, templates, jobs, max_score, overlap=overlap, angles=fine_angles, stride=stride,
                                     max_detections=max_detections, penalty=penalty, pivot=pivot, wrap=wrap, line_caps=line_caps,
                                     margin=margin, min_matched=min_matched, return_boxes=return_boxes,
                                     return_matched=return_matched, return_jobs=return_jobs, gate=gate)


def exhaustive_detect_pyramid_objects(featuremap, level_featuremap, level, templates, objects, max_score, coarse_angles, fine_angles,
                                      half_angles, half_x=None, half_y=None, coarse_stride=1, coarse_max_score=None,
                                      coarse_overlap=1.0, coarse_cross_overlap=None, coarse_max_detections=1024,
                                      coarse_line_caps=None, coarse_margin=None, overlap=0.3, cross_overlap=None, stride=1,
                                      max_detections=1024, penalty=None, pivot="center", wrap=False, line_caps=None, margin=0,
                                      min_matched=None, return_boxes=False, return_matched=False, return_jobs=False,
                                      n_objects=None, return_objects=False, gate="winner"):
    """exhaustive_detect_pyramid with objects: the same composition over exhaustive_detect_objects (on level_featuremap, with
    cross_overlap=coarse_cross_overlap and n_objects) and exhaustive_detect_windows_objects, with the keywords of
    exhaustive_detect_refined_objects."""
    _engine.gate_kind(gate)
    small, pv, pv_small, hx, hy, cms, cm = _pyramid_coarse_args(templates, level, pivot, half_x, half_y, coarse_max_score,
                                                                coarse_margin, margin)
    seeds_l = exhaustive_detect_objects(level_featuremap, small, objects, cms, overlap=coarse_overlap,
                                        cross_overlap=coarse_cross_overlap, stride=coarse_stride,
                                        max_detections=coarse_max_detections, penalty=penalty, angles=coarse_angles, pivot=pv_small,
                                        line_caps=coarse_line_caps, margin=cm, n_objects=n_objects)
    jobs = pose_windows(lift_records(seeds_l, level), coarse_angles, fine_angles, pv, half_angles, hx, hy, stride=stride, wrap=wrap)
    return exhaustive_detect_windows_objects(featuremap, templates, jobs, objects, max_score, overlap=overlap, cross_overlap=cross_overlap,
                                             angles=fine_angles, stride=stride, max_detections=max_detections, penalty=penalty,
                                             pivot=pivot, wrap=wrap, line_caps=line_caps, margin=margin, min_matched=min_matched,
                                             return_boxes=return_boxes, return_matched=return_matched, return_jobs=return_jobs,
                                             n_objects=n_objects, return_objects=return_objects, gate=gate)


# ---------------------------------------------------------------- objects: many views of a few parts (extension)
def object_score_maps(featuremap, templates, objects, stride=1, penalty=None, angles=None, pivot="center", window=None, line_caps=None,
                      min_matched=None, return_matched=False, n_objects=None):
    """best_score_map per object: objects[t] (0 .. G - 1) names the part template t is a view of, and every grid point keeps
    one best pair per object instead of one in all.  Returns (scores [G, ny, nx] float32, pairs [G, ny, nx] int32, grid), or
    with return_matched (scores, pairs, matched, grid): plane o is best_score_map of the templates of object o alone, with the
    pairs numbered in the whole set (NaN, -1 and NaN where no template of the object fits; an object without templates has an
    empty plane).  min_matched: None, a scalar, or one value per object.  n_objects None means max(objects) + 1.  The other
    arguments are best_score_map's."""
    kind, tau = _penalty_args(penalty)
    fm, tset, cs, pv, g = _detect_args(featuremap, templates, angles, pivot, stride, window, line_caps)
    obj, G, _, mm = _engine.object_arrays(objects, n_objects, tset.count, None, min_matched)
    if g[2] == 0 or g[3] == 0:
        empty = (_np.zeros((G, g[3], g[2]), dtype=_np.float32), _np.zeros((G, g[3], g[2]), dtype=_np.int32))
        return empty + ((_np.zeros((G, g[3], g[2]), dtype=_np.float32),) if return_matched else ()) + (g,)
    return fm.best_map_objects(tset, g, obj, G, cs, pv, penalty=kind, tau=tau, min_matched=mm, matched=return_matched) + (g,)


def exhaustive_detect_objects(featuremap, templates, objects, max_score, overlap=0.3, cross_overlap=None, stride=1, max_detections=1024,
                              penalty=None, angles=None, pivot="center", window=None, line_caps=None, margin=0, return_boxes=False,
                              min_matched=None, return_matched=False, n_objects=None, return_objects=False, gate="winner"):
    """exhaustive_detect_all for a set that holds many views of a few parts.  objects[t] (0 .. G - 1) is the part of template
    t; the candidates of the greedy rule are the (grid point, object) entries, each with the best pair among its object's
    templates, so two parts lying at one translation are both candidates.  max_score and min_matched are a scalar or one
    value per object: a clip of 6 lines and a housing of 40 each get their own.  A detection drops the entries of its own
    object whose footprints overlap its own by more than `overlap`, and the entries of other objects by more than
    cross_overlap (None: equal to overlap; 1 lets the objects ignore each other).  Entries are taken in the order (score, grid
    index, pair).  n_objects None means max(objects) + 1.  Returns a MatchList in ascending score, then with return_boxes the
    (n, 4) int32 footprints, with return_matched the (n,) float32 matched fractions and with return_objects the (n,) int32
    objects[tmpl_idx] of the detections, in that order.  The remaining arguments, gate included, are exhaustive_detect_all's;
    with one object the result is exhaustive_detect_all's."""
    _engine.gate_kind(gate)
    kind, tau = _penalty_args(penalty)
    permille = int(round(1000 * float(overlap)))
    cross = permille if cross_overlap is None else int(round(1000 * float(cross_overlap)))
    fm, tset, cs, pv, g = _detect_args(featuremap, templates, angles, pivot, stride, window, line_caps)
    obj, G, ms, mm = _engine.object_arrays(objects, n_objects, tset.count, max_score, min_matched)
    if g[2] == 0 or g[3] == 0:
        res = (_np.zeros(0, dtype=_capi.MATCH_DTYPE),) + ((_np.zeros((0, 4), dtype=_np.int32),) if return_boxes else ())
        res += (_np.zeros(0, dtype=_np.float32),) if return_matched else ()
    else:
        res = fm.exhaustive_detect_objects(tset, g, obj, ms, G, cs, pv, max_detections=max_detections, overlap_permille=permille,
                                           cross_permille=cross, margin=margin, penalty=kind, tau=tau, min_matched=mm,
                                           boxes=return_boxes, matched=return_matched, gate=gate)
        res = res if isinstance(res, tuple) else (res,)
    res += (obj[res[0]["tmpl_idx"]].astype(_np.int32),) if return_objects else ()
    res = (MatchList(res[0]),) + tuple(res[1:])
    return res if len(res) > 1 else res[0]


def exhaustive_detect_windows_objects(featuremap, templates, jobs, objects, max_score, overlap=0.3, cross_overlap=None, angles=None,
                                      stride=1, max_detections=1024, penalty=None, pivot="center", wrap=False, line_caps=None, margin=0,
                                      min_matched=None, return_boxes=False, return_matched=False, return_jobs=False, n_objects=None,
                                      return_objects=False, gate="winner"):
    """exhaustive_detect_windows with objects: a job's object is objects[tmpl] of its template; the job stays when its best
    pose's score is <= its object's max_score and, with min_matched, matches at least its object's share; a detection drops
    the jobs of its own object above `overlap` and those of other objects above cross_overlap (None: equal to overlap).
    max_score and min_matched are a scalar or one value per object; n_objects None means max(objects) + 1.  Returns
    exhaustive_detect_windows' results, and with return_objects the (n,) int32 objects of the detections last.  The other
    arguments are exhaustive_detect_windows'."""
    _engine.gate_kind(gate)
    kind, tau = _penalty_args(penalty)
    permille = int(round(1000 * float(overlap)))
    cross = permille if cross_overlap is None else int(round(1000 * float(cross_overlap)))
    sx, sy = _strides(stride)
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates, line_caps)
    obj, G, ms, mm = _engine.object_arrays(objects, n_objects, tset.count, max_score, min_matched)
    cs = pv = None
    if angles is not None:
        cs, pv = _angles(angles), _pivots(templates, pivot, tset.count)
    res = fm.exhaustive_detect_windows_objects(tset, jobs, obj, ms, G, cs, pv, sx=sx, sy=sy, wrap=wrap, max_detections=max_detections,
                                               overlap_permille=permille, cross_permille=cross, margin=margin, penalty=kind, tau=tau,
                                               min_matched=mm, boxes=return_boxes, matched=return_matched, job_index=return_jobs,
                                               gate=gate)
    res = res if isinstance(res, tuple) else (res,)
    res += (obj[res[0]["tmpl_idx"]].astype(_np.int32),) if return_objects else ()
    res = (MatchList(res[0]),) + tuple(res[1:])
    return res if len(res) > 1 else res[0]


def exhaustive_detect_refined_objects(featuremap, templates, objects, max_score, coarse_angles, fine_angles, coarse_stride, half_angles,
                                      half_x, half_y, coarse_max_score=None, coarse_overlap=1.0, coarse_cross_overlap=None,
                                      coarse_max_detections=1024, overlap=0.3, cross_overlap=None, stride=1, max_detections=1024,
                                      penalty=None, pivot="center", wrap=False, line_caps=None, margin=0, min_matched=None,
                                      return_boxes=False, return_matched=False, return_jobs=False, n_objects=None,
                                      return_objects=False, gate="winner"):
    """exhaustive_detect_refined with objects: pure Python over three calls, and by definition exactly their composition:
      seeds = exhaustive_detect_objects(featuremap, templates, objects, coarse_max_score (None: inf), overlap=coarse_overlap,
                                        cross_overlap=coarse_cross_overlap, stride=coarse_stride,
                                        max_detections=coarse_max_detections, penalty=penalty, angles=coarse_angles, pivot=pivot,
                                        line_caps=line_caps, margin=margin, n_objects=n_objects)
      jobs = pose_windows(seeds, coarse_angles, fine_angles, template_pivots(templates, pivot), half_angles, half_x, half_y,
                          stride=stride, wrap=wrap)
      exhaustive_detect_windows_objects(featuremap, templates, jobs, objects, max_score, overlap=overlap,
                                        cross_overlap=cross_overlap, angles=fine_angles, stride=stride,
                                        max_detections=max_detections, penalty=penalty, pivot=pivot, wrap=wrap,
                                        line_caps=line_caps, margin=margin, min_matched=min_matched, return_boxes=..,
                                        return_matched=.., return_jobs=.., n_objects=n_objects, return_objects=.., gate=gate)
    The coarse stage has no matched-fraction gate and by default neither a threshold nor suppression; its seeds are the best
    (grid point, object) entries, so every object at a point seeds a window of its own.  pose_windows needs no objects: a
    seed carries its template.  return_jobs indexes the seeds.  gate applies to the fine stage only."""
    _engine.gate_kind(gate)
    seeds = exhaustive_detect_objects(featuremap, templates, objects, float("inf") if coarse_max_score is None else coarse_max_score,
                                      overlap=coarse_overlap, cross_overlap=coarse_cross_overlap, stride=coarse_stride,
                                      max_detections=coarse_max_detections, penalty=penalty, angles=coarse_angles, pivot=pivot,
                                      line_caps=line_caps, margin=margin, n_objects=n_objects)
    jobs = pose_windows(seeds, coarse_angles, fine_angles, template_pivots(templates, pivot), half_angles, half_x, half_y,
                        stride=stride, wrap=wrap)
    return exhaustive_detect_windows_objects(featuremap, templates, jobs, objects, max_score, overlap=overlap, cross_overlap=cross_overlap,
                                             angles=fine_angles, stride=stride, max_detections=max_detections, penalty=penalty,
                                             pivot=pivot, wrap=wrap, line_caps=line_caps, margin=margin, min_matched=min_matched,
                                             return_boxes=return_boxes, return_matched=return_matched, return_jobs=return_jobs,
                                             n_objects=n_objects, return_objects=return_objects, gate=gate)


# ---------------------------------------------------------------- per-line caps and line costs (extension)
def line_caps(templates, tau):
    """The caps a scalar line_caps=tau stands for: per template the float32 array float32(tau) * len_i, len_i the line's
    length sqrt(dx * dx + dy * dy) in numpy float32.  A line's cost is roughly the sum of the directional distances under
    its pixels, so such a cap means roughly "a line whose mean distance exceeds tau pixels counts as tau" (approximately:
    within the rasteriser's factor between pixel count and length)."""
    return [_np.float32(tau) * l for l in _engine.line_lengths(templates)]


def line_costs(featuremap, templates, poses, angles=None, pivot="center"):
    """The uncapped cost of every template line at a list of poses: which edges of a detection were found.  poses is an
    (n, 4) int32 array of rows (tmpl, a, x, y): template tmpl under angle a of `angles` (0 without angles, the lines as they
    are) translated by (x, y).  Returns (float32 flat array, int64 offsets of n + 1): pose q's costs, one per line of its
    template in line order, are flat[offsets[q]:offsets[q + 1]]; all NaN when the pose puts the template outside the feature
    map.  Clamping them with the caps and summing in the scores' order gives the score of that pose bit for bit.
    pose_windows(records, angles, angles, pivots, 0, 0, 0)[:, [0, 1, 3, 4]] turns the records of the dense searches over
    `angles` (pivots = template_pivots(templates, pivot)) into poses; for searches without angles the poses are
    (tmpl_idx, 0, transform[2], transform[5]).  With caps c, the matched fraction of a pose is
    sum(len_i[cost_i <= c_i]) / sum(len_i); matched_fractions computes it on the device."""
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates)
    cs = pv = None
    if angles is not None:
        cs, pv = _angles(angles), _pivots(templates, pivot, tset.count)
    return fm.line_costs(tset, poses, cs, pv)


def matched_fractions(featuremap, templates, poses, angles=None, pivot="center", line_caps=None):
    """The matched fraction of every pose of an (n, 4) int32 array of rows (tmpl, a, x, y), as line_costs takes them: the
    share of the template's line length whose lines cost at most their caps (line_caps, exhaustive_search's) at the pose,
    computed on the device by exhaustive_detect_all's rule.  1 for a template whose line lengths sum to 0, NaN where the pose
    puts the template outside the feature map.  In a tracker that follows a pose with exhaustive_window_search, a fraction
    that falls means the track is lost.  Returns an (n,) float32 array."""
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates, line_caps)
    cs = pv = None
    if angles is not None:
        cs, pv = _angles(angles), _pivots(templates, pivot, tset.count)
    return fm.matched_fractions(tset, poses, cs, pv)


# ---------------------------------------------------------------- scene coverage (extension)
def record_poses(records, angles=None, pivots=None):
    """The (n, 4) int32 poses (tmpl, a, x, y) of detection records (a MatchList or its record array, tmpl_idx without a
    base), as line_costs, matched_fractions and scene_coverage take them: pure numpy.  With the angles of the search (and its
    pivots, template_pivots, or None for the origin) exactly pose_windows(records, angles, angles, pivots, 0, 0, 0)[:, [0, 1, 3, 4]];
    without angles (tmpl_idx, 0, rint(transform[2]), rint(transform[5]))."""
    if angles is not None:
        return _np.ascontiguousarray(pose_windows(records, angles, angles, pivots, 0, 0, 0)[:, [0, 1, 3, 4]], dtype=_np.int32)
    rec = records.records() if isinstance(records, MatchList) else _np.asarray(records)
    out = _np.zeros((rec.shape[0], 4), dtype=_np.int32)
    out[:, 0] = rec["tmpl_idx"]
    out[:, 2] = _np.rint(rec["transform"][:, 2].astype(_np.float64)).astype(_np.int64)
    out[:, 3] = _np.rint(rec["transform"][:, 5].astype(_np.float64)).astype(_np.int64)
    return out


def scene_coverage(featuremap, labels, templates, poses, angles=None, pivot="center", radius=2, bin_tolerance=1, margin=None,
                   return_residual=False):
    """Which edge pixels a pose explains: the cue that runs from the scene to the template.  labels is the label image the
    feature map was built from (edge_labels; a numpy array or a contiguous CUDA tensor), poses an (n, 4) int32 array of rows
    (tmpl, a, x, y) as line_costs takes them (record_poses makes them from detections).  Per pose: the number of edge pixels in
    its window -- the template's footprint there, widened by margin (None: radius) and cut to the image -- and the number of
    those within radius pixels of one of the posed template's segments whose orientation slice is within bin_tolerance of the
    pixel's (circular).  explained / edges is near 1 for a part lying alone and low for a hit in clutter, which the score
    and the matched fraction cannot tell apart.  (-1, -1) where the pose puts the template outside the feature map.  Returns
    the (n, 2) int32 counts, and with return_residual also the labels with 255 at every explained pixel (a tensor on the
    same device for a tensor): rebuild_labels(residual) gives the map of the next round of a detect, explain away, detect
    again loop.  The map must be one built from an image or from labels."""
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates)
    cs = pv = None
    if angles is not None:
        cs, pv = _angles(angles), _pivots(templates, pivot, tset.count)
    return fm.scene_coverage(labels, tset, poses, cs, pv, radius=radius, bin_tolerance=bin_tolerance, margin=margin,
                             residual=return_residual)


def scene_select(featuremap, labels, templates, poses, angles=None, pivot="center", radius=2, bin_tolerance=1, margin=None,
                 min_coverage=0.0, min_new=0.5, min_pixels=1, max_selected=1024, return_residual=False):
    """Greedy explain-away over a pose list, on the device: which of the poses, taken in list order (record_poses of a
    detection list is best first), account for scene edges nobody before them has claimed.  Two poses conflict when they
    claim the same edge pixels, not when their boxes overlap, so parts that interlock or lie in each other's notches are
    both kept while shifted copies of an accepted pose are not.  labels, templates, poses, angles, pivot, radius,
    bin_tolerance and margin are scene_coverage's.  A pose is a candidate when it is admissible, explains at least
    min_pixels edge pixels and at least the share min_coverage of the edge pixels in its window; a candidate is accepted
    when at least min_pixels and the share min_new of the pixels it explains are unclaimed at its turn, and then claims what
    it explains; at most max_selected (1 .. 4096) are accepted.  Shares are taken in permille, int(round(1000 * v)).
    Returns (selected, counts): the (k,) int32 indices into poses, ascending, and (k, 3) int32 rows (edges, explained, new);
    with return_residual also the labels with 255 at every claimed pixel (a tensor on the same device for a tensor), which
    is scene_coverage's residual of poses[selected]."""
    fm = _device_map(featuremap)
    tset = _template_cache.get(templates)
    cs = pv = None
    if angles is not None:
        cs, pv = _angles(angles), _pivots(templates, pivot, tset.count)
    return fm.scene_select(labels, tset, poses, cs, pv, radius=radius, bin_tolerance=bin_tolerance, margin=margin,
                           min_coverage=min_coverage, min_new=min_new, min_pixels=min_pixels, max_selected=max_selected,
                           residual=return_residual)


# ---------------------------------------------------------------- match lists (extension)
def detect_matches(featuremap, templates, matches, max_score=float("inf"), overlap=0.3, max_detections=1024, penalty=None, margin=0,
                   line_caps=None, min_matched=0.0, rescore=False, return_indices=False, return_boxes=False, return_matched=False,
                   device_ptr=None, n=0):
    """One record per part out of what search() returns: the greedy rule of exhaustive_detect_all by footprint overlap on a
    match list, on the device.  search() gives a record for every pair of aligned lines near a true pose; each record is
    posed again with its own transform, its lines are costed (line_caps as in exhaustive_search), and the records that lie
    inside the map, whose score divided by the penalty's denominator (penalty: None, DefaultPenalty or ExponentialPenalty) is
    at most max_score and whose matched fraction is at least min_matched go through the rule keyed by (score, position in
    the list), until they run out or max_detections (1 to 4096) is reached.  The score is the record's own (a caller who has
    penalised already passes penalty=None) or, with rescore, the sum of the capped line costs of the posed lines, which is
    close to the search's score but not its bits.  matches: a MatchList or a record array; None for the records of the
    last search() on this feature map, still on the device; or device_ptr and n for records in device memory.  Returns a
    MatchList in ascending score, and in a tuple with it, in this order, with return_indices the (k,) int32 positions of the
    records in the list, with return_boxes the (k, 4) int32 footprints, with return_matched the (k,) float32 fractions."""
    kind, tau = _penalty_args(penalty)
    permille = int(round(1000 * float(overlap)))
    fm, tset = _device_map(featuremap), _template_cache.get(templates, line_caps)
    res = fm.detect_matches(tset, matches, max_score=max_score, overlap_permille=permille, max_detections=max_detections, penalty=kind,
                            tau=tau, margin=margin, min_matched=min_matched, rescore=rescore, indices=return_indices, boxes=return_boxes,
                            matched=return_matched, device_ptr=device_ptr, n=n)
    return (MatchList(res[0]),) + tuple(res[1:]) if isinstance(res, tuple) else MatchList(res)


def detect_matches_objects(featuremap, templates, matches, objects=None, max_score=float("inf"), overlap=0.3, cross_overlap=None,
                           max_detections=1024, penalty=None, margin=0, line_caps=None, min_matched=None, rescore=False,
                           n_objects=None, return_indices=False, return_boxes=False, return_matched=False, return_objects=False,
                           device_ptr=None, n=0):
    """detect_matches for a template list that holds views of several parts, on the list's kind of footprint.  objects[t]
    (0 .. G - 1) is the part of template t (None: one object); max_score and min_matched are a scalar or one value per
    object; a record drops the records of its own object whose footprints overlap its own by more than `overlap` and those
    of other objects by more than cross_overlap (None: equal to overlap; 1 lets the objects ignore each other).  For
    with_footprint(templates, "hull") the footprint of a record is the lattice points of the convex hull of its posed end
    points, built on the device for every candidate record -- the shape that tells two parallel rods at 45 degrees apart,
    whose boxes overlap -- and objects=None is the way to get it without labels.  n_objects None means max(objects) + 1.
    Returns detect_matches' results, and with return_objects the (k,) int32 objects of the records last.  The other arguments
    are detect_matches'."""
    kind, tau = _penalty_args(penalty)
    permille = int(round(1000 * float(overlap)))
    cross = permille if cross_overlap is None else int(round(1000 * float(cross_overlap)))
    fm, tset = _device_map(featuremap), _template_cache.get(templates, line_caps)
    obj = _np.zeros(tset.count, dtype=_np.int32) if objects is None else _np.asarray(objects)
    res = fm.detect_matches_objects(tset, matches, obj, max_score, n_objects=n_objects, overlap_permille=permille, cross_permille=cross,
                                    max_detections=max_detections, penalty=kind, tau=tau, margin=margin, min_matched=min_matched,
                                    rescore=rescore, indices=return_indices, boxes=return_boxes, matched=return_matched,
                                    device_ptr=device_ptr, n=n)
    res = res if isinstance(res, tuple) else (res,)
    res += (obj.reshape(-1).astype(_np.int32)[res[0]["tmpl_idx"]],) if return_objects else ()
    res = (MatchList(res[0]),) + tuple(res[1:])
    return res if len(res) > 1 else res[0]


def match_footprint_spans(templates, matches, margin=0):
    """The hull shapes of the posed lines of every record of a match list, as detect_matches_objects uses them on a "hull"
    list: (row_offsets, spans, areas), record j having the rows row_offsets[j] .. row_offsets[j + 1] of spans, row r at
    y = y0 of match_footprints()[j] + (r - row_offsets[j]), its pixels xl .. xr in the frame of that box, (0, -1) when the row
    is empty.  Host only."""
    return _engine.match_footprint_spans(_template_cache.get(templates), matches, margin)


def match_shapes(featuremap, templates, matches, margin=0, device_ptr=None, n=0):
    """match_footprint_spans from the device kernel, for the records that lie inside the feature map (the others have no rows
    and area 0).  matches: a MatchList or a record array, or device_ptr and n."""
    return _device_map(featuremap).match_shapes(_template_cache.get(templates), matches, margin=margin, device_ptr=device_ptr, n=n)


def verify_matches(featuremap, templates, matches, line_caps=None, device_ptr=None, n=0):
    """Which lines of a match were found: (scores, fractions, costs) of every record of a match list, the forms of which are
    detect_matches'.  costs is an (n, Lmax) float32 array, the uncapped cost of every line of the record's template posed by
    the record's transform, NaN beyond the template's line count; scores the sum of the costs clamped to line_caps, in the
    scores' order; fractions the matched fraction of matched_fractions.  All NaN for a record whose posed lines leave the
    map or whose tmpl_idx is outside the list."""
    fm, tset = _device_map(featuremap), _template_cache.get(templates, line_caps)
    return fm.verify_matches(tset, matches, device_ptr=device_ptr, n=n)


def delta_angles(half_steps, step):
    """The 2 * half_steps + 1 delta angles (-half_steps .. half_steps) * step in radians, float64, for refine_matches; the zero
    is exact, at index half_steps."""
    return _np.arange(-int(half_steps), int(half_steps) + 1, dtype=_np.float64) * float(step)


def refine_matches(featuremap, templates, matches, angles=None, pivot="center", half_x=0, half_y=0, stride=1, line_caps=None,
                   return_poses=False, device_ptr=None, n=0, out_device_ptr=None):
    """The pose of every record of a match list refined on the device: search() takes a record's rotation from one aligned
    pair of lines and its translation from a walk along one scene line, so a record near a true pose is typically a degree
    or two and a few pixels off.  Every record is searched exhaustively in its own small box of poses: the delta rotations
    `angles` (radians, delta_angles(..); None: none) about `pivot` in template coordinates ("center", None for the origin or a
    (T, 2) array), times the translations (i * sx, j * sy) with |i| <= half_x, |j| <= half_y and stride an int or (sx, sy).
    The record is replaced by the best pose of its box -- its score the sum of the line costs there, clamped to line_caps --
    with ties going to the pose it had (the delta whose (cos, sin) is exactly (1, 0), with no translation).  A record whose
    box holds no pose inside the map, or whose tmpl_idx is outside the list, keeps its transform and scores NaN, which
    detect_matches never keeps: search -> refine_matches -> detect_matches is the chain.  matches follows detect_matches: a
    MatchList or a record array, None for the records of the last search() on this feature map, or device_ptr and n for a
    device buffer; out_device_ptr: a device buffer the records go to instead (it may be device_ptr), None standing in their
    place.  Returns a MatchList aligned with the input, and with return_poses also the (n, 3) int32 rows (angle index, i, j),
    (-1, 0, 0) for a record without a pose."""
    fm, tset = _device_map(featuremap), _template_cache.get(templates, line_caps)
    sx, sy = _strides(stride)
    cs = None if angles is None else _angles(angles)
    pv = None if angles is None else _pivots(templates, pivot, tset.count)
    res = fm.refine_matches(tset, matches, cs=cs, pivots=pv, hx=half_x, hy=half_y, sx=sx, sy=sy, poses=return_poses, device_ptr=device_ptr,
                            n=n, out_device_ptr=out_device_ptr)
    recs = res[0] if return_poses else res
    recs = None if recs is None else MatchList(recs)
    return (recs, res[1]) if return_poses else recs


def match_coverage(featuremap, labels, templates, matches, radius=2, bin_tolerance=1, margin=None, return_residual=False,
                   device_ptr=None, n=0):
    """scene_coverage for what search() returns: which edge pixels of labels each record explains, the record posed by its
    own free transform (no angle table, no integer translation).  It tells a hit in texture (explained / edges low) from a
    clean part.  labels is the label image the feature map was built from (a numpy array or a contiguous CUDA tensor; a
    tensor gives the residual as a tensor); a transform maps template to scene coordinates and a scene point is a label
    pixel, so the records may come from a search on any map of the scene.  matches follows detect_matches: a MatchList or a
    record array, None for the records of the last search() on this feature map, or device_ptr and n for a device buffer.
    radius, bin_tolerance and margin (None: the radius) are scene_coverage's; the window of a record is its footprint
    (match_footprints) at the margin, cut to the image.  Returns the (n, 2) int32 counts (edges, explained), (-1, -1) for a
    record whose posed lines leave the map or whose tmpl_idx is outside the list, and with return_residual also the labels
    with 255 at every explained pixel."""
    fm, tset = _device_map(featuremap), _template_cache.get(templates)
    return fm.match_coverage(labels, tset, matches, radius=radius, bin_tolerance=bin_tolerance, margin=margin, residual=return_residual,
                             device_ptr=device_ptr, n=n)


def fit_matches(featuremap, labels, templates, matches, radius=3, bin_tolerance=1, margin=None, iterations=2, min_pixels=8,
                damping=1e-3, max_shift=None, max_angle=0.1, return_info=False, return_rms=False, device_ptr=None, n=0,
                out_device_ptr=None):
    """The continuous last stage of search -> refine_matches -> fit_matches -> detect_matches(rescore=True): every record's
    transform fitted by rigid least squares to the edge pixels of labels it explains, on the device.  search() and
    refine_matches return poses on the lattice they searched; a step here is closed form: every edge pixel of the record's
    window that lies within `radius` of the inside of a posed line of its orientation (bin_tolerance) is assigned to its
    nearest such line, and the rotation and translation that minimise the squared distances to those lines are solved for
    and folded into the transform; `iterations` (1 .. 8) such steps.  A record stops early when it has fewer than min_pixels
    fit pixels (status 1), when the system is singular (2: a single straight line does not fix a pose), when a step exceeds
    max_shift pixels (None: the radius) or max_angle radians (3), or when the step would leave the map (4, not taken); status
    0 took every step and -1 is a record that is invalid or outside the map, which is returned as it is.  damping is the share
    of the diagonal added to it.  labels, matches, radius, bin_tolerance and margin are match_coverage's; out_device_ptr is
    refine_matches'.  Returns a MatchList aligned with the input, scores unchanged (rescore with detect_matches or
    verify_matches); with return_info also the (n, 4) int32 rows (status, steps, fit pixels before, after), with return_rms
    the (n, 2) float32 rms distances of the fit pixels to their lines before and after."""
    fm, tset = _device_map(featuremap), _template_cache.get(templates)
    res = fm.fit_matches(labels, tset, matches, radius=radius, bin_tolerance=bin_tolerance, margin=margin, iterations=iterations,
                         min_pixels=min_pixels, damping=damping, max_shift=max_shift, max_angle=max_angle, info=return_info, rms=return_rms,
                         device_ptr=device_ptr, n=n, out_device_ptr=out_device_ptr)
    res = res if isinstance(res, tuple) else (res,)
    res = (None if res[0] is None else MatchList(res[0]),) + res[1:]
    return res if len(res) > 1 else res[0]


def select_matches(featuremap, labels, templates, matches, radius=2, bin_tolerance=1, margin=None, min_coverage=0.0, min_new=0.5,
                   min_pixels=1, max_selected=1024, return_residual=False, device_ptr=None, n=0):
    """scene_select for what search() returns: greedy explain-away over match records, on the device.  Records conflict when
    they claim the same edge pixels, not when their boxes overlap, so parts that interlock or lie in each other's notches are
    both kept.  The list order is the priority: pass sort_matches(penalize(..)), or the output of
    detect_matches(.., overlap=1.0), which ascends by key and has dropped what lies outside the map.  At most 2^16 records:
    cut a longer list with detect_matches first.  labels, matches, radius, bin_tolerance and margin are match_coverage's;
    min_coverage, min_new, min_pixels and max_selected are scene_select's, the shares taken in permille,
    int(round(1000 * v)).  Returns (selected, counts): the (k,) int32 positions in matches, ascending, and (k, 3) int32 rows
    (edges, explained, new); with return_residual also the labels with 255 at every claimed pixel.  matches[selected] are the
    parts."""
    fm, tset = _device_map(featuremap), _template_cache.get(templates)
    return fm.select_matches(labels, tset, matches, radius=radius, bin_tolerance=bin_tolerance, margin=margin, min_coverage=min_coverage,
                             min_new=min_new, min_pixels=min_pixels, max_selected=max_selected, residual=return_residual,
                             device_ptr=device_ptr, n=n)


def match_footprints(templates, matches, margin=0):
    """The (n, 4) int32 footprints x0, y0, x1, y1 of the posed lines of every record of a match list, as detect_matches uses
    them; (0, 0, -1, -1) for a record whose tmpl_idx is outside the list, a template without lines or a NaN end point."""
    return _engine.match_footprints(_template_cache.get(templates), matches, margin)


from .lineio import read, write  # noqa: E402  (.lines/.scene/.tmpl files, serialization.h)
