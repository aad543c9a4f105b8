"""Thin object layer over the C ABI: HBM-resident feature maps and template sets."""
import ctypes as C

import numpy as np

from . import _capi as capi


def _adopt_matches(ptr, n):
    """Wrap a library-allocated fdcm_match array as a structured numpy array without copying; the
    allocation is released (fdcm_matches_free) when the array is garbage collected."""
    import weakref
    if not ptr or n == 0:
        if ptr:
            capi.lib().fdcm_matches_free(ptr)
        return np.zeros(0, dtype=capi.MATCH_DTYPE)
    raw = (C.c_char * (n * capi.MATCH_DTYPE.itemsize)).from_address(ptr.value)
    res = np.frombuffer(raw, dtype=capi.MATCH_DTYPE)
    weakref.finalize(raw, capi.lib().fdcm_matches_free, C.c_void_p(ptr.value))
    return res


def _rotations(cs, pivots, T):
    """(capi.Rotations, the arrays it points to): cs (n, 2) float32, pivots (T, 2) float32 or None."""
    cs = np.ascontiguousarray(cs, dtype=np.float32).reshape(-1, 2)
    rot = capi.Rotations(capi.fptr(cs), cs.shape[0], None)
    keep = [cs]
    if pivots is not None:
        pv = np.ascontiguousarray(pivots, dtype=np.float32).reshape(-1, 2)
        if pv.shape[0] != T:
            raise ValueError("one pivot per template is required")
        rot.pivots = capi.fptr(pv)
        keep.append(pv)
    return rot, keep


def gate_kind(gate):
    """FDCM_GATE_WINNER / FDCM_GATE_ALL (include/fdcm.h, "Gate inside the minimum") for gate = "winner" / "all"."""
    if gate == "winner":
        return capi.GATE_WINNER
    if gate == "all":
        return capi.GATE_ALL
    raise ValueError('gate must be "winner" or "all"')


def object_arrays(objects, n_objects, T, max_score, min_matched):
    """(objects int32 (T,), G, max_score float32 (G,) or None, min_matched float32 (G,) or None) for the calls with objects
    (include/fdcm.h, "Objects").  n_objects None: max(objects) + 1 (1 for an empty set).  max_score and min_matched: None, a
    scalar for every object, or one value per object.  The library checks the values."""
    obj = np.asarray(objects)
    if obj.size and not np.issubdtype(obj.dtype, np.integer):
        raise ValueError("objects must be integers, one per template")
    obj = np.ascontiguousarray(obj.reshape(-1), dtype=np.int32)
    if obj.shape[0] != T:
        raise ValueError("one object label per template is required")
    G = int(n_objects) if n_objects is not None else (int(obj.max()) + 1 if obj.size else 1)

    def per_object(v, what):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float32)
        if a.ndim == 0:
            return np.full(max(G, 1), a, dtype=np.float32)
        if a.ndim != 1 or a.shape[0] != G:
            raise ValueError(what + " must be a scalar or one value per object")
        return np.ascontiguousarray(a)

    return obj, G, per_object(max_score, "max_score"), per_object(min_matched, "min_matched")


def as_grid(grid):
    """capi.Grid from a capi.Grid or an (x0, y0, nx, ny, sx, sy) sequence."""
    if isinstance(grid, capi.Grid):
        return grid
    vals = [int(v) for v in grid]
    if len(vals) != 6:
        raise ValueError("a grid is (x0, y0, nx, ny, sx, sy)")
    return capi.Grid(*vals)


def as_pose_windows(jobs):
    """(n, 7) contiguous int32 rows in fdcm_pose_window's order, from such an array or a POSE_WINDOW_DTYPE array."""
    a = np.asarray(jobs)
    if a.dtype == capi.POSE_WINDOW_DTYPE:
        a = a.view(np.int32).reshape(-1, 7)
    if a.size == 0:
        return np.zeros((0, 7), dtype=np.int32)
    if a.ndim != 2 or a.shape[1] != 7 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("jobs must be an (n, 7) integer array: tmpl, a0, na, x0, y0, nx, ny")
    if np.any(a != a.astype(np.int32)):
        raise ValueError("jobs: a value does not fit int32")
    return np.ascontiguousarray(a, dtype=np.int32)


def as_poses(poses):
    """(n, 4) contiguous int32 rows (tmpl, a, x, y) of fdcm_line_costs."""
    a = np.asarray(poses)
    if a.size == 0:
        return np.zeros((0, 4), dtype=np.int32)
    if a.ndim != 2 or a.shape[1] != 4 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("poses must be an (n, 4) integer array: tmpl, a, x, y")
    if np.any(a != a.astype(np.int32)):
        raise ValueError("poses: a value does not fit int32")
    return np.ascontiguousarray(a, dtype=np.int32)


def match_records(matches):
    """A match list as one contiguous record array (capi.MATCH_DTYPE): a MatchList's records or such an array, not copied when
    it is contiguous already."""
    rec = matches.records() if hasattr(matches, "records") else np.asarray(matches)
    if rec.dtype != capi.MATCH_DTYPE:
        raise ValueError("matches must be a MatchList or an array of match records")
    return np.ascontiguousarray(rec.reshape(-1))


def match_footprints(templates, matches, margin=0, tmpl_index_base=0):
    """fdcm_matches_footprints: the (n, 4) int32 footprints x0, y0, x1, y1 of the posed lines of every record of a match list
    (include/fdcm.h, "Match lists"); (0, 0, -1, -1) for an invalid record, a template without lines or a NaN end point.  Host
    only.  templates: a DeviceTemplates."""
    rec = match_records(matches)
    out = np.zeros((rec.shape[0], 4), dtype=np.int32)
    capi.check(capi.lib().fdcm_matches_footprints(templates._h, C.c_void_p(rec.ctypes.data) if rec.shape[0] else None, rec.shape[0],
                                                  int(tmpl_index_base), int(margin),
                                                  out.ctypes.data_as(C.POINTER(C.c_int32)) if rec.shape[0] else None))
    return out


def line_lengths(templates):
    """Per template the float32 lengths of its lines, sqrt(dx * dx + dy * dy) in numpy float32."""
    out = []
    for t in templates:
        a = np.asarray(t, dtype=np.float32).reshape(4, -1)
        dx, dy = a[2] - a[0], a[3] - a[1]
        out.append(np.sqrt(dx * dx + dy * dy))
    return out


def flat_line_caps(templates, line_caps, counts=None):
    """The caps of a template list as one float32 array in line order, or None for no caps.  line_caps: None, a scalar tau
    (caps float32(tau) * len_i, line_lengths) or one float array per template."""
    if line_caps is None:
        return None
    if np.isscalar(line_caps) or (isinstance(line_caps, np.ndarray) and line_caps.ndim == 0):
        per = [np.float32(line_caps) * l for l in line_lengths(templates)]
    else:
        per = [np.asarray(c, dtype=np.float32).reshape(-1) for c in line_caps]
    if counts is None:
        counts = [np.asarray(t).reshape(4, -1).shape[1] for t in templates]
    if len(per) != len(counts) or any(len(c) != n for c, n in zip(per, counts)):
        raise ValueError("line_caps needs one array per template with one cap per line")
    flat = np.concatenate(per).astype(np.float32) if per else np.zeros(0, dtype=np.float32)
    if np.any(np.isnan(flat)) or np.any(flat < 0):
        raise ValueError("line_caps must be >= 0 or +inf, never NaN")
    return np.ascontiguousarray(flat)


def _pixels(a, what):
    """(pointer, width, height, row_stride, on_device, keep-alive) of a 2-D uint8 numpy array (copied unless its rows are
    contiguous) or a 2-D CUDA torch.uint8 tensor (by data_ptr(), after its stream's pending work)."""
    if isinstance(a, np.ndarray) or not hasattr(a, "data_ptr"):
        a = np.asarray(a)
        if a.ndim != 2 or a.dtype != np.uint8:
            raise ValueError(f"{what} must be a 2-D uint8 array, got {a.dtype} with shape {a.shape}")
        if a.size and (a.strides[1] != 1 or a.strides[0] < a.shape[1]):
            a = np.ascontiguousarray(a)
        stride = a.strides[0] if a.shape[0] > 1 and a.size else a.shape[1]
        return C.c_void_p(a.ctypes.data), a.shape[1], a.shape[0], stride, 0, a
    import torch
    if a.dim() != 2 or a.dtype != torch.uint8 or not a.is_cuda:
        raise ValueError(f"{what} must be a 2-D uint8 tensor on the GPU")
    if a.numel() and (a.stride(1) != 1 or a.stride(0) < a.shape[1]):
        a = a.contiguous()
    torch.cuda.current_stream(a.device).synchronize()  # the build reads it from the handle's own stream
    stride = a.stride(0) if a.shape[0] > 1 and a.numel() else a.shape[1]
    return C.c_void_p(a.data_ptr()), a.shape[1], a.shape[0], stride, 1, a


def _edge_params(threshold, low, smooth, min_pixels):
    """None when the options are the defaults (the entry points with `threshold` alone take the call), else the
    fdcm_edge_params of the _ex entry points: `threshold` is the high threshold, low=None means low = threshold."""
    if low is None and int(smooth) == 0 and int(min_pixels) == 1:
        return None
    return capi.EdgeParams(int(smooth), int(threshold if low is None else low), int(threshold), int(min_pixels))


def _level_edge_params(threshold, low, smooth, min_pixels):
    """The fdcm_edge_params of the entry points with a level, which take no bare threshold: the defaults are {0, t, t, 1}."""
    return capi.EdgeParams(int(smooth), int(threshold if low is None else low), int(threshold), int(min_pixels))


def image_pyramid_size(width, height, level):
    """(W_l, H_l) of level `level` of a width x height image: W_(l+1) = (W_l + 1) >> 1.  No device work."""
    w, h = C.c_int64(), C.c_int64()
    capi.check(capi.lib().fdcm_image_pyramid_size(int(width), int(height), int(level), C.byref(w), C.byref(h)))
    return w.value, h.value


def image_pyramid(image, level):
    """Level `level` (0 to 12) of a 2-D uint8 image (include/fdcm.h, "image pyramid"): P_(l+1)(x, y) is the smooth = 2 image of
    P_l at (2x, 2y), made on the GPU.  A numpy array gives a numpy array; a CUDA torch tensor gives a tensor on its device,
    written there."""
    p, w, h, stride, dev, keep = _pixels(image, "image")
    wl, hl = image_pyramid_size(w, h, level)
    if dev:
        import torch
        out = torch.empty((hl, wl), dtype=torch.uint8, device=keep.device)
        q = C.c_void_p(out.data_ptr())
    else:
        out = np.empty((hl, wl), dtype=np.uint8)
        q = C.c_void_p(out.ctypes.data)
    capi.check(capi.lib().fdcm_image_pyramid_level(p, w, h, stride, dev, int(level), q, dev))
    return out


class DeviceFeatureMap:
    """Owns an fdcm_featuremap handle (DT3 volume resident in HBM)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        self.refresh()

    def refresh(self):
        info = capi.FeaturemapInfo()
        capi.check(capi.lib().fdcm_featuremap_get_info(self._h, C.byref(info)))
        self.width, self.height, self.depth = info.width, info.height, info.depth
        self.scene_translation = np.array(list(info.scene_translation), dtype=np.float32)
        self.distance = info.distance
        self.keys = np.zeros(self.depth, dtype=np.float32)
        if self.depth:
            capi.check(capi.lib().fdcm_featuremap_keys(self._h, capi.fptr(self.keys)))

    @classmethod
    def build(cls, scene, depth=30, coeff=5.0, padding=2.2, distance=capi.L2, stop_after=3):
        rec = capi.as_records(scene)
        h = C.c_void_p()
        if stop_after == 3:
            rc = capi.lib().fdcm_featuremap_build(capi.fptr(rec), rec.shape[0], int(depth), float(coeff),
                                                  float(padding), int(distance), C.byref(h))
        else:
            rc = capi.lib().fdcm_featuremap_build_staged(capi.fptr(rec), rec.shape[0], int(depth), float(coeff),
                                                         float(padding), int(distance), int(stop_after), C.byref(h))
        capi.check(rc)
        return cls(h)

    @classmethod
    def from_volume(cls, keys, volume, scene_translation):
        """volume: (depth, W, H) float32, [k][x][y]."""
        keys = np.ascontiguousarray(keys, dtype=np.float32)
        vol = np.ascontiguousarray(volume, dtype=np.float32)
        st = np.ascontiguousarray(scene_translation, dtype=np.float32)
        if vol.size == 0:
            m, W, H = len(keys), 0, 0
        else:
            m, W, H = vol.shape
        h = C.c_void_p()
        capi.check(capi.lib().fdcm_featuremap_from_slices(capi.fptr(keys), m, capi.fptr(vol), W, H, capi.fptr(st),
                                                          C.byref(h)))
        return cls(h)

    def rebuild(self, scene):
        rec = capi.as_records(scene)
        capi.check(capi.lib().fdcm_featuremap_rebuild(self._h, capi.fptr(rec), rec.shape[0]))
        self.refresh()

    # ---- feature maps from images (include/fdcm.h, "feature maps from images"): image / labels are 2-D uint8, (H, W), a
    #      numpy array or a CUDA torch tensor (read in place; kept alive here until the next build)
    @classmethod
    def build_image(cls, image, threshold, border=0, depth=30, coeff=5.0, distance=capi.L2, stop_after=3, low=None, smooth=0,
                    min_pixels=1):
        """The DT3 volume whose seeds are the oriented edge pixels of `image`: size (W + 2 border, H + 2 border), scene
        translation (border, border).  low / smooth / min_pixels: hysteresis below `threshold`, smoothing and the smallest
        component kept (include/fdcm.h, fdcm_edge_params)."""
        p, w, h, stride, dev, keep = _pixels(image, "image")
        out = C.c_void_p()
        ex = _edge_params(threshold, low, smooth, min_pixels)
        if ex is not None:
            if stop_after != 3:
                raise ValueError("build_image: stop_after != 3 cannot be combined with low, smooth or min_pixels")
            rc = capi.lib().fdcm_featuremap_build_image_ex(p, w, h, stride, dev, C.byref(ex), int(border), int(depth), float(coeff),
                                                           int(distance), C.byref(out))
        elif stop_after == 3:
            rc = capi.lib().fdcm_featuremap_build_image(p, w, h, stride, dev, int(threshold), int(border), int(depth),
                                                        float(coeff), int(distance), C.byref(out))
        else:
            rc = capi.lib().fdcm_featuremap_build_image_staged(p, w, h, stride, dev, int(threshold), int(border), int(depth),
                                                               float(coeff), int(distance), int(stop_after), C.byref(out))
        capi.check(rc)
        fm = cls(out)
        fm._seed_pixels = keep
        return fm

    @classmethod
    def build_labels(cls, labels, border=0, depth=30, coeff=5.0, distance=capi.L2):
        """The same from a label image: value k < depth's key count seeds slice k, anything else is no edge."""
        p, w, h, stride, dev, keep = _pixels(labels, "labels")
        if stride != w:
            keep = keep.contiguous() if dev else np.ascontiguousarray(keep)
            p = C.c_void_p(keep.data_ptr() if dev else keep.ctypes.data)
        out = C.c_void_p()
        capi.check(capi.lib().fdcm_featuremap_build_labels(p, w, h, dev, int(border), int(depth), float(coeff), int(distance),
                                                           C.byref(out)))
        fm = cls(out)
        fm._seed_pixels = keep
        return fm

    def rebuild_image(self, image, threshold, border=0, low=None, smooth=0, min_pixels=1):
        p, w, h, stride, dev, keep = _pixels(image, "image")
        ex = _edge_params(threshold, low, smooth, min_pixels)
        if ex is not None:
            capi.check(capi.lib().fdcm_featuremap_rebuild_image_ex(self._h, p, w, h, stride, dev, C.byref(ex), int(border)))
        else:
            capi.check(capi.lib().fdcm_featuremap_rebuild_image(self._h, p, w, h, stride, dev, int(threshold), int(border)))
        self._seed_pixels = keep
        self.refresh()

    # ---- feature maps of a pyramid level (include/fdcm.h, "image pyramid"): build_image of the image reduced by 2^level
    @classmethod
    def build_image_level(cls, image, level, threshold, border=0, depth=30, coeff=5.0, distance=capi.L2, low=None, smooth=0,
                          min_pixels=1):
        """The DT3 volume of level `level` (0 to 12) of `image`: by definition build_image of image_pyramid(image, level) with
        the same options; border is in the level's pixels.  The levels are made on the device, in a workspace of the handle."""
        p, w, h, stride, dev, keep = _pixels(image, "image")
        out = C.c_void_p()
        ex = _level_edge_params(threshold, low, smooth, min_pixels)
        capi.check(capi.lib().fdcm_featuremap_build_image_level(p, w, h, stride, dev, int(level), C.byref(ex), int(border), int(depth),
                                                                float(coeff), int(distance), C.byref(out)))
        fm = cls(out)
        fm._seed_pixels = keep
        return fm

    def rebuild_image_level(self, image, level, threshold, border=0, low=None, smooth=0, min_pixels=1):
        p, w, h, stride, dev, keep = _pixels(image, "image")
        ex = _level_edge_params(threshold, low, smooth, min_pixels)
        capi.check(capi.lib().fdcm_featuremap_rebuild_image_level(self._h, p, w, h, stride, dev, int(level), C.byref(ex), int(border)))
        self._seed_pixels = keep
        self.refresh()

    def rebuild_labels(self, labels, border=0):
        p, w, h, stride, dev, keep = _pixels(labels, "labels")
        if stride != w:
            keep = keep.contiguous() if dev else np.ascontiguousarray(keep)
            p = C.c_void_p(keep.data_ptr() if dev else keep.ctypes.data)
        capi.check(capi.lib().fdcm_featuremap_rebuild_labels(self._h, p, w, h, dev, int(border)))
        self._seed_pixels = keep
        self.refresh()

    def slice(self, k):
        """Slice k as an (H, W) array (column-major in memory, as the reference's RawImage)."""
        out = np.zeros((self.width, self.height), dtype=np.float32)
        capi.check(capi.lib().fdcm_featuremap_slice(self._h, int(k), capi.fptr(out)))
        return out.T

    def volume(self):
        """(depth, W, H) float32 copy of the device volume, [k][x][y]."""
        out = np.zeros((self.depth, self.width, self.height), dtype=np.float32)
        for k in range(self.depth):
            capi.check(capi.lib().fdcm_featuremap_slice(self._h, k, capi.fptr(out[k])))
        return out

    def device_pointer(self):
        """Address of the volume in HBM; layout: element k * device_slice_stride() + ((x // 4) * H + y) * 4 + x % 4."""
        p = C.c_void_p()
        capi.check(capi.lib().fdcm_featuremap_device_volume(self._h, C.byref(p)))
        return p.value

    def device_slice_stride(self):
        n = C.c_int64()
        capi.check(capi.lib().fdcm_featuremap_device_volume_stride(self._h, C.byref(n)))
        return n.value

    def minmax_translation(self, tmpl, align_vec):
        """FeatureMap::minmaxTranslation (featuremap.h:113-115 -> dt3cpu.cpp:30-75,119-124): (negative, positive)
        multiplier limits of align_vec for the (4, N) template; runs on the device."""
        rec = capi.as_records(tmpl)
        av = np.ascontiguousarray(align_vec, dtype=np.float32).reshape(2)
        out = np.zeros(2, dtype=np.float32)
        capi.check(capi.lib().fdcm_featuremap_minmax_translation(self._h, capi.fptr(rec), rec.shape[0], capi.fptr(av),
                                                                 capi.fptr(out)))
        return out

    def minmax_translation_batch(self, templates, align_vecs):
        """One launch for a list of templates with one align vector each -> (T, 2) float32."""
        flat, offsets = capi.pack_templates(templates)
        av = np.ascontiguousarray(align_vecs, dtype=np.float32).reshape(len(offsets) - 1, 2)
        out = np.zeros((len(offsets) - 1, 2), dtype=np.float32)
        capi.check(capi.lib().fdcm_featuremap_minmax_translation_batch(
            self._h, capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)), len(offsets) - 1, capi.fptr(av),
            capi.fptr(out)))
        return out

    def evaluate(self, templates, translations):
        """FeatureMap::evaluate (featuremap.h:117-120 -> dt3cpu.cpp:126-179): templates = list of (4, N) arrays,
        translations = per template a list / (n, 2) array of (x, y); returns a list of float32 arrays.  One launch."""
        flat, offsets = capi.pack_templates(templates)
        if len(translations) != len(offsets) - 1:
            raise ValueError("one list of translations per template is required")
        trs = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 2) for t in translations]
        toff = np.zeros(len(trs) + 1, dtype=np.int64)
        for i, t in enumerate(trs):
            toff[i + 1] = toff[i] + t.shape[0]
        tflat = np.ascontiguousarray(np.concatenate(trs, axis=0)) if trs and toff[-1] else np.zeros((0, 2), dtype=np.float32)
        scores = np.zeros(int(toff[-1]), dtype=np.float32)
        capi.check(capi.lib().fdcm_featuremap_evaluate(
            self._h, capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)), len(offsets) - 1, capi.fptr(tflat),
            toff.ctypes.data_as(C.POINTER(C.c_int64)), capi.fptr(scores)))
        return [scores[toff[i]:toff[i + 1]].copy() for i in range(len(trs))]

    # ---- exhaustive translation search (include/fdcm.h): grids are capi.Grid or (x0, y0, nx, ny, sx, sy)
    def exhaustive_window(self, templates, sx=1, sy=1):
        """The smallest grid with strides (sx, sy), origin a multiple of them, that holds every admissible integer
        translation of every template with lines (nx = ny = 0: none).  templates: DeviceTemplates."""
        g = capi.Grid()
        capi.check(capi.lib().fdcm_exhaustive_window(self._h, templates._h, int(sx), int(sy), C.byref(g)))
        return g

    def exhaustive_search(self, templates, grid, k=1, tmpl_index_base=0):
        """Per template with lines: its k best admissible grid points by (score, grid index), as raw match records
        (capi.MATCH_DTYPE) with transform [1, 0, tx, 0, 1, ty]."""
        g = as_grid(grid)
        out, n = C.c_void_p(), C.c_int64()
        capi.check(capi.lib().fdcm_search_exhaustive(self._h, templates._h, C.byref(g), int(k), int(tmpl_index_base),
                                                     C.byref(out), C.byref(n)))
        return _adopt_matches(out, n.value)

    def exhaustive_peaks(self, templates, grid, k=1, rx=0, ry=0, tmpl_index_base=0):
        """Per template with lines: its k best peaks by (score, grid index), a peak being an admissible grid point whose key
        is the minimum of its (2 rx + 1) x (2 ry + 1) window (0 <= rx, ry <= 32, grid steps), as raw match records
        (capi.MATCH_DTYPE) with transform [1, 0, tx, 0, 1, ty].  rx = ry = 0 is exhaustive_search."""
        g = as_grid(grid)
        out, n = C.c_void_p(), C.c_int64()
        capi.check(capi.lib().fdcm_search_exhaustive_peaks(self._h, templates._h, C.byref(g), int(k), int(rx), int(ry),
                                                           int(tmpl_index_base), C.byref(out), C.byref(n)))
        return _adopt_matches(out, n.value)

    # ---- rotations (include/fdcm.h, "Rotations"): cs (n, 2) float32 pairs (c, s); pivots (T, 2) float32 or None (origin)
    def exhaustive_rotations_window(self, templates, cs, pivots=None, sx=1, sy=1):
        """The smallest grid with strides (sx, sy), origin a multiple of them, that holds every admissible integer
        translation of every (template with lines, rotation)."""
        rot, keep = _rotations(cs, pivots, templates.count)
        g = capi.Grid()
        capi.check(capi.lib().fdcm_exhaustive_rotations_window(self._h, templates._h, C.byref(rot), int(sx), int(sy),
                                                               C.byref(g)))
        return g

    def exhaustive_rotation_search(self, templates, grid, cs, pivots=None, k=1, rx=0, ry=0, ra=0, wrap=False,
                                   tmpl_index_base=0):
        """Per template with lines: its k best peaks over (rotation, grid point) by (score, rotation, grid index), the
        window (2 ra + 1) rotations (circular with wrap) x (2 ry + 1) x (2 rx + 1) grid points, as raw match records with
        transform [c, -s, m.x + tx, s, c, m.y + ty].  rx = ry = ra = 0 is the top-k over all (rotation, point) pairs."""
        rot, keep = _rotations(cs, pivots, templates.count)
        g = as_grid(grid)
        out, n = C.c_void_p(), C.c_int64()
        capi.check(capi.lib().fdcm_search_exhaustive_rotations(self._h, templates._h, C.byref(rot), C.byref(g), int(k),
                                                               int(rx), int(ry), int(ra), int(bool(wrap)),
                                                               int(tmpl_index_base), C.byref(out), C.byref(n)))
        return _adopt_matches(out, n.value)

    def exhaustive_window_search(self, templates, jobs, cs=None, pivots=None, sx=1, sy=1, wrap=False, k=1, tmpl_index_base=0):
        """Pose windows (include/fdcm.h): jobs (n, 7) int32 rows (tmpl, a0, na, x0, y0, nx, ny), each one template, a run of
        the rotations cs and a translation grid of its own with strides (sx, sy).  Per job, in the order given, its k best
        (run position, grid point) by (score, position, grid index).  cs None: translations only (a0 = 0, na = 1).
        Returns (raw match records, int64 offsets of n + 1: job j's records are offsets[j] .. offsets[j + 1])."""
        jobs = as_pose_windows(jobs)
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        out, n = C.c_void_p(), C.c_int64()
        offsets = np.zeros(jobs.shape[0] + 1, dtype=np.int64)
        capi.check(capi.lib().fdcm_search_exhaustive_windows(
            self._h, templates._h, C.byref(rot) if rot is not None else None, jobs.ctypes.data_as(C.POINTER(capi.PoseWindow)),
            jobs.shape[0], int(sx), int(sy), int(bool(wrap)), int(k), int(tmpl_index_base), C.byref(out), C.byref(n),
            offsets.ctypes.data_as(C.POINTER(C.c_int64))))
        return _adopt_matches(out, n.value), offsets

    def exhaustive_detect_windows(self, templates, jobs, cs=None, pivots=None, sx=1, sy=1, wrap=False, max_score=float("inf"),
                                  max_detections=1024, overlap_permille=300, margin=0, penalty=None, tau=1.0, min_matched=None,
                                  tmpl_index_base=0, boxes=False, matched=False, job_index=False, gate="winner"):
        """Detections over pose windows (include/fdcm.h): every job of exhaustive_window_search gives its best pose (k = 1);
        the best poses, normalised by the penalty, at most max_score and with at least min_matched of their line length
        matched, go through exhaustive_detect_all's greedy rule by footprint overlap, keyed by (score, job).  Raw match
        records in ascending order; with boxes the (n, 4) int32 footprints, with matched the (n,) float32 fractions, with
        job_index the (n,) int32 job of each record, in that order.  gate "all" ("Gate inside the minimum"): a job's best pose
        is the best among its poses that pass min_matched, not the best pose whatever it matches."""
        kind = gate_kind(gate)
        jobs = as_pose_windows(jobs)
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        out, n = C.c_void_p(), C.c_int64()
        md = int(max_detections) if 1 <= int(max_detections) <= 4096 else 0
        fp = np.zeros((md, 4), dtype=np.int32)
        fr = np.zeros(md, dtype=np.float32)
        ji = np.zeros(md, dtype=np.int32)
        head = (self._h, templates._h, C.byref(rot) if rot is not None else None, jobs.ctypes.data_as(C.POINTER(capi.PoseWindow)),
                jobs.shape[0], int(sx), int(sy), int(bool(wrap)), float(max_score), int(max_detections), int(overlap_permille),
                int(margin), -1 if penalty is None else int(penalty), float(tau), 0.0 if min_matched is None else float(min_matched))
        tail = (int(tmpl_index_base), C.byref(out), C.byref(n), fp.ctypes.data_as(C.POINTER(C.c_int32)) if boxes and md else None,
                capi.fptr(fr) if matched and md else None, ji.ctypes.data_as(C.POINTER(C.c_int32)) if job_index and md else None)
        if kind == capi.GATE_WINNER:
            capi.check(capi.lib().fdcm_search_exhaustive_detect_windows(*head, *tail))
        else:
            capi.check(capi.lib().fdcm_search_exhaustive_detect_windows_gated(*head, kind, *tail))
        res = (_adopt_matches(out, n.value),) + ((fp[:n.value].copy(),) if boxes else ()) + ((fr[:n.value].copy(),) if matched else ())
        res += (ji[:n.value].copy(),) if job_index else ()
        return res if len(res) > 1 else res[0]

    # ---- best map and detections (include/fdcm.h, "Best map and detections"): cs None is the translations alone
    def best_map(self, templates, grid, cs=None, pivots=None, penalty=None, tau=1.0, min_matched=None, matched=False):
        """(scores, pairs): per grid point the lowest length-normalised score over all templates with lines and all
        rotations, (ny, nx) float32 with NaN where no pair is admissible, and the pair t * n + a that gave it, (ny, nx)
        int32 with -1 there.  penalty: None, capi.DEFAULT_PENALTY or capi.EXPONENTIAL_PENALTY (with tau).  min_matched (0 to 1)
        or matched: the gated best map (include/fdcm.h, "Gate inside the minimum"): only pairs with at least min_matched of
        their line length matched at the point compete, and with matched the (ny, nx) float32 fractions of the winning
        pairs, NaN where there is none, come last: (scores, pairs, fractions)."""
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        g = as_grid(grid)
        scores = np.empty((g.ny, g.nx), dtype=np.float32)
        pairs = np.empty((g.ny, g.nx), dtype=np.int32)
        if min_matched is not None or matched:
            frac = np.empty((g.ny, g.nx), dtype=np.float32)
            capi.check(capi.lib().fdcm_best_map_gated(
                self._h, templates._h, C.byref(rot) if rot is not None else None, C.byref(g), -1 if penalty is None else int(penalty),
                float(tau), 0.0 if min_matched is None else float(min_matched), capi.fptr(scores),
                pairs.ctypes.data_as(C.POINTER(C.c_int32)), capi.fptr(frac) if matched else None))
            return (scores, pairs, frac) if matched else (scores, pairs)
        capi.check(capi.lib().fdcm_best_map(self._h, templates._h, C.byref(rot) if rot is not None else None, C.byref(g),
                                            -1 if penalty is None else int(penalty), float(tau), capi.fptr(scores),
                                            pairs.ctypes.data_as(C.POINTER(C.c_int32))))
        return scores, pairs

    def exhaustive_detect(self, templates, grid, cs=None, pivots=None, k=8, rx=0, ry=0, penalty=None, tau=1.0, tmpl_index_base=0):
        """The detections: the first k peaks of best_map's score plane by (score, grid index), a peak being a point whose
        key is the minimum of its (2 rx + 1) x (2 ry + 1) window, as raw match records of the winning (template, rotation)
        with the normalised score, in ascending order."""
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        g = as_grid(grid)
        out, n = C.c_void_p(), C.c_int64()
        capi.check(capi.lib().fdcm_search_exhaustive_detect(
            self._h, templates._h, C.byref(rot) if rot is not None else None, C.byref(g), int(k), int(rx), int(ry),
            -1 if penalty is None else int(penalty), float(tau), int(tmpl_index_base), C.byref(out), C.byref(n)))
        return _adopt_matches(out, n.value)

    def exhaustive_detect_nms(self, templates, grid, cs=None, pivots=None, k=8, overlap_permille=300, margin=0, penalty=None,
                              tau=1.0, tmpl_index_base=0, boxes=False):
        """Detections by footprint overlap (include/fdcm.h): greedily the point of the smallest best-map key, then without
        every point whose footprint (the winning pair's box of line end points, widened by margin pixels, at the point's
        translation) overlaps the detection's by more than overlap_permille / 1000 of their union; at most k.  Raw match
        records as exhaustive_detect's, in ascending order; with boxes also the (n, 4) int32 footprints x0, y0, x1, y1."""
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        g = as_grid(grid)
        out, n = C.c_void_p(), C.c_int64()
        fp = np.zeros((int(k) if 1 <= int(k) <= 64 else 0, 4), dtype=np.int32)
        capi.check(capi.lib().fdcm_search_exhaustive_detect_nms(
            self._h, templates._h, C.byref(rot) if rot is not None else None, C.byref(g), int(k), int(overlap_permille), int(margin),
            -1 if penalty is None else int(penalty), float(tau), int(tmpl_index_base), C.byref(out),
            fp.ctypes.data_as(C.POINTER(C.c_int32)) if boxes and fp.size else None, C.byref(n)))
        rec = _adopt_matches(out, n.value)
        return (rec, fp[:n.value].copy()) if boxes else rec

    def exhaustive_detect_all(self, templates, grid, cs=None, pivots=None, max_score=float("inf"), max_detections=1024,
                              overlap_permille=300, margin=0, penalty=None, tau=1.0, tmpl_index_base=0, boxes=False,
                              min_matched=None, matched=False, gate="winner"):
        """All detections below a score (include/fdcm.h): exhaustive_detect_nms' greedy rule on the points whose normalised
        score is at most max_score, until they run out or max_detections (1 to 4096) is reached.  Raw match records in
        ascending order; with boxes also the (n, 4) int32 footprints.  min_matched (0 to 1) or matched: the call by matched
        fraction (include/fdcm.h, "Detections by matched fraction"): points whose best pair has less than min_matched of its
        line length matched are dropped before the greedy rule, and with matched the (n,) float32 fractions of the records
        come last in the returned tuple.  gate "all" ("Gate inside the minimum"): a point's best pair is the best among its
        pairs that pass min_matched there, and no point is dropped afterwards."""
        kind = gate_kind(gate)
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        g = as_grid(grid)
        out, n = C.c_void_p(), C.c_int64()
        md = int(max_detections) if 1 <= int(max_detections) <= 4096 else 0
        fp = np.zeros((md, 4), dtype=np.int32)
        fp_arg = fp.ctypes.data_as(C.POINTER(C.c_int32)) if boxes and fp.size else None
        if min_matched is None and not matched:
            capi.check(capi.lib().fdcm_search_exhaustive_detect_all(
                self._h, templates._h, C.byref(rot) if rot is not None else None, C.byref(g), float(max_score), int(max_detections),
                int(overlap_permille), int(margin), -1 if penalty is None else int(penalty), float(tau), int(tmpl_index_base),
                C.byref(out), C.byref(n), fp_arg))
            rec = _adopt_matches(out, n.value)
            return (rec, fp[:n.value].copy()) if boxes else rec
        fr = np.zeros(md, dtype=np.float32)
        head = (self._h, templates._h, C.byref(rot) if rot is not None else None, C.byref(g), float(max_score), int(max_detections),
                int(overlap_permille), int(margin), -1 if penalty is None else int(penalty), float(tau),
                0.0 if min_matched is None else float(min_matched))
        tail = (int(tmpl_index_base), C.byref(out), C.byref(n), fp_arg, capi.fptr(fr) if matched and fr.size else None)
        if kind == capi.GATE_WINNER:
            capi.check(capi.lib().fdcm_search_exhaustive_detect_all_matched(*head, *tail))
        else:
            capi.check(capi.lib().fdcm_search_exhaustive_detect_all_gated(*head, kind, *tail))
        res = (_adopt_matches(out, n.value),) + ((fp[:n.value].copy(),) if boxes else ()) + ((fr[:n.value].copy(),) if matched else ())
        return res if len(res) > 1 else res[0]

    # ---- objects (include/fdcm.h, "Objects"): a best pair per (grid point, object), thresholds per object
    def best_map_objects(self, templates, grid, objects, n_objects=None, cs=None, pivots=None, penalty=None, tau=1.0, min_matched=None,
                         matched=False):
        """(scores, pairs) as best_map's, one plane per object: (G, ny, nx) float32 and int32, plane o the best map of the
        templates with objects[t] == o (NaN and -1 where none is a candidate; an object without templates has an empty
        plane).  min_matched: None, a scalar or one value per object, the gate inside the minimum per object.  matched: also
        the (G, ny, nx) float32 fractions of the winning pairs."""
        obj, G, _, mm = object_arrays(objects, n_objects, templates.count, None, min_matched)
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        g = as_grid(grid)
        shape = (G if 1 <= G <= 256 else 0, g.ny, g.nx)
        scores, pairs = np.empty(shape, dtype=np.float32), np.empty(shape, dtype=np.int32)
        frac = np.empty(shape, dtype=np.float32) if matched else None
        capi.check(capi.lib().fdcm_best_map_objects(
            self._h, templates._h, C.byref(rot) if rot is not None else None, C.byref(g), -1 if penalty is None else int(penalty),
            float(tau), obj.ctypes.data_as(C.POINTER(C.c_int32)), G, capi.fptr(mm) if mm is not None else None, capi.fptr(scores),
            pairs.ctypes.data_as(C.POINTER(C.c_int32)), capi.fptr(frac) if matched else None))
        return (scores, pairs, frac) if matched else (scores, pairs)

    def exhaustive_detect_objects(self, templates, grid, objects, max_score=float("inf"), n_objects=None, cs=None, pivots=None,
                                  max_detections=1024, overlap_permille=300, cross_permille=None, margin=0, penalty=None, tau=1.0,
                                  min_matched=None, tmpl_index_base=0, boxes=False, matched=False, gate="winner"):
        """exhaustive_detect_all with objects (include/fdcm.h, "Objects"): the entries are (grid point, object), each with the
        best pair among its object's templates; max_score and min_matched are a scalar or one value per object; a detection
        drops an entry of its own object above overlap_permille and one of another object above cross_permille (None: the
        same limit).  Raw match records in ascending order, then with boxes the (n, 4) int32 footprints and with matched
        the (n,) float32 fractions."""
        kind = gate_kind(gate)
        obj, G, ms, mm = object_arrays(objects, n_objects, templates.count, max_score, min_matched)
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        g = as_grid(grid)
        out, n = C.c_void_p(), C.c_int64()
        md = int(max_detections) if 1 <= int(max_detections) <= 4096 else 0
        fp = np.zeros((md, 4), dtype=np.int32)
        fr = np.zeros(md, dtype=np.float32)
        capi.check(capi.lib().fdcm_search_exhaustive_detect_objects(
            self._h, templates._h, C.byref(rot) if rot is not None else None, C.byref(g), obj.ctypes.data_as(C.POINTER(C.c_int32)), G,
            capi.fptr(ms), capi.fptr(mm) if mm is not None else None, int(max_detections), int(overlap_permille),
            int(overlap_permille if cross_permille is None else cross_permille), int(margin), -1 if penalty is None else int(penalty),
            float(tau), kind, int(tmpl_index_base), C.byref(out), C.byref(n),
            fp.ctypes.data_as(C.POINTER(C.c_int32)) if boxes and md else None, capi.fptr(fr) if matched and md else None))
        res = (_adopt_matches(out, n.value),) + ((fp[:n.value].copy(),) if boxes else ()) + ((fr[:n.value].copy(),) if matched else ())
        return res if len(res) > 1 else res[0]

    def exhaustive_detect_windows_objects(self, templates, jobs, objects, max_score=float("inf"), n_objects=None, cs=None, pivots=None,
                                          sx=1, sy=1, wrap=False, max_detections=1024, overlap_permille=300, cross_permille=None,
                                          margin=0, penalty=None, tau=1.0, min_matched=None, tmpl_index_base=0, boxes=False,
                                          matched=False, job_index=False, gate="winner"):
        """exhaustive_detect_windows with objects (include/fdcm.h, "Objects"): a job's object is its template's; its threshold
        and its need are that object's, and the greedy rule uses overlap_permille between jobs of one object and
        cross_permille (None: the same) between jobs of different objects.  The outputs are exhaustive_detect_windows'."""
        kind = gate_kind(gate)
        obj, G, ms, mm = object_arrays(objects, n_objects, templates.count, max_score, min_matched)
        jobs = as_pose_windows(jobs)
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        out, n = C.c_void_p(), C.c_int64()
        md = int(max_detections) if 1 <= int(max_detections) <= 4096 else 0
        fp = np.zeros((md, 4), dtype=np.int32)
        fr = np.zeros(md, dtype=np.float32)
        ji = np.zeros(md, dtype=np.int32)
        capi.check(capi.lib().fdcm_search_exhaustive_detect_windows_objects(
            self._h, templates._h, C.byref(rot) if rot is not None else None, jobs.ctypes.data_as(C.POINTER(capi.PoseWindow)),
            jobs.shape[0], int(sx), int(sy), int(bool(wrap)), obj.ctypes.data_as(C.POINTER(C.c_int32)), G, capi.fptr(ms),
            capi.fptr(mm) if mm is not None else None, int(max_detections), int(overlap_permille),
            int(overlap_permille if cross_permille is None else cross_permille), int(margin), -1 if penalty is None else int(penalty),
            float(tau), kind, int(tmpl_index_base), C.byref(out), C.byref(n),
            fp.ctypes.data_as(C.POINTER(C.c_int32)) if boxes and md else None, capi.fptr(fr) if matched and md else None,
            ji.ctypes.data_as(C.POINTER(C.c_int32)) if job_index and md else None))
        res = (_adopt_matches(out, n.value),) + ((fp[:n.value].copy(),) if boxes else ()) + ((fr[:n.value].copy(),) if matched else ())
        res += (ji[:n.value].copy(),) if job_index else ()
        return res if len(res) > 1 else res[0]

    def matched_fractions(self, templates, poses, cs=None, pivots=None):
        """Matched fractions (include/fdcm.h, "Detections by matched fraction"): per pose (tmpl, a, x, y), as line_costs takes
        them, the float32 share of the template's line length whose lines cost at most their caps there; 1 for a template
        whose lengths sum to 0, NaN for a pose that is not admissible.  (n,) float32."""
        poses = as_poses(poses)
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        out = np.zeros(poses.shape[0], dtype=np.float32)
        capi.check(capi.lib().fdcm_matched_fractions(self._h, templates._h, C.byref(rot) if rot is not None else None,
                                                     poses.ctypes.data_as(C.POINTER(C.c_int32)), poses.shape[0],
                                                     capi.fptr(out) if out.size else None))
        return out

    def line_costs(self, templates, poses, cs=None, pivots=None):
        """Line costs (include/fdcm.h, "Per-line caps and line costs"): poses (n, 4) int32 rows (tmpl, a, x, y), a an index
        into the rotations cs (0 with cs None, the lines as they are).  Returns (float32 costs, int64 offsets of n + 1): pose
        q's floats are costs[offsets[q]:offsets[q + 1]], the uncapped cost of every line of its template in line order, NaN
        throughout when the pose is not admissible."""
        poses = as_poses(poses)
        rot, keep = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        out = C.POINTER(C.c_float)()
        offsets = np.zeros(poses.shape[0] + 1, dtype=np.int64)
        capi.check(capi.lib().fdcm_line_costs(self._h, templates._h, C.byref(rot) if rot is not None else None,
                                              poses.ctypes.data_as(C.POINTER(C.c_int32)), poses.shape[0], C.byref(out),
                                              offsets.ctypes.data_as(C.POINTER(C.c_int64))))
        try:
            n = int(offsets[-1])
            return (np.ctypeslib.as_array(out, shape=(n,)).copy() if n else np.zeros(0, dtype=np.float32)), offsets
        finally:
            capi.lib().fdcm_lines_free(out)

    # ---- match lists (include/fdcm.h, "Match lists"): the records of search(), verified and suppressed on the device
    def _match_input(self, matches, device_ptr, n):
        """(pointer, n, on_device, the array kept alive) of the three forms: host records, a device buffer, the last search."""
        if device_ptr:
            return C.c_void_p(int(device_ptr)), int(n), 1, None
        if matches is None:
            return None, int(getattr(self, "last_search_count", 0)), 0, None
        rec = match_records(matches)
        return (C.c_void_p(rec.ctypes.data) if rec.shape[0] else None), rec.shape[0], 0, rec

    @staticmethod
    def _detect_outputs(max_detections, indices, boxes, matched):
        """The outputs of a detect call on a match list: (out, k) for the records, the optional arrays' pointers in the C
        order (None where not asked for) and result(), the method's return value after the call."""
        out, k = C.c_void_p(), C.c_int64()
        md = int(max_detections) if 1 <= int(max_detections) <= 4096 else 0  # (an argument out of range is the library's to refuse)
        ji = np.zeros(md, dtype=np.int32)
        fp = np.zeros((md, 4), dtype=np.int32)
        fr = np.zeros(md, dtype=np.float32)
        optional = (ji.ctypes.data_as(C.POINTER(C.c_int32)) if indices and md else None,
                    fp.ctypes.data_as(C.POINTER(C.c_int32)) if boxes and md else None, capi.fptr(fr) if matched and md else None)

        def result():
            res = (_adopt_matches(out, k.value),) + ((ji[:k.value].copy(),) if indices else ()) + ((fp[:k.value].copy(),) if boxes else ())
            res += (fr[:k.value].copy(),) if matched else ()
            return res if len(res) > 1 else res[0]
        return out, k, optional, result

    def verify_matches(self, templates, matches=None, tmpl_index_base=0, device_ptr=None, n=0):
        """fdcm_matches_verify: (scores, fractions, costs) of every record: s(r) and frac(r) as (n,) float32 and the uncapped
        line costs as an (n, Lmax) float32 array, NaN beyond a template's line count, all NaN for a record that is invalid or
        not admissible.  matches: a MatchList or record array on the host; None: the records of the last search_raw on this
        map; device_ptr, n: records in device memory (search_into)."""
        ptr, n, on_device, keep = self._match_input(matches, device_ptr, n)
        lmax = templates.max_lines
        nan = np.float32(np.nan)
        s, f, c = np.full(n, nan, dtype=np.float32), np.full(n, nan, dtype=np.float32), np.full((n, lmax), nan, dtype=np.float32)
        capi.check(capi.lib().fdcm_matches_verify(self._h, templates._h, ptr, n, on_device, int(tmpl_index_base), capi.fptr(s),
                                                  capi.fptr(f), capi.fptr(c)))
        return s, f, c

    def detect_matches(self, templates, matches=None, max_score=float("inf"), overlap_permille=300, max_detections=1024, penalty=None,
                       tau=1.0, margin=0, min_matched=None, rescore=False, tmpl_index_base=0, indices=False, boxes=False,
                       matched=False, device_ptr=None, n=0):
        """fdcm_matches_detect: the greedy rule by footprint overlap on a match list, keyed by (q, position): raw match records
        in ascending order with q for their score; with indices the (k,) int32 positions in the list, with boxes the (k, 4)
        int32 footprints, with matched the (k,) float32 fractions, in that order.  The forms of matches are verify_matches'."""
        ptr, n, on_device, keep = self._match_input(matches, device_ptr, n)
        out, k, optional, result = self._detect_outputs(max_detections, indices, boxes, matched)
        capi.check(capi.lib().fdcm_matches_detect(
            self._h, templates._h, ptr, n, on_device, int(tmpl_index_base), float(max_score), int(max_detections), int(overlap_permille),
            int(margin), -1 if penalty is None else int(penalty), float(tau), 0.0 if min_matched is None else float(min_matched),
            int(bool(rescore)), C.byref(out), C.byref(k), *optional))
        return result()

    def refine_matches(self, templates, matches=None, cs=None, pivots=None, centre=None, hx=0, hy=0, sx=1, sy=1, tmpl_index_base=0,
                       poses=False, device_ptr=None, n=0, out_device_ptr=None):
        """fdcm_matches_refine (include/fdcm.h, "Match lists: refinement"): every record searched in its own window of the
        delta rotations cs ((na, 2) float32 (c, s); None: nothing rotated), about pivots in template coordinates, and the
        translations (i sx, j sy), |i| <= hx, |j| <= hy, and replaced by its best pose; a record without one keeps its
        transform and scores NaN.  centre: the run position of the unrotated delta, -1 for none; None: the first (1, 0) of cs,
        else -1 (0 with cs None).  Returns the raw records aligned with the input, with poses also the (n, 3) int32 rows
        (e, i, j), (-1, 0, 0) without a winner.  The forms of matches are verify_matches'; out_device_ptr: the records go to
        that device buffer (it may be device_ptr: in place) and the return value holds None in their place."""
        ptr, n, on_device, keep = self._match_input(matches, device_ptr, n)
        rot, keep_rot = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        if centre is None:
            centre = 0
            if cs is not None:
                unit = np.flatnonzero(np.all(keep_rot[0] == np.float32([1, 0]), axis=1))
                centre = int(unit[0]) if unit.size else -1
        out = None
        if not out_device_ptr:  # (an empty map or an empty set writes nothing: no record has a winner)
            out = keep.copy() if keep is not None else np.zeros(n, dtype=capi.MATCH_DTYPE)
            out["score"] = np.float32(np.nan)
        pose = np.zeros((n, 3), dtype=np.int32)
        pose[:, 0] = -1
        capi.check(capi.lib().fdcm_matches_refine(
            self._h, templates._h, ptr, n, on_device, int(tmpl_index_base), C.byref(rot) if rot is not None else None, int(centre), int(hx),
            int(hy), int(sx), int(sy), C.c_void_p(int(out_device_ptr)) if out_device_ptr else (C.c_void_p(out.ctypes.data) if n else None),
            1 if out_device_ptr else 0, pose.ctypes.data_as(C.POINTER(C.c_int32)) if poses and n else None))
        return (out, pose) if poses else out

    def detect_matches_objects(self, templates, matches, objects, max_score, n_objects=None, overlap_permille=300, cross_permille=None,
                               max_detections=1024, penalty=None, tau=1.0, margin=0, min_matched=None, rescore=False, tmpl_index_base=0,
                               indices=False, boxes=False, matched=False, device_ptr=None, n=0):
        """fdcm_matches_detect_objects (include/fdcm.h, "Match lists: objects and hull shapes"): detect_matches with objects --
        objects[t] the object of template t, max_score and min_matched a scalar or one value per object, overlap_permille
        between records of one object and cross_permille (None: the same) between records of different objects -- on the
        set's kind of footprint: the box, or for a "hull" set the hull of the posed end points, built on the device.  The
        outputs and the forms of matches are detect_matches'."""
        obj, G, ms, mm = object_arrays(objects, n_objects, templates.count, max_score, min_matched)
        ptr, n, on_device, keep = self._match_input(matches, device_ptr, n)
        out, k, optional, result = self._detect_outputs(max_detections, indices, boxes, matched)
        capi.check(capi.lib().fdcm_matches_detect_objects(
            self._h, templates._h, ptr, n, on_device, int(tmpl_index_base), obj.ctypes.data_as(C.POINTER(C.c_int32)), G,
            capi.fptr(ms) if ms is not None else None, capi.fptr(mm) if mm is not None else None, int(max_detections),
            int(overlap_permille), int(overlap_permille if cross_permille is None else cross_permille), int(margin),
            -1 if penalty is None else int(penalty), float(tau), int(bool(rescore)), C.byref(out), C.byref(k), *optional))
        return result()

    def match_shapes(self, templates, matches, margin=0, tmpl_index_base=0, device_ptr=None, n=0):
        """fdcm_matches_shapes: match_footprint_spans' table from the device kernel, for the records that are valid and
        admissible on this map and whose template has lines; the others have no rows and area 0.  (row_offsets, spans, areas).
        matches: a MatchList or record array on the host, or device_ptr and n."""
        if matches is None and not device_ptr:
            raise ValueError("match_shapes takes host records or device_ptr and n")
        ptr, n, on_device, keep = self._match_input(matches, device_ptr, n)
        return _spans_result(n, 1, lambda off, areas, spans: capi.check(capi.lib().fdcm_matches_shapes(
            self._h, templates._h, ptr, n, on_device, int(tmpl_index_base), int(margin), off, areas, spans)))

    def scene_coverage(self, labels, templates, poses, cs=None, pivots=None, radius=2, bin_tolerance=1, margin=None, residual=False):
        """Scene coverage (include/fdcm.h, "Scene coverage"): per pose (tmpl, a, x, y), as line_costs takes them, the number of
        edge pixels of `labels` in the pose's window (its footprint at `margin`, None: radius) and how many of them the posed
        template explains (within `radius` pixels of one of its segments whose slice is within bin_tolerance of the pixel's).
        (-1, -1) for a pose that is not admissible.  `labels`: 2-D uint8, a numpy array or a contiguous CUDA torch tensor, the
        image this map was built from.  Returns counts, an (n, 2) int32 array, or with residual (counts, residual): the labels
        with 255 at every pixel an admissible pose of the list explains, a tensor on the same device for a tensor."""
        p, w, h, dev, keep, res, q = self._labels_input(labels, residual)
        poses = as_poses(poses)
        rot, keep_rot = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        par = capi.CoverageParams(int(radius), int(bin_tolerance), int(radius if margin is None else margin))
        counts = np.zeros((poses.shape[0], 2), dtype=np.int32)
        capi.check(capi.lib().fdcm_scene_coverage(self._h, p, w, h, dev, templates._h, C.byref(rot) if rot is not None else None,
                                                  poses.ctypes.data_as(C.POINTER(C.c_int32)), poses.shape[0], C.byref(par),
                                                  counts.ctypes.data_as(C.POINTER(C.c_int32)) if counts.size else None, q))
        return (counts, res) if residual else counts

    def scene_select(self, labels, templates, poses, cs=None, pivots=None, radius=2, bin_tolerance=1, margin=None, min_coverage=0.0,
                     min_new=0.5, min_pixels=1, max_selected=1024, residual=False):
        """Scene selection (include/fdcm.h, "Scene selection"): greedy explain-away over the poses (tmpl, a, x, y), the list
        order being the priority.  A pose is a candidate when it is admissible, explains at least min_pixels edge pixels of its
        window and at least the share min_coverage of the window's edge pixels; a candidate is accepted, in order, when at
        least min_pixels and the share min_new of the pixels it explains are not yet claimed by the poses accepted before it,
        and then claims its own; at most max_selected are accepted.  The shares are taken in permille, int(round(1000 * v)).
        labels, templates, cs, pivots, radius, bin_tolerance and margin are scene_coverage's.  Returns (selected, counts): the
        (k,) int32 indices of the accepted poses, ascending, and (k, 3) int32 rows (edges, explained, new), new as at
        acceptance; with residual also the labels with 255 at every claimed pixel, a tensor on the same device for a tensor."""
        p, w, h, dev, keep, res, q = self._labels_input(labels, residual)
        poses = as_poses(poses)
        rot, keep_rot = _rotations(cs, pivots, templates.count) if cs is not None else (None, None)
        par = capi.CoverageParams(int(radius), int(bin_tolerance), int(radius if margin is None else margin))
        sel, outputs, result = self._select_outputs(min_coverage, min_new, min_pixels, max_selected, residual)
        capi.check(capi.lib().fdcm_scene_select(self._h, p, w, h, dev, templates._h, C.byref(rot) if rot is not None else None,
                                                poses.ctypes.data_as(C.POINTER(C.c_int32)), poses.shape[0], C.byref(par), C.byref(sel), *outputs, q))
        return result(res)

    @staticmethod
    def _select_outputs(min_coverage, min_new, min_pixels, max_selected, residual):
        """The rule's parameters and the outputs of a selection call: SelectParams, the pointers of selected, counts and k in
        the C order, and result(res), the method's return value after the call."""
        sel = capi.SelectParams(int(round(1000 * min_coverage)), int(round(1000 * min_new)), int(min_pixels), int(max_selected))
        room = max(1, min(int(max_selected), 4096))          # (an argument out of range is the library's to refuse)
        selected = np.zeros(room, dtype=np.int32)
        counts = np.zeros((room, 3), dtype=np.int32)
        k = C.c_int64(0)
        outputs = (selected.ctypes.data_as(C.POINTER(C.c_int32)), counts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k))

        def result(res):
            got = (selected[:k.value].copy(), counts[:k.value].copy())
            return got + (res,) if residual else got
        return sel, outputs, result

    # ---- the labels of the coverage, selection and fit calls, pose lists and match lists alike
    def _labels_input(self, labels, residual):
        """(pointer, width, height, on_device, kept alive, residual array or tensor, its pointer) of scene coverage's labels."""
        if hasattr(labels, "data_ptr") and not isinstance(labels, np.ndarray) and labels.dim() == 2 and not labels.is_contiguous():
            raise ValueError("labels on the device must be contiguous")
        p, w, h, _, dev, keep = _pixels(labels, "labels")
        if not dev and keep.size and keep.strides[0] != w:
            keep = np.ascontiguousarray(keep)
            p = C.c_void_p(keep.ctypes.data)
        res, q = None, None
        if residual and dev:
            import torch
            res = torch.empty((h, w), dtype=torch.uint8, device=keep.device)
            q = C.c_void_p(res.data_ptr())
        elif residual:
            res = np.empty((h, w), dtype=np.uint8)
            q = C.c_void_p(res.ctypes.data)
        return p, w, h, dev, keep, res, q

    def match_coverage(self, labels, templates, matches=None, radius=2, bin_tolerance=1, margin=None, tmpl_index_base=0, residual=False,
                       device_ptr=None, n=0):
        """fdcm_matches_coverage: scene_coverage for match records, each posed by its own transform.  Returns counts, an (n, 2)
        int32 array of (edges, explained), (-1, -1) for a record that is invalid or not admissible, or with residual (counts,
        residual).  labels, radius, bin_tolerance, margin and the residual are scene_coverage's; the forms of matches are
        verify_matches'."""
        p, w, h, dev, keep, res, q = self._labels_input(labels, residual)
        ptr, n, on_device, keep_rec = self._match_input(matches, device_ptr, n)
        par = capi.CoverageParams(int(radius), int(bin_tolerance), int(radius if margin is None else margin))
        counts = np.zeros((n, 2), dtype=np.int32)
        capi.check(capi.lib().fdcm_matches_coverage(self._h, p, w, h, dev, templates._h, ptr, n, on_device, int(tmpl_index_base),
                                                    C.byref(par), counts.ctypes.data_as(C.POINTER(C.c_int32)) if counts.size else None, q))
        return (counts, res) if residual else counts

    def select_matches(self, labels, templates, matches=None, radius=2, bin_tolerance=1, margin=None, min_coverage=0.0, min_new=0.5,
                       min_pixels=1, max_selected=1024, tmpl_index_base=0, residual=False, device_ptr=None, n=0):
        """fdcm_matches_select: scene_select for match records, the list order being the priority.  Returns (selected, counts):
        the (k,) int32 positions of the accepted records, ascending, and (k, 3) int32 rows (edges, explained, new); with
        residual also the labels with 255 at every claimed pixel.  The rule's parameters are scene_select's, the rest
        match_coverage's."""
        p, w, h, dev, keep, res, q = self._labels_input(labels, residual)
        ptr, n, on_device, keep_rec = self._match_input(matches, device_ptr, n)
        par = capi.CoverageParams(int(radius), int(bin_tolerance), int(radius if margin is None else margin))
        sel, outputs, result = self._select_outputs(min_coverage, min_new, min_pixels, max_selected, residual)
        capi.check(capi.lib().fdcm_matches_select(self._h, p, w, h, dev, templates._h, ptr, n, on_device, int(tmpl_index_base),
                                                  C.byref(par), C.byref(sel), *outputs, q))
        return result(res)

    def fit_matches(self, labels, templates, matches=None, radius=3, bin_tolerance=1, margin=None, iterations=2, min_pixels=8,
                    damping=1e-3, max_shift=None, max_angle=0.1, tmpl_index_base=0, info=False, rms=False, device_ptr=None, n=0,
                    out_device_ptr=None):
        """fdcm_matches_fit (include/fdcm.h, "Match lists: pose fit"): every record's transform fitted by least squares to the
        edge pixels of labels its posed lines explain, in `iterations` closed-form steps on the device.  Returns the raw
        records aligned with the input (tmpl_idx and score unchanged), with info also the (n, 4) int32 rows (status, steps, fit
        pixels at the first pass, at the last) and with rms the (n, 2) float32 rms distances at the first and the last pass.
        max_shift None: the radius.  labels, radius, bin_tolerance, margin and the forms of matches are match_coverage's;
        out_device_ptr: the records go to that device buffer (it may be device_ptr: in place) and the return value holds None
        in their place."""
        p, w, h, dev, keep, _, _ = self._labels_input(labels, False)
        ptr, n, on_device, keep_rec = self._match_input(matches, device_ptr, n)
        par = capi.CoverageParams(int(radius), int(bin_tolerance), int(radius if margin is None else margin))
        fit = capi.FitParams(int(iterations), int(min_pixels), float(damping), float(radius if max_shift is None else max_shift),
                             float(max_angle))
        out = None
        if not out_device_ptr:  # (an empty map or an empty set writes nothing: every record stays as it is, status -1)
            out = keep_rec.copy() if keep_rec is not None else np.zeros(n, dtype=capi.MATCH_DTYPE)
        inf = np.zeros((n, 4), dtype=np.int32)
        inf[:, 0] = -1
        dist = np.full((n, 2), np.nan, dtype=np.float32)
        capi.check(capi.lib().fdcm_matches_fit(
            self._h, p, w, h, dev, templates._h, ptr, n, on_device, int(tmpl_index_base), C.byref(par), C.byref(fit),
            C.c_void_p(int(out_device_ptr)) if out_device_ptr else (C.c_void_p(out.ctypes.data) if n else None), 1 if out_device_ptr else 0,
            inf.ctypes.data_as(C.POINTER(C.c_int32)) if n else None, capi.fptr(dist) if n else None))
        res = (out,) + ((inf,) if info else ()) + ((dist,) if rms else ())
        return res if len(res) > 1 else res[0]

    def rotation_score_map(self, templates, grid, cs, pivots=None):
        """(T, n, ny, nx) float32: the score of every rotated template at every grid point, NaN where not admissible."""
        rot, keep = _rotations(cs, pivots, templates.count)
        g = as_grid(grid)
        out = np.empty((templates.count, rot.n, g.ny, g.nx), dtype=np.float32)
        capi.check(capi.lib().fdcm_score_map_rotations(self._h, templates._h, C.byref(rot), C.byref(g), capi.fptr(out)))
        return out

    def score_map(self, templates, grid):
        """(T, ny, nx) float32: the score of every template at every grid point, NaN where not admissible."""
        g = as_grid(grid)
        out = np.empty((templates.count, g.ny, g.nx), dtype=np.float32)
        capi.check(capi.lib().fdcm_score_map(self._h, templates._h, C.byref(g), capi.fptr(out)))
        return out

    def score_map_into(self, templates, grid, device_ptr):
        """The score map into a device buffer of T * ny * nx floats."""
        g = as_grid(grid)
        capi.check(capi.lib().fdcm_score_map_device(self._h, templates._h, C.byref(g), C.c_void_p(device_ptr)))

    def stage_timing(self, on):
        """Device-side times cost an event between the kernels: True / 1 per-stage times (default), 2 the build's and the
        search's spans only, False / 0 none (build_timing() / search_timing() carry host time and counters only)."""
        capi.check(capi.lib().fdcm_featuremap_stage_timing(self._h, int(on)))

    def build_timing(self):
        t = capi.BuildTiming()
        capi.check(capi.lib().fdcm_featuremap_last_timing(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in t._fields_}

    def search_timing(self):
        t = capi.SearchTiming()
        capi.check(capi.lib().fdcm_search_last_timing(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in t._fields_}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.lib().fdcm_featuremap_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lines_footprints(templates, cs=None, pivots=None, margin=0):
    """DeviceTemplates.footprints for a plain list of line arrays: (T, n, 4) int32, no handle and no device."""
    flat, offsets = capi.pack_templates(templates)
    T = len(offsets) - 1
    rot, keep = _rotations(cs, pivots, T) if cs is not None else (None, None)
    out = np.zeros((T, 1 if rot is None else rot.n, 4), dtype=np.int32)
    capi.check(capi.lib().fdcm_lines_footprints(capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)), T,
                                                C.byref(rot) if rot is not None else None, int(margin),
                                                out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


FOOTPRINT_KINDS = {"box": capi.FOOTPRINT_BOX, "hull": capi.FOOTPRINT_HULL}


def footprint_kind(name):
    """The FDCM_FOOTPRINT_* value of "box" or "hull"; ValueError for anything else."""
    if not isinstance(name, str) or name not in FOOTPRINT_KINDS:
        raise ValueError(f'footprint must be "box" or "hull", got {name!r}')
    return FOOTPRINT_KINDS[name]


def _spans_result(T, n, call):
    """(row_offsets, spans, areas) of a span call: the offsets and areas first, then the spans into an array of that size."""
    off = np.zeros(T * n + 1, dtype=np.int64)
    areas = np.zeros(T * n, dtype=np.int64)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    call(i64(off), i64(areas) if areas.size else None, None)
    spans = np.zeros((int(off[-1]), 2), dtype=np.int32)
    if spans.size:
        call(i64(off), None, spans.ctypes.data_as(C.POINTER(C.c_int32)))
    return off, spans, areas


def lines_footprint_spans(templates, cs=None, pivots=None, margin=0):
    """DeviceTemplates.footprint_spans for a plain list of line arrays: no handle and no device."""
    flat, offsets = capi.pack_templates(templates)
    T = len(offsets) - 1
    rot, keep = _rotations(cs, pivots, T) if cs is not None else (None, None)
    return _spans_result(T, 1 if rot is None else rot.n, lambda off, areas, spans: capi.check(capi.lib().fdcm_lines_footprint_spans(
        capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)), T, C.byref(rot) if rot is not None else None, int(margin), off,
        areas, spans)))


def match_footprint_spans(templates, matches, margin=0, tmpl_index_base=0):
    """fdcm_matches_footprint_spans: the hull shape of every record of a match list (include/fdcm.h, "Match lists: objects and
    hull shapes"), whatever the set's kind: (row_offsets, spans, areas) in lines_footprint_spans' layout with one shape per
    record, row r of record j at y = y0 of match_footprints()[j] + (r - row_offsets[j]); no rows for an invalid record.  Host
    only.  templates: a DeviceTemplates."""
    rec = match_records(matches)
    ptr = C.c_void_p(rec.ctypes.data) if rec.shape[0] else None
    return _spans_result(rec.shape[0], 1, lambda off, areas, spans: capi.check(capi.lib().fdcm_matches_footprint_spans(
        templates._h, ptr, rec.shape[0], int(tmpl_index_base), int(margin), off, areas, spans)))


class DeviceTemplates:
    """Owns an fdcm_templates handle: a list of LineArrays resident in HBM.  line_caps (None, a scalar tau or one float
    array per template: flat_line_caps) gives every line a cap of its cost in the exhaustive calls (include/fdcm.h, "Per-line
    caps and line costs"); search() and the rest of the reference path ignore it.  footprint ("box" or "hull": include/fdcm.h,
    "Hull footprints") is the shape the detection calls with an overlap give the set's pairs; every other call ignores it."""

    def __init__(self, templates, line_caps=None, _packed=None, _caps=None, footprint="box"):
        kind = footprint_kind(footprint)
        flat, offsets = _packed if _packed is not None else capi.pack_templates(templates)
        self.count = len(offsets) - 1
        self.n_lines = int(offsets[-1])
        caps = _caps if _caps is not None else flat_line_caps(templates, line_caps, np.diff(offsets).tolist())
        h = C.c_void_p()
        if kind != capi.FOOTPRINT_BOX:
            capi.check(capi.lib().fdcm_templates_create_shaped(capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)), self.count,
                                                               capi.fptr(caps) if caps is not None else None, kind, C.byref(h)))
        elif caps is None:
            capi.check(capi.lib().fdcm_templates_create(capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                                        self.count, C.byref(h)))
        else:
            capi.check(capi.lib().fdcm_templates_create_capped(capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                                               self.count, capi.fptr(caps), C.byref(h)))
        self._h = h
        self._offsets = np.array(offsets, dtype=np.int64)

    @property
    def max_lines(self):
        """The set's largest line count (0 for an empty set): the row length of verify_matches' costs."""
        return int(np.diff(self._offsets).max()) if self.count else 0

    def line_caps(self):
        """One float32 array of caps per template (+inf: no cap)."""
        out = np.zeros(self.n_lines, dtype=np.float32)
        capi.check(capi.lib().fdcm_templates_line_caps(self._h, capi.fptr(out)))
        return [out[a:b] for a, b in zip(self._offsets[:-1], self._offsets[1:])]

    def line_lengths(self):
        """One float32 array per template: the lengths of its lines as the handle holds them."""
        out = np.zeros(self.n_lines, dtype=np.float32)
        capi.check(capi.lib().fdcm_templates_line_lengths(self._h, capi.fptr(out)))
        return [out[a:b] for a, b in zip(self._offsets[:-1], self._offsets[1:])]

    @property
    def footprint(self):
        """"box" or "hull": the set's kind of footprint (fdcm_templates_footprint_kind)."""
        kind = C.c_int32()
        capi.check(capi.lib().fdcm_templates_footprint_kind(self._h, C.byref(kind)))
        return {v: k for k, v in FOOTPRINT_KINDS.items()}[kind.value]

    def footprint_spans(self, cs=None, pivots=None, margin=0):
        """The hull shapes of every (template, rotation) pair u = t n + a, whatever the set's kind: (row_offsets, spans, areas).
        Pair u has the rows row_offsets[u] .. row_offsets[u + 1] of spans, row r at y = y0 of footprints()[u] + (r -
        row_offsets[u]), its pixels xl .. xr in the frame of that box, (0, -1) when the row is empty.  Host only."""
        rot, keep = _rotations(cs, pivots, self.count) if cs is not None else (None, None)
        return _spans_result(self.count, 1 if rot is None else rot.n, lambda off, areas, spans: capi.check(
            capi.lib().fdcm_templates_footprint_spans(self._h, C.byref(rot) if rot is not None else None, int(margin), off, areas, spans)))

    def footprints(self, cs=None, pivots=None, margin=0):
        """(T, n, 4) int32 footprints x0, y0, x1, y1 of every (template, rotation) pair (n = 1 with cs None: the lines as
        they are), as exhaustive_detect_nms uses them; (0, 0, -1, -1) for a template without lines.  Host only."""
        rot, keep = _rotations(cs, pivots, self.count) if cs is not None else (None, None)
        n = 1 if rot is None else rot.n
        out = np.zeros((self.count, n, 4), dtype=np.int32)
        capi.check(capi.lib().fdcm_templates_footprints(self._h, C.byref(rot) if rot is not None else None, int(margin),
                                                        out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def matched_totals(self):
        """Per template the float32 sum of its line lengths in line order (fdcm_templates_matched_totals): the denominator
        of the matched fraction.  Host only."""
        out = np.zeros(self.count, dtype=np.float32)
        capi.check(capi.lib().fdcm_templates_matched_totals(self._h, capi.fptr(out) if out.size else None))
        return out

    def score_bounds(self, max_score, penalty=None, tau=1.0):
        """Per template the largest float32 sum whose normalised score is <= max_score (fdcm_detect_score_bounds); 0 for a
        template without lines.  Host only."""
        out = np.zeros(self.count, dtype=np.float32)
        capi.check(capi.lib().fdcm_detect_score_bounds(self._h, -1 if penalty is None else int(penalty), float(tau), float(max_score),
                                                       capi.fptr(out)))
        return out

    def lengths(self):
        out = np.zeros(self.count, dtype=np.float32)
        capi.check(capi.lib().fdcm_templates_lengths(self._h, capi.fptr(out)))
        return out

    def capacity(self, n_scene, max_tmpl_lines, max_scene_lines):
        cap = C.c_int64()
        capi.check(capi.lib().fdcm_search_capacity(self._h, n_scene, max_tmpl_lines, max_scene_lines, C.byref(cap)))
        return cap.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.lib().fdcm_templates_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def edge_labels(image, depth=30, threshold=60, low=None, smooth=0, min_pixels=1):
    """The label image of a 2-D uint8 array (include/fdcm.h, "feature maps from images"), computed on the GPU: (H, W) uint8,
    the orientation slice of every edge pixel and 255 elsewhere.  low / smooth / min_pixels as DeviceFeatureMap.build_image's."""
    a = np.asarray(image)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"image must be a 2-D uint8 array, got {a.dtype} with shape {a.shape}")
    p, w, h, stride, _, keep = _pixels(a, "image")
    out = np.empty((h, w), dtype=np.uint8)
    ex = _edge_params(threshold, low, smooth, min_pixels)
    if ex is not None:
        capi.check(capi.lib().fdcm_edge_labels_ex(p, w, h, stride, int(depth), C.byref(ex), C.c_void_p(out.ctypes.data)))
    else:
        capi.check(capi.lib().fdcm_edge_labels(p, w, h, stride, int(depth), int(threshold), C.c_void_p(out.ctypes.data)))
    return out


def _adopt_lines(ptr, n):
    """A library-allocated array of n line records as a (4, n) float32 array of its own (the LineArray openfdcm.read
    returns); the allocation is released."""
    if not ptr or n == 0:
        if ptr:
            capi.lib().fdcm_lines_free(ptr)
        return np.zeros((4, 0), dtype=np.float32)
    try:
        return np.ctypeslib.as_array(ptr, shape=(n, 4)).T.copy()
    finally:
        capi.lib().fdcm_lines_free(ptr)


def lines_from_labels(labels, depth=30, bucket=4, line_pixels=8, line_length=8):
    """The line segments of a label image (include/fdcm.h, "line segments from images"), computed on the GPU: (4, N) float32 in
    image pixels, as openfdcm.read returns them.  `labels`: 2-D uint8, a numpy array or a contiguous CUDA torch tensor, as
    edge_labels makes it for `depth`.  bucket: labels per orientation bucket; line_pixels / line_length: the fewest pixels and
    the shortest extent along the major axis of a kept component."""
    if hasattr(labels, "data_ptr") and not isinstance(labels, np.ndarray) and labels.dim() == 2 and not labels.is_contiguous():
        raise ValueError("labels on the device must be contiguous")
    p, w, h, _, dev, keep = _pixels(labels, "labels")
    if not dev and keep.size and keep.strides[0] != w:
        keep = np.ascontiguousarray(keep)
        p = C.c_void_p(keep.ctypes.data)
    lp = capi.LineParams(int(bucket), int(line_pixels), int(line_length))
    out, n = C.POINTER(C.c_float)(), C.c_int64()
    capi.check(capi.lib().fdcm_lines_from_labels(p, w, h, dev, int(depth), C.byref(lp), C.byref(out), C.byref(n)))
    return _adopt_lines(out, n.value)


def lines_from_image(image, depth=30, threshold=60, low=None, smooth=0, min_pixels=1, bucket=4, line_pixels=8, line_length=8):
    """The line segments of a frame: edge_labels(image, depth, threshold, low, smooth, min_pixels) followed by lines_from_labels,
    with the label image staying on the GPU.  `image`: 2-D uint8, a numpy array or a CUDA torch tensor (rows may be strided)."""
    p, w, h, stride, dev, keep = _pixels(image, "image")
    ex = capi.EdgeParams(int(smooth), int(threshold if low is None else low), int(threshold), int(min_pixels))
    lp = capi.LineParams(int(bucket), int(line_pixels), int(line_length))
    out, n = C.POINTER(C.c_float)(), C.c_int64()
    capi.check(capi.lib().fdcm_lines_from_image(p, w, h, stride, dev, int(depth), C.byref(ex), C.byref(lp), C.byref(out), C.byref(n)))
    return _adopt_lines(out, n.value)


def lines_last_timing():
    """Device milliseconds per stage of this thread's last lines_from_* call (fdcm_lines_timing) as a dict."""
    t = capi.LinesTiming()
    capi.check(capi.lib().fdcm_lines_last_timing(C.byref(t)))
    return {name: getattr(t, name) for name, _ in capi.LinesTiming._fields_}


class Mesh:
    """A triangle mesh with its edge table (include/fdcm.h, "Templates from a mesh"): `vertices` (V, 3) float32, `faces` (F, 3)
    int32, and the crease angle above which an edge between two faces is sharp.  Host memory alone: making one needs no device."""

    def __init__(self, vertices, faces, crease_angle=np.deg2rad(30)):
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        f = np.ascontiguousarray(faces, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"expected (V, 3) vertices and (F, 3) faces, got {v.shape} and {f.shape}")
        self.vertices, self.faces = v, f
        self._h = C.c_void_p()
        capi.check(capi.lib().fdcm_mesh_create(capi.fptr(v), v.shape[0], f.ctypes.data_as(C.POINTER(C.c_int32)), f.shape[0],
                                               float(np.cos(crease_angle)), C.byref(self._h)))
        ne, ns, nb = C.c_int64(), C.c_int64(), C.c_int64()
        capi.check(capi.lib().fdcm_mesh_info(self._h, C.byref(ne), C.byref(ns), C.byref(nb)))
        self.n_edges, self.n_sharp, self.n_boundary = ne.value, ns.value, nb.value

    def edges(self):
        """(verts (E, 2) int32 with i < j, faces (E, 2) int32 with -1 for none, sharp (E,) uint8), in edge order."""
        verts, faces = np.empty((self.n_edges, 2), dtype=np.int32), np.empty((self.n_edges, 2), dtype=np.int32)
        sharp = np.empty(self.n_edges, dtype=np.uint8)
        i32 = C.POINTER(C.c_int32)
        capi.check(capi.lib().fdcm_mesh_edges(self._h, verts.ctypes.data_as(i32), faces.ctypes.data_as(i32),
                                              sharp.ctypes.data_as(C.POINTER(C.c_uint8))))
        return verts, faces, sharp

    def default_depth_tolerance(self):
        """float32(1e-4 * the diagonal of the vertices' bounding box)."""
        d = self.vertices.astype(np.float64).max(axis=0) - self.vertices.astype(np.float64).min(axis=0)
        return np.float32(1e-4 * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))

    def default_near(self):
        """float32(1e-3 * the diagonal of the vertices' bounding box): the pinhole calls' near distance."""
        d = self.vertices.astype(np.float64).max(axis=0) - self.vertices.astype(np.float64).min(axis=0)
        return np.float32(1e-3 * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))

    def close(self):
        if self._h:
            capi.lib().fdcm_mesh_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _views(views):
    r = np.ascontiguousarray(views, dtype=np.float32)
    if r.ndim == 2 and r.shape == (3, 3):
        r = r[None]
    if r.ndim != 3 or r.shape[1:] != (3, 3):
        raise ValueError(f"views must be (n, 3, 3), got {r.shape}")
    return r


MESH_VISIBILITY = {"items": capi.MESH_VIS_ITEMS, "exact": capi.MESH_VIS_EXACT}


def _camera(mesh, n_views, scale, focal, positions, near):
    """None for the orthographic call; else (fdcm_mesh_camera, positions (n_views, 3) float32) of the pinhole one.  Exactly one of
    scale and focal is given."""
    if (scale is None) == (focal is None):
        raise ValueError("exactly one of scale (orthographic) and focal (pinhole) must be given")
    if focal is None:
        if positions is not None or near is not None:
            raise ValueError("positions and near belong to the pinhole call: give focal, not scale")
        return None
    if positions is None:
        raise ValueError("a pinhole call needs positions (view_positions makes them)")
    t = np.ascontiguousarray(positions, dtype=np.float32)
    if t.shape == (3,):
        t = np.ascontiguousarray(np.broadcast_to(t, (n_views, 3)))
    if t.shape != (n_views, 3):
        raise ValueError(f"positions must be (3,) or ({n_views}, 3), got {t.shape}")
    if near is None:
        near = mesh.default_near()
    return capi.MeshCamera(float(focal), float(near)), t


def mesh_view_lines(mesh, views, scale=None, depth_tolerance=None, min_length=2.0, visibility="items", join_tolerance=None, *,
                    focal=None, positions=None, near=None):
    """fdcm_mesh_view_lines_ex as it is: ((N, 4) float32 line records of all views, int64 offsets of n_views + 1).  visibility:
    "items" or "exact" (an integer goes to the library as it is); join_tolerance: pixels, None for no joining.  With focal=
    (and positions=, near=) in place of scale: fdcm_mesh_view_lines_cam, the pinhole views."""
    r = _views(views)
    cam = _camera(mesh, r.shape[0], scale, focal, positions, near)
    tol = mesh.default_depth_tolerance() if depth_tolerance is None else depth_tolerance
    offsets = np.zeros(r.shape[0] + 1, dtype=np.int64)
    out = C.POINTER(C.c_float)()
    params = capi.MeshLineParams(float(tol), float(min_length), int(MESH_VISIBILITY.get(visibility, visibility)),
                                 -1.0 if join_tolerance is None else float(join_tolerance))
    if cam is None:
        capi.check(capi.lib().fdcm_mesh_view_lines_ex(mesh._h, capi.fptr(r), r.shape[0], float(scale), C.byref(params),
                                                      C.byref(out), offsets.ctypes.data_as(C.POINTER(C.c_int64))))
    else:
        capi.check(capi.lib().fdcm_mesh_view_lines_cam(mesh._h, capi.fptr(r), capi.fptr(cam[1]), r.shape[0], C.byref(cam[0]),
                                                       C.byref(params), C.byref(out), offsets.ctypes.data_as(C.POINTER(C.c_int64))))
    n = int(offsets[-1])
    try:
        rec = np.ctypeslib.as_array(out, shape=(n, 4)).copy() if n else np.zeros((0, 4), dtype=np.float32)
    finally:
        if out:
            capi.lib().fdcm_lines_free(out)
    return rec, offsets


def templates_from_mesh(mesh, views, scale=None, depth_tolerance=None, min_length=2.0, visibility="items", join_tolerance=None, *,
                        focal=None, positions=None, near=None):
    """The line template of every view of a mesh, computed on the GPU (include/fdcm.h, "Templates from a mesh"): a list of (4, N)
    float32 arrays, template t being view t, with the projection of the mesh origin at (0, 0).  views: (n, 3, 3) rotations
    (view_rotations makes them); scale: pixels per mesh unit; depth_tolerance: mesh units, None for 1e-4 of the bounding box's
    diagonal; min_length: the shortest line kept, in pixels.  For a smooth, tessellated part take visibility="exact" (every
    face is tested at the sample itself, not the one that owns its pixel) and a join_tolerance in pixels, such as 0.5 (the
    contour's runs are chained at shared vertices and simplified before min_length applies): the defaults keep only
    fragments of such an outline.
    Orthographic with scale=; a pinhole camera with focal= in its place (exactly one of the two): focal in pixels, positions
    (n, 3) or (3,), where the mesh origin lies in the camera's frame for each view -- the camera at the origin looks down -Z,
    so positions[:, 2] < 0, and view_positions(n, distance) makes the on-axis ones -- and near in mesh units, None for 1e-3
    of the bounding box's diagonal: a view with a vertex nearer than that is refused ("Templates from a mesh: pinhole
    views")."""
    rec, offsets = mesh_view_lines(mesh, views, scale, depth_tolerance, min_length, visibility, join_tolerance, focal=focal,
                                   positions=positions, near=near)
    return [np.ascontiguousarray(rec[offsets[i]:offsets[i + 1]].T) for i in range(len(offsets) - 1)]


def mesh_view_items(mesh, view, scale=None, *, focal=None, positions=None, near=None):
    """Test hook (fdcm_mesh_view_items, or with focal= fdcm_mesh_view_items_cam): one view's pixel box (x0, y0, x1, y1) and its
    item buffer, (rows, columns) uint64."""
    r = _views(view)
    if r.shape[0] != 1:
        raise ValueError("one view")
    cam = _camera(mesh, 1, scale, focal, positions, near)
    box = np.zeros(4, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)

    def call(keys, capacity):
        if cam is None:
            capi.check(capi.lib().fdcm_mesh_view_items(mesh._h, capi.fptr(r), float(scale), box.ctypes.data_as(i32), keys, capacity))
        else:
            capi.check(capi.lib().fdcm_mesh_view_items_cam(mesh._h, capi.fptr(r), capi.fptr(cam[1]), C.byref(cam[0]),
                                                           box.ctypes.data_as(i32), keys, capacity))
    call(None, 0)
    w, h = int(box[2]) - int(box[0]) + 1, int(box[3]) - int(box[1]) + 1
    keys = np.empty((h, w), dtype=np.uint64)
    call(keys.ctypes.data_as(C.POINTER(C.c_uint64)), keys.size)
    return tuple(int(b) for b in box), keys


def view_positions(n, distance):
    """n positions (0, 0, -distance), (n, 3) float32: the mesh origin on the optical axis of a pinhole camera, `distance` mesh
    units in front of it."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    if not (np.isfinite(distance) and distance > 0):
        raise ValueError("distance must be finite and > 0")
    t = np.zeros((n, 3), dtype=np.float32)
    t[:, 2] = -np.float32(distance)
    return t


def view_rotations(n, hemisphere=True):
    """n view rotations, (n, 3, 3) float32, pure numpy.  The directions d_k towards the viewer lie on a Fibonacci spiral:
    z_k = 1 - (k + 0.5) / n (hemisphere: 0 < z <= 1) or 1 - (2 k + 1) / n (the sphere), at the azimuth k * pi * (3 - sqrt(5)).
    View k is the matrix with the rows (x, y, d_k): it turns d_k onto +Z.  The in-plane axis is fixed by x = (-d.y, d.x, 0) /
    |(d.x, d.y)|, the horizontal direction at right angles to d -- (1, 0, 0) where d is within 1e-9 of the pole -- and
    y = d x x, so the determinant is +1.  In-plane rotation is what `angles=` and search() cover."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (k + 0.5) / n if hemisphere else 1.0 - (2.0 * k + 1.0) / n
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    x = np.stack([-d[:, 1], d[:, 0], np.zeros(n)], axis=1)
    norm = np.hypot(x[:, 0], x[:, 1])
    pole = norm < 1e-9
    x[~pole] /= norm[~pole, None]
    x[pole] = (1.0, 0.0, 0.0)
    y = np.cross(d, x)
    return np.stack([x, y, d], axis=1).astype(np.float32)


def record_rotations(records, views):
    """Step 5 of the 6-DOF procedure, pure numpy: per match record the (3, 3) float64 rotation Rz(c, s) . views[tmpl_idx] with
    (c, s) = (transform[0], transform[3]), and the image position (transform[2], transform[5]) of the mesh origin's projection.
    Returns ((n, 3, 3) float64, (n, 2) float64)."""
    from .matchlist import records_of
    rec = records_of(records)
    v = np.asarray(views, dtype=np.float64).reshape(-1, 3, 3)
    idx = rec["tmpl_idx"].astype(np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= len(v)):
        raise ValueError("a record's tmpl_idx is outside the views")
    tr = rec["transform"].astype(np.float64).reshape(-1, 6)
    rz = np.zeros((len(rec), 3, 3), dtype=np.float64)
    rz[:, 0, 0], rz[:, 0, 1], rz[:, 1, 0], rz[:, 1, 1], rz[:, 2, 2] = tr[:, 0], -tr[:, 3], tr[:, 3], tr[:, 0], 1.0
    return rz @ v[idx], tr[:, [2, 5]].copy()


def record_camera_poses(records, views, positions, focal, principal=(0.0, 0.0)):
    """The pose of the object in the camera's frame per match record of pinhole templates, pure numpy float64: ((n, 3, 3)
    rotations R_obj, (n, 3) translations T_obj), a mesh point v lying at R_obj v + T_obj in front of a camera that looks down
    -Z with focal length `focal` (pixels) and the principal point `principal` (image pixels).  With Rz from the record's
    (c, s) = (transform[0], transform[3]), (x, y) = (transform[2], transform[5]), t_v = positions[tmpl_idx], d0 = -t_v.z,
    O_v = focal (t_v.x, t_v.y) / d0 and delta = (x, y) - principal - Rz O_v:
        R_obj = Rz . views[tmpl_idx],    T_obj = Rz t_v + (delta.x d0 / focal, delta.y d0 / focal, 0).
    Where delta = 0 this is exact: a rotation about the optical axis commutes with the projection, so the mesh under the pose
    projects onto the record's transform of the template.  Otherwise it is first order: the object is moved parallel to the
    image plane, which moves the image of a point at depth d by delta d0 / d, not by delta, so the image is the moved template
    up to delta (d0 - d) / d -- small where the object is shallow against its distance.  In either case the mesh origin
    projects exactly to (x, y)."""
    from .matchlist import records_of
    rec = records_of(records)
    v = np.asarray(views, dtype=np.float64).reshape(-1, 3, 3)
    t = np.asarray(positions, dtype=np.float64)
    t = np.broadcast_to(t, (len(v), 3)) if t.shape == (3,) else t.reshape(-1, 3)
    if len(t) != len(v):
        raise ValueError("positions must be (3,) or one per view")
    idx = rec["tmpl_idx"].astype(np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= len(v)):
        raise ValueError("a record's tmpl_idx is outside the views")
    focal = float(focal)
    tr = rec["transform"].astype(np.float64).reshape(-1, 6)
    rz = np.zeros((len(rec), 3, 3), dtype=np.float64)
    rz[:, 0, 0], rz[:, 0, 1], rz[:, 1, 0], rz[:, 1, 1], rz[:, 2, 2] = tr[:, 0], -tr[:, 3], tr[:, 3], tr[:, 0], 1.0
    tv = t[idx]
    d0 = -tv[:, 2]
    o = focal * tv[:, :2] / d0[:, None]
    delta = tr[:, [2, 5]] - np.asarray(principal, dtype=np.float64) - np.einsum("nij,nj->ni", rz[:, :2, :2], o)
    T = np.einsum("nij,nj->ni", rz, tv)
    T[:, :2] += delta * (d0 / focal)[:, None]
    return rz @ v[idx], T


def search_raw(fm, templates, scene, max_tmpl_lines, max_scene_lines, optimizer=capi.BATCH_OPTIMIZE, batch_size=10,
               tmpl_index_base=0):
    """Run the search and return the raw matches as a structured array (capi.MATCH_DTYPE)."""
    rec = capi.as_records(scene)
    out = C.c_void_p()
    n = C.c_int64()
    capi.check(capi.lib().fdcm_search(fm._h, templates._h, capi.fptr(rec), rec.shape[0], int(max_tmpl_lines),
                                      int(max_scene_lines), int(optimizer), int(batch_size), int(tmpl_index_base),
                                      C.byref(out), C.byref(n)))
    fm.last_search_count = n.value  # the records the handle keeps on the device (topk, verify_matches, detect_matches)
    return _adopt_matches(out, n.value)


def search_into(fm, templates, scene, max_tmpl_lines, max_scene_lines, optimizer, batch_size, tmpl_index_base,
                device_ptr):
    """Search leaving the matches in a caller-provided device buffer; returns the count."""
    rec = capi.as_records(scene)
    n = C.c_int64()
    capi.check(capi.lib().fdcm_search_device(fm._h, templates._h, capi.fptr(rec), rec.shape[0], int(max_tmpl_lines),
                                             int(max_scene_lines), int(optimizer), int(batch_size),
                                             int(tmpl_index_base), C.c_void_p(device_ptr), C.byref(n)))
    return n.value


class FramePipeline:
    """Owns an fdcm_pipeline: `slots` frames in flight, each running rebuild + search on its own HIP
    stream and host worker thread (include/fdcm.h, "frame pipeline")."""

    def __init__(self, templates, depth=30, coeff=5.0, padding=2.2, distance=capi.L2, max_tmpl_lines=4,
                 max_scene_lines=4, optimizer=capi.BATCH_OPTIMIZE, batch_size=10, tmpl_index_base=0, slots=2):
        self.templates = templates  # keeps the handle alive
        h = C.c_void_p()
        capi.check(capi.lib().fdcm_pipeline_create(int(depth), float(coeff), float(padding), int(distance),
                                                   templates._h, int(max_tmpl_lines), int(max_scene_lines),
                                                   int(optimizer), int(batch_size), int(tmpl_index_base), int(slots),
                                                   C.byref(h)))
        self._h = h
        self.slots = int(slots)
        self.last_build_timing = None
        self.last_search_timing = None

    def submit(self, scene, device_ptr=None, prepared=False):
        """Queue one frame; returns its ticket.  `scene` is a (4, N) LineArray, or with prepared=True the
        (N, 4) float32 records capi.as_records() returns."""
        rec = scene if prepared else capi.as_records(scene)
        t = C.c_int64()
        capi.check(capi.lib().fdcm_pipeline_submit(self._h, capi.fptr(rec), rec.shape[0],
                                                   C.c_void_p(device_ptr) if device_ptr else None, C.byref(t)))
        return t.value

    def wait(self, ticket, to_host=True):
        """Block until frame `ticket` is complete.  Returns the raw matches (structured array) when the frame
        was submitted without a device buffer, else the match count."""
        out, n = C.c_void_p(), C.c_int64()
        bt, st = capi.BuildTiming(), capi.SearchTiming()
        capi.check(capi.lib().fdcm_pipeline_wait(self._h, int(ticket), C.byref(out), C.byref(n), C.byref(bt),
                                                 C.byref(st)))
        self.last_build_timing = {k: getattr(bt, k) for k, _ in bt._fields_}
        self.last_search_timing = {k: getattr(st, k) for k, _ in st._fields_}
        if not out:
            return n.value
        return _adopt_matches(out, n.value)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.lib().fdcm_pipeline_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def topk(fm, templates, k, penalty=None, tau=1.0, tmpl_index_base=0, device_ptr=None, n=0):
    """penalize + sort_matches + [:k] on the device (include/fdcm.h, "device tail").

    Works on the raw matches of the last search_raw() on `fm`, or on a device buffer filled by
    search_into() (`device_ptr`, `n` records).  penalty: None, capi.DEFAULT_PENALTY or
    capi.EXPONENTIAL_PENALTY (with tau).  Returns a structured array (capi.MATCH_DTYPE) of min(k, n)
    records, ascending penalised score, ties in positional order."""
    out, n_out = C.c_void_p(), C.c_int64()
    capi.check(capi.lib().fdcm_topk(fm._h, templates._h, C.c_void_p(device_ptr) if device_ptr else None, int(n),
                                    int(tmpl_index_base), -1 if penalty is None else int(penalty), float(tau), int(k),
                                    C.byref(out), C.byref(n_out)))
    return _adopt_matches(out, n_out.value)


class ShardedEngine:
    """Template shards over several GPUs of this node from one process (fdcm_sharded_* in include/fdcm.h): every
    device rebuilds the DT3 volume and searches a contiguous template range; the records (or the k best of every
    shard) reach the first device in one grouped RCCL send/recv per frame.  Returns what the single-device calls
    return for the whole template list."""

    def __init__(self, templates, devices=None, n_devices=None, depth=30, coeff=5.0, padding=2.2, distance=capi.L2,
                 always_collective=False, allow_same_device=False):
        flat, offsets = capi.pack_templates(templates)
        if devices is not None:
            n_devices = len(devices)
            dev = (C.c_int * n_devices)(*devices)
        else:
            n_devices = n_devices or 1
            dev = None
        h = C.c_void_p()
        capi.check(capi.lib().fdcm_sharded_create(dev, n_devices, capi.fptr(flat) if flat.size else None,
                                                  offsets.ctypes.data_as(C.POINTER(C.c_int64)), len(templates), depth, coeff,
                                                  padding, distance, (capi.SHARDED_ALWAYS_COLLECTIVE if always_collective else 0) |
                                                  (capi.SHARDED_ALLOW_SAME_DEVICE if allow_same_device else 0),
                                                  C.byref(h)))
        self._h, self.n_devices, self.n_templates = h, n_devices, len(templates)

    def info(self):
        n = C.c_int()
        devs = (C.c_int * self.n_devices)()
        begin = (C.c_int64 * (self.n_devices + 1))()
        coll, moved = C.c_int64(), C.c_int64()
        capi.check(capi.lib().fdcm_sharded_info(self._h, C.byref(n), devs, begin, C.byref(coll), C.byref(moved)))
        return {"devices": list(devs), "shard_begin": list(begin), "collectives": coll.value, "bytes_moved": moved.value}

    def search(self, scene, max_tmpl_lines, max_scene_lines, optimizer=capi.BATCH_OPTIMIZE, batch_size=10):
        rec = capi.as_records(scene)
        out, n = C.c_void_p(), C.c_int64()
        capi.check(capi.lib().fdcm_sharded_search(self._h, capi.fptr(rec) if rec.size else None, rec.shape[0], max_tmpl_lines,
                                                  max_scene_lines, optimizer, batch_size, C.byref(out), C.byref(n)))
        return _adopt_matches(out, n.value)

    def search_topk(self, scene, max_tmpl_lines, max_scene_lines, k, penalty=None, tau=1.0, optimizer=capi.BATCH_OPTIMIZE,
                    batch_size=10):
        rec = capi.as_records(scene)
        out, n = C.c_void_p(), C.c_int64()
        capi.check(capi.lib().fdcm_sharded_search_topk(self._h, capi.fptr(rec) if rec.size else None, rec.shape[0],
                                                       max_tmpl_lines, max_scene_lines, optimizer, batch_size,
                                                       -1 if penalty is None else penalty, tau, k, C.byref(out), C.byref(n)))
        return _adopt_matches(out, n.value)

    def set_mode(self, mode):
        """capi.SHARD_TEMPLATES (default: every frame on every device, template ranges, one exchange per frame) or
        capi.SHARD_FRAMES (ticket t whole on device t % n_devices over the whole template list, no exchange).  Only while
        no frame is in flight; tickets restart at 0."""
        capi.check(capi.lib().fdcm_sharded_set_mode(self._h, int(mode)))

    def set_frames_in_flight(self, n_frames):
        """Frame slots per device (1..16); only while no frame is in flight."""
        capi.check(capi.lib().fdcm_sharded_set_frames_in_flight(self._h, int(n_frames)))

    def submit(self, scene, max_tmpl_lines, max_scene_lines, optimizer=capi.BATCH_OPTIMIZE, batch_size=10, k=None,
               penalty=None, tau=1.0, prepared=False):
        """Queue one frame on every device and return its ticket (k given: top-k mode)."""
        rec = scene if prepared else capi.as_records(scene)
        t = C.c_int64()
        if k is None:
            capi.check(capi.lib().fdcm_sharded_submit(self._h, capi.fptr(rec) if rec.size else None, rec.shape[0], max_tmpl_lines,
                                                      max_scene_lines, optimizer, batch_size, C.byref(t)))
        else:
            capi.check(capi.lib().fdcm_sharded_submit_topk(self._h, capi.fptr(rec) if rec.size else None, rec.shape[0],
                                                           max_tmpl_lines, max_scene_lines, optimizer, batch_size,
                                                           -1 if penalty is None else penalty, tau, k, C.byref(t)))
        return t.value

    def wait(self, ticket):
        """Collect a frame: its exchange runs here while the devices compute the frames submitted after it."""
        out, n = C.c_void_p(), C.c_int64()
        capi.check(capi.lib().fdcm_sharded_wait(self._h, int(ticket), C.byref(out), C.byref(n)))
        return _adopt_matches(out, n.value)

    def timing(self, shard=0):
        bt, st = capi.BuildTiming(), capi.SearchTiming()
        capi.check(capi.lib().fdcm_sharded_last_timing(self._h, shard, C.byref(bt), C.byref(st)))
        return ({k: getattr(bt, k) for k, _ in bt._fields_}, {k: getattr(st, k) for k, _ in st._fields_})

    def close(self):
        if self._h:
            capi.check(capi.lib().fdcm_sharded_free(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
