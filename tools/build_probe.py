"""The calls that lay out the build's scratch, the reference search's workspaces, the device tail's, scene coverage's and the
scratch of the calls without a handle, on one fixed list of cases, for comparing the library's paths
and a handle's histories: prints the SHA-256 of everything each case returns.

    python tools/build_probe.py                                    the default path, order "listed"
    python tools/build_probe.py --order listed|reversed|fresh
    FDCM_POISON=1 python tools/build_probe.py                      every buffer filled with a word before a call writes
    FDCM_POISON=1 FDCM_L2_SWEEP=literal FDCM_SEARCH_COMPACT2=1 FDCM_SEARCH_FLAT=1 FDCM_FORCE_HOST_BINS=1 python tools/build_probe.py

One line per case, `build_probe <case> <sha256>`, then `build_probe counts <name> <value> ..` and `build_probe fills <buffer>
<count> ..` (fdcm_selftest_poison_fills: how often FDCM_POISON's word went into each buffer).  The digests of every order and
of every switch must be equal (tests/test_gpu_build_workspace.py runs the switches in fresh processes: they are read once per
process).  "listed" and "reversed" share handles between the cases, one per (depth, distance): a case rebuilds the handle the
case before it left; "fresh" gives every case, and every step of a rebuild sequence, a handle of its own.

A case returns items (spec, array): the array is digested (NaNs canonical), the spec says what the array is by definition, so
that the test can hold it to its referee without this file knowing the referees."""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L2, L2_SQUARED, L1 = 0, 1, 2
DEFAULT_OPTIMIZE, BATCH_OPTIMIZE = 0, 1
DEFAULT, EXPONENTIAL = 0, 1  # the penalties (include/fdcm.h)
COEFF, PADDING = 5.0, 1.0    # of every handle here: a synthetic.scene(S, ..) then gives an S x S map
BASE = 7                     # tmpl_index_base of the searches
LINE = dict(bucket=4, line_pixels=8, line_length=8)
HYST = dict(threshold=100, low=30, smooth=1, min_pixels=6)

# The buffers the cases use, by their names in openfdcm_amd._capi.POISON_BUFFERS: under FDCM_POISON each has a fill count
# above 0 at the end of a run.  bins and bins_stage are used where the bins come from the host (FDCM_FORCE_HOST_BINS).
USED_BUFFERS = ("vol", "ivol", "bitmap", "coldesc", "colmask", "labels", "edge_parent", "edge_roots", "pyr", "offtab", "stack", "plan",
                "build_stage", "scene", "pairs", "records", "flags", "work", "counter", "out", "search_stage", "cnt", "tail", "tail_out",
                "coverage", "coverage_stage", "pixel_pixels", "pixel_labels", "pixel_keys", "pixel_parent", "pixel_counts",
                "pixel_comps", "pixel_out")
HOST_BINS_BUFFERS = ("bins", "bins_stage")


def image(width, height, seed):
    """A grey test image: rotated filled rectangles on a flat background, blurred once, with noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    img = np.full((height, width), 70.0)
    small = min(width, height)
    for _ in range(4):
        cx, cy = rng.uniform(0.2, 0.8) * width, rng.uniform(0.2, 0.8) * height
        hw, hh = rng.uniform(0.15, 0.4) * small + 1, rng.uniform(0.1, 0.3) * small + 1
        ang = rng.uniform(0, np.pi)
        c, s = np.cos(ang), np.sin(ang)
        u, v = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c
        img[(np.abs(u) <= hw) & (np.abs(v) <= hh)] = rng.uniform(120, 230)
    p = np.pad(img, 1, mode="edge")
    img = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] + 4 * img) / 8
    img += rng.normal(0.0, 4.0, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def inputs():
    """Everything the cases take, the same in every process and without a device."""
    from openfdcm_amd import synthetic
    rng = np.random.default_rng(83)
    scenes = {"s60": synthetic.scene(60, 14, 3), "s61": synthetic.scene(61, 16, 23), "s300": synthetic.scene(300, 40, 4),
              "s200": synthetic.scene(200, 45, 5), "s1100": synthetic.scene(1100, 30, 7), "s2100": synthetic.scene(2100, 30, 8),
              "s4130": synthetic.scene(4130, 20, 9), "s190": synthetic.scene(190, 60, 10), "s190b": synthetic.scene(190, 60, 11),
              "p192": synthetic.scene(192, 40, 12), "p320": synthetic.scene(320, 90, 13), "empty": np.zeros((4, 0), dtype=np.float32)}
    images = {"i97x61": image(97, 61, 1), "i130x200": image(130, 200, 2), "i5x3": image(5, 3, 3), "i20x1100a": image(20, 1100, 4),
              "i20x1100b": image(20, 1100, 5), "i70x37": image(70, 37, 6), "blank": np.full((200, 130), 90, dtype=np.uint8)}
    none = [np.zeros((4, 0), dtype=np.float32)]
    mixed = none + [t for n, s in ((2, 31), (3, 32), (13, 33), (70, 34)) for t in synthetic.templates(3, n, 200, s)]
    big = synthetic.templates(700, 6, 200, 35)

    def lines(n, ex, ey):
        return np.stack([rng.uniform(0, ex, n), rng.uniform(0, ey, n), rng.uniform(0, ex, n), rng.uniform(0, ey, n)]).astype(np.float32)
    cover = none + [lines(3, 24, 18), lines(40, 30, 24), lines(300, 34, 26)]
    poses = {}
    for name, (w, h) in (("i130x200", (130, 200)), ("i70x37", (70, 37))):
        p = [[rng.integers(0, 4), 0, rng.integers(-6, w - 8), rng.integers(-6, h - 6)] for _ in range(40)]
        p += [[1, 0, -1000, 0], [3, 0, 0, 5000], [0, 0, 5, 5], [3, 0, 10, 10], [3, 0, 11, 10], [2, 0, 10, 12], [3, 0, 10, 10]]
        poses[name] = np.asarray(p, dtype=np.int32)
    return {"scenes": scenes, "images": images, "tsets": {"mixed": mixed, "big": big, "cover": cover}, "poses": poses}


def canonical(a):
    a = np.ascontiguousarray(a)
    if a.dtype.names and "score" in a.dtype.names:
        a = a.copy()
        for f in ("score", "transform"):
            a[f] = np.where(np.isnan(a[f]), np.float32(np.nan), a[f])
        return a
    return np.where(np.isnan(a), np.float32(np.nan), a) if a.dtype.kind == "f" else a


class Ctx:
    """The inputs, the handles the cases share (none under "fresh"), the template sets on the device, and the counts."""

    def __init__(self, fresh):
        from openfdcm_amd.engine import DeviceTemplates
        self.inp, self.fresh, self.handles = inputs(), fresh, {}
        self.tsets = {k: DeviceTemplates(v) for k, v in self.inp["tsets"].items()}
        self.counts = dict(short_templates=0, worklist_block=0, worklist_generic=0, compact_one=0, compact_two=0, tall=0,
                           hw16=0, hw32=0, hw64=0, left_behind=0, steals_kept=0, hysteresis=0, levels=0, records=0, segments=0, order_history=0, order_proxy=0)

    def scene(self, key):
        return self.inp["scenes"][key]

    def lines_map(self, key, depth, distance, tag="a"):
        """A map of scene `key`: the shared handle of (depth, distance, tag) rebuilt, or a new one."""
        from openfdcm_amd.engine import DeviceFeatureMap
        hk = (depth, distance, tag)
        dev = None if self.fresh else self.handles.get(hk)
        if dev is None:
            dev = DeviceFeatureMap.build(self.scene(key), depth=depth, coeff=COEFF, padding=PADDING, distance=distance)
            if not self.fresh:
                self.handles[hk] = dev
        else:
            self.note_rebuild(dev, self.scene(key))
            dev.rebuild(self.scene(key))
        return dev

    def note_rebuild(self, dev, scene):
        """Counts a rebuild of a lines scene that leaves capacity behind its layout, and one that carries the steal counter over."""
        before = dev.width * dev.height
        if scene.shape[1]:
            ext = float(max(scene[0::2].max() - scene[0::2].min(), scene[1::2].max() - scene[1::2].min()))
            after = int(np.ceil(ext + 1)) ** 2
            self.counts["left_behind"] += int(0 < after < before)
            self.counts["steals_kept"] += int(after == before and dev.distance != L1 and dev.height <= 4096)

    def shape_class(self, dev):
        hw64 = (dev.height + 63) // 64
        self.counts["hw16" if hw64 <= 16 else "hw32" if hw64 <= 32 else "hw64" if hw64 <= 64 else "tall"] += 1
        return hw64


def lines_spec(key, depth, distance, stop_after=3):
    return ("lines_volume", key, depth, distance, stop_after)


# ---------------------------------------------------------------- the cases
def _staged(x, shapes):
    """Fresh staged builds (a rebuild always runs every stage)."""
    from openfdcm_amd.engine import DeviceFeatureMap
    out = []
    for key, depth, distance, stop, want_hw in shapes:
        dev = DeviceFeatureMap.build(x.scene(key), depth=depth, coeff=COEFF, padding=PADDING, distance=distance, stop_after=stop)
        hw = x.shape_class(dev)
        assert want_hw[0] < hw <= want_hw[1], (key, hw)
        out.append((lines_spec(key, depth, distance, stop), dev.volume()))
        dev.close()
    return out


def case_small_builds(x):
    """HW64 <= 16: k_coldesc_tile<16, 64>; depth 7 (k_propagate) and 30 (k_propagate_reg<30>); every distance and stage."""
    out = _staged(x, [("s60", 7, L2, 1, (0, 16)), ("s61", 7, L2_SQUARED, 2, (0, 16)), ("s60", 30, L1, 2, (0, 16)), ("s61", 30, L1, 1, (0, 16))])
    for key, depth, distance in (("s61", 7, L2), ("s60", 7, L2_SQUARED), ("s61", 7, L1), ("s60", 30, L2)):
        dev = x.lines_map(key, depth, distance)
        x.shape_class(dev)
        out.append((lines_spec(key, depth, distance), dev.volume()))
    return out


def case_medium_build(x):
    """16 < HW64 <= 32: k_coldesc_tile<32, 64>."""
    return _staged(x, [("s1100", 7, L2_SQUARED, 2, (16, 32))])


def case_large_build(x):
    """32 < HW64 <= 64: k_coldesc_tile<64, 32>."""
    return _staged(x, [("s2100", 3, L1, 1, (32, 64)), ("s2100", 2, L2, 3, (32, 64))])


def case_tall_builds(x):
    """A height above 4096: bitmap + k_seeds + k_coldesc; L1, and L2 by the literal sweep (H^2 > 2^24)."""
    out = []
    for distance in (L1, L2):
        dev = x.lines_map("s4130", 2, distance)
        assert dev.height > 4096 and x.shape_class(dev) > 64
        out.append((lines_spec("s4130", 2, distance), dev.volume()))
        if not x.fresh:  # the shared handle gives its memory back: 0.4 GB a distance
            x.handles.pop((2, distance, "a")).close()
    return out


def order_counts():
    import ctypes as C
    from openfdcm_amd import _capi
    h, p = C.c_int64(), C.c_int64()
    _capi.check(_capi.lib().fdcm_selftest_sweep_order_counts(C.byref(h), C.byref(p)))
    return h.value, p.value


def case_ordered_sweeps(x):
    """More (slice, chunk) pairs than two per CU: the sweep takes a launch order, from the proxy (the host's for lines, the
    device's for an image) at a handle's first build of a shape and from the previous build's costs at the second."""
    from openfdcm_amd.engine import DeviceFeatureMap
    out = []
    h0, p0 = order_counts()
    dev = DeviceFeatureMap.build(x.scene("s190"), depth=180, coeff=COEFF, padding=PADDING, distance=L2)
    assert dev.depth * ((dev.height + 63) // 64) > 512
    out.append((lines_spec("s190", 180, L2), dev.volume()))
    x.note_rebuild(dev, x.scene("s190b"))
    dev.rebuild(x.scene("s190b"))
    out.append((lines_spec("s190b", 180, L2), dev.volume()))
    dev.close()
    a, b = x.inp["images"]["i20x1100a"], x.inp["images"]["i20x1100b"]
    dev = DeviceFeatureMap.build_image(a, 60, depth=30, distance=L2_SQUARED)
    assert dev.depth * ((dev.height + 63) // 64) > 512
    out.append((("pixel_volume", ("edges", "i20x1100a", 0, 0, 60, 60, 1), 0, 30, L2_SQUARED, 3), dev.volume()))
    dev.rebuild_image(b, 60)
    out.append((("pixel_volume", ("edges", "i20x1100b", 0, 0, 60, 60, 1), 0, 30, L2_SQUARED, 3), dev.volume()))
    dev.close()
    h1, p1 = order_counts()
    # each pair: the proxy, then the history (the literal sweep takes no order)
    assert (h1 - h0, p1 - p0) == ((0, 0) if os.environ.get("FDCM_L2_SWEEP") == "literal" else (2, 2)), (h1 - h0, p1 - p0)
    x.counts["order_history"] += h1 - h0
    x.counts["order_proxy"] += p1 - p0
    return out


def _sequence(x, distance):
    """One handle through builds that shrink, grow and change the seed kind, with an empty scene and a blank image between real
    builds; under "fresh" every step on a handle of its own."""
    from openfdcm_amd.engine import DeviceFeatureMap
    import openfdcm_amd as fd
    depth = 7
    img, small = x.inp["images"]["i130x200"], x.inp["images"]["i70x37"]
    lab = fd.edge_labels(img, depth=depth, threshold=60)
    steps = [("lines", "s300"), ("lines", "s60"), ("labels", lab, 5), ("image", img, {}), ("lines", "empty"), ("image", img, HYST),
             ("level", img, 2), ("image", x.inp["images"]["blank"], {}), ("lines", "s61"), ("image", small, HYST), ("lines", "s300")]
    out = [(("labels", "i130x200", depth, 0, 60, 60, 1), lab)]
    dev = None if x.fresh else x.handles.get((depth, distance, "a"))  # what the cases before left, if anything
    for step in steps:
        if x.fresh and dev is not None:
            dev.close()
            dev = None
        kind = step[0]
        if dev is None:  # the handle's first build: lines (every sequence begins with them), or any kind under "fresh"
            kw = dict(depth=depth, coeff=COEFF, distance=distance)
            if kind == "lines":
                dev = DeviceFeatureMap.build(x.scene(step[1]), padding=PADDING, **kw)
            elif kind == "labels":
                dev = DeviceFeatureMap.build_labels(step[1], border=step[2], **kw)
            elif kind == "image":
                dev = DeviceFeatureMap.build_image(step[1], step[2].get("threshold", 60), **{k: v for k, v in step[2].items() if k != "threshold"}, **kw)
            else:
                dev = DeviceFeatureMap.build_image_level(step[1], step[2], 60, **kw)
        elif kind == "lines":
            x.note_rebuild(dev, x.scene(step[1]))
            dev.rebuild(x.scene(step[1]))
        elif kind == "labels":
            dev.rebuild_labels(step[1], border=step[2])
        elif kind == "image":
            dev.rebuild_image(step[1], step[2].get("threshold", 60), **{k: v for k, v in step[2].items() if k != "threshold"})
        else:
            dev.rebuild_image_level(step[1], step[2], 60)
        if kind == "lines":
            spec = lines_spec(step[1], depth, distance)
        elif kind == "labels":
            spec = ("pixel_volume", ("edges", "i130x200", 0, 0, 60, 60, 1), step[2], depth, distance, 3)
        else:
            name = [k for k, v in x.inp["images"].items() if v is step[1]][0]
            e = step[2] if kind == "image" else {}
            x.counts["hysteresis"] += int(bool(e))
            x.counts["levels"] += int(kind == "level")
            spec = ("pixel_volume", ("edges", name, step[2] if kind == "level" else 0, e.get("smooth", 0), e.get("low", 60), e.get("threshold", 60),
                                     e.get("min_pixels", 1)), 0, depth, distance, 3)
        out.append((spec, dev.volume()))
    if x.fresh:
        dev.close()
    else:
        x.handles[(depth, distance, "a")] = dev
    return out


def case_sequence_l2(x):
    return _sequence(x, L2)


def case_sequence_l1(x):
    return _sequence(x, L1)


def case_sequence_l2sq(x):
    return _sequence(x, L2_SQUARED)


def _searches(x, dev, map_spec, scene_key, sets):
    """Per template set: a host-output search per optimiser, the top k of the last one under each penalty, then the same search
    into a caller's device buffer and the top k of that."""
    import torch
    from openfdcm_amd.engine import search_raw, search_into, topk
    scene = x.scene(scene_key)
    out = []
    for tkey, maxT, maxS in sets:
        tset, tm = x.tsets[tkey], x.inp["tsets"][tkey]
        slots = len(tm) * min(maxT, max(t.shape[1] for t in tm)) * min(maxS, scene.shape[1])
        x.counts["worklist_generic" if slots > 16384 else "worklist_block"] += 1
        x.counts["short_templates"] += sum(1 for t in tm if t.shape[1] < maxT)
        cap = tset.capacity(scene.shape[1], maxT, maxS)
        x.counts["compact_two" if (cap + 1023) // 1024 > 64 or "FDCM_SEARCH_COMPACT2" in os.environ else "compact_one"] += 1
        for optimizer, batch in ((DEFAULT_OPTIMIZE, 1), (BATCH_OPTIMIZE, 3), (BATCH_OPTIMIZE, 10)):
            rspec = ("records", map_spec, tkey, scene_key, maxT, maxS, optimizer, batch, BASE)
            raw = search_raw(dev, tset, scene, maxT, maxS, optimizer, batch, BASE)
            x.counts["records"] += len(raw)
            out.append((rspec, raw))
        for penalty, tau in ((None, 1.0), (DEFAULT, 1.0), (EXPONENTIAL, 1.5)):  # of the last search: rspec
            for k in (1, 25, len(raw) + 5):
                out.append((("topk", rspec, k, penalty, tau), topk(dev, tset, k, penalty, tau, tmpl_index_base=BASE)))
        buf = torch.empty(max(1, cap) * 32, dtype=torch.uint8, device="cuda")
        n = search_into(dev, tset, scene, maxT, maxS, BATCH_OPTIMIZE, 10, BASE, buf.data_ptr())
        from openfdcm_amd import _capi
        out.append((rspec, buf[:n * 32].cpu().numpy().view(_capi.MATCH_DTYPE)))
        for penalty, tau in ((None, 1.0), (DEFAULT, 1.0), (EXPONENTIAL, 0.7)):
            k = min(25, n)
            out.append((("topk", rspec, k, penalty, tau), topk(dev, tset, k, penalty, tau, tmpl_index_base=BASE, device_ptr=buf.data_ptr(), n=n)))
        # the last host-output search's records are still the handle's: the device-output search left them alone
        out.append((("topk", rspec, 10, None, 1.0), topk(dev, tset, 10, None, 1.0, tmpl_index_base=BASE)))
    return out


SETS = [("big", 4, 6), ("mixed", 4, 4), ("big", 4, 6)]


def case_search_lines_map(x):
    """The searches on a lines map: large set -> small set -> large set on one handle."""
    dev = x.lines_map("s200", 30, L2)
    return [(lines_spec("s200", 30, L2), dev.volume())] + _searches(x, dev, lines_spec("s200", 30, L2), "s200", SETS)


def case_search_image_map(x):
    """The same on a map built from an image (its volume, adopted by the oracle, is the referee's map)."""
    from openfdcm_amd.engine import DeviceFeatureMap
    spec = ("pixel_volume", ("edges", "i130x200", 0, 0, 60, 60, 1), 3, 30, L2, 3)
    hk = (30, L2, "a")
    dev = None if x.fresh else x.handles.get(hk)
    if dev is None:
        dev = DeviceFeatureMap.build_image(x.inp["images"]["i130x200"], 60, border=3, depth=30, coeff=COEFF, distance=L2)
        if not x.fresh:
            x.handles[hk] = dev
    else:
        dev.rebuild_image(x.inp["images"]["i130x200"], 60, border=3)
    return [(spec, dev.volume())] + _searches(x, dev, spec, "s60", SETS[1:])


def case_pipeline(x):
    """Three slots, six frames that alternate two scene sizes: every slot sees both."""
    from openfdcm_amd.engine import FramePipeline
    pipe = FramePipeline(x.tsets["mixed"], depth=12, coeff=COEFF, padding=PADDING, distance=L2, max_tmpl_lines=4, max_scene_lines=4,
                         optimizer=BATCH_OPTIMIZE, batch_size=10, tmpl_index_base=BASE, slots=3)
    keys = ["p320", "p192"] * 3
    tickets = [pipe.submit(x.scene(k)) for k in keys[:3]]
    out = []
    for i, key in enumerate(keys):
        out.append((("records", lines_spec(key, 12, L2), "mixed", key, 4, 4, BATCH_OPTIMIZE, 10, BASE), pipe.wait(tickets[i])))
        if i + 3 < len(keys):
            tickets.append(pipe.submit(x.scene(keys[i + 3])))
    pipe.close()
    return out


def case_pixels(x):
    """The calls without a handle, each size followed by a 5 x 3 call."""
    import openfdcm_amd as fd
    out = []
    for name in ("i97x61", "i5x3", "i130x200", "i5x3"):
        img = x.inp["images"][name]
        plain = fd.edge_labels(img, depth=30, threshold=60)
        hyst = fd.edge_labels(img, depth=30, **HYST)
        out += [(("labels", name, 30, 0, 60, 60, 1), plain), (("labels", name, 30, HYST["smooth"], HYST["low"], HYST["threshold"], HYST["min_pixels"]), hyst)]
        seg = fd.lines_from_labels(plain, depth=30, **LINE)
        x.counts["segments"] += seg.shape[1]
        out.append((("segments", ("labels", name, 30, 0, 60, 60, 1)), seg))
        out.append((("segments", ("labels", name, 30, HYST["smooth"], HYST["low"], HYST["threshold"], HYST["min_pixels"])),
                    fd.lines_from_image(img, depth=30, **HYST, **LINE)))
        out += [(("pyramid", name, level), fd.image_pyramid(img, level)) for level in (1, 3)]
    return out


def case_coverage(x):
    """scene_coverage with the residual and scene_select on host labels, a large frame and then a small one on one handle, and
    once on labels on the device."""
    import torch
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    out = []
    dev = None
    for name in ("i130x200", "i70x37"):
        lab = fd.edge_labels(x.inp["images"][name], depth=30, threshold=60)
        lspec = ("labels", name, 30, 0, 60, 60, 1)
        if dev is None:
            dev = DeviceFeatureMap.build_labels(lab, border=0, depth=30, coeff=COEFF, distance=L2)
        elif x.fresh:
            dev.close()
            dev = DeviceFeatureMap.build_labels(lab, border=0, depth=30, coeff=COEFF, distance=L2)
        else:
            dev.rebuild_labels(lab, border=0)
        poses = x.inp["poses"][name]
        counts, res = dev.scene_coverage(lab, x.tsets["cover"], poses, residual=True)
        out += [(lspec, lab), (("coverage_counts", lspec, name), counts), (("coverage_residual", lspec, name), res)]
        sel, cnt, res = dev.scene_select(lab, x.tsets["cover"], poses, min_new=0.3, max_selected=16, residual=True)
        out += [(("select_selected", lspec, name), sel), (("select_counts", lspec, name), cnt), (("select_residual", lspec, name), res)]
        if name == "i130x200":
            t = torch.from_numpy(lab).cuda()
            counts, res = dev.scene_coverage(t, x.tsets["cover"], poses, residual=True)
            out += [(("coverage_counts", lspec, name), counts), (("coverage_residual", lspec, name), res.cpu().numpy())]
            sel, cnt, res = dev.scene_select(t, x.tsets["cover"], poses, min_new=0.3, max_selected=16, residual=True)
            out += [(("select_selected", lspec, name), sel), (("select_counts", lspec, name), cnt), (("select_residual", lspec, name), res.cpu().numpy())]
    dev.close()
    return out


CASES = [("small_builds", case_small_builds), ("medium_build", case_medium_build), ("large_build", case_large_build),
         ("tall_builds", case_tall_builds), ("ordered_sweeps", case_ordered_sweeps), ("sequence_l2", case_sequence_l2),
         ("sequence_l1", case_sequence_l1), ("sequence_l2sq", case_sequence_l2sq), ("search_lines_map", case_search_lines_map),
         ("search_image_map", case_search_image_map), ("pipeline", case_pipeline), ("pixels", case_pixels), ("coverage", case_coverage)]
ORDERS = ("listed", "reversed", "fresh")


def fills():
    """{buffer: fills of this process so far} (fdcm_selftest_poison_fills)."""
    import ctypes as C
    from openfdcm_amd import _capi
    n = len(_capi.POISON_BUFFERS)
    ids, counts = (C.c_int32 * n)(*range(n)), (C.c_int64 * n)()
    _capi.check(_capi.lib().fdcm_selftest_poison_fills(ids, n, counts))
    return dict(zip(_capi.POISON_BUFFERS, counts))


def run(order="listed", keep=False):
    """({case: digest}, counts, {case: items} when keep)."""
    assert order in ORDERS, order
    # The caller's device buffers (search_into) and the labels on the device are torch's.  torch brings a HIP runtime of its
    # own and finds no device once libfdcm_hip.so has loaded the system's, so it comes first.
    import torch  # noqa: F401
    x = Ctx(order == "fresh")
    digests, outputs = {}, {}
    for name, fn in (CASES[::-1] if order == "reversed" else CASES):
        items = fn(x)
        h = hashlib.sha256()
        for spec, a in items:
            a = canonical(a)
            h.update(repr((spec, a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
        digests[name] = h.hexdigest()
        if keep:
            outputs[name] = items
    for dev in x.handles.values():
        dev.close()
    return digests, x.counts, outputs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--order", default="listed", choices=ORDERS)
    a = ap.parse_args()
    digests, counts, _ = run(a.order)
    for name, _ in CASES:
        print("build_probe", name, digests[name])
    print("build_probe counts", " ".join(f"{k} {v}" for k, v in counts.items()))
    print("build_probe fills", " ".join(f"{k} {v}" for k, v in fills().items()))


if __name__ == "__main__":
    main()
