"""Times the detections over pose windows (include/fdcm.h, "Detections over pose windows") as the fine stage of a
coarse-to-fine detector on config 2' (bench.py's feature map and synthetic templates), DESIGN.md section 16's workload: the
first --templates templates, --coarse-angles angles at stride --coarse-stride, a fine table of --fine-angles angles, boxes of
(2 ha + 1) x (2 h + 1)^2 poses.  The seeds are --seeds detections of exhaustive_detect_all on the coarse table at overlap
--coarse-overlap (1: nothing suppressed, the best grid points; the fine stage's rule reduces them).

  detect_windows     one blocking fdcm_search_exhaustive_detect_windows call on the jobs (boxes, job indices), and the same
                     with the gate at --min-matched and the fractions returned
  window_search      fdcm_search_exhaustive_windows at k = 1 on the same jobs: what the call adds is the difference.  With
                     --windows-only this is the only row, for a build from before the call (--package-root: the directory
                     that holds its openfdcm_amd), run as processes in turn with this build's
  composition        what a caller had before: the window search, penalize, matched_fractions and the greedy rule of
                     tests/nms_ref.py on the winners' list in numpy; its records are compared with the call's
  dense              (--dense) exhaustive_detect_all on the whole fine table at stride 1: what the call replaces

Each figure is the median of --reps blocking calls after a warm-up, with the smallest and the largest.

    python tools/window_detect_bench.py [--reps 5] [--dense] [--windows-only] [--package-root DIR] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, reps):
    fn()  # warm-up: workspaces, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "reps": reps}


def list_nms(keys, boxes, permille, max_det):
    """tests/nms_ref.py's rule on a list: keys uint64 (2^64 - 1: no candidate), boxes (n, 4) int64.  The indices found."""
    none = np.uint64(2 ** 64 - 1)
    F = boxes.astype(np.int64)
    area = (F[:, 2] - F[:, 0] + 1) * (F[:, 3] - F[:, 1] + 1)
    left = keys != none
    out = []
    while len(out) < max_det and left.any():
        d = int(np.argmin(np.where(left, keys, none)))
        out.append(d)
        w = np.maximum(0, np.minimum(F[:, 2], F[d, 2]) - np.maximum(F[:, 0], F[d, 0]) + 1)
        h = np.maximum(0, np.minimum(F[:, 3], F[d, 3]) - np.maximum(F[:, 1], F[d, 1]) + 1)
        inter = w * h
        left &= ~(1000 * inter > permille * (area + area[d] - inter))
        left[d] = False
    return np.array(out, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--templates", type=int, default=100)
    ap.add_argument("--coarse-angles", type=int, default=36)
    ap.add_argument("--coarse-stride", type=int, default=4)
    ap.add_argument("--seeds", type=int, default=800)
    ap.add_argument("--coarse-overlap", type=float, default=1.0)
    ap.add_argument("--fine-angles", type=int, default=360)
    ap.add_argument("--half-angles", type=int, default=5)
    ap.add_argument("--half", type=int, default=4)
    ap.add_argument("--overlap", type=float, default=0.3)
    ap.add_argument("--line-caps", type=float, default=3.0)
    ap.add_argument("--min-matched", type=float, default=0.25)
    ap.add_argument("--max-detections", type=int, default=1024)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--windows-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))

    import openfdcm_amd as openfdcm
    from openfdcm_amd import _capi, synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates

    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    sub = tmpls[: args.templates]
    tset = DeviceTemplates(sub, line_caps=args.line_caps)
    piv = openfdcm.template_pivots(sub)
    coarse = np.arange(args.coarse_angles) * (2 * np.pi / args.coarse_angles)
    fine = np.arange(args.fine_angles) * (2 * np.pi / args.fine_angles)
    ccs, fcs = openfdcm._angles(coarse), openfdcm._angles(fine)
    s = args.coarse_stride
    permille = int(round(1000 * args.overlap))
    P = _capi.DEFAULT_PENALTY
    grid = dev.exhaustive_rotations_window(tset, ccs, piv, s, s).as_tuple()
    seeds = dev.exhaustive_detect_all(tset, grid, ccs, piv, max_detections=args.seeds,
                                      overlap_permille=int(round(1000 * args.coarse_overlap)), penalty=P)
    jobs = openfdcm.pose_windows(seeds, coarse, fine, piv, args.half_angles, args.half, args.half, wrap=True)
    res = {"package": os.path.abspath(args.package_root), "templates": len(sub), "seeds": int(len(seeds)), "jobs": int(len(jobs)),
           "box": [int(jobs[0, 2]), int(jobs[0, 5]), int(jobs[0, 6])], "line_caps": args.line_caps, "overlap_permille": permille}
    print(f"{len(seeds)} seeds, {len(jobs)} jobs of {res['box']}", flush=True)

    def windows():
        return dev.exhaustive_window_search(tset, jobs, fcs, piv, wrap=True, k=1)

    (rec, off), res["window_search_k1"] = timed(windows, args.reps)
    print("window_search_k1", res["window_search_k1"], flush=True)
    if not args.windows_only:
        kw = dict(wrap=True, max_detections=args.max_detections, overlap_permille=permille, penalty=P, boxes=True, job_index=True)
        got, res["detect_windows"] = timed(lambda: dev.exhaustive_detect_windows(tset, jobs, fcs, piv, **kw), args.reps)
        res["detections"] = int(len(got[0]))
        print("detect_windows", res["detect_windows"], "detections", len(got[0]), flush=True)
        gated, res["detect_windows_gate_fractions"] = timed(
            lambda: dev.exhaustive_detect_windows(tset, jobs, fcs, piv, min_matched=args.min_matched, matched=True, **kw), args.reps)
        res["detections_gated"] = int(len(gated[0]))
        print("detect_windows_gate_fractions", res["detect_windows_gate_fractions"], "detections", len(gated[0]), flush=True)
        lengths = np.ascontiguousarray(tset.lengths(), dtype=np.float32)
        foot = tset.footprints(fcs, piv, margin=0)

        def composition():
            r, o = windows()
            r = np.array(r)
            job_of = np.repeat(np.arange(len(jobs)), np.diff(o))
            _capi.check(_capi.lib().fdcm_penalize(P, 1.0, C.c_void_p(r.ctypes.data), len(r), _capi.fptr(lengths), len(lengths)))
            poses = openfdcm.pose_windows(r, fine, fine, piv, 0, 0, 0)[:, [0, 1, 3, 4]]
            frac = dev.matched_fractions(tset, poses, fcs, piv)
            ok = frac >= np.float32(args.min_matched)  # (the call compares ML with float32(min_matched TL): equal but for rounding)
            keys = (r["score"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | job_of.astype(np.uint64)
            keys = np.where(ok, keys, np.uint64(2 ** 64 - 1))
            t = np.stack([poses[:, 2], poses[:, 3], poses[:, 2], poses[:, 3]], axis=1)
            boxes = foot.reshape(len(sub), len(fcs), 4)[poses[:, 0], poses[:, 1]] + t
            d = list_nms(keys, boxes, permille, args.max_detections)
            return r[d], boxes[d].astype(np.int32), frac[d], job_of[d].astype(np.int32)

        comp, res["composition_gate_fractions"] = timed(composition, args.reps)
        res["composition_records_equal"] = bool(comp[0].tobytes() == np.array(gated[0]).tobytes() and np.array_equal(comp[1], gated[1]))
        print("composition_gate_fractions", res["composition_gate_fractions"], "records equal", res["composition_records_equal"], flush=True)
        if args.dense:
            fgrid = dev.exhaustive_rotations_window(tset, fcs, piv, 1, 1).as_tuple()
            dense, res["dense_detect_all"] = timed(lambda: dev.exhaustive_detect_all(
                tset, fgrid, fcs, piv, max_detections=args.max_detections, overlap_permille=permille, penalty=P), max(1, args.reps // 2))
            res["dense_detections"], res["dense_grid"] = int(len(dense)), list(fgrid)
            print("dense_detect_all", res["dense_detect_all"], "detections", len(dense), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
