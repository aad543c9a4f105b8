"""Times the detections (include/fdcm.h, "Best map and detections") on config 2': the feature map and the 1000 x 32-line
synthetic templates bench.py uses, all templates on their default window (exhaustive_window) at stride 1, 2 and 4, k = 8,
radius 8, ExponentialPenalty(1.5).  In the same run, on the same grid:

  detect        one blocking fdcm_search_exhaustive_detect call
  best_map      one blocking fdcm_best_map call (both planes to the host)
  top-k         fdcm_search_exhaustive with the same k: the same scoring, a list per template instead of the reduction
  peaks         fdcm_search_exhaustive_peaks with the same k and radius: a score plane per template written and read again
  host          what a caller had before these calls: fdcm_score_map to the host (T x ny x nx floats) and the reduction of
                tests/detect_ref.py in numpy (penalise, minimum pairkey over the templates in batches, peaks of the best
                plane, records); its records are compared with the detect call's

  nms           (--nms) one blocking fdcm_search_exhaustive_detect_nms call (include/fdcm.h, "Detections suppressed by
                footprint overlap") at the same k and at k = 64, overlap --overlap, margin 0; and once what a caller had before
                it: fdcm_best_map to the host (both planes) and the greedy rule of tests/nms_ref.py in numpy, whose records
                are compared with the call's

  all           (--all, on its own: the rows above are left out) "All detections below a score": per stride one blocking
                fdcm_search_exhaustive_detect_nms call at k = 64, the yardstick, which a build from before the new call has
                too; then, where the library has it, fdcm_search_exhaustive_detect_all at max_detections = 64 and max_score =
                +inf and the 50 %, 5 % and 0.5 % quantiles of the finite scores of fdcm_best_map on that grid, each compared
                with the leading records of the +inf list; and once max_detections = 4096 at overlap 1000, the most rounds

  matched       (--matched, on its own) "Detections by matched fraction": per stride fdcm_search_exhaustive_detect_all at
                max_detections = 64, the yardstick, which a build from before the new call has too, at max_score = +inf and the
                5 % quantile of fdcm_best_map's finite scores; then, where the library has it, the call by matched fraction at
                min_matched 0.5 and 0.9, at 0.5 with the fractions returned, without a gate with the fractions returned, and at
                the median of those fractions; and once per run fdcm_matched_fractions beside
                fdcm_line_costs on the poses of 64 and of 8000 grid points.  Meant with --line-caps.

Each device figure is the median of --reps blocking calls after a warm-up; the host composition runs --host-reps times.
--line-caps TAU gives every template line the cap TAU * its length (include/fdcm.h, "Per-line caps and line costs") in every
call of the run, the host composition's score map included.  Off by default.

    python tools/detect_bench.py [--reps 5] [--host-reps 1] [--strides 1,2,4] [--line-caps TAU] [--nms | --all | --matched] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_composition(dev, tset, grid, lengths, penalty, tau, k, r, batch=50):
    """(records, seconds of the download, seconds of the reduction)."""
    from detect_ref import normalised, pair_keys, records
    from peaks_ref import NO_KEY, peaks
    t0 = time.perf_counter()
    maps = dev.score_map(tset, grid)
    t1 = time.perf_counter()
    T, ny, nx = maps.shape
    best = np.full((ny, nx), NO_KEY, dtype=np.uint64)
    for b0 in range(0, T, batch):
        b1 = min(T, b0 + batch)
        q = normalised(maps[b0:b1, None], lengths[b0:b1], penalty, tau)
        keys = pair_keys(q)
        keys[keys != NO_KEY] += np.uint64(b0)  # the pair index of the whole set
        np.minimum(best, keys.min(axis=0), out=best)
    none = best == NO_KEY
    scores = (best >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    scores[none] = np.nan
    pairs = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    pairs[none] = -1
    g, s = peaks(scores, k, r, r)
    rec = records(g, s, pairs, 1, None, None, grid)
    return rec, t1 - t0, time.perf_counter() - t1


def nms_host_composition(dev, tset, grid, penalty, tau, k, permille):
    """(records, seconds of fdcm_best_map to the host, seconds of the greedy rule in numpy)."""
    from nms_ref import detect_nms_ref
    t0 = time.perf_counter()
    scores, pairs = dev.best_map(tset, grid, penalty=penalty, tau=tau)
    t1 = time.perf_counter()
    rec, _ = detect_nms_ref(scores, pairs, tset.footprints().reshape(-1, 4), grid, k, permille)
    return rec, t1 - t0, time.perf_counter() - t1


def all_mode(args, dev, tset, pen, tau, timed, spread):
    """The rows of --all."""
    pm = int(round(1000 * args.overlap))
    has_all = hasattr(dev, "exhaustive_detect_all")
    rows = []
    for s in [int(v) for v in args.strides.split(",")]:
        grid = dev.exhaustive_window(tset, s, s).as_tuple()
        n64_ms, n64_min, nrec = timed(lambda: dev.exhaustive_detect_nms(tset, grid, k=64, overlap_permille=pm, penalty=pen, tau=tau))
        row = {"stride": s, "grid": list(grid), "grid_points": grid[2] * grid[3], "overlap_permille": pm,
               "nms_k64_ms": round(n64_ms, 3), "nms_k64_ms_min": round(n64_min, 3), "nms_k64_ms_spread": round(spread[-1], 3),
               "nms_k64_detections": int(len(nrec))}
        print(f"stride {s}: grid {grid[2]}x{grid[3]}: nms k 64 {n64_ms:.2f} ms (min {n64_min:.2f}, spread {spread[-1]:.2f}), "
              f"{len(nrec)} detections", flush=True)
        if has_all:
            scores, _ = dev.best_map(tset, grid, penalty=pen, tau=tau)
            fin = np.sort(scores[np.isfinite(scores)])
            cases = [("inf", float("inf"))] + [(name, float(fin[min(len(fin) - 1, int(f * len(fin)))]))
                                               for name, f in (("q50", 0.5), ("q5", 0.05), ("q0.5", 0.005))]
            full = None
            for name, ms in cases:
                call = lambda: dev.exhaustive_detect_all(tset, grid, max_score=ms, max_detections=64, overlap_permille=pm, penalty=pen,
                                                         tau=tau)
                a_ms, a_min, rec = timed(call)
                full = rec if full is None else full
                cnt = int((full["score"] <= np.float32(ms)).sum())
                same = rec.tobytes() == (nrec if name == "inf" else full[:cnt]).tobytes()
                row["all_" + name] = {"max_score": ms, "ms": round(a_ms, 3), "ms_min": round(a_min, 3), "ms_spread": round(spread[-1], 3),
                                      "detections": int(len(rec)), "to_nms_k64": round(a_ms / n64_ms, 3), "records_as_predicted": bool(same)}
                print(f"stride {s}: all max_score {name} = {ms:.6g}: {a_ms:.2f} ms (min {a_min:.2f}, spread {spread[-1]:.2f}), "
                      f"{a_ms / n64_ms:.3f} of nms k 64; {len(rec)} detections; as predicted: {same}", flush=True)
            t0 = time.perf_counter()
            rec = dev.exhaustive_detect_all(tset, grid, max_score=float("inf"), max_detections=4096, overlap_permille=1000, penalty=pen,
                                            tau=tau)
            row["all_4096_overlap_1000_ms_once"] = round((time.perf_counter() - t0) * 1e3, 3)
            row["all_4096_overlap_1000_detections"] = int(len(rec))
            print(f"stride {s}: all max_detections 4096, overlap 1000, once: {row['all_4096_overlap_1000_ms_once']:.2f} ms, "
                  f"{len(rec)} detections", flush=True)
        rows.append(row)
    return rows


def matched_mode(args, dev, tset, pen, tau, timed, spread):
    """The rows of --matched."""
    pm = int(round(1000 * args.overlap))
    has = hasattr(dev, "matched_fractions")
    rows = []
    for s in [int(v) for v in args.strides.split(",")]:
        grid = dev.exhaustive_window(tset, s, s).as_tuple()
        scores, pairs = dev.best_map(tset, grid, penalty=pen, tau=tau)
        fin = np.sort(scores[np.isfinite(scores)])
        row = {"stride": s, "grid": list(grid), "grid_points": grid[2] * grid[3], "overlap_permille": pm}
        for name, ms in [("inf", float("inf")), ("q5", float(fin[min(len(fin) - 1, int(0.05 * len(fin)))]))]:
            cases = [("off", {})]
            if has:  # ("median": the median of the fractions the ungated list comes with, so that about half of it passes)
                cases += [("0.5", {"min_matched": 0.5}), ("0.9", {"min_matched": 0.9}), ("0.5_fractions", {"min_matched": 0.5, "matched": True}),
                          ("off_fractions", {"matched": True}), ("median", None)]
            for what, kw in cases:
                if kw is None:
                    kw = {"min_matched": float(np.median(out[1])) if len(out[1]) else 0.0, "matched": True}
                    row[f"{name}_median_min_matched"] = kw["min_matched"]
                call = lambda: dev.exhaustive_detect_all(tset, grid, max_score=ms, max_detections=64, overlap_permille=pm, penalty=pen,
                                                         tau=tau, **kw)
                c_ms, c_min, out = timed(call)
                rec = out[0] if isinstance(out, tuple) else out
                row[f"{name}_{what}"] = {"max_score": ms, "ms": round(c_ms, 3), "ms_min": round(c_min, 3), "ms_spread": round(spread[-1], 3),
                                         "detections": int(len(rec))}
                if isinstance(out, tuple):
                    row[f"{name}_{what}"]["fractions_min_median_max"] = [round(float(v), 4) for v in
                                                                         (out[1].min(), np.median(out[1]), out[1].max())] if len(rec) else []
                print(f"stride {s}: max_score {name} = {ms:.6g}, min_matched {what}: {c_ms:.2f} ms (min {c_min:.2f}, spread "
                      f"{spread[-1]:.2f}); {len(rec)} detections", flush=True)
        if has and s == 1:  # the pose calls, on points that have a candidate
            cand = np.flatnonzero(pairs.reshape(-1) >= 0)
            for n in (64, 8000):
                g = cand[np.linspace(0, len(cand) - 1, n).astype(np.int64)]
                poses = np.stack([pairs.reshape(-1)[g], np.zeros(n, dtype=np.int64), grid[0] + (g % grid[2]) * s, grid[1] + (g // grid[2]) * s],
                                 axis=1).astype(np.int32)
                f_ms, f_min, fr = timed(lambda: dev.matched_fractions(tset, poses))
                f_spread = spread[-1]
                l_ms, l_min, _ = timed(lambda: dev.line_costs(tset, poses))
                row[f"poses_{n}"] = {"matched_fractions_ms": round(f_ms, 3), "matched_fractions_ms_min": round(f_min, 3),
                                     "matched_fractions_ms_spread": round(f_spread, 3), "line_costs_ms": round(l_ms, 3),
                                     "line_costs_ms_min": round(l_min, 3), "fraction_median": round(float(np.median(fr)), 4)}
                print(f"stride {s}: {n} poses: matched_fractions {f_ms:.3f} ms (min {f_min:.3f}), line_costs {l_ms:.3f} ms (min {l_min:.3f})",
                      flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1, help="runs of the host composition (0: leave it out)")
    ap.add_argument("--strides", default="1,2,4")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--tau", type=float, default=1.5)
    ap.add_argument("--line-caps", type=float, default=None, metavar="TAU", help="cap every line's cost at TAU * its length")
    ap.add_argument("--nms", action="store_true", help="also time the detections suppressed by footprint overlap")
    ap.add_argument("--all", action="store_true", help="time all detections below a score, against nms at k = 64 (only)")
    ap.add_argument("--matched", action="store_true", help="time the detections by matched fraction, against --all's call (only)")
    ap.add_argument("--overlap", type=float, default=0.3, help="the overlap threshold of --nms, --all and --matched")
    ap.add_argument("--json", default=None, help="also write the results here")
    args = ap.parse_args()

    from openfdcm_amd import _capi, synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates

    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    tset = DeviceTemplates(tmpls, line_caps=args.line_caps)
    lengths = tset.lengths()
    k, r, pen, tau = args.k, args.radius, _capi.EXPONENTIAL_PENALTY, args.tau

    def timed(call):
        call()  # warm-up: workspaces, code objects
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = call()
            times.append(time.perf_counter() - t0)
        spread.append((max(times) - min(times)) * 1e3)
        return float(np.median(times)) * 1e3, min(times) * 1e3, out

    rows, spread = [], []  # spread: max - min of the last timed() call's repetitions
    if args.all:
        rows = all_mode(args, dev, tset, pen, tau, timed, spread)
    if args.matched:
        rows = matched_mode(args, dev, tset, pen, tau, timed, spread)
    for s in [] if args.all or args.matched else [int(v) for v in args.strides.split(",")]:
        grid = dev.exhaustive_window(tset, s, s).as_tuple()
        det_ms, det_min, recs = timed(lambda: dev.exhaustive_detect(tset, grid, k=k, rx=r, ry=r, penalty=pen, tau=tau))
        det_spread = spread[-1]
        map_ms, map_min, _ = timed(lambda: dev.best_map(tset, grid, penalty=pen, tau=tau))
        top_ms, top_min, _ = timed(lambda: dev.exhaustive_search(tset, grid, k=k))
        pk_ms, pk_min, per = timed(lambda: dev.exhaustive_peaks(tset, grid, k=k, rx=r, ry=r))
        row = {"stride": s, "k": k, "r": r, "grid": list(grid), "grid_points": grid[2] * grid[3],
               "detect_ms": round(det_ms, 3), "detect_ms_min": round(det_min, 3), "best_map_ms": round(map_ms, 3),
               "best_map_ms_min": round(map_min, 3), "topk_ms": round(top_ms, 3), "topk_ms_min": round(top_min, 3),
               "peaks_ms": round(pk_ms, 3), "peaks_ms_min": round(pk_min, 3), "detect_to_topk": round(det_ms / top_ms, 3),
               "detect_to_peaks": round(det_ms / pk_ms, 3), "detections": int(len(recs)), "per_template_records": int(len(per)),
               "detect_ms_spread": round(det_spread, 3)}
        print(f"stride {s}: grid {grid[2]}x{grid[3]}, detect {det_ms:.2f} ms (min {det_min:.2f}), best_map {map_ms:.2f} ms, "
              f"top-k {top_ms:.2f} ms, peaks r {r} {pk_ms:.2f} ms: detect / top-k {det_ms / top_ms:.3f}, detect / peaks "
              f"{det_ms / pk_ms:.3f}; {len(recs)} detections for {len(per)} per-template records", flush=True)
        if args.host_reps > 0:
            runs = [host_composition(dev, tset, grid, lengths, pen, tau, k, r) for _ in range(args.host_reps)]
            dl = float(np.median([v[1] for v in runs])) * 1e3
            red = float(np.median([v[2] for v in runs])) * 1e3
            same = runs[0][0].tobytes() == recs.tobytes()
            row.update({"host_score_map_ms": round(dl, 1), "host_reduction_ms": round(red, 1), "host_total_ms": round(dl + red, 1),
                        "host_to_detect": round((dl + red) / det_ms, 1), "host_records_equal": bool(same)})
            print(f"stride {s}: host composition: score_map {dl:.0f} ms + numpy reduction {red:.0f} ms = {(dl + red) / det_ms:.0f}x "
                  f"the detect call; records equal: {same}", flush=True)
        if args.nms:
            pm = int(round(1000 * args.overlap))
            nms_ms, nms_min, nrec = timed(lambda: dev.exhaustive_detect_nms(tset, grid, k=k, overlap_permille=pm, penalty=pen, tau=tau))
            nms_spread = spread[-1]
            n64_ms, n64_min, nrec64 = timed(lambda: dev.exhaustive_detect_nms(tset, grid, k=64, overlap_permille=pm, penalty=pen, tau=tau))
            href, dl, red = nms_host_composition(dev, tset, grid, pen, tau, k, pm)
            same = href.tobytes() == nrec.tobytes()
            row.update({"overlap_permille": pm, "nms_ms": round(nms_ms, 3), "nms_ms_min": round(nms_min, 3),
                        "nms_ms_spread": round(nms_spread, 3), "nms_k64_ms": round(n64_ms, 3), "nms_k64_ms_min": round(n64_min, 3),
                        "nms_k64_ms_spread": round(spread[-1], 3), "nms_detections": int(len(nrec)),
                        "nms_k64_detections": int(len(nrec64)), "nms_to_detect": round(nms_ms / det_ms, 3),
                        "nms_host_best_map_ms": round(dl * 1e3, 2), "nms_host_rule_ms": round(red * 1e3, 2),
                        "nms_host_total_ms": round((dl + red) * 1e3, 2), "nms_host_records_equal": bool(same)})
            print(f"stride {s}: nms overlap {args.overlap:g}: k {k} {nms_ms:.2f} ms (min {nms_min:.2f}, spread {nms_spread:.2f}; detect "
                  f"{det_ms:.2f}, spread {det_spread:.2f}), k 64 {n64_ms:.2f} ms; {len(nrec)} / {len(nrec64)} detections; host "
                  f"composition: best_map {dl * 1e3:.1f} ms + numpy rule {red * 1e3:.1f} ms; records equal: {same}", flush=True)
        rows.append(row)
    res = {"workload": "config 2': 1024x1024 scene (200 lines, seed 1), depth 30, L2, padding 1.0; 1000 templates x 32 lines "
                       "(seed 2), default window per stride; k %d, radius %d, ExponentialPenalty(%g)" % (k, r, tau),
           "reps": args.reps, "host_reps": args.host_reps, "rows": rows}
    if args.line_caps is not None:
        res["line_caps_tau"] = args.line_caps
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
