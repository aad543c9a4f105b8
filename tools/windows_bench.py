"""Times the pose-window search (include/fdcm.h, "Pose windows") as the refinement step of a coarse-to-fine detection on
config 2' (bench.py's feature map and synthetic templates):

  1. coarse peaks of the first --templates templates: --coarse-angles angles over the circle, stride --coarse-stride,
     k = --seeds per template, radius --radius, angle radius 1 with wrap (fdcm_search_exhaustive_rotations);
  2. jobs on a fine table of --fine-angles angles around every peak: 2 ha + 1 angles x (2 h + 1)^2 translations at stride 1
     (openfdcm.pose_windows);
  3. fdcm_search_exhaustive_windows on all jobs in one blocking call, median of --reps;
  4. the same records without it: one fdcm_search_exhaustive_rotations call per job on the one-template set, alternated with
     (3) repetition by repetition; its own repetitions give the spread the difference is judged by;
  5. the two record arrays must be byte-identical;
  6. the host preparation alone: the same jobs with 1 x 1 windows;
  7. for context, once: the dense search of the whole fine table at stride 1 on the same templates (--no-dense skips it).

    python tools/windows_bench.py [--reps 5] [--json out.json] [--no-dense]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--templates", type=int, default=100)
    ap.add_argument("--coarse-angles", type=int, default=36)
    ap.add_argument("--coarse-stride", type=int, default=4)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--fine-angles", type=int, default=360)
    ap.add_argument("--half-angles", type=int, default=5)
    ap.add_argument("--half", type=int, default=4)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import openfdcm_amd as openfdcm
    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates

    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    sub = tmpls[: args.templates]
    tset = DeviceTemplates(sub)
    one = [DeviceTemplates([t]) for t in sub]
    piv = openfdcm.template_pivots(sub)
    coarse = np.arange(args.coarse_angles) * (2 * np.pi / args.coarse_angles)
    fine = np.arange(args.fine_angles) * (2 * np.pi / args.fine_angles)
    ccs, fcs = openfdcm._angles(coarse), openfdcm._angles(fine)
    s = args.coarse_stride
    grid = dev.exhaustive_rotations_window(tset, ccs, piv, s, s).as_tuple()
    t0 = time.perf_counter()
    seeds = dev.exhaustive_rotation_search(tset, grid, ccs, piv, k=args.seeds, rx=args.radius, ry=args.radius, ra=1, wrap=True)
    coarse_ms = (time.perf_counter() - t0) * 1e3
    jobs = openfdcm.pose_windows(seeds, coarse, fine, piv, args.half_angles, args.half, args.half, wrap=True)
    k = args.k
    print(f"coarse: {len(seeds)} seeds in {coarse_ms:.1f} ms (first call); {len(jobs)} jobs of {jobs[0, 2]} x {jobs[0, 5]} x {jobs[0, 6]}",
          flush=True)

    def windows(j):
        return dev.exhaustive_window_search(tset, j, fcs, piv, wrap=True, k=k)

    def loop():
        out = []
        for t, a0, na, x0, y0, nx, ny in jobs:
            run = (a0 + np.arange(na)) % len(fcs)
            out.append(dev.exhaustive_rotation_search(one[t], (x0, y0, nx, ny, 1, 1), fcs[run], piv[t:t + 1], k=k, tmpl_index_base=int(t)))
        return np.concatenate(out)

    rec, off = windows(jobs)  # warm-up of both: workspaces, code objects
    ref = loop()
    identical = rec.tobytes() == ref.tobytes()
    t_new, t_loop = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        windows(jobs)
        t_new.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        loop()
        t_loop.append((time.perf_counter() - t0) * 1e3)
    unit = jobs.copy()
    unit[:, 3] += args.half
    unit[:, 4] += args.half
    unit[:, 5:] = 1
    windows(unit)
    t_prep = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        windows(unit)
        t_prep.append((time.perf_counter() - t0) * 1e3)
    res = {"workload": f"config 2', {len(sub)} templates; coarse {args.coarse_angles} angles stride {s} k {args.seeds} radius "
                       f"{args.radius} angle radius 1; fine {args.fine_angles} angles, jobs {int(jobs[0, 2])} x {int(jobs[0, 5])} x {int(jobs[0, 6])}, k {k}",
           "jobs": int(len(jobs)), "planes": int(jobs[:, 2].sum()), "poses": int((jobs[:, 2] * jobs[:, 5] * jobs[:, 6]).sum()),
           "records": int(len(rec)), "byte_identical_to_the_loop": bool(identical),
           "windows_ms": [round(v, 3) for v in t_new], "windows_ms_median": round(float(np.median(t_new)), 3),
           "loop_ms": [round(v, 3) for v in t_loop], "loop_ms_median": round(float(np.median(t_loop)), 3),
           "loop_ms_spread": round(max(t_loop) - min(t_loop), 3),
           "speedup": round(float(np.median(t_loop) / np.median(t_new)), 1),
           "host_preparation_ms_median": round(float(np.median(t_prep)), 3),
           "host_preparation_share": round(float(np.median(t_prep) / np.median(t_new)), 3), "coarse_first_call_ms": round(coarse_ms, 1)}
    print(f"windows {res['windows_ms_median']:.2f} ms (1 x 1 windows {res['host_preparation_ms_median']:.2f} ms), loop of {len(jobs)} calls "
          f"{res['loop_ms_median']:.1f} ms (spread {res['loop_ms_spread']:.1f} ms): {res['speedup']}x, byte-identical {identical}", flush=True)
    if not args.no_dense:
        g1 = dev.exhaustive_rotations_window(tset, fcs, piv, 1, 1).as_tuple()
        t0 = time.perf_counter()
        dev.exhaustive_rotation_search(tset, g1, fcs, piv, k=k, wrap=True)
        res["dense_fine_table_stride1_ms_once"] = round((time.perf_counter() - t0) * 1e3, 1)
        print(f"dense {args.fine_angles} angles at stride 1, once: {res['dense_fine_table_stride1_ms_once']:.0f} ms", flush=True)
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if not identical:
        sys.exit("the records of the window search differ from the per-job calls'")


if __name__ == "__main__":
    main()
