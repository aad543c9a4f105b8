"""Times coarse-to-fine detection through the image pyramid (include/fdcm.h, "image pyramid") against the strided coarse pass it
replaces, on the refinement workload of README "Detections over pose windows": the first --templates templates of config 2'
(32 lines each), --coarse-angles coarse angles, a fine table of --fine-angles angles, --seeds seeds, boxes of (2 ha + 1) x 9 x 9
poses.  The maps are built from an image: config 2's scene lines rendered into a 1024 x 1024 uint8 frame (render()).

  refined    a build's exhaustive_detect_refined(coarse_stride=--coarse-stride) on the full-resolution map: the coarse call alone
             (exhaustive_detect_all), the whole chain, and the blocking build of the map
  pyramid    this build's exhaustive_detect_pyramid(level=--level, coarse_stride=1): the coarse call alone on the level's map, the
             whole chain, the blocking builds of the two maps, and image_pyramid alone (host in, host out)

Without --chain the tool runs the chains as processes in turn, --rounds times each: refined from --parent-root (the directory
that holds the parent commit's built openfdcm_amd), then pyramid from this tree, and writes every process's figures and how many
final detections of the two chains coincide.  Each figure is the median of --reps blocking calls after a warm-up, with the
smallest and the largest.

    python tools/pyramid_bench.py --parent-root DIR [--reps 5] [--rounds 2] [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 1024
RENDERING = ("config 2' scene lines (openfdcm_amd.synthetic.make_config('2p'): 200 lines in [0, 1023]^2) on a black 1024 x 1024 uint8 "
             "frame; pixel (x, y) = rint(255 * clip(1.5 - d, 0, 1)), d the distance from (x, y) to the nearest segment: strokes about "
             "two pixels wide with a one-pixel ramp, which the edge detector sees as two edges a few pixels apart")
EDGE = dict(threshold=60, low=30, smooth=1, min_pixels=8)


def render(scene):
    img = np.zeros((SIZE, SIZE), dtype=np.float64)
    for x0, y0, x1, y1 in np.asarray(scene, dtype=np.float64).T:
        xa, xb = int(max(0, np.floor(min(x0, x1)) - 2)), int(min(SIZE, np.ceil(max(x0, x1)) + 3))
        ya, yb = int(max(0, np.floor(min(y0, y1)) - 2)), int(min(SIZE, np.ceil(max(y0, y1)) + 3))
        yy, xx = np.mgrid[ya:yb, xa:xb]
        dx, dy = x1 - x0, y1 - y0
        u = np.clip(((xx - x0) * dx + (yy - y0) * dy) / max(dx * dx + dy * dy, 1e-12), 0, 1)
        d = np.hypot(xx - (x0 + u * dx), yy - (y0 + u * dy))
        img[ya:yb, xa:xb] = np.maximum(img[ya:yb, xa:xb], np.clip(1.5 - d, 0, 1))
    return np.rint(255 * img).astype(np.uint8)


def timed(fn, reps):
    fn()  # warm-up: workspaces, code objects, uploads
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "reps": reps}


def poses_of(openfdcm, dets, fine, piv):
    """(n, 4) int rows (tmpl, fine angle, x, y) of the final detections."""
    return openfdcm.pose_windows(dets, fine, fine, piv, 0, 0, 0)[:, [0, 1, 3, 4]].tolist()


def run_chain(args):
    sys.path.insert(0, os.path.abspath(args.package_root))
    import openfdcm_amd as openfdcm
    from openfdcm_amd import synthetic

    cfg, scene, tmpls = synthetic.make_config("2p")
    frame = render(scene)
    sub = tmpls[: args.templates]
    piv = openfdcm.template_pivots(sub)
    coarse = np.arange(args.coarse_angles) * (2 * np.pi / args.coarse_angles)
    fine = np.arange(args.fine_angles) * (2 * np.pi / args.fine_angles)
    params = openfdcm.Dt3CpuParameters(depth=cfg["depth"], dt3Coeff=5.0)
    pen = openfdcm.DefaultPenalty()
    inf = float("inf")
    res = {"chain": args.chain, "package": os.path.abspath(args.package_root), "templates": len(sub), "edge": EDGE,
           "frame_nonzero_pixels": int((frame > 0).sum())}
    fm0 = openfdcm.build_image_featuremap(frame, params, **EDGE)

    def build0():
        fm0._fm.rebuild_image(frame, EDGE["threshold"], low=EDGE["low"], smooth=EDGE["smooth"], min_pixels=EDGE["min_pixels"])
        return fm0._fm.build_timing()  # (waits for the build)

    _, res["build_level0_map"] = timed(build0, args.reps)
    common = dict(coarse_max_detections=args.seeds, penalty=pen, wrap=True, line_caps=args.line_caps, overlap=args.overlap,
                  max_detections=args.max_detections)
    if args.chain == "refined":
        s = args.coarse_stride
        seeds, res["coarse_call"] = timed(lambda: openfdcm.exhaustive_detect_all(
            fm0, sub, inf, overlap=1.0, stride=s, max_detections=args.seeds, penalty=pen, angles=coarse, line_caps=args.line_caps), args.reps)
        dets, res["whole_chain"] = timed(lambda: openfdcm.exhaustive_detect_refined(
            fm0, sub, inf, coarse, fine, s, args.half_angles, s, s, **common), args.reps)
        res["coarse_grid"] = list(openfdcm.rotation_window(fm0, sub, coarse, stride=s))
    else:
        L = args.level
        fml = openfdcm.build_image_featuremap_level(frame, L, params, **EDGE)

        def buildl():
            fml._fm.rebuild_image_level(frame, L, EDGE["threshold"], low=EDGE["low"], smooth=EDGE["smooth"], min_pixels=EDGE["min_pixels"])
            return fml._fm.build_timing()

        _, res["build_level_map"] = timed(buildl, args.reps)
        _, res["image_pyramid_host"] = timed(lambda: openfdcm.image_pyramid(frame, L), args.reps)
        small = openfdcm.scaled_templates(sub, L)
        caps_l = args.line_caps * 2.0 ** -L  # a line's cost falls with 4^-L, its scalar cap tau * length with 2^-L: the same cap is tau 2^-L
        seeds, res["coarse_call"] = timed(lambda: openfdcm.exhaustive_detect_all(
            fml, small, inf, overlap=1.0, stride=1, max_detections=args.seeds, penalty=pen, angles=coarse,
            pivot=piv * np.float32(2.0 ** -L), line_caps=caps_l), args.reps)
        dets, res["whole_chain"] = timed(lambda: openfdcm.exhaustive_detect_pyramid(
            fm0, fml, L, sub, inf, coarse, fine, args.half_angles, coarse_line_caps=caps_l, **common), args.reps)
        res["coarse_grid"] = list(openfdcm.rotation_window(fml, small, coarse, stride=1, pivot=piv * np.float32(2.0 ** -L)))
        res["level"], res["coarse_line_caps"] = L, caps_l
    res["seeds"], res["detections"] = int(len(seeds)), int(len(dets))
    res["poses"] = poses_of(openfdcm, dets, fine, piv)
    sc = dets.records()["score"]
    res["detection_scores"] = {"min": float(sc.min()), "median": float(np.median(sc)), "max": float(sc.max())} if len(sc) else {}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chain", choices=["refined", "pyramid"], default=None)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--templates", type=int, default=100)
    ap.add_argument("--coarse-angles", type=int, default=36)
    ap.add_argument("--coarse-stride", type=int, default=4)
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=800)
    ap.add_argument("--fine-angles", type=int, default=360)
    ap.add_argument("--half-angles", type=int, default=5)
    ap.add_argument("--overlap", type=float, default=0.3)
    ap.add_argument("--line-caps", type=float, default=3.0)
    ap.add_argument("--max-detections", type=int, default=1024)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a chain's process may take")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.chain:
        return run_chain(args)
    if not args.parent_root:
        ap.error("--parent-root is required: the directory that holds the parent commit's built openfdcm_amd")
    passed = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("reps", "templates", "coarse_angles", "coarse_stride", "level", "seeds",
                                                                     "fine_angles", "half_angles", "overlap", "line_caps", "max_detections")]
    runs = []
    for rnd in range(args.rounds):
        for chain, root in (("refined", args.parent_root), ("pyramid", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--chain", chain, "--package-root", root] + passed,
                                 capture_output=True, text=True, timeout=args.timeout)
            if out.returncode != 0:  # nothing more is started on the GPU after a process that failed
                sys.exit(f"{chain} of round {rnd} ended with {out.returncode}:\n{out.stdout}\n{out.stderr}")
            r = json.loads(out.stdout.strip().splitlines()[-1])
            r["round"], r["package"] = rnd, "the parent commit's build" if chain == "refined" else "this build"
            runs.append(r)
            print(chain, rnd, {k: v["median_ms"] for k, v in r.items() if isinstance(v, dict) and "median_ms" in v}, "detections", r["detections"],
                  flush=True)
    a = [tuple(p) for p in runs[0]["poses"]]
    b = [tuple(p) for p in runs[1]["poses"]]
    n_fine = args.fine_angles
    near = sum(any(p[0] == q[0] and min((p[1] - q[1]) % n_fine, (q[1] - p[1]) % n_fine) <= 1 and abs(p[2] - q[2]) <= 1 and abs(p[3] - q[3]) <= 1
                   for q in b) for p in a)
    res = {"workload": "README, Detections over pose windows: config 2' templates, image-built maps", "rendering": RENDERING,
           "protocol": f"median of {args.reps} blocking calls after a warm-up; refined (parent build) and pyramid (this build) as "
                       f"processes in turn, {args.rounds} times each",
           "arguments": {k: getattr(args, k) for k in ("templates", "coarse_angles", "coarse_stride", "level", "seeds", "fine_angles", "half_angles",
                                                        "overlap", "line_caps", "max_detections")},
           "detection_overlap": {"refined": len(a), "pyramid": len(b), "identical_pose": len(set(a) & set(b)),
                                 "refined_with_a_pyramid_detection_within_1px_1_fine_step": near},
           "same_detections_every_round": all(r["poses"] == runs[i % 2]["poses"] for i, r in enumerate(runs)),
           "runs": [{k: v for k, v in r.items() if k != "poses"} for r in runs],
           "poses_tmpl_angle_x_y": {"refined": [" ".join(map(str, p)) for p in a], "pyramid": [" ".join(map(str, p)) for p in b]}}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "poses_tmpl_angle_x_y"}))


if __name__ == "__main__":
    main()
