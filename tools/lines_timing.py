"""Times fdcm_lines_from_image (include/fdcm.h, "line segments from images") stage by stage on the four 1024 x 1024 synthetic
images of the image builds' measurements (tests/edge_ref.synthetic_image, seeds 1 - 4): edge parameters smooth = 1, low = 20,
high = 60 and then smooth = 0, depth 30, bucket 4, at least 8 pixels and 8 pixels of length.  Per image and setting: the median
over --reps calls after --warmup calls of every stage of fdcm_lines_last_timing (HIP events between the stages) and of the
call's wall time, and beside them the wall time of fdcm_edge_labels_ex alone on the same image.

    python tools/lines_timing.py [--reps 20] [--warmup 5] [--size 1024] [--smooth 1,0] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--smooth", default="1,0", help="the smoothings to run, in order")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import edge_ref
    import openfdcm_amd as fd
    from openfdcm_amd.engine import lines_last_timing
    rows = []
    for smooth in [int(v) for v in args.smooth.split(",")]:
        for seed in (1, 2, 3, 4):
            img = edge_ref.synthetic_image(args.size, args.size, seed)
            edge = dict(depth=30, threshold=60, low=20, smooth=smooth, min_pixels=1)
            stages, wall, wall_edges = [], [], []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                lines = fd.lines_from_image(img, **edge, bucket=4, line_pixels=8, line_length=8)
                t1 = time.perf_counter()
                lab = fd.edge_labels(img, **edge)
                t2 = time.perf_counter()
                if i >= args.warmup:
                    stages.append(lines_last_timing()); wall.append((t1 - t0) * 1e3); wall_edges.append((t2 - t1) * 1e3)
            row = {k: float(np.median([s[k] for s in stages])) for k in stages[0] if k != "n_lines"}
            row.update(smooth=smooth, seed=seed, n_lines=int(lines.shape[1]), edge_pixels=int((lab != 255).sum()),
                       call_wall_ms=float(np.median(wall)), edge_labels_ex_wall_ms=float(np.median(wall_edges)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"size": args.size, "reps": args.reps, "warmup": args.warmup, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
