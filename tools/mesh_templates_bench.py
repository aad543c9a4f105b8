"""Templates from a mesh (include/fdcm.h, "Templates from a mesh"), timed: a bumpy icosphere of 20480 faces (concavities, so
faces hide faces), 1000 hemisphere views at a scale that makes it about 300 pixels wide.

    python tools/mesh_templates_bench.py [--views 1000] [--referee-views 3] [--out profiles/mesh_templates_bench.json]

Two fresh processes, one after another, each: a warm-up call, then the median wall time of 5 blocking templates_from_mesh calls
(upload, all passes, download).  The first process also times the numpy referee (tests/mesh_ref.py, the only statement of the
templates that existed before) on the first views and compares: the tool fails unless they agree byte for byte.  Prints one
JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SCALE, MIN_LENGTH, CALLS = 110.0, 2.0, 5


def bumpy_sphere():
    import numpy as np
    import mesh_cases as MC
    return MC.icosphere(5, bump=lambda p: 1.0 + 0.2 * np.sin(4.0 * p[:, 0]) * np.sin(4.0 * p[:, 1]) + 0.15 * np.cos(5.0 * p[:, 2]))


def child(n_views, referee_views):
    import numpy as np
    import mesh_ref as MR
    from openfdcm_amd import engine
    v, f = bumpy_sphere()
    mesh = engine.Mesh(v, f)
    views = engine.view_rotations(n_views)
    rec, offsets = engine.mesh_view_lines(mesh, views, SCALE, None, MIN_LENGTH)      # warm-up
    times = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        tm = engine.templates_from_mesh(mesh, views, SCALE, None, MIN_LENGTH)
        times.append(time.perf_counter() - t0)
    assert sum(t.shape[1] for t in tm) == len(rec) == offsets[-1]
    width = float(max(rec[:, [0, 2]].max() - rec[:, [0, 2]].min(), rec[:, [1, 3]].max() - rec[:, [1, 3]].min()))
    out = {"median_ms": 1e3 * statistics.median(times), "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times), "lines": int(len(rec)),
           "faces": int(len(f)), "vertices": int(len(v)), "edges": int(mesh.n_edges), "sharp_edges": int(mesh.n_sharp), "views": n_views,
           "scale": SCALE, "width_px": width}
    if referee_views:
        ref = MR.Mesh(v, f, float(np.cos(np.deg2rad(30))))
        t0 = time.perf_counter()
        want, want_off = MR.views_lines(ref, views[:referee_views], np.float32(SCALE), mesh.default_depth_tolerance(), MIN_LENGTH)
        out["referee_views"] = referee_views
        out["referee_ms_per_view"] = 1e3 * (time.perf_counter() - t0) / referee_views
        out["referee_lines"] = int(len(want))
        equal = want_off.tolist() == offsets[:referee_views + 1].tolist() and want.tobytes() == rec[:want_off[-1]].tobytes()
        out["referee_equal"] = bool(equal)
    print("mesh_templates_bench_child " + json.dumps(out), flush=True)
    return 0 if out.get("referee_equal", True) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--referee-views", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_templates_bench.json"))
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child >= 0:
        return child(a.views, a.referee_views if a.child == 0 else 0)
    runs = []
    for i in range(2):      # one after another; nothing is started after a failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--views", str(a.views), "--referee-views", str(a.referee_views),
                            "--child", str(i)], capture_output=True, text=True, timeout=900)
        lines = [l for l in p.stdout.splitlines() if l.startswith("mesh_templates_bench_child ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout + p.stderr)
            print(json.dumps({"error": "process %d failed or disagrees with the referee" % i}))
            return 1
        runs.append(json.loads(lines[-1].split(" ", 1)[1]))
    result = {"bench": "mesh_templates", "processes": runs, "median_ms": [r["median_ms"] for r in runs],
              "ms_per_view": [r["median_ms"] / a.views for r in runs], "lines": runs[0]["lines"],
              "referee_ms_per_view": runs[0].get("referee_ms_per_view"), "referee_equal": runs[0].get("referee_equal")}
    print(json.dumps(result))
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
