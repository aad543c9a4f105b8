"""Templates from a mesh (include/fdcm.h, "Templates from a mesh"), timed: a bumpy icosphere of 20480 faces (concavities, so
faces hide faces), 1000 hemisphere views at a scale that makes it about 300 pixels wide.

    python tools/mesh_templates_bench.py [--views 1000] [--referee-views 3] [--out profiles/mesh_templates_bench.json]
    python tools/mesh_templates_bench.py --distance 5 [--focal F] [--parent DIR]     the pinhole views beside the orthographic ones

Two fresh processes, one after another, each: a warm-up call, then the median wall time of 5 blocking templates_from_mesh calls
(upload, all passes, download).  The first process also times the numpy referee (tests/mesh_ref.py, the only statement of the
templates that existed before) on the first views and compares: the tool fails unless they agree byte for byte.  Prints one
JSON line and writes it to --out.

--distance D (in diagonals of the mesh's bounding box; --focal in pixels, by default SCALE times the distance, which keeps the
size on the image): "Templates from a mesh: pinhole views".  Fresh processes in turn, twice over: with --parent DIR (another
checkout of this project, built) that checkout's default call, then this one's default call and, in each of the modes {items,
exact} x {no joining, 0.5}, the orthographic and the pinhole call.  The first process compares the pinhole lines of the first
--referee-views views with the referee (tests/mesh_cam_ref.py).  Writes profiles/mesh_camera_bench.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.abspath(sys.argv[sys.argv.index("--package") + 1]) if "--package" in sys.argv else ROOT   # a child's checkout
sys.path.insert(0, PACKAGE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SCALE, MIN_LENGTH, CALLS = 110.0, 2.0, 5


def bumpy_sphere():
    import numpy as np
    import mesh_cases as MC
    return MC.icosphere(5, bump=lambda p: 1.0 + 0.2 * np.sin(4.0 * p[:, 0]) * np.sin(4.0 * p[:, 1]) + 0.15 * np.cos(5.0 * p[:, 2]))


def timed_mode(engine, mesh, views, visibility, join):
    """A warm-up call, then CALLS blocking calls in the mode: (record of the times, line counts and kept length; lines, offsets)."""
    import numpy as np
    rec, offsets = engine.mesh_view_lines(mesh, views, SCALE, None, MIN_LENGTH, visibility, join)
    times = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        engine.templates_from_mesh(mesh, views, SCALE, None, MIN_LENGTH, visibility, join)
        times.append(time.perf_counter() - t0)
    length = float(np.hypot(rec[:, 2].astype(np.float64) - rec[:, 0], rec[:, 3].astype(np.float64) - rec[:, 1]).sum())
    return {"visibility": visibility, "join_tolerance": join, "median_ms": 1e3 * statistics.median(times), "min_ms": 1e3 * min(times),
            "max_ms": 1e3 * max(times), "lines": int(len(rec)), "kept_length_px": length}, rec, offsets


def child_mode(n_views, referee_views, visibility, join):
    """--visibility / --join: the mode beside the default mode in the same process; the referee of the mode on the first views."""
    import numpy as np
    import mesh_join_ref as JR
    import mesh_ref as MR
    from openfdcm_amd import engine
    v, f = bumpy_sphere()
    mesh = engine.Mesh(v, f)
    views = engine.view_rotations(n_views)
    out = {"default": timed_mode(engine, mesh, views, "items", None)[0], "views": n_views, "scale": SCALE, "faces": int(len(f))}
    out["mode"], rec, offsets = timed_mode(engine, mesh, views, visibility, join)
    if referee_views:
        ref = MR.Mesh(v, f, float(np.cos(np.deg2rad(30))))
        want, want_off = JR.views_lines(ref, views[:referee_views], np.float32(SCALE), mesh.default_depth_tolerance(), MIN_LENGTH, visibility, join)
        out["referee_views"] = referee_views
        out["referee_equal"] = bool(want_off.tolist() == offsets[:referee_views + 1].tolist() and want.tobytes() == rec[:want_off[-1]].tobytes())
    print("mesh_templates_bench_child " + json.dumps(out), flush=True)
    return 0 if out.get("referee_equal", True) else 1


def _median_ms(call):
    call()      # warm-up
    times = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(times), "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times)}


def child_default(n_views):
    """The default call alone, with whatever checkout --package names: what the parent commit has too."""
    from openfdcm_amd import engine
    v, f = bumpy_sphere()
    mesh = engine.Mesh(v, f)
    views = engine.view_rotations(n_views)
    out = {"package": "this" if PACKAGE == ROOT else "parent", "default": _median_ms(lambda: engine.templates_from_mesh(mesh, views, SCALE, None, MIN_LENGTH))}
    out["default"]["lines"] = int(engine.mesh_view_lines(mesh, views, SCALE, None, MIN_LENGTH)[1][-1])
    print("mesh_templates_bench_child " + json.dumps(out), flush=True)
    return 0


def child_camera(n_views, referee_views, distance, focal):
    import numpy as np
    import mesh_cam_ref as CR
    import mesh_ref as MR
    from openfdcm_amd import engine
    v, f = bumpy_sphere()
    mesh = engine.Mesh(v, f)
    views = engine.view_rotations(n_views)
    d = v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)
    dist = distance * float(np.sqrt(d @ d))
    focal = SCALE * dist if focal is None else focal
    pos = engine.view_positions(n_views, dist)
    out = {"package": "this", "views": n_views, "faces": int(len(f)), "scale": SCALE, "focal": focal, "distance": dist,
           "default": _median_ms(lambda: engine.templates_from_mesh(mesh, views, SCALE, None, MIN_LENGTH)), "modes": {}}
    for visibility in ("items", "exact"):
        for join in (None, 0.5):
            o = _median_ms(lambda: engine.templates_from_mesh(mesh, views, SCALE, None, MIN_LENGTH, visibility, join))
            c = _median_ms(lambda: engine.templates_from_mesh(mesh, views, None, None, MIN_LENGTH, visibility, join, focal=focal, positions=pos))
            rec, offsets = engine.mesh_view_lines(mesh, views, None, None, MIN_LENGTH, visibility, join, focal=focal, positions=pos)
            c["lines"] = int(len(rec))
            c["width_px"] = float(max(rec[:, [0, 2]].max() - rec[:, [0, 2]].min(), rec[:, [1, 3]].max() - rec[:, [1, 3]].min()))
            o["lines"] = int(engine.mesh_view_lines(mesh, views, SCALE, None, MIN_LENGTH, visibility, join)[1][-1])
            out["modes"]["%s,join=%s" % (visibility, join)] = {"orthographic": o, "pinhole": c}
            if referee_views and visibility == "items" and join is None:
                ref = MR.Mesh(v, f, float(np.cos(np.deg2rad(30))))
                want = [CR.view_lines(ref, views[i], pos[i], np.float32(focal), mesh.default_near(), mesh.default_depth_tolerance(), MIN_LENGTH)
                        for i in range(referee_views)]
                out["referee_views"] = referee_views
                out["referee_equal"] = bool(np.concatenate(want).tobytes() == rec[:offsets[referee_views]].tobytes())
    print("mesh_templates_bench_child " + json.dumps(out), flush=True)
    return 0 if out.get("referee_equal", True) else 1


def main_camera(a):
    """Processes in turn, one after another; nothing is started after a failure."""
    runs = []
    for i in range(2):
        for package in ([a.parent] if a.parent else []) + [ROOT]:
            cmd = [sys.executable, os.path.abspath(__file__), "--views", str(a.views), "--child", str(i), "--package", package]
            if package == ROOT:
                cmd += ["--referee-views", str(a.referee_views), "--distance", str(a.distance)] + (["--focal", str(a.focal)] if a.focal else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            lines = [l for l in p.stdout.splitlines() if l.startswith("mesh_templates_bench_child ")]
            if p.returncode != 0 or not lines:
                sys.stderr.write(p.stdout + p.stderr)
                print(json.dumps({"error": "a process failed or disagrees with the referee"}))
                return 1
            runs.append(json.loads(lines[-1].split(" ", 1)[1]))
    mine = [r for r in runs if "modes" in r]
    result = {"bench": "mesh_camera", "processes": runs, "referee_equal": mine[0].get("referee_equal"),
              "default_median_ms": [r["default"]["median_ms"] for r in mine],
              "parent_default_median_ms": [r["default"]["median_ms"] for r in runs if "modes" not in r],
              "median_ms": {k: {p: [r["modes"][k][p]["median_ms"] for r in mine] for p in ("orthographic", "pinhole")} for k in mine[0]["modes"]}}
    print(json.dumps(result))
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return 0


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
    ap.add_argument("--visibility", choices=("items", "exact"), default=None, help="time this mode beside the default mode")
    ap.add_argument("--join", type=float, default=None, help="the joining tolerance in pixels of the mode timed")
    ap.add_argument("--distance", type=float, default=None, help="pinhole views: the camera's distance in bounding-box diagonals")
    ap.add_argument("--focal", type=float, default=None, help="pinhole views: the focal length in pixels (default: SCALE times the distance)")
    ap.add_argument("--parent", default=None, help="pinhole views: a built checkout whose default call is timed in turn")
    ap.add_argument("--package", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.distance is not None or a.package is not None:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "mesh_camera_bench.json")
        if a.child >= 0 and a.distance is None:
            return child_default(a.views)
        if a.child >= 0:
            return child_camera(a.views, a.referee_views if a.child == 0 else 0, a.distance, a.focal)
        return main_camera(a)
    mode = a.visibility is not None or a.join is not None
    if mode and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "mesh_exact_join_bench.json")
    if a.child >= 0 and mode:
        return child_mode(a.views, a.referee_views if a.child == 0 else 0, a.visibility or "items", a.join)
    if a.child >= 0:
        return child(a.views, a.referee_views if a.child == 0 else 0)
    runs = []
    extra = (["--visibility", a.visibility] if a.visibility else []) + (["--join", str(a.join)] if a.join is not None else [])
    for i in range(2):      # one after another; nothing is started after a failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--views", str(a.views), "--referee-views", str(a.referee_views),
                            "--child", str(i)] + extra, capture_output=True, text=True, timeout=900)
        lines = [l for l in p.stdout.splitlines() if l.startswith("mesh_templates_bench_child ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout + p.stderr)
            print(json.dumps({"error": "process %d failed or disagrees with the referee" % i}))
            return 1
        runs.append(json.loads(lines[-1].split(" ", 1)[1]))
    if mode:        # one mode per invocation: its record is added to the file's, keyed by the mode
        key = "%s,join=%s" % (a.visibility or "items", a.join)
        result = {"bench": "mesh_exact_join", "mode": key, "processes": runs, "referee_equal": runs[0].get("referee_equal"),
                  "median_ms": [r["mode"]["median_ms"] for r in runs], "default_median_ms": [r["default"]["median_ms"] for r in runs],
                  "lines": runs[0]["mode"]["lines"], "kept_length_px": runs[0]["mode"]["kept_length_px"],
                  "default_lines": runs[0]["default"]["lines"], "default_kept_length_px": runs[0]["default"]["kept_length_px"]}
        print(json.dumps(result))
        allr = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                allr = json.load(fh)
        allr[key] = result
        with open(a.out, "w") as fh:
            json.dump(allr, fh, indent=1)
            fh.write("\n")
        return 0
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
