"""Times the exhaustive translation search (include/fdcm.h, "exhaustive translation search") on config 2': the feature map
and the 1000 x 32-line synthetic templates bench.py uses, every template over its default window (exhaustive_window), at
stride 1, 2 and 4 with k = 1 and 8, and the peaks (fdcm_search_exhaustive_peaks) at k = 8 with radii 1, 8 and 32 on the
same grids, each beside the top-k call of the same k.  Rotations (fdcm_search_exhaustive_rotations): the first
--rot-templates templates, --rot-angles angles evenly over the circle with wrap, pivot the bounding-box centre, k = --peak-k,
(rx = ry, ra) in --rot-cases at --rot-strides, each beside fdcm_search_exhaustive (ra = rx = 0) or
fdcm_search_exhaustive_peaks (r = rx) of the same k on the host-rotated line sets passed as one template set: the same
scoring work without the rotation code.  The host preparation (rotation, bins, boxes) is timed alone as a call on a
1 x 1 grid.

For every case it prints the wall time of one blocking fdcm_search_exhaustive call (median of --reps after a warm-up),
the admissible translations scored (the sum over templates of the window's points inside each template's admissible
box), and the lookup rate: 2 lookups per template line and admissible translation.  The CPU figure is the oracle's
evaluate<Dt3Cpu> (the reference's code, one host thread) on a random sample of admissible translations, the same
lookups per translation.

--line-caps TAU gives every template line the cap TAU * its length (include/fdcm.h, "Per-line caps and line costs"): the
same cases on the kernels that clamp each line's cost.  Off by default.

    python tools/exhaustive_bench.py [--reps 5] [--cpu-sample 20000] [--radii 1,8,32] [--rot-cases 0:0,8:1,8:2]
                                     [--only-rotations] [--line-caps TAU] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def boxes(dev, tmpls):
    """Per template its admissible box (x0, y0, x1, y1), from the stride-1 window of the template alone."""
    from openfdcm_amd.engine import DeviceTemplates
    out = []
    for t in tmpls:
        ts = DeviceTemplates([t])
        x0, y0, nx, ny, _, _ = dev.exhaustive_window(ts, 1, 1).as_tuple()
        ts.close()
        out.append((x0, y0, x0 + nx - 1, y0 + ny - 1) if nx else None)
    return out


def points_in(lo, hi, g0, n, s):
    """Grid points g0 + i s (0 <= i < n) inside [lo, hi]."""
    i0 = max(0, -((g0 - lo) // s))
    i1 = min(n - 1, (hi - g0) // s)
    return max(0, i1 - i0 + 1)


def rotation_cases(args, dev, tmpls, timed):
    """The rotation search against the translation-only calls on the host-rotated line sets (module docstring)."""
    import openfdcm_amd as openfdcm
    from openfdcm_amd.engine import DeviceTemplates
    sub = tmpls[: args.rot_templates]
    angles = np.arange(args.rot_angles) * (2 * np.pi / args.rot_angles)
    cs = openfdcm._angles(angles)
    piv = openfdcm._pivots(sub, "center", len(sub))
    tset = DeviceTemplates(sub, line_caps=args.line_caps)
    caps = None if args.line_caps is None else [c for c in openfdcm.line_caps(sub, args.line_caps) for _ in cs]  # a line keeps its cap
    rs = DeviceTemplates([openfdcm_rotate(t, c, s, p) for t, p in zip(sub, piv) for c, s in cs], line_caps=caps)
    k = args.peak_k
    cases = [tuple(int(v) for v in c.split(":")) for c in args.rot_cases.split(",")]
    out = {"templates": len(sub), "angles": len(cs), "k": k, "wrap": True, "rows": []}
    prep_ms, _, _ = timed(lambda: dev.exhaustive_rotation_search(tset, (0, 0, 1, 1, 1, 1), cs, piv, k=k))
    out["host_preparation_ms"] = round(prep_ms, 3)
    print(f"rotations: {len(sub)} templates x {len(cs)} angles, host preparation (1 x 1 grid call) {prep_ms:.2f} ms", flush=True)
    for s in [int(v) for v in args.rot_strides.split(",")]:
        grid = dev.exhaustive_rotations_window(tset, cs, piv, s, s).as_tuple()
        for r, ra in cases:
            ms, ms_min, recs = timed(lambda: dev.exhaustive_rotation_search(tset, grid, cs, piv, k=k, rx=r, ry=r, ra=ra, wrap=True))
            if r == 0 and ra == 0:
                base_ms, _, _ = timed(lambda: dev.exhaustive_search(rs, grid, k=k))
                base = "exhaustive_search"
            else:
                base_ms, _, _ = timed(lambda: dev.exhaustive_peaks(rs, grid, k=k, rx=r, ry=r))
                base = f"exhaustive_peaks r {r}"
            out["rows"].append({"stride": s, "r": r, "ra": ra, "grid": list(grid), "ms_per_call": round(ms, 3),
                                "ms_min": round(ms_min, 3), "baseline": base, "baseline_ms_per_call": round(base_ms, 3),
                                "ratio": round(ms / base_ms, 3), "records": int(len(recs)),
                                "host_preparation_share": round(prep_ms / ms, 3)})
            print(f"rotations stride {s} r {r} ra {ra}: {ms:.2f} ms/call (min {ms_min:.2f}), {base} on the host-rotated set "
                  f"{base_ms:.2f} ms: {ms / base_ms:.3f}x, {len(recs)} records, host preparation {prep_ms / ms:.1%}", flush=True)
    return out


def openfdcm_rotate(tm, c, s, p):
    """The rotated line set M_a(t) (include/fdcm.h, "Rotations"), float32 left to right."""
    c, s, px, py = np.float32(c), np.float32(s), np.float32(p[0]), np.float32(p[1])
    ns = -s
    mx, my = px - (c * px + ns * py), py - (s * px + c * py)
    out = np.empty_like(tm)
    for r in (0, 2):
        out[r] = (c * tm[r] + ns * tm[r + 1]) + mx
        out[r + 1] = (s * tm[r] + c * tm[r + 1]) + my
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-sample", type=int, default=20000, help="translations the oracle scores on the host")
    ap.add_argument("--strides", default="1,2,4")
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--radii", default="1,8,32", help="peak radii (rx = ry); empty: no peaks cases")
    ap.add_argument("--peak-k", type=int, default=8)
    ap.add_argument("--rot-templates", type=int, default=100)
    ap.add_argument("--rot-angles", type=int, default=36)
    ap.add_argument("--rot-strides", default="1,2")
    ap.add_argument("--rot-cases", default="0:0,8:1,8:2", help="rx=ry:ra pairs; empty: no rotation cases")
    ap.add_argument("--only-rotations", action="store_true", help="skip the translation-only cases and the CPU figure")
    ap.add_argument("--line-caps", type=float, default=None, metavar="TAU", help="cap every line's cost at TAU * its length")
    ap.add_argument("--json", default=None, help="also write the results here")
    args = ap.parse_args()

    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    from oracle import oracle as O

    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    tset = DeviceTemplates(tmpls, line_caps=args.line_caps)
    n_lines = int(sum(t.shape[1] for t in tmpls))
    bx = boxes(dev, tmpls)
    rows = []
    for s in [int(v) for v in args.strides.split(",")] if not args.only_rotations else []:
        grid = dev.exhaustive_window(tset, s, s).as_tuple()
        x0, y0, nx, ny, sx, sy = grid
        adm = [0 if b is None else points_in(b[0], b[2], x0, nx, sx) * points_in(b[1], b[3], y0, ny, sy) for b in bx]
        lookups = 2 * sum(a * t.shape[1] for a, t in zip(adm, tmpls))
        for k in [int(v) for v in args.ks.split(",")]:
            dev.exhaustive_search(tset, grid, k=k)  # warm-up: workspaces, code objects
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                recs = dev.exhaustive_search(tset, grid, k=k)
                times.append(time.perf_counter() - t0)
            ms = float(np.median(times)) * 1e3
            rows.append({"stride": s, "k": k, "grid": list(grid), "grid_points": nx * ny, "admissible": int(sum(adm)),
                         "lookups": int(lookups), "ms_per_call": round(ms, 3), "ms_min": round(min(times) * 1e3, 3),
                         "lookups_per_s": float(f"{lookups / (ms * 1e-3):.4g}"), "records": int(len(recs))})
            print(f"stride {s} k {k}: grid {nx}x{ny}, {sum(adm)} admissible translations, {lookups:.3g} lookups, "
                  f"{ms:.2f} ms/call (min {min(times) * 1e3:.2f}), {lookups / (ms * 1e-3):.3g} lookups/s", flush=True)

    def timed(call):
        call()  # warm-up: workspaces, code objects
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = call()
            times.append(time.perf_counter() - t0)
        return float(np.median(times)) * 1e3, min(times) * 1e3, out

    peaks = []
    radii = [int(v) for v in args.radii.split(",") if v]
    for s in [int(v) for v in args.strides.split(",")] if radii and not args.only_rotations else []:
        grid = dev.exhaustive_window(tset, s, s).as_tuple()
        k = args.peak_k
        top_ms, _, _ = timed(lambda: dev.exhaustive_search(tset, grid, k=k))
        for r in radii:
            ms, ms_min, recs = timed(lambda: dev.exhaustive_peaks(tset, grid, k=k, rx=r, ry=r))
            peaks.append({"stride": s, "k": k, "r": r, "grid": list(grid), "ms_per_call": round(ms, 3), "ms_min": round(ms_min, 3),
                          "topk_ms_per_call": round(top_ms, 3), "ratio_to_topk": round(ms / top_ms, 3), "records": int(len(recs))})
            print(f"peaks stride {s} k {k} r {r}: {ms:.2f} ms/call (min {ms_min:.2f}), top-k {top_ms:.2f} ms: "
                  f"{ms / top_ms:.2f}x, {len(recs)} records", flush=True)

    rot = rotation_cases(args, dev, tmpls, timed) if args.rot_cases else {}
    if args.only_rotations:
        res = {"workload": "config 2' rotations", "rotations": rot}
        if args.line_caps is not None:
            res["line_caps_tau"] = args.line_caps
        print(json.dumps(res))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
        return

    # the same work on the host: the oracle's evaluate (one thread) on random admissible translations of random templates
    orc = O.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"], nthreads=16)
    rng = np.random.default_rng(7)
    per = 500
    picks = [t for t in rng.permutation(len(tmpls)) if bx[t] is not None][: max(1, args.cpu_sample // per)]
    cpu_s, cpu_lookups = 0.0, 0
    for t in picks:
        b = bx[t]
        tr = np.stack([rng.integers(b[0], b[2] + 1, per), rng.integers(b[1], b[3] + 1, per)], axis=1).astype(np.float32)
        t0 = time.perf_counter()
        O.evaluate(orc, tmpls[t], tr)
        cpu_s += time.perf_counter() - t0
        cpu_lookups += 2 * tmpls[t].shape[1] * per
    cpu = {"threads": 1, "translations": per * len(picks), "lookups": cpu_lookups, "seconds": round(cpu_s, 4),
           "lookups_per_s": float(f"{cpu_lookups / cpu_s:.4g}")}
    print(f"CPU (oracle evaluate<Dt3Cpu>, 1 thread): {cpu['translations']} translations, {cpu_lookups:.3g} lookups in "
          f"{cpu_s * 1e3:.1f} ms: {cpu['lookups_per_s']:.3g} lookups/s", flush=True)
    for r in rows:
        r["speedup_vs_cpu_1thread"] = round(r["lookups_per_s"] / cpu["lookups_per_s"], 1)
    res = {"workload": "config 2': 1024x1024 scene (200 lines, seed 1), depth 30, L2, padding 1.0; 1000 templates x 32 lines "
                       "(seed 2), default window per stride", "template_lines": n_lines, "gpu": rows, "peaks": peaks, "rotations": rot,
           "cpu": cpu}
    if args.line_caps is not None:
        res["line_caps_tau"] = args.line_caps
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
