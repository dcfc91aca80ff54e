#!/usr/bin/env python3
"""Times the gradient cycles of the render driver on its two loops: on host arrays (acn_scene_s_host_cycles_g = 1) and on a
device-resident frame (0).  The workload is the wine glass scene at its script's settings (400 x 400, 100 cycles, 2 samples, threshold
0.03) and at 1920 x 1080 with 20 cycles.

    python scripts/time_frame_cycles.py [--rounds 5] [--sizes 400x400x100,1920x1080x20] [--out profiles/r23/frame_cycles.json]

Every timed image comes from a process of its own: it uploads a kept handle, renders one warm-up image on it and then times
create_image_file of the same scene.  The processes alternate host, frame, host, frame, ...; per path the median and the spread (min,
max) of the wall times are reported.  One more process per size drives the frame's cycles from Python and times plan, render, push and
image + file of every cycle on their own: the split of a cycle.  The host loop's time outside the render call is its wall time minus
the render time of the same positions measured there (its copies through the host form are therefore counted as outside).
--key-repeats N times acn_frame_plan with nothing flagged (key + select, no jitter) N times at each size."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene_of(A, width, height, cycles):
    sc = A.Scene.build("wine_glass", image_width=width, image_height=height)
    sc.set(gradient_cycles=cycles)
    return sc


def child_image(path, width, height, cycles):
    import actinon_amd as A
    A.set_host_cycles(path == "host")
    sc = scene_of(A, width, height, cycles)
    with tempfile.TemporaryDirectory() as tmp, A.KeptHandle() as keep:
        t0 = time.perf_counter()
        sc.create_image_file(os.path.join(tmp, "warm.pnm"), keep=keep)
        t1 = time.perf_counter()
        sc.create_image_file(os.path.join(tmp, "timed.pnm"), keep=keep)
        t2 = time.perf_counter()
        digest = __import__("hashlib").sha256(open(os.path.join(tmp, "timed.pnm"), "rb").read()).hexdigest()
    return dict(path=path, warm_s=t1 - t0, wall_s=t2 - t1, sha256=digest)


def child_split(width, height, cycles, key_repeats):
    import actinon_amd as A
    from actinon_amd._lib import host
    sc = scene_of(A, width, height, cycles)
    thr, K = sc.s.gradient_threshold ** 2, int(sc.s.gradient_samples)
    h = A.Handle(sc.flatten())
    steps = dict(plan=[], render=[], push=[], image_file=[])
    flagged_all = []
    with tempfile.TemporaryDirectory() as tmp, h.frame() as f:
        file = os.path.join(tmp, "split.pnm").encode()
        for rep in range(2):                                   # the first round warms the handle
            f.upload(__import__("numpy").zeros((width * height, 6)))
            for s in steps.values():
                s.clear()
            flagged_all.clear()
            t0 = time.perf_counter()
            f.main_pass()
            main_s = time.perf_counter() - t0
            rval = 21943294
            for _ in range(cycles):
                t = [time.perf_counter()]
                flagged, rval = f.plan(thr, K, rval)
                t.append(time.perf_counter())
                f.render()
                t.append(time.perf_counter())
                f.push()
                t.append(time.perf_counter())
                rgb8 = f.image(rgb=False)[1]
                host.acn_write_pnm8(file, rgb8.ctypes.data, width, height)
                t.append(time.perf_counter())
                for name, a, b in zip(steps, t, t[1:]):
                    steps[name].append(b - a)
                flagged_all.append(flagged)
        key = []
        for _ in range(key_repeats):
            t0 = time.perf_counter()
            f.plan(float("inf"), 1, 0)
            key.append(time.perf_counter() - t0)
            f.push()
    h.close()
    out = dict(main_s=main_s, cycles=cycles, flagged_median=statistics.median(flagged_all), flagged_max=max(flagged_all),
               render_total_s=sum(steps["render"]))
    for name, v in steps.items():
        out[name + "_ms_median"] = 1e3 * statistics.median(v)
        out[name + "_ms_total"] = 1e3 * sum(v)
    if key:
        out["key_select_ms_median"] = 1e3 * statistics.median(key)
        out["key_select_ms_min"] = 1e3 * min(key)
    return out


def run_child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit(f"child {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="400x400x100,1920x1080x20")
    ap.add_argument("--key-repeats", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--size", default=None)
    a = ap.parse_args()
    if a.child:
        w, h, c = map(int, a.size.split("x"))
        res = child_split(w, h, c, a.key_repeats) if a.child == "split" else child_image(a.child, w, h, c)
        print(json.dumps(res))
        return
    report = {}
    for size in a.sizes.split(","):
        w, h, c = map(int, size.split("x"))
        runs = {"host": [], "frame": []}
        for _ in range(a.rounds):
            for path in ("host", "frame"):
                runs[path].append(run_child(["--child", path, "--size", size]))
        split = run_child(["--child", "split", "--size", size, "--key-repeats", str(a.key_repeats)])
        digests = {r["sha256"] for rs in runs.values() for r in rs}
        entry = dict(width=w, height=h, cycles=c, same_bytes=len(digests) == 1, split=split)
        for path, rs in runs.items():
            walls = [r["wall_s"] for r in rs]
            entry[path] = dict(wall_s=walls, median_s=statistics.median(walls), min_s=min(walls), max_s=max(walls))
        entry["host_outside_render_ms_per_cycle"] = 1e3 * (entry["host"]["median_s"] - split["main_s"] - split["render_total_s"]) / c
        entry["frame_outside_render_ms_per_cycle"] = (split["plan_ms_total"] + split["push_ms_total"] + split["image_file_ms_total"]) / c
        report[size] = entry
        print(json.dumps({size: entry}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
