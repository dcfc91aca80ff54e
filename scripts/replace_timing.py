#!/usr/bin/env python3
"""What a change of scene on a live handle costs next to a fresh handle (acn_scene_replace, acn_scene_set_params).

    python scripts/replace_timing.py [--reps 5] [--scenes wine_glass,hanging_lamp,diamond] [--package DIR] [--out FILE.json]

One process, after one throw-away handle (the first stream a process makes costs 85 - 100 ms and is nobody's business here).  Per
scene, `reps` rounds of four measurements, interleaved, wall clock around calls that wait for the device:
  a  upload + first frame + free           a fresh handle, the camera of this round
  b  replace (same kind) + frame           the scene re-made with the camera of this round, put on the warm handle
  c  set_params + frame                    the warm handle's camera moved on by half a step
  d  the steady frame                      the same frame again
The camera orbits the view target by 3 degrees per round, so b and c render frames a, d would cost the same for.  Frames are main
passes into a device buffer (acn_render_main_pass_dev).  The warm handle has rendered three frames before the first round: its queues
are sized and trimmed.  --package: the directory that holds the actinon_amd package to measure (default: this repository); a package
without Handle.replace gives a and d alone, which is how the parent commit is measured.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {
    "wine_glass": ("wine_glass", dict(image_width=1920, image_height=1080, path_samples=64, direct_samples=200)),
    "hanging_lamp": ("fixture:hanging_lamp", dict()),                                  # 600 x 800, the script's own sampling
    "diamond": ("diamond", dict(image_width=400, image_height=300, path_samples=50, direct_samples=50)),   # the size of the reference's video
}


def orbit(params, degrees):
    """camera_position and camera_view_direction turned about the top direction through the view target (actinon_amd.cameras.orbit_camera,
    repeated here so that a package from before it can be measured)"""
    import numpy as np
    pos = np.array([params.camera_position[i] for i in range(3)])
    view = np.array([params.camera_view_direction[i] for i in range(3)])
    axis = np.array([params.camera_top_direction[i] for i in range(3)])
    axis = axis / np.sqrt(axis @ axis)
    a = np.deg2rad(degrees)

    def turn(v):
        return v * np.cos(a) + np.cross(axis, v) * np.sin(a) + axis * (axis @ v) * (1.0 - np.cos(a))

    target = pos + view
    return dict(camera_position=tuple(float(x) for x in target + turn(pos - target)), camera_view_direction=tuple(float(x) for x in turn(view)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="wine_glass,hanging_lamp,diamond")
    ap.add_argument("--package", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.package)
    import torch
    import actinon_amd as A
    warm_api = hasattr(A.Handle, "replace")

    def make(name, degrees):
        builder, ov = SCENES[name]
        if builder.startswith("fixture:"):
            path = os.path.join(ROOT, "tests", "golden", "scenes", builder.split(":")[1] + ".npz")
            flat = A.Flat.load(path, **ov)
            return A.Flat.load(path, **dict(ov, **orbit(flat.params, degrees)))
        sc = A.Scene.build(builder, **ov)
        sc.set(**orbit(sc.prm, degrees))
        return sc.flatten()

    def frame(h, n, out):
        h.render_main_pass_dev(0, n, out.data_ptr(), linear=True)

    def timed(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    throw_away = A.Handle(make("diamond", 0.0))
    throw_away.close()
    result = {"package": os.path.abspath(args.package), "reps": args.reps, "unit": "ms, wall clock", "scenes": {}}
    for name in args.scenes.split(","):
        flat0 = make(name, 0.0)
        n = int(flat0.params.image_width * flat0.params.image_height)
        out = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        warm = A.Handle(flat0)
        for _ in range(3):
            frame(warm, n, out)
        ms = {k: [] for k in ("a", "b", "c", "d", "replace_alone", "set_params_alone")}
        info = []
        for rep in range(args.reps):
            flat = make(name, 3.0 * (rep + 1))

            def cold():
                h = A.Handle(flat)
                frame(h, n, out)
                h.close()
            ms["a"].append(timed(cold))
            if warm_api:
                t = timed(lambda: warm.replace(flat))
                ms["replace_alone"].append(t)
                ms["b"].append(t + timed(lambda: frame(warm, n, out)))
                step = orbit(flat.params, 1.5)
                t = timed(lambda: warm.set_params(**step))
                ms["set_params_alone"].append(t)
                ms["c"].append(t + timed(lambda: frame(warm, n, out)))
                info.append(warm.info())
            ms["d"].append(timed(lambda: frame(warm, n, out)))
        warm.close()
        del out
        torch.cuda.empty_cache()
        entry = {"pixels": n, "path_samples": int(flat0.params.path_samples), "direct_samples": int(flat0.params.direct_samples)}
        for k, v in ms.items():
            if v:
                entry[k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
        if info:
            entry["info_after_last_round"] = info[-1]
        result["scenes"][name] = entry
        print(name, {k: round(v["median"], 2) for k, v in entry.items() if isinstance(v, dict) and "median" in v}, file=sys.stderr)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
