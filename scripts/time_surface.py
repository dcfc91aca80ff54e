#!/usr/bin/env python3
"""Surface calls against the cheapest render of the same rays.

    python scripts/time_surface.py [--steps 10] [--out FILE]

bench.py's frame (wine_glass 1920x1080): acn_surface_positions_dev over the frame's positions in both modes on one warm handle,
device-resident buffers, the caller's stream, the host clock between two device synchronisations.  The yardstick is code this
library had before the surface calls: acn_render_main_pass_dev on a second handle of the same scene with trace_depth 1 and no
path or direct samples (shade_hit still takes one sample per light) -- the same root traversal per pixel, then shading.  Next
to FOLLOW stands the full-depth render without samples.  The four calls alternate step by step.  Prints one JSON line (and
writes it to --out)."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--yardstick-only", action="store_true", help="time the two render calls alone (runs on a library without surface calls)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A

    W, H = 1920, 1080
    n = W * H
    build = lambda **kw: A.Scene.build("wine_glass", image_width=W, image_height=H, **kw).flatten()
    flat = build(path_samples=64, direct_samples=200)
    depth = int(flat.params.trace_depth)
    h = A.Handle(flat)
    h_first = A.Handle(build(path_samples=0, direct_samples=0, trace_depth=1))
    h_chain = A.Handle(build(path_samples=0, direct_samples=0))
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.from_numpy(A.main_pass_positions(W, H)).to("cuda")
    rec = torch.empty((n, 16), dtype=torch.float64, device="cuda")
    rgb = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    assert rec.data_ptr() % 128 == 0

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    calls = {
        "render_depth1_ms": lambda: h_first.render_main_pass_dev(0, n, rgb.data_ptr(), linear=True, stream=stream),
        "render_full_depth_ms": lambda: h_chain.render_main_pass_dev(0, n, rgb.data_ptr(), linear=True, stream=stream),
    }
    if not args.yardstick_only:
        calls["first_hit_ms"] = lambda: h.surface_positions_dev(pos.data_ptr(), n, rec.data_ptr(), follow=False, stream=stream)
        calls["follow_ms"] = lambda: h.surface_positions_dev(pos.data_ptr(), n, rec.data_ptr(), follow=True, stream=stream)
    for _ in range(3):
        for c in calls.values():
            timed(c)
    t = {k: [] for k in calls}
    for _ in range(args.steps):
        for k, c in calls.items():
            t[k].append(timed(c))
    res = {"frame": f"wine_glass {W}x{H}, trace_depth {depth}, warm handles, device buffers, host clock between synchronisations",
           "steps": args.steps}
    for k, v in t.items():
        res[k] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / float(np.median(v))}
    if not args.yardstick_only:
        calls["follow_ms"]()
        torch.cuda.synchronize()
        hops = rec[:, 13]
        res["follow_mean_hops"] = float(hops.mean())
        res["follow_rays_with_hops"] = float((hops > 0).double().mean())
        res["follow_max_hops"] = int(hops.max())
        y = res["render_depth1_ms"]
        res["first_hit_over_render_depth1"] = res["first_hit_ms"]["median"] / y["median"]
        res["first_hit_below_yardstick_by_more_than_its_spread"] = bool(res["first_hit_ms"]["median"] < y["median"] * (1 - y["spread"]))
        res["mrays_per_s"] = {"first_hit": n / res["first_hit_ms"]["median"] / 1e3, "follow": n / res["follow_ms"]["median"] / 1e3}
    for x in (h, h_first, h_chain):
        x.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
