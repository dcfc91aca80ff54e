#!/usr/bin/env python3
"""Time of a depth-of-field frame: the one call against the recipe it replaces.

    python scripts/time_lens.py [--steps 5] [--samples 16] [--width 1920 --height 1080] [--out profiles/r06/lens_times.json]

Frame: wine_glass at p4 / d12, K lens rays per pixel, aperture 0.15 focused at 12.
  call    acn_render_lens_main_pass_dev( 0, n, lens, linear ) + acn_resolve_dev.
  recipe  INTEGRATION.md section 3b, "other lenses", built from calls that need no lens entry point: acn_camera_rays_dev once,
          then per sample k torch makes the lens rays of the whole frame (one lens offset per sample), acn_render_rays_dev
          renders them linear, torch accumulates; acn_resolve_dev at the end.  It keeps a frame of rays and a frame of radiance.
Both run on torch's current stream and end in a synchronise; a host clock is taken around each.  After one warm-up of each the
two alternate --steps times in one process.  Prints one JSON line (and writes it to --out)."""
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A

    w, hh, K = args.width, args.height, args.samples
    n = w * hh
    aperture, focus = 0.15, 12.0
    flat = A.Scene.build("wine_glass", image_width=w, image_height=hh, path_samples=4, direct_samples=12).flatten()
    prm = flat.params
    h = A.Handle(flat)
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda")
    view = torch.tensor(prm.camera_view_direction[:], dtype=torch.float64, device=dev)
    view = view / view.norm()
    top = torch.tensor(prm.camera_top_direction[:], dtype=torch.float64, device=dev)
    top = top - (top @ view) * view
    top = top / top.norm()
    right = torch.linalg.cross(view, top)
    rng = np.random.default_rng(1)
    offsets = []
    while len(offsets) < K:                                   # K points of the unit disc
        u, v = rng.uniform(-1, 1, 2)
        if u * u + v * v <= 1:
            offsets.append((u, v))
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(dev)
    d_pin = torch.empty((n, 6), dtype=torch.float64, device=dev)
    d_lens = torch.empty((n, 6), dtype=torch.float64, device=dev)
    d_lin = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_sum = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    d_call = torch.empty((n, 3), dtype=torch.float64, device=dev)
    retries = {"call": 0, "recipe": 0}

    def call():
        h.render_lens_main_pass_dev(0, n, d_call.data_ptr(), linear=True, stream=stream, samples=K, aperture=aperture, focus=focus)
        retries["call"] += int(h.last_stages()["retries"])
        h.resolve_dev(d_call.data_ptr(), n, None, d_rgb8.data_ptr(), stream=stream)

    def recipe():
        h.camera_rays_dev(d_pos.data_ptr(), n, d_pin.data_ptr(), stream=stream)
        o, d = d_pin[:, :3], d_pin[:, 3:]
        target = o + d * (focus / (d @ view))[:, None]
        d_sum.zero_()
        for u, v in offsets:
            d_lens[:, :3] = o + aperture * (u * right + v * top)
            d_lens[:, 3:] = target - d_lens[:, :3]
            h.render_rays_dev(d_lens.data_ptr(), n, d_lin.data_ptr(), linear=True, stream=stream)
            retries["recipe"] += int(h.last_stages()["retries"])
            d_sum.add_(d_lin, alpha=1.0 / K)
        h.resolve_dev(d_sum.data_ptr(), n, None, d_rgb8.data_ptr(), stream=stream)

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    timed(call), timed(recipe)                                # warm-up: code objects, lanes, learned rates, slice buffers
    times = {"call": [], "recipe": []}
    for _ in range(args.steps):
        times["call"].append(timed(call))
        times["recipe"].append(timed(recipe))
    # the two frames show the same picture (other lens samples: they differ by noise, not by more)
    diff = float((d_call - d_sum).abs().mean())
    level = float(d_sum.abs().mean())
    h.close()
    stats = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [round(x, 2) for x in v]}
    res = {"frame": f"wine_glass {w}x{hh} p4 d12", "samples": K, "aperture": aperture, "focus": focus, "steps": args.steps,
           "call_ms": stats(times["call"]), "recipe_ms": stats(times["recipe"]),
           "call_over_recipe": float(np.median(times["call"]) / np.median(times["recipe"])),
           "retries": retries, "mean_abs_difference_of_the_frames": diff, "mean_abs_radiance": level,
           "slice_buffer_bytes": 72 * K * min(n, max((1 << 21) // K, 1)), "recipe_buffer_bytes": 72 * n}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
