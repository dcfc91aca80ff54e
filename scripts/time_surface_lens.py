#!/usr/bin/env python3
"""What the lens surface records cost.

    python scripts/time_surface_lens.py [--steps 5] [--samples 16] [--width 1920 --height 1080] [--out profiles/r11/surface_lens_times.json]

Frame: wine_glass at p4 / d12, K lens rays per pixel (aperture 0.15, focus 12, jitter), FOLLOW.  In one process, after one warm-up of
each, alternating --steps times:
  surface_lens     acn_surface_lens_main_pass_dev( 0, n )                        rays, records and reduction, slice by slice
  positions_x_K    K times acn_surface_positions_dev of the frame                the tracing it cannot avoid (pinhole rays: the same
                                                                                 number of rays, without the K records per pixel)
  lens_stats       acn_render_lens_stats_main_pass_dev( 0, n, linear )           the render it guides
  reduce_slice     acn_surface_reduce_dev of one slice of records alone          the reduction kernel; times the slices of a frame
Everything runs on torch's current stream and ends in a synchronise; a host clock is taken around each.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    import numpy as np
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [round(x, 3) for x in v]}


def timed(f):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


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
    flat = A.Scene.build("wine_glass", image_width=w, image_height=hh, path_samples=4, direct_samples=12).flatten()
    h = A.Handle(flat)
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda")
    slice_rays = int(os.environ.get("ACN_LENS_SLICE_RAYS", 1 << 21))
    n_slice = min(n, max(slice_rays // K, 1))
    slices = -(-n // n_slice)
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(dev)
    d_surf = torch.empty((n, 16), dtype=torch.float64, device=dev)
    d_pin = torch.empty((n, 16), dtype=torch.float64, device=dev)
    d_stats = torch.empty((n, 8), dtype=torch.float64, device=dev)
    d_rays = torch.empty((n_slice * K, 6), dtype=torch.float64, device=dev)
    d_rec = torch.empty((n_slice, K, 16), dtype=torch.float64, device=dev)
    d_red = torch.empty((n_slice, 16), dtype=torch.float64, device=dev)
    lens_kw = dict(samples=K, aperture=0.15, focus=12.0, jitter=True)
    torch.cuda.synchronize()
    # the records of the first slice, for the reduction alone
    h.lens_rays_dev(d_pos.data_ptr(), n_slice, d_rays.data_ptr(), **lens_kw)
    h.surface_rays_dev(d_rays.data_ptr(), n_slice * K, d_rec.data_ptr(), follow=True)

    def positions_x_k():
        for _ in range(K):
            h.surface_positions_dev(d_pos.data_ptr(), n, d_pin.data_ptr(), follow=True, stream=stream)

    calls = {
        "surface_lens": lambda: h.surface_lens_main_pass_dev(0, n, d_surf.data_ptr(), follow=True, stream=stream, **lens_kw),
        "positions_x_K": positions_x_k,
        "lens_stats": lambda: h.render_lens_stats_main_pass_dev(0, n, None, d_stats.data_ptr(), linear=True, stream=stream, **lens_kw),
        "reduce_slice": lambda: h.surface_reduce_dev(d_rec.data_ptr(), n_slice, K, d_red.data_ptr(), stream=stream),
    }
    for f in calls.values():                                  # warm-up: code objects, lanes, learned rates, slice buffers
        timed(f)
    times = {name: [] for name in calls}
    for _ in range(args.steps):
        for name, f in calls.items():
            times[name].append(timed(f))
    same = bool(torch.equal(d_red, d_surf[:n_slice]))
    coverage = d_surf[:, 15]
    res = {"frame": f"wine_glass {w}x{hh} p4 d12", "samples": K, "steps": args.steps, "mode": "FOLLOW", "lens": lens_kw,
           "slices": slices, "positions_per_slice": n_slice}
    res.update({name + "_ms": stats(v) for name, v in times.items()})
    med = {name: float(np.median(v)) for name, v in times.items()}
    res.update({"surface_lens_over_positions_x_K": med["surface_lens"] / med["positions_x_K"],
                "surface_lens_over_lens_stats": med["surface_lens"] / med["lens_stats"],
                "reduce_of_a_frame_ms_estimate": med["reduce_slice"] * n / n_slice,
                "reduce_share_of_surface_lens": med["reduce_slice"] * n / n_slice / med["surface_lens"],
                "record_bytes_written_and_read_per_frame": 2 * 128 * K * n, "slice_buffer_bytes": 128 * K * n_slice,
                "first_slice_same_bits_as_reduce_alone": same,
                "pixels_of_coverage_below_1": int((coverage < 1).sum()), "pixels_of_coverage_below_0.75": int((coverage < 0.75).sum())})
    h.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
