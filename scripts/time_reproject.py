#!/usr/bin/env python3
"""What the reprojection gather costs per byte beside the statistics merge.

    python scripts/time_reproject.py [--width 1920 --height 1080] [--steps 7] [--out profiles/r16/reproject_time.json]

n = width x height positions against a previous raster of the same size.  The records are synthetic: a plane of one object faces an
axis-aligned camera, the previous raster holds the surface points of its pixel centres with records of four samples, and the current
positions are those points moved half a pixel to the right and down, so that every position has four taps of weight 1 / 4, all valid
(those of the last column and row lose the taps off the image).  Per position the call asks for 128 bytes of its own record and
4 x 192 of the taps and writes 80 (record and motion): 976; the merge moves 192.  In one process, after a warm-up of each, alternating
--steps times between two synchronisations:
  reproject     acn_reproject_dev
  stats_merge   acn_lens_stats_merge_dev on the same n (the accumulator restored from a copy before every timed call, outside the clock)
Prints one JSON line: the times and the time per requested byte of both."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A
    from actinon_amd import abi

    w, hh = args.width, args.height
    n = w * hh
    h = A.Handle(A.Scene.build("wine_glass", image_width=64, image_height=36, path_samples=4, direct_samples=12).flatten())
    dev = torch.device("cuda", h.device)
    f64 = dict(dtype=torch.float64, device=dev)
    prm = abi.Params()
    prm.image_width, prm.image_height, prm.gamma = w, hh, 1.0
    prm.camera_view_direction[:] = (0.0, 1.0, 0.0)
    prm.camera_top_direction[:] = (0.0, 0.0, 1.0)
    prm.camera_focal_length = 1.0
    prm.trace_depth, prm.trace_min_intensity, prm.direct_samples, prm.path_samples, prm.max_path_length = 11, 0.01, 1, 1, 100.0
    half_h, half_w = float(hh >> 1), float(w >> 1)
    depth = half_h                                                            # s = 1 / depth: a step of 1 along x or z is one pixel

    def records(off):
        """the plane's points under the positions ( x + 0.5 + off, y + 0.5 + off )"""
        idx = torch.arange(n, device=dev)
        qx, qy = (idx % w).double() + 0.5 + off, (idx // w).double() + 0.5 + off
        r = torch.zeros((n, 16), **f64)
        r[:, 0] = depth
        r[:, 1], r[:, 2], r[:, 3] = qx - half_w, depth, half_h - qy
        r[:, 5] = -1.0
        r[:, 7], r[:, 8], r[:, 9:12], r[:, 12], r[:, 14] = 3.0, -1.0, 0.5, 2.0, 1.0
        return r

    g = torch.Generator(device=dev).manual_seed(1)
    prev_surf, cur = records(0.0), records(0.5)
    prev_stats = torch.rand((n, 8), generator=g, **f64)
    prev_stats[:, 0], prev_stats[:, 7] = 4.0, 0.0
    part = torch.rand((n, 8), generator=g, **f64)
    part[:, 0], part[:, 7] = 4.0, 0.0
    d_out, d_motion = torch.empty((n, 8), **f64), torch.empty((n, 2), **f64)
    d_acc = prev_stats.clone()
    stream = torch.cuda.current_stream().cuda_stream
    calls = {
        "reproject": lambda: h.reproject_dev(cur.data_ptr(), n, prm, prev_surf.data_ptr(), prev_stats.data_ptr(), d_out.data_ptr(), d_motion.data_ptr(), stream=stream),
        "stats_merge": lambda: h.lens_stats_merge_dev(d_acc.data_ptr(), n, part.data_ptr(), n, None, stream=stream),
    }

    def timed(f):
        d_acc.copy_(prev_stats)
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for f in calls.values():
        timed(f)
    times = {name: [] for name in calls}
    for _ in range(args.steps):
        for name, f in calls.items():
            times[name].append(timed(f))
    out, motion = d_out.cpu().numpy(), d_motion.cpu().numpy()
    h.close()
    inner = (np.arange(n) % w < w - 1) & (np.arange(n) // w < hh - 1)
    pos = A.main_pass_positions(w, hh)
    m = prev_stats[:, 1].cpu().numpy().reshape(hh, w)
    four = (m[:-1, :-1] + m[:-1, 1:] + m[1:, :-1] + m[1:, 1:]).reshape(-1) / 4.0      # the taps of the positions off the last column and row
    checks = {"with_history": float((out[:, 0] >= 1).mean()), "n_is_4": bool(np.allclose(out[:, 0], 4.0, rtol=1e-12)),
              "max_motion_error_px": float(np.abs(motion - (pos + 0.5)).max()),
              "inner_mean_is_the_four_taps": bool(np.allclose(out[inner, 1], four, rtol=1e-9))}
    med = {name: float(np.median(v)) for name, v in times.items()}
    bytes_asked = {"reproject": 976 * n, "stats_merge": 192 * n}
    ns_per_byte = {name: med[name] * 1e6 / bytes_asked[name] for name in bytes_asked}
    res = {"positions": n, "steps": args.steps,
           "ms": {name: {"median": med[name], "min": float(min(v)), "max": float(max(v)), "runs": [round(x, 4) for x in v]} for name, v in times.items()},
           "bytes_requested": bytes_asked, "ns_per_byte": ns_per_byte, "GB_per_s_requested": {name: bytes_asked[name] / (med[name] * 1e6) for name in bytes_asked},
           "reproject_over_merge_per_byte": ns_per_byte["reproject"] / ns_per_byte["stats_merge"], "margin": 1.5, "checks": checks}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
