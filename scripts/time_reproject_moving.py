#!/usr/bin/env python3
"""What the motion table costs the reprojection gather.

    python scripts/time_reproject_moving.py [--width 1920 --height 1080] [--steps 7] [--batch 20] [--out profiles/r18/reproject_moving.json]

n = width x height positions on rendered records: the first-hit surface records of the wine glass at that size, the previous frame at
the scene's camera, the current one a degree further on its orbit; the previous statistics are records of four samples.  In one process,
after a warm-up of each, alternating --steps times:
  reproject      acn_reproject_dev
  moving_rest    acn_reproject_moving_dev with a table whose rows are all REST
  moving_moved   acn_reproject_moving_dev with a table whose rows are all MOVED by the identity: the same taps, every row read whole
each timed two ways: one call between two synchronisations (what profiles/r16 reports for acn_reproject_dev), and --batch calls
enqueued back to back between two synchronisations, per call.  The three must give the same records (checked: all-REST bit for bit,
the identity up to the sign of a zero).  Bytes requested per position with four taps: 128 of its own record, 4 x 192 of the taps, 80
written: 976; the table adds 16 (state and cap) and, MOVED, 96 more.  Prints one JSON line."""
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
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes as C
    import numpy as np
    import torch
    import actinon_amd as A
    from actinon_amd import abi
    from actinon_amd.cameras import orbit_camera

    w, hh = args.width, args.height
    n = w * hh
    flat = A.Scene.build("wine_glass", image_width=w, image_height=hh).flatten()
    h = A.Handle(flat)
    dev = torch.device("cuda", h.device)
    f64 = dict(dtype=torch.float64, device=dev)
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(dev)
    prev_surf, cur = torch.empty((n, 16), **f64), torch.empty((n, 16), **f64)
    torch.cuda.synchronize()
    prm = abi.Params()
    C.memmove(C.addressof(prm), C.addressof(h.params), C.sizeof(abi.Params))
    h.surface_positions_dev(d_pos.data_ptr(), n, prev_surf.data_ptr())
    h.set_params(**orbit_camera(flat.params, 1.0))
    h.surface_positions_dev(d_pos.data_ptr(), n, cur.data_ptr())
    g = torch.Generator(device=dev).manual_seed(1)
    prev_stats = torch.rand((n, 8), generator=g, **f64)
    prev_stats[:, 0], prev_stats[:, 7] = 4.0, 0.0
    rows = int(flat.c.n_nodes)
    rest = np.zeros((rows, 16))
    moved = np.zeros((rows, 16))
    moved[:, [0, 4, 8]] = 1.0
    moved[:, 12] = abi.ACN_MOTION_MOVED
    d_rest, d_moved = torch.from_numpy(rest).to(dev), torch.from_numpy(moved).to(dev)
    outs = {name: (torch.empty((n, 8), **f64), torch.empty((n, 2), **f64)) for name in ("reproject", "moving_rest", "moving_moved")}
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda name, k: outs[name][k].data_ptr()
    calls = {
        "reproject": lambda: h.reproject_dev(cur.data_ptr(), n, prm, prev_surf.data_ptr(), prev_stats.data_ptr(), ptr("reproject", 0), ptr("reproject", 1), stream=stream),
        "moving_rest": lambda: h.reproject_moving_dev(cur.data_ptr(), n, prm, prev_surf.data_ptr(), prev_stats.data_ptr(), d_rest.data_ptr(), rows,
                                                      ptr("moving_rest", 0), ptr("moving_rest", 1), stream=stream),
        "moving_moved": lambda: h.reproject_moving_dev(cur.data_ptr(), n, prm, prev_surf.data_ptr(), prev_stats.data_ptr(), d_moved.data_ptr(), rows,
                                                       ptr("moving_moved", 0), ptr("moving_moved", 1), stream=stream),
    }

    def timed(f, count):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / count

    for f in calls.values():
        timed(f, 2)
    single = {name: [] for name in calls}
    batch = {name: [] for name in calls}
    for _ in range(args.steps):
        for name, f in calls.items():
            single[name].append(timed(f, 1))
        for name, f in calls.items():
            batch[name].append(timed(f, args.batch))
    got = {name: (o[0].cpu().numpy(), o[1].cpu().numpy()) for name, o in outs.items()}
    h.close()
    same = lambda a, b: bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
    took = got["reproject"][0][:, 0] >= 1
    checks = {"with_history": float(took.mean()), "hits": float(np.isfinite(cur[:, 0].cpu().numpy()).mean()), "table_rows": rows,
              "rest_equals_reproject_bitwise": same(got["moving_rest"][0], got["reproject"][0]) and same(got["moving_rest"][1], got["reproject"][1]),
              "identity_equals_reproject": bool(np.array_equal(got["moving_moved"][0], got["reproject"][0])
                                                and np.array_equal(got["moving_moved"][1], got["reproject"][1], equal_nan=True))}
    per_position = {"reproject": 976, "moving_rest": 976 + 16, "moving_moved": 976 + 16 + 96}
    stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [round(x, 4) for x in v]}
    res = {"positions": n, "steps": args.steps, "batch": args.batch, "scene": f"wine_glass {w}x{hh}, first-hit records, the camera a degree apart",
           "ms_single_call": {name: stat(v) for name, v in single.items()}, "ms_per_call_in_a_batch": {name: stat(v) for name, v in batch.items()},
           "bytes_requested_per_position_with_four_taps": per_position, "bytes_requested": {name: b * n for name, b in per_position.items()},
           "ns_per_requested_byte_in_a_batch": {name: float(np.median(batch[name])) * 1e6 / (per_position[name] * n) for name in calls},
           "checks": checks}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
