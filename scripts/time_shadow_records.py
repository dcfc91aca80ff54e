#!/usr/bin/env python3
"""What a shadow record costs per shadow ray, beside the production direct-light path.

    python scripts/time_shadow_records.py [--width 1920 --height 1080] [--samples 16] [--batch 20] [--steps 5] [--out profiles/r24/shadow_records.json]

The first-hit surface records of the wine glass at that size; acn_shadow_records_dev with S = --samples on them, warmed up, then
--steps times --batch calls enqueued back to back on one stream between two device events: ms per call, and ns per asked ray (the
sum of [ 3 ] over the records: the shadow rays the call cast).
Beside it, in the same process at the same commit, the production path: a frame of the same scene and size with path_samples 0 and
direct_samples = --samples, linear, rendered --steps times with ACN_OPT_STAGE_TIMING; the shade stage's device time (k_shade_hits and
the k_shade family, summed over the lanes) and the hard-ray kernels' beside it, divided by the frame's shadow_ray work counter, which
a counted render of the same frame supplies (the counting kernels are not the timed ones).  The two are not the same work: a frame's
shading points include those behind glass and in mirrors, each draws ( uint64 )( 16 * diffuse_intensity ) samples, and k_shade
evaluates the Oren-Nayar term and the light's falloff for every clear sample; the shadow record writes 128 bytes per position and
nothing else.  No ratio is expected in advance.  Prints one JSON line."""
import argparse
import json
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A

    w, hh, S = args.width, args.height, args.samples
    n = w * hh
    flat = A.Scene.build("wine_glass", image_width=w, image_height=hh, path_samples=0, direct_samples=S).flatten()
    h = A.Handle(flat)
    dev = torch.device("cuda", h.device)
    f64 = dict(dtype=torch.float64, device=dev)
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(dev)
    d_surf, d_out = torch.empty((n, 16), **f64), torch.empty((n, 16), **f64)
    torch.cuda.synchronize()
    h.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: h.shadow_records_dev(d_surf.data_ptr(), n, d_out.data_ptr(), samples=S, stream=stream)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.batch):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / args.batch)
    rec = d_out.cpu().numpy()
    asked, clear, sampled = float(rec[:, 3].sum()), float(rec[:, 4].sum()), int((rec[:, 0] == 1).sum())
    stat = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [round(float(x), 4) for x in v]}
    res = {"scene": f"wine_glass {w}x{hh}, first-hit records", "samples": S, "batch": args.batch, "steps": args.steps, "positions": n,
           "sampled_records": sampled, "asked_rays": asked, "clear_rays": clear, "lights": int(rec[rec[:, 0] == 1, 2].max(initial=0)),
           "stage_info": {k: v for k, v in h.stage_info().items() if k in ("prune", "leaf_lights", "lds_nodes")},
           "shadow_records_ms_per_call": stat(ms), "shadow_records_ns_per_asked_ray": float(np.median(ms)) * 1e6 / asked}

    # the production direct-light path on the same scene: path_samples 0, direct_samples S
    d_lin = torch.empty((n, 3), **f64)
    torch.cuda.synchronize()
    h.render_main_pass_dev(0, n, d_lin.data_ptr(), linear=True)                  # warm-up: the handle learns its queue demand
    h.stage_timing = True
    shade, hard, walk, total = [], [], [], []
    for _ in range(args.steps):
        h.render_main_pass_dev(0, n, d_lin.data_ptr(), linear=True)
        st = h.last_stages()
        shade.append(st["shade_ms"]); hard.append(st["hard_ms"]); walk.append(st["walk_ms"]); total.append(st["total_ms"])
    h.stage_timing = False
    h.count_work = True
    h.render_main_pass_dev(0, n, d_lin.data_ptr(), linear=True)
    counters = h.last_counters()
    h.count_work = False
    h.close()
    rays = float(counters["shadow_rays"])
    res["frame"] = {"what": f"wine_glass {w}x{hh} path_samples 0 direct_samples {S}, linear main pass, stage timing", "shade_stage_ms": stat(shade),
                    "hard_ray_kernels_ms": stat(hard), "walk_ms": stat(walk), "total_ms": stat(total), "shadow_ray_counter": rays,
                    "cap_sample_counter": float(counters["cap_samples"]),
                    "shade_stage_ns_per_shadow_ray": float(np.median(shade)) * 1e6 / rays,
                    "shade_and_hard_ns_per_shadow_ray": (float(np.median(shade)) + float(np.median(hard))) * 1e6 / rays}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
