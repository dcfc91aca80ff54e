#!/usr/bin/env python3
"""What the history of the frames before is worth on an orbiting camera.

    python scripts/measure_reproject.py [--frames 8] [--degrees 1] [--samples 4] [--ref-samples 256] [--out profiles/r16/reproject_quality.json]

Frame: wine_glass as its script sets it (400 x 400, p500 / d200); the camera orbits --degrees per frame.  Every frame renders K =
--samples jittered samples per pixel with their statistics (seed = frame) and first-hit surface records; from frame 1 on
acn_reproject_dev fetches the history from the frame before and acn_lens_stats_merge_dev pools it with the frame's own samples, as
tools/render_turntable.py --temporal does.  For the LAST frame, against a converged frame of its camera (--ref-samples jittered
samples, seed 99, rendered in blocks of pixels), the linear RMSE over all pixels and over the pixels that took a history of
  raw          the frame's own K samples
  accumulated  history + own samples
  raw_denoised, accumulated_denoised   either through acn_denoise_stats_dev
and per frame the share of pixels that took a history and the mean n after the merge.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--degrees", type=float, default=1.0)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--ref-samples", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A
    from actinon_amd import abi
    from actinon_amd.cameras import orbit_camera

    flat = A.Scene.build("wine_glass").flatten()
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n, K = w * hh, args.samples
    h = A.Handle(flat)
    f64 = dict(dtype=torch.float64, device=torch.device("cuda", h.device))
    new = lambda *shape: torch.zeros(shape, **f64)
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(f64["device"])
    d_surf, d_prev_surf, d_cur, d_acc, d_prev = new(n, 16), new(n, 16), new(n, 8), new(n, 8), new(n, 8)
    d_a, d_b = new(n, 3), new(n, 3)
    torch.cuda.synchronize()
    prev_params, per_frame = None, []
    for f in range(args.frames):
        if f:
            h.set_params(**orbit_camera(flat.params, args.degrees * f))
        h.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr())
        h.render_lens_stats_main_pass_dev(0, n, None, d_cur.data_ptr(), linear=True, samples=K, jitter=True, seed=f)
        took = torch.zeros(n, dtype=torch.bool, device=f64["device"])
        if f:
            h.reproject_dev(d_surf.data_ptr(), n, prev_params, d_prev_surf.data_ptr(), d_prev.data_ptr(), d_acc.data_ptr())
            took = d_acc[:, 0] >= 1
            h.lens_stats_merge_dev(d_acc.data_ptr(), n, d_cur.data_ptr(), n)
        else:
            d_acc.copy_(d_cur)
            torch.cuda.synchronize()
        per_frame.append({"frame": f, "with_history": float(took.double().mean()), "mean_n": float(d_acc[:, 0].mean())})
        print(per_frame[-1], file=sys.stderr, flush=True)
        prev_params = abi.Params()
        C.memmove(C.addressof(prev_params), C.addressof(h.params), C.sizeof(abi.Params))
        if f < args.frames - 1:
            d_surf, d_prev_surf = d_prev_surf, d_surf
            d_acc, d_prev = d_prev, d_acc
    h.denoise_stats_dev(d_cur.data_ptr(), d_surf.data_ptr(), w, hh, d_a.data_ptr())
    h.denoise_stats_dev(d_acc.data_ptr(), d_surf.data_ptr(), w, hh, d_b.data_ptr())
    frames = {"raw": d_cur[:, 1:4].cpu().numpy(), "accumulated": d_acc[:, 1:4].cpu().numpy(), "raw_denoised": d_a.cpu().numpy(),
              "accumulated_denoised": d_b.cpu().numpy()}
    took = took.cpu().numpy()
    kinds = d_surf[:, 12].cpu().numpy().astype(np.int64)
    hit = np.isfinite(d_surf[:, 0].cpu().numpy())
    eligible = hit & ((kinds & abi.ACN_REPROJECT_DEFAULT_REJECT_KINDS) == 0)
    res = {"scene": f"wine_glass {w}x{hh} p{flat.params.path_samples} d{flat.params.direct_samples}", "frames": args.frames, "degrees_per_frame": args.degrees,
           "samples": K, "ref_samples": args.ref_samples, "pixels": n, "eligible_last_frame": int(eligible.sum()),
           "with_history_of_eligible_last_frame": float(took[eligible].mean()), "per_frame": per_frame, "learning_passes": h.info()["learning_passes"]}
    if args.ref_samples:
        ref = np.empty((n, 3))
        block = 16384
        d_ref = torch.empty((block, 3), **f64)
        for first in range(0, n, block):
            cnt = min(block, n - first)
            h.render_lens_main_pass_dev(first, cnt, d_ref.data_ptr(), linear=True, samples=args.ref_samples, jitter=True, seed=99)
            ref[first:first + cnt] = d_ref[:cnt].cpu().numpy()
            print(f"reference: {first + cnt} of {n} pixels", file=sys.stderr, flush=True)
        for label, mask in (("all", np.ones(n, bool)), ("with_history", took)):
            for name, img in frames.items():
                d = img[mask] - ref[mask]
                res.setdefault("rmse_linear", {}).setdefault(label, {})[name] = float(np.sqrt(np.mean(d * d)))
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
