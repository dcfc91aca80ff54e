#!/usr/bin/env python3
"""What the layered lens records are worth and what they cost.

    python scripts/measure_lens_layers.py [--samples 16] [--ref-samples 1024] [--steps 3] [--out profiles/r12/lens_layers.json]

Frame: wine_glass as its script sets it (400 x 400, p500 / d200) through the lens of tools/render_dof.py -- aperture 0.15, focus 12,
jitter -- K = --samples rays per pixel, seed 0, FOLLOW records.  The calls are those of the tool with and without --layers:
  (a) raw     the mean of acn_render_lens_stats_main_pass_dev
  (b) stats   acn_denoise_stats_dev of those statistics, guided by acn_surface_lens_main_pass_dev
  (c) layers  acn_render_lens_layers_main_pass_dev -> acn_denoise_layers_dev
The converged picture is acn_render_lens_main_pass_dev of the same lens with --ref-samples rays per pixel and seed 9, unfiltered, rendered
in blocks of pixels (0: no reference, times only).  RMSE, linear and after cl_s_sat, over the pixels whose plane-0 coverage is below
0.9 and over all pixels.  Times: after one warm-up of each call, --steps runs under a host clock between two synchronisations, the
filters seven; split_slice is acn_lens_layers_reduce_dev alone on the first 131 072 pixels' worth of records.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LENS = dict(aperture=0.15, focus=12.0, jitter=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--ref-samples", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A

    flat = A.Scene.build("wine_glass").flatten()
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n, K = w * hh, args.samples
    h = A.Handle(flat)
    f64 = dict(dtype=torch.float64, device=torch.device("cuda", h.device))
    d_stats, d_surf1 = torch.empty((n, 8), **f64), torch.empty((n, 16), **f64)
    d_lstats, d_lsurf = torch.empty((3, n, 8), **f64), torch.empty((2, n, 16), **f64)
    d_b, d_c = torch.empty((n, 3), **f64), torch.empty((n, 3), **f64)
    lens = dict(LENS, samples=K, seed=0)

    def timed(fn, reps):
        fn()                                                                  # warm-up
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "runs": [round(x, 3) for x in ms]}

    # one slice of records and radiances for the split alone
    m = min(n, 131072)
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)[:m].copy()).to(f64["device"])
    d_rays, d_rec, d_rad = torch.empty((m * K, 6), **f64), torch.empty((m * K, 16), **f64), torch.empty((m * K, 3), **f64)
    d_ssurf, d_sstats = torch.empty((2, m, 16), **f64), torch.empty((3, m, 8), **f64)
    torch.cuda.synchronize()
    h.lens_rays_dev(d_pos.data_ptr(), m, d_rays.data_ptr(), **lens)
    h.surface_rays_dev(d_rays.data_ptr(), m * K, d_rec.data_ptr(), follow=True)
    h.render_rays_dev(d_rays.data_ptr(), m * K, d_rad.data_ptr(), linear=True)

    ms = {
        "render_lens_stats": timed(lambda: h.render_lens_stats_main_pass_dev(0, n, None, d_stats.data_ptr(), **lens), args.steps),
        "surface_lens": timed(lambda: h.surface_lens_main_pass_dev(0, n, d_surf1.data_ptr(), follow=True, **lens), args.steps),
        "denoise_stats": timed(lambda: h.denoise_stats_dev(d_stats.data_ptr(), d_surf1.data_ptr(), w, hh, d_b.data_ptr()), 7),
        "render_lens_layers": timed(lambda: h.render_lens_layers_main_pass_dev(0, n, None, d_lsurf.data_ptr(), d_lstats.data_ptr(), follow=True, **lens), args.steps),
        "denoise_layers": timed(lambda: h.denoise_layers_dev(d_lstats.data_ptr(), d_lsurf.data_ptr(), w, hh, d_c.data_ptr()), 7),
        "split_slice": timed(lambda: h.lens_layers_reduce_dev(d_rec.data_ptr(), d_rad.data_ptr(), m, K, d_ssurf.data_ptr(), d_sstats.data_ptr()), 7),
    }
    assert torch.equal(d_lsurf[0], d_surf1) and torch.equal(d_ssurf[0], d_surf1[:m]) and torch.equal(d_sstats, d_lstats[:, :m])
    cover = d_lsurf[0, :, 15].cpu().numpy()
    lst = d_lstats.cpu().numpy()
    res = {"scene": f"wine_glass {w}x{hh} p{flat.params.path_samples} d{flat.params.direct_samples}", "samples": K, "ref_samples": args.ref_samples,
           "lens": LENS, "pixels": n, "coverage_below_0.9": int((cover < 0.9).sum()), "pixels_with_layer_1": int((lst[1][:, 0] > 0).sum()),
           "pixels_with_rest": int((lst[2][:, 0] > 0).sum()), "split_slice_positions": m, "ms": ms}
    if args.ref_samples:
        ref = np.empty((n, 3))
        block = 16384
        d_ref = torch.empty((block, 3), **f64)
        for first in range(0, n, block):
            cnt = min(block, n - first)
            h.render_lens_main_pass_dev(first, cnt, d_ref.data_ptr(), linear=True, samples=args.ref_samples, seed=9, **LENS)
            ref[first:first + cnt] = d_ref[:cnt].cpu().numpy()
            print(f"reference: {first + cnt} of {n} pixels", file=sys.stderr, flush=True)
        gamma = float(flat.params.gamma)

        def sat(x):                                                           # cl_s_sat
            with np.errstate(invalid="ignore"):
                return np.clip(np.power(np.maximum(x, 0.0), gamma), 0.0, 1.0)

        frames = {"a_raw": d_stats[:, 1:4].cpu().numpy(), "b_denoise_stats": d_b.cpu().numpy(), "c_denoise_layers": d_c.cpu().numpy()}
        for label, mask in (("coverage_below_0.9", cover < 0.9), ("all", np.ones(n, bool))):
            for name, img in frames.items():
                for kind, f in (("linear", lambda x: x), ("saturated", sat)):
                    d = f(img[mask]) - f(ref[mask])
                    res.setdefault("rmse_" + kind, {}).setdefault(label, {})[name] = float(np.sqrt(np.mean(d * d)))
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
